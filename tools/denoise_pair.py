"""Writes a raw / denoised PNG pair of a low-sample frame: the Mandelbulb of the denoiser's quality test (256 x 256, full mode,
one point light, fast build), 4 samples by default.

  python tools/denoise_pair.py OUT_DIR [--samples N] [--gbuffer f32|f16]

OUT_DIR/denoise_mandelbulb_<N>spp_raw.png is Framebuffer.present(N); ..._denoised.png is present(N, denoise=True)."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--gbuffer", default="f32", choices=("f32", "f16"))
    args = ap.parse_args()
    from raymarching_engine_amd import abi, capture, job as J, native, scene as S

    os.makedirs(args.out_dir, exist_ok=True)
    sc = S.Mandelbulb()
    schema = J.make_schema(sc, 256, 256, counts=(64, 16), render_mode="full", position=(0, 0, -2.5), lights=[J.point_light((2.0, 3.0, -4.0))])
    ctx = native.Context(0)
    h = ctx.create_scene(sc)
    fb = ctx.create_framebuffer(256, 256, gbuffer=args.gbuffer)
    J.reset_halton()
    noise = np.array([J.next_rand_noise() for _ in range(args.samples)], np.float32)
    ctx.render_samples(h, fb, J.uniforms_from_schema(schema, (0.5, 0.5)), noise, None, abi.RM_RENDER_FAST)
    stem = os.path.join(args.out_dir, f"denoise_mandelbulb_{args.samples}spp")
    capture.save_png(fb, args.samples, stem + "_raw.png")
    capture.save_png(fb, args.samples, stem + "_denoised.png", denoise=True)
    print(stem + "_raw.png", stem + "_denoised.png")
    fb.destroy()
    h.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
