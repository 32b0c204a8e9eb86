"""Times rm_denoise_device at 3840 x 2160 with device events: L = 1 and 5, both G-buffer formats; prints ms per call and per pass.

  python tools/time_denoise.py [--reps N]

The planes are random (smooth colour, half sky): the filter's cost does not depend on the values."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    import torch

    from raymarching_engine_amd import native

    W, H, k = args.width, args.height, 4
    ctx = native.Context(0)
    rng = np.random.default_rng(0)
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = -k
    a = np.full((H, W, 4), 0.5 * k, np.float32)
    a[..., 3] = rng.uniform(1.0, 10.0, (H, W)) * k
    a[: H // 2, :, 3] = np.inf
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream(device=0)
    results = []
    for gbuffer in ("f32", "f16"):
        fb = ctx.create_framebuffer(W, H, gbuffer=gbuffer)
        fb.upload(0, c)
        fb.upload(1, n)
        fb.upload(2, a)
        for L in (1, 5):
            p = {"iterations": L}
            with torch.cuda.stream(stream):
                for _ in range(3):  # warm-up (and the context's buffers grown)
                    ctx.denoise_device(fb, k, out.data_ptr(), p, stream.cuda_stream)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.reps):
                    ctx.denoise_device(fb, k, out.data_ptr(), p, stream.cuda_stream)
                e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            r = {"gbuffer": gbuffer, "iterations": L, "width": W, "height": H, "ms": round(ms, 4), "ms_per_pass": round(ms / L, 4)}
            results.append(r)
            print(json.dumps(r), flush=True)
        fb.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
