"""Times the variance-guided denoiser and the render cost of the moments plane.

  python tools/time_denoise_variance.py [--runs N] [--reps N]

1. rm_denoise_variance_device at 3840 x 2160 with device events, L = 1, 3 (its default) and 5, both G-buffer formats, next to rm_denoise_device on
   the same planes: `runs` runs of `reps` calls each; prints the min / median / max of the per-call time over the runs.
2. The headline frame (C3b: Mandelbulb 3840 x 2160, full mode, 256 steps, one light, fast build) with rm_render_timed, with and
   without the moments plane, as the library renders it by default (samples in flight, staged either way) and under
   RM_RENDER_NO_OVERLAP (staged with moments, unstaged without): ms per sample, min / median / max over the runs.
The planes of part 1 are random (smooth colour, half sky, some variance): the filter's cost does not depend on the values."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(xs[len(xs) // 2], 4), "max": round(xs[-1], 4)}


def time_filters(ctx, args):
    import torch

    W, H, k = args.width, args.height, 4
    rng = np.random.default_rng(0)
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = -k
    a = np.full((H, W, 4), 0.5 * k, np.float32)
    a[..., 3] = rng.uniform(1.0, 10.0, (H, W)) * k
    a[: H // 2, :, 3] = np.inf
    M = np.empty((H, W, 2), np.float32)
    M[..., 0] = k * 0.5
    M[..., 1] = k * (0.25 + rng.uniform(0.0, 0.2, (H, W)))
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream(device=0)
    for gbuffer in ("f32", "f16"):
        fb = ctx.create_framebuffer(W, H, gbuffer=gbuffer, moments=True)
        fb.upload(0, c)
        fb.upload(1, n)
        fb.upload(2, a)
        fb.upload_raw(3, M)
        for L in (1, 3, 5):
            for mode, call in (("variance", ctx.denoise_variance_device), ("atrous", ctx.denoise_device)):
                p = {"iterations": L}
                runs = []
                with torch.cuda.stream(stream):
                    for _ in range(3):  # warm-up (and the context's buffers grown)
                        call(fb, k, out.data_ptr(), p, stream.cuda_stream)
                    for _ in range(args.runs):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(args.reps):
                            call(fb, k, out.data_ptr(), p, stream.cuda_stream)
                        e1.record(stream)
                        e1.synchronize()
                        runs.append(e0.elapsed_time(e1) / args.reps)
                r = {"what": "denoise", "mode": mode, "gbuffer": gbuffer, "iterations": L, "width": W, "height": H, "runs": args.runs,
                     "reps": args.reps, "ms": spread(runs)}
                print(json.dumps(r), flush=True)
        fb.destroy()


def time_moments_render(ctx, args):
    import golden_cases as GC
    from raymarching_engine_amd import abi, job as J, scene as S

    sc = S.Mandelbulb()
    schema = J.make_schema(sc, 3840, 2160, counts=(256,), render_mode="full", position=(0, 0, -2.5), lights=GC.LIGHT)
    u = J.uniforms_from_schema(schema, (0.5, 0.5))
    h = ctx.create_scene(sc)
    fbs = {m: ctx.create_framebuffer(3840, 2160, moments=m) for m in (False, True)}
    for extra, label in ((0, "default"), (abi.RM_RENDER_NO_OVERLAP, "no_overlap")):
        flags = abi.RM_RENDER_FAST | extra
        for fb in fbs.values():
            ctx.render_timed(h, fb, u, 2, None, flags)  # the job's cost order settles
        runs = {False: [], True: []}
        for _ in range(args.runs):  # interleaved, so that a drift of the clock hits both alike
            for m, fb in fbs.items():
                runs[m].append(ctx.render_timed(h, fb, u, args.samples, None, flags))
        r = {"what": "render C3b", "flags": label, "samples": args.samples, "runs": args.runs, "ms_without": spread(runs[False]),
             "ms_with_moments": spread(runs[True]),
             "overhead_median": round(sorted(runs[True])[args.runs // 2] / sorted(runs[False])[args.runs // 2] - 1.0, 4)}
        print(json.dumps(r), flush=True)
    for fb in fbs.values():
        fb.destroy()
    h.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--samples", type=int, default=8, help="samples per rm_render_timed call of part 2")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    from raymarching_engine_amd import native

    ctx = native.Context(0)
    time_filters(ctx, args)
    time_moments_render(ctx, args)
    ctx.close()


if __name__ == "__main__":
    main()
