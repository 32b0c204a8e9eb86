"""Times the firefly filter next to a device-to-device copy of the same plane.

  python tools/time_despeckle.py [--runs N] [--reps N] [--width W] [--height H]

rm_filter_device at 3840 x 2160 with device events on the context's stream (a torch stream handed to rm_ctx_set_stream): the
despeckle stage alone for radius 1 / 2 x rank 0 / 1 / 3 (radius 2, rank 1 is the default), and the chain with both stages off,
which is the library's device-to-device copy of the colour plane (hipMemcpyAsync) -- the floor for a kernel that moves 16 B in
and 16 B out per pixel; torch's own copy kernel on the same stream is printed as a second floor.  `runs` runs of `reps` calls
each after a warm-up; prints the min / median / max of the per-call time over the runs and the bytes per second the median is.
The plane is noise with 1 % outliers and 0.5 % non-finite pixels, so the clamp and the repair both run."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    import torch

    from raymarching_engine_amd import native

    W, H, k = args.width, args.height, 4
    rng = np.random.default_rng(0)
    c = (rng.exponential(size=(H, W, 4)) * 0.5 * k).astype(np.float32)
    c[rng.random((H, W)) < 0.01, :3] += 150.0
    c[rng.random((H, W)) < 0.005, 1] = np.nan
    ctx = native.Context(0)
    stream = torch.cuda.Stream(device=0)
    ctx.set_stream(stream.cuda_stream)
    fb = ctx.create_framebuffer(W, H)
    fb.upload(0, c)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    src = torch.empty_like(out)
    moved = 2 * 16 * W * H

    def timed(what, call, **extra):
        runs = []
        with torch.cuda.stream(stream):
            for _ in range(3):
                call()
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.reps):
                    call()
                e1.record(stream)
                e1.synchronize()
                runs.append(e0.elapsed_time(e1) / args.reps)
        ms = spread(runs)
        print(json.dumps({"what": what, **extra, "width": W, "height": H, "runs": args.runs, "reps": args.reps, "ms": ms,
                          "GB_per_s_median": round(moved / ms["median"] / 1e6, 1)}), flush=True)

    timed("copy (rm_filter_device, both stages off)", lambda: ctx.filter_device(fb, k, out.data_ptr()))
    timed("copy (torch copy_ on the same stream)", lambda: out.copy_(src))
    for radius in (2, 1):
        for rank in (1, 0, 3):
            p = {"radius": radius, "rank": rank}
            timed("despeckle", lambda: ctx.filter_device(fb, k, out.data_ptr(), despeckle=p), radius=radius, rank=rank)
    timed("copy (rm_filter_device, both stages off)", lambda: ctx.filter_device(fb, k, out.data_ptr()))
    changed = int((np.ascontiguousarray(fb.filter(k, despeckle=True)).view(np.uint32) != c.view(np.uint32)).any(-1).sum())
    print(json.dumps({"what": "pixels the default filter changed", "changed": changed, "of": W * H}))
    ctx.set_stream(None)
    fb.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
