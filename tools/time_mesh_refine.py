"""Times rm_mesh_refine and asks what it buys: the figures of profiles/mesh_refine.txt.

  python tools/time_mesh_refine.py [--n N] [--calls N] [--no-host-route] [--no-finer]
  python tools/time_mesh_refine.py --trace SCENE FLAGS      (one warmed three-round call, for a kernel trace made round it)
  python tools/time_mesh_refine.py --kernel-stats FILE.csv  (the refinement's rows of such a trace's kernel statistics)

Workloads: S.Mandelbulb() on n^3 cells (default 256) of [-1.25, 1.25]^3 at iso 2^-7, and the csg64 golden scene on n^3 cells of [-2, 2]^3 at iso
0, both without normals, in the strict and in the fast build.  The mesh is extracted, projected at the defaults (reach = half a cell) and then
refined for 1, 2 and 3 rounds with the host's default tolerance (1/64 of a cell) and the same projection inside the rounds.  Per setting: one
warming call, then `calls` calls with a report; median (min .. max) of rm_mesh_timings' two slots of the result (the library's events on the
context's stream: the split rounds; the projections -- and the normals, of which there are none here) and of the whole call on the host's clock,
rm_mesh_destroy of the result included.  Then rm_mesh_deviation at order 4 of each result.
The host route of one round, on entry points that exist without the entry: both arrays downloaded, tests/mesh_refine_ref.py (numpy, and a Python
loop over the triangles) with rm_probe for the distances and the normals.  Its result is compared with the entry's, bit for bit.
The finer grid: the same scene on (2 n)^3 cells through rm_mesh_extract_slabs, unrefined, with and without the projection -- extraction on the
host's clock, and the same deviation."""
import argparse
import csv
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def spread(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:.3f} ({xs[0]:.3f} .. {xs[-1]:.3f})"


def kernel_stats(path):
    """the rows of a kernel-statistics table whose kernels the refinement launches, as the table names its columns"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        print("no rows in", path)
        return
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    keep = ("rm_mesh_refine", "rm_mesh_project", "rm_mesh_scan", "rm_mesh_measure_sum", "rm_probe")
    print("columns:", ", ".join(rows[0].keys()))
    for row in rows:
        if any(k in row[name] for k in keep):
            short = row[name].split("(")[0][-96:]
            print("  " + short + ": " + ", ".join(f"{k} {v}" for k, v in row.items() if k != name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--no-finer", action="store_true")
    ap.add_argument("--trace", nargs=2, metavar=("SCENE", "FLAGS"))
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)

    import golden_cases as GC
    import mesh_refine_ref as RR
    from raymarching_engine_amd import abi, mesh as M, native, scene as S

    ctx = native.Context(0)
    lib = ctx.lib
    workloads = {"mandelbulb": (lambda: S.Mandelbulb(), (-1.25,) * 3, (1.25,) * 3, 2.0 ** -7), "csg64": (lambda: GC.build_scene("csg64"), (-2.0,) * 3, (2.0,) * 3, 0.0)}
    arithmetic = {"strict": 0, "fast": abi.RM_RENDER_FAST}

    def counts(h):
        out = (C.c_ulonglong * 2)()
        lib.rm_mesh_counts(h, out)
        return int(out[0]), int(out[1])

    def deviation(h, scene, iso, flags):
        report = abi.RmMeshDeviationReport()
        block = M.mesh_deviation(iso=iso, flags=flags)
        ctx._check(lib.rm_mesh_deviation(h, scene.h, C.byref(block), C.byref(report), None, None))
        return f"T {report.triangles}, order-4 rms {report.rms:.6g}, max {report.max:.6g}, mean_signed {report.mean_signed:.6g}, area {report.area:.6f}"

    def extract(scene, grid, iso, flags, slabs=False):
        h, g, p = C.c_void_p(), grid.to_c(), M.mesh_params(iso=iso, normals=False, flags=flags)
        if slabs:
            ctx._check(lib.rm_mesh_extract_slabs(ctx.h, scene.h, C.byref(g), C.byref(p), None, C.byref(h)))
        else:
            ctx._check(lib.rm_mesh_extract(ctx.h, scene.h, C.byref(g), C.byref(p), C.byref(h)))
        return h

    def projected(h, scene, block):
        out = C.c_void_p()
        ctx._check(lib.rm_mesh_project(h, scene.h, C.byref(block), C.byref(out), None, None))
        return out

    def refined(h, scene, block, inner, report=None):
        out = C.c_void_p()
        ctx._check(lib.rm_mesh_refine(h, scene.h, C.byref(block), C.byref(inner), C.byref(out), None if report is None else C.byref(report)))
        return out

    for name, (make, lo, hi, iso) in workloads.items():
        for which, flags in arithmetic.items():
            if args.trace and args.trace != [name, which]:
                continue
            scene = ctx.create_scene(make())
            grid = M.Grid(lo, hi, (args.n,) * 3)
            inner = M.mesh_project(iso=iso, reach=M.project_reach(grid), flags=flags)
            tolerance = M.refine_tolerance(grid)
            t0 = time.perf_counter()
            raw = extract(scene, grid, iso, flags)
            t1 = time.perf_counter()
            base = projected(raw, scene, inner)
            t2 = time.perf_counter()
            print(f"{name} {args.n}^3 iso {iso:g} {which}: {counts(base)[0]} vertices, {counts(base)[1]} triangles; extraction {1e3 * (t1 - t0):.1f} ms and projection {1e3 * (t2 - t1):.1f} ms on the host's clock (first calls)")
            print(f"  unrefined, unprojected: {deviation(raw, scene, iso, flags)}")
            print(f"  unrefined, projected:   {deviation(base, scene, iso, flags)}")
            if args.trace:
                block = M.mesh_refine(iso=iso, tolerance=tolerance, rounds=3, flags=flags)
                for _ in range(2):
                    lib.rm_mesh_destroy(refined(base, scene, block, inner))
                print("  traced: two three-round calls (one of them warming)")
            else:
                for rounds in (1, 2, 3):
                    block = M.mesh_refine(iso=iso, tolerance=tolerance, rounds=rounds, flags=flags)
                    lib.rm_mesh_destroy(refined(base, scene, block, inner))
                    split, project, whole, report = [], [], [], abi.RmMeshRefinement()
                    for call in range(args.calls):
                        t0 = time.perf_counter()
                        out = refined(base, scene, block, inner, report)
                        ms = (C.c_float * 3)()
                        lib.rm_mesh_timings(out, ms)
                        if call < args.calls - 1:
                            lib.rm_mesh_destroy(out)
                        whole.append(1e3 * (time.perf_counter() - t0))
                        split.append(ms[1])
                        project.append(ms[2])
                    r = abi.mesh_refinement_dict(report)
                    print(f"  {rounds} round(s), tolerance {tolerance:.6g}: split rounds {spread(split)} ms, projections {spread(project)} ms, whole call on the host's clock {spread(whole)} ms, median (min .. max) of {args.calls}")
                    print(f"    report: V {r['vertices']}, T {r['triangles']}, edges {r['edges'][:rounds]}, split {r['split_edges'][:rounds]}, nonfinite {r['nonfinite_midpoints'][:rounds]}, flipped {r['flipped_triangles']}, max_first {r['max_first']:.6g}, max_last {r['max_last']:.6g}, rounds_run {r['rounds_run']}, stopped {r['stopped']}")
                    print(f"    refined: {deviation(out, scene, iso, flags)}")
                    lib.rm_mesh_destroy(out)
                if not args.no_host_route and name == "mandelbulb":
                    block = M.mesh_refine(iso=iso, tolerance=tolerance, rounds=1, flags=flags)
                    v, t = counts(base)
                    t0 = time.perf_counter()
                    positions, triangles = np.empty((v, 3), np.float32), np.empty((t, 3), np.uint32)
                    lib.rm_mesh_download(base, abi.RM_MESH_POSITIONS, positions.ctypes.data_as(C.c_void_p), positions.nbytes)
                    lib.rm_mesh_download(base, abi.RM_MESH_TRIANGLES, triangles.ctypes.data_as(C.c_void_p), triangles.nbytes)
                    probing = [0.0]

                    def probe(what, q, param=0.0):
                        p0 = time.perf_counter()
                        out = ctx.probe(scene, what, q, param=param, flags=flags)
                        probing[0] += time.perf_counter() - p0
                        return out
                    want = RR.refine(positions, triangles, lambda q: probe(abi.RM_PROBE_SDF, q), iso=iso, tolerance=tolerance, rounds=1,
                                     project=dict(sdf=lambda q: probe(abi.RM_PROBE_SDF, q), normal=lambda q: probe(abi.RM_PROBE_NORMAL, q, inner.normal_delta), iso=iso,
                                                  rounds=inner.rounds, relax=inner.relax, tolerance=inner.tolerance, reach=inner.reach))
                    spent = time.perf_counter() - t0
                    out = refined(base, scene, block, inner)
                    got_p, got_t = np.empty((counts(out)[0], 3), np.float32), np.empty((counts(out)[1], 3), np.uint32)
                    lib.rm_mesh_download(out, abi.RM_MESH_POSITIONS, got_p.ctypes.data_as(C.c_void_p), got_p.nbytes)
                    lib.rm_mesh_download(out, abi.RM_MESH_TRIANGLES, got_t.ctypes.data_as(C.c_void_p), got_t.nbytes)
                    lib.rm_mesh_destroy(out)
                    equal = got_p.tobytes() == want["positions"].tobytes() and got_t.tobytes() == want["triangles"].tobytes()
                    print(f"  1 round through download + numpy restatement + rm_probe: {1e3 * spent:.0f} ms on the host's clock (one run), of which the rm_probe calls {1e3 * probing[0]:.1f} ms; arrays equal to the entry's bit for bit: {equal}")
                if not args.no_finer:
                    fine = M.Grid(lo, hi, (2 * args.n,) * 3)
                    lib.rm_mesh_destroy(extract(scene, fine, iso, flags, slabs=True))
                    t0 = time.perf_counter()
                    h = extract(scene, fine, iso, flags, slabs=True)
                    t1 = time.perf_counter()
                    finer_inner = M.mesh_project(iso=iso, reach=M.project_reach(fine), flags=flags)
                    lib.rm_mesh_destroy(projected(h, scene, finer_inner))
                    t2 = time.perf_counter()
                    moved = projected(h, scene, finer_inner)
                    t3 = time.perf_counter()
                    print(f"  {2 * args.n}^3 through slabs, unrefined: {counts(h)[0]} vertices; extraction {1e3 * (t1 - t0):.1f} ms, projection {1e3 * (t3 - t2):.1f} ms on the host's clock (second calls)")
                    print(f"    unprojected: {deviation(h, scene, iso, flags)}")
                    print(f"    projected:   {deviation(moved, scene, iso, flags)}")
                    lib.rm_mesh_destroy(moved)
                    lib.rm_mesh_destroy(h)
                    # the coarse chain again, warm, for the same clock
                    t0 = time.perf_counter()
                    raw2 = extract(scene, grid, iso, flags)
                    base2 = projected(raw2, scene, inner)
                    t1 = time.perf_counter()
                    print(f"  {args.n}^3 extraction + projection, warm: {1e3 * (t1 - t0):.1f} ms on the host's clock")
                    lib.rm_mesh_destroy(base2)
                    lib.rm_mesh_destroy(raw2)
            lib.rm_mesh_destroy(base)
            lib.rm_mesh_destroy(raw)
            scene.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
