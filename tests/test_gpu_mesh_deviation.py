"""Deviation on the GPU: rm_mesh_deviation against the numpy restatement (tests/mesh_deviation_ref.py) fed with rm_probe(RM_PROBE_SDF) on the same
context and flags.  Every comparison of floats is of their bits; the one inequality is a bound derived from the sphere's geometry."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_deviation_ref as DR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import SAMPLE_HI, SAMPLE_LO, table_with_surfaces
from test_gpu_mesh_parts import FIELDS, arrays, counts, filtered, from_scene, from_values, one_cell, same_arrays
from test_gpu_mesh_project import project, slabbed
from test_gpu_mesh_quadric import placed
from test_gpu_mesh_simplify import simplified

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID
FAST, NO_CULL = abi.RM_RENDER_FAST, abi.RM_RENDER_NO_CULL
GUARD = F(-7.0)
CAMEL = dict(vertices="vertices", triangles="triangles", skipped_triangles="skippedTriangles", unevaluated_triangles="unevaluatedTriangles",
             nonfinite_samples="nonfiniteSamples", over_triangles="overTriangles", worst_triangle="worstTriangle", area="area", over_area="overArea",
             mean_signed="meanSigned", rms="rms", max="max", samples="samples")


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gl_ctx():
    c = native.Context(0)
    c.set_gl_stack(True)
    yield c
    c.close()


def deviation(c, h, scene, block=None, ms=None):
    """rm_mesh_deviation of the handle: (the report's dict, the report's bytes, the T floats from inside a guard pattern that has to survive)"""
    _, t = counts(c, h)
    report, room = abi.RmMeshDeviationReport(), np.full(t + 16, GUARD, F)
    at = room[8:]  # (a view: the call writes behind eight guard floats)
    p = None if block is None else C.byref(block)
    assert c.lib.rm_mesh_deviation(h, scene.h, p, C.byref(report), native._fp(at), ms) == OK, c.lib.rm_last_error(c.h)
    assert (room[:8] == GUARD).all() and (room[8 + t:] == GUARD).all() and list(report.reserved) == [0, 0, 0, 0]
    return abi.mesh_deviation_dict(report), bytes(report), room[8:8 + t].copy()


def packed(report: dict) -> bytes:
    """a report's dict as the struct's bytes"""
    return bytes(abi.RmMeshDeviationReport(**{k: (float(v) if k in DR.DOUBLE_FIELDS + ("max",) else int(v)) for k, v in report.items()}))


def restated(c, h, scene, block):
    """the restatement on the handle's downloaded arrays, with rm_probe of the block's flags for the distances"""
    v, t = counts(c, h)
    positions, triangles = np.empty((v, 3), F), np.empty((t, 3), np.uint32)
    assert c.lib.rm_mesh_download(h, abi.RM_MESH_POSITIONS, positions.ctypes.data_as(C.c_void_p), positions.nbytes) == OK
    assert c.lib.rm_mesh_download(h, abi.RM_MESH_TRIANGLES, triangles.ctypes.data_as(C.c_void_p), triangles.nbytes) == OK
    sdf = lambda q: c.probe(scene, abi.RM_PROBE_SDF, q, flags=block.flags)
    return DR.deviation(positions, triangles, sdf, iso=block.iso, order=block.order, tolerance=block.tolerance)


def check(c, h, scene, **fields):
    """Every field of the report as bytes, and the per-triangle array by its bits.  Returns (report dict, array, the restatement)."""
    block = M.mesh_deviation(**fields)
    (report, raw, got), want = deviation(c, h, scene, block), restated(c, h, scene, block)
    assert got.dtype == want["triangles"].dtype == F and got.shape == want["triangles"].shape
    assert np.array_equal(got.view(np.uint32), want["triangles"].view(np.uint32)), (fields, int((got.view(np.uint32) != want["triangles"].view(np.uint32)).sum()), len(got))
    assert DR.same(report, want["report"]) == [], (fields, report, want["report"])
    assert raw == packed(want["report"]), fields
    return report, got, want


# ---- 1: bit for bit against the restatement ----------------------------------------------------------------------------------------------------

SCENES = [("sphere", lambda: S.single_sphere((0.125, -0.0625, 0.1875), 0.875), (0,)),
          ("kind rows", lambda: S.CsgScene().shape(S.Mandelbulb()).intersect().box((0.0, 0.0, 0.25), (1.25, 1.25, 0.75)), (0,)),
          ("csg64", lambda: S.csg64(), (0, NO_CULL)),  # 64 rows: the big-table path, with the culling grid and without
          ("mandelbulb", lambda: S.Mandelbulb(), (0,))]
GRIDS = [(7, 5, 3), (16, 16, 16), (33, 17, 9)]


def twelve_triangles(c):
    """a (2, 2, 2) grid whose middle corner alone is inside: eight vertices and the six quads round it, in the middle of the scenes.  T * S = 12
    at order 1 and 48 at order 2: launches below one wave"""
    v = np.ones((3, 3, 3), F)
    v[1, 1, 1] = -1.0
    h = from_values(c, (2, 2, 2), v, 0.0, (-0.75, -0.5, -0.625), (0.5, 0.75, 0.625))
    assert counts(c, h) == (8, 12)
    return h


@pytest.mark.parametrize("name, make, cull_flags", SCENES, ids=[s[0] for s in SCENES])
def test_deviation_is_the_restatement_bit_for_bit(ctx, gl_ctx, name, make, cull_flags):
    above = below = 0
    for which, c, arithmetic in (("strict", ctx, 0), ("fast", ctx, FAST), ("gl stack", gl_ctx, 0)):
        scene = c.create_scene(make())
        meshes = [twelve_triangles(c)]
        try:
            meshes += [from_scene(c, scene, M.Grid(SAMPLE_LO, SAMPLE_HI, n), flags=arithmetic, normals=False) for n in GRIDS]
            sizes = [counts(c, h)[1] for h in meshes]
            assert all(t > 0 for t in sizes), (name, which, sizes)
            assert any((t * n * n) % 256 for t in sizes for n in DR.ORDERS) and sizes[0] * 1 < 64 < sizes[-1]
            for h in meshes:
                for cull in cull_flags:
                    for n in DR.ORDERS:
                        report, _, want = check(c, h, scene, order=n, flags=arithmetic | cull)
                        assert report["samples"] == n * n and report["skipped_triangles"] == 0
                        above += int((want["mean"][want["evaluated"]] > 0).sum())
                        below += int((want["mean"][want["evaluated"]] < 0).sum())
        finally:
            for h in meshes:
                c.lib.rm_mesh_destroy(h)
            scene.destroy()
    assert below > 0 and (above > 0 or name == "sphere")  # (a condition on the inputs: every scene but the convex one has triangles on both sides)


def test_parameters_reach_the_kernel(ctx):
    scene = ctx.create_scene(table_with_surfaces())
    h = from_scene(ctx, scene, M.Grid((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), (24, 24, 24)), normals=False)
    try:
        base, array, want = check(ctx, h, scene)
        null_report, null_raw, null_array = deviation(ctx, h, scene, None)  # a NULL block: the defaults
        assert null_raw == packed(want["report"]) and null_array.tobytes() == array.tobytes() and base["samples"] == 16
        assert base["unevaluated_triangles"] == 0 and base["area"] > 0 and base["max"] > 0
        # tolerance 0: every evaluated triangle with max_t > 0 is over
        assert base["over_triangles"] == int((want["evaluated"] & (array > 0)).sum()) > 0 and 0 < base["over_area"] <= base["area"]
        # (flags: the Mandelbulb below, whose fast estimator has other bits than the strict one)
        for fields in (dict(iso=0.03125), dict(order=1), dict(order=2), dict(order=8), dict(tolerance=float(array.mean()))):
            report, other, _ = check(ctx, h, scene, **fields)
            assert packed(report) != packed(base), fields  # (a condition on the input: the field reaches the result)
            assert 0 <= report["over_area"] <= report["area"]
        shifted, moved, _ = check(ctx, h, scene, iso=0.03125)
        assert moved.tobytes() != array.tobytes()
        none, same, _ = check(ctx, h, scene, tolerance=base["max"])  # tolerance at max: no triangle is over
        assert none["over_triangles"] == 0 and none["over_area"] == 0.0 and same.tobytes() == array.tobytes() and none["rms"] == base["rms"]
        some, _, _ = check(ctx, h, scene, tolerance=float(np.median(array)))
        assert 0 < some["over_triangles"] < base["over_triangles"] and 0 < some["over_area"] < base["area"]
    finally:
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


# ---- 2: any mesh, the mesh unchanged, the same bytes on every run -----------------------------------------------------------------------------

def test_meshes_of_every_origin_stay_as_they_were_and_two_calls_agree(ctx):
    scene = ctx.create_scene(table_with_surfaces())
    lo, hi, n, values, iso = FIELDS["noise 1.5"]()
    box = ((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3))
    made = [from_values(ctx, n, values, iso, lo, hi)]
    try:
        made.append(from_scene(ctx, scene, M.Grid(*box, (27, 25, 23)), colours=True))
        made.append(filtered(ctx, made[1], dict(largest=1)))
        made.append(simplified(ctx, made[1], M.Grid(*box, (9, 8, 7))))
        made.append(placed(ctx, made[1], M.Grid(*box, (9, 8, 7))))
        made.append(slabbed(ctx, scene, M.Grid(*box, (27, 25, 23)), 5, normals=False))
        made.append(project(ctx, made[3], scene, M.mesh_project(reach=0.1))[0])
        kinds = ((False, False), (True, True), (True, True), (True, True), (True, True), (False, False), (True, True))
        for h, (normals, colours) in zip(made, kinds):
            assert counts(ctx, h)[1] > 0
            before = arrays(ctx, h, normals, colours)
            for fields in (dict(), dict(order=2, flags=FAST)):
                report, array, _ = check(ctx, h, scene, **fields)
                again, raw, twice = deviation(ctx, h, scene, M.mesh_deviation(**fields))
                assert raw == packed(report) and twice.tobytes() == array.tobytes()  # two calls: the same bytes
            assert same_arrays(arrays(ctx, h, normals, colours), before)  # the mesh's five arrays are as they were
            assert ctx.lib.rm_mesh_download(h, 5, None, 0) == INV  # ... and five they stay
        # the projected mesh's vertices lie on the surface; its triangles still chord it
        on = deviation(ctx, made[6], scene)[0]
        assert on["max"] > 0 and on["rms"] > 0
    finally:
        for h in reversed(made):
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_a_mesh_without_triangles_and_an_empty_mesh_succeed(ctx):
    scene = ctx.create_scene(S.single_sphere())
    lo, hi, n, v, iso = one_cell()
    one = from_values(ctx, n, v, iso, lo, hi)
    empty = from_values(ctx, (4, 4, 4), np.ones((5, 5, 5), F), 0.0, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    try:
        assert counts(ctx, one) == (1, 0) and counts(ctx, empty) == (0, 0)
        for h, vertices in ((one, 1), (empty, 0)):
            for block, samples in ((None, 16), (M.mesh_deviation(order=8, flags=FAST), 64)):
                ms = (C.c_float * 2)(5.0, 5.0)
                report, raw, array = deviation(ctx, h, scene, block, ms)  # (the guard round the buffer is checked in there)
                assert len(array) == 0 and list(ms) == [0.0, 0.0]
                assert raw == bytes(abi.RmMeshDeviationReport(vertices=vertices, samples=samples))
            assert ctx.lib.rm_mesh_deviation(h, scene.h, None, None, None, None) == OK  # report, triangles_host and out_ms2 may be NULL
    finally:
        ctx.lib.rm_mesh_destroy(one)
        ctx.lib.rm_mesh_destroy(empty)
        scene.destroy()


def test_three_levels_of_the_tree_both_spans_timed_the_flags_and_null_outputs(ctx):
    scene = ctx.create_scene(S.Mandelbulb())
    h = from_scene(ctx, scene, M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (96, 96, 96)), iso=0.0078125, normals=False)
    raws = []
    try:
        assert counts(ctx, h)[1] > 256 * 256  # (three levels of the tree)
        for flags in (0, FAST):
            block = M.mesh_deviation(flags=flags, iso=0.0078125, order=1)
            check(ctx, h, scene, flags=flags, iso=0.0078125, order=1)
            ms = (C.c_float * 2)(-1.0, -1.0)
            report, raw, array = deviation(ctx, h, scene, block, ms)
            assert ms[0] > 0.0 and ms[1] > 0.0, list(ms)
            raws.append(raw)
            only = abi.RmMeshDeviationReport()
            assert ctx.lib.rm_mesh_deviation(h, scene.h, C.byref(block), C.byref(only), None, None) == OK and bytes(only) == raw
            room = np.full(len(array), GUARD, F)
            assert ctx.lib.rm_mesh_deviation(h, scene.h, C.byref(block), None, native._fp(room), None) == OK and room.tobytes() == array.tobytes()
        assert raws[0] != raws[1]  # (a condition on the input: the flags reach the evaluator)
    finally:
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


# ---- 3: a bound that is derived ----------------------------------------------------------------------------------------------------------------

def test_a_projected_sphere_chords_by_no_more_than_its_circumradii_allow(ctx):
    """A sphere of radius R about c, extracted and projected with tolerance 0: the corners lie on it to within the projection's max_after.  A
    point of a flat triangle whose corners lie on the sphere is no further from the centre than R and no nearer than sqrt(R^2 - rho^2), rho the
    triangle's circumradius (the plane of the triangle cuts the sphere in its circumcircle; the nearest point of the plane is the circle's
    centre).  So max_t <= R - sqrt(R^2 - rho_t^2) + slack, slack = max_after (the corners' own residual) + 8 ulp of R (the fp32 evaluation of the
    point and the field), every sample lies inside (mean_signed < 0), and the finer grid's triangles chord less."""
    centre, R = (0.125, -0.0625, 0.1875), 0.875
    scene = ctx.create_scene(S.single_sphere(centre, R))
    rms = []
    try:
        for n in (16, 32):
            h = from_scene(ctx, scene, M.Grid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (n, n, n)), normals=False)
            moved, projection, _ = project(ctx, h, scene, M.mesh_project(tolerance=0.0))
            try:
                src = arrays(ctx, moved)
                p = src["positions"].astype(np.float64)[src["triangles"].astype(np.int64)]  # [T, 3, 3]
                a, b, c = (np.linalg.norm(p[:, i] - p[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0)))
                area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
                assert (area > 0).all()
                rho = a * b * c / (4.0 * area)
                assert (rho < R).all()
                slack = float(projection["max_after"]) + 8 * float(np.spacing(F(R)))
                bound = R - np.sqrt(R * R - rho * rho) + slack
                for order in DR.ORDERS:
                    report, array, _ = check(ctx, moved, scene, order=order)
                    worst = float((array.astype(np.float64) - bound).max())
                    print(f"\nsphere {n}^3 order {order}: T {len(array)}, max {report['max']:.6g}, rms {report['rms']:.6g}, mean {report['mean_signed']:.6g}, "
                          f"largest max_t - bound {worst:.3g}, slack {slack:.3g}")
                    assert (array.astype(np.float64) <= bound).all()
                    assert report["mean_signed"] < 0 and report["unevaluated_triangles"] == 0 and report["skipped_triangles"] == 0
                    if order == 4:
                        rms.append(report["rms"])
            finally:
                ctx.lib.rm_mesh_destroy(moved)
                ctx.lib.rm_mesh_destroy(h)
        assert rms[1] < rms[0]
    finally:
        scene.destroy()


# ---- 4: refusals with a device -------------------------------------------------------------------------------------------------------------------

def test_handle_level_refusals(ctx, gl_ctx):
    lib = ctx.lib
    scene, foreign = ctx.create_scene(S.single_sphere()), gl_ctx.create_scene(S.single_sphere())
    h = from_scene(ctx, scene, M.Grid((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (6, 6, 6)), normals=False)
    try:
        t = counts(ctx, h)[1]
        pattern = bytes(range(1, 113))
        report = abi.RmMeshDeviationReport.from_buffer_copy(pattern)
        out, ms = np.full(t, GUARD, F), (C.c_float * 2)(5.0, 5.0)
        o, r = native._fp(out), C.byref(report)
        who = "rm_mesh_deviation: "
        bad = M.mesh_deviation()
        bad.order = 3
        # 1. an invalid block speaks first, whatever the handles are
        for mesh, sc in ((h, scene.h), (None, scene.h), (h, None), (h, foreign.h), (None, None)):
            assert lib.rm_mesh_deviation(mesh, sc, C.byref(bad), r, o, ms) == INV
            text = (lib.rm_last_error(ctx.h) if mesh else lib.rm_last_error(None)).decode()
            assert text == who + "deviation order must be 1, 2, 4 or 8", text
        # 2. then a NULL mesh or scene, before the scene's context is looked at
        for mesh, sc in ((None, scene.h), (h, None), (None, foreign.h), (None, None)):
            for block in (None, C.byref(M.mesh_deviation())):
                assert lib.rm_mesh_deviation(mesh, sc, block, r, o, ms) == INV
                text = (lib.rm_last_error(ctx.h) if mesh else lib.rm_last_error(None)).decode()
                assert text == who + "NULL argument", text
        # 3. then a scene of another context
        assert lib.rm_mesh_deviation(h, foreign.h, None, r, o, ms) == INV
        assert lib.rm_last_error(ctx.h).decode() == who + "the scene belongs to another context"
        assert bytes(report) == pattern and (out == GUARD).all() and list(ms) == [5.0, 5.0]  # no refusal wrote anything
        assert lib.rm_mesh_deviation(h, scene.h, None, r, o, ms) == OK and (out != GUARD).all() and report.triangles == t and report.samples == 16
    finally:
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()
        foreign.destroy()


# ---- 5: the hosts ----------------------------------------------------------------------------------------------------------------------------------

LO, HI, N, ISO = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (40, 40, 40), 0.0078125
CLUSTERS = M.Grid(LO, HI, (10, 10, 10))


def test_python_host_equals_the_c_level_results(ctx):
    scene = ctx.create_scene(S.Mandelbulb())
    g = M.Grid(LO, HI, N)
    try:
        plain = ctx.extract_mesh(scene, g, iso=ISO)
        assert plain.deviation is None and plain.triangle_deviation is None and "deviation" not in plain.timings
        for given, block in ((True, M.mesh_deviation(iso=ISO)), (dict(order=2, flags=FAST), M.mesh_deviation(iso=ISO, order=2, flags=FAST)),
                             (M.mesh_deviation(iso=0.0, order=8), M.mesh_deviation(iso=0.0, order=8))):
            m = ctx.extract_mesh(scene, g, iso=ISO, deviation=given)
            h = from_scene(ctx, scene, g, iso=ISO)
            try:
                report, raw, array = deviation(ctx, h, scene, block)
            finally:
                ctx.lib.rm_mesh_destroy(h)
            assert m.triangle_deviation.dtype == F and m.triangle_deviation.shape == (len(m.triangles),) and m.triangle_deviation.tobytes() == array.tobytes()
            assert packed(m.deviation) == raw and tuple(m.deviation) == DR.FIELDS and m.timings["deviation"] > 0.0 and len(m.triangles) > 0
        # behind simplify, keep and project: the deviation is that of the mesh that is returned
        m = ctx.extract_mesh(scene, g, iso=ISO, simplify=CLUSTERS, keep=True, project=True, deviation=dict(order=2))
        sdf = lambda q: ctx.probe(scene, abi.RM_PROBE_SDF, q)
        want = DR.deviation(m.positions, m.triangles, sdf, iso=ISO, order=2)
        assert m.triangle_deviation.tobytes() == want["triangles"].tobytes() and DR.same(m.deviation, want["report"]) == [] and m.projection is not None
        empty = ctx.extract_mesh(scene, M.Grid((3.0, 3.0, 3.0), (4.0, 4.0, 4.0), (4, 4, 4)), deviation=True)
        assert empty.vertices == 0 and empty.triangle_deviation.shape == (0,) and empty.timings["deviation"] == 0.0 and empty.deviation["samples"] == 16
        for bad in (False, 16, dict(order=3), dict(orders=4)):
            with pytest.raises(ValueError):
                ctx.extract_mesh(scene, g, iso=ISO, deviation=bad)
        reserved = M.mesh_deviation()
        reserved.reserved[1] = 1
        with pytest.raises(Exception, match="deviation reserved must be 0"):
            ctx.extract_mesh(scene, g, iso=ISO, deviation=reserved)
    finally:
        scene.destroy()


def test_node_host_gives_the_python_bytes(ctx, tmp_path):
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(tmp_path)!r};
const ctx = new r.RenderJobContext(0), sc = new r.Mandelbulb(), g = r.meshGrid({list(LO)}, {list(HI)}, {list(N)});
const clusters = r.meshGrid({list(LO)}, {list(HI)}, {list(CLUSTERS.n)});
const save = (name, a) => fs.writeFileSync(d + "/" + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const a = ctx.extractMesh(sc, g, {{ iso: {ISO} }}, null, null, false, null, null, null, false, null, null, true);
const b = ctx.extractMesh(sc, g, {{ iso: {ISO} }}, null, true, false, {{ grid: clusters }}, true, null, false, null, true, {{ order: 2, flags: r.RM.RENDER_FAST }});
const c = ctx.extractMesh(sc, g, {{ iso: {ISO} }}, null, null, false, null, null, null, false, 7, null, {{ order: 8 }});
const plain = ctx.extractMesh(sc, g, {{ iso: {ISO} }});
if ("deviation" in plain || "triangleDeviation" in plain || plain.timings.length !== 3) process.exit(3);
for (const m of [a, b, c]) if (!(m.triangleDeviation instanceof Float32Array) || m.triangleDeviation.length !== m.triangles.length / 3 || !(m.deviation.milliseconds > 0) || m.timings.length !== 3) process.exit(4);
if (!("projection" in b) || "projection" in a) process.exit(5);
save("a", a.triangleDeviation); save("b", b.triangleDeviation); save("c", c.triangleDeviation); save("b_positions", b.positions);
fs.writeFileSync(d + "/reports.json", JSON.stringify([a.deviation, b.deviation, c.deviation]));
let refused = 0;
for (const bad of [{{ order: 3 }}, {{ orders: 4 }}, 7, false, {{ tolerance: -1 }}]) try {{ ctx.extractMesh(sc, g, null, null, null, false, null, null, null, false, null, null, bad); }} catch (e) {{ refused++; }}
if (refused !== 5) process.exit(6);
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    reports = json.loads((tmp_path / "reports.json").read_text())
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        g = M.Grid(LO, HI, N)
        a = ctx.extract_mesh(scene, g, iso=ISO, deviation=True)
        b = ctx.extract_mesh(scene, g, iso=ISO, keep=True, simplify=CLUSTERS, quadric=True, project=True, deviation=dict(order=2, flags=FAST))
        c = ctx.extract_mesh(scene, g, iso=ISO, slabs=7, deviation=dict(order=8))
    finally:
        scene.destroy()
    assert (tmp_path / "b_positions").read_bytes() == b.positions.tobytes()
    for name, m, got in (("a", a, reports[0]), ("b", b, reports[1]), ("c", c, reports[2])):
        assert len(m.triangles) > 0 and m.deviation["max"] > 0
        assert (tmp_path / name).read_bytes() == m.triangle_deviation.tobytes(), name
        assert DR.same({k: got[camel] for k, camel in CAMEL.items()}, m.deviation) == [], (name, got, m.deviation)  # (a JSON number gives every double and float back)
