"""Quadric placement on the GPU: rm_mesh_simplify_quadric against the numpy restatement (tests/mesh_quadric_ref.py) run on the downloaded source
arrays, and against rm_mesh_simplify on the same handle.  Every comparison is exact: integers, and floats by their bits."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_parts_ref as PR
import mesh_quadric_ref as QR
import mesh_simplify_ref as SR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import spread
from test_gpu_mesh_parts import ARRAYS, arrays, as_arrays, counts, filtered, from_scene, from_values, parts, same_arrays
from test_gpu_mesh_simplify import simplified

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def placed(c, h, grid, keep_duplicates=False, quadric=None):
    """rm_mesh_simplify_quadric of the handle on the mesh.Grid of clusters: the new handle (quadric None: a NULL block, the defaults)"""
    out = C.c_void_p()
    g, p = M.mesh_simplify(grid, keep_duplicates)
    q = None if quadric is None else C.byref(quadric)
    assert c.lib.rm_mesh_simplify_quadric(h, C.byref(g), C.byref(p), q, C.byref(out)) == OK, c.lib.rm_last_error(c.h)
    assert out.value
    return out


def check_quadric(c, h, grid, normals=False, colours=False, threshold=None):
    """Both settings of keep_duplicates: the positions are the restatement's bytes on the handle's downloaded arrays, every other array is what
    rm_mesh_simplify gives on the same handle; the source is unchanged afterwards.  Returns the restatement's dict (deduplicated) and the plain
    mesh's arrays."""
    src = arrays(c, h, normals, colours)
    block = None if threshold is None else M.mesh_quadric(threshold)
    for keep in (False, True):
        s, q = simplified(c, h, grid, keep), placed(c, h, grid, keep, block)
        try:
            plain, got = arrays(c, s, normals, colours), arrays(c, q, normals, colours)
            want = QR.simplify_quadric(grid.lo, grid.hi, grid.n, src["positions"], src["triangles"], src["normals"], src["colours"], keep_duplicates=keep,
                                       threshold=0.1 if threshold is None else threshold)
            assert same_arrays(got, dict(plain, positions=want["positions"])), (grid.n, keep)
            assert plain["positions"].tobytes() == want["plain"].tobytes()
            still = want["planes"] == 0  # a cluster without planes holds simplify's own bytes
            assert got["positions"][still].tobytes() == plain["positions"][still].tobytes()
            ms = (C.c_float * 3)()
            assert c.lib.rm_mesh_timings(q, ms) == OK and ms[0] == 0.0 and ms[1] >= 0.0 and ms[2] == 0.0
            if len(src["positions"]):
                assert ms[1] > 0.0
            for name, what, _, _ in ARRAYS:
                assert bool(c.lib.rm_mesh_device_ptr(q, what)) == (got[name] is not None and got[name].size > 0), name
            if not keep:
                first, first_plain = want, plain
        finally:
            c.lib.rm_mesh_destroy(s)
            c.lib.rm_mesh_destroy(q)
    assert same_arrays(arrays(c, h, normals, colours), src)  # the source is untouched
    return first, first_plain


# ---- 1: meshes from values ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sources(ctx):
    """the source meshes of QR.CASES, made once: name -> (handle, field lo, field hi)"""
    made = {}
    for name, make in QR.fields().items():
        lo, hi, n, values, iso = make()
        made[name] = (from_values(ctx, n, values, iso, lo, hi), lo, hi)
    yield made
    for h, _, _ in made.values():
        ctx.lib.rm_mesh_destroy(h)


@pytest.mark.parametrize("case", list(QR.CASES))
def test_a_quadric_placed_field_is_the_restatement(ctx, sources, case):
    field, lo, hi, n = QR.CASES[case]
    h, flo, fhi = sources[field]
    grid = M.Grid(lo or flo, hi or fhi, n)
    m, plain = check_quadric(ctx, h, grid)
    moved = int((m["positions"] != plain["positions"]).any(axis=1).sum())
    print(case, counts(ctx, h), "->", len(m["positions"]), len(m["triangles"]), "moved", moved, "without planes", int((m["planes"] == 0).sum()), "clamped", m["clamped"])
    low, high = SR.box_of(grid.lo, grid.hi, grid.n, m["cells"])
    assert (m["positions"] >= low - np.spacing(np.abs(low))).all() and (m["positions"] <= high + np.spacing(np.abs(high))).all()
    assert (moved > 0) == (case not in QR.UNMOVED)


def test_another_threshold_is_the_restatement_too(ctx, sources):
    h, lo, hi = sources["box 48"]
    a, _ = check_quadric(ctx, h, M.Grid(lo, hi, (12, 12, 12)), threshold=0.0)
    b, _ = check_quadric(ctx, h, M.Grid(lo, hi, (12, 12, 12)), threshold=0.5)
    assert a["positions"].tobytes() != b["positions"].tobytes()  # (a condition on the input: the threshold reaches the solve)


def test_empty_unreferenced_and_zero_area_sources(ctx):
    """An empty source; a source whose only vertex no triangle references; the noise field's unreferenced vertices, whose clusters have no planes
    and hold simplify's bytes (check_quadric asserts that of every case: here the case is shown to have some); and a hand-made field with
    zero-area triangles: a corner of -1e-30 among +1 puts the eight surrounding surface-nets vertices at that corner, so the triangles between
    them have a zero cross product and contribute nothing, beside a sphere whose triangles do."""
    grid = M.Grid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 4, 4))
    h = from_values(ctx, (4, 4, 4), np.ones((5, 5, 5), F), 0.0, grid.lo, grid.hi)  # no vertex at all
    try:
        for keep in (False, True):
            q = placed(ctx, h, grid, keep)
            assert counts(ctx, q) == (0, 0) and all(ctx.lib.rm_mesh_download(q, what, None, 0) == OK for what in (0, 3, 4))
            ms = (C.c_float * 3)(1, 1, 1)
            assert ctx.lib.rm_mesh_timings(q, ms) == OK and list(ms) == [0.0, 0.0, 0.0]
            again = placed(ctx, q, grid)
            assert counts(ctx, again) == (0, 0)
            ctx.lib.rm_mesh_destroy(again)
            ctx.lib.rm_mesh_destroy(q)
    finally:
        ctx.lib.rm_mesh_destroy(h)
    v = np.ones((2, 2, 2), F)
    v[0, 0, 0] = -1.0
    h = from_values(ctx, (1, 1, 1), v, 0.0, grid.lo, grid.hi)  # one vertex, no triangle
    try:
        assert counts(ctx, h) == (1, 0)
        m, plain = check_quadric(ctx, h, grid)
        assert len(m["positions"]) == 1 and m["planes"].tolist() == [0] and m["positions"].tobytes() == plain["positions"].tobytes()
    finally:
        ctx.lib.rm_mesh_destroy(h)
    lo, hi, n, values, iso = PR.noise_field() + (0.25,)
    h = from_values(ctx, n, values, iso, lo, hi)
    try:
        m, _ = check_quadric(ctx, h, M.Grid(lo, hi, (128, 128, 128)))
        assert 0 < int((m["planes"] == 0).sum()) < len(m["planes"])
    finally:
        ctx.lib.rm_mesh_destroy(h)
    lo, hi, n, values = SR.sphere_field(16)
    values = values.copy()
    values[1, 1, 1] = -1e-30
    h = from_values(ctx, n, values, 0.0, lo, hi)
    try:
        src = arrays(ctx, h)
        p, t = src["positions"], src["triangles"].astype(np.int64)
        e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
        flat = ~(np.cross(e1.astype(np.float64), e2.astype(np.float64)) != 0).any(axis=1)
        assert 0 < int(flat.sum()) < len(t)  # (a condition on the input)
        for clusters in ((4, 4, 4), (16, 16, 16), (32, 32, 32)):
            check_quadric(ctx, h, M.Grid(lo, hi, clusters))
    finally:
        ctx.lib.rm_mesh_destroy(h)


# ---- 2: a scene source with normals and colours ---------------------------------------------------------------------------------------------------

BOX_GRID = M.Grid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (48, 48, 48))


def test_a_sharp_box_keeps_its_edges_through_quadric_placement(ctx):
    """The off-grid box of the restatement's tests as a composition-API scene, extracted sharp at 48^3 with normals and colours, clustered at 12^3
    and (11, 9, 13).  Normals and colours are rm_mesh_simplify's bytes (check_quadric); the worst |rm_probe(RM_PROBE_SDF)| at the positions is
    strictly below plain rm_mesh_simplify's on the same handle.  Both are printed; only their order is asserted (the measured values:
    INTEGRATION.md "Quadric placement")."""
    scene = ctx.create_scene(S.CsgScene().box(QR.BOX_CENTRE, QR.BOX_HALF, surface=S.Surface(diffuse=(0.875, 0.5, 0.125), specular=(0.25, 0.25, 0.25), roughness=0.5)))
    h = None
    try:
        h = from_scene(ctx, scene, BOX_GRID, True, normals=True, colours=True)
        assert counts(ctx, h)[0] > 3000
        for n in ((12, 12, 12), (11, 9, 13)):
            m, plain = check_quadric(ctx, h, M.Grid(BOX_GRID.lo, BOX_GRID.hi, n), True, True)
            assert m["normals"] is not None and m["colours"] is not None and len(m["triangles"]) > 0
            off_plain = float(np.abs(ctx.probe(scene, abi.RM_PROBE_SDF, plain["positions"])).max())
            off_quadric = float(np.abs(ctx.probe(scene, abi.RM_PROBE_SDF, m["positions"])).max())
            print(f"sharp box 48^3 -> {n}: {len(m['positions'])} vertices; worst |sdf| plain {off_plain:.3e}, quadric {off_quadric:.3e}")
            assert off_quadric < off_plain
    finally:
        if h is not None:
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


# ---- 3: composition, order of arrival, lifetimes ----------------------------------------------------------------------------------------------------

def test_the_result_is_filtered_labelled_and_simplified_again(ctx, sources):
    h, lo, hi = sources["noise 0.25"]
    q = placed(ctx, h, M.Grid(lo, hi, (37, 29, 53)))
    s = simplified(ctx, h, M.Grid(lo, hi, (37, 29, 53)))
    f = g = None
    try:
        f, g = filtered(ctx, q, None), filtered(ctx, s, None)
        got, kept = arrays(ctx, q), arrays(ctx, f)
        used = np.zeros(len(got["positions"]), bool)
        used[got["triangles"].reshape(-1)] = True
        assert (~used).sum() == 37 and kept["positions"].tobytes() == got["positions"][used].tobytes()
        assert kept["triangles"].tobytes() == arrays(ctx, g)["triangles"].tobytes()
        (labels, sizes), (want_labels, want_sizes) = parts(ctx, q), parts(ctx, s)  # the same connectivity: the same labelling
        assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
        coarse = M.Grid((-0.9, -1.1, -1.0), (1.0, 0.95, 1.2), (9, 11, 7))  # a placed mesh is a source like any other, for both entries
        m, _ = check_quadric(ctx, q, coarse)
        assert 0 < len(m["positions"]) <= 9 * 11 * 7 and len(m["triangles"]) > 0
        again = simplified(ctx, q, coarse)
        assert counts(ctx, again) == (len(m["positions"]), len(m["triangles"]))
        ctx.lib.rm_mesh_destroy(again)
    finally:
        for handle in (f, g, s, q):
            if handle is not None:
                ctx.lib.rm_mesh_destroy(handle)


def test_five_runs_give_identical_bytes(ctx, sources):
    for field, n in (("noise 0.25", (20, 20, 20)), ("box 48", (11, 9, 13))):
        h, lo, hi = sources[field]
        seen = set()
        for _ in range(5):
            blob = b""
            for keep in (False, True):
                q = placed(ctx, h, M.Grid(lo, hi, n), keep)
                try:
                    got = arrays(ctx, q)
                    blob += b"".join(got[k].tobytes() for k in ("positions", "triangles", "cells"))
                finally:
                    ctx.lib.rm_mesh_destroy(q)
            seen.add(blob)
        assert len(seen) == 1, field


def test_lifetime_and_handle_level_refusals(ctx):
    lib = ctx.lib
    lo, hi, n, values, iso = PR.two_balls_field() + (0.0,)
    last = lambda: lib.rm_last_error(ctx.h).decode()
    who = "rm_mesh_simplify_quadric: "
    grid = M.Grid(lo, hi, (6, 6, 6))
    g, p = M.mesh_simplify(grid)
    q = M.mesh_quadric()
    h = from_values(ctx, n, values, iso, lo, hi)
    src = arrays(ctx, h)
    out = C.c_void_p(12345)
    call = lib.rm_mesh_simplify_quadric
    assert call(h, C.byref(g), C.byref(p), C.byref(q), None) == INV and last() == who + "NULL argument"
    assert call(None, C.byref(g), C.byref(p), C.byref(q), C.byref(out)) == INV and out.value == 12345
    assert call(h, None, C.byref(p), C.byref(q), C.byref(out)) == INV and last() == who + "NULL grid" and out.value == 12345
    bad = grid.to_c()
    bad.n[2] = 0
    assert call(h, C.byref(bad), C.byref(p), C.byref(q), C.byref(out)) == INV and last().startswith(who + "grid n must be")
    assert call(h, C.byref(g), C.byref(abi.RmMeshSimplify(2)), C.byref(q), C.byref(out)) == INV and last() == who + "keep_duplicates must be 0 or 1"
    assert call(h, C.byref(g), C.byref(abi.RmMeshSimplify(0, (C.c_int32 * 3)(0, 0, 1))), C.byref(q), C.byref(out)) == INV and last() == who + "simplify reserved must be 0"
    for t in (1.0, -0.125, float("nan"), float("inf")):
        assert call(h, C.byref(g), C.byref(p), C.byref(abi.RmMeshQuadric(t)), C.byref(out)) == INV and last() == who + "quadric threshold must be finite and in [0, 1)"
    assert call(h, C.byref(g), C.byref(p), C.byref(abi.RmMeshQuadric(0.1, (C.c_int32 * 3)(0, 7, 0))), C.byref(out)) == INV and last() == who + "quadric reserved must be 0"
    assert out.value == 12345
    assert call(h, C.byref(g), None, None, C.byref(out)) == OK and out.value not in (None, 12345)  # NULL blocks: the defaults
    s = out
    want = QR.simplify_quadric(grid.lo, grid.hi, grid.n, src["positions"], src["triangles"])
    want = {k: want[k] for k in ("positions", "normals", "colours", "triangles", "cells")}
    assert same_arrays(arrays(ctx, s), want)
    assert same_arrays(arrays(ctx, h), src) and parts(ctx, h)[1].shape == (2, 2)  # the source is unchanged and still usable
    twice = placed(ctx, h, grid, quadric=q)
    assert same_arrays(arrays(ctx, twice), want)
    lib.rm_mesh_destroy(h)  # the result outlives the source
    assert same_arrays(arrays(ctx, s), want) and same_arrays(arrays(ctx, twice), want)
    labels, sizes = parts(ctx, s)  # it starts without a labelling of its own, and gets one like any mesh
    want_labels, want_sizes = PR.components(len(want["positions"]), want["triangles"])
    assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
    buf = np.zeros(16, np.uint8)
    assert lib.rm_mesh_download(s, abi.RM_MESH_NORMALS, buf.ctypes.data_as(C.c_void_p), 0) == INV and "without this array" in last()
    lib.rm_mesh_destroy(twice)
    lib.rm_mesh_destroy(s)


# ---- 4: the hosts ---------------------------------------------------------------------------------------------------------------------------------

def test_python_host_equals_the_c_level_chain(ctx):
    grid, clusters = M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (48, 48, 48)), M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (12, 12, 12))
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        h = from_scene(ctx, scene, grid, iso=2.0 ** -7, colours=True)
        q = placed(ctx, h, clusters)
        loose = placed(ctx, h, clusters, quadric=M.mesh_quadric(0.5))
        f = filtered(ctx, q, None)
        want, (want_labels, want_sizes), unfiltered, other = arrays(ctx, f, True, True), parts(ctx, f), arrays(ctx, q, True, True), arrays(ctx, loose, True, True)
        for handle in (f, loose, q, h):
            ctx.lib.rm_mesh_destroy(handle)
        assert 0 < len(want["positions"]) <= len(unfiltered["positions"]) < 12 ** 3 and other["positions"].tobytes() != unfiltered["positions"].tobytes()
        for quadric in (True, dict(), dict(threshold=0.1), M.mesh_quadric(), abi.RmMeshQuadric(0.1)):
            m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, simplify=clusters, quadric=quadric, keep=True, components=True)
            assert same_arrays(as_arrays(m), want) and np.array_equal(m.labels, want_labels) and np.array_equal(m.component_sizes, want_sizes)
            assert (m.grid.lo, m.grid.hi, m.grid.n) == (clusters.lo, clusters.hi, clusters.n)
            assert m.timings["sampling"] == 0.0 and m.timings["meshing"] > 0.0 and m.timings["attributes"] == 0.0
        m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, simplify=dict(grid=clusters), quadric=dict(threshold=0.5))
        assert same_arrays(as_arrays(m), other) and m.labels is None
        plain = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, simplify=clusters)  # quadric=None: rm_mesh_simplify as before
        assert plain.positions.tobytes() != unfiltered["positions"].tobytes() and same_arrays(dict(as_arrays(plain), positions=unfiltered["positions"]), unfiltered)
        for bad in (False, 3, 0.1, dict(threshold=1.0), dict(threshold=float("nan")), dict(threshold="0.1"), dict(lambda_min=0.1), abi.RmMeshQuadric(-1.0)):
            with pytest.raises(ValueError):
                ctx.extract_mesh(scene, grid, simplify=clusters, quadric=bad)
        for quadric in (True, dict(threshold=0.25)):
            with pytest.raises(ValueError, match="simplify"):
                ctx.extract_mesh(scene, grid, quadric=quadric)
        with pytest.raises(RuntimeError, match="quadric reserved"):
            ctx.extract_mesh(scene, grid, simplify=clusters, quadric=abi.RmMeshQuadric(0.1, (C.c_int32 * 3)(1, 0, 0)))
    finally:
        scene.destroy()
    lo, hi, n, values, iso = PR.noise_field() + (0.25,)
    g, coarse = M.Grid(lo, hi, n), M.Grid(lo, hi, (20, 20, 20))
    h = from_values(ctx, n, values, iso, lo, hi)
    q = placed(ctx, h, coarse, True)
    want = arrays(ctx, q)
    ctx.lib.rm_mesh_destroy(q)
    ctx.lib.rm_mesh_destroy(h)
    m = ctx.mesh_from_values(g, values, iso, simplify=dict(grid=coarse, keep_duplicates=True), quadric=True)
    assert same_arrays(as_arrays(m), want) and len(m.triangles) == 40191 + 214
    with pytest.raises(ValueError, match="simplify"):
        ctx.mesh_from_values(g, values, iso, quadric=True)


def test_node_host_gives_the_python_bytes(ctx, tmp_path):
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    lo, hi, n, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (40, 40, 40), 0.0078125
    flo, fhi, fn, values, fiso = PR.noise_field() + (0.25,)
    np.ascontiguousarray(values, "<f4").tofile(tmp_path / "field")
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(tmp_path)!r};
const ctx = new r.RenderJobContext(0), sc = new r.Mandelbulb(), g = r.meshGrid({list(lo)}, {list(hi)}, {list(n)});
const clusters = r.meshGrid({list(lo)}, {list(hi)}, [10, 10, 10]);
const save = (name, a) => fs.writeFileSync(d + "/" + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const m = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, null, true, true, {{ grid: clusters }}, true);
for (const k of ["positions", "normals", "colours", "triangles", "cells", "labels", "componentSizes"]) save("scene_" + k, m[k]);
const loose = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, undefined, undefined, undefined, {{ grid: clusters, keepDuplicates: true }}, {{ threshold: 0.5 }});
if ("labels" in loose || !(loose.timings[1] > 0) || loose.timings[0] !== 0) process.exit(3);
save("loose_positions", loose.positions);
save("loose_triangles", loose.triangles);
const plain = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, null, null, false, {{ grid: clusters }}, null);
save("plain_positions", plain.positions);
const raw = fs.readFileSync(d + "/field"), values = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);
const fg = r.meshGrid({list(flo)}, {list(fhi)}, {list(fn)}), coarse = r.meshGrid({list(flo)}, {list(fhi)}, [20, 20, 20]);
const f = ctx.meshFromValues(fg, values, {fiso}, null, false, {{ grid: coarse }}, true);
for (const k of ["positions", "triangles", "cells"]) save("field_" + k, f[k]);
if (f.normals !== null || f.colours !== null || "labels" in f) process.exit(5);
let refused = 0;
for (const bad of [{{ threshold: 1 }}, {{ threshold: NaN }}, {{ threshold: "0.1" }}, {{ lambda: 0.1 }}, 7, false])
  try {{ ctx.meshFromValues(fg, values, {fiso}, null, false, {{ grid: coarse }}, bad); }} catch (e) {{ refused++; }}
for (const q of [true, {{ threshold: 0.25 }}]) {{
  try {{ ctx.meshFromValues(fg, values, {fiso}, null, false, null, q); }} catch (e) {{ refused++; }}
  try {{ ctx.extractMesh(sc, g, null, null, null, false, null, q); }} catch (e) {{ refused++; }}
}}
if (refused !== 10) process.exit(6);
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    h = ctx.create_scene(S.Mandelbulb())
    try:
        g, clusters = M.Grid(lo, hi, n), M.Grid(lo, hi, (10, 10, 10))
        want = ctx.extract_mesh(h, g, iso=iso, colours=True, simplify=clusters, quadric=True, keep=True, components=True)
        assert want.vertices > 0 and len(want.triangles) > 0
        for k in ("positions", "normals", "colours", "triangles", "cells", "labels"):
            assert (tmp_path / ("scene_" + k)).read_bytes() == getattr(want, k).tobytes(), k
        assert (tmp_path / "scene_componentSizes").read_bytes() == want.component_sizes.tobytes()
        loose = ctx.extract_mesh(h, g, iso=iso, colours=True, simplify=dict(grid=clusters, keep_duplicates=True), quadric=dict(threshold=0.5))
        assert (tmp_path / "loose_triangles").read_bytes() == loose.triangles.tobytes() and (tmp_path / "loose_positions").read_bytes() == loose.positions.tobytes()
        plain = ctx.extract_mesh(h, g, iso=iso, colours=True, simplify=clusters)
        assert (tmp_path / "plain_positions").read_bytes() == plain.positions.tobytes() != loose.positions.tobytes()
    finally:
        h.destroy()
    want = ctx.mesh_from_values(M.Grid(flo, fhi, fn), values, fiso, simplify=M.Grid(flo, fhi, (20, 20, 20)), quadric=True)
    assert (want.vertices, len(want.triangles)) == (7999, 40191)
    for k in ("positions", "triangles", "cells"):
        assert (tmp_path / ("field_" + k)).read_bytes() == getattr(want, k).tobytes(), k


# ---- one measurement, no bar ------------------------------------------------------------------------------------------------------------------

def test_measure_quadric_placement_on_the_mandelbulb_256_cubed(ctx):
    """Mandelbulb on 256^3 cells of [-1.25, 1.25]^3 at iso 2^-7 (the mesh of profiles/mesh_simplify.txt), strict build, clustered at 64^3.  The
    extraction and each entry are warmed once, then plain rm_mesh_simplify and rm_mesh_simplify_quadric alternate five times: median (min .. max)
    in milliseconds of the call's slot of rm_mesh_timings, and the ratio of the medians.  The last placed mesh is checked against the
    restatement (this is also the large mesh's check).  No assertion on time."""
    lo, hi, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), 0.0078125
    scene = ctx.create_scene(S.Mandelbulb())
    h = None
    try:
        ctx.lib.rm_mesh_destroy(from_scene(ctx, scene, M.Grid(lo, hi, (256, 256, 256)), iso=iso, normals=False))  # warm: the scene's grid, the code objects
        h = from_scene(ctx, scene, M.Grid(lo, hi, (256, 256, 256)), iso=iso, normals=False)
        v, t = counts(ctx, h)
        grid = M.Grid(lo, hi, (64, 64, 64))
        ms = (C.c_float * 3)()
        ctx.lib.rm_mesh_destroy(simplified(ctx, h, grid))
        ctx.lib.rm_mesh_destroy(placed(ctx, h, grid))
        times = {"plain": [], "quadric": []}
        for run in range(5):
            for name, make in (("plain", simplified), ("quadric", placed)):
                s = make(ctx, h, grid)
                assert ctx.lib.rm_mesh_timings(s, ms) == OK
                times[name].append(float(ms[1]))
                after = counts(ctx, s)
                if name == "quadric" and run == 4:
                    got = arrays(ctx, s)
                ctx.lib.rm_mesh_destroy(s)
        ratio = float(np.median(times["quadric"]) / np.median(times["plain"]))
        print(f"\nmandelbulb 256^3 iso 2^-7 strict: {v} vertices, {t} triangles, clusters 64^3 -> {after[0]} vertices, {after[1]} triangles")
        print(f"  rm_mesh_simplify {spread(times['plain'])} ms, rm_mesh_simplify_quadric {spread(times['quadric'])} ms, median (min .. max) of 5 alternating runs; ratio {ratio:.2f}")
        assert all(x > 0.0 for x in times["plain"] + times["quadric"])
        src = arrays(ctx, h)
        want = QR.simplify_quadric(grid.lo, grid.hi, grid.n, src["positions"], src["triangles"])
        assert same_arrays(got, {k: want[k] for k in ("positions", "normals", "colours", "triangles", "cells")})
    finally:
        if h is not None:
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()
