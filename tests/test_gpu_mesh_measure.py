"""Measures and edge topology on the GPU: rm_mesh_measure and rm_mesh_measure_components against the numpy restatement
(tests/mesh_measure_ref.py) run on the handle's downloaded arrays and labels.  Every comparison is exact: integers, and floats and doubles by
their bits."""
import ctypes as C
import math
import shutil
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import mesh_measure_ref as QR
import mesh_simplify_ref as SR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import spread, table_with_surfaces
from test_gpu_mesh_parts import arrays, counts, filtered, from_scene, from_values, parts, same_arrays
from test_gpu_mesh_quadric import placed
from test_gpu_mesh_simplify import simplified

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def measured(c, h, timed=True):
    """(measures dict with component_edges, the struct's 160 bytes + the rows' bytes, [ms topology, ms geometry]) of a handle"""
    block, ms = abi.RmMeshMeasures(), (C.c_float * 2)(-1.0, -1.0)
    assert c.lib.rm_mesh_measure(h, C.byref(block), ms if timed else None) == OK, c.lib.rm_last_error(c.h)
    rows = np.full((int(block.components), 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    assert c.lib.rm_mesh_measure_components(h, rows.ctypes.data_as(C.c_void_p) if len(rows) else None, rows.nbytes) == OK, c.lib.rm_last_error(c.h)
    assert block.reserved == 0
    return dict(abi.mesh_measures_dict(block), component_edges=rows), bytes(block) + rows.tobytes(), [float(ms[0]), float(ms[1])]


def check_measures(c, h, normals=False, colours=False):
    """The handle's measures against the restatement of its downloaded arrays and labels; the arrays and the labelling are unchanged afterwards.
    Returns the measures, with the call's milliseconds as "ms"."""
    src = arrays(c, h, normals, colours)
    got, blob, ms = measured(c, h)
    labels, sizes = parts(c, h)
    want = QR.measure(src["positions"], src["triangles"], labels, len(sizes))
    assert QR.same(got, want) == [], (QR.same(got, want), {k: (got[k], want[k]) for k in QR.same(got, want) if k != "component_edges"})
    assert got["boundary_edges"] + got["regular_edges"] + got["irregular_edges"] == got["edges"]
    assert got["component_edges"][:, 0].sum() == got["edges"] and (got["vertices"], got["triangles"]) == counts(c, h)
    assert (ms[0] > 0.0 and ms[1] > 0.0) or ms == [0.0, 0.0]  # (zero: an empty mesh, or a handle that an earlier test measured)
    again, blob2, ms2 = measured(c, h)  # the stored result: the same bytes, no time
    assert blob2 == blob and ms2 == [0.0, 0.0]
    assert same_arrays(arrays(c, h, normals, colours), src)
    labels2, sizes2 = parts(c, h)
    assert np.array_equal(labels2, labels) and np.array_equal(sizes2, sizes)
    return dict(got, ms=ms)


# ---- 1: the smallest meshes ------------------------------------------------------------------------------------------------------------------------

def test_one_inside_corner_is_the_smallest_closed_mesh(ctx):
    v = np.ones((3, 3, 3), F)
    v[1, 1, 1] = -1.0
    h = from_values(ctx, (2, 2, 2), v, 0.0, *BOX)
    try:
        m = check_measures(ctx, h)
        assert (m["vertices"], m["triangles"], m["edges"], m["regular_edges"], m["euler"], m["closed"]) == (8, 12, 18, 18, 2, True)
        assert (m["components"], m["closed_components"], m["used_vertices"], m["finite_vertices"]) == (1, 1, 8, 8)
        assert m["component_edges"].tolist() == [[18, 0, 0, 0]] and m["volume"] > 0.0 and m["area"] > 0.0 and m["ms"][0] > 0.0 and m["ms"][1] > 0.0
        assert all(abs(x + 1 / 6) < 1e-6 for x in m["lo"]) and all(abs(x - 1 / 6) < 1e-6 for x in m["hi"])  # each vertex: the mean of three crossings at 1/2
    finally:
        ctx.lib.rm_mesh_destroy(h)


def test_the_empty_mesh(ctx):
    h = from_values(ctx, (4, 4, 4), np.ones((5, 5, 5), F), 0.0, *BOX)
    try:
        m, blob, ms = measured(ctx, h)
        assert blob == bytes(160) and ms == [0.0, 0.0] and m["component_edges"].shape == (0, 4) and m["closed"] is False
        assert ctx.lib.rm_mesh_measure_components(h, None, 32) == INV
        check_measures(ctx, h)
    finally:
        ctx.lib.rm_mesh_destroy(h)
    v = np.ones((2, 2, 2), F)
    v[0, 0, 0] = -1.0
    h = from_values(ctx, (1, 1, 1), v, 0.0, *BOX)  # one vertex, no triangle
    try:
        m = check_measures(ctx, h)
        assert (m["vertices"], m["triangles"], m["used_vertices"], m["finite_vertices"], m["components"], m["closed_components"], m["closed"]) == (1, 0, 0, 1, 1, 0, False)
        assert m["lo"] == m["hi"] and m["area"] == 0.0 and m["component_edges"].tolist() == [[0, 0, 0, 0]]
    finally:
        ctx.lib.rm_mesh_destroy(h)


def test_a_plane_through_the_grid_is_open(ctx):
    n = (4, 3, 2)
    z = np.linspace(-1.0, 1.0, n[2] + 1, dtype=np.float64)
    v = np.broadcast_to((z - 0.25)[:, None, None], (n[2] + 1, n[1] + 1, n[0] + 1)).astype(F)
    h = from_values(ctx, n, v, 0.0, *BOX)
    try:
        m = check_measures(ctx, h)
        assert m["boundary_edges"] > 0 and not m["closed"] and m["irregular_edges"] == 0 and m["closed_components"] == 0 and m["triangles"] > 0
        assert m["lo"][2] == m["hi"][2] == 0.25 and abs(m["volume"]) < 1e-12
    finally:
        ctx.lib.rm_mesh_destroy(h)


# ---- 2: the shared fields, and the rest of the chain on them --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sources(ctx):
    """the meshes of SR.fields(), made once: name -> (handle, lo, hi)"""
    made = {}
    for name, make in SR.fields().items():
        lo, hi, n, values, iso = make()
        made[name] = (from_values(ctx, n, values, iso, lo, hi), lo, hi)
    yield made
    for h, _, _ in made.values():
        ctx.lib.rm_mesh_destroy(h)


def test_the_sphere(ctx, sources):
    m = check_measures(ctx, sources["sphere"][0])
    assert (m["vertices"], m["triangles"], m["edges"], m["regular_edges"], m["euler"], m["closed"], m["closed_components"]) == (6928, 13852, 20778, 20778, 2, True, 1)
    assert abs(m["volume"] - 4 / 3 * math.pi * 0.8 ** 3) < 0.01 * m["volume"] and abs(m["area"] - 4 * math.pi * 0.64) < 0.01 * m["area"]


def test_two_balls_and_the_snake(ctx, sources):
    m = check_measures(ctx, sources["two balls"][0])
    assert (m["euler"], m["components"], m["closed_components"], m["closed"]) == (4, 2, 2, True)
    assert (m["component_edges"][:, 1:] == 0).all() and (m["component_edges"][:, 0] > 0).all()
    m = check_measures(ctx, sources["snake"][0])
    assert m["closed"] and m["euler"] == 2 * m["closed_components"] == 2 * m["components"] and m["volume"] > 0.0


def test_the_noise_field_has_every_class(ctx, sources):
    m = check_measures(ctx, sources["noise 0.25"][0])
    assert (m["vertices"], m["triangles"], m["boundary_edges"], m["irregular_edges"]) == (66175, 185110, 7006, 22848)
    assert m["unbalanced_edges"] > 0 and m["used_vertices"] < m["vertices"] and m["components"] > 1 and not m["closed"]
    assert m["regular_edges"] > 0 and m["skipped_triangles"] == 0 and m["unmeasured_triangles"] == 0


@pytest.mark.parametrize("clusters", [4, 8])
@pytest.mark.parametrize("keep_duplicates", [False, True])
def test_the_noise_field_clustered(ctx, sources, clusters, keep_duplicates):
    h, lo, hi = sources["noise 0.25"]
    s = simplified(ctx, h, M.Grid(lo, hi, (clusters,) * 3), keep_duplicates)
    try:
        m = check_measures(ctx, s)
        print("noise clustered", clusters, keep_duplicates, {k: m[k] for k in ("vertices", "triangles", "edges", "boundary_edges", "irregular_edges", "unbalanced_edges")})
        assert m["irregular_edges"] > 0 and m["triangles"] > 0 and not m["closed"]
    finally:
        ctx.lib.rm_mesh_destroy(s)


def test_the_sphere_placed_by_quadrics_and_filtered(ctx, sources):
    h, lo, hi = sources["sphere"]
    q = placed(ctx, h, M.Grid(lo, hi, (12, 12, 12)))
    f = filtered(ctx, q, None)
    try:
        m = check_measures(ctx, q)
        assert m["triangles"] == 836 and m["closed"] and m["euler"] == 2
        mf = check_measures(ctx, f)
        assert QR.same(mf, m) == []  # nothing to drop: the same mesh
    finally:
        ctx.lib.rm_mesh_destroy(f)
        ctx.lib.rm_mesh_destroy(q)


def test_the_snake_clustered_has_irregular_edges_in_both_bodies(ctx, sources):
    h, _, _ = sources["snake"]
    s = simplified(ctx, h, M.Grid((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (8, 8, 8)))
    try:
        m = check_measures(ctx, s)
        assert (m["vertices"], m["triangles"]) == (138, 303) and m["boundary_edges"] == 0 and not m["closed"] and m["closed_components"] == 0
        assert (m["component_edges"][:, 2] > 0).all() and (m["component_edges"][:, 3] > 0).all() and m["components"] == 2
    finally:
        ctx.lib.rm_mesh_destroy(s)


def test_a_filtered_mesh_has_the_sources_rows_of_the_kept_components(ctx, sources):
    h, _, _ = sources["noise 0.25"]
    whole = check_measures(ctx, h)
    _, sizes = parts(ctx, h)
    rule = dict(largest=3)  # (min_triangles 1, the default)
    order = sorted((c for c in range(len(sizes)) if sizes[c, 1] >= 1), key=lambda c: (-int(sizes[c, 1]), c))[:3]
    kept = sorted(order)  # the kept components keep their order
    f = filtered(ctx, h, rule)
    try:
        m = check_measures(ctx, f)
        assert m["components"] == len(kept) > 1 and np.array_equal(m["component_edges"], whole["component_edges"][kept])
        assert m["edges"] == whole["component_edges"][kept, 0].sum() and m["used_vertices"] == m["vertices"]
    finally:
        ctx.lib.rm_mesh_destroy(f)


# ---- 3: scenes ---------------------------------------------------------------------------------------------------------------------------------------------

def test_a_sharp_csg_mesh_with_normals_and_colours(ctx):
    scene = ctx.create_scene(table_with_surfaces())
    h = None
    try:
        h = from_scene(ctx, scene, M.Grid((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), (32, 32, 32)), True, normals=True, colours=True)
        m = check_measures(ctx, h, True, True)
        assert m["vertices"] > 1000 and m["boundary_edges"] == 0 and m["volume"] > 0.0  # the scene lies inside the grid: no open border
    finally:
        if h is not None:
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


@pytest.mark.parametrize("flags", [0, abi.RM_RENDER_FAST])
def test_the_largest_body_of_a_mandelbulb(ctx, flags):
    scene = ctx.create_scene(S.Mandelbulb())
    h = f = None
    try:
        h = from_scene(ctx, scene, M.Grid((-1.25,) * 3, (1.25,) * 3, (32, 32, 32)), iso=2.0 ** -7, normals=False, flags=flags)
        f = filtered(ctx, h, dict(largest=1))
        whole, one = check_measures(ctx, h), check_measures(ctx, f)
        _, sizes = parts(ctx, h)
        largest = min(range(len(sizes)), key=lambda c: (-int(sizes[c, 1]), c))
        assert one["components"] == 1 and 0 < one["triangles"] <= whole["triangles"] and np.array_equal(one["component_edges"][0], whole["component_edges"][largest])
    finally:
        for handle in (f, h):
            if handle is not None:
                ctx.lib.rm_mesh_destroy(handle)
        scene.destroy()


# ---- 4: the depths of the reduction -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, triangles, levels", [(8, 404, 2), (48, 13852, 2), (160, 154448, 3)])
def test_reduction_depths_on_spheres(ctx, n, triangles, levels):
    lo, hi, nn, values = SR.sphere_field(n)
    h = from_values(ctx, nn, values, 0.0, lo, hi)
    try:
        m = check_measures(ctx, h)
        depth, groups = 0, triangles
        while True:
            groups, depth = (groups + 255) // 256, depth + 1
            if groups == 1:
                break
        assert m["triangles"] == triangles and depth == levels and m["closed"]
        # a vertex never leaves its cell: the surface lies between the spheres of radius r -+ h sqrt(3)
        r, cell = 0.8, 2.0 / n * math.sqrt(3.0)
        print(f"sphere n = {n}: volume {m['volume']:.6f} in [{4 / 3 * math.pi * (r - cell) ** 3:.4f}, {4 / 3 * math.pi * (r + cell) ** 3:.4f}], area {m['area']:.6f}")
        assert 4 / 3 * math.pi * (r - cell) ** 3 <= m["volume"] <= 4 / 3 * math.pi * (r + cell) ** 3
    finally:
        ctx.lib.rm_mesh_destroy(h)


# ---- 5: determinism, ownership, refusals -----------------------------------------------------------------------------------------------------------------

def test_three_fresh_handles_give_identical_bytes(ctx):
    lo, hi, n, values, iso = SR.fields()["noise 0.25"]()
    seen = set()
    for _ in range(3):
        h = from_values(ctx, n, values, iso, lo, hi)
        try:
            seen.add(measured(ctx, h)[1])
        finally:
            ctx.lib.rm_mesh_destroy(h)
    assert len(seen) == 1 and len(next(iter(seen))) > 160 + 32


def test_handle_level_refusals_and_order_of_calls(ctx, sources):
    lib = ctx.lib
    last = lambda: lib.rm_last_error(ctx.h).decode()
    lo, hi, n, values, iso = SR.fields()["two balls"]()
    h = from_values(ctx, n, values, iso, lo, hi)
    try:
        rows = np.full((3, 4), 7, np.uint64)
        p = rows.ctypes.data_as(C.c_void_p)
        for size in (0, 32, 63, 65, 96):  # the components entry measures a fresh mesh itself; C = 2
            assert lib.rm_mesh_measure_components(h, p, size) == INV and "exact size" in last() and last().startswith("rm_mesh_measure_components: ")
        assert lib.rm_mesh_measure_components(h, None, 64) == INV and last() == "rm_mesh_measure_components: NULL argument"
        assert (rows == 7).all()
        assert lib.rm_mesh_measure_components(h, p, 64) == OK and (rows[2] == 7).all() and rows[:2].tolist() == [[342, 0, 0, 0], [264, 0, 0, 0]]
        assert lib.rm_mesh_measure(h, None, None) == INV and last() == "rm_mesh_measure: NULL argument"
        m, _, ms = measured(ctx, h)  # made by the components entry already
        assert ms == [0.0, 0.0] and m["closed_components"] == 2
        assert measured(ctx, h, timed=False)[0]["edges"] == 606
    finally:
        lib.rm_mesh_destroy(h)
    a, b = from_values(ctx, n, values, iso, lo, hi), from_values(ctx, n, values, iso, lo, hi)
    try:
        parts(ctx, a)  # labelled before: the measure does not label again; b is labelled by the measure
        ma, blob_a, _ = measured(ctx, a)
        mb, blob_b, _ = measured(ctx, b)
        assert blob_a == blob_b
        la, lb = parts(ctx, a), parts(ctx, b)
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
    finally:
        lib.rm_mesh_destroy(a)
        lib.rm_mesh_destroy(b)


# ---- 6: the hosts ---------------------------------------------------------------------------------------------------------------------------------------------

HOST_GRID, HOST_CLUSTERS, HOST_ISO = M.Grid((-1.25,) * 3, (1.25,) * 3, (40, 40, 40)), M.Grid((-1.25,) * 3, (1.25,) * 3, (10, 10, 10)), 0.0078125


def test_python_host_returns_the_c_calls_struct(ctx, tmp_path):
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        h = from_scene(ctx, scene, HOST_GRID, iso=HOST_ISO)
        s = simplified(ctx, h, HOST_CLUSTERS)
        f = filtered(ctx, s, None)
        want, _, _ = measured(ctx, f)
        for handle in (f, s, h):
            ctx.lib.rm_mesh_destroy(handle)
        m = ctx.extract_mesh(scene, HOST_GRID, iso=HOST_ISO, simplify=HOST_CLUSTERS, keep=True, measures=True)
        assert QR.same(m.measures, want) == [] and m.measures["lo"] == want["lo"] and m.timings["measures"] > 0.0 and m.measures["triangles"] == len(m.triangles) > 0
        assert QR.same(m.measures, QR.measure(m.positions, m.triangles, *components_of(m))) == []
        plain = ctx.extract_mesh(scene, HOST_GRID, iso=HOST_ISO, simplify=HOST_CLUSTERS, keep=True)
        assert plain.measures is None and "measures" not in plain.timings and plain.positions.tobytes() == m.positions.tobytes()
        M.write_stl(m, tmp_path / "m.stl")
        normals, corners = QR.parse_stl((tmp_path / "m.stl").read_bytes())
        assert corners.tobytes() == m.positions[m.triangles.astype(np.int64)].tobytes() and np.isfinite(normals).all()
    finally:
        scene.destroy()
    lo, hi, n, values, iso = SR.fields()["two balls"]()
    m = ctx.mesh_from_values(M.Grid(lo, hi, n), values, iso, measures=True)
    assert m.measures["closed"] and m.measures["component_edges"].tolist() == [[342, 0, 0, 0], [264, 0, 0, 0]] and m.measures["euler"] == 4


def components_of(m):
    import mesh_parts_ref as PR

    labels, sizes = PR.components(m.vertices, m.triangles)
    return labels, len(sizes)


def test_node_host_returns_the_c_calls_struct(ctx, tmp_path):
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    flo, fhi, fn, values, fiso = SR.fields()["two balls"]()
    np.ascontiguousarray(values, "<f4").tofile(tmp_path / "field")
    g = HOST_GRID
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(tmp_path)!r};
const ctx = new r.RenderJobContext(0), sc = new r.Mandelbulb(), g = r.meshGrid({list(g.lo)}, {list(g.hi)}, {list(g.n)});
const clusters = r.meshGrid({list(g.lo)}, {list(g.hi)}, {list(HOST_CLUSTERS.n)});
const flat = (m) => JSON.stringify(m, (k, v) => v instanceof BigUint64Array ? Array.from(v, String) : v);
const m = ctx.extractMesh(sc, g, {{ iso: {HOST_ISO} }}, null, true, false, {{ grid: clusters }}, null, null, true);
if (m.timings.length !== 3 || !(m.measures.milliseconds[0] > 0) || "occlusion" in m) process.exit(3);
fs.writeFileSync(d + "/scene.json", flat(m.measures));
fs.writeFileSync(d + "/scene.stl", r.encodeStl(m));
const plain = ctx.extractMesh(sc, g, {{ iso: {HOST_ISO} }}, null, true, false, {{ grid: clusters }});
if ("measures" in plain) process.exit(4);
const raw = fs.readFileSync(d + "/field"), values = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);
const f = ctx.meshFromValues(r.meshGrid({list(flo)}, {list(fhi)}, {list(fn)}), values, {fiso}, null, false, null, null, true);
fs.writeFileSync(d + "/field.json", flat(f.measures));
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    import json

    names = dict(usedVertices="used_vertices", skippedTriangles="skipped_triangles", unmeasuredTriangles="unmeasured_triangles", finiteVertices="finite_vertices",
                 boundaryEdges="boundary_edges", regularEdges="regular_edges", irregularEdges="irregular_edges", unbalancedEdges="unbalanced_edges",
                 closedComponents="closed_components", componentEdges="component_edges")

    def as_python(path):
        raw = json.loads(path.read_text())
        assert len(raw.pop("milliseconds")) == 2
        got = {names.get(k, k): v for k, v in raw.items()}
        got["component_edges"] = np.array([int(x) for x in got["component_edges"]], np.uint64).reshape(-1, 4)
        return got

    scene = ctx.create_scene(S.Mandelbulb())
    try:
        want = ctx.extract_mesh(scene, g, iso=HOST_ISO, simplify=HOST_CLUSTERS, keep=True, measures=True)
    finally:
        scene.destroy()
    assert QR.same(as_python(tmp_path / "scene.json"), want.measures) == []  # (JSON carries a double's and a float's value exactly)
    assert (tmp_path / "scene.stl").read_bytes() == M.encode_stl(want)
    field = ctx.mesh_from_values(M.Grid(flo, fhi, fn), values, fiso, measures=True)
    assert QR.same(as_python(tmp_path / "field.json"), field.measures) == [] and field.measures["closed"]


# ---- one measurement, no bar ------------------------------------------------------------------------------------------------------------------

def test_measure_the_measures_on_the_mandelbulb_256_cubed(ctx):
    """Mandelbulb on 256^3 cells of [-1.25, 1.25]^3 at iso 2^-7 (the mesh of profiles/mesh_extraction.txt), strict build.  Warmed once, then five
    calls on fresh handles: median (min .. max) in milliseconds of the two slots of out_ms2 -- topology (with the labelling) and geometry.
    Beside it the host-clock time of the only earlier route: downloading the arrays and labels, and the numpy restatement on them.  The last
    handle's measures are checked against that restatement (this is also the large mesh's check).  No assertion on time."""
    lo, hi, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), 0.0078125
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        grid = M.Grid(lo, hi, (256, 256, 256))
        warm = from_scene(ctx, scene, grid, iso=iso, normals=False)
        measured(ctx, warm)
        ctx.lib.rm_mesh_destroy(warm)
        topology, geometry = [], []
        for run in range(5):
            h = from_scene(ctx, scene, grid, iso=iso, normals=False)
            got, _, ms = measured(ctx, h)
            topology.append(ms[0])
            geometry.append(ms[1])
            if run < 4:
                ctx.lib.rm_mesh_destroy(h)
        try:
            t0 = time.perf_counter()
            src = arrays(ctx, h)
            labels, sizes = parts(ctx, h)
            t1 = time.perf_counter()
            want = QR.measure(src["positions"], src["triangles"], labels, len(sizes))
            t2 = time.perf_counter()
        finally:
            ctx.lib.rm_mesh_destroy(h)
        print(f"\nmandelbulb 256^3 iso 2^-7 strict: {got['vertices']} vertices, {got['triangles']} triangles, {got['edges']} edges "
              f"({got['boundary_edges']} boundary, {got['irregular_edges']} irregular), {got['components']} components ({got['closed_components']} closed), "
              f"area {got['area']:.6f}, volume {got['volume']:.6f}")
        print(f"  rm_mesh_measure: topology {spread(topology)} ms, geometry {spread(geometry)} ms, median (min .. max) of 5 fresh handles")
        print(f"  download + numpy: {1e3 * (t1 - t0):.1f} ms download, {1e3 * (t2 - t1):.1f} ms restatement (host clock, once)")
        assert QR.same(got, want) == [] and all(x > 0.0 for x in topology + geometry)
    finally:
        scene.destroy()
