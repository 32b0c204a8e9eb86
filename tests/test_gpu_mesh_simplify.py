"""Simplification on the GPU: rm_mesh_simplify against the numpy restatement (tests/mesh_simplify_ref.py) run on the downloaded source arrays.
Every comparison is exact: integers, and floats by their bits."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_parts_ref as PR
import mesh_simplify_ref as SR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import spread, table_with_surfaces
from test_gpu_mesh_parts import ARRAYS, arrays, as_arrays, counts, filtered, from_scene, from_values, parts, same_arrays
from test_mesh_cpu import read_ply

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


def simplified(c, h, grid, keep_duplicates=False):
    """rm_mesh_simplify of the handle on the mesh.Grid of clusters: the new handle"""
    out = C.c_void_p()
    g, p = M.mesh_simplify(grid, keep_duplicates)
    assert c.lib.rm_mesh_simplify(h, C.byref(g), C.byref(p), C.byref(out)) == OK, c.lib.rm_last_error(c.h)
    assert out.value
    return out


def restate(src, grid, keep_duplicates=False):
    m = SR.simplify(grid.lo, grid.hi, grid.n, src["positions"], src["triangles"], src["normals"], src["colours"], keep_duplicates=keep_duplicates)
    return {k: m[k] for k in ("positions", "normals", "colours", "triangles", "cells")}, m


def check_simplify(c, h, grid, normals=False, colours=False):
    """Both settings of keep_duplicates against the restatement of the handle's downloaded arrays; the source is unchanged afterwards.
    Returns the restatement's dict of the deduplicated mesh (with its counts)."""
    src = arrays(c, h, normals, colours)
    for keep in (False, True):
        s = simplified(c, h, grid, keep)
        try:
            got = arrays(c, s, normals, colours)
            want, full = restate(src, grid, keep)
            assert same_arrays(got, want), (grid.n, keep)
            ms = (C.c_float * 3)()
            assert c.lib.rm_mesh_timings(s, ms) == OK and ms[0] == 0.0 and ms[1] >= 0.0 and ms[2] == 0.0
            if len(src["positions"]):
                assert ms[1] > 0.0
            for name, what, _, _ in ARRAYS:  # the device pointers follow the arrays: NULL for an empty or absent one
                assert bool(c.lib.rm_mesh_device_ptr(s, what)) == (got[name] is not None and got[name].size > 0), name
            if not keep:
                first = full
        finally:
            c.lib.rm_mesh_destroy(s)
    assert same_arrays(arrays(c, h, normals, colours), src)  # the source is untouched
    return first


# ---- 1: meshes from values ---------------------------------------------------------------------------------------------------------------------

# what the issue measured of each row: (V', T', duplicates)
EXPECTED = {"noise 128": (65799, 184252, 0), "noise 20": (7999, 40191, 214), "noise 8 half": (512, 3808, 2263), "noise unequal": (41183, 125514, 84),
            "noise one": (1, 0, 0), "two balls 64": (206, 404, 0), "two balls one": (1, 0, 0), "snake 8 half": (138, 303, 93), "snake one": (1, 0, 0),
            "sphere 12": (420, 836, 0), "sphere 16": (780, 1556, 0)}


@pytest.fixture(scope="module")
def sources(ctx):
    """the source meshes of SR.CASES, made once: name -> (handle, field lo, field hi)"""
    made = {}
    for name, make in SR.fields().items():
        lo, hi, n, values, iso = make()
        made[name] = (from_values(ctx, n, values, iso, lo, hi), lo, hi)
    yield made
    for h, _, _ in made.values():
        ctx.lib.rm_mesh_destroy(h)


@pytest.mark.parametrize("case", list(SR.CASES))
def test_a_simplified_field_is_the_restatement(ctx, sources, case):
    field, lo, hi, n = SR.CASES[case]
    h, flo, fhi = sources[field]
    m = check_simplify(ctx, h, M.Grid(lo or flo, hi or fhi, n))
    print(case, counts(ctx, h), "->", len(m["positions"]), len(m["triangles"]), "duplicates", m["duplicates"], "collapsed", m["collapsed"])
    assert (len(m["positions"]), len(m["triangles"]), m["duplicates"]) == EXPECTED[case]


def test_empty_and_unreferenced_sources(ctx):
    grid = M.Grid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 4, 4))
    h = from_values(ctx, (4, 4, 4), np.ones((5, 5, 5), F), 0.0, grid.lo, grid.hi)  # no vertex at all
    try:
        for keep in (False, True):
            s = simplified(ctx, h, grid, keep)
            assert counts(ctx, s) == (0, 0) and all(ctx.lib.rm_mesh_download(s, what, None, 0) == OK for what in (0, 3, 4))
            assert parts(ctx, s)[1].shape == (0, 2)
            again = simplified(ctx, s, grid)
            assert counts(ctx, again) == (0, 0)
            ctx.lib.rm_mesh_destroy(again)
            ctx.lib.rm_mesh_destroy(s)
    finally:
        ctx.lib.rm_mesh_destroy(h)
    v = np.ones((2, 2, 2), F)
    v[0, 0, 0] = -1.0
    h = from_values(ctx, (1, 1, 1), v, 0.0, grid.lo, grid.hi)  # one vertex, no triangle
    try:
        assert counts(ctx, h) == (1, 0)
        m = check_simplify(ctx, h, grid)
        assert len(m["positions"]) == 1 and len(m["triangles"]) == 0
    finally:
        ctx.lib.rm_mesh_destroy(h)


# ---- 2: scenes with normals and colours -----------------------------------------------------------------------------------------------------------

SCENE_GRID = M.Grid((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), (32, 32, 32))
CLUSTER_GRIDS = [M.Grid(SCENE_GRID.lo, SCENE_GRID.hi, (8, 8, 8)), M.Grid(SCENE_GRID.lo, SCENE_GRID.hi, (5, 7, 3))]


@pytest.mark.parametrize("sharp", [False, True])
def test_a_simplified_scene_carries_mean_normals_and_colours(ctx, sharp):
    scene = ctx.create_scene(table_with_surfaces())
    h = bare = None
    try:
        h = from_scene(ctx, scene, SCENE_GRID, sharp, normals=True, colours=True)
        src = arrays(ctx, h, True, True)
        assert len(src["positions"]) > 1000 and src["normals"] is not None and src["colours"] is not None
        for grid in CLUSTER_GRIDS:
            m = check_simplify(ctx, h, grid, True, True)
            assert 0 < len(m["positions"]) < len(src["positions"]) / 4 and len(m["triangles"]) > 0
            lengths = np.linalg.norm(m["normals"].astype(np.float64), axis=1)
            assert ((np.abs(lengths - 1.0) < 1e-6) | (lengths == 0.0)).all()
            assert len(np.unique(m["colours"], axis=0)) > 3  # means across the three surfaces, not one surface's colour
        bare = from_scene(ctx, scene, SCENE_GRID, sharp, normals=False, colours=True)  # a source without normals gives a result without them
        m = check_simplify(ctx, bare, CLUSTER_GRIDS[0], False, True)
        assert m["normals"] is None and m["colours"] is not None
    finally:
        for handle in (h, bare):
            if handle is not None:
                ctx.lib.rm_mesh_destroy(handle)
        scene.destroy()


# ---- 3: composition with the other mesh entries ---------------------------------------------------------------------------------------------------

def test_simplify_then_filter_drops_exactly_the_orphaned_clusters(ctx, sources):
    h, lo, hi = sources["noise 0.25"]
    s = simplified(ctx, h, M.Grid(lo, hi, (37, 29, 53)))
    f = filtered(ctx, s, None)
    try:
        got, kept = arrays(ctx, s), arrays(ctx, f)
        used = np.zeros(len(got["positions"]), bool)
        used[got["triangles"].reshape(-1)] = True
        assert (~used).sum() == 37  # (a condition on the input: clusters that kept a vertex and lost every triangle)
        renumber = np.cumsum(used) - 1
        assert kept["positions"].tobytes() == got["positions"][used].tobytes() and kept["cells"].tobytes() == got["cells"][used].tobytes()
        assert np.array_equal(kept["triangles"], renumber[got["triangles"].astype(np.int64)].astype(np.uint32))
    finally:
        ctx.lib.rm_mesh_destroy(f)
        ctx.lib.rm_mesh_destroy(s)
    # the snake's tubes on clusters wider than a tube: every triangle collapses, every cluster is orphaned, the filter leaves a valid empty mesh
    h, lo, hi = sources["snake"]
    s = simplified(ctx, h, M.Grid(lo, hi, (3, 3, 1)))
    f = filtered(ctx, s, None)
    try:
        assert counts(ctx, s) == (9, 0) and counts(ctx, f) == (0, 0)
    finally:
        ctx.lib.rm_mesh_destroy(f)
        ctx.lib.rm_mesh_destroy(s)


def test_components_of_the_simplified_sphere(ctx, sources):
    h, lo, hi = sources["sphere"]
    for n in (12, 16):
        s = simplified(ctx, h, M.Grid(lo, hi, (n, n, n)))
        try:
            labels, sizes = parts(ctx, s)
            assert sizes.tolist() == [[EXPECTED[f"sphere {n}"][0], EXPECTED[f"sphere {n}"][1]]] and not labels.any()
            got = arrays(ctx, s)
            edges, uses = SR.edge_uses(got["triangles"])
            assert (uses == 2).all() and len(got["positions"]) - len(edges) + len(got["triangles"]) == 2
        finally:
            ctx.lib.rm_mesh_destroy(s)


def test_filtered_and_simplified_meshes_simplify_again(ctx, sources):
    h, lo, hi = sources["noise 0.25"]
    f = filtered(ctx, h, dict(largest=1))  # a filter's result is a source like any other
    try:
        assert 0 < counts(ctx, f)[0] < counts(ctx, h)[0]
        check_simplify(ctx, f, M.Grid(lo, hi, (20, 20, 20)))
    finally:
        ctx.lib.rm_mesh_destroy(f)
    s = simplified(ctx, h, M.Grid(lo, hi, (37, 29, 53)))  # ... and so is a simplified mesh, on a coarser grid unrelated to the first
    try:
        m = check_simplify(ctx, s, M.Grid((-0.9, -1.1, -1.0), (1.0, 0.95, 1.2), (9, 11, 7)))
        assert 0 < len(m["positions"]) <= 9 * 11 * 7 and len(m["triangles"]) > 0
    finally:
        ctx.lib.rm_mesh_destroy(s)


# ---- 4: nothing depends on the order of arrival ------------------------------------------------------------------------------------------------

def test_five_runs_give_identical_bytes(ctx, sources):
    h, lo, hi = sources["noise 0.25"]
    grid = M.Grid(lo, hi, (20, 20, 20))
    seen = set()
    for _ in range(5):
        blob = b""
        for keep in (False, True):
            s = simplified(ctx, h, grid, keep)
            try:
                got = arrays(ctx, s)
                blob += b"".join(got[k].tobytes() for k in ("positions", "triangles", "cells"))
            finally:
                ctx.lib.rm_mesh_destroy(s)
        seen.add(blob)
    assert len(seen) == 1
    scene = ctx.create_scene(table_with_surfaces())  # and with the attribute sums
    try:
        a = from_scene(ctx, scene, SCENE_GRID, normals=True, colours=True)
        seen = set()
        for _ in range(5):
            s = simplified(ctx, a, CLUSTER_GRIDS[1])
            got = arrays(ctx, s, True, True)
            seen.add(b"".join(got[k].tobytes() for k in ("positions", "normals", "colours", "triangles", "cells")))
            ctx.lib.rm_mesh_destroy(s)
        ctx.lib.rm_mesh_destroy(a)
        assert len(seen) == 1
    finally:
        scene.destroy()


# ---- 5: lifetimes and the refusals at the handles ---------------------------------------------------------------------------------------------------

def test_lifetime_and_handle_level_refusals(ctx):
    lib = ctx.lib
    lo, hi, n, values, iso = PR.two_balls_field() + (0.0,)
    last = lambda: lib.rm_last_error(ctx.h).decode()
    grid = M.Grid(lo, hi, (6, 6, 6))
    g, p = M.mesh_simplify(grid)
    h = from_values(ctx, n, values, iso, lo, hi)
    src = arrays(ctx, h)
    out = C.c_void_p(12345)
    assert lib.rm_mesh_simplify(h, C.byref(g), C.byref(p), None) == INV and last() == "rm_mesh_simplify: NULL argument"
    assert lib.rm_mesh_simplify(h, None, C.byref(p), C.byref(out)) == INV and last() == "rm_mesh_simplify: NULL grid" and out.value == 12345
    bad = grid.to_c()
    bad.n[2] = 0
    assert lib.rm_mesh_simplify(h, C.byref(bad), C.byref(p), C.byref(out)) == INV and last().startswith("rm_mesh_simplify: grid n must be")
    assert lib.rm_mesh_simplify(h, C.byref(g), C.byref(abi.RmMeshSimplify(2)), C.byref(out)) == INV and last() == "rm_mesh_simplify: keep_duplicates must be 0 or 1"
    assert lib.rm_mesh_simplify(h, C.byref(g), C.byref(abi.RmMeshSimplify(0, (C.c_int32 * 3)(0, 0, 1))), C.byref(out)) == INV
    assert last() == "rm_mesh_simplify: simplify reserved must be 0"
    assert lib.rm_mesh_simplify(h, C.byref(g), None, C.byref(out)) == OK and out.value not in (None, 12345)  # NULL params: the defaults
    s = out
    want, _ = restate(src, grid)
    assert same_arrays(arrays(ctx, s), want)
    assert same_arrays(arrays(ctx, h), src)  # the source is unchanged and still usable: labelled, filtered, simplified again
    assert parts(ctx, h)[1].shape == (2, 2)
    twice = simplified(ctx, h, grid)
    assert same_arrays(arrays(ctx, twice), want)
    lib.rm_mesh_destroy(h)  # the result outlives the source
    assert same_arrays(arrays(ctx, s), want) and same_arrays(arrays(ctx, twice), want)
    labels, sizes = parts(ctx, s)  # it starts without a labelling of its own, and gets one like any mesh
    want_labels, want_sizes = PR.components(len(want["positions"]), want["triangles"])
    assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
    # the result's own downloads refuse as any mesh's do
    buf = np.zeros(16, np.uint8)
    assert lib.rm_mesh_download(s, abi.RM_MESH_NORMALS, buf.ctypes.data_as(C.c_void_p), 0) == INV and "without this array" in last()
    assert lib.rm_mesh_download(s, abi.RM_MESH_CELLS, buf.ctypes.data_as(C.c_void_p), 3) == INV and "exact size" in last()
    lib.rm_mesh_destroy(twice)
    lib.rm_mesh_destroy(s)


# ---- 6: the hosts ---------------------------------------------------------------------------------------------------------------------------------

def test_python_host_equals_the_c_level_chain(ctx):
    grid, clusters = M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (48, 48, 48)), M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (12, 12, 12))
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        h = from_scene(ctx, scene, grid, iso=2.0 ** -7, colours=True)
        s = simplified(ctx, h, clusters)
        f = filtered(ctx, s, None)
        want, (want_labels, want_sizes), unfiltered = arrays(ctx, f, True, True), parts(ctx, f), arrays(ctx, s, True, True)
        for handle in (f, s, h):
            ctx.lib.rm_mesh_destroy(handle)
        assert 0 < len(want["positions"]) <= len(unfiltered["positions"]) < 12 ** 3
        for simplify in (clusters, dict(grid=clusters), dict(grid=clusters, keep_duplicates=False), M.mesh_simplify(clusters)):
            m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, simplify=simplify, keep=True, components=True)
            assert same_arrays(as_arrays(m), want) and np.array_equal(m.labels, want_labels) and np.array_equal(m.component_sizes, want_sizes)
            assert (m.grid.lo, m.grid.hi, m.grid.n) == (clusters.lo, clusters.hi, clusters.n)  # the cells index the cluster grid
            assert m.timings["sampling"] == 0.0 and m.timings["meshing"] > 0.0 and m.timings["attributes"] == 0.0
        m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, simplify=clusters)
        assert same_arrays(as_arrays(m), unfiltered) and m.labels is None and m.grid is clusters
        plain = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True)
        assert plain.grid is grid and len(plain.positions) > len(m.positions)
        for bad in (True, 3, dict(keep_duplicates=True), dict(grid=clusters, keep_duplicates=2), (clusters, True)):
            with pytest.raises(ValueError):
                ctx.extract_mesh(scene, grid, simplify=bad)
        with pytest.raises(RuntimeError, match="simplify reserved"):
            ctx.extract_mesh(scene, grid, simplify=(clusters.to_c(), abi.RmMeshSimplify(0, (C.c_int32 * 3)(1, 0, 0))))
    finally:
        scene.destroy()
    lo, hi, n, values, iso = PR.noise_field() + (0.25,)
    g, coarse = M.Grid(lo, hi, n), M.Grid(lo, hi, (20, 20, 20))
    h = from_values(ctx, n, values, iso, lo, hi)
    s = simplified(ctx, h, coarse, True)
    want = arrays(ctx, s)
    ctx.lib.rm_mesh_destroy(s)
    ctx.lib.rm_mesh_destroy(h)
    m = ctx.mesh_from_values(g, values, iso, simplify=dict(grid=coarse, keep_duplicates=True))
    assert same_arrays(as_arrays(m), want) and len(m.triangles) == 40191 + 214


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
const m = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, null, true, true, {{ grid: clusters }});
for (const k of ["positions", "normals", "colours", "triangles", "cells", "labels", "componentSizes"]) save("scene_" + k, m[k]);
const loose = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, undefined, undefined, undefined, {{ grid: clusters, keepDuplicates: true }});
if ("labels" in loose || !(loose.timings[1] > 0) || loose.timings[0] !== 0) process.exit(3);
save("loose_triangles", loose.triangles);
const raw = fs.readFileSync(d + "/field"), values = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);
const fg = r.meshGrid({list(flo)}, {list(fhi)}, {list(fn)}), coarse = r.meshGrid({list(flo)}, {list(fhi)}, [20, 20, 20]);
const f = ctx.meshFromValues(fg, values, {fiso}, null, false, {{ grid: coarse }});
for (const k of ["positions", "triangles", "cells"]) save("field_" + k, f[k]);
if (f.normals !== null || f.colours !== null || "labels" in f) process.exit(5);
let refused = 0;
for (const bad of [{{ }}, {{ grid: coarse, keepDuplicates: 2 }}, {{ grid: coarse, dedupe: 1 }}, 7, {{ grid: {{ lo: [0, 0, 0], hi: [1, 1, 1], n: [0, 1, 1] }} }}])
  try {{ ctx.meshFromValues(fg, values, {fiso}, null, false, bad); }} catch (e) {{ refused++; }}
if (refused !== 5) process.exit(6);
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    h = ctx.create_scene(S.Mandelbulb())
    try:
        g, clusters = M.Grid(lo, hi, n), M.Grid(lo, hi, (10, 10, 10))
        want = ctx.extract_mesh(h, g, iso=iso, colours=True, simplify=clusters, keep=True, components=True)
        assert want.vertices > 0 and len(want.triangles) > 0
        for k in ("positions", "normals", "colours", "triangles", "cells", "labels"):
            assert (tmp_path / ("scene_" + k)).read_bytes() == getattr(want, k).tobytes(), k
        assert (tmp_path / "scene_componentSizes").read_bytes() == want.component_sizes.tobytes()
        loose = ctx.extract_mesh(h, g, iso=iso, colours=True, simplify=dict(grid=clusters, keep_duplicates=True))
        assert (tmp_path / "loose_triangles").read_bytes() == loose.triangles.tobytes()
    finally:
        h.destroy()
    want = ctx.mesh_from_values(M.Grid(flo, fhi, fn), values, fiso, simplify=M.Grid(flo, fhi, (20, 20, 20)))
    assert (want.vertices, len(want.triangles)) == (7999, 40191)
    for k in ("positions", "triangles", "cells"):
        assert (tmp_path / ("field_" + k)).read_bytes() == getattr(want, k).tobytes(), k


def test_ply_of_a_simplified_mesh_reads_back(ctx, tmp_path):
    h = ctx.create_scene(table_with_surfaces())
    try:
        m = ctx.extract_mesh(h, SCENE_GRID, colours=True, simplify=CLUSTER_GRIDS[0], keep=True)
    finally:
        h.destroy()
    assert m.vertices > 0 and len(m.triangles) > 0 and int(m.triangles.max()) < m.vertices
    M.write_ply(m, tmp_path / "light.ply")
    for blob in ((tmp_path / "light.ply").read_bytes(), M.encode_ply(m)):
        ply = read_ply(blob)
        assert np.stack([ply["vertex"][k] for k in "xyz"], -1).astype(F).tobytes() == m.positions.tobytes()
        assert np.stack([ply["vertex"][k] for k in ("nx", "ny", "nz")], -1).astype(F).tobytes() == m.normals.tobytes()
        assert np.array_equal(np.stack([ply["vertex"][k] for k in ("red", "green", "blue")], -1), M.colour_bytes(m.colours))
        assert np.array_equal(ply["face"], m.triangles)


# ---- one measurement, no bar ------------------------------------------------------------------------------------------------------------------

def test_measure_simplify_on_the_mandelbulb_256_cubed(ctx):
    """Mandelbulb on 256^3 cells of [-1.25, 1.25]^3 at iso 2^-7 (the mesh of test_gpu_mesh's measurement), strict build, clustered at 64^3 and
    128^3 with and without duplicates.  The extraction and each setting are warmed once, then five runs: median (min .. max) in milliseconds of rm_mesh_simplify's
    slot of rm_mesh_timings (its kernels between events on the stream), beside the source call's own sampling and meshing milliseconds.  The
    counts are checked against the restatement's at 64^3 (the arrays too: this is also the large mesh's check).  No assertion on time."""
    lo, hi, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), 0.0078125
    scene = ctx.create_scene(S.Mandelbulb())
    h = None
    try:
        ctx.lib.rm_mesh_destroy(from_scene(ctx, scene, M.Grid(lo, hi, (256, 256, 256)), iso=iso, normals=False))  # warm: the scene's grid, the code objects
        h = from_scene(ctx, scene, M.Grid(lo, hi, (256, 256, 256)), iso=iso, normals=False)
        v, t = counts(ctx, h)
        ms = (C.c_float * 3)()
        assert ctx.lib.rm_mesh_timings(h, ms) == OK
        print(f"\nmandelbulb 256^3 iso 2^-7 strict: {v} vertices, {t} triangles; the source call's sampling {ms[0]:.3f} ms, meshing {ms[1]:.3f} ms")
        for n in (64, 128):
            grid = M.Grid(lo, hi, (n, n, n))
            for keep in (False, True):
                ctx.lib.rm_mesh_destroy(simplified(ctx, h, grid, keep))  # warm: code objects, this shape, its allocations
                times, after = [], None
                for _ in range(5):
                    s = simplified(ctx, h, grid, keep)
                    assert ctx.lib.rm_mesh_timings(s, ms) == OK
                    times.append(float(ms[1]))
                    after = counts(ctx, s)
                    if n == 64 and len(times) == 5:
                        got = arrays(ctx, s)
                    ctx.lib.rm_mesh_destroy(s)
                print(f"  clusters {n}^3, keep_duplicates {int(keep)}: {v} -> {after[0]} vertices, {t} -> {after[1]} triangles; rm_mesh_simplify "
                      f"{spread(times)} ms, median (min .. max) of 5")
                assert all(x > 0.0 for x in times)
                if n == 64:
                    want, _ = restate(arrays(ctx, h), grid, keep)
                    assert same_arrays(got, want)
    finally:
        if h is not None:
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()
