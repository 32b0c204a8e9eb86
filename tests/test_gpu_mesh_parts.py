"""Components and islands on the GPU: rm_mesh_components, rm_mesh_components_download and rm_mesh_filter against the numpy restatement
(tests/mesh_parts_ref.py) run on the downloaded source arrays.  Every comparison is exact: integers, and floats by their bits."""
import ctypes as C
import shutil
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import mesh_parts_ref as PR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import BOX_HI, BOX_LO, open_field, spread, table_with_surfaces
from test_mesh_cpu import read_ply, special_field

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
FAST, NO_CULL = abi.RM_RENDER_FAST, abi.RM_RENDER_NO_CULL
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID
ARRAYS = (("positions", abi.RM_MESH_POSITIONS, 3, F), ("normals", abi.RM_MESH_NORMALS, 3, F), ("colours", abi.RM_MESH_COLOURS, 3, F),
          ("triangles", abi.RM_MESH_TRIANGLES, 3, np.uint32), ("cells", abi.RM_MESH_CELLS, 0, np.uint32))


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


# ---- the C ABI, by hand: handles stay alive between the calls ------------------------------------------------------------------------------

def from_values(c, n, values, iso=0.0, lo=BOX_LO, hi=BOX_HI):
    h, g = C.c_void_p(), M.Grid(lo, hi, n).to_c()
    v = np.ascontiguousarray(values, F)
    assert c.lib.rm_mesh_from_values(c.h, C.byref(g), native._fp(v), float(iso), C.byref(h)) == OK, c.lib.rm_last_error(c.h)
    return h


def from_scene(c, scene, grid, sharp=False, **params):
    h, g, p = C.c_void_p(), grid.to_c(), M.mesh_params(**params)
    if sharp:
        rc = c.lib.rm_mesh_extract_sharp(c.h, scene.h, C.byref(g), C.byref(p), None, C.byref(h))
    else:
        rc = c.lib.rm_mesh_extract(c.h, scene.h, C.byref(g), C.byref(p), C.byref(h))
    assert rc == OK, c.lib.rm_last_error(c.h)
    return h


def counts(c, h):
    out = (C.c_ulonglong * 2)()
    assert c.lib.rm_mesh_counts(h, out) == OK
    return int(out[0]), int(out[1])


def arrays(c, h, normals=False, colours=False):
    """The mesh's arrays; normals / colours are None when the mesh was made without them (and then their download is refused)."""
    v, t = counts(c, h)
    out = {}
    for name, what, width, dtype in ARRAYS:
        rows = t if name == "triangles" else v
        a = np.empty((rows, width) if width else (rows,), dtype)
        absent = (name == "normals" and not normals) or (name == "colours" and not colours)
        rc = c.lib.rm_mesh_download(h, what, a.ctypes.data_as(C.c_void_p), a.nbytes)
        assert rc == (INV if absent else OK), (name, rc)
        out[name] = None if absent else a
    return out


def parts(c, h):
    count = C.c_ulonglong(1 << 40)
    assert c.lib.rm_mesh_components(h, C.byref(count)) == OK, c.lib.rm_last_error(c.h)
    v, _ = counts(c, h)
    labels, sizes = np.full(v, 0xFFFFFFFF, np.uint32), np.full((int(count.value), 2), 0xFFFFFFFF, np.uint32)
    assert c.lib.rm_mesh_components_download(h, abi.RM_MESH_PART_LABELS, labels.ctypes.data_as(C.c_void_p) if v else None, labels.nbytes) == OK
    assert c.lib.rm_mesh_components_download(h, abi.RM_MESH_PART_SIZES, sizes.ctypes.data_as(C.c_void_p) if len(sizes) else None, sizes.nbytes) == OK
    return labels, sizes


def filtered(c, h, rule):
    out = C.c_void_p()
    k = None if rule is None else C.byref(M.mesh_keep(**rule))
    assert c.lib.rm_mesh_filter(h, k, C.byref(out)) == OK, c.lib.rm_last_error(c.h)
    assert out.value
    return out


def same_arrays(got, want):
    """Shapes, dtypes and bytes of the five arrays; None matches None."""
    for name, _, _, dtype in ARRAYS:
        a, b = got[name], want[name]
        if a is None or b is None:
            assert a is None and b is None, name
            continue
        assert a.dtype == dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), name
    return True


def check_mesh(c, h, rules, normals=False, colours=False):
    """Labels, sizes and every filter of the mesh against the restatement on its downloaded arrays; the source is unchanged afterwards.
    Returns (source arrays, labels, sizes)."""
    src = arrays(c, h, normals, colours)
    v, t = counts(c, h)
    want_labels, want_sizes = PR.components(v, src["triangles"])
    labels, sizes = parts(c, h)
    assert labels.shape == want_labels.shape and sizes.shape == want_sizes.shape, (sizes.shape, want_sizes.shape)
    assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
    for rule in rules:
        f = filtered(c, h, rule)
        try:
            got = arrays(c, f, normals, colours)
            want = PR.filter_arrays(PR.keep_mask(want_sizes, **(rule or {})), want_labels, src["positions"], src["triangles"], src["cells"], src["normals"], src["colours"])
            assert same_arrays(got, want), rule
            ms = (C.c_float * 3)()
            assert c.lib.rm_mesh_timings(f, ms) == OK and ms[0] == 0.0 and ms[1] >= 0.0 and ms[2] == 0.0
            for name, what, _, _ in ARRAYS:  # the device pointers follow the arrays: NULL for an empty or absent one
                assert bool(c.lib.rm_mesh_device_ptr(f, what)) == (got[name] is not None and got[name].size > 0), name
        finally:
            c.lib.rm_mesh_destroy(f)
    assert same_arrays(arrays(c, h, normals, colours), src)  # the source is untouched
    again = parts(c, h)
    assert np.array_equal(again[0], labels) and np.array_equal(again[1], sizes)
    return src, labels, sizes


# ---- 1: meshes from values ---------------------------------------------------------------------------------------------------------------------

def one_cell():
    v = np.ones((2, 2, 2), F)
    v[0, 0, 0] = -1.0
    return (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (1, 1, 1), v, 0.0


FIELDS = {
    "empty": lambda: ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 4, 4), np.ones((5, 5, 5), F), 0.0),
    "one cell": one_cell,
    "two balls": lambda: PR.two_balls_field() + (0.0,),
    "snake": lambda: PR.snake_field() + (0.0,),
    "noise 1.5": lambda: PR.noise_field() + (1.5,),
    "noise 0.25": lambda: PR.noise_field() + (0.25,),
    "special": lambda: (BOX_LO, BOX_HI, (31, 33, 29), special_field((31, 33, 29), 11), 0.0),
    "open": lambda: (BOX_LO, BOX_HI, (31, 33, 29), open_field((31, 33, 29), 12), 0.0),
}


@pytest.mark.parametrize("name", list(FIELDS))
def test_labels_sizes_and_filters_of_a_field_are_the_restatement(ctx, name):
    lo, hi, n, values, iso = FIELDS[name]()
    h = from_values(ctx, n, values, iso, lo, hi)
    try:
        src, labels, sizes = check_mesh(ctx, h, [None] + PR.KEEP_CASES)
        v, t = counts(ctx, h)
        print(name, v, "vertices", t, "triangles", len(sizes), "components")
        if name == "empty":
            assert (v, t, len(sizes)) == (0, 0, 0)
        if name == "one cell":
            assert (v, t) == (1, 0) and sizes.tolist() == [[1, 0]] and labels.tolist() == [0]
            f = filtered(ctx, h, None)  # the defaults drop the unreferenced vertex: a valid empty mesh
            assert counts(ctx, f) == (0, 0) and all(ctx.lib.rm_mesh_download(f, what, None, 0) == OK for what in (0, 3, 4))
            assert parts(ctx, f)[1].shape == (0, 2)
            ctx.lib.rm_mesh_destroy(f)
        if name == "two balls":
            assert len(sizes) == 2
        if name == "snake":
            assert (v, t) == (1008, 2008) and sizes[:, 0].tolist() == [504, 504]
        if name == "noise 1.5":
            assert len(sizes) > 1000
        if name == "noise 0.25":
            assert v > 65536 and (sizes[:, 1] == 0).any()
    finally:
        ctx.lib.rm_mesh_destroy(h)


# ---- 2: meshes from scenes, in every arithmetic ------------------------------------------------------------------------------------------------

SCENE_CASES = [("table", table_with_surfaces, (24, 24, 24), (-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), dict(colours=True), False),
               ("table sharp", table_with_surfaces, (24, 24, 24), (-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), dict(colours=True), True),
               ("mandelbulb", lambda: S.Mandelbulb(), (64, 64, 64), (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), dict(iso=2.0 ** -7, normals=False), False),
               ("csg64", lambda: S.csg64(), (32, 32, 32), (-1.6, -1.4, -1.5), (1.5, 1.6, 1.45), dict(normals=True), False),
               ("csg64 no cull", lambda: S.csg64(), (32, 32, 32), (-1.6, -1.4, -1.5), (1.5, 1.6, 1.45), dict(normals=True, flags=NO_CULL), False)]
SCENE_RULES = [None, dict(largest=1), dict(min_triangles=13), dict(min_triangles=0, largest=3)]


@pytest.mark.parametrize("which", ["strict", "fast", "gl stack"])
def test_labels_sizes_and_filters_of_a_scene_are_the_restatement(ctx, gl_ctx, which):
    c, arithmetic = (gl_ctx, 0) if which == "gl stack" else (ctx, FAST if which == "fast" else 0)
    for name, make, n, lo, hi, params, sharp in SCENE_CASES:
        params = dict(params, flags=params.get("flags", 0) | arithmetic)
        normals, colours = params.get("normals", True), params.get("colours", False)
        scene = c.create_scene(make())
        h = None
        try:
            h = from_scene(c, scene, M.Grid(lo, hi, n), sharp, **params)
            src, labels, sizes = check_mesh(c, h, SCENE_RULES, normals, colours)
            assert len(src["positions"]) > 0 and (src["normals"] is not None) == bool(normals) and (src["colours"] is not None) == bool(colours)
            one = filtered(c, h, dict(largest=1))
            try:
                _, one_sizes = parts(c, one)
                big = int(np.flatnonzero(sizes[:, 1] == sizes[:, 1].max())[0])
                assert one_sizes.tolist() == [sizes[big].tolist()]  # one component, the largest, lowest index among equals
                rows = labels == big
                for key in ("normals", "colours"):  # the source's rows, bit for bit
                    if src[key] is not None:
                        assert arrays(c, one, normals, colours)[key].tobytes() == src[key][rows].tobytes(), (name, key)
            finally:
                c.lib.rm_mesh_destroy(one)
            if name == "mandelbulb":
                tri = np.sort(sizes[:, 1])[::-1]
                edges = [0, 1, 2, 4, 8, 16, 64, 256, 1024, 1 << 32]
                hist = {f"{a}..{b - 1}": int(((tri >= a) & (tri < b)).sum()) for a, b in zip(edges[:-1], edges[1:])}
                print(f"\nmandelbulb 64^3 iso 2^-7 {which}: {len(labels)} vertices, {int(tri.sum())} triangles, {len(tri)} components; largest {tri[:4].tolist()};"
                      f" components by triangle count {hist}")
        finally:
            if h is not None:
                c.lib.rm_mesh_destroy(h)
            scene.destroy()


# ---- 3: nothing depends on the order of arrival ------------------------------------------------------------------------------------------------

def test_five_runs_give_identical_bytes(ctx):
    lo, hi, n, values, iso = FIELDS["noise 1.5"]()
    seen = set()
    for _ in range(5):
        h = from_values(ctx, n, values, iso, lo, hi)
        try:
            labels, sizes = parts(ctx, h)
            blob = labels.tobytes() + sizes.tobytes()
            for rule in (dict(largest=5), dict(min_triangles=12)):
                f = filtered(ctx, h, rule)
                try:
                    got = arrays(ctx, f)
                    blob += b"".join(got[k].tobytes() for k in ("positions", "triangles", "cells"))
                finally:
                    ctx.lib.rm_mesh_destroy(f)
            seen.add(blob)
        finally:
            ctx.lib.rm_mesh_destroy(h)
    assert len(seen) == 1


# ---- 4: the cached labelling and the handles' lifetimes ----------------------------------------------------------------------------------------

def test_cache_and_lifetime(ctx):
    lo, hi, n, values, iso = FIELDS["noise 1.5"]()
    lib = ctx.lib
    a, b = from_values(ctx, n, values, iso, lo, hi), from_values(ctx, n, values, iso, lo, hi)
    first, second = C.c_ulonglong(), C.c_ulonglong()
    assert lib.rm_mesh_components(a, C.byref(first)) == OK and lib.rm_mesh_components(a, C.byref(second)) == OK and first.value == second.value > 1000
    rule = dict(min_triangles=13, largest=7)
    fa, fb = filtered(ctx, a, rule), filtered(ctx, b, rule)  # a is labelled already, b is fresh: the filter labels it itself
    assert same_arrays(arrays(ctx, fa), arrays(ctx, fb))
    ms_a, ms_b = (C.c_float * 3)(), (C.c_float * 3)()
    assert lib.rm_mesh_timings(fa, ms_a) == OK and lib.rm_mesh_timings(fb, ms_b) == OK
    assert ms_a[0] == ms_b[0] == 0.0 and ms_a[2] == ms_b[2] == 0.0 and ms_a[1] > 0.0 and ms_b[1] > 0.0
    # a filtered mesh is an ordinary mesh without a labelling of its own: its components are the restatement's on its arrays
    got = arrays(ctx, fa)
    labels, sizes = parts(ctx, fa)
    want_labels, want_sizes = PR.components(len(got["positions"]), got["triangles"])
    assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes) and len(sizes) == 7 and (sizes[:, 1] >= 13).all()
    twice = filtered(ctx, fa, rule)  # a kept component is kept whole
    assert same_arrays(arrays(ctx, twice), got)
    # destroy in either order: the source before what was filtered from it, and after
    lib.rm_mesh_destroy(a)
    assert same_arrays(arrays(ctx, fa), got) and np.array_equal(parts(ctx, fa)[0], labels)
    lib.rm_mesh_destroy(twice)
    lib.rm_mesh_destroy(fa)
    lib.rm_mesh_destroy(fb)
    lib.rm_mesh_destroy(b)


# ---- 5: the refusals at the handles -------------------------------------------------------------------------------------------------------------

def test_handle_level_refusals(ctx):
    lib = ctx.lib
    lo, hi, n, values, iso = FIELDS["two balls"]()
    last = lambda: lib.rm_last_error(ctx.h).decode()
    h = from_values(ctx, n, values, iso, lo, hi)
    try:
        v, t = counts(ctx, h)
        buf = np.zeros(4 * v + 64, np.uint8)
        p = buf.ctypes.data_as(C.c_void_p)
        for what in (-1, 2):  # an unknown array speaks before the size is looked at, and before anything is labelled
            assert lib.rm_mesh_components_download(h, what, p, 4 * v) == INV and last() == "rm_mesh_components_download: unknown array"
        assert lib.rm_mesh_components(h, None) == INV and last() == "rm_mesh_components: NULL argument"
        out = C.c_void_p()
        assert lib.rm_mesh_filter(h, None, None) == INV and last() == "rm_mesh_filter: NULL argument"
        assert lib.rm_mesh_filter(h, C.byref(abi.RmMeshKeep(-1, 0)), C.byref(out)) == INV and last().startswith("rm_mesh_filter: keep min_triangles")
        assert lib.rm_mesh_filter(h, C.byref(abi.RmMeshKeep(1, -1)), C.byref(out)) == INV and last().startswith("rm_mesh_filter: keep largest")
        assert lib.rm_mesh_filter(h, C.byref(abi.RmMeshKeep(1, 0, (C.c_int32 * 2)(0, 1))), C.byref(out)) == INV and last().startswith("rm_mesh_filter: keep reserved")
        count = C.c_ulonglong()
        assert lib.rm_mesh_components(h, C.byref(count)) == OK and count.value == 2
        for what, size in ((abi.RM_MESH_PART_LABELS, 4 * v), (abi.RM_MESH_PART_SIZES, 16)):
            assert lib.rm_mesh_components_download(h, what, p, size) == OK
            for wrong in (size - 1, size + 1, 0, size + 4, size - 4):
                assert lib.rm_mesh_components_download(h, what, p, wrong) == INV and "exact size" in last(), (what, wrong)
            assert lib.rm_mesh_components_download(h, what, None, size) == INV and last() == "rm_mesh_components_download: NULL argument"
        # the mesh's own arrays are still what/0..4
        assert lib.rm_mesh_download(h, 5, p, 4 * v) == INV and lib.rm_mesh_device_ptr(h, 5) is None
        assert lib.rm_mesh_download(h, abi.RM_MESH_CELLS, p, 4 * v) == OK
    finally:
        lib.rm_mesh_destroy(h)


# ---- 6: the hosts ---------------------------------------------------------------------------------------------------------------------------------

def as_arrays(m):
    return dict(positions=m.positions, normals=m.normals, colours=m.colours, triangles=m.triangles, cells=m.cells)


def test_python_host_equals_the_c_level_results(ctx):
    grid = M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (48, 48, 48))
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        h = from_scene(ctx, scene, grid, iso=2.0 ** -7, colours=True)
        f = filtered(ctx, h, dict(largest=1))
        want, (want_labels, want_sizes) = arrays(ctx, f, True, True), parts(ctx, f)
        source, (source_labels, source_sizes) = arrays(ctx, h, True, True), parts(ctx, h)
        ctx.lib.rm_mesh_destroy(f)
        ctx.lib.rm_mesh_destroy(h)
        assert len(source_sizes) > 1 and len(want_sizes) == 1
        plain = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True)
        assert same_arrays(as_arrays(plain), source) and plain.labels is None and plain.component_sizes is None
        for keep in (dict(largest=1), abi.RmMeshKeep(1, 1), M.mesh_keep(largest=1)):
            m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, keep=keep, components=True)
            assert same_arrays(as_arrays(m), want) and m.labels.dtype == np.uint32 and m.component_sizes.dtype == np.uint32
            assert np.array_equal(m.labels, want_labels) and np.array_equal(m.component_sizes, want_sizes) and m.component_sizes.shape == (1, 2)
            assert m.timings["sampling"] == 0.0 and m.timings["meshing"] > 0.0 and m.timings["attributes"] == 0.0 and m.grid is grid
        m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, components=True)  # components of the unfiltered mesh
        assert same_arrays(as_arrays(m), source) and np.array_equal(m.labels, source_labels) and np.array_equal(m.component_sizes, source_sizes)
        m = ctx.extract_mesh(scene, grid, iso=2.0 ** -7, colours=True, keep=dict(largest=1))
        assert same_arrays(as_arrays(m), want) and m.labels is None and m.component_sizes is None
        with pytest.raises(ValueError):
            ctx.extract_mesh(scene, grid, keep=dict(largest=-1))
        with pytest.raises(ValueError):
            ctx.extract_mesh(scene, grid, keep=3)
        with pytest.raises(RuntimeError, match="keep reserved"):
            ctx.extract_mesh(scene, grid, keep=abi.RmMeshKeep(1, 0, (C.c_int32 * 2)(1, 0)))
        with pytest.raises(TypeError):
            ctx.extract_mesh(scene, grid, 0.0, True, False, 0, 1e-5, None, True)  # keep is keyword-only
    finally:
        scene.destroy()
    lo, hi, n, values, iso = FIELDS["open"]()
    g = M.Grid(lo, hi, n)
    h = from_values(ctx, n, values, iso, lo, hi)
    f = filtered(ctx, h, None)
    want, (want_labels, want_sizes) = arrays(ctx, f), parts(ctx, f)
    ctx.lib.rm_mesh_destroy(f)
    ctx.lib.rm_mesh_destroy(h)
    m = ctx.mesh_from_values(g, values, iso, keep=True)
    assert same_arrays(as_arrays(m), want) and m.labels is None
    m = ctx.mesh_from_values(g, values, iso, keep=True, components=True)
    assert same_arrays(as_arrays(m), want) and np.array_equal(m.labels, want_labels) and np.array_equal(m.component_sizes, want_sizes)
    assert (m.component_sizes[:, 1] >= 1).all() and len(m.positions) < len(ctx.mesh_from_values(g, values, iso).positions)  # unreferenced vertices went


def test_node_host_gives_the_python_bytes(ctx, tmp_path):
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    lo, hi, n, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (40, 40, 40), 0.0078125
    flo, fhi, fn, values, fiso = FIELDS["noise 1.5"]()
    np.ascontiguousarray(values, "<f4").tofile(tmp_path / "field")
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(tmp_path)!r};
const ctx = new r.RenderJobContext(0), sc = new r.Mandelbulb(), g = r.meshGrid({list(lo)}, {list(hi)}, {list(n)});
const save = (name, a) => fs.writeFileSync(d + "/" + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const m = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, null, {{ largest: 1 }}, true);
for (const k of ["positions", "normals", "colours", "triangles", "cells", "labels", "componentSizes"]) save("scene_" + k, m[k]);
const plain = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }});
const kept = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, undefined, true);
if ("labels" in plain || "componentSizes" in plain || "labels" in kept || "componentSizes" in kept) process.exit(3);
if (m.timings[0] !== 0 || !(m.timings[1] > 0) || m.timings[2] !== 0 || !(plain.timings[0] > 0)) process.exit(4);
save("kept_positions", kept.positions);
const raw = fs.readFileSync(d + "/field"), values = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);
const fg = r.meshGrid({list(flo)}, {list(fhi)}, {list(fn)});
const f = ctx.meshFromValues(fg, values, {fiso}, {{ minTriangles: 12, largest: 5 }}, 1);
for (const k of ["positions", "triangles", "cells", "labels", "componentSizes"]) save("field_" + k, f[k]);
if (f.normals !== null || f.colours !== null || "labels" in ctx.meshFromValues(fg, values, {fiso})) process.exit(5);
let refused = 0;
for (const bad of [{{ largest: -1 }}, {{ minTriangles: 0.5 }}, {{ biggest: 1 }}, 7]) try {{ ctx.meshFromValues(fg, values, {fiso}, bad); }} catch (e) {{ refused++; }}
if (refused !== 4) process.exit(6);
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    h = ctx.create_scene(S.Mandelbulb())
    try:
        g = M.Grid(lo, hi, n)
        want = ctx.extract_mesh(h, g, iso=iso, colours=True, keep=dict(largest=1), components=True)
        assert want.vertices > 0 and len(want.component_sizes) == 1
        for k in ("positions", "normals", "colours", "triangles", "cells", "labels"):
            assert (tmp_path / ("scene_" + k)).read_bytes() == getattr(want, k).tobytes(), k
        assert (tmp_path / "scene_componentSizes").read_bytes() == want.component_sizes.tobytes()
        assert (tmp_path / "kept_positions").read_bytes() == ctx.extract_mesh(h, g, iso=iso, colours=True, keep=True).positions.tobytes()
    finally:
        h.destroy()
    want = ctx.mesh_from_values(M.Grid(flo, fhi, fn), values, fiso, keep=dict(min_triangles=12, largest=5), components=True)
    assert len(want.component_sizes) == 5
    for k in ("positions", "triangles", "cells", "labels"):
        assert (tmp_path / ("field_" + k)).read_bytes() == getattr(want, k).tobytes(), k
    assert (tmp_path / "field_componentSizes").read_bytes() == want.component_sizes.tobytes()


def test_ply_of_a_filtered_mesh_reads_back(ctx, tmp_path):
    h = ctx.create_scene(table_with_surfaces())
    try:
        m = ctx.extract_mesh(h, M.Grid((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), (27, 25, 23)), colours=True, keep=dict(largest=1))
    finally:
        h.destroy()
    assert m.vertices > 0 and len(m.triangles) > 0 and int(m.triangles.max()) < m.vertices
    M.write_ply(m, tmp_path / "kept.ply")
    for blob in ((tmp_path / "kept.ply").read_bytes(), M.encode_ply(m)):
        ply = read_ply(blob)
        assert np.stack([ply["vertex"][k] for k in "xyz"], -1).astype(F).tobytes() == m.positions.tobytes()
        assert np.stack([ply["vertex"][k] for k in ("nx", "ny", "nz")], -1).astype(F).tobytes() == m.normals.tobytes()
        assert np.array_equal(np.stack([ply["vertex"][k] for k in ("red", "green", "blue")], -1), M.colour_bytes(m.colours))
        assert np.array_equal(ply["face"], m.triangles)


# ---- one measurement, no bar ------------------------------------------------------------------------------------------------------------------

def test_measure_components_on_the_mandelbulb_256_cubed(ctx):
    """Mandelbulb on 256^3 cells of [-1.25, 1.25]^3 at iso 2^-7 (the mesh of test_gpu_mesh's measurement), strict and fast.  Warmed once, then
    five runs alternating the two; median (min .. max) in milliseconds of: the labelling rounds (rm_mesh_components on a fresh mesh, host
    clock: the rounds with the host's reads between them, the scan, the labels and the sizes); the filter's slot of rm_mesh_timings for
    largest = 1, on a fresh mesh (labelling + compaction) and on a labelled one (compaction alone); and on the host's clock
    extract_mesh(..., keep=dict(largest=1)) against extract_mesh(...) followed by the numpy restatement on the downloaded arrays (the
    restatement once per build: it takes seconds).  The two routes' arrays are compared, so this is also the large mesh's check.  No assertion
    on time."""
    lo, hi, n, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (256, 256, 256), 0.0078125
    g = M.Grid(lo, hi, n)
    scene = ctx.create_scene(S.Mandelbulb())
    builds = (("strict", 0), ("fast", FAST))
    rule = dict(largest=1)
    try:
        for _, flags in builds:  # warm: code objects, this shape, its allocations
            ctx.extract_mesh(scene, g, iso=iso, flags=flags, keep=rule, components=True)
        st = {name: dict(label=[], fresh=[], labelled=[], kept=[], plain=[]) for name, _ in builds}
        kept, plain = {}, {}
        for _ in range(5):
            for name, flags in builds:
                a, b = from_scene(ctx, scene, g, iso=iso, flags=flags), from_scene(ctx, scene, g, iso=iso, flags=flags)
                try:
                    count = C.c_ulonglong()
                    t = time.perf_counter()
                    assert ctx.lib.rm_mesh_components(a, C.byref(count)) == OK
                    st[name]["label"].append((time.perf_counter() - t) * 1e3)
                    ms = (C.c_float * 3)()
                    for h, key in ((b, "fresh"), (a, "labelled")):
                        f = filtered(ctx, h, rule)
                        assert ctx.lib.rm_mesh_timings(f, ms) == OK
                        st[name][key].append(float(ms[1]))
                        ctx.lib.rm_mesh_destroy(f)
                finally:
                    ctx.lib.rm_mesh_destroy(a)
                    ctx.lib.rm_mesh_destroy(b)
                t = time.perf_counter()
                kept[name] = ctx.extract_mesh(scene, g, iso=iso, flags=flags, keep=rule)
                st[name]["kept"].append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                plain[name] = ctx.extract_mesh(scene, g, iso=iso, flags=flags)
                st[name]["plain"].append((time.perf_counter() - t) * 1e3)
        for name, _ in builds:
            m = plain[name]
            t = time.perf_counter()
            labels, sizes = PR.components(m.vertices, m.triangles)
            want = PR.filter_arrays(PR.keep_mask(sizes, **rule), labels, m.positions, m.triangles, m.cells, m.normals, m.colours)
            restating = (time.perf_counter() - t) * 1e3
            s = st[name]
            print(f"\nmandelbulb 256^3 iso 2^-7 {name}: {m.vertices} vertices, {len(m.triangles)} triangles, {len(sizes)} components, the largest of "
                  f"{int(sizes[:, 1].max())} triangles; ms, median (min .. max) of 5 alternating runs\n"
                  f"  rm_mesh_components on a fresh mesh, host clock: {spread(s['label'])}\n"
                  f"  rm_mesh_filter largest = 1, its slot of rm_mesh_timings: labelling + compaction {spread(s['fresh'])}, compaction alone {spread(s['labelled'])}\n"
                  f"  host clock, arrays into numpy: extract_mesh(keep=largest 1) {spread(s['kept'])}; extract_mesh {spread(s['plain'])} + numpy restatement "
                  f"{restating:.0f} (once)")
            assert same_arrays(as_arrays(kept[name]), want)
            assert all(v >= 0.0 for key in ("fresh", "labelled") for v in s[key])
    finally:
        scene.destroy()
