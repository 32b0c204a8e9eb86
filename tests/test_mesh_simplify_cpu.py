"""Simplification without a GPU: the ABI of rm_mesh_simplify_default / rm_mesh_simplify, every refusal that is made before the handles are looked
at, the two hosts' packing of RmMeshSimplify and of the cluster grid, and the numpy restatement (tests/mesh_simplify_ref.py) on the meshes the GPU
tests use.  The numbers asserted on the restatement are conditions on those inputs: a changed input cannot quietly empty a test."""
import ctypes as C
import json
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_ref as MR
import mesh_simplify_ref as SR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
ENTRY_POINTS = ("rm_mesh_simplify_default", "rm_mesh_simplify")
F = np.float32


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshSimplify",) + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported


def test_defaults_and_struct_layout():
    lib = native.load_library()
    p = abi.RmMeshSimplify(keep_duplicates=7, reserved=(C.c_int32 * 3)(5, 6, 7))
    lib.rm_mesh_simplify_default(C.byref(p))
    lib.rm_mesh_simplify_default(None)  # a no-op
    assert (p.keep_duplicates, list(p.reserved)) == (0, [0, 0, 0])
    grid = M.Grid((-1, -1, -1), (1, 1, 1), (4, 4, 4))
    assert bytes(p) == bytes(M.mesh_simplify(grid)[1]) == bytes(16) and abi.MESH_SIMPLIFY_DEFAULTS == dict(keep_duplicates=0)
    assert C.sizeof(abi.RmMeshSimplify) == 16
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\n'
                       'int main(void){ printf("%zu %zu %zu %zu %zu\\n", sizeof(RmMeshSimplify), offsetof(RmMeshSimplify, keep_duplicates), '
                       'offsetof(RmMeshSimplify, reserved), sizeof(RmGrid), sizeof(RmMeshKeep)); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 0, 4, 40, 16]
    assert [abi.RmMeshSimplify.keep_duplicates.offset, abi.RmMeshSimplify.reserved.offset] == [0, 4]


# ---- the refusals made before the handles are looked at --------------------------------------------------------------------------------------

def c_grid(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), n=(8, 8, 8), reserved=0):
    return abi.RmGrid(lo=(C.c_float * 3)(*lo), hi=(C.c_float * 3)(*hi), n=(C.c_int32 * 3)(*n), reserved=reserved)


def c_params(keep_duplicates=0, reserved=(0, 0, 0)):
    return abi.RmMeshSimplify(keep_duplicates=keep_duplicates, reserved=(C.c_int32 * 3)(*reserved))


BAD_GRIDS = [(dict(n=(0, 8, 8)), "grid n must be"), (dict(n=(8, 8, 1025)), "grid n must be"), (dict(lo=(float("nan"), -1, -1)), "grid lo and hi must be finite"),
             (dict(hi=(1, float("inf"), 1)), "grid lo and hi must be finite"), (dict(lo=(1, -1, -1)), "grid cell size"), (dict(lo=(-3e38, -1, -1), hi=(3e38, 1, 1)), "grid cell size"),
             (dict(n=(1024, 1024, 1024)), "grid must have at most 2^28 corners"), (dict(reserved=1), "grid reserved must be 0")]


def test_every_refusal_speaks_before_the_handles_and_in_order():
    """No mesh exists without a GPU: every call ends in RM_ERR_INVALID, and the text (rm_last_error(NULL)) tells which check spoke."""
    lib = native.load_library()
    out = C.c_void_p()
    last = lambda: lib.rm_last_error(None).decode()
    inv = abi.RM_ERR_INVALID
    for o in (C.byref(out), None):
        # the grid speaks first: before a bad keep_duplicates, a bad reserved and the NULL handles
        for p in (None, C.byref(c_params()), C.byref(c_params(2, (1, 1, 1)))):
            assert lib.rm_mesh_simplify(None, None, p, o) == inv and last() == "rm_mesh_simplify: NULL grid"
            for fields, text in BAD_GRIDS:
                assert lib.rm_mesh_simplify(None, C.byref(c_grid(**fields)), p, o) == inv and last().startswith("rm_mesh_simplify: " + text), (fields, last())
        # then keep_duplicates, before reserved
        for bad in (2, -1, 1 << 30, -(1 << 31)):
            for reserved in ((0, 0, 0), (1, 0, 0), (0, 0, -1)):
                assert lib.rm_mesh_simplify(None, C.byref(c_grid()), C.byref(c_params(bad, reserved)), o) == inv
                assert last() == "rm_mesh_simplify: keep_duplicates must be 0 or 1", (bad, reserved, last())
        # then reserved, each of the three words
        for reserved in ((1, 0, 0), (0, -1, 0), (0, 0, 7), (1, 2, 3)):
            for dup in (0, 1):
                assert lib.rm_mesh_simplify(None, C.byref(c_grid()), C.byref(c_params(dup, reserved)), o) == inv
                assert last() == "rm_mesh_simplify: simplify reserved must be 0", (reserved, last())
        # good blocks, and NULL params (the defaults): the NULL handles are what is refused
        for p in (None, C.byref(c_params()), C.byref(c_params(1))):
            for g in (c_grid(), c_grid(n=(1, 1, 1)), c_grid(n=(1024, 3, 5)), c_grid(lo=(-0.5, 0.0, 3.0), hi=(0.5, 1e-3, 1e6), n=(37, 29, 53))):
                assert lib.rm_mesh_simplify(None, C.byref(g), p, o) == inv and last() == "rm_mesh_simplify: NULL argument"
    # the mesh entries beside it are as they were
    assert lib.rm_mesh_filter(None, None, C.byref(out)) == inv and last() == "rm_mesh_filter: NULL argument"
    assert lib.rm_mesh_filter(None, C.byref(abi.RmMeshKeep(-1, 0)), C.byref(out)) == inv and last().startswith("rm_mesh_filter: keep min_triangles")
    assert lib.rm_mesh_download(None, 0, None, 0) == inv and last() == "rm_mesh_download: NULL mesh"
    count = C.c_ulonglong(77)
    assert lib.rm_mesh_components(None, C.byref(count)) == inv and last() == "rm_mesh_components: NULL argument" and count.value == 77


# ---- the hosts -------------------------------------------------------------------------------------------------------------------------------------

GRID = M.Grid((-1.0, -0.5, 0.25), (1.0, 0.75, 2.0), (8, 9, 10))


@pytest.mark.parametrize("bad", [dict(grid=None), dict(grid=(8, 8, 8)), dict(grid=GRID.to_c()), dict(grid=GRID, keep_duplicates=2), dict(grid=GRID, keep_duplicates=-1),
                                 dict(grid=GRID, keep_duplicates=0.0), dict(grid=GRID, keep_duplicates="1"), dict(grid=GRID, keep_duplicates=None)])
def test_python_refuses_bad_simplify_parameters(bad):
    with pytest.raises(ValueError):
        M.mesh_simplify(**bad)


def test_python_packs_what_it_is_given():
    g, p = M.mesh_simplify(GRID)
    assert isinstance(g, abi.RmGrid) and isinstance(p, abi.RmMeshSimplify) and bytes(g) == bytes(GRID.to_c()) and bytes(p) == bytes(16)
    for yes in (True, 1, np.int64(1), np.uint8(1)):
        assert bytes(M.mesh_simplify(GRID, keep_duplicates=yes)[1]) == np.array([1, 0, 0, 0], "<i4").tobytes()
    # the host's own conversion of `simplify`: a grid, a dict and the pair say the same thing; anything else is refused
    to_c = native.Context._mesh_simplify
    assert to_c(None) is None
    for given, dup in ((GRID, 0), (dict(grid=GRID), 0), (dict(grid=GRID, keep_duplicates=True), 1), (M.mesh_simplify(GRID), 0), (M.mesh_simplify(GRID, True), 1)):
        grid, g, p = to_c(given)
        assert isinstance(grid, M.Grid) and (grid.lo, grid.hi, grid.n) == (GRID.lo, GRID.hi, GRID.n)
        assert bytes(g) == bytes(GRID.to_c()) and bytes(p) == np.array([dup, 0, 0, 0], "<i4").tobytes()
    reserved = abi.RmMeshSimplify(0, (C.c_int32 * 3)(0, 1, 0))  # left for the library to refuse
    assert bytes(to_c((GRID.to_c(), reserved))[2]) == bytes(reserved)
    bad_grid = GRID.to_c()
    bad_grid.n[1] = 0
    for bad in (True, 3, "grid", [GRID], (GRID, True), dict(), dict(keep_duplicates=True), dict(grid=GRID, keepDuplicates=True), dict(grid=GRID, keep_duplicates=2),
                (GRID.to_c(), abi.RmMeshSimplify(2)), (bad_grid, abi.RmMeshSimplify(0))):
        with pytest.raises(ValueError):
            to_c(bad)
    # the mesh of the Python host gained no field
    names = [f for f in M.Mesh.__dataclass_fields__]
    assert names[names.index("timings") + 1:] == ["labels", "component_sizes"]


def test_node_packs_the_simplify_block_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    grid = dict(lo=list(GRID.lo), hi=list(GRID.hi), n=list(GRID.n))
    cases = [dict(grid=grid), dict(grid=grid, keepDuplicates=True), dict(grid=grid, keepDuplicates=0), dict(grid=grid, keepDuplicates=1)]
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const g = %s;
const out = { size: r.addon.sizes().RmMeshSimplify, defaults: r.MESH_SIMPLIFY_DEFAULTS, made: r.meshSimplify({ grid: g }), cases: [], bad: [],
              keep: r.meshKeep(), sharp: r.meshSharp(),
              fns: [typeof r.meshSimplify, typeof r.addon.meshSimplifyBlock, typeof r.RenderJobContext.prototype.extractMesh, typeof r.RenderJobContext.prototype.meshFromValues],
              arity: [r.RenderJobContext.prototype.extractMesh.length, r.RenderJobContext.prototype.meshFromValues.length] };
for (const c of %s) { const b = r.addon.meshSimplifyBlock(r.meshSimplify(c)); out.cases.push([hex(b.grid), hex(b.params)]); }
for (const f of [() => r.meshSimplify(), () => r.meshSimplify(null), () => r.meshSimplify(true), () => r.meshSimplify({}), () => r.meshSimplify({ keepDuplicates: true }),
                 () => r.meshSimplify({ grid: g, keepDuplicates: 2 }), () => r.meshSimplify({ grid: g, keepDuplicates: "1" }), () => r.meshSimplify({ grid: g, keepDuplicates: null }),
                 () => r.meshSimplify({ grid: g, keep_duplicates: 1 }), () => r.meshSimplify({ grid: g, reserved: 0 }), () => r.meshSimplify({ grid: { lo: g.lo, hi: g.hi, n: [0, 1, 1] } }),
                 () => r.meshSimplify({ grid: { lo: g.hi, hi: g.lo, n: g.n } }), () => r.meshSimplify({ grid: [8, 8, 8] }), () => r.addon.meshSimplifyBlock(null),
                 () => r.addon.meshSimplifyBlock({ keepDuplicates: 1 })])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(JS / "index.js"), json.dumps(grid), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 16 and all(out["bad"]), out["bad"]
    assert out["fns"] == ["function"] * 4
    assert out["arity"] == [6, 2]  # the new parameters are appended behind the counted ones
    assert out["defaults"] == dict(keepDuplicates=0) and out["made"] == dict(grid=grid, keepDuplicates=0)
    assert out["keep"] == dict(minTriangles=1, largest=0) and out["sharp"] == dict(refine=6, normalDelta=2.0 ** -10, threshold=0.1)  # as they were
    for c, (got_grid, got_params) in zip(cases, out["cases"]):
        g, p = M.mesh_simplify(GRID, keep_duplicates=bool(c.get("keepDuplicates", False)))
        assert got_grid == bytes(g).hex() and got_params == bytes(p).hex(), c
    dts = (JS / "index.d.ts").read_text()
    assert "export function meshSimplify(" in dts and "export interface MeshSimplify " in dts and "simplify: MeshSimplify | null" in dts


# ---- the restatement on the meshes the GPU tests use ---------------------------------------------------------------------------------------

def source(name):
    """the surface-nets mesh (tests/mesh_ref.py) of a shared field: (lo, hi, positions, triangles, cells)"""
    if name not in source.store:
        lo, hi, n, values, iso = SR.fields()[name]()
        source.store[name] = (lo, hi) + MR.surface_nets(lo, hi, n, values, iso)
    return source.store[name]


source.store = {}


def restated(case, keep_duplicates=False):
    field, lo, hi, n = SR.CASES[case]
    flo, fhi, pos, tri, _ = source(field)
    lo, hi = lo or flo, hi or fhi
    return (lo, hi, n), SR.simplify(lo, hi, n, pos, tri, keep_duplicates=keep_duplicates)


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F)))


def check_simplified(case, vertices, triangles, duplicates):
    """the counts the issue measured, and what holds of every simplified mesh"""
    (lo, hi, n), m = restated(case)
    pos, tri, cells = m["positions"], m["triangles"], m["cells"]
    assert pos.dtype == F and tri.dtype == np.uint32 and cells.dtype == np.uint32 and m["normals"] is None and m["colours"] is None
    assert (len(pos), len(tri), m["duplicates"]) == (vertices, triangles, duplicates), (case, len(pos), len(tri), m["duplicates"])
    assert len(cells) == len(pos) and (np.diff(cells.astype(np.int64)) > 0).all() and int(cells.max()) < n[0] * n[1] * n[2]  # ascending key, strictly
    low, high = SR.box_of(lo, hi, n, cells)
    assert (pos >= low - ulp(low)).all() and (pos <= high + ulp(high)).all()  # inside its cluster cell's closed box
    if len(tri):
        assert int(tri.max()) < len(pos)
        assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 0] != tri[:, 2]).all()
        assert len(np.unique(SR.canonical(tri), axis=0)) == len(tri)  # no two alike
    _, kept = restated(case, keep_duplicates=True)
    assert len(kept["triangles"]) == triangles + duplicates and kept["positions"].tobytes() == pos.tobytes() and kept["cells"].tobytes() == cells.tobytes()
    # the kept ones are the first of their kind, in source order: dropping the later repeats of the long list gives the short one
    _, first = np.unique(SR.canonical(kept["triangles"]), axis=0, return_index=True)
    assert kept["triangles"][np.sort(first)].tobytes() == tri.tobytes()
    return m


def test_restatement_noise_fields():
    _, _, pos, tri, _ = source("noise 0.25")
    assert (len(pos), len(tri)) == (66175, 185110)
    m = check_simplified("noise 128", 65799, 184252, 0)
    assert len(m["positions"]) > 65536  # more occupied clusters than two scan levels number
    check_simplified("noise 20", 7999, 40191, 214)
    check_simplified("noise unequal", 41183, 125514, 84)
    m = check_simplified("noise 8 half", 512, 3808, 2263)
    key, q, _ = SR.cluster_keys((-0.5,) * 3, (0.5,) * 3, (8, 8, 8), pos)
    assert np.bincount(key).max() == 2077  # one cluster holds that many vertices
    outside = np.abs(pos) > 0.5
    assert outside.any(axis=1).sum() > 10000  # most vertices lie outside the cluster grid ...
    assert (q[outside & (pos < 0)] == 0).all() and (q[outside & (pos > 0)] == 1 << 20).all()  # ... and count as lying on its boundary cells' outer faces
    assert ((q >= 0) & (q <= 1 << 20)).all()


@pytest.mark.parametrize("field", ["noise 0.25", "two balls", "snake"])
def test_restatement_one_cluster_collapses_everything(field):
    _, _, pos, tri, _ = source(field)
    case = {"noise 0.25": "noise one", "two balls": "two balls one", "snake": "snake one"}[field]
    m = check_simplified(case, 1, 0, 0)
    assert m["collapsed"] == len(tri) and m["cells"].tolist() == [0]


def test_restatement_identity_on_a_finer_grid():
    _, _, pos, tri, _ = source("two balls")
    assert (len(pos), len(tri)) == (206, 404)
    m = check_simplified("two balls 64", 206, 404, 0)
    assert m["collapsed"] == 0
    # no two vertices share a cluster, and the keys ascend with the source's order here: the triangles are the source's own
    key, _, _ = SR.cluster_keys((-1,) * 3, (1,) * 3, (64, 64, 64), pos)
    order = np.argsort(key, kind="stable")
    renumber = np.empty(len(pos), np.int64)
    renumber[order] = np.arange(len(pos))
    assert np.array_equal(m["triangles"], renumber[tri.astype(np.int64)].astype(np.uint32))
    assert np.abs(m["positions"].astype(np.float64) - pos[order].astype(np.float64)).max() < 2.0 ** -20 * (2.0 / 64) + 1e-7  # the Q20 rounding of a cell


def test_restatement_snake_is_a_thin_tube():
    _, _, pos, tri, _ = source("snake")
    assert (len(pos), len(tri)) == (1008, 2008)
    check_simplified("snake 8 half", 138, 303, 93)


@pytest.mark.parametrize("case,vertices,triangles", [("sphere 12", 420, 836), ("sphere 16", 780, 1556)])
def test_restatement_sphere_stays_a_sphere(case, vertices, triangles):
    _, _, pos, tri, _ = source("sphere")
    assert (len(pos), len(tri)) == (6928, 13852)
    m = check_simplified(case, vertices, triangles, 0)
    edges, uses = SR.edge_uses(m["triangles"])
    assert (uses == 2).all()  # closed and manifold along every edge
    assert vertices - len(edges) + triangles == 2  # Euler characteristic of a sphere
    n = SR.CASES[case][3][0]
    diagonal = np.sqrt(3.0) * 2.0 / n
    off = np.abs(np.linalg.norm(m["positions"].astype(np.float64) - (0.03, -0.02, 0.01), axis=1) - 0.8)
    print(case, "largest distance to the sphere", float(off.max()), "cluster cell diagonal", diagonal)
    assert off.max() < diagonal


def test_restatement_attributes():
    """normals are renormalised means, colours plain means; non-finite components count as 0 and large ones are clamped"""
    pos = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.1, 0.2], [0.9, 0.9, 0.9], [0.6, 0.1, 0.1]], F)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [np.nan, np.inf, 0], [1, 0, 0], [1, 0, 0]], F)
    nrm[3], nrm[4] = (0, 0, 0), (3e38, 0, 0)
    col = np.array([[0.25, 0.5, 1.0], [0.75, 0.5, 0.0], [0.5, -np.inf, 2000.0], [0.125, 0.25, 0.375], [-5000.0, 0.0, 1.0]], F)
    tri = np.array([[0, 1, 2], [0, 3, 4], [3, 4, 0], [4, 3, 0], [0, 3, 3]], np.uint32)
    m = SR.simplify((0, 0, 0), (1, 1, 1), (2, 2, 2), pos, tri, nrm, col)
    assert m["cells"].tolist() == [0, 1, 7] and m["normals"].dtype == F and m["colours"].dtype == F
    r = F(1.0) / np.sqrt(F(2.0))
    third = F(np.float64(1 << 20) / (3.0 * (1 << 20)))
    assert np.allclose(m["normals"][0], (r, r, 0), atol=1e-6) and m["normals"][1].tolist() == [1.0, 0.0, 0.0] and m["normals"][2].tolist() == [0.0, 0.0, 0.0]
    assert m["colours"][0].tolist() == [0.5, third, F(np.float64((1 << 20) + (1024 << 20)) / (3.0 * (1 << 20)))]
    assert m["colours"][1].tolist() == [-1024.0, 0.0, 1.0] and np.array_equal(m["colours"][2], col[3])
    # (0, 1, 2) collapses; (0, 3, 4) -> (0, 2, 1) and its rotation (3, 4, 0) repeat; (4, 3, 0) -> (1, 2, 0) is the other orientation; (0, 3, 3) collapses
    assert m["triangles"].tolist() == [[0, 2, 1], [1, 2, 0]] and (m["collapsed"], m["duplicates"]) == (2, 1)
    assert SR.simplify((0, 0, 0), (1, 1, 1), (2, 2, 2), pos, tri, keep_duplicates=True)["triangles"].tolist() == [[0, 2, 1], [2, 1, 0], [1, 2, 0]]
    empty = SR.simplify((0, 0, 0), (1, 1, 1), (2, 2, 2), np.zeros((0, 3), F), np.zeros((0, 3), np.uint32))
    assert empty["positions"].shape == (0, 3) and empty["triangles"].shape == (0, 3) and empty["cells"].shape == (0,)
