"""Quadric placement without a GPU: the ABI of rm_mesh_quadric_default / rm_mesh_simplify_quadric, every refusal that is made before the handles
are looked at, the two hosts' packing of RmMeshQuadric, and the numpy restatement (tests/mesh_quadric_ref.py) on the meshes the GPU tests use.
The numbers asserted on the restatement are conditions on those inputs: a changed input cannot quietly empty a test."""
import ctypes as C
import json
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_quadric_ref as QR
import mesh_ref as MR
import mesh_simplify_ref as SR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
ENTRY_POINTS = ("rm_mesh_quadric_default", "rm_mesh_simplify_quadric")
F = np.float32


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshQuadric",) + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported


def test_defaults_and_struct_layout():
    lib = native.load_library()
    q = abi.RmMeshQuadric(threshold=0.75, reserved=(C.c_int32 * 3)(5, 6, 7))
    lib.rm_mesh_quadric_default(C.byref(q))
    lib.rm_mesh_quadric_default(None)  # a no-op
    assert (q.threshold, list(q.reserved)) == (float(F(0.1)), [0, 0, 0])
    assert bytes(q) == bytes(M.mesh_quadric()) == np.array([0.1], "<f4").tobytes() + bytes(12) and abi.MESH_QUADRIC_DEFAULTS == dict(threshold=0.1)
    assert C.sizeof(abi.RmMeshQuadric) == 16
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\n'
                       'int main(void){ printf("%zu %zu %zu %zu\\n", sizeof(RmMeshQuadric), offsetof(RmMeshQuadric, threshold), '
                       'offsetof(RmMeshQuadric, reserved), sizeof(RmMeshSimplify)); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 0, 4, 16]
    assert [abi.RmMeshQuadric.threshold.offset, abi.RmMeshQuadric.reserved.offset] == [0, 4]


# ---- the refusals made before the handles are looked at --------------------------------------------------------------------------------------

def c_grid(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), n=(8, 8, 8), reserved=0):
    return abi.RmGrid(lo=(C.c_float * 3)(*lo), hi=(C.c_float * 3)(*hi), n=(C.c_int32 * 3)(*n), reserved=reserved)


def c_params(keep_duplicates=0, reserved=(0, 0, 0)):
    return abi.RmMeshSimplify(keep_duplicates=keep_duplicates, reserved=(C.c_int32 * 3)(*reserved))


def c_quadric(threshold=0.1, reserved=(0, 0, 0)):
    return abi.RmMeshQuadric(threshold=threshold, reserved=(C.c_int32 * 3)(*reserved))


BAD_GRIDS = [(dict(n=(0, 8, 8)), "grid n must be"), (dict(n=(8, 8, 1025)), "grid n must be"), (dict(lo=(float("nan"), -1, -1)), "grid lo and hi must be finite"),
             (dict(hi=(1, float("inf"), 1)), "grid lo and hi must be finite"), (dict(lo=(1, -1, -1)), "grid cell size"), (dict(lo=(-3e38, -1, -1), hi=(3e38, 1, 1)), "grid cell size"),
             (dict(n=(1024, 1024, 1024)), "grid must have at most 2^28 corners"), (dict(reserved=1), "grid reserved must be 0")]
BAD_THRESHOLDS = (1.0, 1.5, -0.125, -1e-30, float("nan"), float("inf"), float("-inf"))
BAD_RESERVED = ((1, 0, 0), (0, -1, 0), (0, 0, 7), (1, 2, 3))


def test_every_refusal_speaks_before_the_handles_and_in_order():
    """No mesh exists without a GPU: every call ends in RM_ERR_INVALID, and the text (rm_last_error(NULL)) tells which check spoke."""
    lib = native.load_library()
    out = C.c_void_p()
    last = lambda: lib.rm_last_error(None).decode()
    inv = abi.RM_ERR_INVALID
    call, who = lib.rm_mesh_simplify_quadric, "rm_mesh_simplify_quadric: "
    worst = C.byref(c_quadric(float("nan"), (1, 1, 1)))
    for o in (C.byref(out), None):
        # simplify's own checks first, in its order and with its texts: the grid before everything ...
        for p in (None, C.byref(c_params()), C.byref(c_params(2, (1, 1, 1)))):
            for q in (None, C.byref(c_quadric()), worst):
                assert call(None, None, p, q, o) == inv and last() == who + "NULL grid"
                for fields, text in BAD_GRIDS:
                    assert call(None, C.byref(c_grid(**fields)), p, q, o) == inv and last().startswith(who + text), (fields, last())
        # ... then keep_duplicates, before simplify's reserved and both quadric checks ...
        for bad in (2, -1, 1 << 30, -(1 << 31)):
            for reserved in ((0, 0, 0), (1, 0, 0), (0, 0, -1)):
                for q in (None, worst):
                    assert call(None, C.byref(c_grid()), C.byref(c_params(bad, reserved)), q, o) == inv
                    assert last() == who + "keep_duplicates must be 0 or 1", (bad, reserved, last())
        # ... then simplify's reserved, each of the three words, before both quadric checks
        for reserved in BAD_RESERVED:
            for dup in (0, 1):
                for q in (None, worst):
                    assert call(None, C.byref(c_grid()), C.byref(c_params(dup, reserved)), q, o) == inv
                    assert last() == who + "simplify reserved must be 0", (reserved, last())
        for p in (None, C.byref(c_params()), C.byref(c_params(1))):
            # then the threshold, before the quadric's reserved
            for t in BAD_THRESHOLDS:
                for reserved in ((0, 0, 0),) + BAD_RESERVED:
                    assert call(None, C.byref(c_grid()), p, C.byref(c_quadric(t, reserved)), o) == inv
                    assert last() == who + "quadric threshold must be finite and in [0, 1)", (t, reserved, last())
            # then the quadric's reserved, each of the three words
            for reserved in BAD_RESERVED:
                for t in (0.0, 0.1, 0.9990234375):
                    assert call(None, C.byref(c_grid()), p, C.byref(c_quadric(t, reserved)), o) == inv
                    assert last() == who + "quadric reserved must be 0", (t, reserved, last())
            # good blocks, and NULL blocks (the defaults): the NULL handles are what is refused
            for q in (None, C.byref(c_quadric()), C.byref(c_quadric(0.0)), C.byref(c_quadric(0.9990234375))):
                for g in (c_grid(), c_grid(n=(1, 1, 1)), c_grid(n=(1024, 3, 5)), c_grid(lo=(-0.5, 0.0, 3.0), hi=(0.5, 1e-3, 1e6), n=(37, 29, 53))):
                    assert call(None, C.byref(g), p, q, o) == inv and last() == who + "NULL argument"
    # rm_mesh_simplify's own texts are as they were, and its struct's reserved words are still refused by both entries
    assert lib.rm_mesh_simplify(None, None, None, C.byref(out)) == inv and last() == "rm_mesh_simplify: NULL grid"
    assert lib.rm_mesh_simplify(None, C.byref(c_grid(n=(0, 8, 8))), None, C.byref(out)) == inv and last().startswith("rm_mesh_simplify: grid n must be")
    assert lib.rm_mesh_simplify(None, C.byref(c_grid()), C.byref(c_params(2, (1, 0, 0))), C.byref(out)) == inv and last() == "rm_mesh_simplify: keep_duplicates must be 0 or 1"
    for reserved in BAD_RESERVED:
        assert lib.rm_mesh_simplify(None, C.byref(c_grid()), C.byref(c_params(0, reserved)), C.byref(out)) == inv and last() == "rm_mesh_simplify: simplify reserved must be 0"
    assert lib.rm_mesh_simplify(None, C.byref(c_grid()), None, C.byref(out)) == inv and last() == "rm_mesh_simplify: NULL argument"
    assert lib.rm_mesh_filter(None, None, C.byref(out)) == inv and last() == "rm_mesh_filter: NULL argument"


# ---- the hosts -------------------------------------------------------------------------------------------------------------------------------------

GRID = M.Grid((-1.0, -0.5, 0.25), (1.0, 0.75, 2.0), (8, 9, 10))


@pytest.mark.parametrize("bad", [None, "0.1", [0.1], True, False, 1.0, 1, -0.125, float("nan"), float("inf"), 1e39, np.float32(1.0)])
def test_python_refuses_bad_quadric_parameters(bad):
    with pytest.raises(ValueError):
        M.mesh_quadric(bad)
    with pytest.raises(ValueError):
        M.mesh_quadric(threshold=bad)


def test_python_packs_what_it_is_given():
    assert isinstance(M.mesh_quadric(), abi.RmMeshQuadric)
    for t in (0, 0.0, 0.1, 0.5, np.float32(0.25), np.float64(0.75), 0.9990234375):
        assert bytes(M.mesh_quadric(t)) == np.array([t], "<f4").tobytes() + bytes(12)
    # the host's own conversion of `quadric`: True, a dict and the struct say the same thing; anything else is refused
    to_c = native.Context._mesh_quadric
    simplify = native.Context._mesh_simplify(GRID)
    assert to_c(None, None) is None and to_c(None, simplify) is None
    for given, t in ((True, 0.1), (dict(), 0.1), (dict(threshold=0.5), 0.5), (M.mesh_quadric(0.25), 0.25), (abi.RmMeshQuadric(0.0), 0.0)):
        block = to_c(given, simplify)
        assert isinstance(block, abi.RmMeshQuadric) and bytes(block) == np.array([t], "<f4").tobytes() + bytes(12)
    reserved = abi.RmMeshQuadric(0.1, (C.c_int32 * 3)(0, 1, 0))  # left for the library to refuse
    assert bytes(to_c(reserved, simplify)) == bytes(reserved)
    for bad in (False, 3, 0.1, "quadric", [0.1], dict(threshold=1.0), dict(threshold=None), dict(thresh=0.1), dict(threshold=0.1, reserved=0), abi.RmMeshQuadric(1.0),
                abi.RmMeshQuadric(float("nan")), abi.RmMeshSimplify(0)):
        with pytest.raises(ValueError):
            to_c(bad, simplify)
    # quadric without simplify: refused before anything runs (no context is needed to find out)
    for given in (True, dict(), dict(threshold=0.5), M.mesh_quadric()):
        with pytest.raises(ValueError, match="simplify"):
            to_c(given, None)
    # the hosts' simplification is as it was
    assert len(native.Context._mesh_simplify(GRID)) == 3 and len(M.mesh_simplify(GRID)) == 2
    assert abi.MESH_SIMPLIFY_DEFAULTS == dict(keep_duplicates=0)
    names = [f for f in M.Mesh.__dataclass_fields__]
    assert names[names.index("timings") + 1:] == ["labels", "component_sizes"]
    import inspect

    for fn in (native.Context.extract_mesh, native.Context.mesh_from_values):
        sig = inspect.signature(fn).parameters
        assert sig["quadric"].kind is inspect.Parameter.KEYWORD_ONLY and sig["quadric"].default is None and sig["simplify"].default is None


def test_node_packs_the_quadric_block_as_python_does():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    cases = [None, dict(), dict(threshold=0), dict(threshold=0.1), dict(threshold=0.5), dict(threshold=0.9990234375)]
    grid = dict(lo=list(GRID.lo), hi=list(GRID.hi), n=list(GRID.n))
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const g = %s;
const out = { size: r.addon.sizes().RmMeshQuadric, defaults: r.MESH_QUADRIC_DEFAULTS, made: r.meshQuadric(), half: r.meshQuadric({ threshold: 0.5 }), cases: [], bad: [],
              simplify: r.meshSimplify({ grid: g }), simplifyDefaults: r.MESH_SIMPLIFY_DEFAULTS,
              fns: [typeof r.meshQuadric, typeof r.addon.meshQuadricBlock, typeof r.addon.meshSimplifyBlock],
              arity: [r.RenderJobContext.prototype.extractMesh.length, r.RenderJobContext.prototype.meshFromValues.length] };
for (const c of %s) out.cases.push(hex(r.addon.meshQuadricBlock(c === null ? null : r.meshQuadric(c))));
for (const f of [() => r.meshQuadric(true), () => r.meshQuadric(0.1), () => r.meshQuadric("0.1"), () => r.meshQuadric({ threshold: 1 }), () => r.meshQuadric({ threshold: -0.125 }),
                 () => r.meshQuadric({ threshold: NaN }), () => r.meshQuadric({ threshold: Infinity }), () => r.meshQuadric({ threshold: "0.1" }), () => r.meshQuadric({ threshold: null }),
                 () => r.meshQuadric({ threshold: 0.1, reserved: 0 }), () => r.meshQuadric({ Threshold: 0.1 }), () => r.addon.meshQuadricBlock(7), () => r.addon.meshQuadricBlock()])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(JS / "index.js"), json.dumps(grid), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 16 and all(out["bad"]), out["bad"]
    assert out["fns"] == ["function"] * 3
    assert out["arity"] == [6, 2]  # the new parameters are appended behind the defaulted ones
    assert out["defaults"] == dict(threshold=0.1) == out["made"] and out["half"] == dict(threshold=0.5)
    assert out["simplify"] == dict(grid=grid, keepDuplicates=0) and out["simplifyDefaults"] == dict(keepDuplicates=0)  # as they were
    for c, got in zip(cases, out["cases"]):
        assert got == bytes(M.mesh_quadric(**(c or {}))).hex(), c
    dts = (JS / "index.d.ts").read_text()
    assert "export function meshQuadric(" in dts and "export interface MeshQuadric " in dts and "quadric: MeshQuadric | true | null" in dts
    assert "export function meshSimplify(" in dts and "export interface MeshSimplify " in dts and "simplify: MeshSimplify | null" in dts


# ---- the restatement on the meshes the GPU tests use ---------------------------------------------------------------------------------------

def source(name):
    """the surface-nets mesh (tests/mesh_ref.py) of a shared field: (lo, hi, positions, triangles, cells)"""
    if name not in source.store:
        lo, hi, n, values, iso = QR.fields()[name]()
        source.store[name] = (lo, hi) + MR.surface_nets(lo, hi, n, values, iso)
    return source.store[name]


source.store = {}


def restated(case):
    """the case's cluster grid and its restatement, computed once and left unchanged"""
    if case not in restated.store:
        field, lo, hi, n = QR.CASES[case]
        flo, fhi, pos, tri, _ = source(field)
        lo, hi = lo or flo, hi or fhi
        restated.store[case] = ((lo, hi, n), QR.simplify_quadric(lo, hi, n, pos, tri))
    return restated.store[case]


restated.store = {}


def errors(case, sdf):
    """(max, rms) of |sdf| at the mean placement and at the quadric placement, float64, in units of the smallest cluster cell edge"""
    (lo, hi, n), m = restated(case)
    h = ((np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / np.asarray(n, np.float64)).min()
    mean, quadric = np.abs(sdf(m["plain"])) / h, np.abs(sdf(m["positions"])) / h
    got = (float(mean.max()), float(np.sqrt((mean ** 2).mean())), float(quadric.max()), float(np.sqrt((quadric ** 2).mean())))
    print(f"{case}: {len(m['positions'])} vertices, mean placement max {got[0]:.4f} rms {got[1]:.4f}, quadric placement max {got[2]:.4f} rms {got[3]:.4f} "
          f"cluster cells; {m['clamped']} clamped")
    return got


@pytest.mark.parametrize("case", list(QR.CASES))
def test_restatement_moves_only_the_positions_and_stays_inside_the_cells(case):
    (lo, hi, n), m = restated(case)
    field = QR.CASES[case][0]
    _, _, pos, tri, _ = source(field)
    for keep in (False, True):
        plain = SR.simplify(lo, hi, n, pos, tri, keep_duplicates=keep)
        got = m if not keep else QR.simplify_quadric(lo, hi, n, pos, tri, keep_duplicates=True)
        for name in ("triangles", "cells"):
            assert got[name].dtype == plain[name].dtype and got[name].tobytes() == plain[name].tobytes(), name
        assert got["normals"] is None and got["colours"] is None and got["plain"].tobytes() == plain["positions"].tobytes()
        assert got["positions"].dtype == F and got["positions"].shape == plain["positions"].shape and np.isfinite(got["positions"]).all()
        assert got["positions"].tobytes() == m["positions"].tobytes()  # keep_duplicates does not reach the positions
    low, high = SR.box_of(lo, hi, n, m["cells"])
    assert (m["positions"] >= low - np.spacing(np.abs(low))).all() and (m["positions"] <= high + np.spacing(np.abs(high))).all()  # the closed box of its cluster cell
    still = m["planes"] == 0
    assert m["positions"][still].tobytes() == m["plain"][still].tobytes()


def test_restatement_conditions_on_the_inputs():
    """what the GPU tests rely on these inputs for"""
    assert [len(source(f)[2]) for f in ("box 48", "box 32")] == [3702, 1578]
    assert [len(restated(c)[1]["positions"]) for c in QR.BOX_CASES] == [216, 210, 96]
    assert (restated("noise 128")[1]["planes"] == 0).sum() == 19  # clusters of unreferenced vertices only: no planes
    one = restated("noise one")[1]
    assert len(one["triangles"]) == 0 and one["planes"].tolist() == [3 * 185110]  # every triangle collapses, yet all contribute planes
    assert len(restated("noise 128")[1]["positions"]) > 65536
    for case in QR.CASES:
        m = restated(case)[1]
        assert (m["positions"] != m["plain"]).any() == (case not in QR.UNMOVED), case


def test_restatement_keeps_the_edges_of_a_box():
    """box 48 -> 12^3: the worst and the rms distance to the true surface at least halve (a float64 run of the same definition: 0.245 -> 0.036 and 0.059 ->
    0.012 cluster cells; this fp32 restatement: 0.2447 -> 0.0358 and 0.0591 -> 0.0123)."""
    mean_max, mean_rms, quadric_max, quadric_rms = errors("box 48 -> 12", QR.box_sdf)
    assert quadric_max <= 0.5 * mean_max and quadric_rms <= 0.5 * mean_rms
    assert restated("box 48 -> 12")[1]["clamped"] <= 4


@pytest.mark.parametrize("case", ["box 48 -> unequal", "box 32 -> 8"])
def test_restatement_on_unequal_and_coarser_clusters(case):
    """s != 1 at (11, 9, 13): strictly better (this restatement: 0.1830 -> 0.0839 of the smallest cluster edge); 32 -> 8: 0.1958 -> 0.0845"""
    mean_max, _, quadric_max, _ = errors(case, QR.box_sdf)
    assert quadric_max < mean_max
    assert restated(case)[1]["clamped"] <= 4


@pytest.mark.parametrize("case", ["sphere 12", "sphere 16"])
def test_restatement_loses_nothing_on_a_sphere(case):
    """this restatement: sphere 12: 0.0243 -> 0.0183; sphere 16: 0.0197 -> 0.0121"""
    mean_max, _, quadric_max, _ = errors(case, QR.sphere_sdf)
    assert quadric_max <= mean_max
    assert restated(case)[1]["clamped"] <= 4


def test_restatement_identity_clustering_moves_little():
    """two balls 64: one vertex per cluster; positions stay inside their cells and within one source-grid cell of S's (every plane of a cluster
    passes through its only vertex, so the minimiser is that vertex and nothing moves at all)"""
    (lo, hi, n), m = restated("two balls 64")
    _, _, pos, tri, _ = source("two balls")
    assert len(m["positions"]) == len(pos) == 206 and (m["planes"] > 0).all()
    source_h = 2.0 / PR_N
    off = np.abs(m["positions"].astype(np.float64) - m["plain"].astype(np.float64)).max()
    print("two balls 64: largest move", float(off), "source cell", source_h)
    assert off <= source_h


PR_N = 16  # cells per axis of mesh_parts_ref.two_balls_field


def test_two_balls_field_is_what_the_bound_assumes():
    import mesh_parts_ref as PR

    lo, hi, n, _ = PR.two_balls_field()
    assert tuple(lo) == (-1.0, -1.0, -1.0) and tuple(hi) == (1.0, 1.0, 1.0) and tuple(n) == (PR_N,) * 3
