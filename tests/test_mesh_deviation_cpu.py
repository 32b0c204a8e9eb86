"""Deviation without a GPU: the ABI of rm_mesh_deviation_default / _weights / rm_mesh_deviation, the layout of its two structs, the sample table
against the restatement bit for bit, every refusal that is made before the handles are looked at, the Python and Node hosts' blocks, and the
numpy restatement (tests/mesh_deviation_ref.py) against closed forms in float64.  The numbers asserted on the restatement are conditions on
those inputs."""
import ctypes as C
import inspect
import json
import math
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_deviation_ref as DR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("rm_mesh_deviation_default", "rm_mesh_deviation_weights", "rm_mesh_deviation")
F = np.float32
PARAMS = [("iso", 0), ("order", 4), ("tolerance", 8), ("flags", 12), ("reserved", 16)]
REPORT = [("vertices", 0), ("triangles", 8), ("skipped_triangles", 16), ("unevaluated_triangles", 24), ("nonfinite_samples", 32), ("over_triangles", 40),
          ("worst_triangle", 48), ("area", 56), ("over_area", 64), ("mean_signed", 72), ("rms", 80), ("max", 88), ("samples", 92), ("reserved", 96)]


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) +{name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshDeviation", "RmMeshDeviationReport") + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported
    assert "---- deviation (opt-in)" in header and "ONE-SIDED" in header and "lower bound" in header


def test_struct_layouts_in_the_header_and_in_python():
    assert C.sizeof(abi.RmMeshDeviation) == 32 and C.sizeof(abi.RmMeshDeviationReport) == 112
    for struct, fields in ((abi.RmMeshDeviation, PARAMS), (abi.RmMeshDeviationReport, REPORT)):
        assert [(n, getattr(struct, n).offset) for n, _ in fields] == fields
        assert [n for n, _ in struct._fields_] == [n for n, _ in fields]
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\nint main(void){ printf("%zu", sizeof(RmMeshDeviation));\n'
                       + "".join(f'printf(" %zu", offsetof(RmMeshDeviation, {n}));\n' for n, _ in PARAMS) + 'printf(" %zu", sizeof(RmMeshDeviationReport));\n'
                       + "".join(f'printf(" %zu", offsetof(RmMeshDeviationReport, {n}));\n' for n, _ in REPORT) + "return 0; }\n")
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32] + [at for _, at in PARAMS] + [112] + [at for _, at in REPORT]
    d = abi.mesh_deviation_dict(abi.RmMeshDeviationReport(vertices=3, worst_triangle=2, rms=0.5, max=0.25, samples=16))
    assert d["vertices"] == 3 and d["worst_triangle"] == 2 and d["rms"] == 0.5 and d["max"] == 0.25 and d["samples"] == 16 and "reserved" not in d
    assert tuple(d) == DR.FIELDS


def test_defaults():
    lib = native.load_library()
    p = abi.RmMeshDeviation(iso=7, order=7, tolerance=7, flags=7, reserved=(7, 7, 7, 7))
    lib.rm_mesh_deviation_default(C.byref(p))
    assert {n: getattr(p, n) for n, _ in PARAMS[:-1]} == abi.MESH_DEVIATION_DEFAULTS == dict(iso=0.0, order=4, tolerance=0.0, flags=0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib.rm_mesh_deviation_default(None)  # (a NULL block is left alone)
    assert bytes(M.mesh_deviation()) == bytes(p)


# ---- the sample table ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", DR.ORDERS)
def test_the_weights_are_the_restatements_bit_for_bit(n):
    lib = native.load_library()
    S = n * n
    room = np.full(4 * S + 8, 7, F)
    assert lib.rm_mesh_deviation_weights(n, native._fp(room[4:])) == abi.RM_OK
    assert (room[:4] == 7).all() and (room[4 + 4 * S:] == 7).all()  # nothing beyond S x 4 floats
    got, want = room[4:4 + 4 * S].reshape(S, 4), DR.weights(n)
    assert got.tobytes() == want.tobytes()
    assert (got[:, :3] > 0).all() and (got[:, 3] == 0).all()
    # every row sums to 1 within 1 ulp of 1 (three quotients of sum exactly 1, each rounded once: at most 3 * 2^-25 off, below 2^-23)
    sums = got[:, :3].astype(np.float64).sum(axis=1)
    assert (np.abs(sums - 1.0) <= 2.0 ** -23).all()
    if n == 1:
        assert got[0, :3].tobytes() == np.full(3, F(1.0 / 3.0), F).tobytes()  # the centroid
    # the S points of a triangle are pairwise distinct, and are the centroids of the n * n congruent sub-triangles
    corners = np.array([[[0.25, -0.5, 1.0], [1.5, 0.25, -0.75], [-0.5, 1.25, 0.5]]], F)
    q = DR.points(corners, n)[0]
    assert len({row.tobytes() for row in q}) == S
    exact = set()
    for r in range(n):  # row r: r + 1 upward and r downward sub-triangles, in lattice coordinates (i, j) of the corners 1 and 2
        for m in range(r + 1):
            exact.add((3 * (r - m) + 1, 3 * m + 1))
        for m in range(r):
            exact.add((3 * (r - m) - 1, 3 * m + 2))
    assert len(exact) == S
    seen = {(int(round(float(w[1]) * 3 * n)), int(round(float(w[2]) * 3 * n))) for w in got}
    assert seen == exact
    for a, b in exact:  # a centroid of a sub-triangle: a and b are 1 or 2 mod 3 alike, and the point lies inside
        assert a % 3 == b % 3 != 0 and a > 0 and b > 0 and a + b < 3 * n


def test_an_invalid_order_is_refused_with_its_text():
    lib = native.load_library()
    last = lambda: lib.rm_last_error(None).decode()
    room = np.full(8, 7, F)
    for order in (0, 3, 16, -1):
        assert lib.rm_mesh_deviation_weights(order, native._fp(room)) == abi.RM_ERR_INVALID
        assert last() == "rm_mesh_deviation_weights: order must be 1, 2, 4 or 8"
    assert lib.rm_mesh_deviation_weights(2, None) == abi.RM_ERR_INVALID and last() == "rm_mesh_deviation_weights: NULL argument"
    assert (room == 7).all()


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------

def block(**fields):
    reserved = fields.pop("reserved", (0, 0, 0, 0))
    return abi.RmMeshDeviation(**{**abi.MESH_DEVIATION_DEFAULTS, **fields}, reserved=reserved)


REFUSALS = [
    (dict(iso=math.nan), "deviation iso must be finite"), (dict(iso=math.inf), "deviation iso must be finite"),
    (dict(order=0), "deviation order must be 1, 2, 4 or 8"), (dict(order=3), "deviation order must be 1, 2, 4 or 8"),
    (dict(order=16), "deviation order must be 1, 2, 4 or 8"),
    (dict(tolerance=-1.0), "deviation tolerance must be finite and >= 0"), (dict(tolerance=math.inf), "deviation tolerance must be finite and >= 0"),
    (dict(tolerance=math.nan), "deviation tolerance must be finite and >= 0"),
    (dict(flags=4), "flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both"),
    (dict(reserved=(1, 0, 0, 0)), "deviation reserved must be 0"), (dict(reserved=(0, 0, 0, 5)), "deviation reserved must be 0"),
]


def test_every_refusal_speaks_before_the_handles_and_in_order():
    lib = native.load_library()
    last = lambda: lib.rm_last_error(None).decode()
    report, room, ms = abi.RmMeshDeviationReport(vertices=7), np.full(4, 7, F), np.full(2, 7, F)
    for fields, text in REFUSALS:
        p = block(**fields)
        assert lib.rm_mesh_deviation(None, None, C.byref(p), C.byref(report), native._fp(room), native._fp(ms)) == abi.RM_ERR_INVALID, fields
        assert last() == "rm_mesh_deviation: " + text, fields
    # the first bad field speaks
    p = block(order=5, tolerance=-1.0, reserved=(3, 0, 0, 0))
    assert lib.rm_mesh_deviation(None, None, C.byref(p), None, None, None) == abi.RM_ERR_INVALID and last() == "rm_mesh_deviation: deviation order must be 1, 2, 4 or 8"
    # a valid block, or none: the handles
    for params in (C.byref(block()), None):
        assert lib.rm_mesh_deviation(None, None, params, C.byref(report), native._fp(room), native._fp(ms)) == abi.RM_ERR_INVALID
        assert last() == "rm_mesh_deviation: NULL argument"
    assert report.vertices == 7 and (room == 7).all() and (ms == 7).all()  # nothing was written


# ---- the Python host -----------------------------------------------------------------------------------------------------------------------

def test_the_python_host_takes_deviation_by_keyword():
    sig = inspect.signature(native.Context.extract_mesh).parameters
    assert sig["deviation"].kind is inspect.Parameter.KEYWORD_ONLY and sig["deviation"].default is None
    assert "deviation" not in inspect.signature(native.Context.mesh_from_values).parameters
    report = dict(samples=16)
    m = M.Mesh(positions=np.zeros((0, 3), F), triangles=np.zeros((0, 3), np.uint32), deviation=report, triangle_deviation=np.zeros(0, F))
    assert m.deviation == report and m.triangle_deviation.shape == (0,)
    plain = M.Mesh(positions=m.positions, triangles=m.triangles)
    assert plain.deviation is None and plain.triangle_deviation is None
    assert "deviation" not in M.Mesh.__dataclass_fields__ and "triangle_deviation" not in M.Mesh.__dataclass_fields__


def test_python_defaults_and_packing():
    p = M.mesh_deviation()
    assert (p.iso, p.order, p.tolerance, p.flags, list(p.reserved)) == (0.0, 4, 0.0, 0, [0, 0, 0, 0])
    p = M.mesh_deviation(iso=0.25, order=8, tolerance=2.0 ** -10, flags=abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL)
    assert (p.iso, p.order, p.tolerance, p.flags) == (0.25, 8, 2.0 ** -10, abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL)
    assert native.Context._mesh_deviation(None, 0.25) is None
    for given in (True, {}):
        q = native.Context._mesh_deviation(given, 0.25)  # iso, where not given, is the extraction's
        assert (q.iso, q.order, q.tolerance, q.flags) == (0.25, 4, 0.0, 0)
    q = native.Context._mesh_deviation(dict(iso=0.5, order=2), 0.25)
    assert (q.iso, q.order) == (0.5, 2)
    given = abi.RmMeshDeviation(iso=0.125, order=1, tolerance=0.5, flags=0, reserved=(0, 5, 0, 0))
    assert bytes(native.Context._mesh_deviation(given, 0.25)) == bytes(given)  # a struct is taken as it stands, its reserved left for the library to refuse
    with pytest.raises(ValueError, match="deviation must be None, True, a dict"):
        native.Context._mesh_deviation(3, 0.0)


@pytest.mark.parametrize("bad", [dict(order=0), dict(order=3), dict(order=16), dict(order=2.0), dict(order=True), dict(order="4"), dict(tolerance=-1),
                                 dict(tolerance=math.inf), dict(tolerance=math.nan), dict(tolerance="0"), dict(iso=math.nan), dict(iso=math.inf), dict(iso=None),
                                 dict(flags=4), dict(flags=True), dict(flags=1.0), dict(samples=16), dict(reserved=0)])
def test_python_refuses_bad_deviation_parameters(bad):
    with pytest.raises(ValueError, match="mesh: (unknown )?deviation "):
        M.mesh_deviation(**bad)
    with pytest.raises(ValueError, match="mesh: (unknown )?deviation "):
        native.Context._mesh_deviation(bad, 0.0)


class RecordingLib:
    """Stands in for the library behind Context._take_mesh: records the names of the calls, answers an empty mesh."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return abi.RM_OK
        return call


def test_the_deviation_runs_on_the_mesh_that_is_returned_behind_the_projection():
    class Scene:
        h = None

    def run(**kw):
        c = native.Context.__new__(native.Context)
        c.lib, c.h = RecordingLib(), None
        got = c._take_mesh(C.c_void_p(), M.Grid((0, 0, 0), (1, 1, 1), (1, 1, 1)), scene=Scene(), **kw)
        return c.lib.calls, got

    today = ["rm_mesh_counts", "rm_mesh_timings", "rm_mesh_download", "rm_mesh_download", "rm_mesh_download", "rm_mesh_destroy"]
    calls, got = run()
    assert calls == today and got.deviation is None and got.triangle_deviation is None and "deviation" not in got.timings
    calls, got = run(deviation=M.mesh_deviation())
    assert calls == today[:-1] + ["rm_mesh_deviation", "rm_mesh_destroy"]
    calls, got = run(project=native.Context._mesh_project(True, 0.0), keep=M.mesh_keep(), deviation=M.mesh_deviation())
    assert calls.index("rm_mesh_filter") < calls.index("rm_mesh_project") < calls.index("rm_mesh_deviation") and calls.count("rm_mesh_deviation") == 1
    assert tuple(got.deviation) == DR.FIELDS and got.triangle_deviation.shape == (0,) and got.triangle_deviation.dtype == F and got.timings["deviation"] == 0.0


# ---- the Node host: the block ------------------------------------------------------------------------------------------------------------------

def test_node_packs_the_deviation_block_as_python_does():
    """meshDeviation and addon.meshDeviationBlock give Python's bytes; extractMesh keeps its arity, passes today's arguments without `deviation`, and
    with it all thirteen (fourteen in slabs) with iso filled in as Python fills it."""
    js = ROOT / "raymarching-engine_amd" / "js"
    assert shutil.which("node") is not None and (js / "rm_napi.node").exists(), "node or the addon is missing"
    cases = [None, dict(), dict(iso=0.25, order=8), dict(order=1, tolerance=2.0 ** -12), dict(order=2, flags=abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL)]
    script = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { sizes: [r.addon.sizes().RmMeshDeviation, r.addon.sizes().RmMeshDeviationReport], defaults: r.MESH_DEVIATION_DEFAULTS, made: r.meshDeviation(), cases: [], bad: [],
              fns: [typeof r.meshDeviation, typeof r.addon.meshDeviationBlock],
              arity: [r.RenderJobContext.prototype.extractMesh.length, r.RenderJobContext.prototype.meshFromValues.length], calls: [], refused: 0 };
for (const c of %s) out.cases.push(hex(r.addon.meshDeviationBlock(c === null ? null : r.meshDeviation(c))));
const g = r.meshGrid([-1, -1, -1], [1, 1, 1], [48, 40, 32]), clusters = r.meshGrid([-1, -1, -1], [1, 1, 1], [12, 12, 7]);
r.addon.extractMesh = (...a) => { out.calls.push(["extractMesh", a.length, a.length === 13 ? [a[11] === null ? null : a[11].iso, a[12]] : null]); return {}; };
r.addon.extractMeshSlabs = (...a) => { out.calls.push(["extractMeshSlabs", a.length, a.length === 14 ? [a[12] === null ? null : a[12].iso, a[13]] : null]); return {}; };
const ctx = Object.create(r.RenderJobContext.prototype);
ctx.ctx = "ctx"; ctx.sceneHandle = () => "scene";
ctx.extractMesh(null, g); ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, null, null, null); ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, null, null, undefined);
ctx.extractMesh(null, g, { iso: 0.25 }, null, null, false, null, null, null, false, null, null, true);
ctx.extractMesh(null, g, { iso: 0.25 }, null, true, true, { grid: clusters }, true, true, true, null, true, { order: 2, iso: 0.5 });
ctx.extractMesh(null, g, null, null, null, false, { grid: clusters }, null, null, false, 5, null, { tolerance: 0.125, flags: 1 });
ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, null, true);
for (const bad of [false, 3, "yes", { order: 3 }, { tolerance: -1 }, { samples: 16 }])
  try { ctx.extractMesh(null, g, null, null, null, false, null, null, null, false, null, null, bad); } catch (e) { out.refused++; }
out.ncalls = out.calls.length;
for (const f of [() => r.meshDeviation(true), () => r.meshDeviation(4), () => r.meshDeviation({ iso: NaN }), () => r.meshDeviation({ iso: "0" }), () => r.meshDeviation({ iso: Infinity }),
                 () => r.meshDeviation({ order: 0 }), () => r.meshDeviation({ order: 3 }), () => r.meshDeviation({ order: 16 }), () => r.meshDeviation({ order: 2.5 }),
                 () => r.meshDeviation({ order: "4" }), () => r.meshDeviation({ tolerance: -1 }), () => r.meshDeviation({ tolerance: Infinity }), () => r.meshDeviation({ tolerance: NaN }),
                 () => r.meshDeviation({ tolerance: null }), () => r.meshDeviation({ flags: 4 }), () => r.meshDeviation({ flags: 0.5 }), () => r.meshDeviation({ samples: 16 }),
                 () => r.meshDeviation({ reserved: 0 }), () => r.addon.meshDeviationBlock(7), () => r.addon.meshDeviationBlock()])
  try { f(); out.bad.push(false); } catch (e) { out.bad.push(true); }
console.log(JSON.stringify(out));
""" % (str(js / "index.js"), json.dumps(cases))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["sizes"] == [32, 112] and all(out["bad"]), out["bad"]
    assert out["fns"] == ["function"] * 2 and out["arity"] == [6, 2]
    made = lambda **kw: dict(dict(out["defaults"]), **kw)
    assert out["calls"] == [["extractMesh", 4, None], ["extractMesh", 4, None], ["extractMesh", 4, None],
                            ["extractMesh", 13, [None, made(iso=0.25)]],
                            ["extractMesh", 13, [0.25, made(iso=0.5, order=2)]],
                            ["extractMeshSlabs", 14, [None, made(tolerance=0.125, flags=1)]], ["extractMesh", 12, None]]
    assert out["refused"] == 6 and out["ncalls"] == 7  # a bad block is refused before the addon is called
    assert out["defaults"] == dict(iso=0, order=4, tolerance=0, flags=0) == out["made"]
    for c, got in zip(cases, out["cases"]):
        assert got == bytes(M.mesh_deviation(**(c or {}))).hex(), c
    dts = (js / "index.d.ts").read_text()
    assert "export function meshDeviation(" in dts and "export interface MeshDeviation " in dts and "export interface MeshDeviationReport " in dts
    assert "deviation: MeshDeviation | true | null): Mesh;" in dts and "deviation?: MeshDeviationReport; triangleDeviation?: Float32Array" in dts


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------------------

def sphere64(radius=1.0):
    """the sphere's distance, evaluated in float64 and rounded once: what a scene's evaluator gives, to half an ulp"""
    return lambda p: (np.linalg.norm(np.asarray(p, np.float64).reshape(-1, 3), axis=1) - radius).astype(F)


OCTAHEDRON = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F),
              np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32))


def test_the_octahedron_in_the_unit_sphere_at_order_1():
    """Each face's centroid lies at 1 / sqrt(3) from the centre, so max_t = 1 - 1 / sqrt(3) and mean_t = -max_t for every face; a face's area is
    sqrt(3) / 2.  Bound: the centroid's three fp32 weights and sums put it within 3 ulp(1/3) of the true one, the field rounds once more, and
    the subtraction of 1 is exact in that binade: a few ulp of fp32 at 0.42, taken as 8 * 2^-25; the area is exact products of small integers in
    double, the root and the tree add a few ulp of double."""
    pos, tri = OCTAHEDRON
    out = DR.deviation(pos, tri, sphere64(), order=1)
    r = out["report"]
    chord = 1.0 - 1.0 / math.sqrt(3.0)
    assert np.abs(out["triangles"].astype(np.float64) - chord).max() <= 8 * 2.0 ** -25
    assert abs(float(r["max"]) - chord) <= 8 * 2.0 ** -25 and r["worst_triangle"] == int(np.argmax(out["triangles"]))
    assert abs(float(r["mean_signed"]) + chord) <= 8 * 2.0 ** -25 and abs(float(r["rms"]) - chord) <= 8 * 2.0 ** -25
    assert abs(float(r["area"]) - 4.0 * math.sqrt(3.0)) <= 16 * 2.0 ** -52 * 4.0 * math.sqrt(3.0)
    assert (r["vertices"], r["triangles"], r["skipped_triangles"], r["unevaluated_triangles"], r["nonfinite_samples"], r["samples"]) == (6, 8, 0, 0, 0, 1)
    assert r["over_triangles"] == 8 and float(r["over_area"]) == float(r["area"])  # tolerance 0: every triangle with max_t > 0 is over
    none = DR.deviation(pos, tri, sphere64(), order=1, tolerance=float(r["max"]))["report"]
    assert none["over_triangles"] == 0 and float(none["over_area"]) == 0.0
    # more samples look nearer the corners, which lie on the sphere, so the mean shrinks; the centroid, a face's deepest point, is a sample of
    # every order (w = (n, n, n) / 3n), so the maximum stays
    for n in (2, 4, 8):
        finer = DR.deviation(pos, tri, sphere64(), order=n)["report"]
        assert finer["samples"] == n * n and -chord < float(finer["mean_signed"]) < 0 and abs(float(finer["max"]) - chord) <= 8 * 2.0 ** -25
        assert float(finer["rms"]) < float(finer["max"])


def test_a_triangle_with_a_foreign_index_is_skipped():
    pos, tri = OCTAHEDRON
    tri = np.concatenate([tri[:3], np.array([[0, 2, 6], [0xFFFFFFFF, 1, 2]], np.uint32), tri[3:]])
    out = DR.deviation(pos, tri, sphere64(), order=2)
    r = out["report"]
    assert r["skipped_triangles"] == 2 and out["skipped"].tolist() == [False] * 3 + [True] * 2 + [False] * 5
    assert out["triangles"][3:5].tobytes() == np.zeros(2, F).tobytes() and (out["triangles"][[0, 1, 2, 5, 6, 7, 8, 9]] > 0).all()
    whole = DR.deviation(*OCTAHEDRON, sphere64(), order=2)["report"]
    assert float(r["area"]) == float(whole["area"]) and r["unevaluated_triangles"] == 0 and r["nonfinite_samples"] == 0 and r["over_triangles"] == 8
    # with no vertex every triangle is skipped; with no triangle nothing is
    empty = DR.deviation(np.zeros((0, 3), F), tri, sphere64())["report"]
    assert empty["skipped_triangles"] == len(tri) and empty["samples"] == 16 and float(empty["area"]) == 0.0 and float(empty["rms"]) == 0.0
    nothing = DR.deviation(pos, np.zeros((0, 3), np.uint32), sphere64())
    assert all(float(nothing["report"][k]) == 0 for k in DR.FIELDS if k not in ("vertices", "samples")) and nothing["triangles"].shape == (0,)


def test_a_nan_at_one_sample_leaves_its_triangle_unevaluated():
    pos, tri = OCTAHEDRON
    order, S = 2, 4
    q = DR.points(pos[tri.astype(np.int64)], order)  # [8, 4, 3]
    poisoned = q[5, 2]

    def field(p):
        p = np.asarray(p, F).reshape(-1, 3)
        d = sphere64()(p)
        d[(p.view(np.uint32) == poisoned.view(np.uint32)).all(axis=1)] = np.nan
        return d

    out, clean = DR.deviation(pos, tri, field, order=order), DR.deviation(pos, tri, sphere64(), order=order)
    r, c = out["report"], clean["report"]
    assert (r["unevaluated_triangles"], r["nonfinite_samples"], r["skipped_triangles"]) == (1, 1, 0) and not out["evaluated"][5] and out["evaluated"].sum() == 7
    finite = np.abs(sphere64()(q[5][[0, 1, 3]]))
    assert out["triangles"][5] == finite.max() > 0  # it keeps its max over the finite samples
    assert float(r["area"]) < float(c["area"]) and abs(float(r["area"]) - 7.0 * math.sqrt(3.0) / 2.0) <= 1e-14  # and is left out of the area
    assert r["over_triangles"] == 7 and r["worst_triangle"] != 5
    # the rms is that of the seven others: by symmetry every face of the octahedron has the same mean and mean square
    assert abs(float(r["rms"]) - float(c["rms"])) <= 2.0 ** -24 and abs(float(r["mean_signed"]) - float(c["mean_signed"])) <= 2.0 ** -24
    allbad = DR.deviation(pos, tri, lambda p: np.full(len(np.asarray(p).reshape(-1, 3)), np.inf, F), order=order)["report"]
    assert (allbad["unevaluated_triangles"], allbad["nonfinite_samples"], allbad["worst_triangle"], float(allbad["max"]), float(allbad["area"]),
            float(allbad["mean_signed"]), float(allbad["rms"])) == (8, 8 * S, 0, 0.0, 0.0, 0.0, 0.0)


def test_the_butterfly_is_a_balanced_tree_with_neighbours_first():
    x = (np.random.default_rng(5).standard_normal((3, 16)) * np.logspace(-8, 0, 16)).astype(np.float64)
    want = ((((x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])) + ((x[:, 4] + x[:, 5]) + (x[:, 6] + x[:, 7])))
            + (((x[:, 8] + x[:, 9]) + (x[:, 10] + x[:, 11])) + ((x[:, 12] + x[:, 13]) + (x[:, 14] + x[:, 15]))))
    assert DR.butterfly(x).tobytes() == want.tobytes()
    assert DR.butterfly(x[:, :1]).tobytes() == x[:, 0].tobytes()
