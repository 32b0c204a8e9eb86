"""Measures and edge topology without a GPU: the ABI of rm_mesh_measure / rm_mesh_measure_components, the layout of RmMeshMeasures, the NULL
refusals, the numpy restatement (tests/mesh_measure_ref.py) on hand-made triangle lists of every edge class, the fixed tree against math.fsum,
the two hosts' STL bytes, and the Node wrapper's call shapes."""
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

import mesh_measure_ref as QR
import mesh_ref as MR
import mesh_simplify_ref as SR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
ENTRY_POINTS = ("rm_mesh_measure", "rm_mesh_measure_components")
F = np.float32
FIELDS = [("vertices", 0), ("triangles", 8), ("used_vertices", 16), ("skipped_triangles", 24), ("unmeasured_triangles", 32), ("finite_vertices", 40),
          ("edges", 48), ("boundary_edges", 56), ("regular_edges", 64), ("irregular_edges", 72), ("unbalanced_edges", 80), ("euler", 88),
          ("components", 96), ("closed_components", 104), ("area", 112), ("volume", 120), ("lo", 128), ("hi", 140), ("closed", 152), ("reserved", 156)]


STRUCT_FIELDS = [n for n, _ in abi.RmMeshMeasures._fields_ if n != "reserved"]  # what the restatement's dict speaks of


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshMeasures",) + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(ENTRY_POINTS) <= exported
    assert "measures and edge topology" in header and "Non-manifold VERTICES" in header


def test_struct_layout_in_the_header_and_in_python():
    assert C.sizeof(abi.RmMeshMeasures) == 160
    assert [(n, getattr(abi.RmMeshMeasures, n).offset) for n, _ in FIELDS] == FIELDS
    assert [n for n, _ in abi.RmMeshMeasures._fields_] == [n for n, _ in FIELDS]
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\nint main(void){ printf("%zu", sizeof(RmMeshMeasures));\n'
                       + "".join(f'printf(" %zu", offsetof(RmMeshMeasures, {n}));\n' for n, _ in FIELDS) + "return 0; }\n")
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [160] + [at for _, at in FIELDS]
    d = abi.mesh_measures_dict(abi.RmMeshMeasures(vertices=3, euler=-2, closed=1, lo=(C.c_float * 3)(1, 2, 3), area=0.5))
    assert d["vertices"] == 3 and d["euler"] == -2 and d["closed"] is True and d["lo"] == (1.0, 2.0, 3.0) and d["area"] == 0.5 and "reserved" not in d


def test_null_arguments_are_refused_with_their_texts():
    lib = native.load_library()
    last = lambda: lib.rm_last_error(None).decode()
    out, ms, room = abi.RmMeshMeasures(vertices=7), (C.c_float * 2)(7.0, 7.0), np.full(4, 7, np.uint64)
    for o, m in ((C.byref(out), ms), (None, ms), (C.byref(out), None), (None, None)):
        assert lib.rm_mesh_measure(None, o, m) == abi.RM_ERR_INVALID and last() == "rm_mesh_measure: NULL argument"
    for host, size in ((room.ctypes.data_as(C.c_void_p), room.nbytes), (None, 0), (None, 32)):
        assert lib.rm_mesh_measure_components(None, host, size) == abi.RM_ERR_INVALID and last() == "rm_mesh_measure_components: NULL argument"
    assert out.vertices == 7 and list(ms) == [7.0, 7.0] and (room == 7).all()  # nothing was written


def test_the_python_host_takes_measures_by_keyword():
    for fn in (native.Context.extract_mesh, native.Context.mesh_from_values):
        sig = inspect.signature(fn).parameters
        assert sig["measures"].kind is inspect.Parameter.KEYWORD_ONLY and sig["measures"].default is False
    m = M.Mesh(positions=np.zeros((0, 3), F), triangles=np.zeros((0, 3), np.uint32), measures=dict(closed=False))
    assert m.measures == dict(closed=False) and M.Mesh(positions=m.positions, triangles=m.triangles).measures is None
    assert "measures" not in M.Mesh.__dataclass_fields__  # the dataclass's own fields stay as they were


class RecordingLib:
    """Stands in for the library behind Context._take_mesh: records the names of the calls, answers an empty mesh."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return abi.RM_OK
        return call


def test_without_the_keyword_the_calls_are_todays():
    def run(**kw):
        c = native.Context.__new__(native.Context)
        c.lib, c.h = RecordingLib(), None
        got = c._take_mesh(C.c_void_p(), M.Grid((0, 0, 0), (1, 1, 1), (1, 1, 1)), **kw)
        return c.lib.calls, got

    today = ["rm_mesh_counts", "rm_mesh_timings", "rm_mesh_download", "rm_mesh_download", "rm_mesh_download", "rm_mesh_destroy"]
    calls, got = run()
    assert calls == today and got.measures is None and "measures" not in got.timings
    calls, got = run(measures=False, keep=M.mesh_keep())
    assert calls == ["rm_mesh_filter"] + today + ["rm_mesh_destroy"] and got.measures is None
    calls, got = run(measures=True, keep=M.mesh_keep())  # behind the filter, before the counts and the downloads
    assert calls == ["rm_mesh_filter", "rm_mesh_measure", "rm_mesh_measure_components"] + today + ["rm_mesh_destroy"]
    assert got.measures["closed"] is False and got.measures["component_edges"].shape == (0, 4) and got.measures["component_edges"].dtype == np.uint64
    assert got.timings["measures"] == 0.0 and set(got.measures) == {n for n, _ in FIELDS if n != "reserved"} | {"component_edges"}


# ---- the restatement on hand-made triangle lists ----------------------------------------------------------------------------------------------

SQUARE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], F)


def ints(m):
    return {k: int(m[k]) for k in QR.INTEGER_FIELDS}


def test_a_single_triangle_has_three_boundary_edges():
    m = QR.measure(SQUARE[:3], [[0, 1, 2]])
    assert list(m) == STRUCT_FIELDS + ["component_edges"] and list(QR.INTEGER_FIELDS) == STRUCT_FIELDS[:14]  # the struct's fields, in its order
    assert (m["edges"], m["boundary_edges"], m["regular_edges"], m["irregular_edges"], m["unbalanced_edges"]) == (3, 3, 0, 0, 0)
    assert (m["used_vertices"], m["euler"], m["closed"], m["components"], m["closed_components"]) == (3, 1, False, 1, 0)
    assert m["area"] == 0.5 and m["volume"] == 0.0 and m["component_edges"].tolist() == [[3, 3, 0, 0]]
    assert m["lo"].tolist() == [0, 0, 0] and m["hi"].tolist() == [1, 1, 0]


def test_a_tetrahedron_is_closed_and_its_volume_signed():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    out = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]  # counter-clockwise seen from outside
    m = QR.measure(p, out)
    assert (m["edges"], m["regular_edges"], m["euler"], m["closed"], m["closed_components"]) == (6, 6, 2, True, 1)
    assert abs(m["volume"] - 1 / 6) < 1e-15 and abs(m["area"] - (1.5 + math.sqrt(3) / 2)) < 1e-15
    flipped = QR.measure(p, [t[::-1] for t in out])
    assert flipped["closed"] and abs(flipped["volume"] + 1 / 6) < 1e-15
    moved = QR.measure(p + F(16), out)  # the volume is taken about the extent's corner: the same terms wherever the mesh lies
    assert moved["volume"] == m["volume"] and moved["area"] == m["area"]


def test_two_triangles_sharing_an_edge_in_the_same_direction():
    m = QR.measure(SQUARE, [[0, 1, 2], [0, 1, 4]])  # both use 0 -> 1
    assert (m["edges"], m["boundary_edges"], m["regular_edges"], m["irregular_edges"], m["unbalanced_edges"]) == (5, 4, 0, 1, 1)
    x, y, f, r = QR.edge_table(5, [[0, 1, 2], [0, 1, 4]])
    assert (x[0], y[0], f[0], r[0]) == (0, 1, 2, 0)
    opposite = QR.measure(SQUARE, [[0, 1, 2], [1, 0, 4]])
    assert (opposite["regular_edges"], opposite["irregular_edges"], opposite["unbalanced_edges"]) == (1, 0, 0)


def test_three_triangles_on_one_edge():
    m = QR.measure(SQUARE, [[0, 1, 2], [1, 0, 3], [0, 1, 4]])  # f = 2, r = 1
    assert (m["edges"], m["boundary_edges"], m["irregular_edges"], m["unbalanced_edges"], m["closed"]) == (7, 6, 1, 1, False)
    four = QR.measure(SQUARE, [[0, 1, 2], [1, 0, 3], [0, 1, 4], [1, 0, 4]])  # f = 2, r = 2 on {0, 1}: irregular but balanced
    x, y, f, r = QR.edge_table(5, [[0, 1, 2], [1, 0, 3], [0, 1, 4], [1, 0, 4]])
    assert (f[0], r[0]) == (2, 2) and four["irregular_edges"] >= 1 and four["boundary_edges"] + four["regular_edges"] + four["irregular_edges"] == four["edges"]


def test_repeated_and_foreign_indices_are_skipped():
    m = QR.measure(SQUARE, [[0, 1, 2], [0, 0, 3], [1, 4, 5], [2, 3, 0xFFFFFFFF]])
    assert (m["triangles"], m["skipped_triangles"], m["edges"], m["used_vertices"], m["unmeasured_triangles"]) == (4, 3, 3, 3, 0)
    assert m["euler"] == 3 - 3 + 1 and m["area"] == 0.5
    none = QR.measure(SQUARE, [[0, 0, 1]])
    assert (none["skipped_triangles"], none["edges"], none["closed"], none["closed_components"], none["finite_vertices"]) == (1, 0, False, 0, 5)


def test_a_nan_coordinate_is_unmeasured_and_not_in_the_extent():
    p = SQUARE.copy()
    p[3] = (np.nan, 7, 7)
    p[4] = (0.5, np.inf, -9)
    m = QR.measure(p, [[0, 1, 2], [0, 2, 3]])
    assert (m["unmeasured_triangles"], m["skipped_triangles"], m["finite_vertices"], m["edges"]) == (1, 0, 3, 5)
    assert m["area"] == 0.5 and m["lo"].tolist() == [0, 0, 0] and m["hi"].tolist() == [1, 1, 0]
    nothing = QR.measure(np.full((3, 3), np.nan, F), [[0, 1, 2]])
    assert nothing["finite_vertices"] == 0 and nothing["lo"].tobytes() == nothing["hi"].tobytes() == bytes(12) and nothing["unmeasured_triangles"] == 1
    assert nothing["area"].tobytes() == nothing["volume"].tobytes() == bytes(8)


def test_negative_zero_coordinates_give_positive_zero_extents():
    p = np.array([[-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, -0.0]], F)
    m = QR.measure(p, np.zeros((0, 3), np.uint32))
    assert m["lo"].tobytes() == m["hi"].tobytes() == bytes(12) and m["finite_vertices"] == 3
    empty = QR.measure(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32))
    assert ints(empty) == dict.fromkeys(QR.INTEGER_FIELDS, 0) and not empty["closed"] and empty["component_edges"].shape == (0, 4)
    assert empty["area"].tobytes() == bytes(8)


def test_components_own_their_edges():
    p = np.concatenate([SQUARE[:4], SQUARE[:4] + F(3)])
    t = [[0, 1, 2], [0, 2, 3], [4, 5, 6]]
    m = QR.measure(p, t, labels=[0, 0, 0, 0, 1, 1, 1, 2], components=3)
    assert m["component_edges"].tolist() == [[5, 4, 0, 0], [3, 3, 0, 0], [0, 0, 0, 0]] and m["closed_components"] == 0
    assert QR.same(m, m) == [] and QR.same(m, dict(m, area=np.nextafter(m["area"], 9.0), edges=9)) == ["edges", "area"]


# ---- the fixed tree ---------------------------------------------------------------------------------------------------------------------------------

def tree_by_hand(values):
    """the definition, one addition at a time"""
    s = [float(v) for v in values]
    if not s:
        return 0.0
    while True:
        s += [0.0] * (-len(s) % 256)
        nxt = []
        for g in range(0, len(s), 256):
            w = s[g:g + 256]
            off = 128
            while off >= 1:
                for i in range(off):
                    w[i] = w[i] + w[i + off]
                off //= 2
            nxt.append(w[0])
        s = nxt
        if len(s) == 1:
            return s[0]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 404, 65536, 65537, 154448])
def test_the_tree_against_fsum(n):
    """A value passes 8 additions per level and ceil(log256 n) levels.  Each addition's rounding error is at most u |partial sum| with u = 2^-53,
    and every partial sum of non-negative terms is at most their total S: so |tree - exact| <= 8 levels u S (1 + 8 levels u), which the bound
    below states with the second-order factor rounded up to 2."""
    x = np.random.default_rng(n).random(n) * np.logspace(-3, 3, n) if n else np.zeros(0)
    got = QR.tree_sum(x)
    if n <= 65537:
        assert got == tree_by_hand(x)
    levels, m = 0, n
    while m > 1:
        m, levels = (m + 255) // 256, levels + 1
    exact = math.fsum(x)
    assert abs(float(got) - exact) <= 2 * 8 * levels * 2.0 ** -53 * exact
    assert QR.tree_sum(np.full(n, -0.0)).tobytes() == bytes(8) or n % 256 == 0  # -0.0 + +0.0 = +0.0 wherever the padding is met


# ---- STL --------------------------------------------------------------------------------------------------------------------------------------------

def sphere_mesh():
    lo, hi, n, values = SR.sphere_field(8)
    p, t, cells = MR.surface_nets(lo, hi, n, values)
    return M.Mesh(positions=p, triangles=t, cells=cells)


def test_python_stl_is_the_restatements_and_parses_back(tmp_path):
    m = sphere_mesh()
    assert len(m.triangles) == 404
    data = M.encode_stl(m)
    assert data == QR.stl_bytes(m.positions, m.triangles) and len(data) == 84 + 50 * 404
    M.write_stl(m, tmp_path / "m.stl")
    assert (tmp_path / "m.stl").read_bytes() == data
    normals, corners = QR.parse_stl(data)
    assert corners.tobytes() == m.positions[m.triangles.astype(np.int64)].tobytes()
    length = np.sqrt((normals.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() < 2.0 ** -22
    centroid = corners.astype(np.float64).mean(axis=1) - np.array([0.03, -0.02, 0.01])
    assert ((normals * centroid).sum(axis=1) > 0).all()  # the mesher's orientation: outward
    empty = M.Mesh(positions=np.zeros((0, 3), F), triangles=np.zeros((0, 3), np.uint32))
    assert M.encode_stl(empty) == b"hip_raymarch mesh" + bytes(63) + bytes(4) == QR.stl_bytes(empty.positions, empty.triangles)


def test_degenerate_and_overflowing_triangles_get_a_zero_normal():
    p = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3e38, 0, 0], [0, 3e38, 0], [np.nan, 0, 0], [0, 0, 1]], F)
    t = np.array([[0, 1, 2], [0, 0, 1], [0, 3, 4], [0, 1, 5], [0, 1, 6]], np.uint32)
    data = M.encode_stl(M.Mesh(positions=p, triangles=t))
    assert data == QR.stl_bytes(p, t)
    normals, corners = QR.parse_stl(data)
    assert not normals[:2].any() and not normals[3].any()  # collinear, repeated, NaN
    assert normals[2].tolist() == [0, 0, 1]  # 9e76 fits a double: the normal is computed there
    assert np.isfinite(normals[4]).all() and normals[4].any()
    assert corners.tobytes() == p[t.astype(np.int64)].tobytes()


def test_node_encodes_the_stl_python_writes():
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    m = sphere_mesh()
    p = np.concatenate([m.positions, np.array([[3e38, 0, 0], [0, 3e38, 0], [np.nan, 0, 0]], F)])
    v = len(m.positions)
    t = np.concatenate([m.triangles, np.array([[0, 0, 1], [0, v, v + 1], [0, 1, v + 2]], np.uint32)])
    with tempfile.TemporaryDirectory() as tmp:
        p.tofile(str(Path(tmp) / "positions"))
        t.tofile(str(Path(tmp) / "triangles"))
        script = """
const r = require(%r), fs = require("fs"), d = %r;
const mesh = { positions: new Float32Array(new Uint8Array(fs.readFileSync(d + "/positions")).buffer),
               triangles: new Uint32Array(new Uint8Array(fs.readFileSync(d + "/triangles")).buffer) };
fs.writeFileSync(d + "/out.stl", r.encodeStl(mesh));
let refused = false;
try { r.encodeStl({ positions: new Float32Array(9), triangles: new Uint32Array([0, 1, 3]) }); } catch (e) { refused = true; }
fs.writeFileSync(d + "/refused", String(refused));
""" % (str(JS / "index.js"), tmp)
        subprocess.run(["node", "-e", script], check=True, timeout=60)
        assert (Path(tmp) / "out.stl").read_bytes() == M.encode_stl(M.Mesh(positions=p, triangles=t))
        assert (Path(tmp) / "refused").read_text() == "true"


# ---- the Node wrapper's call shapes ---------------------------------------------------------------------------------------------------------------

def test_node_passes_the_measures_argument_only_when_given():
    """The addon's two mesh entries replaced by recorders: without `measures` every earlier call shape is what it was, with it the eleven (nine)
    arguments are all there."""
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    script = """
const r = require(%r);
const calls = [];
r.addon.extractMesh = (...a) => { calls.push(["extractMesh", a.length, a.length === 11 && a[10] === true]); return {}; };
r.addon.meshFromValues = (...a) => { calls.push(["meshFromValues", a.length, a.length === 9 && a[8] === true]); return {}; };
const ctx = Object.create(r.RenderJobContext.prototype);
ctx.ctx = "ctx"; ctx.sceneHandle = () => "scene";
const g = r.meshGrid([0, 0, 0], [1, 1, 1], [2, 2, 2]), s = { grid: g }, v = new Float32Array(27);
ctx.extractMesh(null, g); ctx.extractMesh(null, g, null, true); ctx.extractMesh(null, g, null, null, true, true);
ctx.extractMesh(null, g, null, null, null, false, s); ctx.extractMesh(null, g, null, null, null, false, s, true);
ctx.extractMesh(null, g, null, null, null, false, null, null, true);
ctx.extractMesh(null, g, null, null, null, false, null, null, null, false); ctx.extractMesh(null, g, null, null, null, false, null, null, null, undefined);
ctx.extractMesh(null, g, null, null, null, false, null, null, null, true); ctx.extractMesh(null, g, null, true, true, true, s, true, true, true);
ctx.meshFromValues(g, v); ctx.meshFromValues(g, v, 0, true); ctx.meshFromValues(g, v, 0, null, false, s); ctx.meshFromValues(g, v, 0, null, false, s, true);
ctx.meshFromValues(g, v, 0, null, false, null, null, false); ctx.meshFromValues(g, v, 0, null, false, null, null, true); ctx.meshFromValues(g, v, 0, true, true, s, true, true);
console.log(JSON.stringify({ calls, size: r.addon.sizes().RmMeshMeasures, fns: [typeof r.encodeStl],
                             arity: [r.RenderJobContext.prototype.extractMesh.length, r.RenderJobContext.prototype.meshFromValues.length] }));
""" % str(JS / "index.js")
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["size"] == 160 and out["fns"] == ["function"] and out["arity"] == [6, 2]
    assert out["calls"] == [["extractMesh", 4, False], ["extractMesh", 5, False], ["extractMesh", 7, False], ["extractMesh", 8, False], ["extractMesh", 9, False],
                            ["extractMesh", 10, False], ["extractMesh", 4, False], ["extractMesh", 4, False], ["extractMesh", 11, True], ["extractMesh", 11, True],
                            ["meshFromValues", 4, False], ["meshFromValues", 6, False], ["meshFromValues", 7, False], ["meshFromValues", 8, False],
                            ["meshFromValues", 4, False], ["meshFromValues", 9, True], ["meshFromValues", 9, True]]
    dts = (JS / "index.d.ts").read_text()
    assert "export interface MeshMeasures " in dts and "measures?: MeshMeasures" in dts and "export function encodeStl(" in dts and "measures: boolean): Mesh;" in dts
