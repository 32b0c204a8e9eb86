"""Refinement without a GPU: the ABI of rm_mesh_refine_default / rm_mesh_refine, the layout of its two structs, every refusal that is made before
the handles are looked at, the Python host's blocks, and the numpy restatement (tests/mesh_refine_ref.py) on analytic fields: counts, conformity,
every split pattern, and the chord's sagitta falling by four per round.  The numbers asserted on the restatement are conditions on those inputs
or follow from the geometry stated at the test."""
import ctypes as C
import inspect
import math
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mesh_deviation_ref as DR
import mesh_measure_ref as QR
import mesh_project_ref as PR
import mesh_ref as MR
import mesh_refine_ref as RR
from raymarching_engine_amd import abi, mesh as M, native

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("rm_mesh_refine_default", "rm_mesh_refine")
F = np.float32
PARAMS = [("iso", 0), ("tolerance", 4), ("min_edge", 8), ("rounds", 12), ("max_triangles", 16), ("flags", 24), ("reserved", 28)]
REPORT = [("vertices_before", 0), ("triangles_before", 8), ("vertices", 16), ("triangles", 24), ("edges", 32), ("split_edges", 96), ("nonfinite_midpoints", 160),
          ("flipped_triangles", 224), ("max_first", 232), ("max_last", 236), ("rounds_run", 240), ("stopped", 244), ("reserved", 248)]


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_listed():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) +{name}\(", header, re.M), name
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in ("RmMeshRefine", "RmMeshRefinement") + ENTRY_POINTS)
    assert m.group(1).rstrip().endswith("(additions only)")
    assert lib.rm_abi_version() == 9 == abi.RM_ABI_VERSION
    nm = shutil.which("nm")
    assert nm is not None, "no nm to read the library's exports with"
    out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert set(ENTRY_POINTS) <= {line.split()[-1] for line in out.splitlines() if line.split()}
    assert "---- refinement (opt-in)" in header and "edge midpoints only" in header and "remains" in header


def test_struct_layouts_in_the_header_and_in_python():
    assert C.sizeof(abi.RmMeshRefine) == 32 and C.sizeof(abi.RmMeshRefinement) == 256
    for struct, fields in ((abi.RmMeshRefine, PARAMS), (abi.RmMeshRefinement, REPORT)):
        assert [(n, getattr(struct, n).offset) for n, _ in fields] == fields
        assert [n for n, _ in struct._fields_] == [n for n, _ in fields]
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct layout from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\nint main(void){ printf("%zu", sizeof(RmMeshRefine));\n'
                       + "".join(f'printf(" %zu", offsetof(RmMeshRefine, {n}));\n' for n, _ in PARAMS) + 'printf(" %zu", sizeof(RmMeshRefinement));\n'
                       + "".join(f'printf(" %zu", offsetof(RmMeshRefinement, {n}));\n' for n, _ in REPORT) + "return 0; }\n")
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32] + [at for _, at in PARAMS] + [256] + [at for _, at in REPORT]
    r = abi.RmMeshRefinement(vertices=3, max_last=0.25, rounds_run=2, stopped=1)
    r.split_edges[1] = 9
    d = abi.mesh_refinement_dict(r)
    assert d["vertices"] == 3 and d["max_last"] == 0.25 and d["rounds_run"] == 2 and d["stopped"] == 1 and d["split_edges"] == (0, 9, 0, 0, 0, 0, 0, 0)
    assert tuple(d) == RR.FIELDS and "reserved" not in d


def test_defaults():
    lib = native.load_library()
    p = abi.RmMeshRefine(iso=7, tolerance=7, min_edge=7, rounds=7, max_triangles=7, flags=7, reserved=7)
    lib.rm_mesh_refine_default(C.byref(p))
    assert {n: getattr(p, n) for n, _ in PARAMS[:-1]} == abi.MESH_REFINE_DEFAULTS == dict(iso=0.0, tolerance=0.0, min_edge=0.0, rounds=1, max_triangles=0, flags=0)
    assert p.reserved == 0
    lib.rm_mesh_refine_default(None)  # (a NULL block is left alone)
    assert bytes(M.mesh_refine()) == bytes(p)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------

def block(**fields):
    reserved = fields.pop("reserved", 0)
    return abi.RmMeshRefine(**{**abi.MESH_REFINE_DEFAULTS, **fields}, reserved=reserved)


REFUSALS = [
    (dict(iso=math.nan), "refine iso must be finite"), (dict(iso=-math.inf), "refine iso must be finite"),
    (dict(tolerance=-1.0), "refine tolerance must be finite and >= 0"), (dict(tolerance=math.inf), "refine tolerance must be finite and >= 0"),
    (dict(tolerance=math.nan), "refine tolerance must be finite and >= 0"),
    (dict(min_edge=-0.5), "refine min_edge must be finite and >= 0"), (dict(min_edge=math.inf), "refine min_edge must be finite and >= 0"),
    (dict(min_edge=math.nan), "refine min_edge must be finite and >= 0"),
    (dict(rounds=0), "refine rounds must be in 1..8"), (dict(rounds=9), "refine rounds must be in 1..8"), (dict(rounds=-1), "refine rounds must be in 1..8"),
    (dict(flags=4), "flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both"),
    (dict(reserved=1), "refine reserved must be 0"),
]
PROJECT_REFUSALS = [(dict(rounds=0), "project rounds must be in 1..16"), (dict(relax=0.0), "project relax must be finite and in (0, 1]"),
                    (dict(normal_delta=0.0), "project normal_delta must be finite and > 0"), (dict(reserved=2), "project reserved must be 0")]


def test_every_refusal_speaks_before_the_handles_and_in_order():
    lib = native.load_library()
    last = lambda: lib.rm_last_error(None).decode()
    pattern = bytes(range(256))
    report, out = abi.RmMeshRefinement.from_buffer_copy(pattern), C.c_void_p(7)
    for fields, text in REFUSALS:
        p = block(**fields)
        assert lib.rm_mesh_refine(None, None, C.byref(p), None, C.byref(out), C.byref(report)) == abi.RM_ERR_INVALID, fields
        assert last() == "rm_mesh_refine: " + text, fields
    # the first bad field speaks, and the refine block before the project block
    p, q = block(tolerance=-1.0, rounds=0, reserved=3), abi.RmMeshProject(**{**abi.MESH_PROJECT_DEFAULTS, "rounds": 0})
    assert lib.rm_mesh_refine(None, None, C.byref(p), C.byref(q), C.byref(out), None) == abi.RM_ERR_INVALID
    assert last() == "rm_mesh_refine: refine tolerance must be finite and >= 0"
    for fields, text in PROJECT_REFUSALS:
        q = abi.RmMeshProject(**{**abi.MESH_PROJECT_DEFAULTS, **fields})
        for params in (C.byref(block()), None):
            assert lib.rm_mesh_refine(None, None, params, C.byref(q), C.byref(out), C.byref(report)) == abi.RM_ERR_INVALID, fields
            assert last() == "rm_mesh_refine: " + text, fields
    # valid blocks, or none: the handles
    for params in (C.byref(block()), None):
        for inner in (C.byref(M.mesh_project()), None):
            assert lib.rm_mesh_refine(None, None, params, inner, C.byref(out), C.byref(report)) == abi.RM_ERR_INVALID
            assert last() == "rm_mesh_refine: NULL argument"
    assert bytes(report) == pattern and out.value == 7  # nothing was written


# ---- the Python host -----------------------------------------------------------------------------------------------------------------------

def test_the_python_host_takes_refine_by_keyword():
    sig = inspect.signature(native.Context.extract_mesh).parameters
    assert sig["refine"].kind is inspect.Parameter.KEYWORD_ONLY and sig["refine"].default is None
    assert "refine" not in inspect.signature(native.Context.mesh_from_values).parameters
    assert M.Mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)).refinement is None
    assert M.Mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), refinement=dict(stopped=1)).refinement == dict(stopped=1)


def test_python_defaults_and_packing():
    g = M.Grid((-1.0, -1.0, -2.0), (1.0, 1.0, 2.0), (16, 8, 8))
    h = min(F(2.0) / F(16), F(2.0) / F(8), F(4.0) / F(8))
    assert M.refine_tolerance(g) == float(F(2.0 ** -6) * h) == 0.125 / 64
    assert native.Context._mesh_refine(None, 0.25, None) is None
    for given in (True, {}):
        p, q = native.Context._mesh_refine(given, 0.25, None)(g)  # iso, where not given, is the extraction's; the tolerance the grid's
        assert bytes(p) == bytes(M.mesh_refine(iso=0.25, tolerance=0.125 / 64))
        assert bytes(q) == bytes(M.mesh_project(iso=0.25, reach=M.project_reach(g)))  # the defaults, filled as _mesh_project fills them
    p, q = native.Context._mesh_refine(dict(iso=0.5, tolerance=0.0, rounds=3, max_triangles=1000), 0.25, native.Context._mesh_project(dict(rounds=2, reach=0.125), 0.25))(g)
    assert bytes(p) == bytes(M.mesh_refine(iso=0.5, tolerance=0.0, rounds=3, max_triangles=1000))
    assert bytes(q) == bytes(M.mesh_project(iso=0.25, rounds=2, reach=0.125))  # the caller's project block
    given = block(tolerance=0.5, reserved=9)
    assert bytes(native.Context._mesh_refine(given, 0.25, None)(g)[0]) == bytes(given)  # a struct is taken as it stands, its reserved left for the library to refuse
    assert M.mesh_refine(max_triangles=2 ** 40).max_triangles == 2 ** 40


@pytest.mark.parametrize("bad", [False, 3, "yes", dict(rounds=0), dict(rounds=9), dict(rounds=1.5), dict(rounds=True), dict(tolerance=-1.0), dict(tolerance=math.nan),
                                 dict(tolerance="1"), dict(min_edge=-1.0), dict(min_edge=math.inf), dict(iso=math.inf), dict(iso=None), dict(flags=4), dict(flags=True),
                                 dict(max_triangles=-1), dict(max_triangles=2 ** 64), dict(max_triangles=1.0), dict(round=1), block(rounds=0)])
def test_python_refuses_bad_refine_parameters(bad):
    with pytest.raises(ValueError, match="^mesh: "):
        native.Context._mesh_refine(bad, 0.0, None)


def test_mesh_refine_messages_are_the_librarys():
    for fields, text in REFUSALS:
        if "reserved" in fields or "flags" in fields:
            continue
        with pytest.raises(ValueError) as e:
            M.mesh_refine(**fields)
        assert str(e.value).replace(" an integer in", " in") == "mesh: " + text, fields
    with pytest.raises(ValueError, match="^mesh: unknown refine parameter tolerence$"):
        M.mesh_refine(tolerence=1.0)


def test_the_refinement_runs_behind_the_projection_and_before_the_other_stages():
    """the calls _take_mesh makes, on a recorder in the library's place"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            def call(*args):
                calls.append(name)
                return abi.RM_OK
            return call

    c = native.Context.__new__(native.Context)
    c.lib, c.h = Lib(), None
    c._check = lambda rc: None
    scene = type("S", (), {"h": None})()
    g = M.Grid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 4, 4))
    project = native.Context._mesh_project(True, 0.0)
    got = c._take_mesh(C.c_void_p(), g, scene=scene, keep=M.mesh_keep(), project=project, refine=native.Context._mesh_refine(True, 0.0, project), measures=True,
                       components=True, occlusion=M.mesh_occlusion(), deviation=M.mesh_deviation())
    order = [n for n in calls if n in ("rm_mesh_filter", "rm_mesh_project", "rm_mesh_refine", "rm_mesh_measure", "rm_mesh_components", "rm_mesh_occlusion", "rm_mesh_deviation")]
    assert order == ["rm_mesh_filter", "rm_mesh_project", "rm_mesh_refine", "rm_mesh_measure", "rm_mesh_components", "rm_mesh_occlusion", "rm_mesh_deviation"]
    assert calls.count("rm_mesh_destroy") == 4  # the extraction's, the filter's, the projection's, the refinement's
    assert tuple(got.refinement) == RR.FIELDS and set(got.timings) == {"sampling", "meshing", "attributes", "projection", "refinement", "occlusion", "deviation", "measures"}
    calls.clear()
    plain = c._take_mesh(C.c_void_p(), g, scene=scene)
    assert "rm_mesh_refine" not in calls and plain.refinement is None and "refinement" not in plain.timings


# ---- the restatement on analytic fields ------------------------------------------------------------------------------------------------------

def sphere(centre=(0.0, 0.0, 0.0), radius=0.875):
    c = np.asarray(centre, F)

    def sdf(points):
        q = np.ascontiguousarray(points, F).reshape(-1, 3) - c
        with np.errstate(all="ignore"):
            return (np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]).astype(F)) - F(radius)).astype(F)
    return sdf


def nets(sdf, lo, hi, n):
    values = sdf(MR.corner_positions(lo, hi, n).reshape(-1, 3)).reshape(n[2] + 1, n[1] + 1, n[0] + 1)
    return MR.surface_nets(lo, hi, n, values)


def sphere_8(project=True):
    sdf = sphere()
    p, t, cells = nets(sdf, (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (8, 8, 8))
    inner = dict(sdf=sdf, normal=PR.forward_normal(sdf))
    if project:
        p = PR.project(p, t, **inner)["positions"]
    return sdf, p, t, cells, inner


def conforming(vertices, triangles, closed):
    """no T-junction: on a closed mesh every edge is used exactly twice, once in each direction; the Euler characteristic is returned"""
    x, y, f, r = QR.edge_table(vertices, triangles)
    if closed:
        assert ((f == 1) & (r == 1)).all()
        assert MR.directed_balanced(triangles)
    return MR.euler(None, triangles)


def test_tolerance_zero_splits_every_edge_of_the_sphere_and_stays_closed():
    sdf, p, t, cells, inner = sphere_8()
    assert (len(p), len(t)) == (128, 252) and conforming(len(p), t, True) == 2
    rms = [DR.deviation(p, t, sdf)["report"]["rms"]]
    for _ in range(3):
        V, T = len(p), len(t)
        got = RR.refine(p, t, sdf, tolerance=0.0, cells=cells, project=inner)
        r = got["report"]
        E = r["edges"][0]
        assert E == 3 * T // 2 and r["split_edges"][0] == E and r["nonfinite_midpoints"][0] == 0  # (a condition on the input: no midpoint lies exactly on the sphere)
        assert (r["vertices"], r["triangles"]) == (V + E, 4 * T) and r["rounds_run"] == 1 and r["stopped"] == 0 and (got["masks"][0] == 7).all()
        p, t, cells = got["positions"], got["triangles"], got["cells"]
        assert len(cells) == len(p) and conforming(len(p), t, True) == 2
        rms.append(DR.deviation(p, t, sdf)["report"]["rms"])
    assert (len(p), len(t)) == (8066, 16128)
    # The sagitta of a chord of length L on a sphere of radius R is L^2 / (8 R): halving every edge divides it by 4.  The bar is 3 per round.
    ratios = [a / b for a, b in zip(rms, rms[1:])]
    print("order-4 rms per round", rms, "ratios", ratios)
    assert all(ratio > 3.0 for ratio in ratios), ratios
    # three rounds in one call are the three calls
    whole = RR.refine(*sphere_8()[1:3], sdf, tolerance=0.0, rounds=3, project=inner)
    assert whole["positions"].tobytes() == p.tobytes() and whole["triangles"].tobytes() == t.tobytes() and whole["report"]["rounds_run"] == 3


def test_every_mask_occurs_and_mixed_marks_stay_conforming():
    sdf, p, t, cells, inner = sphere_8()
    seen = set()
    # 0.02 cells of the 8^3 grid (the issue's prototype), and tolerances between the sphere's smallest and largest sagitta
    mids = np.abs(sdf(F(0.5) * (p[t[:, 0]] + p[t[:, 1]])))
    for tolerance in (0.02 * 0.3125, float(np.median(mids)), float(np.quantile(mids, 0.8)), float(np.quantile(mids, 0.2))):
        got = RR.refine(p, t, sdf, tolerance=tolerance, rounds=3, project=inner)
        for masks in got["masks"]:
            seen |= set(int(m) for m in masks)
        r = got["report"]
        print("tolerance", tolerance, "edges", r["edges"][:3], "split", r["split_edges"][:3], "stopped", r["stopped"], "order-4 max", DR.deviation(got["positions"], got["triangles"], sdf)["report"]["max"])
        assert conforming(r["vertices"], got["triangles"], True) == 2
        if tolerance == 0.02 * 0.3125:  # (conditions on the input: what the definition's prototype gave)
            assert (r["edges"][:3], r["split_edges"][:3], r["stopped"], r["rounds_run"]) == ((378, 1368, 2070), (330, 234, 0), 1, 3)
        assert r["triangles"] == r["triangles_before"] + sum(sum(bin(int(m)).count("1") for m in masks) for masks, _ in zip(got["masks"], got["projections"]))
        assert r["vertices"] == r["vertices_before"] + sum(r["split_edges"][:len(got["projections"])])
    assert seen == set(range(8)), seen  # every pattern, each rotation of one and two marked edges among them


def test_a_tolerance_that_marks_nothing_a_budget_and_min_edge():
    sdf, p, t, cells, inner = sphere_8()
    none = RR.refine(p, t, sdf, tolerance=1.0, rounds=3)
    assert none["positions"].tobytes() == p.tobytes() and none["triangles"].tobytes() == t.tobytes()
    assert none["report"]["stopped"] == 1 and none["report"]["rounds_run"] == 1 and none["report"]["split_edges"][0] == 0 and none["report"]["max_first"] > 0
    budget = RR.refine(p, t, sdf, rounds=3, max_triangles=len(t))
    assert budget["triangles"].tobytes() == t.tobytes() and budget["report"]["stopped"] == 2 and budget["report"]["split_edges"][0] == 378
    between = RR.refine(p, t, sdf, rounds=3, max_triangles=4 * len(t) + 1)
    assert between["report"]["stopped"] == 2 and between["report"]["rounds_run"] == 2 and between["report"]["triangles"] == 4 * len(t)
    lengths = np.linalg.norm(p[t[:, 0]].astype(np.float64) - p[t[:, 1]], axis=1)
    some = RR.refine(p, t, sdf, min_edge=float(np.median(lengths)))
    assert 0 < some["report"]["split_edges"][0] < 378 and conforming(some["report"]["vertices"], some["triangles"], True) == 2


def test_a_boundary_and_irregular_edges_give_conforming_meshes():
    # the surface leaves the grid: boundary edges are split like any other, and stay used once
    sdf = sphere(radius=1.2)
    p, t, _ = nets(sdf, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (8, 8, 8))
    x, y, f, r = QR.edge_table(len(p), t)
    assert ((f + r) == 1).sum() > 0
    got = RR.refine(p, t, sdf, tolerance=0.01, rounds=2)
    x2, y2, f2, r2 = QR.edge_table(len(got["positions"]), got["triangles"])
    assert got["report"]["split_edges"][0] > 0 and ((f2 + r2) <= 2).all() and (f2 <= 1).all() and (r2 <= 1).all() and ((f2 + r2) == 1).sum() >= ((f + r) == 1).sum()
    # a checkerboard of inside and outside corners: edges used four times, which every triangle round them sees marked alike
    n = (4, 4, 4)
    k, j, i = np.meshgrid(*(np.arange(5),) * 3, indexing="ij")
    values = np.where((i + j + k) % 2 == 0, F(-0.75), F(0.5)).astype(F)
    p, t, _ = MR.surface_nets((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), n, values)
    x, y, f, r = QR.edge_table(len(p), t)
    assert ((f + r) > 2).sum() > 0  # (a condition on the input)
    wobble = lambda q: (np.sin(F(5.0) * q[:, 0]) * np.cos(F(3.0) * q[:, 1]) + F(0.25) * q[:, 2]).astype(F)
    got = RR.refine(p, t, wobble, tolerance=0.3, rounds=2)
    assert 0 < got["report"]["split_edges"][0] < got["report"]["edges"][0]
    # conforming: a child edge on a parent edge is used as often as the parent was, a child edge inside a triangle twice -- a T-junction would
    # leave an edge used once on a side where its parent was used more often
    x2, y2, f2, r2 = QR.edge_table(len(got["positions"]), got["triangles"])
    assert set(np.unique(f2 + r2)) <= set(np.unique(f + r)) | {2} and ((f2 + r2) == 1).sum() <= 2 * ((f + r) == 1).sum()
    assert ((f2 + r2) > 2).sum() > ((f + r) > 2).sum()  # (irregular edges were split)
    first = RR.split(p, t, wobble, tolerance=0.3)
    assert (first["masks"] >= 0).all()
    marks = {}
    lo, hi, edge_of = RR.edges_of(len(p), t)
    for row, mask in zip(edge_of, first["masks"]):
        for s in range(3):
            assert marks.setdefault(int(row[s]), bool(mask >> s & 1)) == bool(mask >> s & 1)


def test_triangles_that_take_no_part_are_carried_unchanged():
    sdf, p, t, cells, inner = sphere_8()
    odd = np.array([[5, 5, 9], [3, len(p), 4], [7, 8, 7], [0xFFFFFFFF, 1, 2]], np.uint32)
    mixed = np.concatenate([t[:100], odd[:2], t[100:], odd[2:]])
    got = RR.refine(p, mixed, sdf, tolerance=0.0)
    clean = RR.refine(p, t, sdf, tolerance=0.0)
    assert got["report"]["edges"][0] == clean["report"]["edges"][0] and got["report"]["triangles"] == 4 * len(t) + 4
    assert got["positions"].tobytes() == clean["positions"].tobytes()
    assert got["triangles"][400:402].tobytes() == odd[:2].tobytes() and got["triangles"][-2:].tobytes() == odd[2:].tobytes()
    assert np.delete(got["triangles"], [400, 401, len(got["triangles"]) - 2, len(got["triangles"]) - 1], axis=0).tobytes() == clean["triangles"].tobytes()
    assert (got["masks"][0][[100, 101, -2, -1]] == -1).all()
    only = RR.refine(p, odd, sdf, tolerance=0.0)
    assert only["report"]["edges"][0] == 0 and only["report"]["stopped"] == 1 and only["triangles"].tobytes() == odd.tobytes()


def test_colours_and_cells_of_the_new_vertices_and_a_nan_midpoint():
    sdf, p, t, cells, inner = sphere_8()
    colours = np.random.default_rng(5).random((len(p), 3)).astype(F)
    got = RR.refine(p, t, sdf, colours=colours, cells=cells)
    lo, hi, _ = RR.edges_of(len(p), t)
    assert got["colours"][len(p):].tobytes() == (F(0.5) * (colours[lo] + colours[hi])).astype(F).tobytes() and got["cells"][len(p):].tobytes() == cells[lo].tobytes()
    assert got["positions"][:len(p)].tobytes() == p.tobytes() and got["colours"][:len(p)].tobytes() == colours.tobytes()
    holed = lambda q: np.where(q[:, 0] > 0.5, F(np.nan), sdf(q)).astype(F)
    got = RR.refine(p, t, holed)
    r = got["report"]
    assert 0 < r["nonfinite_midpoints"][0] == r["edges"][0] - r["split_edges"][0] and math.isfinite(float(r["max_first"]))


# ---- the Node host ---------------------------------------------------------------------------------------------------------------------------

JS = ROOT / "raymarching-engine_amd" / "js"
USAGE = ("extractMeshRefined(ctx, scene, grid, refine, slabs | null, params | null, sharp | null, keep | null, components, simplify | null, quadric | null, "
         "occlusion | null, measures, project | null, deviation | null)")
NODE_CASES = [None, dict(), dict(iso=0.25, tolerance=0.125, minEdge=0.5, rounds=8, maxTriangles=2 ** 40, flags=abi.RM_RENDER_FAST | abi.RM_RENDER_NO_CULL), dict(rounds=3), dict(maxTriangles=1000)]
NODE_BAD = [
    (dict(iso="0"), "RangeError", "mesh: refine iso must be finite"), (dict(tolerance=-1), "RangeError", "mesh: refine tolerance must be finite and >= 0"),
    (dict(minEdge=-1), "RangeError", "mesh: refine minEdge must be finite and >= 0"), (dict(rounds=0), "RangeError", "mesh: refine rounds must be an integer in 1..8"),
    (dict(rounds=9), "RangeError", "mesh: refine rounds must be an integer in 1..8"), (dict(rounds=1.5), "RangeError", "mesh: refine rounds must be an integer in 1..8"),
    (dict(maxTriangles=-1), "RangeError", "mesh: refine maxTriangles must be an integer in 0..2^53 - 1"),
    (dict(flags=4), "RangeError", "mesh: refine flags must be 0, RM.RENDER_FAST, RM.RENDER_NO_CULL or both"), (dict(bogus=1), "TypeError", "mesh: unknown refine parameter bogus"),
    (3, "TypeError", "mesh: expected an object of refine parameters"),
]

NODE_SCRIPT = """
const r = require(%r);
const hex = (b) => Buffer.from(b).toString("hex");
const out = { sizes: [r.addon.sizes().RmMeshRefine, r.addon.sizes().RmMeshRefinement], defaults: r.MESH_REFINE_DEFAULTS, made: r.meshRefine(), cases: [], bad: [], calls: [], refused: [],
              fns: [typeof r.meshRefine, typeof r.meshRefineTolerance, typeof r.addon.meshRefineBlock, typeof r.addon.extractMeshRefined] };
for (const c of %s) out.cases.push(hex(r.addon.meshRefineBlock(c === null ? null : r.meshRefine(c))));
for (const [bad] of %s) { try { r.meshRefine(bad); out.bad.push(["no error", ""]); } catch (e) { out.bad.push([e.constructor.name, e.message]); } }
// the addon's entries as recorders
const real = r.addon.extractMeshRefined, NAMES = ["extractMesh", "extractMeshSlabs", "extractMeshRefined"];
let call = null;
for (const fn of NAMES) r.addon[fn] = (...a) => { call = [fn, a]; return {}; };
const ctx = Object.create(r.RenderJobContext.prototype);
ctx.ctx = "ctx"; ctx.sceneHandle = (s) => "scene";
const g = r.meshGrid([-1, -1, -1], [1.6, 1, 1], [20, 16, 16]), clusters = r.meshGrid([-1, -1, -1], [1.6, 1, 1], [10, 8, 8]);
const record = (...a) => { call = null; ctx.extractMesh("a scene", g, ...a); return JSON.parse(JSON.stringify(call)); };
out.arity = ctx.extractMesh.length;
out.tolerance = [r.meshRefineTolerance(g), r.meshRefineTolerance(clusters)];
out.calls.push(record({ iso: 0.25 }, null, null, false, null, null, null, false, null, null, null, true));
out.calls.push(record({ iso: 0.25 }, true, true, true, { grid: clusters }, true, true, true, 3, { rounds: 2 }, { order: 2 }, { rounds: 3, tolerance: 0, iso: 0.5 }));
out.calls.push(record(null, null, null, false, null, null, null, false, null, null, null, null));
out.calls.push(record(null, null, null, false, null, null, null, false, null, null, null));
out.wanted = [
  [{ ...r.meshRefine({ iso: 0.25, tolerance: r.meshRefineTolerance(g) }), project: r.meshProject({ iso: 0.25, reach: r.meshProjectReach(g) }) }, null, r.meshParams({ iso: 0.25 })],
  [{ ...r.meshRefine({ rounds: 3, tolerance: 0, iso: 0.5 }), project: r.meshProject({ iso: 0.25, reach: r.meshProjectReach(clusters), rounds: 2 }) }, r.meshSlabs({ layers: 3 }), r.meshParams({ iso: 0.25 }),
   r.meshSharp(), r.meshKeep(), true, r.meshSimplify({ grid: clusters }), r.meshQuadric(), r.meshOcclusion(), true, r.meshProject({ iso: 0.25, reach: r.meshProjectReach(clusters), rounds: 2 }), r.meshDeviation({ iso: 0.25, order: 2 })]];
for (const bad of [3, false, { rounds: 0 }, { bogus: 1 }]) { call = null; try { ctx.extractMesh("a scene", g, null, null, null, false, null, null, null, false, null, null, null, bad); out.refused.push(["no error", "", call !== null]); } catch (e) { out.refused.push([e.constructor.name, e.message, call !== null]); } }
out.counts = [];
for (const count of [0, 14, 16]) { try { real(...Array(count).fill(null)); out.counts.push("no error"); } catch (e) { out.counts.push(e.constructor.name + ": " + e.message); } }
try { real(...Array(15).fill(null)); out.counts.push("no error"); } catch (e) { out.counts.push(e.constructor.name + ": " + e.message); }
console.log(JSON.stringify(out));
"""


def test_node_packs_the_refine_block_as_python_does_and_calls_the_refined_entry_only_with_refine():
    import json
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    script = NODE_SCRIPT % (str(JS / "index.js"), json.dumps(NODE_CASES), json.dumps([[b] for b, _, _ in NODE_BAD]))
    out = json.loads(subprocess.run(["node", "-e", script], capture_output=True, text=True, check=True, timeout=60).stdout)
    assert out["sizes"] == [32, 256] and out["fns"] == ["function"] * 4 and out["arity"] == 6
    assert out["defaults"] == out["made"] == dict(iso=0, tolerance=0, minEdge=0, rounds=1, maxTriangles=0, flags=0)
    snake = dict(minEdge="min_edge", maxTriangles="max_triangles")
    for case, got in zip(NODE_CASES, out["cases"]):
        want = M.mesh_refine(**{snake.get(k, k): v for k, v in (case or {}).items()})
        assert got == bytes(want).hex(), case
    assert [tuple(b) for b in out["bad"]] == [(cls, text) for _, cls, text in NODE_BAD]
    g, clusters = M.Grid((-1.0, -1.0, -1.0), (1.6, 1.0, 1.0), (20, 16, 16)), M.Grid((-1.0, -1.0, -1.0), (1.6, 1.0, 1.0), (10, 8, 8))
    assert out["tolerance"] == [M.refine_tolerance(g), M.refine_tolerance(clusters)]
    first, second, without, short = out["calls"]
    # refine alone: the refined entry, all fifteen arguments, every absent stage null or false
    assert first[0] == "extractMeshRefined" and len(first[1]) == 15 and first[1][:3] == ["ctx", "scene", json.loads(json.dumps(dict(lo=list(g.lo), hi=list(g.hi), n=list(g.n))))]
    assert first[1][3:6] == out["wanted"][0] and first[1][6:] == [None, None, False, None, None, None, False, None, None]
    # everything given: the caller's project block is the stage's and the one inside the rounds; slabs travel in the same entry
    assert second[0] == "extractMeshRefined" and len(second[1]) == 15 and second[1][3:] == out["wanted"][1]
    assert second[1][3]["project"] == second[1][13]
    # without refine, null or left out: today's call
    assert without == short == ["extractMesh", ["ctx", "scene", first[1][2], dict(iso=0, normals=1, normalDelta=1e-5, colours=0, flags=0)]]
    assert out["refused"] == [["TypeError", "mesh: expected true or an object of refine parameters", False]] * 2 + [
        ["RangeError", "mesh: refine rounds must be an integer in 1..8", False], ["TypeError", "mesh: unknown refine parameter bogus", False]]
    assert out["counts"] == ["TypeError: " + USAGE] * 4
