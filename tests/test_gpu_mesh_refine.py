"""Refinement on the GPU: rm_mesh_refine against the numpy restatement (tests/mesh_refine_ref.py, composed with mesh_project_ref) fed with rm_probe on
the same context and flags.  Arrays are compared by their bits and the report by its bytes."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_deviation_ref as DR
import mesh_refine_ref as RR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import SAMPLE_HI, SAMPLE_LO, table_with_surfaces
from test_gpu_mesh_deviation import GRIDS, SCENES, deviation, twelve_triangles
from test_gpu_mesh_parts import arrays, counts, from_scene, from_values, same_arrays
from test_gpu_mesh_project import slabbed

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID
FAST, NO_CULL = abi.RM_RENDER_FAST, abi.RM_RENDER_NO_CULL
CAMEL = dict(vertices_before="verticesBefore", triangles_before="trianglesBefore", vertices="vertices", triangles="triangles", edges="edges", split_edges="splitEdges",
             nonfinite_midpoints="nonfiniteMidpoints", flipped_triangles="flippedTriangles", max_first="maxFirst", max_last="maxLast", rounds_run="roundsRun", stopped="stopped")


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


def refine(c, h, scene, block=None, inner=None):
    """rm_mesh_refine of the handle: (the new handle, the report's dict, the report's bytes)"""
    out, report = C.c_void_p(), abi.RmMeshRefinement()
    p, q = (None if b is None else C.byref(b) for b in (block, inner))
    assert c.lib.rm_mesh_refine(h, scene.h, p, q, C.byref(out), C.byref(report)) == OK, c.lib.rm_last_error(c.h)
    assert out.value and list(report.reserved) == [0, 0]
    return out, abi.mesh_refinement_dict(report), bytes(report)


def packed(report: dict) -> bytes:
    """a report's dict as the struct's bytes"""
    r = abi.RmMeshRefinement(**{k: (float(v) if k in ("max_first", "max_last") else int(v)) for k, v in report.items() if k not in RR.ROUND_FIELDS})
    for k in RR.ROUND_FIELDS:
        for i, v in enumerate(report[k]):
            getattr(r, k)[i] = int(v)
    return bytes(r)


def restated(c, src, scene, block, inner):
    """the restatement on the source's downloaded arrays, with rm_probe of each block's flags for the distances and the normals"""
    sdf = lambda q: c.probe(scene, abi.RM_PROBE_SDF, q, flags=block.flags)
    project = None
    if inner is not None:
        project = dict(sdf=lambda q: c.probe(scene, abi.RM_PROBE_SDF, q, flags=inner.flags),
                       normal=lambda q: c.probe(scene, abi.RM_PROBE_NORMAL, q, param=inner.normal_delta, flags=inner.flags),
                       iso=inner.iso, rounds=inner.rounds, relax=inner.relax, tolerance=inner.tolerance, reach=inner.reach)
    return RR.refine(src["positions"], src["triangles"], sdf, iso=block.iso, tolerance=block.tolerance, min_edge=block.min_edge, rounds=block.rounds,
                     max_triangles=block.max_triangles, colours=src["colours"], cells=src["cells"], project=project)


def check(c, h, scene, inner=None, normals=False, colours=False, keep=False, **fields):
    """Result and report of the handle against the restatement; the source unchanged; the normals the probe's at the final positions.  Returns
    (report dict, the restatement's dict[, the result's handle with keep])."""
    block = M.mesh_refine(**fields)
    src = arrays(c, h, normals, colours)
    out, report, raw = refine(c, h, scene, block, inner)
    try:
        want = restated(c, src, scene, block, inner)
        got = arrays(c, out, normals, colours)
        assert counts(c, out) == (len(want["positions"]), len(want["triangles"])), (fields, counts(c, out), report, want["report"])
        delta, flags = (inner.normal_delta, inner.flags) if inner is not None else (2.0 ** -10, block.flags)
        new_normals = c.probe(scene, abi.RM_PROBE_NORMAL, got["positions"], param=delta, flags=flags) if normals else None
        assert same_arrays(got, dict(positions=want["positions"], triangles=want["triangles"], cells=want["cells"], colours=want["colours"] if colours else None,
                                     normals=new_normals)), fields
        assert RR.same(report, want["report"]) == [], (fields, report, want["report"])
        assert raw == packed(want["report"]), fields
        assert same_arrays(arrays(c, h, normals, colours), src)  # the source is as it was
    except BaseException:
        c.lib.rm_mesh_destroy(out)
        raise
    if keep:
        return report, want, out
    c.lib.rm_mesh_destroy(out)
    return report, want


# ---- 1: bit for bit against the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, make, cull_flags", SCENES, ids=[s[0] for s in SCENES])
def test_refinement_is_the_restatement_bit_for_bit(ctx, gl_ctx, name, make, cull_flags):
    seen, edges, sizes = set(), [], []
    for which, c, arithmetic in (("strict", ctx, 0), ("fast", ctx, FAST), ("gl stack", gl_ctx, 0)):
        scene = c.create_scene(make())
        meshes = [twelve_triangles(c)]
        try:
            meshes += [from_scene(c, scene, M.Grid(SAMPLE_LO, SAMPLE_HI, n), flags=arithmetic, normals=False) for n in GRIDS]
            sizes += [counts(c, h)[1] for h in meshes]
            for k, h in enumerate(meshes):
                for cull in cull_flags:
                    flags = arithmetic | cull
                    inner = M.mesh_project(flags=flags, reach=0.05)
                    # tolerance 0, one round, the midpoints stay: every edge whose midpoint is not exactly on the surface
                    all_split, want = check(c, h, scene, flags=flags)
                    edges.append(all_split["edges"][0])
                    assert all_split["rounds_run"] == 1 and all_split["split_edges"][0] + all_split["nonfinite_midpoints"][0] <= all_split["edges"][0]
                    # a tolerance that marks nothing: the arrays are the source's, stopped 1 (arrays: `check` compares them with the restatement's, the source's)
                    none, _ = check(c, h, scene, tolerance=float(all_split["max_first"]), rounds=3, flags=flags)
                    assert none["stopped"] == 1 and none["rounds_run"] == 1 and none["split_edges"][0] == 0 and (none["vertices"], none["triangles"]) == counts(c, h)
                    # mixed marks, three rounds, projected; and with the midpoints left where they are
                    mixed, want = check(c, h, scene, inner, tolerance=0.5 * float(all_split["max_first"]), rounds=3, flags=flags)
                    for masks in want["masks"]:
                        seen |= set(int(m) for m in masks)
                    if k <= 1:
                        check(c, h, scene, None, tolerance=0.5 * float(all_split["max_first"]), rounds=3, flags=flags)
                    if k == 0:  # three rounds at tolerance 0 on the mesh of less than one wave: 12 -> 768 triangles where every midpoint is off
                        check(c, h, scene, inner, rounds=3, flags=flags)
                        check(c, h, scene, inner, flags=flags)
        finally:
            for h in meshes:
                c.lib.rm_mesh_destroy(h)
            scene.destroy()
    assert all(t > 0 for t in sizes) and any(e % 256 for e in edges) and any(t % 256 for t in sizes) and sizes[0] < 64 and max(edges) > 4 * 256
    assert seen >= {0, 7} and len(seen) > 2, seen  # (a condition on the inputs: the mixed tolerance splits some edges of a triangle and not others)


def test_colours_normals_and_cells_two_calls_agree_and_the_source_may_go_first(ctx):
    scene = ctx.create_scene(table_with_surfaces())
    h = from_scene(ctx, scene, M.Grid((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), (13, 12, 11)), colours=True)
    try:
        inner = M.mesh_project(reach=0.1, normal_delta=2.0 ** -9)
        for project in (inner, None):
            report, want, out = check(ctx, h, scene, project, normals=True, colours=True, keep=True, tolerance=0.004, rounds=2)
            ms = (C.c_float * 3)()
            assert ctx.lib.rm_mesh_timings(out, ms) == OK and ms[0] == 0.0 and ms[1] > 0.0 and ms[2] > 0.0  # the split rounds; the projections and the normals
            ctx.lib.rm_mesh_destroy(out)
            assert report["split_edges"][0] > 0 and report["vertices"] > report["vertices_before"]
        block = M.mesh_refine(tolerance=0.004, rounds=2)
        first, _, raw = refine(ctx, h, scene, block, inner)
        got = arrays(ctx, first, True, True)
        ctx.lib.rm_mesh_destroy(h)  # the source goes first
        h = None
        again = arrays(ctx, first, True, True)
        assert same_arrays(again, got)
        second, _, raw2 = refine(ctx, first, scene, M.mesh_refine(tolerance=1e9), inner)  # ... and the result is an ordinary mesh: refined again, nothing marked
        assert raw2 != raw and same_arrays(arrays(ctx, second, True, True), dict(got, normals=ctx.probe(scene, abi.RM_PROBE_NORMAL, got["positions"], param=2.0 ** -9)))
        ctx.lib.rm_mesh_destroy(second)
        ctx.lib.rm_mesh_destroy(first)
        h = from_scene(ctx, scene, M.Grid((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3), (13, 12, 11)), colours=True)
        twice, _, raw3 = refine(ctx, h, scene, block, inner)
        assert raw3 == raw and same_arrays(arrays(ctx, twice, True, True), got)  # two calls: the same bytes
        ctx.lib.rm_mesh_destroy(twice)
    finally:
        if h is not None:
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_a_mesh_without_triangles_and_an_empty_mesh_are_copied(ctx):
    scene = ctx.create_scene(S.single_sphere((0.125, -0.0625, 0.1875), 0.875))
    empty = from_values(ctx, (4, 4, 4), np.ones((5, 5, 5), F), 0.0, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    one = np.ones((2, 2, 2), F)
    one[0, 0, 0] = -1.0
    single = from_values(ctx, (1, 1, 1), one, 0.0, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    try:
        for h, size in ((empty, (0, 0)), (single, (1, 0))):
            assert counts(ctx, h) == size
            for inner in (None, M.mesh_project()):
                out, report, raw = refine(ctx, h, scene, M.mesh_refine(rounds=3), inner)
                assert counts(ctx, out) == size and raw == bytes(abi.RmMeshRefinement(vertices_before=size[0], vertices=size[0], stopped=1))
                assert same_arrays(arrays(ctx, out), arrays(ctx, h))
                ctx.lib.rm_mesh_destroy(out)
            bare = C.c_void_p()
            assert ctx.lib.rm_mesh_refine(h, scene.h, None, None, C.byref(bare), None) == OK and counts(ctx, bare) == size  # (params, project and report may be NULL)
            ctx.lib.rm_mesh_destroy(bare)
    finally:
        ctx.lib.rm_mesh_destroy(empty)
        ctx.lib.rm_mesh_destroy(single)
        scene.destroy()


# ---- 2: budget, topology, deviation ----------------------------------------------------------------------------------------------------------------

def test_budget_closedness_and_the_deviation_after(ctx):
    centre, R = (0.125, -0.0625, 0.1875), 0.875
    scene = ctx.create_scene(S.single_sphere(centre, R))
    h = from_scene(ctx, scene, M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (8, 8, 8)), normals=False)
    made = []
    try:
        v, t = counts(ctx, h)
        inner = M.mesh_project()
        before = abi.RmMeshMeasures()
        assert ctx.lib.rm_mesh_measure(h, C.byref(before), None) == OK and before.closed == 1 and before.euler == 2 and before.components == 1
        # a budget of T: the first round is evaluated and not applied
        stopped, _ = check(ctx, h, scene, inner, rounds=3, max_triangles=t)
        assert stopped["stopped"] == 2 and stopped["rounds_run"] == 1 and stopped["split_edges"][0] > 0 and (stopped["vertices"], stopped["triangles"]) == (v, t)
        # between round 1's and round 2's T': one round is applied
        whole, _ = check(ctx, h, scene, inner, rounds=2)
        # (T' of round 1 is 4 T on a closed mesh all of whose edges are split)
        assert whole["split_edges"][0] == whole["edges"][0] == 3 * t // 2 and whole["triangles"] == 16 * t and whole["stopped"] == 0
        one, _ = check(ctx, h, scene, inner, rounds=3, max_triangles=4 * t + 1)
        assert one["stopped"] == 2 and one["rounds_run"] == 2 and one["triangles"] == 4 * t
        # closed before and after, the same Euler characteristic and components; the deviation after is the restatement's, by bits
        rms = [deviation(ctx, h, scene)[0]["rms"]]
        for rounds in (1, 2, 3):
            report, want, out = check(ctx, h, scene, inner, keep=True, rounds=rounds)
            made.append(out)
            after = abi.RmMeshMeasures()
            assert ctx.lib.rm_mesh_measure(out, C.byref(after), None) == OK
            assert (after.closed, after.euler, after.components, after.boundary_edges, after.irregular_edges, after.unbalanced_edges) == (1, 2, 1, 0, 0, 0)
            assert after.triangles == 4 ** rounds * t
            got = deviation(ctx, out, scene)[0]
            sdf = lambda q: ctx.probe(scene, abi.RM_PROBE_SDF, q)
            ref = DR.deviation(want["positions"], want["triangles"], sdf)["report"]
            assert DR.same(got, ref) == [] and np.float64(got["rms"]).tobytes() == np.float64(ref["rms"]).tobytes()
            rms.append(got["rms"])
        print("\norder-4 rms: unprojected source, then after 1, 2, 3 projected rounds", rms)
        # the sagitta of a chord of length L on a sphere of radius R is L^2 / (8 R): a round that halves every edge divides it by 4 (the bar: 3)
        assert rms[1] / rms[2] > 3.0 and rms[2] / rms[3] > 3.0
    finally:
        for out in made:
            ctx.lib.rm_mesh_destroy(out)
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


# ---- 3: refusals with a device ---------------------------------------------------------------------------------------------------------------------

def test_handle_level_refusals(ctx, gl_ctx):
    lib = ctx.lib
    scene, foreign = ctx.create_scene(S.single_sphere()), gl_ctx.create_scene(S.single_sphere())
    h = from_scene(ctx, scene, M.Grid((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (6, 6, 6)), normals=False)
    try:
        pattern = bytes(range(256))
        report, out = abi.RmMeshRefinement.from_buffer_copy(pattern), C.c_void_p(7)
        o, r = C.byref(out), C.byref(report)
        who = "rm_mesh_refine: "
        bad, bad_inner = M.mesh_refine(), M.mesh_project()
        bad.rounds, bad_inner.relax = 9, 2.0
        text_of = lambda mesh: (lib.rm_last_error(ctx.h) if mesh else lib.rm_last_error(None)).decode()
        # 1. an invalid block speaks first, whatever the handles are; the refine block before the project block
        for mesh, sc in ((h, scene.h), (None, scene.h), (h, None), (h, foreign.h), (None, None)):
            assert lib.rm_mesh_refine(mesh, sc, C.byref(bad), C.byref(bad_inner), o, r) == INV and text_of(mesh) == who + "refine rounds must be in 1..8"
            assert lib.rm_mesh_refine(mesh, sc, None, C.byref(bad_inner), o, r) == INV and text_of(mesh) == who + "project relax must be finite and in (0, 1]"
        # 2. then a NULL mesh, scene or out, before the scene's context is looked at
        for mesh, sc, to in ((None, scene.h, o), (h, None, o), (None, foreign.h, o), (None, None, o), (h, scene.h, None), (h, foreign.h, None)):
            for block in (None, C.byref(M.mesh_refine())):
                assert lib.rm_mesh_refine(mesh, sc, block, None, to, r) == INV and text_of(mesh) == who + "NULL argument"
        # 3. then a scene of another context
        assert lib.rm_mesh_refine(h, foreign.h, None, None, o, r) == INV and text_of(h) == who + "the scene belongs to another context"
        assert bytes(report) == pattern and out.value == 7  # no refusal wrote anything
        assert lib.rm_mesh_refine(h, scene.h, None, None, o, r) == OK and out.value != 7 and report.triangles_before == counts(ctx, h)[1] and report.rounds_run == 1
        lib.rm_mesh_destroy(out)
    finally:
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()
        foreign.destroy()


# ---- 4: the hosts, and slabs -------------------------------------------------------------------------------------------------------------------------

LO, HI, N, ISO = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (24, 24, 24), 0.0078125
CLUSTERS = M.Grid(LO, HI, (12, 12, 12))


def test_python_host_equals_the_c_chain_and_slabs_refine_to_the_dense_bytes(ctx):
    scene = ctx.create_scene(S.Mandelbulb())
    g = M.Grid(LO, HI, N)
    try:
        plain = ctx.extract_mesh(scene, g, iso=ISO)
        assert plain.refinement is None and "refinement" not in plain.timings
        for given, block, project in ((True, M.mesh_refine(iso=ISO, tolerance=M.refine_tolerance(g)), None),
                                      (dict(tolerance=0.002, rounds=2, flags=FAST), M.mesh_refine(iso=ISO, tolerance=0.002, rounds=2, flags=FAST), dict(rounds=2)),
                                      (M.mesh_refine(iso=0.0, tolerance=0.001), M.mesh_refine(iso=0.0, tolerance=0.001), None)):
            m = ctx.extract_mesh(scene, g, iso=ISO, colours=True, project=project, refine=given)
            inner = M.mesh_project(iso=ISO, reach=M.project_reach(g), **(project or {}))
            h = from_scene(ctx, scene, g, iso=ISO, colours=True)
            chain = [h]
            try:
                if project is not None:
                    moved = C.c_void_p()
                    assert ctx.lib.rm_mesh_project(h, scene.h, C.byref(inner), C.byref(moved), None, None) == OK
                    chain.append(moved)
                out, report, raw = refine(ctx, chain[-1], scene, block, inner)
                chain.append(out)
                want = arrays(ctx, out, True, True)
            finally:
                for handle in reversed(chain):
                    ctx.lib.rm_mesh_destroy(handle)
            assert same_arrays(dict(positions=m.positions, normals=m.normals, colours=m.colours, triangles=m.triangles, cells=m.cells), want)
            assert packed(m.refinement) == raw and tuple(m.refinement) == RR.FIELDS and m.timings["refinement"] > 0.0 and m.refinement["split_edges"][0] > 0
            assert (m.projection is not None) == (project is not None)
        # behind simplify and keep, before measures and deviation: both see the refined mesh
        m = ctx.extract_mesh(scene, g, iso=ISO, simplify=CLUSTERS, keep=True, refine=dict(tolerance=0.004), measures=True, deviation=dict(order=2), components=True)
        assert m.refinement["triangles"] == len(m.triangles) == m.measures["triangles"] == m.deviation["triangles"] and len(m.labels) == len(m.positions) == m.refinement["vertices"]
        assert m.refinement["triangles"] > m.refinement["triangles_before"]
        # a slabbed extraction refines to the dense one's bytes
        dense = ctx.extract_mesh(scene, g, iso=ISO, refine=dict(tolerance=0.002, rounds=2))
        slabs = ctx.extract_mesh(scene, g, iso=ISO, slabs=5, refine=dict(tolerance=0.002, rounds=2))
        assert M.encode_ply(dense) == M.encode_ply(slabs) and dense.refinement == slabs.refinement and dense.refinement["rounds_run"] == 2
        empty = ctx.extract_mesh(scene, M.Grid((3.0, 3.0, 3.0), (4.0, 4.0, 4.0), (4, 4, 4)), refine=True)
        assert empty.vertices == 0 and empty.refinement["stopped"] == 1 and empty.refinement["rounds_run"] == 0
        for bad in (False, 16, dict(rounds=9), dict(round=1)):
            with pytest.raises(ValueError):
                ctx.extract_mesh(scene, g, iso=ISO, refine=bad)
        reserved = M.mesh_refine()
        reserved.reserved = 1
        with pytest.raises(Exception, match="refine reserved must be 0"):
            ctx.extract_mesh(scene, g, iso=ISO, refine=reserved)
    finally:
        scene.destroy()


def test_node_host_gives_the_python_bytes(ctx, tmp_path):
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(tmp_path)!r};
const ctx = new r.RenderJobContext(0), sc = new r.Mandelbulb(), g = r.meshGrid({list(LO)}, {list(HI)}, {list(N)});
const clusters = r.meshGrid({list(LO)}, {list(HI)}, {list(CLUSTERS.n)});
const a = ctx.extractMesh(sc, g, {{ iso: {ISO} }}, null, null, false, null, null, null, false, null, null, null, true);
const b = ctx.extractMesh(sc, g, {{ iso: {ISO}, colours: true }}, null, true, false, {{ grid: clusters }}, true, null, true, null, {{ rounds: 2 }}, {{ order: 2 }}, {{ tolerance: 0.004, rounds: 2, flags: r.RM.RENDER_FAST }});
const c = ctx.extractMesh(sc, g, {{ iso: {ISO} }}, null, null, false, null, null, null, false, 5, null, null, {{ tolerance: 0.002, rounds: 2 }});
const plain = ctx.extractMesh(sc, g, {{ iso: {ISO} }});
if ("refinement" in plain) process.exit(3);
for (const m of [a, b, c]) if (!(m.refinement.milliseconds > 0) || m.refinement.triangles !== m.triangles.length / 3 || m.refinement.edges.length !== 8 || m.timings.length !== 3) process.exit(4);
if (!("projection" in b) || "projection" in a || b.measures.triangles !== b.refinement.triangles || b.deviation.triangles !== b.refinement.triangles) process.exit(5);
for (const [name, m] of [["a", a], ["b", b], ["c", c]]) fs.writeFileSync(d + "/" + name + ".ply", Buffer.from(r.encodePly(m)));
fs.writeFileSync(d + "/reports.json", JSON.stringify([a.refinement, b.refinement, c.refinement]));
let refused = 0;
for (const bad of [{{ rounds: 9 }}, {{ round: 1 }}, 7, false, {{ tolerance: -1 }}]) try {{ ctx.extractMesh(sc, g, null, null, null, false, null, null, null, false, null, null, null, bad); }} catch (e) {{ refused++; }}
if (refused !== 5) process.exit(6);
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    reports = json.loads((tmp_path / "reports.json").read_text())
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        g = M.Grid(LO, HI, N)
        a = ctx.extract_mesh(scene, g, iso=ISO, refine=True)
        b = ctx.extract_mesh(scene, g, iso=ISO, colours=True, keep=True, simplify=CLUSTERS, quadric=True, measures=True, project=dict(rounds=2), deviation=dict(order=2),
                             refine=dict(tolerance=0.004, rounds=2, flags=FAST))
        c = ctx.extract_mesh(scene, g, iso=ISO, slabs=5, refine=dict(tolerance=0.002, rounds=2))
    finally:
        scene.destroy()
    for name, m, got in (("a", a, reports[0]), ("b", b, reports[1]), ("c", c, reports[2])):
        assert len(m.triangles) > m.refinement["triangles_before"] > 0
        assert (tmp_path / (name + ".ply")).read_bytes() == M.encode_ply(m), name
        assert RR.same({k: got[camel] for k, camel in CAMEL.items()}, m.refinement) == [], (name, got, m.refinement)  # (a JSON number gives every float back)
