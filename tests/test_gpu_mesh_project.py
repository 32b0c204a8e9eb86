"""Projection onto the surface on the GPU: rm_mesh_project against the numpy restatement (tests/mesh_project_ref.py) fed with rm_probe on the same
context and flags.  Every comparison of floats is of their bits: no tolerance anywhere."""
import ctypes as C
import shutil
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import mesh_project_ref as PR
import mesh_quadric_ref as QR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import SAMPLE_HI, SAMPLE_LO, spread, table_with_surfaces
from test_gpu_mesh_parts import FIELDS, arrays, counts, filtered, from_scene, from_values, one_cell, parts, same_arrays
from test_gpu_mesh_quadric import placed
from test_gpu_mesh_simplify import simplified

pytestmark = pytest.mark.gpu
JS = Path(__file__).resolve().parents[1] / "raymarching-engine_amd" / "js"
F = np.float32
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID
FAST, NO_CULL = abi.RM_RENDER_FAST, abi.RM_RENDER_NO_CULL
GUARD = F(-7.0)


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


def project(c, h, scene, block=None):
    """rm_mesh_project of the handle: (the new handle, the report's dict, the V residuals from inside a guard pattern that has to survive)"""
    v, _ = counts(c, h)
    out, report, room = C.c_void_p(), abi.RmMeshProjection(), np.full(v + 16, GUARD, F)
    at = room[8:]  # (a view: the call writes behind eight guard floats)
    p = None if block is None else C.byref(block)
    assert c.lib.rm_mesh_project(h, scene.h, p, C.byref(out), C.byref(report), native._fp(at)) == OK, c.lib.rm_last_error(c.h)
    assert out.value and (room[:8] == GUARD).all() and (room[8 + v:] == GUARD).all() and report.reserved == 0
    return out, abi.mesh_projection_dict(report), room[8:8 + v].copy()


def restated(c, src, scene, block):
    """the restatement on the source's downloaded arrays, with rm_probe of the block's flags for the distances and the normals"""
    sdf = lambda q: c.probe(scene, abi.RM_PROBE_SDF, q, flags=block.flags)
    normal = lambda q: c.probe(scene, abi.RM_PROBE_NORMAL, q, param=block.normal_delta, flags=block.flags)
    return PR.project(src["positions"], src["triangles"], sdf, normal, iso=block.iso, rounds=block.rounds, relax=block.relax, tolerance=block.tolerance,
                      reach=block.reach)


def check(c, h, scene, normals=False, colours=False, **fields):
    """Result, report and residual of the handle against the restatement; the source unchanged, the carried arrays carried, the normals the
    probe's at the new positions, the timings' slots.  Returns the restatement's dict."""
    block = M.mesh_project(**fields)
    src = arrays(c, h, normals, colours)
    out, report, residual = project(c, h, scene, block)
    try:
        want = restated(c, src, scene, block)
        got = arrays(c, out, normals, colours)
        differ = int((PR.bits(got["positions"]) != PR.bits(want["positions"])).any(axis=1).sum())
        assert got["positions"].shape == want["positions"].shape and differ == 0, (fields, differ, len(src["positions"]))
        assert residual.tobytes() == want["residual"].tobytes(), fields
        assert PR.same(report, want["report"]) == [], (fields, report, want["report"])
        new_normals = c.probe(scene, abi.RM_PROBE_NORMAL, got["positions"], param=block.normal_delta, flags=block.flags) if normals else None
        assert same_arrays(got, dict(src, positions=want["positions"], normals=new_normals))
        assert same_arrays(arrays(c, h, normals, colours), src)  # the source is untouched
        ms = (C.c_float * 3)()
        assert c.lib.rm_mesh_timings(out, ms) == OK and ms[0] == 0.0 and ms[1] > 0.0 and (ms[2] > 0.0) == bool(normals), list(ms)
        assert c.lib.rm_mesh_download(out, 5, None, 0) == INV
    finally:
        c.lib.rm_mesh_destroy(out)
    return want


# ---- 1: bit for bit against the restatement ----------------------------------------------------------------------------------------------------

SCENES = [("sphere", lambda: S.single_sphere((0.125, -0.0625, 0.1875), 0.875), (0,)),
          ("kind rows", lambda: S.CsgScene().shape(S.Mandelbulb()).intersect().box((0.0, 0.0, 0.25), (1.25, 1.25, 0.75)), (0,)),
          ("csg64", lambda: S.csg64(), (0, NO_CULL)),  # 64 rows: the big-table path, with the culling grid and without
          ("mandelbulb", lambda: S.Mandelbulb(), (0,))]
# test_gpu_mesh_occlusion's grids: V of 1, below a wave, and beyond one workgroup without being a multiple of 256
GRIDS = [(7, 5, 3), (16, 16, 16), (33, 17, 9)]
SETTINGS = [dict(rounds=1), dict(rounds=4), dict(rounds=16, tolerance=2.0 ** -12, relax=0.5), dict(rounds=4, reach=2.0 ** -6)]


def one_vertex(c):
    lo, hi, n, v, iso = one_cell()
    h = from_values(c, n, v, iso, (-0.75, -0.5, -0.625), (0.5, 0.75, 0.625))
    assert counts(c, h) == (1, 0)
    return h


@pytest.mark.parametrize("name, make, cull_flags", SCENES, ids=[s[0] for s in SCENES])
def test_projection_is_the_restatement_bit_for_bit(ctx, gl_ctx, name, make, cull_flags):
    moved = clamped = settled_waves = 0
    for which, c, arithmetic in (("strict", ctx, 0), ("fast", ctx, FAST), ("gl stack", gl_ctx, 0)):
        scene = c.create_scene(make())
        meshes = [one_vertex(c)]
        try:
            meshes += [from_scene(c, scene, M.Grid(SAMPLE_LO, SAMPLE_HI, n), flags=arithmetic, normals=False) for n in GRIDS]
            sizes = [counts(c, h)[0] for h in meshes]
            assert sizes[0] == 1 and 64 < max(sizes) and 256 < max(sizes) and any(v % 256 for v in sizes[1:]), (name, which, sizes)
            for h in meshes:
                for cull in cull_flags:
                    for fields in SETTINGS:
                        want = check(c, h, scene, flags=arithmetic | cull, **fields)
                        moved += want["report"]["moved_vertices"]
                        clamped += want["report"]["clamped_vertices"] if "reach" in fields else 0
                        settled_waves += sum(s > 0 for s in want["skipped_waves"]) if "tolerance" in fields else 0
        finally:
            for h in meshes:
                c.lib.rm_mesh_destroy(h)
            scene.destroy()
    # conditions on the inputs: some vertex moves, some vertex is clamped at reach 2^-6, some wave is entirely settled at tolerance 2^-12 (on
    # every scene but the bare fractal, whose vertices at iso 0 never come to rest)
    assert moved > 0 and clamped > 0 and (settled_waves > 0 or name == "mandelbulb"), (name, moved, clamped, settled_waves)


def test_a_mesh_of_more_than_65536_vertices_sums_through_three_levels(ctx):
    lo, hi, n, values, iso = FIELDS["noise 0.25"]()
    scene = ctx.create_scene(S.single_sphere((0.0, 0.0, 0.0), 0.75))
    h = from_values(ctx, n, values, iso, lo, hi)
    s = None
    try:
        field, clo, chi, cn = QR.CASES["noise 128"]
        s = simplified(ctx, h, M.Grid(clo or lo, chi or hi, cn))
        assert counts(ctx, s)[0] > 65536
        want = check(ctx, s, scene, rounds=2)
        assert want["report"]["moved_vertices"] > 65536
    finally:
        if s is not None:
            ctx.lib.rm_mesh_destroy(s)
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_waves_settle_in_the_kernels_that_flush_denormals(ctx):
    """The fast Mandelbulb and the fast kind rows evaluate with fp32 denormals flushed, where the evaluating kernel decides on integers whether a
    wave needs normals.  At iso 2^-7 and tolerance 2^-9 most of a Mandelbulb mesh rests from the first round on while some vertices still move:
    waves skip their normals, and a wave that skipped wrongly would leave a vertex behind the restatement.  A subnormal iso and tolerance go
    through the same branch."""
    skipped = moved = 0
    for make in (lambda: S.Mandelbulb(), lambda: S.CsgScene().shape(S.Mandelbulb()).intersect().box((0.0, 0.0, 0.25), (1.25, 1.25, 0.75))):
        scene = ctx.create_scene(make())
        h = from_scene(ctx, scene, M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (40, 40, 40)), iso=2.0 ** -7, flags=FAST, normals=False)
        try:
            assert counts(ctx, h)[0] > 256
            for fields in (dict(iso=2.0 ** -7, tolerance=2.0 ** -9, rounds=4), dict(iso=2.0 ** -7, tolerance=2.0 ** -9, rounds=16, relax=0.5, reach=2.0 ** -5),
                           dict(iso=1e-40, tolerance=1e-41, rounds=2, reach=2.0 ** -5), dict(iso=0.0, tolerance=1e-41, rounds=2, reach=2.0 ** -5)):
                want = check(ctx, h, scene, flags=FAST, **fields)
                if fields["iso"] == 2.0 ** -7:
                    assert any(x > 0.0 for x in want["skipped_waves"]), (fields, want["skipped_waves"])  # some waves skip their normals
                    skipped += sum(0.0 < x < 1.0 for x in want["skipped_waves"])  # ... in a launch in which others do not
                    moved += want["report"]["moved_vertices"]
        finally:
            ctx.lib.rm_mesh_destroy(h)
            scene.destroy()
    assert skipped > 0 and moved > 0


# ---- 2: any mesh ---------------------------------------------------------------------------------------------------------------------------------

def slabbed(c, scene, grid, layers, **params):
    h, g, p, w = C.c_void_p(), grid.to_c(), M.mesh_params(**params), M.mesh_slabs(layers)
    assert c.lib.rm_mesh_extract_slabs(c.h, scene.h, C.byref(g), C.byref(p), C.byref(w), C.byref(h)) == OK, c.lib.rm_last_error(c.h)
    return h


def test_meshes_of_every_origin(ctx):
    scene = ctx.create_scene(table_with_surfaces())
    lo, hi, n, values, iso = FIELDS["noise 1.5"]()
    box = ((-1.4, -1.3, -1.35), (1.45, 1.4, 1.3))
    made = [from_values(ctx, n, values, iso, lo, hi)]
    try:
        made.append(from_scene(ctx, scene, M.Grid(*box, (27, 25, 23)), colours=True))
        made.append(filtered(ctx, made[1], dict(largest=1)))
        made.append(simplified(ctx, made[1], M.Grid(*box, (9, 8, 7))))
        made.append(placed(ctx, made[1], M.Grid(*box, (9, 8, 7))))
        made.append(slabbed(ctx, scene, M.Grid(*box, (27, 25, 23)), 5, colours=True))
        made.append(project(ctx, made[1], scene, M.mesh_project(rounds=1))[0])  # an earlier projection
        made.append(from_scene(ctx, scene, M.Grid(*box, (27, 25, 23)), sharp=True, normals=False))
        kinds = [(False, False)] + [(True, True)] * 6 + [(False, False)]
        assert all(counts(ctx, h)[0] > 0 for h in made)
        for h, (normals, colours) in zip(made, kinds):
            for flags in (0, FAST):
                check(ctx, h, scene, normals, colours, flags=flags, reach=2.0 ** -5)
    finally:
        for h in reversed(made):
            ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_an_empty_mesh_gives_an_empty_mesh(ctx):
    scene = ctx.create_scene(S.single_sphere())
    h = from_values(ctx, (4, 4, 4), np.ones((5, 5, 5), F), 0.0, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    try:
        assert counts(ctx, h) == (0, 0)
        for block in (None, M.mesh_project(rounds=16, flags=FAST)):
            out, report, residual = project(ctx, h, scene, block)  # (the guard round the buffer is checked in there)
            assert counts(ctx, out) == (0, 0) and all(v == 0 for v in report.values()) and len(residual) == 0
            ms = (C.c_float * 3)(5.0, 5.0, 5.0)
            assert ctx.lib.rm_mesh_timings(out, ms) == OK and list(ms) == [0.0, 0.0, 0.0]
            assert same_arrays(arrays(ctx, out), arrays(ctx, h))
            ctx.lib.rm_mesh_destroy(out)
    finally:
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_five_calls_give_identical_bytes_and_both_slots_are_timed(ctx):
    scene = ctx.create_scene(S.Mandelbulb())
    h = from_scene(ctx, scene, M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (40, 40, 40)), iso=0.0078125)
    try:
        for flags in (0, FAST):
            block = M.mesh_project(iso=0.0078125, flags=flags)
            runs = []
            for _ in range(5):
                out, report, residual = project(ctx, h, scene, block)
                got, ms = arrays(ctx, out, True, False), (C.c_float * 3)()
                assert ctx.lib.rm_mesh_timings(out, ms) == OK and ms[0] == 0.0 and ms[1] > 0.0 and ms[2] > 0.0, list(ms)
                ctx.lib.rm_mesh_destroy(out)
                runs.append(got["positions"].tobytes() + got["normals"].tobytes() + residual.tobytes() + repr(sorted(report.items())).encode())
            assert len(set(runs)) == 1 and report["moved_vertices"] > 0
    finally:
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_rounds_compose_and_stop_by_themselves(ctx):
    """One round and one round are two rounds at reach 0.  On a box, a table scene, 16 rounds at tolerance 2^-16 stop early, and a call with just
    the rounds that ran gives the same bytes."""
    scene = ctx.create_scene(S.CsgScene().box(QR.BOX_CENTRE, QR.BOX_HALF))
    lo, hi, n, values = QR.box_field(32)
    h = from_values(ctx, n, values, 0.0, lo, hi)
    q = placed(ctx, h, M.Grid(lo, hi, (8, 8, 8)))
    try:
        one, _, _ = project(ctx, q, scene, M.mesh_project(rounds=1))
        two, _, two_residual = project(ctx, one, scene, M.mesh_project(rounds=1))
        both, report, both_residual = project(ctx, q, scene, M.mesh_project(rounds=2))
        assert same_arrays(arrays(ctx, two), arrays(ctx, both)) and two_residual.tobytes() == both_residual.tobytes() and report["rounds_run"] == 2
        for handle in (one, two, both):
            ctx.lib.rm_mesh_destroy(handle)
        long, report, residual = project(ctx, q, scene, M.mesh_project(rounds=16, tolerance=2.0 ** -16))
        assert 0 < report["rounds_run"] < 16 and report["settled_after"] == report["vertices"]
        short, again, short_residual = project(ctx, q, scene, M.mesh_project(rounds=report["rounds_run"], tolerance=2.0 ** -16))
        assert same_arrays(arrays(ctx, short), arrays(ctx, long)) and PR.same(again, report) == [] and short_residual.tobytes() == residual.tobytes()
        ctx.lib.rm_mesh_destroy(long)
        ctx.lib.rm_mesh_destroy(short)
        check(ctx, q, scene, rounds=16, tolerance=2.0 ** -16)
    finally:
        ctx.lib.rm_mesh_destroy(q)
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


def test_handle_level_refusals_in_their_order(ctx, gl_ctx):
    lib = ctx.lib
    scene, foreign = ctx.create_scene(S.single_sphere()), gl_ctx.create_scene(S.single_sphere())
    h = from_scene(ctx, scene, M.Grid((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (6, 6, 6)), normals=False)
    try:
        v = counts(ctx, h)[0]
        out, report, room = C.c_void_p(77), abi.RmMeshProjection(vertices=7), np.full(v, GUARD, F)
        o, r, e = C.byref(out), C.byref(report), native._fp(room)
        who = "rm_mesh_project: "
        bad = M.mesh_project()
        bad.rounds = 17
        last = lambda known: (lib.rm_last_error(ctx.h if known else None) or b"").decode()
        # the block speaks first, whatever the handles are
        for mesh, sc, known in ((h, foreign.h, True), (None, None, False), (h, None, True)):
            assert lib.rm_mesh_project(mesh, sc, C.byref(bad), o, r, e) == INV and last(known) == who + "project rounds must be in 1..16"
        # then a NULL handle or out
        for mesh, sc, oo, known in ((None, scene.h, o, False), (h, None, o, True), (h, scene.h, None, True), (h, foreign.h, None, True)):
            assert lib.rm_mesh_project(mesh, sc, None, oo, r, e) == INV and last(known) == who + "NULL argument"
        # then the scene's context
        assert lib.rm_mesh_project(h, foreign.h, None, o, r, e) == INV and last(True) == who + "the scene belongs to another context"
        assert out.value == 77 and report.vertices == 7 and (room == GUARD).all()  # no refusal wrote anything
        # report and residual_host may be NULL
        assert lib.rm_mesh_project(h, scene.h, None, o, None, None) == OK and out.value not in (None, 77)
        lib.rm_mesh_destroy(out)
    finally:
        lib.rm_mesh_destroy(h)
        scene.destroy()
        foreign.destroy()


# ---- 3: what it shows ---------------------------------------------------------------------------------------------------------------------------

def measured(c, h):
    block = abi.RmMeshMeasures()
    assert c.lib.rm_mesh_measure(h, C.byref(block), None) == OK, c.lib.rm_last_error(c.h)
    return abi.mesh_measures_dict(block)


def test_the_vertices_of_a_clustered_box_come_to_lie_on_it(ctx):
    """The box of mesh_quadric_ref as a table scene, 48^3 cells on [-1, 1]^3, clustered at 12^3 by mean placement, projected at the defaults:
    the CPU test's bar, max_after <= max_before / 1000 (the table's box distance is QR.box_sdf's formula in fp32)."""
    scene = ctx.create_scene(S.CsgScene().box(QR.BOX_CENTRE, QR.BOX_HALF))
    lo, hi, n = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (48, 48, 48)
    h = from_scene(ctx, scene, M.Grid(lo, hi, n), normals=False)
    s = simplified(ctx, h, M.Grid(lo, hi, (12, 12, 12)))
    try:
        out, report, residual = project(ctx, s, scene)
        cell = 2.0 / 12
        print(f"\nbox 48 -> 12, mean placement: {report['vertices']} vertices, worst {report['max_before'] / cell:.4f} -> {report['max_after'] / cell:.3g} cluster cells, "
              f"rms {report['rms_before'] / cell:.4f} -> {report['rms_after'] / cell:.3g}, {report['rounds_run']} rounds, {report['flipped_triangles']} flipped")
        assert report["max_after"] <= report["max_before"] / 1000
        assert report["flipped_triangles"] == 0 and report["vertices"] > 0
        before, after = measured(ctx, s), measured(ctx, out)
        for k in ("edges", "boundary_edges", "regular_edges", "irregular_edges", "unbalanced_edges", "euler", "components", "closed"):
            assert after[k] == before[k], k
        exact = np.abs(QR.box_sdf(arrays(ctx, out)["positions"])).max()
        assert exact <= report["max_before"] / 1000  # ... and against the float64 distance
        ctx.lib.rm_mesh_destroy(out)
    finally:
        ctx.lib.rm_mesh_destroy(s)
        ctx.lib.rm_mesh_destroy(h)
        scene.destroy()


# ---- 4: the Python host ---------------------------------------------------------------------------------------------------------------------------

def test_python_host_equals_the_c_level_chain(ctx):
    grid, clusters = M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (48, 48, 48)), M.Grid((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (12, 12, 12))
    iso = 2.0 ** -7
    scene = ctx.create_scene(S.Mandelbulb())
    try:
        h = from_scene(ctx, scene, grid, iso=iso, colours=True)
        q = placed(ctx, h, clusters)
        f = filtered(ctx, q, None)
        block = M.mesh_project(iso=iso, reach=M.project_reach(clusters))
        assert F(block.reach) == F(0.5) * (F(2.5) / F(12))
        out, report, residual = project(ctx, f, scene, block)
        want, (want_labels, want_sizes), want_measures = arrays(ctx, out, True, True), parts(ctx, out), measured(ctx, out)
        ao = np.empty(len(want["positions"]), F)
        assert ctx.lib.rm_mesh_occlusion(out, scene.h, None, native._fp(ao), None) == OK
        fine, fine_report, _ = project(ctx, h, scene, M.mesh_project(iso=iso, reach=M.project_reach(grid), rounds=2))
        want_fine = arrays(ctx, fine, True, True)
        for handle in (fine, out, f, q, h):
            ctx.lib.rm_mesh_destroy(handle)
        assert report["moved_vertices"] > 0
        for given in (True, dict(), dict(iso=iso), block):
            m = ctx.extract_mesh(scene, grid, iso=iso, colours=True, simplify=clusters, quadric=True, keep=True, components=True, measures=True, project=given,
                                 occlusion=True)
            got = dict(positions=m.positions, normals=m.normals, colours=m.colours, triangles=m.triangles, cells=m.cells)
            assert same_arrays(got, want) and np.array_equal(m.labels, want_labels) and np.array_equal(m.component_sizes, want_sizes)
            assert PR.same(m.projection, report) == [] and m.residual.tobytes() == residual.tobytes() and m.occlusion.tobytes() == ao.tobytes()
            assert {k: v for k, v in m.measures.items() if k != "component_edges"} == want_measures
            assert m.timings["projection"] > 0.0 and (m.grid.lo, m.grid.hi, m.grid.n) == (clusters.lo, clusters.hi, clusters.n)
            assert m.timings["sampling"] == 0.0 and m.timings["meshing"] > 0.0 and m.timings["attributes"] == 0.0  # the filter's slots, not the projection's
        m = ctx.extract_mesh(scene, grid, iso=iso, colours=True, project=dict(rounds=2))  # without simplify: the sampling grid's reach
        assert m.positions.tobytes() == want_fine["positions"].tobytes() and m.normals.tobytes() == want_fine["normals"].tobytes()
        assert PR.same(m.projection, fine_report) == []
        assert m.timings["sampling"] > 0.0 and m.timings["meshing"] > 0.0 and m.timings["attributes"] > 0.0 and m.timings["projection"] > 0.0  # the extraction's
        plain = ctx.extract_mesh(scene, grid, iso=iso, colours=True)
        assert plain.projection is None and plain.residual is None and "projection" not in plain.timings and plain.positions.tobytes() != m.positions.tobytes()
        for bad in (False, 3, dict(rounds=0), dict(reach=-1.0), dict(step=1)):
            with pytest.raises(ValueError):
                ctx.extract_mesh(scene, grid, project=bad)
        with pytest.raises(RuntimeError, match="project reserved"):
            ctx.extract_mesh(scene, grid, project=abi.RmMeshProject(iso=0.0, rounds=4, relax=1.0, tolerance=0.0, reach=0.0, normal_delta=2.0 ** -10, flags=0, reserved=1))
    finally:
        scene.destroy()


CAMEL = dict(vertices="vertices", triangles="triangles", moved_vertices="movedVertices", settled_before="settledBefore", settled_after="settledAfter",
             nonfinite_before="nonfiniteBefore", nonfinite_after="nonfiniteAfter", clamped_vertices="clampedVertices", undirected_vertices="undirectedVertices",
             flipped_triangles="flippedTriangles", worst_before="worstBefore", worst_after="worstAfter", mean_before="meanBefore", rms_before="rmsBefore",
             mean_after="meanAfter", rms_after="rmsAfter", max_before="maxBefore", max_after="maxAfter", rounds_run="roundsRun")


def test_node_host_gives_the_python_bytes(ctx, tmp_path):
    assert shutil.which("node") is not None and (JS / "rm_napi.node").exists(), "node or the addon is missing"
    import json

    lo, hi, n, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), (40, 40, 40), 0.0078125
    script = f"""
const r = require({str(JS / "index.js")!r}), fs = require("fs"), d = {str(tmp_path)!r};
const ctx = new r.RenderJobContext(0), sc = new r.Mandelbulb(), g = r.meshGrid({list(lo)}, {list(hi)}, {list(n)});
const clusters = r.meshGrid({list(lo)}, {list(hi)}, [10, 10, 10]);
const save = (name, a) => fs.writeFileSync(d + "/" + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const m = ctx.extractMesh(sc, g, {{ iso: {iso}, colours: true }}, null, true, true, {{ grid: clusters }}, true, true, true, null, true);
for (const k of ["positions", "normals", "colours", "triangles", "cells", "labels", "componentSizes", "occlusion", "residual"]) save("a_" + k, m[k]);
const fine = ctx.extractMesh(sc, g, {{ iso: {iso} }}, null, null, false, null, null, null, false, null, {{ rounds: 2 }});
for (const k of ["positions", "normals", "residual"]) save("b_" + k, fine[k]);
const slabbed = ctx.extractMesh(sc, g, {{ iso: {iso} }}, null, null, false, null, null, null, false, 7, {{ rounds: 2 }});
for (const k of ["positions", "residual"]) save("c_" + k, slabbed[k]);
const plain = ctx.extractMesh(sc, g, {{ iso: {iso} }});
if ("projection" in plain || "residual" in plain || plain.timings.length !== 3) process.exit(3);
if (!(m.projection.milliseconds > 0) || m.timings[0] !== 0 || !(fine.timings[0] > 0)) process.exit(4);
fs.writeFileSync(d + "/reports.json", JSON.stringify([m.projection, fine.projection, slabbed.projection, m.measures.edges]));
ctx.close();
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    reports = json.loads((tmp_path / "reports.json").read_text())
    h = ctx.create_scene(S.Mandelbulb())
    try:
        g, clusters = M.Grid(lo, hi, n), M.Grid(lo, hi, (10, 10, 10))
        want = ctx.extract_mesh(h, g, iso=iso, colours=True, simplify=clusters, quadric=True, keep=True, components=True, measures=True, project=True, occlusion=True)
        assert want.vertices > 0 and want.projection["moved_vertices"] > 0
        for k in ("positions", "normals", "colours", "triangles", "cells", "labels", "occlusion", "residual"):
            assert (tmp_path / ("a_" + k)).read_bytes() == getattr(want, k).tobytes(), k
        assert (tmp_path / "a_componentSizes").read_bytes() == want.component_sizes.tobytes() and reports[3] == want.measures["edges"]
        fine = ctx.extract_mesh(h, g, iso=iso, project=dict(rounds=2))
        for k in ("positions", "normals", "residual"):
            assert (tmp_path / ("b_" + k)).read_bytes() == getattr(fine, k).tobytes(), k
        for k in ("positions", "residual"):  # the slabbed extraction is the same mesh, and so is its projection
            assert (tmp_path / ("c_" + k)).read_bytes() == getattr(fine, k).tobytes(), k
        for got, report in ((reports[0], want.projection), (reports[1], fine.projection), (reports[2], fine.projection)):
            assert PR.same({k: got[c] for k, c in CAMEL.items()}, report) == [], (got, report)  # (a JSON number gives every double and float back)
    finally:
        h.destroy()


# ---- one measurement, no bar on time ------------------------------------------------------------------------------------------------------------

def test_measure_projection_on_the_mandelbulb_256_cubed(ctx):
    """Mandelbulb on 256^3 cells of [-1.25, 1.25]^3 at iso 2^-7, the fine mesh and the same mesh clustered at 64^3, strict and fast, at the defaults
    with the default reach.  Warmed once; median (min .. max) of five runs of the rounds slot of rm_mesh_timings, vertex evaluations per second
    (V * rounds_run / median), and beside it the host-clock time of the same rounds done by the restatement on downloaded positions: what its
    rm_probe calls alone take (upload, kernel, download), and the whole restatement with its numpy arithmetic.  Asserts only rms_after <
    rms_before."""
    lo, hi, iso = (-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), 0.0078125
    scene = ctx.create_scene(S.Mandelbulb())
    h = s = None
    try:
        fine_grid, cluster_grid = M.Grid(lo, hi, (256, 256, 256)), M.Grid(lo, hi, (64, 64, 64))
        h = from_scene(ctx, scene, fine_grid, iso=iso, normals=False)
        s = simplified(ctx, h, cluster_grid)
        ms = (C.c_float * 3)()
        print()
        for name, handle, grid in (("fine", h, fine_grid), ("clustered 64^3", s, cluster_grid)):
            for which, flags in (("strict", 0), ("fast", FAST)):
                block = M.mesh_project(iso=iso, reach=M.project_reach(grid), flags=flags)
                ctx.lib.rm_mesh_destroy(project(ctx, handle, scene, block)[0])
                times = []
                for _ in range(5):
                    out, report, residual = project(ctx, handle, scene, block)
                    assert ctx.lib.rm_mesh_timings(out, ms) == OK
                    times.append(float(ms[1]))
                    ctx.lib.rm_mesh_destroy(out)
                src = arrays(ctx, handle)
                spent = [0.0, 0.0]  # in the rm_probe calls alone; in the whole restatement

                def timed(what, q, **kw):
                    t = time.perf_counter()
                    out = ctx.probe(scene, what, q, flags=flags, **kw)
                    spent[0] += time.perf_counter() - t
                    return out

                t0 = time.perf_counter()
                want = PR.project(src["positions"], src["triangles"], lambda q: timed(abi.RM_PROBE_SDF, q),
                                  lambda q: timed(abi.RM_PROBE_NORMAL, q, param=block.normal_delta), iso=block.iso, rounds=block.rounds, relax=block.relax,
                                  tolerance=block.tolerance, reach=block.reach)
                spent[1] = time.perf_counter() - t0
                rate = report["vertices"] * report["rounds_run"] / (float(np.median(times)) * 1e-3)
                print(f"mandelbulb 256^3 iso 2^-7 {name} {which}: {report['vertices']} vertices, rounds_run {report['rounds_run']}, rounds slot {spread(times)} ms, "
                      f"{rate:.3g} vertex evaluations/s; the same rounds on the host: {spent[0] * 1e3:.1f} ms in rm_probe calls, {spent[1] * 1e3:.1f} ms the whole numpy restatement")
                print(f"  waves that skipped normals per round {['%.3f' % x for x in want['skipped_waves']]}, moved per round {want['moved']}, clamped "
                      f"{report['clamped_vertices']}, flipped {report['flipped_triangles']}")
                print(f"  max {report['max_before']:.3g} -> {report['max_after']:.3g}, rms {report['rms_before']:.3g} -> {report['rms_after']:.3g}")
                assert report["rms_after"] < report["rms_before"]
                assert PR.same(report, want["report"]) == [] and residual.tobytes() == want["residual"].tobytes()  # (this is also the large mesh's check)
    finally:
        for handle in (s, h):
            if handle is not None:
                ctx.lib.rm_mesh_destroy(handle)
        scene.destroy()
