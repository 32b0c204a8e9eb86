"""Every row of the one kind selection (rm_kernels.inc launch_point_kind) gives the probe's bits through every launcher that uses it: the grid
sampler against rm_probe(RM_PROBE_SDF) at the corners, and rm_mesh_occlusion, rm_mesh_project and rm_mesh_deviation against their numpy
restatements fed from rm_probe, exactly as the bit-for-bit tests of those entries feed them.  One scene per row, in the strict, fast and
GL-stack units.  The inputs are the smallest launches there are and do not depend on the scene, so no scene can leave them empty: a (3, 2, 2)
grid of 36 corners, a mesh of one vertex, a mesh of 8 vertices and 12 triangles -- each pass a single partial wave, where a wrong row or a wrong
tail guard would show.  Every comparison of floats is of their bits, a NaN matching a NaN."""
import numpy as np
import pytest

import mesh_ref as MR
from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_gpu_mesh import bits, same_floats
from test_gpu_mesh_deviation import check as deviation_is_restated, twelve_triangles
from test_gpu_mesh_occlusion import check as occlusion_is_restated, one_vertex
from test_gpu_mesh_parts import counts
from test_gpu_mesh_project import check as projection_is_restated

pytestmark = pytest.mark.gpu
FAST, NO_CULL = abi.RM_RENDER_FAST, abi.RM_RENDER_NO_CULL

# the rows of the selection, in its order: a table with kind rows, a table of >= 16 rows (with the culling grid and without), a short plain
# table, and the six other kinds
SCENES = [("kind rows", lambda: S.CsgScene().shape(S.Mandelbulb()).intersect().box((0.0, 0.0, 0.25), (1.25, 1.25, 0.75)), (0,)),
          ("csg64", lambda: S.csg64(), (0, NO_CULL)),
          ("short table", lambda: S.single_sphere((0.125, -0.0625, 0.1875), 0.875), (0,)),
          ("mandelbulb", lambda: S.Mandelbulb(), (0,)),
          ("sphere grid", lambda: S.SphereGridFractal(), (0,)),
          ("sphere lattice", lambda: S.SphereLattice(), (0,)),
          ("menger", lambda: S.MengerSponge(), (0,)),
          ("kifs tree", lambda: S.KifsTree(), (0,)),
          ("kifs box", lambda: S.KifsBox(), (0,))]
# the box of one_vertex and twelve_triangles, in the middle of the scenes; 4 x 3 x 3 = 36 corners
LO, HI, CELLS = (-0.75, -0.5, -0.625), (0.5, 0.75, 0.625), (3, 2, 2)
CORNERS = MR.corner_positions(LO, HI, CELLS)
PROBED = {}  # scene name -> the strict probe's bits at the corners, for the condition on the inputs below


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


@pytest.mark.parametrize("name, make, cull_flags", SCENES, ids=[s[0] for s in SCENES])
def test_every_launcher_gives_the_probes_bits(ctx, gl_ctx, name, make, cull_flags):
    grid = M.Grid(LO, HI, CELLS)
    assert grid.corners == len(CORNERS) == 36
    for which, c, arithmetic in (("strict", ctx, 0), ("fast", ctx, FAST), ("gl stack", gl_ctx, 0)):
        scene = c.create_scene(make())
        vertex, cube = one_vertex(c), twelve_triangles(c)
        try:
            assert counts(c, vertex) == (1, 0) and counts(c, cube) == (8, 12)
            for cull in cull_flags:
                flags = arithmetic | cull
                want = c.probe(scene, abi.RM_PROBE_SDF, CORNERS, flags=flags)
                # a condition on the inputs, from the probe alone: a test that compared nothing but NaNs or infinities would hide a wrong row
                assert np.isfinite(want).any(), (name, which, flags)
                if which == "strict" and cull == 0:
                    PROBED[name] = bits(want).tobytes()
                got = c.sdf_grid(scene, grid, flags)
                assert got.shape == grid.shape and same_floats(got.reshape(-1), want), (name, which, flags, int((bits(got.reshape(-1)) != bits(want)).sum()))
                # lanes: 1 x 16 and 8 x 4 rays, 1 and 8 vertices, 12 x 1 and 12 x 4 samples -- all below one wave
                occlusion_is_restated(c, vertex, scene, flags=flags)
                occlusion_is_restated(c, cube, scene, directions=4, flags=flags)
                projection_is_restated(c, vertex, scene, flags=flags)
                projection_is_restated(c, cube, scene, flags=flags)
                deviation_is_restated(c, cube, scene, order=1, flags=flags)
                deviation_is_restated(c, cube, scene, order=2, flags=flags)
        finally:
            c.lib.rm_mesh_destroy(vertex)
            c.lib.rm_mesh_destroy(cube)
            scene.destroy()


def test_the_scenes_differ_at_the_corners(ctx):
    """The other condition on the inputs: the nine scenes do not all yield the same bits at the grid's corners (comparing constants would hide a
    wrong row).  From the probe's output alone; a scene the test above has not probed in this run is probed here."""
    for name, make, _ in SCENES:
        if name not in PROBED:
            scene = ctx.create_scene(make())
            try:
                PROBED[name] = bits(ctx.probe(scene, abi.RM_PROBE_SDF, CORNERS)).tobytes()
            finally:
                scene.destroy()
    assert len(PROBED) == len(SCENES) == 9
    assert len(set(PROBED.values())) > 1, sorted(PROBED)
