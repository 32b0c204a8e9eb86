"""Who owns what behind the mesh and probe entries, seen from outside: the probes' refusals with a live context, and meshes that give
their device memory back whichever way they end (made, filtered, refused half-way, destroyed in either order)."""
import ctypes as C

import numpy as np
import pytest

from raymarching_engine_amd import abi, mesh as M, native, scene as S
from test_mesh_cpu import c_grid

pytestmark = pytest.mark.gpu
F = np.float32
OK, INV = abi.RM_OK, abi.RM_ERR_INVALID


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def test_probe_refusals_with_a_live_context(ctx):
    lib = ctx.lib
    other = native.Context(0)
    h, foreign = ctx.create_scene(S.single_sphere((0.0, 0.0, 0.0), 0.8)), other.create_scene(S.single_sphere((0.0, 0.0, 0.0), 0.8))
    try:
        n = 5
        points = np.linspace(-1.0, 1.0, 3 * n, dtype=F)
        out = np.full(n, 1234.5, F)
        last = lambda: lib.rm_last_error(ctx.h).decode()
        assert lib.rm_probe(ctx.h, foreign.h, abi.RM_PROBE_SDF, native._fp(points), n, 0.0, 0, native._fp(out)) == INV
        assert last() == "rm_probe: the scene belongs to another context"
        for what in (-1, abi.RM_PROBE_CAST_SHADOW + 1):
            assert lib.rm_probe(ctx.h, h.h, what, native._fp(points), n, 0.0, 0, native._fp(out)) == INV
            assert last() == "rm_probe: unknown probe"
        assert lib.rm_probe(ctx.h, h.h, abi.RM_PROBE_SDF, native._fp(points), 0, 0.0, 0, native._fp(out)) == OK
        assert out.tobytes() == np.full(n, 1234.5, F).tobytes()  # nothing was written, by the refusals either
        a = np.linspace(0.5, 2.0, n, dtype=F)
        for name in ("pow", "atan2", "pow_pair_nm1", "pow_pair_n", "div"):
            assert lib.rm_probe_math(ctx.h, abi.RM_MATH_FUNCTIONS.index(name), native._fp(a), None, n, native._fp(out)) == INV
            assert last() == "rm_probe_math: this function takes two arguments"
        assert out.tobytes() == np.full(n, 1234.5, F).tobytes()
        # and the calls these refuse go through: the distances of a sphere of radius 0.8, a one-argument function without b
        assert lib.rm_probe(ctx.h, h.h, abi.RM_PROBE_SDF, native._fp(points), n, 0.0, 0, native._fp(out)) == OK
        want = np.linalg.norm(points.reshape(n, 3).astype(np.float64), axis=1) - 0.8
        assert np.abs(out - want).max() < 1e-5
        assert lib.rm_probe_math(ctx.h, abi.RM_MATH_FUNCTIONS.index("sqrt"), native._fp(a), None, n, native._fp(out)) == OK
        assert np.abs(out - np.sqrt(a.astype(np.float64))).max() < 1e-6
    finally:
        h.destroy()
        foreign.destroy()
        other.close()


# The sphere of radius 0.8 on [-1, 1]^3: one component, never empty.  Free device memory before and after CYCLES cycles differs by what
# the allocator of the runtime keeps or gives back in blocks of its own; BOUND is twice the largest |drift| of three runs of this test
# against the library before the mesh owned its arrays (0, 0 and 0 bytes: profiles/mesh_host_refactor.txt), and not below 2 MiB.
# The mesh has V = 12 368 vertices: its smallest owned array, the labels, leaked once per cycle is 4 V CYCLES bytes, which the test
# wants at twice the bound -- 3.0 MiB at 64 cycles is short of it, 4.5 MiB at 96 is not.
N, WARMUP, CYCLES = 64, 8, 96
BOUND = 2 * 2 ** 20


def test_meshes_give_their_memory_back(ctx):
    lib = ctx.lib
    h = ctx.create_scene(S.single_sphere((0.0, 0.0, 0.0), 0.8))
    g, bad_g = c_grid(lo=(-1, -1, -1), hi=(1, 1, 1), n=(N, N, N)), c_grid(lo=(-1, -1, -1), hi=(1, 1, 1), n=(0, N, N))
    p = M.mesh_params(normals=True, colours=True)
    largest, bad_keep = M.mesh_keep(largest=1), abi.RmMeshKeep(min_triangles=-1, largest=0)
    counts, parts = (C.c_ulonglong * 2)(), C.c_ulonglong()
    seen = {}

    def cycle(k):
        mesh, kept, none = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.rm_mesh_extract_sharp(ctx.h, h.h, C.byref(g), C.byref(p), None, C.byref(mesh)) == OK, lib.rm_last_error(ctx.h)
        assert lib.rm_mesh_components(mesh, C.byref(parts)) == OK and parts.value == 1
        assert lib.rm_mesh_filter(mesh, C.byref(largest), C.byref(kept)) == OK and kept.value
        assert lib.rm_mesh_counts(mesh, counts) == OK and counts[0] > 0 and counts[1] > 0
        v, t = int(counts[0]), int(counts[1])
        assert lib.rm_mesh_counts(kept, counts) == OK and (int(counts[0]), int(counts[1])) == (v, t)
        positions, triangles = np.empty((v, 3), F), np.empty((t, 3), np.uint32)
        assert lib.rm_mesh_download(mesh, abi.RM_MESH_POSITIONS, positions.ctypes.data_as(C.c_void_p), positions.nbytes) == OK
        assert lib.rm_mesh_download(kept, abi.RM_MESH_TRIANGLES, triangles.ctypes.data_as(C.c_void_p), triangles.nbytes) == OK
        assert lib.rm_mesh_download(mesh, abi.RM_MESH_POSITIONS, positions.ctypes.data_as(C.c_void_p), positions.nbytes - 1) == INV
        assert lib.rm_mesh_filter(mesh, C.byref(bad_keep), C.byref(none)) == INV and not none.value
        assert lib.rm_mesh_extract_sharp(ctx.h, h.h, C.byref(bad_g), C.byref(p), None, C.byref(none)) == INV and not none.value
        for handle in ((mesh, kept) if k % 2 else (kept, mesh)):
            lib.rm_mesh_destroy(handle)
        seen.update(v=v, t=t, triangles=triangles)

    try:
        for k in range(WARMUP):
            cycle(k)
        free0 = ctx.device_memory()[0]
        for k in range(CYCLES):
            cycle(k)
        free1 = ctx.device_memory()[0]
    finally:
        h.destroy()
    v, drift = seen["v"], free1 - free0
    assert int(seen["triangles"].max()) == v - 1  # (the last download is a whole mesh)
    print(f"\n{v} vertices, {seen['t']} triangles; free device memory after {CYCLES} cycles: {drift / 2**20:+.3f} MiB ({drift} bytes); "
          f"one labels array per cycle would be {CYCLES * 4 * v / 2**20:.3f} MiB; the bound is {BOUND / 2**20:.0f} MiB")
    assert CYCLES * 4 * v >= 2 * BOUND  # the smallest owned array (the labels, 4 V bytes) leaked once per cycle would show twofold
    assert abs(drift) < BOUND
