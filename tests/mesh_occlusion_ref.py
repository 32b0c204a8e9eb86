"""Ambient occlusion in numpy, restated from the header's text alone (include/hip_raymarch.h "ambient occlusion"): fp32 with every operation
rounded on its own, the direction table in double.  The scene comes in as two callables on [N, 3] float32 points -- sdf(points) -> [N] and
normal(points) -> [N, 3] -- so the same text runs on analytic fields (the CPU tests) and on rm_probe (the GPU tests, bit for bit)."""
import numpy as np

F = np.float32
DIRECTIONS = (1, 2, 4, 8, 16, 32, 64)
TAPS = (1, 2, 4, 8)


def directions(K):
    """Step 1: [K, 4] float32 (x, y, z, 1 / z), each of x, y, z rounded once from double, the fourth from 1.0 / (double)z_float."""
    k = np.arange(K, dtype=np.float64)
    u = (k + 0.5) / K
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(u)
    z = np.sqrt(1.0 - u).astype(F)
    return np.stack([(r * np.cos(phi)).astype(F), (r * np.sin(phi)).astype(F), z, (1.0 / z.astype(np.float64)).astype(F)], axis=1)


def frame(n):
    """Step 3: the tangent and bitangent [N, 3] of the normals [N, 3]."""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    s = np.copysign(F(1), nz)
    a = F(-1) / (s + nz)
    b = (nx * ny) * a
    t = np.stack([F(1) + ((s * nx) * nx) * a, s * b, (-s) * nx], axis=1)
    bt = np.stack([b, s + (ny * ny) * a, -ny], axis=1)
    return t, bt


def quanta(positions, n, d0, sdf, table, radius, J):
    """Steps 3 and 4: the [V, K, J] uint32 quanta; the taps of all vertices and directions go to `sdf` in one call per j."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    V, K = len(p), len(table)
    radius = F(radius)
    inv_radius = F(1) / radius
    with np.errstate(all="ignore"):
        t, bt = frame(n)
        x, y, z, iz = (table[None, :, c] for c in range(4))
        w = [((x * t[:, c, None]) + (y * bt[:, c, None])) + (z * n[:, c, None]) for c in range(3)]  # [V, K] each
        out = np.zeros((V, K, J), np.uint32)
        for j in range(J):
            tj, itj = radius * F(2.0 ** -j), inv_radius * F(2.0 ** j)
            q = np.stack([p[:, c, None] + w[c] * tj for c in range(3)], axis=2).astype(F)  # [V, K, 3]
            d = np.asarray(sdf(np.ascontiguousarray(q.reshape(-1, 3))), F).reshape(V, K)
            e = z * tj
            ie = iz * itj
            o = ((d0[:, None] + e) - d) * ie
            o = np.where(o >= 0, o, F(0))  # (NaN too)
            o = np.where(o > 1, F(1), o)
            out[:, :, j] = (o * F(65536) + F(0.5)).astype(np.uint32)
    return out


def occlusion(positions, sdf, normal, table, radius=0.25, taps=4, strength=1.0):
    """The header's V floats (1 = open) for the scene given by sdf / normal, the direction table `table` [K, 4] and J = taps."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    table = np.asarray(table, F).reshape(-1, 4)
    K, J = len(table), int(taps)
    assert K in DIRECTIONS and J in TAPS
    if len(p) == 0:
        return np.zeros(0, F)
    n = np.asarray(normal(p), F).reshape(-1, 3)
    d0 = np.asarray(sdf(p), F).reshape(-1)
    S = quanta(p, n, d0, sdf, table, radius, J).reshape(len(p), -1).sum(axis=1, dtype=np.uint64)
    scale = F(2.0 ** -(16 + DIRECTIONS.index(K) + TAPS.index(J)))
    with np.errstate(all="ignore"):
        occ = S.astype(F) * scale  # (S <= 2^25: exact)
        ao = F(1) - F(strength) * occ
    ao = np.where(ao <= 1, ao, F(1))
    return np.where(ao < 0, F(0), ao).astype(F)
