"""The numpy restatement of include/hip_raymarch.h "quadric placement": rm_mesh_simplify_quadric.  Written from the header's definition, not
from the kernels: S is tests/mesh_simplify_ref.py's simplify, the planes are one float32 array operation per rounding, the sums np.add.at on
int64, and the solve is the Jacobi of tests/mesh_sharp_ref.py, vectorised over the clusters.  What the GPU is compared with, exactly."""
import numpy as np

import mesh_sharp_ref as SH
import mesh_simplify_ref as SR

F = np.float32
Q24 = F(16777216.0)


def q24(x):
    """(long long)rintf(x * 16777216.0f) of a float32 array"""
    return np.rint(np.asarray(x, F) * Q24).astype(np.int64)


def quadric_sums(lo, hi, n, positions, triangles):
    """Steps 1 to 3: (A [V', 6] int64 in the order 00 01 02 11 12 22, B [V', 3] int64, planes [V'] int64, g [V', 3] float32, the cell indices
    [V', 3] int64, h [3] float32)"""
    n64 = np.asarray(n, np.int64)
    p = np.asarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    key, q, h = SR.cluster_keys(lo, hi, n, p)
    keys, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    sums = np.zeros((len(keys), 3), np.int64)
    np.add.at(sums, inverse, q)
    g = (sums.astype(np.float64) / (counts.astype(np.float64)[:, None] * 1048576.0)).astype(F)
    idx = np.stack([keys % n64[0], (keys // n64[0]) % n64[1], keys // (n64[0] * n64[1])], -1)
    hmax = h[0]
    hmax = h[1] if h[1] > hmax else hmax
    hmax = h[2] if h[2] > hmax else hmax
    s = (h / hmax).astype(F)
    A, B, planes = np.zeros((len(keys), 6), np.int64), np.zeros((len(keys), 3), np.int64), np.zeros(len(keys), np.int64)
    t = t[(t < len(p)).all(axis=1)] if len(t) else t
    if len(t) == 0:
        return A, B, planes, g, idx, h
    with np.errstate(all="ignore"):
        p0, p1, p2 = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
        e1, e2 = (p1 - p0).astype(F), (p2 - p0).astype(F)
        cx = ((e1[:, 1] * e2[:, 2]).astype(F) - (e1[:, 2] * e2[:, 1]).astype(F)).astype(F)
        cy = ((e1[:, 2] * e2[:, 0]).astype(F) - (e1[:, 0] * e2[:, 2]).astype(F)).astype(F)
        cz = ((e1[:, 0] * e2[:, 1]).astype(F) - (e1[:, 1] * e2[:, 0]).astype(F)).astype(F)
        length = np.sqrt((((cx * cx).astype(F) + (cy * cy).astype(F)).astype(F) + (cz * cz).astype(F)).astype(F)).astype(F)
        ok = (length > 0) & np.isfinite(length)
        t, cx, cy, cz, length = t[ok], cx[ok], cy[ok], cz[ok], length[ok]
        m = [((c / length).astype(F) * s[a]).astype(F) for a, c in enumerate((cx, cy, cz))]
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        terms = np.stack([q24((m[i] * m[j]).astype(F)) for i, j in pairs], -1)
        for k in range(3):
            v = t[:, k]
            o = inverse[v]
            f = (q[v].astype(F) / F(1048576.0)).astype(F)
            d = (f - g[o]).astype(F)
            md = (((m[0] * d[:, 0]).astype(F) + (m[1] * d[:, 1]).astype(F)).astype(F) + (m[2] * d[:, 2]).astype(F)).astype(F)
            np.add.at(A, o, terms)
            np.add.at(B, o, np.stack([q24((m[a] * md).astype(F)) for a in range(3)], -1))
            np.add.at(planes, o, 1)
    return A, B, planes, g, idx, h


def solve(A, B, planes, g, threshold):
    """Step 4 up to the clamp: the fractions x [V', 3] float32 inside the cluster cells, and how many were clamped"""
    count = len(planes)
    with np.errstate(all="ignore"):
        a = (A.astype(np.float64) / 16777216.0).astype(F)
        b = (B.astype(np.float64) / 16777216.0).astype(F)
        a00, a01, a02, a11, a12, a22 = (a[:, k].copy() for k in range(6))
        b0, b1, b2 = b[:, 0], b[:, 1], b[:, 2]
        one, zero = np.ones(count, F), np.zeros(count, F)
        v = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]  # v[column][row]
        for _ in range(5):
            (a00, a11, a01, a02, a12), v[0], v[1] = SH._jacobi(a00, a11, a01, a02, a12, v[0], v[1])  # (0, 1), r = 2
            (a00, a22, a02, a01, a12), v[0], v[2] = SH._jacobi(a00, a22, a02, a01, a12, v[0], v[2])  # (0, 2), r = 1
            (a11, a22, a12, a01, a02), v[1], v[2] = SH._jacobi(a11, a22, a12, a01, a02, v[1], v[2])  # (1, 2), r = 0
        lam = [a00, a11, a22]
        lmax = a00
        lmax = np.where(a11 > lmax, a11, lmax)
        lmax = np.where(a22 > lmax, a22, lmax)
        bar = (F(threshold) * lmax).astype(F)
        w = [np.zeros(count, F) for _ in range(3)]
        for i in range(3):
            kept = (lam[i] > 0) & (lam[i] > bar)
            along = (((v[i][0] * b0).astype(F) + (v[i][1] * b1).astype(F)).astype(F) + (v[i][2] * b2).astype(F)).astype(F)
            along = (along / lam[i]).astype(F)
            for d in range(3):
                w[d] = np.where(kept, (w[d] + (v[i][d] * along).astype(F)).astype(F), w[d]).astype(F)
        x = [(g[:, d] + w[d]).astype(F) for d in range(3)]
        bad = ~(np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2]))
        clamped = np.zeros(count, bool)
        for d in range(3):
            x[d] = np.where(bad, g[:, d], x[d]).astype(F)
            clamped |= (planes > 0) & ((x[d] < 0) | (x[d] > 1))
            x[d] = np.where(x[d] < 0, F(0), x[d])
            x[d] = np.where(x[d] > 1, F(1), x[d]).astype(F)
    return np.stack(x, -1).astype(F), int(clamped.sum())


def simplify_quadric(lo, hi, n, positions, triangles, normals=None, colours=None, keep_duplicates=False, threshold=0.1):
    """SR.simplify's dict with the positions of rm_mesh_simplify_quadric; `plain`: S's positions, `planes` [V'] and `clamped` (a count) beside it"""
    out = SR.simplify(lo, hi, n, positions, triangles, normals, colours, keep_duplicates)
    A, B, planes, g, idx, h = quadric_sums(lo, hi, n, positions, triangles)
    x, clamped = solve(A, B, planes, g, threshold)
    placed = (idx.astype(F) + x).astype(F)
    step = (placed * h).astype(F)
    moved = (np.asarray(lo, F) + step).astype(F)
    out["plain"] = out["positions"]
    out["positions"] = np.where((planes > 0)[:, None], moved, out["plain"]).astype(F).reshape(-1, 3)
    out["planes"], out["clamped"] = planes, clamped
    return out


# the off-grid box: an edge or a corner of it lies inside most of the clusters it crosses
BOX_CENTRE, BOX_HALF = (0.031, -0.017, 0.023), (0.52, 0.41, 0.63)


def box_sdf(points):
    """the box's exact signed distance, float64"""
    q = np.abs(np.asarray(points, np.float64).reshape(-1, 3) - np.asarray(BOX_CENTRE, np.float64)) - np.asarray(BOX_HALF, np.float64)
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)


def box_field(n=48):
    """The box on [-1, 1]^3, n^3 cells, computed in float64 and stored as float32: (lo, hi, cells per axis, corner values)."""
    import mesh_ref as MR

    lo, hi, nn = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (n, n, n)
    d = box_sdf(MR.corner_positions(lo, hi, nn))
    return lo, hi, nn, d.astype(F).reshape(n + 1, n + 1, n + 1)


def sphere_sdf(points, centre=(0.03, -0.02, 0.01), radius=0.8):
    return np.linalg.norm(np.asarray(points, np.float64).reshape(-1, 3) - np.asarray(centre, np.float64), axis=1) - radius


# beside SR.CASES: (source field, cluster lo, hi, n), lo / hi None = the field's own box
BOX_CASES = {
    "box 48 -> 12": ("box 48", None, None, (12, 12, 12)),
    "box 48 -> unequal": ("box 48", None, None, (11, 9, 13)),
    "box 32 -> 8": ("box 32", None, None, (8, 8, 8)),
}
CASES = {**SR.CASES, **BOX_CASES}
# the cases in which no position moves: one vertex per cluster (every plane of a cluster passes through it), and the snake in one cluster (a
# symmetric tube whose mean already is the minimiser, to the bit)
UNMOVED = ("two balls 64", "snake one")


def fields():
    """SR.fields() and the boxes"""
    return {**SR.fields(), "box 48": lambda: box_field(48) + (0.0,), "box 32": lambda: box_field(32) + (0.0,)}
