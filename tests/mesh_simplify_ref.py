"""The numpy restatement of include/hip_raymarch.h "simplification": vertex clustering of a triangle mesh.  Written from the header's
definition, not from the device's procedure: the occupied clusters are np.unique of the keys, the sums np.add.at on int64, the duplicates
np.unique of the canonical triples (whose first occurrence is the smallest source index), and every fp32 rounding of the definition is a float32
array operation of its own.  What the GPU is compared with, exactly."""
import numpy as np

F = np.float32
Q = F(1048576.0)


def q20(x):
    """(long long)rintf(x * 1048576.0f) of a float32 array"""
    return np.rint(np.asarray(x, F) * Q).astype(np.int64)


def cluster_keys(lo, hi, n, positions):
    """(key [V] int64, q [V, 3] int64, h [3] float32) of the definition's step 1"""
    lo, hi, n = np.asarray(lo, F), np.asarray(hi, F), np.asarray(n, np.int64)
    h = (hi - lo) / n.astype(F)
    p = np.asarray(positions, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = (p - lo) / h
        below, above = ~(u >= 0), u >= n.astype(F)
        inside = ~below & ~above
        floor = np.minimum(np.floor(np.where(inside, u, F(0))).astype(np.int64), n - 1)
        i = np.where(below, 0, np.where(above, n - 1, floor))
        f = u - i.astype(F)
        f = np.where(~(f >= 0), F(0), f)
        f = np.where(f > 1, F(1), f).astype(F)
    key = (i[:, 2] * n[1] + i[:, 1]) * n[0] + i[:, 0]
    return key, q20(f), h


def _means(sums, counts):
    return (sums.astype(np.float64) / (counts.astype(np.float64)[:, None] * 1048576.0)).astype(F)


def _attribute_means(x, inverse, counts):
    x = np.asarray(x, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x = np.clip(np.where(np.isfinite(x), x, F(0)), F(-1024), F(1024)).astype(F)
    sums = np.zeros((len(counts), 3), np.int64)
    np.add.at(sums, inverse, q20(x))
    return _means(sums, counts)


def canonical(triangles):
    """every row rotated so that its smallest index stands in front, the cyclic order kept"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    first = np.argmin(t, axis=1)
    rows = np.arange(len(t))
    return np.stack([t[rows, first], t[rows, (first + 1) % 3], t[rows, (first + 2) % 3]], -1)


def simplify(lo, hi, n, positions, triangles, normals=None, colours=None, keep_duplicates=False):
    """The simplified mesh as a dict: positions, triangles, cells, normals, colours (None stays None), and the counts `collapsed` (triangles with
    two equal corners) and `duplicates` (survivors that repeat an earlier one; dropped unless keep_duplicates)."""
    lo32, n64 = np.asarray(lo, F), np.asarray(n, np.int64)
    p = np.asarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    key, q, h = cluster_keys(lo, hi, n, p)
    keys, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)  # ascending key
    inverse = inverse.reshape(-1)
    sums = np.zeros((len(keys), 3), np.int64)
    np.add.at(sums, inverse, q)
    idx = np.stack([keys % n64[0], (keys // n64[0]) % n64[1], keys // (n64[0] * n64[1])], -1)
    placed = idx.astype(F) + _means(sums, counts)
    step = placed * h
    out = dict(positions=(lo32 + step).astype(F).reshape(-1, 3), cells=keys.astype(np.uint32), normals=None, colours=None)
    if normals is not None:
        m = _attribute_means(normals, inverse, counts)
        with np.errstate(all="ignore"):
            xx, yy, zz = m[:, 0] * m[:, 0], m[:, 1] * m[:, 1], m[:, 2] * m[:, 2]
            length = np.sqrt((xx + yy) + zz)
            none = (length == 0) | ~np.isfinite(length)
            out["normals"] = np.where(none[:, None], F(0), m / length[:, None]).astype(F)
    if colours is not None:
        out["colours"] = _attribute_means(colours, inverse, counts)
    mapped = inverse[t] if len(t) else np.zeros((0, 3), np.int64)
    survives = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    survivors = np.flatnonzero(survives)
    forms, count = canonical(mapped[survivors]), len(keys)
    if count ** 3 < 2 ** 62:  # the triple as one number: the same classes, a faster sort
        forms = (forms[:, 0] * count + forms[:, 1]) * count + forms[:, 2]
    _, first = np.unique(forms, axis=0, return_index=True) if len(survivors) else (None, np.zeros(0, np.int64))
    kept = survivors if keep_duplicates else survivors[np.sort(first)]
    out["triangles"] = mapped[kept].astype(np.uint32).reshape(-1, 3)
    out["collapsed"], out["duplicates"] = int(len(t) - len(survivors)), int(len(survivors) - len(first))
    return out


def box_of(lo, hi, n, cells):
    """(low, high) [V, 3] float32: the closed box of each linear cell index, by the library's corner arithmetic lo + i * h"""
    lo32, n64 = np.asarray(lo, F), np.asarray(n, np.int64)
    h = (np.asarray(hi, F) - lo32) / n64.astype(F)
    c = np.asarray(cells, np.int64)
    idx = np.stack([c % n64[0], (c // n64[0]) % n64[1], c // (n64[0] * n64[1])], -1)
    return lo32 + idx.astype(F) * h, lo32 + (idx + 1).astype(F) * h


def edge_uses(triangles):
    """the number of triangles at each undirected edge"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(axis=1)
    return np.unique(e, axis=0, return_counts=True)


def sphere_field(n=48, centre=(0.03, -0.02, 0.01), radius=0.8):
    """An analytic sphere on [-1, 1]^3, n^3 cells, computed in float64 and stored as float32: (lo, hi, cells per axis, corner values)."""
    import mesh_ref as MR

    lo, hi, nn = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (n, n, n)
    p = MR.corner_positions(lo, hi, nn).astype(np.float64)
    d = np.linalg.norm(p - np.asarray(centre, np.float64), axis=1) - radius
    return lo, hi, nn, d.astype(F).reshape(n + 1, n + 1, n + 1)


# the rows of the issue's table: (source field, cluster lo, hi, n); lo / hi None = the field's own box
HALF = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
CASES = {
    "noise 128": ("noise 0.25", None, None, (128, 128, 128)),
    "noise 20": ("noise 0.25", None, None, (20, 20, 20)),
    "noise 8 half": ("noise 0.25",) + HALF + ((8, 8, 8),),
    "noise unequal": ("noise 0.25", None, None, (37, 29, 53)),
    "noise one": ("noise 0.25", None, None, (1, 1, 1)),
    "two balls 64": ("two balls", None, None, (64, 64, 64)),
    "two balls one": ("two balls", None, None, (1, 1, 1)),
    "snake 8 half": ("snake",) + HALF + ((8, 8, 8),),
    "snake one": ("snake", None, None, (1, 1, 1)),
    "sphere 12": ("sphere", None, None, (12, 12, 12)),
    "sphere 16": ("sphere", None, None, (16, 16, 16)),
}


def fields():
    """name -> a function giving (lo, hi, n, corner values, iso): the inputs the CPU and the GPU tests share"""
    import mesh_parts_ref as PR

    return {"noise 0.25": lambda: PR.noise_field() + (0.25,), "two balls": lambda: PR.two_balls_field() + (0.0,), "snake": lambda: PR.snake_field() + (0.0,),
            "sphere": lambda: sphere_field() + (0.0,)}
