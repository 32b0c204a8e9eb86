"""The numpy restatement of include/hip_raymarch.h "components and islands": the connected components of a triangle mesh, the keep rule and
the filtered arrays.  Written from the header's definitions, not from the device's procedure: every vertex carries the least vertex index it
has heard of, the edges pass the smaller one on (np.minimum.at) until nothing changes, and the components are the distinct values in ascending
order.  What the GPU is compared with, exactly."""
import numpy as np


def _edges(triangles):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, 0], t[:, 1], t[:, 2]]), np.concatenate([t[:, 1], t[:, 2], t[:, 0]])


def least_index(vertices, triangles, jump=True):
    """(least[v] = the smallest vertex index of v's component, the sweeps over the edges it took).  jump: between two sweeps every vertex also
    takes the value of the vertex it points at (that one lies in its component), which shortens long components; without it this is plain
    neighbour-minimum propagation, one edge per sweep along the longest component."""
    least = np.arange(int(vertices), dtype=np.int64)
    a, b = _edges(triangles)
    sweeps = 0
    while len(a):
        before = least.copy()
        m = np.minimum(least[a], least[b])
        np.minimum.at(least, a, m)
        np.minimum.at(least, b, m)
        if jump:
            least = least[least]
        sweeps += 1
        if np.array_equal(before, least):
            break
    return least, sweeps


def components(vertices, triangles):
    """(labels [V] uint32, sizes [C, 2] uint32): the components numbered in ascending order of their smallest vertex index; sizes are
    (vertices, triangles), a triangle belonging to the component of its vertices."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    least, _ = least_index(vertices, t)
    firsts, labels = np.unique(least, return_inverse=True)  # ascending: the smallest vertex index of each component
    count = len(firsts)
    sizes = np.zeros((count, 2), np.uint32)
    sizes[:, 0] = np.bincount(labels, minlength=count)
    if len(t):
        assert (labels[t[:, 0]] == labels[t[:, 1]]).all() and (labels[t[:, 0]] == labels[t[:, 2]]).all()
        sizes[:, 1] = np.bincount(labels[t[:, 0]], minlength=count)
    return labels.astype(np.uint32).reshape(-1), sizes


def keep_mask(sizes, min_triangles=1, largest=0):
    """[C] bool: a component passes iff triangles >= min_triangles; largest = k > 0 keeps only the first k passing components in the order
    (triangles descending, component index ascending)."""
    tri = np.asarray(sizes, np.int64).reshape(-1, 2)[:, 1]
    passing = np.flatnonzero(tri >= int(min_triangles))
    if int(largest) > 0:
        ranked = sorted(passing.tolist(), key=lambda c: (-int(tri[c]), c))
        passing = np.asarray(ranked[:int(largest)], np.int64)
    mask = np.zeros(len(tri), bool)
    mask[passing] = True
    return mask


def filter_arrays(mask, labels, positions, triangles, cells, normals=None, colours=None):
    """The filtered mesh as a dict of arrays: the kept vertices and triangles in their original relative order, indices renumbered, the
    per-vertex arrays carried as they are (None stays None)."""
    mask, labels = np.asarray(mask, bool), np.asarray(labels, np.int64)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    vertex_kept = mask[labels] if len(labels) else np.zeros(0, bool)
    triangle_kept = vertex_kept[t[:, 0].astype(np.int64)] if len(t) else np.zeros(0, bool)
    renumbered = np.cumsum(vertex_kept) - 1
    rows = lambda a, width: None if a is None else np.ascontiguousarray(np.asarray(a).reshape((-1,) + width)[vertex_kept])
    return dict(positions=rows(np.asarray(positions, np.float32), (3,)), triangles=renumbered[t[triangle_kept].astype(np.int64)].astype(np.uint32).reshape(-1, 3),
                cells=rows(np.asarray(cells, np.uint32), ()), normals=rows(normals, (3,)), colours=rows(colours, (3,)))


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------

def two_balls_field(n=16):
    """Two analytic spheres well apart on [-1, 1]^3, n^3 cells: (lo, hi, cells per axis, corner values [n + 1, n + 1, n + 1] float32)."""
    import mesh_ref as MR

    lo, hi, nn = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (n, n, n)
    p = MR.corner_positions(lo, hi, nn).astype(np.float64)
    d = np.minimum(np.linalg.norm(p - (-0.47, -0.03, 0.02), axis=1) - 0.31, np.linalg.norm(p - (0.49, 0.05, -0.04), axis=1) - 0.27)
    return lo, hi, nn, d.astype(np.float32).reshape(n + 1, n + 1, n + 1)


def snake_field():
    """Grid (32, 32, 6) cells on [-1, 1]^3, corner values +1 except two boustrophedon paths of -1 corners: plane k = 2, rows j = 2, 6, 10, 14
    along i = 2..30 joined by columns at alternating ends; plane k = 4, rows j = 18..30 step 4, mirrored.  Two long thin tubes."""
    nn = (32, 32, 6)
    v = np.ones((nn[2] + 1, nn[1] + 1, nn[0] + 1), np.float32)
    for k, rows, first_end in ((2, (2, 6, 10, 14), 30), (4, (18, 22, 26, 30), 2)):
        end = first_end
        for r, j in enumerate(rows):
            v[k, j, 2:31] = -1.0
            if r + 1 < len(rows):
                v[k, j:rows[r + 1] + 1, end] = -1.0
                end = 32 - end
    return (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), nn, v


def noise_field():
    """np.random.default_rng(3) standard normals as the field of (41, 41, 40) cells on [-1, 1]^3."""
    v = np.random.default_rng(3).standard_normal((41, 42, 42)).astype(np.float32)
    return (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (41, 41, 40), v


# the keep rules every mesh is filtered by: min_triangles at 0, 1, 12, 13 and beyond any component; largest 1, 2, 5; both together
KEEP_CASES = [dict(min_triangles=0), dict(), dict(min_triangles=12), dict(min_triangles=13), dict(min_triangles=1 << 30), dict(largest=1), dict(largest=2),
              dict(largest=5), dict(min_triangles=13, largest=5), dict(min_triangles=0, largest=3)]
