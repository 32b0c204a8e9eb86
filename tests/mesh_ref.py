"""The numpy restatement of the grid and the surface-nets mesher of include/hip_raymarch.h "mesh extraction": fp32 throughout, every
operation rounded on its own, vectorised over the cells (twelve masked steps, one per edge of a cell).  What the GPU is compared with."""
import numpy as np

F = np.float32


def axis(lo, hi, n):
    """Corner i of an axis: lo + (float)i * h, h = (hi - lo) / (float)n."""
    lo, hi = F(lo), F(hi)
    h = (hi - lo) / F(n)
    return (lo + np.arange(n + 1, dtype=F) * h).astype(F)


def axes(lo, hi, n):
    return [axis(lo[a], hi[a], n[a]) for a in range(3)]


def corner_positions(lo, hi, n):
    """[corners, 3] float32, x fastest: the points at which the sampler evaluates the scene."""
    x, y, z = axes(lo, hi, n)
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(F)


def _corner(a3, offsets, n):
    """The [nz, ny, nx] view of a corner array [nz + 1, ny + 1, nx + 1] at the cells' corner (dx, dy, dz)."""
    dx, dy, dz = offsets
    return a3[dz:dz + n[2], dy:dy + n[1], dx:dx + n[0]]


def surface_nets(lo, hi, n, values, iso=0.0):
    """positions [V, 3] float32, triangles [T, 3] uint32, cells [V] uint32, in the order the header states."""
    n = tuple(int(v) for v in n)
    nx, ny, nz = n
    v = np.ascontiguousarray(values, F).reshape(nz + 1, ny + 1, nx + 1)
    with np.errstate(all="ignore"):
        e = (v - F(iso)).astype(F)
        inside = e < 0  # NaN, +0 and -0 are outside
    coords = axes(lo, hi, n)
    # per cell: the corners' `inside` and e, by offset
    ins = {}
    ee = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ins[(dx, dy, dz)] = _corner(inside, (dx, dy, dz), n)
                ee[(dx, dy, dz)] = _corner(e, (dx, dy, dz), n)
    count = sum(c.astype(np.int32) for c in ins.values())
    active = (count > 0) & (count < 8)
    # the coordinate of the cells' low / high corner along every axis, broadcast to [nz, ny, nx]
    shape = (nz, ny, nx)
    view = {0: (1, 1, nx), 1: (1, ny, 1), 2: (nz, 1, 1)}
    pc = [[np.broadcast_to(coords[a][d:d + n[a]].reshape(view[a]), shape) for d in (0, 1)] for a in range(3)]
    s = [np.zeros(shape, F) for _ in range(3)]
    m = np.zeros(shape, np.int32)
    with np.errstate(all="ignore"):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for ob, oc in ((0, 0), (1, 0), (0, 1), (1, 1)):
                k0 = [0, 0, 0]
                k0[b], k0[c] = ob, oc
                k1 = list(k0)
                k1[a] = 1
                k0, k1 = tuple(k0), tuple(k1)
                cross = ins[k0] != ins[k1]
                e0, e1 = ee[k0], ee[k1]
                t = (e0 / (e0 - e1)).astype(F)
                t = np.where((t >= 0) & (t <= 1), t, F(0.5)).astype(F)
                p = [None, None, None]
                p[a] = (pc[a][0] + (t * (pc[a][1] - pc[a][0]).astype(F)).astype(F)).astype(F)
                p[b] = pc[b][ob]
                p[c] = pc[c][oc]
                for k in range(3):
                    s[k] = np.where(cross, (s[k] + p[k]).astype(F), s[k])
                m += cross
        flat = active.reshape(-1)
        cells = np.flatnonzero(flat).astype(np.uint32)
        mf = m.reshape(-1)[flat].astype(F)
        positions = np.stack([(s[k].reshape(-1)[flat] / mf).astype(F) for k in range(3)], -1).astype(F).reshape(-1, 3)
    vertex_of = np.full(nx * ny * nz, -1, np.int64)
    vertex_of[cells] = np.arange(len(cells))
    vertex_of = vertex_of.reshape(shape)
    # faces: per cell and axis, then put in cell order (a stable sort by (cell, axis))
    lin = np.arange(nx * ny * nz, dtype=np.int64).reshape(shape)
    idx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")  # [z, y, x] index arrays
    index_of = {0: idx[2], 1: idx[1], 2: idx[0]}
    keys, tris = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        k1 = [0, 0, 0]
        k1[a] = 1
        low = ins[(0, 0, 0)]
        emit = (low != ins[tuple(k1)]) & (index_of[b] >= 1) & (index_of[c] >= 1)
        where = np.nonzero(emit)
        if len(where[0]) == 0:
            continue

        def neighbour(db, dc):
            z, y, x = [w.copy() for w in where]
            at = {0: x, 1: y, 2: z}
            at[b] += db
            at[c] += dc
            return vertex_of[at[2], at[1], at[0]]

        q0, q1, q2, q3 = neighbour(-1, -1), neighbour(0, -1), neighbour(0, 0), neighbour(-1, 0)
        assert (np.stack([q0, q1, q2, q3]) >= 0).all()  # every cell round a crossing edge is active
        lw = low[where]
        first = np.where(lw[:, None], np.stack([q0, q1, q2], -1), np.stack([q0, q3, q2], -1))
        second = np.where(lw[:, None], np.stack([q0, q2, q3], -1), np.stack([q0, q2, q1], -1))
        keys.append(lin[where] * 3 + a)
        tris.append(np.stack([first, second], 1))  # [quads, 2, 3]
    if keys:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        triangles = tris[np.argsort(keys, kind="stable")].reshape(-1, 3).astype(np.uint32)
    else:
        triangles = np.zeros((0, 3), np.uint32)
    return positions, triangles, cells


# ---- what a closed, oriented surface satisfies (the tests' invariants) ---------------------------------------------------------

def edge_counts(triangles):
    """(undirected edge -> count, directed edge -> count) as dicts of numpy-unique results: (keys, counts) pairs."""
    t = np.asarray(triangles, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    big = int(t.max()) + 1 if len(t) else 1
    directed = d[:, 0] * big + d[:, 1]
    undirected = np.minimum(d[:, 0], d[:, 1]) * big + np.maximum(d[:, 0], d[:, 1])
    return np.unique(undirected, return_counts=True), np.unique(directed, return_counts=True), big


def directed_balanced(triangles) -> bool:
    """Every directed edge (a, b) occurs as often as (b, a)."""
    _, (keys, counts), big = edge_counts(triangles)
    rev = (keys % big) * big + keys // big
    order = np.argsort(rev)
    return bool(np.array_equal(rev[order], keys) and np.array_equal(counts[order], counts))


def euler(positions, triangles) -> int:
    (ukeys, _), _, _ = edge_counts(triangles)
    used = len(np.unique(np.asarray(triangles)))
    return used - len(ukeys) + len(triangles)


def signed_volume(positions, triangles) -> float:
    p = np.asarray(positions, np.float64)
    a, b, c = p[triangles[:, 0]], p[triangles[:, 1]], p[triangles[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def inside_cell_boxes(lo, hi, n, positions, cells) -> bool:
    """Every vertex lies in the closed box of its cell."""
    x, y, z = axes(lo, hi, n)
    c = np.asarray(cells, np.int64)
    i, j, k = c % n[0], (c // n[0]) % n[1], c // (n[0] * n[1])
    p = np.asarray(positions)
    ok = (p[:, 0] >= x[i]) & (p[:, 0] <= x[i + 1]) & (p[:, 1] >= y[j]) & (p[:, 1] <= y[j + 1]) & (p[:, 2] >= z[k]) & (p[:, 2] <= z[k + 1])
    return bool(ok.all())
