"""The numpy restatement of include/hip_raymarch.h "slabbed extraction": the two passes over windows of z layers -- tally, bases, emit with a
halo layer, empty slabs skipped -- in mesh_ref's arithmetic.  A window's arrays are indexed from its first plane, as the kernels index them;
what it gives has to be mesh_ref.surface_nets' arrays, whatever `layers` is."""
import numpy as np

import mesh_ref

F = np.float32


def slab_layers(n, layers, budget=1 << 26):
    """RmMeshSlabs' rule: the cell layers per slab for `layers` (0 = the largest whose window stays within `budget` corners), in 1..nz;
    ValueError where the library refuses."""
    nx, ny, nz = (int(v) for v in n)
    if layers < 0:
        raise ValueError("slabs layers must be >= 0")
    plane = (nx + 1) * (ny + 1)
    L = layers if layers > 0 else budget // plane - 2
    L = min(max(L, 1), nz)
    if (L + 2) * plane > 1 << 28:
        raise ValueError("slab window must be at most 2^28 corners")
    return L


def _window(coords, n, window, iso, plane0):
    """The cells of a window of planes ([planes, ny + 1, nx + 1], the first one the grid's plane `plane0`), as [layers, ny, nx] arrays:
    active, the quads' mask per axis (by the indices in the WHOLE grid), the low corner's `inside`, and the vertex positions [.., 3]."""
    nx, ny = n[0], n[1]
    nzw = window.shape[0] - 1
    wn = (nx, ny, nzw)
    with np.errstate(all="ignore"):
        e = (window - F(iso)).astype(F)
        inside = e < 0
    ins = {(dx, dy, dz): mesh_ref._corner(inside, (dx, dy, dz), wn) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    ee = {k: mesh_ref._corner(e, k, wn) for k in ins}
    count = sum(c.astype(np.int32) for c in ins.values())
    active = (count > 0) & (count < 8)
    shape = (nzw, ny, nx)
    view = {0: (1, 1, nx), 1: (1, ny, 1), 2: (nzw, 1, 1)}
    local = [coords[0], coords[1], coords[2][plane0:plane0 + nzw + 1]]  # (a plane's coordinate by its index in the whole grid)
    pc = [[np.broadcast_to(local[a][d:d + wn[a]].reshape(view[a]), shape) for d in (0, 1)] for a in range(3)]
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
        positions = np.stack([(s[k] / m.astype(F)).astype(F) for k in range(3)], -1)
    idx = np.meshgrid(np.arange(plane0, plane0 + nzw), np.arange(ny), np.arange(nx), indexing="ij")
    index_of = {0: idx[2], 1: idx[1], 2: idx[0]}
    low = ins[(0, 0, 0)]
    quads = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        k1 = [0, 0, 0]
        k1[a] = 1
        quads.append((low != ins[tuple(k1)]) & (index_of[b] >= 1) & (index_of[c] >= 1))
    return active, quads, low, positions


def surface_nets_slabs(lo, hi, n, values, iso=0.0, layers=0, stats=None):
    """mesh_ref.surface_nets' (positions, triangles, cells) by the slabbed procedure.  stats (a dict, when given) receives the slabs'
    totals [(vertices, quads)] of the tally pass and the indices of the slabs the emit pass skipped."""
    n = tuple(int(v) for v in n)
    nx, ny, nz = n
    L = slab_layers(n, layers)
    v = np.ascontiguousarray(values, F).reshape(nz + 1, ny + 1, nx + 1)
    coords = mesh_ref.axes(lo, hi, n)
    layer = nx * ny
    starts = list(range(0, nz, L))
    # the tally pass: a slab's own planes
    totals = []
    for k0 in starts:
        own = min(L, nz - k0)
        active, quads, _, _ = _window(coords, n, v[k0:k0 + own + 1], iso, k0)
        totals.append((int(active.sum()), int(sum(q.sum() for q in quads))))
    V, Q = sum(t[0] for t in totals), sum(t[1] for t in totals)
    positions = np.zeros((V, 3), F)
    cells = np.zeros(V, np.uint32)
    triangles = np.zeros((2 * Q, 3), np.uint32)
    # the emit pass: the window begins one layer earlier, at the halo
    vertex_base = quad_base = 0
    skipped = []
    for s, k0 in enumerate(starts):
        if totals[s][0] == 0:
            skipped.append(s)
            continue
        own = min(L, nz - k0)
        plane0 = k0 - 1 if k0 > 0 else 0
        halo = (k0 - plane0) * layer
        active, quads, low, pos = _window(coords, n, v[plane0:k0 + own + 1], iso, plane0)
        flat = active.reshape(-1)
        counts_v = flat.astype(np.int64)
        counts_q = sum(q.reshape(-1).astype(np.int64) for q in quads)
        scan_v = np.cumsum(counts_v) - counts_v  # exclusive
        scan_q = np.cumsum(counts_q) - counts_q
        shift = vertex_base - scan_v[halo]
        own_cells = np.flatnonzero(flat)
        own_cells = own_cells[own_cells >= halo]  # halo cells emit nothing
        vertex = scan_v[own_cells] + shift
        positions[vertex] = pos.reshape(-1, 3)[own_cells]
        cells[vertex] = own_cells + plane0 * layer  # the index in the whole grid
        stride = (1, nx, layer)
        lowf = low.reshape(-1)
        at = 2 * (quad_base + scan_q - scan_q[halo])
        for t in own_cells[counts_q[own_cells] > 0]:
            tri = at[t]
            for a in range(3):
                if not quads[a].reshape(-1)[t]:
                    continue
                sb, sc = stride[(a + 1) % 3], stride[(a + 2) % 3]
                q0, q1, q2, q3 = (scan_v[t - sb - sc] + shift, scan_v[t - sc] + shift, scan_v[t] + shift, scan_v[t - sb] + shift)
                assert flat[t - sb - sc] and flat[t - sc] and flat[t - sb]  # every cell round a crossing edge is active
                triangles[tri:tri + 2] = [[q0, q1, q2], [q0, q2, q3]] if lowf[t] else [[q0, q3, q2], [q0, q2, q1]]
                tri += 2
        vertex_base += totals[s][0]
        quad_base += totals[s][1]
    assert vertex_base == V and quad_base == Q
    if stats is not None:
        stats.update(totals=totals, skipped=skipped, layers=L)
    return positions, triangles, cells
