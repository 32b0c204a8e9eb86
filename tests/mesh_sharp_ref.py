"""The numpy restatement of include/hip_raymarch.h "sharp vertices", steps 2 to 5: fp32 throughout, every operation rounded on its own, in the
header's order, vectorised over the vertices (twelve masked steps per stage, one per slot; the Jacobi sweeps are a fixed count).  The scene
comes in as two callables, so the same text serves an analytic field on the CPU and the library's own probes on the GPU."""
import numpy as np

F = np.float32
SLOTS = [(a, ob, oc) for a in range(3) for ob, oc in ((0, 0), (1, 0), (0, 1), (1, 1))]  # the mesher's edge order


def _jacobi(app, aqq, apq, arp, arq, vp, vq):
    """One rotation of the pair (p, q), r the third index; vp, vq: the columns p and q of V as lists of three arrays.  Where a_pq == 0 nothing
    changes."""
    go = apq != 0
    theta = ((aqq - app) / (F(2) * apq)).astype(F)
    t = (np.copysign(F(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + F(1)))).astype(F)
    cr = (F(1) / np.sqrt(t * t + F(1))).astype(F)
    sr = t * cr
    h = t * apq
    pick = lambda new, old: np.where(go, new, old).astype(F)
    out = [pick(app - h, app), pick(aqq + h, aqq), pick(F(0), apq), pick(cr * arp - sr * arq, arp), pick(sr * arp + cr * arq, arq)]
    new_vp = [pick(cr * vp[k] - sr * vq[k], vp[k]) for k in range(3)]
    new_vq = [pick(sr * vp[k] + cr * vq[k], vq[k]) for k in range(3)]
    return out, new_vp, new_vq


def qef_vertex(points, normals, live, lo, hi, threshold):
    """Steps 3 and 5 on given slot arrays: points [12, V, 3] and normals [12, V, 3] float32, live [12, V] bool, the cells' corner coordinates
    lo, hi [V, 3].  Returns (positions [V, 3], mass points [V, 3])."""
    V = points.shape[1]
    with np.errstate(all="ignore"):
        s = [np.zeros(V, F) for _ in range(3)]
        m = np.zeros(V, np.int32)
        for k in range(12):
            for d in range(3):
                s[d] = np.where(live[k], s[d] + points[k, :, d], s[d]).astype(F)
            m += live[k]
        c = [(s[d] / m.astype(F)).astype(F) for d in range(3)]
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = (np.zeros(V, F) for _ in range(9))
        planes = np.zeros(V, np.int32)
        for k in range(12):
            nx, ny, nz = (normals[k, :, d] for d in range(3))
            ok = live[k] & np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz) & ~((nx == 0) & (ny == 0) & (nz == 0))
            dx, dy, dz = ((points[k, :, d] - c[d]).astype(F) for d in range(3))
            nd = (nx * dx + ny * dy + nz * dz).astype(F)  # ((nx dx) + (ny dy)) + (nz dz)
            add = lambda acc, term: np.where(ok, acc + term, acc).astype(F)
            a00, a01, a02, a11, a12, a22 = add(a00, nx * nx), add(a01, nx * ny), add(a02, nx * nz), add(a11, ny * ny), add(a12, ny * nz), add(a22, nz * nz)
            b0, b1, b2 = add(b0, nx * nd), add(b1, ny * nd), add(b2, nz * nd)
            planes += ok
        one, zero = np.ones(V, F), np.zeros(V, F)
        v = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]  # v[column][row]
        for _ in range(5):
            (a00, a11, a01, a02, a12), v[0], v[1] = _jacobi(a00, a11, a01, a02, a12, v[0], v[1])  # (0, 1), r = 2
            (a00, a22, a02, a01, a12), v[0], v[2] = _jacobi(a00, a22, a02, a01, a12, v[0], v[2])  # (0, 2), r = 1
            (a11, a22, a12, a01, a02), v[1], v[2] = _jacobi(a11, a22, a12, a01, a02, v[1], v[2])  # (1, 2), r = 0
        lam = [a00, a11, a22]
        lmax = a00
        lmax = np.where(a11 > lmax, a11, lmax)
        lmax = np.where(a22 > lmax, a22, lmax)
        bar = (F(threshold) * lmax).astype(F)
        o = [np.zeros(V, F) for _ in range(3)]
        for i in range(3):
            kept = (lam[i] > 0) & (lam[i] > bar)
            w = ((v[i][0] * b0 + v[i][1] * b1 + v[i][2] * b2) / lam[i]).astype(F)
            for d in range(3):
                o[d] = np.where(kept, o[d] + v[i][d] * w, o[d]).astype(F)
        x = [(c[d] + o[d]).astype(F) for d in range(3)]
        bad = (planes == 0) | ~(np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2]))
        for d in range(3):
            x[d] = np.where(bad, c[d], x[d])
            x[d] = np.where(x[d] < lo[:, d], lo[:, d], x[d])
            x[d] = np.where(x[d] > hi[:, d], hi[:, d], x[d]).astype(F)
    return np.stack(x, -1).astype(F), np.stack(c, -1).astype(F)


def sharp_positions(cells, values, axes, sdf, normal, iso=0.0, refine=6, normal_delta=2.0 ** -10, threshold=0.1, nets=None, details=False):
    """The positions [V, 3] float32 of rm_mesh_extract_sharp's vertices.  cells: the plain mesh's RM_MESH_CELLS; values: the corner values
    [nz + 1, ny + 1, nx + 1]; axes: the three arrays of corner coordinates; sdf(points [N, 3]) -> [N] float32 and normal(points [N, 3], delta)
    -> [N, 3] float32: the scene.  nets: the plain mesh's positions, the point of a dead slot (nothing depends on its value; the cell's low corner
    when None).  details: also the mass points and the live mask [12, V]."""
    coords = [np.asarray(a, F) for a in axes]
    n = [len(a) - 1 for a in coords]
    cell = np.asarray(cells, np.int64)
    V = len(cell)
    if V == 0:
        empty = np.zeros((0, 3), F)
        return (empty, empty, np.zeros((12, 0), bool)) if details else empty
    idx = [cell % n[0], (cell // n[0]) % n[1], cell // (n[0] * n[1])]
    pc = [[coords[a][idx[a] + d] for d in (0, 1)] for a in range(3)]
    v3 = np.ascontiguousarray(values, F).reshape(n[2] + 1, n[1] + 1, n[0] + 1)
    iso = F(iso)
    with np.errstate(all="ignore"):
        e = {(dx, dy, dz): (v3[idx[2] + dz, idx[1] + dy, idx[0] + dx] - iso).astype(F) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
        nets = np.stack([pc[a][0] for a in range(3)], -1) if nets is None else np.asarray(nets, F)
        live = np.zeros((12, V), bool)
        x0, e0, x1, e1 = (np.zeros((12, V), F) for _ in range(4))
        points = np.empty((12, V, 3), F)
        for s, (a, ob, oc) in enumerate(SLOTS):
            b, c = (a + 1) % 3, (a + 2) % 3
            k0 = [0, 0, 0]
            k0[b], k0[c] = ob, oc
            k1 = list(k0)
            k1[a] = 1
            k0, k1 = tuple(k0), tuple(k1)
            live[s] = (e[k0] < 0) != (e[k1] < 0)
            x0[s], e0[s], x1[s], e1[s] = pc[a][0], e[k0], pc[a][1], e[k1]
            points[s, :, b], points[s, :, c] = pc[b][ob], pc[c][oc]
            points[s, ~live[s]] = nets[~live[s]]

        def place(along):
            for s, (a, _, _) in enumerate(SLOTS):
                points[s, live[s], a] = along[s, live[s]]

        for _ in range(int(refine)):
            xm = (x0 + (F(0.5) * (x1 - x0)).astype(F)).astype(F)
            place(xm)
            em = (np.asarray(sdf(points.reshape(-1, 3)), F).reshape(12, V) - iso).astype(F)
            low = (em < 0) == (e0 < 0)
            x0, e0, x1, e1 = np.where(low, xm, x0), np.where(low, em, e0), np.where(low, x1, xm), np.where(low, e1, em)
        t = (e0 / (e0 - e1)).astype(F)
        t = np.where((t >= 0) & (t <= 1), t, F(0.5)).astype(F)
        place((x0 + (t * (x1 - x0).astype(F)).astype(F)).astype(F))
        normals = np.asarray(normal(points.reshape(-1, 3), normal_delta), F).reshape(12, V, 3)
    lo = np.stack([pc[a][0] for a in range(3)], -1)
    hi = np.stack([pc[a][1] for a in range(3)], -1)
    positions, mass = qef_vertex(points, normals, live, lo, hi, threshold)
    return (positions, mass, live) if details else positions
