"""The numpy restatement of include/hip_raymarch.h "measures and edge topology".  Written from the header's definitions, not from the device's
procedure: the edges are np.unique of the keys x << 32 | y with a bincount per direction, the extent numpy's minima and maxima, the terms float64
array operations of their own (numpy contracts nothing, its division and square root are IEEE), and the fixed tree a reshape to groups of 256 and
seven slice additions per level.  What the GPU is compared with, exactly: integers as integers, floats and doubles by their bits."""
import numpy as np

F = np.float32
ROW_NAMES = ("edges", "boundary", "irregular", "unbalanced")


def tree_sum(terms) -> np.float64:
    """The fixed-tree sum of a float64 list: groups of 256 (+0.0 behind the last), each by off = 128 .. 1: s[i] = s[i] + s[i + off]."""
    s = np.asarray(terms, np.float64).reshape(-1)
    if len(s) == 0:
        return np.float64(0.0)
    while True:
        groups = (len(s) + 255) // 256
        padded = np.zeros(groups * 256, np.float64)
        padded[:len(s)] = s
        g = padded.reshape(groups, 256)
        off = 128
        while off >= 1:
            g = g[:, :off] + g[:, off:2 * off]
            off //= 2
        s = g.reshape(-1)
        if groups == 1:
            return np.float64(s[0])


def participating(vertices, triangles):
    """mask [T]: the three indices are < V and pairwise distinct"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return (t < vertices).all(axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])


def edge_table(vertices, triangles):
    """(x, y, f, r) of the undirected edges of the participating triangles, ascending (x, y): f uses as x -> y, r uses as y -> x"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    t = t[participating(vertices, t)]
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]) if len(t) else np.zeros((0, 2), np.int64)
    forward = d[:, 0] < d[:, 1]
    key = (np.minimum(d[:, 0], d[:, 1]).astype(np.uint64) << np.uint64(32)) | np.maximum(d[:, 0], d[:, 1]).astype(np.uint64)
    keys, inverse = np.unique(key, return_inverse=True)
    inverse = inverse.reshape(-1)
    f = np.bincount(inverse[forward], minlength=len(keys)).astype(np.int64)
    r = np.bincount(inverse[~forward], minlength=len(keys)).astype(np.int64)
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), f, r


def measure(positions, triangles, labels=None, components=None):
    """The measures of a mesh as a dict of RmMeshMeasures' fields (lo, hi float32 [3]; area, volume np.float64; closed bool) plus
    component_edges [C, 4] uint64.  labels [V] and components = C are rm_mesh_components' (None: one component holds everything, or none
    when there is no vertex)."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(p), len(t)
    if labels is None:
        labels, components = np.zeros(V, np.int64), (1 if V else 0)
    labels = np.asarray(labels, np.int64)
    part = participating(V, t)
    tp = t[part]
    P = int(part.sum())
    x, y, f, r = edge_table(V, t)
    uses = f + r
    boundary, regular = uses == 1, (f == 1) & (r == 1)
    irregular = ~boundary & ~regular
    unbalanced = (uses >= 2) & (f != r)
    used = int(len(np.unique(tp)))
    rows = np.zeros((int(components), 4), np.uint64)
    of = labels[x]
    for k, mask in enumerate((np.ones(len(x), bool), boundary, irregular, unbalanced)):
        rows[:, k] = np.bincount(of[mask], minlength=int(components)).astype(np.uint64)
    finite_v = np.isfinite(p).all(axis=1)
    lo = hi = np.zeros(3, F)
    if finite_v.any():
        lo = (p[finite_v].min(axis=0) + F(0.0)).astype(F)
        hi = (p[finite_v].max(axis=0) + F(0.0)).astype(F)
    area_t, vol_t = np.zeros(T, np.float64), np.zeros(T, np.float64)
    measured = part.copy()
    if P:
        measured[part] = np.isfinite(p[tp]).all(axis=(1, 2))
    if measured.any():
        o = lo.astype(np.float64)
        q = p[t[measured]].astype(np.float64)
        a, b, c = q[:, 0] - o, q[:, 1] - o, q[:, 2] - o
        e1, e2 = b - a, c - a

        def cross(u, v):
            return (u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])

        with np.errstate(all="ignore"):
            nx, ny, nz = cross(e1, e2)
            area_t[measured] = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
            mx, my, mz = cross(b, c)
            vol_t[measured] = ((a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz) / 6.0
    with np.errstate(all="ignore"):
        area, volume = tree_sum(area_t), tree_sum(vol_t)
    E = len(x)
    return dict(vertices=V, triangles=T, used_vertices=used, skipped_triangles=T - P, unmeasured_triangles=P - int(measured.sum()),
                finite_vertices=int(finite_v.sum()), edges=E, boundary_edges=int(boundary.sum()), regular_edges=int(regular.sum()),
                irregular_edges=int(irregular.sum()), unbalanced_edges=int(unbalanced.sum()), euler=used - E + P, components=int(components),
                closed_components=int(((rows[:, 0] > 0) & (rows[:, 1] == 0) & (rows[:, 2] == 0)).sum()), area=area, volume=volume, lo=lo, hi=hi,
                closed=bool(P >= 1 and not boundary.any() and not irregular.any()), component_edges=rows)


INTEGER_FIELDS = ("vertices", "triangles", "used_vertices", "skipped_triangles", "unmeasured_triangles", "finite_vertices", "edges", "boundary_edges",
                  "regular_edges", "irregular_edges", "unbalanced_edges", "euler", "components", "closed_components")


def same(got: dict, want: dict) -> list:
    """The names of the fields in which two measures differ: integers as integers, area and volume by their 64 bits, lo and hi by their 32."""
    bad = [k for k in INTEGER_FIELDS if int(got[k]) != int(want[k])]
    bad += [k for k in ("area", "volume") if np.float64(got[k]).tobytes() != np.float64(want[k]).tobytes()]
    bad += [k for k in ("lo", "hi") if np.asarray(got[k], F).tobytes() != np.asarray(want[k], F).tobytes()]
    if bool(got["closed"]) != bool(want["closed"]):
        bad.append("closed")
    if not np.array_equal(np.asarray(got["component_edges"], np.uint64).reshape(-1, 4), np.asarray(want["component_edges"], np.uint64).reshape(-1, 4)):
        bad.append("component_edges")
    return bad


def stl_bytes(positions, triangles) -> bytes:
    """Binary STL as the hosts write it, one triangle at a time in Python floats (doubles): 80 header bytes, uint32 T, then per triangle the
    facet normal, the corners and a uint16 0."""
    import math
    import struct

    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    out = [b"hip_raymarch mesh".ljust(80, b"\0"), struct.pack("<I", len(t))]
    for tri in t:
        p0, p1, p2 = ([float(v) for v in p[i]] for i in tri)
        e1, e2 = [p1[k] - p0[k] for k in range(3)], [p2[k] - p0[k] for k in range(3)]
        c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        try:
            length = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        except (ValueError, OverflowError):
            length = float("nan")
        good = length > 0 and math.isfinite(length)
        normal = np.array([v / length for v in c] if good else [0.0, 0.0, 0.0], np.float64).astype("<f4")
        out.append(normal.tobytes() + np.array(p0 + p1 + p2, "<f4").tobytes() + b"\0\0")
    return b"".join(out)


def parse_stl(data: bytes):
    """(normals [T, 3], corners [T, 3, 3]) float32 of a binary STL; checks the header, the count, the length and the attribute words."""
    assert data[:80] == b"hip_raymarch mesh".ljust(80, b"\0")
    count = int(np.frombuffer(data, "<u4", 1, 80)[0])
    assert len(data) == 84 + 50 * count
    rec = np.frombuffer(data, np.dtype([("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attribute", "<u2")]), count, 84)
    assert not rec["attribute"].any()
    return rec["normal"], rec["corners"]
