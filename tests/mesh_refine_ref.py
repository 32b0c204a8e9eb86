"""The numpy restatement of include/hip_raymarch.h "refinement".  Written from the header's definition, not from the device's procedure: the edge
table is a sort, the owner a minimum over using slots, the scans cumulative sums; whole-array fp32 operations (numpy contracts nothing).  The scene
comes in as callables, like mesh_project_ref, with which it composes: sdf(points [N, 3] float32) -> [N] for the midpoints, and -- where the rounds
project -- project_sdf and normal for mesh_project_ref.project.  What the GPU is compared with, exactly: integers as integers, floats by their bits."""
import numpy as np

import mesh_measure_ref as QR
import mesh_project_ref as PR

F = np.float32
LIMIT = 0x7FFFFFFF // 3  # the kernels' own limit of triangles
ROUND_FIELDS = ("edges", "split_edges", "nonfinite_midpoints")
FIELDS = ("vertices_before", "triangles_before", "vertices", "triangles") + ROUND_FIELDS + ("flipped_triangles", "max_first", "max_last", "rounds_run", "stopped")


def edges_of(vertices, triangles):
    """Step 1.  (lo [E], hi [E], edge_of [T, 3]): the unique edges of the participating triangles in ascending owner order -- the owner is the
    lowest using slot 3 t + s -- and every using slot's edge, -1 in a triangle that takes no part."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    part = QR.participating(vertices, t)
    a, b = t, np.roll(t, -1, axis=1)  # slot s: corner s -> corner (s + 1) % 3
    lo, hi = np.minimum(a, b).reshape(-1), np.maximum(a, b).reshape(-1)
    using = np.flatnonzero(np.repeat(part, 3))  # ascending using slots
    key = lo[using] << 32 | hi[using]
    keys, first, inverse = np.unique(key, return_index=True, return_inverse=True)  # first: each key's lowest using slot (of `using`)
    order = np.argsort(first, kind="stable")  # the edges by ascending owner
    number = np.empty(len(keys), np.int64)
    number[order] = np.arange(len(keys))
    edge_of = np.full(3 * len(t), -1, np.int64)
    edge_of[using] = number[inverse.reshape(-1)]
    owners = using[first[order]]
    return lo[owners], hi[owners], edge_of.reshape(-1, 3)


def children(corners, mid):
    """Step 5 for one participating triangle: corners (3 ints), mid (3 ints, -1 where the edge is not marked) -> the list of child triples"""
    mask = sum(1 << s for s in range(3) if mid[s] >= 0)
    r = 1 if mask in (2, 6) else 2 if mask in (4, 5) else 0
    v0, v1, v2 = (corners[(i + r) % 3] for i in range(3))
    m0, m1, m2 = (mid[(i + r) % 3] for i in range(3))
    bits = bin(mask).count("1")
    if bits == 0:
        return [(v0, v1, v2)]
    if bits == 1:
        return [(v0, m0, v2), (m0, v1, v2)]
    if bits == 2:
        return [(m0, v1, m1)] + ([(v0, m0, v2), (m0, m1, v2)] if m0 < m1 else [(v0, m0, m1), (v0, m1, v2)])
    return [(v0, m0, m2), (m0, v1, m1), (m2, m1, v2), (m0, m1, m2)]


def split(positions, triangles, sdf, iso=0.0, tolerance=0.0, min_edge=0.0, colours=None, cells=None):
    """Steps 1 - 5 of one round, without the budget.  Returns a dict: edges (E), split, nonfinite, max (F), masks [T] (-1 where the triangle takes no
    part), and the round's mesh: positions, triangles, colours, cells (None where not given)."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    V = len(p)
    lo, hi, edge_of = edges_of(V, t)
    E = len(lo)
    with np.errstate(all="ignore"):
        m = (F(0.5) * (p[lo] + p[hi]).astype(F)).astype(F)
        d = np.asarray(sdf(m), F).reshape(-1) if E else np.zeros(0, F)
        err = (d - F(iso)).astype(F)
        delta = (p[hi] - p[lo]).astype(F)
        len2 = ((delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]).astype(F) + delta[:, 2] * delta[:, 2]).astype(F)
        finite = np.isfinite(err)
        marked = finite & (np.abs(err) > F(tolerance)) & (len2 > F(min_edge) * F(min_edge))
    new_index = np.where(marked, V + np.cumsum(marked) - marked, -1)
    out, masks = [], np.full(len(t), -1, np.int64)
    for i, corners in enumerate(t.astype(np.int64)):
        if edge_of[i, 0] < 0:
            out.append(tuple(corners))
            continue
        mid = [int(new_index[e]) for e in edge_of[i]]
        masks[i] = sum(1 << s for s in range(3) if mid[s] >= 0)
        out += children([int(c) for c in corners], mid)
    result = dict(edges=E, split=int(marked.sum()), nonfinite=int((~finite).sum()), max=F(np.abs(err[finite]).max()) if finite.any() else F(0), masks=masks,
                  positions=np.concatenate([p, m[marked]]), triangles=np.asarray(out, np.uint32).reshape(-1, 3), colours=None, cells=None)
    if colours is not None:
        c = np.ascontiguousarray(colours, F).reshape(-1, 3)
        result["colours"] = np.concatenate([c, (F(0.5) * (c[lo[marked]] + c[hi[marked]]).astype(F)).astype(F)])
    if cells is not None:
        k = np.asarray(cells, np.uint32)
        result["cells"] = np.concatenate([k, k[lo[marked]]])
    return result


def refine(positions, triangles, sdf, iso=0.0, tolerance=0.0, min_edge=0.0, rounds=1, max_triangles=0, colours=None, cells=None, project=None):
    """The header's rounds.  project: None (the midpoints stay), or a dict of mesh_project_ref.project's keywords -- sdf and normal among them --
    through which every applied round's mesh goes.  Returns a dict: positions, triangles, colours, cells, report (FIELDS), and what a test may
    want to look at: masks (per round evaluated) and projections (per round applied, mesh_project_ref's reports)."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    limit = min(int(max_triangles), LIMIT) if max_triangles else LIMIT
    per_round = {k: [0] * 8 for k in ROUND_FIELDS}
    report = dict(vertices_before=len(p), triangles_before=len(t), flipped_triangles=0, max_first=F(0), max_last=F(0), rounds_run=0, stopped=1)
    masks, projections = [], []
    if len(p) and len(t):
        report["stopped"] = 0
        for r in range(int(rounds)):
            s = split(p, t, sdf, iso, tolerance, min_edge, colours, cells)
            per_round["edges"][r], per_round["split_edges"][r], per_round["nonfinite_midpoints"][r] = s["edges"], s["split"], s["nonfinite"]
            report["rounds_run"], report["max_last"] = r + 1, s["max"]
            if r == 0:
                report["max_first"] = s["max"]
            masks.append(s["masks"])
            if s["split"] == 0 or len(s["triangles"]) > limit:
                report["stopped"] = 1 if s["split"] == 0 else 2
                break
            p, t, colours, cells = s["positions"], s["triangles"], s["colours"], s["cells"]
            if project is not None:
                moved = PR.project(p, t, **project)
                p = moved["positions"]
                report["flipped_triangles"] += moved["report"]["flipped_triangles"]
                projections.append(moved["report"])
    report.update(vertices=len(p), triangles=len(t), **{k: tuple(v) for k, v in per_round.items()})
    return dict(positions=p, triangles=t, colours=colours, cells=cells, report={k: report[k] for k in FIELDS}, masks=masks, projections=projections)


def same(got: dict, want: dict) -> list:
    """the names of the report's fields in which two reports differ: integers as integers, floats by their bits"""
    out = []
    for k in FIELDS:
        if k in ("max_first", "max_last"):
            equal = F(got[k]).tobytes() == F(want[k]).tobytes()
        elif k in ROUND_FIELDS:
            equal = tuple(int(x) for x in got[k]) == tuple(int(x) for x in want[k])
        else:
            equal = int(got[k]) == int(want[k])
        if not equal:
            out.append(k)
    return out
