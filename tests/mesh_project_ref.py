"""The numpy restatement of include/hip_raymarch.h "projection onto the surface".  Written from the header's definition, not from the device's
procedure: whole-array fp32 operations (numpy contracts nothing), the report's maximum an argmax, its sums mesh_measure_ref.tree_sum.  The scene
comes in as two callables, like mesh_occlusion_ref: sdf(points [N, 3] float32) -> [N] and normal(points) -> [N, 3], which a GPU test feeds with
Context.probe and a CPU test with analytic fields.  What the GPU is compared with, exactly: integers as integers, floats and doubles by their bits."""
import numpy as np

import mesh_measure_ref as QR

F = np.float32
INTEGER_FIELDS = ("vertices", "triangles", "moved_vertices", "settled_before", "settled_after", "nonfinite_before", "nonfinite_after", "clamped_vertices",
                  "undirected_vertices", "flipped_triangles", "worst_before", "worst_after")
DOUBLE_FIELDS = ("mean_before", "rms_before", "mean_after", "rms_after")
FLOAT_FIELDS = ("max_before", "max_after")
FIELDS = INTEGER_FIELDS + DOUBLE_FIELDS + FLOAT_FIELDS + ("rounds_run",)  # the struct's fields, in its order, without `reserved`


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def crosses(positions, triangles):
    """the cross products of "quadric placement" step 2: each product rounded, then the difference"""
    p = np.ascontiguousarray(positions, F)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
        return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)


def flipped(source, final, triangles):
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    t = t[(t < len(source)).all(axis=1)]
    c0, c1 = crosses(source, t), crosses(final, t)
    with np.errstate(all="ignore"):
        dot = (c0[:, 0] * c1[:, 0] + c0[:, 1] * c1[:, 1]) + c0[:, 2] * c1[:, 2]
    return int((dot < 0).sum())


def half(e, tolerance):
    """(settled, nonfinite, worst, max, mean, rms) of one list of residuals"""
    e = np.asarray(e, F)
    finite = np.isfinite(e)
    a = np.abs(e)
    count = int(finite.sum())
    settled, nonfinite = int((finite & (a <= F(tolerance))).sum()), int(len(e) - count)
    if count == 0:
        return settled, nonfinite, 0, F(0), np.float64(0), np.float64(0)
    worst = int(np.argmax(np.where(finite, a, F(-1))))  # the first of the largest
    e64 = e.astype(np.float64)
    total = QR.tree_sum(np.where(finite, a.astype(np.float64), 0.0))
    total2 = QR.tree_sum(np.where(finite, e64 * e64, 0.0))
    return settled, nonfinite, worst, a[worst], np.float64(total / np.float64(count)), np.float64(np.sqrt(total2 / np.float64(count)))


def project(positions, triangles, sdf, normal, iso=0.0, rounds=4, relax=1.0, tolerance=0.0, reach=0.0):
    """The header's steps 1 - 7.  Returns a dict: positions [V, 3], residual [V] (e_after), report (FIELDS), and what a test may want to look at:
    moved (per round), skipped_waves (per round: the fraction of the waves of 64 vertices none of which wanted a normal), clamped and undirected
    (bool [V])."""
    p0 = np.ascontiguousarray(positions, F).reshape(-1, 3)
    V = len(p0)
    iso, relax, tolerance, reach = F(iso), F(relax), F(tolerance), F(reach)
    p = p0.copy()
    clamped, undirected = np.zeros(V, bool), np.zeros(V, bool)
    moved, skipped, e, e_before, last_moved = [], [], np.zeros(0, F), np.zeros(0, F), 0
    with np.errstate(all="ignore"):
        for r in range(int(rounds) if V else 0):
            e = (np.asarray(sdf(p), F).reshape(-1) - iso).astype(F)
            if r == 0:
                e_before = e
            want = np.isfinite(e) & (np.abs(e) > tolerance)
            waves = np.zeros(-(-V // 64) * 64, bool)
            waves[:V] = want
            skipped.append(float(1.0 - waves.reshape(-1, 64).any(axis=1).mean()))
            n = np.zeros((V, 3), F)
            if want.any():
                n[want] = np.asarray(normal(p[want]), F).reshape(-1, 3)
            bad = ~np.isfinite(n).all(axis=1) | (n == 0).all(axis=1)
            undirected |= want & bad
            go = want & ~bad
            s = (e * relax).astype(F)
            q = (p - (n * s[:, None]).astype(F)).astype(F)
            if reach > 0:
                lo, hi = (p0 - reach).astype(F), (p0 + reach).astype(F)
                below = q < lo
                q = np.where(below, lo, q)
                above = q > hi
                q = np.where(above, hi, q)
                clamped |= go & (below | above).any(axis=1)
            ok = go & np.isfinite(q).all(axis=1)
            nxt = np.where(ok[:, None], q, p).astype(F)
            last_moved = int((bits(nxt) != bits(p)).any(axis=1).sum())
            moved.append(last_moved)
            p = nxt
            if last_moved == 0:
                break
        e_after = e if last_moved == 0 else (np.asarray(sdf(p), F).reshape(-1) - iso).astype(F)
    before, after = half(e_before, tolerance), half(e_after, tolerance)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    report = dict(vertices=V, triangles=len(t), moved_vertices=int((bits(p) != bits(p0)).any(axis=1).sum()), settled_before=before[0], settled_after=after[0],
                  nonfinite_before=before[1], nonfinite_after=after[1], clamped_vertices=int(clamped.sum()), undirected_vertices=int(undirected.sum()),
                  flipped_triangles=flipped(p0, p, t) if V else 0, worst_before=before[2], worst_after=after[2], mean_before=before[4], rms_before=before[5],
                  mean_after=after[4], rms_after=after[5], max_before=F(before[3]), max_after=F(after[3]), rounds_run=len(moved))
    return dict(positions=p, residual=np.asarray(e_after, F), report={k: report[k] for k in FIELDS}, moved=moved, skipped_waves=skipped, clamped=clamped,
                undirected=undirected)


def same(got: dict, want: dict) -> list:
    """the names of the report's fields in which two reports differ: integers as integers, floats and doubles by their bits"""
    out = []
    for k in FIELDS:
        if k in DOUBLE_FIELDS:
            equal = np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes()
        elif k in FLOAT_FIELDS:
            equal = F(got[k]).tobytes() == F(want[k]).tobytes()
        else:
            equal = int(got[k]) == int(want[k])
        if not equal:
            out.append(k)
    return out


def forward_normal(sdf, delta=2.0 ** -10):
    """RM_PROBE_NORMAL's shape on a callable field, for the CPU tests: forward differences at `delta`, normalised as v * (1 / length(v)), in fp32"""
    d = F(delta)

    def normal(points):
        p = np.ascontiguousarray(points, F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            at = np.asarray(sdf(p), F)
            g = np.stack([np.asarray(sdf(p + np.array(o, F) * d), F) - at for o in ((1, 0, 0), (0, 1, 0), (0, 0, 1))], -1).astype(F)
            length = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)).astype(F)
            return (g * (F(1) / length)[:, None]).astype(F)
    return normal
