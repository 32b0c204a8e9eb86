"""The numpy restatement of include/hip_raymarch.h "deviation".  Written from the header's definition, not from the device's procedure:
whole-array fp32 and float64 operations (numpy contracts nothing), the per-triangle sums the stated butterfly, the report's sums
mesh_measure_ref.tree_sum, its maximum an argmax.  The scene comes in as a callable, like mesh_occlusion_ref: sdf(points [N, 3] float32) -> [N],
which a GPU test feeds with Context.probe and a CPU test with analytic fields.  What the GPU is compared with, exactly: integers as integers,
floats and doubles by their bits."""
import math

import numpy as np

import mesh_measure_ref as QR

F = np.float32
INTEGER_FIELDS = ("vertices", "triangles", "skipped_triangles", "unevaluated_triangles", "nonfinite_samples", "over_triangles", "worst_triangle")
DOUBLE_FIELDS = ("area", "over_area", "mean_signed", "rms")
FIELDS = INTEGER_FIELDS + DOUBLE_FIELDS + ("max", "samples")  # the struct's fields, in its order, without `reserved`
ORDERS = (1, 2, 4, 8)


def weights(order) -> np.ndarray:
    """step 1: [S, 4] float32 (w0, w1, w2, 0), the centroids of the n * n congruent sub-triangles; integers divided in double, rounded once"""
    n = int(order)
    out = np.zeros((n * n, 4), F)
    for s in range(n * n):
        r = math.isqrt(s)
        c = s - r * r
        if c % 2 == 0:
            m = c // 2
            a, b = 3 * (r - m) + 1, 3 * m + 1
        else:
            m = (c - 1) // 2
            a, b = 3 * (r - m) - 1, 3 * m + 2
        out[s, 0] = F(np.float64(3 * n - a - b) / np.float64(3 * n))
        out[s, 1] = F(np.float64(a) / np.float64(3 * n))
        out[s, 2] = F(np.float64(b) / np.float64(3 * n))
    return out


def points(corners, order) -> np.ndarray:
    """step 2: corners [N, 3 (corner), 3 (component)] float32 -> [N, S, 3], each product and each sum rounded to fp32"""
    p = np.ascontiguousarray(corners, F).reshape(-1, 3, 3)
    w = weights(order)
    with np.errstate(all="ignore"):
        a = (w[None, :, 0, None] * p[:, None, 0, :]).astype(F)
        b = (w[None, :, 1, None] * p[:, None, 1, :]).astype(F)
        c = (w[None, :, 2, None] * p[:, None, 2, :]).astype(F)
        return ((a + b).astype(F) + c).astype(F)


def butterfly(x) -> np.ndarray:
    """[N, S] float64 -> [N]: for m = 1, 2, 4, .. < S: x[i] = x[i] + x[i xor m]"""
    x = np.array(x, np.float64)
    S = x.shape[1]
    index = np.arange(S)
    m = 1
    while m < S:
        x = x + x[:, index ^ m]
        m *= 2
    return x[:, 0]


def areas(corners) -> np.ndarray:
    """step 4's area_t in double, without the measures' shift of the origin"""
    p = np.ascontiguousarray(corners, F).reshape(-1, 3, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        return 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


def deviation(positions, triangles, sdf, iso=0.0, order=4, tolerance=0.0):
    """The header's steps 1 - 5.  Returns a dict: triangles [T] float32 (max_t), report (FIELDS), and what a test may want to look at: mean [T] and
    ms [T] float64 (mean_t, ms_t; 0 where the triangle is not evaluated), area [T] float64, and the masks skipped, evaluated and over [T]."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    V, T, S = len(p), len(t), int(order) * int(order)
    iso, tolerance = F(iso), F(tolerance)
    report = dict.fromkeys(FIELDS, 0)
    report.update(vertices=V, triangles=T, samples=S, area=np.float64(0), over_area=np.float64(0), mean_signed=np.float64(0), rms=np.float64(0), max=F(0))
    skipped = ~(t < V).all(axis=1)
    max_t, mean_t, ms_t, area_t = np.zeros(T, F), np.zeros(T, np.float64), np.zeros(T, np.float64), np.zeros(T, np.float64)
    evaluated, over = np.zeros(T, bool), np.zeros(T, bool)
    if V == 0 or T == 0:
        report["skipped_triangles"] = T if V == 0 else 0
        return dict(triangles=max_t, report=report, mean=mean_t, ms=ms_t, area=area_t, skipped=skipped, evaluated=evaluated, over=over)
    live = np.flatnonzero(~skipped)
    corners = p[t[live]]  # [L, 3, 3]
    q = points(corners, order)
    with np.errstate(all="ignore"):
        d = np.asarray(sdf(q.reshape(-1, 3)), F).reshape(len(live), S)
        e = (d - iso).astype(F)
        finite = np.isfinite(e)
        e64 = e.astype(np.float64)
        largest = np.where(finite, np.abs(e), F(0)).max(axis=1).astype(F)
        s1 = butterfly(np.where(finite, e64, 0.0))
        s2 = butterfly(np.where(finite, e64 * e64, 0.0))
        whole = finite.all(axis=1)
        a = areas(corners)
        max_t[live] = largest
        evaluated[live] = whole
        mean_t[live] = np.where(whole, s1 / np.float64(S), 0.0)
        ms_t[live] = np.where(whole, s2 / np.float64(S), 0.0)
        area_t[live] = np.where(whole, a, 0.0)
        over = evaluated & (max_t > tolerance)
        area = QR.tree_sum(area_t)
        over_area = QR.tree_sum(np.where(over, area_t, 0.0))
        a1 = QR.tree_sum(np.where(evaluated, area_t * mean_t, 0.0))
        a2 = QR.tree_sum(np.where(evaluated, area_t * ms_t, 0.0))
        report.update(skipped_triangles=int(skipped.sum()), unevaluated_triangles=int((~whole).sum()), nonfinite_samples=int((~finite).sum()),
                      over_triangles=int(over.sum()), area=np.float64(area), over_area=np.float64(over_area))
        if area != 0:
            report.update(mean_signed=np.float64(a1 / area), rms=np.float64(np.sqrt(a2 / area)))
    if evaluated.any():
        worst = int(np.argmax(np.where(evaluated, max_t, F(-1))))  # the first of the largest
        report.update(worst_triangle=worst, max=F(max_t[worst]))
    return dict(triangles=max_t, report=report, mean=mean_t, ms=ms_t, area=area_t, skipped=skipped, evaluated=evaluated, over=over)


def same(got: dict, want: dict) -> list:
    """the names of the report's fields in which two reports differ: integers as integers, floats and doubles by their bits"""
    out = []
    for k in FIELDS:
        if k in DOUBLE_FIELDS:
            equal = np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes()
        elif k == "max":
            equal = F(got[k]).tobytes() == F(want[k]).tobytes()
        else:
            equal = int(got[k]) == int(want[k])
        if not equal:
            out.append(k)
    return out
