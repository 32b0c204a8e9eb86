"""A float64 numpy restatement of the distance functions the fast build evaluates with arithmetic of its own, and the unit
its per-point error is measured in.  Written from the scene text (scene.py Mandelbulb.sdf_glsl, CsgScene.sdf_glsl and the
helpers that text calls), not from a kernel or the oracle; imports nothing from the product.

The estimators are ill-conditioned where the Mandelbulb's orbit is chaotic and where a table's value cancels, so a fixed
tolerance per point is either broken by honest rounding or hides a defect.  `unit` is what moving the fp32 point by one
ulp along an axis does to the float64 value, plus the rounding of the value and of the coordinates: the error of ANY fp32
evaluation is a modest multiple of it, a skipped row or a stale derivative thousands."""
from __future__ import annotations

import numpy as np

# include/hip_raymarch.h: the row types and operators table() knows (no domain rows, no kind rows)
SPHERE, BOX, TORUS, CYLINDER, PLANE = 0, 1, 5, 6, 7
UNION, SMOOTH_UNION, SUBTRACT, INTERSECT, SMOOTH_SUBTRACT, SMOOTH_INTERSECT = 0, 1, 2, 3, 4, 5


def _length(*c):
    return np.sqrt(sum(x * x for x in c))


def _mix(x, y, a):
    return x * (1.0 - a) + y * a


def bulb(points, power: float, iterations: int, bailout: float):
    """Mandelbulb.sdf_glsl at float64.  Returns (distance, rounds, margin): the rounds a point's orbit ran (the passes of the
    loop that did not break), and the smallest |r / bailout - 1| over the bailout tests it took (inf if it took none) -- how
    far the point is from running a different number of rounds."""
    pos = np.asarray(points, np.float64).reshape(-1, 3)
    power, bailout = float(np.float32(power)), float(np.float32(bailout))  # the literals of the text are the fp32 parameters
    n = len(pos)
    z = pos.copy()
    dr, r = np.ones(n), np.zeros(n)
    rounds, margin = np.zeros(n, np.int64), np.full(n, np.inf)
    live = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            zl = z[idx]
            rl = _length(zl[:, 0], zl[:, 1], zl[:, 2])
            r[idx] = rl
            margin[idx] = np.fmin(margin[idx], np.abs(rl / bailout - 1.0))
            out = rl > bailout
            live[idx[out]] = False
            idx, zl, rl = idx[~out], zl[~out], rl[~out]
            theta = np.arccos(zl[:, 2] / rl)
            phi = np.arctan2(zl[:, 1], zl[:, 0])
            dr[idx] = np.power(rl, power - 1.0) * power * dr[idx] + 1.0
            zr = np.power(rl, power)
            theta, phi = theta * power, phi * power
            z[idx] = zr[:, None] * np.stack([np.sin(theta) * np.cos(phi), np.sin(phi) * np.sin(theta), np.cos(theta)], 1) + pos[idx]
            rounds[idx] += 1
        d = 0.5 * np.log(r) * r / dr
    return d, rounds, margin


def _shape(prim: int, q, size):
    """One row's distance term at q = p - centre."""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    if prim == SPHERE:  # sdfSphere: distance(position, center) - radius
        return _length(x, y, z) - size[0]
    if prim == BOX:  # sdBox
        a, b, c = np.abs(x) - size[0], np.abs(y) - size[1], np.abs(z) - size[2]
        return _length(np.maximum(a, 0.0), np.maximum(b, 0.0), np.maximum(c, 0.0)) + np.minimum(np.maximum(a, np.maximum(b, c)), 0.0)
    if prim == TORUS:  # rmTorus
        return _length(_length(x, z) - size[0], y) - size[1]
    if prim == CYLINDER:  # rmCylinder
        dx, dy = _length(x, z) - size[0], np.abs(y) - size[1]
        return np.minimum(np.maximum(dx, dy), 0.0) + _length(np.maximum(dx, 0.0), np.maximum(dy, 0.0))
    if prim == PLANE:  # rmPlane
        return x * size[0] + y * size[1] + z * size[2]
    raise ValueError(f"table(): row type {prim} (domain and kind rows are not restated)")


def table(scene, points):
    """CsgScene.sdf_glsl at float64: the left fold of the scene's rows, constants as the fp32 values the table stores."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    d = None
    with np.errstate(all="ignore"):
        for row in scene.prims():
            prim, op, k = row.type & 0xFF, (row.type >> 8) & 0xFF, float(row.k)
            di = _shape(prim, p - np.array([float(v) for v in row.center]), [float(v) for v in row.size])
            if d is None:
                d = di
            elif op == UNION:
                d = np.minimum(d, di)
            elif op == SMOOTH_UNION:
                h = np.clip(0.5 + 0.5 * (di - d) / k, 0.0, 1.0)
                d = _mix(di, d, h) - k * h * (1.0 - h)
            elif op == SUBTRACT:
                d = np.maximum(d, -di)
            elif op == SMOOTH_SUBTRACT:
                h = np.clip(0.5 - 0.5 * (d + di) / k, 0.0, 1.0)
                d = _mix(d, -di, h) + k * h * (1.0 - h)
            elif op == SMOOTH_INTERSECT:
                h = np.clip(0.5 - 0.5 * (d - di) / k, 0.0, 1.0)
                d = _mix(d, di, h) + k * h * (1.0 - h)
            elif op == INTERSECT:
                d = np.maximum(d, di)
            else:
                raise ValueError(f"table(): operator {op}")
    if d is None:
        raise ValueError("table(): no rows")
    return d


def neighbours(points):
    """[6, n, 3] float64: p +- ulp32(p_axis) e_axis, the fp32 points next to each point along the axes."""
    p32 = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    ulp = np.abs(np.spacing(p32)).astype(np.float64)
    out = np.repeat(p[None], 6, 0)
    for axis in range(3):
        out[2 * axis, :, axis] += ulp[:, axis]
        out[2 * axis + 1, :, axis] -= ulp[:, axis]
    return out


def unit_of(fp, fq, points):
    """u(p) from the values at the points (fp [n]) and at their neighbours (fq [6, n])."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        sens = np.abs(fq - fp[None]).max(0)
        return sens + 2.0 ** -23 * (np.abs(fp) + np.abs(p).max(1)) + 1e-15


def unit(f, points):
    """u(p) = sens(p) + 2^-23 (|f(p)| + max |p_axis|) + 1e-15 with sens(p) = max over the six neighbours q of |f(q) - f(p)|,
    for fp32 `points` and a float64 function `f` of [m, 3] points.  (The floor: the fast Mandelbulb's step is 0 where the true
    one is below 1e-18, and the fast build flushes fp32 denormals.)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return unit_of(f(p), np.stack([f(q) for q in neighbours(points)]), p)


def ratio(g, f, u):
    """|g - f| / u per point; where the float64 value f is not finite: 0 if g is of the same class (NaN with NaN, an infinity
    with the same infinity), else inf."""
    g, f = np.asarray(g, np.float64), np.asarray(f, np.float64)
    with np.errstate(all="ignore"):
        out = np.abs(g - f) / u
    odd = ~np.isfinite(f)
    out[odd] = np.where((np.isnan(f) & np.isnan(g)) | (f == g), 0.0, np.inf)[odd]
    out[np.isfinite(f) & ~np.isfinite(g)] = np.inf
    return out
