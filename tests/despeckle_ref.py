"""A float32 numpy restatement of the firefly filter (include/hip_raymarch.h RmDespeckle, INTEGRATION.md "Firefly filter"):
the outlier clamp that runs ahead of the denoisers and the present.  Written from the statement, not from the kernel, and
vectorised over the image: the window's taps as shifted planes, the rank statistic by a sort along the tap axis.  Every
product and sum is a float32 operation of its own, in the stated order, so the kernel can be held to it per pixel."""
from __future__ import annotations

import numpy as np

DEFAULTS = dict(radius=2, rank=1, gain=3.0, floor=0.1, repair=1)  # rm_filters_default's despeckle_params
LUM = (0.2126, 0.7152, 0.0722)
F = np.float32


def luminance(color, samples: int) -> np.ndarray:
    """l = (0.2126f * (C.r * s) + 0.7152f * (C.g * s)) + 0.0722f * (C.b * s) with s = 1.0f / samples, in float32."""
    c = np.asarray(color, np.float32)
    s = F(1.0) / F(samples)
    with np.errstate(all="ignore"):
        return (F(LUM[0]) * (c[..., 0] * s) + F(LUM[1]) * (c[..., 1] * s)) + F(LUM[2]) * (c[..., 2] * s)


def _shift(a, dy: int, dx: int, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` outside the image (no wrap)."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def taps(radius: int):
    """The window without its centre in scan order: dy outer, dx inner."""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def despeckle(color, samples: int, radius: int = DEFAULTS["radius"], rank: int = DEFAULTS["rank"], gain: float = DEFAULTS["gain"],
              floor: float = DEFAULTS["floor"], repair: int = DEFAULTS["repair"]) -> np.ndarray:
    """The despeckled colour plane [H, W, 4] (float32, colour-plane units) of the colour plane after `samples` samples."""
    c = np.ascontiguousarray(color, np.float32)
    out = c.copy()
    l = luminance(c, samples)
    valid = np.isfinite(l)
    window = taps(radius)
    # a tap outside the image or an invalid one is skipped: -inf sorts below every valid (finite) value
    lq = np.stack([_shift(np.where(valid, l, F(-np.inf)), dy, dx, F(-np.inf)) for dy, dx in window])
    ok = lq > F(-np.inf)
    n = ok.sum(0)
    enough = n > rank
    t = np.sort(lq, axis=0)[::-1][rank]  # the (rank + 1)-th largest, duplicates counted one by one
    t = np.where(enough, t, F(0.0)).astype(np.float32)
    with np.errstate(all="ignore"):
        T = F(gain) * t + F(floor)
        clamp = enough & valid & (l > T)
        f = (t / l).astype(np.float32)
        out[..., :3] = np.where(clamp[..., None], c[..., :3] * f[..., None], out[..., :3])
        if repair:
            acc = np.zeros(c.shape[:2] + (3,), np.float32)
            count = np.zeros(c.shape[:2], np.int32)
            for (dy, dx), lt, okt in zip(window, lq, ok):  # scan order, sequentially per channel
                use = okt & (lt <= t)
                acc = acc + np.where(use[..., None], _shift(c[..., :3], dy, dx, F(0.0)), F(0.0))
                count += use
            mean = acc / np.maximum(count, 1).astype(np.float32)[..., None]
            fix = enough & ~valid & np.isfinite(mean).all(-1)
            out[..., :3] = np.where(fix[..., None], mean, out[..., :3])
    return out


def changed(out, color) -> np.ndarray:
    """Pixels whose bits differ from the colour plane's, [H, W] bool."""
    a, b = np.ascontiguousarray(out, np.float32), np.ascontiguousarray(color, np.float32)
    return (a.view(np.uint32) != b.view(np.uint32)).any(-1)
