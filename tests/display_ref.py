"""The frame statistics, the exposure arithmetic and the display transform, restated in numpy from include/hip_raymarch.h
("frame statistics and exposure", "the display transform"): the classification and the bins in fp32 and integer arithmetic on the
bits, the two host functions in float64, steps 1-5 of the transform in fp32 with `pow` taken from the oracle (oracle.math for the
product's arithmetic, oracle.ss_math for the GL stack's) and both unorm8 forms of csrc/rm_device.hpp."""
import numpy as np

BINS = 512
BIAS = 1712  # bits(2^-20) >> 19
TONES = {"clip": 0, "reinhard": 1, "aces": 2}
AUTO_DEFAULTS = dict(key=0.18, low=0.10, high=0.95, min_gain=2.0 ** -10, max_gain=2.0 ** 10)
F = np.float32


def luminance(color, samples):
    """l per pixel in the firefly filter's order: fp32, every product and sum rounded on its own."""
    c = np.asarray(color, F)
    s = F(1.0) / F(samples)
    with np.errstate(all="ignore"):
        return (F(0.2126) * (c[..., 0] * s) + F(0.7152) * (c[..., 1] * s)) + F(0.0722) * (c[..., 2] * s)


def edge(b):
    """lo_b for b = 0..512 (hi_b = lo_(b+1), lo_512 = 2^12): the float with the bits (b + 1712) << 19."""
    return ((np.asarray(b, np.int64) + BIAS) << 19).astype(np.uint32).view(F)


def _key(l):
    """Order-preserving unsigned key of a float's bits: -0 below +0."""
    b = np.ascontiguousarray(l, F).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def classify(l):
    """Per value: -1 non_finite, -2 below, -3 above, else its bin."""
    l = np.ascontiguousarray(l, F)
    with np.errstate(invalid="ignore"):
        cls = (l.view(np.uint32) >> 19).astype(np.int64) - BIAS
        cls[l >= F(4096.0)] = -3
        cls[l < F(2.0 ** -20)] = -2
        cls[~np.isfinite(l)] = -1
    return cls


def stats_of_luminance(l):
    l = np.ascontiguousarray(l, F).ravel()
    cls = classify(l)
    hist = np.bincount(cls[cls >= 0], minlength=BINS).astype(np.uint64)
    assert hist.size == BINS
    fin = l[cls != -1]
    if fin.size:
        k = _key(fin)
        lo, hi = fin[np.argmin(k)], fin[np.argmax(k)]
    else:
        lo, hi = F(np.inf), F(-np.inf)
    return dict(pixels=int(l.size), below=int((cls == -2).sum()), above=int((cls == -3).sum()), non_finite=int((cls == -1).sum()),
                min_l=F(lo), max_l=F(hi), hist=hist)


def stats(color, samples):
    """rm_frame_stats of a colour plane [rows, W, 4] after `samples` samples."""
    return stats_of_luminance(luminance(color, samples))


def add(a, b):
    ka, kb = _key(np.array([a["min_l"], b["min_l"]], F)), _key(np.array([a["max_l"], b["max_l"]], F))
    return dict(pixels=a["pixels"] + b["pixels"], below=a["below"] + b["below"], above=a["above"] + b["above"],
                non_finite=a["non_finite"] + b["non_finite"], min_l=(a["min_l"], b["min_l"])[int(np.argmin(ka))],
                max_l=(a["max_l"], b["max_l"])[int(np.argmax(kb))], hist=a["hist"] + b["hist"])


def percentile(hist, q):
    """rm_stats_percentile in float64; ValueError where it refuses."""
    if not (np.isfinite(q) and 0.0 <= q <= 1.0):
        raise ValueError("q")
    hist = np.asarray(hist, np.uint64)
    N = int(hist.sum())
    if N == 0:
        return F(0.0)
    r = max(1.0, float(np.ceil(np.float64(q) * np.float64(N))))
    C = np.cumsum(hist).astype(np.float64)
    b = int(np.argmax(C >= r))
    return edge(b + 1)


def exposure(hist, **fields):
    """rm_stats_exposure in float64 (the fields are the struct's: rounded to fp32 first); ValueError where it refuses."""
    reserved = fields.pop("reserved", 0)
    p = {k: np.float64(F(v)) for k, v in {**AUTO_DEFAULTS, **fields}.items()}
    if not all(np.isfinite(v) for v in p.values()):
        raise ValueError("non-finite field")
    if not (0.0 <= p["low"] < p["high"] <= 1.0) or not p["key"] > 0.0 or not (0.0 < p["min_gain"] <= p["max_gain"]) or reserved != 0:
        raise ValueError("out of range")
    hist = np.asarray(hist, np.uint64)
    N = int(hist.sum())
    if N == 0:
        return F(1.0)
    a, b = p["low"] * np.float64(N), p["high"] * np.float64(N)
    C = np.cumsum(hist).astype(np.float64)
    before = np.concatenate([[0.0], C[:-1]])
    w = np.maximum(0.0, np.minimum(C, b) - np.maximum(before, a))
    lam = (np.log2(edge(np.arange(BINS)).astype(np.float64)) + np.log2(edge(np.arange(1, BINS + 1)).astype(np.float64))) / 2.0
    m = float((w * lam).sum() / (b - a))
    return F(min(max(p["key"] / 2.0 ** m, p["min_gain"]), p["max_gain"]))


def log_average(hist, low=0.0, high=1.0):
    """m of rm_stats_exposure: the log2-average over the bins' geometric centres between two percentiles."""
    hist = np.asarray(hist, np.uint64)
    N = np.float64(int(hist.sum()))
    a, b = np.float64(low) * N, np.float64(high) * N
    C = np.cumsum(hist).astype(np.float64)
    w = np.maximum(0.0, np.minimum(C, b) - np.maximum(np.concatenate([[0.0], C[:-1]]), a))
    lam = (np.log2(edge(np.arange(BINS)).astype(np.float64)) + np.log2(edge(np.arange(1, BINS + 1)).astype(np.float64))) / 2.0
    return float((w * lam).sum() / (b - a))


# ---- the display transform ---------------------------------------------------------------------------------------------------

def expose(v, gain):
    """Step 1: e = v * gain in fp32."""
    with np.errstate(all="ignore"):
        return np.asarray(v, F) * F(gain)


def tone(e, tone="clip", white=4.0):
    """Steps 2-4 per channel, every operation fp32 and rounded on its own (numpy's float32 division is IEEE's)."""
    e = np.asarray(e, F)
    op = TONES[tone] if isinstance(tone, str) else int(tone)
    if op == 0:
        return e.copy()
    with np.errstate(all="ignore"):
        through = ~(e > F(0.0))
        E = np.minimum(np.where(through, F(1.0), e), F(1048576.0)).astype(F)
        if op == 1:
            w2 = F(white) * F(white)
            q = E / w2
            a = F(1.0) + q
            n = E * a
            d = F(1.0) + E
            t = n / d
        else:
            a = F(2.51) * E
            a = a + F(0.03)
            n = E * a
            b = F(2.43) * E
            b = b + F(0.59)
            b = E * b
            d = b + F(0.14)
            t = n / d
    assert t.dtype == F
    return np.where(through, e, t)


def unorm8(g, gl_stack=False):
    """csrc/rm_device.hpp unorm8: NaN and negatives to 0, above 1 to 1; the product rounds g * 255 + 0.5 down, the GL stack goes
    through 16 bits."""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore"):
        g = np.where(g != g, F(0.0), np.where(g < F(0.0), F(0.0), np.where(g > F(1.0), F(1.0), g))).astype(F)
    if gl_stack:
        c16 = (g * F(65535.0)).astype(np.int32)
        return ((c16 - (c16 >> 8) + 128) >> 8).astype(np.uint8)
    return np.floor(g * F(255.0) + F(0.5)).astype(np.uint8)


def gamma(t, gl_stack=False):
    """Step 5's pow(t, 1 / 2.2) in the context's arithmetic, from the oracle."""
    from oracle import oracle as O

    t = np.ascontiguousarray(t, F)
    y = np.full(t.shape, F(1.0) / F(2.2), F)
    return (O.ss_math("pow", t, y) if gl_stack else O.math("pow", t, y)).reshape(t.shape)


def display_bytes(linear, tone_name="clip", white=4.0, gl_stack=False):
    """Steps 2-5 on rm_present_linear's output [H, W, 4]: the RGBA8 canvas."""
    t = tone(np.asarray(linear, F)[..., :3], tone_name, white)
    out = np.empty(t.shape[:2] + (4,), np.uint8)
    out[..., :3] = unorm8(gamma(t, gl_stack), gl_stack)
    out[..., 3] = 255
    return out
