"""A float64 numpy restatement of the variance-guided denoiser (include/hip_raymarch.h rm_denoise_variance, INTEGRATION.md
"Denoising"): the a-trous filter of tests/denoise_ref.py with the colour weight of SVGF (Schied et al. 2017) -- luminance
distance relative to each pixel's own noise, estimated from the per-pixel moments plane.  Written from the statement, not
from the kernel; plus the fp32 luminance rule of the moments plane and the quality measures of the tests."""
from __future__ import annotations

import numpy as np

import denoise_ref as R

DEFAULTS = dict(iterations=3, sigma_luminance=4.0, sigma_normal=1.0, sigma_depth=0.2)  # rm_denoise_variance_default
EPS = 1e-6  # the floor of the epsilon added to sigma_l sqrt(g_p) ...
EPS_REL = 1e-3  # ... which is EPS_REL |lum(x_p)| above it: far above the fp32 resolution of the luminance, so that a pixel of zero
# variance weighs its taps by a well-conditioned exp(-|dl| / eps) (taps within ~0.1 % of its luminance still count)
G3 = np.array([0.25, 0.5, 0.25])  # the 3x3 prefilter (1, 2, 1)^2 / 16
LUM = (0.2126, 0.7152, 0.0722)


def sample_luminance(c) -> np.ndarray:
    """l of one sample's colour contribution [.., >= 3] in fp32, as the moments plane computes it:
    (0.2126f * r + 0.7152f * g) + 0.0722f * b, every product and sum rounded to fp32 separately."""
    c = np.asarray(c, np.float32)
    w = [np.float32(v) for v in LUM]
    with np.errstate(all="ignore"):
        return ((w[0] * c[..., 0]) + (w[1] * c[..., 1])) + (w[2] * c[..., 2])


def accumulate_moments(samples, blend_mode: str = "additive", factor: float = 0.0, moments=None) -> np.ndarray:
    """The moments plane [H, W, 2] fp32 after blending the per-sample contributions `samples` (an iterable of [H, W, >= 3]),
    in order, by the colour plane's rule: (M.x + l, M.y + l*l) additive, gmix(l, M, f) = f * (M - l) + l in mix mode."""
    M = None if moments is None else np.array(moments, np.float32)
    f = np.float32(factor)
    with np.errstate(all="ignore"):
        for s in samples:
            l = sample_luminance(s)
            v = np.stack([l, l * l], -1)
            if M is None:
                M = np.zeros(v.shape, np.float32)
            M = (M + v) if blend_mode == "additive" else (f * (M - v)) + v
    return M


def luminance(x) -> np.ndarray:
    return LUM[0] * x[..., 0] + LUM[1] * x[..., 1] + LUM[2] * x[..., 2]


def prepare_variance(moments, m, samples: int) -> np.ndarray:
    """v_p = max(0, M.y s - (M.x s)^2) s / max(lum(m_p), 1e-3)^2, and 0 where that is not finite."""
    s = float(np.float32(1.0) / np.float32(samples))
    M = np.asarray(moments, np.float64)
    with np.errstate(all="ignore"):
        mu = M[..., 0] * s
        v = np.maximum(0.0, M[..., 1] * s - mu * mu) * s / np.maximum(luminance(m), 1e-3) ** 2
    return np.where(np.isfinite(v), v, 0.0)


def prefilter(v) -> np.ndarray:
    """g = the 3x3 Gaussian (1, 2, 1)^2 / 16 of v; taps outside the image are skipped and the sum is divided by the weight of
    the taps inside."""
    H, W = v.shape
    inside = np.ones((H, W), bool)
    acc, ws = np.zeros((H, W)), np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            w = G3[dy + 1] * G3[dx + 1] * R._shift(inside, dy, dx, False)
            acc += w * R._shift(v, dy, dx, 0.0)
            ws += w
    return acc / ws


def epsilon(l):
    """eps_p = max(EPS_REL |lum(x_p)|, EPS)."""
    with np.errstate(invalid="ignore"):
        return np.maximum(EPS_REL * np.abs(l), EPS)


def variance_pass(x, v, n, z, i: int, sigma_luminance: float, sigma_normal: float, sigma_depth: float):
    """Pass i (step 2^i): (x', v') from the demodulated colour x and its variance v, guided by n and z."""
    H, W = x.shape[:2]
    h = 2 ** i
    x_fin = np.isfinite(x).all(-1)
    z_fin = np.isfinite(z)
    g = prefilter(v)
    lp = luminance(x)
    inv_l = 1.0 / (sigma_luminance * np.sqrt(g) + epsilon(lp))
    acc, accv, wsum = np.zeros_like(x), np.zeros((H, W)), np.zeros((H, W))
    inside = np.ones((H, W), bool)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                xq = R._shift(x, dy * h, dx * h, np.nan)
                vq = R._shift(v, dy * h, dx * h, 0.0)
                nq = R._shift(n, dy * h, dx * h, 0.0)
                zq = R._shift(z, dy * h, dx * h, 0.0)
                ok = R._shift(inside, dy * h, dx * h, False) & np.isfinite(xq).all(-1)
                w_l = np.exp(-np.abs(lp - luminance(xq)) * inv_l)
                w_n = np.exp(-((n - nq) ** 2).sum(-1) / sigma_normal ** 2)
                if dx == 0 and dy == 0:
                    w_z = np.ones((H, W))
                else:
                    zq_fin = np.isfinite(zq)
                    both = z_fin & zq_fin
                    d = np.where(both, np.abs(z - zq), 0.0)
                    w_z = np.exp(-d / (sigma_depth * np.maximum(np.where(z_fin, z, 1.0), 1e-6) * h * np.hypot(dx, dy)))
                    w_z = np.where(both, w_z, np.where(~z_fin & ~zq_fin, 1.0, 0.0))
                w = np.where(ok, R.B[dx + 2] * R.B[dy + 2] * w_l * w_n * w_z, 0.0)
                acc += w[..., None] * np.where(ok[..., None], xq, 0.0)
                accv += w * w * np.where(ok, vq, 0.0)
                wsum += w
        xo = acc / wsum[..., None]
        vo = accv / (wsum * wsum)
    return np.where(x_fin[..., None], xo, x), np.where(x_fin, vo, v)


def denoise_variance(color, normal_dof, albedo_depth, moments, samples: int, iterations: int = DEFAULTS["iterations"],
                     sigma_luminance: float = DEFAULTS["sigma_luminance"], sigma_normal: float = DEFAULTS["sigma_normal"],
                     sigma_depth: float = DEFAULTS["sigma_depth"]) -> np.ndarray:
    """The filtered colour plane [H, W, 4] (float64, colour-plane units) of the planes after `samples` samples."""
    c = np.asarray(color, np.float64)
    if iterations == 0:
        return c.copy()
    x, n, z, m = R.prepare(color, normal_dof, albedo_depth, samples)
    v = prepare_variance(moments, m, samples)
    for i in range(iterations):
        x, v = variance_pass(x, v, n, z, i, sigma_luminance, sigma_normal, sigma_depth)
    out = np.empty_like(c)
    with np.errstate(all="ignore"):
        out[..., :3] = x * m * float(samples)
    out[..., 3] = c[..., 3]
    return out


def quality(low_color, low_normal, low_albedo, low_moments, low_samples: int, ref_color, ref_normal, ref_albedo, ref_samples: int,
            params=None):
    """MSE against the converged frame of the raw frame, today's filter (denoise_ref defaults) and the variance-guided filter,
    on the whole frame and on edge pixels, as a dict."""
    p = dict(DEFAULTS, **(params or {}))
    ref = R.displayed(ref_color, ref_samples)
    edges = R.edge_mask(ref_normal, ref_albedo, ref_samples)
    raw = R.displayed(low_color, low_samples)
    old = R.displayed(R.denoise(low_color, low_normal, low_albedo, low_samples), low_samples)
    var = R.displayed(denoise_variance(low_color, low_normal, low_albedo, low_moments, low_samples, **p), low_samples)
    return {"raw": R.mse(raw, ref), "atrous": R.mse(old, ref), "variance": R.mse(var, ref),
            "raw_edges": R.mse(raw, ref, edges), "atrous_edges": R.mse(old, ref, edges), "variance_edges": R.mse(var, ref, edges)}
