"""A float64 numpy restatement of the denoiser (include/hip_raymarch.h rm_denoise, INTEGRATION.md "Denoising"): the
edge-avoiding a-trous wavelet filter of Dammertz et al. 2010, guided by the G-buffer, with albedo demodulation.  Written
from the statement, not from the kernel, and vectorised over the image; plus the quality measures the tests score a
denoised frame with."""
from __future__ import annotations

import numpy as np

B = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0])
DEFAULTS = dict(iterations=5, sigma_color=2.5, sigma_normal=2.0, sigma_depth=0.2)  # rm_denoise_default
UNGUIDED = dict(sigma_normal=np.inf, sigma_depth=np.inf)  # the same filter on colour alone


def prepare(color, normal_dof, albedo_depth, samples: int):
    """(x, n, z, m): demodulated colour [H, W, 3], unit normal (0 for sky) [H, W, 3], depth [H, W], modulation [H, W, 3]."""
    s = float(np.float32(1.0) / np.float32(samples))  # the present pass's own 1.0f / k
    c, nd, ad = (np.asarray(a, np.float64) for a in (color, normal_dof, albedo_depth))
    with np.errstate(all="ignore"):
        m = np.fmax(ad[..., :3] * s, 1e-3)
        x = c[..., :3] * s / m
        n = nd[..., :3] * s
        length = np.sqrt((n * n).sum(-1))
        ok = (length >= 1e-6) & np.isfinite(length)
        n = np.where(ok[..., None], n / np.where(ok, length, 1.0)[..., None], 0.0)
        z = ad[..., 3] * s
    return x, n, z, m


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


def atrous_pass(x, n, z, i: int, sigma_color: float, sigma_normal: float, sigma_depth: float):
    """Pass i (step 2^i) of the filter on the demodulated colour x, guided by n and z."""
    H, W = x.shape[:2]
    h = 2 ** i
    x_fin = np.isfinite(x).all(-1)
    z_fin = np.isfinite(z)
    acc = np.zeros_like(x)
    wsum = np.zeros((H, W))
    inside = np.ones((H, W), bool)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                xq = _shift(x, dy * h, dx * h, np.nan)
                nq = _shift(n, dy * h, dx * h, 0.0)
                zq = _shift(z, dy * h, dx * h, 0.0)
                ok = _shift(inside, dy * h, dx * h, False) & np.isfinite(xq).all(-1)
                w_c = np.exp(-((x - xq) ** 2).sum(-1) / (sigma_color ** 2 * 4.0 ** -i))
                w_n = np.exp(-((n - nq) ** 2).sum(-1) / sigma_normal ** 2)
                if dx == 0 and dy == 0:
                    w_z = np.ones((H, W))
                else:
                    zq_fin = np.isfinite(zq)
                    both = z_fin & zq_fin
                    d = np.where(both, np.abs(z - zq), 0.0)
                    w_z = np.exp(-d / (sigma_depth * np.maximum(np.where(z_fin, z, 1.0), 1e-6) * h * np.hypot(dx, dy)))
                    w_z = np.where(both, w_z, np.where(~z_fin & ~zq_fin, 1.0, 0.0))
                w = np.where(ok, B[dx + 2] * B[dy + 2] * w_c * w_n * w_z, 0.0)
                acc += w[..., None] * np.where(ok[..., None], xq, 0.0)
                wsum += w
        out = acc / wsum[..., None]
    return np.where(x_fin[..., None], out, x)


def denoise(color, normal_dof, albedo_depth, samples: int, iterations: int = DEFAULTS["iterations"],
            sigma_color: float = DEFAULTS["sigma_color"], sigma_normal: float = DEFAULTS["sigma_normal"],
            sigma_depth: float = DEFAULTS["sigma_depth"]) -> np.ndarray:
    """The filtered colour plane [H, W, 4] (float64, colour-plane units) of the planes after `samples` samples."""
    c = np.asarray(color, np.float64)
    if iterations == 0:
        return c.copy()
    x, n, z, m = prepare(color, normal_dof, albedo_depth, samples)
    for i in range(iterations):
        x = atrous_pass(x, n, z, i, sigma_color, sigma_normal, sigma_depth)
    out = np.empty_like(c)
    with np.errstate(all="ignore"):
        out[..., :3] = x * m * float(samples)
    out[..., 3] = c[..., 3]
    return out


# ---- quality -------------------------------------------------------------------------------------------------------

def displayed(color, samples: int) -> np.ndarray:
    """What the present pass shows before its gamma, clipped to [0, 1]: colour.rgb / samples (NaN as 0)."""
    return np.clip(np.nan_to_num(np.asarray(color, np.float64)[..., :3] / samples, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)


def edge_mask(normal_dof, albedo_depth, samples: int) -> np.ndarray:
    """Pixels whose 3x3 neighbourhood (in the given, well-converged G-buffer) holds a depth ratio > 1.1 or a normal dot
    product < 0.9; sky (zero normal) against a surface counts as an edge, sky against sky does not."""
    c0 = np.zeros(np.shape(normal_dof)[:2] + (4,))
    _, n, z, _ = prepare(c0, normal_dof, albedo_depth, samples)
    sky = ~(n != 0).any(-1)
    z_fin = np.isfinite(z) & (z > 0)
    edge = np.zeros(z.shape, bool)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                inside = _shift(np.ones(z.shape, bool), dy, dx, False)
                nq, zq, skyq = _shift(n, dy, dx, 0.0), _shift(z, dy, dx, 0.0), _shift(sky, dy, dx, True)
                zq_fin = np.isfinite(zq) & (zq > 0)
                depth_edge = np.where(z_fin & zq_fin, np.maximum(z / zq, zq / z) > 1.1, z_fin != zq_fin)
                normal_edge = np.where(~sky & ~skyq, (n * nq).sum(-1) < 0.9, sky != skyq)
                edge |= inside & (depth_edge | normal_edge)
    return edge


def mse(a, b, mask=None) -> float:
    d = ((np.asarray(a) - np.asarray(b)) ** 2).mean(-1)
    return float(d[mask].mean() if mask is not None else d.mean())


def quality(low_color, low_normal, low_albedo, low_samples: int, ref_color, ref_normal, ref_albedo, ref_samples: int, params=None):
    """MSE against the converged frame of: the raw frame, the denoised frame, the unguided filter (whole frame and edge
    pixels), as a dict."""
    p = dict(DEFAULTS, **(params or {}))
    ref = displayed(ref_color, ref_samples)
    edges = edge_mask(ref_normal, ref_albedo, ref_samples)
    raw = displayed(low_color, low_samples)
    den = displayed(denoise(low_color, low_normal, low_albedo, low_samples, **p), low_samples)
    ung = displayed(denoise(low_color, low_normal, low_albedo, low_samples, **dict(p, **UNGUIDED)), low_samples)
    return {"raw": mse(raw, ref), "denoised": mse(den, ref), "unguided": mse(ung, ref),
            "raw_edges": mse(raw, ref, edges), "denoised_edges": mse(den, ref, edges), "unguided_edges": mse(ung, ref, edges),
            "edge_fraction": float(edges.mean())}
