"""The moments plane and the variance-guided denoiser on the MI355X (RM_FB_MOMENTS, rm_denoise_variance*): the moments bit for
bit against the GPU's own single samples and the oracle's, the planes unchanged by them, the kernels against the float64
restatement (tests/denoise_var_ref.py), the present and device variants, convergence on the fast build's renders, and both
hosts."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as R
import denoise_var_ref as V
from oracle import oracle as O
from raymarching_engine_amd import abi, capture, job as J, native, scene as S
from test_gpu_denoise import _job, _quality_jobs, assert_close, random_planes, upload, widened

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
N = 6  # samples of the bit-exact moments tests


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def _small_job(W=40, H=24):
    sc = S.CsgScene().box((0, 0, 0), (1.0, 0.6, 0.8)).subtract().sphere((0.4, 0.3, -0.6), 0.7).smooth_union(0.3).sphere((-1.2, 0.2, 0.0), 0.5)
    schema = J.make_schema(sc, W, H, counts=(48, 24), render_mode="full", position=(0.3, 0.2, -4.0), lights=[J.point_light((2.0, 3.0, -4.0))],
                           dof_amount=0.02, dof_distance=3.5)
    J.reset_halton()
    noise = np.array([J.next_rand_noise() for _ in range(N)], np.float32)
    return sc, schema, noise


def _uniforms(schema, blend):
    u = J.uniforms_from_schema(schema, (0.5, 0.5))
    if blend == "mix":
        u.blendMode, u.blendWithPreviousFactor = 0, 0.75
    else:
        u.blendMode = 1
    return u


def _single_samples(ctx, h, schema, noise, flags, W, H):
    """Each sample's colour contribution: one additive sample into a cleared framebuffer (0 + s = s)."""
    u = _uniforms(schema, "additive")
    fb = ctx.create_framebuffer(W, H)
    out = []
    try:
        ctx.set_sample_batch(1)
        for i in range(len(noise)):
            fb.clear()
            ctx.render_samples(h, fb, u, noise[i:i + 1], None, flags)
            out.append(fb.download(0))
    finally:
        fb.destroy()
        ctx.set_sample_batch(0)
    return out


CONFIGS = [  # (sample batch, samples in flight, extra flags, tile)
    (1, 1, 0, None), (8, 3, 0, None), (0, 3, 0, None), (0, 1, 0, None), (0, 3, abi.RM_RENDER_NO_OVERLAP, None), (0, 3, 0, (5, 3, 17, 11)),
]


@pytest.mark.parametrize("blend", ["additive", "mix"])
@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_moments_are_the_fp32_accumulation_of_the_gpus_own_samples(ctx, gbuffer, blend):
    W, H = 40, 24
    sc, schema, noise = _small_job(W, H)
    h = ctx.create_scene(sc)
    flags = abi.RM_RENDER_FAST
    try:
        singles = _single_samples(ctx, h, schema, noise, flags, W, H)
        u = _uniforms(schema, blend)
        want = V.accumulate_moments(singles, blend, u.blendWithPreviousFactor)
        for batch, sif, extra, tile in CONFIGS:
            ctx.set_sample_batch(batch)
            ctx.set_samples_in_flight(sif)
            with_m = ctx.create_framebuffer(W, H, gbuffer=gbuffer, moments=True)
            without = ctx.create_framebuffer(W, H, gbuffer=gbuffer)
            try:
                assert with_m.moments and not without.moments
                rect = abi.RmRect(*tile) if tile else None
                for fb in (with_m, without):
                    ctx.render_samples(h, fb, u, noise, rect, flags | extra)
                got = with_m.download_raw(abi.RM_PLANE_MOMENTS)
                expect = want.copy()
                if tile:
                    x, y, w, hh = tile
                    inside = np.zeros((H, W), bool)
                    inside[y:y + hh, x:x + w] = True
                    expect[~inside] = 0.0
                assert np.array_equal(got.view(np.uint32), expect.view(np.uint32)), (batch, sif, extra, tile)
                for i in range(3):  # the other planes are byte-identical with and without moments
                    assert np.array_equal(with_m.download_raw(i).view(np.uint8), without.download_raw(i).view(np.uint8)), (i, batch, sif, extra, tile)
            finally:
                with_m.destroy()
                without.destroy()
    finally:
        ctx.set_sample_batch(0)
        ctx.set_samples_in_flight(3)
        h.destroy()


def test_strict_moments_are_the_oracles(ctx):
    W, H = 40, 24
    sc, schema, noise = _small_job(W, H)
    u0 = _uniforms(schema, "additive")
    singles = []
    for i in range(3):
        one = O.Frame(W, H)
        u = J.uniforms_from_schema(schema, tuple(noise[i]))
        u.blendMode = 1
        O.render(sc, u, one, threads=min(16, O.host_cores()))
        singles.append(one.color)
    h = ctx.create_scene(sc)
    fb = ctx.create_framebuffer(W, H, moments=True)
    try:
        ctx.render_samples(h, fb, u0, noise[:3], None, abi.RM_RENDER_STRICT)
        want = V.accumulate_moments(singles)
        assert np.array_equal(fb.download_raw(abi.RM_PLANE_MOMENTS).view(np.uint32), want.view(np.uint32))
    finally:
        fb.destroy()
        h.destroy()


def test_moments_plane_access_clear_and_preview(ctx):
    W, H = 40, 24
    sc, schema, noise = _small_job(W, H)
    h = ctx.create_scene(sc)
    fb = ctx.create_framebuffer(W, H, moments=True)
    plain = ctx.create_framebuffer(W, H)
    try:
        assert fb.device_ptr(abi.RM_PLANE_MOMENTS) != 0 and plain.device_ptr(abi.RM_PLANE_MOMENTS) == 0
        assert np.all(fb.download_raw(abi.RM_PLANE_MOMENTS) == 0.0)
        with pytest.raises(native.RmError):
            plain.download_raw(abi.RM_PLANE_MOMENTS)
        data = np.arange(H * W * 2, dtype=np.float32).reshape(H, W, 2)
        fb.upload_raw(abi.RM_PLANE_MOMENTS, data)
        assert np.array_equal(fb.download_raw(abi.RM_PLANE_MOMENTS), data)
        fb.clear()
        assert np.all(fb.download_raw(abi.RM_PLANE_MOMENTS) == 0.0)
        preview = J.uniforms_from_schema(schema, (0.5, 0.5))
        preview.renderMode = 1
        ctx.render_samples(h, fb, preview, noise, None, abi.RM_RENDER_FAST)
        assert np.all(fb.download_raw(abi.RM_PLANE_MOMENTS) == 0.0)  # preview mode leaves the plane as it is
        lib = ctx.lib
        import ctypes as C

        out = C.c_void_p()
        assert lib.rm_fb_create_striped_fmt(ctx.h, W, H, 8, 2, 0, None, None, None, abi.RM_FB_MOMENTS, C.byref(out)) == abi.RM_ERR_INVALID
        assert lib.rm_fb_wrap_fmt(ctx.h, W, H, 0, H, C.c_void_p(fb.device_ptr(0)), None, None, abi.RM_FB_MOMENTS, C.byref(out)) == abi.RM_ERR_INVALID
        with pytest.raises(ValueError):
            native.Framebuffer(ctx, W, H, 0, 0, striped=(8, 2, 0, None, None, None), moments=True)
    finally:
        fb.destroy()
        plain.destroy()
        h.destroy()


def random_moments(H, W, k, seed):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.05, 1.5, (H, W))
    var = rng.uniform(0.01, 0.5, (H, W)) * mean
    M = np.empty((H, W, 2), np.float32)
    M[..., 0] = k * mean
    M[..., 1] = k * (mean * mean + var)
    M[: H // 3, : W // 3] = 0.0  # a corner of exactly zero variance next to noisy pixels (a flat sky against a surface)
    M[-(H // 4):, W // 2:, 0], M[-(H // 4):, W // 2:, 1] = k * 0.5, k * 0.35  # and a region of uniform moments
    return M


def upload_var(ctx, planes, M, gbuffer):
    H, W = planes[0].shape[:2]
    fb = ctx.create_framebuffer(W, H, gbuffer=gbuffer, moments=True)
    fb.upload(0, planes[0])
    for i in (1, 2):
        if gbuffer == "f16":
            with np.errstate(over="ignore"):
                fb.upload_raw(i, planes[i].astype(np.float16))
        else:
            fb.upload(i, planes[i])
    fb.upload_raw(abi.RM_PLANE_MOMENTS, M)
    return fb


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
@pytest.mark.parametrize("shape", [(1, 1), (19, 37), (173, 300)])
def test_kernel_matches_the_restatement(ctx, gbuffer, shape):
    H, W = shape
    k = 3
    M = random_moments(H, W, k, seed=H + W)
    fb = upload_var(ctx, random_planes(H, W, k, seed=H * W), M, gbuffer)
    planes = widened(fb)
    try:
        for L in range(9):
            p = dict(V.DEFAULTS, iterations=L)
            got = fb.denoise_variance(k, p)
            if L == 0:
                assert np.array_equal(got.view(np.uint32), planes[0].view(np.uint32))
            else:
                assert_close(got, V.denoise_variance(*planes, M, k, **p))
        p = dict(iterations=4, sigma_luminance=1.0, sigma_normal=0.5, sigma_depth=0.1)
        assert_close(fb.denoise_variance(k, p), V.denoise_variance(*planes, M, k, **p))
    finally:
        fb.destroy()


@pytest.mark.parametrize("gl_stack", [False, True])
@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_present_variant_is_present_of_the_filtered_colour(ctx, gbuffer, gl_stack):
    H, W, k = 61, 83, 4
    planes = random_planes(H, W, k, seed=7)
    planes[1][..., 3] = np.linspace(0.0, 0.2, W, dtype=np.float32) * k
    fb = upload_var(ctx, planes, random_moments(H, W, k, seed=8), gbuffer)
    ctx.set_gl_stack(gl_stack)
    try:
        plain = fb.present(k)
        for d in ("variance", {"mode": "variance", "iterations": 0}, {"mode": "variance", "iterations": 3, "sigma_luminance": 1.0},
                  abi.RmDenoiseVariance(iterations=2, sigma_luminance=2.0, sigma_normal=1.0, sigma_depth=0.5)):
            den = fb.denoise_variance(k, d)
            other = ctx.create_framebuffer(W, H, gbuffer=gbuffer)
            other.upload(0, den)
            for i in (1, 2):
                other.upload_raw(i, fb.download_raw(i))
            assert np.array_equal(fb.present(k, denoise=d), other.present(k))
            other.destroy()
        assert np.array_equal(fb.present(k), plain)
        assert np.array_equal(fb.present(k, denoise=True), fb.present(k, denoise={"mode": "atrous"}))  # today's filter, unchanged
    finally:
        ctx.set_gl_stack(False)
        fb.destroy()


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_zero_variance_pixels_come_back_unchanged(ctx, gbuffer):
    """No variance anywhere, luminances >= 4 % apart: every pass keeps every finite pixel (to fp32 rounding of the
    demodulation), at every iteration count -- the property convergence rests on."""
    from test_denoise_variance_cpu import _luminance_ladder

    H, W, k = 12, 12, 4
    c, n, a = _luminance_ladder(H, W, k, seed=11)
    c[5, 6, 1] = np.nan
    fb = upload_var(ctx, [c, n, a], np.zeros((H, W, 2), np.float32), gbuffer)
    try:
        fin = np.isfinite(c[..., :3]).all(-1)
        for L in range(1, 9):
            got = fb.denoise_variance(k, dict(V.DEFAULTS, iterations=L))
            assert np.allclose(got[fin], c[fin], rtol=1e-5, atol=0), L
            assert np.isnan(got[5, 6, 1])
    finally:
        fb.destroy()


def test_device_variant_on_a_callers_stream(ctx):
    import torch

    H, W, k = 97, 131, 2
    fb = upload_var(ctx, random_planes(H, W, k, seed=3), random_moments(H, W, k, seed=4), "f16")
    try:
        want = fb.denoise_variance(k)
        out = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            ctx.denoise_variance_device(fb, k, out.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        fb.destroy()


def test_invalid_arguments_are_refused(ctx):
    import ctypes as C

    lib = ctx.lib
    fb = ctx.create_framebuffer(16, 16, moments=True)
    plain = ctx.create_framebuffer(16, 16)
    out = np.zeros((16, 16, 4), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))

    def call(f=fb, samples=1, **kw):
        p = abi.RmDenoiseVariance(**{**abi.DENOISE_VARIANCE_DEFAULTS, **kw})
        return lib.rm_denoise_variance(ctx.h, f.h, samples, C.byref(p), fp)

    try:
        assert call() == abi.RM_OK
        assert lib.rm_denoise_variance(ctx.h, fb.h, 1, None, fp) == abi.RM_OK
        for kw in (dict(samples=0), dict(iterations=-1), dict(iterations=9), dict(sigma_luminance=0.0), dict(sigma_normal=-1.0),
                   dict(sigma_depth=float("nan")), dict(sigma_luminance=float("inf")), dict(reserved=1)):
            assert call(**kw) == abi.RM_ERR_INVALID, kw
        assert call(plain) == abi.RM_ERR_INVALID  # no moments plane
        assert lib.rm_present_denoised_variance(ctx.h, plain.h, 1, None, out.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.RM_ERR_INVALID
        window = ctx.create_framebuffer(16, 16, 4, 8, moments=True)
        assert call(window) == abi.RM_ERR_INVALID
        window.destroy()
        with pytest.raises(native.RmError):
            plain.present(1, denoise="variance")
        with pytest.raises(ValueError):
            fb.present(1, denoise={"mode": "variance", "iterations": 9})
    finally:
        fb.destroy()
        plain.destroy()


# ---- convergence on the fast build's renders --------------------------------------------------------------------------

@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
@pytest.mark.parametrize("name", ["mandelbulb", "csg_dof"])
def test_quality_converges_on_fast_renders(ctx, name, gbuffer, tmp_path):
    sc, schema = _quality_jobs()[name]
    h = ctx.create_scene(sc)
    J.reset_halton()
    noise = np.array([J.next_rand_noise() for _ in range(64 + 1024)], np.float32)
    u = J.uniforms_from_schema(schema, (0.5, 0.5))
    lo, hi = ctx.create_framebuffer(256, 256, gbuffer=gbuffer, moments=True), ctx.create_framebuffer(256, 256, gbuffer=gbuffer)
    try:
        for i in range(64, 64 + 1024, 256):
            ctx.render_samples(h, hi, u, noise[i:i + 256], None, abi.RM_RENDER_FAST)
        high = widened(hi)
        ref = R.displayed(high[0], 1024)
        edges = R.edge_mask(high[1], high[2], 1024)
        done, failures = 0, []
        for k in (4, 16, 64):
            ctx.render_samples(h, lo, u, noise[done:k], None, abi.RM_RENDER_FAST)
            done = k
            raw_d = R.displayed(lo.download(0), k)
            var_d = R.displayed(lo.denoise_variance(k), k)
            old_d = R.displayed(lo.denoise(k), k)
            q = {"raw": R.mse(raw_d, ref), "variance": R.mse(var_d, ref), "atrous": R.mse(old_d, ref),
                 "raw_edges": R.mse(raw_d, ref, edges), "variance_edges": R.mse(var_d, ref, edges), "atrous_edges": R.mse(old_d, ref, edges)}
            print(name, gbuffer, k, json.dumps({key: round(v, 6) for key, v in q.items()}), "ratio", round(q["variance"] / q["raw"], 3),
                  "edges", round(q["variance_edges"] / q["raw_edges"], 3), "atrous", round(q["atrous"] / q["raw"], 3))
            if k == 4:
                # the CSG scene with depth of field: today's filter reaches 0.62 / 0.66 there, so it is held to "better than raw"
                if name == "mandelbulb" and not q["variance"] <= 0.5 * q["raw"]:
                    failures.append((k, "0.5 x raw"))
                if not q["variance"] <= q["raw"]:
                    failures.append((k, "raw"))
                if not q["variance"] <= 1.1 * q["atrous"]:
                    failures.append((k, "1.1 x atrous"))
            else:
                if not q["variance"] <= q["raw"]:
                    failures.append((k, "raw"))
                if not q["variance_edges"] <= q["raw_edges"]:
                    failures.append((k, "raw edges"))
            if k == 4:  # the PNG capture follows present
                capture.save_png(lo, 4, str(tmp_path / "variance.png"), denoise="variance")
                assert np.array_equal(capture.decode_png((tmp_path / "variance.png").read_bytes()), lo.present(4, denoise="variance")[::-1])
        assert not failures, failures
    finally:
        lo.destroy()
        hi.destroy()
        h.destroy()


# ---- the hosts ----------------------------------------------------------------------------------------------------

def test_job_present_callback_gives_the_python_bytes():
    sc, schema = _job()
    c = J.RenderJobContext(0, gbuffer="f16", moments=True)
    try:
        frames = []
        J.reset_halton()
        assert J.drain(J.do_render_job(schema, c)(J.collect_presents(frames, denoise="variance"))) == {"success": True}
        samples, den = frames[-1]
        fb = c.fbo_create(64, 32, 1)
        assert fb.moments
        assert np.array_equal(den, fb.present(samples, denoise="variance"))
        assert not np.array_equal(den, fb.present(samples))
    finally:
        c.close()


@pytest.mark.skipif(shutil.which("node") is None or not (JS / "rm_napi.node").exists(), reason="node or the addon is missing")
def test_node_host_gives_the_python_bytes(tmp_path):
    sc, schema = _job()
    c = J.RenderJobContext(0, gbuffer="f16", moments=True)
    try:
        frames = []
        J.reset_halton()
        J.drain(J.do_render_job(schema, c)(lambda s, cx, fb, n: frames.append(
            (n, fb.present(n, denoise={"mode": "variance", "iterations": 4}), fb.denoise_variance(n, {"iterations": 3}))) if n > 0 else None))
        n, want8, want32 = frames[-1]
    finally:
        c.close()
    plain = {k: v for k, v in schema.items() if k != "sdfScene"}
    out8, out32 = tmp_path / "canvas.rgba", tmp_path / "denoised.f32"
    script = f"""
const fs = require("fs");
const rm = require({str(JS / "index.js")!r});
(async () => {{
  const schema = Object.assign({json.dumps(plain)}, {{
    sdfScene: new rm.CsgScene().box([0, 0, 0], [1.0, 0.6, 0.8]).subtract().sphere([0.4, 0.3, -0.6], 0.7).smoothUnion(0.3).sphere([-1.2, 0.2, 0.0], 0.5) }});
  const ctx = new rm.RenderJobContext({{ gbuffer: "f16", moments: true }});
  rm.resetHalton();
  let last = null, den = null;
  const gen = (await rm.doRenderJob(schema, ctx))((s, c, fb, n) => {{ if (n > 0) {{
    last = fb.present(n, {{ denoise: {{ mode: "variance", iterations: 4 }} }}); den = fb.denoiseVariance(n, {{ iterations: 3 }});
    if (!fb.toDataURL(n, {{ denoise: "variance" }}).startsWith("data:image/png;base64,")) throw new Error("toDataURL"); }} }});
  let r = gen.next();
  while (!r.done) r = gen.next();
  if (!r.value.success) throw new Error(JSON.stringify(r.value));
  fs.writeFileSync({str(out8)!r}, Buffer.from(last));
  fs.writeFileSync({str(out32)!r}, Buffer.from(den.buffer));
  ctx.close();
}})().catch((e) => {{ console.error(e); process.exit(1); }});
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(out8, np.uint8).reshape(32, 64, 4), want8)
    assert np.array_equal(np.fromfile(out32, np.float32).reshape(32, 64, 4).view(np.uint32), want32.view(np.uint32))
