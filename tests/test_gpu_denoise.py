"""The denoiser on the MI355X (rm_denoise*, rm_frame_kernels.inc "denoise"): the kernels against the float64 restatement
(tests/denoise_ref.py), the present path, the device variant, quality on the fast build's renders, and both hosts."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as R
import golden_cases as GC
from raymarching_engine_amd import abi, capture, job as J, native, scene as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def random_planes(H, W, k, seed):
    """Planes after k samples with sky pixels (zero normal, +inf or 1e8 depth), NaN / inf colours and albedo 0."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32) * k
    n = rng.normal(size=(H, W, 4)).astype(np.float32) * k
    a = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32) * k
    a[..., 3] = rng.uniform(0.5, 10.0, (H, W)).astype(np.float32) * k
    # a few smooth regions, so that the weights are not all ~0 in every pass
    c[: H // 2, : W // 2, :3] = 0.7 * k
    a[: H // 2, : W // 2, :3] = 0.5 * k
    sky = rng.random((H, W)) < 0.1
    n[sky, :3] = 0.0
    a[sky, 3] = np.where(rng.random(int(sky.sum())) < 0.5, np.inf, 1e8)
    a[rng.random((H, W)) < 0.05, :3] = 0.0
    c[rng.random((H, W)) < 0.02, 0] = np.nan
    c[rng.random((H, W)) < 0.02, 1] = np.inf
    return c, n, a


def upload(ctx, planes, gbuffer):
    H, W = planes[0].shape[:2]
    fb = ctx.create_framebuffer(W, H, gbuffer=gbuffer)
    fb.upload(0, planes[0])
    for i in (1, 2):
        if gbuffer == "f16":
            with np.errstate(over="ignore"):
                fb.upload_raw(i, planes[i].astype(np.float16))
        else:
            fb.upload(i, planes[i])
    return fb


def widened(fb):
    return [fb.download(i) for i in range(3)]


def assert_close(got, ref):
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
        err = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    assert err.max(initial=0.0) <= 1e-4, f"max relative error {err.max()}"


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
@pytest.mark.parametrize("shape", [(1, 1), (19, 37), (173, 300)])
def test_kernel_matches_the_restatement(ctx, gbuffer, shape):
    H, W = shape
    k = 3
    fb = upload(ctx, random_planes(H, W, k, seed=H * W), gbuffer)
    planes = widened(fb)  # what the filter reads: the half planes widened exactly
    try:
        for L in range(9):
            p = dict(R.DEFAULTS, iterations=L)
            got = fb.denoise(k, p)
            ref = R.denoise(*planes, k, **p)
            if L == 0:
                assert np.array_equal(got.view(np.uint32), planes[0].view(np.uint32))
            else:
                assert_close(got, ref)
        p = dict(iterations=4, sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.1)  # sharper weights
        assert_close(fb.denoise(k, p), R.denoise(*planes, k, **p))
    finally:
        fb.destroy()


@pytest.mark.parametrize("gl_stack", [False, True])
@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_present_denoised_is_present_of_the_denoised_colour(ctx, gbuffer, gl_stack):
    H, W, k = 61, 83, 4
    planes = random_planes(H, W, k, seed=7)
    planes[1][..., 3] = np.linspace(0.0, 0.2, W, dtype=np.float32) * k  # a DoF radius: the blur of the present pass is on
    fb = upload(ctx, planes, gbuffer)
    ctx.set_gl_stack(gl_stack)
    try:
        plain = fb.present(k)
        for params in (True, {"iterations": 0}, {"iterations": 3, "sigma_color": 1.0}):
            den = fb.denoise(k, params)
            other = ctx.create_framebuffer(W, H, gbuffer=gbuffer)
            other.upload(0, den)
            for i in (1, 2):
                other.upload_raw(i, fb.download_raw(i))
            assert np.array_equal(fb.present(k, denoise=params), other.present(k))
            other.destroy()
        assert np.array_equal(fb.present(k), plain)  # without `denoise` the bytes are the present's
        assert np.array_equal(fb.present(k, denoise={"iterations": 0}), plain)
    finally:
        ctx.set_gl_stack(False)
        fb.destroy()


def test_device_variant_on_a_callers_stream(ctx):
    import torch

    H, W, k = 97, 131, 2
    fb = upload(ctx, random_planes(H, W, k, seed=3), "f16")
    try:
        want = fb.denoise(k)
        out = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            ctx.denoise_device(fb, k, out.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        fb.destroy()


def test_invalid_arguments_are_refused(ctx):
    """The library's own checks (the Python host checks the parameters first, so these go to the C entry points directly)."""
    lib = ctx.lib
    fb = ctx.create_framebuffer(16, 16)
    out = np.zeros((16, 16, 4), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))

    def call(f=fb, samples=1, **kw):
        p = abi.RmDenoise(**{**abi.DENOISE_DEFAULTS, **kw})
        return lib.rm_denoise(ctx.h, f.h, samples, C.byref(p), fp)

    try:
        assert call() == abi.RM_OK
        for kw in (dict(samples=0), dict(iterations=-1), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_normal=-1.0),
                   dict(sigma_depth=float("nan")), dict(sigma_color=float("inf"))):
            assert call(**kw) == abi.RM_ERR_INVALID, kw
        window = ctx.create_framebuffer(16, 16, 4, 8)
        assert call(window) == abi.RM_ERR_INVALID
        window.destroy()
        striped = ctx.create_striped_framebuffer(16, 16, 8, 2, 0)
        assert call(striped) == abi.RM_ERR_INVALID
        striped.destroy()
        other = native.Context(0)
        ofb = other.create_framebuffer(16, 16)
        assert call(ofb) == abi.RM_ERR_INVALID
        assert lib.rm_present_denoised(ctx.h, ofb.h, 1, None, out.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.RM_ERR_INVALID
        ofb.destroy()
        other.close()
        with pytest.raises(ValueError):
            fb.present(1, denoise={"iterations": 9})
    finally:
        fb.destroy()


# ---- quality on the fast build's renders ----------------------------------------------------------------------------

def _quality_jobs():
    bulb = S.Mandelbulb()
    csg = S.CsgScene().box((0, 0, 0), (1.0, 0.6, 0.8)).subtract().sphere((0.4, 0.3, -0.6), 0.7).smooth_union(0.3).sphere((-1.2, 0.2, 0.0), 0.5)
    return {
        "mandelbulb": (bulb, J.make_schema(bulb, 256, 256, counts=(64, 16), render_mode="full", position=(0, 0, -2.5),
                                           lights=[J.point_light((2.0, 3.0, -4.0))])),
        "csg_dof": (csg, J.make_schema(csg, 256, 256, counts=(48, 24), render_mode="full", position=(0.3, 0.2, -4.0), lights=GC.LIGHT,
                                       dof_amount=0.02, dof_distance=3.5)),
    }


# The CSG scene with depth of field does not reach the CPU test's bars: measured on MI355X, denoised / raw MSE 0.62 (f32) and
# 0.66 (f16), and on its edges -- blurred by the depth of field in the colour more than in the accumulated guides -- the
# unguided filter does better in f32.  It is held to "better than the raw frame" only.
FULL_BARS = ("mandelbulb",)


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
@pytest.mark.parametrize("name", ["mandelbulb", "csg_dof"])
def test_quality_on_fast_renders(ctx, name, gbuffer, tmp_path):
    sc, schema = _quality_jobs()[name]
    h = ctx.create_scene(sc)
    J.reset_halton()
    noise = np.array([J.next_rand_noise() for _ in range(4 + 1024)], np.float32)
    u = J.uniforms_from_schema(schema, (0.5, 0.5))
    lo, hi = ctx.create_framebuffer(256, 256, gbuffer=gbuffer), ctx.create_framebuffer(256, 256, gbuffer=gbuffer)
    try:
        ctx.render_samples(h, lo, u, noise[:4], None, abi.RM_RENDER_FAST)
        for i in range(4, 4 + 1024, 256):
            ctx.render_samples(h, hi, u, noise[i:i + 256], None, abi.RM_RENDER_FAST)
        low, high = widened(lo), widened(hi)
        got = lo.denoise(4)
        ref = R.displayed(high[0], 1024)
        edges = R.edge_mask(high[1], high[2], 1024)
        raw_d, den_d = R.displayed(low[0], 4), R.displayed(got, 4)
        ung_d = R.displayed(lo.denoise(4, dict(sigma_normal=3.0e38, sigma_depth=3.0e38)), 4)
        q = {"raw": R.mse(raw_d, ref), "denoised": R.mse(den_d, ref), "unguided": R.mse(ung_d, ref),
             "raw_edges": R.mse(raw_d, ref, edges), "denoised_edges": R.mse(den_d, ref, edges), "unguided_edges": R.mse(ung_d, ref, edges)}
        print(name, gbuffer, json.dumps({k: round(v, 6) for k, v in q.items()}), "ratio", q["denoised"] / q["raw"])
        # the PNG capture: without `denoise` the present's bytes, with it the denoised present's
        capture.save_png(lo, 4, str(tmp_path / "raw.png"))
        capture.save_png(lo, 4, str(tmp_path / "denoised.png"), denoise=True)
        assert np.array_equal(capture.decode_png((tmp_path / "raw.png").read_bytes()), lo.present(4)[::-1])
        assert np.array_equal(capture.decode_png((tmp_path / "denoised.png").read_bytes()), lo.present(4, denoise=True)[::-1])
        assert q["denoised"] < q["raw"] and q["denoised_edges"] < q["raw_edges"]
        if name in FULL_BARS:  # the CPU test's bars
            assert q["denoised"] <= 0.5 * q["raw"]
            assert q["denoised_edges"] < q["unguided_edges"]
    finally:
        lo.destroy()
        hi.destroy()
        h.destroy()


# ---- the hosts ----------------------------------------------------------------------------------------------------

def _job():
    sc = S.CsgScene().box((0, 0, 0), (1.0, 0.6, 0.8)).subtract().sphere((0.4, 0.3, -0.6), 0.7).smooth_union(0.3).sphere((-1.2, 0.2, 0.0), 0.5)
    schema = J.make_schema(sc, 64, 32, render_mode="full", counts=(48, 24), position=(0.3, 0.2, -4.0), lights=GC.LIGHT,
                           samples_per_pixel=4, sample_yield_interval=4, dof_amount=0.05, dof_distance=3.5, frameid=1)
    return sc, schema


def test_job_present_callback_can_denoise():
    sc, schema = _job()
    c = J.RenderJobContext(0, gbuffer="f16")
    try:
        frames = []

        def cb(schema_, context, fb, samples):
            if samples > 0:
                frames.append((samples, fb.present(samples, denoise=True), fb.present(samples)))

        J.reset_halton()
        assert J.drain(J.do_render_job(schema, c)(cb)) == {"success": True}
        samples, den, plain = frames[-1]
        fb = c.fbo_create(64, 32, 1)
        assert np.array_equal(den, fb.present(samples, denoise=True)) and np.array_equal(plain, fb.present(samples))
        assert not np.array_equal(den, plain)
    finally:
        c.close()


@pytest.mark.skipif(shutil.which("node") is None or not (JS / "rm_napi.node").exists(), reason="node or the addon is missing")
def test_node_host_gives_the_python_bytes(tmp_path):
    sc, schema = _job()
    c = J.RenderJobContext(0, gbuffer="f16")
    try:
        frames = []
        J.reset_halton()
        J.drain(J.do_render_job(schema, c)(lambda s, cx, fb, n: frames.append((n, fb.present(n, denoise=True), fb.denoise(n, {"iterations": 3}))) if n > 0 else None))
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
  const ctx = new rm.RenderJobContext({{ gbuffer: "f16" }});
  rm.resetHalton();
  let last = null, den = null;
  const gen = (await rm.doRenderJob(schema, ctx))((s, c, fb, n) => {{ if (n > 0) {{ last = fb.present(n, {{ denoise: true }}); den = fb.denoise(n, {{ iterations: 3 }});
    if (!fb.toDataURL(n, {{ denoise: true }}).startsWith("data:image/png;base64,")) throw new Error("toDataURL"); }} }});
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
