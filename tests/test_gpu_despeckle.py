"""The firefly filter on the MI355X (rm_filter*, rm_frame_kernels.inc "despeckle"): the kernel against the float32 restatement
(tests/despeckle_ref.py), the chain as an exact composition of its stages, off being off, the device variant, every refusal,
both hosts, and one measurement on the fast build's renders."""
import ctypes as C
import itertools
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as R
import despeckle_ref as D
from raymarching_engine_amd import abi, capture, job as J, native, scene as S
from test_gpu_denoise import _job, _quality_jobs, random_planes, upload, widened
from test_gpu_denoise_variance import random_moments

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def with_outliers(c, k):
    """random_planes' colour plus outliers where the kernel's tiles meet: the corners, x or y in {15, 16} and {31, 32}, an
    adjacent pair and an L-shaped triple (whatever of them fits the frame)."""
    H, W = c.shape[:2]
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    spots += [(y, x) for y in (15, 16, 31, 32) for x in (3, 15, 16, 31, 32, W - 2)]
    spots += [(y, x) for x in (15, 16, 31, 32) for y in (5, H - 3)]
    spots += [(9, 22), (9, 23)]                 # an adjacent pair
    spots += [(24, 7), (25, 7), (25, 8)]        # an L-shaped triple
    spots += [(12, 15), (12, 16), (15, 40), (16, 40)]  # pairs across a tile seam
    for i, (y, x) in enumerate(spots):
        if 0 <= y < H and 0 <= x < W:
            c[y, x, :3] = np.float32(40.0 + 7.0 * i) * k * np.array([1.0, 0.6, 0.3], np.float32)
    return c


PARAMS = [dict(radius=r, rank=n, gain=g, floor=f, repair=p)
          for r, n, g, f, p in itertools.product((1, 2), (0, 1, 3), (1.0, 3.0), (0.0, 0.5), (0, 1))]


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 3), (19, 37), (40, 50)])
def test_kernel_matches_the_restatement(ctx, shape):
    """Both sides are fp32 in the stated order, so the set of changed pixels is equal exactly and every unchanged pixel is bitwise
    the colour plane's; a changed value carries two fp32 roundings on either side plus the division: 1e-6 relative, about 3 ulp."""
    H, W = shape
    k = 3
    planes = list(random_planes(H, W, k, seed=H * W + 1))
    planes[0] = with_outliers(planes[0], k)
    fb = upload(ctx, planes, "f16" if H % 2 else "f32")
    try:
        c = fb.download(0)
        assert np.array_equal(bits(c), bits(planes[0]))
        total = 0
        for p in PARAMS:
            got = fb.filter(k, despeckle=p)
            ref = D.despeckle(c, k, **p)
            ch_got, ch_ref = D.changed(got, c), D.changed(ref, c)
            assert np.array_equal(ch_got, ch_ref), (p, np.argwhere(ch_got != ch_ref)[:8].tolist())
            assert np.array_equal(bits(got)[~ch_got], bits(c)[~ch_got]), p
            assert np.array_equal(bits(got[..., 3]), bits(c[..., 3])), p
            g, r = got[ch_got][:, :3].astype(np.float64), ref[ch_ref][:, :3].astype(np.float64)
            assert np.isfinite(g).all() and np.isfinite(r).all(), p  # a clamp scales a valid colour, a repair is taken only when finite
            assert (np.abs(g - r) <= 1e-6 * np.abs(r)).all(), (p, float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-30), initial=0.0)))
            total += int(ch_got.sum())
        print(shape, "changed pixels over", len(PARAMS), "parameter sets:", total)
        if H * W > 2:
            assert total > 0  # the planes do exercise the clamp and the repair
    finally:
        fb.destroy()


def upload_all(ctx, planes, M, gbuffer):
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


def raw_planes(fb):
    return [fb.download_raw(i).copy() for i in range(4 if fb.moments else 3)]


@pytest.mark.parametrize("gl_stack", [False, True])
@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_the_chain_is_the_exact_composition_of_its_stages(ctx, gbuffer, gl_stack):
    """The despeckled colour uploaded into a second framebuffer with the same guides and moments: the chain's denoise stage and
    its present are then that framebuffer's, bit for bit and byte for byte."""
    H, W, k = 61, 83, 4
    planes = list(random_planes(H, W, k, seed=7))
    planes[0] = with_outliers(planes[0], k)
    planes[1][..., 3] = np.linspace(0.0, 0.2, W, dtype=np.float32) * k  # a DoF radius: the blur of the present pass is on
    fb = upload_all(ctx, planes, random_moments(H, W, k, seed=8), gbuffer)
    other = ctx.create_framebuffer(W, H, gbuffer=gbuffer, moments=True)
    ctx.set_gl_stack(gl_stack)
    try:
        before = raw_planes(fb)
        for i in (1, 2, 3):
            other.upload_raw(i, before[i])
        for p in (True, dict(radius=1, rank=0, gain=1.5, floor=0.0, repair=0)):
            desp = fb.filter(k, despeckle=p)
            assert D.changed(desp, before[0]).any()
            other.upload(0, desp)
            assert np.array_equal(bits(other.download(0)), bits(desp))
            for d in (None, True, {"iterations": 3, "sigma_color": 1.0}, {"iterations": 0}, "variance",
                      {"mode": "variance", "iterations": 2, "sigma_luminance": 1.0}, {"mode": "variance", "iterations": 0}):
                got = fb.filter(k, despeckle=p, denoise=d)
                if d is None:
                    want = desp
                elif native.denoise_mode(d)[0] == "variance":
                    want = other.denoise_variance(k, d)
                else:
                    want = other.denoise(k, d)
                assert np.array_equal(bits(got), bits(want)), (p, d)
                assert np.array_equal(fb.present(k, despeckle=p, denoise=d), other.present(k, denoise=d)), (p, d)
        # with the despeckle stage off the chain is exactly today's entry points
        for d in (True, "variance", {"iterations": 0}):
            want = fb.denoise_variance(k, d) if d == "variance" else fb.denoise(k, d)
            assert np.array_equal(bits(fb.filter(k, denoise=d)), bits(want))
        after = raw_planes(fb)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    finally:
        ctx.set_gl_stack(False)
        fb.destroy()
        other.destroy()


def test_off_is_off(ctx):
    H, W, k = 33, 47, 2
    planes = list(random_planes(H, W, k, seed=5))
    planes[0] = with_outliers(planes[0], k)
    planes[1][..., 3] = 0.05 * k
    fb = upload(ctx, planes, "f32")
    try:
        before = raw_planes(fb)
        plain = fb.present(k)
        assert np.array_equal(fb.present(k, despeckle=None), plain)
        assert np.array_equal(fb.present(k, denoise=True, despeckle=None), fb.present(k, denoise=True))
        assert np.array_equal(bits(fb.filter(k)), bits(before[0]))
        f = native.filters()
        out = np.empty((H, W, 4), np.uint8)
        ctx._check(ctx.lib.rm_present_filtered(ctx.h, fb.h, k, C.byref(f), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        assert np.array_equal(out, plain)  # both stages off: rm_present's bytes
        assert not np.array_equal(fb.present(k, despeckle=True), plain)
        fb.filter(k, despeckle=True, denoise=True)
        after = raw_planes(fb)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    finally:
        fb.destroy()


def test_device_variant_on_a_callers_stream(ctx):
    import torch

    H, W, k = 97, 131, 2
    planes = list(random_planes(H, W, k, seed=3))
    planes[0] = with_outliers(planes[0], k)
    fb = upload(ctx, planes, "f16")
    try:
        s = torch.cuda.Stream(device=0)
        for kw in (dict(despeckle=True), dict(despeckle={"rank": 0}, denoise=True), dict()):
            want = fb.filter(k, **kw)
            out = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
            with torch.cuda.stream(s):
                ctx.filter_device(fb, k, out.data_ptr(), stream=s.cuda_stream, **kw)
            s.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), kw
    finally:
        fb.destroy()


def test_every_refusal(ctx):
    """The library's own checks (the Python host checks the parameters first, so these go to the C entry points directly)."""
    import torch

    lib = ctx.lib
    fb = ctx.create_framebuffer(16, 16, moments=True)
    plain = ctx.create_framebuffer(16, 16)
    out = np.zeros((16, 16, 4), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    out8 = np.zeros((16, 16, 4), np.uint8)
    dev = torch.zeros((16 * 16 * 4 + 4,), dtype=torch.float32, device="cuda:0")

    def call(f=fb, samples=1, despeckle=True, denoise=None, stage=None, mode=None, **fields):
        flt = native.filters(despeckle, denoise)
        for name, v in fields.items():
            setattr(flt.despeckle_params, name, v)
        if stage is not None:
            flt.despeckle = stage
        if mode is not None:
            flt.denoise = mode
        return lib.rm_filter(ctx.h, f.h if f is not None else None, samples, C.byref(flt), fp)

    try:
        assert call() == abi.RM_OK
        assert call(denoise=True) == abi.RM_OK and call(denoise="variance") == abi.RM_OK and call(despeckle=None) == abi.RM_OK
        ok = native.filters(True)
        # NULL arguments
        assert call(f=None) == abi.RM_ERR_INVALID
        assert lib.rm_filter(None, fb.h, 1, C.byref(ok), fp) == abi.RM_ERR_INVALID
        assert lib.rm_filter(ctx.h, fb.h, 1, None, fp) == abi.RM_ERR_INVALID
        assert lib.rm_filter(ctx.h, fb.h, 1, C.byref(ok), None) == abi.RM_ERR_INVALID
        assert lib.rm_present_filtered(ctx.h, fb.h, 1, C.byref(ok), None) == abi.RM_ERR_INVALID
        assert lib.rm_present_filtered(ctx.h, fb.h, 1, None, out8.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.RM_ERR_INVALID
        assert lib.rm_present_filtered(ctx.h, fb.h, 1, C.byref(ok), out8.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.RM_OK
        # samples, the stage switches, the despeckle parameters (only when the stage is on)
        assert call(samples=0) == abi.RM_ERR_INVALID
        for stage in (-1, 2):
            assert call(stage=stage) == abi.RM_ERR_INVALID
        for mode in (-1, 3):
            assert call(mode=mode) == abi.RM_ERR_INVALID
        for fields in (dict(radius=0), dict(radius=3), dict(rank=-1), dict(rank=4), dict(gain=0.5), dict(gain=float("nan")), dict(gain=float("inf")),
                       dict(floor=-0.5), dict(floor=float("inf")), dict(reserved=1)):
            assert call(**fields) == abi.RM_ERR_INVALID, fields
            assert call(stage=0, **fields) == abi.RM_OK, fields
        assert call(repair=-7) == abi.RM_OK  # any value: 0 = off
        # everything the selected denoiser refuses
        assert call(denoise="variance", f=plain) == abi.RM_ERR_INVALID  # no moments plane
        assert call(denoise=True, f=plain) == abi.RM_OK
        for block, fields in (("atrous", dict(iterations=9)), ("atrous", dict(sigma_color=0.0)), ("variance", dict(sigma_luminance=float("nan"))),
                              ("variance", dict(reserved=1)), ("variance", dict(iterations=-1))):
            flt = native.filters(True, True if block == "atrous" else "variance")
            for name, v in fields.items():
                setattr(getattr(flt, block), name, v)
            assert lib.rm_filter(ctx.h, fb.h, 1, C.byref(flt), fp) == abi.RM_ERR_INVALID, (block, fields)
            flt.denoise = abi.RM_DENOISE_NONE  # the stage off: its block is not looked at
            assert lib.rm_filter(ctx.h, fb.h, 1, C.byref(flt), fp) == abi.RM_OK, (block, fields)
        # a window, a striped framebuffer, a framebuffer of another context
        window = ctx.create_framebuffer(16, 16, 4, 8)
        assert call(window) == abi.RM_ERR_INVALID
        window.destroy()
        striped = ctx.create_striped_framebuffer(16, 16, 8, 2, 0)
        assert call(striped) == abi.RM_ERR_INVALID
        striped.destroy()
        other = native.Context(0)
        ofb = other.create_framebuffer(16, 16)
        assert call(ofb) == abi.RM_ERR_INVALID
        ofb.destroy()
        other.close()
        # the device output
        assert lib.rm_filter_device(ctx.h, fb.h, 1, C.byref(ok), None, None) == abi.RM_ERR_INVALID
        assert lib.rm_filter_device(ctx.h, fb.h, 1, C.byref(ok), C.c_void_p(dev.data_ptr() + 4), None) == abi.RM_ERR_INVALID
        assert lib.rm_filter_device(ctx.h, fb.h, 1, C.byref(ok), C.c_void_p(dev.data_ptr()), None) == abi.RM_OK
        ctx.sync()
        # despeckle alone takes a colour-only wrapped whole frame; the guided stages do not
        colour = torch.zeros((16, 16, 4), dtype=torch.float32, device="cuda:0")
        colour[..., :3] = 0.5
        colour[7, 9, :3] = 90.0
        wrapped = ctx.wrap_framebuffer(16, 16, 0, 16, colour.data_ptr())
        assert call(wrapped) == abi.RM_OK
        assert D.changed(out, colour.cpu().numpy()).sum() == 1 and np.allclose(out[7, 9, :3], 0.5)
        assert call(wrapped, denoise=True) == abi.RM_ERR_INVALID
        wrapped.destroy()
        # the Python host refuses before the library is asked
        with pytest.raises(ValueError):
            fb.present(1, despeckle={"rank": 9})
        with pytest.raises(native.RmError):
            plain.filter(1, despeckle=True, denoise="variance")
    finally:
        fb.destroy()
        plain.destroy()


# ---- the hosts ----------------------------------------------------------------------------------------------------

def test_job_present_callback_can_despeckle():
    sc, schema = _job()
    c = J.RenderJobContext(0, gbuffer="f16")
    try:
        frames = []
        J.reset_halton()
        assert J.drain(J.do_render_job(schema, c)(J.collect_presents(frames, despeckle=True))) == {"success": True}
        samples, canvas = frames[-1]
        fb = c.fbo_create(64, 32, 1)
        assert np.array_equal(canvas, fb.present(samples, despeckle=True))
        # the filter at its most eager does change this frame, and the capture follows present
        eager = dict(radius=1, rank=0, gain=1.0, floor=0.0)
        assert not np.array_equal(fb.present(samples, despeckle=eager), fb.present(samples))
    finally:
        c.close()


def test_png_capture_follows_present(ctx, tmp_path):
    H, W, k = 20, 28, 2
    planes = list(random_planes(H, W, k, seed=9))
    planes[0] = with_outliers(planes[0], k)
    fb = upload(ctx, planes, "f32")
    try:
        capture.save_png(fb, k, str(tmp_path / "a.png"), despeckle=True)
        capture.save_png(fb, k, str(tmp_path / "b.png"), denoise=True, despeckle={"rank": 0})
        assert np.array_equal(capture.decode_png((tmp_path / "a.png").read_bytes()), fb.present(k, despeckle=True)[::-1])
        assert np.array_equal(capture.decode_png((tmp_path / "b.png").read_bytes()), fb.present(k, denoise=True, despeckle={"rank": 0})[::-1])
    finally:
        fb.destroy()


@pytest.mark.skipif(shutil.which("node") is None or not (JS / "rm_napi.node").exists(), reason="node or the addon is missing")
def test_node_host_gives_the_python_bytes(tmp_path):
    sc, schema = _job()
    eager = dict(radius=1, rank=0, gain=1.0, floor=0.0, repair=1)
    c = J.RenderJobContext(0, gbuffer="f16")
    try:
        frames = []
        J.reset_halton()
        J.drain(J.do_render_job(schema, c)(lambda s, cx, fb, n: frames.append(
            (n, fb.present(n, denoise=True, despeckle=True), fb.filter(n, despeckle=eager), fb.present(n, despeckle=eager),
             fb.filter(n, despeckle=eager, denoise={"iterations": 2}))) if n > 0 else None))
        n, want8, want32, want8e, want32d = frames[-1]
    finally:
        c.close()
    plain = {k: v for k, v in schema.items() if k != "sdfScene"}
    paths = [tmp_path / name for name in ("canvas.rgba", "filtered.f32", "eager.rgba", "chain.f32")]
    script = f"""
const fs = require("fs");
const rm = require({str(JS / "index.js")!r});
(async () => {{
  const schema = Object.assign({json.dumps(plain)}, {{
    sdfScene: new rm.CsgScene().box([0, 0, 0], [1.0, 0.6, 0.8]).subtract().sphere([0.4, 0.3, -0.6], 0.7).smoothUnion(0.3).sphere([-1.2, 0.2, 0.0], 0.5) }});
  const ctx = new rm.RenderJobContext({{ gbuffer: "f16" }});
  const eager = {json.dumps(eager)};
  rm.resetHalton();
  let out = null;
  const gen = (await rm.doRenderJob(schema, ctx))((s, c, fb, n) => {{ if (n > 0) {{
    out = [fb.present(n, {{ denoise: true, despeckle: true }}), fb.filter(n, {{ despeckle: eager }}), fb.present(n, {{ despeckle: eager }}),
           fb.filter(n, {{ despeckle: eager, denoise: {{ iterations: 2 }} }})];
    if (Buffer.compare(Buffer.from(fb.present(n, {{}})), Buffer.from(fb.present(n))) !== 0) throw new Error("present without despeckle");
    if (Buffer.compare(Buffer.from(fb.filter(n).buffer), Buffer.from(fb.download(0).buffer)) !== 0) throw new Error("filter with both stages off");
    if (!fb.toDataURL(n, {{ despeckle: true }}).startsWith("data:image/png;base64,")) throw new Error("toDataURL"); }} }});
  let r = gen.next();
  while (!r.done) r = gen.next();
  if (!r.value.success) throw new Error(JSON.stringify(r.value));
  const paths = {json.dumps([str(p) for p in paths])};
  out.forEach((a, i) => fs.writeFileSync(paths[i], Buffer.from(a.buffer, a.byteOffset, a.byteLength)));
  ctx.close();
  let threw = false;
  try {{ const sh = new rm.ShardedRenderJobContext({{ devices: [0] }}); const sfb = sh.fboCreate(16, 16, 1);
        try {{ sfb.present(1, false, {{ despeckle: true }}); }} catch (e) {{ threw = /sharded/.test(e.message); }} sh.close(); }}
  catch (e) {{ throw e; }}
  if (!threw) throw new Error("the sharded context did not refuse despeckle");
}})().catch((e) => {{ console.error(e); process.exit(1); }});
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(paths[0], np.uint8).reshape(32, 64, 4), want8)
    assert np.array_equal(np.fromfile(paths[1], np.float32).reshape(32, 64, 4).view(np.uint32), want32.view(np.uint32))
    assert np.array_equal(np.fromfile(paths[2], np.uint8).reshape(32, 64, 4), want8e)
    assert np.array_equal(np.fromfile(paths[3], np.float32).reshape(32, 64, 4).view(np.uint32), want32d.view(np.uint32))


# ---- one measurement on the fast build's renders ---------------------------------------------------------------------------

def test_measurement_on_fast_renders(ctx):
    """The CSG scene of the denoisers' quality jobs with glossy surfaces (roughness 0.05, specular 0.6: the direct-light specular
    term reaches 127 x the light colour), 256 x 256, f32, k = 4, 16, 64 against 1024 samples; INTEGRATION.md "Firefly filter" has
    the table this prints.  The one assertion: despeckle + variance is no worse than 1.05 x variance alone on the whole frame --
    against the same frame without the filter, the 5 % being legitimately bright single-pixel highlights the filter may dim.
    Measured on MI355X: that ratio 0.984 / 1.001 / 1.000 at k = 4 / 16 / 64; the filter changed 0.021 % / 0.023 % / 0 of this
    scene's pixels (none was non-finite) and 0.82 % / 0.003 % / 0 of the unmodified Mandelbulb job's."""
    jobs = _quality_jobs()
    sc, schema = jobs["csg_dof"]
    sc.material = S.Material(roughness=0.05, specular=(0.6, 0.6, 0.6))
    h = ctx.create_scene(sc)
    J.reset_halton()
    noise = np.array([J.next_rand_noise() for _ in range(64 + 1024)], np.float32)
    u = J.uniforms_from_schema(schema, (0.5, 0.5))
    lo, hi = ctx.create_framebuffer(256, 256, moments=True), ctx.create_framebuffer(256, 256)
    failures = []
    try:
        for i in range(64, 64 + 1024, 256):
            ctx.render_samples(h, hi, u, noise[i:i + 256], None, abi.RM_RENDER_FAST)
        high = widened(hi)
        ref = R.displayed(high[0], 1024)
        edges = R.edge_mask(high[1], high[2], 1024)
        done = 0
        for k in (4, 16, 64):
            ctx.render_samples(h, lo, u, noise[done:k], None, abi.RM_RENDER_FAST)
            done = k
            c = lo.download(0)
            raw_d = R.displayed(c, k)
            var_d = R.displayed(lo.denoise_variance(k), k)
            both_d = R.displayed(lo.filter(k, despeckle=True, denoise="variance"), k)
            share = float(D.changed(lo.filter(k, despeckle=True), c).mean())
            q = {"raw": R.mse(raw_d, ref), "variance": R.mse(var_d, ref), "despeckle_variance": R.mse(both_d, ref),
                 "raw_edges": R.mse(raw_d, ref, edges), "variance_edges": R.mse(var_d, ref, edges), "despeckle_variance_edges": R.mse(both_d, ref, edges),
                 "changed": share, "non_finite": float((~np.isfinite(c[..., :3]).all(-1)).mean())}
            print("csg_glossy", k, json.dumps({key: round(v, 6) for key, v in q.items()}), "ratio", round(q["despeckle_variance"] / q["variance"], 4))
            if not q["despeckle_variance"] <= 1.05 * q["variance"]:
                failures.append((k, q["despeckle_variance"], q["variance"]))
    finally:
        lo.destroy()
        hi.destroy()
        h.destroy()
    bulb, bschema = jobs["mandelbulb"]
    h = ctx.create_scene(bulb)
    fb = ctx.create_framebuffer(256, 256)
    try:
        ub = J.uniforms_from_schema(bschema, (0.5, 0.5))
        done = 0
        for k in (4, 16, 64):
            ctx.render_samples(h, fb, ub, noise[done:k], None, abi.RM_RENDER_FAST)
            done = k
            c = fb.download(0)
            print("mandelbulb", k, "changed", round(float(D.changed(fb.filter(k, despeckle=True), c).mean()), 6))
    finally:
        fb.destroy()
        h.destroy()
    assert not failures, failures
