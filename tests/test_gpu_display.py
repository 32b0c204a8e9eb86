"""Frame statistics, the linear output and the display transform on the GPU against tests/display_ref.py: the statistics kernel
field by field, the parts of a frame adding up, the chain's statistics, the new float output tied to the pinned present pass, the
three tone operators byte for byte, off-is-off, the device variant, every refusal, the hosts, and one printed measurement."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import display_ref as DR
from raymarching_engine_amd import abi, capture, job as J, native, scene as S
from test_gpu_denoise import _job, _quality_jobs, random_planes, upload
from test_gpu_denoise_variance import random_moments
from test_gpu_despeckle import raw_planes, upload_all, with_outliers

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
JS = ROOT / "raymarching-engine_amd" / "js"
F = np.float32
K = 3  # samples: s = 1.0f / 3 is inexact
# (257, 263): several workgroups; (523, 517): more than 1024 x 256 pixels, so the statistics kernel's grid-stride loop repeats and, with
# 8247 pixels beyond one stride, only some lanes of it take the second load of a pair
SHAPES = [(1, 1), (1, 2), (3, 5), (19, 37), (61, 83), (257, 263), (523, 517)]
EDGES = [F(2.0 ** -20), np.nextafter(F(2.0 ** -20), F(0)), F(1.0), np.nextafter(F(1.0625), F(0)), F(1.0625), F(0.18), np.nextafter(F(4096.0), F(0)), F(4096.0)]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_floats(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def special_colours(k):
    """Colours whose luminance lands in every class and on the bin rule's edges: a NaN, +inf, -inf, negatives, +0, -0, a subnormal,
    the edge values of the CPU test divided by s (grey, so l is the value up to the roundings of the weights), values far above."""
    grey = lambda v: [v, v, v]
    rows = [grey(F(0.5) * k), grey(F(0.0)), grey(F(1e5) * k), [np.nan, 1.0, 1.0], [np.inf, 0.0, 0.0], [-np.inf, 0.0, 0.0], grey(F(-3.0)), [-1.0, 0.5, -2.0],
            grey(F(-0.0)), grey(F(3e-40)), [3e6 * k, 0.0, 0.0], [0.0, -0.0, 9e-7 * k]]
    rows += [grey(F(v) * F(k)) for v in EDGES]
    return np.array(rows, F)


def stats_frame(H, W, k, seed):
    """random_planes' colour with the special colours scattered over it (as many as fit) and a constant 16 x 64 block."""
    c = random_planes(H, W, k, seed)[0]
    if H >= 24 and W >= 70:
        c[5:21, 3:67, :3] = np.array([0.9, 0.2, 0.4], F) * k  # every lane of a wave in one bin
    sp = special_colours(k)
    flat = c.reshape(-1, 4)
    step = max(1, (H * W) // (len(sp) + 1))
    for i, colour in enumerate(sp):
        if i * step < H * W:
            flat[(i * step + (7 if H * W > 64 else 0)) % (H * W), :3] = colour
    return c


def colour_only(ctx, c, **kw):
    fb = ctx.create_framebuffer(c.shape[1], c.shape[0], **kw)
    fb.upload(0, c)
    return fb


def assert_stats_equal(got, want, what=""):
    """A native.FrameStats against display_ref's dict, every field exactly (min / max bit for bit)."""
    for name in ("pixels", "below", "above", "non_finite"):
        assert getattr(got, name) == want[name], (what, name, getattr(got, name), want[name])
    assert np.array_equal(got.hist, want["hist"]), (what, np.flatnonzero(got.hist != want["hist"])[:8].tolist())
    assert bits(F(got.raw.min_l)) == bits(want["min_l"]) and bits(F(got.raw.max_l)) == bits(want["max_l"]), (what, got.min, got.max, want["min_l"], want["max_l"])
    assert got.pixels == got.below + got.above + got.non_finite + int(got.hist.sum())


# ---- statistics -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_match_the_restatement(ctx, shape):
    H, W = shape
    for what, c in (("random", stats_frame(H, W, K, seed=H * W + 3)), ("constant", np.full((H, W, 4), F(0.7) * K, F))):
        fb = colour_only(ctx, c)
        try:
            got, want = fb.stats(K), DR.stats(c, K)
            print(shape, what, "below", got.below, "above", got.above, "non-finite", got.non_finite, "binned", int(got.hist.sum()), "bins used",
                  int((got.hist > 0).sum()), "min", got.min, "max", got.max)
            assert_stats_equal(got, want, (shape, what))
            if what == "random" and H * W > 400:  # each of the four classes is there
                assert got.below > 0 and got.above > 0 and got.non_finite > 0 and got.hist.sum() > 0 and (got.hist > 0).sum() > 16
            if what == "constant":
                assert (got.hist > 0).sum() == 1 and got.hist.max() == H * W and got.min == got.max
        finally:
            fb.destroy()


def test_no_finite_pixel_and_other_sample_counts(ctx):
    c = np.full((5, 9, 4), np.nan, F)
    c[2, :, 0] = np.inf
    fb = colour_only(ctx, c)
    try:
        got = fb.stats(1)
        assert (got.non_finite, got.pixels, int(got.hist.sum())) == (45, 45, 0) and got.min == float("inf") and got.max == -float("inf")
        assert got.percentile(0.5) == 0.0 and got.exposure() == 1.0
    finally:
        fb.destroy()
    c = stats_frame(33, 47, 7, seed=4)
    fb = colour_only(ctx, c)
    try:
        for k in (1, 7, 64):
            assert_stats_equal(fb.stats(k), DR.stats(c, k), k)
    finally:
        fb.destroy()


def test_parts_add_up_to_the_whole_frame(ctx):
    H, W = 61, 83
    c = stats_frame(H, W, K, seed=12)
    whole = colour_only(ctx, c)
    try:
        want = whole.stats(K)
        assert_stats_equal(want, DR.stats(c, K))
        for parts in (2, 3):
            total = native.FrameStats()
            for part in range(parts):
                rows = [r for r in range(H) if (r // 8) % parts == part]
                fb = ctx.create_striped_framebuffer(W, H, 8, parts, part)
                assert fb.row_count == len(rows)
                fb.upload(0, c[rows])
                st = fb.stats(K)
                assert_stats_equal(st, DR.stats(c[rows], K), (parts, part))
                total = total + st
                fb.destroy()
            assert bytes(total.raw) == bytes(want.raw), parts
        total = native.FrameStats()
        for begin, count in ((0, 23), (23, H - 23)):  # two windows
            fb = ctx.create_framebuffer(W, H, begin, count)
            fb.upload(0, c[begin:begin + count])
            total = total + fb.stats(K)
            fb.destroy()
        assert bytes(total.raw) == bytes(want.raw)
        # a wrapped colour-only frame
        import torch

        t = torch.from_numpy(c).to("cuda:0")
        wrapped = ctx.wrap_framebuffer(W, H, 0, H, t.data_ptr())
        assert bytes(wrapped.stats(K).raw) == bytes(want.raw)
        wrapped.destroy()
    finally:
        whole.destroy()


def test_statistics_of_the_chain_are_those_of_its_result(ctx):
    H, W, k = 61, 83, 4
    planes = list(random_planes(H, W, k, seed=7))
    planes[0] = with_outliers(planes[0], k)
    fb = upload_all(ctx, planes, random_moments(H, W, k, seed=8), "f32")
    other = ctx.create_framebuffer(W, H)
    try:
        before = raw_planes(fb)
        plain = fb.stats(k)
        for kw in (dict(despeckle=True), dict(despeckle={"radius": 1, "rank": 0, "gain": 1.5, "floor": 0.0}, denoise={"iterations": 2}), dict(denoise="variance"),
                   dict(denoise={"iterations": 0})):
            filtered = fb.filter(k, **kw)
            other.upload(0, filtered)
            got = fb.stats(k, **kw)
            assert bytes(got.raw) == bytes(other.stats(k).raw), kw
            assert_stats_equal(got, DR.stats(filtered, k), kw)
        assert bytes(fb.stats(k, denoise={"iterations": 0}).raw) == bytes(plain.raw)
        assert bytes(fb.stats(k, despeckle=True).raw) != bytes(plain.raw)  # the fireflies are gone from the numbers
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, raw_planes(fb)))
    finally:
        fb.destroy()
        other.destroy()


# ---- the linear output and the display bytes ------------------------------------------------------------------------------------

def display_planes(H, W, k, seed):
    """The chain test's planes (DoF radius rising from 0 at column 0, so the blur is on) with, in column 0 where a pixel is its own
    single tap, channels that are zero, negative, NaN, +inf and above 2^20 after the 1 / k."""
    planes = list(random_planes(H, W, k, seed=seed))
    planes[0] = with_outliers(planes[0], k)
    planes[1][..., 3] = np.linspace(0.0, 0.2, W, dtype=F) * k
    col = planes[0][:, 0, :3]
    col[2] = [0.0, -0.0, 0.25 * k]
    col[4] = [-1.5 * k, 0.5 * k, -1e-3 * k]
    col[6] = [np.nan, 1.0 * k, 2.0 * k]
    col[8] = [np.inf, 3.0 * k, 0.1 * k]
    col[10] = [4e6 * k, 2.5e6 * k, 1.0 * k]
    col[12] = [1e30, 0.7 * k, 3e38]
    col[14] = [0.18 * k, 1.0 * k, 4.0 * k]
    return planes


@pytest.mark.parametrize("gl_stack", [False, True])
@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_linear_output_and_display_bytes(ctx, gbuffer, gl_stack):
    H, W, k = 61, 83, 4
    fb = upload_all(ctx, display_planes(H, W, k, seed=7), random_moments(H, W, k, seed=8), gbuffer)
    ctx.set_gl_stack(gl_stack)
    try:
        before = raw_planes(fb)
        lin = fb.linear(k)
        rgb = lin[..., :3]
        assert np.array_equal(lin[..., 3], np.ones((H, W), F))
        with np.errstate(invalid="ignore"):
            present = dict(zero=(rgb == 0).any(), negative=(rgb < 0).any(), nan=np.isnan(rgb).any(), inf=np.isposinf(rgb).any(), huge=(np.isfinite(rgb) & (rgb > 2.0 ** 20)).any())
        assert all(present.values()), present
        # the new float output is what the pinned pass holds in front of its pow, blur included
        assert np.array_equal(fb.present(k), DR.display_bytes(lin, "clip", gl_stack=gl_stack))
        for g in (0.37, 2.0, 11.5):
            lg = fb.linear(k, display={"gain": g, "tone": "aces"})  # the tone is checked, not applied
            assert same_floats(lg[..., :3], DR.expose(rgb, g)), g
            assert np.array_equal(lg[..., 3], np.ones((H, W), F))
            for tone, white in (("clip", 4.0), ("reinhard", 4.0), ("reinhard", 0.75), ("aces", 4.0)):
                got = fb.present(k, display={"gain": g, "tone": tone, "white": white})
                want = DR.display_bytes(lg, tone, white, gl_stack=gl_stack)
                assert np.array_equal(got, want), (g, tone, white, np.argwhere(got != want)[:6].tolist())
        assert not np.array_equal(fb.present(k, display={"tone": "reinhard"}), fb.present(k, display={"tone": "aces"}))
        # the chain feeds it as it feeds rm_present_filtered
        for kw in (dict(despeckle=True), dict(despeckle={"rank": 0}, denoise=True), dict(denoise="variance")):
            assert np.array_equal(fb.present(k, display={}, **kw), fb.present(k, **kw)), kw
            lf = fb.linear(k, display={"gain": 2.0}, **kw)
            assert np.array_equal(fb.present(k, display={"gain": 2.0, "tone": "aces"}, **kw), DR.display_bytes(lf, "aces", gl_stack=gl_stack)), kw
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, raw_planes(fb)))
    finally:
        ctx.set_gl_stack(False)
        fb.destroy()


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 5), (19, 37), (257, 263)])
def test_small_frames(ctx, shape):
    H, W = shape
    planes = list(random_planes(H, W, K, seed=H * W + 5))
    planes[1][..., 3] = 0.03 * K
    fb = upload(ctx, planes, "f32")
    try:
        lin = fb.linear(K, display={"gain": 1.7})
        assert np.array_equal(fb.present(K), DR.display_bytes(fb.linear(K), "clip"))
        for tone in ("reinhard", "aces"):
            assert np.array_equal(fb.present(K, display={"gain": 1.7, "tone": tone, "white": 2.0}), DR.display_bytes(lin, tone, 2.0))
    finally:
        fb.destroy()


# ---- off is off, the device variant ------------------------------------------------------------------------------------------

def test_off_is_off(ctx):
    H, W, k = 33, 47, 2
    planes = list(random_planes(H, W, k, seed=5))
    planes[0] = with_outliers(planes[0], k)
    planes[1][..., 3] = 0.05 * k
    fb = upload(ctx, planes, "f32")
    try:
        before = raw_planes(fb)
        plain = fb.present(k)
        assert np.array_equal(fb.present(k, display=None), plain)
        out = np.empty((H, W, 4), np.uint8)
        p8 = out.ctypes.data_as(C.POINTER(C.c_uint8))
        d = abi.RmDisplay()
        ctx.lib.rm_display_default(C.byref(d))
        for f in (None, native.filters()):  # NULL filters = both stages off; with the default filters: rm_present's bytes
            for disp in (None, d):
                out[:] = 7
                ctx._check(ctx.lib.rm_present_display(ctx.h, fb.h, k, C.byref(f) if f is not None else None, C.byref(disp) if disp is not None else None, p8))
                assert np.array_equal(out, plain)
        for kw in (dict(despeckle=True), dict(denoise=True), dict(despeckle=True, denoise={"iterations": 2})):
            assert np.array_equal(fb.present(k, display={}, **kw), fb.present(k, **kw)), kw  # rm_present_filtered's bytes
        assert not np.array_equal(fb.present(k, display={"gain": 2.0}), plain)
        fb.linear(k, despeckle=True, denoise=True)
        fb.stats(k, despeckle=True)
        fb.present(k, display="auto")
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, raw_planes(fb)))
    finally:
        fb.destroy()


def test_auto_is_the_gain_of_the_same_chains_statistics(ctx):
    H, W, k = 40, 56, 4
    planes = list(random_planes(H, W, k, seed=21))
    planes[0] = with_outliers(planes[0], k)
    planes[0][..., :3] *= F(0.05)  # a dark frame: the gain is well above 1
    fb = upload(ctx, planes, "f32")
    try:
        g = fb.stats(k).exposure()
        assert 1.5 < g < 1024.0
        assert np.array_equal(fb.present(k, display="auto"), fb.present(k, display={"gain": g}))
        assert fb.display_block(k, display="auto").gain == float(F(g))
        gd = fb.stats(k, despeckle=True).exposure(key=0.3, low=0.2)
        assert np.array_equal(fb.present(k, despeckle=True, display={"auto": {"key": 0.3, "low": 0.2}, "tone": "aces"}),
                              fb.present(k, despeckle=True, display={"gain": gd, "tone": "aces"}))
        assert same_floats(fb.linear(k, display="auto"), fb.linear(k, display={"gain": g}))
        with pytest.raises(ValueError):
            fb.present(k, display={"auto": True, "gain": 2.0})
        with pytest.raises(ValueError):
            fb.present(k, display={"auto": {"low": 0.9, "high": 0.1}})
    finally:
        fb.destroy()


def test_device_variant_on_a_callers_stream(ctx):
    import torch

    H, W, k = 97, 131, 2
    planes = list(random_planes(H, W, k, seed=3))
    planes[0] = with_outliers(planes[0], k)
    planes[1][..., 3] = 0.04 * k
    fb = upload(ctx, planes, "f16")
    try:
        s = torch.cuda.Stream(device=0)
        for kw in (dict(), dict(display={"gain": 1.5, "tone": "reinhard"}), dict(despeckle=True, display={"tone": "aces"}),
                   dict(despeckle={"rank": 0}, denoise=True, display="auto")):
            want = fb.present(k, **kw) if "display" in kw else fb.present(k)
            out = torch.full((H, W, 4), 9, dtype=torch.uint8, device="cuda:0")
            with torch.cuda.stream(s):
                ctx.present_display_device(fb, k, out.data_ptr(), stream=s.cuda_stream, **kw)
            s.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), kw
    finally:
        fb.destroy()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_every_refusal(ctx):
    """The library's own checks (the Python host checks the blocks first, so these go to the C entry points directly)."""
    import torch

    lib = ctx.lib
    fb = ctx.create_framebuffer(16, 16, moments=True)
    plain = ctx.create_framebuffer(16, 16)
    out8 = np.zeros((16, 16, 4), np.uint8)
    p8 = out8.ctypes.data_as(C.POINTER(C.c_uint8))
    out32 = np.zeros((16, 16, 4), F)
    p32 = out32.ctypes.data_as(C.POINTER(C.c_float))
    dev = torch.zeros((16 * 16 * 4 + 8,), dtype=torch.uint8, device="cuda:0")
    st = abi.RmFrameStats()
    INVALID, OK = abi.RM_ERR_INVALID, abi.RM_OK

    def ref(x):
        return C.byref(x) if x is not None else None

    def calls(f=None, d=None, frame=fb, samples=1, context=ctx):
        """The three display entries with the same arguments: their return codes."""
        fh = frame.h if frame is not None else None
        ch = context.h if context is not None else None
        return [lib.rm_present_display(ch, fh, samples, ref(f), ref(d), p8), lib.rm_present_linear(ch, fh, samples, ref(f), ref(d), p32),
                lib.rm_present_display_device(ch, fh, samples, ref(f), ref(d), C.c_void_p(dev.data_ptr()), None)]

    def display(**fields):
        d = abi.RmDisplay()
        lib.rm_display_default(C.byref(d))
        for name, v in fields.items():
            setattr(d, name, v)
        return d

    try:
        assert calls() == [OK] * 3 and calls(native.filters(True, True), display(gain=2.0, tone=abi.RM_TONE_REINHARD)) == [OK] * 3
        # the display block
        for fields in (dict(gain=0.0), dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(tone=-1), dict(tone=3), dict(reserved=1),
                       dict(tone=abi.RM_TONE_REINHARD, white=0.0), dict(tone=abi.RM_TONE_REINHARD, white=-1.0), dict(tone=abi.RM_TONE_REINHARD, white=float("nan")),
                       dict(tone=abi.RM_TONE_REINHARD, white=float("inf"))):
            assert calls(d=display(**fields)) == [INVALID] * 3, fields
        for tone in (abi.RM_TONE_CLIP, abi.RM_TONE_ACES):  # white is the Reinhard operator's: not looked at for the others
            for white in (0.0, -1.0, float("nan"), float("inf")):
                assert calls(d=display(tone=tone, white=white)) == [OK] * 3, (tone, white)
        # handles, samples
        assert calls(frame=None) == [INVALID] * 3 and calls(context=None) == [INVALID] * 3 and calls(samples=0) == [INVALID] * 3
        # everything rm_present_filtered refuses; a stage that is off is not looked at
        for stage in (-1, 2):
            f = native.filters()
            f.despeckle = stage
            assert calls(f) == [INVALID] * 3
        for mode in (-1, 3):
            f = native.filters()
            f.denoise = mode
            assert calls(f) == [INVALID] * 3
        for fields in (dict(radius=0), dict(rank=4), dict(gain=0.5), dict(floor=-0.5), dict(reserved=1)):
            f = native.filters(True)
            for name, v in fields.items():
                setattr(f.despeckle_params, name, v)
            assert calls(f) == [INVALID] * 3, fields
            assert lib.rm_frame_stats(ctx.h, fb.h, 1, C.byref(f), C.byref(st)) == INVALID, fields
            f.despeckle = 0
            assert calls(f) == [OK] * 3, fields
            assert lib.rm_frame_stats(ctx.h, fb.h, 1, C.byref(f), C.byref(st)) == OK, fields
        for block, fields in (("atrous", dict(iterations=9)), ("atrous", dict(sigma_color=0.0)), ("variance", dict(sigma_luminance=float("nan"))),
                              ("variance", dict(reserved=1))):
            f = native.filters(None, True if block == "atrous" else "variance")
            for name, v in fields.items():
                setattr(getattr(f, block), name, v)
            assert calls(f) == [INVALID] * 3, (block, fields)
            assert lib.rm_frame_stats(ctx.h, fb.h, 1, C.byref(f), C.byref(st)) == INVALID, (block, fields)
            f.denoise = abi.RM_DENOISE_NONE
            assert calls(f) == [OK] * 3, (block, fields)
        assert calls(native.filters(None, "variance"), frame=plain) == [INVALID] * 3  # no moments plane
        assert lib.rm_frame_stats(ctx.h, plain.h, 1, C.byref(native.filters(None, "variance")), C.byref(st)) == INVALID
        # a window, a striped framebuffer: the display entries and the chain's statistics need the whole frame, the plain statistics do not
        window = ctx.create_framebuffer(16, 16, 4, 8)
        striped = ctx.create_striped_framebuffer(16, 16, 8, 2, 0)
        for part in (window, striped):
            assert calls(frame=part) == [INVALID] * 3
            assert lib.rm_frame_stats(ctx.h, part.h, 1, C.byref(native.filters(True)), C.byref(st)) == INVALID
            assert lib.rm_frame_stats(ctx.h, part.h, 1, None, C.byref(st)) == OK and st.pixels == 8 * 16
            part.destroy()
        # a framebuffer of another context
        other = native.Context(0)
        ofb = other.create_framebuffer(16, 16)
        assert calls(frame=ofb) == [INVALID] * 3
        assert lib.rm_frame_stats(ctx.h, ofb.h, 1, None, C.byref(st)) == INVALID
        ofb.destroy()
        other.close()
        # the outputs
        d = display()
        assert lib.rm_present_display(ctx.h, fb.h, 1, None, C.byref(d), None) == INVALID
        assert lib.rm_present_linear(ctx.h, fb.h, 1, None, C.byref(d), None) == INVALID
        assert lib.rm_present_display_device(ctx.h, fb.h, 1, None, C.byref(d), None, None) == INVALID
        for off in (1, 2, 3):
            assert lib.rm_present_display_device(ctx.h, fb.h, 1, None, C.byref(d), C.c_void_p(dev.data_ptr() + off), None) == INVALID
        assert lib.rm_present_display_device(ctx.h, fb.h, 1, None, C.byref(d), C.c_void_p(dev.data_ptr() + 4), None) == OK
        ctx.sync()
        # the statistics' own arguments
        assert lib.rm_frame_stats(ctx.h, fb.h, 1, None, C.byref(st)) == OK and st.pixels == 256
        assert lib.rm_frame_stats(ctx.h, fb.h, 0, None, C.byref(st)) == INVALID
        assert lib.rm_frame_stats(ctx.h, fb.h, 1, None, None) == INVALID
        assert lib.rm_frame_stats(ctx.h, None, 1, None, C.byref(st)) == INVALID
        assert lib.rm_frame_stats(None, fb.h, 1, None, C.byref(st)) == INVALID
        assert lib.rm_frame_stats(ctx.h, fb.h, 1, C.byref(native.filters(True)), None) == INVALID
        # the Python host refuses before the library is asked
        with pytest.raises(ValueError):
            fb.present(1, display={"gain": -1.0})
        with pytest.raises(ValueError):
            fb.linear(1, display={"tone": "filmic"})
        with pytest.raises(native.RmError):
            plain.present(1, denoise="variance", display={})
    finally:
        fb.destroy()
        plain.destroy()


# ---- the hosts ------------------------------------------------------------------------------------------------------------------

def test_job_present_callback_and_png_capture_follow_present(tmp_path):
    sc, schema = _job()
    c = J.RenderJobContext(0, gbuffer="f16")
    try:
        frames = []
        J.reset_halton()
        assert J.drain(J.do_render_job(schema, c)(J.collect_presents(frames, display="auto"))) == {"success": True}
        samples, canvas = frames[-1]
        fb = c.fbo_create(64, 32, 1)
        assert np.array_equal(canvas, fb.present(samples, display="auto"))
        assert not np.array_equal(canvas, fb.present(samples))
        capture.save_png(fb, samples, str(tmp_path / "a.png"), display="auto")
        capture.save_png(fb, samples, str(tmp_path / "b.png"), despeckle=True, display={"auto": True, "tone": "reinhard", "white": 2.0})
        assert np.array_equal(capture.decode_png((tmp_path / "a.png").read_bytes()), canvas[::-1])
        assert np.array_equal(capture.decode_png((tmp_path / "b.png").read_bytes()),
                              fb.present(samples, despeckle=True, display={"auto": True, "tone": "reinhard", "white": 2.0})[::-1])
    finally:
        c.close()


@pytest.mark.skipif(shutil.which("node") is None or not (JS / "rm_napi.node").exists(), reason="node or the addon is missing")
def test_node_host_gives_the_python_bytes(tmp_path):
    sc, schema = _job()
    disp = {"gain": 1.7, "tone": "reinhard", "white": 3.0}
    c = J.RenderJobContext(0, gbuffer="f16")
    try:
        frames = []
        J.reset_halton()
        J.drain(J.do_render_job(schema, c)(lambda s, cx, fb, n: frames.append(
            (n, fb.present(n, display=disp), fb.present(n, despeckle=True, display="auto"), fb.linear(n, display={"gain": 0.5}), fb.stats(n),
             fb.stats(n, despeckle=True), fb.present(n, display={"auto": {"key": 0.3}, "tone": "aces"}))) if n > 0 else None))
        n, want_disp, want_auto, want_lin, want_stats, want_stats_d, want_aces = frames[-1]
    finally:
        c.close()
    plain = {k: v for k, v in schema.items() if k != "sdfScene"}
    paths = [tmp_path / name for name in ("disp.rgba", "auto.rgba", "lin.f32", "aces.rgba", "stats.json")]
    script = f"""
const fs = require("fs");
const rm = require({str(JS / "index.js")!r});
(async () => {{
  const schema = Object.assign({json.dumps(plain)}, {{
    sdfScene: new rm.CsgScene().box([0, 0, 0], [1.0, 0.6, 0.8]).subtract().sphere([0.4, 0.3, -0.6], 0.7).smoothUnion(0.3).sphere([-1.2, 0.2, 0.0], 0.5) }});
  const ctx = new rm.RenderJobContext({{ gbuffer: "f16" }});
  rm.resetHalton();
  let out = null, stats = null;
  const flat = (s) => ({{ pixels: s.pixels, below: s.below, above: s.above, nonFinite: s.nonFinite, min: s.min, max: s.max, hist: Array.from(s.hist) }});
  const gen = (await rm.doRenderJob(schema, ctx))((s, c, fb, n) => {{ if (n > 0) {{
    out = [fb.present(n, {{ display: {json.dumps(disp)} }}), fb.present(n, {{ despeckle: true, display: "auto" }}), fb.linear(n, {{ display: {{ gain: 0.5 }} }}),
           fb.present(n, {{ display: {{ auto: {{ key: 0.3 }}, tone: "aces" }} }})];
    const st = fb.stats(n), sd = fb.stats(n, {{ despeckle: true }});
    stats = {{ plain: flat(st), despeckled: flat(sd), exposure: rm.statsExposure(st), exposureKey: rm.statsExposure(st, {{ key: 0.3 }}), median: rm.statsPercentile(st, 0.5) }};
    if (Buffer.compare(Buffer.from(fb.present(n, {{ display: {{}} }})), Buffer.from(fb.present(n))) !== 0) throw new Error("the default display");
    if (!fb.toDataURL(n, {{ display: "auto" }}).startsWith("data:image/png;base64,")) throw new Error("toDataURL");
    for (const bad of [{{ gain: 0 }}, {{ tone: "filmic" }}, {{ tone: "reinhard", white: -1 }}, {{ exposure: 1 }}, "reinhard", 3]) {{
      let threw = false;
      try {{ fb.present(n, {{ display: bad }}); }} catch (e) {{ threw = true; }}
      if (!threw) throw new Error("display " + JSON.stringify(bad) + " was not refused");
    }} }} }});
  let r = gen.next();
  while (!r.done) r = gen.next();
  if (!r.value.success) throw new Error(JSON.stringify(r.value));
  const paths = {json.dumps([str(p) for p in paths])};
  out.forEach((a, i) => fs.writeFileSync(paths[i], Buffer.from(a.buffer, a.byteOffset, a.byteLength)));
  fs.writeFileSync(paths[4], JSON.stringify(stats));
  ctx.close();
  let threw = false;
  const sh = new rm.ShardedRenderJobContext({{ devices: [0] }}); const sfb = sh.fboCreate(16, 16, 1);
  try {{ sfb.present(1, false, {{ display: "auto" }}); }} catch (e) {{ threw = /sharded/.test(e.message); }}
  sh.close();
  if (!threw) throw new Error("the sharded context did not refuse display");
}})().catch((e) => {{ console.error(e); process.exit(1); }});
"""
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(paths[0], np.uint8).reshape(32, 64, 4), want_disp)
    assert np.array_equal(np.fromfile(paths[1], np.uint8).reshape(32, 64, 4), want_auto)
    assert same_floats(np.fromfile(paths[2], F).reshape(32, 64, 4), want_lin)
    assert np.array_equal(np.fromfile(paths[3], np.uint8).reshape(32, 64, 4), want_aces)
    got = json.loads(paths[4].read_text())
    for name, want in (("plain", want_stats), ("despeckled", want_stats_d)):
        g = got[name]
        assert (g["pixels"], g["below"], g["above"], g["nonFinite"]) == (want.pixels, want.below, want.above, want.non_finite), name
        assert g["min"] == want.min and g["max"] == want.max and g["hist"] == want.hist.tolist(), name
    assert got["exposure"] == want_stats.exposure() and got["exposureKey"] == want_stats.exposure(key=0.3) and got["median"] == want_stats.percentile(0.5)


# ---- one printed measurement ---------------------------------------------------------------------------------------------------

def test_statistics_kernel_is_not_slower_than_present_rows():
    """3840 x 2160, a rendered Mandelbulb frame and a constant one.  First the statistics of both against the restatement, every
    field exactly: the size every real frame has, where each lane loops over 32 pixels.  Then the median of 20 timings of
    rm_frame_stats beside rm_present_rows on the same frame, each timing 8 calls in a row between two device events on the
    context's stream, every call waited for (rm_frame_stats is synchronous; rm_present_rows is followed by rm_sync), so both carry
    the same host round trip and a stall of the shared host weighs an eighth.  The statistics kernel reads the same 133 MB,
    writes none and computes no pow: it must not be slower on either frame (if it is, the histogram is contended).
    rm_present_display per operator is printed beside rm_present; profiles/display_transform.txt keeps what this printed."""
    import torch

    W, H, k = 3840, 2160, 2
    ctx = native.Context(0)
    stream = torch.cuda.Stream(device=0)
    ctx.set_stream(stream.cuda_stream)
    bulb, schema = _quality_jobs()["mandelbulb"]
    schema = J.make_schema(bulb, W, H, counts=(64, 16), render_mode="full", position=(0, 0, -2.5), lights=[J.point_light((2.0, 3.0, -4.0))])
    scene = ctx.create_scene(bulb)
    fb = ctx.create_framebuffer(W, H)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")

    def median_ms(call, n=20, reps=8):
        times = []
        with torch.cuda.stream(stream):
            for _ in range(3):
                call()
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    call()
                e1.record(stream)
                e1.synchronize()
                times.append(e0.elapsed_time(e1) / reps)
        return sorted(times)[n // 2]

    def rows():
        ctx.present_rows(fb, k, out.data_ptr())
        ctx.sync()

    try:
        J.reset_halton()
        noise = np.array([J.next_rand_noise() for _ in range(k)], F)
        ctx.render_samples(scene, fb, J.uniforms_from_schema(schema, (0.5, 0.5)), noise, None, abi.RM_RENDER_FAST)
        ctx.sync()
        floor_ms = W * H * 16 / 6.3e12 * 1e3  # the colour plane once at the 6.3 TB/s a float4 copy reaches
        print(f"\nframe {W} x {H}: {W * H * 16 / 1e6:.1f} MB of colour plane; HBM floor at 6.3 TB/s {floor_ms:.4f} ms")
        failures = []
        for what in ("mandelbulb", "constant"):
            if what == "constant":
                fb.upload(0, np.full((H, W, 4), F(0.7) * k, F))
            st = fb.stats(k)
            assert_stats_equal(st, DR.stats(fb.download(0), k), what)
            if what == "constant":
                assert st.hist.max() == W * H
            t_stats, t_rows = median_ms(lambda: fb.stats(k)), median_ms(rows)
            print(f"{what}: rm_frame_stats {t_stats:.4f} ms, rm_present_rows {t_rows:.4f} ms (median of 20 timings of 8 calls); bins used {int((st.hist > 0).sum())}, "
                  f"below {st.below}, above {st.above}, non-finite {st.non_finite}")
            if not t_stats <= t_rows:
                failures.append((what, t_stats, t_rows))
        t_present = median_ms(lambda: fb.present(k), 5, 1)
        print(f"rm_present (host canvas included) {t_present:.3f} ms")
        for tone in ("clip", "reinhard", "aces"):
            print(f"rm_present_display {tone} {median_ms(lambda: fb.present(k, display={'gain': 1.5, 'tone': tone}), 5, 1):.3f} ms")
        dev = median_ms(lambda: (ctx.present_display_device(fb, k, out.data_ptr(), display={"gain": 1.5, "tone": "aces"}), ctx.sync()))
        print(f"rm_present_display_device aces {dev:.4f} ms, rm_present_rows {median_ms(rows):.4f} ms")
        assert not failures, failures
    finally:
        ctx.set_stream(None)
        fb.destroy()
        scene.destroy()
        ctx.close()
