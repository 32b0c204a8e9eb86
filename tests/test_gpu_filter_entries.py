"""The nine frame-filter entry points on the MI355X as one family (rm_denoise*, rm_denoise_variance*, rm_filter*): the code AND
the text of every refusal with a real context, one fault at a time, and the context's scratch buffers growing and shrinking
across frame sizes while work is queued on a caller's stream."""
import ctypes as C

import numpy as np
import pytest

from raymarching_engine_amd import abi, native
from test_filter_entries_cpu import CHAIN_FAULTS, ENTRIES
from test_gpu_denoise import random_planes
from test_gpu_denoise_variance import random_moments, upload_var

pytestmark = pytest.mark.gpu

WHOLE_FRAME = "the filter reads neighbouring rows, so it needs a framebuffer holding the whole frame"
NO_GUIDES = "the framebuffer has no G-buffer planes to guide the filter"
NO_MOMENTS = "the framebuffer has no moments plane (create it with RM_FB_MOMENTS)"
DEVICE_OUT = "the output must be a 16-byte aligned device buffer"
ITERATIONS = "iterations must be in 0..8"
SIGMA = "every sigma must be finite and > 0"
ATROUS_FAULTS = [("iterations", -1, ITERATIONS), ("iterations", 9, ITERATIONS), ("sigma_color", 0.0, SIGMA), ("sigma_color", float("inf"), SIGMA),
                 ("sigma_normal", -1.0, SIGMA), ("sigma_depth", float("nan"), SIGMA)]
VARIANCE_FAULTS = [("iterations", -1, ITERATIONS), ("iterations", 9, ITERATIONS), ("sigma_luminance", 0.0, SIGMA),
                   ("sigma_luminance", float("inf"), SIGMA), ("sigma_luminance", float("nan"), SIGMA), ("sigma_normal", -1.0, SIGMA),
                   ("sigma_depth", float("nan"), SIGMA), ("reserved", 1, "reserved must be 0")]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_refusal_by_code_and_text(name):
    import torch

    family, ending = ENTRIES[name]
    ctx, other = native.Context(0), native.Context(0)
    lib = ctx.lib
    fn = getattr(lib, name)
    W = H = 16
    fb = ctx.create_framebuffer(W, H, moments=True)
    plain = ctx.create_framebuffer(W, H)
    window = ctx.create_framebuffer(W, H, 4, 8, moments=True)
    striped = ctx.create_striped_framebuffer(W, H, 8, 2, 0)
    foreign = other.create_framebuffer(W, H, moments=True)
    colour = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    wrapped = ctx.wrap_framebuffer(W, H, 0, H, colour.data_ptr())
    host = np.zeros((H, W, 4), np.float32)
    host8 = np.zeros((H, W, 4), np.uint8)
    dev = torch.zeros((H * W * 4 + 4,), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    good_out = {"host": host.ctypes.data_as(C.POINTER(C.c_float)), "device": C.c_void_p(dev.data_ptr()),
                "rgba8": host8.ctypes.data_as(C.POINTER(C.c_uint8))}[ending]

    def block(den=None, desp=True, **fields):
        """The entry point's parameter block with `fields` set afterwards, unchecked.  The chain (stages `desp` and `den` as
        native.filters takes them): a field of the chain itself, else of the block of the denoiser `den` selects, else of the
        despeckle block."""
        if family == "atrous":
            return abi.RmDenoise(**{**abi.DENOISE_DEFAULTS, **fields})
        if family == "variance":
            return abi.RmDenoiseVariance(**{**abi.DENOISE_VARIANCE_DEFAULTS, **fields})
        f = native.filters(desp, den)
        stage = f.despeckle_params if den is None else f.atrous if den is True else f.variance
        for k, v in fields.items():
            setattr(f if k in ("despeckle", "denoise") else stage, k, v)
        return f

    def call(c=ctx, f=fb, samples=1, b=None, out=good_out, null_block=False):
        """(code, text): one call with the sentinel texts laid down first, so that the text read back is this call's."""
        b = block() if b is None else b
        lib.rm_ctx_create(0, None)
        assert lib.rm_ctx_set_retire_eps(ctx.h, -1.0) == abi.RM_ERR_INVALID
        args = [c.h if c is not None else None, f.h if f is not None else None, samples, None if null_block else C.byref(b), out]
        rc = fn(*args, None) if ending == "device" else fn(*args)
        return rc, lib.rm_last_error(c.h if c is not None else None).decode()

    def refused(text, **kw):
        assert call(**kw) == (abi.RM_ERR_INVALID, f"{name}: {text}"), kw

    try:
        assert call()[0] == abi.RM_OK
        # the handles
        refused("NULL argument", c=None)
        refused("NULL argument", f=None)
        refused("framebuffer belongs to another context", f=foreign)
        refused(WHOLE_FRAME, f=window)
        # samples
        refused("samples must be >= 1", samples=0)
        refused("samples must be >= 1", samples=-3)
        # the output
        if ending == "device":
            refused(DEVICE_OUT, out=None)
            refused(DEVICE_OUT, out=C.c_void_p(dev.data_ptr() + 4))
        else:
            refused("NULL argument", out=None)
        # the parameter block and what the selected filter needs of the framebuffer
        if family == "atrous":
            assert call(null_block=True)[0] == abi.RM_OK  # NULL = the defaults
            assert call(f=plain)[0] == abi.RM_OK
            refused(WHOLE_FRAME, f=striped)
            refused(NO_GUIDES, f=wrapped)
            for field, value, text in ATROUS_FAULTS:
                refused(text, b=block(**{field: value}))
        elif family == "variance":
            assert call(null_block=True)[0] == abi.RM_OK
            refused(NO_MOMENTS, f=plain)
            for field, value, text in VARIANCE_FAULTS:
                refused(text, b=block(**{field: value}))
        else:
            refused("NULL argument", null_block=True)
            refused(WHOLE_FRAME, f=striped)
            assert call(f=wrapped)[0] == abi.RM_OK  # despeckle alone takes a colour-only frame
            assert call(f=wrapped, b=block(desp=None))[0] == abi.RM_OK
            refused(NO_GUIDES, f=wrapped, b=block(den=True))
            refused(NO_GUIDES, f=wrapped, b=block(den=True, desp=None))
            assert call(f=plain, b=block(den=True))[0] == abi.RM_OK
            refused(NO_MOMENTS, f=plain, b=block(den="variance"))
            for field, value, text in CHAIN_FAULTS:
                refused(text, b=block(**{field: value}))
            for field, value, text in ATROUS_FAULTS:
                refused(text, b=block(den=True, **{field: value}))
                refused(text, b=block(den=True, desp=None, **{field: value}))
                bad = block(den=True, **{field: value})
                bad.denoise = abi.RM_DENOISE_NONE  # the stage off: its block is not looked at
                assert call(b=bad)[0] == abi.RM_OK
            for field, value, text in VARIANCE_FAULTS:
                refused(text, b=block(den="variance", **{field: value}))
                bad = block(den="variance", **{field: value})
                bad.denoise = abi.RM_DENOISE_ATROUS
                assert call(b=bad)[0] == abi.RM_OK
        ctx.sync()
    finally:
        for f in (fb, plain, window, striped, wrapped, foreign):
            f.destroy()
        other.close()
        ctx.close()


def test_scratch_grows_and_is_reused_across_sizes_and_streams():
    """One context sees 5 x 7, 33 x 47 and 5 x 7 again: its scratch buffers are made, then freed and made larger -- the despeckle
    buffer while two denoisers are still queued on a caller's stream --, then reused with room to spare.  Every result is the one a
    context gives that only ever saw that size."""
    import torch

    k = 3
    chain = dict(despeckle=True, denoise=True)
    side = torch.cuda.Stream(device=0)

    def results(c, W, H, seed):
        fb = upload_var(c, random_planes(H, W, k, seed=seed), random_moments(H, W, k, seed=seed + 1), "f32")
        try:
            outs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
            torch.cuda.synchronize()
            with torch.cuda.stream(side):  # no wait between the three: the later ones grow buffers behind the earlier ones' work
                c.denoise_device(fb, k, outs[0].data_ptr(), stream=side.cuda_stream)
                c.denoise_variance_device(fb, k, outs[1].data_ptr(), stream=side.cuda_stream)
                c.filter_device(fb, k, outs[2].data_ptr(), stream=side.cuda_stream, **chain)
            side.synchronize()
            got = [o.cpu().numpy() for o in outs]
            got += [fb.denoise(k), fb.denoise_variance(k), fb.filter(k, **chain)]
            got += [fb.present(k, denoise=True), fb.present(k, denoise="variance"), fb.present(k, **chain)]
            return got
        finally:
            fb.destroy()

    a = native.Context(0)
    try:
        for step, (W, H) in enumerate([(5, 7), (33, 47), (5, 7)]):
            got = results(a, W, H, seed=10 + step)
            fresh = native.Context(0)
            try:
                want = results(fresh, W, H, seed=10 + step)
            finally:
                fresh.close()
            assert len(got) == len(want) == 9
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (step, W, H, i)
            # the filters did something: neither output is the colour plane or the untouched fill
            assert not np.array_equal(got[0], got[2]) and not (got[0] == -1.0).all()
    finally:
        a.close()
