"""The framebuffer entry points on the MI355X as one family (include/hip_raymarch.h rm_fb_create*, rm_fb_wrap*, rm_fb_clear,
rm_fb_download / _upload and their _raw forms, rm_buffer_*): the code AND the text of every refusal of the six constructors, one
fault at a time; the ORDER of the refusals, two faults at a time; what each constructor makes; the copies' round trips, bit for
bit; and that the caller's planes stay the caller's."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as GC
from raymarching_engine_amd import abi, job as J, native, scene as S, shard

pytestmark = pytest.mark.gpu

F32, F16, MOMENTS = abi.RM_GBUFFER_F32, abi.RM_GBUFFER_F16, abi.RM_FB_MOMENTS
UNKNOWN_FORMATS = (2, 255)  # neither is a format, neither carries the RM_FB_MOMENTS bit
SIZE = "framebuffer: size must be 1..65536"
WINDOW = "framebuffer: row window outside the image"
FORMAT = "unknown G-buffer format (RM_GBUFFER_F32 or RM_GBUFFER_F16)"
ALIGNED = "planes must be aligned to their pixel (16 bytes; 8 for half G-buffer planes)"
STRIPED_MOMENTS = "rm_fb_create_striped: RM_FB_MOMENTS needs a framebuffer holding the whole frame (rm_fb_create_fmt)"
STRIPED_PARTS = "rm_fb_create_striped: need stripe_rows >= 1 and 0 <= part < parts"
STRIPED_PLANES = "rm_fb_create_striped: give all planes, colour only, or none"
STRIPED_EMPTY = "rm_fb_create_striped: this part holds no rows"
WRAP_MOMENTS = "rm_fb_wrap: RM_FB_MOMENTS is for owned framebuffers (rm_fb_create_fmt)"
WRAP_PLANES = "rm_fb_wrap: give both G-buffer planes or neither"


class Calls:
    """The six constructors through ctypes with every argument in the caller's hands: (code, text, handle) of one call, the
    sentinel texts laid down first so that the text read back is this call's.  Handles that were made are destroyed by close()."""

    def __init__(self):
        import torch

        self.ctx = native.Context(0)
        self.lib = self.ctx.lib
        self.made = []
        # three caller planes of 16 x 16 float4 with room behind them for a pointer that is off by 4 or 8 bytes
        self.planes = [torch.zeros((16 * 16 * 4 + 4,), dtype=torch.float32, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        self.c, self.n, self.a = (p.data_ptr() for p in self.planes)

    def _call(self, fn, null_ctx, args, null_out):
        lib, h = self.lib, C.c_void_p()
        lib.rm_ctx_create(0, None)
        assert lib.rm_ctx_set_retire_eps(self.ctx.h, -1.0) == abi.RM_ERR_INVALID
        rc = fn(None if null_ctx else self.ctx.h, *args, None if null_out else C.byref(h))
        if h.value:
            self.made.append(h)
        return rc, lib.rm_last_error(None if null_ctx else self.ctx.h).decode(), h

    def create(self, W=16, H=16, begin=0, count=None, fmt=F32, null_ctx=False, null_out=False, plain=False):
        args = (W, H, begin, H if count is None else count)
        return self._call(self.lib.rm_fb_create, null_ctx, args, null_out) if plain else \
            self._call(self.lib.rm_fb_create_fmt, null_ctx, args + (fmt,), null_out)

    def striped(self, W=16, H=16, stripe=8, parts=2, part=0, c=None, n=None, a=None, fmt=F32, null_ctx=False, null_out=False, plain=False):
        args = (W, H, stripe, parts, part, C.c_void_p(c or 0), C.c_void_p(n or 0), C.c_void_p(a or 0))
        return self._call(self.lib.rm_fb_create_striped, null_ctx, args, null_out) if plain else \
            self._call(self.lib.rm_fb_create_striped_fmt, null_ctx, args + (fmt,), null_out)

    def wrap(self, W=16, H=16, begin=0, count=None, c="own", n=None, a=None, fmt=F32, null_ctx=False, null_out=False, plain=False):
        c = self.c if c == "own" else c
        args = (W, H, begin, H if count is None else count, C.c_void_p(c or 0), C.c_void_p(n or 0), C.c_void_p(a or 0))
        return self._call(self.lib.rm_fb_wrap, null_ctx, args, null_out) if plain else \
            self._call(self.lib.rm_fb_wrap_fmt, null_ctx, args + (fmt,), null_out)

    def close(self):
        for h in self.made:
            self.lib.rm_fb_destroy(h)
        self.ctx.close()


@pytest.fixture
def calls():
    k = Calls()
    try:
        yield k
    finally:
        k.close()


def refused(result, text):
    rc, got, h = result
    assert (rc, got, h.value) == (abi.RM_ERR_INVALID, text, None)


def accepted(result):
    rc, _, h = result
    assert rc == abi.RM_OK and h.value


def test_every_refusal_of_rm_fb_create(calls):
    k = calls
    for plain in (False, True):  # rm_fb_create forwards to rm_fb_create_fmt: the same refusals
        accepted(k.create(plain=plain))
        refused(k.create(null_ctx=True, plain=plain), "rm_fb_create: NULL argument")
        refused(k.create(null_out=True, plain=plain), "rm_fb_create: NULL argument")
        for size in (0, 65537):
            refused(k.create(W=size, plain=plain), SIZE)
            refused(k.create(H=size, count=1, plain=plain), SIZE)
        refused(k.create(begin=-1, count=4, plain=plain), WINDOW)
        refused(k.create(begin=0, count=0, plain=plain), WINDOW)
        refused(k.create(begin=9, count=8, plain=plain), WINDOW)
    for fmt in UNKNOWN_FORMATS:
        refused(k.create(fmt=fmt), "rm_fb_create: " + FORMAT)
        refused(k.create(fmt=fmt | MOMENTS), "rm_fb_create: " + FORMAT)
    for fmt in (F32, F16, F32 | MOMENTS, F16 | MOMENTS):
        accepted(k.create(fmt=fmt))
    accepted(k.create(begin=8, count=8))


def test_every_refusal_of_rm_fb_create_striped(calls):
    k = calls
    for plain in (False, True):
        accepted(k.striped(plain=plain))
        refused(k.striped(null_ctx=True, plain=plain), "rm_fb_create_striped: NULL argument")
        refused(k.striped(null_out=True, plain=plain), "rm_fb_create_striped: NULL argument")
        for size in (0, 65537):
            refused(k.striped(W=size, plain=plain), SIZE)
            refused(k.striped(H=size, plain=plain), SIZE)
        refused(k.striped(stripe=0, plain=plain), STRIPED_PARTS)
        refused(k.striped(parts=0, part=0, plain=plain), STRIPED_PARTS)
        refused(k.striped(part=-1, plain=plain), STRIPED_PARTS)
        refused(k.striped(parts=2, part=2, plain=plain), STRIPED_PARTS)
        # the three planes: all, colour only, or none
        for c, n, a in ((0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1)):
            refused(k.striped(c=c and k.c, n=n and k.n, a=a and k.a, plain=plain), STRIPED_PLANES)
        accepted(k.striped(c=k.c, plain=plain))
        accepted(k.striped(c=k.c, n=k.n, a=k.a, plain=plain))
        # alignment: to the plane's own pixel
        refused(k.striped(c=k.c + 4, plain=plain), "rm_fb_create_striped: " + ALIGNED)
        refused(k.striped(c=k.c, n=k.n + 4, a=k.a, plain=plain), "rm_fb_create_striped: " + ALIGNED)
        refused(k.striped(c=k.c, n=k.n, a=k.a + 8, plain=plain), "rm_fb_create_striped: " + ALIGNED)  # (fp32 planes: 16 bytes)
        refused(k.striped(H=8, stripe=8, parts=2, part=1, plain=plain), STRIPED_EMPTY)
    refused(k.striped(fmt=F32 | MOMENTS), STRIPED_MOMENTS)
    refused(k.striped(fmt=F16 | MOMENTS), STRIPED_MOMENTS)
    for fmt in UNKNOWN_FORMATS:
        refused(k.striped(fmt=fmt), "rm_fb_create_striped: " + FORMAT)
    for off in ("n", "a"):  # a half G-buffer plane: 8 bytes
        ptrs = dict(c=k.c, n=k.n, a=k.a)
        refused(k.striped(**{**ptrs, off: ptrs[off] + 4}, fmt=F16), "rm_fb_create_striped: " + ALIGNED)
        accepted(k.striped(**{**ptrs, off: ptrs[off] + 8}, fmt=F16))
    refused(k.striped(c=k.c + 8, n=k.n, a=k.a, fmt=F16), "rm_fb_create_striped: " + ALIGNED)  # (the colour plane stays fp32)


def test_every_refusal_of_rm_fb_wrap(calls):
    k = calls
    for plain in (False, True):
        accepted(k.wrap(plain=plain))
        accepted(k.wrap(n=k.n, a=k.a, plain=plain))
        refused(k.wrap(null_ctx=True, plain=plain), "rm_fb_wrap: NULL argument")
        refused(k.wrap(null_out=True, plain=plain), "rm_fb_wrap: NULL argument")
        refused(k.wrap(c=None, plain=plain), "rm_fb_wrap: NULL argument")
        refused(k.wrap(c=None, n=k.n, a=k.a, plain=plain), "rm_fb_wrap: NULL argument")
        for size in (0, 65537):
            refused(k.wrap(W=size, plain=plain), SIZE)
            refused(k.wrap(H=size, count=1, plain=plain), SIZE)
        refused(k.wrap(begin=-1, count=4, plain=plain), WINDOW)
        refused(k.wrap(begin=0, count=0, plain=plain), WINDOW)
        refused(k.wrap(begin=9, count=8, plain=plain), WINDOW)
        refused(k.wrap(n=k.n, plain=plain), WRAP_PLANES)
        refused(k.wrap(a=k.a, plain=plain), WRAP_PLANES)
        refused(k.wrap(c=k.c + 4, plain=plain), "rm_fb_wrap: " + ALIGNED)
        refused(k.wrap(n=k.n + 4, a=k.a, plain=plain), "rm_fb_wrap: " + ALIGNED)
        refused(k.wrap(n=k.n, a=k.a + 8, plain=plain), "rm_fb_wrap: " + ALIGNED)  # (fp32 planes: 16 bytes)
    refused(k.wrap(fmt=F32 | MOMENTS), WRAP_MOMENTS)
    refused(k.wrap(fmt=F16 | MOMENTS), WRAP_MOMENTS)
    for fmt in UNKNOWN_FORMATS:
        refused(k.wrap(fmt=fmt), "rm_fb_wrap: " + FORMAT)
    for off in ("n", "a"):
        ptrs = dict(n=k.n, a=k.a)
        refused(k.wrap(**{**ptrs, off: ptrs[off] + 4}, fmt=F16), "rm_fb_wrap: " + ALIGNED)
        accepted(k.wrap(**{**ptrs, off: ptrs[off] + 8}, fmt=F16))
    refused(k.wrap(c=k.c + 8, n=k.n, a=k.a, fmt=F16), "rm_fb_wrap: " + ALIGNED)


def test_the_order_of_the_refusals(calls):
    """Two faults in one call: the text is that of the fault the family checks first.  One call per pair of neighbours in each
    family's order -- rm_fb_create_fmt: NULL, format, size and window; rm_fb_create_striped_fmt: NULL, moments, format, size,
    stripe / parts / part, plane combination, alignment, "holds no rows"; rm_fb_wrap_fmt: NULL (colour included), moments, format,
    size and window, plane pair, alignment."""
    k = calls
    bad = UNKNOWN_FORMATS[0]
    refused(k.create(null_out=True, fmt=bad), "rm_fb_create: NULL argument")
    refused(k.create(fmt=bad, W=0), "rm_fb_create: " + FORMAT)
    refused(k.create(fmt=bad, begin=9, count=8), "rm_fb_create: " + FORMAT)
    refused(k.create(W=0, begin=9, count=8), SIZE)  # (and the size before the window)

    refused(k.striped(null_out=True, fmt=F32 | MOMENTS), "rm_fb_create_striped: NULL argument")
    refused(k.striped(fmt=bad | MOMENTS), STRIPED_MOMENTS)
    refused(k.striped(fmt=bad, W=0), "rm_fb_create_striped: " + FORMAT)
    refused(k.striped(W=0, stripe=0), SIZE)
    refused(k.striped(stripe=0, n=k.n), STRIPED_PARTS)
    refused(k.striped(c=k.c + 4, n=k.n), STRIPED_PLANES)
    refused(k.striped(H=8, stripe=8, parts=2, part=1, c=k.c + 4), "rm_fb_create_striped: " + ALIGNED)

    refused(k.wrap(c=None, fmt=F32 | MOMENTS), "rm_fb_wrap: NULL argument")
    refused(k.wrap(null_out=True, fmt=F32 | MOMENTS), "rm_fb_wrap: NULL argument")
    refused(k.wrap(fmt=bad | MOMENTS), WRAP_MOMENTS)
    refused(k.wrap(fmt=bad, W=0), "rm_fb_wrap: " + FORMAT)
    refused(k.wrap(begin=9, count=8, n=k.n), WINDOW)
    refused(k.wrap(c=k.c + 4, n=k.n), WRAP_PLANES)


def described(lib, h):
    return (lib.rm_fb_rows(h), lib.rm_fb_width(h), lib.rm_fb_height(h), lib.rm_fb_gbuffer(h), lib.rm_fb_has_moments(h))


def planes_of(fb):
    return (0, 1, 2, 3) if fb.moments else (0, 1, 2)


def assert_all_zero(fb):
    for plane in planes_of(fb):
        raw = fb.download_raw(plane)
        assert raw.shape == (fb.row_count, fb.width, 2 if plane == 3 else 4) and raw.dtype == fb.plane_dtype(plane)
        assert not raw.view(np.uint8).any(), plane


def render_then_clear(ctx, scene, fb, schema):
    """A render leaves something in the planes; rm_fb_clear zeroes every one of them again, the moments plane included."""
    ctx.render_sample(scene, fb, J.uniforms_from_schema(schema, (0.5, 1.0 / 3.0)), None, abi.RM_RENDER_FAST)
    assert fb.download_raw(0).any()
    if fb.moments:
        fb.upload_raw(3, np.ones((fb.row_count, fb.width, 2), np.float32))
    fb.clear()
    assert_all_zero(fb)


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_what_each_constructor_makes(gbuffer):
    import torch

    code = native.gbuffer_code(gbuffer)
    W, H = 40, 100  # ragged: 12.5 stripes of 8 rows
    sc = S.Mandelbulb()
    schema = J.make_schema(sc, W, H, counts=(40,), render_mode="full", position=(0, 0, -2.5), lights=GC.LIGHT)
    ctx = native.Context(0)
    lib = ctx.lib
    try:
        scene = ctx.create_scene(sc)
        for moments in (False, True):
            whole = ctx.create_framebuffer(W, H, gbuffer=gbuffer, moments=moments)
            assert described(lib, whole.h) == (H, W, H, code, int(moments)) and whole.moments == moments
            window = ctx.create_framebuffer(W, H, 30, 17, gbuffer=gbuffer, moments=moments)
            assert described(lib, window.h) == (17, W, H, code, int(moments))
            for fb in (whole, window):
                assert (lib.rm_fb_device_ptr(fb.h, 3) is not None) == moments
                assert_all_zero(fb)
                render_then_clear(ctx, scene, fb, schema)
                fb.destroy()
        for part in range(3):
            rows = len(shard.owned_rows(H, 3, part, 8))
            fb = ctx.create_striped_framebuffer(W, H, 8, 3, part, gbuffer=gbuffer)
            assert described(lib, fb.h) == (rows, W, H, code, 0) and fb.row_count == rows
            assert lib.rm_fb_device_ptr(fb.h, 3) is None
            assert_all_zero(fb)
            render_then_clear(ctx, scene, fb, schema)
            fb.destroy()
        # over the caller's planes: a wrapped window, and a striped part
        dtype = torch.float16 if gbuffer == "f16" else torch.float32
        colour = torch.full((17, W, 4), 3.0, dtype=torch.float32, device="cuda:0")
        guides = [torch.full((17, W, 4), 3.0, dtype=dtype, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        for fb, rows in ((ctx.wrap_framebuffer(W, H, 30, 17, colour.data_ptr(), gbuffer=gbuffer), 17),
                         (ctx.wrap_framebuffer(W, H, 30, 17, colour.data_ptr(), guides[0].data_ptr(), guides[1].data_ptr(), gbuffer=gbuffer), 17),
                         (ctx.create_striped_framebuffer(W, H, 8, 8, 2, colour.data_ptr(), gbuffer=gbuffer), 16),
                         (ctx.create_striped_framebuffer(W, H, 8, 8, 2, colour.data_ptr(), guides[0].data_ptr(), guides[1].data_ptr(), gbuffer=gbuffer), 16)):
            assert described(lib, fb.h) == (rows, W, H, code, 0)
            assert fb.device_ptr(0) == colour.data_ptr()
            assert fb.device_ptr(1) in (0, guides[0].data_ptr()) and fb.device_ptr(2) in (0, guides[1].data_ptr())
            assert (fb.device_ptr(1) == 0) == (fb.device_ptr(2) == 0)
            assert lib.rm_fb_device_ptr(fb.h, 3) is None
            fb.destroy()
        assert bool((colour == 3.0).all()) and all(bool((g == 3.0).all()) for g in guides)  # nothing was zeroed: they are the caller's
        scene.destroy()
    finally:
        ctx.close()


def exact_in_half(rng, shape):
    """Values binary16 holds exactly (multiples of 1/8 below 256), none of them zero."""
    return (rng.integers(1, 2048, size=shape) / 8.0).astype(np.float32) * rng.choice([-1.0, 1.0], size=shape).astype(np.float32)


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_round_trips_are_bitwise(gbuffer):
    W, H, begin, rows = 24, 32, 5, 10  # a 24 x 10 window: neither a multiple of 8
    rng = np.random.default_rng(7)
    ctx = native.Context(0)
    lib = ctx.lib
    try:
        fb = ctx.create_framebuffer(W, H, begin, rows, gbuffer=gbuffer, moments=True)
        for plane in (0, 1, 2):
            want = exact_in_half(rng, (rows, W, 4))
            fb.upload(plane, want)
            assert np.array_equal(fb.download(plane).view(np.uint32), want.view(np.uint32)), plane
            stored = want.astype(fb.plane_dtype(plane))
            raw = fb.download_raw(plane)
            assert raw.dtype == stored.dtype and np.array_equal(raw.view(np.uint8), stored.view(np.uint8)), plane
            want = exact_in_half(rng, (rows, W, 4))
            fb.upload_raw(plane, want.astype(fb.plane_dtype(plane)))
            assert np.array_equal(fb.download_raw(plane).view(np.uint8), want.astype(fb.plane_dtype(plane)).view(np.uint8)), plane
            assert np.array_equal(fb.download(plane).view(np.uint32), want.view(np.uint32)), plane
        m = exact_in_half(rng, (rows, W, 2))
        fb.upload_raw(3, m)
        assert np.array_equal(fb.download_raw(3).view(np.uint32), m.view(np.uint32))
        # the float entries take planes 0..2, the raw ones 0..3, and the raw ones the plane's size to the byte
        host = np.zeros((rows, W, 4), np.float32)
        for name in ("rm_fb_download", "rm_fb_upload"):
            assert getattr(lib, name)(fb.h, 3, host.ctypes.data_as(C.POINTER(C.c_float))) == abi.RM_ERR_INVALID
            assert lib.rm_last_error(ctx.h).decode() == f"{name}: bad argument"
        for name in ("rm_fb_download_raw", "rm_fb_upload_raw"):
            fn = getattr(lib, name)
            assert fn(fb.h, 4, host.ctypes.data_as(C.c_void_p), host.nbytes) == abi.RM_ERR_INVALID
            assert lib.rm_last_error(ctx.h).decode() == f"{name}: bad argument"
            for plane in (0, 1, 3):
                px = 8 if plane == 3 or (plane == 1 and gbuffer == "f16") else 16
                holds = rows * W * px
                for given in (holds - 1, holds + 1):
                    assert fn(fb.h, plane, host.ctypes.data_as(C.c_void_p), given) == abi.RM_ERR_INVALID
                    assert lib.rm_last_error(ctx.h).decode() == \
                        f"{name}: plane {plane} holds {holds} bytes ({rows} x {W} pixels of {px} bytes), not {given}"
        plain = ctx.create_framebuffer(W, H, begin, rows, gbuffer=gbuffer)
        for name in ("rm_fb_download_raw", "rm_fb_upload_raw"):
            assert getattr(lib, name)(plain.h, 3, host.ctypes.data_as(C.c_void_p), rows * W * 8) == abi.RM_ERR_INVALID
            assert lib.rm_last_error(ctx.h).decode() == f"{name}: this framebuffer has no such plane"
        plain.destroy()
        fb.destroy()
    finally:
        ctx.close()


def test_buffers_round_trip_and_refuse():
    ctx, other = native.Context(0), native.Context(0)
    lib = ctx.lib
    try:
        b = ctx.buffer(1000)
        assert not b.download().any()  # zero-filled
        data = np.random.default_rng(3).integers(0, 256, size=1000, dtype=np.uint8)
        b.upload(data)
        assert np.array_equal(b.download(), data)
        b.upload(data[:10][::-1])  # fewer bytes than it holds: from its base
        assert np.array_equal(b.download(), np.concatenate([data[:10][::-1], data[10:]]))
        host = np.zeros(1001, np.uint8)
        foreign = other.buffer(1000)
        for name in ("rm_buffer_download", "rm_buffer_upload"):
            fn = getattr(lib, name)
            assert fn(ctx.h, b.ptr, host.ctypes.data_as(C.c_void_p), 1001) == abi.RM_ERR_INVALID
            assert lib.rm_last_error(ctx.h).decode() == f"{name}: more bytes than the buffer holds"
            for ptr in (foreign.ptr, b.ptr + 16):  # another context's buffer; not a base address
                assert fn(ctx.h, ptr, host.ctypes.data_as(C.c_void_p), 8) == abi.RM_ERR_INVALID
                assert lib.rm_last_error(ctx.h).decode() == f"{name}: not a buffer of this context"
            assert fn(ctx.h, b.ptr, None, 8) == abi.RM_ERR_INVALID
            assert lib.rm_last_error(ctx.h).decode() == f"{name}: NULL argument"
        assert np.array_equal(b.download()[10:], data[10:])  # the refused calls moved nothing
        ptr = b.ptr
        b.destroy()
        assert lib.rm_buffer_destroy(ctx.h, ptr) == abi.RM_ERR_INVALID  # a second destroy
        assert lib.rm_last_error(ctx.h).decode() == "rm_buffer_destroy: not a buffer of this context"
        assert lib.rm_buffer_destroy(ctx.h, foreign.ptr) == abi.RM_ERR_INVALID
        assert lib.rm_buffer_destroy(ctx.h, None) == abi.RM_OK
        foreign.destroy()
    finally:
        ctx.close()
        other.close()


@pytest.mark.parametrize("gbuffer", ["f32", "f16"])
def test_the_callers_planes_stay_the_callers(gbuffer):
    """Destroying a wrapped framebuffer, or a striped one over the caller's planes, frees nothing of the caller's: the tensors hold
    the bytes they held and can be written again."""
    import torch

    W, H = 24, 16
    dtype = torch.float16 if gbuffer == "f16" else torch.float32
    ctx = native.Context(0)
    try:
        for make in ("wrap", "striped"):
            planes = [torch.arange(H * W * 4, device="cuda:0").remainder(251).to(torch.float32 if i == 0 else dtype).reshape(H, W, 4) for i in range(3)]
            before = [p.clone() for p in planes]
            torch.cuda.synchronize()
            ptrs = [p.data_ptr() for p in planes]
            fb = ctx.wrap_framebuffer(W, H, 0, H, *ptrs, gbuffer=gbuffer) if make == "wrap" else \
                ctx.create_striped_framebuffer(W, H, 8, 1, 0, *ptrs, gbuffer=gbuffer)
            assert fb.row_count == H
            want = exact_in_half(np.random.default_rng(5), (H, W, 4))
            fb.upload(1, want)  # through the library into the caller's plane
            assert np.array_equal(planes[1].cpu().numpy().astype(np.float32), want)
            fb.destroy()
            torch.cuda.synchronize()
            assert torch.equal(planes[0], before[0]) and torch.equal(planes[2], before[2])
            assert np.array_equal(planes[1].cpu().numpy().astype(np.float32), want)
            for p in planes:  # still the caller's memory: written and read again
                p.fill_(2.0)
            torch.cuda.synchronize()
            assert all(bool((p == 2.0).all()) for p in planes)
    finally:
        ctx.close()
