"""The framebuffer entry points and the sharded present without a GPU (include/hip_raymarch.h rm_fb_*, rm_present_sharded*):
what each answers to NULL handles.  No context exists without a GPU, so every refusal that has a text leaves it in
rm_last_error(NULL)."""
import ctypes as C

import numpy as np
import pytest

from raymarching_engine_amd import abi, native

# constructor -> (family its texts are prefixed with, the arguments between the context and `out`)
CONSTRUCTORS = {
    "rm_fb_create": ("rm_fb_create", (16, 16, 0, 16)),
    "rm_fb_create_fmt": ("rm_fb_create", (16, 16, 0, 16, abi.RM_GBUFFER_F32)),
    "rm_fb_create_striped": ("rm_fb_create_striped", (16, 16, 8, 2, 0, None, None, None)),
    "rm_fb_create_striped_fmt": ("rm_fb_create_striped", (16, 16, 8, 2, 0, None, None, None, abi.RM_GBUFFER_F32)),
    "rm_fb_wrap": ("rm_fb_wrap", (16, 16, 0, 16, None, None, None)),
    "rm_fb_wrap_fmt": ("rm_fb_wrap", (16, 16, 0, 16, None, None, None, abi.RM_GBUFFER_F32)),
}


def sentinel(lib):
    """Leaves a text of its own behind, so that the one read afterwards is the next call's."""
    lib.rm_ctx_create(0, None)
    assert lib.rm_last_error(None).decode() == "rm_ctx_create: out is NULL"


@pytest.mark.parametrize("name", sorted(CONSTRUCTORS))
def test_a_constructor_without_a_context_is_refused_by_family(name):
    lib = native.load_library()
    family, args = CONSTRUCTORS[name]
    for out in (C.byref(C.c_void_p()), None):
        sentinel(lib)
        assert getattr(lib, name)(None, *args, out) == abi.RM_ERR_INVALID
        assert lib.rm_last_error(None).decode() == f"{family}: NULL argument"


def test_the_sharded_present_without_its_arrays_is_refused():
    lib = native.load_library()
    out = np.zeros(16, np.uint8)
    out_p = out.ctypes.data_as(C.POINTER(C.c_uint8))
    calls = [
        ("rm_present_sharded: NULL argument", lambda: lib.rm_present_sharded(None, None, 2, 1, 0, out_p, out.nbytes)),
        ("rm_present_sharded: NULL argument", lambda: lib.rm_present_sharded(None, None, 2, 1, 0, None, 0)),
        ("rm_present_sharded: NULL argument", lambda: lib.rm_present_sharded_start(None, None, 2, 1, 0)),
        ("rm_present_sharded_finish: NULL argument", lambda: lib.rm_present_sharded_finish(None, 2, out_p, out.nbytes)),
    ]
    for text, call in calls:
        sentinel(lib)
        assert call() == abi.RM_ERR_INVALID
        assert lib.rm_last_error(None).decode() == text


def test_a_null_framebuffer_is_refused_or_answered_with_the_defaults():
    lib = native.load_library()
    host = np.zeros(16, np.float32)
    fp, vp = host.ctypes.data_as(C.POINTER(C.c_float)), host.ctypes.data_as(C.c_void_p)
    for plane in (0, 1, 2):
        assert lib.rm_fb_download(None, plane, fp) == abi.RM_ERR_INVALID
        assert lib.rm_fb_upload(None, plane, fp) == abi.RM_ERR_INVALID
        assert lib.rm_fb_download_raw(None, plane, vp, host.nbytes) == abi.RM_ERR_INVALID
        assert lib.rm_fb_upload_raw(None, plane, vp, host.nbytes) == abi.RM_ERR_INVALID
    assert lib.rm_fb_clear(None) == abi.RM_ERR_INVALID
    assert lib.rm_fb_rows(None) == 0 and lib.rm_fb_width(None) == 0 and lib.rm_fb_height(None) == 0
    assert lib.rm_fb_gbuffer(None) == abi.RM_GBUFFER_F32
    assert lib.rm_fb_has_moments(None) == 0
    for plane in (0, 1, 2, 3):
        assert lib.rm_fb_device_ptr(None, plane) is None
    lib.rm_fb_destroy(None)  # and a NULL handle is nothing to destroy
