"""The nine frame-filter entry points without a GPU (include/hip_raymarch.h rm_denoise*, rm_denoise_variance*, rm_filter*): the
text of every refusal that needs no context.  No context exists without a GPU, so every call ends in RM_ERR_INVALID and its text
is rm_last_error(NULL)'s."""
import ctypes as C

import numpy as np
import pytest

from raymarching_engine_amd import abi, native

# entry point -> (family, ending); the ending decides the arguments after the parameter block
ENTRIES = {
    "rm_denoise": ("atrous", "host"), "rm_denoise_device": ("atrous", "device"), "rm_present_denoised": ("atrous", "rgba8"),
    "rm_denoise_variance": ("variance", "host"), "rm_denoise_variance_device": ("variance", "device"),
    "rm_present_denoised_variance": ("variance", "rgba8"),
    "rm_filter": ("chain", "host"), "rm_filter_device": ("chain", "device"), "rm_present_filtered": ("chain", "rgba8"),
}
CHAIN = [name for name, (family, _) in ENTRIES.items() if family == "chain"]

# the chain's own values, which rm_filter* checks before the handles: (field of the despeckle block or of the chain, value, text)
CHAIN_FAULTS = [
    ("despeckle", -1, "despeckle must be 0 or 1"), ("despeckle", 2, "despeckle must be 0 or 1"),
    ("denoise", -1, "unknown denoise mode"), ("denoise", 3, "unknown denoise mode"),
    ("radius", 0, "despeckle radius must be 1 or 2"), ("radius", 3, "despeckle radius must be 1 or 2"),
    ("rank", -1, "despeckle rank must be in 0..3"), ("rank", 4, "despeckle rank must be in 0..3"),
    ("gain", 0.5, "despeckle gain must be finite and >= 1"), ("gain", float("inf"), "despeckle gain must be finite and >= 1"),
    ("gain", float("nan"), "despeckle gain must be finite and >= 1"),
    ("floor", -0.1, "despeckle floor must be finite and >= 0"), ("floor", float("inf"), "despeckle floor must be finite and >= 0"),
    ("floor", float("nan"), "despeckle floor must be finite and >= 0"),
    ("reserved", 1, "despeckle reserved must be 0"),
]


def call_without_a_context(lib, name, block):
    """(code, text) of the entry point with NULL handles and NULL outputs (a host output for the float plane, as a caller's)."""
    out = np.zeros(4, np.float32)
    tail = {"host": (out.ctypes.data_as(C.POINTER(C.c_float)),), "device": (None, None), "rgba8": (None,)}[ENTRIES[name][1]]
    lib.rm_ctx_create(0, None)  # leaves a text of its own behind, so that the one read below is this call's
    assert lib.rm_last_error(None).decode() == "rm_ctx_create: out is NULL"
    rc = getattr(lib, name)(None, None, 1, C.byref(block) if block is not None else None, *tail)
    return rc, lib.rm_last_error(None).decode()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_handles_are_refused_by_name(name):
    lib = native.load_library()
    blocks = {"atrous": [None, native.denoise_params()], "variance": [None, native.denoise_variance_params()],
              "chain": [None, native.filters(), native.filters(True, True), native.filters(True, "variance")]}[ENTRIES[name][0]]
    for block in blocks:  # NULL parameters are the older families' defaults and the chain's refusal: the same text either way
        assert call_without_a_context(lib, name, block) == (abi.RM_ERR_INVALID, f"{name}: NULL argument")


@pytest.mark.parametrize("name", CHAIN)
def test_the_chains_own_values_are_refused_first_and_by_name(name):
    lib = native.load_library()
    for field, value, text in CHAIN_FAULTS:
        f = native.filters(despeckle=True, denoise=True)
        setattr(f if field in ("despeckle", "denoise") else f.despeckle_params, field, value)
        assert call_without_a_context(lib, name, f) == (abi.RM_ERR_INVALID, f"{name}: {text}"), (field, value)
        if field not in ("despeckle", "denoise"):
            f.despeckle = 0  # the stage off: its parameters are not looked at
            assert call_without_a_context(lib, name, f) == (abi.RM_ERR_INVALID, f"{name}: NULL argument"), (field, value)
