"""The probe entry points without a GPU (include/hip_raymarch.h rm_probe, rm_probe_math, rm_probe_camera, rm_probe_rng): what each
answers to a NULL context.  No context exists without a GPU, so every refusal leaves its text in rm_last_error(NULL)."""
import ctypes as C

import numpy as np

from raymarching_engine_amd import abi, native
from test_frame_entries_cpu import sentinel


def test_a_probe_without_a_context_is_refused_with_its_text():
    lib = native.load_library()
    a, out = np.zeros(16, np.float32), np.zeros(64, np.float32)
    u = abi.RmUniforms()
    calls = [
        ("rm_probe: NULL argument", lambda: lib.rm_probe(None, None, abi.RM_PROBE_SDF, native._fp(a), 5, 0.0, 0, native._fp(out))),
        ("rm_probe_math: bad argument", lambda: lib.rm_probe_math(None, 0, native._fp(a), None, 5, native._fp(out))),
        ("probe: bad argument", lambda: lib.rm_probe_camera(None, C.byref(u), 2, 2, native._fp(out))),
        ("probe: bad argument", lambda: lib.rm_probe_rng(None, C.byref(u), 2, 2, 4, native._fp(out))),
    ]
    for text, call in calls:
        sentinel(lib)
        assert call() == abi.RM_ERR_INVALID
        assert lib.rm_last_error(None).decode() == text
