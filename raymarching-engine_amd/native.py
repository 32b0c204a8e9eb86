"""ctypes binding of libhip_raymarch.so (include/hip_raymarch.h).

The library is the product's compute path.  If it is missing this module
raises: there is no Python or CPU fallback for rendering.
"""
from __future__ import annotations

import ctypes as C
import math
from pathlib import Path
from typing import Optional

import numpy as np

from . import abi
from .scene import Scene

import os

# Process environment the device path depends on, set where the library is loaded so that EVERY host gets it (bench.py,
# the job API, the tests), unless the user has set it.  Read by the HIP / HSA runtime when it starts, so it has to be in
# place before anything in this process touches the GPU:
#  * HSA_ENABLE_IPC_MODE_LEGACY=0: dmabuf IPC, which RCCL needs across processes on this driver.
# The runtime's hardware queues stay at its default: side streams that share one serialise, and
# rm_ctx_set_samples_in_flight says so (rm_ctx_last_warning).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

# RM_LIB selects an experiment build of the SAME library (tools/); default = the in-tree product
LIB_PATH = Path(os.environ.get("RM_LIB") or Path(__file__).resolve().parent / "libhip_raymarch.so")

# every symbol include/hip_raymarch.h declares
EXPORTS = [
    "rm_abi_version", "rm_material_default", "rm_ctx_create", "rm_ctx_destroy", "rm_last_error", "rm_ctx_set_stream",
    "rm_ctx_set_retire_eps", "rm_ctx_set_samples_in_flight", "rm_ctx_last_warning", "rm_ctx_set_cost_order", "rm_ctx_set_cull_min_pixels", "rm_ctx_set_cull_budget", "rm_ctx_cull_stats", "rm_debug_counters", "rm_device_memory", "rm_sync", "rm_scene_create", "rm_scene_destroy", "rm_fb_create", "rm_fb_create_striped", "rm_fb_rows", "rm_fb_width", "rm_fb_height", "rm_fb_wrap", "rm_fb_clear", "rm_fb_destroy",
    "rm_fb_download", "rm_fb_upload", "rm_fb_device_ptr", "rm_buffer_create", "rm_buffer_destroy", "rm_buffer_download", "rm_buffer_upload", "rm_render_sample", "rm_render_samples", "rm_ctx_set_sample_batch", "rm_ctx_set_gl_stack", "rm_render_timed",
    "rm_probe", "rm_probe_camera", "rm_probe_rng", "rm_probe_math", "rm_assemble_striped", "rm_assemble_striped_bytes", "rm_present", "rm_present_planes", "rm_present_device", "rm_present_rows", "rm_pack_present_rows", "rm_ctx_last_pipeline", "rm_present_sharded", "rm_present_sharded_start", "rm_present_sharded_finish", "rm_present_striped_rows", "rm_debug_cull_cell",
    "rm_fb_create_fmt", "rm_fb_create_striped_fmt", "rm_fb_wrap_fmt", "rm_fb_gbuffer", "rm_fb_download_raw", "rm_fb_upload_raw",
    "rm_denoise_default", "rm_denoise", "rm_denoise_device", "rm_present_denoised",
    "rm_fb_has_moments", "rm_denoise_variance_default", "rm_denoise_variance", "rm_denoise_variance_device", "rm_present_denoised_variance",
    "rm_filters_default", "rm_filter", "rm_filter_device", "rm_present_filtered",
    "rm_frame_stats", "rm_auto_exposure_default", "rm_stats_percentile", "rm_stats_exposure",
    "rm_display_default", "rm_present_display", "rm_present_display_device", "rm_present_linear",
    "rm_grid_axis", "rm_sdf_grid", "rm_sdf_grid_device", "rm_mesh_params_default", "rm_mesh_extract", "rm_mesh_from_values", "rm_mesh_counts", "rm_mesh_timings",
    "rm_mesh_download", "rm_mesh_device_ptr", "rm_mesh_destroy", "rm_mesh_sharp_default", "rm_mesh_extract_sharp",
    "rm_mesh_keep_default", "rm_mesh_components", "rm_mesh_components_download", "rm_mesh_filter",
    "rm_mesh_simplify_default", "rm_mesh_simplify", "rm_mesh_quadric_default", "rm_mesh_simplify_quadric",
    "rm_mesh_occlusion_default", "rm_mesh_occlusion_directions", "rm_mesh_occlusion",
    "rm_mesh_measure", "rm_mesh_measure_components",
    "rm_mesh_slabs_default", "rm_mesh_extract_slabs", "rm_mesh_extract_sharp_slabs", "rm_mesh_from_values_slabs",
    "rm_mesh_project_default", "rm_mesh_project",
    "rm_mesh_deviation_default", "rm_mesh_deviation_weights", "rm_mesh_deviation",
    "rm_mesh_refine_default", "rm_mesh_refine",
]

# G-buffer formats of a framebuffer (include/hip_raymarch.h RM_GBUFFER_*): "f32" (the default: the software GL stack's planes, which the
# goldens were rendered on) or "f16" (the reference's RGBA16F normal + DoF radius and albedo + depth planes, LoadRenderJobContext.tsx:81-119)
GBUFFER_FORMATS = {"f32": abi.RM_GBUFFER_F32, "f16": abi.RM_GBUFFER_F16}


def gbuffer_code(gbuffer: str) -> int:
    """The RM_GBUFFER_* value of a format name; ValueError for anything else."""
    if not isinstance(gbuffer, str) or gbuffer not in GBUFFER_FORMATS:
        raise ValueError(f"gbuffer must be one of {sorted(GBUFFER_FORMATS)}, not {gbuffer!r}")
    return GBUFFER_FORMATS[gbuffer]


# The hosts' parameter blocks (include/hip_raymarch.h), one table each for _params: the prefix of its messages, the forms that mean
# "the defaults" as the refusal of any other form lists them, the defaults, the dict entry that may name the filter ("mode"), the
# fields a dict has to give as integers / as numbers, and the library's own checks in the library's order as field: (holds, text)
# -- `reserved` is listed where it must be 0.
_POSITIVE = (lambda v: math.isfinite(v) and v > 0.0, "must be finite and > 0")
_ITERATIONS = (lambda v: 0 <= v <= 8, "must be in 0..8")
_ZERO = (lambda v: v == 0, "must be 0")
_BLOCKS = {
    abi.RmDenoise: dict(label="denoise", forms="True", defaults=abi.DENOISE_DEFAULTS,
                        checks=dict(iterations=_ITERATIONS, sigma_color=_POSITIVE, sigma_normal=_POSITIVE, sigma_depth=_POSITIVE)),
    abi.RmDenoiseVariance: dict(label="denoise", forms='True, "variance"', defaults=abi.DENOISE_VARIANCE_DEFAULTS, mode="variance",
                                checks=dict(iterations=_ITERATIONS, sigma_luminance=_POSITIVE, sigma_normal=_POSITIVE, sigma_depth=_POSITIVE,
                                            reserved=_ZERO)),
    abi.RmDespeckle: dict(label="despeckle", forms="True", defaults=abi.DESPECKLE_DEFAULTS, integers=("radius", "rank", "repair"),
                          numbers=("gain", "floor"),
                          checks=dict(radius=(lambda v: v in (1, 2), "must be 1 or 2"), rank=(lambda v: 0 <= v <= 3, "must be in 0..3"),
                                      gain=(lambda v: math.isfinite(v) and v >= 1.0, "must be finite and >= 1"),
                                      floor=(lambda v: math.isfinite(v) and v >= 0.0, "must be finite and >= 0"), reserved=_ZERO)),
    # white is checked for the operator that reads it alone (display_params), as the library does
    abi.RmDisplay: dict(label="display", forms="True", defaults=abi.DISPLAY_DEFAULTS, integers=("tone",), numbers=("gain", "white"),
                        checks=dict(gain=_POSITIVE, tone=(lambda v: v in abi.TONE_NAMES.values(), 'must be "clip", "reinhard" or "aces"'),
                                    reserved=_ZERO)),
    abi.RmAutoExposure: dict(label="auto exposure", forms="True", defaults=abi.AUTO_EXPOSURE_DEFAULTS,
                             numbers=("key", "low", "high", "min_gain", "max_gain"),
                             checks=dict(key=_POSITIVE, low=(lambda v: 0.0 <= v < 1.0, "must be in [0, 1)"), high=(lambda v: 0.0 < v <= 1.0, "must be in (0, 1]"),
                                         min_gain=_POSITIVE, max_gain=_POSITIVE, reserved=_ZERO)),
}


def _params(struct, params):
    """The block `struct` from None / True / its mode's name (the defaults), a dict of some of its fields over the defaults, or a
    `struct`, which is returned as it is; checked as the library checks it: ValueError otherwise."""
    b = _BLOCKS[struct]
    label, mode = b["label"], b.get("mode")
    if isinstance(params, struct):
        p = params
    else:
        if params is None or params is True or (mode is not None and params == mode):
            fields = {}
        elif isinstance(params, dict):
            fields = dict(params)
            if mode is not None and fields.pop("mode", mode) != mode:
                raise ValueError(f"{label}: mode {params['mode']!r} is not the {mode}-guided filter")
        else:
            raise ValueError(f"{label}: expected {b['forms']}, a dict or abi.{struct.__name__}, got {params!r}")
        unknown = set(fields) - set(b["defaults"])
        if unknown:
            raise ValueError(f"{label}: unknown parameter(s) {sorted(unknown)}; known: {sorted(b['defaults'])}")
        fields = {**b["defaults"], **fields}
        for name in b.get("integers", ()):
            if isinstance(fields[name], bool):
                fields[name] = int(fields[name])
            if not isinstance(fields[name], (int, np.integer)):
                raise ValueError(f"{label}: {name} must be an integer")
        for name in b.get("numbers", ()):
            if isinstance(fields[name], bool) or not isinstance(fields[name], (int, float, np.integer, np.floating)):
                raise ValueError(f"{label}: {name} must be a number")
        p = struct(**fields)
    for name, (holds, text) in b["checks"].items():
        if not holds(getattr(p, name)):
            raise ValueError(f"{label}: {name} {text}")
    return p


def denoise_params(params=None) -> abi.RmDenoise:
    """An abi.RmDenoise from None / True (the defaults, rm_denoise_default), a dict of some of its fields over the defaults, or an
    abi.RmDenoise.  Checked here as the library checks it (iterations in 0..8, every sigma finite and > 0): ValueError otherwise."""
    return _params(abi.RmDenoise, params)


def denoise_variance_params(params=None) -> abi.RmDenoiseVariance:
    """An abi.RmDenoiseVariance from None / True / "variance" (the defaults, rm_denoise_variance_default), a dict of some of its
    fields over the defaults (a "mode": "variance" entry allowed), or an abi.RmDenoiseVariance.  Checked as the library checks it
    (iterations in 0..8, every sigma finite and > 0, reserved 0): ValueError otherwise."""
    return _params(abi.RmDenoiseVariance, params)


def denoise_mode(denoise):
    """The filter a present's `denoise` asks for: ("variance", abi.RmDenoiseVariance) for "variance", an abi.RmDenoiseVariance or
    a dict with "mode": "variance"; ("atrous", abi.RmDenoise) for every form denoise_params takes, and a dict with
    "mode": "atrous"."""
    if isinstance(denoise, abi.RmDenoiseVariance) or (isinstance(denoise, str) and denoise == "variance") or \
            (isinstance(denoise, dict) and denoise.get("mode") == "variance"):
        return "variance", denoise_variance_params(denoise)
    if isinstance(denoise, dict) and "mode" in denoise:
        if denoise["mode"] != "atrous":
            raise ValueError(f"denoise: unknown mode {denoise['mode']!r} (\"atrous\" or \"variance\")")
        denoise = {k: v for k, v in denoise.items() if k != "mode"}
    return "atrous", denoise_params(denoise)


def despeckle_params(params=None) -> abi.RmDespeckle:
    """An abi.RmDespeckle from None / True (the defaults, rm_filters_default's), a dict of some of its fields over the defaults, or
    an abi.RmDespeckle.  Checked here as the library checks it (radius 1 or 2, rank in 0..3, gain finite and >= 1, floor finite and
    >= 0, reserved 0): ValueError otherwise."""
    return _params(abi.RmDespeckle, params)


def filters(despeckle=None, denoise=None) -> abi.RmFilters:
    """The abi.RmFilters of a chain: `despeckle` None (stage off) or what despeckle_params takes, `denoise` None (stage off) or what
    denoise_mode takes.  The blocks of a stage that is off keep their defaults (rm_filters_default)."""
    f = abi.RmFilters()
    load_library().rm_filters_default(C.byref(f))
    if despeckle is not None:
        f.despeckle, f.despeckle_params = 1, despeckle_params(despeckle)
    if denoise is not None:
        mode, p = denoise_mode(denoise)
        if mode == "variance":
            f.denoise, f.variance = abi.RM_DENOISE_VARIANCE, p
        else:
            f.denoise, f.atrous = abi.RM_DENOISE_ATROUS, p
    return f


def display_params(display=None) -> abi.RmDisplay:
    """An abi.RmDisplay from None / True (the defaults, rm_display_default: gain 1, the hard clip), a dict of some of its fields over
    the defaults -- `tone` as "clip" / "reinhard" / "aces" or its RM_TONE_* value -- or an abi.RmDisplay.  Checked here as the
    library checks it (gain finite and > 0, a known tone, white finite and > 0 for "reinhard", reserved 0): ValueError otherwise."""
    if isinstance(display, dict) and isinstance(display.get("tone"), str):
        if display["tone"] not in abi.TONE_NAMES:
            raise ValueError(f"display: unknown tone {display['tone']!r}; known: {sorted(abi.TONE_NAMES)}")
        display = {**display, "tone": abi.TONE_NAMES[display["tone"]]}
    p = _params(abi.RmDisplay, display)
    if p.tone == abi.RM_TONE_REINHARD and not _POSITIVE[0](p.white):
        raise ValueError(f"display: white {_POSITIVE[1]}")
    return p


def auto_exposure_params(params=None) -> abi.RmAutoExposure:
    """An abi.RmAutoExposure from None / True (rm_auto_exposure_default's values), a dict of some of its fields over them, or an
    abi.RmAutoExposure; checked as rm_stats_exposure checks it: ValueError otherwise."""
    p = _params(abi.RmAutoExposure, params)
    if not p.low < p.high:
        raise ValueError("auto exposure: low must be below high")
    if not p.min_gain <= p.max_gain:
        raise ValueError("auto exposure: min_gain must not exceed max_gain")
    return p


def display_is_auto(display) -> bool:
    """True for the forms of `display` whose gain comes from the frame's statistics: "auto", or a dict with an "auto" entry."""
    return (isinstance(display, str) and display == "auto") or (isinstance(display, dict) and "auto" in display)


class FrameStats:
    """An abi.RmFrameStats (rm_frame_stats): `hist` is a numpy view of its 512 bins, the other fields are attributes; the statistics
    of the parts of a frame add up (`+`: counts summed, min / max taken).  percentile and exposure are the library's host
    arithmetic (rm_stats_percentile, rm_stats_exposure)."""

    def __init__(self, raw: Optional[abi.RmFrameStats] = None):
        self.raw = raw if raw is not None else abi.RmFrameStats(min_l=math.inf, max_l=-math.inf)

    pixels = property(lambda self: int(self.raw.pixels))
    below = property(lambda self: int(self.raw.below))
    above = property(lambda self: int(self.raw.above))
    non_finite = property(lambda self: int(self.raw.non_finite))
    min = property(lambda self: float(self.raw.min_l))
    max = property(lambda self: float(self.raw.max_l))

    @property
    def hist(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.raw.hist)

    def __add__(self, other: "FrameStats") -> "FrameStats":
        if not isinstance(other, FrameStats):
            return NotImplemented
        r = abi.RmFrameStats()
        for name in ("pixels", "below", "above", "non_finite"):
            setattr(r, name, getattr(self.raw, name) + getattr(other.raw, name))
        r.min_l, r.max_l = min(self.raw.min_l, other.raw.min_l), max(self.raw.max_l, other.raw.max_l)
        out = FrameStats(r)
        out.hist[:] = self.hist + other.hist
        return out

    def percentile(self, q: float) -> float:
        """hi_b of the bin that holds the ceil(q N)-th smallest binned pixel (0 when nothing is binned)."""
        l = C.c_float()
        if load_library().rm_stats_percentile(C.byref(self.raw), float(q), C.byref(l)) != abi.RM_OK:
            raise ValueError(f"percentile: q must be in [0, 1], not {q!r}")
        return float(l.value)

    def exposure(self, **fields) -> float:
        """The gain that brings the log-average luminance between the `low` and `high` percentiles to `key` (rm_stats_exposure;
        fields left out take rm_auto_exposure_default's values)."""
        p = auto_exposure_params(fields or None)
        g = C.c_float()
        if load_library().rm_stats_exposure(C.byref(self.raw), C.byref(p), C.byref(g)) != abi.RM_OK:
            raise ValueError("exposure: refused by rm_stats_exposure")
        return float(g.value)


def cull_cell(scene, centre, radius: float, margin: float = 0.0):
    """Rows of a primitive table that an evaluation anywhere in the ball (centre, radius) has to fold: a bool per row
    (rm_debug_cull_cell -- the rule behind the culling grid of the fast build; host arithmetic, no GPU)."""
    lib = load_library()
    desc = scene.desc()
    words = (desc.nprims + 63) // 64
    out = (C.c_ulonglong * words)()
    c = (C.c_double * 3)(*[float(v) for v in centre])
    rc = lib.rm_debug_cull_cell(C.byref(desc), c, float(radius), float(margin), out)
    if rc != abi.RM_OK:
        raise RmError(rc, "rm_debug_cull_cell: not a table of shapes only")
    return [bool((out[i >> 6] >> (i & 63)) & 1) for i in range(desc.nprims)]


class RmError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


_lib = None
_libs: dict = {}
# the tests' cross-check build of the same sources (build.py build_crosscheck): the library plus the wavefront pipeline.  NOT what a
# host loads: Context(library=XCHECK_LIB_PATH) is for tests/ and the tools that time both implementations.
XCHECK_LIB_PATH = Path(__file__).resolve().parent.parent / "tests" / "_xcheck" / "libhip_raymarch_xcheck.so"


def _share_torch_hip_runtime():
    """One HIP/HSA runtime per process.  PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 (same sonames as
    /opt/rocm's); if this library pulls in /opt/rocm's copies first and torch initialises its own afterwards, the
    second HSA runtime finds no GPU ("No HIP GPUs are available").  When torch is installed, load ITS runtime first:
    libhip_raymarch.so then binds to it by soname, whichever of the two is imported first.  Hosts without torch (the
    Node addon) use /opt/rocm's."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return  # torch's runtime is already in the process
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = Path(list(spec.submodule_search_locations)[0]) / "lib"
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        p = libdir / name
        if p.exists():
            try:
                C.CDLL(str(p), mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load_library(path=None):
    """dlopen the HIP library (loading needs no GPU; creating a context does).  `path`: another build of the same library (the
    tests' cross-check build); default = the product."""
    global _lib
    path = Path(path) if path is not None else LIB_PATH
    if str(path) in _libs:
        return _libs[str(path)]
    if not path.exists():
        raise RmError(abi.RM_ERR_DEVICE, f"{path} is missing: build it with `python raymarching-engine_amd/build.py` "
                                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _share_torch_hip_runtime()
    lib = C.CDLL(str(path))
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.c_int
    sig = {
        "rm_abi_version": (ip, []),
        "rm_material_default": (None, [C.POINTER(abi.RmMaterial)]),
        "rm_ctx_create": (ip, [ip, C.POINTER(vp)]),
        "rm_ctx_destroy": (None, [vp]),
        "rm_last_error": (C.c_char_p, [vp]),
        "rm_ctx_set_stream": (ip, [vp, vp]),
        "rm_ctx_set_retire_eps": (ip, [vp, C.c_float]),
        "rm_ctx_set_samples_in_flight": (ip, [vp, C.c_int]),
        "rm_ctx_last_warning": (C.c_char_p, [vp]),
        "rm_ctx_set_sample_batch": (ip, [vp, C.c_int]),
        "rm_ctx_set_gl_stack": (ip, [vp, C.c_int]),
        "rm_device_memory": (ip, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "rm_buffer_create": (ip, [vp, C.c_size_t, C.POINTER(C.c_void_p)]),
        "rm_buffer_destroy": (ip, [vp, vp]),
        "rm_buffer_download": (ip, [vp, vp, vp, C.c_size_t]),
        "rm_buffer_upload": (ip, [vp, vp, vp, C.c_size_t]),
        "rm_ctx_set_cost_order": (ip, [vp, C.c_int]),
        "rm_ctx_set_cull_min_pixels": (ip, [vp, C.c_longlong]),
        "rm_ctx_set_cull_budget": (ip, [vp, C.c_size_t]),
        "rm_ctx_cull_stats": (ip, [vp, C.POINTER(C.c_ulonglong)]),
        "rm_debug_counters": (ip, [vp, C.POINTER(C.c_ulonglong), ip]),
        "rm_debug_cull_cell": (ip, [C.POINTER(abi.RmSceneDesc), C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_ulonglong)]),
        "rm_sync": (ip, [vp]),
        "rm_scene_create": (ip, [vp, C.POINTER(abi.RmSceneDesc), C.POINTER(vp)]),
        "rm_scene_destroy": (None, [vp]),
        "rm_fb_create": (ip, [vp, ip, ip, ip, ip, C.POINTER(vp)]),
        "rm_fb_wrap": (ip, [vp, ip, ip, ip, ip, vp, vp, vp, C.POINTER(vp)]),
        "rm_fb_create_striped": (ip, [vp, ip, ip, ip, ip, ip, vp, vp, vp, C.POINTER(vp)]),
        "rm_fb_rows": (ip, [vp]),
        "rm_fb_width": (ip, [vp]),
        "rm_fb_height": (ip, [vp]),
        "rm_fb_clear": (ip, [vp]),
        "rm_fb_destroy": (None, [vp]),
        "rm_fb_download": (ip, [vp, ip, fp]),
        "rm_fb_upload": (ip, [vp, ip, fp]),
        "rm_fb_device_ptr": (vp, [vp, ip]),
        "rm_fb_create_fmt": (ip, [vp, ip, ip, ip, ip, ip, C.POINTER(vp)]),
        "rm_fb_wrap_fmt": (ip, [vp, ip, ip, ip, ip, vp, vp, vp, ip, C.POINTER(vp)]),
        "rm_fb_create_striped_fmt": (ip, [vp, ip, ip, ip, ip, ip, vp, vp, vp, ip, C.POINTER(vp)]),
        "rm_fb_gbuffer": (ip, [vp]),
        "rm_fb_download_raw": (ip, [vp, ip, vp, C.c_size_t]),
        "rm_fb_upload_raw": (ip, [vp, ip, vp, C.c_size_t]),
        "rm_render_sample": (ip, [vp, vp, vp, C.POINTER(abi.RmUniforms), C.POINTER(abi.RmRect), ip]),
        "rm_render_samples": (ip, [vp, vp, vp, C.POINTER(abi.RmUniforms), fp, ip, C.POINTER(abi.RmRect), ip]),
        "rm_render_timed": (ip, [vp, vp, vp, C.POINTER(abi.RmUniforms), ip, C.POINTER(abi.RmRect), ip, fp]),
        "rm_probe": (ip, [vp, vp, ip, fp, ip, C.c_float, ip, fp]),
        "rm_probe_camera": (ip, [vp, C.POINTER(abi.RmUniforms), ip, ip, fp]),
        "rm_probe_rng": (ip, [vp, C.POINTER(abi.RmUniforms), ip, ip, ip, fp]),
        "rm_probe_math": (ip, [vp, ip, fp, fp, ip, fp]),
        "rm_assemble_striped": (ip, [vp, vp, ip, ip, ip, ip, ip, vp, vp]),
        "rm_assemble_striped_bytes": (ip, [vp, vp, ip, ip, C.c_longlong, ip, ip, vp, vp]),
        "rm_present_device": (ip, [vp, vp, vp, ip, ip, ip, vp, vp]),
        "rm_present_rows": (ip, [vp, vp, ip, vp, vp]),
        "rm_pack_present_rows": (ip, [vp, vp, vp, vp]),
        "rm_ctx_last_pipeline": (ip, [vp]),
        "rm_present_sharded": (ip, [C.POINTER(vp), C.POINTER(vp), ip, ip, ip, C.POINTER(C.c_uint8), C.c_size_t]),
        "rm_present_sharded_start": (ip, [C.POINTER(vp), C.POINTER(vp), ip, ip, ip]),
        "rm_present_sharded_finish": (ip, [C.POINTER(vp), ip, C.POINTER(C.c_uint8), C.c_size_t]),
        "rm_present_striped_rows": (ip, [vp, vp, vp, ip, ip, ip, ip, ip, ip, vp, vp]),
        "rm_present": (ip, [vp, vp, ip, C.POINTER(C.c_uint8)]),
        "rm_present_planes": (ip, [vp, vp, vp, ip, ip, ip, C.POINTER(C.c_uint8)]),
        "rm_denoise_default": (None, [C.POINTER(abi.RmDenoise)]),
        "rm_denoise": (ip, [vp, vp, ip, C.POINTER(abi.RmDenoise), fp]),
        "rm_denoise_device": (ip, [vp, vp, ip, C.POINTER(abi.RmDenoise), vp, vp]),
        "rm_present_denoised": (ip, [vp, vp, ip, C.POINTER(abi.RmDenoise), C.POINTER(C.c_uint8)]),
        "rm_fb_has_moments": (ip, [vp]),
        "rm_denoise_variance_default": (None, [C.POINTER(abi.RmDenoiseVariance)]),
        "rm_denoise_variance": (ip, [vp, vp, ip, C.POINTER(abi.RmDenoiseVariance), fp]),
        "rm_denoise_variance_device": (ip, [vp, vp, ip, C.POINTER(abi.RmDenoiseVariance), vp, vp]),
        "rm_present_denoised_variance": (ip, [vp, vp, ip, C.POINTER(abi.RmDenoiseVariance), C.POINTER(C.c_uint8)]),
        "rm_filters_default": (None, [C.POINTER(abi.RmFilters)]),
        "rm_filter": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), fp]),
        "rm_filter_device": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), vp, vp]),
        "rm_present_filtered": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), C.POINTER(C.c_uint8)]),
        "rm_frame_stats": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), C.POINTER(abi.RmFrameStats)]),
        "rm_auto_exposure_default": (None, [C.POINTER(abi.RmAutoExposure)]),
        "rm_stats_percentile": (ip, [C.POINTER(abi.RmFrameStats), C.c_double, fp]),
        "rm_stats_exposure": (ip, [C.POINTER(abi.RmFrameStats), C.POINTER(abi.RmAutoExposure), fp]),
        "rm_display_default": (None, [C.POINTER(abi.RmDisplay)]),
        "rm_present_display": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), C.POINTER(abi.RmDisplay), C.POINTER(C.c_uint8)]),
        "rm_present_display_device": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), C.POINTER(abi.RmDisplay), vp, vp]),
        "rm_present_linear": (ip, [vp, vp, ip, C.POINTER(abi.RmFilters), C.POINTER(abi.RmDisplay), fp]),
        "rm_grid_axis": (ip, [C.POINTER(abi.RmGrid), ip, fp]),
        "rm_sdf_grid": (ip, [vp, vp, C.POINTER(abi.RmGrid), ip, fp]),
        "rm_sdf_grid_device": (ip, [vp, vp, C.POINTER(abi.RmGrid), ip, vp, vp]),
        "rm_mesh_params_default": (None, [C.POINTER(abi.RmMeshParams)]),
        "rm_mesh_extract": (ip, [vp, vp, C.POINTER(abi.RmGrid), C.POINTER(abi.RmMeshParams), C.POINTER(vp)]),
        "rm_mesh_from_values": (ip, [vp, C.POINTER(abi.RmGrid), fp, C.c_float, C.POINTER(vp)]),
        "rm_mesh_counts": (ip, [vp, C.POINTER(C.c_ulonglong)]),
        "rm_mesh_timings": (ip, [vp, fp]),
        "rm_mesh_download": (ip, [vp, ip, vp, C.c_size_t]),
        "rm_mesh_device_ptr": (vp, [vp, ip]),
        "rm_mesh_destroy": (None, [vp]),
        "rm_mesh_sharp_default": (None, [C.POINTER(abi.RmMeshSharp)]),
        "rm_mesh_extract_sharp": (ip, [vp, vp, C.POINTER(abi.RmGrid), C.POINTER(abi.RmMeshParams), C.POINTER(abi.RmMeshSharp), C.POINTER(vp)]),
        "rm_mesh_keep_default": (None, [C.POINTER(abi.RmMeshKeep)]),
        "rm_mesh_components": (ip, [vp, C.POINTER(C.c_ulonglong)]),
        "rm_mesh_components_download": (ip, [vp, ip, vp, C.c_size_t]),
        "rm_mesh_filter": (ip, [vp, C.POINTER(abi.RmMeshKeep), C.POINTER(vp)]),
        "rm_mesh_simplify_default": (None, [C.POINTER(abi.RmMeshSimplify)]),
        "rm_mesh_simplify": (ip, [vp, C.POINTER(abi.RmGrid), C.POINTER(abi.RmMeshSimplify), C.POINTER(vp)]),
        "rm_mesh_quadric_default": (None, [C.POINTER(abi.RmMeshQuadric)]),
        "rm_mesh_simplify_quadric": (ip, [vp, C.POINTER(abi.RmGrid), C.POINTER(abi.RmMeshSimplify), C.POINTER(abi.RmMeshQuadric), C.POINTER(vp)]),
        "rm_mesh_occlusion_default": (None, [C.POINTER(abi.RmMeshOcclusion)]),
        "rm_mesh_occlusion_directions": (ip, [ip, fp]),
        "rm_mesh_occlusion": (ip, [vp, vp, C.POINTER(abi.RmMeshOcclusion), fp, fp]),
        "rm_mesh_measure": (ip, [vp, C.POINTER(abi.RmMeshMeasures), fp]),
        "rm_mesh_measure_components": (ip, [vp, vp, C.c_size_t]),
        "rm_mesh_slabs_default": (None, [C.POINTER(abi.RmMeshSlabs)]),
        "rm_mesh_extract_slabs": (ip, [vp, vp, C.POINTER(abi.RmGrid), C.POINTER(abi.RmMeshParams), C.POINTER(abi.RmMeshSlabs), C.POINTER(vp)]),
        "rm_mesh_extract_sharp_slabs": (ip, [vp, vp, C.POINTER(abi.RmGrid), C.POINTER(abi.RmMeshParams), C.POINTER(abi.RmMeshSharp), C.POINTER(abi.RmMeshSlabs),
                                             C.POINTER(vp)]),
        "rm_mesh_from_values_slabs": (ip, [vp, C.POINTER(abi.RmGrid), fp, C.c_float, C.POINTER(abi.RmMeshSlabs), C.POINTER(vp)]),
        "rm_mesh_project_default": (None, [C.POINTER(abi.RmMeshProject)]),
        "rm_mesh_project": (ip, [vp, vp, C.POINTER(abi.RmMeshProject), C.POINTER(vp), C.POINTER(abi.RmMeshProjection), fp]),
        "rm_mesh_deviation_default": (None, [C.POINTER(abi.RmMeshDeviation)]),
        "rm_mesh_deviation_weights": (ip, [ip, fp]),
        "rm_mesh_deviation": (ip, [vp, vp, C.POINTER(abi.RmMeshDeviation), C.POINTER(abi.RmMeshDeviationReport), fp, fp]),
        "rm_mesh_refine_default": (None, [C.POINTER(abi.RmMeshRefine)]),
        "rm_mesh_refine": (ip, [vp, vp, C.POINTER(abi.RmMeshRefine), C.POINTER(abi.RmMeshProject), C.POINTER(vp), C.POINTER(abi.RmMeshRefinement)]),
    }
    for name, (res, args) in sig.items():
        if name.startswith("rm_debug_") and not hasattr(lib, name) and os.environ.get("RM_LIB"):
            continue  # an experiment build of an older source tree (tools/): the debug entries are not part of what it measures
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _libs[str(path)] = lib
    if path == LIB_PATH:
        _lib = lib
    return lib


def present_sharded(contexts, framebuffers, samples: int, dof: bool) -> np.ndarray:
    """rm_present_sharded: the canvas [H, W, 4] of a frame whose stripes ONE process renders on several contexts (part p of
    len(contexts) on contexts[p]); the rows travel to contexts[0]'s GPU by peer copies."""
    n = len(contexts)
    assert n == len(framebuffers) and n >= 1
    cs = (C.c_void_p * n)(*[c.h for c in contexts])
    fs = (C.c_void_p * n)(*[f.h for f in framebuffers])
    out = np.empty((framebuffers[0].height, framebuffers[0].width, 4), np.uint8)
    contexts[0]._check(contexts[0].lib.rm_present_sharded(cs, fs, n, int(samples), 1 if dof else 0, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes))
    return out


def present_sharded_start(contexts, framebuffers, samples: int, dof: bool):
    """rm_present_sharded_start: snapshot and send; returns at once (the next samples can be handed out while the frame travels)."""
    n = len(contexts)
    assert n == len(framebuffers) and n >= 1
    cs = (C.c_void_p * n)(*[c.h for c in contexts])
    fs = (C.c_void_p * n)(*[f.h for f in framebuffers])
    contexts[0]._check(contexts[0].lib.rm_present_sharded_start(cs, fs, n, int(samples), 1 if dof else 0))


def present_sharded_finish(contexts, width: int, height: int) -> np.ndarray:
    """rm_present_sharded_finish: the canvas [H, W, 4] of the present that was started."""
    n = len(contexts)
    cs = (C.c_void_p * n)(*[c.h for c in contexts])
    out = np.empty((height, width, 4), np.uint8)
    contexts[0]._check(contexts[0].lib.rm_present_sharded_finish(cs, n, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes))
    return out


def scene_key(scene: Scene) -> bytes:
    """Cache key of a scene description (the reference keys its program cache
    by the source string, ShaderCache.tsx:91-119)."""
    d = scene.desc()
    prims = bytes(C.string_at(d.prims, C.sizeof(abi.RmPrim) * d.nprims)) if d.nprims else b""
    surfaces = bytes(C.string_at(d.surfaces, C.sizeof(abi.RmSurface) * d.nsurfaces)) if d.nsurfaces else b""
    return bytes([d.kind & 0xFF]) + bytes(d.params) + bytes(d.material) + prims + surfaces


def _fp(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_float))


class DeviceBuffer:
    """rm_buffer_*: `nbytes` of device memory owned by the library; .ptr is the device address."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        ctx._check(ctx.lib.rm_buffer_create(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def download(self, dtype=np.uint8) -> np.ndarray:
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        self.ctx._check(self.ctx.lib.rm_buffer_download(self.ctx.h, self.ptr, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.rm_buffer_upload(self.ctx.h, self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def destroy(self):
        if self.ptr:
            self.ctx._check(self.ctx.lib.rm_buffer_destroy(self.ctx.h, self.ptr))
            self.ptr = None


class Context:
    gl_stack_on = False

    def __init__(self, device: int = 0, library=None):
        self.lib = load_library(library)
        h = C.c_void_p()
        rc = self.lib.rm_ctx_create(device, C.byref(h))
        if rc != abi.RM_OK:
            raise RmError(rc, self.lib.rm_last_error(None).decode())
        self.h = h
        self.device = device
        self.settings = {}  # setter name -> arguments, as last called: what a second context needs to behave like this one (tests)

    def _check(self, rc: int):
        if rc != abi.RM_OK:
            raise RmError(rc, self.lib.rm_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.rm_ctx_destroy(self.h)
            self.h = None

    def set_stream(self, hip_stream: Optional[int]):
        """A hipStream_t (as an integer) for all later launches; None = the context's own stream.  torch's DEFAULT
        stream has the handle 0 (the NULL stream), which cannot be told from None here and with which the context's
        own non-blocking stream is not ordered: give torch work that shares buffers with the renders a stream of its own
        (torch.cuda.Stream) and pass that one."""
        if hip_stream is not None and int(hip_stream) == 0:
            raise RmError(abi.RM_ERR_INVALID, "set_stream(0): the NULL stream is not supported; use a torch.cuda.Stream() "
                                              "(or None for the context's own stream)")
        self._check(self.lib.rm_ctx_set_stream(self.h, C.c_void_p(hip_stream or 0)))

    def set_samples_in_flight(self, n: int):
        """Consecutive full-mode samples that may overlap on the GPU (1 = none); the planes get the same bits."""
        self.settings["set_samples_in_flight"] = (n,)
        self._check(self.lib.rm_ctx_set_samples_in_flight(self.h, int(n)))
        note = self.lib.rm_ctx_last_warning(self.h).decode()
        if note.startswith("warning:"):  # accepted, but the process environment will keep the samples from overlapping
            import warnings

            warnings.warn(note)

    def device_memory(self):
        """(free, total) bytes of the context's GPU."""
        f, t = C.c_size_t(), C.c_size_t()
        self._check(self.lib.rm_device_memory(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def buffer(self, nbytes: int) -> "DeviceBuffer":
        """Zero-filled raw device memory (for rm_present_rows / rm_assemble_striped_bytes on hosts without torch)."""
        return DeviceBuffer(self, nbytes)

    def set_gl_stack(self, on: bool):
        """Parity mode: strict-flag renders, probes and presents in the arithmetic of the GL stack the goldens were
        rendered under (include/hip_raymarch.h rm_ctx_set_gl_stack)."""
        self._check(self.lib.rm_ctx_set_gl_stack(self.h, int(on)))  # True / 1: on; 2: on, with the stack's own tan
        self.gl_stack_on = bool(on)

    def set_sample_batch(self, n: int):
        """Samples per launch of render_samples (0 = automatic, 1 = one launch per sample, up to 8); same bits."""
        self.settings["set_sample_batch"] = (n,)
        self._check(self.lib.rm_ctx_set_sample_batch(self.h, int(n)))

    def assemble_striped(self, src_ptr: int, parts: int, max_rows: int, width: int, height: int, stripe_rows: int, dst_ptr: int,
                         stream: Optional[int] = None):
        """Gathered striped windows (device pointer, parts x max_rows x width float4) -> the frame in image order,
        on `stream` (a hipStream_t as an integer) or the context's stream."""
        self._check(self.lib.rm_assemble_striped(self.h, C.c_void_p(src_ptr), parts, max_rows, width, height, stripe_rows, C.c_void_p(dst_ptr),
                                                 C.c_void_p(stream) if stream else None))

    def assemble_striped_bytes(self, src_ptr: int, parts: int, max_rows: int, row_bytes: int, height: int, stripe_rows: int, dst_ptr: int,
                               stream: Optional[int] = None):
        """assemble_striped for rows of opaque bytes (RGBA8 after present_rows: row_bytes = 4 * width)."""
        self._check(self.lib.rm_assemble_striped_bytes(self.h, C.c_void_p(src_ptr), parts, max_rows, int(row_bytes), height, stripe_rows,
                                                       C.c_void_p(dst_ptr), C.c_void_p(stream) if stream else None))

    def present_device(self, color_ptr: int, normal_dof_ptr: Optional[int], width: int, height: int, samples: int, out_ptr: int,
                       stream: Optional[int] = None):
        """display.frag into DEVICE memory (height*width*4 bytes), asynchronous."""
        self._check(self.lib.rm_present_device(self.h, C.c_void_p(color_ptr), C.c_void_p(normal_dof_ptr or 0), width, height, int(samples),
                                               C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def present_striped_rows(self, color_ptr: int, normal_dof_ptr: Optional[int], width: int, height: int, samples: int, stripe_rows: int, parts: int,
                             part: int, out_ptr: int, stream: Optional[int] = None):
        """display.frag for the rows part `part` of `parts` holds, read from the WHOLE frame in DEVICE memory, into DEVICE memory
        (that part's packed rows x width x 4 bytes), asynchronous: each rank's share of a sharded frame's blur."""
        self._check(self.lib.rm_present_striped_rows(self.h, C.c_void_p(color_ptr), C.c_void_p(normal_dof_ptr or 0), width, height, int(samples), stripe_rows,
                                                     parts, part, C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def denoise_device(self, fb: "Framebuffer", samples: int, out_ptr: int, params=None, stream: Optional[int] = None):
        """rm_denoise_device: Framebuffer.denoise into rows x W float4 of device memory at out_ptr, enqueued on `stream` (None =
        the context's); no host wait."""
        p = denoise_params(params)
        self._check(self.lib.rm_denoise_device(self.h, fb.h, int(samples), C.byref(p), C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def denoise_variance_device(self, fb: "Framebuffer", samples: int, out_ptr: int, params=None, stream: Optional[int] = None):
        """rm_denoise_variance_device: Framebuffer.denoise_variance into rows x W float4 of device memory at out_ptr, enqueued on
        `stream` (None = the context's); no host wait."""
        p = denoise_variance_params(params)
        self._check(self.lib.rm_denoise_variance_device(self.h, fb.h, int(samples), C.byref(p), C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def filter_device(self, fb: "Framebuffer", samples: int, out_ptr: int, despeckle=None, denoise=None, stream: Optional[int] = None):
        """rm_filter_device: Framebuffer.filter into rows x W float4 of device memory at out_ptr, enqueued on `stream` (None = the
        context's); no host wait."""
        f = filters(despeckle, denoise)
        self._check(self.lib.rm_filter_device(self.h, fb.h, int(samples), C.byref(f), C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def present_display_device(self, fb: "Framebuffer", samples: int, out_ptr: int, denoise=None, despeckle=None, display=None,
                               stream: Optional[int] = None):
        """rm_present_display_device: Framebuffer.present(..., display=...) into rows x W x 4 bytes of device memory at out_ptr,
        enqueued on `stream` (None = the context's); no host wait."""
        d = fb.display_block(samples, denoise, despeckle, display)
        f = filters(despeckle, denoise)
        self._check(self.lib.rm_present_display_device(self.h, fb.h, int(samples), C.byref(f), C.byref(d), C.c_void_p(out_ptr),
                                                       C.c_void_p(stream) if stream else None))

    def present_rows(self, fb: "Framebuffer", samples: int, out_ptr: int, stream: Optional[int] = None):
        """Tone-map the rows `fb` holds (no depth of field) into DEVICE memory (rows*width*4 bytes), asynchronous."""
        self._check(self.lib.rm_present_rows(self.h, fb.h, int(samples), C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def pack_present_rows(self, fb: "Framebuffer", out_ptr: int, stream: Optional[int] = None):
        """(colour.rgb, normal_dof.w) of the rows `fb` holds into DEVICE memory (rows*width float4), asynchronous: what a
        sharded job with depth of field gathers; assembled, it is both planes of present_device."""
        self._check(self.lib.rm_pack_present_rows(self.h, fb.h, C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def last_pipeline(self) -> str:
        """Which implementation the last render call dispatched: "megakernel" (the pixel kernel) or "wavefront"."""
        return {abi.RM_PIPELINE_PIXEL_KERNEL: "megakernel", abi.RM_PIPELINE_WAVEFRONT: "wavefront"}.get(int(self.lib.rm_ctx_last_pipeline(self.h)), "none")

    def set_cost_order(self, on: bool):
        """Start the tiles of a job most-expensive-first by their cost in the previous sample (scheduling only)."""
        self.settings["set_cost_order"] = (on,)
        self._check(self.lib.rm_ctx_set_cost_order(self.h, 1 if on else 0))

    def set_cull_min_pixels(self, pixels: int):
        """Pixel-samples a scene has to be asked for before its culling grid is built (0: with the first render; same bits)."""
        self.settings["set_cull_min_pixels"] = (pixels,)
        self._check(self.lib.rm_ctx_set_cull_min_pixels(self.h, int(pixels)))

    def set_cull_budget(self, nbytes: int):
        """The bytes this context's culling grids may hold together (default: a sixteenth of the device's memory, at most 1 GiB)."""
        self.settings["set_cull_budget"] = (nbytes,)
        self._check(self.lib.rm_ctx_set_cull_budget(self.h, int(nbytes)))

    def cull_stats(self) -> dict:
        out = (C.c_ulonglong * 4)()
        self._check(self.lib.rm_ctx_cull_stats(self.h, out))
        return dict(built=int(out[0]), bytes=int(out[1]), grids=int(out[2]), budget=int(out[3]))

    def set_retire_eps(self, eps: float):
        self.settings["set_retire_eps"] = (eps,)
        self._check(self.lib.rm_ctx_set_retire_eps(self.h, float(eps)))

    def debug_counters(self, reset: bool = True):
        out = (C.c_ulonglong * 16)()
        self._check(self.lib.rm_debug_counters(self.h, out, 1 if reset else 0))
        return list(out)

    def sync(self):
        self._check(self.lib.rm_sync(self.h))

    def create_scene(self, scene: Scene) -> "SceneHandle":
        return SceneHandle(self, scene)

    def create_framebuffer(self, width: int, height: int, row_begin: int = 0, row_count: Optional[int] = None, gbuffer: str = "f32",
                           moments: bool = False) -> "Framebuffer":
        """gbuffer: "f32" (default) or "f16", the reference's half-precision normal + DoF radius and albedo + depth planes.
        moments: also keep the per-pixel luminance moments plane (RM_FB_MOMENTS) the variance-guided denoiser reads."""
        return Framebuffer(self, width, height, row_begin, height if row_count is None else row_count, gbuffer=gbuffer, moments=moments)

    def create_striped_framebuffer(self, width, height, stripe_rows, parts, part, color_ptr=None, normal_ptr=None, albedo_ptr=None,
                                   gbuffer: str = "f32") -> "Framebuffer":
        """Rows r with (r // stripe_rows) % parts == part, packed (row sharding across GPUs)."""
        return Framebuffer(self, width, height, 0, 0, striped=(stripe_rows, parts, part, color_ptr, normal_ptr, albedo_ptr), gbuffer=gbuffer)

    def wrap_framebuffer(self, width, height, row_begin, row_count, color_ptr, normal_ptr=None, albedo_ptr=None, gbuffer: str = "f32") -> "Framebuffer":
        return Framebuffer(self, width, height, row_begin, row_count, wrap=(color_ptr, normal_ptr, albedo_ptr), gbuffer=gbuffer)

    def render_sample(self, scene: "SceneHandle", fb: "Framebuffer", uniforms: abi.RmUniforms, tile: Optional[abi.RmRect] = None,
                      flags: int = abi.RM_RENDER_STRICT):
        self._check(self.lib.rm_render_sample(self.h, scene.h, fb.h, C.byref(uniforms), C.byref(tile) if tile is not None else None, flags))

    def render_samples(self, scene, fb, uniforms, rand_noise_pairs, tile=None, flags=abi.RM_RENDER_STRICT):
        rn = np.ascontiguousarray(rand_noise_pairs, np.float32).reshape(-1, 2)
        self._check(self.lib.rm_render_samples(self.h, scene.h, fb.h, C.byref(uniforms), _fp(rn), len(rn),
                                               C.byref(tile) if tile is not None else None, flags))

    def render_timed(self, scene, fb, uniforms, count: int, tile=None, flags=abi.RM_RENDER_STRICT) -> float:
        ms = C.c_float(0.0)
        self._check(self.lib.rm_render_timed(self.h, scene.h, fb.h, C.byref(uniforms), count,
                                             C.byref(tile) if tile is not None else None, flags, C.byref(ms)))
        return float(ms.value)

    def probe(self, scene: "SceneHandle", what: int, inputs: np.ndarray, param: float = 0.0, flags: int = abi.RM_RENDER_STRICT) -> np.ndarray:
        in_w = {abi.RM_PROBE_SDF: 3, abi.RM_PROBE_CAST_RAY: 6, abi.RM_PROBE_NORMAL: 3, abi.RM_PROBE_MATERIAL: 3, abi.RM_PROBE_CAST_STEPS: 6, abi.RM_PROBE_CAST_SHADOW: 9}[what]
        out_w = {abi.RM_PROBE_SDF: 1, abi.RM_PROBE_CAST_RAY: 3, abi.RM_PROBE_NORMAL: 3, abi.RM_PROBE_MATERIAL: 12, abi.RM_PROBE_CAST_STEPS: 1, abi.RM_PROBE_CAST_SHADOW: 1}[what]
        a = np.ascontiguousarray(inputs, np.float32).reshape(-1, in_w)
        out = np.empty((len(a), out_w), np.float32)
        self._check(self.lib.rm_probe(self.h, scene.h, what, _fp(a), len(a), float(param), flags, _fp(out)))
        return out[:, 0] if out_w == 1 else out

    def sdf_grid(self, scene: "SceneHandle", grid, flags: int = abi.RM_RENDER_STRICT) -> np.ndarray:
        """The scene's distance at every corner of `grid` (mesh.Grid), float32 [nz + 1, ny + 1, nx + 1]: what probe(RM_PROBE_SDF) gives
        at the corners' positions with the same flags, bit for bit (rm_sdf_grid)."""
        g = grid.to_c()
        out = np.empty(grid.shape, np.float32)
        self._check(self.lib.rm_sdf_grid(self.h, scene.h, C.byref(g), int(flags), _fp(out)))
        return out

    def sdf_grid_device(self, scene: "SceneHandle", grid, out_ptr: int, flags: int = abi.RM_RENDER_STRICT, stream: Optional[int] = None):
        """rm_sdf_grid_device: sdf_grid into grid.corners floats of device memory at out_ptr, enqueued on `stream` (None = the
        context's); no allocation, no host wait."""
        g = grid.to_c()
        self._check(self.lib.rm_sdf_grid_device(self.h, scene.h, C.byref(g), int(flags), C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def _take_mesh(self, handle, grid, normals=False, colours=False, keep=None, components=False, simplify=None, quadric=None, scene=None, occlusion=None, measures=False,
                   project=None, deviation=None, refine=None):
        """The arrays of a mesh handle as a mesh.Mesh (normals / colours: whether the call that made it asked for them); destroys the handle.
        simplify (_mesh_simplify's triple): the mesh is first clustered on the device (rm_mesh_simplify) and the Mesh's grid is the cluster grid,
        which its cells then index -- with quadric (an abi.RmMeshQuadric) by rm_mesh_simplify_quadric; keep (an abi.RmMeshKeep): that mesh is filtered on the device (rm_mesh_filter), which also removes the vertices
        simplification left without triangles; the last of them is what is downloaded.  components: its labels and component sizes come with it.
        occlusion (an abi.RmMeshOcclusion, with the scene): that last mesh's ambient occlusion comes with it (rm_mesh_occlusion), and the
        timings gain "occlusion", the milliseconds of its probes and taps.  measures: that last mesh is measured before anything is downloaded
        (rm_mesh_measure, rm_mesh_measure_components): Mesh.measures, and the timings gain "measures", the milliseconds of topology and geometry.
        project (_mesh_project's function of the grid the mesh lies on, with the scene): behind simplify and keep, that mesh's vertices are
        projected onto the scene's level set (rm_mesh_project) and everything after sees the projected mesh: Mesh.projection, Mesh.residual,
        and the timings gain "projection", the milliseconds of its rounds and its normals; sampling, meshing and attributes stay those of the
        mesh that was projected, so nothing is counted twice.  deviation (an abi.RmMeshDeviation, with the scene): how far the triangles of
        the mesh that is returned lie off the scene's level set (rm_mesh_deviation): Mesh.deviation, Mesh.triangle_deviation, and the timings
        gain "deviation", the milliseconds of its evaluation and its reduction.  refine (_mesh_refine's function of the grid the mesh lies on, with
        the scene): behind project, that mesh's chording edges are split on the device (rm_mesh_refine) and everything after sees the refined
        mesh: Mesh.refinement, and the timings gain "refinement", the milliseconds of its split rounds, its projections and its normals."""
        from .mesh import Mesh

        handles = [handle]
        try:
            if simplify is not None:
                grid, clusters, params = simplify
                simplified = C.c_void_p()
                if quadric is None:
                    self._check(self.lib.rm_mesh_simplify(handle, C.byref(clusters), C.byref(params), C.byref(simplified)))
                else:
                    self._check(self.lib.rm_mesh_simplify_quadric(handle, C.byref(clusters), C.byref(params), C.byref(quadric), C.byref(simplified)))
                handles.append(simplified)
                handle = simplified
            if keep is not None:
                filtered = C.c_void_p()
                self._check(self.lib.rm_mesh_filter(handle, C.byref(keep), C.byref(filtered)))
                handles.append(filtered)
                handle = filtered
            projected = None
            if project is not None:
                block, moved, report = project(grid), C.c_void_p(), abi.RmMeshProjection()
                counts, produced_ms = (C.c_ulonglong * 2)(), (C.c_float * 3)()
                self._check(self.lib.rm_mesh_counts(handle, counts))
                self._check(self.lib.rm_mesh_timings(handle, produced_ms))  # (the producing mesh's three slots stay the result's)
                residual = np.empty(int(counts[0]), np.float32)
                self._check(self.lib.rm_mesh_project(handle, scene.h, C.byref(block), C.byref(moved), C.byref(report), _fp(residual)))
                handles.append(moved)
                handle = moved
                projected = (abi.mesh_projection_dict(report), residual, produced_ms)
            refined = None
            if refine is not None:
                (block, inner), finer, report = refine(grid), C.c_void_p(), abi.RmMeshRefinement()
                stage_ms = (C.c_float * 3)()
                self._check(self.lib.rm_mesh_timings(handle, stage_ms))  # (of the mesh that is refined: the producing mesh's, or the projection's)
                self._check(self.lib.rm_mesh_refine(handle, scene.h, C.byref(block), C.byref(inner), C.byref(finer), C.byref(report)))
                handles.append(finer)
                handle = finer
                refined = (abi.mesh_refinement_dict(report), stage_ms)
            measured = None
            if measures:
                block, measure_ms = abi.RmMeshMeasures(), (C.c_float * 2)()
                self._check(self.lib.rm_mesh_measure(handle, C.byref(block), measure_ms))
                rows = np.empty((int(block.components), 4), np.uint64)
                self._check(self.lib.rm_mesh_measure_components(handle, rows.ctypes.data_as(C.c_void_p), rows.nbytes))
                measured = dict(abi.mesh_measures_dict(block), component_edges=rows)
            counts, ms = (C.c_ulonglong * 2)(), (C.c_float * 3)()
            self._check(self.lib.rm_mesh_counts(handle, counts))
            self._check(self.lib.rm_mesh_timings(handle, ms))
            v, t = int(counts[0]), int(counts[1])
            arrays = {}
            present = {abi.RM_MESH_NORMALS: bool(normals), abi.RM_MESH_COLOURS: bool(colours)}
            for name, what, shape, dtype in (("positions", abi.RM_MESH_POSITIONS, (v, 3), np.float32), ("normals", abi.RM_MESH_NORMALS, (v, 3), np.float32),
                                             ("colours", abi.RM_MESH_COLOURS, (v, 3), np.float32), ("triangles", abi.RM_MESH_TRIANGLES, (t, 3), np.uint32),
                                             ("cells", abi.RM_MESH_CELLS, (v,), np.uint32)):
                if not present.get(what, True):
                    arrays[name] = None  # the mesh was made without this array
                    continue
                a = np.empty(shape, dtype)
                self._check(self.lib.rm_mesh_download(handle, what, a.ctypes.data_as(C.c_void_p), a.nbytes))
                arrays[name] = a
            if components:
                count = C.c_ulonglong()
                self._check(self.lib.rm_mesh_components(handle, C.byref(count)))
                for name, what, shape in (("labels", abi.RM_MESH_PART_LABELS, (v,)), ("component_sizes", abi.RM_MESH_PART_SIZES, (int(count.value), 2))):
                    a = np.empty(shape, np.uint32)
                    self._check(self.lib.rm_mesh_components_download(handle, what, a.ctypes.data_as(C.c_void_p), a.nbytes))
                    arrays[name] = a
            timings = dict(sampling=float(ms[0]), meshing=float(ms[1]), attributes=float(ms[2]))
            refinement_ms = None
            if refined is not None:  # (the handle is the refinement's: its meshing slot is the split rounds, its attributes slot projections and normals)
                arrays["refinement"], stage_ms = refined
                refinement_ms, ms = float(ms[1]) + float(ms[2]), stage_ms
                timings = dict(sampling=float(ms[0]), meshing=float(ms[1]), attributes=float(ms[2]))
            if projected is not None:  # (the handle is the projection's: its meshing slot is the rounds, its attributes slot the normals)
                arrays["projection"], arrays["residual"], produced_ms = projected
                timings = dict(sampling=float(produced_ms[0]), meshing=float(produced_ms[1]), attributes=float(produced_ms[2]),
                               projection=float(ms[1]) + float(ms[2]))
            if refinement_ms is not None:
                timings["refinement"] = refinement_ms
            if occlusion is not None:
                ao, ms2 = np.empty(v, np.float32), (C.c_float * 2)()
                self._check(self.lib.rm_mesh_occlusion(handle, scene.h, C.byref(occlusion), _fp(ao), ms2))
                arrays["occlusion"] = ao
                timings["occlusion"] = float(ms2[0]) + float(ms2[1])
            if deviation is not None:
                report, worst, ms2 = abi.RmMeshDeviationReport(), np.empty(t, np.float32), (C.c_float * 2)()
                self._check(self.lib.rm_mesh_deviation(handle, scene.h, C.byref(deviation), C.byref(report), _fp(worst), ms2))
                arrays["deviation"], arrays["triangle_deviation"] = abi.mesh_deviation_dict(report), worst
                timings["deviation"] = float(ms2[0]) + float(ms2[1])
            if measured is not None:
                arrays["measures"] = measured
                timings["measures"] = float(measure_ms[0]) + float(measure_ms[1])
            return Mesh(grid=grid, timings=timings, **arrays)
        finally:
            for h in reversed(handles):
                self.lib.rm_mesh_destroy(h)

    @staticmethod
    def _mesh_block(name: str, value, struct):
        """The `sharp` / `keep` of extract_mesh / mesh_from_values as its struct, through mesh.mesh_<name>'s checks: None stays None, True is
        the defaults, a dict that function's arguments, a struct its fields -- whose `reserved` is left for the library to refuse."""
        from . import mesh

        make = getattr(mesh, "mesh_" + name)
        if value is None:
            return None
        if isinstance(value, struct):
            block = make(**{f: getattr(value, f) for f, _ in struct._fields_ if f != "reserved"})
            block.reserved = value.reserved
            return block
        if value is True:
            return make()
        if isinstance(value, dict):
            return make(**value)
        raise ValueError(f"mesh: {name} must be None, True, a dict of mesh_{name}'s arguments or an abi.{struct.__name__}")

    @staticmethod
    def _mesh_keep(keep):
        return Context._mesh_block("keep", keep, abi.RmMeshKeep)

    @staticmethod
    def _mesh_occlusion(occlusion):
        """The `occlusion` of extract_mesh as an abi.RmMeshOcclusion (_mesh_block's rules)."""
        return Context._mesh_block("occlusion", occlusion, abi.RmMeshOcclusion)

    @staticmethod
    def _mesh_project(project, iso):
        """The `project` of extract_mesh as a function of the mesh.Grid the projected mesh lies on, which gives the abi.RmMeshProject
        (_mesh_block's rules); None stays None.  True and a dict take the extraction's iso where they name none, and mesh.project_reach of that
        grid where they name no reach; a struct is taken as it stands."""
        from . import mesh

        if project is None:
            return None
        if isinstance(project, abi.RmMeshProject):
            block = Context._mesh_block("project", project, abi.RmMeshProject)
            return lambda grid: block
        if project is True:
            project = {}
        if not isinstance(project, dict):
            raise ValueError("mesh: project must be None, True, a dict of mesh_project's arguments or an abi.RmMeshProject")
        fields = {"iso": iso, **project}
        mesh.mesh_project(**{"reach": 0.0, **fields})  # (refused before anything runs)
        return lambda grid: mesh.mesh_project(**{"reach": mesh.project_reach(grid), **fields})

    @staticmethod
    def _mesh_refine(refine, iso, project):
        """The `refine` of extract_mesh as a function of the mesh.Grid the refined mesh lies on, which gives the pair (abi.RmMeshRefine,
        abi.RmMeshProject) of rm_mesh_refine (_mesh_block's rules); None stays None.  True and a dict take the extraction's iso where they name
        none, and mesh.refine_tolerance of that grid where they name no tolerance; a struct is taken as it stands.  The projection inside the
        rounds is the caller's `project` (the function _mesh_project made of it), or the defaults filled the same way where there is none."""
        from . import mesh

        if refine is None:
            return None
        inner = project if project is not None else Context._mesh_project(True, iso)
        if isinstance(refine, abi.RmMeshRefine):
            block = Context._mesh_block("refine", refine, abi.RmMeshRefine)
            return lambda grid: (block, inner(grid))
        if refine is True:
            refine = {}
        if not isinstance(refine, dict):
            raise ValueError("mesh: refine must be None, True, a dict of mesh_refine's arguments or an abi.RmMeshRefine")
        fields = {"iso": iso, **refine}
        mesh.mesh_refine(**fields)  # (refused before anything runs)
        return lambda grid: (mesh.mesh_refine(**{"tolerance": mesh.refine_tolerance(grid), **fields}), inner(grid))

    @staticmethod
    def _mesh_deviation(deviation, iso):
        """The `deviation` of extract_mesh as an abi.RmMeshDeviation (_mesh_block's rules); None stays None.  True and a dict take the
        extraction's iso where they name none; a struct is taken as it stands."""
        if deviation is True:
            deviation = {}
        if isinstance(deviation, dict):
            deviation = {"iso": iso, **deviation}
        return Context._mesh_block("deviation", deviation, abi.RmMeshDeviation)

    @staticmethod
    def _mesh_quadric(quadric, simplify):
        """The `quadric` of extract_mesh / mesh_from_values as an abi.RmMeshQuadric (_mesh_block's rules); without `simplify` there is nothing
        to place: ValueError."""
        if isinstance(quadric, dict) and set(quadric) - set(abi.MESH_QUADRIC_DEFAULTS):
            raise ValueError(f"mesh: unknown quadric parameter {sorted(set(quadric) - set(abi.MESH_QUADRIC_DEFAULTS))[0]}")
        block = Context._mesh_block("quadric", quadric, abi.RmMeshQuadric)
        if block is not None and simplify is None:
            raise ValueError("mesh: quadric places the vertices of a simplification: give simplify as well")
        return block

    @staticmethod
    def _mesh_simplify(simplify):
        """The `simplify` of extract_mesh / mesh_from_values as (mesh.Grid of the clusters, abi.RmGrid, abi.RmMeshSimplify), through
        mesh.mesh_simplify's checks: None stays None; a mesh.Grid is that grid with the defaults, a dict mesh_simplify's arguments, a pair
        (abi.RmGrid, abi.RmMeshSimplify) its fields -- whose `reserved` are left for the library to refuse."""
        from . import mesh

        if simplify is None:
            return None
        if isinstance(simplify, mesh.Grid):
            return (simplify,) + mesh.mesh_simplify(simplify)
        if isinstance(simplify, dict):
            unknown = set(simplify) - {"grid", "keep_duplicates"}
            if unknown or "grid" not in simplify:
                raise ValueError(f"mesh: unknown simplify parameter {sorted(unknown)[0]}" if unknown else "mesh: simplify needs a grid")
            return (simplify["grid"],) + mesh.mesh_simplify(**simplify)
        if isinstance(simplify, tuple) and len(simplify) == 2 and isinstance(simplify[0], abi.RmGrid) and isinstance(simplify[1], abi.RmMeshSimplify):
            g, p = simplify
            grid = mesh.Grid(tuple(g.lo), tuple(g.hi), tuple(g.n))
            mesh.mesh_simplify(grid, p.keep_duplicates)
            return grid, g, p
        raise ValueError("mesh: simplify must be None, a mesh.Grid, a dict of mesh_simplify's arguments or its (abi.RmGrid, abi.RmMeshSimplify)")

    @staticmethod
    def _mesh_slabs(slabs, grid):
        """The `slabs` of extract_mesh / mesh_from_values as an abi.RmMeshSlabs (_mesh_block's rules, and an int is `layers`); a grid made with
        slabs=True can only be extracted in slabs: ValueError without them."""
        if isinstance(slabs, (int, np.integer)) and not isinstance(slabs, bool):
            slabs = dict(layers=slabs)
        if isinstance(slabs, dict) and set(slabs) - set(abi.MESH_SLABS_DEFAULTS):
            raise ValueError(f"mesh: unknown slabs parameter {sorted(set(slabs) - set(abi.MESH_SLABS_DEFAULTS))[0]}")
        block = Context._mesh_block("slabs", slabs, abi.RmMeshSlabs)
        if block is None and getattr(grid, "slabs", False):
            raise ValueError("mesh: a grid made with slabs=True is extracted in slabs: give slabs as well")
        return block

    def extract_mesh(self, scene: "SceneHandle", grid, iso: float = 0.0, normals: bool = True, colours: bool = False, flags: int = 0,
                     normal_delta: float = 1e-5, sharp=None, *, keep=None, components: bool = False, simplify=None, quadric=None,
                     measures: bool = False, slabs=None, deviation=None, refine=None, project=None, occlusion=None):
        """The level set `iso` of the scene on `grid` (mesh.Grid) as a mesh.Mesh: rm_mesh_extract -- the distances sampled and meshed
        (surface nets) on the device, with per-vertex normals / diffuse colours from the scene's probes when asked for.  `sharp`: None is
        that call; True (the defaults), a dict of mesh.mesh_sharp's arguments or an abi.RmMeshSharp is rm_mesh_extract_sharp -- the same
        triangles with every vertex at its cell's QEF minimiser, which keeps the edges and corners of hard-edged scenes.  `keep`: None
        is that mesh; True (the defaults: drop unreferenced vertices), a dict of mesh.mesh_keep's arguments or an abi.RmMeshKeep filters its
        connected components on the device before anything is downloaded (rm_mesh_filter).  `components`: the returned mesh carries
        labels and component_sizes (rm_mesh_components).  `simplify`: None is that mesh; a mesh.Grid of clusters, a dict of
        mesh.mesh_simplify's arguments or its pair merges the vertices of every cluster cell into one on the device (rm_mesh_simplify) before
        `keep` and `components` are applied, and the returned mesh's grid is the cluster grid.  `quadric` (with `simplify` only): None is
        that call; True (the defaults), a dict of mesh.mesh_quadric's arguments or an abi.RmMeshQuadric is rm_mesh_simplify_quadric -- the same
        mesh with every cluster's vertex at the minimiser of its plane quadrics, which keeps the edges and corners inside a cluster.
        `occlusion`: None is that mesh; True (the defaults), a dict of mesh.mesh_occlusion's arguments or an abi.RmMeshOcclusion bakes the
        scene's ambient occlusion at the vertices of the mesh that is returned -- behind `simplify`, `keep` and `components` -- into
        Mesh.occlusion (rm_mesh_occlusion; 1 = open), which encode_ply writes as `quality` and mesh.shaded multiplies into the colours.
        `measures`: True measures the mesh that is returned on the device -- behind `simplify` and `keep`, before the download -- into
        Mesh.measures (rm_mesh_measure): a dict of abi.RmMeshMeasures' fields (lo and hi as tuples, closed as bool) plus component_edges,
        [C, 4] uint64 rows of (edges, boundary, irregular, unbalanced) per component.
        `slabs`: None is that call; True (the defaults), an int (the cell layers per slab), a dict of mesh.mesh_slabs' arguments or an
        abi.RmMeshSlabs is rm_mesh_extract_slabs / rm_mesh_extract_sharp_slabs -- the same mesh, byte for byte, made from one window of z
        layers at a time, which also takes a grid beyond 2^28 corners (mesh.Grid(..., slabs=True)).  Every other setting composes with it.
        `project`: None is that mesh; True (the defaults), a dict of mesh.mesh_project's arguments or an abi.RmMeshProject moves the vertices of
        the mesh that is returned onto the scene's level set by Newton steps on the device (rm_mesh_project) -- behind `simplify`, `quadric`
        and `keep`, before `components`, `occlusion` and `measures`, which then see the projected mesh.  iso, where not given, is the
        extraction's; reach, where not given, is half the smallest cell side of the grid the returned mesh lies on (the cluster grid with
        `simplify`, else the sampling grid).  The mesh carries Mesh.projection (a dict of abi.RmMeshProjection's fields), Mesh.residual ([V]
        float32: the distance minus iso at the new vertices) and timings["projection"], the milliseconds of the rounds and the normals; the
        other three timings stay those of the mesh that was projected.
        `deviation`: None is that mesh; True (the defaults), a dict of mesh.mesh_deviation's arguments or an abi.RmMeshDeviation measures on the
        device how far the triangles of the mesh that is returned -- behind every stage above, `project` included -- lie off the scene's level
        set at order * order fixed samples each (rm_mesh_deviation).  iso, where not given, is the extraction's.  The mesh carries
        Mesh.deviation (a dict of abi.RmMeshDeviationReport's fields), Mesh.triangle_deviation ([T] float32: each triangle's largest
        |distance - iso| over its samples) and timings["deviation"].
        `refine`: None is that mesh; True (the defaults), a dict of mesh.mesh_refine's arguments or an abi.RmMeshRefine splits, on the device,
        the edges of the mesh that is returned whose midpoint lies further than `tolerance` off the scene's level set, and repeats for `rounds`
        rounds (rm_mesh_refine) -- behind `simplify`, `quadric`, `keep` and `project`, before `components`, `measures`, `occlusion` and
        `deviation`, which then see the refined mesh.  Every round's mesh is projected with the `project` block, or with its defaults (iso and
        reach filled as above) where none is given.  iso, where not given, is the extraction's; tolerance, where not given, is 1/64 of the
        smallest cell side of the grid the mesh lies on (mesh.refine_tolerance: a default, not a bar).  The criterion looks at edge midpoints
        only: `deviation` remains the judge of the result.  The mesh carries Mesh.refinement (a dict of abi.RmMeshRefinement's fields) and
        timings["refinement"]."""
        from .mesh import mesh_params

        keep, simplify, quadric = self._mesh_keep(keep), self._mesh_simplify(simplify), self._mesh_quadric(quadric, simplify)  # (refused before anything runs)
        occlusion, project = self._mesh_occlusion(occlusion), self._mesh_project(project, iso)
        deviation, refine = self._mesh_deviation(deviation, iso), self._mesh_refine(refine, iso, project)
        g, p = grid.to_c(), mesh_params(iso=iso, normals=normals, colours=colours, flags=flags, normal_delta=normal_delta)
        h = C.c_void_p()
        s = self._mesh_block("sharp", sharp, abi.RmMeshSharp)
        w = self._mesh_slabs(slabs, grid)
        if s is None and w is None:
            self._check(self.lib.rm_mesh_extract(self.h, scene.h, C.byref(g), C.byref(p), C.byref(h)))
        elif w is None:
            self._check(self.lib.rm_mesh_extract_sharp(self.h, scene.h, C.byref(g), C.byref(p), C.byref(s), C.byref(h)))
        elif s is None:
            self._check(self.lib.rm_mesh_extract_slabs(self.h, scene.h, C.byref(g), C.byref(p), C.byref(w), C.byref(h)))
        else:
            self._check(self.lib.rm_mesh_extract_sharp_slabs(self.h, scene.h, C.byref(g), C.byref(p), C.byref(s), C.byref(w), C.byref(h)))
        return self._take_mesh(h, grid, normals=p.normals, colours=p.colours, keep=keep, components=components, simplify=simplify, quadric=quadric,
                               scene=scene, occlusion=occlusion, measures=measures, project=project, deviation=deviation, refine=refine)

    def mesh_from_values(self, grid, values: np.ndarray, iso: float = 0.0, *, keep=None, components: bool = False, simplify=None, quadric=None,
                         measures: bool = False, slabs=None):
        """The mesher alone on the caller's field: `values` float32 [nz + 1, ny + 1, nx + 1] (rm_mesh_from_values).  keep, components,
        simplify, quadric, measures and slabs (rm_mesh_from_values_slabs): as in extract_mesh."""
        keep, simplify, quadric = self._mesh_keep(keep), self._mesh_simplify(simplify), self._mesh_quadric(quadric, simplify)
        w = self._mesh_slabs(slabs, grid)
        g = grid.to_c()
        v = np.ascontiguousarray(values, np.float32)
        if v.shape != grid.shape:
            raise ValueError(f"values must have the shape {grid.shape} of the grid's corners, not {v.shape}")
        h = C.c_void_p()
        if w is None:
            self._check(self.lib.rm_mesh_from_values(self.h, C.byref(g), _fp(v), float(iso), C.byref(h)))
        else:
            self._check(self.lib.rm_mesh_from_values_slabs(self.h, C.byref(g), _fp(v), float(iso), C.byref(w), C.byref(h)))
        return self._take_mesh(h, grid, keep=keep, components=components, simplify=simplify, quadric=quadric, measures=measures)

    def probe_camera(self, uniforms: abi.RmUniforms, width: int, height: int) -> np.ndarray:
        out = np.empty((height, width, 8), np.float32)
        self._check(self.lib.rm_probe_camera(self.h, C.byref(uniforms), width, height, _fp(out)))
        return out

    def probe_rng(self, uniforms: abi.RmUniforms, width: int, height: int, count: int) -> np.ndarray:
        out = np.empty((height, width, count), np.float32)
        self._check(self.lib.rm_probe_rng(self.h, C.byref(uniforms), width, height, count, _fp(out)))
        return out

    def probe_math(self, name: str, a: np.ndarray, b: np.ndarray = None) -> np.ndarray:
        """One transcendental of this context's parity arithmetic on an array (rm_probe_math; name: abi.RM_MATH_FUNCTIONS)."""
        a = np.ascontiguousarray(a, np.float32).ravel()
        b = np.ascontiguousarray(b, np.float32).ravel() if b is not None else None
        out = np.empty_like(a)
        self._check(self.lib.rm_probe_math(self.h, abi.RM_MATH_FUNCTIONS.index(name), _fp(a), _fp(b) if b is not None else None, a.size, _fp(out)))
        return out


class SceneHandle:
    def __init__(self, ctx: Context, scene: Scene):
        self.ctx = ctx
        desc = scene.desc()
        h = C.c_void_p()
        ctx._check(ctx.lib.rm_scene_create(ctx.h, C.byref(desc), C.byref(h)))
        self.h = h

    def destroy(self):
        if self.h:
            self.ctx.lib.rm_scene_destroy(self.h)
            self.h = None


class Framebuffer:
    def __init__(self, ctx: Context, width, height, row_begin, row_count, wrap=None, striped=None, gbuffer: str = "f32", moments: bool = False):
        fmt = gbuffer_code(gbuffer)
        if moments:
            if wrap is not None or striped is not None:
                raise ValueError("moments=True is for framebuffers the library allocates whole (Context.create_framebuffer)")
            fmt |= abi.RM_FB_MOMENTS
        self.ctx = ctx
        self.width, self.height, self.row_begin, self.row_count = width, height, row_begin, row_count
        self.gbuffer = gbuffer
        h = C.c_void_p()
        if striped is not None:
            s, n, r, c0, c1, c2 = striped
            ctx._check(ctx.lib.rm_fb_create_striped_fmt(ctx.h, width, height, s, n, r, C.c_void_p(c0 or 0), C.c_void_p(c1 or 0),
                                                        C.c_void_p(c2 or 0), fmt, C.byref(h)))
            self.row_count = int(ctx.lib.rm_fb_rows(h))
        elif wrap is None:
            ctx._check(ctx.lib.rm_fb_create_fmt(ctx.h, width, height, row_begin, row_count, fmt, C.byref(h)))
        else:
            ctx._check(ctx.lib.rm_fb_wrap_fmt(ctx.h, width, height, row_begin, row_count, C.c_void_p(wrap[0]),
                                              C.c_void_p(wrap[1] or 0), C.c_void_p(wrap[2] or 0), fmt, C.byref(h)))
        self.h = h

    @property
    def moments(self) -> bool:
        """True when the framebuffer keeps the moments plane (rm_fb_has_moments)."""
        return bool(self.ctx.lib.rm_fb_has_moments(self.h))

    def plane_dtype(self, plane: int):
        """numpy dtype of a plane as stored: float32, or float16 for the G-buffer planes of an "f16" framebuffer."""
        return np.float16 if (plane in (abi.RM_PLANE_NORMAL_DOF, abi.RM_PLANE_ALBEDO_DEPTH) and self.gbuffer == "f16") else np.float32

    def download_raw(self, plane: int = abi.RM_PLANE_COLOR) -> np.ndarray:
        """A plane as stored ([rows, W, 4] of plane_dtype(plane)): the half bits of an "f16" G-buffer plane, not widened.
        Plane 3 (abi.RM_PLANE_MOMENTS) is [rows, W, 2] float32: (sum l, sum l^2)."""
        out = np.empty((self.row_count, self.width, 2 if plane == abi.RM_PLANE_MOMENTS else 4), self.plane_dtype(plane))
        self.ctx._check(self.ctx.lib.rm_fb_download_raw(self.h, plane, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def upload_raw(self, plane: int, data: np.ndarray):
        """Stores [rows, W, 4] of plane_dtype(plane) into a plane as they are."""
        a = np.ascontiguousarray(data, self.plane_dtype(plane))
        assert a.shape == (self.row_count, self.width, 2 if plane == abi.RM_PLANE_MOMENTS else 4)
        self.ctx._check(self.ctx.lib.rm_fb_upload_raw(self.h, plane, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def clear(self):
        self.ctx._check(self.ctx.lib.rm_fb_clear(self.h))

    def destroy(self):
        if self.h:
            self.ctx.lib.rm_fb_destroy(self.h)
            self.h = None

    def download(self, plane: int = abi.RM_PLANE_COLOR) -> np.ndarray:
        """A plane as float32 (a half plane widened exactly)."""
        out = np.empty((self.row_count, self.width, 4), np.float32)
        self.ctx._check(self.ctx.lib.rm_fb_download(self.h, plane, _fp(out)))
        return out

    def upload(self, plane: int, data: np.ndarray):
        """float32 data into a plane (a half plane rounds it to nearest even, on the device)."""
        a = np.ascontiguousarray(data, np.float32)
        assert a.shape == (self.row_count, self.width, 4)
        self.ctx._check(self.ctx.lib.rm_fb_upload(self.h, plane, _fp(a)))

    def device_ptr(self, plane: int = abi.RM_PLANE_COLOR) -> int:
        return int(self.ctx.lib.rm_fb_device_ptr(self.h, plane) or 0)

    def stats(self, samples: int, despeckle=None, denoise=None) -> FrameStats:
        """The luminance statistics of the rows this framebuffer holds (rm_frame_stats): of the colour plane as it is, or with
        `despeckle` / `denoise` (what filter takes) of the chain's result -- what will be shown once the fireflies are gone."""
        out = abi.RmFrameStats()
        f = filters(despeckle, denoise) if (despeckle is not None or denoise is not None) else None
        self.ctx._check(self.ctx.lib.rm_frame_stats(self.ctx.h, self.h, int(samples), C.byref(f) if f is not None else None, C.byref(out)))
        return FrameStats(out)

    def display_block(self, samples: int, denoise=None, despeckle=None, display=None) -> abi.RmDisplay:
        """The abi.RmDisplay of a present's `display`: what display_params takes, or "auto" / a dict with an "auto" entry (True or
        the fields of rm_stats_exposure's block) next to `tone` and `white`: the gain then comes from `stats` of the same chain."""
        if not display_is_auto(display):
            return display_params(display)
        fields = {} if isinstance(display, str) else dict(display)
        auto = fields.pop("auto", True)
        if "gain" in fields:
            raise ValueError("display: give either a gain or \"auto\"")
        d = display_params(fields)
        p = auto_exposure_params(None if auto is True else auto)
        d.gain = self.stats(samples, despeckle=despeckle, denoise=denoise).exposure(**{k: getattr(p, k) for k in abi.AUTO_EXPOSURE_DEFAULTS})
        return d

    def linear(self, samples: int, denoise=None, despeckle=None, display=None) -> np.ndarray:
        """The blurred, exposed frame as floats (rm_present_linear): what present holds in front of its tone operator and pow,
        (e.r, e.g, e.b, 1) as float32 [H, W, 4], row 0 = bottom.  `display` as present takes it (its tone is checked, not applied)."""
        d = self.display_block(samples, denoise, despeckle, display)
        f = filters(despeckle, denoise)
        out = np.empty((self.row_count, self.width, 4), np.float32)
        self.ctx._check(self.ctx.lib.rm_present_linear(self.ctx.h, self.h, int(samples), C.byref(f), C.byref(d), _fp(out)))
        return out

    def present(self, samples: int, denoise=None, despeckle=None, display=None) -> np.ndarray:
        """Tone-mapped RGBA8 image of the whole frame (display.frag:16-64), row 0 = bottom.  `denoise`: None (the default: the
        accumulated colour as it is), or True / a dict / abi.RmDenoise to present the denoised colour (rm_present_denoised); or
        "variance" / abi.RmDenoiseVariance / a dict with "mode": "variance" for the variance-guided filter
        (rm_present_denoised_variance; the framebuffer needs moments=True).  `despeckle`: None (the default: no firefly filter, and
        exactly the calls above), or True / a dict / abi.RmDespeckle to run the firefly filter ahead of the denoiser and the present
        (rm_present_filtered).  `display`: None (the default: the reference's transform, and exactly the calls above), or a dict /
        abi.RmDisplay -- gain, tone ("clip", "reinhard", "aces"), white -- for the display transform behind the blur
        (rm_present_display); "auto" or {"auto": True or rm_stats_exposure's fields, "tone": ...} takes the gain from the
        statistics of the same chain (stats, FrameStats.exposure)."""
        out = np.empty((self.row_count, self.width, 4), np.uint8)
        if display is not None:
            d = self.display_block(samples, denoise, despeckle, display)
            f = filters(despeckle, denoise)
            self.ctx._check(self.ctx.lib.rm_present_display(self.ctx.h, self.h, int(samples), C.byref(f), C.byref(d), out.ctypes.data_as(C.POINTER(C.c_uint8))))
            return out
        if despeckle is not None:
            f = filters(despeckle, denoise)
            self.ctx._check(self.ctx.lib.rm_present_filtered(self.ctx.h, self.h, int(samples), C.byref(f), out.ctypes.data_as(C.POINTER(C.c_uint8))))
            return out
        if denoise is None:
            self.ctx._check(self.ctx.lib.rm_present(self.ctx.h, self.h, int(samples), out.ctypes.data_as(C.POINTER(C.c_uint8))))
            return out
        mode, p = denoise_mode(denoise)
        fn = self.ctx.lib.rm_present_denoised_variance if mode == "variance" else self.ctx.lib.rm_present_denoised
        self.ctx._check(fn(self.ctx.h, self.h, int(samples), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def filter(self, samples: int, despeckle=None, denoise=None) -> np.ndarray:
        """The colour plane after the chain despeckle -> denoise (rm_filter): float32 [rows, W, 4] in colour-plane units, row 0 =
        bottom.  `despeckle`: None (off) or True / a dict / abi.RmDespeckle; `denoise`: None (off) or what present's takes.  With
        both off it is the colour plane itself."""
        f = filters(despeckle, denoise)
        out = np.empty((self.row_count, self.width, 4), np.float32)
        self.ctx._check(self.ctx.lib.rm_filter(self.ctx.h, self.h, int(samples), C.byref(f), _fp(out)))
        return out

    def denoise(self, samples: int, params=None) -> np.ndarray:
        """The colour plane after the G-buffer-guided a-trous filter (rm_denoise): float32 [rows, W, 4] in colour-plane units,
        row 0 = bottom.  `params`: None / True (the defaults), a dict of some RmDenoise fields, or abi.RmDenoise."""
        p = denoise_params(params)
        out = np.empty((self.row_count, self.width, 4), np.float32)
        self.ctx._check(self.ctx.lib.rm_denoise(self.ctx.h, self.h, int(samples), C.byref(p), _fp(out)))
        return out

    def denoise_variance(self, samples: int, params=None) -> np.ndarray:
        """The colour plane after the variance-guided filter (rm_denoise_variance; the framebuffer needs moments=True): float32
        [rows, W, 4] in colour-plane units, row 0 = bottom.  `params`: None / True (the defaults), a dict of some
        RmDenoiseVariance fields, or abi.RmDenoiseVariance."""
        p = denoise_variance_params(params)
        out = np.empty((self.row_count, self.width, 4), np.float32)
        self.ctx._check(self.ctx.lib.rm_denoise_variance(self.ctx.h, self.h, int(samples), C.byref(p), _fp(out)))
        return out
