"""ctypes mirror of include/hip_raymarch.h (POD structs and constants only)."""
from __future__ import annotations

import ctypes as C

RM_ABI_VERSION = 9
RM_MAX_BOUNCES = 10
RM_MAX_LIGHTS = 10
RM_MAX_PRIMS = 256

RM_OK, RM_ERR_INVALID, RM_ERR_DEVICE, RM_ERR_NO_DEVICE = 0, 1, 2, 3

(RM_SCENE_TABLE, RM_SCENE_MANDELBULB, RM_SCENE_SPHERE_GRID, RM_SCENE_SPHERE_LATTICE,
 RM_SCENE_MENGER, RM_SCENE_KIFS_TREE, RM_SCENE_KIFS_BOX) = range(7)
RM_PRIM_SPHERE, RM_PRIM_BOX, RM_PRIM_REPEAT, RM_PRIM_FOLD, RM_PRIM_KIND, RM_PRIM_TORUS, RM_PRIM_CYLINDER, RM_PRIM_PLANE = 0, 1, 2, 3, 4, 5, 6, 7
RM_OP_UNION, RM_OP_SMOOTH_UNION, RM_OP_SUBTRACT, RM_OP_INTERSECT, RM_OP_SMOOTH_SUBTRACT, RM_OP_SMOOTH_INTERSECT = 0, 1, 2, 3, 4, 5

RM_RENDER_STRICT, RM_RENDER_FAST, RM_RENDER_COLOR_ONLY, RM_RENDER_MEGAKERNEL, RM_RENDER_NO_COST_CLASSES, RM_RENDER_WAVEFRONT = 0, 1, 2, 4, 8, 16
RM_RENDER_NO_OVERLAP = 32
RM_RENDER_NO_FAR_JUMP = 64
RM_RENDER_NO_CULL = 128
RM_PIPELINE_NONE, RM_PIPELINE_PIXEL_KERNEL, RM_PIPELINE_WAVEFRONT = 0, 1, 2
RM_PLANE_COLOR, RM_PLANE_NORMAL_DOF, RM_PLANE_ALBEDO_DEPTH = 0, 1, 2
RM_GBUFFER_F32, RM_GBUFFER_F16 = 0, 1  # G-buffer formats (ABI 9)
RM_FB_MOMENTS = 0x100  # OR'ed into rm_fb_create_fmt's format: the moments plane (ABI 9)
RM_PLANE_MOMENTS = 3
RM_PROBE_SDF, RM_PROBE_CAST_RAY, RM_PROBE_NORMAL, RM_PROBE_MATERIAL, RM_PROBE_CAST_STEPS, RM_PROBE_CAST_SHADOW = 0, 1, 2, 3, 4, 5
RM_MATH_FUNCTIONS = ("sin", "cos", "log", "exp", "pow", "acos", "atan2", "tan", "pow_pair_nm1", "pow_pair_n", "sincos_s", "sincos_c", "sqrt", "div")  # RM_MATH_*


class RmUniforms(C.Structure):
    _fields_ = [
        ("blendWithPreviousFactor", C.c_float),
        ("randNoise", C.c_float * 2),
        ("position", C.c_float * 3),
        ("rotation", C.c_float * 16),
        ("dofAmount", C.c_float),
        ("dofFocalPlaneDistance", C.c_float),
        ("cameraMode", C.c_int32),
        ("fov", C.c_float),
        ("reflections", C.c_float),
        ("raymarchingSteps", C.c_float),
        ("indirectLightingRaymarchingSteps", C.c_float),
        ("aspect", C.c_float),
        ("fogDensity", C.c_float),
        ("exposure", C.c_float),
        ("raymarchingStepCountsArray", C.c_float * RM_MAX_BOUNCES),
        ("blendMode", C.c_int32),
        ("renderMode", C.c_int32),
        ("lightPositions", (C.c_float * 3) * RM_MAX_LIGHTS),
        ("lightColors", (C.c_float * 3) * RM_MAX_LIGHTS),
        ("lightSizes", C.c_float * RM_MAX_LIGHTS),
        ("lightCount", C.c_int32),
        ("showDofFocalPlane", C.c_int32),
    ]


class RmPrim(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("k", C.c_float),
        ("center", C.c_float * 3),
        ("size", C.c_float * 3),
    ]


class RmMaterial(C.Structure):
    _fields_ = [
        ("diffuse", C.c_float * 3),
        ("diffuse_cutoff", C.c_float),
        ("specular", C.c_float * 3),
        ("specular_cutoff", C.c_float),
        ("roughness", C.c_float),
        ("subsurface", C.c_float),
        ("subsurface_color", C.c_float * 3),
        ("ior", C.c_float),
        ("sky_color", C.c_float * 3),
        ("sky_floor", C.c_float),
        ("sky_scale", C.c_float),
        ("sky_radius", C.c_float),
        ("sky_axis", C.c_int32),
        ("reserved", C.c_int32),
    ]


RM_MAX_SURFACES = 15


class RmSurface(C.Structure):
    _fields_ = [
        ("diffuse", C.c_float * 3),
        ("roughness", C.c_float),
        ("specular", C.c_float * 3),
        ("subsurface", C.c_float),
        ("subsurface_color", C.c_float * 3),
        ("ior", C.c_float),
    ]


class RmSceneDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("nprims", C.c_int32),
        ("prims", C.POINTER(RmPrim)),
        ("params", C.c_float * 16),
        ("material", RmMaterial),
        ("nsurfaces", C.c_int32),
        ("reserved", C.c_int32),
        ("surfaces", C.POINTER(RmSurface)),
    ]


class RmRect(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class RmDenoise(C.Structure):
    """Parameters of rm_denoise* (ABI 9): the G-buffer-guided a-trous filter (include/hip_raymarch.h)."""
    _fields_ = [
        ("iterations", C.c_int32),
        ("sigma_color", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_int32),
    ]


DENOISE_DEFAULTS = dict(iterations=5, sigma_color=2.5, sigma_normal=2.0, sigma_depth=0.2)  # rm_denoise_default


class RmDenoiseVariance(C.Structure):
    """Parameters of rm_denoise_variance* (ABI 9): the variance-guided filter (include/hip_raymarch.h)."""
    _fields_ = [
        ("iterations", C.c_int32),
        ("sigma_luminance", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_int32),
    ]


DENOISE_VARIANCE_DEFAULTS = dict(iterations=3, sigma_luminance=4.0, sigma_normal=1.0, sigma_depth=0.2)  # rm_denoise_variance_default


class RmDespeckle(C.Structure):
    """Parameters of the firefly filter (ABI 9): the outlier clamp ahead of the denoisers (include/hip_raymarch.h)."""
    _fields_ = [
        ("radius", C.c_int32),
        ("rank", C.c_int32),
        ("gain", C.c_float),
        ("floor", C.c_float),
        ("repair", C.c_int32),
        ("reserved", C.c_int32),
    ]


DESPECKLE_DEFAULTS = dict(radius=2, rank=1, gain=3.0, floor=0.1, repair=1)  # rm_filters_default's despeckle_params

RM_DENOISE_NONE, RM_DENOISE_ATROUS, RM_DENOISE_VARIANCE = 0, 1, 2


class RmFilters(C.Structure):
    """The chain ahead of the present, despeckle -> denoise (ABI 9; rm_filter, rm_filter_device, rm_present_filtered)."""
    _fields_ = [
        ("despeckle", C.c_int32),
        ("denoise", C.c_int32),
        ("despeckle_params", RmDespeckle),
        ("atrous", RmDenoise),
        ("variance", RmDenoiseVariance),
    ]

assert C.sizeof(RmPrim) == 32 and C.sizeof(RmSurface) == 48 and C.sizeof(RmDespeckle) == 24 and C.sizeof(RmFilters) == 72


RM_STATS_BINS = 512


class RmFrameStats(C.Structure):
    """rm_frame_stats' result (ABI 9): the luminance histogram of a frame, 16 bins per octave over [2^-20, 2^12), the three classes
    outside it and the exact minimum and maximum over the finite luminances (include/hip_raymarch.h)."""
    _fields_ = [
        ("pixels", C.c_uint64),
        ("below", C.c_uint64),
        ("above", C.c_uint64),
        ("non_finite", C.c_uint64),
        ("min_l", C.c_float),
        ("max_l", C.c_float),
        ("hist", C.c_uint64 * RM_STATS_BINS),
    ]


class RmAutoExposure(C.Structure):
    """Parameters of rm_stats_exposure (ABI 9): the gain that brings the log-average between two percentiles to `key`."""
    _fields_ = [
        ("key", C.c_float),
        ("low", C.c_float),
        ("high", C.c_float),
        ("min_gain", C.c_float),
        ("max_gain", C.c_float),
        ("reserved", C.c_int32),
    ]


AUTO_EXPOSURE_DEFAULTS = dict(key=0.18, low=0.10, high=0.95, min_gain=2.0 ** -10, max_gain=2.0 ** 10)  # rm_auto_exposure_default

RM_TONE_CLIP, RM_TONE_REINHARD, RM_TONE_ACES = 0, 1, 2
TONE_NAMES = {"clip": RM_TONE_CLIP, "reinhard": RM_TONE_REINHARD, "aces": RM_TONE_ACES}


class RmDisplay(C.Structure):
    """The display transform behind the present pass's blur (ABI 9; rm_present_display, rm_present_display_device, rm_present_linear)."""
    _fields_ = [
        ("gain", C.c_float),
        ("tone", C.c_int32),
        ("white", C.c_float),
        ("reserved", C.c_int32),
    ]


DISPLAY_DEFAULTS = dict(gain=1.0, tone=RM_TONE_CLIP, white=4.0)  # rm_display_default

assert C.sizeof(RmFrameStats) == 4136 and C.sizeof(RmAutoExposure) == 24 and C.sizeof(RmDisplay) == 16


RM_MESH_POSITIONS, RM_MESH_NORMALS, RM_MESH_COLOURS, RM_MESH_TRIANGLES, RM_MESH_CELLS = 0, 1, 2, 3, 4


class RmGrid(C.Structure):
    """The grid of rm_sdf_grid / rm_mesh_* (ABI 9): n CELLS per axis, n + 1 corners at lo + i * (hi - lo) / n (include/hip_raymarch.h)."""
    _fields_ = [
        ("lo", C.c_float * 3),
        ("hi", C.c_float * 3),
        ("n", C.c_int32 * 3),
        ("reserved", C.c_int32),
    ]


class RmMeshParams(C.Structure):
    """Parameters of rm_mesh_extract (ABI 9): the level, and which per-vertex arrays the scene's probes add (include/hip_raymarch.h)."""
    _fields_ = [
        ("iso", C.c_float),
        ("normals", C.c_int32),
        ("normal_delta", C.c_float),
        ("colours", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
    ]


MESH_DEFAULTS = dict(iso=0.0, normals=1, normal_delta=1e-5, colours=0, flags=0)  # rm_mesh_params_default

assert C.sizeof(RmGrid) == 40 and C.sizeof(RmMeshParams) == 24


class RmMeshSharp(C.Structure):
    """Parameters of rm_mesh_extract_sharp (ABI 9): the bisection rounds of an edge crossing, the step of the normals at the crossings and the
    relative eigenvalue below which the QEF is truncated (include/hip_raymarch.h "sharp vertices")."""
    _fields_ = [
        ("refine", C.c_int32),
        ("normal_delta", C.c_float),
        ("threshold", C.c_float),
        ("reserved", C.c_int32),
    ]


MESH_SHARP_DEFAULTS = dict(refine=6, normal_delta=2.0 ** -10, threshold=0.1)  # rm_mesh_sharp_default

assert C.sizeof(RmMeshSharp) == 16


RM_MESH_PART_LABELS, RM_MESH_PART_SIZES = 0, 1


class RmMeshKeep(C.Structure):
    """The keep rule of rm_mesh_filter (ABI 9): a component passes with at least min_triangles triangles; largest = k > 0 keeps only the k
    passing components with the most triangles (include/hip_raymarch.h "components and islands")."""
    _fields_ = [
        ("min_triangles", C.c_int32),
        ("largest", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


MESH_KEEP_DEFAULTS = dict(min_triangles=1, largest=0)  # rm_mesh_keep_default

assert C.sizeof(RmMeshKeep) == 16


class RmMeshSimplify(C.Structure):
    """Parameters of rm_mesh_simplify (ABI 9): keep_duplicates = 1 keeps every surviving triangle, 0 only the first of each canonical form
    (include/hip_raymarch.h "simplification")."""
    _fields_ = [
        ("keep_duplicates", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


MESH_SIMPLIFY_DEFAULTS = dict(keep_duplicates=0)  # rm_mesh_simplify_default

assert C.sizeof(RmMeshSimplify) == 16


class RmMeshQuadric(C.Structure):
    """Parameters of rm_mesh_simplify_quadric (ABI 9): eigenvalues at or below threshold * the largest are dropped from a cluster's solve
    (include/hip_raymarch.h "quadric placement")."""
    _fields_ = [
        ("threshold", C.c_float),
        ("reserved", C.c_int32 * 3),
    ]


MESH_QUADRIC_DEFAULTS = dict(threshold=0.1)  # rm_mesh_quadric_default

assert C.sizeof(RmMeshQuadric) == 16


class RmMeshOcclusion(C.Structure):
    """Parameters of rm_mesh_occlusion (ABI 9): `directions` directions over every vertex, `taps` taps along each, the first at `radius`
    (include/hip_raymarch.h "ambient occlusion")."""
    _fields_ = [
        ("radius", C.c_float),
        ("directions", C.c_int32),
        ("taps", C.c_int32),
        ("normal_delta", C.c_float),
        ("strength", C.c_float),
        ("flags", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


MESH_OCCLUSION_DEFAULTS = dict(radius=0.25, directions=16, taps=4, normal_delta=2.0 ** -10, strength=1.0, flags=0)  # rm_mesh_occlusion_default

assert C.sizeof(RmMeshOcclusion) == 32


class RmMeshMeasures(C.Structure):
    """What rm_mesh_measure says of a mesh (ABI 9): counts of vertices, triangles and edge classes, the Euler characteristic, components,
    area, signed volume and extent (include/hip_raymarch.h "measures and edge topology")."""
    _fields_ = [
        ("vertices", C.c_uint64),
        ("triangles", C.c_uint64),
        ("used_vertices", C.c_uint64),
        ("skipped_triangles", C.c_uint64),
        ("unmeasured_triangles", C.c_uint64),
        ("finite_vertices", C.c_uint64),
        ("edges", C.c_uint64),
        ("boundary_edges", C.c_uint64),
        ("regular_edges", C.c_uint64),
        ("irregular_edges", C.c_uint64),
        ("unbalanced_edges", C.c_uint64),
        ("euler", C.c_int64),
        ("components", C.c_uint64),
        ("closed_components", C.c_uint64),
        ("area", C.c_double),
        ("volume", C.c_double),
        ("lo", C.c_float * 3),
        ("hi", C.c_float * 3),
        ("closed", C.c_int32),
        ("reserved", C.c_int32),
    ]


assert C.sizeof(RmMeshMeasures) == 160


class RmMeshSlabs(C.Structure):
    """The window of rm_mesh_extract_slabs / _sharp_slabs / rm_mesh_from_values_slabs (ABI 9): cell layers per slab, 0 = chosen by the library
    (include/hip_raymarch.h "slabbed extraction")."""
    _fields_ = [
        ("layers", C.c_int32),
        ("reserved", C.c_int32),
    ]


MESH_SLABS_DEFAULTS = dict(layers=0)  # rm_mesh_slabs_default

assert C.sizeof(RmMeshSlabs) == 8


class RmMeshProject(C.Structure):
    """Parameters of rm_mesh_project (ABI 9): up to `rounds` Newton steps p <- p - n * relax * (d - iso) of every vertex, at most `reach` per
    axis from where it started (include/hip_raymarch.h "projection onto the surface")."""
    _fields_ = [
        ("iso", C.c_float),
        ("rounds", C.c_int32),
        ("relax", C.c_float),
        ("tolerance", C.c_float),
        ("reach", C.c_float),
        ("normal_delta", C.c_float),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
    ]


MESH_PROJECT_DEFAULTS = dict(iso=0.0, rounds=4, relax=1.0, tolerance=0.0, reach=0.0, normal_delta=2.0 ** -10, flags=0)  # rm_mesh_project_default

assert C.sizeof(RmMeshProject) == 32


class RmMeshProjection(C.Structure):
    """What rm_mesh_project says of its work (ABI 9): how far off the level set the vertices were and are, and what the steps met."""
    _fields_ = [
        ("vertices", C.c_uint64),
        ("triangles", C.c_uint64),
        ("moved_vertices", C.c_uint64),
        ("settled_before", C.c_uint64),
        ("settled_after", C.c_uint64),
        ("nonfinite_before", C.c_uint64),
        ("nonfinite_after", C.c_uint64),
        ("clamped_vertices", C.c_uint64),
        ("undirected_vertices", C.c_uint64),
        ("flipped_triangles", C.c_uint64),
        ("worst_before", C.c_uint64),
        ("worst_after", C.c_uint64),
        ("mean_before", C.c_double),
        ("rms_before", C.c_double),
        ("mean_after", C.c_double),
        ("rms_after", C.c_double),
        ("max_before", C.c_float),
        ("max_after", C.c_float),
        ("rounds_run", C.c_int32),
        ("reserved", C.c_int32),
    ]


assert C.sizeof(RmMeshProjection) == 144


def mesh_projection_dict(r: "RmMeshProjection") -> dict:
    """The struct's fields as a dict, `reserved` left out."""
    return {name: getattr(r, name) for name, _ in RmMeshProjection._fields_ if name != "reserved"}


class RmMeshDeviation(C.Structure):
    """Parameters of rm_mesh_deviation (ABI 9): the scene's distance minus `iso` at order * order fixed points inside every triangle
    (include/hip_raymarch.h "deviation")."""
    _fields_ = [
        ("iso", C.c_float),
        ("order", C.c_int32),
        ("tolerance", C.c_float),
        ("flags", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


MESH_DEVIATION_DEFAULTS = dict(iso=0.0, order=4, tolerance=0.0, flags=0)  # rm_mesh_deviation_default

assert C.sizeof(RmMeshDeviation) == 32


class RmMeshDeviationReport(C.Structure):
    """What rm_mesh_deviation says of a mesh (ABI 9): how far its triangles lie off the level set at their samples, area-weighted."""
    _fields_ = [
        ("vertices", C.c_uint64),
        ("triangles", C.c_uint64),
        ("skipped_triangles", C.c_uint64),
        ("unevaluated_triangles", C.c_uint64),
        ("nonfinite_samples", C.c_uint64),
        ("over_triangles", C.c_uint64),
        ("worst_triangle", C.c_uint64),
        ("area", C.c_double),
        ("over_area", C.c_double),
        ("mean_signed", C.c_double),
        ("rms", C.c_double),
        ("max", C.c_float),
        ("samples", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


assert C.sizeof(RmMeshDeviationReport) == 112


def mesh_deviation_dict(r: "RmMeshDeviationReport") -> dict:
    """The struct's fields as a dict, `reserved` left out."""
    return {name: getattr(r, name) for name, _ in RmMeshDeviationReport._fields_ if name != "reserved"}


class RmMeshRefine(C.Structure):
    """Parameters of rm_mesh_refine (ABI 9): split the edges whose midpoint lies further than `tolerance` off the level `iso`
    (include/hip_raymarch.h "refinement")."""
    _fields_ = [
        ("iso", C.c_float),
        ("tolerance", C.c_float),
        ("min_edge", C.c_float),
        ("rounds", C.c_int32),
        ("max_triangles", C.c_uint64),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
    ]


MESH_REFINE_DEFAULTS = dict(iso=0.0, tolerance=0.0, min_edge=0.0, rounds=1, max_triangles=0, flags=0)  # rm_mesh_refine_default

assert C.sizeof(RmMeshRefine) == 32


class RmMeshRefinement(C.Structure):
    """What rm_mesh_refine says of its work (ABI 9): the sizes before and after, per round the edges examined, split and without a finite
    distance, the projections' flips, the largest |distance - iso| of the first and the last round, and why it stopped."""
    _fields_ = [
        ("vertices_before", C.c_uint64),
        ("triangles_before", C.c_uint64),
        ("vertices", C.c_uint64),
        ("triangles", C.c_uint64),
        ("edges", C.c_uint64 * 8),
        ("split_edges", C.c_uint64 * 8),
        ("nonfinite_midpoints", C.c_uint64 * 8),
        ("flipped_triangles", C.c_uint64),
        ("max_first", C.c_float),
        ("max_last", C.c_float),
        ("rounds_run", C.c_int32),
        ("stopped", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


assert C.sizeof(RmMeshRefinement) == 256


def mesh_refinement_dict(r: "RmMeshRefinement") -> dict:
    """The struct's fields as a dict: the per-round arrays as tuples of eight, `reserved` left out."""
    d = {name: getattr(r, name) for name, _ in RmMeshRefinement._fields_ if name != "reserved"}
    for name in ("edges", "split_edges", "nonfinite_midpoints"):
        d[name] = tuple(int(x) for x in d[name])
    return d


def mesh_measures_dict(m: "RmMeshMeasures") -> dict:
    """The struct's fields as a dict: lo and hi as tuples, `closed` as bool, `reserved` left out."""
    d = {name: getattr(m, name) for name, _ in RmMeshMeasures._fields_ if name != "reserved"}
    d["lo"], d["hi"], d["closed"] = tuple(float(x) for x in m.lo), tuple(float(x) for x in m.hi), bool(m.closed)
    return d
