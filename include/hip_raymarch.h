/*
 * hip_raymarch.h -- C ABI of libhip_raymarch.so
 *
 * MI355X (gfx950) implementation of the one hot path of
 * radian628/raymarching-engine: the per-pixel sphere-tracing fragment shader
 *   client/public/shader/raymarcher.frag            (kernel, 387 lines of GLSL)
 * behind the boundary the reference's host crosses for every sample,
 *   client/src/renderer/RenderJobExecutor.tsx:195-326 (bind prev, set uniforms, draw, blit).
 *
 * Every entry point cites the reference interface it replaces.  The ABI is
 * plain C: pointers, sizes and POD structs of fp32/int32 only, no C++ or
 * torch types.  Error convention (the reference returns errors as values,
 * RenderJobExecutor.tsx:56-68,112-136; ShaderCache.tsx:4-11): every call
 * returns an int status, RM_OK == 0, and the text for the last failure is
 * kept per context (rm_last_error).  Nothing throws across the ABI.
 *
 * Threading: one caller per rm_ctx (the reference is single threaded,
 * index.tsx:120); launches are asynchronous on the context's HIP stream and
 * rm_sync() is the completion point.  One rm_ctx per GPU.
 */
#ifndef HIP_RAYMARCH_H
#define HIP_RAYMARCH_H

#include <stddef.h>
#include <stdint.h>

/* The library is built -fvisibility=hidden: exactly the entry points below are exported (tests/test_host_cpu.py compares
 * this header with `nm -D`). */
#ifndef RM_API
#define RM_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RM_ABI_VERSION 9 /* 9: RM_GBUFFER_F32 / _F16, rm_fb_create_fmt, rm_fb_create_striped_fmt, rm_fb_wrap_fmt, rm_fb_gbuffer, rm_fb_download_raw, rm_fb_upload_raw, RmDenoise, rm_denoise_default, rm_denoise, rm_denoise_device, rm_present_denoised, RM_FB_MOMENTS, RM_PLANE_MOMENTS, rm_fb_has_moments, RmDenoiseVariance, rm_denoise_variance_default, rm_denoise_variance, rm_denoise_variance_device, rm_present_denoised_variance, RmDespeckle, RmFilters, RM_DENOISE_NONE / _ATROUS / _VARIANCE, rm_filters_default, rm_filter, rm_filter_device, rm_present_filtered, RM_STATS_BINS, RmFrameStats, rm_frame_stats, RmAutoExposure, rm_auto_exposure_default, rm_stats_percentile, rm_stats_exposure, RM_TONE_CLIP / _REINHARD / _ACES, RmDisplay, rm_display_default, rm_present_display, rm_present_display_device, rm_present_linear, RmGrid, rm_grid_axis, rm_sdf_grid, rm_sdf_grid_device, RmMeshParams, rm_mesh_params_default, rm_mesh, rm_mesh_extract, rm_mesh_from_values, rm_mesh_counts, rm_mesh_timings, RM_MESH_POSITIONS / _NORMALS / _COLOURS / _TRIANGLES / _CELLS, rm_mesh_download, rm_mesh_device_ptr, rm_mesh_destroy, RmMeshSharp, rm_mesh_sharp_default, rm_mesh_extract_sharp, RmMeshKeep, rm_mesh_keep_default, rm_mesh_components, RM_MESH_PART_LABELS / _SIZES, rm_mesh_components_download, rm_mesh_filter, RmMeshSimplify, rm_mesh_simplify_default, rm_mesh_simplify, RmMeshQuadric, rm_mesh_quadric_default, rm_mesh_simplify_quadric, RmMeshOcclusion, rm_mesh_occlusion_default, rm_mesh_occlusion_directions, rm_mesh_occlusion, RmMeshMeasures, rm_mesh_measure, rm_mesh_measure_components, RmMeshSlabs, rm_mesh_slabs_default, rm_mesh_extract_slabs, rm_mesh_extract_sharp_slabs, rm_mesh_from_values_slabs, RmMeshProject, RmMeshProjection, rm_mesh_project_default, rm_mesh_project, RmMeshDeviation, RmMeshDeviationReport, rm_mesh_deviation_default, rm_mesh_deviation_weights, rm_mesh_deviation, RmMeshRefine, RmMeshRefinement, rm_mesh_refine_default, rm_mesh_refine (additions only); 8: RM_PRIM_TORUS / _CYLINDER / _PLANE, RM_OP_SMOOTH_SUBTRACT / _INTERSECT, rm_probe_math (additions only); 7: rm_present_sharded_finish / rm_present_sharded take the size of the host buffer (a changed signature), rm_ctx_set_cull_min_pixels, rm_ctx_set_cull_budget, rm_ctx_cull_stats; 6: rm_present_striped_rows, rm_present_sharded_start / _finish, rm_ctx_last_warning, RM_PROBE_CAST_SHADOW, RM_PRIM_KIND (additions only); 3: rm_ctx_set_sample_batch, rm_buffer_*; 4: rm_ctx_set_gl_stack; 5: RmSurface / RmSceneDesc.surfaces (the struct grew), rm_pack_present_rows, rm_present_sharded, rm_ctx_last_pipeline, RM_RENDER_NO_FAR_JUMP, RM_RENDER_NO_CULL (additions only) */

#define RM_MAX_BOUNCES 10 /* raymarchingStepCountsArray[10], raymarcher.frag:31 */
#define RM_MAX_LIGHTS 10  /* lightPositions[10],             raymarcher.frag:37-39 */
#define RM_MAX_PRIMS 256  /* primitive table rows staged in LDS (32 B each) */

/* status codes */
enum {
  RM_OK = 0,
  RM_ERR_INVALID = 1,  /* bad argument / failed validation (the "compile error" of a scene) */
  RM_ERR_DEVICE = 2,   /* HIP runtime error */
  RM_ERR_NO_DEVICE = 3 /* no usable GPU: the library has NO CPU fallback */
};

/* ---- uniforms ---------------------------------------------------------- */

/*
 * Exactly the uniform block of raymarcher.frag:6-42, as assembled per sample
 * at RenderJobExecutor.tsx:212-297.  `rotation` is column-major like
 * gl.uniformMatrix4fv(..., false, m) (RenderJobExecutor.tsx:293-297).
 * The three sampler uniforms are the framebuffer handle; textureSize() is the
 * framebuffer's full image size.  `reflections` is a float in the reference
 * (loop bound, raymarcher.frag:21,252).  `raymarchingSteps` and
 * `indirectLightingRaymarchingSteps` are set by the reference but never read
 * by the shader (raymarcher.frag:22-23): accepted, unused.
 */
typedef struct RmUniforms {
  float blendWithPreviousFactor;
  float randNoise[2];
  float position[3];
  float rotation[16];
  float dofAmount;
  float dofFocalPlaneDistance;
  int32_t cameraMode; /* 0 perspective, 1 orthographic, 2 panoramic (RenderJobExecutor.tsx:228-232) */
  float fov;          /* fov | orthographic size | 1 (RenderJobExecutor.tsx:233-239) */
  float reflections;
  float raymarchingSteps;
  float indirectLightingRaymarchingSteps;
  float aspect;
  float fogDensity;
  float exposure; /* render.exposure / samplesPerPixel (RenderJobExecutor.tsx:254-256) */
  float raymarchingStepCountsArray[RM_MAX_BOUNCES];
  int32_t blendMode;  /* 1 additive, 0 mix (RenderJobExecutor.tsx:258) */
  int32_t renderMode; /* 1 preview, 0 full (RenderJobExecutor.tsx:259) */
  float lightPositions[RM_MAX_LIGHTS][3];
  float lightColors[RM_MAX_LIGHTS][3];
  float lightSizes[RM_MAX_LIGHTS];
  int32_t lightCount;
  int32_t showDofFocalPlane;
} RmUniforms;

/* ---- scene ------------------------------------------------------------- */

/*
 * The reference's scene is GLSL text defining sdf() and up to seven material
 * functions, spliced into the shader and compiled by the GL driver
 * (RenderJobExecutor.tsx:121-127, Validate.tsx:8-57).  A HIP kernel cannot
 * take GLSL, so the scene crosses this ABI as data: a scene kind (the
 * kernel is specialised per kind), its parameters (the scene's "custom
 * uniforms", RenderJobExecutor.tsx:266), an optional primitive table, and a
 * material block holding the constants of the seven material functions.
 */
enum {
  RM_SCENE_TABLE = 0,          /* fold of primitives with CSG operators; sdfSphere raymarcher.frag:74, sdBox :108, opSmoothUnion examples/smooth-tree.glsl:20-22 */
  RM_SCENE_MANDELBULB = 1,     /* power-n Mandelbulb distance estimator (authored by this project; BASELINE.json configs[2]) */
  RM_SCENE_SPHERE_GRID = 2,    /* examples/guide.glsl:91-102, examples/fractal1.glsl:23-34 */
  RM_SCENE_SPHERE_LATTICE = 3, /* dist/examples/sphere-grid.glsl:42-49 */
  RM_SCENE_MENGER = 4,         /* examples/menger-sponge.glsl:6-23 */
  RM_SCENE_KIFS_TREE = 5,      /* examples/tree.glsl:16-36, examples/smooth-tree.glsl:30-56 */
  RM_SCENE_KIFS_BOX = 6,       /* examples/rotation-fractal.glsl:16-35 */
  RM_SCENE_KIND_COUNT = 7
};

/* Shapes, and the domain operators of the composition API: a domain row produces no distance, it
 * transforms the point at which the FOLLOWING rows are evaluated (and the factor their distances are scaled by):
 *   RM_PRIM_REPEAT  q = mod(q + 0.5 * period, period) - 0.5 * period         period = size[0..2] (> 0); the `repeat`
 *                   of the reference's sphere-grid example (dist/examples/sphere-grid.glsl:42-49)
 *   RM_PRIM_FOLD    q = abs(q / scale) - offset;  q = the three plane rotations by angles;  factor *= scale
 *                   scale = k (> 0), offset = center[0..2], angles = size[0..2] (radians): one level of the
 *                   reference's kaleidoscopic folds (examples/tree.glsl:24-32, rotation-fractal.glsl:21-29)
 * A shape row contributes  shape(q) * factor.
 *   RM_PRIM_KIND    (ABI 6) a SHAPE row whose distance term is a scene kind's own estimator, so that a composition like "a
 *                   Mandelbulb cut by a box" or "a lattice of spheres inside a ball" is table data and not a new kind
 *                   (the reference takes any GLSL sdf(): RenderJobExecutor.tsx:121-127):  kind(q - center)  with
 *                   kind = (int)size[0] one of RM_SCENE_MANDELBULB, RM_SCENE_SPHERE_LATTICE and the kind's parameters in
 *                   RmSceneDesc.params (its own slots: one kind per table, any number of rows of it).  Operator, k and
 *                   surface as for a sphere or a box.  A table with such a row renders with the pixel kernel, without the
 *                   far-field exits and the row culling (both are arguments about spheres and boxes).
 *   (ABI 8) three more shapes and the smooth forms of the other two operators -- the vocabulary a scene author composes with next
 *   to sphere / box / smooth union (the reference's helper set is those three: raymarcher.frag:74,:108, smooth-tree.glsl:20-22; any
 *   other shape is GLSL of the author's own, which cannot cross this ABI).  About the row's centre c, axis y:
 *   RM_PRIM_TORUS     length(vec2(length((q - c).xz) - R, (q - c).y)) - r                R = size[0], r = size[1]
 *   RM_PRIM_CYLINDER  capped: dx = length((q - c).xz) - r, dy = |(q - c).y| - h;          r = size[0], h = size[1]
 *                     min(max(dx, dy), 0) + length(max(vec2(dx, dy), 0))
 *   RM_PRIM_PLANE     dot(q - c, n)                                                      n = size[0..2] (the caller's unit normal)
 *   RM_OP_SMOOTH_SUBTRACT   h = clamp(0.5 - 0.5 (d + di) / k, 0, 1);  mix(d, -di, h) + k h (1 - h)      (k > 0)
 *   RM_OP_SMOOTH_INTERSECT  h = clamp(0.5 - 0.5 (d - di) / k, 0, 1);  mix(d,  di, h) + k h (1 - h)
 *   A table with one of these renders with the general fold, step by step: the far-field exits and the row culling are
 *   arguments about spheres, boxes and the four older operators. */
enum { RM_PRIM_SPHERE = 0, RM_PRIM_BOX = 1, RM_PRIM_REPEAT = 2, RM_PRIM_FOLD = 3, RM_PRIM_KIND = 4, RM_PRIM_TORUS = 5, RM_PRIM_CYLINDER = 6, RM_PRIM_PLANE = 7 };
enum { RM_OP_UNION = 0, RM_OP_SMOOTH_UNION = 1, RM_OP_SUBTRACT = 2, RM_OP_INTERSECT = 3, RM_OP_SMOOTH_SUBTRACT = 4, RM_OP_SMOOTH_INTERSECT = 5 };

/* One row of the primitive table, 32 bytes.  The scene distance is the left
 * fold  d = shape[0];  d = op_i(d, shape[i])  over the shape rows, in table order
 * (the operator of the first shape row is ignored); at least one row must be a shape. */
typedef struct RmPrim {
  int32_t type; /* RM_PRIM_* in bits 0..7, RM_OP_* in bits 8..15, surface index of a shape row in bits 16..23 (RmSurface) */
  float k;      /* smooth-union radius */
  float center[3];
  float size[3]; /* sphere: size[0] = radius; box: half extents; repeat: period; fold: angles; kind: size[0] = the RM_SCENE_* kind;
                    torus: R, r; cylinder: r, half height; plane: unit normal */
} RmPrim;

/* parameter slots of RmSceneDesc.params per kind */
enum {
  /* RM_SCENE_MANDELBULB */
  RM_P_BULB_POWER = 0, RM_P_BULB_ITERATIONS = 1, RM_P_BULB_BAILOUT = 2,
  /* RM_SCENE_SPHERE_GRID: bigSphereSize, fractalIterations, gridScaleFactor, bigSphereCenter.xyz */
  RM_P_GRID_BIG_SIZE = 0, RM_P_GRID_ITERATIONS = 1, RM_P_GRID_SCALE = 2, RM_P_GRID_CENTER = 3,
  /* RM_SCENE_SPHERE_LATTICE: period, radius */
  RM_P_LATTICE_PERIOD = 0, RM_P_LATTICE_RADIUS = 1,
  /* RM_SCENE_MENGER: fractalIterations */
  RM_P_MENGER_ITERATIONS = 0,
  /* RM_SCENE_KIFS_TREE / RM_SCENE_KIFS_BOX: fractalIterations, scaleFactor, angles.xyz, offset, smoothen */
  RM_P_KIFS_ITERATIONS = 0, RM_P_KIFS_SCALE = 1, RM_P_KIFS_ANGLES = 2, RM_P_KIFS_OFFSET = 5, RM_P_KIFS_SMOOTH = 6
};

/* Constants of the seven material functions (Validate.tsx:18-51 are the
 * defaults; examples override some).  colour = value inside `*_cutoff`,
 * 0 outside (length(position) > cutoff). */
typedef struct RmMaterial {
  float diffuse[3];
  float diffuse_cutoff;
  float specular[3];
  float specular_cutoff;
  float roughness;
  float subsurface;
  float subsurface_color[3];
  float ior;
  /* emission = sky_color * max(normalize(p)[sky_axis], sky_floor) * sky_scale  where length(p) > sky_radius, else 0 */
  float sky_color[3];
  float sky_floor;
  float sky_scale;
  float sky_radius;
  int32_t sky_axis;
  int32_t reserved;
} RmMaterial;

/* Position-dependent materials of a composed scene.  The reference's contract is seven FUNCTIONS of position
 * (Validate.tsx:18-51; examples/guide.glsl:51-88 writes its own); a primitive table gets them per shape: a shape row
 * names a surface (RmPrim.type bits 16..23: 0 = the scene's RmMaterial block, k = surfaces[k - 1]) and the material
 * functions at `position` return the values of the shape row whose distance there -- the row's own term of the fold,
 * domain rows applied, before its operator -- is the smallest (the earliest such row on a tie, a NaN distance never
 * wins); the cut-off radii and the sky (emission) stay the scene's.  The composer emits the same rule as GLSL
 * (scene.py / js/index.js: rmSurfaceIndex + the seven functions), which is what pins it against the reference's shader. */
#define RM_MAX_SURFACES 15
typedef struct RmSurface {
  float diffuse[3];
  float roughness;
  float specular[3];
  float subsurface;
  float subsurface_color[3];
  float ior;
} RmSurface;

typedef struct RmSceneDesc {
  int32_t kind;
  int32_t nprims;
  const RmPrim* prims; /* host pointer, nprims rows (RM_SCENE_TABLE only) */
  float params[16];
  RmMaterial material;
  int32_t nsurfaces;         /* 0..RM_MAX_SURFACES (RM_SCENE_TABLE only) */
  int32_t reserved;
  const RmSurface* surfaces; /* host pointer, nsurfaces entries, or NULL */
} RmSceneDesc;

/* Fills *m with the reference defaults of Validate.tsx:18-51. */
RM_API void rm_material_default(RmMaterial* m);

/* ---- handles ----------------------------------------------------------- */

typedef struct rm_ctx rm_ctx;
typedef struct rm_scene rm_scene;
typedef struct rm_fb rm_fb;

typedef struct RmRect {
  int32_t x, y, w, h; /* pixels, origin bottom-left like gl.scissor */
} RmRect;

/* render flags */
enum {
  RM_RENDER_STRICT = 0,      /* fixed step counts, IEEE division/sqrt, no contraction: the parity build */
  RM_RENDER_FAST = 1,        /* hardware-rate math in the distance evaluations; same image statistics, not the same bits */
  RM_RENDER_COLOR_ONLY = 2,  /* do not read/write the two G-buffer planes (benchmark "single colour frame" mode) */
  RM_RENDER_MEGAKERNEL = 4,  /* force the one-thread-one-pixel kernel (whole main() per thread) */
  RM_RENDER_WAVEFRONT = 16,  /* NOT in this library since round 5 (RM_ERR_INVALID): the wavefront pipeline -- the same per-pixel program cut
                                at its marches into queue-driven stages -- is the tests' second implementation and is compiled into
                                their cross-check build of these sources only (tests/_xcheck/libhip_raymarch_xcheck.so, -DRM_WITH_WAVEFRONT=1;
                                rm_api.hip says why).  There the flag is a request: tables with surfaces or kind rows take the pixel
                                kernel whatever is asked (rm_ctx_last_pipeline tells).  The product's own cross-check of its exact
                                shortcuts is the stepwise march: RM_RENDER_NO_FAR_JUMP | RM_RENDER_NO_CULL (same bits). */
  RM_RENDER_NO_COST_CLASSES = 8, /* (cross-check build) wavefront march in one pass even for scene kinds whose sdf cost depends on the
                                   point (Mandelbulb); a measurement switch, same results */
  RM_RENDER_NO_OVERLAP = 32, /* this sample runs alone on the context's stream and blends in its own kernel (see
                                rm_ctx_set_samples_in_flight); for timing one launch.  Same results. */
  RM_RENDER_NO_FAR_JUMP = 64, /* RM_RENDER_FAST, bounded scenes (Mandelbulb, tables without domain rows, the sponge, the
                                rotation and sphere-grid fractals): march an escaping ray step by step instead of setting
                                it to the end state its remaining steps are known to reach (castRay, raymarcher.frag:163-170,
                                has no distance bound: such a ray overflows to a fixed +-Inf / NaN pattern) -- also a ray that
                                is certain to miss the scene, or every shape of a long table -- and a long table's shadow ray
                                that escapes with too few steps left for the overflow is marched to the end instead of being
                                stopped once its comparison (raymarcher.frag:362-363) is certain.  A measurement and test
                                switch: the same bits in every plane either way. */
  RM_RENDER_NO_CULL = 128     /* long primitive tables (no domain rows): evaluate every row of the table at every point instead of
                                the rows the point's grid cell lists.  A row that is an exact no-op everywhere in the cell is
                                skipped: min(d, di) with the shape further away than the running value, max(d, +-di) with the term
                                below it; and a far smooth-union row whose rounding of the running value -- d' = fl(di -
                                fl(di - d)), what mix(di, d, 1) does -- is provably the identity because d already lies on a
                                grid at least as coarse.  Other smooth-union rows are never skipped.
                                Both builds since round 4 (the parity build's GL-stack arithmetic folds every row).  A measurement
                                and test switch: the same bits either way. */
};

enum { RM_PLANE_COLOR = 0, RM_PLANE_NORMAL_DOF = 1, RM_PLANE_ALBEDO_DEPTH = 2 };

/* ---- context ----------------------------------------------------------- */

/* Replaces loadRenderJobContext(gl) (LoadRenderJobContext.tsx:268-287): binds
 * a device, creates the stream the launches go to.  Fails with
 * RM_ERR_NO_DEVICE when there is no GPU -- there is no CPU path. */
RM_API int rm_ctx_create(int device, rm_ctx** out);
RM_API void rm_ctx_destroy(rm_ctx* ctx);
/* Text of the last error on this context ("" if none); ctx may be NULL for
 * errors of rm_ctx_create itself.  Replaces ShaderError.infoLog. */
RM_API const char* rm_last_error(const rm_ctx* ctx);
/* Use an externally owned hipStream_t (e.g. torch's current stream) for all
 * later launches; NULL restores the context's own stream.  The switch is
 * ordered on the device (an event, no host wait): work this library queued on
 * the old stream -- the zeroing of rm_fb_create / rm_fb_clear, uploads,
 * renders -- completes before anything enqueued on the new stream after the
 * call.  The old stream must still exist when this is called. */
RM_API int rm_ctx_set_stream(rm_ctx* ctx, void* hip_stream);
/* Samples in flight (default 3, 1 = off; environment RM_SAMPLES_IN_FLIGHT).  The reference submits its draw calls
 * back to back (RenderJobExecutor.tsx:240-260) and the GPU overlaps them; here a full-mode sample of the pixel
 * kernel renders on an internal side stream into a staging buffer (it reads no plane) and a small kernel on the
 * context's stream blends it into the planes, in call order, so up to n consecutive rm_render_sample(s) calls
 * overlap.  Every call is still ordered on the context's stream as far as the planes are concerned: work enqueued
 * there afterwards sees the sample blended.  The planes receive the same bits as without overlap.  Costs 3 planes
 * of staging per sample in flight. */
RM_API int rm_ctx_set_samples_in_flight(rm_ctx* ctx, int n);
/* Advice that came with the last rm_ctx_set_samples_in_flight that SUCCEEDED ("" = none): the process environment
 * (GPU_MAX_HW_QUEUES < 8, read by the HIP runtime when it starts) will keep the samples from overlapping.  Not an
 * error: rm_last_error is for failures only.  The pointer stays valid until the next such call on the context. */
RM_API const char* rm_ctx_last_warning(const rm_ctx* ctx);
/* Samples per launch of rm_render_samples (default 0 = automatic, 1 = one launch per sample, 2..8 = fixed).  A small
 * window -- one GPU's rows of a sharded frame -- has too few workgroups to keep the chip busy to the end of a launch
 * (a ray is a serial chain of ~1 ms); rm_render_samples therefore renders up to 8 consecutive samples of the job in
 * ONE launch, a workgroup per (tile, sample), each sample staged separately and blended into the planes in sample
 * order by one small kernel -- the same bits as one launch per sample.  Automatic = as many as bring the launch to
 * about 16 384 workgroups (a whole 3840x2160 frame has 16 320, so whole frames are not batched), within a staging
 * budget of a quarter of the device's free memory.  Staging costs 48 bytes per pixel of the TILE a launch renders, per
 * sample of a batch and per launch in flight; a launch whose staging cannot be allocated renders unstaged (same bits). */
RM_API int rm_ctx_set_sample_batch(rm_ctx* ctx, int n);
/* Cost-ordered dispatch (default on; environment RM_COST_ORDER=0 turns it off).  From the second sample of a job on
 * (same framebuffer window, tile and scene kind, >= 512 workgroups), the pixel kernel starts its tiles in the order of
 * their cost in the previous sample, most expensive first, so that a launch does not end on a few late, long
 * workgroups.  Scheduling only: the planes receive the same bits. */
RM_API int rm_ctx_set_cost_order(rm_ctx* ctx, int on);
/* RM_RENDER_FAST only, opt-in: a marching lane counts as settled once its step
 * |d| <= eps * max(1, |p|_inf).  The default is 0: only the exact test
 * (position bitwise unchanged), which is what RM_RENDER_STRICT always uses.
 * A tolerance is NOT neutral for the image: rays stop a few ulps above the
 * surface, where the forward-difference normals (delta = 1e-5) are less noisy
 * than at the reference's fixed point, and lit pixels come out brighter --
 * Mandelbulb, 32 spp, mean of the lit pixels against the parity build:
 * eps 2^-25 +0.7 %, 2^-24 +2.9 %, 2^-23 +4.7 %, 2^-21 +6.8 %, 1e-5 +14 %, for
 * 1 %, 3 %, 8 %, 12 % and 28 % less time (tools/eps_study.py). */
RM_API int rm_ctx_set_retire_eps(rm_ctx* ctx, float eps);
/* Parity mode of the strict build: on != 0 makes everything this context does WITHOUT RM_RENDER_FAST -- rm_render_sample(s),
 * rm_probe*, rm_present* -- compute in the arithmetic of the GL stack the reference's golden images were rendered under
 * (SwiftShader as shipped in HeadlessChrome 88): its sin / cos / log / exp / pow / acos / atan as IEEE operation sequences,
 * min / max as x86 computes them, fract clamped below 1, the canvas's unorm conversion through 16 bits.  GLSL leaves all of
 * these to the implementation (raymarcher.frag has one value only together with a GL stack); with this switch the GPU
 * reproduces tests/golden/ -- distances, marches, whole main() images, the present pass -- bit for bit.  The pixel kernel
 * only (the wavefront pipeline is not built in this arithmetic); slower than the default strict arithmetic's IEEE-derived
 * shortcuts allow.  Off by default.  on == 2 additionally replaces the portable tangent (the fixed operation sequence every
 * other arithmetic of this library uses for tan(), see RmUniforms / DESIGN.md) by that stack's own tan = sin / cos: what the
 * reference's UNMODIFIED shader text computes under it, random stream and camera included (that switch is one per DEVICE:
 * the GL-stack contexts of a device share it, and changing it waits for the device). */
RM_API int rm_ctx_set_gl_stack(rm_ctx* ctx, int on);
/* Culling grids (long primitive tables without domain rows; RM_RENDER_NO_CULL): a scene's grid is built -- on a stream of
 * the context's own, with no wait on the host; the render that asks for it waits for the build on the device -- once the
 * scene has been asked for `pixels` pixel-samples since it was created (default 4 Mi: a 4K frame's first sample builds it,
 * a host that shows a NEW scene in every 1080p frame, like the reference's sliders do (index.tsx:121-182), never pays for a
 * grid it would not earn back); 0 = with the first render.  Counted per JOB: every sample of an rm_render_samples call, and
 * a striped framebuffer's part of a frame as the whole frame (every rank of a sharded job reaches the threshold when a
 * single GPU would).  The same bits with and without a grid.  rm_ctx_cull_stats: out4 = {grids built so far, bytes the
 * scenes' grids hold now, grids held now, the budget in bytes (a sixteenth of the device's memory, at most 1 GiB: beyond it
 * the least recently rendered scene gives its grid up and renders on without one; a grid larger than the whole budget is
 * not built until the budget is raised)}.  Buffers of grids that were given up are kept for the next build (at most 4, at
 * most half the budget) and count against the budget: grids + recycled buffers never exceed it.  Lowering the budget
 * (rm_ctx_set_cull_budget) takes effect at once. */
RM_API int rm_ctx_set_cull_min_pixels(rm_ctx* ctx, long long pixels);
RM_API int rm_ctx_set_cull_budget(rm_ctx* ctx, size_t bytes); /* the bytes a context's grids may hold (a host that knows its memory better; the tests: small, to see grids go) */
RM_API int rm_ctx_cull_stats(const rm_ctx* ctx, unsigned long long* out4);
/* Diagnostics of the wavefront march, filled only by builds compiled with
 * -DRM_WF_STATS (zeros otherwise): out16[8*shadow + 4*pass2 + {0,1,2}] =
 * rays marched, lane-steps, wave-steps since the last reset. */
RM_API int rm_debug_counters(rm_ctx* ctx, unsigned long long* out16, int reset);

/* Debug (tests): the rows of a primitive table (no domain rows) that an evaluation anywhere in the ball (centre, radius) has
 * to fold -- what the culling grid stores per cell (RM_RENDER_NO_CULL) -- as (nprims + 63) / 64 64-bit words,
 * bit i = row i stays (row 0 always does); `margin` = the allowance for fp32 rounding (0 tests the rule in
 * exact arithmetic).  Host arithmetic:
 * needs no GPU and no context.  Returns RM_ERR_INVALID for a table with domain rows. */
RM_API int rm_debug_cull_cell(const RmSceneDesc* desc, const double* centre, double radius, double margin, unsigned long long* out_words);
/* Which implementation of the per-pixel program the LAST rm_render_sample(s) / rm_render_timed call on this context
 * dispatched (the library picks per job unless a flag forces one; same results either way): what a host reports next to a
 * timing instead of re-deriving the library's rule. */
enum { RM_PIPELINE_NONE = 0, RM_PIPELINE_PIXEL_KERNEL = 1, RM_PIPELINE_WAVEFRONT = 2 };
RM_API int rm_ctx_last_pipeline(const rm_ctx* ctx);
/* Free and total memory of the context's GPU (hipMemGetInfo): what a host sizes its frames against -- the planes of
 * a W x H frame take 48 W H bytes, staging 48 W H per sample in flight or in a batch, the wavefront pipeline 240 bytes
 * per pixel of a launch (the reference asks MAX_TEXTURE_SIZE instead). */
RM_API int rm_device_memory(rm_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
/* Completion point: the reference's generator yield / present cadence
 * (RenderJobExecutor.tsx:163-166) maps to "enqueue samples, rm_sync, present". */
RM_API int rm_sync(rm_ctx* ctx);
RM_API int rm_abi_version(void);

/* ---- scene ------------------------------------------------------------- */

/* Replaces programCache.getProgram(vert, frag-with-scene)
 * (RenderJobExecutor.tsx:121-127, ShaderCache.tsx:91-119): validates the
 * description (the analogue of a GLSL compile) and uploads the primitive
 * table.  On failure returns RM_ERR_INVALID and rm_last_error() is the
 * "info log". */
RM_API int rm_scene_create(rm_ctx* ctx, const RmSceneDesc* desc, rm_scene** out);
RM_API void rm_scene_destroy(rm_scene* scene);

/* ---- framebuffers ------------------------------------------------------ */

/* Replaces context.fbo.create(w, h, frameid) (LoadRenderJobContext.tsx:186-223):
 * three accumulation planes of float4 per pixel (color RGBA, normal+dofRadius,
 * albedo+depth; raymarcher.frag:70-72).  The reference ping-pongs prev/curr
 * and copies curr->prev after every draw (RenderJobExecutor.tsx:301-326);
 * here each pixel is read and written by the one thread that owns it, so a
 * single in-place set is the same result.  The frame may be a window of rows
 * [row_begin, row_begin+row_count) of a width x height image (row sharding
 * across GPUs): pixel coordinates, texcoord and aspect stay global.
 * Planes are zero-initialised.  Row 0 is the BOTTOM row (GL convention). */
RM_API int rm_fb_create(rm_ctx* ctx, int width, int height, int row_begin, int row_count, rm_fb** out);
/* Row-striped window for sharding one image over several GPUs with balanced
 * cost: the frame is cut into stripes of `stripe_rows` rows and this
 * framebuffer holds, packed in ascending order, the stripes k with
 * k % parts == part (rows r with (r / stripe_rows) % parts == part).
 * rm_fb_rows() tells how many rows that is.  Planes may be caller-owned
 * (non-NULL color; normal_dof/albedo_depth both or neither) or NULL to let the
 * library allocate them.  Pixel coordinates stay global as in rm_fb_create. */
RM_API int rm_fb_create_striped(rm_ctx* ctx, int width, int height, int stripe_rows, int parts, int part,
                         void* color, void* normal_dof, void* albedo_depth, rm_fb** out);
/* Number of image rows a framebuffer holds; width / height of the image it is a window of. */
RM_API int rm_fb_rows(const rm_fb* fb);
RM_API int rm_fb_width(const rm_fb* fb);
RM_API int rm_fb_height(const rm_fb* fb);
/* Same, but over caller-owned device memory (e.g. torch tensors): each plane
 * pointer addresses row_count*width float4; normal_dof/albedo_depth may be
 * NULL (then only RM_RENDER_COLOR_ONLY renders are accepted). */
RM_API int rm_fb_wrap(rm_ctx* ctx, int width, int height, int row_begin, int row_count,
               void* color, void* normal_dof, void* albedo_depth, rm_fb** out);
/* The clear-on-new-frameid of LoadRenderJobContext.tsx:196-208. */
RM_API int rm_fb_clear(rm_fb* fb);
RM_API void rm_fb_destroy(rm_fb* fb);
/* Copies one plane (row_count*width*4 floats) to / from host memory; synchronous. */
RM_API int rm_fb_download(rm_fb* fb, int plane, float* host);
RM_API int rm_fb_upload(rm_fb* fb, int plane, const float* host);
/* Device address of a plane (for collectives / zero-copy wrapping). */
RM_API void* rm_fb_device_ptr(rm_fb* fb, int plane);

/* (ABI 9) The format of the G-buffer planes.  LoadRenderJobContext.tsx:81-119 allocates colour as RGBA32F and
 * normal + DoF radius and albedo + depth as RGBA16F; the framebuffers above keep all three planes in fp32, which is what
 * the reference computes on the software GL stack its golden images were rendered under (and stays the default).
 * RM_GBUFFER_F16 stores planes 1 and 2 as 4 x IEEE binary16 per pixel (8 bytes, RGBA; rows as for fp32) and
 * accumulates them as raymarcher.frag:347-351 does with an RGBA16F attachment: the stored value widened to fp32, the
 * sample's contribution added in fp32, the sum rounded to binary16 to nearest even (overflow to +-inf, subnormals kept),
 * after EVERY sample, whatever the batching.  So a pixel's summed normal stops at 2048 and a sky pixel's depth is +inf,
 * as the reference's users see them.  The colour plane is float4 in both formats.  A frame is 64 bytes per pixel
 * instead of 96.  A render that writes a half G-buffer is always staged (the samples-in-flight staging, 48 bytes per
 * pixel of the tile per sample; one slot under RM_RENDER_NO_OVERLAP): when that staging cannot be allocated the call
 * fails with RM_ERR_DEVICE instead of rendering unstaged -- render in tiles.  RM_RENDER_WAVEFRONT (the tests'
 * cross-check library) renders a half G-buffer with the pixel kernel (rm_ctx_last_pipeline tells). */
enum { RM_GBUFFER_F32 = 0, RM_GBUFFER_F16 = 1 };
/* rm_fb_create / rm_fb_create_striped / rm_fb_wrap with a G-buffer format.  Caller-owned half planes address
 * row_count*width*8 bytes and are 8-byte aligned (colour: float4, 16-byte aligned).  An unknown format or a misaligned
 * plane is RM_ERR_INVALID. */
RM_API int rm_fb_create_fmt(rm_ctx* ctx, int width, int height, int row_begin, int row_count, int gbuffer, rm_fb** out);
RM_API int rm_fb_create_striped_fmt(rm_ctx* ctx, int width, int height, int stripe_rows, int parts, int part,
                             void* color, void* normal_dof, void* albedo_depth, int gbuffer, rm_fb** out);
RM_API int rm_fb_wrap_fmt(rm_ctx* ctx, int width, int height, int row_begin, int row_count,
                   void* color, void* normal_dof, void* albedo_depth, int gbuffer, rm_fb** out);
/* The G-buffer format of a framebuffer (RM_GBUFFER_F32 for every framebuffer made without one). */
RM_API int rm_fb_gbuffer(const rm_fb* fb);
/* A plane's bytes as stored, either format: `bytes` must be exactly row_count*width*16 (colour, fp32 G-buffer) or
 * row_count*width*8 (half G-buffer), else RM_ERR_INVALID.  Synchronous.  rm_fb_download / rm_fb_upload keep working on
 * half planes: the download widens exactly, the upload rounds to nearest even on the device, as the render kernels do.
 * rm_fb_device_ptr of a half plane addresses binary16 data.  The raw-pointer entry points (rm_present_planes,
 * rm_present_device, rm_present_striped_rows, rm_assemble_striped) take fp32 planes only: a framebuffer with the half
 * G-buffer reaches them through rm_pack_present_rows, whose output is float4 in either format; rm_present,
 * rm_present_rows, rm_pack_present_rows and rm_present_sharded* take either. */
RM_API int rm_fb_download_raw(rm_fb* fb, int plane, void* host, size_t bytes);
RM_API int rm_fb_upload_raw(rm_fb* fb, int plane, const void* host, size_t bytes);

/* (ABI 9) The moments plane (opt-in): RM_FB_MOMENTS OR'ed into rm_fb_create_fmt's `gbuffer` argument gives an owned
 * framebuffer a fourth plane, RM_PLANE_MOMENTS, of 2 x fp32 per pixel (8 bytes, rows as the other planes) in either
 * G-buffer format: (sum l, sum l^2), where l is the luminance of one sample's colour contribution (the staged
 * light * exposure, c), computed in fp32 in exactly this order, every product and sum rounded on its own, no contraction:
 *   l = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 * It is blended by the colour plane's rule: (M.x + l, M.y + l * l) in additive mode, and in mix mode
 * (f * (M.x - l) + l, f * (M.y - l * l) + l * l) with the colour's factor f.  Like the half G-buffer it is written only by
 * rm_combine_kernel, so a render into a framebuffer with moments that writes the G-buffer (full mode, at least one
 * bounce, not RM_RENDER_COLOR_ONLY) is always staged (one slot under RM_RENDER_NO_OVERLAP) and fails with RM_ERR_DEVICE
 * when the staging cannot be allocated; other renders (preview mode, colour only) leave the plane as it is.  Created
 * zero-filled and cleared by rm_fb_clear.  rm_fb_download_raw / rm_fb_upload_raw take plane 3 with exactly
 * row_count*width*8 bytes and rm_fb_device_ptr(fb, 3) addresses it; without moments plane 3 is RM_ERR_INVALID / NULL.
 * rm_fb_download / rm_fb_upload stay planes 0..2.  rm_fb_create_striped_fmt and rm_fb_wrap_fmt refuse the flag
 * (RM_ERR_INVALID): the variance-guided denoiser, its only reader, needs a whole frame. */
#define RM_FB_MOMENTS 0x100
enum { RM_PLANE_MOMENTS = 3 };
/* 1 when the framebuffer has the moments plane, else 0 (NULL included). */
RM_API int rm_fb_has_moments(const rm_fb* fb);

/* Raw device memory for hosts that have no allocator of their own: rm_present_rows, rm_present_device and
 * rm_assemble_striped_bytes take DEVICE pointers (in the reference these are textures the GL context owns,
 * LoadRenderJobContext.tsx:43-124; a torch host passes tensor addresses instead).  Created zero-filled; the copies
 * take the buffer's base address and at most its size, are synchronous and ordered after the work on the context's
 * stream; rm_ctx_destroy frees what is left. */
RM_API int rm_buffer_create(rm_ctx* ctx, size_t bytes, void** device_ptr);
RM_API int rm_buffer_destroy(rm_ctx* ctx, void* device_ptr);
RM_API int rm_buffer_download(rm_ctx* ctx, const void* device_ptr, void* host, size_t bytes);
RM_API int rm_buffer_upload(rm_ctx* ctx, void* device_ptr, const void* host, size_t bytes);

/* ---- the hot path ------------------------------------------------------ */

/* One sample of every pixel of `tile` (clipped to the framebuffer's rows):
 * replaces  bind prev -> setUniforms -> gl.drawArrays -> blit
 * (RenderJobExecutor.tsx:195-326) = one run of raymarcher.frag main()
 * (raymarcher.frag:178-388) per pixel.  tile == NULL means the whole window.
 * Asynchronous on the context's stream. */
RM_API int rm_render_sample(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* uniforms,
                     const RmRect* tile, int flags);

/* `count` samples back to back, sample i using randNoise[i] (pairs); every
 * other uniform as given: the sample loop of a render job
 * (RenderJobExecutor.tsx:160-222 -- only randNoise changes from sample to
 * sample).  Same planes, bit for bit, as `count` calls of rm_render_sample;
 * full-mode samples of the pixel kernel go out several to a launch (see
 * rm_ctx_set_sample_batch). */
RM_API int rm_render_samples(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* uniforms,
                      const float* rand_noise_pairs, int count, const RmRect* tile, int flags);

/* Like rm_render_samples with one fixed randNoise, but brackets the `count`
 * launches with HIP events on the context's stream and returns the average
 * kernel time per launch in *ms_per_launch (synchronous). */
RM_API int rm_render_timed(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* uniforms,
                    int count, const RmRect* tile, int flags, float* ms_per_launch);

/* ---- probes (RNG-free building blocks of the path) --------------------- */

/* The reference's own functions evaluated on caller-supplied inputs, the
 * device analogue of the harness main() used to generate the goldens.
 * All buffers are HOST pointers; synchronous.
 *   RM_PROBE_SDF      in: n x float3 p                  out: n x float   sdf(p)            (scene text / examples)
 *   RM_PROBE_CAST_RAY in: n x (float3 p, float3 dir)    out: n x float3  castRay(p,dir,steps)   raymarcher.frag:163-170
 *   RM_PROBE_NORMAL   in: n x float3 p                  out: n x float3  sceneNormal(p, delta)  raymarcher.frag:153-160
 *   RM_PROBE_MATERIAL in: n x float3 p                  out: n x 12 floats diffuse,specular,emission,(roughness,subsurface,ior)
 *   RM_PROBE_CAST_STEPS in: n x (float3 p, float3 dir)  out: n x float   number of castRay steps after which the ray's
 *                                                       position no longer changes bitwise (= steps if it never settles);
 *                                                       a measurement aid for the wave-retire, not a reference function
 *   RM_PROBE_CAST_SHADOW in: n x (float3 p, float3 dir, float3 light)  out: n x float  1 if the light is seen, else 0: the shadow
 *                                                       test of one light, distance(castRay(p, dir, steps), light) >= distance(p, light)
 *                                                       (raymarcher.frag:362-363), marched as the pixel kernel marches a shadow ray
 * A table of 16 rows or more is marched as its pixel kernels march it (the long tables' far-field exits included).
 */
enum { RM_PROBE_SDF = 0, RM_PROBE_CAST_RAY = 1, RM_PROBE_NORMAL = 2, RM_PROBE_MATERIAL = 3, RM_PROBE_CAST_STEPS = 4, RM_PROBE_CAST_SHADOW = 5 };
RM_API int rm_probe(rm_ctx* ctx, rm_scene* scene, int what, const float* in, int n, float param,
             int flags, float* out);

/* Camera block of main() without jitter or depth of field
 * (raymarcher.frag:186-205 with randomDirectionOffset = dofOffset = 0):
 * out = height*width x 8 floats (origin.xyz, deltaZ, dir.xyz, 0), HOST pointer. */
RM_API int rm_probe_camera(rm_ctx* ctx, const RmUniforms* uniforms, int width, int height, float* out);

/* The per-pixel random stream (raymarcher.frag:46-49,78-101): for each pixel
 * of a width x height image the first `count` values of uniformSample().
 * out = height*width*count floats, HOST pointer. */
RM_API int rm_probe_rng(rm_ctx* ctx, const RmUniforms* uniforms, int width, int height, int count, float* out);

/* The transcendental functions of the parity arithmetic on arrays, as the kernels call them: the fp32 sequences of
 * csrc/rm_pm_math.hpp (the text of oracle/pm_math.h), or the GL stack's (rm_ss_math.hpp = oracle/ss_math.h) on a context
 * with rm_ctx_set_gl_stack -- so that "the same bits as the oracle" is tested function by function on millions of
 * arguments, not only through rendered frames.  POW is pow(|a|, b) (the oracle's gl_pow), ATAN2 atan(a, b) with a = y,
 * TAN the portable tangent of the random stream and camera (oracle/rm_oracle.c or_tan); POW_PAIR_NM1 / _N are
 * pow(a, b - 1) / pow(a, b) from one logarithm and SINCOS_S / _C sin / cos from one reduction, the shared forms the
 * Mandelbulb uses (they must have the bits of the separate calls).  a, b, out: HOST pointers to n floats; b may be NULL
 * for the functions of one argument.  Test infrastructure like rm_probe: no part of a render job calls it. */
enum { RM_MATH_SIN = 0, RM_MATH_COS = 1, RM_MATH_LOG = 2, RM_MATH_EXP = 3, RM_MATH_POW = 4, RM_MATH_ACOS = 5, RM_MATH_ATAN2 = 6, RM_MATH_TAN = 7,
       RM_MATH_POW_PAIR_NM1 = 8, RM_MATH_POW_PAIR_N = 9, RM_MATH_SINCOS_S = 10, RM_MATH_SINCOS_C = 11, RM_MATH_SQRT = 12, RM_MATH_DIV = 13, RM_MATH_COUNT = 14 };
RM_API int rm_probe_math(rm_ctx* ctx, int fn, const float* a, const float* b, int n, float* out);

/* ---- assembling a sharded frame ------------------------------------------ */

/* Puts the planes of a frame that was rendered as `parts` striped windows (rm_fb_create_striped: stripes of
 * `stripe_rows` rows dealt round-robin) back into image order, in one launch on the context's stream.
 * src: DEVICE pointer to parts x max_rows x width float4 (the gathered planes, part p at p * max_rows * width;
 * a part's rows beyond its own count are padding), dst: DEVICE pointer to height x width float4.  What a
 * multi-GPU host runs on the rank that shows the frame, after the gather (raymarching_engine_amd/dist.py).
 * hip_stream: the hipStream_t to launch on, NULL = the context's stream (a host that keeps rendering while the
 * frame is put together gives it a stream of its own, ordered after the gather). */
RM_API int rm_assemble_striped(rm_ctx* ctx, const void* src, int parts, int max_rows, int width, int height, int stripe_rows, void* dst,
                        void* hip_stream);
/* The same for rows of `row_bytes` opaque bytes (a multiple of 4; buffers 16-byte aligned): RGBA8 rows after the
 * per-rank present (rm_present_rows, row_bytes = 4 * width), or any other per-pixel payload. */
RM_API int rm_assemble_striped_bytes(rm_ctx* ctx, const void* src, int parts, int max_rows, long long row_bytes, int height, int stripe_rows,
                              void* dst, void* hip_stream);

/* ---- present ----------------------------------------------------------- */

/* The present pass of the reference (display.frag:16-64, driven from
 * index.tsx:25-59): colour x 1/samples, Gaussian blur whose radius is the
 * accumulated DoF radius (normal_dof.w / samples x 200, clamped to 16 pixels;
 * NEAREST + REPEAT taps), gamma 1/2.2, RGBA8.  out_rgba8 = height*width*4
 * bytes, HOST pointer, row 0 = bottom row.  The blur reads neighbouring rows,
 * so rm_present needs a framebuffer holding the whole frame; for a sharded
 * frame gather the planes first and use rm_present_planes (device pointers;
 * normal_dof may be NULL = no blur). */
RM_API int rm_present(rm_ctx* ctx, rm_fb* fb, int samples, uint8_t* out_rgba8);
RM_API int rm_present_planes(rm_ctx* ctx, const void* color, const void* normal_dof, int width, int height, int samples, uint8_t* out_rgba8);
/* The same pass left on the device and asynchronous: out_rgba8_device = height*width*4 bytes of DEVICE memory,
 * launched on hip_stream (NULL = the context's stream); no allocation, no host wait.  For a host that shows the
 * frame from device memory or reads it back itself (index.tsx:25-59 draws straight to the canvas). */
RM_API int rm_present_device(rm_ctx* ctx, const void* color, const void* normal_dof, int width, int height, int samples,
                      void* out_rgba8_device, void* hip_stream);
/* The present pass of the rows ONE framebuffer window holds, for jobs without depth of field (dof.amount = 0: the
 * blur radius of display.frag:24-27 is 0 and its only tap is the pixel itself, so no neighbour row is needed and
 * the bytes equal rm_present's).  out_rgba8_device = rm_fb_rows(fb)*width*4 bytes of DEVICE memory, in the
 * window's own row order.  This is what a sharded run gathers instead of the fp32 colour plane: a quarter of the
 * bytes (raymarching_engine_amd/dist.py); rm_assemble_striped_bytes puts the stripes in image order. */
RM_API int rm_present_rows(rm_ctx* ctx, rm_fb* fb, int samples, void* out_rgba8_device, void* hip_stream);
/* What a sharded job WITH depth of field gathers instead: the blur of display.frag:44-55 reads up to 16 rows either
 * side of a pixel, rows that other GPUs hold, so the present pass has to run where the whole frame is.  It reads two
 * things per pixel -- the accumulated colour (display.frag:19,53) and the accumulated DoF radius, normalAndDofRadius.w
 * (:21-23) -- and this call packs exactly those for the rows `fb` holds: out_float4_device = rm_fb_rows(fb)*width
 * float4 (colour.r, colour.g, colour.b, normal_dof.w) of DEVICE memory, in the window's own row order, asynchronous on
 * hip_stream (NULL = the context's stream).  Gathered and put in image order (rm_assemble_striped) the buffer is
 * passed to rm_present_device / rm_present_planes as BOTH `color` and `normal_dof` (they read .rgb of the one and .w of
 * the other): the bytes are those rm_present gives for the unsharded frame (raymarching_engine_amd/dist.py,
 * index.tsx:25-59 is the caller this serves). */
RM_API int rm_pack_present_rows(rm_ctx* ctx, rm_fb* fb, void* out_float4_device, void* hip_stream);
/* The present pass (display.frag:16-64) of ONE PART of a striped frame: `color` / `normal_dof` are DEVICE pointers to the WHOLE
 * frame in image order (height x width float4 each; with depth of field the gathered and assembled rows of
 * rm_pack_present_rows serve as both), out_rgba8_device receives the rows part `part` of `parts` holds (stripes of
 * stripe_rows rows dealt round-robin, packed as in rm_fb_create_striped: rows(part) x width x 4 bytes).  The taps,
 * their order and the arithmetic are rm_present_device's: assembled (rm_assemble_striped_bytes) the parts' bytes are
 * rm_present's.  This is how a sharded frame WITH depth of field is shown without one GPU blurring all of it: every
 * GPU gets the packed frame (an all-gather), blurs the stripes it holds -- 1 / parts of the pass -- and only RGBA8
 * travels to the GPU that shows the frame.  Asynchronous on hip_stream (NULL = the context's stream). */
RM_API int rm_present_striped_rows(rm_ctx* ctx, const void* color, const void* normal_dof, int width, int height, int samples, int stripe_rows, int parts, int part,
                            void* out_rgba8_device, void* hip_stream);

/* ---- denoise (opt-in): the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010, guided by the G-buffer ----
 * The filter display.frag:27-42 sketches, on the three planes after `samples` (= k) samples; INTEGRATION.md "Denoising"
 * states it in full.  With s = 1.0f / k, per pixel p: modulation m_p = max(albedo.xyz s, 1e-3) per channel, demodulated
 * colour x_p = colour.rgb s / m_p, normal n_p = normalize(normal.xyz s) (the zero vector when the length is < 1e-6 or
 * not finite: sky), depth z_p = albedo_depth.w s.  Pass i = 0 .. iterations-1 (step h = 2^i) averages the taps
 * q = p + h (dx, dy), dx, dy in -2..2 (a tap outside the image is skipped, no wrap), with weights
 *   b[dx] b[dy] exp(-|x_p - x_q|^2 / (sigma_color^2 4^-i)) exp(-|n_p - n_q|^2 / sigma_normal^2) w_z,  b = (1,4,6,4,1)/16,
 *   w_z = 1 at the centre or when both depths are non-finite, 0 when exactly one is, else
 *         exp(-|z_p - z_q| / (sigma_depth max(z_p, 1e-6) h sqrt(dx^2 + dy^2)));
 * a tap whose x_q is not finite weighs 0 and a pixel whose x_p is not finite keeps it.  Only x changes between passes.
 * The result is in colour-plane units: (x m_p k, colour.w); iterations = 0 is an exact copy of the colour plane.
 * The planes of an RM_GBUFFER_F16 framebuffer are widened exactly.  A NULL RmDenoise* means rm_denoise_default.
 * RM_ERR_INVALID before any device work for a windowed or striped framebuffer (the filter reads neighbouring rows), a
 * framebuffer of another context or without G-buffer planes, samples < 1, iterations outside 0..8, or a sigma that is
 * <= 0 or not finite.  The passes run in buffers the context owns (grown on demand, freed with it): one denoise at a
 * time per context. */
typedef struct RmDenoise {
  int iterations;       /* passes L, 0..8 (default 5) */
  float sigma_color;    /* of the demodulated colour, halved every pass (default 2.5) */
  float sigma_normal;   /* default 2.0 */
  float sigma_depth;    /* relative to the centre's depth (default 0.2) */
  int reserved;         /* 0 */
} RmDenoise;
RM_API void rm_denoise_default(RmDenoise* params);
/* out_host = rm_fb_rows(fb) x width x 4 floats of HOST memory, colour-plane units, row 0 = bottom; waits for the result. */
RM_API int rm_denoise(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoise* params, float* out_host);
/* The same left on the device: out_float4_device = rm_fb_rows(fb) x width float4 of DEVICE memory (16-byte aligned),
 * enqueued on hip_stream (NULL = the context's stream); no host wait. */
RM_API int rm_denoise_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoise* params, void* out_float4_device, void* hip_stream);
/* The denoised colour through exactly rm_present's pass (display.frag, the GL stack's arithmetic under rm_ctx_set_gl_stack,
 * the framebuffer's own normal + DoF plane): the bytes rm_present gives for a framebuffer whose colour plane holds
 * rm_denoise's result.  out_rgba8 = height x width x 4 bytes of HOST memory, row 0 = bottom. */
RM_API int rm_present_denoised(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoise* params, uint8_t* out_rgba8);

/* ---- variance-guided denoise (opt-in): rm_denoise's filter with the colour weight of SVGF (Schied et al. 2017) ----
 * The same passes, taps, spatial kernel b, normal weight and depth weight as rm_denoise, on a framebuffer with the
 * moments plane (RM_FB_MOMENTS); INTEGRATION.md "Denoising" states it in full.  With s, m_p, x_p, n_p, z_p as there and
 * lum(c) = 0.2126 c.r + 0.7152 c.g + 0.0722 c.b, each pixel carries the variance of its demodulated luminance
 *   v_p = max(0, M.y s - (M.x s)^2) s / max(lum(m_p), 1e-3)^2   (0 where that is not finite).
 * Before each pass g = the 3x3 Gaussian (1,2,1)^2/16 of v (taps outside the image skipped, renormalised); the colour
 * weight of the tap q is
 *   w_l = exp(-|lum(x_p) - lum(x_q)| / (sigma_luminance sqrt(g_p) + eps_p)),   eps_p = max(1e-3 |lum(x_p)|, 1e-6)
 * in place of rm_denoise's, and the pass filters the variance with the squared weights: v'_p = sum w^2 v_q / (sum w)^2.
 * A pixel whose variance is 0 keeps its colour up to taps within a few tenths of a percent of its luminance, so the
 * weights tighten as samples accumulate, while low-sample frames are smoothed (INTEGRATION.md gives the measured
 * error against converged frames, edges and depth of field included).  The defaults differ from rm_denoise's.  Non-finite colours and depths, sky, the image border,
 * the output units and iterations = 0 (an exact copy of the colour plane) are rm_denoise's.  RM_ERR_INVALID before any
 * device work for everything rm_denoise refuses, a framebuffer without the moments plane, and a sigma that is <= 0 or
 * not finite, or reserved != 0.  The passes use the same context buffers as rm_denoise (one denoise at a time per
 * context). */
typedef struct RmDenoiseVariance {
  int iterations;         /* passes L, 0..8 (default 3) */
  float sigma_luminance;  /* of the luminance distance, in units of the prefiltered standard deviation (default 4.0) */
  float sigma_normal;     /* default 1.0 */
  float sigma_depth;      /* relative to the centre's depth (default 0.2) */
  int reserved;           /* must be 0 */
} RmDenoiseVariance;
RM_API void rm_denoise_variance_default(RmDenoiseVariance* params);
/* rm_denoise, rm_denoise_device and rm_present_denoised with the variance-guided filter (NULL params = the defaults). */
RM_API int rm_denoise_variance(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoiseVariance* params, float* out_host);
RM_API int rm_denoise_variance_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoiseVariance* params, void* out_float4_device, void* hip_stream);
RM_API int rm_present_denoised_variance(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoiseVariance* params, uint8_t* out_rgba8);

/* ---- firefly filter (opt-in): an outlier clamp ahead of the denoisers and the present ----
 * The direct-light specular term of raymarcher.frag:368-371 reaches 1 / (pi roughness^2) times the light colour in single
 * pixels, and pow() leaves non-finite ones; both denoisers are edge-avoiding and keep such a pixel (above: "a pixel whose x_p
 * is not finite keeps it").  This stage dims a pixel whose luminance stands out of its neighbourhood to the neighbourhood's
 * rank statistic and, optionally, repairs a non-finite one; INTEGRATION.md "Firefly filter" states it in full, with what was
 * measured.  Input is the colour plane C after `samples` (= k) samples, s = 1.0f / k; all arithmetic is fp32, every product and
 * sum rounded on its own:
 *   l_p = (0.2126f * (C.r * s) + 0.7152f * (C.g * s)) + 0.0722f * (C.b * s);      a pixel is VALID iff l_p is finite.
 * The neighbourhood is the (2 radius + 1)^2 window without the centre, scanned dy = -radius..radius outer, dx inner; taps
 * outside the image (no wrap) and invalid taps are skipped.  n = the number of valid taps, t = the (rank + 1)-th largest l_q
 * among them (duplicates counted one by one), T = gain * t + floor (two roundings).
 *   n <= rank:                     the pixel is unchanged.
 *   valid centre, l_p <= T:        unchanged, bit for bit.
 *   valid centre, l_p > T:         out.rgb = C.rgb * f, f = t / l_p: the hue stays, the luminance becomes the rank statistic's.
 *   invalid centre, repair != 0:   out.rgb = the mean of the taps with l_q <= t: C_q.rgb summed in scan order, sequentially per
 *                                  channel, divided by (float)count; unchanged if any channel of the result is not finite.
 *   invalid centre, repair == 0:   unchanged.
 * out.w = C.w always; the output is in colour-plane units, like rm_denoise's.  A pixel with l_p <= floor is therefore never
 * changed (floor is in mean-colour, i.e. display, units), and rank = 1 tolerates one bright neighbour.  The filter reads the
 * colour plane alone: it is the same for both G-buffer formats and runs on framebuffers without G-buffer planes. */
typedef struct RmDespeckle {
  int radius;    /* 1 or 2 (default 2) */
  int rank;      /* 0..3 (default 1) */
  float gain;    /* finite, >= 1 (default 3.0) */
  float floor;   /* finite, >= 0 (default 0.1) */
  int repair;    /* 0 = leave non-finite pixels (default 1) */
  int reserved;  /* must be 0 */
} RmDespeckle;

/* The chain ahead of the present: despeckle -> denoise.  The denoise stage reads the despeckled colour where its statement
 * reads the colour plane (the .w of its result included); its guides and the moments plane are the framebuffer's own.  With the
 * despeckle stage off the chain is exactly rm_denoise* / rm_denoise_variance*; with both stages off it is an exact copy of the
 * colour plane.  rm_present_filtered runs rm_present's pass on the result (the GL stack's arithmetic under rm_ctx_set_gl_stack,
 * the framebuffer's own normal + DoF plane).  The despeckled plane lives in a buffer the context owns (grown on demand, freed
 * with it): one filter chain at a time per context.  RM_ERR_INVALID before any device work for a NULL argument, a framebuffer of
 * another context, a windowed or striped framebuffer (the filter reads neighbouring rows), samples < 1, `despeckle` outside
 * 0 / 1, an unknown denoise mode, a despeckle parameter outside the ranges above (checked only when that stage is on),
 * everything the selected denoiser refuses, and a misaligned or NULL device output.  Despeckle alone accepts a framebuffer
 * without G-buffer planes and a wrapped whole-frame one.  Outputs as rm_denoise / rm_denoise_device / rm_present_denoised. */
enum { RM_DENOISE_NONE = 0, RM_DENOISE_ATROUS = 1, RM_DENOISE_VARIANCE = 2 };
typedef struct RmFilters {          /* all POD */
  int despeckle;                    /* 0 off, 1 on */
  int denoise;                      /* RM_DENOISE_* */
  RmDespeckle despeckle_params;
  RmDenoise atrous;
  RmDenoiseVariance variance;
} RmFilters;
RM_API void rm_filters_default(RmFilters* filters);   /* both stages off, every parameter block at its own default */
RM_API int rm_filter(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, float* out_host);
RM_API int rm_filter_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, void* out_float4_device, void* hip_stream);
RM_API int rm_present_filtered(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, uint8_t* out_rgba8);

/* ---- frame statistics and exposure (opt-in) ----
 * rm_frame_stats reduces a frame to numbers on the device: the histogram of the luminance the firefly filter computes, in the same
 * order.  With s = 1.0f / samples, fp32, every product and sum rounded on its own:
 *   l = (0.2126f * (C.r * s) + 0.7152f * (C.g * s)) + 0.0722f * (C.b * s)
 * and every pixel falls in exactly one class:
 *   l NaN or +-inf                                            non_finite
 *   l < 2^-20 (negatives, +-0 and subnormals included)        below
 *   l >= 2^12                                                 above
 *   otherwise                                                 hist[(bits(l) >> 19) - 1712]
 * 16 bins per octave over 32 octaves: bin b covers [lo_b, hi_b), lo_b = the float with the bits (b + 1712) << 19, hi_b = lo_(b+1),
 * hi_511 = 2^12.  Integer arithmetic on the float's bits: no logarithm on the device, and nothing depends on the order of arrival.
 * min_l / max_l are the exact minimum and maximum over the finite l (-0 orders below +0); +inf / -inf when no pixel is finite.
 * filters == NULL: the statistics of the colour plane as it is, of ANY framebuffer of the context -- a window, a striped part, a
 * wrapped colour-only frame: pixels = rows held x width.  The counts are integers, so the RmFrameStats of a sharded frame's parts add
 * up exactly to the whole frame's.  filters != NULL: the statistics of the chain's result (rm_filter's), and everything rm_filter
 * refuses is refused.  RM_ERR_INVALID before any device work for a NULL handle or output, a framebuffer of another context and
 * samples < 1.  Synchronous; the counters live in a buffer the context owns. */
#define RM_STATS_BINS 512
typedef struct RmFrameStats {      /* 4136 bytes */
  uint64_t pixels, below, above, non_finite;   /* pixels = below + above + non_finite + sum(hist) */
  float min_l, max_l;
  uint64_t hist[RM_STATS_BINS];
} RmFrameStats;
RM_API int rm_frame_stats(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, RmFrameStats* out);

/* Host arithmetic on an RmFrameStats, all in double: no GPU, no context (like rm_debug_cull_cell).  N = sum(hist): only binned pixels
 * are ranked; C_b = the cumulative count through bin b (C_-1 = 0).
 *   rm_stats_percentile: *l = hi_b of the bin that holds the r-th smallest binned pixel, r = max(1, ceil(q N)); 0 when N == 0.
 *     RM_ERR_INVALID for a NULL argument and q outside [0, 1] or not finite.
 *   rm_stats_exposure: the gain that brings the log-average luminance of the pixels between two percentiles to `key`:
 *     a = low N, b = high N, w_b = max(0, min(C_b, b) - max(C_(b-1), a)), m = sum(w_b lambda_b) / (b - a) with
 *     lambda_b = (log2(lo_b) + log2(hi_b)) / 2, *gain = clamp(key / exp2(m), min_gain, max_gain) rounded to fp32; 1 when N == 0.
 *     params == NULL: the defaults.  RM_ERR_INVALID for a NULL stats or gain, unless 0 <= low < high <= 1, key > 0,
 *     0 < min_gain <= max_gain, every field finite and reserved == 0 all hold. */
typedef struct RmAutoExposure {
  float key;        /* the display value the log-average goes to (default 0.18) */
  float low, high;  /* the percentiles between which pixels count (default 0.10, 0.95) */
  float min_gain, max_gain;  /* default 2^-10, 2^10 */
  int reserved;     /* must be 0 */
} RmAutoExposure;
RM_API void rm_auto_exposure_default(RmAutoExposure* params);
RM_API int rm_stats_percentile(const RmFrameStats* stats, double q, float* l);
RM_API int rm_stats_exposure(const RmFrameStats* stats, const RmAutoExposure* params, float* gain);

/* ---- the display transform (opt-in): a fourth stage, behind the present pass's blur ----
 * Let v_c be what rm_present holds per channel in front of its pow (a / count * brightness: the blurred colour x 1 / samples), from
 * the chain's result as rm_present_filtered feeds it, in the arithmetic rm_present uses on that context (the GL stack's under
 * rm_ctx_set_gl_stack).  Every operation is fp32 and rounded on its own, with IEEE division, in this order:
 *   1. e_c = v_c * gain
 *   2. RM_TONE_CLIP: t_c = e_c
 *   3. otherwise a channel with !(e_c > 0) (zero, negative, NaN) passes through: t_c = e_c
 *   4. else E = min(e_c, 1048576.0f) and
 *        RM_TONE_REINHARD: q = E / w2; a = 1.0f + q; n = E * a; d = 1.0f + E; t = n / d    (w2 = white * white, once, in fp32)
 *        RM_TONE_ACES (Narkowicz's fit): a = 2.51f * E; a = a + 0.03f; n = E * a; b = 2.43f * E; b = b + 0.59f; b = E * b;
 *                                        d = b + 0.14f; t = n / d
 *   5. out_c = unorm8(pow(t_c, 1.0f / 2.2f)), alpha 255
 * rm_present_linear stops after step 1: (e.r, e.g, e.b, 1.0f), height x width x 4 floats, row 0 = bottom (tone and white are still
 * checked).  x * 1.0f is x: with the default RmDisplay rm_present_display gives rm_present_filtered's bytes, with the default
 * filters as well rm_present's.  filters == NULL: both stages off; display == NULL: the default.  RM_ERR_INVALID before any device
 * work, and before the handles are looked at, for a gain that is not finite or <= 0, an unknown tone, a white that is not finite or
 * <= 0 (checked for RM_TONE_REINHARD only) and reserved != 0; after those everything rm_present_filtered refuses; the device
 * output must be non-NULL and 4-byte aligned (height x width x 4 bytes, enqueued on hip_stream, NULL = the context's: no host
 * wait).  The striped, rows and sharded presents keep the reference's transform. */
enum { RM_TONE_CLIP = 0, RM_TONE_REINHARD = 1, RM_TONE_ACES = 2 };
typedef struct RmDisplay {
  float gain;    /* finite, > 0 (default 1) */
  int tone;      /* RM_TONE_* (default RM_TONE_CLIP) */
  float white;   /* RM_TONE_REINHARD: the value that maps to 1; finite, > 0 (default 4) */
  int reserved;  /* must be 0 */
} RmDisplay;
RM_API void rm_display_default(RmDisplay* display);
RM_API int rm_present_display(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, uint8_t* out_rgba8);
RM_API int rm_present_display_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, void* out_rgba8_device,
                                     void* hip_stream);
RM_API int rm_present_linear(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, float* out_float4_host);

/* The present of a frame that ONE process renders on several GPUs -- the shape of the reference's own host: one
 * thread, one render loop (index.tsx:120), here with a context per GPU, each holding one part of the frame's stripes
 * (rm_fb_create_striped with parts = `parts`, part = p on ctxs[p]; the host hands every sample to each context in turn
 * and the GPUs render concurrently, launches being asynchronous).
 *   rm_present_sharded_start: every context snapshots the rows it holds on its own stream -- tone-mapped (dof == 0,
 *     rm_present_rows) or packed (dof != 0, rm_pack_present_rows) -- and everything after that is enqueued on streams of
 *     the present's own, so the host can hand out the next samples at once (RenderJobExecutor.tsx:163-166 yields after a
 *     present; here the frame travels WHILE the next samples render).  dof == 0: the RGBA8 rows go to ctxs[0]'s GPU by
 *     peer copies over xGMI (hipMemcpyPeerAsync; no collective library, no second process) and are put in image order
 *     there.  dof != 0: the packed rows go to EVERY GPU, each puts the frame together, blurs and tone-maps the stripes
 *     it holds (rm_present_striped_rows: 1 / parts of the pass per GPU) and sends those bytes to ctxs[0]'s GPU.  The
 *     canvas is copied to pinned host memory.  Nothing is waited for.  One present at a time: finish before the next start.
 *   rm_present_sharded_finish: waits for THAT present only (an event; renders enqueued since keep running) and copies
 *     the canvas to out_rgba8 = height*width*4 bytes of HOST memory, row 0 = bottom: the bytes rm_present gives for the
 *     same samples on one framebuffer.  out_bytes = the size of that buffer: RM_ERR_INVALID, with the present still pending,
 *     when it is smaller than the canvas of the present that was STARTED (the library knows that size, the caller of a
 *     finish alone may not: round 4's signature trusted it).
 *   rm_present_sharded: both, one after the other (synchronous).
 * (Hosts with a process per GPU -- bench.py, job.RenderJobContext(group=...) -- move the same rows over RCCL instead:
 * raymarching_engine_amd/dist.py.) */
RM_API int rm_present_sharded_start(rm_ctx* const* ctxs, rm_fb* const* fbs, int parts, int samples, int dof);
RM_API int rm_present_sharded_finish(rm_ctx* const* ctxs, int parts, uint8_t* out_rgba8, size_t out_bytes);
RM_API int rm_present_sharded(rm_ctx* const* ctxs, rm_fb* const* fbs, int parts, int samples, int dof, uint8_t* out_rgba8, size_t out_bytes);

/* ---- mesh extraction (opt-in): the surface of a scene as triangles ----
 * The scenes are signed distance fields; these entries sample one on a regular grid and mesh the level set `iso` with surface nets,
 * on the device.  No render kernel, entry point or result above changes.
 *
 * The grid.  n = CELLS per axis, so an axis has n + 1 corners; corner i of axis a lies at  lo[a] + (float)i * h[a]  with
 * h[a] = (hi[a] - lo[a]) / (float)n[a], everything fp32: the difference, the IEEE division, the product and the sum each rounded on
 * their own, no contraction.  The kernels compute the same bits; rm_grid_axis is the host statement of them (out = n[axis] + 1 floats;
 * host arithmetic, no GPU and no context, like rm_stats_percentile).  A grid is valid iff every lo, hi and h is finite and h > 0,
 * 1 <= n[a] <= 1024, (n0 + 1)(n1 + 1)(n2 + 1) <= 2^28 and reserved == 0.  Values are stored x fastest:
 * v[(k * (ny + 1) + j) * (nx + 1) + i]. */
typedef struct RmGrid { float lo[3], hi[3]; int32_t n[3]; int32_t reserved; } RmGrid; /* 40 bytes */
RM_API int rm_grid_axis(const RmGrid* grid, int axis, float* out);

/* The scene's distance at every corner: out[corner] is bit for bit what rm_probe(RM_PROBE_SDF) returns at that corner's position with
 * the same flags on the same context -- the same kind selection (kind rows; the long tables' evaluation from 16 rows), the same scene
 * block and culling grid, RM_RENDER_FAST the fast build, otherwise the GL stack's arithmetic on a context with rm_ctx_set_gl_stack,
 * else the strict build.  flags: 0, RM_RENDER_FAST, RM_RENDER_NO_CULL, alone or together; anything else is RM_ERR_INVALID.
 * rm_sdf_grid: out_host = corners floats of HOST memory, synchronous.  rm_sdf_grid_device: out_device = corners floats of DEVICE
 * memory (4-byte aligned), enqueued on hip_stream (NULL = the context's stream), no allocation and no host wait.  On a stream of the
 * caller's the context's own stream is made to wait, on the device, behind the launch: whatever the context does later with the scene
 * or its culling grid (a rebuild, rm_scene_destroy) is ordered behind this reader as it is behind the context's own work. */
RM_API int rm_sdf_grid(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, float* out_host);
RM_API int rm_sdf_grid_device(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, void* out_device, void* hip_stream);

/* The mesher: surface nets (no case table).  With e = v - iso (one fp32 subtraction) a corner is INSIDE iff e < 0 -- NaN, +0 and -0
 * are outside -- and a cell is ACTIVE iff its 8 corners are not all alike.
 *   The vertex of an active cell (i, j, k): walk its 12 edges, axis a = x, then y, then z with (a, b, c) cyclic -- (x, y, z), (y, z, x),
 *   (z, x, y) -- and within an axis the four edges along a at offsets (ob, oc) = (0,0), (1,0), (0,1), (1,1) from the cell's low corner.
 *   For an edge from corner c0 to c1 = c0 + 1 along a whose ends differ in `inside`:  t = e0 / (e0 - e1);  if !(t >= 0 && t <= 1) t = 0.5f;
 *   the crossing point has c0's coordinates except along a:  p0 + t * (p1 - p0)  (three roundings).  The points are summed per
 *   component, sequentially, in that edge order, and the vertex is  sum / (float)m  (IEEE division), m = the number of such edges.
 *   Vertices come in ascending linear cell index (k * ny + j) * nx + i.
 *   Faces: cells in the same order, within a cell a = x, y, z: the edge from the cell's low corner along a emits a quad iff its ends
 *   differ in `inside` and the cell's index along b and along c is >= 1 (edges on the grid's boundary emit nothing).  The quad's
 *   vertices q0..q3 belong to the cells at (b, c) offsets (-1,-1), (0,-1), (0,0), (-1,0); a low corner that is inside emits the
 *   triangles (q0,q1,q2), (q0,q2,q3), otherwise (q0,q3,q2), (q0,q2,q1): counter-clockwise seen from outside, towards increasing
 *   distance.  Degenerate triangles are kept.  Indices are uint32.
 * The order is exactly this one on every run (a prefix scan over per-cell counts places the output; no arrival-order atomics).
 *
 * rm_mesh_extract: rm_sdf_grid's values, which never leave the device, then the mesher.  params == NULL: the defaults (iso 0,
 *   normals 1, normal_delta 1e-5f, colours 0, flags 0 -- flags as rm_sdf_grid takes them).
 * rm_mesh_from_values: the mesher on the caller's field (corners floats of HOST memory, x fastest).
 * Arrays of a mesh (rm_mesh_download: `bytes` must be the array's exact size, else RM_ERR_INVALID; rm_mesh_device_ptr: NULL for an
 * absent or empty array):
 *   RM_MESH_POSITIONS  V x 3 fp32       RM_MESH_TRIANGLES  T x 3 uint32       RM_MESH_CELLS  V uint32, each vertex's linear cell index
 *   RM_MESH_NORMALS    V x 3 fp32, RM_MESH_COLOURS  V x 3 fp32: only when asked for, only from rm_mesh_extract: what
 *     rm_probe(RM_PROBE_NORMAL, param = normal_delta) and the first three outputs of rm_probe(RM_PROBE_MATERIAL) give at the vertex
 *     positions with the same flags (the probe kernel itself, on the mesh's arrays).
 * rm_mesh_counts: out2 = {vertices, triangles}.  An empty mesh is valid: 0 / 0, and downloads of 0 bytes succeed.  A mesh owns its
 * arrays; the sampler's and the mesher's scratch is freed before the call returns; a failed allocation is RM_ERR_DEVICE with
 * nothing leaked.  Like a scene, a mesh belongs to its context and is destroyed before it.  Synchronous.
 * rm_mesh_timings: out_ms3 = {sampling, meshing, attributes} in milliseconds, from events on the context's stream round the kernels of
 * each stage of the call that made the mesh: the sampler; count + scan, and emit (the totals' way to the host and the allocation of the
 * arrays between the two are not in it); the normals and colours probes.  0 for a stage that did not run.
 * RM_ERR_INVALID before any device work -- and, as for rm_present_display, before the handles are looked at -- for an invalid grid,
 * an iso that is not finite, normals or colours outside 0 / 1, a normal_delta that is not finite or <= 0 when normals are on, flags
 * outside rm_sdf_grid's set and reserved != 0; then for NULL handles or outputs, a scene of another context, an unknown `what` and a
 * wrong `bytes`. */
typedef struct RmMeshParams { float iso; int32_t normals; float normal_delta; int32_t colours; int32_t flags; int32_t reserved; } RmMeshParams; /* 24 bytes */
RM_API void rm_mesh_params_default(RmMeshParams* params);
typedef struct rm_mesh rm_mesh;
RM_API int rm_mesh_extract(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, rm_mesh** out);
RM_API int rm_mesh_from_values(rm_ctx* ctx, const RmGrid* grid, const float* values_host, float iso, rm_mesh** out);
RM_API int rm_mesh_counts(const rm_mesh* mesh, unsigned long long* out2);
RM_API int rm_mesh_timings(const rm_mesh* mesh, float* out_ms3);
enum { RM_MESH_POSITIONS = 0, RM_MESH_NORMALS = 1, RM_MESH_COLOURS = 2, RM_MESH_TRIANGLES = 3, RM_MESH_CELLS = 4 };
RM_API int rm_mesh_download(rm_mesh* mesh, int what, void* host, size_t bytes);
RM_API void* rm_mesh_device_ptr(rm_mesh* mesh, int what);
RM_API void rm_mesh_destroy(rm_mesh* mesh);

/* ---- sharp vertices (opt-in): dual contouring over the surface-nets mesh ----
 * Surface nets puts a cell's vertex at the mean of its edge crossings, which bevels every edge and corner of a scene by about half a cell.
 * rm_mesh_extract_sharp keeps that mesh -- RM_MESH_TRIANGLES, RM_MESH_CELLS, the vertex count and order are bit for bit those of
 * rm_mesh_extract with the same grid and params -- and moves each vertex to the minimiser of a quadratic error function (QEF) of the
 * surface's tangent planes at the cell's edge crossings.  Normals and colours, when asked for, are the probes at the NEW positions, with
 * params.normal_delta as before.  The result is an ordinary rm_mesh.  params == NULL and sharp == NULL: the defaults (refine 6, normal_delta
 * 0x1p-10f, threshold 0.1f).  rm_mesh_extract and rm_mesh_from_values are unchanged (a field has no normals: no sharp variant of the latter).
 *
 * All arithmetic below is fp32, every operation rounded on its own, no contraction, division and square root IEEE, in the strict build
 * whatever params.flags say: the flags select only the unit whose probe kernel evaluates the scene, as in rm_mesh_extract.
 *   1. Sample, count, scan, emit: rm_mesh_extract's.
 *   2. Crossings.  A vertex has 12 slots, its cell's edges in the mesher's order (axis a = x, y, z; offsets (0,0), (1,0), (0,1), (1,1)).  A slot
 *      is LIVE iff its edge's ends differ in `inside` and then holds a bracket (x0, e0, x1, e1): the ends' coordinates along a and their
 *      v - iso.  `refine` times:  xm = x0 + 0.5f * (x1 - x0);  em = sdf(the edge's point with xm along a) - iso;  if (em < 0) == (e0 < 0) then
 *      (x0, e0) = (xm, em) else (x1, e1) = (xm, em)  (a NaN is outside, as in the mesher).  Then  t = e0 / (e0 - e1);  if !(t >= 0 && t <= 1)
 *      t = 0.5f;  the crossing lies at  x0 + t * (x1 - x0)  along a (difference, product, sum), its other coordinates are the edge's.  sdf is
 *      rm_probe's RM_PROBE_SDF launch with params.flags over all slots at once, one launch per round; a dead slot holds the cell's
 *      surface-nets vertex, so that the probes evaluate a defined point, and contributes nothing.  With refine == 0 the crossings are the
 *      mesher's own.
 *   3. Mass point.  c = the live crossings summed per component, sequentially in slot order, each sum divided by (float)m, m = their number.
 *   4. Normals.  One RM_PROBE_NORMAL launch with param = sharp.normal_delta and params.flags at the slots' points.  A live slot CONTRIBUTES
 *      iff its normal's three components are finite and not all zero.
 *   5. QEF.  With d = p - c per contributing slot (p its crossing, n its normal), sequentially in slot order:  A = sum n n^T  as six sums
 *      a00 += nx nx, a01 += nx ny, a02 += nx nz, a11 += ny ny, a12 += ny nz, a22 += nz nz  and  b += n * nd,  nd = (nx dx + ny dy) + nz dz.
 *      Eigenvectors by cyclic Jacobi: V = I, then 5 sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index; a pair with
 *      a_pq == 0 is skipped, otherwise
 *        theta = (a_qq - a_pp) / (2 a_pq);   t = copysign(1, theta) / (|theta| + sqrt(theta theta + 1));
 *        cr = 1 / sqrt(t t + 1);   sr = t cr;   h = t a_pq;
 *        a_pp = a_pp - h;   a_qq = a_qq + h;   a_pq = 0;
 *        (a_rp, a_rq) = (cr a_rp - sr a_rq,  sr a_rp + cr a_rq)      -- both from the old pair, each product rounded, then the sum
 *        (v_kp, v_kq) = (cr v_kp - sr v_kq,  sr v_kp + cr v_kq)      for the rows k = 0, 1, 2 of V
 *      lambda_i = a_ii, its vector column i of V.  lmax = lambda_0; if (lambda_1 > lmax) lmax = lambda_1; likewise lambda_2.  Pair i is KEPT
 *      iff lambda_i > 0 and lambda_i > threshold * lmax.  o = 0; for i = 0, 1, 2, if kept:  w = ((v_0i b_0 + v_1i b_1) + v_2i b_2) / lambda_i,
 *      o_k = o_k + v_ki w.  x = c + o.  If no slot contributes or a component of x is not finite, x = c.  Finally each component is clamped
 *      to its cell's own corner coordinates (if x < lo then lo; if x > hi then hi): a vertex never leaves its cell, so the connectivity stays valid.
 * The scratch is 12 slots of (bracket, point, probe output) per vertex and a mask word, freed before the call returns; a failed allocation
 * is RM_ERR_DEVICE with nothing leaked, and so is a mesh with 12 V > INT_MAX (the probe's count is an int).  The time of steps 2-5 is added
 * to the meshing slot of rm_mesh_timings.  RM_ERR_INVALID, in this order: everything rm_mesh_extract refuses before the handles are looked
 * at; at that same point refine outside 0..16, a normal_delta that is not finite or <= 0, a threshold that is not finite or outside [0, 1),
 * reserved != 0; then NULL handles or outputs and a scene of another context. */
typedef struct RmMeshSharp { int32_t refine; float normal_delta; float threshold; int32_t reserved; } RmMeshSharp; /* 16 bytes */
RM_API void rm_mesh_sharp_default(RmMeshSharp* sharp);
RM_API int rm_mesh_extract_sharp(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSharp* sharp, rm_mesh** out);

/* ---- components and islands (opt-in): what hangs together, and a mesh of the parts worth keeping ----
 * A level set of a fractal scene is one body in a cloud of detached specks, and a cell that is active only on the grid's boundary yields a vertex
 * that no triangle references.  These entries label a mesh's connected components and compact the kept ones into a new mesh, on the device.  They
 * work on any rm_mesh (rm_mesh_extract, _sharp, _from_values, an earlier rm_mesh_filter) and change nothing of it.  For V vertices and T triangles:
 *   Connected.  Two vertices are connected iff a chain of triangles links them: two vertices of one triangle are linked (degenerate triangles
 *     count: their indices are distinct).  A vertex in no triangle is a component of its own with 0 triangles.
 *   Component index.  The components are numbered 0 .. C-1 in ascending order of their smallest vertex index.
 *   RM_MESH_PART_LABELS  V uint32: labels[v] is the index of v's component.
 *   RM_MESH_PART_SIZES   C x 2 uint32: (vertices, triangles) of component c.  A triangle belongs to the component of its vertices.
 *   Keep rule (RmMeshKeep: rm_mesh_keep_default gives min_triangles 1, largest 0).  A component PASSES iff triangles >= min_triangles.  With
 *     largest == 0 every passing component is kept.  With largest = k > 0 only the first k passing components are kept, in the order (triangles
 *     descending, component index ascending).  The defaults therefore drop exactly the unreferenced vertices.
 *   Filtered mesh.  An ordinary rm_mesh of the same context: the kept vertices in their original relative order, the kept triangles in theirs,
 *     indices renumbered, and positions, cells (still the linear cell index in the source's grid), and normals and colours when the source has
 *     them, carried bit for bit.  An array the source was made without is absent from the result too.  A kept component is kept whole, so
 *     filtering a filtered mesh by the same rule gives the same arrays.  An empty source or an empty selection gives a valid empty mesh (0 / 0).
 * Every output is defined without reference to the order in which the device's threads arrive: it is the same on every run.
 * Procedure (rm_mesh_kernels.inc "components and islands": integer kernels, the same in every build):
 *   1. Labelling.  parent[v] = v, then rounds of HOOK (one thread per triangle: find the roots of an edge's ends, atomicMin the larger root's
 *      parent to the smaller) and FLATTEN (parent[v] = root(v)).  parent[x] <= x holds at every instant, so a root chase strictly descends and
 *      ends by itself: no thread waits for another.  The hook pass sets a word when it met two roots.  The host reads it behind each round and
 *      stops at the first round that left it 0, a whole pass that found every edge inside one tree.  At most 64 rounds: reaching that is a
 *      defect, RM_ERR_DEVICE "did not converge".
 *   2. The roots (parent[v] == v) are numbered by the mesher's scan, labels[v] = the number of parent[v], and the sizes are integer atomic adds.
 *   3. rm_mesh_filter: the C pairs come to the host, the keep rule is applied there, a mask per component goes back.  The vertex and the triangle
 *      keep flags are scanned, one kernel gathers the vertex arrays, one writes the renumbered triangles.
 * rm_mesh_components: labels the mesh once and keeps the result with it (4 V + 8 C bytes of device memory, freed by rm_mesh_destroy: a mesh's
 *   arrays never change, so it stays valid).  Later calls, rm_mesh_components_download and rm_mesh_filter reuse it.  *out_count = C.  Synchronous,
 *   on the stream of the mesh's context.  A filtered mesh starts without a labelling of its own.
 * rm_mesh_components_download: `bytes` must be exactly 4 V (labels) or 8 C (sizes).  It labels the mesh if nobody has.  host may be NULL only with
 *   0 bytes.
 * rm_mesh_filter: keep == NULL is the defaults.  rm_mesh_timings of the result is {0, the milliseconds of the labelling (if this call ran it) and of
 *   the compaction kernels between events on the stream, 0}.  rm_mesh_download and rm_mesh_device_ptr serve the result as they serve any mesh.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): before the handles are looked at, keep
 * min_triangles < 0, keep largest < 0, a non-zero keep reserved.  Then a NULL mesh, out or out_count ("NULL argument").  Then an unknown `what`.
 * Then a wrong `bytes` ("exact size").  RM_ERR_DEVICE: a mesh with T >= 2^32 (the sizes are uint32), a failed allocation (nothing leaked). */
typedef struct RmMeshKeep { int32_t min_triangles; int32_t largest; int32_t reserved[2]; } RmMeshKeep; /* 16 bytes */
RM_API void rm_mesh_keep_default(RmMeshKeep* keep);
RM_API int rm_mesh_components(rm_mesh* mesh, unsigned long long* out_count);
enum { RM_MESH_PART_LABELS = 0, RM_MESH_PART_SIZES = 1 };
RM_API int rm_mesh_components_download(rm_mesh* mesh, int what, void* host, size_t bytes);
RM_API int rm_mesh_filter(rm_mesh* mesh, const RmMeshKeep* keep, rm_mesh** out);

/* ---- simplification (opt-in): vertex clustering, a lighter mesh that averages the fine one ----
 * Every stage above keeps the triangle count its sampling grid dictates.  rm_mesh_simplify lays a second grid, `clusters`, over a mesh, merges
 * the vertices of each of its cells into one, and drops the triangles that collapse or repeat.  It works on any rm_mesh (rm_mesh_extract, _sharp,
 * _from_values, rm_mesh_filter, an earlier rm_mesh_simplify) and changes nothing of it; the result is an ordinary rm_mesh of the same context, which
 * every mesh entry serves.  `clusters` is valid by RmGrid's rule and need not be related to the grid the mesh was sampled on; n[a] cells of
 * h[a] = (hi[a] - lo[a]) / (float)n[a] per axis, as everywhere.  There is no care for manifoldness: a cluster's vertex
 * is the mean of its vertices (rm_mesh_simplify_quadric below places it by error quadrics), and thin sheets closer than a cluster cell merge.
 * Arithmetic: fp32 unless it says double, every operation rounded on its own (no contraction), IEEE division and square root, the same whatever
 * build made the source.  Q20(x) = (long long)rintf(x * 1048576.0f).  For V vertices and T triangles:
 *   1. Cluster of a vertex p.  Per axis a: u = (p[a] - lo[a]) / h[a]; i = 0 if !(u >= 0) (NaN too), i = n[a] - 1 if u >= (float)n[a], else
 *      i = min((int)floorf(u), n[a] - 1).  key = (k * ny + j) * nx + i.  The fraction f = u - (float)i, then 0 if !(f >= 0), 1 if f > 1 (a vertex
 *      outside `clusters` lands on its boundary cell's face), and q[a] = Q20(f) in 0 .. 2^20.
 *   2. Vertices.  One per occupied cluster, in ascending key; RM_MESH_CELLS of the result is that key, the linear cell index in `clusters`.  With m
 *      the cluster's vertex count and S[a] the integer sum of its q[a]: g = (float)((double)S[a] / ((double)m * 1048576.0)) (one double division),
 *      position[a] = lo[a] + ((float)i + g) * h[a] (a sum, a product, a sum).
 *   3. Normals and colours, when the source has them (an array the source lacks is absent from the result).  Per component x: a non-finite x
 *      counts as 0, x is clamped to [-1024, 1024], Q20(x) is summed per cluster as a signed 64-bit integer S, mean = (float)((double)S /
 *      ((double)m * 1048576.0)).  A colour is that mean.  A normal is the mean renormalised: len = sqrtf((x * x + y * y) + z * z), each component
 *      divided by len; (0, 0, 0) if len is 0 or not finite.
 *   4. Triangles.  Corners are mapped to the new indices.  A triangle with two equal corners is dropped.  Unless keep_duplicates, among the
 *      surviving triangles of one canonical form only the one with the smallest source index is kept; the canonical form rotates the smallest
 *      index to the front and preserves the cyclic order, so (a, b, c) and (a, c, b) are different triangles.  The kept triangles stand in their
 *      source order and are stored as mapped, not rotated.  A cluster whose triangles all vanished keeps its vertex: rm_mesh_filter with the
 *      defaults, applied to the result, removes exactly those (simplify first, then filter).
 *   5. An empty source gives a valid empty mesh.  The result starts without a labelling of its own.
 * Every output is a function of integer sums, minima and scans: it is the same on every run, whatever order the device's threads arrive in.
 * Procedure (rm_mesh_kernels.inc "simplification": in the strict unit, the same for every source).  No thread waits for another and every loop
 * is bounded.
 *   1. One thread per vertex marks its cluster's word in a dense array of 8 bytes per cluster cell; the mesher's scan numbers the occupied ones.
 *   2. One thread per vertex adds its q, its Q20 attributes and 1 to its cluster's row of 64-bit integers (atomic adds: they commute; a run of
 *      neighbouring lanes with one cluster is summed in the wave first and adds once); one thread per output vertex divides, renormalises
 *      and places.
 *   3. One thread per triangle maps it.  Unless keep_duplicates, every survivor enters an open-addressing table of triangle indices (a power of
 *      two >= 2 T slots, hashed over the canonical triple): atomicCAS on an empty slot; where the occupant's canonical triple equals its own,
 *      atomicMin; otherwise the next slot.  A slot's class never changes once claimed, so it ends holding the smallest index of its class, and a
 *      triangle is kept iff its slot holds its own index.  A probe that went round the whole table sets an error word: RM_ERR_DEVICE.
 *   4. The keep flags are scanned and the kept triangles gathered.
 * rm_mesh_simplify: params == NULL is the defaults.  Synchronous, on the stream of the mesh's context.  rm_mesh_timings of the result is {0, the
 *   milliseconds of these kernels between events on the stream, 0}.  The scratch (8 bytes per cluster cell, one row per output vertex, 4 V + 20 T
 *   bytes and the table) is freed before the call returns.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): before the handles are looked at, a NULL or
 * invalid `clusters` (RmGrid's texts), keep_duplicates outside 0 / 1, a non-zero reserved.  Then a NULL mesh or out ("NULL argument").
 * RM_ERR_DEVICE: a mesh with T >= 2^32, a failed allocation (nothing leaked). */
typedef struct RmMeshSimplify { int32_t keep_duplicates; int32_t reserved[3]; } RmMeshSimplify; /* 16 bytes */
RM_API void rm_mesh_simplify_default(RmMeshSimplify* params);
RM_API int rm_mesh_simplify(rm_mesh* mesh, const RmGrid* clusters, const RmMeshSimplify* params, rm_mesh** out);

/* ---- quadric placement (opt-in): a cluster's vertex where it best keeps the surface ----
 * rm_mesh_simplify puts a cluster's vertex at the mean of its vertices, which bevels every edge and corner inside a cluster by a fraction of a
 * CLUSTER cell -- what rm_mesh_extract_sharp had won back on the fine grid.  rm_mesh_simplify_quadric is to rm_mesh_simplify what
 * rm_mesh_extract_sharp is to rm_mesh_extract: the same mesh, with every vertex moved to the minimiser of the summed plane quadrics of the source
 * triangles that touch its cluster (Lindstrom, "Out-of-core simplification of large polygonal models", 2000).  Only the positions move.  The
 * source is unchanged; the result is an ordinary rm_mesh of the same context, which every mesh entry serves.  rm_mesh_simplify, its struct and
 * its refusals are as they were.  params == NULL and quadric == NULL: the defaults (keep_duplicates 0; threshold 0.1f).
 * Arithmetic: fp32 unless it says double, every operation rounded on its own (no contraction), IEEE division and square root, the same whatever
 * build made the source.  Let S be the result of rm_mesh_simplify(mesh, clusters, params): it gives, for every source vertex v, its output vertex
 * o(v) and its clamped quantised fractions q_v[a] (step 1 there), and for every output vertex its cell indices i[a] and mean fractions g[a] (step
 * 2 there).  Q24(x) = (long long)rintf(x * 16777216.0f).  For V vertices and T triangles of the source:
 *   0. Every array of the result except RM_MESH_POSITIONS is bit for bit the corresponding array of S: the vertex count and order, RM_MESH_CELLS,
 *      RM_MESH_TRIANGLES (both settings of keep_duplicates), and normals and colours when the source has them -- those stay the cluster means, a
 *      mesh has no scene to probe again.  The result starts without a labelling.
 *   1. Axis scale.  hmax = h[0]; if (h[1] > hmax) hmax = h[1]; if (h[2] > hmax) hmax = h[2];  s[a] = h[a] / hmax.
 *   2. Planes.  Every source triangle (i0, i1, i2) whose three indices are < V takes part, whether or not it survives in S (collapsed and
 *      duplicate triangles count too).  e1 = p1 - p0, e2 = p2 - p0;  c = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x), each
 *      product rounded, then the difference;  len = sqrtf((cx cx + cy cy) + cz cz).  If !(len > 0) or len is not finite the triangle contributes
 *      nothing.  n = c / len (three divisions);  m[a] = n[a] * s[a]: the plane's normal in cluster-cell coordinates, scaled so that |m| <= 1
 *      and residuals stay proportional to world distances.
 *   3. Sums.  For each corner k = 0, 1, 2 of a contributing triangle, with v = i_k and o = o(v):  f[a] = (float)q_v[a] / 1048576.0f (exact);
 *      d[a] = f[a] - g_o[a];  md = (m0 d0 + m1 d1) + m2 d2.  Cluster o gains  A00 += Q24(m0 m0), A01 += Q24(m0 m1), A02 += Q24(m0 m2),
 *      A11 += Q24(m1 m1), A12 += Q24(m1 m2), A22 += Q24(m2 m2),  B[a] += Q24(m[a] md)  and  planes += 1.  The sums are signed 64-bit integers:
 *      every term is below 2^26 and there are at most 3 * 2^32 of them, so nothing overflows.  A triangle with several corners in one cluster adds
 *      once per corner.
 *   4. Solve, per output vertex with planes > 0.  a_ij = (float)((double)A_ij / 16777216.0), b likewise.  Then exactly step 5 of "sharp vertices"
 *      from its Jacobi on: V = I, the 5 sweeps over the pairs (0,1), (0,2), (1,2); lmax; pair i is kept iff lambda_i > 0 and lambda_i > threshold *
 *      lmax; the truncated solve, which gives the offset w (o there).  x[a] = g[a] + w[a]; if a component of x is not finite, x = g.  Clamp:
 *      if (x[a] < 0) x[a] = 0; if (x[a] > 1) x[a] = 1 -- a vertex never leaves its cluster cell.  position[a] = lo[a] + ((float)i[a] + x[a]) *
 *      h[a] (simplify's own sum, product, sum).  With planes == 0 the position is S's, bit for bit.
 *   5. An empty source gives a valid empty mesh.  rm_mesh_timings of the result is {0, the milliseconds of all kernels of the call between
 *      events on the stream, 0}.
 * Every output is a function of integer sums: the same bytes on every run.  Triangles may fold where a minimiser is clamped, and manifoldness is
 * no more preserved than by rm_mesh_simplify.  Quadrics are not weighted by area; there are no boundary or feature constraints.
 * Procedure (rm_mesh_kernels.inc "quadric placement", in the strict unit).  rm_mesh_simplify's kernels run as they are.  Behind its place kernel,
 * one thread per source triangle computes the plane once and adds to a second scratch of ten 64-bit words per output vertex (integer atomic adds:
 * they commute); the corners of a triangle that share a cluster are merged in registers first, which leaves one to three slots, and for each slot
 * runs of neighbouring lanes with one cluster are summed in the wave and add once.  Then one thread per output vertex converts, solves, clamps
 * and overwrites the position.  No thread waits for another and no loop is unbounded.  The scratch is freed before the call returns.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): everything rm_mesh_simplify refuses before the
 * handles are looked at, in its order and with its texts (a NULL or invalid `clusters`, keep_duplicates outside 0 / 1, a non-zero simplify
 * reserved); a threshold that is not finite or outside [0, 1); a non-zero quadric reserved; then a NULL mesh or out ("NULL argument").
 * RM_ERR_DEVICE: as rm_mesh_simplify (T >= 2^32, a failed allocation with nothing leaked). */
typedef struct RmMeshQuadric { float threshold; int32_t reserved[3]; } RmMeshQuadric; /* 16 bytes */
RM_API void rm_mesh_quadric_default(RmMeshQuadric* q);
RM_API int rm_mesh_simplify_quadric(rm_mesh* mesh, const RmGrid* clusters, const RmMeshSimplify* params, const RmMeshQuadric* quadric, rm_mesh** out);

/* ---- ambient occlusion (opt-in): how open the scene is over every vertex, from the distance field ----
 * The mesh entries end with positions, normals and a flat diffuse colour; the cavities and creases that make a scene legible are a property of
 * the SCENE, which nothing downstream of the mesh can add.  rm_mesh_occlusion bakes them per vertex from the exact distance field (Evans,
 * "Fast approximations for global illumination on dynamic scenes", 2006; Quilez's distance-field occlusion): a fixed fan of K directions over
 * the surface, J taps along each, and at every tap the distance the scene has against the distance an open half-space would have.  No ray is
 * cast and the triangles are not read.  It works on any rm_mesh (rm_mesh_extract, _sharp, _from_values, rm_mesh_filter, rm_mesh_simplify,
 * _quadric) with any scene of the mesh's context, and changes nothing of the mesh: the occlusion is not one of its arrays (rm_mesh_download
 * serves `what` 0..4 as before), it goes to the caller's V floats.  1 means open.  The result is a function of (scene, positions, params)
 * only -- the mesh's stored normals are not used.
 * params == NULL: the defaults (radius 0.25f, directions 16, taps 4, normal_delta 0x1p-10f -- the sharp vertices' default, for the same
 * reason --, strength 1, flags 0).  A block is valid iff radius is finite and in [0x1p-64f, 0x1p64f], directions K is one of 1, 2, 4, 8, 16,
 * 32, 64, taps J is one of 1, 2, 4, 8, normal_delta is finite and > 0, strength is finite and in [0, 4], flags are of rm_sdf_grid's set and
 * reserved is 0.
 * Arithmetic: fp32 unless it says double, every operation rounded on its own (no contraction), IEEE division.
 *   1. Direction table, on the host in double (rm_mesh_occlusion_directions writes it: K x 4 floats, no GPU and no context, like rm_grid_axis).
 *      For k = 0 .. K-1:  u = (k + 0.5) / K;  phi = k * (pi * (3 - sqrt(5)));  z = sqrt(1 - u);  r = sqrt(u);  x = r cos(phi);  y = r sin(phi).
 *      Each of x, y, z is rounded to float; the fourth float is (float)(1.0 / (double)z_float).  Every direction has z > 0: a cosine-weighted
 *      fan over the hemisphere.  The device gets this table from the host and recomputes nothing of it.
 *   2. Per vertex with position p:  n = what rm_probe(RM_PROBE_NORMAL, param = normal_delta, flags) gives at p;  d0 = what
 *      rm_probe(RM_PROBE_SDF, flags) gives at p.
 *   3. Frame (Duff et al., "Building an orthonormal basis, revisited", 2017).  s = copysignf(1, n.z);  a = -1.0f / (s + n.z);
 *      b = (n.x * n.y) * a;  t = (1 + ((s * n.x) * n.x) * a,  s * b,  (-s) * n.x);  bt = (b,  s + (n.y * n.y) * a,  -n.y).
 *      Direction k, per component c:  w[c] = ((x * t[c]) + (y * bt[c])) + (z * n[c]).
 *   4. Taps j = 0 .. J-1.  t_j = radius * 2^-j;  inv_t_j = inv_radius * 2^j with inv_radius = 1.0f / radius (both scalings exact);
 *      q[c] = p[c] + w[c] * t_j;  d = the scene's distance at q, RM_PROBE_SDF's bits for these flags on this context;  e = z * t_j;
 *      ie = (1 / z) * inv_t_j (the table's fourth float);  o = ((d0 + e) - d) * ie;  if (!(o >= 0)) o = 0;  if (o > 1) o = 1 (NaN gives 0);
 *      quantum = (uint32)(o * 65536.0f + 0.5f), truncating.  Over a flat open surface d = d0 + e, and over a convex one d is larger: o = 0.
 *      d0 takes out, to first order, the fraction of a cell by which a surface-nets vertex sits off the surface.
 *   5. S = the integer sum of the K * J quanta (at most 2^25; no order).  occ = (float)S * 2^-(16 + log2 K + log2 J) (the scale is exact);
 *      ao = 1 - strength * occ;  if (!(ao <= 1)) ao = 1;  if (ao < 0) ao = 0.
 * The same bytes on every run.
 * Procedure (rm_mesh_kernels.inc "ambient occlusion", in all three units: it calls the scene's evaluator).  Two probe launches on the mesh's
 * positions make n and d0 in scratch, as the attribute pass does; then one lane per (vertex, direction) -- a vertex's K lanes are neighbours
 * in one wave -- sets its J points up, evaluates them, and the K integer sums are added across the lanes; the first of them stores.  No atomics.
 * The call is synchronous on the context's stream and frees its scratch before it returns.  out_ms2 (may be NULL) receives the milliseconds
 * between events on the stream of {the two probes, the taps}; an empty mesh succeeds, writes nothing to out_host and {0, 0} to out_ms2.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): an invalid block, one text per field, before
 * the handles are looked at; a NULL mesh, scene or out_host ("NULL argument"); a scene of another context than the mesh's.
 * RM_ERR_DEVICE: V * directions >= 2^31; a failed allocation, with nothing leaked. */
typedef struct RmMeshOcclusion {
  float radius;        /* the first tap's distance along its direction; tap j lies at radius * 2^-j */
  int32_t directions;  /* K */
  int32_t taps;        /* J */
  float normal_delta;  /* of the RM_PROBE_NORMAL that gives the frame */
  float strength;      /* ao = 1 - strength * occ, clamped to [0, 1] */
  int32_t flags;       /* 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both, as rm_sdf_grid */
  int32_t reserved[2];
} RmMeshOcclusion; /* 32 bytes */
RM_API void rm_mesh_occlusion_default(RmMeshOcclusion* params);
RM_API int rm_mesh_occlusion_directions(int directions, float* out);
RM_API int rm_mesh_occlusion(rm_mesh* mesh, rm_scene* scene, const RmMeshOcclusion* params, float* out_host, float* out_ms2);

/* ---- measures and edge topology (opt-in): is the mesh closed and oriented, how many edges are open, its area, volume and extent ----
 * What a caller who exports a mesh asks of it: rm_mesh_simplify has "no care for manifoldness", an extraction whose grid cuts the surface
 * leaves open borders, a fractal level set is one body plus specks.  rm_mesh_measure answers on the device, without a download.  It works
 * on any rm_mesh (rm_mesh_extract, _sharp, _from_values, rm_mesh_filter, rm_mesh_simplify, _quadric) and changes nothing of the mesh; the
 * result is kept with the mesh once made, as the labelling is (a mesh's arrays never change): a second call returns the stored bytes.
 * For V vertices and T triangles:
 *   Participating triangles.  A triangle PARTICIPATES iff its three indices are < V and pairwise distinct; skipped_triangles counts the
 *     others (no mesh of this library has one; the kernels read nothing but the three indices of such a triangle).  P = the participating ones.
 *   Edges.  A participating triangle (a, b, c) uses the directed edges a->b, b->c, c->a.  The undirected edge {x, y}, x < y, has f uses as
 *     x->y and r uses as y->x.  edges = E = the undirected edges with f + r >= 1.  An edge is BOUNDARY iff f + r = 1; REGULAR iff f = 1 and
 *     r = 1; otherwise IRREGULAR (three or more uses, or two in the same direction).  It is UNBALANCED iff f + r >= 2 and f != r: the places
 *     where the orientation disagrees, a subset of the irregular edges.  boundary + regular + irregular = E.
 *   Topology.  used_vertices counts the vertices named by at least one participating triangle.  euler = used_vertices - E + P.
 *     closed = 1 iff P >= 1, boundary_edges = 0 and irregular_edges = 0: every edge is then shared by exactly two triangles in opposite
 *     directions -- a closed, consistently oriented surface without non-manifold edges.  Non-manifold VERTICES (two fans that meet in a
 *     point) are not examined.
 *   Components.  components = C of rm_mesh_components; the call labels the mesh if nobody has, and the labelling stays with the mesh.  An
 *     edge belongs to the component of its ends.  rm_mesh_measure_components gives per component c, in rm_mesh_components' numbering, four
 *     uint64: (edges, boundary, irregular, unbalanced); `bytes` must be exactly 32 C, `host` may be NULL only with 0 bytes; it measures the
 *     mesh if nobody has.  closed_components counts the components that have at least one participating triangle and whose edges are all
 *     regular.
 *   Extent.  finite_vertices counts the vertices whose three coordinates are finite, referenced or not; lo[a] is the minimum and hi[a] the
 *     maximum of their coordinate a, and 0.0f is added to each of the six floats at the end, so a zero is stored as +0 whatever order the
 *     device compares in.  With no finite vertex lo = hi = 0.
 *   Area and volume, in double: every operation rounded on its own (no contraction), IEEE division and square root.  o[a] = (double)lo[a].
 *     A participating triangle is MEASURED iff its nine coordinates are finite; unmeasured_triangles counts the participating ones that are
 *     not.  For a measured triangle with p0, p1, p2 converted to double:  a = p0 - o, b = p1 - o, c = p2 - o;  e1 = b - a, e2 = c - a;
 *     n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x), each product rounded, then the difference;
 *     area_t = 0.5 * sqrt((nx nx + ny ny) + nz nz);  m = the same cross product of b and c;  vol_t = ((ax mx + ay my) + az mz) / 6.0.
 *     Every other triangle has area_t = vol_t = +0.0 at its place.  area and volume are the FIXED-TREE sums of the T terms in triangle
 *     order: pad the list with +0.0 to a multiple of 256; each group of 256 becomes one value by `for off = 128, 64, .., 1: s[i] = s[i] +
 *     s[i + off] for i < off`; the group values, in group order, are the next list; repeat until one value is left (an empty list sums to
 *     +0.0).  volume is signed, positive for the mesher's outward orientation, and means an enclosed volume only when `closed`.
 * Determinism: every output is a function of integer sums, minima and maxima, and of that fixed tree: the same bytes on every run.
 * Procedure (rm_mesh_kernels.inc "measures and edge topology", strict unit only: no scene arithmetic).  Topology: the labelling if the mesh
 * has none; then one thread per triangle inserts its three edges into an open-addressing table of 64-bit keys x << 32 | y (all-ones is the
 * empty word, and no key since x < y; a power of two of slots, the first >= 4 T) -- atomicCAS on an empty slot, the next slot on a foreign
 * key -- and makes one 64-bit atomicAdd on the slot's count word, 1 for a use x->y and 1 << 32 for y->x (both halves stay below 2^32 since
 * T < 2^32); it also sets its corners' flags.  A probe that went round the whole table sets an error word: RM_ERR_DEVICE.  One thread per slot
 * classifies its edge; totals and component rows are integer atomic adds, summed in the wave first where its edges lie in one component;
 * one thread per vertex counts the flags.  Geometry: one thread per vertex for the extent (integer atomicMin / atomicMax on an
 * order-preserving code of the floats, reduced in the wave first), then one thread per triangle computes its two terms and its workgroup
 * makes the first level of the tree in LDS; every further level is one launch.  No floating-point atomics, no thread waits for another, every
 * loop is bounded.  Scratch, freed before the call returns: 16 bytes per slot (at most 128 T), 4 V bytes of flags, 32 C bytes of rows,
 * 16 ceil(T / 256) bytes of group sums and 1/255 of that for the levels behind, 120 bytes of totals.
 * The call is synchronous on the context's stream.  out_ms2 (may be NULL) receives the milliseconds between events on the stream of
 * {topology, including the labelling if this call ran it; geometry}, and {0, 0} when the stored result is returned.  An empty mesh succeeds:
 * all zero, closed 0, 0 rows.
 * RM_ERR_INVALID (the text through rm_last_error(NULL) when no context is known): a NULL mesh or out ("NULL argument"); for
 * rm_mesh_measure_components a NULL mesh ("NULL argument"), then a wrong `bytes` ("exact size"), then a NULL host with bytes > 0.
 * RM_ERR_DEVICE: T >= 2^32; a failed allocation, with nothing leaked. */
typedef struct RmMeshMeasures {            /* 160 bytes */
  uint64_t vertices, triangles;            /*   0,   8: V, T as rm_mesh_counts */
  uint64_t used_vertices;                  /*  16 */
  uint64_t skipped_triangles;              /*  24 */
  uint64_t unmeasured_triangles;           /*  32 */
  uint64_t finite_vertices;                /*  40 */
  uint64_t edges, boundary_edges, regular_edges, irregular_edges, unbalanced_edges; /* 48, 56, 64, 72, 80 */
  int64_t  euler;                          /*  88 */
  uint64_t components, closed_components;  /*  96, 104 */
  double   area, volume;                   /* 112, 120 */
  float    lo[3], hi[3];                   /* 128, 140 */
  int32_t  closed;                         /* 152 */
  int32_t  reserved;                       /* 156: written as 0 */
} RmMeshMeasures;
RM_API int rm_mesh_measure(rm_mesh* mesh, RmMeshMeasures* out, float* out_ms2);
RM_API int rm_mesh_measure_components(rm_mesh* mesh, void* host, size_t bytes);

/* ---- slabbed extraction (opt-in): grids beyond 2^28 corners, meshed in windows of z layers ----
 * rm_mesh_extract, _sharp and _from_values hold the whole corner field at once and refuse more than 2^28 corners (about 645^3).  The three
 * entries below walk the grid in SLABS of cell layers, hold one window of values at a time, and give one ordinary rm_mesh: every later
 * stage (components, filter, simplify, quadric, occlusion, measure, the downloads) serves it unchanged, so a labelling runs across slabs.
 * Contract: wherever the unslabbed entry runs, all arrays of the result (RM_MESH_POSITIONS, _TRIANGLES, _CELLS, and _NORMALS / _COLOURS
 * when asked for) and rm_mesh_counts are byte for byte that entry's, for every scene, flag combination and admissible `layers`; `layers`
 * never changes a byte of a result.
 * Grid rule (these three entries only): RmGrid's rule without the bound on the corners -- 1 <= n[a] <= 1024 stays, so a grid has at most
 *   2^30 cells, and RM_MESH_CELLS (the linear cell index in the WHOLE grid) and the uint32 vertex indices still hold.  Totals are 64-bit.
 * Window.  slabs == NULL: the defaults (layers 0).  layers = L >= 1 is the number of cell layers per slab; above nz it is nz.  Slab s owns
 *   the layers s L .. min(nz, (s + 1) L) - 1.  The window of a slab that starts at layer k0 > 0 also covers the HALO layer k0 - 1: corner
 *   planes k0 - 1 .. k0 + L.  (L + 2) (nx + 1) (ny + 1) must not exceed 2^28, so every index inside a window is an int.  layers == 0: the
 *   largest L whose (L + 2) (nx + 1) (ny + 1) stays within 2^26 corners (profiles/mesh_slabs.txt), at least 1.
 * Procedure (rm_mesh_kernels.inc "slabbed extraction"), two passes over the slabs; a window's values are indexed from its first plane:
 *   1. Tally.  Per slab: its own planes k0 .. k0 + L are filled -- by the sampler of rm_sdf_grid with the plane's index in the whole grid
 *      (z = lo[2] + (float)k * h[2]: the dense sampler's bits), or for rm_mesh_from_values_slabs by a copy of those planes -- and one
 *      thread per own cell evaluates the mesher's (active, quads); the words are summed in the wave, in the workgroup, and by one 64-bit
 *      integer atomic add per workgroup into the slab's total.  Integer sums: the same on every run.  One read of the totals gives every
 *      slab's vertex and triangle base and the sizes of the three arrays, which are allocated once.
 *   2. Emit.  Per slab with at least one vertex (the others are skipped, their second sampling saved): the window is filled again, halo
 *      plane included (the planes two windows share are sampled again, not kept); count over the window's cells, the halo's first; the
 *      scan of rm_mesh_extract; emit, where halo cells emit nothing, a cell's vertex index is scanned[cell] - scanned[first own cell] +
 *      the slab's vertex base (its neighbours' likewise), RM_MESH_CELLS is the cell's index in the whole grid, and the boundary rule of
 *      the quads uses the indices in the whole grid.
 *   3. rm_mesh_extract_sharp_slabs: the kernels of "sharp vertices" run per slab behind its emit, on the slab's run of vertices, while the
 *      window's values are resident; "12 V > INT_MAX" applies per slab.
 *   4. Normals and colours: the probes of rm_mesh_extract, once, on the finished arrays.
 * rm_mesh_timings: {sampling or upload, both passes; tally, count, scan, emit and sharpening; attributes}, summed over the windows.
 * Memory: (L + 2)(nx + 1)(ny + 1) floats and (L + 1) nx ny 64-bit counts, allocated once per call, beside the mesh itself.
 * Refused (RM_ERR_INVALID), in this order and before the handles are looked at: the grid; params; sharp; then slabs -- layers < 0, reserved
 * != 0, "slab window ..." above 2^28 corners (rm_mesh_from_values_slabs: the grid, iso, slabs).  Then a NULL handle or out ("NULL
 * argument") and a scene of another context.  RM_ERR_DEVICE: a failed allocation, with nothing leaked; a slab whose second sampling does not
 * count what its first counted (the host compares the scan's total with the tally before the emit writes anything). */
typedef struct RmMeshSlabs {  /* 8 bytes */
  int32_t layers;             /* cell layers per slab; 0 = chosen by the library */
  int32_t reserved;           /* must be 0 */
} RmMeshSlabs;
RM_API void rm_mesh_slabs_default(RmMeshSlabs* slabs);
RM_API int rm_mesh_extract_slabs(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSlabs* slabs, rm_mesh** out);
RM_API int rm_mesh_extract_sharp_slabs(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSharp* sharp,
                                       const RmMeshSlabs* slabs, rm_mesh** out);
RM_API int rm_mesh_from_values_slabs(rm_ctx* ctx, const RmGrid* grid, const float* values_host, float iso, const RmMeshSlabs* slabs, rm_mesh** out);

/* ---- projection onto the surface (opt-in): Newton steps of a mesh's vertices onto a level set of a scene ----
 * Every stage that moves a vertex leaves it off the level set it came from: surface nets averages edge crossings, rm_mesh_simplify averages
 * vertices, rm_mesh_simplify_quadric minimises against the source triangles.  rm_mesh_project puts the vertices back with the exact distance
 * field, p <- p - n (d - iso), and reports on the device how far off they were and are.  It works on any rm_mesh (rm_mesh_extract, _sharp,
 * _from_values, rm_mesh_filter, rm_mesh_simplify, _quadric, the slabbed entries, an earlier projection) with any scene of the mesh's context.
 * The source is unchanged; the result is an ordinary rm_mesh of the same context that every later stage serves.  RM_MESH_TRIANGLES and
 * RM_MESH_CELLS are carried bit for bit, RM_MESH_COLOURS too when the source has them; RM_MESH_NORMALS exist iff the source has them and are
 * then rm_probe(RM_PROBE_NORMAL, param = normal_delta, flags) at the final positions.  The result starts without a labelling or measures;
 * rm_mesh_download serves `what` 0..4 as before.  Only the VERTICES come to lie on the level set: triangles still chord it, and a vertex inside
 * a corner goes to the nearest face, not to the corner -- the stage complements "sharp vertices" and "quadric placement", it replaces neither.
 * params == NULL: the defaults (iso 0, rounds 4, relax 1, tolerance 0, reach 0, normal_delta 0x1p-10f, flags 0).  A block is valid iff iso is
 * finite, rounds is in 1..16, relax is finite and in (0, 1], tolerance is finite and >= 0, reach is finite and >= 0, normal_delta is finite
 * and > 0, flags are of rm_sdf_grid's set and reserved is 0.
 * Arithmetic: fp32, every operation rounded on its own (no contraction), IEEE division, whatever the flags are: they select only the unit that
 * evaluates the scene.  Per vertex with source position p0, p = p0, and for round r = 0, 1, ..:
 *   1. d = RM_PROBE_SDF's bits at p for these flags on this context;  e = d - iso.  Round 0's e is e_before.
 *   2. If e is not finite or |e| <= tolerance the vertex does not move this round.  Otherwise n = RM_PROBE_NORMAL's bits at p (param =
 *      normal_delta); if a component of n is not finite or all three are zero the vertex is UNDIRECTED and does not move.
 *   3. s = e * relax;  q[c] = p[c] - n[c] * s (one product, one difference).  With reach > 0: lo = p0[c] - reach, hi = p0[c] + reach;
 *      if (q[c] < lo) q[c] = lo;  if (q[c] > hi) q[c] = hi; the vertex is CLAMPED if either test changed q.  If a component of q is not finite
 *      the vertex does not move; otherwise p = q.  The round's `moved` counts the vertices whose p changed in bits.
 *   4. The host reads `moved` behind each round and stops after the first round that moved nobody (every later round would repeat it, so the
 *      result does not depend on the stop) or after `rounds` rounds.  rounds_run is the number of rounds evaluated.
 *   5. e_after = RM_PROBE_SDF at the final p, minus iso.  Where the last round moved nobody these are that round's values.
 *   6. Report.  Counts are integer sums.  max and worst come from one 64-bit atomicMax per wave on the key bits(|e|) << 32 | (0xFFFFFFFF - v)
 *      over the finite e: the largest |e|, and among equals the smallest vertex.  mean = sum / count, rms = sqrt(sum2 / count) in double over
 *      the finite e, where sum and sum2 are the FIXED-TREE sums of "measures and edge topology" of the V terms (double)|e| and (double)e *
 *      (double)e in vertex order, +0.0 for a non-finite e.  With no finite e: worst, max, mean and rms are 0.
 *   7. Flipped triangles.  Only triangles whose three indices are < V are examined.  c0, c1 = the cross product of "quadric placement" step 2
 *      on the source and on the final positions;  dot = (c0x c1x + c0y c1y) + c0z c1z;  flipped iff dot < 0 (a NaN is not).
 * Every output is a function of scene bits, integer sums and maxima, and that fixed tree: the same bytes on every run.
 * Procedure (rm_mesh_kernels.inc "projection").  A round is two launches.  Evaluate, in all three units with launch_sdf_grid's kind selection:
 * one lane per vertex stages the scene and enters the math mode as the probe kernel does, evaluates d, and evaluates the normal only when its
 * wave has a lane with a finite e above the tolerance -- the evaluators branch wave-uniformly, so whole waves stop paying for normals as their
 * vertices settle.  (A unit that runs with fp32 denormals flushed decides this on integers and, where d, iso or e is subnormal, for the
 * normals; the step below decides for itself.)  Step, in the strict unit: the arithmetic of 1 - 3, a flags word per vertex, `moved` reduced in
 * the wave, and in round 0 and behind the last round the report's terms with the first level of the tree.  One launch per triangle counts the
 * flips.  No thread waits for another, no loop is unbounded, there are no floating-point atomics.  Scratch, freed before the call returns:
 * 24 V bytes of d, n, flags and residual, 16 ceil(V / 256) bytes of group sums and 1/255 of that behind, 240 bytes of totals.
 * The call is synchronous on the context's stream.  rm_mesh_timings of the result is {0, the rounds and the report between events on the
 * stream, the normals' probe}.  report (may be NULL) receives the struct below; residual_host (may be NULL) V floats, e_after.  An empty mesh
 * gives a valid empty mesh, an all-zero report (rounds_run 0) and nothing in residual_host.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): an invalid block, one text per field, before
 * the handles are looked at; a NULL mesh, scene or out ("NULL argument"); a scene of another context than the mesh's ("the scene belongs to
 * another context").  No refusal writes to out, report or residual_host.
 * RM_ERR_DEVICE: V > INT_MAX; a failed allocation, with nothing leaked. */
typedef struct RmMeshProject {   /* 32 bytes */
  float iso;           /* the level to project onto (a mesh does not remember its own) */
  int32_t rounds;      /* 1..16 */
  float relax;         /* step = relax * (d - iso); finite, in (0, 1] */
  float tolerance;     /* a vertex with |d - iso| <= tolerance does not move; finite, >= 0 */
  float reach;         /* per axis, how far a vertex may end from where it started; finite, >= 0; 0 = no limit */
  float normal_delta;  /* of the RM_PROBE_NORMAL that gives the direction; finite, > 0 */
  int32_t flags;       /* 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both, as rm_sdf_grid */
  int32_t reserved;    /* must be 0 */
} RmMeshProject;
typedef struct RmMeshProjection {  /* 144 bytes */
  uint64_t vertices, triangles;                       /*   0,   8 */
  uint64_t moved_vertices;                            /*  16: final position bits != source bits */
  uint64_t settled_before, settled_after;             /*  24,  32: e finite and |e| <= tolerance */
  uint64_t nonfinite_before, nonfinite_after;         /*  40,  48 */
  uint64_t clamped_vertices, undirected_vertices;     /*  56,  64: in at least one round the reach clamp changed q / the normal was unusable */
  uint64_t flipped_triangles;                         /*  72 */
  uint64_t worst_before, worst_after;                 /*  80,  88: vertex index of the max, smallest index among ties; 0 with no finite e */
  double mean_before, rms_before, mean_after, rms_after; /* 96..120: of |e| over the finite ones; 0 with none */
  float max_before, max_after;                        /* 128, 132 */
  int32_t rounds_run, reserved;                       /* 136, 140: reserved is written as 0 */
} RmMeshProjection;
RM_API void rm_mesh_project_default(RmMeshProject* params);
RM_API int rm_mesh_project(rm_mesh* mesh, rm_scene* scene, const RmMeshProject* params, rm_mesh** out, RmMeshProjection* report, float* residual_host);

/* ---- deviation (opt-in): how far a mesh's triangles lie off a level set of a scene ----
 * Every stage above says of its result that only the vertices come to lie on the surface and that triangles still chord it.  rm_mesh_deviation
 * says by how much: it evaluates the scene's distance field at S = n * n fixed points inside every triangle and returns, per triangle, the
 * largest |d - iso| it met, and an area-weighted report.  It works on any rm_mesh (rm_mesh_extract, _sharp, _from_values, rm_mesh_filter,
 * rm_mesh_simplify, _quadric, the slabbed entries, rm_mesh_project) with any scene of the mesh's context.  It changes nothing of the mesh and
 * is not one of its arrays: rm_mesh_download serves `what` 0..4 as before.  The measure is ONE-SIDED, mesh to surface, and taken at S samples:
 * a lower bound of the triangle's true maximum, in the field's own units (a distance ESTIMATE such as the Mandelbulb's is no metric distance),
 * and it says nothing of parts of the surface that no triangle lies near.
 * params == NULL: the defaults (iso 0, order 4, tolerance 0, flags 0).  A block is valid iff iso is finite, order is 1, 2, 4 or 8, tolerance is
 * finite and >= 0, flags are of rm_sdf_grid's set and reserved is 0.
 * Arithmetic: fp32 unless it says double, every operation rounded on its own (no contraction), IEEE division and square root, whatever the
 * flags are: they select only the unit that evaluates the scene.  For V vertices, T triangles, n = order, S = n * n:
 *   1. Sample table (rm_mesh_deviation_weights: host arithmetic in double; the device gets the table from the host).  The samples are the
 *      centroids of the n * n congruent sub-triangles.  For s = 0 .. S - 1:  r = floor(sqrt(s)), c = s - r * r (row r has 2 r + 1
 *      sub-triangles).  c even, m = c / 2:  A = 3 (r - m) + 1, B = 3 m + 1.  c odd, m = (c - 1) / 2:  A = 3 (r - m) - 1, B = 3 m + 2.
 *      w1 = A / (3 n), w2 = B / (3 n), w0 = (3 n - A - B) / (3 n): integers divided in double, each quotient rounded once to float.
 *      out[4 s .. 4 s + 3] = (w0, w1, w2, 0).  All weights are > 0; the S samples carry equal area, so a plain mean over them is the
 *      triangle's area mean.
 *   2. Points.  For triangle t with corners p0, p1, p2 and sample s:  q[c] = ((w0 * p0[c]) + (w1 * p1[c])) + (w2 * p2[c]).
 *   3. Field.  d = RM_PROBE_SDF's bits at q for these flags on this context;  e = d - iso.
 *   4. Per triangle.  A triangle is SKIPPED iff one of its indices is >= V (the kernels read nothing but its three indices): +0 in
 *      triangles_host, and it contributes nowhere.  Otherwise F = the number of samples whose e is finite; max_t = the maximum of |e| over
 *      those samples (on the bits: any order gives the same), +0 with F = 0; it goes to triangles_host[t].  s1, s2 = the sums of (double)e and
 *      (double)e * (double)e over the S samples, +0.0 for a non-finite e, summed by the butterfly `for m = 1, 2, 4, .. < S: x[i] = x[i] +
 *      x[i xor m]` (a balanced tree, neighbours first).  The triangle is EVALUATED iff F == S; then mean_t = s1 / S and ms_t = s2 / S.
 *      area_t in double: e1 = p1 - p0, e2 = p2 - p0 with the corners converted to double,  n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,
 *      e1x e2y - e1y e2x), each product rounded, then the difference;  area_t = 0.5 * sqrt((nx nx + ny ny) + nz nz)  (the area of "measures
 *      and edge topology" without its shift of the origin).  The triangle is OVER iff it is evaluated and max_t > tolerance.
 *   5. Report.  Counts are integer sums; nonfinite_samples runs over the triangles that are not skipped.  area, over_area, A1 = sum of
 *      area_t * mean_t and A2 = sum of area_t * ms_t are the FIXED-TREE sums of "measures and edge topology" over the T terms in triangle
 *      order, +0.0 for a triangle that is not evaluated (for over_area: not over).  mean_signed = A1 / area, rms = sqrt(A2 / area), both 0
 *      when area == 0.  max and worst_triangle come from one 64-bit atomicMax per wave on the key bits(max_t) << 32 | (0xFFFFFFFF - t) over
 *      the evaluated triangles: the largest max_t, and among equals the smallest triangle; both 0 with no evaluated triangle.
 * Every output is a function of scene bits, integer sums and maxima, and that fixed tree: the same bytes on every run.
 * Procedure (rm_mesh_kernels.inc "deviation").  Evaluate, in all three units with launch_sdf_grid's kind selection: one lane per (triangle,
 * sample) -- S divides 64, so a triangle's lanes are neighbours in one wave -- reads its triangle's indices and corners, makes q, parks it in
 * LDS ahead of a barrier (so that the point provably precedes the unit's math mode, as in "ambient occlusion"), stages the scene, evaluates
 * and stores d, 4 bytes per sample.  Lanes beyond T * S repeat the last sample and store nothing; lanes of a skipped triangle evaluate vertex
 * 0's position.  Reduce, in the strict unit (plain fp32 and double, whatever unit evaluated): one lane per sample makes e, the finite flag and
 * the two squares' terms, the butterflies run over the triangle's S lanes, and the triangle's first lane computes area_t, writes max_t and the
 * four double terms and takes part in the wave's counts and atomicMax.  The tree's first level is made in LDS per workgroup of 256 terms,
 * every further level is one launch (the kernels of "measures and edge topology").  No floating-point atomics, no thread waits for another,
 * every loop is bounded.  Scratch, freed before the call returns: 4 T S bytes of d, 36 T bytes of max_t and terms, 32 ceil(T / 256) bytes of
 * group sums and 1/255 of that behind, 16 S bytes of table, 20 KiB of totals (256 copies of the counts and the key, a workgroup's atomics
 * going to the copy of its number mod 256, so that T S / 64 waves do not queue on one address; the host adds the counts and takes the largest
 * key, which any order gives alike).
 * The call is synchronous on the context's stream.  report (may be NULL) receives the struct below; triangles_host (may be NULL) T floats,
 * max_t; out_ms2 (may be NULL) the milliseconds between events on the stream of {evaluate; reduce and report}.  A mesh with V = 0 or T = 0
 * succeeds: a report that is zero but for vertices, triangles, samples and, with V = 0, skipped_triangles = T; nothing is written to
 * triangles_host; out_ms2 = {0, 0}.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): an invalid block, one text per field, before
 * the handles are looked at; a NULL mesh or scene ("NULL argument"); a scene of another context than the mesh's ("the scene belongs to
 * another context").  rm_mesh_deviation_weights: an order that is not 1, 2, 4 or 8, then a NULL out.  No refusal writes to report,
 * triangles_host or out_ms2.
 * RM_ERR_DEVICE: T * S >= 2^31; a failed allocation, with nothing leaked. */
typedef struct RmMeshDeviation {     /* 32 bytes */
  float   iso;         /* the level the mesh stands for (a mesh does not remember its own); finite */
  int32_t order;       /* n: 1, 2, 4 or 8; S = n * n samples per triangle */
  float   tolerance;   /* a triangle is OVER iff its max |e| > tolerance; finite, >= 0 */
  int32_t flags;       /* 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both, as rm_sdf_grid */
  int32_t reserved[4]; /* must be 0 */
} RmMeshDeviation;
typedef struct RmMeshDeviationReport { /* 112 bytes */
  uint64_t vertices, triangles;        /*  0,  8 */
  uint64_t skipped_triangles;          /* 16: an index >= V */
  uint64_t unevaluated_triangles;      /* 24: not skipped, at least one sample's e not finite */
  uint64_t nonfinite_samples;          /* 32: over the triangles that are not skipped */
  uint64_t over_triangles;             /* 40 */
  uint64_t worst_triangle;             /* 48: of max, smallest index among ties; 0 with none */
  double   area, over_area;            /* 56, 64: of the evaluated / the over triangles */
  double   mean_signed, rms;           /* 72, 80: area-weighted over the evaluated triangles; 0 when area == 0 */
  float    max;                        /* 88 */
  int32_t  samples;                    /* 92: S */
  int32_t  reserved[4];                /* 96: written as 0 */
} RmMeshDeviationReport;
RM_API void rm_mesh_deviation_default(RmMeshDeviation* params);
RM_API int rm_mesh_deviation_weights(int order, float* out); /* S x 4 floats; host arithmetic, no GPU, no context */
RM_API int rm_mesh_deviation(rm_mesh* mesh, rm_scene* scene, const RmMeshDeviation* params, RmMeshDeviationReport* report, float* triangles_host,
                             float* out_ms2);

/* ---- refinement (opt-in): split the edges that chord a level set of a scene ----
 * rm_mesh_deviation measures how far triangles lie off the level set; the only lever against it used to be a finer grid everywhere.
 * rm_mesh_refine is adaptive: it splits only the edges whose MIDPOINT is off the surface, puts the new vertices on the surface (with
 * rm_mesh_project's arithmetic, when a project block is given) and repeats.  It works on any rm_mesh with any scene of the mesh's context.  The
 * source is unchanged and may be destroyed first; the result is an ordinary rm_mesh of the same context that every later stage serves.
 * The criterion looks at edge midpoints only: a triangle's interior can still lie further off than `tolerance`, so rm_mesh_deviation remains
 * the judge of the result.  d is in the field's own units, as for deviation (a distance ESTIMATE such as the Mandelbulb's is no metric distance).
 * params == NULL: the defaults (iso 0, tolerance 0, min_edge 0, rounds 1, max_triangles 0, flags 0).  A block is valid iff iso is finite,
 * tolerance and min_edge are finite and >= 0, rounds is in 1..8, flags are of rm_sdf_grid's set and reserved is 0.  project == NULL: the
 * midpoints stay where they are; otherwise a block that rm_mesh_project accepts (its own iso, flags and normal_delta apply to it).
 * Arithmetic: fp32, every operation rounded on its own (no contraction), whatever the flags are: they select only the unit that evaluates the
 * scene.  One round on a mesh of V vertices and T triangles:
 *   1. Edge table.  The triangles that TAKE PART are rm_mesh_measure's: all three indices < V and pairwise different.  Every other triangle is
 *      carried unchanged and takes no part.  Using slot u = 3 t + s is the edge of triangle t from corner s to corner (s + 1) % 3.  Every
 *      undirected edge (lo, hi) of a participating triangle is entered into a lock-free 64-bit table (the measures' key lo << 32 | hi and
 *      hash) with an atomicMin of u: the edge's OWNER is its lowest using slot.  The unique edges are numbered in ascending owner order (a flag
 *      per using slot, the mesher's scan); E is their count.
 *   2. Evaluation.  For edge e:  m[c] = 0.5f * (p_lo[c] + p_hi[c]);  d[e] = RM_PROBE_SDF's bits at m for these flags on this context.
 *   3. Marking.  err = d[e] - iso;  dx, dy, dz = p_hi - p_lo;  len2 = (dx * dx + dy * dy) + dz * dz.  The edge is MARKED iff err is finite,
 *      |err| > tolerance and len2 > min_edge * min_edge (one product).  The marked edges get the new vertex indices V + k, k counting the marked
 *      edges in edge order (scan).
 *   4. New vertices.  Position m; colour 0.5f * (c_lo[c] + c_hi[c]) where the mesh has colours; cell that of lo.  Normals are not interpolated
 *      (see "end of call").  The V old vertices keep their indices and their bits.
 *   5. Emit.  mask has bit s set iff edge s of the triangle is marked; m_s is that edge's new vertex.  The children keep the parent's
 *      orientation and stand, in this order, at the triangle's scanned offset (a triangle that takes no part: itself).  r is the rotation of the
 *      corners (v_i = corner (i + r) % 3, m_i likewise) that brings a single marked edge to e0, and two marked edges to e0 and e1:
 *        mask 0:  (v0, v1, v2)
 *        one:     (v0, m0, v2), (m0, v1, v2)
 *        two:     (m0, v1, m1), then if the index m0 < m1:  (v0, m0, v2), (m0, m1, v2)   else:  (v0, m0, m1), (v0, m1, v2)
 *        mask 7:  (v0, m0, m2), (m0, v1, m1), (m2, m1, v2), (m0, m1, m2)
 *      The diagonal of "two" is an integer rule: no float ties.  Every triangle at an edge sees the same mark, so no T-junction can arise, at
 *      irregular edges (used three times or more) too.
 *   6. Budget and projection.  V' = V + marked and T' = T + the sum of the masks' bit counts are known before anything is emitted.  If no edge
 *      is marked the call ends (stopped 1).  If T' > max_triangles -- max_triangles == 0: the kernels' own limit, 3 T' < 2^31 -- the round is not
 *      applied and the call ends (stopped 2).  Otherwise the round's mesh is made, and with project != NULL ALL its vertices go through
 *      rm_mesh_project's steps 1 - 7 (the same kernels); the next round marks on the projected positions.
 * Rounds: at most `rounds`; stopped 0 when they were all applied.  rounds_run counts the rounds that were evaluated (steps 1 - 3), applied or not.
 * End of call.  RM_MESH_NORMALS exist iff the source has them and are then rm_probe(RM_PROBE_NORMAL, param = project's normal_delta, or 0x1p-10f
 * with project == NULL, flags = project's, or params' with project == NULL) at every vertex of the result -- also when no round was applied.
 * RM_MESH_COLOURS and RM_MESH_CELLS exist iff the source has them.  The result starts without a labelling or measures.
 * Report: integers and maxima only, the same bytes on every run.  max_first / max_last: the largest finite |err| over the midpoints of the first
 * / the last round evaluated (+0 with none).  flipped_triangles: the sum of the projections' flipped_triangles.
 * Procedure (rm_mesh_kernels.inc "refinement").  Per round: insert (one thread per triangle), flags (one per using slot), scan, E to the host,
 * number (one per using slot: every slot learns its edge, the owner writes the ends), evaluate -- in all three units with launch_sdf_grid's
 * kind selection, one lane per edge; the midpoint is made and parked in LDS ahead of a barrier so that it provably precedes the unit's math
 * mode, as in "deviation"; lanes beyond E repeat the last edge and store nothing -- mark (plain fp32), children per triangle, two scans, one
 * read of (marked, T') by the host, then the new vertices (one thread per edge) and the children (one per triangle).  No thread waits for
 * another, every loop is bounded, there are no floating-point atomics.
 * The call is synchronous on the context's stream.  rm_mesh_timings of the result is {0, the split rounds, the projections and the normals}.
 * report (may be NULL) receives the struct below.  An empty mesh, or one without triangles, gives a copy and stopped 1 with rounds_run 0.
 * RM_ERR_INVALID, in this order (the text through rm_last_error(NULL) when no context is known): an invalid block, one text per field, then an
 * invalid project block (rm_mesh_project's texts), before the handles are looked at; a NULL mesh, scene or out ("NULL argument"); a scene of
 * another context than the mesh's.  No refusal writes to out or report.
 * RM_ERR_DEVICE: 3 T >= 2^31; V' > INT_MAX; an edge that found no slot; a failed allocation, with nothing leaked. */
typedef struct RmMeshRefine {    /* 32 bytes */
  float iso;              /* the level the mesh stands for (a mesh does not remember its own); finite */
  float tolerance;        /* an edge is split iff |d(midpoint) - iso| > tolerance; finite, >= 0 */
  float min_edge;         /* ... and its length > min_edge; finite, >= 0 */
  int32_t rounds;         /* 1..8 */
  uint64_t max_triangles; /* a round that would give more is not applied; 0 = the kernels' own limit */
  int32_t flags;          /* 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both, as rm_sdf_grid */
  int32_t reserved;       /* must be 0 */
} RmMeshRefine;
typedef struct RmMeshRefinement { /* 256 bytes */
  uint64_t vertices_before, triangles_before;  /*   0,   8 */
  uint64_t vertices, triangles;                /*  16,  24: of the result */
  uint64_t edges[8];                           /*  32: per round evaluated, the unique edges examined */
  uint64_t split_edges[8];                     /*  96: ... of them marked (also in a round the budget did not apply) */
  uint64_t nonfinite_midpoints[8];             /* 160: ... whose d - iso is not finite */
  uint64_t flipped_triangles;                  /* 224: the sum of the projections' */
  float max_first, max_last;                   /* 232, 236 */
  int32_t rounds_run;                          /* 240 */
  int32_t stopped;                             /* 244: 0 rounds done, 1 nothing to split, 2 budget */
  int32_t reserved[2];                         /* 248: written as 0 */
} RmMeshRefinement;
RM_API void rm_mesh_refine_default(RmMeshRefine* params);
RM_API int rm_mesh_refine(rm_mesh* mesh, rm_scene* scene, const RmMeshRefine* params, const RmMeshProject* project, rm_mesh** out,
                          RmMeshRefinement* report);

#ifdef __cplusplus
}
#endif
#endif /* HIP_RAYMARCH_H */
