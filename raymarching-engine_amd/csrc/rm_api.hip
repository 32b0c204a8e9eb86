// rm_api.hip -- the C ABI of libhip_raymarch.so (include/hip_raymarch.h).
//
// Host side only: contexts, scene upload/validation, framebuffers and the
// launches.  There is NO CPU path: without a GPU rm_ctx_create fails with
// RM_ERR_NO_DEVICE and nothing else can be called.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hip_raymarch.h"
#include "rm_params.hpp"

#ifndef RM_WITH_WAVEFRONT
#define RM_WITH_WAVEFRONT 0  // 1: the tests' cross-check build (rm_wavefront_host.inc)
#endif
#if RM_WITH_WAVEFRONT
#include "rm_wavefront_host.inc"
#endif

#define RM_SP_MAX 8

// rm_glstack.hip: the parity build in the GL stack's arithmetic.  Its scene passes are rm_params.hpp's launchers in namespace rm_gl (their
// parameter blocks are global types); what takes types of namespace rm, or no block at all, sits behind C entry points.
namespace rm_gl {
hipError_t launch_pixels_strict(const KParams& P, hipStream_t stream);
hipError_t launch_probe_strict(const ProbeParams& P, hipStream_t stream);
hipError_t launch_sdf_grid_strict(const SdfGridParams& P, hipStream_t stream);
hipError_t launch_mesh_occlusion_strict(const MeshOcclusionPass& P, hipStream_t stream);
hipError_t launch_mesh_project_eval_strict(const MeshProjectEval& P, hipStream_t stream);
hipError_t launch_mesh_deviation_eval_strict(const MeshDeviationSdf& P, hipStream_t stream);
hipError_t launch_mesh_refine_eval_strict(const MeshRefineMidpoints& P, hipStream_t stream);
}  // namespace rm_gl
// A scene pass `name` in the unit the flags and the context select: the fast build, the GL stack's arithmetic, or the parity build.
#define RM_SCENE_PASS(ctx, flags, name, P, stream)              \
  (((flags) & RM_RENDER_FAST) ? rm::name##_fast(P, stream)      \
   : (ctx)->gl_stack          ? rm_gl::name##_strict(P, stream) \
                              : rm::name##_strict(P, stream))
extern "C" {
hipError_t rm_gl_launch_math_probe(int fn, const float* a, const float* b, int n, float* out, hipStream_t stream);
hipError_t rm_gl_launch_camera_rng(const RmUniforms* u, int W, int H, int what, int count, float* out, hipStream_t stream);
hipError_t rm_gl_launch_present(const float4* color, const void* normal_dof, bool nd_half, int W, int H, float brightness, uchar4* out, hipStream_t stream);
hipError_t rm_gl_launch_present_striped(const float4* color, const float4* normal_dof, int W, int H, float brightness, uchar4* out, int stripe_rows, int parts,
                                        int part, int local_rows, hipStream_t stream);
hipError_t rm_gl_launch_present_display(const float4* color, const void* normal_dof, bool nd_half, int W, int H, float brightness, const DisplayPass* D, bool linear,
                                        void* out, hipStream_t stream);
hipError_t rm_gl_launch_present_rows(const float4* color, long long pixels, float brightness, uchar4* out, hipStream_t stream);
hipError_t rm_gl_set_native_tan(int on, hipStream_t stream);
}

// Samples in flight (pixel-kernel path, full mode): sample n renders on side stream n % depth into a staging
// buffer and is blended into the planes, in order, by a small kernel on the context's stream; the next samples
// render meanwhile.  One sample alone leaves the chip partly idle: a ray is a serial chain of ~2e5 instructions
// (~1 ms), so every launch ends in a tail and a small shard never fills the SIMDs.
struct SamplesInFlight {
  int depth = 3;  // RM_SAMPLES_IN_FLIGHT, rm_ctx_set_samples_in_flight
  hipStream_t stream[RM_SP_MAX] = {};
  hipEvent_t done[RM_SP_MAX] = {}, free[RM_SP_MAX] = {};  // slot's render finished; the blend that read its staging finished
  float4* stage[RM_SP_MAX] = {};
  size_t elems = 0;  // float4 elements of every slot's staging buffer (3 planes x tile pixels x samples of a batch)
  unsigned int next = 0;
  bool ready = false;

  hipError_t ensure_slots(int n) {
    hipError_t e;
    // side streams are made as the depth asks for them, not all RM_SP_MAX at once: the HIP runtime deals a process's streams
    // over a few hardware queues, and streams that share a queue serialise (measured: 0.59 instead of 0.42 ms per sample on a 1/8 shard)
    for (int s = 0; s < n; s++) {
      if (stream[s]) continue;
      if ((e = hipStreamCreateWithFlags(&stream[s], hipStreamNonBlocking)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&done[s], hipEventDisableTiming)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&free[s], hipEventDisableTiming)) != hipSuccess) return e;
    }
    ready = true;
    return hipSuccess;
  }
  // frees the staging buffers (the caller has synchronised the device, or is giving the buffers up)
  void release_staging() {
    for (float4*& p : stage) { if (p) (void)hipFree(p); p = nullptr; }
    elems = 0;
  }
  // staging of `need` float4 in each of the first n slots (a larger launch than any before waits for the device and makes them
  // all anew), and the slot the next launch takes
  hipError_t reserve(size_t need, int n, int* slot) {
    hipError_t e;
    if (elems < need) {
      if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
      release_staging();
      for (int s = 0; s < n; s++)
        if ((e = hipMalloc(reinterpret_cast<void**>(&stage[s]), sizeof(float4) * need)) != hipSuccess) { release_staging(); return e; }
      elems = need;
    }
    *slot = (int)(next++ % (unsigned int)n);
    if (stage[*slot]) return hipSuccess;
    return hipMalloc(reinterpret_cast<void**>(&stage[*slot]), sizeof(float4) * elems);  // the depth was raised after the buffers were made
  }
  size_t held_bytes() const {
    size_t held = 0;
    for (const float4* p : stage) held += p ? sizeof(float4) * elems : 0;
    return held;
  }
  hipError_t sync_all() {
    for (int s = 0; s < RM_SP_MAX; s++)
      if (stream[s]) { const hipError_t e = hipStreamSynchronize(stream[s]); if (e != hipSuccess) return e; }
    return hipSuccess;
  }
  void destroy() {
    for (int s = 0; s < RM_SP_MAX; s++) {
      if (stream[s]) { (void)hipStreamSynchronize(stream[s]); (void)hipStreamDestroy(stream[s]); }
      if (done[s]) (void)hipEventDestroy(done[s]);
      if (free[s]) (void)hipEventDestroy(free[s]);
      if (stage[s]) (void)hipFree(stage[s]);
    }
  }
};

// Cost-ordered dispatch of the pixel kernel when samples run one at a time: the tiles of a job in the order of their
// cost in the previous sample of the same job (same framebuffer window, tile and scene kind), most expensive first.
// One set per stream the kernel runs on (the side streams of the samples in flight, and the context's stream): a
// launch orders by the costs the previous launch ON ITS STREAM left, so no ordering between streams is needed.
struct Lpt {
  // Off the critical path (the context's own slot) there are two cost / order buffers, used in turn.  The costs of launch n
  // are sorted on a side stream WHILE launch n + 1 runs, and launch n + 2 starts in that order -- tile costs hardly
  // change from one sample to the next, so an order that is one sample old is as good, and the sort's two small launches
  // (one workgroup) no longer stand between two launches.  A sample-in-flight slot uses [0] alone.
  unsigned int* cost[2] = {nullptr, nullptr};
  unsigned int* order[2] = {nullptr, nullptr};
  hipEvent_t rendered[2] = {nullptr, nullptr}, sorted[2] = {nullptr, nullptr};
  int capacity = 0;   // tiles the buffers hold
  long long key[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the job the costs belong to
  bool have_cost = false;
  unsigned long long launches = 0;  // of this job (the context's own slot)
  int to_sort = 0;  // a sample-in-flight slot: tiles whose costs the last render left to sort_slot_costs (0: it recorded none)

  void forget() { have_cost = false; }  // the next launch starts a new job
  // room for `tiles`, in `sets` sets of buffers; what still uses the old ones runs on `stream` or `sort_stream`
  hipError_t grow(long long tiles, int sets, hipStream_t stream, hipStream_t sort_stream) {
    if (capacity >= tiles) return hipSuccess;
    hipError_t e;
    if (cost[0]) {
      (void)hipStreamSynchronize(stream);
      if (sort_stream) (void)hipStreamSynchronize(sort_stream);
    }
    free_buffers();
    const size_t order_elems = (size_t)tiles + rm::rm_order_scratch_elems(tiles);  // the sort's per-workgroup histograms behind the order
    for (int k = 0; k < sets; k++) {
      if ((e = hipMalloc(reinterpret_cast<void**>(&cost[k]), sizeof(unsigned int) * (size_t)tiles)) != hipSuccess) return e;
      if ((e = hipMalloc(reinterpret_cast<void**>(&order[k]), sizeof(unsigned int) * order_elems)) != hipSuccess) return e;
    }
    capacity = (int)tiles;
    forget();
    return hipSuccess;
  }
  void free_buffers() {
    for (int k = 0; k < 2; k++) {
      if (cost[k]) (void)hipFree(cost[k]);
      if (order[k]) (void)hipFree(order[k]);
      cost[k] = order[k] = nullptr;
    }
    capacity = 0;
  }
  void destroy() {
    free_buffers();
    for (int k = 0; k < 2; k++) {
      if (rendered[k]) (void)hipEventDestroy(rendered[k]);
      if (sorted[k]) (void)hipEventDestroy(sorted[k]);
    }
  }
};

// Device scratch of the present and the frame filters that lives with the context (a live loop presents, and filters, every
// sample): grown on demand by scratch_reserve, which states the rule, and freed with the context.
enum {
  SCRATCH_PRESENT,        // rm_present / rm_present_planes: the RGBA8 image before it goes to the host
  SCRATCH_DENOISE_X0,     // the denoisers' two ping-pong buffers of x
  SCRATCH_DENOISE_X1,
  SCRATCH_DENOISE_GUIDE,  // and their guide
  SCRATCH_DESPECKLE,      // the despeckled colour plane the denoise stage reads
  SCRATCH_STATS,          // rm_frame_stats: the counters (RM_STATS_BYTES), zeroed on the stream each call
  SCRATCH_STATS_HOST,     // and their page-locked host copy
  SCRATCH_COUNT
};
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
  bool pinned_host = false;  // page-locked host memory instead of device memory
  void release() {
    if (p) (void)(pinned_host ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes = 0;
  }
};

// Device memory that one call, or one mesh, owns: freed with its owner.  Waiting for the stream before memory that a kernel may still
// read goes is the owner's business (rm_mesh_destroy; the waits of the probe and mesh entries).
struct DeviceArray {
  void* p = nullptr;
  DeviceArray() = default;
  DeviceArray(DeviceArray&& o) noexcept : p(o.p) { o.p = nullptr; }  // moves, never copies: one owner
  ~DeviceArray() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; }
  hipError_t reserve(size_t bytes) { release(); return bytes ? hipMalloc(&p, bytes) : hipSuccess; }  // (0 bytes: NULL)
  float* f32() const { return static_cast<float*>(p); }
  unsigned int* u32() const { return static_cast<unsigned int*>(p); }
  unsigned long long* u64() const { return static_cast<unsigned long long*>(p); }
};

// Stage timing of the mesh entries (rm_mesh_timings): a span is a pair of events on the context's stream, made with the first mesh
// that runs the stage.
struct MeshSpans {
  enum { SAMPLE, COUNT_SCAN, EMIT, SHARPEN, ATTRIBUTES, LABEL, KEEP_FLAGS, GATHER, CLUSTER_NUMBER, CLUSTER_MERGE, CLUSTER_GATHER, OCCLUSION_PROBES, OCCLUSION_TAPS,
         MEASURE_TOPOLOGY, MEASURE_GEOMETRY, PROJECT_ROUNDS, PROJECT_NORMALS, DEVIATION_EVALUATE, DEVIATION_REDUCE, REFINE_SPLIT, REFINE_NORMALS, COUNT };
  hipEvent_t ev[COUNT][2] = {};
  hipError_t begin(int span, hipStream_t stream) { return record(ev[span][0], stream); }
  hipError_t end(int span, hipStream_t stream) { return record(ev[span][1], stream); }
  // milliseconds of a span that the stream has passed; 0 when the runtime cannot tell
  float ms(int span) const {
    float t = 0.0f;
    return hipEventElapsedTime(&t, ev[span][0], ev[span][1]) == hipSuccess ? t : 0.0f;
  }
  void destroy() {
    for (auto& pair : ev)
      for (hipEvent_t e : pair)
        if (e) (void)hipEventDestroy(e);
  }
  static hipError_t record(hipEvent_t& e, hipStream_t stream) {
    const hipError_t made = e ? hipSuccess : hipEventCreate(&e);
    return made != hipSuccess ? made : hipEventRecord(e, stream);
  }
};

// rm_present_sharded (one process driving several GPUs): this context's rows of the payload, and on the context that shows the
// frame -- the root -- the gathered parts and the frame in image order; grown on demand (scratch_reserve), freed with the context.
struct ShardPresent {
  enum {
    ROWS,    // this context's rows of the payload (packed float4 or RGBA8)
    ROWS8,   // depth of field: this context's rows after ITS blur (RGBA8)
    ALL,     // depth of field: every part's packed rows (the all-gather's receive side)
    RECV,    // root: every part's RGBA8 rows
    FRAME,   // depth of field: the packed frame in image order (every context)
    CANVAS,  // root: the RGBA8 canvas in image order
    HOST,    // root: pinned host copy of the canvas (rm_present_sharded_finish reads it)
    COUNT
  };
  Scratch buf[COUNT];
  hipStream_t stream = nullptr;                         // copies, assembly and blur of a present travel here, next to the renders
  hipEvent_t snap = nullptr, ev = nullptr, done = nullptr;  // snapshot written; this context's part delivered; root: canvas on the host
  bool pending = false;                                 // root: a start without its finish
  int w = 0, h = 0;                                     // root: the canvas of the pending present

  ShardPresent() { buf[HOST].pinned_host = true; }
  template <class T> T* as(int which) const { return static_cast<T*>(buf[which].p); }
  // the stream and the events, made with the first present (the caller has selected the device); `done` on the root alone
  hipError_t ensure(bool root) {
    hipError_t e = hipSuccess;
    if (!stream) e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    for (hipEvent_t* event : {&snap, &ev, root ? &done : nullptr})
      if (e == hipSuccess && event && !*event) e = hipEventCreateWithFlags(event, hipEventDisableTiming);
    return e;
  }
  // waits for the present stream before anything it may still write is freed; then the buffers, the stream, the events
  void destroy() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (Scratch& b : buf) b.release();
    if (stream) (void)hipStreamDestroy(stream);
    for (hipEvent_t event : {snap, ev, done})
      if (event) (void)hipEventDestroy(event);
  }
};

struct rm_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float retire_eps = 0.0f;  // opt-in (rm_ctx_set_retire_eps): any tolerance brightens lit pixels, see the header
  bool gl_stack = false;    // rm_ctx_set_gl_stack: strict-flag work runs in the GL stack's arithmetic (rm_glstack.hip)
#if RM_WITH_WAVEFRONT
  WavefrontHost wf;
#endif
  SamplesInFlight sp;
  int last_pipeline = 0;   // rm_ctx_last_pipeline: what the last render call dispatched
  // Sample batch of rm_render_samples (KParams::batch): 0 = as many samples per launch as bring it to about
  // RM_BATCH_TARGET_TILES workgroups (a whole 4K frame has 16 320), 1 = one launch per sample, 2..RM_BATCH_MAX = fixed.
  int sample_batch = 0;
  Lpt lpt[RM_SP_MAX + 1];  // one per stream the kernel runs on: the sample-in-flight slots, and [RM_SP_MAX] the context's own
  hipStream_t lpt_stream = nullptr;
  bool lpt_enabled = true;
  hipEvent_t switch_ev = nullptr;  // orders the old stream before the new one in rm_ctx_set_stream
  MeshSpans mesh_spans;             // the mesh entries' stages (rm_mesh_timings)
  hipEvent_t mesh_order = nullptr; // rm_sdf_grid_device on a caller's stream: the context's stream waits behind that launch (sdf_grid_enqueue)
  std::unordered_map<void*, size_t> buffers;  // rm_buffer_create: base address -> bytes
  Scratch scratch[SCRATCH_COUNT];  // scratch_reserve
  rm_ctx() { scratch[SCRATCH_STATS_HOST].pinned_host = true; }
  template <class T> T* scratch_as(int which) const { return static_cast<T*>(scratch[which].p); }
  ShardPresent shard;  // rm_present_sharded
  unsigned long long peer_enabled = 0;  // devices this context's GPU has been given peer access to
  // Culling grids of this context's scenes (scene_cull_grid): built once a scene has been asked for cull_min_pixels pixel-samples
  // (rm_ctx_set_cull_min_pixels), held within cull_budget bytes -- the least recently rendered scene gives its grid up first, and
  // renders on without one (same bits) -- and their buffers recycled: no hipMalloc / hipFree, which wait for the device, per scene.
  long long cull_min_pixels = 4ll << 20;
  size_t cull_budget = 0, cull_bytes = 0;
  unsigned long long cull_built = 0, use_clock = 0;
  std::vector<rm_scene*> cull_scenes;
  struct CullBuffer { unsigned long long* p; size_t bytes; bool idle; };  // idle: nothing enqueued anywhere still reads it
  std::vector<CullBuffer> cull_pool;
  // builds run on a stream of their own, NOT behind the context's: a new scene's grid is then built while the previous frame still
  // renders, and the new frame's render -- which waits for cull_event, on whichever stream it runs -- overlaps that frame's tail as
  // it would without a build (on the context's stream the build sat behind the previous frame's blend, i.e. behind its render)
  hipStream_t cull_stream = nullptr;
  hipEvent_t cull_event = nullptr, cull_order = nullptr;
  std::string error;
  std::string warning;  // rm_ctx_last_warning: advice that came with a call that SUCCEEDED (never an error)
};

struct rm_scene {
  rm_ctx* ctx = nullptr;
  DevScene dev{};
  RmPrim* d_prims = nullptr;
  RmSurface* d_surfaces = nullptr;
  unsigned long long* d_cull = nullptr;
  // the culling grid of a long CSG table is built once the scene has earned it (scene_cull_grid: rm_ctx_set_cull_min_pixels): a host that
  // creates many scenes it never renders, or shows a new one in every small frame, does not pay ((n^3 + (levels - 1) n_outer^3 + 1) x words
  // x 8 B -- 4.7 MB at 12 rows, 14 MB at 192 of hard operators; 31.5 MB per 64 rows of smooth unions, whose rule wants 128^3 cells near the
  // shapes -- and a build kernel per scene)
  bool cull_wanted = false;
  CullGrid cull_grid{};
  CullBuild cull_build{};
  size_t cull_bytes = 0;           // of d_cull
  long long px_seen = 0;           // pixel-samples asked of this scene while it had no grid
  unsigned long long last_use = 0; // rm_ctx::use_clock at the last render / probe
};

struct FbGeometry {
  int width = 0, height = 0, row_begin = 0, row_count = 0;  // row_count = rows held by the planes
  int stripe_rows = 0, parts = 1, part = 0;                 // striped window when stripe_rows > 0
};
struct rm_fb : FbGeometry {
  rm_ctx* ctx = nullptr;
  float4* plane[3] = {nullptr, nullptr, nullptr};  // planes 1 and 2 hold rm_half4 when gbuffer == RM_GBUFFER_F16
  bool owned = false;
  int gbuffer = RM_GBUFFER_F32;
  float2* moments = nullptr;  // RM_FB_MOMENTS (owned framebuffers only): plane 3, (sum l, sum l^2) per pixel
};

// bytes per pixel of a plane, and of the whole plane
static size_t plane_px_bytes(int gbuffer, int plane) {
  return plane == RM_PLANE_MOMENTS ? sizeof(float2) : (plane > 0 && gbuffer == RM_GBUFFER_F16) ? sizeof(rm_half4) : sizeof(float4);
}
static size_t plane_bytes(const rm_fb* fb, int plane) { return plane_px_bytes(fb->gbuffer, plane) * (size_t)fb->width * (size_t)fb->row_count; }
// device address of plane 0..3 (3: the moments plane, NULL without one)
static void* plane_ptr(const rm_fb* fb, int plane) { return plane == RM_PLANE_MOMENTS ? static_cast<void*>(fb->moments) : static_cast<void*>(fb->plane[plane]); }

static thread_local std::string g_create_error;

static int fail(rm_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->error = msg;
  else g_create_error = msg;
  return code;
}

#define RM_HIP(ctx, expr)                                                                              \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(ctx, RM_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// An entry's refusals, with its name in front of the text: RM_ERR_INVALID unless the code says otherwise.
struct Refuse {
  rm_ctx* ctx;
  const char* who;
  int operator()(const char* what, int code = RM_ERR_INVALID) const { return fail(ctx, code, std::string(who) + ": " + what); }
};
// ... and RM_HIP for the entries that put their name, not the expression, in front of the runtime's text
#define RM_HIP_AS(refuse, expr)                                                   \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) return refuse(hipGetErrorString(e_), RM_ERR_DEVICE);    \
  } while (0)

// The pair (context, scene) of an entry that takes both; `others`: whether the entry's further pointers, part of the same test, are there.
static int scene_check(const Refuse& refuse, const rm_scene* scene, bool others) {
  if (!refuse.ctx || !scene || !others) return refuse("NULL argument");
  if (scene->ctx != refuse.ctx) return refuse("the scene belongs to another context");
  return RM_OK;
}

// A host vector of the call's own that a mesh entry (rm_mesh_host.inc) reads its work back into, so that a refusal writes nothing of the
// caller's: sized before anything is enqueued; false when the host has no memory for it.
template <class T>
static bool host_staging(std::vector<T>& v, size_t n) {
  try {
    v.resize(n);
  } catch (const std::bad_alloc&) {
    return false;
  }
  return true;
}

extern "C" {

int rm_abi_version(void) { return RM_ABI_VERSION; }

void rm_material_default(RmMaterial* m) {  // Validate.tsx:18-51
  std::memset(m, 0, sizeof *m);
  m->diffuse[0] = m->diffuse[1] = m->diffuse[2] = 0.6f;
  m->diffuse_cutoff = 35.0f;
  m->specular[0] = m->specular[1] = m->specular[2] = 0.6f;
  m->specular_cutoff = 35.0f;
  m->roughness = 0.2f;
  m->subsurface = 11111115.0f;
  m->subsurface_color[0] = m->subsurface_color[1] = m->subsurface_color[2] = 1.0f;
  m->ior = 100.0f;
  m->sky_color[0] = 0.7f;
  m->sky_color[1] = 0.8f;
  m->sky_color[2] = 1.0f;
  m->sky_floor = 0.2f;
  m->sky_scale = 2.0f;
  m->sky_radius = 36.0f;
  m->sky_axis = 1;
}

int rm_ctx_create(int device, rm_ctx** out) {
  if (!out) return fail(nullptr, RM_ERR_INVALID, "rm_ctx_create: out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, RM_ERR_NO_DEVICE, "no HIP device: libhip_raymarch has no CPU fallback (" +
                                               std::string(e == hipSuccess ? "device count 0" : hipGetErrorString(e)) + ")");
  if (device < 0 || device >= count) return fail(nullptr, RM_ERR_INVALID, "rm_ctx_create: device index out of range");
  rm_ctx* ctx = new (std::nothrow) rm_ctx();
  if (!ctx) return fail(nullptr, RM_ERR_DEVICE, "out of host memory");
  ctx->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&ctx->switch_ev, hipEventDisableTiming)) != hipSuccess) {
    std::string msg = std::string("rm_ctx_create: ") + hipGetErrorString(e);
    delete ctx;
    return fail(nullptr, RM_ERR_DEVICE, msg);
  }
  ctx->stream = ctx->own_stream;
  if (const char* v = std::getenv("RM_COST_ORDER")) ctx->lpt_enabled = std::atoi(v) != 0;
  if (const char* v = std::getenv("RM_SAMPLES_IN_FLIGHT")) { int n = std::atoi(v); if (n >= 1 && n <= RM_SP_MAX) ctx->sp.depth = n; }
  if (const char* v = std::getenv("RM_CULL_MIN_PIXELS")) { long long n = std::atoll(v); if (n >= 0) ctx->cull_min_pixels = n; }  // (the tests: 0, so that small renders go through the grid)
  {  // the culling grids of this context's scenes: a sixteenth of the device's memory, at most 1 GiB (a 256-row table's grid is 126 MB)
    size_t free_b = 0, total_b = 0;
    ctx->cull_budget = (size_t)1 << 30;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b / 16 < ctx->cull_budget) ctx->cull_budget = total_b / 16;
    else (void)hipGetLastError();
  }
  *out = ctx;
  return RM_OK;
}

void rm_ctx_destroy(rm_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
#if RM_WITH_WAVEFRONT
  ctx->wf.destroy();
#endif
  if (ctx->lpt_stream) { (void)hipStreamSynchronize(ctx->lpt_stream); (void)hipStreamDestroy(ctx->lpt_stream); }
  for (auto& l : ctx->lpt) l.destroy();
  ctx->sp.destroy();
  for (auto& s : ctx->scratch) s.release();
  ctx->shard.destroy();
  if (ctx->cull_stream) { (void)hipStreamSynchronize(ctx->cull_stream); (void)hipStreamDestroy(ctx->cull_stream); }
  for (auto& b : ctx->cull_pool) (void)hipFree(b.p);
  if (ctx->cull_event) (void)hipEventDestroy(ctx->cull_event);
  if (ctx->cull_order) (void)hipEventDestroy(ctx->cull_order);
  for (auto& b : ctx->buffers) (void)hipFree(b.first);  // rm_buffer_create'd memory the host did not destroy
  if (ctx->switch_ev) (void)hipEventDestroy(ctx->switch_ev);
  ctx->mesh_spans.destroy();
  if (ctx->mesh_order) (void)hipEventDestroy(ctx->mesh_order);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

const char* rm_last_error(const rm_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int rm_ctx_set_stream(rm_ctx* ctx, void* hip_stream) {
  if (!ctx) return RM_ERR_INVALID;
  hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  if (next == ctx->stream) return RM_OK;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  // Everything already queued on the old stream (the zeroing of rm_fb_create / rm_fb_clear, uploads, renders, the
  // blends of samples in flight) is ordered before whatever the caller enqueues on the new one: an event, no host wait.
  RM_HIP(ctx, hipEventRecord(ctx->switch_ev, ctx->stream));
  RM_HIP(ctx, hipStreamWaitEvent(next, ctx->switch_ev, 0));
  ctx->stream = next;
  return RM_OK;
}

int rm_ctx_set_samples_in_flight(rm_ctx* ctx, int n) {
  if (!ctx) return RM_ERR_INVALID;
  if (n < 1 || n > RM_SP_MAX) return fail(ctx, RM_ERR_INVALID, "rm_ctx_set_samples_in_flight: n must be in 1..8");
  if (ctx->sp.ready) RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->sp.depth = n;
  ctx->warning.clear();
  if (n > 1) {
    // every sample in flight renders on a side stream; the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES
    // hardware queues (default 4, read when the runtime starts) and streams that share a queue serialise
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    const int queues = q ? std::atoi(q) : 4;
    if (queues < 8) {
      char msg[320];
      std::snprintf(msg, sizeof msg, "warning: %d samples in flight but GPU_MAX_HW_QUEUES is %s%d: the side streams will share hardware queues and "
                    "serialise (measured: 0.59 instead of 0.42 ms per sample on a 1/8 shard)", n, q ? "" : "unset = ", queues);
      ctx->warning = msg;  // accepted all the same: RM_OK, and rm_last_error stays what it was -- the note goes to rm_ctx_last_warning
    }
  }
  return RM_OK;
}

const char* rm_ctx_last_warning(const rm_ctx* ctx) { return ctx ? ctx->warning.c_str() : ""; }

int rm_ctx_set_cost_order(rm_ctx* ctx, int on) {
  if (!ctx) return RM_ERR_INVALID;
  ctx->lpt_enabled = on != 0;
  for (auto& l : ctx->lpt) l.forget();
  return RM_OK;
}

int rm_ctx_set_retire_eps(rm_ctx* ctx, float eps) {
  if (!ctx) return RM_ERR_INVALID;
  if (!(eps >= 0.0f && eps <= 1e-3f)) return fail(ctx, RM_ERR_INVALID, "rm_ctx_set_retire_eps: eps must be in [0, 1e-3]");
  ctx->retire_eps = eps;
  return RM_OK;
}

int rm_ctx_set_gl_stack(rm_ctx* ctx, int on) {
  if (!ctx) return RM_ERR_INVALID;
  if (on != 0 && on != 1 && on != 2) return fail(ctx, RM_ERR_INVALID, "rm_ctx_set_gl_stack: 0 (off), 1 (on) or 2 (on, with the stack's own tan)");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // samples in flight finish in the arithmetic they started in
  // The kernels read the stack's-own-tan switch from a __device__ symbol: one per DEVICE (the contexts of a device share it).
  // What each device holds is remembered per device, under a lock; the copy is synchronous (its source is this frame's).
  static std::mutex guard;
  static int native_tan[64];  // 0 after the module is loaded on a device, like the symbol
  if (on != 0) {
    std::lock_guard<std::mutex> lock(guard);
    const int slot = ctx->device & 63, v = on == 2 ? 1 : 0;
    if (native_tan[slot] != v) {
      RM_HIP(ctx, hipDeviceSynchronize());  // launches of the device's other contexts finish with the value they started with
      RM_HIP(ctx, rm_gl_set_native_tan(v, nullptr));
      native_tan[slot] = v;
    }
  }
  ctx->gl_stack = on != 0;
  return RM_OK;
}

int rm_debug_counters(rm_ctx* ctx, unsigned long long* out16, int reset) {
  if (!ctx || !out16) return RM_ERR_INVALID;
  for (int i = 0; i < 16; i++) out16[i] = 0;
#if RM_WITH_WAVEFRONT  // (the product has no stats: zeros)
  if (!ctx->wf.stats) return RM_OK;
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  RM_HIP(ctx, hipMemcpy(out16, ctx->wf.stats, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
  if (reset) RM_HIP(ctx, hipMemset(ctx->wf.stats, 0, sizeof(unsigned long long) * 16));
#endif
  return RM_OK;
}

int rm_ctx_last_pipeline(const rm_ctx* ctx) { return ctx ? ctx->last_pipeline : RM_PIPELINE_NONE; }

int rm_device_memory(rm_ctx* ctx, size_t* free_bytes, size_t* total_bytes) {
  if (!ctx || !free_bytes || !total_bytes) return fail(ctx, RM_ERR_INVALID, "rm_device_memory: NULL argument");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, hipMemGetInfo(free_bytes, total_bytes));
  return RM_OK;
}

int rm_sync(rm_ctx* ctx) {
  if (!ctx) return RM_ERR_INVALID;
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

// ---- scene -------------------------------------------------------------------

static bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// Where an escaping ray of a primitive table ends (Sdf<RM_SCENE_TABLE>::far_jump).  Without domain rows every shape lies
// inside a sphere about the origin, and outside it the fold is bounded below: a shape's distance is >= |p| - (|c| + extent),
// min / max keep that bound (max(d, -di) and max(d, di) only raise d), and a CHAIN of smooth unions stays within k of it however
// long it is: one smooth union is at most k / 4 (1 - |t| / k)^2 below min(d, di), t = di - d, so once the running value is D below the
// bound a term above the bound (|t| > D) lowers it by at most k / 4 (1 - D / k)^2 more -- D + k / 4 (1 - D / k)^2 <= k on [0, k], and
// nothing at all from D = k on -- and a term below the bound resets D to at most k as well (checked numerically: 0.995 k under a
// greedy adversary, 0.94 k for 200 equal terms).  Round 3 first allowed k / 4 per smooth union: R' = 5.9 for CSG-64 instead of 2.95,
// and every escaping ray marched to twice the radius before its jump.  A ray out
// there that is not moving inward never returns and doubles its distance from step to step until |p|^2 overflows; at that
// step p - c = p for every shape (the centres are below the spacing of floats of that size), so every shape's distance is
// +Inf at once and the march's step is the fold of all-+Inf terms: +Inf -- the position becomes +-Inf by the sign of the
// direction components, a fixed point -- or NaN, when a smooth union meets Inf - Inf -- then every coordinate is NaN, for
// good.  That fold is evaluated here, with the operators' own semantics (IEEE minNum / maxNum drop a NaN, as v_min / v_max do).
static void table_far_field(const RmSceneDesc* desc, DevScene* dev) {
  dev->far_end = 0;
  dev->far_r2 = 0.0f;
  double reach = 0.0, kmax = 0.0;
  int smooth = 0;
  float d = 0.0f;
  bool first = true;
  const float inf = std::numeric_limits<float>::infinity();
  for (int i = 0; i < desc->nprims; i++) {
    const RmPrim& p = desc->prims[i];
    const int type = p.type & 0xff, op = (p.type >> 8) & 0xff;
    if (type == RM_PRIM_REPEAT || type == RM_PRIM_FOLD || type == RM_PRIM_KIND) return;  // a tiled or folded space has no far field; a kind's estimator is not a sphere's or a box's
    if (type > RM_PRIM_KIND || op > RM_OP_INTERSECT) return;  // ABI 8's shapes and smooth operators: no end state has been derived for them (a plane has no far field at all)
    const double c = std::sqrt((double)p.center[0] * p.center[0] + (double)p.center[1] * p.center[1] + (double)p.center[2] * p.center[2]);
    const double extent = type == RM_PRIM_SPHERE ? std::fabs((double)p.size[0])
                                                 : std::sqrt((double)p.size[0] * p.size[0] + (double)p.size[1] * p.size[1] + (double)p.size[2] * p.size[2]);
    reach = std::fmax(reach, c + extent);
    if (first) { d = inf; first = false; continue; }
    if (op == RM_OP_UNION) d = std::fmin(d, inf);
    else if (op == RM_OP_SMOOTH_UNION) { d = std::numeric_limits<float>::quiet_NaN(); smooth++; kmax = std::fmax(kmax, std::fabs((double)p.k)); }  // Inf - Inf, or a NaN handed on
    else if (op == RM_OP_SUBTRACT) d = std::fmax(d, -inf);
    else d = std::fmax(d, inf);
  }
  const double r = 2.0 * (reach + (smooth ? 1.01 * kmax : 0.0)) + 1.0;
  if (first || !(r < 1e9)) return;
  dev->far_r2 = (float)(r * r);
  dev->far_end = d == inf ? 1 : (d != d ? 2 : 0);
  // A ray that passes every shape at a distance (Sdf<RM_SCENE_TABLE>::clear_miss): if it stays K = k_max + b0 clear of every shape's
  // bounding sphere, the fold is >= b0 all along it (a chain of smooth unions is within k_max of the nearest term): the march never
  // settles.  How long can it take to leave?  Let rho hold every shape's sphere and K (rho = 1.15 (reach + k_max), b0 <= rho / 8).
  // Inside that sphere a step is >= b0, outside >= |x| - rho + b0; two steps bring a ray from up to 60 Rp away to it, and the worst
  // chord (through the centre) is crossed and the ray out at 2.6 rho -- beyond the jump's 2 Rp, moving outward -- within
  // 2 rho / (0.99 b0) + 6 steps (tools: the recurrence iterated over every closest approach).  Then the jump's first case: far_need's 71 steps.
  // So a march with `left` steps may take b0 = 2.05 rho / (left - 84): 128 steps -> b0 = rho / 21 (C4: 0.16, clearance 0.37).
  if (dev->far_end != 0 && reach + kmax >= 1.05) {
    dev->clear_k = (float)((smooth ? 1.01 * kmax : 0.0) + 1e-3 * (1.0 + reach));
    dev->clear_rho = (float)(1.15 * (reach + (smooth ? kmax : 0.0)));
  }
}

// The culling grid of a primitive table without domain rows (rm_params.hpp CullGrid; rm_kernels.inc rm_cull_build_kernel has the
// argument and fills it on the device; fast policy only): nested cubes of RM_CULL_N^3 cells about the shapes' bounding box, each
// twice as wide as the one before, out to where fp32 no longer tells the rows apart.
// For tables of at least RM_CULL_MIN_ROWS rows (round 3: those of mostly hard operators; round 4: every one, rm_params.hpp rm_cull_cell).
#ifndef RM_CULL_MIN_ROWS
#define RM_CULL_MIN_ROWS 12
#endif
#ifndef RM_CULL_N
#define RM_CULL_N 32
#endif
#ifndef RM_CULL_N_SMOOTH
#define RM_CULL_N_SMOOTH 128  // C4 12.4 ms without the grid, 9.8 with 64^3 cells, 9.1 with 128^3 (profiles/r04_smooth_union_culling.txt)
#endif
#ifndef RM_CULL_SMOOTH_LEVELS
#define RM_CULL_SMOOTH_LEVELS 8  // out to 128 scene widths (a camera further away folds every row until its rays get there)
#endif
#ifndef RM_CULL_OUTER_DIV
#define RM_CULL_OUTER_DIV 2  // the levels around the first: cells twice as wide (1: as fine as level 0 -- rounds 3-4, 134 MB per 64 rows instead of 31.5)
#endif
#ifndef RM_CULL_MAX_LEVELS
#define RM_CULL_MAX_LEVELS 18
#endif
static bool table_cull_params(const RmSceneDesc* desc, CullGrid* g, CullBuild* build) {
  *g = CullGrid{};
  *build = CullBuild{};
  const int n = desc->nprims;
  if (n < RM_CULL_MIN_ROWS) return false;
  if (const char* v = std::getenv("RM_NO_CULL"))
    if (v[0] == '1') return false;
  double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30}, kmax = 0.0;
  for (int i = 0; i < n; i++) {
    const RmPrim& p = desc->prims[i];
    const int type = p.type & 0xff;
    if (type != RM_PRIM_SPHERE && type != RM_PRIM_BOX) return false;  // domain rows: no grid in the table's own space (ABI 8's shapes: no rule)
    if (((p.type >> 8) & 0xff) > RM_OP_INTERSECT) return false;         // ... nor for its smooth subtraction / intersection
    for (int a = 0; a < 3; a++) {
      const double e = std::fabs((double)(type == RM_PRIM_SPHERE ? p.size[0] : p.size[a]));
      lo[a] = std::fmin(lo[a], p.center[a] - e);
      hi[a] = std::fmax(hi[a], p.center[a] + e);
    }
    if (((p.type >> 8) & 0xff) == RM_OP_SMOOTH_UNION) kmax = std::fmax(kmax, (double)p.k);
  }
  // a table of mostly smooth unions (CSG-64; round 4): their far rows are dropped where the rounding they perform is provably the
  // identity (rm_params.hpp rm_cull_cell) -- on a finer grid, the binade tests want small cells
  const bool smooth_spheres = rm_cull_mostly_smooth(desc->prims, n);
  if (smooth_spheres && n < RM_TABLE_BIG_ROWS) return false;  // about half of such a table's rows stay: too few to pay for the lookup
  double half = 0.0, reach = 0.0;
  for (int a = 0; a < 3; a++) {
    half = std::fmax(half, 0.5 * (hi[a] - lo[a]));
    reach = std::fmax(reach, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
    build->centre[a] = 0.5 * (lo[a] + hi[a]);
  }
  half = 1.1 * half + kmax + 1e-3;
  if (!(half < 1e6) || !(reach < 1e6)) return false;
  // levels: out to where the fp32 allowance of the build kernel (1.2e-7 (n + 8) |coordinates|) exceeds the scene's own width
  int levels = 1;
  while (levels < RM_CULL_MAX_LEVELS && 1.2e-7 * (n + 8) * 1.74 * std::ldexp(half, levels) < 2.0 * half) levels++;
  if (smooth_spheres && levels > RM_CULL_SMOOTH_LEVELS) levels = RM_CULL_SMOOTH_LEVELS;
  build->half0 = half;
  build->reach = reach;
  build->nprims = n;
  const int cells = smooth_spheres ? (n >= 32 ? RM_CULL_N_SMOOTH : RM_CULL_N_SMOOTH / 2) : RM_CULL_N;  // (17 MB instead of 134 for the shorter tables)
  build->n = cells;
  build->n_outer = smooth_spheres ? cells / RM_CULL_OUTER_DIV : cells;  // (the hard operators' sharper test works on large cells as it is)
  build->levels = levels;
  build->words = (n + 63) / 64;
  for (int a = 0; a < 3; a++) g->centre[a] = (float)build->centre[a];
  g->inv_half0 = (float)(1.0 / half);
  g->scale0 = (float)(cells / (2.0 * half));
  g->n = cells;
  g->n_outer = build->n_outer;
  g->levels = levels;
  g->words = build->words;
  return true;
}

int rm_debug_cull_cell(const RmSceneDesc* desc, const double* centre, double radius, double margin, unsigned long long* out_words) {
  if (!desc || !centre || !out_words || desc->kind != RM_SCENE_TABLE || desc->nprims < 1 || desc->nprims > RM_MAX_PRIMS || !desc->prims) return RM_ERR_INVALID;
  for (int i = 0; i < desc->nprims; i++) {
    const int type = desc->prims[i].type & 0xff;
    if ((type != RM_PRIM_SPHERE && type != RM_PRIM_BOX) || ((desc->prims[i].type >> 8) & 0xff) > RM_OP_INTERSECT) return RM_ERR_INVALID;
  }
  rm_cull_cell(desc->prims, desc->nprims, (desc->nprims + 63) / 64, centre, radius, margin, out_words);
  return RM_OK;
}

// The far field of the kaleidoscopic kinds (rm_device.hpp Sdf<RM_SCENE_KIFS_BOX>::far_jump, Sdf<RM_SCENE_KIFS_TREE>::eval).
// A level maps t to rotate(|t / s| - off): norms obey |t'| >= |t| / s - |off|, so after n levels |t_n| s^n >= |p| - |off| s / (1 - s),
// and sdBox(q, b) >= |q| - |b|: every level's box is >= |p| - R' with R' = |off| s / (1 - s) + |b| (b <= the unit-level box).
//  * rotation-fractal (one box at the last level): the estimate grows with |p| and a ray that leaves overflows like a table's;
//    far_end = 1 (the +-Inf pattern is a fixed point whatever the folds make of an infinite point: sdBox drops their NaNs and
//    returns +Inf or 0), provided the deepest point t_n = p / s^n stays finite up to the overflow of |p|^2 (s^n >= 1e-15).
//  * tree / smooth-tree: the estimate starts from min_dist = 9999, so beyond |p| = 9999 + R' it IS 9999 -- min(9999, box), and
//    the smooth union's mix(box, 9999, 1) = box + (9999 - box) is exact while box < 2^24 -- and a ray out there walks 9999 per
//    step to the end of its budget: far_end = 3 lets the fast evaluation return the constant without its levels.
static void kifs_far_field(const RmSceneDesc* desc, DevScene* dev) {
  dev->far_end = 0;
  dev->far_r2 = 0.0f;
  const double iters = desc->params[RM_P_KIFS_ITERATIONS], s = desc->params[RM_P_KIFS_SCALE], off = std::fabs((double)desc->params[RM_P_KIFS_OFFSET]);
  if (!(s > 0.05 && s <= 0.9) || !(iters >= 0.0 && iters <= 64.0) || !(off < 1e6)) return;
  if (desc->kind == RM_SCENE_KIFS_BOX) {
    if (std::pow(s, std::ceil(iters)) < 1e-15) return;
    const double r = 2.0 * std::sqrt(3.0) * (off * s / (1.0 - s) + 1.0) + 1.0;
    dev->far_r2 = (float)(r * r);
    dev->far_end = 1;
  } else {
    const double r = 9999.0 + 1.01 * (off * s / (1.0 - s) + 1.0) + 2.0;
    dev->far_r2 = (float)(r * r);
    dev->far_end = 3;
  }
}

int rm_scene_create(rm_ctx* ctx, const RmSceneDesc* desc, rm_scene** out) {
  if (!ctx || !desc || !out) return fail(ctx, RM_ERR_INVALID, "rm_scene_create: NULL argument");
  *out = nullptr;
  char buf[256];
  // the analogue of the GLSL compile: reject what the kernels cannot run, with an "info log"
  if (desc->kind < 0 || desc->kind >= RM_SCENE_KIND_COUNT) {
    std::snprintf(buf, sizeof buf, "scene: unknown kind %d", desc->kind);
    return fail(ctx, RM_ERR_INVALID, buf);
  }
  if (!finite_all(desc->params, 16)) return fail(ctx, RM_ERR_INVALID, "scene: non-finite parameter");
  if (desc->material.sky_axis < 0 || desc->material.sky_axis > 2) return fail(ctx, RM_ERR_INVALID, "scene: material.sky_axis must be 0, 1 or 2");
  if (desc->nsurfaces < 0 || desc->nsurfaces > RM_MAX_SURFACES || (desc->nsurfaces > 0 && (!desc->surfaces || desc->kind != RM_SCENE_TABLE))) {
    std::snprintf(buf, sizeof buf, "scene: 0..%d surfaces, for a primitive table (got %d)", RM_MAX_SURFACES, desc->nsurfaces);
    return fail(ctx, RM_ERR_INVALID, buf);
  }
  for (int i = 0; i < desc->nsurfaces; i++)
    if (!finite_all(reinterpret_cast<const float*>(&desc->surfaces[i]), 12)) return fail(ctx, RM_ERR_INVALID, "scene: non-finite surface value");
  if (desc->kind == RM_SCENE_TABLE) {
    if (desc->nprims < 1 || desc->nprims > RM_MAX_PRIMS || !desc->prims) {
      std::snprintf(buf, sizeof buf, "scene: primitive table needs 1..%d rows (got %d)", RM_MAX_PRIMS, desc->nprims);
      return fail(ctx, RM_ERR_INVALID, buf);
    }
    int shapes = 0, kind_of_rows = -1;
    for (int i = 0; i < desc->nprims; i++) {
      const RmPrim& p = desc->prims[i];
      const int type = p.type & 0xff, op = (p.type >> 8) & 0xff;
      if (type > RM_PRIM_PLANE || op > RM_OP_SMOOTH_INTERSECT || (p.type >> 24) != 0) {
        std::snprintf(buf, sizeof buf, "scene: row %d: unknown primitive/operator 0x%x", i, p.type);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      const int surface = (p.type >> 16) & 0xff;
      if (type == RM_PRIM_KIND) {
        const int kind = (int)p.size[0];
        if ((float)kind != p.size[0] || (kind != RM_SCENE_MANDELBULB && kind != RM_SCENE_SPHERE_LATTICE)) {
          std::snprintf(buf, sizeof buf, "scene: row %d: a kind row evaluates RM_SCENE_MANDELBULB or RM_SCENE_SPHERE_LATTICE (size[0] = %g)", i, (double)p.size[0]);
          return fail(ctx, RM_ERR_INVALID, buf);
        }
        if (kind_of_rows >= 0 && kind_of_rows != kind) return fail(ctx, RM_ERR_INVALID, "scene: the kind rows of a table evaluate ONE kind (its parameters are the scene's parameter block)");
        kind_of_rows = kind;
        if (kind == RM_SCENE_MANDELBULB && !(desc->params[RM_P_BULB_ITERATIONS] >= 0.0f && desc->params[RM_P_BULB_ITERATIONS] <= 64.0f))
          return fail(ctx, RM_ERR_INVALID, "scene: mandelbulb iterations must be in 0..64");
        if (kind == RM_SCENE_SPHERE_LATTICE && !(desc->params[RM_P_LATTICE_PERIOD] > 0.0f)) return fail(ctx, RM_ERR_INVALID, "scene: the lattice's period must be > 0");
      }
      const bool shape = type != RM_PRIM_REPEAT && type != RM_PRIM_FOLD;
      if (surface > desc->nsurfaces || (surface != 0 && !shape)) {
        std::snprintf(buf, sizeof buf, "scene: row %d: surface %d of %d (only shape rows name a surface)", i, surface, desc->nsurfaces);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      if (!finite_all(p.center, 3) || !finite_all(p.size, 3) || !std::isfinite(p.k)) {
        std::snprintf(buf, sizeof buf, "scene: row %d: non-finite value", i);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      if (type == RM_PRIM_REPEAT && !(p.size[0] > 0.0f && p.size[1] > 0.0f && p.size[2] > 0.0f)) {
        std::snprintf(buf, sizeof buf, "scene: row %d: repeat needs a period > 0 on every axis", i);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      if (type == RM_PRIM_FOLD && !(p.k > 0.0f)) {
        std::snprintf(buf, sizeof buf, "scene: row %d: fold needs scale > 0", i);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      if (shape && (op == RM_OP_SMOOTH_UNION || op == RM_OP_SMOOTH_SUBTRACT || op == RM_OP_SMOOTH_INTERSECT) && !(p.k > 0.0f) && shapes > 0) {
        std::snprintf(buf, sizeof buf, "scene: row %d: smooth %s needs k > 0", i, op == RM_OP_SMOOTH_UNION ? "union" : op == RM_OP_SMOOTH_SUBTRACT ? "subtraction" : "intersection");
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      if ((type == RM_PRIM_TORUS || type == RM_PRIM_CYLINDER) && !(p.size[0] >= 0.0f && p.size[1] >= 0.0f)) {
        std::snprintf(buf, sizeof buf, "scene: row %d: a torus / cylinder needs radii (and a half height) >= 0", i);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      if (type == RM_PRIM_PLANE && !(p.size[0] != 0.0f || p.size[1] != 0.0f || p.size[2] != 0.0f)) {
        std::snprintf(buf, sizeof buf, "scene: row %d: a plane needs a normal", i);
        return fail(ctx, RM_ERR_INVALID, buf);
      }
      shapes += shape ? 1 : 0;
    }
    if (shapes == 0) return fail(ctx, RM_ERR_INVALID, "scene: the table has no shape row (sphere / box), only domain operators");
  } else if (desc->kind == RM_SCENE_MANDELBULB) {
    if (!(desc->params[RM_P_BULB_ITERATIONS] >= 0.0f && desc->params[RM_P_BULB_ITERATIONS] <= 64.0f))
      return fail(ctx, RM_ERR_INVALID, "scene: mandelbulb iterations must be in 0..64");
  } else if (desc->kind == RM_SCENE_SPHERE_GRID || desc->kind == RM_SCENE_MENGER || desc->kind == RM_SCENE_KIFS_TREE ||
             desc->kind == RM_SCENE_KIFS_BOX) {
    // one evaluation loops `iterations` times, a sample evaluates ~10^3 times per pixel: an unbounded count is an endless kernel
    const int slot = desc->kind == RM_SCENE_SPHERE_GRID ? RM_P_GRID_ITERATIONS : desc->kind == RM_SCENE_MENGER ? RM_P_MENGER_ITERATIONS : RM_P_KIFS_ITERATIONS;
    if (!(desc->params[slot] <= 64.0f)) return fail(ctx, RM_ERR_INVALID, "scene: fractal iterations must be <= 64");
  }
  rm_scene* s = new (std::nothrow) rm_scene();
  if (!s) return fail(ctx, RM_ERR_DEVICE, "out of host memory");
  s->ctx = ctx;
  s->dev.kind = desc->kind;
  s->dev.nprims = desc->kind == RM_SCENE_TABLE ? desc->nprims : 0;
  if (desc->kind == RM_SCENE_TABLE) {
    bool spheres_smooth = true, domain = false, boxes = false, surfaces = false, kinds = false, more = false;
    for (int i = 0; i < desc->nprims; i++) {
      const int type = desc->prims[i].type & 0xff, op = (desc->prims[i].type >> 8) & 0xff;
      if (((desc->prims[i].type >> 16) & 0xff) != 0) surfaces = true;
      if (type != RM_PRIM_SPHERE || (i > 0 && op != RM_OP_SMOOTH_UNION)) spheres_smooth = false;
      if (type == RM_PRIM_REPEAT || type == RM_PRIM_FOLD) domain = true;
      if (type == RM_PRIM_BOX || type == RM_PRIM_TORUS || type == RM_PRIM_CYLINDER || type == RM_PRIM_PLANE) boxes = true;  // (RM_TABLE_NO_BOXES is a promise about spheres)
      if (type == RM_PRIM_KIND) kinds = true;
      if (type > RM_PRIM_KIND || op > RM_OP_INTERSECT) more = true;
    }
    // (RM_TABLE_NO_BOXES promises a non-finite distance at a non-finite point: not said of a kind's estimator, so a kind row withdraws it)
    s->dev.table_flags = (spheres_smooth ? RM_TABLE_SPHERES_SMOOTH : 0) | (domain ? RM_TABLE_HAS_DOMAIN : 0) | (boxes || kinds ? 0 : RM_TABLE_NO_BOXES) |
                         (surfaces ? RM_TABLE_HAS_SURFACES : 0) | (kinds ? RM_TABLE_HAS_KIND : 0) | (more ? RM_TABLE_MORE : 0);
    if (spheres_smooth && desc->nprims >= 2 && desc->nprims * 3 <= RM_MAX_PRIMS * 2) {  // one smooth-union radius for the whole table (the usual case): it travels as a kernel argument, and a compact image of the rows fits behind them in LDS
      bool one_k = true;
      for (int i = 2; i < desc->nprims; i++) one_k = one_k && desc->prims[i].k == desc->prims[1].k;
      if (one_k) s->dev.table_flags |= RM_TABLE_UNIFORM_K;
    }
  }
  if (desc->kind == RM_SCENE_TABLE) table_far_field(desc, &s->dev);
  if (desc->kind == RM_SCENE_KIFS_BOX || desc->kind == RM_SCENE_KIFS_TREE) kifs_far_field(desc, &s->dev);
  if (desc->kind == RM_SCENE_SPHERE_GRID) {  // the sphere-grid fractal lives inside its big sphere (Sdf<RM_SCENE_SPHERE_GRID>::far_jump)
    const float* c = &desc->params[RM_P_GRID_CENTER];
    const double r = 2.0 * (std::sqrt((double)c[0] * c[0] + (double)c[1] * c[1] + (double)c[2] * c[2]) + std::fabs((double)desc->params[RM_P_GRID_BIG_SIZE])) + 1.0;
    if (r < 1e9) { s->dev.far_r2 = (float)(r * r); s->dev.far_end = 1; }
  }
  std::memcpy(s->dev.p, desc->params, sizeof s->dev.p);
  if (s->dev.table_flags & RM_TABLE_UNIFORM_K) {
    s->dev.p[0] = desc->prims[1].k;
    s->dev.p[1] = 0.5f * (1.0f / desc->prims[1].k);  // the bits the kernel's staging computes per row otherwise
  }
  s->dev.mat = desc->material;
  (void)hipSetDevice(ctx->device);
  if (s->dev.nprims > 0) {
    const size_t bytes = sizeof(RmPrim) * (size_t)s->dev.nprims;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_prims), bytes);
    if (e == hipSuccess) e = hipMemcpy(s->d_prims, desc->prims, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (s->d_prims) (void)hipFree(s->d_prims);
      delete s;
      return fail(ctx, RM_ERR_DEVICE, std::string("rm_scene_create: ") + hipGetErrorString(e));
    }
    s->dev.prims = s->d_prims;
  }
  if (desc->kind == RM_SCENE_TABLE) {
    CullGrid g;
    CullBuild build;
    if (table_cull_params(desc, &g, &build)) {  // built on first use: scene_cull_grid
      s->cull_wanted = true;
      s->cull_grid = g;
      s->cull_build = build;
    }
  }
  if (s->dev.table_flags & RM_TABLE_HAS_SURFACES) {  // entry 0 = the scene's own material block, then the surfaces as given
    RmSurface all[RM_MAX_SURFACES + 1];
    const RmMaterial& m = desc->material;
    all[0] = RmSurface{{m.diffuse[0], m.diffuse[1], m.diffuse[2]}, m.roughness, {m.specular[0], m.specular[1], m.specular[2]}, m.subsurface,
                       {m.subsurface_color[0], m.subsurface_color[1], m.subsurface_color[2]}, m.ior};
    for (int i = 0; i < desc->nsurfaces; i++) all[i + 1] = desc->surfaces[i];
    const size_t bytes = sizeof(RmSurface) * (size_t)(desc->nsurfaces + 1);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_surfaces), bytes);
    if (e == hipSuccess) e = hipMemcpy(s->d_surfaces, all, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (s->d_surfaces) (void)hipFree(s->d_surfaces);
      if (s->d_prims) (void)hipFree(s->d_prims);
      delete s;
      return fail(ctx, RM_ERR_DEVICE, std::string("rm_scene_create: ") + hipGetErrorString(e));
    }
    s->dev.surfaces = s->d_surfaces;
    s->dev.nsurfaces = desc->nsurfaces;
  }
  *out = s;
  return RM_OK;
}

static void cull_release(rm_ctx* ctx, rm_scene* s, bool idle);
void rm_scene_destroy(rm_scene* scene) {
  if (!scene) return;
  (void)hipSetDevice(scene->ctx->device);
  (void)hipStreamSynchronize(scene->ctx->stream);
  if (scene->d_prims) (void)hipFree(scene->d_prims);
  if (scene->d_surfaces) (void)hipFree(scene->d_surfaces);
  cull_release(scene->ctx, scene, true);  // (to the context's pool: the next scene's grid is usually the same size; the stream has been waited for above)
  delete scene;
}

// ---- framebuffers --------------------------------------------------------------

static int fb_check(rm_ctx* ctx, int width, int height, int row_begin, int row_count) {
  if (width < 1 || height < 1 || width > 65536 || height > 65536) return fail(ctx, RM_ERR_INVALID, "framebuffer: size must be 1..65536");
  // ray and tile counts are 32-bit in the kernels' index arithmetic (8x8 tiles round a frame up by < 2 %)
  if ((long long)width * (long long)height > (1ll << 28)) return fail(ctx, RM_ERR_INVALID, "framebuffer: width x height must be <= 2^28 pixels");
  if (row_begin < 0 || row_count < 1 || row_begin + row_count > height) return fail(ctx, RM_ERR_INVALID, "framebuffer: row window outside the image");
  return RM_OK;
}

static int gbuffer_check(rm_ctx* ctx, int gbuffer, const char* what) {
  if (gbuffer != RM_GBUFFER_F32 && gbuffer != RM_GBUFFER_F16)
    return fail(ctx, RM_ERR_INVALID, std::string(what) + ": unknown G-buffer format (RM_GBUFFER_F32 or RM_GBUFFER_F16)");
  return RM_OK;
}

// caller-owned planes: colour 16-byte aligned, the G-buffer planes aligned to their own pixel (16 or 8 bytes)
static int planes_aligned(const void* color, const void* normal_dof, const void* albedo_depth, int gbuffer) {
  const uintptr_t g = (uintptr_t)plane_px_bytes(gbuffer, 1) - 1;
  return !((reinterpret_cast<uintptr_t>(color) & 15u) || (reinterpret_cast<uintptr_t>(normal_dof) & g) || (reinterpret_cast<uintptr_t>(albedo_depth) & g));
}

// Frees the planes the library allocated (the moments plane is always the library's) and the framebuffer itself.
static void fb_release(rm_fb* fb) {
  if (fb->owned)
    for (auto* pl : fb->plane)
      if (pl) (void)hipFree(pl);
  if (fb->moments) (void)hipFree(fb->moments);
  delete fb;
}

// Allocates the planes the library owns -- 0..2, and 3, the moments plane, when asked for -- and zeroes them on the context's
// stream.  One way out of a failure: what was allocated is freed, and the framebuffer with it.
static int fb_allocate(rm_fb* fb, bool moments, const char* who) {
  rm_ctx* ctx = fb->ctx;
  (void)hipSetDevice(ctx->device);
  for (int i = 0; i < (moments ? 4 : 3); i++) {
    const size_t bytes = plane_bytes(fb, i);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (i == RM_PLANE_MOMENTS) fb->moments = static_cast<float2*>(p);
    else fb->plane[i] = static_cast<float4*>(p);
    if (e == hipSuccess) e = hipMemsetAsync(p, 0, bytes, ctx->stream);
    if (e != hipSuccess) {
      fb_release(fb);
      return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
  }
  return RM_OK;
}

// The framebuffer every constructor ends in, after its own checks: over the caller's three planes, or with planes of the
// library's own (zeroed; with the moments plane when asked for).
static int fb_make(rm_ctx* ctx, const char* who, const FbGeometry& geometry, int gbuffer, void* const* planes, bool moments, rm_fb** out) {
  rm_fb* fb = new (std::nothrow) rm_fb();
  if (!fb) return fail(ctx, RM_ERR_DEVICE, "out of host memory");
  static_cast<FbGeometry&>(*fb) = geometry;
  fb->ctx = ctx;
  fb->gbuffer = gbuffer;
  fb->owned = planes == nullptr;
  if (planes)
    for (int i = 0; i < 3; i++) fb->plane[i] = static_cast<float4*>(planes[i]);
  else if (int rc = fb_allocate(fb, moments, who))
    return rc;
  *out = fb;
  return RM_OK;
}

int rm_fb_create(rm_ctx* ctx, int width, int height, int row_begin, int row_count, rm_fb** out) {
  return rm_fb_create_fmt(ctx, width, height, row_begin, row_count, RM_GBUFFER_F32, out);
}

int rm_fb_create_fmt(rm_ctx* ctx, int width, int height, int row_begin, int row_count, int gbuffer, rm_fb** out) {
  if (!ctx || !out) return fail(ctx, RM_ERR_INVALID, "rm_fb_create: NULL argument");
  *out = nullptr;
  const bool moments = (gbuffer & RM_FB_MOMENTS) != 0;
  gbuffer &= ~RM_FB_MOMENTS;
  if (int rc = gbuffer_check(ctx, gbuffer, "rm_fb_create")) return rc;
  if (int rc = fb_check(ctx, width, height, row_begin, row_count)) return rc;
  return fb_make(ctx, "rm_fb_create", FbGeometry{width, height, row_begin, row_count}, gbuffer, nullptr, moments, out);
}

// rows r < y owned by a striped framebuffer
static int striped_rows_below(int y, int stripe, int parts, int part) {
  const int period = stripe * parts;
  const int q = y / period, rem = y % period;
  int in = rem - part * stripe;
  in = in < 0 ? 0 : (in > stripe ? stripe : in);
  return q * stripe + in;
}

int rm_fb_create_striped(rm_ctx* ctx, int width, int height, int stripe_rows, int parts, int part, void* color,
                         void* normal_dof, void* albedo_depth, rm_fb** out) {
  return rm_fb_create_striped_fmt(ctx, width, height, stripe_rows, parts, part, color, normal_dof, albedo_depth, RM_GBUFFER_F32, out);
}

int rm_fb_create_striped_fmt(rm_ctx* ctx, int width, int height, int stripe_rows, int parts, int part, void* color,
                             void* normal_dof, void* albedo_depth, int gbuffer, rm_fb** out) {
  if (!ctx || !out) return fail(ctx, RM_ERR_INVALID, "rm_fb_create_striped: NULL argument");
  *out = nullptr;
  if (gbuffer & RM_FB_MOMENTS) return fail(ctx, RM_ERR_INVALID, "rm_fb_create_striped: RM_FB_MOMENTS needs a framebuffer holding the whole frame (rm_fb_create_fmt)");
  if (int rc = gbuffer_check(ctx, gbuffer, "rm_fb_create_striped")) return rc;
  if (int rc = fb_check(ctx, width, height, 0, 1)) return rc;
  if (stripe_rows < 1 || parts < 1 || part < 0 || part >= parts) return fail(ctx, RM_ERR_INVALID, "rm_fb_create_striped: need stripe_rows >= 1 and 0 <= part < parts");
  if ((normal_dof == nullptr) != (albedo_depth == nullptr) || (!color && normal_dof)) return fail(ctx, RM_ERR_INVALID, "rm_fb_create_striped: give all planes, colour only, or none");
  if (!planes_aligned(color, normal_dof, albedo_depth, gbuffer))
    return fail(ctx, RM_ERR_INVALID, "rm_fb_create_striped: planes must be aligned to their pixel (16 bytes; 8 for half G-buffer planes)");
  const int rows = striped_rows_below(height, stripe_rows, parts, part);
  if (rows < 1) return fail(ctx, RM_ERR_INVALID, "rm_fb_create_striped: this part holds no rows");
  void* const planes[3] = {color, normal_dof, albedo_depth};
  return fb_make(ctx, "rm_fb_create_striped", FbGeometry{width, height, 0, rows, stripe_rows, parts, part}, gbuffer, color ? planes : nullptr, false, out);
}

int rm_fb_rows(const rm_fb* fb) { return fb ? fb->row_count : 0; }
int rm_fb_width(const rm_fb* fb) { return fb ? fb->width : 0; }
int rm_fb_height(const rm_fb* fb) { return fb ? fb->height : 0; }

int rm_fb_wrap(rm_ctx* ctx, int width, int height, int row_begin, int row_count, void* color, void* normal_dof,
               void* albedo_depth, rm_fb** out) {
  return rm_fb_wrap_fmt(ctx, width, height, row_begin, row_count, color, normal_dof, albedo_depth, RM_GBUFFER_F32, out);
}

int rm_fb_wrap_fmt(rm_ctx* ctx, int width, int height, int row_begin, int row_count, void* color, void* normal_dof,
                   void* albedo_depth, int gbuffer, rm_fb** out) {
  if (!ctx || !out || !color) return fail(ctx, RM_ERR_INVALID, "rm_fb_wrap: NULL argument");
  *out = nullptr;
  if (gbuffer & RM_FB_MOMENTS) return fail(ctx, RM_ERR_INVALID, "rm_fb_wrap: RM_FB_MOMENTS is for owned framebuffers (rm_fb_create_fmt)");
  if (int rc = gbuffer_check(ctx, gbuffer, "rm_fb_wrap")) return rc;
  if (int rc = fb_check(ctx, width, height, row_begin, row_count)) return rc;
  if ((normal_dof == nullptr) != (albedo_depth == nullptr)) return fail(ctx, RM_ERR_INVALID, "rm_fb_wrap: give both G-buffer planes or neither");
  if (!planes_aligned(color, normal_dof, albedo_depth, gbuffer))
    return fail(ctx, RM_ERR_INVALID, "rm_fb_wrap: planes must be aligned to their pixel (16 bytes; 8 for half G-buffer planes)");
  void* const planes[3] = {color, normal_dof, albedo_depth};
  return fb_make(ctx, "rm_fb_wrap", FbGeometry{width, height, row_begin, row_count}, gbuffer, planes, false, out);
}

int rm_fb_gbuffer(const rm_fb* fb) { return fb ? fb->gbuffer : RM_GBUFFER_F32; }
int rm_fb_has_moments(const rm_fb* fb) { return fb && fb->moments ? 1 : 0; }

int rm_fb_clear(rm_fb* fb) {
  if (!fb) return RM_ERR_INVALID;
  rm_ctx* ctx = fb->ctx;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i <= RM_PLANE_MOMENTS; i++)
    if (void* p = plane_ptr(fb, i)) RM_HIP(ctx, hipMemsetAsync(p, 0, plane_bytes(fb, i), ctx->stream));
  return RM_OK;
}

void rm_fb_destroy(rm_fb* fb) {
  if (!fb) return;
  (void)hipSetDevice(fb->ctx->device);
  (void)hipStreamSynchronize(fb->ctx->stream);
  fb_release(fb);
}

// The one copy between host memory and the context's device: `bytes` on the context's stream, and back once they have arrived.
static int copy_and_wait(rm_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

// a half plane through fp32 on the device (rm_narrow / rm_widen, the render kernels' own helpers): a scratch plane of float4,
// made per call -- kept with the context it would hold 16 bytes per pixel for a conversion a live loop never asks for
static int convert_half_plane(rm_fb* fb, int plane, void* host, bool upload) {
  rm_ctx* ctx = fb->ctx;
  const long long pixels = (long long)fb->width * (long long)fb->row_count;
  const size_t bytes = sizeof(float4) * (size_t)pixels;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  void* tmp = nullptr;
  RM_HIP(ctx, hipMalloc(&tmp, bytes));
  hipError_t e;
  if (upload) {
    e = hipMemcpyAsync(tmp, host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = rm::launch_convert(tmp, fb->plane[plane], pixels, true, ctx->stream);
  } else {
    e = rm::launch_convert(fb->plane[plane], tmp, pixels, false, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(host, tmp, bytes, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t s = hipStreamSynchronize(ctx->stream);
  (void)hipFree(tmp);
  RM_HIP(ctx, e);
  RM_HIP(ctx, s);
  return RM_OK;
}

// the float entries: planes 0..2 as fp32 whatever the framebuffer stores
static int float_plane_check(rm_fb* fb, int plane, const float* host, const char* what) {
  if (!fb || !host || plane < 0 || plane > 2) return fb ? fail(fb->ctx, RM_ERR_INVALID, std::string(what) + ": bad argument") : RM_ERR_INVALID;
  if (!fb->plane[plane]) return fail(fb->ctx, RM_ERR_INVALID, std::string(what) + ": this framebuffer has no such plane");
  return RM_OK;
}

int rm_fb_download(rm_fb* fb, int plane, float* host) {
  if (int rc = float_plane_check(fb, plane, host, "rm_fb_download")) return rc;
  if (plane_px_bytes(fb->gbuffer, plane) != sizeof(float4)) return convert_half_plane(fb, plane, host, false);
  return copy_and_wait(fb->ctx, host, fb->plane[plane], plane_bytes(fb, plane), hipMemcpyDeviceToHost);
}

int rm_fb_upload(rm_fb* fb, int plane, const float* host) {
  if (int rc = float_plane_check(fb, plane, host, "rm_fb_upload")) return rc;
  if (plane_px_bytes(fb->gbuffer, plane) != sizeof(float4)) return convert_half_plane(fb, plane, const_cast<float*>(host), true);
  return copy_and_wait(fb->ctx, fb->plane[plane], host, plane_bytes(fb, plane), hipMemcpyHostToDevice);
}

static int raw_check(rm_fb* fb, int plane, const void* host, size_t bytes, const char* what) {
  if (!fb || !host || plane < 0 || plane > 3) return fb ? fail(fb->ctx, RM_ERR_INVALID, std::string(what) + ": bad argument") : RM_ERR_INVALID;
  if (!plane_ptr(fb, plane)) return fail(fb->ctx, RM_ERR_INVALID, std::string(what) + ": this framebuffer has no such plane");
  if (bytes != plane_bytes(fb, plane)) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "%s: plane %d holds %zu bytes (%d x %d pixels of %zu bytes), not %zu", what, plane, plane_bytes(fb, plane), fb->row_count,
                  fb->width, plane_px_bytes(fb->gbuffer, plane), bytes);
    return fail(fb->ctx, RM_ERR_INVALID, buf);
  }
  return RM_OK;
}

int rm_fb_download_raw(rm_fb* fb, int plane, void* host, size_t bytes) {
  if (int rc = raw_check(fb, plane, host, bytes, "rm_fb_download_raw")) return rc;
  return copy_and_wait(fb->ctx, host, plane_ptr(fb, plane), bytes, hipMemcpyDeviceToHost);
}

int rm_fb_upload_raw(rm_fb* fb, int plane, const void* host, size_t bytes) {
  if (int rc = raw_check(fb, plane, host, bytes, "rm_fb_upload_raw")) return rc;
  return copy_and_wait(fb->ctx, plane_ptr(fb, plane), host, bytes, hipMemcpyHostToDevice);
}

void* rm_fb_device_ptr(rm_fb* fb, int plane) { return (fb && plane >= 0 && plane <= 3) ? plane_ptr(fb, plane) : nullptr; }

// ---- raw device memory for hosts without an allocator of their own ---------------------

int rm_buffer_create(rm_ctx* ctx, size_t bytes, void** device_ptr) {
  if (!ctx || !device_ptr || bytes == 0 || bytes > ((size_t)1 << 36)) return fail(ctx, RM_ERR_INVALID, "rm_buffer_create: NULL argument or a size outside 1 .. 2^36 bytes");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return fail(ctx, RM_ERR_DEVICE, "rm_buffer_create: out of device memory");
  hipError_t e = hipMemsetAsync(p, 0, bytes, ctx->stream);
  if (e != hipSuccess) { (void)hipFree(p); return fail(ctx, RM_ERR_DEVICE, std::string("rm_buffer_create: ") + hipGetErrorString(e)); }
  ctx->buffers[p] = bytes;
  *device_ptr = p;
  return RM_OK;
}

int rm_buffer_destroy(rm_ctx* ctx, void* device_ptr) {
  if (!ctx) return RM_ERR_INVALID;
  if (!device_ptr) return RM_OK;
  auto it = ctx->buffers.find(device_ptr);
  if (it == ctx->buffers.end()) return fail(ctx, RM_ERR_INVALID, "rm_buffer_destroy: not a buffer of this context");
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->buffers.erase(it);
  RM_HIP(ctx, hipFree(device_ptr));
  return RM_OK;
}

// the copies take the buffer's base address and at most its size
static int buffer_check(rm_ctx* ctx, const void* device_ptr, const void* host, size_t bytes, const char* what) {
  if (!ctx || !device_ptr || !host) return fail(ctx, RM_ERR_INVALID, std::string(what) + ": NULL argument");
  auto it = ctx->buffers.find(const_cast<void*>(device_ptr));
  if (it == ctx->buffers.end()) return fail(ctx, RM_ERR_INVALID, std::string(what) + ": not a buffer of this context");
  if (bytes > it->second) return fail(ctx, RM_ERR_INVALID, std::string(what) + ": more bytes than the buffer holds");
  return RM_OK;
}

int rm_buffer_download(rm_ctx* ctx, const void* device_ptr, void* host, size_t bytes) {
  if (int rc = buffer_check(ctx, device_ptr, host, bytes, "rm_buffer_download")) return rc;
  return copy_and_wait(ctx, host, device_ptr, bytes, hipMemcpyDeviceToHost);
}

int rm_buffer_upload(rm_ctx* ctx, void* device_ptr, const void* host, size_t bytes) {
  if (int rc = buffer_check(ctx, device_ptr, host, bytes, "rm_buffer_upload")) return rc;
  return copy_and_wait(ctx, device_ptr, host, bytes, hipMemcpyHostToDevice);
}

// The culling grid of a scene that has one coming (rm_scene_create), before a call that reads it (either build; not the GL stack's
// arithmetic).  Round 5: built once the scene has been asked for ctx->cull_min_pixels pixel-samples (until then it renders without
// one: the same bits, and a host that shows a new scene every frame at a small size never pays for a grid it would not earn back);
// the build kernel is enqueued on a stream of its own, the render that triggered it waits for it on the device -- no wait on the host -- into a
// buffer recycled from the context's pool; the grids of a context stay within its budget, the least recently used scene giving its
// grid up first.  Running out of memory is not an error (the fold of every row gives the same bits); any other failure is.
// The pool: buffers of grids that were given up, kept for the next build of the same size (a host that shows a new scene in every frame
// builds a grid per frame: no hipMalloc / hipFree each time).  At most 4 buffers and half the budget, and -- since round 6 -- the
// pooled bytes COUNT against the budget: grids held + buffers pooled <= rm_ctx_set_cull_budget at every moment (cull_trim_pool).
static size_t cull_pooled_bytes(const rm_ctx* ctx) {
  size_t pooled = 0;
  for (auto& b : ctx->cull_pool) pooled += b.bytes;
  return pooled;
}
static void cull_trim_pool(rm_ctx* ctx, size_t room_for) {  // frees pooled buffers until grids + pool + room_for fit the budget
  while (!ctx->cull_pool.empty() && ctx->cull_bytes + cull_pooled_bytes(ctx) + room_for > ctx->cull_budget) {
    (void)hipFree(ctx->cull_pool.back().p);  // (waits for the device)
    ctx->cull_pool.pop_back();
  }
}
static void cull_release(rm_ctx* ctx, rm_scene* s, bool idle) {  // the scene's grid back to the pool; idle: the caller has waited for the renders that read it
  if (!s->d_cull) return;
  const size_t pooled = cull_pooled_bytes(ctx);
  if (ctx->cull_pool.size() < 4 && pooled + s->cull_bytes <= ctx->cull_budget / 2) ctx->cull_pool.push_back({s->d_cull, s->cull_bytes, idle});
  else (void)hipFree(s->d_cull);  // (waits for the device)
  ctx->cull_bytes -= s->cull_bytes;
  for (size_t i = 0; i < ctx->cull_scenes.size(); i++)
    if (ctx->cull_scenes[i] == s) { ctx->cull_scenes.erase(ctx->cull_scenes.begin() + (long)i); break; }
  s->d_cull = nullptr;
  s->cull_bytes = 0;
  s->dev.cull.cells = nullptr;
}

static int scene_cull_grid(rm_ctx* ctx, rm_scene* s, int flags, long long pixels) {
  s->last_use = ++ctx->use_clock;
  if (!s->cull_wanted || (flags & RM_RENDER_NO_CULL) || (ctx->gl_stack && !(flags & RM_RENDER_FAST))) return RM_OK;
  s->px_seen += pixels;
  if (s->px_seen < ctx->cull_min_pixels) return RM_OK;
  CullGrid g = s->cull_grid;
  CullBuild build = s->cull_build;
  const size_t bytes = (size_t)(rm_cull_cells(g.n, g.n_outer, g.levels) + 1) * (size_t)g.words * sizeof(unsigned long long);
  if (bytes > ctx->cull_budget) return RM_OK;  // (still wanted: a host may raise the budget -- rm_ctx_set_cull_budget -- and the next render builds it)
  s->cull_wanted = false;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  while (ctx->cull_bytes + bytes > ctx->cull_budget && !ctx->cull_scenes.empty()) {  // the least recently used grid goes (a kernel still
    rm_scene* victim = ctx->cull_scenes[0];                                            // reading it is ahead of the next build on this stream)
    for (rm_scene* c : ctx->cull_scenes)
      if (c->last_use < victim->last_use) victim = c;
    cull_release(ctx, victim, false);
    victim->cull_wanted = true;  // ... and may earn it back
    victim->px_seen = 0;
  }
  unsigned long long* cells = nullptr;
  bool idle = true;
  for (size_t i = 0; i < ctx->cull_pool.size(); i++)
    if (ctx->cull_pool[i].bytes == bytes) { cells = ctx->cull_pool[i].p; idle = ctx->cull_pool[i].idle; ctx->cull_pool.erase(ctx->cull_pool.begin() + (long)i); break; }
  if (!cells) {
    cull_trim_pool(ctx, bytes);  // the pooled buffers count against the budget too
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&cells), bytes);
    if (e == hipErrorOutOfMemory) {  // give the pool back and try once more
      (void)hipGetLastError();
      for (auto& b : ctx->cull_pool) (void)hipFree(b.p);
      ctx->cull_pool.clear();
      e = hipMalloc(reinterpret_cast<void**>(&cells), bytes);
    }
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return RM_OK; }
    if (e != hipSuccess) return fail(ctx, RM_ERR_DEVICE, std::string("culling grid: ") + hipGetErrorString(e));
  }
  build.prims = s->d_prims;
  build.cells = cells;
  hipError_t e = hipSuccess;
  if (!ctx->cull_stream) e = hipStreamCreateWithFlags(&ctx->cull_stream, hipStreamNonBlocking);
  if (e == hipSuccess && !ctx->cull_event) e = hipEventCreateWithFlags(&ctx->cull_event, hipEventDisableTiming);
  if (e == hipSuccess && !ctx->cull_order) e = hipEventCreateWithFlags(&ctx->cull_order, hipEventDisableTiming);
  if (e == hipSuccess && !idle) {  // a grid given up for the budget's sake: renders enqueued before now may still read it -- every one of them is
    e = hipEventRecord(ctx->cull_order, ctx->stream);  // followed by its blend on the context's stream, so behind this point they are done
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->cull_stream, ctx->cull_order, 0);
  }
  if (e == hipSuccess) e = rm::launch_cull_build(build, ctx->cull_stream);
  if (e == hipSuccess) e = hipEventRecord(ctx->cull_event, ctx->cull_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->cull_event, 0);  // what runs on the context's own stream; the side streams wait where they launch
  if (e != hipSuccess) {
    (void)hipFree(cells);
    return fail(ctx, RM_ERR_DEVICE, std::string("culling grid: ") + hipGetErrorString(e));
  }
  s->d_cull = cells;
  s->cull_bytes = bytes;
  g.cells = cells;
  s->dev.cull = g;
  ctx->cull_bytes += bytes;
  ctx->cull_built++;
  ctx->cull_scenes.push_back(s);
  return RM_OK;
}

// The scene block a pass gets for its flags (behind scene_cull_grid, where the pass obtains the grid): the scene's own, without the culling
// grid's cells under RM_RENDER_NO_CULL.
static DevScene scene_view(const rm_scene* scene, int flags) {
  DevScene view = scene->dev;
  if (flags & RM_RENDER_NO_CULL) view.cull.cells = nullptr;
  return view;
}

int rm_ctx_set_cull_min_pixels(rm_ctx* ctx, long long pixels) {
  if (!ctx) return RM_ERR_INVALID;
  if (pixels < 0) return fail(ctx, RM_ERR_INVALID, "rm_ctx_set_cull_min_pixels: pixels must be >= 0");
  ctx->cull_min_pixels = pixels;
  return RM_OK;
}

int rm_ctx_set_cull_budget(rm_ctx* ctx, size_t bytes) {
  if (!ctx) return RM_ERR_INVALID;
  ctx->cull_budget = bytes;
  // a lowered budget takes effect now: the least recently rendered scenes give their grids up (and may earn them back), then the pool shrinks
  RM_HIP(ctx, hipSetDevice(ctx->device));
  while (ctx->cull_bytes > ctx->cull_budget && !ctx->cull_scenes.empty()) {
    rm_scene* victim = ctx->cull_scenes[0];
    for (rm_scene* c : ctx->cull_scenes)
      if (c->last_use < victim->last_use) victim = c;
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (renders that read the grid are followed by their blend on this stream)
    RM_HIP(ctx, ctx->sp.sync_all());
    cull_release(ctx, victim, true);
    victim->cull_wanted = true;
    victim->px_seen = 0;
  }
  cull_trim_pool(ctx, 0);
  return RM_OK;
}

int rm_ctx_cull_stats(const rm_ctx* ctx, unsigned long long* out4) {
  if (!ctx || !out4) return RM_ERR_INVALID;
  out4[0] = ctx->cull_built;
  out4[1] = (unsigned long long)ctx->cull_bytes;  // (the grids scenes hold; recycled buffers waiting in the pool are extra, and within the budget with them)
  out4[2] = (unsigned long long)ctx->cull_scenes.size();
  out4[3] = (unsigned long long)ctx->cull_budget;
  return RM_OK;
}

// ---- the hot path ---------------------------------------------------------------

// what one sample of a tw x th tile asks of the scene, in pixel-samples of the JOB: a striped framebuffer holds one part of `parts` of the frame, and
// the other ranks render the rest of it (each with a grid of its own to earn: the threshold is the same for a sharded job as for a whole one)
static long long job_pixel_samples(const rm_fb* fb, int tw, int th) { return (long long)tw * (long long)th * (fb->stripe_rows > 0 ? (long long)fb->parts : 1ll); }

static int build_params(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* u, const RmRect* tile, int flags,
                        KParams* P, bool* empty) {
  if (!ctx || !scene || !fb || !u) return fail(ctx, RM_ERR_INVALID, "render: NULL argument");
  if (scene->ctx != ctx || fb->ctx != ctx) return fail(ctx, RM_ERR_INVALID, "render: scene/framebuffer belong to another context");
  if (u->renderMode != 0 && u->renderMode != 1) return fail(ctx, RM_ERR_INVALID, "render: renderMode must be 0 (full) or 1 (preview)");
  if (!RM_WITH_WAVEFRONT && (flags & RM_RENDER_WAVEFRONT))
    return fail(ctx, RM_ERR_INVALID, "render: RM_RENDER_WAVEFRONT -- this library is built without the wavefront pipeline (it is the tests' second implementation: "
                                     "tests/_xcheck/libhip_raymarch_xcheck.so); the product's own cross-check is RM_RENDER_NO_FAR_JUMP | RM_RENDER_NO_CULL");
  if (!(u->reflections >= 0.0f && u->reflections <= (float)RM_MAX_BOUNCES)) return fail(ctx, RM_ERR_INVALID, "render: reflections must be in 0..10 (raymarchingStepCountsArray[10])");
  if (u->lightCount < 0 || u->lightCount > RM_MAX_LIGHTS) return fail(ctx, RM_ERR_INVALID, "render: lightCount must be in 0..10");
  // `for (float i = 0.; i < steps; i++)` (raymarcher.frag:165, :210) never ends once i stops growing at 2^24
  for (int b = 0; b < RM_MAX_BOUNCES; b++)
    if (u->raymarchingStepCountsArray[b] > 1048576.0f) return fail(ctx, RM_ERR_INVALID, "render: a step count above 2^20");
  const bool color_only = (flags & RM_RENDER_COLOR_ONLY) != 0;
  if (!color_only && u->renderMode == 0 && (!fb->plane[1] || !fb->plane[2]))
    return fail(ctx, RM_ERR_INVALID, "render: framebuffer has no G-buffer planes; pass RM_RENDER_COLOR_ONLY");
  RmRect t = tile ? *tile : RmRect{0, 0, fb->width, fb->height};
  // clip to the image, then to the rows this framebuffer holds (as LOCAL row indices)
  const int x0 = t.x < 0 ? 0 : t.x, x1 = t.x + t.w > fb->width ? fb->width : t.x + t.w;
  int y0 = t.y < 0 ? 0 : t.y, y1 = t.y + t.h > fb->height ? fb->height : t.y + t.h;
  if (y1 < y0) y1 = y0;
  int l0, l1;
  if (fb->stripe_rows > 0) {
    l0 = striped_rows_below(y0, fb->stripe_rows, fb->parts, fb->part);
    l1 = striped_rows_below(y1, fb->stripe_rows, fb->parts, fb->part);
  } else {
    l0 = (y0 < fb->row_begin ? fb->row_begin : y0) - fb->row_begin;
    l1 = (y1 > fb->row_begin + fb->row_count ? fb->row_begin + fb->row_count : y1) - fb->row_begin;
  }
  *empty = x1 <= x0 || l1 <= l0;
  if (int rc = scene_cull_grid(ctx, scene, flags, *empty ? 0ll : job_pixel_samples(fb, x1 - x0, l1 - l0))) return rc;
  P->u = *u;
  P->scene = scene_view(scene, flags);
  P->color = fb->plane[0];
  P->normal_dof = color_only ? nullptr : fb->plane[1];
  P->albedo_depth = color_only ? nullptr : fb->plane[2];
  P->W = fb->width; P->H = fb->height; P->row_begin = fb->row_begin;
  P->stripe_rows = fb->stripe_rows; P->parts = fb->parts; P->part = fb->part;
  P->tx = x0; P->ty = l0; P->tw = x1 - x0; P->th = l1 - l0;
  P->retire_eps = (flags & RM_RENDER_FAST) ? ctx->retire_eps : 0.0f;
  P->stage = nullptr;
  P->stage_stride = 0;
  P->batch = 0;
  P->tile_wide = 0;
  std::memset(P->batch_noise, 0, sizeof P->batch_noise);
  P->block_order = nullptr;
  P->block_cost = nullptr;
  P->no_far_jump = (flags & RM_RENDER_NO_FAR_JUMP) ? 1 : 0;
  P->gbuffer_half = fb->gbuffer == RM_GBUFFER_F16 ? 1 : 0;
  P->moments = color_only ? nullptr : fb->moments;  // blended by rm_combine_kernel, so only behind a staged launch (launch)
  if (P->no_far_jump) P->scene.far_end = 0, P->scene.clear_rho = 0.0f;  // the far-field shortcuts inside an evaluation (KIFS tree) read the scene block
  return RM_OK;
}

#define RM_BATCH_TARGET_TILES 16384ll  // workgroups a batch launch of rm_render_samples aims for

// The implementation a render call uses (same results either way).  The pixel kernel is the faster one for every measured job in
// both builds, so the wavefront pipeline (rm_wavefront.inc, launched by rm_wavefront_host.inc) runs only where a caller of the tests'
// cross-check build asks for it.  The GL-stack arithmetic exists as the pixel kernel only, and so do
// position-dependent materials (RM_TABLE_HAS_SURFACES): the pipeline's stages carry one material block per scene -- its light
// stage has no scene table staged -- so such scenes render with the pixel kernel whatever the flags ask for (same results).
static bool uses_wavefront(const rm_ctx* ctx, const KParams& P, int flags) {
  if (!RM_WITH_WAVEFRONT) return false;  // the product library (build_params refuses the flag)
  if (ctx->gl_stack && !(flags & RM_RENDER_FAST)) return false;
  if (P.scene.table_flags & (RM_TABLE_HAS_SURFACES | RM_TABLE_HAS_KIND)) return false;
  if (P.gbuffer_half || P.moments) return false;  // the half G-buffer and the moments are blended by rm_combine_kernel behind the staged pixel kernel only
  return (flags & RM_RENDER_WAVEFRONT) != 0;
}

// Whether a job's samples are staged (launch_pixels_in_flight), and over how many slots.
struct Staging { enum Rule { NEVER, MAY, MUST } rule; int depth; };
static Staging staging_rule(const rm_ctx* ctx, const KParams& P, int flags) {
  // full mode with at least one bounce: the kernel's only use of the planes is the final blend, which can be split off
  if (uses_wavefront(ctx, P, flags) || !(P.u.renderMode == 0 && P.u.reflections > 0.0f)) return {Staging::NEVER, 0};
  const bool overlap = !(flags & RM_RENDER_NO_OVERLAP);
  // The half G-buffer (RM_GBUFFER_F16) is blended by rm_combine_kernel only -- the pixel kernel's own blend is the fp32 one, left
  // exactly as it was -- so a render that writes the G-buffer (the planes asked for: raymarcher.frag:347-351 runs at bounce 0) is
  // always staged; with RM_RENDER_NO_OVERLAP on one staging slot, so that a sample's render waits for the previous sample's blend.
  // No unstaged fallback: without room for the staging of the tile the call fails (render in tiles).
  // The moments plane (RM_FB_MOMENTS) is written by rm_combine_kernel only too, under the same rule.
  if ((P.gbuffer_half || P.moments != nullptr) && P.normal_dof != nullptr) return {Staging::MUST, overlap ? ctx->sp.depth : 1};
  // Otherwise staging is there for the overlap: a launch that finds no room for it renders unstaged (same bits).  On ONE slot a
  // single sample gains nothing from it and launch() leaves it unstaged; a batch of rm_render_samples still saves its launches.
  return {overlap ? Staging::MAY : Staging::NEVER, ctx->sp.depth};
}

// Staging the library may hold for a job: a quarter of what the device has free (counting what staging already holds).
// rm_render_samples sizes its automatic batch by it, and a launch whose staging cannot be allocated at all renders
// unstaged, one sample at a time on the context's stream, instead of failing (launch / rm_render_samples).
static size_t staging_budget(rm_ctx* ctx) {
  if (const char* v = std::getenv("RM_STAGING_BUDGET_MB")) {  // a fixed budget (tests; hosts that share the device with other allocators)
    const long long mb = std::atoll(v);
    if (mb >= 0) return (size_t)mb << 20;
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (size_t)1 << 30;
  return (free_b + ctx->sp.held_bytes()) / 4;
}

// the pixel kernel in the build the flags and the context ask for
static hipError_t launch_pixel_kernel(const rm_ctx* ctx, const KParams& P, int flags, hipStream_t stream) {
  return RM_SCENE_PASS(ctx, flags, launch_pixels, P, stream);
}

// Cost order on a sample-in-flight slot: the costs are sorted on the slot's own stream right AFTER the render (sort_slot_costs, called once the render's
// completion event is recorded), so the sort's two small launches sit in the shadow of the other slots' renders instead of in front of this slot's next one
static hipError_t launch_ordered_on_slot(rm_ctx* ctx, Lpt& L, KParams Q, int flags, hipStream_t stream, long long tiles) {
  hipError_t e;
  Q.block_cost = L.cost[0];
  if (L.have_cost) Q.block_order = L.order[0];
  else if ((e = hipMemsetAsync(L.cost[0], 0, sizeof(unsigned int) * (size_t)tiles, stream)) != hipSuccess) return e;
  L.have_cost = true;
  L.to_sort = (int)tiles;
  return launch_pixel_kernel(ctx, Q, flags, stream);
}

static hipError_t sort_slot_costs(rm_ctx* ctx, int slot, hipStream_t stream) {
  Lpt& L = ctx->lpt[slot];
  return L.to_sort > 0 ? rm::launch_order(L.cost[0], L.order[0], L.order[0] + L.capacity, L.to_sort, stream) : hipSuccess;
}

// Cost order on the context's own stream: the sort runs on lpt_stream, one sample behind (see Lpt)
static hipError_t launch_ordered_on_own_stream(rm_ctx* ctx, Lpt& L, KParams Q, int flags, long long tiles) {
  hipError_t e;
  hipStream_t stream = ctx->stream;
  if (!ctx->lpt_stream && (e = hipStreamCreateWithFlags(&ctx->lpt_stream, hipStreamNonBlocking)) != hipSuccess) return e;
  for (int k = 0; k < 2; k++) {
    if (!L.rendered[k] && (e = hipEventCreateWithFlags(&L.rendered[k], hipEventDisableTiming)) != hipSuccess) return e;
    if (!L.sorted[k] && (e = hipEventCreateWithFlags(&L.sorted[k], hipEventDisableTiming)) != hipSuccess) return e;
  }
  if (!L.have_cost) {  // a new job: both cost buffers start from zero, no order yet
    if ((e = hipStreamSynchronize(ctx->lpt_stream)) != hipSuccess) return e;  // sorts of the previous job still use the buffers
    if ((e = hipMemsetAsync(L.cost[0], 0, sizeof(unsigned int) * (size_t)tiles, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(L.cost[1], 0, sizeof(unsigned int) * (size_t)tiles, stream)) != hipSuccess) return e;
    L.launches = 0;
    L.have_cost = true;
  }
  const int cur = (int)(L.launches & 1ull);
  unsigned int* cost_cur = L.cost[cur];
  unsigned int* order_cur = L.order[cur];
  // launch n writes its costs into buffer n % 2 (zeroed by the sort of launch n - 2, which launch n therefore waits
  // for -- it ran during launch n - 1) and starts in the order that sort left in the same buffer's order array
  if (L.launches >= 2) {
    if ((e = hipStreamWaitEvent(stream, L.sorted[cur], 0)) != hipSuccess) return e;
    Q.block_order = order_cur;
  }
  Q.block_cost = cost_cur;
  if ((e = launch_pixel_kernel(ctx, Q, flags, stream)) != hipSuccess) return e;
  if ((e = hipEventRecord(L.rendered[cur], stream)) != hipSuccess) return e;
  if ((e = hipStreamWaitEvent(ctx->lpt_stream, L.rendered[cur], 0)) != hipSuccess) return e;
  if ((e = rm::launch_order(cost_cur, order_cur, order_cur + L.capacity, (int)tiles, ctx->lpt_stream)) != hipSuccess) return e;  // sorts and zeroes the costs
  if ((e = hipEventRecord(L.sorted[cur], ctx->lpt_stream)) != hipSuccess) return e;
  L.launches++;
  return hipSuccess;
}

// The pixel kernel on `stream`, its tiles in the order of their cost in the previous launch of the same job on that stream
// (slot = which of the context's streams: a sample-in-flight slot, or RM_SP_MAX for the context's own stream).
static hipError_t launch_pixels_ordered(rm_ctx* ctx, const KParams& P, int flags, hipStream_t stream, int slot) {
  int gx = 0, gy = 0;
  rm::pixel_grid(P, &gx, &gy);
  const long long tiles = (long long)gx * gy;
  if (!ctx->lpt_enabled || tiles < 512 || tiles > (1ll << 22))  // small jobs end on launch latency, not on a tail
    return launch_pixel_kernel(ctx, P, flags, stream);
  Lpt& L = ctx->lpt[slot];
  const long long key[8] = {P.W, P.H, ((long long)P.tx << 32) | (unsigned int)P.ty, ((long long)P.tw << 32) | (unsigned int)P.th,
                            ((long long)P.stripe_rows << 40) | ((long long)P.parts << 20) | P.part, P.row_begin,
                            ((long long)P.scene.kind << 8) | P.u.renderMode, tiles};
  const bool own_stream = slot == RM_SP_MAX;
  if (hipError_t e = L.grow(tiles, own_stream ? 2 : 1, stream, ctx->lpt_stream)) return e;
  if (std::memcmp(key, L.key, sizeof key) != 0) {
    std::memcpy(L.key, key, sizeof key);
    L.forget();
  }
  return own_stream ? launch_ordered_on_own_stream(ctx, L, P, flags, tiles) : launch_ordered_on_slot(ctx, L, P, flags, stream, tiles);
}

// The pixel kernel of one sample -- or of a batch of `batch` samples, randNoise pairs in `noise` -- on a side stream,
// staged, and its blend on the context's stream (see SamplesInFlight).
// depth: staging slots to rotate through (1 = a sample's render waits for the previous blend)
static hipError_t launch_pixels_in_flight(rm_ctx* ctx, const KParams& P, int flags, int depth, int batch = 1, const float* noise = nullptr) {
  hipError_t e;
  SamplesInFlight& S = ctx->sp;
  if ((e = S.ensure_slots(depth)) != hipSuccess) return e;
  // A slot's staging holds the launch's TILE, compact (tile pixel i of sample k at k * 3 * stride + i), so it is sized by the
  // largest batch x tile a job has used -- not by the frame: a subdivided 8192^2 render stages a tile, not 3.2 GB x batch.
  const size_t tile_px = (size_t)P.tw * (size_t)P.th;
  int slot = 0;
  if ((e = S.reserve(3 * tile_px * (size_t)batch, depth, &slot)) != hipSuccess) return e;
  KParams Q = P;
  Q.stage = S.stage[slot];
  Q.stage_stride = (long long)tile_px;
  if (batch > 1) {
    Q.batch = batch;
    std::memcpy(Q.batch_noise, noise, sizeof(float) * 2 * (size_t)batch);
  }
  hipStream_t side = S.stream[slot];
  // the render reads no plane: it only has to wait until the blend that last used this staging buffer is done
  if ((e = hipStreamWaitEvent(side, S.free[slot], 0)) != hipSuccess) return e;
  if (ctx->cull_event && (e = hipStreamWaitEvent(side, ctx->cull_event, 0)) != hipSuccess) return e;  // ... and for the scene's culling grid, built on the context's cull_stream (scene_cull_grid records cull_event behind the build)
  ctx->lpt[slot].to_sort = 0;
  if ((e = launch_pixels_ordered(ctx, Q, flags, side, slot)) != hipSuccess) return e;
  if ((e = hipEventRecord(S.done[slot], side)) != hipSuccess) return e;
  if ((e = sort_slot_costs(ctx, slot, side)) != hipSuccess) return e;  // behind the completion event
  if ((e = hipStreamWaitEvent(ctx->stream, S.done[slot], 0)) != hipSuccess) return e;
  if ((e = rm::launch_combine(Q, ctx->stream)) != hipSuccess) return e;
  return hipEventRecord(S.free[slot], ctx->stream);
}

static hipError_t launch(rm_ctx* ctx, const KParams& P, int flags) {
  const bool wavefront = uses_wavefront(ctx, P, flags);
  ctx->last_pipeline = wavefront ? RM_PIPELINE_WAVEFRONT : RM_PIPELINE_PIXEL_KERNEL;
#if RM_WITH_WAVEFRONT
  if (wavefront) return launch_wavefront(ctx->wf, P, flags, ctx->stream, &ctx->error);
#endif
  const Staging s = staging_rule(ctx, P, flags);
  if (s.rule == Staging::MUST) return launch_pixels_in_flight(ctx, P, flags, s.depth);
  if (s.rule == Staging::MAY && s.depth > 1) {
    const hipError_t e = launch_pixels_in_flight(ctx, P, flags, s.depth);
    if (e != hipErrorOutOfMemory) return e;
    (void)hipGetLastError();  // no room for the staging of this tile: render it unstaged (same bits, no overlap)
  }
  return launch_pixels_ordered(ctx, P, flags, ctx->stream, RM_SP_MAX);
}

int rm_render_sample(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* uniforms, const RmRect* tile, int flags) {
  KParams P;
  bool empty = false;
  if (int rc = build_params(ctx, scene, fb, uniforms, tile, flags, &P, &empty)) return rc;
  if (empty) return RM_OK;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, launch(ctx, P, flags));
  return RM_OK;
}

int rm_render_samples(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* uniforms, const float* rand_noise_pairs,
                      int count, const RmRect* tile, int flags) {
  KParams P;
  bool empty = false;
  if (int rc = build_params(ctx, scene, fb, uniforms, tile, flags, &P, &empty)) return rc;
  if (count < 0 || (count > 0 && !rand_noise_pairs)) return fail(ctx, RM_ERR_INVALID, "rm_render_samples: bad count / NULL randNoise");
  if (empty) return RM_OK;
  if (count > 1 && scene->cull_wanted)  // build_params counted one sample of the tile: the call asks for `count` (the grid, if this earns it, serves the next call)
    scene->px_seen += (long long)(count - 1) * job_pixel_samples(fb, P.tw, P.th);
  RM_HIP(ctx, hipSetDevice(ctx->device));
  // Samples that are staged with overlap go out in batches: one launch per batch.
  const Staging s = staging_rule(ctx, P, flags);
  int per_launch = 1;
  if (s.rule != Staging::NEVER && !(flags & RM_RENDER_NO_OVERLAP) && ctx->sample_batch != 1) {
    per_launch = ctx->sample_batch;
    if (per_launch == 0) {
      int gx = 0, gy = 0;
      rm::pixel_grid(P, &gx, &gy);
      const long long tiles = (long long)gx * gy;
      per_launch = tiles > 0 ? (int)((RM_BATCH_TARGET_TILES + tiles / 2) / tiles) : 1;  // to the nearest: a 1/8 shard of the headline frame has 2 160 tiles -> 8
    }
    per_launch = per_launch < 1 ? 1 : per_launch > RM_BATCH_MAX ? RM_BATCH_MAX : per_launch;
    // the staging of a batch is 48 bytes per tile pixel, sample of the batch and launch in flight: within the budget
    const size_t per_sample = sizeof(float4) * 3 * (size_t)P.tw * (size_t)P.th * (size_t)s.depth;
    const size_t fit = staging_budget(ctx) / (per_sample ? per_sample : 1);
    if ((size_t)per_launch > fit) per_launch = fit < 1 ? 1 : (int)fit;
  }
  ctx->last_pipeline = uses_wavefront(ctx, P, flags) ? RM_PIPELINE_WAVEFRONT : RM_PIPELINE_PIXEL_KERNEL;
  for (int i = 0; i < count;) {
    int n = count - i < per_launch ? count - i : per_launch;
    if (n > 1) {
      const hipError_t e = launch_pixels_in_flight(ctx, P, flags, s.depth, n, rand_noise_pairs + 2 * i);
      if (e == hipErrorOutOfMemory) {  // the batch's staging does not fit after all: one sample per launch from here on
        (void)hipGetLastError();
        per_launch = 1;
        continue;
      }
      RM_HIP(ctx, e);
    } else {
      P.u.randNoise[0] = rand_noise_pairs[2 * i];
      P.u.randNoise[1] = rand_noise_pairs[2 * i + 1];
      RM_HIP(ctx, launch(ctx, P, flags));
    }
    i += n;
  }
  return RM_OK;
}

int rm_ctx_set_sample_batch(rm_ctx* ctx, int n) {
  if (!ctx) return RM_ERR_INVALID;
  if (n < 0 || n > RM_BATCH_MAX) return fail(ctx, RM_ERR_INVALID, "rm_ctx_set_sample_batch: n must be 0 (automatic) or 1..8");
  ctx->sample_batch = n;
  return RM_OK;
}

int rm_render_timed(rm_ctx* ctx, rm_scene* scene, rm_fb* fb, const RmUniforms* uniforms, int count, const RmRect* tile,
                    int flags, float* ms_per_launch) {
  KParams P;
  bool empty = false;
  if (int rc = build_params(ctx, scene, fb, uniforms, tile, flags, &P, &empty)) return rc;
  if (count < 1 || !ms_per_launch) return fail(ctx, RM_ERR_INVALID, "rm_render_timed: bad count / NULL result");
  if (empty) return fail(ctx, RM_ERR_INVALID, "rm_render_timed: empty tile");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (int i = 0; i < count; i++) RM_HIP(ctx, launch(ctx, P, flags));
  RM_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  RM_HIP(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0.0f;
  RM_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ms_per_launch = ms / (float)count;
  return RM_OK;
}

// ---- assembling a sharded frame -------------------------------------------------------

int rm_assemble_striped_bytes(rm_ctx* ctx, const void* src, int parts, int max_rows, long long row_bytes, int height, int stripe_rows,
                              void* dst, void* hip_stream) {
  if (!ctx || !src || !dst) return fail(ctx, RM_ERR_INVALID, "rm_assemble_striped: NULL argument");
  if (parts < 1 || row_bytes < 4 || (row_bytes & 3) || row_bytes > (1ll << 24) || height < 1 || stripe_rows < 1)
    return fail(ctx, RM_ERR_INVALID, "rm_assemble_striped: parts, height and stripe_rows must be >= 1, row_bytes a multiple of 4");
  if (max_rows < striped_rows_below(height, stripe_rows, parts, 0))  // part 0 holds the most rows
    return fail(ctx, RM_ERR_INVALID, "rm_assemble_striped: max_rows is smaller than the largest part's window");
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) return fail(ctx, RM_ERR_INVALID, "rm_assemble_striped: buffers must be 16-byte aligned");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, rm::launch_assemble(src, parts, max_rows, row_bytes, height, stripe_rows, dst, hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream));
  return RM_OK;
}

int rm_assemble_striped(rm_ctx* ctx, const void* src, int parts, int max_rows, int width, int height, int stripe_rows, void* dst,
                        void* hip_stream) {
  if (width < 1) return fail(ctx, RM_ERR_INVALID, "rm_assemble_striped: width must be >= 1");
  return rm_assemble_striped_bytes(ctx, src, parts, max_rows, (long long)width * 16, height, stripe_rows, dst, hip_stream);
}

// ---- present ---------------------------------------------------------------------

// nd_half: normal_dof is a plane of rm_half4 (rm_present of a framebuffer with the half G-buffer); the raw-pointer entry points are fp32
static int present_device(rm_ctx* ctx, const void* color, const void* normal_dof, bool nd_half, int width, int height, int samples, void* out_rgba8_device,
                          void* hip_stream) {
  if (!ctx || !color || !out_rgba8_device) return fail(ctx, RM_ERR_INVALID, "rm_present_device: NULL argument");
  if (width < 1 || height < 1 || samples < 1) return fail(ctx, RM_ERR_INVALID, "rm_present_device: width, height and samples must be >= 1");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, (ctx->gl_stack ? rm_gl_launch_present : rm::launch_present)(static_cast<const float4*>(color), normal_dof, nd_half, width, height,
                                 1.0f / (float)samples, static_cast<uchar4*>(out_rgba8_device), hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream));
  return RM_OK;
}

int rm_present_device(rm_ctx* ctx, const void* color, const void* normal_dof, int width, int height, int samples, void* out_rgba8_device,
                      void* hip_stream) {
  return present_device(ctx, color, normal_dof, false, width, height, samples, out_rgba8_device, hip_stream);
}

int rm_present_rows(rm_ctx* ctx, rm_fb* fb, int samples, void* out_rgba8_device, void* hip_stream) {
  if (!ctx || !fb || !out_rgba8_device) return fail(ctx, RM_ERR_INVALID, "rm_present_rows: NULL argument");
  if (fb->ctx != ctx) return fail(ctx, RM_ERR_INVALID, "rm_present_rows: framebuffer belongs to another context");
  if (samples < 1) return fail(ctx, RM_ERR_INVALID, "rm_present_rows: samples must be >= 1");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, (ctx->gl_stack ? rm_gl_launch_present_rows : rm::launch_present_rows)(fb->plane[0], (long long)fb->width * (long long)fb->row_count, 1.0f / (float)samples,
                                      static_cast<uchar4*>(out_rgba8_device), hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream));
  return RM_OK;
}

int rm_pack_present_rows(rm_ctx* ctx, rm_fb* fb, void* out_float4_device, void* hip_stream) {
  if (!ctx || !fb || !out_float4_device) return fail(ctx, RM_ERR_INVALID, "rm_pack_present_rows: NULL argument");
  if (fb->ctx != ctx) return fail(ctx, RM_ERR_INVALID, "rm_pack_present_rows: framebuffer belongs to another context");
  if (reinterpret_cast<uintptr_t>(out_float4_device) & 15u) return fail(ctx, RM_ERR_INVALID, "rm_pack_present_rows: the buffer must be 16-byte aligned");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, rm::launch_pack_rows(fb->plane[0], fb->plane[1], fb->gbuffer == RM_GBUFFER_F16, (long long)fb->width * (long long)fb->row_count, static_cast<float4*>(out_float4_device),
                                   hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream));
  return RM_OK;
}

// Room for `bytes` in one of the context's buffers (its device has been selected), for work about to be enqueued on `stream`.  The
// rule, for all of them: with enough capacity there is nothing to do.  Otherwise wait for the context's stream AND for `stream`
// -- what still uses the old buffer was enqueued on one of them --, free it, and set the capacity to 0 before allocating: a
// failed allocation then leaves an empty buffer, from which the next call starts over.
static int scratch_reserve(rm_ctx* ctx, Scratch& s, size_t bytes, hipStream_t stream) {
  if (s.bytes >= bytes) return RM_OK;
  if (s.p) {
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stream != ctx->stream) RM_HIP(ctx, hipStreamSynchronize(stream));
  }
  s.release();
  void* p = nullptr;
  RM_HIP(ctx, s.pinned_host ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes));
  s.p = p;
  s.bytes = bytes;
  return RM_OK;
}

static int present_planes(rm_ctx* ctx, const void* color, const void* normal_dof, bool nd_half, int width, int height, int samples, uint8_t* out_rgba8) {
  if (!ctx || !color || !out_rgba8) return fail(ctx, RM_ERR_INVALID, "rm_present_planes: NULL argument");
  if (width < 1 || height < 1 || samples < 1) return fail(ctx, RM_ERR_INVALID, "rm_present_planes: width, height and samples must be >= 1");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)width * (size_t)height * 4;
  if (int rc = scratch_reserve(ctx, ctx->scratch[SCRATCH_PRESENT], bytes, ctx->stream)) return rc;
  void* rgba8 = ctx->scratch[SCRATCH_PRESENT].p;
  if (int rc = present_device(ctx, color, normal_dof, nd_half, width, height, samples, rgba8, nullptr)) return rc;
  RM_HIP(ctx, hipMemcpyAsync(out_rgba8, rgba8, bytes, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

int rm_present_planes(rm_ctx* ctx, const void* color, const void* normal_dof, int width, int height, int samples, uint8_t* out_rgba8) {
  return present_planes(ctx, color, normal_dof, false, width, height, samples, out_rgba8);
}

int rm_present(rm_ctx* ctx, rm_fb* fb, int samples, uint8_t* out_rgba8) {
  if (!ctx || !fb) return fail(ctx, RM_ERR_INVALID, "rm_present: NULL argument");
  if (fb->stripe_rows > 0 || fb->row_begin != 0 || fb->row_count != fb->height)
    return fail(ctx, RM_ERR_INVALID, "rm_present: the blur reads neighbouring rows, so it needs the whole frame: gather the planes and use rm_present_planes (or rm_present_rows when depth of field is off)");
  return present_planes(ctx, fb->plane[0], fb->plane[1], fb->gbuffer == RM_GBUFFER_F16, fb->width, fb->height, samples, out_rgba8);
}

// ---- frame filters: despeckle -> denoise ahead of the present (rm_frame_kernels.inc "denoise", "the variance-guided mode", "despeckle") ----
// Nine entry points, one path.  RmFilters states all of them: rm_denoise* is the chain with the a-trous stage alone, rm_denoise_variance*
// the chain with the variance-guided stage alone.  Each export builds or takes its RmFilters and ends in filter_to_device,
// filter_to_host or filter_to_rgba8, which check (filters_check), enqueue (filters_enqueue) and deliver.

void rm_denoise_default(RmDenoise* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->iterations = 5;
  p->sigma_color = 2.5f;
  p->sigma_normal = 2.0f;
  p->sigma_depth = 0.2f;
}

void rm_denoise_variance_default(RmDenoiseVariance* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->iterations = 3;
  p->sigma_luminance = 4.0f;
  p->sigma_normal = 1.0f;
  p->sigma_depth = 0.2f;
}

void rm_filters_default(RmFilters* f) {
  if (!f) return;
  std::memset(f, 0, sizeof *f);  // both stages off
  f->despeckle_params.radius = 2;
  f->despeckle_params.rank = 1;
  f->despeckle_params.gain = 3.0f;
  f->despeckle_params.floor = 0.1f;
  f->despeckle_params.repair = 1;
  rm_denoise_default(&f->atrous);
  rm_denoise_variance_default(&f->variance);
}

// the chains the older entry points stand for: one denoiser, despeckle off; NULL params = that denoiser's defaults
static RmFilters atrous_chain(const RmDenoise* params) {
  RmFilters f;
  rm_filters_default(&f);
  f.denoise = RM_DENOISE_ATROUS;
  if (params) f.atrous = *params;
  return f;
}
static RmFilters variance_chain(const RmDenoiseVariance* params) {
  RmFilters f;
  rm_filters_default(&f);
  f.denoise = RM_DENOISE_VARIANCE;
  if (params) f.variance = *params;
  return f;
}

// Every check of the nine entry points but the output's, before any device work, in ONE order: the chain's own values (they need
// neither a context nor a GPU: a NULL chain, the stage switches, the despeckle block when that stage is on), the handles (NULL,
// another context's framebuffer, a window or stripes), samples, and then what the selected denoiser refuses: a framebuffer
// without G-buffer planes, its block (reserved -- the variance block's alone --, iterations, the sigmas), a framebuffer without
// the moments plane.  A stage that is off is not looked at.  *d = the denoise stage's parameters as filters_enqueue takes them
// (sigma_color holding the variance-guided mode's sigma_luminance).
static int filters_check(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* f, const char* who, RmDenoise* d) {
  auto refuse = [&](const char* what) { return fail(ctx, RM_ERR_INVALID, std::string(who) + ": " + what); };
  if (!f) return refuse("NULL argument");
  if (f->despeckle != 0 && f->despeckle != 1) return refuse("despeckle must be 0 or 1");
  if (f->denoise != RM_DENOISE_NONE && f->denoise != RM_DENOISE_ATROUS && f->denoise != RM_DENOISE_VARIANCE) return refuse("unknown denoise mode");
  if (f->despeckle) {
    const RmDespeckle& p = f->despeckle_params;
    if (p.radius != 1 && p.radius != 2) return refuse("despeckle radius must be 1 or 2");
    if (p.rank < 0 || p.rank > 3) return refuse("despeckle rank must be in 0..3");
    if (!(std::isfinite(p.gain) && p.gain >= 1.0f)) return refuse("despeckle gain must be finite and >= 1");
    if (!(std::isfinite(p.floor) && p.floor >= 0.0f)) return refuse("despeckle floor must be finite and >= 0");
    if (p.reserved != 0) return refuse("despeckle reserved must be 0");
  }
  if (!ctx || !fb) return refuse("NULL argument");
  if (fb->ctx != ctx) return refuse("framebuffer belongs to another context");
  if (fb->stripe_rows > 0 || fb->row_begin != 0 || fb->row_count != fb->height)
    return refuse("the filter reads neighbouring rows, so it needs a framebuffer holding the whole frame");
  if (samples < 1) return refuse("samples must be >= 1");
  if (f->denoise == RM_DENOISE_NONE) return RM_OK;
  const bool var = f->denoise == RM_DENOISE_VARIANCE;
  *d = var ? RmDenoise{f->variance.iterations, f->variance.sigma_luminance, f->variance.sigma_normal, f->variance.sigma_depth, 0} : f->atrous;
  if (!fb->plane[1] || !fb->plane[2]) return refuse("the framebuffer has no G-buffer planes to guide the filter");
  if (var && f->variance.reserved != 0) return refuse("reserved must be 0");
  if (d->iterations < 0 || d->iterations > 8) return refuse("iterations must be in 0..8");
  for (float v : {d->sigma_color, d->sigma_normal, d->sigma_depth})
    if (!(v > 0.0f && std::isfinite(v))) return refuse("every sigma must be finite and > 0");
  if (var && !fb->moments) return refuse("the framebuffer has no moments plane (create it with RM_FB_MOMENTS)");
  return RM_OK;
}

// Enqueues the chain on `stream` (after filters_check, whose *d this takes).  out: the result, or NULL for one of the context's
// buffers; *result = where it is.  The denoise stage reads the despeckled colour where its statement reads the colour plane; the
// guides and the moments are the framebuffer's own.  With no pass to run -- the denoise stage off, or on with 0 iterations -- the
// result is the despeckled colour, written straight into `out`, or without that stage the colour plane: copied into `out`, and
// without an `out` the plane itself.
static int filters_enqueue(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* f, const RmDenoise* d, float4* out, hipStream_t stream,
                           const float4** result) {
  RM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)fb->width * (size_t)fb->height * sizeof(float4);
  const bool var = f->denoise == RM_DENOISE_VARIANCE;
  const int L = f->denoise == RM_DENOISE_NONE ? 0 : d->iterations;
  float4* despeckled = (L == 0 && out) ? out : nullptr;
  if (f->despeckle && !despeckled) {
    if (int rc = scratch_reserve(ctx, ctx->scratch[SCRATCH_DESPECKLE], bytes, stream)) return rc;
    despeckled = ctx->scratch_as<float4>(SCRATCH_DESPECKLE);
  }
  if (L > 0)  // a live loop denoises every present: the ping-pong buffers of x and the guide stay with the context
    for (int b : {SCRATCH_DENOISE_X0, SCRATCH_DENOISE_X1, SCRATCH_DENOISE_GUIDE})
      if (int rc = scratch_reserve(ctx, ctx->scratch[b], bytes, stream)) return rc;
  const float4* color = fb->plane[0];
  if (f->despeckle) {
    DespecklePass P{};
    P.color = color;
    P.out = despeckled;
    P.W = fb->width;
    P.H = fb->height;
    P.s = 1.0f / (float)samples;  // present_device's scale
    P.gain = f->despeckle_params.gain;
    P.floor = f->despeckle_params.floor;
    P.repair = f->despeckle_params.repair;
    RM_HIP(ctx, rm::launch_despeckle(P, f->despeckle_params.radius, f->despeckle_params.rank, stream));
    color = despeckled;
  }
  if (L == 0) {  // nothing (more) to run: an exact copy
    if (out && color != out) RM_HIP(ctx, hipMemcpyAsync(out, color, bytes, hipMemcpyDeviceToDevice, stream));
    *result = out ? out : color;
    return RM_OK;
  }
  float4* const x[2] = {ctx->scratch_as<float4>(SCRATCH_DENOISE_X0), ctx->scratch_as<float4>(SCRATCH_DENOISE_X1)};
  DenoisePass P{};
  P.color = color;
  P.normal_dof = fb->plane[1];
  P.albedo_depth = fb->plane[2];
  P.guide = ctx->scratch_as<float4>(SCRATCH_DENOISE_GUIDE);
  P.W = fb->width;
  P.H = fb->height;
  P.s = 1.0f / (float)samples;  // present_device's scale
  P.k = (float)samples;
  P.inv_normal = 1.0f / (d->sigma_normal * d->sigma_normal);
  P.moments = var ? fb->moments : nullptr;
  P.sigma_l = d->sigma_color;
  const bool half = fb->gbuffer == RM_GBUFFER_F16;
  for (int i = 0; i < L; i++) {
    P.step = 1 << i;
    P.inv_color = (float)(1 << (2 * i)) / (d->sigma_color * d->sigma_color);  // sigma_c^2 4^-i
    P.sigma_z_h = d->sigma_depth * (float)P.step;
    P.x_in = i > 0 ? x[(i - 1) % 2] : nullptr;
    P.out = (i == L - 1 && out) ? out : x[i % 2];
    RM_HIP(ctx, (var ? rm::launch_denoise_variance_pass : rm::launch_denoise_pass)(P, half, i == 0, i == L - 1, stream));
  }
  *result = P.out;
  return RM_OK;
}

// The three endings.  Onto a caller's device buffer, on the caller's stream (NULL = the context's): no host wait.
static int filter_to_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* f, const char* who, void* out_float4_device, void* hip_stream) {
  RmDenoise d{};
  if (int rc = filters_check(ctx, fb, samples, f, who, &d)) return rc;
  if (!out_float4_device || (reinterpret_cast<uintptr_t>(out_float4_device) & 15u))
    return fail(ctx, RM_ERR_INVALID, std::string(who) + ": the output must be a 16-byte aligned device buffer");
  const float4* r = nullptr;
  return filters_enqueue(ctx, fb, samples, f, &d, static_cast<float4*>(out_float4_device), hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream, &r);
}

// Into host float4, on the context's stream; returns once it is idle.
static int filter_to_host(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* f, const char* who, float* out_host) {
  RmDenoise d{};
  if (int rc = filters_check(ctx, fb, samples, f, who, &d)) return rc;
  if (!out_host) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  const float4* r = nullptr;
  if (int rc = filters_enqueue(ctx, fb, samples, f, &d, nullptr, ctx->stream, &r)) return rc;
  RM_HIP(ctx, hipMemcpyAsync(out_host, r, (size_t)fb->width * (size_t)fb->height * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

// Through rm_present's pass into host RGBA8, likewise.
static int filter_to_rgba8(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* f, const char* who, uint8_t* out_rgba8) {
  RmDenoise d{};
  if (int rc = filters_check(ctx, fb, samples, f, who, &d)) return rc;
  if (!out_rgba8) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  const float4* r = nullptr;
  if (int rc = filters_enqueue(ctx, fb, samples, f, &d, nullptr, ctx->stream, &r)) return rc;
  return present_planes(ctx, r, fb->plane[1], fb->gbuffer == RM_GBUFFER_F16, fb->width, fb->height, samples, out_rgba8);
}

int rm_denoise_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoise* params, void* out_float4_device, void* hip_stream) {
  const RmFilters f = atrous_chain(params);
  return filter_to_device(ctx, fb, samples, &f, "rm_denoise_device", out_float4_device, hip_stream);
}
int rm_denoise(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoise* params, float* out_host) {
  const RmFilters f = atrous_chain(params);
  return filter_to_host(ctx, fb, samples, &f, "rm_denoise", out_host);
}
int rm_present_denoised(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoise* params, uint8_t* out_rgba8) {
  const RmFilters f = atrous_chain(params);
  return filter_to_rgba8(ctx, fb, samples, &f, "rm_present_denoised", out_rgba8);
}

int rm_denoise_variance_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoiseVariance* params, void* out_float4_device, void* hip_stream) {
  const RmFilters f = variance_chain(params);
  return filter_to_device(ctx, fb, samples, &f, "rm_denoise_variance_device", out_float4_device, hip_stream);
}
int rm_denoise_variance(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoiseVariance* params, float* out_host) {
  const RmFilters f = variance_chain(params);
  return filter_to_host(ctx, fb, samples, &f, "rm_denoise_variance", out_host);
}
int rm_present_denoised_variance(rm_ctx* ctx, rm_fb* fb, int samples, const RmDenoiseVariance* params, uint8_t* out_rgba8) {
  const RmFilters f = variance_chain(params);
  return filter_to_rgba8(ctx, fb, samples, &f, "rm_present_denoised_variance", out_rgba8);
}

int rm_filter_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, void* out_float4_device, void* hip_stream) {
  return filter_to_device(ctx, fb, samples, filters, "rm_filter_device", out_float4_device, hip_stream);
}
int rm_filter(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, float* out_host) {
  return filter_to_host(ctx, fb, samples, filters, "rm_filter", out_host);
}
int rm_present_filtered(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, uint8_t* out_rgba8) {
  return filter_to_rgba8(ctx, fb, samples, filters, "rm_present_filtered", out_rgba8);
}

// ---- the display transform: a fourth stage behind the blur, and a fourth ending (rm_frame_kernels.inc "the display transform") ----

void rm_display_default(RmDisplay* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->gain = 1.0f;
  p->tone = RM_TONE_CLIP;
  p->white = 4.0f;
}

// The display block's own values, ahead of filters_check as that orders its own: they need neither a context nor a GPU.
// in == NULL: the default.  *D = the block as the kernel takes it.
static int display_check(rm_ctx* ctx, const RmDisplay* in, const char* who, DisplayPass* D) {
  auto refuse = [&](const char* what) { return fail(ctx, RM_ERR_INVALID, std::string(who) + ": " + what); };
  RmDisplay d;
  rm_display_default(&d);
  if (in) d = *in;
  if (!(std::isfinite(d.gain) && d.gain > 0.0f)) return refuse("display gain must be finite and > 0");
  if (d.tone != RM_TONE_CLIP && d.tone != RM_TONE_REINHARD && d.tone != RM_TONE_ACES) return refuse("display tone must be RM_TONE_CLIP, RM_TONE_REINHARD or RM_TONE_ACES");
  if (d.tone == RM_TONE_REINHARD && !(std::isfinite(d.white) && d.white > 0.0f)) return refuse("display white must be finite and > 0");
  if (d.reserved != 0) return refuse("display reserved must be 0");
  *D = DisplayPass{d.gain, d.tone, d.white * d.white};
  return RM_OK;
}

// The chain, then rm_present's pass ending in the display transform, on `stream`: W x H uchar4 into `out`, or W x H float4 with `linear`.
static int display_enqueue(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* f, const RmDenoise* d, const DisplayPass& D, bool linear, void* out,
                           hipStream_t stream) {
  const float4* r = nullptr;
  if (int rc = filters_enqueue(ctx, fb, samples, f, d, nullptr, stream, &r)) return rc;
  const bool half = fb->gbuffer == RM_GBUFFER_F16;
  const float brightness = 1.0f / (float)samples;  // present_device's scale
  RM_HIP(ctx, ctx->gl_stack ? rm_gl_launch_present_display(r, fb->plane[1], half, fb->width, fb->height, brightness, &D, linear, out, stream)
                            : rm::launch_present_display(r, fb->plane[1], half, fb->width, fb->height, brightness, D, linear, out, stream));
  return RM_OK;
}

// Into host memory through the context's present buffer, on the context's stream; returns once it is idle.
static int display_to_host(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, const char* who, bool linear, void* out_host) {
  DisplayPass D{};
  if (int rc = display_check(ctx, display, who, &D)) return rc;
  RmFilters off;
  rm_filters_default(&off);
  const RmFilters* f = filters ? filters : &off;
  RmDenoise d{};
  if (int rc = filters_check(ctx, fb, samples, f, who, &d)) return rc;
  if (!out_host) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)fb->width * (size_t)fb->height * (linear ? sizeof(float4) : sizeof(uchar4));
  if (int rc = scratch_reserve(ctx, ctx->scratch[SCRATCH_PRESENT], bytes, ctx->stream)) return rc;
  void* image = ctx->scratch[SCRATCH_PRESENT].p;
  if (int rc = display_enqueue(ctx, fb, samples, f, &d, D, linear, image, ctx->stream)) return rc;
  RM_HIP(ctx, hipMemcpyAsync(out_host, image, bytes, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

int rm_present_display(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, uint8_t* out_rgba8) {
  return display_to_host(ctx, fb, samples, filters, display, "rm_present_display", false, out_rgba8);
}
int rm_present_linear(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, float* out_float4_host) {
  return display_to_host(ctx, fb, samples, filters, display, "rm_present_linear", true, out_float4_host);
}
int rm_present_display_device(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, const RmDisplay* display, void* out_rgba8_device, void* hip_stream) {
  const char* who = "rm_present_display_device";
  DisplayPass D{};
  if (int rc = display_check(ctx, display, who, &D)) return rc;
  RmFilters off;
  rm_filters_default(&off);
  const RmFilters* f = filters ? filters : &off;
  RmDenoise d{};
  if (int rc = filters_check(ctx, fb, samples, f, who, &d)) return rc;
  if (!out_rgba8_device || (reinterpret_cast<uintptr_t>(out_rgba8_device) & 3u))
    return fail(ctx, RM_ERR_INVALID, std::string(who) + ": the output must be a 4-byte aligned device buffer");
  return display_enqueue(ctx, fb, samples, f, &d, D, false, out_rgba8_device, hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream);
}

// ---- frame statistics and exposure (rm_frame_kernels.inc "frame statistics") ----------------------------------------------

int rm_frame_stats(rm_ctx* ctx, rm_fb* fb, int samples, const RmFilters* filters, RmFrameStats* out) {
  const char* who = "rm_frame_stats";
  RmDenoise d{};
  if (filters) {
    if (int rc = filters_check(ctx, fb, samples, filters, who, &d)) return rc;
    if (!out) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  } else {
    if (!ctx || !fb || !out) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
    if (fb->ctx != ctx) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": framebuffer belongs to another context");
    if (samples < 1) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": samples must be >= 1");
  }
  RM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = scratch_reserve(ctx, ctx->scratch[SCRATCH_STATS], RM_STATS_BYTES, ctx->stream)) return rc;
  if (int rc = scratch_reserve(ctx, ctx->scratch[SCRATCH_STATS_HOST], RM_STATS_BYTES, ctx->stream)) return rc;
  unsigned long long* const counters = ctx->scratch_as<unsigned long long>(SCRATCH_STATS);
  const unsigned long long* const host = ctx->scratch_as<unsigned long long>(SCRATCH_STATS_HOST);
  const float4* color = fb->plane[0];
  if (filters)
    if (int rc = filters_enqueue(ctx, fb, samples, filters, &d, nullptr, ctx->stream, &color)) return rc;
  const long long pixels = (long long)fb->width * (long long)fb->row_count;
  RM_HIP(ctx, hipMemsetAsync(counters, 0, RM_STATS_BYTES, ctx->stream));
  RM_HIP(ctx, rm::launch_frame_stats(color, pixels, 1.0f / (float)samples, counters, ctx->stream));
  RM_HIP(ctx, hipMemcpyAsync(ctx->scratch[SCRATCH_STATS_HOST].p, counters, RM_STATS_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memset(out, 0, sizeof *out);
  out->pixels = (uint64_t)pixels;
  out->below = host[RM_STATS_BELOW];
  out->above = host[RM_STATS_ABOVE];
  out->non_finite = host[RM_STATS_NON_FINITE];
  for (int b = 0; b < RM_STATS_BINS; b++) out->hist[b] = host[b];
  unsigned int keys[2];  // the complement of the minimum's key, the maximum's key (rm_frame_kernels.inc stats_key)
  std::memcpy(keys, host + RM_STATS_COUNTERS, sizeof keys);
  auto unkey = [](unsigned int k) {
    const unsigned int b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    std::memcpy(&v, &b, sizeof v);
    return v;
  };
  const bool any_finite = out->non_finite < out->pixels;
  out->min_l = any_finite ? unkey(~keys[0]) : std::numeric_limits<float>::infinity();
  out->max_l = any_finite ? unkey(keys[1]) : -std::numeric_limits<float>::infinity();
  return RM_OK;
}

void rm_auto_exposure_default(RmAutoExposure* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->key = 0.18f;
  p->low = 0.10f;
  p->high = 0.95f;
  p->min_gain = 1.0f / 1024.0f;
  p->max_gain = 1024.0f;
}

// lo_b of bin b = 0..RM_STATS_BINS (hi_b = lo_(b+1); lo_512 = 2^12): the float with the bits (b + 1712) << 19
static float stats_bin_edge(int b) {
  const uint32_t bits = (uint32_t)(b + 1712) << 19;
  float v;
  std::memcpy(&v, &bits, sizeof v);
  return v;
}

int rm_stats_percentile(const RmFrameStats* stats, double q, float* l) {
  if (!stats || !l || !(q >= 0.0 && q <= 1.0)) return RM_ERR_INVALID;
  uint64_t N = 0;
  for (uint64_t c : stats->hist) N += c;
  *l = 0.0f;
  if (N == 0) return RM_OK;
  const double r = std::fmax(1.0, std::ceil(q * (double)N));
  uint64_t C = 0;
  for (int b = 0; b < RM_STATS_BINS; b++) {
    C += stats->hist[b];
    if ((double)C >= r) {
      *l = stats_bin_edge(b + 1);
      return RM_OK;
    }
  }
  *l = stats_bin_edge(RM_STATS_BINS);  // not reached: C_511 = N >= r
  return RM_OK;
}

int rm_stats_exposure(const RmFrameStats* stats, const RmAutoExposure* params, float* gain) {
  if (!stats || !gain) return RM_ERR_INVALID;
  RmAutoExposure p;
  rm_auto_exposure_default(&p);
  if (params) p = *params;
  for (float v : {p.key, p.low, p.high, p.min_gain, p.max_gain})
    if (!std::isfinite(v)) return RM_ERR_INVALID;
  if (!(0.0f <= p.low && p.low < p.high && p.high <= 1.0f) || !(p.key > 0.0f) || !(0.0f < p.min_gain && p.min_gain <= p.max_gain) || p.reserved != 0)
    return RM_ERR_INVALID;
  uint64_t N = 0;
  for (uint64_t c : stats->hist) N += c;
  *gain = 1.0f;
  if (N == 0) return RM_OK;
  const double a = (double)p.low * (double)N, b = (double)p.high * (double)N;
  double sum = 0.0;
  uint64_t C = 0;
  for (int i = 0; i < RM_STATS_BINS; i++) {
    const double before = (double)C;
    C += stats->hist[i];
    const double w = std::fmax(0.0, std::fmin((double)C, b) - std::fmax(before, a));
    if (w > 0.0) sum += w * ((std::log2((double)stats_bin_edge(i)) + std::log2((double)stats_bin_edge(i + 1))) / 2.0);
  }
  const double g = (double)p.key / std::exp2(sum / (b - a));
  *gain = (float)std::fmin(std::fmax(g, (double)p.min_gain), (double)p.max_gain);
  return RM_OK;
}

// ---- present of a frame sharded over the GPUs of ONE process ----------------------------------------

int rm_present_striped_rows(rm_ctx* ctx, const void* color, const void* normal_dof, int width, int height, int samples, int stripe_rows, int parts, int part,
                            void* out_rgba8_device, void* hip_stream) {
  if (!ctx || !color || !out_rgba8_device) return fail(ctx, RM_ERR_INVALID, "rm_present_striped_rows: NULL argument");
  if (width < 1 || height < 1 || samples < 1 || stripe_rows < 1 || parts < 1 || part < 0 || part >= parts)
    return fail(ctx, RM_ERR_INVALID, "rm_present_striped_rows: width, height, samples, stripe_rows and parts must be >= 1, 0 <= part < parts");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RM_HIP(ctx, (ctx->gl_stack ? rm_gl_launch_present_striped : rm::launch_present_striped)(
                  static_cast<const float4*>(color), static_cast<const float4*>(normal_dof), width, height, 1.0f / (float)samples, static_cast<uchar4*>(out_rgba8_device),
                  stripe_rows, parts, part, striped_rows_below(height, stripe_rows, parts, part), hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream));
  return RM_OK;
}

// device-to-device, over xGMI between two GPUs (direct access where the topology has it; the copy works either way)
static int shard_copy(rm_ctx* root, rm_ctx* from, rm_ctx* to, void* dst, const void* src, size_t bytes, hipStream_t stream) {
  if (from->device == to->device) {
    RM_HIP(root, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    return RM_OK;
  }
  if (!(from->peer_enabled & (1ull << (to->device & 63)))) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, from->device, to->device) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(to->device, 0);
    (void)hipGetLastError();  // "already enabled" is fine
    from->peer_enabled |= 1ull << (to->device & 63);
  }
  RM_HIP(root, hipMemcpyPeerAsync(dst, to->device, src, from->device, bytes, stream));
  return RM_OK;
}

int rm_present_sharded_start(rm_ctx* const* ctxs, rm_fb* const* fbs, int parts, int samples, int dof) {
  rm_ctx* root = (ctxs && parts >= 1) ? ctxs[0] : nullptr;
  if (!root || !fbs) return fail(root, RM_ERR_INVALID, "rm_present_sharded: NULL argument");
  if (samples < 1) return fail(root, RM_ERR_INVALID, "rm_present_sharded: samples must be >= 1");
  if (root->shard.pending) return fail(root, RM_ERR_INVALID, "rm_present_sharded_start: the previous present has not been finished (rm_present_sharded_finish)");
  using S = ShardPresent;
  const rm_fb* f0 = fbs[0];
  for (int p = 0; p < parts; p++) {
    const rm_fb* f = fbs[p];
    if (!ctxs[p] || !f || f->ctx != ctxs[p]) return fail(root, RM_ERR_INVALID, "rm_present_sharded: framebuffer p must belong to context p");
    if (f->stripe_rows < 1 || f->parts != parts || f->part != p || f->width != f0->width || f->height != f0->height || f->stripe_rows != f0->stripe_rows)
      return fail(root, RM_ERR_INVALID, "rm_present_sharded: framebuffer p must be part p of `parts` striped windows of one image (rm_fb_create_striped)");
    if (dof && !f->plane[1]) return fail(root, RM_ERR_INVALID, "rm_present_sharded: depth of field needs the normal_dof plane");
  }
  const int W = f0->width, H = f0->height, stripe = f0->stripe_rows;
  const int max_rows = striped_rows_below(H, stripe, parts, 0);  // part 0 holds the most rows
  const size_t part8 = (size_t)max_rows * (size_t)W * sizeof(uchar4), part32 = (size_t)max_rows * (size_t)W * sizeof(float4);
  const size_t canvas_bytes = (size_t)H * (size_t)W * sizeof(uchar4);
  // every context's present stream first, then its buffers: what may still use a buffer that has to grow runs on that stream
  for (int p = 0; p < parts; p++) {
    rm_ctx* c = ctxs[p];
    ShardPresent& s = c->shard;
    RM_HIP(root, hipSetDevice(c->device));
    RM_HIP(root, s.ensure(c == root));
    auto reserve = [&](int which, size_t bytes) { return scratch_reserve(c, s.buf[which], bytes, s.stream); };
    int rc = RM_OK;
    if (c == root) rc = reserve(S::RECV, part8 * (size_t)parts);
    if (!rc && c == root) rc = reserve(S::CANVAS, canvas_bytes);
    if (!rc && c == root) rc = reserve(S::HOST, canvas_bytes);
    if (!rc) rc = reserve(S::ROWS, dof ? part32 : part8);
    if (!rc && dof) rc = reserve(S::ROWS8, part8);
    if (!rc && dof) rc = reserve(S::ALL, part32 * (size_t)parts);
    if (!rc && dof) rc = reserve(S::FRAME, (size_t)H * (size_t)W * sizeof(float4));
    if (rc) return c == root ? rc : fail(root, rc, rm_last_error(c));
  }
  // 1. every context snapshots what it holds, on the stream its renders are ordered on: the next samples may start at once (the planes
  //    are accumulated in place).  (The previous present was finished -- checked above -- so its buffers are free.)
  for (int p = 0; p < parts; p++) {
    rm_ctx* c = ctxs[p];
    rm_fb* f = fbs[p];
    RM_HIP(root, hipSetDevice(c->device));
    const long long pixels = (long long)W * (long long)f->row_count;
    if (dof) RM_HIP(root, rm::launch_pack_rows(f->plane[0], f->plane[1], f->gbuffer == RM_GBUFFER_F16, pixels, c->shard.as<float4>(S::ROWS), c->stream));
    else RM_HIP(root, (c->gl_stack ? rm_gl_launch_present_rows : rm::launch_present_rows)(f->plane[0], pixels, 1.0f / (float)samples, c->shard.as<uchar4>(S::ROWS), c->stream));
    RM_HIP(root, hipEventRecord(c->shard.snap, c->stream));
    RM_HIP(root, hipStreamWaitEvent(c->shard.stream, c->shard.snap, 0));
  }
  // 2. everything else travels on the contexts' present streams, beside the renders
  if (dof) {
    // all-gather: every context's packed rows to every context (display.frag:44-55 reads up to 16 rows either side of a pixel, and with
    // 8-row stripes those are other GPUs' rows) ...
    for (int p = 0; p < parts; p++) {
      rm_ctx* c = ctxs[p];
      RM_HIP(root, hipSetDevice(c->device));
      for (int q = 0; q < parts; q++)
        if (int rc = shard_copy(root, c, ctxs[q], ctxs[q]->shard.as<char>(S::ALL) + part32 * (size_t)p, c->shard.buf[S::ROWS].p, (size_t)fbs[p]->row_count * (size_t)W * sizeof(float4), c->shard.stream)) return rc;
      RM_HIP(root, hipEventRecord(c->shard.ev, c->shard.stream));
    }
    // ... then every context puts the frame in image order, blurs and tone-maps ITS stripes (1 / parts of the pass each) and sends
    // the bytes to the root
    for (int q = 0; q < parts; q++) {
      rm_ctx* c = ctxs[q];
      RM_HIP(root, hipSetDevice(c->device));
      for (int p = 0; p < parts; p++) RM_HIP(root, hipStreamWaitEvent(c->shard.stream, ctxs[p]->shard.ev, 0));
      RM_HIP(root, rm::launch_assemble(c->shard.buf[S::ALL].p, parts, max_rows, (long long)W * (long long)sizeof(float4), H, stripe, c->shard.buf[S::FRAME].p, c->shard.stream));
      RM_HIP(root, (c->gl_stack ? rm_gl_launch_present_striped : rm::launch_present_striped)(c->shard.as<const float4>(S::FRAME), c->shard.as<const float4>(S::FRAME), W, H,
                                                                                                1.0f / (float)samples, c->shard.as<uchar4>(S::ROWS8), stripe, parts, q,
                                                                                                fbs[q]->row_count, c->shard.stream));
    }
    for (int q = 0; q < parts; q++) {
      rm_ctx* c = ctxs[q];
      RM_HIP(root, hipSetDevice(c->device));
      if (int rc = shard_copy(root, c, root, root->shard.as<char>(S::RECV) + part8 * (size_t)q, c->shard.buf[S::ROWS8].p, (size_t)fbs[q]->row_count * (size_t)W * sizeof(uchar4), c->shard.stream)) return rc;
      RM_HIP(root, hipEventRecord(c->shard.ev, c->shard.stream));  // (the root waited for the first record above; this one is the next in stream order)
    }
  } else {
    for (int p = 0; p < parts; p++) {
      rm_ctx* c = ctxs[p];
      RM_HIP(root, hipSetDevice(c->device));
      if (int rc = shard_copy(root, c, root, root->shard.as<char>(S::RECV) + part8 * (size_t)p, c->shard.buf[S::ROWS].p, (size_t)fbs[p]->row_count * (size_t)W * sizeof(uchar4), c->shard.stream)) return rc;
      RM_HIP(root, hipEventRecord(c->shard.ev, c->shard.stream));
    }
  }
  // 3. the root puts the bytes in image order and brings the canvas to the host (pinned: the copy is asynchronous)
  RM_HIP(root, hipSetDevice(root->device));
  for (int p = 0; p < parts; p++) RM_HIP(root, hipStreamWaitEvent(root->shard.stream, ctxs[p]->shard.ev, 0));
  RM_HIP(root, rm::launch_assemble(root->shard.buf[S::RECV].p, parts, max_rows, (long long)W * (long long)sizeof(uchar4), H, stripe, root->shard.buf[S::CANVAS].p, root->shard.stream));
  RM_HIP(root, hipMemcpyAsync(root->shard.buf[S::HOST].p, root->shard.buf[S::CANVAS].p, canvas_bytes, hipMemcpyDeviceToHost, root->shard.stream));
  RM_HIP(root, hipEventRecord(root->shard.done, root->shard.stream));
  root->shard.pending = true;
  root->shard.w = W;
  root->shard.h = H;
  return RM_OK;
}

int rm_present_sharded_finish(rm_ctx* const* ctxs, int parts, uint8_t* out_rgba8, size_t out_bytes) {
  rm_ctx* root = (ctxs && parts >= 1) ? ctxs[0] : nullptr;
  if (!root || !out_rgba8) return fail(root, RM_ERR_INVALID, "rm_present_sharded_finish: NULL argument");
  if (!root->shard.pending) return fail(root, RM_ERR_INVALID, "rm_present_sharded_finish: no present was started");
  const size_t bytes = (size_t)root->shard.h * (size_t)root->shard.w * sizeof(uchar4);
  if (out_bytes < bytes) {  // (the present stays pending: the caller can come back with the right buffer)
    char buf[160];
    std::snprintf(buf, sizeof buf, "rm_present_sharded_finish: the pending present is %d x %d (%zu bytes), the buffer holds %zu", root->shard.w, root->shard.h, bytes, out_bytes);
    return fail(root, RM_ERR_INVALID, buf);
  }
  root->shard.pending = false;
  RM_HIP(root, hipSetDevice(root->device));
  RM_HIP(root, hipEventSynchronize(root->shard.done));  // the present's own work only: the renders enqueued since go on
  std::memcpy(out_rgba8, root->shard.buf[ShardPresent::HOST].p, bytes);
  return RM_OK;
}

int rm_present_sharded(rm_ctx* const* ctxs, rm_fb* const* fbs, int parts, int samples, int dof, uint8_t* out_rgba8, size_t out_bytes) {
  rm_ctx* root = (ctxs && parts >= 1) ? ctxs[0] : nullptr;
  if (!out_rgba8) return fail(root, RM_ERR_INVALID, "rm_present_sharded: NULL argument");
  if (fbs && parts >= 1 && fbs[0] && out_bytes < (size_t)fbs[0]->width * (size_t)fbs[0]->height * sizeof(uchar4))
    return fail(root, RM_ERR_INVALID, "rm_present_sharded: the buffer is smaller than width * height * 4 bytes");  // (before anything is started)
  if (int rc = rm_present_sharded_start(ctxs, fbs, parts, samples, dof)) return rc;
  return rm_present_sharded_finish(ctxs, parts, out_rgba8, out_bytes);
}

// ---- probes ----------------------------------------------------------------------

// One probe launch on device arrays: the scene as the flags shape it, in the unit the flags and the context select.  rm_probe's, and the
// mesh entries' for the normals and colours of a mesh (rm_mesh_host.inc).
static hipError_t probe_enqueue(rm_ctx* ctx, rm_scene* scene, int what, const float* d_in, float* d_out, int n, float param, int flags, hipStream_t stream) {
  ProbeParams P{scene_view(scene, flags), d_in, d_out, n, what, param, (flags & RM_RENDER_FAST) ? ctx->retire_eps : 0.0f, (flags & RM_RENDER_NO_FAR_JUMP) ? 1 : 0};
  if (P.no_far_jump) P.scene.far_end = 0, P.scene.clear_rho = 0.0f;
  return RM_SCENE_PASS(ctx, flags, launch_probe, P, stream);
}

int rm_probe(rm_ctx* ctx, rm_scene* scene, int what, const float* in, int n, float param, int flags, float* out) {
  const Refuse refuse{ctx, "rm_probe"};
  if (int rc = scene_check(refuse, scene, in && out)) return rc;
  if (what < RM_PROBE_SDF || what > RM_PROBE_CAST_SHADOW) return refuse("unknown probe");
  if (n <= 0) return RM_OK;
  static const int in_w[6] = {3, 6, 3, 3, 6, 9}, out_w[6] = {1, 3, 3, 12, 1, 1};
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray d_in, d_out;  // (freed behind the wait below; a call that fails before it leaves that wait to hipFree)
  const size_t in_bytes = sizeof(float) * (size_t)in_w[what] * (size_t)n, out_bytes = sizeof(float) * (size_t)out_w[what] * (size_t)n;
  RM_HIP(ctx, d_in.reserve(in_bytes));
  RM_HIP_AS(refuse, d_out.reserve(out_bytes));
  RM_HIP_AS(refuse, hipMemcpyAsync(d_in.p, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = scene_cull_grid(ctx, scene, flags, 1ll << 40)) return rc;  // (a probe is a test's call: with the grid)
  RM_HIP_AS(refuse, probe_enqueue(ctx, scene, what, d_in.f32(), d_out.f32(), n, param, flags, ctx->stream));
  RM_HIP_AS(refuse, hipMemcpyAsync(out, d_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP_AS(refuse, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

static int camera_rng(rm_ctx* ctx, const RmUniforms* u, int width, int height, int what, int count, float* out) {
  const Refuse refuse{ctx, "probe"};
  if (!ctx || !u || !out || width < 1 || height < 1 || count < 1) return refuse("bad argument");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray d_out;
  const size_t bytes = sizeof(float) * (size_t)width * (size_t)height * (size_t)(what == 1 ? count : 8);
  RM_HIP(ctx, d_out.reserve(bytes));
  RM_HIP_AS(refuse, ctx->gl_stack ? rm_gl_launch_camera_rng(u, width, height, what, count, d_out.f32(), ctx->stream)
                                  : rm::launch_camera_rng(*u, width, height, what, count, d_out.f32(), ctx->stream));
  RM_HIP_AS(refuse, hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP_AS(refuse, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

int rm_probe_math(rm_ctx* ctx, int fn, const float* a, const float* b, int n, float* out) {
  const Refuse refuse{ctx, "rm_probe_math"};
  if (!ctx || !a || !out || n < 1 || fn < 0 || fn >= RM_MATH_COUNT) return refuse("bad argument");
  const bool two = fn == RM_MATH_POW || fn == RM_MATH_ATAN2 || fn == RM_MATH_POW_PAIR_NM1 || fn == RM_MATH_POW_PAIR_N || fn == RM_MATH_DIV;
  if (two && !b) return refuse("this function takes two arguments");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray abo;  // a | b | out
  const size_t bytes = sizeof(float) * (size_t)n;
  RM_HIP(ctx, abo.reserve(3 * bytes));
  float* d = abo.f32();
  RM_HIP_AS(refuse, hipMemcpyAsync(d, a, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (two) RM_HIP_AS(refuse, hipMemcpyAsync(d + n, b, bytes, hipMemcpyHostToDevice, ctx->stream));
  RM_HIP_AS(refuse, ctx->gl_stack ? rm_gl_launch_math_probe(fn, d, two ? d + n : nullptr, n, d + 2 * (size_t)n, ctx->stream)
                                  : rm::launch_math_probe(fn, d, two ? d + n : nullptr, n, d + 2 * (size_t)n, ctx->stream));
  RM_HIP_AS(refuse, hipMemcpyAsync(out, d + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP_AS(refuse, hipStreamSynchronize(ctx->stream));
  return RM_OK;
}

int rm_probe_camera(rm_ctx* ctx, const RmUniforms* uniforms, int width, int height, float* out) {
  return camera_rng(ctx, uniforms, width, height, 0, 1, out);
}

int rm_probe_rng(rm_ctx* ctx, const RmUniforms* uniforms, int width, int height, int count, float* out) {
  return camera_rng(ctx, uniforms, width, height, 1, count, out);
}

#include "rm_mesh_host.inc"

}  // extern "C"
