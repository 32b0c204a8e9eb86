// ---- mesh extraction (include/hip_raymarch.h "mesh extraction"; kernels: rm_mesh_kernels.inc) ------------------------------------
// Included by rm_api.hip inside its extern "C" block, behind the probes.

struct rm_mesh {
  rm_ctx* ctx = nullptr;
  unsigned long long vertices = 0, triangles = 0;
  void* array[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // RM_MESH_*; NULL when absent or empty
  bool has[5] = {true, false, false, true, true};                   // normals and colours: when rm_mesh_extract was asked for them
  float ms[3] = {0.0f, 0.0f, 0.0f};                                 // rm_mesh_timings: sampling, meshing, attributes
  // rm_mesh_components' result, kept once made (the arrays above never change): V labels, `components` pairs of sizes; NULL when empty
  bool labelled = false;
  unsigned long long components = 0;
  void* labels = nullptr;
  void* sizes = nullptr;
};

// device memory that is freed when the call that made it returns, unless the mesh has taken it
struct MeshBuffer {
  void* p = nullptr;
  ~MeshBuffer() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) { return bytes ? hipMalloc(&p, bytes) : hipSuccess; }
  void* release() { void* q = p; p = nullptr; return q; }
  float* f32() const { return static_cast<float*>(p); }
  unsigned int* u32() const { return static_cast<unsigned int*>(p); }
  unsigned long long* u64() const { return static_cast<unsigned long long*>(p); }
};

static size_t mesh_array_bytes(const rm_mesh* m, int what) {
  return what == RM_MESH_TRIANGLES ? (size_t)m->triangles * 12u : what == RM_MESH_CELLS ? (size_t)m->vertices * 4u : (size_t)m->vertices * 12u;
}

// RmGrid's rule, and the grid as the kernels take it
static int grid_check(rm_ctx* ctx, const RmGrid* grid, const char* who, GridDims* G) {
  auto refuse = [&](const char* what) { return fail(ctx, RM_ERR_INVALID, std::string(who) + ": " + what); };
  if (!grid) return refuse("NULL grid");
  long long corners = 1;
  for (int a = 0; a < 3; a++) {
    if (grid->n[a] < 1 || grid->n[a] > 1024) return refuse("grid n must be in 1..1024 cells per axis");
    if (!std::isfinite(grid->lo[a]) || !std::isfinite(grid->hi[a])) return refuse("grid lo and hi must be finite");
    const float extent = grid->hi[a] - grid->lo[a];
    const float h = extent / (float)grid->n[a];
    if (!(std::isfinite(h) && h > 0.0f)) return refuse("grid cell size (hi - lo) / n must be finite and > 0");
    G->lo[a] = grid->lo[a];
    G->h[a] = h;
    G->nc[a] = grid->n[a] + 1;
    corners *= grid->n[a] + 1;
  }
  if (corners > (1ll << 28)) return refuse("grid must have at most 2^28 corners");
  if (grid->reserved != 0) return refuse("grid reserved must be 0");
  G->corners = (int)corners;
  return RM_OK;
}

static int sdf_flags_check(rm_ctx* ctx, int flags, const char* who) {
  if (flags & ~(RM_RENDER_FAST | RM_RENDER_NO_CULL)) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both");
  return RM_OK;
}

static int mesh_params_check(rm_ctx* ctx, const RmMeshParams* in, const char* who, RmMeshParams* p) {
  auto refuse = [&](const char* what) { return fail(ctx, RM_ERR_INVALID, std::string(who) + ": " + what); };
  rm_mesh_params_default(p);
  if (in) *p = *in;
  if (!std::isfinite(p->iso)) return refuse("iso must be finite");
  if (p->normals != 0 && p->normals != 1) return refuse("normals must be 0 or 1");
  if (p->colours != 0 && p->colours != 1) return refuse("colours must be 0 or 1");
  if (p->normals && !(std::isfinite(p->normal_delta) && p->normal_delta > 0.0f)) return refuse("normal_delta must be finite and > 0");
  if (int rc = sdf_flags_check(ctx, p->flags, who)) return rc;
  if (p->reserved != 0) return refuse("reserved must be 0");
  return RM_OK;
}

int rm_grid_axis(const RmGrid* grid, int axis, float* out) {
  GridDims G{};
  if (int rc = grid_check(nullptr, grid, "rm_grid_axis", &G)) return rc;
  if (axis < 0 || axis > 2 || !out) return fail(nullptr, RM_ERR_INVALID, "rm_grid_axis: axis must be 0..2 and out non-NULL");
  for (int i = 0; i < G.nc[axis]; i++) out[i] = rm_grid_coord(G, axis, i);
  return RM_OK;
}

void rm_mesh_params_default(RmMeshParams* params) {
  if (!params) return;
  *params = RmMeshParams{0.0f, 1, 1e-5f, 0, 0, 0};
}

// The marks between the stages of an extraction, on the context's stream (timing events the context keeps): 0 | sampler | 1 | count, scan | 2
// ... the totals come to the host, the arrays are allocated ... 3 | emit | 4, 5 | normals, colours | 6.  rm_mesh_extract_sharp has, between 4
// and 5 and behind the allocation of its scratch, 7 | crossings, rounds, normals, QEF | 8.
// rm_mesh_components and rm_mesh_filter have marks of their own: 9 | init, rounds, scan, labels, sizes | 10, and 11 | keep flags, scans | 12 ...
// the totals come to the host, the arrays are allocated ... 13 | gathers | 14.
enum { MESH_MARK_BEGIN, MESH_MARK_SAMPLED, MESH_MARK_SCANNED, MESH_MARK_EMIT, MESH_MARK_EMITTED, MESH_MARK_ATTRIBUTES, MESH_MARK_END, MESH_MARK_SHARPEN,
       MESH_MARK_SHARPENED, MESH_MARK_LABEL, MESH_MARK_LABELLED, MESH_MARK_FLAG, MESH_MARK_FLAGGED, MESH_MARK_GATHER, MESH_MARK_GATHERED, MESH_MARKS };
static_assert(MESH_MARKS == sizeof(rm_ctx::mesh_ev) / sizeof(hipEvent_t), "rm_ctx::mesh_ev holds one event per mark");
static hipError_t mesh_mark(rm_ctx* ctx, int k) {
  if (!ctx->mesh_ev[k]) {
    const hipError_t e = hipEventCreate(&ctx->mesh_ev[k]);
    if (e != hipSuccess) return e;
  }
  return hipEventRecord(ctx->mesh_ev[k], ctx->stream);
}
// milliseconds between two marks that the stream has passed; 0 when the runtime cannot tell
static float mesh_between(rm_ctx* ctx, int from, int to) {
  float ms = 0.0f;
  return hipEventElapsedTime(&ms, ctx->mesh_ev[from], ctx->mesh_ev[to]) == hipSuccess ? ms : 0.0f;
}

// the sampler on `stream`, with the culling grid as rm_probe obtains it
static int sdf_grid_enqueue(rm_ctx* ctx, rm_scene* scene, const GridDims& G, int flags, float* d_out, hipStream_t stream, const char* who) {
  RM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = scene_cull_grid(ctx, scene, flags, 1ll << 40)) return rc;
  const bool foreign = stream != ctx->stream;
  if (foreign && ctx->cull_event) RM_HIP(ctx, hipStreamWaitEvent(stream, ctx->cull_event, 0));  // (the grid is built on a stream of its own)
  SdfGridParams P{scene->dev, G, d_out};
  if (flags & RM_RENDER_NO_CULL) P.scene.cull.cells = nullptr;
  const hipError_t e = (flags & RM_RENDER_FAST) ? rm::launch_sdf_grid_fast(P, stream) : ctx->gl_stack ? rm_gl_launch_sdf_grid(&P, stream) : rm::launch_sdf_grid_strict(P, stream);
  if (e != hipSuccess) return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
  if (foreign) {
    // Everything that gives a scene's table or culling grid up -- rm_scene_destroy, the grids' budget (cull_release, cull_order) -- orders itself
    // behind the CONTEXT's stream: so that stream waits behind this launch, on the device, and the caller's stream needs no care of the host's.
    if (!ctx->mesh_order) RM_HIP(ctx, hipEventCreateWithFlags(&ctx->mesh_order, hipEventDisableTiming));
    RM_HIP(ctx, hipEventRecord(ctx->mesh_order, stream));
    RM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->mesh_order, 0));
  }
  return RM_OK;
}

static int sdf_grid_check(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, const void* out, const char* who, GridDims* G) {
  if (int rc = grid_check(ctx, grid, who, G)) return rc;
  if (int rc = sdf_flags_check(ctx, flags, who)) return rc;
  if (!ctx || !scene || !out) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  if (scene->ctx != ctx) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": the scene belongs to another context");
  return RM_OK;
}

int rm_sdf_grid_device(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, void* out_device, void* hip_stream) {
  const char* who = "rm_sdf_grid_device";
  GridDims G{};
  if (int rc = sdf_grid_check(ctx, scene, grid, flags, out_device, who, &G)) return rc;
  if (reinterpret_cast<uintptr_t>(out_device) & 3u) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": the output must be a 4-byte aligned device buffer");
  return sdf_grid_enqueue(ctx, scene, G, flags, static_cast<float*>(out_device), hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream, who);
}

int rm_sdf_grid(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, float* out_host) {
  const char* who = "rm_sdf_grid";
  GridDims G{};
  if (int rc = sdf_grid_check(ctx, scene, grid, flags, out_host, who, &G)) return rc;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  MeshBuffer values;
  RM_HIP(ctx, values.reserve(sizeof(float) * (size_t)G.corners));
  if (int rc = sdf_grid_enqueue(ctx, scene, G, flags, values.f32(), ctx->stream, who)) return rc;
  return copy_and_wait(ctx, out_host, values.p, sizeof(float) * (size_t)G.corners, hipMemcpyDeviceToHost);
}

// The mesher on d_values (on the context's stream): count, scan, read the totals, emit.  The mesh takes its three arrays; the counts and
// the scan's scratch go when this returns.
static int mesh_build(rm_ctx* ctx, const GridDims& G, const float* d_values, float iso, rm_mesh* mesh) {
  const long long cells = (long long)(G.nc[0] - 1) * (G.nc[1] - 1) * (G.nc[2] - 1);
  const size_t scratch_elems = rm::rm_mesh_scan_scratch_elems(cells) + 1;  // ... and the total behind the levels
  MeshBuffer counts, scratch, positions, vertex_cells, triangles;
  RM_HIP(ctx, counts.reserve(sizeof(unsigned long long) * (size_t)cells));
  RM_HIP(ctx, scratch.reserve(sizeof(unsigned long long) * scratch_elems));
  unsigned long long* d_total = scratch.u64() + (scratch_elems - 1);
  MeshParams P{G, d_values, iso, counts.u64(), nullptr, nullptr, nullptr};
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_SAMPLED));  // (behind the sampler, or the upload of the caller's field)
  RM_HIP(ctx, rm::launch_mesh_count(P, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_scan(P.counts, cells, scratch.u64(), d_total, ctx->stream));
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_SCANNED));
  unsigned long long total = 0;
  if (int rc = copy_and_wait(ctx, &total, d_total, sizeof total, hipMemcpyDeviceToHost)) return rc;
  mesh->vertices = total & 0xFFFFFFFFull;
  mesh->triangles = 2ull * (total >> 32);
  mesh->ms[1] = mesh_between(ctx, MESH_MARK_SAMPLED, MESH_MARK_SCANNED);
  if (mesh->vertices == 0) return RM_OK;
  RM_HIP(ctx, positions.reserve(mesh_array_bytes(mesh, RM_MESH_POSITIONS)));
  RM_HIP(ctx, vertex_cells.reserve(mesh_array_bytes(mesh, RM_MESH_CELLS)));
  RM_HIP(ctx, triangles.reserve(mesh_array_bytes(mesh, RM_MESH_TRIANGLES)));
  P.positions = positions.f32();
  P.cells = vertex_cells.u32();
  P.triangles = triangles.u32();
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_EMIT));
  RM_HIP(ctx, rm::launch_mesh_emit(P, ctx->stream));
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_EMITTED));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mesh->ms[1] += mesh_between(ctx, MESH_MARK_EMIT, MESH_MARK_EMITTED);
  mesh->array[RM_MESH_POSITIONS] = positions.release();
  mesh->array[RM_MESH_CELLS] = vertex_cells.release();
  mesh->array[RM_MESH_TRIANGLES] = triangles.release();
  return RM_OK;
}

void rm_mesh_destroy(rm_mesh* mesh) {
  if (!mesh) return;
  (void)hipSetDevice(mesh->ctx->device);
  (void)hipStreamSynchronize(mesh->ctx->stream);
  for (void* p : mesh->array)
    if (p) (void)hipFree(p);
  if (mesh->labels) (void)hipFree(mesh->labels);
  if (mesh->sizes) (void)hipFree(mesh->sizes);
  delete mesh;
}

int rm_mesh_from_values(rm_ctx* ctx, const RmGrid* grid, const float* values_host, float iso, rm_mesh** out) {
  const char* who = "rm_mesh_from_values";
  GridDims G{};
  if (int rc = grid_check(ctx, grid, who, &G)) return rc;
  if (!std::isfinite(iso)) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": iso must be finite");
  if (!ctx || !values_host || !out) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  MeshBuffer values;
  RM_HIP(ctx, values.reserve(sizeof(float) * (size_t)G.corners));
  RM_HIP(ctx, hipMemcpyAsync(values.p, values_host, sizeof(float) * (size_t)G.corners, hipMemcpyHostToDevice, ctx->stream));
  rm_mesh* mesh = new (std::nothrow) rm_mesh;
  if (!mesh) return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": out of host memory");
  mesh->ctx = ctx;
  if (int rc = mesh_build(ctx, G, values.f32(), iso, mesh)) { rm_mesh_destroy(mesh); return rc; }  // (it has waited for the stream)
  *out = mesh;
  return RM_OK;
}

// The arrays only a scene can give: the probe kernel (probe_enqueue, rm_probe's own launch) at the vertex positions.  Enqueued only: the
// caller waits for the stream once, and the material records are freed behind that wait.
static int mesh_attributes(rm_ctx* ctx, rm_scene* scene, const RmMeshParams& p, rm_mesh* mesh, MeshBuffer& material) {
  const int n = (int)mesh->vertices;
  const float* positions = static_cast<const float*>(mesh->array[RM_MESH_POSITIONS]);
  MeshBuffer normals, colours;
  if (p.normals) RM_HIP(ctx, normals.reserve(mesh_array_bytes(mesh, RM_MESH_NORMALS)));
  if (p.colours) {  // the probe writes 12 floats per point: the diffuse colour is the first three
    RM_HIP(ctx, colours.reserve(mesh_array_bytes(mesh, RM_MESH_COLOURS)));
    RM_HIP(ctx, material.reserve(sizeof(float) * 12u * (size_t)n));
  }
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_ATTRIBUTES));
  if (p.normals) RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, positions, normals.f32(), n, p.normal_delta, p.flags, ctx->stream));
  if (p.colours) {
    RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_MATERIAL, positions, material.f32(), n, 0.0f, p.flags, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_colours(material.f32(), colours.f32(), n, ctx->stream));
  }
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_END));
  mesh->array[RM_MESH_NORMALS] = normals.release();  // (the mesh's from here: rm_mesh_destroy waits for the stream before it frees them)
  mesh->array[RM_MESH_COLOURS] = colours.release();
  return RM_OK;
}

// Sharp vertices (the header's "sharp vertices"): the emitted mesh's positions become the QEF's.  Per vertex 12 slots of bracket, point and
// probe output, owned here and gone when this returns; the scene is evaluated by the probe kernel on the slot arrays, one launch per round
// and one for the normals.  Waits for the stream: the scratch is freed behind the last kernel that reads it.
static int mesh_sharpen(rm_ctx* ctx, rm_scene* scene, const GridDims& G, const float* d_values, const RmMeshParams& p, const RmMeshSharp& sharp, rm_mesh* mesh,
                        const char* who) {
  if (mesh->vertices > (unsigned long long)INT_MAX / 12ull)
    return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": the mesh has more vertices than the probe's int count holds twelve slots of (12 V > INT_MAX)");
  const size_t slots = 12u * (size_t)mesh->vertices;
  MeshBuffer state, points, probed, live;
  RM_HIP(ctx, state.reserve(sizeof(float4) * slots));
  RM_HIP(ctx, points.reserve(sizeof(float) * 3u * slots));
  RM_HIP(ctx, probed.reserve(sizeof(float) * 3u * slots));
  RM_HIP(ctx, live.reserve(sizeof(unsigned int) * (size_t)mesh->vertices));
  MeshSharpParams P{};
  P.mesh = MeshParams{G, d_values, p.iso, nullptr, static_cast<float*>(mesh->array[RM_MESH_POSITIONS]), static_cast<unsigned int*>(mesh->array[RM_MESH_CELLS]), nullptr};
  P.vertices = (int)mesh->vertices;
  P.state = static_cast<float4*>(state.p);
  P.points = points.f32();
  P.probed = probed.f32();
  P.live = live.u32();
  P.threshold = sharp.threshold;
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_SHARPEN));
  RM_HIP(ctx, rm::launch_mesh_cross(P, 1, 0, sharp.refine == 0, ctx->stream));
  for (int round = 0; round < sharp.refine; round++) {
    RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_SDF, points.f32(), probed.f32(), (int)slots, 0.0f, p.flags, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_cross(P, 0, 1, round == sharp.refine - 1, ctx->stream));
  }
  RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, points.f32(), probed.f32(), (int)slots, sharp.normal_delta, p.flags, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_qef(P, ctx->stream));
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_SHARPENED));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mesh->ms[1] += mesh_between(ctx, MESH_MARK_SHARPEN, MESH_MARK_SHARPENED);
  return RM_OK;
}

void rm_mesh_sharp_default(RmMeshSharp* sharp) {
  if (!sharp) return;
  *sharp = RmMeshSharp{6, 0x1p-10f, 0.1f, 0};
}

static int mesh_sharp_check(rm_ctx* ctx, const RmMeshSharp* in, const char* who, RmMeshSharp* s) {
  auto refuse = [&](const char* what) { return fail(ctx, RM_ERR_INVALID, std::string(who) + ": " + what); };
  rm_mesh_sharp_default(s);
  if (in) *s = *in;
  if (s->refine < 0 || s->refine > 16) return refuse("sharp refine must be in 0..16");
  if (!(std::isfinite(s->normal_delta) && s->normal_delta > 0.0f)) return refuse("sharp normal_delta must be finite and > 0");
  if (!(std::isfinite(s->threshold) && s->threshold >= 0.0f && s->threshold < 1.0f)) return refuse("sharp threshold must be finite and in [0, 1)");
  if (s->reserved != 0) return refuse("sharp reserved must be 0");
  return RM_OK;
}

// rm_mesh_extract and rm_mesh_extract_sharp: `sharpen` tells them apart, `sharp` (NULL = the defaults) is looked at only with it
static int mesh_extract(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, bool sharpen, const RmMeshSharp* sharp, rm_mesh** out,
                        const char* who) {
  GridDims G{};
  RmMeshParams p;
  RmMeshSharp s{};
  if (int rc = grid_check(ctx, grid, who, &G)) return rc;
  if (int rc = mesh_params_check(ctx, params, who, &p)) return rc;
  if (sharpen)
    if (int rc = mesh_sharp_check(ctx, sharp, who, &s)) return rc;
  if (!ctx || !scene || !out) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  if (scene->ctx != ctx) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": the scene belongs to another context");
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  MeshBuffer values, material;
  RM_HIP(ctx, values.reserve(sizeof(float) * (size_t)G.corners));
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_BEGIN));
  if (int rc = sdf_grid_enqueue(ctx, scene, G, p.flags, values.f32(), ctx->stream, who)) return rc;
  rm_mesh* mesh = new (std::nothrow) rm_mesh;
  if (!mesh) return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": out of host memory");
  mesh->ctx = ctx;
  mesh->has[RM_MESH_NORMALS] = p.normals != 0;
  mesh->has[RM_MESH_COLOURS] = p.colours != 0;
  int rc = mesh_build(ctx, G, values.f32(), p.iso, mesh);
  if (rc == RM_OK && sharpen && mesh->vertices > 0) rc = mesh_sharpen(ctx, scene, G, values.f32(), p, s, mesh, who);
  const bool attributes = rc == RM_OK && mesh->vertices > 0 && (p.normals || p.colours);
  if (attributes) rc = mesh_attributes(ctx, scene, p, mesh, material);
  if (rc == RM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RM_ERR_DEVICE, std::string(who) + ": the stream failed");
  if (rc != RM_OK) { rm_mesh_destroy(mesh); return rc; }
  mesh->ms[0] = mesh_between(ctx, MESH_MARK_BEGIN, MESH_MARK_SAMPLED);
  if (attributes) mesh->ms[2] = mesh_between(ctx, MESH_MARK_ATTRIBUTES, MESH_MARK_END);
  *out = mesh;
  return RM_OK;
}

int rm_mesh_extract(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, rm_mesh** out) {
  return mesh_extract(ctx, scene, grid, params, false, nullptr, out, "rm_mesh_extract");
}

int rm_mesh_extract_sharp(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSharp* sharp, rm_mesh** out) {
  return mesh_extract(ctx, scene, grid, params, true, sharp, out, "rm_mesh_extract_sharp");
}

int rm_mesh_counts(const rm_mesh* mesh, unsigned long long* out2) {
  if (!mesh || !out2) return RM_ERR_INVALID;
  out2[0] = mesh->vertices;
  out2[1] = mesh->triangles;
  return RM_OK;
}

int rm_mesh_timings(const rm_mesh* mesh, float* out_ms3) {
  if (!mesh || !out_ms3) return RM_ERR_INVALID;
  for (int k = 0; k < 3; k++) out_ms3[k] = mesh->ms[k];
  return RM_OK;
}

int rm_mesh_download(rm_mesh* mesh, int what, void* host, size_t bytes) {
  if (!mesh) return fail(nullptr, RM_ERR_INVALID, "rm_mesh_download: NULL mesh");
  rm_ctx* ctx = mesh->ctx;
  if (what < RM_MESH_POSITIONS || what > RM_MESH_CELLS) return fail(ctx, RM_ERR_INVALID, "rm_mesh_download: unknown array");
  if (!mesh->has[what]) return fail(ctx, RM_ERR_INVALID, "rm_mesh_download: the mesh was made without this array");
  if (bytes != (mesh->array[what] ? mesh_array_bytes(mesh, what) : 0u)) return fail(ctx, RM_ERR_INVALID, "rm_mesh_download: bytes must be the array's exact size");
  if (bytes == 0) return RM_OK;
  if (!host) return fail(ctx, RM_ERR_INVALID, "rm_mesh_download: NULL argument");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  return copy_and_wait(ctx, host, mesh->array[what], bytes, hipMemcpyDeviceToHost);
}

void* rm_mesh_device_ptr(rm_mesh* mesh, int what) {
  if (!mesh || what < RM_MESH_POSITIONS || what > RM_MESH_CELLS) return nullptr;
  return mesh->array[what];
}

// ---- components and islands (include/hip_raymarch.h "components and islands") --------------------------------------------------------

void rm_mesh_keep_default(RmMeshKeep* keep) {
  if (!keep) return;
  *keep = RmMeshKeep{1, 0, {0, 0}};
}

// The labelling, once per mesh: a forest over the vertices by rounds of hook + flatten until a hook pass met no two roots, the roots numbered
// by the scan, the sizes counted.  On the context's stream; waits for it.  *ms (when given) gains the time between its marks if it ran.
static int mesh_label(rm_mesh* mesh, const char* who, float* ms) {
  if (mesh->labelled) return RM_OK;
  rm_ctx* ctx = mesh->ctx;
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  if (T >= (1ull << 32)) return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": the mesh has more triangles than a uint32 size holds (T >= 2^32)");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  if (V == 0) {
    mesh->labelled = true;
    return RM_OK;
  }
  const size_t scratch_elems = rm::rm_mesh_scan_scratch_elems((long long)V) + 2;  // ... the total, and the word the hook pass sets, behind the levels
  MeshBuffer parent, words, scratch, labels, sizes;
  RM_HIP(ctx, parent.reserve(sizeof(unsigned int) * (size_t)V));
  RM_HIP(ctx, words.reserve(sizeof(unsigned long long) * (size_t)V));
  RM_HIP(ctx, scratch.reserve(sizeof(unsigned long long) * scratch_elems));
  RM_HIP(ctx, labels.reserve(sizeof(unsigned int) * (size_t)V));
  unsigned long long* d_total = scratch.u64() + (scratch_elems - 2);
  unsigned int* d_changed = reinterpret_cast<unsigned int*>(scratch.u64() + (scratch_elems - 1));
  const unsigned int* triangles = static_cast<const unsigned int*>(mesh->array[RM_MESH_TRIANGLES]);
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_LABEL));
  RM_HIP(ctx, rm::launch_mesh_link_init(parent.u32(), (long long)V, ctx->stream));
  const int max_rounds = 64;
  int round = 0;
  for (unsigned int changed = T > 0 ? 1u : 0u; changed != 0u; round++) {
    if (round == max_rounds) return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": the labelling did not converge in 64 rounds");
    RM_HIP(ctx, hipMemsetAsync(d_changed, 0, sizeof(unsigned long long), ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_link_hook(parent.u32(), triangles, (long long)V, (long long)T, d_changed, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_link_flatten(parent.u32(), (long long)V, ctx->stream));
    if (int rc = copy_and_wait(ctx, &changed, d_changed, sizeof changed, hipMemcpyDeviceToHost)) return rc;
  }
  RM_HIP(ctx, rm::launch_mesh_roots(parent.u32(), words.u64(), (long long)V, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_scan(words.u64(), (long long)V, scratch.u64(), d_total, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_labels(parent.u32(), words.u64(), labels.u32(), (long long)V, ctx->stream));
  unsigned long long total = 0;
  if (int rc = copy_and_wait(ctx, &total, d_total, sizeof total, hipMemcpyDeviceToHost)) return rc;
  RM_HIP(ctx, sizes.reserve(sizeof(unsigned int) * 2u * (size_t)total));
  RM_HIP(ctx, hipMemsetAsync(sizes.p, 0, sizeof(unsigned int) * 2u * (size_t)total, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_part_sizes(labels.u32(), nullptr, (long long)V, sizes.u32(), 0, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_part_sizes(labels.u32(), triangles, (long long)T, sizes.u32(), 1, ctx->stream));
  RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_LABELLED));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ms) *ms += mesh_between(ctx, MESH_MARK_LABEL, MESH_MARK_LABELLED);
  mesh->components = total;
  mesh->labels = labels.release();
  mesh->sizes = sizes.release();
  mesh->labelled = true;
  return RM_OK;
}

int rm_mesh_components(rm_mesh* mesh, unsigned long long* out_count) {
  if (!mesh || !out_count) return fail(mesh ? mesh->ctx : nullptr, RM_ERR_INVALID, "rm_mesh_components: NULL argument");
  if (int rc = mesh_label(mesh, "rm_mesh_components", nullptr)) return rc;
  *out_count = mesh->components;
  return RM_OK;
}

int rm_mesh_components_download(rm_mesh* mesh, int what, void* host, size_t bytes) {
  const char* who = "rm_mesh_components_download";
  if (!mesh) return fail(nullptr, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  rm_ctx* ctx = mesh->ctx;
  if (what != RM_MESH_PART_LABELS && what != RM_MESH_PART_SIZES) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": unknown array");
  if (int rc = mesh_label(mesh, who, nullptr)) return rc;
  const size_t size = what == RM_MESH_PART_LABELS ? (size_t)mesh->vertices * 4u : (size_t)mesh->components * 8u;
  if (bytes != size) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": bytes must be the array's exact size");
  if (bytes == 0) return RM_OK;
  if (!host) return fail(ctx, RM_ERR_INVALID, std::string(who) + ": NULL argument");
  return copy_and_wait(ctx, host, what == RM_MESH_PART_LABELS ? mesh->labels : mesh->sizes, bytes, hipMemcpyDeviceToHost);
}

// The keep rule, stated once: a component passes iff triangles >= min_triangles; with largest == 0 every passing one is kept, else the first
// `largest` of them in the order (triangles descending, component index ascending).  sizes: (vertices, triangles) pairs.
static std::vector<unsigned int> mesh_keep_mask(const std::vector<unsigned int>& sizes, const RmMeshKeep& k) {
  const size_t C = sizes.size() / 2;
  std::vector<unsigned int> keep(C, 0u), passing;
  for (size_t c = 0; c < C; c++)
    if ((unsigned long long)sizes[2 * c + 1] >= (unsigned long long)k.min_triangles) passing.push_back((unsigned int)c);
  if (k.largest > 0) {
    std::stable_sort(passing.begin(), passing.end(), [&](unsigned int a, unsigned int b) { return sizes[2 * (size_t)a + 1] > sizes[2 * (size_t)b + 1]; });
    if (passing.size() > (size_t)k.largest) passing.resize((size_t)k.largest);
  }
  for (unsigned int c : passing) keep[c] = 1u;
  return keep;
}

int rm_mesh_filter(rm_mesh* mesh, const RmMeshKeep* keep, rm_mesh** out) {
  const char* who = "rm_mesh_filter";
  rm_ctx* ctx = mesh ? mesh->ctx : nullptr;
  auto refuse = [&](const char* what) { return fail(ctx, RM_ERR_INVALID, std::string(who) + ": " + what); };
  RmMeshKeep k;
  rm_mesh_keep_default(&k);
  if (keep) k = *keep;
  if (k.min_triangles < 0) return refuse("keep min_triangles must be >= 0");
  if (k.largest < 0) return refuse("keep largest must be >= 0");
  if (k.reserved[0] != 0 || k.reserved[1] != 0) return refuse("keep reserved must be 0");
  if (!mesh || !out) return refuse("NULL argument");
  *out = nullptr;
  float ms = 0.0f;
  if (int rc = mesh_label(mesh, who, &ms)) return rc;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  rm_mesh* made = new (std::nothrow) rm_mesh;
  if (!made) return fail(ctx, RM_ERR_DEVICE, std::string(who) + ": out of host memory");
  made->ctx = ctx;
  for (int a = 0; a < 5; a++) made->has[a] = mesh->has[a];
  // everything below returns through here: a refused step gives the half-made mesh up (its arrays are still the MeshBuffers')
  auto build = [&]() -> int {
    const unsigned long long V = mesh->vertices, T = mesh->triangles, C = mesh->components;
    if (V == 0) return RM_OK;
    std::vector<unsigned int> sizes(2 * (size_t)C);
    if (int rc = copy_and_wait(ctx, sizes.data(), mesh->sizes, sizeof(unsigned int) * sizes.size(), hipMemcpyDeviceToHost)) return rc;
    const std::vector<unsigned int> mask = mesh_keep_mask(sizes, k);
    const size_t vertex_scratch = rm::rm_mesh_scan_scratch_elems((long long)V), triangle_scratch = rm::rm_mesh_scan_scratch_elems((long long)T);
    MeshBuffer d_keep, vertex_at, triangle_at, scratch, arrays[5];
    RM_HIP(ctx, d_keep.reserve(sizeof(unsigned int) * (size_t)C));
    RM_HIP(ctx, vertex_at.reserve(sizeof(unsigned long long) * (size_t)V));
    RM_HIP(ctx, triangle_at.reserve(sizeof(unsigned long long) * (size_t)T));
    RM_HIP(ctx, scratch.reserve(sizeof(unsigned long long) * (vertex_scratch + triangle_scratch + 2)));
    unsigned long long* d_totals = scratch.u64() + vertex_scratch + triangle_scratch;
    const unsigned int* labels = static_cast<const unsigned int*>(mesh->labels);
    const unsigned int* triangles = static_cast<const unsigned int*>(mesh->array[RM_MESH_TRIANGLES]);
    RM_HIP(ctx, hipMemcpyAsync(d_keep.p, mask.data(), sizeof(unsigned int) * (size_t)C, hipMemcpyHostToDevice, ctx->stream));
    RM_HIP(ctx, hipMemsetAsync(d_totals, 0, 2 * sizeof(unsigned long long), ctx->stream));  // (a mesh without triangles scans nothing)
    RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_FLAG));
    RM_HIP(ctx, rm::launch_mesh_keep_flags(labels, nullptr, d_keep.u32(), (long long)V, vertex_at.u64(), ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_scan(vertex_at.u64(), (long long)V, scratch.u64(), d_totals, ctx->stream));
    if (T > 0) {
      RM_HIP(ctx, rm::launch_mesh_keep_flags(labels, triangles, d_keep.u32(), (long long)T, triangle_at.u64(), ctx->stream));
      RM_HIP(ctx, rm::launch_mesh_scan(triangle_at.u64(), (long long)T, scratch.u64() + vertex_scratch, d_totals + 1, ctx->stream));
    }
    RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_FLAGGED));
    unsigned long long totals[2] = {0, 0};
    if (int rc = copy_and_wait(ctx, totals, d_totals, sizeof totals, hipMemcpyDeviceToHost)) return rc;  // (the mask's upload is done too)
    ms += mesh_between(ctx, MESH_MARK_FLAG, MESH_MARK_FLAGGED);
    made->vertices = totals[0];
    made->triangles = totals[1];
    if (made->vertices == 0) return RM_OK;
    rm::MeshGather G{};
    G.labels = labels;
    G.keep = d_keep.u32();
    G.vertex_at = vertex_at.u64();
    const int order[4] = {RM_MESH_POSITIONS, RM_MESH_NORMALS, RM_MESH_COLOURS, RM_MESH_CELLS};
    for (int a = 0; a < 4; a++) {
      const int what = order[a];
      if (!mesh->array[what]) continue;  // (absent; a mesh with vertices has the others)
      RM_HIP(ctx, arrays[what].reserve(mesh_array_bytes(made, what)));
      G.src[a] = static_cast<const unsigned int*>(mesh->array[what]);
      G.dst[a] = arrays[what].u32();
    }
    RM_HIP(ctx, arrays[RM_MESH_TRIANGLES].reserve(mesh_array_bytes(made, RM_MESH_TRIANGLES)));
    RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_GATHER));
    RM_HIP(ctx, rm::launch_mesh_gather_vertices(G, (long long)V, ctx->stream));
    if (made->triangles > 0)
      RM_HIP(ctx, rm::launch_mesh_gather_triangles(G, triangles, triangle_at.u64(), (long long)T, arrays[RM_MESH_TRIANGLES].u32(), ctx->stream));
    RM_HIP(ctx, mesh_mark(ctx, MESH_MARK_GATHERED));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ms += mesh_between(ctx, MESH_MARK_GATHER, MESH_MARK_GATHERED);
    for (int a = 0; a < 5; a++) made->array[a] = arrays[a].release();
    return RM_OK;
  };
  if (int rc = build()) {
    (void)hipStreamSynchronize(ctx->stream);  // (the scratch is freed behind whatever was enqueued)
    rm_mesh_destroy(made);
    return rc;
  }
  made->ms[1] = ms;
  *out = made;
  return RM_OK;
}
