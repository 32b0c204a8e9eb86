// ---- mesh extraction (include/hip_raymarch.h "mesh extraction"; kernels: rm_mesh_kernels.inc) ------------------------------------
// Included by rm_api.hip inside its extern "C" block, behind the probes.

enum { MESH_LABELS = 5, MESH_SIZES = 6, MESH_ARRAYS = 7 };  // rm_mesh_components' two arrays, behind the five of RM_MESH_* (rm_mesh_measure's result lives on the host)

struct rm_mesh {
  explicit rm_mesh(rm_ctx* of) : ctx(of) {}
  rm_ctx* const ctx;
  unsigned long long vertices = 0, triangles = 0;
  DeviceArray array[MESH_ARRAYS];                    // the mesh's own, freed with it (rm_mesh_destroy); NULL when absent or empty
  bool has[5] = {true, false, false, true, true};    // normals and colours: when rm_mesh_extract was asked for them
  float ms[3] = {0.0f, 0.0f, 0.0f};                  // rm_mesh_timings: sampling, meshing, attributes
  // rm_mesh_components' result, kept once made (the five arrays never change): V labels, `components` pairs of sizes
  bool labelled = false;
  unsigned long long components = 0;
  // rm_mesh_measure's result, kept once made for the same reason: the struct, and `components` rows of four counts
  bool measured = false;
  RmMeshMeasures measures{};
  std::vector<unsigned long long> edge_rows;
};

// A mesh under construction: given up through rm_mesh_destroy, which waits for the stream before it frees -- so the scratch of the call
// that gives it up (declared before the mesh, freed behind it) and the half-made arrays go behind whatever was enqueued.
// `*out = made.release()` hands a finished one over.
using MeshPtr = std::unique_ptr<rm_mesh, void (*)(rm_mesh*)>;

// a max / worst key of the reports, bits(value) << 32 | (0xFFFFFFFF - index), maximised: the value, and the lowest index that has it
static void mesh_key_decode(unsigned long long key, float* max, uint64_t* worst) {
  const unsigned int bits = (unsigned int)(key >> 32);
  std::memcpy(max, &bits, sizeof bits);
  *worst = 0xFFFFFFFFull - (key & 0xFFFFFFFFull);
}

// The fixed tree of sums over n > 0 values of each of two lists (rm_mesh_measure, rm_mesh_project, rm_mesh_deviation), 256 to a group: level k
// holds groups[k] values of each list, the last level one.  The levels of more than one value lie in scratch, one behind the other, a level's
// first list and then its second: `elems` values per list, 2 * elems doubles per tree.  The level of one value is two neighbouring words, `out`.
struct SumTree {
  long long groups[8];  // (256^8 = 2^64)
  size_t levels = 0, elems = 0;
  explicit SumTree(long long n) {
    for (long long g = (n + 255) / 256; n > 0; g = (g + 255) / 256) {
      groups[levels++] = g;
      if (g == 1) break;
      elems += (size_t)g;
    }
  }
  struct Lists { double *first, *second; };
  Lists level(size_t k, double* scratch, double* out) const {
    if (groups[k] == 1) return {out, out + 1};
    for (size_t j = 0; j < k; j++) scratch += 2 * groups[j];
    return {scratch, scratch + groups[k]};
  }
  // the lists (a, b) of n values each into level k, and on through every further level.  k = 0: from lists of the caller's own; k = 1: a
  // kernel of the caller's has written level 0 itself, at level(0, ...).
  hipError_t run(size_t k, const double* a, const double* b, long long n, double* scratch, double* out, hipStream_t stream) const {
    for (; k < levels; k++) {
      const Lists to = level(k, scratch, out);
      const hipError_t e = rm::launch_mesh_measure_sum(a, b, n, to.first, to.second, stream);
      if (e != hipSuccess) return e;
      a = to.first;
      b = to.second;
      n = groups[k];
    }
    return hipSuccess;
  }
};

static size_t mesh_array_bytes(const rm_mesh* m, int which) {
  if (which == MESH_SIZES) return (size_t)m->components * 8u;
  if (which == RM_MESH_TRIANGLES) return (size_t)m->triangles * 12u;
  return (size_t)m->vertices * (which == RM_MESH_CELLS || which == MESH_LABELS ? 4u : 12u);
}

// RmGrid's rule, and the grid as the kernels take it.  capped = false (the slabbed entries alone): without the bound on the corners, and then
// G->corners, which cannot hold them, is 0 -- those entries work on windows with corner counts of their own.
static int grid_check(const Refuse& refuse, const RmGrid* grid, GridDims* G, bool capped = true) {
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
  if (capped && corners > (1ll << 28)) return refuse("grid must have at most 2^28 corners");
  if (grid->reserved != 0) return refuse("grid reserved must be 0");
  G->corners = corners > (1ll << 28) ? 0 : (int)corners;
  return RM_OK;
}

static int sdf_flags_check(const Refuse& refuse, int flags) {
  if (flags & ~(RM_RENDER_FAST | RM_RENDER_NO_CULL)) return refuse("flags must be 0, RM_RENDER_FAST, RM_RENDER_NO_CULL or both");
  return RM_OK;
}

static int mesh_params_check(const Refuse& refuse, const RmMeshParams* in, RmMeshParams* p) {
  rm_mesh_params_default(p);
  if (in) *p = *in;
  if (!std::isfinite(p->iso)) return refuse("iso must be finite");
  if (p->normals != 0 && p->normals != 1) return refuse("normals must be 0 or 1");
  if (p->colours != 0 && p->colours != 1) return refuse("colours must be 0 or 1");
  if (p->normals && !(std::isfinite(p->normal_delta) && p->normal_delta > 0.0f)) return refuse("normal_delta must be finite and > 0");
  if (int rc = sdf_flags_check(refuse, p->flags)) return rc;
  if (p->reserved != 0) return refuse("reserved must be 0");
  return RM_OK;
}

int rm_grid_axis(const RmGrid* grid, int axis, float* out) {
  const Refuse refuse{nullptr, "rm_grid_axis"};
  GridDims G{};
  if (int rc = grid_check(refuse, grid, &G)) return rc;
  if (axis < 0 || axis > 2 || !out) return refuse("axis must be 0..2 and out non-NULL");
  for (int i = 0; i < G.nc[axis]; i++) out[i] = rm_grid_coord(G, axis, i);
  return RM_OK;
}

void rm_mesh_params_default(RmMeshParams* params) {
  if (!params) return;
  *params = RmMeshParams{0.0f, 1, 1e-5f, 0, 0, 0};
}

// the sampler on `stream`, with the culling grid obtained as every scene pass obtains it; plane0 > 0: G is a window of a grid's z planes that begins there
static int sdf_grid_enqueue(const Refuse& refuse, rm_scene* scene, const GridDims& G, int flags, float* d_out, hipStream_t stream, int plane0 = 0) {
  rm_ctx* ctx = refuse.ctx;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = scene_cull_grid(ctx, scene, flags, 1ll << 40)) return rc;
  const bool foreign = stream != ctx->stream;
  if (foreign && ctx->cull_event) RM_HIP(ctx, hipStreamWaitEvent(stream, ctx->cull_event, 0));  // (the grid is built on a stream of its own)
  const SdfGridParams P{scene_view(scene, flags), G, d_out, plane0};
  RM_HIP_AS(refuse, RM_SCENE_PASS(ctx, flags, launch_sdf_grid, P, stream));
  if (foreign) {
    // Everything that gives a scene's table or culling grid up -- rm_scene_destroy, the grids' budget (cull_release, cull_order) -- orders itself
    // behind the CONTEXT's stream: so that stream waits behind this launch, on the device, and the caller's stream needs no care of the host's.
    if (!ctx->mesh_order) RM_HIP(ctx, hipEventCreateWithFlags(&ctx->mesh_order, hipEventDisableTiming));
    RM_HIP(ctx, hipEventRecord(ctx->mesh_order, stream));
    RM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->mesh_order, 0));
  }
  return RM_OK;
}

static int sdf_grid_check(const Refuse& refuse, rm_scene* scene, const RmGrid* grid, int flags, const void* out, GridDims* G) {
  if (int rc = grid_check(refuse, grid, G)) return rc;
  if (int rc = sdf_flags_check(refuse, flags)) return rc;
  return scene_check(refuse, scene, out != nullptr);
}

int rm_sdf_grid_device(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, void* out_device, void* hip_stream) {
  const Refuse refuse{ctx, "rm_sdf_grid_device"};
  GridDims G{};
  if (int rc = sdf_grid_check(refuse, scene, grid, flags, out_device, &G)) return rc;
  if (reinterpret_cast<uintptr_t>(out_device) & 3u) return refuse("the output must be a 4-byte aligned device buffer");
  return sdf_grid_enqueue(refuse, scene, G, flags, static_cast<float*>(out_device), hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream);
}

int rm_sdf_grid(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, int flags, float* out_host) {
  const Refuse refuse{ctx, "rm_sdf_grid"};
  GridDims G{};
  if (int rc = sdf_grid_check(refuse, scene, grid, flags, out_host, &G)) return rc;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray values;
  RM_HIP(ctx, values.reserve(sizeof(float) * (size_t)G.corners));
  if (int rc = sdf_grid_enqueue(refuse, scene, G, flags, values.f32(), ctx->stream)) return rc;
  return copy_and_wait(ctx, out_host, values.p, sizeof(float) * (size_t)G.corners, hipMemcpyDeviceToHost);
}

// The mesher on d_values (on the context's stream): count, scan, read the totals, emit into the mesh's three arrays.  The counts and the
// scan's scratch go when this returns, behind its waits.
static int mesh_build(rm_ctx* ctx, const GridDims& G, const float* d_values, float iso, rm_mesh* mesh) {
  MeshSpans& spans = ctx->mesh_spans;
  const long long cells = (long long)(G.nc[0] - 1) * (G.nc[1] - 1) * (G.nc[2] - 1);
  const size_t scratch_elems = rm::rm_mesh_scan_scratch_elems(cells) + 1;  // ... and the total behind the levels
  DeviceArray counts, scratch;
  RM_HIP(ctx, counts.reserve(sizeof(unsigned long long) * (size_t)cells));
  RM_HIP(ctx, scratch.reserve(sizeof(unsigned long long) * scratch_elems));
  unsigned long long* d_total = scratch.u64() + (scratch_elems - 1);
  MeshParams P{G, d_values, iso, counts.u64(), nullptr, nullptr, nullptr};
  RM_HIP(ctx, spans.begin(MeshSpans::COUNT_SCAN, ctx->stream));  // (behind the sampler, or the upload of the caller's field)
  RM_HIP(ctx, rm::launch_mesh_count(P, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_scan(P.counts, cells, scratch.u64(), d_total, ctx->stream));
  RM_HIP(ctx, spans.end(MeshSpans::COUNT_SCAN, ctx->stream));
  unsigned long long total = 0;
  if (int rc = copy_and_wait(ctx, &total, d_total, sizeof total, hipMemcpyDeviceToHost)) return rc;
  mesh->vertices = total & 0xFFFFFFFFull;
  mesh->triangles = 2ull * (total >> 32);
  mesh->ms[1] = spans.ms(MeshSpans::COUNT_SCAN);
  if (mesh->vertices == 0) return RM_OK;
  for (int what : {RM_MESH_POSITIONS, RM_MESH_CELLS, RM_MESH_TRIANGLES}) RM_HIP(ctx, mesh->array[what].reserve(mesh_array_bytes(mesh, what)));
  P.positions = mesh->array[RM_MESH_POSITIONS].f32();
  P.cells = mesh->array[RM_MESH_CELLS].u32();
  P.triangles = mesh->array[RM_MESH_TRIANGLES].u32();
  RM_HIP(ctx, spans.begin(MeshSpans::EMIT, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_emit(P, ctx->stream));
  RM_HIP(ctx, spans.end(MeshSpans::EMIT, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mesh->ms[1] += spans.ms(MeshSpans::EMIT);
  return RM_OK;
}

void rm_mesh_destroy(rm_mesh* mesh) {
  if (!mesh) return;
  (void)hipSetDevice(mesh->ctx->device);
  (void)hipStreamSynchronize(mesh->ctx->stream);
  delete mesh;
}

int rm_mesh_from_values(rm_ctx* ctx, const RmGrid* grid, const float* values_host, float iso, rm_mesh** out) {
  const Refuse refuse{ctx, "rm_mesh_from_values"};
  GridDims G{};
  if (int rc = grid_check(refuse, grid, &G)) return rc;
  if (!std::isfinite(iso)) return refuse("iso must be finite");
  if (!ctx || !values_host || !out) return refuse("NULL argument");
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray values;
  RM_HIP(ctx, values.reserve(sizeof(float) * (size_t)G.corners));
  RM_HIP(ctx, hipMemcpyAsync(values.p, values_host, sizeof(float) * (size_t)G.corners, hipMemcpyHostToDevice, ctx->stream));
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  if (int rc = mesh_build(ctx, G, values.f32(), iso, made.get())) return rc;
  *out = made.release();
  return RM_OK;
}

// The arrays only a scene can give: the probe kernel (probe_enqueue, rm_probe's own launch) at the vertex positions.  Enqueued only: the
// caller waits for the stream once, and the material records are freed behind that wait.
static int mesh_attributes(rm_ctx* ctx, rm_scene* scene, const RmMeshParams& p, rm_mesh* mesh, DeviceArray& material) {
  const int n = (int)mesh->vertices;
  const float* positions = mesh->array[RM_MESH_POSITIONS].f32();
  DeviceArray& normals = mesh->array[RM_MESH_NORMALS];
  DeviceArray& colours = mesh->array[RM_MESH_COLOURS];
  if (p.normals) RM_HIP(ctx, normals.reserve(mesh_array_bytes(mesh, RM_MESH_NORMALS)));
  if (p.colours) {  // the probe writes 12 floats per point: the diffuse colour is the first three
    RM_HIP(ctx, colours.reserve(mesh_array_bytes(mesh, RM_MESH_COLOURS)));
    RM_HIP(ctx, material.reserve(sizeof(float) * 12u * (size_t)n));
  }
  RM_HIP(ctx, ctx->mesh_spans.begin(MeshSpans::ATTRIBUTES, ctx->stream));
  if (p.normals) RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, positions, normals.f32(), n, p.normal_delta, p.flags, ctx->stream));
  if (p.colours) {
    RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_MATERIAL, positions, material.f32(), n, 0.0f, p.flags, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_colours(material.f32(), colours.f32(), n, ctx->stream));
  }
  RM_HIP(ctx, ctx->mesh_spans.end(MeshSpans::ATTRIBUTES, ctx->stream));
  return RM_OK;
}

// Sharp vertices (the header's "sharp vertices"): the emitted mesh's positions become the QEF's.  Per vertex 12 slots of bracket, point and
// probe output, the caller's (SharpScratch, reserved for at least `count` vertices); the scene is evaluated by the probe kernel on the slot
// arrays, one launch per round and one for the normals.  Waits for the stream: the scratch may be freed, or used again, when this returns.
// The vertices are `count` from `first` on, and d_values begins at the grid's plane `plane0`: the whole mesh over the whole grid (0, 0,
// mesh->vertices), or one slab's run of vertices over its window (mesh_build_slabs).
struct SharpScratch {
  DeviceArray state, points, probed, live;
  hipError_t reserve(size_t vertices) {
    const size_t slots = 12u * vertices;
    hipError_t e = state.reserve(sizeof(float4) * slots);
    if (e == hipSuccess) e = points.reserve(sizeof(float) * 3u * slots);
    if (e == hipSuccess) e = probed.reserve(sizeof(float) * 3u * slots);
    if (e == hipSuccess) e = live.reserve(sizeof(unsigned int) * vertices);
    return e;
  }
};

static int mesh_sharp_fits(const Refuse& refuse, unsigned long long vertices) {
  if (vertices > (unsigned long long)INT_MAX / 12ull)
    return refuse("the mesh has more vertices than the probe's int count holds twelve slots of (12 V > INT_MAX)", RM_ERR_DEVICE);
  return RM_OK;
}

static int mesh_sharpen(const Refuse& refuse, rm_scene* scene, const GridDims& G, const float* d_values, int plane0, const RmMeshParams& p,
                        const RmMeshSharp& sharp, rm_mesh* mesh, unsigned long long first, unsigned long long count, const SharpScratch& tmp) {
  rm_ctx* ctx = refuse.ctx;
  const size_t slots = 12u * (size_t)count;
  const DeviceArray &points = tmp.points, &probed = tmp.probed;
  MeshSharpParams P{};
  P.mesh = MeshParams{G, d_values, p.iso, nullptr, mesh->array[RM_MESH_POSITIONS].f32() + 3u * (size_t)first, mesh->array[RM_MESH_CELLS].u32() + (size_t)first,
                      nullptr, plane0};
  P.vertices = (int)count;
  P.state = static_cast<float4*>(tmp.state.p);
  P.points = points.f32();
  P.probed = probed.f32();
  P.live = tmp.live.u32();
  P.threshold = sharp.threshold;
  RM_HIP(ctx, ctx->mesh_spans.begin(MeshSpans::SHARPEN, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_cross(P, 1, 0, sharp.refine == 0, ctx->stream));
  for (int round = 0; round < sharp.refine; round++) {
    RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_SDF, points.f32(), probed.f32(), (int)slots, 0.0f, p.flags, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_cross(P, 0, 1, round == sharp.refine - 1, ctx->stream));
  }
  RM_HIP(ctx, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, points.f32(), probed.f32(), (int)slots, sharp.normal_delta, p.flags, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_qef(P, ctx->stream));
  RM_HIP(ctx, ctx->mesh_spans.end(MeshSpans::SHARPEN, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mesh->ms[1] += ctx->mesh_spans.ms(MeshSpans::SHARPEN);
  return RM_OK;
}

void rm_mesh_sharp_default(RmMeshSharp* sharp) {
  if (!sharp) return;
  *sharp = RmMeshSharp{6, 0x1p-10f, 0.1f, 0};
}

static int mesh_sharp_check(const Refuse& refuse, const RmMeshSharp* in, RmMeshSharp* s) {
  rm_mesh_sharp_default(s);
  if (in) *s = *in;
  if (s->refine < 0 || s->refine > 16) return refuse("sharp refine must be in 0..16");
  if (!(std::isfinite(s->normal_delta) && s->normal_delta > 0.0f)) return refuse("sharp normal_delta must be finite and > 0");
  if (!(std::isfinite(s->threshold) && s->threshold >= 0.0f && s->threshold < 1.0f)) return refuse("sharp threshold must be finite and in [0, 1)");
  if (s->reserved != 0) return refuse("sharp reserved must be 0");
  return RM_OK;
}

// ---- slabbed extraction (include/hip_raymarch.h "slabbed extraction") ------------------------------------------------------------------

static const long long kMeshSlabWindow = 1ll << 26;  // the default budget of window corners (profiles/mesh_slabs.txt)

void rm_mesh_slabs_default(RmMeshSlabs* slabs) {
  if (!slabs) return;
  *slabs = RmMeshSlabs{0, 0};
}

// RmMeshSlabs' rule on a checked grid: *layers = the cell layers per slab, in 1..nz
static int mesh_slabs_check(const Refuse& refuse, const RmMeshSlabs* in, const GridDims& G, int* layers) {
  RmMeshSlabs s;
  rm_mesh_slabs_default(&s);
  if (in) s = *in;
  if (s.layers < 0) return refuse("slabs layers must be >= 0");
  if (s.reserved != 0) return refuse("slabs reserved must be 0");
  const long long plane = (long long)G.nc[0] * G.nc[1];
  const int nz = G.nc[2] - 1;
  long long L = s.layers;
  if (L == 0) L = kMeshSlabWindow / plane - 2;
  if (L < 1) L = 1;
  if (L > nz) L = nz;
  if ((L + 2) * plane > (1ll << 28)) return refuse("slab window (layers + 2) * (nx + 1) * (ny + 1) must be at most 2^28 corners");
  *layers = (int)L;
  return RM_OK;
}

// The slabbed mesher on the context's stream, into the mesh's three arrays: the tally pass over every slab, the totals read once, the emit
// pass over the slabs that have vertices, each sharpened behind its emit when `sharp` is given.  A window is filled by the sampler (scene) or
// from values_host; the planes two windows share are filled again, not kept.  Returns with the stream idle; mesh->ms[0] and ms[1] are the
// sums over the windows.  The window buffers are the caller's `tmp`, declared before the mesh.
struct SlabScratch {
  DeviceArray values, counts, levels, totals;
  SharpScratch sharp;
};

static int mesh_build_slabs(const Refuse& refuse, rm_scene* scene, const float* values_host, const GridDims& G, int L, const RmMeshParams& p,
                            const RmMeshSharp* sharp, SlabScratch& tmp, rm_mesh* mesh) {
  rm_ctx* ctx = refuse.ctx;
  MeshSpans& spans = ctx->mesh_spans;
  const int nz = G.nc[2] - 1, slabs = (nz + L - 1) / L;
  const size_t plane = (size_t)G.nc[0] * G.nc[1], layer = (size_t)(G.nc[0] - 1) * (G.nc[1] - 1);
  const int halo = slabs > 1 ? 1 : 0;  // (only a slab behind the first has one)
  const long long window_cells = (long long)(L + halo) * (long long)layer;
  const size_t level_elems = rm::rm_mesh_scan_scratch_elems(window_cells) + 1;  // ... and the scan's total behind the levels
  RM_HIP(ctx, tmp.values.reserve(sizeof(float) * (size_t)(L + halo + 1) * plane));
  RM_HIP(ctx, tmp.counts.reserve(sizeof(unsigned long long) * (size_t)window_cells));
  RM_HIP(ctx, tmp.levels.reserve(sizeof(unsigned long long) * level_elems));
  RM_HIP(ctx, tmp.totals.reserve(sizeof(unsigned long long) * (size_t)slabs));
  RM_HIP(ctx, hipMemsetAsync(tmp.totals.p, 0, sizeof(unsigned long long) * (size_t)slabs, ctx->stream));
  float* d_values = tmp.values.f32();
  unsigned long long* d_scan_total = tmp.levels.u64() + (level_elems - 1);

  // planes plane0 .. plane0 + planes - 1 into the window, in the SAMPLE span
  const auto fill = [&](int plane0, int planes) -> int {
    RM_HIP(ctx, spans.begin(MeshSpans::SAMPLE, ctx->stream));
    if (values_host) {
      RM_HIP(ctx, hipMemcpyAsync(d_values, values_host + (size_t)plane0 * plane, sizeof(float) * (size_t)planes * plane, hipMemcpyHostToDevice, ctx->stream));
    } else {
      GridDims W = G;
      W.nc[2] = planes;
      W.corners = (int)((size_t)planes * plane);
      if (int rc = sdf_grid_enqueue(refuse, scene, W, p.flags, d_values, ctx->stream, plane0)) return rc;
    }
    RM_HIP(ctx, spans.end(MeshSpans::SAMPLE, ctx->stream));
    return RM_OK;
  };

  MeshSlab S{};
  S.mesh = MeshParams{G, d_values, p.iso, nullptr, nullptr, nullptr, nullptr, 0};
  for (int s = 0; s < slabs; s++) {  // the tally pass: a slab's own planes are enough
    S.own0 = S.mesh.plane0 = s * L;
    S.layers = nz - S.own0 < L ? nz - S.own0 : L;
    S.total = tmp.totals.u64() + s;
    if (int rc = fill(S.own0, S.layers + 1)) return rc;
    RM_HIP(ctx, spans.begin(MeshSpans::COUNT_SCAN, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_slab_tally(S, ctx->stream));
    RM_HIP(ctx, spans.end(MeshSpans::COUNT_SCAN, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    mesh->ms[0] += spans.ms(MeshSpans::SAMPLE);
    mesh->ms[1] += spans.ms(MeshSpans::COUNT_SCAN);
  }
  std::vector<unsigned long long> totals((size_t)slabs);
  if (int rc = copy_and_wait(ctx, totals.data(), tmp.totals.p, sizeof(unsigned long long) * totals.size(), hipMemcpyDeviceToHost)) return rc;
  unsigned long long vertices = 0, quads = 0, most = 0;
  for (unsigned long long t : totals) {
    vertices += t & 0xFFFFFFFFull;
    quads += t >> 32;
    if ((t & 0xFFFFFFFFull) > most) most = t & 0xFFFFFFFFull;
  }
  mesh->vertices = vertices;
  mesh->triangles = 2ull * quads;
  if (vertices == 0) return RM_OK;
  if (sharp) {
    if (int rc = mesh_sharp_fits(refuse, most)) return rc;  // (per slab: a slab's vertices are one run of the probe)
    RM_HIP(ctx, tmp.sharp.reserve((size_t)most));
  }
  for (int what : {RM_MESH_POSITIONS, RM_MESH_CELLS, RM_MESH_TRIANGLES}) RM_HIP(ctx, mesh->array[what].reserve(mesh_array_bytes(mesh, what)));
  S.mesh.counts = tmp.counts.u64();
  S.mesh.positions = mesh->array[RM_MESH_POSITIONS].f32();
  S.mesh.cells = mesh->array[RM_MESH_CELLS].u32();
  S.mesh.triangles = mesh->array[RM_MESH_TRIANGLES].u32();
  S.total = nullptr;
  S.vertex_base = S.quad_base = 0;
  for (int s = 0; s < slabs; s++) {  // the emit pass
    const unsigned long long own_vertices = totals[(size_t)s] & 0xFFFFFFFFull, own_quads = totals[(size_t)s] >> 32;
    if (own_vertices == 0) continue;  // (and no quads: the cell that owns one is active)
    S.own0 = s * L;
    S.mesh.plane0 = S.own0 > 0 ? S.own0 - 1 : 0;
    S.layers = nz - S.own0 < L ? nz - S.own0 : L;
    const int layers = S.own0 - S.mesh.plane0 + S.layers;  // (with the halo)
    if (int rc = fill(S.mesh.plane0, layers + 1)) return rc;
    RM_HIP(ctx, spans.begin(MeshSpans::COUNT_SCAN, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_slab_count(S, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_scan(S.mesh.counts, (long long)layers * (long long)layer, tmp.levels.u64(), d_scan_total, ctx->stream));
    RM_HIP(ctx, spans.end(MeshSpans::COUNT_SCAN, ctx->stream));
    // The emit writes at the tally's bases: what the scan counted of the slab's own cells has to be what the tally counted, or nothing is written.
    unsigned long long all = 0, before = 0;
    if (int rc = copy_and_wait(ctx, &all, d_scan_total, sizeof all, hipMemcpyDeviceToHost)) return rc;
    if (int rc = copy_and_wait(ctx, &before, S.mesh.counts + (size_t)(S.own0 - S.mesh.plane0) * layer, sizeof before, hipMemcpyDeviceToHost)) return rc;
    if (all - before != totals[(size_t)s]) return refuse("the two samplings of a slab disagree", RM_ERR_DEVICE);
    RM_HIP(ctx, spans.begin(MeshSpans::EMIT, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_slab_emit(S, ctx->stream));
    RM_HIP(ctx, spans.end(MeshSpans::EMIT, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    mesh->ms[0] += spans.ms(MeshSpans::SAMPLE);
    mesh->ms[1] += spans.ms(MeshSpans::COUNT_SCAN) + spans.ms(MeshSpans::EMIT);
    if (sharp)
      if (int rc = mesh_sharpen(refuse, scene, G, d_values, S.mesh.plane0, p, *sharp, mesh, S.vertex_base, own_vertices, tmp.sharp)) return rc;
    S.vertex_base += own_vertices;
    S.quad_base += own_quads;
  }
  return RM_OK;
}

// rm_mesh_extract and rm_mesh_extract_sharp, and with `slabbed` rm_mesh_extract_slabs and rm_mesh_extract_sharp_slabs.  `sharpen` tells the
// sharp ones apart; `sharp` and `slabs` (NULL = the defaults) are looked at only with their flags.  Slabbed: the grid's corners are not
// bounded, the slabs' check stands behind the others', and mesh_build_slabs samples, meshes and sharpens window by window.
static int mesh_extract(const Refuse& refuse, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, bool sharpen, const RmMeshSharp* sharp,
                        bool slabbed, const RmMeshSlabs* slabs, rm_mesh** out) {
  rm_ctx* ctx = refuse.ctx;
  GridDims G{};
  RmMeshParams p;
  RmMeshSharp s{};
  int layers = 0;
  if (int rc = grid_check(refuse, grid, &G, !slabbed)) return rc;
  if (int rc = mesh_params_check(refuse, params, &p)) return rc;
  if (sharpen)
    if (int rc = mesh_sharp_check(refuse, sharp, &s)) return rc;
  if (slabbed)
    if (int rc = mesh_slabs_check(refuse, slabs, G, &layers)) return rc;
  if (int rc = scene_check(refuse, scene, out != nullptr)) return rc;
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  SlabScratch tmp;  // (before the mesh: freed behind the wait of whatever gives the mesh up, or the one below); unslabbed: its values and sharp alone
  DeviceArray material;
  if (!slabbed) {
    RM_HIP(ctx, tmp.values.reserve(sizeof(float) * (size_t)G.corners));
    RM_HIP(ctx, ctx->mesh_spans.begin(MeshSpans::SAMPLE, ctx->stream));
    if (int rc = sdf_grid_enqueue(refuse, scene, G, p.flags, tmp.values.f32(), ctx->stream)) return rc;
    RM_HIP(ctx, ctx->mesh_spans.end(MeshSpans::SAMPLE, ctx->stream));
  }
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  made->has[RM_MESH_NORMALS] = p.normals != 0;
  made->has[RM_MESH_COLOURS] = p.colours != 0;
  if (slabbed) {
    if (int rc = mesh_build_slabs(refuse, scene, nullptr, G, layers, p, sharpen ? &s : nullptr, tmp, made.get())) return rc;
  } else {
    if (int rc = mesh_build(ctx, G, tmp.values.f32(), p.iso, made.get())) return rc;
    if (sharpen && made->vertices > 0) {
      if (int rc = mesh_sharp_fits(refuse, made->vertices)) return rc;
      RM_HIP(ctx, tmp.sharp.reserve((size_t)made->vertices));
      if (int rc = mesh_sharpen(refuse, scene, G, tmp.values.f32(), 0, p, s, made.get(), 0, made->vertices, tmp.sharp)) return rc;
    }
  }
  const bool attributes = made->vertices > 0 && (p.normals || p.colours);
  if (attributes)
    if (int rc = mesh_attributes(ctx, scene, p, made.get(), material)) return rc;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return refuse("the stream failed", RM_ERR_DEVICE);
  if (!slabbed) made->ms[0] = ctx->mesh_spans.ms(MeshSpans::SAMPLE);  // (slabbed: mesh_build_slabs has summed its windows')
  if (attributes) made->ms[2] = ctx->mesh_spans.ms(MeshSpans::ATTRIBUTES);
  *out = made.release();
  return RM_OK;
}

int rm_mesh_extract(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, rm_mesh** out) {
  return mesh_extract(Refuse{ctx, "rm_mesh_extract"}, scene, grid, params, false, nullptr, false, nullptr, out);
}

int rm_mesh_extract_sharp(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSharp* sharp, rm_mesh** out) {
  return mesh_extract(Refuse{ctx, "rm_mesh_extract_sharp"}, scene, grid, params, true, sharp, false, nullptr, out);
}

int rm_mesh_extract_slabs(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSlabs* slabs, rm_mesh** out) {
  return mesh_extract(Refuse{ctx, "rm_mesh_extract_slabs"}, scene, grid, params, false, nullptr, true, slabs, out);
}

int rm_mesh_extract_sharp_slabs(rm_ctx* ctx, rm_scene* scene, const RmGrid* grid, const RmMeshParams* params, const RmMeshSharp* sharp,
                                const RmMeshSlabs* slabs, rm_mesh** out) {
  return mesh_extract(Refuse{ctx, "rm_mesh_extract_sharp_slabs"}, scene, grid, params, true, sharp, true, slabs, out);
}

int rm_mesh_from_values_slabs(rm_ctx* ctx, const RmGrid* grid, const float* values_host, float iso, const RmMeshSlabs* slabs, rm_mesh** out) {
  const Refuse refuse{ctx, "rm_mesh_from_values_slabs"};
  GridDims G{};
  int layers = 0;
  if (int rc = grid_check(refuse, grid, &G, false)) return rc;
  if (!std::isfinite(iso)) return refuse("iso must be finite");
  if (int rc = mesh_slabs_check(refuse, slabs, G, &layers)) return rc;
  if (!ctx || !values_host || !out) return refuse("NULL argument");
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  RmMeshParams p;
  rm_mesh_params_default(&p);
  p.iso = iso;
  SlabScratch tmp;
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  if (int rc = mesh_build_slabs(refuse, nullptr, values_host, G, layers, p, nullptr, tmp, made.get())) return rc;
  *out = made.release();
  return RM_OK;
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

// the exact-size copy-out of the download entries: one of the mesh's seven arrays, whole
static int mesh_copy_out(const Refuse& refuse, rm_mesh* mesh, int which, void* host, size_t bytes) {
  rm_ctx* ctx = mesh->ctx;
  if (bytes != (mesh->array[which].p ? mesh_array_bytes(mesh, which) : 0u)) return refuse("bytes must be the array's exact size");
  if (bytes == 0) return RM_OK;
  if (!host) return refuse("NULL argument");
  RM_HIP(ctx, hipSetDevice(ctx->device));
  return copy_and_wait(ctx, host, mesh->array[which].p, bytes, hipMemcpyDeviceToHost);
}

int rm_mesh_download(rm_mesh* mesh, int what, void* host, size_t bytes) {
  const Refuse refuse{mesh ? mesh->ctx : nullptr, "rm_mesh_download"};
  if (!mesh) return refuse("NULL mesh");
  if (what < RM_MESH_POSITIONS || what > RM_MESH_CELLS) return refuse("unknown array");
  if (!mesh->has[what]) return refuse("the mesh was made without this array");
  return mesh_copy_out(refuse, mesh, what, host, bytes);
}

void* rm_mesh_device_ptr(rm_mesh* mesh, int what) {
  if (!mesh || what < RM_MESH_POSITIONS || what > RM_MESH_CELLS) return nullptr;
  return mesh->array[what].p;
}

// ---- components and islands (include/hip_raymarch.h "components and islands") --------------------------------------------------------

void rm_mesh_keep_default(RmMeshKeep* keep) {
  if (!keep) return;
  *keep = RmMeshKeep{1, 0, {0, 0}};
}

// The labelling, once per mesh: a forest over the vertices by rounds of hook + flatten until a hook pass met no two roots, the roots numbered
// by the scan, the sizes counted.  On the context's stream; waits for it.  *ms (when given) gains the time of its span if it ran.
static int mesh_label(const Refuse& refuse, rm_mesh* mesh, float* ms) {
  if (mesh->labelled) return RM_OK;
  rm_ctx* ctx = mesh->ctx;
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  if (T >= (1ull << 32)) return refuse("the mesh has more triangles than a uint32 size holds (T >= 2^32)", RM_ERR_DEVICE);
  RM_HIP(ctx, hipSetDevice(ctx->device));
  if (V == 0) {
    mesh->labelled = true;
    return RM_OK;
  }
  const size_t scratch_elems = rm::rm_mesh_scan_scratch_elems((long long)V) + 2;  // ... the total, and the word the hook pass sets, behind the levels
  DeviceArray parent, words, scratch;
  DeviceArray &labels = mesh->array[MESH_LABELS], &sizes = mesh->array[MESH_SIZES];  // (read only once `labelled` says they are whole)
  RM_HIP(ctx, parent.reserve(sizeof(unsigned int) * (size_t)V));
  RM_HIP(ctx, words.reserve(sizeof(unsigned long long) * (size_t)V));
  RM_HIP(ctx, scratch.reserve(sizeof(unsigned long long) * scratch_elems));
  RM_HIP(ctx, labels.reserve(sizeof(unsigned int) * (size_t)V));
  unsigned long long* d_total = scratch.u64() + (scratch_elems - 2);
  unsigned int* d_changed = reinterpret_cast<unsigned int*>(scratch.u64() + (scratch_elems - 1));
  const unsigned int* triangles = mesh->array[RM_MESH_TRIANGLES].u32();
  RM_HIP(ctx, ctx->mesh_spans.begin(MeshSpans::LABEL, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_link_init(parent.u32(), (long long)V, ctx->stream));
  const int max_rounds = 64;
  int round = 0;
  for (unsigned int changed = T > 0 ? 1u : 0u; changed != 0u; round++) {
    if (round == max_rounds) return refuse("the labelling did not converge in 64 rounds", RM_ERR_DEVICE);
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
  RM_HIP(ctx, ctx->mesh_spans.end(MeshSpans::LABEL, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ms) *ms += ctx->mesh_spans.ms(MeshSpans::LABEL);
  mesh->components = total;
  mesh->labelled = true;
  return RM_OK;
}

int rm_mesh_components(rm_mesh* mesh, unsigned long long* out_count) {
  const Refuse refuse{mesh ? mesh->ctx : nullptr, "rm_mesh_components"};
  if (!mesh || !out_count) return refuse("NULL argument");
  if (int rc = mesh_label(refuse, mesh, nullptr)) return rc;
  *out_count = mesh->components;
  return RM_OK;
}

int rm_mesh_components_download(rm_mesh* mesh, int what, void* host, size_t bytes) {
  const Refuse refuse{mesh ? mesh->ctx : nullptr, "rm_mesh_components_download"};
  if (!mesh) return refuse("NULL argument");
  if (what != RM_MESH_PART_LABELS && what != RM_MESH_PART_SIZES) return refuse("unknown array");
  if (int rc = mesh_label(refuse, mesh, nullptr)) return rc;
  return mesh_copy_out(refuse, mesh, what == RM_MESH_PART_LABELS ? MESH_LABELS : MESH_SIZES, host, bytes);
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

// The kept components of a labelled `mesh` with vertices, gathered into `made`: the keep mask up, flags and scans, the totals to the host,
// the gathers into made's own arrays.  *ms gains the time of its two spans.  The scratch goes when this returns: behind its last wait, or,
// where a step is refused, behind the wait of whoever gives `made` up.
static int mesh_gather_kept(const rm_mesh* mesh, const RmMeshKeep& k, rm_mesh* made, float* ms) {
  rm_ctx* ctx = mesh->ctx;
  MeshSpans& spans = ctx->mesh_spans;
  const unsigned long long V = mesh->vertices, T = mesh->triangles, C = mesh->components;
  std::vector<unsigned int> sizes(2 * (size_t)C);
  if (int rc = copy_and_wait(ctx, sizes.data(), mesh->array[MESH_SIZES].p, sizeof(unsigned int) * sizes.size(), hipMemcpyDeviceToHost)) return rc;
  const std::vector<unsigned int> mask = mesh_keep_mask(sizes, k);
  const size_t vertex_scratch = rm::rm_mesh_scan_scratch_elems((long long)V), triangle_scratch = rm::rm_mesh_scan_scratch_elems((long long)T);
  DeviceArray d_keep, vertex_at, triangle_at, scratch;
  RM_HIP(ctx, d_keep.reserve(sizeof(unsigned int) * (size_t)C));
  RM_HIP(ctx, vertex_at.reserve(sizeof(unsigned long long) * (size_t)V));
  RM_HIP(ctx, triangle_at.reserve(sizeof(unsigned long long) * (size_t)T));
  RM_HIP(ctx, scratch.reserve(sizeof(unsigned long long) * (vertex_scratch + triangle_scratch + 2)));
  unsigned long long* d_totals = scratch.u64() + vertex_scratch + triangle_scratch;
  const unsigned int* labels = mesh->array[MESH_LABELS].u32();
  const unsigned int* triangles = mesh->array[RM_MESH_TRIANGLES].u32();
  RM_HIP(ctx, hipMemcpyAsync(d_keep.p, mask.data(), sizeof(unsigned int) * (size_t)C, hipMemcpyHostToDevice, ctx->stream));
  RM_HIP(ctx, hipMemsetAsync(d_totals, 0, 2 * sizeof(unsigned long long), ctx->stream));  // (a mesh without triangles scans nothing)
  RM_HIP(ctx, spans.begin(MeshSpans::KEEP_FLAGS, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_keep_flags(labels, nullptr, d_keep.u32(), (long long)V, vertex_at.u64(), ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_scan(vertex_at.u64(), (long long)V, scratch.u64(), d_totals, ctx->stream));
  if (T > 0) {
    RM_HIP(ctx, rm::launch_mesh_keep_flags(labels, triangles, d_keep.u32(), (long long)T, triangle_at.u64(), ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_scan(triangle_at.u64(), (long long)T, scratch.u64() + vertex_scratch, d_totals + 1, ctx->stream));
  }
  RM_HIP(ctx, spans.end(MeshSpans::KEEP_FLAGS, ctx->stream));
  unsigned long long totals[2] = {0, 0};
  if (int rc = copy_and_wait(ctx, totals, d_totals, sizeof totals, hipMemcpyDeviceToHost)) return rc;  // (the mask's upload is done too)
  *ms += spans.ms(MeshSpans::KEEP_FLAGS);
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
    if (!mesh->array[what].p) continue;  // (absent; a mesh with vertices has the others)
    RM_HIP(ctx, made->array[what].reserve(mesh_array_bytes(made, what)));
    G.src[a] = mesh->array[what].u32();
    G.dst[a] = made->array[what].u32();
  }
  RM_HIP(ctx, made->array[RM_MESH_TRIANGLES].reserve(mesh_array_bytes(made, RM_MESH_TRIANGLES)));
  RM_HIP(ctx, spans.begin(MeshSpans::GATHER, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_gather_vertices(G, (long long)V, ctx->stream));
  if (made->triangles > 0)
    RM_HIP(ctx, rm::launch_mesh_gather_triangles(G, triangles, triangle_at.u64(), (long long)T, made->array[RM_MESH_TRIANGLES].u32(), ctx->stream));
  RM_HIP(ctx, spans.end(MeshSpans::GATHER, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *ms += spans.ms(MeshSpans::GATHER);
  return RM_OK;
}

int rm_mesh_filter(rm_mesh* mesh, const RmMeshKeep* keep, rm_mesh** out) {
  rm_ctx* ctx = mesh ? mesh->ctx : nullptr;
  const Refuse refuse{ctx, "rm_mesh_filter"};
  RmMeshKeep k;
  rm_mesh_keep_default(&k);
  if (keep) k = *keep;
  if (k.min_triangles < 0) return refuse("keep min_triangles must be >= 0");
  if (k.largest < 0) return refuse("keep largest must be >= 0");
  if (k.reserved[0] != 0 || k.reserved[1] != 0) return refuse("keep reserved must be 0");
  if (!mesh || !out) return refuse("NULL argument");
  *out = nullptr;
  float ms = 0.0f;
  if (int rc = mesh_label(refuse, mesh, &ms)) return rc;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  for (int a = 0; a < 5; a++) made->has[a] = mesh->has[a];
  if (mesh->vertices > 0)
    if (int rc = mesh_gather_kept(mesh, k, made.get(), &ms)) return rc;
  made->ms[1] = ms;
  *out = made.release();
  return RM_OK;
}

// ---- simplification (include/hip_raymarch.h "simplification") -----------------------------------------------------------------------------

void rm_mesh_simplify_default(RmMeshSimplify* params) {
  if (!params) return;
  *params = RmMeshSimplify{0, {0, 0, 0}};
}

// what a simplification needs beside its result: owned by rm_mesh_simplify, declared before the mesh it makes
struct SimplifyScratch {
  DeviceArray marks, levels, sums, vertex_to, mapped, words, table, quadrics;
};

// `mesh` (with vertices) clustered on G into `made`: number the occupied clusters, read V'; sum, place, map and deduplicate, read T' and the
// error word; gather.  On the context's stream; returns with it idle.  made->ms[1] is the time of its three spans.  quadric (NULL: the cluster
// means stay): behind the place kernel, inside its span, the source triangles' plane quadrics are summed per cluster and the positions of the
// output vertices that have planes are moved to the minimisers (rm_mesh_simplify_quadric).
static int mesh_cluster(const Refuse& refuse, const rm_mesh* mesh, const GridDims& G, bool keep_duplicates, const RmMeshQuadric* quadric,
                        SimplifyScratch& tmp, rm_mesh* made) {
  rm_ctx* ctx = mesh->ctx;
  MeshSpans& spans = ctx->mesh_spans;
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  const long long cells = (long long)(G.nc[0] - 1) * (G.nc[1] - 1) * (G.nc[2] - 1);
  const size_t cell_levels = rm::rm_mesh_scan_scratch_elems(cells), triangle_levels = rm::rm_mesh_scan_scratch_elems((long long)T + 1);
  RM_HIP(ctx, tmp.marks.reserve(sizeof(unsigned long long) * (size_t)cells));
  RM_HIP(ctx, tmp.levels.reserve(sizeof(unsigned long long) * (cell_levels + triangle_levels + 3)));  // ... V', T' and the error word behind the levels
  unsigned long long* d_totals = tmp.levels.u64() + cell_levels + triangle_levels;
  rm::MeshQuadric S{};  // (the simplification's own fields, and the placement's behind them)
  S.grid = G;
  S.vertices = (long long)V;
  S.triangles = (long long)T;
  S.positions = mesh->array[RM_MESH_POSITIONS].f32();
  S.normals = mesh->array[RM_MESH_NORMALS].f32();
  S.colours = mesh->array[RM_MESH_COLOURS].f32();
  S.source_triangles = mesh->array[RM_MESH_TRIANGLES].u32();
  S.marks = tmp.marks.u64();
  S.error = reinterpret_cast<unsigned int*>(d_totals + 2);
  RM_HIP(ctx, spans.begin(MeshSpans::CLUSTER_NUMBER, ctx->stream));
  RM_HIP(ctx, hipMemsetAsync(tmp.marks.p, 0, sizeof(unsigned long long) * (size_t)cells, ctx->stream));
  RM_HIP(ctx, hipMemsetAsync(d_totals, 0, 3 * sizeof(unsigned long long), ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_simplify_mark(S, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_scan(S.marks, cells, tmp.levels.u64(), d_totals, ctx->stream));
  RM_HIP(ctx, spans.end(MeshSpans::CLUSTER_NUMBER, ctx->stream));
  unsigned long long totals[3] = {0, 0, 0};
  if (int rc = copy_and_wait(ctx, totals, d_totals, sizeof totals[0], hipMemcpyDeviceToHost)) return rc;
  float ms = spans.ms(MeshSpans::CLUSTER_NUMBER);
  made->vertices = totals[0];
  S.out_vertices = (long long)made->vertices;
  S.row = 4 + (S.normals ? 3 : 0) + (S.colours ? 3 : 0);
  const size_t sums_bytes = sizeof(unsigned long long) * (size_t)S.row * (size_t)made->vertices;
  RM_HIP(ctx, tmp.sums.reserve(sums_bytes));
  RM_HIP(ctx, tmp.vertex_to.reserve(sizeof(unsigned int) * (size_t)V));
  for (int what : {RM_MESH_POSITIONS, RM_MESH_NORMALS, RM_MESH_COLOURS, RM_MESH_CELLS})
    if (mesh->array[what].p) RM_HIP(ctx, made->array[what].reserve(mesh_array_bytes(made, what)));
  S.sums = tmp.sums.u64();
  S.vertex_to = tmp.vertex_to.u32();
  S.out_positions = made->array[RM_MESH_POSITIONS].f32();
  S.out_normals = made->array[RM_MESH_NORMALS].f32();
  S.out_colours = made->array[RM_MESH_COLOURS].f32();
  S.out_cells = made->array[RM_MESH_CELLS].u32();
  if (T > 0) {
    RM_HIP(ctx, tmp.mapped.reserve(sizeof(unsigned int) * 3u * (size_t)T));
    RM_HIP(ctx, tmp.words.reserve(sizeof(unsigned long long) * ((size_t)T + 1)));
    S.mapped = tmp.mapped.u32();
    S.words = tmp.words.u64();
    if (!keep_duplicates) {
      S.slots = 1ull;
      while (S.slots < 2ull * T) S.slots <<= 1;
      RM_HIP(ctx, tmp.table.reserve(sizeof(unsigned int) * (size_t)S.slots));
      S.table = tmp.table.u32();
    }
  }
  const bool planes = quadric != nullptr && T > 0 && made->vertices > 0;
  const size_t quadrics_bytes = sizeof(unsigned long long) * 10u * (size_t)made->vertices;
  if (planes) {
    RM_HIP(ctx, tmp.quadrics.reserve(quadrics_bytes));
    S.quadrics = tmp.quadrics.u64();
    float hmax = G.h[0];
    if (G.h[1] > hmax) hmax = G.h[1];
    if (G.h[2] > hmax) hmax = G.h[2];
    for (int a = 0; a < 3; a++) S.scale[a] = G.h[a] / hmax;
    S.threshold = quadric->threshold;
  }
  RM_HIP(ctx, spans.begin(MeshSpans::CLUSTER_MERGE, ctx->stream));
  RM_HIP(ctx, hipMemsetAsync(tmp.sums.p, 0, sums_bytes, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_simplify_sums(S, ctx->stream));
  RM_HIP(ctx, rm::launch_mesh_simplify_place(S, ctx->stream));
  if (planes) {
    RM_HIP(ctx, hipMemsetAsync(tmp.quadrics.p, 0, quadrics_bytes, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_quadric_sums(S, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_quadric_place(S, ctx->stream));
  }
  if (T > 0) {
    RM_HIP(ctx, rm::launch_mesh_simplify_map(S, ctx->stream));
    if (!keep_duplicates) {
      RM_HIP(ctx, hipMemsetAsync(tmp.table.p, 0xFF, sizeof(unsigned int) * (size_t)S.slots, ctx->stream));
      RM_HIP(ctx, rm::launch_mesh_simplify_insert(S, ctx->stream));
      RM_HIP(ctx, rm::launch_mesh_simplify_keep(S, ctx->stream));
    }
    RM_HIP(ctx, rm::launch_mesh_scan(S.words, (long long)T + 1, tmp.levels.u64() + cell_levels, d_totals + 1, ctx->stream));
  }
  RM_HIP(ctx, spans.end(MeshSpans::CLUSTER_MERGE, ctx->stream));
  if (int rc = copy_and_wait(ctx, totals + 1, d_totals + 1, 2 * sizeof totals[0], hipMemcpyDeviceToHost)) return rc;
  ms += spans.ms(MeshSpans::CLUSTER_MERGE);
  if ((unsigned int)totals[2] != 0u) return refuse("a triangle found no slot in the table", RM_ERR_DEVICE);
  made->triangles = totals[1];
  if (made->triangles > 0) {
    RM_HIP(ctx, made->array[RM_MESH_TRIANGLES].reserve(mesh_array_bytes(made, RM_MESH_TRIANGLES)));
    S.out_triangles = made->array[RM_MESH_TRIANGLES].u32();
    RM_HIP(ctx, spans.begin(MeshSpans::CLUSTER_GATHER, ctx->stream));
    RM_HIP(ctx, rm::launch_mesh_simplify_gather(S, ctx->stream));
    RM_HIP(ctx, spans.end(MeshSpans::CLUSTER_GATHER, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ms += spans.ms(MeshSpans::CLUSTER_GATHER);
  }
  made->ms[1] = ms;
  return RM_OK;
}

// rm_mesh_simplify (quadric NULL and unasked) and rm_mesh_simplify_quadric (asked; a NULL block is the defaults): one path, the checks in the
// header's order
static int mesh_simplify_entry(const char* who, rm_mesh* mesh, const RmGrid* clusters, const RmMeshSimplify* params, bool asked,
                               const RmMeshQuadric* quadric, rm_mesh** out) {
  rm_ctx* ctx = mesh ? mesh->ctx : nullptr;
  const Refuse refuse{ctx, who};
  GridDims G{};
  RmMeshSimplify p;
  rm_mesh_simplify_default(&p);
  if (params) p = *params;
  RmMeshQuadric q;
  rm_mesh_quadric_default(&q);
  if (quadric) q = *quadric;
  if (int rc = grid_check(refuse, clusters, &G)) return rc;
  if (p.keep_duplicates != 0 && p.keep_duplicates != 1) return refuse("keep_duplicates must be 0 or 1");
  if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return refuse("simplify reserved must be 0");
  if (asked) {
    if (!(std::isfinite(q.threshold) && q.threshold >= 0.0f && q.threshold < 1.0f)) return refuse("quadric threshold must be finite and in [0, 1)");
    if (q.reserved[0] != 0 || q.reserved[1] != 0 || q.reserved[2] != 0) return refuse("quadric reserved must be 0");
  }
  if (!mesh || !out) return refuse("NULL argument");
  *out = nullptr;
  if (mesh->triangles >= (1ull << 32)) return refuse("the mesh has more triangles than a uint32 index holds (T >= 2^32)", RM_ERR_DEVICE);
  RM_HIP(ctx, hipSetDevice(ctx->device));
  SimplifyScratch tmp;  // (before the mesh: freed behind the wait of whatever gives the mesh up)
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  for (int a = 0; a < 5; a++) made->has[a] = mesh->has[a];
  if (mesh->vertices > 0)
    if (int rc = mesh_cluster(refuse, mesh, G, p.keep_duplicates != 0, asked ? &q : nullptr, tmp, made.get())) return rc;
  *out = made.release();
  return RM_OK;
}

int rm_mesh_simplify(rm_mesh* mesh, const RmGrid* clusters, const RmMeshSimplify* params, rm_mesh** out) {
  return mesh_simplify_entry("rm_mesh_simplify", mesh, clusters, params, false, nullptr, out);
}

// ---- quadric placement (include/hip_raymarch.h "quadric placement") ---------------------------------------------------------------------------

void rm_mesh_quadric_default(RmMeshQuadric* q) {
  if (!q) return;
  *q = RmMeshQuadric{0.1f, {0, 0, 0}};
}

int rm_mesh_simplify_quadric(rm_mesh* mesh, const RmGrid* clusters, const RmMeshSimplify* params, const RmMeshQuadric* quadric, rm_mesh** out) {
  return mesh_simplify_entry("rm_mesh_simplify_quadric", mesh, clusters, params, true, quadric, out);
}

// ---- ambient occlusion (include/hip_raymarch.h "ambient occlusion") ----------------------------------------------------------------------------

void rm_mesh_occlusion_default(RmMeshOcclusion* params) {
  if (!params) return;
  *params = RmMeshOcclusion{0.25f, 16, 4, 0x1p-10f, 1.0f, 0, {0, 0}};
}

// log2 of a power of two in 1..limit, -1 for anything else
static int occlusion_log2(int n, int limit) {
  for (int l = 0; (1 << l) <= limit; l++)
    if (n == (1 << l)) return l;
  return -1;
}

// the table in double, every output rounded once (the header's "direction table")
static void occlusion_directions(int K, float* out) {
  const double golden = M_PI * (3.0 - std::sqrt(5.0));
  for (int k = 0; k < K; k++) {
    const double u = ((double)k + 0.5) / (double)K;
    const double phi = (double)k * golden;
    const double r = std::sqrt(u);
    const float z = (float)std::sqrt(1.0 - u);
    out[4 * k] = (float)(r * std::cos(phi));
    out[4 * k + 1] = (float)(r * std::sin(phi));
    out[4 * k + 2] = z;
    out[4 * k + 3] = (float)(1.0 / (double)z);
  }
}

int rm_mesh_occlusion_directions(int directions, float* out) {
  const Refuse refuse{nullptr, "rm_mesh_occlusion_directions"};
  if (occlusion_log2(directions, 64) < 0) return refuse("directions must be 1, 2, 4, 8, 16, 32 or 64");
  if (!out) return refuse("NULL argument");
  occlusion_directions(directions, out);
  return RM_OK;
}

static int mesh_occlusion_check(const Refuse& refuse, const RmMeshOcclusion* in, RmMeshOcclusion* p) {
  rm_mesh_occlusion_default(p);
  if (in) *p = *in;
  if (!(std::isfinite(p->radius) && p->radius >= 0x1p-64f && p->radius <= 0x1p64f)) return refuse("occlusion radius must be finite and in [2^-64, 2^64]");
  if (occlusion_log2(p->directions, 64) < 0) return refuse("occlusion directions must be 1, 2, 4, 8, 16, 32 or 64");
  if (occlusion_log2(p->taps, 8) < 0) return refuse("occlusion taps must be 1, 2, 4 or 8");
  if (!(std::isfinite(p->normal_delta) && p->normal_delta > 0.0f)) return refuse("occlusion normal_delta must be finite and > 0");
  if (!(std::isfinite(p->strength) && p->strength >= 0.0f && p->strength <= 4.0f)) return refuse("occlusion strength must be finite and in [0, 4]");
  if (int rc = sdf_flags_check(refuse, p->flags)) return rc;
  if (p->reserved[0] != 0 || p->reserved[1] != 0) return refuse("occlusion reserved must be 0");
  return RM_OK;
}

int rm_mesh_occlusion(rm_mesh* mesh, rm_scene* scene, const RmMeshOcclusion* params, float* out_host, float* out_ms2) {
  rm_ctx* ctx = mesh ? mesh->ctx : nullptr;
  const Refuse refuse{ctx, "rm_mesh_occlusion"};
  RmMeshOcclusion p;
  if (int rc = mesh_occlusion_check(refuse, params, &p)) return rc;
  if (int rc = scene_check(refuse, scene, out_host != nullptr)) return rc;  // (a NULL mesh is a NULL context there)
  if (out_ms2) out_ms2[0] = out_ms2[1] = 0.0f;
  if (mesh->vertices == 0) return RM_OK;
  const int log2_k = occlusion_log2(p.directions, 64), log2_j = occlusion_log2(p.taps, 8);
  if ((mesh->vertices << log2_k) >= (1ull << 31))
    return refuse("the mesh has more vertices than the kernel's index holds rays of (V * directions >= 2^31)", RM_ERR_DEVICE);
  const size_t V = (size_t)mesh->vertices;
  float table[64 * 4];
  occlusion_directions(p.directions, table);
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray normals, d0, directions, ao;  // (freed behind the wait of the copy below; a call that fails before it leaves that wait to hipFree)
  RM_HIP_AS(refuse, normals.reserve(sizeof(float) * 3u * V));
  RM_HIP_AS(refuse, d0.reserve(sizeof(float) * V));
  RM_HIP_AS(refuse, directions.reserve(sizeof(float) * 4u * (size_t)p.directions));
  RM_HIP_AS(refuse, ao.reserve(sizeof(float) * V));
  if (int rc = scene_cull_grid(ctx, scene, p.flags, 1ll << 40)) return rc;
  const float* positions = mesh->array[RM_MESH_POSITIONS].f32();
  MeshOcclusionPass P{};
  P.scene = scene_view(scene, p.flags);
  P.positions = positions;
  P.normals = normals.f32();
  P.d0 = d0.f32();
  P.directions = static_cast<const float4*>(directions.p);
  P.out = ao.f32();
  P.vertices = (int)V;
  P.log2_directions = log2_k;
  P.taps = p.taps;
  P.radius = p.radius;
  P.inv_radius = 1.0f / p.radius;
  P.strength = p.strength;
  P.scale = std::ldexp(1.0f, -(16 + log2_k + log2_j));
  MeshSpans& spans = ctx->mesh_spans;
  RM_HIP_AS(refuse, hipMemcpyAsync(directions.p, table, sizeof(float) * 4u * (size_t)p.directions, hipMemcpyHostToDevice, ctx->stream));
  RM_HIP_AS(refuse, spans.begin(MeshSpans::OCCLUSION_PROBES, ctx->stream));
  RM_HIP_AS(refuse, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, positions, normals.f32(), (int)V, p.normal_delta, p.flags, ctx->stream));
  RM_HIP_AS(refuse, probe_enqueue(ctx, scene, RM_PROBE_SDF, positions, d0.f32(), (int)V, 0.0f, p.flags, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::OCCLUSION_PROBES, ctx->stream));
  RM_HIP_AS(refuse, spans.begin(MeshSpans::OCCLUSION_TAPS, ctx->stream));
  RM_HIP_AS(refuse, RM_SCENE_PASS(ctx, p.flags, launch_mesh_occlusion, P, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::OCCLUSION_TAPS, ctx->stream));
  if (int rc = copy_and_wait(ctx, out_host, ao.p, sizeof(float) * V, hipMemcpyDeviceToHost)) return rc;
  if (out_ms2) {
    out_ms2[0] = spans.ms(MeshSpans::OCCLUSION_PROBES);
    out_ms2[1] = spans.ms(MeshSpans::OCCLUSION_TAPS);
  }
  return RM_OK;
}

// ---- measures and edge topology (include/hip_raymarch.h "measures and edge topology") ----------------------------------------------------------

// a coordinate out of the extent kernel's code, with the header's + 0.0f
static float measure_extent_float(unsigned int code) {
  const unsigned int bits = (code & 0x80000000u) ? (code & 0x7FFFFFFFu) : ~code;
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f + 0.0f;
}

// The measures, once per mesh: the labelling if the mesh has none, the edge table, its classes and the used vertices; the extent, the terms
// and the levels of their tree.  Everything is allocated before the first launch; on the context's stream, and waits for it: the scratch goes
// when this returns.  ms2 (when given): the two spans' milliseconds, {0, 0} when the stored result stands.
static int mesh_measure(const Refuse& refuse, rm_mesh* mesh, float* ms2) {
  if (ms2) ms2[0] = ms2[1] = 0.0f;
  if (mesh->measured) return RM_OK;
  rm_ctx* ctx = mesh->ctx;
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  if (T >= (1ull << 32)) return refuse("the mesh has more triangles than a uint32 count holds (T >= 2^32)", RM_ERR_DEVICE);
  float ms[2] = {0.0f, 0.0f};
  if (int rc = mesh_label(refuse, mesh, &ms[0])) return rc;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned long long C = mesh->components;
  RmMeshMeasures m{};
  m.vertices = V;
  m.triangles = T;
  m.components = C;
  std::vector<unsigned long long> rows;
  if (V == 0) {
    m.skipped_triangles = T;  // (no index is < 0 vertices)
  } else {
    if (!host_staging(rows, 4 * (size_t)C)) return refuse("out of host memory", RM_ERR_DEVICE);
    unsigned long long slots = 0;
    if (T > 0)
      for (slots = 1ull; slots < 4ull * T; slots <<= 1) {}
    const SumTree tree((long long)T);  // of area and volume: the terms kernel writes level 0, the level of one value is the totals' own two words
    DeviceArray keys, counts, used, totals, d_rows, levels;
    RM_HIP_AS(refuse, keys.reserve(sizeof(unsigned long long) * (size_t)slots));
    RM_HIP_AS(refuse, counts.reserve(sizeof(unsigned long long) * (size_t)slots));
    RM_HIP_AS(refuse, used.reserve(sizeof(unsigned int) * (size_t)V));
    RM_HIP_AS(refuse, totals.reserve(sizeof(unsigned long long) * rm::RM_MEASURE_WORDS));
    RM_HIP_AS(refuse, d_rows.reserve(sizeof(unsigned long long) * 4u * (size_t)C));
    RM_HIP_AS(refuse, levels.reserve(sizeof(double) * 2u * tree.elems));
    unsigned long long first[rm::RM_MEASURE_WORDS] = {};
    const unsigned int identities[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    std::memcpy(first + rm::RM_MEASURE_EXTENT, identities, sizeof identities);
    rm::MeshMeasure M{};
    M.vertices = (long long)V;
    M.triangles = (long long)T;
    M.positions = mesh->array[RM_MESH_POSITIONS].f32();
    M.corners = mesh->array[RM_MESH_TRIANGLES].u32();
    M.labels = mesh->array[MESH_LABELS].u32();
    M.keys = keys.u64();
    M.counts = counts.u64();
    M.slots = slots;
    M.used = used.u32();
    M.totals = totals.u64();
    M.rows = d_rows.u64();
    static_assert(rm::RM_MEASURE_VOLUME == rm::RM_MEASURE_AREA + 1, "the tree's two sums are neighbours");
    double* const d_sums = reinterpret_cast<double*>(M.totals + rm::RM_MEASURE_AREA);
    MeshSpans& spans = ctx->mesh_spans;
    RM_HIP_AS(refuse, hipMemcpyAsync(totals.p, first, sizeof first, hipMemcpyHostToDevice, ctx->stream));
    RM_HIP_AS(refuse, spans.begin(MeshSpans::MEASURE_TOPOLOGY, ctx->stream));
    RM_HIP_AS(refuse, hipMemsetAsync(used.p, 0, sizeof(unsigned int) * (size_t)V, ctx->stream));
    RM_HIP_AS(refuse, hipMemsetAsync(d_rows.p, 0, sizeof(unsigned long long) * 4u * (size_t)C, ctx->stream));
    if (T > 0) {
      RM_HIP_AS(refuse, hipMemsetAsync(keys.p, 0xFF, sizeof(unsigned long long) * (size_t)slots, ctx->stream));
      RM_HIP_AS(refuse, hipMemsetAsync(counts.p, 0, sizeof(unsigned long long) * (size_t)slots, ctx->stream));
      RM_HIP_AS(refuse, rm::launch_mesh_measure_edges(M, ctx->stream));
      RM_HIP_AS(refuse, rm::launch_mesh_measure_classes(M, ctx->stream));
    }
    RM_HIP_AS(refuse, rm::launch_mesh_measure_used(M, ctx->stream));
    RM_HIP_AS(refuse, spans.end(MeshSpans::MEASURE_TOPOLOGY, ctx->stream));
    RM_HIP_AS(refuse, spans.begin(MeshSpans::MEASURE_GEOMETRY, ctx->stream));
    RM_HIP_AS(refuse, rm::launch_mesh_measure_extent(M, ctx->stream));
    if (T > 0) {
      const SumTree::Lists terms = tree.level(0, static_cast<double*>(levels.p), d_sums);
      RM_HIP_AS(refuse, rm::launch_mesh_measure_terms(M, terms.first, terms.second, ctx->stream));
      RM_HIP_AS(refuse, tree.run(1, terms.first, terms.second, tree.groups[0], static_cast<double*>(levels.p), d_sums, ctx->stream));
    }
    RM_HIP_AS(refuse, spans.end(MeshSpans::MEASURE_GEOMETRY, ctx->stream));
    unsigned long long got[rm::RM_MEASURE_WORDS] = {};
    if (C > 0)
      if (int rc = copy_and_wait(ctx, rows.data(), d_rows.p, sizeof(unsigned long long) * rows.size(), hipMemcpyDeviceToHost)) return rc;
    if (int rc = copy_and_wait(ctx, got, totals.p, sizeof got, hipMemcpyDeviceToHost)) return rc;
    ms[0] += spans.ms(MeshSpans::MEASURE_TOPOLOGY);
    ms[1] = spans.ms(MeshSpans::MEASURE_GEOMETRY);
    if (got[rm::RM_MEASURE_ERROR] != 0ull) return refuse("an edge found no slot in the table", RM_ERR_DEVICE);
    m.skipped_triangles = got[rm::RM_MEASURE_SKIPPED];
    m.used_vertices = got[rm::RM_MEASURE_USED];
    m.unmeasured_triangles = got[rm::RM_MEASURE_UNMEASURED];
    m.finite_vertices = got[rm::RM_MEASURE_FINITE];
    m.edges = got[rm::RM_MEASURE_EDGES];
    m.boundary_edges = got[rm::RM_MEASURE_BOUNDARY];
    m.regular_edges = got[rm::RM_MEASURE_REGULAR];
    m.irregular_edges = got[rm::RM_MEASURE_IRREGULAR];
    m.unbalanced_edges = got[rm::RM_MEASURE_UNBALANCED];
    std::memcpy(&m.area, got + rm::RM_MEASURE_AREA, sizeof m.area);
    std::memcpy(&m.volume, got + rm::RM_MEASURE_VOLUME, sizeof m.volume);
    if (m.finite_vertices > 0) {
      unsigned int extent[6];
      std::memcpy(extent, got + rm::RM_MEASURE_EXTENT, sizeof extent);
      for (int a = 0; a < 3; a++) {
        m.lo[a] = measure_extent_float(extent[a]);
        m.hi[a] = measure_extent_float(extent[3 + a]);
      }
    }
  }
  const unsigned long long P = T - m.skipped_triangles;
  m.euler = (long long)m.used_vertices - (long long)m.edges + (long long)P;
  m.closed = P >= 1 && m.boundary_edges == 0 && m.irregular_edges == 0 ? 1 : 0;
  for (size_t c = 0; c < rows.size() / 4; c++)
    if (rows[4 * c] > 0 && rows[4 * c + 1] == 0 && rows[4 * c + 2] == 0) m.closed_components++;
  mesh->measures = m;
  mesh->edge_rows = std::move(rows);
  mesh->measured = true;
  if (ms2) { ms2[0] = ms[0]; ms2[1] = ms[1]; }
  return RM_OK;
}

int rm_mesh_measure(rm_mesh* mesh, RmMeshMeasures* out, float* out_ms2) {
  const Refuse refuse{mesh ? mesh->ctx : nullptr, "rm_mesh_measure"};
  if (!mesh || !out) return refuse("NULL argument");
  if (int rc = mesh_measure(refuse, mesh, out_ms2)) return rc;
  *out = mesh->measures;
  return RM_OK;
}

int rm_mesh_measure_components(rm_mesh* mesh, void* host, size_t bytes) {
  const Refuse refuse{mesh ? mesh->ctx : nullptr, "rm_mesh_measure_components"};
  if (!mesh) return refuse("NULL argument");
  if (int rc = mesh_measure(refuse, mesh, nullptr)) return rc;
  if (bytes != sizeof(unsigned long long) * mesh->edge_rows.size()) return refuse("bytes must be the rows' exact size (32 per component)");
  if (bytes == 0) return RM_OK;
  if (!host) return refuse("NULL argument");
  std::memcpy(host, mesh->edge_rows.data(), bytes);
  return RM_OK;
}

// ---- projection onto the surface (include/hip_raymarch.h "projection onto the surface") -----------------------------------------------------------

void rm_mesh_project_default(RmMeshProject* params) {
  if (!params) return;
  *params = RmMeshProject{0.0f, 4, 1.0f, 0.0f, 0.0f, 0x1p-10f, 0, 0};
}

static int mesh_project_check(const Refuse& refuse, const RmMeshProject* in, RmMeshProject* p) {
  rm_mesh_project_default(p);
  if (in) *p = *in;
  if (!std::isfinite(p->iso)) return refuse("project iso must be finite");
  if (p->rounds < 1 || p->rounds > 16) return refuse("project rounds must be in 1..16");
  if (!(std::isfinite(p->relax) && p->relax > 0.0f && p->relax <= 1.0f)) return refuse("project relax must be finite and in (0, 1]");
  if (!(std::isfinite(p->tolerance) && p->tolerance >= 0.0f)) return refuse("project tolerance must be finite and >= 0");
  if (!(std::isfinite(p->reach) && p->reach >= 0.0f)) return refuse("project reach must be finite and >= 0");
  if (!(std::isfinite(p->normal_delta) && p->normal_delta > 0.0f)) return refuse("project normal_delta must be finite and > 0");
  if (int rc = sdf_flags_check(refuse, p->flags)) return rc;
  if (p->reserved != 0) return refuse("project reserved must be 0");
  return RM_OK;
}

// The projection of a checked block on checked handles, for rm_mesh_project and for rm_mesh_refine's rounds (`refuse` names the entry).
// probe_normals = false (the rounds: the normals are probed once, at the end of that call): the result has no RM_MESH_NORMALS array yet.
static int mesh_project_run(const Refuse& refuse, rm_mesh* mesh, rm_scene* scene, const RmMeshProject& p, bool probe_normals, rm_mesh** out,
                            RmMeshProjection* report, float* residual_host) {
  rm_ctx* ctx = mesh->ctx;
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  if (V > (unsigned long long)INT_MAX) return refuse("the mesh has more vertices than the kernels' int index holds (V > INT_MAX)", RM_ERR_DEVICE);
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray d, normals, flags, residual, totals, levels;  // (before the mesh: freed behind the wait of whatever gives the mesh up, or the last one below)
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  for (int a = 0; a < 5; a++) made->has[a] = mesh->has[a];
  RmMeshProjection r{};
  if (V == 0) {
    if (report) *report = r;
    *out = made.release();
    return RM_OK;
  }
  made->vertices = V;
  made->triangles = T;
  const SumTree tree((long long)V);  // of a report half's two sums: the step kernel writes level 0
  for (int what : {RM_MESH_POSITIONS, RM_MESH_NORMALS, RM_MESH_COLOURS, RM_MESH_TRIANGLES, RM_MESH_CELLS})
    if (mesh->array[what].p && (probe_normals || what != RM_MESH_NORMALS)) RM_HIP_AS(refuse, made->array[what].reserve(mesh_array_bytes(made.get(), what)));
  RM_HIP_AS(refuse, d.reserve(sizeof(float) * (size_t)V));
  RM_HIP_AS(refuse, normals.reserve(sizeof(float) * 3u * (size_t)V));
  RM_HIP_AS(refuse, flags.reserve(sizeof(unsigned int) * (size_t)V));
  RM_HIP_AS(refuse, residual.reserve(sizeof(float) * (size_t)V));
  RM_HIP_AS(refuse, totals.reserve(sizeof(unsigned long long) * rm::RM_PROJECT_WORDS));
  RM_HIP_AS(refuse, levels.reserve(sizeof(double) * 2u * tree.elems));
  if (int rc = scene_cull_grid(ctx, scene, p.flags, 1ll << 40)) return rc;
  for (int what : {RM_MESH_POSITIONS, RM_MESH_COLOURS, RM_MESH_TRIANGLES, RM_MESH_CELLS})
    if (mesh->array[what].p)
      RM_HIP_AS(refuse, hipMemcpyAsync(made->array[what].p, mesh->array[what].p, mesh_array_bytes(made.get(), what), hipMemcpyDeviceToDevice, ctx->stream));
  float* positions = made->array[RM_MESH_POSITIONS].f32();
  MeshProjectEval E{};
  E.scene = scene_view(scene, p.flags);
  E.positions = positions;
  E.d = d.f32();
  E.normals = normals.f32();
  E.vertices = (int)V;
  E.iso = p.iso;
  E.tolerance = p.tolerance;
  E.normal_delta = p.normal_delta;
  rm::MeshProject S{};
  S.vertices = (long long)V;
  S.triangles = (long long)T;
  S.source = mesh->array[RM_MESH_POSITIONS].f32();
  S.positions = positions;
  S.d = d.f32();
  S.normals = normals.f32();
  S.residual = residual.f32();
  S.flags = flags.u32();
  S.corners = made->array[RM_MESH_TRIANGLES].u32();
  S.totals = totals.u64();
  S.iso = p.iso;
  S.relax = p.relax;
  S.tolerance = p.tolerance;
  S.reach = p.reach;
  // a half of the report: the step kernel's first level, then the further levels into the half's two words of the totals
  const auto report_half = [&](int round, int word) -> int {
    double* const d_sums = reinterpret_cast<double*>(S.totals + word);
    const SumTree::Lists sums = tree.level(0, static_cast<double*>(levels.p), d_sums);
    RM_HIP_AS(refuse, rm::launch_mesh_project_step(S, round, sums.first, sums.second, ctx->stream));
    RM_HIP_AS(refuse, tree.run(1, sums.first, sums.second, tree.groups[0], static_cast<double*>(levels.p), d_sums, ctx->stream));
    return RM_OK;
  };
  MeshSpans& spans = ctx->mesh_spans;
  RM_HIP_AS(refuse, hipMemsetAsync(totals.p, 0, sizeof(unsigned long long) * rm::RM_PROJECT_WORDS, ctx->stream));
  RM_HIP_AS(refuse, hipMemsetAsync(flags.p, 0, sizeof(unsigned int) * (size_t)V, ctx->stream));
  RM_HIP_AS(refuse, spans.begin(MeshSpans::PROJECT_ROUNDS, ctx->stream));
  unsigned long long moved = 0;
  int rounds_run = 0;
  for (int round = 0; round < p.rounds; round++) {
    RM_HIP_AS(refuse, RM_SCENE_PASS(ctx, p.flags, launch_mesh_project_eval, E, ctx->stream));
    if (round == 0) {
      if (int rc = report_half(0, rm::RM_PROJECT_SUM_BEFORE)) return rc;
    } else {
      RM_HIP_AS(refuse, rm::launch_mesh_project_step(S, round, nullptr, nullptr, ctx->stream));
    }
    rounds_run = round + 1;
    if (int rc = copy_and_wait(ctx, &moved, S.totals + rm::RM_PROJECT_MOVED + round, sizeof moved, hipMemcpyDeviceToHost)) return rc;
    if (moved == 0) break;  // (every later round would repeat this one)
  }
  // the residual after: where the last round moved nobody, d is already the distance at the final positions
  if (moved != 0) RM_HIP_AS(refuse, probe_enqueue(ctx, scene, RM_PROBE_SDF, positions, d.f32(), (int)V, 0.0f, p.flags, ctx->stream));
  if (int rc = report_half(-1, rm::RM_PROJECT_SUM_AFTER)) return rc;
  RM_HIP_AS(refuse, rm::launch_mesh_project_flips(S, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::PROJECT_ROUNDS, ctx->stream));
  const bool with_normals = made->array[RM_MESH_NORMALS].p != nullptr;
  if (with_normals) {
    RM_HIP_AS(refuse, spans.begin(MeshSpans::PROJECT_NORMALS, ctx->stream));
    RM_HIP_AS(refuse, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, positions, made->array[RM_MESH_NORMALS].f32(), (int)V, p.normal_delta, p.flags, ctx->stream));
    RM_HIP_AS(refuse, spans.end(MeshSpans::PROJECT_NORMALS, ctx->stream));
  }
  unsigned long long got[rm::RM_PROJECT_WORDS] = {};
  std::vector<float> e_after;
  if (residual_host) {  // (through a buffer of the call's own: a refusal below writes nothing of the caller's)
    if (!host_staging(e_after, (size_t)V)) return refuse("out of host memory", RM_ERR_DEVICE);
    RM_HIP_AS(refuse, hipMemcpyAsync(e_after.data(), residual.p, sizeof(float) * (size_t)V, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (int rc = copy_and_wait(ctx, got, totals.p, sizeof got, hipMemcpyDeviceToHost)) return rc;
  made->ms[1] = spans.ms(MeshSpans::PROJECT_ROUNDS);
  if (with_normals) made->ms[2] = spans.ms(MeshSpans::PROJECT_NORMALS);
  r.vertices = V;
  r.triangles = T;
  r.moved_vertices = got[rm::RM_PROJECT_MOVED_VERTICES];
  r.settled_before = got[rm::RM_PROJECT_SETTLED_BEFORE];
  r.settled_after = got[rm::RM_PROJECT_SETTLED_AFTER];
  r.nonfinite_before = got[rm::RM_PROJECT_NONFINITE_BEFORE];
  r.nonfinite_after = got[rm::RM_PROJECT_NONFINITE_AFTER];
  r.clamped_vertices = got[rm::RM_PROJECT_CLAMPED];
  r.undirected_vertices = got[rm::RM_PROJECT_UNDIRECTED];
  r.flipped_triangles = got[rm::RM_PROJECT_FLIPPED];
  r.rounds_run = rounds_run;
  const auto half = [&](int key_word, int sum_word, unsigned long long nonfinite, uint64_t* worst, float* max, double* mean, double* rms) {
    const unsigned long long key = got[key_word], count = V - nonfinite;
    if (key == 0ull || count == 0ull) return;  // no finite e: everything stays 0
    mesh_key_decode(key, max, worst);
    double sum, sum2;
    std::memcpy(&sum, got + sum_word, sizeof sum);
    std::memcpy(&sum2, got + sum_word + 1, sizeof sum2);
    *mean = sum / (double)count;
    *rms = std::sqrt(sum2 / (double)count);
  };
  half(rm::RM_PROJECT_KEY_BEFORE, rm::RM_PROJECT_SUM_BEFORE, r.nonfinite_before, &r.worst_before, &r.max_before, &r.mean_before, &r.rms_before);
  half(rm::RM_PROJECT_KEY_AFTER, rm::RM_PROJECT_SUM_AFTER, r.nonfinite_after, &r.worst_after, &r.max_after, &r.mean_after, &r.rms_after);
  if (report) *report = r;
  if (residual_host) std::memcpy(residual_host, e_after.data(), sizeof(float) * (size_t)V);
  *out = made.release();
  return RM_OK;
}

int rm_mesh_project(rm_mesh* mesh, rm_scene* scene, const RmMeshProject* params, rm_mesh** out, RmMeshProjection* report, float* residual_host) {
  const Refuse refuse{mesh ? mesh->ctx : nullptr, "rm_mesh_project"};
  RmMeshProject p;
  if (int rc = mesh_project_check(refuse, params, &p)) return rc;
  if (int rc = scene_check(refuse, scene, out != nullptr)) return rc;  // (a NULL mesh is a NULL context there)
  return mesh_project_run(refuse, mesh, scene, p, true, out, report, residual_host);
}

// ---- deviation (include/hip_raymarch.h "deviation") ------------------------------------------------------------------------------------------------

void rm_mesh_deviation_default(RmMeshDeviation* params) {
  if (!params) return;
  *params = RmMeshDeviation{0.0f, 4, 0.0f, 0, {0, 0, 0, 0}};
}

// log2 of the samples per triangle, S = order * order, for an order of 1, 2, 4 or 8; -1 for anything else
static int deviation_log2_samples(int order) {
  for (int l = 0; l <= 3; l++)
    if (order == (1 << l)) return 2 * l;
  return -1;
}

// the table in double, every weight rounded once (the header's "sample table")
static void deviation_weights(int n, float* out) {
  const double denominator = (double)(3 * n);
  for (int s = 0, r = 0; s < n * n; s++) {
    if ((r + 1) * (r + 1) <= s) r++;  // r = floor(sqrt(s))
    const int c = s - r * r, m = c / 2;
    const int A = (c & 1) ? 3 * (r - m) - 1 : 3 * (r - m) + 1;
    const int B = (c & 1) ? 3 * m + 2 : 3 * m + 1;
    out[4 * s] = (float)((double)(3 * n - A - B) / denominator);
    out[4 * s + 1] = (float)((double)A / denominator);
    out[4 * s + 2] = (float)((double)B / denominator);
    out[4 * s + 3] = 0.0f;
  }
}

int rm_mesh_deviation_weights(int order, float* out) {
  const Refuse refuse{nullptr, "rm_mesh_deviation_weights"};
  if (deviation_log2_samples(order) < 0) return refuse("order must be 1, 2, 4 or 8");
  if (!out) return refuse("NULL argument");
  deviation_weights(order, out);
  return RM_OK;
}

static int mesh_deviation_check(const Refuse& refuse, const RmMeshDeviation* in, RmMeshDeviation* p) {
  rm_mesh_deviation_default(p);
  if (in) *p = *in;
  if (!std::isfinite(p->iso)) return refuse("deviation iso must be finite");
  if (deviation_log2_samples(p->order) < 0) return refuse("deviation order must be 1, 2, 4 or 8");
  if (!(std::isfinite(p->tolerance) && p->tolerance >= 0.0f)) return refuse("deviation tolerance must be finite and >= 0");
  if (int rc = sdf_flags_check(refuse, p->flags)) return rc;
  for (int r : p->reserved)
    if (r != 0) return refuse("deviation reserved must be 0");
  return RM_OK;
}

int rm_mesh_deviation(rm_mesh* mesh, rm_scene* scene, const RmMeshDeviation* params, RmMeshDeviationReport* report, float* triangles_host, float* out_ms2) {
  rm_ctx* ctx = mesh ? mesh->ctx : nullptr;
  const Refuse refuse{ctx, "rm_mesh_deviation"};
  RmMeshDeviation p;
  if (int rc = mesh_deviation_check(refuse, params, &p)) return rc;
  if (int rc = scene_check(refuse, scene, true)) return rc;  // (a NULL mesh is a NULL context there)
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  const int log2_s = deviation_log2_samples(p.order), S = 1 << log2_s;
  RmMeshDeviationReport r{};
  r.vertices = V;
  r.triangles = T;
  r.samples = S;
  if (V == 0 || T == 0) {
    if (V == 0) r.skipped_triangles = T;  // (no index is < 0 vertices)
    if (report) *report = r;
    if (out_ms2) out_ms2[0] = out_ms2[1] = 0.0f;
    return RM_OK;
  }
  if (T >= (1ull << (31 - log2_s)))
    return refuse("the mesh has more triangles than the kernels' index holds samples of (T * S >= 2^31)", RM_ERR_DEVICE);
  float table[64 * 4];
  deviation_weights(p.order, table);
  const SumTree tree((long long)T);  // of each of the two pairs of terms, from the reducer's lists on
  std::vector<float> max_host;
  if (triangles_host) {  // (through a buffer of the call's own: a refusal below writes nothing of the caller's)
    if (!host_staging(max_host, (size_t)T)) return refuse("out of host memory", RM_ERR_DEVICE);
  }
  RM_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray d, weights, triangle_max, terms, levels, totals;  // (freed behind the wait of the copy below; a call that fails before it leaves that wait to hipFree)
  RM_HIP_AS(refuse, d.reserve(sizeof(float) * ((size_t)T << log2_s)));
  RM_HIP_AS(refuse, weights.reserve(sizeof(float) * 4u * (size_t)S));
  RM_HIP_AS(refuse, triangle_max.reserve(sizeof(float) * (size_t)T));
  RM_HIP_AS(refuse, terms.reserve(sizeof(double) * 4u * (size_t)T));
  RM_HIP_AS(refuse, levels.reserve(sizeof(double) * 4u * tree.elems));
  constexpr size_t kTotalsWords = (size_t)rm::RM_DEVIATION_COPIES * rm::RM_DEVIATION_WORDS;
  RM_HIP_AS(refuse, totals.reserve(sizeof(unsigned long long) * kTotalsWords));
  if (int rc = scene_cull_grid(ctx, scene, p.flags, 1ll << 40)) return rc;
  MeshDeviationSdf E{};
  E.scene = scene_view(scene, p.flags);
  E.positions = mesh->array[RM_MESH_POSITIONS].f32();
  E.corners = mesh->array[RM_MESH_TRIANGLES].u32();
  E.weights = static_cast<const float4*>(weights.p);
  E.d = d.f32();
  E.vertices = (long long)V;
  E.triangles = (int)T;
  E.log2_samples = log2_s;
  rm::MeshDeviation D{};
  D.vertices = (long long)V;
  D.triangles = (int)T;
  D.log2_samples = log2_s;
  D.positions = E.positions;
  D.corners = E.corners;
  D.d = d.f32();
  D.triangle_max = triangle_max.f32();
  D.terms = static_cast<double*>(terms.p);
  D.totals = totals.u64();
  D.iso = p.iso;
  D.tolerance = p.tolerance;
  // one pair of the reducer's lists through every level of the tree, into two neighbouring words of copy 0 of the totals
  const auto sum_pair = [&](int pair, int word) {
    return tree.run(0, D.terms + 2 * (size_t)pair * (size_t)T, D.terms + (2 * (size_t)pair + 1) * (size_t)T, (long long)T,
                    static_cast<double*>(levels.p) + 2 * (size_t)pair * tree.elems, reinterpret_cast<double*>(D.totals + word), ctx->stream);
  };
  MeshSpans& spans = ctx->mesh_spans;
  RM_HIP_AS(refuse, hipMemcpyAsync(weights.p, table, sizeof(float) * 4u * (size_t)S, hipMemcpyHostToDevice, ctx->stream));
  RM_HIP_AS(refuse, hipMemsetAsync(totals.p, 0, sizeof(unsigned long long) * kTotalsWords, ctx->stream));
  RM_HIP_AS(refuse, spans.begin(MeshSpans::DEVIATION_EVALUATE, ctx->stream));
  RM_HIP_AS(refuse, RM_SCENE_PASS(ctx, p.flags, launch_mesh_deviation_eval, E, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::DEVIATION_EVALUATE, ctx->stream));
  RM_HIP_AS(refuse, spans.begin(MeshSpans::DEVIATION_REDUCE, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_deviation_reduce(D, ctx->stream));
  RM_HIP_AS(refuse, sum_pair(0, rm::RM_DEVIATION_AREA));
  RM_HIP_AS(refuse, sum_pair(1, rm::RM_DEVIATION_SUM1));
  RM_HIP_AS(refuse, spans.end(MeshSpans::DEVIATION_REDUCE, ctx->stream));
  if (triangles_host) RM_HIP_AS(refuse, hipMemcpyAsync(max_host.data(), triangle_max.p, sizeof(float) * (size_t)T, hipMemcpyDeviceToHost, ctx->stream));
  static_assert(kTotalsWords * sizeof(unsigned long long) <= 32768, "the copies are read into the stack");
  unsigned long long copies[kTotalsWords] = {};
  if (int rc = copy_and_wait(ctx, copies, totals.p, sizeof copies, hipMemcpyDeviceToHost)) return rc;
  unsigned long long got[rm::RM_DEVIATION_WORDS] = {};  // the copies' counts added, the largest of their keys, copy 0's four sums
  for (int k = rm::RM_DEVIATION_AREA; k < rm::RM_DEVIATION_WORDS; k++) got[k] = copies[k];
  for (int copy = 0; copy < rm::RM_DEVIATION_COPIES; copy++) {
    const unsigned long long* row = copies + (size_t)copy * rm::RM_DEVIATION_WORDS;
    for (int k = rm::RM_DEVIATION_SKIPPED; k <= rm::RM_DEVIATION_OVER; k++) got[k] += row[k];
    if (row[rm::RM_DEVIATION_KEY] > got[rm::RM_DEVIATION_KEY]) got[rm::RM_DEVIATION_KEY] = row[rm::RM_DEVIATION_KEY];
  }
  r.skipped_triangles = got[rm::RM_DEVIATION_SKIPPED];
  r.unevaluated_triangles = got[rm::RM_DEVIATION_UNEVALUATED];
  r.nonfinite_samples = got[rm::RM_DEVIATION_NONFINITE];
  r.over_triangles = got[rm::RM_DEVIATION_OVER];
  if (const unsigned long long key = got[rm::RM_DEVIATION_KEY]) {  // (0: no evaluated triangle, max and worst stay 0)
    mesh_key_decode(key, &r.max, &r.worst_triangle);
  }
  double sum1, sum2;
  std::memcpy(&r.area, got + rm::RM_DEVIATION_AREA, sizeof r.area);
  std::memcpy(&r.over_area, got + rm::RM_DEVIATION_OVER_AREA, sizeof r.over_area);
  std::memcpy(&sum1, got + rm::RM_DEVIATION_SUM1, sizeof sum1);
  std::memcpy(&sum2, got + rm::RM_DEVIATION_SUM2, sizeof sum2);
  if (r.area != 0.0) {
    r.mean_signed = sum1 / r.area;
    r.rms = std::sqrt(sum2 / r.area);
  }
  if (report) *report = r;
  if (triangles_host) std::memcpy(triangles_host, max_host.data(), sizeof(float) * (size_t)T);
  if (out_ms2) {
    out_ms2[0] = spans.ms(MeshSpans::DEVIATION_EVALUATE);
    out_ms2[1] = spans.ms(MeshSpans::DEVIATION_REDUCE);
  }
  return RM_OK;
}

// ---- refinement (include/hip_raymarch.h "refinement") ------------------------------------------------------------------------------------------------

void rm_mesh_refine_default(RmMeshRefine* params) {
  if (!params) return;
  *params = RmMeshRefine{0.0f, 0.0f, 0.0f, 1, 0ull, 0, 0};
}

static int mesh_refine_check(const Refuse& refuse, const RmMeshRefine* in, RmMeshRefine* p) {
  rm_mesh_refine_default(p);
  if (in) *p = *in;
  if (!std::isfinite(p->iso)) return refuse("refine iso must be finite");
  if (!(std::isfinite(p->tolerance) && p->tolerance >= 0.0f)) return refuse("refine tolerance must be finite and >= 0");
  if (!(std::isfinite(p->min_edge) && p->min_edge >= 0.0f)) return refuse("refine min_edge must be finite and >= 0");
  if (p->rounds < 1 || p->rounds > 8) return refuse("refine rounds must be in 1..8");
  if (int rc = sdf_flags_check(refuse, p->flags)) return rc;
  if (p->reserved != 0) return refuse("refine reserved must be 0");
  return RM_OK;
}

static const unsigned long long kRefineTriangles = 0x7FFFFFFFull / 3ull;  // the kernels' own limit: a using slot 3 t + s is below 2^31

// what a round says of itself: the unique edges, the marked ones, the non-finite midpoints, the largest finite |d - iso|
struct RefineRound {
  unsigned long long edges = 0, split = 0, nonfinite = 0;
  float max = 0.0f;
};

// One round on `cur` (V > 0, 0 < T <= kRefineTriangles): steps 1 - 3, and, where an edge is marked and the round's T' is within `limit`, steps 4
// and 5 into *next -- which otherwise stays empty.  On the context's stream; returns with the stream idle, so the scratch goes with it.  *ms
// gains the round's spans.
static int mesh_refine_round(const Refuse& refuse, rm_scene* scene, const RmMeshRefine& p, unsigned long long limit, const rm_mesh* cur, MeshPtr& next,
                             RefineRound* said, float* ms) {
  rm_ctx* ctx = refuse.ctx;
  MeshSpans& spans = ctx->mesh_spans;
  const unsigned long long V = cur->vertices, T = cur->triangles;
  unsigned long long slots = 1ull;
  while (slots < 4ull * T) slots <<= 1;
  DeviceArray keys, owners, words, edge_of, levels, totals, ends, d, marked, marks;
  RM_HIP_AS(refuse, keys.reserve(sizeof(unsigned long long) * (size_t)slots));
  RM_HIP_AS(refuse, owners.reserve(sizeof(unsigned long long) * (size_t)slots));
  RM_HIP_AS(refuse, words.reserve(sizeof(unsigned long long) * 3u * (size_t)T));
  RM_HIP_AS(refuse, edge_of.reserve(sizeof(unsigned int) * 3u * (size_t)T));
  RM_HIP_AS(refuse, levels.reserve(sizeof(unsigned long long) * (rm::rm_mesh_scan_scratch_elems(3ll * (long long)T) + 1)));  // (every scan here is of 3 T words at most)
  RM_HIP_AS(refuse, totals.reserve(sizeof(unsigned long long) * rm::RM_REFINE_WORDS));
  rm::MeshRefine R{};
  R.vertices = (long long)V;
  R.triangles = (long long)T;
  R.positions = cur->array[RM_MESH_POSITIONS].f32();
  R.colours = cur->array[RM_MESH_COLOURS].f32();
  R.cells = cur->array[RM_MESH_CELLS].u32();
  R.corners = cur->array[RM_MESH_TRIANGLES].u32();
  R.keys = keys.u64();
  R.owners = owners.u64();
  R.slots = slots;
  R.words = words.u64();
  R.edge_of = edge_of.u32();
  R.totals = totals.u64();
  R.iso = p.iso;
  R.tolerance = p.tolerance;
  R.min_edge2 = p.min_edge * p.min_edge;
  unsigned long long got[rm::RM_REFINE_WORDS] = {};
  // 1: the table, the owners' flags, their scan
  RM_HIP_AS(refuse, hipMemsetAsync(totals.p, 0, sizeof got, ctx->stream));
  RM_HIP_AS(refuse, spans.begin(MeshSpans::REFINE_SPLIT, ctx->stream));
  RM_HIP_AS(refuse, hipMemsetAsync(keys.p, 0xFF, sizeof(unsigned long long) * (size_t)slots, ctx->stream));
  RM_HIP_AS(refuse, hipMemsetAsync(owners.p, 0xFF, sizeof(unsigned long long) * (size_t)slots, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_edges(R, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_flags(R, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_scan(R.words, 3ll * (long long)T, levels.u64(), R.totals + rm::RM_REFINE_EDGES, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::REFINE_SPLIT, ctx->stream));
  if (int rc = copy_and_wait(ctx, got, totals.p, sizeof got, hipMemcpyDeviceToHost)) return rc;
  *ms += spans.ms(MeshSpans::REFINE_SPLIT);
  if (got[rm::RM_REFINE_ERROR] != 0ull) return refuse("an edge found no slot in the table", RM_ERR_DEVICE);
  const unsigned long long E = got[rm::RM_REFINE_EDGES];
  said->edges = E;
  if (E == 0) return RM_OK;  // (no triangle takes part)
  // 2, 3: the edges' numbers and ends, d at the midpoints, the marks, the children; two scans, one read
  RM_HIP_AS(refuse, ends.reserve(sizeof(unsigned int) * 2u * (size_t)E));
  RM_HIP_AS(refuse, d.reserve(sizeof(float) * (size_t)E));
  RM_HIP_AS(refuse, marked.reserve(sizeof(unsigned int) * (size_t)E));
  RM_HIP_AS(refuse, marks.reserve(sizeof(unsigned long long) * (size_t)E));
  if (int rc = scene_cull_grid(ctx, scene, p.flags, 1ll << 40)) return rc;
  R.edges = (long long)E;
  R.ends = ends.u32();
  R.d = d.f32();
  R.marked = marked.u32();
  R.marks = marks.u64();
  MeshRefineMidpoints Q{};
  Q.scene = scene_view(scene, p.flags);
  Q.positions = R.positions;
  Q.ends = R.ends;
  Q.d = d.f32();
  Q.edges = (int)E;
  RM_HIP_AS(refuse, spans.begin(MeshSpans::REFINE_SPLIT, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_number(R, ctx->stream));
  RM_HIP_AS(refuse, RM_SCENE_PASS(ctx, p.flags, launch_mesh_refine_eval, Q, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_mark(R, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_count(R, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_scan(R.marks, (long long)E, levels.u64(), R.totals + rm::RM_REFINE_SPLIT, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_scan(R.words, (long long)T, levels.u64(), R.totals + rm::RM_REFINE_CHILDREN, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::REFINE_SPLIT, ctx->stream));
  if (int rc = copy_and_wait(ctx, got, totals.p, sizeof got, hipMemcpyDeviceToHost)) return rc;
  *ms += spans.ms(MeshSpans::REFINE_SPLIT);
  const unsigned long long K = got[rm::RM_REFINE_SPLIT], T2 = got[rm::RM_REFINE_CHILDREN];
  said->split = K;
  said->nonfinite = got[rm::RM_REFINE_NONFINITE];
  const unsigned int most = (unsigned int)got[rm::RM_REFINE_MAX];
  std::memcpy(&said->max, &most, sizeof most);
  if (K == 0 || T2 > limit) return RM_OK;
  if (V + K > (unsigned long long)INT_MAX)
    return refuse("the refined mesh has more vertices than the kernels' int index holds (V' > INT_MAX)", RM_ERR_DEVICE);
  // 4, 5: the round's mesh
  MeshPtr made(new (std::nothrow) rm_mesh(ctx), rm_mesh_destroy);
  if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
  for (int a = 0; a < 5; a++) made->has[a] = cur->has[a];
  made->vertices = V + K;
  made->triangles = T2;
  for (int what : {RM_MESH_POSITIONS, RM_MESH_COLOURS, RM_MESH_TRIANGLES, RM_MESH_CELLS})
    if (cur->array[what].p) RM_HIP_AS(refuse, made->array[what].reserve(mesh_array_bytes(made.get(), what)));
  R.out_positions = made->array[RM_MESH_POSITIONS].f32();
  R.out_colours = made->array[RM_MESH_COLOURS].f32();
  R.out_cells = made->array[RM_MESH_CELLS].u32();
  R.out_corners = made->array[RM_MESH_TRIANGLES].u32();
  RM_HIP_AS(refuse, spans.begin(MeshSpans::REFINE_SPLIT, ctx->stream));
  for (int what : {RM_MESH_POSITIONS, RM_MESH_COLOURS, RM_MESH_CELLS})
    if (cur->array[what].p)
      RM_HIP_AS(refuse, hipMemcpyAsync(made->array[what].p, cur->array[what].p, mesh_array_bytes(cur, what), hipMemcpyDeviceToDevice, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_vertices(R, ctx->stream));
  RM_HIP_AS(refuse, rm::launch_mesh_refine_emit(R, ctx->stream));
  RM_HIP_AS(refuse, spans.end(MeshSpans::REFINE_SPLIT, ctx->stream));
  RM_HIP_AS(refuse, hipStreamSynchronize(ctx->stream));
  *ms += spans.ms(MeshSpans::REFINE_SPLIT);
  next = std::move(made);
  return RM_OK;
}

int rm_mesh_refine(rm_mesh* mesh, rm_scene* scene, const RmMeshRefine* params, const RmMeshProject* project, rm_mesh** out, RmMeshRefinement* report) {
  rm_ctx* ctx = mesh ? mesh->ctx : nullptr;
  const Refuse refuse{ctx, "rm_mesh_refine"};
  RmMeshRefine p;
  RmMeshProject q;
  if (int rc = mesh_refine_check(refuse, params, &p)) return rc;
  if (int rc = mesh_project_check(refuse, project, &q)) return rc;  // (NULL: the defaults, of which the normals' delta alone is used)
  if (!project) q.flags = p.flags;
  if (int rc = scene_check(refuse, scene, out != nullptr)) return rc;  // (a NULL mesh is a NULL context there)
  const unsigned long long V = mesh->vertices, T = mesh->triangles;
  if (T > kRefineTriangles) return refuse("the mesh has more triangles than the kernels' index holds edge slots of (3 T >= 2^31)", RM_ERR_DEVICE);
  if (V > (unsigned long long)INT_MAX) return refuse("the mesh has more vertices than the kernels' int index holds (V > INT_MAX)", RM_ERR_DEVICE);
  *out = nullptr;
  RM_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned long long limit = p.max_triangles != 0ull && p.max_triangles < kRefineTriangles ? p.max_triangles : kRefineTriangles;
  RmMeshRefinement r{};
  r.vertices_before = V;
  r.triangles_before = T;
  r.stopped = 1;
  float ms_split = 0.0f, ms_project = 0.0f;
  MeshPtr made(nullptr, rm_mesh_destroy);  // the last round applied; none: the source stands
  const rm_mesh* at = mesh;
  if (V > 0 && T > 0) {
    r.stopped = 0;
    for (int round = 0; round < p.rounds; round++) {
      MeshPtr next(nullptr, rm_mesh_destroy);
      RefineRound said;
      if (int rc = mesh_refine_round(refuse, scene, p, limit, at, next, &said, &ms_split)) return rc;
      r.edges[round] = said.edges;
      r.split_edges[round] = said.split;
      r.nonfinite_midpoints[round] = said.nonfinite;
      r.rounds_run = round + 1;
      r.max_last = said.max;
      if (round == 0) r.max_first = said.max;
      if (!next) {
        r.stopped = said.split == 0 ? 1 : 2;
        break;
      }
      if (project) {
        rm_mesh* moved = nullptr;
        RmMeshProjection projection{};
        if (int rc = mesh_project_run(refuse, next.get(), scene, q, false, &moved, &projection, nullptr)) return rc;
        next.reset(moved);
        r.flipped_triangles += projection.flipped_triangles;
        ms_project += moved->ms[1];
      }
      made = std::move(next);
      at = made.get();
    }
  }
  if (!made) {  // no round was applied: the source's arrays, but for the normals
    made.reset(new (std::nothrow) rm_mesh(ctx));
    if (!made) return refuse("out of host memory", RM_ERR_DEVICE);
    made->vertices = V;
    made->triangles = T;
    for (int what : {RM_MESH_POSITIONS, RM_MESH_COLOURS, RM_MESH_TRIANGLES, RM_MESH_CELLS})
      if (mesh->array[what].p) {
        RM_HIP_AS(refuse, made->array[what].reserve(mesh_array_bytes(mesh, what)));
        RM_HIP_AS(refuse, hipMemcpyAsync(made->array[what].p, mesh->array[what].p, mesh_array_bytes(mesh, what), hipMemcpyDeviceToDevice, ctx->stream));
      }
  }
  for (int a = 0; a < 5; a++) made->has[a] = mesh->has[a];
  const bool with_normals = mesh->array[RM_MESH_NORMALS].p != nullptr && made->vertices > 0;
  if (with_normals) {
    RM_HIP_AS(refuse, made->array[RM_MESH_NORMALS].reserve(mesh_array_bytes(made.get(), RM_MESH_NORMALS)));
    RM_HIP_AS(refuse, ctx->mesh_spans.begin(MeshSpans::REFINE_NORMALS, ctx->stream));
    RM_HIP_AS(refuse, probe_enqueue(ctx, scene, RM_PROBE_NORMAL, made->array[RM_MESH_POSITIONS].f32(), made->array[RM_MESH_NORMALS].f32(), (int)made->vertices,
                                    q.normal_delta, q.flags, ctx->stream));
    RM_HIP_AS(refuse, ctx->mesh_spans.end(MeshSpans::REFINE_NORMALS, ctx->stream));
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return refuse("the stream failed", RM_ERR_DEVICE);
  made->ms[0] = 0.0f;
  made->ms[1] = ms_split;
  made->ms[2] = ms_project + (with_normals ? ctx->mesh_spans.ms(MeshSpans::REFINE_NORMALS) : 0.0f);
  r.vertices = made->vertices;
  r.triangles = made->triangles;
  if (report) *report = r;
  *out = made.release();
  return RM_OK;
}
