// Mesh kernels (include/hip_raymarch.h "mesh extraction" and the sections behind it).  Included by rm_strict.hip / rm_fast.hip /
// rm_glstack.hip behind rm_kernels.inc.
//
// In every unit, in that unit's arithmetic -- the kernels that evaluate the scene, each launched by launch_point_kind (rm_kernels.inc):
//   - the sampler: a scene's distance on a grid of corners                                  (rm_sdf_grid, rm_mesh_extract*)
//   - ambient occlusion: the distance at a fan of taps over every vertex                    (rm_mesh_occlusion)
//   - projection: the distance and, where wanted, the normal at every vertex                (rm_mesh_project)
//   - deviation: the distance at fixed points inside every triangle                         (rm_mesh_deviation)
//   - refinement: the distance at every unique edge's midpoint                              (rm_mesh_refine)
// In the strict unit only -- they have no arithmetic of a policy's own:
//   - the mesher: surface nets over such a grid, whole or in z-slabs                        (rm_mesh_extract*, rm_mesh_from_values*)
//   - sharp vertices: the two kernels that move vertices to their cells' QEF minimisers     (rm_mesh_extract_sharp*)
//   - components and islands: the integer kernels that label and compact                    (rm_mesh_components, rm_mesh_filter)
//   - simplification: vertex clustering, and the quadric placement on top of it             (rm_mesh_simplify, rm_mesh_simplify_quadric)
//   - measures: the edge table, classes, extent and the fixed-tree sums                     (rm_mesh_measure)
//   - projection's step and report, deviation's reducer                                     (behind their evaluating kernels)
//   - refinement's edge table, marks, new vertices and children                             (around its evaluating kernel)
namespace rm {

// ---- the sampler: rm_probe's RM_PROBE_SDF with the point made from the corner's indices -------------------------------------
// One thread per corner, x fastest, so a wave's stores are one run of a row.  Lanes beyond the last corner evaluate the last corner
// and store nothing: the evaluators ballot and branch wave-uniformly (rm_probe_kernel keeps whole waves alive the same way).
template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void rm_sdf_grid_kernel(const SdfGridParams P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;
  __shared__ SceneLds lds;
  const GridDims& g = P.grid;
  const int gi = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = gi < g.corners ? gi : g.corners - 1;
  const int i = c % g.nc[0], row = c / g.nc[0];
  const v3 p = V(rm_grid_coord(g, 0, i), rm_grid_coord(g, 1, row % g.nc[1]), rm_grid_coord(g, 2, row / g.nc[1] + P.plane0));  // (a window's plane by its index in the whole grid)
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();
  const float d = Sdf<KIND>::template eval<MM>(P.scene, lds, p);
  if (gi < g.corners) P.out[c] = d;
}

#ifndef RM_ONLY_KERNELS
// (launch_point_kind: a corner's value has to be the probe's at that point)
hipError_t RM_LAUNCH(launch_sdf_grid)(const SdfGridParams& P, hipStream_t stream) {
  const dim3 grid((unsigned int)((P.grid.corners + 255) / 256));
  return launch_point_kind(P.scene, [&](auto kind) { hipLaunchKernelGGL((rm_sdf_grid_kernel<decltype(kind)::value, kFast>), grid, dim3(256), 0, stream, P); });
}
#endif

// ---- ambient occlusion: the scene's distance at a fixed fan of taps over every vertex (the header's "ambient occlusion") -----------
// One lane per (vertex, direction): a vertex's K lanes are consecutive, and K divides 64, so they sit in one wave.  A lane builds the
// frame of its vertex's probed normal, turns its direction into it and makes all its taps' points BEFORE enter_math_mode (the fast
// Mandelbulb flushes denormals: what can go subnormal behind it reaches only the quantiser, where it is 0 either way).  The points
// wait in LDS, [tap][component][thread], and that is what holds the order: the compiler orders no floating-point operation against a
// write of the mode register (with the points in registers the fast Mandelbulb's code had the switch ahead of the whole set-up), but
// the stores that take them lie ahead of a barrier, and the switch behind it.  It also spares the evaluator 24 registers.  Then the
// lane evaluates its taps one after the other and sums its quanta; the K integer sums are added across the vertex's lanes (any order
// gives the same sum), and lane k = 0 scales, shades and stores.  Lanes beyond V * K repeat the last ray and store nothing: the
// evaluators ballot and branch wave-uniformly, as above.  The triangles are not read.
template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void rm_mesh_occlusion_kernel(const MeshOcclusionPass P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;
  __shared__ SceneLds lds;
  __shared__ float taps[8][3][256];  // a lane's points: only that lane reads them back
  const unsigned int rays = (unsigned int)P.vertices << P.log2_directions;  // < 2^31 (rm_mesh_occlusion)
  const unsigned int gi = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned int ray = gi < rays ? gi : rays - 1u;
  const unsigned int v = ray >> P.log2_directions, k = ray & ((1u << P.log2_directions) - 1u);
  const float* const pv = P.positions + 3 * (size_t)v;
  const float* const nv = P.normals + 3 * (size_t)v;
  const float px = pv[0], py = pv[1], pz = pv[2];
  const float nx = nv[0], ny = nv[1], nz = nv[2];
  const float d0 = P.d0[v];
  const float4 dir = P.directions[k];  // (x, y, z, 1 / z) in the frame
  // the frame (Duff et al. 2017) and the direction in it
  const float s = copysignf(1.0f, nz);
  const float a = -1.0f / (s + nz);
  const float b = (nx * ny) * a;
  const float tx = 1.0f + ((s * nx) * nx) * a, ty = s * b, tz = (-s) * nx;
  const float bx = b, by = s + (ny * ny) * a, bz = -ny;
  const float wx = ((dir.x * tx) + (dir.y * bx)) + (dir.z * nx);
  const float wy = ((dir.x * ty) + (dir.y * by)) + (dir.z * ny);
  const float wz = ((dir.x * tz) + (dir.y * bz)) + (dir.z * nz);
  {
    float t = P.radius;
#pragma unroll
    for (int j = 0; j < 8; j++) {  // (taps beyond J are made and never evaluated)
      taps[j][0][threadIdx.x] = px + wx * t;
      taps[j][1][threadIdx.x] = py + wy * t;
      taps[j][2][threadIdx.x] = pz + wz * t;
      t *= 0.5f;
    }
  }
  __syncthreads();
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();
  unsigned int sum = 0;
  float t = P.radius, it = P.inv_radius;
  for (int j = 0; j < P.taps; j++) {
    const float d = Sdf<KIND>::template eval<MM>(P.scene, lds, V(taps[j][0][threadIdx.x], taps[j][1][threadIdx.x], taps[j][2][threadIdx.x]));
    const float e = dir.z * t;
    const float ie = dir.w * it;
    float o = ((d0 + e) - d) * ie;
    if (!(o >= 0.0f)) o = 0.0f;
    if (o > 1.0f) o = 1.0f;
    sum += (unsigned int)(o * 65536.0f + 0.5f);
    t *= 0.5f;
    it *= 2.0f;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1)
    if (m < (1 << P.log2_directions)) sum += (unsigned int)__shfl_xor((int)sum, m);
  if (gi < rays && k == 0) {
    const float occ = (float)sum * P.scale;
    float ao = 1.0f - P.strength * occ;
    if (!(ao <= 1.0f)) ao = 1.0f;
    if (ao < 0.0f) ao = 0.0f;
    P.out[v] = ao;
  }
}

#ifndef RM_ONLY_KERNELS
hipError_t RM_LAUNCH(launch_mesh_occlusion)(const MeshOcclusionPass& P, hipStream_t stream) {
  const long long rays = (long long)P.vertices << P.log2_directions;
  const dim3 grid((unsigned int)((rays + 255) / 256));
  return launch_point_kind(P.scene, [&](auto kind) { hipLaunchKernelGGL((rm_mesh_occlusion_kernel<decltype(kind)::value, kFast>), grid, dim3(256), 0, stream, P); });
}
#endif

// ---- projection: the scene's distance and normal at every vertex (the header's "projection onto the surface") ------------------------------
// Whether a lane's vertex may step this round: e = d - iso is finite and |e| > tolerance.  The step kernel decides that for itself, in plain
// IEEE; this copy only tells the evaluating kernel whether the wave needs normals, so it may say yes too often and never too seldom.  In a
// kernel that runs with fp32 denormals flushed (enter_math_mode) the subtraction reads a subnormal operand as zero and writes a subnormal
// result as zero, so everything behind it is integer: with a subnormal d or iso the answer is yes unless their bits agree; a difference of
// zero is a true zero only where d == iso, and otherwise a flushed subnormal, which a tolerance below the normals cannot be told to cover.
template <bool FLUSHED>
__device__ inline bool mesh_project_wants(float d, float iso, float tolerance) {
  if (!FLUSHED) {
    const float e = d - iso;
    return isfinite(e) && fabsf(e) > tolerance;
  }
  const unsigned int bd = __float_as_uint(d), bi = __float_as_uint(iso), bt = __float_as_uint(tolerance) & 0x7FFFFFFFu;
  const unsigned int ad = bd & 0x7FFFFFFFu, ai = bi & 0x7FFFFFFFu;
  if (ad >= 0x7F800000u) return false;       // (iso is finite: e is not)
  if (bd == bi || (ad | ai) == 0u) return false;  // e is a zero
  if ((ad != 0u && ad < 0x00800000u) || (ai != 0u && ai < 0x00800000u)) return true;
  const unsigned int ae = __float_as_uint(d - iso) & 0x7FFFFFFFu;
  if (ae >= 0x7F800000u) return false;
  if (ae < 0x00800000u) return bt < 0x00800000u;  // a flushed subnormal
  return ae > bt;
}

// One lane per vertex.  The scene is staged and the math mode entered as the probe kernel does, and d and the normal are that kernel's
// RM_PROBE_SDF and RM_PROBE_NORMAL at the vertex: the same calls on the same policies.  A wave none of whose lanes wants a normal leaves
// before scene_normal's four evaluations, whole: the evaluators ballot and branch wave-uniformly, so no single lane may.  Lanes beyond V
// repeat the last vertex, which changes no ballot, and store nothing.
template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void rm_mesh_project_eval_kernel(const MeshProjectEval P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;
  constexpr bool kFlushed = FAST && (KIND == RM_SCENE_MANDELBULB || KIND == RM_KIND_BULB8 || KIND == RM_KIND_TABLE_KINDS);  // enter_math_mode's rule
  __shared__ SceneLds lds;
  const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;  // (V goes up to INT_MAX: the last workgroup's indices pass it)
  const int v = gi < P.vertices ? (int)gi : P.vertices - 1;
  const v3 p = V(P.positions[3 * (size_t)v], P.positions[3 * (size_t)v + 1], P.positions[3 * (size_t)v + 2]);
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();
  const float d = Sdf<KIND>::template eval<MM>(P.scene, lds, p);
  if (gi < P.vertices) P.d[v] = d;
  if (__ballot(mesh_project_wants<kFlushed>(d, P.iso, P.tolerance)) == 0ull) return;
  const v3 n = scene_normal<KIND>(P.scene, lds, p, P.normal_delta);
  if (gi < P.vertices) {
    P.normals[3 * (size_t)v] = n.x;
    P.normals[3 * (size_t)v + 1] = n.y;
    P.normals[3 * (size_t)v + 2] = n.z;
  }
}

#ifndef RM_ONLY_KERNELS
hipError_t RM_LAUNCH(launch_mesh_project_eval)(const MeshProjectEval& P, hipStream_t stream) {
  const dim3 grid((unsigned int)(((long long)P.vertices + 255) / 256));
  return launch_point_kind(P.scene, [&](auto kind) { hipLaunchKernelGGL((rm_mesh_project_eval_kernel<decltype(kind)::value, kFast>), grid, dim3(256), 0, stream, P); });
}
#endif

// ---- deviation: the scene's distance at fixed points inside every triangle (the header's "deviation") -----------------------------------------
// One lane per (triangle, sample): a triangle's S lanes are consecutive, and S divides 64, so they sit in one wave.  A lane reads its
// triangle's indices and corners and makes its point BEFORE enter_math_mode; the point waits in LDS, [component][thread], ahead of a barrier,
// and the switch lies behind it -- the ordering rm_mesh_occlusion_kernel documents: the compiler orders no floating-point operation against a
// write of the mode register, and the fast Mandelbulb flushes denormals.  Lanes beyond T * S repeat the last sample and store nothing: the
// evaluators ballot and branch wave-uniformly.  A lane of a skipped triangle (an index >= V) reads nothing out of range: it evaluates vertex
// 0's position, and the reducer ignores what it stores.
template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void rm_mesh_deviation_eval_kernel(const MeshDeviationSdf P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;
  __shared__ SceneLds lds;
  __shared__ float point[3][256];  // a lane's point: only that lane reads it back
  const unsigned int lanes = (unsigned int)P.triangles << P.log2_samples;  // < 2^31 (rm_mesh_deviation)
  const unsigned int gi = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned int i = gi < lanes ? gi : lanes - 1u;
  const unsigned int t = i >> P.log2_samples, s = i & ((1u << P.log2_samples) - 1u);
  unsigned int i0 = P.corners[3 * (size_t)t], i1 = P.corners[3 * (size_t)t + 1], i2 = P.corners[3 * (size_t)t + 2];
  if (!((long long)i0 < P.vertices && (long long)i1 < P.vertices && (long long)i2 < P.vertices)) i0 = i1 = i2 = 0u;
  const float* const p0 = P.positions + 3 * (size_t)i0;
  const float* const p1 = P.positions + 3 * (size_t)i1;
  const float* const p2 = P.positions + 3 * (size_t)i2;
  const float4 w = P.weights[s];  // (w0, w1, w2, 0)
#pragma unroll
  for (int c = 0; c < 3; c++) point[c][threadIdx.x] = ((w.x * p0[c]) + (w.y * p1[c])) + (w.z * p2[c]);
  __syncthreads();
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();
  const float d = Sdf<KIND>::template eval<MM>(P.scene, lds, V(point[0][threadIdx.x], point[1][threadIdx.x], point[2][threadIdx.x]));
  if (gi < lanes) P.d[gi] = d;
}

#ifndef RM_ONLY_KERNELS
hipError_t RM_LAUNCH(launch_mesh_deviation_eval)(const MeshDeviationSdf& P, hipStream_t stream) {
  const long long lanes = (long long)P.triangles << P.log2_samples;
  const dim3 grid((unsigned int)((lanes + 255) / 256));
  return launch_point_kind(P.scene, [&](auto kind) { hipLaunchKernelGGL((rm_mesh_deviation_eval_kernel<decltype(kind)::value, kFast>), grid, dim3(256), 0, stream, P); });
}
#endif

// ---- refinement: the scene's distance at every unique edge's midpoint (the header's "refinement") ---------------------------------------------
// One lane per edge.  A lane reads its edge's ends and makes the midpoint BEFORE enter_math_mode; the point waits in LDS, [component][thread],
// ahead of a barrier, and the switch lies behind it -- the ordering rm_mesh_deviation_eval_kernel documents, and for the same reason: the
// compiler orders no floating-point operation against a write of the mode register, and the fast Mandelbulb flushes denormals.  Lanes beyond E
// repeat the last edge and store nothing: the evaluators ballot and branch wave-uniformly.  An edge's ends are < V (refine_number wrote them).
template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void rm_mesh_refine_eval_kernel(const MeshRefineMidpoints P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;
  __shared__ SceneLds lds;
  __shared__ float point[3][256];  // a lane's point: only that lane reads it back
  const unsigned int edges = (unsigned int)P.edges;
  const unsigned int gi = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned int e = gi < edges ? gi : edges - 1u;
  const float* const a = P.positions + 3 * (size_t)P.ends[2 * (size_t)e];
  const float* const b = P.positions + 3 * (size_t)P.ends[2 * (size_t)e + 1];
#pragma unroll
  for (int c = 0; c < 3; c++) point[c][threadIdx.x] = 0.5f * (a[c] + b[c]);
  __syncthreads();
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();
  const float d = Sdf<KIND>::template eval<MM>(P.scene, lds, V(point[0][threadIdx.x], point[1][threadIdx.x], point[2][threadIdx.x]));
  if (gi < edges) P.d[gi] = d;
}

#ifndef RM_ONLY_KERNELS
hipError_t RM_LAUNCH(launch_mesh_refine_eval)(const MeshRefineMidpoints& P, hipStream_t stream) {
  const dim3 grid((unsigned int)(((long long)P.edges + 255) / 256));
  return launch_point_kind(P.scene, [&](auto kind) { hipLaunchKernelGGL((rm_mesh_refine_eval_kernel<decltype(kind)::value, kFast>), grid, dim3(256), 0, stream, P); });
}
#endif

#if !RM_BUILD_FAST && !RM_GL_STACK
// ---- the mesher: surface nets ---------------------------------------------------------------------------------------------------
// A corner is inside iff v - iso < 0 (NaN, +0, -0 are outside); a cell is active iff its 8 corners are not all alike and then owns
// one vertex, the mean of its edges' crossing points; an edge whose ends differ, away from the grid's boundary, owns one quad
// between the four cells round it.  Three steps: count per cell, scan, emit -- so vertices and faces come out in ascending cell
// order on every run, with no atomics.  One thread per cell; a cell reads its 8 corners (two runs of a row per wave and pair of rows).

struct MeshCell {
  int idx[3];      // the cell's indices
  int cell;        // (k * ny + j) * nx + i
  float e[8];      // v - iso of corner dx | dy << 1 | dz << 2
  unsigned int inside;  // bit per corner
};

__device__ inline MeshCell mesh_cell(const MeshParams& P, int cell) {
  const GridDims& g = P.grid;
  const int nx = g.nc[0] - 1, ny = g.nc[1] - 1;
  MeshCell c;
  c.cell = cell;
  c.idx[0] = cell % nx;
  c.idx[1] = (cell / nx) % ny;
  c.idx[2] = cell / (nx * ny);
  const size_t base = ((size_t)(c.idx[2] - P.plane0) * g.nc[1] + c.idx[1]) * g.nc[0] + c.idx[0];  // (the values begin at plane P.plane0)
  c.inside = 0u;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const size_t at = base + (size_t)(k & 1) + (size_t)((k >> 1) & 1) * g.nc[0] + (size_t)(k >> 2) * g.nc[0] * g.nc[1];
    c.e[k] = P.values[at] - P.iso;
    c.inside |= (c.e[k] < 0.0f ? 1u : 0u) << k;
  }
  return c;
}

// the quads the cell's three low edges own, as a mask over the axes
__device__ inline unsigned int mesh_quads(const MeshCell& c) {
  unsigned int q = 0u;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, cc = (a + 2) % 3;
    const bool crosses = ((c.inside ^ (c.inside >> (1 << a))) & 1u) != 0u;
    if (crosses && c.idx[b] >= 1 && c.idx[cc] >= 1) q |= 1u << a;
  }
  return q;
}

__global__ __launch_bounds__(256) void rm_mesh_count_kernel(const MeshParams P, int cells) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= cells) return;
  const MeshCell c = mesh_cell(P, cell);
  const unsigned long long active = (c.inside != 0u && c.inside != 0xFFu) ? 1ull : 0ull;
  P.counts[cell] = active | ((unsigned long long)__popc(mesh_quads(c)) << 32);
}

// Exclusive scan of 64-bit words (two 32-bit sums side by side: neither reaches 2^32), 256 per workgroup: every element becomes the sum
// of those before it IN ITS WORKGROUP and sums[workgroup] the workgroup's total; the totals are scanned the same way (launch_mesh_scan)
// and added back.  n is a long long: 2^28 cells at most, but the words are addressed with it.
__global__ __launch_bounds__(256) void rm_mesh_scan_kernel(unsigned long long* data, long long n, unsigned long long* sums) {
  __shared__ unsigned long long s[256];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long v = i < n ? data[i] : 0ull;
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned long long u = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += u;
    __syncthreads();
  }
  if (i < n) data[i] = s[threadIdx.x] - v;
  if (threadIdx.x == 255) sums[blockIdx.x] = s[255];
}
__global__ __launch_bounds__(256) void rm_mesh_scan_add_kernel(unsigned long long* data, long long n, const unsigned long long* sums) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) data[i] += sums[blockIdx.x];
}

// the vertex of an active cell: the mean of its edges' crossing points
__device__ inline void mesh_vertex(const GridDims& g, const MeshCell& c, float* out) {
  float pc[3][2];  // the corners' coordinates
#pragma unroll
  for (int a = 0; a < 3; a++) { pc[a][0] = rm_grid_coord(g, a, c.idx[a]); pc[a][1] = rm_grid_coord(g, a, c.idx[a] + 1); }
  float sum[3] = {0.0f, 0.0f, 0.0f};
  int m = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, cc = (a + 2) % 3;
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const int ob = o & 1, oc = o >> 1, k0 = (ob << b) | (oc << cc), k1 = k0 | (1 << a);
      if ((((c.inside >> k0) ^ (c.inside >> k1)) & 1u) == 0u) continue;
      float t = c.e[k0] / (c.e[k0] - c.e[k1]);
      if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
      const float span = pc[a][1] - pc[a][0], step = t * span;
      float p[3];
      p[a] = pc[a][0] + step;
      p[b] = pc[b][ob];
      p[cc] = pc[cc][oc];
      sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2];
      m++;
    }
  }
  const float fm = (float)m;
  out[0] = sum[0] / fm;
  out[1] = sum[1] / fm;
  out[2] = sum[2] / fm;
}

// The cell's quads from triangle `tri` on: vertices of the cells at (b, c) offsets (-1,-1), (0,-1), (0,0), (-1,0); counter-clockwise seen
// from outside.  vertex_of(d): the vertex of the cell d cells before this one.
template <class VertexOf>
__device__ inline void mesh_write_quads(const GridDims& g, const MeshCell& c, unsigned int vertex, size_t tri, unsigned int* triangles, VertexOf vertex_of) {
  const unsigned int quads = mesh_quads(c);
  const int stride[3] = {1, g.nc[0] - 1, (g.nc[0] - 1) * (g.nc[1] - 1)};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!((quads >> a) & 1u)) continue;
    const int sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];
    const unsigned int q0 = vertex_of(sb + sc), q1 = vertex_of(sc), q2 = vertex, q3 = vertex_of(sb);
    unsigned int* t = triangles + 3 * tri;
    if (c.inside & 1u) { t[0] = q0; t[1] = q1; t[2] = q2; t[3] = q0; t[4] = q2; t[5] = q3; }
    else { t[0] = q0; t[1] = q3; t[2] = q2; t[3] = q0; t[4] = q2; t[5] = q1; }
    tri += 2;
  }
}

__global__ __launch_bounds__(256) void rm_mesh_emit_kernel(const MeshParams P, int cells) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= cells) return;
  const MeshCell c = mesh_cell(P, cell);
  if (c.inside == 0u || c.inside == 0xFFu) return;  // (an edge that owns a quad crosses: its cell is active)
  const unsigned long long first = P.counts[cell];
  const unsigned int vertex = (unsigned int)first;
  mesh_vertex(P.grid, c, P.positions + 3 * (size_t)vertex);
  P.cells[vertex] = (unsigned int)cell;
  mesh_write_quads(P.grid, c, vertex, 2 * (size_t)(first >> 32), P.triangles, [&](int d) { return (unsigned int)P.counts[cell - d]; });
}

// ---- slabbed extraction (include/hip_raymarch.h "slabbed extraction") ------------------------------------------------------------------
// The mesher over a window of z planes.  Cell indices are those of the whole grid (at most 2^30: an int), so mesh_cell, mesh_quads' boundary
// rule and RM_MESH_CELLS are the dense mesher's; only the values and the counts are addressed from the window's first plane.

// The tally pass: one thread per cell of the slab's own layers, the words (active) | (quads << 32) summed in the wave, then in the
// workgroup, then by one 64-bit atomic add per workgroup.  Integer sums: the same on every run.
__global__ __launch_bounds__(256) void rm_mesh_slab_tally_kernel(const MeshSlab S, int first, int cells) {
  __shared__ unsigned long long waves[4];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long word = 0ull;
  if (t < cells) {
    const MeshCell c = mesh_cell(S.mesh, first + t);
    const unsigned long long active = (c.inside != 0u && c.inside != 0xFFu) ? 1ull : 0ull;
    word = active | ((unsigned long long)__popc(mesh_quads(c)) << 32);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) word += __shfl_down(word, off, 64);
  if ((threadIdx.x & 63u) == 0u) waves[threadIdx.x >> 6] = word;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const unsigned long long sum = (waves[0] + waves[1]) + (waves[2] + waves[3]);
    if (sum != 0ull) atomicAdd(S.total, sum);
  }
}

// The emit pass's count: one thread per cell of the window, the halo layer's first.
__global__ __launch_bounds__(256) void rm_mesh_slab_count_kernel(const MeshSlab S, int first, int cells) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells) return;
  const MeshCell c = mesh_cell(S.mesh, first + t);
  const unsigned long long active = (c.inside != 0u && c.inside != 0xFFu) ? 1ull : 0ull;
  S.mesh.counts[t] = active | ((unsigned long long)__popc(mesh_quads(c)) << 32);
}

// ... and its emit, over the scanned counts: the halo's cells emit nothing (they are the slab's before); what the scan counted of them,
// its value at the slab's first own cell, goes off every index, and the slabs' bases on.
__global__ __launch_bounds__(256) void rm_mesh_slab_emit_kernel(const MeshSlab S, int first, int halo, int cells) {
  const int t = halo + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells) return;
  const MeshCell c = mesh_cell(S.mesh, first + t);
  if (c.inside == 0u || c.inside == 0xFFu) return;
  const unsigned long long* counts = S.mesh.counts;
  const unsigned long long before = counts[halo], at = counts[t];
  const unsigned int shift = (unsigned int)S.vertex_base - (unsigned int)before;  // (mod 2^32: every index it meets is below 2^32)
  const unsigned int vertex = (unsigned int)at + shift;
  mesh_vertex(S.mesh.grid, c, S.mesh.positions + 3 * (size_t)vertex);
  S.mesh.cells[vertex] = (unsigned int)c.cell;
  const size_t tri = 2 * (size_t)(S.quad_base + ((at >> 32) - (before >> 32)));
  mesh_write_quads(S.mesh.grid, c, vertex, tri, S.mesh.triangles, [&](int d) { return (unsigned int)counts[t - d] + shift; });
}

// the first three of every twelve floats: the diffuse colour out of the material probe's records
// (the name matters to an existing test: tests/test_gbuffer_half_cpu.py runs llvm-objdump -D over the code objects, data sections included, and
// that tool faults on some symbol-table offsets read as instructions; kernel names shift those offsets -- rerun that test after renaming one)
__global__ __launch_bounds__(256) void rm_mesh_take3_kernel(const float* material, float* colours, long long n3) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n3) colours[i] = material[(i / 3) * 12 + i % 3];
}

// ---- sharp vertices: dual contouring over the emitted mesh (include/hip_raymarch.h "sharp vertices") ----------------------------------
// One thread per vertex, the cell through RM_MESH_CELLS.  The scene is evaluated by the probe kernel between these launches (rm_mesh_host.inc
// mesh_sharpen); these two only prepare its input and consume its output, in this unit's plain fp32: every operation rounded on its own.

// The 12 slots of a vertex: a slot is live iff its edge's ends differ in `inside`, and then carries a bracket (x0, e0, x1, e1) along its axis.
// init: the bracket is the edge itself, and a dead slot's point becomes the surface-nets vertex.  consume: the probe's value at the bracket's
// midpoint replaces the end it agrees with in `inside`.  last: the point is the bracket's linear crossing and the live mask is written;
// otherwise the point is the bracket's midpoint, for the next round, and the bracket is kept.
__global__ __launch_bounds__(256) void rm_mesh_cross_kernel(const MeshSharpParams P, int init, int consume, int last) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= P.vertices) return;
  const size_t V = (size_t)P.vertices;
  const GridDims& g = P.mesh.grid;
  const MeshCell c = mesh_cell(P.mesh, (int)P.mesh.cells[v]);
  float pc[3][2];
#pragma unroll
  for (int a = 0; a < 3; a++) { pc[a][0] = rm_grid_coord(g, a, c.idx[a]); pc[a][1] = rm_grid_coord(g, a, c.idx[a] + 1); }
  float nets[3] = {0.0f, 0.0f, 0.0f};
  if (init) { nets[0] = P.mesh.positions[3 * (size_t)v]; nets[1] = P.mesh.positions[3 * (size_t)v + 1]; nets[2] = P.mesh.positions[3 * (size_t)v + 2]; }
  unsigned int live = 0u;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, cc = (a + 2) % 3;
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const int ob = o & 1, oc = o >> 1, k0 = (ob << b) | (oc << cc), k1 = k0 | (1 << a);
      const size_t at = (size_t)(4 * a + o) * V + (size_t)v;
      float* point = P.points + 3 * at;
      if ((((c.inside >> k0) ^ (c.inside >> k1)) & 1u) == 0u) {
        if (init) { point[0] = nets[0]; point[1] = nets[1]; point[2] = nets[2]; }
        continue;
      }
      live |= 1u << (4 * a + o);
      float x0, e0, x1, e1;
      if (init) {
        x0 = pc[a][0]; e0 = c.e[k0]; x1 = pc[a][1]; e1 = c.e[k1];
      } else {
        const float4 s = P.state[at];
        x0 = s.x; e0 = s.y; x1 = s.z; e1 = s.w;
      }
      if (consume) {
        const float half = 0.5f * (x1 - x0), xm = x0 + half;  // (the point this round's probe evaluated)
        const float em = P.probed[at] - P.mesh.iso;
        if ((em < 0.0f) == (e0 < 0.0f)) { x0 = xm; e0 = em; }
        else { x1 = xm; e1 = em; }
      }
      float t = 0.5f;
      if (last) {
        t = e0 / (e0 - e1);
        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
      } else {
        P.state[at] = make_float4(x0, e0, x1, e1);
      }
      const float span = x1 - x0, step = t * span;
      float p[3];
      p[a] = x0 + step;
      p[b] = pc[b][ob];
      p[cc] = pc[cc][oc];
      point[0] = p[0]; point[1] = p[1]; point[2] = p[2];
    }
  }
  if (last) P.live[v] = live;
}

// one Jacobi rotation of the pair (p, q) of a symmetric 3 x 3 matrix, r the third index, and of the columns p and q of V (the header's text)
__device__ inline void mesh_jacobi(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q, float& v1p, float& v1q, float& v2p,
                                   float& v2q) {
  if (apq == 0.0f) return;
  const float theta = (aqq - app) / (2.0f * apq);
  const float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
  const float cr = 1.0f / sqrtf(t * t + 1.0f), sr = t * cr, h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0f;
  const float rp = cr * arp - sr * arq, rq = sr * arp + cr * arq;
  arp = rp; arq = rq;
  const float w0p = cr * v0p - sr * v0q, w0q = sr * v0p + cr * v0q;
  v0p = w0p; v0q = w0q;
  const float w1p = cr * v1p - sr * v1q, w1q = sr * v1p + cr * v1q;
  v1p = w1p; v1q = w1q;
  const float w2p = cr * v2p - sr * v2q, w2q = sr * v2p + cr * v2q;
  v2p = w2p; v2q = w2q;
}

// The vertex of the quadratic error function of the live slots' planes (point, normal), about their mass point, its small eigenvalues
// truncated, kept inside the cell.  Everything is named scalars: the 3 x 3 state stays in registers.
__global__ __launch_bounds__(256) void rm_mesh_qef_kernel(const MeshSharpParams P) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= P.vertices) return;
  const size_t V = (size_t)P.vertices;
  const unsigned int live = P.live[v];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  int m = 0;
#pragma unroll
  for (int s = 0; s < 12; s++) {
    if (!((live >> s) & 1u)) continue;
    const float* p = P.points + 3 * ((size_t)s * V + (size_t)v);
    sx += p[0]; sy += p[1]; sz += p[2];
    m++;
  }
  const float fm = (float)m;
  const float cx = sx / fm, cy = sy / fm, cz = sz / fm;
  float a00 = 0.0f, a01 = 0.0f, a02 = 0.0f, a11 = 0.0f, a12 = 0.0f, a22 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  int planes = 0;
#pragma unroll
  for (int s = 0; s < 12; s++) {
    if (!((live >> s) & 1u)) continue;
    const size_t at = 3 * ((size_t)s * V + (size_t)v);
    const float nx = P.probed[at], ny = P.probed[at + 1], nz = P.probed[at + 2];
    if (!(isfinite(nx) && isfinite(ny) && isfinite(nz)) || (nx == 0.0f && ny == 0.0f && nz == 0.0f)) continue;
    const float dx = P.points[at] - cx, dy = P.points[at + 1] - cy, dz = P.points[at + 2] - cz;
    const float nd = nx * dx + ny * dy + nz * dz;
    a00 += nx * nx; a01 += nx * ny; a02 += nx * nz; a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
    b0 += nx * nd; b1 += ny * nd; b2 += nz * nd;
    planes++;
  }
  float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll
  for (int sweep = 0; sweep < 5; sweep++) {
    mesh_jacobi(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    mesh_jacobi(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    mesh_jacobi(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  float lmax = a00;
  if (a11 > lmax) lmax = a11;
  if (a22 > lmax) lmax = a22;
  const float bar = P.threshold * lmax;
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  if (a00 > 0.0f && a00 > bar) {
    const float w = (v00 * b0 + v10 * b1 + v20 * b2) / a00;
    ox += v00 * w; oy += v10 * w; oz += v20 * w;
  }
  if (a11 > 0.0f && a11 > bar) {
    const float w = (v01 * b0 + v11 * b1 + v21 * b2) / a11;
    ox += v01 * w; oy += v11 * w; oz += v21 * w;
  }
  if (a22 > 0.0f && a22 > bar) {
    const float w = (v02 * b0 + v12 * b1 + v22 * b2) / a22;
    ox += v02 * w; oy += v12 * w; oz += v22 * w;
  }
  float x = cx + ox, y = cy + oy, z = cz + oz;
  if (planes == 0 || !(isfinite(x) && isfinite(y) && isfinite(z))) { x = cx; y = cy; z = cz; }
  const GridDims& g = P.mesh.grid;
  const int cells_x = g.nc[0] - 1, cells_y = g.nc[1] - 1, cell = (int)P.mesh.cells[v];
  const int i = cell % cells_x, j = (cell / cells_x) % cells_y, k = cell / (cells_x * cells_y);
  const float lx = rm_grid_coord(g, 0, i), hx = rm_grid_coord(g, 0, i + 1), ly = rm_grid_coord(g, 1, j), hy = rm_grid_coord(g, 1, j + 1);
  const float lz = rm_grid_coord(g, 2, k), hz = rm_grid_coord(g, 2, k + 1);
  if (x < lx) x = lx;
  if (x > hx) x = hx;
  if (y < ly) y = ly;
  if (y > hy) y = hy;
  if (z < lz) z = lz;
  if (z > hz) z = hz;
  P.mesh.positions[3 * (size_t)v] = x;
  P.mesh.positions[3 * (size_t)v + 1] = y;
  P.mesh.positions[3 * (size_t)v + 2] = z;
}

// ---- components and islands (include/hip_raymarch.h "components and islands") ---------------------------------------------------------
// A forest over the vertices, parent[v] <= v at every instant: a root is its own parent, and the least vertex of a finished tree.  Parents are
// read with relaxed agent-scope atomic loads -- other workgroups lower them while this one reads -- and only ever lowered, by atomicMin, to a
// vertex of the same component: a stale parent is an older, larger ancestor, so a chase strictly descends and ends by itself.  No thread waits
// for another.  The host repeats hook + flatten until a hook pass met no two roots (rm_mesh_host.inc mesh_label).

__device__ inline unsigned int mesh_link_root(const unsigned int* parent, unsigned int v) {
  for (;;) {
    const unsigned int p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= v) return v;  // (p > v never happens; it would end the chase all the same)
    v = p;
  }
}

// Unite the trees of a and b: the larger root's parent is lowered to the smaller root.  When the larger was no root any more (old != hi), its
// parent is now min(old, lo) and the link to the other of the two may be gone, so old and lo are united in its place: hi is below one of
// them and both are smaller than hi, so this descends too.  Returns whether a and b were in different trees.
__device__ inline bool mesh_link_unite(unsigned int* parent, unsigned int a, unsigned int b) {
  bool met = false;
  for (;;) {
    a = mesh_link_root(parent, a);
    b = mesh_link_root(parent, b);
    if (a == b) return met;
    met = true;
    const unsigned int hi = a > b ? a : b, lo = a > b ? b : a;
    const unsigned int old = atomicMin(parent + hi, lo);
    if (old == hi) return met;
    a = old;
    b = lo;
  }
}

__global__ __launch_bounds__(256) void rm_mesh_link_init_kernel(unsigned int* parent, long long vertices) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < vertices) parent[v] = (unsigned int)v;
}

// one thread per triangle; two of its edges connect its three vertices.  A triangle with an index beyond the mesh links nothing.
__global__ __launch_bounds__(256) void rm_mesh_link_hook_kernel(unsigned int* parent, const unsigned int* triangles, long long vertices, long long n,
                                                                unsigned int* changed) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool met = false;
  if (t < n) {
    const unsigned int a = triangles[3 * t], b = triangles[3 * t + 1], c = triangles[3 * t + 2];
    if (a < vertices && b < vertices && c < vertices) {
      met = mesh_link_unite(parent, a, b);
      met = mesh_link_unite(parent, b, c) || met;
    }
  }
  const unsigned long long any = __ballot(met);  // one store per wave that met two roots
  if (any != 0ull && (int)(threadIdx.x & 63u) == __ffsll((long long)any) - 1) *changed = 1u;
}

__global__ __launch_bounds__(256) void rm_mesh_link_flatten_kernel(unsigned int* parent, long long vertices) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= vertices) return;
  const unsigned int r = mesh_link_root(parent, (unsigned int)v);
  if (r != (unsigned int)v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (roots stay roots in this pass)
}

__global__ __launch_bounds__(256) void rm_mesh_roots_kernel(const unsigned int* parent, unsigned long long* words, long long vertices) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < vertices) words[v] = parent[v] == (unsigned int)v ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void rm_mesh_labels_kernel(const unsigned int* parent, const unsigned long long* scanned, unsigned int* labels,
                                                             long long vertices) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < vertices) labels[v] = (unsigned int)scanned[parent[v]];
}

// the component of vertex i (triangles == NULL) or of triangle i: that of its first vertex
__device__ inline unsigned int mesh_part_of(const unsigned int* labels, const unsigned int* triangles, long long i) {
  return labels[triangles ? triangles[3 * i] : (unsigned int)i];
}

// sizes[2 c + slot] += 1 per element.  Integer adds: any order gives the same sums.  Most of a wave's elements usually lie in one component:
// where all of them do, one lane adds their count.
__global__ __launch_bounds__(256) void rm_mesh_part_sizes_kernel(const unsigned int* labels, const unsigned int* triangles, long long n, unsigned int* sizes,
                                                                 int slot) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < n;
  const unsigned int c = valid ? mesh_part_of(labels, triangles, i) : 0u;
  const unsigned long long lanes = __ballot(valid);
  if (lanes == 0ull) return;
  const int lead = __ffsll((long long)lanes) - 1;
  const unsigned int first = (unsigned int)__shfl((int)c, lead);
  if (__ballot(valid && c == first) == lanes) {
    if ((int)(threadIdx.x & 63u) == lead) atomicAdd(sizes + 2 * (size_t)first + slot, (unsigned int)__popcll(lanes));
  } else if (valid) {
    atomicAdd(sizes + 2 * (size_t)c + slot, 1u);
  }
}

__global__ __launch_bounds__(256) void rm_mesh_keep_flags_kernel(const unsigned int* labels, const unsigned int* triangles, const unsigned int* keep, long long n,
                                                                 unsigned long long* words) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) words[i] = keep[mesh_part_of(labels, triangles, i)] ? 1ull : 0ull;
}

// one thread per source vertex: a kept one copies its rows, as words, to its place among the kept
__global__ __launch_bounds__(256) void rm_mesh_gather_vertices_kernel(const MeshGather G, long long vertices) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= vertices || !G.keep[G.labels[v]]) return;
  const size_t to = (size_t)G.vertex_at[v];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!G.src[a]) continue;
    G.dst[a][3 * to] = G.src[a][3 * v];
    G.dst[a][3 * to + 1] = G.src[a][3 * v + 1];
    G.dst[a][3 * to + 2] = G.src[a][3 * v + 2];
  }
  G.dst[3][to] = G.src[3][v];
}

// one thread per source triangle: a kept one (its vertices are kept with it) goes to its place with its indices renumbered
__global__ __launch_bounds__(256) void rm_mesh_gather_triangles_kernel(const MeshGather G, const unsigned int* triangles, const unsigned long long* triangle_at,
                                                                       long long n, unsigned int* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n || !G.keep[G.labels[triangles[3 * t]]]) return;
  const size_t to = (size_t)triangle_at[t];
  out[3 * to] = (unsigned int)G.vertex_at[triangles[3 * t]];
  out[3 * to + 1] = (unsigned int)G.vertex_at[triangles[3 * t + 1]];
  out[3 * to + 2] = (unsigned int)G.vertex_at[triangles[3 * t + 2]];
}

// ---- simplification: vertex clustering (include/hip_raymarch.h "simplification") ------------------------------------------------------------
// Everything a run can differ in is an integer: the means are sums of Q20 integers (atomic adds commute), the survivor of a class of equal
// triangles is a minimum.  The fp32 around them is this unit's plain arithmetic, every operation rounded on its own.  No thread waits for
// another; the one loop, the table's probe, is bounded by the table's size.

__device__ inline long long mesh_q20(float x) { return (long long)rintf(x * 1048576.0f); }

// a normal's or a colour's component as it is summed: non-finite counts as 0, clamped to [-1024, 1024]
__device__ inline unsigned long long mesh_q20_attribute(float x) {
  if (!isfinite(x)) x = 0.0f;
  if (x < -1024.0f) x = -1024.0f;
  if (x > 1024.0f) x = 1024.0f;
  return (unsigned long long)mesh_q20(x);  // (two's complement: the row's unsigned adds sum it as a signed value)
}

struct MeshCluster {
  unsigned int key;   // (k * ny + j) * nx + i
  unsigned int q[3];  // the position inside the cluster cell, 0 .. 2^20 per axis
};

__device__ inline MeshCluster mesh_cluster(const GridDims& g, const float* p) {
  MeshCluster c;
  int idx[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int n = g.nc[a] - 1;
    const float d = p[a] - g.lo[a], u = d / g.h[a];
    int i;
    if (!(u >= 0.0f)) i = 0;  // (NaN too)
    else if (u >= (float)n) i = n - 1;
    else {
      i = (int)floorf(u);
      if (i > n - 1) i = n - 1;
    }
    float f = u - (float)i;
    if (!(f >= 0.0f)) f = 0.0f;
    if (f > 1.0f) f = 1.0f;
    idx[a] = i;
    c.q[a] = (unsigned int)mesh_q20(f);
  }
  c.key = (unsigned int)((idx[2] * (g.nc[1] - 1) + idx[1]) * (g.nc[0] - 1) + idx[0]);
  return c;
}

__global__ __launch_bounds__(256) void rm_mesh_simplify_mark_kernel(const MeshSimplify S) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < S.vertices) S.marks[mesh_cluster(S.grid, S.positions + 3 * v).key] = 1ull;  // (every writer of a word writes the same)
}

// Behind the scan: marks[key] is the cluster's output vertex.  Vertices stand in ascending source cell order, so neighbouring lanes often share
// a cluster: every run of consecutive lanes with one cluster is summed in the wave first (a segmented shuffle reduction; integer sums, so the
// totals are what one add per vertex gives) and the run's first lane makes the adds.  Every lane of a wave stays to the end: the shuffles read
// all of them; a lane beyond the last vertex is a run of its own that adds nothing.
__global__ __launch_bounds__(256) void rm_mesh_simplify_sums_kernel(const MeshSimplify S) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool valid = v < S.vertices;
  MeshCluster c{};
  unsigned int to = 0xFFFFFFFFu;
  if (valid) {
    c = mesh_cluster(S.grid, S.positions + 3 * v);
    to = (unsigned int)S.marks[c.key];
    S.vertex_to[v] = to;
  }
  const unsigned int before = (unsigned int)__shfl_up((int)to, 1);
  const bool head = lane == 0 || before != to;
  const unsigned long long heads = __ballot(head), above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int last = above != 0ull ? lane + __ffsll((long long)above) - 1 : 63;  // the last lane of this lane's run
  // the count and the q sums of a run fit 32 bits (64 lanes of at most 2^20); the attributes' do not
  unsigned int n = valid ? 1u : 0u, q[3] = {c.q[0], c.q[1], c.q[2]};
  unsigned long long w[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  if (valid && S.normals) {
#pragma unroll
    for (int a = 0; a < 3; a++) w[a] = mesh_q20_attribute(S.normals[3 * v + a]);
  }
  if (valid && S.colours) {
#pragma unroll
    for (int a = 0; a < 3; a++) w[3 + a] = mesh_q20_attribute(S.colours[3 * v + a]);
  }
  const bool wide = S.normals != nullptr || S.colours != nullptr;  // (uniform)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const bool mine = lane + off <= last;
    const unsigned int dn = (unsigned int)__shfl_down((int)n, off);
    if (mine) n += dn;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const unsigned int dq = (unsigned int)__shfl_down((int)q[a], off);
      if (mine) q[a] += dq;
    }
    if (wide) {
#pragma unroll
      for (int a = 0; a < 6; a++) {
        const unsigned long long dw = __shfl_down(w[a], off);
        if (mine) w[a] += dw;
      }
    }
  }
  if (!head || !valid) return;
  S.out_cells[to] = c.key;  // (the same from every run of the cluster)
  unsigned long long* row = S.sums + (size_t)to * (size_t)S.row;
  atomicAdd(row, (unsigned long long)n);
#pragma unroll
  for (int a = 0; a < 3; a++) atomicAdd(row + 1 + a, (unsigned long long)q[a]);
  int at = 4;
  if (S.normals) {
#pragma unroll
    for (int a = 0; a < 3; a++) atomicAdd(row + at + a, w[a]);
    at += 3;
  }
  if (S.colours) {
#pragma unroll
    for (int a = 0; a < 3; a++) atomicAdd(row + at + a, w[3 + a]);
  }
}

__device__ inline float mesh_q20_mean(unsigned long long sum, double count_q20) { return (float)((double)(long long)sum / count_q20); }

__global__ __launch_bounds__(256) void rm_mesh_simplify_place_kernel(const MeshSimplify S) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= S.out_vertices) return;
  const GridDims& g = S.grid;
  const unsigned long long* row = S.sums + (size_t)o * (size_t)S.row;
  const double m = (double)row[0] * 1048576.0;
  const int nx = g.nc[0] - 1, ny = g.nc[1] - 1, key = (int)S.out_cells[o];
  const int idx[3] = {key % nx, (key / nx) % ny, key / (nx * ny)};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float s = (float)idx[a] + mesh_q20_mean(row[1 + a], m), step = s * g.h[a];
    S.out_positions[3 * o + a] = g.lo[a] + step;
  }
  int at = 4;
  if (S.out_normals) {
    const float x = mesh_q20_mean(row[at], m), y = mesh_q20_mean(row[at + 1], m), z = mesh_q20_mean(row[at + 2], m);
    const float xx = x * x, yy = y * y, zz = z * z, xy = xx + yy, len = sqrtf(xy + zz);
    const bool none = len == 0.0f || !isfinite(len);
    S.out_normals[3 * o] = none ? 0.0f : x / len;
    S.out_normals[3 * o + 1] = none ? 0.0f : y / len;
    S.out_normals[3 * o + 2] = none ? 0.0f : z / len;
    at += 3;
  }
  if (S.out_colours) {
#pragma unroll
    for (int a = 0; a < 3; a++) S.out_colours[3 * o + a] = mesh_q20_mean(row[at + a], m);
  }
}

// one thread per triangle, and one more for the word behind the last: the scan's total lands there, so "kept" reads as words[t + 1] != words[t].
// A triangle with an index beyond the mesh (none of this library's has one) is dropped.
__global__ __launch_bounds__(256) void rm_mesh_simplify_map_kernel(const MeshSimplify S) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t > S.triangles) return;
  if (t == S.triangles) { S.words[t] = 0ull; return; }
  const unsigned int a = S.source_triangles[3 * t], b = S.source_triangles[3 * t + 1], c = S.source_triangles[3 * t + 2];
  const bool valid = a < S.vertices && b < S.vertices && c < S.vertices;
  const unsigned int ma = valid ? S.vertex_to[a] : 0u, mb = valid ? S.vertex_to[b] : 0u, mc = valid ? S.vertex_to[c] : 0u;
  S.mapped[3 * t] = ma;
  S.mapped[3 * t + 1] = mb;
  S.mapped[3 * t + 2] = mc;
  S.words[t] = (ma != mb && mb != mc && ma != mc) ? 1ull : 0ull;
}

// the smallest index in front, the cyclic order kept (the three differ)
struct MeshTriple {
  unsigned int a, b, c;
};
__device__ inline MeshTriple mesh_canonical(const unsigned int* m) {
  const unsigned int x = m[0], y = m[1], z = m[2];
  if (x < y && x < z) return MeshTriple{x, y, z};
  if (y < z) return MeshTriple{y, z, x};
  return MeshTriple{z, x, y};
}

__global__ __launch_bounds__(256) void rm_mesh_simplify_insert_kernel(const MeshSimplify S) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= S.triangles || S.words[t] == 0ull) return;
  const MeshTriple mine = mesh_canonical(S.mapped + 3 * t);
  unsigned long long h = (mine.a * 0x9E3779B97F4A7C15ull) ^ (mine.b * 0xC2B2AE3D27D4EB4Full) ^ (mine.c * 0x165667B19E3779F9ull);
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  const unsigned long long mask = S.slots - 1ull;
  unsigned long long slot = h & mask;
  for (unsigned long long probe = 0; probe < S.slots; probe++, slot = (slot + 1ull) & mask) {
    unsigned int held = __hip_atomic_load(S.table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (held == 0xFFFFFFFFu) {
      held = atomicCAS(S.table + slot, 0xFFFFFFFFu, (unsigned int)t);
      if (held == 0xFFFFFFFFu) { S.words[t] = slot + 1ull; return; }
    }
    // whoever holds the slot is of the class that claimed it: any of them tells which
    const MeshTriple theirs = mesh_canonical(S.mapped + 3 * (size_t)held);
    if (theirs.a == mine.a && theirs.b == mine.b && theirs.c == mine.c) {
      atomicMin(S.table + slot, (unsigned int)t);
      S.words[t] = slot + 1ull;
      return;
    }
  }
  S.words[t] = 0ull;
  *S.error = 1u;
}

__global__ __launch_bounds__(256) void rm_mesh_simplify_keep_kernel(const MeshSimplify S) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= S.triangles) return;
  const unsigned long long at = S.words[t];
  S.words[t] = (at != 0ull && S.table[at - 1ull] == (unsigned int)t) ? 1ull : 0ull;
}

// (named with rm_mesh_take3_kernel's caution: the lengths of the kernel names decide whether llvm-objdump -D reads this code object whole)
__global__ __launch_bounds__(256) void rm_mesh_simplify_take_kernel(const MeshSimplify S) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= S.triangles) return;
  const size_t to = (size_t)S.words[t];
  if (S.words[t + 1] == to) return;
  S.out_triangles[3 * to] = S.mapped[3 * t];
  S.out_triangles[3 * to + 1] = S.mapped[3 * t + 1];
  S.out_triangles[3 * to + 2] = S.mapped[3 * t + 2];
}

// ---- quadric placement (include/hip_raymarch.h "quadric placement") ---------------------------------------------------------------------------
// Behind the sums and the place kernel: vertex_to and the rows of the means are final.  Again everything a run can differ in is an integer: the
// plane quadrics are sums of Q24 integers per cluster, ten 64-bit words a row (a00 a01 a02 a11 a12 a22 b0 b1 b2 planes).

__device__ inline long long mesh_q24(float x) { return (long long)rintf(x * 16777216.0f); }

// One corner slot of every lane of a wave into the rows: `to` is the slot's output vertex (0xFFFFFFFF: an empty slot), `planes` the corners it
// stands for, r.. the Q24 terms times that count.  Source triangles stand in cell order, so neighbouring lanes often meet in a cluster: every run
// of consecutive lanes with one `to` is summed in the wave first (the segmented shuffle reduction of the sums kernel; integer sums, so the totals
// are what one add per corner gives) and the run's first lane makes the ten adds.  Of a run of at most 64 lanes the six sums of A and the count
// fit 32 bits (|m_i m_j| <= 1: 192 terms of at most 2^24, the mixed ones signed and at most half that); the sums of b do not.  Every lane of
// the wave calls this and stays to the end of the shuffles.
__device__ inline void mesh_quadric_run_add(unsigned long long* quadrics, int lane, unsigned int to, unsigned int planes, unsigned int r00, int r01, int r02,
                                            unsigned int r11, int r12, unsigned int r22, long long rb0, long long rb1, long long rb2) {
  const unsigned int before = (unsigned int)__shfl_up((int)to, 1);
  const bool head = lane == 0 || before != to;
  const unsigned long long heads = __ballot(head), above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int last = above != 0ull ? lane + __ffsll((long long)above) - 1 : 63;  // the last lane of this lane's run
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const bool mine = lane + off <= last;
    const unsigned int dn = (unsigned int)__shfl_down((int)planes, off);
    const unsigned int d00 = (unsigned int)__shfl_down((int)r00, off), d11 = (unsigned int)__shfl_down((int)r11, off);
    const unsigned int d22 = (unsigned int)__shfl_down((int)r22, off);
    const int d01 = __shfl_down(r01, off), d02 = __shfl_down(r02, off), d12 = __shfl_down(r12, off);
    const long long db0 = __shfl_down(rb0, off), db1 = __shfl_down(rb1, off), db2 = __shfl_down(rb2, off);
    if (mine) {
      planes += dn; r00 += d00; r11 += d11; r22 += d22;
      r01 += d01; r02 += d02; r12 += d12;
      rb0 += db0; rb1 += db1; rb2 += db2;
    }
  }
  if (!head || to == 0xFFFFFFFFu) return;
  unsigned long long* row = quadrics + (size_t)to * 10u;
  atomicAdd(row, (unsigned long long)r00);
  atomicAdd(row + 1, (unsigned long long)(long long)r01);  // (two's complement: the unsigned adds sum signed values)
  atomicAdd(row + 2, (unsigned long long)(long long)r02);
  atomicAdd(row + 3, (unsigned long long)r11);
  atomicAdd(row + 4, (unsigned long long)(long long)r12);
  atomicAdd(row + 5, (unsigned long long)r22);
  atomicAdd(row + 6, (unsigned long long)rb0);
  atomicAdd(row + 7, (unsigned long long)rb1);
  atomicAdd(row + 8, (unsigned long long)rb2);
  atomicAdd(row + 9, (unsigned long long)planes);
}

// One thread per source triangle: its plane once, then one term per corner for the corner's cluster.  The corners that share a cluster are merged
// in registers first, which leaves one to three slots (cluster, corners, sums of b); then the wave merges each slot with its neighbours'.  A lane
// beyond the last triangle, or with a triangle that contributes nothing, has three empty slots.
// (rm_mesh_take3_kernel's caution holds here too: these kernels' mangled names, their parameter type included, decide whether llvm-objdump -D
// reads this code object whole)
__global__ __launch_bounds__(256) void rm_mesh_quadric_sums_kernel(const MeshQuadric S) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  bool contributes = false;
  unsigned int o[3] = {0u, 0u, 0u};
  unsigned int a00 = 0u, a11 = 0u, a22 = 0u;
  int a01 = 0, a02 = 0, a12 = 0;
  long long b[3][3] = {{0ll, 0ll, 0ll}, {0ll, 0ll, 0ll}, {0ll, 0ll, 0ll}};
  if (t < S.triangles) {
    const unsigned int i[3] = {S.source_triangles[3 * t], S.source_triangles[3 * t + 1], S.source_triangles[3 * t + 2]};
    if (i[0] < S.vertices && i[1] < S.vertices && i[2] < S.vertices) {
      const float* p0 = S.positions + 3 * (size_t)i[0];
      const float* p1 = S.positions + 3 * (size_t)i[1];
      const float* p2 = S.positions + 3 * (size_t)i[2];
      const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
      const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
      const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
      const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
      if (len > 0.0f && isfinite(len)) {
        contributes = true;
        const float m0 = (cx / len) * S.scale[0], m1 = (cy / len) * S.scale[1], m2 = (cz / len) * S.scale[2];
        a00 = (unsigned int)mesh_q24(m0 * m0); a11 = (unsigned int)mesh_q24(m1 * m1); a22 = (unsigned int)mesh_q24(m2 * m2);
        a01 = (int)mesh_q24(m0 * m1); a02 = (int)mesh_q24(m0 * m2); a12 = (int)mesh_q24(m1 * m2);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const MeshCluster c = mesh_cluster(S.grid, S.positions + 3 * (size_t)i[k]);
          o[k] = S.vertex_to[i[k]];
          const unsigned long long* row = S.sums + (size_t)o[k] * (size_t)S.row;
          const double count = (double)row[0] * 1048576.0;
          const float d0 = (float)c.q[0] / 1048576.0f - mesh_q20_mean(row[1], count);
          const float d1 = (float)c.q[1] / 1048576.0f - mesh_q20_mean(row[2], count);
          const float d2 = (float)c.q[2] / 1048576.0f - mesh_q20_mean(row[3], count);
          const float md = (m0 * d0 + m1 * d1) + m2 * d2;
          b[k][0] = mesh_q24(m0 * md); b[k][1] = mesh_q24(m1 * md); b[k][2] = mesh_q24(m2 * md);
        }
      }
    }
  }
  // corners of one cluster: corner 1 into 0, corner 2 into 0 or 1; n[k] = the corners that row k now stands for
  unsigned int n[3] = {contributes ? 1u : 0u, contributes ? 1u : 0u, contributes ? 1u : 0u};
  if (contributes && o[1] == o[0]) {
    b[0][0] += b[1][0]; b[0][1] += b[1][1]; b[0][2] += b[1][2];
    n[0] += 1u; n[1] = 0u;
  }
  if (contributes && o[2] == o[0]) {
    b[0][0] += b[2][0]; b[0][1] += b[2][1]; b[0][2] += b[2][2];
    n[0] += 1u; n[2] = 0u;
  } else if (contributes && n[1] != 0u && o[2] == o[1]) {
    b[1][0] += b[2][0]; b[1][1] += b[2][1]; b[1][2] += b[2][2];
    n[1] += 1u; n[2] = 0u;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned int times = n[k];
    mesh_quadric_run_add(S.quadrics, lane, times != 0u ? o[k] : 0xFFFFFFFFu, times, times * a00, (int)times * a01, (int)times * a02, times * a11, (int)times * a12,
                         times * a22, b[k][0], b[k][1], b[k][2]);
  }
}

__device__ inline float mesh_q24_value(unsigned long long sum) { return (float)((double)(long long)sum / 16777216.0); }

// One thread per output vertex with planes: the truncated solve of "sharp vertices" step 5 on the cluster's sums, about the mean fractions g that
// the place kernel used, clamped to the cluster cell; the position is overwritten.  A vertex without planes keeps the place kernel's.  The 3 x 3
// state is named scalars, as in rm_mesh_qef_kernel.
__global__ __launch_bounds__(256) void rm_mesh_quadric_place_kernel(const MeshQuadric S) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= S.out_vertices) return;
  const unsigned long long* sums = S.quadrics + (size_t)o * 10u;
  if (sums[9] == 0ull) return;
  float a00 = mesh_q24_value(sums[0]), a01 = mesh_q24_value(sums[1]), a02 = mesh_q24_value(sums[2]);
  float a11 = mesh_q24_value(sums[3]), a12 = mesh_q24_value(sums[4]), a22 = mesh_q24_value(sums[5]);
  const float b0 = mesh_q24_value(sums[6]), b1 = mesh_q24_value(sums[7]), b2 = mesh_q24_value(sums[8]);
  float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll
  for (int sweep = 0; sweep < 5; sweep++) {
    mesh_jacobi(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    mesh_jacobi(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    mesh_jacobi(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  float lmax = a00;
  if (a11 > lmax) lmax = a11;
  if (a22 > lmax) lmax = a22;
  const float bar = S.threshold * lmax;
  float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
  if (a00 > 0.0f && a00 > bar) {
    const float w = (v00 * b0 + v10 * b1 + v20 * b2) / a00;
    w0 += v00 * w; w1 += v10 * w; w2 += v20 * w;
  }
  if (a11 > 0.0f && a11 > bar) {
    const float w = (v01 * b0 + v11 * b1 + v21 * b2) / a11;
    w0 += v01 * w; w1 += v11 * w; w2 += v21 * w;
  }
  if (a22 > 0.0f && a22 > bar) {
    const float w = (v02 * b0 + v12 * b1 + v22 * b2) / a22;
    w0 += v02 * w; w1 += v12 * w; w2 += v22 * w;
  }
  const GridDims& g = S.grid;
  const unsigned long long* row = S.sums + (size_t)o * (size_t)S.row;
  const double count = (double)row[0] * 1048576.0;
  const float g0 = mesh_q20_mean(row[1], count), g1 = mesh_q20_mean(row[2], count), g2 = mesh_q20_mean(row[3], count);
  float x[3] = {g0 + w0, g1 + w1, g2 + w2};
  if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) { x[0] = g0; x[1] = g1; x[2] = g2; }
  const int nx = g.nc[0] - 1, ny = g.nc[1] - 1, key = (int)S.out_cells[o];
  const int idx[3] = {key % nx, (key / nx) % ny, key / (nx * ny)};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (x[a] < 0.0f) x[a] = 0.0f;
    if (x[a] > 1.0f) x[a] = 1.0f;
    const float s = (float)idx[a] + x[a], step = s * g.h[a];
    S.out_positions[3 * o + a] = g.lo[a] + step;
  }
}

// ---- measures and edge topology (include/hip_raymarch.h "measures and edge topology") -------------------------------------------------------
// Everything a run can differ in is an integer sum, a minimum or a maximum; the doubles are summed by a tree whose shape depends on T alone.
// No thread waits for another; the one loop, the table's probe, is bounded by the table's size.  A triangle with a repeated index or one beyond
// the mesh is looked at no further than its three indices.

// lanes of this wave for which `flag` holds, added to *word by the wave's first lane (every lane of the wave calls this)
__device__ inline void mesh_measure_count(unsigned long long* word, bool flag) {
  const unsigned long long lanes = __ballot(flag);
  if (lanes != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(word, (unsigned long long)__popcll(lanes));
}

// one use of the directed edge from -> to
__device__ inline void mesh_measure_edge(const MeshMeasure& M, unsigned int from, unsigned int to) {
  const bool forward = from < to;
  const unsigned long long key = forward ? ((unsigned long long)from << 32 | to) : ((unsigned long long)to << 32 | from);
  unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  const unsigned long long mask = M.slots - 1ull;
  unsigned long long slot = h & mask;
  for (unsigned long long probe = 0; probe < M.slots; probe++, slot = (slot + 1ull) & mask) {
    unsigned long long held = __hip_atomic_load(M.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (held == ~0ull) {
      held = atomicCAS(M.keys + slot, ~0ull, key);
      if (held == ~0ull) held = key;
    }
    if (held == key) {
      atomicAdd(M.counts + slot, forward ? 1ull : 1ull << 32);
      return;
    }
  }
  M.totals[RM_MEASURE_ERROR] = 1ull;  // (every writer writes the same)
}

__global__ __launch_bounds__(256) void rm_mesh_measure_edges_kernel(const MeshMeasure M) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = t < M.triangles;
  unsigned int a = 0u, b = 0u, c = 0u;
  if (valid) { a = M.corners[3 * t]; b = M.corners[3 * t + 1]; c = M.corners[3 * t + 2]; }
  const bool takes_part = valid && a < M.vertices && b < M.vertices && c < M.vertices && a != b && b != c && a != c;
  mesh_measure_count(M.totals + RM_MEASURE_SKIPPED, valid && !takes_part);
  if (!takes_part) return;
  M.used[a] = 1u;  // (every writer of a flag writes the same)
  M.used[b] = 1u;
  M.used[c] = 1u;
  mesh_measure_edge(M, a, b);
  mesh_measure_edge(M, b, c);
  mesh_measure_edge(M, c, a);
}

// One thread per slot.  The five totals are counted over the wave and added once; the component rows too where all the wave's edges lie in
// one component (a mesh of one body: every wave), else every edge adds to its own row.
__global__ __launch_bounds__(256) void rm_mesh_measure_classes_kernel(const MeshMeasure M) {
  const unsigned long long slot = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long key = slot < M.slots ? M.keys[slot] : ~0ull;
  const bool edge = key != ~0ull;
  const unsigned long long lanes = __ballot(edge);
  if (lanes == 0ull) return;
  unsigned int part = 0u;
  bool boundary = false, regular = false, irregular = false, unbalanced = false;
  if (edge) {
    const unsigned long long uses = M.counts[slot];
    const unsigned long long f = uses & 0xFFFFFFFFull, r = uses >> 32;
    boundary = f + r == 1ull;
    regular = f == 1ull && r == 1ull;
    irregular = !boundary && !regular;
    unbalanced = f + r >= 2ull && f != r;
    part = M.labels[(unsigned int)(key >> 32)];
  }
  const unsigned long long n_boundary = (unsigned long long)__popcll(__ballot(boundary)), n_regular = (unsigned long long)__popcll(__ballot(regular));
  const unsigned long long n_irregular = (unsigned long long)__popcll(__ballot(irregular)), n_unbalanced = (unsigned long long)__popcll(__ballot(unbalanced));
  const int lane = (int)(threadIdx.x & 63u), lead = __ffsll((long long)lanes) - 1;
  const unsigned int first = (unsigned int)__shfl((int)part, lead);
  const bool together = __ballot(edge && part == first) == lanes;
  if (lane == lead) {
    atomicAdd(M.totals + RM_MEASURE_EDGES, (unsigned long long)__popcll(lanes));
    if (n_boundary) atomicAdd(M.totals + RM_MEASURE_BOUNDARY, n_boundary);
    if (n_regular) atomicAdd(M.totals + RM_MEASURE_REGULAR, n_regular);
    if (n_irregular) atomicAdd(M.totals + RM_MEASURE_IRREGULAR, n_irregular);
    if (n_unbalanced) atomicAdd(M.totals + RM_MEASURE_UNBALANCED, n_unbalanced);
  }
  unsigned long long* row = M.rows + 4 * (size_t)part;
  if (together) {
    if (lane != lead) return;
    atomicAdd(row, (unsigned long long)__popcll(lanes));
    if (n_boundary) atomicAdd(row + 1, n_boundary);
    if (n_irregular) atomicAdd(row + 2, n_irregular);
    if (n_unbalanced) atomicAdd(row + 3, n_unbalanced);
  } else if (edge) {
    atomicAdd(row, 1ull);
    if (boundary) atomicAdd(row + 1, 1ull);
    if (irregular) atomicAdd(row + 2, 1ull);
    if (unbalanced) atomicAdd(row + 3, 1ull);
  }
}

__global__ __launch_bounds__(256) void rm_mesh_measure_used_kernel(const MeshMeasure M) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  mesh_measure_count(M.totals + RM_MEASURE_USED, v < M.vertices && M.used[v] != 0u);
}

// a float's bits as an unsigned integer that orders as the floats do (-0 below +0; NaN is never coded), and back
__device__ inline unsigned int mesh_measure_code(float x) {
  const unsigned int u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float mesh_measure_decode(unsigned int c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7FFFFFFFu) : ~c); }

// One thread per vertex: the finite ones are counted, and their coordinates' codes reduced over the wave by integer minima and maxima, then one
// atomicMin / atomicMax per wave and word.  A lane without a finite vertex holds the identities.
__global__ __launch_bounds__(256) void rm_mesh_measure_extent_kernel(const MeshMeasure M) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  bool finite = false;
  if (v < M.vertices) {
    const float x = M.positions[3 * v], y = M.positions[3 * v + 1], z = M.positions[3 * v + 2];
    finite = isfinite(x) && isfinite(y) && isfinite(z);
    if (finite) {
      lo[0] = hi[0] = mesh_measure_code(x);
      lo[1] = hi[1] = mesh_measure_code(y);
      lo[2] = hi[2] = mesh_measure_code(z);
    }
  }
  const unsigned long long lanes = __ballot(finite);
  if (lanes == 0ull) return;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const unsigned int l = (unsigned int)__shfl_xor((int)lo[a], m), h = (unsigned int)__shfl_xor((int)hi[a], m);
      if (l < lo[a]) lo[a] = l;
      if (h > hi[a]) hi[a] = h;
    }
  }
  if ((threadIdx.x & 63u) != 0u) return;
  atomicAdd(M.totals + RM_MEASURE_FINITE, (unsigned long long)__popcll(lanes));
  unsigned int* extent = reinterpret_cast<unsigned int*>(M.totals + RM_MEASURE_EXTENT);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    atomicMin(extent + a, lo[a]);
    atomicMax(extent + 3 + a, hi[a]);
  }
}

// the stated tree over a workgroup's 256 values of each list: for off = 128 .. 1, s[i] = s[i] + s[i + off] for i < off; s[0] holds the sum
__device__ inline void mesh_measure_tree(double (*s)[256]) {
  for (int off = 128; off >= 1; off >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < off) {
      s[0][threadIdx.x] = s[0][threadIdx.x] + s[0][threadIdx.x + off];
      s[1][threadIdx.x] = s[1][threadIdx.x] + s[1][threadIdx.x + off];
    }
  }
}

// One thread per triangle: its two terms in double, every operation rounded on its own (this unit is built without contraction; '/' and sqrt
// are IEEE in double), +0.0 for a triangle that is not measured and for the places behind the last; then the first level of the tree.
__global__ __launch_bounds__(256) void rm_mesh_measure_terms_kernel(const MeshMeasure M, double* area, double* volume) {
  __shared__ double s[2][256];
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  double area_t = 0.0, volume_t = 0.0;
  bool unmeasured = false;
  if (t < M.triangles) {
    const unsigned int i0 = M.corners[3 * t], i1 = M.corners[3 * t + 1], i2 = M.corners[3 * t + 2];
    if (i0 < M.vertices && i1 < M.vertices && i2 < M.vertices && i0 != i1 && i1 != i2 && i0 != i2) {
      const float* p0 = M.positions + 3 * (size_t)i0;
      const float* p1 = M.positions + 3 * (size_t)i1;
      const float* p2 = M.positions + 3 * (size_t)i2;
      const float q[9] = {p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2]};
      bool finite = true;
#pragma unroll
      for (int k = 0; k < 9; k++) finite = finite && isfinite(q[k]);
      unmeasured = !finite;
      if (finite) {
        // (a measured triangle has finite vertices: the extent is there)
        const unsigned int* extent = reinterpret_cast<const unsigned int*>(M.totals + RM_MEASURE_EXTENT);
        const double ox = (double)(mesh_measure_decode(extent[0]) + 0.0f), oy = (double)(mesh_measure_decode(extent[1]) + 0.0f);
        const double oz = (double)(mesh_measure_decode(extent[2]) + 0.0f);
        const double ax = (double)q[0] - ox, ay = (double)q[1] - oy, az = (double)q[2] - oz;
        const double bx = (double)q[3] - ox, by = (double)q[4] - oy, bz = (double)q[5] - oz;
        const double cx = (double)q[6] - ox, cy = (double)q[7] - oy, cz = (double)q[8] - oz;
        const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        area_t = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
        const double mx = by * cz - bz * cy, my = bz * cx - bx * cz, mz = bx * cy - by * cx;
        volume_t = ((ax * mx + ay * my) + az * mz) / 6.0;
      }
    }
  }
  mesh_measure_count(M.totals + RM_MEASURE_UNMEASURED, unmeasured);
  s[0][threadIdx.x] = area_t;
  s[1][threadIdx.x] = volume_t;
  mesh_measure_tree(s);
  if (threadIdx.x == 0u) { area[blockIdx.x] = s[0][0]; volume[blockIdx.x] = s[1][0]; }
}

// one further level: workgroup g sums values [256 g, 256 g + 256) of each list, +0.0 behind the last
__global__ __launch_bounds__(256) void rm_mesh_measure_sum_kernel(const double* area, const double* volume, long long n, double* out_area, double* out_volume) {
  __shared__ double s[2][256];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  s[0][threadIdx.x] = i < n ? area[i] : 0.0;
  s[1][threadIdx.x] = i < n ? volume[i] : 0.0;
  mesh_measure_tree(s);
  if (threadIdx.x == 0u) { out_area[blockIdx.x] = s[0][0]; out_volume[blockIdx.x] = s[1][0]; }
}

// ---- projection: the step and the report (include/hip_raymarch.h "projection onto the surface") ---------------------------------------------
// The scene is evaluated by rm_mesh_project_eval_kernel between these launches (rm_mesh_host.inc rm_mesh_project); this kernel only consumes
// its output, in this unit's plain fp32: every operation rounded on its own.  One thread per vertex, and every thread of a workgroup stays to
// the end: the ballots and the tree read all of them.  What a run can differ in is an integer sum or a maximum; the doubles go through the
// measures' fixed tree.
__global__ __launch_bounds__(256) void rm_mesh_project_step_kernel(const MeshProject S, int round, double* sum, double* sum2) {
  __shared__ double s[2][256];
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = v < S.vertices;
  float e = 0.0f;
  bool finite = false, moved = false;
  if (valid) {
    e = S.d[v] - S.iso;
    finite = isfinite(e);
  }
  if (round >= 0) {
    if (valid && finite && fabsf(e) > S.tolerance) {
      const float nx = S.normals[3 * v], ny = S.normals[3 * v + 1], nz = S.normals[3 * v + 2];
      unsigned int flags = 0u;
      if (!(isfinite(nx) && isfinite(ny) && isfinite(nz)) || (nx == 0.0f && ny == 0.0f && nz == 0.0f)) {
        flags = RM_PROJECT_FLAG_UNDIRECTED;
      } else {
        const float step = e * S.relax;
        const float n[3] = {nx, ny, nz};
        float p[3], q[3];
        bool clamped = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          p[c] = S.positions[3 * v + c];
          const float along = n[c] * step;
          q[c] = p[c] - along;
          if (S.reach > 0.0f) {
            const float p0 = S.source[3 * v + c], lo = p0 - S.reach, hi = p0 + S.reach;
            if (q[c] < lo) { q[c] = lo; clamped = true; }
            if (q[c] > hi) { q[c] = hi; clamped = true; }
          }
        }
        if (clamped) flags = RM_PROJECT_FLAG_CLAMPED;
        if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) {
#pragma unroll
          for (int c = 0; c < 3; c++) {
            moved = moved || __float_as_uint(q[c]) != __float_as_uint(p[c]);
            S.positions[3 * v + c] = q[c];
          }
        }
      }
      if (flags != 0u) S.flags[v] |= flags;  // (the vertex is this thread's alone)
    }
    mesh_measure_count(S.totals + RM_PROJECT_MOVED + round, moved);
    if (round > 0) return;  // (the whole workgroup)
  } else {
    unsigned int flags = 0u;
    if (valid) {
      S.residual[v] = e;
      flags = S.flags[v];
      moved = __float_as_uint(S.positions[3 * v]) != __float_as_uint(S.source[3 * v]) ||
              __float_as_uint(S.positions[3 * v + 1]) != __float_as_uint(S.source[3 * v + 1]) ||
              __float_as_uint(S.positions[3 * v + 2]) != __float_as_uint(S.source[3 * v + 2]);
    }
    mesh_measure_count(S.totals + RM_PROJECT_CLAMPED, (flags & RM_PROJECT_FLAG_CLAMPED) != 0u);
    mesh_measure_count(S.totals + RM_PROJECT_UNDIRECTED, (flags & RM_PROJECT_FLAG_UNDIRECTED) != 0u);
    mesh_measure_count(S.totals + RM_PROJECT_MOVED_VERTICES, moved);
  }
  // a half of the report: round 0 the one before, round -1 the one after
  const int after = round < 0 ? 1 : 0;
  mesh_measure_count(S.totals + RM_PROJECT_SETTLED_BEFORE + after, valid && finite && fabsf(e) <= S.tolerance);
  mesh_measure_count(S.totals + RM_PROJECT_NONFINITE_BEFORE + after, valid && !finite);
  unsigned long long key = valid && finite ? ((unsigned long long)__float_as_uint(fabsf(e)) << 32 | (0xFFFFFFFFull - (unsigned long long)v)) : 0ull;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long other = __shfl_xor(key, m);
    if (other > key) key = other;
  }
  if ((threadIdx.x & 63u) == 0u && key != 0ull) atomicMax(S.totals + RM_PROJECT_KEY_BEFORE + after, key);
  s[0][threadIdx.x] = valid && finite ? (double)fabsf(e) : 0.0;
  s[1][threadIdx.x] = valid && finite ? (double)e * (double)e : 0.0;
  mesh_measure_tree(s);
  if (threadIdx.x == 0u) { sum[blockIdx.x] = s[0][0]; sum2[blockIdx.x] = s[1][0]; }
}

// One thread per triangle with three indices < V: the cross products of "quadric placement" step 2 on the source and on the final positions;
// flipped iff their dot product is < 0 (a NaN is not).
__device__ inline void mesh_project_cross(const float* positions, unsigned int i0, unsigned int i1, unsigned int i2, float* c) {
  const float* p0 = positions + 3 * (size_t)i0;
  const float* p1 = positions + 3 * (size_t)i1;
  const float* p2 = positions + 3 * (size_t)i2;
  const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  c[0] = e1y * e2z - e1z * e2y;
  c[1] = e1z * e2x - e1x * e2z;
  c[2] = e1x * e2y - e1y * e2x;
}
__global__ __launch_bounds__(256) void rm_mesh_project_flips_kernel(const MeshProject S) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool flipped = false;
  if (t < S.triangles) {
    const unsigned int i0 = S.corners[3 * t], i1 = S.corners[3 * t + 1], i2 = S.corners[3 * t + 2];
    if (i0 < S.vertices && i1 < S.vertices && i2 < S.vertices) {
      float c0[3], c1[3];
      mesh_project_cross(S.source, i0, i1, i2, c0);
      mesh_project_cross(S.positions, i0, i1, i2, c1);
      const float dot = (c0[0] * c1[0] + c0[1] * c1[1]) + c0[2] * c1[2];
      flipped = dot < 0.0f;
    }
  }
  mesh_measure_count(S.totals + RM_PROJECT_FLIPPED, flipped);
}

// ---- deviation: per triangle and the report's terms (include/hip_raymarch.h "deviation") -------------------------------------------------------
// The scene is evaluated by rm_mesh_deviation_eval_kernel ahead of this launch; this kernel only consumes d, in this unit's plain fp32 and
// double, so that no unit's denormal mode touches e, |e| or the squares.  One lane per sample, the eval kernel's lanes; every lane stays to the
// end: the butterflies over a triangle's S lanes and the wave's ballots read all of them.  The triangle's first lane computes the area, writes
// max_t and the four terms (the fixed tree is rm_mesh_measure_sum_kernel's, launched by the host) and holds the key of the wave's maximum.
__global__ __launch_bounds__(256) void rm_mesh_deviation_reduce_kernel(const MeshDeviation D) {
  const unsigned int lanes = (unsigned int)D.triangles << D.log2_samples;  // < 2^31
  const unsigned int S = 1u << D.log2_samples;
  const unsigned int gi = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = gi < lanes;
  const unsigned int t = valid ? gi >> D.log2_samples : 0u;
  const bool first = valid && (gi & (S - 1u)) == 0u;
  unsigned int i0 = 0u, i1 = 0u, i2 = 0u;
  bool live = false;
  if (valid) {
    i0 = D.corners[3 * (size_t)t];
    i1 = D.corners[3 * (size_t)t + 1];
    i2 = D.corners[3 * (size_t)t + 2];
    live = (long long)i0 < D.vertices && (long long)i1 < D.vertices && (long long)i2 < D.vertices;
  }
  float e = 0.0f;
  bool finite = false;
  if (live) {
    e = D.d[gi] - D.iso;
    finite = isfinite(e);
  }
  unsigned int largest = finite ? __float_as_uint(fabsf(e)) : 0u;  // (the bits of non-negative floats order as the floats do)
  double s1 = finite ? (double)e : 0.0, s2 = finite ? (double)e * (double)e : 0.0;
  unsigned int F = finite ? 1u : 0u;
#pragma unroll
  for (unsigned int m = 1u; m < 64u; m <<= 1) {
    if (m < S) {  // (the same for every lane)
      const unsigned int other = (unsigned int)__shfl_xor((int)largest, (int)m);
      if (other > largest) largest = other;
      s1 = s1 + __shfl_xor(s1, (int)m);
      s2 = s2 + __shfl_xor(s2, (int)m);
      F += (unsigned int)__shfl_xor((int)F, (int)m);
    }
  }
  const bool evaluated = first && live && F == S;
  bool over = false;
  unsigned long long key = 0ull;
  if (first) {
    double area_t = 0.0;
    const float max_t = live ? __uint_as_float(largest) : 0.0f;
    if (evaluated) {
      const float* p0 = D.positions + 3 * (size_t)i0;
      const float* p1 = D.positions + 3 * (size_t)i1;
      const float* p2 = D.positions + 3 * (size_t)i2;
      const double ax = (double)p0[0], ay = (double)p0[1], az = (double)p0[2];
      const double e1x = (double)p1[0] - ax, e1y = (double)p1[1] - ay, e1z = (double)p1[2] - az;
      const double e2x = (double)p2[0] - ax, e2y = (double)p2[1] - ay, e2z = (double)p2[2] - az;
      const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
      area_t = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
      over = max_t > D.tolerance;
      key = (unsigned long long)largest << 32 | (0xFFFFFFFFull - (unsigned long long)t);
    }
    const double mean_t = s1 / (double)S, ms_t = s2 / (double)S;
    const size_t T = (size_t)D.triangles;
    D.triangle_max[t] = max_t;
    D.terms[t] = evaluated ? area_t : 0.0;
    D.terms[T + t] = over ? area_t : 0.0;
    D.terms[2 * T + t] = evaluated ? area_t * mean_t : 0.0;
    D.terms[3 * T + t] = evaluated ? area_t * ms_t : 0.0;
  }
  // a wave's atomics go to one of RM_DEVIATION_COPIES copies of the words, chosen by the workgroup: T S / 64 waves on one address would
  // queue behind each other for longer than the evaluation takes.  The host adds the copies' counts and takes the largest key: any order
  // gives the same.
  unsigned long long* const totals = D.totals + (size_t)(blockIdx.x % RM_DEVIATION_COPIES) * RM_DEVIATION_WORDS;
  mesh_measure_count(totals + RM_DEVIATION_SKIPPED, first && !live);
  mesh_measure_count(totals + RM_DEVIATION_UNEVALUATED, first && live && !evaluated);
  mesh_measure_count(totals + RM_DEVIATION_NONFINITE, live && !finite);
  mesh_measure_count(totals + RM_DEVIATION_OVER, over);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long other = __shfl_xor(key, m);
    if (other > key) key = other;
  }
  if ((threadIdx.x & 63u) == 0u && key != 0ull) atomicMax(totals + RM_DEVIATION_KEY, key);
}

// ---- refinement: the edge table, the marks and the children (include/hip_raymarch.h "refinement") ------------------------------------------------
// The scene is evaluated by rm_mesh_refine_eval_kernel between these launches (rm_mesh_host.inc rm_mesh_refine); these kernels are integer but
// for the mark's plain fp32.  The table is the measures': the same key, the same hash, linear probing bounded by the table's size; what it
// holds per edge is the lowest using slot 3 t + s, an atomicMin, so owner and numbering are the same on every run.  No thread waits for another.

// the table's slot of the undirected edge {a, b}: with `insert` the key is entered where it is missing; all-ones when the table has no room
// (insert) or not the key (lookup: only behind an insertion that failed)
template <bool INSERT>
__device__ inline unsigned long long mesh_refine_slot(const MeshRefine& R, unsigned int a, unsigned int b) {
  const unsigned long long key = a < b ? ((unsigned long long)a << 32 | b) : ((unsigned long long)b << 32 | a);
  unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  const unsigned long long mask = R.slots - 1ull;
  unsigned long long slot = h & mask;
  for (unsigned long long probe = 0; probe < R.slots; probe++, slot = (slot + 1ull) & mask) {
    unsigned long long held = INSERT ? __hip_atomic_load(R.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : R.keys[slot];
    if (INSERT && held == ~0ull) {
      held = atomicCAS(R.keys + slot, ~0ull, key);
      if (held == ~0ull) held = key;
    }
    if (held == key) return slot;
    if (!INSERT && held == ~0ull) break;
  }
  return ~0ull;
}

// the triangle's corners; whether it takes part: all three < V and pairwise different (rm_mesh_measure's rule)
__device__ inline bool mesh_refine_corners(const MeshRefine& R, long long t, unsigned int* c) {
  c[0] = R.corners[3 * t];
  c[1] = R.corners[3 * t + 1];
  c[2] = R.corners[3 * t + 2];
  return c[0] < R.vertices && c[1] < R.vertices && c[2] < R.vertices && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

__global__ __launch_bounds__(256) void rm_mesh_refine_edges_kernel(const MeshRefine R) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned int c[3];
  if (t >= R.triangles || !mesh_refine_corners(R, t, c)) return;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const unsigned long long slot = mesh_refine_slot<true>(R, c[s], c[(s + 1) % 3]);
    if (slot == ~0ull) R.totals[RM_REFINE_ERROR] = 1ull;  // (every writer writes the same)
    else atomicMin(R.owners + slot, (unsigned long long)(3 * t + s));
  }
}

// One thread per using slot u = 3 t + s.  NUMBER = false: words[u] = 1 iff u is its edge's owner.  NUMBER = true, behind the scan of the words:
// edge_of[u] = the edge's number, and the owner writes the edge's ends (lo, hi).
template <bool NUMBER>
__global__ __launch_bounds__(256) void rm_mesh_refine_slots_kernel(const MeshRefine R) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= 3 * R.triangles) return;
  const long long t = u / 3;
  const int s = (int)(u - 3 * t);
  unsigned int c[3];
  unsigned long long owner = ~0ull;
  if (mesh_refine_corners(R, t, c)) {
    const unsigned long long slot = mesh_refine_slot<false>(R, c[s], c[(s + 1) % 3]);
    if (slot != ~0ull) owner = R.owners[slot];
  }
  if (!NUMBER) {
    R.words[u] = owner == (unsigned long long)u ? 1ull : 0ull;
    return;
  }
  if (owner == ~0ull) {
    R.edge_of[u] = 0xFFFFFFFFu;
    return;
  }
  const unsigned int e = (unsigned int)R.words[owner];
  R.edge_of[u] = e;
  if (owner == (unsigned long long)u) {
    const unsigned int a = c[s], b = c[(s + 1) % 3];
    R.ends[2 * (size_t)e] = a < b ? a : b;
    R.ends[2 * (size_t)e + 1] = a < b ? b : a;
  }
}

// One thread per edge, and every thread of a wave stays to the end: the counts and the maximum read all of them.
__global__ __launch_bounds__(256) void rm_mesh_refine_mark_kernel(const MeshRefine R) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = e < R.edges;
  bool finite = false, marked = false;
  float err = 0.0f;
  if (valid) {
    const float* const a = R.positions + 3 * (size_t)R.ends[2 * e];
    const float* const b = R.positions + 3 * (size_t)R.ends[2 * e + 1];
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const float len2 = (dx * dx + dy * dy) + dz * dz;
    err = R.d[e] - R.iso;
    finite = isfinite(err);
    marked = finite && fabsf(err) > R.tolerance && len2 > R.min_edge2;
    R.marked[e] = marked ? 1u : 0u;
    R.marks[e] = marked ? 1ull : 0ull;
  }
  mesh_measure_count(R.totals + RM_REFINE_NONFINITE, valid && !finite);
  unsigned int most = valid && finite ? __float_as_uint(fabsf(err)) : 0u;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned int other = (unsigned int)__shfl_xor((int)most, m);
    if (other > most) most = other;
  }
  if ((threadIdx.x & 63u) == 0u && most != 0u) atomicMax(R.totals + RM_REFINE_MAX, (unsigned long long)most);
}

// the new vertex on edge e of a triangle that takes part: all-ones where the edge is not marked
__device__ inline unsigned int mesh_refine_midpoint(const MeshRefine& R, long long u) {
  const unsigned int e = R.edge_of[u];
  if (e == 0xFFFFFFFFu || R.marked[e] == 0u) return 0xFFFFFFFFu;  // (no number: only behind an insertion that failed)
  return (unsigned int)((unsigned long long)R.vertices + R.marks[e]);
}

__global__ __launch_bounds__(256) void rm_mesh_refine_count_kernel(const MeshRefine R) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= R.triangles) return;
  unsigned int c[3];
  unsigned long long children = 1ull;
  if (mesh_refine_corners(R, t, c))
    for (int s = 0; s < 3; s++)
      if (mesh_refine_midpoint(R, 3 * t + s) != 0xFFFFFFFFu) children++;  // (ahead of the scan of the marks: only whether there is one)
  R.words[t] = children;
}

__global__ __launch_bounds__(256) void rm_mesh_refine_vertices_kernel(const MeshRefine R) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= R.edges || R.marked[e] == 0u) return;
  const unsigned int lo = R.ends[2 * e], hi = R.ends[2 * e + 1];
  const size_t k = (size_t)R.vertices + (size_t)R.marks[e];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    R.out_positions[3 * k + c] = 0.5f * (R.positions[3 * (size_t)lo + c] + R.positions[3 * (size_t)hi + c]);
    if (R.out_colours) R.out_colours[3 * k + c] = 0.5f * (R.colours[3 * (size_t)lo + c] + R.colours[3 * (size_t)hi + c]);
  }
  if (R.out_cells) R.out_cells[k] = R.cells[lo];
}

__device__ inline void mesh_refine_child(unsigned int* out, unsigned int a, unsigned int b, unsigned int c) {
  out[0] = a;
  out[1] = b;
  out[2] = c;
}

// One thread per triangle: its children at its scanned offset, in the header's order, the parent's orientation kept.
__global__ __launch_bounds__(256) void rm_mesh_refine_emit_kernel(const MeshRefine R) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= R.triangles) return;
  unsigned int c[3], mid[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  unsigned int* out = R.out_corners + 3 * (size_t)R.words[t];
  int mask = 0;
  if (mesh_refine_corners(R, t, c))
    for (int s = 0; s < 3; s++) {
      mid[s] = mesh_refine_midpoint(R, 3 * t + s);
      if (mid[s] != 0xFFFFFFFFu) mask |= 1 << s;
    }
  // the rotation that brings the pattern to its form: the one marked edge to e0; two marked edges to e0 and e1
  const int r = mask == 2 || mask == 6 ? 1 : mask == 4 || mask == 5 ? 2 : 0;
  const unsigned int v0 = c[r], v1 = c[(r + 1) % 3], v2 = c[(r + 2) % 3];
  const unsigned int m0 = mid[r], m1 = mid[(r + 1) % 3], m2 = mid[(r + 2) % 3];
  switch (__popc((unsigned int)mask)) {
    case 0:
      mesh_refine_child(out, v0, v1, v2);
      break;
    case 1:
      mesh_refine_child(out, v0, m0, v2);
      mesh_refine_child(out + 3, m0, v1, v2);
      break;
    case 2:
      mesh_refine_child(out, m0, v1, m1);
      if (m0 < m1) {
        mesh_refine_child(out + 3, v0, m0, v2);
        mesh_refine_child(out + 6, m0, m1, v2);
      } else {
        mesh_refine_child(out + 3, v0, m0, m1);
        mesh_refine_child(out + 6, v0, m1, v2);
      }
      break;
    default:
      mesh_refine_child(out, v0, m0, m2);
      mesh_refine_child(out + 3, m0, v1, m1);
      mesh_refine_child(out + 6, m2, m1, v2);
      mesh_refine_child(out + 9, m0, m1, m2);
      break;
  }
}

#ifndef RM_ONLY_KERNELS
static inline long long mesh_cells(const GridDims& g) { return (long long)(g.nc[0] - 1) * (g.nc[1] - 1) * (g.nc[2] - 1); }

hipError_t launch_mesh_count(const MeshParams& P, hipStream_t stream) {
  const long long cells = mesh_cells(P.grid);
  hipLaunchKernelGGL(rm_mesh_count_kernel, dim3((unsigned int)((cells + 255) / 256)), dim3(256), 0, stream, P, (int)cells);
  return hipGetLastError();
}

// the workgroup totals of every level but the last, one level behind the other
size_t rm_mesh_scan_scratch_elems(long long cells) {
  size_t elems = 0;
  for (long long n = (cells + 255) / 256; n > 1; n = (n + 255) / 256) elems += (size_t)n;
  return elems;
}

// counts[0 .. cells) -> the exclusive scan, in place; *total (device) = the sum of all of them
hipError_t launch_mesh_scan(unsigned long long* counts, long long cells, unsigned long long* scratch, unsigned long long* total, hipStream_t stream) {
  unsigned long long* data[8];
  long long n[8];
  int levels = 0;
  data[0] = counts;
  n[0] = cells;
  for (;;) {  // down: 2^28 cells make four levels
    const long long groups = (n[levels] + 255) / 256;
    unsigned long long* sums = groups == 1 ? total : scratch;
    hipLaunchKernelGGL(rm_mesh_scan_kernel, dim3((unsigned int)groups), dim3(256), 0, stream, data[levels], n[levels], sums);
    if (groups == 1) break;
    scratch += groups;
    levels++;
    data[levels] = sums;
    n[levels] = groups;
  }
  for (int l = levels - 1; l >= 0; l--)  // and up
    hipLaunchKernelGGL(rm_mesh_scan_add_kernel, dim3((unsigned int)((n[l] + 255) / 256)), dim3(256), 0, stream, data[l], n[l], data[l + 1]);
  return hipGetLastError();
}

hipError_t launch_mesh_colours(const float* material, float* colours, long long vertices, hipStream_t stream) {
  hipLaunchKernelGGL(rm_mesh_take3_kernel, dim3((unsigned int)((3 * vertices + 255) / 256)), dim3(256), 0, stream, material, colours, 3 * vertices);
  return hipGetLastError();
}

hipError_t launch_mesh_cross(const MeshSharpParams& P, int init, int consume, int last, hipStream_t stream) {
  hipLaunchKernelGGL(rm_mesh_cross_kernel, dim3((unsigned int)((P.vertices + 255) / 256)), dim3(256), 0, stream, P, init, consume, last);
  return hipGetLastError();
}

hipError_t launch_mesh_qef(const MeshSharpParams& P, hipStream_t stream) {
  hipLaunchKernelGGL(rm_mesh_qef_kernel, dim3((unsigned int)((P.vertices + 255) / 256)), dim3(256), 0, stream, P);
  return hipGetLastError();
}

// components and islands: n < 2^32 elements, one thread each, workgroups of 256; nothing is launched for n == 0
#define RM_MESH_PARTS_LAUNCH(kernel, n, ...)                                                                            \
  do {                                                                                                                  \
    if ((n) > 0) hipLaunchKernelGGL(kernel, dim3((unsigned int)(((n) + 255) / 256)), dim3(256), 0, stream, __VA_ARGS__); \
    return hipGetLastError();                                                                                           \
  } while (0)

hipError_t launch_mesh_link_init(unsigned int* parent, long long vertices, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_link_init_kernel, vertices, parent, vertices);
}
hipError_t launch_mesh_link_hook(unsigned int* parent, const unsigned int* triangles, long long vertices, long long n, unsigned int* changed, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_link_hook_kernel, n, parent, triangles, vertices, n, changed);
}
hipError_t launch_mesh_link_flatten(unsigned int* parent, long long vertices, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_link_flatten_kernel, vertices, parent, vertices);
}
hipError_t launch_mesh_roots(const unsigned int* parent, unsigned long long* words, long long vertices, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_roots_kernel, vertices, parent, words, vertices);
}
hipError_t launch_mesh_labels(const unsigned int* parent, const unsigned long long* scanned, unsigned int* labels, long long vertices, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_labels_kernel, vertices, parent, scanned, labels, vertices);
}
hipError_t launch_mesh_part_sizes(const unsigned int* labels, const unsigned int* triangles, long long n, unsigned int* sizes, int slot, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_part_sizes_kernel, n, labels, triangles, n, sizes, slot);
}
hipError_t launch_mesh_keep_flags(const unsigned int* labels, const unsigned int* triangles, const unsigned int* keep, long long n, unsigned long long* words,
                                  hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_keep_flags_kernel, n, labels, triangles, keep, n, words);
}
hipError_t launch_mesh_gather_vertices(const MeshGather& G, long long vertices, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_gather_vertices_kernel, vertices, G, vertices);
}
hipError_t launch_mesh_gather_triangles(const MeshGather& G, const unsigned int* triangles, const unsigned long long* triangle_at, long long n,
                                        unsigned int* out, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_gather_triangles_kernel, n, G, triangles, triangle_at, n, out);
}

// simplification: one thread per source vertex, output vertex or source triangle (map: and one more)
hipError_t launch_mesh_simplify_mark(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_mark_kernel, S.vertices, S); }
hipError_t launch_mesh_simplify_sums(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_sums_kernel, S.vertices, S); }
hipError_t launch_mesh_simplify_place(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_place_kernel, S.out_vertices, S); }
hipError_t launch_mesh_simplify_map(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_map_kernel, S.triangles + 1, S); }
hipError_t launch_mesh_simplify_insert(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_insert_kernel, S.triangles, S); }
hipError_t launch_mesh_simplify_keep(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_keep_kernel, S.triangles, S); }
hipError_t launch_mesh_simplify_gather(const MeshSimplify& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_simplify_take_kernel, S.triangles, S); }
hipError_t launch_mesh_quadric_sums(const MeshQuadric& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_quadric_sums_kernel, S.triangles, S); }
hipError_t launch_mesh_quadric_place(const MeshQuadric& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_quadric_place_kernel, S.out_vertices, S); }
// measures: one thread per triangle, slot or vertex; the sums one workgroup per 256 values
hipError_t launch_mesh_measure_edges(const MeshMeasure& M, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_measure_edges_kernel, M.triangles, M); }
hipError_t launch_mesh_measure_classes(const MeshMeasure& M, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_measure_classes_kernel, (long long)M.slots, M); }
hipError_t launch_mesh_measure_used(const MeshMeasure& M, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_measure_used_kernel, M.vertices, M); }
hipError_t launch_mesh_measure_extent(const MeshMeasure& M, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_measure_extent_kernel, M.vertices, M); }
hipError_t launch_mesh_measure_terms(const MeshMeasure& M, double* area, double* volume, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_measure_terms_kernel, M.triangles, M, area, volume);
}
hipError_t launch_mesh_measure_sum(const double* area, const double* volume, long long n, double* out_area, double* out_volume, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_measure_sum_kernel, n, area, volume, n, out_area, out_volume);
}
// projection: one thread per vertex or triangle
hipError_t launch_mesh_project_step(const MeshProject& S, int round, double* sum, double* sum2, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_project_step_kernel, S.vertices, S, round, sum, sum2);
}
hipError_t launch_mesh_project_flips(const MeshProject& S, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_project_flips_kernel, S.triangles, S); }
// deviation: one thread per (triangle, sample)
hipError_t launch_mesh_deviation_reduce(const MeshDeviation& D, hipStream_t stream) {
  RM_MESH_PARTS_LAUNCH(rm_mesh_deviation_reduce_kernel, (long long)D.triangles << D.log2_samples, D);
}
// refinement: one thread per triangle, using slot or edge
hipError_t launch_mesh_refine_edges(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_edges_kernel, R.triangles, R); }
hipError_t launch_mesh_refine_flags(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_slots_kernel<false>, 3 * R.triangles, R); }
hipError_t launch_mesh_refine_number(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_slots_kernel<true>, 3 * R.triangles, R); }
hipError_t launch_mesh_refine_mark(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_mark_kernel, R.edges, R); }
hipError_t launch_mesh_refine_count(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_count_kernel, R.triangles, R); }
hipError_t launch_mesh_refine_vertices(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_vertices_kernel, R.edges, R); }
hipError_t launch_mesh_refine_emit(const MeshRefine& R, hipStream_t stream) { RM_MESH_PARTS_LAUNCH(rm_mesh_refine_emit_kernel, R.triangles, R); }
#undef RM_MESH_PARTS_LAUNCH

hipError_t launch_mesh_emit(const MeshParams& P, hipStream_t stream) {
  const long long cells = mesh_cells(P.grid);
  hipLaunchKernelGGL(rm_mesh_emit_kernel, dim3((unsigned int)((cells + 255) / 256)), dim3(256), 0, stream, P, (int)cells);
  return hipGetLastError();
}

// slabbed extraction: a layer has at most 2^20 cells and a window at most 2^28 corners, so every count here is an int
static inline int mesh_layer_cells(const GridDims& g) { return (g.nc[0] - 1) * (g.nc[1] - 1); }

hipError_t launch_mesh_slab_tally(const MeshSlab& S, hipStream_t stream) {
  const int layer = mesh_layer_cells(S.mesh.grid), cells = S.layers * layer;
  hipLaunchKernelGGL(rm_mesh_slab_tally_kernel, dim3((unsigned int)((cells + 255) / 256)), dim3(256), 0, stream, S, S.own0 * layer, cells);
  return hipGetLastError();
}
hipError_t launch_mesh_slab_count(const MeshSlab& S, hipStream_t stream) {
  const int layer = mesh_layer_cells(S.mesh.grid), cells = (S.own0 - S.mesh.plane0 + S.layers) * layer;
  hipLaunchKernelGGL(rm_mesh_slab_count_kernel, dim3((unsigned int)((cells + 255) / 256)), dim3(256), 0, stream, S, S.mesh.plane0 * layer, cells);
  return hipGetLastError();
}
hipError_t launch_mesh_slab_emit(const MeshSlab& S, hipStream_t stream) {
  const int layer = mesh_layer_cells(S.mesh.grid), halo = (S.own0 - S.mesh.plane0) * layer, cells = halo + S.layers * layer;
  hipLaunchKernelGGL(rm_mesh_slab_emit_kernel, dim3((unsigned int)((cells - halo + 255) / 256)), dim3(256), 0, stream, S, S.mesh.plane0 * layer, halo, cells);
  return hipGetLastError();
}
#endif
#endif  // !RM_BUILD_FAST && !RM_GL_STACK

}  // namespace rm
