// rm_params.hpp -- kernel argument blocks shared by the API and both kernel builds.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/hip_raymarch.h"

// table_flags of DevScene (set by rm_scene_create)
#define RM_TABLE_SPHERES_SMOOTH 1  /* every row is a sphere and every fold after the first a smooth union */
#define RM_TABLE_HAS_DOMAIN 2      /* the table has domain rows (RM_PRIM_REPEAT / RM_PRIM_FOLD) */
#define RM_TABLE_NO_BOXES 8         /* no RM_PRIM_BOX row: the sdf of a point with a non-finite coordinate is itself non-finite */
#define RM_TABLE_UNIFORM_K 4       /* RM_TABLE_SPHERES_SMOOTH with one k for every fold: k in p[0], 0.5 / k in p[1] */
#define RM_TABLE_HAS_KIND 32      /* some shape row evaluates a scene kind's estimator (RM_PRIM_KIND): its own pixel kernel, no far-field exits, no row culling */
#define RM_TABLE_MORE 64          /* some row uses ABI 8's vocabulary (torus / cylinder / plane, smooth subtraction / intersection): the second copy of the general fold */
#define RM_TABLE_HAS_SURFACES 16   /* some shape row names a surface (RmPrim.type bits 16..23): the material functions depend on the position */

#define RM_BATCH_MAX 8  /* samples one pixel-kernel launch can render (KParams::batch) */

// Row culling for primitive tables without domain rows (round 3; both builds since round 4; rm_kernels.inc rm_cull_build_kernel fills
// it before the first launch that can use it, rm_device.hpp Sdf<RM_SCENE_TABLE>::culled_rows reads it).  Nested uniform grids about
// the shapes' bounding box: level l is a cube with half-width half0 * 2^l about `centre`, of n^3 cells for level 0 and n_outer^3 for
// the levels around it (round 5: a ray spends its steps near the shapes, where the cells have to be small; the levels it merely
// crosses on its way in take cells twice as wide -- 31.5 MB instead of 134 for CSG-64), and a point belongs to
// the lowest level that holds it.  Per cell one bit per row -- clear = the row's operator cannot change the running value of the fold
// anywhere in the cell (an exact no-op there), so an evaluation may skip it.  cells = [level 0: n^3][levels 1 ..: n_outer^3 each][words]
// 64-bit words, then one cell that lists every row (points beyond the last level, non-finite points).
struct CullGrid {
  const unsigned long long* cells;  // device pointer; nullptr = no culling
  float centre[3];
  float inv_half0;  // 1 / half0
  float scale0;     // cells per unit length at level 0: n / (2 half0)
  int n, n_outer, levels, words;  // n_outer is n or n / 2
};
struct CullBuild {  // argument block of rm_cull_build_kernel
  const RmPrim* prims;
  unsigned long long* cells;
  int nprims, n, n_outer, levels, words;
  double centre[3], half0;
  double reach;  // the largest |coordinate| of a shape: scale of the fp32 error allowance
};
__host__ __device__ inline long long rm_cull_cells(int n, int n_outer, int levels) {  // without the cell that lists every row
  return (long long)n * n * n + (long long)(levels - 1) * n_outer * n_outer * n_outer;
}

// the fp32 allowance of the culling tests: n + 8 roundings at the magnitude of the coordinates involved
__host__ __device__ inline double rm_cull_margin(int nprims, double magnitude) { return 1e-4 + 1.2e-7 * (nprims + 8) * magnitude; }
// a shape row as the rule reads it: the table's floats widened once, and what the rule derives from them per row and not per cell
// (round 5: the build kernel stages these in LDS once per workgroup; rounds 3-4 read the 32-byte RmPrim from memory and divided
// by k twice, per row AND cell)
struct CullRow {
  double c[3], size[3], k, half_inv_k;
  double reach;  // a box's half-diagonal (0 for a sphere): how far its nearest point can be from its centre
  int shape, op;
};
__host__ __device__ inline CullRow rm_cull_row(const RmPrim& p) {
  CullRow r;
  for (int a = 0; a < 3; a++) { r.c[a] = p.center[a]; r.size[a] = p.size[a]; }
  r.k = (double)p.k;
  r.half_inv_k = 0.5 / r.k;  // (Inf for k = 0: only read for smooth unions, whose k > 0)
  r.shape = p.type & 0xff;
  r.op = (p.type >> 8) & 0xff;
  r.reach = r.shape == RM_PRIM_SPHERE ? 0.0 : sqrt(r.size[0] * r.size[0] + r.size[1] * r.size[1] + r.size[2] * r.size[2]);
  return r;
}
__host__ __device__ inline double rm_cull_shape_distance(const CullRow& p, const double* c) {
  const double x = c[0] - p.c[0], y = c[1] - p.c[1], z = c[2] - p.c[2];
  if (p.shape == RM_PRIM_SPHERE) return sqrt(x * x + y * y + z * z) - p.size[0];
  const double qx = fabs(x) - p.size[0], qy = fabs(y) - p.size[1], qz = fabs(z) - p.size[2];  // sdBox, raymarcher.frag:108-112
  const double ox = fmax(qx, 0.0), oy = fmax(qy, 0.0), oz = fmax(qz, 0.0);
  return sqrt(ox * ox + oy * oy + oz * oz) + fmin(fmax(qx, fmax(qy, qz)), 0.0);
}
// The rows of a table (no domain rows) that an evaluation anywhere in the ball (c, rad) has to fold: bit i of out[] set = row i
// stays.  The argument is with rm_cull_build_kernel (rm_kernels.inc), which calls this once per cell; host-callable so that the
// CPU tests can check it against the fold itself (rm_debug_cull_cell).
//
// Hard operators: min(d, di) with the shape further away than the running value can be anywhere in the cell, max(d, +-di) with
// the term below it -- exact no-ops whatever the arithmetic.
//
// Smooth unions (round 4).  Round 3 built row culling for them, measured it (C4 14.2 -> 7.0 ms) and took it out: a row further than k
// from the running value does not leave it alone -- mix(di, d, 1), in both builds' arithmetic, is  d' = fl(di - fl(di - d)): it ROUNDS
// d to the grid of (di - d), and that noise is what the creeping shadow rays of a smooth-union scene live on (14 % fewer lit pixels
// without it).  The rounding itself can be reasoned about exactly.  Write e(x) = floor(log2 |x|); a float x is a multiple of
// 2^(e(x) - 23) (the argument is the same in any binary precision).
//  * EXECUTING a far row m (t = fl(dm - d), d' = fl(dm - t)): dm and t are multiples of 2^(g - 23), g = min(e(dm), e(t)), so is their
//    difference, and it is representable when |d'| < 2^(g + 1): then d' = dm - t exactly and d' lies ON THE GRID 2^(g - 23).
//  * a later far row i finds d on a grid 2^(B - 23) with B >= e(di - d) and e(di - d) <= e(di): then di and d are both multiples of
//    the unit of t = di - d, t is exact, and d'' = di - t = d: the row is an EXACT NO-OP and may be skipped.
//  * any row that is executed and is not certainly far -- a near smooth union, a hard operator that may take the other value --
//    moves d off every grid: the chain starts again after it; a far row that is executed without meeting the no-op conditions
//    leaves d on ITS grid, which may be finer than the one before; a row that is skipped leaves d, and the grid it is on, alone.
// Per cell the rule runs this bookkeeping on INTERVALS: the running value in [L, U] (the smooth minimum is monotone in both
// arguments, so its interval is the smooth minimum of the ends), row i's distance in [lo_i, hi_i], binades taken where the whole
// interval lies in one; a distance that is negative or changes sign in the cell claims nothing.  What the rule cannot decide it
// keeps: a kept row is the reference's own arithmetic, and any superset of a point's list gives the same bits (the extra rows are
// identities there) -- which is what lets a wave fold the union of its lanes' lists.  About half of CSG-64's 64 rows stay per cell.
// tests/test_cull_rule_cpu.py checks the rule against fp32 restatements of both builds' folds; the GPU suite holds the culled fold
// to RM_RENDER_NO_CULL bit for bit.
// the exponent of a positive, finite, normal double, read off its exponent field (round 5; rounds 3-4 called the library's
// logarithm -- three times per row and cell, most of the build kernel's 8.9 ms on CSG-64's grid)
__host__ __device__ inline int rm_exponent(double v) { return ilogb(v); }
__host__ __device__ inline double rm_smooth_min(double a, double b, double k, double half_inv_k) {  // examples/smooth-tree.glsl:20-22, in double (0.5 / k given)
  double h = 0.5 + (b - a) * half_inv_k;
  h = h < 0.0 ? 0.0 : (h > 1.0 ? 1.0 : h);
  return b + h * (a - b) - k * h * (1.0 - h);
}
// tables whose rows are mostly smooth unions get the finer grid: the binade tests want small cells (rm_api.hip table_cull_params)
__host__ __device__ inline bool rm_cull_mostly_smooth(const RmPrim* prims, int nprims) {
  int smooth = 0;
  for (int i = 1; i < nprims; i++) smooth += ((prims[i].type >> 8) & 0xff) == RM_OP_SMOOTH_UNION;
  return 2 * smooth > nprims;
}

__host__ __device__ inline void rm_cull_cell_rows(const CullRow* prims, int nprims, int words, const double* c, double rad, double margin, unsigned long long* out) {
  const int NONE = -100000;
  for (int w = 0; w < words; w++) out[w] = 0ull;
  const double d0 = rm_cull_shape_distance(prims[0], c);
  double L = d0 - rad, U = d0 + rad;
  int best = 0;  // the nearest earlier row at c that bounds the running value from above (-1: none)
  double best_d = d0;
  int B = NONE;  // the running value is certainly a multiple of 2^(B - 23)
  out[0] |= 1ull;
  for (int i = 1; i < nprims; i++) {
    const CullRow& p = prims[i];
    const int op = p.op;
    const double di = rm_cull_shape_distance(p, c), lo_i = di - rad, hi_i = di + rad;
    bool keep;
    if (op == RM_OP_SMOOTH_UNION) {
      const double k = p.k;  // > 0 (rm_scene_create)
      keep = true;
      if (!(lo_i - U >= 1.002 * k + 2.0 * margin)) {
        B = NONE;  // possibly near: whatever grid d was on, it leaves it
      } else {
        const double emin = lo_i - U - 2.0 * margin, emax = hi_i - L + 2.0 * margin;  // t = di - d over the cell, both > 0
        const int bmin = rm_exponent(emin * (1.0 - 1e-5)), bmax = rm_exponent(emax * (1.0 + 1e-5));
        // the lowest binade of |di| over the cell; a far row's distance may be negative (the running value is then further inside
        // still) or change sign in the cell: then |di| has no lowest binade and nothing is claimed
        const double lo_m = lo_i - margin, hi_m = hi_i + margin;
        const int bdi = lo_m > 0.0 ? rm_exponent(lo_m * (1.0 - 1e-5)) : (hi_m < 0.0 ? rm_exponent(-hi_m * (1.0 - 1e-5)) : NONE);
        if (B != NONE && B >= bmax && bmax <= bdi) {
          keep = false;  // an exact no-op everywhere in the cell
        } else {
          const int g = bmin < bdi ? bmin : bdi;
          const double big = (fabs(L) > fabs(U) ? fabs(L) : fabs(U)) + margin;
          B = g != NONE && big * (1.0 + 1e-5) < ldexp(1.0, g + 1) ? g : NONE;  // the grid this row leaves d on, when d' = dm - t is exact
        }
      }
      const double u_smooth = rm_smooth_min(U, hi_i, k, p.half_inv_k) + margin;
      U = fmin(fmin(U, hi_i), u_smooth);
      L = rm_smooth_min(L, lo_i, k, p.half_inv_k) - margin;  // (at most k / 4 below the minimum)
      if (best < 0 || di < best_d) { best = i; best_d = di; }
    } else if (op == RM_OP_UNION) {
      const double k = 0.0;
      keep = !(lo_i >= U + margin);
      if (keep && best >= 0) {
        const CullRow& q = prims[best];
        const double sx = p.c[0] - q.c[0], sy = p.c[1] - q.c[1], sz = p.c[2] - q.c[2];
        // the point the gradient of a shape's distance points away from: a sphere's centre; the nearest point of a box (within its
        // half-diagonal of the centre, at the distance itself -- which has to be positive over the ball)
        const bool ps = p.shape == RM_PRIM_SPHERE, qs = q.shape == RM_PRIM_SPHERE;
        const double pe = p.reach, qe = q.reach;
        const double s = sqrt(sx * sx + sy * sy + sz * sz) + pe + qe;
        const double a = (ps ? di + p.size[0] : di) - rad, b = (qs ? best_d + q.size[0] : best_d) - rad;
        if (a > 0.0 && b > 0.0) {
          const double lip = fmin(2.0, s / sqrt(a * b));
          keep = !(di - best_d - rad * lip >= k + margin);
        }
      }
      U = fmin(U, hi_i);
      L = fmin(L, lo_i);
      if (best < 0 || di < best_d) { best = i; best_d = di; }
      if (keep) B = NONE;  // min(d, di) may hand on di
    } else if (op == RM_OP_SUBTRACT) {
      keep = !(-lo_i <= L - margin);
      U = fmax(U, -lo_i);
      L = fmax(L, -hi_i);
      if (keep) best = -1, B = NONE;  // the value may now exceed every earlier term
    } else {
      keep = !(hi_i <= L - margin);
      U = fmax(U, hi_i);
      L = fmax(L, lo_i);
      if (keep) best = -1, B = NONE;  // max(d, di) where di may win: no earlier term bounds the value from above any more
    }
    if (keep) out[i >> 6] |= 1ull << (i & 63);
  }
}

// ... from the table's own rows (the host's rm_debug_cull_cell; at most RM_MAX_PRIMS of them)
__host__ __device__ inline void rm_cull_cell(const RmPrim* prims, int nprims, int words, const double* c, double rad, double margin, unsigned long long* out) {
  CullRow rows[RM_MAX_PRIMS];
  for (int i = 0; i < nprims; i++) rows[i] = rm_cull_row(prims[i]);
  rm_cull_cell_rows(rows, nprims, words, c, rad, margin, out);
}

struct DevScene {
  int kind;
  int nprims;
  int table_flags;
  int reserved;
  const RmPrim* prims;  // device pointer (RM_SCENE_TABLE)
  float p[16];
  RmMaterial mat;
  const RmSurface* surfaces;  // device pointer: nsurfaces + 1 entries, [0] = the values of `mat` (RM_TABLE_HAS_SURFACES)
  int nsurfaces;
  // The far field of a primitive table without domain rows (rm_device.hpp Sdf<RM_SCENE_TABLE>::far_jump; set by rm_scene_create):
  // far_end = 0: no jump; 1: an escaping ray ends at +-Inf by the sign of its direction components; 2: at (NaN, NaN, NaN).
  // far_r2 = (2 R' + 1)^2 with R' = the radius of a sphere about the origin that holds every shape, plus 1.01 x the largest smooth-union radius k (a chain of
  // smooth unions stays within k of the minimum): rm_api.hip table_far_field; far_escape's Rp is R' + 1/2.
  int far_end;
  float far_r2;
  // a ray that passes every shape of a table at a distance (rm_device.hpp Sdf<RM_SCENE_TABLE>::clear_miss): the clearance beyond a
  // shape's bounding sphere is clear_k (the largest smooth-union radius) + the step b0 the march is then sure of, which the steps it
  // has left decide: b0 = 2.05 clear_rho / (left - 84), clear_rho = the radius of a sphere about the origin that holds every
  // shape's sphere with 15 % to spare.  clear_rho = 0: no such test
  float clear_k;
  float clear_rho;
  CullGrid cull;
};

// ---- the half-precision G-buffer (RM_GBUFFER_F16: LoadRenderJobContext.tsx:81-119 allocates normal + DoF radius and albedo + depth
// as RGBA16F) ---------------------------------------------------------------------------------------------------------------------------
// A pixel of such a plane is 4 x IEEE binary16, 8 bytes, RGBA.  An accumulation reads the stored value widened to fp32 (exact), adds
// the sample's contribution in fp32 as the fp32 planes do, and stores the sum rounded to binary16 to nearest even (overflow to +-inf,
// subnormals kept): what raymarcher.frag:347-351 does with an RGBA16F attachment.  Every kernel that touches a half plane goes
// through these two helpers.  (_Float16)(float) is round-to-nearest-even; on gfx950 it lowers to v_cvt_pk_f16_f32 / v_cvt_f16_f32,
// which round by the MODE register (RNE) -- never v_cvt_pkrtz_f16_f32, which truncates.  The kernels keep hipcc's default
// float_denorm_mode_16_64 = 3: flushing f16 subnormals would change small normal components.
typedef _Float16 rm_half4 __attribute__((ext_vector_type(4)));  // 8 bytes, 8-byte aligned: one dwordx2 load / store
static_assert(sizeof(rm_half4) == 8, "rm_half4 is 8 bytes");

__device__ inline float4 rm_widen(const rm_half4 h) { return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w); }
__device__ inline rm_half4 rm_narrow(const float4 v) {
  rm_half4 h;
  h.x = (_Float16)v.x; h.y = (_Float16)v.y; h.z = (_Float16)v.z; h.w = (_Float16)v.w;
  return h;
}

struct KParams {
  RmUniforms u;
  DevScene scene;
  float4* color;
  float4* normal_dof;    // nullptr = colour only
  float4* albedo_depth;
  int W, H;            // full image (textureSize(previousColor), raymarcher.frag:183)
  int row_begin;       // contiguous window: first image row held by the planes
  int stripe_rows, parts, part;  // striped window (stripe_rows > 0): rows r with (r / stripe_rows) % parts == part
  int tx, ty, tw, th;  // tile clipped to the window; ty/th count LOCAL rows (rows of the planes)
  float retire_eps;    // 0 = exact (fixed-point) retire only
  // Staged output (full mode, samples in flight): the pixel kernel does not touch the planes; it leaves what
  // the sample adds -- (light * exposure, -), (normal, dofRadius), (albedo, depth) -- in stage[0..2][pixel] and
  // rm_combine_kernel applies the blend afterwards, in sample order.  nullptr = blend in the kernel.
  float4* stage;
  long long stage_stride;  // elements between the three staged planes
  // Sample batch (rm_render_samples, staged output only): ONE launch renders `batch` consecutive samples of the job --
  // workgroup b renders tile b / batch for sample b % batch, with randNoise batch_noise[sample] instead of u.randNoise
  // and its output staged at stage + sample * 3 * stage_stride -- so that a small window (one GPU's share of a frame)
  // still gives the chip a full frame's worth of workgroups.  0 or 1 = one sample.
  int batch;
  int tile_wide;  // set by the launcher: 0 = the kind's own tile; n > 0 = 8-wave workgroups with 2^(n-1) waves across (3: 32 x 16 pixels instead of 16 x 32; rm_kernels.inc BlockShape)
  float batch_noise[RM_BATCH_MAX][2];
  // Cost-ordered dispatch (pixel kernel): workgroup b of the launch renders tile block_order[b], and every workgroup
  // leaves its duration in block_cost[tile] for the next sample's order (rm_order_kernel).  nullptr = in launch order.
  const unsigned int* block_order;
  unsigned int* block_cost;
  int no_far_jump;  // RM_RENDER_NO_FAR_JUMP: march escaping rays step by step (a measurement / test switch, same bits)
  int gbuffer_half;  // RM_GBUFFER_F16: normal_dof / albedo_depth point at rm_half4 planes -- read by rm_combine_kernel; a launch of
                     // the pixel kernel that would blend into them itself is never made (rm_api.hip launch: always staged)
  float2* moments;   // RM_FB_MOMENTS: (sum l, sum l^2) per pixel, written by rm_combine_kernel only (like the half planes: a launch
                     // that writes the G-buffer into a framebuffer with moments is always staged); nullptr = none
};

// a table long enough for the compacting pixel kernel (rm_device.hpp RM_KIND_TABLE_BIG); launcher and grid computation agree through this
#define RM_TABLE_BIG_ROWS 16
__host__ __device__ inline bool rm_table_big(const KParams& P) {
  return P.scene.kind == RM_SCENE_TABLE && P.scene.nprims >= RM_TABLE_BIG_ROWS && P.u.renderMode == 0 && !(P.scene.table_flags & RM_TABLE_HAS_KIND);
}

// image row of a local (plane) row
__host__ __device__ inline int rm_global_row(const KParams& P, int local) {
  if (P.stripe_rows <= 0) return P.row_begin + local;
  return ((local / P.stripe_rows) * P.parts + P.part) * P.stripe_rows + local % P.stripe_rows;
}

struct ProbeParams {
  DevScene scene;
  const float* in;
  float* out;
  int n;
  int what;
  float param;
  float retire_eps;
  int no_far_jump;
};
// (the probe follows RM_RENDER_NO_CULL through scene.cull.cells, which rm_probe clears)

// A grid of corners as the mesh kernels take it (rm_mesh_kernels.inc; RmGrid checked, h divided once on the host): corner i of axis a
// lies at lo[a] + (float)i * h[a], each operation rounded on its own; nc = corners per axis (cells + 1), x fastest in memory.
struct GridDims {
  float lo[3], h[3];
  int nc[3];
  int corners;  // nc[0] * nc[1] * nc[2] <= 2^28
};
__host__ __device__ inline float rm_grid_coord(const GridDims& g, int axis, int i) {
#pragma clang fp contract(off)  // (the host unit is not built contract-off)
  const float step = (float)i * g.h[axis];
  return g.lo[axis] + step;
}
// rm_sdf_grid: Sdf<KIND>::eval at every corner, with the probe's scene block
struct SdfGridParams {
  DevScene scene;
  GridDims grid;
  float* out;
  int plane0;  // a window of z planes (slabbed extraction): grid.nc[2] and grid.corners are the window's, out[0] is corner (0, 0, plane0); 0 = the whole grid
};
// rm_mesh_occlusion: one lane per (vertex, direction), Sdf<KIND>::eval at its taps, with the probe's scene block.  normals and d0 are
// the probes' outputs at the positions (RM_PROBE_NORMAL, RM_PROBE_SDF); directions is the host's table (rm_mesh_occlusion_directions).
struct MeshOcclusionPass {
  DevScene scene;
  const float* positions;    // V x 3
  const float* normals;      // V x 3
  const float* d0;           // V
  const float4* directions;  // K x (x, y, z, 1 / z)
  float* out;                // V
  int vertices;              // V << log2_directions < 2^31
  int log2_directions;       // K = 1 << log2_directions <= 64
  int taps;                  // J in 1..8
  float radius, inv_radius;  // inv_radius = 1.0f / radius, divided once on the host
  float strength;
  float scale;               // 2^-(16 + log2 K + log2 J)
};
// rm_mesh_project's evaluating launch: one lane per vertex, Sdf<KIND>::eval at its position with the probe's scene block, and scene_normal
// there in the waves that have a lane with a finite d - iso above the tolerance (the other waves leave their normals as they are).
struct MeshProjectEval {
  DevScene scene;
  const float* positions;  // V x 3: the round's p
  float* d;                // V
  float* normals;          // V x 3
  int vertices;
  float iso, tolerance, normal_delta;
};
// rm_mesh_deviation's evaluating launch: one lane per (triangle, sample), Sdf<KIND>::eval at the sample's point with the probe's scene block.
// weights is the host's table (rm_mesh_deviation_weights).
struct MeshDeviationSdf {
  DevScene scene;
  const float* positions;       // V x 3
  const unsigned int* corners;  // T x 3
  const float4* weights;        // S x (w0, w1, w2, 0)
  float* d;                     // T x S
  long long vertices;           // V >= 1
  int triangles;                // T >= 1, T << log2_samples < 2^31
  int log2_samples;             // S = 1 << log2_samples <= 64
};
// rm_mesh_refine's evaluating launch: one lane per unique edge, Sdf<KIND>::eval at the edge's midpoint with the probe's scene block.
struct MeshRefineMidpoints {
  DevScene scene;
  const float* positions;     // V x 3
  const unsigned int* ends;   // E x (lo, hi)
  float* d;                   // E
  int edges;                  // E >= 1
};
// The surface-nets mesher over a grid of values.  counts: per cell (vertex flag) | (quads << 32), scanned in place into the cell's
// first vertex | first quad; the emit pass reads a neighbour's vertex index from there (every cell round a crossing edge is active).
struct MeshParams {
  GridDims grid;
  const float* values;
  float iso;
  unsigned long long* counts;  // cells entries
  float* positions;            // emit: V x 3
  unsigned int* cells;         // emit: V
  unsigned int* triangles;     // emit: T x 3
  int plane0;                  // values[0] is corner (0, 0, plane0) of the grid: a window of z planes (slabbed extraction); 0 = the whole grid
};
// One slab of rm_mesh_extract_slabs (the header's "slabbed extraction").  mesh.grid is the WHOLE grid and cell indices are global; mesh.values
// holds the window's planes from mesh.plane0 on, mesh.counts the window's cells: those of layer mesh.plane0 first, which is the halo layer
// when own0 > plane0.  The slab's own cells are layers own0 .. own0 + layers - 1.
struct MeshSlab {
  MeshParams mesh;
  int own0, layers;
  unsigned long long vertex_base, quad_base;  // emit: the vertices and quads of the slabs before this one
  unsigned long long* total;                  // tally: this slab's (vertices) | (quads << 32), summed by atomics
};
// The sharp vertices of rm_mesh_extract_sharp over an emitted mesh: 12 slots per vertex, the cell's edges in the mesher's order.  Slot s of
// vertex v lies at s * vertices + v in every slot array, so a wave's accesses to one slot are one run.  mesh.positions holds the surface-nets
// vertices on the way in (the point of a dead slot) and the QEF's on the way out; mesh.counts and mesh.triangles are not used.
struct MeshSharpParams {
  MeshParams mesh;
  int vertices;
  float4* state;        // 12 V: (x0, e0, x1, e1) of a live slot's bracket
  float* points;        // 12 V x 3: what the probes evaluate -- a round's midpoints, at the end the crossings
  const float* probed;  // 12 V x 3 floats of room: a round's RM_PROBE_SDF output (12 V floats), then the RM_PROBE_NORMAL output
  unsigned int* live;   // V: bit s = slot s is live
  float threshold;
};

// One pass of the denoiser (rm_frame_kernels.inc "denoise").  Pass 0 reads color / normal_dof / albedo_depth and writes
// guide; later passes read x_in and guide; the last pass reads color (.w) and albedo_depth (the modulation) again.
struct DenoisePass {
  const float4* color;
  const void* normal_dof;    // float4 or rm_half4 planes
  const void* albedo_depth;
  const float4* x_in;        // the previous pass's demodulated colour (.w unused)
  float4* guide;             // (n.xyz, z) per pixel
  float4* out;               // demodulated colour, or on the last pass the result in colour-plane units
  int W, H, step;            // step h = 2^pass
  float s, k;                // 1 / samples, samples
  float inv_color, inv_normal, sigma_z_h;  // 1 / (sigma_c^2 4^-pass), 1 / sigma_n^2, sigma_z h
  // the variance-guided mode only (rm_denoise_variance): x.w carries the variance v of the demodulated luminance
  const float2* moments;     // (sum l, sum l^2) per pixel, read by pass 0
  float sigma_l;             // sigma_luminance
};

// The firefly filter's one launch (rm_frame_kernels.inc "despeckle"): colour plane in, despeckled colour out.
struct DespecklePass {
  const float4* color;
  float4* out;
  int W, H;
  float s;            // 1 / samples
  float gain, floor;  // T = gain * t + floor
  int repair;         // != 0: an invalid centre takes the mean of its ordinary taps
};

// The display transform behind the blur (rm_frame_kernels.inc "the display transform"): RmDisplay as the kernel takes it.
struct DisplayPass {
  float gain;
  int tone;   // RM_TONE_*
  float w2;   // white * white, rounded once on the host (RM_TONE_REINHARD)
};

// rm_frame_stats' device counters (rm_frame_kernels.inc "frame statistics"): 64-bit, the bins first, then the three other classes,
// and behind them two 32-bit words: the complement of the minimum's key and the maximum's key.
enum {
  RM_STATS_BELOW = RM_STATS_BINS,
  RM_STATS_ABOVE,
  RM_STATS_NON_FINITE,
  RM_STATS_COUNTERS,
  RM_STATS_BYTES = RM_STATS_COUNTERS * 8 + 8,
  RM_STATS_GRID = 1024,  // workgroups at most: each adds its non-zero counters to the global ones once
};

namespace rm {
enum {
  WF_POS = 0,   // xyz ray position (march in/out), w = step budget
  WF_DIR,       // xyz ray direction, w = deltaZ (preview)
  WF_OLD,       // xyz position at the start of the bounce, w = rng.seed
  WF_ALB,       // xyz albedo accumulated over bounces
  WF_LIG,       // xyz light accumulated over bounces
  WF_NRM,       // xyz normal of the current bounce
  WF_PDIR,      // xyz prevRayDirection
  WF_DIF,       // xyz diffuseCol
  WF_SPC,       // xyz specularCol
  WF_PALB,      // xyz prevAlbedo
  WF_ADJ,       // xyz adjustedLightPosition, w = distance(rayPosition, adjustedLightPosition)
  WF_CONTRIB,   // xyz what the current light adds if its shadow test passes (:368-371)
  WF_SPOS,      // shadow ray position (march in/out), w = step budget
  WF_SDIR,      // shadow ray direction
  WF_AUX,       // preview: x = stepsTaken, y = depth
  WF_ARRAYS
};

struct WfParams {
  KParams k;
  float4* a[WF_ARRAYS];
  unsigned int* head;  // queue head of THIS march launch (zeroed by the host)
  const unsigned int* list_in;        // pass 2: the queue is list_in[0 .. *list_in_count)
  const unsigned int* list_in_count;
  unsigned int* list_out;             // where this launch parks rays (pass 1: rays that need the deep evaluation;
  unsigned int* list_out_count;       //   pass 2 with repark > 0: the survivors of thinned-out waves); zeroed by the host
  int repark;                         // pass 2: once the queue is drained, a wave with <= repark active lanes parks them and exits
  unsigned long long* stats;  // RM_WF_STATS builds: [shadow?][pass2?][rays, lane-steps, wave-steps, -]
  int n_rays;          // tiles_x * tiles_y * 64
  int tiles_x;
  int bounce;          // current bounce index
  int light;           // current light index
  int last_bounce;     // 1: this is the last bounce of the sample
  int pos_array, dir_array;  // which arrays the march kernel works on
  int claims_per_wave;       // queue chunks a wave claims over a launch, on average
};

// pass 0: single pass; 1: cheap pass (parks rays that need the deep evaluation); 2: full pass over the parked list
hipError_t wf_launch_march_strict(const WfParams& W, bool preview, int pass, int blocks, hipStream_t stream);
hipError_t wf_launch_march_fast(const WfParams& W, bool preview, int pass, int blocks, hipStream_t stream);
hipError_t launch_combine(const KParams& P, hipStream_t stream);
// scratch: 64 counters per RM_ORDER_TILES_PER_GROUP tiles (rm_order_scratch_elems)
hipError_t launch_order(unsigned int* cost, unsigned int* order, unsigned int* scratch, int n, hipStream_t stream);
inline size_t rm_order_scratch_elems(long long tiles) { return (size_t)(64 * ((tiles + 4095) / 4096)); }
hipError_t launch_cull_build(const CullBuild& B, hipStream_t stream);
void pixel_grid(const KParams& P, int* gx, int* gy);  // workgroup grid the pixel kernel uses for this job
hipError_t wf_launch_shade_strict(const WfParams& W, hipStream_t stream);
hipError_t wf_launch_shade_fast(const WfParams& W, hipStream_t stream);
bool wf_kind_has_cost_classes(int kind);
hipError_t launch_assemble(const void* src, int parts, int max_rows, long long row_bytes, int H, int stripe_rows, void* dst, hipStream_t stream);
hipError_t launch_pack_rows(const float4* color, const void* normal_dof, bool nd_half, long long pixels, float4* out, hipStream_t stream);
// one plane between fp32 and half (rm_fb_upload / rm_fb_download of a half plane): narrow = fp32 -> half with rm_narrow, else rm_widen
hipError_t launch_convert(const void* src, void* dst, long long pixels, bool narrow, hipStream_t stream);
hipError_t launch_present_rows(const float4* color, long long pixels, float brightness, uchar4* out, hipStream_t stream);
// one pass of rm_denoise (rm_frame_kernels.inc "denoise"); half: the G-buffer planes hold rm_half4
hipError_t launch_denoise_pass(const DenoisePass& P, bool half, bool prep, bool last, hipStream_t stream);
// one pass of rm_denoise_variance (the same, x.w = the variance; P.moments read by pass 0)
hipError_t launch_denoise_variance_pass(const DenoisePass& P, bool half, bool prep, bool last, hipStream_t stream);
// the firefly filter ahead of the denoisers (rm_filter*); radius 1 or 2, rank 0..3
hipError_t launch_despeckle(const DespecklePass& P, int radius, int rank, hipStream_t stream);
hipError_t launch_present(const float4* color, const void* normal_dof, bool nd_half, int W, int H, float brightness, uchar4* out, hipStream_t stream);
hipError_t launch_present_striped(const float4* color, const float4* normal_dof, int W, int H, float brightness, uchar4* out, int stripe_rows, int parts, int part,
                                  int local_rows, hipStream_t stream);
// rm_present's pass ending in the display transform: W x H uchar4, or with `linear` W x H float4 (e.rgb, 1)
hipError_t launch_present_display(const float4* color, const void* normal_dof, bool nd_half, int W, int H, float brightness, const DisplayPass& D, bool linear,
                                  void* out, hipStream_t stream);
// the luminance histogram of `pixels` float4 colours into RM_STATS_BYTES of zeroed counters (rm_frame_stats)
hipError_t launch_frame_stats(const float4* color, long long pixels, float s, unsigned long long* counters, hipStream_t stream);
hipError_t wf_launch_stage(const WfParams& W, int stage, hipStream_t stream);
hipError_t launch_pixels_strict(const KParams& P, hipStream_t stream);
hipError_t launch_pixels_fast(const KParams& P, hipStream_t stream);
hipError_t launch_probe_strict(const ProbeParams& P, hipStream_t stream);
hipError_t launch_probe_fast(const ProbeParams& P, hipStream_t stream);
// rm_mesh_kernels.inc: the grid sampler in each unit's arithmetic; the mesher's three steps (strict unit only, arithmetic-independent)
hipError_t launch_sdf_grid_strict(const SdfGridParams& P, hipStream_t stream);
hipError_t launch_sdf_grid_fast(const SdfGridParams& P, hipStream_t stream);
hipError_t launch_mesh_occlusion_strict(const MeshOcclusionPass& P, hipStream_t stream);
hipError_t launch_mesh_occlusion_fast(const MeshOcclusionPass& P, hipStream_t stream);
size_t rm_mesh_scan_scratch_elems(long long cells);  // 64-bit words of scratch launch_mesh_scan needs behind the counts
hipError_t launch_mesh_count(const MeshParams& P, hipStream_t stream);
hipError_t launch_mesh_scan(unsigned long long* counts, long long cells, unsigned long long* scratch, unsigned long long* total, hipStream_t stream);
hipError_t launch_mesh_emit(const MeshParams& P, hipStream_t stream);
hipError_t launch_mesh_slab_tally(const MeshSlab& S, hipStream_t stream);
hipError_t launch_mesh_slab_count(const MeshSlab& S, hipStream_t stream);
hipError_t launch_mesh_slab_emit(const MeshSlab& S, hipStream_t stream);
hipError_t launch_mesh_colours(const float* material, float* colours, long long vertices, hipStream_t stream);  // 12 floats per vertex -> the first 3
// rm_mesh_extract_sharp's two kernels.  cross: `init` makes the brackets from the corner values (else they are read), `consume` takes a round's
// probe output in, `last` writes the crossings and the live mask (else the next round's midpoints and the brackets).  qef: the vertex positions.
hipError_t launch_mesh_cross(const MeshSharpParams& P, int init, int consume, int last, hipStream_t stream);
hipError_t launch_mesh_qef(const MeshSharpParams& P, hipStream_t stream);
// Components and islands (rm_mesh_components, rm_mesh_filter): integer kernels over a mesh's vertices (n = V) and triangles (n = T).
// link_init: parent[v] = v.  link_hook: every triangle unites its vertices' trees, *changed = 1 when it met two roots.  link_flatten: parent[v]
// = root(v).  roots: words[v] = (parent[v] == v), for the scan; labels: labels[v] = scanned words[parent[v]].  part_sizes: sizes[2 c + slot]
// += 1 per vertex (triangles == NULL, slot 0) or per triangle (slot 1) of component c.  keep_flags: words[i] = keep[component of vertex or
// triangle i].  gather_vertices / gather_triangles: the kept rows to their scanned places, the triangles' indices remapped.
struct MeshGather {
  const unsigned int* labels;
  const unsigned int* keep;            // per component: 0 or 1
  const unsigned long long* vertex_at;  // the scanned vertex keep flags
  const unsigned int* src[4];           // positions, normals, colours (3 words per vertex; NULL when absent), cells (1 word)
  unsigned int* dst[4];
};
hipError_t launch_mesh_link_init(unsigned int* parent, long long vertices, hipStream_t stream);
hipError_t launch_mesh_link_hook(unsigned int* parent, const unsigned int* triangles, long long vertices, long long n, unsigned int* changed, hipStream_t stream);
hipError_t launch_mesh_link_flatten(unsigned int* parent, long long vertices, hipStream_t stream);
hipError_t launch_mesh_roots(const unsigned int* parent, unsigned long long* words, long long vertices, hipStream_t stream);
hipError_t launch_mesh_labels(const unsigned int* parent, const unsigned long long* scanned, unsigned int* labels, long long vertices, hipStream_t stream);
hipError_t launch_mesh_part_sizes(const unsigned int* labels, const unsigned int* triangles, long long n, unsigned int* sizes, int slot, hipStream_t stream);
hipError_t launch_mesh_keep_flags(const unsigned int* labels, const unsigned int* triangles, const unsigned int* keep, long long n, unsigned long long* words,
                                  hipStream_t stream);
hipError_t launch_mesh_gather_vertices(const MeshGather& G, long long vertices, hipStream_t stream);
hipError_t launch_mesh_gather_triangles(const MeshGather& G, const unsigned int* triangles, const unsigned long long* triangle_at, long long n,
                                        unsigned int* out, hipStream_t stream);
// Simplification (rm_mesh_simplify): vertex clustering over a mesh's arrays.  grid: the CLUSTER grid (nc = cells + 1 per axis).  sums: one row of
// `row` 64-bit words per output vertex -- the count, the three q sums, then the Q20 sums of the normals and of the colours where the source has
// them.  simplify_mark: marks[key of v] = 1.  simplify_sums (behind the scan of the marks): vertex_to[v] = the scanned mark, the row's atomic
// adds, cells[that] = key.  simplify_place: one thread per output vertex, the rows into positions / normals / colours.  simplify_map: mapped[t]
// = the triangle's corners through vertex_to, words[t] = 1 if no two are equal, else 0.  simplify_insert: every survivor into `table` (slots of
// 0xFFFFFFFF, a power of two of them), words[t] = its slot + 1; *error = 1 where a probe went round.  simplify_keep: words[t] = 1 iff the slot
// holds t.  simplify_gather (behind the scan of words[0 .. T], words[T] = 0): the kept triangles, those whose scanned word differs from the next.
struct MeshSimplify {
  GridDims grid;
  long long vertices, out_vertices, triangles;
  const float* positions;              // the source's: V x 3
  const float* normals;                // V x 3 or NULL
  const float* colours;                // V x 3 or NULL
  const unsigned int* source_triangles;  // T x 3
  unsigned long long* marks;           // per cluster cell
  unsigned long long* sums;            // out_vertices x row
  int row;                             // 4, 7 or 10
  unsigned int* vertex_to;             // V
  float* out_positions;                // out_vertices x 3
  float* out_normals;
  float* out_colours;
  unsigned int* out_cells;
  unsigned int* mapped;                // T x 3
  unsigned long long* words;           // T + 1
  unsigned int* table;
  unsigned long long slots;            // a power of two
  unsigned int* error;
  unsigned int* out_triangles;
};
// Quadric placement (rm_mesh_simplify_quadric) on top of a simplification: quadric_sums (behind simplify_place) adds every source triangle's
// plane to the rows of its corners' clusters, ten 64-bit words each (a00 a01 a02 a11 a12 a22 b0 b1 b2 in Q24, planes); quadric_place
// overwrites the positions of the output vertices that have planes.
struct MeshQuadric : MeshSimplify {
  unsigned long long* quadrics;  // out_vertices x 10
  float scale[3];                // h[a] / max h
  float threshold;
};
hipError_t launch_mesh_simplify_mark(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_simplify_sums(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_simplify_place(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_simplify_map(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_simplify_insert(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_simplify_keep(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_simplify_gather(const MeshSimplify& S, hipStream_t stream);
hipError_t launch_mesh_quadric_sums(const MeshQuadric& S, hipStream_t stream);
hipError_t launch_mesh_quadric_place(const MeshQuadric& S, hipStream_t stream);
// Measures and edge topology (rm_mesh_measure): integer kernels over a mesh's triangles, the slots of an edge table and its vertices, and the
// double-precision terms of area and volume with their fixed-tree sums.  totals: RM_MEASURE_WORDS 64-bit words, set by the host before the
// first launch (the extent's six words to the identities of min and max, everything else 0).  measure_edges: one thread per triangle, its
// three edges into the table (keys of all-ones, a power of two of them; counts of 0), used[v] = 1 for its corners.  measure_classes: one thread
// per slot.  measure_used: one thread per vertex, counts the flags.  measure_extent: one thread per vertex.  measure_terms (behind
// measure_extent: it reads the extent's low corner): one thread per triangle, and the first level of the tree; measure_sum: one further level,
// n values of each of the two lists into ceil(n / 256).
enum {
  RM_MEASURE_SKIPPED, RM_MEASURE_USED, RM_MEASURE_EDGES, RM_MEASURE_BOUNDARY, RM_MEASURE_REGULAR, RM_MEASURE_IRREGULAR, RM_MEASURE_UNBALANCED,
  RM_MEASURE_UNMEASURED, RM_MEASURE_FINITE, RM_MEASURE_ERROR,
  RM_MEASURE_EXTENT,                         // three words: six uint32, lo[3] then hi[3], floats in an order-preserving integer code
  RM_MEASURE_AREA = RM_MEASURE_EXTENT + 3,   // the two sums, as doubles
  RM_MEASURE_VOLUME,
  RM_MEASURE_WORDS
};
struct MeshMeasure {
  long long vertices, triangles;
  const float* positions;         // V x 3
  const unsigned int* corners;    // T x 3
  const unsigned int* labels;     // V
  unsigned long long* keys;       // slots
  unsigned long long* counts;     // slots: uses x -> y in the low half, y -> x in the high half
  unsigned long long slots;       // a power of two
  unsigned int* used;             // V
  unsigned long long* totals;     // RM_MEASURE_WORDS
  unsigned long long* rows;       // components x 4: edges, boundary, irregular, unbalanced
};
hipError_t launch_mesh_measure_edges(const MeshMeasure& M, hipStream_t stream);
hipError_t launch_mesh_measure_classes(const MeshMeasure& M, hipStream_t stream);
hipError_t launch_mesh_measure_used(const MeshMeasure& M, hipStream_t stream);
hipError_t launch_mesh_measure_extent(const MeshMeasure& M, hipStream_t stream);
// area[g], volume[g] = the tree sums of group g's 256 triangles
hipError_t launch_mesh_measure_terms(const MeshMeasure& M, double* area, double* volume, hipStream_t stream);
hipError_t launch_mesh_measure_sum(const double* area, const double* volume, long long n, double* out_area, double* out_volume, hipStream_t stream);
// Projection (rm_mesh_project).  project_eval, in each unit's arithmetic: d and, where a wave needs them, the normals at the round's positions.
// project_step (strict unit: plain fp32): round r >= 0 takes one step of every vertex from (d, normals), counts the moved ones into
// totals[RM_PROJECT_MOVED + r], keeps the flags, and in round 0 makes the report's "before" half; round -1 moves nothing: d is the distance at
// the final positions, and it writes the residual, the report's "after" half and the counts over the flags.  A report half: the counts, the
// key of the maximum, and the first level of the two fixed-tree sums into sum[g], sum2[g] (launch_mesh_measure_sum makes the further levels).
// project_flips: one thread per triangle.  totals: RM_PROJECT_WORDS 64-bit words, zeroed by the host before the first launch.
enum {
  RM_PROJECT_SETTLED_BEFORE, RM_PROJECT_SETTLED_AFTER, RM_PROJECT_NONFINITE_BEFORE, RM_PROJECT_NONFINITE_AFTER, RM_PROJECT_MOVED_VERTICES,
  RM_PROJECT_CLAMPED, RM_PROJECT_UNDIRECTED, RM_PROJECT_FLIPPED,
  RM_PROJECT_KEY_BEFORE, RM_PROJECT_KEY_AFTER,  // bits(|e|) << 32 | (0xFFFFFFFF - v), maximised; 0: no finite e
  RM_PROJECT_SUM_BEFORE, RM_PROJECT_SUM2_BEFORE, RM_PROJECT_SUM_AFTER, RM_PROJECT_SUM2_AFTER,  // doubles
  RM_PROJECT_MOVED,                             // 16 words: the vertices that round r moved
  RM_PROJECT_WORDS = RM_PROJECT_MOVED + 16
};
enum { RM_PROJECT_FLAG_CLAMPED = 1, RM_PROJECT_FLAG_UNDIRECTED = 2 };
struct MeshProject {
  long long vertices, triangles;
  const float* source;          // V x 3: p0
  float* positions;             // V x 3: p
  const float* d;               // V
  const float* normals;         // V x 3
  float* residual;              // V: written by round -1
  unsigned int* flags;          // V
  const unsigned int* corners;  // T x 3
  unsigned long long* totals;   // RM_PROJECT_WORDS
  float iso, relax, tolerance, reach;
};
hipError_t launch_mesh_project_eval_strict(const MeshProjectEval& P, hipStream_t stream);
hipError_t launch_mesh_project_eval_fast(const MeshProjectEval& P, hipStream_t stream);
hipError_t launch_mesh_project_step(const MeshProject& S, int round, double* sum, double* sum2, hipStream_t stream);
hipError_t launch_mesh_project_flips(const MeshProject& S, hipStream_t stream);
// Deviation (rm_mesh_deviation).  deviation_eval, in each unit's arithmetic: d at every (triangle, sample).  deviation_reduce (strict unit:
// plain fp32 and double): one lane per sample; per triangle max_t into triangle_max[t] and the four terms into terms[k * T + t] (k = area,
// over_area, area * mean, area * ms), the counts and the key of the maximum into totals.  launch_mesh_measure_sum makes every level of the
// two pairs' trees.  totals: RM_DEVIATION_COPIES x RM_DEVIATION_WORDS 64-bit words, zeroed by the host before the launch: workgroup b adds its
// counts and its key to copy b % RM_DEVIATION_COPIES, the host combines the copies; the trees' four sums are in copy 0.
enum {
  RM_DEVIATION_SKIPPED, RM_DEVIATION_UNEVALUATED, RM_DEVIATION_NONFINITE, RM_DEVIATION_OVER,
  RM_DEVIATION_KEY,  // bits(max_t) << 32 | (0xFFFFFFFF - t), maximised over the evaluated triangles; 0: none
  RM_DEVIATION_AREA, RM_DEVIATION_OVER_AREA, RM_DEVIATION_SUM1, RM_DEVIATION_SUM2,  // doubles
  RM_DEVIATION_WORDS = 10,
  RM_DEVIATION_COPIES = 256
};
struct MeshDeviation {
  long long vertices;
  int triangles;                // T << log2_samples < 2^31
  int log2_samples;
  const float* positions;       // V x 3
  const unsigned int* corners;  // T x 3
  const float* d;               // T x S
  float* triangle_max;          // T
  double* terms;                // 4 x T
  unsigned long long* totals;   // RM_DEVIATION_COPIES x RM_DEVIATION_WORDS
  float iso, tolerance;
};
hipError_t launch_mesh_deviation_eval_strict(const MeshDeviationSdf& P, hipStream_t stream);
hipError_t launch_mesh_deviation_eval_fast(const MeshDeviationSdf& P, hipStream_t stream);
hipError_t launch_mesh_deviation_reduce(const MeshDeviation& D, hipStream_t stream);
// Refinement (rm_mesh_refine), one round.  refine_edges: one thread per triangle, its three edges into the table (the measures' key and hash;
// keys and owners of all-ones, a power of two of them), atomicMin of the using slot 3 t + s into the edge's owner.  refine_flags: one thread per
// using slot, words[u] = 1 iff u owns its edge; the host scans the words.  refine_number: one thread per using slot, edge_of[u] = the scanned
// word of its edge's owner (all-ones for a slot of a triangle that takes no part), and the owner writes the edge's ends.  refine_eval, in each
// unit's arithmetic: d at every edge's midpoint.  refine_mark (plain fp32): marked[e], marks[e] (for the scan), the counts and the maximum.
// refine_count: one thread per triangle, words[t] = its number of children; the host scans marks and words.  refine_vertices: one thread per
// edge, a marked edge writes its vertex.  refine_emit: one thread per triangle.  totals: RM_REFINE_WORDS 64-bit words, zeroed by the host.
enum { RM_REFINE_EDGES, RM_REFINE_SPLIT, RM_REFINE_CHILDREN, RM_REFINE_NONFINITE, RM_REFINE_MAX, RM_REFINE_ERROR, RM_REFINE_WORDS };
struct MeshRefine {
  long long vertices, triangles;
  long long edges;                // E: known behind the first scan
  const float* positions;         // V x 3
  const float* colours;           // V x 3 or NULL
  const unsigned int* cells;      // V
  const unsigned int* corners;    // T x 3
  unsigned long long* keys;       // slots
  unsigned long long* owners;     // slots
  unsigned long long slots;       // a power of two
  unsigned long long* words;      // 3 T: the owner flags and their scan; then T: the children and their scan
  unsigned int* edge_of;          // 3 T
  unsigned int* ends;             // E x 2
  const float* d;                 // E
  unsigned int* marked;           // E
  unsigned long long* marks;      // E: marked, and its scan
  unsigned long long* totals;     // RM_REFINE_WORDS
  float* out_positions;           // V' x 3
  float* out_colours;             // V' x 3 or NULL
  unsigned int* out_cells;        // V'
  unsigned int* out_corners;      // T' x 3
  float iso, tolerance, min_edge2;  // min_edge2 = min_edge * min_edge, rounded once on the host
};
hipError_t launch_mesh_refine_edges(const MeshRefine& R, hipStream_t stream);
hipError_t launch_mesh_refine_flags(const MeshRefine& R, hipStream_t stream);
hipError_t launch_mesh_refine_number(const MeshRefine& R, hipStream_t stream);
hipError_t launch_mesh_refine_eval_strict(const MeshRefineMidpoints& P, hipStream_t stream);
hipError_t launch_mesh_refine_eval_fast(const MeshRefineMidpoints& P, hipStream_t stream);
hipError_t launch_mesh_refine_mark(const MeshRefine& R, hipStream_t stream);
hipError_t launch_mesh_refine_count(const MeshRefine& R, hipStream_t stream);
hipError_t launch_mesh_refine_vertices(const MeshRefine& R, hipStream_t stream);
hipError_t launch_mesh_refine_emit(const MeshRefine& R, hipStream_t stream);
hipError_t launch_camera_rng(const RmUniforms& u, int W, int H, int what, int count, float* out, hipStream_t stream);
hipError_t launch_math_probe(int fn, const float* a, const float* b, int n, float* out, hipStream_t stream);
}  // namespace rm
