// rm_kernels.inc -- the per-pixel kernel (one thread = one pixel-sample = one
// run of raymarcher.frag main(), :178-388) and the probe kernels.  Included by
// rm_strict.hip (RM_BUILD_FAST 0) and rm_fast.hip (RM_BUILD_FAST 1) after rm_device.hpp.
//
// Launch shape: each 64-lane wavefront owns an 8x8 pixel tile (compact tiles keep
// the lanes of a wave on similar rays); a workgroup is 4 waves = 16x16 pixels, or
// 8 waves = 16x32 for the Mandelbulb (BlockShape).  The scene table is staged once
// per workgroup in LDS.  What the kernel does about rays of very different length,
// in the order it is explained below:
//   * a lane stops at its own settle step, a wave when all its lanes have (cast_ray);
//   * the rays still marching are packed into fewer waves through LDS every
//     RM_REPACK_STEPS steps (cast_ray_block, preview_march_block; compacting kinds);
//   * registers are capped so that 8 waves fit a SIMD (RM_PIXEL_WAVES_PER_EU);
//   * tiles start most-expensive-first by their cost in the previous sample
//     (KParams::block_order, rm_order_kernel);
//   * full-mode samples can leave their result in a staging buffer instead of
//     blending it (KParams::stage), so that consecutive samples overlap (rm_api.hip).
// None of these changes a bit of the result.
//
// Retire (all builds, exact).  The reference marches a FIXED number of steps
// (:163-170, the early-out at :167 is commented out).  The march is the
// iteration p <- p + dir*sdf(p) of a deterministic function, so once a lane's p is
// bitwise unchanged by a step it is at a fixed point and every later step
// reproduces it (converged on a smooth surface, or overflowed to a stable
// +-Inf/NaN pattern): it can stop with bit-identical results.  RM_RENDER_FAST can
// additionally retire lanes whose step is below a tolerance (retire_eps, opt-in:
// it changes the image, see the header).

namespace rm {

// One sdf evaluation of the march.  RM_FARFIELD_PM=1 (off by default) makes the
// fast build fall back to the precise policy for lanes beyond 2^16 in any
// coordinate, where fp32 absorbs the scene and what a ray does next (e.g. a
// shadow ray cast from ~1e18 away landing exactly on the origin by
// cancellation, :279,:362) depends on the exact rounding sequence.  Measured
// on MI355X: it does not change the statistics of those pixels (means agree
// to 1e-4 either way) but costs 4.5x on the headline config (VGPR 52 -> 111,
// precise evaluator inside the hot loop), so it is not the default.
template <int KIND, class M>
RM_DEV float march_sdf(const DevScene& sc, const SceneLds& lds, v3 p) {
#ifndef RM_FARFIELD_PM
#define RM_FARFIELD_PM 0
#endif
  if (M::fast && RM_FARFIELD_PM) {
    const bool far = !(gmax(fabsf(p.x), gmax(fabsf(p.y), fabsf(p.z))) <= 65536.0f);
    if (far) return Sdf<KIND>::template eval<PM>(sc, lds, p);
  }
  return Sdf<KIND>::template eval<M>(sc, lds, p);
}

// castRay, :163-170.  M = math policy of the march.  A lane stops at its OWN
// settle step (bitwise fixed point, or the tolerance of the fast build) and
// keeps that position while the wave finishes -- the same rule as the wavefront
// march (rm_wavefront.inc), so both implementations give the same bits and the
// result of a ray does not depend on its neighbours; the wave leaves the loop
// when all its lanes have stopped.
template <int KIND, class M>
RM_DEV v3 cast_ray(const DevScene& sc, const SceneLds& lds, v3 p, v3 dir, float steps, float retire_eps, bool jump = true, int need_e = 1000) {
  bool done = false;
  if constexpr (!(ExactExits<M>::value && FarJump<KIND>::value)) jump = false;
  else jump = jump && Sdf<KIND>::far_jump_applies(sc);
  if constexpr (ExactExits<M>::value && IsBigTable<KIND>::value) {  // a ray that passes every shape at a distance: its end state (rm_device.hpp clear_miss)
    const int left0 = (int)gmin(ceilf(steps), 1048576.0f);
    const bool ask = jump && steps > 0.0f && Sdf<RM_SCENE_TABLE>::clear_miss_applies(sc, p, dir, left0);
    if (ballot(ask) != 0ull && ask && Sdf<RM_SCENE_TABLE>::clear_miss(sc, lds, p, dir, left0)) return Sdf<RM_SCENE_TABLE>::far_end_state(sc, dir);
  }
  for (float i = 0.0f; i < steps; i += 1.0f) {
    if constexpr (ExactExits<M>::value && FarJump<KIND>::value) {  // an escaping ray with enough steps left: its end state (rm_device.hpp far_jump)
      if (jump && !done) {
        v3 end;
        if (Sdf<KIND>::far_jump(sc, p, dir, (int)gmin(steps - i, 1048576.0f), end)) { p = end; done = true; }  // (steps left, rounded down: the safe side here)
        if constexpr (IsBigTable<KIND>::value)  // a shadow ray (need_e < 1000) whose comparison is certain (rm_device.hpp far_shadow_escape): steps left, exactly
          if (!done && need_e < 1000 && far_shadow_escape(p, dir, (int)gmin(ceilf(steps - i), 1048576.0f), sc.far_r2, need_e, end)) { p = end; done = true; }
      }
    }
    if (!done) {
      const float d = march_sdf<KIND, M>(sc, lds, p);
      // the position update is NOT fused in any build: a shadow ray cast from ~1e18
      // away lands on the origin by exact cancellation of the two-rounding mul+add
      // (as in GLSL); an FMA leaves a ~1e11 residual instead, the ray misses the
      // scene and whole skies of multi-bounce renders gain a light quantum (+3 %)
      const v3 q = p + dir * d;
      done = same_bits(p, q);
      if (M::fast && retire_eps > 0.0f)
        done = done || fabsf(d) <= retire_eps * gmax(1.0f, gmax(fabsf(q.x), gmax(fabsf(q.y), fabsf(q.z))));
      p = q;
    }
    if (ballot(!done) == 0ull) break;  // every lane of the wave has stopped
  }
  return p;
}

// sceneNormal, :153-160 (forward differences)
// Math of the evaluations outside the march (normals, subsurface test): precise in the parity build, the
// fast policy in the fast build.  Measured (tools/normal_study.py, six scenes, 32 spp): the mean of the
// pixels that differ from the parity build stays within its standard error (Mandelbulb 0.998 +- 0.0013),
// and the headline frame gains 12 %.
#ifndef RM_NORMAL_POLICY
#if RM_BUILD_FAST
#define RM_NORMAL_POLICY FM
#else
#define RM_NORMAL_POLICY PM
#endif
#endif
using NM = RM_NORMAL_POLICY;
template <int KIND>
RM_DEV v3 scene_normal(const DevScene& sc, const SceneLds& lds, v3 p, float delta) {
  if (!RM_GL_STACK && Sdf<KIND>::nonfinite_normal_is_nan(sc) && any_nonfinite(p)) {  // escaped ray: the result is known (rm_device.hpp)
    const float nan = __builtin_nanf("");
    return V(nan, nan, nan);
  }
  const float at = Sdf<KIND>::template eval<NM>(sc, lds, p);
  return normalize<PM>(V(Sdf<KIND>::template eval<NM>(sc, lds, V(p.x + delta, p.y, p.z)) - at,
                         Sdf<KIND>::template eval<NM>(sc, lds, V(p.x, p.y + delta, p.z)) - at,
                         Sdf<KIND>::template eval<NM>(sc, lds, V(p.x, p.y, p.z + delta)) - at));
}

// The material values at p: the scene's constants, or -- a primitive table whose shapes name surfaces -- those of the
// nearest shape (rm_device.hpp surface_index; the index evaluation on the policy of the other evaluations outside the march).
template <int KIND>
RM_DEV Surface surface_at(const DevScene& sc, const SceneLds& lds, v3 p) {
  if constexpr (IsTable<KIND>::value && KIND != RM_KIND_TABLE_SMOOTH) {  // (the smooth-union kernel is not launched for tables with surfaces)
    if (sc.table_flags & RM_TABLE_HAS_SURFACES) {  // kernel-uniform
      const int k = Sdf<KIND>::template surface_index<NM>(sc, lds, p);
      const float4 a = lds.surf[3 * k], b = lds.surf[3 * k + 1], c = lds.surf[3 * k + 2];
      return Surface{V(a.x, a.y, a.z), V(b.x, b.y, b.z), V(c.x, c.y, c.z), a.w, b.w, c.w};
    }
  }
  return scene_surface(sc);
}
template <int KIND>
RM_DEV bool has_surfaces(const DevScene& sc) { return IsTable<KIND>::value && KIND != RM_KIND_TABLE_SMOOTH && (sc.table_flags & RM_TABLE_HAS_SURFACES) != 0; }

// ---- workgroup-level ray compaction for the march of the pixel kernel ---------------------------
// The 256 rays of a workgroup (a 16x16 pixel tile) settle at very different steps, and in an 8x8
// wave the slowest lane decides (on the headline frame half of the lanes of the executed VALU
// instructions were idle, SQ_THREAD_CYCLES_VALU).  Every RM_REPACK_STEPS steps the four waves of
// the workgroup count their rays still marching; when those fit into fewer waves, the rays move
// -- through LDS -- to the low lanes of the workgroup, so that whole waves fall idle (an idle wave
// skips the march body) instead of every wave running with a few live lanes.  A ray carries its
// complete march state, is stepped by exactly the operations of cast_ray, and delivers its end
// point to the thread that owns its pixel: results are bit-identical to cast_ray.
// (Round 2 also tried a geometric two-class key at every repack -- rays inside |p| < 1.25, which run most of their
// rounds, to the low slots, the others behind them: rounds used / issued 0.794 -> 0.801, frame time unchanged.  The
// idle rounds are not a mix of far and near rays in one wave; they are neighbouring rays of the approach phase that
// differ by a round or two, and that changes from step to step.)
// (Also tried: ordering the rays by the round count of their last Mandelbulb evaluation at every
// repack, a counting sort through LDS, so that a wave holds rays of one cost -- 47 % of the issued
// lane-rounds are idle, tools/lane_stats.py.  The count of one step predicts the next ones badly:
// used/issued rounds went from 0.53 to 0.56 only and the frame from 3.7 to 4.0 ms.  Not kept.)
#ifndef RM_REPACK_STEPS
#define RM_REPACK_STEPS 16
#endif
// ... and every 8 for the tables: since their escaping rays leave at once (the far-field exits of rm_device.hpp) a table frame's
// lanes empty faster than the Mandelbulb's -- C5 after the shadow rays' exit: lanes active 0.68 -- and the barriers are cheap
// beside a 64-row fold.  Measured: C5 162.5 -> 153.2 ms, C4 12.25 -> 12.04 (4 steps: 155.7 / 12.17); the headline kernel 1.863 -> 1.878 with 8.
#ifndef RM_REPACK_STEPS_TABLE
#define RM_REPACK_STEPS_TABLE 8
#endif
template <int KIND> struct RepackSteps { static constexpr int value = IsTable<KIND>::value ? RM_REPACK_STEPS_TABLE : RM_REPACK_STEPS; };
// Scene kinds whose pixel kernel compacts (bit k = kind k).  Measured on MI355X: the Mandelbulb gains
// and the Menger
// sponge gain 9 % (lanes of one tile need very different step counts); on the table scenes and the other
// folded fractals the workgroup barriers cost more than the idle lanes did (+2 .. 5 %).
#ifndef RM_REPACK_KIND_MASK
#define RM_REPACK_KIND_MASK ((1u << RM_SCENE_MANDELBULB) | (1u << RM_KIND_BULB8) | (1u << RM_SCENE_MENGER) | (1u << RM_KIND_TABLE_BIG) | (1u << RM_KIND_TABLE_SMOOTH))
#endif
template <int KIND>
struct BlockRepack {
  static constexpr bool value = ((RM_REPACK_KIND_MASK >> KIND) & 1u) != 0u;
};

// Waves per workgroup of a compacting kernel: 4 (16x16 pixels), 8 (16x32) or 16 (32x32).  After compaction the
// last wave of a workgroup is partly filled for the rest of the march -- half a wave per workgroup that holds rays,
// which on the headline frame is most of what is left of the idle lanes -- so a larger workgroup wastes less, but
// its parked waves also hold more wave slots of the CU while a few waves creep.  Measured at 8 waves per SIMD
// (RM_PIXEL_WAVES_PER_EU): Mandelbulb 4K lit 3.35 / 3.13 / 3.20 ms and preview 1.68 / 1.50 / 1.52 for 4 / 8 / 16 waves;
// Menger sponge 5.33 / 5.48 / 7.07.  (At 4 waves per SIMD, where the compiler lands by itself, 2, 4 and 8 measured the
// same and 16 was 13 % slower: parked waves were the bottleneck.)
#ifndef RM_REPACK_WAVES
#define RM_REPACK_WAVES(KIND) ((KIND) == RM_SCENE_MANDELBULB || (KIND) == RM_KIND_BULB8 || (KIND) == RM_KIND_TABLE_BIG || (KIND) == RM_KIND_TABLE_SMOOTH ? 8 : 4)
#endif
template <int KIND>
struct BlockShape {
  static constexpr int waves = BlockRepack<KIND>::value ? RM_REPACK_WAVES(KIND) : 4;
  static constexpr int wx = waves == 16 ? 4 : 2, wy = waves / wx;  // waves across and up the workgroup's pixel tile
  // An 8-wave workgroup can also lie on its side (KParams::tile_wide: 4 waves across, 2 up = 32 x 16 pixels instead of
  // 16 x 32).  On a whole frame the shape does not matter (8 x 64 ... 64 x 8: 2.05-2.06 ms on the headline, builds with
  // -DRM_TILE_EXPERIMENT); but the 270 rows one of 8 GPUs holds are 9 upright tile rows with 6.7 % of the lanes beyond
  // the last row, against 17 rows and 0.7 % on the side -- 4 % of that rank's step.  tile_is_wide() picks the side when
  // it saves at least 3 % of the workgroups.
  static constexpr bool can_lie = waves == 8;
  static constexpr int threads = waves * 64, px = wx * 8, py = wy * 8;
};

template <int WAVES>  // 0: the kind does not compact
struct MarchSharedT {
  static constexpr int N = WAVES > 0 ? WAVES * 64 : 1;
  float4 pos_i[N];      // xyz position, w = steps left (int bits)
  float4 dir_steps[N];  // xyz direction, w = the thread that owns the ray's pixel (int bits)
  float4 result[N];     // end point of the ray owned by thread t
  int wave_count[WAVES > 0 ? WAVES : 1];
};

// (Round 3, tried: a fill order for the compaction that goes round the SIMDs -- HW_REG_HW_ID says where a wave sits --
// instead of packing the rays into the workgroup's first waves.  Unnecessary and harmful: the dispatcher already puts
// waves 0-3 of a workgroup on the four SIMDs of its CU and waves 4-7 on the same four again, and it starts every
// workgroup one SIMD further (tools/ubench/hwid_probe.hip: e.g. 1 3 0 2 | 1 3 0 2, the next workgroup of the CU 2 1 3 0),
// so the first waves ARE the balanced choice; an order built from the SIMD ids with a per-tile start was 3.5 % slower on
// the headline frame and 8 % on the Menger sponge -- which also says how much that balance is worth.)

template <int KIND, class M>
RM_DEV v3 cast_ray_block(const DevScene& sc, const SceneLds& lds, MarchSharedT<0>&, v3 p0, v3 dir0, float steps0, float retire_eps,
                         bool, bool jump, int need_e = 1000) {
  return cast_ray<KIND, M>(sc, lds, p0, dir0, steps0, retire_eps, jump, need_e);
}

template <int KIND, class M, int WAVES>
RM_DEV v3 cast_ray_block(const DevScene& sc, const SceneLds& lds, MarchSharedT<WAVES>& sm, v3 p0, v3 dir0, float steps0, float retire_eps,
                         bool wanted, bool jump, int need_e = 1000) {
  if constexpr (!(ExactExits<M>::value && FarJump<KIND>::value)) jump = false;
  else jump = jump && Sdf<KIND>::far_jump_applies(sc);  // kernel-uniform
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // the ray this lane is marching (its own to begin with), and how many steps it still has to take: the reference's
  // `for (float i = 0.; i < steps; i++)` runs ceil(steps) times (0 for steps <= 0 or NaN); a ray that settles, and
  // a lane without a ray, have 0 left -- the wave's live mask is one integer compare
  v3 p = p0, dir = dir0;
  int left = wanted && steps0 > 0.0f ? (int)ceilf(gmin(steps0, 16777216.0f)) : 0;
  int owner = tid;
  sm.result[tid] = make_float4(p0.x, p0.y, p0.z, 0.0f);  // rays with no step to take end where they start
  if constexpr (ExactExits<M>::value && IsBigTable<KIND>::value) {  // a ray that passes every shape at a distance: its end state (rm_device.hpp clear_miss)
    const bool ask = jump && left > 0 && Sdf<RM_SCENE_TABLE>::clear_miss_applies(sc, p, dir, left);
    if (ballot(ask) != 0ull) {
      if (ask && Sdf<RM_SCENE_TABLE>::clear_miss(sc, lds, p, dir, left)) {
        const v3 e = Sdf<RM_SCENE_TABLE>::far_end_state(sc, dir);
        sm.result[tid] = make_float4(e.x, e.y, e.z, 0.0f);
        left = 0;
      }
    }
  }
  __syncthreads();
  // one step of the lanes that have one to take, from position `a` to position `b` (two register sets used in turn:
  // the old position is needed for the settle test, and copying the new one back would cost three moves per step)
  auto step = [&](const v3& a, v3& b) {
    if constexpr (M::fast && FusedJump<KIND>::value && !RM_FARFIELD_PM) {  // the evaluation carries the jump's test (rm_device.hpp pow8_eval_or_jump)
      if (left > 0) {
        float d;
        if (Sdf<KIND>::template eval_or_jump<M>(sc, lds, a, dir, left, jump, d, b)) {
          left = 0;
          sm.result[owner] = make_float4(b.x, b.y, b.z, 0.0f);
        } else {
          b = a + dir * d;  // not fused, see cast_ray
          bool done = same_bits(a, b);
          if (retire_eps > 0.0f) done = done || fabsf(d) <= retire_eps * gmax(1.0f, gmax(fabsf(b.x), gmax(fabsf(b.y), fabsf(b.z))));
          left = done ? 0 : left - 1;
          if (left <= 0) sm.result[owner] = make_float4(b.x, b.y, b.z, 0.0f);
        }
      }
      return;
    }
    if constexpr (ExactExits<M>::value && FarJump<KIND>::value) {  // an escaping ray with enough steps left: its end state (rm_device.hpp far_jump)
      if (jump && left > 0 && Sdf<KIND>::far_jump(sc, a, dir, left, b)) {
        left = 0;
        sm.result[owner] = make_float4(b.x, b.y, b.z, 0.0f);
      }
      if constexpr (IsBigTable<KIND>::value) {  // a shadow ray whose comparison is certain (rm_device.hpp far_shadow_escape); need_e travels with the ray
        if (jump && left > 0 && need_e < 1000 && far_shadow_escape(a, dir, left, sc.far_r2, need_e, b)) {
          left = 0;
          sm.result[owner] = make_float4(b.x, b.y, b.z, 0.0f);
        }
      }
    }
    if (left > 0) {
      const float d = march_sdf<KIND, M>(sc, lds, a);
      b = a + dir * d;  // not fused, see cast_ray
      bool done = same_bits(a, b);
      if (M::fast && retire_eps > 0.0f)
        done = done || fabsf(d) <= retire_eps * gmax(1.0f, gmax(fabsf(b.x), gmax(fabsf(b.y), fabsf(b.z))));
      left = done ? 0 : left - 1;
      if (left <= 0) sm.result[owner] = make_float4(b.x, b.y, b.z, 0.0f);
    }
  };
  static_assert(RepackSteps<KIND>::value % 2 == 0, "the march body takes its steps in pairs");
#ifndef RM_REPACK_FIRST
#define RM_REPACK_FIRST 0  // 1 (measurement builds): pack the rays once BEFORE the first steps (rays that left at once -- an exit taken at step 0 -- never hold a lane)
#endif
#ifndef RM_REPACK_RAMP
#define RM_REPACK_RAMP 0   // n > 0 (measurement builds): the first rounds are short -- n, 2n, 4n ... steps up to the kind's round
#endif
  bool skip_march = RM_REPACK_FIRST != 0;
  int round_steps = RM_REPACK_RAMP > 0 ? RM_REPACK_RAMP : RepackSteps<KIND>::value;
  for (;;) {
    if (!skip_march && ballot(left > 0) != 0ull) {  // an idle wave skips the march body
      v3 q = p;
      bool in_q = false;  // wave-uniform: the current positions are in q
      for (int k = 0; k < round_steps; k += 2) {
        step(p, q);
        in_q = true;
        if (ballot(left > 0) == 0ull) break;
        step(q, p);
        in_q = false;
        if (ballot(left > 0) == 0ull) break;
      }
      if (in_q) p = q;
    }
    skip_march = false;
    if (RM_REPACK_RAMP > 0) round_steps = min(2 * round_steps, RepackSteps<KIND>::value);
    const bool active = left > 0;
    const unsigned long long mask = ballot(active);
    if (lane == 0) sm.wave_count[wave] = __popcll(mask);
    __syncthreads();
    // every wave adds up the counts itself: lane w holds wave w's count, a 16-lane prefix sum, two broadcasts
    const int mine = lane < WAVES ? sm.wave_count[lane] : 0;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < WAVES; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    const int total = __builtin_amdgcn_readfirstlane(__shfl(incl, WAVES - 1));  // (every lane holds the same sum: the compiler is told so, and the branches below are scalar)
    if (total == 0) break;
    const int used = __popcll(ballot(mine > 0)), needed = (total + 63) >> 6;
    if (needed < used) {  // workgroup-uniform
      const int base = __shfl(incl - mine, wave);
      if (active) {
        const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
        sm.pos_i[slot] = make_float4(p.x, p.y, p.z, __int_as_float(left));
        sm.dir_steps[slot] = make_float4(dir.x, dir.y, dir.z, __int_as_float(owner | ((need_e + 256) << 16)));
      }
      __syncthreads();
      left = 0;  // (rotating the wave that keeps the rays from workgroup to workgroup is 4 % slower: see above)
      if (tid < total) {
        const float4 a = sm.pos_i[tid], b = sm.dir_steps[tid];
        p = V(a.x, a.y, a.z);
        left = __float_as_int(a.w);
        dir = V(b.x, b.y, b.z);
        owner = __float_as_int(b.w) & 0xffff;
        need_e = (__float_as_int(b.w) >> 16) - 256;
      }
    }
    __syncthreads();  // wave_count and the staging arrays are rewritten in the next round
  }
  __syncthreads();
  const float4 r = sm.result[tid];
  return V(r.x, r.y, r.z);
}

// ---- the preview march (:207-221) --------------------------------------------------------------------
// One step of a preview ray: besides the position it keeps the index of the last step that still moved
// (stepsTaken, the shade of preview mode) and the depth along the view axis (focal-plane overlay).
struct PreviewRay {
  v3 p, dir;
  float i, delta_z, steps_taken, depth;
};

// returns true when the ray is finished (settled, or out of steps)
template <int KIND, class M>
RM_DEV bool preview_step(const DevScene& sc, const SceneLds& lds, const RmUniforms& u, float steps, float retire_eps, PreviewRay& r) {
  const float d = march_sdf<KIND, M>(sc, lds, r.p);
  v3 q = r.p;
  if (d < 100000000000.0f) {
    q = r.p + r.dir * d;  // not fused, see cast_ray
    r.depth += r.delta_z * d;
  }
  if (d > 0.0001f) r.steps_taken = r.i;
  bool settled = same_bits(r.p, q);
  if (M::fast && retire_eps > 0.0f)
    settled = settled || fabsf(d) <= retire_eps * gmax(1.0f, gmax(fabsf(q.x), gmax(fabsf(q.y), fabsf(q.z))));
  r.p = q;
  if (settled && r.i + 1.0f < steps) {  // fixed point: the remaining steps see the same d
    if (d > 0.0001f) r.steps_taken = ceilf(steps) - 1.0f;
    if (u.showDofFocalPlane != 0 && d < 100000000000.0f)
      for (float k = r.i + 1.0f; k < steps; k += 1.0f) r.depth += r.delta_z * d;
  }
  r.i += 1.0f;
  return settled || !(r.i < steps);
}

template <int WAVES>
struct PreviewShared {
  static constexpr int N = WAVES * 64;
  float4 pos_i[N], dir_dz[N], result[N];  // result: xyz end point, w = stepsTaken
  float2 taken_depth[N];
  float depth_out[N];
  int owner[N];
  int wave_count[WAVES];
};

// The preview march of a workgroup with the ray compaction of cast_ray_block (same scheme, same guarantees).
template <int KIND, class M, int WAVES>
RM_DEV void preview_march_block(const DevScene& sc, const SceneLds& lds, const RmUniforms& u, PreviewShared<WAVES>& sm, float steps,
                                float retire_eps, bool wanted, PreviewRay& r) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int owner = tid;
  bool active = wanted && r.i < steps;
  sm.result[tid] = make_float4(r.p.x, r.p.y, r.p.z, r.steps_taken);
  sm.depth_out[tid] = r.depth;
  __syncthreads();
  for (;;) {
    if (ballot(active) != 0ull) {
      for (int k = 0; k < RM_REPACK_STEPS; k++) {
        if (active && preview_step<KIND, M>(sc, lds, u, steps, retire_eps, r)) {
          sm.result[owner] = make_float4(r.p.x, r.p.y, r.p.z, r.steps_taken);
          sm.depth_out[owner] = r.depth;
          active = false;
        }
        if (ballot(active) == 0ull) break;
      }
    }
    const unsigned long long mask = ballot(active);
    if (lane == 0) sm.wave_count[wave] = __popcll(mask);
    __syncthreads();
    const int mine = lane < WAVES ? sm.wave_count[lane] : 0;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < WAVES; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    const int total = __builtin_amdgcn_readfirstlane(__shfl(incl, WAVES - 1));  // (every lane holds the same sum: the compiler is told so, and the branches below are scalar)
    if (total == 0) break;
    const int used = __popcll(ballot(mine > 0)), needed = (total + 63) >> 6;
    if (needed < used) {  // workgroup-uniform
      const int base = __shfl(incl - mine, wave);
      if (active) {
        const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
        sm.pos_i[slot] = make_float4(r.p.x, r.p.y, r.p.z, r.i);
        sm.dir_dz[slot] = make_float4(r.dir.x, r.dir.y, r.dir.z, r.delta_z);
        sm.taken_depth[slot] = make_float2(r.steps_taken, r.depth);
        sm.owner[slot] = owner;
      }
      __syncthreads();
      active = tid < total;
      if (active) {
        const float4 a = sm.pos_i[tid], b = sm.dir_dz[tid];
        const float2 c = sm.taken_depth[tid];
        r.p = V(a.x, a.y, a.z);
        r.i = a.w;
        r.dir = V(b.x, b.y, b.z);
        r.delta_z = b.w;
        r.steps_taken = c.x;
        r.depth = c.y;
        owner = sm.owner[tid];
      }
    }
    __syncthreads();
  }
  __syncthreads();
  const float4 e = sm.result[tid];
  r.p = V(e.x, e.y, e.z);
  r.steps_taken = e.w;
  r.depth = sm.depth_out[tid];
}

// ---- the launch's argument block, re-read where it is used (round 5) ---------------------------------------------------------
// KParams is ~200 dwords (the uniforms' light arrays, the material block, the culling grid's constants ...) and arrives in the kernarg
// segment.  Read as `P.field`, every load is an invariant scalar load that the compiler hoists to the top of the kernel and then
// has to keep: at 8 waves per SIMD a wave has 76 usable SGPRs, so C5's kernel spilled 269 of them into the lanes of a VGPR
// (v_writelane / v_readlane -- the culling grid's constants were re-read from v63 inside the march's loops) and that VGPR was one of
// its 64.  karg() hands out the same segment through a pointer the optimiser cannot see through (an empty asm on the SGPR pair), so
// a load from it is issued where the code stands -- an s_load at the start of a march or of a bounce's shading, dead at its end --
// and nothing of the block is carried across the marches.  Same values, same operations on them.
typedef const __attribute__((address_space(4))) KParams KArg;
RM_DEV KArg* karg() {
  KArg* p = (KArg*)__builtin_amdgcn_kernarg_segment_ptr();  // the kernel's only argument starts the segment
  asm volatile("" : "+s"(p));
  return p;
}
// a sub-block by value (scalar loads of the fields that are read; no field of DevScene is indexed by a variable)
template <class T>
RM_DEV T karg_load(const __attribute__((address_space(4))) T* p) {
  T r;
  __builtin_memcpy(&r, p, sizeof(T));
  return r;
}
#ifndef RM_KARG_FRESH
#define RM_KARG_FRESH 1  // 0: the argument block as the compiler likes it (measurement builds)
#endif

// Waves per SIMD the register allocation aims for.  Left alone the compiler takes ~100 registers for the full-mode
// kernel (4 waves per SIMD): fine for a SIMD whose waves all work, but waves parked by the compaction or waiting in a
// divergent stage leave it with one or two.  Capped at 64 registers (8 waves; some shading values spill, outside the
// march) the headline frame goes from 3.68 to 3.36 ms, the KIFS tree from 5.15 to 4.57; the sphere-grid fractal and
// the Menger sponge, whose folds keep more values live, are best at 6 (2.49 against 2.91 at 8 / 2.50 at 4).
#ifndef RM_PIXEL_WAVES_PER_EU
#define RM_PIXEL_WAVES_PER_EU(KIND) ((KIND) == RM_SCENE_SPHERE_GRID || (KIND) == RM_SCENE_MENGER ? 6 : 8)
#endif
// EPS: the opt-in retire tolerance of the fast build is in use (rm_ctx_set_retire_eps); the default kernels are
// compiled without the test (as an exec-masked region it would still be issued on every step)
// ONE_LIGHT: kernel variants by the SHAPE of the job (full mode, both builds since round 4; launch_kind picks).  The general kernel keeps a
// bounce's normal, directions, colours and the next ray alive across every shadow march, for the next light and the next bounce:
// 34 dwords that do not fit beside the march (132 B of scratch per lane on the headline kernel, 2.6 GB of traffic per frame against
// 0.8 GB of planes -- VERDICT r2 #7).  Most jobs do not need that generality, and a kernel that knows so has nothing to spill:
//   1: exactly one light -- its term is computed BEFORE its shadow march (it does not depend on it), so the bounce's values are
//      dead across it;
//   2: one light and one bounce (reflectionIterationCounts has one entry: BASELINE's C3b, C4) -- nothing of the bounce but the
//      light sum is alive across the shadow march: the headline kernel has NO scratch (2.00 -> 1.86 ms), CSG-64's 12 B;
// (Also built: a variant without any light code for jobs without lights -- the job the reference's page starts with.  Less
// scratch, 12 B against 24, and 16 % SLOWER on that job, 1.56 against 1.34 ms: not launched.)
// Same operations in the same order on the same values: the same bits as the general kernel (the GPU suite runs every job shape
// through both implementations).
template <int KIND, bool PREVIEW, bool FAST, bool EPS, int ONE_LIGHT = 0>
__global__ __launch_bounds__(BlockShape<KIND>::threads, RM_PIXEL_WAVES_PER_EU(KIND)) void rm_pixel_kernel(const KParams P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;  // math of the march
  const float retire_eps = EPS ? P.retire_eps : 0.0f;
  __shared__ SceneLds lds;
  __shared__ MarchSharedT<BlockRepack<KIND>::value ? BlockShape<KIND>::waves : 0> march_shared;
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();

  const RmUniforms& u = P.u;
  const DevScene& sc = P.scene;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  using Shape = BlockShape<KIND>;
  // which tile of the job this workgroup renders: in launch order, or the most expensive tiles of the previous
  // sample first (KParams::block_order), so that the launch does not end on a few late, long workgroups
  unsigned int tile_id = blockIdx.y * gridDim.x + blockIdx.x;
  // a batch launch (KParams::batch) has `batch` workgroups per tile, one per sample, next to each other in launch order
  unsigned int sample = 0;
  if (!PREVIEW && P.batch > 1) {
    sample = tile_id % (unsigned int)P.batch;
    tile_id /= (unsigned int)P.batch;
  }
  if (P.block_order != nullptr) tile_id = P.block_order[tile_id];
  const long long t_start = P.block_cost != nullptr ? (long long)__builtin_amdgcn_s_memtime() : 0ll;  // scalar
#ifdef RM_DIAG_TIMELINE  // diagnostic build (tools/timeline.py): when and where every workgroup ran
  const unsigned long long tl_start = __builtin_amdgcn_s_memrealtime();
#endif
  const int lg_wx = Shape::can_lie && P.tile_wide ? P.tile_wide - 1 : (Shape::wx == 4 ? 2 : 1);  // log2 of the waves across the tile
  const int tile_px = 8 << lg_wx, tile_py = (Shape::waves >> lg_wx) * 8;
  const int bx = (int)(tile_id % gridDim.x) * tile_px + (wave & ((1 << lg_wx) - 1)) * 8 + (lane & 7);
  const int by = (int)(tile_id / gridDim.x) * tile_py + (wave >> lg_wx) * 8 + (lane >> 3);
  const bool valid = bx < P.tw && by < P.th;
  // every wave reports when it is done; the tile's cost is the latest
  auto report_cost = [&]() {
    if (P.block_cost != nullptr && lane == 0) {
      const long long dt = ((long long)__builtin_amdgcn_s_memtime() - t_start) >> 6;
      atomicMax(&P.block_cost[tile_id], (unsigned int)(dt < 0 ? 0 : dt > 0x7fffffffll ? 0x7fffffffll : dt));
    }
  };
  // lanes outside the tile shadow the last valid pixel (no store) so that
  // wave ballots are not held up by rays nobody asked for
  const int px = P.tx + (bx < P.tw ? bx : P.tw - 1);
  const int ly = P.ty + (by < P.th ? by : P.th - 1);  // local (plane) row
  const int py = rm_global_row(P, ly);
  const size_t pix = (size_t)ly * (size_t)P.W + (size_t)px;

  // texcoord = (pixel centre) / size (raymarcher.vert:8-11); IEEE division in both builds
  const float tcx = ((float)px + 0.5f) / (float)P.W;
  const float tcy = ((float)py + 0.5f) / (float)P.H;
  const bool batched = !PREVIEW && P.batch > 1;
  // (Round 4, tried: the stream's two per-pixel constants parked in LDS in the variants that run at the register cap -- the allocator's
  // first victims there, reloaded from scratch twice per random number.  Scratch_Size of C5's kernel went UP, 192 -> 288 B (what the
  // allocator does with two freed registers is its own business), C5 stayed at 150 ms and the live five-bounce job lost 9 %.  Not kept.)
  Rng rng = rng_init(tcx, tcy, batched ? P.batch_noise[sample][0] : u.randNoise[0], batched ? P.batch_noise[sample][1] : u.randNoise[1]);

  // ---- camera, :180-205
  v3 dir = V(0.0f, 0.0f, 0.0f), pos = V(0.0f, 0.0f, 0.0f);
  const v3 cam = V(u.position[0], u.position[1], u.position[2]);
  float jx = uniform_sample(rng);
  float jy = uniform_sample(rng);
  jx = jx / (float)P.W * 1.0f;
  jy = jy / (float)P.H * 1.0f;
  const float t2x = tcx + jx, t2y = tcy + jy;
  float delta_z = 1.0f;
  if (u.cameraMode == 0) {
    const float th = rm_tan(u.fov / 2.0f);
    const float ppx = (t2x * 2.0f - 1.0f) * u.aspect * th;
    const float ppy = (t2y * 2.0f - 1.0f) * 1.0f * th;
    const v3 goal = mat_rotate(u.rotation, V(ppx + jx, ppy + jy, 1.0f)) * u.dofFocalPlaneDistance;
    // sphereSample() * dofAmount: the next draw of the stream (the goal does not draw), usually times 0
    const bool neg_zero = is_neg_zero(cam.x) || is_neg_zero(cam.y) || is_neg_zero(cam.z) || is_neg_zero(goal.x) || is_neg_zero(goal.y) || is_neg_zero(goal.z);
    const v3 dof = sphere_sample_times(rng, u.dofAmount, neg_zero);
    pos = cam + dof;
    delta_z = 1.0f / length<PM>(V(ppx, ppy, 1.0f));
    dir = normalize<PM>(goal - dof);
  } else if (u.cameraMode == 1) {
    dir = normalize<PM>(mat_rotate(u.rotation, V(0.0f, 0.0f, 1.0f)));
    pos = cam + mat_rotate(u.rotation, V((t2x - 0.5f) * u.aspect * u.fov, (t2y - 0.5f) * 1.0f * u.fov, 0.0f));
  } else if (u.cameraMode == 2) {
    const float ax = (t2x - 0.5f) * (2.0f * 3.141592f), ay = (t2y - 0.5f) * 3.141592f;
    dir = mat_rotate(u.rotation, V(PM::cos(ax) * PM::cos(ay), PM::sin(ay), PM::sin(ax) * PM::cos(ay)));
    pos = cam;
  }

  const bool staged = !PREVIEW && P.stage != nullptr;  // kernel-uniform
  float4* const stage = P.stage + (long long)sample * 3ll * P.stage_stride;  // this sample's three staged planes, tile-compact:
  const long long spix = (long long)(ly - P.ty) * (long long)P.tw + (long long)(px - P.tx);  // pixel i of the tile at [i] (stage_stride = tw * th)
#ifndef RM_DIAG_STOP
#define RM_DIAG_STOP 0  // diagnostic builds (tools/phase_cost.sh): leave the kernel after phase n, keeping its values alive
#endif
#define RM_DIAG_EXIT(n, a, b, c)                                                   \
  if (RM_DIAG_STOP == (n)) {                                                       \
    if (valid) P.color[pix] = make_float4((a), (b), (c), rng.seed);                \
    report_cost();                                                                 \
    return;                                                                        \
  }
  RM_DIAG_EXIT(1, pos.x + dir.x, pos.y + dir.y, pos.z + dir.z)  // camera block done

  if (PREVIEW) {  // :207-244
    const float steps = u.raymarchingStepCountsArray[0];
    PreviewRay ray{pos, dir, 0.0f, delta_z, 0.0f, 0.0f};
    if constexpr (BlockRepack<KIND>::value) {
      __shared__ PreviewShared<BlockShape<KIND>::waves> preview_shared;
      preview_march_block<KIND, MM>(sc, lds, u, preview_shared, steps, retire_eps, valid, ray);
    } else {
      bool done = !(0.0f < steps);
      while (ballot(!done) != 0ull) {  // a lane stops at its own settle step, the wave when all have
        if (!done) done = preview_step<KIND, MM>(sc, lds, u, steps, retire_eps, ray);
      }
    }
    pos = ray.p;
    const float steps_taken = ray.steps_taken, depth = ray.depth;
    const float4 prev_color = P.color[pix];
    const float shade = 1.0f - steps_taken / steps;
    const Surface psf = surface_at<KIND>(sc, lds, pos);
    const v3 out = (cut_color(psf.diffuse, sc.mat.diffuse_cutoff, pos) + cut_color(psf.specular, sc.mat.specular_cutoff, pos)) * shade + scene_emission(sc, pos);
    float4 col;
    if (u.blendMode == 0) {
      const float f = u.blendWithPreviousFactor;
      col = make_float4(gmix<PM>(out.x, prev_color.x, f), gmix<PM>(out.y, prev_color.y, f), gmix<PM>(out.z, prev_color.z, f),
                        gmix<PM>(1.0f, prev_color.w, f));
    } else {
      col = make_float4(prev_color.x + out.x * u.exposure, prev_color.y + out.y * u.exposure,
                        prev_color.z + out.z * u.exposure, prev_color.w + 0.0f * u.exposure);
    }
    if (u.showDofFocalPlane != 0) {  // :233-239
      const float focus = fabsf(depth - u.dofFocalPlaneDistance) / depth;
      if (focus < u.dofFocalPlaneDistance * 0.005f) col = make_float4(1.0f, gmod<PM>(col.y + 0.5f, 1.0f), gmod<PM>(col.z + 0.5f, 1.0f), 1.0f);
    }
    if (valid) P.color[pix] = col;
    report_cost();
    return;
  }

  // ---- full path trace, :246-387
  // (from here on the argument block is read through karg(): each march and each bounce's shading loads what it needs where it stands)
#if RM_KARG_FRESH
#define RM_SCENE_HERE(name) const DevScene name = karg_load(&karg()->scene)
#define RM_KARGS(name) KArg* const name = karg()
#else
#define RM_SCENE_HERE(name) const DevScene& name = P.scene
#define RM_KARGS(name) const KParams* const name = &P
#endif
  v3 albedo = V(1.0f, 1.0f, 1.0f), light = V(0.0f, 0.0f, 0.0f);
  for (float i = 0.0f;; i += 1.0f) {
    RM_KARGS(K0);
    if (!(i < K0->u.reflections)) break;
    const v3 old = pos;
#ifndef RM_CULL_ALL_BOUNCES
#define RM_CULL_ALL_BOUNCES 0  // 1 (measurement builds): the grid's lookup in every bounce
#endif
    if constexpr (KIND == RM_KIND_TABLE_SMOOTH && !RM_CULL_ALL_BOUNCES) {
      if (i == 1.0f) {  // from the second bounce on the rays of a wave are all over the scene: no common row list (eval_spheres_one_k)
        __syncthreads();
        if (threadIdx.x == 0) lds.cull_here = 0u;
        __syncthreads();
      }
    }
    {
      RM_SCENE_HERE(scm);  // the march's copy: dead when the march is
      pos = cast_ray_block<KIND, MM>(scm, lds, march_shared, pos, dir, K0->u.raymarchingStepCountsArray[(int)i], retire_eps, valid, K0->no_far_jump == 0);  // :255
    }
    RM_DIAG_EXIT(2, pos.x, pos.y, pos.z)  // + camera march
    RM_SCENE_HERE(sc);  // the shading's copy
    RM_KARGS(K);
    const float path_length = inv_exp_dist(uniform_sample(rng), K->u.fogDensity);    // :257
    light = light + albedo * scene_emission(sc, pos);                             // :261
    v3 normal = scene_normal<KIND>(sc, lds, pos, 0.00001f);                       // :264

    // :266-271 are only read by the subsurface and surface branches below: an escaped ray (most pixels of a frame are
    // sky) skips their values -- a uniform sample, a logarithm, a sphere sample, two normalisations -- and advances the
    // stream by the same seed additions
    const bool escaped = distance<PM>(old, pos) > path_length || any_nonfinite(pos);  // :278
    // the material functions at the end of the march (:266, :274-275, :286, :325, :329); an escaped ray reads none of them
    const Surface sf = (!escaped && has_surfaces<KIND>(sc)) ? surface_at<KIND>(sc, lds, pos) : scene_surface(sc);
    v3 subsurf_pos = pos;
    if (!escaped) {
      const float subsurf = -1.0f / sf.subsurface * PM::log(1.0f - uniform_sample(rng));
      v3 sdir = normalize<PM>(sphere_sample(rng));
      sdir = normalize<PM>(V(gmix<PM>(dir.x, sdir.x, 1.0f), gmix<PM>(dir.y, sdir.y, 1.0f), gmix<PM>(dir.z, sdir.z, 1.0f)));
      sdir = sdir * -gsign(dot<PM>(sdir, normal));
      subsurf_pos = pos + sdir * subsurf;
    } else {
      rng_skip_uniform(rng);
      rng_skip_sphere(rng);
    }

    const v3 prev_albedo = albedo;
    v3 diffuse_col = cut_color(sf.diffuse, sc.mat.diffuse_cutoff, pos);
    v3 specular_col = cut_color(sf.specular, sc.mat.specular_cutoff, pos);
    v3 prev_dir = dir;

    if (escaped) {  // :278-283
      pos = old + dir * gmin(path_length, 1000000.0f);
      dir = sphere_sample(rng);
      diffuse_col = V(1.0f, 1.0f, 1.0f);
      specular_col = V(1.0f, 1.0f, 1.0f);
      prev_dir = dir;
    } else if (Sdf<KIND>::template eval<NM>(sc, lds, subsurf_pos) > 0.001f) {  // :284-288
      albedo = albedo * sf.subsurface_color;
      pos = subsurf_pos;
      const v3 sp = sphere_sample(rng);
      dir = normalize<PM>(V(gmix<PM>(dir.x, sp.x, 1.0f), gmix<PM>(dir.y, sp.y, 1.0f), gmix<PM>(dir.z, sp.z, 1.0f)));
    } else {  // :290-331
      const float db = length<PM>(diffuse_col), sb = length<PM>(specular_col);
      const float prob = (db > sb) ? (1.0f - sb / db / 2.0f) : (db / sb / 2.0f);
      if (uniform_sample(rng) < prob) {  // diffuse, :300-319
        albedo = albedo * diffuse_col;
        const v3 nd = sphere_sample(rng);
        dir = nd * gsign(dot<PM>(normal, nd));
      } else {  // specular, :322-330
        const float f = gclamp(schlick(-dot<PM>(dir, normal), 1.0f, sf.ior), 0.0f, 1.0f);
        albedo = albedo * (specular_col * f);
        const v3 rv = sphere_sample(rng);
        dir = reflect<PM>(dir, normal);
        const v3 axis = normalize<PM>(cross(rv, dir));
        dir = rodrigues(dir, axis, sf.roughness * uniform_sample(rng));
      }
    }
    pos = pos + dir * 0.001f;  // :334
    RM_DIAG_EXIT(3, pos.x + normal.x + albedo.x, pos.y + normal.y + albedo.y, pos.z + normal.z + light.x)  // + shading of the bounce

    if (i == 0.0f) {  // :336-352
      // the sanitised normal is also what the light loop below sees (same variable in the GLSL)
      if (is_inf(normal.x) || is_nan(normal.x)) normal.x = 0.0f;
      if (is_inf(normal.y) || is_nan(normal.y)) normal.y = 0.0f;
      if (is_inf(normal.z) || is_nan(normal.z)) normal.z = 0.0f;
    }
    if (i == 0.0f && K->normal_dof != nullptr) {
      const float depth = gclamp(distance<PM>(pos, V(K->u.position[0], K->u.position[1], K->u.position[2])), 0.00001f, 100000000.0f);
      float dof_radius = gclamp(K->u.dofAmount * fabsf(depth - K->u.dofFocalPlaneDistance) / depth, 0.0f, 1.0f);
      if (is_inf(dof_radius) || is_nan(dof_radius)) dof_radius = 0.0f;
      if (valid && staged) {
        stage[K->stage_stride + spix] = make_float4(normal.x, normal.y, normal.z, dof_radius);
        stage[2 * K->stage_stride + spix] = make_float4(albedo.x, albedo.y, albedo.z, depth);
      } else if (valid) {
        const float4 pn = K->normal_dof[pix], pa = K->albedo_depth[pix];
        K->normal_dof[pix] = make_float4(pn.x + normal.x, pn.y + normal.y, pn.z + normal.z, pn.w + dof_radius);
        K->albedo_depth[pix] = make_float4(pa.x + albedo.x, pa.y + albedo.y, pa.z + albedo.z, pa.w + depth);
      }
    }

    // (Tried: a single-light specialisation that computes the light's term before its shadow march, so that the
    // bounce's normal and colours are dead across it: 152 instead of 224 B of spills per lane, but more HBM traffic
    // and no time gained -- the allocator moved the spills to a worse place.  Not kept.  Round 3, again on the kernel with the
    // far-field jump: Scratch_Size 188 B against 124 -- a third inlined copy of the block march costs more than the dead values save.)
    // sceneSpecularRoughness(rayPosition) of the light term (:366) is evaluated where the ray has been MOVED to (:334, or the
    // far point of an escaped ray, or the subsurface exit): with surfaces that is a lookup of its own
    const float light_rough = (K->u.lightCount > 0 && has_surfaces<KIND>(sc)) ? surface_at<KIND>(sc, lds, pos).roughness : sc.mat.roughness;
    if constexpr (ONE_LIGHT != 0) {  // :354-373 for lightCount == 1
      const v3 lp = V(K->u.lightPositions[0][0], K->u.lightPositions[0][1], K->u.lightPositions[0][2]);
      const v3 lc = V(K->u.lightColors[0][0], K->u.lightColors[0][1], K->u.lightColors[0][2]);
      const v3 adj = lp + sphere_sample_times(rng, K->u.lightSizes[0], is_neg_zero(lp.x) || is_neg_zero(lp.y) || is_neg_zero(lp.z));
      const v3 to_light = normalize<PM>(adj - pos);
      const float r = gmax(0.0f, dot<PM>(to_light, reflect<PM>(prev_dir, normal)));
      const float rough = light_rough;
      const float ndl = gmax(0.0f, dot<PM>(to_light, normal));
      const float pd = 3.14159265f * PM::pow(r * r * (rough * rough - 1.0f) + 1.0f, 2.0f);
      const v3 a = ((prev_albedo * diffuse_col) * lc) * ndl;
      v3 b = (((prev_albedo * specular_col) * lc) * rough) * rough;
      b = V(b.x / pd, b.y / pd, b.z / pd);
      const v3 contrib = a + b;
      const float start_dist = distance<PM>(pos, adj);
      RM_DIAG_EXIT(4, to_light.x + contrib.x + albedo.x, to_light.y + contrib.y + albedo.y, to_light.z + contrib.z + light.x)  // + light sample
      v3 result;
      {
        RM_SCENE_HERE(scs);
        RM_KARGS(Ks);
        result = cast_ray_block<KIND, MM>(scs, lds, march_shared, pos, to_light, Ks->u.raymarchingStepCountsArray[(int)i], retire_eps, valid, Ks->no_far_jump == 0,
                                          ExactExits<MM>::value && IsBigTable<KIND>::value ? shadow_need_exponent(start_dist, adj) : 1000);
      }
      RM_DIAG_EXIT(5, result.x + contrib.x + albedo.x, result.y + contrib.y + albedo.y, result.z + contrib.z + light.x)  // + shadow march
      if (distance<PM>(result, adj) >= start_dist) light = light + contrib;
    } else {
      for (int j = 0;; j++) {  // :354-373
        RM_KARGS(Kl);
        if (!(j < Kl->u.lightCount)) break;
        const v3 lp = V(Kl->u.lightPositions[j][0], Kl->u.lightPositions[j][1], Kl->u.lightPositions[j][2]);
        const v3 adj = lp + sphere_sample_times(rng, Kl->u.lightSizes[j], is_neg_zero(lp.x) || is_neg_zero(lp.y) || is_neg_zero(lp.z));
        const v3 to_light = normalize<PM>(adj - pos);
        RM_DIAG_EXIT(4, to_light.x + normal.x + albedo.x, to_light.y + normal.y + albedo.y, to_light.z + normal.z + light.x)  // + light sample
        const float start_dist = distance<PM>(pos, adj);
        v3 result;
        {
          RM_SCENE_HERE(scs);
          result = cast_ray_block<KIND, MM>(scs, lds, march_shared, pos, to_light, Kl->u.raymarchingStepCountsArray[(int)i], retire_eps, valid, Kl->no_far_jump == 0,
                                            ExactExits<MM>::value && IsBigTable<KIND>::value ? shadow_need_exponent(start_dist, adj) : 1000);
        }
        RM_DIAG_EXIT(5, result.x + normal.x + albedo.x, result.y + normal.y + albedo.y, result.z + normal.z + light.x)  // + shadow march
        if (distance<PM>(result, adj) >= start_dist) {
          RM_KARGS(Kc);
          const v3 lc = V(Kc->u.lightColors[j][0], Kc->u.lightColors[j][1], Kc->u.lightColors[j][2]);
          const float r = gmax(0.0f, dot<PM>(to_light, reflect<PM>(prev_dir, normal)));
          const float rough = light_rough;
          const float ndl = gmax(0.0f, dot<PM>(to_light, normal));
          const float pd = 3.14159265f * PM::pow(r * r * (rough * rough - 1.0f) + 1.0f, 2.0f);
          const v3 a = ((prev_albedo * diffuse_col) * lc) * ndl;
          v3 b = (((prev_albedo * specular_col) * lc) * rough) * rough;
          b = V(b.x / pd, b.y / pd, b.z / pd);
          light = light + (a + b);
        }
      }
    }
    if constexpr (ONE_LIGHT == 2) break;  // the only bounce
  }

  RM_KARGS(Ke);
  const float exposure = Ke->u.exposure;
  if (staged) {  // the blend (:379-387) happens in rm_combine_kernel
    if (valid) stage[spix] = make_float4(light.x * exposure, light.y * exposure, light.z * exposure, 0.0f);
    report_cost();
    return;
  }
  // :379-387
  const float4 prev_color = Ke->color[pix];
  float4 col;
  if (Ke->u.blendMode == 0) {
    const float f = Ke->u.blendWithPreviousFactor;
    col = make_float4(gmix<PM>(light.x * exposure, prev_color.x, f), gmix<PM>(light.y * exposure, prev_color.y, f),
                      gmix<PM>(light.z * exposure, prev_color.z, f), gmix<PM>(1.0f, prev_color.w, f));
  } else {
    col = make_float4(light.x * exposure + prev_color.x, light.y * exposure + prev_color.y,
                      light.z * exposure + prev_color.z, 1.0f + prev_color.w);
  }
  if (valid) Ke->color[pix] = col;
#undef RM_SCENE_HERE
#undef RM_KARGS
#ifdef RM_DIAG_TIMELINE
  if (threadIdx.x == 0 && valid) {
    const unsigned long long tl_end = __builtin_amdgcn_s_memrealtime();
    unsigned int hw_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    unsigned int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    P.color[pix] = make_float4(__uint_as_float((unsigned int)tl_start), __uint_as_float((unsigned int)tl_end), __uint_as_float(hw_id), __uint_as_float(xcc));
  }
#endif
  report_cost();
}

// ---- probes: the building blocks on caller-supplied inputs ---------------------

template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void rm_probe_kernel(const ProbeParams P) {
  using MM = typename std::conditional<FAST, FM, PM>::type;
  __shared__ SceneLds lds;
  enter_math_mode<KIND, FAST>();
  Sdf<KIND>::stage(P.scene, lds);
  __syncthreads();
  const int gi = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gi < P.n ? gi : P.n - 1;  // keep whole waves alive for the ballots
  const DevScene& sc = P.scene;
  if (P.what == RM_PROBE_SDF) {
    const float d = Sdf<KIND>::template eval<MM>(sc, lds, V(P.in[3 * i], P.in[3 * i + 1], P.in[3 * i + 2]));
    if (gi < P.n) P.out[i] = d;
  } else if (P.what == RM_PROBE_CAST_RAY) {
    const v3 r = cast_ray<KIND, MM>(sc, lds, V(P.in[6 * i], P.in[6 * i + 1], P.in[6 * i + 2]),
                                V(P.in[6 * i + 3], P.in[6 * i + 4], P.in[6 * i + 5]), P.param, P.retire_eps, P.no_far_jump == 0);
    if (gi < P.n) { P.out[3 * i] = r.x; P.out[3 * i + 1] = r.y; P.out[3 * i + 2] = r.z; }
  } else if (P.what == RM_PROBE_CAST_SHADOW) {  // a light's shadow test (:362-363) on a caller's ray: 1 = the light is seen from pos
    const v3 pos = V(P.in[9 * i], P.in[9 * i + 1], P.in[9 * i + 2]), dir = V(P.in[9 * i + 3], P.in[9 * i + 4], P.in[9 * i + 5]);
    const v3 adj = V(P.in[9 * i + 6], P.in[9 * i + 7], P.in[9 * i + 8]);
    const float start_dist = distance<PM>(pos, adj);
    const v3 r = cast_ray<KIND, MM>(sc, lds, pos, dir, P.param, P.retire_eps, P.no_far_jump == 0,
                                    ExactExits<MM>::value && IsBigTable<KIND>::value ? shadow_need_exponent(start_dist, adj) : 1000);
    if (gi < P.n) P.out[i] = distance<PM>(r, adj) >= start_dist ? 1.0f : 0.0f;
  } else if (P.what == RM_PROBE_CAST_STEPS) {
    v3 p = V(P.in[6 * i], P.in[6 * i + 1], P.in[6 * i + 2]);
    const v3 dir = V(P.in[6 * i + 3], P.in[6 * i + 4], P.in[6 * i + 5]);
    float settled = P.param;
    for (float s = 0.0f; s < P.param; s += 1.0f) {
      const float d = march_sdf<KIND, MM>(sc, lds, p);
      const v3 q = p + dir * d;
      if (same_bits(p, q) || (P.retire_eps > 0.0f && fabsf(d) <= P.retire_eps * gmax(1.0f, gmax(fabsf(q.x), gmax(fabsf(q.y), fabsf(q.z)))))) { settled = s; break; }
      p = q;
    }
    if (gi < P.n) P.out[i] = settled;
  } else if (P.what == RM_PROBE_NORMAL) {
    const v3 r = scene_normal<KIND>(sc, lds, V(P.in[3 * i], P.in[3 * i + 1], P.in[3 * i + 2]), P.param);
    if (gi < P.n) { P.out[3 * i] = r.x; P.out[3 * i + 1] = r.y; P.out[3 * i + 2] = r.z; }
  } else {
    const v3 q = V(P.in[3 * i], P.in[3 * i + 1], P.in[3 * i + 2]);
    const Surface qs = surface_at<KIND>(sc, lds, q);
    const v3 d = cut_color(qs.diffuse, sc.mat.diffuse_cutoff, q), s = cut_color(qs.specular, sc.mat.specular_cutoff, q), e = scene_emission(sc, q);
    if (gi < P.n) {
      float* o = P.out + 12 * i;
      o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = s.x; o[4] = s.y; o[5] = s.z; o[6] = e.x; o[7] = e.y; o[8] = e.z;
      o[9] = qs.roughness; o[10] = qs.subsurface; o[11] = qs.ior;
    }
  }
}

#if !RM_BUILD_FAST
// rm_probe_math: the transcendental functions of this unit's arithmetic on arrays (PM: rm_pm_math.hpp, or the GL stack's
// rm_ss_math.hpp), as the kernels call them -- pow_pair / sincos are the shared forms the Mandelbulb uses.  fn: hip_raymarch.h.
__global__ __launch_bounds__(256) void rm_math_probe_kernel(int fn, const float* a, const float* b, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b ? b[i] : 0.0f;
  float r = 0.0f, other = 0.0f;
  switch (fn) {
    case 0: r = PM::sin(x); break;
    case 1: r = PM::cos(x); break;
    case 2: r = PM::log(x); break;
    case 3: r = PM::exp(x); break;
    case 4: r = PM::pow(x, y); break;
    case 5: r = PM::acos(x); break;
    case 6: r = PM::atan2(x, y); break;
    case 7: r = rm_tan(x); break;
    case 8: PM::pow_pair(x, y, r, other); break;
    case 9: PM::pow_pair(x, y, other, r); break;
    case 10: PM::sincos(x, r, other); break;
    case 11: PM::sincos(x, other, r); break;
    case 12: r = PM::sqrt(x); break;
    case 13: r = PM::div(x, y); break;
    default: break;
  }
  out[i] = r;
}
#endif

#if !RM_BUILD_FAST
// camera block with randomDirectionOffset = dofOffset = 0; what = 1: first `count` uniformSample() values
__global__ __launch_bounds__(256) void rm_camera_rng_kernel(const RmUniforms u, int W, int H, int what, int count, float* out) {
  const int gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= W * H) return;
  const int x = gi % W, y = gi / W;
  const float tcx = ((float)x + 0.5f) / (float)W, tcy = ((float)y + 0.5f) / (float)H;
  if (what == 1) {
    Rng rng = rng_init(tcx, tcy, u.randNoise[0], u.randNoise[1]);
    for (int k = 0; k < count; k++) out[(size_t)gi * count + k] = uniform_sample(rng);
    return;
  }
  v3 dir = V(0.0f, 0.0f, 0.0f), pos = V(0.0f, 0.0f, 0.0f);
  const v3 cam = V(u.position[0], u.position[1], u.position[2]);
  float delta_z = 1.0f;
  if (u.cameraMode == 0) {
    const float th = rm_tan(u.fov / 2.0f);
    const float ppx = (tcx * 2.0f - 1.0f) * u.aspect * th;
    const float ppy = (tcy * 2.0f - 1.0f) * 1.0f * th;
    const v3 goal = mat_rotate(u.rotation, V(ppx, ppy, 1.0f)) * u.dofFocalPlaneDistance;
    delta_z = 1.0f / length<PM>(V(ppx, ppy, 1.0f));
    dir = normalize<PM>(goal);
    pos = cam;
  } else if (u.cameraMode == 1) {
    dir = normalize<PM>(mat_rotate(u.rotation, V(0.0f, 0.0f, 1.0f)));
    pos = cam + mat_rotate(u.rotation, V((tcx - 0.5f) * u.aspect * u.fov, (tcy - 0.5f) * 1.0f * u.fov, 0.0f));
  } else if (u.cameraMode == 2) {
    const float ax = (tcx - 0.5f) * (2.0f * 3.141592f), ay = (tcy - 0.5f) * 3.141592f;
    dir = mat_rotate(u.rotation, V(PM::cos(ax) * PM::cos(ay), PM::sin(ay), PM::sin(ax) * PM::cos(ay)));
    pos = cam;
  }
  float* o = out + (size_t)gi * 8;
  o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = delta_z;
  o[4] = dir.x; o[5] = dir.y; o[6] = dir.z; o[7] = 0.0f;
}

#endif

// ---- launchers (called from rm_api.hip) ---------------------------------------
#ifndef RM_ONLY_KERNELS  // (tools/one_kernel.hip: a TU that instantiates single kernels for a look at their code)

#if RM_BUILD_FAST
#define RM_LAUNCH(name) name##_fast
#else
#define RM_LAUNCH(name) name##_strict
#endif
static constexpr bool kFast = RM_BUILD_FAST != 0;
static constexpr bool kVariants = !RM_GL_STACK;  // the job-shape variants of the pixel kernel (ONE_LIGHT): both builds since round 4

// the pixel tile of a workgroup for this job, and whether an 8-wave workgroup lies on its side (BlockShape)
// log2 of the waves across the tile, + 1 (KParams::tile_wide; 0 = the kind's own shape)
template <int KIND>
static int tile_is_wide(const KParams& P) {
  using Shape = BlockShape<KIND>;
  if (!Shape::can_lie) return 0;
#ifdef RM_TILE_EXPERIMENT
  if (const char* v = std::getenv("RM_TILE_LG")) return std::atoi(v) + 1;
#endif
  const long long upright = (long long)((P.tw + Shape::px - 1) / Shape::px) * ((P.th + Shape::py - 1) / Shape::py);
  const long long side = (long long)((P.tw + Shape::py - 1) / Shape::py) * ((P.th + Shape::px - 1) / Shape::px);
  return side * 100 <= upright * 97 ? 3 : 0;
}

template <int KIND>
static void grid_kind(const KParams& P, int* gx, int* gy) {
  using Shape = BlockShape<KIND>;
  const int w = tile_is_wide<KIND>(P);
  const int px = w ? 8 << (w - 1) : Shape::px, py = w ? (Shape::waves >> (w - 1)) * 8 : Shape::py;
  *gx = (P.tw + px - 1) / px;
  *gy = (P.th + py - 1) / py;
}

template <int KIND>
static hipError_t launch_kind(const KParams& P0, bool preview, hipStream_t stream) {
  using Shape = BlockShape<KIND>;
  KParams P = P0;
  P.tile_wide = tile_is_wide<KIND>(P0);
  int gx = 0, gy = 0;
  grid_kind<KIND>(P0, &gx, &gy);
  const int per_tile = !preview && P.batch > 1 ? P.batch : 1;  // workgroups per tile (KParams::batch)
  const dim3 grid(gx, gy * per_tile), block(Shape::threads);
  const bool eps = kFast && P.retire_eps > 0.0f;
  if (preview && eps) hipLaunchKernelGGL((rm_pixel_kernel<KIND, true, kFast, kFast>), grid, block, 0, stream, P);
  else if (preview) hipLaunchKernelGGL((rm_pixel_kernel<KIND, true, kFast, false>), grid, block, 0, stream, P);
  else if (eps) hipLaunchKernelGGL((rm_pixel_kernel<KIND, false, kFast, kFast>), grid, block, 0, stream, P);
  else if (kVariants && P.u.lightCount == 1 && P.u.reflections > 0.0f && P.u.reflections <= 1.0f)
    hipLaunchKernelGGL((rm_pixel_kernel<KIND, false, kFast, false, kVariants ? 2 : 0>), grid, block, 0, stream, P);
  else if (kVariants && P.u.lightCount == 1) hipLaunchKernelGGL((rm_pixel_kernel<KIND, false, kFast, false, kVariants ? 1 : 0>), grid, block, 0, stream, P);
  else hipLaunchKernelGGL((rm_pixel_kernel<KIND, false, kFast, false>), grid, block, 0, stream, P);
  return hipGetLastError();
}

hipError_t RM_LAUNCH(launch_pixels)(const KParams& P, hipStream_t stream) {
  const bool preview = P.u.renderMode == 1;
  switch (P.scene.kind) {
    case RM_SCENE_TABLE:
      if (P.scene.table_flags & RM_TABLE_HAS_KIND) return launch_kind<RM_KIND_TABLE_KINDS>(P, preview, stream);
#if RM_BUILD_FAST
      if (rm_table_big(P) && (P.scene.table_flags & (RM_TABLE_UNIFORM_K | RM_TABLE_HAS_SURFACES)) == RM_TABLE_UNIFORM_K) return launch_kind<RM_KIND_TABLE_SMOOTH>(P, preview, stream);
#endif
      return rm_table_big(P) ? launch_kind<RM_KIND_TABLE_BIG>(P, preview, stream) : launch_kind<RM_SCENE_TABLE>(P, preview, stream);
    case RM_SCENE_MANDELBULB:
#if RM_BUILD_FAST
      if (P.scene.p[RM_P_BULB_POWER] == 8.0f && (int)P.scene.p[RM_P_BULB_ITERATIONS] == 8) return launch_kind<RM_KIND_BULB8>(P, preview, stream);
#endif
      return launch_kind<RM_SCENE_MANDELBULB>(P, preview, stream);
    case RM_SCENE_SPHERE_GRID: return launch_kind<RM_SCENE_SPHERE_GRID>(P, preview, stream);
    case RM_SCENE_SPHERE_LATTICE: return launch_kind<RM_SCENE_SPHERE_LATTICE>(P, preview, stream);
    case RM_SCENE_MENGER: return launch_kind<RM_SCENE_MENGER>(P, preview, stream);
    case RM_SCENE_KIFS_TREE: return launch_kind<RM_SCENE_KIFS_TREE>(P, preview, stream);
    case RM_SCENE_KIFS_BOX: return launch_kind<RM_SCENE_KIFS_BOX>(P, preview, stream);
    default: return hipErrorInvalidValue;
  }
}

#if !RM_BUILD_FAST  // not templates: once, in the parity TU
void pixel_grid(const KParams& P, int* gx, int* gy) {
  switch (P.scene.kind) {
    case RM_SCENE_TABLE: if (rm_table_big(P)) grid_kind<RM_KIND_TABLE_BIG>(P, gx, gy); else grid_kind<RM_SCENE_TABLE>(P, gx, gy); break;
    case RM_SCENE_MANDELBULB: grid_kind<RM_SCENE_MANDELBULB>(P, gx, gy); break;
    case RM_SCENE_SPHERE_GRID: grid_kind<RM_SCENE_SPHERE_GRID>(P, gx, gy); break;
    case RM_SCENE_SPHERE_LATTICE: grid_kind<RM_SCENE_SPHERE_LATTICE>(P, gx, gy); break;
    case RM_SCENE_MENGER: grid_kind<RM_SCENE_MENGER>(P, gx, gy); break;
    case RM_SCENE_KIFS_TREE: grid_kind<RM_SCENE_KIFS_TREE>(P, gx, gy); break;
    case RM_SCENE_KIFS_BOX: grid_kind<RM_SCENE_KIFS_BOX>(P, gx, gy); break;
    default: *gx = *gy = 0;
  }
}

// The order of the next launch from the costs of the last one: tiles by decreasing cost, to the resolution of 64
// buckets (eighths of an octave), which is all longest-processing-time-first scheduling needs; within a bucket by tile
// index (a stable counting sort: the same order on every run).  Clears the costs for the next launch.
// Round 5: any number of workgroups (rounds 1-4: ONE workgroup of 1 024 threads walked all the tiles -- 0.05 ms on the headline
// frame, 2.6 ms on average and 19 ms at worst on C5's 131 072 tiles).  A workgroup owns RM_ORDER_CHUNK consecutive tiles:
//   rm_order_hist_kernel     its histogram over the buckets -> scratch[workgroup][64]
//   rm_order_scatter_kernel  where its tiles of bucket b start = the tiles of lower buckets anywhere + the tiles of bucket b
//                            in earlier workgroups; inside the workgroup thread t owns 16 consecutive tiles and places them
//                            after those of the threads before it (a per-bucket prefix over the threads, in LDS).
#define RM_ORDER_THREADS 256
#define RM_ORDER_PER_THREAD 16
#define RM_ORDER_CHUNK (RM_ORDER_THREADS * RM_ORDER_PER_THREAD)
RM_DEV int order_bucket(unsigned int c) {
  const int b = (int)(8.0f * (log2f((float)c + 1.0f) - 6.0f));
  return 63 - (b < 0 ? 0 : b > 63 ? 63 : b);  // most expensive first
}
__global__ __launch_bounds__(RM_ORDER_THREADS) void rm_order_hist_kernel(const unsigned int* cost, unsigned int* scratch, int n) {
  __shared__ unsigned int hist[64];
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * RM_ORDER_CHUNK;
  for (int j = 0; j < RM_ORDER_PER_THREAD; j++) {
    const int i = base + j * RM_ORDER_THREADS + (int)threadIdx.x;
    if (i < n) atomicAdd(&hist[order_bucket(cost[i])], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 64) scratch[blockIdx.x * 64 + threadIdx.x] = hist[threadIdx.x];
}
__global__ __launch_bounds__(RM_ORDER_THREADS) void rm_order_scatter_kernel(unsigned int* cost, unsigned int* order, const unsigned int* scratch, int n) {
  __shared__ unsigned short off[RM_ORDER_THREADS][66];  // off[t][b]: tiles of bucket b owned by the threads before t (after the prefix)
  __shared__ unsigned int part[4][64][2], start[64];
  const int tid = threadIdx.x, b = tid & 63, q = tid >> 6, groups = gridDim.x, me = blockIdx.x;
  // the tiles of bucket b in all workgroups, and in the workgroups before this one
  unsigned int all = 0, before = 0;
  for (int g = q; g < groups; g += 4) {
    const unsigned int h = scratch[g * 64 + b];
    all += h;
    before += g < me ? h : 0u;
  }
  part[q][b][0] = all;
  part[q][b][1] = before;
  for (int k = 0; k < 64; k += 4) off[tid][k + 0] = off[tid][k + 1] = off[tid][k + 2] = off[tid][k + 3] = 0;
  __syncthreads();
  if (tid < 64) start[tid] = part[0][tid][0] + part[1][tid][0] + part[2][tid][0] + part[3][tid][0];
  __syncthreads();
  if (tid == 0) {  // exclusive scan over the 64 buckets
    unsigned int s = 0;
    for (int k = 0; k < 64; k++) { const unsigned int c = start[k]; start[k] = s; s += c; }
  }
  __syncthreads();
  if (tid < 64) start[tid] += part[0][tid][1] + part[1][tid][1] + part[2][tid][1] + part[3][tid][1];
  // this thread's tiles and their buckets
  const int first = me * RM_ORDER_CHUNK + tid * RM_ORDER_PER_THREAD;
  unsigned char mine[RM_ORDER_PER_THREAD];
#pragma unroll
  for (int j = 0; j < RM_ORDER_PER_THREAD; j++) {
    const int i = first + j;
    mine[j] = i < n ? (unsigned char)order_bucket(cost[i]) : (unsigned char)255;
    if (i < n) off[tid][mine[j]]++;
  }
  __syncthreads();
  {  // prefix over the threads, bucket by bucket: thread (b, q) walks its quarter of the threads, then the quarters are chained
    unsigned int s = 0;
    for (int t = q * 64; t < q * 64 + 64; t++) { const unsigned int c = off[t][b]; off[t][b] = (unsigned short)s; s += c; }
    part[q][b][0] = s;
  }
  __syncthreads();
  {
    unsigned int add = 0;
    for (int k = 0; k < q; k++) add += part[k][b][0];
    if (add != 0u)
      for (int t = q * 64; t < q * 64 + 64; t++) off[t][b] = (unsigned short)(off[t][b] + add);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RM_ORDER_PER_THREAD; j++) {
    const int i = first + j;
    if (i < n) {
      const int k = mine[j];
      order[start[k] + off[tid][k]++] = (unsigned int)i;
      cost[i] = 0;
    }
  }
}

hipError_t launch_order(unsigned int* cost, unsigned int* order, unsigned int* scratch, int n, hipStream_t stream) {
  const int groups = (n + RM_ORDER_CHUNK - 1) / RM_ORDER_CHUNK;
  if (groups <= 0) return hipSuccess;
  hipLaunchKernelGGL(rm_order_hist_kernel, dim3(groups), dim3(RM_ORDER_THREADS), 0, stream, cost, scratch, n);
  hipLaunchKernelGGL(rm_order_scatter_kernel, dim3(groups), dim3(RM_ORDER_THREADS), 0, stream, cost, order, scratch, n);
  return hipGetLastError();
}

// ---- the culling grid of a primitive table (rm_params.hpp CullGrid; built once per scene, in double precision) ------------
// One thread per cell, centre c, half-diagonal R.  Every shape's distance is 1-Lipschitz, so over the cell row i's term lies in
// [d_i(c) - R, d_i(c) + R], and interval arithmetic on the fold gives bounds [L, U] of its running value before every row.  A row
// is dropped for the cell when its operator cannot change any value the fold can have there:
//    union         min(d, di):            di >= d          <=  lo_i >= U
//    smooth union  d + g (...), g = 0:    di >= d + k      <=  lo_i >= U + k        (smooth_row: exact at that clamp)
//    subtract      max(d, -di):           -di <= d         <=  -lo_i <= L
//    intersect     max(d, di):            di <= d          <=  hi_i <= L
// For the two unions there is a second, sharper test against ONE earlier row j (the nearest so far at c, with only unions between
// it and row i, so that the running value is <= d_j): the difference d_i - d_j has the gradient u_i - u_j of two unit vectors
// pointing at p from a point of either shape, |u_i - u_j| <= |x_i - x_j| / sqrt(|p - x_i| |p - x_j|) -- a sphere's centre, the
// nearest point of a box (then the cell has to lie outside it) -- so far away from the scene, where
// every term changes at rate 1 but their differences hardly at all, large cells still separate the rows:
//    di - d_j >= k  everywhere in the cell   <=   d_i(c) - d_j(c) - R * Lip_ij >= k.
// Every test carries a margin for what fp32 makes of the terms and of the running value (n + 8 roundings at the magnitude of
// the level's coordinates), and R is inflated for points the kernel's own index arithmetic puts into a neighbouring cell.  The
// first row starts the fold and always stays.
__global__ __launch_bounds__(256) void rm_cull_build_kernel(const CullBuild B) {
  __shared__ CullRow rows[RM_MAX_PRIMS];  // the table as the rule reads it, once per workgroup (22 KB at 256 rows)
  for (int i = threadIdx.x; i < B.nprims; i += blockDim.x) rows[i] = rm_cull_row(B.prims[i]);
  __syncthreads();
  const long long level0 = (long long)B.n * B.n * B.n, per_outer = (long long)B.n_outer * B.n_outer * B.n_outer;
  const long long all = rm_cull_cells(B.n, B.n_outer, B.levels), cell_id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell_id > all) return;
  unsigned long long* out = B.cells + cell_id * B.words;
  if (cell_id == all) {  // the cell of the points outside every level
    for (int w = 0; w < B.words; w++) out[w] = 0ull;
    for (int i = 0; i < B.nprims; i++) out[i >> 6] |= 1ull << (i & 63);
    return;
  }
  const int level = cell_id < level0 ? 0 : 1 + (int)((cell_id - level0) / per_outer);
  const int in_level = (int)(level == 0 ? cell_id : (cell_id - level0) % per_outer), n = level == 0 ? B.n : B.n_outer;
  const int ix = in_level % n, iy = (in_level / n) % n, iz = in_level / (n * n);
  const double half = ldexp(B.half0, level), cell = 2.0 * half / n;
  const double c[3] = {B.centre[0] - half + (ix + 0.5) * cell, B.centre[1] - half + (iy + 0.5) * cell, B.centre[2] - half + (iz + 0.5) * cell};
  const double magnitude = 1.7320508 * half + B.reach;
  rm_cull_cell_rows(rows, B.nprims, B.words, c, 0.8660254 * cell * 1.002 + 4e-7 * magnitude, rm_cull_margin(B.nprims, magnitude), out);
}

hipError_t launch_cull_build(const CullBuild& B, hipStream_t stream) {
  const long long cells = rm_cull_cells(B.n, B.n_outer, B.levels) + 1;
  hipLaunchKernelGGL(rm_cull_build_kernel, dim3((unsigned int)((cells + 255) / 256)), dim3(256), 0, stream, B);
  return hipGetLastError();
}
#endif

// The kind a kernel that evaluates the scene at points of its own runs as, stated once: the probe's, and so that of the mesh passes
// (rm_mesh_kernels.inc), whose distances have to be the probe's at the same point.  `launch` is a generic lambda that starts its kernel for
// the kind it is handed as a PointKind<K>.  (launch_pixels selects otherwise: RM_KIND_TABLE_SMOOTH, RM_KIND_BULB8 and the preview are its own.)
template <int K>
using PointKind = std::integral_constant<int, K>;
template <class Launch>
static hipError_t launch_point_kind(const DevScene& scene, Launch&& launch) {
  const bool table = scene.kind == RM_SCENE_TABLE;
  if (table && (scene.table_flags & RM_TABLE_HAS_KIND)) launch(PointKind<RM_KIND_TABLE_KINDS>{});
  else if (table && scene.nprims >= RM_TABLE_BIG_ROWS) launch(PointKind<RM_KIND_TABLE_BIG>{});  // the march of the long tables' pixel kernels (their finer far-field exits)
  else switch (scene.kind) {
    case RM_SCENE_TABLE: launch(PointKind<RM_SCENE_TABLE>{}); break;
    case RM_SCENE_MANDELBULB: launch(PointKind<RM_SCENE_MANDELBULB>{}); break;
    case RM_SCENE_SPHERE_GRID: launch(PointKind<RM_SCENE_SPHERE_GRID>{}); break;
    case RM_SCENE_SPHERE_LATTICE: launch(PointKind<RM_SCENE_SPHERE_LATTICE>{}); break;
    case RM_SCENE_MENGER: launch(PointKind<RM_SCENE_MENGER>{}); break;
    case RM_SCENE_KIFS_TREE: launch(PointKind<RM_SCENE_KIFS_TREE>{}); break;
    case RM_SCENE_KIFS_BOX: launch(PointKind<RM_SCENE_KIFS_BOX>{}); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t RM_LAUNCH(launch_probe)(const ProbeParams& P, hipStream_t stream) {
  const dim3 grid((P.n + 255) / 256);
  return launch_point_kind(P.scene, [&](auto kind) { hipLaunchKernelGGL((rm_probe_kernel<decltype(kind)::value, kFast>), grid, dim3(256), 0, stream, P); });
}

#if !RM_BUILD_FAST
hipError_t launch_math_probe(int fn, const float* a, const float* b, int n, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(rm_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, a, b, n, out);
  return hipGetLastError();
}
#endif

#if !RM_BUILD_FAST
hipError_t launch_camera_rng(const RmUniforms& u, int W, int H, int what, int count, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(rm_camera_rng_kernel, dim3((W * H + 255) / 256), dim3(256), 0, stream, u, W, H, what, count, out);
  return hipGetLastError();
}
#endif

#endif  // RM_ONLY_KERNELS

}  // namespace rm
