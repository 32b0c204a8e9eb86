// rm_wavefront_host.inc -- host side of the wavefront pipeline (rm_wavefront.inc): its workspace, its tuning and its launches.
// Included by rm_api.hip in the tests' CROSS-CHECK build only (-DRM_WITH_WAVEFRONT=1, build.py build_crosscheck).
#define RM_MAX_MARCHES (RM_MAX_BOUNCES * (1 + RM_MAX_LIGHTS))
#define RM_COUNTERS_PER_MARCH 8  // queue heads and parked counts of the launches of one march
#define RM_WF_STREAMS 4
#define RM_WF_MAX_BANDS 8

// a tuning knob from the environment: the integer in `name` when it lies in lo..hi, else the default
static int env_int(const char* name, int lo, int hi, int dflt) {
  const char* v = std::getenv(name);
  const int n = v ? std::atoi(v) : dflt;
  return n >= lo && n <= hi ? n : dflt;
}

struct WavefrontHost {
  int cu_count = 256;  // (the device's, once the first launch has asked)
  // persistent-grid sizes in workgroups per CU, from a sweep on the headline frame (tools/sweep.sh, DESIGN.md):
  // the Mandelbulb passes want FEW waves (every wave ends in a tail of a few long rays), the table march wants all slots
  int pass2_blocks_per_cu = env_int("RM_PASS2_BLOCKS_PER_CU", 1, 8, 2);
  int pass1_blocks_per_cu = env_int("RM_PASS1_BLOCKS_PER_CU", 1, 8, 2);
  int pass2_rounds = env_int("RM_PASS2_ROUNDS", 1, 3, 1);  // launches over the parked rays (the last one runs every ray to its end); >1 measured slower (DESIGN.md)
  int repark = env_int("RM_REPARK", 0, 63, 24);  // a drained pass-2 wave with this many active lanes or fewer hands them to the next round
  // workspace (per-ray state + queue heads), grown on demand
  float4* ws = nullptr;
  size_t ws_rays = 0;
  unsigned int* heads = nullptr;  // 3 counters per march launch: head(pass 0/1), head(pass 2), parked count
  unsigned int* ws_list = nullptr;  // parked ray ids (two lists, ping-pong between pass-2 rounds)
  unsigned int* ws_list2 = nullptr;
  unsigned long long* stats = nullptr;  // 16 counters, filled by RM_WF_STATS builds only
  hipStream_t wf_stream[RM_WF_STREAMS] = {nullptr, nullptr, nullptr, nullptr};  // side streams of the banded pipeline
  hipEvent_t wf_join[RM_WF_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t wf_fork = nullptr;
  int wf_bands = env_int("RM_WF_BANDS", 1, 8, 0);  // bands of rows in flight on side streams; 0 = automatic (2 for large tiles: measured best)
  int wf_blocks_per_cu = env_int("RM_WF_BLOCKS_PER_CU", 1, 8, 8);
  int claims_per_wave = env_int("RM_WF_CLAIMS", 1, 64, 8);

  // (the caller has synchronised the context's stream)
  void destroy() {
    if (ws) (void)hipFree(ws);
    if (heads) (void)hipFree(heads);
    if (ws_list) (void)hipFree(ws_list);
    if (ws_list2) (void)hipFree(ws_list2);
    if (stats) (void)hipFree(stats);
    for (int s = 0; s < RM_WF_STREAMS; s++) {
      if (wf_stream[s]) { (void)hipStreamSynchronize(wf_stream[s]); (void)hipStreamDestroy(wf_stream[s]); }
      if (wf_join[s]) (void)hipEventDestroy(wf_join[s]);
    }
    if (wf_fork) (void)hipEventDestroy(wf_fork);
  }
};

// One band of rows through the wavefront pipeline (rm_wavefront.inc) on `stream`.
static hipError_t launch_wavefront_band(const WavefrontHost& wf, const KParams& P, int flags, hipStream_t stream, float4* ws,
                                        unsigned int* list, unsigned int* list2, unsigned int* heads) {
  const bool fast = (flags & RM_RENDER_FAST) != 0;
  rm::WfParams W{};
  W.k = P;
  W.tiles_x = (P.tw + 7) / 8;
  const int tiles_y = (P.th + 7) / 8;
  W.n_rays = W.tiles_x * tiles_y * 64;
  for (int i = 0; i < rm::WF_ARRAYS; i++) W.a[i] = ws + (size_t)i * (size_t)W.n_rays;
  W.stats = wf.stats;
  hipError_t e;
  const bool classes = rm::wf_kind_has_cost_classes(P.scene.kind) && !(flags & RM_RENDER_NO_COST_CLASSES);
  // persistent march grid: every SIMD slot of the chip, or fewer when there are few rays
  int blocks = wf.cu_count * wf.wf_blocks_per_cu;
  const int needed = (W.n_rays + 255) / 256;
  if (blocks > needed) blocks = needed;
  int march = 0;
  auto do_march = [&](int pos_array, int dir_array, bool preview) -> hipError_t {
    W.pos_array = pos_array;
    W.dir_array = dir_array;
    unsigned int* c = heads + RM_COUNTERS_PER_MARCH * march++;  // [0] head of pass 0/1, [1] parked by pass 1, [2..] heads/counts of the pass-2 rounds
    auto go = [&](int pass) { return fast ? rm::wf_launch_march_fast(W, preview, pass, blocks, stream) : rm::wf_launch_march_strict(W, preview, pass, blocks, stream); };
    W.head = c;
    W.claims_per_wave = wf.claims_per_wave;
    W.repark = 0;
    W.list_in = nullptr;
    W.list_in_count = nullptr;
    W.list_out = list;
    W.list_out_count = c + 1;
    if (!classes) return go(0);
    const int saved = blocks;
    const int pass1 = wf.cu_count * wf.pass1_blocks_per_cu;
    if (blocks > pass1) blocks = pass1;
    hipError_t e1 = go(1);  // cheap evaluations; parks the rays that need the deep one
    blocks = saved;
    if (e1 != hipSuccess) return e1;
    // The parked rays, compacted, in up to three rounds.  Fewer waves than SIMD slots on purpose (2 per SIMD keep the VALU of this
    // dependent-chain code busy), and a round whose queue has drained does not let its waves thin out to a few never-settling rays
    // each: a wave with <= repark active lanes parks them again and the next, smaller round re-compacts the survivors.
    unsigned int* in = list;
    unsigned int* outl = list2;
    unsigned int* in_count = c + 1;
    int round_blocks = wf.cu_count * wf.pass2_blocks_per_cu;
    for (int round = 0; round < wf.pass2_rounds; round++) {
      const bool last = round == wf.pass2_rounds - 1;
      W.head = c + 2 + 2 * round;
      W.list_in = in;
      W.list_in_count = in_count;
      W.list_out = outl;
      W.list_out_count = c + 3 + 2 * round;
      W.repark = last ? 0 : wf.repark;
      blocks = round_blocks < saved ? round_blocks : saved;
      hipError_t e2 = go(2);
      if (e2 != hipSuccess) { blocks = saved; return e2; }
      in_count = W.list_out_count;
      unsigned int* t = in; in = outl; outl = t;
      round_blocks = round_blocks / 4 > wf.cu_count / 4 ? round_blocks / 4 : wf.cu_count / 4;
    }
    blocks = saved;
    return hipSuccess;
  };
  if ((e = rm::wf_launch_stage(W, 0, stream)) != hipSuccess) return e;  // setup
  if (P.u.renderMode == 1) {
    if ((e = do_march(rm::WF_POS, rm::WF_DIR, true)) != hipSuccess) return e;
    return rm::wf_launch_stage(W, 1, stream);
  }
  int bounces = 0;
  for (float i = 0.0f; i < P.u.reflections; i += 1.0f) bounces++;
  if (bounces == 0) return rm::wf_launch_stage(W, 2, stream);
  for (int b = 0; b < bounces; b++) {
    W.bounce = b;
    W.last_bounce = b == bounces - 1;
    if ((e = do_march(rm::WF_POS, rm::WF_DIR, false)) != hipSuccess) return e;
    if ((e = fast ? rm::wf_launch_shade_fast(W, stream) : rm::wf_launch_shade_strict(W, stream)) != hipSuccess) return e;
    for (int j = 0; j < P.u.lightCount; j++) {
      W.light = j;
      if ((e = do_march(rm::WF_SPOS, rm::WF_SDIR, false)) != hipSuccess) return e;
      if ((e = rm::wf_launch_stage(W, 3, stream)) != hipSuccess) return e;  // light
    }
  }
  return hipSuccess;
}

// One sample through the wavefront pipeline, on `stream` (the context's).  A large tile is cut into bands of rows that go down the
// pipeline on RM_WF_STREAMS side streams: every kernel of the pipeline ends with a tail in which the chip drains (a few long rays, the
// last workgroups), and the next band's kernels fill those holes.  Bands are independent (every pixel is), so this changes nothing
// in the results.  *error: the context's message, set where the error code alone would not say enough
static hipError_t launch_wavefront(WavefrontHost& wf, const KParams& P, int flags, hipStream_t stream, std::string* error) {
  const int tiles_x = (P.tw + 7) / 8, tiles_y = (P.th + 7) / 8;
  int bands = wf.wf_bands > 0 ? wf.wf_bands : (tiles_y >= 32 ? 2 : 1);
  if (bands > RM_WF_MAX_BANDS) bands = RM_WF_MAX_BANDS;
  if (bands > tiles_y) bands = tiles_y;
  const size_t total_rays = (size_t)tiles_x * (size_t)tiles_y * 64;
  hipError_t e;
  if (!wf.heads) {
    int device = 0, cus = 0;
    if (hipGetDevice(&device) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) wf.cu_count = cus;
    if ((e = hipMalloc(reinterpret_cast<void**>(&wf.heads), sizeof(unsigned int) * RM_COUNTERS_PER_MARCH * RM_MAX_MARCHES * RM_WF_MAX_BANDS)) != hipSuccess) return e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&wf.stats), sizeof(unsigned long long) * 16)) != hipSuccess) return e;
    if ((e = hipMemset(wf.stats, 0, sizeof(unsigned long long) * 16)) != hipSuccess) return e;
    for (int s = 0; s < RM_WF_STREAMS; s++) {
      if ((e = hipStreamCreateWithFlags(&wf.wf_stream[s], hipStreamNonBlocking)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&wf.wf_join[s], hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipEventCreateWithFlags(&wf.wf_fork, hipEventDisableTiming)) != hipSuccess) return e;
  }
  if (wf.ws_rays < total_rays) {
    if (wf.ws) {
      if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
      (void)hipFree(wf.ws);
      (void)hipFree(wf.ws_list);
      (void)hipFree(wf.ws_list2);
      wf.ws = nullptr;
      wf.ws_list = nullptr;
      wf.ws_list2 = nullptr;
      wf.ws_rays = 0;
    }
    if ((e = hipMalloc(reinterpret_cast<void**>(&wf.ws), sizeof(float4) * (size_t)rm::WF_ARRAYS * total_rays)) != hipSuccess) {
      char msg[160];
      std::snprintf(msg, sizeof msg, "wavefront pipeline: cannot allocate its %.1f GB ray workspace (%zu rays x %d B); render in tiles or use RM_RENDER_MEGAKERNEL",
                    (double)(sizeof(float4) * (size_t)rm::WF_ARRAYS * total_rays) / 1e9, total_rays, (int)(sizeof(float4) * rm::WF_ARRAYS));
      *error = msg;
      return e;
    }
    if ((e = hipMalloc(reinterpret_cast<void**>(&wf.ws_list), sizeof(unsigned int) * total_rays)) != hipSuccess) return e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&wf.ws_list2), sizeof(unsigned int) * total_rays)) != hipSuccess) return e;
    wf.ws_rays = total_rays;
  }
  if ((e = hipMemsetAsync(wf.heads, 0, sizeof(unsigned int) * RM_COUNTERS_PER_MARCH * RM_MAX_MARCHES * RM_WF_MAX_BANDS, stream)) != hipSuccess) return e;
  if (bands == 1) return launch_wavefront_band(wf, P, flags, stream, wf.ws, wf.ws_list, wf.ws_list2, wf.heads);
  if ((e = hipEventRecord(wf.wf_fork, stream)) != hipSuccess) return e;
  for (int s = 0; s < RM_WF_STREAMS; s++)
    if ((e = hipStreamWaitEvent(wf.wf_stream[s], wf.wf_fork, 0)) != hipSuccess) return e;
  size_t rays_before = 0;
  for (int b = 0; b < bands; b++) {
    const int t0 = (int)((long long)tiles_y * b / bands), t1 = (int)((long long)tiles_y * (b + 1) / bands);
    KParams B = P;
    B.ty = P.ty + t0 * 8;
    B.th = (t1 * 8 < P.th ? t1 * 8 : P.th) - t0 * 8;
    const size_t band_rays = (size_t)tiles_x * (size_t)(t1 - t0) * 64;
    if ((e = launch_wavefront_band(wf, B, flags, wf.wf_stream[b % RM_WF_STREAMS], wf.ws + (size_t)rm::WF_ARRAYS * rays_before,
                                   wf.ws_list + rays_before, wf.ws_list2 + rays_before, wf.heads + (size_t)RM_COUNTERS_PER_MARCH * RM_MAX_MARCHES * b)) != hipSuccess)
      return e;
    rays_before += band_rays;
  }
  for (int s = 0; s < RM_WF_STREAMS; s++) {
    if ((e = hipEventRecord(wf.wf_join[s], wf.wf_stream[s])) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(stream, wf.wf_join[s], 0)) != hipSuccess) return e;
  }
  return hipSuccess;
}
