// rm_napi.cc -- Node N-API binding of libhip_raymarch.so (include/hip_raymarch.h).
//
// Deliberately thin: structs are laid out in JS ArrayBuffers (index.js knows
// the byte offsets of RmUniforms / RmSceneDesc) and handed over as pointers;
// handles travel as N-API externals.  Every function returns a value or
// throws a JS Error carrying rm_last_error(); the render-job layer above
// (index.js doRenderJob) turns those into the reference's error VALUES
// ({success:false, why}), RenderJobExecutor.tsx:112-136.
#include <node_api.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/hip_raymarch.h"

#define NAPI_OK(call)                                             \
  do {                                                            \
    if ((call) != napi_ok) {                                      \
      napi_throw_error(env, nullptr, "N-API call failed: " #call); \
      return nullptr;                                             \
    }                                                             \
  } while (0)

static napi_value throw_rm(napi_env env, rm_ctx* ctx, const char* what) {
  std::string msg = std::string(what) + ": " + rm_last_error(ctx);
  napi_throw_error(env, "RM_ERROR", msg.c_str());
  return nullptr;
}

// Handles travel as externals that carry their kind, so a scene passed where a framebuffer is expected (or a
// destroyed handle used again) is a TypeError in JS, not a wild pointer in the library.
enum HandleKind : uint32_t { KIND_CTX = 0x726d6301u, KIND_SCENE = 0x726d7302u, KIND_FB = 0x726d6603u };
struct Handle {
  uint32_t kind;
  void* ptr;
};
template <class T> struct KindOf;
template <> struct KindOf<rm_ctx> { static constexpr uint32_t value = KIND_CTX; };
template <> struct KindOf<rm_scene> { static constexpr uint32_t value = KIND_SCENE; };
template <> struct KindOf<rm_fb> { static constexpr uint32_t value = KIND_FB; };

static void finalize_handle(napi_env, void* data, void*) { delete static_cast<Handle*>(data); }

template <class T>
static napi_value make_external(napi_env env, T* p) {
  Handle* h = new Handle{KindOf<T>::value, p};
  napi_value out;
  if (napi_create_external(env, h, finalize_handle, nullptr, &out) != napi_ok) {
    delete h;
    napi_throw_error(env, nullptr, "N-API call failed: napi_create_external");
    return nullptr;
  }
  return out;
}

// the handle of kind T, or nullptr (wrong kind, not an external, or already destroyed); take = the caller destroys it
template <class T>
static T* get_external(napi_env env, napi_value v, bool take = false) {
  void* p = nullptr;
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_external) return nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
  Handle* h = static_cast<Handle*>(p);
  if (h->kind != KindOf<T>::value) return nullptr;
  T* out = static_cast<T*>(h->ptr);
  if (take) h->ptr = nullptr;
  return out;
}

static bool get_buffer(napi_env env, napi_value v, void** data, size_t* len) {
  bool is_ab = false;
  if (napi_is_arraybuffer(env, v, &is_ab) == napi_ok && is_ab) return napi_get_arraybuffer_info(env, v, data, len) == napi_ok;
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) == napi_ok && is_ta) {
    napi_typedarray_type t;
    size_t n, off;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &n, data, &ab, &off) != napi_ok) return false;
    static const size_t width[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
    *len = n * width[t];
    return true;
  }
  return false;
}

static napi_value CtxCreate(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t device = 0;
  if (argc > 0) napi_get_value_int32(env, argv[0], &device);
  rm_ctx* ctx = nullptr;
  if (rm_ctx_create(device, &ctx) != RM_OK) return throw_rm(env, nullptr, "rm_ctx_create");
  return make_external(env, ctx);
}

static napi_value CtxDestroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx_destroy(get_external<rm_ctx>(env, argv[0], true));
  return nullptr;
}

static napi_value Sync(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  if (rm_sync(ctx) != RM_OK) return throw_rm(env, ctx, "rm_sync");
  return nullptr;
}

// sceneCreate(ctx, descBuffer /* RmSceneDesc bytes, prims pointer ignored */, primsBuffer | null)
static napi_value SceneCreate(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !get_buffer(env, argv[1], &d, &n) || n != sizeof(RmSceneDesc)) {
    napi_throw_type_error(env, nullptr, "sceneCreate(ctx, desc: ArrayBuffer(sizeof RmSceneDesc), prims)");
    return nullptr;
  }
  RmSceneDesc desc;
  std::memcpy(&desc, d, sizeof desc);
  desc.prims = nullptr;
  void* p = nullptr;
  size_t pn = 0;
  if (argc > 2 && get_buffer(env, argv[2], &p, &pn)) {
    if (pn != sizeof(RmPrim) * (size_t)desc.nprims) {
      napi_throw_type_error(env, nullptr, "sceneCreate: prims buffer must hold nprims rows of 32 bytes");
      return nullptr;
    }
    desc.prims = static_cast<const RmPrim*>(p);
  }
  // sceneCreate(ctx, desc, prims | null, surfaces | null): RmSurface rows (48 bytes each), desc.nsurfaces of them
  desc.surfaces = nullptr;
  void* sf = nullptr;
  size_t sn = 0;
  if (argc > 3 && get_buffer(env, argv[3], &sf, &sn)) {
    if (sn != sizeof(RmSurface) * (size_t)desc.nsurfaces) {
      napi_throw_type_error(env, nullptr, "sceneCreate: surfaces buffer must hold nsurfaces rows of 48 bytes");
      return nullptr;
    }
    desc.surfaces = static_cast<const RmSurface*>(sf);
  } else if (desc.nsurfaces != 0) {
    napi_throw_type_error(env, nullptr, "sceneCreate: desc.nsurfaces is set but no surfaces buffer was given");
    return nullptr;
  }
  rm_scene* scene = nullptr;
  if (rm_scene_create(ctx, &desc, &scene) != RM_OK) return throw_rm(env, ctx, "rm_scene_create");
  return make_external(env, scene);
}

static napi_value SceneDestroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_scene_destroy(get_external<rm_scene>(env, argv[0], true));
  return nullptr;
}

// fbCreate(ctx, width, height, rowBegin, rowCount[, gbuffer]): gbuffer = RM_GBUFFER_F32 (default) or RM_GBUFFER_F16
static napi_value FbCreate(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  int32_t v[5] = {0, 0, 0, 0, RM_GBUFFER_F32};
  for (int i = 0; i < 5 && 1 + i < (int)argc; i++) napi_get_value_int32(env, argv[1 + i], &v[i]);
  rm_fb* fb = nullptr;
  if (rm_fb_create_fmt(ctx, v[0], v[1], v[2], v[3], v[4], &fb) != RM_OK) return throw_rm(env, ctx, "rm_fb_create");
  return make_external(env, fb);
}

static napi_value FbClear(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_fb* fb = get_external<rm_fb>(env, argv[0]);
  if (!fb) {
    napi_throw_type_error(env, nullptr, "fbClear(fb): not a framebuffer handle");
    return nullptr;
  }
  if (rm_fb_clear(fb) != RM_OK) {
    napi_throw_error(env, "RM_ERROR", "rm_fb_clear failed");
    return nullptr;
  }
  return nullptr;
}

static napi_value FbDestroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_fb_destroy(get_external<rm_fb>(env, argv[0], true));
  return nullptr;
}

// fbDownload(ctx, fb, plane, out: Float32Array(rows*width*4))
static napi_value FbDownload(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  rm_fb* fb = get_external<rm_fb>(env, argv[1]);
  int32_t plane = 0;
  napi_get_value_int32(env, argv[2], &plane);
  void* d = nullptr;
  size_t n = 0;
  if (!fb || !get_buffer(env, argv[3], &d, &n)) {
    napi_throw_type_error(env, nullptr, "fbDownload(ctx, fb, plane, out: Float32Array)");
    return nullptr;
  }
  const size_t need = (size_t)rm_fb_rows(fb) * (size_t)rm_fb_width(fb) * 16;
  if (n < need) {
    napi_throw_range_error(env, nullptr, "fbDownload: out is smaller than rows * width * 4 floats");
    return nullptr;
  }
  if (rm_fb_download(fb, plane, static_cast<float*>(d)) != RM_OK) return throw_rm(env, ctx, "rm_fb_download");
  return nullptr;
}

// present(ctx, fb, samples, out: Uint8Array(width * height * 4)): display.frag on the GPU, RGBA8, row 0 = bottom
static napi_value Present(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  rm_fb* fb = get_external<rm_fb>(env, argv[1]);
  int32_t samples = 1;
  napi_get_value_int32(env, argv[2], &samples);
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !fb || !get_buffer(env, argv[3], &d, &n)) {
    napi_throw_type_error(env, nullptr, "present(ctx, fb, samples, out: Uint8Array)");
    return nullptr;
  }
  if (n < (size_t)rm_fb_width(fb) * (size_t)rm_fb_height(fb) * 4) {
    napi_throw_range_error(env, nullptr, "present: out is smaller than width * height * 4 bytes");
    return nullptr;
  }
  if (rm_present(ctx, fb, samples, static_cast<uint8_t*>(d)) != RM_OK) return throw_rm(env, ctx, "rm_present");
  return nullptr;
}

// ---- the frame filters: denoise*, denoiseVariance*, filter* ----
// A parameter block's fields as JS names them.  INT: a number truncated to int (-1 beyond +-1e9, which every range check refuses);
// FLAG: 1 for a number other than 0, else 0; UINT64: a number truncated to uint64_t (all-ones for one that is no such count).  The library checks the values (RM_ERR_INVALID before any device work).
struct Field {
  const char* name;
  enum Kind { INT, FLOAT, FLAG, UINT64 } kind;
  size_t offset;
};
static const Field DENOISE_FIELDS[] = {{"iterations", Field::INT, offsetof(RmDenoise, iterations)}, {"sigma_color", Field::FLOAT, offsetof(RmDenoise, sigma_color)},
                                       {"sigma_normal", Field::FLOAT, offsetof(RmDenoise, sigma_normal)}, {"sigma_depth", Field::FLOAT, offsetof(RmDenoise, sigma_depth)}};
static const Field VARIANCE_FIELDS[] = {{"iterations", Field::INT, offsetof(RmDenoiseVariance, iterations)}, {"sigma_luminance", Field::FLOAT, offsetof(RmDenoiseVariance, sigma_luminance)},
                                        {"sigma_normal", Field::FLOAT, offsetof(RmDenoiseVariance, sigma_normal)}, {"sigma_depth", Field::FLOAT, offsetof(RmDenoiseVariance, sigma_depth)}};
static const Field DESPECKLE_FIELDS[] = {{"radius", Field::INT, offsetof(RmDespeckle, radius)}, {"rank", Field::INT, offsetof(RmDespeckle, rank)}, {"gain", Field::FLOAT, offsetof(RmDespeckle, gain)},
                                         {"floor", Field::FLOAT, offsetof(RmDespeckle, floor)}, {"repair", Field::FLAG, offsetof(RmDespeckle, repair)}};

// A parameter block of a JS value, over the defaults the caller has filled in: null / undefined leave them (*given = false); an
// object's properties named in `fields` (numbers) replace them, its other properties are ignored; anything else is refused.
template <size_t N>
static bool get_block(napi_env env, napi_value v, void* block, const Field (&fields)[N], bool* given = nullptr) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok) return false;
  if (given) *given = t == napi_object;
  if (t == napi_undefined || t == napi_null) return true;
  if (t != napi_object) return false;
  for (const Field& f : fields) {
    bool has = false;
    napi_value x;
    if (napi_has_named_property(env, v, f.name, &has) != napi_ok) return false;
    if (!has) continue;
    double d = 0.0;
    if (napi_get_named_property(env, v, f.name, &x) != napi_ok || napi_get_value_double(env, x, &d) != napi_ok) return false;
    char* at = static_cast<char*>(block) + f.offset;
    if (f.kind == Field::FLOAT) *reinterpret_cast<float*>(at) = (float)d;
    else if (f.kind == Field::UINT64) *reinterpret_cast<uint64_t*>(at) = (d >= 0.0 && d < 18446744073709551616.0) ? (uint64_t)d : ~(uint64_t)0;
    else *reinterpret_cast<int*>(at) = f.kind == Field::FLAG ? (d != 0.0 ? 1 : 0) : (d >= -1e9 && d <= 1e9) ? (int)d : -1;
  }
  return true;
}

// The RmFilters (at rm_filters_default) of a JS object { despeckle, denoise, atrous, variance }: `despeckle` (null / undefined = the
// stage off, an object of its parameters = the stage on), `denoise` (the RM_DENOISE_* number; undefined = none) and the parameter
// blocks `atrous` / `variance` as denoise / denoiseVariance take them.
static bool get_filters(napi_env env, napi_value v, RmFilters* f) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_object) return false;
  napi_value d, m, a, va;
  if (napi_get_named_property(env, v, "despeckle", &d) != napi_ok || napi_get_named_property(env, v, "denoise", &m) != napi_ok ||
      napi_get_named_property(env, v, "atrous", &a) != napi_ok || napi_get_named_property(env, v, "variance", &va) != napi_ok)
    return false;
  bool on = false;
  if (!get_block(env, d, &f->despeckle_params, DESPECKLE_FIELDS, &on)) return false;
  f->despeckle = on ? 1 : 0;
  if (napi_typeof(env, m, &t) != napi_ok) return false;
  if (t == napi_number) {
    int32_t mode = 0;
    if (napi_get_value_int32(env, m, &mode) != napi_ok) return false;
    f->denoise = mode;
  } else if (t != napi_undefined && t != napi_null) {
    return false;
  }
  return get_block(env, a, &f->atrous, DENOISE_FIELDS) && get_block(env, va, &f->variance, VARIANCE_FIELDS);
}

// The six exports, (ctx, fb, samples, params | filters, out), each through its own C entry point.  `out` of the float plane:
// Float32Array(width * height * 4), colour-plane units; of the present: Uint8Array(width * height * 4); row 0 = bottom.
//   denoise         = rm_denoise           presentDenoised         = rm_present_denoised            params: RmDenoise's fields, or null
//   denoiseVariance = rm_denoise_variance  presentDenoisedVariance = rm_present_denoised_variance   params: RmDenoiseVariance's, or null
//   filter          = rm_filter            presentFiltered         = rm_present_filtered            filters: what get_filters takes
enum Family { ATROUS, VARIANCE, CHAIN };
static napi_value filter_common(napi_env env, napi_callback_info info, Family family, bool present) {
  static const char* const JS_NAME[3][2] = {{"denoise", "presentDenoised"}, {"denoiseVariance", "presentDenoisedVariance"}, {"filter", "presentFiltered"}};
  static const char* const C_NAME[3][2] = {{"rm_denoise", "rm_present_denoised"}, {"rm_denoise_variance", "rm_present_denoised_variance"}, {"rm_filter", "rm_present_filtered"}};
  const std::string who = JS_NAME[family][present];
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = argc == 5 ? get_external<rm_ctx>(env, argv[0]) : nullptr;
  rm_fb* fb = argc == 5 ? get_external<rm_fb>(env, argv[1]) : nullptr;
  int32_t samples = 1;
  RmFilters f;
  rm_filters_default(&f);
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !fb || napi_get_value_int32(env, argv[2], &samples) != napi_ok ||
      !(family == ATROUS ? get_block(env, argv[3], &f.atrous, DENOISE_FIELDS) : family == VARIANCE ? get_block(env, argv[3], &f.variance, VARIANCE_FIELDS) : get_filters(env, argv[3], &f)) ||
      !get_buffer(env, argv[4], &d, &n)) {
    napi_throw_type_error(env, nullptr, (who + "(ctx, fb, samples, " + (family == CHAIN ? "filters" : "params") + ", out: " + (present ? "Uint8Array" : "Float32Array") + ")").c_str());
    return nullptr;
  }
  const size_t need = (size_t)rm_fb_width(fb) * (size_t)rm_fb_rows(fb) * 4 * (present ? 1 : sizeof(float));
  if (n < need) {
    napi_throw_range_error(env, nullptr, (who + ": out is smaller than the frame").c_str());
    return nullptr;
  }
  uint8_t* rgba8 = static_cast<uint8_t*>(d);
  float* plane = static_cast<float*>(d);
  const int rc = family == ATROUS     ? (present ? rm_present_denoised(ctx, fb, samples, &f.atrous, rgba8) : rm_denoise(ctx, fb, samples, &f.atrous, plane))
                 : family == VARIANCE ? (present ? rm_present_denoised_variance(ctx, fb, samples, &f.variance, rgba8) : rm_denoise_variance(ctx, fb, samples, &f.variance, plane))
                                      : (present ? rm_present_filtered(ctx, fb, samples, &f, rgba8) : rm_filter(ctx, fb, samples, &f, plane));
  if (rc != RM_OK) return throw_rm(env, ctx, C_NAME[family][present]);
  return nullptr;
}
static napi_value Denoise(napi_env env, napi_callback_info info) { return filter_common(env, info, ATROUS, false); }
static napi_value PresentDenoised(napi_env env, napi_callback_info info) { return filter_common(env, info, ATROUS, true); }
static napi_value DenoiseVariance(napi_env env, napi_callback_info info) { return filter_common(env, info, VARIANCE, false); }
static napi_value PresentDenoisedVariance(napi_env env, napi_callback_info info) { return filter_common(env, info, VARIANCE, true); }
static napi_value Filter(napi_env env, napi_callback_info info) { return filter_common(env, info, CHAIN, false); }
static napi_value PresentFiltered(napi_env env, napi_callback_info info) { return filter_common(env, info, CHAIN, true); }

// ---- the display transform and the frame statistics: presentDisplay, presentLinear, frameStats, statsExposure, statsPercentile ----
static const Field DISPLAY_FIELDS[] = {{"gain", Field::FLOAT, offsetof(RmDisplay, gain)}, {"tone", Field::INT, offsetof(RmDisplay, tone)}, {"white", Field::FLOAT, offsetof(RmDisplay, white)}};
static const Field AUTO_EXPOSURE_FIELDS[] = {{"key", Field::FLOAT, offsetof(RmAutoExposure, key)}, {"low", Field::FLOAT, offsetof(RmAutoExposure, low)}, {"high", Field::FLOAT, offsetof(RmAutoExposure, high)},
                                             {"min_gain", Field::FLOAT, offsetof(RmAutoExposure, min_gain)}, {"max_gain", Field::FLOAT, offsetof(RmAutoExposure, max_gain)}};

// presentDisplay(ctx, fb, samples, filters, display, out: Uint8Array(width * height * 4))   = rm_present_display
// presentLinear(ctx, fb, samples, filters, display, out: Float32Array(width * height * 4))  = rm_present_linear
// filters: what get_filters takes; display: { gain, tone (the RM_TONE_* number), white } or null (the default)
static napi_value display_common(napi_env env, napi_callback_info info, bool linear) {
  const std::string who = linear ? "presentLinear" : "presentDisplay";
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = argc == 6 ? get_external<rm_ctx>(env, argv[0]) : nullptr;
  rm_fb* fb = argc == 6 ? get_external<rm_fb>(env, argv[1]) : nullptr;
  int32_t samples = 1;
  RmFilters f;
  rm_filters_default(&f);
  RmDisplay disp;
  rm_display_default(&disp);
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !fb || napi_get_value_int32(env, argv[2], &samples) != napi_ok || !get_filters(env, argv[3], &f) || !get_block(env, argv[4], &disp, DISPLAY_FIELDS) ||
      !get_buffer(env, argv[5], &d, &n)) {
    napi_throw_type_error(env, nullptr, (who + "(ctx, fb, samples, filters, display, out: " + (linear ? "Float32Array" : "Uint8Array") + ")").c_str());
    return nullptr;
  }
  if (n < (size_t)rm_fb_width(fb) * (size_t)rm_fb_height(fb) * 4 * (linear ? sizeof(float) : 1)) {
    napi_throw_range_error(env, nullptr, (who + ": out is smaller than the frame").c_str());
    return nullptr;
  }
  const int rc = linear ? rm_present_linear(ctx, fb, samples, &f, &disp, static_cast<float*>(d)) : rm_present_display(ctx, fb, samples, &f, &disp, static_cast<uint8_t*>(d));
  if (rc != RM_OK) return throw_rm(env, ctx, linear ? "rm_present_linear" : "rm_present_display");
  return nullptr;
}
static napi_value PresentDisplay(napi_env env, napi_callback_info info) { return display_common(env, info, false); }
static napi_value PresentLinear(napi_env env, napi_callback_info info) { return display_common(env, info, true); }

// frameStats(ctx, fb, samples, filters | null, out: ArrayBuffer(sizeof(RmFrameStats))) = rm_frame_stats: the struct as it is
static napi_value FrameStats(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = argc == 5 ? get_external<rm_ctx>(env, argv[0]) : nullptr;
  rm_fb* fb = argc == 5 ? get_external<rm_fb>(env, argv[1]) : nullptr;
  int32_t samples = 1;
  RmFilters f;
  rm_filters_default(&f);
  napi_valuetype t = napi_undefined;
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !fb || napi_get_value_int32(env, argv[2], &samples) != napi_ok || napi_typeof(env, argv[3], &t) != napi_ok ||
      !(t == napi_null || t == napi_undefined || get_filters(env, argv[3], &f)) || !get_buffer(env, argv[4], &d, &n) || n != sizeof(RmFrameStats)) {
    napi_throw_type_error(env, nullptr, "frameStats(ctx, fb, samples, filters | null, out: ArrayBuffer of sizeof(RmFrameStats) bytes)");
    return nullptr;
  }
  RmFrameStats st;
  if (rm_frame_stats(ctx, fb, samples, (t == napi_null || t == napi_undefined) ? nullptr : &f, &st) != RM_OK) return throw_rm(env, ctx, "rm_frame_stats");
  std::memcpy(d, &st, sizeof st);
  return nullptr;
}

// statsExposure(stats: ArrayBuffer(sizeof(RmFrameStats)), params | null) = rm_stats_exposure; statsPercentile(stats, q) = rm_stats_percentile
static napi_value stats_host(napi_env env, napi_callback_info info, bool exposure) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  void* d = nullptr;
  size_t n = 0;
  RmAutoExposure p;
  rm_auto_exposure_default(&p);
  double q = 0.0;
  if (argc != 2 || !get_buffer(env, argv[0], &d, &n) || n != sizeof(RmFrameStats) ||
      !(exposure ? get_block(env, argv[1], &p, AUTO_EXPOSURE_FIELDS) : napi_get_value_double(env, argv[1], &q) == napi_ok)) {
    napi_throw_type_error(env, nullptr, exposure ? "statsExposure(stats: ArrayBuffer of sizeof(RmFrameStats) bytes, params | null)" : "statsPercentile(stats: ArrayBuffer of sizeof(RmFrameStats) bytes, q: number)");
    return nullptr;
  }
  RmFrameStats st;
  std::memcpy(&st, d, sizeof st);
  float r = 0.0f;
  if ((exposure ? rm_stats_exposure(&st, &p, &r) : rm_stats_percentile(&st, q, &r)) != RM_OK) {
    napi_throw_range_error(env, nullptr, exposure ? "statsExposure: refused by rm_stats_exposure (0 <= low < high <= 1, key > 0, 0 < min_gain <= max_gain, all finite)" : "statsPercentile: q must be in [0, 1]");
    return nullptr;
  }
  napi_value out;
  NAPI_OK(napi_create_double(env, (double)r, &out));
  return out;
}
static napi_value StatsExposure(napi_env env, napi_callback_info info) { return stats_host(env, info, true); }
static napi_value StatsPercentile(napi_env env, napi_callback_info info) { return stats_host(env, info, false); }

// ---- mesh extraction: meshBlocks, sdfGrid, extractMesh, meshFromValues (include/hip_raymarch.h "mesh extraction") ----
static const Field MESH_FIELDS[] = {{"iso", Field::FLOAT, offsetof(RmMeshParams, iso)}, {"normals", Field::INT, offsetof(RmMeshParams, normals)},
                                    {"normalDelta", Field::FLOAT, offsetof(RmMeshParams, normal_delta)}, {"colours", Field::INT, offsetof(RmMeshParams, colours)},
                                    {"flags", Field::INT, offsetof(RmMeshParams, flags)}};

// The RmGrid of { lo: [x, y, z], hi: [x, y, z], n: [nx, ny, nz] } (numbers; n truncated as an INT field is).  The library checks the values.
static bool get_grid(napi_env env, napi_value v, RmGrid* g) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_object) return false;
  std::memset(g, 0, sizeof *g);
  static const char* const NAMES[3] = {"lo", "hi", "n"};
  for (int k = 0; k < 3; k++) {
    napi_value a;
    uint32_t len = 0;
    bool is_array = false;
    if (napi_get_named_property(env, v, NAMES[k], &a) != napi_ok || napi_is_array(env, a, &is_array) != napi_ok || !is_array ||
        napi_get_array_length(env, a, &len) != napi_ok || len != 3)
      return false;
    for (uint32_t i = 0; i < 3; i++) {
      napi_value x;
      double d = 0.0;
      if (napi_get_element(env, a, i, &x) != napi_ok || napi_get_value_double(env, x, &d) != napi_ok) return false;
      if (k == 0) g->lo[i] = (float)d;
      else if (k == 1) g->hi[i] = (float)d;
      else g->n[i] = (d >= -1e9 && d <= 1e9) ? (int32_t)d : -1;
    }
  }
  return true;
}

static const Field MESH_SHARP_FIELDS[] = {{"refine", Field::INT, offsetof(RmMeshSharp, refine)}, {"normalDelta", Field::FLOAT, offsetof(RmMeshSharp, normal_delta)},
                                          {"threshold", Field::FLOAT, offsetof(RmMeshSharp, threshold)}};
static const Field MESH_KEEP_FIELDS[] = {{"minTriangles", Field::INT, offsetof(RmMeshKeep, min_triangles)}, {"largest", Field::INT, offsetof(RmMeshKeep, largest)}};
static const Field MESH_SIMPLIFY_FIELDS[] = {{"keepDuplicates", Field::FLAG, offsetof(RmMeshSimplify, keep_duplicates)}};
static const Field MESH_QUADRIC_FIELDS[] = {{"threshold", Field::FLOAT, offsetof(RmMeshQuadric, threshold)}};
static const Field MESH_OCCLUSION_FIELDS[] = {{"radius", Field::FLOAT, offsetof(RmMeshOcclusion, radius)}, {"directions", Field::INT, offsetof(RmMeshOcclusion, directions)},
                                              {"taps", Field::INT, offsetof(RmMeshOcclusion, taps)}, {"normalDelta", Field::FLOAT, offsetof(RmMeshOcclusion, normal_delta)},
                                              {"strength", Field::FLOAT, offsetof(RmMeshOcclusion, strength)}, {"flags", Field::INT, offsetof(RmMeshOcclusion, flags)}};
static const Field MESH_PROJECT_FIELDS[] = {{"iso", Field::FLOAT, offsetof(RmMeshProject, iso)}, {"rounds", Field::INT, offsetof(RmMeshProject, rounds)},
                                            {"relax", Field::FLOAT, offsetof(RmMeshProject, relax)}, {"tolerance", Field::FLOAT, offsetof(RmMeshProject, tolerance)},
                                            {"reach", Field::FLOAT, offsetof(RmMeshProject, reach)}, {"normalDelta", Field::FLOAT, offsetof(RmMeshProject, normal_delta)},
                                            {"flags", Field::INT, offsetof(RmMeshProject, flags)}};
static const Field MESH_DEVIATION_FIELDS[] = {{"iso", Field::FLOAT, offsetof(RmMeshDeviation, iso)}, {"order", Field::INT, offsetof(RmMeshDeviation, order)},
                                              {"tolerance", Field::FLOAT, offsetof(RmMeshDeviation, tolerance)}, {"flags", Field::INT, offsetof(RmMeshDeviation, flags)}};
static const Field MESH_REFINE_FIELDS[] = {{"iso", Field::FLOAT, offsetof(RmMeshRefine, iso)}, {"tolerance", Field::FLOAT, offsetof(RmMeshRefine, tolerance)},
                                           {"minEdge", Field::FLOAT, offsetof(RmMeshRefine, min_edge)}, {"rounds", Field::INT, offsetof(RmMeshRefine, rounds)},
                                           {"maxTriangles", Field::UINT64, offsetof(RmMeshRefine, max_triangles)}, {"flags", Field::INT, offsetof(RmMeshRefine, flags)}};
static const Field MESH_SLABS_FIELDS[] = {{"layers", Field::INT, offsetof(RmMeshSlabs, layers)}};

// A block of the mesh calls of a JS value: the library's defaults, then get_block's rules (null / undefined = the defaults and *given = false,
// an object = its fields over them)
template <class T, size_t N>
static bool get_mesh_block(napi_env env, napi_value v, T* block, const Field (&fields)[N], void (*defaults)(T*), bool* given = nullptr) {
  defaults(block);
  return get_block(env, v, block, fields, given);
}

// the simplify block: an object { grid: { lo, hi, n }, keepDuplicates } = rm_mesh_simplify on that grid of clusters
struct MeshSimplifyBlock {
  RmGrid clusters;
  RmMeshSimplify params;
};
static bool get_mesh_simplify(napi_env env, napi_value v, MeshSimplifyBlock* s, bool* given) {
  std::memset(&s->clusters, 0, sizeof s->clusters);
  if (!get_mesh_block(env, v, &s->params, MESH_SIMPLIFY_FIELDS, rm_mesh_simplify_default, given)) return false;
  if (!*given) return true;
  napi_value g;
  return napi_get_named_property(env, v, "grid", &g) == napi_ok && get_grid(env, g, &s->clusters);
}

// any value as its truth (JavaScript's ToBoolean)
static bool get_bool(napi_env env, napi_value v, bool* out) {
  napi_value b;
  return napi_coerce_to_bool(env, v, &b) == napi_ok && napi_get_value_bool(env, b, out) == napi_ok;
}

static napi_value make_array(napi_env env, napi_typedarray_type type, size_t count, void** data) {
  napi_value ab, out;
  if (napi_create_arraybuffer(env, count * 4, data, &ab) != napi_ok || napi_create_typedarray(env, type, count, ab, 0, &out) != napi_ok) return nullptr;
  return out;
}

// The seven exports mesh<Name>Block(block | null) -> ArrayBuffer(the block's struct): the bytes the mesh calls hand to the library (null: the defaults)
template <class T, size_t N>
static napi_value mesh_block_bytes(napi_env env, napi_callback_info info, const Field (&fields)[N], void (*defaults)(T*), const char* usage) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  T block;
  if (argc != 1 || !get_mesh_block(env, argv[0], &block, fields, defaults)) {
    napi_throw_type_error(env, nullptr, usage);
    return nullptr;
  }
  napi_value b;
  void* d = nullptr;
  NAPI_OK(napi_create_arraybuffer(env, sizeof block, &d, &b));
  std::memcpy(d, &block, sizeof block);
  return b;
}
static napi_value MeshSharpBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_SHARP_FIELDS, rm_mesh_sharp_default, "meshSharpBlock(sharp | null)"); }
static napi_value MeshKeepBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_KEEP_FIELDS, rm_mesh_keep_default, "meshKeepBlock(keep | null)"); }
static napi_value MeshQuadricBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_QUADRIC_FIELDS, rm_mesh_quadric_default, "meshQuadricBlock(quadric | null)"); }
static napi_value MeshOcclusionBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_OCCLUSION_FIELDS, rm_mesh_occlusion_default, "meshOcclusionBlock(occlusion | null)"); }
static napi_value MeshProjectBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_PROJECT_FIELDS, rm_mesh_project_default, "meshProjectBlock(project | null)"); }
static napi_value MeshDeviationBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_DEVIATION_FIELDS, rm_mesh_deviation_default, "meshDeviationBlock(deviation | null)"); }
static napi_value MeshRefineBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_REFINE_FIELDS, rm_mesh_refine_default, "meshRefineBlock(refine | null)"); }
static napi_value MeshSlabsBlock(napi_env env, napi_callback_info info) { return mesh_block_bytes(env, info, MESH_SLABS_FIELDS, rm_mesh_slabs_default, "meshSlabsBlock(slabs | null)"); }

// { grid: ArrayBuffer(RmGrid), params: ArrayBuffer(the block's struct) }: what meshBlocks and meshSimplifyBlock return
template <class T>
static napi_value grid_and_params(napi_env env, const RmGrid& g, const T& p) {
  napi_value o, gb, pb;
  void *gd = nullptr, *pd = nullptr;
  NAPI_OK(napi_create_object(env, &o));
  NAPI_OK(napi_create_arraybuffer(env, sizeof g, &gd, &gb));
  NAPI_OK(napi_create_arraybuffer(env, sizeof p, &pd, &pb));
  std::memcpy(gd, &g, sizeof g);
  std::memcpy(pd, &p, sizeof p);
  NAPI_OK(napi_set_named_property(env, o, "grid", gb));
  NAPI_OK(napi_set_named_property(env, o, "params", pb));
  return o;
}

// meshSimplifyBlock(simplify) -> the bytes the mesh calls hand to rm_mesh_simplify; there is no default grid, so a block must be given
static napi_value MeshSimplifyBlockOf(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  MeshSimplifyBlock s;
  bool given = false;
  if (argc != 1 || !get_mesh_simplify(env, argv[0], &s, &given) || !given) {
    napi_throw_type_error(env, nullptr, "meshSimplifyBlock(simplify: { grid: { lo, hi, n }, keepDuplicates })");
    return nullptr;
  }
  return grid_and_params(env, s.clusters, s.params);
}

// meshBlocks(grid, params | null) -> the bytes the calls below hand to the library
static napi_value MeshBlocks(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  RmGrid g;
  RmMeshParams p;
  if (argc != 2 || !get_grid(env, argv[0], &g) || !get_mesh_block(env, argv[1], &p, MESH_FIELDS, rm_mesh_params_default)) {
    napi_throw_type_error(env, nullptr, "meshBlocks(grid: { lo, hi, n }, params | null)");
    return nullptr;
  }
  return grid_and_params(env, g, p);
}

// sdfGrid(ctx, scene, grid, flags, out: Float32Array(corners)) = rm_sdf_grid
static napi_value SdfGrid(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = argc == 5 ? get_external<rm_ctx>(env, argv[0]) : nullptr;
  rm_scene* scene = argc == 5 ? get_external<rm_scene>(env, argv[1]) : nullptr;
  RmGrid g;
  int32_t flags = 0;
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !scene || !get_grid(env, argv[2], &g) || napi_get_value_int32(env, argv[3], &flags) != napi_ok || !get_buffer(env, argv[4], &d, &n)) {
    napi_throw_type_error(env, nullptr, "sdfGrid(ctx, scene, grid, flags, out: Float32Array)");
    return nullptr;
  }
  float probe[1025];
  if (rm_grid_axis(&g, 0, probe) != RM_OK) return throw_rm(env, nullptr, "rm_sdf_grid");  // (the size below is a valid grid's)
  if (n != (size_t)(g.n[0] + 1) * (size_t)(g.n[1] + 1) * (size_t)(g.n[2] + 1) * sizeof(float)) {
    napi_throw_range_error(env, nullptr, "sdfGrid: out must hold (nx + 1)(ny + 1)(nz + 1) floats");
    return nullptr;
  }
  if (rm_sdf_grid(ctx, scene, &g, flags, static_cast<float*>(d)) != RM_OK) return throw_rm(env, ctx, "rm_sdf_grid");
  return nullptr;
}

struct Number {
  const char* name;
  double value;
};
// a table of names and numbers as properties of o
template <size_t N>
static bool set_numbers(napi_env env, napi_value o, const Number (&table)[N]) {
  napi_value v = nullptr;
  for (const Number& n : table)
    if (napi_create_double(env, n.value, &v) != napi_ok || napi_set_named_property(env, o, n.name, v) != napi_ok) return false;
  return true;
}
// floats as a JS array of Numbers, or nullptr
static napi_value float_array(napi_env env, const float* values, uint32_t count) {
  napi_value a = nullptr, v = nullptr;
  if (napi_create_array_with_length(env, count, &a) != napi_ok) return nullptr;
  for (uint32_t k = 0; k < count; k++)
    if (napi_create_double(env, (double)values[k], &v) != napi_ok || napi_set_element(env, a, k, v) != napi_ok) return nullptr;
  return a;
}

// the `measures` of a mesh result: RmMeshMeasures' fields in camel case, the counts as Numbers (all below 2^53: V, T < 2^32, E <= 3 T), lo / hi as
// arrays of three, closed as a boolean, componentEdges: BigUint64Array(4 C) (rm_mesh_measure_components), milliseconds: [topology, geometry]
static napi_value measures_object(napi_env env, const RmMeshMeasures& m, const float* ms2, rm_mesh* mesh, bool* rm_failed) {
  *rm_failed = false;
  napi_value o = nullptr, v = nullptr;
  if (napi_create_object(env, &o) != napi_ok) return nullptr;
  const Number NUMBERS[] = {
      {"vertices", (double)m.vertices}, {"triangles", (double)m.triangles}, {"usedVertices", (double)m.used_vertices}, {"skippedTriangles", (double)m.skipped_triangles},
      {"unmeasuredTriangles", (double)m.unmeasured_triangles}, {"finiteVertices", (double)m.finite_vertices}, {"edges", (double)m.edges},
      {"boundaryEdges", (double)m.boundary_edges}, {"regularEdges", (double)m.regular_edges}, {"irregularEdges", (double)m.irregular_edges},
      {"unbalancedEdges", (double)m.unbalanced_edges}, {"euler", (double)m.euler}, {"components", (double)m.components},
      {"closedComponents", (double)m.closed_components}, {"area", m.area}, {"volume", m.volume}};
  if (!set_numbers(env, o, NUMBERS)) return nullptr;
  const struct { const char* name; const float* values; uint32_t count; } TRIPLES[] = {{"lo", m.lo, 3}, {"hi", m.hi, 3}, {"milliseconds", ms2, 2}};
  for (const auto& t : TRIPLES)
    if (!(v = float_array(env, t.values, t.count)) || napi_set_named_property(env, o, t.name, v) != napi_ok) return nullptr;
  if (napi_get_boolean(env, m.closed != 0, &v) != napi_ok || napi_set_named_property(env, o, "closed", v) != napi_ok) return nullptr;
  napi_value ab = nullptr, rows = nullptr;
  void* data = nullptr;
  const size_t words = 4u * (size_t)m.components;
  if (napi_create_arraybuffer(env, words * 8u, &data, &ab) != napi_ok || napi_create_typedarray(env, napi_biguint64_array, words, ab, 0, &rows) != napi_ok) return nullptr;
  if (rm_mesh_measure_components(mesh, data, words * 8u) != RM_OK) {
    *rm_failed = true;
    return nullptr;
  }
  if (napi_set_named_property(env, o, "componentEdges", rows) != napi_ok) return nullptr;
  return o;
}

// Every stage a mesh call may run behind its extraction: the blocks, whether each was given, and the scene the scene passes evaluate
struct MeshStages {
  RmMeshSharp sharp;
  RmMeshKeep keep;
  MeshSimplifyBlock simplify;
  RmMeshQuadric quadric;
  RmMeshOcclusion occlusion;
  RmMeshProject project;
  RmMeshDeviation deviation;
  RmMeshRefine refine;           // extractMeshRefined alone: the block, and the projection inside its rounds
  RmMeshProject refine_project;
  bool has_refine = false;
  bool has_sharp = false, has_keep = false, components = false, has_simplify = false, has_quadric = false, has_occlusion = false, measures = false,
       has_project = false, has_deviation = false;
  bool normals = false, colours = false;  // whether the extraction was asked for them
  rm_scene* scene = nullptr;
};
// the stages as the entries' arguments list them: extractMesh / extractMeshSlabs take all nine, meshFromValues / meshFromValuesSlabs the five without a scene
enum class Stage { SHARP, KEEP, COMPONENTS, SIMPLIFY, QUADRIC, OCCLUSION, MEASURES, PROJECT, DEVIATION };
static const Stage SCENE_STAGES[] = {Stage::SHARP, Stage::KEEP, Stage::COMPONENTS, Stage::SIMPLIFY, Stage::QUADRIC, Stage::OCCLUSION, Stage::MEASURES, Stage::PROJECT, Stage::DEVIATION};
static const Stage VALUES_STAGES[] = {Stage::KEEP, Stage::COMPONENTS, Stage::SIMPLIFY, Stage::QUADRIC, Stage::MEASURES};
// argv[at ...] as the `accepted` stages (an argument the caller left out is undefined: the stage is off); a quadric block without a simplify block is refused
template <size_t N>
static bool get_mesh_stages(napi_env env, const napi_value* argv, size_t at, const Stage (&accepted)[N], MeshStages* m) {
  for (size_t i = 0; i < N; i++) {
    const napi_value v = argv[at + i];
    bool ok = false;
    switch (accepted[i]) {
      case Stage::SHARP: ok = get_mesh_block(env, v, &m->sharp, MESH_SHARP_FIELDS, rm_mesh_sharp_default, &m->has_sharp); break;
      case Stage::KEEP: ok = get_mesh_block(env, v, &m->keep, MESH_KEEP_FIELDS, rm_mesh_keep_default, &m->has_keep); break;
      case Stage::COMPONENTS: ok = get_bool(env, v, &m->components); break;
      case Stage::SIMPLIFY: ok = get_mesh_simplify(env, v, &m->simplify, &m->has_simplify); break;
      case Stage::QUADRIC: ok = get_mesh_block(env, v, &m->quadric, MESH_QUADRIC_FIELDS, rm_mesh_quadric_default, &m->has_quadric); break;
      case Stage::OCCLUSION: ok = get_mesh_block(env, v, &m->occlusion, MESH_OCCLUSION_FIELDS, rm_mesh_occlusion_default, &m->has_occlusion); break;
      case Stage::MEASURES: ok = get_bool(env, v, &m->measures); break;
      case Stage::PROJECT: ok = get_mesh_block(env, v, &m->project, MESH_PROJECT_FIELDS, rm_mesh_project_default, &m->has_project); break;
      case Stage::DEVIATION: ok = get_mesh_block(env, v, &m->deviation, MESH_DEVIATION_FIELDS, rm_mesh_deviation_default, &m->has_deviation); break;
    }
    if (!ok) return false;
  }
  return !m->has_quadric || m->has_simplify;
}

// The mesh behind the stages that were given, as { positions, normals | null, colours | null: Float32Array(3 V), triangles: Uint32Array(3 T), cells:
// Uint32Array(V), timings: [sampling, meshing, attributes] in ms (rm_mesh_timings) }; every handle is destroyed as soon as the next one exists, the
// last on the way out.  On the device, in this order: simplify (rm_mesh_simplify, with quadric rm_mesh_simplify_quadric), keep (rm_mesh_filter,
// which also removes the vertices the clustering left without triangles), project (rm_mesh_project: `projection` and `residual`), measures
// (rm_mesh_measure: `measures`); then the arrays are copied, with components `labels`: Uint32Array(V) and `componentSizes`: Uint32Array(2 C)
// (rm_mesh_components); then on the mesh that is returned occlusion (rm_mesh_occlusion: `occlusion`: Float32Array(V), its milliseconds as
// timings[3]) and deviation (rm_mesh_deviation: `deviation` and `triangleDeviation`: Float32Array(T)).
static napi_value mesh_result(napi_env env, rm_ctx* ctx, rm_mesh* mesh, const MeshStages& m) {
  rm_scene* const scene = m.scene;
  struct Guard {  // the handle in hand is destroyed on every way out
    rm_mesh* h;
    ~Guard() { rm_mesh_destroy(h); }
  } guard{mesh};
  const auto napi_failed = [&]() -> napi_value {
    napi_throw_error(env, nullptr, "N-API call failed while the mesh was copied");
    return nullptr;
  };
  if (m.has_simplify) {
    rm_mesh* simplified = nullptr;
    if (m.has_quadric) {
      if (rm_mesh_simplify_quadric(mesh, &m.simplify.clusters, &m.simplify.params, &m.quadric, &simplified) != RM_OK) return throw_rm(env, ctx, "rm_mesh_simplify_quadric");
    } else if (rm_mesh_simplify(mesh, &m.simplify.clusters, &m.simplify.params, &simplified) != RM_OK) return throw_rm(env, ctx, "rm_mesh_simplify");
    rm_mesh_destroy(mesh);
    guard.h = mesh = simplified;
  }
  if (m.has_keep) {
    rm_mesh* filtered = nullptr;
    if (rm_mesh_filter(mesh, &m.keep, &filtered) != RM_OK) return throw_rm(env, ctx, "rm_mesh_filter");
    rm_mesh_destroy(mesh);
    guard.h = mesh = filtered;
  }
  // project (with the scene): behind simplify and keep, that mesh's vertices are projected onto the scene's level set (rm_mesh_project) and
  // everything below sees the projected mesh; `timings` stays the producing mesh's, the projection's milliseconds go into its own object
  float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  rm_mesh_timings(mesh, ms);
  RmMeshProjection projected{};
  float projected_ms = 0.0f;
  napi_value residual = nullptr;
  if (m.has_project) {
    unsigned long long before[2] = {0, 0};
    rm_mesh_counts(mesh, before);
    void* data = nullptr;
    if (!(residual = make_array(env, napi_float32_array, (size_t)before[0], &data))) return napi_failed();
    rm_mesh* moved = nullptr;
    if (rm_mesh_project(mesh, scene, &m.project, &moved, &projected, static_cast<float*>(data)) != RM_OK) return throw_rm(env, ctx, "rm_mesh_project");
    rm_mesh_destroy(mesh);
    guard.h = mesh = moved;
    float slots[3] = {0.0f, 0.0f, 0.0f};
    rm_mesh_timings(mesh, slots);
    projected_ms = slots[1] + slots[2];
  }
  // refine (with the scene): behind the projection, that mesh's chording edges are split (rm_mesh_refine) and everything below sees the refined mesh
  RmMeshRefinement refined{};
  float refined_ms = 0.0f;
  if (m.has_refine) {
    rm_mesh* finer = nullptr;
    if (rm_mesh_refine(mesh, scene, &m.refine, &m.refine_project, &finer, &refined) != RM_OK) return throw_rm(env, ctx, "rm_mesh_refine");
    rm_mesh_destroy(mesh);
    guard.h = mesh = finer;
    float slots[3] = {0.0f, 0.0f, 0.0f};
    rm_mesh_timings(mesh, slots);
    refined_ms = slots[1] + slots[2];
  }
  RmMeshMeasures measured{};
  float measured_ms[2] = {0.0f, 0.0f};
  if (m.measures && rm_mesh_measure(mesh, &measured, measured_ms) != RM_OK) return throw_rm(env, ctx, "rm_mesh_measure");
  unsigned long long counts[2] = {0, 0}, parts = 0;
  rm_mesh_counts(mesh, counts);
  enum { ALWAYS, NORMALS, COLOURS, COMPONENTS };  // when an array is there: with every mesh, or when the call asked for it
  static const struct { const char* name; int what; napi_typedarray_type type; int when, per_vertex, per_triangle, per_part; } ARRAYS[] = {
      {"positions", RM_MESH_POSITIONS, napi_float32_array, ALWAYS, 3, 0, 0},  {"normals", RM_MESH_NORMALS, napi_float32_array, NORMALS, 3, 0, 0},
      {"colours", RM_MESH_COLOURS, napi_float32_array, COLOURS, 3, 0, 0},     {"triangles", RM_MESH_TRIANGLES, napi_uint32_array, ALWAYS, 0, 3, 0},
      {"cells", RM_MESH_CELLS, napi_uint32_array, ALWAYS, 1, 0, 0},           {"labels", RM_MESH_PART_LABELS, napi_uint32_array, COMPONENTS, 1, 0, 0},
      {"componentSizes", RM_MESH_PART_SIZES, napi_uint32_array, COMPONENTS, 0, 0, 2}};
  napi_value o = nullptr;
  if (napi_create_object(env, &o) != napi_ok) return napi_failed();
  for (const auto& a : ARRAYS) {
    napi_value v = nullptr;
    if (a.when == COMPONENTS) {
      if (!m.components) continue;  // (no property at all)
      if (rm_mesh_components(mesh, &parts) != RM_OK) return throw_rm(env, ctx, "rm_mesh_download");  // (labelled once, behind the five arrays)
    }
    if ((a.when == NORMALS && !m.normals) || (a.when == COLOURS && !m.colours)) {
      if (napi_get_null(env, &v) != napi_ok) return napi_failed();  // the mesh was made without this array
    } else {
      const size_t count = (size_t)counts[0] * a.per_vertex + (size_t)counts[1] * a.per_triangle + (size_t)parts * a.per_part;
      void* data = nullptr;
      if (!(v = make_array(env, a.type, count, &data))) return napi_failed();
      const int rc = a.when == COMPONENTS ? rm_mesh_components_download(mesh, a.what, data, count * 4) : rm_mesh_download(mesh, a.what, data, count * 4);
      if (rc != RM_OK) return throw_rm(env, ctx, "rm_mesh_download");
    }
    if (napi_set_named_property(env, o, a.name, v) != napi_ok) return napi_failed();
  }
  if (m.has_project) {  // RmMeshProjection's fields in camel case, the counts as Numbers (all below 2^53), and the milliseconds of the rounds and the normals
    napi_value r = nullptr;
    if (napi_create_object(env, &r) != napi_ok) return napi_failed();
    const Number NUMBERS[] = {
        {"vertices", (double)projected.vertices}, {"triangles", (double)projected.triangles}, {"movedVertices", (double)projected.moved_vertices},
        {"settledBefore", (double)projected.settled_before}, {"settledAfter", (double)projected.settled_after},
        {"nonfiniteBefore", (double)projected.nonfinite_before}, {"nonfiniteAfter", (double)projected.nonfinite_after},
        {"clampedVertices", (double)projected.clamped_vertices}, {"undirectedVertices", (double)projected.undirected_vertices},
        {"flippedTriangles", (double)projected.flipped_triangles}, {"worstBefore", (double)projected.worst_before}, {"worstAfter", (double)projected.worst_after},
        {"meanBefore", projected.mean_before}, {"rmsBefore", projected.rms_before}, {"meanAfter", projected.mean_after}, {"rmsAfter", projected.rms_after},
        {"maxBefore", (double)projected.max_before}, {"maxAfter", (double)projected.max_after}, {"roundsRun", (double)projected.rounds_run},
        {"milliseconds", (double)projected_ms}};
    if (!set_numbers(env, r, NUMBERS) || napi_set_named_property(env, o, "projection", r) != napi_ok || napi_set_named_property(env, o, "residual", residual) != napi_ok) return napi_failed();
  }
  if (m.has_refine) {  // RmMeshRefinement's fields in camel case, the counts as Numbers (all below 2^53), the per-round counts as arrays of eight, and the milliseconds
    napi_value r = nullptr;
    if (napi_create_object(env, &r) != napi_ok) return napi_failed();
    const Number NUMBERS[] = {
        {"verticesBefore", (double)refined.vertices_before}, {"trianglesBefore", (double)refined.triangles_before}, {"vertices", (double)refined.vertices},
        {"triangles", (double)refined.triangles}, {"flippedTriangles", (double)refined.flipped_triangles}, {"maxFirst", (double)refined.max_first},
        {"maxLast", (double)refined.max_last}, {"roundsRun", (double)refined.rounds_run}, {"stopped", (double)refined.stopped}, {"milliseconds", (double)refined_ms}};
    if (!set_numbers(env, r, NUMBERS)) return napi_failed();
    const struct { const char* name; const uint64_t* values; } ROUNDS[] = {{"edges", refined.edges}, {"splitEdges", refined.split_edges}, {"nonfiniteMidpoints", refined.nonfinite_midpoints}};
    for (const auto& rounds : ROUNDS) {
      napi_value a = nullptr, x = nullptr;
      if (napi_create_array_with_length(env, 8, &a) != napi_ok) return napi_failed();
      for (uint32_t k = 0; k < 8; k++)
        if (napi_create_double(env, (double)rounds.values[k], &x) != napi_ok || napi_set_element(env, a, k, x) != napi_ok) return napi_failed();
      if (napi_set_named_property(env, r, rounds.name, a) != napi_ok) return napi_failed();
    }
    if (napi_set_named_property(env, o, "refinement", r) != napi_ok) return napi_failed();
  }
  if (m.has_occlusion) {
    napi_value v = nullptr;
    void* data = nullptr;
    float ms2[2] = {0.0f, 0.0f};
    if (!(v = make_array(env, napi_float32_array, (size_t)counts[0], &data))) return napi_failed();
    if (rm_mesh_occlusion(mesh, scene, &m.occlusion, static_cast<float*>(data), ms2) != RM_OK) return throw_rm(env, ctx, "rm_mesh_occlusion");
    if (napi_set_named_property(env, o, "occlusion", v) != napi_ok) return napi_failed();
    ms[3] = ms2[0] + ms2[1];
  }
  if (m.has_deviation) {  // RmMeshDeviationReport's fields in camel case, the counts as Numbers (all below 2^53), the milliseconds of both spans; max_t per triangle
    napi_value r = nullptr, worst = nullptr;
    void* data = nullptr;
    RmMeshDeviationReport report{};
    float ms2[2] = {0.0f, 0.0f};
    if (!(worst = make_array(env, napi_float32_array, (size_t)counts[1], &data))) return napi_failed();
    if (rm_mesh_deviation(mesh, scene, &m.deviation, &report, static_cast<float*>(data), ms2) != RM_OK) return throw_rm(env, ctx, "rm_mesh_deviation");
    if (napi_create_object(env, &r) != napi_ok) return napi_failed();
    const Number NUMBERS[] = {
        {"vertices", (double)report.vertices}, {"triangles", (double)report.triangles}, {"skippedTriangles", (double)report.skipped_triangles},
        {"unevaluatedTriangles", (double)report.unevaluated_triangles}, {"nonfiniteSamples", (double)report.nonfinite_samples},
        {"overTriangles", (double)report.over_triangles}, {"worstTriangle", (double)report.worst_triangle}, {"area", report.area},
        {"overArea", report.over_area}, {"meanSigned", report.mean_signed}, {"rms", report.rms}, {"max", (double)report.max},
        {"samples", (double)report.samples}, {"milliseconds", (double)(ms2[0] + ms2[1])}};
    if (!set_numbers(env, r, NUMBERS) || napi_set_named_property(env, o, "deviation", r) != napi_ok || napi_set_named_property(env, o, "triangleDeviation", worst) != napi_ok) return napi_failed();
  }
  napi_value timings = float_array(env, ms, m.has_occlusion ? 4u : 3u);
  if (!timings || napi_set_named_property(env, o, "timings", timings) != napi_ok) return napi_failed();
  if (m.measures) {
    bool rm_failed = false;
    napi_value v = measures_object(env, measured, measured_ms, mesh, &rm_failed);
    if (!v) return rm_failed ? throw_rm(env, ctx, "rm_mesh_measure_components") : napi_failed();
    if (napi_set_named_property(env, o, "measures", v) != napi_ok) return napi_failed();
  }
  return o;
}

// The four mesh entries: each checks its argument count, parses its own leading arguments and then the stages (get_mesh_stages), extracts, and
// hands the mesh to mesh_result.
// extractMesh(ctx, scene, grid, params | null[, sharp | null[, keep | null[, components[, simplify | null[, quadric | null[, occlusion | null[, measures[,
// project | null[, deviation | null]]]]]]]]]) = rm_mesh_extract, or with a sharp block rm_mesh_extract_sharp
// extractMeshSlabs(ctx, scene, grid, slabs | null, params | null, sharp | null, keep | null, components, simplify | null, quadric | null, occlusion | null,
// measures[, project | null[, deviation | null]]) = rm_mesh_extract_slabs / rm_mesh_extract_sharp_slabs: the first twelve arguments are all given
static napi_value extract_common(napi_env env, napi_callback_info info, bool slabbed, bool with_refine = false) {
  size_t argc = 16;
  napi_value argv[16];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const bool counted = with_refine ? argc == 15 : slabbed ? argc >= 12 && argc <= 14 : argc >= 4 && argc <= 13;
  rm_ctx* ctx = counted ? get_external<rm_ctx>(env, argv[0]) : nullptr;
  MeshStages m;
  m.scene = counted ? get_external<rm_scene>(env, argv[1]) : nullptr;
  RmGrid g;
  RmMeshSlabs w;
  RmMeshParams p;
  if (with_refine) {
    napi_value inner = nullptr;
    bool has_inner = false;
    if (!ctx || !m.scene || !get_grid(env, argv[2], &g) || !get_mesh_block(env, argv[3], &m.refine, MESH_REFINE_FIELDS, rm_mesh_refine_default, &m.has_refine) || !m.has_refine ||
        napi_get_named_property(env, argv[3], "project", &inner) != napi_ok ||
        !get_mesh_block(env, inner, &m.refine_project, MESH_PROJECT_FIELDS, rm_mesh_project_default, &has_inner) || !has_inner ||
        !get_mesh_block(env, argv[4], &w, MESH_SLABS_FIELDS, rm_mesh_slabs_default, &slabbed) || !get_mesh_block(env, argv[5], &p, MESH_FIELDS, rm_mesh_params_default) ||
        !get_mesh_stages(env, argv, 6, SCENE_STAGES, &m)) {
      napi_throw_type_error(env, nullptr, "extractMeshRefined(ctx, scene, grid, refine, slabs | null, params | null, sharp | null, keep | null, components, simplify | null, quadric | null, occlusion | null, measures, project | null, deviation | null)");
      return nullptr;
    }
  }
  const size_t at = slabbed ? 4 : 3;  // where the parameters stand: behind the slabs block, or behind the grid
  if (!with_refine &&
      (!ctx || !m.scene || !get_grid(env, argv[2], &g) || (slabbed && !get_mesh_block(env, argv[3], &w, MESH_SLABS_FIELDS, rm_mesh_slabs_default)) ||
      !get_mesh_block(env, argv[at], &p, MESH_FIELDS, rm_mesh_params_default) || !get_mesh_stages(env, argv, at + 1, SCENE_STAGES, &m))) {
    napi_throw_type_error(env, nullptr, slabbed ? "extractMeshSlabs(ctx, scene, grid, slabs | null, params | null, sharp | null, keep | null, components, simplify | null, quadric | null, occlusion | null, measures[, project | null[, deviation | null]])"
                                                : "extractMesh(ctx, scene, grid, params | null[, sharp | null[, keep | null[, components[, simplify | null[, quadric | null[, occlusion | null[, measures[, project | null[, deviation | null]]]]]]]]])");
    return nullptr;
  }
  m.normals = p.normals != 0;
  m.colours = p.colours != 0;
  rm_mesh* mesh = nullptr;
  if (slabbed) {
    if (m.has_sharp) {
      if (rm_mesh_extract_sharp_slabs(ctx, m.scene, &g, &p, &m.sharp, &w, &mesh) != RM_OK) return throw_rm(env, ctx, "rm_mesh_extract_sharp_slabs");
    } else if (rm_mesh_extract_slabs(ctx, m.scene, &g, &p, &w, &mesh) != RM_OK) return throw_rm(env, ctx, "rm_mesh_extract_slabs");
  } else if (m.has_sharp) {
    if (rm_mesh_extract_sharp(ctx, m.scene, &g, &p, &m.sharp, &mesh) != RM_OK) return throw_rm(env, ctx, "rm_mesh_extract_sharp");
  } else if (rm_mesh_extract(ctx, m.scene, &g, &p, &mesh) != RM_OK) return throw_rm(env, ctx, "rm_mesh_extract");
  return mesh_result(env, ctx, mesh, m);
}
// with_refine: extractMeshRefined(ctx, scene, grid, refine, slabs | null, params | null, sharp | null, keep | null, components, simplify | null, quadric | null,
// occlusion | null, measures, project | null, deviation | null): all fifteen arguments are given; refine is the block's fields and `project`, the block of the
// projection inside its rounds; slabs an object = the slabbed extraction
static napi_value ExtractMesh(napi_env env, napi_callback_info info) { return extract_common(env, info, false); }
static napi_value ExtractMeshSlabs(napi_env env, napi_callback_info info) { return extract_common(env, info, true); }
static napi_value ExtractMeshRefined(napi_env env, napi_callback_info info) { return extract_common(env, info, false, true); }

// meshFromValues(ctx, grid, values: Float32Array(corners), iso[, keep | null[, components[, simplify | null[, quadric | null[, measures]]]]]) = rm_mesh_from_values
// meshFromValuesSlabs(ctx, grid, values, iso, slabs | null, keep | null, components, simplify | null, quadric | null, measures) = rm_mesh_from_values_slabs:
// every argument is given
static napi_value values_common(napi_env env, napi_callback_info info, bool slabbed) {
  size_t argc = 10;
  napi_value argv[10];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = (slabbed ? argc == 10 : argc >= 4 && argc <= 9) ? get_external<rm_ctx>(env, argv[0]) : nullptr;
  MeshStages m;
  RmGrid g;
  RmMeshSlabs w;
  double iso = 0.0;
  void* d = nullptr;
  size_t n = 0;
  if (!ctx || !get_grid(env, argv[1], &g) || !get_buffer(env, argv[2], &d, &n) || napi_get_value_double(env, argv[3], &iso) != napi_ok ||
      (slabbed && !get_mesh_block(env, argv[4], &w, MESH_SLABS_FIELDS, rm_mesh_slabs_default)) || !get_mesh_stages(env, argv, slabbed ? 5 : 4, VALUES_STAGES, &m)) {
    napi_throw_type_error(env, nullptr, slabbed ? "meshFromValuesSlabs(ctx, grid, values: Float32Array, iso, slabs | null, keep | null, components, simplify | null, quadric | null, measures)"
                                                : "meshFromValues(ctx, grid, values: Float32Array, iso[, keep | null[, components[, simplify | null[, quadric | null[, measures]]]]])");
    return nullptr;
  }
  // the size below needs sane counts: the whole grid is checked where 2^28 corners bound it, the counts alone where slabs lift that bound (the
  // library checks the rest of such a grid)
  float probe[1025];
  if (!slabbed) {
    if (rm_grid_axis(&g, 0, probe) != RM_OK) return throw_rm(env, nullptr, "rm_mesh_from_values");
  } else if (g.n[0] < 1 || g.n[0] > 1024 || g.n[1] < 1 || g.n[1] > 1024 || g.n[2] < 1 || g.n[2] > 1024) {
    napi_throw_range_error(env, nullptr, "meshFromValuesSlabs: grid n must be in 1..1024 cells per axis");
    return nullptr;
  }
  if (n !=(size_t)(g.n[0] + 1) * (size_t)(g.n[1] + 1) * (size_t)(g.n[2] + 1) * sizeof(float)) {
    napi_throw_range_error(env, nullptr, slabbed ? "meshFromValuesSlabs: values must hold (nx + 1)(ny + 1)(nz + 1) floats" : "meshFromValues: values must hold (nx + 1)(ny + 1)(nz + 1) floats");
    return nullptr;
  }
  rm_mesh* mesh = nullptr;
  if (slabbed) {
    if (rm_mesh_from_values_slabs(ctx, &g, static_cast<const float*>(d), (float)iso, &w, &mesh) != RM_OK) return throw_rm(env, ctx, "rm_mesh_from_values_slabs");
  } else if (rm_mesh_from_values(ctx, &g, static_cast<const float*>(d), (float)iso, &mesh) != RM_OK) return throw_rm(env, ctx, "rm_mesh_from_values");
  return mesh_result(env, ctx, mesh, m);
}
static napi_value MeshFromValues(napi_env env, napi_callback_info info) { return values_common(env, info, false); }
static napi_value MeshFromValuesSlabs(napi_env env, napi_callback_info info) { return values_common(env, info, true); }

// fbCreateStriped(ctx, width, height, stripeRows, parts, part[, gbuffer]): the stripes k with k % parts == part of a width x height image,
// planes owned by the library (rm_fb_create_striped) -- what one GPU of a sharded frame holds
static napi_value FbCreateStriped(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  if (!ctx || argc < 6) {
    napi_throw_type_error(env, nullptr, "fbCreateStriped(ctx, width, height, stripeRows, parts, part[, gbuffer])");
    return nullptr;
  }
  int32_t v[6] = {0, 0, 0, 0, 0, RM_GBUFFER_F32};
  for (int i = 0; i < 6 && 1 + i < (int)argc; i++) napi_get_value_int32(env, argv[1 + i], &v[i]);
  rm_fb* fb = nullptr;
  if (rm_fb_create_striped_fmt(ctx, v[0], v[1], v[2], v[3], v[4], nullptr, nullptr, nullptr, v[5], &fb) != RM_OK) return throw_rm(env, ctx, "rm_fb_create_striped");
  return make_external(env, fb);
}

// fbRows(fb): image rows the framebuffer holds
static napi_value FbRows(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_fb* fb = get_external<rm_fb>(env, argv[0]);
  if (!fb) {
    napi_throw_type_error(env, nullptr, "fbRows(fb): not a framebuffer handle");
    return nullptr;
  }
  NAPI_OK(napi_create_int32(env, rm_fb_rows(fb), &out));
  return out;
}

// setSamplesInFlight(ctx, n): rm_ctx_set_samples_in_flight
static napi_value SetSamplesInFlight(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  int32_t n = 1;
  if (argc > 1) napi_get_value_int32(env, argv[1], &n);
  if (!ctx) {
    napi_throw_type_error(env, nullptr, "setSamplesInFlight(ctx, n): not a context handle");
    return nullptr;
  }
  if (rm_ctx_set_samples_in_flight(ctx, n) != RM_OK) return throw_rm(env, ctx, "rm_ctx_set_samples_in_flight");
  return nullptr;
}

// The present of a frame whose stripes this process renders on several GPUs (part p on ctxs[p]); RGBA8, row 0 = bottom.
//   presentSharded(ctxs: ctx[], fbs: fb[], samples, dof: boolean, out: Uint8Array(width * height * 4)) = rm_present_sharded
//   presentShardedStart(ctxs, fbs, samples, dof)   = rm_present_sharded_start: snapshot and send, returns at once
//   presentShardedFinish(ctxs, out: Uint8Array)     = rm_present_sharded_finish: the canvas of the present that was started
static bool handle_arrays(napi_env env, napi_value a_ctxs, napi_value a_fbs, rm_ctx** ctxs, rm_fb** fbs, uint32_t* count, const char* who) {
  uint32_t n = 0, m = 0;
  bool is_a = false, is_b = true;
  if (napi_is_array(env, a_ctxs, &is_a) != napi_ok || !is_a || napi_get_array_length(env, a_ctxs, &n) != napi_ok || n == 0 || n > 64 ||
      (fbs && (napi_is_array(env, a_fbs, &is_b) != napi_ok || !is_b || napi_get_array_length(env, a_fbs, &m) != napi_ok || n != m))) {
    napi_throw_type_error(env, nullptr, (std::string(who) + ": ctxs (and fbs) must be arrays of the same length (1..64)").c_str());
    return false;
  }
  for (uint32_t i = 0; i < n; i++) {
    napi_value a, b;
    if (napi_get_element(env, a_ctxs, i, &a) != napi_ok) return false;
    ctxs[i] = get_external<rm_ctx>(env, a);
    if (fbs) {
      if (napi_get_element(env, a_fbs, i, &b) != napi_ok) return false;
      fbs[i] = get_external<rm_fb>(env, b);
    }
    if (!ctxs[i] || (fbs && !fbs[i])) {
      napi_throw_type_error(env, nullptr, (std::string(who) + ": wrong or destroyed handle in ctxs / fbs").c_str());
      return false;
    }
  }
  *count = n;
  return true;
}

static napi_value PresentShardedImpl(napi_env env, napi_callback_info info, bool start, bool finish) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const char* who = start && finish ? "presentSharded" : start ? "presentShardedStart" : "presentShardedFinish";
  const size_t need = start && finish ? 5 : start ? 4 : 2;
  if (argc < need) {
    napi_throw_type_error(env, nullptr, (std::string(who) + ": too few arguments").c_str());
    return nullptr;
  }
  rm_ctx* ctxs[64];
  rm_fb* fbs[64];
  uint32_t n = 0;
  if (!handle_arrays(env, argv[0], start ? argv[1] : nullptr, ctxs, start ? fbs : nullptr, &n, who)) return nullptr;
  void* d = nullptr;
  size_t len = 0;
  if (finish && !get_buffer(env, argv[start ? 4 : 1], &d, &len)) {
    napi_throw_type_error(env, nullptr, (std::string(who) + ": out must be a Uint8Array").c_str());
    return nullptr;
  }
  if (start && finish && len < (size_t)rm_fb_width(fbs[0]) * (size_t)rm_fb_height(fbs[0]) * 4) {
    napi_throw_range_error(env, nullptr, "presentSharded: out is smaller than width * height * 4 bytes");
    return nullptr;
  }
  if (start) {
    int32_t samples = 1;
    napi_get_value_int32(env, argv[2], &samples);
    bool dof = false;
    napi_get_value_bool(env, argv[3], &dof);
    if (rm_present_sharded_start(ctxs, fbs, (int)n, samples, dof ? 1 : 0) != RM_OK) return throw_rm(env, ctxs[0], "rm_present_sharded_start");
  }
  // (presentShardedFinish: the library knows the canvas of the pending present and refuses a smaller `out`, leaving the present pending)
  if (finish && rm_present_sharded_finish(ctxs, (int)n, static_cast<uint8_t*>(d), len) != RM_OK) return throw_rm(env, ctxs[0], "rm_present_sharded_finish");
  return nullptr;
}
static napi_value PresentSharded(napi_env env, napi_callback_info info) { return PresentShardedImpl(env, info, true, true); }
static napi_value PresentShardedStart(napi_env env, napi_callback_info info) { return PresentShardedImpl(env, info, true, false); }
static napi_value PresentShardedFinish(napi_env env, napi_callback_info info) { return PresentShardedImpl(env, info, false, true); }

// renderSample(ctx, scene, fb, uniforms: ArrayBuffer(sizeof RmUniforms), tile: Int32Array(4) | null, flags)
static napi_value RenderSample(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  rm_scene* scene = get_external<rm_scene>(env, argv[1]);
  rm_fb* fb = get_external<rm_fb>(env, argv[2]);
  void* u = nullptr;
  size_t un = 0;
  if (!ctx || !scene || !fb) {
    napi_throw_type_error(env, nullptr, "renderSample(ctx, scene, fb, ...): wrong or destroyed handle");
    return nullptr;
  }
  if (!get_buffer(env, argv[3], &u, &un) || un != sizeof(RmUniforms)) {
    napi_throw_type_error(env, nullptr, "renderSample: uniforms must be an ArrayBuffer of sizeof(RmUniforms) bytes");
    return nullptr;
  }
  RmRect tile;
  const RmRect* tp = nullptr;
  void* t = nullptr;
  size_t tn = 0;
  if (argc > 4 && get_buffer(env, argv[4], &t, &tn) && tn == sizeof(RmRect)) {
    std::memcpy(&tile, t, sizeof tile);
    tp = &tile;
  }
  int32_t flags = 0;
  if (argc > 5) napi_get_value_int32(env, argv[5], &flags);
  if (rm_render_sample(ctx, scene, fb, static_cast<const RmUniforms*>(u), tp, flags) != RM_OK) return throw_rm(env, ctx, "rm_render_sample");
  return nullptr;
}

// renderSamples(ctx, scene, fb, uniforms: ArrayBuffer(sizeof RmUniforms), randNoise: Float32Array(2 * count), tile: Int32Array(4) | null, flags)
// = rm_render_samples: the samples between two yields of a job in one call (RenderJobExecutor.tsx:160-222)
static napi_value RenderSamples(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  rm_ctx* ctx = get_external<rm_ctx>(env, argv[0]);
  rm_scene* scene = get_external<rm_scene>(env, argv[1]);
  rm_fb* fb = get_external<rm_fb>(env, argv[2]);
  void* u = nullptr;
  size_t un = 0;
  if (!ctx || !scene || !fb) {
    napi_throw_type_error(env, nullptr, "renderSamples(ctx, scene, fb, ...): wrong or destroyed handle");
    return nullptr;
  }
  if (!get_buffer(env, argv[3], &u, &un) || un != sizeof(RmUniforms)) {
    napi_throw_type_error(env, nullptr, "renderSamples: uniforms must be an ArrayBuffer of sizeof(RmUniforms) bytes");
    return nullptr;
  }
  void* rn = nullptr;
  size_t rnn = 0;
  if (!get_buffer(env, argv[4], &rn, &rnn) || rnn % (2 * sizeof(float)) != 0 || rnn > (size_t)1 << 24) {
    napi_throw_type_error(env, nullptr, "renderSamples: randNoise must be a Float32Array of 2 * count values");
    return nullptr;
  }
  RmRect tile;
  const RmRect* tp = nullptr;
  void* t = nullptr;
  size_t tn = 0;
  if (argc > 5 && get_buffer(env, argv[5], &t, &tn) && tn == sizeof(RmRect)) {
    std::memcpy(&tile, t, sizeof tile);
    tp = &tile;
  }
  int32_t flags = 0;
  if (argc > 6) napi_get_value_int32(env, argv[6], &flags);
  if (rm_render_samples(ctx, scene, fb, static_cast<const RmUniforms*>(u), static_cast<const float*>(rn), (int)(rnn / (2 * sizeof(float))), tp, flags) != RM_OK)
    return throw_rm(env, ctx, "rm_render_samples");
  return nullptr;
}

static napi_value Sizes(napi_env env, napi_callback_info) {
  napi_value o, v;
  NAPI_OK(napi_create_object(env, &o));
  const struct { const char* k; uint32_t v; } items[] = {
      {"RmUniforms", (uint32_t)sizeof(RmUniforms)}, {"RmSceneDesc", (uint32_t)sizeof(RmSceneDesc)}, {"RmPrim", (uint32_t)sizeof(RmPrim)},
      {"RmMaterial", (uint32_t)sizeof(RmMaterial)}, {"RmRect", (uint32_t)sizeof(RmRect)}, {"RmSurface", (uint32_t)sizeof(RmSurface)}, {"RmDenoise", (uint32_t)sizeof(RmDenoise)},
      {"RmDenoiseVariance", (uint32_t)sizeof(RmDenoiseVariance)}, {"RmDespeckle", (uint32_t)sizeof(RmDespeckle)}, {"RmFilters", (uint32_t)sizeof(RmFilters)}, {"RmFrameStats", (uint32_t)sizeof(RmFrameStats)},
      {"RmAutoExposure", (uint32_t)sizeof(RmAutoExposure)}, {"RmDisplay", (uint32_t)sizeof(RmDisplay)}, {"RmGrid", (uint32_t)sizeof(RmGrid)},
      {"RmMeshParams", (uint32_t)sizeof(RmMeshParams)}, {"RmMeshSharp", (uint32_t)sizeof(RmMeshSharp)}, {"RmMeshKeep", (uint32_t)sizeof(RmMeshKeep)}, {"RmMeshSimplify", (uint32_t)sizeof(RmMeshSimplify)}, {"RmMeshQuadric", (uint32_t)sizeof(RmMeshQuadric)}, {"RmMeshOcclusion", (uint32_t)sizeof(RmMeshOcclusion)}, {"RmMeshMeasures", (uint32_t)sizeof(RmMeshMeasures)}, {"RmMeshSlabs", (uint32_t)sizeof(RmMeshSlabs)}, {"RmMeshProject", (uint32_t)sizeof(RmMeshProject)}, {"RmMeshProjection", (uint32_t)sizeof(RmMeshProjection)}, {"RmMeshDeviation", (uint32_t)sizeof(RmMeshDeviation)}, {"RmMeshDeviationReport", (uint32_t)sizeof(RmMeshDeviationReport)}, {"RmMeshRefine", (uint32_t)sizeof(RmMeshRefine)}, {"RmMeshRefinement", (uint32_t)sizeof(RmMeshRefinement)}, {"abi", (uint32_t)rm_abi_version()}};
  for (const auto& it : items) {
    NAPI_OK(napi_create_uint32(env, it.v, &v));
    NAPI_OK(napi_set_named_property(env, o, it.k, v));
  }
  return o;
}

static napi_value Init(napi_env env, napi_value exports) {
  const struct { const char* name; napi_callback fn; } fns[] = {
      {"ctxCreate", CtxCreate}, {"ctxDestroy", CtxDestroy}, {"sync", Sync}, {"sceneCreate", SceneCreate}, {"sceneDestroy", SceneDestroy},
      {"fbCreate", FbCreate}, {"fbClear", FbClear}, {"fbDestroy", FbDestroy}, {"fbDownload", FbDownload}, {"present", Present}, {"denoise", Denoise}, {"presentDenoised", PresentDenoised}, {"denoiseVariance", DenoiseVariance}, {"presentDenoisedVariance", PresentDenoisedVariance}, {"filter", Filter}, {"presentFiltered", PresentFiltered}, {"presentDisplay", PresentDisplay}, {"presentLinear", PresentLinear}, {"frameStats", FrameStats}, {"statsExposure", StatsExposure}, {"statsPercentile", StatsPercentile}, {"renderSample", RenderSample}, {"renderSamples", RenderSamples},
      {"fbCreateStriped", FbCreateStriped}, {"fbRows", FbRows}, {"setSamplesInFlight", SetSamplesInFlight}, {"presentSharded", PresentSharded}, {"presentShardedStart", PresentShardedStart}, {"presentShardedFinish", PresentShardedFinish},
      {"meshBlocks", MeshBlocks}, {"meshSharpBlock", MeshSharpBlock}, {"meshKeepBlock", MeshKeepBlock}, {"meshSimplifyBlock", MeshSimplifyBlockOf}, {"meshQuadricBlock", MeshQuadricBlock}, {"meshOcclusionBlock", MeshOcclusionBlock}, {"meshProjectBlock", MeshProjectBlock}, {"meshDeviationBlock", MeshDeviationBlock}, {"meshRefineBlock", MeshRefineBlock}, {"extractMeshRefined", ExtractMeshRefined}, {"sdfGrid", SdfGrid}, {"extractMesh", ExtractMesh}, {"meshFromValues", MeshFromValues}, {"meshSlabsBlock", MeshSlabsBlock}, {"extractMeshSlabs", ExtractMeshSlabs}, {"meshFromValuesSlabs", MeshFromValuesSlabs}, {"sizes", Sizes}};
  for (const auto& f : fns) {
    napi_value fn;
    if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &fn) != napi_ok) return nullptr;
    if (napi_set_named_property(env, exports, f.name, fn) != napi_ok) return nullptr;
  }
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
