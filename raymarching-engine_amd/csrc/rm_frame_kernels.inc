// rm_frame_kernels.inc -- the small memory-bound kernels around the pixel kernel: the blend of staged samples (rm_combine_kernel),
// the present pass (display.frag: rm_present*), the assembly of gathered stripes.  One copy, in the parity TU (and one in the GL
// stack's arithmetic, whose canvas conversion differs).  Until round 5 these lived at the end of rm_wavefront.inc; the wavefront
// pipeline is now compiled into the tests' cross-check build only (rm_api.hip), these are the product's.
namespace rm {

#if !RM_BUILD_FAST
// ---- assemble: gathered striped windows -> the frame in image order (rm_assemble_striped) ----------------
// Rows are opaque bytes (float4 colour, or RGBA8 after the per-rank present): V = the widest vector the row length allows.
// These small memory-bound kernels (assemble, combine, present of a window) run NEXT TO the render kernels of the
// following samples, whose long workgroups hold every wave slot of the chip: a grid of thousands of tiny workgroups
// then waits for slots one by one (8 640 workgroups of one 4 KB row piece each took ~0.8 ms to get through, and
// frame n + 1's gather waits for frame n's assembly).  So: at most RM_SMALL_GRID workgroups, each looping.
#define RM_SMALL_GRID 512
template <class V>
__global__ __launch_bounds__(256) void rm_assemble_kernel(const V* src, int parts, int max_rows, int row_elems, int H, int stripe_rows, V* dst) {
  const long long total = (long long)row_elems * H;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / row_elems), x = (int)(i % row_elems);  // y = image row
    const int stripe = y / stripe_rows, part = stripe % parts;
    const int local = (stripe / parts) * stripe_rows + y % stripe_rows;  // row of that part's packed window (rm_global_row inverted)
    dst[i] = src[((size_t)part * max_rows + local) * row_elems + x];
  }
}

static int small_grid(long long items) {
  const long long g = (items + 255) / 256;
  return (int)(g < RM_SMALL_GRID ? (g < 1 ? 1 : g) : RM_SMALL_GRID);
}

hipError_t launch_assemble(const void* src, int parts, int max_rows, long long row_bytes, int H, int stripe_rows, void* dst, hipStream_t stream) {
  if (row_bytes % 16 == 0) {
    const int n = (int)(row_bytes / 16);
    hipLaunchKernelGGL(rm_assemble_kernel<float4>, dim3(small_grid((long long)n * H)), dim3(256), 0, stream, static_cast<const float4*>(src), parts, max_rows, n, H, stripe_rows, static_cast<float4*>(dst));
  } else {
    const int n = (int)(row_bytes / 4);
    hipLaunchKernelGGL(rm_assemble_kernel<unsigned int>, dim3(small_grid((long long)n * H)), dim3(256), 0, stream, static_cast<const unsigned int*>(src), parts, max_rows, n, H, stripe_rows, static_cast<unsigned int*>(dst));
  }
  return hipGetLastError();
}

// ---- combine: the blend of staged samples into the planes (raymarcher.frag:350-351, :379-387) ----------
// Exactly the operations the pixel kernel performs when it blends itself, on the values it staged
// (KParams::stage), so a staged sample leaves the same bits in the planes; the samples of a batch
// (KParams::batch) are blended one after the other, in sample order, as separate launches would.
// MOMENTS: also the moments plane (RM_FB_MOMENTS, KParams::moments), by the colour's rule, on l = the luminance of the staged
// colour in the order include/hip_raymarch.h states (this TU is contract-off: every product and sum is rounded on its own).
template <bool MOMENTS>
__device__ inline void rm_combine(const KParams& P) {
  const long long total = (long long)P.tw * P.th;
  const RmUniforms& u = P.u;
  const int samples = P.batch > 1 ? P.batch : 1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % P.tw), y = (int)(i / P.tw);
    const size_t pix = (size_t)(P.ty + y) * (size_t)P.W + (size_t)(P.tx + x);
    float4 col = P.color[pix];
    float2 mo;
    if (MOMENTS) mo = P.moments[pix];
    for (int k = 0; k < samples; k++) {
      const float4 s = P.stage[(long long)k * 3ll * P.stage_stride + i], prev = col;  // staged tile-compact: pixel i of the tile
      if (u.blendMode == 0) {
        const float f = u.blendWithPreviousFactor;
        col = make_float4(gmix<PM>(s.x, prev.x, f), gmix<PM>(s.y, prev.y, f), gmix<PM>(s.z, prev.z, f), gmix<PM>(1.0f, prev.w, f));
      } else {
        col = make_float4(s.x + prev.x, s.y + prev.y, s.z + prev.z, 1.0f + prev.w);
      }
      if (MOMENTS) {
        const float l = (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z, l2 = l * l;
        if (u.blendMode == 0) {
          const float f = u.blendWithPreviousFactor;
          mo = make_float2(gmix<PM>(l, mo.x, f), gmix<PM>(l2, mo.y, f));
        } else {
          mo = make_float2(mo.x + l, mo.y + l2);
        }
      }
    }
    P.color[pix] = col;
    if (MOMENTS) P.moments[pix] = mo;
    if (P.normal_dof != nullptr && P.gbuffer_half) {  // RGBA16F: rounded to half after EVERY sample, as separate draws would
      rm_half4* const hn = reinterpret_cast<rm_half4*>(P.normal_dof);
      rm_half4* const ha = reinterpret_cast<rm_half4*>(P.albedo_depth);
      rm_half4 qn = hn[pix], qa = ha[pix];
      for (int k = 0; k < samples; k++) {
        const float4* st = P.stage + (long long)k * 3ll * P.stage_stride;
        const float4 n = st[P.stage_stride + i], a = st[2 * P.stage_stride + i];
        const float4 pn = rm_widen(qn), pa = rm_widen(qa);
        qn = rm_narrow(make_float4(pn.x + n.x, pn.y + n.y, pn.z + n.z, pn.w + n.w));
        qa = rm_narrow(make_float4(pa.x + a.x, pa.y + a.y, pa.z + a.z, pa.w + a.w));
      }
      hn[pix] = qn;
      ha[pix] = qa;
    } else if (P.normal_dof != nullptr) {
      float4 pn = P.normal_dof[pix], pa = P.albedo_depth[pix];
      for (int k = 0; k < samples; k++) {
        const float4* st = P.stage + (long long)k * 3ll * P.stage_stride;
        const float4 n = st[P.stage_stride + i], a = st[2 * P.stage_stride + i];
        pn = make_float4(pn.x + n.x, pn.y + n.y, pn.z + n.z, pn.w + n.w);
        pa = make_float4(pa.x + a.x, pa.y + a.y, pa.z + a.z, pa.w + a.w);
      }
      P.normal_dof[pix] = pn;
      P.albedo_depth[pix] = pa;
    }
  }
}

__global__ __launch_bounds__(256) void rm_combine_kernel(const KParams P) { rm_combine<false>(P); }
__global__ __launch_bounds__(256) void rm_combine_moments_kernel(const KParams P) { rm_combine<true>(P); }

hipError_t launch_combine(const KParams& P, hipStream_t stream) {
  if (P.moments) hipLaunchKernelGGL(rm_combine_moments_kernel, dim3(small_grid((long long)P.tw * P.th)), dim3(256), 0, stream, P);
  else hipLaunchKernelGGL(rm_combine_kernel, dim3(small_grid((long long)P.tw * P.th)), dim3(256), 0, stream, P);
  return hipGetLastError();
}

// ---- present pass: client/public/shader/display.frag:16-64 ---------------------------------
// One thread per output pixel: DoF-radius driven Gaussian blur of the accumulated colour
// (NEAREST + REPEAT taps like the reference's textures), x 1/samples, gamma 1/2.2, RGBA8.
// A pixel's blur reaches up to 16 pixels to every side (up to 33 x 33 taps): a 16x16-pixel workgroup first finds
// the largest radius among its pixels and, if that is not 0, stages the colours it can reach -- its tile plus a halo
// of that radius + 1, wrapped at the image borders like the taps -- in LDS (at most 50 x 50 x 12 B = 30 KB); the
// taps are the same taps in the same order with the same arithmetic, read from LDS (a tap outside the staged
// rectangle, which rounding could only produce at its very rim, is read from memory).  Without depth of field every
// radius is 0, the one tap is the pixel itself and nothing is staged.
#define RM_PRESENT_HALO 17
// Round 4: the same pass for ONE PART of a striped frame (STRIPED): the workgroup's tile is TY rows of one stripe (TY divides the
// stripe's rows, TX = 256 / TY columns), the taps come from the whole frame in image order (`color` / `normal_dof`: the gathered
// planes) and the result goes to the part's packed rows -- so that with depth of field on every GPU blurs the stripes it holds
// instead of one GPU blurring the whole frame (display.frag:44-55 reads up to 16 rows either side of a pixel: other GPUs' rows).
// The same taps in the same order with the same arithmetic: the bytes of the whole-frame pass (TY = 1: nothing is staged).
// ND: the element of the normal_dof plane -- float4, or rm_half4 for a framebuffer with the half G-buffer (its .w widened exactly).
__device__ inline float dof_of(const float4& v) { return v.w; }
__device__ inline float dof_of(const rm_half4& v) { return rm_widen(v).w; }

// present_blur: the pass up to display.frag's pow -- v = a / count * brightness per channel and `at` = the pixel's index in the
// output; false for a thread outside the image (after the workgroup's barriers).  rm_present_kernel ends it in pow and RGBA8,
// rm_display_pass_kernel (below) in the display transform.
template <int TY, bool STRIPED, class ND>
RM_DEV bool present_blur(const float4* color, const ND* normal_dof, int W, int H, float brightness, int stripe_rows, int parts, int part, int local_rows,
                         float (&v)[3], size_t& at) {
  constexpr int TX = 256 / TY;
  constexpr int SPAN_X = TX + 2 * RM_PRESENT_HALO, SPAN_Y = TY + 2 * RM_PRESENT_HALO;
  __shared__ float tile[TY > 1 ? SPAN_X * SPAN_Y * 3 : 1];
  __shared__ int wg_reach;
  const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
  const int x = blockIdx.x * TX + lx;
  const int row0_local = blockIdx.y * TY;  // the tile's first row: of the image, or of the part's packed rows
  const int row0 = STRIPED ? ((row0_local / stripe_rows) * parts + part) * stripe_rows + row0_local % stripe_rows : row0_local;  // rm_global_row
  const int y = row0 + ly;
  const bool inside = x < W && (STRIPED ? row0_local + ly < local_rows : y < H);
  const float dof = (inside && normal_dof) ? dof_of(normal_dof[(size_t)y * W + x]) * brightness : 0.0f;
  const float kernel = gclamp(dof * 200.0f, 0.0f, 16.0f);
  if (threadIdx.x == 0) wg_reach = 0;
  __syncthreads();
  if (TY > 1 && kernel > 0.0f) atomicMax(&wg_reach, (int)ceilf(kernel) + 1);
  __syncthreads();
  const int reach = wg_reach;                                  // pixels to every side that a tap of this tile can reach
  const int span_x = TX + 2 * reach, span_y = TY + 2 * reach;  // staged rectangle
  const int x0 = (int)blockIdx.x * TX - reach, y0 = row0 - reach;
  if (reach > 0) {
    for (int i = threadIdx.x; i < span_x * span_y; i += 256) {
      int gx = (x0 + i % span_x) % W, gy = (y0 + i / span_x) % H;
      gx += gx < 0 ? W : 0;
      gy += gy < 0 ? H : 0;
      const float4 c = color[(size_t)gy * W + gx];
      tile[3 * i] = c.x; tile[3 * i + 1] = c.y; tile[3 * i + 2] = c.z;
    }
    __syncthreads();
  }
  if (!inside) return false;
  const float tcx = ((float)x + 0.5f) / (float)W, tcy = ((float)y + 0.5f) / (float)H;
  const float sigma = gmax(kernel, 1.0f) * 0.3f;
  float ax = 0.0f, ay = 0.0f, az = 0.0f, count = 0.0f;
  for (float oy = -kernel; oy <= kernel; oy += 1.0f) {
    float ty = tcy + oy / (float)H;
    ty = ty - floorf(ty);
    int sy = (int)floorf(ty * (float)H);
    sy = sy >= H ? H - 1 : sy;
    int dy = sy - y0;
    dy += dy < 0 ? H : 0;
    dy -= dy >= H ? H : 0;
    for (float ox = -kernel; ox <= kernel; ox += 1.0f) {
      const float f = 1.0f / (2.0f * 3.1415926535f * sigma * sigma) * PM::exp(-((ox * ox + oy * oy) / (2.0f * sigma * sigma)));
      count += f;
      float tx = tcx + ox / (float)W;
      tx = tx - floorf(tx);
      int sx = (int)floorf(tx * (float)W);
      sx = sx >= W ? W - 1 : sx;
      int dx = sx - x0;
      dx += dx < 0 ? W : 0;
      dx -= dx >= W ? W : 0;
      float cx, cy, cz;
      if (reach > 0 && dx < span_x && dy < span_y) {
        const float* t = &tile[3 * (dy * span_x + dx)];
        cx = t[0]; cy = t[1]; cz = t[2];
      } else {
        const float4 c = color[(size_t)sy * W + sx];
        cx = c.x; cy = c.y; cz = c.z;
      }
      ax += cx * f;
      ay += cy * f;
      az += cz * f;
    }
  }
  v[0] = ax / count * brightness;
  v[1] = ay / count * brightness;
  v[2] = az / count * brightness;
  at = (size_t)(STRIPED ? row0_local + ly : y) * W + x;
  return true;
}

template <int TY, bool STRIPED, class ND = float4>
__global__ __launch_bounds__(256) void rm_present_kernel(const float4* color, const ND* normal_dof, int W, int H, float brightness,
                                                         uchar4* out, int stripe_rows, int parts, int part, int local_rows) {
  float v[3];
  size_t at;
  if (!present_blur<TY, STRIPED, ND>(color, normal_dof, W, H, brightness, stripe_rows, parts, part, local_rows, v, at)) return;
  unsigned char o[3];
  for (int k = 0; k < 3; k++) {
    float g = PM::pow(v[k], 1.0f / 2.2f);
    o[k] = unorm8(g);
  }
  out[at] = make_uchar4(o[0], o[1], o[2], 255);
}

// ---- the display transform: a fourth stage behind the blur (rm_present_display*, rm_present_linear; opt-in) ----------------
// include/hip_raymarch.h and INTEGRATION.md "Display transform" state it in full, tests/display_ref.py restates it.  Per channel,
// every operation fp32 and rounded on its own, '/' IEEE's:  e = v * gain;  RM_TONE_CLIP, or a channel with !(e > 0): t = e;
// else E = min(e, 2^20) and Reinhard's extended operator or Narkowicz's ACES fit;  out = unorm8(pow(t, 1 / 2.2)).
// LINEAR stops at e: (e.r, e.g, e.b, 1) as float4.  With gain 1 and RM_TONE_CLIP these are rm_present_kernel's bytes.
RM_DEV float display_tone(float e, const DisplayPass& D) {
  if (D.tone == RM_TONE_CLIP || !(e > 0.0f)) return e;
  const float E = e < 1048576.0f ? e : 1048576.0f;
  if (D.tone == RM_TONE_REINHARD) {
    const float q = E / D.w2;
    const float a = 1.0f + q;
    const float n = E * a;
    const float d = 1.0f + E;
    return n / d;
  }
  float a = 2.51f * E;
  a = a + 0.03f;
  const float n = E * a;
  float b = 2.43f * E;
  b = b + 0.59f;
  b = E * b;
  const float d = b + 0.14f;
  return n / d;
}

// (A kernel added or renamed in this unit changes the string-table offsets of every symbol behind it.  ROCm's llvm-objdump -D, which
// tests/test_gbuffer_half_cpu.py runs over the code objects, faults while it "disassembles" .symtab / .dynsym when a symbol of
// section index 7 gets a name offset whose low nine bits are 0xF9 -- whichever symbol that is: if that test dies in llvm-objdump
// after such a change, another name length cures it.)
template <class ND, bool LINEAR>
__global__ __launch_bounds__(256) void rm_display_pass_kernel(const float4* color, const ND* normal_dof, int W, int H, float brightness, const DisplayPass D,
                                                                 void* out) {
  float v[3];
  size_t at;
  if (!present_blur<16, false, ND>(color, normal_dof, W, H, brightness, 0, 0, 0, 0, v, at)) return;
  const float e[3] = {v[0] * D.gain, v[1] * D.gain, v[2] * D.gain};
  if (LINEAR) {
    static_cast<float4*>(out)[at] = make_float4(e[0], e[1], e[2], 1.0f);
    return;
  }
  unsigned char o[3];
  for (int k = 0; k < 3; k++) o[k] = unorm8(PM::pow(display_tone(e[k], D), 1.0f / 2.2f));
  static_cast<uchar4*>(out)[at] = make_uchar4(o[0], o[1], o[2], 255);
}

// linear: out = W x H float4 (rm_present_linear), else W x H uchar4
hipError_t launch_present_display(const float4* color, const void* normal_dof, bool nd_half, int W, int H, float brightness, const DisplayPass& D, bool linear,
                                  void* out, hipStream_t stream) {
  const dim3 grid((W + 15) / 16, (H + 15) / 16);
#define RM_PRESENT_DISPLAY(ND, LINEAR) \
  hipLaunchKernelGGL((rm_display_pass_kernel<ND, LINEAR>), grid, dim3(256), 0, stream, color, static_cast<const ND*>(normal_dof), W, H, brightness, D, out)
  if (nd_half) {
    if (linear) RM_PRESENT_DISPLAY(rm_half4, true);
    else RM_PRESENT_DISPLAY(rm_half4, false);
  } else {
    if (linear) RM_PRESENT_DISPLAY(float4, true);
    else RM_PRESENT_DISPLAY(float4, false);
  }
#undef RM_PRESENT_DISPLAY
  return hipGetLastError();
}

// nd_half: normal_dof is a plane of rm_half4 (a framebuffer with the half G-buffer, rm_present)
hipError_t launch_present(const float4* color, const void* normal_dof, bool nd_half, int W, int H, float brightness, uchar4* out, hipStream_t stream) {
  if (nd_half)
    hipLaunchKernelGGL((rm_present_kernel<16, false, rm_half4>), dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, stream, color,
                       static_cast<const rm_half4*>(normal_dof), W, H, brightness, out, 0, 0, 0, 0);
  else
    hipLaunchKernelGGL((rm_present_kernel<16, false>), dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, stream, color,
                       static_cast<const float4*>(normal_dof), W, H, brightness, out, 0, 0, 0, 0);
  return hipGetLastError();
}

// part `part` of `parts` striped windows (stripes of stripe_rows rows, dealt round-robin): out = that part's packed rows
hipError_t launch_present_striped(const float4* color, const float4* normal_dof, int W, int H, float brightness, uchar4* out, int stripe_rows, int parts,
                                  int part, int local_rows, hipStream_t stream) {
  if (local_rows <= 0) return hipSuccess;
#define RM_PRESENT_STRIPED(TY)                                                                                                                              \
  hipLaunchKernelGGL((rm_present_kernel<TY, true>), dim3((W + 256 / TY - 1) / (256 / TY), (local_rows + TY - 1) / TY), dim3(256), 0, stream, color, normal_dof, W, \
                     H, brightness, out, stripe_rows, parts, part, local_rows)
  if (stripe_rows % 16 == 0) RM_PRESENT_STRIPED(16);
  else if (stripe_rows % 8 == 0) RM_PRESENT_STRIPED(8);
  else if (stripe_rows % 4 == 0) RM_PRESENT_STRIPED(4);
  else RM_PRESENT_STRIPED(1);
#undef RM_PRESENT_STRIPED
  return hipGetLastError();
}

// The present pass of a window of rows when depth of field is off (no normal_dof plane = blur radius 0): the one tap
// of display.frag's loop is the pixel itself, so it needs no neighbour rows and a rank can tone-map the stripes it
// holds.  The same operations as rm_present_kernel performs for kernel = 0, hence the same bytes.
__global__ __launch_bounds__(256) void rm_present_rows_kernel(const float4* color, long long pixels, float brightness, uchar4* out) {
  const float sigma = gmax(0.0f, 1.0f) * 0.3f;
  const float f = 1.0f / (2.0f * 3.1415926535f * sigma * sigma) * PM::exp(-((0.0f * 0.0f + 0.0f * 0.0f) / (2.0f * sigma * sigma)));
  const float count = 0.0f + f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (long long)gridDim.x * 256) {
    const float4 c = color[i];
    const float v[3] = {(0.0f + c.x * f) / count * brightness, (0.0f + c.y * f) / count * brightness, (0.0f + c.z * f) / count * brightness};
    unsigned char o[3];
    for (int k = 0; k < 3; k++) {
      float g = PM::pow(v[k], 1.0f / 2.2f);
      o[k] = unorm8(g);
    }
    out[i] = make_uchar4(o[0], o[1], o[2], 255);
  }
}

hipError_t launch_present_rows(const float4* color, long long pixels, float brightness, uchar4* out, hipStream_t stream) {
  hipLaunchKernelGGL(rm_present_rows_kernel, dim3(small_grid(pixels)), dim3(256), 0, stream, color, pixels, brightness, out);
  return hipGetLastError();
}

// What the present pass reads of a window of rows, one float4 per pixel: (colour.rgb, normal_dof.w) -- display.frag reads the
// colour (:19,:53) and the accumulated depth-of-field radius (:21-23) and nothing else.  A sharded frame WITH depth of field
// gathers these rows instead of tone-mapped bytes (the blur reads up to 16 rows either side, which other ranks hold);
// assembled in image order the buffer serves rm_present_device as BOTH its colour and its normal_dof plane.
// (With the half G-buffer the .w is widened exactly: the packed rows stay float4, and everything downstream of them is unchanged.)
template <class ND>
__global__ __launch_bounds__(256) void rm_pack_rows_kernel(const float4* color, const ND* normal_dof, long long pixels, float4* out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (long long)gridDim.x * 256) {
    const float4 c = color[i];
    out[i] = make_float4(c.x, c.y, c.z, normal_dof != nullptr ? dof_of(normal_dof[i]) : 0.0f);
  }
}

hipError_t launch_pack_rows(const float4* color, const void* normal_dof, bool nd_half, long long pixels, float4* out, hipStream_t stream) {
  if (nd_half)
    hipLaunchKernelGGL(rm_pack_rows_kernel<rm_half4>, dim3(small_grid(pixels)), dim3(256), 0, stream, color, static_cast<const rm_half4*>(normal_dof), pixels, out);
  else
    hipLaunchKernelGGL(rm_pack_rows_kernel<float4>, dim3(small_grid(pixels)), dim3(256), 0, stream, color, static_cast<const float4*>(normal_dof), pixels, out);
  return hipGetLastError();
}

// ---- a half plane from / to fp32 (rm_fb_upload / rm_fb_download of a framebuffer with the half G-buffer) -------------------
// The upload narrows with the helper the render kernels store with, so what a host uploads is rounded exactly as an accumulation is.
__global__ __launch_bounds__(256) void rm_narrow_kernel(const float4* src, rm_half4* dst, long long pixels) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (long long)gridDim.x * 256) dst[i] = rm_narrow(src[i]);
}
__global__ __launch_bounds__(256) void rm_widen_kernel(const rm_half4* src, float4* dst, long long pixels) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (long long)gridDim.x * 256) dst[i] = rm_widen(src[i]);
}

hipError_t launch_convert(const void* src, void* dst, long long pixels, bool narrow, hipStream_t stream) {
  if (narrow)
    hipLaunchKernelGGL(rm_narrow_kernel, dim3(small_grid(pixels)), dim3(256), 0, stream, static_cast<const float4*>(src), static_cast<rm_half4*>(dst), pixels);
  else
    hipLaunchKernelGGL(rm_widen_kernel, dim3(small_grid(pixels)), dim3(256), 0, stream, static_cast<const rm_half4*>(src), static_cast<float4*>(dst), pixels);
  return hipGetLastError();
}
#endif

#if !RM_BUILD_FAST && !RM_GL_STACK
// ---- denoise: edge-avoiding a-trous wavelet filter guided by the G-buffer (Dammertz et al. 2010) --------------------
// The filter display.frag:27-42 asks for ("How do I account for normals with denoising? ... i might focus more on depth
// now"), run on the planes after k samples; INTEGRATION.md "Denoising" states it in full, tests/denoise_ref.py restates it
// in float64.  With s = 1 / k (present_device's scale), per pixel p:
//   m_p = max(A.xyz s, 1e-3)   x_p = C.rgb s / m_p   n_p = normalize(N.xyz s) (0 when |.| < 1e-6 or not finite)   z_p = A.w s
// Pass i = 0 .. L-1, step h = 2^i, taps q = p + h (dx, dy), dx, dy in -2..2, taps outside the image skipped:
//   w = b[dx] b[dy] exp(-|x_p - x_q|^2 / (sigma_c^2 4^-i)) exp(-|n_p - n_q|^2 / sigma_n^2) w_z,   b = (1, 4, 6, 4, 1) / 16
//   w_z = 1 at the centre or when both depths are non-finite, 0 when one is, else
//         exp(-|z_p - z_q| / (sigma_z max(z_p, 1e-6) h sqrt(dx^2 + dy^2)));  a tap with a non-finite x_q weighs 0
//   x'_p = sum w x_q / sum w   (a non-finite x_p keeps its value);  the guides n, z stay those of the input.
// Output: (x_L m_p k, C.w).  One launch per pass, 16 x 16 pixels per workgroup, one thread per pixel.  Pass 0 computes x and
// the guide (n.xyz, z) of the pixels it reads from the planes and writes each pixel's guide once; the last pass multiplies
// the modulation back.  Steps 1 and 2 stage the tile and its halo of 2h pixels in LDS (20^2 or 24^2 pixels x 32 B); wider
// steps read x and the guide through the caches.  No pixel kernel is touched.
template <class GB>
__device__ inline float4 dn_load(const void* plane, size_t i);
template <>
__device__ inline float4 dn_load<float4>(const void* plane, size_t i) { return static_cast<const float4*>(plane)[i]; }
template <>
__device__ inline float4 dn_load<rm_half4>(const void* plane, size_t i) { return rm_widen(static_cast<const rm_half4*>(plane)[i]); }

__device__ inline float3 dn_modulation(const float4 a, float s) { return make_float3(fmaxf(a.x * s, 1e-3f), fmaxf(a.y * s, 1e-3f), fmaxf(a.z * s, 1e-3f)); }
__device__ inline bool dn_finite3(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
__device__ inline float dn_scaled(float d, float inv) { return d > 0.0f ? d * inv : 0.0f; }  // d * inv, and 0 for d = 0 even when inv = inf

// x (demodulated colour, .w unused) and guide (n.xyz, z) of pixel i, from the planes
template <class GB>
__device__ inline void dn_prepare(const DenoisePass& P, size_t i, float4& x, float4& g) {
  const float4 c = P.color[i], a = dn_load<GB>(P.albedo_depth, i), n = dn_load<GB>(P.normal_dof, i);
  const float3 m = dn_modulation(a, P.s);
  x = make_float4(c.x * P.s / m.x, c.y * P.s / m.y, c.z * P.s / m.z, 0.0f);
  const float nx = n.x * P.s, ny = n.y * P.s, nz = n.z * P.s;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  g = (len >= 1e-6f && isfinite(len)) ? make_float4(nx / len, ny / len, nz / len, a.w * P.s) : make_float4(0.0f, 0.0f, 0.0f, a.w * P.s);
}

// ---- the variance-guided mode (rm_denoise_variance; SVGF's colour weight, Schied et al. 2017) ----
// x.w carries v, the variance of the pixel's demodulated luminance: pass 0 computes it from the moments plane,
//   v_p = max(0, M.y s - (M.x s)^2) s / max(lum(m_p), 1e-3)^2   (0 where not finite),
// and every pass filters it with the squared weights, v'_p = sum w^2 v_q / (sum w)^2.  The colour weight of a pass is
//   w_l = exp(-|lum(x_p) - lum(x_q)| / (sigma_l sqrt(g_p) + eps_p)),   eps_p = max(1e-3 |lum(x_p)|, 1e-6),
//   g = the 3x3 Gaussian (1,2,1)^2/16 of v
// (taps outside the image skipped, renormalised), read from the tile in LDS at steps 1 and 2 and through the caches beyond.
// The normal and depth weights, the spatial kernel, the taps and the remodulation are the mode above's.
__device__ inline float dn_lum(const float4 v) { return (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z; }

template <class GB>
__device__ inline void dn_prepare_var(const DenoisePass& P, size_t i, float4& x, float4& g) {
  dn_prepare<GB>(P, i, x, g);
  const float3 m = dn_modulation(dn_load<GB>(P.albedo_depth, i), P.s);
  const float2 M = P.moments[i];
  const float mu = M.x * P.s, lm = fmaxf((0.2126f * m.x + 0.7152f * m.y) + 0.0722f * m.z, 1e-3f);
  const float v = fmaxf(0.0f, M.y * P.s - mu * mu) * P.s / (lm * lm);
  x.w = isfinite(v) ? v : 0.0f;
}

// STAGE: the step h of a pass staged in LDS (1 or 2), 0 for a pass that reads through the caches.  PREP: pass 0 (reads the
// planes).  LAST: the last pass (writes colour-plane units).  GB: float4, or rm_half4 for the planes of a half G-buffer.
// VAR: the variance-guided mode (above); false is rm_denoise's filter.
template <int STAGE, bool PREP, bool LAST, class GB, bool VAR>
__global__ __launch_bounds__(256) void rm_denoise_kernel(const DenoisePass P) {
  static_assert(!(VAR && PREP && STAGE == 0), "pass 0 is staged");
  constexpr int HALO = 2 * STAGE, SPAN = 16 + 2 * HALO;
  __shared__ float4 sx[STAGE > 0 ? SPAN * SPAN : 1], sg[STAGE > 0 ? SPAN * SPAN : 1];
  const int lx = threadIdx.x % 16, ly = threadIdx.x / 16;
  const int x = blockIdx.x * 16 + lx, y = blockIdx.y * 16 + ly;
  const int h = P.step;
  if (STAGE > 0) {
    const int x0 = (int)blockIdx.x * 16 - HALO, y0 = (int)blockIdx.y * 16 - HALO;
    for (int i = threadIdx.x; i < SPAN * SPAN; i += 256) {
      const int gx = x0 + i % SPAN, gy = y0 + i / SPAN;
      if (gx < 0 || gx >= P.W || gy < 0 || gy >= P.H) continue;  // never read: a tap outside the image is skipped
      const size_t q = (size_t)gy * P.W + gx;
      if (PREP) {
        if (VAR) dn_prepare_var<GB>(P, q, sx[i], sg[i]);
        else dn_prepare<GB>(P, q, sx[i], sg[i]);
      }
      else { sx[i] = P.x_in[q]; sg[i] = P.guide[q]; }
    }
    __syncthreads();
  }
  if (x >= P.W || y >= P.H) return;
  const size_t p = (size_t)y * P.W + x;
  float4 xp, gp;
  if (STAGE > 0) {
    const int c = (ly + HALO) * SPAN + lx + HALO;
    xp = sx[c];
    gp = sg[c];
  } else if (PREP) {
    if (VAR) dn_prepare_var<GB>(P, p, xp, gp);
    else dn_prepare<GB>(P, p, xp, gp);
  } else {
    xp = P.x_in[p];
    gp = P.guide[p];
  }
  if (PREP) P.guide[p] = gp;
  float4 r = xp;
  if (dn_finite3(xp)) {
    constexpr float b[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float zp = gp.w;
    float lp = 0.0f, inv_l = 0.0f, av = 0.0f;
    if (VAR) {  // g_p: the 3x3 prefilter of v around p
      float gs = 0.0f, gw = 0.0f;
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
        if (y + dy < 0 || y + dy >= P.H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          if (x + dx < 0 || x + dx >= P.W) continue;
          const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
          gs += k * (STAGE > 0 ? sx[(ly + HALO + dy) * SPAN + lx + HALO + dx].w : P.x_in[(size_t)(y + dy) * P.W + (x + dx)].w);
          gw += k;
        }
      }
      lp = dn_lum(xp);
      inv_l = 1.0f / (P.sigma_l * sqrtf(gs / gw) + fmaxf(1e-3f * fabsf(lp), 1e-6f));  // eps_p: well above lum's fp32 resolution
    }
    const bool zp_finite = isfinite(zp);
    const float inv_z = 1.0f / (P.sigma_z_h * fmaxf(zp, 1e-6f));
    float ax = 0.0f, ay = 0.0f, az = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
      const int qy = y + dy * h;
      if (qy < 0 || qy >= P.H) continue;
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int qx = x + dx * h;
        if (qx < 0 || qx >= P.W) continue;
        float4 xq, gq;
        if (STAGE > 0) {
          const int t = (ly + HALO + dy * STAGE) * SPAN + lx + HALO + dx * STAGE;
          xq = sx[t];
          gq = sg[t];
        } else {
          const size_t q = (size_t)qy * P.W + qx;
          xq = P.x_in[q];
          gq = P.guide[q];
        }
        if (!dn_finite3(xq)) continue;
        const float cx = xp.x - xq.x, cy = xp.y - xq.y, cz = xp.z - xq.z;
        const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
        float e = (VAR ? dn_scaled(fabsf(lp - dn_lum(xq)), inv_l) : dn_scaled(cx * cx + cy * cy + cz * cz, P.inv_color)) +
                  dn_scaled(nx * nx + ny * ny + nz * nz, P.inv_normal);
        if (dx != 0 || dy != 0) {
          const bool zq_finite = isfinite(gq.w);
          if (zq_finite != zp_finite) continue;
          if (zp_finite) e += dn_scaled(fabsf(zp - gq.w), inv_z * (1.0f / sqrtf((float)(dx * dx + dy * dy))));
        }
        const float w = b[dx + 2] * b[dy + 2] * expf(-e);
        ax += w * xq.x;
        ay += w * xq.y;
        az += w * xq.z;
        wsum += w;
        if (VAR) av += w * w * xq.w;
      }
    }
    r = make_float4(ax / wsum, ay / wsum, az / wsum, VAR ? av / (wsum * wsum) : 0.0f);  // wsum >= b[2]^2: the centre tap weighs (3/8)^2
  }
  if (LAST) {
    const float3 m = dn_modulation(dn_load<GB>(P.albedo_depth, p), P.s);
    r = make_float4(r.x * m.x * P.k, r.y * m.y * P.k, r.z * m.z * P.k, P.color[p].w);
  }
  P.out[p] = r;
}

template <bool VAR>
static hipError_t launch_denoise_pass_t(const DenoisePass& P, bool half, bool prep, bool last, hipStream_t stream) {
  const dim3 grid((P.W + 15) / 16, (P.H + 15) / 16);
#define RM_DENOISE(STAGE, PREP, GB)                                                                                    \
  do {                                                                                                                 \
    if (last) hipLaunchKernelGGL((rm_denoise_kernel<STAGE, PREP, true, GB, VAR>), grid, dim3(256), 0, stream, P);     \
    else hipLaunchKernelGGL((rm_denoise_kernel<STAGE, PREP, false, GB, VAR>), grid, dim3(256), 0, stream, P);         \
  } while (0)
  if (prep) {  // pass 0: h = 1
    if (half) RM_DENOISE(1, true, rm_half4);
    else RM_DENOISE(1, true, float4);
  } else if (P.step == 2) {
    if (half) RM_DENOISE(2, false, rm_half4);
    else RM_DENOISE(2, false, float4);
  } else {
    if (half) RM_DENOISE(0, false, rm_half4);
    else RM_DENOISE(0, false, float4);
  }
#undef RM_DENOISE
  return hipGetLastError();
}

hipError_t launch_denoise_pass(const DenoisePass& P, bool half, bool prep, bool last, hipStream_t stream) {
  return launch_denoise_pass_t<false>(P, half, prep, last, stream);
}
hipError_t launch_denoise_variance_pass(const DenoisePass& P, bool half, bool prep, bool last, hipStream_t stream) {
  return launch_denoise_pass_t<true>(P, half, prep, last, stream);
}

// ---- despeckle: the firefly filter ahead of the denoisers and the present (rm_filter*, opt-in) ----------------------
// An outlier clamp on the colour plane after k samples; include/hip_raymarch.h and INTEGRATION.md "Firefly filter" state it in
// full, tests/despeckle_ref.py restates it in float32.  With s = 1.0f / k, every product and sum rounded on its own:
//   l_p = (0.2126f * (C.r * s) + 0.7152f * (C.g * s)) + 0.0722f * (C.b * s);   a pixel is valid iff l_p is finite.
// Over the (2 radius + 1)^2 window without the centre (dy outer, dx inner; taps outside the image and invalid taps skipped):
//   n = the number of valid taps,  t = the (rank + 1)-th largest l_q,  T = gain * t + floor.
//   n <= rank: unchanged.   valid centre: l_p <= T unchanged (bit for bit), else C.rgb * (t / l_p).
//   invalid centre: with repair the mean of the taps with l_q <= t (summed in scan order, / (float)count; unchanged unless
//   every channel of it is finite), else unchanged.   .w is always C.w.
// One launch, 16 x 16 pixels per workgroup, one thread per pixel.  The tile and its halo of RADIUS pixels are staged in LDS as
// the colour and l (computed once per staged pixel); a slot outside the image is marked invalid (NaN) and never read from
// memory.  The RANK + 1 largest values stay in registers (unrolled insertion), and only an invalid centre walks the window a
// second time.  Reads the colour plane alone: 16 B in, 16 B out per pixel, whatever the G-buffer.
template <int RADIUS, int RANK>
__global__ __launch_bounds__(256) void rm_despeckle_kernel(const DespecklePass P) {
  constexpr int SPAN = 16 + 2 * RADIUS;
  __shared__ float4 sc[SPAN * SPAN];
  __shared__ float sl[SPAN * SPAN];
  const int lx = threadIdx.x % 16, ly = threadIdx.x / 16;
  const int x = blockIdx.x * 16 + lx, y = blockIdx.y * 16 + ly;
  const int x0 = (int)blockIdx.x * 16 - RADIUS, y0 = (int)blockIdx.y * 16 - RADIUS;
  for (int i = threadIdx.x; i < SPAN * SPAN; i += 256) {
    const int gx = x0 + i % SPAN, gy = y0 + i / SPAN;
    if (gx < 0 || gx >= P.W || gy < 0 || gy >= P.H) {
      sl[i] = __int_as_float(0x7fc00000);  // invalid: a tap outside the image is skipped
      continue;
    }
    const float4 c = P.color[(size_t)gy * P.W + gx];
    sc[i] = c;
    sl[i] = (0.2126f * (c.x * P.s) + 0.7152f * (c.y * P.s)) + 0.0722f * (c.z * P.s);
  }
  __syncthreads();
  if (x >= P.W || y >= P.H) return;
  const int ci = (ly + RADIUS) * SPAN + lx + RADIUS;
  const float4 c = sc[ci];
  const float lp = sl[ci];
  float top[RANK + 1];  // the RANK + 1 largest valid l_q so far, descending
#pragma unroll
  for (int j = 0; j <= RANK; j++) top[j] = -INFINITY;
  int n = 0;
#pragma unroll
  for (int dy = -RADIUS; dy <= RADIUS; dy++) {
#pragma unroll
    for (int dx = -RADIUS; dx <= RADIUS; dx++) {
      if (dx == 0 && dy == 0) continue;
      float v = sl[ci + dy * SPAN + dx];
      if (!isfinite(v)) continue;
      n++;
#pragma unroll
      for (int j = 0; j <= RANK; j++) {
        const float hi = fmaxf(v, top[j]), lo = fminf(v, top[j]);  // both finite or -inf: no NaN reaches here
        top[j] = hi;
        v = lo;
      }
    }
  }
  float4 r = c;
  if (n > RANK) {
    const float t = top[RANK];
    if (isfinite(lp)) {
      const float T = P.gain * t + P.floor;
      if (lp > T) {
        const float f = t / lp;
        r = make_float4(c.x * f, c.y * f, c.z * f, c.w);
      }
    } else if (P.repair) {
      float ax = 0.0f, ay = 0.0f, az = 0.0f;
      int count = 0;
      for (int dy = -RADIUS; dy <= RADIUS; dy++) {
        for (int dx = -RADIUS; dx <= RADIUS; dx++) {
          if (dx == 0 && dy == 0) continue;
          const int q = ci + dy * SPAN + dx;
          const float v = sl[q];
          if (!isfinite(v) || !(v <= t)) continue;
          const float4 cq = sc[q];
          ax += cq.x;
          ay += cq.y;
          az += cq.z;
          count++;
        }
      }
      const float mx = ax / (float)count, my = ay / (float)count, mz = az / (float)count;  // count >= 1: the tap that gave t
      if (isfinite(mx) && isfinite(my) && isfinite(mz)) r = make_float4(mx, my, mz, c.w);
    }
  }
  P.out[(size_t)y * P.W + x] = r;
}

hipError_t launch_despeckle(const DespecklePass& P, int radius, int rank, hipStream_t stream) {
  const dim3 grid((P.W + 15) / 16, (P.H + 15) / 16);
#define RM_DESPECKLE(RADIUS)                                                                                   \
  switch (rank) {                                                                                              \
    case 0: hipLaunchKernelGGL((rm_despeckle_kernel<RADIUS, 0>), grid, dim3(256), 0, stream, P); break;        \
    case 1: hipLaunchKernelGGL((rm_despeckle_kernel<RADIUS, 1>), grid, dim3(256), 0, stream, P); break;        \
    case 2: hipLaunchKernelGGL((rm_despeckle_kernel<RADIUS, 2>), grid, dim3(256), 0, stream, P); break;        \
    case 3: hipLaunchKernelGGL((rm_despeckle_kernel<RADIUS, 3>), grid, dim3(256), 0, stream, P); break;        \
    default: return hipErrorInvalidValue;                                                                      \
  }
  if (radius == 1) { RM_DESPECKLE(1) }
  else if (radius == 2) { RM_DESPECKLE(2) }
  else return hipErrorInvalidValue;
#undef RM_DESPECKLE
  return hipGetLastError();
}

// ---- frame statistics: the luminance histogram of a colour plane (rm_frame_stats) ------------------------------------------
// l as the firefly filter computes it (s = 1.0f / k, every product and sum rounded on its own); every pixel falls in one class:
// non-finite, below 2^-20 (negatives, zeros, subnormals), at or above 2^12, or bin (bits(l) >> 19) - 1712 of 512 (16 per octave
// over 32 octaves: integer arithmetic on the float's bits, no logarithm), and min / max over the finite l.  Grid-stride, one
// float4 load per pixel, two in flight per lane; a workgroup counts in LDS (32-bit: its share of the frame) and adds its non-zero
// counters to the 64-bit global ones once (integer sums: nothing depends on the order of arrival).  A wave first takes the
// lanes that share its first lane's class in ONE LDS atomic of their number (a constant region -- sky -- would otherwise
// serialise 64 atomics on one word); the others add 1 each.  min / max travel as order-preserving unsigned keys (-0 below +0),
// the minimum as its complement, so that the zeroed buffer is their neutral element: two 32-bit words behind the counters.
// Measured against per-workgroup slabs and a sum kernel (3840 x 2160, MI355X): the atomics took 0.075 ms a call on a rendered
// frame (190 bins in use) and 0.062 ms on a constant one, the slabs 0.114 ms on both (profiles/display_transform.txt).
RM_DEV unsigned int stats_key(float l) {
  const unsigned int b = __float_as_uint(l);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one pixel into the workgroup's counters and the thread's running extremes (lo = ~key of the minimum, hi = key of the maximum)
RM_DEV void stats_count(const float4 c, float s, unsigned int* h, unsigned int& lo, unsigned int& hi) {
  const float l = (0.2126f * (c.x * s) + 0.7152f * (c.y * s)) + 0.0722f * (c.z * s);
  int cls;
  if (!finite(l)) {
    cls = RM_STATS_NON_FINITE;
  } else {
    const unsigned int key = stats_key(l);
    lo = lo > ~key ? lo : ~key;
    hi = hi > key ? hi : key;
    cls = l < 9.5367431640625e-07f ? RM_STATS_BELOW : l >= 4096.0f ? RM_STATS_ABOVE : (int)(__float_as_uint(l) >> 19) - 1712;
  }
  const int first = __builtin_amdgcn_readfirstlane(cls);  // of the lanes that are here
  const unsigned long long same = ballot(cls == first);
  if (cls != first) atomicAdd(&h[cls], 1u);
  else if ((same & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0ull) atomicAdd(&h[first], (unsigned int)__popcll(same));
}

__global__ __launch_bounds__(256) void rm_frame_stats_kernel(const float4* color, long long pixels, float s, unsigned long long* counters) {
  __shared__ unsigned int h[RM_STATS_COUNTERS + 2];  // the counters, then ~key of the minimum and key of the maximum
  for (int i = threadIdx.x; i < RM_STATS_COUNTERS + 2; i += 256) h[i] = 0u;
  __syncthreads();
  unsigned int lo = 0u, hi = 0u;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pixels; i += 2 * stride) {  // two loads in flight per lane
    const long long j = i + stride;
    const float4 c0 = color[i];
    if (j < pixels) {
      const float4 c1 = color[j];
      stats_count(c0, s, h, lo, hi);
      stats_count(c1, s, h, lo, hi);
    } else {
      stats_count(c0, s, h, lo, hi);
    }
  }
  if (hi != 0u) {  // this thread saw a finite l
    atomicMax(&h[RM_STATS_COUNTERS], lo);
    atomicMax(&h[RM_STATS_COUNTERS + 1], hi);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RM_STATS_COUNTERS; i += 256)
    if (h[i] != 0u) atomicAdd(&counters[i], (unsigned long long)h[i]);
  if (threadIdx.x == 0 && h[RM_STATS_COUNTERS + 1] != 0u) {
    unsigned int* const keys = reinterpret_cast<unsigned int*>(counters + RM_STATS_COUNTERS);
    atomicMax(&keys[0], h[RM_STATS_COUNTERS]);
    atomicMax(&keys[1], h[RM_STATS_COUNTERS + 1]);
  }
}

// counters: RM_STATS_BYTES of device memory, zeroed on `stream` before this launch
hipError_t launch_frame_stats(const float4* color, long long pixels, float s, unsigned long long* counters, hipStream_t stream) {
  const long long g = (pixels + 255) / 256;
  hipLaunchKernelGGL(rm_frame_stats_kernel, dim3((unsigned int)(g < 1 ? 1 : g < RM_STATS_GRID ? g : RM_STATS_GRID)), dim3(256), 0, stream, color, pixels, s, counters);
  return hipGetLastError();
}
#endif

}  // namespace rm
