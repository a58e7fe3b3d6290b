// Background-corrected pattern ingest ("Pattern correction"): what a raw
// detector pattern needs before it looks like the simulated dictionary, as one stage of the
// on-device scan path.  Per pattern, on the centre-cropped (oh, ow) window (crop.h offsets, no
// padding):
//
//   v = float32(src), non-finite -> 0
//   s = v | v - bg | v / bg                  static background bg (H0, W0), cropped here
//   b = G_sigma * s                          separable, x then y, border "reflect" (d c b a | a b c d),
//                                            taps (radius + 1, one-sided) computed by the host
//   d = s | s - b | s / b (0 where b == 0)   dynamic background
//   out = (d - min d) / (max d - min d)      0 everywhere when max == min
//
// Both blur passes run out of LDS planes with an ODD row stride (ow | 1 floats).  The x pass
// maps a wave's lanes to consecutive rows (addresses y * stride + x: stride odd -> 32 lanes on
// 32 banks), the y pass maps them to consecutive columns (addresses y * stride + x: consecutive
// banks); a stride of exactly 128 floats would put every lane of the x pass on one bank.  Each
// thread produces kRun adjacent outputs of its line from a register window of taps, so one
// sample read and one (broadcast) tap read feed kRun FMAs.  Every output is one fma chain over
// the taps from -radius to +radius, whichever kernel computes it.
//
// oh * ow <= 128 * 128: one launch, one block per pattern, the s and x-pass planes in LDS
// (2 x 64.5 KiB at 128 x 128), source read once and output written once.  Larger windows (up to
// 256 x 256) take the same device functions in three launches: x pass over bands of 64 rows ->
// plane in `work`; y pass + dynamic step over bands of 64 columns -> d in dst, the band's min /
// max in `work`; rescale of dst in place.  The values are bit-identical between the two paths.
#include <math.h>

#include "common.h"
#include "crop.h"
#include "pattern_src.h"
#include "../../include/ebsdvae.h"

namespace ev {

constexpr int kRun = 8;             // adjacent outputs per thread and blur line
constexpr int kCorrThreads = 1024;  // 16 waves; one block per CU on the 128 x 128 fused path
constexpr int kCorrWaves = kCorrThreads / 64;
constexpr int kBand = 64;           // rows (x pass) / columns (y pass) of a phased block
constexpr int kCorrMaxSide = 256;   // out_h, out_w limit
constexpr int kFusedMaxPx = 128 * 128;
constexpr int kMaxRadius = kCorrMaxSide;
constexpr int kTapWin = 2 * kMaxRadius + kRun;   // taps -r .. r, then kRun - 1 zeros (+1 spare)

struct CorrArgs {
  int H0, W0, oh, ow, top, left;
  const float* bg;     // (H0, W0) or nullptr
  const float* taps;   // radius + 1 or nullptr
  int smode, dmode, radius;
};

// steps 1 and 2 at window pixel (y, x) of one pattern
template <typename T>
EV_DEVINL float load_static(const T* __restrict__ pat, const CorrArgs& a, int y, int x) {
  const size_t o = (size_t)(y + a.top) * a.W0 + (x + a.left);
  float v = finite_or_zero((float)pat[o]);
  if (a.smode == 1) v = v - a.bg[o];
  else if (a.smode == 2) v = v / a.bg[o];
  return v;
}

EV_DEVINL float dynamic_step(float s, float b, int dmode) {
  if (dmode == 1) return s - b;
  if (dmode == 2) return b == 0.f ? 0.f : s / b;
  return s;
}

EV_DEVINL float rescale(float d, float lo, float hi) {
  return hi == lo ? 0.f : (d - lo) / (hi - lo);
}

// taps[|i|] for i = -r .. r at win[i + r], zeros up to win[2r + kRun - 1]
EV_DEVINL void stage_taps(float* win, const CorrArgs& a) {
  if (a.dmode == 0) return;
  const int r = a.radius;
  for (int i = threadIdx.x; i < 2 * r + kRun; i += blockDim.x)
    win[i] = i <= 2 * r ? a.taps[abs(i - r)] : 0.f;
}

// acc[k] = sum_{i = -r .. r} taps[|i|] * line[reflect(p0 + k + i) * stride], k < kRun: sample
// p0 + j meets output k with tap j - k, held in tw[k]; the window slides by one register per
// sample.  The zero taps outside [-r, r] add +0 and leave the chain of output k the ascending
// sum over its own 2r + 1 taps.  len >= r, so one reflection lands inside; the clamp only
// serves the outputs past the line's end of a last, partial run (never stored).
EV_DEVINL void blur_run(const float* line, int stride, int len, int p0, const float* win, int r,
                        float (&acc)[kRun]) {
  float tw[kRun];
#pragma unroll
  for (int k = 0; k < kRun; ++k) acc[k] = 0.f, tw[k] = 0.f;
#pragma unroll kRun
  for (int j = -r; j < r + kRun; ++j) {
#pragma unroll
    for (int k = kRun - 1; k > 0; --k) tw[k] = tw[k - 1];
    tw[0] = win[j + r];
    int p = p0 + j;
    p ^= p >> 31;                             // p < 0 -> -1 - p (branch-free)
    p = max(min(p, 2 * len - 1 - p), 0);      // p >= len -> 2 len - 1 - p
    const float v = line[p * stride];
#pragma unroll
    for (int k = 0; k < kRun; ++k) acc[k] = fmaf(tw[k], v, acc[k]);
  }
}

// x pass over `rows` rows of S into X (both rows x ps in LDS): a wave's lanes take consecutive
// rows of one run of columns
EV_DEVINL void x_pass(const float* S, float* X, int rows, int ow, int ps, const float* win, int r) {
  const int items = rows * ((ow + kRun - 1) / kRun);
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int y = it % rows, x0 = (it / rows) * kRun;
    float acc[kRun];
    blur_run(S + y * ps, 1, ow, x0, win, r, acc);
#pragma unroll
    for (int k = 0; k < kRun; ++k)
      if (x0 + k < ow) X[y * ps + x0 + k] = acc[k];
  }
}

// block-wide min / max, the same value in every thread: xor-shuffle tree per wave, then the
// waves' results through LDS in wave order
EV_DEVINL void block_minmax(float& lo, float& hi, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) red[2 * wave] = lo, red[2 * wave + 1] = hi;
  __syncthreads();
  lo = red[0], hi = red[1];
  for (int w = 1; w < nw; ++w) lo = fminf(lo, red[2 * w]), hi = fmaxf(hi, red[2 * w + 1]);
}

// ---- oh * ow <= kFusedMaxPx: the whole pattern in one block
template <typename T>
__global__ __launch_bounds__(kCorrThreads) void correct_fused_kernel(const T* __restrict__ src,
                                                                     CorrArgs a,
                                                                     float* __restrict__ dst) {
  extern __shared__ float planes[];   // S (oh x ps), X (oh x ps)
  __shared__ float win[kTapWin];
  __shared__ float red[2 * kCorrWaves];
  const int oh = a.oh, ow = a.ow, ps = ow | 1, n = oh * ow;
  float* S = planes;
  float* X = planes + oh * ps;
  const T* pat = src + (size_t)blockIdx.x * a.H0 * a.W0;
  stage_taps(win, a);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int y = i / ow, x = i - y * ow;
    S[y * ps + x] = load_static(pat, a, y, x);
  }
  __syncthreads();
  float lo = INFINITY, hi = -INFINITY;
  if (a.dmode != 0) {
    x_pass(S, X, oh, ow, ps, win, a.radius);
    __syncthreads();
    // y pass: a wave's lanes take consecutive columns of one run of rows; d replaces s
    const int items = ow * ((oh + kRun - 1) / kRun);
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
      const int x = it % ow, y0 = (it / ow) * kRun;
      float acc[kRun];
      blur_run(X + x, ps, oh, y0, win, a.radius, acc);
#pragma unroll
      for (int k = 0; k < kRun; ++k)
        if (y0 + k < oh) {
          const float d = dynamic_step(S[(y0 + k) * ps + x], acc[k], a.dmode);
          S[(y0 + k) * ps + x] = d;
          lo = fminf(lo, d), hi = fmaxf(hi, d);
        }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int y = i / ow, x = i - y * ow;
      const float d = S[y * ps + x];
      lo = fminf(lo, d), hi = fmaxf(hi, d);
    }
  }
  block_minmax(lo, hi, red);   // its barrier also orders the d writes before the reads below
  float* out = dst + (size_t)blockIdx.x * n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int y = i / ow, x = i - y * ow;
    out[i] = rescale(S[y * ps + x], lo, hi);
  }
}

// ---- larger windows, phase 1: s and the x pass for rows [band * kBand, ...) of one pattern
template <typename T>
__global__ __launch_bounds__(kCorrThreads) void correct_xpass_kernel(const T* __restrict__ src,
                                                                     CorrArgs a, int nbands,
                                                                     float* __restrict__ xplane) {
  extern __shared__ float planes[];   // S (rows x ps), X (rows x ps)
  __shared__ float win[kTapWin];
  const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
  const int ow = a.ow, ps = ow | 1;
  const int y0 = band * kBand, rows = min(kBand, a.oh - y0), n = rows * ow;
  float* S = planes;
  float* X = planes + kBand * ps;
  const T* pat = src + (size_t)b * a.H0 * a.W0;
  stage_taps(win, a);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int y = i / ow, x = i - y * ow;
    S[y * ps + x] = load_static(pat, a, y0 + y, x);
  }
  __syncthreads();
  x_pass(S, X, rows, ow, ps, win, a.radius);
  __syncthreads();
  float* out = xplane + ((size_t)b * a.oh + y0) * ow;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int y = i / ow, x = i - y * ow;
    out[i] = X[y * ps + x];
  }
}

// phase 2: y pass and dynamic step for columns [band * kBand, ...) of one pattern; d -> dst,
// the band's {min, max} -> part[(b * nbands + band) * 2]
template <typename T>
__global__ __launch_bounds__(kCorrThreads) void correct_ypass_kernel(const T* __restrict__ src,
                                                                     CorrArgs a, int nbands,
                                                                     const float* __restrict__ xplane,
                                                                     float* __restrict__ dst,
                                                                     float* __restrict__ part) {
  extern __shared__ float planes[];   // X columns (oh x pc)
  __shared__ float win[kTapWin];
  __shared__ float red[2 * kCorrWaves];
  constexpr int pc = kBand | 1;
  const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
  const int oh = a.oh, ow = a.ow;
  const int x0 = band * kBand, cols = min(kBand, ow - x0);
  const T* pat = src + (size_t)b * a.H0 * a.W0;
  float* out = dst + (size_t)b * oh * ow;
  float lo = INFINITY, hi = -INFINITY;
  if (a.dmode != 0) {
    stage_taps(win, a);
    const float* xin = xplane + (size_t)b * oh * ow;
    for (int i = threadIdx.x; i < oh * cols; i += blockDim.x) {
      const int y = i / cols, x = i - y * cols;
      planes[y * pc + x] = xin[(size_t)y * ow + x0 + x];
    }
    __syncthreads();
    const int items = cols * ((oh + kRun - 1) / kRun);
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
      const int x = it % cols, yr = (it / cols) * kRun;
      float acc[kRun];
      blur_run(planes + x, pc, oh, yr, win, a.radius, acc);
#pragma unroll
      for (int k = 0; k < kRun; ++k)
        if (yr + k < oh) {
          const float d = dynamic_step(load_static(pat, a, yr + k, x0 + x), acc[k], a.dmode);
          out[(size_t)(yr + k) * ow + x0 + x] = d;
          lo = fminf(lo, d), hi = fmaxf(hi, d);
        }
    }
  } else {
    for (int i = threadIdx.x; i < oh * cols; i += blockDim.x) {
      const int y = i / cols, x = i - y * cols;
      const float d = load_static(pat, a, y, x0 + x);
      out[(size_t)y * ow + x0 + x] = d;
      lo = fminf(lo, d), hi = fmaxf(hi, d);
    }
  }
  block_minmax(lo, hi, red);
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x * 2] = lo;
    part[(size_t)blockIdx.x * 2 + 1] = hi;
  }
}

// phase 3: the pattern's min / max from its bands (in band order), dst rescaled in place
__global__ __launch_bounds__(256) void correct_rescale_kernel(float* __restrict__ dst,
                                                              const float* __restrict__ part,
                                                              int nbands, int n, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float* p = part + (i / n) * nbands * 2;
  float lo = p[0], hi = p[1];
  for (int k = 1; k < nbands; ++k) lo = fminf(lo, p[2 * k]), hi = fmaxf(hi, p[2 * k + 1]);
  dst[i] = rescale(dst[i], lo, hi);
}

// acc[p] += sum over the batch, in batch order, of float64(src[b][p]): one thread per pixel
template <typename T>
__global__ __launch_bounds__(256) void accumulate_kernel(const T* __restrict__ src, int B, int npx,
                                                         double* __restrict__ acc) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  double s = acc[p];
#pragma unroll 8
  for (int b = 0; b < B; ++b) s += (double)src[(size_t)b * npx + p];
  acc[p] = s;
}

static int col_bands(int ow) { return (ow + kBand - 1) / kBand; }
static bool fused_path(int oh, int ow) { return (long long)oh * ow <= kFusedMaxPx; }

// more than 64 KiB of dynamic LDS has to be allowed per kernel; the kernels' static arrays
// (taps, reduction) come on top, so the allowance is what the launch asks for, not all 160 KiB
template <typename K>
static bool allow_lds(K k, size_t bytes) {
  return bytes <= 64 * 1024 ||
         hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes) == hipSuccess;
}

template <typename T>
static bool launch_correct(const T* src, const CorrArgs& a, int B, float* dst, float* work,
                           hipStream_t st) {
  const int oh = a.oh, ow = a.ow, ps = ow | 1;
  if (fused_path(oh, ow)) {
    const size_t lds = (size_t)2 * oh * ps * sizeof(float);
    if (!allow_lds(correct_fused_kernel<T>, lds)) return false;
    hipLaunchKernelGGL(correct_fused_kernel<T>, dim3(B), dim3(kCorrThreads), lds, st, src, a, dst);
    return true;
  }
  const int rb = (oh + kBand - 1) / kBand, cb = col_bands(ow);
  float* xplane = work;
  float* part = work + (size_t)B * oh * ow;
  if (a.dmode != 0) {
    const size_t lds = (size_t)2 * kBand * ps * sizeof(float);
    if (!allow_lds(correct_xpass_kernel<T>, lds)) return false;
    hipLaunchKernelGGL(correct_xpass_kernel<T>, dim3((unsigned)B * rb), dim3(kCorrThreads), lds, st,
                       src, a, rb, xplane);
  }
  const size_t lds = (size_t)oh * (kBand | 1) * sizeof(float);
  if (!allow_lds(correct_ypass_kernel<T>, lds)) return false;
  hipLaunchKernelGGL(correct_ypass_kernel<T>, dim3((unsigned)B * cb), dim3(kCorrThreads), lds, st,
                     src, a, cb, xplane, dst, part);
  const long long total = (long long)B * oh * ow;
  hipLaunchKernelGGL(correct_rescale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     dst, part, cb, oh * ow, total);
  return true;
}

}  // namespace ev

using namespace ev;

extern "C" size_t ebsdvae_correct_patterns_work(int B, int out_h, int out_w) {
  if (B <= 0 || out_h <= 0 || out_w <= 0 || out_h > kCorrMaxSide || out_w > kCorrMaxSide) return 0;
  if (fused_path(out_h, out_w)) return 0;
  return ((size_t)B * out_h * out_w + (size_t)B * col_bands(out_w) * 2) * sizeof(float);
}

extern "C" int ebsdvae_correct_patterns(const void* src, int src_dtype, int B, int H0, int W0,
                                        int out_h, int out_w, const float* static_bg,
                                        int static_mode, const float* taps, int radius,
                                        int dynamic_mode, float* dst, void* work,
                                        ebsdvae_stream_t stream) {
  EV_REQUIRE(src && dst && B >= 0 && H0 > 0 && W0 > 0 && out_h > 0 && out_w > 0,
             "correct_patterns: bad args");
  EV_REQUIRE(src_dtype >= 0 && src_dtype <= 2, "correct_patterns: src_dtype %d (0 f64, 1 f32, 2 u8)",
             src_dtype);
  EV_REQUIRE(out_h <= kCorrMaxSide && out_w <= kCorrMaxSide,
             "correct_patterns: window %dx%d larger than %dx%d", out_h, out_w, kCorrMaxSide,
             kCorrMaxSide);
  EV_REQUIRE(H0 >= out_h && W0 >= out_w,
             "correct_patterns: the %dx%d window does not fit the %dx%d pattern (no padding)", out_h,
             out_w, H0, W0);
  EV_REQUIRE((long long)H0 * W0 < (1LL << 31) && (long long)B * col_bands(out_w) < (1LL << 24),
             "correct_patterns: pattern or batch too large");
  EV_REQUIRE(static_mode >= 0 && static_mode <= 2 && (static_mode != 0) == (static_bg != nullptr),
             "correct_patterns: static_mode %d needs %s background", static_mode,
             static_mode ? "a" : "no");
  EV_REQUIRE(dynamic_mode >= 0 && dynamic_mode <= 2 && (dynamic_mode != 0) == (taps != nullptr),
             "correct_patterns: dynamic_mode %d needs %s taps", dynamic_mode,
             dynamic_mode ? "the" : "no");
  EV_REQUIRE(dynamic_mode == 0 || (radius >= 0 && radius <= out_h && radius <= out_w),
             "correct_patterns: radius %d outside [0, min(%d, %d)]", radius, out_h, out_w);
  if (B == 0) return 0;
  EV_REQUIRE(fused_path(out_h, out_w) || work != nullptr,
             "correct_patterns: a %dx%d window needs the work buffer", out_h, out_w);
  CorrArgs a;
  a.H0 = H0, a.W0 = W0, a.oh = out_h, a.ow = out_w;
  a.top = crop_offset(H0, out_h), a.left = crop_offset(W0, out_w);
  a.bg = static_bg, a.taps = taps;
  a.smode = static_mode, a.dmode = dynamic_mode, a.radius = dynamic_mode ? radius : 0;
  const hipStream_t st = (hipStream_t)stream;
  bool ok = false;
  evh::with_src(src, src_dtype, [&](auto p) { ok = launch_correct(p, a, B, dst, (float*)work, st); });
  if (!ok) {
    (void)hipGetLastError();
    evh::set_error("correct_patterns: the device refused the LDS a %dx%d window needs", out_h, out_w);
    return 2;
  }
  return evh::check_launch("correct_patterns");
}

extern "C" int ebsdvae_accumulate_patterns(const void* src, int src_dtype, int B, int H0, int W0,
                                           double* acc, ebsdvae_stream_t stream) {
  EV_REQUIRE(src && acc && B >= 0 && H0 > 0 && W0 > 0, "accumulate_patterns: bad args");
  EV_REQUIRE(src_dtype >= 0 && src_dtype <= 2,
             "accumulate_patterns: src_dtype %d (0 f64, 1 f32, 2 u8)", src_dtype);
  EV_REQUIRE((long long)H0 * W0 < (1LL << 31), "accumulate_patterns: pattern too large");
  if (B == 0) return 0;
  const int npx = H0 * W0;
  const dim3 grid((unsigned)((npx + 255) / 256));
  const hipStream_t st = (hipStream_t)stream;
  evh::with_src(src, src_dtype, [&](auto p) {
    hipLaunchKernelGGL(accumulate_kernel<evh::elem_t<decltype(p)>>, grid, dim3(256), 0, st, p, B, npx, acc);
  });
  return evh::check_launch("accumulate_patterns");
}
