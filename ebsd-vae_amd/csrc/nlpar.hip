// NLPAR, non-local pattern averaging and re-weighting ("Non-local pattern
// averaging"): the neighbour averaging of csrc/neighbour.hip with weights that differ per output.
// Pattern p at (i, j) = (p / cols, p % cols), n = h w pixels, D(p, q) = sum (T[p] - T[q])^2:
//
//   s_p   = max(min D(p, q) / (2 n), sigma_floor^2) over the on-grid 3 x 3 ring of p
//           (sigma_floor^2 without a ring; sigma^2 for every p when sigma is given)
//   v     = s_p + s_q,  d = max((D(p, q) - n v) / (v sqrt(2 n)), 0)
//   Wt[p][a][b] = exp(-d / lam^2), 0 where d > dthresh, 0 off the grid, 1 at the centre
//   A[p]  = sum Wt[p][a][b] T[q] / sum Wt[p][a][b]      the fma chains of neighbour.hip
//
// Four kernels.  nlpar_distance_kernel is the hot one and has neighbour_kernel's structure: a
// thread owns a float4 of pixels and slides along a scan row with the distance window's columns
// in registers; per centre and offset it squares its four differences, the wave sums them by
// xor shuffles and the block's four waves through the LDS: one float32 partial per (centre,
// offset, block of 1024 pixels).  The pixel set of a partial and the order of every addition in
// it are fixed by the pixel block alone, never by the launch, and (x - y)^2 == (y - x)^2, so a
// partial is a function of the two patterns.  nlpar_sigma_kernel and nlpar_weights_kernel add
// the partials in ascending block order in double, round D to float32 once and finish in
// float32 with expf / sqrtf and true divisions, contraction off.  No atomics anywhere.
// nlpar_average_kernel is neighbour_kernel with the weights read per output: their address is
// the same in every lane, so they are scalar loads into scalar registers.
//
// The distance window is the averaging window widened to at least 3 x 3 (the ring of s_p).  The
// weights of outputs [p0, p0 + count) need s_q of every pattern of their windows, so distances
// are formed around every centre of the flat range [p0 - (hr cols + hc), p0 + count + (hr cols
// + hc)) on the grid; what is read lies within (hr + 1) cols + (hc + 1) of the outputs.
// Nothing off the grid is ever addressed: such a tap counts as the value 0 and its distance is
// never used.
#include "common.h"
#include "../../include/ebsdvae.h"

#include <math.h>

namespace ev {

constexpr int kNlThreads = 256;          // 1024 pixels per block: the pixel set of one partial
constexpr int kNlWaves = kNlThreads / 64;
constexpr int kNlMaxHalf = 2;            // windows up to 5 x 5
constexpr int kNlRun = 16;               // outputs a thread walks along a scan row, as neighbour.hip

struct NlDistArgs {
  const float* src;       // ring of `cap` patterns, pattern q in slot q % cap
  float* dpart;           // (e1 - e0, NA * NB, pb) partial distances
  long long e0, e1;       // the centres
  int cap, rows, cols, hw4, run, chunks, row0, pb;
};

template <int HR, int HC>
__global__ __launch_bounds__(kNlThreads) void nlpar_distance_kernel(const NlDistArgs g) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1, NOFF = NA * NB;
  __shared__ float red[2][kNlWaves][NOFF];
  const int f = blockIdx.y * kNlThreads + threadIdx.x;   // this thread's float4 of pixels
  const bool px_ok = f < g.hw4;                          // past the pattern: zeros, nothing read
  // the run: scan row i, columns [lo, hi) of the column chunk, clipped to [e0, e1)
  const int i = g.row0 + (int)(blockIdx.x / (unsigned)g.chunks);
  const int c0 = (int)(blockIdx.x % (unsigned)g.chunks) * g.run;
  const long long rowbase = (long long)i * g.cols;
  const long long first = g.e0 - rowbase, last = g.e1 - rowbase;
  const int lo = first > c0 ? (int)first : c0;
  const int end = c0 + g.run < g.cols ? c0 + g.run : g.cols;
  const int hi = last < end ? (int)last : end;
  if (lo >= hi) return;   // the same in every thread of the block

  bool row_ok[NA];     // the neighbour row is on the grid
  int slot[NA];        // ring slot of the next column this row loads
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int r = i + a - HR;
    row_ok[a] = r >= 0 && r < g.rows;
    long long q = ((long long)r * g.cols + (lo - HC)) % g.cap;   // q may be negative
    slot[a] = (int)(q < 0 ? q + g.cap : q);
  }

  const size_t hw = (size_t)g.hw4 * 4;
  const float* src = g.src + (size_t)(px_ok ? f : 0) * 4;
  float4 win[NB][NA];   // win[k]: the column whose offset from lo - HC is k modulo NB

  // load grid column c into win[k]; what is not on the grid is not read and counts as 0
  auto load_column = [&](int k, int c) EV_LAMBDA_INLINE {
    const bool col_ok = px_ok && c >= 0 && c < g.cols;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      if (col_ok && row_ok[a]) win[k][a] = ld4(src + (size_t)slot[a] * hw);
      else win[k][a] = make_float4(0.f, 0.f, 0.f, 0.f);
      slot[a] = slot[a] + 1 == g.cap ? 0 : slot[a] + 1;
    }
  };

#pragma unroll
  for (int k = 0; k < NB - 1; ++k) load_column(k, lo - HC + k);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = hi - lo;
  for (int t0 = 0; t0 < n; t0 += NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (t0 + u >= n) break;
      const int j = lo + t0 + u;
      load_column((u + NB - 1) % NB, j + HC);
      const float4 c = win[(u + HC) % NB][HR];
      // two LDS buffers by the centre's parity: one barrier per centre is enough
      float(*rk)[NOFF] = red[(t0 + u) & 1];
#pragma unroll
      for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (a == HR && b == HC) continue;
          const float4 v = win[(u + b) % NB][a];
          const float dx = c.x - v.x, dy = c.y - v.y, dz = c.z - v.z, dw = c.w - v.w;
          float s = dx * dx;
          s = fmaf(dy, dy, s);
          s = fmaf(dz, dz, s);
          s = fmaf(dw, dw, s);
          s = wave_sum(s);
          if (lane == 0) rk[wave][a * NB + b] = s;
        }
      }
      __syncthreads();
      if (threadIdx.x < NOFF) {
        const int o = threadIdx.x;
        const float tot = o == HR * NB + HC ? 0.f : (rk[0][o] + rk[1][o]) + (rk[2][o] + rk[3][o]);
        g.dpart[((size_t)(rowbase + j - g.e0) * NOFF + o) * g.pb + blockIdx.y] = tot;
      }
    }
  }
}

struct NlFinArgs {
  const float* dpart;     // (e1 - e0, NA * NB, pb), the distance window (HRD, HCD)
  float* s;               // (e1 - e0,) noise variances
  float* weights;         // (count, 2 hr + 1, 2 hc + 1)
  float* sigma;           // (count,) or null
  long long e0, e1, p0, count;
  int rows, cols, pb, hr, hc, hrd, hcd;
  float n, two_n, sqrt_two_n;   // h w, 2 h w and sqrtf(2 h w)
  float s_fixed;                // sigma^2, or 0: estimate
  float floor2, lam2;           // sigma_floor^2, lam^2
  float dthresh;                // < 0: no threshold
};

// D(centre e0 + c, offset o of the distance window) as float32: the partials in ascending
// block order, in double, rounded once
EV_DEVINL float nl_distance(const NlFinArgs& g, long long c, int o) {
  const float* p = g.dpart + ((size_t)c * (2 * g.hrd + 1) * (2 * g.hcd + 1) + o) * g.pb;
  double d = 0.0;
  for (int k = 0; k < g.pb; ++k) d += (double)p[k];
  return (float)d;
}

__global__ __launch_bounds__(kNlThreads) void nlpar_sigma_kernel(const NlFinArgs g) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * kNlThreads + threadIdx.x;
  if (c >= g.e1 - g.e0) return;
  float s = g.s_fixed;
  if (!(s > 0.f)) {
    const int i = (int)((g.e0 + c) / g.cols), j = (int)((g.e0 + c) % g.cols);
    bool any = false;
    float m = 0.f;
    for (int a = -1; a <= 1; ++a) {
      for (int b = -1; b <= 1; ++b) {
        if ((a == 0 && b == 0) || i + a < 0 || i + a >= g.rows || j + b < 0 || j + b >= g.cols)
          continue;
        const float d = nl_distance(g, c, (a + g.hrd) * (2 * g.hcd + 1) + (b + g.hcd));
        m = any ? fminf(m, d) : d;
        any = true;
      }
    }
    s = any ? fmaxf(m / g.two_n, g.floor2) : g.floor2;
  }
  g.s[c] = s;
}

__global__ __launch_bounds__(kNlThreads) void nlpar_weights_kernel(const NlFinArgs g) {
#pragma clang fp contract(off)
  const int nb = 2 * g.hc + 1, noff = (2 * g.hr + 1) * nb;
  const long long t = (long long)blockIdx.x * kNlThreads + threadIdx.x;
  if (t >= g.count * noff) return;
  const long long p = g.p0 + t / noff;
  const int o = (int)(t % noff), a = o / nb - g.hr, b = o % nb - g.hc;
  const int i = (int)(p / g.cols), j = (int)(p % g.cols);
  const float sp = g.s[p - g.e0];
  float w;
  if (a == 0 && b == 0) {
    w = 1.f;
    if (g.sigma) g.sigma[p - g.p0] = sqrtf(sp);
  } else if (i + a < 0 || i + a >= g.rows || j + b < 0 || j + b >= g.cols) {
    w = 0.f;
  } else {
    const long long q = p + (long long)a * g.cols + b;   // in [e0, e1): within hr cols + hc of p
    const float v = sp + g.s[q - g.e0];
    const float D = nl_distance(g, p - g.e0, (a + g.hrd) * (2 * g.hcd + 1) + (b + g.hcd));
    const float d = fmaxf((D - g.n * v) / (v * g.sqrt_two_n), 0.f);
    w = expf(-d / g.lam2);
    if (g.dthresh >= 0.f && d > g.dthresh) w = 0.f;
  }
  g.weights[t] = w;
}

struct NlAvgArgs {
  const float* src;       // ring of `cap` patterns, pattern q in slot q % cap
  float* dst;             // count patterns
  long long p0, count;
  int cap, rows, cols, hw4, run, chunks, row0;
};

// neighbour_kernel (csrc/neighbour.hip) with per-output weights (count, NA, NB): 0 off the grid
// and where the threshold cut, so a dropped tap enters its chain with weight 0
template <int HR, int HC>
__global__ __launch_bounds__(kNlThreads) void nlpar_average_kernel(
    const NlAvgArgs g, const float* __restrict__ weights) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1;
  const int f = blockIdx.y * kNlThreads + threadIdx.x;   // this thread's float4 of pixels
  const int i = g.row0 + (int)(blockIdx.x / (unsigned)g.chunks);
  const int c0 = (int)(blockIdx.x % (unsigned)g.chunks) * g.run;
  const long long rowbase = (long long)i * g.cols;
  const long long first = g.p0 - rowbase, last = g.p0 + g.count - rowbase;
  const int lo = first > c0 ? (int)first : c0;
  const int end = c0 + g.run < g.cols ? c0 + g.run : g.cols;
  const int hi = last < end ? (int)last : end;
  if (lo >= hi || f >= g.hw4) return;

  bool row_ok[NA];     // the neighbour row is on the grid
  int slot[NA];        // ring slot of the next column this row loads
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int r = i + a - HR;
    row_ok[a] = r >= 0 && r < g.rows;
    long long q = ((long long)r * g.cols + (lo - HC)) % g.cap;   // q may be negative
    slot[a] = (int)(q < 0 ? q + g.cap : q);
  }

  const size_t hw = (size_t)g.hw4 * 4;
  const float* src = g.src + (size_t)f * 4;
  float* dst = g.dst + ((size_t)(rowbase + lo - g.p0) * g.hw4 + f) * 4;
  // the same address in every lane and nothing in this launch writes them: read through the
  // constant address space, the weights arrive by scalar loads in scalar registers
  typedef const float __attribute__((address_space(4))) * uniform_floats;
  uniform_floats wt = (uniform_floats)(weights + (size_t)(rowbase + lo - g.p0) * (NA * NB));
  float4 win[NB][NA];   // win[k]: the column whose offset from lo - HC is k modulo NB

  auto load_column = [&](int k, int c) EV_LAMBDA_INLINE {
    const bool col_ok = c >= 0 && c < g.cols;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      if (col_ok && row_ok[a]) win[k][a] = ld4(src + (size_t)slot[a] * hw);
      else win[k][a] = make_float4(0.f, 0.f, 0.f, 0.f);
      slot[a] = slot[a] + 1 == g.cap ? 0 : slot[a] + 1;
    }
  };

#pragma unroll
  for (int k = 0; k < NB - 1; ++k) load_column(k, lo - HC + k);

  const int n = hi - lo;
  for (int t0 = 0; t0 < n; t0 += NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (t0 + u >= n) break;
      load_column((u + NB - 1) % NB, lo + t0 + u + HC);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      float ws = 0.f;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float wv = wt[a * NB + b];   // 0 off the grid: fma(0, 0, s) == s
          const float4 v = win[(u + b) % NB][a];
          acc.x = fmaf(wv, v.x, acc.x);
          acc.y = fmaf(wv, v.y, acc.y);
          acc.z = fmaf(wv, v.z, acc.z);
          acc.w = fmaf(wv, v.w, acc.w);
          ws = fmaf(wv, 1.f, ws);
        }
      }
      st4(dst, make_float4(acc.x / ws, acc.y / ws, acc.z / ws, acc.w / ws));
      dst += hw;
      wt += NA * NB;
    }
  }
}

// what the three entry points check alike; `who` names the caller in the message
static int nl_check_shape(const char* who, int rows, int cols, int hr, int hc, int h, int w) {
  EV_REQUIRE(hr >= 0 && hr <= kNlMaxHalf && hc >= 0 && hc <= kNlMaxHalf,
             "%s: half widths hr=%d hc=%d outside 0..%d", who, hr, hc, kNlMaxHalf);
  EV_REQUIRE(rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31), "%s: grid %d x %d", who,
             rows, cols);
  EV_REQUIRE(h > 0 && w > 0 && (long long)h * w < (1LL << 24) && ((long long)h * w) % 4 == 0,
             "%s: h*w = %lld must be a positive multiple of 4 below 2^24", who, (long long)h * w);
  return 0;
}

static long long nl_min(long long a, long long b) { return a < b ? a : b; }
static int nl_pixel_blocks(int h, int w) { return (h * w / 4 + kNlThreads - 1) / kNlThreads; }
// centres of `count` outputs at most, distance-window offsets, pixel blocks
static void nl_plan(int rows, int cols, long long count, int hr, int hc, int h, int w,
                    long long* centres, int* noff, int* pb) {
  *centres = nl_min((long long)rows * cols, count + 2 * ((long long)hr * cols + hc));
  *noff = (2 * (hr > 1 ? hr : 1) + 1) * (2 * (hc > 1 ? hc : 1) + 1);
  *pb = nl_pixel_blocks(h, w);
}

}  // namespace ev

using namespace ev;

extern "C" size_t ebsdvae_nlpar_work(int rows, int cols, long long count, int hr, int hc, int h,
                                     int w) {
  if (nl_check_shape("nlpar_work", rows, cols, hr, hc, h, w)) return 0;
  if (count < 0 || count > (long long)rows * cols) return 0;
  long long centres;
  int noff, pb;
  nl_plan(rows, cols, count, hr, hc, h, w, &centres, &noff, &pb);
  // the partials, the variances, and 16 bytes so that an accepted shape never answers 0
  return (size_t)centres * ((size_t)noff * pb + 1) * sizeof(float) + 16;
}

extern "C" int ebsdvae_nlpar_weights(const float* src, long long ring_cap, int rows, int cols,
                                     long long p0, long long count, int hr, int hc, int h, int w,
                                     double lam, int fixed_sigma, double sigma, double sigma_floor,
                                     int cut, double dthresh, float* weights, float* sigma_out,
                                     void* work, ebsdvae_stream_t stream) {
  if (nl_check_shape("nlpar_weights", rows, cols, hr, hc, h, w)) return 1;
  EV_REQUIRE(src && weights && work, "nlpar_weights: null pointer");
  EV_REQUIRE(lam > 0.0 && isfinite(lam), "nlpar_weights: lam=%g must be positive", lam);
  EV_REQUIRE(!fixed_sigma || (sigma > 0.0 && isfinite(sigma)),
             "nlpar_weights: sigma=%g must be positive", sigma);
  EV_REQUIRE(sigma_floor > 0.0 && isfinite(sigma_floor),
             "nlpar_weights: sigma_floor=%g must be positive", sigma_floor);
  EV_REQUIRE(!cut || (dthresh >= 0.0 && isfinite(dthresh)),
             "nlpar_weights: dthresh=%g must not be negative", dthresh);
  const long long n = (long long)rows * cols;
  EV_REQUIRE(count >= 0 && p0 >= 0 && p0 <= n && count <= n - p0,
             "nlpar_weights: range [%lld, %lld + %lld) leaves the %d x %d grid", p0, p0, count,
             rows, cols);
  const long long reach_w = (long long)hr * cols + hc;
  const long long need = count + 2 * ((long long)(hr + 1) * cols + (hc + 1));
  EV_REQUIRE(ring_cap >= nl_min(need, n) && ring_cap < (1LL << 31),
             "nlpar_weights: ring of %lld patterns, %lld outputs of this window need %lld",
             ring_cap, count, nl_min(need, n));
  if (count == 0) return 0;

  long long centres;
  int noff, pb;
  nl_plan(rows, cols, count, hr, hc, h, w, &centres, &noff, &pb);
  const long long e0 = p0 > reach_w ? p0 - reach_w : 0, e1 = nl_min(n, p0 + count + reach_w);
  // e1 - e0 <= centres: what ebsdvae_nlpar_work sized the scratch for
  float* dpart = (float*)work;
  float* s = dpart + (size_t)centres * noff * pb;
  hipStream_t st = (hipStream_t)stream;
  const int hrd = hr > 1 ? hr : 1, hcd = hc > 1 ? hc : 1;

  if (!fixed_sigma || hr + hc > 0) {   // a fixed sigma under a 1 x 1 window needs no distance
    NlDistArgs g;
    g.src = src, g.dpart = dpart, g.e0 = e0, g.e1 = e1;
    g.cap = (int)ring_cap, g.rows = rows, g.cols = cols;
    g.hw4 = h * w / 4, g.pb = pb;
    g.run = kNlRun < cols ? kNlRun : cols;
    g.chunks = (cols + g.run - 1) / g.run;
    g.row0 = (int)(e0 / cols);
    const long long runs = ((e1 - 1) / cols - g.row0 + 1) * g.chunks;
    EV_REQUIRE(runs < (1LL << 31) && pb <= 65535, "nlpar_weights: launch too large");
    const dim3 grid((unsigned)runs, (unsigned)pb);
    evh::with_const<1, 2>(hrd, [&](auto HRc) {
      evh::with_const<1, 2>(hcd, [&](auto HCc) {
        hipLaunchKernelGGL((nlpar_distance_kernel<decltype(HRc)::value, decltype(HCc)::value>),
                           grid, dim3(kNlThreads), 0, st, g);
      });
    });
  }

  NlFinArgs g;
  g.dpart = dpart, g.s = s, g.weights = weights, g.sigma = sigma_out;
  g.e0 = e0, g.e1 = e1, g.p0 = p0, g.count = count;
  g.rows = rows, g.cols = cols, g.pb = pb, g.hr = hr, g.hc = hc, g.hrd = hrd, g.hcd = hcd;
  g.n = (float)(h * w), g.two_n = (float)(2 * h * w), g.sqrt_two_n = sqrtf((float)(2 * h * w));
  g.s_fixed = fixed_sigma ? (float)(sigma * sigma) : 0.f;
  g.floor2 = (float)(sigma_floor * sigma_floor);
  g.lam2 = (float)(lam * lam);
  g.dthresh = cut ? (float)dthresh : -1.f;
  EV_REQUIRE(!fixed_sigma || g.s_fixed > 0.f, "nlpar_weights: sigma=%g squares to 0", sigma);
  EV_REQUIRE(g.floor2 > 0.f && g.lam2 > 0.f && isfinite(g.lam2),
             "nlpar_weights: sigma_floor=%g or lam=%g leaves float32", sigma_floor, lam);
  const long long nw = count * (2 * hr + 1) * (2 * hc + 1);
  EV_REQUIRE(nw < (1LL << 31) * kNlThreads, "nlpar_weights: launch too large");
  hipLaunchKernelGGL(nlpar_sigma_kernel, dim3((unsigned)((e1 - e0 + kNlThreads - 1) / kNlThreads)),
                     dim3(kNlThreads), 0, st, g);
  hipLaunchKernelGGL(nlpar_weights_kernel, dim3((unsigned)((nw + kNlThreads - 1) / kNlThreads)),
                     dim3(kNlThreads), 0, st, g);
  return evh::check_launch("nlpar_weights");
}

extern "C" int ebsdvae_nlpar_average(const float* src, long long ring_cap, int rows, int cols,
                                     long long p0, long long count, const float* weights, int hr,
                                     int hc, int h, int w, float* dst, ebsdvae_stream_t stream) {
  if (nl_check_shape("nlpar_average", rows, cols, hr, hc, h, w)) return 1;
  EV_REQUIRE(src && weights && dst, "nlpar_average: null pointer");
  const long long n = (long long)rows * cols;
  EV_REQUIRE(count >= 0 && p0 >= 0 && p0 <= n && count <= n - p0,
             "nlpar_average: range [%lld, %lld + %lld) leaves the %d x %d grid", p0, p0, count,
             rows, cols);
  const long long need = count + 2 * ((long long)hr * cols + hc);
  EV_REQUIRE(ring_cap >= nl_min(need, n) && ring_cap < (1LL << 31),
             "nlpar_average: ring of %lld patterns, %lld outputs of this window need %lld",
             ring_cap, count, nl_min(need, n));
  if (count == 0) return 0;

  NlAvgArgs g;
  g.src = src, g.dst = dst, g.p0 = p0, g.count = count;
  g.cap = (int)ring_cap, g.rows = rows, g.cols = cols;
  g.hw4 = h * w / 4;
  g.run = kNlRun < cols ? kNlRun : cols;
  g.chunks = (cols + g.run - 1) / g.run;
  g.row0 = (int)(p0 / cols);
  const long long runs = ((p0 + count - 1) / cols - g.row0 + 1) * g.chunks;
  const int pxblocks = nl_pixel_blocks(h, w);
  EV_REQUIRE(runs < (1LL << 31) && pxblocks <= 65535, "nlpar_average: launch too large");
  const dim3 grid((unsigned)runs, (unsigned)pxblocks);
  evh::with_const<0, 1, 2>(hr, [&](auto HRc) {
    evh::with_const<0, 1, 2>(hc, [&](auto HCc) {
      hipLaunchKernelGGL((nlpar_average_kernel<decltype(HRc)::value, decltype(HCc)::value>), grid,
                         dim3(kNlThreads), 0, (hipStream_t)stream, g, weights);
    });
  });
  return evh::check_launch("nlpar_average");
}
