// NLPAR, non-local pattern averaging and re-weighting ("Non-local pattern
// averaging"): the neighbour averaging of csrc/neighbour.hip with weights that differ per output.
// Pattern p at (i, j) = (p / cols, p % cols), n = h w pixels, D(p, q) = sum (T[p] - T[q])^2:
//   s_p   = max(min D(p, q) / (2 n), sigma_floor^2) over the on-grid 3 x 3 ring of p
//           (sigma_floor^2 without a ring; sigma^2 for every p when sigma is given)
//   v     = s_p + s_q,  d = max((D(p, q) - n v) / (v sqrt(2 n)), 0)
//   Wt[p][a][b] = exp(-d / lam^2), 0 where d > dthresh, 0 off the grid, 1 at the centre
//   A[p]  = sum Wt[p][a][b] T[q] / sum Wt[p][a][b]      the fma chains of neighbour.hip
// nlpar_distance_kernel walks the distance window (the averaging window widened to the 3 x 3
// ring of s_p) around every centre within hr cols + hc of the outputs: one float32 partial per
// (centre, offset, block of 1024 pixels), fixed by the pixel block alone.  nlpar_sigma_kernel and
// nlpar_weights_kernel add the partials in block order in double and finish in float32,
// contraction off; nlpar_average_kernel is neighbour.hip's chain with per-output weights.
#include "scan_window.h"
#include "../../include/ebsdvae.h"
#include <math.h>

namespace ev {

constexpr int kNlThreads = kSwThreads;   // 1024 pixels per block: the pixel set of one partial
constexpr int kNlWaves = kNlThreads / 64;
constexpr int kNlRun = 16;               // outputs a thread walks along a scan row, as neighbour.hip

// dpart: (centres, NA * NB, pb) partial distances of the centres [g.first, g.last)
template <int HR, int HC>
__global__ __launch_bounds__(kNlThreads) void nlpar_distance_kernel(const ScanWalk g, float* dpart,
                                                                    int pb) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1, NOFF = NA * NB;
  __shared__ float red[2][kNlWaves][NOFF];
  const int f = blockIdx.y * kNlThreads + threadIdx.x;   // this thread's float4 of pixels
  // past the pattern: zeros, nothing read.  No early return: the whole block meets the barrier
  const bool px_ok = f < g.hw4;
  const ScanRun r = scan_run(g);
  if (r.lo >= r.hi) return;   // the same in every thread of the block

  walk_scan_window<HR, HC>(
      g, r, f, px_ok, [](int, bool on_grid) EV_LAMBDA_INLINE { return on_grid; },
      [&](int j, int u, const float4(&win)[NB][NA]) EV_LAMBDA_INLINE {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const float4 c = win[(u + HC) % NB][HR];
        // two LDS buffers by the centre's parity: one barrier per centre is enough
        float(*rk)[NOFF] = red[(j - r.lo) & 1];
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
          dpart[((size_t)(r.rowbase + j - g.first) * NOFF + o) * pb + blockIdx.y] = tot;
        }
      });
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

// the walk with neighbour.hip's chain and per-output weights (count, NA, NB): 0 off the grid
// and where the threshold cut, so a dropped tap enters its chain with weight 0
template <int HR, int HC>
__global__ __launch_bounds__(kNlThreads) void nlpar_average_kernel(
    const ScanWalk g, const float* __restrict__ weights, float* out) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1;
  const int f = blockIdx.y * kNlThreads + threadIdx.x;   // this thread's float4 of pixels
  const ScanRun r = scan_run(g);
  if (r.lo >= r.hi || f >= g.hw4) return;

  // the same address in every lane and nothing in this launch writes them: read through the
  // constant address space, the weights arrive by scalar loads in scalar registers
  typedef const float __attribute__((address_space(4))) * uniform_floats;
  uniform_floats wt = (uniform_floats)(weights + (size_t)(r.rowbase + r.lo - g.first) * (NA * NB));
  walk_and_average<HR, HC>(
      g, r, f, out, [](int, bool on_grid) EV_LAMBDA_INLINE { return on_grid; },
      [&](int, int a, int b) EV_LAMBDA_INLINE { return wt[a * NB + b]; },   // 0 off the grid
      [&]() EV_LAMBDA_INLINE { wt += NA * NB; });
}

static long long nl_min(long long a, long long b) { return a < b ? a : b; }
// centres of `count` outputs at most, distance-window offsets, pixel blocks
struct NlPlan { long long centres; int noff, pb; };
static NlPlan nl_plan(int rows, int cols, long long count, int hr, int hc, int h, int w) {
  return {nl_min((long long)rows * cols, count + 2 * ((long long)hr * cols + hc)),
          (2 * (hr > 1 ? hr : 1) + 1) * (2 * (hc > 1 ? hc : 1) + 1),
          (h * w / 4 + kNlThreads - 1) / kNlThreads};
}

}  // namespace ev

using namespace ev;

extern "C" size_t ebsdvae_nlpar_work(int rows, int cols, long long count, int hr, int hc, int h,
                                     int w) {
  if (evh::check_scan_shape("nlpar_work", true, rows, cols, hr, hc, h, w, true)) return 0;
  if (count < 0 || count > (long long)rows * cols) return 0;
  const NlPlan pl = nl_plan(rows, cols, count, hr, hc, h, w);
  // the partials, the variances, and 16 bytes so that an accepted shape never answers 0
  return (size_t)pl.centres * ((size_t)pl.noff * pl.pb + 1) * sizeof(float) + 16;
}

extern "C" int ebsdvae_nlpar_weights(const float* src, long long ring_cap, int rows, int cols,
                                     long long p0, long long count, int hr, int hc, int h, int w,
                                     double lam, int fixed_sigma, double sigma, double sigma_floor,
                                     int cut, double dthresh, float* weights, float* sigma_out,
                                     void* work, ebsdvae_stream_t stream) {
  const char* who = "nlpar_weights";
  if (evh::check_scan_shape(who, src && weights && work, rows, cols, hr, hc, h, w, true)) return 1;
  EV_REQUIRE(lam > 0.0 && isfinite(lam), "nlpar_weights: lam=%g must be positive", lam);
  EV_REQUIRE(!fixed_sigma || (sigma > 0.0 && isfinite(sigma)),
             "nlpar_weights: sigma=%g must be positive", sigma);
  EV_REQUIRE(sigma_floor > 0.0 && isfinite(sigma_floor),
             "nlpar_weights: sigma_floor=%g must be positive", sigma_floor);
  EV_REQUIRE(!cut || (dthresh >= 0.0 && isfinite(dthresh)),
             "nlpar_weights: dthresh=%g must not be negative", dthresh);
  // what is read lies within (hr + 1) cols + (hc + 1) of the outputs
  const long long n = (long long)rows * cols, reach_w = (long long)hr * cols + hc;
  if (evh::check_scan_range(who, ring_cap, rows, cols, p0, count, reach_w + cols + 1)) return 1;
  if (count == 0) return 0;

  const NlPlan pl = nl_plan(rows, cols, count, hr, hc, h, w);
  const int pb = pl.pb;
  const long long e0 = p0 > reach_w ? p0 - reach_w : 0, e1 = nl_min(n, p0 + count + reach_w);
  // e1 - e0 <= centres: what ebsdvae_nlpar_work sized the scratch for
  float* dpart = (float*)work;
  float* s = dpart + (size_t)pl.centres * pl.noff * pb;
  hipStream_t st = (hipStream_t)stream;
  const int hrd = hr > 1 ? hr : 1, hcd = hc > 1 ? hc : 1;

  if (!fixed_sigma || hr + hc > 0) {   // a fixed sigma under a 1 x 1 window needs no distance
    ScanWalk g;
    dim3 grid;   // its y is pb
    if (evh::plan_scan_walk(who, src, ring_cap, rows, cols, e0, e1, h, w, kNlRun, &g, &grid))
      return 1;
    evh::with_const<1, 2>(hrd, [&](auto HRc) {
      evh::with_const<1, 2>(hcd, [&](auto HCc) {
        hipLaunchKernelGGL((nlpar_distance_kernel<decltype(HRc)::value, decltype(HCc)::value>),
                           grid, dim3(kNlThreads), 0, st, g, dpart, pb);
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
  return evh::check_launch(who);
}

extern "C" int ebsdvae_nlpar_average(const float* src, long long ring_cap, int rows, int cols,
                                     long long p0, long long count, const float* weights, int hr,
                                     int hc, int h, int w, float* dst, ebsdvae_stream_t stream) {
  return evh::run_scan_average(
      "nlpar_average", true, kNlRun, src, src && weights && dst, ring_cap, rows, cols, p0, count,
      hr, hc, h, w, [&](auto HR, auto HC, dim3 grid, const ScanWalk& g) {
        hipLaunchKernelGGL((nlpar_average_kernel<decltype(HR)::value, decltype(HC)::value>), grid,
                           dim3(kNlThreads), 0, (hipStream_t)stream, g, weights, dst);
      });
}
