// Dictionary simulation ("Dictionary simulation"): dictionary patterns
// projected from a master pattern on the device, one gather-and-interpolate launch per batch in
// front of the encoder.  Per pattern b and detector pixel p (row-major, h * w of them), with
// n = (M - 1) / 2 and every float32 step written out so that it rounds once (no contraction):
//
//   (a) g = float32(Bunge passive matrix of euler[b]), entries formed in float64 from the
//       float64 sines and cosines of the angles times pi / 180
//   (b) v_i = fma(g_i2, d_z, fma(g_i1, d_y, g_i0 * d_x)),  d = dirs[:, p]
//   (c) lower hemisphere iff v_z < 0;  s = sqrt(fma(x, x, y * y) / (1 + |z|));
//       x == 0 && y == 0: tx = ty = 0
//       |y| <= |x|:       tx = copysign(s, x),  ty = tx * (k * atan(y / x)),  k = float32(4 / pi)
//       otherwise:        ty = copysign(s, y),  tx = ty * (k * atan(x / y))
//   (d) u = min(max(fma(n, tx, n), 0), 2n), j0 = min(int(u), 2n - 1), fu = u - j0; the row r
//       likewise from ty;  top = fma(fu, m[r0][j0 + 1] - m[r0][j0], m[r0][j0]), bot the same on
//       row r0 + 1, value = fma(fr, bot - top, top)
//   (e) rescale: hi == lo ? 0 : (v - lo) / (hi - lo) over the pattern
//
// One block of 1024 threads per pattern.  The pixels are taken flat, four adjacent ones per
// thread and step where h * w is a multiple of 4 (then every load of a direction plane and every
// store is a whole aligned 16-byte line, whatever w is), one otherwise.  Consecutive lanes take
// consecutive groups, so a wave's gathers fall on neighbouring texels of a few master rows.  Up
// to 128 x 128 pixels a thread keeps its 16 values in registers between the min / max and the
// store; larger patterns write the interpolated values to dst, and every thread rescales its
// own stores in place after the block's min / max (no scratch, still one launch).  All four
// forms run the same device function per pixel, so they give the same bits.
//
// The directions (196 KB at 128 x 128) are shared by every block and stay in L2.  One pattern
// reads a compact patch of one or both hemispheres; over a batch of unrelated orientations the
// patches cover the whole master, so a master pair larger than an XCD's 4 MiB of L2 is served
// in part from the Infinity Cache.
#include <math.h>

#include "common.h"
#include "../../include/ebsdvae.h"

namespace ev {
namespace sim {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSide = 256;
constexpr int kRegPx = 128 * 128;          // values kept in registers up to here
constexpr int kRegPerThread = kRegPx / kThreads;
constexpr int kMinM = 3, kMaxM = 4097;

struct Args {
  const float* up;
  const float* lo;
  const float* dirs;     // (3, n)
  const double* euler;   // (B, 3)
  float* dst;            // (B, n)
  int M, n, rescale;
};

// (a): thread 0..2 take one angle each, threads 0..8 one entry each
EV_DEVINL void orientation_matrix(const double* __restrict__ e, double* sc, float* g) {
  const int t = threadIdx.x;
  if (t < 3) {
    const double a = e[t] * (M_PI / 180.0);
    sc[2 * t] = cos(a), sc[2 * t + 1] = sin(a);
  }
  __syncthreads();
  if (t < 9) {
    const double c1 = sc[0], s1 = sc[1], c = sc[2], s = sc[3], c2 = sc[4], s2 = sc[5];
    double v;
    switch (t) {
      case 0: v = c1 * c2 - s1 * s2 * c; break;
      case 1: v = s1 * c2 + c1 * s2 * c; break;
      case 2: v = s2 * s; break;
      case 3: v = -c1 * s2 - s1 * c2 * c; break;
      case 4: v = -s1 * s2 + c1 * c2 * c; break;
      case 5: v = c2 * s; break;
      case 6: v = s1 * s; break;
      case 7: v = -c1 * s; break;
      default: v = c; break;
    }
    g[t] = (float)v;
  }
  __syncthreads();
}

// (d) along one axis: texel index and fraction of the Lambert coordinate t
EV_DEVINL void texel(float t, float nf, int n2, int& i0, float& f) {
  const float u = fminf(fmaxf(fmaf(nf, t, nf), 0.f), (float)n2);
  i0 = min((int)u, n2 - 1);
  f = u - (float)i0;
}

// (b) - (d) at one pixel
EV_DEVINL float sample(const Args& a, const float (&g)[9], float dx, float dy, float dz) {
#pragma clang fp contract(off)
  const float x = fmaf(g[2], dz, fmaf(g[1], dy, g[0] * dx));
  const float y = fmaf(g[5], dz, fmaf(g[4], dy, g[3] * dx));
  const float z = fmaf(g[8], dz, fmaf(g[7], dy, g[6] * dx));
  const float* __restrict__ m = z < 0.f ? a.lo : a.up;
  const float s = sqrtf(fmaf(x, x, y * y) / (1.f + fabsf(z)));
  constexpr float k = 1.27323954473516268615f;   // 4 / pi
  float tx = 0.f, ty = 0.f;
  if (x != 0.f || y != 0.f) {
    if (fabsf(y) <= fabsf(x)) {
      tx = copysignf(s, x);
      ty = tx * (k * atanf(y / x));
    } else {
      ty = copysignf(s, y);
      tx = ty * (k * atanf(x / y));
    }
  }
  const int n2 = a.M - 1;
  const float nf = (float)(n2 >> 1);
  int j0, r0;
  float fu, fr;
  texel(tx, nf, n2, j0, fu);
  texel(ty, nf, n2, r0, fr);
  const float* p = m + r0 * a.M + j0;
  const float m00 = p[0], m01 = p[1], m10 = p[a.M], m11 = p[a.M + 1];
  const float top = fmaf(fu, m01 - m00, m00);
  const float bot = fmaf(fu, m11 - m10, m10);
  return fmaf(fr, bot - top, top);
}

EV_DEVINL float rescale_px(float v, float lo, float hi) {
#pragma clang fp contract(off)
  return hi == lo ? 0.f : (v - lo) / (hi - lo);
}

// block-wide min / max, the same value in every thread (the waves' results in wave order)
EV_DEVINL void block_minmax(float& lo, float& hi, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[2 * wave] = lo, red[2 * wave + 1] = hi;
  __syncthreads();
  lo = red[0], hi = red[1];
  for (int w = 1; w < kWaves; ++w) lo = fminf(lo, red[2 * w]), hi = fmaxf(hi, red[2 * w + 1]);
}

// kVec pixels (1 or 4) of item `it` of the pattern into v[0 .. kVec)
template <int kVec>
EV_DEVINL void sample_item(const Args& a, const float (&g)[9], int it, float* v) {
  const float* dx = a.dirs + (size_t)it * kVec;
  const float* dy = dx + a.n;
  const float* dz = dy + a.n;
  if constexpr (kVec == 4) {
    const float4 X = ld4(dx), Y = ld4(dy), Z = ld4(dz);
    v[0] = sample(a, g, X.x, Y.x, Z.x);
    v[1] = sample(a, g, X.y, Y.y, Z.y);
    v[2] = sample(a, g, X.z, Y.z, Z.z);
    v[3] = sample(a, g, X.w, Y.w, Z.w);
  } else {
    v[0] = sample(a, g, dx[0], dy[0], dz[0]);
  }
}

template <int kVec>
EV_DEVINL void store_item(float* out, int it, const float* v) {
  if constexpr (kVec == 4) st4(out + (size_t)it * 4, make_float4(v[0], v[1], v[2], v[3]));
  else out[it] = v[0];
}

// kVec: pixels per item (4 needs n % 4 == 0 and 16-byte aligned dirs and dst); kReg: the
// pattern's values fit the registers of one block (n <= kRegPx)
template <int kVec, bool kReg>
__global__ __launch_bounds__(kThreads) void simulate_kernel(Args a) {
  __shared__ double sc[6];
  __shared__ float gs[9];
  __shared__ float red[2 * kWaves];
  orientation_matrix(a.euler + (size_t)blockIdx.x * 3, sc, gs);
  float g[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) g[i] = gs[i];
  const int items = a.n / kVec;
  float* out = a.dst + (size_t)blockIdx.x * a.n;
  float lo = INFINITY, hi = -INFINITY;
  if constexpr (kReg) {
    constexpr int kItems = kRegPerThread / kVec;
    float v[kRegPerThread];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int it = threadIdx.x + k * kThreads;
      if (it < items) {
        sample_item<kVec>(a, g, it, v + k * kVec);
#pragma unroll
        for (int e = 0; e < kVec; ++e) lo = fminf(lo, v[k * kVec + e]), hi = fmaxf(hi, v[k * kVec + e]);
      }
    }
    if (a.rescale) block_minmax(lo, hi, red);
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int it = threadIdx.x + k * kThreads;
      if (it < items) {
        if (a.rescale) {
#pragma unroll
          for (int e = 0; e < kVec; ++e) v[k * kVec + e] = rescale_px(v[k * kVec + e], lo, hi);
        }
        store_item<kVec>(out, it, v + k * kVec);
      }
    }
  } else {
    float v[kVec];
    for (int it = threadIdx.x; it < items; it += kThreads) {
      sample_item<kVec>(a, g, it, v);
#pragma unroll
      for (int e = 0; e < kVec; ++e) lo = fminf(lo, v[e]), hi = fmaxf(hi, v[e]);
      store_item<kVec>(out, it, v);
    }
    if (!a.rescale) return;
    block_minmax(lo, hi, red);
    // every thread rescales the items it stored itself: program order, no fence needed
    for (int it = threadIdx.x; it < items; it += kThreads) {
      if constexpr (kVec == 4) {
        const float4 r = ld4(out + (size_t)it * 4);
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
      } else {
        v[0] = out[it];
      }
#pragma unroll
      for (int e = 0; e < kVec; ++e) v[e] = rescale_px(v[e], lo, hi);
      store_item<kVec>(out, it, v);
    }
  }
}

}  // namespace sim
}  // namespace ev

using namespace ev;

extern "C" int ebsdvae_simulate_patterns(const float* master_upper, const float* master_lower,
                                         int M, const float* dirs, const double* euler, int B,
                                         int h, int w, int rescale, float* dst,
                                         ebsdvae_stream_t stream) {
  EV_REQUIRE(master_upper && master_lower && dirs && euler && dst,
             "simulate_patterns: null pointer");
  EV_REQUIRE(M >= sim::kMinM && M <= sim::kMaxM && (M & 1),
             "simulate_patterns: master side %d (odd, %d..%d)", M, sim::kMinM, sim::kMaxM);
  EV_REQUIRE(h >= 1 && w >= 1 && h <= sim::kMaxSide && w <= sim::kMaxSide,
             "simulate_patterns: detector %dx%d outside 1..%d", h, w, sim::kMaxSide);
  EV_REQUIRE(B >= 0, "simulate_patterns: B = %d", B);
  EV_REQUIRE(rescale == 0 || rescale == 1, "simulate_patterns: rescale %d (0 or 1)", rescale);
  if (B == 0) return 0;
  sim::Args a;
  a.up = master_upper, a.lo = master_lower, a.dirs = dirs, a.euler = euler, a.dst = dst;
  a.M = M, a.n = h * w, a.rescale = rescale;
  const bool vec = a.n % 4 == 0 && ((uintptr_t)dirs | (uintptr_t)dst) % 16 == 0;
  const bool reg = a.n <= sim::kRegPx;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)B), block(sim::kThreads);
  if (vec && reg) hipLaunchKernelGGL((sim::simulate_kernel<4, true>), grid, block, 0, st, a);
  else if (vec) hipLaunchKernelGGL((sim::simulate_kernel<4, false>), grid, block, 0, st, a);
  else if (reg) hipLaunchKernelGGL((sim::simulate_kernel<1, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((sim::simulate_kernel<1, false>), grid, block, 0, st, a);
  return evh::check_launch("simulate_patterns");
}
