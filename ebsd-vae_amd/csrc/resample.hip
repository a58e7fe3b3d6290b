// Detector binning ("Detector resampling"): an exact area-mean resample of
// a region of interest (top, left, rh, rw) of every raw detector pattern (H0, W0) to the model's
// input size (oh, ow), oh <= rh <= 8 oh and ow <= rw <= 8 ow, the stage in front of the ingest
// and correction kernels.  Per pattern:
//
//   u[y][x] = float32(src[top + y][left + x]), non-finite -> 0
//   r[y][j] = sum_t xwts[j][t] * u[y][xstart[j] + t]          float32 fma chain from 0, t ascending
//   S[i][j] = sum_t ywts[i][t] * r[ystart[i] + t][j]          the same
//   out[i][j] = S[i][j] / denom                               one true division
//
// The host builds the tables (overlap of source and output pixels, in output-pixel units): a
// zero weight pads a row of the table, and fma(0, u, s) = s for the finite u of the load rule,
// so the chain of an output is the ascending sum over the source pixels it overlaps, whatever
// the padding.  Tap positions are clamped into the rows and columns the block has staged, which
// keeps every read inside the pattern and the planes for any table contents.
//
// One block per (pattern, band of kRsBand output rows), and inside it one pass per chunk of cw
// output columns (cw = ow unless the planes would not fit 64 KiB of LDS):
//   1. the tables of the band and the chunk go to LDS, and the source rows of the band, columns
//      of the chunk, as they are (uint8, float32
//      or float64): coalesced loads, one aligned 4-byte word per lane for uint8 -- a row starts
//      at any byte, so its words are fetched from the aligned address below it and the row's
//      offset in the word (0..3) is kept as the row's offset in LDS;
//   2. x pass: a wave's lanes take consecutive source rows of one output column (tables are
//      wave-uniform), plane X (rows x cw) in LDS;
//   3. y pass: lanes take consecutive columns of one output row, divide, store whole lines.
// Both planes have an odd row stride in banks (as correct.hip), so the lane-per-row accesses of
// step 2 are conflict-free.  Source rows shared by two bands are read by both.  No scratch, no
// atomics; HBM-bound: the ROI's bytes read once (plus the shared rows) and 4 oh ow written.
#include <math.h>

#include "common.h"
#include "pattern_src.h"
#include "../../include/ebsdvae.h"

namespace ev {

constexpr int kRsThreads = 256;
constexpr int kRsBand = 8;          // output rows per block
constexpr int kRsStage = 8;         // loads in flight per thread while staging
constexpr int kRsMaxSide = 256;     // out_h, out_w limit
constexpr int kRsMaxTaps = 9;       // ceil(8) + 1
constexpr int kRsMaxFactor = 8;
constexpr size_t kRsLdsBudget = 64 * 1024;

struct RsArgs {
  int H0, W0, top, left, rh, rw, oh, ow;
  const int* ystart;
  const float* ywts;
  int ytaps;
  const int* xstart;
  const float* xwts;
  int xtaps;
  float denom;
  int nbands, cw, cap_rows, cap_cols;
  int pitch;   // row pitch of the source plane in LDS, bytes
  int xoff;    // byte offset of plane X in LDS; the chunk's tables follow it
};

// LDS bytes of a source row of `cols` elements: an odd number of 4-byte (8-byte for float64)
// units; a uint8 row also holds the up to 3 bytes in front of it in its first word
static inline int rs_pitch(int esize, int cols) {
  if (esize == 1) return 4 * (((cols + 3 + 3) / 4) | 1);
  return esize * (cols | 1);
}

// rows (columns) of the source that `n` consecutive outputs of an axis can span, with the
// table's padding: floor((n - 1) R / O) + 1 between the first taps, and taps behind the last
static inline int rs_span(int n, int R, int O, int taps) {
  const long long s = (long long)(n - 1) * R / O + 1 + taps;
  return (int)(s < R ? s : R);
}

static inline size_t rs_lds_bytes(int esize, const RsArgs& a, int cw, int* pitch, int* xoff) {
  const int cols = rs_span(cw, a.rw, a.ow, a.xtaps);
  *pitch = rs_pitch(esize, cols);
  *xoff = ((a.cap_rows * *pitch + 15) / 16) * 16;
  return (size_t)*xoff + (size_t)a.cap_rows * (cw | 1) * 4 + (size_t)cw * 4 +
         (size_t)cw * a.xtaps * 4 + (size_t)kRsBand * 4 + (size_t)kRsBand * a.ytaps * 4;
}

// offset (0..3) of a uint8 row in its first aligned word
EV_DEVINL int rs_misalign(const void* src, size_t element) {
  return (int)(((uintptr_t)src + element) & 3);
}

// XT = a.xtaps, a compile-time constant: the x pass, where most of the work is, issues the LDS
// reads of an item together and runs its chain out of registers
// the aligned word at p of a uint8 batch [lo, hi), byte by byte; bytes outside it read as 0
EV_DEVINL uint32_t rs_word_bytewise(uintptr_t p, uintptr_t lo, uintptr_t hi) {
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (p + e >= lo && p + e < hi)
      v |= (uint32_t)(*reinterpret_cast<const unsigned char*>(p + e)) << (8 * e);
  return v;
}

// y pass of one chunk for a.ytaps <= YC: all LDS reads of an item first, then the chain over
// the first a.ytaps of them
template <int YC>
EV_DEVINL void rs_y_pass(const RsArgs& a, const float* X, const int* ys, const float* yw,
                         float* __restrict__ out, int rows, int r0, int i0, int ni, int c0, int nc) {
  const int px = nc | 1, items = ni * nc;
  int it = threadIdx.x, i = it / nc, j = it - i * nc;
  const int di = kRsThreads / nc, dj = kRsThreads - di * nc;
  for (; it < items; it += kRsThreads) {
    const float* wt = yw + i * a.ytaps;
    const int s = ys[i];
    float v[YC], w[YC];
#pragma unroll
    for (int t = 0; t < YC; ++t) {
      const int y = min(max(min(max(s + t, 0), a.rh - 1) - r0, 0), rows - 1);
      v[t] = X[y * px + j];
      w[t] = wt[min(t, a.ytaps - 1)];
    }
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < YC; ++t) acc = t < a.ytaps ? fmaf(w[t], v[t], acc) : acc;
    out[(size_t)(i0 + i) * a.ow + c0 + j] = acc / a.denom;
    i += di, j += dj;
    if (j >= nc) j -= nc, ++i;
  }
}

template <typename T, int XT>
__global__ __launch_bounds__(kRsThreads) void resample_kernel(const T* __restrict__ src,
                                                              long long total, RsArgs a,
                                                              float* __restrict__ dst) {
  extern __shared__ __align__(16) unsigned char lds[];
  T* S = reinterpret_cast<T*>(lds);
  float* X = reinterpret_cast<float*>(lds + a.xoff);
  const int b = blockIdx.x / a.nbands, band = blockIdx.x - b * a.nbands;
  const int i0 = band * kRsBand, ni = min(kRsBand, a.oh - i0);
  // the band's source rows [r0, r0 + rows) of the ROI
  const int r0 = min(max(a.ystart[i0], 0), a.rh - 1);
  const int r1 = min(max(a.ystart[i0 + ni - 1] + a.ytaps - 1, r0), a.rh - 1);
  const int rows = min(r1 - r0 + 1, a.cap_rows);
  const size_t pat0 = (size_t)b * a.H0 * a.W0;
  float* out = dst + (size_t)b * a.oh * a.ow;

  for (int c0 = 0; c0 < a.ow; c0 += a.cw) {
    const int nc = min(a.cw, a.ow - c0), px = nc | 1;
    int* xs = reinterpret_cast<int*>(X + a.cap_rows * (a.cw | 1));
    float* xw = reinterpret_cast<float*>(xs + a.cw);
    int* ys = reinterpret_cast<int*>(xw + a.cw * XT);     // the band's y tables
    float* yw = reinterpret_cast<float*>(ys + kRsBand);
    // the chunk's source columns [x0, x0 + cols) of the ROI
    const int x0 = min(max(a.xstart[c0], 0), a.rw - 1);
    const int x1 = min(max(a.xstart[c0 + nc - 1] + a.xtaps - 1, x0), a.rw - 1);
    const int cols = min(x1 - x0 + 1, a.cap_cols);
    // element index of (row r0 + y, column x0) of the ROI in the batch
    const size_t org = pat0 + (size_t)(a.top + r0) * a.W0 + a.left + x0;

    // ---- 1. tables (positions relative to x0) and the source plane
    for (int j = threadIdx.x; j < nc; j += kRsThreads) xs[j] = a.xstart[c0 + j] - x0;
    for (int k = threadIdx.x; k < nc * XT; k += kRsThreads) xw[k] = a.xwts[(size_t)c0 * XT + k];
    if (c0 == 0) {
      for (int i = threadIdx.x; i < ni; i += kRsThreads) ys[i] = a.ystart[i0 + i];
      for (int k = threadIdx.x; k < ni * a.ytaps; k += kRsThreads)
        yw[k] = a.ywts[(size_t)i0 * a.ytaps + k];
    }
    // kRsStage independent loads per thread are in flight before the first is stored
    if constexpr (sizeof(T) == 1) {
      const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)total;
      const uintptr_t lo4 = (lo + 3) & ~(uintptr_t)3, hi4 = hi & ~(uintptr_t)3;
      const int pw = a.pitch >> 2, wmax = (cols + 6) >> 2, nw = rows * wmax;
      uint32_t* Sw = reinterpret_cast<uint32_t*>(lds);
      if (lo4 + 4 <= hi4) {
        for (int base = threadIdx.x; base < nw; base += kRsThreads * kRsStage) {
          uint32_t v[kRsStage];
          uintptr_t p[kRsStage];
          int slot[kRsStage];
#pragma unroll
          for (int u = 0; u < kRsStage; ++u) {
            const int idx = min(base + u * kRsThreads, nw - 1);
            const int y = idx / wmax, k = idx - y * wmax;
            const uintptr_t row = lo + org + (size_t)y * a.W0;
            const int mis = (int)(row & 3);
            p[u] = row - mis + 4 * (uintptr_t)k;
            slot[u] = (base + u * kRsThreads < nw && k < ((mis + cols + 3) >> 2)) ? y * pw + k : -1;
            // an aligned word inside the batch: this one, but for the first and the last of the
            // batch where they lie across its ends
            const uintptr_t q = min(max(p[u], lo4), hi4 - 4);
            v[u] = *reinterpret_cast<const uint32_t*>(q);
          }
#pragma unroll
          for (int u = 0; u < kRsStage; ++u) {
            if (slot[u] < 0) continue;
            if (p[u] < lo4 || p[u] + 4 > hi4) v[u] = rs_word_bytewise(p[u], lo, hi);
            Sw[slot[u]] = v[u];
          }
        }
      } else {   // a batch of less than two words
        for (int idx = threadIdx.x; idx < nw; idx += kRsThreads) {
          const int y = idx / wmax, k = idx - y * wmax;
          const uintptr_t row = lo + org + (size_t)y * a.W0;
          const int mis = (int)(row & 3);
          if (k < ((mis + cols + 3) >> 2))
            Sw[y * pw + k] = rs_word_bytewise(row - mis + 4 * (uintptr_t)k, lo, hi);
        }
      }
    } else {
      const int pe = a.pitch / (int)sizeof(T), n = rows * cols;
      const T* from = src + org;
      for (int base = threadIdx.x; base < n; base += kRsThreads * kRsStage) {
        T v[kRsStage];
        int slot[kRsStage];
#pragma unroll
        for (int u = 0; u < kRsStage; ++u) {
          const int idx = min(base + u * kRsThreads, n - 1);
          const int y = idx / cols, x = idx - y * cols;
          slot[u] = base + u * kRsThreads < n ? y * pe + x : -1;
          v[u] = from[(size_t)y * a.W0 + x];
        }
#pragma unroll
        for (int u = 0; u < kRsStage; ++u)
          if (slot[u] >= 0) S[slot[u]] = v[u];
      }
    }
    __syncthreads();

    // ---- 2. x pass: item = (source row y, output column j), lanes along y
    {
      const int items = rows * nc;
      int it = threadIdx.x, j = it / rows, y = it - j * rows;
      const int dj = kRsThreads / rows, dy = kRsThreads - dj * rows;
      for (; it < items; it += kRsThreads) {
        const float* wt = xw + j * XT;
        const int s = min(max(xs[j], 0), cols - 1);
        float u[XT];
        if constexpr (sizeof(T) == 1) {
          // the XT bytes from column s on, as aligned words shifted into place; bytes past the
          // row's end belong to zero weights (any uint8 is finite), the word index stays in the row
          constexpr int NA = (XT + 3) / 4;
          const int pw = a.pitch >> 2;
          const uint32_t* wl = reinterpret_cast<const uint32_t*>(lds) + y * pw;
          const int p = rs_misalign(src, org + (size_t)y * a.W0) + s, k = p >> 2;
          uint32_t w[NA + 1];
#pragma unroll
          for (int i = 0; i <= NA; ++i) w[i] = wl[min(k + i, pw - 1)];
#pragma unroll
          for (int i = 0; i < NA; ++i) w[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], p & 3);
#pragma unroll
          for (int t = 0; t < XT; ++t) u[t] = (float)((w[t >> 2] >> (8 * (t & 3))) & 0xffu);
        } else {
          const T* line = reinterpret_cast<const T*>(lds + (size_t)y * a.pitch);
#pragma unroll
          for (int t = 0; t < XT; ++t) u[t] = finite_or_zero((float)line[min(s + t, cols - 1)]);
        }
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < XT; ++t) acc = fmaf(wt[t], u[t], acc);
        X[y * px + j] = acc;
        j += dj, y += dy;
        if (y >= rows) y -= rows, ++j;
      }
    }
    __syncthreads();

    // ---- 3. y pass: item = (output row i, output column j), lanes along j
    if (a.ytaps <= 3) rs_y_pass<3>(a, X, ys, yw, out, rows, r0, i0, ni, c0, nc);
    else if (a.ytaps <= 5) rs_y_pass<5>(a, X, ys, yw, out, rows, r0, i0, ni, c0, nc);
    else rs_y_pass<kRsMaxTaps>(a, X, ys, yw, out, rows, r0, i0, ni, c0, nc);
    // the next chunk's loads touch only the source plane and the tables, which no thread
    // reads after the barrier above; its own barrier orders them against this y pass's X
  }
}

template <typename T>
static void launch_resample(const T* src, int B, RsArgs a, float* dst, hipStream_t st) {
  // the widest chunk of output columns whose planes fit the budget; one column always does
  int cw = a.ow;
  size_t lds;
  while ((lds = rs_lds_bytes((int)sizeof(T), a, cw, &a.pitch, &a.xoff)) > kRsLdsBudget && cw > 1)
    cw = (cw + 1) / 2;
  a.cw = cw;
  a.cap_cols = rs_span(cw, a.rw, a.ow, a.xtaps);
  const long long total = (long long)B * a.H0 * a.W0;
  evh::with_const<1, 2, 3, 4, 5, 6, 7, 8, 9>(a.xtaps, [&](auto xt) {
    hipLaunchKernelGGL((resample_kernel<T, decltype(xt)::value>), dim3((unsigned)B * a.nbands),
                       dim3(kRsThreads), lds, st, src, total, a, dst);
  });
}

}  // namespace ev

using namespace ev;

extern "C" int ebsdvae_resample_patterns(const void* src, int src_dtype, int B, int H0, int W0,
                                         int top, int left, int rh, int rw, int out_h, int out_w,
                                         const int* ystart, const float* ywts, int ytaps,
                                         const int* xstart, const float* xwts, int xtaps,
                                         float denom, float* dst, ebsdvae_stream_t stream) {
  EV_REQUIRE(src && dst && ystart && ywts && xstart && xwts, "resample_patterns: null pointer");
  EV_REQUIRE(B >= 0 && H0 > 0 && W0 > 0, "resample_patterns: bad args (B=%d H0=%d W0=%d)", B, H0, W0);
  EV_REQUIRE(src_dtype >= 0 && src_dtype <= 2, "resample_patterns: src_dtype %d (0 f64, 1 f32, 2 u8)",
             src_dtype);
  EV_REQUIRE(out_h >= 1 && out_h <= kRsMaxSide && out_w >= 1 && out_w <= kRsMaxSide,
             "resample_patterns: output %dx%d outside 1..%d per axis", out_h, out_w, kRsMaxSide);
  EV_REQUIRE(top >= 0 && left >= 0 && rh > 0 && rw > 0 && (long long)top + rh <= H0 &&
                 (long long)left + rw <= W0,
             "resample_patterns: the region (%d, %d, %d, %d) leaves the %dx%d pattern", top, left,
             rh, rw, H0, W0);
  EV_REQUIRE(rh >= out_h && rw >= out_w,
             "resample_patterns: a %dx%d region to %dx%d would upsample (downsampling only)", rh, rw,
             out_h, out_w);
  EV_REQUIRE(rh <= kRsMaxFactor * out_h && rw <= kRsMaxFactor * out_w,
             "resample_patterns: a %dx%d region to %dx%d is a factor above %d", rh, rw, out_h, out_w,
             kRsMaxFactor);
  EV_REQUIRE(ytaps >= 1 && ytaps <= kRsMaxTaps && xtaps >= 1 && xtaps <= kRsMaxTaps,
             "resample_patterns: taps %d / %d outside 1..%d", ytaps, xtaps, kRsMaxTaps);
  EV_REQUIRE(denom > 0.f && denom <= 3.4028235e38f, "resample_patterns: denom %g is not a positive "
             "finite number", (double)denom);
  const int nbands = (out_h + kRsBand - 1) / kRsBand;
  EV_REQUIRE((long long)H0 * W0 < (1LL << 31) && (long long)B * nbands < (1LL << 31),
             "resample_patterns: pattern or batch too large");
  if (B == 0) return 0;
  RsArgs a;
  a.H0 = H0, a.W0 = W0, a.top = top, a.left = left, a.rh = rh, a.rw = rw, a.oh = out_h, a.ow = out_w;
  a.ystart = ystart, a.ywts = ywts, a.ytaps = ytaps;
  a.xstart = xstart, a.xwts = xwts, a.xtaps = xtaps;
  a.denom = denom;
  a.nbands = nbands;
  a.cap_rows = rs_span(out_h < kRsBand ? out_h : kRsBand, rh, out_h, ytaps);
  a.cw = a.cap_cols = a.pitch = a.xoff = 0;
  const hipStream_t st = (hipStream_t)stream;
  evh::with_src(src, src_dtype, [&](auto p) { launch_resample(p, B, a, dst, st); });
  return evh::check_launch("resample_patterns");
}
