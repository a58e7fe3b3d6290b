// Neighbour pattern averaging ("Neighbour pattern averaging"): every
// transformed pattern of a scan becomes the weighted mean of itself and its neighbours on the
// scan grid, before the encoder sees it.  Pattern p sits at (i, j) = (p / cols, p % cols):
//
//   A[p] = sum W[a + hr][b + hc] * T[(i + a) cols + (j + b)]  /  sum W[a + hr][b + hc]
//
// over the offsets -hr <= a <= hr, -hc <= b <= hc with W != 0 and (i + a, j + b) on the grid
// (neighbours off the grid are dropped, the remaining weights renormalise).  Both sums are
// float32 fma chains from 0, a ascending then b ascending, followed by one true division: a
// pattern's output is a function of T, W and the grid alone.
//
// HBM-bound: 4 h w bytes read and written per pattern at the floor.  A thread owns a float4 of
// pixels and walks a run of consecutive outputs along one scan row.  It keeps the window's
// (2 hc + 1) columns of (2 hr + 1) neighbour values in registers, so moving one output to the
// right costs 2 hr + 1 loads, not (2 hr + 1)(2 hc + 1); the window rotates through a register
// array whose indices are compile-time constants (the run is unrolled by the window's width), so
// nothing is moved.  Every output still runs the whole chain over its window: the sliding shares
// loads, never partial sums.  The re-reads across scan rows are left to the L2 and the Infinity
// Cache.  A run of 1 is the plain tap loop (every neighbour loaded per output).
//
// The ring slot (q % ring_cap), the on-grid tests and the weights are per pattern: the same in
// every lane.  A tap that the definition drops (off the grid, or weight 0) enters its chain with
// weight 0 and, off the grid, the value 0: for the finite T of the contract fma(0, t, s) == s
// bit for bit, so the chain is the definition's.  Nothing off the grid is ever addressed.
#include "common.h"
#include "../../include/ebsdvae.h"

namespace ev {

constexpr int kNbThreads = 256;
constexpr int kNbMaxHalf = 2;   // windows up to 5 x 5

struct NbArgs {
  const float* src;       // ring of `cap` patterns, pattern q in slot q % cap
  const float* weights;   // (2 hr + 1) x (2 hc + 1)
  float* dst;             // count patterns
  long long p0, count;
  int cap, rows, cols, hw4, run, chunks, row0;
};

template <int HR, int HC>
__global__ __launch_bounds__(kNbThreads) void neighbour_kernel(const NbArgs g) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1;
  const int f = blockIdx.y * kNbThreads + threadIdx.x;   // this thread's float4 of pixels
  // the run: scan row i, columns [lo, hi) of the column chunk, clipped to [p0, p0 + count)
  const int i = g.row0 + (int)(blockIdx.x / (unsigned)g.chunks);
  const int c0 = (int)(blockIdx.x % (unsigned)g.chunks) * g.run;
  const long long rowbase = (long long)i * g.cols;
  const long long first = g.p0 - rowbase, last = g.p0 + g.count - rowbase;
  const int lo = first > c0 ? (int)first : c0;
  const int end = c0 + g.run < g.cols ? c0 + g.run : g.cols;
  const int hi = last < end ? (int)last : end;
  if (lo >= hi || f >= g.hw4) return;

  float wt[NA][NB];    // the weights, 0 in a neighbour row that is off the grid
  bool row_ok[NA];     // the neighbour row is on the grid and has a nonzero weight
  int slot[NA];        // ring slot of the next column this row loads
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int r = i + a - HR;
    const bool on_grid = r >= 0 && r < g.rows;
    row_ok[a] = false;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      wt[a][b] = on_grid ? g.weights[a * NB + b] : 0.f;
      row_ok[a] = row_ok[a] || wt[a][b] != 0.f;
    }
    long long q = ((long long)r * g.cols + (lo - HC)) % g.cap;   // q may be negative
    slot[a] = (int)(q < 0 ? q + g.cap : q);
  }

  const size_t hw = (size_t)g.hw4 * 4;
  const float* src = g.src + (size_t)f * 4;
  float* dst = g.dst + ((size_t)(rowbase + lo - g.p0) * g.hw4 + f) * 4;
  float4 win[NB][NA];   // win[k]: the column whose offset from lo - HC is k modulo NB

  // load grid column c into win[k]; what is not on the grid is not read and counts as 0
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
      const int j = lo + t0 + u;
      load_column((u + NB - 1) % NB, j + HC);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      float ws = 0.f;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          // a dropped tap enters with weight 0: fma(0, finite, s) == s, bit for bit
          const int c = j + b - HC;
          const float wv = c >= 0 && c < g.cols ? wt[a][b] : 0.f;
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
    }
  }
}

}  // namespace ev

using namespace ev;

extern "C" int ebsdvae_average_neighbours(const float* src, long long ring_cap, int rows, int cols,
                                          long long p0, long long count, const float* weights,
                                          int hr, int hc, int h, int w, float* dst,
                                          ebsdvae_stream_t stream) {
  EV_REQUIRE(hr >= 0 && hr <= kNbMaxHalf && hc >= 0 && hc <= kNbMaxHalf,
             "average_neighbours: half widths hr=%d hc=%d outside 0..%d", hr, hc, kNbMaxHalf);
  EV_REQUIRE(src && weights && dst, "average_neighbours: null pointer");
  EV_REQUIRE(rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31),
             "average_neighbours: grid %d x %d", rows, cols);
  EV_REQUIRE(h > 0 && w > 0 && (long long)h * w < (1LL << 31) && ((long long)h * w) % 4 == 0,
             "average_neighbours: h*w = %lld must be a positive multiple of 4", (long long)h * w);
  const long long n = (long long)rows * cols;
  EV_REQUIRE(count >= 0 && p0 >= 0 && p0 <= n && count <= n - p0,
             "average_neighbours: range [%lld, %lld + %lld) leaves the %d x %d grid", p0, p0, count,
             rows, cols);
  const long long reach = (long long)hr * cols + hc, need = count + 2 * reach;
  EV_REQUIRE(ring_cap >= (need < n ? need : n) && ring_cap < (1LL << 31),
             "average_neighbours: ring of %lld patterns, %lld outputs of this window need %lld",
             ring_cap, count, need < n ? need : n);
  if (count == 0) return 0;

  // outputs a thread walks along a scan row.  16 measured best at 128 x 128 patterns on a
  // 128-column scan (1, the plain tap loop, is 1.6x - 2.5x slower; at 32
  // the grid gets coarse); the switch is there for that A/B
  static const int run_pref = evh::env_int("EBSDVAE_NEIGHBOUR_RUN", 16, 1, 64);
  NbArgs g;
  g.src = src, g.weights = weights, g.dst = dst;
  g.p0 = p0, g.count = count;
  g.cap = (int)ring_cap, g.rows = rows, g.cols = cols;
  g.hw4 = (int)((long long)h * w / 4);
  g.run = run_pref < cols ? run_pref : cols;
  g.chunks = (cols + g.run - 1) / g.run;
  g.row0 = (int)(p0 / cols);
  const long long nrows = (p0 + count - 1) / cols - g.row0 + 1;
  const long long runs = nrows * g.chunks;
  const int pxblocks = (g.hw4 + kNbThreads - 1) / kNbThreads;
  EV_REQUIRE(runs < (1LL << 31) && pxblocks <= 65535, "average_neighbours: launch too large");
  const dim3 grid((unsigned)runs, (unsigned)pxblocks);
  evh::with_const<0, 1, 2>(hr, [&](auto HRc) {
    evh::with_const<0, 1, 2>(hc, [&](auto HCc) {
      hipLaunchKernelGGL((neighbour_kernel<decltype(HRc)::value, decltype(HCc)::value>), grid,
                         dim3(kNbThreads), 0, (hipStream_t)stream, g);
    });
  });
  return evh::check_launch("average_neighbours");
}
