// The sliding-window walk over the scan grid ("The scan-window walker")
// that the kernels of csrc/neighbour.hip and csrc/nlpar.hip give a body each.  Block (x, y) takes
// run x (a scan row and a chunk of `run` columns, clipped to the launch's range) and pixel block
// y; a thread owns a float4.  What is off the grid is never addressed and counts as 0.
#pragma once
#include "common.h"

namespace ev {

constexpr int kSwThreads = 256;   // float4s of a pixel block
constexpr int kSwMaxHalf = 2;     // windows up to 5 x 5

struct ScanWalk {
  const float* src;        // ring of `cap` patterns, pattern q in slot q % cap
  long long first, last;   // the flat range of the launch's outputs (or centres)
  int cap, rows, cols, hw4, run, chunks, row0;
};

// a block's run: scan row i (first pattern: rowbase), columns [lo, hi); empty when lo >= hi
struct ScanRun { int i, lo, hi; long long rowbase; };
EV_DEVINL ScanRun scan_run(const ScanWalk& g) {
  ScanRun r;
  r.i = g.row0 + (int)(blockIdx.x / (unsigned)g.chunks);
  const int c0 = (int)(blockIdx.x % (unsigned)g.chunks) * g.run;
  r.rowbase = (long long)r.i * g.cols;
  const long long first = g.first - r.rowbase, last = g.last - r.rowbase;
  r.lo = first > c0 ? (int)first : c0;
  const int end = c0 + g.run < g.cols ? c0 + g.run : g.cols;
  r.hi = last < end ? (int)last : end;
  return r;
}

// Walks the run r.  For every output column j, left to right, `body(j, u, win)` finds grid
// column j + b - HC of neighbour row i + a - HR in win[(u + b) % NB][a]; u is a compile-time
// constant once the loop is unrolled.  With px_ok false thread f reads nothing and its window
// holds zeros.  `row_loaded(a, on_grid)`: neighbour row a is read (never off the grid), else it
// counts as 0.  g and r by value: the registers are then those of the walk written out.
template <int HR, int HC, class RowLoaded, class Body>
EV_DEVINL void walk_scan_window(const ScanWalk g, const ScanRun r, int f, bool px_ok,
                                RowLoaded&& row_loaded, Body&& body) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1;
  bool row_ok[NA];     // the neighbour row is loaded
  int slot[NA];        // ring slot of the next column this row loads
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int row = r.i + a - HR;
    row_ok[a] = row_loaded(a, row >= 0 && row < g.rows);
    long long q = ((long long)row * g.cols + (r.lo - HC)) % g.cap;   // q may be negative
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
  for (int k = 0; k < NB - 1; ++k) load_column(k, r.lo - HC + k);

  const int n = r.hi - r.lo;
  for (int t0 = 0; t0 < n; t0 += NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (t0 + u >= n) break;
      const int j = r.lo + t0 + u;
      load_column((u + NB - 1) % NB, j + HC);
      body(j, u, win);
    }
  }
}

// The two averaging kernels' walk: every output is its window's mean under weight(j, a, b), 0 for
// a tap the definition drops (fma(0, finite, s) == s, bit for bit), stored to `out`.  The fma
// chains run a ascending then b ascending, one division ends them; step() follows each output.
template <int HR, int HC, class RowLoaded, class Weight, class Step>
EV_DEVINL void walk_and_average(const ScanWalk g, const ScanRun r, int f, float* out,
                                RowLoaded&& row_loaded, Weight&& weight, Step&& step) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1;
  const size_t hw = (size_t)g.hw4 * 4;
  float* dst = out + ((size_t)(r.rowbase + r.lo - g.first) * g.hw4 + f) * 4;
  walk_scan_window<HR, HC>(g, r, f, true, row_loaded,
                           [&](int j, int u, const float4(&win)[NB][NA]) EV_LAMBDA_INLINE {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float ws = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float wv = weight(j, a, b);
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
    step();
  });
}

}  // namespace ev

// ---------------------------------------------------------------- the host side
namespace evh {

// what every scan-stage entry checks alike, `who` naming it.  `pointers`: none is null.  The
// NLPAR entries (`nlpar`) bound h w by 2^24, not 2^31, and test their pointers last, not second
inline int check_scan_shape(const char* who, bool pointers, int rows, int cols, int hr, int hc,
                            int h, int w, bool nlpar) {
  EV_REQUIRE(hr >= 0 && hr <= ev::kSwMaxHalf && hc >= 0 && hc <= ev::kSwMaxHalf,
             "%s: half widths hr=%d hc=%d outside 0..%d", who, hr, hc, ev::kSwMaxHalf);
  EV_REQUIRE(nlpar || pointers, "%s: null pointer", who);
  EV_REQUIRE(rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31), "%s: grid %d x %d", who,
             rows, cols);
  const long long hw = (long long)h * w;
  EV_REQUIRE(h > 0 && w > 0 && hw < (1LL << (nlpar ? 24 : 31)) && hw % 4 == 0,
             "%s: h*w = %lld must be a positive multiple of 4%s", who, hw,
             nlpar ? " below 2^24" : "");
  EV_REQUIRE(pointers, "%s: null pointer", who);
  return 0;
}

// the outputs [p0, p0 + count) lie on the grid; the ring holds all within `reach` of them
inline int check_scan_range(const char* who, long long ring_cap, int rows, int cols, long long p0,
                            long long count, long long reach) {
  const long long n = (long long)rows * cols;
  EV_REQUIRE(count >= 0 && p0 >= 0 && p0 <= n && count <= n - p0,
             "%s: range [%lld, %lld + %lld) leaves the %d x %d grid", who, p0, p0, count, rows, cols);
  const long long need = count + 2 * reach < n ? count + 2 * reach : n;
  EV_REQUIRE(ring_cap >= need && ring_cap < (1LL << 31),
             "%s: ring of %lld patterns, %lld outputs of this window need %lld", who, ring_cap,
             count, need);
  return 0;
}

// the walk over the non-empty flat range [first, last) and its grid (runs, pixel blocks)
inline int plan_scan_walk(const char* who, const float* ring, long long ring_cap, int rows, int cols,
                          long long first, long long last, int h, int w, int run_pref,
                          ev::ScanWalk* g, dim3* grid) {
  g->src = ring, g->first = first, g->last = last;
  g->cap = (int)ring_cap, g->rows = rows, g->cols = cols;
  g->hw4 = (int)((long long)h * w / 4);
  g->run = run_pref < cols ? run_pref : cols;
  g->chunks = (cols + g->run - 1) / g->run;
  g->row0 = (int)(first / cols);
  const long long runs = ((last - 1) / cols - g->row0 + 1) * g->chunks;
  const int pxblocks = (g->hw4 + ev::kSwThreads - 1) / ev::kSwThreads;
  EV_REQUIRE(runs < (1LL << 31) && pxblocks <= 65535, "%s: launch too large", who);
  *grid = dim3((unsigned)runs, (unsigned)pxblocks);
  return 0;
}

// The two averaging entries: checks, plan and launch(HR, HC, grid, walk), the half widths as
// integral constants
template <class Launch>
inline int run_scan_average(const char* who, bool nlpar, int run_pref, const float* src,
                            bool pointers, long long ring_cap, int rows, int cols, long long p0,
                            long long count, int hr, int hc, int h, int w, Launch&& launch) {
  if (check_scan_shape(who, pointers, rows, cols, hr, hc, h, w, nlpar)) return 1;
  if (check_scan_range(who, ring_cap, rows, cols, p0, count, (long long)hr * cols + hc)) return 1;
  if (count == 0) return 0;
  ev::ScanWalk g;
  dim3 grid;
  if (plan_scan_walk(who, src, ring_cap, rows, cols, p0, p0 + count, h, w, run_pref, &g, &grid))
    return 1;
  with_const<0, 1, 2>(hr, [&](auto HR) {
    with_const<0, 1, 2>(hc, [&](auto HC) { launch(HR, HC, grid, g); });
  });
  return check_launch(who);
}

}  // namespace evh
