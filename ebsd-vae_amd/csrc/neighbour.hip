// Neighbour pattern averaging ("Neighbour pattern averaging", has the
// definition): pattern p at (i, j) = (p / cols, p % cols) of the scan grid becomes
//   A[p] = sum W[a + hr][b + hc] * T[(i + a) cols + (j + b)]  /  sum W[a + hr][b + hc]
// over the window's offsets with W != 0 and (i + a, j + b) on the grid: float32 fma chains from
// 0, a ascending then b ascending, and one true division (walk_and_average, scan_window.h).
#include "scan_window.h"
#include "../../include/ebsdvae.h"

namespace ev {

// The pointers lead the arguments: the weights' base arrives with the first kernel-argument
// load, so their scalar loads issue back to back
template <int HR, int HC>
__global__ __launch_bounds__(kSwThreads) void neighbour_kernel(const float* weights, float* out,
                                                               const ScanWalk g) {
  constexpr int NA = 2 * HR + 1, NB = 2 * HC + 1;
  const int f = blockIdx.y * kSwThreads + threadIdx.x;   // this thread's float4 of pixels
  const ScanRun r = scan_run(g);
  if (r.lo >= r.hi || f >= g.hw4) return;

  float wt[NA][NB];    // the weights, 0 in a neighbour row that is off the grid
  bool row_used[NA];   // the row has a nonzero weight: an all-zero row is not loaded
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int row = r.i + a - HR;
    const bool on_grid = row >= 0 && row < g.rows;
    row_used[a] = false;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      wt[a][b] = on_grid ? weights[a * NB + b] : 0.f;
      row_used[a] = row_used[a] || wt[a][b] != 0.f;
    }
  }

  walk_and_average<HR, HC>(
      g, r, f, out, [&](int a, bool) EV_LAMBDA_INLINE { return row_used[a]; },
      [&](int j, int a, int b) EV_LAMBDA_INLINE {   // off-grid columns are masked per tap
        const int c = j + b - HC;
        return c >= 0 && c < g.cols ? wt[a][b] : 0.f;
      },
      []() EV_LAMBDA_INLINE {});
}

}  // namespace ev

using namespace ev;

extern "C" int ebsdvae_average_neighbours(const float* src, long long ring_cap, int rows, int cols,
                                          long long p0, long long count, const float* weights,
                                          int hr, int hc, int h, int w, float* dst,
                                          ebsdvae_stream_t stream) {
  // outputs a thread walks along a scan row: 16 measured best, 1 is the plain tap loop
  static const int run_pref = evh::env_int("EBSDVAE_NEIGHBOUR_RUN", 16, 1, 64);
  return evh::run_scan_average(
      "average_neighbours", false, run_pref, src, src && weights && dst, ring_cap, rows, cols, p0,
      count, hr, hc, h, w, [&](auto HR, auto HC, dim3 grid, const ScanWalk& g) {
        hipLaunchKernelGGL((neighbour_kernel<decltype(HR)::value, decltype(HC)::value>), grid,
                           dim3(kSwThreads), 0, (hipStream_t)stream, weights, dst, g);
      });
}
