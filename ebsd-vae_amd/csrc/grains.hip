// Grains of an indexed scan ("Grains"; the definitions are in
// include/ebsdvae.h): connected components of the scan grid under the cubic disorientation, ids
// in row-major order of each grain's first point, the grain mean orientation, GROD, GOS and the
// grain boundary.  Unlike the scan maps this needs scratch, LDS and atomics; all of it is integer,
// so every output is the same bits on every run.  Float arithmetic is float64 with the helpers of
// orient_math.h, contraction off.
//
// Launches, in stream order (no workgroup ever waits on another one; whatever needs a global order
// is the next launch):
//   zero      [mean / GROD / GOS] the per-root accumulators to zero
//   local     one block per kTile x kTile tile of the grid, one thread per point: the FORWARD
//             edges (p the lower flat index) that stay inside the tile are evaluated, as kam_kernel
//             does it, and the accepted ones united by a union-find in LDS; parent[p] = the flat
//             index of p's root within its tile (-1 for an unusable point).  Nothing global is
//             contended here: a scan that is one grain arrives at the next launch as one tree per
//             tile, every point one step from its tile's root.
//   hook      one thread per point: the forward edges that leave the tile are evaluated (so every
//             edge is evaluated once, in one of the two launches), and an accepted edge unites the
//             two trees: find both roots, atomicCAS the higher root under the lower, retry if it
//             stopped being a root.  The higher root always goes under the lower, here and in the
//             tile, so a component's final root is its lowest flat index whatever order the atomics
//             arrive in.
//   flatten   grain_id[p] = root of p (plain reads: the hook launch is complete)
//   accum     [mean / GROD / GOS] the member's cubic equivalent nearest the root's orientation,
//             sign towards it, in fixed point 2^-31, added to the root's four 64-bit integer
//             accumulators, and 1 to its count.  Lanes of a wave that hold consecutive points of
//             one root are summed by a segmented shuffle reduction first, runs that go on into
//             the block's next wave are joined through LDS, and only the first lane of each run of
//             the block issues atomics: integer addition is associative, so any order is exact.
//   grod      [mean / GROD / GOS] every member normalises its root's sum itself (4 loads): the
//             mean as Euler angles, its disorientation to the mean, and that in fixed point 2^-24
//             added to the root's GROD sum the same way
//   finish    [GOS / boundary] GOS = GROD sum / count; the boundary from the neighbours' roots
//   count, offsets, rank    exclusive prefix sum of "p is a root" over the scan: per-block counts
//             (kScanBlock points a block), one block scans the counts, every block ranks its points
//   relabel   grain_id[p] = rank[root], in place, last
#include "scan_grid.h"
#include "../../include/ebsdvae.h"

#include <float.h>
#include <math.h>

namespace ev {

constexpr int kGrainThreads = 256;
constexpr int kGrainWaves = kGrainThreads / 64;
constexpr int kTile = 16;   // the local launch's tile: kTile x kTile points, one block
static_assert(kTile * kTile == kGrainThreads, "one thread per point of a tile");
constexpr int kScanChunks = 16;
constexpr int kScanBlock = kGrainThreads * kScanChunks;   // points per block of the prefix sum
constexpr int kAcc = 6;   // 64-bit accumulators per root: x, y, z, w, GROD, count
constexpr double kQuatFix = 2147483648.0;   // 2^31: |component| <= 1, n < 2^31 members -> < 2^62
constexpr double kGrodFix = 16777216.0;     // 2^24: <= 63 degrees, n < 2^31 members -> < 2^61

struct GrainWork {
  long long* acc;   // (n, kAcc), used at the roots' rows
  int* parent;      // (n,)
  int* rank;        // (n,)
  int* bsum;        // (blocks of the prefix sum,)
};

EV_DEVINL bool usable_point(const double* __restrict__ euler, const int* __restrict__ valid,
                            long long p) {
  return finite3(euler[3 * p], euler[3 * p + 1], euler[3 * p + 2]) && (!valid || valid[p] != 0);
}

EV_DEVINL Q4 point_quat(const double* __restrict__ euler, long long p) {
  return from_euler_zxz(euler[3 * p], euler[3 * p + 1], euler[3 * p + 2]);
}

// min over the 24 operators S, in order, of |conj(a) (S b)| in degrees: kam_kernel's loop
EV_DEVINL double disorientation_deg(const Q4& ainv, const Q4& b) {
#pragma clang fp contract(off)
  double best = 1e300;
  for (int c = 0; c < 24; ++c) {
    const double w = qmag(qmul(ainv, qmul(cubic_op(c), b)));
    if (w < best) best = w;
  }
  return best / kDeg;
}

// Every row is zeroed, 48 bytes a point, although only the roots' rows are ever read: the roots are
// not known yet, and one contiguous write is cheaper than finding them first.
__global__ __launch_bounds__(kGrainThreads) void grain_zero_kernel(int n,
                                                                   long long* __restrict__ acc) {
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  if (p >= n) return;
#pragma unroll
  for (int c = 0; c < kAcc; ++c) acc[kAcc * p + c] = 0;
}

// parent[] while a kernel unites trees in it (the tile's array in LDS in the local launch, SCOPE
// workgroup; the scan's in global memory in the hook launch, SCOPE agent).  Invariants:
// parent[x] <= x for every usable x, equal only at a root; a word only ever decreases; and whatever
// value a reader gets for parent[x], however stale, is x itself or an ancestor of x in x's tree.
// Other threads (in the hook launch: other workgroups, on other XCDs) change these words under us,
// so every read is a relaxed atomic load of that scope: a stale value is still an ancestor, a value
// the compiler kept in a register across a retry is not re-read at all.
template <int SCOPE>
EV_DEVINL int uf_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// The root of x.  Ends because every step goes to a strictly smaller index.  On the way parent[x]
// is lowered to its grandparent (path halving): x is no root there and never becomes one again,
// so this never meets the CAS of a union, and atomicMin keeps the word decreasing.
template <int SCOPE>
EV_DEVINL int uf_find(int* parent, int x) {
  int p = uf_load<SCOPE>(parent + x);
  while (p != x) {
    const int g = uf_load<SCOPE>(parent + p);
    if (g != p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// Lock-free: the CAS fails only if the higher root got a parent meanwhile, which is below it, so
// the retry starts strictly lower; nothing here waits for another thread to act.
template <int SCOPE>
EV_DEVINL void uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(parent, a);
    b = uf_find<SCOPE>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);   // device scope (wider than the tile needs)
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_local_kernel(
    const double* __restrict__ euler, const int* __restrict__ valid, int rows, int cols,
    int connectivity, double threshold, int* __restrict__ parent) {
#pragma clang fp contract(off)
  __shared__ int lp[kGrainThreads];          // the tile's parents: thread indices, -1 = unusable
  __shared__ double lq[kGrainThreads][4];    // the tile's quaternions
  const int tid = threadIdx.x, ti = tid / kTile, tj = tid % kTile;
  const int tiles_c = (int)(((long long)cols + kTile - 1) / kTile);
  const long long i0 = (long long)(blockIdx.x / tiles_c) * kTile;
  const long long j0 = (long long)(blockIdx.x % tiles_c) * kTile;
  const long long i = i0 + ti, j = j0 + tj;
  const bool on = i < rows && j < cols;
  const long long p = i * cols + j;
  const bool use = on && usable_point(euler, valid, p);
  Q4 q{0.0, 0.0, 0.0, 1.0};
  if (use) q = point_quat(euler, p);
  lp[tid] = use ? tid : -1;
  lq[tid][0] = q.x, lq[tid][1] = q.y, lq[tid][2] = q.z, lq[tid][3] = q.w;
  __syncthreads();
  if (use) {
    const Q4 pinv = qconj(q);
    for (int a = 0; a <= 1; ++a) {
      for (int b = -1; b <= 1; ++b) {
        if (!map_offset(connectivity, a, b) || (a == 0 && b < 0)) continue;
        if (ti + a >= kTile || tj + b < 0 || tj + b >= kTile) continue;   // the hook launch's edge
        const int t = tid + a * kTile + b;
        // off the grid or unusable: -1, which no union ever writes or removes
        if (uf_load<__HIP_MEMORY_SCOPE_WORKGROUP>(lp + t) < 0) continue;
        const Q4 qq{lq[t][0], lq[t][1], lq[t][2], lq[t][3]};
        if (disorientation_deg(pinv, qq) <= threshold)
          uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, tid, t);
      }
    }
  }
  __syncthreads();
  if (on) {
    // thread order within the tile is flat-index order, so the tile root is the lowest flat index
    const int l = use ? uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, tid) : 0;
    parent[p] = use ? (int)((i0 + l / kTile) * cols + j0 + l % kTile) : -1;
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_hook_kernel(
    const double* __restrict__ euler, const int* __restrict__ valid, int rows, int cols,
    int connectivity, double threshold, int* parent) {
#pragma clang fp contract(off)
  const long long n = (long long)rows * cols;
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  if (p >= n) return;
  const int i = (int)(p / cols), j = (int)(p % cols);
  // only the last row and the first and last column of a tile have forward edges that leave it
  if (i % kTile != kTile - 1 && j % kTile != 0 && j % kTile != kTile - 1) return;
  if (!usable_point(euler, valid, p)) return;
  const Q4 pinv = qconj(point_quat(euler, p));
  // the forward half of map_offset's neighbours: right, then below-left, below, below-right
  for (int a = 0; a <= 1; ++a) {
    for (int b = -1; b <= 1; ++b) {
      if (!map_offset(connectivity, a, b) || (a == 0 && b < 0)) continue;
      if (i + a >= rows || j + b < 0 || j + b >= cols) continue;
      if (i / kTile == (i + a) / kTile && j / kTile == (j + b) / kTile) continue;   // local's edge
      const long long q = p + (long long)a * cols + b;
      if (!usable_point(euler, valid, q)) continue;
      if (disorientation_deg(pinv, point_quat(euler, q)) <= threshold)
        uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)p, (int)q);
    }
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_flatten_kernel(
    const int* __restrict__ parent, int n, int* __restrict__ root) {
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  if (p >= n) return;
  int x = parent[p];
  if (x >= 0) {
    for (int up = parent[x]; up != x; up = parent[x]) x = up;
  }
  root[p] = x;
}

// Threads of a block hold consecutive points.  Within each run of threads with the same key,
// v[0..K) of the run's first thread becomes the run's sum; returns whether this thread is such a
// first thread.  Every thread of the block must call it (it has a barrier).  First a segmented
// shuffle reduction within each wave; then a run that starts a wave and continues the wave before
// hands its sum over through LDS to the thread where the run began.  (A key may come back in a
// later run: runs, not keys, are what is summed, so the reach of a lane ends at its own run's
// last lane.)
template <int K>
EV_DEVINL bool run_sum(int key, long long (&v)[K]) {
  __shared__ int first_key[kGrainWaves], last_key[kGrainWaves], whole[kGrainWaves];
  __shared__ long long first_sum[kGrainWaves][K];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(key, 1, 64);
  const bool head = lane == 0 || before != key;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int last = above ? lane + __ffsll((long long)above) - 1 : 63;   // of this lane's run
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const long long t = __shfl_down(v[c], o, 64);
      if (lane + o <= last) v[c] += t;
    }
  }
  if (lane == 0) {
    first_key[wave] = key;
    whole[wave] = last == 63;
#pragma unroll
    for (int c = 0; c < K; ++c) first_sum[wave][c] = v[c];
  }
  if (lane == 63) last_key[wave] = key;
  __syncthreads();
  if (!head) return false;
  if (lane == 0 && wave > 0 && last_key[wave - 1] == key) return false;   // begun in an earlier wave
  if (last == 63) {
    for (int w = wave + 1; w < kGrainWaves && first_key[w] == key; ++w) {
#pragma unroll
      for (int c = 0; c < K; ++c) v[c] += first_sum[w][c];
      if (!whole[w]) break;
    }
  }
  return true;
}

EV_DEVINL void acc_add(long long* slot, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)v);   // two's complement
}

__global__ __launch_bounds__(kGrainThreads) void grain_accum_kernel(
    const double* __restrict__ euler, const int* __restrict__ root, int n,
    long long* __restrict__ acc) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  const int r = p < n ? root[p] : -1;
  long long v[5] = {0, 0, 0, 0, 0};
  if (r >= 0) {
    const Q4 qr = point_quat(euler, r), rinv = qconj(qr), qp = point_quat(euler, p);
    Q4 eq = qp;
    double best = 1e300;
    for (int c = 0; c < 24; ++c) {
      const Q4 s = qmul(cubic_op(c), qp);
      const double w = qmag(qmul(rinv, s));
      if (w < best) {
        best = w;
        eq = s;
      }
    }
    const double sign = eq.x * qr.x + eq.y * qr.y + eq.z * qr.z + eq.w * qr.w < 0.0 ? -1.0 : 1.0;
    v[0] = llrint(sign * eq.x * kQuatFix);
    v[1] = llrint(sign * eq.y * kQuatFix);
    v[2] = llrint(sign * eq.z * kQuatFix);
    v[3] = llrint(sign * eq.w * kQuatFix);
    v[4] = 1;
  }
  const bool head = run_sum(r, v);
  if (head && r >= 0) {
    long long* slot = acc + (long long)kAcc * r;
    acc_add(slot + 0, v[0]);
    acc_add(slot + 1, v[1]);
    acc_add(slot + 2, v[2]);
    acc_add(slot + 3, v[3]);
    acc_add(slot + 5, v[4]);
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_grod_kernel(
    const double* __restrict__ euler, const int* __restrict__ root, int n,
    long long* acc, double* __restrict__ grain_euler, float* __restrict__ grod, int want_gos) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  const int r = p < n ? root[p] : -1;
  long long v[1] = {0};
  if (r >= 0) {
    // the quaternion sums are complete (the accum launch is), the GROD slot is not read here
    const long long* slot = acc + (long long)kAcc * r;
    const Q4 mean = qnormalize(Q4{(double)slot[0], (double)slot[1], (double)slot[2], (double)slot[3]});
    if (grain_euler) {
      double e[3];
      as_euler_zxz(mean, e);
      grain_euler[3 * p] = e[0], grain_euler[3 * p + 1] = e[1], grain_euler[3 * p + 2] = e[2];
    }
    if (grod || want_gos) {
      const double deg = disorientation_deg(qconj(point_quat(euler, p)), mean);
      if (grod) grod[p] = (float)deg;
      v[0] = llrint(deg * kGrodFix);
    }
  } else if (p < n) {
    if (grain_euler) grain_euler[3 * p] = grain_euler[3 * p + 1] = grain_euler[3 * p + 2] = NAN;
    if (grod) grod[p] = NAN;
  }
  if (want_gos) {   // uniform: every thread of the block gets here
    const bool head = run_sum(r, v);
    if (head && r >= 0) acc_add(acc + (long long)kAcc * r + 4, v[0]);
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_finish_kernel(
    const int* __restrict__ root, const long long* __restrict__ acc, int rows, int cols,
    int connectivity, float* __restrict__ gos, unsigned char* __restrict__ boundary) {
#pragma clang fp contract(off)
  const long long n = (long long)rows * cols;
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  if (p >= n) return;
  const int r = root[p];
  if (gos) {
    float g = NAN;
    if (r >= 0) {
      const long long* slot = acc + (long long)kAcc * r;
      g = (float)((double)slot[4] / kGrodFix / (double)slot[5]);
    }
    gos[p] = g;
  }
  if (boundary) {
    unsigned char edge = 0;
    if (r >= 0) {
      const int i = (int)(p / cols), j = (int)(p % cols);
      for (int a = -1; a <= 1; ++a) {
        for (int b = -1; b <= 1; ++b) {
          if (!map_offset(connectivity, a, b)) continue;
          if (i + a < 0 || i + a >= rows || j + b < 0 || j + b >= cols) continue;
          // two points have the same id iff they have the same root; -1 stays -1
          if (root[p + (long long)a * cols + b] != r) edge = 1;
        }
      }
    }
    boundary[p] = edge;
  }
}

// exclusive prefix sum of v over the block's threads and its total; lds holds kGrainWaves ints
EV_DEVINL int block_scan_excl(int v, int* lds, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kGrainWaves; ++k) {
    const int t = lds[k];
    if (k < w) before += t;
    total += t;
  }
  __syncthreads();
  return before + inc - v;
}

// block b owns the points [b kScanBlock, (b + 1) kScanBlock): how many of them are roots
__global__ __launch_bounds__(kGrainThreads) void grain_count_kernel(
    const int* __restrict__ root, int n, int* __restrict__ bsum) {
  __shared__ int lds[kGrainWaves];
  const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  int mine = 0;
#pragma unroll
  for (int c = 0; c < kScanChunks; ++c) {
    const long long p = base + (long long)c * kGrainThreads;
    mine += p < n && root[p] == (int)p;
  }
  int total;
  block_scan_excl(mine, lds, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: bsum (nb,) -> its exclusive prefix sum, in place, kGrainThreads entries at a time
__global__ __launch_bounds__(kGrainThreads) void grain_offsets_kernel(int* __restrict__ bsum,
                                                                      int nb) {
  __shared__ int lds[kGrainWaves];
  int carry = 0;
  for (int s = 0; s < nb; s += kGrainThreads) {   // uniform trip count
    const int k = s + threadIdx.x;
    const int v = k < nb ? bsum[k] : 0;
    int total;
    const int ex = block_scan_excl(v, lds, total);
    if (k < nb) bsum[k] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_rank_kernel(
    const int* __restrict__ root, int n, const int* __restrict__ bsum, int* __restrict__ rank) {
  __shared__ int lds[kGrainWaves];
  const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  int carry = bsum[blockIdx.x];
#pragma unroll 1
  for (int c = 0; c < kScanChunks; ++c) {   // uniform trip count: every thread reaches the barriers
    const long long p = base + (long long)c * kGrainThreads;
    const int flag = p < n && root[p] == (int)p;
    int total;
    const int ex = block_scan_excl(flag, lds, total);
    if (p < n) rank[p] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(kGrainThreads) void grain_relabel_kernel(
    const int* __restrict__ rank, int n, int* __restrict__ grain_id) {
  const long long p = (long long)blockIdx.x * kGrainThreads + threadIdx.x;
  if (p >= n) return;
  const int r = grain_id[p];   // only this thread touches grain_id[p]
  grain_id[p] = r >= 0 ? rank[r] : -1;
}

static bool grain_grid_ok(int rows, int cols) {
  return rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31);
}

static long long grain_scan_blocks(long long n) { return (n + kScanBlock - 1) / kScanBlock; }

}  // namespace ev

using namespace ev;

extern "C" size_t ebsdvae_grain_work(int rows, int cols) {
  if (!grain_grid_ok(rows, cols)) return 0;
  const long long n = (long long)rows * cols;
  return (size_t)n * (kAcc * sizeof(long long) + 2 * sizeof(int)) +
         (size_t)grain_scan_blocks(n) * sizeof(int);
}

extern "C" int ebsdvae_segment_grains(const double* euler, const int* valid, int rows, int cols,
                                      int connectivity, double threshold_deg, int* grain_id,
                                      double* grain_euler, float* gos, float* grod,
                                      unsigned char* boundary, void* work,
                                      ebsdvae_stream_t stream) {
  EV_REQUIRE(euler && grain_id && work, "segment_grains: null pointer");
  EV_REQUIRE(((uintptr_t)work & 7) == 0, "segment_grains: work must be 8-byte aligned");
  EV_REQUIRE(grain_grid_ok(rows, cols), "segment_grains: grid %d x %d", rows, cols);
  EV_REQUIRE(connectivity == 4 || connectivity == 8,
             "segment_grains: connectivity=%d is neither 4 nor 8", connectivity);
  EV_REQUIRE(threshold_deg >= 0.0 && threshold_deg <= DBL_MAX,
             "segment_grains: threshold_deg=%g must be finite and not negative", threshold_deg);
  const long long nn = (long long)rows * cols;
  const int n = (int)nn;
  GrainWork w;
  w.acc = (long long*)work;
  w.parent = (int*)(w.acc + kAcc * nn);
  w.rank = w.parent + nn;
  w.bsum = w.rank + nn;
  const int nb = (int)grain_scan_blocks(nn);
  const bool sums = grain_euler || gos || grod;
  const dim3 grid((unsigned)((nn + kGrainThreads - 1) / kGrainThreads)), block(kGrainThreads);
  hipStream_t s = (hipStream_t)stream;

  const long long tiles = (((long long)rows + kTile - 1) / kTile) * (((long long)cols + kTile - 1) / kTile);
  if (sums) hipLaunchKernelGGL(grain_zero_kernel, grid, block, 0, s, n, w.acc);
  hipLaunchKernelGGL(grain_local_kernel, dim3((unsigned)tiles), block, 0, s, euler, valid, rows,
                     cols, connectivity, threshold_deg, w.parent);
  hipLaunchKernelGGL(grain_hook_kernel, grid, block, 0, s, euler, valid, rows, cols, connectivity,
                     threshold_deg, w.parent);
  hipLaunchKernelGGL(grain_flatten_kernel, grid, block, 0, s, (const int*)w.parent, n, grain_id);
  if (sums) {
    hipLaunchKernelGGL(grain_accum_kernel, grid, block, 0, s, euler, (const int*)grain_id, n,
                       w.acc);
    hipLaunchKernelGGL(grain_grod_kernel, grid, block, 0, s, euler, (const int*)grain_id, n, w.acc,
                       grain_euler, grod, gos ? 1 : 0);
  }
  if (gos || boundary)
    hipLaunchKernelGGL(grain_finish_kernel, grid, block, 0, s, (const int*)grain_id,
                       (const long long*)w.acc, rows, cols, connectivity, gos, boundary);
  hipLaunchKernelGGL(grain_count_kernel, dim3((unsigned)nb), block, 0, s, (const int*)grain_id, n,
                     w.bsum);
  hipLaunchKernelGGL(grain_offsets_kernel, dim3(1), block, 0, s, w.bsum, nb);
  hipLaunchKernelGGL(grain_rank_kernel, dim3((unsigned)nb), block, 0, s, (const int*)grain_id, n,
                     (const int*)w.bsum, w.rank);
  hipLaunchKernelGGL(grain_relabel_kernel, grid, block, 0, s, (const int*)w.rank, n, grain_id);
  return evh::check_launch("segment_grains");
}
