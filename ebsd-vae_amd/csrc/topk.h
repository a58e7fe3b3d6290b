// Wave-level running top-k shared by the cosine search (search.hip) and the fused scan
// indexing kernel (scan_index.hip): slot s of a query's list lives in lane s, the worst kept
// slot is a wave-uniform admission threshold, and the final list is bitonic-sorted across the
// wave.  Order is (score desc, row index asc) everywhere, so ties break to the lower row.
#pragma once
#include "common.h"

#include <float.h>

namespace ev {

constexpr int TK_WAVES = 4;     // waves per block (each its own query group, same chunk)
constexpr int TK_MAXK = 64;
constexpr int TK_MAXD = 64;

// (s, i) beats (t, j)
EV_DEVINL bool tk_better(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// running top-k of one query in one wave: lane l < k holds slot l
struct TopK {
  float v;
  int i;
  float thr;   // wave-uniform: the worst kept slot (admission threshold)
  int thr_i;
  int thr_lane;
};

EV_DEVINL void tk_init(TopK& t, int k, int lane) {
  t.v = -FLT_MAX;
  t.i = 0x7fffffff;
  (void)k;
  (void)lane;
  t.thr = -FLT_MAX;
  t.thr_i = 0x7fffffff;
  t.thr_lane = 0;
}

// recompute the worst slot among lanes < k (wave reduction, ties -> larger index is worse)
EV_DEVINL void tk_refresh(TopK& t, int k, int lane) {
  float v = lane < k ? t.v : FLT_MAX;
  int i = lane < k ? t.i : -1;
  int l = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    const int l2 = __shfl_xor(l, o, 64);
    // keep the WORSE of the two (the one the other beats)
    if (tk_better(v, i, v2, i2) || (v == v2 && i == i2 && l2 < l)) { v = v2; i = i2; l = l2; }
  }
  t.thr = v;
  t.thr_i = i;
  t.thr_lane = l;
}

// offer candidate (s, idx) held by each lane (valid where ok); inserts the qualifying ones
EV_DEVINL void tk_offer(TopK& t, float s, int idx, bool ok, int k, int lane) {
  unsigned long long m = __ballot(ok && tk_better(s, idx, t.thr, t.thr_i));
  while (m) {
    const int src = __builtin_ctzll(m);
    m &= m - 1;
    const float cs = __shfl(s, src, 64);
    const int ci = __shfl(idx, src, 64);
    if (!tk_better(cs, ci, t.thr, t.thr_i)) continue;   // threshold rose meanwhile
    if (lane == t.thr_lane) { t.v = cs; t.i = ci; }
    tk_refresh(t, k, lane);
  }
}

// bitonic sort of the 64 lanes' (v, i), best first (slots >= k hold -FLT_MAX / INT_MAX)
EV_DEVINL void tk_sort(float& v, int& i, int lane) {
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const float v2 = __shfl_xor(v, stride, 64);
      const int i2 = __shfl_xor(i, stride, 64);
      const bool asc = (lane & size) == 0;          // this block orders best-first
      const bool lower = (lane & stride) == 0;
      const bool take = (lower == asc) ? tk_better(v2, i2, v, i) : tk_better(v, i, v2, i2);
      if (take) { v = v2; i = i2; }
    }
  }
}

// one wave merges the nchunk partial lists of query q (pass 1's [q][chunk][k] layout) and
// sorts them: on return lane l < k holds the l-th best (v, i); an unfilled slot has
// i == 0x7fffffff
EV_DEVINL void tk_merge_sorted(const float* __restrict__ ps, const int* __restrict__ pi, int q,
                               int nchunk, int k, int lane, float& v, int& i) {
  TopK t;
  tk_init(t, k, lane);
  const size_t base = (size_t)q * nchunk * k;
  const int total = nchunk * k;
  for (int c0 = 0; c0 < total; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = c < total;
    const float s = ok ? ps[base + c] : -FLT_MAX;
    const int j = ok ? pi[base + c] : 0x7fffffff;
    tk_offer(t, s, j, ok && j != 0x7fffffff, k, lane);
  }
  v = lane < k ? t.v : -FLT_MAX;
  i = lane < k ? t.i : 0x7fffffff;
  tk_sort(v, i, lane);
}

// ---- host side of pass 1 (defined in search.hip) ----------------------------------------
// chunks the dictionary is cut into for (N, Q, d); the partial lists need
// Q * chunks * k * (sizeof(float) + sizeof(int)) bytes of scratch
int topk_chunks(long long N, int Q, int d);
// launches topk_chunk_kernel<d> over nc chunks; partial lists to ps / pi ([q][chunk][k])
void topk_launch_chunks(const float* db, long long N, const float* queries, int Q, int d, int k,
                        int nc, float* ps, int* pi, hipStream_t stream);

}  // namespace ev
