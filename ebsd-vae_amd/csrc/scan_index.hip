// Whole-scan indexing: cosine top-k and orientation consensus without the launch boundary
// between them, so a query's candidate list never leaves the wave that merged it.
//
//   ebsdvae_index_latents   per query: the k best dictionary rows (search.hip), then the
//                           consensus of their orientations (orient.hip); writes only the
//                           compact per-query result -- best orientation, success, top score,
//                           top row, size of the similar set -- and the candidate lists only
//                           when asked for.
//
// Pass 1 is search.hip's chunked scoring (topk_chunk_kernel<D>), launched unchanged.  Pass 2
// is one wave per query: it merges and sorts the chunk lists exactly as topk_merge_kernel
// does (tk_merge_sorted), after which lane l < k holds candidate l in match order; the same
// lane loads orientations[row] and the wave runs orient_consensus_kernel's body, restated
// here statement for statement over the shared helpers of orient_math.h (the compiler
// contracts a * b + c by context, so the consensus is kept in this one form in both kernels;
// tests/test_gpu_scan_index.py holds the two to the same bits).  Every output equals
// ebsdvae_cosine_topk followed by ebsdvae_orient_consensus bit for bit; a query's result does
// not depend on the others in the launch (the chunk count does, but the merged list is the
// exact top-k under a total order, whatever the chunking).
#include "common.h"
#include "topk.h"
#include "orient_math.h"
#include "../../include/ebsdvae.h"

namespace ev {

__global__ __launch_bounds__(64) void index_merge_consensus_kernel(
    const float* __restrict__ ps, const int* __restrict__ pi, int nchunk, int k,
    const double* __restrict__ ori, double thr_deg, int min_matches, int max_iter,
    double* __restrict__ best, int* __restrict__ success, float* __restrict__ top_score,
    long long* __restrict__ top_row, int* __restrict__ n_similar, float* __restrict__ cand_s,
    long long* __restrict__ cand_i) {
  const int q = blockIdx.x, lane = threadIdx.x;
  float v;
  int i;
  tk_merge_sorted(ps, pi, q, nchunk, k, lane, v, i);
  const bool live = lane < k;
  const long long found = (i == 0x7fffffff) ? -1 : (long long)i;
  if (live) {
    if (cand_s) cand_s[(size_t)q * k + lane] = v;
    if (cand_i) cand_i[(size_t)q * k + lane] = found;
  }
  const long long row = (live && found >= 0) ? found : 0;
  const double* e = ori + row * 3;
  const Q4 cq = live ? from_euler_zxz(e[0], e[1], e[2]) : Q4{0, 0, 0, 1};
  // from here on orient_consensus_kernel's body, statement for statement (n == k)
  const int n = k;
  const int iters = min(max_iter, n);
  unsigned long long mask = 0;
  int ok = 0;
  double mean_e[3] = {NAN, NAN, NAN};
  for (int it = 0; it < iters; ++it) {
    const Q4 ref{__shfl(cq.x, it, 64), __shfl(cq.y, it, 64), __shfl(cq.z, it, 64), __shfl(cq.w, it, 64)};
    const Q4 rinv = qconj(ref);
    const double ang = qmag(qmul(rinv, cq)) / kDeg;
    mask = __ballot(live && ang < thr_deg);
    if (__popcll(mask) >= min_matches) {
      const bool mine = (mask >> lane) & 1ull;
      Q4 s{0, 0, 0, 1};
      if (mine) {   // closest cubic-symmetry equivalent to ref (first minimum)
        double bm = 1e300;
        for (int c = 0; c < 24; ++c) {
          const Q4 sym = qnormalize(Q4{kCubic[c][0], kCubic[c][1], kCubic[c][2], kCubic[c][3]});
          const Q4 eq = qmul(sym, cq);
          const double m = qmag(qmul(rinv, eq));
          if (m < bm) { bm = m; s = eq; }
        }
      }
      // mean: K = sum q q^T over the similar set (scipy Rotation.mean, unit weights)
      const double f = mine ? 1.0 : 0.0;
      const double qv[4] = {s.x, s.y, s.z, s.w};
      double K[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {
          K[a][b] = wsum64(f * qv[a] * qv[b]);
          K[b][a] = K[a][b];
        }
      const Q4 m = top_eigvec(K);
      as_euler_zxz(m, mean_e);
      ok = 1;
      break;
    }
  }
  if (lane == 0) {
    success[q] = ok;
    top_score[q] = v;
    top_row[q] = found;
    n_similar[q] = __popcll(mask);
#pragma unroll
    for (int c = 0; c < 3; ++c) best[(size_t)q * 3 + c] = ok ? mean_e[c] : e[c];
  }
}

}  // namespace ev

using namespace ev;

extern "C" size_t ebsdvae_index_latents_work(long long N, int Q, int d, int k) {
  return ebsdvae_cosine_topk_work(N, Q, d, k);
}

extern "C" int ebsdvae_index_latents(const float* db, long long N, const double* orientations,
                                     const float* queries, int Q, int d, int k,
                                     double threshold_deg, int min_matches, int max_iterations,
                                     double* best, int* success, float* top_score,
                                     long long* top_row, int* n_similar, float* cand_scores,
                                     long long* cand_idx, void* work, ebsdvae_stream_t stream) {
  EV_REQUIRE(db && orientations && queries && best && success && top_score && top_row &&
                 n_similar && work, "index_latents: null pointer");
  EV_REQUIRE(N > 0 && N < 0x7fffffffLL && Q > 0, "index_latents: N=%lld Q=%d out of range", N, Q);
  EV_REQUIRE(k >= 1 && k <= TK_MAXK && k <= N, "index_latents: k=%d (1..%d, <= N)", k, TK_MAXK);
  EV_REQUIRE(d == 16 || d == 32 || d == 64, "index_latents: d=%d (16, 32 or 64)", d);
  const int nc = topk_chunks(N, Q, d);
  float* ps = reinterpret_cast<float*>(work);
  int* pi = reinterpret_cast<int*>(ps + (size_t)Q * nc * k);
  hipStream_t s = (hipStream_t)stream;
  topk_launch_chunks(db, N, queries, Q, d, k, nc, ps, pi, s);
  hipLaunchKernelGGL(index_merge_consensus_kernel, dim3(Q), dim3(64), 0, s, ps, pi, nc, k,
                     orientations, threshold_deg, min_matches, max_iterations, best, success,
                     top_score, top_row, n_similar, cand_scores, cand_idx);
  return evh::check_launch("index_latents");
}
