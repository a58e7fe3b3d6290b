// Batched orientation consensus: the reference's per-query
// `find_best_orientation` (latice/index/faiss_db.py:258-372, identical in chroma_db.py:261-375)
// for many queries in one launch, one wave per query, one lane per candidate.  Float64
// throughout, restating scipy 1.15 `Rotation` (the reference's dependency) arithmetic:
//
//   from_euler("zxz", deg)  extrinsic: q = q_z(c) (x) q_x(b) (x) q_z(a), scalar-last quats
//   p * q                   Hamilton product p (x) q (q applied first)
//   inv()                   conjugate;   magnitude() = 2 atan2(|v|, |w|)
//   mean()                  the eigenvector of the largest eigenvalue of sum q q^T
//   as_euler("zxz", deg)    Bernardes & Viollet (2022), scipy's algorithm incl. its
//                           gimbal-lock branches (third angle 0) and the wrap to [-180, 180]
//
// Per query (candidates = the orientations of its top-n cosine matches, in match order):
//   for it < min(max_iter, n): ref = cand[it]; similar = {j : angle(ref^-1 cand_j) < thr}
//     if |similar| >= min_matches: each similar candidate is replaced by the one of its 24
//       cubic-symmetry equivalents QUAT_SYM_i (x) cand_j closest to ref (first minimum,
//       faiss_db.py:374-398); mean of those -> Euler; success; stop.
//   best = mean on success, else cand[0]; similar = the last iteration's set (a bit mask).
// The symmetric equivalents are kept as quaternions; the reference round-trips them through
// Euler angles before the mean, which moves the result by ~1e-12 degrees.
#include "common.h"
#include "orient_math.h"
#include "../../include/ebsdvae.h"

namespace ev {

__global__ __launch_bounds__(64) void orient_consensus_kernel(
    const double* __restrict__ ori, const long long* __restrict__ idx, int n, double thr_deg,
    int min_matches, int max_iter, double* __restrict__ best, double* __restrict__ mean,
    int* __restrict__ success, unsigned long long* __restrict__ similar) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const bool live = lane < n;
  long long row = live ? idx[(size_t)q * n + lane] : -1;
  if (row < 0) row = 0;
  const double* e = ori + row * 3;
  const Q4 cq = live ? from_euler_zxz(e[0], e[1], e[2]) : Q4{0, 0, 0, 1};
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
        for (int k = 0; k < 24; ++k) {
          const Q4 sym = qnormalize(Q4{kCubic[k][0], kCubic[k][1], kCubic[k][2], kCubic[k][3]});
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
    similar[q] = mask;
    double b[3];
    if (ok) {
      b[0] = mean_e[0]; b[1] = mean_e[1]; b[2] = mean_e[2];
    } else {
      b[0] = e[0]; b[1] = e[1]; b[2] = e[2];   // the closest match (candidate 0)
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      best[(size_t)q * 3 + i] = b[i];
      mean[(size_t)q * 3 + i] = mean_e[i];
    }
  }
}

}  // namespace ev

using namespace ev;

extern "C" int ebsdvae_orient_consensus(const double* orientations, const long long* cand_idx,
                                        int Q, int n, double threshold_deg, int min_matches,
                                        int max_iterations, double* best, double* mean,
                                        int* success, unsigned long long* similar_mask,
                                        ebsdvae_stream_t stream) {
  EV_REQUIRE(orientations && cand_idx && best && mean && success && similar_mask,
             "orient_consensus: null pointer");
  EV_REQUIRE(Q >= 0 && n >= 1 && n <= 64, "orient_consensus: n=%d (1..64)", n);
  if (Q == 0) return 0;
  hipLaunchKernelGGL(orient_consensus_kernel, dim3(Q), dim3(64), 0, (hipStream_t)stream, orientations,
                     cand_idx, n, threshold_deg, min_matches, max_iterations, best, mean, success,
                     similar_mask);
  return evh::check_launch("orient_consensus");
}
