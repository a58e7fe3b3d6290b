// Scan maps ("Scan maps"): what a finished scan is looked at with, from the
// result rows index_scan leaves on the device.  Three independent kernels, no scratch, no LDS, no
// atomics; every output is a function of its inputs alone, bit for bit.  All float arithmetic is
// float64 with the helpers of orient_math.h, contraction off.
//
//   ipf_kernel   one thread per orientation: ColorKeyGenerator.generate_ipf_color
//                (latice/utils/colorkey.py:64-130) of row `axis` of the rotation matrix, as
//                get_color_key (latice/utils/utils.py:206-240) feeds it.  The 24 cubic equivalents
//                of the direction in QUAT_SYM order, then their 24 negations; each flipped to
//                z >= 0; chi = acos(z), eta = atan2(y, x); the FIRST one inside the reference's
//                sector 0 <= eta <= 45 deg, 0 <= chi <= acos(1 / sqrt 3) wins (the sector is larger
//                than the fundamental triangle, so the order is observable), else the last tried.
//   osm_kernel   one wave per scan point, candidate l of the point's row in lane l.  A neighbour's
//                row is loaded once, entry l in lane l, and broadcast entry by entry; a lane keeps
//                whether its own candidate occurred, one ballot counts the lanes.  Integers up to
//                the one or two float32 divisions.
//   kam_kernel   one thread per scan point: the cubic disorientation to each on-grid neighbour in
//                row-major offset order, the consensus kernel's min over the 24 equivalents
//                (csrc/orient.hip), a float64 sum in that order and one division.
// cubic_op, finite3 and map_offset are shared with grains.hip: scan_grid.h.
#include "scan_grid.h"
#include "../../include/ebsdvae.h"

#include <math.h>

namespace ev {

constexpr int kMapThreads = 256;
constexpr int kMapWaves = kMapThreads / 64;

// scipy Rotation.as_matrix of a unit quaternion
EV_DEVINL void qmatrix(const Q4& q, double m[3][3]) {
#pragma clang fp contract(off)
  const double x2 = q.x * q.x, y2 = q.y * q.y, z2 = q.z * q.z, w2 = q.w * q.w;
  const double xy = q.x * q.y, zw = q.z * q.w, xz = q.x * q.z, yw = q.y * q.w;
  const double yz = q.y * q.z, xw = q.x * q.w;
  m[0][0] = x2 - y2 - z2 + w2;
  m[1][0] = 2.0 * (xy + zw);
  m[2][0] = 2.0 * (xz - yw);
  m[0][1] = 2.0 * (xy - zw);
  m[1][1] = -x2 + y2 - z2 + w2;
  m[2][1] = 2.0 * (yz + xw);
  m[0][2] = 2.0 * (xz + yw);
  m[1][2] = 2.0 * (yz - xw);
  m[2][2] = -x2 - y2 + z2 + w2;
}

// a colour channel 255 v / max as 8 bits, ties to even as Python's round; what is not a number
// (no equivalent inside the sector: the reference's sqrt of a negative) is 0
EV_DEVINL unsigned char ipf_level(double v, double mx) {
#pragma clang fp contract(off)
  const double l = rint(255.0 * v / mx);
  return l >= 0.0 ? (unsigned char)(l < 255.0 ? l : 255.0) : (unsigned char)0;
}

__global__ __launch_bounds__(kMapThreads) void ipf_kernel(const double* __restrict__ euler,
                                                          long long n, int axis,
                                                          unsigned char* __restrict__ rgb) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= n) return;
  const double ea = euler[3 * i], eb = euler[3 * i + 1], ec = euler[3 * i + 2];
  unsigned char* out = rgb + 3 * i;
  if (!finite3(ea, eb, ec)) {
    out[0] = out[1] = out[2] = 0;
    return;
  }
  double m[3][3];
  qmatrix(from_euler_zxz(ea, eb, ec), m);
  double vx = axis == 0 ? m[0][0] : axis == 1 ? m[1][0] : m[2][0];
  double vy = axis == 0 ? m[0][1] : axis == 1 ? m[1][1] : m[2][1];
  double vz = axis == 0 ? m[0][2] : axis == 1 ? m[1][2] : m[2][2];
  const double nrm = sqrt(vx * vx + vy * vy + vz * vz);
  vx /= nrm, vy /= nrm, vz /= nrm;

  const double eta_hi = 45.0 * (kPi / 180.0), chi_hi = acos(1.0 / sqrt(3.0));
  double chi = 0.0, eta = 0.0;
  bool found = false;
  for (int t = 0; t < 48 && !found; ++t) {
    double s[3][3];
    qmatrix(cubic_op(t < 24 ? t : t - 24), s);
    double x = s[0][0] * vx + s[0][1] * vy + s[0][2] * vz;
    double y = s[1][0] * vx + s[1][1] * vy + s[1][2] * vz;
    double z = s[2][0] * vx + s[2][1] * vy + s[2][2] * vz;
    if (t >= 24) x = -x, y = -y, z = -z;
    if (z < 0.0) x = -x, y = -y, z = -z;
    // a pole may come out one ulp above 1, where the reference's acos has no answer: chi = 0
    chi = acos(z < 1.0 ? z : 1.0);
    eta = atan2(y, x);
    found = !(eta < 0.0 || eta > eta_hi || chi < 0.0 || chi > chi_hi);
  }

  const double k180 = 180.0 / kPi;
  const double chi_max = chi_hi * k180, eta_deg = eta * k180, chi_deg = chi * k180;
  double r = 1.0 - chi_deg / chi_max;
  double b = fabs(eta_deg - 0.0) / (45.0 - 0.0);
  double g = 1.0 - b;
  g *= chi_deg / chi_max;
  b *= chi_deg / chi_max;
  r = sqrt(r), g = sqrt(g), b = sqrt(b);
  double mx = r;   // Python's max: the first of the largest, a later one only if greater
  if (g > mx) mx = g;
  if (b > mx) mx = b;
  out[0] = ipf_level(r, mx);
  out[1] = ipf_level(g, mx);
  out[2] = ipf_level(b, mx);
}

__global__ __launch_bounds__(kMapThreads) void osm_kernel(const long long* __restrict__ cand,
                                                          int k, int rows, int cols,
                                                          int connectivity, int normalize,
                                                          float* __restrict__ osm) {
  const long long n = (long long)rows * cols;
  const long long p = (long long)blockIdx.x * kMapWaves + (threadIdx.x >> 6);
  if (p >= n) return;   // the same in every lane of the wave
  const int lane = threadIdx.x & 63;
  const int i = (int)(p / cols), j = (int)(p % cols);
  const long long mine = lane < k ? cand[p * k + lane] : -1;
  int shared = 0, neighbours = 0;
  for (int a = -1; a <= 1; ++a) {
    for (int b = -1; b <= 1; ++b) {
      if (!map_offset(connectivity, a, b)) continue;
      if (i + a < 0 || i + a >= rows || j + b < 0 || j + b >= cols) continue;
      const long long q = p + (long long)a * cols + b;
      const long long theirs = lane < k ? cand[q * k + lane] : -1;
      // entry l of the neighbour's row, the same in every lane: l is uniform, so the two halves
      // are read out of lane l into scalar registers (v_readlane_b32), no trip through the LDS
      const int lo = (int)theirs, hi = (int)(theirs >> 32);
      bool occurs = false;
      for (int l = 0; l < k; ++l) {
        const long long entry = ((long long)__builtin_amdgcn_readlane(hi, l) << 32) |
                                (unsigned)__builtin_amdgcn_readlane(lo, l);
        occurs |= entry == mine;
      }
      shared += __popcll(__ballot(occurs && mine >= 0));
      ++neighbours;
    }
  }
  if (lane == 0) {
    float v = 0.f;
    if (neighbours) {
      v = (float)shared / (float)neighbours;
      if (normalize) v = v / (float)k;
    }
    osm[p] = v;
  }
}

__global__ __launch_bounds__(kMapThreads) void kam_kernel(const double* __restrict__ euler,
                                                          int rows, int cols, int connectivity,
                                                          double max_deg, float* __restrict__ kam) {
#pragma clang fp contract(off)
  const long long n = (long long)rows * cols;
  const long long p = (long long)blockIdx.x * kMapThreads + threadIdx.x;
  if (p >= n) return;
  const double pa = euler[3 * p], pb = euler[3 * p + 1], pc = euler[3 * p + 2];
  if (!finite3(pa, pb, pc)) {
    kam[p] = NAN;
    return;
  }
  const Q4 pinv = qconj(from_euler_zxz(pa, pb, pc));
  const int i = (int)(p / cols), j = (int)(p % cols);
  double sum = 0.0;
  int kept = 0;
  for (int a = -1; a <= 1; ++a) {
    for (int b = -1; b <= 1; ++b) {
      if (!map_offset(connectivity, a, b)) continue;
      if (i + a < 0 || i + a >= rows || j + b < 0 || j + b >= cols) continue;
      const long long q = p + (long long)a * cols + b;
      const double qa = euler[3 * q], qb = euler[3 * q + 1], qc = euler[3 * q + 2];
      if (!finite3(qa, qb, qc)) continue;
      const Q4 qq = from_euler_zxz(qa, qb, qc);
      double best = 1e300;
      for (int c = 0; c < 24; ++c) {
        const double w = qmag(qmul(pinv, qmul(cubic_op(c), qq)));
        if (w < best) best = w;
      }
      const double deg = best / kDeg;
      if (deg <= max_deg) {
        sum += deg;
        ++kept;
      }
    }
  }
  kam[p] = kept ? (float)(sum / kept) : 0.f;
}

static int map_check_grid(const char* who, int rows, int cols, int connectivity) {
  EV_REQUIRE(rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31), "%s: grid %d x %d", who,
             rows, cols);
  EV_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity=%d is neither 4 nor 8", who,
             connectivity);
  return 0;
}

}  // namespace ev

using namespace ev;

extern "C" int ebsdvae_ipf_colors(const double* euler, long long n, int axis, unsigned char* rgb,
                                  ebsdvae_stream_t stream) {
  EV_REQUIRE(euler && rgb, "ipf_colors: null pointer");
  EV_REQUIRE(axis >= 0 && axis <= 2, "ipf_colors: axis=%d outside 0..2", axis);
  EV_REQUIRE(n >= 0 && n < (1LL << 31) * kMapThreads, "ipf_colors: n=%lld", n);
  if (n == 0) return 0;
  hipLaunchKernelGGL(ipf_kernel, dim3((unsigned)((n + kMapThreads - 1) / kMapThreads)),
                     dim3(kMapThreads), 0, (hipStream_t)stream, euler, n, axis, rgb);
  return evh::check_launch("ipf_colors");
}

extern "C" int ebsdvae_orientation_similarity(const long long* cand_idx, int k, int rows, int cols,
                                              int connectivity, int normalize, float* osm,
                                              ebsdvae_stream_t stream) {
  EV_REQUIRE(cand_idx && osm, "orientation_similarity: null pointer");
  EV_REQUIRE(k >= 1 && k <= 64, "orientation_similarity: k=%d outside 1..64", k);
  if (map_check_grid("orientation_similarity", rows, cols, connectivity)) return 1;
  const long long n = (long long)rows * cols;
  hipLaunchKernelGGL(osm_kernel, dim3((unsigned)((n + kMapWaves - 1) / kMapWaves)),
                     dim3(kMapThreads), 0, (hipStream_t)stream, cand_idx, k, rows, cols,
                     connectivity, normalize, osm);
  return evh::check_launch("orientation_similarity");
}

extern "C" int ebsdvae_kernel_misorientation(const double* euler, int rows, int cols,
                                             int connectivity, double max_deg, float* kam,
                                             ebsdvae_stream_t stream) {
  EV_REQUIRE(euler && kam, "kernel_misorientation: null pointer");
  if (map_check_grid("kernel_misorientation", rows, cols, connectivity)) return 1;
  EV_REQUIRE(max_deg >= 0.0, "kernel_misorientation: max_deg=%g must not be negative", max_deg);
  const long long n = (long long)rows * cols;
  hipLaunchKernelGGL(kam_kernel, dim3((unsigned)((n + kMapThreads - 1) / kMapThreads)),
                     dim3(kMapThreads), 0, (hipStream_t)stream, euler, rows, cols, connectivity,
                     max_deg, kam);
  return evh::check_launch("kernel_misorientation");
}
