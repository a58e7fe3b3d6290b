// On-device pattern ingest: the reference's per-sample CPU
// transform of DPdataset.__getitem__ (latice/data_module.py:125-133 + the default pipeline
// create_default_transform, :17-33) applied to a whole batch in one launch:
//
//   dp = raw.astype(float64)                      data_module.py:132
//   ToPILImage:  u8 = uint8(dp * 255)             torchvision 0.21 to_pil_image, float ndarray
//                                                 -> (npimg * 255).astype(np.uint8): truncation
//   Grayscale:   identity on an "L" image
//   CenterCrop(image_size):                       torchvision center_crop: zero-pad a too-small
//                                                 axis by ((c-s)//2, (c-s+1)//2), else offset
//                                                 round((s-c)/2) (Python round: half to even)
//   ToTensor:    float32(u8) / 255                (1, h, w)
//
// Values outside [0, 1] are clamped before the uint8 cast (numpy's out-of-range float->uint8
// cast is platform-defined); NaN maps to 0.  HBM-bound: one thread per output pixel, reads
// the source pixel once (8 B for float64), writes 4 B.
//
// ebsdvae_ingest_patterns_u8 takes detector data that already is uint8: the same crop / pad
// geometry and ToTensor's float32(v) / 255 alone (a true division), which is what the float
// entry point gives for v / 255.0 -- (v / 255.0) * 255.0 truncates back to v for all 256 values.
// One kernel over the source type; the two conversions are overloads of `to_unit`.
#include "common.h"
#include "crop.h"
#include "pattern_src.h"
#include "../../include/ebsdvae.h"

namespace ev {

EV_DEVINL float to_unit(double raw) {
  const double v = raw * 255.0;
  const double c = v > 255.0 ? 255.0 : (v > 0.0 ? v : 0.0);   // NaN -> 0
  const int u8 = (int)c;                                        // truncation, as astype
  return (float)u8 / 255.0f;
}
EV_DEVINL float to_unit(float raw) { return to_unit((double)raw); }
EV_DEVINL float to_unit(unsigned char v) { return (float)v / 255.0f; }

template <typename T>
__global__ __launch_bounds__(256) void ingest_kernel(const T* __restrict__ src, int H0, int W0,
                                                     int oh, int ow, int top, int left,
                                                     long long n, float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % ow);
  const long long r = i / ow;
  const int y = (int)(r % oh);
  const long long b = r / oh;
  const int sy = y + top, sx = x + left;
  float out = 0.f;
  if (sy >= 0 && sy < H0 && sx >= 0 && sx < W0) out = to_unit(src[(b * H0 + sy) * W0 + sx]);
  dst[i] = out;
}

// both entry points: the float one takes src_dtype 0 and 1 (max_dtype 1), the uint8 one is 2
static int ingest(const char* what, int max_dtype, const void* src, int src_dtype, int B, int H0,
                  int W0, int out_h, int out_w, float* dst, ebsdvae_stream_t stream) {
  EV_REQUIRE(src && dst && B >= 0 && H0 > 0 && W0 > 0 && out_h > 0 && out_w > 0, "%s: bad args", what);
  EV_REQUIRE(src_dtype >= 0 && src_dtype <= max_dtype, "%s: src_dtype %d (0 f64, 1 f32)", what, src_dtype);
  if (B == 0) return 0;
  const long long n = (long long)B * out_h * out_w;
  const int top = crop_offset(H0, out_h), left = crop_offset(W0, out_w);
  evh::with_src(src, src_dtype, [&](auto p) {
    hipLaunchKernelGGL(ingest_kernel<evh::elem_t<decltype(p)>>, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, (hipStream_t)stream, p, H0, W0, out_h, out_w, top, left, n, dst);
  });
  return evh::check_launch(what);
}

}  // namespace ev

extern "C" int ebsdvae_ingest_patterns(const void* src, int src_dtype, int B, int H0, int W0,
                                       int out_h, int out_w, float* dst, ebsdvae_stream_t stream) {
  return ev::ingest("ingest_patterns", 1, src, src_dtype, B, H0, W0, out_h, out_w, dst, stream);
}

extern "C" int ebsdvae_ingest_patterns_u8(const unsigned char* src, int B, int H0, int W0, int out_h,
                                          int out_w, float* dst, ebsdvae_stream_t stream) {
  return ev::ingest("ingest_patterns_u8", 2, src, 2, B, H0, W0, out_h, out_w, dst, stream);
}

