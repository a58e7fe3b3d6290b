// Centre-crop geometry shared by the ingest kernels (ingest.hip, correct.hip).
#pragma once

namespace ev {

// torchvision center_crop source offset along one axis (negative = leading zero padding)
inline int crop_offset(int size, int crop) {
  if (crop > size) return -((crop - size) / 2);
  const int d = size - crop;             // round(d / 2.0), ties to even
  const int h = d / 2;
  if ((d & 1) == 0) return h;
  return (h & 1) == 0 ? h : h + 1;
}

}  // namespace ev
