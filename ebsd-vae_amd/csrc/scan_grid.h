// What the kernels that walk a scan's (rows, cols) grid of orientations share (scan_maps.hip,
// grains.hip): the cubic operators as unit quaternions, the finiteness of an Euler row and the
// neighbour offsets of a connectivity.
#pragma once
#include "orient_math.h"

#include <math.h>

namespace ev {

EV_DEVINL Q4 cubic_op(int c) {
  return qnormalize(Q4{kCubic[c][0], kCubic[c][1], kCubic[c][2], kCubic[c][3]});
}

EV_DEVINL bool finite3(double a, double b, double c) {
  return isfinite(a) && isfinite(b) && isfinite(c);
}

// the (a, b) offsets of a connectivity, row-major: 4 = the cross, 8 = the square
EV_DEVINL bool map_offset(int connectivity, int a, int b) {
  return (a != 0 || b != 0) && (connectivity == 8 || a == 0 || b == 0);
}

}  // namespace ev
