// bx_resize.h — the fixed-point bilinear resize rule of DESIGN.md 2.14, shared by the ECC
// preprocessing (bx_cmc.hip) and the ReID crops (bx_reid.hip): per axis a source index pair and an
// 11-bit weight, then one integer blend with a single rounding.  Exact integer arithmetic after
// the float64 source coordinate; agreement with OpenCV's INTER_LINEAR is unmeasured.
#pragma once
#include <hip/hip_runtime.h>

namespace bx {

// source index pair and 11-bit weight of the float64 source coordinate f on an axis of source
// length L: s0 = floor(f), a = f - s0; left of the axis s0 = 0, a = 0; at or past its last pixel
// s0 = L - 1, a = 0; s1 = min(s0 + 1, L - 1); q = round_half_even(a * 2048)
__device__ __forceinline__ void axis_tap_at(double f, int L, int& s0, int& s1, unsigned& q) {
  const double fl = floor(f);
  double a = f - fl;
  if (fl < 0.0) {
    s0 = 0;
    a = 0.0;
  } else if (fl >= (double)(L - 1)) {
    s0 = L - 1;
    a = 0.0;
  } else {
    s0 = (int)fl;
  }
  s1 = min(s0 + 1, L - 1);
  q = (unsigned)rint(a * 2048.0);
}

// output index d of an axis resized by one ratio for both axes (ECC: f = (d + 0.5) / scale - 0.5)
__device__ __forceinline__ void axis_tap(int d, double scale, int L, int& s0, int& s1,
                                         unsigned& q) {
  axis_tap_at(((double)d + 0.5) / scale - 0.5, L, s0, s1, q);
}

// output index d of an axis of source length L resized to O outputs (crops: a ratio per axis,
// f = (d + 0.5) * L / O - 0.5, evaluated left to right)
__device__ __forceinline__ void axis_tap_ratio(int d, int L, int O, int& s0, int& s1,
                                               unsigned& q) {
  axis_tap_at(((double)d + 0.5) * (double)L / (double)O - 0.5, L, s0, s1, q);
}

// the blend of the four taps (g01: x1, g10: y1), values 0..255: fits 32 bits, one rounding
__device__ __forceinline__ unsigned blend_q11(unsigned g00, unsigned g01, unsigned g10,
                                              unsigned g11, unsigned qx, unsigned qy) {
  const unsigned px = 2048u - qx, py = 2048u - qy;
  return (g00 * px * py + g01 * qx * py + g10 * px * qy + g11 * qx * qy + (1u << 21)) >> 22;
}

}  // namespace bx
