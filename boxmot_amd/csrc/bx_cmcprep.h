// bx_cmcprep.h — the preprocessing rule of the camera-motion stages (include/bxcmc.h, DESIGN.md
// 2.14): BGR -> grey in 14-bit integer weights and the fixed-point bilinear resize to the working
// size.  Shared by the ECC alignment (bx_cmc.hip) and the sparse optical flow (bx_sof.hip), which
// must see the same working image of a frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bx_resize.h"

namespace bx {

struct PrepArgs {
  const uint8_t* frames;
  const int32_t* streams;
  int H, W, ch, h, w;
  int resize;    // 0: working size = frame size
  double scale;
};

__device__ __forceinline__ unsigned grey_at(const uint8_t* f, int W, int ch, int x, int y) {
  const uint8_t* p = f + ((size_t)y * W + x) * ch;
  if (ch == 1) return p[0];
  return (1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14;
}

// (axis_tap and blend_q11, the resize rule itself, live in bx_resize.h: the ReID crops share them)
__device__ __forceinline__ unsigned work_pixel(const PrepArgs& a, const uint8_t* f, int x, int y) {
  if (!a.resize) return grey_at(f, a.W, a.ch, x, y);
  int x0, x1, y0, y1;
  unsigned qx, qy;
  axis_tap(x, a.scale, a.W, x0, x1, qx);
  axis_tap(y, a.scale, a.H, y0, y1, qy);
  const unsigned g00 = grey_at(f, a.W, a.ch, x0, y0), g01 = grey_at(f, a.W, a.ch, x1, y0);
  const unsigned g10 = grey_at(f, a.W, a.ch, x0, y1), g11 = grey_at(f, a.W, a.ch, x1, y1);
  return blend_q11(g00, g01, g10, g11, qx, qy);
}

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  if (i < 0) return -i;
  if (i >= n) return 2 * n - 2 - i;
  return i;
}

}  // namespace bx
