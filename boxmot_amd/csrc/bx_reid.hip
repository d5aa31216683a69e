// bx_reid.hip — the ReID front end (include/bxreid.h): batched crops into the network's input
// tensor, and the unit rows of its output.  The contract is DESIGN.md 2.15; this file is its
// device form.  One launch each, on the caller's stream; no state.
//
//   reid_crops_kernel      a float32 256x128 crop is 393 KB out, its source window a few KB that
//                          the caches serve, so the kernel is shaped around its stores (what the
//                          counters show it waiting on instead is in DESIGN.md 2.15): a lane owns a run of 16 bytes of consecutive output x (4
//                          floats / 8 halves) and walks the rows of its tile with it, so the x
//                          taps (a float64 coordinate each) are computed once per lane and the y
//                          tap once per row; each plane's run goes out as one 16-byte store.  The
//                          grid is (box, row tile): one box alone still spreads over the chip.
//   reid_normalize_kernel  one wave per row: numpy's float32 pairwise sum of squares
//                          (bx_device.h), sqrtf, one correctly rounded division per element.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/bxassoc.h"
#include "../../include/bxreid.h"
#include "bx_device.h"
#include "bx_resize.h"
#include "bx_host.h"


using namespace bx;

namespace {

int re_err(int code, const std::string& msg) { return bx_record_error(code, msg.c_str()); }
constexpr int CT = 256;       // threads of a crop workgroup
constexpr int ROW_WALK = 4;   // rows a lane walks with one set of x taps (a tile's depth)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct CropArgs {
  const uint8_t* frames;
  const float* boxes;
  const int32_t* frame_of;
  void* out;
  int32_t* code;
  int F, H, W, oh, ow;
  int cols;       // lanes across a row: min(runs per row, CT)
  int rows_par;   // rows a workgroup covers at once: CT / cols
  int tile_rows;  // rows_par * ROW_WALK
  int tiles;      // row tiles per box
  int swap_rb;
  float mean[3], std[3];
};

// one corner coordinate: half-even rounding in float32, clamped in floating point to [0, hi]
__device__ __forceinline__ int crop_corner(float v, int hi) {
  return (int)fminf(fmaxf(rintf(v), 0.0f), (float)hi);
}

template <typename OT>
struct Run;
template <>
struct Run<float> {
  static constexpr int R = 4;
  typedef f32x4 vec;
};
template <>
struct Run<_Float16> {
  static constexpr int R = 8;
  typedef f16x8 vec;
};

// `cnt` (1..16 bytes' worth) consecutive elements to p: one 16-byte store when the run is whole
// and p is aligned (always, for a contiguous output whose out_w is a multiple of the run), element
// stores otherwise
template <typename OT>
__device__ __forceinline__ void store_run(OT* p, const OT* v, int cnt) {
  constexpr int R = Run<OT>::R;
  if (cnt == R && ((uintptr_t)p & 15) == 0) {
    typename Run<OT>::vec w;
#pragma unroll
    for (int k = 0; k < R; k++) w[k] = v[k];
    *reinterpret_cast<typename Run<OT>::vec*>(p) = w;
  } else {
    for (int k = 0; k < cnt; k++) p[k] = v[k];
  }
}

template <typename OT, bool NHWC>
__global__ __launch_bounds__(CT) void reid_crops_kernel(CropArgs a) {
  constexpr int R = Run<OT>::R;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  // the box: the same for the whole workgroup
  const float* bp = a.boxes + (size_t)b * 4;
  const float bx1 = bp[0], by1 = bp[1], bx2 = bp[2], by2 = bp[3];
  const int fr = a.frame_of ? a.frame_of[b] : 0;
  bool ok = isfinite(bx1) && isfinite(by1) && isfinite(bx2) && isfinite(by2) && fr >= 0 &&
            fr < a.F;
  int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
  if (ok) {
    x1 = crop_corner(bx1, a.W);
    y1 = crop_corner(by1, a.H);
    x2 = crop_corner(bx2, a.W);
    y2 = crop_corner(by2, a.H);
    ok = x2 > x1 && y2 > y1;
  }
  if (tile == 0 && threadIdx.x == 0 && a.code) a.code[b] = ok ? BX_CROP_OK : BX_CROP_EMPTY;

  const int col = threadIdx.x % a.cols, rl = threadIdx.x / a.cols;
  if (rl >= a.rows_par) return;
  const int Lx = x2 - x1, Ly = y2 - y1;
  const int nrun = (a.ow + R - 1) / R;
  const int row_end = min(a.oh, (tile + 1) * a.tile_rows);
  // (every source index below is x1 + s with 0 <= s < Lx, so < x2 <= W; likewise in y)
  const uint8_t* f = a.frames + ((size_t)(ok ? fr : 0) * a.H + y1) * ((size_t)a.W * 3) +
                     (size_t)x1 * 3;
  const Div32 by255(255.0f);
  Div32 bystd[3];
  float mean[3];
  int sc[3];  // source channel of output channel c
#pragma unroll
  for (int c = 0; c < 3; c++) {
    bystd[c] = Div32(a.std[c]);
    mean[c] = a.mean[c];
    sc[c] = a.swap_rb ? 2 - c : c;
  }
  OT* out = (OT*)a.out;

  for (int run = col; run < nrun; run += a.cols) {
    const int xs = run * R, cnt = min(R, a.ow - xs);
    int t0[R], t1[R];  // byte offsets of the two x taps in a source row
    unsigned tq[R];
    if (ok) {
#pragma unroll
      for (int k = 0; k < R; k++) {  // (past the row's end: the last pixel again, not stored)
        int s0, s1;
        axis_tap_ratio(min(xs + k, a.ow - 1), Lx, a.ow, s0, s1, tq[k]);
        t0[k] = s0 * 3;
        t1[k] = s1 * 3;
      }
    }
    for (int y = tile * a.tile_rows + rl; y < row_end; y += a.rows_par) {
      OT v[3][R];
      if (ok) {
        int y0, yy1;
        unsigned qy;
        axis_tap_ratio(y, Ly, a.oh, y0, yy1, qy);
        const uint8_t* r0 = f + (size_t)y0 * a.W * 3;
        const uint8_t* r1 = f + (size_t)yy1 * a.W * 3;
#pragma unroll
        for (int k = 0; k < R; k++) {
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const unsigned g = blend_q11(r0[t0[k] + sc[c]], r0[t1[k] + sc[c]], r1[t0[k] + sc[c]],
                                         r1[t1[k] + sc[c]], tq[k], qy);
            float u = by255((float)g);
            if constexpr (sizeof(OT) == 2) u = (float)(_Float16)u;
            v[c][k] = (OT)bystd[c](u - mean[c]);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < R; k++) v[0][k] = v[1][k] = v[2][k] = (OT)0.0f;
      }
      if constexpr (NHWC) {
        OT w[3 * R];
#pragma unroll
        for (int k = 0; k < R; k++)
#pragma unroll
          for (int c = 0; c < 3; c++) w[3 * k + c] = v[c][k];
        OT* p = out + (((size_t)b * a.oh + y) * a.ow + xs) * 3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const int left = 3 * cnt - j * R;
          if (left > 0) store_run<OT>(p + j * R, w + j * R, min(R, left));
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; c++)
          store_run<OT>(out + (((size_t)b * 3 + c) * a.oh + y) * a.ow + xs, v[c], cnt);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
constexpr int NT = 256;  // 4 rows per workgroup

template <typename XT, typename OT>
__global__ __launch_bounds__(NT) void reid_normalize_kernel(const XT* in, int64_t stride, int n,
                                                            int F, OT* out) {
  const int row = blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6);
  if (row >= n) return;  // (whole waves: no barrier follows)
  const XT* x = in + (size_t)row * stride;
  const float nrm = sqrtf(np_sumsq_wave(x, F));
  const Div32 by(nrm);
  OT* o = out + (size_t)row * F;
  for (int k = threadIdx.x & 63; k < F; k += WAVE) o[k] = (OT)by((float)x[k]);
}

}  // namespace

extern "C" {

int bx_reid_crops(const uint8_t* frames, int F, int H, int W, const float* boxes,
                  const int32_t* frame_of, int n, int out_h, int out_w, float mean0, float mean1,
                  float mean2, float std0, float std1, float std2, int flags, void* out,
                  int32_t* code, void* hip_stream) {
  if (F < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1 || n < 0)
    return re_err(BX_ERR_INVALID, "sizes must be at least 1 (n at least 0)");
  if (flags & ~(BX_CROP_HALF | BX_CROP_NHWC | BX_CROP_SWAP_RB))
    return re_err(BX_ERR_INVALID, "unknown flag bits");
  const float mean[3] = {mean0, mean1, mean2}, std[3] = {std0, std1, std2};
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f)
      return re_err(BX_ERR_INVALID, "mean / std must be finite and std non-zero");
  // (corners are clamped in float32: H and W must be exact there)
  if (H > (1 << 24) || W > (1 << 24) || (long long)H * W * 3 > (1LL << 40))
    return re_err(BX_ERR_INVALID, "frame too large");
  if (n == 0) return BX_OK;
  if (!frames || !boxes || !out) return re_err(BX_ERR_INVALID, "null argument");
  const bool half = flags & BX_CROP_HALF, nhwc = flags & BX_CROP_NHWC;
  const int R = half ? 8 : 4;
  CropArgs a{};
  a.frames = frames;
  a.boxes = boxes;
  a.frame_of = frame_of;
  a.out = out;
  a.code = code;
  a.F = F; a.H = H; a.W = W; a.oh = out_h; a.ow = out_w;
  const int nrun = (out_w + R - 1) / R;
  a.cols = nrun < CT ? nrun : CT;
  a.rows_par = CT / a.cols;
  a.tile_rows = a.rows_par * ROW_WALK;
  a.tiles = (out_h + a.tile_rows - 1) / a.tile_rows;
  a.swap_rb = (flags & BX_CROP_SWAP_RB) ? 1 : 0;
  for (int c = 0; c < 3; c++) {
    a.mean[c] = mean[c];
    a.std[c] = std[c];
  }
  const long long blocks = (long long)n * a.tiles;
  if (blocks > 0x7fffffffLL) return re_err(BX_ERR_INVALID, "too many crops for one launch");
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)blocks), block(CT);
  if (half && nhwc) reid_crops_kernel<_Float16, true><<<grid, block, 0, st>>>(a);
  else if (half) reid_crops_kernel<_Float16, false><<<grid, block, 0, st>>>(a);
  else if (nhwc) reid_crops_kernel<float, true><<<grid, block, 0, st>>>(a);
  else reid_crops_kernel<float, false><<<grid, block, 0, st>>>(a);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_reid_normalize(const void* in, int in_half, int64_t in_stride, int n, int F, void* out,
                      int out_f64, void* hip_stream) {
  if (F < 1 || n < 0 || in_stride < F) return re_err(BX_ERR_INVALID, "bad n / F / in_stride");
  if (n == 0) return BX_OK;
  if (!in || !out) return re_err(BX_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((n + NT / WAVE - 1) / (NT / WAVE))), block(NT);
  if (in_half && out_f64)
    reid_normalize_kernel<<<grid, block, 0, st>>>((const _Float16*)in, in_stride, n, F, (double*)out);
  else if (in_half)
    reid_normalize_kernel<<<grid, block, 0, st>>>((const _Float16*)in, in_stride, n, F, (float*)out);
  else if (out_f64)
    reid_normalize_kernel<<<grid, block, 0, st>>>((const float*)in, in_stride, n, F, (double*)out);
  else
    reid_normalize_kernel<<<grid, block, 0, st>>>((const float*)in, in_stride, n, F, (float*)out);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

}  // extern "C"
