// bx_det.hip — the detector front end (include/bxdet.h): the letterbox into the network's input
// tensor, and the post-process of its output (score filter, batched NMS, rescale).  The contract
// is DESIGN.md 2.27; this file is its device form.  Every launch on the caller's stream; no state.
//
//   det_letterbox_kernel  shaped like reid_crops_kernel (bx_reid.hip): a lane owns a run of 16
//                         bytes of consecutive output x and walks the rows of its tile with it, so
//                         the x taps are computed once per lane, the y tap once per row, and a
//                         workgroup's rows share their source rows through the caches.  The
//                         float64 normalisation is a 3 x 256 table built in LDS by each workgroup:
//                         the kernel proper is a gather through it.
//   det_filter_kernel     a row of pred per lane: class argmax, score, the threshold; the
//                         candidates of a wave are compacted by one ballot and one atomic on the
//                         image's counter.  (Their order in the list is not fixed; the keys are
//                         unique, so the sort's result is.)
//   det_sort_kernel       one workgroup per image: a bitonic sort of the 64-bit keys
//                         (~score bits, row) in LDS, in chunks of 8192 keys with the strides past
//                         a chunk done in global memory; then the boxes and classes of the first
//                         cand_cap candidates in order.
//   det_matrix_kernel     grid (image, row block, column block): one 64-bit word of the
//                         suppression matrix per candidate and column block, a wave64 ballot.
//   det_sweep_kernel      one wave per image, the only sequential part: per block of 64
//                         candidates the diagonal words resolve the block in registers, then the
//                         rows of the kept ones are ORed into the bitset of the later blocks (64
//                         independent loads per lane: one memory round trip per block, not per
//                         candidate).
//   det_write_kernel      one workgroup per image: its offset (the scan of the counts), then rows.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/bxassoc.h"
#include "../../include/bxdet.h"
#include "bx_resize.h"
#include "bx_host.h"

using namespace bx;

namespace {

int de_err(int code, const std::string& msg) { return bx_record_error(code, msg.c_str()); }

typedef unsigned long long u64;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------- letterbox
constexpr int LT = 256;       // threads of a letterbox workgroup
constexpr int ROW_WALK = 4;   // rows a lane walks with one set of x taps
constexpr unsigned PAD = 114;

struct LbArgs {
  const uint8_t* frames;
  void* out;
  int H, W, ih, iw, rh, rw;
  int cols;       // lanes across a row: min(runs per row, LT)
  int rows_par;   // rows a workgroup covers at once: LT / cols
  int tile_rows;  // rows_par * ROW_WALK
  int tiles;      // row tiles per frame
  int swap_rb, no_mean, no_std;
  double mean[3], std[3];
};

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
// and p is aligned, element stores otherwise (an in_w that is no multiple of the run)
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

template <typename OT>
__global__ __launch_bounds__(LT) void det_letterbox_kernel(LbArgs a) {
  constexpr int R = Run<OT>::R;
  __shared__ float lut[3][256];  // the normalised value of v on output channel c
  for (int e = threadIdx.x; e < 768; e += LT) {
    const int c = e >> 8;
    double u = (double)(e & 255) / 255.0;
    if (!a.no_mean) u = u - a.mean[c];
    if (!a.no_std) u = u / a.std[c];
    lut[c][e & 255] = (float)u;
  }
  __syncthreads();
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int col = threadIdx.x % a.cols, rl = threadIdx.x / a.cols;
  if (rl >= a.rows_par) return;
  const int nrun = (a.iw + R - 1) / R;
  const int row_end = min(a.ih, (tile + 1) * a.tile_rows);
  const uint8_t* fr = a.frames + (size_t)f * a.H * a.W * 3;
  int sc[3];
  OT pad[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    sc[c] = a.swap_rb ? 2 - c : c;
    pad[c] = (OT)lut[c][PAD];
  }
  OT* out = (OT*)a.out;

  for (int run = col; run < nrun; run += a.cols) {
    const int xs = run * R, cnt = min(R, a.iw - xs);
    int t0[R], t1[R];  // byte offsets of the two x taps in a source row
    unsigned tq[R];
    if (xs < a.rw) {
#pragma unroll
      for (int k = 0; k < R; k++) {  // (past the resized width: its last pixel again, not used)
        int s0, s1;
        axis_tap_ratio(min(xs + k, a.rw - 1), a.W, a.rw, s0, s1, tq[k]);
        t0[k] = s0 * 3;
        t1[k] = s1 * 3;
      }
    }
    for (int y = tile * a.tile_rows + rl; y < row_end; y += a.rows_par) {
      OT v[3][R];
#pragma unroll
      for (int k = 0; k < R; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) v[c][k] = pad[c];
      if (y < a.rh && xs < a.rw) {
        int y0, y1;
        unsigned qy;
        axis_tap_ratio(y, a.H, a.rh, y0, y1, qy);
        const uint8_t* r0 = fr + (size_t)y0 * a.W * 3;
        const uint8_t* r1 = fr + (size_t)y1 * a.W * 3;
#pragma unroll
        for (int k = 0; k < R; k++) {
          if (xs + k < a.rw) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
              const unsigned g = blend_q11(r0[t0[k] + sc[c]], r0[t1[k] + sc[c]],
                                           r1[t0[k] + sc[c]], r1[t1[k] + sc[c]], tq[k], qy);
              v[c][k] = (OT)lut[c][g];
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; c++)
        store_run<OT>(out + (((size_t)f * 3 + c) * a.ih + y) * a.iw + xs, v[c], cnt);
    }
  }
}

// ----------------------------------------------------------------------------- post-process
constexpr int FT = 256;        // threads of a filter workgroup
constexpr int ST = 1024;       // threads of a sort workgroup
constexpr int SORT_L = 8192;   // keys of an LDS chunk (64 KiB)
constexpr int MT = 256;        // threads of a matrix workgroup: 4 waves, 16 rows each
constexpr int WT = 256;        // threads of a write workgroup

// the scratch of a call, every part 256-byte aligned
struct Lay {
  size_t ints, keys, skeys, cbox, ccls, keep, mask, total;
  int KS;    // keys per image in `keys`: A rounded up to a power of two
  int capb;  // 64-candidate blocks at cand_cap
};

Lay layout(int B, int A, int cap) {
  Lay l{};
  l.KS = 1;
  while (l.KS < A) l.KS <<= 1;
  l.capb = (cap + 63) / 64;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) & ~(size_t)255;
    return at;
  };
  l.ints = take(sizeof(int) * 4 * (size_t)B);  // candidates, sorted candidates, kept, code
  l.keys = take(sizeof(u64) * (size_t)B * l.KS);
  l.skeys = take(sizeof(u64) * (size_t)B * cap);
  l.cbox = take(sizeof(float) * 4 * (size_t)B * cap);
  l.ccls = take(sizeof(int) * (size_t)B * cap);
  l.keep = take(sizeof(int) * (size_t)B * cap);
  // (rows rounded up to whole blocks: the sweep loads all 64 rows of a block)
  l.mask = take(sizeof(u64) * (size_t)B * l.capb * 64 * l.capb);
  l.total = o;
  return l;
}

struct DetArgs {
  const void* pred;
  int B, A, C;
  long long row_stride, img_stride;
  float conf, thr;
  const int32_t* class_ok;
  const float* ratio;
  int cap, capb, KS, max_det, agnostic;
  int *ncand, *nsort, *nkeep, *flags;  // [B] each
  u64* keys;     // [B][KS]
  u64* skeys;    // [B][cap]
  float4* cbox;  // [B][cap]
  int* ccls;     // [B][cap]
  int* keep;     // [B][cap]
  u64* mask;     // [B][capb * 64][capb]
  float* dets;
  int32_t *det_off, *anchor_of, *frame_of, *code;
};

// class and score of one row: the first maximum (a NaN counts as one), obj times it
template <typename PT>
__device__ __forceinline__ float row_score(const PT* p, int C, int& cls) {
  float best = (float)p[5];
  int k = 0;
  for (int c = 1; c < C; c++) {
    const float v = (float)p[5 + c];
    if (v > best || (v != v && best == best)) {
      best = v;
      k = c;
    }
  }
  cls = k;
  return (float)p[4] * best;
}

template <typename PT>
__global__ __launch_bounds__(FT) void det_filter_kernel(DetArgs a, int nblk) {
  const int img = blockIdx.x / nblk, row = (blockIdx.x % nblk) * FT + threadIdx.x;
  bool cand = false;
  u64 key = 0;
  if (row < a.A) {
    const PT* p = (const PT*)a.pred + (size_t)img * a.img_stride + (size_t)row * a.row_stride;
    int cls;
    const float score = row_score(p, a.C, cls);
    cand = score >= a.conf;
    key = ((u64)(~__float_as_uint(score + 0.0f)) << 32) | (unsigned)row;
  }
  const u64 bal = __ballot(cand);
  if (bal == 0) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(a.ncand + img, __popcll(bal));
  base = __shfl(base, 0);
  // (at most A candidates per image, so base + rank < A <= KS)
  if (cand) a.keys[(size_t)img * a.KS + base + __popcll(bal & ((1ull << lane) - 1))] = key;
}

// one compare-exchange pass of stride j inside an LDS chunk of n keys that starts at global
// index base; k is the length of the bitonic runs being merged
__device__ __forceinline__ void lds_pass(u64* s, int n, int base, int k, int j) {
  for (int t = threadIdx.x; t < (n >> 1); t += ST) {
    const int i = 2 * t - (t & (j - 1)), p = i + j;
    const bool up = ((base + i) & k) == 0;
    const u64 x = s[i], y = s[p];
    if ((x > y) == up) {
      s[i] = y;
      s[p] = x;
    }
  }
  __syncthreads();
}

template <typename PT>
__global__ __launch_bounds__(ST) void det_sort_kernel(DetArgs a) {
  __shared__ u64 s[SORT_L];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int n = min(a.ncand[img], a.A);
  const int m = min(n, a.cap);
  if (tid == 0) {
    a.nsort[img] = m;
    a.flags[img] = n > a.cap ? BX_DET_CAND_OVERFLOW : 0;
  }
  if (n == 0) return;
  int P = 1;
  while (P < n) P <<= 1;  // (<= KS)
  u64* g = a.keys + (size_t)img * a.KS;
  const int Lc = min(P, SORT_L), nchunk = P / Lc;
  if (nchunk > 1) {  // the strides past a chunk run on the global list: pad it
    for (int i = n + tid; i < P; i += ST) g[i] = ~0ull;
    __syncthreads();
  }
  // every chunk sorted, ascending or descending by its place
  for (int c = 0; c < nchunk; c++) {
    const int base = c * Lc;
    for (int i = tid; i < Lc; i += ST) s[i] = base + i < n ? g[base + i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= Lc; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) lds_pass(s, Lc, base, k, j);
    if (nchunk > 1) {
      for (int i = tid; i < Lc; i += ST) g[base + i] = s[i];
      __syncthreads();
    }
  }
  // the merges longer than a chunk
  for (int k = 2 * Lc; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= Lc; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += ST) {
        const int i = 2 * t - (t & (j - 1)), p = i + j;
        const bool up = (i & k) == 0;
        const u64 x = g[i], y = g[p];
        if ((x > y) == up) {
          g[i] = y;
          g[p] = x;
        }
      }
      __syncthreads();
    }
    for (int c = 0; c < nchunk; c++) {
      const int base = c * Lc;
      for (int i = tid; i < Lc; i += ST) s[i] = g[base + i];
      __syncthreads();
      for (int j = Lc >> 1; j > 0; j >>= 1) lds_pass(s, Lc, base, k, j);
      for (int i = tid; i < Lc; i += ST) g[base + i] = s[i];
      __syncthreads();
    }
  }
  // the first m in order, with their boxes and classes
  const u64* src = nchunk > 1 ? g : s;
  for (int i = tid; i < m; i += ST) {
    const u64 key = src[i];
    const PT* p = (const PT*)a.pred + (size_t)img * a.img_stride +
                  (size_t)(unsigned)key * a.row_stride;
    const float cx = (float)p[0], cy = (float)p[1], hw = (float)p[2] / 2.0f,
                hh = (float)p[3] / 2.0f;
    int cls;
    row_score(p, a.C, cls);
    const size_t o = (size_t)img * a.cap + i;
    a.skeys[o] = key;
    a.cbox[o] = make_float4(cx - hw, cy - hh, cx + hw, cy + hh);
    a.ccls[o] = cls;
  }
}

// a: the earlier box, b: the later one (include/bxdet.h)
__device__ __forceinline__ float det_iou(const float4 a, const float4 b) {
  const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
  const float xx2 = b.z < a.z ? b.z : a.z, xx1 = b.x > a.x ? b.x : a.x;
  const float yy2 = b.w < a.w ? b.w : a.w, yy1 = b.y > a.y ? b.y : a.y;
  const float dw = xx2 - xx1, dh = yy2 - yy1;
  const float iw = dw > 0.0f ? dw : 0.0f, ih = dh > 0.0f ? dh : 0.0f;
  const float inter = iw * ih;
  return inter / ((area_a + area_b) - inter);
}

__global__ __launch_bounds__(MT) void det_matrix_kernel(DetArgs a) {
  __shared__ float4 rbox[64];
  __shared__ int rcls[64];
  const int img = blockIdx.x, rb = blockIdx.y, cb = blockIdx.z;
  const int m = a.nsort[img];
  if (cb < rb || cb * 64 >= m) return;  // (rb <= cb: the row block has candidates too)
  const size_t o = (size_t)img * a.cap;
  if (threadIdx.x < 64 && rb * 64 + threadIdx.x < m) {
    rbox[threadIdx.x] = a.cbox[o + rb * 64 + threadIdx.x];
    rcls[threadIdx.x] = a.ccls[o + rb * 64 + threadIdx.x];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, b = cb * 64 + lane;
  const bool valid = b < m;
  float4 bb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int bc = 0;
  if (valid) {
    bb = a.cbox[o + b];
    bc = a.ccls[o + b];
  }
  u64* mrow = a.mask + (size_t)img * a.capb * 64 * a.capb;
  for (int r = threadIdx.x >> 6; r < 64; r += MT / 64) {
    const int i = rb * 64 + r;
    if (i >= m) break;  // (the whole wave)
    const bool hit = valid && b > i && (a.agnostic || bc == rcls[r]) &&
                     det_iou(rbox[r], bb) > a.thr;
    const u64 bal = __ballot(hit);
    if (lane == 0) mrow[(size_t)i * a.capb + cb] = bal;
  }
}

__global__ __launch_bounds__(64) void det_sweep_kernel(DetArgs a) {
  __shared__ u64 removed[BX_DET_CAND_MAX / 64];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int m = a.nsort[img], nb = (m + 63) / 64;
  for (int w = lane; w < nb; w += 64) removed[w] = 0;
  __syncthreads();
  const u64* mrow = a.mask + (size_t)img * a.capb * 64 * a.capb;
  const size_t o = (size_t)img * a.cap;
  int count = 0;  // survivors that pass the class list, so far
  for (int ib = 0; ib < nb; ib++) {
    const int i0 = ib * 64, i = i0 + lane;
    const bool valid = i < m;
    const u64 diag = valid ? mrow[(size_t)i * a.capb + ib] : 0;
    u64 rem = removed[ib];
    if (m - i0 < 64) rem |= ~0ull << (m - i0);
    // the block against itself, in order (every lane computes the same word)
#pragma unroll
    for (int l = 0; l < 64; l++) {
      const u64 d = __shfl(diag, l);
      if (!((rem >> l) & 1)) rem |= d;
    }
    const u64 kept = ~rem;
    // the rows of the kept ones into the later blocks; a row that was not kept is loaded and
    // dropped, so that the 64 loads are independent of the word above and of one another
    for (int w = ib + 1 + lane; w < nb; w += 64) {
      u64 acc = 0;
#pragma unroll 16
      for (int l = 0; l < 64; l++) {
        const u64 v = mrow[(size_t)(i0 + l) * a.capb + w];
        acc |= ((kept >> l) & 1) ? v : 0;
      }
      removed[w] |= acc;
    }
    const bool ok = valid && ((kept >> lane) & 1) &&
                    (!a.class_ok || a.class_ok[a.ccls[o + i]] != 0);
    const u64 okb = __ballot(ok);
    const int rank = count + __popcll(okb & ((1ull << lane) - 1));
    if (ok && rank < a.max_det) a.keep[o + rank] = i;
    count += __popcll(okb);
    if (count > a.max_det) break;  // (one past the limit is all the flag needs)
    __syncthreads();
  }
  if (lane == 0) {
    a.nkeep[img] = min(count, a.max_det);
    if (count > a.max_det) a.flags[img] |= BX_DET_MAX_DET;
  }
}

__global__ __launch_bounds__(WT) void det_write_kernel(DetArgs a) {
  __shared__ int part[WT];
  const int img = blockIdx.x, tid = threadIdx.x;
  int sum = 0;
  for (int j = tid; j < img; j += WT) sum += a.nkeep[j];
  part[tid] = sum;
  __syncthreads();
  for (int h = WT / 2; h > 0; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  const int off = part[0], n = a.nkeep[img];
  if (tid == 0) {
    a.det_off[img] = off;
    if (img == a.B - 1) a.det_off[a.B] = off + n;
    if (a.code) a.code[img] = a.flags[img];
  }
  const float r = a.ratio ? a.ratio[img] : 1.0f;
  const size_t o = (size_t)img * a.cap;
  for (int t = tid; t < n; t += WT) {
    const int ci = a.keep[o + t];
    const float4 bx4 = a.cbox[o + ci];
    const u64 key = a.skeys[o + ci];
    float* d = a.dets + (size_t)(off + t) * 6;
    d[0] = bx4.x / r;
    d[1] = bx4.y / r;
    d[2] = bx4.z / r;
    d[3] = bx4.w / r;
    d[4] = __uint_as_float(~(unsigned)(key >> 32));
    d[5] = (float)a.ccls[o + ci];
    if (a.anchor_of) a.anchor_of[off + t] = (int)(unsigned)key;
    if (a.frame_of) a.frame_of[off + t] = img;
  }
}

}  // namespace

extern "C" {

int bx_det_letterbox(const uint8_t* frames, int F, int H, int W, int in_h, int in_w, int rh,
                     int rw, double mean0, double mean1, double mean2, double std0, double std1,
                     double std2, int flags, void* out, void* hip_stream) {
  if (F < 0 || H < 1 || W < 1 || in_h < 1 || in_w < 1)
    return de_err(BX_ERR_INVALID, "sizes must be at least 1 (F at least 0)");
  if (rh < 1 || rh > in_h || rw < 1 || rw > in_w)
    return de_err(BX_ERR_INVALID, "the resized size must lie in 1..in_h, 1..in_w");
  if (flags & ~(BX_LB_HALF | BX_LB_SWAP_RB | BX_LB_NO_MEAN | BX_LB_NO_STD))
    return de_err(BX_ERR_INVALID, "unknown flag bits");
  const double mean[3] = {mean0, mean1, mean2}, std[3] = {std0, std1, std2};
  for (int c = 0; c < 3; c++) {
    if (!(flags & BX_LB_NO_MEAN) && !std::isfinite(mean[c]))
      return de_err(BX_ERR_INVALID, "mean must be finite");
    if (!(flags & BX_LB_NO_STD) && (!std::isfinite(std[c]) || std[c] == 0.0))
      return de_err(BX_ERR_INVALID, "std must be finite and non-zero");
  }
  if ((long long)H * W * 3 > (1LL << 40)) return de_err(BX_ERR_INVALID, "frame too large");
  if (F == 0) return BX_OK;
  if (!frames || !out) return de_err(BX_ERR_INVALID, "null argument");
  const bool half = flags & BX_LB_HALF;
  const int R = half ? 8 : 4;
  LbArgs a{};
  a.frames = frames;
  a.out = out;
  a.H = H; a.W = W; a.ih = in_h; a.iw = in_w; a.rh = rh; a.rw = rw;
  const int nrun = (in_w + R - 1) / R;
  a.cols = nrun < LT ? nrun : LT;
  a.rows_par = LT / a.cols;
  a.tile_rows = a.rows_par * ROW_WALK;
  a.tiles = (in_h + a.tile_rows - 1) / a.tile_rows;
  a.swap_rb = (flags & BX_LB_SWAP_RB) ? 1 : 0;
  a.no_mean = (flags & BX_LB_NO_MEAN) ? 1 : 0;
  a.no_std = (flags & BX_LB_NO_STD) ? 1 : 0;
  for (int c = 0; c < 3; c++) {
    a.mean[c] = mean[c];
    a.std[c] = std[c];
  }
  const long long blocks = (long long)F * a.tiles;
  if (blocks > 0x7fffffffLL) return de_err(BX_ERR_INVALID, "too many frames for one launch");
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)blocks), block(LT);
  if (half) det_letterbox_kernel<_Float16><<<grid, block, 0, st>>>(a);
  else det_letterbox_kernel<float><<<grid, block, 0, st>>>(a);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

static int det_sizes_ok(int B, int A, int cand_cap) {
  if (B < 0 || A < 0 || A > (1 << 24)) return de_err(BX_ERR_INVALID, "bad B / A");
  if (cand_cap < 1 || cand_cap > BX_DET_CAND_MAX)
    return de_err(BX_ERR_INVALID, "cand_cap must lie in 1..BX_DET_CAND_MAX");
  return BX_OK;
}

int bx_det_scratch_bytes(int B, int A, int cand_cap, size_t* bytes) {
  if (!bytes) return de_err(BX_ERR_INVALID, "null argument");
  if (int rc = det_sizes_ok(B, A, cand_cap)) return rc;
  *bytes = layout(B, A, cand_cap).total;
  return BX_OK;
}

int bx_det_postprocess(const void* pred, int B, int A, int C, int64_t row_stride,
                       int64_t img_stride, float conf_thre, float nms_thre,
                       const int32_t* class_ok, const float* ratio, int cand_cap, int max_det,
                       int flags, void* scratch, float* dets, int32_t* det_off,
                       int32_t* anchor_of, int32_t* frame_of, int32_t* code, void* hip_stream) {
  if (int rc = det_sizes_ok(B, A, cand_cap)) return rc;
  if (C < 1 || C > (1 << 20)) return de_err(BX_ERR_INVALID, "C must be at least 1");
  if (row_stride < 5 + C || (A > 1 && img_stride < (int64_t)(A - 1) * row_stride + 5 + C))
    return de_err(BX_ERR_INVALID, "a stride of pred is too small");
  if (max_det < 1 || (long long)B * max_det > 0x7fffffffLL)
    return de_err(BX_ERR_INVALID, "max_det must be at least 1 and B * max_det below 2^31");
  if (!(conf_thre >= 0.0f && conf_thre <= 1.0f) || !(nms_thre >= 0.0f && nms_thre <= 1.0f))
    return de_err(BX_ERR_INVALID, "thresholds must lie in [0, 1]");
  if (flags & ~(BX_DET_PRED_HALF | BX_DET_AGNOSTIC))
    return de_err(BX_ERR_INVALID, "unknown flag bits");
  if (B == 0) return BX_OK;
  if ((A > 0 && !pred) || !scratch || !dets || !det_off)
    return de_err(BX_ERR_INVALID, "null argument");
  if ((uintptr_t)scratch & 255) return de_err(BX_ERR_INVALID, "scratch must be 256-byte aligned");
  const int nblk = (A + FT - 1) / FT;
  if ((long long)B * nblk > 0x7fffffffLL)
    return de_err(BX_ERR_INVALID, "too many rows for one launch");
  const Lay l = layout(B, A, cand_cap);
  char* s = (char*)scratch;
  DetArgs a{};
  a.pred = pred;
  a.B = B; a.A = A; a.C = C;
  a.row_stride = row_stride;
  a.img_stride = img_stride;
  a.conf = conf_thre;
  a.thr = nms_thre;
  a.class_ok = class_ok;
  a.ratio = ratio;
  a.cap = cand_cap; a.capb = l.capb; a.KS = l.KS; a.max_det = max_det;
  a.agnostic = (flags & BX_DET_AGNOSTIC) ? 1 : 0;
  a.ncand = (int*)(s + l.ints);
  a.nsort = a.ncand + B;
  a.nkeep = a.nsort + B;
  a.flags = a.nkeep + B;
  a.keys = (u64*)(s + l.keys);
  a.skeys = (u64*)(s + l.skeys);
  a.cbox = (float4*)(s + l.cbox);
  a.ccls = (int*)(s + l.ccls);
  a.keep = (int*)(s + l.keep);
  a.mask = (u64*)(s + l.mask);
  a.dets = dets;
  a.det_off = det_off;
  a.anchor_of = anchor_of;
  a.frame_of = frame_of;
  a.code = code;
  hipStream_t st = (hipStream_t)hip_stream;
  const bool half = flags & BX_DET_PRED_HALF;
  BX_HIPCHK(hipMemsetAsync(a.ncand, 0, sizeof(int) * B, st));
  if (A > 0) {
    const dim3 grid((unsigned)((long long)B * nblk));
    if (half) det_filter_kernel<_Float16><<<grid, dim3(FT), 0, st>>>(a, nblk);
    else det_filter_kernel<float><<<grid, dim3(FT), 0, st>>>(a, nblk);
  }
  if (half) det_sort_kernel<_Float16><<<dim3(B), dim3(ST), 0, st>>>(a);
  else det_sort_kernel<float><<<dim3(B), dim3(ST), 0, st>>>(a);
  det_matrix_kernel<<<dim3(B, l.capb, l.capb), dim3(MT), 0, st>>>(a);
  det_sweep_kernel<<<dim3(B), dim3(64), 0, st>>>(a);
  det_write_kernel<<<dim3(B), dim3(WT), 0, st>>>(a);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

}  // extern "C"
