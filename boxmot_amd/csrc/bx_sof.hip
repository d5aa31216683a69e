// bx_sof.hip — sparse-optical-flow camera-motion compensation (include/bxsof.h): Shi-Tomasi
// keypoints of the previous frame tracked into the new one by pyramidal Lucas-Kanade, and a
// similarity fitted to the tracked pairs by a deterministic consensus, the stage motion/cmc/sof.py
// hands to OpenCV.  The contract is DESIGN.md 2.17; this file is its device form.
//
// Launches per step, all on the caller's stream (nl: pyramid levels, 1..4):
//   sof_prep_kernel    one thread per working pixel: grey + resize (bx_cmcprep.h, ECC's rule) into
//                      level 0 of the stream's new pyramid
//   sof_pyr_kernel     (nl - 1 launches) one thread per pixel of level l: the 5x5 binomial of
//                      level l - 1 at even pixels, integer
//   sof_track_kernel   one wave per keypoint: every level and every iteration inside; the window
//                      is strided over the lanes, the template patch and its derivatives stay in
//                      the wave's LDS slab across a level's iterations, sums through the
//                      fixed-order butterfly of bx_device.h
//   sof_fit_kernel     one workgroup per stream: tracked pairs compacted into LDS, waves take
//                      hypotheses, lanes take points, argmax on (count, -k), wave 0 makes the
//                      final least-squares sums
//   sof_resp_kernel    one thread per working pixel: the minimum eigenvalue, and its maximum by
//                      an integer atomic max on the bit pattern (exact: the values are >= 0)
//   sof_select_kernel  one workgroup per stream: candidates compacted in pixel order, the
//                      max_corners-th largest lambda found by a radix pass over its bits, the
//                      survivors ranked in LDS; then the stream's state is switched
// No device-wide barrier, no host round trip.
//
// The chained apply runs n consecutive frames per call from the same __device__
// bodies, each frame in a slot of its own; its launches are listed above sof_chain_prep_kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/bxassoc.h"
#include "../../include/bxcmc.h"
#include "../../include/bxsof.h"
#include "bx_device.h"
#include "bx_cmcprep.h"
#include "bx_host.h"

using namespace bx;

namespace {

int sf_err(int code, const std::string& msg) { return bx_record_error(code, msg.c_str()); }
constexpr int MAXC = BX_SOF_MAX_CORNERS, MAXL = BX_SOF_MAX_LEVELS, NHYP = BX_SOF_HYPOTHESES;
constexpr int PT = 256;            // threads of a per-pixel workgroup
constexpr int ST = 1024, SW = 16;  // threads / waves of the selection workgroup
constexpr int TW = 2;              // waves (keypoints) of a tracking workgroup
constexpr int FT = 256, FW = 4;    // threads / waves of the fit workgroup (block_compact's WG)
static_assert(FT == WG, "the fit kernel uses bx_device.h's block_compact");

// the levels of a call: sizes and offsets into a pyramid buffer
struct Lv {
  int nl;
  int h[MAXL], w[MAXL], off[MAXL];
};

// Everything the kernels read or write.
struct SofDev {
  int n_streams, cap, pcap;  // cap = max_h * max_w; pcap: bytes of one pyramid buffer
  uint8_t* pyr;              // [n_streams][2][pcap] the two pyramids, swapped by par[]
  double* lam;               // [n_streams][cap] minimum eigenvalue of the new level 0
  unsigned long long* lmax;  // [n_streams] bits of its maximum
  unsigned long long* ckey;  // [n_streams][cap] candidates in pixel order: lambda's bits
  int* cidx;                 // [n_streams][cap] and pixel index
  double* kp;                // [n_streams][MAXC][2] keypoints
  double *rprev, *rnext;     // [n_streams][MAXC][2] the last tracking record
  int* riter;                // [n_streams][MAXC]
  uint8_t *rok, *rinl;       // [n_streams][MAXC]
  int *has_prev, *ph, *pw, *pnl, *par, *nkp, *rn, *rwin;  // [n_streams]
  int* status;               // latched BX_ERR_*
};

// Scratch of the chained apply (bx_sof_chain_reserve): one slot per frame of a call, each what a
// stream holds for one frame; nothing is carried from one call to the next.
struct SofChain {
  int max_frames;
  uint8_t* pyr;                    // [max_frames][pcap]
  double* lam;                     // [max_frames][cap]
  unsigned long long *lmax, *ckey;  // [max_frames], [max_frames][cap]
  int* cidx;                       // [max_frames][cap]
  double *kp, *rprev, *rnext;      // [max_frames][MAXC][2]
  int* riter;                      // [max_frames][MAXC]
  uint8_t *rok, *rinl;             // [max_frames][MAXC]
  int *nkp, *rn, *rwin;            // [max_frames]
  int *plan, *topar;               // [max_frames] PL_* of a frame; a group's final par[]
};

struct SofHandle {
  SofDev d{};
  SofChain c{};
  int max_h = 0, max_w = 0;
  uint8_t* sframes = nullptr;
  size_t sframes_bytes = 0;
  int32_t* sstreams = nullptr;
  double* swarps = nullptr;
  int32_t* sints = nullptr;  // [4][n_streams]: code, n_keypoints, n_tracked, n_inliers
  // staging of the chained host entry, grown with the slots
  int32_t* cstreams = nullptr;  // [max_frames]
  double* cwarps = nullptr;     // [max_frames][6]
  int32_t* cints = nullptr;     // [4][max_frames]
};

// a tracking record: the arrays of one stream or of one slot
struct Rec {
  double *prev, *next;
  int* iter;
  uint8_t *ok, *inl;
};
__device__ __forceinline__ Rec rec_of(const SofDev& d, int s) {
  const size_t o = (size_t)s * BX_SOF_MAX_CORNERS;
  return Rec{d.rprev + 2 * o, d.rnext + 2 * o, d.riter + o, d.rok + o, d.rinl + o};
}
__device__ __forceinline__ Rec rec_of(const SofChain& c, int i) {
  const size_t o = (size_t)i * BX_SOF_MAX_CORNERS;
  return Rec{c.rprev + 2 * o, c.rnext + 2 * o, c.riter + o, c.rok + o, c.rinl + o};
}

__device__ __forceinline__ bool bad_stream(const SofDev& d, int s) {
  return s < 0 || s >= d.n_streams;
}
// the stream starts over: no previous frame, or one of another shape
__device__ __forceinline__ bool is_first(const SofDev& d, int s, int h, int w, int nl) {
  return !d.has_prev[s] || d.ph[s] != h || d.pw[s] != w || d.pnl[s] != nl;
}
__device__ __forceinline__ bool is_first(const SofDev& d, int s, const Lv& lv) {
  return is_first(d, s, lv.h[0], lv.w[0], lv.nl);
}
__device__ __forceinline__ uint8_t* pyr_of(const SofDev& d, int s, int which) {
  return d.pyr + ((size_t)s * 2 + which) * d.pcap;
}
// reflect-101 for any reach (period 2n - 2)
__device__ __forceinline__ int refl(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// ------------------------------------------------------------------------------------------
// level 0
__global__ __launch_bounds__(PT) void sof_prep_kernel(SofDev d, PrepArgs a) {
  const int k = blockIdx.y;
  const int s = a.streams[k];
  if (bad_stream(d, s)) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicMax(d.status, (int)BX_ERR_INVALID);
    return;
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) d.lmax[s] = 0ull;  // (read two launches later)
  const int idx = blockIdx.x * PT + threadIdx.x;
  if (idx >= a.h * a.w) return;
  const int x = idx % a.w, y = idx / a.w;
  const uint8_t* f = a.frames + (size_t)k * a.H * a.W * a.ch;
  pyr_of(d, s, d.par[s] ^ 1)[idx] = (uint8_t)work_pixel(a, f, x, y);
}

// level l from level l - 1
struct PyrArgs {
  const int32_t* streams;
  Lv lv;
  int l;
};
// pixel idx of level l of the pyramid at base
__device__ __forceinline__ void pyr_pixel(uint8_t* base, const PyrArgs& a, int idx) {
  const int l = a.l, w = a.lv.w[l], h = a.lv.h[l], sw = a.lv.w[l - 1], sh = a.lv.h[l - 1];
  if (idx >= h * w) return;
  const int x = idx % w, y = idx / w;
  const uint8_t* src = base + a.lv.off[l - 1];
  const int kq[5] = {1, 4, 6, 4, 1};
  int xs[5];
#pragma unroll
  for (int j = 0; j < 5; j++) xs[j] = refl(2 * x + j - 2, sw);
  int sum = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint8_t* row = src + (size_t)refl(2 * y + i - 2, sh) * sw;
    int r = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) r += kq[j] * (int)row[xs[j]];
    sum += kq[i] * r;
  }
  base[a.lv.off[l] + idx] = (uint8_t)((sum + 128) >> 8);
}
__global__ __launch_bounds__(PT) void sof_pyr_kernel(SofDev d, PyrArgs a) {
  const int s = a.streams[blockIdx.y];
  if (bad_stream(d, s)) return;
  pyr_pixel(pyr_of(d, s, d.par[s] ^ 1), a, blockIdx.x * PT + threadIdx.x);
}

// ------------------------------------------------------------------------------------------
// minimum eigenvalue of the 3x3 structure tensor
__device__ __forceinline__ void sobel_at(const uint8_t* I, int w, int h, int x, int y, int& dx,
                                         int& dy) {
  const int xl = refl(x - 1, w), xr = refl(x + 1, w), yu = refl(y - 1, h), yd = refl(y + 1, h);
  const uint8_t *ru = I + (size_t)yu * w, *rc = I + (size_t)y * w, *rd = I + (size_t)yd * w;
  const int ul = ru[xl], uc = ru[x], ur = ru[xr], cl = rc[xl], cr = rc[xr];
  const int dl = rd[xl], dc = rd[x], dr = rd[xr];
  dx = (ur - ul) + 2 * (cr - cl) + (dr - dl);
  dy = (dl - ul) + 2 * (dc - uc) + (dr - ur);
}
__device__ __forceinline__ double min_eig(double a, double b, double c) {
  const double hd = 0.25 * ((a - c) * (a - c));
  return 0.5 * (a + c) - sqrt(hd + b * b);
}

struct RespArgs {
  const int32_t* streams;
  Lv lv;
};
// pixel idx of the w x h level 0 at I: its lambda into L, the plane's maximum into *lmax.  Called
// by whole waves.
__device__ __forceinline__ void resp_pixel(const uint8_t* I, int w, int h, int idx, double* L,
                                           unsigned long long* lmax) {
  unsigned long long bits = 0ull;
  if (idx < h * w) {
    const int x = idx % w, y = idx / w;
    int sa = 0, sb = 0, sc = 0;
#pragma unroll
    for (int i = -1; i <= 1; i++)
#pragma unroll
      for (int j = -1; j <= 1; j++) {
        int dx, dy;
        sobel_at(I, w, h, refl(x + j, w), refl(y + i, h), dx, dy);
        sa += dx * dx;
        sb += dx * dy;
        sc += dy * dy;
      }
    const double lam = min_eig((double)sa, (double)sb, (double)sc);
    L[idx] = lam;
    if (lam > 0.0) bits = (unsigned long long)__double_as_longlong(lam);
  }
  // the wave's maximum, then one atomic per wave (non-negative doubles order like their bits)
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) {
    const unsigned long long o = __shfl_xor(bits, dd);
    bits = o > bits ? o : bits;
  }
  if ((threadIdx.x & 63) == 0 && bits) atomicMax(lmax, bits);
}
__global__ __launch_bounds__(PT) void sof_resp_kernel(SofDev d, RespArgs a) {
  const int s = a.streams[blockIdx.y];
  if (bad_stream(d, s)) return;
  resp_pixel(pyr_of(d, s, d.par[s] ^ 1), a.lv.w[0], a.lv.h[0], blockIdx.x * PT + threadIdx.x,
             d.lam + (size_t)s * d.cap, d.lmax + s);
}

// ------------------------------------------------------------------------------------------
// selection and the switch of the stream's state
struct SelArgs {
  const int32_t* streams;
  int h, w, nl;  // level 0's size and the level count
  int max_corners;
  double quality;
  int32_t *code, *n_keypoints;
};

// exclusive prefix of a 0/1 flag over the 1024 threads in thread order; tmp: SW ints
__device__ __forceinline__ int scan1024(bool f, int* tmp, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) tmp[wv] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < SW; k++) {
    const int c = tmp[k];
    off += k < wv ? c : 0;
    tot += c;
  }
  total = tot;
  __syncthreads();
  return off + pre;
}

// The corners of the w x h lambda plane L (maximum's bits: lmax) ranked into kp; ck / ci: the
// plane's candidate scratch; tmp: SW ints of LDS.  Returns their number.  By the ST threads of a
// workgroup.
__device__ __forceinline__ int select_corners(const double* L, unsigned long long lmax,
                                              unsigned long long* ck, int* ci, double* kp, int w,
                                              int h, int K, double quality, int* tmp) {
  __shared__ unsigned long long skey[MAXC];
  __shared__ int sidx[MAXC];
  __shared__ int hist[256];
  __shared__ unsigned long long sh_prefix;
  __shared__ int sh_need;
  const int tid = threadIdx.x;
  const int npix = h * w;
  const double floor_lam = quality * __longlong_as_double((long long)lmax);

  // candidates, compacted in pixel order
  int nc = 0;
  for (int c0 = 0; c0 < npix; c0 += ST) {
    const int idx = c0 + tid;
    bool f = false;
    double v = 0.0;
    if (idx < npix) {
      const int x = idx % w, y = idx / w;
      if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
        v = L[idx];
        f = v > 0.0 && v >= floor_lam;
        if (f) {
#pragma unroll
          for (int i = -1; i <= 1; i++)
#pragma unroll
            for (int j = -1; j <= 1; j++)
              if (i != 0 || j != 0) f = f && v >= L[idx + i * w + j];
        }
      }
    }
    int tot;
    const int pos = scan1024(f, tmp, tot);
    if (f) {
      ck[nc + pos] = (unsigned long long)__double_as_longlong(v);
      ci[nc + pos] = idx;
    }
    nc += tot;
  }
  __syncthreads();  // (the candidates are read by other threads below)

  // the K-th largest key by a radix pass from the top byte; need: how many equal to it survive
  unsigned long long thr = 0ull;  // survivors: key > thr, and the first `need` with key == thr
  int need = 0;
  if (nc > K) {
    if (tid == 0) {
      sh_prefix = 0ull;
      sh_need = K;
    }
    for (int b = 7; b >= 0; b--) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = sh_prefix;
      const unsigned long long himask = b == 7 ? 0ull : ~0ull << (8 * (b + 1));
      for (int k = tid; k < nc; k += ST) {
        const unsigned long long key = ck[k];
        if ((key & himask) == prefix) atomicAdd(&hist[(int)((key >> (8 * b)) & 255ull)], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int left = sh_need, bin = 255;
        for (; bin > 0; bin--) {
          if (hist[bin] >= left) break;
          left -= hist[bin];
        }
        sh_prefix = prefix | ((unsigned long long)bin << (8 * b));
        sh_need = left;
      }
      __syncthreads();
    }
    thr = sh_prefix;
    need = sh_need;
  }

  // survivors into LDS, still in pixel order
  int ns = 0, neq = 0;
  for (int c0 = 0; c0 < nc; c0 += ST) {
    const int k = c0 + tid;
    unsigned long long key = 0ull;
    int idx = 0;
    if (k < nc) {
      key = ck[k];
      idx = ci[k];
    }
    const bool eq = k < nc && nc > K && key == thr;
    int teq;
    const int peq = scan1024(eq, tmp, teq);
    const bool f = k < nc && (key > thr || (eq && neq + peq < need));
    int tot;
    const int pos = scan1024(f, tmp, tot);
    if (f) {
      skey[ns + pos] = key;
      sidx[ns + pos] = idx;
    }
    neq += teq;
    ns += tot;
  }
  __syncthreads();

  // rank: lambda descending, pixel index ascending
  if (tid < ns) {
    const unsigned long long key = skey[tid];
    const int idx = sidx[tid];
    int rank = 0;
    for (int j = 0; j < ns; j++) {
      const unsigned long long kj = skey[j];
      rank += (kj > key || (kj == key && sidx[j] < idx)) ? 1 : 0;
    }
    kp[2 * rank] = (double)(idx % w);
    kp[2 * rank + 1] = (double)(idx / w);
  }
  return ns;
}

__global__ __launch_bounds__(ST) void sof_select_kernel(SofDev d, SelArgs a) {
  __shared__ int tmp[SW];
  const int tid = threadIdx.x;
  const int s = a.streams[blockIdx.x];
  if (bad_stream(d, s)) return;
  const int w = a.w, h = a.h;
  const bool first = is_first(d, s, h, w, a.nl);
  double* kp = d.kp + (size_t)s * MAXC * 2;
  const int ns = select_corners(d.lam + (size_t)s * d.cap, d.lmax[s], d.ckey + (size_t)s * d.cap,
                                d.cidx + (size_t)s * d.cap, kp, w, h, a.max_corners, a.quality,
                                tmp);
  int nk = ns;
  if (ns == 0 && !first) {
    // no corner on this frame: the tracked points are kept, in order
    const int n = d.rn[s];
    const double* rq = d.rnext + (size_t)s * MAXC * 2;
    const uint8_t* ok = d.rok + (size_t)s * MAXC;
    const bool f = tid < n && ok[tid];
    int tot;
    const int pos = scan1024(f, tmp, tot);
    if (f) {
      kp[2 * pos] = rq[2 * tid];
      kp[2 * pos + 1] = rq[2 * tid + 1];
    }
    nk = tot;
  }
  if (tid == 0) {
    a.n_keypoints[s] = nk;
    if (first && nk == 0) {
      a.code[s] = BX_SOF_NO_KEYPOINTS;
      if (d.has_prev[s]) atomicMax(d.status, (int)BX_ERR_SHAPE);
      d.has_prev[s] = 0;
    } else {
      if (first && d.has_prev[s]) atomicMax(d.status, (int)BX_ERR_SHAPE);
      d.has_prev[s] = 1;
      d.ph[s] = h;
      d.pw[s] = w;
      d.pnl[s] = a.nl;
      d.par[s] ^= 1;
    }
    d.nkp[s] = nk;
  }
}

// ------------------------------------------------------------------------------------------
// tracking
struct TrackArgs {
  const int32_t* streams;
  Lv lv;
  int win, max_iter;
  double eps;
};

struct Win {
  int x0, y0;
  double w00, w01, w10, w11;
};
// the window anchored at (tx, ty): false when it is not inside the w x h level (NaN included)
__device__ __forceinline__ bool window_at(double tx, double ty, int win, int w, int h, Win& o) {
  const double fx = floor(tx), fy = floor(ty);
  if (!(fx >= 0.0 && fx + (double)win <= (double)(w - 1) && fy >= 0.0 &&
        fy + (double)win <= (double)(h - 1)))
    return false;
  const double ax = tx - fx, ay = ty - fy;
  o.x0 = (int)fx;
  o.y0 = (int)fy;
  o.w00 = (1.0 - ax) * (1.0 - ay);
  o.w01 = ax * (1.0 - ay);
  o.w10 = (1.0 - ax) * ay;
  o.w11 = ax * ay;
  return true;
}
__device__ __forceinline__ double blend(const Win& o, double v00, double v01, double v10,
                                        double v11) {
  return ((o.w00 * v00 + o.w01 * v01) + o.w10 * v10) + o.w11 * v11;
}

// One wave tracks keypoint pt of kp from the pyramid P into the pyramid C and writes entry pt of
// the record r; TI: the wave's LDS slab of 3 * win * win doubles.
__device__ __forceinline__ void track_point(const uint8_t* P, const uint8_t* C, const double* kp,
                                            int pt, const TrackArgs& a, double* TI, const Rec& r) {
  const int lane = threadIdx.x & 63;
  const int win = a.win, nw = win * win;
  const double half = (double)((win - 1) / 2);
  double *TX = TI + nw, *TY = TX + nw;
  const double px = kp[2 * pt], py = kp[2 * pt + 1];
  const double eps2 = a.eps * a.eps;
  double qx = 0.0, qy = 0.0;
  int iters = 0;
  bool lost = false;
  for (int l = a.lv.nl - 1; l >= 0; l--) {
    const int w = a.lv.w[l], h = a.lv.h[l];
    const uint8_t *Pl = P + a.lv.off[l], *Cl = C + a.lv.off[l];
    const double sc = 1.0 / (double)(1 << l);
    const double plx = px * sc, ply = py * sc;
    if (l == a.lv.nl - 1) {
      qx = plx;
      qy = ply;
    } else {
      qx = 2.0 * qx;
      qy = 2.0 * qy;
    }
    Win o;
    bool fail = !window_at(plx - half, ply - half, win, w, h, o);
    double gxx = 0.0, gxy = 0.0, gyy = 0.0, det = 0.0;
    if (!fail) {
      double sxx = 0.0, sxy = 0.0, syy = 0.0;
      for (int k = lane; k < nw; k += WAVE) {
        const int i = k / win, j = k - i * win;
        const int x = o.x0 + j, y = o.y0 + i;  // taps x, x + 1 and y, y + 1 are inside
        int xs[4], v[4][4];
        xs[0] = refl(x - 1, w);
        xs[1] = x;
        xs[2] = x + 1;
        xs[3] = refl(x + 2, w);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int yy = r == 0 ? refl(y - 1, h) : r == 3 ? refl(y + 2, h) : y + r - 1;
          const uint8_t* row = Pl + (size_t)yy * w;
#pragma unroll
          for (int c = 0; c < 4; c++) v[r][c] = row[xs[c]];
        }
        double ix[2][2], iy[2][2];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
          for (int c = 0; c < 2; c++) {
            ix[r][c] = (double)(3 * (v[r][c + 2] - v[r][c]) + 10 * (v[r + 1][c + 2] - v[r + 1][c]) +
                                3 * (v[r + 2][c + 2] - v[r + 2][c]));
            iy[r][c] = (double)(3 * (v[r + 2][c] - v[r][c]) + 10 * (v[r + 2][c + 1] - v[r][c + 1]) +
                                3 * (v[r + 2][c + 2] - v[r][c + 2]));
          }
        const double iv = blend(o, (double)v[1][1], (double)v[1][2], (double)v[2][1],
                                (double)v[2][2]);
        const double dxv = blend(o, ix[0][0], ix[0][1], ix[1][0], ix[1][1]);
        const double dyv = blend(o, iy[0][0], iy[0][1], iy[1][0], iy[1][1]);
        TI[k] = iv;
        TX[k] = dxv;
        TY[k] = dyv;
        sxx += dxv * dxv;
        sxy += dxv * dyv;
        syy += dyv * dyv;
      }
      gxx = wave_bfly_desc_f64(sxx);
      gxy = wave_bfly_desc_f64(sxy);
      gyy = wave_bfly_desc_f64(syy);
      det = gxx * gyy - gxy * gxy;
      const double me = min_eig(gxx, gxy, gyy) / (1048576.0 * (double)nw);
      if (me < 1e-4 || !(det > 0.0)) fail = true;
    }
    if (!fail) {
      double pdx = 0.0, pdy = 0.0;
      for (int j = 0; j < a.max_iter; j++) {
        if (!window_at(qx - half, qy - half, win, w, h, o)) {
          fail = true;
          break;
        }
        double b1 = 0.0, b2 = 0.0;
        for (int k = lane; k < nw; k += WAVE) {
          const int i = k / win, jj = k - i * win;
          const uint8_t* row = Cl + (size_t)(o.y0 + i) * w + (o.x0 + jj);
          const double jv = blend(o, (double)row[0], (double)row[1], (double)row[w],
                                  (double)row[w + 1]);
          const double df = 32.0 * (jv - TI[k]);  // the Scharr kernel's gain (exact)
          b1 += df * TX[k];
          b2 += df * TY[k];
        }
        b1 = wave_bfly_desc_f64(b1);
        b2 = wave_bfly_desc_f64(b2);
        const double dx = (gxy * b2 - gyy * b1) / det;
        const double dy = (gxy * b1 - gxx * b2) / det;
        qx += dx;
        qy += dy;
        iters++;
        if (dx * dx + dy * dy <= eps2) break;
        if (j > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
          qx -= 0.5 * dx;
          qy -= 0.5 * dy;
          break;
        }
        pdx = dx;
        pdy = dy;
      }
    }
    if (fail && l == 0) lost = true;
  }
  if (!lost && !(qx >= 0.0 && qx <= (double)(a.lv.w[0] - 1) && qy >= 0.0 &&
                 qy <= (double)(a.lv.h[0] - 1)))
    lost = true;
  if (lane == 0) {
    r.prev[2 * pt] = px;
    r.prev[2 * pt + 1] = py;
    r.next[2 * pt] = qx;
    r.next[2 * pt + 1] = qy;
    r.ok[pt] = lost ? 0 : 1;
    r.inl[pt] = 0;
    r.iter[pt] = iters;
  }
}

__global__ __launch_bounds__(TW * WAVE) void sof_track_kernel(SofDev d, TrackArgs a) {
  extern __shared__ double tl[];  // [TW][3][win * win]: template I, Ix, Iy of the wave's point
  const int wv = threadIdx.x >> 6;
  const int s = a.streams[blockIdx.y];
  if (bad_stream(d, s)) return;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (is_first(d, s, a.lv)) {
    if (lead) d.rn[s] = 0;
    return;
  }
  const int n = d.nkp[s];
  if (lead) d.rn[s] = n;
  const int pt = blockIdx.x * TW + wv;
  if (pt >= n) return;
  const int par = d.par[s];
  track_point(pyr_of(d, s, par), pyr_of(d, s, par ^ 1), d.kp + (size_t)s * MAXC * 2, pt, a,
              tl + (size_t)wv * 3 * a.win * a.win, rec_of(d, s));
}

// ------------------------------------------------------------------------------------------
// the fit
struct FitArgs {
  const int32_t* streams;
  int h, w, nl;
  double thr2, scale;
  double* warps;
  int32_t *code, *n_tracked, *n_inliers;
};

__host__ __device__ inline uint32_t sof_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

struct Sim {
  double a, b, tx, ty;
};
__device__ __forceinline__ bool sim_inlier(const Sim& m, double px, double py, double qx,
                                           double qy, double thr2) {
  const double rx = ((m.a * px - m.b * py) + m.tx) - qx;
  const double ry = ((m.b * px + m.a * py) + m.ty) - qy;
  return rx * rx + ry * ry <= thr2;
}

// the fit's LDS, FIT_LDS bytes: the tracked pairs, their record indices and the reductions
constexpr size_t FIT_LDS = (size_t)MAXC * (4 * 8 + 2) + 4 * 4 + FW * 8;
struct FitLds {
  double *PX, *PY, *QX, *QY;  // [MAXC] each
  unsigned long long* best;   // [FW]
  int* tmp;                   // [4]
  short* CI;                  // [MAXC]
};
__device__ __forceinline__ FitLds fit_lds(void* base) {
  FitLds f;
  f.PX = (double*)base;
  f.PY = f.PX + MAXC;
  f.QX = f.PY + MAXC;
  f.QY = f.QX + MAXC;
  f.best = (unsigned long long*)(f.QY + MAXC);
  f.tmp = (int*)(f.best + FW);
  f.CI = (short*)(f.tmp + 4);
  return f;
}

// One result row (thread 0 writes): the warp of the similarity m (the identity without one), the
// code, the counts, and the winner into *rwin.
__device__ __forceinline__ void fit_finish(const FitArgs& a, size_t row, int* rwin, int code,
                                           int ntrk, int ninl, int winner, const Sim* m) {
  if (threadIdx.x != 0) return;
  double* W = a.warps + row * 6;
  double o[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (m) {
    o[0] = m->a;
    o[1] = -m->b;
    o[2] = m->tx;
    o[3] = m->b;
    o[4] = m->a;
    o[5] = m->ty;
    if (a.scale > 0.0 && a.scale < 1.0) {
      o[2] = o[2] / a.scale;
      o[5] = o[5] / a.scale;
    }
  }
  for (int q = 0; q < 6; q++) W[q] = o[q];
  a.code[row] = code;
  a.n_tracked[row] = ntrk;
  a.n_inliers[row] = ninl;
  *rwin = winner;
}

// The consensus fit over the n entries of the record r, by the FT threads of a workgroup; the
// result goes to row `row`.  Every thread returns; the LDS may be reused after a barrier.
__device__ __forceinline__ void fit_pairs(const Rec& r, int n, const FitArgs& a, size_t row,
                                          int* rwin, const FitLds& F) {
  double *PX = F.PX, *PY = F.PY, *QX = F.QX, *QY = F.QY;
  short* CI = F.CI;
  unsigned long long* best = F.best;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto finish = [&](int code, int ntrk, int ninl, int winner, const Sim* m) {
    fit_finish(a, row, rwin, code, ntrk, ninl, winner, m);
  };
  const int m = block_compact(
      n, [&](int k) { return r.ok[k] != 0; },
      [&](int k, int pos) {
        PX[pos] = r.prev[2 * k];
        PY[pos] = r.prev[2 * k + 1];
        QX[pos] = r.next[2 * k];
        QY[pos] = r.next[2 * k + 1];
        CI[pos] = (short)k;
      },
      F.tmp);
  if (m < 4) {
    finish(BX_SOF_TOO_FEW, m, 0, -1, nullptr);
    return;
  }
  auto model = [&](int k, Sim& o) {  // false: the hypothesis is skipped
    const int i = (int)(sof_mix(2u * (uint32_t)k) % (uint32_t)m);
    const int j = (int)(sof_mix(2u * (uint32_t)k + 1u) % (uint32_t)m);
    const double dx = PX[j] - PX[i], dy = PY[j] - PY[i];
    if (dx == 0.0 && dy == 0.0) return false;
    const double ex = QX[j] - QX[i], ey = QY[j] - QY[i];
    const double n2 = dx * dx + dy * dy;
    o.a = (dx * ex + dy * ey) / n2;
    o.b = (dx * ey - dy * ex) / n2;
    o.tx = QX[i] - (o.a * PX[i] - o.b * PY[i]);
    o.ty = QY[i] - (o.b * PX[i] + o.a * PY[i]);
    return true;
  };
  // waves take hypotheses, lanes take points; key (count, -k), 0: nothing usable
  unsigned long long bk = 0ull;
  for (int k = wv; k < NHYP; k += FW) {
    Sim hm;
    if (!model(k, hm)) continue;  // (wave-uniform)
    int cnt = 0;
    for (int c0 = 0; c0 < m; c0 += WAVE) {
      const int q = c0 + lane;
      const bool in = q < m && sim_inlier(hm, PX[q], PY[q], QX[q], QY[q], a.thr2);
      cnt += __popcll(__ballot(in));
    }
    const unsigned long long key = ((unsigned long long)cnt << 32) | (0xffffffffu - (uint32_t)k);
    bk = key > bk ? key : bk;
  }
  if (lane == 0) best[wv] = bk;
  __syncthreads();
  bk = 0ull;
#pragma unroll
  for (int k = 0; k < FW; k++) bk = best[k] > bk ? best[k] : bk;
  if (bk == 0ull) {
    finish(BX_SOF_NO_MODEL, m, 0, -1, nullptr);
    return;
  }
  const int winner = (int)(0xffffffffu - (uint32_t)(bk & 0xffffffffull));
  if (wv != 0) return;
  // wave 0: the least-squares similarity over the winner's inliers, two passes
  Sim hm;
  model(winner, hm);
  double sp = 0.0, sq = 0.0, sr = 0.0, st = 0.0;
  int cnt = 0;
  for (int q = lane; q < m; q += WAVE) {
    if (!sim_inlier(hm, PX[q], PY[q], QX[q], QY[q], a.thr2)) continue;
    r.inl[CI[q]] = 1;
    cnt++;
    sp += PX[q];
    sq += PY[q];
    sr += QX[q];
    st += QY[q];
  }
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) cnt += __shfl_xor(cnt, dd);
  sp = wave_bfly_desc_f64(sp);
  sq = wave_bfly_desc_f64(sq);
  sr = wave_bfly_desc_f64(sr);
  st = wave_bfly_desc_f64(st);
  const double cn = (double)cnt;
  const double mpx = sp / cn, mpy = sq / cn, mqx = sr / cn, mqy = st / cn;
  double spq = 0.0, sxq = 0.0, spp = 0.0;
  for (int q = lane; q < m; q += WAVE) {
    if (!sim_inlier(hm, PX[q], PY[q], QX[q], QY[q], a.thr2)) continue;
    const double ux = PX[q] - mpx, uy = PY[q] - mpy, vx = QX[q] - mqx, vy = QY[q] - mqy;
    spq += ux * vx + uy * vy;
    sxq += ux * vy - uy * vx;
    spp += ux * ux + uy * uy;
  }
  spq = wave_bfly_desc_f64(spq);
  sxq = wave_bfly_desc_f64(sxq);
  spp = wave_bfly_desc_f64(spp);
  if (cnt < 1 || !(spp > 0.0)) {
    finish(BX_SOF_NO_MODEL, m, 0, -1, nullptr);
    return;
  }
  Sim ls;
  ls.a = spq / spp;
  ls.b = sxq / spp;
  ls.tx = mqx - (ls.a * mpx - ls.b * mpy);
  ls.ty = mqy - (ls.b * mpx + ls.a * mpy);
  finish(BX_SOF_OK, m, cnt, winner, &ls);
}

__global__ __launch_bounds__(FT) void sof_fit_kernel(SofDev d, FitArgs a) {
  __shared__ double fl[FIT_LDS / 8];
  static_assert(FIT_LDS % 8 == 0, "the fit's LDS is carved from doubles");
  const int s = a.streams[blockIdx.x];
  if (bad_stream(d, s)) return;
  if (is_first(d, s, a.h, a.w, a.nl)) {
    fit_finish(a, (size_t)s, d.rwin + s, BX_SOF_FIRST_FRAME, 0, 0, -1, nullptr);
    return;
  }
  fit_pairs(rec_of(d, s), d.rn[s], a, (size_t)s, d.rwin + s, fit_lds(fl));
}

// ------------------------------------------------------------------------------------------
// The chained apply: n frames per call, frame i in slot i.  Frame i is tracked
// from frame i - 1 of the call when both are of one stream, else from the stream's stored state.
// A group is a stream's run of adjacent frames.  Launches, all on the caller's stream:
//   sof_chain_prep_kernel      level 0 of every slot's pyramid
//   sof_chain_pyr_kernel       (nl - 1 launches) the higher levels
//   sof_chain_resp_kernel      every slot's lambda plane and its maximum
//   sof_chain_select_kernel    every slot's corners into the slot's keypoints; no stream state
//   sof_chain_plan_kernel      one thread per group walks it: which frames are first frames (a
//                              prefix: the stored state is first and no frame so far had a corner),
//                              which keep the tracked points (no corner, not first), which pairs
//                              are deferred (their template frame keeps tracked points)
//   sof_chain_track_kernel     sof_track_kernel's body for every pair that is not deferred
//   sof_chain_fit_kernel       sof_fit_kernel's body for the same pairs; first frames' rows
//   sof_chain_tail_kernel      one workgroup per group walks its frames in order: a deferred pair
//                              is tracked (a wave per keypoint, looped) and fitted, a frame that
//                              keeps the tracked points compacts them into its slot.  Without such
//                              a frame it reads one flag per frame
//   sof_chain_handover_kernel  the last slot of every group becomes its stream's state.  A launch
//                              of its own: the workgroups of a group's first pair read the stream's
//                              stored pyramid and keypoints, so nothing before may write them
// No workgroup waits for another, no host round trip.
constexpr int PL_FIRST = 1, PL_NOKP = 2, PL_KEEP = 4, PL_DEFER = 8;

struct ChainArgs {
  const int32_t* streams;  // [n]
  const int64_t* dst;      // [n] result row of each frame, or null: row i
  int n;
  Lv lv;
};
__device__ __forceinline__ size_t row_of(const ChainArgs& a, int i) {
  return a.dst ? (size_t)a.dst[i] : (size_t)i;
}
__device__ __forceinline__ uint8_t* slot_pyr(const SofDev& d, const SofChain& c, int i) {
  return c.pyr + (size_t)i * d.pcap;
}
__device__ __forceinline__ bool chained(const ChainArgs& a, int i) {
  return i > 0 && a.streams[i - 1] == a.streams[i];
}

__global__ __launch_bounds__(PT) void sof_chain_prep_kernel(SofDev d, SofChain c, PrepArgs a) {
  const int i = blockIdx.y;
  const int s = a.streams[i];
  if (bad_stream(d, s)) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicMax(d.status, (int)BX_ERR_INVALID);
    return;
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) c.lmax[i] = 0ull;  // (read two launches later)
  const int idx = blockIdx.x * PT + threadIdx.x;
  if (idx >= a.h * a.w) return;
  const int x = idx % a.w, y = idx / a.w;
  const uint8_t* f = a.frames + (size_t)i * a.H * a.W * a.ch;
  slot_pyr(d, c, i)[idx] = (uint8_t)work_pixel(a, f, x, y);
}

__global__ __launch_bounds__(PT) void sof_chain_pyr_kernel(SofDev d, SofChain c, PyrArgs a) {
  const int i = blockIdx.y;
  if (bad_stream(d, a.streams[i])) return;
  pyr_pixel(slot_pyr(d, c, i), a, blockIdx.x * PT + threadIdx.x);
}

__global__ __launch_bounds__(PT) void sof_chain_resp_kernel(SofDev d, SofChain c, RespArgs a) {
  const int i = blockIdx.y;
  if (bad_stream(d, a.streams[i])) return;
  resp_pixel(slot_pyr(d, c, i), a.lv.w[0], a.lv.h[0], blockIdx.x * PT + threadIdx.x,
             c.lam + (size_t)i * d.cap, c.lmax + i);
}

// a.n_keypoints: the rows by frame; a.code is not used
__global__ __launch_bounds__(ST) void sof_chain_select_kernel(SofDev d, SofChain c, SelArgs a,
                                                              const int64_t* dst) {
  __shared__ int tmp[SW];
  const int i = blockIdx.x;
  if (bad_stream(d, a.streams[i])) return;
  const int ns = select_corners(c.lam + (size_t)i * d.cap, c.lmax[i], c.ckey + (size_t)i * d.cap,
                                c.cidx + (size_t)i * d.cap, c.kp + (size_t)i * MAXC * 2, a.w, a.h,
                                a.max_corners, a.quality, tmp);
  if (threadIdx.x == 0) {
    c.nkp[i] = ns;  // (a frame that keeps the tracked points gets its count from the tail)
    a.n_keypoints[dst ? (size_t)dst[i] : (size_t)i] = ns;
  }
}

__global__ __launch_bounds__(PT) void sof_chain_plan_kernel(SofDev d, SofChain c, ChainArgs a) {
  const int g = blockIdx.x * PT + threadIdx.x;
  if (g >= a.n) return;
  const int s = a.streams[g];
  if (bad_stream(d, s) || chained(a, g)) return;  // (one thread per group: its first frame)
  bool first = is_first(d, s, a.lv);
  if (first && d.has_prev[s]) atomicMax(d.status, (int)BX_ERR_SHAPE);
  int flips = 0, i = g;
  bool kept = false;  // the frame before keeps tracked points as its keypoints
  for (; i < a.n && a.streams[i] == s; i++) {
    const bool corners = c.nkp[i] > 0;
    int p = 0;
    if (first) p = corners ? PL_FIRST : PL_FIRST | PL_NOKP;
    else p = (corners ? 0 : PL_KEEP) | (kept ? PL_DEFER : 0);
    c.plan[i] = p;
    kept = (p & PL_KEEP) != 0;
    if (!(p & PL_NOKP)) flips++;
    first = first && !corners;
  }
  c.topar[i - 1] = d.par[s] ^ (flips & 1);  // as many switches as the plain applies make
}

struct ChainTrackArgs {
  ChainArgs ch;
  TrackArgs t;  // (t.streams is not used)
};
// the pair of frame i: where its keypoints and its previous pyramid are
__device__ __forceinline__ void pair_source(const SofDev& d, const SofChain& c, const ChainArgs& a,
                                            int i, const uint8_t*& P, const double*& kp, int& n) {
  if (chained(a, i)) {
    P = slot_pyr(d, c, i - 1);
    kp = c.kp + (size_t)(i - 1) * MAXC * 2;
    n = c.nkp[i - 1];
  } else {
    const int s = a.streams[i];
    P = pyr_of(d, s, d.par[s]);
    kp = d.kp + (size_t)s * MAXC * 2;
    n = d.nkp[s];
  }
}

__global__ __launch_bounds__(TW * WAVE) void sof_chain_track_kernel(SofDev d, SofChain c,
                                                                     ChainTrackArgs a) {
  extern __shared__ double tl[];  // [TW][3][win * win]
  const int wv = threadIdx.x >> 6;
  const int i = blockIdx.y;
  if (bad_stream(d, a.ch.streams[i])) return;
  const int p = c.plan[i];
  if (p & PL_DEFER) return;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (p & PL_FIRST) {
    if (lead) c.rn[i] = 0;
    return;
  }
  const uint8_t* P;
  const double* kp;
  int n;
  pair_source(d, c, a.ch, i, P, kp, n);
  if (lead) c.rn[i] = n;
  const int pt = blockIdx.x * TW + wv;
  if (pt >= n) return;
  track_point(P, slot_pyr(d, c, i), kp, pt, a.t, tl + (size_t)wv * 3 * a.t.win * a.t.win,
              rec_of(c, i));
}

struct ChainFitArgs {
  ChainArgs ch;
  FitArgs f;  // (f.streams is not used; its rows are by frame)
};
__global__ __launch_bounds__(FT) void sof_chain_fit_kernel(SofDev d, SofChain c, ChainFitArgs a) {
  __shared__ double fl[FIT_LDS / 8];
  const int i = blockIdx.x;
  if (bad_stream(d, a.ch.streams[i])) return;
  const int p = c.plan[i];
  if (p & PL_DEFER) return;
  const size_t row = row_of(a.ch, i);
  if (p & PL_FIRST) {
    fit_finish(a.f, row, c.rwin + i, (p & PL_NOKP) ? BX_SOF_NO_KEYPOINTS : BX_SOF_FIRST_FRAME, 0, 0,
               -1, nullptr);
    return;
  }
  fit_pairs(rec_of(c, i), c.rn[i], a.f, row, c.rwin + i, fit_lds(fl));
}

struct ChainTailArgs {
  ChainArgs ch;
  TrackArgs t;
  FitArgs f;
  int tw;  // waves that track: tw slabs fit the dynamic LDS
  int32_t* n_keypoints;
};
__global__ __launch_bounds__(FT) void sof_chain_tail_kernel(SofDev d, SofChain c,
                                                            ChainTailArgs a) {
  extern __shared__ double tl[];  // max(tw track slabs, FIT_LDS), one after the other in time
  const int wv = threadIdx.x >> 6;
  const int g = blockIdx.x;
  const int s = a.ch.streams[g];
  if (bad_stream(d, s) || chained(a.ch, g)) return;  // (one workgroup per group)
  for (int i = g; i < a.ch.n && a.ch.streams[i] == s; i++) {  // (uniform)
    const int p = c.plan[i];
    if (!(p & (PL_DEFER | PL_KEEP))) continue;
    const Rec r = rec_of(c, i);
    const size_t row = row_of(a.ch, i);
    if (p & PL_DEFER) {
      // the template frame's keypoints are the tracked points compacted one turn earlier
      const double* kp = c.kp + (size_t)(i - 1) * MAXC * 2;
      const int n = c.nkp[i - 1];
      if (threadIdx.x == 0) c.rn[i] = n;
      if (wv < a.tw)
        for (int pt = wv; pt < n; pt += a.tw)
          track_point(slot_pyr(d, c, i - 1), slot_pyr(d, c, i), kp, pt, a.t,
                      tl + (size_t)wv * 3 * a.t.win * a.t.win, r);
      __syncthreads();  // the record is read by every thread; the slabs become the fit's arrays
      fit_pairs(r, n, a.f, row, c.rwin + i, fit_lds(tl));
      __syncthreads();
    }
    if (p & PL_KEEP) {
      // no corner on this frame: the tracked points are kept, in order
      double* kp = c.kp + (size_t)i * MAXC * 2;
      const int nk = block_compact(
          c.rn[i], [&](int k) { return r.ok[k] != 0; },
          [&](int k, int pos) {
            kp[2 * pos] = r.next[2 * k];
            kp[2 * pos + 1] = r.next[2 * k + 1];
          },
          (int*)tl);
      if (threadIdx.x == 0) {
        c.nkp[i] = nk;
        a.n_keypoints[row] = nk;
      }
      __syncthreads();
    }
  }
}

// The last frame of each group: its slot becomes the stream's state, as after a plain apply of
// every frame of the group.  Rows of the keypoints and of the record beyond the last frame's
// counts are those of the latest frame of the group that wrote them, as the plain applies leave
// them.
__global__ __launch_bounds__(PT) void sof_chain_handover_kernel(SofDev d, SofChain c,
                                                                ChainArgs a) {
  const int k = blockIdx.y;
  const int s = a.streams[k];
  if (bad_stream(d, s)) return;
  if (k + 1 < a.n && a.streams[k + 1] == s) return;
  const int idx = blockIdx.x * PT + threadIdx.x;
  const int h = a.lv.h[0], w = a.lv.w[0], nl = a.lv.nl;
  const int p = c.plan[k];
  const bool none = (p & PL_NOKP) != 0;  // every frame of the group was a first one without a corner
  if (idx == 0) {
    d.has_prev[s] = none ? 0 : 1;
    if (!none) {
      d.ph[s] = h;
      d.pw[s] = w;
      d.pnl[s] = nl;
    }
    d.nkp[s] = c.nkp[k];
    d.rn[s] = c.rn[k];
    d.rwin[s] = c.rwin[k];
    d.lmax[s] = c.lmax[k];
    d.par[s] = c.topar[k];  // (no thread of this launch reads par[])
  }
  const int to = c.topar[k];
  if (!none) {
    const int bytes = a.lv.off[nl - 1] + a.lv.h[nl - 1] * a.lv.w[nl - 1];
    if (idx < bytes) pyr_of(d, s, to)[idx] = slot_pyr(d, c, k)[idx];
  }
  if (idx < h * w) d.lam[(size_t)s * d.cap + idx] = c.lam[(size_t)k * d.cap + idx];
  if (idx < MAXC) {
    const Rec rs = rec_of(d, s);
    bool kdone = false, rdone = false;
    for (int i = k; i >= 0 && a.streams[i] == s && !(kdone && rdone); i--) {
      if (!kdone && idx < c.nkp[i]) {
        const double* kp = c.kp + (size_t)i * MAXC * 2;
        d.kp[((size_t)s * MAXC + idx) * 2] = kp[2 * idx];
        d.kp[((size_t)s * MAXC + idx) * 2 + 1] = kp[2 * idx + 1];
        kdone = true;
      }
      if (!rdone && idx < c.rn[i]) {
        const Rec ri = rec_of(c, i);
        rs.prev[2 * idx] = ri.prev[2 * idx];
        rs.prev[2 * idx + 1] = ri.prev[2 * idx + 1];
        rs.next[2 * idx] = ri.next[2 * idx];
        rs.next[2 * idx + 1] = ri.next[2 * idx + 1];
        rs.iter[idx] = ri.iter[idx];
        rs.ok[idx] = ri.ok[idx];
        rs.inl[idx] = ri.inl[idx];
        rdone = true;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// host
void level_sizes(int h, int w, int win, int max_level, Lv& lv) {
  lv.nl = 1;
  lv.h[0] = h;
  lv.w[0] = w;
  lv.off[0] = 0;
  for (int l = 1; l < MAXL; l++) lv.h[l] = lv.w[l] = lv.off[l] = 0;
  for (int l = 1; l < MAXL && l <= max_level; l++) {
    const int nh = (lv.h[l - 1] + 1) / 2, nw = (lv.w[l - 1] + 1) / 2;
    if (!(nh > win && nw > win)) break;
    lv.h[l] = nh;
    lv.w[l] = nw;
    lv.off[l] = lv.off[l - 1] + lv.h[l - 1] * lv.w[l - 1];
    lv.nl = l + 1;
  }
}

int check_params(const bx_sof_params* p) {
  if (!p) return sf_err(BX_ERR_INVALID, "null sof parameters");
  if (p->max_corners < 1 || p->max_corners > MAXC)
    return sf_err(BX_ERR_INVALID, "max_corners must be 1.." + std::to_string(MAXC));
  if (p->win_size < 5 || p->win_size > 31 || p->win_size % 2 == 0)
    return sf_err(BX_ERR_INVALID, "win_size must be odd, 5..31");
  if (p->max_level < 0 || p->max_level >= MAXL)
    return sf_err(BX_ERR_INVALID, "max_level must be 0.." + std::to_string(MAXL - 1));
  if (p->max_iter < 0 || !(p->eps >= 0.0) || !(p->quality_level > 0.0 && p->quality_level <= 1.0) ||
      !(p->threshold > 0.0) || !(p->scale == p->scale))
    return sf_err(BX_ERR_INVALID, "max_iter/eps/quality_level/threshold/scale out of range");
  return BX_OK;
}

// argument checks shared by the two entries; sets the levels
int check_args(SofHandle* H_, int n, int H, int W, int ch, const bx_sof_params* p, Lv* lv) {
  if (!H_) return sf_err(BX_ERR_INVALID, "null sof handle");
  int rc = check_params(p);
  if (rc != BX_OK) return rc;
  if (n < 0 || H < 1 || W < 1 || (ch != 1 && ch != 3))
    return sf_err(BX_ERR_INVALID, "n/H/W/channels out of range");
  if ((long long)H * W * ch * (long long)(n > 0 ? n : 1) >= (1LL << 40))
    return sf_err(BX_ERR_INVALID, "frames too large");
  int h, w;
  rc = bx_ecc_work_size(H, W, p->scale, &h, &w);
  if (rc != BX_OK) return rc;
  if (n > H_->d.n_streams)
    return sf_err(BX_ERR_CAPACITY, "more frames than the handle has streams");
  if (h > H_->max_h || w > H_->max_w)
    return sf_err(BX_ERR_CAPACITY, "working image " + std::to_string(h) + "x" + std::to_string(w) +
                                       " exceeds the handle's " + std::to_string(H_->max_h) + "x" +
                                       std::to_string(H_->max_w));
  level_sizes(h, w, p->win_size, p->max_level, *lv);
  return BX_OK;
}

int launch(SofHandle* H_, int n, int H, int W, int ch, const uint8_t* frames,
           const int32_t* streams, const bx_sof_params& p, const Lv& lv, double* warps,
           int32_t* code, int32_t* nkp, int32_t* ntrk, int32_t* ninl, hipStream_t st) {
  const SofDev& d = H_->d;
  const int h = lv.h[0], w = lv.w[0];
  PrepArgs pa{frames, streams, H, W, ch, h, w, (p.scale > 0.0 && p.scale < 1.0) ? 1 : 0, p.scale};
  hipLaunchKernelGGL(sof_prep_kernel, dim3((h * w + PT - 1) / PT, n), dim3(PT), 0, st, d, pa);
  for (int l = 1; l < lv.nl; l++) {
    PyrArgs ya{streams, lv, l};
    hipLaunchKernelGGL(sof_pyr_kernel, dim3((lv.h[l] * lv.w[l] + PT - 1) / PT, n), dim3(PT), 0, st,
                       d, ya);
  }
  TrackArgs ta{streams, lv, p.win_size, p.max_iter, p.eps};
  const size_t lds = (size_t)TW * 3 * p.win_size * p.win_size * sizeof(double);  // <= 46128 B
  hipLaunchKernelGGL(sof_track_kernel, dim3(MAXC / TW, n), dim3(TW * WAVE), lds, st, d, ta);
  FitArgs fa{streams, h, w, lv.nl, p.threshold * p.threshold, p.scale, warps, code, ntrk, ninl};
  hipLaunchKernelGGL(sof_fit_kernel, dim3(n), dim3(FT), 0, st, d, fa);
  RespArgs ra{streams, lv};
  hipLaunchKernelGGL(sof_resp_kernel, dim3((h * w + PT - 1) / PT, n), dim3(PT), 0, st, d, ra);
  SelArgs sa{streams, h, w, lv.nl, p.max_corners, p.quality_level, code, nkp};
  hipLaunchKernelGGL(sof_select_kernel, dim3(n), dim3(ST), 0, st, d, sa);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

// the chained entries' checks: a call's frames are bounded by the reserved slots, not by the
// streams
int check_chain_args(SofHandle* H_, int n, int H, int W, int ch, const bx_sof_params* p, Lv* lv) {
  if (n < 0) return sf_err(BX_ERR_INVALID, "n/H/W/channels out of range");
  int rc = check_args(H_, 0, H, W, ch, p, lv);
  if (rc != BX_OK) return rc;
  if ((long long)H * W * ch * (long long)(n > 0 ? n : 1) >= (1LL << 40))
    return sf_err(BX_ERR_INVALID, "frames too large");
  if (n > H_->c.max_frames)
    return sf_err(BX_ERR_CAPACITY, "more frames than chain slots reserved (" +
                                       std::to_string(H_->c.max_frames) + ")");
  return BX_OK;
}

int launch_chain(SofHandle* H_, int n, int H, int W, int ch, const uint8_t* frames,
                 const int32_t* streams, const int64_t* dst, const bx_sof_params& p, const Lv& lv,
                 double* warps, int32_t* code, int32_t* nkp, int32_t* ntrk, int32_t* ninl,
                 hipStream_t st) {
  const SofDev& d = H_->d;
  const SofChain& c = H_->c;
  const int h = lv.h[0], w = lv.w[0];
  const dim3 pg((h * w + PT - 1) / PT, n);
  PrepArgs pa{frames, streams, H, W, ch, h, w, (p.scale > 0.0 && p.scale < 1.0) ? 1 : 0, p.scale};
  hipLaunchKernelGGL(sof_chain_prep_kernel, pg, dim3(PT), 0, st, d, c, pa);
  for (int l = 1; l < lv.nl; l++) {
    PyrArgs ya{streams, lv, l};
    hipLaunchKernelGGL(sof_chain_pyr_kernel, dim3((lv.h[l] * lv.w[l] + PT - 1) / PT, n), dim3(PT),
                       0, st, d, c, ya);
  }
  RespArgs ra{streams, lv};
  hipLaunchKernelGGL(sof_chain_resp_kernel, pg, dim3(PT), 0, st, d, c, ra);
  SelArgs sa{streams, h, w, lv.nl, p.max_corners, p.quality_level, code, nkp};
  hipLaunchKernelGGL(sof_chain_select_kernel, dim3(n), dim3(ST), 0, st, d, c, sa, dst);
  ChainArgs ca{streams, dst, n, lv};
  hipLaunchKernelGGL(sof_chain_plan_kernel, dim3((n + PT - 1) / PT), dim3(PT), 0, st, d, c, ca);
  TrackArgs ta{streams, lv, p.win_size, p.max_iter, p.eps};
  const size_t slab = (size_t)3 * p.win_size * p.win_size * sizeof(double);
  hipLaunchKernelGGL(sof_chain_track_kernel, dim3(MAXC / TW, n), dim3(TW * WAVE), TW * slab, st, d,
                     c, ChainTrackArgs{ca, ta});
  FitArgs fa{streams, h, w, lv.nl, p.threshold * p.threshold, p.scale, warps, code, ntrk, ninl};
  hipLaunchKernelGGL(sof_chain_fit_kernel, dim3(n), dim3(FT), 0, st, d, c, ChainFitArgs{ca, fa});
  // the tail's LDS: the larger of its track slabs and the fit's arrays (at most 48 KiB)
  const int tw = FW * slab <= 48 * 1024 ? FW : TW;
  const size_t tail_lds = tw * slab > FIT_LDS ? tw * slab : FIT_LDS;
  hipLaunchKernelGGL(sof_chain_tail_kernel, dim3(n), dim3(FT), tail_lds, st, d, c,
                     ChainTailArgs{ca, ta, fa, tw, nkp});
  const int bytes = lv.off[lv.nl - 1] + lv.h[lv.nl - 1] * lv.w[lv.nl - 1];
  const int most = bytes > MAXC ? bytes : MAXC;
  hipLaunchKernelGGL(sof_chain_handover_kernel, dim3((most + PT - 1) / PT, n), dim3(PT), 0, st, d,
                     c, ca);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

void free_chain(SofHandle* H_) {
  SofChain& c = H_->c;
  void** ps[] = {(void**)&c.pyr,   (void**)&c.lam,   (void**)&c.lmax,  (void**)&c.ckey,
                 (void**)&c.cidx,  (void**)&c.kp,    (void**)&c.rprev, (void**)&c.rnext,
                 (void**)&c.riter, (void**)&c.rok,   (void**)&c.rinl,  (void**)&c.nkp,
                 (void**)&H_->cstreams, (void**)&H_->cwarps, (void**)&H_->cints};
  for (void** p : ps) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  c.rn = c.rwin = c.plan = c.topar = nullptr;  // (parts of nkp's allocation)
  c.max_frames = 0;
}

}  // namespace

extern "C" {

int bx_sof_levels(int h, int w, int win_size, int max_level, int* n_levels, int* lh, int* lw) {
  if (!n_levels || !lh || !lw || h < 1 || w < 1 || win_size < 1 || max_level < 0)
    return sf_err(BX_ERR_INVALID, "bad level arguments");
  Lv lv;
  level_sizes(h, w, win_size, max_level, lv);
  *n_levels = lv.nl;
  for (int l = 0; l < MAXL; l++) {
    lh[l] = lv.h[l];
    lw[l] = lv.w[l];
  }
  return BX_OK;
}

int bx_sof_create(int n_streams, int max_h, int max_w, void** out) {
  if (!out) return sf_err(BX_ERR_INVALID, "null argument");
  if (n_streams < 1 || n_streams > BX_SOF_MAX_STREAMS || max_h < 1 || max_w < 1 ||
      (long long)max_h * max_w > (1LL << 26) ||
      (long long)n_streams * max_h * max_w * 24 > (1LL << 36))
    return sf_err(BX_ERR_INVALID, "n_streams/max_h/max_w out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return sf_err(BX_ERR_NO_DEVICE, "no HIP device visible");
  SofHandle* H_ = new SofHandle();
  H_->max_h = max_h;
  H_->max_w = max_w;
  SofDev& d = H_->d;
  d.n_streams = n_streams;
  d.cap = max_h * max_w;
  Lv top;
  level_sizes(max_h, max_w, 0, MAXL - 1, top);  // every level any call can build fits
  d.pcap = top.off[top.nl - 1] + top.h[top.nl - 1] * top.w[top.nl - 1];
  const size_t ns = (size_t)n_streams, planes = ns * d.cap;
  auto fail = [&](hipError_t e) {
    bx_sof_destroy(H_);
    return sf_err(BX_ERR_HIP, hipGetErrorString(e));
  };
  hipError_t e;
  auto alloc0 = [&](void** p, size_t bytes) {
    if ((e = hipMalloc(p, bytes)) != hipSuccess) return false;
    return (e = hipMemset(*p, 0, bytes)) == hipSuccess;
  };
  if (!alloc0((void**)&d.pyr, ns * 2 * d.pcap)) return fail(e);
  if (!alloc0((void**)&d.lam, planes * 8)) return fail(e);
  if (!alloc0((void**)&d.lmax, ns * 8)) return fail(e);
  if (!alloc0((void**)&d.ckey, planes * 8)) return fail(e);
  if (!alloc0((void**)&d.cidx, planes * 4)) return fail(e);
  if (!alloc0((void**)&d.kp, ns * MAXC * 16)) return fail(e);
  if (!alloc0((void**)&d.rprev, ns * MAXC * 16)) return fail(e);
  if (!alloc0((void**)&d.rnext, ns * MAXC * 16)) return fail(e);
  if (!alloc0((void**)&d.riter, ns * MAXC * 4)) return fail(e);
  if (!alloc0((void**)&d.rok, ns * MAXC)) return fail(e);
  if (!alloc0((void**)&d.rinl, ns * MAXC)) return fail(e);
  if (!alloc0((void**)&d.has_prev, ns * 8 * 4 + 4)) return fail(e);
  d.ph = d.has_prev + ns;
  d.pw = d.ph + ns;
  d.pnl = d.pw + ns;
  d.par = d.pnl + ns;
  d.nkp = d.par + ns;
  d.rn = d.nkp + ns;
  d.rwin = d.rn + ns;
  d.status = d.rwin + ns;
  if (!alloc0((void**)&H_->sstreams, ns * 4)) return fail(e);
  if (!alloc0((void**)&H_->swarps, ns * 48)) return fail(e);
  if (!alloc0((void**)&H_->sints, ns * 16)) return fail(e);
  *out = H_;
  return BX_OK;
}

int bx_sof_destroy(void* h) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_) return BX_OK;
  SofDev& d = H_->d;
  void* ps[] = {d.pyr, d.lam, d.lmax, d.ckey, d.cidx, d.kp, d.rprev, d.rnext, d.riter, d.rok,
                d.rinl, d.has_prev, H_->sframes, H_->sstreams, H_->swarps, H_->sints};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  free_chain(H_);
  delete H_;
  return BX_OK;
}

int bx_sof_reset(void* h, int stream, void* hip_stream) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_) return sf_err(BX_ERR_INVALID, "null sof handle");
  if (stream >= H_->d.n_streams) return sf_err(BX_ERR_INVALID, "stream index out of range");
  hipStream_t st = (hipStream_t)hip_stream;
  if (stream < 0)
    BX_HIPCHK(hipMemsetAsync(H_->d.has_prev, 0, (size_t)H_->d.n_streams * 4, st));
  else
    BX_HIPCHK(hipMemsetAsync(H_->d.has_prev + stream, 0, 4, st));
  return BX_OK;
}

int bx_sof_apply(void* h, int n, int H, int W, int channels, const uint8_t* frames,
                 const int32_t* streams, const bx_sof_params* params, double* warps,
                 int32_t* code, int32_t* n_keypoints, int32_t* n_tracked, int32_t* n_inliers,
                 void* hip_stream) {
  SofHandle* H_ = (SofHandle*)h;
  Lv lv;
  int rc = check_args(H_, n, H, W, channels, params, &lv);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames || !streams || !warps || !code || !n_keypoints || !n_tracked || !n_inliers)
    return sf_err(BX_ERR_INVALID, "null argument");
  return launch(H_, n, H, W, channels, frames, streams, *params, lv, warps, code, n_keypoints,
                n_tracked, n_inliers, (hipStream_t)hip_stream);
}

int bx_sof_apply_host(void* h, int n, int H, int W, int channels, const uint8_t* frames_host,
                      const int32_t* streams_host, const bx_sof_params* params,
                      double* warps_host, int32_t* code_host, int32_t* n_keypoints_host,
                      int32_t* n_tracked_host, int32_t* n_inliers_host, void* hip_stream) {
  SofHandle* H_ = (SofHandle*)h;
  Lv lv;
  int rc = check_args(H_, n, H, W, channels, params, &lv);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames_host || !streams_host || !warps_host || !code_host || !n_keypoints_host ||
      !n_tracked_host || !n_inliers_host)
    return sf_err(BX_ERR_INVALID, "null argument");
  const int S = H_->d.n_streams;
  std::vector<char> seen(S, 0);
  for (int k = 0; k < n; k++) {
    const int s = streams_host[k];
    if (s < 0 || s >= S) return sf_err(BX_ERR_INVALID, "stream index out of range");
    if (seen[s]) return sf_err(BX_ERR_INVALID, "a stream is listed twice");
    seen[s] = 1;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t fb = (size_t)n * H * W * channels;
  if (fb > H_->sframes_bytes) {
    BX_HIPCHK(hipStreamSynchronize(st));
    if (H_->sframes) (void)hipFree(H_->sframes);
    H_->sframes = nullptr;
    H_->sframes_bytes = 0;
    BX_HIPCHK(hipMalloc(&H_->sframes, fb));
    H_->sframes_bytes = fb;
  }
  BX_HIPCHK(hipMemcpyAsync(H_->sframes, frames_host, fb, hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipMemcpyAsync(H_->sstreams, streams_host, (size_t)n * 4, hipMemcpyHostToDevice, st));
  int32_t* si = H_->sints;
  rc = launch(H_, n, H, W, channels, H_->sframes, H_->sstreams, *params, lv, H_->swarps, si,
              si + S, si + 2 * S, si + 3 * S, st);
  if (rc != BX_OK) return rc;
  std::vector<double> wv((size_t)S * 6);
  std::vector<int32_t> iv((size_t)S * 4);
  BX_HIPCHK(hipMemcpyAsync(wv.data(), H_->swarps, (size_t)S * 48, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(iv.data(), si, (size_t)S * 16, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < n; k++) {
    const int s = streams_host[k];
    for (int q = 0; q < 6; q++) warps_host[(size_t)s * 6 + q] = wv[(size_t)s * 6 + q];
    code_host[s] = iv[s];
    n_keypoints_host[s] = iv[(size_t)S + s];
    n_tracked_host[s] = iv[(size_t)2 * S + s];
    n_inliers_host[s] = iv[(size_t)3 * S + s];
  }
  return BX_OK;
}

int bx_sof_chain_reserve(void* h, int max_frames) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_) return sf_err(BX_ERR_INVALID, "null sof handle");
  const SofDev& d = H_->d;
  const size_t cap = (size_t)d.cap, pcap = (size_t)d.pcap;
  if (max_frames < 1 || max_frames > BX_SOF_MAX_STREAMS ||
      (long long)max_frames * (long long)(pcap + cap * 20) > (1LL << 36))
    return sf_err(BX_ERR_INVALID, "max_frames out of range");
  if (max_frames <= H_->c.max_frames) return BX_OK;
  // grown: the slots hold nothing between calls, so the old ones are dropped once the device
  // has finished with them
  BX_HIPCHK(hipDeviceSynchronize());
  free_chain(H_);
  SofChain& c = H_->c;
  const size_t m = (size_t)max_frames;
  void** ps[] = {(void**)&c.pyr,   (void**)&c.lam,   (void**)&c.lmax,  (void**)&c.ckey,
                 (void**)&c.cidx,  (void**)&c.kp,    (void**)&c.rprev, (void**)&c.rnext,
                 (void**)&c.riter, (void**)&c.rok,   (void**)&c.rinl,  (void**)&c.nkp,
                 (void**)&H_->cstreams, (void**)&H_->cwarps, (void**)&H_->cints};
  const size_t bytes[] = {m * pcap,      m * cap * 8,   m * 8,         m * cap * 8,
                          m * cap * 4,   m * MAXC * 16, m * MAXC * 16, m * MAXC * 16,
                          m * MAXC * 4,  m * MAXC,      m * MAXC,      m * 5 * 4,
                          m * 4,         m * 48,        m * 16};
  for (int q = 0; q < 15; q++) {
    hipError_t e = hipMalloc(ps[q], bytes[q]);
    if (e != hipSuccess) {
      free_chain(H_);
      return sf_err(BX_ERR_HIP, hipGetErrorString(e));
    }
  }
  c.rn = c.nkp + m;
  c.rwin = c.rn + m;
  c.plan = c.rwin + m;
  c.topar = c.plan + m;
  c.max_frames = max_frames;
  return BX_OK;
}

int bx_sof_apply_chain(void* h, int n, int H, int W, int channels, const uint8_t* frames,
                       const int32_t* streams, const int64_t* dst, const bx_sof_params* params,
                       double* warps, int32_t* code, int32_t* n_keypoints, int32_t* n_tracked,
                       int32_t* n_inliers, void* hip_stream) {
  SofHandle* H_ = (SofHandle*)h;
  Lv lv;
  int rc = check_chain_args(H_, n, H, W, channels, params, &lv);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames || !streams || !warps || !code || !n_keypoints || !n_tracked || !n_inliers)
    return sf_err(BX_ERR_INVALID, "null argument");
  return launch_chain(H_, n, H, W, channels, frames, streams, dst, *params, lv, warps, code,
                      n_keypoints, n_tracked, n_inliers, (hipStream_t)hip_stream);
}

int bx_sof_apply_chain_host(void* h, int n, int H, int W, int channels,
                            const uint8_t* frames_host, const int32_t* streams_host,
                            const bx_sof_params* params, double* warps_host, int32_t* code_host,
                            int32_t* n_keypoints_host, int32_t* n_tracked_host,
                            int32_t* n_inliers_host, void* hip_stream) {
  SofHandle* H_ = (SofHandle*)h;
  Lv lv;
  int rc = check_chain_args(H_, n, H, W, channels, params, &lv);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames_host || !streams_host || !warps_host || !code_host || !n_keypoints_host ||
      !n_tracked_host || !n_inliers_host)
    return sf_err(BX_ERR_INVALID, "null argument");
  const int S = H_->d.n_streams;
  std::vector<char> seen(S, 0);
  for (int k = 0; k < n; k++) {
    const int s = streams_host[k];
    if (s < 0 || s >= S) return sf_err(BX_ERR_INVALID, "stream index out of range");
    if (seen[s] && streams_host[k - 1] != s)
      return sf_err(BX_ERR_INVALID, "the frames of a stream are not adjacent");
    seen[s] = 1;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t fb = (size_t)n * H * W * channels;
  if (fb > H_->sframes_bytes) {
    BX_HIPCHK(hipStreamSynchronize(st));
    if (H_->sframes) (void)hipFree(H_->sframes);
    H_->sframes = nullptr;
    H_->sframes_bytes = 0;
    BX_HIPCHK(hipMalloc(&H_->sframes, fb));
    H_->sframes_bytes = fb;
  }
  BX_HIPCHK(hipMemcpyAsync(H_->sframes, frames_host, fb, hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipMemcpyAsync(H_->cstreams, streams_host, (size_t)n * 4, hipMemcpyHostToDevice, st));
  const size_t m = (size_t)H_->c.max_frames;
  int32_t* ci = H_->cints;
  rc = launch_chain(H_, n, H, W, channels, H_->sframes, H_->cstreams, nullptr, *params, lv,
                    H_->cwarps, ci, ci + m, ci + 2 * m, ci + 3 * m, st);
  if (rc != BX_OK) return rc;
  BX_HIPCHK(hipMemcpyAsync(warps_host, H_->cwarps, (size_t)n * 48, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(code_host, ci, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(n_keypoints_host, ci + m, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(n_tracked_host, ci + 2 * m, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(n_inliers_host, ci + 3 * m, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  return BX_OK;
}

int bx_sof_status(void* h, int* status) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_ || !status) return sf_err(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(status, H_->d.status, 4, hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_sof_pyramid_bytes(void* h, size_t* bytes) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_ || !bytes) return sf_err(BX_ERR_INVALID, "null argument");
  *bytes = (size_t)H_->d.pcap;
  return BX_OK;
}

int bx_sof_state_host(void* h, int stream, int* has_prev, int* n_levels, int* lh, int* lw,
                      uint8_t* pyramid, int* n_keypoints, double* keypoints, double* lam) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_ || !has_prev || !n_levels || !lh || !lw) return sf_err(BX_ERR_INVALID, "null argument");
  const SofDev& d = H_->d;
  if (stream < 0 || stream >= d.n_streams) return sf_err(BX_ERR_INVALID, "stream index out of range");
  BX_HIPCHK(hipDeviceSynchronize());
  int ph = 0, pw = 0, pnl = 0, par = 0;
  BX_HIPCHK(hipMemcpy(has_prev, d.has_prev + stream, 4, hipMemcpyDeviceToHost));
  BX_HIPCHK(hipMemcpy(&ph, d.ph + stream, 4, hipMemcpyDeviceToHost));
  BX_HIPCHK(hipMemcpy(&pw, d.pw + stream, 4, hipMemcpyDeviceToHost));
  BX_HIPCHK(hipMemcpy(&pnl, d.pnl + stream, 4, hipMemcpyDeviceToHost));
  BX_HIPCHK(hipMemcpy(&par, d.par + stream, 4, hipMemcpyDeviceToHost));
  *n_levels = *has_prev ? pnl : 0;
  for (int l = 0; l < MAXL; l++) {
    lh[l] = lw[l] = 0;
    if (*has_prev && l < pnl) {
      lh[l] = l == 0 ? ph : (lh[l - 1] + 1) / 2;
      lw[l] = l == 0 ? pw : (lw[l - 1] + 1) / 2;
    }
  }
  if (pyramid)
    BX_HIPCHK(hipMemcpy(pyramid, d.pyr + ((size_t)stream * 2 + (par & 1)) * d.pcap, d.pcap,
                        hipMemcpyDeviceToHost));
  if (n_keypoints) BX_HIPCHK(hipMemcpy(n_keypoints, d.nkp + stream, 4, hipMemcpyDeviceToHost));
  if (keypoints)
    BX_HIPCHK(hipMemcpy(keypoints, d.kp + (size_t)stream * MAXC * 2, (size_t)MAXC * 16,
                        hipMemcpyDeviceToHost));
  if (lam)
    BX_HIPCHK(hipMemcpy(lam, d.lam + (size_t)stream * d.cap, (size_t)d.cap * 8,
                        hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_sof_points_host(void* h, int stream, int* n, double* prev, double* next, uint8_t* tracked,
                       int32_t* iterations, uint8_t* inlier, int* winner) {
  SofHandle* H_ = (SofHandle*)h;
  if (!H_ || !n) return sf_err(BX_ERR_INVALID, "null argument");
  const SofDev& d = H_->d;
  if (stream < 0 || stream >= d.n_streams) return sf_err(BX_ERR_INVALID, "stream index out of range");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(n, d.rn + stream, 4, hipMemcpyDeviceToHost));
  const size_t o = (size_t)stream * MAXC;
  if (prev) BX_HIPCHK(hipMemcpy(prev, d.rprev + 2 * o, (size_t)MAXC * 16, hipMemcpyDeviceToHost));
  if (next) BX_HIPCHK(hipMemcpy(next, d.rnext + 2 * o, (size_t)MAXC * 16, hipMemcpyDeviceToHost));
  if (tracked) BX_HIPCHK(hipMemcpy(tracked, d.rok + o, MAXC, hipMemcpyDeviceToHost));
  if (iterations)
    BX_HIPCHK(hipMemcpy(iterations, d.riter + o, (size_t)MAXC * 4, hipMemcpyDeviceToHost));
  if (inlier) BX_HIPCHK(hipMemcpy(inlier, d.rinl + o, MAXC, hipMemcpyDeviceToHost));
  if (winner) BX_HIPCHK(hipMemcpy(winner, d.rwin + stream, 4, hipMemcpyDeviceToHost));
  return BX_OK;
}

}  // extern "C"
