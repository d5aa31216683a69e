// bx_cmc.hip — camera-motion compensation (include/bxcmc.h): the ECC alignment of every frame
// to its stream's previous frame, the stage motion/cmc/ecc.py hands to cv2.findTransformECC.
// The contract is DESIGN.md 2.14; this file is its device form.
//
// Two launches per step, both on the caller's stream:
//   cmc_prep_kernel  one thread per working pixel of every frame: BGR -> grey, the fixed-point
//                    bilinear resize (integer arithmetic, exact) and the central-difference
//                    gradients of the resized image (each thread recomputes its four neighbours:
//                    the image is small, a second launch would cost more)
//   cmc_ecc_kernel   one persistent workgroup of 1024 threads per stream; the whole iteration
//                    loop runs inside: a pass over the template pixels accumulating the raw
//                    moments in fp64, a fixed-order reduction (DPP butterfly per wave, the 16
//                    waves in ascending order through LDS), then thread 0 finishes the iteration
//                    (correlation, Cholesky, lambda, parameter update) and publishes the new warp
//                    through LDS.  No host round trip, no device-wide barrier.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/bxassoc.h"
#include "../../include/bxcmc.h"
#include "bx_device.h"
#include "bx_cmcprep.h"
#include "bx_host.h"


using namespace bx;

namespace {

int cm_err(int code, const std::string& msg) { return bx_record_error(code, msg.c_str()); }
constexpr int ET = BX_ECC_THREADS, EW = ET / WAVE;  // 1024 threads = 16 waves
constexpr int PT = 256;                              // threads of a prep workgroup

// Everything the kernels read or write.
struct CmDev {
  int n_streams, cap;         // cap = max_h * max_w: stride of the per-stream planes
  uint8_t *prev, *cur;        // [n_streams][cap] previous / new grey image at working scale
  float *curf, *gx, *gy;      // [n_streams][cap] the new image as float, its gradients
  int *has_prev, *ph, *pw;    // [n_streams] state: previous image present, its size
  int* status;                // latched BX_ERR_*
};

// Scratch of the chained apply (bx_ecc_chain_reserve): one slot per frame of a call, each the
// planes a stream has for its new image, with the same cap stride.
struct CmChain {
  int max_frames;
  uint8_t* grey;         // [max_frames][cap]
  float *curf, *gx, *gy;  // [max_frames][cap]
};

struct CmHandle {
  CmDev d{};
  CmChain c{};
  int max_h = 0, max_w = 0;
  // staging of the chained host entry ([max_frames] each, grown with the slots)
  int32_t* cstreams = nullptr;
  double *cwarps = nullptr, *crho = nullptr;
  int32_t *citers = nullptr, *ccode = nullptr;
  // staging of the host entry (grown to the largest call)
  uint8_t* sframes = nullptr;
  size_t sframes_bytes = 0;
  int32_t* sstreams = nullptr;
  double *sinit = nullptr, *swarps = nullptr, *srho = nullptr;
  int32_t *siters = nullptr, *scode = nullptr;
};

// ------------------------------------------------------------------------------------------
// preprocessing (PrepArgs, grey_at, work_pixel and reflect101, the grey and resize rule, live in
// bx_cmcprep.h: the sparse optical flow shares them)
__global__ __launch_bounds__(PT) void cmc_prep_kernel(CmDev d, PrepArgs a) {
  const int k = blockIdx.y;
  const int s = a.streams[k];
  if (s < 0 || s >= d.n_streams) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicMax(d.status, (int)BX_ERR_INVALID);
    return;
  }
  const int idx = blockIdx.x * PT + threadIdx.x;
  if (idx >= a.h * a.w) return;
  const int x = idx % a.w, y = idx / a.w;
  const uint8_t* f = a.frames + (size_t)k * a.H * a.W * a.ch;
  const unsigned c = work_pixel(a, f, x, y);
  const int xl = reflect101(x - 1, a.w), xr = reflect101(x + 1, a.w);
  const int yu = reflect101(y - 1, a.h), yd = reflect101(y + 1, a.h);
  const float l = (float)work_pixel(a, f, xl, y), r = (float)work_pixel(a, f, xr, y);
  const float u = (float)work_pixel(a, f, x, yu), dn = (float)work_pixel(a, f, x, yd);
  const size_t o = (size_t)s * d.cap + idx;
  d.cur[o] = (uint8_t)c;
  d.curf[o] = (float)c;
  d.gx[o] = 0.5f * (r - l);
  d.gy[o] = 0.5f * (dn - u);
}

// ------------------------------------------------------------------------------------------
// the solve
struct EccArgs {
  const int32_t* streams;
  const double* init;  // [n_streams][6] or null
  int h, w, max_iter;
  double eps, scale;
  double *warps, *rho;
  int32_t *iters, *code;
};

template <int MODE>
struct Model {
  static constexpr int K = MODE == BX_ECC_TRANSLATION ? 2 : MODE == BX_ECC_EUCLIDEAN ? 3 : 6;
  static constexpr int NS = 6 + 3 * K + K * (K + 1) / 2;  // 15, 21, 45 sums
};

enum { CTL_RUN = 0, CTL_DONE = 1, CTL_FAIL = 2, CTL_FIRST = 3, CTL_SKIP = 4 };

// zero-border read of a float plane
__device__ __forceinline__ double tap(const float* p, int w, int h, int x, int y) {
  return (x >= 0 && x < w && y >= 0 && y < h) ? (double)p[(size_t)y * w + x] : 0.0;
}

// Thread 0's end of an iteration, from the reduced sums S (layout: n, SI, SII, ST, STT, SIT,
// SJ[K], SJI[K], SJT[K], SJJ[j <= k packed by k]).  m: the warp (6) and the angle (m[6]).
// Returns false on the not-converged exits; *rho_out is set either way.
template <int MODE>
__device__ inline bool ecc_finish(const double* S, double* m, double* rho_out) {
  constexpr int K = Model<MODE>::K;
  const double n = S[0];
  const double mI = S[1] / n, mT = S[3] / n;
  const double nI2 = S[2] - S[1] * S[1] / n;  // |I_zm|^2
  const double nT2 = S[4] - S[3] * S[3] / n;  // |T_zm|^2
  const double corr = S[5] - S[1] * S[3] / n;
  const double rho = corr / (sqrt(nI2) * sqrt(nT2));
  *rho_out = rho;
  if (rho != rho) return false;
  double ip[K], tp[K], L[K][K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    ip[k] = S[6 + K + k] - mI * S[6 + k];      // J^T I_zm
    tp[k] = S[6 + 2 * K + k] - mT * S[6 + k];  // J^T T_zm
  }
  // Cholesky H = L L^T of the packed Hessian (entry (j, k), j <= k, at k (k + 1) / 2 + j)
  const double* Hs = S + 6 + 3 * K;
#pragma unroll
  for (int j = 0; j < K; j++) {
    double dg = Hs[j * (j + 1) / 2 + j];
#pragma unroll
    for (int q = 0; q < j; q++) dg -= L[j][q] * L[j][q];
    if (!(dg > 0.0)) return false;
    dg = sqrt(dg);
    L[j][j] = dg;
#pragma unroll
    for (int i = j + 1; i < K; i++) {
      double s = Hs[i * (i + 1) / 2 + j];
#pragma unroll
      for (int q = 0; q < j; q++) s -= L[i][q] * L[j][q];
      L[i][j] = s / dg;
    }
  }
  auto solve = [&](const double* b, double* x) {
    double y[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
      double s = b[i];
#pragma unroll
      for (int q = 0; q < i; q++) s -= L[i][q] * y[q];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = K - 1; i >= 0; i--) {
      double s = y[i];
#pragma unroll
      for (int q = i + 1; q < K; q++) s -= L[q][i] * x[q];
      x[i] = s / L[i][i];
    }
  };
  double hi[K];  // H^-1 i
  solve(ip, hi);
  double ihi = 0.0, thi = 0.0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    ihi += ip[k] * hi[k];
    thi += tp[k] * hi[k];
  }
  const double ln = nI2 - ihi, ld = corr - thi;
  if (!(ld > 0.0)) return false;
  const double lam = ln / ld;
  double e[K], dp[K];
#pragma unroll
  for (int k = 0; k < K; k++) e[k] = lam * tp[k] - ip[k];  // J^T (lambda T_zm - I_zm)
  solve(e, dp);
  if (MODE == BX_ECC_TRANSLATION) {
    m[2] += dp[0];
    m[5] += dp[1];
  } else if (MODE == BX_ECC_EUCLIDEAN) {
    m[6] += dp[0];
    m[2] += dp[1];
    m[5] += dp[2];
    const double c = cos(m[6]), s = sin(m[6]);
    m[0] = c;
    m[1] = -s;
    m[3] = s;
    m[4] = c;
  } else {
    m[0] += dp[0];
    m[3] += dp[1];
    m[1] += dp[2];
    m[4] += dp[3];
    m[2] += dp[4];
    m[5] += dp[5];
  }
  return true;
}

// One pass over the template pixels and its reduction into tot[].  PART 0: every sum; PART 1:
// all but the Hessian's; PART 2: the Hessian's alone (the affine model runs 1 then 2: its 45
// accumulators do not fit the 128 registers a thread of a 1024-thread workgroup has).
template <int MODE, int PART>
__device__ __forceinline__ void ecc_pass(const uint8_t* T, const float* I, const float* GX,
                                         const float* GY, int w, int h, const double* sm,
                                         double* red, double* tot) {
  constexpr int K = Model<MODE>::K, NB = 6 + 3 * K, NH = K * (K + 1) / 2;
  constexpr int NP = PART == 0 ? NB + NH : PART == 1 ? NB : NH;  // sums of this pass
  constexpr int OFF = PART == 2 ? NB : 0;                        // its first slot in tot[]
  constexpr int HO = PART == 2 ? 0 : NB;                         // the Hessian's slot in acc[]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, npix = h * w;
  const double m00 = sm[0], m01 = sm[1], m02 = sm[2], m10 = sm[3], m11 = sm[4], m12 = sm[5];
  double acc[NP];
#pragma unroll
  for (int q = 0; q < NP; q++) acc[q] = 0.0;
  for (int idx = tid; idx < npix; idx += ET) {
    const int y = idx / w, x = idx - y * w;
    const double xd = (double)x, yd = (double)y;
    const double xs = (m00 * xd + m01 * yd) + m02;
    const double ys = (m10 * xd + m11 * yd) + m12;
    // nearest source pixel floor(v + 0.5) inside the image (false for a NaN coordinate)
    const bool in = xs + 0.5 >= 0.0 && xs + 0.5 < (double)w && ys + 0.5 >= 0.0 &&
                    ys + 0.5 < (double)h;
    if (!in) continue;
    const double fx = floor(xs), fy = floor(ys);
    const double ax = xs - fx, ay = ys - fy;
    const int x0 = (int)fx, y0 = (int)fy;  // in [-1, w - 1] x [-1, h - 1]
    const double w00 = (1.0 - ax) * (1.0 - ay), w01 = ax * (1.0 - ay);
    const double w10 = (1.0 - ax) * ay, w11 = ax * ay;
    const double gxv = ((w00 * tap(GX, w, h, x0, y0) + w01 * tap(GX, w, h, x0 + 1, y0)) +
                        w10 * tap(GX, w, h, x0, y0 + 1)) + w11 * tap(GX, w, h, x0 + 1, y0 + 1);
    const double gyv = ((w00 * tap(GY, w, h, x0, y0) + w01 * tap(GY, w, h, x0 + 1, y0)) +
                        w10 * tap(GY, w, h, x0, y0 + 1)) + w11 * tap(GY, w, h, x0 + 1, y0 + 1);
    double J[K];
    if (MODE == BX_ECC_TRANSLATION) {
      J[0] = gxv;
      J[1] = gyv;
    } else if (MODE == BX_ECC_EUCLIDEAN) {
      const double cs = m00, sn = m10;
      const double hx = -(xd * sn) - yd * cs, hy = xd * cs - yd * sn;
      J[0] = gxv * hx + gyv * hy;
      J[1] = gxv;
      J[2] = gyv;
    } else {
      J[0] = gxv * xd;
      J[1] = gyv * xd;
      J[2] = gxv * yd;
      J[3] = gyv * yd;
      J[4] = gxv;
      J[5] = gyv;
    }
    if (PART != 2) {
      const double iv = ((w00 * tap(I, w, h, x0, y0) + w01 * tap(I, w, h, x0 + 1, y0)) +
                         w10 * tap(I, w, h, x0, y0 + 1)) + w11 * tap(I, w, h, x0 + 1, y0 + 1);
      const double tv = (double)T[idx];
      acc[0] += 1.0;
      acc[1] += iv;
      acc[2] += iv * iv;
      acc[3] += tv;
      acc[4] += tv * tv;
      acc[5] += iv * tv;
#pragma unroll
      for (int k = 0; k < K; k++) {
        acc[6 + k] += J[k];
        acc[6 + K + k] += J[k] * iv;
        acc[6 + 2 * K + k] += J[k] * tv;
      }
    }
    if (PART != 1) {
#pragma unroll
      for (int k = 0; k < K; k++)
#pragma unroll
        for (int j = 0; j <= k; j++) acc[HO + k * (k + 1) / 2 + j] += J[j] * J[k];
    }
  }
  // fixed-order reduction: butterfly within the wave, then the waves in ascending order
#pragma unroll
  for (int q = 0; q < NP; q++) {
    const double v = wave_bfly_desc_f64(acc[q]);
    if (lane == 0) red[wv * NP + q] = v;
  }
  __syncthreads();
  if (tid < NP) {
    double sum = 0.0;
    for (int k = 0; k < EW; k++) sum += red[k * NP + tid];
    tot[OFF + tid] = sum;
  }
  __syncthreads();
}

template <int MODE>
__global__ __launch_bounds__(ET) void cmc_ecc_kernel(CmDev d, EccArgs a) {
  constexpr int K = Model<MODE>::K, NS = Model<MODE>::NS;
  constexpr int NR = MODE == BX_ECC_AFFINE ? 6 + 3 * K : NS;  // sums of the largest pass
  __shared__ double red[EW * NR];
  __shared__ double tot[NS];
  __shared__ double sm[8];  // warp (6), angle
  __shared__ int ctl;
  const int tid = threadIdx.x;
  const int s = a.streams[blockIdx.x];
  if (s < 0 || s >= d.n_streams) return;  // (latched by the prep kernel)
  const int w = a.w, h = a.h, npix = h * w;
  const size_t base = (size_t)s * d.cap;
  const uint8_t* T = d.prev + base;
  const float *I = d.curf + base, *GX = d.gx + base, *GY = d.gy + base;

  // thread 0's loop state
  double rho = -1.0, last_rho = -a.eps;
  int it = 0;
  if (tid == 0) {
    for (int q = 0; q < 6; q++)
      sm[q] = a.init ? a.init[(size_t)s * 6 + q] : (q == 0 || q == 4 ? 1.0 : 0.0);
    sm[6] = asin(sm[3]);
    int c;
    if (!d.has_prev[s]) {
      c = CTL_FIRST;
    } else if (d.ph[s] != h || d.pw[s] != w) {
      atomicMax(d.status, (int)BX_ERR_SHAPE);
      c = CTL_FIRST;
    } else {
      c = (1 <= a.max_iter && fabs(rho - last_rho) >= a.eps) ? CTL_RUN : CTL_DONE;
    }
    ctl = c;
  }
  __syncthreads();
  int c = ctl;
  while (c == CTL_RUN) {
    if (MODE == BX_ECC_AFFINE) {
      ecc_pass<MODE, 1>(T, I, GX, GY, w, h, sm, red, tot);
      ecc_pass<MODE, 2>(T, I, GX, GY, w, h, sm, red, tot);
    } else {
      ecc_pass<MODE, 0>(T, I, GX, GY, w, h, sm, red, tot);
    }
    if (tid == 0) {
      double S[NS], m[7];
#pragma unroll
      for (int q = 0; q < NS; q++) S[q] = tot[q];
#pragma unroll
      for (int q = 0; q < 7; q++) m[q] = sm[q];
      last_rho = rho;
      it++;
      if (!ecc_finish<MODE>(S, m, &rho)) {
        ctl = CTL_FAIL;
      } else {
#pragma unroll
        for (int q = 0; q < 7; q++) sm[q] = m[q];
        ctl = (it + 1 <= a.max_iter && fabs(rho - last_rho) >= a.eps) ? CTL_RUN : CTL_DONE;
      }
    }
    __syncthreads();
    c = ctl;
  }
  if (tid == 0) {
    double o[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (c == CTL_DONE) {
      for (int q = 0; q < 6; q++) o[q] = sm[q];
      if (a.scale > 0.0 && a.scale < 1.0) {
        o[2] = o[2] / a.scale;
        o[5] = o[5] / a.scale;
      }
    }
    for (int q = 0; q < 6; q++) a.warps[(size_t)s * 6 + q] = o[q];
    a.rho[s] = c == CTL_FIRST ? 0.0 : rho;
    a.iters[s] = it;
    a.code[s] = c == CTL_DONE ? BX_ECC_OK : c == CTL_FIRST ? BX_ECC_FIRST_FRAME : BX_ECC_NOT_CONVERGED;
    d.has_prev[s] = 1;
    d.ph[s] = h;
    d.pw[s] = w;
  }
  // the new image becomes the previous one (every read of T is behind the loop's barriers)
  uint8_t* P = d.prev + base;
  const uint8_t* C = d.cur + base;
  for (int idx = tid; idx < npix; idx += ET) P[idx] = C[idx];
}

// ------------------------------------------------------------------------------------------
// the chained apply: n frames per call, frame i aligned to frame i - 1 of the
// call when both are of one stream, else to the stream's stored previous image.  Three launches:
//   cmc_chain_prep_kernel      cmc_prep_kernel writing slot i instead of the stream's planes
//   cmc_ecc_chain_kernel       cmc_ecc_kernel reading its template from slot i - 1 or d.prev and
//                              its image from slot i; it writes results only, never the state
//   cmc_chain_handover_kernel  the last frame of every stream becomes that stream's state.  It
//                              is a launch of its own because the workgroup of a stream's first
//                              frame reads d.prev for its whole loop: no workgroup of the solve
//                              may write it.
__global__ __launch_bounds__(PT) void cmc_chain_prep_kernel(CmDev d, CmChain c, PrepArgs a) {
  const int k = blockIdx.y;
  const int s = a.streams[k];
  if (s < 0 || s >= d.n_streams) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicMax(d.status, (int)BX_ERR_INVALID);
    return;
  }
  const int idx = blockIdx.x * PT + threadIdx.x;
  if (idx >= a.h * a.w) return;
  const int x = idx % a.w, y = idx / a.w;
  const uint8_t* f = a.frames + (size_t)k * a.H * a.W * a.ch;
  const unsigned g = work_pixel(a, f, x, y);
  const int xl = reflect101(x - 1, a.w), xr = reflect101(x + 1, a.w);
  const int yu = reflect101(y - 1, a.h), yd = reflect101(y + 1, a.h);
  const float l = (float)work_pixel(a, f, xl, y), r = (float)work_pixel(a, f, xr, y);
  const float u = (float)work_pixel(a, f, x, yu), dn = (float)work_pixel(a, f, x, yd);
  const size_t o = (size_t)k * d.cap + idx;
  c.grey[o] = (uint8_t)g;
  c.curf[o] = (float)g;
  c.gx[o] = 0.5f * (r - l);
  c.gy[o] = 0.5f * (dn - u);
}

struct ChainArgs {
  const int32_t* streams;  // [n]
  const int64_t* dst;      // [n] result row of each frame, or null: row i
  int h, w, max_iter;
  double eps, scale;
  double *warps, *rho;
  int32_t *iters, *code;
};

template <int MODE>
__global__ __launch_bounds__(ET) void cmc_ecc_chain_kernel(CmDev d, CmChain ch, ChainArgs a) {
  constexpr int K = Model<MODE>::K, NS = Model<MODE>::NS;
  constexpr int NR = MODE == BX_ECC_AFFINE ? 6 + 3 * K : NS;  // sums of the largest pass
  __shared__ double red[EW * NR];
  __shared__ double tot[NS];
  __shared__ double sm[8];  // warp (6), angle
  __shared__ int ctl;
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  const int s = a.streams[i];
  if (s < 0 || s >= d.n_streams) return;  // (latched by the prep kernel)
  const bool chained = i > 0 && a.streams[i - 1] == s;
  const int w = a.w, h = a.h;
  const size_t base = (size_t)i * d.cap;
  const uint8_t* T = chained ? ch.grey + (size_t)(i - 1) * d.cap : d.prev + (size_t)s * d.cap;
  const float *I = ch.curf + base, *GX = ch.gx + base, *GY = ch.gy + base;

  // thread 0's loop state
  double rho = -1.0, last_rho = -a.eps;
  int it = 0;
  if (tid == 0) {
    for (int q = 0; q < 6; q++) sm[q] = (q == 0 || q == 4) ? 1.0 : 0.0;
    sm[6] = asin(sm[3]);
    int c;
    if (!chained && !d.has_prev[s]) {
      c = CTL_FIRST;
    } else if (!chained && (d.ph[s] != h || d.pw[s] != w)) {
      atomicMax(d.status, (int)BX_ERR_SHAPE);
      c = CTL_FIRST;
    } else {
      c = (1 <= a.max_iter && fabs(rho - last_rho) >= a.eps) ? CTL_RUN : CTL_DONE;
    }
    ctl = c;
  }
  __syncthreads();
  int c = ctl;
  while (c == CTL_RUN) {
    if (MODE == BX_ECC_AFFINE) {
      ecc_pass<MODE, 1>(T, I, GX, GY, w, h, sm, red, tot);
      ecc_pass<MODE, 2>(T, I, GX, GY, w, h, sm, red, tot);
    } else {
      ecc_pass<MODE, 0>(T, I, GX, GY, w, h, sm, red, tot);
    }
    if (tid == 0) {
      double S[NS], m[7];
#pragma unroll
      for (int q = 0; q < NS; q++) S[q] = tot[q];
#pragma unroll
      for (int q = 0; q < 7; q++) m[q] = sm[q];
      last_rho = rho;
      it++;
      if (!ecc_finish<MODE>(S, m, &rho)) {
        ctl = CTL_FAIL;
      } else {
#pragma unroll
        for (int q = 0; q < 7; q++) sm[q] = m[q];
        ctl = (it + 1 <= a.max_iter && fabs(rho - last_rho) >= a.eps) ? CTL_RUN : CTL_DONE;
      }
    }
    __syncthreads();
    c = ctl;
  }
  if (tid == 0) {
    double o[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (c == CTL_DONE) {
      for (int q = 0; q < 6; q++) o[q] = sm[q];
      if (a.scale > 0.0 && a.scale < 1.0) {
        o[2] = o[2] / a.scale;
        o[5] = o[5] / a.scale;
      }
    }
    const size_t r = a.dst ? (size_t)a.dst[i] : (size_t)i;
    for (int q = 0; q < 6; q++) a.warps[r * 6 + q] = o[q];
    a.rho[r] = c == CTL_FIRST ? 0.0 : rho;
    a.iters[r] = it;
    a.code[r] = c == CTL_DONE ? BX_ECC_OK : c == CTL_FIRST ? BX_ECC_FIRST_FRAME : BX_ECC_NOT_CONVERGED;
  }
}

// The last frame of each stream's group: its grey image and gradients become the stream's, as
// after a plain apply of that frame (d.cur / d.curf are scratch of the plain apply, rewritten by
// its prep kernel before anything reads them).
__global__ __launch_bounds__(PT) void cmc_chain_handover_kernel(CmDev d, CmChain c,
                                                                const int32_t* streams, int n,
                                                                int h, int w) {
  const int k = blockIdx.y;
  const int s = streams[k];
  if (s < 0 || s >= d.n_streams) return;
  if (k + 1 < n && streams[k + 1] == s) return;
  const int idx = blockIdx.x * PT + threadIdx.x;
  if (idx == 0) {
    d.has_prev[s] = 1;
    d.ph[s] = h;
    d.pw[s] = w;
  }
  if (idx >= h * w) return;
  const size_t from = (size_t)k * d.cap + idx, to = (size_t)s * d.cap + idx;
  d.prev[to] = c.grey[from];
  d.gx[to] = c.gx[from];
  d.gy[to] = c.gy[from];
}

int round_half_even(double v) { return (int)std::nearbyint(v); }

int launch_chain(CmHandle* H_, int n, int H, int W, int ch, const uint8_t* frames,
                 const int32_t* streams, const int64_t* dst, int mode, double eps, int max_iter,
                 double scale, int h, int w, double* warps, double* rho, int32_t* iters,
                 int32_t* code, hipStream_t st) {
  PrepArgs p{frames, streams, H, W, ch, h, w, (scale > 0.0 && scale < 1.0) ? 1 : 0, scale};
  const dim3 pg((h * w + PT - 1) / PT, n);
  hipLaunchKernelGGL(cmc_chain_prep_kernel, pg, dim3(PT), 0, st, H_->d, H_->c, p);
  ChainArgs a{streams, dst, h, w, max_iter, eps, scale, warps, rho, iters, code};
  if (mode == BX_ECC_TRANSLATION)
    hipLaunchKernelGGL(cmc_ecc_chain_kernel<BX_ECC_TRANSLATION>, dim3(n), dim3(ET), 0, st, H_->d,
                       H_->c, a);
  else if (mode == BX_ECC_EUCLIDEAN)
    hipLaunchKernelGGL(cmc_ecc_chain_kernel<BX_ECC_EUCLIDEAN>, dim3(n), dim3(ET), 0, st, H_->d,
                       H_->c, a);
  else
    hipLaunchKernelGGL(cmc_ecc_chain_kernel<BX_ECC_AFFINE>, dim3(n), dim3(ET), 0, st, H_->d,
                       H_->c, a);
  hipLaunchKernelGGL(cmc_chain_handover_kernel, pg, dim3(PT), 0, st, H_->d, H_->c, streams, n, h, w);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int launch(CmHandle* H_, int n, int H, int W, int ch, const uint8_t* frames, const int32_t* streams,
           int mode, double eps, int max_iter, double scale, int h, int w, const double* init,
           double* warps, double* rho, int32_t* iters, int32_t* code, hipStream_t st) {
  PrepArgs p{frames, streams, H, W, ch, h, w, (scale > 0.0 && scale < 1.0) ? 1 : 0, scale};
  hipLaunchKernelGGL(cmc_prep_kernel, dim3((h * w + PT - 1) / PT, n), dim3(PT), 0, st, H_->d, p);
  EccArgs a{streams, init, h, w, max_iter, eps, scale, warps, rho, iters, code};
  if (mode == BX_ECC_TRANSLATION)
    hipLaunchKernelGGL(cmc_ecc_kernel<BX_ECC_TRANSLATION>, dim3(n), dim3(ET), 0, st, H_->d, a);
  else if (mode == BX_ECC_EUCLIDEAN)
    hipLaunchKernelGGL(cmc_ecc_kernel<BX_ECC_EUCLIDEAN>, dim3(n), dim3(ET), 0, st, H_->d, a);
  else
    hipLaunchKernelGGL(cmc_ecc_kernel<BX_ECC_AFFINE>, dim3(n), dim3(ET), 0, st, H_->d, a);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

// argument checks shared by the two entries; sets the working size
int check_args(CmHandle* H_, int n, int H, int W, int ch, int mode, int max_iter, double scale,
               int* h, int* w) {
  if (!H_) return cm_err(BX_ERR_INVALID, "null ecc handle");
  if (mode == BX_ECC_HOMOGRAPHY)
    return cm_err(BX_ERR_INVALID, "MOTION_HOMOGRAPHY is not supported: no engine takes a 3x3 warp");
  if (mode != BX_ECC_TRANSLATION && mode != BX_ECC_EUCLIDEAN && mode != BX_ECC_AFFINE)
    return cm_err(BX_ERR_INVALID, "unknown warp_mode");
  if (n < 0 || H < 1 || W < 1 || (ch != 1 && ch != 3) || max_iter < 0 || !(scale == scale))
    return cm_err(BX_ERR_INVALID, "n/H/W/channels/max_iter/scale out of range");
  if ((long long)H * W * ch * (long long)(n > 0 ? n : 1) >= (1LL << 40))
    return cm_err(BX_ERR_INVALID, "frames too large");
  int rc = bx_ecc_work_size(H, W, scale, h, w);
  if (rc != BX_OK) return rc;
  if (n > H_->d.n_streams)
    return cm_err(BX_ERR_CAPACITY, "more frames than the handle has streams");
  if (*h > H_->max_h || *w > H_->max_w)
    return cm_err(BX_ERR_CAPACITY, "working image " + std::to_string(*h) + "x" + std::to_string(*w) +
                                       " exceeds the handle's " + std::to_string(H_->max_h) + "x" +
                                       std::to_string(H_->max_w));
  return BX_OK;
}

// the same for the chained entries: a call's frames are bounded by the reserved slots, not by
// the streams
int check_chain_args(CmHandle* H_, int n, int H, int W, int ch, int mode, int max_iter,
                     double scale, int* h, int* w) {
  if (n < 0) return cm_err(BX_ERR_INVALID, "n/H/W/channels/max_iter/scale out of range");
  int rc = check_args(H_, 0, H, W, ch, mode, max_iter, scale, h, w);
  if (rc != BX_OK) return rc;
  if ((long long)H * W * ch * (long long)(n > 0 ? n : 1) >= (1LL << 40))
    return cm_err(BX_ERR_INVALID, "frames too large");
  if (n > H_->c.max_frames)
    return cm_err(BX_ERR_CAPACITY, "more frames than chain slots reserved (" +
                                       std::to_string(H_->c.max_frames) + ")");
  return BX_OK;
}

}  // namespace

extern "C" {

int bx_ecc_work_size(int H, int W, double scale, int* h, int* w) {
  if (!h || !w || H < 1 || W < 1) return cm_err(BX_ERR_INVALID, "bad size arguments");
  if (scale > 0.0 && scale < 1.0) {
    *h = round_half_even((double)H * scale);
    *w = round_half_even((double)W * scale);
    if (*h < 1 || *w < 1) return cm_err(BX_ERR_INVALID, "the scale leaves no pixel");
  } else {
    *h = H;
    *w = W;
  }
  return BX_OK;
}

int bx_ecc_create(int n_streams, int max_h, int max_w, void** out) {
  if (!out) return cm_err(BX_ERR_INVALID, "null argument");
  // (n_streams bounds a call's frames, which are the prep grid's y dimension)
  if (n_streams < 1 || n_streams > BX_ECC_MAX_STREAMS || max_h < 1 || max_w < 1 ||
      (long long)max_h * max_w > (1LL << 26) ||
      (long long)n_streams * max_h * max_w * 14 > (1LL << 36))
    return cm_err(BX_ERR_INVALID, "n_streams/max_h/max_w out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return cm_err(BX_ERR_NO_DEVICE, "no HIP device visible");
  CmHandle* H_ = new CmHandle();
  H_->max_h = max_h;
  H_->max_w = max_w;
  CmDev& d = H_->d;
  d.n_streams = n_streams;
  d.cap = max_h * max_w;
  const size_t planes = (size_t)n_streams * d.cap;
  auto fail = [&](hipError_t e) {
    bx_ecc_destroy(H_);
    return cm_err(BX_ERR_HIP, hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = hipMalloc(&d.prev, planes)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&d.cur, planes)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&d.curf, planes * 4)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&d.gx, planes * 4)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&d.gy, planes * 4)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&d.has_prev, (size_t)n_streams * 3 * 4 + 4)) != hipSuccess) return fail(e);
  d.ph = d.has_prev + n_streams;
  d.pw = d.ph + n_streams;
  d.status = d.pw + n_streams;
  if ((e = hipMemset(d.has_prev, 0, (size_t)n_streams * 3 * 4 + 4)) != hipSuccess) return fail(e);
  if ((e = hipMemset(d.prev, 0, planes)) != hipSuccess) return fail(e);
  if ((e = hipMemset(d.gx, 0, planes * 4)) != hipSuccess) return fail(e);
  if ((e = hipMemset(d.gy, 0, planes * 4)) != hipSuccess) return fail(e);
  const size_t ns = (size_t)n_streams;
  if ((e = hipMalloc(&H_->sstreams, ns * 4)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&H_->sinit, ns * 48)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&H_->swarps, ns * 48)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&H_->srho, ns * 8)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&H_->siters, ns * 4)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&H_->scode, ns * 4)) != hipSuccess) return fail(e);
  *out = H_;
  return BX_OK;
}

int bx_ecc_destroy(void* h) {
  CmHandle* H_ = (CmHandle*)h;
  if (!H_) return BX_OK;
  CmDev& d = H_->d;
  void* ps[] = {d.prev, d.cur, d.curf, d.gx, d.gy, d.has_prev, H_->sframes, H_->sstreams,
                H_->sinit, H_->swarps, H_->srho, H_->siters, H_->scode,
                H_->c.grey, H_->c.curf, H_->c.gx, H_->c.gy, H_->cstreams, H_->cwarps, H_->crho,
                H_->citers, H_->ccode};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  delete H_;
  return BX_OK;
}

int bx_ecc_reset(void* h, int stream, void* hip_stream) {
  CmHandle* H_ = (CmHandle*)h;
  if (!H_) return cm_err(BX_ERR_INVALID, "null ecc handle");
  if (stream >= H_->d.n_streams) return cm_err(BX_ERR_INVALID, "stream index out of range");
  hipStream_t st = (hipStream_t)hip_stream;
  if (stream < 0)
    BX_HIPCHK(hipMemsetAsync(H_->d.has_prev, 0, (size_t)H_->d.n_streams * 4, st));
  else
    BX_HIPCHK(hipMemsetAsync(H_->d.has_prev + stream, 0, 4, st));
  return BX_OK;
}

int bx_ecc_apply(void* h, int n, int H, int W, int channels, const uint8_t* frames,
                 const int32_t* streams, int warp_mode, double eps, int max_iter, double scale,
                 const double* init_warps, double* warps, double* rho, int32_t* iterations,
                 int32_t* code, void* hip_stream) {
  CmHandle* H_ = (CmHandle*)h;
  int hh, ww;
  int rc = check_args(H_, n, H, W, channels, warp_mode, max_iter, scale, &hh, &ww);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames || !streams || !warps || !rho || !iterations || !code)
    return cm_err(BX_ERR_INVALID, "null argument");
  return launch(H_, n, H, W, channels, frames, streams, warp_mode, eps, max_iter, scale, hh, ww,
                init_warps, warps, rho, iterations, code, (hipStream_t)hip_stream);
}

int bx_ecc_apply_host(void* h, int n, int H, int W, int channels, const uint8_t* frames_host,
                      const int32_t* streams_host, int warp_mode, double eps, int max_iter,
                      double scale, const double* init_warps_host, double* warps_host,
                      double* rho_host, int32_t* iterations_host, int32_t* code_host,
                      void* hip_stream) {
  CmHandle* H_ = (CmHandle*)h;
  int hh, ww;
  int rc = check_args(H_, n, H, W, channels, warp_mode, max_iter, scale, &hh, &ww);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames_host || !streams_host || !warps_host || !rho_host || !iterations_host || !code_host)
    return cm_err(BX_ERR_INVALID, "null argument");
  const int S = H_->d.n_streams;
  std::vector<char> seen(S, 0);
  for (int k = 0; k < n; k++) {
    const int s = streams_host[k];
    if (s < 0 || s >= S) return cm_err(BX_ERR_INVALID, "stream index out of range");
    if (seen[s]) return cm_err(BX_ERR_INVALID, "a stream is listed twice");
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
  if (init_warps_host)
    BX_HIPCHK(hipMemcpyAsync(H_->sinit, init_warps_host, (size_t)S * 48, hipMemcpyHostToDevice, st));
  rc = launch(H_, n, H, W, channels, H_->sframes, H_->sstreams, warp_mode, eps, max_iter, scale,
              hh, ww, init_warps_host ? H_->sinit : nullptr, H_->swarps, H_->srho, H_->siters,
              H_->scode, st);
  if (rc != BX_OK) return rc;
  std::vector<double> wv((size_t)S * 6), rv(S);
  std::vector<int32_t> iv(S), cv(S);
  BX_HIPCHK(hipMemcpyAsync(wv.data(), H_->swarps, (size_t)S * 48, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(rv.data(), H_->srho, (size_t)S * 8, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(iv.data(), H_->siters, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(cv.data(), H_->scode, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < n; k++) {
    const int s = streams_host[k];
    for (int q = 0; q < 6; q++) warps_host[(size_t)s * 6 + q] = wv[(size_t)s * 6 + q];
    rho_host[s] = rv[s];
    iterations_host[s] = iv[s];
    code_host[s] = cv[s];
  }
  return BX_OK;
}

int bx_ecc_chain_reserve(void* h, int max_frames) {
  CmHandle* H_ = (CmHandle*)h;
  if (!H_) return cm_err(BX_ERR_INVALID, "null ecc handle");
  const size_t cap = (size_t)H_->d.cap;
  if (max_frames < 1 || max_frames > BX_ECC_MAX_STREAMS ||
      (long long)max_frames * (long long)cap * 14 > (1LL << 36))
    return cm_err(BX_ERR_INVALID, "max_frames out of range");
  if (max_frames <= H_->c.max_frames) return BX_OK;
  // grown: the slots hold nothing between calls, so the old ones are dropped once the device
  // has finished with them
  BX_HIPCHK(hipDeviceSynchronize());
  CmChain& c = H_->c;
  void** ps[] = {(void**)&c.grey,       (void**)&c.curf,   (void**)&c.gx,
                 (void**)&c.gy,         (void**)&H_->cstreams, (void**)&H_->cwarps,
                 (void**)&H_->crho,     (void**)&H_->citers,   (void**)&H_->ccode};
  for (void** p : ps) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  c.max_frames = 0;
  const size_t m = (size_t)max_frames;
  const size_t bytes[] = {m * cap, m * cap * 4, m * cap * 4, m * cap * 4, m * 4,
                          m * 48,  m * 8,       m * 4,       m * 4};
  for (int q = 0; q < 9; q++) {
    hipError_t e = hipMalloc(ps[q], bytes[q]);
    if (e != hipSuccess) {
      for (void** p : ps) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
      }
      return cm_err(BX_ERR_HIP, hipGetErrorString(e));
    }
  }
  c.max_frames = max_frames;
  return BX_OK;
}

int bx_ecc_apply_chain(void* h, int n, int H, int W, int channels, const uint8_t* frames,
                       const int32_t* streams, const int64_t* dst, int warp_mode, double eps,
                       int max_iter, double scale, double* warps, double* rho,
                       int32_t* iterations, int32_t* code, void* hip_stream) {
  CmHandle* H_ = (CmHandle*)h;
  int hh, ww;
  int rc = check_chain_args(H_, n, H, W, channels, warp_mode, max_iter, scale, &hh, &ww);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames || !streams || !warps || !rho || !iterations || !code)
    return cm_err(BX_ERR_INVALID, "null argument");
  return launch_chain(H_, n, H, W, channels, frames, streams, dst, warp_mode, eps, max_iter,
                      scale, hh, ww, warps, rho, iterations, code, (hipStream_t)hip_stream);
}

int bx_ecc_apply_chain_host(void* h, int n, int H, int W, int channels,
                            const uint8_t* frames_host, const int32_t* streams_host,
                            int warp_mode, double eps, int max_iter, double scale,
                            double* warps_host, double* rho_host, int32_t* iterations_host,
                            int32_t* code_host, void* hip_stream) {
  CmHandle* H_ = (CmHandle*)h;
  int hh, ww;
  int rc = check_chain_args(H_, n, H, W, channels, warp_mode, max_iter, scale, &hh, &ww);
  if (rc != BX_OK) return rc;
  if (n == 0) return BX_OK;
  if (!frames_host || !streams_host || !warps_host || !rho_host || !iterations_host || !code_host)
    return cm_err(BX_ERR_INVALID, "null argument");
  const int S = H_->d.n_streams;
  std::vector<char> seen(S, 0);
  for (int k = 0; k < n; k++) {
    const int s = streams_host[k];
    if (s < 0 || s >= S) return cm_err(BX_ERR_INVALID, "stream index out of range");
    if (seen[s] && streams_host[k - 1] != s)
      return cm_err(BX_ERR_INVALID, "the frames of a stream are not adjacent");
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
  rc = launch_chain(H_, n, H, W, channels, H_->sframes, H_->cstreams, nullptr, warp_mode, eps,
                    max_iter, scale, hh, ww, H_->cwarps, H_->crho, H_->citers, H_->ccode, st);
  if (rc != BX_OK) return rc;
  BX_HIPCHK(hipMemcpyAsync(warps_host, H_->cwarps, (size_t)n * 48, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(rho_host, H_->crho, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(iterations_host, H_->citers, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(code_host, H_->ccode, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  return BX_OK;
}

int bx_ecc_status(void* h, int* status) {
  CmHandle* H_ = (CmHandle*)h;
  if (!H_ || !status) return cm_err(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(status, H_->d.status, 4, hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_ecc_state_host(void* h, int stream, int* has_prev, int* hh, int* ww, uint8_t* grey,
                      float* gx, float* gy) {
  CmHandle* H_ = (CmHandle*)h;
  if (!H_ || !has_prev || !hh || !ww) return cm_err(BX_ERR_INVALID, "null argument");
  const CmDev& d = H_->d;
  if (stream < 0 || stream >= d.n_streams) return cm_err(BX_ERR_INVALID, "stream index out of range");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(has_prev, d.has_prev + stream, 4, hipMemcpyDeviceToHost));
  BX_HIPCHK(hipMemcpy(hh, d.ph + stream, 4, hipMemcpyDeviceToHost));
  BX_HIPCHK(hipMemcpy(ww, d.pw + stream, 4, hipMemcpyDeviceToHost));
  const size_t o = (size_t)stream * d.cap;
  if (grey) BX_HIPCHK(hipMemcpy(grey, d.prev + o, d.cap, hipMemcpyDeviceToHost));
  if (gx) BX_HIPCHK(hipMemcpy(gx, d.gx + o, (size_t)d.cap * 4, hipMemcpyDeviceToHost));
  if (gy) BX_HIPCHK(hipMemcpy(gy, d.gy + o, (size_t)d.cap * 4, hipMemcpyDeviceToHost));
  return BX_OK;
}

}  // extern "C"
