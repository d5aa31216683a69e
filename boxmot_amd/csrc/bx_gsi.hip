// bx_gsi.hip — GSI post-processing (include/bxgsi.h): tracklet interpolation and fixed-kernel
// Gaussian-process smoothing of MOT result rows, restating boxmot/postprocessing/gsi.py.
//
// Interpolation: a bitonic sort of (sequence, id, frame, row index) keys (the index makes keys
// unique, so the network reproduces np.lexsort's stable order), one workgroup's scan of the
// per-row gap counts and tracklet starts, then a fill pass.  The inserted rows are plain float64
// arithmetic in the reference's written order (the library is built with -ffp-contract=off), so
// the output is bitwise the reference's.
//
// Smoothing: one workgroup per tracklet.  The factor lives in one packed layout on both paths:
// rows 0..n-1 are the lower triangle of K + 1e-10*I (row i at i(i+1)/2), rows n..n+3 are the four
// right-hand sides (columns 2..5) as full rows of length n.  Factoring the triangle right-looking
// with the right-hand sides carried as four more rows leaves z = L^-1 y in them — the forward
// solve costs nothing extra.  A backward sweep turns z into alpha in place, and the mean K @ alpha
// recomputes K (without the jitter, diagonal exactly 1) on the fly.
//   * n <= BX_GSI_LDS_N: the layout is in LDS, factored column by column.
//   * longer: the layout is in an HBM slot; panels of BX_GSI_NB columns — diagonal block factored
//     in LDS by the same column routine, panel rows solved one per thread against it, trailing
//     update by 64x64 tiles whose two panel slices sit in LDS, accumulated with plain fp64 FMAs
//     (4x4 per thread) and subtracted once.
// The sums of every element run in a fixed order that depends only on n and the path, never on
// the launch shape, so a batch returns the bits of single calls.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/bxassoc.h"
#include "../../include/bxgsi.h"
#include "bx_device.h"
#include "bx_host.h"


using namespace bx;

namespace {

int gsi_err(int code, const std::string& msg) { return bx_record_error(code, msg.c_str()); }
constexpr int LDS_N = BX_GSI_LDS_N, NB = BX_GSI_NB, MAX_N = BX_GSI_MAX_N;
constexpr int TILE = 64, TLD = 66;  // trailing tile edge, padded leading dimension in LDS
constexpr int MAX_SLOTS = 512;      // persistent workgroups of the blocked kernel
constexpr size_t SLOT_BUDGET = (size_t)1 << 30;
constexpr double JITTER = 1e-10;    // GaussianProcessRegressor(alpha=1e-10)

// ------------------------------------------------------------------------------ interpolation
struct Key {
  double id, frame;
  int seq, idx;
};

__device__ __forceinline__ bool key_less(const Key& a, const Key& b) {
  if (a.seq != b.seq) return a.seq < b.seq;
  if (a.id != b.id) return a.id < b.id;
  if (a.frame != b.frame) return a.frame < b.frame;
  return a.idx < b.idx;
}

__global__ void gsi_keys_kernel(const double* rows, const int32_t* seq, int R, int C, int P,
                                Key* keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  Key k;
  if (i < R) {
    k.frame = rows[(size_t)i * C];
    k.id = rows[(size_t)i * C + 1];
    k.seq = seq ? seq[i] : 0;
    k.idx = i;
  } else {  // padding up to the power of two: sorts last
    k.frame = 0.0;
    k.id = 0.0;
    k.seq = INT_MAX;
    k.idx = i;
  }
  keys[i] = k;
}

__global__ void gsi_bitonic_kernel(Key* keys, int P, int k, int j) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const int l = i ^ j;
  if (l <= i) return;
  const Key a = keys[i], b = keys[l];
  const bool asc = (i & k) == 0;
  if (key_less(b, a) == asc) {
    keys[i] = b;
    keys[l] = a;
  }
}

// rows the gap before sorted row p inserts, and whether p starts a tracklet
__device__ __forceinline__ void gsi_gap(const Key* keys, int p, int interval, int& cnt,
                                        int& start) {
  cnt = 0;
  start = 1;
  if (p == 0) return;
  const Key c = keys[p], v = keys[p - 1];
  if (c.seq != v.seq || c.id != v.id) return;
  start = 0;
  const long long pf = (long long)v.frame, cf = (long long)c.frame;
  if (pf + 1 < cf && cf < pf + interval) cnt = (int)(cf - pf - 1);
}

// one workgroup: exclusive scans of the gap counts and tracklet starts in sorted order
__global__ void __launch_bounds__(1024) gsi_scan_kernel(const Key* keys, int R, int interval,
                                                        int* cnt, int* opos, int* tidx,
                                                        long long* counts) {
  __shared__ int wa[16], wb[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long ca = 0;
  int cb = 0;
  for (int base = 0; base < R; base += 1024) {
    const int p = base + (int)threadIdx.x;
    int a = 0, b = 0;
    if (p < R) gsi_gap(keys, p, interval, a, b);
    int xa = a, xb = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ya = __shfl_up(xa, d), yb = __shfl_up(xb, d);
      if (lane >= d) {
        xa += ya;
        xb += yb;
      }
    }
    if (lane == 63) {
      wa[w] = xa;
      wb[w] = xb;
    }
    __syncthreads();
    int oa = 0, ob = 0, ta = 0, tb = 0;
    for (int q = 0; q < 16; q++) {
      if (q < w) {
        oa += wa[q];
        ob += wb[q];
      }
      ta += wa[q];
      tb += wb[q];
    }
    if (p < R) {
      cnt[p] = a;
      opos[p] = (int)(p + ca + oa + xa);  // where row p itself lands (its gap rows before it)
      tidx[p] = cb + ob + xb - 1;
    }
    ca += ta;
    cb += tb;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] = R + ca;
    counts[1] = cb;
  }
}

__global__ void gsi_fill_kernel(const Key* keys, const double* rows, int R, int C,
                                const int* cnt, const int* opos, const int* tidx, double* out,
                                int32_t* out_seq, long long cap, int32_t* track_off) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= R) return;
  const Key c = keys[p];
  const int n = cnt[p], pos = opos[p];
  const double* row = rows + (size_t)c.idx * C;
  if (n > 0) {
    const Key v = keys[p - 1];
    const double* prow = rows + (size_t)v.idx * C;
    const long long d = (long long)c.frame - (long long)v.frame;
    for (int i = 1; i <= n; i++) {
      const long long o = (long long)pos - n + i - 1;
      if (o < 0 || o >= cap) continue;
      const double f = (double)i / (double)d;
      for (int q = 0; q < C; q++) out[o * C + q] = prow[q] + (row[q] - prow[q]) * f;
      if (out_seq) out_seq[o] = c.seq;
    }
  }
  if (pos >= 0 && pos < cap) {
    for (int q = 0; q < C; q++) out[(size_t)pos * C + q] = row[q];
    if (out_seq) out_seq[pos] = c.seq;
  }
  const int t = tidx[p];
  if (p == 0 || tidx[p - 1] != t) track_off[t] = pos;
  if (p == R - 1) track_off[t + 1] = pos + 1;
}

// ---------------------------------------------------------------- result slots in device memory
// The slot-aware key/pack stage.  One thread per candidate row i of the packed order (slot 0's
// rows, then slot 1's, ...): its slot is the last q with pre[q] <= i (pre: the exclusive prefix of
// n, n_seq + 1 entries; empty slots share a prefix value with their successor and are passed
// over), its row's columns 0..7 go to packed[i] and its key to keys[i].  Only rows inside a slot
// are addressed.  Threads R..P-1 write the padding keys of gsi_keys_kernel.
__global__ void gsi_slot_pack_kernel(const double* rows, long long stride, const long long* base,
                                     const long long* pre, int n_seq, int R, int P,
                                     double* packed, Key* keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  Key k;
  if (i < R) {
    int lo = 0, hi = n_seq - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= i) lo = mid;
      else hi = mid - 1;
    }
    const double* r = rows + (size_t)(base[lo] + ((long long)i - pre[lo])) * (size_t)stride;
    double* p = packed + (size_t)i * 8;
#pragma unroll
    for (int q = 0; q < 8; q++) p[q] = r[q];
    k.frame = p[0];
    k.id = p[1];
    k.seq = lo;
    k.idx = i;
  } else {
    k.frame = 0.0;
    k.id = 0.0;
    k.seq = INT_MAX;
    k.idx = i;
  }
  keys[i] = k;
}

// The finalise stage, one thread per output row, sequence and tracklet (whichever are more):
//   * row i: every value truncated toward zero, what "%d" writes and a reader gets back; the
//     + 0.0 turns the -0.0 of a negative fraction into +0.0 (the library is built without
//     fast-math, so it stays);
//   * sequence q: out_base / out_n from the sorted labels oseq, as the lower bounds of q and
//     q + 1, so a sequence without rows, wherever it lies, gets its successor's base and n = 0;
//   * tracklet t: the smallest t whose factorisation failed, into *fail (preset above any t).
__global__ void gsi_finalise_kernel(double* out, const int32_t* oseq, int n_out, int n_seq,
                                    int truncate, const int32_t* status, int n_tracks,
                                    long long* out_base, long long* out_n, int* fail) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_out && truncate) {
    double* o = out + (size_t)i * 9;
#pragma unroll
    for (int q = 0; q < 9; q++) o[q] = trunc(o[q]) + 0.0;
  }
  if (i < n_seq) {
    int b[2];
    for (int e = 0; e < 2; e++) {
      int lo = 0, hi = n_out;  // first row whose label is >= i + e
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (oseq[mid] < i + e) lo = mid + 1;
        else hi = mid;
      }
      b[e] = lo;
    }
    out_base[i] = b[0];
    out_n[i] = b[1] - b[0];
  }
  if (i < n_tracks && status[i] != BX_OK) atomicMin(fail, i);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
int pow2_at_least(int64_t n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
struct PlanLayout {
  size_t keys, cnt, opos, tidx, total;
  int P;
};
PlanLayout plan_layout(int64_t R) {
  PlanLayout l;
  l.P = pow2_at_least(R > 0 ? R : 1);
  l.keys = 0;
  l.cnt = align256((size_t)l.P * sizeof(Key));
  l.opos = l.cnt + align256((size_t)R * 4);
  l.tidx = l.opos + align256((size_t)R * 4);
  l.total = l.tidx + align256((size_t)R * 4) + 256;
  return l;
}
// the sort of the P keys in the workspace w and the scan of the first R of them
void sort_scan(const PlanLayout& l, int R, int interval, char* w, int64_t* counts,
               hipStream_t st) {
  Key* keys = (Key*)(w + l.keys);
  const int P = l.P, nblk = (P + 255) / 256;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) gsi_bitonic_kernel<<<nblk, 256, 0, st>>>(keys, P, k, j);
  gsi_scan_kernel<<<1, 1024, 0, st>>>(keys, R, interval, (int*)(w + l.cnt), (int*)(w + l.opos),
                                      (int*)(w + l.tidx), (long long*)counts);
}

// device allocations that live as long as their owner
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() {
    for (void* q : p) (void)hipFree(q);
  }
  hipError_t get(void** q, size_t bytes) {
    const hipError_t e = hipMalloc(q, bytes ? bytes : 1);
    if (e == hipSuccess) p.push_back(*q);
    return e;
  }
};

// what bx_gsi_device_plan leaves for bx_gsi_device_run
struct DevicePlan {
  DevBufs bufs;
  int64_t R = 0, n_out = 0;
  int n_seq = 0, n_tracks = 0;
  double* packed = nullptr;  // [R][8], slot order
  void* ws = nullptr;        // plan_layout(R)
};

// ---------------------------------------------------------------------------------- smoothing
// offset of row i of the packed layout of a tracklet of n rows (rows >= n: right-hand sides)
__device__ __forceinline__ size_t roff(int i, int n) {
  return i < n ? (size_t)i * (size_t)(i + 1) / 2
               : (size_t)n * (size_t)(n + 1) / 2 + (size_t)(i - n) * (size_t)n;
}
__host__ __device__ inline size_t layout_doubles(int n) {
  return (size_t)n * (size_t)(n + 1) / 2 + 4 * (size_t)n;
}

__device__ __forceinline__ double gsi_length_scale(double tau, int n) {
  const double ls = tau * log(tau * tau * tau / (double)n);
  return fmin(fmax(ls, 1.0 / tau), tau * tau);
}

// K + jitter*I (lower triangle) and the right-hand sides into the packed layout A; ts = t / ls
__device__ __forceinline__ void gsi_build(double* A, const double* ts, const double* rows, int C,
                                          int n) {
  for (int i = 0; i < n; i++) {
    const double ti = ts[i];
    double* ri = A + roff(i, n);
    for (int j = threadIdx.x; j <= i; j += WG) {
      const double d = ti - ts[j];
      ri[j] = j == i ? 1.0 + JITTER : exp(-0.5 * (d * d));
    }
  }
  for (int k = threadIdx.x; k < 4 * n; k += WG) {
    const int q = k / n, j = k - q * n;
    A[roff(n + q, n) + j] = rows[(size_t)j * C + 2 + q];
  }
}

// Right-looking Cholesky of the packed layout A (n triangle rows, m >= n rows in all), column
// by column, by the whole workgroup; col: m doubles of LDS.  False (for every thread) on a
// non-positive pivot.  Callers synchronise before and after.
__device__ __forceinline__ bool gsi_chol_packed(double* A, int n, int m, double* col) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int k = 0; k < n; k++) {
    const double d = A[roff(k, n) + k];
    if (!(d > 0.0)) return false;
    const double s = sqrt(d);
    __syncthreads();  // every thread holds the pivot before it is replaced
    for (int i = k + (int)threadIdx.x; i < m; i += WG) {
      double* p = A + roff(i, n) + k;
      const double v = i == k ? s : *p / s;
      *p = v;
      col[i] = v;
    }
    __syncthreads();
    for (int i = k + 1 + ty; i < m; i += 16) {
      const double lik = col[i];
      const int jmax = i < n ? i : n - 1;
      double* ri = A + roff(i, n);
      for (int j = k + 1 + tx; j <= jmax; j += 16) ri[j] = fma(-lik, col[j], ri[j]);
    }
    __syncthreads();
  }
  return true;
}

// L^T alpha = z in place on the right-hand-side rows of the packed layout
__device__ __forceinline__ void gsi_backward(double* A, int n) {
  double* z = A + roff(n, n);
  for (int k = n - 1; k >= 0; k--) {
    const double* rk = A + roff(k, n);
    if (threadIdx.x < 4) z[(size_t)threadIdx.x * n + k] = z[(size_t)threadIdx.x * n + k] / rk[k];
    __syncthreads();
    const double a0 = z[k], a1 = z[(size_t)n + k], a2 = z[2 * (size_t)n + k],
                 a3 = z[3 * (size_t)n + k];
    for (int j = threadIdx.x; j < k; j += WG) {
      const double l = rk[j];
      z[j] = fma(-l, a0, z[j]);
      z[(size_t)n + j] = fma(-l, a1, z[(size_t)n + j]);
      z[2 * (size_t)n + j] = fma(-l, a2, z[2 * (size_t)n + j]);
      z[3 * (size_t)n + j] = fma(-l, a3, z[3 * (size_t)n + j]);
    }
    __syncthreads();
  }
}

// output rows of one tracklet: mean = K @ alpha (al: 4 rows of n), or the unsmoothed columns
// when the factorisation failed.  A wave per row, lanes over j, a fixed butterfly.
__device__ __forceinline__ void gsi_emit(const double* ts, const double* al, const double* rows,
                                         int C, int n, double* out, bool ok) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = w; i < n; i += WG / 64) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (ok) {
      const double ti = ts[i];
      for (int j = lane; j < n; j += 64) {
        const double d = ti - ts[j];
        const double kij = exp(-0.5 * (d * d));
        s0 = fma(kij, al[j], s0);
        s1 = fma(kij, al[(size_t)n + j], s1);
        s2 = fma(kij, al[2 * (size_t)n + j], s2);
        s3 = fma(kij, al[3 * (size_t)n + j], s3);
      }
      s0 = wave_bfly_desc_f64(s0);
      s1 = wave_bfly_desc_f64(s1);
      s2 = wave_bfly_desc_f64(s2);
      s3 = wave_bfly_desc_f64(s3);
    }
    if (lane == 0) {
      const double* r = rows + (size_t)i * C;
      double* o = out + (size_t)i * 9;
      o[0] = r[0];
      o[1] = r[1];
      o[2] = ok ? s0 : r[2];
      o[3] = ok ? s1 : r[3];
      o[4] = ok ? s2 : r[4];
      o[5] = ok ? s3 : r[5];
      o[6] = r[6];
      o[7] = r[7];
      o[8] = -1.0;
    }
  }
}

// tracklets of at most LDS_N rows: dynamic LDS = layout_doubles(n) + n doubles (ts)
__global__ void __launch_bounds__(WG) gsi_smooth_lds_kernel(const double* rows, int C,
                                                            const int32_t* track_off, double tau,
                                                            double* out, int32_t* status) {
  extern __shared__ double lds[];
  __shared__ double col[LDS_N + 4];
  const int k = blockIdx.x;
  const int r0 = track_off[k], n = track_off[k + 1] - r0;
  if (n <= 0 || n > LDS_N) return;
  double* A = lds;
  double* ts = lds + layout_doubles(n);
  const double* trows = rows + (size_t)r0 * C;
  const double ls = gsi_length_scale(tau, n);
  for (int i = threadIdx.x; i < n; i += WG) ts[i] = trows[(size_t)i * C] / ls;
  __syncthreads();
  gsi_build(A, ts, trows, C, n);
  __syncthreads();
  const bool ok = gsi_chol_packed(A, n, n + 4, col);
  __syncthreads();
  if (ok) gsi_backward(A, n);
  if (threadIdx.x == 0) status[k] = ok ? BX_OK : BX_ERR_INVALID;
  gsi_emit(ts, A + roff(n, n), trows, C, n, out + (size_t)r0 * 9, ok);
}

// Blocked path: persistent workgroups, each with one HBM slot, over the tracklets longer than
// `above` rows.
__global__ void __launch_bounds__(WG) gsi_smooth_blocked_kernel(const double* rows, int C,
                                                                const int32_t* track_off,
                                                                int n_tracks, int above,
                                                                double tau, double* slots,
                                                                size_t slot_doubles, double* out,
                                                                int32_t* status) {
  __shared__ double ts[MAX_N];
  __shared__ double D[NB * (NB + 1) / 2];
  __shared__ double col[NB];
  __shared__ __attribute__((aligned(16))) double PI[NB * TLD], PJ[NB * TLD];
  double* A = slots + (size_t)blockIdx.x * slot_doubles;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int k = blockIdx.x; k < n_tracks; k += gridDim.x) {
    const int r0 = track_off[k], n = track_off[k + 1] - r0;
    if (n <= above || n > MAX_N) continue;
    const int m = n + 4;
    const double* trows = rows + (size_t)r0 * C;
    const double ls = gsi_length_scale(tau, n);
    __syncthreads();  // the previous tracklet's readers of ts are done
    for (int i = threadIdx.x; i < n; i += WG) ts[i] = trows[(size_t)i * C] / ls;
    __syncthreads();
    gsi_build(A, ts, trows, C, n);
    __syncthreads();
    bool ok = true;
    for (int kb = 0; kb < n && ok; kb += NB) {
      const int nb = n - kb < NB ? n - kb : NB;
      // diagonal block into LDS, padded to NB with the identity
      for (int e = threadIdx.x; e < NB * NB; e += WG) {
        const int a = e / NB, b = e % NB;
        if (b > a) continue;
        D[roff(a, NB) + b] = (a < nb && b < nb) ? A[roff(kb + a, n) + kb + b] : (a == b ? 1.0 : 0.0);
      }
      __syncthreads();
      ok = gsi_chol_packed(D, NB, NB, col);
      __syncthreads();
      if (!ok) break;
      for (int e = threadIdx.x; e < NB * NB; e += WG) {
        const int a = e / NB, b = e % NB;
        if (b <= a && a < nb) A[roff(kb + a, n) + kb + b] = D[roff(a, NB) + b];
      }
      // panel rows (and the right-hand sides): x = a_row * Ldiag^-T, one row per thread, in place
      // (the row's 256 bytes stay in cache; holding it in registers spilled)
      for (int i = kb + nb + (int)threadIdx.x; i < m; i += WG) {
        double* p = A + roff(i, n) + kb;
        for (int b = 0; b < nb; b++) {
          const double* db = D + b * (b + 1) / 2;
          double s = p[b];
          for (int c = 0; c < b; c++) s = fma(-p[c], db[c], s);
          p[b] = s / db[b];
        }
      }
      __syncthreads();
      // trailing update: rows and columns from kb + nb on, 64 x 64 tiles on and below the diagonal
      const int t0 = kb + nb;
      for (int I0 = t0; I0 < m; I0 += TILE) {
        for (int J0 = t0; J0 <= I0 && J0 < n; J0 += TILE) {
          for (int e = threadIdx.x; e < NB * TILE; e += WG) {
            const int r = e / NB, c = e % NB;
            const int i = I0 + r, j = J0 + r;
            PI[c * TLD + r] = (i < m && c < nb) ? A[roff(i, n) + kb + c] : 0.0;
            PJ[c * TLD + r] = (j < n && c < nb) ? A[roff(j, n) + kb + c] : 0.0;
          }
          __syncthreads();
          double acc[4][4] = {};
#pragma unroll 4
          for (int c = 0; c < NB; c++) {
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
              a[q] = PI[c * TLD + ty * 4 + q];
              b[q] = PJ[c * TLD + tx * 4 + q];
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
              for (int v = 0; v < 4; v++) acc[u][v] = fma(a[u], b[v], acc[u][v]);
          }
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int i = I0 + ty * 4 + u;
            if (i >= m) continue;
            double* ri = A + roff(i, n);
#pragma unroll
            for (int v = 0; v < 4; v++) {
              const int j = J0 + tx * 4 + v;
              if (j < n && j <= i) ri[j] -= acc[u][v];
            }
          }
          __syncthreads();
        }
      }
    }
    __syncthreads();
    if (ok) gsi_backward(A, n);
    if (threadIdx.x == 0) status[k] = ok ? BX_OK : BX_ERR_INVALID;
    gsi_emit(ts, A + roff(n, n), trows, C, n, out + (size_t)r0 * 9, ok);
  }
}

struct SmoothPlan {
  int max_lds = 0, max_blk = 0, n_blk = 0, slots = 0;
  size_t off_bytes = 0, slot_doubles = 0, total = 0;
};
int smooth_plan(const int32_t* off, int n_tracks, int force_blocked, SmoothPlan& p) {
  if (n_tracks < 0 || (n_tracks > 0 && !off)) return gsi_err(BX_ERR_INVALID, "gsi: bad tracklet offsets");
  for (int k = 0; k < n_tracks; k++) {
    const long long n = (long long)off[k + 1] - off[k];
    if (n < 0) return gsi_err(BX_ERR_INVALID, "gsi: tracklet offsets must not decrease");
    if (n > MAX_N)
      return gsi_err(BX_ERR_CAPACITY, "gsi: tracklet of " + std::to_string(n) + " rows exceeds BX_GSI_MAX_N");
    if (n == 0) continue;
    if (force_blocked || n > LDS_N) {
      p.n_blk++;
      if (n > p.max_blk) p.max_blk = (int)n;
    } else if (n > p.max_lds) {
      p.max_lds = (int)n;
    }
  }
  p.off_bytes = align256(((size_t)n_tracks + 1) * 4);
  if (p.n_blk) {
    p.slot_doubles = (layout_doubles(p.max_blk) + 31) & ~(size_t)31;
    size_t fit = SLOT_BUDGET / (p.slot_doubles * 8);
    if (fit < 1) fit = 1;
    p.slots = p.n_blk;
    if (p.slots > MAX_SLOTS) p.slots = MAX_SLOTS;
    if ((size_t)p.slots > fit) p.slots = (int)fit;
  }
  p.total = p.off_bytes + (size_t)p.slots * p.slot_doubles * 8;
  return BX_OK;
}

}  // namespace

extern "C" {

int bx_gsi_plan_workspace_bytes(int64_t R, size_t* bytes) {
  if (R < 0 || R >= INT_MAX / 2 || !bytes) return gsi_err(BX_ERR_INVALID, "gsi: bad row count");
  *bytes = plan_layout(R).total;
  return BX_OK;
}

int bx_gsi_interpolate_plan(const double* rows, const int32_t* seq, int64_t R, int C, int interval,
                            void* ws, size_t ws_bytes, int64_t* counts, void* stream) {
  if (R < 0 || R >= INT_MAX / 2 || C < 2 || !counts || !ws || (R > 0 && !rows))
    return gsi_err(BX_ERR_INVALID, "gsi: bad interpolation arguments");
  const PlanLayout l = plan_layout(R);
  if (ws_bytes < l.total) return gsi_err(BX_ERR_CAPACITY, "gsi: interpolation workspace too small");
  hipStream_t st = (hipStream_t)stream;
  gsi_keys_kernel<<<(l.P + 255) / 256, 256, 0, st>>>(rows, seq, (int)R, C, l.P,
                                                     (Key*)((char*)ws + l.keys));
  sort_scan(l, (int)R, interval, (char*)ws, counts, st);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_gsi_interpolate(const double* rows, int64_t R, int C, const void* ws, double* out,
                       int32_t* out_seq, int64_t cap, int32_t* track_off, void* stream) {
  if (R < 0 || R >= INT_MAX / 2 || C < 2 || !ws || cap < 0 || !track_off || (R > 0 && (!rows || !out)))
    return gsi_err(BX_ERR_INVALID, "gsi: bad interpolation arguments");
  if (R == 0) return BX_OK;
  const PlanLayout l = plan_layout(R);
  const char* w = (const char*)ws;
  gsi_fill_kernel<<<(int)((R + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const Key*)(w + l.keys), rows, (int)R, C, (const int*)(w + l.cnt),
      (const int*)(w + l.opos), (const int*)(w + l.tidx), out, out_seq, (long long)cap,
      track_off);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_gsi_workspace_bytes(const int32_t* track_off_host, int n_tracks, int force_blocked,
                           size_t* bytes) {
  SmoothPlan p;
  if (!bytes) return gsi_err(BX_ERR_INVALID, "gsi: null bytes");
  if (const int rc = smooth_plan(track_off_host, n_tracks, force_blocked, p)) return rc;
  *bytes = p.total;
  return BX_OK;
}

int bx_gsi_smooth(const double* rows, int C, const int32_t* track_off_host, int n_tracks,
                  double tau, int force_blocked, void* ws, size_t ws_bytes, double* out,
                  int32_t* status, void* stream) {
  SmoothPlan p;
  if (C < 8) return gsi_err(BX_ERR_INVALID, "gsi: smoothing needs at least 8 columns");
  if (!(tau > 0.0)) return gsi_err(BX_ERR_INVALID, "gsi: tau must be positive");
  if (const int rc = smooth_plan(track_off_host, n_tracks, force_blocked, p)) return rc;
  if (n_tracks == 0) return BX_OK;
  if (!rows || !out || !status || !ws) return gsi_err(BX_ERR_INVALID, "gsi: null pointer");
  if (ws_bytes < p.total) return gsi_err(BX_ERR_CAPACITY, "gsi: smoothing workspace too small");
  hipStream_t st = (hipStream_t)stream;
  int32_t* off = (int32_t*)ws;
  BX_HIPCHK(hipMemcpyAsync(off, track_off_host, ((size_t)n_tracks + 1) * 4, hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipMemsetAsync(status, 0, (size_t)n_tracks * 4, st));
  if (p.max_lds) {
    const size_t lds = (layout_doubles(p.max_lds) + p.max_lds) * 8;
    BX_HIPCHK(bx_lds_attr((const void*)gsi_smooth_lds_kernel, lds));
    gsi_smooth_lds_kernel<<<n_tracks, WG, lds, st>>>(rows, C, off, tau, out, status);
  }
  if (p.n_blk) {
    double* slots = (double*)((char*)ws + p.off_bytes);
    gsi_smooth_blocked_kernel<<<p.slots, WG, 0, st>>>(rows, C, off, n_tracks,
                                                      force_blocked ? 0 : LDS_N, tau, slots,
                                                      p.slot_doubles, out, status);
  }
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_gsi_run_host(const double* rows_host, int64_t R, int C, int interval, double tau,
                    double* out_host, int64_t cap, int64_t* n_out, void* stream) {
  if (R < 0 || C < 8 || !n_out || cap < 0 || (R > 0 && !rows_host))
    return gsi_err(BX_ERR_INVALID, "gsi: bad arguments");
  *n_out = 0;
  if (R == 0) return BX_OK;
  hipStream_t st = (hipStream_t)stream;
  DevBufs bufs;
  size_t pbytes = 0;
  if (const int rc = bx_gsi_plan_workspace_bytes(R, &pbytes)) return rc;
  void *d_rows, *d_plan, *d_counts;
  BX_HIPCHK(bufs.get(&d_rows, (size_t)R * C * 8));
  BX_HIPCHK(bufs.get(&d_plan, pbytes));
  BX_HIPCHK(bufs.get(&d_counts, 16));
  BX_HIPCHK(hipMemcpyAsync(d_rows, rows_host, (size_t)R * C * 8, hipMemcpyHostToDevice, st));
  if (const int rc = bx_gsi_interpolate_plan((const double*)d_rows, nullptr, R, C, interval,
                                             d_plan, pbytes, (int64_t*)d_counts, st))
    return rc;
  int64_t counts[2] = {0, 0};
  BX_HIPCHK(hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  *n_out = counts[0];
  if (counts[0] > cap || !out_host)
    return gsi_err(BX_ERR_CAPACITY, "gsi: output holds fewer rows than the interpolation yields");
  const int nt = (int)counts[1];
  void *d_interp, *d_off, *d_out, *d_status, *d_ws;
  BX_HIPCHK(bufs.get(&d_interp, (size_t)counts[0] * C * 8));
  BX_HIPCHK(bufs.get(&d_off, ((size_t)nt + 1) * 4));
  if (const int rc = bx_gsi_interpolate((const double*)d_rows, R, C, d_plan, (double*)d_interp,
                                        nullptr, counts[0], (int32_t*)d_off, st))
    return rc;
  std::vector<int32_t> off((size_t)nt + 1), status((size_t)nt);
  BX_HIPCHK(hipMemcpyAsync(off.data(), d_off, off.size() * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  size_t sbytes = 0;
  if (const int rc = bx_gsi_workspace_bytes(off.data(), nt, 0, &sbytes)) return rc;
  BX_HIPCHK(bufs.get(&d_ws, sbytes));
  BX_HIPCHK(bufs.get(&d_out, (size_t)counts[0] * 9 * 8));
  BX_HIPCHK(bufs.get(&d_status, (size_t)nt * 4));
  if (const int rc = bx_gsi_smooth((const double*)d_interp, C, off.data(), nt, tau, 0, d_ws, sbytes,
                                   (double*)d_out, (int32_t*)d_status, st))
    return rc;
  BX_HIPCHK(hipMemcpyAsync(out_host, d_out, (size_t)counts[0] * 9 * 8, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(status.data(), d_status, status.size() * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < nt; k++)
    if (status[k] != BX_OK)
      return gsi_err(BX_ERR_INVALID, "gsi: tracklet " + std::to_string(k) +
                                         ": the kernel matrix is not positive definite");
  return BX_OK;
}

int bx_gsi_device_plan(const double* rows, int64_t row_stride, const int64_t* base,
                       const int64_t* n, int n_seq, int interval, int64_t* counts_host,
                       void** plan, void* stream) {
  if (!counts_host || !plan || n_seq < 0 || row_stride < 8 || (n_seq > 0 && (!base || !n)))
    return gsi_err(BX_ERR_INVALID, "gsi: bad result-slot arguments");
  *plan = nullptr;
  counts_host[0] = counts_host[1] = 0;
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> hb((size_t)n_seq), hn((size_t)n_seq), pre((size_t)n_seq + 1, 0);
  if (n_seq) {
    BX_HIPCHK(hipMemcpyAsync(hb.data(), base, (size_t)n_seq * 8, hipMemcpyDeviceToHost, st));
    BX_HIPCHK(hipMemcpyAsync(hn.data(), n, (size_t)n_seq * 8, hipMemcpyDeviceToHost, st));
    BX_HIPCHK(hipStreamSynchronize(st));
  }
  for (int q = 0; q < n_seq; q++) {
    if (hb[q] < 0 || hn[q] < 0)
      return gsi_err(BX_ERR_INVALID, "gsi: slot " + std::to_string(q) + " has a negative base or n");
    pre[q + 1] = pre[q] + hn[q];
    if (pre[q + 1] >= INT_MAX / 2)
      return gsi_err(BX_ERR_INVALID, "gsi: the slots hold too many rows for one call");
  }
  const int64_t R = pre[n_seq];
  if (R > 0 && !rows) return gsi_err(BX_ERR_INVALID, "gsi: null rows");
  DevicePlan* p = new DevicePlan;
  struct Guard {  // (released on success)
    DevicePlan* p;
    ~Guard() { delete p; }
  } guard{p};
  p->R = R;
  p->n_seq = n_seq;
  if (R > 0) {
    const PlanLayout l = plan_layout(R);
    void *d_pre, *d_counts, *d_packed;
    BX_HIPCHK(p->bufs.get(&d_pre, pre.size() * 8));
    BX_HIPCHK(p->bufs.get(&d_counts, 16));
    BX_HIPCHK(p->bufs.get(&d_packed, (size_t)R * 8 * sizeof(double)));
    BX_HIPCHK(p->bufs.get(&p->ws, l.total));
    p->packed = (double*)d_packed;
    BX_HIPCHK(hipMemcpyAsync(d_pre, pre.data(), pre.size() * 8, hipMemcpyHostToDevice, st));
    gsi_slot_pack_kernel<<<(l.P + 255) / 256, 256, 0, st>>>(
        rows, (long long)row_stride, (const long long*)base, (const long long*)d_pre, n_seq,
        (int)R, l.P, p->packed, (Key*)((char*)p->ws + l.keys));
    sort_scan(l, (int)R, interval, (char*)p->ws, (int64_t*)d_counts, st);
    BX_HIPCHK(hipGetLastError());
    BX_HIPCHK(hipMemcpyAsync(counts_host, d_counts, 16, hipMemcpyDeviceToHost, st));
    BX_HIPCHK(hipStreamSynchronize(st));
    if (counts_host[0] >= INT_MAX / 2)
      return gsi_err(BX_ERR_INVALID, "gsi: the interpolation yields too many rows for one call");
    p->n_out = counts_host[0];
    p->n_tracks = (int)counts_host[1];
  }
  guard.p = nullptr;
  *plan = p;
  return BX_OK;
}

int bx_gsi_device_run(void* plan, double tau, int truncate, double* out, int64_t cap,
                      int64_t* out_base, int64_t* out_n, void* stream) {
  DevicePlan* p = (DevicePlan*)plan;
  if (!p || cap < 0 || (p->n_seq > 0 && (!out_base || !out_n)))
    return gsi_err(BX_ERR_INVALID, "gsi: bad result-slot arguments");
  if (!(tau > 0.0)) return gsi_err(BX_ERR_INVALID, "gsi: tau must be positive");
  if (p->n_out > cap || (p->n_out > 0 && !out))
    return gsi_err(BX_ERR_CAPACITY, "gsi: output holds fewer rows than the interpolation yields");
  hipStream_t st = (hipStream_t)stream;
  if (p->n_out == 0) {  // no slot has a row
    if (p->n_seq) {
      BX_HIPCHK(hipMemsetAsync(out_base, 0, (size_t)p->n_seq * 8, st));
      BX_HIPCHK(hipMemsetAsync(out_n, 0, (size_t)p->n_seq * 8, st));
    }
    BX_HIPCHK(hipStreamSynchronize(st));
    return BX_OK;
  }
  const int nt = p->n_tracks, n_out = (int)p->n_out;
  void *d_interp, *d_oseq, *d_off, *d_status, *d_fail, *d_ws;
  BX_HIPCHK(p->bufs.get(&d_interp, (size_t)n_out * 8 * sizeof(double)));
  BX_HIPCHK(p->bufs.get(&d_oseq, (size_t)n_out * 4));
  BX_HIPCHK(p->bufs.get(&d_off, ((size_t)nt + 1) * 4));
  BX_HIPCHK(p->bufs.get(&d_status, (size_t)nt * 4));
  BX_HIPCHK(p->bufs.get(&d_fail, 4));
  if (const int rc = bx_gsi_interpolate(p->packed, p->R, 8, p->ws, (double*)d_interp,
                                        (int32_t*)d_oseq, n_out, (int32_t*)d_off, st))
    return rc;
  std::vector<int32_t> off((size_t)nt + 1);
  BX_HIPCHK(hipMemcpyAsync(off.data(), d_off, off.size() * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  size_t sbytes = 0;
  if (const int rc = bx_gsi_workspace_bytes(off.data(), nt, 0, &sbytes)) return rc;
  BX_HIPCHK(p->bufs.get(&d_ws, sbytes));
  if (const int rc = bx_gsi_smooth((const double*)d_interp, 8, off.data(), nt, tau, 0, d_ws, sbytes,
                                   out, (int32_t*)d_status, st))
    return rc;
  BX_HIPCHK(hipMemsetAsync(d_fail, 0x7f, 4, st));  // above any tracklet index
  const int threads = n_out > p->n_seq ? n_out : p->n_seq;  // (n_out >= nt)
  gsi_finalise_kernel<<<(threads + 255) / 256, 256, 0, st>>>(
      out, (const int32_t*)d_oseq, n_out, p->n_seq, truncate, (const int32_t*)d_status, nt,
      (long long*)out_base, (long long*)out_n, (int*)d_fail);
  BX_HIPCHK(hipGetLastError());
  int fail = 0;
  BX_HIPCHK(hipMemcpyAsync(&fail, d_fail, 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  if (fail < nt) {
    double id = 0.0;
    BX_HIPCHK(hipMemcpy(&id, (const double*)d_interp + (size_t)off[fail] * 8 + 1, 8,
                        hipMemcpyDeviceToHost));
    char ident[32];
    snprintf(ident, sizeof(ident), "%g", id);
    return gsi_err(BX_ERR_INVALID, std::string("the kernel matrix of id ") + ident + " (" +
                                       std::to_string(off[fail + 1] - off[fail]) +
                                       " rows) is not positive definite: duplicate or "
                                       "non-finite frames?");
  }
  return BX_OK;
}

int bx_gsi_device_free(void* plan) {
  delete (DevicePlan*)plan;
  return BX_OK;
}

}  // extern "C"
