// bx_eval.hip — MOT evaluation (include/bxeval.h): HOTA, CLEAR and Identity of MOT16/17/20
// pedestrian result rows against ground truth, the stage engine/val.py hands to a TrackEval
// subprocess.  The contract is DESIGN.md 2.13; this file is its device form.
//
// Host: rows are bucketed by (sequence, frame) and the raw ids of each side relabelled 0..n-1
// per sequence (sorted order).  Device, seven launches over the whole batch:
//   pre      one wave per (sequence, frame): the IoU tile, the preprocessing assignment, distractor
//            removal, compaction of the kept boxes (ids and their IoU tile) and per-id box counts
//   hota1    one workgroup per sequence walking its frames: pot (fixed frame order) and the
//            Identity co-occurrence counts
//   hota2    one wave per (sequence, frame): the assignment on G * iou, all 19 alphas from it
//   clear    one wave per sequence walking its frames (the recurrence is sequential)
//   identity one wave per sequence: the (GT_IDs + IDs)^2 assignment, state in LDS or HBM
//   finish   one workgroup per sequence: association sums (fixed tree), ratios
//   combine  one workgroup per group of sequences: its COMBINED
// bx_eval_run_device takes the tracker rows from device memory instead: four more launches
// (trcount, relabel, trscatter, trgather) bucket and relabel them there, against a ground truth
// made resident once by bx_eval_set_gt_host, for several groups of result sets at once.
// Every assignment is bx_jv.h's lapjv (register-resident up to 64, else state in LDS / HBM): an
// exact solver, so wherever the optimum's value-carrying pairs are unique they are scipy's.
// Integer counts use integer atomics; every floating-point sum runs in a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bxassoc.h"
#include "../../include/bxeval.h"
#include "bx_device.h"
#include "bx_host.h"


using namespace bx;

namespace {

#include "bx_jv.h"

int ev_err(int code, const std::string& msg) { return bx_record_error(code, msg.c_str()); }
constexpr int NA = BX_EVAL_NALPHA, NF = BX_EVAL_NF, LDS_N = BX_EVAL_LDS_N;
constexpr double EPS = DBL_EPSILON;
constexpr double ID_BIG = 1e10;  // fn and fp of an entry no assignment may use
constexpr int FT = 256;          // threads of the per-sequence walking / finishing workgroups

struct Alphas {
  double a[NA];
};

// Everything the kernels read or write; pointers into the handle's arena.
struct EvDev {
  int S, F, mot20;
  int gsz;                       // sequences of one group: a COMBINED record follows every gsz
  // per side rows, bucketed by (sequence, frame)
  const double *gbox, *tbox;     // [.][4] xywh
  const int *gid, *tid;          // relabelled id within the sequence
  const int *gcls, *gzm;         // gt class, zero_marked != 0
  const int *gfoff, *tfoff;      // [F + 1] row offsets of every frame
  const int* gsrc;               // [F] first row of a frame's gt in gbox / gid / gcls / gzm
                                 // (gfoff itself, or the resident gt's offsets for every group)
  const long long* ioff;         // [F + 1] offsets of the frames' gt x tracker tiles
  const int* fseq;               // [F] sequence of a frame
  const int* fbase;              // [S + 1] first frame of a sequence
  const int *gidoff, *tidoff;    // [S + 1] offsets of the sequences' id ranges
  const long long* moff;         // [S + 1] offsets of the sequences' gt-id x tracker-id matrices
  const long long* coff;         // [S + 1] offsets of the Identity cost matrices
  const long long* jvoff;        // [S] byte offset of a sequence's HBM solver state, -1: LDS
  // written by pre
  double *cst, *ksim;            // assignment costs (scratch, reused); kept IoU tiles
  int *kgid, *ktid, *nkg, *nkt;  // kept ids of a frame (compacted), their counts [F]
  int *gcount, *tcount;          // kept boxes per id
  // HOTA
  double* pot;
  int *idpot, *mc;               // mc: [NA] matrices, alpha-major
  long long mtot;                // entries of one alpha's mc
  int* ftp;                      // [F][NA] TPs of a frame
  double* floc;                  // [F][NA] their IoU sums
  // CLEAR
  int *prev, *prevt, *ptep, *mcount, *frag;
  double* clr;                   // [S][8]: TP FN FP IDSW MOTP_sum
  // Identity
  double* idc;
  unsigned char* jvg;
  int *gl, *tl;                  // kept id lists
  double* idr;                   // [S][8]: IDFN IDFP Dets GT_Dets IDs GT_IDs
  double* out;                   // [S / gsz][gsz + 1][NF]
};

// Record of sequence s: the groups' records lie one after another, each followed by COMBINED.
__device__ __forceinline__ double* ev_record(const EvDev& g, int s) {
  return g.out + (size_t)(s + s / g.gsz) * NF;
}

// IoU of two xywh boxes as the contract words it (areas from the corner form).
__device__ __forceinline__ double ev_iou(const double* a, const double* b) {
  const double ax1 = a[0] + a[2], ay1 = a[1] + a[3], bx1 = b[0] + b[2], by1 = b[1] + b[3];
  const double iw = fmax(fmin(ax1, bx1) - fmax(a[0], b[0]), 0.0);
  const double ih = fmax(fmin(ay1, by1) - fmax(a[1], b[1]), 0.0);
  double inter = iw * ih;
  const double aa = (ax1 - a[0]) * (ay1 - a[1]), ab = (bx1 - b[0]) * (by1 - b[1]);
  double uni = aa + ab - inter;
  if (aa <= EPS || ab <= EPS) inter = 0.0;
  if (uni <= EPS) inter = 0.0, uni = 1.0;
  return inter / uni;
}

__device__ __forceinline__ bool ev_distractor(int c, int mot20) {
  return c == 2 || c == 7 || c == 8 || c == 12 || (mot20 && c == 6);
}

// The solver state is carved for at least a wave's 64 columns (the register-resident solver
// hands its result over lane by lane).
__device__ __forceinline__ int ev_jv_n(int n) { return n > OW ? n : OW; }

// lapjv of the row-major nr x nc cost C (zero-padded to the square) by this one-wave workgroup,
// state in LDS: w.x[i] is row i's column, >= nc when it has none.
__device__ __forceinline__ void ev_solve(const double* C, int nr, int nc, JvLds& w) {
  if ((nr > nc ? nr : nc) <= OW)
    jv_wave64(C, nr, nc, w);
  else
    jv_wave(C, nr, nc, w, SyncBlock{});
  __syncthreads();
}

// LDS of the per-frame kernels: solver state for n <= cap, then three int arrays of cap.
__host__ __device__ constexpr size_t ev_frame_lds(int cap) {
  return ((jv_bytes(cap) + 15) / 16) * 16 + 3 * (size_t)cap * 4 + (size_t)cap * 8;
}

__global__ __launch_bounds__(OW) void ev_pre_kernel(EvDev g, int cap) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int s = g.fseq[f];
  const int g0 = g.gfoff[f], ng = g.gfoff[f + 1] - g0;
  const int gr = g.gsrc[f];  // (g0 unless the gt is shared between groups)
  const int t0 = g.tfoff[f], nt = g.tfoff[f + 1] - t0;
  int* rem = (int*)(smem + ((jv_bytes(cap) + 15) / 16) * 16);
  int* kgi = rem + cap;
  int* kti = kgi + cap;
  for (int j = lane; j < nt; j += OW) rem[j] = 0;
  __syncthreads();
  if (ng > 0 && nt > 0) {
    double* C = g.cst + g.ioff[f];
    for (int k = lane; k < ng * nt; k += OW) {
      const int i = k / nt, j = k - i * nt;
      const double v = ev_iou(g.gbox + 4 * (size_t)(gr + i), g.tbox + 4 * (size_t)(t0 + j));
      C[k] = -(v < 0.5 - EPS ? 0.0 : v);
    }
    __syncthreads();
    JvLds w = jv_bind(smem, ev_jv_n(ng > nt ? ng : nt));
    ev_solve(C, ng, nt, w);
    for (int i = lane; i < ng; i += OW) {
      const int j = w.x[i];
      if (j >= 0 && j < nt && -C[i * nt + j] > EPS && ev_distractor(g.gcls[gr + i], g.mot20))
        rem[j] = 1;  // (a column has one row: no two lanes write one flag)
    }
    __syncthreads();
  }
  const int a = wave_compact(
      ng, [&](int i) { return g.gzm[gr + i] != 0 && g.gcls[gr + i] == 1; },
      [&](int i, int p) { kgi[p] = i; });
  const int b = wave_compact(nt, [&](int j) { return rem[j] == 0; }, [&](int j, int p) { kti[p] = j; });
  for (int p = lane; p < a; p += OW) {
    const int id = g.gid[gr + kgi[p]];
    g.kgid[g0 + p] = id;
    atomicAdd(&g.gcount[g.gidoff[s] + id], 1);
  }
  for (int q = lane; q < b; q += OW) {
    const int id = g.tid[t0 + kti[q]];
    g.ktid[t0 + q] = id;
    atomicAdd(&g.tcount[g.tidoff[s] + id], 1);
  }
  if (lane == 0) g.nkg[f] = a, g.nkt[f] = b;
  double* K = g.ksim + g.ioff[f];
  for (int k = lane; k < a * b; k += OW) {
    const int p = k / b, q = k - p * b;
    K[k] = ev_iou(g.gbox + 4 * (size_t)(gr + kgi[p]), g.tbox + 4 * (size_t)(t0 + kti[q]));
  }
}

// HOTA pass 1 and the Identity co-occurrence counts: frames in order; within a frame every
// (gt id, tracker id) pair occurs once, so the entries of one frame are independent.
__global__ __launch_bounds__(FT) void ev_hota1_kernel(EvDev g, int cap) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* rs = (double*)smem;
  double* cs = rs + cap;
  const int s = blockIdx.x, t = threadIdx.x;
  const int ntid = g.tidoff[s + 1] - g.tidoff[s];
  double* pot = g.pot + g.moff[s];
  int* idpot = g.idpot + g.moff[s];
  for (int f = g.fbase[s]; f < g.fbase[s + 1]; f++) {
    const int a = g.nkg[f], b = g.nkt[f];
    if (a == 0 || b == 0) continue;
    const double* K = g.ksim + g.ioff[f];
    const int* gi = g.kgid + g.gfoff[f];
    const int* ti = g.ktid + g.tfoff[f];
    for (int p = t; p < a; p += FT) {
      double r = 0.0;
      for (int q = 0; q < b; q++) r += K[p * b + q];
      rs[p] = r;
    }
    for (int q = t; q < b; q += FT) {
      double c = 0.0;
      for (int p = 0; p < a; p++) c += K[p * b + q];
      cs[q] = c;
    }
    __syncthreads();
    for (int k = t; k < a * b; k += FT) {
      const int p = k / b, q = k - p * b;
      const double v = K[k];
      const double den = rs[p] + cs[q] - v;
      const size_t e = (size_t)gi[p] * ntid + ti[q];
      if (den > EPS) pot[e] += v / den;
      if (v >= 0.5 - EPS) idpot[e] += 1;
    }
    __syncthreads();
  }
}

// HOTA pass 2: the frame's assignment on G * iou; lanes 0..18 then tally one alpha each, in row
// order.
__global__ __launch_bounds__(OW) void ev_hota2_kernel(EvDev g, int cap, Alphas al) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int a = g.nkg[f], b = g.nkt[f];
  if (a == 0 || b == 0) return;  // (ftp / floc stay zero)
  const int s = g.fseq[f];
  int* mcol = (int*)(smem + ((jv_bytes(cap) + 15) / 16) * 16);
  double* miou = (double*)(mcol + 3 * cap);
  const int ntid = g.tidoff[s + 1] - g.tidoff[s];
  const double* pot = g.pot + g.moff[s];
  const int* gc = g.gcount + g.gidoff[s];
  const int* tc = g.tcount + g.tidoff[s];
  const double* K = g.ksim + g.ioff[f];
  const int* gi = g.kgid + g.gfoff[f];
  const int* ti = g.ktid + g.tfoff[f];
  double* C = g.cst + g.ioff[f];
  for (int k = lane; k < a * b; k += OW) {
    const int p = k / b, q = k - p * b;
    const double pm = pot[(size_t)gi[p] * ntid + ti[q]];
    const double G = pm / ((double)gc[gi[p]] + (double)tc[ti[q]] - pm);
    C[k] = -(G * K[k]);
  }
  __syncthreads();
  JvLds w = jv_bind(smem, ev_jv_n(a > b ? a : b));
  ev_solve(C, a, b, w);
  for (int p = lane; p < a; p += OW) {
    const int q = w.x[p];
    const bool m = q >= 0 && q < b;
    mcol[p] = m ? q : -1;
    miou[p] = m ? K[p * b + q] : -1.0;
  }
  __syncthreads();
  if (lane < NA) {
    const double thr = al.a[lane] - EPS;
    int* mc = g.mc + (size_t)lane * g.mtot + g.moff[s];
    int tp = 0;
    double loc = 0.0;
    for (int p = 0; p < a; p++) {
      const double v = miou[p];
      if (mcol[p] >= 0 && v >= thr) {
        tp++;
        loc += v;
        atomicAdd(&mc[(size_t)gi[p] * ntid + ti[mcol[p]]], 1);
      }
    }
    g.ftp[(size_t)f * NA + lane] = tp;
    g.floc[(size_t)f * NA + lane] = loc;
  }
}

// CLEAR: one wave walks the sequence.  prev_t is valid where its epoch is the last rebuild's.
__global__ __launch_bounds__(OW) void ev_clear_kernel(EvDev g, int cap) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int s = blockIdx.x, lane = threadIdx.x;
  int* mcol = (int*)(smem + ((jv_bytes(cap) + 15) / 16) * 16);
  double* miou = (double*)(mcol + 3 * cap);
  int* prev = g.prev + g.gidoff[s];
  int* prevt = g.prevt + g.gidoff[s];
  int* ptep = g.ptep + g.gidoff[s];
  int* mcount = g.mcount + g.gidoff[s];
  int* frag = g.frag + g.gidoff[s];
  long long tp = 0, fn = 0, fp = 0, idsw = 0;
  double motp = 0.0;
  int epoch = 0;
  for (int f = g.fbase[s]; f < g.fbase[s + 1]; f++) {
    const int a = g.nkg[f], b = g.nkt[f];
    if (a == 0) {
      fp += b;
      continue;
    }
    if (b == 0) {
      fn += a;
      epoch++;  // (cleared: a rebuild from no match)
      continue;
    }
    const double* K = g.ksim + g.ioff[f];
    const int* gi = g.kgid + g.gfoff[f];
    const int* ti = g.ktid + g.tfoff[f];
    double* C = g.cst + g.ioff[f];
    for (int k = lane; k < a * b; k += OW) {
      const int p = k / b, q = k - p * b;
      const int gidx = gi[p];
      const bool same = epoch > 0 && ptep[gidx] == epoch && prevt[gidx] == ti[q];
      const double v = K[k];
      double sc = (same ? 1000.0 : 0.0) + v;
      if (v < 0.5 - EPS) sc = 0.0;
      C[k] = -sc;
    }
    __syncthreads();
    JvLds w = jv_bind(smem, ev_jv_n(a > b ? a : b));
    ev_solve(C, a, b, w);
    int n_m = 0, n_sw = 0;
    for (int c = 0; c < a; c += OW) {
      const int p = c + lane;
      bool m = false, sw = false;
      if (p < a) {
        const int q = w.x[p];
        m = q >= 0 && q < b && -C[p * b + q] > EPS;
        miou[p] = m ? K[p * b + q] : -1.0;
        if (m) {
          const int gidx = gi[p], tq = ti[q];
          sw = prev[gidx] >= 0 && prev[gidx] != tq;
          mcount[gidx] += 1;
          if (!(epoch > 0 && ptep[gidx] == epoch)) frag[gidx] += 1;
          prev[gidx] = tq;
          prevt[gidx] = tq;
          ptep[gidx] = epoch + 1;
        }
      }
      n_m += __popcll(__ballot(m));
      n_sw += __popcll(__ballot(sw));
    }
    __syncthreads();
    for (int p = 0; p < a; p++)  // (every lane the same sum, in row order)
      if (miou[p] >= 0.0) motp += miou[p];
    epoch++;
    tp += n_m;
    fn += a - n_m;
    fp += b - n_m;
    idsw += n_sw;
    __syncthreads();
  }
  if (lane == 0) {
    double* o = g.clr + 8 * (size_t)s;
    o[0] = (double)tp, o[1] = (double)fn, o[2] = (double)fp, o[3] = (double)idsw, o[4] = motp;
  }
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Identity: the ids with kept boxes, the (GT_IDs + IDs)^2 problem, its lapjv.
__global__ __launch_bounds__(OW) void ev_identity_kernel(EvDev g) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int ngid = g.gidoff[s + 1] - g.gidoff[s], ntid = g.tidoff[s + 1] - g.tidoff[s];
  const int* gc = g.gcount + g.gidoff[s];
  const int* tc = g.tcount + g.tidoff[s];
  int* gl = g.gl + g.gidoff[s];
  int* tl = g.tl + g.tidoff[s];
  const int G = wave_compact(ngid, [&](int i) { return gc[i] > 0; }, [&](int i, int p) { gl[p] = i; });
  const int T = wave_compact(ntid, [&](int j) { return tc[j] > 0; }, [&](int j, int p) { tl[p] = j; });
  long long gd = 0, td = 0;
  for (int i = lane; i < ngid; i += OW) gd += gc[i];
  for (int j = lane; j < ntid; j += OW) td += tc[j];
  gd = wave_sum_ll(gd);
  td = wave_sum_ll(td);
  long long idfn = 0, idfp = 0;
  if (G == 0 || T == 0) {
    idfn = gd;  // no tracker box: every gt box is an IDFN; no gt box: every tracker box an IDFP
    idfp = td;
  } else {
    const int n = G + T;
    const int* idpot = g.idpot + g.moff[s];
    double* C = g.idc + g.coff[s];
    for (size_t k = lane; k < (size_t)n * n; k += OW) {
      const int i = (int)(k / n), j = (int)(k - (size_t)i * n);
      double fnv, fpv;
      if (i < G && j < T) {
        const int pm = idpot[(size_t)gl[i] * ntid + tl[j]];
        fnv = (double)(gc[gl[i]] - pm);
        fpv = (double)(tc[tl[j]] - pm);
      } else if (i < G) {
        fnv = j == T + i ? (double)gc[gl[i]] : ID_BIG;
        fpv = j == T + i ? 0.0 : ID_BIG;
      } else if (j < T) {
        fnv = i == G + j ? 0.0 : ID_BIG;
        fpv = i == G + j ? (double)tc[tl[j]] : ID_BIG;
      } else {
        fnv = fpv = 0.0;
      }
      C[k] = fnv + fpv;
    }
    __syncthreads();
    const long long jo = g.jvoff[s];
    JvLds w = jv_bind(jo >= 0 ? g.jvg + jo : smem, ev_jv_n(n));
    if (n <= OW)
      jv_wave64(C, n, n, w);
    else if (jo >= 0)
      jv_wave(C, n, n, w, SyncWaveG{});
    else
      jv_wave(C, n, n, w, SyncBlock{});
    __syncthreads();
    for (int i = lane; i < G; i += OW) {
      const int j = w.x[i];
      idfn += gc[gl[i]] - (j >= 0 && j < T ? idpot[(size_t)gl[i] * ntid + tl[j]] : 0);
    }
    for (int j = lane; j < T; j += OW) {
      const int i = w.y[j];
      idfp += tc[tl[j]] - (i >= 0 && i < G ? idpot[(size_t)gl[i] * ntid + tl[j]] : 0);
    }
    idfn = wave_sum_ll(idfn);
    idfp = wave_sum_ll(idfp);
  }
  if (lane == 0) {
    double* o = g.idr + 8 * (size_t)s;
    o[0] = (double)idfn, o[1] = (double)idfp, o[2] = (double)td, o[3] = (double)gd;
    o[4] = (double)T, o[5] = (double)G;
  }
}

// Sum of one value per thread over the workgroup in a fixed tree; the result in every thread.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int d = FT / 2; d > 0; d >>= 1) {
    if (t < d) red[t] += red[t + d];
    __syncthreads();
  }
  return red[0];
}

// The ratio fields of one record from its counts and sums (a sequence's, or COMBINED's).
__device__ void ev_hota_final(double* o, int a) {
  const double tp = o[BX_EVAL_H_TP + a], fn = o[BX_EVAL_H_FN + a], fp = o[BX_EVAL_H_FP + a];
  const double deta = tp / fmax(1.0, tp + fn + fp);
  o[BX_EVAL_H_DETA + a] = deta;
  o[BX_EVAL_H_DETRE + a] = tp / fmax(1.0, tp + fn);
  o[BX_EVAL_H_DETPR + a] = tp / fmax(1.0, tp + fp);
  o[BX_EVAL_H_HOTA + a] = sqrt(deta * o[BX_EVAL_H_ASSA + a]);
}
__device__ void ev_clear_final(double* c, bool degenerate) {
  const double tp = c[0], fn = c[1], fp = c[2], idsw = c[3], mt = c[4], pt = c[5], ml = c[6];
  const double motp = c[8];
  const double gt = fmax(1.0, tp + fn), ids = fmax(1.0, mt + pt + ml);
  c[10] = (tp - fp - idsw) / gt;
  c[11] = motp / fmax(1.0, tp);
  c[12] = (tp - fp) / gt;
  c[13] = (motp - fp - idsw) / gt;
  c[14] = tp / gt;
  c[15] = tp / fmax(1.0, tp + fp);
  c[16] = mt / ids;
  c[17] = pt / ids;
  c[18] = degenerate ? 1.0 : ml / ids;
}
__device__ void ev_id_final(double* d) {
  const double idtp = d[0], idfn = d[1], idfp = d[2];
  d[3] = idtp / fmax(1.0, idtp + 0.5 * idfp + 0.5 * idfn);
  d[4] = idtp / fmax(1.0, idtp + idfn);
  d[5] = idtp / fmax(1.0, idtp + idfp);
}

__global__ __launch_bounds__(FT) void ev_finish_kernel(EvDev g) {
  __shared__ double red[FT];
  __shared__ int cnt[4];
  const int s = blockIdx.x, t = threadIdx.x;
  double* o = ev_record(g, s);
  const int ngid = g.gidoff[s + 1] - g.gidoff[s], ntid = g.tidoff[s + 1] - g.tidoff[s];
  const int* gc = g.gcount + g.gidoff[s];
  const int* tc = g.tcount + g.tidoff[s];
  const double* idr = g.idr + 8 * (size_t)s;
  const double dets = idr[2], gdets = idr[3], nids = idr[4], ngids = idr[5];
  const bool degenerate = dets == 0.0 || gdets == 0.0;
  // HOTA: per alpha the frames' TPs and IoU sums in frame order
  if (t < NA) {
    long long tp = 0;
    double loc = 0.0;
    for (int f = g.fbase[s]; f < g.fbase[s + 1]; f++) {
      tp += g.ftp[(size_t)f * NA + t];
      loc += g.floc[(size_t)f * NA + t];
    }
    o[BX_EVAL_H_TP + t] = (double)tp;
    o[BX_EVAL_H_FN + t] = gdets - (double)tp;
    o[BX_EVAL_H_FP + t] = dets - (double)tp;
    o[BX_EVAL_H_LOCA + t] = degenerate ? 1.0 : loc / fmax(1e-10, (double)tp);
  }
  __syncthreads();
  const size_t M = (size_t)ngid * ntid;
  for (int a = 0; a < NA; a++) {
    const int* mc = g.mc + (size_t)a * g.mtot + g.moff[s];
    double sa = 0.0, sr = 0.0, sp = 0.0;
    for (size_t e = t; e < M; e += FT) {
      const int m = mc[e];
      if (m == 0) continue;
      const int i = (int)(e / ntid), j = (int)(e - (size_t)i * ntid);
      const double dm = (double)m, dg = (double)gc[i], dt = (double)tc[j];
      sa += dm * (dm / fmax(1.0, dg + dt - dm));
      sr += dm * (dm / fmax(1.0, dg));
      sp += dm * (dm / fmax(1.0, dt));
    }
    sa = block_sum(sa, red);
    sr = block_sum(sr, red);
    sp = block_sum(sp, red);
    if (t == 0) {
      const double tp = fmax(1.0, o[BX_EVAL_H_TP + a]);
      o[BX_EVAL_H_ASSA + a] = sa / tp;
      o[BX_EVAL_H_ASSRE + a] = sr / tp;
      o[BX_EVAL_H_ASSPR + a] = sp / tp;
      ev_hota_final(o, a);
    }
  }
  // CLEAR: MT / PT / Frag over the ids with boxes
  if (t < 4) cnt[t] = 0;
  __syncthreads();
  const int* mcount = g.mcount + g.gidoff[s];
  const int* frag = g.frag + g.gidoff[s];
  for (int i = t; i < ngid; i += FT) {
    if (gc[i] == 0) continue;
    const double r = (double)mcount[i] / (double)gc[i];
    if (r > 0.8) atomicAdd(&cnt[0], 1);
    if (r >= 0.2) atomicAdd(&cnt[1], 1);
    if (frag[i] > 0) atomicAdd(&cnt[2], frag[i] - 1);
  }
  __syncthreads();
  if (t == 0) {
    double* c = o + BX_EVAL_CLEAR;
    const double* cl = g.clr + 8 * (size_t)s;
    const double mt = (double)cnt[0], pt = (double)(cnt[1] - cnt[0]);
    c[0] = cl[0], c[1] = cl[1], c[2] = cl[2], c[3] = cl[3];
    c[4] = mt, c[5] = pt, c[6] = ngids - mt - pt, c[7] = (double)cnt[2];
    c[8] = cl[4];
    c[9] = degenerate ? 0.0 : (double)(g.fbase[s + 1] - g.fbase[s]);
    ev_clear_final(c, degenerate);
    double* d = o + BX_EVAL_IDENTITY;
    d[1] = idr[0], d[2] = idr[1], d[0] = gdets - idr[0];
    ev_id_final(d);
    double* n = o + BX_EVAL_COUNT;
    n[0] = dets, n[1] = gdets, n[2] = nids, n[3] = ngids;
  }
}

// COMBINED of group blockIdx.x (record gsz of the group): sums over its sequences in order,
// weighted means, ratios recomputed.
__global__ __launch_bounds__(OW) void ev_combine_kernel(EvDev g) {
  const int t = threadIdx.x, S = g.gsz;
  const double* recs = g.out + (size_t)blockIdx.x * (S + 1) * NF;
  double* o = g.out + ((size_t)blockIdx.x * (S + 1) + S) * NF;
  if (t < NA) {
    double tp = 0, fn = 0, fp = 0, wa = 0, wr = 0, wp = 0, wl = 0;
    for (int s = 0; s < S; s++) {
      const double* r = recs + (size_t)s * NF;
      const double w = r[BX_EVAL_H_TP + t];
      tp += w, fn += r[BX_EVAL_H_FN + t], fp += r[BX_EVAL_H_FP + t];
      wa += r[BX_EVAL_H_ASSA + t] * w;
      wr += r[BX_EVAL_H_ASSRE + t] * w;
      wp += r[BX_EVAL_H_ASSPR + t] * w;
      wl += r[BX_EVAL_H_LOCA + t] * w;
    }
    o[BX_EVAL_H_TP + t] = tp, o[BX_EVAL_H_FN + t] = fn, o[BX_EVAL_H_FP + t] = fp;
    o[BX_EVAL_H_ASSA + t] = wa / fmax(1.0, tp);
    o[BX_EVAL_H_ASSRE + t] = wr / fmax(1.0, tp);
    o[BX_EVAL_H_ASSPR + t] = wp / fmax(1.0, tp);
    o[BX_EVAL_H_LOCA + t] = tp == 0.0 ? 1.0 : wl / tp;
    ev_hota_final(o, t);
  }
  if (t == 32) {
    double* c = o + BX_EVAL_CLEAR;
    double* d = o + BX_EVAL_IDENTITY;
    double* n = o + BX_EVAL_COUNT;
    for (int k = 0; k < 10; k++) c[k] = 0.0;
    for (int k = 0; k < 3; k++) d[k] = 0.0;
    for (int k = 0; k < 4; k++) n[k] = 0.0;
    for (int s = 0; s < S; s++) {
      const double* r = recs + (size_t)s * NF;
      for (int k = 0; k < 10; k++) c[k] += r[BX_EVAL_CLEAR + k];
      for (int k = 0; k < 3; k++) d[k] += r[BX_EVAL_IDENTITY + k];
      for (int k = 0; k < 4; k++) n[k] += r[BX_EVAL_COUNT + k];
    }
    ev_clear_final(c, false);
    ev_id_final(d);
  }
}

// ------------------------------------------------------- tracker rows from device memory
// bx_eval_run_device buckets and relabels the tracker side on the device (the host path's
// bucket_side): count + validate, relabel, scatter, gather.  Input errors are latched, never
// acted on: one 64-bit key, smallest first, ordered as bucket_side meets them (sequence, then
// stage, then row), so the status is the host path's.
struct TrIn {
  const double* rows;     // [.][stride]: frame, id, x, y, w, h, ...
  long long stride;
  const long long *base;  // [Q] first row of a sequence
  const long long *n;     // [Q] its rows
};

constexpr unsigned long long EV_NOERR = ~0ull;
constexpr long long TAB_EMPTY = 0x7f7f7f7f7f7f7f7fll;  // a byte pattern beyond every valid id
constexpr int CT = 256;    // threads of the count / scatter workgroups
constexpr int CB = 8;      // their workgroups per sequence
constexpr int RT = 1024;   // threads of the per-sequence relabel workgroup
enum { ST_RANGE = 0, ST_ROW = 1, ST_IDS = 2, ST_BOXES = 3, ST_TWICE = 4 };

__device__ __forceinline__ void ev_latch(unsigned long long* latch, int q, int stage, long long row,
                                         int kind) {
  atomicMin(latch, ((unsigned long long)q << 44) | ((unsigned long long)stage << 41) |
                       (((unsigned long long)row & ((1ull << 40) - 1)) << 1) |
                       (unsigned long long)kind);
}
__device__ __forceinline__ bool ev_frame_ok(double fr, int T) {
  return fr >= 1.0 && fr <= (double)T && fr == floor(fr);
}
__device__ __forceinline__ bool ev_id_ok(double idv) { return idv == floor(idv) && fabs(idv) < 9e15; }

// Rows per (sequence, frame), every row validated.  Workgroups q * CB .. q * CB + CB - 1 stride
// over the rows of sequence q.
__global__ __launch_bounds__(CT) void ev_trcount_kernel(TrIn in, const int* fbase, int max_boxes,
                                                        int* cnt, unsigned long long* latch) {
  const int q = blockIdx.x / CB, c = blockIdx.x - q * CB;
  const long long b = in.base[q], n = in.n[q];
  if (b < 0 || n < 0 || n >= INT_MAX / 4) {
    if (c == 0 && threadIdx.x == 0) {
      if (b < 0 || n < 0)
        ev_latch(latch, q, ST_RANGE, 0, 0);
      else
        ev_latch(latch, q, ST_BOXES, 0, 1);
    }
    return;
  }
  const int f0 = fbase[q], T = fbase[q + 1] - f0;
  for (long long k = (long long)c * CT + threadIdx.x; k < n; k += CB * CT) {
    const double* r = in.rows + (b + k) * in.stride;
    const double fr = r[0];
    if (!ev_frame_ok(fr, T)) {
      ev_latch(latch, q, ST_ROW, k, 0);
      continue;
    }
    if (!ev_id_ok(r[1])) ev_latch(latch, q, ST_ROW, k, 1);
    const int t = (int)fr - 1;
    if (atomicAdd(&cnt[f0 + t], 1) == max_boxes) ev_latch(latch, q, ST_BOXES, t + 1, 0);
  }
}

// Sorted distinct ids of sequence blockIdx.x: deduplicated into its open-addressing table
// (tab_n slots, a power of two), compacted into LDS, sorted by a bitonic network over the padded
// power of two and written back over the table's first nid[q] slots.  A row's label is its id's
// rank there (ev_trgather_kernel).
__global__ __launch_bounds__(RT) void ev_relabel_kernel(TrIn in, long long* tab, int tab_n,
                                                        int max_ids, int* nid,
                                                        unsigned long long* latch) {
  extern __shared__ __align__(16) unsigned char smem[];
  long long* sk = (long long*)smem;
  __shared__ int nd, nc, over;
  const int q = blockIdx.x, t = threadIdx.x;
  const long long b = in.base[q], n = in.n[q];
  if (b < 0 || n < 0 || n >= INT_MAX / 4) return;  // (latched by the count; nid[q] stays 0)
  long long* tb = tab + (size_t)q * tab_n;
  if (t == 0) nd = 0, nc = 0, over = 0;
  __syncthreads();
  for (long long k = t; k < n; k += RT) {
    const double idv = in.rows[(b + k) * in.stride + 1];
    if (!ev_id_ok(idv)) continue;  // (latched by the count)
    if (*(volatile int*)&nd > max_ids) break;
    const long long id = (long long)idv;
    unsigned h = (unsigned)(((unsigned long long)id * 0x9E3779B97F4A7C15ull) >> 40) & (tab_n - 1);
    int probe = 0;
    for (; probe < tab_n; probe++) {
      long long cur = __hip_atomic_load(&tb[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == TAB_EMPTY) {
        cur = (long long)atomicCAS((unsigned long long*)&tb[h], (unsigned long long)TAB_EMPTY,
                                   (unsigned long long)id);
        if (cur == TAB_EMPTY) {
          atomicAdd(&nd, 1);
          break;
        }
      }
      if (cur == id) break;
      h = (h + 1) & (tab_n - 1);
    }
    if (probe == tab_n) over = 1;
  }
  __syncthreads();
  const int D = nd;
  if (D > max_ids || over) {
    if (t == 0) ev_latch(latch, q, ST_IDS, 0, 0);
    return;
  }
  int P = 1;
  while (P < D) P <<= 1;
  for (int i = t; i < P; i += RT) sk[i] = LLONG_MAX;
  __syncthreads();
  for (int h = t; h < tab_n; h += RT) {
    const long long v = __hip_atomic_load(&tb[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v != TAB_EMPTY) sk[atomicAdd(&nc, 1)] = v;  // (nc ends at D <= P)
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += RT) {
        const int x = i ^ j;
        if (x > i) {
          const long long a = sk[i], c = sk[x];
          if ((a > c) == ((i & k) == 0)) sk[i] = c, sk[x] = a;
        }
      }
      __syncthreads();
    }
  for (int i = t; i < D; i += RT) tb[i] = sk[i];
  if (t == 0) nid[q] = D;
}

// Source index (within the sequence) of every valid row into its frame's bucket, in arrival
// order; ev_trgather_kernel restores the source order.
__global__ __launch_bounds__(CT) void ev_trscatter_kernel(TrIn in, const int* fbase, const int* tfoff,
                                                          int* fill, int* src) {
  const int q = blockIdx.x / CB, c = blockIdx.x - q * CB;
  const long long b = in.base[q], n = in.n[q];
  if (b < 0 || n < 0 || n >= INT_MAX / 4) return;
  const int f0 = fbase[q], T = fbase[q + 1] - f0;
  for (long long k = (long long)c * CT + threadIdx.x; k < n; k += CB * CT) {
    const double fr = in.rows[(b + k) * in.stride];
    if (!ev_frame_ok(fr, T)) continue;
    const int f = f0 + (int)fr - 1;
    src[tfoff[f] + atomicAdd(&fill[f], 1)] = (int)k;
  }
}

// One wave per frame: its source indices sorted in LDS (the host's stable counting sort keeps
// source order within a frame), boxes gathered, ids ranked by binary search in the sequence's
// sorted ids, an id twice in the frame latched.  pw: the padded power of two of the LDS sort.
__global__ __launch_bounds__(OW) void ev_trgather_kernel(TrIn in, const int* fseq, const int* fbase,
                                                         const int* tfoff, const int* src,
                                                         const long long* tab, int tab_n,
                                                         const int* nid, int max_boxes, int pw,
                                                         double* tbox, int* tid,
                                                         unsigned long long* latch) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* idx = (int*)smem;
  int* lab = idx + pw;
  const int f = blockIdx.x, lane = threadIdx.x;
  const int t0 = tfoff[f], nt = tfoff[f + 1] - t0;
  if (nt == 0 || nt > max_boxes) return;  // (over capacity: latched by the count)
  const int q = fseq[f];
  int P = 1;
  while (P < nt) P <<= 1;
  for (int i = lane; i < P; i += OW) idx[i] = i < nt ? src[t0 + i] : INT_MAX;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < P; i += OW) {
        const int x = i ^ j;
        if (x > i) {
          const int a = idx[i], c = idx[x];
          if ((a > c) == ((i & k) == 0)) idx[i] = c, idx[x] = a;
        }
      }
      __syncthreads();
    }
  const long long* U = tab + (size_t)q * tab_n;
  const int D = nid[q];
  const long long b = in.base[q];
  for (int j = lane; j < nt; j += OW) {
    const double* r = in.rows + (b + idx[j]) * in.stride;
    double* o = tbox + 4 * (size_t)(t0 + j);
    o[0] = r[2], o[1] = r[3], o[2] = r[4], o[3] = r[5];
    const long long id = (long long)r[1];
    int lo = 0, hi = D;
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (U[m] < id)
        lo = m + 1;
      else
        hi = m;
    }
    if (lo >= D) lo = D > 0 ? D - 1 : 0;  // (only where the sequence is latched already)
    tid[t0 + j] = lo;
    lab[j] = lo;
  }
  __syncthreads();
  bool twice = false;
  for (int j = lane; j < nt; j += OW)
    for (int i = 0; i < j; i++) twice |= lab[i] == lab[j];
  if (twice) ev_latch(latch, q, ST_TWICE, f - fbase[q] + 1, 0);
}

// -------------------------------------------------------------------------------- host side
struct Eval {
  int max_boxes, max_ids, max_frames;
  void* arena = nullptr;
  size_t arena_bytes = 0;
  // the resident ground truth of bx_eval_set_gt_host: its own allocation (box, id, cls, zm) and
  // the host-side offsets of its S sequences
  void* gt = nullptr;
  int gt_S = 0, gt_rows = 0, gt_cap = 0;  // gt_cap: most gt rows in one frame
  size_t gt_o_id = 0, gt_o_cls = 0, gt_o_zm = 0;
  std::vector<int> gt_frames, gt_fbase, gt_foff, gt_idoff;
  // bx_eval_run_device's buffers ahead of the arena carve: fbase, counts, latch, id tables
  void* front = nullptr;
  size_t front_bytes = 0;
};

// One side's rows bucketed by (sequence, frame), ids relabelled per sequence.
struct Side {
  std::vector<double> box;
  std::vector<int> id, cls, zm, foff, idoff;
};

int bucket_side(const Eval& E, const char* what, int S, const int32_t* frames, const int* fbase,
                const int64_t* off, const double* rows, int ncol, bool gt, Side& o) {
  const int F = fbase[S];
  const int64_t R = off[S];
  o.box.resize((size_t)R * 4);
  o.id.resize(R);
  if (gt) o.cls.resize(R), o.zm.resize(R);
  o.foff.assign(F + 1, 0);
  o.idoff.assign(S + 1, 0);
  std::vector<long long> ids;
  std::vector<int> fill, seen;
  for (int s = 0; s < S; s++) {
    const int T = frames[s];
    const double* r0 = rows + (size_t)off[s] * ncol;
    const int64_t n = off[s + 1] - off[s];
    if (n < 0) return ev_err(BX_ERR_INVALID, std::string(what) + ": offsets must not decrease");
    ids.resize(n);
    for (int64_t k = 0; k < n; k++) {
      const double fr = r0[k * ncol], idv = r0[k * ncol + 1];
      if (!(fr >= 1.0 && fr <= (double)T) || fr != std::floor(fr))
        return ev_err(BX_ERR_INVALID, std::string(what) + ": sequence " + std::to_string(s) +
                                          " has frame " + std::to_string(fr) + " outside 1.." +
                                          std::to_string(T));
      if (idv != std::floor(idv) || !(std::fabs(idv) < 9e15))
        return ev_err(BX_ERR_INVALID, std::string(what) + ": sequence " + std::to_string(s) +
                                          " has a non-integer id");
      ids[k] = (long long)idv;
      o.foff[fbase[s] + (int)fr - 1 + 1]++;
    }
    std::vector<long long> uniq(ids);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    if ((int64_t)uniq.size() > E.max_ids)
      return ev_err(BX_ERR_CAPACITY, std::string(what) + ": sequence " + std::to_string(s) + " has " +
                                         std::to_string(uniq.size()) + " ids, capacity " +
                                         std::to_string(E.max_ids));
    o.idoff[s + 1] = o.idoff[s] + (int)uniq.size();
    for (int64_t k = 0; k < n; k++)
      ids[k] = std::lower_bound(uniq.begin(), uniq.end(), ids[k]) - uniq.begin();
    // counts -> offsets of this sequence's frames (foff[f + 1] holds frame f's count so far)
    for (int t = 0; t < T; t++) {
      const int f = fbase[s] + t;
      if (o.foff[f + 1] > E.max_boxes)
        return ev_err(BX_ERR_CAPACITY, std::string(what) + ": sequence " + std::to_string(s) +
                                           " frame " + std::to_string(t + 1) + " has " +
                                           std::to_string(o.foff[f + 1]) + " boxes, capacity " +
                                           std::to_string(E.max_boxes));
      o.foff[f + 1] += o.foff[f];
    }
    fill.assign(T, 0);
    seen.assign(uniq.size(), -1);
    for (int64_t k = 0; k < n; k++) {
      const double* r = r0 + k * ncol;
      const int t = (int)r[0] - 1;
      const int dst = o.foff[fbase[s] + t] + fill[t]++;
      for (int c = 0; c < 4; c++) o.box[(size_t)dst * 4 + c] = r[2 + c];
      o.id[dst] = (int)ids[k];
      if (gt) o.zm[dst] = r[6] != 0.0, o.cls[dst] = (int)r[7];
    }
    for (int t = 0; t < T; t++)
      for (int k = o.foff[fbase[s] + t]; k < o.foff[fbase[s] + t + 1]; k++) {
        if (seen[o.id[k]] == t)
          return ev_err(BX_ERR_INVALID, std::string(what) + ": sequence " + std::to_string(s) +
                                            " frame " + std::to_string(t + 1) + " has id " +
                                            std::to_string(uniq[o.id[k]]) + " twice");
        seen[o.id[k]] = t;
      }
  }
  return BX_OK;
}

// Arena layout: every buffer 256-byte aligned; `zero` buffers are cleared before a run.
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256 + 256;
    return o;
  }
};

// Grow-only device allocation of a handle.
int ev_reserve(void*& p, size_t& have, size_t need, const char* who) {
  if (need <= have) return BX_OK;
  if (p) BX_HIPCHK(hipFree(p));
  p = nullptr, have = 0;
  if (hipMalloc(&p, need) != hipSuccess) {
    p = nullptr;
    return ev_err(BX_ERR_HIP, std::string(who) + ": hipMalloc of " + std::to_string(need) +
                                  " bytes failed");
  }
  have = need;
  return BX_OK;
}

// A batch with both sides' offsets known on the host: S sequences in groups of gsz.
struct Batch {
  int S, F, gsz, benchmark;
  const int *fbase, *gfoff, *tfoff, *gidoff, *tidoff;  // [S + 1], [F + 1], [F + 1], [S + 1] x 2
  int NG, NT;    // rows of the two sides (NG counts every group's gt)
  int NGd;       // gt rows kept in the arena (0: the resident gt is read in place)
  int cap;       // most rows of one side in a frame
  bool metrics;  // false: bucket the tracker rows only (an input error is already latched)
};
// Where the arena keeps what the caller fills in.
struct Offs {
  size_t gbox, tbox, gid, tid, gcls, gzm, fseq, fbase, tfoff, gsrc, fill, src;
};

// The common back half of the two entries: offsets, arena carve, uploads, `fill` (which puts the
// bucketed rows in place and may redirect the gt pointers), the seven launches, the copy out.
template <class Fill>
int ev_launch(Eval& E, const Batch& b, Fill&& fill, double* out_host, hipStream_t st,
              const char* who) {
  const int S = b.S, F = b.F, NG = b.NG, NT = b.NT;
  const int K = S / b.gsz;
  std::vector<int> fseq(F);
  std::vector<long long> ioff(F + 1, 0), moff(S + 1, 0), coff(S + 1, 0), jvoff(S, -1);
  size_t jv_total = 0;
  for (int s = 0; s < S; s++) {
    for (int f = b.fbase[s]; f < b.fbase[s + 1]; f++) {
      fseq[f] = s;
      ioff[f + 1] = ioff[f] + (b.metrics ? (long long)(b.gfoff[f + 1] - b.gfoff[f]) *
                                               (b.tfoff[f + 1] - b.tfoff[f])
                                         : 0);
    }
    if (!b.metrics) continue;
    const long long a = b.gidoff[s + 1] - b.gidoff[s], c = b.tidoff[s + 1] - b.tidoff[s];
    moff[s + 1] = moff[s] + a * c;
    coff[s + 1] = coff[s] + (a + c) * (a + c);
    if (a + c > LDS_N) {  // (an upper bound of GT_IDs + IDs: some ids may lose every box)
      jvoff[s] = (long long)jv_total;
      jv_total += (jv_bytes((int)(a + c)) + 255) / 256 * 256;  // (a + c > 64)
    }
  }
  const size_t I = (size_t)ioff[F], M = (size_t)moff[S], CC = (size_t)coff[S];
  const size_t NGI = (size_t)b.gidoff[S], NTI = (size_t)b.tidoff[S];
  if (M * NA >= (size_t)1 << 33)
    return ev_err(BX_ERR_CAPACITY, std::string(who) + ": id matrices of the batch exceed 32 GiB");

  // ---- arena: inputs first, then the zero-initialised block, then prev (-1) and scratch
  Carve cv;
  Offs o;
  o.gbox = cv.take((size_t)b.NGd * 32), o.tbox = cv.take((size_t)NT * 32);
  o.gid = cv.take((size_t)b.NGd * 4), o.tid = cv.take((size_t)NT * 4);
  o.gcls = cv.take((size_t)b.NGd * 4), o.gzm = cv.take((size_t)b.NGd * 4);
  const size_t o_gfoff = cv.take((size_t)(F + 1) * 4);
  o.tfoff = cv.take((size_t)(F + 1) * 4);
  const size_t o_ioff = cv.take((size_t)(F + 1) * 8);
  o.fseq = cv.take((size_t)F * 4);
  o.fbase = cv.take((size_t)(S + 1) * 4);
  const size_t o_gidoff = cv.take((size_t)(S + 1) * 4), o_tidoff = cv.take((size_t)(S + 1) * 4);
  const size_t o_moff = cv.take((size_t)(S + 1) * 8), o_coff = cv.take((size_t)(S + 1) * 8);
  const size_t o_jvoff = cv.take((size_t)S * 8);
  o.gsrc = cv.take(b.NGd ? 0 : (size_t)F * 4);
  o.src = cv.take(b.NGd ? 0 : (size_t)NT * 4);
  const size_t z0 = cv.off;
  o.fill = cv.take(b.NGd ? 0 : (size_t)F * 4);
  const size_t o_gcount = cv.take(NGI * 4), o_tcount = cv.take(NTI * 4);
  const size_t o_pot = cv.take(M * 8), o_idpot = cv.take(M * 4), o_mc = cv.take(M * NA * 4);
  const size_t o_ftp = cv.take((size_t)F * NA * 4), o_floc = cv.take((size_t)F * NA * 8);
  const size_t o_prevt = cv.take(NGI * 4), o_ptep = cv.take(NGI * 4);
  const size_t o_mcount = cv.take(NGI * 4), o_frag = cv.take(NGI * 4);
  const size_t o_nkg = cv.take((size_t)F * 4), o_nkt = cv.take((size_t)F * 4);
  const size_t o_clr = cv.take((size_t)S * 64), o_idr = cv.take((size_t)S * 64);
  const size_t o_out = cv.take((size_t)(S + K) * NF * 8);
  const size_t z1 = cv.off;
  const size_t o_prev = cv.take(NGI * 4);
  const size_t p1 = cv.off;
  const size_t o_cst = cv.take(I * 8), o_ksim = cv.take(I * 8);
  const size_t o_kgid = cv.take((size_t)NG * 4), o_ktid = cv.take((size_t)NT * 4);
  const size_t o_idc = cv.take(CC * 8), o_jvg = cv.take(jv_total);
  const size_t o_gl = cv.take(NGI * 4), o_tl = cv.take(NTI * 4);
  int rc = ev_reserve(E.arena, E.arena_bytes, cv.off, who);
  if (rc != BX_OK) return rc;
  unsigned char* A = (unsigned char*)E.arena;
  auto up = [&](size_t at, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(A + at, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  BX_HIPCHK(up(o_gfoff, b.gfoff, (size_t)(F + 1) * 4));
  BX_HIPCHK(up(o.tfoff, b.tfoff, (size_t)(F + 1) * 4));
  BX_HIPCHK(up(o_ioff, ioff.data(), (size_t)(F + 1) * 8));
  BX_HIPCHK(up(o.fseq, fseq.data(), (size_t)F * 4));
  BX_HIPCHK(up(o.fbase, b.fbase, (size_t)(S + 1) * 4));
  BX_HIPCHK(up(o_gidoff, b.gidoff, (size_t)(S + 1) * 4));
  BX_HIPCHK(up(o_tidoff, b.tidoff, (size_t)(S + 1) * 4));
  BX_HIPCHK(up(o_moff, moff.data(), (size_t)(S + 1) * 8));
  BX_HIPCHK(up(o_coff, coff.data(), (size_t)(S + 1) * 8));
  BX_HIPCHK(up(o_jvoff, jvoff.data(), (size_t)S * 8));
  BX_HIPCHK(hipMemsetAsync(A + z0, 0, z1 - z0, st));
  BX_HIPCHK(hipMemsetAsync(A + z1, 0xff, p1 - z1, st));

  EvDev g;
  g.S = S, g.F = F, g.mot20 = b.benchmark == 20, g.gsz = b.gsz;
  g.gbox = (const double*)(A + o.gbox), g.tbox = (const double*)(A + o.tbox);
  g.gid = (const int*)(A + o.gid), g.tid = (const int*)(A + o.tid);
  g.gcls = (const int*)(A + o.gcls), g.gzm = (const int*)(A + o.gzm);
  g.gfoff = (const int*)(A + o_gfoff), g.tfoff = (const int*)(A + o.tfoff);
  g.gsrc = g.gfoff;
  g.ioff = (const long long*)(A + o_ioff), g.fseq = (const int*)(A + o.fseq);
  g.fbase = (const int*)(A + o.fbase);
  g.gidoff = (const int*)(A + o_gidoff), g.tidoff = (const int*)(A + o_tidoff);
  g.moff = (const long long*)(A + o_moff), g.coff = (const long long*)(A + o_coff);
  g.jvoff = (const long long*)(A + o_jvoff);
  g.cst = (double*)(A + o_cst), g.ksim = (double*)(A + o_ksim);
  g.kgid = (int*)(A + o_kgid), g.ktid = (int*)(A + o_ktid);
  g.nkg = (int*)(A + o_nkg), g.nkt = (int*)(A + o_nkt);
  g.gcount = (int*)(A + o_gcount), g.tcount = (int*)(A + o_tcount);
  g.pot = (double*)(A + o_pot), g.idpot = (int*)(A + o_idpot), g.mc = (int*)(A + o_mc);
  g.mtot = (long long)M;
  g.ftp = (int*)(A + o_ftp), g.floc = (double*)(A + o_floc);
  g.prev = (int*)(A + o_prev), g.prevt = (int*)(A + o_prevt), g.ptep = (int*)(A + o_ptep);
  g.mcount = (int*)(A + o_mcount), g.frag = (int*)(A + o_frag);
  g.clr = (double*)(A + o_clr), g.idc = (double*)(A + o_idc), g.jvg = A + o_jvg;
  g.gl = (int*)(A + o_gl), g.tl = (int*)(A + o_tl), g.idr = (double*)(A + o_idr);
  g.out = (double*)(A + o_out);

  if ((rc = fill(g, A, o)) != BX_OK) return rc;
  if (!b.metrics) return ev_err(BX_ERR_INVALID, std::string(who) + ": invalid tracker rows");

  Alphas al;
  for (int a = 0; a < NA; a++) al.a[a] = 0.05 + a * 0.05;  // np.arange(0.05, 0.99, 0.05)
  // the per-frame solver state is sized by the batch's largest frame, not by the capacity
  const int cap = (std::max(b.cap, 1) + 63) / 64 * 64;
  const size_t lds = ev_frame_lds(cap);
  hipLaunchKernelGGL(ev_pre_kernel, dim3(F), dim3(OW), lds, st, g, cap);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(ev_hota1_kernel, dim3(S), dim3(FT), (size_t)cap * 16, st, g, cap);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(ev_hota2_kernel, dim3(F), dim3(OW), lds, st, g, cap, al);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(ev_clear_kernel, dim3(S), dim3(OW), lds, st, g, cap);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(ev_identity_kernel, dim3(S), dim3(OW), jv_bytes(LDS_N), st, g);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(ev_finish_kernel, dim3(S), dim3(FT), 0, st, g);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(ev_combine_kernel, dim3(K), dim3(OW), 0, st, g);
  BX_HIPCHK(hipGetLastError());
  BX_HIPCHK(hipMemcpyAsync(out_host, g.out, (size_t)(S + K) * NF * 8, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  return BX_OK;
}

// Checks shared by bx_eval_run_host and bx_eval_set_gt_host: fbase [S + 1] of the sequences.
int ev_frames(const Eval& E, const char* who, int S, const int32_t* frames, std::vector<int>& fbase) {
  fbase.assign(S + 1, 0);
  for (int s = 0; s < S; s++) {
    if (frames[s] < 1)
      return ev_err(BX_ERR_INVALID, std::string(who) + ": a sequence needs at least one frame");
    if (frames[s] > E.max_frames)
      return ev_err(BX_ERR_CAPACITY, "sequence " + std::to_string(s) + " has " +
                                         std::to_string(frames[s]) + " frames, capacity " +
                                         std::to_string(E.max_frames));
    if ((long long)fbase[s] + frames[s] >= INT_MAX / (2 * NA))
      return ev_err(BX_ERR_CAPACITY, std::string(who) + ": too many frames in one batch");
    fbase[s + 1] = fbase[s] + frames[s];
  }
  return BX_OK;
}

// The latched key of the device bucketing as a status and its text.
int ev_latched(unsigned long long key, const Eval& E) {
  const int q = (int)(key >> 44), stage = (int)(key >> 41) & 7, kind = (int)(key & 1);
  const long long row = (long long)((key >> 1) & ((1ull << 40) - 1));
  const std::string seq = "results: sequence " + std::to_string(q);
  switch (stage) {
    case ST_RANGE: return ev_err(BX_ERR_INVALID, seq + " has a negative first row or row count");
    case ST_ROW:
      return ev_err(BX_ERR_INVALID,
                    seq + (kind ? " has a non-integer id (row " : " has a frame outside 1..frames (row ") +
                        std::to_string(row) + ")");
    case ST_IDS:
      return ev_err(BX_ERR_CAPACITY, seq + " has more ids than the capacity " + std::to_string(E.max_ids));
    case ST_BOXES:
      if (kind) return ev_err(BX_ERR_CAPACITY, seq + " has too many rows");
      return ev_err(BX_ERR_CAPACITY, seq + " frame " + std::to_string(row) + " has more boxes than the capacity " +
                                         std::to_string(E.max_boxes));
    default: return ev_err(BX_ERR_INVALID, seq + " frame " + std::to_string(row) + " has an id twice");
  }
}

}  // namespace

extern "C" {

int bx_eval_create(int max_boxes, int max_ids, int max_frames, void** out) {
  if (!out) return ev_err(BX_ERR_INVALID, "bx_eval_create: null argument");
  if (max_boxes == 0) max_boxes = BX_EVAL_MAX_BOXES;
  if (max_ids == 0) max_ids = BX_EVAL_MAX_IDS;
  if (max_frames == 0) max_frames = BX_EVAL_MAX_FRAMES;
  if (max_boxes < 1 || max_boxes > 1024 || max_ids < 1 || max_ids > 16384 || max_frames < 1)
    return ev_err(BX_ERR_INVALID,
                  "bx_eval_create: max_boxes in 1..1024, max_ids in 1..16384, max_frames >= 1");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return ev_err(BX_ERR_NO_DEVICE, "no HIP device visible");
  Eval* E = new Eval;
  E->max_boxes = max_boxes, E->max_ids = max_ids, E->max_frames = max_frames;
  *out = E;
  return BX_OK;
}

int bx_eval_destroy(void* h) {
  if (!h) return BX_OK;
  Eval* E = (Eval*)h;
  if (E->arena) (void)hipFree(E->arena);
  if (E->gt) (void)hipFree(E->gt);
  if (E->front) (void)hipFree(E->front);
  delete E;
  return BX_OK;
}

int bx_eval_capacity(void* h, int* max_boxes, int* max_ids, int* max_frames, int* lds_n) {
  if (!h) return ev_err(BX_ERR_INVALID, "bx_eval_capacity: null handle");
  const Eval* E = (const Eval*)h;
  if (max_boxes) *max_boxes = E->max_boxes;
  if (max_ids) *max_ids = E->max_ids;
  if (max_frames) *max_frames = E->max_frames;
  if (lds_n) *lds_n = LDS_N;
  return BX_OK;
}

int bx_eval_run_host(void* h, int n_seq, int benchmark, const int32_t* seq_frames_host,
                     const int64_t* gt_off_host, const double* gt_rows_host,
                     const int64_t* tr_off_host, const double* tr_rows_host, double* out_host,
                     void* stream) {
  if (!h) return ev_err(BX_ERR_INVALID, "bx_eval_run_host: null handle");
  Eval& E = *(Eval*)h;
  const int S = n_seq;
  if (S < 1 || !seq_frames_host || !gt_off_host || !tr_off_host || !out_host)
    return ev_err(BX_ERR_INVALID, "bx_eval_run_host: n_seq >= 1 and non-null arrays");
  if (benchmark != 16 && benchmark != 17 && benchmark != 20)
    return ev_err(BX_ERR_INVALID, "bx_eval_run_host: benchmark must be 16, 17 or 20");
  if (gt_off_host[0] != 0 || tr_off_host[0] != 0 || (gt_off_host[S] > 0 && !gt_rows_host) ||
      (tr_off_host[S] > 0 && !tr_rows_host))
    return ev_err(BX_ERR_INVALID, "bx_eval_run_host: offsets start at 0; rows must be given");
  if (gt_off_host[S] >= INT_MAX / 4 || tr_off_host[S] >= INT_MAX / 4)
    return ev_err(BX_ERR_CAPACITY, "bx_eval_run_host: too many rows in one batch");
  std::vector<int> fbase;
  int rc = ev_frames(E, "bx_eval_run_host", S, seq_frames_host, fbase);
  if (rc != BX_OK) return rc;
  const int F = fbase[S];
  Side gs, ts;
  rc = bucket_side(E, "gt", S, seq_frames_host, fbase.data(), gt_off_host, gt_rows_host, 9, true, gs);
  if (rc != BX_OK) return rc;
  rc = bucket_side(E, "results", S, seq_frames_host, fbase.data(), tr_off_host, tr_rows_host, 6,
                   false, ts);
  if (rc != BX_OK) return rc;
  Batch b;
  b.S = S, b.F = F, b.gsz = S, b.benchmark = benchmark, b.metrics = true;
  b.fbase = fbase.data(), b.gfoff = gs.foff.data(), b.tfoff = ts.foff.data();
  b.gidoff = gs.idoff.data(), b.tidoff = ts.idoff.data();
  b.NG = b.NGd = (int)gs.id.size(), b.NT = (int)ts.id.size();
  b.cap = 1;
  for (int f = 0; f < F; f++)
    b.cap = std::max(b.cap, std::max(gs.foff[f + 1] - gs.foff[f], ts.foff[f + 1] - ts.foff[f]));
  hipStream_t st = (hipStream_t)stream;
  auto fill = [&](EvDev&, unsigned char* A, const Offs& o) {
    auto up = [&](size_t at, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(A + at, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    BX_HIPCHK(up(o.gbox, gs.box.data(), (size_t)b.NG * 32));
    BX_HIPCHK(up(o.tbox, ts.box.data(), (size_t)b.NT * 32));
    BX_HIPCHK(up(o.gid, gs.id.data(), (size_t)b.NG * 4));
    BX_HIPCHK(up(o.tid, ts.id.data(), (size_t)b.NT * 4));
    BX_HIPCHK(up(o.gcls, gs.cls.data(), (size_t)b.NG * 4));
    BX_HIPCHK(up(o.gzm, gs.zm.data(), (size_t)b.NG * 4));
    return (int)BX_OK;
  };
  return ev_launch(E, b, fill, out_host, st, "bx_eval_run_host");
}

int bx_eval_set_gt_host(void* h, int n_seq, const int32_t* seq_frames_host,
                        const int64_t* gt_off_host, const double* gt_rows_host) {
  if (!h) return ev_err(BX_ERR_INVALID, "bx_eval_set_gt_host: null handle");
  Eval& E = *(Eval*)h;
  const int S = n_seq;
  if (S < 1 || !seq_frames_host || !gt_off_host)
    return ev_err(BX_ERR_INVALID, "bx_eval_set_gt_host: n_seq >= 1 and non-null arrays");
  if (gt_off_host[0] != 0 || (gt_off_host[S] > 0 && !gt_rows_host))
    return ev_err(BX_ERR_INVALID, "bx_eval_set_gt_host: offsets start at 0; rows must be given");
  if (gt_off_host[S] >= INT_MAX / 4)
    return ev_err(BX_ERR_CAPACITY, "bx_eval_set_gt_host: too many rows in one batch");
  std::vector<int> fbase;
  int rc = ev_frames(E, "bx_eval_set_gt_host", S, seq_frames_host, fbase);
  if (rc != BX_OK) return rc;
  Side gs;
  rc = bucket_side(E, "gt", S, seq_frames_host, fbase.data(), gt_off_host, gt_rows_host, 9, true, gs);
  if (rc != BX_OK) return rc;
  const size_t NG = gs.id.size();
  Carve cv;
  cv.take(NG * 32);
  const size_t o_id = cv.take(NG * 4), o_cls = cv.take(NG * 4), o_zm = cv.take(NG * 4);
  void* dev = nullptr;
  if (hipMalloc(&dev, cv.off) != hipSuccess)
    return ev_err(BX_ERR_HIP, "bx_eval_set_gt_host: hipMalloc of " + std::to_string(cv.off) +
                                  " bytes failed");
  unsigned char* A = (unsigned char*)dev;
  hipError_t e = hipSuccess;
  if (NG) {
    e = hipMemcpy(A, gs.box.data(), NG * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A + o_id, gs.id.data(), NG * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A + o_cls, gs.cls.data(), NG * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A + o_zm, gs.zm.data(), NG * 4, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return ev_err(BX_ERR_HIP, std::string("bx_eval_set_gt_host: ") + hipGetErrorString(e));
  }
  if (E.gt) (void)hipFree(E.gt);
  E.gt = dev;
  E.gt_S = S, E.gt_rows = (int)NG;
  E.gt_o_id = o_id, E.gt_o_cls = o_cls, E.gt_o_zm = o_zm;
  E.gt_frames.assign(seq_frames_host, seq_frames_host + S);
  E.gt_fbase = fbase;
  E.gt_foff = gs.foff;
  E.gt_idoff = gs.idoff;
  E.gt_cap = 0;
  for (int f = 0; f < fbase[S]; f++) E.gt_cap = std::max(E.gt_cap, gs.foff[f + 1] - gs.foff[f]);
  return BX_OK;
}

int bx_eval_run_device(void* h, int n_groups, int benchmark, const void* tr_rows,
                       int64_t row_stride, const void* tr_base, const void* tr_n, double* out_host,
                       void* stream) {
  if (!h) return ev_err(BX_ERR_INVALID, "bx_eval_run_device: null handle");
  Eval& E = *(Eval*)h;
  if (E.gt_S < 1)
    return ev_err(BX_ERR_INVALID, "bx_eval_run_device: no ground truth set (bx_eval_set_gt_host)");
  if (n_groups < 1 || !tr_rows || !tr_base || !tr_n || !out_host || row_stride < 6)
    return ev_err(BX_ERR_INVALID,
                  "bx_eval_run_device: n_groups >= 1, non-null arrays and row_stride >= 6");
  if (benchmark != 16 && benchmark != 17 && benchmark != 20)
    return ev_err(BX_ERR_INVALID, "bx_eval_run_device: benchmark must be 16, 17 or 20");
  const int S1 = E.gt_S, F1 = E.gt_fbase[S1], K = n_groups;
  const long long Ql = (long long)K * S1, Fl = (long long)K * F1, NGl = (long long)K * E.gt_rows;
  if (Ql >= 1 << 20 || Fl >= INT_MAX / (2 * NA) || NGl >= INT_MAX / 4)
    return ev_err(BX_ERR_CAPACITY, "bx_eval_run_device: too many sequences, frames or gt rows in "
                                   "one batch");
  const int Q = (int)Ql, F = (int)Fl;
  hipStream_t st = (hipStream_t)stream;

  // ---- host offsets of the Q = K * S evaluator sequences (sequence q has gt sequence q % S)
  std::vector<int> fbase(Q + 1), gfoff(F + 1), gsrc(F), gidoff(Q + 1);
  for (int k = 0; k < K; k++) {
    for (int s = 0; s <= S1; s++) {
      fbase[k * S1 + s] = k * F1 + E.gt_fbase[s];
      gidoff[k * S1 + s] = k * E.gt_idoff[S1] + E.gt_idoff[s];
    }
    for (int f = 0; f <= F1; f++) gfoff[k * F1 + f] = k * E.gt_rows + E.gt_foff[f];
    for (int f = 0; f < F1; f++) gsrc[k * F1 + f] = E.gt_foff[f];
  }

  // ---- count + validate and relabel, ahead of the arena (its carve needs their counts)
  int tab_n = 64;
  while (tab_n < 2 * E.max_ids) tab_n <<= 1;
  int sort_n = 1;
  while (sort_n < E.max_ids) sort_n <<= 1;
  Carve fc;
  const size_t o_fbase = fc.take((size_t)(Q + 1) * 4);
  const size_t c0 = fc.off;
  const size_t o_cnt = fc.take((size_t)F * 4), o_nid = fc.take((size_t)Q * 4);
  const size_t c1 = fc.off;
  const size_t o_latch = fc.take(8);
  const size_t o_tab = fc.take((size_t)Q * tab_n * 8);
  int rc = ev_reserve(E.front, E.front_bytes, fc.off, "bx_eval_run_device");
  if (rc != BX_OK) return rc;
  unsigned char* P = (unsigned char*)E.front;
  int* d_fbase = (int*)(P + o_fbase);
  int* d_cnt = (int*)(P + o_cnt);
  int* d_nid = (int*)(P + o_nid);
  unsigned long long* d_latch = (unsigned long long*)(P + o_latch);
  long long* d_tab = (long long*)(P + o_tab);
  BX_HIPCHK(hipMemcpyAsync(d_fbase, fbase.data(), (size_t)(Q + 1) * 4, hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipMemsetAsync(P + c0, 0, c1 - c0, st));
  BX_HIPCHK(hipMemsetAsync(d_latch, 0xff, 8, st));
  BX_HIPCHK(hipMemsetAsync(d_tab, 0x7f, (size_t)Q * tab_n * 8, st));
  TrIn in;
  in.rows = (const double*)tr_rows, in.stride = row_stride;
  in.base = (const long long*)tr_base, in.n = (const long long*)tr_n;
  hipLaunchKernelGGL(ev_trcount_kernel, dim3((unsigned)Q * CB), dim3(CT), 0, st, in, d_fbase,
                     E.max_boxes, d_cnt, d_latch);
  BX_HIPCHK(hipGetLastError());
  const size_t sort_lds = (size_t)sort_n * 8;
  BX_HIPCHK(bx_lds_attr((const void*)ev_relabel_kernel, sort_lds));
  hipLaunchKernelGGL(ev_relabel_kernel, dim3(Q), dim3(RT), sort_lds, st, in, d_tab, tab_n, E.max_ids,
                     d_nid, d_latch);
  BX_HIPCHK(hipGetLastError());
  std::vector<int> tfoff(F + 1, 0), tidoff(Q + 1, 0);
  unsigned long long key = EV_NOERR;
  BX_HIPCHK(hipMemcpyAsync(tfoff.data() + 1, d_cnt, (size_t)F * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(tidoff.data() + 1, d_nid, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(&key, d_latch, 8, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));

  // ---- counts -> offsets, as bucket_side forms them
  int capt = 0;
  long long nt = 0;
  for (int f = 0; f < F; f++) {
    capt = std::max(capt, tfoff[f + 1]);
    nt += tfoff[f + 1];
    if (nt >= INT_MAX / 4)
      return ev_err(BX_ERR_CAPACITY, "bx_eval_run_device: too many rows in one batch");
    tfoff[f + 1] = (int)nt;
  }
  for (int q = 0; q < Q; q++) tidoff[q + 1] += tidoff[q];
  Batch b;
  b.S = Q, b.F = F, b.gsz = S1, b.benchmark = benchmark, b.metrics = key == EV_NOERR;
  b.fbase = fbase.data(), b.gfoff = gfoff.data(), b.tfoff = tfoff.data();
  b.gidoff = gidoff.data(), b.tidoff = tidoff.data();
  b.NG = (int)NGl, b.NGd = 0, b.NT = (int)nt;
  b.cap = std::max(E.gt_cap, capt);
  int pw = 1;  // LDS of the gather: the sort's padded indices, then the labels
  while (pw < std::min(capt, E.max_boxes)) pw <<= 1;
  auto fill = [&](EvDev& g, unsigned char* A, const Offs& o) {
    const unsigned char* G = (const unsigned char*)E.gt;
    g.gbox = (const double*)G, g.gid = (const int*)(G + E.gt_o_id);
    g.gcls = (const int*)(G + E.gt_o_cls), g.gzm = (const int*)(G + E.gt_o_zm);
    g.gsrc = (const int*)(A + o.gsrc);
    BX_HIPCHK(hipMemcpyAsync(A + o.gsrc, gsrc.data(), (size_t)F * 4, hipMemcpyHostToDevice, st));
    if (b.NT > 0) {
      hipLaunchKernelGGL(ev_trscatter_kernel, dim3((unsigned)Q * CB), dim3(CT), 0, st, in, g.fbase,
                         g.tfoff, (int*)(A + o.fill), (int*)(A + o.src));
      BX_HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(ev_trgather_kernel, dim3(F), dim3(OW), (size_t)pw * 4 + (size_t)E.max_boxes * 4,
                         st, in, g.fseq, g.fbase, g.tfoff, (const int*)(A + o.src),
                         (const long long*)d_tab, tab_n, (const int*)d_nid, E.max_boxes, pw,
                         (double*)(A + o.tbox), (int*)(A + o.tid), d_latch);
      BX_HIPCHK(hipGetLastError());
    }
    BX_HIPCHK(hipMemcpyAsync(&key, d_latch, 8, hipMemcpyDeviceToHost, st));
    BX_HIPCHK(hipStreamSynchronize(st));
    return key == EV_NOERR ? (int)BX_OK : ev_latched(key, E);
  };
  return ev_launch(E, b, fill, out_host, st, "bx_eval_run_device");
}

}  // extern "C"
