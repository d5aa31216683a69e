// bx_hybridsort.hip — the HybridSort per-frame update on MI355X.
//
// Reference: boxmot/trackers/hybridsort/hybridsort.py:431-741 (HybridSort.update), its
// KalmanBoxTracker (:110-347: a 9-state / 5-measurement XYSR filter that also tracks the
// detection score, four corner velocities, confidence / confidence_pre, the smoothed feature and
// the 30-deep feature bank) over KalmanFilterXYSR with the observation-centric re-update
// (motion/kalman_filters/aabb/xysr_kf.py:137-291), associate_4_points_with_score_with_reid
// (hybridsort/association.py:537-644), cost_vel (:328-349), embedding_distance (:734-751) and
// linear_assignment (:312-325), with the patches H1-H3 of tests/golden/make_golden_hybridsort.py
// (H1: the ORU replay of a 5-vector measurement).  use_byte is not built.  The
// ECC switch (KalmanBoxTracker.camera_update, :237-249, :448-451) is hyb_camera_kernel, a phase
// ahead of the frame kernel that only an engine on which bx_hybrid_set_ecc_host has switched a
// sequence on launches.
//
// Per frame, three launches on the caller's stream:
//   hyb_dist_kernel     max(0, 1 - u.v / (|u||v|)) of every detection against every pre-frame
//                       track's smooth_feat (z = 0) and feature-bank mean (z = 1): the fp64 MFMA
//                       tile of bx_embtile.h with the row norms taken by the same workgroup
//   hyb_frame_kernel    one wave64 workgroup per sequence on the shared device code of
//                       bx_ocs_device.h (observation ring, LDS carve, lapjv-ordered LAP): predict,
//                       first association (asso_func + four-corner direction consistency - score
//                       difference, + appearance), the long-term-ReID correction filter, updates
//                       with ORU, the OCR round, births, outputs, deaths; emits feature records
//   hyb_feature_kernel  wave per record: normalise the detection feature, moving average of
//                       smooth_feat, push into the bank ring, recompute the bank mean
// The Kalman filter runs on 16 lanes per track (lane r owns row min(r, 8) of x and P).  The
// reference's float32 arithmetic (setup_decorator hands update() float32 detections, and
// HybridSort never widens them) is kept where it reaches the outputs: convert_bbox_to_z and the
// ORU interpolation are float32.  The library builds with -ffp-contract=off.
#include <float.h>
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/bxhybridsort.h"
#include "bx_classes_glue.h"
#include "bx_device.h"
#include "bx_host.h"

using namespace bx;


namespace {

#include "bx_ocs_device.h"
#include "bx_ocs_host.h"
#include "bx_embtile.h"

constexpr int HX = 9, HZ = 5;  // state [u v s c r du dv ds dc], measurement [u v s c r]
constexpr int BANK = 30;       // longterm_bank_length (hybridsort.py:126,208-209)
// doubles per track of per-frame scratch: box4, kalman_score, simple_score, k-previous obs5,
// last_obs5, corner velocities lt rt lb rb as (y, x)
constexpr int HTB = 24;
enum { HT_KS = 4, HT_SS = 5, HT_KOBS = 6, HT_LAST = 11, HT_VEL = 16 };

struct HybTrk {
  double x[HX], P[HX * HX];
  double sx[HX], sP[HX * HX];   // freeze() snapshot (attr_saved)
  double last_obs[5];
  double obs_box[OBS_KEEP][5];  // observations dict: the entry of age a sits in slot a % 8
  double vel[4][2];             // velocity_lt, _rt, _lb, _rb as (y, x)
  double conf, cls, det_ind;
  float hbox[5];                // last non-None entry of history_obs (float32, as the reference's)
  float confidence, conf_pre;
  int obs_age[OBS_KEEP];
  int last_age, has_vel, id, tsu, hits, hit_streak, age, has_pre;  // last_age < 0: no obs
  int observed, has_saved, hvalid, htail;
};

// One sequence's entry of HybridSort's per-sequence parameter table: OCSort's entry (min_conf,
// q_xy, q_s and use_byte stay 0, as in the engine's own OcsDev) plus the two appearance weights.
// o.set 0: the sequence runs on the engine's own parameters.
struct HybSeqPar {
  OcsSeqPar o;
  double tcm_w, lt_w;
};

struct HybDev {
  OcsDev o;            // shared geometry, thresholds, lists and scratch; o.trk is unused (null)
  int F;               // embedding width
  int x_off;           // bytes of LDS the shared carve takes (pp follows)
  double tcm_w, lt_w;  // TCM_first_step_weight, longterm_reid_weight
  double q[HX];        // diag of Q (hybridsort.py:169-171)
  HybTrk* trk;         // [S][T]
  double* smooth;      // [S][T][F] smooth_feat by slot
  double* lmean;       // [S][T][F] mean of the rows present in the bank
  double* bank;        // [S][T][BANK][F] feature ring: push k lands in row k % BANK
  int* bcnt;           // [S][T] pushes so far
  double* ec;          // [S][2][D][T] distances by (detection of the frame, pre-frame position)
  int* rec;            // [S][D] per detection of the frame: the slot its feature goes to, or -1
  int* rec_b;          // [S][D] 1: the slot is a newborn's
  // [S] per-sequence parameters (bx_hybrid_set_seq_params_host), or null: none was ever set.  The
  // frame kernel reads it, never writes it; hyb_dist_kernel and hyb_feature_kernel read no
  // per-sequence field.
  const HybSeqPar* seqpar = nullptr;
};

// The kernel-entry override (bx_ocs_device.h ocs_seq_apply) for HybDev: sequence `seq`'s entry,
// when there is a table and the entry is set, replaces the per-sequence fields of the kernel's own
// copy of `gd`.  Wave-uniform scalar loads, all before the first store.
__device__ __forceinline__ void hyb_seq_override(HybDev& gd, int seq) {
  if (!gd.seqpar) return;
  const HybSeqPar* p = gd.seqpar + seq;
  if (!p->o.set) return;
  const double tcm_w = p->tcm_w, lt_w = p->lt_w;
  ocs_seq_apply(gd.o, &p->o);
  gd.tcm_w = tcm_w;
  gd.lt_w = lt_w;
}

// ------------------------------------------------------------------------------------------
// The 9/5 filter on 16 lanes per track: lane r owns row rr = min(r, 8) (lanes 9..15 mirror row 8
// and never write).  Every element is computed by one lane in the order of the 7/4 filter of
// bx_ocs_device.h; shuffles only move operands between rows.
__device__ __forceinline__ double hsh(double v, int src) { return __shfl(v, src, 16); }

struct Kf9 {
  double x, P[HX];
};

__device__ __forceinline__ void row_load9(const double* x, const double* P, int rr, Kf9& k) {
  k.x = x[rr];
#pragma unroll
  for (int j = 0; j < HX; j++) k.P[j] = P[rr * HX + j];
}

__device__ __forceinline__ void row_store9(double* x, double* P, int r, const Kf9& k) {
  if (r < HX) {
    x[r] = k.x;
#pragma unroll
    for (int j = 0; j < HX; j++) P[r * HX + j] = k.P[j];
  }
}

// x = F x ; P = 1.0 * (F P F') + Q  (F = I + e_i e_{i+5}' for i < 4)
__device__ void kf9_predict(const HybDev& g, int rr, Kf9& k) {
  const int src = rr < 4 ? rr + 5 : rr;
  const double xv = hsh(k.x, src);
  k.x = rr < 4 ? k.x + xv : k.x;
  double FP[HX];
#pragma unroll
  for (int j = 0; j < HX; j++) {
    const double pv = hsh(k.P[j], src);
    FP[j] = rr < 4 ? k.P[j] + pv : k.P[j];
  }
#pragma unroll
  for (int j = 0; j < HX; j++) {
    const double m = j < 4 ? FP[j] + FP[j + 5] : FP[j];
    const double q = rr == j ? g.q[j] : 0.0;
    k.P[j] = 1.0 * m + q;
  }
}

// np.linalg.inv of a 5x5: inv4 of bx_ocs_device.h (LU with partial pivoting, then the solve
// against the identity) for one more row
__device__ __forceinline__ void swap_rows5(double* M, int k, int p) {
#pragma unroll
  for (int i = 0; i < HZ; i++)
    if (i > k && i == p)
#pragma unroll
      for (int j = 0; j < HZ; j++) {
        const double t = M[k * HZ + j];
        M[k * HZ + j] = M[i * HZ + j];
        M[i * HZ + j] = t;
      }
}

__device__ __forceinline__ void inv5(const double* Ain, double* B) {
  double A[HZ * HZ];
  int piv[HZ];
#pragma unroll
  for (int i = 0; i < HZ * HZ; i++) A[i] = Ain[i];
#pragma unroll
  for (int k = 0; k < HZ; k++) {
    int p = k;
    double mx = fabs(A[k * HZ + k]);
#pragma unroll
    for (int i = k + 1; i < HZ; i++)
      if (fabs(A[i * HZ + k]) > mx) mx = fabs(A[i * HZ + k]), p = i;
    piv[k] = p;
    swap_rows5(A, k, p);
    if (A[k * HZ + k] != 0.0) {
      if (fabs(A[k * HZ + k]) >= DBL_MIN) {
        const double r = 1.0 / A[k * HZ + k];
#pragma unroll
        for (int i = k + 1; i < HZ; i++) A[i * HZ + k] *= r;
      } else {
#pragma unroll
        for (int i = k + 1; i < HZ; i++) A[i * HZ + k] /= A[k * HZ + k];
      }
    }
#pragma unroll
    for (int j = k + 1; j < HZ; j++) {
      const double t = -A[k * HZ + j];
#pragma unroll
      for (int i = k + 1; i < HZ; i++) A[i * HZ + j] = A[i * HZ + j] + A[i * HZ + k] * t;
    }
  }
#pragma unroll
  for (int i = 0; i < HZ * HZ; i++) B[i] = (i % (HZ + 1) == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < HZ; k++) swap_rows5(B, k, piv[k]);
#pragma unroll
  for (int j = 0; j < HZ; j++) {
#pragma unroll
    for (int k = 0; k < HZ; k++)
      if (B[k * HZ + j] != 0.0)
#pragma unroll
        for (int i = k + 1; i < HZ; i++) B[i * HZ + j] -= B[k * HZ + j] * A[i * HZ + k];
#pragma unroll
    for (int k = HZ - 1; k >= 0; k--)
      if (B[k * HZ + j] != 0.0) {
        B[k * HZ + j] /= A[k * HZ + k];
#pragma unroll
        for (int i = 0; i < k; i++) B[i * HZ + j] -= B[k * HZ + j] * A[i * HZ + k];
      }
  }
}

// update with a measurement (R = diag(1,1,10,10,10), H = [I5 0], Joseph form); z uniform per
// 16-lane group
__device__ void kf9_update(int rr, Kf9& k, const double* z) {
  const double Rd[HZ] = {1.0, 1.0, 10.0, 10.0, 10.0};
  double y[HZ], S[HZ * HZ], SI[HZ * HZ];
#pragma unroll
  for (int a = 0; a < HZ; a++) y[a] = z[a] - hsh(k.x, a);
#pragma unroll
  for (int a = 0; a < HZ; a++)
#pragma unroll
    for (int b = 0; b < HZ; b++) S[a * HZ + b] = hsh(k.P[b], a) + (a == b ? Rd[a] : 0.0);
  inv5(S, SI);  // every lane of the group inverts the same S identically
  double K[HZ];
#pragma unroll
  for (int b = 0; b < HZ; b++) {
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < HZ; a++) acc += k.P[a] * SI[a * HZ + b];
    K[b] = acc;
  }
  {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < HZ; b++) acc += K[b] * y[b];
    k.x = k.x + acc;
  }
  double ikh[HX], A[HX];
#pragma unroll
  for (int c = 0; c < HX; c++) ikh[c] = (rr == c ? 1.0 : 0.0) - (c < HZ ? K[c] : 0.0);
#pragma unroll
  for (int j = 0; j < HX; j++) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < HX; c++) acc += ikh[c] * hsh(k.P[j], c);
    A[j] = acc;
  }
#pragma unroll
  for (int j = 0; j < HX; j++) {
    double Kj[HZ];
#pragma unroll
    for (int b = 0; b < HZ; b++) Kj[b] = hsh(K[b], j);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < HX; c++) acc += A[c] * ((j == c ? 1.0 : 0.0) - (c < HZ ? Kj[c] : 0.0));
    double kr = 0.0;
#pragma unroll
    for (int b = 0; b < HZ; b++) kr += (K[b] * Rd[b]) * Kj[b];
    k.P[j] = acc + kr;
  }
}

// convert_x_to_bbox (hybridsort.py:55-67): the aspect ratio is x[4]
__device__ void x9_to_bbox(const double* x, double* b) {
  const double w = sqrt(x[2] * x[4]);
  const double h = x[2] / w;
  b[0] = x[0] - w / 2.0;
  b[1] = x[1] - h / 2.0;
  b[2] = x[0] + w / 2.0;
  b[3] = x[1] + h / 2.0;
}

// convert_bbox_to_z (hybridsort.py:36-52) of a float32 detection row, in float32 as numpy
// evaluates it.  A score of 0 would take the reference's 4-vector branch; it cannot get here:
// only detections with score > det_thresh >= 0 reach the filter.
__device__ __forceinline__ void box_to_z(const double* b5, float* z) {
  const float x1 = (float)b5[0], y1 = (float)b5[1], x2 = (float)b5[2], y2 = (float)b5[3];
  const float w = x2 - x1, h = y2 - y1;
  z[0] = x1 + w / 2.0f;
  z[1] = y1 + h / 2.0f;
  z[2] = w * h;
  z[3] = (float)b5[4];
  z[4] = w / (h + 1e-6f);
}

// speed_direction_lt / _rt / _lb / _rb (hybridsort.py:78-107) of box p -> box b, set or added.
// The reference's names: "rt" is (x1, y2), "lb" is (x2, y1).
__device__ __forceinline__ void corner_dirs(const double* p, const double* b, double (*v)[2],
                                            bool add) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int ix = c < 2 ? 0 : 2, iy = (c & 1) ? 3 : 1;
    const double dy = b[iy] - p[iy], dx = b[ix] - p[ix];
    const double norm = sqrt(dy * dy + dx * dx) + 1e-6;
    const double vy = dy / norm, vx = dx / norm;
    v[c][0] = add ? v[c][0] + vy : vy;
    v[c][1] = add ? v[c][1] + vx : vx;
  }
}

// KalmanBoxTracker.update with a detection row [x1,y1,x2,y2,score] + cls (hybridsort.py:251-312),
// 16 lanes wide: lane 0 keeps the bookkeeping, the group runs the Kalman update (with the ORU
// replay of xysr_kf.py:183-209 per H1 when the track was frozen).  The feature is not touched
// here (the frame kernel emits a record for the first round's matches).
__device__ void hyb_update_det(const HybDev& gd, HybTrk& t, int r, const double* b5, double cls,
                               double det_ind) {
  const OcsDev& g = gd.o;
  const int rr = r < HX ? r : HX - 1;
  const int observed = t.observed, has_saved = t.has_saved;
  const int hv = t.hvalid, gap = t.htail + 1;
  float b1[5];
#pragma unroll
  for (int q = 0; q < 5; q++) b1[q] = t.hbox[q];
  if (r == 0) {
    t.det_ind = det_ind;
    t.conf = b5[4];
    t.cls = cls;
    if (sum5(t.last_obs) >= 0) {
      double v[4][2];
      bool any = false;
      for (int i = 0; i < g.delta_t; i++) {  // summed over every hit of age-1 .. age-delta_t
        const int want = t.age - i - 1;
        if (want < 0 || t.obs_age[want & (OBS_KEEP - 1)] != want) continue;
        corner_dirs(t.obs_box[want & (OBS_KEEP - 1)], b5, v, any);
        any = true;
      }
      if (!any) corner_dirs(t.last_obs, b5, v, false);
#pragma unroll
      for (int c = 0; c < 4; c++) {
        t.vel[c][0] = v[c][0];
        t.vel[c][1] = v[c][1];
      }
      t.has_vel = 1;
    }
    for (int k = 0; k < 5; k++) t.last_obs[k] = b5[k];
    const int slot = t.age & (OBS_KEEP - 1);  // observations[age] = bbox
    t.obs_age[slot] = t.age;
    for (int k = 0; k < 5; k++) t.obs_box[slot][k] = b5[k];
    t.last_age = t.age;
    t.tsu = 0;
    t.hits++;
    t.hit_streak++;
    t.conf_pre = t.confidence;
    t.has_pre = 1;
    t.confidence = (float)b5[4];
  }
  float zf[5];
  box_to_z(b5, zf);
  const double z[5] = {zf[0], zf[1], zf[2], zf[3], zf[4]};
  Kf9 k;
  const bool unfreeze = !observed && has_saved;
  if (unfreeze) {
    row_load9(t.sx, t.sP, rr, k);
    if (hv) {
      // H1: x, y, w, h and the score run linearly from the last observation to this one.  The
      // stored measurements are float32: numpy takes w, h and the differences in float32 and
      // widens at the division by the (int64) gap; the score line stays float32
      const float x1 = b1[0], y1 = b1[1], s1 = b1[2], c1 = b1[3], r1 = b1[4];
      const float w1 = sqrtf(s1 * r1), h1 = sqrtf(s1 / r1);
      const float x2 = zf[0], y2 = zf[1], s2 = zf[2], c2 = zf[3], r2 = zf[4];
      const float w2 = sqrtf(s2 * r2), h2 = sqrtf(s2 / r2);
      const double dg = (double)gap;
      const double dx = (double)(x2 - x1) / dg, dy = (double)(y2 - y1) / dg;
      const double dw = (double)(w2 - w1) / dg, dh = (double)(h2 - h1) / dg;
      for (int i = 0; i < gap; i++) {
        const double m = (double)(i + 1);
        const double xx = x1 + m * dx, yy = y1 + m * dy;
        const double ww = w1 + m * dw, hh = h1 + m * dh;
        const float cc = c1 + ((float)(i + 1) * (c2 - c1)) / (float)gap;
        const double nb[5] = {xx, yy, ww * hh, cc, ww / hh};
        kf9_update(rr, k, nb);
        if (i != gap - 1) kf9_predict(gd, rr, k);
      }
    }
  } else {
    row_load9(t.x, t.P, rr, k);
  }
  kf9_update(rr, k, z);
  row_store9(t.x, t.P, r, k);
  if (r == 0) {
    if (unfreeze) t.has_saved = 0;
    t.observed = 1;
#pragma unroll
    for (int q = 0; q < 5; q++) t.hbox[q] = zf[q];
    t.htail = 0;
    t.hvalid = 1;
  }
}

// update(None, None, None, None) (hybridsort.py:313-315): the first miss after an observation
// freezes (x, P); confidence_pre = None
__device__ void hyb_update_none(const OcsDev& g, HybTrk& t, int r) {
  const int observed = t.observed;
  if (observed && r < HX) {
    t.sx[r] = t.x[r];
#pragma unroll
    for (int j = 0; j < HX; j++) t.sP[r * HX + j] = t.P[r * HX + j];
  }
  if (r == 0) {
    t.htail++;
    if (t.htail >= g.max_obs) t.hvalid = 0;  // the box left the deque(maxlen=max_obs)
    if (observed) t.has_saved = 1;
    t.observed = 0;
    t.has_pre = 0;
  }
}

// ------------------------------------------------------------------------------------------
// embedding_distance (association.py:734-751): np.maximum(0, cdist(tracks, dets, "cosine")),
// one 32 x 64 tile of detections x tracks.  cdist's cosine is 1 - u.v / (|u| |v|) with the
// cosine clamped to [-1, 1].  The workgroup takes the norms of its own rows first (8 threads per
// detection row, 4 per track row: the staging roles of the tile).
__device__ __forceinline__ void dist_tile(double* lds, double* nrm, int F, int d0, int t0, int nd,
                                          int nt, const double* arow, const double* brow,
                                          double* out, int ld) {
  const int tid = threadIdx.x;
  const int ar = ec_arow(tid), br = ec_brow(tid);
  const bool a_ok = d0 + ar < nd, b_ok = t0 + br < nt;
  double sa = 0.0, sb = 0.0;
  if (a_ok)
    for (int k = tid & 7; k < F; k += 8) sa += arow[k] * arow[k];
  if (b_ok)
    for (int k = tid & 3; k < F; k += 4) sb += brow[k] * brow[k];
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) sa += __shfl_xor(sa, o);
#pragma unroll
  for (int o = 1; o < 4; o <<= 1) sb += __shfl_xor(sb, o);
  if ((tid & 7) == 0) nrm[ar] = sqrt(sa);
  if ((tid & 3) == 0) nrm[EC_BM + br] = sqrt(sb);
  d4 acc[2];
  ec_tile(lds, F, a_ok, arow + ec_ak(tid), b_ok, brow + ec_bk(tid), acc);  // (syncs: nrm is visible)
  const int lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wc = w >> 1;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int cl = wc * 32 + j * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int rl = wr * 16 + (lane >> 4) + 4 * q;
      if (d0 + rl < nd && t0 + cl < nt) {
        double c = acc[j][q] / (nrm[rl] * nrm[EC_BM + cl]);
        if (fabs(c) > 1.0) c = c < 0 ? -1.0 : 1.0;
        const double d = 1.0 - c;
        out[(size_t)(d0 + rl) * ld + t0 + cl] = d < 0.0 ? 0.0 : d;
      }
    }
  }
}

__global__ void __launch_bounds__(256)
    hyb_dist_kernel(HybDev g, int seq0, const int* __restrict__ det_off,
                    const double* __restrict__ embs) {
  __shared__ double lds[2 * EC_STAGE];
  __shared__ double nrm[EC_BM + EC_BN];
  const int b = blockIdx.x, seq = seq0 + b;
  const int T = g.o.T;
  const int r0 = det_off[b];
  int nd = det_off[b + 1] - r0;
  if (nd > g.o.D) nd = g.o.D;
  const int nt = g.o.seqst[(size_t)seq * SQO + SO_NTR];
  const int d0 = (int)blockIdx.y / ec_tiles_t(T) * EC_BM;
  const int t0 = (int)blockIdx.y % ec_tiles_t(T) * EC_BN;
  if (d0 >= nd || t0 >= nt) return;  // workgroup-uniform
  const int F = g.F;
  const int* order = g.o.order + (size_t)seq * T;
  const double* temb = (blockIdx.z ? g.lmean : g.smooth) + (size_t)seq * T * F;
  const int tid = threadIdx.x;
  const int ar = ec_arow(tid), br = ec_brow(tid);
  const double* ap = embs + (size_t)(r0 + (d0 + ar < nd ? d0 + ar : 0)) * F;
  const double* bp = temb + (size_t)(t0 + br < nt ? order[t0 + br] : 0) * F;
  dist_tile(lds, nrm, F, d0, t0, nd, nt, ap, bp,
            g.ec + ((size_t)seq * 2 + blockIdx.z) * g.o.D * T, T);
}

// the op: the same tile on plain arrays, grid (tiles of nd x nt)
__global__ void __launch_bounds__(256)
    hyb_dist_op_kernel(int nd, int nt, int F, const double* __restrict__ A,
                       const double* __restrict__ B, double* __restrict__ out) {
  __shared__ double lds[2 * EC_STAGE];
  __shared__ double nrm[EC_BM + EC_BN];
  const int d0 = (int)blockIdx.x / ec_tiles_t(nt) * EC_BM;
  const int t0 = (int)blockIdx.x % ec_tiles_t(nt) * EC_BN;
  if (d0 >= nd || t0 >= nt) return;
  const int tid = threadIdx.x;
  const int ar = ec_arow(tid), br = ec_brow(tid);
  const double* ap = A + (size_t)(d0 + ar < nd ? d0 + ar : 0) * F;
  const double* bp = B + (size_t)(t0 + br < nt ? t0 + br : 0) * F;
  dist_tile(lds, nrm, F, d0, t0, nd, nt, ap, bp, out, nt);
}

// np.vstack(list(features)).mean(0) of one track's ring after `cnt` pushes: the rows present,
// oldest first, summed row by row and divided by their number; one wave, lane-strided over F
__device__ __forceinline__ void bank_mean(const double* bank, int cnt, int F, int lane,
                                          double* out) {
  const int n = cnt < BANK ? cnt : BANK;
  const int first = cnt < BANK ? 0 : cnt % BANK;
  for (int q = lane; q < F; q += 64) {
    double s = 0.0;
    for (int k = 0; k < n; k++) {
      int row = first + k;
      if (row >= BANK) row -= BANK;
      const double v = bank[(size_t)row * F + q];
      s = k ? s + v : v;
    }
    out[q] = s / (double)n;
  }
}

__global__ void __launch_bounds__(64)
    hyb_bank_mean_op_kernel(int nt, int F, const double* __restrict__ bank,
                            const int* __restrict__ cnt, double* __restrict__ out) {
  const int t = blockIdx.x;
  if (t >= nt || cnt[t] <= 0) return;
  bank_mean(bank + (size_t)t * BANK * F, cnt[t], F, threadIdx.x, out + (size_t)t * F);
}

// KalmanBoxTracker.camera_update (hybridsort.py:237-249) of one track, by one lane: state ->
// corner box -> the two warped corners -> convert_bbox_to_z, all float64; only x[0], x[1], x[2]
// and x[4] are written (the score passes through).  numpy's `warp @ [x, y, 1]` of a 2x3 is BLAS's
// gemv, whose row sum is fma(m0, x, m1 * y) + m2 (pinned by tests/golden/hybcmc_*.npz): the
// fma is the one fused operation of the phase, spelled out; nothing else contracts.  A state
// score of exactly 0 is where the reference raises (convert_bbox_to_z returns 4 rows): the track
// is left as it was and counted; returns whether it was.
__device__ __forceinline__ bool hyb_camera_update(HybTrk& t, const double* w) {
  if (t.x[3] == 0.0) return true;
  double b[4];
  x9_to_bbox(t.x, b);
  const double x1 = fma(w[0], b[0], w[1] * b[1]) + w[2], y1 = fma(w[3], b[0], w[4] * b[1]) + w[5];
  const double x2 = fma(w[0], b[2], w[1] * b[3]) + w[2], y2 = fma(w[3], b[2], w[4] * b[3]) + w[5];
  const double bw = x2 - x1, bh = y2 - y1;
  t.x[0] = x1 + bw / 2.0;
  t.x[1] = y1 + bh / 2.0;
  t.x[2] = bw * bh;
  t.x[4] = bw / (bh + 1e-6);
  return false;
}

// The camera-update phase of the frame (hybridsort.py:448-451), ahead of hyb_frame_kernel on the
// same stream and launched only by an engine that has ECC switches: one wave per sequence of the
// call, a lane per live track, for the sequences whose switch is on - under the identity (a null
// table) too.  sw: [S][2] per engine sequence, the switch and the tracks skipped for a score of
// 0; warps: [nseq][6] of the call, or null.  A phase of its own launch and not a second
// instantiation of the frame kernel: see DESIGN.md 2.28.
__global__ void __launch_bounds__(OW)
    hyb_camera_kernel(HybDev gd, int seq0, int* __restrict__ sw, const double* __restrict__ warps) {
  const int b = blockIdx.x, seq = seq0 + b;
  if (!sw[2 * seq]) return;  // workgroup-uniform
  const int T = gd.o.T, lane = threadIdx.x;
  int nt = gd.o.seqst[(size_t)seq * SQO + SO_NTR];
  if (nt > T) nt = T;
  const int* order = gd.o.order + (size_t)seq * T;
  HybTrk* trk = gd.trk + (size_t)seq * T;
  double w[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (warps)
    for (int q = 0; q < 6; q++) w[q] = warps[(size_t)b * 6 + q];
  int skipped = 0;
  for (int c = 0; c < nt; c += OW) {
    const int p = c + lane;
    bool sk = false;
    if (p < nt) {
      const int slot = order[p];
      if (slot >= 0 && slot < T) sk = hyb_camera_update(trk[slot], w);
    }
    skipped += __popcll(__ballot(sk));
  }
  if (skipped && lane == 0) sw[2 * seq + 1] += skipped;
}

__global__ void __launch_bounds__(OW)
    hyb_frame_kernel(HybDev gd, int seq0, const float* __restrict__ dets,
                     const int* __restrict__ det_off, double* __restrict__ out,
                     int* __restrict__ out_count) {
  extern __shared__ __align__(16) char lds_raw[];
  const int seq = seq0 + blockIdx.x;
  hyb_seq_override(gd, seq);  // this sequence's own parameters, when the table holds some
  const OcsDev& g = gd.o;
  OcsLds L;
  carve(g, lds_raw, L);
  int* pp = (int*)(lds_raw + gd.x_off);  // [T] pre-frame list position of each kept track
  const int lane = threadIdx.x;
  L.jv.dc = nullptr;
  const OcsFrame F = ocs_frame_begin<HTB>(g, L, seq, dets, det_off);
  HybTrk* trk = gd.trk + (size_t)seq * g.T;
  double* tb = F.tb;
  const double* ec0 = gd.ec + (size_t)seq * 2 * g.D * g.T;
  const double* ec1 = ec0 + (size_t)g.D * g.T;
  int* rec = gd.rec + (size_t)seq * g.D;
  int* rec_b = gd.rec_b + (size_t)seq * g.D;
  const int nt0 = F.nt0;
  const double thr = F.thr, fw = F.fw, fh = F.fh;
  const int ak = F.ak;
  for (int i = lane; i < F.n; i += OW) rec[i] = -1;
  __syncthreads();
  // remain_inds = scores > det_thresh on the float32 scores (hybridsort.py:466); the rest of the
  // frame's detections is dropped (the BYTE round that would take some of it is not built)
  const float dthr = (float)g.det_thresh;
  const int nh = wave_compact(
      F.n, [&](int i) { return (float)L.dd[6 * i + 4] > dthr; }, [&](int i, int p) { L.hi[p] = i; });

  // cls and det_ind of a kept detection are read from dets0 = [dets, scores], the UNFILTERED
  // frame, at the detection's index among the kept ones (hybridsort.py:458,467,604,709): the
  // class of another row wherever a detection under det_thresh precedes it, and its score
  // column for det_ind.  Kept as the reference has it.
  auto d0cls = [&](int dk) { return L.dd[6 * dk + 5]; };
  auto d0ind = [&](int dk) { return L.dd[6 * dk + 4]; };

  const int grp = lane >> 4, r16 = lane & 15, rr = r16 < HX ? r16 : HX - 1;

  // predict every track (16 lanes per track); tracks whose prediction has a NaN leave the list
  // (hybridsort.py:474-488).  tb row per kept track as laid out at HTB
  int nt = 0;
  for (int c = 0; c < nt0; c += 4) {
    const int p = c + grp;
    bool keep = false;
    int slot = -1;
    double v0 = 0.0, v1 = 0.0;  // this lane's two tb entries: [r16] and [16 + r16]
    if (p < nt0) {
      slot = L.lst2[p];
      HybTrk& t = trk[slot];
      Kf9 k;
      row_load9(t.x, t.P, rr, k);
      if ((hsh(k.x, 7) + hsh(k.x, 2)) <= 0 && rr == 7) k.x *= 0.0;
      kf9_predict(gd, rr, k);
      row_store9(t.x, t.P, r16, k);
      const int age = t.age + 1;
      if (r16 == 0) {
        t.age = age;
        if (t.tsu > 0) t.hit_streak = 0;
        t.tsu++;
      }
      double xs[5], bx[4];
#pragma unroll
      for (int q = 0; q < 5; q++) xs[q] = hsh(k.x, q);
      x9_to_bbox(xs, bx);
      keep = !(isnan(bx[0]) || isnan(bx[1]) || isnan(bx[2]) || isnan(bx[3]) || isnan(xs[3]));
      // np.clip(kf.x[3], 0.6, 1.0) and the simple score around confidence_pre, the latter in the
      // float32 of the stored confidences (hybridsort.py:330-341)
      const double ks = fmin(fmax(xs[3], 0.6), 1.0);
      const float cf = t.confidence;
      const float sraw = (t.has_pre && t.conf_pre != 0.0f) ? cf - (t.conf_pre - cf) : cf;
      const double ss = (double)fminf(fmaxf(sraw, 0.1f), 0.6f);
      // k_previous_obs (hybridsort.py:25-33) with the post-predict age
      int qq = -1;
      const int last_age = t.last_age;
      if (last_age >= 0) {
        qq = obs_first(t, age - g.delta_t, g.delta_t);
        if (qq < 0) qq = last_age & (OBS_KEEP - 1);  // observations[max(keys)]
      }
      auto val = [&](int e) -> double {
        if (e < 4) return e == 0 ? bx[0] : e == 1 ? bx[1] : e == 2 ? bx[2] : bx[3];
        if (e == HT_KS) return ks;
        if (e == HT_SS) return ss;
        if (e < HT_LAST) return qq < 0 ? -1.0 : t.obs_box[qq][e - HT_KOBS];
        if (e < HT_VEL) return t.last_obs[e - HT_LAST];
        return t.has_vel ? t.vel[(e - HT_VEL) >> 1][(e - HT_VEL) & 1] : 0.0;
      };
      v0 = val(r16);
      if (r16 < HTB - 16) v1 = val(16 + r16);
    }
    const unsigned long long m = __ballot(keep && r16 == 0);
    if (keep) {
      const int q = nt + __popcll(m & ((1ull << (lane & ~15)) - 1ull));
      if (r16 == 0) {
        L.lst[q] = slot;
        pp[q] = p;
      }
      double* row = tb + (size_t)q * HTB;
      row[r16] = v0;
      if (r16 < HTB - 16) row[16 + r16] = v1;
    }
    nt += __popcll(m);
  }
  __syncthreads();

  // ---- first association (association.py:537-644): always the LAP ---------------------------
  int nmi = 0;
  if (nt > 0 && nh > 0) {
    double* C = ocs_cost_buf(g, L, F, nh, nt);
    for (int c = 0; c < nt; c += OW) {
      const int ti = c + lane;
      if (ti < nt) {
        const double* r = tb + (size_t)ti * HTB;
        const double* p = r + HT_KOBS;
        const double ks = r[HT_KS];
        const double valid = p[4] < 0 ? 0.0 : 1.0;
        const int col = pp[ti];
        for (int d = 0; d < nh; d++) {
          const int i = L.hi[d];
          const double* a = L.dd + 6 * i;
          const double o = asso_pair(ak, a, r, fw, fh);
          // cost_vel of the four corners (speed_direction_batch_lt/_rt/_lb/_rb against the
          // k-previous observation), each scaled by the detection score, summed lt+rt+lb+rb
          double ang = 0.0;
          for (int cn = 0; cn < 4; cn++) {
            const int ix = cn < 2 ? 0 : 2, iy = (cn & 1) ? 3 : 1;
            double dx = a[ix] - p[ix], dy = a[iy] - p[iy];
            const double norm = sqrt(dx * dx + dy * dy) + 1e-6;
            dx = dx / norm;
            dy = dy / norm;
            const double vy = r[HT_VEL + 2 * cn], vx = r[HT_VEL + 2 * cn + 1];
            double cth = vx * dx + vy * dy;
            cth = cth < -1 ? -1 : (cth > 1 ? 1 : cth);
            double an = ocs_acos(cth);
            an = (3.14159265358979323846 / 2.0 - fabs(an)) / 3.14159265358979323846;
            const double mc = ((valid * an) * g.inertia) * a[4];
            ang = cn ? ang + mc : mc;
          }
          const double sd = fabs(ks - a[4]);
          ang = ang - sd * gd.tcm_w;
          const double e0 = ec0[(size_t)i * g.T + col], e1 = ec1[(size_t)i * g.T + col];
          C[d * nt + ti] = (1.0 * (-(o + ang)) + 1.3 * e0) + gd.lt_w * e1;
        }
      }
    }
    __syncthreads();
    nmi = ocs_lap(C, nh, nt, L.jv, L.mi);
  }
  // the correction filter (association.py:608-637): a pair is dropped only if the embedding is far
  // AND iou - score_dif is under the threshold
  const OcsSplit sp = ocs_split(g, L, nh, nt, nmi, [&](int d, int ti) {
    const int i = L.hi[d];
    const double* r = tb + (size_t)ti * HTB;
    const double o = asso_pair(ak, L.dd + 6 * i, r, fw, fh);
    const double sd = fabs(r[HT_KS] - L.dd[6 * i + 4]);
    const double e0 = ec0[(size_t)i * g.T + pp[ti]];
    return !(e0 > 0.4 && (o - sd) < thr);
  });
  // update(det) of list position ti with the dk-th kept detection, 16 lanes wide
  auto update = [&](int dk, int ti) {
    hyb_update_det(gd, trk[L.lst[ti]], r16, L.dd + 6 * L.hi[dk], d0cls(dk), d0ind(dk));
  };
  ocs_each<16>(sp.nm, [&](int q) {
    const int dk = L.mm[2 * q], ti = L.mm[2 * q + 1];
    update(dk, ti);
    if (r16 == 0) {
      rec_b[L.hi[dk]] = 0;
      rec[L.hi[dk]] = L.lst[ti];
    }
  });
  __syncthreads();

  // ---- OCR round on the last observations (hybridsort.py:666-700); no feature update --------
  const OcsRematch u =
      ocs_rematch<HTB, 16>(g, L, F, nh, nt, sp.nud, L.hi, L.ud, sp.nut, HT_LAST, update);
  ocs_each<16>(u.nut, [&](int k) { hyb_update_none(g, trk[L.lst[L.ut[k]]], r16); });

  // ---- new tracks for the unmatched detections (free slots ascending) -----------------------
  const int nnew = ocs_free_slots(g, L, nt, u.nud);
  ocs_each<16>(nnew, [&](int k) {
    const int slot = L.lst2[k];
    const int dk = L.ud[k];
    const int i = L.hi[dk];
    const double* r = L.dd + 6 * i;
    HybTrk& t = trk[slot];
    float zf[5];
    box_to_z(r, zf);
    if (r16 < HX) {  // kf.x[:5] = z; P = diag(10 x5, 10000 x4) (hybridsort.py:164-173)
      t.x[r16] = r16 == 0 ? zf[0] : r16 == 1 ? zf[1] : r16 == 2 ? zf[2] : r16 == 3 ? zf[3]
                 : r16 == 4 ? zf[4] : 0.0;
      const double pd = r16 < 5 ? 10.0 : 10000.0;
#pragma unroll
      for (int j = 0; j < HX; j++) t.P[r16 * HX + j] = j == r16 ? pd : 0.0;
    }
    if (r16 == 0) {
      ocs_born_common(t, F.id0 + k, r[4]);
      t.cls = d0cls(dk);
      t.det_ind = d0ind(dk);
      t.confidence = (float)r[4];
      t.conf_pre = 0.0f;
      t.has_pre = 0;
      for (int q = 0; q < 4; q++) t.vel[q][0] = t.vel[q][1] = 0.0;
      L.lst[nt + k] = slot;
      rec_b[i] = 1;
      rec[i] = slot;
    }
  });
  __syncthreads();

  // ---- outputs in reversed list order, then deletion of the dead (hybridsort.py:716-741); the
  // id as it is: the per-sequence counter starts at 1 (count 0, id + 1)
  ocs_frame_end(g, L, F, trk, out, out_count, nt + nnew, nnew, 0,
                [](const double* x, double* d) { x9_to_bbox(x, d); });
}

// update_features (hybridsort.py:216-235) of the first round's matches and the newborns; wave per
// detection of the frame, 4 per workgroup.  Norms are lane-strided partial sums, then a
// butterfly over the wave.  A newborn's feat, smooth_feat and bank entry are one array in the
// reference, normalised twice in place.
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  return s;
}

__global__ void __launch_bounds__(256)
    hyb_feature_kernel(HybDev g, int seq0, const int* __restrict__ det_off,
                       const double* __restrict__ embs) {
  const int b = blockIdx.y, seq = seq0 + b;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r0 = det_off[b];
  int n = det_off[b + 1] - r0;
  if (n > g.o.D) n = g.o.D;
  if (k >= n) return;  // whole waves leave together
  const int slot = g.rec[(size_t)seq * g.o.D + k];
  if (slot < 0) return;
  const bool born = g.rec_b[(size_t)seq * g.o.D + k] != 0;
  const int F = g.F;
  const size_t ts = (size_t)seq * g.o.T + slot;
  double* e = g.smooth + ts * F;
  double* bank = g.bank + ts * BANK * F;
  const double* x = embs + (size_t)(r0 + k) * F;
  double s = 0.0;
  for (int q = lane; q < F; q += 64) s += x[q] * x[q];
  const double nx = sqrt(wave_sum(s));
  const int cnt = born ? 0 : g.bcnt[ts];
  double* brow = bank + (size_t)(cnt % BANK) * F;
  const double alpha = 0.8, om = 1 - alpha;
  s = 0.0;
  for (int q = lane; q < F; q += 64) {
    const double f = x[q] / nx;
    const double v = born ? f : alpha * e[q] + om * f;
    brow[q] = f;
    e[q] = v;
    s += v * v;
  }
  const double nv = sqrt(wave_sum(s));
  for (int q = lane; q < F; q += 64) {
    e[q] = e[q] / nv;
    if (born) brow[q] = e[q];
  }
  if (lane == 0) g.bcnt[ts] = cnt + 1;
  bank_mean(bank, cnt + 1, F, lane, g.lmean + ts * F);  // each lane reads the columns it wrote
}

__global__ void hyb_reset_kernel(HybDev g, int seq0, int nseq) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nseq * SQO) g.o.seqst[(size_t)seq0 * SQO + k] = (k % SQO == SO_IDS) ? 1 : 0;
}

}  // namespace

struct bx_hybrid : OcsHost {
  HybDev dev;
  bx_hybrid_config cfg;
  void* arena = nullptr;
  size_t lds = 0;
  ClsGlue pc;     // per_class=True: the class state
  BxProbe probe;  // stages: 0 distances, 1 frame, 2 feature
  // per-sequence parameters (bx_hybrid_set_seq_params_host): the device table dev.seqpar points
  // to, allocated by the first set, and its host mirror
  BxSeqTable<HybSeqPar> seqtab;
  // the ECC switch (bx_hybrid_set_ecc_host): [S][2] on the device (switch, score-zero skips),
  // allocated by the first call that switches a sequence on; null until then, and no camera
  // kernel is launched.  ecc_on: the switches' host mirror
  int* ecc = nullptr;
  std::vector<int> ecc_on;
  // the update_host forms' warps: device buffer and pinned mirror, [S][6], on first use
  double *h_warp = nullptr, *p_warp = nullptr;
};

// the field checks bx_hybrid_create and bx_hybrid_set_seq_params_host share
static bool bad_delta_t(int delta_t) { return delta_t < 1 || delta_t > OBS_KEEP - 1; }
static bool bad_asso_kind(int k) { return k < ASSO_IOU || k > ASSO_CENTROID; }

static int launch(bx_hybrid* e, int seq0, int nseq, const float* dets, const int* off,
                  const double* embs, const double* warps, double* out, int* cnt,
                  hipStream_t st) {
  const HybDev& d = e->dev;
  int rc;
  if (!embs) return bx_record_error(BX_ERR_SHAPE, "HybridSort needs embeddings");
  if ((rc = e->probe.begin(0, st))) return rc;
  hipLaunchKernelGGL(hyb_dist_kernel, dim3(nseq, ec_tiles(d.o.D, d.o.T), 2), dim3(256), 0, st, d,
                     seq0, off, embs);
  BX_HIPCHK(hipGetLastError());
  if ((rc = e->probe.end(0, st))) return rc;
  if ((rc = e->probe.begin(1, st))) return rc;
  if (e->ecc) {  // (null until a sequence is switched on: the frame's launches as they always were)
    hipLaunchKernelGGL(hyb_camera_kernel, dim3(nseq), dim3(OW), 0, st, d, seq0, e->ecc, warps);
    BX_HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(hyb_frame_kernel, dim3(nseq), dim3(OW), e->lds, st, d, seq0, dets, off, out,
                     cnt);
  BX_HIPCHK(hipGetLastError());
  if ((rc = e->probe.end(1, st))) return rc;
  if ((rc = e->probe.begin(2, st))) return rc;
  hipLaunchKernelGGL(hyb_feature_kernel, dim3((d.o.D + 3) / 4, nseq), dim3(256), 0, st, d, seq0,
                     off, embs);
  BX_HIPCHK(hipGetLastError());
  if ((rc = e->probe.end(2, st))) return rc;
  return BX_OK;
}

// a host warp table [n][6] through the pinned mirror to the device buffer on `st` (null: none)
static int put_warps(bx_hybrid* e, const double* warps_host, int n, hipStream_t st,
                     const double** dev) {
  *dev = nullptr;
  if (!warps_host) return BX_OK;
  if (!e->h_warp) {
    const size_t bytes = sizeof(double) * 6 * e->dev.o.S;
    BX_HIPCHK(hipMalloc(&e->h_warp, bytes));
    BX_HIPCHK(hipHostMalloc(&e->p_warp, bytes));
  }
  memcpy(e->p_warp, warps_host, sizeof(double) * 6 * n);
  BX_HIPCHK(hipMemcpyAsync(e->h_warp, e->p_warp, sizeof(double) * 6 * n, hipMemcpyHostToDevice, st));
  *dev = e->h_warp;
  return BX_OK;
}

// the switch table on first use: zeroed, every sequence off
static int ecc_alloc(bx_hybrid* e) {
  if (e->ecc) return BX_OK;
  const size_t S = e->dev.o.S;
  int* p = nullptr;
  if (hipMalloc(&p, S * 2 * sizeof(int)) != hipSuccess)
    return bx_record_error(BX_ERR_HIP, "allocation of the HybridSort ECC switches failed");
  if (hipMemset(p, 0, S * 2 * sizeof(int)) != hipSuccess) {
    (void)hipFree(p);
    return bx_record_error(BX_ERR_HIP, "allocation of the HybridSort ECC switches failed");
  }
  e->ecc = p;
  e->ecc_on.assign(S, 0);
  return BX_OK;
}

// bytes of one sequence's state in bx_hybrid_state_save_host's layout
static size_t state_bytes(const HybDev& d) {
  const size_t T = d.o.T, F = d.F;
  return SQO * sizeof(int) + T * sizeof(int) * 2 + T * sizeof(HybTrk) +
         T * F * sizeof(double) * (2 + BANK);
}

extern "C" {

int bx_hybrid_create(const bx_hybrid_config* c, bx_hybrid** out) {
  if (!c || !out) return bx_record_error(BX_ERR_INVALID, "null argument");
  if (c->n_seq <= 0 || c->track_cap <= 0 || c->det_cap <= 0 || c->track_cap > 512 ||
      c->det_cap > 512)
    return bx_record_error(BX_ERR_INVALID, "n_seq/track_cap/det_cap out of range");
  if (bad_delta_t(c->delta_t))
    return bx_record_error(BX_ERR_INVALID, "delta_t must be in [1, 7]");
  if (c->emb_dim <= 0) return bx_record_error(BX_ERR_INVALID, "emb_dim must be positive");
  if (c->det_thresh < 0.0) return bx_record_error(BX_ERR_INVALID, "det_thresh must be >= 0");
  if (bad_asso_kind(c->asso_kind))
    return bx_record_error(BX_ERR_INVALID, "unknown asso_kind");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return bx_record_error(BX_ERR_NO_DEVICE, "no HIP device visible");
  bx_hybrid* e = new bx_hybrid();
  e->cfg = *c;
  e->o = &e->dev.o;
  // everything that can fail runs in `fill`: a failure frees what was allocated so far
  auto fill = [&]() -> int {
    HybDev& dd = e->dev;
    OcsDev& d = dd.o;
    d.S = c->n_seq;
    d.T = c->track_cap;
    d.D = c->det_cap;
    d.N = d.T > d.D ? d.T : d.D;
    d.min_conf = 0.0;
    d.det_thresh = c->det_thresh;
    d.asso_threshold = c->iou_threshold;
    d.inertia = c->inertia;
    d.q_xy = d.q_s = 0.0;
    d.max_age = c->max_age;
    d.min_hits = c->min_hits;
    d.delta_t = c->delta_t;
    d.use_byte = 0;
    d.asso_kind = c->asso_kind;
    // basetracker.py:59-62: max_obs = 50, or max_age + 5 when max_age >= 50
    d.max_obs = c->max_age >= 50 ? c->max_age + 5 : 50;
    dd.F = c->emb_dim;
    dd.tcm_w = c->tcm_first_step_weight;
    dd.lt_w = c->longterm_reid_weight;
    // Q = I; Q[-1,-1] *= .01; Q[-2,-2] *= .01; Q[5:,5:] *= .01 (hybridsort.py:169-171)
    for (int k = 0; k < HX; k++) dd.q[k] = 1.0;
    dd.q[8] *= 0.01;
    dd.q[7] *= 0.01;
    for (int k = 5; k < HX; k++) dd.q[k] *= 0.01;
    size_t x_off;
    int rc = ocs_lds_budget(d, ((size_t)d.T * 4 + 7) / 8 * 8, &x_off, &e->lds);
    if (rc) return rc;
    dd.x_off = (int)x_off;
    const bool need_g = (long)d.D * d.T > d.cost_lds;
    const size_t S = d.S, T = d.T, D = d.D, F = dd.F;
    BxCarve carve_b;
    const size_t o_trk = carve_b(S * T * sizeof(HybTrk));
    const size_t o_sq = carve_b(S * SQO * sizeof(int));
    const size_t o_ord = carve_b(S * T * sizeof(int));
    const size_t o_tb = carve_b(S * T * HTB * sizeof(double));
    const size_t o_cg = need_g ? carve_b(S * D * T * sizeof(double)) : 0;
    const size_t o_st = carve_b(sizeof(int) * 4);
    const size_t o_fsz = carve_b(S * 2 * sizeof(double));
    const size_t o_sm = carve_b(S * T * F * sizeof(double));
    const size_t o_lm = carve_b(S * T * F * sizeof(double));
    const size_t o_bk = carve_b(S * T * BANK * F * sizeof(double));
    const size_t o_bc = carve_b(S * T * sizeof(int));
    const size_t o_ec = carve_b(S * 2 * D * T * sizeof(double));
    const size_t o_rec = carve_b(S * D * sizeof(int));
    const size_t o_rb = carve_b(S * D * sizeof(int));
    if (hipMalloc(&e->arena, carve_b.off) != hipSuccess)
      return bx_record_error(BX_ERR_HIP, "hipMalloc of the HybridSort arena failed");
    BX_HIPCHK(hipMemset(e->arena, 0, carve_b.off));
    char* base = (char*)e->arena;
    dd.trk = (HybTrk*)(base + o_trk);
    d.trk = nullptr;
    d.seqst = (int*)(base + o_sq);
    d.order = (int*)(base + o_ord);
    d.tb = (double*)(base + o_tb);
    d.cost_g = need_g ? (double*)(base + o_cg) : nullptr;
    d.status = (int*)(base + o_st);
    d.fsz = (double*)(base + o_fsz);
    d.dbg = nullptr;
    dd.smooth = (double*)(base + o_sm);
    dd.lmean = (double*)(base + o_lm);
    dd.bank = (double*)(base + o_bk);
    dd.bcnt = (int*)(base + o_bc);
    dd.ec = (double*)(base + o_ec);
    dd.rec = (int*)(base + o_rec);
    dd.rec_b = (int*)(base + o_rb);
    if ((rc = ocs_upload_initial(d, c->frame_w, c->frame_h, 1))) return rc;
    BX_HIPCHK(bx_lds_attr((const void*)hyb_frame_kernel, e->lds));
    return e->sg.alloc(sizeof(float) * 6 * D, sizeof(double) * D * F, 0, 8, d.D, SQO);
  };
  const int rc = fill();
  if (rc) {
    bx_hybrid_destroy(e);
    return rc;
  }
  *out = e;
  return BX_OK;
}

int bx_hybrid_copy_state(bx_hybrid* dst, bx_hybrid* src) {
  if (!dst || !src) return bx_record_error(BX_ERR_INVALID, "null engine");
  const OcsDev &a = src->dev.o, &b = dst->dev.o;
  if (a.S != b.S || b.T < a.T || b.D < a.D || src->dev.F != dst->dev.F)
    return bx_record_error(BX_ERR_INVALID, "bx_hybrid_copy_state: destination must have the "
                                           "source's sequences and embedding width and at least "
                                           "its capacities");
  BX_HIPCHK(hipDeviceSynchronize());
  const size_t S = a.S, Ta = a.T, Tb = b.T, F = src->dev.F;
  // [S][T][per_track] arrays: a sequence's tracks are one run in both engines
  auto rows = [&](void* d, const void* s, size_t per_track) {
    for (size_t q = 0; q < S; q++) {
      const hipError_t r = hipMemcpy((char*)d + q * Tb * per_track, (const char*)s + q * Ta * per_track,
                                     Ta * per_track, hipMemcpyDeviceToDevice);
      if (r != hipSuccess) return r;
    }
    return hipSuccess;
  };
  BX_HIPCHK(rows(dst->dev.trk, src->dev.trk, sizeof(HybTrk)));
  BX_HIPCHK(rows(b.order, a.order, sizeof(int)));
  BX_HIPCHK(rows(dst->dev.bcnt, src->dev.bcnt, sizeof(int)));
  BX_HIPCHK(rows(dst->dev.smooth, src->dev.smooth, F * sizeof(double)));
  BX_HIPCHK(rows(dst->dev.lmean, src->dev.lmean, F * sizeof(double)));
  BX_HIPCHK(rows(dst->dev.bank, src->dev.bank, BANK * F * sizeof(double)));
  BX_HIPCHK(hipMemcpy(b.seqst, a.seqst, S * SQO * sizeof(int), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.fsz, a.fsz, S * 2 * sizeof(double), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.status, a.status, 4 * sizeof(int), hipMemcpyDeviceToDevice));
  dst->cache_seq = -1;
  BX_HIPCHK(hipDeviceSynchronize());
  // the ECC switches and skip counts: the source's, or all off for a source that never set one
  if (src->ecc) {
    if (int rc = ecc_alloc(dst)) return rc;
    BX_HIPCHK(hipMemcpy(dst->ecc, src->ecc, S * 2 * sizeof(int), hipMemcpyDeviceToDevice));
    dst->ecc_on = src->ecc_on;
  } else if (dst->ecc) {
    BX_HIPCHK(hipMemset(dst->ecc, 0, S * 2 * sizeof(int)));
    dst->ecc_on.assign(S, 0);
  }
  return cls_glue_copy(dst->pc, src->pc, b.S, b.D, dst->dev.F, 1);
}

int bx_hybrid_destroy(bx_hybrid* e) {
  if (!e) return BX_OK;
  e->probe.destroy();
  (void)hipFree(e->arena);
  (void)hipFree(e->ecc);
  (void)hipFree(e->h_warp);
  (void)hipHostFree(e->p_warp);
  e->seqtab.free();
  e->sg.free();
  cls_glue_free(e->pc);
  delete e;
  return BX_OK;
}

int bx_hybrid_reset(bx_hybrid* e, int seq0, int nseq, void* stream) {
  if (!e || seq0 < 0 || nseq < 0 || seq0 + nseq > e->dev.o.S)
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  if (!nseq) return BX_OK;
  e->cache_seq = -1;
  hipLaunchKernelGGL(hyb_reset_kernel, dim3((nseq * SQO + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, e->dev, seq0, nseq);
  BX_HIPCHK(hipGetLastError());
  if (e->ecc) {  // the range's switches go off, its skip counts to 0
    BX_HIPCHK(hipMemsetAsync(e->ecc + 2 * (size_t)seq0, 0, sizeof(int) * 2 * nseq,
                             (hipStream_t)stream));
    for (int k = 0; k < nseq; k++) e->ecc_on[seq0 + k] = 0;
  }
  return cls_glue_reset(e->pc, seq0, nseq, stream);
}

int bx_hybrid_step_cmc(bx_hybrid* e, int seq0, int nseq, const float* dets,
                       const int32_t* det_off, const double* embs, const double* warps,
                       double* out, int32_t* out_count, void* stream) {
  if (!e || seq0 < 0 || nseq <= 0 || seq0 + nseq > e->dev.o.S || !det_off || !out || !out_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_step");
  e->cache_seq = -1;
  return launch(e, seq0, nseq, dets, det_off, embs, warps, out, out_count, (hipStream_t)stream);
}

int bx_hybrid_step(bx_hybrid* e, int seq0, int nseq, const float* dets, const int32_t* det_off,
                   const double* embs, double* out, int32_t* out_count, void* stream) {
  return bx_hybrid_step_cmc(e, seq0, nseq, dets, det_off, embs, nullptr, out, out_count, stream);
}

int bx_hybrid_update_host_cmc(bx_hybrid* e, int seq, const float* dets, int n,
                              const double* embs, const double* warp_host, double* out,
                              int* n_out, void* stream) {
  if (!e || seq < 0 || seq >= e->dev.o.S || n < 0 || (n && (!dets || !out)) || !n_out)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_update_host");
  if (n > e->dev.o.D) return bx_record_error(BX_ERR_CAPACITY, "detections exceed det_cap");
  const size_t F = e->dev.F;
  if (n && !embs) return bx_record_error(BX_ERR_SHAPE, "HybridSort needs embeddings");
  hipStream_t st = (hipStream_t)stream;
  BxStaging& sg = e->sg;
  int rc;
  if (n && (rc = sg.put(sg.h_embs, sg.p_embs, embs, sizeof(double) * F * n, st))) return rc;
  const double* warp = nullptr;
  if ((rc = put_warps(e, warp_host, 1, st, &warp))) return rc;
  return ocs_update_host_roundtrip(
      *e, seq, dets, n, out, n_out, st, true,
      [&] {
        return launch(e, seq, 1, (float*)sg.h_dets, sg.h_off, (double*)sg.h_embs, warp, sg.h_out,
                      sg.h_cnt, st);
      },
      OcsStreamSync{st});
}

int bx_hybrid_update_host(bx_hybrid* e, int seq, const float* dets, int n, const double* embs,
                          double* out, int* n_out, void* stream) {
  return bx_hybrid_update_host_cmc(e, seq, dets, n, embs, nullptr, out, n_out, stream);
}

int bx_hybrid_set_ecc_host(bx_hybrid* e, int seq0, int nseq, const int32_t* on) {
  if (!e || seq0 < 0 || nseq < 0 || seq0 > e->dev.o.S - nseq)
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  if (nseq && !on) return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_set_ecc_host");
  bool any = false;
  for (int k = 0; k < nseq; k++) any = any || on[k] != 0;
  if (!nseq || (!any && !e->ecc)) return BX_OK;  // (nothing to switch off)
  BX_HIPCHK(hipDeviceSynchronize());  // a reset's clear of the range may still be queued
  if (int rc = ecc_alloc(e)) return rc;
  // one strided copy: the switches are the first int of each [2] entry, the counts stay
  std::vector<int> v(nseq);
  for (int k = 0; k < nseq; k++) v[k] = on[k] != 0;
  BX_HIPCHK(hipMemcpy2D(e->ecc + 2 * (size_t)seq0, 2 * sizeof(int), v.data(), sizeof(int),
                        sizeof(int), nseq, hipMemcpyHostToDevice));
  for (int k = 0; k < nseq; k++) e->ecc_on[seq0 + k] = v[k];
  return BX_OK;
}

int bx_hybrid_ecc_host(bx_hybrid* e, int seq, int* on, int* score_zero_skips) {
  if (!e || seq < 0 || seq >= e->dev.o.S)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_ecc_host");
  if (on) *on = e->ecc ? e->ecc_on[seq] : 0;
  if (score_zero_skips) {
    *score_zero_skips = 0;
    if (e->ecc) {
      BX_HIPCHK(hipDeviceSynchronize());
      BX_HIPCHK(hipMemcpy(score_zero_skips, e->ecc + 2 * (size_t)seq + 1, sizeof(int),
                          hipMemcpyDeviceToHost));
    }
  }
  return BX_OK;
}

int bx_hybrid_set_seq_params_host(bx_hybrid* e, int seq0, int nseq,
                                  const bx_hybrid_seq_params* params_host, void* stream) {
  if (!e || e->seqtab.bad_range(seq0, nseq, e->dev.o.S))
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  for (int k = 0; params_host && k < nseq; k++) {  // every entry first: a bad one changes nothing
    if (bad_delta_t(params_host[k].delta_t))
      return bx_record_error(BX_ERR_INVALID, "delta_t must be in [1, 7]");
    if (!(params_host[k].det_thresh >= 0.0))
      return bx_record_error(BX_ERR_INVALID, "det_thresh must be >= 0");
    if (bad_asso_kind(params_host[k].asso_kind))
      return bx_record_error(BX_ERR_INVALID, "unknown asso_kind");
  }
  if (!nseq || (!params_host && !e->seqtab.allocated())) return BX_OK;  // (nothing to clear)
  std::vector<HybSeqPar> stage(nseq, HybSeqPar{});
  for (int k = 0; params_host && k < nseq; k++) {
    const bx_hybrid_seq_params& p = params_host[k];
    HybSeqPar& d = stage[k];
    d.o.det_thresh = p.det_thresh;
    d.o.asso_threshold = p.iou_threshold;
    d.o.inertia = p.inertia;
    d.o.max_age = p.max_age;
    d.o.min_hits = p.min_hits;
    d.o.delta_t = p.delta_t;
    d.o.asso_kind = p.asso_kind;
    d.o.set = 1;
    d.tcm_w = p.tcm_first_step_weight;
    d.lt_w = p.longterm_reid_weight;
  }
  if (int rc = e->seqtab.put(seq0, stage, e->dev.o.S, (hipStream_t)stream,
                             "allocation or copy of the HybridSort parameter table failed"))
    return rc;
  e->dev.seqpar = e->seqtab.dev;
  return BX_OK;
}

int bx_hybrid_seq_params_host(bx_hybrid* e, int seq, bx_hybrid_seq_params* out_host) {
  if (!e || seq < 0 || seq >= e->dev.o.S || !out_host)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_seq_params_host");
  const bx_hybrid_config& c = e->cfg;
  bx_hybrid_seq_params o = {c.det_thresh, c.iou_threshold, c.inertia, c.longterm_reid_weight,
                            c.tcm_first_step_weight, c.max_age, c.min_hits, c.delta_t,
                            c.asso_kind};
  if (const HybSeqPar* d = e->seqtab.set_entry(seq))
    o = {d->o.det_thresh, d->o.asso_threshold, d->o.inertia, d->lt_w, d->tcm_w, d->o.max_age,
         d->o.min_hits, d->o.delta_t, d->o.asso_kind};
  *out_host = o;
  return BX_OK;
}

int bx_hybrid_probe(bx_hybrid* e, int stage) {
  if (!e || stage < -1 || stage > 2) return bx_record_error(BX_ERR_INVALID, "bad probe stage");
  e->probe.set(stage);
  return BX_OK;
}

int bx_hybrid_probe_read(bx_hybrid* e, double* total_ms, int* count) {
  if (!e || !total_ms || !count) return bx_record_error(BX_ERR_INVALID, "null argument");
  return e->probe.read(total_ms, count);
}

// per_class=True (include/bxclasses.h): class c of sequence s is engine sequence s * C + c; the
// frame is split -> the three launches over the class sequences -> merge, all on `stream`.
int bx_hybrid_step_classes_cmc(bx_hybrid* e, int seq0, int nseq, int n_classes,
                               const float* dets, const int32_t* det_off, const double* embs,
                               const double* warps, double* out, int32_t* out_count,
                               void* stream) {
  if (!e) return bx_record_error(BX_ERR_INVALID, "null engine");
  if (!embs) return bx_record_error(BX_ERR_SHAPE, "HybridSort needs embeddings");
  e->cache_seq = -1;
  hipStream_t st = (hipStream_t)stream;
  return cls_glue_step(e->pc, e->dev.o.S, e->dev.o.D, e->dev.F, 1, e->dev.o.seqst + SO_IDS, SQO,
                       seq0, nseq, n_classes, dets, det_off, embs, out, out_count, st,
                       [&](int q0, int nq, const float* d, const int* off, const double* em,
                           double* o, int* cnt) {
                         return launch(e, q0, nq, d, off, em, warps, o, cnt, st);
                       });
}

int bx_hybrid_step_classes(bx_hybrid* e, int seq0, int nseq, int n_classes, const float* dets,
                           const int32_t* det_off, const double* embs, double* out,
                           int32_t* out_count, void* stream) {
  return bx_hybrid_step_classes_cmc(e, seq0, nseq, n_classes, dets, det_off, embs, nullptr, out,
                                    out_count, stream);
}

int bx_hybrid_classes_config(bx_hybrid* e, int n_classes, int map_cap) {
  if (!e || map_cap <= 0) return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_classes_config");
  if (e->pc.cls) return bx_record_error(BX_ERR_INVALID, "the engine's class state already exists");
  e->pc.map_cap = map_cap;
  return cls_glue_get(e->pc, e->dev.o.S, e->dev.o.D, e->dev.F, n_classes, 1);
}

int bx_hybrid_classes(bx_hybrid* e, bx_classes** out) {
  if (!e || !out) return bx_record_error(BX_ERR_INVALID, "null argument");
  *out = e->pc.cls;
  return BX_OK;
}

int bx_hybrid_update_classes_host_cmc(bx_hybrid* e, int seq, int n_classes, const float* dets,
                                      int n, const double* embs, const double* warps_host,
                                      int* id_count, double* out, int* n_out, void* stream) {
  if (!e || seq < 0 || n < 0 || (n && (!dets || !out)) || !n_out || !id_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_update_classes_host");
  if (n > e->dev.o.D) return bx_record_error(BX_ERR_CAPACITY, "detections exceed det_cap");
  const size_t F = e->dev.F;
  if (n && !embs) return bx_record_error(BX_ERR_SHAPE, "HybridSort needs embeddings");
  int rc = cls_glue_get(e->pc, e->dev.o.S, e->dev.o.D, e->dev.F, n_classes, 1);
  if (rc) return rc;
  if ((seq + 1) * (long)n_classes > e->dev.o.S) return bx_record_error(BX_ERR_INVALID, "bad sequence");
  hipStream_t st = (hipStream_t)stream;
  BxStaging& sg = e->sg;
  if (n && (rc = sg.put(sg.h_embs, sg.p_embs, embs, sizeof(double) * F * n, st))) return rc;
  const double* warps = nullptr;
  if ((rc = put_warps(e, warps_host, n_classes, st, &warps))) return rc;
  return ocs_update_host_roundtrip(
      *e, -1, dets, n, out, n_out, st, true,
      [&] {
        if (int r = cls_glue_put_ids(e->pc, seq, *id_count, st)) return r;
        return bx_hybrid_step_classes_cmc(e, seq, 1, n_classes, (float*)sg.h_dets, sg.h_off,
                                          (double*)sg.h_embs, warps, sg.h_out, sg.h_cnt, st);
      },
      [&](int* cstatus) { return cls_glue_take_ids(e->pc, seq, id_count, cstatus, st); });
}

int bx_hybrid_update_classes_host(bx_hybrid* e, int seq, int n_classes, const float* dets, int n,
                                  const double* embs, int* id_count, double* out, int* n_out,
                                  void* stream) {
  return bx_hybrid_update_classes_host_cmc(e, seq, n_classes, dets, n, embs, nullptr, id_count,
                                           out, n_out, stream);
}

int bx_hybrid_status(bx_hybrid* e, int* status) {
  if (!e || !status) return bx_record_error(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipMemcpy(status, e->dev.o.status, sizeof(int), hipMemcpyDeviceToHost));
  return cls_glue_status(e->pc, status);
}

int bx_hybrid_counters_host(bx_hybrid* e, int seq, int* frame_count, int* id_count,
                            int* n_tracks) {
  return ocs_counters(e, seq, frame_count, id_count, n_tracks);
}

int bx_hybrid_set_id_count(bx_hybrid* e, int seq, int id_count, void* stream) {
  return ocs_set_id_count(e, seq, id_count, stream);
}

int bx_hybrid_set_frame_size(bx_hybrid* e, int seq, double w, double h, void* stream) {
  return ocs_set_frame_size(e, seq, w, h, stream);
}

int bx_hybrid_tracks_host(bx_hybrid* e, int seq, int cap, int32_t* ids, double* x, double* p,
                          double* emb, double* bank_mean, double* vel, int32_t* bank_count,
                          int* n) {
  if (!e || seq < 0 || seq >= e->dev.o.S || cap < 0 || !n)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_tracks_host");
  std::vector<int> ord;
  int rc = ocs_list_order(e->dev.o, seq, ord);
  if (rc) return rc;
  const int nt = (int)ord.size();
  const size_t F = e->dev.F, T = e->dev.o.T;
  for (int k = 0; k < nt && k < cap; k++) {
    HybTrk t;
    const size_t ts = (size_t)seq * T + ord[k];
    BX_HIPCHK(hipMemcpy(&t, e->dev.trk + ts, sizeof(HybTrk), hipMemcpyDeviceToHost));
    if (ids) ids[k] = t.id;
    if (x) memcpy(x + HX * k, t.x, sizeof(t.x));
    if (p) memcpy(p + HX * HX * k, t.P, sizeof(t.P));
    if (emb)
      BX_HIPCHK(hipMemcpy(emb + F * k, e->dev.smooth + ts * F, sizeof(double) * F, hipMemcpyDeviceToHost));
    if (bank_mean)
      BX_HIPCHK(hipMemcpy(bank_mean + F * k, e->dev.lmean + ts * F, sizeof(double) * F,
                     hipMemcpyDeviceToHost));
    if (vel)  // zeros until the second update, as the reference's None is read
      for (int c = 0; c < 8; c++) vel[8 * k + c] = t.has_vel ? t.vel[c >> 1][c & 1] : 0.0;
    if (bank_count)
      BX_HIPCHK(hipMemcpy(bank_count + k, e->dev.bcnt + ts, sizeof(int), hipMemcpyDeviceToHost));
  }
  *n = nt;
  return BX_OK;
}

int bx_hybrid_state_set_host(bx_hybrid* e, int seq, int n, const int32_t* ids, const double* x,
                             const double* p) {
  if (!e || seq < 0 || seq >= e->dev.o.S || n < 0 || (n && !ids))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_state_set_host");
  std::vector<int> ord;
  int rc = ocs_list_order(e->dev.o, seq, ord);
  if (rc) return rc;
  for (int j = 0; j < n; j++) {
    HybTrk t;
    int slot;
    if ((rc = ocs_find_track(e->dev.o, e->dev.trk, seq, ord, ids[j], t, &slot))) return rc;
    if (x) memcpy(t.x, x + HX * j, sizeof(t.x));
    if (p) memcpy(t.P, p + HX * HX * j, sizeof(t.P));
    BX_HIPCHK(hipMemcpy(e->dev.trk + (size_t)seq * e->dev.o.T + slot, &t, sizeof(HybTrk),
                   hipMemcpyHostToDevice));
  }
  return BX_OK;
}

int bx_hybrid_state_bytes(bx_hybrid* e, size_t* bytes) {
  if (!e || !bytes) return bx_record_error(BX_ERR_INVALID, "null argument");
  *bytes = state_bytes(e->dev);
  return BX_OK;
}

// one sequence's whole state, to or from a host blob: counters, list order, bank counts, track
// records, smooth features, bank means, banks
static int state_xfer(bx_hybrid* e, int seq, char* blob, bool save) {
  const HybDev& d = e->dev;
  const size_t T = d.o.T, F = d.F;
  BX_HIPCHK(hipDeviceSynchronize());
  size_t off = 0;
  auto part = [&](void* dev, size_t bytes) {
    const hipError_t r = save ? hipMemcpy(blob + off, dev, bytes, hipMemcpyDeviceToHost)
                              : hipMemcpy(dev, blob + off, bytes, hipMemcpyHostToDevice);
    off += bytes;
    return r;
  };
  BX_HIPCHK(part(d.o.seqst + (size_t)seq * SQO, SQO * sizeof(int)));
  BX_HIPCHK(part(d.o.order + (size_t)seq * T, T * sizeof(int)));
  BX_HIPCHK(part(d.bcnt + (size_t)seq * T, T * sizeof(int)));
  BX_HIPCHK(part(d.trk + (size_t)seq * T, T * sizeof(HybTrk)));
  BX_HIPCHK(part(d.smooth + (size_t)seq * T * F, T * F * sizeof(double)));
  BX_HIPCHK(part(d.lmean + (size_t)seq * T * F, T * F * sizeof(double)));
  BX_HIPCHK(part(d.bank + (size_t)seq * T * BANK * F, T * BANK * F * sizeof(double)));
  e->cache_seq = -1;
  return BX_OK;
}

int bx_hybrid_state_save_host(bx_hybrid* e, int seq, void* blob, size_t bytes) {
  if (!e || seq < 0 || seq >= e->dev.o.S || !blob || bytes != state_bytes(e->dev))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_state_save_host");
  return state_xfer(e, seq, (char*)blob, true);
}

int bx_hybrid_state_load_host(bx_hybrid* e, int seq, const void* blob, size_t bytes) {
  if (!e || seq < 0 || seq >= e->dev.o.S || !blob || bytes != state_bytes(e->dev))
    return bx_record_error(BX_ERR_INVALID, "bx_hybrid_state_load_host: the blob must come from an "
                                           "engine with the same track_cap and emb_dim");
  return state_xfer(e, seq, (char*)blob, false);
}

int bx_hybrid_cosdist(int nd, int nt, int F, const double* dets_embs, const double* trk_embs,
                      double* out, void* stream) {
  if (nd < 0 || nt < 0 || F <= 0 || ((nd && nt) && (!dets_embs || !trk_embs || !out)))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_cosdist");
  if (!nd || !nt) return BX_OK;
  hipLaunchKernelGGL(hyb_dist_op_kernel, dim3(ec_tiles(nd, nt)), dim3(256), 0, (hipStream_t)stream,
                     nd, nt, F, dets_embs, trk_embs, out);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_hybrid_bank_mean(int nt, int F, const double* bank, const int32_t* pushed, double* out,
                        void* stream) {
  if (nt < 0 || F <= 0 || (nt && (!bank || !pushed || !out)))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_hybrid_bank_mean");
  if (!nt) return BX_OK;
  hipLaunchKernelGGL(hyb_bank_mean_op_kernel, dim3(nt), dim3(64), 0, (hipStream_t)stream, nt, F,
                     bank, pushed, out);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

}  // extern "C"
