// bx_ocs_device.h — the device code the three OC-SORT-family frame kernels are built from
// (ocsort_frame_kernel, deepoc_frame_kernel, hyb_frame_kernel: one wave64 workgroup per sequence).
// Included inside the including translation unit's anonymous namespace (after bx_device.h), like
// bx_jv.h.
//
// First the records and the XYSR filter of OCSort and DeepOCSort: the track record, the Kalman
// filter on an octet of lanes (predict, update, the ORU replay), KalmanBoxTracker's update(det) /
// update(None), the observation ring, the LDS carve and the legacy lapx LAP.  HybridSort brings
// its own record and 9-state filter and shares the ring, the carve and the LAP.
//
// Then the phases of a frame ("The frame phases" below), in the order a kernel calls them.  They
// are templates over what differs between the kernels and nothing else: the track record, the
// lanes per track W (8 / 16), the `tb` row stride TBS and the offset of the last observation in
// it, and small callables.  Everything inlines; wave-uniform counts go in and out by value.
//   ocs_frame_begin      clamp n (capacity latch), detections and list order into LDS, counters
//   ocs_predict_octet    predict + compact the track list, fill tb        (octet kernels)
//   ocs_pass1_count, ocs_one_to_one   the one-to-one test                  (octet kernels)
//   ocs_cost_fill        -(IoU + direction consistency [+ a kernel's term]) (octet kernels)
//   ocs_split            unmatched lists, accepted pairs, rejected pairs appended (P3/P5)
//   ocs_rematch[_max/_solve]   the OCR round, and OCSort's BYTE round
//   ocs_free_slots, ocs_born_common, ocs_born_octet   births
//   ocs_frame_end        outputs in reversed list order, deletion of the dead, counter row
// A kernel keeps the code that is its own between these calls: OCSort the parameter override, the
// confidence splits and the phase stamps; DeepOCSort the warp, the appearance term and its
// embedding records; HybridSort its filter, predict loop, corner cost and correction rule.

constexpr int OBS_KEEP = 8;   // newest observations kept (lookups reach back delta_t <= 7)
constexpr int SQO = 8;        // ints of per-sequence state
enum { SO_FRAME = 0, SO_IDS = 1, SO_NTR = 2, SO_NOUT = 3 };
constexpr int TB = 16;        // doubles per track of per-frame scratch (box4 kobs5 last5 vel2)

struct OcsTrk {
  double x[7], P[49];
  double sx[7], sP[49];         // freeze() snapshot (attr_saved)
  double hbox[4];               // last non-None entry of history_obs
  double last_obs[5];
  double obs_box[OBS_KEEP][5];  // observations dict: the entry of age a sits in slot a % 8
  double vel[2];
  double conf, cls;
  int obs_age[OBS_KEEP];
  int last_age, has_vel, id, tsu, hits, hit_streak, age, det_ind;  // last_age < 0: no obs
  int observed, has_saved, hvalid, htail;
};

// One sequence's entry of the per-sequence parameter table: the OcsDev fields that size no
// memory.  `set` 0: the sequence runs on the engine's own parameters.
struct OcsSeqPar {
  double min_conf, det_thresh, asso_threshold, inertia, q_xy, q_s;
  int max_age, min_hits, delta_t, use_byte, asso_kind;
  int set;
};

struct OcsDev {
  int S, T, D, N;  // N = max(T, D): largest assignment problem
  double min_conf, det_thresh, asso_threshold, inertia, q_xy, q_s;
  int max_age, min_hits, delta_t, use_byte, max_obs;
  int asso_kind;    // ASSO_* (BaseTracker asso_func): iou unless configured otherwise
  double* fsz;      // [S][2] frame (w, h) per sequence, for the centroid mode
  int cost_lds;     // doubles of LDS for a cost matrix (larger ones go to `cost_g`)
  OcsTrk* trk;      // [S][T]
  int* seqst;       // [S][SQO]
  int* order;       // [S][T] slot ids in the reference's list order
  double* tb;       // [S][T][TB]
  double* cost_g;   // [S][D*T] or null
  int* status;
  unsigned long long* dbg;  // [S][OCS_DBG] phase stamps (diagnostic builds only, else null)
  // [S] per-sequence parameters, or null: none was ever set (OCSort's table: DeepOCSort and
  // HybridSort leave it null and keep a table of their own entry struct in DocDev / HybDev).  A
  // kernel reads it, never writes it.
  const OcsSeqPar* seqpar = nullptr;
};

// The kernel-entry override, in two parts.  ocs_seq_apply puts the eleven shared per-sequence
// fields of one table entry into a kernel's own copy of its OcsDev (and max_obs, which follows
// max_age); everything downstream reads them through `g` as before.  All three frame kernels use
// it: OCSort on an OcsSeqPar entry (ocs_seq_override), DeepOCSort and HybridSort on the OcsSeqPar
// their own entry structs begin with.  `seq` is wave-uniform, so the loads are scalar loads, once
// per workgroup, and all of them come before the first store into `g`.
__device__ __forceinline__ void ocs_seq_apply(OcsDev& g, const OcsSeqPar* p) {
  const double min_conf = p->min_conf, det_thresh = p->det_thresh;
  const double asso_threshold = p->asso_threshold, inertia = p->inertia;
  const double q_xy = p->q_xy, q_s = p->q_s;
  const int max_age = p->max_age, min_hits = p->min_hits, delta_t = p->delta_t;
  const int use_byte = p->use_byte, asso_kind = p->asso_kind;
  g.min_conf = min_conf;
  g.det_thresh = det_thresh;
  g.asso_threshold = asso_threshold;
  g.inertia = inertia;
  g.q_xy = q_xy;
  g.q_s = q_s;
  g.max_age = max_age;
  g.max_obs = max_age >= 50 ? max_age + 5 : 50;  // derived, as the engine's create does
  g.min_hits = min_hits;
  g.delta_t = delta_t;
  g.use_byte = use_byte;
  g.asso_kind = asso_kind;
}

// OCSort's: sequence `seq`'s entry of g.seqpar, when there is a table and the entry is set.
__device__ __forceinline__ void ocs_seq_override(OcsDev& g, int seq) {
  if (!g.seqpar) return;
  const OcsSeqPar* p = g.seqpar + seq;
  if (!p->set) return;
  ocs_seq_apply(g, p);
}

// Diagnostic phase stamps and counters (build with -DBX_PHASE_TIMING; never shipped): per
// sequence, cycles accumulated per phase over all frames [0, 16), event counters [16, 24) and
// the JV's counters [24, 40).
constexpr int OCS_DBG = 40;
#ifdef BX_PHASE_TIMING
#define OSTAMP(k)                                                                    \
  do {                                                                               \
    __syncthreads();                                                                 \
    if (threadIdx.x == 0 && g.dbg) {                                                 \
      const unsigned long long _now = __builtin_amdgcn_s_memtime();                  \
      g.dbg[(size_t)seq * OCS_DBG + (k)] += _now - t_last;                           \
      t_last = _now;                                                                 \
    }                                                                                \
  } while (0)
#define OCOUNT(k, v)                                                                 \
  do {                                                                               \
    if (threadIdx.x == 0 && g.dbg) g.dbg[(size_t)seq * OCS_DBG + 16 + (k)] += (v);   \
  } while (0)
#else
#define OSTAMP(k) \
  do {            \
  } while (0)
#define OCOUNT(k, v) \
  do {               \
  } while (0)
#endif

// ------------------------------------------------------------------------------------------
// fdlibm acos (oracle/bxo_ocsort.c bxo_acos)
__device__ double ocs_acos(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17,
               pi_c = 3.14159265358979311600e+00, pS0 = 1.66666666666666657415e-01,
               pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04,
               pS5 = 3.47933107596021167570e-05, qS1 = -2.40339491173441421878e+00,
               qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  const long long bits = __double_as_longlong(x);
  const int hx = (int)(bits >> 32);
  const int ix = hx & 0x7fffffff;
  if (ix >= 0x3ff00000) {
    if (x == 1.0) return 0.0;
    if (x == -1.0) return pi_c + 2.0 * pio2_lo;
    return __builtin_nan("");
  }
  if (ix < 0x3fe00000) {
    if (ix <= 0x3c600000) return pio2_hi + pio2_lo;
    const double z = x * x;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    return pio2_hi - (x - (pio2_lo - x * r));
  } else if (hx < 0) {
    const double z = (1.0 + x) * 0.5;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double s = sqrt(z);
    const double r = p / q;
    const double w = r * s - pio2_lo;
    return pi_c - 2.0 * (s + w);
  } else {
    const double z = (1.0 - x) * 0.5;
    const double s = sqrt(z);
    const double df = __longlong_as_double(__double_as_longlong(s) & (long long)0xffffffff00000000ULL);
    const double c = (z - df * df) / (s + df);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    const double w = r * s + c;
    return 2.0 * (df + w);
  }
}

// ------------------------------------------------------------------------------------------
// XYSR Kalman filter (xysr_kf.py) on 8 lanes per track (an "octet"): lane r of the octet owns
// row rr = min(r, 6) of the 7-state mean and covariance (lane 7 mirrors row 6 and never writes).
// Every element is computed by one lane with the oracle's operation order (kf_predict7,
// kf_update7_core in oracle/bxo_ocsort.c); shuffles only move operands between rows.
__device__ __forceinline__ double osh(double v, int src) { return __shfl(v, src, 8); }

struct KfRow {
  double x, P[7];
};

__device__ __forceinline__ void row_load(const double* x, const double* P, int rr, KfRow& k) {
  k.x = x[rr];
#pragma unroll
  for (int j = 0; j < 7; j++) k.P[j] = P[rr * 7 + j];
}

__device__ __forceinline__ void row_store(double* x, double* P, int r, const KfRow& k) {
  if (r < 7) {
    x[r] = k.x;
#pragma unroll
    for (int j = 0; j < 7; j++) P[r * 7 + j] = k.P[j];
  }
}

// x = F x ; P = 1.0 * (F P F') + Q  (F = I + e_i e_{i+4}' for i < 3)
__device__ void kfo_predict(const OcsDev& g, int rr, KfRow& k) {
  const int src = rr < 3 ? rr + 4 : rr;
  const double x4 = osh(k.x, src);
  k.x = rr < 3 ? k.x + x4 : k.x;
  double FP[7];
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const double p4 = osh(k.P[j], src);
    FP[j] = rr < 3 ? k.P[j] + p4 : k.P[j];
  }
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const double m = j < 3 ? FP[j] + FP[j + 4] : FP[j];
    double q = 0.0;
    if (rr == j) q = (rr == 4 || rr == 5) ? g.q_xy : (rr == 6 ? g.q_s : 1.0);
    k.P[j] = 1.0 * m + q;
  }
}

// np.linalg.inv of a 4x4 (oracle inv4: dgetf2 LU with partial pivoting, then dgetrs).  Row
// swaps are written as predicated swaps over constant indices so both matrices stay in VGPRs.
__device__ __forceinline__ void swap_rows4(double* M, int k, int p) {
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (i > k && i == p)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const double t = M[k * 4 + j];
        M[k * 4 + j] = M[i * 4 + j];
        M[i * 4 + j] = t;
      }
}

__device__ __forceinline__ void inv4(const double* Ain, double* B) {
  double A[16];
  int piv[4];
#pragma unroll
  for (int i = 0; i < 16; i++) A[i] = Ain[i];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int p = k;
    double mx = fabs(A[k * 4 + k]);
#pragma unroll
    for (int i = k + 1; i < 4; i++)
      if (fabs(A[i * 4 + k]) > mx) mx = fabs(A[i * 4 + k]), p = i;
    piv[k] = p;
    swap_rows4(A, k, p);
    if (A[k * 4 + k] != 0.0) {
      if (fabs(A[k * 4 + k]) >= DBL_MIN) {
        const double r = 1.0 / A[k * 4 + k];
#pragma unroll
        for (int i = k + 1; i < 4; i++) A[i * 4 + k] *= r;
      } else {
#pragma unroll
        for (int i = k + 1; i < 4; i++) A[i * 4 + k] /= A[k * 4 + k];
      }
    }
#pragma unroll
    for (int j = k + 1; j < 4; j++) {
      const double t = -A[k * 4 + j];
#pragma unroll
      for (int i = k + 1; i < 4; i++) A[i * 4 + j] = A[i * 4 + j] + A[i * 4 + k] * t;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; i++) B[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) swap_rows4(B, k, piv[k]);
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (B[k * 4 + j] != 0.0)
#pragma unroll
        for (int i = k + 1; i < 4; i++) B[i * 4 + j] -= B[k * 4 + j] * A[i * 4 + k];
#pragma unroll
    for (int k = 3; k >= 0; k--)
      if (B[k * 4 + j] != 0.0) {
        B[k * 4 + j] /= A[k * 4 + k];
#pragma unroll
        for (int i = 0; i < k; i++) B[i * 4 + j] -= B[k * 4 + j] * A[i * 4 + k];
      }
  }
}

// update with a measurement (R = diag(1,1,10,10), H = [I4 0], Joseph form); z uniform per octet
__device__ void kfo_update(int rr, KfRow& k, const double* z) {
  const double Rd[4] = {1.0, 1.0, 10.0, 10.0};
  double y[4], S[16], SI[16];
#pragma unroll
  for (int a = 0; a < 4; a++) y[a] = z[a] - osh(k.x, a);
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) S[a * 4 + b] = osh(k.P[b], a) + (a == b ? Rd[a] : 0.0);
  inv4(S, SI);  // every lane of the octet inverts the same S identically
  double K[4];
#pragma unroll
  for (int b = 0; b < 4; b++) {
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; a++) acc += k.P[a] * SI[a * 4 + b];
    K[b] = acc;
  }
  {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 4; b++) acc += K[b] * y[b];
    k.x = k.x + acc;
  }
  double ikh[7], A[7];
#pragma unroll
  for (int c = 0; c < 7; c++) ikh[c] = (rr == c ? 1.0 : 0.0) - (c < 4 ? K[c] : 0.0);
#pragma unroll
  for (int j = 0; j < 7; j++) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 7; c++) acc += ikh[c] * osh(k.P[j], c);
    A[j] = acc;
  }
#pragma unroll
  for (int j = 0; j < 7; j++) {
    double Kj[4];
#pragma unroll
    for (int b = 0; b < 4; b++) Kj[b] = osh(K[b], j);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 7; c++) acc += A[c] * ((j == c ? 1.0 : 0.0) - (c < 4 ? Kj[c] : 0.0));
    double kr = 0.0;
#pragma unroll
    for (int b = 0; b < 4; b++) kr += (K[b] * Rd[b]) * Kj[b];
    k.P[j] = acc + kr;
  }
}

// ocsort.py:31-45
__device__ void x_to_bbox(const double* x, double* b) {
  const double w = sqrt(x[2] * x[3]);
  const double h = x[2] / w;
  b[0] = x[0] - w / 2.0;
  b[1] = x[1] - h / 2.0;
  b[2] = x[0] + w / 2.0;
  b[3] = x[1] + h / 2.0;
}

__device__ double sum5(const double* b) { return (((b[0] + b[1]) + b[2]) + b[3]) + b[4]; }

// The observations dict (ocsort.py:73,158) is read only at ages within delta_t <= 7 of the
// current age, plus its newest key; keeping the entry of age a in slot a % 8 loses only entries
// at least 8 ages older than a newer one, which no lookup reaches.
// First hit of `want0 + i` for i < cnt (ascending), or -1; the probes are independent loads.
template <class Trk>
__device__ __forceinline__ int obs_first(const Trk& t, int want0, int cnt) {
  int q = -1;
  for (int i = cnt - 1; i >= 0; i--) {
    const int want = want0 + i;
    if (want >= 0 && t.obs_age[want & (OBS_KEEP - 1)] == want) q = want & (OBS_KEEP - 1);
  }
  return q;
}

// ocsort.py:136-171 (update with a detection row [x1,y1,x2,y2,conf] + cls), octet-wide: lane 0
// keeps the track's bookkeeping, the octet runs the Kalman update (with the ORU replay of
// xysr_kf.py:183-209 when the track was frozen)
__device__ void ocs_update_det(const OcsDev& g, OcsTrk& t, int r, const double* b5, double cls,
                               int det_ind) {
  const int rr = r < 7 ? r : 6;
  const int observed = t.observed, has_saved = t.has_saved;
  const int hv = t.hvalid, gap = t.htail + 1;
  const double b1[4] = {t.hbox[0], t.hbox[1], t.hbox[2], t.hbox[3]};
  if (r == 0) {
    t.det_ind = det_ind;
    t.conf = b5[4];
    t.cls = cls;
    if (sum5(t.last_obs) >= 0) {
      const int q = obs_first(t, t.age - g.delta_t, g.delta_t);
      const double* prev = q >= 0 ? t.obs_box[q] : t.last_obs;
      // ocsort.py:48-53 speed_direction
      const double cx1 = (prev[0] + prev[2]) / 2.0, cy1 = (prev[1] + prev[3]) / 2.0;
      const double cx2 = (b5[0] + b5[2]) / 2.0, cy2 = (b5[1] + b5[3]) / 2.0;
      const double sy = cy2 - cy1, sx = cx2 - cx1;
      const double norm = sqrt((cy2 - cy1) * (cy2 - cy1) + (cx2 - cx1) * (cx2 - cx1)) + 1e-6;
      t.vel[0] = sy / norm;
      t.vel[1] = sx / norm;
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
  }
  // P1 xyxy2xysr
  const double w = b5[2] - b5[0], h = b5[3] - b5[1];
  const double z[4] = {b5[0] + w / 2.0, b5[1] + h / 2.0, w * h, w / (h + 1e-6)};
  KfRow k;
  const bool unfreeze = !observed && has_saved;
  if (unfreeze) {
    // new_history = history + [z]: the previous non-None entry is hbox, htail+1 steps back;
    // self.__dict__ = attr_saved restores (x, P); its history is overwritten by z below
    row_load(t.sx, t.sP, rr, k);
    if (hv) {
      const double x1 = b1[0], y1 = b1[1], s1 = b1[2], r1 = b1[3];
      const double w1 = sqrt(s1 * r1), h1 = sqrt(s1 / r1);
      const double x2 = z[0], y2 = z[1], s2 = z[2], r2 = z[3];
      const double w2 = sqrt(s2 * r2), h2 = sqrt(s2 / r2);
      const double dx = (x2 - x1) / gap, dy = (y2 - y1) / gap;
      const double dw = (w2 - w1) / gap, dh = (h2 - h1) / gap;
      for (int i = 0; i < gap; i++) {
        const double xx = x1 + (i + 1) * dx, yy = y1 + (i + 1) * dy;
        const double ww = w1 + (i + 1) * dw, hh = h1 + (i + 1) * dh;
        const double nb[4] = {xx, yy, ww * hh, ww / (double)hh};
        kfo_update(rr, k, nb);
        if (i != gap - 1) kfo_predict(g, rr, k);
      }
    }
  } else {
    row_load(t.x, t.P, rr, k);
  }
  kfo_update(rr, k, z);
  row_store(t.x, t.P, r, k);
  if (r == 0) {
    if (unfreeze) t.has_saved = 0;
    t.observed = 1;
    for (int q = 0; q < 4; q++) t.hbox[q] = z[q];
    t.htail = 0;
    t.hvalid = 1;
  }
}

// update(None), octet-wide: history_obs gets a None; the first miss after an observation
// freezes (x, P)
__device__ void ocs_update_none(const OcsDev& g, OcsTrk& t, int r) {
  const int observed = t.observed;
  if (observed && r < 7) {
    t.sx[r] = t.x[r];
#pragma unroll
    for (int j = 0; j < 7; j++) t.sP[r * 7 + j] = t.P[r * 7 + j];
  }
  if (r == 0) {
    t.det_ind = -1;
    t.htail++;
    if (t.htail >= g.max_obs) t.hvalid = 0;  // the box left the deque(maxlen=max_obs)
    if (observed) t.has_saved = 1;
    t.observed = 0;
  }
}

#include "bx_jv.h"

struct OcsLds {
  double* dd;     // [D][6] detections of the frame (float32 values as f64)
  double* cost;   // [cost_lds]
  int *hi, *lo;   // [D] detection indices of the two confidence splits
  int *lst, *lst2;          // [T] slots in list order
  int *mi, *mm;             // [2N] candidate / validated (det, trk) pairs
  int *ud, *ut;             // [D+T] unmatched lists
  int *rowcnt, *colcnt, *rowcol;  // [N] each
  int *fl;                  // [N] flags
  int* sc;                  // [16] broadcast scalars
  double* sd;               // [4]
  JvLds jv;
};

__device__ void carve(const OcsDev& g, char* base, OcsLds& L) {
  size_t o = 0;
  auto takeD = [&](size_t n) { double* p = (double*)(base + o); o += n * 8; return p; };
  auto takeI = [&](size_t n) { int* p = (int*)(base + o); o += ((n * 4 + 7) / 8) * 8; return p; };
  const int N = g.N, D = g.D, T = g.T;
  L.dd = takeD((size_t)D * 6);
  L.cost = takeD(g.cost_lds);
  L.jv.v = takeD(N);
  L.jv.d = takeD(N);
  L.sd = takeD(4);
  L.jv.sd = takeD(2);
  L.hi = takeI(D);
  L.lo = takeI(D);
  L.lst = takeI(T);
  L.lst2 = takeI(T);
  L.mi = takeI(2 * N);
  L.mm = takeI(2 * N);
  L.ud = takeI(D + T);
  L.ut = takeI(D + T);
  L.rowcnt = takeI(N);
  L.colcnt = takeI(N);
  L.rowcol = takeI(N);
  L.fl = takeI(N);
  L.sc = takeI(16);
  L.jv.x = takeI(N);
  L.jv.y = takeI(N);
  L.jv.matches = takeI(N);
  L.jv.freer = takeI(N);
  L.jv.pred = takeI(N);
  L.jv.col = takeI(N);
  L.jv.sc = takeI(8);
}

size_t lds_bytes(int D, int T, int N, int cost_lds) {
  auto dI = [](size_t n) { return ((n * 4 + 7) / 8) * 8; };
  return (size_t)D * 6 * 8 + (size_t)cost_lds * 8 + 2 * (size_t)N * 8 + 6 * 8 + 2 * dI(D) +
         2 * dI(T) + 2 * dI(2 * N) + 2 * dI(D + T) + 4 * dI(N) + dI(16) + 6 * dI(N) + dI(8);
}

// lapjv(-cost, extend_cost=True): the shortest-augmenting-path solve + uniqueness test first,
// lapjv itself for a tied optimum (legacy_lap_ssp; the IoU-only BYTE / OCR rounds tie more often:
// non-overlapping pairs cost exactly 0, like lapjv's padding).  BX_OCS_SSP=0: lapjv always.
#ifndef BX_OCS_SSP
#define BX_OCS_SSP 1
#endif
__device__ __forceinline__ int ocs_lap(const double* C, int nr, int nc, JvLds& jv, int* out) {
#if BX_OCS_SSP
  bool jv_ran;
  return legacy_lap_ssp(C, nr, nc, jv, out, SyncBlock{}, jv_ran);
#else
  return legacy_lap(C, nr, nc, jv, out);
#endif
}

// ------------------------------------------------------------------------------------------
// The frame phases.  `F` is what a workgroup knows of its sequence; `L` the LDS carve.  Counts
// (nh, nt, nud, nut, ...) are wave-uniform and travel by value.  A phase that ends on a
// __syncthreads() says so; the callers rely on it.
struct OcsFrame {
  int b, r0, n;         // workgroup, its first detection row, detections (at most g.D)
  int frame, id0, nt0;  // this frame's number, the next id, tracks on the list
  int* sq;              // [SQO]
  int* order;           // [T]
  double* tb;           // [T][TBS]
  double* cost;         // [D*T] or null
  double thr, fw, fh;   // asso_threshold, frame size
  int ak;               // asso_kind
};

struct OcsSplit {
  int nm, nud, nut;  // validated pairs in L.mm, unmatched detections in L.ud, tracks in L.ut
};
struct OcsRematch {
  int nud, nut, ran;  // the unmatched that remain; ran: the round got past its gate
};

// the `n` items of a list, W lanes per item (every lane of the group calls fn(item))
template <int W, class Fn>
__device__ __forceinline__ void ocs_each(int n, Fn fn) {
  const int grp = threadIdx.x / W;
  for (int c = 0; c < n; c += OW / W) {
    const int q = c + grp;
    if (q < n) fn(q);
  }
}

__device__ __forceinline__ double* ocs_cost_buf(const OcsDev& g, const OcsLds& L,
                                                const OcsFrame& F, int nr, int nc) {
  return (nr * nc <= g.cost_lds) ? L.cost : F.cost;
}

// Frame preamble: the detections (setup_decorator's float32 rounding is the input format) as
// f64 into L.dd, the list order into L.lst2.  The caller syncs before reading either.
template <int TBS>
__device__ __forceinline__ OcsFrame ocs_frame_begin(const OcsDev& g, OcsLds& L, int seq,
                                                    const float* __restrict__ dets,
                                                    const int* __restrict__ det_off) {
  const int lane = threadIdx.x;
  OcsFrame F;
  F.b = blockIdx.x;
  F.r0 = det_off[F.b];
  F.n = det_off[F.b + 1] - F.r0;
  if (F.n > g.D) {  // the host checks det_cap; a device-side overflow is latched, never run past
    if (threadIdx.x == 0) atomicExch(g.status, (int)BX_ERR_CAPACITY);
    F.n = g.D;
  }
  F.sq = g.seqst + (size_t)seq * SQO;
  F.order = g.order + (size_t)seq * g.T;
  F.tb = g.tb + (size_t)seq * g.T * TBS;
  F.cost = g.cost_g ? g.cost_g + (size_t)seq * g.D * g.T : nullptr;
  F.frame = F.sq[SO_FRAME] + 1;
  F.id0 = F.sq[SO_IDS];
  F.nt0 = F.sq[SO_NTR];
  F.thr = g.asso_threshold;
  F.ak = g.asso_kind;
  F.fw = g.fsz[2 * seq];
  F.fh = g.fsz[2 * seq + 1];
  for (int q = lane; q < F.n * 6; q += OW) L.dd[q] = (double)dets[(size_t)F.r0 * 6 + q];
  for (int p = lane; p < F.nt0; p += OW) L.lst2[p] = F.order[p];
  return F;
}

// Predict every track (an octet per track); tracks whose prediction has a NaN leave the list
// (ocsort.py:278-288).  tb row per kept track: box[4], k-previous obs[5], last_obs[5], vel[2];
// pp (when given) gets the kept track's pre-frame list position.  Returns the tracks kept, their
// slots in L.lst; ends on a sync.
__device__ __forceinline__ int ocs_predict_octet(const OcsDev& g, OcsLds& L, const OcsFrame& F,
                                                 OcsTrk* trk, int* pp) {
  const int lane = threadIdx.x;
  const int oct = lane >> 3, r8 = lane & 7, rr8 = r8 < 7 ? r8 : 6;
  int nt = 0;
  for (int c = 0; c < F.nt0; c += 8) {
    const int p = c + oct;
    bool keep = false;
    int slot = -1;
    double v0 = 0.0, v1 = 0.0;  // this lane's two tb entries: [r8] and [8 + r8]
    if (p < F.nt0) {
      slot = L.lst2[p];
      OcsTrk& t = trk[slot];
      KfRow k;
      row_load(t.x, t.P, rr8, k);
      if ((osh(k.x, 6) + osh(k.x, 2)) <= 0 && rr8 == 6) k.x *= 0.0;
      kfo_predict(g, rr8, k);
      row_store(t.x, t.P, r8, k);
      const int age = t.age + 1;
      if (r8 == 0) {
        t.age = age;
        if (t.tsu > 0) t.hit_streak = 0;
        t.tsu++;
      }
      double xs[4], bx[4];
#pragma unroll
      for (int q = 0; q < 4; q++) xs[q] = osh(k.x, q);
      x_to_bbox(xs, bx);
      keep = !(isnan(bx[0]) || isnan(bx[1]) || isnan(bx[2]) || isnan(bx[3]));
      // k_previous_obs (ocsort.py:17-28) with the post-predict age
      int qq = -1;
      const int last_age = t.last_age;
      if (last_age >= 0) {
        qq = obs_first(t, age - g.delta_t, g.delta_t);
        if (qq < 0) qq = last_age & (OBS_KEEP - 1);  // observations[max(keys)]
      }
      auto val = [&](int e) -> double {
        if (e < 4) return e == 0 ? bx[0] : e == 1 ? bx[1] : e == 2 ? bx[2] : bx[3];
        if (e < 9) return qq < 0 ? -1.0 : t.obs_box[qq][e - 4];
        if (e < 14) return t.last_obs[e - 9];
        return t.has_vel ? t.vel[e - 14] : 0.0;
      };
      v0 = val(r8);
      v1 = val(8 + r8);
    }
    const unsigned long long m = __ballot(keep && r8 == 0);
    if (keep) {
      const int q = nt + __popcll(m & ((1ull << (lane & ~7)) - 1ull));
      if (r8 == 0) {
        L.lst[q] = slot;
        if (pp) pp[q] = p;
      }
      double* row = F.tb + (size_t)q * TB;
      row[r8] = v0;
      row[8 + r8] = v1;
    }
    nt += __popcll(m);
  }
  __syncthreads();
  return nt;
}

// Pass 1 of the first association (lane per track, dets broadcast from LDS): per detection and
// per track, how many IoU > threshold; L.rowcol[d] the track of a detection's (last) hit.  A
// pair without overlap has IoU 0/U, never above a threshold >= 0, so only overlapping pairs
// divide.  Ends on a sync.
__device__ __forceinline__ void ocs_pass1_count(const OcsDev& g, OcsLds& L, const OcsFrame& F,
                                                int nh, int nt) {
  const int lane = threadIdx.x;
  const double thr = F.thr;
  const int ak = F.ak;
  for (int k = lane; k < g.N; k += OW) L.rowcnt[k] = 0;
  __syncthreads();
  for (int c = 0; c < nt; c += OW) {
    const int ti = c + lane;
    if (ti < nt) {
      const double* bq = F.tb + (size_t)ti * TB;
      const double b0 = bq[0], b1 = bq[1], b2 = bq[2], b3 = bq[3];
      const double at = (b2 - b0) * (b3 - b1);
      int cc = 0;
      for (int d = 0; d < nh; d++) {
        const double* a = L.dd + 6 * L.hi[d];
        const double xx1 = fmax(a[0], b0), yy1 = fmax(a[1], b1);
        const double xx2 = fmin(a[2], b2), yy2 = fmin(a[3], b3);
        const double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
        const double wh = w * h;
        // the other registry modes score disjoint pairs too: no shortcut for them
        if (wh > 0.0 || thr < 0.0 || ak != ASSO_IOU) {
          const double o = ak == ASSO_IOU ? wh / ((a[2] - a[0]) * (a[3] - a[1]) + at - wh)
                                          : asso_pair(ak, a, bq, F.fw, F.fh);
          if (o > thr) {
            atomicAdd(&L.rowcnt[d], 1);
            L.rowcol[d] = ti;
            cc++;
          }
        }
      }
      L.colcnt[ti] = cc;
    }
  }
  __syncthreads();
}

// The one-to-one test on pass 1's counts: when every detection and every track has at most one
// hit, the candidate pairs are np.stack(np.where(iou > thr), 1), row-major, into L.mi; returns
// their number, or -1 when the full cost and the LAP have to decide.
__device__ __forceinline__ int ocs_one_to_one(OcsLds& L, int nh, int nt) {
  const int lane = threadIdx.x;
  int mr = 0, mcx = 0;
  for (int k = lane; k < nh; k += OW) mr = max(mr, L.rowcnt[k]);
  for (int k = lane; k < nt; k += OW) mcx = max(mcx, L.colcnt[k]);
  for (int o = 32; o >= 1; o >>= 1) {
    mr = max(mr, __shfl_xor(mr, o));
    mcx = max(mcx, __shfl_xor(mcx, o));
  }
  if (!(mr == 1 && mcx == 1)) return -1;
  return wave_compact(
      nh, [&](int d) { return L.rowcnt[d] == 1; },
      [&](int d, int p) {
        L.mi[2 * p] = d;
        L.mi[2 * p + 1] = L.rowcol[d];
      });
}

// Pass 2: C[d][ti] = -total(d, ti, IoU + direction consistency), the cost P4's legacy
// linear_assignment takes.  `total` is the identity for OCSort; DeepOCSort adds its appearance
// term there.  Ends on a sync.
template <class Total>
__device__ __forceinline__ void ocs_cost_fill(const OcsDev& g, OcsLds& L, const OcsFrame& F,
                                              double* C, int nh, int nt, Total total) {
  const int lane = threadIdx.x;
  for (int c = 0; c < nt; c += OW) {
    const int ti = c + lane;
    if (ti < nt) {
      const double* r = F.tb + (size_t)ti * TB;
      const double* p = r + 4;
      const double cx2 = (p[0] + p[2]) / 2.0, cy2 = (p[1] + p[3]) / 2.0;
      const double vy = r[14], vx = r[15];
      const double valid = p[4] < 0 ? 0.0 : 1.0;
      for (int d = 0; d < nh; d++) {
        const double* a = L.dd + 6 * L.hi[d];
        const double o = asso_pair(F.ak, a, r, F.fw, F.fh);
        // speed_direction_batch (association.py:10-20) against the k-previous obs
        const double cx1 = (a[0] + a[2]) / 2.0, cy1 = (a[1] + a[3]) / 2.0;
        double dx = cx1 - cx2, dy = cy1 - cy2;
        const double norm = sqrt(dx * dx + dy * dy) + 1e-6;
        dx = dx / norm;
        dy = dy / norm;
        double cth = vx * dx + vy * dy;
        cth = cth < -1 ? -1 : (cth > 1 ? 1 : cth);
        double ang = ocs_acos(cth);
        ang = (3.14159265358979323846 / 2.0 - fabs(ang)) / 3.14159265358979323846;
        const double mc = (valid * ang) * g.inertia;
        C[d * nt + ti] = -total(d, ti, o + mc);
      }
    }
  }
  __syncthreads();
}

// P3: unmatched = absent from the `nmi` candidate pairs of L.mi, ascending; then the validation
// accept(d, ti) of each pair, accepted pairs into L.mm in pair order, rejected pairs appended to
// the unmatched in pair order (P5).  Without tracks every detection is unmatched.  Ends on a
// sync, except without tracks (the caller's next sync covers L.ud).
template <class Accept>
__device__ __forceinline__ OcsSplit ocs_split(const OcsDev& g, OcsLds& L, int nh, int nt,
                                              int nmi, Accept accept) {
  const int lane = threadIdx.x;
  if (nt == 0) {
    for (int k = lane; k < nh; k += OW) L.ud[k] = k;
    return {0, nh, 0};
  }
  for (int k = lane; k < g.N; k += OW) L.rowcnt[k] = L.colcnt[k] = 0;
  __syncthreads();
  for (int q = lane; q < nmi; q += OW) {
    L.rowcnt[L.mi[2 * q]] = 1;
    L.colcnt[L.mi[2 * q + 1]] = 1;
  }
  __syncthreads();
  int nm = 0;
  int nud = wave_compact(nh, [&](int d) { return L.rowcnt[d] == 0; }, [&](int d, int p) { L.ud[p] = d; });
  int nut = wave_compact(nt, [&](int t) { return L.colcnt[t] == 0; }, [&](int t, int p) { L.ut[p] = t; });
  for (int c = 0; c < nmi; c += OW) {
    const int q = c + lane;
    bool ok = false, rej = false;
    int d = 0, ti = 0;
    if (q < nmi) {
      d = L.mi[2 * q];
      ti = L.mi[2 * q + 1];
      ok = accept(d, ti);
      rej = !ok;
    }
    const unsigned long long mo = __ballot(ok), mr = __ballot(rej);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (ok) {
      const int p = nm + __popcll(mo & below);
      L.mm[2 * p] = d;
      L.mm[2 * p + 1] = ti;
    }
    if (rej) {
      const int p = __popcll(mr & below);
      L.ud[nud + p] = d;
      L.ut[nut + p] = ti;
    }
    nm += __popcll(mo);
    nud += __popcll(mr);
    nut += __popcll(mr);
  }
  __syncthreads();
  return {nm, nud, nut};
}

// A rematch round (OCR on the last observations, ocsort.py:358-386; BYTE on the low-confidence
// detections, :330-356) of `nr` detections, L.dd rows dsel[dmap ? dmap[a] : a], against the
// `nut` unmatched tracks L.ut, their boxes at offset `boff` of the tb rows.
//
// The gate: the maximum of the association matrix.  In the plain IoU mode with a threshold >= 0
// only overlapping pairs divide.  A disjoint pair scores 0/U: 0, -0 or NaN, which fmax either
// ignores or cannot lift above a maximum that `mx > thr` would pass, and when every pair is
// disjoint both -inf and 0 fail `mx > thr >= 0`; so the gate is the one of the full matrix.
template <int TBS>
__device__ __forceinline__ double ocs_rematch_max(const OcsLds& L, const OcsFrame& F, int nr,
                                                  const int* dsel, const int* dmap, int nut,
                                                  int boff) {
  const int lane = threadIdx.x;
  const double thr = F.thr;
  const int ak = F.ak;
  double mx = -INF;
  for (int c = 0; c < nut; c += OW) {
    const int k = c + lane;
    if (k < nut) {
      const double* bq = F.tb + (size_t)L.ut[k] * TBS + boff;
      const double b0 = bq[0], b1 = bq[1], b2 = bq[2], b3 = bq[3];
      const double at = (b2 - b0) * (b3 - b1);
      for (int d = 0; d < nr; d++) {
        const double* a = L.dd + 6 * dsel[dmap ? dmap[d] : d];
        const double xx1 = fmax(a[0], b0), yy1 = fmax(a[1], b1);
        const double xx2 = fmin(a[2], b2), yy2 = fmin(a[3], b3);
        const double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
        const double wh = w * h;
        if (ak != ASSO_IOU)
          mx = fmax(mx, asso_pair(ak, a, bq, F.fw, F.fh));
        else if (wh > 0.0 || thr < 0.0)
          mx = fmax(mx, wh / ((a[2] - a[0]) * (a[3] - a[1]) + at - wh));
      }
    }
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  return mx;
}

// Past the gate: the full matrix -asso into C, its LAP, apply(a', ti) by the W lanes of a group
// for every pair the threshold keeps (a' indexes dsel, ti the track list), and the unmatched
// recompacted as np.setdiff1d does: ascending, unique.  With dmap null (BYTE) the detections
// are not listed again.  Ends on a sync.
template <int TBS, int W, class Apply>
__device__ __forceinline__ OcsRematch ocs_rematch_solve(const OcsDev& g, OcsLds& L,
                                                        const OcsFrame& F, int nh, int nt, int nr,
                                                        const int* dsel, const int* dmap, int nut,
                                                        int boff, Apply apply) {
  const int lane = threadIdx.x;
  double* C = ocs_cost_buf(g, L, F, nr, nut);
  for (int c = 0; c < nut; c += OW) {
    const int k = c + lane;
    if (k < nut) {
      const double* bq = F.tb + (size_t)L.ut[k] * TBS + boff;
      for (int d = 0; d < nr; d++)
        C[d * nut + k] = -asso_pair(F.ak, L.dd + 6 * dsel[dmap ? dmap[d] : d], bq, F.fw, F.fh);
    }
  }
  __syncthreads();
  const int np_ = ocs_lap(C, nr, nut, L.jv, L.mi);
  for (int k = lane; k < g.N; k += OW) {
    if (dmap) L.rowcnt[k] = 0;
    L.fl[k] = 0;
  }
  __syncthreads();
  ocs_each<W>(np_, [&](int q) {
    const int a = L.mi[2 * q], k = L.mi[2 * q + 1];
    if (!(-C[a * nut + k] < F.thr)) {
      const int di = dmap ? dmap[a] : a, ti = L.ut[k];
      apply(di, ti);
      if (lane % W == 0) {
        if (dmap) L.rowcnt[di] = 2;
        L.fl[ti] = 2;  // removed
      }
    }
  });
  __syncthreads();
  if (dmap)
    for (int k = lane; k < nr; k += OW)
      if (L.rowcnt[dmap[k]] == 0) L.rowcnt[dmap[k]] = 1;
  for (int k = lane; k < nut; k += OW)
    if (L.fl[L.ut[k]] == 0) L.fl[L.ut[k]] = 1;
  __syncthreads();
  OcsRematch u = {nr, nut, 1};
  if (dmap)
    u.nud = wave_compact(nh, [&](int d) { return L.rowcnt[d] == 1; }, [&](int d, int p) { L.ud[p] = d; });
  u.nut = wave_compact(nt, [&](int t) { return L.fl[t] == 1; }, [&](int t, int p) { L.ut[p] = t; });
  return u;
}

template <int TBS, int W, class Apply>
__device__ __forceinline__ OcsRematch ocs_rematch(const OcsDev& g, OcsLds& L, const OcsFrame& F,
                                                  int nh, int nt, int nr, const int* dsel,
                                                  const int* dmap, int nut, int boff,
                                                  Apply apply) {
  if (nr > 0 && nut > 0 && ocs_rematch_max<TBS>(L, F, nr, dsel, dmap, nut, boff) > F.thr)
    return ocs_rematch_solve<TBS, W>(g, L, F, nh, nt, nr, dsel, dmap, nut, boff, apply);
  return {nr, nut, 0};
}

// Births: the free slots ascending into L.lst2, and how many of the `nud` unmatched detections
// get one (all, or BX_ERR_TRACK_OVERFLOW is latched).
__device__ __forceinline__ int ocs_free_slots(const OcsDev& g, OcsLds& L, int nt, int nud) {
  const int lane = threadIdx.x;
  for (int s2 = lane; s2 < g.T; s2 += OW) L.fl[s2] = 0;
  __syncthreads();
  for (int p = lane; p < nt; p += OW) L.fl[L.lst[p]] = 1;
  __syncthreads();
  const int nfree = wave_compact(g.T, [&](int s2) { return L.fl[s2] == 0; }, [&](int s2, int p) { L.lst2[p] = s2; });
  if (nud > nfree) {
    if (lane == 0) atomicExch(g.status, (int)BX_ERR_TRACK_OVERFLOW);
    return nfree;
  }
  return nud;
}

// the bookkeeping of a newborn every record shares (one lane)
template <class Trk>
__device__ __forceinline__ void ocs_born_common(Trk& t, int id, double conf) {
  t.observed = 0;
  t.has_saved = 0;
  t.hvalid = 0;
  t.htail = 0;
  t.id = id;
  t.conf = conf;
  for (int q = 0; q < 5; q++) t.last_obs[q] = -1.0;
  t.last_age = -1;
  for (int q = 0; q < OBS_KEEP; q++) t.obs_age[q] = -1;
  t.has_vel = 0;
  t.tsu = t.hits = t.hit_streak = t.age = 0;
}

// KalmanBoxTracker(det) of OCSort and DeepOCSort (ocsort.py:83-134), octet-wide: x = [z, 0 0 0],
// P = diag(10 x4, 10000 x3); lane 0 the bookkeeping
__device__ __forceinline__ void ocs_born_octet(OcsTrk& t, int r8, const double* r, int id,
                                               int det_ind) {
  const double w = r[2] - r[0], h = r[3] - r[1];
  const double z[4] = {r[0] + w / 2.0, r[1] + h / 2.0, w * h, w / (h + 1e-6)};
  if (r8 < 7) {
    t.x[r8] = r8 == 0 ? z[0] : r8 == 1 ? z[1] : r8 == 2 ? z[2] : r8 == 3 ? z[3] : 0.0;
    const double pd = r8 < 4 ? 10.0 : 10000.0;
#pragma unroll
    for (int j = 0; j < 7; j++) t.P[r8 * 7 + j] = j == r8 ? pd : 0.0;
  }
  if (r8 == 0) {
    ocs_born_common(t, id, r[4]);
    t.cls = r[5];
    t.det_ind = det_ind;
    t.vel[0] = t.vel[1] = 0.0;
  }
}

// Outputs in reversed list order (ocsort.py:414-436: [box, id + id_bias, conf, cls, det_ind],
// the box the last observation or, without one, to_box of the state), then the deletion of the
// dead into `order`, then the sequence's counter row.  `ntr` tracks are on L.lst, `nnew` of them
// newborn.
template <class Trk, class ToBox>
__device__ __forceinline__ void ocs_frame_end(const OcsDev& g, OcsLds& L, const OcsFrame& F,
                                              Trk* trk, double* __restrict__ out,
                                              int* __restrict__ out_count, int ntr, int nnew,
                                              int id_bias, ToBox to_box) {
  double* orow = out + (size_t)F.r0 * 8;
  const int nout = wave_compact(
      ntr,
      [&](int k) {
        const Trk& t = trk[L.lst[ntr - 1 - k]];
        return t.tsu < 1 && (t.hit_streak >= g.min_hits || F.frame <= g.min_hits);
      },
      [&](int k, int p) {
        const Trk& t = trk[L.lst[ntr - 1 - k]];
        double d[4];
        if (sum5(t.last_obs) < 0) {
          to_box(t.x, d);
        } else {
          for (int q = 0; q < 4; q++) d[q] = t.last_obs[q];
        }
        if (p < F.n) {
          double* o = orow + (size_t)p * 8;
          o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3];
          o[4] = (double)(t.id + id_bias);
          o[5] = t.conf;
          o[6] = t.cls;
          o[7] = (double)t.det_ind;
        }
      });
  const int nkeep = wave_compact(
      ntr, [&](int k) { return trk[L.lst[k]].tsu <= g.max_age; },
      [&](int k, int p) { F.order[p] = L.lst[k]; });
  if (threadIdx.x == 0) {
    out_count[F.b] = nout < F.n ? nout : F.n;
    F.sq[SO_FRAME] = F.frame;
    F.sq[SO_IDS] = F.id0 + nnew;
    F.sq[SO_NTR] = nkeep;
    F.sq[SO_NOUT] = nout;
  }
}
