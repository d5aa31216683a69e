// bx_ocs_device.h — the device code OCSort and DeepOCSort share: the track record, the XYSR
// Kalman filter on an octet of lanes (predict, update, the ORU replay), KalmanBoxTracker's
// update(det) / update(None), the observation ring, the LDS carve and the legacy lapx LAP.
// Included inside the including translation unit's anonymous namespace (after bx_device.h), like
// bx_jv.h; bx_ocsort.hip's frame kernel is built from exactly this text.

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
  // [S] per-sequence parameters, or null: none was ever set (OCSort only: DeepOCSort and
  // HybridSort leave it null).  A kernel reads it, never writes it.
  const OcsSeqPar* seqpar = nullptr;
};

// The kernel-entry override: sequence `seq`'s entry of the table, when it is set, replaces the
// eleven per-sequence fields in the kernel's own copy of `g` (and max_obs, which follows
// max_age); everything downstream reads them through `g` as before.  `seq` is wave-uniform, so
// these are scalar loads, once per workgroup.
__device__ __forceinline__ void ocs_seq_override(OcsDev& g, int seq) {
  if (!g.seqpar) return;
  const OcsSeqPar* p = g.seqpar + seq;
  if (!p->set) return;
  g.min_conf = p->min_conf;
  g.det_thresh = p->det_thresh;
  g.asso_threshold = p->asso_threshold;
  g.inertia = p->inertia;
  g.q_xy = p->q_xy;
  g.q_s = p->q_s;
  g.max_age = p->max_age;
  g.max_obs = p->max_age >= 50 ? p->max_age + 5 : 50;  // derived, as the engine's create does
  g.min_hits = p->min_hits;
  g.delta_t = p->delta_t;
  g.use_byte = p->use_byte;
  g.asso_kind = p->asso_kind;
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
__device__ __forceinline__ int obs_first(const OcsTrk& t, int want0, int cnt) {
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
