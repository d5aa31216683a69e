// bx_deepocsort.hip — the DeepOCSort per-frame update on MI355X.
//
// Reference: boxmot/trackers/deepocsort/deepocsort.py:265-498 (DeepOcSort.update), its
// KalmanBoxTracker (deepocsort.py:51-235: OCSort's, plus apply_affine_correction and the
// embedding moving average) over the XYSR Kalman filter with observation-centric re-update
// (motion/kalman_filters/aabb/xysr_kf.py:48-291, apply_affine_correction :111-135),
// enhanced_associate with the appearance term (utils/association.py:377-556),
// compute_aw_max_metric (:320-374) and the legacy lapx linear_assignment (:105-114), with the
// patches P1-P5 of SURVEY.md Appendix A as in bx_ocsort.hip.
//
// Per frame, three launches on the caller's stream:
//   deepoc_embcost_kernel  dets_embs @ trk_embs.T for every detection x pre-frame track of every
//                          sequence: the fp64 MFMA tile of bx_embtile.h (shared with BoostTrack)
//   deepoc_frame_kernel    one wave64 workgroup per sequence, the frame phases of
//                          bx_ocs_device.h plus its own: CMC affine correction, predict,
//                          first association (IoU + direction consistency + appearance), updates,
//                          OCR round, births, outputs, deaths; emits embedding records
//   deepoc_feature_kernel  wave per record: emb = a*emb + (1-a)*det, emb /= ||emb|| (wave-order
//                          norm, as boost_feature_kernel), or the newborn's copy of its row
// The library builds with -ffp-contract=off; every expression keeps numpy's operation order.
#include <float.h>
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/bxdeepocsort.h"
#include "bx_classes_glue.h"
#include "bx_device.h"
#include "bx_host.h"

using namespace bx;


namespace {

#include "bx_ocs_device.h"
#include "bx_ocs_host.h"
#include "bx_embtile.h"

// OCSort's device record (o.min_conf unused, o.use_byte 0) plus the appearance state.  Per
// sequence, seqst[SO_IDS] starts at 1 (KalmanBoxTracker.count = 1, deepocsort.py:305).
// One sequence's entry of DeepOCSort's per-sequence parameter table: OCSort's entry (min_conf and
// use_byte stay 0, as in the engine's own OcsDev) plus the appearance parameters.  o.set 0: the
// sequence runs on the engine's own parameters.
struct DocSeqPar {
  OcsSeqPar o;
  double w_emb, alpha_fixed, aw_param;
  int aw_off, pad_;
};

struct DocDev {
  OcsDev o;
  int F;               // embedding width (0 with embedding_off)
  int x_off;           // bytes of LDS the shared carve takes (DocLds follows)
  int emb_off, aw_off;
  double w_emb, alpha_fixed, aw_param;
  double* emb;         // [S][T][F] track embeddings by slot
  double* ec;          // [S][D][T] emb cost by (detection of the frame, pre-frame list position)
  double* em;          // [S][D*T] the masked emb cost of the first association, [nh][nt]
  int* rec;            // [S][D] per detection of the frame: the slot its embedding goes to, or -1
  double* rec_a;       // [S][D] EMA weight alpha, < 0: newborn copy
  // [S] per-sequence parameters (bx_deepoc_set_seq_params_host), or null: none was ever set.  The
  // frame kernel reads it, never writes it; no other kernel reads a per-sequence field
  // (alpha_fixed reaches deepoc_feature_kernel through rec_a).
  const DocSeqPar* seqpar = nullptr;
};

// The kernel-entry override (bx_ocs_device.h ocs_seq_apply) for DocDev: sequence `seq`'s entry,
// when there is a table and the entry is set, replaces the per-sequence fields of the kernel's own
// copy of `gd`.  Wave-uniform scalar loads, all before the first store.
__device__ __forceinline__ void doc_seq_override(DocDev& gd, int seq) {
  if (!gd.seqpar) return;
  const DocSeqPar* p = gd.seqpar + seq;
  if (!p->o.set) return;
  const double w_emb = p->w_emb, alpha_fixed = p->alpha_fixed, aw_param = p->aw_param;
  const int aw_off = p->aw_off;
  ocs_seq_apply(gd.o, &p->o);
  gd.w_emb = w_emb;
  gd.alpha_fixed = alpha_fixed;
  gd.aw_param = aw_param;
  gd.aw_off = aw_off;
}

// LDS past the shared carve: pre-frame list position of each kept track, AW weights and flags
struct DocLds {
  int* pp;      // [T]
  double* rw;   // [D]
  double* cw;   // [T]
  int *ra, *ca; // [D], [T]
};

__host__ __device__ inline size_t doc_i8(size_t n) { return ((n * 4 + 7) / 8) * 8; }
size_t doc_lds_extra(int D, int T) {
  return doc_i8(T) + (size_t)D * 8 + (size_t)T * 8 + doc_i8(D) + doc_i8(T);
}
__device__ void doc_carve(const OcsDev& g, char* base, DocLds& X) {
  size_t o = 0;
  X.pp = (int*)(base + o);
  o += doc_i8(g.T);
  X.rw = (double*)(base + o);
  o += (size_t)g.D * 8;
  X.cw = (double*)(base + o);
  o += (size_t)g.T * 8;
  X.ra = (int*)(base + o);
  o += doc_i8(g.D);
  X.ca = (int*)(base + o);
}

// m @ p + t of the two corner points of a box (deepocsort.py:196-198)
__device__ __forceinline__ void warp_box(const double* w, double* b) {
  const double x1 = (w[0] * b[0] + w[1] * b[1]) + w[2], y1 = (w[3] * b[0] + w[4] * b[1]) + w[5];
  const double x2 = (w[0] * b[2] + w[1] * b[3]) + w[2], y2 = (w[3] * b[2] + w[4] * b[3]) + w[5];
  b[0] = x1;
  b[1] = y1;
  b[2] = x2;
  b[3] = y2;
}

// P[i0:i0+2, i0:i0+2] = m @ P[..] @ m.T, left to right (xysr_kf.py:122-123)
__device__ __forceinline__ void warp_cov(const double* w, double* P, int i0) {
  const double p00 = P[i0 * 7 + i0], p01 = P[i0 * 7 + i0 + 1];
  const double p10 = P[(i0 + 1) * 7 + i0], p11 = P[(i0 + 1) * 7 + i0 + 1];
  const double a00 = w[0] * p00 + w[1] * p10, a01 = w[0] * p01 + w[1] * p11;
  const double a10 = w[3] * p00 + w[4] * p10, a11 = w[3] * p01 + w[4] * p11;
  P[i0 * 7 + i0] = a00 * w[0] + a01 * w[1];
  P[i0 * 7 + i0 + 1] = a00 * w[3] + a01 * w[4];
  P[(i0 + 1) * 7 + i0] = a10 * w[0] + a11 * w[1];
  P[(i0 + 1) * 7 + i0 + 1] = a10 * w[3] + a11 * w[4];
}

// KalmanFilterXYSR.apply_affine_correction on one (x, P) (xysr_kf.py:119-123)
__device__ __forceinline__ void warp_state(const double* w, double* x, double* P) {
  const double x0 = (w[0] * x[0] + w[1] * x[1]) + w[2], x1 = (w[3] * x[0] + w[4] * x[1]) + w[5];
  const double v0 = w[0] * x[4] + w[1] * x[5], v1 = w[3] * x[4] + w[4] * x[5];
  x[0] = x0;
  x[1] = x1;
  x[4] = v0;
  x[5] = v1;
  warp_cov(w, P, 0);
  warp_cov(w, P, 4);
}

// KalmanBoxTracker.apply_affine_correction (deepocsort.py:191-208) of one track, by one lane.
// last_observation and observations[its age] are ONE array in the reference (update stores the
// same `bbox` object in both), so a write through either name shows through the other: the
// newest observation is warped once as last_observation (only if its sum is > 0) and once more
// when the loop over ages age-delta_t..age reaches its key.  Here the two are separate copies,
// kept equal.
__device__ void doc_affine(const OcsDev& g, OcsTrk& t, const double* w) {
  double lo[4] = {t.last_obs[0], t.last_obs[1], t.last_obs[2], t.last_obs[3]};
  if (sum5(t.last_obs) > 0) warp_box(w, lo);
  for (int dt = g.delta_t; dt >= 0; dt--) {
    const int want = t.age - dt;
    if (want < 0 || t.obs_age[want & (OBS_KEEP - 1)] != want) continue;
    if (want == t.last_age)
      warp_box(w, lo);
    else
      warp_box(w, t.obs_box[want & (OBS_KEEP - 1)]);
  }
  if (t.last_age >= 0) {
    for (int q = 0; q < 4; q++) t.last_obs[q] = t.obs_box[t.last_age & (OBS_KEEP - 1)][q] = lo[q];
  }
  warp_state(w, t.x, t.P);
  // the frozen snapshot (attr_saved) of a track that is not observed; its last_measurement is
  // warped too in the reference but never read again
  if (!t.observed && t.has_saved) warp_state(w, t.sx, t.sP);
}

__global__ void __launch_bounds__(256)
    deepoc_embcost_kernel(DocDev g, int seq0, const int* __restrict__ det_off,
                          const double* __restrict__ embs) {
  __shared__ double lds[2 * EC_STAGE];
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
  const double* temb = g.emb + (size_t)seq * T * F;
  const int tid = threadIdx.x;
  const int ar = ec_arow(tid), br = ec_brow(tid);
  const bool a_ok = d0 + ar < nd, b_ok = t0 + br < nt;
  const double* ap = embs + (size_t)(r0 + (a_ok ? d0 + ar : 0)) * F + ec_ak(tid);
  const double* bp = temb + (size_t)(b_ok ? order[t0 + br] : 0) * F + ec_bk(tid);
  d4 acc[2];
  ec_tile(lds, F, a_ok, ap, b_ok, bp, acc);
  ec_tile_store(acc, d0, t0, nd, nt, g.ec + (size_t)seq * g.o.D * T, T);
}

// the op: the same tile on plain arrays, grid (1, tiles of nd x nt)
__global__ void __launch_bounds__(256)
    deepoc_embcost_op_kernel(int nd, int nt, int F, const double* __restrict__ A,
                             const double* __restrict__ B, double* __restrict__ out) {
  __shared__ double lds[2 * EC_STAGE];
  const int d0 = (int)blockIdx.x / ec_tiles_t(nt) * EC_BM;
  const int t0 = (int)blockIdx.x % ec_tiles_t(nt) * EC_BN;
  if (d0 >= nd || t0 >= nt) return;
  const int tid = threadIdx.x;
  const int ar = ec_arow(tid), br = ec_brow(tid);
  const bool a_ok = d0 + ar < nd, b_ok = t0 + br < nt;
  const double* ap = A + (size_t)(a_ok ? d0 + ar : 0) * F + ec_ak(tid);
  const double* bp = B + (size_t)(b_ok ? t0 + br : 0) * F + ec_bk(tid);
  d4 acc[2];
  ec_tile(lds, F, a_ok, ap, b_ok, bp, acc);
  ec_tile_store(acc, d0, t0, nd, nt, out, nt);
}

// (two waves per SIMD, as OCSort's kernel gets unasked: with every phase inlined the allocator
// would otherwise take a few registers past 256 and halve the occupancy)
__global__ void __launch_bounds__(OW) __attribute__((amdgpu_waves_per_eu(2)))
    deepoc_frame_kernel(DocDev gd, int seq0, const float* __restrict__ dets,
                        const int* __restrict__ det_off, const double* __restrict__ warps,
                        double* __restrict__ out, int* __restrict__ out_count) {
  extern __shared__ __align__(16) char lds_raw[];
  const int seq = seq0 + blockIdx.x;
  doc_seq_override(gd, seq);  // this sequence's own parameters, when the table holds some
  const OcsDev& g = gd.o;
  OcsLds L;
  DocLds X;
  carve(g, lds_raw, L);
  doc_carve(g, lds_raw + gd.x_off, X);
  const int lane = threadIdx.x;
  L.jv.dc = nullptr;
  const OcsFrame F = ocs_frame_begin<TB>(g, L, seq, dets, det_off);  // deepocsort.py:339
  OcsTrk* trk = g.trk + (size_t)seq * g.T;
  const bool use_emb = !gd.emb_off;
  const double* ec = use_emb ? gd.ec + (size_t)seq * g.D * g.T : nullptr;
  double* em = use_emb ? gd.em + (size_t)seq * g.D * g.T : nullptr;
  int* rec = gd.rec + (size_t)seq * g.D;
  double* rec_a = gd.rec_a + (size_t)seq * g.D;
  if (use_emb)
    for (int i = lane; i < F.n; i += OW) rec[i] = -1;
  __syncthreads();
  const int nh = wave_compact(
      F.n, [&](int i) { return L.dd[6 * i + 4] > g.det_thresh; }, [&](int i, int p) { L.hi[p] = i; });

  // embedding record of detection row i (deepocsort.py:357-360, :415, :446): the track slot and
  // alpha = af + (1 - af) * (1 - trust), trust = (conf - det_thresh) / (1 - det_thresh)
  auto emit = [&](int i, int slot, bool born) {
    if (!use_emb) return;
    const double trust = (L.dd[6 * i + 4] - g.det_thresh) / (1 - g.det_thresh);
    const double af = gd.alpha_fixed;
    rec_a[i] = born ? -1.0 : af + (1 - af) * (1 - trust);
    rec[i] = slot;
  };
  const int r8 = lane & 7;
  // update(det) of list position ti with detection row i, octet-wide, and its embedding record
  auto update = [&](int i, int ti) {
    const int slot = L.lst[ti];
    const double* r = L.dd + 6 * i;
    ocs_update_det(g, trk[slot], r8, r, r[5], i);
    if (r8 == 0) emit(i, slot, false);
  };

  // ---- CMC affine correction of every track (deepocsort.py:352-355), a lane per track -------
  if (warps) {
    double w[6];
    for (int q = 0; q < 6; q++) w[q] = warps[(size_t)F.b * 6 + q];
    for (int p = lane; p < F.nt0; p += OW) doc_affine(g, trk[L.lst2[p]], w);
    __syncthreads();
  }

  // predict (deepocsort.py:367-382); X.pp = a kept track's pre-frame list position (the column
  // of ec)
  const int nt = ocs_predict_octet(g, L, F, trk, X.pp);

  // ---- first association: associate(dets over det_thresh, predicted tracks, emb cost) -------
  int nmi = 0;
  if (nt > 0 && nh > 0) {
    ocs_pass1_count(g, L, F, nh, nt);
    nmi = ocs_one_to_one(L, nh, nt);
    if (nmi < 0) {
      // the appearance term (association.py:464-473): emb = ec.copy(); emb[iou <= 0] = 0,
      // then the adaptive weights of its rows and columns, or the fixed weight
      if (use_emb) {
        for (int c = 0; c < nt; c += OW) {
          const int ti = c + lane;
          if (ti < nt) {
            const double* r = F.tb + (size_t)ti * TB;
            const int col = X.pp[ti];
            for (int d = 0; d < nh; d++) {
              const double o = asso_pair(F.ak, L.dd + 6 * L.hi[d], r, F.fw, F.fh);
              em[d * nt + ti] = o <= 0 ? 0.0 : ec[(size_t)L.hi[d] * g.T + col];
            }
          }
        }
        __syncthreads();
        if (!gd.aw_off) {
          for (int d = lane; d < nh; d += OW) {
            bool ap;
            X.rw[d] = aw_weight(em + (size_t)d * nt, nt, 1, gd.aw_param, &ap);
            X.ra[d] = ap;
          }
          for (int ti = lane; ti < nt; ti += OW) {
            bool ap;
            X.cw[ti] = aw_weight(em + ti, nh, nt, gd.aw_param, &ap);
            X.ca[ti] = ap;
          }
          __syncthreads();
        }
      }
      // the full cost -((IoU + direction consistency) + appearance) and P4's legacy
      // linear_assignment of it
      double* C = ocs_cost_buf(g, L, F, nh, nt);
      ocs_cost_fill(g, L, F, C, nh, nt, [&](int d, int ti, double s) {
        double total = s;
        if (use_emb) {
          const double e = em[d * nt + ti];
          if (gd.aw_off) {
            total += e * gd.w_emb;
          } else {  // compute_aw_max_metric: ((w * row) * col) * emb
            double w = gd.w_emb;
            if (X.ra[d]) w *= X.rw[d];
            if (X.ca[ti]) w *= X.cw[ti];
            total += w * e;
          }
        }
        return total;
      });
      nmi = ocs_lap(C, nh, nt, L.jv, L.mi);
    }
  }
  const OcsSplit sp = ocs_split(g, L, nh, nt, nmi, [&](int d, int ti) {
    return asso_pair(F.ak, L.dd + 6 * L.hi[d], F.tb + (size_t)ti * TB, F.fw, F.fh) >= F.thr;
  });
  ocs_each<8>(sp.nm, [&](int q) { update(L.hi[L.mm[2 * q]], L.mm[2 * q + 1]); });
  __syncthreads();

  // ---- OCR round on the last observations (deepocsort.py:420-456) ---------------------------
  const OcsRematch u = ocs_rematch<TB, 8>(g, L, F, nh, nt, sp.nud, L.hi, L.ud, sp.nut, 9,
                                          [&](int di, int ti) { update(L.hi[di], ti); });
  ocs_each<8>(u.nut, [&](int k) { ocs_update_none(g, trk[L.lst[L.ut[k]]], r8); });

  // ---- new tracks for the unmatched detections (free slots ascending) -----------------------
  const int nnew = ocs_free_slots(g, L, nt, u.nud);
  ocs_each<8>(nnew, [&](int k) {
    const int slot = L.lst2[k], i = L.hi[L.ud[k]];
    ocs_born_octet(trk[slot], r8, L.dd + 6 * i, F.id0 + k, i);
    if (r8 == 0) {
      L.lst[nt + k] = slot;
      emit(i, slot, true);  // emb = the detection's raw row (deepocsort.py:466)
    }
  });
  __syncthreads();

  // ---- outputs in reversed list order, then deletion of the dead (deepocsort.py:473-495); the
  // id without +1 (deepocsort.py:489): the counter starts at 1
  ocs_frame_end(g, L, F, trk, out, out_count, nt + nnew, nnew, 0,
                [](const double* x, double* d) { x_to_bbox(x, d); });
}

// update_emb (deepocsort.py:184-186) / the newborn's emb = its detection's row; wave per
// detection of the frame, 4 per workgroup.  The norm is summed in boost_feature_kernel's order:
// lane-strided partial sums, then a butterfly over the wave.
__global__ void __launch_bounds__(256)
    deepoc_feature_kernel(DocDev g, int seq0, const int* __restrict__ det_off,
                          const double* __restrict__ embs) {
  const int b = blockIdx.y, seq = seq0 + b;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r0 = det_off[b];
  int n = det_off[b + 1] - r0;
  if (n > g.o.D) n = g.o.D;
  if (k >= n) return;  // whole waves leave together
  const int slot = g.rec[(size_t)seq * g.o.D + k];
  if (slot < 0) return;
  const double alpha = g.rec_a[(size_t)seq * g.o.D + k];
  const int F = g.F;
  double* e = g.emb + ((size_t)seq * g.o.T + slot) * F;
  const double* x = embs + (size_t)(r0 + k) * F;
  if (alpha < 0.0) {
    for (int q = lane; q < F; q += 64) e[q] = x[q];
    return;
  }
  const double om = 1 - alpha;
  double s = 0.0;
  for (int q = lane; q < F; q += 64) {
    const double v = alpha * e[q] + om * x[q];
    e[q] = v;
    s += v * v;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  const double nrm = sqrt(s);
  for (int q = lane; q < F; q += 64) e[q] = e[q] / nrm;
}

__global__ void deepoc_reset_kernel(DocDev g, int seq0, int nseq) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nseq * SQO) g.o.seqst[(size_t)seq0 * SQO + k] = (k % SQO == SO_IDS) ? 1 : 0;
}

}  // namespace

struct bx_deepoc : OcsHost {
  DocDev dev;
  bx_deepoc_config cfg;
  void* arena = nullptr;
  size_t lds = 0;
  // per_class=True: the class state and the staging of the per-class warps
  ClsGlue pc;
  double* h_cwarp = nullptr;
  double* p_cwarp = nullptr;
  BxProbe probe;  // stages: 0 embcost, 1 frame, 2 feature
  // per-sequence parameters (bx_deepoc_set_seq_params_host): the device table dev.seqpar points
  // to, allocated by the first set, and its host mirror
  BxSeqTable<DocSeqPar> seqtab;
};

// the field checks bx_deepoc_create and bx_deepoc_set_seq_params_host share
static bool bad_delta_t(int delta_t) { return delta_t < 1 || delta_t > OBS_KEEP - 1; }
static bool bad_asso_kind(int k) { return k < ASSO_IOU || k > ASSO_CENTROID; }

static int launch(bx_deepoc* e, int seq0, int nseq, const float* dets, const int* off,
                  const double* embs, const double* warps, double* out, int* cnt, hipStream_t st) {
  const DocDev& d = e->dev;
  const bool emb = !d.emb_off;
  int rc;
  if (emb && !embs) return bx_record_error(BX_ERR_SHAPE, "DeepOCSort needs embeddings unless embedding_off");
  if (emb) {
    if ((rc = e->probe.begin(0, st))) return rc;
    hipLaunchKernelGGL(deepoc_embcost_kernel, dim3(nseq, ec_tiles(d.o.D, d.o.T)), dim3(256), 0, st,
                       d, seq0, off, embs);
    BX_HIPCHK(hipGetLastError());
    if ((rc = e->probe.end(0, st))) return rc;
  }
  if ((rc = e->probe.begin(1, st))) return rc;
  hipLaunchKernelGGL(deepoc_frame_kernel, dim3(nseq), dim3(OW), e->lds, st, d, seq0, dets, off,
                     warps, out, cnt);
  BX_HIPCHK(hipGetLastError());
  if ((rc = e->probe.end(1, st))) return rc;
  if (emb) {
    if ((rc = e->probe.begin(2, st))) return rc;
    hipLaunchKernelGGL(deepoc_feature_kernel, dim3((d.o.D + 3) / 4, nseq), dim3(256), 0, st, d,
                       seq0, off, embs);
    BX_HIPCHK(hipGetLastError());
    if ((rc = e->probe.end(2, st))) return rc;
  }
  return BX_OK;
}

extern "C" {

int bx_deepoc_create(const bx_deepoc_config* c, bx_deepoc** out) {
  if (!c || !out) return bx_record_error(BX_ERR_INVALID, "null argument");
  if (c->n_seq <= 0 || c->track_cap <= 0 || c->det_cap <= 0 || c->track_cap > 512 ||
      c->det_cap > 512)
    return bx_record_error(BX_ERR_INVALID, "n_seq/track_cap/det_cap out of range");
  if (bad_delta_t(c->delta_t))
    return bx_record_error(BX_ERR_INVALID, "delta_t must be in [1, 7]");
  if (!c->embedding_off && c->emb_dim <= 0)
    return bx_record_error(BX_ERR_INVALID, "emb_dim must be positive unless embedding_off");
  if (bad_asso_kind(c->asso_kind))
    return bx_record_error(BX_ERR_INVALID, "unknown asso_kind");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return bx_record_error(BX_ERR_NO_DEVICE, "no HIP device visible");
  bx_deepoc* e = new bx_deepoc();
  e->cfg = *c;
  e->o = &e->dev.o;
  // everything that can fail runs in `fill`: a failure frees what was allocated so far
  auto fill = [&]() -> int {
    DocDev& dd = e->dev;
    OcsDev& d = dd.o;
    d.S = c->n_seq;
    d.T = c->track_cap;
    d.D = c->det_cap;
    d.N = d.T > d.D ? d.T : d.D;
    d.min_conf = 0.0;
    d.det_thresh = c->det_thresh;
    d.asso_threshold = c->iou_threshold;
    d.inertia = c->inertia;
    d.q_xy = 1.0 * c->q_xy_scaling;
    d.q_s = 1.0 * c->q_s_scaling;
    d.max_age = c->max_age;
    d.min_hits = c->min_hits;
    d.delta_t = c->delta_t;
    d.use_byte = 0;
    d.asso_kind = c->asso_kind;
    // basetracker.py:59-62: max_obs = 50, or max_age + 5 when max_age >= 50
    d.max_obs = c->max_age >= 50 ? c->max_age + 5 : 50;
    dd.emb_off = c->embedding_off != 0;
    dd.aw_off = c->aw_off != 0;
    dd.F = dd.emb_off ? 0 : c->emb_dim;
    dd.w_emb = c->w_association_emb;
    dd.alpha_fixed = c->alpha_fixed_emb;
    dd.aw_param = c->aw_param;
    size_t x_off;
    int rc = ocs_lds_budget(d, doc_lds_extra(d.D, d.T), &x_off, &e->lds);
    if (rc) return rc;
    dd.x_off = (int)x_off;
    const bool need_g = (long)d.D * d.T > d.cost_lds;
    const size_t S = d.S, T = d.T, D = d.D, F = dd.F;
    BxCarve carve_b;
    const size_t o_trk = carve_b(S * T * sizeof(OcsTrk));
    const size_t o_sq = carve_b(S * SQO * sizeof(int));
    const size_t o_ord = carve_b(S * T * sizeof(int));
    const size_t o_tb = carve_b(S * T * TB * sizeof(double));
    const size_t o_cg = need_g ? carve_b(S * D * T * sizeof(double)) : 0;
    const size_t o_st = carve_b(sizeof(int) * 4);
    const size_t o_fsz = carve_b(S * 2 * sizeof(double));
    const size_t o_emb = carve_b(S * T * (F ? F : 1) * sizeof(double));
    const size_t o_ec = carve_b(F ? S * D * T * sizeof(double) : 8);
    const size_t o_em = carve_b(F ? S * D * T * sizeof(double) : 8);
    const size_t o_rec = carve_b(S * D * sizeof(int));
    const size_t o_ra = carve_b(S * D * sizeof(double));
    if (hipMalloc(&e->arena, carve_b.off) != hipSuccess)
      return bx_record_error(BX_ERR_HIP, "hipMalloc of the DeepOCSort arena failed");
    BX_HIPCHK(hipMemset(e->arena, 0, carve_b.off));
    char* base = (char*)e->arena;
    d.trk = (OcsTrk*)(base + o_trk);
    d.seqst = (int*)(base + o_sq);
    d.order = (int*)(base + o_ord);
    d.tb = (double*)(base + o_tb);
    d.cost_g = need_g ? (double*)(base + o_cg) : nullptr;
    d.status = (int*)(base + o_st);
    d.fsz = (double*)(base + o_fsz);
    d.dbg = nullptr;
    dd.emb = (double*)(base + o_emb);
    dd.ec = (double*)(base + o_ec);
    dd.em = (double*)(base + o_em);
    dd.rec = (int*)(base + o_rec);
    dd.rec_a = (double*)(base + o_ra);
    if ((rc = ocs_upload_initial(d, c->frame_w, c->frame_h, 1))) return rc;
    BX_HIPCHK(bx_lds_attr((const void*)deepoc_frame_kernel, e->lds));
    return e->sg.alloc(sizeof(float) * 6 * D, sizeof(double) * D * F, 6, 8, d.D, SQO);
  };
  const int rc = fill();
  if (rc) {
    bx_deepoc_destroy(e);
    return rc;
  }
  *out = e;
  return BX_OK;
}

int bx_deepoc_copy_state(bx_deepoc* dst, bx_deepoc* src) {
  if (!dst || !src) return bx_record_error(BX_ERR_INVALID, "null engine");
  const OcsDev &a = src->dev.o, &b = dst->dev.o;
  if (a.S != b.S || b.T < a.T || b.D < a.D || src->dev.F != dst->dev.F)
    return bx_record_error(BX_ERR_INVALID, "bx_deepoc_copy_state: destination must have the "
                                           "source's sequences and embedding width and at least "
                                           "its capacities");
  BX_HIPCHK(hipDeviceSynchronize());
  const size_t S = a.S, Ta = a.T, Tb = b.T, F = src->dev.F;
  BX_HIPCHK(hipMemcpy2D(b.trk, Tb * sizeof(OcsTrk), a.trk, Ta * sizeof(OcsTrk), Ta * sizeof(OcsTrk), S,
                   hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy2D(b.order, Tb * sizeof(int), a.order, Ta * sizeof(int), Ta * sizeof(int), S,
                   hipMemcpyDeviceToDevice));
  if (F)
    BX_HIPCHK(hipMemcpy2D(dst->dev.emb, Tb * F * sizeof(double), src->dev.emb, Ta * F * sizeof(double),
                     Ta * F * sizeof(double), S, hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.seqst, a.seqst, S * SQO * sizeof(int), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.fsz, a.fsz, S * 2 * sizeof(double), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.status, a.status, 4 * sizeof(int), hipMemcpyDeviceToDevice));
  dst->cache_seq = -1;
  BX_HIPCHK(hipDeviceSynchronize());
  return cls_glue_copy(dst->pc, src->pc, b.S, b.D, dst->dev.F, 1);
}

int bx_deepoc_destroy(bx_deepoc* e) {
  if (!e) return BX_OK;
  e->probe.destroy();
  (void)hipFree(e->arena);
  e->seqtab.free();
  e->sg.free();
  cls_glue_free(e->pc);
  (void)hipFree(e->h_cwarp);
  (void)hipHostFree(e->p_cwarp);
  delete e;
  return BX_OK;
}

int bx_deepoc_reset(bx_deepoc* e, int seq0, int nseq, void* stream) {
  if (!e || seq0 < 0 || nseq < 0 || seq0 + nseq > e->dev.o.S)
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  if (!nseq) return BX_OK;
  e->cache_seq = -1;
  hipLaunchKernelGGL(deepoc_reset_kernel, dim3((nseq * SQO + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, e->dev, seq0, nseq);
  BX_HIPCHK(hipGetLastError());
  return cls_glue_reset(e->pc, seq0, nseq, stream);
}

int bx_deepoc_step(bx_deepoc* e, int seq0, int nseq, const float* dets, const int32_t* det_off,
                   const double* embs, const double* warps, double* out, int32_t* out_count,
                   void* stream) {
  if (!e || seq0 < 0 || nseq <= 0 || seq0 + nseq > e->dev.o.S || !det_off || !out || !out_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_step");
  e->cache_seq = -1;
  return launch(e, seq0, nseq, dets, det_off, embs, warps, out, out_count, (hipStream_t)stream);
}

int bx_deepoc_update_host(bx_deepoc* e, int seq, const float* dets, int n, const double* embs,
                          const double* warp, double* out, int* n_out, void* stream) {
  if (!e || seq < 0 || seq >= e->dev.o.S || n < 0 || (n && (!dets || !out)) || !n_out)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_update_host");
  if (n > e->dev.o.D) return bx_record_error(BX_ERR_CAPACITY, "detections exceed det_cap");
  const size_t F = e->dev.F;
  if (n && F && !embs)
    return bx_record_error(BX_ERR_SHAPE, "DeepOCSort needs embeddings unless embedding_off");
  hipStream_t st = (hipStream_t)stream;
  BxStaging& sg = e->sg;
  int rc;
  if (n && F && (rc = sg.put(sg.h_embs, sg.p_embs, embs, sizeof(double) * F * n, st))) return rc;
  if (warp && (rc = sg.put(sg.h_warp, sg.p_warp, warp, sizeof(double) * 6, st))) return rc;
  return ocs_update_host_roundtrip(
      *e, seq, dets, n, out, n_out, st, true,
      [&] {
        return launch(e, seq, 1, (float*)sg.h_dets, sg.h_off, (double*)sg.h_embs,
                      warp ? sg.h_warp : nullptr, sg.h_out, sg.h_cnt, st);
      },
      OcsStreamSync{st});
}

// per_class=True (include/bxclasses.h): class c of sequence s is engine sequence s * C + c; the
// frame is split -> the three launches over the class sequences -> merge, all on `stream`.
int bx_deepoc_step_classes(bx_deepoc* e, int seq0, int nseq, int n_classes, const float* dets,
                           const int32_t* det_off, const double* embs, const double* warps,
                           double* out, int32_t* out_count, void* stream) {
  if (!e) return bx_record_error(BX_ERR_INVALID, "null engine");
  if (!e->dev.emb_off && !embs)
    return bx_record_error(BX_ERR_SHAPE, "DeepOCSort needs embeddings unless embedding_off");
  e->cache_seq = -1;
  hipStream_t st = (hipStream_t)stream;
  return cls_glue_step(e->pc, e->dev.o.S, e->dev.o.D, e->dev.F, 1, e->dev.o.seqst + SO_IDS, SQO,
                       seq0, nseq, n_classes, dets, det_off, embs, out, out_count, st,
                       [&](int q0, int nq, const float* d, const int* off, const double* em,
                           double* o, int* cnt) {
                         return launch(e, q0, nq, d, off, em, warps, o, cnt, st);
                       });
}

int bx_deepoc_classes_config(bx_deepoc* e, int n_classes, int map_cap) {
  if (!e || map_cap <= 0) return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_classes_config");
  if (e->pc.cls) return bx_record_error(BX_ERR_INVALID, "the engine's class state already exists");
  e->pc.map_cap = map_cap;
  return cls_glue_get(e->pc, e->dev.o.S, e->dev.o.D, e->dev.F, n_classes, 1);
}

int bx_deepoc_classes(bx_deepoc* e, bx_classes** out) {
  if (!e || !out) return bx_record_error(BX_ERR_INVALID, "null argument");
  *out = e->pc.cls;
  return BX_OK;
}

int bx_deepoc_update_classes_host(bx_deepoc* e, int seq, int n_classes, const float* dets, int n,
                                  const double* embs, const double* warps, int* id_count,
                                  double* out, int* n_out, void* stream) {
  if (!e || seq < 0 || n < 0 || (n && (!dets || !out)) || !n_out || !id_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_update_classes_host");
  if (n > e->dev.o.D) return bx_record_error(BX_ERR_CAPACITY, "detections exceed det_cap");
  const size_t F = e->dev.F;
  if (n && F && !embs)
    return bx_record_error(BX_ERR_SHAPE, "DeepOCSort needs embeddings unless embedding_off");
  int rc = cls_glue_get(e->pc, e->dev.o.S, e->dev.o.D, e->dev.F, n_classes, 1);
  if (rc) return rc;
  if ((seq + 1) * (long)n_classes > e->dev.o.S) return bx_record_error(BX_ERR_INVALID, "bad sequence");
  hipStream_t st = (hipStream_t)stream;
  BxStaging& sg = e->sg;
  if (n && F && (rc = sg.put(sg.h_embs, sg.p_embs, embs, sizeof(double) * F * n, st))) return rc;
  if (warps) {
    if (!e->h_cwarp) {
      BX_HIPCHK(hipMalloc(&e->h_cwarp, sizeof(double) * 6 * n_classes));
      BX_HIPCHK(hipHostMalloc(&e->p_cwarp, sizeof(double) * 6 * n_classes));
    }
    memcpy(e->p_cwarp, warps, sizeof(double) * 6 * n_classes);
    BX_HIPCHK(hipMemcpyAsync(e->h_cwarp, e->p_cwarp, sizeof(double) * 6 * n_classes,
                        hipMemcpyHostToDevice, st));
  }
  return ocs_update_host_roundtrip(
      *e, -1, dets, n, out, n_out, st, true,
      [&] {
        if (int r = cls_glue_put_ids(e->pc, seq, *id_count, st)) return r;
        return bx_deepoc_step_classes(e, seq, 1, n_classes, (float*)sg.h_dets, sg.h_off,
                                      F ? (double*)sg.h_embs : nullptr,
                                      warps ? e->h_cwarp : nullptr, sg.h_out, sg.h_cnt, st);
      },
      [&](int* cstatus) { return cls_glue_take_ids(e->pc, seq, id_count, cstatus, st); });
}

int bx_deepoc_status(bx_deepoc* e, int* status) {
  if (!e || !status) return bx_record_error(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipMemcpy(status, e->dev.o.status, sizeof(int), hipMemcpyDeviceToHost));
  return cls_glue_status(e->pc, status);
}

int bx_deepoc_counters_host(bx_deepoc* e, int seq, int* frame_count, int* id_count,
                            int* n_tracks) {
  return ocs_counters(e, seq, frame_count, id_count, n_tracks);
}

int bx_deepoc_set_id_count(bx_deepoc* e, int seq, int id_count, void* stream) {
  return ocs_set_id_count(e, seq, id_count, stream);
}

int bx_deepoc_set_frame_size(bx_deepoc* e, int seq, double w, double h, void* stream) {
  return ocs_set_frame_size(e, seq, w, h, stream);
}

int bx_deepoc_set_seq_params_host(bx_deepoc* e, int seq0, int nseq,
                                  const bx_deepoc_seq_params* params_host, void* stream) {
  if (!e || e->seqtab.bad_range(seq0, nseq, e->dev.o.S))
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  for (int k = 0; params_host && k < nseq; k++) {  // every entry first: a bad one changes nothing
    if (bad_delta_t(params_host[k].delta_t))
      return bx_record_error(BX_ERR_INVALID, "delta_t must be in [1, 7]");
    if (bad_asso_kind(params_host[k].asso_kind))
      return bx_record_error(BX_ERR_INVALID, "unknown asso_kind");
  }
  if (!nseq || (!params_host && !e->seqtab.allocated())) return BX_OK;  // (nothing to clear)
  std::vector<DocSeqPar> stage(nseq, DocSeqPar{});
  for (int k = 0; params_host && k < nseq; k++) {
    const bx_deepoc_seq_params& p = params_host[k];
    DocSeqPar& d = stage[k];
    d.o.min_conf = 0.0;
    d.o.det_thresh = p.det_thresh;
    d.o.asso_threshold = p.iou_threshold;
    d.o.inertia = p.inertia;
    d.o.q_xy = 1.0 * p.q_xy_scaling;
    d.o.q_s = 1.0 * p.q_s_scaling;
    d.o.max_age = p.max_age;
    d.o.min_hits = p.min_hits;
    d.o.delta_t = p.delta_t;
    d.o.use_byte = 0;
    d.o.asso_kind = p.asso_kind;
    d.o.set = 1;
    d.w_emb = p.w_association_emb;
    d.alpha_fixed = p.alpha_fixed_emb;
    d.aw_param = p.aw_param;
    d.aw_off = p.aw_off != 0;
  }
  if (int rc = e->seqtab.put(seq0, stage, e->dev.o.S, (hipStream_t)stream,
                             "allocation or copy of the DeepOCSort parameter table failed"))
    return rc;
  e->dev.seqpar = e->seqtab.dev;
  return BX_OK;
}

int bx_deepoc_seq_params_host(bx_deepoc* e, int seq, bx_deepoc_seq_params* out_host) {
  if (!e || seq < 0 || seq >= e->dev.o.S || !out_host)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_seq_params_host");
  const bx_deepoc_config& c = e->cfg;
  bx_deepoc_seq_params o = {c.det_thresh, c.iou_threshold, c.inertia, c.q_xy_scaling,
                            c.q_s_scaling, c.w_association_emb, c.alpha_fixed_emb, c.aw_param,
                            c.max_age, c.min_hits, c.delta_t, c.aw_off != 0, c.asso_kind};
  if (const DocSeqPar* d = e->seqtab.set_entry(seq))
    o = {d->o.det_thresh, d->o.asso_threshold, d->o.inertia, d->o.q_xy, d->o.q_s, d->w_emb,
         d->alpha_fixed, d->aw_param, d->o.max_age, d->o.min_hits, d->o.delta_t, d->aw_off,
         d->o.asso_kind};
  *out_host = o;
  return BX_OK;
}

int bx_deepoc_tracks_host(bx_deepoc* e, int seq, int cap, int32_t* ids, double* x, double* p,
                          double* emb, int* n) {
  if (!e || seq < 0 || seq >= e->dev.o.S || cap < 0 || !n)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_tracks_host");
  std::vector<int> ord;
  int rc = ocs_list_order(e->dev.o, seq, ord);
  if (rc) return rc;
  const int nt = (int)ord.size();
  const size_t F = e->dev.F, T = e->dev.o.T;
  for (int k = 0; k < nt && k < cap; k++) {
    OcsTrk t;
    BX_HIPCHK(hipMemcpy(&t, e->dev.o.trk + (size_t)seq * T + ord[k], sizeof(OcsTrk),
                   hipMemcpyDeviceToHost));
    if (ids) ids[k] = t.id;
    if (x) memcpy(x + 7 * k, t.x, sizeof(t.x));
    if (p) memcpy(p + 49 * k, t.P, sizeof(t.P));
    if (emb && F)
      BX_HIPCHK(hipMemcpy(emb + F * k, e->dev.emb + ((size_t)seq * T + ord[k]) * F, sizeof(double) * F,
                     hipMemcpyDeviceToHost));
  }
  *n = nt;
  return BX_OK;
}

int bx_deepoc_state_set_host(bx_deepoc* e, int seq, int n, const int32_t* ids, const double* x,
                             const double* p, const double* emb) {
  if (!e || seq < 0 || seq >= e->dev.o.S || n < 0 || (n && !ids))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_state_set_host");
  std::vector<int> ord;
  int rc = ocs_list_order(e->dev.o, seq, ord);
  if (rc) return rc;
  const size_t F = e->dev.F, T = e->dev.o.T;
  for (int j = 0; j < n; j++) {
    OcsTrk t;
    int slot;
    if ((rc = ocs_find_track(e->dev.o, e->dev.o.trk, seq, ord, ids[j], t, &slot))) return rc;
    if (x) memcpy(t.x, x + 7 * j, sizeof(t.x));
    if (p) memcpy(t.P, p + 49 * j, sizeof(t.P));
    BX_HIPCHK(hipMemcpy(e->dev.o.trk + (size_t)seq * T + slot, &t, sizeof(OcsTrk),
                   hipMemcpyHostToDevice));
    if (emb && F)
      BX_HIPCHK(hipMemcpy(e->dev.emb + ((size_t)seq * T + slot) * F, emb + F * j, sizeof(double) * F,
                     hipMemcpyHostToDevice));
  }
  return BX_OK;
}

int bx_deepoc_frame_stats_host(bx_deepoc* e, int seq0, int nseq, int64_t* sums) {
  return ocs_frame_stats(e, "bx_deepoc_frame_stats_host", seq0, nseq, sums);
}

int bx_deepoc_probe(bx_deepoc* e, int stage) {
  if (!e || stage < -1 || stage > 2) return bx_record_error(BX_ERR_INVALID, "bad probe stage");
  e->probe.set(stage);
  return BX_OK;
}

int bx_deepoc_probe_read(bx_deepoc* e, double* total_ms, int* count) {
  if (!e || !total_ms || !count) return bx_record_error(BX_ERR_INVALID, "null argument");
  return e->probe.read(total_ms, count);
}

int bx_deepoc_embcost(int nd, int nt, int F, const double* dets_embs, const double* trk_embs,
                      double* out, void* stream) {
  if (nd < 0 || nt < 0 || F <= 0 || ((nd && nt) && (!dets_embs || !trk_embs || !out)))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_deepoc_embcost");
  if (!nd || !nt) return BX_OK;
  hipLaunchKernelGGL(deepoc_embcost_op_kernel, dim3(ec_tiles(nd, nt)), dim3(256), 0,
                     (hipStream_t)stream, nd, nt, F, dets_embs, trk_embs, out);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

}  // extern "C"
