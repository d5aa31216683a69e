// bx_ocsort.hip — the OCSort per-frame update on MI355X: one wave64 workgroup per sequence.
//
// Reference: boxmot/trackers/ocsort/ocsort.py:195-439 (OcSort.update), its KalmanBoxTracker
// (ocsort.py:56-192) over the XYSR Kalman filter with observation-centric re-update
// (motion/kalman_filters/aabb/xysr_kf.py:48-291), enhanced_associate
// (utils/association.py:377-536) and the legacy lapx linear_assignment (association.py:105-114),
// with the minimal patches P1-P5 documented in oracle/bxo_ocsort.c and SURVEY.md Appendix A.
//
// Every floating-point expression restates oracle/bxo_ocsort.c operation-for-operation (the
// library builds with -ffp-contract=off; f64 division and sqrt are correctly rounded), so track
// states, ids and outputs are bitwise those of the oracle.  The Jonker-Volgenant solve below is
// lapx's dense lapjv (oracle/bxo_ops.c bxo_lapjv) with the same tie order: its column minima,
// reduction-transfer minima and shortest-path relaxations run lane-parallel, and the steps
// whose order decides ties (the column-reduction sweep, the minimum scan over the `col`
// permutation, the swaps it makes, the augmentation) run in the oracle's order.
//
// Track state stays in HBM ([S][T] OcsTrk slots; the per-sequence list `order` keeps the
// reference's list order).  history_obs is kept compactly: the ORU replay only ever reads the
// last non-None box and how many Nones follow it, and the frozen history it restores is
// immediately overwritten by the new observation, so the snapshot needs only (x, P).
#include <float.h>
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/bxocsort.h"
#include "bx_device.h"
#include "bx_host.h"

using namespace bx;

namespace {

#include "bx_ocs_device.h"
#include "bx_ocs_host.h"

__global__ void __launch_bounds__(OW)
    ocsort_frame_kernel(OcsDev g, int seq0, const float* __restrict__ dets,
                        const int* __restrict__ det_off, double* __restrict__ out,
                        int* __restrict__ out_count) {
  extern __shared__ __align__(16) char lds_raw[];
  OcsLds L;
  carve(g, lds_raw, L);
  const int seq = seq0 + blockIdx.x;
  ocs_seq_override(g, seq);  // this sequence's own parameters, when the table holds some
  L.jv.dc = g.dbg ? g.dbg + (size_t)seq * OCS_DBG + 24 : nullptr;
#ifdef BX_PHASE_TIMING
  unsigned long long t_last = __builtin_amdgcn_s_memtime();
#endif
  const OcsFrame F = ocs_frame_begin<TB>(g, L, seq, dets, det_off);
  OcsTrk* trk = g.trk + (size_t)seq * g.T;
  __syncthreads();
  // the splits: the BYTE round's low-confidence detections and the rest of the frame's
  const int nl = wave_compact(
      F.n, [&](int i) { const double c = L.dd[6 * i + 4]; return c > g.min_conf && c < g.det_thresh; },
      [&](int i, int p) { L.lo[p] = i; });
  const int nh = wave_compact(
      F.n, [&](int i) { return L.dd[6 * i + 4] > g.det_thresh; }, [&](int i, int p) { L.hi[p] = i; });
  const int r8 = threadIdx.x & 7;
  // update(det) of list position ti with detection row i, octet-wide
  auto update = [&](int i, int ti) {
    const double* r = L.dd + 6 * i;
    ocs_update_det(g, trk[L.lst[ti]], r8, r, r[5], i);
  };

  const int nt = ocs_predict_octet(g, L, F, trk, nullptr);
  OSTAMP(1);

  // ---- first association: enhanced_associate(high dets, predicted tracks) -----------------
  int nmi = 0;
  if (nt > 0 && nh > 0) {
    ocs_pass1_count(g, L, F, nh, nt);
    OSTAMP(2);
    nmi = ocs_one_to_one(L, nh, nt);
    if (nmi < 0) {
      double* C = ocs_cost_buf(g, L, F, nh, nt);
      ocs_cost_fill(g, L, F, C, nh, nt, [](int, int, double s) { return s; });
      nmi = ocs_lap(C, nh, nt, L.jv, L.mi);
      OCOUNT(0, 1);
      OCOUNT(1, nh > nt ? nh : nt);
    }
    OSTAMP(3);
  }
  const OcsSplit sp = ocs_split(g, L, nh, nt, nmi, [&](int d, int ti) {
    return asso_pair(F.ak, L.dd + 6 * L.hi[d], F.tb + (size_t)ti * TB, F.fw, F.fh) >= F.thr;
  });
  int nud = sp.nud, nut = sp.nut;
  ocs_each<8>(sp.nm, [&](int q) { update(L.hi[L.mm[2 * q]], L.mm[2 * q + 1]); });
  __syncthreads();
  OSTAMP(4);

  // ---- BYTE round on the low-confidence detections (ocsort.py:330-356) ---------------------
  if (g.use_byte) {
    const OcsRematch u = ocs_rematch<TB, 8>(g, L, F, nh, nt, nl, L.lo, nullptr, nut, 0,
                                            [&](int dl, int ti) { update(L.lo[dl], ti); });
    nut = u.nut;
    OCOUNT(2, u.ran);
  }
  OSTAMP(5);

  // ---- OCR round on the last observations (ocsort.py:358-386) -------------------------------
  if (nud > 0 && nut > 0) {
    const double mx = ocs_rematch_max<TB>(L, F, nud, L.hi, L.ud, nut, 9);
    OSTAMP(6);
    if (mx > F.thr) {
      OCOUNT(3, 1);
      OCOUNT(4, nud > nut ? nud : nut);
      const OcsRematch u = ocs_rematch_solve<TB, 8>(g, L, F, nh, nt, nud, L.hi, L.ud, nut, 9,
                                                    [&](int di, int ti) { update(L.hi[di], ti); });
      nud = u.nud;
      nut = u.nut;
    }
  }
  OSTAMP(7);
  ocs_each<8>(nut, [&](int k) { ocs_update_none(g, trk[L.lst[L.ut[k]]], r8); });

  // ---- new tracks for the unmatched high detections (free slots ascending) ----------------
  const int nnew = ocs_free_slots(g, L, nt, nud);
  ocs_each<8>(nnew, [&](int k) {
    const int slot = L.lst2[k], i = L.hi[L.ud[k]];
    ocs_born_octet(trk[slot], r8, L.dd + 6 * i, F.id0 + k, i);
    if (r8 == 0) L.lst[nt + k] = slot;
  });
  __syncthreads();
  OSTAMP(8);

  // ---- outputs in reversed list order, then deletion of the dead (ocsort.py:414-436) ---------
  ocs_frame_end(g, L, F, trk, out, out_count, nt + nnew, nnew, 1,
                [](const double* x, double* d) { x_to_bbox(x, d); });
  OSTAMP(9);
  OCOUNT(5, nt);
  OCOUNT(6, nh);
  OCOUNT(7, 1);
}

__global__ void ocsort_reset_kernel(OcsDev g, int seq0, int nseq) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nseq * SQO) g.seqst[(size_t)seq0 * SQO + k] = 0;
}

thread_local std::string g_ocs_err;

// Op-level XYSR filter (bx_kf_xysr_*): one octet per track running the frame kernel's octet code
// (kfo_predict / kfo_update), so the op and the tracker are bit-identical.  op 0 initiate
// (ocsort.py:83-111 from xyxy boxes), 1 predict (ocsort.py:177-180: the s + ds <= 0 clamp, then
// F/Q of the tracker), 2 update (xysr_kf.py:256-283 with R = diag(1, 1, 10, 10)).
__global__ __launch_bounds__(256) void kf_xysr_kernel(int op, int n, double* __restrict__ x,
                                                      double* __restrict__ P,
                                                      const double* __restrict__ arg, double q_xy,
                                                      double q_s) {
  const int gt = blockIdx.x * 256 + threadIdx.x;
  const int k = gt >> 3, r = gt & 7, rr = r < 7 ? r : 6;
  if (k >= n) return;  // whole octets leave together
  double* xk = x + 7 * (size_t)k;
  double* Pk = P + 49 * (size_t)k;
  if (op == 0) {
    const double* b = arg + 4 * (size_t)k;
    const double w = b[2] - b[0], h = b[3] - b[1];
    const double z[4] = {b[0] + w / 2.0, b[1] + h / 2.0, w * h, w / (h + 1e-6)};
    if (r < 7) {
      xk[r] = r < 4 ? z[r] : 0.0;
      for (int j = 0; j < 7; j++) Pk[7 * r + j] = j == r ? (r < 4 ? 10.0 : 10000.0) : 0.0;
    }
    return;
  }
  KfRow kr;
  row_load(xk, Pk, rr, kr);
  if (op == 1) {
    OcsDev g;
    g.q_xy = q_xy;
    g.q_s = q_s;
    if (rr == 6 && xk[6] + xk[2] <= 0) kr.x *= 0.0;
    kfo_predict(g, rr, kr);
  } else {
    const double* zk = arg + 4 * (size_t)k;
    const double z[4] = {zk[0], zk[1], zk[2], zk[3]};
    kfo_update(rr, kr, z);
  }
  row_store(xk, Pk, r, kr);
}

}  // namespace

struct bx_ocsort : OcsHost {
  OcsDev dev;
  bx_ocsort_config cfg;
  void* arena = nullptr;
  size_t lds = 0;
  int device = 0;
  // per_class host path (bx_ocsort_update_classes_host): per sequence the local -> class-global
  // track id map and the local id counter the map covers; class offsets [C+1], counts [C]
  std::vector<std::vector<int>> gid;
  std::vector<int> lids;
  int* h_coff = nullptr;
  int* h_ccnt = nullptr;
  int ncls_alloc = 0;
  BxProbe probe;  // the frame kernel is stage 0
  // per-sequence parameters (bx_ocsort_set_seq_params_host): the device table dev.seqpar points
  // to, allocated by the first set, and its host mirror
  BxSeqTable<OcsSeqPar> seqtab;
};

// the field checks bx_ocsort_create and bx_ocsort_set_seq_params_host share
static bool bad_delta_t(int delta_t) { return delta_t < 1 || delta_t > OBS_KEEP - 1; }
static bool bad_asso_kind(int k) { return k < ASSO_IOU || k > ASSO_CENTROID; }

static int launch(bx_ocsort* e, int seq0, int nseq, const float* dets, const int* off,
                  double* out, int* cnt, hipStream_t st) {
  int rc;
  if ((rc = e->probe.begin(0, st))) return rc;
  hipLaunchKernelGGL(ocsort_frame_kernel, dim3(nseq), dim3(OW), e->lds, st, e->dev, seq0, dets,
                     off, out, cnt);
  BX_HIPCHK(hipGetLastError());
  return e->probe.end(0, st);
}

extern "C" {

int bx_ocsort_create(const bx_ocsort_config* c, bx_ocsort** out) {
  if (!c || !out) return bx_record_error(BX_ERR_INVALID, "null argument");
  if (c->n_seq <= 0 || c->track_cap <= 0 || c->det_cap <= 0 || c->track_cap > 512 ||
      c->det_cap > 512)
    return bx_record_error(BX_ERR_INVALID, "n_seq/track_cap/det_cap out of range");
  if (bad_delta_t(c->delta_t))
    return bx_record_error(BX_ERR_INVALID, "delta_t must be in [1, 7]");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return bx_record_error(BX_ERR_NO_DEVICE, "no HIP device visible");
  if (bad_asso_kind(c->asso_kind))
    return bx_record_error(BX_ERR_INVALID, "unknown asso_kind");
  bx_ocsort* e = new bx_ocsort();
  e->cfg = *c;
  e->o = &e->dev;
  // everything that can fail runs in `fill`: a failure frees what was allocated so far
  auto fill = [&]() -> int {
    BX_HIPCHK(hipGetDevice(&e->device));
    OcsDev& d = e->dev;
    d.S = c->n_seq;
    d.T = c->track_cap;
    d.D = c->det_cap;
    d.N = d.T > d.D ? d.T : d.D;
    d.min_conf = c->min_conf;
    d.det_thresh = c->det_thresh;
    d.asso_threshold = c->asso_threshold;
    d.inertia = c->inertia;
    d.q_xy = 1.0 * c->q_xy_scaling;
    d.q_s = 1.0 * c->q_s_scaling;
    d.max_age = c->max_age;
    d.min_hits = c->min_hits;
    d.delta_t = c->delta_t;
    d.use_byte = c->use_byte;
    d.asso_kind = c->asso_kind;
    // basetracker.py:59-62: max_obs = 50, or max_age + 5 when max_age >= 50
    d.max_obs = c->max_age >= 50 ? c->max_age + 5 : 50;
    size_t x_off;
    int rc = ocs_lds_budget(d, 0, &x_off, &e->lds);
    if (rc) return rc;
    const bool need_g = (long)d.D * d.T > d.cost_lds;
    const size_t S = d.S, T = d.T;
    BxCarve carve_b;
    const size_t o_trk = carve_b(S * T * sizeof(OcsTrk));
    const size_t o_sq = carve_b(S * SQO * sizeof(int));
    const size_t o_ord = carve_b(S * T * sizeof(int));
    const size_t o_tb = carve_b(S * T * TB * sizeof(double));
    const size_t o_cg = need_g ? carve_b(S * (size_t)d.D * T * sizeof(double)) : 0;
    const size_t o_st = carve_b(sizeof(int) * 4);
    const size_t o_fsz = carve_b(S * 2 * sizeof(double));
#ifdef BX_PHASE_TIMING
    const size_t o_dbg = carve_b(S * OCS_DBG * sizeof(unsigned long long));
#endif
    if (hipMalloc(&e->arena, carve_b.off) != hipSuccess)
      return bx_record_error(BX_ERR_HIP, "hipMalloc of the OCSort arena failed");
    BX_HIPCHK(hipMemset(e->arena, 0, carve_b.off));
    char* base = (char*)e->arena;
    d.trk = (OcsTrk*)(base + o_trk);
    d.seqst = (int*)(base + o_sq);
    d.order = (int*)(base + o_ord);
    d.tb = (double*)(base + o_tb);
    d.cost_g = need_g ? (double*)(base + o_cg) : nullptr;
    d.status = (int*)(base + o_st);
    d.fsz = (double*)(base + o_fsz);
#ifdef BX_PHASE_TIMING
    d.dbg = (unsigned long long*)(base + o_dbg);
#else
    d.dbg = nullptr;
#endif
    if ((rc = ocs_upload_initial(d, c->frame_w, c->frame_h, 0))) return rc;
    BX_HIPCHK(bx_lds_attr((const void*)ocsort_frame_kernel, e->lds));
    return e->sg.alloc(sizeof(float) * 6 * d.D, 0, 0, 8, d.D, SQO);
  };
  const int rc = fill();
  if (rc) {
    bx_ocsort_destroy(e);
    return rc;
  }
  *out = e;
  return BX_OK;
}

int bx_ocsort_copy_state(bx_ocsort* dst, bx_ocsort* src) {
  if (!dst || !src) return bx_record_error(BX_ERR_INVALID, "null engine");
  const OcsDev &a = src->dev, &b = dst->dev;
  if (a.S != b.S || b.T < a.T || b.D < a.D)
    return bx_record_error(BX_ERR_INVALID, "bx_ocsort_copy_state: destination must have the "
                                           "source's sequences and at least its capacities");
  BX_HIPCHK(hipDeviceSynchronize());
  const size_t S = a.S, Ta = a.T, Tb = b.T;
  // per-slot records [S][T] and the list order [S][T]; per-sequence scalars and frame sizes
  BX_HIPCHK(hipMemcpy2D(b.trk, Tb * sizeof(OcsTrk), a.trk, Ta * sizeof(OcsTrk), Ta * sizeof(OcsTrk), S,
                   hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy2D(b.order, Tb * sizeof(int), a.order, Ta * sizeof(int), Ta * sizeof(int), S,
                   hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.seqst, a.seqst, S * SQO * sizeof(int), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.fsz, a.fsz, S * 2 * sizeof(double), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.status, a.status, 4 * sizeof(int), hipMemcpyDeviceToDevice));
  dst->gid = src->gid;
  dst->lids = src->lids;
  dst->cache_seq = -1;
  BX_HIPCHK(hipDeviceSynchronize());
  return BX_OK;
}

int bx_ocsort_destroy(bx_ocsort* e) {
  if (!e) return BX_OK;
  e->probe.destroy();
  (void)hipFree(e->arena);
  e->seqtab.free();
  e->sg.free();
  (void)hipFree(e->h_coff);
  (void)hipFree(e->h_ccnt);
  delete e;
  return BX_OK;
}

int bx_ocsort_reset(bx_ocsort* e, int seq0, int nseq, void* stream) {
  if (!e || seq0 < 0 || nseq < 0 || seq0 + nseq > e->dev.S)
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  if (!nseq) return BX_OK;
  e->cache_seq = -1;
  hipLaunchKernelGGL(ocsort_reset_kernel, dim3((nseq * SQO + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, e->dev, seq0, nseq);
  BX_HIPCHK(hipGetLastError());
  for (int s = seq0; s < seq0 + nseq && !e->lids.empty(); s++) {
    e->lids[s] = 0;
    e->gid[s].clear();
  }
  return BX_OK;
}

int bx_ocsort_step(bx_ocsort* e, int seq0, int nseq, const float* dets, const int32_t* det_off,
                   double* out, int32_t* out_count, void* stream) {
  if (!e || seq0 < 0 || nseq <= 0 || seq0 + nseq > e->dev.S || !det_off || !out || !out_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_ocsort_step");
  e->cache_seq = -1;
  return launch(e, seq0, nseq, dets, det_off, out, out_count, (hipStream_t)stream);
}

int bx_ocsort_update_host(bx_ocsort* e, int seq, const float* dets, int n, double* out,
                          int* n_out, void* stream) {
  if (!e || seq < 0 || seq >= e->dev.S || n < 0 || (n && (!dets || !out)) || !n_out)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_ocsort_update_host");
  if (n > e->dev.D) return bx_record_error(BX_ERR_CAPACITY, "detections exceed det_cap");
  hipStream_t st = (hipStream_t)stream;
  return ocs_update_host_roundtrip(
      *e, seq, dets, n, out, n_out, st, false,
      [&] { return launch(e, seq, 1, (float*)e->sg.h_dets, e->sg.h_off, e->sg.h_out, e->sg.h_cnt, st); },
      OcsStreamSync{st});
}

// per_class=True (basetracker.py:155-201): OCSort keeps all of its state in active_tracks, so
// the decorator's per-class swap gives every class an isolated tracker — only the frame counter
// (equal for all: each class is called once per frame) and KalmanBoxTracker.count (class-global,
// ocsort.py:61,115-116) are shared.  Here class c is engine sequence seq0 + c and the whole frame
// is ONE launch over the n_classes sequences; ids are then renumbered into the reference's
// class-global order (births of class 0 first, then class 1, ...), continuing *id_count.
int bx_ocsort_update_classes_host(bx_ocsort* e, int seq0, int n_classes, const float* dets,
                                  int n, int* id_count, double* out, int* n_out, void* stream) {
  if (!e || n_classes <= 0 || seq0 < 0 || seq0 + n_classes > e->dev.S || n < 0 ||
      (n && !dets) || !n_out || !id_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_ocsort_update_classes_host");
  if (n > e->dev.D) return bx_record_error(BX_ERR_CAPACITY, "detections exceed det_cap");
  hipStream_t st = (hipStream_t)stream;
  const int C = n_classes;
  if (e->lids.empty()) {
    e->lids.assign(e->dev.S, 0);
    e->gid.assign(e->dev.S, {});
  }
  if (e->ncls_alloc < C) {
    (void)hipFree(e->h_coff);
    (void)hipFree(e->h_ccnt);
    BX_HIPCHK(hipMalloc(&e->h_coff, sizeof(int) * (C + 1)));
    BX_HIPCHK(hipMalloc(&e->h_ccnt, sizeof(int) * C));
    e->ncls_alloc = C;
  }
  auto cls_of = [&](int i) -> int {
    const float v = dets[6 * i + 5];
    return (v >= 0.f && v < (float)C && v == (float)(int)v) ? (int)v : -1;
  };
  std::vector<int> cnt(C + 1, 0);
  for (int i = 0; i < n; i++)
    if (cls_of(i) >= 0) cnt[cls_of(i) + 1]++;
  for (int c = 0; c < C; c++) cnt[c + 1] += cnt[c];
  const int m = cnt[C];
  std::vector<int> fill(cnt.begin(), cnt.end() - 1);
  std::vector<float> hd((size_t)6 * (m ? m : 1));
  for (int i = 0; i < n; i++) {
    const int c = cls_of(i);
    if (c >= 0) memcpy(&hd[6 * (size_t)fill[c]++], dets + 6 * (size_t)i, 6 * sizeof(float));
  }
  if (m) BX_HIPCHK(hipMemcpyAsync((float*)e->sg.h_dets, hd.data(), sizeof(float) * 6 * m, hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipMemcpyAsync(e->h_coff, cnt.data(), sizeof(int) * (C + 1), hipMemcpyHostToDevice, st));
  e->cache_seq = -1;
  int rc = launch(e, seq0, C, (float*)e->sg.h_dets, e->h_coff, e->sg.h_out, e->h_ccnt, st);
  if (rc) return rc;
  std::vector<int> oc(C), sq((size_t)C * SQO);
  std::vector<double> ho((size_t)8 * (m ? m : 1));
  BX_HIPCHK(hipMemcpyAsync(oc.data(), e->h_ccnt, sizeof(int) * C, hipMemcpyDeviceToHost, st));
  if (m) BX_HIPCHK(hipMemcpyAsync(ho.data(), e->sg.h_out, sizeof(double) * 8 * m, hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(sq.data(), e->dev.seqst + (size_t)seq0 * SQO, sizeof(int) * C * SQO,
                      hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  int status = 0;
  BX_HIPCHK(hipMemcpy(&status, e->dev.status, sizeof(int), hipMemcpyDeviceToHost));
  if (status)
    return bx_record_error(BX_ERR_TRACK_OVERFLOW, "a sequence ran out of track slots (raise track_cap)");
  int g = *id_count;
  for (int c = 0; c < C; c++) {  // births in class order take the next class-global ids
    std::vector<int>& map = e->gid[seq0 + c];
    for (int l = e->lids[seq0 + c]; l < sq[(size_t)c * SQO + SO_IDS]; l++) {
      if ((int)map.size() <= l) map.resize(l + 1, -1);
      map[l] = g++;
    }
    e->lids[seq0 + c] = sq[(size_t)c * SQO + SO_IDS];
  }
  *id_count = g;
  int k = 0;
  for (int c = 0; c < C; c++)
    for (int j = 0; j < oc[c]; j++, k++) {
      double* o = out + 8 * (size_t)k;
      memcpy(o, &ho[8 * ((size_t)cnt[c] + j)], 8 * sizeof(double));
      o[4] = (double)(e->gid[seq0 + c][(int)o[4] - 1] + 1);
    }
  *n_out = k;
  return BX_OK;
}

static int kf_xysr_launch(int op, int n, double* x, double* P, const double* arg, double q_xy,
                          double q_s, void* stream) {
  if (n < 0 || !x || !P || (op != 1 && n && !arg))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_kf_xysr_*");
  if (!n) return BX_OK;
  hipLaunchKernelGGL(kf_xysr_kernel, dim3((8 * n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     op, n, x, P, arg, q_xy, q_s);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_kf_xysr_initiate(int n, const double* bbox, double* x, double* P, void* stream) {
  return kf_xysr_launch(0, n, x, P, bbox, 0.0, 0.0, stream);
}
int bx_kf_xysr_predict(int n, double* x, double* P, double q_xy_scaling, double q_s_scaling,
                       void* stream) {
  return kf_xysr_launch(1, n, x, P, nullptr, q_xy_scaling, q_s_scaling, stream);
}
int bx_kf_xysr_update(int n, double* x, double* P, const double* z, void* stream) {
  return kf_xysr_launch(2, n, x, P, z, 0.0, 0.0, stream);
}

int bx_ocsort_status(bx_ocsort* e, int* status) {
  if (!e || !status) return bx_record_error(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipMemcpy(status, e->dev.status, sizeof(int), hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_ocsort_counters_host(bx_ocsort* e, int seq, int* frame_count, int* id_count,
                            int* n_tracks) {
  return ocs_counters(e, seq, frame_count, id_count, n_tracks);
}

int bx_ocsort_set_id_count(bx_ocsort* e, int seq, int id_count, void* stream) {
  return ocs_set_id_count(e, seq, id_count, stream);
}

int bx_ocsort_set_frame_size(bx_ocsort* e, int seq, double w, double h, void* stream) {
  return ocs_set_frame_size(e, seq, w, h, stream);
}

int bx_ocsort_set_seq_params_host(bx_ocsort* e, int seq0, int nseq,
                                  const bx_ocsort_seq_params* params_host, void* stream) {
  if (!e || e->seqtab.bad_range(seq0, nseq, e->dev.S))
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  for (int k = 0; params_host && k < nseq; k++) {  // every entry first: a bad one changes nothing
    if (bad_delta_t(params_host[k].delta_t))
      return bx_record_error(BX_ERR_INVALID, "delta_t must be in [1, 7]");
    if (bad_asso_kind(params_host[k].asso_kind))
      return bx_record_error(BX_ERR_INVALID, "unknown asso_kind");
  }
  if (!nseq || (!params_host && !e->seqtab.allocated())) return BX_OK;  // (nothing to clear)
  std::vector<OcsSeqPar> stage(nseq, OcsSeqPar{});
  for (int k = 0; params_host && k < nseq; k++) {
    const bx_ocsort_seq_params& p = params_host[k];
    OcsSeqPar& d = stage[k];
    d.min_conf = p.min_conf;
    d.det_thresh = p.det_thresh;
    d.asso_threshold = p.asso_threshold;
    d.inertia = p.inertia;
    d.q_xy = 1.0 * p.q_xy_scaling;
    d.q_s = 1.0 * p.q_s_scaling;
    d.max_age = p.max_age;
    d.min_hits = p.min_hits;
    d.delta_t = p.delta_t;
    d.use_byte = p.use_byte;
    d.asso_kind = p.asso_kind;
    d.set = 1;
  }
  if (int rc = e->seqtab.put(seq0, stage, e->dev.S, (hipStream_t)stream,
                             "allocation or copy of the OCSort parameter table failed"))
    return rc;
  e->dev.seqpar = e->seqtab.dev;
  return BX_OK;
}

int bx_ocsort_seq_params_host(bx_ocsort* e, int seq, bx_ocsort_seq_params* out_host) {
  if (!e || seq < 0 || seq >= e->dev.S || !out_host)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_ocsort_seq_params_host");
  const bx_ocsort_config& c = e->cfg;
  bx_ocsort_seq_params o = {c.min_conf, c.det_thresh, c.asso_threshold, c.inertia, c.q_xy_scaling,
                            c.q_s_scaling, c.max_age, c.min_hits, c.delta_t, c.use_byte,
                            c.asso_kind};
  if (const OcsSeqPar* d = e->seqtab.set_entry(seq))
    o = {d->min_conf, d->det_thresh, d->asso_threshold, d->inertia, d->q_xy, d->q_s, d->max_age,
         d->min_hits, d->delta_t, d->use_byte, d->asso_kind};
  *out_host = o;
  return BX_OK;
}

int bx_ocsort_tracks_host(bx_ocsort* e, int seq, int cap, int32_t* ids, double* x, double* p,
                          int* n) {
  if (!e || seq < 0 || seq >= e->dev.S || cap < 0 || !n)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_ocsort_tracks_host");
  std::vector<int> ord;
  int rc = ocs_list_order(e->dev, seq, ord);
  if (rc) return rc;
  const int nt = (int)ord.size();
  for (int k = 0; k < nt && k < cap; k++) {
    OcsTrk t;
    BX_HIPCHK(hipMemcpy(&t, e->dev.trk + (size_t)seq * e->dev.T + ord[k], sizeof(OcsTrk),
                   hipMemcpyDeviceToHost));
    // a per-class sequence reports the class-global id its rows carry (minus one)
    const bool g = seq < (int)e->gid.size() && t.id >= 0 && t.id < (int)e->gid[seq].size();
    if (ids) ids[k] = g ? e->gid[seq][t.id] : t.id;
    if (x) memcpy(x + 7 * k, t.x, sizeof(t.x));
    if (p) memcpy(p + 49 * k, t.P, sizeof(t.P));
  }
  *n = nt;
  return BX_OK;
}

int bx_ocsort_state_set_host(bx_ocsort* e, int seq, int n, const int32_t* ids, const double* x,
                             const double* p) {
  if (!e || seq < 0 || seq >= e->dev.S || n < 0 || (n && !ids))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_ocsort_state_set_host");
  std::vector<int> ord;
  int rc = ocs_list_order(e->dev, seq, ord);
  if (rc) return rc;
  for (int j = 0; j < n; j++) {
    OcsTrk t;
    int slot;
    if ((rc = ocs_find_track(e->dev, e->dev.trk, seq, ord, ids[j], t, &slot))) return rc;
    if (x) memcpy(t.x, x + 7 * j, sizeof(t.x));
    if (p) memcpy(t.P, p + 49 * j, sizeof(t.P));
    BX_HIPCHK(hipMemcpy(e->dev.trk + (size_t)seq * e->dev.T + slot, &t, sizeof(OcsTrk),
                   hipMemcpyHostToDevice));
  }
  return BX_OK;
}

int bx_ocsort_frame_stats_host(bx_ocsort* e, int seq0, int nseq, int64_t* sums) {
  return ocs_frame_stats(e, "bx_ocsort_frame_stats_host", seq0, nseq, sums);
}

// diagnostic (not in the public header): the phase stamps of every sequence, [S][OCS_DBG]
int bx_ocsort_debug_host(bx_ocsort* e, unsigned long long* out) {
  if (!e || !out || !e->dev.dbg) return bx_record_error(BX_ERR_INVALID, "not a timing build");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(out, e->dev.dbg, sizeof(unsigned long long) * OCS_DBG * e->dev.S,
                 hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_ocsort_probe(bx_ocsort* e, int on) {
  if (!e) return bx_record_error(BX_ERR_INVALID, "null engine");
  e->probe.set(on != 0 ? 0 : -1);
  return BX_OK;
}

int bx_ocsort_probe_read(bx_ocsort* e, double* total_ms, int* count) {
  if (!e || !total_ms || !count) return bx_record_error(BX_ERR_INVALID, "null argument");
  return e->probe.read(total_ms, count);
}

}  // extern "C"
