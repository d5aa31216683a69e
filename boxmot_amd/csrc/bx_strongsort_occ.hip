// bx_strongsort_occ.hip - StrongSort's occlusion handling (handle_occlusions=True) as the last
// launch of a frame, in a code object of its own: bx_strongsort.hip up to the end of its kernels,
// then ss_occ_kernel and the entry points bx_strongsort.hip's host code calls.  Only an engine on
// which bx_ss_set_occlusion_host was ever called launches it; every other engine runs the code
// objects it ran before this unit existed (as 2.24 for the table builds).
//
// Reference: OcclusionAwareTracker.update_with_occlusion_handling and OcclusionStateManager
// (utils/occlusion_handler.py:45-439; strongsort.py:150-154, 195-201, 324-354), as
// boxmot_amd/occlusion.py (OcclusionHandler.__call__) and oracle/bxo_strongsort.c
// (occlusion_update) restate them.  All fp64, in their operation order.
#define BX_SS_OCC_UNIT
#include "bx_strongsort.hip"

#include "bx_pyset.h"

namespace {

enum { OJ_APPEND = 1, OJ_MOVE = 2, OJ_BLEND = 4, OJ_RELEASE = 8, OJ_MOVED = 16 };

// One ordered visit (i, j) of update_occlusion_state over boxes in LDS (the tlwh rows read as
// corner boxes): 0 no occlusion above the threshold, 1 i occludes j, 2 j occludes i, 3 mutual.
// _pair_tables: the overlap and the ratio are formed for the pair's lower position first; the
// ratio of the visit from the higher position is 1.0 / r, not the other quotient.
__device__ __forceinline__ int occ_pair(const double* bx, const double* area, int i, int j,
                                        double thr, double& o_out) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  const double* A = bx + 4 * a;
  const double* B = bx + 4 * b;
  const double xx1 = pymax(A[0], B[0]), yy1 = pymax(A[1], B[1]);
  const double xx2 = pymin(A[2], B[2]), yy2 = pymin(A[3], B[3]);
  const double inter = pymax(0.0, xx2 - xx1) * pymax(0.0, yy2 - yy1);
  const double o = inter > 0 ? pymax(inter / area[a], inter / area[b]) : 0.0;
  if (!(o > thr)) return 0;
  double r = area[b] > 0 ? area[a] / area[b] : 1.0;
  if (i > j) r = 1.0 / r;
  o_out = o;
  return r > 1.2 ? 1 : (r < 0.8 ? 2 : 3);
}

// ss_occ_kernel: one workgroup of four waves per stepped sequence, after ss_fit_kernel.
//   1 the track list's tlwh rows, areas and ids into LDS (thread per track)
//   2 analysis, thread per row i over j ascending (box j is an LDS broadcast): visibility as the
//     ordered product, the row's occluder count, a mutual visit -> latch and return
//   3 pool: entries of ids in neither the list nor the lost buffer are released, each row finds
//     its entry; scalar edits (thread per row); new entries in list order (wave 0, ballot scan)
//   4 F-wide work, a wave per vector: ring appends (waves strided over rows), blends of
//     emerging tracks (wave 0; ss_feat_set_kernel's steps and reduction orders)
//   5 moves, wave 0 in list order (a move reads occluder means an earlier move may have
//     written): occluders by ballot compaction, set order and centre sum on lane 0
//   6 the sequence's output rows again (wave 0, ss_post_kernel's list-order scan)
__global__ void __launch_bounds__(256)
    ss_occ_kernel(SsDev g, SsOcc oc, int seq0, const int* __restrict__ det_off,
                  double* __restrict__ out) {
  extern __shared__ __align__(16) char occ_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, seq = seq0 + b;
  if (!oc.on[seq] || oc.mutual[seq]) return;
  int* sq = g.sq + (size_t)seq * SQS;
  const int n = sq[Q_NTR];
  if (n <= 0 || n > g.T) return;
  const int T = g.T, F = g.F, cap = oc.cap;
  double* bx = (double*)occ_lds;
  double* area = bx + 4 * T;
  double* lvl = area + T;
  double* leaf = lvl + T;
  int* slot = (int*)(leaf + PW_MAXLEAF);
  int* ids = slot + T;
  int* nocc = ids + T;
  int* job = nocc + T;
  int* pe = job + T;
  int* adds = pe + T;
  int* keys = adds + T;
  int* sord = keys + T;
  int* tabA = sord + T;
  int* tabB = tabA + oc.setcap;
  int* pid = tabB + oc.setcap;
  int* lo = pid + cap;
  int* ln = lo + PW_MAXLEAF;
  int* sc = ln + PW_MAXLEAF;
  SsTrk* trk = g.trk + (size_t)seq * T;
  const int* order = g.order + (size_t)seq * T;
  const double thr = oc.thr[seq];
  const size_t p0 = (size_t)seq * cap;

  // ---- 1: boxes ------------------------------------------------------------------------------
  for (int p = tid; p < n; p += 256) {
    const int s = order[p];
    const SsTrk& t = trk[s];
    double r[4];
    to_tlwh(t, r);
    slot[p] = s;
    ids[p] = t.id;
    bx[4 * p] = r[0], bx[4 * p + 1] = r[1], bx[4 * p + 2] = r[2], bx[4 * p + 3] = r[3];
    area[p] = (r[2] - r[0]) * (r[3] - r[1]);
  }
  for (int e = tid; e < cap; e += 256) pid[e] = oc.pid[p0 + e];
  if (tid == 0) sc[0] = 0;
  __syncthreads();

  // ---- 2: update_occlusion_state ---------------------------------------------------------------
  for (int i = tid; i < n; i += 256) {
    double vis = 1.0;
    int k = 0;
    bool mut = false;
    for (int j = 0; j < n; j++) {
      if (j == i) continue;
      double o;
      const int c = occ_pair(bx, area, i, j, thr, o);
      if (c == 3) mut = true;
      if (c == 2) {
        vis *= (1.0 - o);
        k++;
      }
    }
    lvl[i] = 1.0 - vis;
    nocc[i] = k;
    job[i] = 0;
    pe[i] = -1;
    if (mut) sc[0] = 1;
  }
  __syncthreads();
  if (sc[0]) {  // _resolve_mutual_occlusion's TypeError: no edits, the update count latched
    if (tid == 0) oc.mutual[seq] = sq[Q_FRAME];
    return;
  }

  // ---- 3: the pool and the scalar edits --------------------------------------------------------
  {
    const int nlost = sq[Q_NLOST];
    const int* lost = g.lost + (size_t)seq * LOSTN;
    for (int e = tid; e < cap; e += 256) {
      const int id = pid[e];
      if (!id) continue;
      // the host keeps a dead track's buffer for ever; only an id that can come back matters, and
      // ID recovery revives ids of the lost buffer: an entry goes when its id is in neither
      bool live = false;
      for (int p = 0; p < n && !live; p++) live = ids[p] == id;
      for (int k = 0; k < nlost && k < LOSTN && !live; k++) live = trk[lost[k]].id == id;
      if (!live) {
        pid[e] = 0;
        oc.pid[p0 + e] = 0;
        oc.pcnt[p0 + e] = 0;
        oc.phead[p0 + e] = 0;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {  // _apply_occlusion_modifications' scalar part
    int e = -1;
    for (int q = 0; q < cap; q++)
      if (pid[q] == ids[i]) {
        e = q;
        break;
      }
    pe[i] = e;
    SsTrk& t = trk[slot[i]];
    const double L = lvl[i];
    int jb = 0;
    if (L > 0.3) {
      t.max_age = t.max_age >= (1 << 29) ? (1 << 30) : (int)(t.max_age * 2.0);
      t.quality = pymax(t.quality, 0.6);
      if (t.nfeat > 0) jb |= OJ_APPEND;
      if (L > 0.8 && nocc[i] > 0) jb |= OJ_MOVE;
    } else if (e >= 0) {  // _handle_emerging_track
      t.conf = pymin(t.conf + 0.1, 1.0);
      if (oc.pcnt[p0 + e] > 0 && t.nfeat > 0) jb |= OJ_BLEND;
      jb |= OJ_RELEASE;
    }
    job[i] = jb;
  }
  __syncthreads();
  if (wave == 0) {  // first appends take a free entry, in list order; a full pool skips the append
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool need = i < n && (job[i] & OJ_APPEND) && pe[i] < 0;
      unsigned long long m = __ballot(need);
      if (lane == 0)
        while (m) {
          const int ii = base + __ffsll((long long)m) - 1;
          m &= m - 1;
          int e = 0;
          while (e < cap && pid[e] != 0) e++;
          if (e < cap) {
            pid[e] = ids[ii];
            pe[ii] = e;
            oc.pid[p0 + e] = ids[ii];
            oc.pcnt[p0 + e] = 0;
            oc.phead[p0 + e] = 0;
          } else {
            atomicExch(g.status, (int)BX_ERR_CAPACITY);
            job[ii] &= ~OJ_APPEND;
          }
        }
      wsync();
    }
  }
  __syncthreads();

  // ---- 4: ring appends (deque(maxlen=10).append(features[-1])) ----------------------------------
  for (int i = wave; i < n; i += 4) {
    if (!(job[i] & OJ_APPEND)) continue;
    const SsTrk& t = trk[slot[i]];
    const size_t pi = p0 + pe[i];
    const int cnt = oc.pcnt[pi], head = oc.phead[pi];
    const int w = cnt < OCC_RING ? (head + cnt) % OCC_RING : head;  // full: over the oldest
    const double* src = vecp(g, seq, slot[i], t.feat[t.nfeat - 1]);
    double* dst = oc.pvec + (pi * OCC_RING + w) * (size_t)F;
    for (int q = lane; q < F; q += 64) dst[q] = src[q];
    const double nv = sqrt(wdot(src, src, F));
    wsync();
    if (lane == 0) {
      oc.pnorm[pi * OCC_RING + w] = nv;
      if (cnt < OCC_RING) oc.pcnt[pi] = cnt + 1;
      else oc.phead[pi] = (head + 1) % OCC_RING;
    }
  }
  if (wave == 0) {
    // ---- 4: blends of emerging tracks (their entries are not appended to this frame) ----------
    for (int i = 0; i < n; i++) {
      if (!(job[i] & OJ_BLEND)) continue;
      SsTrk& t = trk[slot[i]];
      const size_t pi = p0 + pe[i];
      const int cnt = oc.pcnt[pi], head = oc.phead[pi];
      int best = 0;  // max(stored, key=norm): the first of the largest
      double bn = oc.pnorm[pi * OCC_RING + head % OCC_RING];
      for (int k = 1; k < cnt; k++) {
        const double v = oc.pnorm[pi * OCC_RING + (head + k) % OCC_RING];
        if (v > bn) bn = v, best = k;
      }
      const double* bv = oc.pvec + (pi * OCC_RING + (head + best) % OCC_RING) * (size_t)F;
      const int lv = t.feat[t.nfeat - 1];
      int v = 0;
      if (lane == 0) {  // (ss_feat_set_kernel: the gallery keeps the replaced vector's content)
        v = ((t.gmask >> lv) & 1ull) ? pool_alloc(t, g.VP) : lv;
        if (v < 0) atomicExch(g.status, (int)BX_ERR_TRACK_OVERFLOW);
      }
      v = __shfl(v, 0);
      if (v < 0) continue;
      const double* cur = vecp(g, seq, slot[i], lv);
      double* dst = vecp(g, seq, slot[i], v);
      double s = 0.0;
      for (int q = lane; q < F; q += 64) {
        const double x = 0.7 * cur[q] + 0.3 * bv[q];
        s += x * x;
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
      const double ns = sqrt(s) + 1e-8;
      for (int q = lane; q < F; q += 64) {  // (in place when v == lv: a lane's own elements)
        const double x = 0.7 * cur[q] + 0.3 * bv[q];
        dst[q] = x / ns;
      }
      wsync();
      const double wn = sqrt(wdot(dst, dst, F));
      const double pn = wpw_norm(dst, F, lo, ln, leaf) + 1e-8;
      double* dstn = vecnp(g, seq, slot[i], v);
      for (int q = lane; q < F; q += 64) dstn[nn_pos(q, F)] = dst[q] / pn;
      if (lane == 0) {
        const size_t vi = vidx(g, seq, slot[i], v);
        g.vwn[vi] = wn;
        g.vden[vi] = pn;
        t.feat[t.nfeat - 1] = v;
      }
      wsync();
    }
    // ---- 5: _update_track_with_predicted_position, in list order -------------------------------
    for (int i = 0; i < n; i++) {
      if (!(job[i] & OJ_MOVE)) continue;
      int cnt = 0;  // the row's occluders, ascending list position: the set's insertion order
      for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        bool p = false;
        if (j < n && j != i) {
          double o;
          p = occ_pair(bx, area, i, j, thr, o) == 2;
        }
        const unsigned long long m = __ballot(p);
        if (p) {
          const int k = cnt + __popcll(m & ((1ull << lane) - 1ull));
          adds[k] = j;
          keys[k] = ids[j];
        }
        cnt += __popcll(m);
      }
      wsync();
      SsTrk& t = trk[slot[i]];
      if (lane == 0) {
        const int m = bx_pyset_order<int>(keys, cnt, tabA, tabB, sord);
        double c0 = 0.0, c1 = 0.0;
        int kc = 0;
        for (int q = 0; q < m; q++) {  // the occluders' current means, earlier moves included
          double bb[4];
          to_tlwh(trk[slot[adds[sord[q]]]], bb);
          const double cx = (bb[0] + bb[2]) / 2, cy = (bb[1] + bb[3]) / 2;
          c0 = kc ? c0 + cx : cx;
          c1 = kc ? c1 + cy : cy;
          kc++;
        }
        const double px = c0 / kc - 50 / 2.0, py = c1 / kc - 100 / 2.0;
        const double pw = 50.0, ph = 100.0;
        t.mean[0] = px + pw / 2;
        t.mean[1] = py + ph / 2;
        t.mean[2] = pw / ph;
        t.mean[3] = ph;
        job[i] |= OJ_MOVED;
      }
      if (lane < 16) t.cov[8 * (lane >> 2) + (lane & 3)] *= 1.5;
      wsync();
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256)  // del occlusion_buffer[track.id]
    if (job[i] & OJ_RELEASE) {
      oc.pid[p0 + pe[i]] = 0;
      oc.pcnt[p0 + pe[i]] = 0;
      oc.phead[p0 + pe[i]] = 0;
    }

  // ---- 6: the output rows (strongsort.py:324-354) ------------------------------------------------
  if (wave == 0) {
    const int r0 = det_off[b];
    int nd = det_off[b + 1] - r0;
    if (nd > g.D) nd = g.D;
    double* orow = out + (size_t)r0 * 10;
    int q0 = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      bool p = false;
      if (i < n) {
        const SsTrk& t = trk[slot[i]];
        p = t.state == 2 && t.tsu < 1;
      }
      const unsigned long long m = __ballot(p);
      if (p) {
        const int q = q0 + __popcll(m & ((1ull << lane) - 1ull));
        if (q < nd) {
          const SsTrk& t = trk[slot[i]];
          double* o = orow + (size_t)q * 10;
          if (job[i] & OJ_MOVED) {
            double bb[4];
            to_tlbr(t, bb);
            o[0] = bb[0], o[1] = bb[1], o[2] = bb[2], o[3] = bb[3];
          }
          o[5] = t.conf, o[8] = t.quality, o[9] = lvl[i];
        }
      }
      q0 += __popcll(m);
    }
  }
}

}  // namespace

int bx_ss_occ_lds_attr(size_t lds) { return (int)bx_lds_attr((const void*)ss_occ_kernel, lds); }

void bx_ss_occ_launch(const void* dev, const void* occ, int nseq, size_t lds, hipStream_t st,
                      int seq0, const int* off, double* out) {
  hipLaunchKernelGGL(ss_occ_kernel, dim3(nseq), dim3(256), lds, st, *(const SsDev*)dev,
                     *(const SsOcc*)occ, seq0, off, out);
}
