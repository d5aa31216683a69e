// bx_classes.hip — per_class=True on the device: class split and id merge (include/bxclasses.h).
//
// Reference: per_class_decorator (boxmot/trackers/basetracker.py:155-201) over
// get_class_dets_n_embs (:83-106): the update runs once per class id on dets[dets[:, 5] == c],
// every class on its own track list, KalmanBoxTracker.count shared, the classes' rows stacked in
// class order.  bx_ocsort_update_classes_host restates that loop on the host (split, one launch
// over the classes, renumber); here the split and the renumbering are kernels, for S sequences of
// C classes per launch, so the batched flow and the resident feeder never return to the host
// within a frame:
//   class_count_kernel  one workgroup per sequence: rows per class (LDS histogram; a count does
//                       not depend on the order of its atomic adds) and their sum
//   class_split_kernel  one workgroup (4 waves) per sequence: its first output row is the sum of
//                       the earlier sequences' kept rows, the class offsets an exclusive scan of
//                       its histogram, a row's place the class offset plus the rows of its class
//                       before it (counted, no atomics: stable and deterministic); dets rows move
//                       as three 8-byte pairs, embedding rows a wave per row as 16-byte loads and
//                       stores (8-byte ones where source and destination differ in 16-byte phase:
//                       odd emb_dim)
//   class_merge_kernel  one workgroup per sequence: births per class from the engines' next-id
//                       counters, their class-global ids into the map, column 4 through the map,
//                       rows compacted in class order
// Values are written with plain C++ and vector stores; everything runs on the caller's stream.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/bxclasses.h"
#include "bx_host.h"


namespace {

constexpr int CW = 256;  // threads per workgroup (4 waves)

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

struct ClsDev {
  int S, C, F, row_cap, map_cap, id0;
  int* hist;    // [S][C] rows per class of the call's sequences
  int* tot;     // [S] kept rows of the call's sequences (the sum of a hist row)
  int* lids;    // [S * C] next-id counter of each engine sequence as the last merge saw it
  int* gctr;    // [S] class-global next id
  int* map;     // [S * C][map_cap] local id - id0 -> class-global id
  int* status;
};

// cls_of of bx_ocsort_update_classes_host: an integer in [0, C), else -1
__device__ __forceinline__ int cls_of(float v, int C) {
  return (v >= 0.f && v < (float)C && v == (float)(int)v) ? (int)v : -1;
}

// rows of call-local sequence s; more than row_cap (or a descending det_off): none, latched
__device__ __forceinline__ int seq_rows(const ClsDev& d, const int* det_off, int s, int* r0) {
  *r0 = det_off[s];
  const int n = det_off[s + 1] - *r0;
  if (n < 0 || n > d.row_cap) {
    if (threadIdx.x == 0) atomicMax(d.status, (int)BX_ERR_CAPACITY);
    return 0;
  }
  return n;
}

__global__ void __launch_bounds__(CW)
class_count_kernel(ClsDev d, const float* __restrict__ dets, const int* __restrict__ det_off) {
  const int s = blockIdx.x, tid = threadIdx.x;
  __shared__ int h[BX_CLASSES_MAX];
  for (int c = tid; c < d.C; c += CW) h[c] = 0;
  __syncthreads();
  int r0;
  const int n = seq_rows(d, det_off, s, &r0);
  for (int i = tid; i < n; i += CW) {
    const int c = cls_of(dets[(size_t)(r0 + i) * 6 + 5], d.C);
    if (c >= 0) atomicAdd(&h[c], 1);
  }
  __syncthreads();
  int kept = 0;
  for (int c = tid; c < d.C; c += CW) {
    d.hist[(size_t)s * d.C + c] = h[c];
    kept += h[c];
  }
  // the sequence's kept rows, so that the split's prefix runs over S values, not S * C
  __shared__ int part[CW / 64];
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_down(kept, o);
  if ((tid & 63) == 0) part[tid >> 6] = kept;
  __syncthreads();
  if (tid == 0) {
    int a = 0;
    for (int w = 0; w < CW / 64; w++) a += part[w];
    d.tot[s] = a;
  }
}

__global__ void __launch_bounds__(CW)
class_split_kernel(ClsDev d, int nseq, const float* __restrict__ dets,
                   const int* __restrict__ det_off, const double* __restrict__ embs,
                   float* __restrict__ o_dets, double* __restrict__ o_embs,
                   int* __restrict__ o_off, int* __restrict__ o_src) {
  const int s = blockIdx.x, tid = threadIdx.x, C = d.C;
  __shared__ int start[BX_CLASSES_MAX + 1];
  __shared__ short cls[BX_CLASSES_ROW_MAX];
  __shared__ short perm[BX_CLASSES_ROW_MAX];
  __shared__ int part[CW / 64];
  // first output row: the kept rows of the call's earlier sequences
  int sum = 0;
  for (int q = tid; q < s; q += CW) sum += d.tot[q];
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
  if ((tid & 63) == 0) part[tid >> 6] = sum;
  int r0;
  const int n = seq_rows(d, det_off, s, &r0);
  for (int i = tid; i < n; i += CW) cls[i] = (short)cls_of(dets[(size_t)(r0 + i) * 6 + 5], C);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < CW / 64; w++) base += part[w];
  if (tid == 0) {
    int a = 0;
    for (int c = 0; c < C; c++) {
      start[c] = a;
      a += d.hist[(size_t)s * C + c];
    }
    start[C] = a;
  }
  __syncthreads();
  const int kept = start[C];
  for (int c = tid; c < C; c += CW) o_off[(size_t)s * C + c] = base + start[c];
  if (tid == 0 && s == nseq - 1) o_off[(size_t)nseq * C] = base + kept;
  // a row's place: its class's first row plus the rows of its class before it
  for (int i = tid; i < n; i += CW) {
    const int c = cls[i];
    if (c < 0) continue;
    int before = 0;
    for (int j = 0; j < i; j++) before += cls[j] == c;
    const int p = start[c] + before;
    if (p < kept) perm[p] = (short)i;  // (always: the histogram counted these rows)
  }
  __syncthreads();
  for (int p = tid; p < kept; p += CW) o_src[base + p] = perm[p];
  // dets: 6 floats = three 8-byte pairs per row
  for (int k = tid; k < kept * 3; k += CW) {
    const int p = k / 3, j = k - p * 3;
    const f2* src = (const f2*)(dets + (size_t)(r0 + perm[p]) * 6);
    f2* dst = (f2*)(o_dets + (size_t)(base + p) * 6);
    dst[j] = src[j];
  }
  const int F = d.F;
  if (!F) return;
  // embeddings: a wave per row
  const int wave = tid >> 6, lane = tid & 63;
  for (int p = wave; p < kept; p += CW / 64) {
    const double* src = embs + (size_t)(r0 + perm[p]) * F;
    double* dst = o_embs + (size_t)(base + p) * F;
    const uintptr_t ms = (uintptr_t)src & 15, md = (uintptr_t)dst & 15;
    if (ms != md) {
      for (int i = lane; i < F; i += 64) dst[i] = src[i];
      continue;
    }
    const int head = ms ? 1 : 0;  // one element reaches the 16-byte boundary
    if (lane == 0 && head) dst[0] = src[0];
    const int nv = (F - head) / 2;
    const d2* sv = (const d2*)(src + head);
    d2* dv = (d2*)(dst + head);
    for (int i = lane; i < nv; i += 64) dv[i] = sv[i];
    const int done = head + 2 * nv;
    if (lane == 0 && done < F) dst[done] = src[done];
  }
}

__global__ void __launch_bounds__(CW)
class_merge_kernel(ClsDev d, int seq0, const int* __restrict__ c_off,
                   const double* __restrict__ c_out, const int* __restrict__ c_cnt,
                   const int* __restrict__ ids, int ids_stride, const int* __restrict__ det_off,
                   double* __restrict__ out, int* __restrict__ out_count) {
  const int k = blockIdx.x, seq = seq0 + k, tid = threadIdx.x, C = d.C;
  __shared__ int gfirst[BX_CLASSES_MAX];  // class-global id of the class's first birth
  __shared__ int ofirst[BX_CLASSES_MAX + 1];
  __shared__ int bad, gnext;
  const size_t q0 = (size_t)seq * C;  // the sequence's first engine sequence
  const int room = det_off[k + 1] - det_off[k];
  if (tid == 0) {
    // the gid loop of bx_ocsort_update_classes_host: births in class order take the next ids
    int g = d.gctr[seq], o = 0, b = 0;
    for (int c = 0; c < C; c++) {
      const int now = ids[(q0 + c) * (size_t)ids_stride], had = d.lids[q0 + c];
      const int cnt = c_cnt[(size_t)k * C + c];
      const int cap = c_off[(size_t)k * C + c + 1] - c_off[(size_t)k * C + c];
      if (now < had || now - d.id0 > d.map_cap || cnt < 0 || cnt > cap) b = 1;
      gfirst[c] = g;
      ofirst[c] = o;
      g += now - had;
      o += cnt;
    }
    ofirst[C] = o;
    gnext = g;
    if (o > room) b = 1;
    bad = b;
  }
  __syncthreads();
  if (bad) {  // nothing is stored for the sequence
    if (tid == 0) {
      atomicMax(d.status, (int)BX_ERR_CAPACITY);
      out_count[k] = 0;
    }
    return;
  }
  for (int c = 0; c < C; c++) {
    const int now = ids[(q0 + c) * (size_t)ids_stride], had = d.lids[q0 + c];
    int* map = d.map + (q0 + c) * (size_t)d.map_cap;
    for (int l = had + tid; l < now; l += CW) map[l - d.id0] = gfirst[c] + (l - had);
  }
  __syncthreads();  // the map is written, the counters are read
  double* orow = out + (size_t)det_off[k] * 8;
  for (int c = 0; c < C; c++) {
    const int now = ids[(q0 + c) * (size_t)ids_stride];
    const int* map = d.map + (q0 + c) * (size_t)d.map_cap;
    const double* src = c_out + (size_t)c_off[(size_t)k * C + c] * 8;
    const int cnt = ofirst[c + 1] - ofirst[c];
    for (int j = tid; j < cnt; j += CW) {
      const d2* sv = (const d2*)(src + (size_t)j * 8);
      d2 v0 = sv[0], v1 = sv[1], v2 = sv[2], v3 = sv[3];
      const int l = (int)v2.x - d.id0;
      if (l >= 0 && l < now - d.id0) v2.x = (double)map[l];
      else atomicMax(d.status, (int)BX_ERR_INVALID);  // (an id the engine never gave out)
      d2* dv = (d2*)(orow + (size_t)(ofirst[c] + j) * 8);
      dv[0] = v0;
      dv[1] = v1;
      dv[2] = v2;
      dv[3] = v3;
    }
    if (tid == 0) d.lids[q0 + c] = now;
  }
  if (tid == 0) {
    d.gctr[seq] = gnext;
    out_count[k] = ofirst[C];
  }
}

__global__ void class_reset_kernel(ClsDev d, int seq0, int nseq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nseq * d.C) d.lids[(size_t)seq0 * d.C + i] = d.id0;
  if (i < nseq) d.gctr[seq0 + i] = d.id0;
}

}  // namespace

struct bx_classes {
  ClsDev dev{};
  void* arena = nullptr;
  float* s_dets = nullptr;
  double* s_embs = nullptr;
  int* s_off = nullptr;
  int* s_src = nullptr;
  double* s_out = nullptr;
  int* s_cnt = nullptr;
};

extern "C" {

int bx_classes_create(int n_seq, int n_classes, int emb_dim, int row_cap, int map_cap, int id0,
                      bx_classes** out) {
  if (!out) return bx_record_error(BX_ERR_INVALID, "null argument");
  if (n_seq <= 0 || n_classes <= 0 || n_classes > BX_CLASSES_MAX || emb_dim < 0 || row_cap <= 0 ||
      row_cap > BX_CLASSES_ROW_MAX || map_cap <= 0 || id0 < 0)
    return bx_record_error(BX_ERR_INVALID, "bx_classes_create: n_seq/n_classes/emb_dim/row_cap/"
                                           "map_cap/id0 out of range");
  const size_t S = n_seq, C = n_classes, F = emb_dim, R = S * (size_t)row_cap;
  if (S * C >= (1u << 30) || R >= (1u << 30) || S * C * (size_t)map_cap >= ((size_t)1 << 40))
    return bx_record_error(BX_ERR_INVALID, "bx_classes_create: too large");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return bx_record_error(BX_ERR_NO_DEVICE, "no HIP device visible");
  bx_classes* c = new bx_classes();
  auto fill = [&]() -> int {
    ClsDev& d = c->dev;
    d.S = n_seq;
    d.C = n_classes;
    d.F = emb_dim;
    d.row_cap = row_cap;
    d.map_cap = map_cap;
    d.id0 = id0;
    BxCarve carve;
    const size_t o_hist = carve(S * C * 4), o_lids = carve(S * C * 4), o_g = carve(S * 4);
    const size_t o_tot = carve(S * 4);
    const size_t o_map = carve(S * C * (size_t)map_cap * 4), o_st = carve(16);
    const size_t o_sd = carve(R * 6 * 4), o_se = carve(R * (F ? F : 1) * 8);
    const size_t o_so = carve((S * C + 1) * 4), o_ss = carve(R * 4), o_sr = carve(R * 8 * 8);
    const size_t o_sc = carve(S * C * 4);
    if (hipMalloc(&c->arena, carve.off) != hipSuccess)
      return bx_record_error(BX_ERR_HIP, "hipMalloc of the class state failed");
    BX_HIPCHK(hipMemset(c->arena, 0, carve.off));
    char* b = (char*)c->arena;
    d.hist = (int*)(b + o_hist);
    d.tot = (int*)(b + o_tot);
    d.lids = (int*)(b + o_lids);
    d.gctr = (int*)(b + o_g);
    d.map = (int*)(b + o_map);
    d.status = (int*)(b + o_st);
    c->s_dets = (float*)(b + o_sd);
    c->s_embs = (double*)(b + o_se);
    c->s_off = (int*)(b + o_so);
    c->s_src = (int*)(b + o_ss);
    c->s_out = (double*)(b + o_sr);
    c->s_cnt = (int*)(b + o_sc);
    std::vector<int> one(S * C, id0);
    BX_HIPCHK(hipMemcpy(d.lids, one.data(), S * C * 4, hipMemcpyHostToDevice));
    BX_HIPCHK(hipMemcpy(d.gctr, one.data(), S * 4, hipMemcpyHostToDevice));
    return BX_OK;
  };
  const int rc = fill();
  if (rc) {
    bx_classes_destroy(c);
    return rc;
  }
  *out = c;
  return BX_OK;
}

int bx_classes_destroy(bx_classes* c) {
  if (!c) return BX_OK;
  (void)hipFree(c->arena);
  delete c;
  return BX_OK;
}

int bx_classes_shape(bx_classes* c, int* n_seq, int* n_classes, int* emb_dim, int* row_cap,
                     int* map_cap, int* id0) {
  if (!c) return bx_record_error(BX_ERR_INVALID, "null class state");
  if (n_seq) *n_seq = c->dev.S;
  if (n_classes) *n_classes = c->dev.C;
  if (emb_dim) *emb_dim = c->dev.F;
  if (row_cap) *row_cap = c->dev.row_cap;
  if (map_cap) *map_cap = c->dev.map_cap;
  if (id0) *id0 = c->dev.id0;
  return BX_OK;
}

int bx_classes_scratch(bx_classes* c, void** s_dets, void** s_off, void** s_embs, void** s_src,
                       void** s_out, void** s_cnt) {
  if (!c) return bx_record_error(BX_ERR_INVALID, "null class state");
  if (s_dets) *s_dets = c->s_dets;
  if (s_off) *s_off = c->s_off;
  if (s_embs) *s_embs = c->dev.F ? c->s_embs : nullptr;
  if (s_src) *s_src = c->s_src;
  if (s_out) *s_out = c->s_out;
  if (s_cnt) *s_cnt = c->s_cnt;
  return BX_OK;
}

int bx_classes_state(bx_classes* c, void** id_counters, void** status) {
  if (!c) return bx_record_error(BX_ERR_INVALID, "null class state");
  if (id_counters) *id_counters = c->dev.gctr;
  if (status) *status = c->dev.status;
  return BX_OK;
}

int bx_classes_split(bx_classes* c, int nseq, const float* dets, const int32_t* det_off,
                     const double* embs, float* o_dets, double* o_embs, int32_t* o_off,
                     int32_t* o_src, void* stream) {
  if (!c || nseq <= 0 || nseq > c->dev.S || !dets || !det_off || !o_dets || !o_off || !o_src ||
      (c->dev.F && (!embs || !o_embs)))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_classes_split");
  if (((uintptr_t)dets | (uintptr_t)o_dets) & 7)
    return bx_record_error(BX_ERR_INVALID, "bx_classes_split: dets must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(class_count_kernel, dim3(nseq), dim3(CW), 0, st, c->dev, dets, det_off);
  BX_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(class_split_kernel, dim3(nseq), dim3(CW), 0, st, c->dev, nseq, dets, det_off,
                     embs, o_dets, o_embs, o_off, o_src);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_classes_merge(bx_classes* c, int seq0, int nseq, const int32_t* c_off, const double* c_out,
                     const int32_t* c_cnt, const int32_t* ids, int ids_stride,
                     const int32_t* det_off, double* out, int32_t* out_count, void* stream) {
  if (!c || seq0 < 0 || nseq <= 0 || seq0 + nseq > c->dev.S || !c_off || !c_out || !c_cnt ||
      !ids || ids_stride <= 0 || !det_off || !out || !out_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_classes_merge");
  if (((uintptr_t)c_out | (uintptr_t)out) & 15)
    return bx_record_error(BX_ERR_INVALID, "bx_classes_merge: out rows must be 16-byte aligned");
  hipLaunchKernelGGL(class_merge_kernel, dim3(nseq), dim3(CW), 0, (hipStream_t)stream, c->dev,
                     seq0, c_off, c_out, c_cnt, ids, ids_stride, det_off, out, out_count);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_classes_reset(bx_classes* c, int seq0, int nseq, void* stream) {
  if (!c || seq0 < 0 || nseq < 0 || seq0 + nseq > c->dev.S)
    return bx_record_error(BX_ERR_INVALID, "bad sequence range");
  if (!nseq) return BX_OK;
  hipLaunchKernelGGL(class_reset_kernel, dim3((nseq * c->dev.C + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, c->dev, seq0, nseq);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_classes_status(bx_classes* c, int* status) {
  if (!c || !status) return bx_record_error(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(status, c->dev.status, sizeof(int), hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_classes_id_count_host(bx_classes* c, int seq, int* id_count) {
  if (!c || seq < 0 || seq >= c->dev.S || !id_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_classes_id_count_host");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(id_count, c->dev.gctr + seq, sizeof(int), hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_classes_set_id_count(bx_classes* c, int seq, int id_count, void* stream) {
  if (!c || seq < 0 || seq >= c->dev.S) return bx_record_error(BX_ERR_INVALID, "bad sequence");
  BX_HIPCHK(hipMemcpyAsync(c->dev.gctr + seq, &id_count, sizeof(int), hipMemcpyHostToDevice,
                      (hipStream_t)stream));
  BX_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return BX_OK;
}

int bx_classes_map_host(bx_classes* c, int seq, int cls, int cap, int32_t* map_host, int* n) {
  if (!c || seq < 0 || seq >= c->dev.S || cls < 0 || cls >= c->dev.C || cap < 0 || !n ||
      (cap && !map_host))
    return bx_record_error(BX_ERR_INVALID, "bad arguments to bx_classes_map_host");
  const size_t q = (size_t)seq * c->dev.C + cls;
  int now = 0;
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(&now, c->dev.lids + q, sizeof(int), hipMemcpyDeviceToHost));
  int m = now - c->dev.id0;
  if (m > c->dev.map_cap) m = c->dev.map_cap;
  *n = m;
  if (m > cap) m = cap;
  if (m > 0)
    BX_HIPCHK(hipMemcpy(map_host, c->dev.map + q * (size_t)c->dev.map_cap, sizeof(int) * m,
                   hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_classes_copy_state(bx_classes* dst, bx_classes* src) {
  if (!dst || !src) return bx_record_error(BX_ERR_INVALID, "null class state");
  const ClsDev &a = src->dev, &b = dst->dev;
  if (a.S != b.S || a.C != b.C || a.F != b.F || b.map_cap < a.map_cap || b.row_cap < a.row_cap ||
      a.id0 != b.id0)
    return bx_record_error(BX_ERR_INVALID, "bx_classes_copy_state: destination must have the "
                                           "source's sequences, classes, emb_dim and id0 and at "
                                           "least its map_cap and row_cap");
  const size_t Q = (size_t)a.S * a.C;
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(b.lids, a.lids, Q * sizeof(int), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.gctr, a.gctr, (size_t)a.S * sizeof(int), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy2D(b.map, (size_t)b.map_cap * sizeof(int), a.map, (size_t)a.map_cap * sizeof(int),
                   (size_t)a.map_cap * sizeof(int), Q, hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipMemcpy(b.status, a.status, sizeof(int), hipMemcpyDeviceToDevice));
  BX_HIPCHK(hipDeviceSynchronize());
  return BX_OK;
}

}  // extern "C"
