// bx_classes_glue.h — what DeepOCSort's and HybridSort's engines share of per_class=True: the
// lazily built class state (include/bxclasses.h) and split -> the engine's own launches over the
// class sequences -> merge, on one stream.  Included by bx_deepocsort.hip and bx_hybridsort.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bxclasses.h"
#include "bx_host.h"


struct ClsGlue {
  bx_classes* cls = nullptr;
  int map_cap = BX_CLASSES_MAP_CAP;
  int* p_g = nullptr;  // pinned: [0] id counter in, [1] id counter out, [2] class status
};

inline void cls_glue_free(ClsGlue& g) {
  bx_classes_destroy(g.cls);
  if (g.p_g) (void)hipHostFree(g.p_g);
  g.cls = nullptr;
  g.p_g = nullptr;
}

// the class state of an engine of S sequences, built by the first per-class call; every later
// call must name the same n_classes
inline int cls_glue_get(ClsGlue& g, int S, int D, int F, int n_classes, int id0) {
  if (n_classes <= 0 || S % n_classes)
    return bx_record_error(BX_ERR_INVALID, "per-class step: the engine's n_seq must be a multiple "
                                           "of n_classes");
  if (g.cls) {
    int c = 0;
    bx_classes_shape(g.cls, nullptr, &c, nullptr, nullptr, nullptr, nullptr);
    if (c != n_classes)
      return bx_record_error(BX_ERR_INVALID, "per-class step: n_classes differs from the engine's "
                                             "first per-class call");
    return BX_OK;
  }
  if (!g.p_g && hipHostMalloc(&g.p_g, sizeof(int) * 4) != hipSuccess)
    return bx_record_error(BX_ERR_HIP, "hipHostMalloc of the per-class mirrors failed");
  return bx_classes_create(S / n_classes, n_classes, F, D, g.map_cap, id0, &g.cls);
}

// One per-class frame for sequences [seq0, seq0 + nseq) of n_classes classes.  ids: the engine's
// next-id counter of engine sequence 0, ids_stride ints apart.  launch(eng_seq0, eng_nseq, dets,
// det_off, embs, out, out_count) is the engine's own frame over engine sequences.
template <class Launch>
int cls_glue_step(ClsGlue& g, int S, int D, int F, int id0, const int* ids, int ids_stride,
                  int seq0, int nseq, int n_classes, const float* dets, const int* det_off,
                  const double* embs, double* out, int* out_count, hipStream_t st,
                  Launch launch) {
  int rc = cls_glue_get(g, S, D, F, n_classes, id0);
  if (rc) return rc;
  if (seq0 < 0 || nseq <= 0 || (seq0 + nseq) * (long)n_classes > S || !dets || !det_off || !out ||
      !out_count)
    return bx_record_error(BX_ERR_INVALID, "bad arguments to the per-class step");
  void *sd, *so, *se, *ss, *sr, *sc;
  bx_classes_scratch(g.cls, &sd, &so, &se, &ss, &sr, &sc);
  if ((rc = bx_classes_split(g.cls, nseq, dets, det_off, embs, (float*)sd, (double*)se, (int*)so,
                             (int*)ss, st)))
    return rc;
  if ((rc = launch(seq0 * n_classes, nseq * n_classes, (const float*)sd, (const int*)so,
                   (const double*)se, (double*)sr, (int*)sc)))
    return rc;
  return bx_classes_merge(g.cls, seq0, nseq, (const int*)so, (const double*)sr, (const int*)sc,
                          ids, ids_stride, det_off, out, out_count, st);
}

inline int cls_glue_reset(ClsGlue& g, int eng_seq0, int eng_nseq, void* stream) {
  if (!g.cls || !eng_nseq) return BX_OK;
  int C = 1;
  bx_classes_shape(g.cls, nullptr, &C, nullptr, nullptr, nullptr, nullptr);
  const int first = eng_seq0 / C, last = (eng_seq0 + eng_nseq + C - 1) / C;
  return bx_classes_reset(g.cls, first, last - first, stream);
}

// capacity growth: the destination engine takes over the source's counters and maps
inline int cls_glue_copy(ClsGlue& dst, ClsGlue& src, int S, int D, int F, int id0) {
  if (!src.cls) return BX_OK;
  int C = 1;
  bx_classes_shape(src.cls, nullptr, &C, nullptr, nullptr, nullptr, nullptr);
  if (!dst.cls) {
    if (dst.map_cap < src.map_cap) dst.map_cap = src.map_cap;
    const int rc = cls_glue_get(dst, S, D, F, C, id0);
    if (rc) return rc;
  }
  return bx_classes_copy_state(dst.cls, src.cls);
}

inline int cls_glue_status(ClsGlue& g, int* status) {
  if (!g.cls || *status) return BX_OK;
  return bx_classes_status(g.cls, status);
}

// the host form's class-level id counter: written before the frame, read back (with the class
// status) after it; take synchronises the stream
inline int cls_glue_put_ids(ClsGlue& g, int seq, int id_count, hipStream_t st) {
  void *ctr, *status;
  bx_classes_state(g.cls, &ctr, &status);
  g.p_g[0] = id_count;
  BX_HIPCHK(hipMemcpyAsync((int*)ctr + seq, g.p_g, sizeof(int), hipMemcpyHostToDevice, st));
  return BX_OK;
}

inline int cls_glue_take_ids(ClsGlue& g, int seq, int* id_count, int* cstatus, hipStream_t st) {
  void *ctr, *status;
  bx_classes_state(g.cls, &ctr, &status);
  BX_HIPCHK(hipMemcpyAsync(g.p_g + 1, (int*)ctr + seq, sizeof(int), hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipMemcpyAsync(g.p_g + 2, status, sizeof(int), hipMemcpyDeviceToHost, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  *id_count = g.p_g[1];
  *cstatus = g.p_g[2];
  return BX_OK;
}
