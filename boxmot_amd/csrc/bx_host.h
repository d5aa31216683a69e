// bx_host.h — the host layer every translation unit of the library shares: the HIP error check,
// the stage timing probe, the update_host staging buffers, the arena carve and the per-sequence
// parameter table.  Host code only
// (nothing __device__ or __global__): including it leaves a file's device code as it was.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bxassoc.h"

int bx_record_error(int code, const char* msg);          // bx_engine.hip (shared bx_last_error)
hipError_t bx_lds_attr(const void* kern, size_t bytes);  // bx_engine.hip (never lowers a limit)

// check a HIP call: on failure record "<call>: <HIP's text>" and return BX_ERR_HIP
#define BX_HIPCHK(x)                                                                      \
  do {                                                                                    \
    hipError_t _e = (x);                                                                  \
    if (_e != hipSuccess)                                                                 \
      return bx_record_error(BX_ERR_HIP,                                                  \
                             (std::string(#x) + ": " + hipGetErrorString(_e)).c_str());   \
  } while (0)

// Arena layout: offsets of consecutive blocks, each rounded up to 256 bytes.
struct BxCarve {
  size_t off = 0;
  size_t operator()(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

// Timing probe: an event pair around every launch of the probed stage.  The events are
// timing-only (no system-scope fence on record, so the probe does not perturb the kernels around
// it) and created on first use; begin/end are a compare-and-return while the stage is off.
struct BxProbe {
  int stage = -1;  // the probed stage (-1: off)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  int used = 0;

  int begin(int s, hipStream_t st) { return s != stage ? BX_OK : record_begin(st); }
  int end(int s, hipStream_t st) {
    if (s != stage) return BX_OK;
    BX_HIPCHK(hipEventRecord(ev[used++].second, st));
    return BX_OK;
  }
  void set(int s) {
    stage = s < 0 ? -1 : s;
    used = 0;
  }
  // the summed time of the pairs recorded since the last set/read, and how many they were
  int read(double* total_ms, int* count) {
    double s = 0.0;
    for (int k = 0; k < used; k++) {
      BX_HIPCHK(hipEventSynchronize(ev[k].second));
      float ms = 0.f;
      BX_HIPCHK(hipEventElapsedTime(&ms, ev[k].first, ev[k].second));
      s += ms;
    }
    *total_ms = s;
    *count = used;
    used = 0;
    return BX_OK;
  }
  void destroy() {
    for (auto& p : ev) {
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
    ev.clear();
    used = 0;
  }

 private:
  int record_begin(hipStream_t st) {
    if (used == (int)ev.size()) {
      hipEvent_t a, b;
      BX_HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
      if (hipError_t r = hipEventCreateWithFlags(&b, hipEventDisableSystemFence); r != hipSuccess) {
        (void)hipEventDestroy(a);
        BX_HIPCHK(r);
      }
      ev.push_back({a, b});
    }
    BX_HIPCHK(hipEventRecord(ev[used].first, st));
    return BX_OK;
  }
};

// An entry's `set` flag: its own, or that of the OcsSeqPar it wraps (DeepOCSort, HybridSort).
template <class E> auto bx_entry_set(const E& e) -> decltype(e.set) { return e.set; }
template <class E> auto bx_entry_set(const E& e) -> decltype(e.o.set) { return e.o.set; }

struct BxNoGiven {};

// The per-sequence parameter table of an engine (*_set_seq_params_host): a zeroed [S] device table
// allocated on first use, its host mirror and, for an engine that echoes the caller's struct back,
// the structs as given.  An engine validates and resolves its entries into a staged range; put()
// is the one place that allocates, uploads and rolls back.
template <class Entry, class Given = BxNoGiven>
struct BxSeqTable {
  Entry* dev = nullptr;       // [S], what the engine's dev.seqpar points to after a put
  std::vector<Entry> mirror;  // [S] once allocated
  std::vector<Given> given;   // [S] once allocated

  static bool bad_range(int seq0, int nseq, int S) {
    return seq0 < 0 || nseq < 0 || seq0 > S - nseq;
  }
  bool allocated() const { return dev != nullptr; }
  // sequence `seq`'s entry when it has one of its own, else null
  const Entry* set_entry(int seq) const {
    return allocated() && bx_entry_set(mirror[seq]) ? &mirror[seq] : nullptr;
  }

  // Entries [seq0, seq0 + stage.size()) := stage (a default Entry clears one), on `st`, which is
  // synchronised.  Nothing is committed before the device holds the range: on a failure a table
  // allocated by this call is freed, an older one gets the mirror's entries back, and pointer,
  // mirror and `given` are as they were.  given_in: the caller's structs of the range, or null.
  int put(int seq0, const std::vector<Entry>& stage, size_t S, hipStream_t st, const char* what,
          const Given* given_in = nullptr) {
    const size_t n = stage.size();
    Entry* tbl = dev;
    const bool first = !tbl;
    bool ok = true;
    if (first) {
      if (hipMalloc(&tbl, S * sizeof(Entry)) != hipSuccess) tbl = nullptr, ok = false;
      ok = ok && hipMemset(tbl, 0, S * sizeof(Entry)) == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(tbl + seq0, stage.data(), n * sizeof(Entry), hipMemcpyHostToDevice,
                              st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
      if (first)
        (void)hipFree(tbl);
      else
        (void)hipMemcpy(tbl + seq0, mirror.data() + seq0, n * sizeof(Entry),
                        hipMemcpyHostToDevice);
      return bx_record_error(BX_ERR_HIP, what);
    }
    if (first) {
      dev = tbl;
      mirror.assign(S, Entry{});
      given.assign(S, Given{});
    }
    for (size_t k = 0; k < n; k++) {
      mirror[seq0 + k] = stage[k];
      if (given_in) given[seq0 + k] = given_in[k];
    }
    return BX_OK;
  }

  // safe on a table that was never allocated, and twice
  void free() {
    (void)hipFree(dev);
    dev = nullptr;
    mirror.clear();
    given.clear();
  }
};

// The buffers of one update_host frame: a device buffer h_* and its pinned mirror p_* (true
// asynchronous copies, one synchronisation per frame) for the detections, the embeddings and
// the warp (both optional), the output rows, the offsets and the output count; p_sq mirrors the
// sequence's counter row.  p_cnt: [0] out count, [1] status, [2..3] the frame's offsets {0, n}.
// Sized in bytes: the element types differ between the engines.
struct BxStaging {
  void *h_dets = nullptr, *p_dets = nullptr, *h_embs = nullptr, *p_embs = nullptr;
  double *h_warp = nullptr, *p_warp = nullptr, *h_out = nullptr, *p_out = nullptr;
  int *h_off = nullptr, *h_cnt = nullptr, *p_cnt = nullptr, *p_sq = nullptr;
  int out_w = 8, sq_n = 0;

  // det_bytes / emb_bytes: one frame at full det_cap (emb_bytes 0: no embeddings); warp_n: the
  // warp's doubles (0: no warp); out_w: doubles per output row; sq_n: ints of the counter row
  int alloc(size_t det_bytes, size_t emb_bytes, int warp_n, int out_w_, int det_cap, int sq_n_) {
    out_w = out_w_;
    sq_n = sq_n_;
    const size_t out_bytes = sizeof(double) * out_w * det_cap;
    BX_HIPCHK(hipMalloc(&h_dets, det_bytes));
    BX_HIPCHK(hipHostMalloc(&p_dets, det_bytes));
    if (emb_bytes) {
      BX_HIPCHK(hipMalloc(&h_embs, emb_bytes));
      BX_HIPCHK(hipHostMalloc(&p_embs, emb_bytes));
    }
    if (warp_n) {
      BX_HIPCHK(hipMalloc(&h_warp, sizeof(double) * warp_n));
      BX_HIPCHK(hipHostMalloc(&p_warp, sizeof(double) * warp_n));
    }
    BX_HIPCHK(hipMalloc(&h_out, out_bytes));
    BX_HIPCHK(hipHostMalloc(&p_out, out_bytes));
    BX_HIPCHK(hipMalloc(&h_off, sizeof(int) * 2));
    BX_HIPCHK(hipMalloc(&h_cnt, sizeof(int)));
    BX_HIPCHK(hipHostMalloc(&p_cnt, sizeof(int) * 4));
    BX_HIPCHK(hipHostMalloc(&p_sq, sizeof(int) * sq_n));
    return BX_OK;
  }

  // safe on a half-allocated object, and twice
  void free() {
    void** dev[] = {&h_dets, &h_embs, (void**)&h_warp, (void**)&h_out, (void**)&h_off,
                    (void**)&h_cnt};
    void** pin[] = {&p_dets, &p_embs, (void**)&p_warp, (void**)&p_out, (void**)&p_cnt,
                    (void**)&p_sq};
    for (void** p : dev) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    for (void** p : pin) {
      if (*p) (void)hipHostFree(*p);
      *p = nullptr;
    }
  }

  // one input through its pinned mirror to its device buffer, on `st`
  int put(void* h, void* p, const void* src, size_t bytes, hipStream_t st) {
    memcpy(p, src, bytes);
    BX_HIPCHK(hipMemcpyAsync(h, p, bytes, hipMemcpyHostToDevice, st));
    return BX_OK;
  }
  // the frame's offsets {0, n}
  int put_off(int n, hipStream_t st) {
    p_cnt[2] = 0;
    p_cnt[3] = n;
    BX_HIPCHK(hipMemcpyAsync(h_off, p_cnt + 2, sizeof(int) * 2, hipMemcpyHostToDevice, st));
    return BX_OK;
  }
  // queue the copies back: count, status, the rows (at most n) and, if given, the counter row
  int take(const int* d_status, const int* d_sq, int n, hipStream_t st) {
    BX_HIPCHK(hipMemcpyAsync(p_cnt, h_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    BX_HIPCHK(hipMemcpyAsync(p_cnt + 1, d_status, sizeof(int), hipMemcpyDeviceToHost, st));
    if (n)
      BX_HIPCHK(hipMemcpyAsync(p_out, h_out, sizeof(double) * out_w * n, hipMemcpyDeviceToHost, st));
    if (d_sq) BX_HIPCHK(hipMemcpyAsync(p_sq, d_sq, sizeof(int) * sq_n, hipMemcpyDeviceToHost, st));
    return BX_OK;
  }
};
