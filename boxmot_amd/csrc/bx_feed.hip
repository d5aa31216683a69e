// bx_feed.hip — device-resident feeder of the many-sequence runner (include/bxfeed.h).
//
// Reference: the per-frame loop of process_sequence (boxmot/engine/val.py:304-354) over
// MOT17Sequence's mask selection (utils/dataloaders/MOT17.py:181-200) and convert_to_mot_format
// (engine/utils.py:101-133).  motio.run_sequences' default path does that assembly on the host
// for every run of sequences of every frame index; here the packed rows of all sequences live in
// HBM and two kernels per frame index do it:
//   feed_gather_kernel  one workgroup (4 waves) per sequence that has detections at the frame
//                       index: finds its run in the host-decided run table, sums the detection
//                       counts of the run's earlier sequences (its det_off entry), and copies
//                       its rows — contiguous in the packed arrays and in the run's batch — as
//                       flat 16-byte vector loads and stores (8-byte ones where source and
//                       destination differ in 16-byte phase: odd emb_dim)
//   feed_append_kernel  one workgroup per sequence: a thread per output row formats the MOT row
//                       and stores it behind the sequence's cursor; a row count that does not
//                       fit latches BX_ERR_CAPACITY and stores nothing
// Values are written with plain C++ and vector stores; everything runs on the caller's stream.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/bxfeed.h"
#include "bx_host.h"


namespace {

constexpr int FW = 256;  // threads per workgroup of both kernels (4 waves)
static_assert(BX_FEED_ROW_ALIGN * 48 % 256 == 0 && BX_FEED_ROW_ALIGN * 80 % 256 == 0,
              "float64 dets and 10-column out rows keep the run regions 256-byte aligned");

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

// One run of one frame index: sequences [k0, k1), its first row in the gathered arrays (a
// multiple of BX_FEED_ROW_ALIGN) and its first entry in the det_off array.
struct Run {
  int k0, k1, row0, off0;
};

struct FeedDev {
  int S, F;
  const long long* seq_row0;   // [S + 1] first packed row of each sequence in dets / embs
  const int* src;              // [S] the sequence whose packed rows sequence k gathers from
                               // (bx_feed_create_shared), or null: its own
  const long long* tab_off;    // [S + 1]
  const long long* row_start;  // [entries] within the sequence
  const int* row_cnt;          // [entries]
  const int* frame_id;         // [entries]
  const Run* runs;             // [all runs], frame index by frame index
  const float* dets;           // [R][6]
  const double* embs;          // [R][F]
  float* g_dets;               // gathered [stage_rows][6]
  double* g_embs;              // [stage_rows][F]
  int* g_off;                  // [off_cap]
  double* g_out;               // [stage_rows][8]
  int* g_cnt;                  // [S]
  double* res;                 // [res_rows][9]
  const long long* res_base;   // [S + 1]
  long long* res_n;            // [S]
  int* status;
  double* g_dets64;            // gathered [stage_rows][6] of the float64 mode (g_dets is null)
};

// detections of sequence k at frame index t (0 past its last frame) and the table entry
__device__ __forceinline__ int feed_cnt(const FeedDev& d, int k, int t, long long* entry) {
  const long long a = d.tab_off[k], b = d.tab_off[k + 1];
  if (t >= b - a) return 0;
  if (entry) *entry = a + t;
  return d.row_cnt[a + t];
}

// the run of frame-table slice [runs, runs + n) that holds sequence k (k0 ascending); -1: none
__device__ __forceinline__ int feed_find_run(const Run* runs, int n, int k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (runs[mid].k1 <= k) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && runs[lo].k0 <= k) ? lo : -1;
}

// n elements of T from src to dst, both sizeof(T)-aligned: V-wide (2 T) where both are
// V-aligned after the same head, otherwise element by element
template <class T, class V>
__device__ __forceinline__ void feed_copy(T* __restrict__ dst, const T* __restrict__ src,
                                          long long n, int tid) {
  const uintptr_t ms = (uintptr_t)src & (sizeof(V) - 1), md = (uintptr_t)dst & (sizeof(V) - 1);
  if (ms != md) {
    for (long long i = tid; i < n; i += FW) dst[i] = src[i];
    return;
  }
  const long long head = ms ? (n < 1 ? n : 1) : 0;  // one element reaches the V boundary
  if (tid == 0 && head) dst[0] = src[0];
  const long long nv = (n - head) / 2;
  const V* s = (const V*)(src + head);
  V* o = (V*)(dst + head);
  for (long long i = tid; i < nv; i += FW) o[i] = s[i];
  const long long done = head + 2 * nv;
  if (tid == 0 && done < n) dst[done] = src[done];
}

// F64 (bx_feed_create_shared_fmt's det_f64): the run's dets are written as float64, each value
// the exact widening of the packed float32 (what numpy's astype(float64) gives)
template <bool F64>
__global__ void __launch_bounds__(FW)
feed_gather_kernel(FeedDev d, int t, int run_first, int n_runs) {
  const int k = blockIdx.x, tid = threadIdx.x;
  long long entry = 0;
  const int n = feed_cnt(d, k, t, &entry);
  if (n <= 0) return;  // (uniform over the workgroup)
  const Run* runs = d.runs + run_first;
  const int r = feed_find_run(runs, n_runs, k);
  if (r < 0) return;
  const Run run = runs[r];
  // det_off entry: detections of the run's sequences before k
  __shared__ int part[FW / 64];
  int s = 0;
  for (int q = run.k0 + tid; q < k; q += FW) s += feed_cnt(d, q, t, nullptr);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < FW / 64; w++) before += part[w];
  if (tid == 0) {
    d.g_off[run.off0 + (k - run.k0)] = before;
    if (k == run.k1 - 1) d.g_off[run.off0 + (run.k1 - run.k0)] = before + n;
  }
  const long long src = d.seq_row0[d.src ? d.src[k] : k] + d.row_start[entry];
  const long long dst = (long long)run.row0 + before;
  if constexpr (F64) {
    // both sides 8-byte aligned (6 floats a row, 6 doubles a row): a float pair in, a double
    // pair out
    const f2* s2 = (const f2*)(d.dets + src * 6);
    d2* o2 = (d2*)(d.g_dets64 + dst * 6);
    for (long long i = tid; i < (long long)n * 3; i += FW) {
      const f2 v = s2[i];
      d2 w;
      w.x = (double)v.x;
      w.y = (double)v.y;
      o2[i] = w;
    }
  } else {
    feed_copy<float, f2>(d.g_dets + dst * 6, d.dets + src * 6, (long long)n * 6, tid);
  }
  if (d.F) feed_copy<double, d2>(d.g_embs + dst * d.F, d.embs + src * d.F, (long long)n * d.F, tid);
}

// OC: columns of the steps' out rows (8, or 10 for StrongSort's, whose first 8 are the same)
template <int OC>
__global__ void __launch_bounds__(FW)
feed_append_kernel(FeedDev d, int t, int run_first, int n_runs) {
  const int k = blockIdx.x, tid = threadIdx.x;
  long long entry = 0;
  const int n = feed_cnt(d, k, t, &entry);
  if (n <= 0) return;
  const Run* runs = d.runs + run_first;
  const int r = feed_find_run(runs, n_runs, k);
  if (r < 0) return;
  const Run run = runs[r];
  const int c = d.g_cnt[k];
  const long long have = d.res_n[k], cap = d.res_base[k + 1] - d.res_base[k];
  if (c < 0 || c > n || have + c > cap) {
    if (tid == 0) atomicMax(d.status, (int)BX_ERR_CAPACITY);
    return;
  }
  const double* out = d.g_out + ((long long)run.row0 + d.g_off[run.off0 + (k - run.k0)]) * OC;
  double* res = d.res + (d.res_base[k] + have) * 9;
  const double fid = (double)d.frame_id[entry];
  for (int i = tid; i < c; i += FW) {
    const double* r8 = out + (long long)i * OC;
    // ops.xyxy2ltwh: [x1, y1, x2 - x1, y2 - y1]; .round() half-to-even; astype(int32)
    const double l = r8[0], tp = r8[1], w = r8[2] - r8[0], h = r8[3] - r8[1];
    double* o = res + (long long)i * 9;
    o[0] = fid;
    o[1] = (double)(int)r8[4];
    o[2] = (double)(int)rint(l);
    o[3] = (double)(int)rint(tp);
    o[4] = (double)(int)rint(w);
    o[5] = (double)(int)rint(h);
    o[6] = 1.0;
    o[7] = (double)(int)r8[6];
    o[8] = r8[5];
  }
  __syncthreads();  // every thread has read the cursor
  if (tid == 0) d.res_n[k] = have + c;
}

}  // namespace

struct bx_feed {
  FeedDev dev{};
  int S = 0, F = 0, T = 0, max_runs = 0;
  std::vector<long long> seq_row0, tab_off, res_base;
  std::vector<int> src;       // bx_feed_create_shared's map (empty: every sequence its own source)
  size_t device_bytes = 0;
  std::vector<Run> runs;
  std::vector<int> run_off;   // [T + 1] into runs
  std::vector<int> run_rows;  // detections of each run
  long long res_rows = 0;
  std::vector<void*> allocs;
  int det_f64 = 0, out_cols = 8;  // bx_feed_create_shared_fmt's mode
};

static void feed_free(bx_feed* f) {
  for (void* p : f->allocs) (void)hipFree(p);
  delete f;
}

static int feed_run_of(bx_feed* f, int t, int r, int* idx) {
  if (!f) return bx_record_error(BX_ERR_INVALID, "null feeder");
  if (t < 0 || t >= f->T) return bx_record_error(BX_ERR_INVALID, "frame index out of range");
  if (r < 0 || r >= f->run_off[t + 1] - f->run_off[t])
    return bx_record_error(BX_ERR_INVALID, "run out of range");
  *idx = f->run_off[t] + r;
  return BX_OK;
}

// bx_feed_create (src_map null: every sequence owns its rows) and bx_feed_create_shared
static int feed_create(int n_seq, int emb_dim, const int64_t* seq_rows, const int64_t* tab_off,
                       const int64_t* row_start, const int32_t* row_cnt, const int32_t* frame_id,
                       const int64_t* res_cap, int guard_rows, const int32_t* src_map,
                       int det_f64, int out_cols, bx_feed** out) {
  if (!out || !seq_rows || !tab_off) return bx_record_error(BX_ERR_INVALID, "null argument");
  if ((det_f64 != 0 && det_f64 != 1) || (out_cols != 8 && out_cols != 10))
    return bx_record_error(BX_ERR_INVALID, "det_f64 must be 0 or 1 and out_cols 8 or 10");
  if (n_seq <= 0 || emb_dim < 0 || guard_rows < 0)
    return bx_record_error(BX_ERR_INVALID, "n_seq/emb_dim/guard_rows out of range");
  const int S = n_seq;
  if (tab_off[0] != 0) return bx_record_error(BX_ERR_INVALID, "tab_off must start at 0");
  long long T = 0;
  for (int k = 0; src_map && k < S; k++) {
    const int q = src_map[k];
    if (q < 0 || q > k || src_map[q] != q)
      return bx_record_error(BX_ERR_INVALID, "src must satisfy src[k] <= k and src[src[k]] == src[k]");
  }
  for (int k = 0; k < S; k++) {  // (seq_rows of a sequence that reads another's rows is not read)
    const bool own = !src_map || src_map[k] == k;
    if (tab_off[k + 1] < tab_off[k] || (own && seq_rows[k] < 0))
      return bx_record_error(BX_ERR_INVALID, "tab_off must ascend and seq_rows be non-negative");
    if (tab_off[k + 1] - tab_off[k] > T) T = tab_off[k + 1] - tab_off[k];
  }
  const long long E = tab_off[S];
  if (E && (!row_start || !row_cnt || !frame_id))
    return bx_record_error(BX_ERR_INVALID, "null frame table");
  if (T >= (1LL << 31)) return bx_record_error(BX_ERR_INVALID, "too many frame indices");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return bx_record_error(BX_ERR_NO_DEVICE, "no HIP device visible");
  bx_feed* f = new bx_feed();
  f->S = S;
  f->F = emb_dim;
  f->T = (int)T;
  f->seq_row0.assign(S + 1, 0);
  f->tab_off.assign(tab_off, tab_off + S + 1);
  f->res_base.assign(S + 1, 0);
  if (src_map) f->src.assign(src_map, src_map + S);
  f->det_f64 = det_f64;
  f->out_cols = out_cols;
  auto fill = [&]() -> int {
    for (int k = 0; k < S; k++) {
      // only a source sequence owns packed rows; the others read their source's
      const int q = src_map ? src_map[k] : k;
      f->seq_row0[k + 1] = f->seq_row0[k] + (q == k ? seq_rows[k] : 0);
      long long total = 0;
      for (long long e = tab_off[k]; e < tab_off[k + 1]; e++) {
        if (row_cnt[e] < 0 || row_start[e] < 0 || row_start[e] + row_cnt[e] > seq_rows[q])
          return bx_record_error(BX_ERR_INVALID, "a frame table entry reaches outside its sequence");
        total += row_cnt[e];
      }
      const long long cap = res_cap ? res_cap[k] : total;
      if (cap < 0) return bx_record_error(BX_ERR_INVALID, "negative result capacity");
      f->res_base[k + 1] = f->res_base[k] + cap;
    }
    f->res_rows = f->res_base[S] + guard_rows;
    // the schedule: per frame index the maximal ranges of sequences that have detections
    long long stage_rows = 0, off_cap = 0;
    f->run_off.assign(f->T + 1, 0);
    for (int t = 0; t < f->T; t++) {
      long long row = 0, off = 0;
      int k = 0;
      auto cnt = [&](int q) -> long long {
        return t < tab_off[q + 1] - tab_off[q] ? row_cnt[tab_off[q] + t] : 0;
      };
      while (k < S) {
        if (cnt(k) == 0) {
          k++;
          continue;
        }
        int k1 = k;
        long long rows = 0;
        while (k1 < S && cnt(k1) != 0) rows += cnt(k1++);
        if (row + rows >= (1LL << 31) || rows >= (1LL << 31))
          return bx_record_error(BX_ERR_CAPACITY, "a frame index has 2^31 detections or more");
        f->runs.push_back(Run{k, k1, (int)row, (int)off});
        f->run_rows.push_back((int)rows);
        row += (rows + BX_FEED_ROW_ALIGN - 1) / BX_FEED_ROW_ALIGN * BX_FEED_ROW_ALIGN;
        off += k1 - k + 1;
        k = k1;
      }
      f->run_off[t + 1] = (int)f->runs.size();
      const int nr = f->run_off[t + 1] - f->run_off[t];
      if (nr > f->max_runs) f->max_runs = nr;
      if (row > stage_rows) stage_rows = row;
      if (off > off_cap) off_cap = off;
    }
    if (stage_rows >= (1LL << 31))
      return bx_record_error(BX_ERR_CAPACITY, "a frame index has 2^31 detections or more");
    FeedDev& d = f->dev;
    d.S = S;
    d.F = emb_dim;
    auto dev_alloc = [&](void** p, size_t bytes) -> int {
      *p = nullptr;
      BX_HIPCHK(hipMalloc(p, bytes ? bytes : 256));
      f->allocs.push_back(*p);
      f->device_bytes += bytes ? bytes : 256;
      return BX_OK;
    };
    auto dev_put = [&](const void** p, const void* src, size_t bytes) -> int {
      void* q = nullptr;
      int rc = dev_alloc(&q, bytes);
      if (rc) return rc;
      if (bytes) BX_HIPCHK(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice));
      *p = q;
      return BX_OK;
    };
    int rc;
    const long long R = f->seq_row0[S];
    if ((rc = dev_put((const void**)&d.seq_row0, f->seq_row0.data(), sizeof(long long) * (S + 1)))) return rc;
    if (src_map && (rc = dev_put((const void**)&d.src, src_map, sizeof(int) * S))) return rc;
    if ((rc = dev_put((const void**)&d.tab_off, tab_off, sizeof(long long) * (S + 1)))) return rc;
    if ((rc = dev_put((const void**)&d.row_start, row_start, sizeof(long long) * E))) return rc;
    if ((rc = dev_put((const void**)&d.row_cnt, row_cnt, sizeof(int) * E))) return rc;
    if ((rc = dev_put((const void**)&d.frame_id, frame_id, sizeof(int) * E))) return rc;
    if ((rc = dev_put((const void**)&d.runs, f->runs.data(), sizeof(Run) * f->runs.size()))) return rc;
    if ((rc = dev_put((const void**)&d.res_base, f->res_base.data(), sizeof(long long) * (S + 1)))) return rc;
    if ((rc = dev_alloc((void**)&d.dets, sizeof(float) * 6 * R))) return rc;
    if ((rc = dev_alloc((void**)&d.embs, sizeof(double) * emb_dim * R))) return rc;
    if (det_f64) {
      if ((rc = dev_alloc((void**)&d.g_dets64, sizeof(double) * 6 * stage_rows))) return rc;
    } else {
      if ((rc = dev_alloc((void**)&d.g_dets, sizeof(float) * 6 * stage_rows))) return rc;
    }
    if ((rc = dev_alloc((void**)&d.g_embs, sizeof(double) * emb_dim * stage_rows))) return rc;
    if ((rc = dev_alloc((void**)&d.g_off, sizeof(int) * off_cap))) return rc;
    if ((rc = dev_alloc((void**)&d.g_out, sizeof(double) * out_cols * stage_rows))) return rc;
    if ((rc = dev_alloc((void**)&d.g_cnt, sizeof(int) * S))) return rc;
    if ((rc = dev_alloc((void**)&d.res, sizeof(double) * 9 * f->res_rows))) return rc;
    if ((rc = dev_alloc((void**)&d.res_n, sizeof(long long) * S))) return rc;
    if ((rc = dev_alloc((void**)&d.status, 256))) return rc;
    BX_HIPCHK(hipMemset(d.res, 0xFF, sizeof(double) * 9 * f->res_rows));
    BX_HIPCHK(hipMemset(d.res_n, 0, sizeof(long long) * S));
    BX_HIPCHK(hipMemset(d.g_cnt, 0, sizeof(int) * S));
    BX_HIPCHK(hipMemset(d.status, 0, 256));
    BX_HIPCHK(hipDeviceSynchronize());
    return BX_OK;
  };
  const int rc = fill();
  if (rc) {
    feed_free(f);
    return rc;
  }
  *out = f;
  return BX_OK;
}

extern "C" {

int bx_feed_create(int n_seq, int emb_dim, const int64_t* seq_rows, const int64_t* tab_off,
                   const int64_t* row_start, const int32_t* row_cnt, const int32_t* frame_id,
                   const int64_t* res_cap, int guard_rows, bx_feed** out) {
  return feed_create(n_seq, emb_dim, seq_rows, tab_off, row_start, row_cnt, frame_id, res_cap,
                     guard_rows, nullptr, 0, 8, out);
}

int bx_feed_create_shared(int n_seq, int emb_dim, const int64_t* seq_rows, const int64_t* tab_off,
                          const int64_t* row_start, const int32_t* row_cnt,
                          const int32_t* frame_id, const int64_t* res_cap, int guard_rows,
                          const int32_t* src, bx_feed** out) {
  if (!src || n_seq <= 0) return bx_record_error(BX_ERR_INVALID, "null argument");
  return feed_create(n_seq, emb_dim, seq_rows, tab_off, row_start, row_cnt, frame_id, res_cap,
                     guard_rows, src, 0, 8, out);
}

int bx_feed_create_shared_fmt(int n_seq, int emb_dim, const int64_t* seq_rows,
                              const int64_t* tab_off, const int64_t* row_start,
                              const int32_t* row_cnt, const int32_t* frame_id,
                              const int64_t* res_cap, int guard_rows, const int32_t* src,
                              int det_f64, int out_cols, bx_feed** out) {
  if (!src || n_seq <= 0) return bx_record_error(BX_ERR_INVALID, "null argument");
  return feed_create(n_seq, emb_dim, seq_rows, tab_off, row_start, row_cnt, frame_id, res_cap,
                     guard_rows, src, det_f64, out_cols, out);
}

int bx_feed_device_bytes(bx_feed* f, int64_t* bytes) {
  if (!f || !bytes) return bx_record_error(BX_ERR_INVALID, "null argument");
  *bytes = (int64_t)f->device_bytes;
  return BX_OK;
}

int bx_feed_destroy(bx_feed* f) {
  if (f) feed_free(f);
  return BX_OK;
}

int bx_feed_upload_host(bx_feed* f, int seq, const float* dets, const double* embs) {
  if (!f || seq < 0 || seq >= f->S) return bx_record_error(BX_ERR_INVALID, "bad feeder or sequence");
  if (!f->src.empty() && f->src[seq] != seq)
    return bx_record_error(BX_ERR_INVALID, "the sequence reads another sequence's rows: upload to its source");
  const long long r0 = f->seq_row0[seq], n = f->seq_row0[seq + 1] - r0;
  if (n == 0) return BX_OK;
  if (!dets || (f->F && !embs)) return bx_record_error(BX_ERR_INVALID, "null rows");
  BX_HIPCHK(hipMemcpy((float*)f->dev.dets + r0 * 6, dets, sizeof(float) * 6 * n, hipMemcpyHostToDevice));
  if (f->F)
    BX_HIPCHK(hipMemcpy((double*)f->dev.embs + r0 * f->F, embs, sizeof(double) * f->F * n,
                   hipMemcpyHostToDevice));
  return BX_OK;
}

int bx_feed_shape(bx_feed* f, int* n_frames, int* max_runs) {
  if (!f) return bx_record_error(BX_ERR_INVALID, "null feeder");
  if (n_frames) *n_frames = f->T;
  if (max_runs) *max_runs = f->max_runs;
  return BX_OK;
}

int bx_feed_frame_runs(bx_feed* f, int t, int* n_runs) {
  if (!f || !n_runs) return bx_record_error(BX_ERR_INVALID, "null argument");
  if (t < 0 || t >= f->T) return bx_record_error(BX_ERR_INVALID, "frame index out of range");
  *n_runs = f->run_off[t + 1] - f->run_off[t];
  return BX_OK;
}

int bx_feed_run(bx_feed* f, int t, int r, int* seq0, int* nseq, int* rows, void** dets,
                void** det_off, void** embs, void** out, void** out_count) {
  int i, rc;
  if ((rc = feed_run_of(f, t, r, &i))) return rc;
  const Run& u = f->runs[i];
  const FeedDev& d = f->dev;
  if (seq0) *seq0 = u.k0;
  if (nseq) *nseq = u.k1 - u.k0;
  if (rows) *rows = f->run_rows[i];
  if (dets)
    *dets = f->det_f64 ? (void*)(d.g_dets64 + (size_t)u.row0 * 6)
                       : (void*)(d.g_dets + (size_t)u.row0 * 6);
  if (det_off) *det_off = d.g_off + u.off0;
  if (embs) *embs = f->F ? d.g_embs + (size_t)u.row0 * f->F : nullptr;
  if (out) *out = d.g_out + (size_t)u.row0 * f->out_cols;
  if (out_count) *out_count = d.g_cnt + u.k0;
  return BX_OK;
}

int bx_feed_gather(bx_feed* f, int t, void* stream) {
  if (!f) return bx_record_error(BX_ERR_INVALID, "null feeder");
  if (t < 0 || t >= f->T) return bx_record_error(BX_ERR_INVALID, "frame index out of range");
  const int nr = f->run_off[t + 1] - f->run_off[t];
  if (nr == 0) return BX_OK;
  if (f->det_f64)
    hipLaunchKernelGGL(feed_gather_kernel<true>, dim3(f->S), dim3(FW), 0, (hipStream_t)stream,
                       f->dev, t, f->run_off[t], nr);
  else
    hipLaunchKernelGGL(feed_gather_kernel<false>, dim3(f->S), dim3(FW), 0, (hipStream_t)stream, f->dev, t,
                     f->run_off[t], nr);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_feed_append(bx_feed* f, int t, void* stream) {
  if (!f) return bx_record_error(BX_ERR_INVALID, "null feeder");
  if (t < 0 || t >= f->T) return bx_record_error(BX_ERR_INVALID, "frame index out of range");
  const int nr = f->run_off[t + 1] - f->run_off[t];
  if (nr == 0) return BX_OK;
  if (f->out_cols == 10)
    hipLaunchKernelGGL(feed_append_kernel<10>, dim3(f->S), dim3(FW), 0, (hipStream_t)stream,
                       f->dev, t, f->run_off[t], nr);
  else
    hipLaunchKernelGGL(feed_append_kernel<8>, dim3(f->S), dim3(FW), 0, (hipStream_t)stream, f->dev, t,
                     f->run_off[t], nr);
  BX_HIPCHK(hipGetLastError());
  return BX_OK;
}

int bx_feed_status(bx_feed* f, int* status) {
  if (!f || !status) return bx_record_error(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipDeviceSynchronize());
  BX_HIPCHK(hipMemcpy(status, f->dev.status, sizeof(int), hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_feed_result_rows(bx_feed* f, int64_t* rows) {
  if (!f || !rows) return bx_record_error(BX_ERR_INVALID, "null argument");
  *rows = f->res_rows;
  return BX_OK;
}

int bx_feed_results_host(bx_feed* f, double* res, int64_t* base, int64_t* n) {
  if (!f || !base || !n || (f->res_rows && !res))
    return bx_record_error(BX_ERR_INVALID, "null argument");
  BX_HIPCHK(hipDeviceSynchronize());
  if (f->res_rows)
    BX_HIPCHK(hipMemcpy(res, f->dev.res, sizeof(double) * 9 * f->res_rows, hipMemcpyDeviceToHost));
  static_assert(sizeof(long long) == sizeof(int64_t), "int64 layout");
  BX_HIPCHK(hipMemcpy(n, f->dev.res_n, sizeof(int64_t) * f->S, hipMemcpyDeviceToHost));
  for (int k = 0; k <= f->S; k++) base[k] = f->res_base[k];
  return BX_OK;
}

int bx_feed_results_device(bx_feed* f, void** res, void** base, void** n, int64_t* rows) {
  if (!f || !res || !base || !n || !rows) return bx_record_error(BX_ERR_INVALID, "null argument");
  *res = f->dev.res;
  *base = (void*)f->dev.res_base;
  *n = f->dev.res_n;
  *rows = f->res_rows;
  return BX_OK;
}

int bx_feed_read_run_host(bx_feed* f, int t, int r, void* dets, int32_t* det_off, double* embs) {
  int i, rc;
  if ((rc = feed_run_of(f, t, r, &i))) return rc;
  const Run& u = f->runs[i];
  const FeedDev& d = f->dev;
  const size_t rows = (size_t)f->run_rows[i];
  BX_HIPCHK(hipDeviceSynchronize());
  if (dets && f->det_f64)
    BX_HIPCHK(hipMemcpy(dets, d.g_dets64 + (size_t)u.row0 * 6, sizeof(double) * 6 * rows,
                        hipMemcpyDeviceToHost));
  else if (dets)
    BX_HIPCHK(hipMemcpy(dets, d.g_dets + (size_t)u.row0 * 6, sizeof(float) * 6 * rows,
                   hipMemcpyDeviceToHost));
  if (det_off)
    BX_HIPCHK(hipMemcpy(det_off, d.g_off + u.off0, sizeof(int) * (u.k1 - u.k0 + 1),
                   hipMemcpyDeviceToHost));
  if (embs && f->F)
    BX_HIPCHK(hipMemcpy(embs, d.g_embs + (size_t)u.row0 * f->F, sizeof(double) * f->F * rows,
                   hipMemcpyDeviceToHost));
  return BX_OK;
}

int bx_feed_write_run_host(bx_feed* f, int t, int r, const double* out, const int32_t* out_count) {
  int i, rc;
  if ((rc = feed_run_of(f, t, r, &i))) return rc;
  if (!out || !out_count) return bx_record_error(BX_ERR_INVALID, "null argument");
  const Run& u = f->runs[i];
  const FeedDev& d = f->dev;
  BX_HIPCHK(hipDeviceSynchronize());
  const size_t oc = (size_t)f->out_cols;
  BX_HIPCHK(hipMemcpy(d.g_out + (size_t)u.row0 * oc, out, sizeof(double) * oc * (size_t)f->run_rows[i],
                 hipMemcpyHostToDevice));
  BX_HIPCHK(hipMemcpy(d.g_cnt + u.k0, out_count, sizeof(int) * (u.k1 - u.k0), hipMemcpyHostToDevice));
  return BX_OK;
}

}  // extern "C"
