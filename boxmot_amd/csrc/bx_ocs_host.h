// bx_ocs_host.h — the host side OCSort, DeepOCSort and HybridSort share, written once over the
// OcsDev view and the SQO counter row they all sit on: the LDS budget, the initial uploads, the
// counter reads (with the update_host cache), the list order, the track lookup of state_set and
// the update_host round trip.  The host counterpart of bx_ocs_device.h: included inside the
// including translation unit's anonymous namespace, after bx_ocs_device.h (the file includes
// bx_host.h itself, at file scope, before it).

// What the helpers need of an engine; each engine's handle derives from it, so a null handle
// arrives here as a null OcsHost and is refused with the entry point's usual message.
struct OcsHost {
  OcsDev* o = nullptr;  // the engine's OcsDev (its `dev`, or `dev.o`), set by its create
  BxStaging sg;         // update_host staging; sg.p_sq: the counter row of sequence cache_seq
  int cache_seq = -1;   // the sequence whose counters sg.p_sq holds (-1: none / stale)
};

// The frame kernel's LDS: the fixed part plus `extra` bytes the engine appends, plus as much cost
// matrix as keeps ~4 workgroups per CU resident.  Sets d.cost_lds; *x_off: where the engine's
// extra part starts; *total: the launch's dynamic LDS.
inline int ocs_lds_budget(OcsDev& d, size_t extra, size_t* x_off, size_t* total) {
  const size_t fixed = lds_bytes(d.D, d.T, d.N, 0) + extra;
  long budget = 40 * 1024 - (long)fixed;
  int cl = budget > 0 ? (int)(budget / 8) : 0;
  if (cl > d.D * d.T) cl = d.D * d.T;
  if (cl < 64) cl = 64;
  d.cost_lds = cl;
  *x_off = lds_bytes(d.D, d.T, d.N, cl);
  *total = *x_off + extra;
  if (*total > 160 * 1024)
    return bx_record_error(BX_ERR_INVALID, "track_cap/det_cap too large for one workgroup's LDS");
  return BX_OK;
}

// every sequence's frame size, and its first track id where that is not the arena's zero
inline int ocs_upload_initial(const OcsDev& d, double frame_w, double frame_h, int first_id) {
  const size_t S = d.S;
  std::vector<double> f(2 * S);
  for (size_t k = 0; k < S; k++) {
    f[2 * k] = frame_w;
    f[2 * k + 1] = frame_h;
  }
  BX_HIPCHK(hipMemcpy(d.fsz, f.data(), sizeof(double) * 2 * S, hipMemcpyHostToDevice));
  if (first_id) {
    std::vector<int> sq(S * SQO, 0);
    for (size_t k = 0; k < S; k++) sq[k * SQO + SO_IDS] = first_id;
    BX_HIPCHK(hipMemcpy(d.seqst, sq.data(), sizeof(int) * sq.size(), hipMemcpyHostToDevice));
  }
  return BX_OK;
}

// a sequence's counters: from the row the last update_host of that sequence brought back, else
// from the device
inline int ocs_counters(const OcsHost* h, int seq, int* frame_count, int* id_count,
                        int* n_tracks) {
  if (!h || seq < 0 || seq >= h->o->S) return bx_record_error(BX_ERR_INVALID, "bad sequence");
  int s[SQO];
  if (seq == h->cache_seq) {
    memcpy(s, h->sg.p_sq, sizeof(s));
  } else {
    BX_HIPCHK(hipDeviceSynchronize());
    BX_HIPCHK(hipMemcpy(s, h->o->seqst + (size_t)seq * SQO, sizeof(s), hipMemcpyDeviceToHost));
  }
  if (frame_count) *frame_count = s[SO_FRAME];
  if (id_count) *id_count = s[SO_IDS];
  if (n_tracks) *n_tracks = s[SO_NTR];
  return BX_OK;
}

inline int ocs_set_id_count(OcsHost* h, int seq, int id_count, void* stream) {
  if (!h || seq < 0 || seq >= h->o->S) return bx_record_error(BX_ERR_INVALID, "bad sequence");
  hipStream_t st = (hipStream_t)stream;
  h->cache_seq = -1;
  BX_HIPCHK(hipMemcpyAsync(h->o->seqst + (size_t)seq * SQO + SO_IDS, &id_count, sizeof(int),
                           hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  return BX_OK;
}

inline int ocs_set_frame_size(OcsHost* h, int seq, double fw, double fh, void* stream) {
  if (!h || seq < 0 || seq >= h->o->S) return bx_record_error(BX_ERR_INVALID, "bad sequence");
  hipStream_t st = (hipStream_t)stream;
  const double f[2] = {fw, fh};
  BX_HIPCHK(hipMemcpyAsync(h->o->fsz + 2 * (size_t)seq, f, sizeof(f), hipMemcpyHostToDevice, st));
  BX_HIPCHK(hipStreamSynchronize(st));
  return BX_OK;
}

// sums over [seq0, seq0 + nseq): live tracks, output rows; and the largest frame counter.
// `name`: the entry point, for the message
inline int ocs_frame_stats(const OcsHost* h, const char* name, int seq0, int nseq,
                           int64_t* sums) {
  if (!h || !sums || seq0 < 0 || nseq < 0 || seq0 + nseq > h->o->S)
    return bx_record_error(BX_ERR_INVALID, (std::string("bad arguments to ") + name).c_str());
  std::vector<int> s((size_t)nseq * SQO);
  BX_HIPCHK(hipDeviceSynchronize());
  if (nseq)
    BX_HIPCHK(hipMemcpy(s.data(), h->o->seqst + (size_t)seq0 * SQO, sizeof(int) * s.size(),
                        hipMemcpyDeviceToHost));
  int64_t t = 0, o = 0, f = 0;
  for (int k = 0; k < nseq; k++) {
    t += s[(size_t)k * SQO + SO_NTR];
    o += s[(size_t)k * SQO + SO_NOUT];
    f = s[(size_t)k * SQO + SO_FRAME] > f ? s[(size_t)k * SQO + SO_FRAME] : f;
  }
  sums[0] = t;
  sums[1] = o;
  sums[2] = f;
  return BX_OK;
}

// the list order of a sequence, on the host
inline int ocs_list_order(const OcsDev& d, int seq, std::vector<int>& ord) {
  BX_HIPCHK(hipDeviceSynchronize());
  int s[SQO];
  BX_HIPCHK(hipMemcpy(s, d.seqst + (size_t)seq * SQO, sizeof(s), hipMemcpyDeviceToHost));
  ord.resize(s[SO_NTR]);
  if (s[SO_NTR])
    BX_HIPCHK(hipMemcpy(ord.data(), d.order + (size_t)seq * d.T, sizeof(int) * s[SO_NTR],
                        hipMemcpyDeviceToHost));
  return BX_OK;
}

// state_set's lookup: the first listed track of the sequence with that id, read into `t`; *slot
// is its slot.  trk: the engine's [S][T] records.
template <class Trk>
int ocs_find_track(const OcsDev& d, Trk* trk, int seq, const std::vector<int>& ord, int id,
                   Trk& t, int* slot) {
  for (int k : ord) {
    BX_HIPCHK(hipMemcpy(&t, trk + (size_t)seq * d.T + k, sizeof(Trk), hipMemcpyDeviceToHost));
    if (t.id == id) {
      *slot = k;
      return BX_OK;
    }
  }
  return bx_record_error(BX_ERR_INVALID, "state_set: no live track with that id");
}

// the plain round trip's synchronisation (the class paths synchronise in cls_glue_take_ids)
struct OcsStreamSync {
  hipStream_t st;
  int operator()(int*) const {
    BX_HIPCHK(hipStreamSynchronize(st));
    return BX_OK;
  }
};

// One update_host frame: the detections through their pinned mirror, the offsets, the engine's
// launch(), then count, status, rows and the counter row back, sync(&class_status) — the one
// synchronisation — and the status mapped to an error.  The caller has checked its arguments and
// queued its own optional inputs (embeddings, warp, class ids) on `st`.
//   seq >= 0: a plain frame of that sequence; its counter row is cached for ocs_counters.
//   seq < 0:  a per-class frame: no counter row, the count clamped to [0, n], and the class
//             status sync() reports joins the mapping.
//   capacity_status: a latched BX_ERR_CAPACITY is reported as such (OCSort's own update path
//             reports every status as a slot overflow).
template <class Launch, class Sync>
int ocs_update_host_roundtrip(OcsHost& h, int seq, const float* dets, int n, double* out,
                              int* n_out, hipStream_t st, bool capacity_status, Launch launch,
                              Sync sync) {
  const OcsDev& d = *h.o;
  BxStaging& sg = h.sg;
  const bool cls = seq < 0;
  int rc;
  if (n && (rc = sg.put(sg.h_dets, sg.p_dets, dets, sizeof(float) * 6 * n, st))) return rc;
  if ((rc = sg.put_off(n, st))) return rc;
  h.cache_seq = -1;
  if ((rc = launch())) return rc;
  if ((rc = sg.take(d.status, cls ? nullptr : d.seqst + (size_t)seq * SQO, n, st))) return rc;
  int cstatus = 0;
  if ((rc = sync(&cstatus))) return rc;
  int cnt = sg.p_cnt[0];
  const int status = sg.p_cnt[1];
  if (cls)
    cnt = cnt > 0 && cnt <= n ? cnt : 0;
  else
    h.cache_seq = seq;
  if (cnt) memcpy(out, sg.p_out, sizeof(double) * 8 * cnt);
  *n_out = cnt;
  if (capacity_status && (status == BX_ERR_CAPACITY || cstatus == BX_ERR_CAPACITY))
    return bx_record_error(BX_ERR_CAPACITY,
                           cls ? "a sequence's detections exceeded det_cap, or a class's births "
                                 "its id map, on the device"
                               : "a sequence's detections exceeded det_cap on the device");
  if (status)
    return bx_record_error(BX_ERR_TRACK_OVERFLOW, "a sequence ran out of track slots (raise track_cap)");
  if (cstatus) return bx_record_error(cstatus, "the class merge met an id the engine never gave out");
  return BX_OK;
}
