/*
 * bxhybridsort.h — C ABI of the HybridSort engine in libbxassoc.so (MI355X, gfx950).
 *
 * Boundary: everything HybridSort.update(dets, img, embs) computes per frame once the ReID
 * embeddings are given — the 9-state / 5-measurement XYSR Kalman filter that also tracks the
 * detection score (predict, update, observation-centric re-update), the cosine distances of the
 * detection features to every track's smoothed feature and to the mean of its 30-deep feature
 * bank, the association on asso_func + four-corner direction consistency - score difference +
 * appearance, the long-term-ReID correction filter, the observation-centric recovery (OCR)
 * round, the feature moving average and bank, births, deaths and the output rows — runs on the
 * GPU behind these entry points.  One frame is three launches: the two distance contractions
 * (fp64 MFMA, a 4-wave workgroup per 32x64 tile), the frame (one wave64 workgroup per sequence)
 * and the feature update (a wave per record).
 *
 * Reference interfaces replaced (file:line in muntherr/boxmot):
 *   bx_hybrid_create/step/update_host  HybridSort.__init__ / HybridSort.update
 *                                      boxmot/trackers/hybridsort/hybridsort.py:372-741
 *     KalmanBoxTracker                 hybridsort.py:110-347
 *     KalmanFilterXYSR (ORU)           boxmot/motion/kalman_filters/aabb/xysr_kf.py:48-291
 *     associate_4_points_with_score_with_reid   hybridsort/association.py:537-644
 *     cost_vel                         hybridsort/association.py:328-349
 *     linear_assignment                hybridsort/association.py:312-325
 *   bx_hybrid_cosdist                  embedding_distance  hybridsort/association.py:734-751
 * The reference does not run as published; parity is defined against it with the patches H1-H3
 * listed in tests/golden/make_golden_hybridsort.py.  use_byte is not built.
 * The reference's ECC switch (False by default) is per sequence here: bx_hybrid_set_ecc_host and
 * the *_cmc entry points below carry the camera-motion warp.
 *
 * Conventions as in bxassoc.h: device pointers unless a name ends in _host, asynchronous on
 * `stream`, every function returns a bx_status (bx_last_error explains failures).
 */
#ifndef BXHYBRIDSORT_H
#define BXHYBRIDSORT_H

#include <stddef.h>
#include <stdint.h>

#include "bxassoc.h"
#include "bxclasses.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HybridSort constructor parameters (hybridsort.py:372-388: det_thresh has no default, max_age
 * 30, min_hits 3, iou_threshold .3, delta_t 3, inertia .2, longterm_reid_weight 0,
 * TCM_first_step_weight 0).  asso_kind and the frame size as in bx_ocsort_config.  emb_dim is
 * the embedding width F, any positive value.  det_thresh must be >= 0. */
typedef struct {
    int32_t n_seq;      /* independent sequences held by this engine */
    int32_t track_cap;  /* track slots per sequence (<= 512) */
    int32_t det_cap;    /* max detections per frame per sequence (<= 512) */
    int32_t emb_dim;
    double det_thresh, iou_threshold, inertia;
    double longterm_reid_weight, tcm_first_step_weight;
    int32_t max_age, min_hits, delta_t;
    int32_t asso_kind;
    double frame_w, frame_h;
} bx_hybrid_config;

/* The fields of bx_hybrid_config that size no memory and decide no launch: the ones a sequence
 * may have of its own (bx_hybrid_set_seq_params_host below).  n_seq, the caps, emb_dim and the
 * frame size stay engine-wide.  max_obs, which the create call derives from max_age (50, or
 * max_age + 5 from 50 on), follows a sequence's own max_age by the same rule; it is the only
 * field the create call derives from one of these (the filter's Q is constant). */
typedef struct {
    double det_thresh, iou_threshold, inertia;
    double longterm_reid_weight, tcm_first_step_weight;
    int32_t max_age, min_hits, delta_t;
    int32_t asso_kind;
} bx_hybrid_seq_params;

typedef struct bx_hybrid bx_hybrid;

int bx_hybrid_create(const bx_hybrid_config *cfg, bx_hybrid **out);
int bx_hybrid_destroy(bx_hybrid *e);
/* Forget all tracks of sequences [seq0, seq0+nseq): frame counter 0, id counter back to 1.  Their
 * per-sequence parameters, when set, stay. */
int bx_hybrid_reset(bx_hybrid *e, int seq0, int nseq, void *stream);
/* One frame for sequences [seq0, seq0+nseq) — three launches.
 *   dets    [sum N][6] float32 (x1,y1,x2,y2,conf,cls)
 *   det_off [nseq+1] int32 prefix offsets
 *   embs    [sum N][emb_dim] float64, one row per detection
 *   out     [sum N][8] float64 rows [x1,y1,x2,y2,id,conf,cls,det_ind], sequence k from row
 *           det_off[k], in the reference's (reversed track list) order; ids start at 1.  The
 *           reference reads cls and det_ind from the unfiltered frame at an index into the kept
 *           detections, and det_ind from its score column (hybridsort.py:458,467,604): column 7
 *           is a confidence
 *   out_count [nseq] int32 */
int bx_hybrid_step(bx_hybrid *e, int seq0, int nseq, const float *dets, const int32_t *det_off,
                   const double *embs, double *out, int32_t *out_count, void *stream);
/* Host-memory path for one sequence (the drop-in update): copies in, launches, copies out,
 * synchronises.  embs [n][emb_dim] (NULL only when n == 0); out must hold n rows. */
int bx_hybrid_update_host(bx_hybrid *e, int seq, const float *dets, int n, const double *embs,
                          double *out, int *n_out, void *stream);
/* per_class=True (bxclasses.h): one frame for sequences [seq0, seq0+nseq) of n_classes classes,
 * on an engine built with n_seq = S * n_classes (class c of sequence s is engine sequence
 * s * n_classes + c).  bx_hybrid_step's arguments with det_off / out / out_count per SEQUENCE (a
 * sequence has at most det_cap rows).  Runs class split -> the three launches over the class
 * sequences -> id merge on `stream`, nothing returning to the host; rows come out in class order
 * with class-global ids.  The first per-class call fixes n_classes: another value is
 * BX_ERR_INVALID.  A class whose births pass the id map's capacity latches BX_ERR_CAPACITY. */
int bx_hybrid_step_classes(bx_hybrid *e, int seq0, int nseq, int n_classes, const float *dets,
                           const int32_t *det_off, const double *embs, double *out,
                           int32_t *out_count, void *stream);
/* Build the class state before the first per-class call with an id map of map_cap births per
 * class sequence instead of BX_CLASSES_MAP_CAP. */
int bx_hybrid_classes_config(bx_hybrid *e, int n_classes, int map_cap);
/* The engine's class state (NULL before the first per-class call); it stays the engine's. */
int bx_hybrid_classes(bx_hybrid *e, bx_classes **out);
/* Host form of one per-class frame of sequence seq (the drop-in update): *id_count_host is the
 * class-level id counter, written to the device before the frame and read back after it.
 * Synchronises once. */
int bx_hybrid_update_classes_host(bx_hybrid *e, int seq, int n_classes, const float *dets_host,
                                  int n, const double *embs_host, int *id_count_host,
                                  double *out_host, int *n_out, void *stream);
/* Timing probe: while stage is 0 (distances), 1 (frame) or 2 (feature update), every step records
 * a HIP event pair around that launch; -1 turns it off.  probe_read synchronises and returns the
 * summed milliseconds and the number of pairs since the last read. */
int bx_hybrid_probe(bx_hybrid *e, int stage);
int bx_hybrid_probe_read(bx_hybrid *e, double *total_ms, int *count);
/* Capacity growth (the reference's track list is unbounded): copy every sequence's tracker
 * state of `src` into `dst`, a fresh engine with the same configuration and sequences and
 * track_cap / det_cap at least src's (slot ids stay valid).  Synchronous.  Tracks only: the
 * per-sequence parameter table is not copied. */
int bx_hybrid_copy_state(bx_hybrid *dst, bx_hybrid *src);
/* Per-sequence parameters, the contract of bx_ocsort_set_seq_params_host (bxocsort.h): a sweep
 * runs K configurations x S sequences as K*S sequences of ONE engine.  params_host [nseq] gives
 * sequences [seq0, seq0+nseq) parameters of their own; NULL clears the range, whose sequences then
 * run on the engine's parameters again.  Every entry is validated as the create call validates
 * the same fields (delta_t within the 8-slot observation ring, a known asso_kind, det_thresh >=
 * 0); an invalid entry, or a range outside [0, n_seq), returns BX_ERR_INVALID and changes
 * nothing.  The values live in a device table the frame kernel reads at its entry (uniform loads,
 * once per workgroup) and never writes; the distance and feature kernels read none of them.
 * Until the first set there is no table and the kernel runs as it always did.  Copies on
 * `stream`, then synchronises it.
 * The table is indexed by engine sequence: for a bx_hybrid_step_classes engine that is the class
 * sequence s * n_classes + c, and nothing more is promised there.
 * Meant for use between sequences, at frame 0 (after a reset): changing a sequence's parameters
 * while it holds tracks is allowed, but no reference behaviour is defined for it.  A reset keeps
 * the table; a state copy carries tracks only, so the destination keeps its own table (the
 * state blob of bx_hybrid_state_save_host carries tracks only too).
 * The second entry point reads a sequence's effective parameters back (its entry, or the
 * engine's when it has none); host memory, no device work. */
int bx_hybrid_set_seq_params_host(bx_hybrid *e, int seq0, int nseq,
                                  const bx_hybrid_seq_params *params_host, void *stream);
int bx_hybrid_seq_params_host(bx_hybrid *e, int seq, bx_hybrid_seq_params *out_host);
/* Camera-motion compensation: the reference's `ECC` attribute (hybridsort.py:417, 448-451;
 * KalmanBoxTracker.camera_update :237-249), DESIGN.md 2.28.
 *
 * bx_hybrid_set_ecc_host: on [nseq] (!= 0 switches on) for sequences [seq0, seq0+nseq).  Every
 * switch is off after create and after a reset of its sequence; bx_hybrid_copy_state carries the
 * switches and the skip counts (the state blob of bx_hybrid_state_save_host does not).  A range
 * outside [0, n_seq) or a null `on` is BX_ERR_INVALID and changes nothing.  Host, synchronous
 * (it synchronises the device first).  The first call that switches a sequence on allocates the
 * switches; from then on every frame of the engine has a fourth launch, the camera-update
 * kernel ahead of the frame kernel (one wave per sequence of the call; a sequence whose switch
 * is off leaves it after one uniform load).  Until then - and a call that only switches off on
 * such an engine changes nothing - a frame is the three launches it always was, of unchanged
 * kernels.  bx_hybrid_probe's stage 1 times the camera-update launch with the frame's.
 *
 * A sequence whose switch is on starts every frame with camera_update of every live track under
 * its warp, before the predict: state -> corner box (w = sqrt(x2 x4), h = x2 / w) -> the two
 * warped corners -> convert_bbox_to_z, in float64; x[0], x[1], x[2], x[4] are rewritten, the score
 * x[3], the covariance, the observations, the corner velocities and the features are not.  The
 * phase runs whenever the switch is on, under the identity too (the round trip is not the
 * identity in floating point).  A track whose state score is exactly 0 - where the reference
 * raises - is left as it was and counted.  A negative x2 x4 gives NaN, as numpy's does.
 *
 * The *_cmc entry points are bx_hybrid_step / update_host / step_classes / update_classes_host
 * plus the warps, which those call with NULL:
 *   warps      [nseq][6] float64 device, the row-major 2x3 affine per sequence of the call
 *              (step_classes: [nseq * n_classes][6], one per class sequence); NULL = identity
 *   warp_host  [6] host (update_host_cmc), warps_host [n_classes][6] host
 *              (update_classes_host_cmc); NULL = identity
 * Warps are read by sequences whose switch is on and ignored by the others.
 *
 * bx_hybrid_ecc_host: a sequence's switch and the number of tracks its camera updates left out
 * for a score of exactly 0 since the last reset (either pointer may be NULL).  Host; the switch
 * comes from the host mirror, and only a non-NULL count synchronises the device. */
int bx_hybrid_set_ecc_host(bx_hybrid *e, int seq0, int nseq, const int32_t *on);
int bx_hybrid_ecc_host(bx_hybrid *e, int seq, int *on, int *score_zero_skips);
int bx_hybrid_step_cmc(bx_hybrid *e, int seq0, int nseq, const float *dets,
                       const int32_t *det_off, const double *embs, const double *warps,
                       double *out, int32_t *out_count, void *stream);
int bx_hybrid_update_host_cmc(bx_hybrid *e, int seq, const float *dets, int n,
                              const double *embs, const double *warp_host, double *out,
                              int *n_out, void *stream);
int bx_hybrid_step_classes_cmc(bx_hybrid *e, int seq0, int nseq, int n_classes,
                               const float *dets, const int32_t *det_off, const double *embs,
                               const double *warps, double *out, int32_t *out_count,
                               void *stream);
int bx_hybrid_update_classes_host_cmc(bx_hybrid *e, int seq, int n_classes,
                                      const float *dets_host, int n, const double *embs_host,
                                      const double *warps_host, int *id_count_host,
                                      double *out_host, int *n_out, void *stream);
/* Latched device status (BX_OK, BX_ERR_TRACK_OVERFLOW or BX_ERR_CAPACITY). */
int bx_hybrid_status(bx_hybrid *e, int *status);
int bx_hybrid_counters_host(bx_hybrid *e, int seq, int *frame_count, int *id_count,
                            int *n_tracks);
/* KalmanBoxTracker.count is class-global in the reference (hybridsort.py:115,176-177,418); the
 * Python drop-in mirrors it through this. */
int bx_hybrid_set_id_count(bx_hybrid *e, int seq, int id_count, void *stream);
/* Frame size (w, h) of a sequence — BaseTracker latches img.shape on the first frame. */
int bx_hybrid_set_frame_size(bx_hybrid *e, int seq, double w, double h, void *stream);
/* Track list of a sequence in list order (host, synchronous): ids [cap], Kalman means x
 * [cap][9], covariances p [cap][81], smoothed features emb [cap][emb_dim], feature-bank means
 * bank_mean [cap][emb_dim], corner velocities vel [cap][8] (lt, rt, lb, rb as (y, x); zeros
 * while the reference holds None) and the number of features pushed into each bank so far,
 * bank_count [cap] (any may be NULL); *n = number of tracks. */
int bx_hybrid_tracks_host(bx_hybrid *e, int seq, int cap, int32_t *ids, double *x, double *p,
                          double *emb, double *bank_mean, double *vel, int32_t *bank_count,
                          int *n);
/* Write kf.x [n][9] / kf.P [n][81] of live tracks by id (host, synchronous; either may be
 * NULL).  BX_ERR_INVALID for an unknown id. */
int bx_hybrid_state_set_host(bx_hybrid *e, int seq, int n, const int32_t *ids, const double *x,
                             const double *p);
/* One sequence's whole tracker state (counters, list order, track records, smoothed features,
 * banks) as an opaque host blob of bx_hybrid_state_bytes bytes, and back into a sequence of an
 * engine with the same track_cap and emb_dim.  Host, synchronous. */
int bx_hybrid_state_bytes(bx_hybrid *e, size_t *bytes);
int bx_hybrid_state_save_host(bx_hybrid *e, int seq, void *blob, size_t bytes);
int bx_hybrid_state_load_host(bx_hybrid *e, int seq, const void *blob, size_t bytes);
/* Op-level distance on plain device arrays, the same tile code as the tracker's:
 * out [nd][nt] = max(0, 1 - d.t / (|d| |t|)) of dets_embs [nd][F] against trk_embs [nt][F],
 * float64 (the transpose of embedding_distance(tracks, dets)). */
int bx_hybrid_cosdist(int nd, int nt, int F, const double *dets_embs, const double *trk_embs,
                      double *out, void *stream);
/* Op-level bank mean, the tracker's own: bank [nt][30][F] feature rings (push k in row k % 30),
 * pushed [nt] pushes so far (> 0); out [nt][F] = mean of the rows present, oldest first. */
int bx_hybrid_bank_mean(int nt, int F, const double *bank, const int32_t *pushed, double *out,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BXHYBRIDSORT_H */
