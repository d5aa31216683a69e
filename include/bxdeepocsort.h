/*
 * bxdeepocsort.h — C ABI of the DeepOCSort engine in libbxassoc.so (MI355X, gfx950).
 *
 * Boundary: everything DeepOcSort.update(dets, img, embs) computes per frame once the ReID
 * embeddings and the camera-motion warp are given — the affine correction of every track (live
 * state, frozen snapshot, last observation and observation ring), the XYSR Kalman predict and
 * update with the observation-centric re-update (ORU), the appearance contraction
 * dets_embs @ trk_embs.T, the association on IoU + direction consistency + the (adaptively
 * weighted) appearance term, the observation-centric recovery (OCR) round, the embedding moving
 * average, births, deaths and the output rows — runs on the GPU behind these entry points.  One
 * frame is three launches: the contraction (fp64 MFMA, a 4-wave workgroup per 32x64 tile), the
 * frame (one wave64 workgroup per sequence) and the embedding update (a wave per record).
 *
 * Reference interfaces replaced (file:line in muntherr/boxmot):
 *   bx_deepoc_create/step/update_host  DeepOcSort.__init__ / DeepOcSort.update
 *                                      boxmot/trackers/deepocsort/deepocsort.py:265-498
 *     KalmanBoxTracker                 deepocsort.py:51-235
 *       apply_affine_correction        deepocsort.py:191-208
 *       update_emb                     deepocsort.py:184-186
 *     KalmanFilterXYSR (ORU)           boxmot/motion/kalman_filters/aabb/xysr_kf.py:48-291
 *       apply_affine_correction        xysr_kf.py:111-135
 *     associate (enhanced)             boxmot/utils/association.py:377-556
 *     compute_aw_max_metric            boxmot/utils/association.py:320-374
 *     linear_assignment (legacy lapx)  boxmot/utils/association.py:105-114
 *   bx_deepoc_embcost                  dets_embs @ trk_embs.T            deepocsort.py:397
 * The association follows the reference with the patches P1-P5 of SURVEY.md Appendix A, as the
 * OCSort engine does; the tests/golden/deepoc_*.npz fixtures are captured from the reference
 * patched that way.  Embeddings cross this ABI as float64 (see DESIGN.md 2.9 for what that
 * leaves out of the reference's mixed-width behaviour).
 *
 * Conventions as in bxassoc.h: device pointers unless a name ends in _host, asynchronous on
 * `stream`, every function returns a bx_status (bx_last_error explains failures).
 */
#ifndef BXDEEPOCSORT_H
#define BXDEEPOCSORT_H

#include <stdint.h>

#include "bxassoc.h"
#include "bxclasses.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DeepOcSort constructor parameters (deepocsort.py:265-287: det_thresh .3, max_age 30, min_hits 3,
 * iou_threshold .3, delta_t 3, inertia .2, w_association_emb .5, alpha_fixed_emb .95, aw_param
 * .5, embedding_off 0, aw_off 0, Q_xy_scaling .01, Q_s_scaling 1e-4).  asso_kind and the frame
 * size as in bx_ocsort_config.  emb_dim is the embedding width F, any positive value (ignored
 * when embedding_off is set). */
typedef struct {
    int32_t n_seq;      /* independent sequences held by this engine */
    int32_t track_cap;  /* track slots per sequence (<= 512) */
    int32_t det_cap;    /* max detections per frame per sequence (<= 512) */
    int32_t emb_dim;
    double det_thresh, iou_threshold, inertia, q_xy_scaling, q_s_scaling;
    double w_association_emb, alpha_fixed_emb, aw_param;
    int32_t max_age, min_hits, delta_t;
    int32_t embedding_off, aw_off;
    int32_t asso_kind;
    double frame_w, frame_h;
} bx_deepoc_config;

/* The fields of bx_deepoc_config that size no memory and decide no launch: the ones a sequence
 * may have of its own (bx_deepoc_set_seq_params_host below).  embedding_off stays engine-wide (it
 * decides emb_dim, the contraction launch and the feature launch), as do n_seq, the caps, emb_dim
 * and the frame size.  max_obs, which the create call derives from max_age (50, or max_age + 5
 * from 50 on), follows a sequence's own max_age by the same rule. */
typedef struct {
    double det_thresh, iou_threshold, inertia, q_xy_scaling, q_s_scaling;
    double w_association_emb, alpha_fixed_emb, aw_param;
    int32_t max_age, min_hits, delta_t;
    int32_t aw_off;
    int32_t asso_kind;
} bx_deepoc_seq_params;

typedef struct bx_deepoc bx_deepoc;

int bx_deepoc_create(const bx_deepoc_config *cfg, bx_deepoc **out);
int bx_deepoc_destroy(bx_deepoc *e);
/* Forget all tracks of sequences [seq0, seq0+nseq): frame counter 0, id counter back to 1
 * (KalmanBoxTracker.count = 1, deepocsort.py:305).  Their per-sequence parameters, when set,
 * stay. */
int bx_deepoc_reset(bx_deepoc *e, int seq0, int nseq, void *stream);
/* One frame for sequences [seq0, seq0+nseq) — three launches (two with embedding_off).
 *   dets    [sum N][6] float32 (x1,y1,x2,y2,conf,cls)
 *   det_off [nseq+1] int32 prefix offsets
 *   embs    [sum N][emb_dim] float64, one row per detection (NULL with embedding_off)
 *   warps   [nseq][6] float64 row-major 2x3 CMC affines, NULL = identity (cmc_off)
 *   out     [sum N][8] float64 rows [x1,y1,x2,y2,id,conf,cls,det_ind], sequence k from row
 *           det_off[k], in the reference's (reversed track list) order; ids start at 1
 *   out_count [nseq] int32 */
int bx_deepoc_step(bx_deepoc *e, int seq0, int nseq, const float *dets, const int32_t *det_off,
                   const double *embs, const double *warps, double *out, int32_t *out_count,
                   void *stream);
/* Host-memory path for one sequence (the drop-in update): copies in, launches, copies out,
 * synchronises.  embs [n][emb_dim] or NULL (embedding_off / n == 0), warp [6] or NULL; out
 * must hold n rows. */
int bx_deepoc_update_host(bx_deepoc *e, int seq, const float *dets, int n, const double *embs,
                          const double *warp, double *out, int *n_out, void *stream);
/* per_class=True (bxclasses.h): one frame for sequences [seq0, seq0+nseq) of n_classes classes,
 * on an engine built with n_seq = S * n_classes (class c of sequence s is engine sequence
 * s * n_classes + c).  bx_deepoc_step's arguments, except: det_off / out / out_count are per
 * SEQUENCE (a sequence has at most det_cap rows), warps is [nseq * n_classes][6] (one per class
 * call) or NULL.  Runs class split -> the three launches over the class sequences -> id merge on
 * `stream`, nothing returning to the host; rows come out in class order with class-global ids.
 * The first per-class call fixes n_classes: another value is BX_ERR_INVALID.  A class whose
 * births pass the id map's capacity latches BX_ERR_CAPACITY (bx_deepoc_status). */
int bx_deepoc_step_classes(bx_deepoc *e, int seq0, int nseq, int n_classes, const float *dets,
                           const int32_t *det_off, const double *embs, const double *warps,
                           double *out, int32_t *out_count, void *stream);
/* Build the class state before the first per-class call with an id map of map_cap births per
 * class sequence instead of BX_CLASSES_MAP_CAP. */
int bx_deepoc_classes_config(bx_deepoc *e, int n_classes, int map_cap);
/* The engine's class state (NULL before the first per-class call): counters and maps are read
 * through bxclasses.h.  It stays the engine's. */
int bx_deepoc_classes(bx_deepoc *e, bx_classes **out);
/* Host form of one per-class frame of sequence seq (the drop-in update): warps_host
 * [n_classes][6] or NULL; *id_count_host is the class-level id counter, written to the device
 * before the frame and read back after it.  Synchronises once. */
int bx_deepoc_update_classes_host(bx_deepoc *e, int seq, int n_classes, const float *dets_host,
                                  int n, const double *embs_host, const double *warps_host,
                                  int *id_count_host, double *out_host, int *n_out, void *stream);
/* Capacity growth (the reference's track list is unbounded): copy every sequence's tracker
 * state of `src` into `dst`, a fresh engine with the same configuration and sequences and
 * track_cap / det_cap at least src's (slot ids stay valid).  Synchronous.  Tracks only: the
 * per-sequence parameter table is not copied. */
int bx_deepoc_copy_state(bx_deepoc *dst, bx_deepoc *src);
/* Per-sequence parameters, the contract of bx_ocsort_set_seq_params_host (bxocsort.h): a sweep
 * runs K configurations x S sequences as K*S sequences of ONE engine.  params_host [nseq] gives
 * sequences [seq0, seq0+nseq) parameters of their own; NULL clears the range, whose sequences then
 * run on the engine's parameters again.  Every entry is validated as the create call validates
 * the same fields (delta_t within the 8-slot observation ring, a known asso_kind); an invalid
 * entry, or a range outside [0, n_seq), returns BX_ERR_INVALID and changes nothing.  The values
 * live in a device table the frame kernel reads at its entry (uniform loads, once per workgroup)
 * and never writes; the other kernels of a step read none of them (alpha_fixed_emb reaches the
 * feature kernel through the records the frame kernel writes).  Until the first set there is no
 * table and the kernel runs as it always did.  Copies on `stream`, then synchronises it.
 * The table is indexed by engine sequence: for a bx_deepoc_step_classes engine that is the class
 * sequence s * n_classes + c, and nothing more is promised there.
 * Meant for use between sequences, at frame 0 (after a reset): changing a sequence's parameters
 * while it holds tracks is allowed, but no reference behaviour is defined for it.  A reset keeps
 * the table; a state copy carries tracks only, so the destination keeps its own table.
 * The second entry point reads a sequence's effective parameters back (its entry, or the
 * engine's when it has none); host memory, no device work. */
int bx_deepoc_set_seq_params_host(bx_deepoc *e, int seq0, int nseq,
                                  const bx_deepoc_seq_params *params_host, void *stream);
int bx_deepoc_seq_params_host(bx_deepoc *e, int seq, bx_deepoc_seq_params *out_host);
/* Latched device status (BX_OK, BX_ERR_TRACK_OVERFLOW or BX_ERR_CAPACITY). */
int bx_deepoc_status(bx_deepoc *e, int *status);
int bx_deepoc_counters_host(bx_deepoc *e, int seq, int *frame_count, int *id_count,
                            int *n_tracks);
/* KalmanBoxTracker.count is class-global in the reference (deepocsort.py:56,117-118,305); the
 * Python drop-in mirrors it through this. */
int bx_deepoc_set_id_count(bx_deepoc *e, int seq, int id_count, void *stream);
/* Frame size (w, h) of a sequence — BaseTracker latches img.shape on the first frame. */
int bx_deepoc_set_frame_size(bx_deepoc *e, int seq, double w, double h, void *stream);
/* Track list of a sequence in list order (host, synchronous): ids [cap], Kalman means x
 * [cap][7], covariances p [cap][49] and embeddings emb [cap][emb_dim] (any may be NULL; emb is
 * not written with embedding_off); *n = number of tracks. */
int bx_deepoc_tracks_host(bx_deepoc *e, int seq, int cap, int32_t *ids, double *x, double *p,
                          double *emb, int *n);
/* Write kf.x [n][7] / kf.P [n][49] / emb [n][emb_dim] of live tracks by id (host, synchronous;
 * any may be NULL).  BX_ERR_INVALID for an unknown id. */
int bx_deepoc_state_set_host(bx_deepoc *e, int seq, int n, const int32_t *ids, const double *x,
                             const double *p, const double *emb);
/* Last-frame statistics over sequences [seq0, seq0+nseq) (host, synchronous): sums[3] =
 * {tracks alive after the frame, output rows, max frame counter}. */
int bx_deepoc_frame_stats_host(bx_deepoc *e, int seq0, int nseq, int64_t *sums);
/* Timing probe: while stage is 0 (contraction), 1 (frame) or 2 (embedding update), every step
 * records a HIP event pair around that launch; -1 turns it off.  probe_read synchronises and
 * returns the summed milliseconds and launch count, then clears. */
int bx_deepoc_probe(bx_deepoc *e, int stage);
int bx_deepoc_probe_read(bx_deepoc *e, double *total_ms, int *count);
/* Op-level contraction on plain device arrays, the same tile code as the tracker's:
 * out [nd][nt] = dets_embs [nd][F] @ trk_embs [nt][F].T, float64, each entry an ascending-k fma
 * chain. */
int bx_deepoc_embcost(int nd, int nt, int F, const double *dets_embs, const double *trk_embs,
                      double *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BXDEEPOCSORT_H */
