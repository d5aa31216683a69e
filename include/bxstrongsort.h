/*
 * bxstrongsort.h — C ABI of the StrongSort engine in libbxassoc.so (MI355X, gfx950).
 *
 * Boundary: everything the fork's "enhanced" StrongSort.update(dets, img, embs) computes per
 * frame — detection quality and ordering, crowd detection and its parameter adjustments, camera
 * warp, XYAH Kalman predict, the three-stage matching (appearance cascade on high- then
 * medium-confidence detections: NN-gallery cosine distance on the fp64 matrix cores, Mahalanobis
 * gating, motion/quality/confidence cost shaping, scipy's linear_sum_assignment; then IoU), the
 * Kalman/feature updates, misses, ID recovery from the lost-track buffer, births, deaths, the
 * gallery's partial_fit budget pruning and the output rows — runs on the GPU behind these entry
 * points: per frame a detection-feature kernel (wave per detection), the gallery distance
 * (fp64 MFMA, wave per confirmed track and detection block), the recovery similarities, the
 * pre-match kernel (one wave per sequence), the stage 1/2 costs (wave per confirmed track), the
 * matching kernel (one wave per sequence), the track updates (wave per match), the post-match
 * kernel (recovery, births, lost buffer, outputs; wave per sequence) and partial_fit (wave per
 * track).
 *
 * Reference interfaces replaced (file:line in muntherr/boxmot @ /root/reference):
 *   bx_ss_create/step/update_host  StrongSort.__init__ / StrongSort.update
 *                                  boxmot/trackers/strongsort/strongsort.py:45-181, 285-345
 *     Tracker                      trackers/strongsort/sort/tracker.py:63-344
 *     Track / Detection            sort/track.py:76-400, sort/detection.py:35-42
 *     matching_cascade, min_cost_matching, gate_cost_matrix + cost shaping,
 *     NearestNeighborDistanceMetric sort/linear_assignment.py:14-618
 *     iou_cost                     sort/iou_matching.py:10-87
 *     detect_crowd_situations      utils/occlusion_handler.py:45-87, 464-490
 * The fork needs the minimal patch P6; `born_confirmed` stands for its
 * GITHUB_ACTIONS=true switch (D8).  handle_occlusions=True (OcclusionAwareTracker,
 * utils/occlusion_handler.py:312-439) is a host post-process (boxmot_amd/occlusion.py) over the
 * track-attribute calls below, which raises where the reference crashes on mutual occlusion (D7)
 * and which the single-stream drop-in uses; or, for the many-sequence flows, an eleventh kernel
 * at the end of the frame (bx_ss_set_occlusion_host) that makes the same edits on the device.
 * Bit-identical to oracle/bxo_strongsort.c (pinned by tests/golden/trk_strongsort_*.npz).
 *
 * Conventions as in bxassoc.h: device pointers unless a name ends in _host, asynchronous on
 * `stream`, every function returns a bx_status (bx_last_error explains failures).
 */
#ifndef BXSTRONGSORT_H
#define BXSTRONGSORT_H

#include <stdint.h>

#include "bxassoc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* StrongSort constructor parameters (strongsort.py:45-66 names and defaults: min_conf .1,
 * max_cos_dist .15, max_iou_dist .7, max_age 50, n_init 2, nn_budget 150, mc_lambda .995,
 * ema_alpha .9, conf_thresh_high .7, conf_thresh_low .3, id_preservation_weight .1,
 * crowd_detection 1). */
typedef struct {
    int32_t n_seq;      /* independent sequences held by this engine */
    int32_t track_cap;  /* track slots per sequence, live + lost-buffer (<= 1024) */
    int32_t det_cap;    /* max detections per frame per sequence (<= 1024) */
    int32_t emb_dim;    /* embedding dimension F (float64 embeddings, required) */
    int32_t vec_cap;    /* feature vectors kept per track slot (its features + gallery
                           samples; <= 64, default 32).  max(nn_budget, crowd budget) + 10
                           <= 320 (gallery entries per track) */
    double min_conf, max_cos_dist, max_iou_dist;
    int32_t max_age, n_init, nn_budget;
    double mc_lambda, ema_alpha, conf_thresh_high, conf_thresh_low, id_preservation_weight;
    int32_t crowd_detection, born_confirmed;
} bx_ss_config;

typedef struct bx_ss bx_ss;

int bx_ss_create(const bx_ss_config *cfg, bx_ss **out);
int bx_ss_destroy(bx_ss *e);
/* Forget all tracks of sequences [seq0, seq0+nseq). */
int bx_ss_reset(bx_ss *e, int seq0, int nseq, void *stream);
/* One frame for sequences [seq0, seq0+nseq).
 *   dets    [sum N][6] float64 (x1,y1,x2,y2,conf,cls) — StrongSort has no setup_decorator,
 *           detections are not rounded to float32
 *   det_off [nseq+1] int32 prefix offsets
 *   embs    [sum N][emb_dim] float64
 *   warps   [nseq][6] float64 2x3 camera-motion affine per sequence, NULL = identity
 *   out     [sum N][10] float64 rows [x1,y1,x2,y2,id,conf,cls,det_ind,quality,occlusion]
 *           in track-list order, sequence k from row det_off[k]; occlusion is 0 unless the
 *           sequence runs the occlusion pass (bx_ss_set_occlusion_host), which writes the level
 *   out_count [nseq] int32 */
int bx_ss_step(bx_ss *e, int seq0, int nseq, const double *dets, const int32_t *det_off,
               const double *embs, const double *warps, double *out, int32_t *out_count,
               void *stream);
/* Host-memory path for one sequence (the drop-in update). out must hold n rows of 10. */
int bx_ss_update_host(bx_ss *e, int seq, const double *dets, int n, const double *embs,
                      const double *warp, double *out, int *n_out, void *stream);
/* Latched device status (BX_OK, BX_ERR_TRACK_OVERFLOW — track slots or a slot's vector pool
 * exhausted — or BX_ERR_CAPACITY). */
/* Capacity growth (the reference's track list is unbounded: sort/tracker.py:118-181 (self.tracks), sort/track.py:98-105): copy every
 * sequence's tracker state of `src` into `dst`, a fresh engine with the same configuration and
 * sequences and track_cap / det_cap at least src's (slot ids stay valid).  Synchronous. */
int bx_ss_copy_state(bx_ss *dst, bx_ss *src);
/* Per-sequence parameters (a hyper-parameter sweep: K configs x S sequences as K*S sequences of
 * one engine; boxmot_amd.tune.sweep_strong).  The names, order and meaning of
 * bx_ss_config's: every field of it that sizes no memory. */
typedef struct {
    double min_conf, max_cos_dist, max_iou_dist;
    int32_t max_age, n_init, nn_budget;
    double mc_lambda, ema_alpha, conf_thresh_high, conf_thresh_low, id_preservation_weight;
    int32_t crowd_detection, born_confirmed;
} bx_ss_seq_params;
/* Give sequences [seq0, seq0+nseq) parameters of their own: params_host [nseq], read as
 * bx_ss_create reads the configuration, the flags as != 0.  NULL clears the range: those
 * sequences run on the engine's values again.  n_seq, track_cap, det_cap, emb_dim and vec_cap stay
 * engine-wide.  Every entry is checked before anything is written, by bx_ss_create's checks on the
 * same fields: nn_budget > 0, max_age >= 0, max(nn_budget, crowd budget min(2 nn_budget, 300))
 * + 10 <= 320, and no more than the engine's own nn_budget gives, which sized the galleries.  A
 * failing entry or a bad range is BX_ERR_INVALID and changes nothing.
 *
 * Contract with the state crowd mode adapts.  A sequence's live max_age, nn_budget and
 * metric.matching_threshold are device state that crowd mode saves, scales and restores per
 * sequence.  An entry's max_age, nn_budget and max_cos_dist are the SEEDS of that state, not live
 * values: the set writes them into the sequence's state (live value and restore value alike),
 * bx_ss_reset seeds a sequence from its entry when it has one and from the engine's configuration
 * otherwise, and crowd mode then works on the sequence's state exactly as without a table, so it
 * restores to the entry's values.  A set or a clear is therefore accepted only for sequences
 * whose frame counter (bx_ss_counters_host) is 0, fresh or just reset; otherwise it is
 * BX_ERR_INVALID and changes nothing.  A clear seeds the engine's values.  The other ten fields
 * are read by the frame's kernels each frame.
 *
 * The entry applies to bx_ss_step and bx_ss_update_host alike.  The first set allocates the
 * device table; an engine on which none was ever set launches the kernels built without it.
 * bx_ss_reset keeps the table, bx_ss_copy_state does not copy it (it copies the tracks and the
 * sequences' adapted state: set the table on the fresh engine first, then copy).  Synchronises the
 * device before anything is read or written and `stream` after. */
int bx_ss_set_seq_params_host(bx_ss *e, int seq0, int nseq, const bx_ss_seq_params *params_host,
                              void *stream);
/* The parameters sequence `seq` runs on (host mirror, no device work): its own as they were given
 * when set, else the engine's.  max_age, nn_budget and max_cos_dist are the seeds, not what crowd
 * mode made of them. */
int bx_ss_seq_params_host(bx_ss *e, int seq, bx_ss_seq_params *out_host);
int bx_ss_status(bx_ss *e, int *status);
/* Per-sequence counters (host): frame count, next id, live tracks, lost-buffer tracks. */
int bx_ss_counters_host(bx_ss *e, int seq, int *frame_count, int *next_id, int *n_tracks,
                        int *n_lost);
/* Track list in list order (host): ids, states (1 tentative, 2 confirmed), means [8], covs [64]. */
int bx_ss_tracks_host(bx_ss *e, int seq, int cap, int32_t *ids, int32_t *state, double *mean,
                      double *cov, int *n);
/* Write Track.mean [n][8] / Track.covariance [n][64] of live tracks by id (host, synchronous;
 * either may be NULL): the state edit OcclusionAwareTracker._update_track_with_predicted_position
 * makes (utils/occlusion_handler.py:380-398; sort/track.py:76-400 attributes).
 * BX_ERR_INVALID for an unknown id. */
int bx_ss_state_set_host(bx_ss *e, int seq, int n, const int32_t *ids, const double *mean,
                         const double *cov);
/* Track attributes the host-side OcclusionAwareTracker reads and edits
 * (utils/occlusion_handler.py:341-417; sort/track.py:76-131 attributes), host and synchronous,
 * list order / by id:
 *   bx_ss_track_attrs_host      ids, quality_score, conf, _max_age, len(features) (any NULL)
 *   bx_ss_track_attrs_set_host  quality_score / conf / _max_age by id (NULL arrays untouched)
 *   bx_ss_last_feature_host     features[-1] [n][emb_dim] by id
 *   bx_ss_last_feature_set_host `features[-1] = v` [n][emb_dim] by id (normalize: v / (wave-order
 *                               norm + 1e-8) first, the engine's np.linalg.norm order); the
 *                               gallery keeps the replaced vector's content
 * BX_ERR_INVALID for an unknown id (or a track without features for the feature calls). */
int bx_ss_track_attrs_host(bx_ss *e, int seq, int cap, int32_t *ids, double *quality,
                           double *conf, int32_t *max_age, int32_t *n_features, int *n);
int bx_ss_track_attrs_set_host(bx_ss *e, int seq, int n, const int32_t *ids, const double *quality,
                               const double *conf, const int32_t *max_age);
int bx_ss_last_feature_host(bx_ss *e, int seq, int n, const int32_t *ids, double *feats);
int bx_ss_last_feature_set_host(bx_ss *e, int seq, int n, const int32_t *ids, const double *feats,
                                int normalize);
/* Occlusion handling on the device: OcclusionAwareTracker.update_with_occlusion_handling
 * (utils/occlusion_handler.py:312-439) as the last kernel of a frame, one workgroup per stepped
 * sequence, bit for bit what boxmot_amd/occlusion.py's OcclusionHandler does through the host
 * calls above: the O(T^2) overlap analysis over the track list's tlwh rows (read as corner
 * boxes, as the reference reads them), _max_age doubled (held at 2^30) and quality_score floored
 * at 0.6 for a level above 0.3, features[-1] buffered, the mean replaced by the occluders' mean
 * centre (summed in the iteration order of the reference's Python set; covariance[:4,:4] x 1.5)
 * above 0.8, an emerging track's conf + 0.1 and features[-1] blended with its strongest buffered
 * vector, and the sequence's output rows written again (moved boxes, conf, quality, column 9 the
 * level).  The reference's occlusion_stats events are not kept.
 *
 * bx_ss_set_occlusion_host: on [nseq] (!= 0 enables) and threshold [nseq] (occlusion_threshold)
 * of sequences [seq0, seq0+nseq).  The first call allocates, per sequence, a pool of occ_cap
 * buffered tracks (each an id and a ring of the 10 newest vectors, deque(maxlen=10)); occ_cap is
 * fixed from then on, another value is BX_ERR_INVALID.  Accepted only for sequences whose frame
 * counter is 0, as the parameter table.  An engine on which it was never called launches exactly
 * the kernels it launched before; afterwards every frame ends with the pass, which returns at
 * once for a sequence that is off.  Synchronises the device and `stream`.
 *
 * A pool entry is released when its track emerges (the reference deletes the buffer) and when
 * its id is in neither the track list nor the lost buffer: such an id cannot come back (ID
 * recovery revives ids from the lost buffer only), while the reference keeps the dead buffer for
 * ever.  A full pool latches BX_ERR_CAPACITY (bx_ss_status) and skips that append; nothing else
 * of the frame changes.  Entries of tracks that emerge in a frame become free at the end of that
 * frame, while the host deletes and appends in list order: a pool that is exactly full can
 * therefore skip an append for which the host order had room.  The error is on the safe side;
 * size occ_cap with one frame's emergences to spare.  The pass is outside bx_ss_probe's stages.
 *
 * A mutual occlusion (size ratio in [0.8, 1.2] above the threshold) is where the reference raises
 * TypeError (D7): the sequence makes no edit in that frame, its update count (the frame counter)
 * is latched and the pass skips the sequence from then on.
 *
 * bx_ss_occlusion_host: the settings, the latched update count (0: none) and the pool entries in
 * use (any pointer may be NULL).  bx_ss_occlusion_buffer_host: the buffer of track `id`, oldest
 * first, vecs [10][emb_dim] (may be NULL), n = 0 without one.  bx_ss_reset clears a sequence's
 * pool and latch and keeps its settings; bx_ss_copy_state copies pools, latches and settings
 * (allocating the destination's pools with the source's occ_cap when it has none; a source that
 * never enabled the pass clears the destination's pools, latches and settings). */
int bx_ss_set_occlusion_host(bx_ss *e, int seq0, int nseq, const int32_t *on,
                             const double *threshold, int occ_cap, void *stream);
int bx_ss_occlusion_host(bx_ss *e, int seq, int *on, double *threshold, int *mutual_frame,
                         int *n_buffered);
int bx_ss_occlusion_buffer_host(bx_ss *e, int seq, int id, double *vecs, int *n);
/* Iteration order of a CPython set of non-negative ints after adding adds[0..n) in order
 * (hash(i) = i, 9 linear probes then perturb >>= 5, growth to the first power of two above
 * 4 * fill when fill * 5 >= mask * 3, iteration in table order; csrc/bx_pyset.h, the function the
 * occlusion kernel runs in LDS): out [n] gets the distinct keys, n_out their number.  Host only. */
int bx_pyset_order_host(const int64_t *adds, int n, int64_t *out, int *n_out);
/* Last-frame statistics over sequences [seq0, seq0+nseq) (host): sums[7] = {detections kept,
 * tracks entering the frame, confirmed tracks queried next frame, gallery sample rows compared,
 * output rows, max frame counter, matches} — bench.py's unit counts. */
int bx_ss_frame_stats_host(bx_ss *e, int seq0, int nseq, int64_t *sums);
/* How the cascade / IoU LSAPs (linear_assignment.py:14-93's linear_sum_assignment) are solved:
 * fast = 1 (default) solve + certify — rows' minima in parallel, Crouse's search for the
 * contested ones, then a reduced-cost certificate that the optimum is unique up to pairs
 * min_cost_matching rejects; scipy's own row order only for a tied level (and a whole cascade
 * stage in scipy's order when a tie follows a level whose unmatched order was not certified).
 * fast = 0: scipy's row order always.  Both give the reference's matches.  Synchronous. */
int bx_ss_set_lsap_mode(bx_ss *e, int fast);
/* LSAP counters of sequences [seq0, seq0+nseq) since creation: sums[5] = {solves, certified
 * unique, certified unique up to rejected pairs, ties re-solved in scipy's order, cascade stages
 * restarted in scipy's order}.  Synchronous. */
int bx_ss_lsap_stats_host(bx_ss *e, int seq0, int nseq, int64_t *sums);
/* Test entry point of the match kernel's LSAP on a dense row-major [R][CC] float64 cost (device),
 * 1 <= R <= CC <= 1024: fast = 0 scipy's linear_sum_assignment row order, 1 solve + certify
 * against max_d (min_cost_matching's rejection threshold).  rows / cols [R] (device) get the
 * pairs in row order; info[2] (device) = {pairs, or -1 when fast found a tie that could change a
 * real (<= max_d) pair; 0 unique, 1 unique up to rejected pairs, 2 tie}; status (device) is
 * latched BX_ERR_INVALID on an engine fault. */
int bx_ss_lsap_op(const double *cost, int R, int CC, double max_d, int fast, int32_t *rows,
                  int32_t *cols, int32_t *info, int32_t *status, void *stream);
/* Timing probe: stage 0 = detection features, 1 = gallery distance, 2 = recovery similarities,
 * 3 = pre-match (crowd, warp, quality, predict), 4 = stage 1/2 costs, 5 = matching, 6 = track
 * updates, 7 = post-match, 8 = partial_fit; -1 = off (see bx_boost_probe). */
int bx_ss_probe(bx_ss *e, int stage);
int bx_ss_probe_read(bx_ss *e, double *total_ms, int *count);

#ifdef __cplusplus
}
#endif

#endif /* BXSTRONGSORT_H */
