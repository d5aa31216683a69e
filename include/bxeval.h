/*
 * bxeval.h — C ABI of the MOT evaluation in libbxassoc.so: HOTA, CLEAR and Identity metrics of
 * MOT16 / MOT17 / MOT20 pedestrian result rows against ground truth, for many sequences at once.
 *
 * Reference stage replaced: the TrackEval subprocess of engine/val.py:224-267 (its numbers are
 * what parse_mot_results, val.py:190-219, reads back).  The contract — similarity, the
 * distractor preprocessing, the three metric families and how sequences combine — is DESIGN.md
 * section 2.13.
 *
 * Conventions as in bxassoc.h: every function returns a bx_status and bx_last_error carries the
 * text of a failure.  All arithmetic is float64.  Results are deterministic run to run: integer
 * counts use integer atomics, every floating-point sum runs in a fixed order.
 */
#ifndef BXEVAL_H
#define BXEVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Default capacities of bx_eval_create (an argument of 0 selects them). */
#define BX_EVAL_MAX_BOXES 256   /* gt rows, or tracker rows, in one frame (at most 1024) */
#define BX_EVAL_MAX_IDS 4096    /* distinct gt ids, or tracker ids, in one sequence (at most 16384) */
#define BX_EVAL_MAX_FRAMES 8192 /* frames of one sequence */
/* The Identity assignment of a sequence (size GT_IDs + IDs) keeps its solver state in LDS up to
 * this size (10 KiB per one-wave workgroup); larger problems keep it in HBM. */
#define BX_EVAL_LDS_N 256

#define BX_EVAL_NALPHA 19 /* HOTA localisation thresholds 0.05, 0.10, ..., 0.95 */

/* Layout of one result record (float64; counts are exact integers).  The HOTA fields are
 * BX_EVAL_NALPHA-vectors, one after another in this order. */
enum {
  BX_EVAL_H_TP = 0,   /* HOTA_TP, then HOTA_FN, HOTA_FP, AssA, AssRe, AssPr, LocA, DetA, DetRe, */
  BX_EVAL_H_FN = 19,  /* DetPr, HOTA: 11 vectors */
  BX_EVAL_H_FP = 38,
  BX_EVAL_H_ASSA = 57,
  BX_EVAL_H_ASSRE = 76,
  BX_EVAL_H_ASSPR = 95,
  BX_EVAL_H_LOCA = 114,
  BX_EVAL_H_DETA = 133,
  BX_EVAL_H_DETRE = 152,
  BX_EVAL_H_DETPR = 171,
  BX_EVAL_H_HOTA = 190,
  /* CLEAR: CLR_TP, CLR_FN, CLR_FP, IDSW, MT, PT, ML, Frag, MOTP_sum, CLR_Frames, MOTA, MOTP,
   * MODA, sMOTA, CLR_Re, CLR_Pr, MTR, PTR, MLR */
  BX_EVAL_CLEAR = 209,
  /* Identity: IDTP, IDFN, IDFP, IDF1, IDR, IDP */
  BX_EVAL_IDENTITY = 228,
  /* Count: Dets, GT_Dets, IDs, GT_IDs (boxes and distinct ids kept by the preprocessing) */
  BX_EVAL_COUNT = 234,
  BX_EVAL_NF = 238
};

/* A handle with its capacities (0 = the default above).  The handle owns a device arena that
 * grows to the largest batch it has run.  BX_ERR_INVALID for a capacity out of range. */
int bx_eval_create(int max_boxes, int max_ids, int max_frames, void **out);
int bx_eval_destroy(void *h);
/* The handle's capacities, and the LDS-resident Identity size. */
int bx_eval_capacity(void *h, int *max_boxes, int *max_ids, int *max_frames, int *lds_n);

/* Evaluate n_seq sequences from host arrays, copying in and out and synchronising.
 *   benchmark        16, 17 or 20 (MOT20 adds class 6 to the distractors 2, 7, 8, 12)
 *   seq_frames_host  [n_seq] frames of each sequence
 *   gt_off_host      [n_seq + 1] prefix offsets of each sequence's rows in gt_rows_host
 *   gt_rows_host     [.][9]: frame, id, x, y, w, h, zero_marked, class, visibility
 *   tr_off_host      [n_seq + 1] likewise for tr_rows_host
 *   tr_rows_host     [.][6]: frame, id, x, y, w, h
 *   out_host         [n_seq + 1][BX_EVAL_NF]: one record per sequence, then COMBINED
 * Rows of a sequence may come in any order.  BX_ERR_INVALID: a frame outside 1..frames, a
 * non-integer frame or id, an id twice in one frame of one side.  BX_ERR_CAPACITY: more rows of
 * one side in a frame than max_boxes, more distinct ids of one side in a sequence than max_ids,
 * more frames than max_frames — never a silent truncation. */
int bx_eval_run_host(void *h, int n_seq, int benchmark, const int32_t *seq_frames_host,
                     const int64_t *gt_off_host, const double *gt_rows_host,
                     const int64_t *tr_off_host, const double *tr_rows_host, double *out_host,
                     void *stream);

/* Bucket and upload the ground truth of n_seq sequences (arguments and errors as the gt side of
 * bx_eval_run_host) into an allocation the handle keeps until the next call replaces it or the
 * handle is destroyed.  Synchronous.  bx_eval_run_host ignores it. */
int bx_eval_set_gt_host(void *h, int n_seq, const int32_t *seq_frames_host,
                        const int64_t *gt_off_host, const double *gt_rows_host);

/* Evaluate tracker rows that lie in device memory against the resident ground truth of S
 * sequences, for n_groups groups at once: evaluator sequence q = k * S + s is scored against gt
 * sequence s.  The rows never cross to the host; O(frames + sequences) integers do.
 *   tr_rows     DEVICE float64 [.][row_stride], row_stride >= 6: frame, id, x, y, w, h, ...
 *   tr_base     DEVICE int64 [n_groups * S] first row of sequence q
 *   tr_n        DEVICE int64 [n_groups * S] rows of sequence q; rows outside [base, base + n)
 *               are never read
 *   out_host    [n_groups][S + 1][BX_EVAL_NF]: a group's S records, then its COMBINED
 * The work is queued on `stream` and synchronised; the caller orders the rows' producer before
 * it.  Results are bit-identical to bx_eval_run_host on the same rows in the same order, and the
 * statuses are the same (BX_ERR_INVALID also when no gt is set, or for a negative base or n);
 * out_host is written only on BX_OK. */
int bx_eval_run_device(void *h, int n_groups, int benchmark, const void *tr_rows,
                       int64_t row_stride, const void *tr_base, const void *tr_n, double *out_host,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif
