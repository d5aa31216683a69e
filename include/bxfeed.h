/*
 * bxfeed.h — C ABI of the device-resident sequence feeder in libbxassoc.so (MI355X, gfx950).
 *
 * The many-sequence runner (boxmot_amd.motio.run_sequences) drives S independent sequences
 * through one batched engine, frame index by frame index.  Its default path assembles every
 * frame on the host: per run of sequences it concatenates the detections and embeddings, copies
 * them to the device, steps, and copies the rows back.  The feeder keeps all of that in HBM:
 *   - every sequence's packed detections (float32 [rows][6]), embeddings (float64
 *     [rows][emb_dim]) and frame table are uploaded once;
 *   - per frame index one kernel gathers, for every run of sequences that has an update, the
 *     batched dets / embs / det_off arrays a step entry point takes (a ragged gather: sequences
 *     differ in length and in detections per frame);
 *   - per frame index a second kernel turns the steps' out / out_count into MOT rows (the value
 *     order of the host formatter in bxio.h) and appends them to a per-sequence device buffer;
 *   - one device-to-host copy at the end returns every sequence's rows.
 *
 * Reference interfaces replaced (file:line in muntherr/boxmot):
 *   the per-frame mask selection of a sequence's rows   boxmot/utils/dataloaders/MOT17.py:181-200
 *   convert_to_mot_format (numpy branch)                boxmot/engine/utils.py:101-133
 *   the per-frame loop of process_sequence              boxmot/engine/val.py:304-354
 *
 * A run is a maximal range of consecutive sequences [seq0, seq0 + nseq) that all have
 * detections at the frame index; sequences without detections there are not stepped
 * (val.py:347).  The host decides the runs once, at creation, from the frame tables.
 *
 * Conventions as in bxassoc.h: pointer arguments are DEVICE pointers unless their name ends in
 * _host, calls are asynchronous on `stream` (NULL = the default stream) unless said otherwise,
 * every function returns a bx_status and bx_last_error carries the text of a failure.
 */
#ifndef BXFEED_H
#define BXFEED_H

#include <stdint.h>

#include "bxassoc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every run's region of the gathered arrays starts at a multiple of this many rows, so the
 * dets, embs and out pointers of a run are all 256-byte aligned for any emb_dim. */
#define BX_FEED_ROW_ALIGN 32

typedef struct bx_feed bx_feed;

/* Lay out the feeder for n_seq sequences and allocate its device memory (synchronous).
 *   emb_dim          embedding width F; 0 = no embeddings are fed
 *   seq_rows_host    [n_seq] int64: packed rows of each sequence
 *   tab_off_host     [n_seq + 1] int64: prefix offsets of the sequences' frame tables; sequence
 *                    k iterates tab_off[k + 1] - tab_off[k] frame indices
 *   row_start_host   [tab_off[n_seq]] int64: first packed row (within its sequence) of entry
 *   row_cnt_host     [tab_off[n_seq]] int32: detections of the entry (0: not stepped)
 *   frame_id_host    [tab_off[n_seq]] int32: the frame number its MOT rows carry
 *   res_cap_host     [n_seq] int64 rows of each sequence's result buffer, or NULL: the sum of
 *                    its row_cnt (a step never returns more rows than it was given detections)
 *   guard_rows       extra rows allocated behind the last result buffer (tests read them back)
 * The result buffers and the guard rows start filled with 0xFF bytes (NaN rows).
 * BX_ERR_INVALID when an entry reaches outside its sequence's rows. */
int bx_feed_create(int n_seq, int emb_dim, const int64_t *seq_rows_host,
                   const int64_t *tab_off_host, const int64_t *row_start_host,
                   const int32_t *row_cnt_host, const int32_t *frame_id_host,
                   const int64_t *res_cap_host, int guard_rows, bx_feed **out);
/* bx_feed_create for sequences that share packed rows: sequence k gathers from the packed rows
 * of sequence src_host[k] ([n_seq] int32).  A hyper-parameter sweep runs K configurations x S
 * sequences as K*S sequences whose detections and embeddings are K copies of the same S arrays;
 * with src[k*S + s] = s they are stored and uploaded once.
 *   - src[k] <= k and src[src[k]] == src[k] (a source is its own source), and every frame table
 *     entry of sequence k lies inside the rows of src[k]; otherwise BX_ERR_INVALID;
 *   - only a source owns storage and accepts bx_feed_upload_host (BX_ERR_INVALID for another);
 *     seq_rows_host of a sequence that is not a source is ignored;
 *   - frame tables, runs, the gathered per-frame arrays, result buffers and appends stay per
 *     sequence, so every step is fed exactly as from bx_feed_create.
 * bx_feed_create is the identity map, with unchanged behaviour and layout. */
int bx_feed_create_shared(int n_seq, int emb_dim, const int64_t *seq_rows_host,
                          const int64_t *tab_off_host, const int64_t *row_start_host,
                          const int32_t *row_cnt_host, const int32_t *frame_id_host,
                          const int64_t *res_cap_host, int guard_rows, const int32_t *src_host,
                          bx_feed **out);
/* bx_feed_create_shared with a choice of the steps' types, for an engine whose step takes
 * float64 detections and writes 10-column rows (bx_ss_step):
 *   det_f64   0: the runs' dets are float32 [rows][6]; 1: float64 [rows][6].  The packed rows are
 *             stored and uploaded as float32 either way (bx_feed_upload_host is unchanged); the
 *             gather writes each value widened to float64, which is exact
 *   out_cols  8 or 10: columns of the runs' out rows.  With 10 the append reads the first 8
 *             columns of each row (stride 10) and writes the same 9-column MOT row
 * (0, 8) is bx_feed_create_shared exactly; any other det_f64 or out_cols is BX_ERR_INVALID.
 * Run regions stay 256-byte aligned: BX_FEED_ROW_ALIGN rows of 48 or of 80 bytes are multiples of
 * 256.  bx_feed_run reports, and bx_feed_read_run_host / bx_feed_write_run_host take, dets and out
 * of the mode's types. */
int bx_feed_create_shared_fmt(int n_seq, int emb_dim, const int64_t *seq_rows_host,
                              const int64_t *tab_off_host, const int64_t *row_start_host,
                              const int32_t *row_cnt_host, const int32_t *frame_id_host,
                              const int64_t *res_cap_host, int guard_rows,
                              const int32_t *src_host, int det_f64, int out_cols, bx_feed **out);
int bx_feed_destroy(bx_feed *f);
/* Bytes of device memory the feeder allocated at creation (host, no device work). */
int bx_feed_device_bytes(bx_feed *f, int64_t *bytes);
/* Upload sequence seq's packed rows (synchronous): dets_host float32 [rows][6], embs_host
 * float64 [rows][emb_dim] (ignored when emb_dim is 0).  Either may be NULL for 0 rows. */
int bx_feed_upload_host(bx_feed *f, int seq, const float *dets_host, const double *embs_host);
/* Shape of the schedule: frame indices, and the most runs any of them has. */
int bx_feed_shape(bx_feed *f, int *n_frames, int *max_runs);
/* Runs of frame index t. */
int bx_feed_frame_runs(bx_feed *f, int t, int *n_runs);
/* Run r of frame index t: its sequences, its detections and the device arrays of its step —
 * dets float32 [rows][6], det_off int32 [nseq + 1], embs float64 [rows][emb_dim] (NULL when
 * emb_dim is 0), out float64 [rows][8] and out_count int32 [nseq]; dets float64 [rows][6] and out
 * float64 [rows][out_cols] in the modes of bx_feed_create_shared_fmt.  The arrays are the
 * feeder's and are reused by the next frame index. */
int bx_feed_run(bx_feed *f, int t, int r, int *seq0, int *nseq, int *rows, void **dets,
                void **det_off, void **embs, void **out, void **out_count);
/* Gather every run of frame index t (one launch; none when the frame has no run). */
int bx_feed_gather(bx_feed *f, int t, void *stream);
/* Append the MOT rows of every run of frame index t, from the out / out_count its steps left:
 * row = frame, id, round(l), round(t), round(w), round(h), 1, cls, conf as the host formatter
 * writes them, sequence k's rows behind the ones it already has.  A sequence whose rows would
 * not fit its buffer, or whose out_count is outside [0, detections], appends nothing and
 * latches BX_ERR_CAPACITY. */
int bx_feed_append(bx_feed *f, int t, void *stream);
/* Latched device status (BX_OK or BX_ERR_CAPACITY); synchronises. */
int bx_feed_status(bx_feed *f, int *status);
/* Rows of the whole result allocation: the sum of the capacities plus guard_rows. */
int bx_feed_result_rows(bx_feed *f, int64_t *rows);
/* The one device-to-host copy (synchronous): res_host [result_rows][9] float64, the whole
 * allocation; base_host [n_seq + 1] int64 first row of each sequence's buffer; n_host [n_seq]
 * int64 rows each sequence appended. */
int bx_feed_results_host(bx_feed *f, double *res_host, int64_t *base_host, int64_t *n_host);
/* The same three buffers where they lie, as DEVICE pointers: res float64 [result_rows][9], base
 * int64 [n_seq + 1], n int64 [n_seq]; rows = result_rows.  No copy and no synchronisation: the
 * caller orders its reads behind the appends.  Valid until bx_feed_destroy. */
int bx_feed_results_device(bx_feed *f, void **res, void **base, void **n, int64_t *rows);
/* Diagnostics (synchronous): read back the gathered inputs of run r of frame index t (after a
 * gather of t), and write out / out_count of that run from host arrays (before an append).
 * dets_host is float32 [rows][6], or float64 [rows][6] for a feeder created with det_f64;
 * out_host is float64 [rows][out_cols]. */
int bx_feed_read_run_host(bx_feed *f, int t, int r, void *dets_host, int32_t *det_off_host,
                          double *embs_host);
int bx_feed_write_run_host(bx_feed *f, int t, int r, const double *out_host,
                           const int32_t *out_count_host);

#ifdef __cplusplus
}
#endif

#endif /* BXFEED_H */
