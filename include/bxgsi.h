/*
 * bxgsi.h — C ABI of the GSI post-processing in libbxassoc.so: Gaussian-smoothed interpolation
 * of MOT result rows (StrongSORT++), for many sequences and all their tracklets at once.
 *
 * Reference interfaces replaced (boxmot/postprocessing/gsi.py):
 *   bx_gsi_interpolate_plan + bx_gsi_interpolate   linear_interpolation   gsi.py:13-54
 *   bx_gsi_smooth                                  gaussian_smooth        gsi.py:57-93
 *   bx_gsi_run_host                                process_file's two calls  gsi.py:106-109
 *   bx_gsi_device_plan + bx_gsi_device_run         the same two calls, then process_file's
 *                                                  np.savetxt(fmt="%d ...") and the evaluator's
 *                                                  read of that file, for rows that stay in
 *                                                  device memory
 *
 * Conventions as in bxassoc.h: pointer arguments are DEVICE pointers unless their name ends in
 * _host, calls are asynchronous on `stream` (NULL = the default stream), every function returns
 * a bx_status and bx_last_error carries the text of a failure.  Rows are row-major float64 with
 * the frame in column 0 and the track id in column 1 (MOT ids are integers).  Row counts and
 * output row counts must stay below 2^31.
 */
#ifndef BXGSI_H
#define BXGSI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Longest tracklet (rows of one id after interpolation) bx_gsi_smooth factors; a longer one is
 * BX_ERR_CAPACITY.  (MOT20 sequences exceed 3000 frames.) */
#define BX_GSI_MAX_N 4096
/* Tracklets of at most this many rows are factored in LDS (packed lower triangle + the four
 * right-hand sides: 129 KiB of the CU's 160 KiB); longer ones take the blocked path. */
#define BX_GSI_LDS_N 176
/* Panel width of the blocked path. */
#define BX_GSI_NB 32

/* Bytes of workspace the two interpolation passes need for R input rows. */
int bx_gsi_plan_workspace_bytes(int64_t R, size_t *bytes);

/* Pass 1 of linear_interpolation over the rows of many sequences: sorts the rows by (sequence,
 * id, frame) — np.lexsort's stable order — counts the rows every gap prev+1 < cur < prev+interval
 * between consecutive rows of one id inserts, and prefixes the counts.
 *   rows   [R][C] float64, C >= 2
 *   seq    [R] int32 sequence of each row, or NULL (one sequence)
 *   ws     bx_gsi_plan_workspace_bytes(R) bytes; holds the plan for bx_gsi_interpolate
 *   counts [2] int64: rows of the interpolated output, tracklets (runs of one sequence and id) */
int bx_gsi_interpolate_plan(const double *rows, const int32_t *seq, int64_t R, int C,
                            int interval, void *ws, size_t ws_bytes, int64_t *counts,
                            void *stream);
/* Pass 2: writes the interpolated rows in (sequence, id, frame) order: every inserted row is
 * prev_row + (row - prev_row) * (i / (cur - prev)) on every column, in that float64 order.
 *   ws        the plan pass 1 left (same rows, R, C)
 *   out       [cap][C]; out_seq [cap] int32 sequence of each output row, or NULL
 *   track_off [tracklets + 1] int32 prefix offsets of the tracklets into out
 * cap must be at least counts[0] (rows past cap are not written). */
int bx_gsi_interpolate(const double *rows, int64_t R, int C, const void *ws, double *out,
                       int32_t *out_seq, int64_t cap, int32_t *track_off, void *stream);

/* Bytes of workspace bx_gsi_smooth needs for these tracklets (the device copy of the offsets and
 * the HBM factor slots of the blocked path). */
int bx_gsi_workspace_bytes(const int32_t *track_off_host, int n_tracks, int force_blocked,
                           size_t *bytes);
/* gaussian_smooth for a batch of tracklets, one workgroup per tracklet, float64 throughout:
 * tracklet k owns rows track_off_host[k]..track_off_host[k+1] of `rows` ([.][C], C >= 8).  With
 * n rows and frames t, ls = clip(tau*log(tau^3/n), 1/tau, tau^2), K[i][j] = exp(-0.5 * (t_i/ls -
 * t_j/ls)^2) (diagonal exactly 1), K + 1e-10*I = L L^T, alpha = the solve for columns 2..5, and
 * the smoothed columns are K @ alpha.
 *   out    [rows][9]: frame, id, the 4 smoothed columns, columns 6 and 7, -1
 *   status [n_tracks] int32: BX_OK, or BX_ERR_INVALID for a tracklet whose factorisation met a
 *          non-positive pivot (the reference raises LinAlgError); its rows then carry columns
 *          2..5 unsmoothed, never NaN from the failed factor
 *   force_blocked  0: tracklets of at most BX_GSI_LDS_N rows are factored in LDS, longer ones by
 *          the blocked right-looking factorisation in the workspace; 1: every tracklet takes the
 *          blocked path (tests use it to show the two paths agree)
 * A tracklet longer than BX_GSI_MAX_N is BX_ERR_CAPACITY (nothing is launched). */
int bx_gsi_smooth(const double *rows, int C, const int32_t *track_off_host, int n_tracks,
                  double tau, int force_blocked, void *ws, size_t ws_bytes, double *out,
                  int32_t *status, void *stream);

/* Host-memory path for one file's rows: interpolation then smoothing, copying in and out, and
 * synchronising.  rows_host [R][C] (C >= 8); out_host [cap][9]; *n_out receives the row count
 * (BX_ERR_CAPACITY when it exceeds cap; *n_out is still set).  BX_ERR_INVALID when a tracklet's
 * factorisation failed. */
int bx_gsi_run_host(const double *rows_host, int64_t R, int C, int interval, double tau,
                    double *out_host, int64_t cap, int64_t *n_out, void *stream);

/* GSI from result slots in device memory to evaluator-ready rows in device memory: what
 * bx_feed_results_device hands out goes in, what bx_eval_run_device takes (row_stride 9) comes
 * out, and no result row crosses to the host.  Sequence q owns rows [base[q], base[q] + n[q]) of
 * `rows`; rows outside the slots (slack, guard rows) are never read.  A tracklet is a run of one
 * (sequence, id): equal ids in different sequences never merge.
 *
 * Plan: packs the slots' rows (columns 0..7) densely in slot order, sorts and counts them as
 * bx_gsi_interpolate_plan does, and synchronises to bring two numbers back.
 *   rows   [.][row_stride] float64, row_stride >= 8
 *   base   [n_seq] int64, n [n_seq] int64 (both are read back: 16 * n_seq bytes)
 *   counts_host [2] int64: rows of the output, tracklets
 *   plan   receives a handle that owns its device memory; bx_gsi_device_free releases it
 * BX_ERR_INVALID for a negative base or n, or a total of 2^30 - 1 rows or more (the limit of
 * bx_gsi_interpolate_plan). */
int bx_gsi_device_plan(const double *rows, int64_t row_stride, const int64_t *base,
                       const int64_t *n, int n_seq, int interval, int64_t *counts_host,
                       void **plan, void *stream);
/* Run: interpolation, smoothing (bx_gsi_smooth: its paths, its bits, its BX_ERR_CAPACITY for a
 * tracklet over BX_GSI_MAX_N) and the finalise pass; synchronises for the tracklet offsets and at
 * the end.
 *   out      [cap][9] float64, cap >= counts_host[0] (else BX_ERR_CAPACITY): sequences
 *            consecutively in input order, within a sequence ids ascending and frames ascending
 *            within an id, the values of bx_gsi_smooth on that sequence's rows alone
 *   out_base [n_seq] int64 first output row of each sequence; out_n [n_seq] int64 its row count
 *            (0 for a sequence without rows)
 *   truncate nonzero: every value is truncated toward zero, as the reference's
 *            np.savetxt(fmt="%d ...") leaves it in a file, and a zero is +0.0; 0: the float rows
 * Read back: the tracklet offsets (4 bytes per tracklet) and one int32, the first tracklet whose
 * factorisation met a non-positive pivot.  That is BX_ERR_INVALID; the message names the
 * tracklet's id and its row count. */
int bx_gsi_device_run(void *plan, double tau, int truncate, double *out, int64_t cap,
                      int64_t *out_base, int64_t *out_n, void *stream);
int bx_gsi_device_free(void *plan);

#ifdef __cplusplus
}
#endif
#endif
