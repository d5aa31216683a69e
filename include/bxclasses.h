/*
 * bxclasses.h — C ABI of the device class split and id merge in libbxassoc.so (MI355X, gfx950).
 *
 * per_class=True (reference boxmot/trackers/basetracker.py:155-201): the tracker's update runs
 * once per class id 0..nr_classes-1 on that class's detections (get_class_dets_n_embs,
 * basetracker.py:83-106), every class keeping its own track list, and the rows of the classes are
 * stacked in class order.  KalmanBoxTracker.count is shared by the classes, so the ids of a
 * frame's births ascend in class order.
 *
 * Here class c of sequence s is ENGINE sequence s * C + c of an engine built with S * C
 * sequences.  Per frame, around the engine's own launches over those S * C sequences:
 *   bx_classes_split   a stable counting sort of every sequence's rows by class: class-major
 *                      dets / embs, the (S * C) + 1 offsets the engine takes as det_off, and each
 *                      sorted row's source index.  A row whose class is not an integer in [0, C)
 *                      is dropped.
 *   bx_classes_merge   gives the frame's births their class-global ids (class 0's first, then
 *                      class 1's, ...) from a per-sequence counter, rewrites column 4 of every
 *                      class's output rows through the device-resident map local id -> global id,
 *                      and compacts the classes' rows in class order into the sequence's out rows
 *                      and out_count.  Columns 0-3 and 5-7 are copied as they are: column 7 is what
 *                      the engine wrote for the class call (DeepOCSort: the row's index within the
 *                      class's detections, as the reference's det_ind under per_class).
 * Nothing returns to the host within a frame.
 *
 * The engine's ids are local to an engine sequence and ascend from id0 in birth order; `ids`
 * points at the engines' next-id counters.  The map has a stated capacity, map_cap births per
 * engine sequence: a frame that would pass it latches BX_ERR_CAPACITY and stores nothing for that
 * sequence (out_count 0, class counters and map unchanged).  The engine's own launches have run
 * by then (tracks were born and aged, its id counters advanced), so the class state no longer
 * matches the engine: the sequence is dead after the latch and has to be reset (or the whole run
 * repeated with a larger map_cap), not merely one frame skipped.  The drop-ins grow the map before
 * it can fill.
 *
 * Conventions as in bxassoc.h: pointer arguments are DEVICE pointers unless their name ends in
 * _host, calls are asynchronous on `stream` (NULL = the default stream) unless said otherwise,
 * every function returns a bx_status and bx_last_error carries the text of a failure.
 */
#ifndef BXCLASSES_H
#define BXCLASSES_H

#include <stdint.h>

#include "bxassoc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BX_CLASSES_MAX 1024      /* most classes */
#define BX_CLASSES_ROW_MAX 2048  /* most rows of one sequence in one frame */
#define BX_CLASSES_MAP_CAP 4096  /* the engines' default map_cap */

typedef struct bx_classes bx_classes;

/* State for n_seq sequences of n_classes classes (synchronous).
 *   emb_dim   embedding width F of the split's embs (0: none)
 *   row_cap   most rows one sequence may have in one frame (<= BX_CLASSES_ROW_MAX); a sequence
 *             with more latches BX_ERR_CAPACITY and is split as if it had none
 *   map_cap   births an engine sequence's id map holds
 *   id0       the first id an engine sequence and the class-global counter give out */
int bx_classes_create(int n_seq, int n_classes, int emb_dim, int row_cap, int map_cap, int id0,
                      bx_classes **out);
int bx_classes_destroy(bx_classes *c);
int bx_classes_shape(bx_classes *c, int *n_seq, int *n_classes, int *emb_dim, int *row_cap,
                     int *map_cap, int *id0);
/* The scratch arrays the engines put between split, their launches and merge, sized for n_seq
 * sequences of row_cap rows: s_dets float32 [rows][6], s_off int32 [n_seq * C + 1], s_embs
 * float64 [rows][emb_dim], s_src int32 [rows], s_out float64 [rows][8], s_cnt int32 [n_seq * C]. */
int bx_classes_scratch(bx_classes *c, void **s_dets, void **s_off, void **s_embs, void **s_src,
                       void **s_out, void **s_cnt);
/* Split sequences [0, nseq) of a call: dets float32 [sum n][6] and embs float64 [sum n][emb_dim]
 * (NULL when emb_dim is 0) with det_off int32 [nseq + 1], into o_dets / o_embs (at most as many
 * rows as the input), o_off int32 [nseq * C + 1] starting at 0, and o_src int32 [rows]: the index
 * of each sorted row within its sequence's input rows.  dets and o_dets must be 8-byte aligned. */
int bx_classes_split(bx_classes *c, int nseq, const float *dets, const int32_t *det_off,
                     const double *embs, float *o_dets, double *o_embs, int32_t *o_off,
                     int32_t *o_src, void *stream);
/* Merge sequences [seq0, seq0 + nseq) after the engine's step over engine sequences
 * [seq0 * C, (seq0 + nseq) * C): c_off / c_out / c_cnt are the det_off, out and out_count of that
 * step (call-local, as split wrote c_off); ids[(q) * ids_stride] is the next-id counter of
 * ABSOLUTE engine sequence q.  Sequence seq0 + k's rows go to out + det_off[k] * 8 and
 * out_count[k]. */
int bx_classes_merge(bx_classes *c, int seq0, int nseq, const int32_t *c_off, const double *c_out,
                     const int32_t *c_cnt, const int32_t *ids, int ids_stride,
                     const int32_t *det_off, double *out, int32_t *out_count, void *stream);
/* The device arrays a caller may copy from or to on its own stream: id_counters int32 [n_seq], the
 * class-global next ids, and the latched status (one int32). */
int bx_classes_state(bx_classes *c, void **id_counters, void **status);
/* Forget sequences [seq0, seq0 + nseq): counters back to id0. */
int bx_classes_reset(bx_classes *c, int seq0, int nseq, void *stream);
/* Latched device status (BX_OK or BX_ERR_CAPACITY); synchronises. */
int bx_classes_status(bx_classes *c, int *status);
/* The class-global id counter of a sequence (synchronous). */
int bx_classes_id_count_host(bx_classes *c, int seq, int *id_count);
int bx_classes_set_id_count(bx_classes *c, int seq, int id_count, void *stream);
/* The id map of class cls of sequence seq (synchronous): n = ids given out so far, map_host[k] =
 * the class-global id of local id id0 + k, for k < min(n, cap). */
int bx_classes_map_host(bx_classes *c, int seq, int cls, int cap, int32_t *map_host, int *n);
/* Copy counters, maps and the latched status of `src` into `dst` (same n_seq, n_classes, emb_dim
 * and id0, map_cap and row_cap at least the source's; synchronous). */
int bx_classes_copy_state(bx_classes *dst, bx_classes *src);

#ifdef __cplusplus
}
#endif

#endif /* BXCLASSES_H */
