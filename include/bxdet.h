/*
 * bxdet.h — C ABI of the detector front end in libbxassoc.so: the two stages around a detector
 * network that are not the network itself.
 *
 * Reference stages replaced: YoloXStrategy.yolox_preprocess (engine/detectors/yolox.py:197-226:
 * one cv2.resize per frame into a padded float64 image, then the normalisation) and the
 * post-process (:249-276): YOLOX's published postprocess (score filter, torchvision's batched NMS)
 * and the rescale to image coordinates.  The network between them is the caller's.  The contract
 * is DESIGN.md section 2.27.
 *
 * Conventions as in bxreid.h: every function returns a bx_status and bx_last_error carries the
 * text of a failure; every launch goes to the caller's stream.  No host synchronisation, no
 * handle, no state.  Results are deterministic and an image's result does not depend on which
 * others share the call.
 *
 * Letterbox of one frame [H][W][3] uint8 into [3][in_h][in_w]:
 *   size     the caller passes rh, rw, the resized size: int(H * r), int(W * r) with
 *            r = min(in_h / H, in_w / W) in float64 (the Python layer computes them)
 *   resize   the top-left rh x rw of the output is the bilinear resize of the whole frame by the
 *            rule of bxreid.h with a ratio per axis (f = (d + 0.5) * L / O - 0.5 in float64, 11-bit
 *            weights, one integer blend): an integer v in 0..255 per channel.  Agreement with
 *            OpenCV's INTER_LINEAR is unmeasured.
 *   padding  every other element is v = 114
 *   colour   swap_rb: output channel c reads source channel 2 - c
 *   norm     float32(((double)v / 255.0 - mean[c]) / std[c]) in float64, cast once (the
 *            reference's padded_img is a float64 array); BX_LB_NO_MEAN / BX_LB_NO_STD leave the
 *            step out; fp16 output is that float32 value rounded once to fp16
 *
 * Post-process of one image's pred [A][5 + C] = cx, cy, w, h, obj, cls_0..cls_{C-1} (fp16 is
 * widened first), all in float32 with every operation rounded once:
 *   corners    x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2
 *   class      cls = the first maximum of cls_k (a NaN counts as a maximum, as torch.max has it);
 *              score = obj * that maximum
 *   candidate  score >= conf_thre (a NaN fails; a score of -0 counts, and is reported, as +0)
 *   order      descending score, ties by ascending row of pred; only the first cand_cap
 *              candidates in that order go on (more: BX_DET_CAND_OVERFLOW)
 *   IoU        area = (x2 - x1) * (y2 - y1); for an earlier a and a later b
 *              iw = pos(min(x2a, x2b) - max(x1a, x1b)), ih likewise, inter = iw * ih,
 *              iou = inter / ((area_a + area_b) - inter), with min(p, q) = q < p ? q : p,
 *              max(p, q) = q > p ? q : p and pos(d) = d > 0 ? d : 0 (so a NaN never wins a
 *              comparison)
 *   NMS        greedy in that order: a kept a suppresses every later b with iou(a, b) > nms_thre,
 *              strictly (0 / 0 = NaN suppresses nothing); without BX_DET_AGNOSTIC only pairs of
 *              equal cls are compared, on the unshifted boxes.  Agreement with torchvision's
 *              coordinate-offset form of batched NMS on borderline pairs is unmeasured.
 *   classes    class_ok, when given, drops survivors of other classes after NMS (they still
 *              suppressed)
 *   rows       [x1 / r, y1 / r, x2 / r, y2 / r, score, (float)cls], each a division; at most
 *              max_det rows per image in that order (more survive: BX_DET_MAX_DET)
 */
#ifndef BXDET_H
#define BXDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags of bx_det_letterbox */
enum {
  BX_LB_HALF = 1,    /* fp16 output */
  BX_LB_SWAP_RB = 2, /* output channel c reads source channel 2 - c (the reference, the default) */
  BX_LB_NO_MEAN = 4, /* no "- mean" step */
  BX_LB_NO_STD = 8   /* no "/ std" step */
};

/* flags of bx_det_postprocess */
enum {
  BX_DET_PRED_HALF = 1, /* pred is fp16 */
  BX_DET_AGNOSTIC = 2   /* compare boxes of different classes too */
};

/* bits of an image's code */
enum { BX_DET_CAND_OVERFLOW = 1, BX_DET_MAX_DET = 2 };

/* the largest cand_cap (the suppression matrix takes cand_cap^2 / 8 bytes per image) */
enum { BX_DET_CAND_MAX = 16384 };

/* All F frames in one launch on hip_stream.
 *   frames  device [F][H][W][3] uint8
 *   rh, rw  the resized size, 1 <= rh <= in_h, 1 <= rw <= in_w
 *   mean, std  float64 per output channel, by value
 *   out     device [F][3][in_h][in_w] float32, or fp16 with BX_LB_HALF
 * BX_ERR_INVALID (nothing launched): a null frames / out, H, W, in_h or in_w < 1, F < 0, rh or
 * rw out of range, a std of 0 or a non-finite mean / std (unless switched off), unknown flag
 * bits, a frame over 2^40 bytes, or more than 2^31 - 1 workgroups.  F == 0 is a valid no-op. */
int bx_det_letterbox(const uint8_t *frames, int F, int H, int W, int in_h, int in_w, int rh,
                     int rw, double mean0, double mean1, double mean2, double std0, double std1,
                     double std2, int flags, void *out, void *hip_stream);

/* Bytes of scratch bx_det_postprocess needs for B images of A rows at cand_cap. */
int bx_det_scratch_bytes(int B, int A, int cand_cap, size_t *bytes);

/* All B images on hip_stream: a memset and five launches, det_off included (a device scan).
 *   pred        device [B][A][5 + C] float32 (fp16 with BX_DET_PRED_HALF); row_stride elements
 *               from row to row (>= 5 + C), img_stride from image to image
 *   class_ok    device [C] int32 or null (every class): non-zero marks a class that is reported
 *   ratio       device [B] float32 or null (1 for every image)
 *   scratch     device, bx_det_scratch_bytes(B, A, cand_cap) bytes, 256-byte aligned, the
 *               call's own until its work on hip_stream is done
 *   dets        device [B * max_det][6] float32: the images' rows one after the other; rows
 *               from det_off[B] on are left as they were
 *   det_off     device [B + 1] int32
 *   anchor_of   device [B * max_det] int32 or null: the row of pred behind each detection
 *   frame_of    device [B * max_det] int32 or null: the image of each detection
 *   code        device [B] int32 or null: BX_DET_CAND_OVERFLOW | BX_DET_MAX_DET
 * BX_ERR_INVALID (nothing launched): a null pred (with A > 0) / scratch / dets / det_off, B or
 * A < 0, C < 1, a stride too small, cand_cap outside 1..BX_DET_CAND_MAX, max_det < 1,
 * B * max_det over 2^31 - 1, a threshold outside [0, 1], unknown flag bits.  B == 0 is a valid
 * no-op. */
int bx_det_postprocess(const void *pred, int B, int A, int C, int64_t row_stride,
                       int64_t img_stride, float conf_thre, float nms_thre,
                       const int32_t *class_ok, const float *ratio, int cand_cap, int max_det,
                       int flags, void *scratch, float *dets, int32_t *det_off,
                       int32_t *anchor_of, int32_t *frame_of, int32_t *code, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
