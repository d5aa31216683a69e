/*
 * bxreid.h — C ABI of the ReID front end in libbxassoc.so: the two stages between an image and
 * the embeddings the appearance trackers take that are not the network itself.
 *
 * Reference stages replaced: BaseModelBackend.get_crops (appearance/backends/base_backend.py:34-73:
 * one cv2.resize and one host-to-device copy per box, then the batch normalisation) and the
 * division by np.linalg.norm in get_features (:84).  The network between them is the caller's.
 * The contract is DESIGN.md section 2.15.
 *
 * Conventions as in bxcmc.h: every function returns a bx_status and bx_last_error carries the
 * text of a failure; every launch goes to the caller's stream.  No host synchronisation, no
 * handle, no state.  Results are deterministic and a box's (a row's) result does not depend on
 * which others share the call.
 *
 * Crop of one box (x1, y1, x2, y2 float32) from its frame [H][W][3] uint8:
 *   corners  each coordinate is rounded half to even in float32 (numpy's round), clamped in
 *            floating point to [0, W] (x) or [0, H] (y), then converted to int: the reference's
 *            x1 = max(0, x1), x2 = min(W, x2), ...; the crop is rows y1..y2-1, columns x1..x2-1
 *   empty    a non-finite coordinate, x2 <= x1 or y2 <= y1 after the clamp, or a frame index
 *            outside 0..F-1: code BX_CROP_EMPTY and an all-zero row (cv2.resize raises there)
 *   resize   bilinear per channel by the rule of bxcmc.h with a ratio per axis: output index d of
 *            an axis of crop length L and output length O reads f = (d + 0.5) * L / O - 0.5
 *            (float64, left to right); s0, s1, the border clamps, q = round_half_even(a * 2048)
 *            and the (... + (1 << 21)) >> 22 blend are bxcmc.h's.  Agreement with OpenCV's
 *            INTER_LINEAR is unmeasured.
 *   colour   swap_rb: output channel c reads source channel 2 - c (BGR -> RGB)
 *   norm     float32: ((float)v / 255.0f - mean[c]) / std[c], every operation rounded once
 *            half:    h = fp16((float)v / 255.0f); fp16(((float)h - mean[c]) / std[c])
 *            (c is the output channel) — what the framework's crops / 255.0 and
 *            (crops - mean) / std compute on float32 mean / std tensors
 *
 * Feature rows: out[i][k] = (float)in[i][k] / sqrtf(S_i), S_i numpy's float32 pairwise sum of the
 * float32 squares of row i (np.linalg.norm(x, axis=-1)).  fp16 input is widened to float32 first:
 * the float16 norm numpy would take of a float16 array is not reproduced.
 */
#ifndef BXREID_H
#define BXREID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-box result code of bx_reid_crops */
enum { BX_CROP_OK = 0, BX_CROP_EMPTY = 1 };

/* flags of bx_reid_crops */
enum {
  BX_CROP_HALF = 1,   /* fp16 output */
  BX_CROP_NHWC = 2,   /* [n][out_h][out_w][3] instead of [n][3][out_h][out_w] */
  BX_CROP_SWAP_RB = 4 /* output channel c reads source channel 2 - c (BGR frames, RGB crops:
                         what the reference does, and the Python default) */
};

/* All n boxes of all frames in one launch on hip_stream.
 *   frames    device [F][H][W][3] uint8
 *   boxes     device [n][4] float32 xyxy
 *   frame_of  device [n] int32 or null (every box belongs to frame 0)
 *   mean, std float32 per output channel, by value
 *   out       device [n][3][out_h][out_w] (BX_CROP_NHWC: [n][out_h][out_w][3]) float32, or fp16
 *             with BX_CROP_HALF
 *   code      device [n] int32 or null: BX_CROP_OK / BX_CROP_EMPTY
 * BX_ERR_INVALID (nothing launched): a null frames / boxes / out, F, H, W, out_h or out_w < 1,
 * n < 0, a std of 0 (or a non-finite mean / std), unknown flag bits, a frame side over 2^24 (the
 * corners are clamped in float32) or a frame over 2^40 bytes, or more than 2^31 - 1 workgroups
 * (n times the row tiles of a crop).  n == 0 is a valid no-op. */
int bx_reid_crops(const uint8_t *frames, int F, int H, int W, const float *boxes,
                  const int32_t *frame_of, int n, int out_h, int out_w, float mean0, float mean1,
                  float mean2, float std0, float std1, float std2, int flags, void *out,
                  int32_t *code, void *hip_stream);

/* in [n][F] (float32, or fp16 when in_half; in_stride elements from row to row, >= F) to the
 * contiguous out [n][F] (float32, or float64 when out_f64: the exact widening of the float32
 * quotient).  One wave per row.  A zero row gives NaN, as numpy does.
 * BX_ERR_INVALID: a null pointer, F < 1, n < 0 or in_stride < F.  n == 0 is a valid no-op. */
int bx_reid_normalize(const void *in, int in_half, int64_t in_stride, int n, int F, void *out,
                      int out_f64, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
