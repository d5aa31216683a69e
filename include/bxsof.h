/*
 * bxsof.h — C ABI of the sparse-optical-flow camera-motion compensation in libbxassoc.so: the
 * stage the reference's motion/cmc/sof.py hands to goodFeaturesToTrack, calcOpticalFlowPyrLK and
 * estimateAffinePartial2D on every frame, for n_streams independent cameras at once.
 *
 * Reference stage replaced: SOF.apply (motion/cmc/sof.py:64-160) with BaseCMC.preprocess
 * (base_cmc.py:27-43).  The contract is DESIGN.md section 2.17; this header repeats its
 * arithmetic.  Conventions as in bxassoc.h and bxcmc.h: every function returns a bx_status,
 * results are deterministic run to run and a stream's result does not depend on which other
 * streams share the call.  Pyramids and keypoints live on the device.
 *
 * Per stream, at working size h x w (everything "reflect-101": index -k reads k, index
 * n - 1 + k reads n - 1 - k, repeated for an axis shorter than the reach):
 *
 * 1 preprocessing  exactly bxcmc.h's integer grey and resize rule.
 * 2 pyramid        level 0 is the working image; level l + 1 has ((n + 1) / 2) pixels per axis:
 *                  pixel (x, y) is (sum_{i,j} k[i] k[j] L_l(2x + j - 2, 2y + i - 2) + 128) >> 8 with
 *                  k = [1 4 6 4 1], reflect-101, integer.  Level l >= 1 is built while l <=
 *                  max_level and both its sides exceed win_size.
 * 3 keypoints      Sobel 3x3 Dx = (R(-1) + 2 R(0) + R(+1)) with R(j) = I(x + 1, y + j) -
 *                  I(x - 1, y + j), Dy likewise; a = sum Dx^2, b = sum Dx Dy, c = sum Dy^2 over
 *                  the 3x3 block (int32, exact, reflect-101 at both steps: the derivative plane
 *                  is reflected); lambda = 0.5 (a + c) - sqrt(0.25 (a - c)^2 + b^2), float64.
 *                  Candidates: 1 <= x <= w - 2, 1 <= y <= h - 2, lambda > 0, lambda >=
 *                  quality_level * max lambda (the maximum over the whole image), lambda >= each
 *                  of its eight neighbours.  Keypoints: the first max_corners candidates by
 *                  lambda descending, then pixel index y w + x ascending; pixel centres, no
 *                  sub-pixel refinement.
 * 4 tracking       per keypoint p, from the coarsest built level L down to 0: p_l = p * 2^-l;
 *                  the new position q starts at p_L and is doubled on the way down.  With half =
 *                  (win - 1) / 2 a window anchored at t (t = p_l - half, or q - half) has the
 *                  integer corner (fx, fy) = floor(t), fractions (ax, ay) = t - floor(t) and lies
 *                  inside when 0 <= fx, fx + win <= w_l - 1, 0 <= fy, fy + win <= h_l - 1.  A
 *                  sample at window pixel (i, j) is ((w00 v00 + w01 v01) + w10 v10) + w11 v11 with
 *                  w00 = (1 - ax)(1 - ay), w01 = ax (1 - ay), w10 = (1 - ax) ay, w11 = ax ay and
 *                  v00 at (fx + j, fy + i), v01 one to the right, v10 one down.  Template I, Ix, Iy:
 *                  the previous level and its Scharr derivatives Ix = 3 R(-1) + 10 R(0) + 3 R(+1)
 *                  (reflect-101, int32) sampled this way; G = sum [Ix^2, Ix Iy; Ix Iy, Iy^2].
 *                  The level fails when a window is not inside, when
 *                  (0.5 (Gxx + Gyy) - sqrt(0.25 (Gxx - Gyy)^2 + Gxy^2)) / (2^20 win^2) < 1e-4, or
 *                  when det = Gxx Gyy - Gxy^2 is not positive.  Iterations j = 0 .. max_iter - 1:
 *                  the window at q must be inside (else the level fails), J sampled from the new
 *                  level, b = sum 32 (J - I) [Ix, Iy] (32: the gain of the Scharr kernel, which
 *                  the image difference has to carry too), delta = -G^-1 b = ((Gxy b2 - Gyy b1) /
 *                  det, (Gxy b1 - Gxx b2) / det), q += delta; stop when delta . delta <= eps^2; when
 *                  j > 0 and |delta + previous delta| < 0.01 on both axes, q -= 0.5 delta and stop.
 *                  A level that fails loses the point at level 0 and is left (q as it stands)
 *                  otherwise.  After level 0 the point is also lost unless 0 <= q.x <= w - 1 and
 *                  0 <= q.y <= h - 1.  Every window sum: lane r of a 64-lane wave adds window
 *                  pixels r, r + 64, ... (row-major) in ascending order, then the 64 partial
 *                  sums go through the descending xor butterfly (distance 32, 16, ..., 1).
 * 5 fit            m tracked pairs (p_n, q_n) in keypoint order.  m < 4: BX_SOF_TOO_FEW.  Else
 *                  BX_SOF_HYPOTHESES hypotheses k: i = mix(2k) mod m, j = mix(2k + 1) mod m,
 *                  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
 *                  x ^= x >> 16 (uint32).  Skipped when p_i == p_j.  With d = p_j - p_i, e = q_j -
 *                  q_i, n2 = d.x d.x + d.y d.y: a = (d.x e.x + d.y e.y) / n2, b = (d.x e.y - d.y
 *                  e.x) / n2, tx = q_i.x - (a p_i.x - b p_i.y), ty = q_i.y - (b p_i.x + a p_i.y).
 *                  Inlier: rx = ((a p.x - b p.y) + tx) - q.x, ry = ((b p.x + a p.y) + ty) - q.y,
 *                  rx rx + ry ry <= threshold^2.  Winner: most inliers, lowest k on ties.  The
 *                  warp is the least-squares similarity over the winner's inliers (means, then
 *                  centred sums: a = sum(p~ . q~) / sum |p~|^2, b = sum(p~ x q~) / sum |p~|^2,
 *                  t = mean q - [a -b; b a] mean p; sums in the wave order of step 4 over the
 *                  tracked pairs).  No usable hypothesis (or a zero denominator): BX_SOF_NO_MODEL.
 * 6 state          the new pyramid becomes the previous one; the keypoints are detected again
 *                  on the new frame; if it has none the tracked points q are kept.
 */
#ifndef BXSOF_H
#define BXSOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-stream result code of an apply */
enum {
  BX_SOF_OK = 0,           /* the warp is the estimate */
  BX_SOF_FIRST_FRAME = 1,  /* the stream had no previous frame: identity, keypoints detected */
  BX_SOF_TOO_FEW = 2,      /* fewer than 4 points tracked (sof.py:122-132): identity */
  BX_SOF_NO_MODEL = 3,     /* no usable hypothesis: identity */
  BX_SOF_NO_KEYPOINTS = 4  /* a first frame without a corner: identity, the stream stays
                              uninitialised (sof.py:93-94) */
};

#define BX_SOF_MAX_STREAMS 65535
#define BX_SOF_MAX_CORNERS 1024 /* most keypoints of a stream */
#define BX_SOF_MAX_LEVELS 4     /* pyramid levels 0 .. 3 */
#define BX_SOF_HYPOTHESES 256   /* hypotheses of the consensus fit */

typedef struct bx_sof_params {
  int32_t max_corners;    /* 1 .. BX_SOF_MAX_CORNERS (reference: 1000) */
  int32_t win_size;       /* odd, 5 .. 31 (21) */
  int32_t max_level;      /* 0 .. BX_SOF_MAX_LEVELS - 1 (3) */
  int32_t max_iter;       /* >= 0 (30) */
  double quality_level;   /* (0, 1] (0.01) */
  double eps;             /* >= 0 (0.01) */
  double threshold;       /* consensus threshold in working pixels, > 0 (3.0) */
  double scale;           /* bxcmc.h's scale: 0 or >= 1 keeps the frame's size */
} bx_sof_params;

/* A handle for n_streams cameras whose working images are at most max_h x max_w.  Device memory:
 * about n_streams * max_h * max_w * 24 bytes.  BX_ERR_INVALID for an argument out of range. */
int bx_sof_create(int n_streams, int max_h, int max_w, void **out);
int bx_sof_destroy(void *h);
/* Forget the previous frame of one stream (stream < 0: of all). */
int bx_sof_reset(void *h, int stream, void *hip_stream);
/* The level rule of step 2: the number of levels of an h x w working image and their sizes
 * (lh, lw: BX_SOF_MAX_LEVELS entries each). */
int bx_sof_levels(int h, int w, int win_size, int max_level, int *n_levels, int *lh, int *lw);

/* One step of n <= n_streams frames, all launches on hip_stream, no host synchronisation.
 *   frames, streams   as bx_ecc_apply
 *   warps        device [n_streams][6] float64, row-major 2x3 [a -b tx; b a ty], previous-frame
 *                coordinates to new-frame coordinates; the translation column is divided by
 *                scale when 0 < scale < 1 (sof.py:145-147)
 *   code         device [n_streams] int32: BX_SOF_*
 *   n_keypoints  device [n_streams] int32: keypoints the stream holds after the call
 *   n_tracked    device [n_streams] int32: points tracked into this frame (0 on a first frame)
 *   n_inliers    device [n_streams] int32: inliers of the winning hypothesis (0 unless OK)
 * A stream that is not listed is left untouched (state and outputs).  BX_ERR_CAPACITY (nothing
 * launched, state unchanged): n > n_streams or a working image larger than max_h x max_w.
 * BX_ERR_INVALID: a null pointer, channels not 1 or 3, a parameter out of range.  A stream index
 * out of range skips that frame and latches BX_ERR_INVALID in bx_sof_status; a frame whose working
 * size or level count differs from its stream's previous frame is taken as a first frame and
 * latches BX_ERR_SHAPE. */
int bx_sof_apply(void *h, int n, int H, int W, int channels, const uint8_t *frames,
                 const int32_t *streams, const bx_sof_params *params, double *warps,
                 int32_t *code, int32_t *n_keypoints, int32_t *n_tracked, int32_t *n_inliers,
                 void *hip_stream);
/* The same from host arrays: stages the frames, runs, copies the listed streams' entries back
 * and synchronises once.  Also BX_ERR_INVALID (nothing launched) for a stream index out of range
 * or listed twice. */
int bx_sof_apply_host(void *h, int n, int H, int W, int channels, const uint8_t *frames_host,
                      const int32_t *streams_host, const bx_sof_params *params,
                      double *warps_host, int32_t *code_host, int32_t *n_keypoints_host,
                      int32_t *n_tracked_host, int32_t *n_inliers_host, void *hip_stream);
/* ---- the chained apply: many consecutive frames of a camera per call.
 *
 * Scratch for max_frames <= BX_SOF_MAX_STREAMS frames per call on an existing handle: per frame a
 * slot with what a stream holds while one frame is in flight: a pyramid (bx_sof_pyramid_bytes,
 * about 4/3 max_h * max_w), the lambda plane and the candidate scratch (max_h * max_w * 20 bytes),
 * the keypoints with their count and a tracking record (BX_SOF_MAX_CORNERS * 54 bytes), 28 bytes
 * of scalars: max_h * max_w * 21.4 + 55 324 bytes per slot, and 68 bytes of staging for the host
 * entry.  Idempotent; a larger max_frames grows the scratch (waiting for the device first), a
 * smaller one changes nothing.  The slots carry nothing from one call to the next.
 * BX_ERR_INVALID for max_frames out of range. */
int bx_sof_chain_reserve(void *h, int max_frames);

/* n <= max_frames frames of one H x W in one call, all launches on hip_stream, no host
 * synchronisation.
 *   frames      device [n][H][W][channels] uint8, as bx_sof_apply
 *   streams     device [n] int32: the stream of each frame.  A stream may repeat: its frames are
 *               adjacent in the call and in time order, so a stream forms at most one group per
 *               call.  A stream listed in two separate groups (0,1,0) is undefined behaviour (the
 *               results and the state of that stream are garbage; the accesses stay in bounds).
 *   dst         device [n] int64 or null: the row of the five result arrays that frame i writes
 *               (null: row i).  The caller sizes the arrays for the rows it names.
 *   warps       device [.][6] float64; code, n_keypoints, n_tracked, n_inliers [.] int32: row
 *               dst[i] holds frame i's result, with the meanings of bx_sof_apply; other rows are
 *               untouched
 * Frame i is tracked from frame i - 1 of the call when streams[i - 1] == streams[i], otherwise
 * from the stored state of its stream: a first frame if there is none, and also (with BX_ERR_SHAPE
 * latched) if its working size or level count is another, with bx_sof_apply's codes.  After the
 * call each listed stream's state (previous pyramid, size, level count, keypoints, lambda plane,
 * tracking record, whether it has a previous frame) is that of its last frame in the call.  The
 * five results and the final state, as bx_sof_state_host and bx_sof_points_host show it, are bit
 * for bit those of n successive bx_sof_apply calls of one frame each; this includes a frame
 * without a corner that keeps the tracked points, a first frame without a corner, and runs of
 * them anywhere in a call.
 * BX_ERR_CAPACITY (nothing launched, state unchanged): n > max_frames reserved or a working image
 * larger than max_h x max_w.  BX_ERR_INVALID: as bx_sof_apply.  A stream index out of range
 * skips that frame (its rows are untouched) and latches BX_ERR_INVALID in bx_sof_status. */
int bx_sof_apply_chain(void *h, int n, int H, int W, int channels, const uint8_t *frames,
                       const int32_t *streams, const int64_t *dst, const bx_sof_params *params,
                       double *warps, int32_t *code, int32_t *n_keypoints, int32_t *n_tracked,
                       int32_t *n_inliers, void *hip_stream);
/* The same from host arrays: stages the frames, runs, copies the n result rows back (row i is
 * frame i) and synchronises once.  Also BX_ERR_INVALID (nothing launched) for a stream index out
 * of range or a stream whose frames are not adjacent. */
int bx_sof_apply_chain_host(void *h, int n, int H, int W, int channels,
                            const uint8_t *frames_host, const int32_t *streams_host,
                            const bx_sof_params *params, double *warps_host, int32_t *code_host,
                            int32_t *n_keypoints_host, int32_t *n_tracked_host,
                            int32_t *n_inliers_host, void *hip_stream);

/* Latched device-side status (BX_OK, BX_ERR_INVALID or BX_ERR_SHAPE); synchronises. */
int bx_sof_status(void *h, int *status);
/* Bytes of one stream's pyramid buffer (the levels one after another, level 0 first). */
int bx_sof_pyramid_bytes(void *h, size_t *bytes);
/* A stream's state, copied to the host (synchronises): whether it has a previous frame, its
 * levels and their sizes (BX_SOF_MAX_LEVELS entries each), and (each nullable) the pyramid
 * (bx_sof_pyramid_bytes bytes, level l row-major at the sum of the sizes before it), the keypoint
 * count, the keypoints (2 * BX_SOF_MAX_CORNERS doubles, x then y per point) and the lambda plane of
 * the last frame the stream was given (max_h * max_w doubles, the first h * w used). */
int bx_sof_state_host(void *h, int stream, int *has_prev, int *n_levels, int *lh, int *lw,
                      uint8_t *pyramid, int *n_keypoints, double *keypoints, double *lam);
/* The tracking record of a stream's last apply (synchronises): the n points that were tracked
 * from, in keypoint order (arrays of BX_SOF_MAX_CORNERS entries, points x then y): their
 * positions, the positions found, tracked flags, iterations summed over the levels, the winning
 * hypothesis' inlier flags, and its index (-1 without one). */
int bx_sof_points_host(void *h, int stream, int *n, double *prev, double *next, uint8_t *tracked,
                       int32_t *iterations, uint8_t *inlier, int *winner);

#ifdef __cplusplus
}
#endif
#endif
