/*
 * bxcmc.h — C ABI of the camera-motion compensation in libbxassoc.so: the ECC image alignment
 * (Evangelidis & Psarakis 2008, the algorithm behind cv2.findTransformECC) that the reference's
 * motion/cmc/ecc.py runs on every frame, for n_streams independent cameras at once.
 *
 * Reference stage replaced: ECC.apply (motion/cmc/ecc.py:63-128) with BaseCMC.preprocess
 * (base_cmc.py:27-43).  The contract — the integer arithmetic of the preprocessing, the
 * iteration, its exits and the reduction order — is DESIGN.md section 2.14.
 *
 * Conventions as in bxassoc.h: every function returns a bx_status and bx_last_error carries the
 * text of a failure.  Results are deterministic run to run (every sum runs in a fixed order) and
 * a stream's result does not depend on which other streams share the call.
 *
 * Preprocessing (integer, exact):
 *   grey   g = (1868 * B + 9617 * G + 4899 * R + 8192) >> 14            (BGR uint8 input)
 *   size   w = round_half_even(W * scale), h = round_half_even(H * scale); a scale of 0 or >= 1
 *          keeps the frame's size and skips the resize
 *   resize output pixel d of an axis of source length L reads the source coordinate
 *          f = (d + 0.5) / scale - 0.5 (float64): s0 = floor(f), a = f - s0; s0 < 0 gives s0 = 0,
 *          a = 0; s0 >= L - 1 gives s0 = L - 1, a = 0; s1 = min(s0 + 1, L - 1);
 *          q = round_half_even(a * 2048) (an integer 0..2048).  With qx, qy of the two axes
 *          v = (g00 * (2048 - qx) * (2048 - qy) + g01 * qx * (2048 - qy)
 *               + g10 * (2048 - qx) * qy + g11 * qx * qy + (1 << 21)) >> 22   (g01: x1, g10: y1)
 *   grads  gx = 0.5 * (I[x + 1] - I[x - 1]), gy likewise in y, float32, reflect-101 borders
 *          (index -1 reads 1, index L reads L - 2; an axis of length 1 has gradient 0)
 */
#ifndef BXCMC_H
#define BXCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* warp_mode: cv2's MOTION_* values.  BX_ECC_HOMOGRAPHY is refused with BX_ERR_INVALID: no
 * engine takes a 3x3 warp. */
enum { BX_ECC_TRANSLATION = 0, BX_ECC_EUCLIDEAN = 1, BX_ECC_AFFINE = 2, BX_ECC_HOMOGRAPHY = 3 };

/* per-stream result code of an apply */
enum {
  BX_ECC_OK = 0,          /* converged or ran out of iterations: the warp is the estimate */
  BX_ECC_FIRST_FRAME = 1, /* the stream had no previous image: identity */
  BX_ECC_NOT_CONVERGED = 2 /* NaN correlation, singular Hessian or non-positive lambda
                              denominator (cv2's StsNoConv, ecc.py:96-104): identity */
};

/* The solve runs one workgroup of this many threads per stream. */
#define BX_ECC_THREADS 1024

/* Most streams of one handle (a call's frames are one dimension of a launch grid). */
#define BX_ECC_MAX_STREAMS 65535

/* A handle for n_streams <= BX_ECC_MAX_STREAMS cameras whose working images (after the resize)
 * are at most max_h x max_w.  Device memory: n_streams * max_h * max_w * 14 bytes.
 * BX_ERR_INVALID for an argument out of range. */
int bx_ecc_create(int n_streams, int max_h, int max_w, void **out);
int bx_ecc_destroy(void *h);
/* Forget the previous image of one stream (stream < 0: of all). */
int bx_ecc_reset(void *h, int stream, void *hip_stream);
/* Working size of an H x W frame at a scale (the "size" rule above). */
int bx_ecc_work_size(int H, int W, double scale, int *h, int *w);

/* One step of n <= n_streams frames, all launches on hip_stream, no host synchronisation.
 *   frames      device [n][H][W][channels] uint8, channels 3 (BGR) or 1 (grey)
 *   streams     device [n] int32: the stream of each frame, all different; a stream that is not
 *               listed is left untouched (state and outputs)
 *   init_warps  device [n_streams][6] float64 or null: the warp each stream's iteration starts
 *               from, at working scale (null: the identity, as the reference)
 *   warps       device [n_streams][6] float64, row-major 2x3: what the engines' warps take; the
 *               translation column is divided by scale when 0 < scale < 1 (ecc.py:107-109)
 *   rho         device [n_streams] float64: the last correlation computed (0 on a first frame)
 *   iterations  device [n_streams] int32: passes over the image
 *   code        device [n_streams] int32: BX_ECC_OK / FIRST_FRAME / NOT_CONVERGED
 * The new grey image becomes the stream's previous image whatever the code.
 * BX_ERR_CAPACITY (nothing launched, state unchanged): n > n_streams or a working image larger
 * than max_h x max_w.  BX_ERR_INVALID: a null pointer, channels not 1 or 3, a frame smaller than
 * 1 x 1, max_iter < 0, warp_mode unknown or BX_ECC_HOMOGRAPHY.  A stream index out of range
 * skips that frame and latches BX_ERR_INVALID in bx_ecc_status; a frame whose working size
 * differs from its stream's previous image is taken as a first frame and latches BX_ERR_SHAPE. */
int bx_ecc_apply(void *h, int n, int H, int W, int channels, const uint8_t *frames,
                 const int32_t *streams, int warp_mode, double eps, int max_iter, double scale,
                 const double *init_warps, double *warps, double *rho, int32_t *iterations,
                 int32_t *code, void *hip_stream);
/* The same from host arrays: stages the frames, runs, copies the listed streams' entries back
 * and synchronises once.  Also BX_ERR_INVALID (nothing launched) for a stream index out of
 * range or listed twice. */
int bx_ecc_apply_host(void *h, int n, int H, int W, int channels, const uint8_t *frames_host,
                      const int32_t *streams_host, int warp_mode, double eps, int max_iter,
                      double scale, const double *init_warps_host, double *warps_host,
                      double *rho_host, int32_t *iterations_host, int32_t *code_host,
                      void *hip_stream);
/* ---- the chained apply: many consecutive frames of a camera per call.
 *
 * Scratch for max_frames <= BX_ECC_MAX_STREAMS frames per call on an existing handle: per frame
 * a slot with a grey image, its float copy and its two gradients, max_h * max_w * 14 bytes.
 * Idempotent; a larger max_frames grows the scratch (waiting for the device first), a smaller
 * one changes nothing.  The slots carry nothing from one call to the next.  BX_ERR_INVALID for
 * max_frames out of range. */
int bx_ecc_chain_reserve(void *h, int max_frames);

/* n <= max_frames frames in one call, all launches on hip_stream, no host synchronisation.
 *   frames      device [n][H][W][channels] uint8, as bx_ecc_apply
 *   streams     device [n] int32: the stream of each frame.  A stream may repeat: its frames are
 *               adjacent in the call and in time order, so a stream forms at most one group per
 *               call.  A stream listed in two separate groups (0,1,0) is undefined behaviour
 *               (the results and the state of that stream are garbage; the accesses stay in
 *               bounds).
 *   dst         device [n] int64 or null: the row of the four result arrays that frame i writes
 *               (null: row i).  The caller sizes the arrays for the rows it names.
 *   warps       device [.][6] float64; rho [.] float64; iterations, code [.] int32: row dst[i]
 *               holds frame i's result, with the meanings of bx_ecc_apply; other rows are
 *               untouched
 * Frame i is aligned to frame i - 1 of the call when streams[i - 1] == streams[i], otherwise to
 * the stored previous image of its stream: BX_ECC_FIRST_FRAME if there is none, and also (with
 * BX_ERR_SHAPE latched) if its working size is another.  Every iteration starts at the identity
 * (there is no init_warps).  After the call each listed stream's previous image, size and
 * gradients are those of its last frame in the call, whatever the codes.  The results and the
 * final state are, bit for bit, those of n successive bx_ecc_apply calls of one frame each.
 * BX_ERR_CAPACITY (nothing launched, state unchanged): n > max_frames reserved or a working image
 * larger than max_h x max_w.  BX_ERR_INVALID: as bx_ecc_apply.  A stream index out of range
 * skips that frame (its row is untouched) and latches BX_ERR_INVALID in bx_ecc_status. */
int bx_ecc_apply_chain(void *h, int n, int H, int W, int channels, const uint8_t *frames,
                       const int32_t *streams, const int64_t *dst, int warp_mode, double eps,
                       int max_iter, double scale, double *warps, double *rho,
                       int32_t *iterations, int32_t *code, void *hip_stream);
/* The same from host arrays: stages the frames, runs, copies the n result rows back (row i is
 * frame i) and synchronises once.  Also BX_ERR_INVALID (nothing launched) for a stream index out
 * of range or a stream whose frames are not adjacent. */
int bx_ecc_apply_chain_host(void *h, int n, int H, int W, int channels,
                            const uint8_t *frames_host, const int32_t *streams_host,
                            int warp_mode, double eps, int max_iter, double scale,
                            double *warps_host, double *rho_host, int32_t *iterations_host,
                            int32_t *code_host, void *hip_stream);

/* Latched device-side status (BX_OK, BX_ERR_INVALID or BX_ERR_SHAPE); synchronises. */
int bx_ecc_status(void *h, int *status);
/* A stream's state, copied to the host (synchronises): whether it has a previous image, its
 * size, and (each nullable, max_h * max_w entries, the first hh * ww used, row-major) the
 * previous grey image and the gradients of the last frame the stream was given. */
int bx_ecc_state_host(void *h, int stream, int *has_prev, int *hh, int *ww, uint8_t *grey,
                      float *gx, float *gy);

#ifdef __cplusplus
}
#endif
#endif
