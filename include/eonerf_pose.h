/* eonerf_pose.h -- camera offset refinement, entry points of libeonerf_hip.so: the gradient of a training step's loss with respect to
 * the ORIGINS of its rays, and its per-image sum.  The reference switches the capability on with --rpc_correction (opt.py:80, "internal
 * bundle adjustment of RPC camera models using offset correction"): a learned 3-D offset per image, added to that image's ray
 * origins; there autograd carries the loss through  positions = origins[ray_indices] + viewdirs * t.
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer,
 * the call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 *
 * The quantity, for a training call (EONERF_F_TRAIN, with or without EONERF_F_SHADOWS / EONERF_F_RGB_LOSS):
 *
 *   d_origins[r, :] =   sum over the camera samples i of ray r of g_cam[i, :]
 *                     + sum over the shadow samples j of ray r of g_sun[j, :]          (EONERF_F_SHADOWS only)
 *   g[., :]         = (W_0^T dY_0 + W_5[:, 256:]^T dY_5) . d enc / d x                 (what the shadow pass' input-gradient tail forms)
 *   d_offsets[j, :] += sum over the rays r with img_idx[r] == j of d_origins[r, :]
 *
 * The shadow term is there because a shadow ray starts at o + depth * d (sat_rendering.py:90); the dependence of depth itself on o
 * runs through the camera samples' d sigma, which dY_0 / dY_5 of the camera pass already hold.  The view direction, near / far and
 * the sun direction are not differentiated.
 *
 * Call order.  eonerf_render_origin_grad is called DIRECTLY BEHIND eonerf_render_backward / eonerf_render_backward_loss, on the same
 * stream, with the same (flat, rays, img_idx, n_rays, flags, ws).  It only READS the render workspace: the camera pass' dY_0 / dY_5,
 * the sample positions, the per-ray offsets and counts and the shadow pass' d sigma / d position; the camera pass' own d position
 * lives in `scratch`.  Nothing of the forward or the backward changes when this call is or is not made: workspace sizes, launch
 * sequences, outputs and parameter gradients are those of a library without it.
 *
 * EONERF_E_STATE, with nothing launched and no output touched, when the call is not behind a completed render backward on that
 * workspace: no backward yet, another call that writes a workspace ran in between (a forward, eonerf_presample, eonerf_set_weights,
 * eonerf_set_noise_seed, a sampler or field call ...), or n_rays / flags / the sample count differ from the backward's.  The call
 * does not use the record up: it may be repeated.
 *
 * Precisions.  fp32 contexts: supported (a reader of the dY rows the weight-gradient GEMM reads).  bf16 contexts on the layer-pipelined
 * path (the training path): supported (the MFMA tail of the shadow pass over the camera pass' tiles).  bf16 contexts whose backward
 * ran on the chain + GEMM path (EONERF_PIPE=0, or after the fault fallback): EONERF_E_UNSUPPORTED.  fp16 x 3 contexts:
 * EONERF_E_UNSUPPORTED, like the backward.
 *
 * Sums are taken in a fixed order -- a ray's samples in index order per lane of its wavefront, lanes in a fixed tree; an image's rays
 * in index order per thread, threads in a fixed tree -- without atomics: results are bit-identical from run to run in every mode.
 */
#ifndef EONERF_POSE_H
#define EONERF_POSE_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_POSE_VERSION 1
int eonerf_pose_version(void);

/* Bytes of `scratch` for a call with these n_rays and flags at the context's current sample count; 0 for a null context, a negative
 * n_rays or a size beyond what the backward itself accepts. */
size_t eonerf_origin_grad_scratch_bytes(const eonerf_ctx* ctx, int n_rays, int flags);

/* d_origins[n_rays * 3] is OVERWRITTEN (a ray without samples: exactly 0); d_offsets[n_images * 3] is ACCUMULATED INTO (rows of images
 * without a ray in the batch are not written).  Either may be NULL, not both.  img_idx[n_rays] indexes the rows of d_offsets.
 * EONERF_E_ARG: a null ctx / flat / rays / img_idx / ws / scratch, n_rays < 0, both outputs null.  EONERF_E_STATE: flags without
 * EONERF_F_TRAIN or with EONERF_F_ONLY_DEPTH, and the order rule above.  EONERF_E_WORKSPACE: ws_bytes or scratch_bytes too small.
 * n_rays == 0 succeeds and writes nothing. */
int eonerf_render_origin_grad(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx, int n_rays, int flags,
                              const void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                              float* d_origins, float* d_offsets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
