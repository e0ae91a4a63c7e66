/* eonerf_sweep.h -- sun sweep, entry points of libeonerf_hip.so: one view rendered under K sun directions from ONE camera pass
 * (shadow maps over a day, relit views, sun-exposure maps on a DSM grid).
 *
 * Nothing in the camera pass of eonerf_render_forward depends on the sun: the sampler, the full forward chain with the albedo and
 * transient heads, depth, albedo, transient_s, beta and the sample counts.  Only the ambient head (once per ray), the shadow ray's
 * sample count, the shadow pass and the final shading do.  The sweep runs the former once and the latter once per sun.
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer
 * (the workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 */
#ifndef EONERF_SWEEP_H
#define EONERF_SWEEP_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_SWEEP_VERSION 1
int eonerf_sweep_version(void);

/* Bytes of the workspace eonerf_render_sun_sweep needs for n_rays rays under the context's current sample count: the layout of
 * eonerf_render_workspace_bytes(ctx, n_rays, EONERF_F_SHADOWS) followed by one copy of the ray table.  It does not depend on n_suns
 * (the parameter is kept so that a later layout may use it).  0 for a null context, n_rays < 0, n_suns < 1 or a batch beyond the
 * sweep's ray bound (below). */
size_t eonerf_sun_sweep_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int n_suns);

/* rays [n_rays][11], img_idx, zsteps, u_cam, u_retry: as eonerf_render_forward.
 * u_sun [n_suns][n_rays][n_samples] jitter of the shadow passes, or NULL exactly when u_cam is NULL (Philox mode).
 * suns [n_suns][3] fp32, device: what columns 8..10 of a normalised ray table hold (unit vectors; columns 8..10 of `rays` are not read).
 * flags: EONERF_F_EVAL or 0; EONERF_F_SHADOWS is implied.
 * out [n_suns][n_rays][21]; n_samples_dev: the camera pass's sample count, as eonerf_render_forward (may be NULL).
 *
 * Contract.  For every k, out[k] holds the same 21 x n_rays fp32 words, bit for bit, as
 * eonerf_render_forward(flags | EONERF_F_SHADOWS) would write on the same context, weights and sample count for a ray table equal to
 * `rays` with columns 8..10 of every row replaced by suns[k], with the same u_cam and u_retry, and u_sun[k] as its u_sun -- in every
 * precision (fp32, bf16, fp16x3): the same kernels see the same inputs.  Columns 3:7 and 11:15 (depth, albedo, transient_s, beta,
 * entropy, pts_per_ray) are equal for every k.
 *
 * Philox mode (u_cam == NULL): the call takes ONE call number of the context's jitter stream; every sun's shadow pass draws under
 * it, as the shadow pass of eonerf_render_forward draws under its camera pass's number.  out[0] is what eonerf_render_forward gives
 * from the same seed and call count.
 *
 * A pending eonerf_presample record is dropped, as eonerf_render_forward drops one it does not consume.  eonerf_range_status keeps
 * working for fp16x3 contexts.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null ctx / flat_params / rays / img_idx / zsteps / suns / out / ws, n_suns < 1, n_rays < 0, u_retry or u_sun
 *                         with a null u_cam, a null u_sun with a u_cam
 *   EONERF_E_STATE        weights not set
 *   (EONERF_OK            n_rays == 0)
 *   EONERF_E_UNSUPPORTED  EONERF_F_TRAIN or EONERF_F_ONLY_DEPTH in flags
 *   EONERF_E_UNSUPPORTED  n_rays x (n_samples - 1) > INT_MAX - 255 (formed in 64 bits), or beyond eonerf_render_forward's own bound
 *   EONERF_E_WORKSPACE    ws_bytes < eonerf_sun_sweep_workspace_bytes() */
int eonerf_render_sun_sweep(eonerf_ctx* ctx, const float* flat_params, const float* rays, const int64_t* img_idx, const float* zsteps,
                            const float* u_cam, const float* u_retry, const float* u_sun, const float* suns, int n_suns, int n_rays,
                            int flags, float* out, int* n_samples_dev, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
