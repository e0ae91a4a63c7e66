/* eonerf_march.h -- block-wise early ray termination for export renders, entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer
 * (the workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 *
 * A pass (camera or shadow) of eonerf_render_forward runs every valid sample of every ray through the field.  The march runs a pass in
 * ROUNDS of `block` sampler slots -- per round one sampler launch, one chain launch, one compositing launch over the rays still alive --
 * and a ray whose transmittance has fallen below early_stop_eps drops out of all later rounds.  Nothing leaves the device between
 * rounds; a round in which no ray is alive costs its launches only.
 *
 * THE RULE, for one pass of one ray with ns = n_samples.
 *   Validity.  The slots are i = 0 .. ns - 2.  valid(i) is eonerf_render_forward's rule: the cube filter and, while a grid is set on the
 *     context (eonerf_occ.h), its culling rule, "the last cube-valid sample is kept" included.  sd_i = sigma_i * delta_i with the dense
 *     call's delta_i; on the camera pass the ray's last valid slot -- of the whole ray, not of a round -- ends at 1e10.
 *   Rounds.  Round j covers slots [j * block, (j + 1) * block).  OD_j = the sum of sd_i over valid i < j * block.  The ray is alive in
 *     round 0; it is alive in round j > 0 iff it was alive in round j - 1 and exp(-OD_j) >= early_stop_eps.  KEPT samples are the
 *     valid slots of alive rounds; all kept samples of a round contribute, also those behind the point inside the round where the
 *     transmittance crosses early_stop_eps.
 *   Weights.  w_i = exp(-(sum of sd over the kept slots in front of i)) * (1 - exp(-sd_i)) for kept slots, 0 otherwise.  The per-ray
 *     sums are the dense ones over these weights: depth, albedo, transient scalar, beta (+ 0.05), weight sum.
 *   geo_shadows is the exclusive transmittance at the shadow ray's last valid sample if that sample was kept; otherwise exp(-OD_j*)
 *     at the boundary j* where the ray died (< early_stop_eps); 1 for a ray without samples.
 *   Columns 14 and 15 (pts_per_ray, sc_pts_per_ray) are what the dense call with the same grid writes: the FULL count of the first
 *     draw, and the full count of the shadow ray that starts at the march's depth.  The kept counts go to n_samples_dev (summed over
 *     the camera pass) and to `kept`.
 *   "Resample if any ray is empty" is decided on the full counts of the first draw, as in the dense call.  The Philox call numbering
 *     is the dense call's: one call number per render, the shadow pass draws under its camera pass's number.
 *   early_stop_eps = 0 keeps everything: the result is the dense render up to the order of the fp32 sums.  A terminated ray misses a
 *     total weight of exp(-OD_j*) < eps, so against the eps = 0 result of the same call the camera columns move by at most
 *         |depth| <= 2 eps;   |albedo|, |transient_s|, |weight sum| <= eps;   |beta| <= eps * max(transient beta).
 */
#ifndef EONERF_MARCH_H
#define EONERF_MARCH_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_MARCH_VERSION 1
int eonerf_march_version(void);

/* Bytes of the workspace of eonerf_render_forward_march / eonerf_march_sample_round: a layout of its own (per-ray sampler results and
 * march state, then the buffers of one round: n_rays x block sample slots).  0 for a null context, n_rays < 0 or a block size other
 * than 16, 32, 64. */
size_t eonerf_march_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int flags, int block);

/* eonerf_render_forward by the rule above.  Arguments and their rules are eonerf_render_forward's (flags: EONERF_F_SHADOWS,
 * EONERF_F_EVAL, EONERF_F_ONLY_DEPTH; noise buffers or in-kernel Philox); the occupancy grid set on the context is honoured as by an
 * inference forward.  n_samples_dev (may be NULL) receives the number of kept camera samples; kept (may be NULL) is int [2][n_rays]:
 * the kept samples per ray of the camera pass and, with EONERF_F_SHADOWS, of the shadow pass (row 1 is not written otherwise).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null ctx / flat_params / rays / img_idx / zsteps / out / workspace, n_rays < 0
 *   EONERF_E_STATE        weights not set
 *   EONERF_E_UNSUPPORTED  EONERF_F_TRAIN
 *   EONERF_E_ARG          early_stop_eps outside [0, 1) or NaN
 *   EONERF_E_ARG          block not in {16, 32, 64}
 *   (n_rays == 0 returns EONERF_OK here)
 *   EONERF_E_ARG          noise buffers that do not fit together (as eonerf_render_forward)
 *   EONERF_E_UNSUPPORTED  more rays than a call takes (as eonerf_render_forward)
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_march_workspace_bytes(ctx, n_rays, flags, block) */
int eonerf_render_forward_march(eonerf_ctx* ctx, const float* flat_params, const float* rays, const int64_t* img_idx, const float* zsteps,
                                const float* u_cam, const float* u_retry, const float* u_sun, int n_rays, int flags,
                                float early_stop_eps, int block, float* out /* [n_rays][21] */, int* n_samples_dev, int* kept,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The march's sampler alone, the counterpart of eonerf_occ_sample_rays: the valid samples of slots [round * block, (round + 1) * block)
 * of the rays with alive[ray] != 0 (alive == NULL: all), compact in ray order; every sample is bit-equal to the one eonerf_sample_rays
 * (with a grid set on the context: eonerf_occ_sample_rays with that grid) returns for that slot.  *n_out (device int) receives their
 * number; ray_indices, t_starts and t_ends hold at least n_rays x min(block, n_samples - 1) elements.  Workspace:
 * eonerf_march_workspace_bytes(ctx, n_rays, EONERF_F_ONLY_DEPTH, block).
 * EONERF_E_ARG: a null ctx / rays / zsteps / ray_indices / t_starts / t_ends / n_out / workspace, n_rays < 0, round < 0 or beyond the
 * last round, block not in {16, 32, 64}; EONERF_E_WORKSPACE: a short workspace. */
int eonerf_march_sample_round(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays,
                              int round, int block, const int* alive, int64_t* ray_indices, float* t_starts, float* t_ends, int* n_out,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
