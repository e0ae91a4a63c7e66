/* eonerf_quantile.h -- quantile depth of export renders (the median surface and its confidence band), entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer
 * (the workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 *
 * The expected depth sum(w * mid) of eonerf_render_forward moves with every small weight a ray collects in front of and behind the
 * surface.  The quantile depth t_q is the distance at which the ray's accumulated opacity 1 - exp(-optical depth) crosses q: it is
 * decided by the samples in front of the crossing alone.  q = 0.5 is the median surface, (0.16, 0.84) a confidence band around it.
 *
 * THE RULE, for one camera ray of one call.
 *   k = 0 .. n - 1 are the samples the EONERF_F_ONLY_DEPTH inference forward composites for that ray, in slot order: after the cube
 *     filter, after the occupancy rule while a grid is set on the context (eonerf_occ.h), of the draw that rendered (the first draw, or
 *     the retry draw under "resample if any ray is empty").
 *   ts_k, te_k   the sampler's interval ends; te of the last sample is the sampler's own value here, not 1e10.
 *   sigma_k      the density the forward's density chain gives.
 *   sd_k = sigma_k * delta_k with the forward's delta: the ray's last valid slot ends at 1e10.
 *   E_k = the exclusive prefix sum of sd, I_k = E_k + sd_k.
 *   For a quantile q in (0, 1):  L_q = (float)(-log1p(-(double)q)).
 *   The bracket b is the first k with I_k >= L_q; then sigma_b > 0 and
 *       t_q = ts_b + min(max((L_q - E_b) / sigma_b, 0), te_b - ts_b)       in fp32 operations, without contraction.
 *   If no k qualifies (all density zero to the end): t_q = te_{n-1}.  A ray without samples gives 0 in every column.
 *   The rule works on optical depths only: no exp is involved.
 *
 * OUTPUT  out[n_rays][2 + n_q]:
 *   column 0        the expected depth;
 *   column 1        od_front, the optical depth in front of whatever ended the ray: E_{n-1}, or -- march mode, a ray that died at a
 *                   round boundary -- the OD_j* of that boundary (eonerf_march.h).  It tells how much of the ray was absorbed before the
 *                   forced-opaque last sample;
 *   columns 2 ..    t_q in the order of the quantiles.
 *
 * DENSE MODE (early_stop_eps == 0; `block` is ignored).  One sampler launch, one density-chain launch -- both eonerf_render_forward's own,
 *   with its EONERF_F_ONLY_DEPTH arguments -- and one compositing launch.  Column 0 and n_samples_dev are bit-equal to
 *   eonerf_render_forward(... EONERF_F_ONLY_DEPTH ...) on the same inputs.
 * MARCH MODE (early_stop_eps > 0).  The pass runs in rounds of `block` sampler slots by eonerf_march.h's rule, unchanged (validity,
 *   alive, kept, the patched last slot).  Column 0 carries the march's bound, 2 eps against dense.  A quantile is written in the round
 *   with OD_j < L_q <= OD_{j+1}; the call is refused unless L_qmax * (1 + 1e-4) < -log(eps) (in double), so every requested bracket lies
 *   among the kept samples -- early termination does not move a quantile beyond the order of the fp32 sums.
 */
#ifndef EONERF_QUANTILE_H
#define EONERF_QUANTILE_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_QUANTILE_VERSION 1
int eonerf_quantile_version(void);

/* Bytes of the workspace of eonerf_render_depth_quantiles.  block == 0: the dense layout; 16, 32, 64: the march layout of that block.
 * 0 for a null context, n_rays < 0 (or more rays than a call takes), n_q outside 1 .. 8 or any other block. */
size_t eonerf_quantile_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int n_q, int block);

/* Expected depth, od_front and n_q quantile depths of n_rays camera rays by the rule above.  rays, zsteps, u_cam, u_retry: as
 * eonerf_render_forward (noise buffers or in-kernel Philox; the call uses ONE Philox call number).  quantiles: HOST float[n_q], strictly
 * increasing, each in (0, 1).  The occupancy grid set on the context is honoured as by an inference forward.  n_samples_dev (may be
 * NULL) receives the number of composited (march: kept) samples.  s_ray (int64), s_ts, s_te, s_sigma: all four NULL or all four set,
 * n_rays * (n_samples - 1) elements each -- dense mode only: the composited samples, compact in ray order, and their densities.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null ctx / flat_params / rays / zsteps / quantiles / out / workspace, n_rays < 0, some but not all of s_*
 *   EONERF_E_STATE        weights not set
 *   EONERF_E_ARG          n_q outside 1 .. 8; a quantile that is NaN, outside (0, 1) or not above the one before
 *   EONERF_E_ARG          early_stop_eps outside [0, 1) or NaN
 *   EONERF_E_ARG          early_stop_eps > 0 with a block not in {16, 32, 64}
 *   EONERF_E_ARG          early_stop_eps > 0 and not L_qmax * (1 + 1e-4) < -log(early_stop_eps)
 *   EONERF_E_UNSUPPORTED  s_* with early_stop_eps > 0
 *   (n_rays == 0 returns EONERF_OK here)
 *   EONERF_E_ARG          u_retry without u_cam (as eonerf_render_forward)
 *   EONERF_E_UNSUPPORTED  more rays than a call takes (as eonerf_render_forward)
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_quantile_workspace_bytes(ctx, n_rays, n_q, early_stop_eps > 0 ? block : 0) */
int eonerf_render_depth_quantiles(eonerf_ctx* ctx, const float* flat_params, const float* rays, const float* zsteps,
                                  const float* u_cam, const float* u_retry, int n_rays, const float* quantiles, int n_q,
                                  float early_stop_eps, int block, float* out /* [n_rays][2 + n_q] */, int* n_samples_dev,
                                  int64_t* s_ray, float* s_ts, float* s_te, float* s_sigma,
                                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
