/* eonerf_normals.h -- the density gradient of the field and the surface normals of export renders, entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer
 * (the workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 *
 * The gradient is taken in FORWARD mode inside the density-only inference chain: every sample travels as four columns of the chain's
 * matrix products -- the value and its three partial derivatives -- through the same packed weights.  Nothing is saved, no weight
 * gradient is formed, and the chain runs in the inference precisions: EONERF_FP32 and EONERF_F16X3.  The value column is the column
 * eonerf_query_density computes, bit for bit.
 *
 * THE RULE, for one camera ray of one call.
 *   k = 0 .. n - 1 are the samples the EONERF_F_ONLY_DEPTH inference forward composites for that ray, in slot order: after the cube
 *     filter, after the occupancy rule while a grid is set on the context (eonerf_occ.h), of the draw that rendered (the first draw, or
 *     the retry draw under "resample if any ray is empty").  ts_k, te_k, delta_k and the weights w_k are the forward's own.
 *   p_k          the position the forward's chain evaluates: o + d * mid_k.
 *   sigma_k      the density the density chain gives at p_k.
 *   g_k          the gradient of sigma at p_k, componentwise times axis_scale (a gradient is a covector: with axis_scale =
 *                1 / scene_scale it is expressed in the metric east / north / up frame).
 *   u_k = g_k / |g_k| with |g_k| = sqrt(gx * gx + gy * gy + gz * gz), in fp32 operations without contraction;
 *   u_k = 0 where |g_k| is 0 or not finite.
 *   N = -sum_k w_k u_k (it points out of the surface, against increasing density), A = sum_k w_k: fp32, one ray per wavefront, lane
 *     partial sums in slot order and the compositing forward's wave reduction.
 *   N is NOT normalised: |N| <= A, and |N| / A tells how well the samples of the ray agree on a direction.
 *
 * OUTPUT  out[n_rays][5]:  column 0 the expected depth, bit-equal to eonerf_render_forward under EONERF_F_ONLY_DEPTH on the same
 *   inputs (as is n_samples_dev);  columns 1..3 N;  column 4 A.  A ray without samples gives zeros.
 *
 * Launches of eonerf_render_normals: the forward's sampler launch, one launch of the four-column chain, one compositing launch.
 * The chain is dense only: there is no march mode (early_stop_eps) here.
 */
#ifndef EONERF_NORMALS_H
#define EONERF_NORMALS_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_NORMALS_VERSION 1
int eonerf_normals_version(void);

/* Points one call of eonerf_field_density_grad takes, and samples (n_rays x (n_samples - 1), rounded up to 256) one call of
 * eonerf_render_normals takes: four chain columns per sample must stay an int. */
#define EONERF_NORMALS_MAX_POINTS (1 << 28)

/* Bytes of the workspace of eonerf_field_density_grad.  0 for a null context, n_points < 0 or more points than a call takes. */
size_t eonerf_density_grad_workspace_bytes(const eonerf_ctx* ctx, int n_points);

/* sigma[n] and grad[n][3] = d sigma / d (x, y, z) at the n points xyz[n][3].  sigma is bit-equal to eonerf_query_density.
 * With EONERF_F16X3 the range flag (eonerf_range_status) covers every operand of the chain, the derivative columns included.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null ctx / flat_params / xyz / sigma / grad / workspace, n_points < 0
 *   EONERF_E_STATE        weights not set
 *   EONERF_E_UNSUPPORTED  a bf16 context
 *   (n_points == 0 returns EONERF_OK here)
 *   EONERF_E_UNSUPPORTED  more than EONERF_NORMALS_MAX_POINTS points
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_density_grad_workspace_bytes(ctx, n_points) */
int eonerf_field_density_grad(eonerf_ctx* ctx, const float* flat_params, const float* xyz /* [n][3] */, int n_points,
                              float* sigma /* [n] */, float* grad /* [n][3] */, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of the workspace of eonerf_render_normals.  0 for a null context, n_rays < 0 or more rays than a call takes. */
size_t eonerf_normals_workspace_bytes(const eonerf_ctx* ctx, int n_rays);

/* Expected depth, composited normal and accumulated weight of n_rays camera rays by the rule above.  rays, zsteps, u_cam, u_retry: those of
 * eonerf_render_forward -- noise buffers or in-kernel Philox; the call uses ONE Philox call number.  axis_scale: HOST float[3], or NULL
 * for ones.  The occupancy grid set on the context is honoured as by an inference forward.  n_samples_dev (may be NULL) receives the
 * number of composited samples.  s_ray (int64), s_ts, s_te, s_sigma, s_grad ([.][3], BEFORE axis_scale): all five NULL or all five set,
 * n_rays * (n_samples - 1) elements (s_grad: three times that) each -- the composited samples, compact in ray order.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null ctx / flat_params / rays / zsteps / out / workspace, n_rays < 0
 *   EONERF_E_STATE        weights not set
 *   EONERF_E_ARG          some but not all of s_*
 *   EONERF_E_ARG          an axis_scale entry that is NaN, infinite or zero
 *   EONERF_E_UNSUPPORTED  a bf16 context
 *   (n_rays == 0 returns EONERF_OK here)
 *   EONERF_E_ARG          u_retry without u_cam (as eonerf_render_depth_quantiles)
 *   EONERF_E_UNSUPPORTED  more rays than a call takes (as eonerf_render_depth_quantiles, and EONERF_NORMALS_MAX_POINTS samples)
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_normals_workspace_bytes(ctx, n_rays) */
int eonerf_render_normals(eonerf_ctx* ctx, const float* flat_params, const float* rays, const float* zsteps,
                          const float* u_cam, const float* u_retry, int n_rays, const float* axis_scale,
                          float* out /* [n_rays][5] */, int* n_samples_dev,
                          int64_t* s_ray, float* s_ts, float* s_te, float* s_sigma, float* s_grad,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
