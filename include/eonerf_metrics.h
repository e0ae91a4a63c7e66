/* eonerf_metrics.h -- per-image validation metrics, entry points of libeonerf_hip.so: what the reference evaluates on every held-out
 * image after render_image (train_eonerf.py:229-230, eval_eonerf.py:379-381), on the device.
 *
 *   metrics.py:17-22    uncertainty_aware_loss (colour term, log-beta term, their sum)
 *   metrics.py:60-69    mse, psnr
 *
 * Conventions are those of eonerf_hip.h, eonerf_dsm.h and eonerf_prior.h: plain C, raw DEVICE pointers, a hipStream_t passed as
 * void*, the caller owns every buffer (the workspace included), every call is asynchronous on `stream`, nothing is allocated and
 * nothing synchronises.  The calls are stateless: no eonerf_ctx.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h,
 * > 0 = hipError_t.  Every result is run-to-run bit-identical: fixed-order fp64 sums, no floating-point atomics.
 */
#ifndef EONERF_METRICS_H
#define EONERF_METRICS_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_METRICS_VERSION 1
int eonerf_metrics_version(void);

/* Bytes of the partial sums eonerf_image_metrics needs: one partial (4 doubles) per block of its fixed grid, whatever n is. */
size_t eonerf_metrics_workspace_bytes(void);

/* The metrics of one rendered image of n rays against its ground truth.
 *
 * rgb, beta, gt: fp32, ray r's values at rgb[r * rgb_stride + 0..2], beta[r * beta_stride], gt[r * gt_stride + 0..2]; strides in
 * floats per ray.  The packed out[R,21] of eonerf_render_forward is read in place (rgb = out, stride 21; beta = out + 12, stride 21),
 * separate [n,3] / [n,1] arrays with strides 3 / 1.  beta may be NULL.
 *
 * result[6] (device doubles), every term formed in fp64 from the fp32 inputs, unfused:
 *   [1] coarse_color   = (1 / 3n) * sum over rays and channels of (rgb - gt)^2 / (2 * beta^2)
 *   [2] coarse_logbeta = (3 + (1 / n) * sum over rays of log(beta)) / 2
 *   [0] loss           = coarse_color + coarse_logbeta                                  (metrics.py:17-22)
 *   [3] mse            = (1 / 3n) * sum over rays and channels of (rgb - gt)^2
 *   [4] psnr           = -10 * log10(mse)                                               (metrics.py:60-69)
 *   [5] n              the number of rays summed (as a double)
 * beta == NULL: [0..2] are NaN, [3..5] as usual.  Edge cases are IEEE's, as torch's: mse == 0 gives psnr = +inf, beta <= 0 gives
 * what log and the division give (-inf / NaN / inf), a NaN input propagates to every entry it feeds.
 *
 * Order of summation (the contract behind "bit-identical"): a fixed grid of 256 blocks x 256 threads; thread t of block b adds its
 * rays r = b * 256 + t, r + 65536, ... in increasing order (the three channels of a ray in order 0, 1, 2); a wavefront's 64 sums
 * are folded by shuffles (offsets 32, 16, .. 1), the block's four wavefronts in order 0..3; one partial per block goes to the
 * workspace, and a second kernel folds the 256 partials the same way.  The workspace's earlier contents are never read.
 *
 * Refused, with nothing written: EONERF_E_ARG for n <= 0, a null rgb / gt / result / workspace, rgb_stride or gt_stride < 3,
 * beta_stride < 1 with a beta, a result or workspace that is not 8-byte aligned; EONERF_E_WORKSPACE for
 * workspace_bytes < eonerf_metrics_workspace_bytes(). */
int eonerf_image_metrics(const float* rgb, int rgb_stride, const float* beta, int beta_stride, const float* gt, int gt_stride, long n,
                         double* result, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
