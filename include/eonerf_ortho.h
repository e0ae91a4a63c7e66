/* eonerf_ortho.h -- true orthophoto on the device, entry points of libeonerf_hip.so: the input images resampled onto a rendered (or
 * given) surface through their own RPCs, occluded cells left out, fused into one mosaic.  The reference carries the two functions of
 * the chain and never calls them:
 *
 *   datasets/satellite.py:502-543    get_utmalt_from_nerf_prediction / get_lonlatalt_from_nerf_prediction (ray + depth -> lon, lat, alt)
 *   sat_utils.py:420-432             rpc_projection_differentiable (the rational cubic, ground -> image)
 *   sat_rendering.py:288-306         the per-image radiometric gain A and bias b, rgb_j = clip(A * rgb + b)
 *
 * Conventions are those of eonerf_hip.h, eonerf_dsm.h and eonerf_prior.h: plain C, raw DEVICE pointers, a hipStream_t passed as
 * void*, the caller owns every buffer, every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * The calls are stateless: no eonerf_ctx, no workspace.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 * One thread per point; no atomics, so every result is run-to-run bit-identical.  All arithmetic is fp64 and unfused, with one
 * cast to fp32 per fp32 output.
 * Sizes, for all three calls: EONERF_E_UNSUPPORTED where n needs more than 2^31 - 1 workgroups of 256 points, or where a table's
 * element count (h * w * channels, K * n * channels; formed in 64 bits) leaves 2^62.
 */
#ifndef EONERF_ORTHO_H
#define EONERF_ORTHO_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_ORTHO_VERSION 1
#define EONERF_ORTHO_MAX_MEDIAN 64      /* images the median of eonerf_ortho_fuse takes (one cell's values live in private memory) */
int eonerf_ortho_version(void);

/* Surface points of a render: rays[n] (fp32 rows of ray_stride >= 6 floats: origin3, dir3, ...) and depth[n] (fp32) ->
 * lonlatalt_out[n*3] (fp64: lon, lat in degrees, alt in metres).
 *   xyz = (o + d * depth) * scene_scale + scene_offset        in fp64 on the widened fp32 values (get_utmalt_from_nerf_prediction)
 *   lon, lat = inverse UTM of (east, north) = (xyz[0], xyz[1]) in "+proj=utm +zone=<utm_zone> [+south]" on WGS84 (the series of
 *   eonerf_prior.h);  alt = xyz[2].
 * A non-finite depth gives three NaNs.
 * Refused with EONERF_E_ARG: a null pointer, n < 0, ray_stride < 6, a non-finite scale or offset, a zone outside 1 .. 60.
 * n == 0 succeeds and writes nothing. */
int eonerf_ortho_ground(const float* rays, int ray_stride, const float* depth, long n, const float scene_scale[3],
                        const float scene_offset[3], int utm_zone, int south, double* lonlatalt_out, void* stream);

/* One image gathered at the points of eonerf_ortho_ground.  rpc: the image's RPC at the image's downscale, passed by value to the kernel.
 * pixels[h*w*channels]: fp32, row-major, channel-last, NaN = no data, 1 <= channels <= 4; may be NULL when only colrow_out is wanted.
 * gain[channels], bias[channels]: HOST arrays, the image's radiometry v_image = gain * v_common + bias (identity: 1 and 0).
 * visibility[n]: fp32 transmittance from the point towards the image's satellite, or NULL (no occlusion test).
 *
 * Projection: col, row = the rational cubic of the normalised (lat, lon, alt), times col / row scale plus offset -- the expression of
 *   eonerf_prior_reproject.  Written to colrow_out as computed, inside the image or not.
 * Pixel convention: the integer coordinate (c, r) IS pixel [r, c]; no half-pixel offset (load_data localises
 *   meshgrid(arange(w), arange(h)), datasets/satellite.py:449).
 * Sample: c0 = floor(col), r0 = floor(row), c1 = min(c0 + 1, w - 1), r1 = min(r0 + 1, h - 1), fx = col - c0, fy = row - r0; per
 *   channel, in fp64 on the widened pixels,
 *     v = (1 - fy) * ((1 - fx) * p[r0,c0] + fx * p[r0,c1]) + fy * ((1 - fx) * p[r1,c0] + fx * p[r1,c1]),
 *   then (v - bias_c) / gain_c, and one cast to fp32.
 * Weight: 0 if any of these fails (NaN fails every comparison): lon, lat, alt finite; 0 <= col <= w - 1 and 0 <= row <= h - 1; all
 *   four taps finite in every channel; visibility >= min_visibility when a visibility is given.  Otherwise the visibility, or 1
 *   without one.  Where the weight is 0 the layer holds NaN in every channel.
 *
 * Outputs, each may be NULL (not all three): layer_out[n*channels] fp32, weight_out[n] fp32, colrow_out[n*2] fp64 (col, row).
 * Refused with EONERF_E_ARG: a null lonlatalt or rpc, n < 0, no output, layer_out or weight_out without pixels (or without gain / bias),
 * h or w < 1, channels outside 1 .. 4, a zero or non-finite gain, a non-finite bias, a non-finite min_visibility.
 * n == 0 succeeds and writes nothing. */
int eonerf_ortho_gather(const double* lonlatalt, long n, const eonerf_rpc* rpc, const float* pixels, int h, int w, int channels,
                        const float* gain, const float* bias, const float* visibility, float min_visibility,
                        float* layer_out, float* weight_out, double* colrow_out, void* stream);

/* K layers -> one mosaic.  layers[K*n*channels], weights[K*n] as eonerf_ortho_gather wrote them, image-major.
 *   count_out[n] int32: the number of k with weights[k] > 0;  weight_sum_out[n] fp32: the fp64 sum of those weights, cast.
 *   mode 0 (EONERF_ORTHO_MEAN): sum_k w_k v_k / sum_k w_k over the k with w_k > 0, summed in fp64 in ascending k.
 *   mode 1 (EONERF_ORTHO_MEDIAN): per channel the median of the v_k with w_k > 0, unweighted, numpy's definition:
 *     0.5 * (s[(m-1)/2] + s[m/2]) on the ascending sort of the m values, in fp64, one cast.
 *   count == 0: a NaN mosaic and a zero weight sum.
 * Each output may be NULL (not all three).
 * Refused: EONERF_E_ARG for null layers or weights, n < 0, K < 1, channels outside 1 .. 4, a mode other than 0 or 1, no output;
 * EONERF_E_UNSUPPORTED for mode 1 with K > EONERF_ORTHO_MAX_MEDIAN (mode 0 takes any K) and for K * n * channels beyond 2^62 elements.
 * n == 0 succeeds and writes nothing. */
#define EONERF_ORTHO_MEAN 0
#define EONERF_ORTHO_MEDIAN 1
int eonerf_ortho_fuse(const float* layers, const float* weights, int K, long n, int channels, int mode, float* mosaic_out,
                      float* weight_sum_out, int32_t* count_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
