/* eonerf_prior.h -- depth priors from an initial DSM, entry points of libeonerf_hip.so: what the reference does BEFORE training when
 * it is given --init_dsm_path / --init_conf_path, on the device.
 *
 *   sat_utils.py:310-362             reproject_dsm_alt_to_satellite_image (DSM -> one image's pixel grid through that image's RPC)
 *   sat_utils.py:420-432             the RPC projection (rational cubic, ground -> image)
 *   datasets/satellite.py:644-653    altitude -> depth along each pixel's ray, NaN -> -1
 *   datasets/satellite.py:677-679    the same reprojection of a second raster (the confidence), NaN -> -1
 *
 * Conventions are those of eonerf_hip.h and eonerf_dsm.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns
 * every buffer (the workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * The calls are stateless: no eonerf_ctx.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 * Rasters are row-major fp32 [height, width], NaN = no data.  Every result is run-to-run bit-identical: the only atomics are integer
 * maxima, which do not depend on the order in which they arrive.
 */
#ifndef EONERF_PRIOR_H
#define EONERF_PRIOR_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_PRIOR_VERSION 1
int eonerf_prior_version(void);

/* Bytes of the winner image eonerf_prior_reproject needs for an out_h x out_w image (0 for sizes it refuses). */
size_t eonerf_prior_workspace_bytes(int out_h, int out_w);

/* reproject_dsm_alt_to_satellite_image (sat_utils.py:310-362) for one image, fused with the altitude -> depth step of
 * load_depth_priors_from_dsm (datasets/satellite.py:644-653).  fp64 arithmetic, unfused, one cast to fp32 at the end.
 *
 * dsm[h*w] fp32: the initial DSM.  bounds = {left, bottom, right, top} of its raster in UTM metres (rasterio's src.bounds); the DSM's
 * CRS is "+proj=utm +zone=<utm_zone> [+south]" on WGS84.  rpc: the image's RPC, already rescaled to the image's downscale.
 *
 * Sample points: the (2h) x (2w) grid (pt_density = 2), point p = i * 2w + j in raveled order:
 *   east  = linspace(min(left, right), max(left, right), 2w)[j],  north = linspace(max(bottom, top), min(bottom, top), 2h)[i]
 *           (numpy's formula: start + k * step with step = (stop - start) / (n - 1), the last element exactly stop);
 *   cell  = (int(linspace(0, h-1, 2h)[i]), int(linspace(0, w-1, 2w)[j])) by truncation;  alt = dsm[cell] widened to fp64;
 *   lon, lat = inverse UTM (below);  col, row = RPC projection of (lon, lat, alt).
 * A point is valid iff 0 <= col < out_w and 0 <= row < out_h (a NaN altitude fails every comparison); its pixel is
 * (int(row), int(col)).  A pixel hit by several points takes the LAST one in raveled order, as numpy's fancy-index assignment does:
 * the call clears workspace[out_h*out_w] (uint32) on the stream and every valid point does one atomic max of p + 1 into it.
 *
 * Outputs, each may be NULL (not both):
 *   raster_out[out_h*out_w] fp32: values[cell of the winner] -- `values` is a second raster of the DSM's size (other_val_path: the
 *     confidence), or NULL for the DSM itself.  No winner: NaN.  raster_nan_to_minus_one != 0 writes -1.0 where the value is NaN
 *     (datasets/satellite.py:679).
 *   depth_out[out_h*out_w] fp32: from the DSM's altitude at the winner (whatever `values` is), with the image's normalised rays
 *     `rays` (fp32 rows of ray_stride >= 6 floats: origin3, dir3, ...; row-major pixels) and the dataset's fp32 Z offset / scale:
 *       a = (double(alt) - double(z_offset)) / double(z_scale);  depth = (a - double(o_z)) / double(d_z);  NaN -> -1.0;  (float)depth
 *   One call with `values` = the confidence therefore yields the depth prior AND the reprojected confidence of an image; the
 *   reference runs the reprojection twice and gets the same winners.
 *
 * Inverse UTM: pyproj / PROJ are not vendored with the reference; pinned by a definition-based arbitrary-precision transverse Mercator
 * (tests/geodesy_exact.py, tests/test_geodesy_gpu.py; pyproj itself still absent).  It is restated from the published
 * algorithm PROJ's etmerc implements (Karney 2011: the 6th-order Krueger series with the beta coefficients, then Newton on
 * tau = tan(lat) from the conformal latitude, a fixed five iterations); the forward series of eonerf_generate_rays has the same
 * status.  tests/prior_restated.py is the contract; the rest is pinned by golden g13, recorded from the reference's own code.
 *
 * Refused: EONERF_E_UNSUPPORTED for 4*h*w >= 2^32 - 1 (the winner index) and for out_h or out_w > 32767 (the reference's
 * astype(np.int16) wraps there); EONERF_E_WORKSPACE for workspace_bytes < eonerf_prior_workspace_bytes(out_h, out_w);
 * EONERF_E_ARG for null or non-finite arguments, no output, a depth output without rays, ray_stride < 6, z_scale == 0, a zone
 * outside 1 .. 60, a workspace that is not 4-byte aligned. */
int eonerf_prior_reproject(const float* dsm, const float* values, int h, int w, const double bounds[4], const eonerf_rpc* rpc,
                           int utm_zone, int south, int out_h, int out_w, float* raster_out, int raster_nan_to_minus_one,
                           const float* rays, int ray_stride, float z_offset, float z_scale, float* depth_out,
                           void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
