/* eonerf_dsm.h -- DSM evaluation entry points of libeonerf_hip.so: what the reference does AFTER render_image on its evaluation path
 * (nadir virtual camera, point cloud -> raster, NCC registration against the lidar DSM, MAE), on the device.
 *
 *   eval_eonerf.py:78-95,130-249      create_rays_from_nadir / generate_rays_from_virtual_pinhole (non-pinhole branch)
 *   datasets/satellite.py:545-610     get_dsm_from_nerf_prediction -> plyflatten(radius=1, sigma=inf)
 *   dsmr.py                           compute_shift / apply_shift
 *   sat_utils.py:133-256              dsm_pointwise_diff (water mask, registration, clip) and nanmean(|diff|)
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer
 * (accumulators and workspaces included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * The calls are stateless: no eonerf_ctx.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 * Rasters are row-major fp32 [height, width], NaN = no data.  Every result is run-to-run bit-identical: integer atomics in the
 * rasteriser, fixed-order fp64 sums everywhere else (no floating-point atomics).
 */
#ifndef EONERF_DSM_H
#define EONERF_DSM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_DSM_VERSION 1
int eonerf_dsm_version(void);

/* create_rays_from_nadir (eval_eonerf.py:78-95) around the non-pinhole branch of generate_rays_from_virtual_pinhole (:130-249).
 * h, w: the raster's size AFTER the caller's int(h // img_downscale).  The reference calls it with radius 2, elevation 0, azimuth 0,
 * near max(0, radius - 2), far near + 2.5.  Every ray has the direction d = normalise(get_dir_vec_from_el_az(el, az) / scene_scale);
 * origins lie on the plane through pt_a = (0,0,-1) - radius * d perpendicular to d:
 *   x = (i - w/2) / (w/radius) + pt_a.x,   y = -(j - h/2) / (h/radius) + pt_a.y,   z from the plane equation   (pixel i of row j)
 * The sun direction is normalise(get_dir_vec_from_el_az(sun_el, sun_az) / scene_scale), WITHOUT the 90-degree flip of the dataset
 * loader (:90-93 pass the angles straight through).  fp64 arithmetic, one cast to fp32 at the end, as the reference's numpy.
 * -> rays[h*w, 11] fp32 = origin3, dir3, near, far, sun3, row-major over (j, i). */
int eonerf_nadir_rays(int h, int w, double radius, double elevation_deg, double azimuth_deg, double near, double far,
                      const double scene_scale[3], double sun_elevation_deg, double sun_azimuth_deg, float* rays, void* stream);

/* get_dsm_from_nerf_prediction (datasets/satellite.py:545-610) in one pass over the rays.
 * Per ray (fp64, unfused, as get_utmalt_from_nerf_prediction :502-533): xyz = (o + d * depth) * scale + offset; a negative northing
 * gets + 10e6 (:560); rays with depth < 0 are dropped (:562).  Rays whose depth or position is not finite, or whose |altitude| is
 * 2^31 m or more, are dropped as well: the reference has NO defined behaviour there (a NaN reaches plyflatten's index arithmetic).
 * Splat = plyflatten(cloud, xoff, yoff, res, xsize, ysize, radius=1, sigma=inf):
 *   cell i = floor((east - xoff) / res), j = floor((yoff - north) / res); every in-bounds cell of the 3x3 window around (j, i)
 *   receives the altitude with weight 1; a cell's value is the mean of what it received, NaN if nothing.
 * PARITY UNPINNED: plyflatten is a third-party package that is not vendored with the reference; the lines above are the contract of
 * this call (restated in tests/dsm_restated.py), not a bit-level claim about plyflatten.
 * Accumulation is fixed point, so the raster does not depend on the order in which rays arrive: llrint(altitude * 2^16) summed into
 * acc_sum[ysize*xsize] (int64) and a count into acc_cnt[ysize*xsize] (int32) with integer atomics, then dsm = sum / 2^16 / count in
 * fp64, rounded once to fp32.  The call clears both accumulators itself on the stream: they may be passed in dirty.
 * rays: fp32 rows of ray_stride floats (>= 6: origin3, dir3, ...; 11 for the usual table); depth[n] fp32.
 * (xoff, yoff) is the raster's upper-left corner: with a ROI quadruple (x, y, size, res) that is yoff = y + size * res (:570). */
int eonerf_dsm_rasterize(const float* rays, int ray_stride, const float* depth, long n, const double scale[3], const double offset[3],
                         double xoff, double yoff, int xsize, int ysize, double res,
                         int64_t* acc_sum, int32_t* acc_cnt, float* dsm, void* stream);

/* sat_utils.py:181-185: sec[j,i] = NaN where water[j,i] != 0, over the common top-left extent of the two.  In place.
 * The reference masks the predicted DSM BEFORE it registers it, so this comes before eonerf_dsm_register. */
int eonerf_dsm_mask_water(float* sec, int sec_h, int sec_w, const uint8_t* water, int water_h, int water_w, void* stream);

/* dsmr.compute_shift(ref, sec, scaling) with no host round trip between pyramid levels.
 *   mean_std(u, v, dx, dy): only pixels where u[j,i] and v[j+dy,i+dx] are both finite (out of bounds = NaN); means first, then the
 *     centred sums; sig = sqrt(sum / count), ncc = xcorr / (sigu * sigv).  fp64 accumulators over the fp32 rasters, as numba types them.
 *   compute_ncc: 121 shifts, centre +- 5, scanned y outer / x inner; the first strict maximum wins; a NaN score never wins (an
 *     all-NaN sec leaves the centre; where the reference divides 0 / 0 and raises, the scores here are NaN).
 *   recursive_ncc: one more level while min(h, w) of ref > 100; the coarse (dx, dy) * 2 is the next level's centre.
 *   downsample2x: out[J,I] = mean of the finite values of u[2J+1 .. 2J+2, 2I+1 .. 2I+2] with the window's origin clipped to the last
 *     row / column (dsmr.py:24-38: every (j,i) writes out[j//2, i//2], the last writer wins); size ceil(n/2); kept in fp64 as the
 *     reference's np.zeros output is.
 *   a = sigu / sigv if scaling else 1;  b = muu - muv * a, both at the final shift.
 * Sums are taken per (shift, band of 16 rows) workgroup and added in a fixed order: run-to-run identical, and within 1e-9 of the
 * reference's sequential sum for rasters below 2^14 cells of |value| < 2^9.
 * -> out4 (device) = dx, dy, a, b as doubles.
 * workspace: eonerf_dsm_register_workspace_bytes(...) bytes, 16-byte aligned, contents on entry irrelevant.  After the call it holds,
 * for tests and diagnostics (eonerf_dsm_register_level gives the byte offsets): per level its (dx, dy) as int32[2], its 121 scores
 * as double[121] in scan order, and the fp64 pyramid levels >= 1 of ref and sec.  Level 0 is the full resolution. */
size_t eonerf_dsm_register_workspace_bytes(int ref_h, int ref_w, int sec_h, int sec_w);
int eonerf_dsm_register_levels(int ref_h, int ref_w);
/* dims = {ref_h, ref_w, sec_h, sec_w} of `level`; offs = byte offsets in the workspace of {shift int32[2], scores double[121],
 * ref level, sec level} (the last two are (size_t)-1 for level 0, which is read from the caller's rasters). */
int eonerf_dsm_register_level(int ref_h, int ref_w, int sec_h, int sec_w, int level, int dims[4], size_t offs[4]);
int eonerf_dsm_register(const float* ref, int ref_h, int ref_w, const float* sec, int sec_h, int sec_w, int scaling,
                        double* out4, void* workspace, size_t workspace_bytes, void* stream);

/* The tail of dsm_pointwise_diff (sat_utils.py:198-207) and the nanmean of :255, fused:
 *   apply_shift: reg[j,i] = a * sec[j+dy, i+dx] + b (NaN outside sec), rounded to fp32 as the reference's GeoTIFF holds it (the
 *     reference's c*i + d*j terms are zero: dsmr.py:144 reuses the name c for its channel loop, which runs over [0]);
 *   clip to [min(gt) - 10, max(gt) + 10] in fp32;  err = reg[:h,:w] - gt[:h,:w] in fp32, h, w = the common extent.
 * min / max of gt are taken over its FINITE cells; the reference's ndarray.min()/max() return NaN for a GT with holes, which turns
 * its whole result into NaN.
 * transform4 (device) = dx, dy, a, b as eonerf_dsm_register writes them.  water (may be NULL): cells of sec under the mask read as
 * NaN (the same effect as eonerf_dsm_mask_water on a sec that must stay intact).
 * -> out2 (device) = nanmean(|err|), n_valid as doubles (NaN, 0 if no cell is valid); err (may be NULL): [h, w] fp32.
 * workspace: eonerf_dsm_mae_workspace_bytes() bytes. */
size_t eonerf_dsm_mae_workspace_bytes(void);
int eonerf_dsm_mae(const float* gt, int gt_h, int gt_w, const float* sec, int sec_h, int sec_w,
                   const uint8_t* water, int water_h, int water_w, const double* transform4,
                   double* out2, float* err, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
