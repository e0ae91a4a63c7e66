/* eonerf_occ.h -- occupancy grid, entry points of libeonerf_hip.so: the one-level 128^3 OccGridEstimator the reference trains,
 * saves and reloads (train_eonerf.py:74,112-119, eval_eonerf.py:66-73) but never samples with (sat_rendering.py:92-94), built on the
 * device and USED: inference renders skip the samples of empty cells.
 *
 * Conventions are those of eonerf_hip.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer
 * (the workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.
 * Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 *
 * THE GRID.  One level over the cube [-1,1]^3, r cells per axis, 1 <= r <= 256 (the reference: 128, opt.py:86).  Its state is
 *     occs [r^3] fp32                       the running occupancy value of every cell
 *     bits [ceil(r^3 / 32)] uint32          cell c is bit (c & 31) of word (c >> 5); the unused bits of the last word are zero
 * with the flat cell index  c = (ix * r + iy) * r + iz  (nerfacc's binaries[0, ix, iy, iz]).
 *
 * THE CELL OF A POINT.  Per axis, in fp32, as three separately rounded operations (no fused multiply-add):
 *     i = min(r - 1, (int)(((x + 1) * 0.5f) * (float)r))
 * The clamp is needed: x = 1 - 2^-24 lies inside the cube and x + 1 rounds to 2.0f.  (The kernels also clamp at 0; no coordinate
 * with |x| < 1 reaches that clamp.)
 *
 * THE CULLING RULE.  Of the samples of a ray that pass the sampler's cube filter (|x|, |y|, |z| < 1 at the mid point), one is kept
 * if and only if ITS CELL'S BIT IS SET OR IT IS THE LAST CUBE-VALID SAMPLE OF ITS RAY.  Hence
 *   - a ray has a sample exactly when it has one without the grid: "resample if any ray is empty" (sat_rendering.py:260-262) is
 *     the same decision with and without a grid;
 *   - the 1e10 interval of the camera pass (radiance_fields/eonerf.py:218-220) lands on the same sample as without the grid;
 *   - an all-ones grid is the identity, bit for bit;
 *   - a gridded render is the ungridded render with the culled samples' alphas set to zero;
 *   - columns 14 and 15 of the 21 output columns (pts_per_ray, sc_pts_per_ray) report the KEPT counts.
 * The rule covers the camera pass, its retry draw and the shadow pass (the shadow-ray count of the camera compositing launch and
 * the sun sampler).  Only lanes whose sample is cube-valid look a bit up, with the clamped index: no address outside `bits` is
 * formed, whatever the ray table holds.
 */
#ifndef EONERF_OCC_H
#define EONERF_OCC_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_OCC_VERSION 1
int eonerf_occ_version(void);

#define EONERF_OCC_MAX_RESOLUTION 256

/* Bytes of the workspace eonerf_occ_update needs: the field workspace of one chunk of min(r^3, 2^18) cells
 * (eonerf_field_workspace_bytes) plus the reduction scratch -- beyond 2^18 cells it does not grow with r.  0 for a null context
 * or r outside 1 .. 256. */
size_t eonerf_occ_workspace_bytes(const eonerf_ctx* ctx, int r);

/* One OccGridEstimator update over ALL r^3 cells (nerfacc v0.5.2's update_every_n_steps body as SURVEY.md 2.1 recalls it, without
 * its warm-up / random-quarter cell selection):
 *   point    one per cell, per axis  x = ((i + u) / r) * 2 - 1, every operation rounded in fp32 ((float)i + u, / (float)r, * 2, - 1).
 *            jitter != 0: (u_x, u_y, u_z) = words 0..2 of the context's Philox4x32-10 stream (key: eonerf_set_noise_seed) at counter
 *            (cell, 0, 3, seed_call), 24 bits -> [0,1) as the sampler's jitter; draw number 3 belongs to this call (0..2: the
 *            sampler).  The context's own call counter is not advanced.  jitter == 0: u = 0.5.
 *            points_out [r^3][3] fp32 (may be NULL) receives the points.
 *   density  sigma = the context's density-only chain at the points (the launch eonerf_query_density makes), cells in chunks of
 *            at most 2^18.
 *   value    occ = sigma * step_size, ONE fp32 multiply (query_opacity);  occs[c] = max(occs[c] * decay, occ).
 *   thr      mean = (sum of occs in fp64, in a fixed order) / r^3;  thr = min((float)mean, occ_thre);  *thr_out = thr (device
 *            float, may be NULL).
 *   bits     bit c = occs[c] > thr; the unused bits of the last word are written as zero.
 * Two calls with the same inputs and the same seed_call give the same bits, word for word.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null ctx / flat_params / occs / bits / workspace
 *   EONERF_E_STATE        weights not set
 *   EONERF_E_UNSUPPORTED  r outside 1 .. 256
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_occ_workspace_bytes(ctx, r) */
int eonerf_occ_update(eonerf_ctx* ctx, const float* flat_params, float* occs, uint32_t* bits, int r, float step_size, float decay,
                      float occ_thre, int jitter, uint32_t seed_call, float* points_out, float* thr_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* bits_out: a cell is set if any of its 27 neighbours (itself included) is set in bits_in; neighbours outside the cube do not
 * exist.  bits_in and bits_out must not overlap.  EONERF_E_ARG: a null pointer or bits_in == bits_out; EONERF_E_UNSUPPORTED: r
 * outside 1 .. 256. */
int eonerf_occ_dilate(const uint32_t* bits_in, uint32_t* bits_out, int r, void* stream);

/* The context remembers `bits` (a BORROWED device pointer: the caller keeps the ceil(r^3 / 32) words alive and unchanged until
 * every call that was enqueued while the grid was set has completed, and clears the grid before freeing them).  bits == NULL
 * clears it (r is ignored).  EONERF_E_ARG: a null ctx; EONERF_E_UNSUPPORTED: r outside 1 .. 256 with a non-null bits.
 *
 * While a grid is set, these calls cull samples by the rule above:
 *     eonerf_render_forward WITHOUT EONERF_F_TRAIN (EONERF_F_ONLY_DEPTH included), eonerf_render_sun_sweep.
 * These calls ignore it:
 *     eonerf_render_forward with EONERF_F_TRAIN and its backward, eonerf_presample, eonerf_sample_rays, eonerf_rendering*,
 *     the field entry points (eonerf_field_*, eonerf_query_density) and eonerf_occ_update itself.
 * Workspace sizes do not change: the capacity of a pass stays n_rays x (n_samples - 1). */
int eonerf_set_occupancy(eonerf_ctx* ctx, const uint32_t* bits, int r);

/* eonerf_sample_rays with an explicit grid: the cube-filtered stratified samples of `rays`, culled by the rule above (no 1e10
 * patch: t_ends are the sampler's own).  Every other argument, the workspace (eonerf_render_workspace_bytes(ctx, n_rays,
 * EONERF_F_ONLY_DEPTH)) and the refusals are those of eonerf_sample_rays; pts_per_ray receives the kept counts.  The grid set on
 * the context is not read.  In addition EONERF_E_ARG: a null bits; EONERF_E_UNSUPPORTED: r outside 1 .. 256. */
int eonerf_occ_sample_rays(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays,
                           const uint32_t* bits, int r, int64_t* ray_indices, float* t_starts, float* t_ends, float* pts_per_ray,
                           int* n_dev, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
