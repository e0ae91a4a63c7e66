/* eonerf_layout.h -- a READ-ONLY query of where the entry points of eonerf_hip.h put their buffers inside the caller's workspace, entry
 * point of libeonerf_hip.so.  For tests and tools that decode what a training call left behind (the saved-activation slab, the
 * saved-gradient slab, the per-sample arrays): they ask the library instead of restating its bump allocator, whose result depends on
 * context internals (precision, backward path, number of pipelines, summation mode, sample count).
 *
 * Conventions are those of eonerf_hip.h.  Host code only: nothing is launched, no device memory is touched, the context is not changed.
 * The answer is what the NEXT call of that kind on this context would carve (eonerf_set_n_samples changes it).
 *
 * out[] receives EONERF_LAYOUT_ENTRIES values in the fixed order below: byte offsets from the start of the workspace, every one a
 * multiple of 256; UINT64_MAX for a buffer the layout does not have (no shadow pass, an inference layout, the chain + GEMM path ...).
 *
 *   [EONERF_LAYOUT_P_CAP]      not an offset: the sample capacity of a pass (leading dimension of every per-sample array, multiple of 256)
 *   [EONERF_LAYOUT_BYTES]      not an offset: the workspace size of that call (eonerf_*_workspace_bytes)
 *   [EONERF_LAYOUT_M_BOTT]     fp32 [2][128][256] bottleneck factors dA1^T X8 | dT1^T X8, then [256] db_A1 | db_T1
 *   [EONERF_LAYOUT_DY_IN]      render, pipelined path: dY_7 in B-operand unit order, p_cap x 512 B
 *   [EONERF_LAYOUT_ENC_PART]   render, pipelined path with the shadow pass: per-workgroup partials of the encoding products
 *   [EONERF_LAYOUT_CAM + m]    member m (EONERF_PASS_*) of the camera pass -- for EONERF_LAYOUT_FIELD_TRAIN: of the one pass
 *   [EONERF_LAYOUT_SUN + m]    member m of the shadow pass
 *
 * Pass members, in the order of the carve: counts, offsets, n_pts (int); px, py, pz, tmid, delta, sigma, albedo [3][p_cap], ts, tb
 * (fp32 [p_cap]); simg (int [p_cap]); act, grd (the two slabs, bf16 or fp32 by the context's precision); masks; g_sigma, g_albedo
 * [3][p_cap], g_ts, g_tb, g_emb [p_cap][4], g_pos [3][p_cap] (fp32).
 *
 * eonerf_ray_layout is a second table with the same conventions, for the PER-RAY buffers a render call carves in front of its passes
 * (n_rays rays; RAY_REC floats per record and its RR_* columns: csrc/eonerf_rays.h):
 *
 *   [EONERF_RAY_CNT_FIRST]     int [R]: samples of the first draw of the camera sampler
 *   [EONERF_RAY_CNT_RETRY]     int [R]: samples of the retry draw; a call with the shadow pass leaves the shadow rays' counts here
 *   [EONERF_RAY_FLAGS]         int [4]: bit 0 of word 0 = the retry draw was taken, as the LAST sampler launch of the call left it (the
 *                              shadow pass' sampler never retries and overwrites the camera pass' bit)
 *   [EONERF_RAY_REC]           fp32 [R][RAY_REC]: the per-ray record of compositing
 *   [EONERF_RAY_G_RAY]         fp32 [R][RAY_REC]: its gradient (training layouts only)
 *   [EONERF_RAY_AMB_SAVE]      fp32 [R][160]: sun encoding (27, padded to 32) and 128 hidden values of the ambient head (training only)
 *   [EONERF_RAY_RAD_RAYS]      fp32 [R][6]: per-ray radiometric gradient terms (training on a deterministic context only)
 *   [EONERF_RAY_EMB_RAYS]      fp32 [R][4]: per-ray embedding gradient sums (training on a deterministic context only)
 */
#ifndef EONERF_LAYOUT_H
#define EONERF_LAYOUT_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_LAYOUT_VERSION 1
int eonerf_layout_version(void);

/* kind */
#define EONERF_LAYOUT_FIELD_TRAIN 0 /* eonerf_field_forward_train / eonerf_field_backward: n points; flags: 1 = density_only */
#define EONERF_LAYOUT_RENDER 1      /* eonerf_render_forward / _backward(_loss): n rays; flags: the EONERF_F_* of the call */

enum {
    EONERF_PASS_COUNTS = 0, EONERF_PASS_OFFSETS, EONERF_PASS_N_PTS, EONERF_PASS_PX, EONERF_PASS_PY, EONERF_PASS_PZ, EONERF_PASS_TMID,
    EONERF_PASS_DELTA, EONERF_PASS_SIGMA, EONERF_PASS_ALBEDO, EONERF_PASS_TS, EONERF_PASS_TB, EONERF_PASS_SIMG, EONERF_PASS_ACT,
    EONERF_PASS_GRD, EONERF_PASS_MASKS, EONERF_PASS_G_SIGMA, EONERF_PASS_G_ALBEDO, EONERF_PASS_G_TS, EONERF_PASS_G_TB, EONERF_PASS_G_EMB,
    EONERF_PASS_G_POS, EONERF_PASS_MEMBERS
};
enum {
    EONERF_LAYOUT_P_CAP = 0, EONERF_LAYOUT_BYTES, EONERF_LAYOUT_M_BOTT, EONERF_LAYOUT_DY_IN, EONERF_LAYOUT_ENC_PART,
    EONERF_LAYOUT_CAM, EONERF_LAYOUT_SUN = EONERF_LAYOUT_CAM + EONERF_PASS_MEMBERS, EONERF_LAYOUT_ENTRIES = EONERF_LAYOUT_SUN + EONERF_PASS_MEMBERS
};

/* Returns EONERF_LAYOUT_ENTRIES (> 0) and fills out[0 .. EONERF_LAYOUT_ENTRIES).  EONERF_E_ARG: a null ctx / out, n < 0, an unknown kind,
 * cap < EONERF_LAYOUT_ENTRIES (nothing is written). */
int eonerf_workspace_layout(const eonerf_ctx* ctx, int kind, int n, int flags, uint64_t* out, int cap);

/* entries of eonerf_ray_layout, in the order of the carve */
#define EONERF_RAY_CNT_FIRST 0
#define EONERF_RAY_CNT_RETRY 1
#define EONERF_RAY_FLAGS 2
#define EONERF_RAY_REC 3
#define EONERF_RAY_G_RAY 4
#define EONERF_RAY_AMB_SAVE 5
#define EONERF_RAY_RAD_RAYS 6
#define EONERF_RAY_EMB_RAYS 7
#define EONERF_RAY_ENTRIES 8

/* The per-ray buffers of eonerf_render_forward / _backward(_loss) on n_rays rays with the EONERF_F_* flags of the call (also the layout of
 * eonerf_rendering_train / _backward: EONERF_F_TRAIN, with EONERF_F_ONLY_DEPTH for depth_only).  Returns EONERF_RAY_ENTRIES (> 0) and fills
 * out[0 .. EONERF_RAY_ENTRIES).  EONERF_E_ARG: a null ctx / out, n_rays < 0, cap < EONERF_RAY_ENTRIES (nothing is written). */
int eonerf_ray_layout(const eonerf_ctx* ctx, int n_rays, int flags, uint64_t* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
