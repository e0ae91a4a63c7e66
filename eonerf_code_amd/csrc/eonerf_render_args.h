// Argument blocks of an inference / training forward of the render path, filled from (ctx, the carved workspace, the call's own
// pointers): ONE definition for eonerf_render_forward, eonerf_presample (eonerf_render.hip) and eonerf_render_sun_sweep
// (eonerf_sweep.hip), so that a sweep's launches are the forward's launches by construction.  Host logic only.
#pragma once
#include "eonerf_ctx.h"

// camera pass compositing; w.amb_save is null outside training
inline CompositeArgs composite_args(const eonerf_ctx* ctx, const RenderWs& w, const float* flat, const float* rays, int n_rays, int p_cap, bool depth_only) {
    CompositeArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.n_samples = ctx->n_samples;
    ca.rays = rays; ca.offsets = w.cam.offsets; ca.counts = w.cam.counts;
    ca.sigma = w.cam.sigma; ca.delta = w.cam.delta; ca.tmid = w.cam.tmid; ca.albedo = w.cam.albedo; ca.ts = w.cam.ts; ca.tb = w.cam.tb;
    ca.p_pad = p_cap; ca.n_rays = n_rays; ca.depth_only = depth_only ? 1 : 0; ca.amb = ambient_w(ctx, flat); ca.ray_out = w.ray_rec;
    ca.amb_save = depth_only ? nullptr : w.amb_save;
    return ca;
}

// Arguments of the camera pass's sampler launch (eonerf_render_forward, eonerf_presample, eonerf_render_sun_sweep); the Philox call
// number is the caller's.  cull: the call honours the context's occupancy grid (include/eonerf_occ.h: inference forwards and the sun
// sweep; never a training forward or eonerf_presample) -- sun_sample_args inherits it, so the shadow pass culls by the same grid
inline SampleArgs camera_sample_args(const eonerf_ctx* ctx, const RenderWs& w, const float* rays, const int64_t* img_idx, const float* zsteps,
                                     const float* u_cam, const float* u_retry, int n_rays, int* n_samples_dev, bool cull = false) {
    SampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n_samples = ctx->n_samples;
    sa.rays = rays; sa.img_idx = img_idx; sa.zsteps = zsteps; sa.u = u_cam; sa.u_retry = u_retry;
    sa.perturb = 1; sa.retry = (!u_cam || u_retry) ? 1 : 0;
    if (!u_cam) sa.seed = ctx->noise_seed;
    sa.n_rays = n_rays; sa.sun_pass = 0; sa.patch_last = 1;
    sa.cnt_first = w.cnt_first; sa.cnt_retry = w.cnt_retry; sa.counts = w.cam.counts; sa.offsets = w.cam.offsets;
    sa.flags = w.flags; sa.n_pts = w.cam.n_pts; sa.n_pts_copy = n_samples_dev;       // the scan kernel also fills the caller's count
    sa.px = w.cam.px; sa.py = w.cam.py; sa.pz = w.cam.pz; sa.tmid = w.cam.tmid; sa.delta = w.cam.delta; sa.simg = w.cam.simg;
    if (cull && ctx->occ_bits) { sa.occ_bits = ctx->occ_bits; sa.occ_r = ctx->occ_r; }
    return sa;
}

// irradiance model + radiometric affine + packing (sat_rendering.py:265-312): done by the chunk's LAST compositing launch, ray by ray
inline ShadeArgs shade_args(const eonerf_ctx* ctx, const RenderWs& w, const float* flat, const int64_t* img_idx, int n_rays, bool shadows, int flags, float* out) {
    ShadeArgs sh;
    sh.ray_rec = w.ray_rec; sh.img_idx = img_idx;
    sh.radiometric = ctx->cfg.radiometric ? flat + ctx->pl.t[ctx->pl.rad].offset : nullptr;
    sh.pts_first = w.cnt_first; sh.sc_counts = shadows ? w.sun.counts : w.cnt_first;
    sh.n_rays = n_rays; sh.use_shadow = shadows ? 1 : 0; sh.eval = (flags & EONERF_F_EVAL) ? 1 : 0; sh.out = out;
    return sh;
}

// sun pass: shadow rays from the rendered surface toward the sun, derived from the camera pass's sampler arguments `sa` (its ray table,
// step table, seed and call number: the shadow pass draws under its camera pass's call number)
inline SampleArgs sun_sample_args(const SampleArgs& sa, const RenderWs& w, const float* u_sun) {
    SampleArgs ss = sa;
    ss.img_idx = nullptr; ss.u = u_sun; ss.u_retry = nullptr; ss.retry = 0;
    ss.depth = w.ray_rec + RR_DEPTH; ss.depth_stride = RAY_REC; ss.sun_pass = 1; ss.patch_last = 0;
    ss.cnt_first = w.sun.counts; ss.cnt_retry = w.cnt_retry; ss.counts = w.sun.counts; ss.offsets = w.sun.offsets;
    ss.n_pts = w.sun.n_pts; ss.n_pts_copy = nullptr;
    ss.px = w.sun.px; ss.py = w.sun.py; ss.pz = w.sun.pz; ss.tmid = w.sun.tmid; ss.delta = w.sun.delta; ss.simg = w.sun.simg;
    return ss;
}

// The camera compositing launch of a chunk: it shades (do_shade) unless a shadow pass follows; then it counts the shadow rays' samples
// instead (count_sun) and the shadow pass's compositing launch shades
inline CompositeArgs camera_composite_args(const eonerf_ctx* ctx, const RenderWs& w, const float* flat, const float* rays, int n_rays, int p_cap, bool depth_only,
                                           const ShadeArgs& sh, bool shadows, const SampleArgs& ss) {
    CompositeArgs ca = composite_args(ctx, w, flat, rays, n_rays, p_cap, depth_only);
    ca.shade = sh; ca.do_shade = shadows ? 0 : 1;
    if (shadows) { ca.count_sun = 1; ca.sun = ss; }
    return ca;
}

// the shadow pass's compositing launch (transmittance at the last sample, then shading), from its chunk's camera compositing arguments
inline CompositeArgs shadow_composite_args(const CompositeArgs& ca, const RenderWs& w) {
    CompositeArgs cs = ca;
    cs.offsets = w.sun.offsets; cs.counts = w.sun.counts; cs.sigma = w.sun.sigma; cs.delta = w.sun.delta; cs.tmid = w.sun.tmid;
    cs.shadow_only = 1; cs.depth_only = 0; cs.count_sun = 0; cs.do_shade = 1;
    return cs;
}
