// Sun sweep (include/eonerf_sweep.h): one camera pass, then per sun direction the launches eonerf_render_forward makes behind its camera
// chain -- camera compositing (ambient head, shadow-ray counts), sun sampler, density-only chain, shadow compositing + shading -- with
// the arguments eonerf_render_forward passes (eonerf_render_args.h), on a workspace whose first bytes are eonerf_render_forward's carve.
// The only device code of its own is the copy of the ray table with the sun columns replaced.
#include "eonerf_render_args.h"
#include "../../include/eonerf_sweep.h"

namespace {

// table[r][0..7] = rays[r][0..7], table[r][8..10] = sun[0..2]: one thread per word of the [n_rays][11] table
__global__ __launch_bounds__(256) void k_sweep_rays(const float* __restrict__ rays, const float* __restrict__ sun, size_t n_words, float* __restrict__ table) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    const int c = (int)(i % 11);
    table[i] = c < 8 ? rays[i] : sun[c - 8];
}

}  // namespace

extern "C" {

int eonerf_sweep_version(void) { return EONERF_SWEEP_VERSION; }

size_t eonerf_sun_sweep_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int n_suns) {
    if (!ctx || n_rays < 0 || n_suns < 1 || !sweep_rays_addressable(n_rays, ctx->n_samples)) return 0;
    return carve_sweep(carve_cfg(ctx), nullptr, n_rays).bytes;
}

int eonerf_render_sun_sweep(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx, const float* zsteps,
                            const float* u_cam, const float* u_retry, const float* u_sun, const float* suns, int n_suns, int n_rays,
                            int flags, float* out, int* n_samples_dev, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !rays || !img_idx || !zsteps || !suns || !out || !ws || n_suns < 1 || n_rays < 0) return EONERF_E_ARG;
    const bool philox = u_cam == nullptr;       // production: no noise buffers, the sampler draws its own jitter
    if (philox ? (u_retry || u_sun) : !u_sun) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (n_rays == 0) return EONERF_OK;
    if (flags & (EONERF_F_TRAIN | EONERF_F_ONLY_DEPTH)) return EONERF_E_UNSUPPORTED;
    // (rays_in_range admits batches whose sample capacity wraps an int between 129 and 255 samples per ray: the exact bound first)
    if (!sweep_rays_addressable(n_rays, ctx->n_samples) || !rays_in_range(ctx, n_rays)) return EONERF_E_UNSUPPORTED;
    const SweepWs s = carve_sweep(carve_cfg(ctx), ws, n_rays);
    if (ws_bytes < s.bytes) return EONERF_E_WORKSPACE;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }
    const RenderWs& w = s.r;
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);
    const int fwd_flags = (flags & EONERF_F_EVAL) | EONERF_F_SHADOWS;
    ctx->pre.valid = false; ctx->pose.valid = false;      // dropped: this call's kernels write the workspace the record described (or the caller moved on)

    // ---- camera pass, once: sample -> field.  Its sampler reads columns 0..6 of the table only ----------------
    SampleArgs sa = camera_sample_args(ctx, w, rays, img_idx, zsteps, u_cam, u_retry, n_rays, n_samples_dev, true);      // (honours the context's occupancy grid)
    if (philox) sa.call = ctx->noise_call++;      // the ONE call number of the sweep: every shadow pass draws under it
    HIP_TRY(eo_launch_sampler(sa, st));
    int rc = eo_run_mlp_fwd(ctx, w.cam, flat, p_cap, true, 0, st, EONERF_PROF_FWD_CHAIN_CAMERA, false);
    if (rc) return rc;
    sa.rays = s.table;      // from here on the launches read the table copy: the forward's `rays` with this sun in columns 8..10

    // ---- per sun: table copy -> camera compositing (ambient head, shadow-ray counts) -> sun sampler -> density chain -> shadow compositing
    const size_t n_words = (size_t)n_rays * 11;
    for (int k = 0; k < n_suns; ++k) {
        hipLaunchKernelGGL(k_sweep_rays, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, rays, suns + (size_t)k * 3, n_words, s.table);
        HIP_TRY(hipGetLastError());
        const float* u_k = u_sun ? u_sun + (size_t)k * n_rays * ctx->n_samples : nullptr;
        float* out_k = out + (size_t)k * n_rays * 21;
        const ShadeArgs sh = shade_args(ctx, w, flat, img_idx, n_rays, true, fwd_flags, out_k);
        const SampleArgs ss = sun_sample_args(sa, w, u_k);
        const CompositeArgs ca = camera_composite_args(ctx, w, flat, s.table, n_rays, p_cap, false, sh, true, ss);
        HIP_TRY(eo_launch_composite_fwd(ca, st));
        HIP_TRY(eo_launch_sampler(ss, st, true));
        rc = eo_run_mlp_fwd(ctx, w.sun, flat, p_cap, false, 0, st, EONERF_PROF_FWD_CHAIN_SUN, false);
        if (rc) return rc;
        HIP_TRY(eo_launch_composite_fwd(shadow_composite_args(ca, w), st));
    }
    return EONERF_OK;
}

}  // extern "C"
