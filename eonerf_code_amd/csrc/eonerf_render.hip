// Sampling, rendering and the training step (eonerf_sample_rays, eonerf_rendering*, eonerf_presample*, eonerf_render_*): entry points of
// libeonerf_hip.so (include/eonerf_hip.h).  Host logic only: argument blocks and kernel sequencing over the caller's workspace.
#include "eonerf_ctx.h"
#include "eonerf_render_args.h"

int eo_run_mlp_fwd(eonerf_ctx* ctx, const PassBuffers& b, const float* flat, int p_cap, bool full, int mode, hipStream_t st, int prof_id, bool render_train) {
    if (!full) { const int rc = eo_ensure_density_streams(ctx, flat, st); if (rc) return rc; }
    const DevStream& ds = full ? ctx->fwd_full : ctx->fwd_dens;
    MlpFwdArgs a;
    a.px = b.px; a.py = b.py; a.pz = b.pz; a.simg = b.simg;
    a.emb = flat + ctx->pl.t[ctx->pl.emb].offset;
    a.n_pts = b.n_pts; a.p_pad = p_cap;
    a.stream = ds.data; a.chunks = ds.chunks; a.n_chunks = ds.n_chunks;
    a.sigma = b.sigma; a.albedo = b.albedo; a.ts = b.ts; a.tb = b.tb;
    a.act = b.act; a.masks = b.masks;
    a.range_flag = ctx->dev_status + RANGE_WORD;
    a.stagger = ctx->stagger;
    // training passes of the render path with the pipelined backward: the trunk's ReLU' comes from the X images, only the heads chain
    // reads mask bits (slot 7 = X_8 for its last layer)
    a.mask_from = (render_train && ctx->pipe) ? 7 : 0;
    if (ctx->prec == EONERF_F16X3 && mode != 0) return EONERF_E_UNSUPPORTED;      // the split precision is an inference precision
    ProfScope ps(ctx, prof_id, st);      // (prof_id < 0: off)
    return (int)eo_launch_mlp_fwd(a, ctx->prec, full, mode, chain_grid(ctx, p_cap), st);
}

// One pipelined launch of a backward call (eonerf_bwd_pipe.hip): trunk layers 7..1 of one pass, dX chain + weight gradients.  Reads dY_7
// from w.pipe.dy_in (written by the heads chain), accumulates dW / db of the trunk into d_flat, saves dY_5 / dY_0 in b.grd.  `slot` = which
// of the PIPE_LAUNCHES sync blocks it uses; the FIRST pipelined launch of the call (first_of_backward) zeroes all of them together with
// the GEMM's accumulator and work queue, which sit right in front (one memset for everything the backward needs zeroed).  A watchdog
// that fires goes to the context's STICKY status word (ctx->dev_status), which no launch clears.
static int run_bwd_pipe(eonerf_ctx* ctx, const RenderWs& w, const PassBuffers& b, int p_cap, float* d_flat, int prof_id, hipStream_t st, int slot, bool first_of_backward,
                        const AmbientBwdArgs* amb = nullptr) {
    const ParamLayout& pl = ctx->pl;
    if (first_of_backward) { const ZeroSpan z = backward_zero_span(w); HIP_TRY(hipMemsetAsync(z.base, 0, z.bytes, st)); }
    ProfScope ps(ctx, prof_id, st);
    BwdPipeArgs pa;
    memset(&pa, 0, sizeof(pa));
    uint32_t* sync = w.pipe.sync + (size_t)slot * (w.pipe.sync_bytes / sizeof(uint32_t));
    pa.n_pts = b.n_pts; pa.p_pad = p_cap; pa.n_pipes = ctx->n_pipes; pa.n_stages = PIPE_STAGES;
    pa.act = b.act; pa.grd = b.grd;
    pa.rings = w.pipe.rings; pa.role_counter = reinterpret_cast<int*>(sync) + 32; pa.error = ctx->dev_status;
    pa.scratch_word = sync + 64; pa.flags = sync + 64 + (size_t)ctx->n_pipes * PIPE_STAGES * 32;
    pa.d_flat = d_flat; pa.partials = w.det.pipe_part;
    pa.wt = ctx->pipe_wt.data; pa.dy_in = w.pipe.dy_in;
    pa.xcd_local = ctx->pipe_xcd;
    pa.fault_stage = ctx->pipe_fault_stage; pa.stamps = ctx->pipe_stamps;
    if (amb) { pa.amb = *amb; pa.amb_blocks = pipe_spare_cus(ctx); }
    for (int s = 0; s < PIPE_STAGES; ++s) {
        const int l = 7 - s;
        pa.dw_off[s] = pl.t[pl.trunk_w[l]].offset; pa.db_off[s] = pl.t[pl.trunk_b[l]].offset; pa.dw_ld[s] = l == 5 ? 319 : 256;
    }
    HIP_TRY(eo_launch_bwd_pipe(pa, st));
    if (pa.partials) HIP_TRY(eo_launch_pipe_reduce(pa, st));
    return 0;
}

// Weight gradients of up to two MLP passes in ONE split-K launch (eonerf_wgrad.hip; the jobs and their slices: eonerf_wgrad_plan.h) + the
// products that follow from the bottleneck factors.  defer_bott != nullptr: those products are NOT launched here; their arguments are
// handed back (the render path runs them in one launch with the embedding and ambient-head gradients, eo_launch_step_tail)
int eo_run_weight_gradients(eonerf_ctx* ctx, const float* flat, float* d_flat, const PassBuffers* full, const PassBuffers* dens, int p_cap, float* m_bott,
                            int* queue, hipStream_t st, WgradPlanOpts o, float* det_partials, BottWgradArgs* defer_bott) {
    const ParamLayout& pl = ctx->pl;
    auto dptr = [&](int ti) { return d_flat + pl.t[ti].offset; };
    o.riders = ctx->wgrad_riders; o.deterministic = det_partials != nullptr;
    WgradJobTable tab;
    if (!wgrad_plan(tab, full, dens, ctx->bf16, p_cap, ctx->n_cu, d_flat, pl, ctx->enc_colmap, m_bott, o)) return EONERF_E_UNSUPPORTED;
    if (full && !o.zeroed) HIP_TRY(hipMemsetAsync(m_bott, 0, BOTT_SCRATCH_F * sizeof(float), st));
    {
        ProfScope ps(ctx, EONERF_PROF_WGRAD, st);
        HIP_TRY(eo_launch_wgrad(tab, ctx->n_cu - (ctx->exch_event ? ctx->exch_cus : 0), p_cap, queue, ctx->bf16, st, det_partials, !o.zeroed));
    }
    if (full) {   // the three weight gradients that follow from the bottleneck factors the GEMM above accumulated
        BottWgradArgs bw;
        bw.w_a1 = flat + pl.t[pl.a1_w].offset; bw.m_a = m_bott; bw.db_at = m_bott + 2 * 128 * 256;
        bw.w_t1 = o.transient ? flat + pl.t[pl.t_w[0]].offset : nullptr; bw.m_t = m_bott + 128 * 256;
        bw.w_bott_t = ctx->fold + FOLD_FLOATS; bw.b_bott = flat + pl.t[pl.bot_b].offset;       // (the transposed copy is as current as the packed streams)
        bw.d_w = dptr(pl.bot_w); bw.d_b = dptr(pl.bot_b);
        bw.d_w_a1 = dptr(pl.a1_w); bw.d_b_a1 = dptr(pl.a1_b);
        bw.d_w_t1 = o.transient ? dptr(pl.t_w[0]) : nullptr; bw.d_b_t1 = o.transient ? dptr(pl.t_b[0]) : nullptr;
        if (defer_bott) *defer_bott = bw;
        else HIP_TRY(eo_launch_bott_wgrad(bw, st));
    }
    return 0;
}

// ---- argument blocks filled from (ctx, the carved workspace, the call's own pointers) ---------------------------------------------
static AmbientBwdArgs ambient_bwd_args(const eonerf_ctx* ctx, const RenderWs& w, const float* flat, const float* rays, int n_rays, float* d_flat) {
    const ParamLayout& pl = ctx->pl;
    AmbientBwdArgs ag;
    ag.w = ambient_w(ctx, flat); ag.rays = rays; ag.ray_rec = w.ray_rec; ag.g_ray = w.g_ray; ag.amb_save = w.amb_save; ag.n_rays = n_rays;
    ag.d_w1 = d_flat + pl.t[pl.am1_w].offset; ag.d_b1 = d_flat + pl.t[pl.am1_b].offset; ag.d_w2 = d_flat + pl.t[pl.am2_w].offset; ag.d_b2 = d_flat + pl.t[pl.am2_b].offset;
    return ag;
}
// d_emb_rays: deterministic mode's per-ray sums (DetWs::emb_rays), or nullptr
static EmbGradArgs emb_grad_args(const eonerf_ctx* ctx, const RenderWs& w, const int64_t* img_idx, int n_rays, float* d_flat, float* d_emb_rays) {
    EmbGradArgs eg;
    eg.n_samples = ctx->n_samples;
    eg.offsets = w.cam.offsets; eg.counts = w.cam.counts; eg.img_idx = img_idx; eg.g_emb = w.cam.g_emb; eg.d_emb = d_flat + ctx->pl.t[ctx->pl.emb].offset; eg.n_rays = n_rays;
    eg.lds_images = ctx->cfg.n_images <= 4096 ? ctx->cfg.n_images : 0; eg.d_emb_rays = d_emb_rays;
    return eg;
}
static PackedArgs packed_args(const RenderWs& w, const float* rays, const int64_t* img_idx, const float* t_starts, const float* t_ends, const int64_t* ray_indices, int n, int n_rays) {
    PackedArgs pa;
    pa.rays = rays; pa.img_idx = img_idx; pa.t_starts = t_starts; pa.t_ends = t_ends; pa.ray_indices = ray_indices;
    pa.n = n; pa.n_rays = n_rays; pa.counts = w.cam.counts; pa.offsets = w.cam.offsets; pa.n_pts = w.cam.n_pts;
    pa.px = w.cam.px; pa.py = w.cam.py; pa.pz = w.cam.pz; pa.tmid = w.cam.tmid; pa.delta = w.cam.delta; pa.simg = w.cam.simg;
    return pa;
}

// The camera pass backwards, from the gradient of the per-ray record (w.g_ray): compositing -> heads chain -> [pipelined trunk] -> weight
// gradients (together with the sun pass' remaining jobs, if any) -> embedding table and, with `ambient`, the per-ray ambient head.
// density_only: the pass was a density-only one (render_depth): its gradient flows through the sigma row alone.
static int camera_backward(eonerf_ctx* ctx, const RenderWs& w, const float* flat, const float* rays, const int64_t* img_idx, int n_rays, int p_cap,
                           float* d_flat, bool transient, bool ambient, bool first_pipe, const PassBuffers* sun, bool density_only, hipStream_t st,
                           const unsigned long long* digest = nullptr, bool sun_enc_done = false) {
    const ParamLayout& pl = ctx->pl;
    auto dptr = [&](int ti) { return d_flat + pl.t[ti].offset; };
    CompositeBwdArgs cb;
    memset(&cb, 0, sizeof(cb));
    cb.n_samples = ctx->n_samples;
    cb.rays = rays; cb.p_pad = p_cap; cb.n_rays = n_rays; cb.ray_rec = w.ray_rec; cb.g_ray = w.g_ray;
    cb.offsets = w.cam.offsets; cb.counts = w.cam.counts; cb.sigma = w.cam.sigma; cb.delta = w.cam.delta; cb.tmid = w.cam.tmid;
    cb.albedo = w.cam.albedo; cb.ts = w.cam.ts; cb.tb = w.cam.tb;
    cb.g_sigma = w.cam.g_sigma; cb.g_albedo = w.cam.g_albedo; cb.g_ts = w.cam.g_ts; cb.g_tb = w.cam.g_tb;
    cb.depth_only = density_only ? 1 : 0;
    if (sun && !density_only) { cb.sun_offsets = sun->offsets; cb.sun_counts = sun->counts; cb.sun_g_pos = sun->g_pos; }      // d depth of the shadow rays' origins
    if (digest) { cb.chk_a = digest; cb.chk_b = digest + 1; cb.chk_status = ctx->dev_status; }      // presample guard (eonerf_rays.h)
    HIP_TRY(eo_launch_cam_composite_bwd(cb, st));
    const bool pipe = ctx->pipe && w.pipe.dy_in;
    if (density_only) { const int rc = eo_ensure_density_streams(ctx, flat, st); if (rc) return rc; }
    const DevStream& bs = density_only ? (pipe ? ctx->bwd_dens_heads : ctx->bwd_dens)
                        : pipe ? (transient ? ctx->bwd_full_heads : ctx->bwd_rgb_heads) : (transient ? ctx->bwd_full : ctx->bwd_rgb);
    MlpBwdArgs mc = mlp_bwd_args(ctx, w.cam, p_cap, bs);
    mc.dy7_units = pipe ? w.pipe.dy_in : nullptr;
    { ProfScope ps(ctx, EONERF_PROF_BWD_CHAIN_CAMERA, st);
      HIP_TRY(eo_launch_mlp_bwd(mc, ctx->bf16, !density_only, density_only, transient && !density_only, chain_grid(ctx, p_cap), st, pipe ? 1 : 0)); }
    BottWgradArgs bott;
    if (pipe) {
        const int rcp = run_bwd_pipe(ctx, w, w.cam, p_cap, d_flat, EONERF_PROF_BWD_PIPE_CAMERA, st, 1, first_pipe); if (rcp) return rcp;
        // the trunk's pipelined layers are complete in d_flat here (the shadow pass' launch ran before this one)
        if (ctx->exch_event && !density_only) { HIP_TRY(hipEventRecord(ctx->exch_event, st)); ctx->exch_recorded = true; }
    }
    const PassBuffers *full = density_only ? nullptr : &w.cam, *dens = density_only ? &w.cam : sun;
    WgradPlanOpts o;
    o.transient = transient; o.dens_enc_done = sun_enc_done && !density_only;
    o.full_trunk_done = pipe; o.dens_trunk_done = pipe && dens;      // (accumulated by the pipelined launches)
    o.zeroed = pipe;                                                  // (by the call's first kernel or first pipelined launch: backward_zero_span)
    const int rcw = eo_run_weight_gradients(ctx, flat, d_flat, full, dens, p_cap, w.m_bott, w.queue, st, o, w.det.wgrad_part,
                                            (full && !ctx->deterministic) ? &bott : nullptr);
    if (rcw) return rcw;
    if (density_only) return EONERF_OK;
    if (!ctx->deterministic) {
        // the three independent tails of the backward -- bottleneck-factor products, embedding table, per-ray ambient head -- in ONE launch
        const EmbGradArgs eg = emb_grad_args(ctx, w, img_idx, n_rays, d_flat, nullptr);
        const AmbientBwdArgs ag = ambient_bwd_args(ctx, w, flat, rays, n_rays, d_flat);
        EncPartReduceArgs er;
        er.part = w.enc_part; er.n_wg = ctx->n_cu; er.dw0 = dptr(pl.trunk_w[0]); er.db0 = dptr(pl.trunk_b[0]); er.dw5s = dptr(pl.trunk_w[5]) + 256; er.col_map = ctx->enc_colmap;
        return (int)eo_launch_step_tail(&bott, transient ? &eg : nullptr, ambient ? &ag : nullptr, st, sun_enc_done ? &er : nullptr);
    }

    // ---- embeddings and the per-ray ambient head -----------------------------------------------------------
    if (transient) {
        const EmbGradArgs eg = emb_grad_args(ctx, w, img_idx, n_rays, d_flat, w.det.emb_rays);
        HIP_TRY(eo_launch_emb_grad(eg, st));
        if (eg.d_emb_rays) HIP_TRY(eo_launch_table_reduce(eg.d_emb_rays, img_idx, n_rays, 4, 4, ctx->cfg.n_images, 0, eg.d_emb, st));
    }
    if (!ambient) return EONERF_OK;      // s == 1: rgb = albedo, the ambient head is outside the graph (sat_rendering.py:269-276,294)
    // (27 -> 128 -> 3, fp32, ~35 us on a few dozen workgroups.  Running it on a side stream beside the weight-gradient GEMM was tried
    //  and bought nothing: every large kernel of the step holds the whole register file of its CUs -- 8 waves x 256 registers -- so
    //  the small kernel's workgroups only start when the large one's leave)
    HIP_TRY(eo_launch_ambient_bwd(ambient_bwd_args(ctx, w, flat, rays, n_rays, d_flat), st, ctx->deterministic));
    return EONERF_OK;
}

extern "C" {

size_t eonerf_render_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int flags) {
    if (!ctx || n_rays < 0) return 0;
    return carve_render(ctx, nullptr, n_rays, flags).bytes;
}

int eonerf_set_n_samples(eonerf_ctx* ctx, int n_samples) {
    if (!ctx) return EONERF_E_ARG;
    if (n_samples < 2 || n_samples > 256) return EONERF_E_UNSUPPORTED;
    ctx->n_samples = n_samples;
    return EONERF_OK;
}

int eonerf_set_noise_seed(eonerf_ctx* ctx, uint64_t seed) {
    if (!ctx) return EONERF_E_ARG;
    ctx->noise_seed = seed; ctx->noise_call = 0; ctx->pre.valid = false; ctx->pose.valid = false;
    return EONERF_OK;
}

int eonerf_sample_rays(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays,
                       int64_t* ray_indices, float* t_starts, float* t_ends, float* pts_per_ray, int* n_dev,
                       void* ws, size_t ws_bytes, void* stream) {
    return eo_sample_rays(ctx, rays, zsteps, u, perturb, n_rays, nullptr, 0, ray_indices, t_starts, t_ends, pts_per_ray, n_dev, ws, ws_bytes, stream);
}

}  // extern "C"

int eo_sample_rays(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays, const uint32_t* bits, int r,
                   int64_t* ray_indices, float* t_starts, float* t_ends, float* pts_per_ray, int* n_dev, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_rays == 0) return EONERF_OK;
    if (!ctx || !rays || !zsteps || !ray_indices || !t_starts || !t_ends || n_rays < 0 || !ws) return EONERF_E_ARG;
    RenderWs w = carve_render(ctx, ws, n_rays, EONERF_F_ONLY_DEPTH);
    drop_presample(ctx, ws);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    SampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n_samples = ctx->n_samples;
    sa.rays = rays; sa.zsteps = zsteps; sa.u = u; sa.n_rays = n_rays; sa.perturb = perturb ? 1 : 0;
    if (perturb && !u) { sa.seed = ctx->noise_seed; sa.call = ctx->noise_call++; }
    sa.cnt_first = w.cnt_first; sa.cnt_retry = w.cnt_retry; sa.counts = w.cam.counts; sa.offsets = w.cam.offsets;
    sa.flags = w.flags; sa.n_pts = w.cam.n_pts;
    sa.px = w.cam.px; sa.py = w.cam.py; sa.pz = w.cam.pz; sa.tmid = w.cam.tmid; sa.delta = w.cam.delta; sa.simg = w.cam.simg;
    sa.o_ray = ray_indices; sa.o_ts = t_starts; sa.o_te = t_ends;
    sa.occ_bits = bits; sa.occ_r = bits ? r : 0;
    HIP_TRY(eo_launch_sampler(sa, st));
    if (n_dev) HIP_TRY(hipMemcpyAsync(n_dev, w.cam.n_pts, sizeof(int), hipMemcpyDeviceToDevice, st));
    if (pts_per_ray) HIP_TRY(eo_launch_int_to_float(w.cam.counts, n_rays, pts_per_ray, st));
    return EONERF_OK;
}

extern "C" {

// EONerfMLP.rendering / render_depth on the caller's flattened samples.  train: under autograd (radiance_fields/eonerf.py:172-248) -- the
// same kernels with the training-mode forward chain (activations, masks and the compositing inputs stay in the workspace for
// eonerf_rendering_backward)
static int rendering_impl(bool train, eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                          const float* t_starts, const float* t_ends, const int64_t* ray_indices, int n, int n_rays, int depth_only,
                          float* albedo, float* depth, float* beta, float* transient_s, float* ambient, float* entropy,
                          void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !rays || !depth || n < 0 || n_rays < 1 || !ws) return EONERF_E_ARG;
    if (n > 0 && (!t_starts || !t_ends || !ray_indices)) return EONERF_E_ARG;
    if (!depth_only && (!albedo || !beta || !transient_s || !ambient || !entropy || !img_idx)) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (!rays_in_range(ctx, n_rays) || (train && !slabs_addressable(ctx, (size_t)p_cap_of(n_rays, ctx->n_samples)))) return EONERF_E_UNSUPPORTED;
    if ((long long)n > (long long)n_rays * (ctx->n_samples - 1)) return EONERF_E_UNSUPPORTED;           // at most n_samples - 1 intervals per ray
    if (train && ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }      // (after the fault fallback)
    const int flags = (train ? EONERF_F_TRAIN : 0) | (depth_only ? EONERF_F_ONLY_DEPTH : 0);
    RenderWs w = carve_render(ctx, ws, n_rays, flags);
    drop_presample(ctx, ws);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    if (train) note_train_forward(ctx, ws);
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);
    HIP_TRY(eo_launch_from_packed(packed_args(w, rays, img_idx, t_starts, t_ends, ray_indices, n, n_rays), st));
    int rc = eo_run_mlp_fwd(ctx, w.cam, flat, p_cap, !depth_only, train ? 1 : 0, st, -1, train);
    if (rc) return rc;
    HIP_TRY(eo_launch_composite_fwd(composite_args(ctx, w, flat, rays, n_rays, p_cap, depth_only != 0), st));
    RenderingOutArgs ro{w.ray_rec, n_rays, depth_only ? nullptr : albedo, depth, beta, transient_s, ambient, entropy};
    return (int)eo_launch_rendering_out(ro, st);
}

int eonerf_rendering(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                     const float* t_starts, const float* t_ends, const int64_t* ray_indices, int n, int n_rays, int depth_only,
                     float* albedo, float* depth, float* beta, float* transient_s, float* ambient, float* entropy,
                     void* ws, size_t ws_bytes, void* stream) {
    return rendering_impl(false, ctx, flat, rays, img_idx, t_starts, t_ends, ray_indices, n, n_rays, depth_only, albedo, depth, beta, transient_s, ambient, entropy, ws, ws_bytes, stream);
}
int eonerf_rendering_train(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                           const float* t_starts, const float* t_ends, const int64_t* ray_indices, int n, int n_rays, int depth_only,
                           float* albedo, float* depth, float* beta, float* transient_s, float* ambient, float* entropy,
                           void* ws, size_t ws_bytes, void* stream) {
    return rendering_impl(true, ctx, flat, rays, img_idx, t_starts, t_ends, ray_indices, n, n_rays, depth_only, albedo, depth, beta, transient_s, ambient, entropy, ws, ws_bytes, stream);
}

// gradients of the per-ray outputs (row-major as autograd hands them over; null = zero) -> ACCUMULATED parameter gradients.  `ws` must be
// the workspace an eonerf_rendering_train call with the same (rays, img_idx, n_rays, depth_only) filled.
int eonerf_rendering_backward(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx, int n_rays, int depth_only,
                              const float* g_albedo, const float* g_depth, const float* g_beta, const float* g_transient_s, const float* g_ambient,
                              float* d_flat, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !rays || !d_flat || n_rays < 1 || !ws) return EONERF_E_ARG;
    if (ctx->prec == EONERF_F16X3) return EONERF_E_UNSUPPORTED;
    if (!depth_only && !img_idx) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (!rays_in_range(ctx, n_rays) || !slabs_addressable(ctx, (size_t)p_cap_of(n_rays, ctx->n_samples))) return EONERF_E_UNSUPPORTED;      // (the forward's own bounds)
    ctx->pose.valid = false;
    PipeModeGuard mode(ctx, ws);
    const int flags = EONERF_F_TRAIN | (depth_only ? EONERF_F_ONLY_DEPTH : 0);
    RenderWs w = carve_render(ctx, ws, n_rays, flags);
    if (ctx->pre.valid && ctx->pre.ws == ws) return EONERF_E_STATE;      // eonerf_presample ran between this backward and its forward
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);
    RenderingOutBwdArgs rb{w.ray_rec, n_rays, depth_only ? nullptr : g_albedo, g_depth, depth_only ? nullptr : g_beta,
                           depth_only ? nullptr : g_transient_s, depth_only ? nullptr : g_ambient, w.g_ray};
    HIP_TRY(eo_launch_rendering_out_bwd(rb, st));
    return camera_backward(ctx, w, flat, rays, img_idx, n_rays, p_cap, d_flat, true, !depth_only, true, nullptr, depth_only != 0, st);
}

/* The camera pass's sampler of the NEXT eonerf_render_forward(EONERF_F_TRAIN, production noise), launched ahead of it: it reads the rays and
 * the seed only, so a data-parallel trainer runs it on the compute stream while the gradient all-reduce of the step before is in flight
 * (the exchange's serial tail).  The workspace must be free (the backward that used it has been enqueued on `stream`). */
int eonerf_presample(eonerf_ctx* ctx, const float* rays, const int64_t* img_idx, const float* zsteps, int n_rays, int flags,
                     int* n_samples_dev, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !rays || !img_idx || !zsteps || n_rays < 0 || !ws) return EONERF_E_ARG;
    if (!(flags & EONERF_F_TRAIN) || (flags & EONERF_F_ONLY_DEPTH)) return EONERF_E_STATE;
    ctx->pre.valid = false; ctx->pose.valid = false;
    if (n_rays == 0) return EONERF_OK;
    if (!rays_in_range(ctx, n_rays) || !slabs_addressable(ctx, (size_t)p_cap_of(n_rays, ctx->n_samples))) return EONERF_E_UNSUPPORTED;
    RenderWs w = carve_render(ctx, ws, n_rays, flags);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    SampleArgs sa = camera_sample_args(ctx, w, rays, img_idx, zsteps, nullptr, nullptr, n_rays, n_samples_dev);
    sa.call = ctx->noise_call++;
    // content guard: the sampler sums a digest of the rays it reads; the backward of the forward that consumes the record sums it again
    // from the same buffers and raises the status word if they were refilled in between (pointer identity alone cannot see that)
    unsigned long long* digest = reinterpret_cast<unsigned long long*>(ctx->dev_status + DIGEST_WORD);
    HIP_TRY(hipMemsetAsync(digest, 0, 2 * sizeof(unsigned long long), st));
    sa.digest = digest;
    HIP_TRY(eo_launch_sampler(sa, st));
    eonerf_ctx::Presample& p = ctx->pre;
    p.valid = true; p.ws = ws; p.rays = rays; p.img_idx = img_idx; p.zsteps = zsteps; p.count_out = n_samples_dev; p.n_rays = n_rays; p.flags = flags;
    p.n_samples = ctx->n_samples; p.pipe = ctx->pipe; p.call = sa.call;
    return EONERF_OK;
}

int eonerf_presample_cancel(eonerf_ctx* ctx) {
    if (!ctx) return EONERF_E_ARG;
    ctx->pre.valid = false;
    return EONERF_OK;
}

int eonerf_render_forward(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                          const float* zsteps, const float* u_cam, const float* u_retry, const float* u_sun,
                          int n_rays, int flags, float* out, int* n_samples_dev,
                          void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !rays || !img_idx || !zsteps || !out || n_rays < 0 || !ws) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    ctx->pose.valid = false;
    if (n_rays == 0) return EONERF_OK;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }
    const bool shadows = (flags & EONERF_F_SHADOWS) && !(flags & EONERF_F_ONLY_DEPTH);
    const bool train = flags & EONERF_F_TRAIN, od = flags & EONERF_F_ONLY_DEPTH;
    const bool philox = u_cam == nullptr;       // production: no noise buffers, the sampler draws its own jitter
    if (philox ? (u_retry || u_sun) : (shadows && !u_sun)) return EONERF_E_ARG;
    if (train && od) return EONERF_E_UNSUPPORTED;
    if (!rays_in_range(ctx, n_rays) || (train && !slabs_addressable(ctx, (size_t)p_cap_of(n_rays, ctx->n_samples)))) return EONERF_E_UNSUPPORTED;
    RenderWs w = carve_render(ctx, ws, n_rays, flags);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    if (train) note_train_forward(ctx, ws);
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);

    // ---- camera pass: sample -> field -> composite -------------------------------------------------------
    const eonerf_ctx::Presample pre = ctx->pre;
    const bool presampled = pre.valid && philox && pre.ws == ws && pre.rays == rays && pre.img_idx == img_idx && pre.zsteps == zsteps &&
                            pre.count_out == n_samples_dev && pre.n_rays == n_rays && pre.flags == flags && pre.n_samples == ctx->n_samples && pre.pipe == ctx->pipe;
    ctx->pre.valid = false;      // consumed, or dropped: this call's kernels write the workspace the record described (or the caller moved on)
    ctx->pre_consumed_ws = (presampled && train) ? ws : nullptr;
    SampleArgs sa = camera_sample_args(ctx, w, rays, img_idx, zsteps, u_cam, u_retry, n_rays, n_samples_dev, !train);      // (a training forward never culls)
    if (presampled) sa.call = pre.call;                       // (the shadow pass draws under the same call number)
    else {
        if (philox) sa.call = ctx->noise_call++;
        HIP_TRY(eo_launch_sampler(sa, st));
    }
    const bool rgb_loss = train && !shadows && (flags & EONERF_F_RGB_LOSS);
    int rc = eo_run_mlp_fwd(ctx, w.cam, flat, p_cap, !od, train ? (rgb_loss ? 2 : 1) : 0, st, EONERF_PROF_FWD_CHAIN_CAMERA, train);
    if (rc) return rc;
    // the chunk's LAST compositing launch shades; with the shadow pass on, the camera compositing counts the shadow rays' samples
    const ShadeArgs sh = shade_args(ctx, w, flat, img_idx, n_rays, shadows, flags, out);
    const SampleArgs ss = sun_sample_args(sa, w, u_sun);
    const CompositeArgs ca = camera_composite_args(ctx, w, flat, rays, n_rays, p_cap, od, sh, shadows, ss);
    HIP_TRY(eo_launch_composite_fwd(ca, st));

    // ---- sun pass ---------------------------------------------------------------------------------------------
    if (shadows) {
        HIP_TRY(eo_launch_sampler(ss, st, true));
        rc = eo_run_mlp_fwd(ctx, w.sun, flat, p_cap, false, train ? 1 : 0, st, EONERF_PROF_FWD_CHAIN_SUN, train);
        if (rc) return rc;
        HIP_TRY(eo_launch_composite_fwd(shadow_composite_args(ca, w), st));
    }
    return EONERF_OK;
}

// The ONE decision whether a render backward is refused.  true: the call ends here with *rc (EONERF_OK: an empty batch).  The workspace is
// measured in the layout of the path the forward ran on.  spend: a call refused behind that lookup has used the forward's path record up, as
// the backward itself does (PipeModeGuard); false: the record is left to the backward that follows (a caller with a launch in front of it)
static bool render_backward_refused(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx, int n_rays, int flags,
                                    const float* d_flat, const void* ws, size_t ws_bytes, bool spend, int* rc) {
    auto with = [&](int code) { *rc = code; return true; };
    if (!ctx || !flat || !rays || !img_idx || !d_flat || n_rays < 0 || !ws) return with(EONERF_E_ARG);
    if (!(flags & EONERF_F_TRAIN) || (flags & EONERF_F_ONLY_DEPTH)) return with(EONERF_E_STATE);
    if (ctx->prec == EONERF_F16X3) return with(EONERF_E_UNSUPPORTED);
    if (!ctx->weights_set) return with(EONERF_E_STATE);
    if (n_rays == 0) return with(EONERF_OK);
    if (!rays_in_range(ctx, n_rays) || !slabs_addressable(ctx, (size_t)p_cap_of(n_rays, ctx->n_samples))) return with(EONERF_E_UNSUPPORTED);
    PipeModeGuard mode(ctx, ws, false);
    const int bad = (ctx->pre.valid && ctx->pre.ws == ws) ? EONERF_E_STATE      // eonerf_presample ran between this backward and its forward
                  : ws_bytes < carve_render(ctx, nullptr, n_rays, flags).bytes ? EONERF_E_WORKSPACE : EONERF_OK;
    if (bad && spend) ctx->ws_pipe.erase(ws);
    return bad ? with(bad) : false;
}

struct LossSpec { const float *out, *pixels; int kind; float* loss; };      // fused loss (eonerf_render_backward_loss) or nullptr
// d_out (or, with ls, the loss gradient formed in the first kernel) -> ACCUMULATED parameter gradients; one of the two is given
static int render_backward_impl(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                                int n_rays, int flags, const float* d_out, const LossSpec* ls, float* d_flat,
                                void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int refusal;
    if (ctx) ctx->pose.valid = false;
    if (render_backward_refused(ctx, flat, rays, img_idx, n_rays, flags, d_flat, ws, ws_bytes, true, &refusal)) return refusal;
    PipeModeGuard mode(ctx, ws);
    const bool shadows = flags & EONERF_F_SHADOWS;
    ctx->exch_recorded = false;
    RenderWs w = carve_render(ctx, ws, n_rays, flags);
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);
    const ParamLayout& pl = ctx->pl;
    const int grid = chain_grid(ctx, p_cap);
    auto dptr = [&](int ti) { return d_flat + pl.t[ti].offset; };

    // ---- d out -> d ray record (+ radiometric table) -----------------------------------------------------
    ShadeBwdArgs sb;
    sb.ray_rec = w.ray_rec; sb.d_out = d_out; sb.img_idx = img_idx;
    sb.loss_kind = -1; sb.loss_out = nullptr; sb.loss_gt = nullptr; sb.loss = nullptr; sb.loss_scratch = nullptr;
    if (ls) { sb.loss_kind = ls->kind; sb.loss_out = ls->out; sb.loss_gt = ls->pixels; sb.loss = ls->loss; sb.loss_scratch = ctx->loss_scratch; }
    sb.radiometric = ctx->cfg.radiometric ? flat + pl.t[pl.rad].offset : nullptr;
    sb.d_radiometric = ctx->cfg.radiometric ? dptr(pl.rad) : nullptr;
    sb.g_ray = w.g_ray; sb.n_rays = n_rays; sb.use_shadow = shadows ? 1 : 0; sb.eval = (flags & EONERF_F_EVAL) ? 1 : 0;
    sb.lds_images = ctx->cfg.n_images <= 2048 ? ctx->cfg.n_images : 0;
    sb.d_rad_rays = sb.d_radiometric ? w.det.rad_rays : nullptr;
    const bool chk = ctx->pre_consumed_ws == ws;      // this backward's forward ran on presampled rays: digest of the buffers as they are now
    ctx->pre_consumed_ws = nullptr;
    unsigned long long* digest = reinterpret_cast<unsigned long long*>(ctx->dev_status + DIGEST_WORD);
    sb.chk_rays = chk ? rays : nullptr; sb.chk_sum = chk ? digest + 1 : nullptr;
    // pipelined path: this first kernel of the call also zeroes [bottleneck factors | GEMM queue | sync blocks] (backward_zero_span)
    const bool prezeroed = ctx->pipe && w.pipe.dy_in;
    sb.zero_base = nullptr; sb.zero_bytes = 0;
    if (prezeroed) {
        const ZeroSpan z = backward_zero_span(w);
        sb.zero_base = reinterpret_cast<uint32_t*>(z.base); sb.zero_bytes = z.bytes;
        if ((reinterpret_cast<uintptr_t>(z.base) | z.bytes) & 15) return EONERF_E_STATE;
    }
    HIP_TRY(eo_launch_shade_bwd(sb, st));
    if (sb.d_rad_rays) HIP_TRY(eo_launch_table_reduce(sb.d_rad_rays, img_idx, n_rays, 6, 9, ctx->cfg.n_images, sb.eval, sb.d_radiometric, st));

    CompositeBwdArgs cb;
    memset(&cb, 0, sizeof(cb));
    cb.n_samples = ctx->n_samples;
    cb.rays = rays; cb.p_pad = p_cap; cb.n_rays = n_rays; cb.ray_rec = w.ray_rec; cb.g_ray = w.g_ray;
    bool ambient_done = false, sun_enc_done = false;

    // ---- shadow pass backwards: d geo -> d sigma_sun -> (chain, input grad) -> d pos -> d depth -----------
    if (shadows) {
        CompositeBwdArgs cs = cb;
        cs.offsets = w.sun.offsets; cs.counts = w.sun.counts; cs.sigma = w.sun.sigma; cs.delta = w.sun.delta;
        cs.g_sigma = w.sun.g_sigma; cs.g_pos = w.sun.g_pos;
        HIP_TRY(eo_launch_sun_composite_bwd(cs, st));
        const bool pipe_sun = ctx->pipe && w.pipe.dy_in;
        MlpBwdArgs ms = mlp_bwd_args(ctx, w.sun, p_cap, pipe_sun ? ctx->bwd_dens_heads : ctx->bwd_dens);
        if (pipe_sun) {      // heads (sigma row) -> pipelined trunk -> input-gradient tail
            ms.dy7_units = w.pipe.dy_in;
            { ProfScope ps(ctx, EONERF_PROF_BWD_CHAIN_SUN, st); HIP_TRY(eo_launch_mlp_bwd(ms, true, false, true, false, grid, st, true)); }
            // (the spare CUs of this launch take the ambient-head backward: its inputs -- g_ray, the saved head activations -- are final)
            const AmbientBwdArgs ag = ambient_bwd_args(ctx, w, flat, rays, n_rays, d_flat);
            ambient_done = pipe_spare_cus(ctx) > 0;
            const int rcp = run_bwd_pipe(ctx, w, w.sun, p_cap, d_flat, EONERF_PROF_BWD_PIPE_SUN, st, 0, !prezeroed, ambient_done ? &ag : nullptr);
            if (rcp) return rcp;
            if (w.enc_part) {
                // ONE pass over the dY_0 / dY_5 tiles the launch above left: d sigma / d position (needed now: it flows into the camera pass)
                // and the pass' two weight-gradient products against the encoding (otherwise two jobs of the GEMM launch at the end)
                EncPairArgs ea;
                ea.n_pts = w.sun.n_pts; ea.p_pad = p_cap; ea.grd = w.sun.grd; ea.act = w.sun.act; ea.wt = ctx->ig_tail_wt.data;
                ea.px = w.sun.px; ea.py = w.sun.py; ea.pz = w.sun.pz; ea.g_pos = w.sun.g_pos;
                ea.part = w.enc_part;
                { ProfScope ps(ctx, EONERF_PROF_IG_TAIL_SUN, st); HIP_TRY(eo_launch_enc_pair(ea, ctx->n_cu, st)); }
                sun_enc_done = true;
            } else {
                IgTailArgs ta;
                ta.n_pts = w.sun.n_pts; ta.p_pad = p_cap; ta.grd = w.sun.grd; ta.wt = ctx->ig_tail_wt.data;
                ta.px = w.sun.px; ta.py = w.sun.py; ta.pz = w.sun.pz; ta.g_pos = w.sun.g_pos;
                { ProfScope ps(ctx, EONERF_PROF_IG_TAIL_SUN, st); HIP_TRY(eo_launch_ig_tail(ta, ctx->n_cu, st)); }
            }
        } else {
            ProfScope ps(ctx, EONERF_PROF_BWD_CHAIN_SUN, st);
            HIP_TRY(eo_launch_mlp_bwd(ms, ctx->bf16, false, true, false, grid, st));
        }
    }

    const int rcc = camera_backward(ctx, w, flat, rays, img_idx, n_rays, p_cap, d_flat, shadows || !(flags & EONERF_F_RGB_LOSS), shadows && !ambient_done, !shadows && !prezeroed,
                                    shadows ? &w.sun : nullptr, false, st, chk ? digest : nullptr, sun_enc_done);
    // (chain + GEMM path: the trunk's gradients come out of the GEMM launch -- the early block is final where everything is)
    if (!rcc && ctx->exch_event && !ctx->exch_recorded) HIP_TRY(hipEventRecord(ctx->exch_event, st));
    if (!rcc) {      // (ctx->pipe is the forward's path here: PipeModeGuard)
        ctx->pose.valid = true; ctx->pose.ws = ws; ctx->pose.n_rays = n_rays; ctx->pose.flags = flags; ctx->pose.n_samples = ctx->n_samples;
        ctx->pose.pipe = ctx->pipe && w.pipe.dy_in;
    }
    return rcc;
}

int eonerf_render_backward(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                           int n_rays, int flags, const float* d_out, float* d_flat,
                           void* ws, size_t ws_bytes, void* stream) {
    if (!d_out) return EONERF_E_ARG;
    return render_backward_impl(ctx, flat, rays, img_idx, n_rays, flags, d_out, nullptr, d_flat, ws, ws_bytes, stream);
}

int eonerf_render_backward_loss(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx,
                                int n_rays, int flags, const float* out, const float* pixels, int kind, float* d_out_scratch, float* loss,
                                float* d_flat, void* ws, size_t ws_bytes, void* stream) {
    if (!ctx || !out || !pixels || !loss || (kind != 0 && kind != 1) || n_rays < 1) return EONERF_E_ARG;
    if ((n_rays + 255) / 256 > LOSS_MAX_BLOCKS) {      // beyond the fused kernel's ticket sum: the two calls it replaces
        if (!d_out_scratch) return EONERF_E_ARG;
        // (the loss kernel writes d_out_scratch and *loss: nothing is launched for a call the backward behind it will refuse)
        int rc;
        if (render_backward_refused(ctx, flat, rays, img_idx, n_rays, flags, d_flat, ws, ws_bytes, false, &rc)) return rc;
        rc = eonerf_train_loss(ctx, out, pixels, n_rays, kind, d_out_scratch, loss, stream);
        return rc ? rc : render_backward_impl(ctx, flat, rays, img_idx, n_rays, flags, d_out_scratch, nullptr, d_flat, ws, ws_bytes, stream);
    }
    const LossSpec ls{out, pixels, kind, loss};
    return render_backward_impl(ctx, flat, rays, img_idx, n_rays, flags, nullptr, &ls, d_flat, ws, ws_bytes, stream);
}

}  // extern "C"
