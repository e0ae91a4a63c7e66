// Block-wise early ray termination (include/eonerf_march.h): a pass of an export render in rounds of `block` sampler slots.  Per round
// the windowed emit (k_march_emit) writes the round's samples of the rays still alive compactly, the chain kernels run over them
// unchanged, and the compositing kernel (k_march_composite) continues every ray's sums from its state, decides whether the ray lives on
// and counts its next window.  One wave per ray, as in eonerf_rays.hip; rounds are separate launches on the caller's stream -- no kernel
// waits for another.  Built with -ffp-contract=off: the sample arithmetic is sample_ray's, bit for bit.
#include "eonerf_ctx.h"
#include "eonerf_render_args.h"
#include "eonerf_rays_dev.h"
#include "eonerf_march_dev.h"
#include "../../include/eonerf_march.h"

namespace {

// ---- begin of a pass: the full first-draw and retry-draw counts (the dense call's k_count), each draw's last valid slot and first
//      window count, and the ray's march state ---------------------------------------------------------------------------------------
template <int SPL> EO_DEV void ray_summary(const RaySamples<SPL>& s, int block, int& cnt, int& last, int& win) {
    cnt = 0; last = -1;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const unsigned long long mk = __ballot(s.valid[k]);
        cnt += __popcll(mk);
        if (mk) last = 64 * k + 63 - __clzll(mk);
        if (k == 0) win = __popcll(mk & (block == 64 ? ~0ull : (1ull << block) - 1ull));
    }
}
template <int SPL, bool GRID>
EO_DEV void march_begin_ray(const MarchArgs& m, int ray, int lane, const RayGeom& g) {
    const SampleArgs& a = m.s;
    float u[SPL];
    jitter<SPL>(a, a.u, a.sun_pass ? 2 : 0, ray, lane, u);
    RaySamples<SPL> s = sample_ray<SPL>(a.zsteps, a.n_samples, a.perturb, u, g.near, g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, lane);
    if constexpr (GRID) cull_by_grid<SPL>(s, a.occ_bits, a.occ_r, lane);
    int cnt, last, win;
    ray_summary<SPL>(s, m.block, cnt, last, win);
    int cnt_r = cnt, last_r = last, win_r = win;
    if (a.retry) {
        jitter<SPL>(a, a.u_retry, 1, ray, lane, u);
        RaySamples<SPL> s2 = sample_ray<SPL>(a.zsteps, a.n_samples, a.perturb, u, 0.f, g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, lane);
        if constexpr (GRID) cull_by_grid<SPL>(s2, a.occ_bits, a.occ_r, lane);
        ray_summary<SPL>(s2, m.block, cnt_r, last_r, win_r);
    }
    if (lane == 0) {
        a.cnt_first[ray] = cnt; m.last_a[ray] = last; m.win_a[ray] = win;
        if (a.retry) { a.cnt_retry[ray] = cnt_r; m.last_b[ray] = last_r; m.win_b[ray] = win_r; }
        m.alive[ray] = 1; m.kept[ray] = 0; m.od[ray] = 0.f;
    }
    if (m.acc && lane < MARCH_ACC) m.acc[(size_t)ray * MARCH_ACC + lane] = 0.f;
}
template <int SPL, bool GRID>
__global__ __launch_bounds__(256) void k_march_begin(MarchArgs m) {
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) { m.s.flags[0] = 0; if (m.n_total) *m.n_total = 0; }
    if (ray >= m.s.n_rays) return;
    march_begin_ray<SPL, GRID>(m, ray, lane, ray_geom(m.s, ray));
}

// eonerf_march_sample_round: the window counts of an arbitrary round under the caller's alive mask
template <bool GRID>
__global__ __launch_bounds__(256) void k_march_wcount(MarchArgs m, const int* alive) {
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= m.s.n_rays) return;
    const int n = (!alive || alive[ray]) ? window_count<GRID>(m, ray, lane, m.round, false) : 0;
    if (lane == 0) m.win_a[ray] = n;
}

// ---- the round's scan on its own (batches beyond SCAN_FUSED_MAX_RAYS): offsets, counts, totals and -- deciding round -- the retry flag
constexpr int SCAN_FUSED_MAX_RAYS = 8192;
__global__ __launch_bounds__(1024) void k_march_scan(MarchArgs m) {
    const SampleArgs& a = m.s;
    __shared__ int wsum[16];
    __shared__ int carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool retry = false;
    if (a.retry) {
        if (m.decide) {
            int any = 0;
            for (int i = tid; i < a.n_rays; i += 1024) any |= a.cnt_first[i] == 0 ? 1 : 0;
            retry = __syncthreads_or(any) != 0;
        } else retry = (a.flags[0] & 1) != 0;
    }
    const int* cnt = retry ? m.win_b : m.win_a;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < a.n_rays; base += 1024) {
        const int i = base + tid;
        const int v = i < a.n_rays ? cnt[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int c = carry;
        if (i < a.n_rays) { a.offsets[i] = c + woff + incl - v; a.counts[i] = v; }
        __syncthreads();
        if (tid == 1023) carry = c + woff + incl;
        __syncthreads();
    }
    if (tid == 0) {
        if (m.decide) a.flags[0] = retry ? 1 : 0;
        a.offsets[a.n_rays] = carry; *a.n_pts = carry;
        if (m.n_total) *m.n_total += carry;
    }
}

// ---- windowed emit: the round's valid slots of every ray with a non-empty window, compact in ray order.  SCAN: as k_emit's -- every
//      block sums the window counts in front of its own rays itself and (deciding round) takes the retry decision from the full counts
template <bool SCAN, bool GRID>
__global__ __launch_bounds__(256) void k_march_emit(MarchArgs m) {
    const SampleArgs& a = m.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ray = blockIdx.x * RAYS_PER_BLOCK + wave;
    // the deciding round: the fused scan decides below; behind k_march_scan the decision is already in flags[0]
    bool retry = a.retry && (SCAN ? !m.decide : true) && (a.flags[0] & 1);
    int off = 0, n = 0;
    if constexpr (SCAN) {
        __shared__ int s_red[RAYS_PER_BLOCK][5];
        const int base = blockIdx.x * RAYS_PER_BLOCK;
        const bool both = a.retry && m.decide;
        int v[5] = {0, 0, 0, 0, 0};      // counts in front of this block (first draw, retry draw), totals (first, retry), any empty ray
        for (int i = threadIdx.x; i < a.n_rays; i += 256) {
            const int wa = retry ? m.win_b[i] : m.win_a[i], wb = both ? m.win_b[i] : wa;
            v[2] += wa; v[3] += wb; v[4] |= (both && a.cnt_first[i] == 0) ? 1 : 0;
            if (i < base) { v[0] += wa; v[1] += wb; }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v[q], o, 64); v[q] = q == 4 ? (v[q] | t) : (v[q] + t); }
        }
        if (lane == 0) { for (int q = 0; q < 5; ++q) s_red[wave][q] = v[q]; }
        __syncthreads();
        int t[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) t[q] = q == 4 ? (s_red[0][q] | s_red[1][q] | s_red[2][q] | s_red[3][q]) : (s_red[0][q] + s_red[1][q]) + (s_red[2][q] + s_red[3][q]);
        const bool second = both && t[4] != 0;      // this round decides, and decides for the retry draw
        if (both) retry = second;
        const int* cnt = retry ? m.win_b : m.win_a;
        off = second ? t[1] : t[0];
        for (int j = base; j < ray && j < a.n_rays; ++j) off += cnt[j];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const int total = second ? t[3] : t[2];
            if (m.decide) a.flags[0] = retry ? 1 : 0;
            a.offsets[a.n_rays] = total; *a.n_pts = total;
            if (m.n_total) *m.n_total += total;
        }
        if (ray < a.n_rays) { n = cnt[ray]; if (lane == 0) { a.offsets[ray] = off; a.counts[ray] = n; } }
    } else {
        if (ray < a.n_rays) { off = a.offsets[ray]; n = a.counts[ray]; }
    }
    if (ray >= a.n_rays || n == 0) return;
    const int last = retry ? m.last_b[ray] : m.last_a[ray];
    const WinSample s = window_of<GRID>(m, ray, lane, m.round, retry, last);
    const unsigned long long mk = __ballot(s.valid);
    const int rank = __popcll(mk & ((1ull << lane) - 1ull));
    if (!s.valid || rank >= n) return;      // (rank < n: n is this window's count by the same function; the guard keeps every store inside the round's span)
    const int p = off + rank;
    a.px[p] = s.x; a.py[p] = s.y; a.pz[p] = s.z;
    a.simg[p] = a.img_idx ? (int)a.img_idx[ray] : 0;
    a.tmid[p] = s.mid;
    // camera pass: the ray's overall last valid slot ends at 1e10 (k_emit: rank == n - 1 of the whole ray)
    const float te = (a.patch_last && m.round * m.block + lane == last) ? 1e10f : s.te;
    a.delta[p] = __fsub_rn(te, s.ts);
    if (a.o_ts) { a.o_ray[p] = ray; a.o_ts[p] = s.ts; a.o_te[p] = s.te; }
}

// ---- compositing with carry: the round's at most `block` <= 64 samples of a ray, one per lane, continue the ray's sums -----------------
template <bool GRID>
__global__ __launch_bounds__(256) void k_march_composite(MarchArgs m) {
    const SampleArgs& a = m.s;
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    if (!m.alive[ray]) return;      // (its window count is 0 since the round it stopped in)
    const bool retry = a.retry && (a.flags[0] & 1);
    const int off = a.offsets[ray], n = a.counts[ray];
    const int last = retry ? m.last_b[ray] : m.last_a[ray];
    const float od = m.od[ray];
    const float sd = lane < n ? m.sigma[off + lane] * a.delta[off + lane] : 0.f;
    const float inc = wave_incl_scan(sd, lane);
    const float prev = __shfl_up(inc, 1, 64);      // exclusive prefix = the previous lane's inclusive one (ray_weights: never "inclusive - self")
    const float T = expf(-(lane == 0 ? od : od + prev));
    const float w = lane < n ? T * (1.f - expf(-sd)) : 0.f;
    const float od_new = od + __shfl(inc, 63, 64);
    if (!m.geo) {
        float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // depth, albedo3, ts, tb, wsum
        if (lane < n) {
            const int p = off + lane;
            acc[0] = w * a.tmid[p];
            if (!m.depth_only) {
                acc[1] = w * m.albedo[p];
                acc[2] = w * m.albedo[(size_t)m.p_pad + p];
                acc[3] = w * m.albedo[2 * (size_t)m.p_pad + p];
                acc[4] = w * m.ts[p];
                acc[5] = w * m.tb[p];
            }
            acc[6] = w;
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) acc[j] = wave_sum(acc[j]);
        if (n > 0) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 7; ++j) v = lane == j ? acc[j] : v;
            if (lane < 7) m.acc[(size_t)ray * MARCH_ACC + lane] += v;
        }
    }
    // the ray's last valid slot lies in this round: it was kept, geo_shadows is the transmittance in front of it
    const bool ends_here = last >= 0 && last / m.block == m.round;
    const float T_last = __shfl(T, n > 0 ? n - 1 : 0, 64);
    const bool more = last >= (m.round + 1) * m.block;
    const bool lives = more && expf(-od_new) >= m.eps;
    const int next = lives ? window_count<GRID>(m, ray, lane, m.round + 1, retry) : 0;
    if (lane == 0) {
        if (m.geo) {
            if (ends_here && n > 0) m.geo[(size_t)ray * RAY_REC] = T_last;
            else if (more && !lives) m.geo[(size_t)ray * RAY_REC] = expf(-od_new);      // died at this boundary: < eps
        }
        m.od[ray] = od_new; m.kept[ray] += n;
        m.alive[ray] = lives ? 1 : 0;
        m.win_a[ray] = next;
        if (retry) m.win_b[ray] = next;
    }
}

// ---- behind the last camera round: the ray record from the sums, the ambient head once per ray, and -- with a shadow pass -- the begin
//      of the shadow ray that starts at the depth just rendered --------------------------------------------------------------------------
struct FinishArgs {
    MarchArgs sun; int count_sun;
    const float *rays, *acc; float* ray_rec;
    AmbientW amb; int n_rays, depth_only;
};
template <int SPL, bool GRID>
__global__ __launch_bounds__(256) void k_march_finish_cam(FinishArgs f) {
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= f.n_rays) return;
    const float* r = f.rays + (size_t)ray * 11;
    const float* acc = f.acc + (size_t)ray * MARCH_ACC;
    float amb[3] = {0.f, 0.f, 0.f};
    if (!f.depth_only) {
        const AmbientRay ar = ambient_forward(f.amb, r[8], r[9], r[10], lane);
        amb[0] = ar.out[0]; amb[1] = ar.out[1]; amb[2] = ar.out[2];
    }
    const float depth = acc[0];
    if (lane == 0) {
        float* o = f.ray_rec + (size_t)ray * RAY_REC;
        o[RR_DEPTH] = depth;
        o[RR_ALB + 0] = acc[1]; o[RR_ALB + 1] = acc[2]; o[RR_ALB + 2] = acc[3];
        o[RR_TS] = acc[4];
        o[RR_TB] = acc[5] + 0.05f;                      // beta_min, as k_composite_fwd
        o[RR_WSUM] = acc[6];
        o[RR_AMB + 0] = amb[0]; o[RR_AMB + 1] = amb[1]; o[RR_AMB + 2] = amb[2];
        o[RR_GEO] = 1.0f; o[RR_GEO + 1] = 0.f;
    }
    if (f.count_sun) march_begin_ray<SPL, GRID>(f.sun, ray, lane, sun_geom(r, depth));
}

hipError_t launch_begin(const MarchArgs& m, hipStream_t st) {
    const dim3 blocks((m.s.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    eo_dispatch_spl(m.s.n_samples, [&](auto spl) {
        dispatch_grid(m.s.occ_bits, [&](auto grid) {
            hipLaunchKernelGGL((k_march_begin<decltype(spl)::value, decltype(grid)::value>), blocks, dim3(256), 0, st, m);
        });
    });
    return hipGetLastError();
}
hipError_t launch_emit(const MarchArgs& m, hipStream_t st) {
    const dim3 blocks((m.s.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    dispatch_grid(m.s.occ_bits, [&](auto grid) {
        constexpr bool GRID = decltype(grid)::value;
        if (m.s.n_rays <= SCAN_FUSED_MAX_RAYS) hipLaunchKernelGGL((k_march_emit<true, GRID>), blocks, dim3(256), 0, st, m);
        else {
            hipLaunchKernelGGL(k_march_scan, dim3(1), dim3(1024), 0, st, m);
            hipLaunchKernelGGL((k_march_emit<false, GRID>), blocks, dim3(256), 0, st, m);
        }
    });
    return hipGetLastError();
}
hipError_t launch_composite(const MarchArgs& m, hipStream_t st) {
    const dim3 blocks((m.s.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    dispatch_grid(m.s.occ_bits, [&](auto grid) { hipLaunchKernelGGL((k_march_composite<decltype(grid)::value>), blocks, dim3(256), 0, st, m); });
    return hipGetLastError();
}
hipError_t launch_finish_cam(const FinishArgs& f, int n_samples, hipStream_t st) {
    const dim3 blocks((f.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    eo_dispatch_spl(n_samples, [&](auto spl) {
        dispatch_grid(f.count_sun ? f.sun.s.occ_bits : nullptr, [&](auto grid) {
            hipLaunchKernelGGL((k_march_finish_cam<decltype(spl)::value, decltype(grid)::value>), blocks, dim3(256), 0, st, f);
        });
    });
    return hipGetLastError();
}

}  // namespace

hipError_t eo_march_launch_begin(const MarchArgs& m, hipStream_t st) { return launch_begin(m, st); }
hipError_t eo_march_launch_emit(const MarchArgs& m, hipStream_t st) { return launch_emit(m, st); }

extern "C" {

int eonerf_march_version(void) { return EONERF_MARCH_VERSION; }

size_t eonerf_march_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int flags, int block) {
    if (!ctx || n_rays < 0 || !march_block_ok(block)) return 0;
    return carve_march(carve_cfg(ctx), nullptr, n_rays, flags, block).bytes;
}

int eonerf_render_forward_march(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx, const float* zsteps,
                                const float* u_cam, const float* u_retry, const float* u_sun, int n_rays, int flags,
                                float early_stop_eps, int block, float* out, int* n_samples_dev, int* kept,
                                void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !rays || !img_idx || !zsteps || !out || n_rays < 0 || !ws) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    int rc = march_refusal(flags, early_stop_eps, block, 0, 0);      // the call's own arguments; the workspace below
    if (rc) return rc;
    if (n_rays == 0) return EONERF_OK;
    const bool od = flags & EONERF_F_ONLY_DEPTH, shadows = (flags & EONERF_F_SHADOWS) && !od;
    const bool philox = u_cam == nullptr;
    if (philox ? (u_retry || u_sun) : (shadows && !u_sun)) return EONERF_E_ARG;
    if (!rays_in_range(ctx, n_rays)) return EONERF_E_UNSUPPORTED;
    const MarchWs w = carve_march(carve_cfg(ctx), ws, n_rays, flags, block);
    rc = march_refusal(flags, early_stop_eps, block, ws_bytes, w.bytes);
    if (rc) return rc;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }
    drop_presample(ctx, ws);
    const int rounds = march_rounds(ctx->n_samples, block);

    // ---- camera pass ---------------------------------------------------------------------------------------------------------------
    RenderWs none;
    memset(&none, 0, sizeof(none));
    MarchArgs mc;
    memset(&mc, 0, sizeof(mc));
    mc.s = camera_sample_args(ctx, none, rays, img_idx, zsteps, u_cam, u_retry, n_rays, nullptr, true);
    if (philox) mc.s.call = ctx->noise_call++;      // one call number per render
    mc.s.cnt_first = w.cnt_first; mc.s.cnt_retry = w.cnt_retry; mc.s.flags = w.flags;
    round_outputs(mc.s, w);
    mc.block = block; mc.win_a = w.win_first; mc.win_b = w.win_retry; mc.last_a = w.last_first; mc.last_b = w.last_retry;
    mc.n_total = n_samples_dev;
    mc.alive = w.alive; mc.kept = kept ? kept : w.kept_cam; mc.od = w.od; mc.acc = w.acc; mc.geo = nullptr;
    mc.eps = early_stop_eps;
    mc.sigma = w.round.sigma; mc.albedo = w.round.albedo; mc.ts = w.round.ts; mc.tb = w.round.tb; mc.p_pad = w.p_cap; mc.depth_only = od ? 1 : 0;
    HIP_TRY(launch_begin(mc, st));
    for (int j = 0; j < rounds; ++j) {
        mc.round = j; mc.decide = j == 0 ? 1 : 0;
        HIP_TRY(launch_emit(mc, st));
        rc = eo_run_mlp_fwd(ctx, w.round, flat, w.p_cap, !od, 0, st, EONERF_PROF_FWD_CHAIN_CAMERA);
        if (rc) return rc;
        HIP_TRY(launch_composite(mc, st));
    }

    // ---- the ray record; the shadow pass from the depth just rendered ----------------------------------------------------------------
    MarchArgs ms = mc;
    ms.s.img_idx = nullptr; ms.s.u = u_sun; ms.s.u_retry = nullptr; ms.s.retry = 0;
    ms.s.depth = w.ray_rec + RR_DEPTH; ms.s.depth_stride = RAY_REC; ms.s.sun_pass = 1; ms.s.patch_last = 0;
    ms.s.cnt_first = w.sun_cnt; ms.s.cnt_retry = w.sun_cnt;
    ms.win_a = ms.win_b = w.sun_win; ms.last_a = ms.last_b = w.sun_last;
    ms.n_total = nullptr; ms.decide = 0; ms.round = 0;
    ms.kept = kept ? kept + n_rays : w.kept_sun; ms.acc = nullptr; ms.geo = w.ray_rec + RR_GEO; ms.depth_only = 1;
    FinishArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.sun = ms; fa.count_sun = shadows ? 1 : 0;
    fa.rays = rays; fa.acc = w.acc; fa.ray_rec = w.ray_rec; fa.amb = ambient_w(ctx, flat); fa.n_rays = n_rays; fa.depth_only = od ? 1 : 0;
    HIP_TRY(launch_finish_cam(fa, ctx->n_samples, st));
    if (shadows) {
        for (int j = 0; j < rounds; ++j) {
            ms.round = j;
            HIP_TRY(launch_emit(ms, st));
            rc = eo_run_mlp_fwd(ctx, w.round, flat, w.p_cap, false, 0, st, EONERF_PROF_FWD_CHAIN_SUN);
            if (rc) return rc;
            HIP_TRY(launch_composite(ms, st));
        }
    }
    // shading through shade_ray: columns 14 / 15 are the dense call's FULL counts (first draw; the shadow ray from the march's depth)
    ShadeArgs sh;
    sh.ray_rec = w.ray_rec; sh.img_idx = img_idx;
    sh.radiometric = ctx->cfg.radiometric ? flat + ctx->pl.t[ctx->pl.rad].offset : nullptr;
    sh.pts_first = w.cnt_first; sh.sc_counts = shadows ? w.sun_cnt : w.cnt_first;
    sh.n_rays = n_rays; sh.use_shadow = shadows ? 1 : 0; sh.eval = (flags & EONERF_F_EVAL) ? 1 : 0; sh.out = out;
    return (int)eo_launch_shade_fwd(sh, st);
}

int eonerf_march_sample_round(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays,
                              int round, int block, const int* alive, int64_t* ray_indices, float* t_starts, float* t_ends, int* n_out,
                              void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !rays || !zsteps || !ray_indices || !t_starts || !t_ends || !n_out || n_rays < 0 || !ws) return EONERF_E_ARG;
    if (!march_block_ok(block) || round < 0 || round >= march_rounds(ctx->n_samples, block)) return EONERF_E_ARG;
    if (n_rays == 0) return EONERF_OK;
    if (!rays_in_range(ctx, n_rays)) return EONERF_E_UNSUPPORTED;
    const MarchWs w = carve_march(carve_cfg(ctx), ws, n_rays, EONERF_F_ONLY_DEPTH, block);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    drop_presample(ctx, ws);
    MarchArgs m;
    memset(&m, 0, sizeof(m));
    SampleArgs& sa = m.s;
    sa.n_samples = ctx->n_samples;
    sa.rays = rays; sa.zsteps = zsteps; sa.u = u; sa.n_rays = n_rays; sa.perturb = perturb ? 1 : 0;
    if (perturb && !u) { sa.seed = ctx->noise_seed; sa.call = ctx->noise_call++; }
    sa.cnt_first = w.cnt_first; sa.cnt_retry = w.cnt_retry; sa.flags = w.flags;
    round_outputs(sa, w);
    sa.o_ray = ray_indices; sa.o_ts = t_starts; sa.o_te = t_ends;
    if (ctx->occ_bits) { sa.occ_bits = ctx->occ_bits; sa.occ_r = ctx->occ_r; }
    m.round = round; m.block = block; m.decide = 0;
    m.win_a = w.win_first; m.win_b = w.win_retry; m.last_a = w.last_first; m.last_b = w.last_retry;
    m.alive = w.alive; m.kept = w.kept_cam; m.od = w.od; m.acc = w.acc;
    HIP_TRY(launch_begin(m, st));
    const dim3 blocks((n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    if (sa.occ_bits) hipLaunchKernelGGL((k_march_wcount<true>), blocks, dim3(256), 0, st, m, alive);
    else hipLaunchKernelGGL((k_march_wcount<false>), blocks, dim3(256), 0, st, m, alive);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_emit(m, st));
    HIP_TRY(hipMemcpyAsync(n_out, w.round.n_pts, sizeof(int), hipMemcpyDeviceToDevice, st));
    return EONERF_OK;
}

}  // extern "C"
