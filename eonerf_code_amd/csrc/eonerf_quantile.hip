// Quantile depth (include/eonerf_quantile.h): the distance at which a camera ray's optical depth crosses L_q = -log1p(-q).  Dense mode
// runs the ONLY_DEPTH forward's sampler and density-chain launches with the forward's arguments (eonerf_render_args.h) and one
// compositing launch of its own; march mode runs the pass in eonerf_march.h's rounds (begin and windowed emit: eonerf_march.hip's) with
// a compositing kernel that carries the optical depth as k_march_composite does.  One wave per ray, no LDS, no atomics.
// Built with -ffp-contract=off: the rule is written in separately rounded fp32 operations.
#include <math.h>
#include "eonerf_ctx.h"
#include "eonerf_render_args.h"
#include "eonerf_rays_dev.h"
#include "eonerf_march_dev.h"
#include "../../include/eonerf_quantile.h"

namespace {

struct QuantileArgs {
    int n_q; float L[QUANTILE_MAX];      // L_q per requested quantile, ascending
    float* out;                          // [R][2 + n_q]
    const float *o_ts, *o_te;            // the sampler's interval ends of the samples being composited
    float* s_sigma;                      // dense mode: the caller's copy of the densities, or nullptr
};

// t_q inside the bracket sample: E = the optical depth in front of it
EO_DEV float quantile_t(float L, float E, float sigma, float ts, float te) {
    return ts + fminf(fmaxf((L - E) / sigma, 0.f), te - ts);      // (fmaxf: a 0 / 0 of a tied, empty bracket counts as 0)
}

// ---- dense: the forward's compositing of the depth column (ray_weights, the same accumulation order), then the brackets ----------------
template <int SPL>
__global__ __launch_bounds__(256) void k_quantile_dense(CompositeArgs a, QuantileArgs q) {
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const int off = a.offsets[ray], n = a.counts[ray];
    const RayWeights<SPL> rw = ray_weights<SPL>(a.sigma, a.delta, off, n, lane);
    float depth = 0.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        if (i < n) depth += rw.w[k] * a.tmid[off + i];
    }
    depth = wave_sum(depth);
    // inclusive prefix of element i = the exclusive prefix of element i + 1 (never "inclusive - self"); behind the last lane of a group
    // stands the next group's first element, behind the last group the total
    float I[SPL], sg[SPL], ts[SPL], te[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        const float next = __shfl_down(rw.ex[k], 1, 64);
        const float head = k + 1 < SPL ? __shfl(rw.ex[k + 1 < SPL ? k + 1 : k], 0, 64) : rw.total;
        I[k] = lane == 63 ? head : next;
        sg[k] = ts[k] = te[k] = 0.f;
        if (i < n) { sg[k] = a.sigma[off + i]; ts[k] = q.o_ts[off + i]; te[k] = q.o_te[off + i]; }
        if (q.s_sigma && i < n) q.s_sigma[off + i] = sg[k];
    }
    float* o = q.out + (size_t)ray * (2 + q.n_q);
    const int last = n - 1;
    if (lane == 0) o[0] = depth;
    if (n == 0) { if (lane < 1 + q.n_q) o[1 + lane] = 0.f; return; }
#pragma unroll
    for (int k = 0; k < SPL; ++k)
        if (lane + 64 * k == last) o[1] = rw.ex[k];      // od_front = E_{n-1}
    const float te_last = q.o_te[off + last];
    for (int j = 0; j < q.n_q; ++j) {
        const float L = q.L[j];
        bool found = false;
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const unsigned long long mk = __ballot(lane + 64 * k < n && I[k] >= L);
            if (!found && mk) {      // (wave-uniform) the first set lane owns the bracket
                found = true;
                if (lane == __ffsll(mk) - 1) o[2 + j] = quantile_t(L, rw.ex[k], sg[k], ts[k], te[k]);
            }
        }
        if (!found && lane == 0) o[2 + j] = te_last;
    }
}

// ---- march: k_march_composite's depth sum and decisions, with the brackets of the round the optical depth crosses L_q in -----------------
template <bool GRID>
__global__ __launch_bounds__(256) void k_quantile_march(MarchArgs m, QuantileArgs q) {
    const SampleArgs& a = m.s;
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    if (!m.alive[ray]) return;      // (its window count is 0 since the round it stopped in)
    const bool retry = a.retry && (a.flags[0] & 1);
    const int off = a.offsets[ray], n = a.counts[ray];
    const int last = retry ? m.last_b[ray] : m.last_a[ray];
    const float od = m.od[ray];
    float sg = 0.f, ts = 0.f, te = 0.f, dl = 0.f, mid = 0.f;
    if (lane < n) { const int p = off + lane; sg = m.sigma[p]; dl = a.delta[p]; mid = a.tmid[p]; ts = q.o_ts[p]; te = q.o_te[p]; }
    const float sd = lane < n ? sg * dl : 0.f;
    const float inc = wave_incl_scan(sd, lane);
    const float prev = __shfl_up(inc, 1, 64);      // exclusive prefix = the previous lane's inclusive one (ray_weights: never "inclusive - self")
    const float E = lane == 0 ? od : od + prev;
    const float I = od + inc;                      // (= the next lane's E)
    const float T = expf(-E);
    const float w = lane < n ? T * (1.f - expf(-sd)) : 0.f;
    const float od_new = od + __shfl(inc, 63, 64);
    const float part = wave_sum(lane < n ? w * mid : 0.f);
    const bool more = last >= (m.round + 1) * m.block;
    const bool lives = more && expf(-od_new) >= m.eps;
    const int next = lives ? window_count<GRID>(m, ray, lane, m.round + 1, retry) : 0;
    float* o = q.out + (size_t)ray * (2 + q.n_q);
    // an alive ray without a further round ends here: its last valid slot lies in this round (n > 0), or it has no sample at all
    const float te_end = n > 0 ? q.o_te[off + n - 1] : 0.f;
    for (int j = 0; j < q.n_q; ++j) {
        const float L = q.L[j];
        if (od < L && L <= od_new) {      // this round decides (then n > 0): the first lane at or beyond L, the round's last sample on a tie of the two sums
            const unsigned long long mk = __ballot(lane < n && I >= L);
            const int b = mk ? __ffsll(mk) - 1 : n - 1;
            if (lane == b) o[2 + j] = quantile_t(L, E, sg, ts, te);
        } else if (!lives && od_new < L) {
            if (lane == 0) o[2 + j] = te_end;
        }
    }
    const float E_last = __shfl(E, n > 0 ? n - 1 : 0, 64);
    if (lane == 0) {
        const float depth = n > 0 ? m.acc[(size_t)ray * MARCH_ACC] + part : m.acc[(size_t)ray * MARCH_ACC];
        m.acc[(size_t)ray * MARCH_ACC] = depth;
        if (!lives) {
            o[0] = depth;
            o[1] = more ? od_new : (n > 0 ? E_last : 0.f);      // died at this boundary: OD_j*; else E of the ray's last sample
        }
        m.od[ray] = od_new; m.kept[ray] += n;
        m.alive[ray] = lives ? 1 : 0;
        m.win_a[ray] = next;
        if (retry) m.win_b[ray] = next;
    }
}

hipError_t launch_dense(const CompositeArgs& a, const QuantileArgs& q, hipStream_t st) {
    const dim3 blocks((a.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    eo_dispatch_spl(a.n_samples, [&](auto spl) { hipLaunchKernelGGL((k_quantile_dense<decltype(spl)::value>), blocks, dim3(256), 0, st, a, q); });
    return hipGetLastError();
}
hipError_t launch_march(const MarchArgs& m, const QuantileArgs& q, hipStream_t st) {
    const dim3 blocks((m.s.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    dispatch_grid(m.s.occ_bits, [&](auto grid) { hipLaunchKernelGGL((k_quantile_march<decltype(grid)::value>), blocks, dim3(256), 0, st, m, q); });
    return hipGetLastError();
}

bool quantile_rays_ok(const eonerf_ctx* ctx, int n_rays) { return sweep_rays_addressable(n_rays, ctx->n_samples) && rays_in_range(ctx, n_rays); }

}  // namespace

extern "C" {

int eonerf_quantile_version(void) { return EONERF_QUANTILE_VERSION; }

size_t eonerf_quantile_workspace_bytes(const eonerf_ctx* ctx, int n_rays, int n_q, int block) {
    if (!ctx || n_rays < 0 || n_q < 1 || n_q > QUANTILE_MAX || !quantile_block_ok(block) || !quantile_rays_ok(ctx, n_rays)) return 0;
    return carve_quantile(carve_cfg(ctx), nullptr, n_rays, block).bytes;
}

int eonerf_render_depth_quantiles(eonerf_ctx* ctx, const float* flat, const float* rays, const float* zsteps, const float* u_cam,
                                  const float* u_retry, int n_rays, const float* quantiles, int n_q, float early_stop_eps, int block,
                                  float* out, int* n_samples_dev, int64_t* s_ray, float* s_ts, float* s_te, float* s_sigma,
                                  void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !rays || !zsteps || !quantiles || !out || n_rays < 0 || !ws) return EONERF_E_ARG;
    const int n_s = (s_ray ? 1 : 0) + (s_ts ? 1 : 0) + (s_te ? 1 : 0) + (s_sigma ? 1 : 0);
    if (n_s != 0 && n_s != 4) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (n_q < 1 || n_q > QUANTILE_MAX) return EONERF_E_ARG;
    QuantileArgs qa;
    memset(&qa, 0, sizeof(qa));
    double L_max = 0.0;
    for (int j = 0; j < n_q; ++j) {
        const float qj = quantiles[j];
        if (!(qj > 0.0f && qj < 1.0f) || (j > 0 && !(qj > quantiles[j - 1]))) return EONERF_E_ARG;      // (NaN fails every comparison)
        L_max = -log1p(-(double)qj);
        qa.L[j] = (float)L_max;
    }
    if (!(early_stop_eps >= 0.0f && early_stop_eps < 1.0f)) return EONERF_E_ARG;
    const bool march = early_stop_eps > 0.0f;
    if (march && !march_block_ok(block)) return EONERF_E_ARG;
    if (march && !(L_max * (1.0 + 1e-4) < -log((double)early_stop_eps))) return EONERF_E_ARG;      // every bracket among the kept samples
    if (march && n_s) return EONERF_E_UNSUPPORTED;
    if (n_rays == 0) return EONERF_OK;
    const bool philox = u_cam == nullptr;       // production: no noise buffers, the sampler draws its own jitter
    if (philox && u_retry) return EONERF_E_ARG;
    if (!quantile_rays_ok(ctx, n_rays)) return EONERF_E_UNSUPPORTED;
    const QuantileWs w = carve_quantile(carve_cfg(ctx), ws, n_rays, march ? block : 0);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }
    ctx->pre.valid = false; ctx->pose.valid = false;      // dropped: this call's kernels write the workspace the record described (or the caller moved on)
    qa.n_q = n_q; qa.out = out;

    if (!march) {
        // ---- the ONLY_DEPTH forward's sampler and chain launches; the sampler also leaves its flattened outputs ---------------------
        SampleArgs sa = camera_sample_args(ctx, w.r, rays, nullptr, zsteps, u_cam, u_retry, n_rays, n_samples_dev, true);
        if (philox) sa.call = ctx->noise_call++;
        sa.o_ray = n_s ? s_ray : w.o_ray; sa.o_ts = n_s ? s_ts : w.o_ts; sa.o_te = n_s ? s_te : w.o_te;
        HIP_TRY(eo_launch_sampler(sa, st));
        const int rc = eo_run_mlp_fwd(ctx, w.r.cam, flat, w.p_cap, false, 0, st, EONERF_PROF_FWD_CHAIN_CAMERA, false);
        if (rc) return rc;
        qa.o_ts = sa.o_ts; qa.o_te = sa.o_te; qa.s_sigma = s_sigma;
        return (int)launch_dense(composite_args(ctx, w.r, flat, rays, n_rays, w.p_cap, true), qa, st);
    }

    // ---- the camera pass of eonerf_render_forward_march(EONERF_F_ONLY_DEPTH), with the quantile compositing per round -----------------
    const MarchWs& mw = w.m;
    RenderWs none;
    memset(&none, 0, sizeof(none));
    MarchArgs mc;
    memset(&mc, 0, sizeof(mc));
    mc.s = camera_sample_args(ctx, none, rays, nullptr, zsteps, u_cam, u_retry, n_rays, nullptr, true);
    if (philox) mc.s.call = ctx->noise_call++;
    mc.s.cnt_first = mw.cnt_first; mc.s.cnt_retry = mw.cnt_retry; mc.s.flags = mw.flags;
    round_outputs(mc.s, mw);
    mc.s.o_ray = w.o_ray; mc.s.o_ts = w.o_ts; mc.s.o_te = w.o_te;
    mc.block = block; mc.win_a = mw.win_first; mc.win_b = mw.win_retry; mc.last_a = mw.last_first; mc.last_b = mw.last_retry;
    mc.n_total = n_samples_dev;
    mc.alive = mw.alive; mc.kept = mw.kept_cam; mc.od = mw.od; mc.acc = mw.acc; mc.geo = nullptr;
    mc.eps = early_stop_eps;
    mc.sigma = mw.round.sigma; mc.p_pad = mw.p_cap; mc.depth_only = 1;
    qa.o_ts = w.o_ts; qa.o_te = w.o_te;
    HIP_TRY(eo_march_launch_begin(mc, st));
    const int rounds = march_rounds(ctx->n_samples, block);
    for (int j = 0; j < rounds; ++j) {
        mc.round = j; mc.decide = j == 0 ? 1 : 0;
        HIP_TRY(eo_march_launch_emit(mc, st));
        const int rc = eo_run_mlp_fwd(ctx, mw.round, flat, mw.p_cap, false, 0, st, EONERF_PROF_FWD_CHAIN_CAMERA);
        if (rc) return rc;
        HIP_TRY(launch_march(mc, qa, st));
    }
    return EONERF_OK;
}

}  // extern "C"
