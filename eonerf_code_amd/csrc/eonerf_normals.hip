// Density gradient and surface normals (include/eonerf_normals.h).  k_sigma_jvp is the density-only inference chain of
// eonerf_mlp_fwd.hip in FORWARD mode: a sample occupies the four columns (lanes) of a quad -- plane 0 its value, planes 1..3 the
// derivatives along x, y, z -- and every plane goes through the same packed weights (WStream, run_layer, TileSched and the density-only
// streams as they are).  A derivative column takes no bias and the ReLU decision of its quad's plane 0, one DPP quad broadcast away.
// Columns of an MFMA are independent, so plane 0 is the inference chain's own column bit for bit.  k_normal_composite forms the per-ray
// sums of the header's rule, one wave per ray.  Built with -ffp-contract=off: the rule is written in separately rounded fp32 operations
// (plane 0 has no operation a contraction could change: the encoder's scale by 2^k is exact).
#include <math.h>
#include "eonerf_ctx.h"
#include "eonerf_render_args.h"
#include "eonerf_rays_dev.h"
#include "eonerf_normals_check.h"

namespace {

struct JvpArgs {
    const float *px, *py, *pz;     // [p_pad] compact sample positions (SoA)
    const int* n_pts;              // device scalar: number of live samples
    int p_pad;
    const uint8_t* stream;         // the density-only packed stream of the context's precision
    const ChunkDesc* chunks;
    int n_chunks;
    float* sigma;                  // [p_pad]
    float* grad;                   // [3][p_pad]
    int* range_flag;               // fp16 x 3 policy: as MlpFwdArgs::range_flag, over all four planes
};

// the value of the quad's plane-0 lane (v_mov_b32_dpp quad_perm:[0,0,0,0]); every lane of the wave is active where this is called
EO_DEV float quad0(float v) {
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x00, 0xf, 0xf, true));
}

// run_layer's bias selector: the lane's half picks the bias rows, and only plane 0 takes them
struct PlaneSel { int h; bool primal; };
EO_DEV f32x16 bias_init(const uint8_t* bias32, PlaneSel s) {
    const f32x16 b = ::bias_init(bias32, s.h);
    f32x16 r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = s.primal ? b[i] : 0.f;
    return r;
}

template <class P> struct EncUnits { typename P::U u[ENC_SLOTS / P::KF]; };

// encoding slots of one column (eonerf_common.h: half 0 sin(2^k c) | x | y, half 1 sin(2^k c + pi/2) | z | pad).  Plane 0: the chain's own
// encoder.  Plane 1 + j: the derivative along coordinate j -- 2^k cos(arg) at the fp32 argument plane 0 takes the sine of, in the
// slots of coordinate j; 1 in the raw slot of coordinate j; 0 elsewhere
template <class P>
EO_DEV EncUnits<P> encode_plane(float x, float y, float z, int h, int plane) {
    EncUnits<P> E;
    const float off = h ? EO_PI_2_F : 0.0f;
    constexpr int NU = ENC_SLOTS / P::KF;
#pragma unroll
    for (int kg = 0; kg < NU; ++kg)
#pragma unroll
        for (int e = 0; e < P::NE; ++e) {
            const int q = kg * P::NE + e;
            float v;
            if (q < 30) {
                const int k = q / 3, d = q % 3;
                const float c = d == 0 ? x : (d == 1 ? y : z);
                const float arg = c * (float)(1 << k) + off;
                if (plane == 0) v = sinf(arg);
                else v = plane == d + 1 ? (float)(1 << k) * cosf(arg) : 0.0f;
            } else if (q == 30) {
                v = plane == 0 ? (h ? z : x) : (plane == (h ? 3 : 1) ? 1.0f : 0.0f);
            } else {
                v = h ? 0.0f : (plane == 0 ? y : (plane == 2 ? 1.0f : 0.0f));
            }
            set_elem(E.u[kg], e, v);
        }
    return E;
}

// epilogue slice of a trunk layer: every plane keeps its accumulator where the quad's plane 0 is positive.  In plane 0 this IS the
// chain's ReLU (relu_slice), NaN behaviour of the split policy included
EO_DEV Sl<PF32> jvp_slice(PF32, const f32x16& acc, int s, uint32_t&) {
    const float a0 = acc[2 * s], a1 = acc[2 * s + 1];
    const float p0 = quad0(a0), p1 = quad0(a1);
    return Sl<PF32>{p0 > 0.f ? a0 : 0.f, p1 > 0.f ? a1 : 0.f};
}
// split policy: the running maximum of relu_slice is taken on the magnitudes (a derivative may be negative), so mask_commit sees every
// operand the next layer multiplies
EO_DEV Sl<PH3> jvp_slice(PH3, const f32x16& acc, int s, uint32_t& bits) {
    const float p0 = quad0(acc[2 * s]), p1 = quad0(acc[2 * s + 1]);
    const float a0 = !(p0 <= 0.f) ? acc[2 * s] : 0.f, a1 = !(p1 <= 0.f) ? acc[2 * s + 1] : 0.f;
    const uint32_t b0 = __builtin_bit_cast(uint32_t, a0) & 0x7fffffffu, b1 = __builtin_bit_cast(uint32_t, a1) & 0x7fffffffu;
    const uint32_t m01 = b0 > b1 ? b0 : b1;
    bits = s == 0 ? m01 : (bits > m01 ? bits : m01);
    return split_pair(a0, a1);
}

template <class P>
__global__ __launch_bounds__(P::NT) void k_sigma_jvp(JvpArgs a) {
    constexpr int SLOT = FwdSlot<P>::BYTES;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    typedef typename P::U U;
    constexpr int HKG = 256 / P::KF;
    constexpr int EKG = ENC_SLOTS / P::KF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int plane = c & 3;                 // a wave tile starts at a multiple of 32 columns: the quad of lanes is the quad of planes
    const int n_pts = *a.n_pts;
    const PlaneSel sel{h, plane == 0};

    WStream<P, SLOT> ws;
    ws.g = a.stream; ws.tab = a.chunks; ws.lds = smem; ws.n_chunks = a.n_chunks;
    ws.wave_b = __builtin_amdgcn_readfirstlane(wave) * 1024; ws.lane_b = lane * 16;
    const TileSched<P> sched(4 * n_pts, gridDim.x, blockIdx.x);      // columns, four per sample (n_pts <= EONERF_NORMALS_MAX_POINTS)
    if (sched.iters() == 0) return;      // uniform per workgroup
    ws.start();

    for (int it = 0; it < sched.iters(); ++it) {
        const int wt = sched.first(it) + __builtin_amdgcn_readfirstlane(wave);      // this wave's 32 columns = 8 samples
        if (__builtin_amdgcn_readfirstlane(wave) >= sched.waves(it)) { ws.idle_tile(); continue; }
        const int p = wt * 8 + (c >> 2);     // this lane's sample (the four lanes of a quad and both halves share it)
        const bool live = p < n_pts;
        const float x = live ? a.px[p] : 0.f, y = live ? a.py[p] : 0.f, z = live ? a.pz[p] : 0.f;
        const EncUnits<P> E = encode_plane<P>(x, y, z, h, plane);
        NoSlab mid;
        U H[HKG], N[HKG];
        uint32_t rflag = 0;      // split policy: wave-uniform "an operand of this tile left fp16's range" (mask_commit(PH3))
        if constexpr (P::IS_SPLIT) {
            // the raw coordinates are operands of layer 0 and of the skip layer; the derivative planes' encoding is bounded by 2^9
            rflag = __builtin_amdgcn_ballot_w64(!(fabsf(x) <= 65504.f && fabsf(y) <= 65504.f && fabsf(z) <= 65504.f)) != 0ull ? 1u : 0u;
        }
        uint32_t tbits = 0;
        auto epi = [&](U* dst, int mt, const f32x16& accv, int s) {
            const Sl<P> v = jvp_slice(P(), accv, s, tbits);
            put_slice(P(), dst, mt, s, v);
            if constexpr (P::IS_SPLIT) { if (s == EPI_SLICES - 1) mask_commit(P(), mt, tbits, rflag); }
        };
        auto plain_layer = [&](U* src, U* dst) {
            run_layer<P, SLOT, HKG, 8, true>(ws, mid, lane, sel, [&](int kg) { return src[kg]; },
                [&](int mt, const f32x16& v, int s) { epi(dst, mt, v, s); });
        };

        // layer 0: enc(64) -> 256
        run_layer<P, SLOT, EKG, 8, true>(ws, mid, lane, sel, [&](int kg) { return E.u[kg]; },
            [&](int mt, const f32x16& v, int s) { epi(H, mt, v, s); });
        plain_layer(H, N);
        plain_layer(N, H);
        plain_layer(H, N);
        plain_layer(N, H);
        // layer 5 consumes [h, enc]: the skip re-reads the encoding, derivative planes included
        run_layer<P, SLOT, HKG + EKG, 8, true>(ws, mid, lane, sel,
            [&](int kg) { return kg < HKG ? H[kg < HKG ? kg : 0] : E.u[kg >= HKG ? kg - HKG : 0]; },
            [&](int mt, const f32x16& v, int s) { epi(N, mt, v, s); });
        plain_layer(N, H);
        plain_layer(H, N);
        // sigma row: plane 0 the raw density, planes 1..3 its derivatives
        float raw = 0.f;
        run_layer<P, SLOT, HKG, 1, true>(ws, mid, lane, sel, [&](int kg) { return N[kg]; },
            [&](int, const f32x16& v, int s) { if (s == 0) raw = v[0]; });
        const float raw0 = quad0(raw);
        if (h == 0 && live) {
            if (plane == 0) a.sigma[p] = softplus_f(raw);
            else a.grad[(size_t)(plane - 1) * a.p_pad + p] = raw / (1.f + expf(-raw0));      // softplus' = sigmoid (1 beyond its threshold of 20, in fp32)
        }
        if constexpr (P::IS_SPLIT) {
            if (rflag != 0u && lane == 0) atomicOr(a.range_flag, 1);      // (wave-uniform condition)
        }
    }
}

template <class P>
hipError_t launch_jvp(const JvpArgs& a, int grid, hipStream_t st) {
    constexpr int SMEM = 2 * FwdSlot<P>::BYTES;
    static EoAttrOnce attr;
    {
        const hipError_t e = attr.ensure([&] { return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sigma_jvp<P>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, SMEM); });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_sigma_jvp<P>), dim3(grid), dim3(P::NT), SMEM, st, a);
    return hipGetLastError();
}

// one launch of the four-column chain over the samples of `b`; grad = [3][p_cap]
int run_sigma_jvp(eonerf_ctx* ctx, const PassBuffers& b, const float* flat, int p_cap, float* grad, hipStream_t st) {
    const int rc = eo_ensure_density_streams(ctx, flat, st);
    if (rc) return rc;
    const DevStream& ds = ctx->fwd_dens;
    JvpArgs a;
    a.px = b.px; a.py = b.py; a.pz = b.pz; a.n_pts = b.n_pts; a.p_pad = p_cap;
    a.stream = ds.data; a.chunks = ds.chunks; a.n_chunks = ds.n_chunks;
    a.sigma = b.sigma; a.grad = grad;
    a.range_flag = ctx->dev_status + RANGE_WORD;
    static_assert(PF32::TILE == PH3::TILE, "one grid rule");
    const int grid = std::min(ctx->n_cu, 4 * (p_cap / PF32::TILE));      // persistent workgroups, never more than column tiles
    return (int)(ctx->prec == EONERF_F16X3 ? launch_jvp<PH3>(a, grid, st) : launch_jvp<PF32>(a, grid, st));
}

struct NormalArgs {
    float* out;                    // [R][5]
    const float* grad;             // [3][p_pad]
    float ax, ay, az;              // axis_scale
    float *s_sigma, *s_grad;       // the caller's copies of the densities and the (unscaled) gradients, or nullptr
};

// the forward's compositing of the depth column (ray_weights, the same accumulation order), with the normal and weight sums beside it
template <int SPL>
__global__ __launch_bounds__(256) void k_normal_composite(CompositeArgs a, NormalArgs q) {
    const int lane = threadIdx.x & 63, ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const int off = a.offsets[ray], n = a.counts[ray];
    const RayWeights<SPL> rw = ray_weights<SPL>(a.sigma, a.delta, off, n, lane);
    float depth = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, acc = 0.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        if (i < n) {
            const size_t p = (size_t)off + i;
            const float w = rw.w[k];
            depth += w * a.tmid[p];
            const float gx = q.grad[p], gy = q.grad[(size_t)a.p_pad + p], gz = q.grad[2 * (size_t)a.p_pad + p];
            if (q.s_grad) {
                q.s_sigma[p] = a.sigma[p];
                q.s_grad[3 * p] = gx; q.s_grad[3 * p + 1] = gy; q.s_grad[3 * p + 2] = gz;
            }
            const float sx = gx * q.ax, sy = gy * q.ay, sz = gz * q.az;
            const float len = sqrtf(sx * sx + sy * sy + sz * sz);
            const bool ok = len > 0.f && len <= 3.402823466e38f;      // (NaN fails both)
            const float ux = ok ? sx / len : 0.f, uy = ok ? sy / len : 0.f, uz = ok ? sz / len : 0.f;
            nx += w * ux; ny += w * uy; nz += w * uz; acc += w;
        }
    }
    depth = wave_sum(depth); nx = wave_sum(nx); ny = wave_sum(ny); nz = wave_sum(nz); acc = wave_sum(acc);
    if (lane == 0) {
        float* o = q.out + (size_t)ray * 5;
        o[0] = depth; o[1] = 0.f - nx; o[2] = 0.f - ny; o[3] = 0.f - nz; o[4] = acc;
    }
}

hipError_t launch_composite(const CompositeArgs& a, const NormalArgs& q, hipStream_t st) {
    const dim3 blocks((a.n_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK);
    eo_dispatch_spl(a.n_samples, [&](auto spl) { hipLaunchKernelGGL((k_normal_composite<decltype(spl)::value>), blocks, dim3(256), 0, st, a, q); });
    return hipGetLastError();
}

// layouts: the pass' own (carve_field; carve_quantile's dense layout, i.e. the ONLY_DEPTH forward's followed by the sampler's flattened
// outputs) followed by the gradient planes (eonerf_normals_check.h)
struct PointsWs { PassBuffers b; int p_cap; float* grad; size_t bytes; };
PointsWs carve_points(const eonerf_ctx* ctx, void* base, int n) {
    PointsWs w;
    w.p_cap = field_p_cap_of(n);
    const FieldWs f = carve_field(carve_cfg(ctx), base, w.p_cap);
    const NormalsExt e = normals_ext(f.bytes, (uint64_t)w.p_cap);
    w.b = f.b;
    w.grad = base ? reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(base) + e.grad_off) : nullptr;
    w.bytes = e.bytes;
    return w;
}
struct NormalsWs { QuantileWs q; float* grad; size_t bytes; };
NormalsWs carve_normals(const eonerf_ctx* ctx, void* base, int n_rays) {
    NormalsWs w;
    w.q = carve_quantile(carve_cfg(ctx), base, n_rays, 0);
    const NormalsExt e = normals_ext(w.q.bytes, (uint64_t)w.q.p_cap);
    w.grad = base ? reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(base) + e.grad_off) : nullptr;
    w.bytes = e.bytes;
    return w;
}

}  // namespace

extern "C" {

int eonerf_normals_version(void) { return EONERF_NORMALS_VERSION; }

size_t eonerf_density_grad_workspace_bytes(const eonerf_ctx* ctx, int n_points) {
    if (!ctx || n_points < 0 || !normals_p_cap(n_points, 1)) return 0;
    return carve_points(ctx, nullptr, n_points).bytes;
}

int eonerf_field_density_grad(eonerf_ctx* ctx, const float* flat, const float* xyz, int n, float* sigma, float* grad,
                              void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    bool empty = false;
    const int rc0 = normals_points_refusal(ctx, flat, xyz, sigma, grad, ws, n, ctx ? ctx->weights_set : false, ctx ? ctx->prec : 0, &empty);
    if (rc0 || empty) return rc0;
    const PointsWs w = carve_points(ctx, ws, n);
    if (normals_check_workspace(ws_bytes, w.bytes)) return EONERF_E_WORKSPACE;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }
    drop_presample(ctx, ws);
    HIP_TRY(eo_launch_points_to_soa(xyz, nullptr, n, w.p_cap, w.b.px, w.b.py, w.b.pz, w.b.simg, w.b.n_pts, st));
    const int rc = run_sigma_jvp(ctx, w.b, flat, w.p_cap, w.grad, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sigma, w.b.sigma, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return (int)eo_launch_soa3_to_aos(w.grad, w.p_cap, n, grad, st);
}

size_t eonerf_normals_workspace_bytes(const eonerf_ctx* ctx, int n_rays) {
    if (!ctx || n_rays < 0 || !normals_rays_ok(n_rays, ctx->n_samples)) return 0;
    return carve_normals(ctx, nullptr, n_rays).bytes;
}

int eonerf_render_normals(eonerf_ctx* ctx, const float* flat, const float* rays, const float* zsteps, const float* u_cam,
                          const float* u_retry, int n_rays, const float* axis_scale, float* out, int* n_samples_dev,
                          int64_t* s_ray, float* s_ts, float* s_te, float* s_sigma, float* s_grad,
                          void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int n_s = (s_ray ? 1 : 0) + (s_ts ? 1 : 0) + (s_te ? 1 : 0) + (s_sigma ? 1 : 0) + (s_grad ? 1 : 0);
    bool empty = false;
    const int rc0 = normals_render_refusal(ctx, flat, rays, zsteps, out, ws, n_rays, ctx ? ctx->weights_set : false, n_s, axis_scale,
                                           ctx ? ctx->prec : 0, u_cam != nullptr, u_retry != nullptr, ctx ? ctx->n_samples : 0, &empty);
    if (rc0 || empty) return rc0;
    const NormalsWs w = carve_normals(ctx, ws, n_rays);
    if (normals_check_workspace(ws_bytes, w.bytes)) return EONERF_E_WORKSPACE;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }
    ctx->pre.valid = false; ctx->pose.valid = false;      // dropped: this call's kernels write the workspace the record described (or the caller moved on)

    // ---- the ONLY_DEPTH forward's sampler launch, as eonerf_render_depth_quantiles issues it ------------------------------------
    const bool philox = u_cam == nullptr;
    SampleArgs sa = camera_sample_args(ctx, w.q.r, rays, nullptr, zsteps, u_cam, u_retry, n_rays, n_samples_dev, true);
    if (philox) sa.call = ctx->noise_call++;
    sa.o_ray = n_s ? s_ray : w.q.o_ray; sa.o_ts = n_s ? s_ts : w.q.o_ts; sa.o_te = n_s ? s_te : w.q.o_te;
    HIP_TRY(eo_launch_sampler(sa, st));
    const int rc = run_sigma_jvp(ctx, w.q.r.cam, flat, w.q.p_cap, w.grad, st);
    if (rc) return rc;
    NormalArgs na;
    na.out = out; na.grad = w.grad;
    na.ax = axis_scale ? axis_scale[0] : 1.f; na.ay = axis_scale ? axis_scale[1] : 1.f; na.az = axis_scale ? axis_scale[2] : 1.f;
    na.s_sigma = s_sigma; na.s_grad = s_grad;
    return (int)launch_composite(composite_args(ctx, w.q.r, flat, rays, n_rays, w.q.p_cap, true), na, st);
}

}  // extern "C"
