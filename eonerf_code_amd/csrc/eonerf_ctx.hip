// Context, weights and status entry points of libeonerf_hip.so (include/eonerf_hip.h): create / destroy, the parameter layout, the packed
// weight streams and their re-pack kernels, the measurement hooks, the status words and the optimizer step.
#include <math.h>
#include <new>

#include "eonerf_ctx.h"

namespace {

int upload(DevStream& d, const PackedStream& s) {
    d.bytes = s.bytes; d.n_chunks = (int)s.chunks.size(); d.n16 = (int)s.e16.size(); d.n32 = (int)s.e32.size(); d.n16lo = (int)s.e16lo.size();
    HIP_TRY(hipMalloc(&d.data, s.bytes + 1024));      // + slack: the chain kernels copy whole 1-KiB pieces (WStream::round)
    HIP_TRY(hipMemset(d.data, 0, s.bytes + 1024));
    HIP_TRY(hipMalloc(&d.chunks, s.chunks.size() * sizeof(ChunkDesc)));
    HIP_TRY(hipMemcpy(d.chunks, s.chunks.data(), s.chunks.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice));
    if (d.n16) {
        HIP_TRY(hipMalloc(&d.e16, s.e16.size() * sizeof(PackEntry)));
        HIP_TRY(hipMemcpy(d.e16, s.e16.data(), s.e16.size() * sizeof(PackEntry), hipMemcpyHostToDevice));
    }
    if (d.n32) {
        HIP_TRY(hipMalloc(&d.e32, s.e32.size() * sizeof(PackEntry)));
        HIP_TRY(hipMemcpy(d.e32, s.e32.data(), s.e32.size() * sizeof(PackEntry), hipMemcpyHostToDevice));
    }
    if (d.n16lo) {
        HIP_TRY(hipMalloc(&d.e16lo, s.e16lo.size() * sizeof(PackEntry)));
        HIP_TRY(hipMemcpy(d.e16lo, s.e16lo.data(), s.e16lo.size() * sizeof(PackEntry), hipMemcpyHostToDevice));
    }
    return 0;
}
void release(DevStream& d) {
    if (d.data) (void)hipFree(d.data);
    if (d.chunks) (void)hipFree(d.chunks);
    if (d.e16) (void)hipFree(d.e16);
    if (d.e32) (void)hipFree(d.e32);
    if (d.e16lo) (void)hipFree(d.e16lo);
    d = DevStream();
}

// (re)packs the fp32 master weights into up to PACK_MAX_JOBS packed streams in ONE launch (blockIdx.y = job): after every
// optimizer step three streams x {bf16, fp32} entries are rewritten, and six ~5 us launches cost more than the copies
constexpr int PACK_MAX_JOBS = 16;
struct PackJob { const PackEntry* e; int n; uint8_t* data; int kind; };      // kind: 0 fp32, 1 bf16, 2 fp16 (hi half of a split value), 3 its lo half
struct PackJobs { PackJob j[PACK_MAX_JOBS]; };
// sources >= fold_base come from the fold buffer (ParamLayout::fold_w / fold_b)
__global__ void k_pack(const float* flat, const float* fold, int fold_base, PackJobs jobs, int* range_flag) {
    const PackJob jb = jobs.j[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < jb.n; i += gridDim.x * blockDim.x) {
        const PackEntry pe = jb.e[i];
        const float v = pe.src < 0 ? 0.f : (pe.src >= fold_base ? fold[pe.src - fold_base] : flat[pe.src]);
        if (jb.kind == 1) *reinterpret_cast<__bf16*>(jb.data + pe.dst) = (__bf16)v;
        else if (jb.kind == 0) *reinterpret_cast<float*>(jb.data + pe.dst) = v;
        else {
            const _Float16 hi = (_Float16)v;
            *reinterpret_cast<_Float16*>(jb.data + pe.dst) = jb.kind == 2 ? hi : (_Float16)(v - (float)hi);
            if (jb.kind == 2 && !(fabsf(v) <= 65504.f)) atomicOr(range_flag + (RANGE_STICKY_WORD - RANGE_WORD), 1);      // a weight (or folded weight) outside fp16's range, or not finite
        }
    }
}

// The heads' first layers folded with the bottleneck layer (eonerf_pack.h): fold[o][i] = sum_k W_AT[o][k] W_b[k][i], b_f[o] = sum_k
// W_AT[o][k] b_b[k] + b_AT[o], with W_AT = [W_A1; W_T1[:, :256]].  fp32 FMAs in a fixed order (four interleaved partial sums over k:
// deterministic).  Block = 2 output rows, thread = column i: 16.8 M MACs on 128 workgroups in front of every re-pack; the k loop is
// unrolled so that 64 loads of a W_b column are in flight (a batch of 16 was still a chain of L2 round trips: 14 us).
struct FoldArgs { const float *w_a1, *b_a1, *w_t1, *b_t1, *w_b, *b_b; float* fold; float* wbt; };
__global__ __launch_bounds__(256) void k_fold(FoldArgs a) {
    __shared__ float wat[2][256];
    const int o0 = blockIdx.x * 2, i = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int o = o0 + r;
        wat[r][i] = o < 128 ? a.w_a1[(size_t)o * 256 + i] : a.w_t1[(size_t)(o - 128) * 260 + i];
    }
    __syncthreads();
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll 16
    for (int k = 0; k < 256; k += 4) {
        float wb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) wb[u] = a.w_b[(size_t)(k + u) * 256 + i];
#pragma unroll
        for (int u = 0; u < 4; ++u) { acc[0][u] = fmaf(wat[0][k + u], wb[u], acc[0][u]); acc[1][u] = fmaf(wat[1][k + u], wb[u], acc[1][u]); }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) a.fold[(size_t)(o0 + r) * 256 + i] = (acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3]);
    // by-product for the backward's tail kernel (bott_wgrad_body): W_bott transposed, two of its rows per block
#pragma unroll
    for (int r = 0; r < 2; ++r) a.wbt[(size_t)i * 256 + o0 + r] = a.w_b[(size_t)(o0 + r) * 256 + i];
    if (i < 2) {
        const int o = o0 + i;
        float b4[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 256; ++k) b4[k & 3] = fmaf(wat[i][k], a.b_b[k], b4[k & 3]);
        a.fold[256 * 256 + o] = ((b4[0] + b4[1]) + (b4[2] + b4[3])) + (o < 128 ? a.b_a1[o] : a.b_t1[o - 128]);
    }
}
// fp16 x 3 contexts, at every re-pack: the weight matrices the split streams are made of must lie where hi + lo fp16 carries them to
// fp32-level accuracy (include/eonerf_hip.h, eonerf_range_status).  One block per matrix: max |w| over the matrix
//   > F16X3_W_MAX (or not finite): an absolute operand error of 2^-25 per activation is amplified beyond what "fp32-level" means
//   < F16X3_W_MIN: the lo halves are fp16 subnormals for the whole matrix, the weights keep < 16 bits relative to the largest one
// -> the range flag is raised and the Python layer renders on an fp32 context instead.
constexpr float F16X3_W_MAX = 64.f, F16X3_W_MIN = 1.f / 512.f;
struct RangeJob { const float* w; int n; int check_min; };
struct RangeJobs { RangeJob j[24]; };
__global__ __launch_bounds__(256) void k_weight_range(RangeJobs jobs, int* range_flag) {
    __shared__ float red[256];
    __shared__ int bad[1];
    const RangeJob jb = jobs.j[blockIdx.x];
    if (threadIdx.x == 0) bad[0] = 0;
    __syncthreads();
    float m = 0.f;
    for (int i = threadIdx.x; i < jb.n; i += 256) {
        const float v = fabsf(jb.w[i]);
        if (!(v <= 3.0e38f)) bad[0] = 1;      // inf / NaN
        else m = fmaxf(m, v);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) {
        const float mx = red[0];
        const float hi_lim = jb.check_min ? F16X3_W_MAX : 65504.f;       // (operands that are not weights -- the embedding rows -- only have to fit)
        if (bad[0] || mx > hi_lim || (jb.check_min && mx > 0.f && mx < F16X3_W_MIN)) atomicOr(range_flag + (RANGE_STICKY_WORD - RANGE_WORD), 1);
    }
}
int weight_range(const eonerf_ctx* ctx, const float* flat, hipStream_t st) {
    const ParamLayout& pl = ctx->pl;
    RangeJobs jobs;
    int n = 0;
    auto add = [&](int ti, int check_min) { jobs.j[n++] = RangeJob{flat + pl.t[ti].offset, pl.t[ti].rows * pl.t[ti].cols, check_min}; };
    for (int l = 0; l < 8; ++l) add(pl.trunk_w[l], 1);
    add(pl.sig_w, 1); add(pl.a2_w, 1);
    for (int l = 1; l < 4; ++l) add(pl.t_w[l], 1);
    add(pl.tsc_w, 1); add(pl.tbe_w, 1);
    add(pl.t_w[0], 0);      // its embedding columns are packed as they are; its bottleneck columns enter through the fold
    add(pl.emb, 0);
    jobs.j[n++] = RangeJob{ctx->fold, 256 * 256, 1};      // [W_A1; W_T1'] W_bott, what the streams hold of the three folded layers
    hipLaunchKernelGGL(k_weight_range, dim3(n), dim3(256), 0, st, jobs, ctx->dev_status + RANGE_WORD);
    return (int)hipGetLastError();
}

int fold_heads(const eonerf_ctx* ctx, const float* flat, hipStream_t st) {
    const ParamLayout& pl = ctx->pl;
    FoldArgs a{flat + pl.t[pl.a1_w].offset, flat + pl.t[pl.a1_b].offset, flat + pl.t[pl.t_w[0]].offset, flat + pl.t[pl.t_b[0]].offset,
               flat + pl.t[pl.bot_w].offset, flat + pl.t[pl.bot_b].offset, ctx->fold, ctx->fold + FOLD_FLOATS};
    hipLaunchKernelGGL(k_fold, dim3(128), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

// Measurement hook (eonerf_clock_probe): a FIXED amount of dense bf16 MFMA work on every CU -- 4 waves per workgroup (one per SIMD), each
// CLOCK_PROBE_MFMAS v_mfma_f32_32x32x16_bf16 on four independent accumulators -- bracketed, in workgroup 0, by the shader-clock counter
// (s_memtime) and the constant 100-MHz counter (s_memrealtime).  cycles / ticks x 100 = the shader clock in MHz the chip held over the
// probe; the probe's duration (ticks x 10 ns) is the same statement without trusting s_memtime: fixed work, time ~ 1 / clock.
constexpr int CLOCK_PROBE_MFMAS = 8192;
typedef __attribute__((ext_vector_type(8))) __bf16 probe_bf16x8;
typedef __attribute__((ext_vector_type(16))) float probe_f32x16;
__global__ __launch_bounds__(256) void k_clock_probe(float* out) {
    probe_bf16x8 a, b;
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = (__bf16)(0.001f * (float)(threadIdx.x + e)); b[e] = (__bf16)(0.002f * (float)(threadIdx.x ^ e)); }
    probe_f32x16 c0 = {}, c1 = {}, c2 = {}, c3 = {};
    const unsigned long long t0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < CLOCK_PROBE_MFMAS / 4; ++i) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c3, 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) s += (c0[e] + c1[e]) + (c2[e] + c3[e]);
    const unsigned long long t1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float cyc = (float)(t1 - t0), ticks = (float)(r1 - r0);
        out[0] = cyc; out[1] = ticks; out[2] = ticks > 0.f ? cyc / ticks * 100.f : 0.f;
        out[3] = s == 12345.678f ? 1.f : 0.f;      // keeps the accumulators live
    }
}

}  // namespace

// (a stream set that needs more than PACK_MAX_JOBS jobs goes out in several launches: today's largest set is 9 streams, 13 jobs)
int eo_pack(const eonerf_ctx* ctx, const std::vector<const DevStream*>& streams, const float* flat, hipStream_t st) {
    PackJobs jobs;
    int n = 0, most = 1;
    auto flush = [&]() {
        if (n) hipLaunchKernelGGL(k_pack, dim3(std::min((most + 255) / 256, 1024), n), dim3(256), 0, st, flat, ctx->fold, (int)ctx->pl.total, jobs, ctx->dev_status + RANGE_WORD);
        n = 0; most = 1;
    };
    for (const DevStream* d : streams) {
        if (n + 3 > PACK_MAX_JOBS) flush();
        if (d->n16) jobs.j[n++] = PackJob{d->e16, d->n16, d->data, d->n16lo ? 2 : 1};
        if (d->n16lo) jobs.j[n++] = PackJob{d->e16lo, d->n16lo, d->data, 3};
        if (d->n32) jobs.j[n++] = PackJob{d->e32, d->n32, d->data, 0};
        most = std::max(most, std::max(d->n16, d->n32));
    }
    flush();
    return (int)hipGetLastError();
}

int eo_ensure_density_streams(eonerf_ctx* ctx, const float* flat, hipStream_t st) {
    ctx->dens_used = true;
    if (!ctx->dens_dirty) return 0;
    const int rc = ctx->prec == EONERF_F16X3 ? eo_pack(ctx, {&ctx->fwd_dens}, flat, st)
                 : ctx->pipe ? eo_pack(ctx, {&ctx->fwd_dens, &ctx->bwd_dens, &ctx->bwd_dens_heads, &ctx->ig_tail_wt}, flat, st)
                             : eo_pack(ctx, {&ctx->fwd_dens, &ctx->bwd_dens}, flat, st);
    if (!rc) ctx->dens_dirty = false;
    return rc;
}

extern "C" {

int eonerf_version(void) { return EONERF_VERSION; }

const char* eonerf_strerror(int code) {
    switch (code) {
        case EONERF_OK: return "ok";
        case EONERF_E_ARG: return "eonerf: invalid argument";
        case EONERF_E_WORKSPACE: return "eonerf: workspace too small";
        case EONERF_E_STATE: return "eonerf: call sequence error (set_weights / train forward missing, or a ray buffer refilled between eonerf_presample and its forward)";
        case EONERF_E_UNSUPPORTED: return "eonerf: unsupported configuration";
        case EONERF_E_RANGE: return "eonerf: a weight, an activation or a position left fp16's range (|v| > 65504 or not finite) in an fp16 x 3 call since the last check; its outputs are invalid -- render in fp32";
        case EONERF_E_DEVICE: return "eonerf: a device-side hand-off timed out (pipelined backward watchdog) on this or another rank; the gradients of that step are invalid and every optimizer update since has been skipped";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "eonerf: unknown error";
    }
}

int eonerf_create(eonerf_ctx** out, const eonerf_config* cfg) {
    if (!out || !cfg || cfg->n_images < 1) return EONERF_E_ARG;
    if (cfg->n_samples < 2 || cfg->n_samples > 256) return EONERF_E_UNSUPPORTED;      // (a ray's samples live in the 64 lanes x 4 slots of one wavefront)
    if (cfg->precision != EONERF_FP32 && cfg->precision != EONERF_BF16 && cfg->precision != EONERF_F16X3) return EONERF_E_ARG;
    eonerf_ctx* ctx = new (std::nothrow) eonerf_ctx();
    if (!ctx) return EONERF_E_ARG;
    ctx->cfg = *cfg;
    ctx->n_samples = cfg->n_samples;
    ctx->prec = cfg->precision;
    ctx->bf16 = cfg->precision == EONERF_BF16;
    const bool infer_only = cfg->precision == EONERF_F16X3;      // forward streams only
    { const char* e = getenv("EONERF_DETERMINISTIC"); ctx->deterministic = e && atoi(e) != 0; }
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { delete ctx; return (int)hipErrorNoDevice; }
    ctx->n_cu = prop.multiProcessorCount;
    { const char* e = getenv("EONERF_WGRAD_RIDERS"); if (e) ctx->wgrad_riders = atoi(e); }
    { const char* e = getenv("EONERF_STAGGER"); if (e) ctx->stagger = atoi(e); }
    { const char* e = getenv("EONERF_PIPE_XCD"); if (e) ctx->pipe_xcd = atoi(e); }
    { const char* e = getenv("EONERF_ENC_PAIR"); if (e) ctx->enc_pair = atoi(e); }
    ctx->pl.build(cfg->n_images);
    int rc = upload(ctx->fwd_full, build_fwd_stream(ctx->pl, ctx->prec, true));
    if (!rc) rc = upload(ctx->fwd_dens, build_fwd_stream(ctx->pl, ctx->prec, false));
    if (!rc && !infer_only) rc = upload(ctx->bwd_full, build_bwd_stream(ctx->pl, ctx->bf16, true, false));
    if (!rc && !infer_only) rc = upload(ctx->bwd_dens, build_bwd_stream(ctx->pl, ctx->bf16, false, true));
    if (!rc && !infer_only) rc = upload(ctx->bwd_rgb, build_bwd_stream(ctx->pl, ctx->bf16, true, false, false));
    if (!rc && !infer_only) rc = upload(ctx->bwd_full_ig, build_bwd_stream(ctx->pl, ctx->bf16, true, true, true));
    {
        const char* e = getenv("EONERF_PIPE");
        ctx->n_pipes = ctx->n_cu / PIPE_STAGES;
        ctx->pipe = ctx->bf16 && ctx->n_pipes >= 1 && !(e && atoi(e) == 0);
        // Residency: the pipelined launch needs its 7 x n_pipes workgroups on the chip AT THE SAME TIME (one per CU: 128 KB of LDS, the
        // whole register file).  Where that cannot hold by construction -- the kernel does not fit a CU of this device, or the process
        // was given a CU mask (HSA_CU_MASK / ROC_GLOBAL_CU_MASK: the runtime still reports every CU) -- the chain + GEMM path is used
        // from the start instead of timing out in the first step.  A co-tenant on the card cannot be seen from here: see eonerf_device_status.
        if (ctx->pipe && !(e && atoi(e) == 1)) {
            if (!eo_bwd_pipe_fits_a_cu() || getenv("HSA_CU_MASK") || getenv("ROC_GLOBAL_CU_MASK")) ctx->pipe = false;
        }
        { const char* fb = getenv("EONERF_PIPE_FALLBACK"); ctx->pipe_fallback = !(fb && atoi(fb) == 0); }
        if (!rc && ctx->pipe) rc = upload(ctx->pipe_wt, build_pipe_stream(ctx->pl));
        if (!rc && ctx->pipe) rc = upload(ctx->bwd_full_heads, build_bwd_stream(ctx->pl, true, true, false, true, 1));
        if (!rc && ctx->pipe) rc = upload(ctx->bwd_rgb_heads, build_bwd_stream(ctx->pl, true, true, false, false, 1));
        if (!rc && ctx->pipe) rc = upload(ctx->bwd_dens_heads, build_bwd_stream(ctx->pl, true, false, true, false, 1));
        if (!rc && ctx->pipe) rc = upload(ctx->ig_tail_wt, build_ig_tail_stream(ctx->pl));
        { const char* f = getenv("EONERF_PIPE_FAULT"); ctx->pipe_fault_stage = f ? atoi(f) : -1; }
        { const char* f = getenv("EONERF_PIPE_STAMPS");
          if (!rc && ctx->pipe && f && atoi(f)) rc = (int)hipMalloc(&ctx->pipe_stamps, (size_t)ctx->n_pipes * PIPE_STAGES * 128 * sizeof(unsigned long long)); }
    }
    if (!rc) rc = (int)hipMalloc(&ctx->fold, (FOLD_FLOATS + 256 * 256) * sizeof(float));      // + W_bott transposed (k_fold)
    if (!rc) rc = (int)hipMalloc(&ctx->loss_scratch, (LOSS_MAX_BLOCKS + 4) * sizeof(float));
    if (!rc) rc = (int)hipMemset(ctx->loss_scratch, 0, (LOSS_MAX_BLOCKS + 4) * sizeof(float));
    if (!rc) rc = (int)hipMalloc(&ctx->dev_status, 64 * sizeof(int));
    if (!rc) rc = (int)hipMemset(ctx->dev_status, 0, 64 * sizeof(int));
    if (!rc) {
        int cm[64];
        for (int s = 0; s < 64; ++s) cm[s] = enc_col_of_slot(ctx->bf16, s);
        rc = (int)hipMalloc(&ctx->enc_colmap, sizeof(cm));
        if (!rc) rc = (int)hipMemcpy(ctx->enc_colmap, cm, sizeof(cm), hipMemcpyHostToDevice);
    }
    if (rc) { eonerf_destroy(ctx); return rc; }
    *out = ctx;
    return EONERF_OK;
}

int eonerf_profile_enable(eonerf_ctx* ctx, int max_launches) {
    if (!ctx || max_launches < 0) return EONERF_E_ARG;
    for (int k = 0; k < EONERF_PROF_KERNELS; ++k) {
        for (int s = 0; s < 2; ++s) {
            for (hipEvent_t e : ctx->prof_ev[k][s]) (void)hipEventDestroy(e);
            ctx->prof_ev[k][s].clear();
            for (int i = 0; i < max_launches; ++i) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); ctx->prof_ev[k][s].push_back(e); }
        }
        ctx->prof_n[k] = 0;
    }
    ctx->prof_cap = max_launches;
    return EONERF_OK;
}

int eonerf_clock_probe(eonerf_ctx* ctx, float* out4, void* stream) {
    if (!ctx || !out4) return EONERF_E_ARG;
    hipLaunchKernelGGL(k_clock_probe, dim3(ctx->n_cu), dim3(256), 0, (hipStream_t)stream, out4);
    return (int)hipGetLastError();
}

const char* eonerf_profile_name(int kernel) {
    static const char* const names[EONERF_PROF_KERNELS] = {"fwd_chain_camera", "bwd_chain_camera", "wgrad_gemm", "fwd_chain_sun", "bwd_chain_sun",
                                                           "bwd_pipe_camera", "bwd_pipe_sun", "ig_tail_sun"};
    return kernel >= 0 && kernel < EONERF_PROF_KERNELS ? names[kernel] : nullptr;
}

int eonerf_profile_read(eonerf_ctx* ctx, int kernel, float* total_ms, int* launches) {
    if (!ctx || kernel < 0 || kernel >= EONERF_PROF_KERNELS || !total_ms || !launches) return EONERF_E_ARG;
    float sum = 0.f;
    for (int i = 0; i < ctx->prof_n[kernel]; ++i) {
        HIP_TRY(hipEventSynchronize(ctx->prof_ev[kernel][1][i]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->prof_ev[kernel][0][i], ctx->prof_ev[kernel][1][i]));
        sum += ms;
    }
    *total_ms = sum; *launches = ctx->prof_n[kernel];
    return EONERF_OK;
}

int eonerf_destroy(eonerf_ctx* ctx) {
    if (!ctx) return EONERF_E_ARG;
    for (int k = 0; k < EONERF_PROF_KERNELS; ++k) for (int s = 0; s < 2; ++s) for (hipEvent_t e : ctx->prof_ev[k][s]) (void)hipEventDestroy(e);
    release(ctx->fwd_full); release(ctx->fwd_dens); release(ctx->bwd_full); release(ctx->bwd_dens); release(ctx->bwd_rgb); release(ctx->bwd_full_ig); release(ctx->pipe_wt); release(ctx->bwd_full_heads); release(ctx->bwd_rgb_heads); release(ctx->bwd_dens_heads); release(ctx->ig_tail_wt);
    if (ctx->fold) (void)hipFree(ctx->fold);
    if (ctx->loss_scratch) (void)hipFree(ctx->loss_scratch);
    if (ctx->enc_colmap) (void)hipFree(ctx->enc_colmap);
    if (ctx->pipe_stamps) (void)hipFree(ctx->pipe_stamps);
    if (ctx->dev_status) (void)hipFree(ctx->dev_status);
    delete ctx;
    return EONERF_OK;
}

int eonerf_param_tensors(const eonerf_ctx* ctx) { return ctx ? (int)ctx->pl.t.size() : 0; }
size_t eonerf_param_floats(const eonerf_ctx* ctx) { return ctx ? ctx->pl.total : 0; }
int eonerf_param_info(const eonerf_ctx* ctx, int index, const char** name, size_t* offset, int* rows, int* cols) {
    if (!ctx || index < 0 || index >= (int)ctx->pl.t.size()) return EONERF_E_ARG;
    const ParamInfo& p = ctx->pl.t[index];
    if (name) *name = p.name.c_str();
    if (offset) *offset = p.offset;
    if (rows) *rows = p.rows;
    if (cols) *cols = p.cols;
    return EONERF_OK;
}

int eonerf_set_weights(eonerf_ctx* ctx, const float* flat, void* stream) {
    if (!ctx || !flat) return EONERF_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    ctx->pose.valid = false;
    // pipelined backward: the camera pass reads the heads-only streams + the stage-stationary trunk weights; the density-only streams
    // ride along when something has read them since the last re-pack (shadow pass on: they would be re-packed a few kernels later anyway)
    std::vector<const DevStream*> v;
    v.push_back(&ctx->fwd_full);
    if (ctx->prec == EONERF_F16X3) {}      // forward streams only
    else if (ctx->pipe) { v.push_back(&ctx->bwd_full_heads); v.push_back(&ctx->bwd_rgb_heads); }
    else { v.push_back(&ctx->bwd_full); v.push_back(&ctx->bwd_rgb); }
    if (ctx->pipe) v.push_back(&ctx->pipe_wt);
    const bool with_dens = ctx->dens_used;
    if (with_dens) {      // the same set ensure_density_streams packs
        v.push_back(&ctx->fwd_dens);
        if (ctx->prec != EONERF_F16X3) v.push_back(&ctx->bwd_dens);
        if (ctx->pipe) { v.push_back(&ctx->bwd_dens_heads); v.push_back(&ctx->ig_tail_wt); }
    }
    ctx->need_repack = false;
    int rc = fold_heads(ctx, flat, st);      // the folded head weights are a gather source of the streams below
    if (!rc && ctx->prec == EONERF_F16X3) {      // the weight criteria describe THESE weights until the next re-pack (eonerf_range_status does not clear them)
        rc = (int)hipMemsetAsync(ctx->dev_status + RANGE_STICKY_WORD, 0, sizeof(int), st);
        if (!rc) rc = weight_range(ctx, flat, st);
    }
    if (!rc) rc = eo_pack(ctx, v, flat, st);
    if (!rc) { ctx->weights_set = true; ctx->dens_dirty = !with_dens; ctx->full_ig_dirty = true; ctx->dens_used = false; }
    return rc;
}

// diagnostics: copies the cycle sums of the last pipelined backward ([n_pipes * 7 roles][2 waves][8] u64) to the host; returns the
// number of u64 written (0 when EONERF_PIPE_STAMPS is off)
int eonerf_debug_pipe_stamps(eonerf_ctx* ctx, unsigned long long* host_out, int capacity) {
    if (!ctx || !ctx->pipe_stamps || !host_out) return 0;
    const int n = ctx->n_pipes * PIPE_STAGES * 128;
    if (capacity < n) return 0;
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    if (hipMemcpy(host_out, ctx->pipe_stamps, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

int eonerf_device_status(eonerf_ctx* ctx, void* stream) {
    if (!ctx) return EONERF_E_ARG;
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, ctx->dev_status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (!err) return EONERF_OK;
    HIP_TRY(hipMemsetAsync(ctx->dev_status, 0, sizeof(int), (hipStream_t)stream));
    // only the presample guard: a training forward consumed samples eonerf_presample had drawn for OTHER ray contents (the caller refilled
    // the buffer in place); k_adam skipped that step's update like any flagged step.  A call-sequence error, not a device fault: the
    // pipelined path stays
    if ((err & ~0x100) == EO_STATUS_PRESAMPLE_STALE) return EONERF_E_STATE;      // (0x100: k_adam's echo of the sealed flag in the gradient message)
    // A hand-off timed out: the launch did not have the card's CUs to itself (a co-tenant, a partitioned or CU-masked GPU) or a stage
    // stalled.  The fault is reported (the caller decides: the launcher ends the job) and THIS context leaves the pipelined path: a
    // caller that carries on trains through the chain + GEMM backward instead of paying a 0.3-s timeout in every step.  Data-parallel
    // ranks all see the fault (flag in the gradient message) and all switch.  Backwards of forwards that ran BEFORE this call keep the
    // pipelined path (ws_pipe / PipeModeGuard: their workspace layout and mask slots are that path's).
    if (ctx->pipe && ctx->pipe_fallback) { ctx->pipe = false; ctx->need_repack = true; }
    return EONERF_E_DEVICE;
}

int eonerf_range_status(eonerf_ctx* ctx, void* stream) {
    if (!ctx) return EONERF_E_ARG;
    if (ctx->prec != EONERF_F16X3) return EONERF_OK;
    static_assert(RANGE_STICKY_WORD == RANGE_WORD + 1, "both words in one copy");
    int flag[2] = {0, 0};      // [0] operands of the calls since the last check, [1] the weights of the last re-pack (stays up until they change)
    HIP_TRY(hipMemcpyAsync(flag, ctx->dev_status + RANGE_WORD, 2 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (!flag[0] && !flag[1]) return EONERF_OK;
    if (flag[0]) HIP_TRY(hipMemsetAsync(ctx->dev_status + RANGE_WORD, 0, sizeof(int), (hipStream_t)stream));
    return EONERF_E_RANGE;
}

int eonerf_render_status(eonerf_ctx* ctx, int n_rays, int flags, void* ws, size_t ws_bytes, void* stream) {
    (void)n_rays; (void)flags; (void)ws; (void)ws_bytes;
    return eonerf_device_status(ctx, stream);
}

size_t eonerf_grad_floats(const eonerf_ctx* ctx) { return ctx ? ctx->pl.total + 4 : 0; }
size_t eonerf_grad_early_floats(const eonerf_ctx* ctx) { return ctx ? ctx->pl.early : 0; }

int eonerf_set_exchange_event(eonerf_ctx* ctx, void* hip_event, int reserve_cus) {
    if (!ctx || reserve_cus < 0 || reserve_cus > ctx->n_cu / 2) return EONERF_E_ARG;
    ctx->exch_event = (hipEvent_t)hip_event;
    ctx->exch_cus = hip_event ? reserve_cus : 0;
    return EONERF_OK;
}

int eonerf_grad_seal(eonerf_ctx* ctx, float* d_flat, void* stream) {
    if (!ctx || !d_flat) return EONERF_E_ARG;
    return (int)eo_launch_grad_seal(d_flat + ctx->pl.total, ctx->dev_status, (hipStream_t)stream);
}

int eonerf_train_loss(eonerf_ctx* ctx, const float* out, const float* pixels, int n_rays, int kind, float* d_out, float* loss, void* stream) {
    if (!ctx || !out || !pixels || !d_out || !loss || n_rays < 1 || (kind != 0 && kind != 1)) return EONERF_E_ARG;
    return (int)eo_launch_loss(out, pixels, n_rays, kind, d_out, loss, ctx->loss_scratch, (hipStream_t)stream);
}

static int adam_common(eonerf_ctx* ctx, float* flat, float* d_flat, bool zero_grad, float* exp_avg, float* exp_avg_sq,
                       int step, float lr, float beta1, float beta2, float eps, float grad_scale, const float* fault_flag, void* stream) {
    if (!ctx || !flat || !d_flat || !exp_avg || !exp_avg_sq || step < 1) return EONERF_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(eo_launch_adam(flat, d_flat, zero_grad, exp_avg, exp_avg_sq, ctx->pl.total, step, lr, beta1, beta2, eps, grad_scale, ctx->dev_status, fault_flag, st));
    return eonerf_set_weights(ctx, flat, stream);
}
int eonerf_adam_step(eonerf_ctx* ctx, float* flat, const float* d_flat, float* exp_avg, float* exp_avg_sq,
                     int step, float lr, float beta1, float beta2, float eps, float grad_scale, const float* fault_flag, void* stream) {
    return adam_common(ctx, flat, const_cast<float*>(d_flat), false, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, grad_scale, fault_flag, stream);
}
int eonerf_adam_step_zero_grad(eonerf_ctx* ctx, float* flat, float* d_flat, float* exp_avg, float* exp_avg_sq,
                               int step, float lr, float beta1, float beta2, float eps, float grad_scale, const float* fault_flag, void* stream) {
    return adam_common(ctx, flat, d_flat, true, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, grad_scale, fault_flag, stream);
}

}  // extern "C"
