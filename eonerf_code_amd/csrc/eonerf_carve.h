// Workspace carving of the C ABI (eonerf_render_workspace_bytes / eonerf_render_forward / _backward; eonerf_field_*): plain host code,
// no HIP runtime calls -- shared by the entry points (eonerf_field.hip, eonerf_render.hip) and the host-only sanitizer test (tests/host/host_checks.cpp, built for the CPU
// under the address + undefined-behaviour sanitizers).  The caller (PyTorch) owns the workspace; these functions only lay it out.
#pragma once
#include <stdint.h>
#include <limits.h>
#include <string.h>
#include <algorithm>
#include "../../include/eonerf_hip.h"
#include "eonerf_kernels.h"
#include "eonerf_rays.h"

constexpr int BOTT_SCRATCH_F = 2 * 128 * 256 + 256;       // bottleneck factors M_a | M_t, then db_A1 | db_T1

struct CarveCfg {          // what the layout depends on besides (n_rays, flags): see eonerf_ctx
    bool bf16 = true, pipe = false, deterministic = false, pipe_partials = false;
    int n_pipes = 0;
    int enc_part_wgs = 0;  // > 0: workgroups of eonerf_enc_pair.hip, each with a partial of the shadow pass' encoding products (0: ig_tail + GEMM jobs)
    int n_samples = 128;   // int(2 / render_step_size) of the calls this layout serves (eonerf_set_n_samples)
};

// bump allocator over the caller's workspace (256-byte aligned); with base == nullptr it only measures
struct Carver {
    uint8_t* base; size_t off = 0;
    explicit Carver(void* b) : base(reinterpret_cast<uint8_t*>(b)) {}
    template <class T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

struct PassBuffers {       // one MLP pass (camera or sun) over up to p_cap samples
    int *counts, *offsets, *n_pts;
    float *px, *py, *pz, *tmid, *delta, *sigma, *albedo, *ts, *tb;
    int* simg;
    void *act, *grd; uint32_t* masks;
    float *g_sigma, *g_albedo, *g_ts, *g_tb, *g_emb, *g_pos;
};

struct PipeWs {            // layer-pipelined backward (eonerf_bwd_pipe.hip)
    uint8_t* dy_in;        // dY_7 in unit order: p_cap x 512 B (heads chain -> trunk pipeline)
    uint8_t* rings;        // [pipelines][edges][PIPE_RING][16 KiB]
    uint32_t* sync;        // PIPE_LAUNCHES consecutive blocks, one per pipelined launch of a backward call (sun trunk, camera trunk):
                           // [32] role counter, [64..) one scratch line per workgroup, then the edge flags -- all zeroed by ONE memset
    size_t sync_bytes;     // of one block
};
constexpr int PIPE_LAUNCHES = 2;

struct DetWs {             // EONERF_DETERMINISTIC: partial sums instead of atomics
    float* pipe_part;      // [n_pipes * 7][256 * 256 + 256]
    float* wgrad_part;     // [WGRAD_MAX_JOBS * 48 items][256 * 256 + 256]
    float* rad_rays;       // [R][6]
    float* emb_rays;       // [R][4]
};

struct RenderWs {
    PipeWs pipe;
    DetWs det;
    int *cnt_first, *cnt_retry, *flags;
    float* ray_rec; float* g_ray; float* amb_save;
    float* m_bott;        // [2][128][256] fp32: dA1^T X8 and dT1^T X8 (the bottleneck factors), then [256] db_A1 | db_T1 of this call
    int* queue;           // work-item counter of the weight-gradient GEMM (behind them)
    float* enc_part;      // [enc_part_wgs][ENC_PART_F] partials of eonerf_enc_pair.hip (training with the shadow pass on the pipelined path), or nullptr
    PassBuffers cam, sun;
    size_t bytes;
};

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// capacity of the compact per-sample arrays of a pass: a ray has n_samples - 1 intervals at most (n_samples = int(2 / render_step_size))
inline int p_cap_of(int n_rays, int n_samples) { return round_up(std::max(n_rays, 1) * (n_samples - 1), 256); }
// a 256-row block of a training slab ([sample tile][256 rows][64 B]) is addressed through ONE buffer descriptor with 32-bit byte offsets
// (SlabWriter, the GEMM's and the pipeline's operand loads): p_cap / samples-per-tile x 16 KiB must stay below 4 GiB --
// 66,050 rays (8.39 M samples) per call in bf16 mode, 33,024 in fp32 mode.  Larger batches are chunked by the caller (render_image does)
inline bool slab_blocks_addressable(bool bf16, size_t p_cap) { return p_cap / (bf16 ? 32 : 16) * 256 * SEG_B < (1ull << 32); }

inline void carve_pass(Carver& c, PassBuffers& b, int n_rays, int p_cap, bool full, bool train, bool input_grad, int act_bytes) {
    b.counts = c.take<int>(n_rays);
    b.offsets = c.take<int>(n_rays + 1);
    b.n_pts = c.take<int>(4);
    b.px = c.take<float>(p_cap); b.py = c.take<float>(p_cap); b.pz = c.take<float>(p_cap);
    b.tmid = c.take<float>(p_cap); b.delta = c.take<float>(p_cap);
    b.simg = c.take<int>(p_cap);
    b.sigma = c.take<float>(p_cap);
    b.albedo = full ? c.take<float>(3 * (size_t)p_cap) : nullptr;
    b.ts = full ? c.take<float>(p_cap) : nullptr;
    b.tb = full ? c.take<float>(p_cap) : nullptr;
    b.act = b.grd = nullptr; b.masks = nullptr;
    b.g_sigma = b.g_albedo = b.g_ts = b.g_tb = b.g_emb = b.g_pos = nullptr;
    if (train) {
        b.act = c.take<uint8_t>((size_t)(full ? ACT_ROWS_FULL : ACT_ROWS_DENSITY) * p_cap * act_bytes);
        b.grd = c.take<uint8_t>((size_t)(full ? GRD_ROWS_FULL : GRD_ROWS_DENSITY) * p_cap * act_bytes);
        b.masks = c.take<uint32_t>((size_t)(full ? MASK_SLOTS_FULL : MASK_SLOTS_DENSITY) * p_cap * 8);
        b.g_sigma = c.take<float>(p_cap);
        if (full) {
            b.g_albedo = c.take<float>(3 * (size_t)p_cap);
            b.g_ts = c.take<float>(p_cap); b.g_tb = c.take<float>(p_cap);
            b.g_emb = c.take<float>(4 * (size_t)p_cap);
        }
        if (input_grad) b.g_pos = c.take<float>(3 * (size_t)p_cap);
    }
}

inline RenderWs carve_render(const CarveCfg& cfg, void* base, int n_rays, int flags) {
    const CarveCfg* ctx = &cfg;
    Carver c(base);
    RenderWs w;
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);
    const bool train = flags & EONERF_F_TRAIN, shadows = flags & EONERF_F_SHADOWS, od = flags & EONERF_F_ONLY_DEPTH;
    const int ab = ctx->bf16 ? 2 : 4;
    w.cnt_first = c.take<int>(n_rays); w.cnt_retry = c.take<int>(n_rays); w.flags = c.take<int>(4);
    w.ray_rec = c.take<float>((size_t)n_rays * RAY_REC);
    w.g_ray = train ? c.take<float>((size_t)n_rays * RAY_REC) : nullptr;
    w.amb_save = train ? c.take<float>((size_t)n_rays * 160) : nullptr;
    // [bottleneck factors | GEMM work queue] and, right behind them, the pipeline's sync block: everything the backward needs zeroed, so
    // that the first pipeline launch of a backward call clears all of it with ONE memset
    w.m_bott = train ? c.take<float>(BOTT_SCRATCH_F + 64) : nullptr;
    w.queue = w.m_bott ? reinterpret_cast<int*>(w.m_bott + BOTT_SCRATCH_F) : nullptr;      // (measuring pass: no arithmetic on a null base)
    memset(&w.pipe, 0, sizeof(w.pipe));
    if (train && ctx->pipe) {
        const size_t wgs = (size_t)ctx->n_pipes * PIPE_STAGES;
        const size_t edges = (size_t)ctx->n_pipes * (PIPE_STAGES - 1);
        w.pipe.sync_bytes = (64 + wgs * 32 + edges * 64) * sizeof(uint32_t);
        w.pipe.sync = c.take<uint32_t>(PIPE_LAUNCHES * w.pipe.sync_bytes / sizeof(uint32_t));
        w.pipe.dy_in = c.take<uint8_t>((size_t)p_cap * 512);
        w.pipe.rings = c.take<uint8_t>(edges * PIPE_RING * PIPE_UNIT_B);
    }
    memset(&w.det, 0, sizeof(w.det));
    if (train && ctx->pipe && ctx->pipe_partials)
        w.det.pipe_part = c.take<float>((size_t)ctx->n_pipes * PIPE_STAGES * WGRAD_PART_F);
    if (train && ctx->deterministic) {
        w.det.wgrad_part = c.take<float>((size_t)WGRAD_MAX_JOBS * 48 * WGRAD_PART_F);
        w.det.rad_rays = c.take<float>((size_t)n_rays * 6);
        w.det.emb_rays = c.take<float>((size_t)n_rays * 4);
    }
    w.enc_part = (train && shadows && !od && ctx->pipe && ctx->enc_part_wgs > 0) ? c.take<float>((size_t)ctx->enc_part_wgs * ENC_PART_F) : nullptr;
    // (a density-only training pass -- render_depth under autograd -- may end in the chain kernel's input-gradient variant: room for d position)
    carve_pass(c, w.cam, n_rays, p_cap, !od, train, train && od, ab);
    if (shadows && !od) carve_pass(c, w.sun, n_rays, p_cap, false, train, true, ab); else memset(&w.sun, 0, sizeof(w.sun));
    w.bytes = c.off + 256;
    return w;
}

// ---- eonerf_render_sun_sweep (include/eonerf_sweep.h): one camera pass, then a shadow pass per sun direction ----
// The bound of a sweep on its batch, in 64 bits: p_cap_of must not wrap, i.e. n_rays x (n_samples - 1) rounded up to 256 stays an int
inline bool sweep_rays_addressable(int n_rays, int n_samples) { return (long long)n_rays * (n_samples - 1) <= (long long)INT_MAX - 255; }

struct SweepWs { RenderWs r; float* table; size_t bytes; };
// carve_render(EONERF_F_SHADOWS) unchanged -- every launch of the forward sees the forward's layout -- followed by the sweep's own
// copy of the ray table ([n_rays][11]: columns 8..10 hold the current sun).  The layout does not depend on the number of suns
inline SweepWs carve_sweep(const CarveCfg& cfg, void* base, int n_rays) {
    SweepWs s;
    s.r = carve_render(cfg, base, n_rays, EONERF_F_SHADOWS);
    Carver c(base);
    c.off = s.r.bytes - 256;      // (where carve_render's own allocator stopped)
    s.table = c.take<float>((size_t)n_rays * 11);
    s.bytes = c.off + 256;
    return s;
}

// ---- eonerf_render_forward_march (include/eonerf_march.h): a layout of its own.  Per-ray sampler results and march state, then the
//      buffers of ONE round of ONE pass -- n_rays x block sample slots, shared by the camera and the shadow pass ----
inline bool march_block_ok(int block) { return block == 16 || block == 32 || block == 64; }
inline int march_p_cap_of(int n_rays, int block) { return round_up(std::max(n_rays, 1) * block, 256); }
inline int march_rounds(int n_samples, int block) { return (n_samples - 1 + block - 1) / block; }
constexpr int MARCH_ACC = 8;      // per-ray sums carried between rounds: depth, albedo3, ts, tb, wsum (+ one spare float)
struct MarchWs {
    int *cnt_first, *cnt_retry, *last_first, *last_retry, *win_first, *win_retry, *flags;      // camera pass: full counts, last valid slot, window count per draw
    int *sun_cnt, *sun_last, *sun_win;                                                         // shadow pass (one draw)
    int *alive, *kept_cam, *kept_sun; float *od, *acc;                                         // march state; acc [R][MARCH_ACC]
    float* ray_rec;
    PassBuffers round; int p_cap;
    size_t bytes;
};
inline MarchWs carve_march(const CarveCfg& cfg, void* base, int n_rays, int flags, int block) {
    Carver c(base);
    MarchWs w;
    const bool od = flags & EONERF_F_ONLY_DEPTH;
    w.cnt_first = c.take<int>(n_rays); w.cnt_retry = c.take<int>(n_rays); w.last_first = c.take<int>(n_rays); w.last_retry = c.take<int>(n_rays);
    w.win_first = c.take<int>(n_rays); w.win_retry = c.take<int>(n_rays); w.flags = c.take<int>(4);
    w.sun_cnt = c.take<int>(n_rays); w.sun_last = c.take<int>(n_rays); w.sun_win = c.take<int>(n_rays);
    w.alive = c.take<int>(n_rays); w.kept_cam = c.take<int>(n_rays); w.kept_sun = c.take<int>(n_rays);
    w.od = c.take<float>(n_rays); w.acc = c.take<float>((size_t)n_rays * MARCH_ACC);
    w.ray_rec = c.take<float>((size_t)n_rays * RAY_REC);
    w.p_cap = march_p_cap_of(n_rays, block);
    carve_pass(c, w.round, n_rays, w.p_cap, !od, false, false, cfg.bf16 ? 2 : 4);
    w.bytes = c.off + 256;
    return w;
}
// The ONE decision whether a march call is refused on its own arguments, in the documented order (include/eonerf_march.h); `need` =
// carve_march(...).bytes, only looked at when the block size is a legal one
inline int march_refusal(int flags, float early_stop_eps, int block, size_t ws_bytes, size_t need) {
    if (flags & EONERF_F_TRAIN) return EONERF_E_UNSUPPORTED;
    if (!(early_stop_eps >= 0.0f && early_stop_eps < 1.0f)) return EONERF_E_ARG;      // (NaN fails both comparisons)
    if (!march_block_ok(block)) return EONERF_E_ARG;
    if (ws_bytes < need) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

// ---- eonerf_render_depth_quantiles (include/eonerf_quantile.h): the layout of the pass it runs -- dense (block == 0): carve_render's
//      ONLY_DEPTH layout unchanged, so that the sampler and chain launches see the forward's; march: carve_march's -- followed by the
//      sampler's flattened outputs (ray index, interval ends) of that pass' sample capacity ----
constexpr int QUANTILE_MAX = 8;
inline bool quantile_block_ok(int block) { return block == 0 || march_block_ok(block); }
struct QuantileWs { RenderWs r; MarchWs m; int64_t* o_ray; float *o_ts, *o_te; int p_cap; size_t bytes; };
inline QuantileWs carve_quantile(const CarveCfg& cfg, void* base, int n_rays, int block) {
    QuantileWs q;
    memset(&q, 0, sizeof(q));
    Carver c(base);
    if (block == 0) {
        q.r = carve_render(cfg, base, n_rays, EONERF_F_ONLY_DEPTH);
        q.p_cap = p_cap_of(n_rays, cfg.n_samples);
        c.off = q.r.bytes - 256;      // (where the pass' own allocator stopped)
    } else {
        q.m = carve_march(cfg, base, n_rays, EONERF_F_ONLY_DEPTH, block);
        q.p_cap = q.m.p_cap;
        c.off = q.m.bytes - 256;
    }
    q.o_ray = c.take<int64_t>(q.p_cap); q.o_ts = c.take<float>(q.p_cap); q.o_te = c.take<float>(q.p_cap);
    q.bytes = c.off + 256;
    return q;
}

// Everything a pipelined backward call needs zeroed, as ONE span: [bottleneck factors | GEMM work queue | the PIPE_LAUNCHES sync blocks].
// Cleared by the call's first kernel (ShadeBwdArgs::zero_base) or by the memset in front of its first pipelined launch
struct ZeroSpan { uint8_t* base; size_t bytes; };
inline ZeroSpan backward_zero_span(const RenderWs& w) {
    uint8_t* lo = reinterpret_cast<uint8_t*>(w.m_bott);
    uint8_t* hi = reinterpret_cast<uint8_t*>(w.pipe.sync) + PIPE_LAUNCHES * w.pipe.sync_bytes;
    return ZeroSpan{lo, (size_t)(hi - lo)};
}

// ---- EONerfMLP.forward / query_density on caller-provided points (eonerf_field_*): ONE pass over round_up(n, 256) samples ----
inline int field_p_cap_of(int n_points) { return round_up(std::max(n_points, 1), 256); }

struct FieldWs { PassBuffers b; size_t bytes; };
// inference (eonerf_field_forward, eonerf_query_density): the layout does not depend on which outputs the call asks for
inline FieldWs carve_field(const CarveCfg& cfg, void* base, int p_cap) {
    Carver c(base);
    FieldWs w;
    carve_pass(c, w.b, 1, p_cap, true, false, false, cfg.bf16 ? 2 : 4);
    w.bytes = c.off + 256;
    return w;
}

// ---- eonerf_occ_update (include/eonerf_occ.h): the field workspace of ONE chunk of cells (at most OCC_CHUNK, whatever r is) followed by
//      the reduction scratch: one fp64 partial per block of the fixed grid, then [mean (fp64), thr (fp32)] ----
constexpr int OCC_CHUNK = 1 << 18;
constexpr int OCC_SUM_BLOCKS = 256;
inline long long occ_cells(int r) { return (long long)r * r * r; }
inline int occ_chunk_cells(int r) { return (int)std::min<long long>(occ_cells(r), OCC_CHUNK); }
struct OccWs { PassBuffers b; int p_cap; double* partial; double* result; size_t bytes; };
inline OccWs carve_occ(const CarveCfg& cfg, void* base, int r) {
    OccWs w;
    w.p_cap = field_p_cap_of(occ_chunk_cells(r));
    const FieldWs f = carve_field(cfg, base, w.p_cap);
    w.b = f.b;
    Carver c(base);
    c.off = f.bytes - 256;      // (where carve_field's own allocator stopped)
    w.partial = c.take<double>(OCC_SUM_BLOCKS);
    w.result = c.take<double>(2);
    w.bytes = c.off + 256;
    return w;
}

struct FieldTrainWs { PassBuffers b; float* m_bott; int* queue; size_t bytes; };
// autograd pair (eonerf_field_forward_train / eonerf_field_backward): saved slabs, input gradient, the GEMM's bottleneck factors and queue
inline FieldTrainWs carve_field_train(const CarveCfg& cfg, void* base, int p_cap, bool full) {
    Carver c(base);
    FieldTrainWs w;
    carve_pass(c, w.b, 1, p_cap, full, true, true, cfg.bf16 ? 2 : 4);
    w.m_bott = c.take<float>(BOTT_SCRATCH_F);
    w.queue = c.take<int>(4);
    w.bytes = c.off + 256;
    return w;
}
