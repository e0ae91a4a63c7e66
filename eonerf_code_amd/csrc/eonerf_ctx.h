// The context behind the C ABI (include/eonerf_hip.h) and what its translation units share: eonerf_ctx.hip (context, weights, status,
// optimizer), eonerf_field.hip (eonerf_field_*, ray generation) and eonerf_render.hip (sampling, rendering, the training step).  Host
// logic only; no device memory is allocated after eonerf_create.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <unordered_map>

#include "../../include/eonerf_hip.h"
#include "eonerf_kernels.h"
#include "eonerf_pack.h"
#include "eonerf_rays.h"
#include "eonerf_carve.h"
#include "eonerf_wgrad_plan.h"

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

struct DevStream {
    uint8_t* data = nullptr; size_t bytes = 0;
    ChunkDesc* chunks = nullptr; int n_chunks = 0;
    PackEntry *e16 = nullptr, *e32 = nullptr, *e16lo = nullptr; int n16 = 0, n32 = 0, n16lo = 0;      // e16lo: lo halves of an fp16 x 3 stream
};

constexpr int RANGE_WORD = 16;      // ctx->dev_status[RANGE_WORD]: fp16 x 3 range flag (a cache line of its own; eonerf_range_status)
constexpr int RANGE_STICKY_WORD = 17;   // ... and the WEIGHT criteria of the last re-pack: reported like RANGE_WORD, cleared only by the next eonerf_set_weights
constexpr int DIGEST_WORD = 32;     // ctx->dev_status[32..35]: two 64-bit ray digests (eonerf_rays.h: ray_word_digest) -- [0] what eonerf_presample's
                                    // sampler read, [1] what the backward of the forward that consumed those samples finds in the same buffers

struct eonerf_ctx {
    eonerf_config cfg;
    int n_samples = 128;  // int(2 / render_step_size) of the next calls: 2 .. 256 (eonerf_set_n_samples; cfg.n_samples at create)
    int prec;             // cfg.precision: EONERF_FP32 / EONERF_BF16 / EONERF_F16X3 (inference only)
    bool bf16;
    int n_cu;
    int enc_pair = 1;       // the shadow pass' encoding products and input-gradient tail in one kernel (eonerf_enc_pair.hip; EONERF_ENC_PAIR=0: ig_tail + two GEMM jobs)
    int pipe_xcd = 0;       // XCD-local pipelines of the pipelined backward (EONERF_PIPE_XCD; BwdPipeArgs::xcd_local)
    int stagger = 0;        // wave stagger of the chain kernels (EONERF_STAGGER; MlpFwdArgs::stagger)
    int wgrad_riders = 1;   // EONERF_WGRAD_RIDERS=0: the sigma row and the embedding columns as jobs of their own (A/B switch)
    ParamLayout pl;
    DevStream fwd_full, fwd_dens, bwd_full, bwd_dens, bwd_rgb, bwd_full_ig, pipe_wt, bwd_full_heads, bwd_rgb_heads, bwd_dens_heads, ig_tail_wt;
    bool pipe = false;               // layer-pipelined trunk backward (bf16 camera pass; EONERF_PIPE=0 switches back to chain + GEMM)
    int n_pipes = 0;
    float* loss_scratch = nullptr;   // [LOSS_MAX_BLOCKS] per-block partial sums of k_loss + its arrival counter (self-resetting: no memset per step)
    float* fold = nullptr;           // [FOLD_FLOATS (+ 256 x 256: W_bott transposed, for the backward's tail kernel)] fp32: the heads' first layers folded with the bottleneck layer (eonerf_pack.h), re-computed
                                     // by k_fold in front of every re-pack
    bool pipe_fallback = true;       // after a REPORTED watchdog fault the context leaves the pipelined path for good (EONERF_PIPE_FALLBACK=0: stay)
    bool need_repack = false;        // ... and the chain + GEMM path's weight streams have to be packed before the next call
    // Training forwards whose backward is still outstanding: workspace -> the path (pipelined or chain + GEMM) its layout was carved for and
    // its mask slots were written for.  A backward runs in the mode of ITS forward even if eonerf_device_status switched the context in
    // between (the autograd paths keep a workspace across arbitrary host code: render_image chunks, EONerfMLP.rendering)
    std::unordered_map<const void*, bool> ws_pipe;
    int pipe_fault_stage = -1;       // test hook (EONERF_PIPE_FAULT)
    bool deterministic = false;      // EONERF_DETERMINISTIC=1: every atomic flush of the backward is replaced by partials + a fixed-order sum
                                     // (the pipelined launches: partial buffers + a reduction kernel)
    unsigned long long* pipe_stamps = nullptr;   // diagnostics (EONERF_PIPE_STAMPS=1): cycle sums per stage, read by eonerf_debug_pipe_stamps
    uint64_t noise_seed = 0x5eed5eedULL; uint32_t noise_call = 0;   // in-kernel Philox jitter (eonerf_set_noise_seed)
    // eonerf_presample: the camera sampler of the NEXT training forward already ran (under the gradient exchange of the step before);
    // the forward whose arguments and carve match consumes the record, any other forward drops it and samples again
    struct Presample { bool valid = false; const void* ws = nullptr; const float* rays = nullptr; const int64_t* img_idx = nullptr;
                       const float* zsteps = nullptr; const int* count_out = nullptr; int n_rays = 0, flags = 0, n_samples = 0; bool pipe = false; uint32_t call = 0; } pre;
    // two-bucket gradient exchange (eonerf_set_exchange_event): recorded on the backward's stream as soon as the EARLY block of the
    // gradient message (ParamLayout::early) is final; exch_cus CUs are left out of the grids of the gradient kernels launched behind that
    // point, so that the collective's kernel finds a CU while they run (every large kernel here fills the CUs it is given)
    hipEvent_t exch_event = nullptr; int exch_cus = 0; bool exch_recorded = false;
    const void* pre_consumed_ws = nullptr;   // workspace of the training forward that consumed a presample record: its backward checks the ray digest
    // include/eonerf_pose.h: the last render backward that completed -- what eonerf_render_origin_grad may read (the forward's path record
    // in ws_pipe is spent by then); dropped by every call that writes a workspace, re-packs the weights or presamples
    struct PoseRec { bool valid = false; const void* ws = nullptr; int n_rays = 0, flags = 0, n_samples = 0; bool pipe = false; } pose;
    bool full_ig_dirty = false;      // packed lazily: only a differentiable EONerfMLP.forward with an input gradient reads it
    int* enc_colmap = nullptr;       // [64] device: encoding slot -> reference column (or -1)
    int* dev_status = nullptr;       // STICKY device status word (watchdog bits of the pipelined backward, bit 8: a remote rank's fault);
                                     // written by the kernels, gates eonerf_adam_step, read and cleared only by eonerf_device_status
    // occupancy grid of the export renders (eonerf_set_occupancy, include/eonerf_occ.h): a BORROWED device bit field, or nullptr
    const uint32_t* occ_bits = nullptr; int occ_r = 0;
    bool weights_set = false;
    bool dens_dirty = false;         // density-only streams are re-packed lazily (only the shadow pass reads them) ...
    bool dens_used = false;          // ... unless the cycle since the last re-pack used them: then they are re-packed with the others (one launch fewer per step)
    // measurement hooks
    int prof_cap = 0;
    std::vector<hipEvent_t> prof_ev[EONERF_PROF_KERNELS][2];
    int prof_n[EONERF_PROF_KERNELS] = {};
};

inline CarveCfg carve_cfg(const eonerf_ctx* ctx) {
    CarveCfg c;
    c.bf16 = ctx->bf16; c.pipe = ctx->pipe; c.deterministic = ctx->deterministic; c.pipe_partials = ctx->deterministic;
    c.n_pipes = ctx->n_pipes; c.n_samples = ctx->n_samples;
    c.enc_part_wgs = (ctx->enc_pair && ctx->pipe && !ctx->deterministic) ? ctx->n_cu : 0;
    return c;
}
inline RenderWs carve_render(const eonerf_ctx* ctx, void* base, int n_rays, int flags) { return carve_render(carve_cfg(ctx), base, n_rays, flags); }

struct ProfScope {      // brackets one kernel launch with events when profiling is on
    eonerf_ctx* c; int k; hipStream_t st; bool on;
    ProfScope(eonerf_ctx* ctx, int kernel, hipStream_t s) : c(ctx), k(kernel), st(s), on(kernel >= 0 && ctx->prof_cap > 0 && ctx->prof_n[kernel] < ctx->prof_cap) {
        if (on) (void)hipEventRecord(c->prof_ev[k][0][c->prof_n[k]], st);
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(c->prof_ev[k][1][c->prof_n[k]], st); c->prof_n[k]++; } }
};

inline bool slabs_addressable(const eonerf_ctx* ctx, size_t p_cap) { return slab_blocks_addressable(ctx->bf16, p_cap); }
// a call that writes `ws` ends what eonerf_presample left there
inline void drop_presample(eonerf_ctx* ctx, const void* ws) { if (ctx->pre.valid && ctx->pre.ws == ws) ctx->pre.valid = false; ctx->pose.valid = false; }
// rays per call: n_rays x (n_samples - 1) samples must stay below 2^31
inline bool rays_in_range(const eonerf_ctx* ctx, int n_rays) { return n_rays <= (1 << 24) / (ctx->n_samples > 128 ? ctx->n_samples / 128 : 1); }
// grid of the chain kernels (eonerf_mlp_fwd.hip, eonerf_mlp_bwd.hip): persistent workgroups, one per CU, never more than sample tiles
inline int chain_grid(const eonerf_ctx* ctx, int p_cap) { return std::min(ctx->n_cu, p_cap / (ctx->bf16 ? PBf16::TILE : PF32::TILE)); }

inline void note_train_forward(eonerf_ctx* ctx, const void* ws) {
    if (ctx->ws_pipe.size() > 1024) ctx->ws_pipe.clear();       // forwards that never saw a backward (caller dropped the graph)
    ctx->ws_pipe[ws] = ctx->pipe;
}
// A backward call runs on the path its forward ran on; the context's own choice is restored on return.  spend: the forward's record is
// used up (a backward runs once per forward); false: only looked up, for a check in front of the backward itself
struct PipeModeGuard {
    eonerf_ctx* c; bool keep; const void* ws_; bool spend;
    PipeModeGuard(eonerf_ctx* ctx, const void* ws, bool spend_record = true) : c(ctx), keep(ctx->pipe), ws_(ws), spend(spend_record) {
        auto it = c->ws_pipe.find(ws);
        if (it != c->ws_pipe.end()) c->pipe = it->second;
    }
    ~PipeModeGuard() { c->pipe = keep; if (spend) c->ws_pipe.erase(ws_); }
};

inline AmbientW ambient_w(const eonerf_ctx* ctx, const float* flat) {
    const ParamLayout& pl = ctx->pl;
    return AmbientW{flat + pl.t[pl.am1_w].offset, flat + pl.t[pl.am1_b].offset, flat + pl.t[pl.am2_w].offset, flat + pl.t[pl.am2_b].offset};
}

// CUs the pipelined launch leaves without a stage (256 - 7 x 36 = 4): enough of them, and the per-ray ambient-head backward rides there
inline int pipe_spare_cus(const eonerf_ctx* ctx) {
    const int spare = ctx->n_cu - ctx->n_pipes * PIPE_STAGES;
    return (ctx->pipe && !ctx->deterministic && spare >= 2) ? std::min(spare, 8) : 0;
}

// what a backward chain launch (eonerf_mlp_bwd.hip) takes from its pass' buffers and its packed stream; buffers a pass does not have are null
inline MlpBwdArgs mlp_bwd_args(const eonerf_ctx* ctx, const PassBuffers& b, int p_cap, const DevStream& bs) {
    MlpBwdArgs m;
    memset(&m, 0, sizeof(m));
    m.stagger = ctx->stagger;
    m.n_pts = b.n_pts; m.p_pad = p_cap;
    m.stream = bs.data; m.chunks = bs.chunks; m.n_chunks = bs.n_chunks;
    m.sigma = b.sigma; m.albedo = b.albedo; m.ts = b.ts; m.tb = b.tb;
    m.g_sigma = b.g_sigma; m.g_albedo = b.g_albedo; m.g_ts = b.g_ts; m.g_tb = b.g_tb;
    m.masks = b.masks; m.grd = b.grd; m.g_emb = b.g_emb;
    m.px = b.px; m.py = b.py; m.pz = b.pz; m.g_pos = b.g_pos;      // (density variants only: the chain + GEMM path ends in d position)
    return m;
}

// eonerf_ctx.hip: (re)packs the fp32 master weights into the given streams; the density-only streams on their first use since the last re-pack
int eo_pack(const eonerf_ctx* ctx, const std::vector<const DevStream*>& streams, const float* flat, hipStream_t st);
int eo_ensure_density_streams(eonerf_ctx* ctx, const float* flat, hipStream_t st);
// eonerf_render.hip: eonerf_sample_rays with an explicit occupancy grid (bits == nullptr: none) -- eonerf_occ_sample_rays
int eo_sample_rays(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays, const uint32_t* bits, int r,
                   int64_t* ray_indices, float* t_starts, float* t_ends, float* pts_per_ray, int* n_dev, void* ws, size_t ws_bytes, void* stream);
// eonerf_render.hip: one MLP pass forwards; the weight gradients of up to two passes
int eo_run_mlp_fwd(eonerf_ctx* ctx, const PassBuffers& b, const float* flat, int p_cap, bool full, int mode, hipStream_t st, int prof_id = -1, bool render_train = false);
int eo_run_weight_gradients(eonerf_ctx* ctx, const float* flat, float* d_flat, const PassBuffers* full, const PassBuffers* dens, int p_cap, float* m_bott,
                            int* queue, hipStream_t st, WgradPlanOpts o, float* det_partials = nullptr, BottWgradArgs* defer_bott = nullptr);
