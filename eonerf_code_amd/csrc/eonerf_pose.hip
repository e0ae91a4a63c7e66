// Camera offset refinement (include/eonerf_pose.h): d loss / d ray origin of a training step and its per-image sum, taken behind the
// render backward from what that backward left in its workspace.  The workspace is only read.
//   camera samples:  g = (W_0^T dY_0 + W_5[:, 256:]^T dY_5) . d enc / d x
//     bf16, pipelined path: the camera slab holds dY_0 / dY_5 in B-operand unit order exactly as the shadow slab does -> k_ig_tail
//                           (eonerf_ig_tail.hip) on the camera pass' tiles and positions;
//     fp32:                 k_pose_ig_f32 below, a reader of the feature-major dY rows the weight-gradient GEMM reads;
//   shadow samples:  the backward's own w.sun.g_pos (a shadow ray starts at o + depth * d, sat_rendering.py:90);
//   k_pose_rays:     one wavefront per ray, its camera samples and then its shadow samples -- the walk of k_cam_composite_bwd's
//                    sun_g_pos loop;  k_pose_images: one workgroup per image over the rays in index order.
// No atomics: every sum has a fixed order.
#include "eonerf_ctx.h"
#include "eonerf_pose_check.h"

namespace {

struct PoseIgF32Args {
    const int* n_pts; int p_pad;
    const float* grd;            // fp32 gradient slab (block-major, eonerf_common.h): segment = one feature row of 16 samples
    const float *w0, *w5; int ld0, ld5;   // trunk layer 0 [256][63] and layer 5 [256][319] of the flat parameter buffer, their row strides
    const float *px, *py, *pz;
    float* g_pos;                // [3][p_pad]
};

// one workgroup per 16-sample tile: thread = (sample s, column group cg), columns cg, cg + 16, cg + 32, cg + 48 of the 63 encoding
// columns in the reference's order (mlp.py:190-208: x y z | sin(2^k x_d) | sin(2^k x_d + pi/2), k-major); rows summed in index order
__global__ __launch_bounds__(256) void k_pose_ig_f32(PoseIgF32Args a) {
    __shared__ float denc[64][16];
    const int n_pts = *a.n_pts;
    const int tile = blockIdx.x;
    if (tile * 16 >= n_pts) return;                 // (uniform for the workgroup)
    const int s = threadIdx.x & 15, cg = threadIdx.x >> 4;
    const size_t nt = (size_t)a.p_pad / 16;
    const float* y0 = a.grd + ((size_t)GRD_ROW_Y0 * nt + (size_t)tile * 256) * 16 + s;
    const float* y5 = a.grd + ((size_t)(GRD_ROW_Y0 + 5 * 256) * nt + (size_t)tile * 256) * 16 + s;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < 256; ++m) {
        const float v0 = y0[(size_t)m * 16], v5 = y5[(size_t)m * 16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = cg + 16 * k;
            if (col < 63) acc[k] += a.w0[m * a.ld0 + col] * v0 + a.w5[m * a.ld5 + 256 + col] * v5;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) denc[cg + 16 * k][s] = acc[k];
    __syncthreads();
    if (threadIdx.x < 48) {
        const int d = threadIdx.x >> 4, p = tile * 16 + s;
        if (p < n_pts) {
            const float x = d == 0 ? a.px[p] : (d == 1 ? a.py[p] : a.pz[p]);
            float g = denc[d][s];
            for (int k = 0; k < 10; ++k) {
                const float f = (float)(1 << k), arg = x * f;
                g += denc[3 + 3 * k + d][s] * (cosf(arg) * f);
                g += denc[33 + 3 * k + d][s] * (cosf(arg + EO_PI_2_F) * f);
            }
            a.g_pos[(size_t)d * a.p_pad + p] = g;
        }
    }
}

struct PoseRaysArgs {
    int n_rays, p_pad;
    const int *cam_offsets, *cam_counts; const float* cam_g;       // [3][p_pad]
    const int *sun_offsets, *sun_counts; const float* sun_g;       // shadow pass, or null
    float* d_origins;                                              // [n_rays][3]
};

// lane l takes samples l, l + 64, ... of the ray in index order (camera pass, then shadow pass); the 64 partial sums meet in a fixed tree
__global__ __launch_bounds__(256) void k_pose_rays(PoseRaysArgs a) {
    const int lane = threadIdx.x & 63, ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    float g[3] = {0.f, 0.f, 0.f};
    {
        const int off = a.cam_offsets[ray], n = a.cam_counts[ray];
        for (int i = lane; i < n; i += 64)
#pragma unroll
            for (int d = 0; d < 3; ++d) g[d] += a.cam_g[(size_t)d * a.p_pad + off + i];
    }
    if (a.sun_g) {
        const int off = a.sun_offsets[ray], n = a.sun_counts[ray];
        for (int i = lane; i < n; i += 64)
#pragma unroll
            for (int d = 0; d < 3; ++d) g[d] += a.sun_g[(size_t)d * a.p_pad + off + i];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) g[d] += __shfl_xor(g[d], m, 64);
    if (lane < 3) a.d_origins[(size_t)ray * 3 + lane] = lane == 0 ? g[0] : (lane == 1 ? g[1] : g[2]);
}

// one workgroup per image: thread t takes rays t, t + 256, ... in index order, the 256 partial sums meet in a fixed tree; an image
// without a ray in the batch is not written
__global__ __launch_bounds__(256) void k_pose_images(const float* d_origins, const int64_t* img_idx, int n_rays, float* d_offsets) {
    __shared__ float part[3][256];
    __shared__ int any[256];
    const int img = blockIdx.x, t = threadIdx.x;
    float g[3] = {0.f, 0.f, 0.f};
    int hit = 0;
    for (int r = t; r < n_rays; r += 256)
        if (img_idx[r] == img) {
            hit = 1;
#pragma unroll
            for (int d = 0; d < 3; ++d) g[d] += d_origins[(size_t)r * 3 + d];
        }
#pragma unroll
    for (int d = 0; d < 3; ++d) part[d][t] = g[d];
    any[t] = hit;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int d = 0; d < 3; ++d) part[d][t] += part[d][t + w];
            any[t] |= any[t + w];
        }
        __syncthreads();
    }
    if (t < 3 && any[0]) d_offsets[(size_t)img * 3 + t] += part[t][0];
}

}  // namespace

extern "C" {

int eonerf_pose_version(void) { return EONERF_POSE_VERSION; }

size_t eonerf_origin_grad_scratch_bytes(const eonerf_ctx* ctx, int n_rays, int flags) {
    (void)flags;
    PoseScratch s;
    if (!ctx || n_rays < 0 || !pose_scratch(n_rays, ctx->n_samples, &s)) return 0;
    return s.bytes;
}

int eonerf_render_origin_grad(eonerf_ctx* ctx, const float* flat, const float* rays, const int64_t* img_idx, int n_rays, int flags,
                              const void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                              float* d_origins, float* d_offsets, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = pose_check_args(ctx, flat, rays, img_idx, n_rays, flags, ws, scratch, d_origins, d_offsets);
    if (rc) return rc;
    if (ctx->prec == EONERF_F16X3) return EONERF_E_UNSUPPORTED;
    if (n_rays == 0) return EONERF_OK;
    const eonerf_ctx::PoseRec& rec = ctx->pose;
    rc = pose_check_record(rec.valid, rec.ws, rec.n_rays, rec.flags, rec.n_samples, ws, n_rays, flags, ctx->n_samples);
    if (rc) return rc;
    if (ctx->bf16 && !rec.pipe) return EONERF_E_UNSUPPORTED;      // chain + GEMM path in bf16: its camera chain has no input-gradient tail
    // the layout of the path the backward ran on (the context may have left the pipelined path since: eonerf_device_status)
    CarveCfg cc = carve_cfg(ctx);
    cc.pipe = rec.pipe;
    cc.enc_part_wgs = (ctx->enc_pair && rec.pipe && !ctx->deterministic) ? ctx->n_cu : 0;
    const RenderWs w = carve_render(cc, const_cast<void*>(ws), n_rays, flags);
    rc = pose_check_sizes(n_rays, ctx->n_samples, ws_bytes, w.bytes, scratch_bytes);
    if (rc) return rc;
    PoseScratch ps;
    pose_scratch(n_rays, ctx->n_samples, &ps);
    const int p_cap = p_cap_of(n_rays, ctx->n_samples);
    float* cam_g = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch) + ps.g_pos_off);
    float* per_ray = d_origins ? d_origins : reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch) + ps.rays_off);
    const ParamLayout& pl = ctx->pl;

    if (ctx->bf16) {
        // W_0^T / W_5 skip^T as A units: packed with the density streams, which a step without the shadow pass leaves for later
        if (ctx->dens_dirty) { rc = eo_pack(ctx, {&ctx->ig_tail_wt}, flat, st); if (rc) return rc; }
        IgTailArgs ta;
        ta.n_pts = w.cam.n_pts; ta.p_pad = p_cap; ta.grd = w.cam.grd; ta.wt = ctx->ig_tail_wt.data;
        ta.px = w.cam.px; ta.py = w.cam.py; ta.pz = w.cam.pz; ta.g_pos = cam_g;
        HIP_TRY(eo_launch_ig_tail(ta, ctx->n_cu, st));
    } else {
        PoseIgF32Args fa;
        fa.n_pts = w.cam.n_pts; fa.p_pad = p_cap; fa.grd = reinterpret_cast<const float*>(w.cam.grd);
        fa.w0 = flat + pl.t[pl.trunk_w[0]].offset; fa.w5 = flat + pl.t[pl.trunk_w[5]].offset;
        fa.ld0 = pl.t[pl.trunk_w[0]].cols; fa.ld5 = pl.t[pl.trunk_w[5]].cols;
        if (fa.ld0 != 63 || fa.ld5 != 319) return EONERF_E_UNSUPPORTED;
        fa.px = w.cam.px; fa.py = w.cam.py; fa.pz = w.cam.pz; fa.g_pos = cam_g;
        hipLaunchKernelGGL(k_pose_ig_f32, dim3(p_cap / 16), dim3(256), 0, st, fa);
        HIP_TRY(hipGetLastError());
    }
    PoseRaysArgs ra;
    ra.n_rays = n_rays; ra.p_pad = p_cap;
    ra.cam_offsets = w.cam.offsets; ra.cam_counts = w.cam.counts; ra.cam_g = cam_g;
    const bool shadows = flags & EONERF_F_SHADOWS;
    ra.sun_offsets = shadows ? w.sun.offsets : nullptr; ra.sun_counts = shadows ? w.sun.counts : nullptr; ra.sun_g = shadows ? w.sun.g_pos : nullptr;
    ra.d_origins = per_ray;
    hipLaunchKernelGGL(k_pose_rays, dim3((n_rays + 3) / 4), dim3(256), 0, st, ra);
    HIP_TRY(hipGetLastError());
    if (d_offsets) {
        hipLaunchKernelGGL(k_pose_images, dim3(ctx->cfg.n_images), dim3(256), 0, st, per_ray, img_idx, n_rays, d_offsets);
        HIP_TRY(hipGetLastError());
    }
    return EONERF_OK;
}

}  // extern "C"
