// EONerfMLP.forward / query_density on caller-provided points (eonerf_field_*: inference, and the autograd pair) and the ray generator:
// entry points of libeonerf_hip.so (include/eonerf_hip.h).  Host logic only.
#include <math.h>

#include "eonerf_ctx.h"
#include "eonerf_raygen.h"
#include "eonerf_rpc_dev.h"
#include "eonerf_layout_table.h"

extern "C" {

size_t eonerf_field_workspace_bytes(const eonerf_ctx* ctx, int n_points) {
    if (!ctx || n_points < 0) return 0;
    return carve_field(carve_cfg(ctx), nullptr, field_p_cap_of(n_points)).bytes;
}

static int field_common(eonerf_ctx* ctx, const float* flat, const float* xyz, const int64_t* img, int n, bool full,
                        void* ws, size_t ws_bytes, PassBuffers& b, int& p_cap, hipStream_t st) {
    if (!ctx || !xyz || n < 0 || !ws) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (ws_bytes < eonerf_field_workspace_bytes(ctx, n)) return EONERF_E_WORKSPACE;
    drop_presample(ctx, ws);
    p_cap = field_p_cap_of(n);
    b = carve_field(carve_cfg(ctx), ws, p_cap).b;
    HIP_TRY(eo_launch_points_to_soa(xyz, img, n, p_cap, b.px, b.py, b.pz, b.simg, b.n_pts, st));
    return eo_run_mlp_fwd(ctx, b, flat, p_cap, full, 0, st);
}

int eonerf_field_forward(eonerf_ctx* ctx, const float* flat, const float* xyz, const float* sun, const int64_t* img, int n,
                         float* sigma, float* albedo, float* ambient, float* ts, float* tb,
                         void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return EONERF_OK;
    if (!sun || !img || !sigma || !albedo || !ambient || !ts || !tb || !flat) return EONERF_E_ARG;
    PassBuffers b; int p_cap;
    int rc = field_common(ctx, flat, xyz, img, n, true, ws, ws_bytes, b, p_cap, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sigma, b.sigma, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(ts, b.ts, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(tb, b.tb, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(eo_launch_soa3_to_aos(b.albedo, p_cap, n, albedo, st));
    return (int)eo_launch_ambient_points(ambient_w(ctx, flat), sun, n, ambient, st);
}

int eonerf_query_density(eonerf_ctx* ctx, const float* flat, const float* xyz, int n, float* sigma, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return EONERF_OK;
    if (!sigma || !flat) return EONERF_E_ARG;
    PassBuffers b; int p_cap;
    int rc = field_common(ctx, flat, xyz, nullptr, n, false, ws, ws_bytes, b, p_cap, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sigma, b.sigma, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return EONERF_OK;
}

// ---- differentiable EONerfMLP.forward / query_density (radiance_fields/eonerf.py:141-170 under autograd) ----------------
// (layout: carve_field_train, eonerf_carve.h)
size_t eonerf_field_train_workspace_bytes(const eonerf_ctx* ctx, int n_points, int density_only) {
    if (!ctx || n_points < 0) return 0;
    return carve_field_train(carve_cfg(ctx), nullptr, field_p_cap_of(n_points), !density_only).bytes;
}

int eonerf_field_forward_train(eonerf_ctx* ctx, const float* flat, const float* xyz, const float* sun, const int64_t* img, int n,
                               int density_only, float* sigma, float* albedo, float* ambient, float* ts, float* tb,
                               void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !xyz || !sigma || n < 0 || !ws) return EONERF_E_ARG;
    if (!density_only && (!sun || !img || !albedo || !ambient || !ts || !tb)) return EONERF_E_ARG;
    drop_presample(ctx, ws);
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (n == 0) return EONERF_OK;
    if (n > (1 << 30)) return EONERF_E_UNSUPPORTED;
    const int p_cap = round_up(n, 256);
    if (!slabs_addressable(ctx, (size_t)p_cap)) return EONERF_E_UNSUPPORTED;
    const bool full = !density_only;
    FieldTrainWs w = carve_field_train(carve_cfg(ctx), ws, p_cap, full);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    if (ctx->need_repack) { const int rcr = eonerf_set_weights(ctx, flat, stream); if (rcr) return rcr; }      // (after the fault fallback)
    HIP_TRY(eo_launch_points_to_soa(xyz, full ? img : nullptr, n, p_cap, w.b.px, w.b.py, w.b.pz, w.b.simg, w.b.n_pts, st));
    int rc = eo_run_mlp_fwd(ctx, w.b, flat, p_cap, full, 1, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sigma, w.b.sigma, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (!full) return EONERF_OK;
    HIP_TRY(hipMemcpyAsync(ts, w.b.ts, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(tb, w.b.tb, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(eo_launch_soa3_to_aos(w.b.albedo, p_cap, n, albedo, st));
    return (int)eo_launch_ambient_points(ambient_w(ctx, flat), sun, n, ambient, st);
}

int eonerf_field_backward(eonerf_ctx* ctx, const float* flat, const float* sun, int n, int density_only,
                          const float* g_sigma, const float* g_albedo, const float* g_ambient, const float* g_ts, const float* g_tb,
                          float* d_flat, float* d_xyz, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !d_flat || n < 0 || !ws) return EONERF_E_ARG;
    if (ctx->prec == EONERF_F16X3) return EONERF_E_UNSUPPORTED;
    if (ctx->pre.valid && ctx->pre.ws == ws) return EONERF_E_STATE;
    if (!density_only && g_ambient && !sun) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (n == 0) return EONERF_OK;
    if (n > (1 << 30)) return EONERF_E_UNSUPPORTED;
    const int p_cap = round_up(n, 256);
    if (!slabs_addressable(ctx, (size_t)p_cap)) return EONERF_E_UNSUPPORTED;
    const bool full = !density_only;
    FieldTrainWs w = carve_field_train(carve_cfg(ctx), ws, p_cap, full);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    const ParamLayout& pl = ctx->pl;
    PassBuffers& b = w.b;
    HIP_TRY(eo_launch_field_grads_to_soa(g_sigma, g_albedo, g_ts, g_tb, n, p_cap, b.g_sigma, b.g_albedo, b.g_ts, b.g_tb, st));
    if (full && ctx->full_ig_dirty) {
        const int rc = eo_pack(ctx, {&ctx->bwd_full_ig}, flat, st);
        if (rc) return rc;
        ctx->full_ig_dirty = false;
    }
    if (!full) { const int rc = eo_ensure_density_streams(ctx, flat, st); if (rc) return rc; }
    const MlpBwdArgs m = mlp_bwd_args(ctx, b, p_cap, full ? ctx->bwd_full_ig : ctx->bwd_dens);
    HIP_TRY(eo_launch_mlp_bwd(m, ctx->bf16, full, true, full, chain_grid(ctx, p_cap), st));
    const int rc = eo_run_weight_gradients(ctx, flat, d_flat, full ? &b : nullptr, full ? nullptr : &b, p_cap, w.m_bott, w.queue, st, WgradPlanOpts());
    if (rc) return rc;
    if (d_xyz) HIP_TRY(eo_launch_soa3_to_aos(b.g_pos, p_cap, n, d_xyz, st));
    if (!full) return EONERF_OK;
    HIP_TRY(eo_launch_emb_grad_points(b.g_emb, b.simg, n, d_flat + pl.t[pl.emb].offset, st));
    if (g_ambient)
        HIP_TRY(eo_launch_ambient_points_bwd(ambient_w(ctx, flat), sun, g_ambient, n, d_flat + pl.t[pl.am1_w].offset, d_flat + pl.t[pl.am1_b].offset,
                                             d_flat + pl.t[pl.am2_w].offset, d_flat + pl.t[pl.am2_b].offset, st));
    return EONERF_OK;
}

int eonerf_generate_rays(const eonerf_rpc* rpc, const double* cols, const double* rows, long n, int width,
                         double min_alt, double max_alt, int utm_zone, int south,
                         double sun_elevation_deg, double sun_azimuth_deg, const float offset[3], const float scale[3],
                         float* raw8, float* rays, double* geo, void* stream) {
    if (!rpc || n < 0 || (!raw8 && !rays && !geo) || (!cols != !rows) || (!cols && width < 1) || utm_zone < 1 || utm_zone > 60) return EONERF_E_ARG;
    if (rays && (!offset || !scale)) return EONERF_E_ARG;
    if (n == 0) return EONERF_OK;
    static_assert(sizeof(eonerf_rpc) == sizeof(RpcModel), "RPC struct mismatch");
    RayGenArgs a;
    memcpy(&a.rpc, rpc, sizeof(RpcModel));
    a.utm = eo_utm_params(utm_zone, south);
    a.cols = cols; a.rows = rows; a.n = n; a.width = width; a.min_alt = min_alt; a.max_alt = max_alt;
    // get_sun_dirs(90 - elevation, azimuth) -> get_dir_vec_from_el_az (datasets/satellite.py:457,57-63)
    const double d2r = 0.017453292519943295;
    const double el = (90.0 - (90.0 - sun_elevation_deg)) * d2r, az = sun_azimuth_deg * d2r;
    a.sun[0] = -1.0 * (sin(az) * cos(el)); a.sun[1] = -1.0 * (cos(az) * cos(el)); a.sun[2] = -1.0 * sin(el);
    for (int k = 0; k < 3; ++k) { a.offset[k] = offset ? offset[k] : 0.f; a.scale[k] = scale ? scale[k] : 1.f; }
    a.raw8 = raw8; a.rays = rays; a.geo = geo;
    return (int)eo_launch_raygen(a, (hipStream_t)stream);
}

// ---- include/eonerf_layout.h: where the next call of that kind on this context puts its buffers (host arithmetic only) ----
int eonerf_layout_version(void) { return EONERF_LAYOUT_VERSION; }

int eonerf_workspace_layout(const eonerf_ctx* ctx, int kind, int n, int flags, uint64_t* out, int cap) {
    if (!ctx) return EONERF_E_ARG;
    return workspace_layout_table(carve_cfg(ctx), kind, n, flags, out, cap);
}

int eonerf_ray_layout(const eonerf_ctx* ctx, int n_rays, int flags, uint64_t* out, int cap) {
    if (!ctx) return EONERF_E_ARG;
    return ray_layout_table(carve_cfg(ctx), n_rays, flags, out, cap);
}

}  // extern "C"
