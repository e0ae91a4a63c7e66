// True orthophoto on the device (include/eonerf_ortho.h): surface points of a render -> inverse UTM series -> each image's RPC ->
// bilinear gather of the image's own pixels, occluded points left out -> mean or median mosaic.  The gather form of the chain
// k_prior_splat (eonerf_prior.hip) runs as a scatter; follows datasets/satellite.py:502-543 and sat_utils.py:420-432 of the reference.
// Everything is fp64 (one thread per point) until the one cast to fp32 of each output.
// Built with -ffp-contract=off: the reference's numpy / torch arithmetic is unfused.
// Cost: the ground step is the Krueger series and five Newton steps per point, hoisted out of the per-image call; the gather is four
// cubics and two divides per point and image; the RPC is uniform across the wave and travels in the kernel arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_ortho.h"
#include "eonerf_ortho_check.h"
#include "eonerf_rpc_dev.h"

namespace {

constexpr int kBlock = kOrthoBlock;

struct GroundArgs {
    const float* rays; int stride; const float* depth; long n;
    double scale[3], offset[3];
    UtmParams utm; double beta[6];
    double* out;
};

__global__ __launch_bounds__(kBlock) void k_ortho_ground(GroundArgs a) {
    const long p = (long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    double* o = a.out + (size_t)p * 3;
    const double depth = (double)a.depth[p];
    if (!isfinite(depth)) { o[0] = o[1] = o[2] = __builtin_nan(""); return; }
    const float* ray = a.rays + (size_t)p * a.stride;
    double xyz[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) xyz[k] = ((double)ray[k] + (double)ray[3 + k] * depth) * a.scale[k] + a.offset[k];      // satellite.py:521-524
    double lon, lat;
    utm_inverse(a.utm, a.beta, xyz[0], xyz[1], lon, lat);
    o[0] = lon; o[1] = lat; o[2] = xyz[2];
}

struct GatherArgs {
    RpcModel rpc;
    const double* lla; long n;
    const float* pixels; int h, w, channels;
    double gain[4], bias[4];
    const float* vis; float min_vis;
    float* layer; float* weight; double* colrow;
};

__global__ __launch_bounds__(kBlock) void k_ortho_gather(GatherArgs a) {
    const long p = (long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const double lon = a.lla[(size_t)p * 3], lat = a.lla[(size_t)p * 3 + 1], alt = a.lla[(size_t)p * 3 + 2];
    const RpcModel& r = a.rpc;
    double x, y;
    project_n(r, (lat - r.lat_offset) / r.lat_scale, (lon - r.lon_offset) / r.lon_scale, (alt - r.alt_offset) / r.alt_scale, x, y);
    const double col = x * r.col_scale + r.col_offset, row = y * r.row_scale + r.row_offset;
    if (a.colrow) { a.colrow[(size_t)p * 2] = col; a.colrow[(size_t)p * 2 + 1] = row; }
    if (!a.layer && !a.weight) return;
    bool ok = isfinite(lon) && isfinite(lat) && isfinite(alt);
    ok = ok && col >= 0.0 && col <= (double)(a.w - 1) && row >= 0.0 && row <= (double)(a.h - 1);          // NaN fails
    float wgt = 1.0f;
    if (a.vis) {
        wgt = a.vis[p];
        ok = ok && wgt >= a.min_vis;
    }
    double v[4] = {0, 0, 0, 0};
    if (ok) {       // only now are the four taps inside the image
        const double fc = floor(col), fr = floor(row);
        const int c0 = (int)fc, r0 = (int)fr;
        const int c1 = min(c0 + 1, a.w - 1), r1 = min(r0 + 1, a.h - 1);
        const double fx = col - fc, fy = row - fr;
        const int C = a.channels;
        const float* p00 = a.pixels + ((size_t)r0 * a.w + c0) * C;
        const float* p01 = a.pixels + ((size_t)r0 * a.w + c1) * C;
        const float* p10 = a.pixels + ((size_t)r1 * a.w + c0) * C;
        const float* p11 = a.pixels + ((size_t)r1 * a.w + c1) * C;
        for (int c = 0; c < C; ++c) {
            const double t00 = (double)p00[c], t01 = (double)p01[c], t10 = (double)p10[c], t11 = (double)p11[c];
            ok = ok && isfinite(t00) && isfinite(t01) && isfinite(t10) && isfinite(t11);
            const double s = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t01) + fy * ((1.0 - fx) * t10 + fx * t11);
            v[c] = (s - a.bias[c]) / a.gain[c];
        }
    }
    if (!ok || wgt == 0.0f) wgt = 0.0f;
    if (a.weight) a.weight[p] = wgt;
    if (a.layer)
        for (int c = 0; c < a.channels; ++c) a.layer[(size_t)p * a.channels + c] = wgt != 0.0f ? (float)v[c] : __builtin_nanf("");
}

struct FuseArgs {
    const float* layers; const float* weights; int K; long n; int channels;
    float* mosaic; float* wsum; int32_t* count;
};

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_ortho_fuse(FuseArgs a) {
    const long p = (long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const int C = a.channels;
    const size_t n = (size_t)a.n;
    int m = 0;
    double ws = 0.0;
    for (int k = 0; k < a.K; ++k) {
        const float w = a.weights[(size_t)k * n + p];
        if (w > 0.0f) { ++m; ws += (double)w; }
    }
    if (a.count) a.count[p] = m;
    if (a.wsum) a.wsum[p] = (float)ws;
    if (!a.mosaic) return;
    float* out = a.mosaic + (size_t)p * C;
    if (m == 0) {
        for (int c = 0; c < C; ++c) out[c] = __builtin_nanf("");
        return;
    }
    if (MODE == EONERF_ORTHO_MEAN) {
        for (int c = 0; c < C; ++c) {
            double acc = 0.0;
            for (int k = 0; k < a.K; ++k) {                                  // ascending k: the sum's order is fixed
                const float w = a.weights[(size_t)k * n + p];
                if (w > 0.0f) acc += (double)w * (double)a.layers[((size_t)k * n + p) * C + c];
            }
            out[c] = (float)(acc / ws);
        }
    } else {
        float s[EONERF_ORTHO_MAX_MEDIAN];                                    // one cell's values of one channel, kept sorted; K <= 64 (host check)
        for (int c = 0; c < C; ++c) {
            int cnt = 0;
            for (int k = 0; k < a.K; ++k) {
                if (!(a.weights[(size_t)k * n + p] > 0.0f)) continue;
                const float val = a.layers[((size_t)k * n + p) * C + c];
                int j = cnt;                                                 // cnt < m <= K <= 64: s[j] stays inside the array
                while (j > 0 && s[j - 1] > val) { s[j] = s[j - 1]; --j; }
                s[j] = val;
                ++cnt;
            }
            out[c] = (float)(0.5 * ((double)s[(m - 1) / 2] + (double)s[m / 2]));       // numpy's median
        }
    }
}

}  // namespace

extern "C" {

int eonerf_ortho_version(void) { return EONERF_ORTHO_VERSION; }

int eonerf_ortho_ground(const float* rays, int ray_stride, const float* depth, long n, const float scene_scale[3],
                        const float scene_offset[3], int utm_zone, int south, double* lonlatalt_out, void* stream) {
    const int rc = ortho_check_ground(rays, ray_stride, depth, n, scene_scale, scene_offset, utm_zone, lonlatalt_out);
    if (rc != EONERF_OK || n == 0) return rc;
    GroundArgs a;
    a.rays = rays; a.stride = ray_stride; a.depth = depth; a.n = n; a.out = lonlatalt_out;
    for (int k = 0; k < 3; ++k) { a.scale[k] = (double)scene_scale[k]; a.offset[k] = (double)scene_offset[k]; }
    a.utm = eo_utm_params(utm_zone, south);
    eo_krueger_beta(a.beta);
    hipLaunchKernelGGL(k_ortho_ground, dim3(ortho_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int eonerf_ortho_gather(const double* lonlatalt, long n, const eonerf_rpc* rpc, const float* pixels, int h, int w, int channels,
                        const float* gain, const float* bias, const float* visibility, float min_visibility,
                        float* layer_out, float* weight_out, double* colrow_out, void* stream) {
    const int rc = ortho_check_gather(lonlatalt, n, rpc, pixels, h, w, channels, gain, bias, min_visibility, layer_out, weight_out, colrow_out);
    if (rc != EONERF_OK || n == 0) return rc;
    static_assert(sizeof(eonerf_rpc) == sizeof(RpcModel), "RPC struct mismatch");
    GatherArgs a;
    memcpy(&a.rpc, rpc, sizeof(RpcModel));
    a.lla = lonlatalt; a.n = n; a.pixels = pixels; a.h = h; a.w = w; a.channels = channels;
    for (int c = 0; c < 4; ++c) {
        a.gain[c] = (gain && c < channels) ? (double)gain[c] : 1.0;
        a.bias[c] = (bias && c < channels) ? (double)bias[c] : 0.0;
    }
    a.vis = visibility; a.min_vis = min_visibility;
    a.layer = layer_out; a.weight = weight_out; a.colrow = colrow_out;
    hipLaunchKernelGGL(k_ortho_gather, dim3(ortho_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int eonerf_ortho_fuse(const float* layers, const float* weights, int K, long n, int channels, int mode, float* mosaic_out,
                      float* weight_sum_out, int32_t* count_out, void* stream) {
    const int rc = ortho_check_fuse(layers, weights, K, n, channels, mode, mosaic_out, weight_sum_out, count_out);
    if (rc != EONERF_OK || n == 0) return rc;
    FuseArgs a;
    a.layers = layers; a.weights = weights; a.K = K; a.n = n; a.channels = channels;
    a.mosaic = mosaic_out; a.wsum = weight_sum_out; a.count = count_out;
    if (mode == EONERF_ORTHO_MEAN) hipLaunchKernelGGL(k_ortho_fuse<EONERF_ORTHO_MEAN>, dim3(ortho_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_ortho_fuse<EONERF_ORTHO_MEDIAN>, dim3(ortho_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
