// Depth priors from an initial DSM on the device (include/eonerf_prior.h): DSM -> every sample point through the inverse UTM series and
// the image's RPC -> last-writer-wins splat onto the image's pixel grid -> altitude (or a second raster) per pixel -> depth along the ray.
// Follows sat_utils.py:310-362,420-432 and datasets/satellite.py:644-653,677-679 of the reference.  pyproj's Transformer belongs to an
// un-vendored package and is restated from its published algorithm:
//   PROJ "+proj=utm" (etmerc), inverse   (6th-order Krueger series, beta coefficients; Newton on tan(lat) from the conformal latitude)
// -- utm_inverse of eonerf_rpc_dev.h, shared with eonerf_ortho.hip.
// Everything is fp64 (one thread per sample point / per pixel) until the one cast to fp32 of each output.
// Built with -ffp-contract=off: the reference's numpy / torch arithmetic is unfused.
// Reproducibility: numpy's fancy-index assignment keeps, for a pixel hit several times, the LAST point in raveled order.  "Last" is the
// largest point index, so the splat is an integer atomic max of (index + 1): order-independent, hence run-to-run bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_prior.h"
#include "eonerf_rpc_dev.h"

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

namespace {

constexpr int kBlock = 256;

struct PriorArgs {
    RpcModel rpc; UtmParams utm;
    double beta[6];
    const float *dsm, *values;      // values: what the raster output samples (never NULL: the DSM itself without a second raster)
    int h, w, out_h, out_w;
    double x_min, x_max, y_min, y_max;
    uint32_t* winner;               // [out_h*out_w]: 1 + raveled index of the last valid sample point, 0 = none
    float* raster; int nan_fill;
    const float* rays; int stride;
    float z_offset, z_scale;
    float* depth;
};

// np.linspace(start, stop, n)[k], n >= 2: arange(n) * step + start with step = (stop - start) / (n - 1), last element = stop
__device__ __forceinline__ double linspace_at(double start, double stop, int n, int k) {
    if (k == n - 1) return stop;
    const double step = (stop - start) / (double)(n - 1);
    return (double)k * step + start;
}

// raveled index1d of sample point p (sat_utils.py:331-333): truncation of the two linspaces over the DSM's rows and columns
__device__ __forceinline__ size_t source_cell(const PriorArgs& a, uint32_t p) {
    const int i = (int)(p / (uint32_t)(2 * a.w)), j = (int)(p % (uint32_t)(2 * a.w));
    const int r = (int)linspace_at(0.0, (double)(a.h - 1), 2 * a.h, i), c = (int)linspace_at(0.0, (double)(a.w - 1), 2 * a.w, j);
    return (size_t)r * a.w + c;
}

__global__ __launch_bounds__(kBlock) void k_prior_splat(PriorArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint64_t)4 * a.h * a.w) return;
    const uint32_t p = (uint32_t)t;
    const int i = (int)(p / (uint32_t)(2 * a.w)), j = (int)(p % (uint32_t)(2 * a.w));
    const double east = linspace_at(a.x_min, a.x_max, 2 * a.w, j), north = linspace_at(a.y_max, a.y_min, 2 * a.h, i);     // :329
    const double alt = (double)a.dsm[source_cell(a, p)];                                                                   // :334
    double lon, lat, x, y;
    utm_inverse(a.utm, a.beta, east, north, lon, lat);                                                                     // :337-339
    const RpcModel& r = a.rpc;                                                                                             // :420-432
    project_n(r, (lat - r.lat_offset) / r.lat_scale, (lon - r.lon_offset) / r.lon_scale, (alt - r.alt_offset) / r.alt_scale, x, y);
    const double col = x * r.col_scale + r.col_offset, row = y * r.row_scale + r.row_offset;
    if (!(col >= 0.0 && col < (double)a.out_w && row >= 0.0 && row < (double)a.out_h)) return;                            // :342-344, NaN fails
    atomicMax(a.winner + (size_t)(int)row * a.out_w + (int)col, p + 1u);                                                   // :360
}

__global__ __launch_bounds__(kBlock) void k_prior_resolve(PriorArgs a) {
    const long q = (long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= (long)a.out_h * a.out_w) return;
    const uint32_t win = a.winner[q];
    const size_t cell = win ? source_cell(a, win - 1u) : 0;
    if (a.raster) {
        float v = win ? a.values[cell] : __builtin_nanf("");
        if (a.nan_fill && isnan(v)) v = -1.0f;                                         // datasets/satellite.py:679
        a.raster[q] = v;
    }
    if (a.depth) {
        const double alt = win ? (double)a.dsm[cell] : __builtin_nan("");
        const float* ray = a.rays + (size_t)q * a.stride;
        const double an = (alt - (double)a.z_offset) / (double)a.z_scale;              // datasets/satellite.py:648
        double depth = (an - (double)ray[2]) / (double)ray[5];                          // :650
        if (isnan(depth)) depth = -1.0;                                                // :653
        a.depth[q] = (float)depth;
    }
}

bool image_ok(int out_h, int out_w) { return out_h >= 1 && out_w >= 1 && out_h <= 32767 && out_w <= 32767; }
unsigned blocks_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int eonerf_prior_version(void) { return EONERF_PRIOR_VERSION; }

size_t eonerf_prior_workspace_bytes(int out_h, int out_w) {
    return image_ok(out_h, out_w) ? (size_t)out_h * out_w * sizeof(uint32_t) : 0;
}

int eonerf_prior_reproject(const float* dsm, const float* values, int h, int w, const double bounds[4], const eonerf_rpc* rpc,
                           int utm_zone, int south, int out_h, int out_w, float* raster_out, int raster_nan_to_minus_one,
                           const float* rays, int ray_stride, float z_offset, float z_scale, float* depth_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!dsm || !bounds || !rpc || !workspace || h < 1 || w < 1 || out_h < 1 || out_w < 1 || utm_zone < 1 || utm_zone > 60) return EONERF_E_ARG;
    if (!raster_out && !depth_out) return EONERF_E_ARG;
    if (depth_out && (!rays || ray_stride < 6 || !(z_scale != 0.f) || !isfinite(z_scale) || !isfinite(z_offset))) return EONERF_E_ARG;
    for (int k = 0; k < 4; ++k)
        if (!isfinite(bounds[k])) return EONERF_E_ARG;
    if ((uintptr_t)workspace & 3) return EONERF_E_ARG;
    if (!image_ok(out_h, out_w)) return EONERF_E_UNSUPPORTED;                      // the reference's astype(np.int16) wraps beyond
    const uint64_t points = (uint64_t)4 * (uint64_t)h * (uint64_t)w;
    if (points >= 0xffffffffull) return EONERF_E_UNSUPPORTED;                       // index + 1 must fit the uint32 winner
    if (workspace_bytes < eonerf_prior_workspace_bytes(out_h, out_w)) return EONERF_E_WORKSPACE;
    static_assert(sizeof(eonerf_rpc) == sizeof(RpcModel), "RPC struct mismatch");
    PriorArgs a;
    memcpy(&a.rpc, rpc, sizeof(RpcModel));
    a.utm = eo_utm_params(utm_zone, south);
    eo_krueger_beta(a.beta);
    a.dsm = dsm; a.values = values ? values : dsm;
    a.h = h; a.w = w; a.out_h = out_h; a.out_w = out_w;
    a.x_min = fmin(bounds[0], bounds[2]); a.x_max = fmax(bounds[0], bounds[2]);     // sat_utils.py:318-321
    a.y_min = fmin(bounds[1], bounds[3]); a.y_max = fmax(bounds[1], bounds[3]);
    a.winner = (uint32_t*)workspace;
    a.raster = raster_out; a.nan_fill = raster_nan_to_minus_one;
    a.rays = rays; a.stride = ray_stride; a.z_offset = z_offset; a.z_scale = z_scale; a.depth = depth_out;
    const size_t pixels = (size_t)out_h * out_w;
    HIP_TRY(hipMemsetAsync(a.winner, 0, pixels * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_prior_splat, dim3(blocks_for(points)), dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_prior_resolve, dim3(blocks_for(pixels)), dim3(kBlock), 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
