// DSM evaluation on the device (include/eonerf_dsm.h): nadir virtual camera, point cloud -> raster, NCC registration, MAE.
// Follows eval_eonerf.py:78-95,130-249, datasets/satellite.py:502-533,545-587, dsmr.py and sat_utils.py:181-207,255 of the reference.
// Everything is fp64 except where the reference itself holds fp32 (the rasters, the registered DSM and the error raster).
// Built with -ffp-contract=off: the reference's numpy / numba arithmetic is unfused.
// Reproducibility: the rasteriser adds integers (order-independent); every floating-point sum is a per-workgroup partial written with
// ordinary stores and added in a fixed order by a small second kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_dsm.h"

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

namespace {

constexpr int kBlock = 256;
constexpr int kShifts = 121;        // (2 * irange + 1)^2, irange = 5 (dsmr.py:120)
constexpr int kBandRows = 16;       // rows of ref per workgroup of the NCC passes
constexpr int kMaeBlocks = 256;     // workgroups (and partial sums) of the MAE kernels

// ---------------------------------------------------------------------------------------------------------------- nadir rays
struct NadirArgs {
    int h, w;
    double radius, near, far;
    double d[3], pt_a[3], view[3], sun[3];
    float* rays;
};

__global__ __launch_bounds__(kBlock) void k_nadir_rays(NadirArgs a) {
    const long p = (long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (long)a.h * a.w) return;
    const int i = (int)(p % a.w), j = (int)(p / a.w);
    const double x = ((double)i - a.w * 0.5) / (a.w / a.radius) + a.pt_a[0];                 // eval_eonerf.py:196-199
    const double y = -((double)j - a.h * 0.5) / (a.h / a.radius) + a.pt_a[1];
    const double z = ((-a.d[0] * (x - a.pt_a[0]) - a.d[1] * (y - a.pt_a[1])) / a.d[2]) + a.pt_a[2];
    float* o = a.rays + p * 11;
    o[0] = (float)x; o[1] = (float)y; o[2] = (float)z;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[3 + k] = (float)a.view[k]; o[8 + k] = (float)a.sun[k]; }
    o[6] = (float)a.near;
    o[7] = (float)a.far;
}

void dir_vec_from_el_az(double elevation_deg, double azimuth_deg, const double scale[3], double out[3]) {   // datasets/satellite.py:57-63
    const double d2r = M_PI / 180.0;
    const double el = (90.0 - elevation_deg) * d2r, az = azimuth_deg * d2r;
    out[0] = -1.0 * (sin(az) * cos(el)); out[1] = -1.0 * (cos(az) * cos(el)); out[2] = -1.0 * sin(el);
    double n = 0;
    for (int k = 0; k < 3; ++k) { out[k] /= scale[k]; n += out[k] * out[k]; }
    n = sqrt(n);
    for (int k = 0; k < 3; ++k) out[k] /= n;
}

// ---------------------------------------------------------------------------------------------------------------- rasteriser
struct RasterArgs {
    const float* rays; int stride; const float* depth; long n;
    double scale[3], offset[3], xoff, yoff, res;
    int xsize, ysize;
    unsigned long long* acc_sum; int* acc_cnt;
};

__global__ __launch_bounds__(kBlock) void k_dsm_splat(RasterArgs a) {
    const long r = (long)blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.n) return;
    const double depth = (double)a.depth[r];
    if (!(depth >= 0.0) || !isfinite(depth)) return;                       // :562, and NaN / inf
    const float* ray = a.rays + r * a.stride;
    double xyz[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) xyz[k] = ((double)ray[k] + (double)ray[3 + k] * depth) * a.scale[k] + a.offset[k];
    if (!isfinite(xyz[0]) || !isfinite(xyz[1]) || !(fabs(xyz[2]) < 2147483648.0)) return;
    if (xyz[1] < 0) xyz[1] += 10e6;                                        // :560
    const double fi = floor((xyz[0] - a.xoff) / a.res), fj = floor((a.yoff - xyz[1]) / a.res);
    if (!(fi >= -1.0 && fi <= (double)a.xsize && fj >= -1.0 && fj <= (double)a.ysize)) return;      // the window cannot reach the grid
    const int ci = (int)fi, cj = (int)fj;
    const unsigned long long q = (unsigned long long)llrint(xyz[2] * 65536.0);     // two's complement: unsigned adds wrap like signed ones
    for (int dj = -1; dj <= 1; ++dj) {
        const int j = cj + dj;
        if (j < 0 || j >= a.ysize) continue;
        for (int di = -1; di <= 1; ++di) {
            const int i = ci + di;
            if (i < 0 || i >= a.xsize) continue;
            const size_t c = (size_t)j * a.xsize + i;
            atomicAdd(a.acc_sum + c, q);
            atomicAdd(a.acc_cnt + c, 1);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_dsm_finalize(const int64_t* acc_sum, const int* acc_cnt, long cells, float* dsm) {
    const long c = (long)blockIdx.x * kBlock + threadIdx.x;
    if (c >= cells) return;
    const int n = acc_cnt[c];
    dsm[c] = n > 0 ? (float)((double)acc_sum[c] / 65536.0 / (double)n) : __builtin_nanf("");
}

__global__ __launch_bounds__(kBlock) void k_mask_water(float* sec, int sec_w, const uint8_t* water, int water_w, int h, int w) {
    const long p = (long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (long)h * w) return;
    const int j = (int)(p / w), i = (int)(p % w);
    if (water[(size_t)j * water_w + i]) sec[(size_t)j * sec_w + i] = __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------------------- registration
template <typename T>
__device__ __forceinline__ double valnan(const T* u, int h, int w, int i, int j) {      // dsmr.py:7-13
    return (i >= 0 && j >= 0 && i < w && j < h) ? (double)u[(size_t)j * w + i] : __builtin_nan("");
}

// dsmr.py:17-39.  out[J,I] is what the LAST (j, i) with j//2 == J, i//2 == I wrote: the 2x2 window at (min(2J+1, h-1), min(2I+1, w-1)).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_downsample2x(const T* u, int h, int w, double* out, int oh, int ow) {
    const long p = (long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (long)oh * ow) return;
    const int J = (int)(p / ow), I = (int)(p % ow);
    const int j = min(2 * J + 1, h - 1), i = min(2 * I + 1, w - 1);
    double v = 0;
    int count = 0;
    for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 2; ++l) {
            const double t = valnan(u, h, w, i + k, j + l);
            if (isfinite(t)) { v = v + t; ++count; }
        }
    out[p] = count > 0 ? v / count : __builtin_nan("");
}

// sum of three doubles over the workgroup in a fixed order: lanes by shuffle, then the four waves in order; valid in thread 0
__device__ __forceinline__ void block_sum3(double s[3], double (*lds)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) lds[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) s[k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
}

struct NccArgs {
    const void *u, *v;
    int uh, uw, vh, vw, bands;
    const int* coarse;      // the coarser level's (dx, dy) in device memory, or nullptr at the coarsest level (centre 0, 0)
    double* partial;        // [kShifts][bands][3]
    double* stats;          // [kShifts][3] = muu, muv, count (written by k_ncc_means)
};

// grid (bands, 121).  PASS 1: count, sum u, sum v over the pairs that are both finite (dsmr.py:63-73); PASS 2: the centred sums (:75-83)
template <typename T, int PASS>
__global__ __launch_bounds__(kBlock) void k_ncc_pass(NccArgs a) {
    __shared__ double lds[4][3];
    const int s = blockIdx.y;
    const int cx = a.coarse ? 2 * a.coarse[0] : 0, cy = a.coarse ? 2 * a.coarse[1] : 0;
    const int dx = cx + s % 11 - 5, dy = cy + s / 11 - 5;
    const T *u = (const T*)a.u, *v = (const T*)a.v;
    const int j0 = blockIdx.x * kBandRows, rows = min(kBandRows, a.uh - j0);
    const double muu = PASS == 2 ? a.stats[s * 3] : 0.0, muv = PASS == 2 ? a.stats[s * 3 + 1] : 0.0;
    double acc[3] = {0, 0, 0};
    for (int idx = threadIdx.x; idx < rows * a.uw; idx += kBlock) {
        const int j = j0 + idx / a.uw, i = idx % a.uw;
        const double vu = (double)u[(size_t)j * a.uw + i] - muu;
        const double vv = valnan(v, a.vh, a.vw, i + dx, j + dy) - muv;
        if (isfinite(vu) && isfinite(vv)) {
            if (PASS == 1) { acc[0] += vu; acc[1] += vv; acc[2] += 1.0; }
            else { acc[0] += vu * vu; acc[1] += vv * vv; acc[2] += vu * vv; }
        }
    }
    block_sum3(acc, lds);
    if (threadIdx.x == 0) {
        double* p = a.partial + ((size_t)s * a.bands + blockIdx.x) * 3;
        p[0] = acc[0]; p[1] = acc[1]; p[2] = acc[2];
    }
}

__global__ __launch_bounds__(128) void k_ncc_means(NccArgs a) {
    const int s = threadIdx.x;
    if (s >= kShifts) return;
    double su = 0, sv = 0, n = 0;
    for (int b = 0; b < a.bands; ++b) {
        const double* p = a.partial + ((size_t)s * a.bands + b) * 3;
        su += p[0]; sv += p[1]; n += p[2];
    }
    a.stats[s * 3] = su / n; a.stats[s * 3 + 1] = sv / n; a.stats[s * 3 + 2] = n;      // 0 / 0 = NaN: no pair, no score
}

// scores of the 121 shifts, the argmax of compute_ncc (dsmr.py:102-117) and, at level 0, the result of compute_shift (:185-190)
__global__ __launch_bounds__(128) void k_ncc_pick(NccArgs a, int* shift, double* scores, int scaling, double* out4) {
    __shared__ double sc[kShifts], sgu[kShifts], sgv[kShifts];
    const int s = threadIdx.x;
    if (s < kShifts) {
        double uu = 0, vv = 0, uv = 0;
        for (int b = 0; b < a.bands; ++b) {
            const double* p = a.partial + ((size_t)s * a.bands + b) * 3;
            uu += p[0]; vv += p[1]; uv += p[2];
        }
        const double n = a.stats[s * 3 + 2];
        sgu[s] = sqrt(uu / n); sgv[s] = sqrt(vv / n);
        sc[s] = (uv / n) / (sgu[s] * sgv[s]);
        scores[s] = sc[s];
    }
    __syncthreads();
    if (s != 0) return;
    const int cx = a.coarse ? 2 * a.coarse[0] : 0, cy = a.coarse ? 2 * a.coarse[1] : 0;
    int best = kShifts / 2;                     // the centre: what compute_ncc returns when no score beats -inf
    double maxv = -INFINITY;
    for (int k = 0; k < kShifts; ++k)
        if (sc[k] > maxv) { maxv = sc[k]; best = k; }
    const int dx = cx + best % 11 - 5, dy = cy + best / 11 - 5;
    shift[0] = dx; shift[1] = dy;
    if (out4) {
        const double aa = scaling ? sgu[best] / sgv[best] : 1.0;
        out4[0] = dx; out4[1] = dy; out4[2] = aa;
        out4[3] = a.stats[best * 3] - a.stats[best * 3 + 1] * aa;
    }
}

// workspace of eonerf_dsm_register
struct Level { int uh, uw, vh, vw; size_t shift, scores, u, v; };
constexpr int kMaxLevels = 32;
struct RegLayout { int n; Level l[kMaxLevels]; size_t stats, partial, bytes; };

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

RegLayout reg_layout(int uh, int uw, int vh, int vw) {
    RegLayout r;
    r.n = 0;
    size_t off = 0;
    const int bands0 = (uh + kBandRows - 1) / kBandRows;
    for (;;) {
        Level& L = r.l[r.n++];
        L.uh = uh; L.uw = uw; L.vh = vh; L.vw = vw;
        L.shift = off; off += 16;
        L.scores = off; off = align16(off + kShifts * sizeof(double));
        if (!(min(uh, uw) > 100) || r.n == kMaxLevels) break;       // dsmr.py:125
        uh = (uh + 1) / 2; uw = (uw + 1) / 2; vh = (vh + 1) / 2; vw = (vw + 1) / 2;
    }
    r.stats = off; off = align16(off + kShifts * 3 * sizeof(double));
    r.partial = off; off = align16(off + (size_t)kShifts * bands0 * 3 * sizeof(double));
    r.l[0].u = r.l[0].v = (size_t)-1;
    for (int k = 1; k < r.n; ++k) {
        r.l[k].u = off; off = align16(off + (size_t)r.l[k].uh * r.l[k].uw * sizeof(double));
        r.l[k].v = off; off = align16(off + (size_t)r.l[k].vh * r.l[k].vw * sizeof(double));
    }
    r.bytes = off;
    return r;
}

bool raster_ok(int h, int w) { return h >= 1 && w >= 1 && (long)h * w < (1L << 31); }
unsigned blocks_for(long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ---------------------------------------------------------------------------------------------------------------- MAE
struct MaeArgs {
    const float *gt, *sec; const uint8_t* water;
    int gt_h, gt_w, sec_h, sec_w, water_h, water_w, h, w;
    const double* tr;       // dx, dy, a, b
    double* minmax;         // [kMaeBlocks][2]
    double* sums;           // [kMaeBlocks][2] = sum |err|, count
    float* err;
};

__global__ __launch_bounds__(kBlock) void k_gt_minmax(MaeArgs a) {
    __shared__ float lmin[kBlock], lmax[kBlock];
    float mn = INFINITY, mx = -INFINITY;
    const long cells = (long)a.gt_h * a.gt_w;
    for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < cells; p += (long)kMaeBlocks * kBlock) {
        const float g = a.gt[p];
        if (isfinite(g)) { mn = fminf(mn, g); mx = fmaxf(mx, g); }
    }
    lmin[threadIdx.x] = mn; lmax[threadIdx.x] = mx;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            lmin[threadIdx.x] = fminf(lmin[threadIdx.x], lmin[threadIdx.x + off]);
            lmax[threadIdx.x] = fmaxf(lmax[threadIdx.x], lmax[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { a.minmax[blockIdx.x * 2] = lmin[0]; a.minmax[blockIdx.x * 2 + 1] = lmax[0]; }
}

__global__ __launch_bounds__(kBlock) void k_mae_err(MaeArgs a) {
    static_assert(kMaeBlocks == kBlock, "one partial per thread below");
    __shared__ float lmin[kBlock], lmax[kBlock];
    __shared__ double lds[4][3];
    lmin[threadIdx.x] = (float)a.minmax[threadIdx.x * 2]; lmax[threadIdx.x] = (float)a.minmax[threadIdx.x * 2 + 1];
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            lmin[threadIdx.x] = fminf(lmin[threadIdx.x], lmin[threadIdx.x + off]);
            lmax[threadIdx.x] = fmaxf(lmax[threadIdx.x], lmax[threadIdx.x + off]);
        }
        __syncthreads();
    }
    const float lo = lmin[0] - 10.f, hi = lmax[0] + 10.f;                  // sat_utils.py:203-205, fp32 as the rasters
    const int dx = (int)a.tr[0], dy = (int)a.tr[1];
    const double ca = a.tr[2], cb = a.tr[3];
    double acc[3] = {0, 0, 0};
    const long cells = (long)a.h * a.w;
    for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < cells; p += (long)kMaeBlocks * kBlock) {
        const int j = (int)(p / a.w), i = (int)(p % a.w);
        const int jj = j + dy, ii = i + dx;
        double v = __builtin_nan("");
        if (ii >= 0 && jj >= 0 && ii < a.sec_w && jj < a.sec_h) {
            v = (double)a.sec[(size_t)jj * a.sec_w + ii];
            if (a.water && jj < a.water_h && ii < a.water_w && a.water[(size_t)jj * a.water_w + ii]) v = __builtin_nan("");
        }
        float r = (float)(ca * v + cb);                                    // dsmr.py:147 into the fp32 raster
        r = r < lo ? lo : (r > hi ? hi : r);                               // np.clip: NaN stays NaN
        const float e = r - a.gt[(size_t)j * a.gt_w + i];
        if (a.err) a.err[p] = e;
        if (!isnan(e)) { acc[0] += fabs((double)e); acc[1] += 1.0; }
    }
    block_sum3(acc, lds);
    if (threadIdx.x == 0) { a.sums[blockIdx.x * 2] = acc[0]; a.sums[blockIdx.x * 2 + 1] = acc[1]; }
}

__global__ void k_mae_final(const double* sums, double* out2) {
    double s = 0, n = 0;
    for (int b = 0; b < kMaeBlocks; ++b) { s += sums[b * 2]; n += sums[b * 2 + 1]; }
    out2[0] = s / n;
    out2[1] = n;
}

template <typename T>
int ncc_level(NccArgs a, int* shift, double* scores, int scaling, double* out4, hipStream_t st) {
    const dim3 grid(a.bands, kShifts);
    hipLaunchKernelGGL((k_ncc_pass<T, 1>), grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_ncc_means, dim3(1), dim3(128), 0, st, a);
    hipLaunchKernelGGL((k_ncc_pass<T, 2>), grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_ncc_pick, dim3(1), dim3(128), 0, st, a, shift, scores, scaling, out4);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int eonerf_dsm_version(void) { return EONERF_DSM_VERSION; }

int eonerf_nadir_rays(int h, int w, double radius, double elevation_deg, double azimuth_deg, double near, double far,
                      const double scene_scale[3], double sun_elevation_deg, double sun_azimuth_deg, float* rays, void* stream) {
    if (!raster_ok(h, w) || !scene_scale || !rays || !(radius != 0.0) || !isfinite(radius)) return EONERF_E_ARG;
    for (int k = 0; k < 3; ++k)
        if (!(scene_scale[k] != 0.0) || !isfinite(scene_scale[k])) return EONERF_E_ARG;
    NadirArgs a;
    a.h = h; a.w = w; a.radius = radius; a.near = near; a.far = far; a.rays = rays;
    dir_vec_from_el_az(elevation_deg, azimuth_deg, scene_scale, a.d);                  // eval_eonerf.py:168-170
    if (a.d[2] == 0.0) return EONERF_E_ARG;                                             // a horizontal camera has no plane equation in z
    const double pt_o[3] = {0.0, 0.0, -1.0};
    double n = 0;
    for (int k = 0; k < 3; ++k) { a.pt_a[k] = pt_o[k] - radius * a.d[k]; n += a.d[k] * a.d[k]; }       // :180-181
    n = sqrt(n);
    for (int k = 0; k < 3; ++k) a.view[k] = a.d[k] / n;                                 // :238
    dir_vec_from_el_az(sun_elevation_deg, sun_azimuth_deg, scene_scale, a.sun);         // :90-93
    hipLaunchKernelGGL(k_nadir_rays, dim3(blocks_for((long)h * w)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int eonerf_dsm_rasterize(const float* rays, int ray_stride, const float* depth, long n, const double scale[3], const double offset[3],
                         double xoff, double yoff, int xsize, int ysize, double res,
                         int64_t* acc_sum, int32_t* acc_cnt, float* dsm, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || (n > 0 && (!rays || !depth)) || ray_stride < 6 || !scale || !offset || !acc_sum || !acc_cnt || !dsm) return EONERF_E_ARG;
    if (!raster_ok(ysize, xsize) || !(res > 0.0) || !isfinite(res) || !isfinite(xoff) || !isfinite(yoff)) return EONERF_E_ARG;
    if (n > (1L << 40)) return EONERF_E_UNSUPPORTED;
    const long cells = (long)xsize * ysize;
    HIP_TRY(hipMemsetAsync(acc_sum, 0, cells * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(acc_cnt, 0, cells * sizeof(int32_t), st));
    if (n > 0) {
        RasterArgs a;
        a.rays = rays; a.stride = ray_stride; a.depth = depth; a.n = n;
        for (int k = 0; k < 3; ++k) { a.scale[k] = scale[k]; a.offset[k] = offset[k]; }
        a.xoff = xoff; a.yoff = yoff; a.res = res; a.xsize = xsize; a.ysize = ysize;
        a.acc_sum = (unsigned long long*)acc_sum; a.acc_cnt = acc_cnt;
        hipLaunchKernelGGL(k_dsm_splat, dim3(blocks_for(n)), dim3(kBlock), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_dsm_finalize, dim3(blocks_for(cells)), dim3(kBlock), 0, st, acc_sum, acc_cnt, cells, dsm);
    return (int)hipGetLastError();
}

int eonerf_dsm_mask_water(float* sec, int sec_h, int sec_w, const uint8_t* water, int water_h, int water_w, void* stream) {
    if (!sec || !water || !raster_ok(sec_h, sec_w) || !raster_ok(water_h, water_w)) return EONERF_E_ARG;
    const int h = min(sec_h, water_h), w = min(sec_w, water_w);
    hipLaunchKernelGGL(k_mask_water, dim3(blocks_for((long)h * w)), dim3(kBlock), 0, (hipStream_t)stream, sec, sec_w, water, water_w, h, w);
    return (int)hipGetLastError();
}

size_t eonerf_dsm_register_workspace_bytes(int ref_h, int ref_w, int sec_h, int sec_w) {
    if (!raster_ok(ref_h, ref_w) || !raster_ok(sec_h, sec_w)) return 0;
    return reg_layout(ref_h, ref_w, sec_h, sec_w).bytes;
}

int eonerf_dsm_register_levels(int ref_h, int ref_w) {
    if (!raster_ok(ref_h, ref_w)) return EONERF_E_ARG;
    return reg_layout(ref_h, ref_w, 1, 1).n;
}

int eonerf_dsm_register_level(int ref_h, int ref_w, int sec_h, int sec_w, int level, int dims[4], size_t offs[4]) {
    if (!raster_ok(ref_h, ref_w) || !raster_ok(sec_h, sec_w) || !dims || !offs) return EONERF_E_ARG;
    const RegLayout r = reg_layout(ref_h, ref_w, sec_h, sec_w);
    if (level < 0 || level >= r.n) return EONERF_E_ARG;
    const Level& L = r.l[level];
    dims[0] = L.uh; dims[1] = L.uw; dims[2] = L.vh; dims[3] = L.vw;
    offs[0] = L.shift; offs[1] = L.scores; offs[2] = L.u; offs[3] = L.v;
    return EONERF_OK;
}

int eonerf_dsm_register(const float* ref, int ref_h, int ref_w, const float* sec, int sec_h, int sec_w, int scaling,
                        double* out4, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ref || !sec || !out4 || !workspace || !raster_ok(ref_h, ref_w) || !raster_ok(sec_h, sec_w)) return EONERF_E_ARG;
    if ((uintptr_t)workspace & 15) return EONERF_E_ARG;
    const RegLayout r = reg_layout(ref_h, ref_w, sec_h, sec_w);
    if (workspace_bytes < r.bytes) return EONERF_E_WORKSPACE;
    char* ws = (char*)workspace;
    // pyramid, fine to coarse (dsmr.py:126-127)
    for (int k = 1; k < r.n; ++k) {
        const Level &f = r.l[k - 1], &c = r.l[k];
        double *cu = (double*)(ws + c.u), *cv = (double*)(ws + c.v);
        if (k == 1) {
            hipLaunchKernelGGL(k_downsample2x<float>, dim3(blocks_for((long)c.uh * c.uw)), dim3(kBlock), 0, st, ref, f.uh, f.uw, cu, c.uh, c.uw);
            hipLaunchKernelGGL(k_downsample2x<float>, dim3(blocks_for((long)c.vh * c.vw)), dim3(kBlock), 0, st, sec, f.vh, f.vw, cv, c.vh, c.vw);
        } else {
            hipLaunchKernelGGL(k_downsample2x<double>, dim3(blocks_for((long)c.uh * c.uw)), dim3(kBlock), 0, st, (const double*)(ws + f.u), f.uh, f.uw, cu, c.uh, c.uw);
            hipLaunchKernelGGL(k_downsample2x<double>, dim3(blocks_for((long)c.vh * c.vw)), dim3(kBlock), 0, st, (const double*)(ws + f.v), f.vh, f.vw, cv, c.vh, c.vw);
        }
        HIP_TRY(hipGetLastError());
    }
    // search, coarse to fine: each level reads the coarser level's shift from the workspace (:128-134)
    for (int k = r.n - 1; k >= 0; --k) {
        const Level& L = r.l[k];
        NccArgs a;
        a.u = k ? (const void*)(ws + L.u) : (const void*)ref;
        a.v = k ? (const void*)(ws + L.v) : (const void*)sec;
        a.uh = L.uh; a.uw = L.uw; a.vh = L.vh; a.vw = L.vw;
        a.bands = (L.uh + kBandRows - 1) / kBandRows;
        a.coarse = k + 1 < r.n ? (const int*)(ws + r.l[k + 1].shift) : nullptr;
        a.partial = (double*)(ws + r.partial);
        a.stats = (double*)(ws + r.stats);
        int* shift = (int*)(ws + L.shift);
        double* scores = (double*)(ws + L.scores);
        const int rc = k ? ncc_level<double>(a, shift, scores, scaling, nullptr, st) : ncc_level<float>(a, shift, scores, scaling, out4, st);
        if (rc) return rc;
    }
    return EONERF_OK;
}

size_t eonerf_dsm_mae_workspace_bytes(void) { return (size_t)kMaeBlocks * 4 * sizeof(double); }

int eonerf_dsm_mae(const float* gt, int gt_h, int gt_w, const float* sec, int sec_h, int sec_w,
                   const uint8_t* water, int water_h, int water_w, const double* transform4,
                   double* out2, float* err, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!gt || !sec || !transform4 || !out2 || !workspace || !raster_ok(gt_h, gt_w) || !raster_ok(sec_h, sec_w)) return EONERF_E_ARG;
    if (water && !raster_ok(water_h, water_w)) return EONERF_E_ARG;
    if ((uintptr_t)workspace & 7) return EONERF_E_ARG;
    if (workspace_bytes < eonerf_dsm_mae_workspace_bytes()) return EONERF_E_WORKSPACE;
    MaeArgs a;
    a.gt = gt; a.sec = sec; a.water = water;
    a.gt_h = gt_h; a.gt_w = gt_w; a.sec_h = sec_h; a.sec_w = sec_w; a.water_h = water_h; a.water_w = water_w;
    a.h = min(gt_h, sec_h); a.w = min(gt_w, sec_w);                        // sat_utils.py:201-202
    a.tr = transform4;
    a.minmax = (double*)workspace; a.sums = a.minmax + kMaeBlocks * 2;
    a.err = err;
    hipLaunchKernelGGL(k_gt_minmax, dim3(kMaeBlocks), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_mae_err, dim3(kMaeBlocks), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_mae_final, dim3(1), dim3(1), 0, st, a.sums, out2);
    return (int)hipGetLastError();
}

}  // extern "C"
