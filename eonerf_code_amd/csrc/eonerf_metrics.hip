// Per-image validation metrics on the device (include/eonerf_metrics.h): metrics.uncertainty_aware_loss (metrics.py:17-22) and
// metrics.mse / psnr (:60-69) of one rendered image in one pass over its rays.
// Everything is fp64 formed from the fp32 inputs.  Built with -ffp-contract=off: the terms are the unfused ones the header states.
// Reproducibility: a fixed grid, every thread adds its rays in increasing order, lanes fold by shuffle, waves and blocks in index order;
// one partial per block through the workspace (plain stores, every slot written by every call), no floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_metrics.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBlocks = 256;        // the fixed grid: the order of summation must not depend on n
constexpr int kSums = 4;            // colour term, log beta, squared error, rays

struct MetricsArgs {
    const float *rgb, *beta, *gt;
    int rgb_stride, beta_stride, gt_stride;
    long n;
    double* partial;                // [kBlocks][kSums]
    double* result;                 // [6]
};

// sum of four doubles over the workgroup in a fixed order: lanes by shuffle, then the four waves in order; valid in thread 0
__device__ __forceinline__ void block_sum4(double s[kSums], double (*lds)[kSums]) {
#pragma unroll
    for (int k = 0; k < kSums; ++k)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kSums; ++k) lds[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < kSums; ++k) s[k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
}

__global__ __launch_bounds__(kBlock) void k_metrics_partial(MetricsArgs a) {
    __shared__ double lds[kBlock / 64][kSums];
    double acc[kSums] = {0, 0, 0, 0};
    for (long r = (long)blockIdx.x * kBlock + threadIdx.x; r < a.n; r += (long)kBlocks * kBlock) {
        const float* p = a.rgb + (size_t)r * a.rgb_stride;
        const float* g = a.gt + (size_t)r * a.gt_stride;
        double den = 0.0;
        if (a.beta) {
            const double b = (double)a.beta[(size_t)r * a.beta_stride];
            den = 2.0 * (b * b);                                           // metrics.py:18
            acc[1] += log(b);                                              // :19
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)p[c] - (double)g[c];
            const double sq = d * d;
            if (a.beta) acc[0] += sq / den;
            acc[2] += sq;                                                  // :61
        }
        acc[3] += 1.0;
    }
    block_sum4(acc, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < kSums; ++k) a.partial[blockIdx.x * kSums + k] = acc[k];
}

__global__ __launch_bounds__(kBlock) void k_metrics_final(MetricsArgs a) {
    static_assert(kBlocks == kBlock, "one partial per thread");
    __shared__ double lds[kBlock / 64][kSums];
    double s[kSums];
    for (int k = 0; k < kSums; ++k) s[k] = a.partial[threadIdx.x * kSums + k];
    block_sum4(s, lds);
    if (threadIdx.x != 0) return;
    const double n = s[3], nan = __builtin_nan("");
    const double color = a.beta ? s[0] / (3.0 * n) : nan;
    const double logbeta = a.beta ? (3.0 + s[1] / n) / 2.0 : nan;          // :19
    const double mse = s[2] / (3.0 * n);
    a.result[0] = color + logbeta;                                         // :20
    a.result[1] = color;
    a.result[2] = logbeta;
    a.result[3] = mse;
    a.result[4] = -10.0 * log10(mse);                                      // :69
    a.result[5] = n;
}

}  // namespace

extern "C" {

int eonerf_metrics_version(void) { return EONERF_METRICS_VERSION; }

size_t eonerf_metrics_workspace_bytes(void) { return (size_t)kBlocks * kSums * sizeof(double); }

int eonerf_image_metrics(const float* rgb, int rgb_stride, const float* beta, int beta_stride, const float* gt, int gt_stride, long n,
                         double* result, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!rgb || !gt || !result || !workspace || n <= 0) return EONERF_E_ARG;
    if (rgb_stride < 3 || gt_stride < 3 || (beta && beta_stride < 1)) return EONERF_E_ARG;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)result & 7)) return EONERF_E_ARG;
    if (workspace_bytes < eonerf_metrics_workspace_bytes()) return EONERF_E_WORKSPACE;
    MetricsArgs a;
    a.rgb = rgb; a.beta = beta; a.gt = gt;
    a.rgb_stride = rgb_stride; a.beta_stride = beta_stride; a.gt_stride = gt_stride;
    a.n = n;
    a.partial = (double*)workspace; a.result = result;
    hipLaunchKernelGGL(k_metrics_partial, dim3(kBlocks), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_metrics_final, dim3(1), dim3(kBlock), 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
