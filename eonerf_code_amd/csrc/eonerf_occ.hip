// Occupancy grid (include/eonerf_occ.h): the update of all r^3 cells -- one sample point per cell, the context's density-only chain
// over chunks of at most OCC_CHUNK cells, occs = max(occs * decay, sigma * step), the mean as a fixed-order fp64 sum (the two-kernel
// pattern of eonerf_metrics.hip), the bit field packed by wave ballots -- the 27-neighbour dilation, and the entry points that hand a
// grid to the sampler (the culling itself: cull_by_grid, eonerf_rays.hip).  Built with -ffp-contract=off: the point arithmetic is the
// unfused one the header states.
#include "eonerf_ctx.h"
#include "eonerf_rays_dev.h"
#include "../../include/eonerf_occ.h"

namespace {

struct OccPointArgs {
    int r, base, n, p_pad;          // cells base .. base + n - 1 of the grid go to slots 0 .. n - 1 of the pass
    int jitter; uint64_t seed; uint32_t call;
    float *px, *py, *pz; int* simg; int* n_pts;
    float* points_out;              // [r^3][3] or nullptr
};

EO_DEV float occ_coord(int i, float u, int r) {      // ((i + u) / r) * 2 - 1
    return __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn((float)i, u), (float)r), 2.0f), 1.0f);
}

// what k_points_to_soa leaves for the chain (SoA positions, image 0, the sample count, zeroed slots up to the next multiple of 256),
// with the points formed here instead of read
__global__ __launch_bounds__(256) void k_occ_points(OccPointArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *a.n_pts = a.n;
    if (i >= a.p_pad) return;
    if (i < a.n) {
        const int c = a.base + i;
        const int iz = c % a.r, iy = (c / a.r) % a.r, ix = c / (a.r * a.r);
        float u[4] = {0.5f, 0.5f, 0.5f, 0.5f};
        if (a.jitter) philox_u4(a.seed, (uint32_t)c, 0u, 3u, a.call, u);
        const float x = occ_coord(ix, u[0], a.r), y = occ_coord(iy, u[1], a.r), z = occ_coord(iz, u[2], a.r);
        a.px[i] = x; a.py[i] = y; a.pz[i] = z; a.simg[i] = 0;
        if (a.points_out) { float* o = a.points_out + 3 * (size_t)c; o[0] = x; o[1] = y; o[2] = z; }
    } else if (i < ((a.n + 255) & ~255)) {
        a.px[i] = 0.f; a.py[i] = 0.f; a.pz[i] = 0.f; a.simg[i] = 0;
    }
}

__global__ __launch_bounds__(256) void k_occ_value(const float* __restrict__ sigma, int n, float step_size, float decay, float* __restrict__ occs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    occs[i] = fmaxf(__fmul_rn(occs[i], decay), __fmul_rn(sigma[i], step_size));
}

// sum over the workgroup in a fixed order: lanes by shuffle, then the four waves in order; valid in thread 0
EO_DEV double block_sum(double s, double* lds) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}
__global__ __launch_bounds__(256) void k_occ_partial(const float* __restrict__ occs, int n, double* __restrict__ partial) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += OCC_SUM_BLOCKS * 256) acc += (double)occs[c];      // (a fixed grid: the order does not depend on n)
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void k_occ_final(const double* __restrict__ partial, int n, float occ_thre, double* __restrict__ result, float* thr_out) {
    static_assert(OCC_SUM_BLOCKS == 256, "one partial per thread");
    __shared__ double lds[4];
    const double s = block_sum(partial[threadIdx.x], lds);
    if (threadIdx.x != 0) return;
    const double mean = s / (double)n;
    const float thr = fminf((float)mean, occ_thre);
    result[0] = mean;
    reinterpret_cast<float*>(result + 1)[0] = thr;
    if (thr_out) *thr_out = thr;
}

// 64 cells per wave -> one ballot -> two words, written by lane 0.  Every lane of every wave takes part in the ballot; cells beyond the
// grid vote zero, so the unused bits of the last word are zero; words beyond the field are not written
EO_DEV void store_ballot(bool on, int cell0, int n_words, uint32_t* bits) {
    const unsigned long long m = __ballot(on);
    if ((threadIdx.x & 63) == 0) {
        const int w = cell0 >> 5;
        if (w < n_words) bits[w] = (uint32_t)m;
        if (w + 1 < n_words) bits[w + 1] = (uint32_t)(m >> 32);
    }
}
__global__ __launch_bounds__(256) void k_occ_bits(const float* __restrict__ occs, int n, const double* __restrict__ result, uint32_t* __restrict__ bits) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const float thr = reinterpret_cast<const float*>(result + 1)[0];
    store_ballot(c < n && occs[c] > thr, c & ~63, (n + 31) >> 5, bits);
}
__global__ __launch_bounds__(256) void k_occ_dilate(const uint32_t* __restrict__ in, int r, int n, uint32_t* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (c < n) {
        const int iz = c % r, iy = (c / r) % r, ix = c / (r * r);
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    const int x = ix + dx, y = iy + dy, z = iz + dz;
                    if (x < 0 || y < 0 || z < 0 || x >= r || y >= r || z >= r) continue;      // the cube border is clipped
                    const uint32_t q = (uint32_t)((x * r + y) * r + z);
                    on = on || ((in[q >> 5] >> (q & 31)) & 1u);
                }
    }
    store_ballot(on, c & ~63, (n + 31) >> 5, out);
}

inline bool occ_r_ok(int r) { return r >= 1 && r <= EONERF_OCC_MAX_RESOLUTION; }

}  // namespace

extern "C" {

int eonerf_occ_version(void) { return EONERF_OCC_VERSION; }

size_t eonerf_occ_workspace_bytes(const eonerf_ctx* ctx, int r) {
    if (!ctx || !occ_r_ok(r)) return 0;
    return carve_occ(carve_cfg(ctx), nullptr, r).bytes;
}

int eonerf_occ_update(eonerf_ctx* ctx, const float* flat, float* occs, uint32_t* bits, int r, float step_size, float decay,
                      float occ_thre, int jitter, uint32_t seed_call, float* points_out, float* thr_out,
                      void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ctx || !flat || !occs || !bits || !ws) return EONERF_E_ARG;
    if (!ctx->weights_set) return EONERF_E_STATE;
    if (!occ_r_ok(r)) return EONERF_E_UNSUPPORTED;
    const OccWs w = carve_occ(carve_cfg(ctx), ws, r);
    if (ws_bytes < w.bytes) return EONERF_E_WORKSPACE;
    drop_presample(ctx, ws);
    const int n_cells = (int)occ_cells(r);
    for (int base = 0; base < n_cells; base += OCC_CHUNK) {
        const int n = std::min(OCC_CHUNK, n_cells - base);
        OccPointArgs pa;
        pa.r = r; pa.base = base; pa.n = n; pa.p_pad = w.p_cap;
        pa.jitter = jitter ? 1 : 0; pa.seed = ctx->noise_seed; pa.call = seed_call;
        pa.px = w.b.px; pa.py = w.b.py; pa.pz = w.b.pz; pa.simg = w.b.simg; pa.n_pts = w.b.n_pts;
        pa.points_out = points_out;
        hipLaunchKernelGGL(k_occ_points, dim3((w.p_cap + 255) / 256), dim3(256), 0, st, pa);
        HIP_TRY(hipGetLastError());
        const int rc = eo_run_mlp_fwd(ctx, w.b, flat, w.p_cap, false, 0, st);      // the density-only chain, as eonerf_query_density launches it
        if (rc) return rc;
        hipLaunchKernelGGL(k_occ_value, dim3((n + 255) / 256), dim3(256), 0, st, w.b.sigma, n, step_size, decay, occs + base);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_occ_partial, dim3(OCC_SUM_BLOCKS), dim3(256), 0, st, occs, n_cells, w.partial);
    hipLaunchKernelGGL(k_occ_final, dim3(1), dim3(256), 0, st, w.partial, n_cells, occ_thre, w.result, thr_out);
    hipLaunchKernelGGL(k_occ_bits, dim3((n_cells + 255) / 256), dim3(256), 0, st, occs, n_cells, w.result, bits);
    return (int)hipGetLastError();
}

int eonerf_occ_dilate(const uint32_t* bits_in, uint32_t* bits_out, int r, void* stream) {
    if (!bits_in || !bits_out || bits_in == bits_out) return EONERF_E_ARG;
    if (!occ_r_ok(r)) return EONERF_E_UNSUPPORTED;
    const int n_cells = (int)occ_cells(r);
    hipLaunchKernelGGL(k_occ_dilate, dim3((n_cells + 255) / 256), dim3(256), 0, (hipStream_t)stream, bits_in, r, n_cells, bits_out);
    return (int)hipGetLastError();
}

int eonerf_set_occupancy(eonerf_ctx* ctx, const uint32_t* bits, int r) {
    if (!ctx) return EONERF_E_ARG;
    if (bits && !occ_r_ok(r)) return EONERF_E_UNSUPPORTED;
    ctx->occ_bits = bits; ctx->occ_r = bits ? r : 0;
    return EONERF_OK;
}

int eonerf_occ_sample_rays(eonerf_ctx* ctx, const float* rays, const float* zsteps, const float* u, int perturb, int n_rays,
                           const uint32_t* bits, int r, int64_t* ray_indices, float* t_starts, float* t_ends, float* pts_per_ray,
                           int* n_dev, void* ws, size_t ws_bytes, void* stream) {
    if (!bits) return EONERF_E_ARG;
    if (!occ_r_ok(r)) return EONERF_E_UNSUPPORTED;
    return eo_sample_rays(ctx, rays, zsteps, u, perturb, n_rays, bits, r, ray_indices, t_starts, t_ends, pts_per_ray, n_dev, ws, ws_bytes, stream);
}

}  // extern "C"
