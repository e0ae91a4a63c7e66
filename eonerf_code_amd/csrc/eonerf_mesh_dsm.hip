// include/eonerf_mesh_dsm.h: a triangle mesh rasterised straight from above into a DSM, a face raster and attribute rasters.
// The rule is stated once, in eonerf_mesh_dsm_check.h; the kernels here decide only who evaluates it where.
//
// k_mdsm_raster: a wave takes 64 consecutive triangles, every lane sets one up.  The real workload is millions of triangles of a few
// cells each (a 256^3 extraction on a 512^2 or 1024^2 grid), so a lane whose clamped box has at most EONERF_MESH_DSM_LANE_CELLS cells
// walks it alone.  A larger triangle would stall its wave behind one lane -- two triangles of a coarse mesh can cover millions of cells
// -- so the wave walks those together: the ballot of "large" lanes, one triangle at a time, its setup broadcast from the owning lane
// with shuffles, and the 64 lanes laid over the box as a tw x (64 / tw) tile (tw the power of two that fits the box's width, so that
// narrow boxes waste few lanes and wide ones write whole rows).  Every covered (cell, triangle) pair is one 64-bit atomic maximum.
// k_mdsm_resolve / k_mdsm_attributes are element-wise over the cells.  The counters take one atomic add per wave.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_mesh_dsm.h"
#include "eonerf_mesh_dsm_check.h"

namespace {

constexpr int kWave = 64;
static_assert(kMdsmBlock % kWave == 0, "whole waves");

struct RasterArgs {
    MdsmGrid g;
    const float* vertices; long long n_vertices;
    const int32_t* triangles; long long n_triangles;
    unsigned long long* keys;
    unsigned long long* counts;
};

__device__ inline void count_wave(bool flag, unsigned long long* counter, int lane) {
    const unsigned long long m = __ballot(flag);
    if (m != 0 && lane == (int)__builtin_ctzll(m)) atomicAdd(counter, (unsigned long long)__builtin_popcountll(m));
}

__device__ inline void put_key(unsigned long long* keys, const MdsmGrid& g, const MdsmTri& t, uint32_t face, int i, int j) {
    const uint64_t key = mdsm_sample(t, face, i, j);
    if (key != 0) atomicMax(keys + (size_t)j * (size_t)g.xsize + (size_t)i, (unsigned long long)key);
}

__device__ inline int64_t shfl_i64(int64_t v, int src) { return (int64_t)__shfl((long long)v, src, kWave); }

__global__ __launch_bounds__(kMdsmBlock) void k_mdsm_raster(RasterArgs a) {
    const int lane = (int)(threadIdx.x % kWave);
    const long long f = (long long)blockIdx.x * kMdsmBlock + threadIdx.x;        // a wave's 64 triangles are consecutive
    MdsmTri t;
    t.state = -1;                                                              // beyond the mesh: nothing to do and nothing to count
    t.i0 = t.j0 = 0; t.i1 = t.j1 = -1;
    if (f < a.n_triangles) t = mdsm_setup(a.g, a.vertices, a.n_vertices, a.triangles + (size_t)f * 3);
    count_wave(t.state == MDSM_KEEP, a.counts + 0, lane);
    count_wave(t.state == MDSM_DROPPED, a.counts + 1, lane);
    count_wave(t.state == MDSM_DEGENERATE, a.counts + 2, lane);
    const int64_t cells = t.state == MDSM_KEEP ? mdsm_box_cells(t) : 0;
    if (cells > 0 && cells <= kMdsmLaneCells) {
        for (int j = t.j0; j <= t.j1; ++j)
            for (int i = t.i0; i <= t.i1; ++i) put_key(a.keys, a.g, t, (uint32_t)f, i, j);
    }
    unsigned long long large = __ballot(cells > kMdsmLaneCells);               // the same in every lane
    while (large != 0) {
        const int src = (int)__builtin_ctzll(large);
        large &= large - 1;
        MdsmTri b;
        for (int k = 0; k < 3; ++k) {
            b.X[k] = shfl_i64(t.X[k], src);
            b.Y[k] = shfl_i64(t.Y[k], src);
            b.z[k] = __shfl(t.z[k], src, kWave);
        }
        b.area = shfl_i64(t.area, src);
        b.sign = __shfl(t.sign, src, kWave);
        b.state = MDSM_KEEP;
        b.i0 = __shfl(t.i0, src, kWave); b.i1 = __shfl(t.i1, src, kWave);
        b.j0 = __shfl(t.j0, src, kWave); b.j1 = __shfl(t.j1, src, kWave);
        const uint32_t face = (uint32_t)(f - lane + src);
        const int bw = b.i1 - b.i0 + 1;
        const int shift = bw > 32 ? 6 : bw > 16 ? 5 : bw > 8 ? 4 : 3;          // tile width 64, 32, 16 or 8; height 1, 2, 4 or 8
        const int tw = 1 << shift, th = kWave >> shift;
        const int lx = lane & (tw - 1), ly = lane >> shift;
        for (int j = b.j0 + ly; j <= b.j1; j += th)
            for (int i = b.i0 + lx; i <= b.i1; i += tw) put_key(a.keys, a.g, b, face, i, j);
    }
}

__global__ __launch_bounds__(kMdsmBlock) void k_mdsm_resolve(const unsigned long long* keys, long long n, float* dsm, int32_t* face,
                                                             unsigned long long* covered) {
    const long long c = (long long)blockIdx.x * kMdsmBlock + threadIdx.x;
    const unsigned long long key = c < n ? keys[c] : 0ull;
    if (c < n) {
        dsm[c] = key != 0 ? mdsm_key_altitude(key) : __int_as_float(0x7fc00000);
        if (face) face[c] = key != 0 ? mdsm_key_face(key) : -1;
    }
    count_wave(key != 0, covered, (int)(threadIdx.x % kWave));
}

struct AttrArgs {
    MdsmGrid g;
    const float* vertices; long long n_vertices;
    const int32_t* triangles; long long n_triangles;
    const int32_t* face; const float* attr; int channels; float* out;
};

__global__ __launch_bounds__(kMdsmBlock) void k_mdsm_attributes(AttrArgs a) {
    const long long n = (long long)a.g.xsize * a.g.ysize;
    const long long c = (long long)blockIdx.x * kMdsmBlock + threadIdx.x;
    if (c >= n) return;
    float* out = a.out + (size_t)c * a.channels;
    const float nan = __int_as_float(0x7fc00000);
    const int32_t f = a.face[c];
    bool ok = f >= 0 && (long long)f < a.n_triangles;
    MdsmTri t;
    int64_t w[3] = {0, 0, 0};
    const int32_t* tri = a.triangles + (size_t)(ok ? f : 0) * 3;
    if (ok) {
        t = mdsm_setup(a.g, a.vertices, a.n_vertices, tri);                     // checks the three indices before it reads a vertex
        ok = t.state == MDSM_KEEP && mdsm_weights(t, (int)(c % a.g.xsize), (int)(c / a.g.xsize), w);
    }
    if (!ok) {
        for (int k = 0; k < a.channels; ++k) out[k] = nan;
        return;
    }
    const float* a0 = a.attr + (size_t)tri[0] * a.channels;
    const float* a1 = a.attr + (size_t)tri[1] * a.channels;
    const float* a2 = a.attr + (size_t)tri[2] * a.channels;
    for (int k = 0; k < a.channels; ++k) out[k] = (float)mdsm_interpolate(w, t.area, (double)a0[k], (double)a1[k], (double)a2[k]);
}

unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

MdsmGrid grid_of(const double* scale, const double* offset, double xoff, double yoff, int xsize, int ysize, double res) {
    MdsmGrid g;
    for (int c = 0; c < 3; ++c) { g.scale[c] = scale[c]; g.offset[c] = offset[c]; }
    g.xoff = xoff; g.yoff = yoff; g.res = res; g.xsize = xsize; g.ysize = ysize;
    return g;
}

}  // namespace

extern "C" {

int eonerf_mesh_dsm_version(void) { return EONERF_MESH_DSM_VERSION; }

int eonerf_mesh_dsm_rasterize(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const double scale[3],
                              const double offset[3], double xoff, double yoff, int xsize, int ysize, double res, uint64_t* keys, float* dsm,
                              int32_t* face, int64_t* counts_dev, void* stream) {
    const int rc = mdsm_check_rasterize(vertices, n_vertices, triangles, n_triangles, scale, offset, xoff, yoff, xsize, ysize, res, keys, dsm,
                                        counts_dev);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)xsize * ysize;
    hipError_t e = hipMemsetAsync(keys, 0, (size_t)n * sizeof(uint64_t), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    RasterArgs a;
    a.g = grid_of(scale, offset, xoff, yoff, xsize, ysize, res);
    a.vertices = vertices; a.n_vertices = (long long)n_vertices; a.triangles = triangles; a.n_triangles = (long long)n_triangles;
    a.keys = (unsigned long long*)keys; a.counts = (unsigned long long*)counts_dev;
    if (n_triangles > 0) hipLaunchKernelGGL(k_mdsm_raster, dim3(blocks_of(a.n_triangles, kMdsmBlock)), dim3(kMdsmBlock), 0, s, a);
    hipLaunchKernelGGL(k_mdsm_resolve, dim3(blocks_of(n, kMdsmBlock)), dim3(kMdsmBlock), 0, s, (const unsigned long long*)keys, n, dsm, face,
                       (unsigned long long*)(counts_dev + 3));
    return (int)hipGetLastError();
}

int eonerf_mesh_dsm_attributes(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const double scale[3],
                               const double offset[3], double xoff, double yoff, int xsize, int ysize, double res, const int32_t* face,
                               const float* attr, int channels, float* out, void* stream) {
    const int rc = mdsm_check_attributes(vertices, n_vertices, triangles, n_triangles, scale, offset, xoff, yoff, xsize, ysize, res, face, attr,
                                         channels, out);
    if (rc) return rc;
    AttrArgs a;
    a.g = grid_of(scale, offset, xoff, yoff, xsize, ysize, res);
    a.vertices = vertices; a.n_vertices = (long long)n_vertices; a.triangles = triangles; a.n_triangles = (long long)n_triangles;
    a.face = face; a.attr = attr; a.channels = channels; a.out = out;
    hipLaunchKernelGGL(k_mdsm_attributes, dim3(blocks_of((long long)xsize * ysize, kMdsmBlock)), dim3(kMdsmBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
