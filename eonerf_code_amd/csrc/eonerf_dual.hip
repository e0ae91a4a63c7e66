// Dual contouring on the device (eonerf_dual.h): one vertex per surface cell from the Hermite data of its edges, one quad per
// sign-changing axis edge.  count = classify + scan; hermite = one thread per lattice point writing its own crossing points; emit =
// one workgroup per scan tile: quads of its points, then the tile's active cells gathered into a dense list and solved side by side.
// The rule itself (classification, the fp64 solve, the ring of a quad) is in eonerf_dual_check.h; this file is the launches.
// Built with -ffp-contract=off, and the arithmetic uses the _rn intrinsics: vertices are bit-pinned.
// Cost: classify and hermite are memory bound like their marching-tetrahedra twins (the volume comes from memory once per pass;
// classify writes 7 bytes per point).  emit reads those 7 bytes per point and touches the volume and the gradient table only around
// the surface; active cells are a few per cent of a tile, so without the dense list a wave would run the ~150 dependent fp64
// operations of a solve with one or two lanes alive.  The blocked scan is eonerf_mesh.hip's, restated over four sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "eonerf_dual.h"
#include "eonerf_dual_check.h"

namespace {

struct DualWs { uint16_t* lh; uint16_t* lc; uint16_t* lq; uint8_t* info; uint4* l1; uint4* l2; uint4* l3; };

DualWs carve_of(void* workspace, const DualCarve& c) {
    char* b = (char*)workspace;
    DualWs w;
    w.lh = (uint16_t*)(b + c.lh_off); w.lc = (uint16_t*)(b + c.lc_off); w.lq = (uint16_t*)(b + c.lq_off); w.info = (uint8_t*)(b + c.info_off);
    w.l1 = (uint4*)(b + c.l1_off); w.l2 = (uint4*)(b + c.l2_off); w.l3 = (uint4*)(b + c.l3_off);
    return w;
}

__device__ inline uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline uint4 sub4(uint4 a, uint4 b) { return make_uint4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// Exclusive scan of one tile: element r * kMeshBlock + tid of the tile is val[r] of thread tid.  All four components at once.
// One barrier; called once per kernel, so the shared array is never reused.
__device__ inline void scan_tile(const uint4 (&val)[kMeshRounds], uint4 (&excl)[kMeshRounds], uint4& total) {
    constexpr int kWaves = kMeshBlock / 64;
    __shared__ uint4 wave_total[kMeshRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 inc[kMeshRounds];
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        uint4 v = val[r];
        for (int o = 1; o < 64; o <<= 1) {
            const uint4 u = make_uint4(__shfl_up(v.x, o, 64), __shfl_up(v.y, o, 64), __shfl_up(v.z, o, 64), __shfl_up(v.w, o, 64));
            if (lane >= o) v = add4(v, u);
        }
        inc[r] = v;
        if (lane == 63) wave_total[r][wave] = v;
    }
    __syncthreads();
    uint4 run = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        uint4 mine = run;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            run = add4(run, wave_total[r][w]);
        }
        excl[r] = sub4(add4(mine, inc[r]), val[r]);
    }
    total = run;
}

__device__ inline void point_of(unsigned p, int nx, int ny, int& i, int& j, int& k) {
    const unsigned q = p / (unsigned)nx;
    i = (int)(p - q * (unsigned)nx); j = (int)(q % (unsigned)ny); k = (int)(q / (unsigned)ny);
}

__global__ __launch_bounds__(kMeshBlock) void k_dual_classify(const float* f, int nx, int ny, int nz, unsigned n, float level, DualWs w) {
    const unsigned base = blockIdx.x * (unsigned)kMeshTile;
    uint4 val[kMeshRounds], excl[kMeshRounds], total;
    unsigned info[kMeshRounds];
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        val[r] = make_uint4(0u, 0u, 0u, 0u);
        info[r] = 0;
        if (p < n) {
            int i, j, k;
            point_of(p, nx, ny, i, j, k);
            const DualPoint c = dual_classify(f, nx, ny, nz, i, j, k, p, level);
            val[r] = make_uint4((unsigned)__popc(c.mask), c.active, c.quads, c.nonfinite);
            info[r] = dual_info(c);
        }
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        if (p < n) {
            w.lh[p] = (uint16_t)excl[r].x;
            w.lc[p] = (uint16_t)excl[r].y;
            w.lq[p] = (uint16_t)excl[r].z;
            w.info[p] = (uint8_t)info[r];
        }
    }
    if (threadIdx.x == 0) w.l1[blockIdx.x] = total;
}

// data[0 .. n) -> its exclusive scan inside each tile, in place; sums[tile] = the tile's total
__global__ __launch_bounds__(kMeshBlock) void k_dual_scan(uint4* data, unsigned n, uint4* sums) {
    const unsigned base = blockIdx.x * (unsigned)kMeshTile;
    uint4 val[kMeshRounds], excl[kMeshRounds], total;
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        val[r] = p < n ? data[p] : make_uint4(0u, 0u, 0u, 0u);
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        if (p < n) data[p] = excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[p] += offs[p / tile]; the grand total goes to counts[0 .. 3] (two triangles per quad)
__global__ __launch_bounds__(kMeshBlock) void k_dual_add(uint4* data, unsigned n, const uint4* offs, const uint4* grand, long long* counts) {
    const unsigned p = blockIdx.x * (unsigned)kMeshBlock + threadIdx.x;
    if (p < n) data[p] = add4(data[p], offs[p / (unsigned)kMeshTile]);
    if (p == 0) {
        counts[0] = (long long)grand->x; counts[1] = (long long)grand->y; counts[2] = 2ll * (long long)grand->z; counts[3] = (long long)grand->w;
    }
}

struct DualArgs {
    const float* f; int nx, ny, nz; unsigned n; float level;
    float origin[3], spacing[3];
    const uint16_t* lh; const uint16_t* lc; const uint16_t* lq; const uint8_t* info; const uint4* l1;
    float* points; long long cap_h; long long* point_key;                                               // hermite
    const float* gradient; long long n_gradient; double lambda;                                         // emit
    float* vertices; long long cap_v; long long* cell_key; int32_t* triangles; unsigned long long cap_t; unsigned long long* report;
    int* status;
};

__global__ __launch_bounds__(kMeshBlock) void k_dual_hermite(DualArgs a) {
    const unsigned p = blockIdx.x * (unsigned)kMeshBlock + threadIdx.x;
    if (p >= a.n) return;
    const unsigned mask = a.info[p] & kDualMask;
    if (!mask) return;
    int i, j, k;
    point_of(p, a.nx, a.ny, i, j, k);
    const unsigned first = a.l1[p / (unsigned)kMeshTile].x + a.lh[p];
    bool overflow = false;
    for (int s = 0; s < 3; ++s) {
        if (!((mask >> s) & 1)) continue;
        // (the mask is the workspace's word: an edge is followed only where its far end is inside the lattice)
        if ((s == 0 && i + 1 >= a.nx) || (s == 1 && j + 1 >= a.ny) || (s == 2 && k + 1 >= a.nz)) continue;
        const long long id = (long long)(first + (unsigned)__popc(mask & ((1u << s) - 1u)));
        if (id >= a.cap_h) { overflow = true; continue; }
        float v[3];
        dual_hermite_point(a.f, a.nx, a.ny, i, j, k, p, s, a.level, a.origin, a.spacing, v);
        float* out = a.points + (size_t)id * 3;
        out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
        if (a.point_key) a.point_key[id] = (long long)p * 8 + s;
    }
    if (overflow) atomicOr(a.status, EONERF_DUAL_STATUS_CAPACITY);
}

struct HermiteOf {
    const DualArgs& a;
    __device__ int64_t operator()(unsigned q, int slot) const {
        return (int64_t)(a.l1[q / (unsigned)kMeshTile].x + a.lh[q] + (unsigned)__popc((unsigned)a.info[q] & ((1u << slot) - 1u)));
    }
};
struct VertexOf {
    const DualArgs& a;
    __device__ int32_t operator()(unsigned q) const { return (int32_t)(a.l1[q / (unsigned)kMeshTile].y + a.lc[q]); }
};
struct PutTriangle {
    const DualArgs& a; bool* overflow;
    __device__ void operator()(uint64_t at, int32_t v0, int32_t v1, int32_t v2) const {
        if (at < a.cap_t) {
            int32_t* t = a.triangles + (size_t)at * 3;
            t[0] = v0; t[1] = v1; t[2] = v2;
        } else {
            *overflow = true;
        }
    }
};

__global__ __launch_bounds__(kMeshBlock) void k_dual_emit(DualArgs a) {
    __shared__ uint16_t list[kMeshTile];
    const unsigned tile = blockIdx.x, base = tile * (unsigned)kMeshTile;
    const uint4 first = a.l1[tile];
    bool overflow = false;
    // the quads of this tile's points, and its active cells into the list: the scan inside the tile is a cell's place in it
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        if (p >= a.n) continue;
        const unsigned info = a.info[p];
        if (info & kDualActive) {
            const unsigned at = a.lc[p];
            if (at < (unsigned)kMeshTile) list[at] = (uint16_t)(p - base);
        }
        if (info >> kDualQuadShift) {
            int i, j, k;
            point_of(p, a.nx, a.ny, i, j, k);
            dual_point_quads(info & kDualMask, a.f[p] >= a.level, a.nx, a.ny, a.nz, i, j, k, p, 2 * ((uint64_t)first.z + a.lq[p]), VertexOf{a},
                             PutTriangle{a, &overflow});
        }
    }
    __syncthreads();
    const unsigned last = (base + (unsigned)kMeshTile < a.n ? base + (unsigned)kMeshTile : a.n) - 1u;
    unsigned cells = (unsigned)a.lc[last] + ((a.info[last] & kDualActive) ? 1u : 0u);
    if (cells > (unsigned)kMeshTile) cells = (unsigned)kMeshTile;
    unsigned clamped = 0, fallback = 0, dropped = 0;
    for (unsigned at = threadIdx.x; at < cells; at += (unsigned)kMeshBlock) {
        const unsigned p = base + list[at];
        int i, j, k;
        point_of(p, a.nx, a.ny, i, j, k);
        if (p >= a.n || i + 1 >= a.nx || j + 1 >= a.ny || k + 1 >= a.nz) continue;          // (never with count's own workspace)
        const long long id = (long long)first.y + at;
        if (id >= a.cap_v) { overflow = true; continue; }
        const DualVertex v = dual_cell_vertex(a.f, a.nx, a.ny, p, a.level, a.spacing, a.lambda, a.gradient, (int64_t)a.n_gradient, HermiteOf{a});
        clamped += v.clamped; fallback += v.fallback; dropped += v.dropped;
        if (v.beyond) overflow = true;
        float pos[3];
        dual_vertex_position(v, i, j, k, a.origin, a.spacing, pos);
        float* out = a.vertices + (size_t)id * 3;
        out[0] = pos[0]; out[1] = pos[1]; out[2] = pos[2];
        if (a.cell_key) a.cell_key[id] = (long long)p;
    }
    if (overflow) atomicOr(a.status, EONERF_DUAL_STATUS_CAPACITY);
    // counters: sums, so the order of the adds does not matter
    for (int o = 32; o > 0; o >>= 1) {
        clamped += __shfl_down(clamped, o, 64); fallback += __shfl_down(fallback, o, 64); dropped += __shfl_down(dropped, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (clamped) atomicAdd(a.report, (unsigned long long)clamped);
        if (fallback) atomicAdd(a.report + 1, (unsigned long long)fallback);
        if (dropped) atomicAdd(a.report + 2, (unsigned long long)dropped);
    }
}

inline unsigned blocks_of(uint64_t n, int per) { return (unsigned)((n + per - 1) / per); }     // n <= 2^28: at most 2^20 workgroups

DualArgs args_of(const float* f, int nx, int ny, int nz, float level, const float* origin, const float* spacing, const DualCarve& c, const DualWs& w) {
    DualArgs a = {};
    a.f = f; a.nx = nx; a.ny = ny; a.nz = nz; a.n = (unsigned)c.n; a.level = level;
    for (int k = 0; k < 3; ++k) { a.origin[k] = origin[k]; a.spacing[k] = spacing[k]; }
    a.lh = w.lh; a.lc = w.lc; a.lq = w.lq; a.info = w.info; a.l1 = w.l1;
    return a;
}

}  // namespace

extern "C" {

int eonerf_dual_version(void) { return EONERF_DUAL_VERSION; }

size_t eonerf_dual_workspace_bytes(int nx, int ny, int nz) {
    const uint64_t n = mesh_points(nx, ny, nz);
    return n ? dual_carve(n).bytes : 0;
}

int eonerf_dual_count(const float* f, int nx, int ny, int nz, float level, int64_t* counts_dev, void* workspace, size_t workspace_bytes,
                      void* stream) {
    const int rc = dual_check_count(f, nx, ny, nz, level, counts_dev, workspace, workspace_bytes);
    if (rc != EONERF_OK) return rc;
    const DualCarve c = dual_carve(mesh_points(nx, ny, nz));
    const DualWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dual_classify, dim3((unsigned)c.n1), dim3(kMeshBlock), 0, s, f, nx, ny, nz, (unsigned)c.n, level, w);
    hipLaunchKernelGGL(k_dual_scan, dim3((unsigned)c.n2), dim3(kMeshBlock), 0, s, w.l1, (unsigned)c.n1, w.l2);
    hipLaunchKernelGGL(k_dual_scan, dim3(1), dim3(kMeshBlock), 0, s, w.l2, (unsigned)c.n2, w.l3);
    hipLaunchKernelGGL(k_dual_add, dim3(blocks_of(c.n1, kMeshBlock)), dim3(kMeshBlock), 0, s, w.l1, (unsigned)c.n1, (const uint4*)w.l2,
                       (const uint4*)w.l3, (long long*)counts_dev);
    return (int)hipGetLastError();
}

int eonerf_dual_hermite(const float* f, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3],
                        const void* workspace, size_t workspace_bytes, float* points, int64_t cap_h, int64_t* point_key, int32_t* status_dev,
                        void* stream) {
    const int rc = dual_check_hermite(f, nx, ny, nz, level, origin, spacing, workspace, workspace_bytes, points, cap_h, status_dev);
    if (rc != EONERF_OK) return rc;
    const DualCarve c = dual_carve(mesh_points(nx, ny, nz));
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    DualArgs a = args_of(f, nx, ny, nz, level, origin, spacing, c, carve_of(const_cast<void*>(workspace), c));
    a.points = points; a.cap_h = (long long)cap_h; a.point_key = (long long*)point_key; a.status = (int*)status_dev;
    hipLaunchKernelGGL(k_dual_hermite, dim3(blocks_of(c.n, kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    return (int)hipGetLastError();
}

int eonerf_dual_emit(const float* f, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3], const float* gradient,
                     int64_t n_gradient, float regularisation, const void* workspace, size_t workspace_bytes, float* vertices, int64_t cap_v,
                     int64_t* cell_key, int32_t* triangles, int64_t cap_t, int64_t* report_dev, int32_t* status_dev, void* stream) {
    const int rc = dual_check_emit(f, nx, ny, nz, level, origin, spacing, gradient, n_gradient, regularisation, workspace, workspace_bytes, vertices,
                                   cap_v, triangles, cap_t, report_dev, status_dev);
    if (rc != EONERF_OK) return rc;
    const DualCarve c = dual_carve(mesh_points(nx, ny, nz));
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(report_dev, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    DualArgs a = args_of(f, nx, ny, nz, level, origin, spacing, c, carve_of(const_cast<void*>(workspace), c));
    a.gradient = gradient; a.n_gradient = (long long)n_gradient; a.lambda = (double)regularisation;
    a.vertices = vertices; a.cap_v = (long long)cap_v; a.cell_key = (long long*)cell_key; a.triangles = triangles;
    a.cap_t = (unsigned long long)cap_t; a.report = (unsigned long long*)report_dev; a.status = (int*)status_dev;
    hipLaunchKernelGGL(k_dual_emit, dim3((unsigned)c.n1), dim3(kMeshBlock), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
