// Mesh export on the device (include/eonerf_mesh.h): marching tetrahedra over the Kuhn split of every cell of a sampled volume.
// count = classify + scan, emit = one thread per lattice point writing its own vertices and its own cell's triangles at the scanned
// offsets.  The rule itself (table, classification, vertex, triangle order) is in eonerf_mesh_check.h; this file is the launches.
// Built with -ffp-contract=off, and the coordinate arithmetic uses the _rn intrinsics: vertices are bit-pinned.
// Cost: every kernel is memory bound.  Consecutive lanes take consecutive x, so the eight corner reads of a wave are eight coalesced
// rows of which seven are another wave's own row (cache hits): the volume comes from memory once per pass.  classify writes 5 bytes per
// point; emit reads them back only around the surface's cells.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_mesh.h"
#include "eonerf_mesh_check.h"

namespace {

__constant__ MeshTable kTable = mesh_make_table();

struct MeshWs { uint16_t* lv; uint16_t* lt; uint8_t* mask; uint2* l1; uint2* l2; uint2* l3; };

MeshWs carve_of(void* workspace, const MeshCarve& c) {
    char* b = (char*)workspace;
    MeshWs w;
    w.lv = (uint16_t*)(b + c.lv_off); w.lt = (uint16_t*)(b + c.lt_off); w.mask = (uint8_t*)(b + c.mask_off);
    w.l1 = (uint2*)(b + c.l1_off); w.l2 = (uint2*)(b + c.l2_off); w.l3 = (uint2*)(b + c.l3_off);
    return w;
}

// Exclusive scan of one tile: element r * kMeshBlock + tid of the tile is val[r] of thread tid.  Both components at once.
// One barrier; called once per kernel, so the shared array is never reused.
__device__ inline void scan_tile(const uint2 (&val)[kMeshRounds], uint2 (&excl)[kMeshRounds], uint2& total) {
    constexpr int kWaves = kMeshBlock / 64;
    __shared__ uint2 wave_total[kMeshRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint2 inc[kMeshRounds];
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        uint2 v = val[r];
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned a = __shfl_up(v.x, o, 64), b = __shfl_up(v.y, o, 64);
            if (lane >= o) { v.x += a; v.y += b; }
        }
        inc[r] = v;
        if (lane == 63) wave_total[r][wave] = v;
    }
    __syncthreads();
    uint2 run = make_uint2(0u, 0u);
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        uint2 mine = run;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            const uint2 t = wave_total[r][w];
            run.x += t.x; run.y += t.y;
        }
        excl[r] = make_uint2(mine.x + inc[r].x - val[r].x, mine.y + inc[r].y - val[r].y);
    }
    total = run;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_classify(const float* f, int nx, int ny, int nz, unsigned n, float level, MeshWs w,
                                                              unsigned long long* nonfinite) {
    const unsigned base = blockIdx.x * (unsigned)kMeshTile;
    uint2 val[kMeshRounds], excl[kMeshRounds], total;
    unsigned mask[kMeshRounds], nf = 0;
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        val[r] = make_uint2(0u, 0u);
        mask[r] = 0;
        if (p < n) {
            const unsigned q = p / (unsigned)nx;
            const int i = (int)(p - q * (unsigned)nx), j = (int)(q % (unsigned)ny), k = (int)(q / (unsigned)ny);
            const MeshPoint c = mesh_classify(kTable, f, nx, ny, nz, i, j, k, p, level);
            val[r] = make_uint2((unsigned)__popc(c.mask), c.triangles);
            mask[r] = c.mask;
            nf += c.nonfinite;
        }
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        if (p < n) {
            w.lv[p] = (uint16_t)excl[r].x;
            w.lt[p] = (uint16_t)excl[r].y;
            w.mask[p] = (uint8_t)mask[r];
        }
    }
    if (threadIdx.x == 0) w.l1[blockIdx.x] = total;
    // the one counter that is not part of the scan: a sum, so the order of the adds does not matter
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_down(nf, o, 64);
    if ((threadIdx.x & 63) == 0 && nf) atomicAdd(nonfinite, (unsigned long long)nf);
}

// data[0 .. n) -> its exclusive scan inside each tile, in place; sums[tile] = the tile's total
__global__ __launch_bounds__(kMeshBlock) void k_mesh_scan(uint2* data, unsigned n, uint2* sums) {
    const unsigned base = blockIdx.x * (unsigned)kMeshTile;
    uint2 val[kMeshRounds], excl[kMeshRounds], total;
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        val[r] = p < n ? data[p] : make_uint2(0u, 0u);
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kMeshRounds; ++r) {
        const unsigned p = base + r * kMeshBlock + threadIdx.x;
        if (p < n) data[p] = excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[p] += offs[p / tile]; the grand total goes to counts[0], counts[1]
__global__ __launch_bounds__(kMeshBlock) void k_mesh_add(uint2* data, unsigned n, const uint2* offs, const uint2* grand, long long* counts) {
    const unsigned p = blockIdx.x * (unsigned)kMeshBlock + threadIdx.x;
    if (p < n) {
        const uint2 o = offs[p / (unsigned)kMeshTile];
        uint2 v = data[p];
        v.x += o.x; v.y += o.y;
        data[p] = v;
    }
    if (p == 0) { counts[0] = (long long)grand->x; counts[1] = (long long)grand->y; }
}

struct EmitArgs {
    const float* f; int nx, ny, nz; unsigned n; float level;
    float origin[3], spacing[3];
    const uint16_t* lv; const uint16_t* lt; const uint8_t* mask; const uint2* l1;
    float* vertices; long long cap_v; int32_t* triangles; unsigned long long cap_t; long long* key; int* status;
};

struct IdOf {
    const EmitArgs& a; unsigned p, nxy;
    __device__ int32_t operator()(int corner, int slot) const {
        const unsigned q = p + mesh_corner_offset(corner, (unsigned)a.nx, nxy);
        return (int32_t)(a.l1[q / (unsigned)kMeshTile].x + a.lv[q] + (unsigned)__popc((unsigned)a.mask[q] & ((1u << slot) - 1u)));
    }
};
struct Put {
    const EmitArgs& a; bool* overflow;
    __device__ void operator()(uint64_t at, int32_t v0, int32_t v1, int32_t v2) const {
        if (at < a.cap_t) {
            int32_t* t = a.triangles + (size_t)at * 3;
            t[0] = v0; t[1] = v1; t[2] = v2;
        } else {
            *overflow = true;
        }
    }
};

__global__ __launch_bounds__(kMeshBlock) void k_mesh_emit(EmitArgs a) {
    const unsigned p = blockIdx.x * (unsigned)kMeshBlock + threadIdx.x;
    if (p >= a.n) return;
    const unsigned nxy = (unsigned)a.nx * (unsigned)a.ny;
    const unsigned q = p / (unsigned)a.nx;
    const int i = (int)(p - q * (unsigned)a.nx), j = (int)(q % (unsigned)a.ny), k = (int)(q / (unsigned)a.ny);
    bool overflow = false;
    const unsigned mask = a.mask[p];
    if (mask) {
        const unsigned first = a.l1[p / (unsigned)kMeshTile].x + a.lv[p];
        for (int s = 0; s < 7; ++s) {
            if (!((mask >> s) & 1)) continue;
            const long long id = (long long)(first + (unsigned)__popc(mask & ((1u << s) - 1u)));
            if (id >= a.cap_v) { overflow = true; continue; }
            float v[3];
            mesh_vertex(a.f, a.nx, a.ny, i, j, k, p, s, a.level, a.origin, a.spacing, v);
            float* out = a.vertices + (size_t)id * 3;
            out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
            if (a.key) a.key[id] = (long long)p * 8 + s;
        }
    }
    if (i + 1 < a.nx && j + 1 < a.ny && k + 1 < a.nz) {
        unsigned in8 = 0;
        for (int c = 0; c < 8; ++c)
            if (a.f[p + mesh_corner_offset(c, (unsigned)a.nx, nxy)] >= a.level) in8 |= 1u << c;
        if (in8 != 0 && in8 != 0xffu) {
            const uint64_t tri0 = (uint64_t)a.l1[p / (unsigned)kMeshTile].y + a.lt[p];
            mesh_cell_triangles(kTable, in8, tri0, IdOf{a, p, nxy}, Put{a, &overflow});
        }
    }
    if (overflow) atomicOr(a.status, EONERF_MESH_STATUS_CAPACITY);
}

struct LatticeArgs { float origin[3], spacing[3]; int nx, ny, z0; unsigned n; float* out; };

__global__ __launch_bounds__(kMeshBlock) void k_mesh_lattice(LatticeArgs a) {
    const unsigned p = blockIdx.x * (unsigned)kMeshBlock + threadIdx.x;
    if (p >= a.n) return;
    const unsigned q = p / (unsigned)a.nx;
    const int i = (int)(p - q * (unsigned)a.nx), j = (int)(q % (unsigned)a.ny), k = a.z0 + (int)(q / (unsigned)a.ny);
    float* o = a.out + (size_t)p * 3;
    o[0] = mesh_position(a.origin[0], a.spacing[0], i, 0.f);
    o[1] = mesh_position(a.origin[1], a.spacing[1], j, 0.f);
    o[2] = mesh_position(a.origin[2], a.spacing[2], k, 0.f);
}

inline unsigned blocks_of(uint64_t n, int per) { return (unsigned)((n + per - 1) / per); }     // n <= 2^28: at most 2^20 workgroups

}  // namespace

extern "C" {

int eonerf_mesh_version(void) { return EONERF_MESH_VERSION; }

size_t eonerf_mesh_workspace_bytes(int nx, int ny, int nz) {
    const uint64_t n = mesh_points(nx, ny, nz);
    return n ? mesh_carve(n).bytes : 0;
}

int eonerf_mesh_lattice_points(const float origin[3], const float spacing[3], int nx, int ny, int z0, int nz, float* xyz_out, void* stream) {
    const int rc = mesh_check_lattice(origin, spacing, nx, ny, z0, nz, xyz_out);
    if (rc != EONERF_OK) return rc;
    LatticeArgs a;
    for (int c = 0; c < 3; ++c) { a.origin[c] = origin[c]; a.spacing[c] = spacing[c]; }
    a.nx = nx; a.ny = ny; a.z0 = z0; a.n = (unsigned)mesh_slab_points(nx, ny, z0, nz); a.out = xyz_out;
    hipLaunchKernelGGL(k_mesh_lattice, dim3(blocks_of(a.n, kMeshBlock)), dim3(kMeshBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int eonerf_mesh_count(const float* f, int nx, int ny, int nz, float level, int64_t* counts_dev, void* workspace, size_t workspace_bytes,
                      void* stream) {
    const int rc = mesh_check_count(f, nx, ny, nz, level, counts_dev, workspace, workspace_bytes);
    if (rc != EONERF_OK) return rc;
    const MeshCarve c = mesh_carve(mesh_points(nx, ny, nz));
    const MeshWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)c.n1), dim3(kMeshBlock), 0, s, f, nx, ny, nz, (unsigned)c.n, level, w,
                       (unsigned long long*)(counts_dev + 2));
    hipLaunchKernelGGL(k_mesh_scan, dim3((unsigned)c.n2), dim3(kMeshBlock), 0, s, w.l1, (unsigned)c.n1, w.l2);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMeshBlock), 0, s, w.l2, (unsigned)c.n2, w.l3);
    hipLaunchKernelGGL(k_mesh_add, dim3(blocks_of(c.n1, kMeshBlock)), dim3(kMeshBlock), 0, s, w.l1, (unsigned)c.n1, (const uint2*)w.l2,
                       (const uint2*)w.l3, (long long*)counts_dev);
    return (int)hipGetLastError();
}

int eonerf_mesh_emit(const float* f, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3],
                     const void* workspace, size_t workspace_bytes, float* vertices, int64_t cap_v, int32_t* triangles, int64_t cap_t,
                     int64_t* vertex_key, int32_t* status_dev, void* stream) {
    const int rc = mesh_check_emit(f, nx, ny, nz, level, origin, spacing, workspace, workspace_bytes, vertices, cap_v, triangles, cap_t, status_dev);
    if (rc != EONERF_OK) return rc;
    const MeshCarve c = mesh_carve(mesh_points(nx, ny, nz));
    const MeshWs w = carve_of(const_cast<void*>(workspace), c);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    EmitArgs a;
    a.f = f; a.nx = nx; a.ny = ny; a.nz = nz; a.n = (unsigned)c.n; a.level = level;
    for (int k = 0; k < 3; ++k) { a.origin[k] = origin[k]; a.spacing[k] = spacing[k]; }
    a.lv = w.lv; a.lt = w.lt; a.mask = w.mask; a.l1 = w.l1;
    a.vertices = vertices; a.cap_v = (long long)cap_v; a.triangles = triangles; a.cap_t = (unsigned long long)cap_t;
    a.key = (long long*)vertex_key; a.status = (int*)status_dev;
    hipLaunchKernelGGL(k_mesh_emit, dim3(blocks_of(c.n, kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
