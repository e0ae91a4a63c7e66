// eonerf_simplify.h: mesh simplification by vertex clustering.  The rule is stated once, in eonerf_simplify_check.h; the kernels here
// decide only who evaluates it where.  Built with -ffp-contract=off, and the coordinate arithmetic uses the _rn intrinsics.
//
// count: k_simp_accumulate (one lane per vertex: quantise, remember the cell id, add 1 and the local coordinates to the cell's sums),
// k_simp_cells (occupancy flags, scanned inside tiles of 1024 cells), k_simp_classify (one lane per triangle: its class from the three
// cell ids, the keep flags scanned inside tiles of 1024 triangles), and over both sets of tile sums the plain blocked scan of
// eonerf_mesh.hip: scan inside tiles level by level up to one sum, then add the offsets back down.  No look-back, no flags.
// emit: k_simp_select (key minimum per vertex, vertex_map), k_simp_place (positions and source of the occupied cells), k_simp_write
// (kept triangles at their scanned offsets).  Every kernel is memory bound and element-wise but for the tile scans.
//
// The hot spots are the two vertex launches: vertices arrive in lattice order, so many lanes of a wave hit the same cell -- with four
// atomic adds each in k_simp_accumulate, with a 64-bit atomic minimum each in k_simp_select.  Runs of equal cell ids in consecutive
// lanes are combined by a segmented shuffle scan and the last lane of a run issues the run's atomics.  Integer sums and a minimum: no
// bit changes.  EONERF_SIMPLIFY_PLAIN=1 in the environment selects the per-lane atomics (the A/B of scripts/simplify_ab.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/eonerf_hip.h"
#include "eonerf_simplify.h"
#include "eonerf_simplify_check.h"

namespace {

constexpr int kWave = 64;
static_assert(kSimpBlock % kWave == 0, "whole waves");

struct SimpWs {
    unsigned* n; unsigned long long* sum; unsigned long long* key; uint16_t* cid; int32_t* vcell; uint16_t* tflag;
    unsigned* lc[kSimpMaxLevels]; unsigned* lt[kSimpMaxLevels];
};

SimpWs carve_of(void* workspace, const SimpCarve& c) {
    char* b = (char*)workspace;
    SimpWs w;
    w.n = (unsigned*)(b + c.n_off); w.sum = (unsigned long long*)(b + c.sum_off); w.key = (unsigned long long*)(b + c.key_off);
    w.cid = (uint16_t*)(b + c.cid_off); w.vcell = (int32_t*)(b + c.vcell_off); w.tflag = (uint16_t*)(b + c.tflag_off);
    for (int k = 0; k < kSimpMaxLevels; ++k) {
        w.lc[k] = k < c.lc.count ? (unsigned*)(b + c.lc.off[k]) : nullptr;
        w.lt[k] = k < c.lt.count ? (unsigned*)(b + c.lt.off[k]) : nullptr;
    }
    return w;
}

// Exclusive scan of one tile: element r * kSimpBlock + tid of the tile is val[r] of thread tid.  One barrier; called once per kernel.
__device__ inline void scan_tile(const unsigned (&val)[kSimpRounds], unsigned (&excl)[kSimpRounds], unsigned& total) {
    constexpr int kWaves = kSimpBlock / kWave;
    __shared__ unsigned wave_total[kSimpRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc[kSimpRounds];
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        unsigned v = val[r];
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned a = __shfl_up(v, o, kWave);
            if (lane >= o) v += a;
        }
        inc[r] = v;
        if (lane == kWave - 1) wave_total[r][wave] = v;
    }
    __syncthreads();
    unsigned run = 0;
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        unsigned mine = run;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) mine = run;
            run += wave_total[r][w];
        }
        excl[r] = mine + inc[r] - val[r];
    }
    total = run;
}

__device__ inline void count_wave(bool flag, unsigned long long* counter, int lane) {
    const unsigned long long m = __ballot(flag);
    if (m != 0 && lane == (int)__builtin_ctzll(m)) atomicAdd(counter, (unsigned long long)__builtin_popcountll(m));
}

struct AccArgs { SimpGrid g; const float* vertices; unsigned n_vertices; unsigned* n; unsigned long long* sum; int32_t* vcell; };

template <bool kAggregate>
__global__ __launch_bounds__(kSimpBlock) void k_simp_accumulate(AccArgs a) {
    const unsigned v = blockIdx.x * (unsigned)kSimpBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x % kWave);
    SimpVertex q;
    q.cell = -1; q.L[0] = q.L[1] = q.L[2] = 0;
    if (v < a.n_vertices) {
        q = simp_vertex(a.g, a.vertices + (size_t)v * 3);
        a.vcell[v] = q.cell;
    }
    unsigned cnt = q.cell >= 0 ? 1u : 0u, sx = (unsigned)q.L[0], sy = (unsigned)q.L[1], sz = (unsigned)q.L[2];
    bool add = q.cell >= 0;
    if (kAggregate) {
        // runs of equal cell ids in consecutive lanes: head = the first lane of mine; an inclusive scan that does not cross a head; the
        // last lane of a run holds its totals (64 local coordinates below 2^14 each: far inside 32 bits)
        const int before = __shfl_up(q.cell, 1, kWave), after = __shfl_down(q.cell, 1, kWave);
        const unsigned long long heads = __ballot(lane == 0 || before != q.cell);
        const int head = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned c = __shfl_up(cnt, o, kWave), x = __shfl_up(sx, o, kWave), y = __shfl_up(sy, o, kWave), z = __shfl_up(sz, o, kWave);
            if (lane - o >= head) { cnt += c; sx += x; sy += y; sz += z; }
        }
        add = add && (lane == kWave - 1 || after != q.cell);
    }
    if (add) {
        atomicAdd(a.n + q.cell, cnt);
        unsigned long long* s = a.sum + (size_t)q.cell * 3;
        atomicAdd(s + 0, (unsigned long long)sx);
        atomicAdd(s + 1, (unsigned long long)sy);
        atomicAdd(s + 2, (unsigned long long)sz);
    }
}

__global__ __launch_bounds__(kSimpBlock) void k_simp_cells(const unsigned* n, unsigned cells, uint16_t* cid, unsigned* sums) {
    const unsigned base = blockIdx.x * (unsigned)kSimpTile;
    unsigned val[kSimpRounds], excl[kSimpRounds], total;
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        const unsigned p = base + r * kSimpBlock + threadIdx.x;
        val[r] = p < cells && n[p] != 0 ? 1u : 0u;
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        const unsigned p = base + r * kSimpBlock + threadIdx.x;
        if (p < cells) cid[p] = (uint16_t)excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSimpBlock) void k_simp_classify(const int32_t* triangles, unsigned n_triangles, const int32_t* vcell, long long n_vertices,
                                                              uint16_t* tflag, unsigned* sums, unsigned long long* counts) {
    const unsigned base = blockIdx.x * (unsigned)kSimpTile;
    const int lane = (int)(threadIdx.x % kWave);
    unsigned val[kSimpRounds], excl[kSimpRounds], total;
    int state[kSimpRounds];
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        const unsigned t = base + r * kSimpBlock + threadIdx.x;
        state[r] = -1;
        if (t < n_triangles) {
            int32_t cells[3];
            state[r] = simp_classify(vcell, n_vertices, triangles + (size_t)t * 3, cells);
        }
        val[r] = state[r] == SIMP_KEEP ? 1u : 0u;
        // dropped triangles are rare; the collapsed ones -- most of a mesh -- are what the scan leaves: T - kept - dropped (k_simp_scan)
        count_wave(state[r] == SIMP_DROPPED, counts + 2, lane);
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        const unsigned t = base + r * kSimpBlock + threadIdx.x;
        if (t < n_triangles) tflag[t] = (uint16_t)(((unsigned)state[r] << 14) | excl[r]);
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[0 .. n) -> its exclusive scan inside each tile, in place; sums[tile] = the tile's total; grand (where given, at the last level):
// grand[0] = that of tile 0 and, where rest_of >= 0, grand[2] = rest_of - grand[0] - grand[1]
__global__ __launch_bounds__(kSimpBlock) void k_simp_scan(unsigned* data, unsigned n, unsigned* sums, long long* grand, long long rest_of) {
    const unsigned base = blockIdx.x * (unsigned)kSimpTile;
    unsigned val[kSimpRounds], excl[kSimpRounds], total;
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        const unsigned p = base + r * kSimpBlock + threadIdx.x;
        val[r] = p < n ? data[p] : 0u;
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kSimpRounds; ++r) {
        const unsigned p = base + r * kSimpBlock + threadIdx.x;
        if (p < n) data[p] = excl[r];
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        if (grand && blockIdx.x == 0) {
            grand[0] = (long long)total;
            if (rest_of >= 0) grand[2] = rest_of - (long long)total - grand[1];
        }
    }
}

// data[p] += offs[p / tile]
__global__ __launch_bounds__(kSimpBlock) void k_simp_add(unsigned* data, unsigned n, const unsigned* offs) {
    const unsigned p = blockIdx.x * (unsigned)kSimpBlock + threadIdx.x;
    if (p < n) data[p] += offs[p / (unsigned)kSimpTile];
}

struct SelectArgs {
    SimpGrid g; const float* vertices; unsigned n_vertices;
    const unsigned* n; const unsigned long long* sum; unsigned long long* key; const uint16_t* cid; const unsigned* l0; const int32_t* vcell;
    int32_t* vertex_map;
};

template <bool kAggregate>
__global__ __launch_bounds__(kSimpBlock) void k_simp_select(SelectArgs a) {
    const unsigned v = blockIdx.x * (unsigned)kSimpBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x % kWave);
    const int32_t cell = v < a.n_vertices ? a.vcell[v] : -1;
    if (v < a.n_vertices && a.vertex_map) a.vertex_map[v] = cell < 0 ? -1 : (int32_t)(a.l0[(unsigned)cell / (unsigned)kSimpTile] + a.cid[cell]);
    unsigned long long key = ~0ull;                            // above every real key (d2 < 2^30)
    if (cell >= 0) {
        const SimpVertex q = simp_vertex(a.g, a.vertices + (size_t)v * 3);
        const unsigned long long* s = a.sum + (size_t)cell * 3;
        const uint64_t S[3] = {s[0], s[1], s[2]};
        key = (unsigned long long)simp_key(q.L, S, a.n[cell], v);
    }
    bool offer = cell >= 0;
    if (kAggregate) {
        // as in k_simp_accumulate: the smallest key of a run of equal cells ends up in the run's last lane, which offers it
        const int before = __shfl_up(cell, 1, kWave), after = __shfl_down(cell, 1, kWave);
        const unsigned long long heads = __ballot(lane == 0 || before != cell);
        const int head = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned long long k = __shfl_up(key, o, kWave);
            if (lane - o >= head && k < key) key = k;
        }
        offer = offer && (lane == kWave - 1 || after != cell);
    }
    if (offer) atomicMin(a.key + cell, key);
}

struct PlaceArgs {
    SimpGrid g; const float* vertices; unsigned n_vertices, cells; int representative;
    const unsigned* n; const unsigned long long* sum; const unsigned long long* key; const uint16_t* cid; const unsigned* l0;
    float* out_vertices; long long cap_vertices; int32_t* source; int* status;
};

__global__ __launch_bounds__(kSimpBlock) void k_simp_place(PlaceArgs a) {
    const unsigned c = blockIdx.x * (unsigned)kSimpBlock + threadIdx.x;
    if (c >= a.cells) return;
    const unsigned n = a.n[c];
    if (n == 0) return;
    const long long id = (long long)(a.l0[c / (unsigned)kSimpTile] + a.cid[c]);
    if (id >= a.cap_vertices) { atomicOr(a.status, EONERF_SIMPLIFY_STATUS_CAPACITY); return; }
    const unsigned src = (unsigned)(a.key[c] & 0xFFFFFFFFull);                 // a vertex of this cell
    float* out = a.out_vertices + (size_t)id * 3;
    if (src >= a.n_vertices) {                                                 // not the mesh the count call saw: read nothing through it
        if (a.source) a.source[id] = -1;
        out[0] = out[1] = out[2] = __int_as_float(0x7fc00000);
        return;
    }
    if (a.source) a.source[id] = (int32_t)src;
    if (a.representative == EONERF_SIMPLIFY_NEAREST) {
        const float* in = a.vertices + (size_t)src * 3;
        out[0] = in[0]; out[1] = in[1]; out[2] = in[2];
    } else {
        const unsigned gx = (unsigned)a.g.dims[0], gy = (unsigned)a.g.dims[1];
        const unsigned r = c / gx;
        const int32_t q[3] = {(int32_t)(c - r * gx), (int32_t)(r % gy), (int32_t)(r / gy)};
        for (int k = 0; k < 3; ++k) out[k] = simp_mean_position(a.g, k, q[k], a.sum[(size_t)c * 3 + k], n);
    }
}

struct WriteArgs {
    const int32_t* triangles; unsigned n_triangles, n_vertices; const int32_t* vcell; const uint16_t* cid; const unsigned* l0c; const uint16_t* tflag;
    const unsigned* l0t; int32_t* out_triangles; unsigned long long cap_triangles; int* status;
};

__global__ __launch_bounds__(kSimpBlock) void k_simp_write(WriteArgs a) {
    const unsigned t = blockIdx.x * (unsigned)kSimpBlock + threadIdx.x;
    if (t >= a.n_triangles) return;
    const unsigned f = a.tflag[t];
    if ((f >> 14) != SIMP_KEEP) return;
    const unsigned long long at = (unsigned long long)a.l0t[t / (unsigned)kSimpTile] + (f & 0x3FFFu);
    if (at >= a.cap_triangles) { atomicOr(a.status, EONERF_SIMPLIFY_STATUS_CAPACITY); return; }
    const int32_t* tri = a.triangles + (size_t)t * 3;           // kept: its three indices are inside the mesh and name kept vertices
    int32_t* out = a.out_triangles + (size_t)at * 3;
    for (int k = 0; k < 3; ++k) {
        const int32_t cell = (unsigned)tri[k] < a.n_vertices ? a.vcell[tri[k]] : -1;      // (-1: not the mesh the count call saw)
        out[k] = cell < 0 ? -1 : (int32_t)(a.l0c[(unsigned)cell / (unsigned)kSimpTile] + a.cid[cell]);
    }
}

// EONERF_SIMPLIFY_PLAIN=1: the two vertex launches with one atomic per lane, without the combination inside the wave (A/B switch)
bool plain_atomics() {
    const char* e = getenv("EONERF_SIMPLIFY_PLAIN");
    return e && atoi(e) != 0;
}

inline unsigned blocks_of(uint64_t n, int per) { return (unsigned)((n + per - 1) / per); }     // n < 2^31: at most 2^23 workgroups

// the levels above the tile sums l[0]: scan up to one sum, add the offsets back down; the grand total goes to grand[0] (and with
// rest_of >= 0 what is neither it nor grand[1] to grand[2])
void scan_levels(const SimpLevels& lv, unsigned* const* l, long long* grand, long long rest_of, hipStream_t s) {
    for (int k = 0; k + 1 < lv.count; ++k)
        hipLaunchKernelGGL(k_simp_scan, dim3((unsigned)lv.m[k + 1]), dim3(kSimpBlock), 0, s, l[k], (unsigned)lv.m[k], l[k + 1],
                           k + 2 == lv.count ? grand : (long long*)nullptr, rest_of);
    for (int k = lv.count - 3; k >= 0; --k)
        hipLaunchKernelGGL(k_simp_add, dim3(blocks_of(lv.m[k], kSimpBlock)), dim3(kSimpBlock), 0, s, l[k], (unsigned)lv.m[k], (const unsigned*)l[k + 1]);
}

}  // namespace

extern "C" {

int eonerf_simplify_version(void) { return EONERF_SIMPLIFY_VERSION; }

size_t eonerf_simplify_workspace_bytes(const int dims[3], int64_t n_vertices, int64_t n_triangles) {
    return simp_workspace_bytes(dims, n_vertices, n_triangles);
}

int eonerf_simplify_count(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const float origin[3],
                          const float cell[3], const int dims[3], void* workspace, size_t workspace_bytes, int64_t* counts_dev, void* stream) {
    const int rc = simp_check_count(vertices, n_vertices, triangles, n_triangles, origin, cell, dims, workspace, workspace_bytes, counts_dev);
    if (rc != EONERF_OK) return rc;
    const SimpCarve c = simp_carve(simp_cells(dims), (uint64_t)n_vertices, (uint64_t)n_triangles);
    const SimpWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(w.n, 0, c.sum_off - c.n_off + (size_t)c.cells * 3 * sizeof(uint64_t), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_vertices > 0) {
        AccArgs a;
        a.g = simp_grid(origin, cell, dims);
        a.vertices = vertices; a.n_vertices = (unsigned)n_vertices; a.n = w.n; a.sum = w.sum; a.vcell = w.vcell;
        if (plain_atomics())
            hipLaunchKernelGGL(k_simp_accumulate<false>, dim3(blocks_of(c.n_vertices, kSimpBlock)), dim3(kSimpBlock), 0, s, a);
        else
            hipLaunchKernelGGL(k_simp_accumulate<true>, dim3(blocks_of(c.n_vertices, kSimpBlock)), dim3(kSimpBlock), 0, s, a);
    }
    hipLaunchKernelGGL(k_simp_cells, dim3((unsigned)c.lc.m[0]), dim3(kSimpBlock), 0, s, (const unsigned*)w.n, (unsigned)c.cells, w.cid, w.lc[0]);
    scan_levels(c.lc, w.lc, (long long*)counts_dev + 0, -1, s);
    if (n_triangles > 0) {
        hipLaunchKernelGGL(k_simp_classify, dim3((unsigned)c.lt.m[0]), dim3(kSimpBlock), 0, s, triangles, (unsigned)n_triangles, (const int32_t*)w.vcell,
                           (long long)n_vertices, w.tflag, w.lt[0], (unsigned long long*)counts_dev);
        scan_levels(c.lt, w.lt, (long long*)counts_dev + 1, (long long)n_triangles, s);      // kept, and collapsed = T - kept - dropped
    }
    return (int)hipGetLastError();
}

int eonerf_simplify_emit(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const float origin[3],
                         const float cell[3], const int dims[3], int representative, void* workspace, size_t workspace_bytes,
                         float* out_vertices, int64_t cap_vertices, int32_t* out_triangles, int64_t cap_triangles, int32_t* source,
                         int32_t* vertex_map, int32_t* status_dev, void* stream) {
    const int rc = simp_check_emit(vertices, n_vertices, triangles, n_triangles, origin, cell, dims, representative, workspace, workspace_bytes,
                                   out_vertices, cap_vertices, out_triangles, cap_triangles, status_dev);
    if (rc != EONERF_OK) return rc;
    const SimpCarve c = simp_carve(simp_cells(dims), (uint64_t)n_vertices, (uint64_t)n_triangles);
    const SimpWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(w.key, 0xFF, (size_t)c.cells * sizeof(uint64_t), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(status_dev, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    const SimpGrid g = simp_grid(origin, cell, dims);
    if (n_vertices > 0) {
        SelectArgs a;
        a.g = g; a.vertices = vertices; a.n_vertices = (unsigned)n_vertices;
        a.n = w.n; a.sum = w.sum; a.key = w.key; a.cid = w.cid; a.l0 = w.lc[0]; a.vcell = w.vcell; a.vertex_map = vertex_map;
        if (plain_atomics())
            hipLaunchKernelGGL(k_simp_select<false>, dim3(blocks_of(c.n_vertices, kSimpBlock)), dim3(kSimpBlock), 0, s, a);
        else
            hipLaunchKernelGGL(k_simp_select<true>, dim3(blocks_of(c.n_vertices, kSimpBlock)), dim3(kSimpBlock), 0, s, a);
        PlaceArgs p;
        p.g = g; p.vertices = vertices; p.n_vertices = (unsigned)n_vertices; p.cells = (unsigned)c.cells; p.representative = representative;
        p.n = w.n; p.sum = w.sum; p.key = w.key; p.cid = w.cid; p.l0 = w.lc[0];
        p.out_vertices = out_vertices; p.cap_vertices = (long long)cap_vertices; p.source = source; p.status = (int*)status_dev;
        hipLaunchKernelGGL(k_simp_place, dim3(blocks_of(c.cells, kSimpBlock)), dim3(kSimpBlock), 0, s, p);
    }
    if (n_triangles > 0) {
        WriteArgs t;
        t.triangles = triangles; t.n_triangles = (unsigned)n_triangles; t.n_vertices = (unsigned)n_vertices; t.vcell = w.vcell; t.cid = w.cid; t.l0c = w.lc[0]; t.tflag = w.tflag;
        t.l0t = w.lt[0]; t.out_triangles = out_triangles; t.cap_triangles = (unsigned long long)cap_triangles; t.status = (int*)status_dev;
        hipLaunchKernelGGL(k_simp_write, dim3(blocks_of(c.n_triangles, kSimpBlock)), dim3(kSimpBlock), 0, s, t);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
