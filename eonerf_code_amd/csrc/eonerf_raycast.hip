// eonerf_raycast.h: rays against a triangle mesh through a uniform grid.  The rule is stated once, in eonerf_raycast_check.h; the
// kernels here decide only who evaluates it where.  Built with -ffp-contract=off, and the rule's arithmetic uses the _rn intrinsics.
//
// count: k_rc_count (a lane per triangle: live or dropped, its padded cell range, one 32-bit atomic add per cell; a range of more than
// kRcLaneCells cells is walked by the whole wave -- the ballot of "large" lanes, one triangle at a time, its range broadcast from the
// owning lane with shuffles, as k_mdsm_raster does -- so that two ground-plane triangles on a fine grid do not serialise on one lane).
// build: k_rc_tiles and the plain blocked scan of eonerf_simplify.hip over the cell counts (scan inside tiles level by level up to one
// sum, add the offsets back down; no look-back, no flags), then k_rc_fill, k_rc_count's walk again with an atomic cursor per cell.
// casts: k_rc_closest / k_rc_occluded, a lane per ray: the stepper of eonerf_raycast_check.h, per cell a loop over its list -- three
// indices, three vertices and the rule's test per entry.  The order of entries inside a list depends on arrival; the closest form
// takes a lexicographic minimum and the any-hit form a disjunction, so no output bit does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "eonerf_raycast.h"
#include "eonerf_raycast_check.h"

namespace {

constexpr int kWave = 64;
static_assert(kRcBlock % kWave == 0, "whole waves");

struct RcWs { unsigned* start; unsigned* cursor; unsigned* l[kRcMaxLevels]; unsigned* list; };

RcWs carve_of(const void* workspace, const RcCarve& c) {
    char* b = (char*)workspace;
    RcWs w;
    w.start = (unsigned*)(b + c.start_off); w.cursor = (unsigned*)(b + c.cursor_off); w.list = (unsigned*)(b + c.list_off);
    for (int k = 0; k < kRcMaxLevels; ++k) w.l[k] = k < c.lv.count ? (unsigned*)(b + c.lv.off[k]) : nullptr;
    return w;
}

// Exclusive scan of one tile: element r * kRcBlock + tid of the tile is val[r] of thread tid.  One barrier; called once per kernel.
__device__ inline void scan_tile(const unsigned (&val)[kRcRounds], unsigned (&excl)[kRcRounds], unsigned& total) {
    constexpr int kWaves = kRcBlock / kWave;
    __shared__ unsigned wave_total[kRcRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc[kRcRounds];
#pragma unroll
    for (int r = 0; r < kRcRounds; ++r) {
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
    for (int r = 0; r < kRcRounds; ++r) {
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

struct MeshArgs { RcGrid g; const float* vertices; long long n_vertices; const int32_t* triangles; long long n_triangles; };

// The walk count and fill share: every lane of the wave reaches it (no early return in front of it).  visit(cell, face) runs once per
// (cell of the padded range, live triangle): by the triangle's own lane for a small range, by the wave's lanes in turn for a large one.
// Returns the cells of this lane's triangle (0: beyond the mesh or dropped) and whether it was dropped.
template <class Visit>
__device__ inline int64_t walk_ranges(const MeshArgs& a, bool* dropped, Visit visit) {
    const int lane = (int)(threadIdx.x % kWave);
    const long long f = (long long)blockIdx.x * kRcBlock + threadIdx.x;        // a wave's 64 triangles are consecutive
    int c0[3] = {0, 0, 0}, c1[3] = {-1, -1, -1};
    int64_t cells = 0;
    *dropped = false;
    if (f < a.n_triangles) {
        const int32_t* p = a.triangles + (size_t)f * 3;
        const int32_t tri[3] = {p[0], p[1], p[2]};
        double v[3][3];
        if (rc_live(a.g, a.vertices, a.n_vertices, tri, v)) {
            rc_cell_range(a.g, v, c0, c1);
            cells = rc_range_cells(c0, c1);
        } else {
            *dropped = true;
        }
    }
    if (cells > 0 && cells <= kRcLaneCells)
        for (int64_t k = 0; k < cells; ++k) visit(rc_range_cell(a.g, c0, c1, k), (uint32_t)f);
    unsigned long long large = __ballot(cells > kRcLaneCells);                 // the same in every lane
    while (large != 0) {
        const int src = (int)__builtin_ctzll(large);
        large &= large - 1;
        int b0[3], b1[3];
        for (int c = 0; c < 3; ++c) { b0[c] = __shfl(c0[c], src, kWave); b1[c] = __shfl(c1[c], src, kWave); }
        const int64_t n = rc_range_cells(b0, b1);
        const uint32_t face = (uint32_t)(f - lane + src);
        for (int64_t k = lane; k < n; k += kWave) visit(rc_range_cell(a.g, b0, b1, k), face);
    }
    return cells;
}

__global__ __launch_bounds__(kRcBlock) void k_rc_count(MeshArgs a, unsigned* cnt, unsigned long long* counts) {
    bool dropped;
    const int64_t cells = walk_ranges(a, &dropped, [cnt](uint32_t cell, uint32_t) { atomicAdd(cnt + cell, 1u); });
    if (cells > 0) atomicAdd(counts + 0, (unsigned long long)cells);
    count_wave(dropped, counts + 1, (int)(threadIdx.x % kWave));
}

__global__ __launch_bounds__(kRcBlock) void k_rc_fill(MeshArgs a, const unsigned* start, const unsigned* l0, unsigned* cursor, unsigned* list, unsigned entries) {
    bool dropped;
    walk_ranges(a, &dropped, [=](uint32_t cell, uint32_t face) {
        const unsigned long long at = (unsigned long long)l0[cell / (unsigned)kRcTile] + start[cell] + atomicAdd(cursor + cell, 1u);
        if (at < entries) list[at] = face;                                     // (below it for the counts of eonerf_raycast_count)
    });
}

// cnt[0 .. n) -> its exclusive scan inside each tile (start), sums[tile] = the tile's total
__global__ __launch_bounds__(kRcBlock) void k_rc_tiles(const unsigned* cnt, unsigned n, unsigned* start, unsigned* sums) {
    const unsigned base = blockIdx.x * (unsigned)kRcTile;
    unsigned val[kRcRounds], excl[kRcRounds], total;
#pragma unroll
    for (int r = 0; r < kRcRounds; ++r) {
        const unsigned p = base + r * kRcBlock + threadIdx.x;
        val[r] = p < n ? cnt[p] : 0u;
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kRcRounds; ++r) {
        const unsigned p = base + r * kRcBlock + threadIdx.x;
        if (p < n) start[p] = excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[0 .. n) -> its exclusive scan inside each tile, in place; sums[tile] = the tile's total
__global__ __launch_bounds__(kRcBlock) void k_rc_scan(unsigned* data, unsigned n, unsigned* sums) {
    const unsigned base = blockIdx.x * (unsigned)kRcTile;
    unsigned val[kRcRounds], excl[kRcRounds], total;
#pragma unroll
    for (int r = 0; r < kRcRounds; ++r) {
        const unsigned p = base + r * kRcBlock + threadIdx.x;
        val[r] = p < n ? data[p] : 0u;
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kRcRounds; ++r) {
        const unsigned p = base + r * kRcBlock + threadIdx.x;
        if (p < n) data[p] = excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[p] += offs[p / tile]
__global__ __launch_bounds__(kRcBlock) void k_rc_add(unsigned* data, unsigned n, const unsigned* offs) {
    const unsigned p = blockIdx.x * (unsigned)kRcBlock + threadIdx.x;
    if (p < n) data[p] += offs[p / (unsigned)kRcTile];
}

struct CastArgs {
    MeshArgs m;
    const unsigned* start; const unsigned* l0; const unsigned* cursor; const unsigned* list; unsigned entries;
    const float* origins; long long origin_stride; const float* dirs; long long dir_stride; long long n_rays;
    double t_min, t_max;
};

// The triangles of the walk's cell, one after the other: hit(face, h) returns true to end the ray's walk at once.  Reads nothing
// through a list that is not the one eonerf_raycast_build left: the list stays inside the entries, the face inside the mesh, and
// rc_live checks the indices again before it reads a vertex.
template <class Hit>
__device__ inline bool cell_triangles(const CastArgs& a, const RcRay& r, uint32_t cell, Hit hit) {
    const unsigned long long first = (unsigned long long)a.l0[cell / (unsigned)kRcTile] + a.start[cell];
    const unsigned n = a.cursor[cell];
    for (unsigned k = 0; k < n; ++k) {
        if (first + k >= a.entries) break;
        const unsigned f = a.list[first + k];
        if ((long long)f >= a.m.n_triangles) continue;
        const int32_t* p = a.m.triangles + (size_t)f * 3;
        const int32_t tri[3] = {p[0], p[1], p[2]};
        double v[3][3];
        if (!rc_live(a.m.g, a.m.vertices, a.m.n_vertices, tri, v)) continue;
        RcHit h;
        if (rc_test(r, v, a.t_min, a.t_max, &h) && hit((int32_t)f, h)) return true;
    }
    return false;
}

__device__ inline RcRay load_ray(const CastArgs& a, long long i) {
    const float* po = a.origins + (size_t)i * (size_t)a.origin_stride;
    const float* pd = a.dirs + (size_t)i * (size_t)a.dir_stride;
    const float o[3] = {po[0], po[1], po[2]}, d[3] = {pd[0], pd[1], pd[2]};
    return rc_ray(o, d);
}

__global__ __launch_bounds__(kRcBlock) void k_rc_closest(CastArgs a, double* t_out, int32_t* face_out, float* bary_out, unsigned long long* counts) {
    const long long i = (long long)blockIdx.x * kRcBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x % kWave);
    bool rejected = false, found = false;
    if (i < a.n_rays) {
        const RcRay r = load_ray(a, i);
        rejected = !r.ok;
        int32_t best_face = -1;
        RcHit best;
        best.t = best.U = best.V = best.W = best.det = 0.0;
        if (r.ok) {
            RcWalk w = rc_walk(a.m.g, r, a.t_min, a.t_max);
            if (w.in) {
                do {
                    cell_triangles(a, r, rc_walk_cell(a.m.g, w), [&](int32_t f, const RcHit& h) {
                        if (rc_closer(h.t, f, best.t, best_face)) { best = h; best_face = f; }
                        return false;
                    });
                } while (rc_walk_step(a.m.g, w, best_face >= 0, best.t));
            }
        }
        found = best_face >= 0;
        const float nan = __int_as_float(0x7fc00000);
        float bary[3] = {nan, nan, nan};
        if (found) rc_bary(best, bary);
        t_out[i] = found ? best.t : __longlong_as_double(0x7ff8000000000000ll);
        face_out[i] = best_face;
        bary_out[(size_t)i * 3 + 0] = bary[0]; bary_out[(size_t)i * 3 + 1] = bary[1]; bary_out[(size_t)i * 3 + 2] = bary[2];
    }
    count_wave(i < a.n_rays, counts + 0, lane);
    count_wave(rejected, counts + 1, lane);
    count_wave(found, counts + 2, lane);
}

__global__ __launch_bounds__(kRcBlock) void k_rc_occluded(CastArgs a, const int32_t* skip, uint8_t* out, unsigned long long* counts) {
    const long long i = (long long)blockIdx.x * kRcBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x % kWave);
    bool rejected = false, found = false;
    if (i < a.n_rays) {
        const RcRay r = load_ray(a, i);
        rejected = !r.ok;
        const bool has_skip = skip != nullptr;
        const int32_t own = has_skip ? skip[i] : -1;
        if (r.ok) {
            RcWalk w = rc_walk(a.m.g, r, a.t_min, a.t_max);
            if (w.in) {
                do {
                    found = cell_triangles(a, r, rc_walk_cell(a.m.g, w), [&](int32_t f, const RcHit&) { return !(has_skip && f == own); });
                } while (!found && rc_walk_step(a.m.g, w, false, 0.0));
            }
        }
        out[i] = found ? 1 : 0;
    }
    count_wave(i < a.n_rays, counts + 0, lane);
    count_wave(rejected, counts + 1, lane);
    count_wave(found, counts + 2, lane);
}

inline unsigned blocks_of(uint64_t n, int per) { return (unsigned)((n + per - 1) / per); }     // n < 2^31: at most 2^23 workgroups

MeshArgs mesh_of(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* lo, const double* hi, const int* dims) {
    MeshArgs m;
    m.g = rc_grid(lo, hi, dims);
    m.vertices = (const float*)vertices; m.n_vertices = n_vertices; m.triangles = (const int32_t*)triangles; m.n_triangles = n_triangles;
    return m;
}

int cast(bool closest, const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* lo, const double* hi, const int* dims,
         int64_t entries, const void* workspace, size_t workspace_bytes, const float* origins, int64_t origin_stride, const float* dirs, int64_t dir_stride,
         int64_t n_rays, double t_min, double t_max, void* t_out, void* face_out, void* bary_out, const void* skip, void* occluded_out, void* counts_dev,
         void* stream) {
    const RcRays rays = {n_rays, origin_stride, dir_stride, t_min, t_max};
    const bool outputs_null = !counts_dev || (closest ? (!t_out || !face_out || !bary_out) : !occluded_out);
    const int rc = rc_check_cast(vertices, n_vertices, triangles, n_triangles, lo, hi, dims, entries, workspace, workspace_bytes, origins, dirs, rays, outputs_null);
    if (rc != EONERF_OK) return rc;
    const RcCarve c = rc_carve((uint64_t)rc_cells(dims), (uint64_t)entries);
    const RcWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts_dev, 0, 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_rays > 0) {
        CastArgs a;
        a.m = mesh_of(vertices, n_vertices, triangles, n_triangles, lo, hi, dims);
        a.start = w.start; a.l0 = w.l[0]; a.cursor = w.cursor; a.list = w.list; a.entries = (unsigned)entries;
        a.origins = origins; a.origin_stride = origin_stride; a.dirs = dirs; a.dir_stride = dir_stride; a.n_rays = n_rays;
        a.t_min = t_min; a.t_max = t_max;
        const dim3 grid(blocks_of((uint64_t)n_rays, kRcBlock));
        if (closest)
            hipLaunchKernelGGL(k_rc_closest, grid, dim3(kRcBlock), 0, s, a, (double*)t_out, (int32_t*)face_out, (float*)bary_out, (unsigned long long*)counts_dev);
        else
            hipLaunchKernelGGL(k_rc_occluded, grid, dim3(kRcBlock), 0, s, a, (const int32_t*)skip, (uint8_t*)occluded_out, (unsigned long long*)counts_dev);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int eonerf_raycast_version(void) { return EONERF_RAYCAST_VERSION; }

size_t eonerf_raycast_workspace_bytes(const int dims[3], int64_t n_triangles, int64_t entries) { return rc_workspace_bytes(dims, n_triangles, entries); }

int eonerf_raycast_count(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                         const int dims[3], void* cell_counts, void* counts_dev, void* stream) {
    const int rc = rc_check_count(vertices, n_vertices, triangles, n_triangles, lo, hi, dims, cell_counts, counts_dev);
    if (rc != EONERF_OK) return rc;
    const int64_t cells = rc_cells(dims);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts_dev, 0, 2 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(cell_counts, 0, (size_t)cells * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_triangles > 0)
        hipLaunchKernelGGL(k_rc_count, dim3(blocks_of((uint64_t)n_triangles, kRcBlock)), dim3(kRcBlock), 0, s,
                           mesh_of(vertices, n_vertices, triangles, n_triangles, lo, hi, dims), (unsigned*)cell_counts, (unsigned long long*)counts_dev);
    return (int)hipGetLastError();
}

int eonerf_raycast_build(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                         const int dims[3], const void* cell_counts, int64_t entries, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = rc_check_build(vertices, n_vertices, triangles, n_triangles, lo, hi, dims, cell_counts, entries, workspace, workspace_bytes);
    if (rc != EONERF_OK) return rc;
    const RcCarve c = rc_carve((uint64_t)rc_cells(dims), (uint64_t)entries);
    const RcWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(w.cursor, 0, (size_t)c.cells * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_rc_tiles, dim3((unsigned)c.lv.m[0]), dim3(kRcBlock), 0, s, (const unsigned*)cell_counts, (unsigned)c.cells, w.start, w.l[0]);
    for (int k = 0; k + 1 < c.lv.count; ++k)            // the levels above the tile sums: scan up to one sum, add the offsets back down
        hipLaunchKernelGGL(k_rc_scan, dim3((unsigned)c.lv.m[k + 1]), dim3(kRcBlock), 0, s, w.l[k], (unsigned)c.lv.m[k], w.l[k + 1]);
    for (int k = c.lv.count - 3; k >= 0; --k)
        hipLaunchKernelGGL(k_rc_add, dim3(blocks_of(c.lv.m[k], kRcBlock)), dim3(kRcBlock), 0, s, w.l[k], (unsigned)c.lv.m[k], (const unsigned*)w.l[k + 1]);
    if (n_triangles > 0)
        hipLaunchKernelGGL(k_rc_fill, dim3(blocks_of((uint64_t)n_triangles, kRcBlock)), dim3(kRcBlock), 0, s,
                           mesh_of(vertices, n_vertices, triangles, n_triangles, lo, hi, dims), (const unsigned*)w.start, (const unsigned*)w.l[0], w.cursor, w.list,
                           (unsigned)entries);
    return (int)hipGetLastError();
}

int eonerf_raycast_closest(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                           const int dims[3], int64_t entries, const void* workspace, size_t workspace_bytes, const float* origins, int64_t origin_stride,
                           const float* dirs, int64_t dir_stride, int64_t n_rays, double t_min, double t_max, void* t_out, void* face_out, void* bary_out,
                           void* counts_dev, void* stream) {
    return cast(true, vertices, n_vertices, triangles, n_triangles, lo, hi, dims, entries, workspace, workspace_bytes, origins, origin_stride, dirs, dir_stride, n_rays,
                t_min, t_max, t_out, face_out, bary_out, nullptr, nullptr, counts_dev, stream);
}

int eonerf_raycast_occluded(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                            const int dims[3], int64_t entries, const void* workspace, size_t workspace_bytes, const float* origins, int64_t origin_stride,
                            const float* dirs, int64_t dir_stride, int64_t n_rays, double t_min, double t_max, const void* skip, void* occluded_out,
                            void* counts_dev, void* stream) {
    return cast(false, vertices, n_vertices, triangles, n_triangles, lo, hi, dims, entries, workspace, workspace_bytes, origins, origin_stride, dirs, dir_stride, n_rays,
                t_min, t_max, nullptr, nullptr, nullptr, skip, occluded_out, counts_dev, stream);
}

}  // extern "C"
