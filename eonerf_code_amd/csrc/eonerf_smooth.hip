// eonerf_smooth.h: Taubin lambda|mu smoothing of a mesh in fixed point.  The rule is stated once, in eonerf_smooth_check.h; the
// kernels here decide only who evaluates it where.  Built with -ffp-contract=off, and the coordinate arithmetic uses the _rn intrinsics.
//
// build: k_smooth_quantise (a lane per vertex: its record Q_x, Q_y, Q_z, flags), k_smooth_count (a lane per face: live or dead, one
// 32-bit atomic add per corner), k_smooth_tiles and the plain blocked scan of eonerf_simplify.hip over the corner counts (scan inside
// tiles level by level up to one sum, add the offsets back down; no look-back, no flags), k_smooth_fill (a lane per face: its three
// corners (next, prev) into their vertices' lists through an atomic cursor), k_smooth_flags (a lane per vertex: B1, B2 over its own
// list, the flags, the counts).
// run: k_smooth_step once per factor -- a lane per vertex loops over its corners, gathers the 16-byte records of next and prev from the
// buffer of the step before and writes its own into the other buffer: a gather, no atomics, the hot path -- then k_smooth_emit.
// The order of corners inside a list depends on arrival; every quantity taken from a list is an integer sum, so no output bit does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "eonerf_smooth.h"
#include "eonerf_smooth_check.h"

namespace {

constexpr int kWave = 64;
static_assert(kSmoothBlock % kWave == 0, "whole waves");

struct SmoothWs {
    int4* q[3]; unsigned* cnt; unsigned* cursor; unsigned* start; uint2* corner; unsigned* l[kSmoothMaxLevels];
};

SmoothWs carve_of(void* workspace, const SmoothCarve& c) {
    char* b = (char*)workspace;
    SmoothWs w;
    for (int k = 0; k < 3; ++k) w.q[k] = (int4*)(b + c.q_off[k]);
    w.cnt = (unsigned*)(b + c.cnt_off); w.cursor = (unsigned*)(b + c.cursor_off); w.start = (unsigned*)(b + c.start_off);
    w.corner = (uint2*)(b + c.corner_off);
    for (int k = 0; k < kSmoothMaxLevels; ++k) w.l[k] = k < c.lv.count ? (unsigned*)(b + c.lv.off[k]) : nullptr;
    return w;
}

// Exclusive scan of one tile: element r * kSmoothBlock + tid of the tile is val[r] of thread tid.  One barrier; called once per kernel.
__device__ inline void scan_tile(const unsigned (&val)[kSmoothRounds], unsigned (&excl)[kSmoothRounds], unsigned& total) {
    constexpr int kWaves = kSmoothBlock / kWave;
    __shared__ unsigned wave_total[kSmoothRounds][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc[kSmoothRounds];
#pragma unroll
    for (int r = 0; r < kSmoothRounds; ++r) {
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
    for (int r = 0; r < kSmoothRounds; ++r) {
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

__global__ __launch_bounds__(kSmoothBlock) void k_smooth_quantise(SmoothGrid g, const float* vertices, unsigned n_vertices, int4* q0) {
    const unsigned v = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    if (v >= n_vertices) return;
    const float* p = vertices + (size_t)v * 3;
    const float xyz[3] = {p[0], p[1], p[2]};
    int32_t Q[3];
    const bool ok = smooth_quantise(g, xyz, Q);
    q0[v] = make_int4(Q[0], Q[1], Q[2], ok ? SMOOTH_QUANTISABLE : 0);
}

__device__ inline bool live_face(const int32_t* tri, long long n_vertices, const int4* q0) {
    return smooth_live(tri, n_vertices, [q0](int32_t v) { return q0[v].w; });
}

__global__ __launch_bounds__(kSmoothBlock) void k_smooth_count(const int32_t* triangles, unsigned n_triangles, long long n_vertices, const int4* q0,
                                                                unsigned* cnt, unsigned long long* counts) {
    const unsigned t = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x % kWave);
    bool dead = false;
    if (t < n_triangles) {
        const int32_t* p = triangles + (size_t)t * 3;
        const int32_t tri[3] = {p[0], p[1], p[2]};
        dead = !live_face(tri, n_vertices, q0);
        if (!dead)
            for (int k = 0; k < 3; ++k) atomicAdd(cnt + tri[k], 1u);
    }
    count_wave(dead, counts + 5, lane);
}

__global__ __launch_bounds__(kSmoothBlock) void k_smooth_fill(const int32_t* triangles, unsigned n_triangles, long long n_vertices, const int4* q0,
                                                               const unsigned* start, const unsigned* l0, unsigned* cursor, uint2* corner) {
    const unsigned t = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    if (t >= n_triangles) return;
    const int32_t* p = triangles + (size_t)t * 3;
    const int32_t tri[3] = {p[0], p[1], p[2]};
    if (!live_face(tri, n_vertices, q0)) return;
    for (int k = 0; k < 3; ++k) {
        const unsigned v = (unsigned)tri[k];
        const unsigned at = l0[v / (unsigned)kSmoothTile] + start[v] + atomicAdd(cursor + v, 1u);      // below the 3 T corners the counts add up to
        corner[at] = make_uint2((unsigned)tri[(k + 1) % 3], (unsigned)tri[(k + 2) % 3]);
    }
}

// cnt[0 .. n) -> its exclusive scan inside each tile (start), sums[tile] = the tile's total
__global__ __launch_bounds__(kSmoothBlock) void k_smooth_tiles(const unsigned* cnt, unsigned n, unsigned* start, unsigned* sums) {
    const unsigned base = blockIdx.x * (unsigned)kSmoothTile;
    unsigned val[kSmoothRounds], excl[kSmoothRounds], total;
#pragma unroll
    for (int r = 0; r < kSmoothRounds; ++r) {
        const unsigned p = base + r * kSmoothBlock + threadIdx.x;
        val[r] = p < n ? cnt[p] : 0u;
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kSmoothRounds; ++r) {
        const unsigned p = base + r * kSmoothBlock + threadIdx.x;
        if (p < n) start[p] = excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[0 .. n) -> its exclusive scan inside each tile, in place; sums[tile] = the tile's total
__global__ __launch_bounds__(kSmoothBlock) void k_smooth_scan(unsigned* data, unsigned n, unsigned* sums) {
    const unsigned base = blockIdx.x * (unsigned)kSmoothTile;
    unsigned val[kSmoothRounds], excl[kSmoothRounds], total;
#pragma unroll
    for (int r = 0; r < kSmoothRounds; ++r) {
        const unsigned p = base + r * kSmoothBlock + threadIdx.x;
        val[r] = p < n ? data[p] : 0u;
    }
    scan_tile(val, excl, total);
#pragma unroll
    for (int r = 0; r < kSmoothRounds; ++r) {
        const unsigned p = base + r * kSmoothBlock + threadIdx.x;
        if (p < n) data[p] = excl[r];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[p] += offs[p / tile]
__global__ __launch_bounds__(kSmoothBlock) void k_smooth_add(unsigned* data, unsigned n, const unsigned* offs) {
    const unsigned p = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    if (p < n) data[p] += offs[p / (unsigned)kSmoothTile];
}

__global__ __launch_bounds__(kSmoothBlock) void k_smooth_flags(unsigned n_vertices, int4* q0, const unsigned* cnt, const unsigned* start, const unsigned* l0,
                                                                const uint2* corner, const uint8_t* pinned, int pin_open, unsigned long long* counts) {
    const unsigned v = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x % kWave);
    int bits = 0;
    if (v < n_vertices) {
        const unsigned c = cnt[v];
        const uint2* list = corner + (size_t)(l0[v / (unsigned)kSmoothTile] + start[v]);
        int64_t B1 = 0;
        uint64_t B2 = 0;
        for (unsigned k = 0; k < c; ++k) {
            const uint2 e = list[k];
            smooth_balance(e.x, e.y, &B1, &B2);
        }
        const bool held = pinned != nullptr && pinned[v] != 0;
        const int flags = smooth_flags((q0[v].w & SMOOTH_QUANTISABLE) != 0, c, B1, B2, held, pin_open != 0);
        q0[v].w = flags;
        bits = smooth_count_bits(flags, c, held);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) count_wave((bits >> k) & 1, counts + k, lane);
}

struct StepArgs { unsigned n_vertices, n_corners; int lam_q; const int4* in; int4* out; const unsigned* cnt; const unsigned* start; const unsigned* l0; const uint2* corner; int* status; };

__global__ __launch_bounds__(kSmoothBlock) void k_smooth_step(StepArgs a) {
    const unsigned v = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    if (v >= a.n_vertices) return;
    int4 rec = a.in[v];
    if (rec.w & SMOOTH_FREE) {
        const unsigned c = a.cnt[v];
        const unsigned first = a.l0[v / (unsigned)kSmoothTile] + a.start[v];
        const uint2* list = a.corner + (size_t)first;
        long long S[3] = {0, 0, 0};
        for (unsigned k = 0; k < c; ++k) {
            if ((unsigned long long)first + k >= a.n_corners) break;      // (not the workspace the build call left: read nothing through it)
            const uint2 e = list[k];
            if (e.x >= a.n_vertices || e.y >= a.n_vertices) continue;     // (likewise; corners name vertices of live faces: inside the mesh)
            const int4 p = a.in[e.x], q = a.in[e.y];
            S[0] += (long long)p.x + q.x; S[1] += (long long)p.y + q.y; S[2] += (long long)p.z + q.z;
        }
        bool clamped = false;
        const int64_t n = 2 * (int64_t)c;
        rec.x = smooth_step(rec.x, S[0], n, a.lam_q, &clamped);
        rec.y = smooth_step(rec.y, S[1], n, a.lam_q, &clamped);
        rec.z = smooth_step(rec.z, S[2], n, a.lam_q, &clamped);
        if (clamped) atomicOr(a.status, EONERF_SMOOTH_STATUS_CLAMPED);
    }
    a.out[v] = rec;
}

__global__ __launch_bounds__(kSmoothBlock) void k_smooth_emit(SmoothGrid g, const uint32_t* vertices, unsigned n_vertices, const int4* q, uint32_t* out) {
    const unsigned v = blockIdx.x * (unsigned)kSmoothBlock + threadIdx.x;
    if (v >= n_vertices) return;
    const int4 rec = q[v];
    const uint32_t* in = vertices + (size_t)v * 3;
    uint32_t w[3] = {in[0], in[1], in[2]};                    // the input bits, whatever they spell
    if (rec.w & SMOOTH_FREE) {
        w[0] = __float_as_uint(smooth_dequantise(g, 0, rec.x));
        w[1] = __float_as_uint(smooth_dequantise(g, 1, rec.y));
        w[2] = __float_as_uint(smooth_dequantise(g, 2, rec.z));
    }
    uint32_t* o = out + (size_t)v * 3;
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
}

inline unsigned blocks_of(uint64_t n, int per) { return (unsigned)((n + per - 1) / per); }     // n < 2^31: at most 2^23 workgroups

// the levels above the tile sums l[0]: scan up to one sum, add the offsets back down
void scan_levels(const SmoothLevels& lv, unsigned* const* l, hipStream_t s) {
    for (int k = 0; k + 1 < lv.count; ++k)
        hipLaunchKernelGGL(k_smooth_scan, dim3((unsigned)lv.m[k + 1]), dim3(kSmoothBlock), 0, s, l[k], (unsigned)lv.m[k], l[k + 1]);
    for (int k = lv.count - 3; k >= 0; --k)
        hipLaunchKernelGGL(k_smooth_add, dim3(blocks_of(lv.m[k], kSmoothBlock)), dim3(kSmoothBlock), 0, s, l[k], (unsigned)lv.m[k], (const unsigned*)l[k + 1]);
}

}  // namespace

extern "C" {

int eonerf_smooth_version(void) { return EONERF_SMOOTH_VERSION; }

size_t eonerf_smooth_workspace_bytes(int64_t n_vertices, int64_t n_triangles) { return smooth_workspace_bytes(n_vertices, n_triangles); }

int eonerf_smooth_build(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const float origin[3], const float unit[3],
                        const void* pinned, int pin_open, void* workspace, size_t workspace_bytes, void* counts_dev, void* stream) {
    const int rc = smooth_check_build(vertices, n_vertices, triangles, n_triangles, origin, unit, workspace, workspace_bytes, counts_dev);
    if (rc != EONERF_OK) return rc;
    const SmoothCarve c = smooth_carve((uint64_t)n_vertices, (uint64_t)n_triangles);
    const SmoothWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts_dev, 0, 6 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_vertices > 0) {
        e = hipMemsetAsync(w.cnt, 0, c.start_off - c.cnt_off, s);                 // the counts and the cursors
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_smooth_quantise, dim3(blocks_of(c.n_vertices, kSmoothBlock)), dim3(kSmoothBlock), 0, s, smooth_grid(origin, unit),
                           (const float*)vertices, (unsigned)n_vertices, w.q[0]);
    }
    if (n_triangles > 0)
        hipLaunchKernelGGL(k_smooth_count, dim3(blocks_of(c.n_triangles, kSmoothBlock)), dim3(kSmoothBlock), 0, s, (const int32_t*)triangles, (unsigned)n_triangles,
                           (long long)n_vertices, (const int4*)w.q[0], w.cnt, (unsigned long long*)counts_dev);
    if (n_vertices > 0) {
        hipLaunchKernelGGL(k_smooth_tiles, dim3((unsigned)c.lv.m[0]), dim3(kSmoothBlock), 0, s, (const unsigned*)w.cnt, (unsigned)n_vertices, w.start, w.l[0]);
        scan_levels(c.lv, w.l, s);
        if (n_triangles > 0)
            hipLaunchKernelGGL(k_smooth_fill, dim3(blocks_of(c.n_triangles, kSmoothBlock)), dim3(kSmoothBlock), 0, s, (const int32_t*)triangles, (unsigned)n_triangles,
                               (long long)n_vertices, (const int4*)w.q[0], (const unsigned*)w.start, (const unsigned*)w.l[0], w.cursor, w.corner);
        hipLaunchKernelGGL(k_smooth_flags, dim3(blocks_of(c.n_vertices, kSmoothBlock)), dim3(kSmoothBlock), 0, s, (unsigned)n_vertices, w.q[0], (const unsigned*)w.cnt,
                           (const unsigned*)w.start, (const unsigned*)w.l[0], (const uint2*)w.corner, (const uint8_t*)pinned, pin_open, (unsigned long long*)counts_dev);
    }
    return (int)hipGetLastError();
}

int eonerf_smooth_run(const void* vertices, int64_t n_vertices, int64_t n_triangles, const float origin[3], const float unit[3], const int32_t* lam_q_host,
                      int n_steps, void* workspace, size_t workspace_bytes, void* out_vertices, void* status_dev, void* stream) {
    const int rc = smooth_check_run(vertices, n_vertices, n_triangles, origin, unit, lam_q_host, n_steps, workspace, workspace_bytes, out_vertices, status_dev);
    if (rc != EONERF_OK) return rc;
    const SmoothCarve c = smooth_carve((uint64_t)n_vertices, (uint64_t)n_triangles);
    const SmoothWs w = carve_of(workspace, c);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_vertices > 0) {
        const unsigned blocks = blocks_of(c.n_vertices, kSmoothBlock);
        StepArgs a;
        a.n_vertices = (unsigned)n_vertices; a.n_corners = (unsigned)(3 * c.n_triangles); a.cnt = w.cnt; a.start = w.start; a.l0 = w.l[0]; a.corner = w.corner; a.status = (int*)status_dev;
        const int4* last = w.q[0];                            // what build left; the steps alternate between the other two tables
        for (int k = 0; k < n_steps; ++k) {
            a.lam_q = lam_q_host[k]; a.in = last; a.out = w.q[1 + (k & 1)];
            hipLaunchKernelGGL(k_smooth_step, dim3(blocks), dim3(kSmoothBlock), 0, s, a);
            last = a.out;
        }
        hipLaunchKernelGGL(k_smooth_emit, dim3(blocks), dim3(kSmoothBlock), 0, s, smooth_grid(origin, unit), (const uint32_t*)vertices, (unsigned)n_vertices, last,
                           (uint32_t*)out_vertices);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
