// Host side of eonerf_raycast.h: the refusals of the entry points in their documented order and the 64-bit size arithmetic of the
// workspace, in functions with no HIP call so that a stand-alone program can include them (tests/host/raycast_checks.cpp).
// The rule itself -- which triangles are live, the setup of a ray, the test of one triangle, the padded cell range of a triangle, the
// stepper's start, step and stop -- is here too, as functions the kernels of eonerf_raycast.hip call per lane and the stand-alone
// program calls in a loop: one statement of the rule for the device and for the host check.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eonerf_raycast.h"

#if defined(__HIPCC__)
#define RC_HD __host__ __device__
#else
#define RC_HD
#endif
// one fp64 operation each, never contracted: the device intrinsics say so themselves, the host build has no fused form to contract to
#if defined(__HIP_DEVICE_COMPILE__)
#define RC_ADD(a, b) __dadd_rn((a), (b))
#define RC_SUB(a, b) __dsub_rn((a), (b))
#define RC_MUL(a, b) __dmul_rn((a), (b))
#define RC_DIV(a, b) __ddiv_rn((a), (b))
#else
#define RC_ADD(a, b) ((a) + (b))
#define RC_SUB(a, b) ((a) - (b))
#define RC_MUL(a, b) ((a) * (b))
#define RC_DIV(a, b) ((a) / (b))
#endif

constexpr int kRcBlock = 256;                                       // threads of every kernel of the group: four waves
constexpr int kRcTile = EONERF_RAYCAST_TILE;                        // cells / sums one workgroup scans
constexpr int kRcRounds = kRcTile / kRcBlock;
constexpr int kRcMaxLevels = 3;                                     // 1024^2 < 2^27 <= 1024^3
constexpr int64_t kRcMaxCells = (int64_t)1 << 27, kRcMaxCount = (int64_t)INT32_MAX;
constexpr int64_t kRcMaxStride = EONERF_RAYCAST_MAX_STRIDE;                 // floats between two rays: their offsets stay inside 2^57 bytes
constexpr int kRcLaneCells = EONERF_RAYCAST_LANE_CELLS;
constexpr double kRcPad = EONERF_RAYCAST_PAD;
static_assert(kRcTile % kRcBlock == 0, "whole rounds");
static_assert((uint64_t)kRcMaxCells <= (uint64_t)kRcTile * kRcTile * kRcTile, "three scan levels cover a grid");
static_assert(kRcPad == 1.0 / 256, "2^-8 of a cell");
static_assert((int64_t)EONERF_RAYCAST_MAX_DIM * EONERF_RAYCAST_MAX_DIM * EONERF_RAYCAST_MAX_DIM < ((int64_t)1 << 62), "a box's cells fit 64 bits");

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// the sums above n scanned cells: m[0] = tiles, m[k + 1] = tiles of m[k], down to one; at least two levels, so that the last one
// always holds the grand total
struct RcLevels { int count; uint64_t m[kRcMaxLevels]; size_t off[kRcMaxLevels]; };

struct RcCarve {
    uint64_t cells, entries;
    size_t start_off, cursor_off, list_off, bytes;
    RcLevels lv;
};

inline size_t rc_align(size_t b) { return (b + 255) / 256 * 256; }

inline RcLevels rc_levels(uint64_t n, size_t* at) {
    RcLevels l;
    l.count = 0;
    for (int k = 0; k < kRcMaxLevels; ++k) { l.m[k] = 0; l.off[k] = 0; }
    uint64_t m = (n + kRcTile - 1) / kRcTile;
    for (;;) {
        l.m[l.count] = m;
        l.off[l.count] = *at;
        *at += rc_align((size_t)m * sizeof(uint32_t));
        ++l.count;
        if (m == 1 && l.count >= 2) break;
        m = (m + kRcTile - 1) / kRcTile;
    }
    return l;
}

// the cells of a grid, or 0 where dims is not one: an entry outside 1 .. MAX_DIM (-1), more than 2^27 cells (-2)
inline int64_t rc_cells(const int* dims) {
    int64_t n = 1;
    for (int c = 0; c < 3; ++c) {
        if (dims[c] < 1 || dims[c] > EONERF_RAYCAST_MAX_DIM) return -1;
        n *= dims[c];                                                // at most 2^36
    }
    return n > kRcMaxCells ? -2 : n;
}

// 1 <= cells <= 2^27, 0 <= entries <= 2^31 - 1
inline RcCarve rc_carve(uint64_t cells, uint64_t entries) {
    RcCarve c;
    c.cells = cells; c.entries = entries;
    size_t at = 0;
    c.start_off = at;  at += rc_align((size_t)cells * sizeof(uint32_t));
    c.cursor_off = at; at += rc_align((size_t)cells * sizeof(uint32_t));
    c.lv = rc_levels(cells, &at);
    c.list_off = at;   at += rc_align((size_t)entries * sizeof(uint32_t));
    c.bytes = at;                                                    // below 2^27 * 8 + 2^31 * 4 + the sums: far inside size_t
    return c;
}

inline size_t rc_workspace_bytes(const int* dims, int64_t n_triangles, int64_t entries) {
    if (!dims || n_triangles < 0 || n_triangles > kRcMaxCount || entries < 0 || entries > kRcMaxCount) return 0;
    const int64_t cells = rc_cells(dims);
    return cells < 1 ? 0 : rc_carve((uint64_t)cells, (uint64_t)entries).bytes;
}

// ---- refusals ---------------------------------------------------------------------------------------------------------------------
// One order for all entry points.  any_null: one of the pointers the call may not have null is.  entries < -1 never; entries == -1 with
// with_entries == false: the call takes none (count).  with_rays: a cast (n_rays, the strides, t_min, t_max).
struct RcRays { int64_t n_rays, origin_stride, dir_stride; double t_min, t_max; };

inline int rc_check(bool any_null, int64_t n_vertices, int64_t n_triangles, const double* lo, const double* hi, const int* dims, bool with_entries,
                    int64_t entries, const RcRays* rays, bool with_workspace, size_t workspace_bytes) {
    if (any_null || !lo || !hi || !dims) return EONERF_E_ARG;
    if (n_vertices < 0 || n_triangles < 0 || (rays && rays->n_rays < 0)) return EONERF_E_ARG;
    if (n_vertices > kRcMaxCount || n_triangles > kRcMaxCount || (rays && rays->n_rays > kRcMaxCount)) return EONERF_E_UNSUPPORTED;
    for (int c = 0; c < 3; ++c)
        if (!isfinite(lo[c]) || !isfinite(hi[c]) || !(lo[c] < hi[c])) return EONERF_E_ARG;
    const int64_t cells = rc_cells(dims);
    if (cells == -1) return EONERF_E_ARG;
    if (cells == -2) return EONERF_E_UNSUPPORTED;
    if (with_entries) {
        if (entries < 0) return EONERF_E_ARG;
        if (entries > kRcMaxCount) return EONERF_E_UNSUPPORTED;
    }
    if (rays) {
        if (rays->origin_stride < 3 || rays->dir_stride < 3 || rays->origin_stride > kRcMaxStride || rays->dir_stride > kRcMaxStride) return EONERF_E_ARG;
        if (!(rays->t_min >= 0.0) || !(rays->t_min <= rays->t_max) || isinf(rays->t_min)) return EONERF_E_ARG;      // false for a NaN
    }
    if (with_workspace && workspace_bytes < rc_carve((uint64_t)cells, (uint64_t)entries).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

inline int rc_check_count(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* lo, const double* hi,
                          const int* dims, const void* cell_counts, const void* counts_dev) {
    return rc_check(!vertices || !triangles || !cell_counts || !counts_dev, n_vertices, n_triangles, lo, hi, dims, false, 0, nullptr, false, 0);
}

inline int rc_check_build(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* lo, const double* hi,
                          const int* dims, const void* cell_counts, int64_t entries, const void* workspace, size_t workspace_bytes) {
    return rc_check(!vertices || !triangles || !cell_counts || !workspace, n_vertices, n_triangles, lo, hi, dims, true, entries, nullptr, true, workspace_bytes);
}

// outputs_null: one of the cast's own outputs (t / face / bary, or the occluded bytes) or counts_dev is null
inline int rc_check_cast(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* lo, const double* hi,
                         const int* dims, int64_t entries, const void* workspace, size_t workspace_bytes, const void* origins, const void* dirs,
                         const RcRays& rays, bool outputs_null) {
    return rc_check(!vertices || !triangles || !workspace || !origins || !dirs || outputs_null, n_vertices, n_triangles, lo, hi, dims, true, entries, &rays,
                    true, workspace_bytes);
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
struct RcGrid { double lo[3], hi[3], inv[3]; int dims[3]; };        // inv = dims / (hi - lo): cells per unit

inline RcGrid rc_grid(const double* lo, const double* hi, const int* dims) {
    RcGrid g;
    for (int c = 0; c < 3; ++c) { g.lo[c] = lo[c]; g.hi[c] = hi[c]; g.dims[c] = dims[c]; g.inv[c] = (double)dims[c] / (hi[c] - lo[c]); }
    return g;
}

// the three vertices of a live triangle, widened; false where the triangle is dropped.  Reads a vertex only after its index passed.
RC_HD inline bool rc_live(const RcGrid& g, const float* vertices, int64_t n_vertices, const int32_t* tri, double v[3][3]) {
    for (int k = 0; k < 3; ++k)
        if (tri[k] < 0 || (int64_t)tri[k] >= n_vertices) return false;
    bool ok = true;
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) {
            const double p = (double)vertices[(size_t)tri[k] * 3 + c];
            v[k][c] = p;
            ok = ok && p >= g.lo[c] && p <= g.hi[c];                 // false for a NaN; an infinity is outside a finite box
        }
    return ok;
}

// the cells floor(min g - PAD) .. floor(max g + PAD) of a live triangle per axis, clamped to the grid
RC_HD inline int rc_cell_clamp(double f, int n) {
    f = fmin(fmax(f, 0.0), (double)(n - 1));                         // (a NaN becomes 0: fmax returns its other argument)
    return (int)f;
}

RC_HD inline void rc_cell_range(const RcGrid& g, const double v[3][3], int c0[3], int c1[3]) {
    for (int c = 0; c < 3; ++c) {
        const double a = RC_MUL(RC_SUB(v[0][c], g.lo[c]), g.inv[c]), b = RC_MUL(RC_SUB(v[1][c], g.lo[c]), g.inv[c]), d = RC_MUL(RC_SUB(v[2][c], g.lo[c]), g.inv[c]);
        c0[c] = rc_cell_clamp(floor(RC_SUB(fmin(fmin(a, b), d), kRcPad)), g.dims[c]);
        c1[c] = rc_cell_clamp(floor(RC_ADD(fmax(fmax(a, b), d), kRcPad)), g.dims[c]);
    }
}

RC_HD inline int64_t rc_range_cells(const int c0[3], const int c1[3]) {
    return (int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
}

// cell number k of a range, x fastest, as an index into the grid
RC_HD inline uint32_t rc_range_cell(const RcGrid& g, const int c0[3], const int c1[3], int64_t k) {
    const int wx = c1[0] - c0[0] + 1, wy = c1[1] - c0[1] + 1;
    const int x = c0[0] + (int)(k % wx), y = c0[1] + (int)(k / wx % wy), z = c0[2] + (int)(k / ((int64_t)wx * wy));
    return (uint32_t)(((int64_t)z * g.dims[1] + y) * g.dims[0] + x);
}

// a[k] by selects: an index that is not known at compile time would put the array into scratch memory on the device
RC_HD inline double rc_pick(const double a[3], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : a[2]; }

// po: the origin in the order (kx, ky, kz)
struct RcRay { double o[3], d[3], po[3], Sx, Sy, Sz; int kx, ky, kz; bool ok; };

RC_HD inline RcRay rc_ray(const float* o, const float* d) {
    RcRay r;
    r.ok = true;
    for (int c = 0; c < 3; ++c) {
        r.o[c] = (double)o[c]; r.d[c] = (double)d[c];
        r.ok = r.ok && isfinite(r.o[c]) && isfinite(r.d[c]);
    }
    r.ok = r.ok && !(r.d[0] == 0.0 && r.d[1] == 0.0 && r.d[2] == 0.0);
    r.kz = 0;
    if (fabs(r.d[1]) > fabs(r.d[0])) r.kz = 1;
    if (fabs(r.d[2]) > fabs(rc_pick(r.d, r.kz))) r.kz = 2;
    r.kx = (r.kz + 1) % 3; r.ky = (r.kx + 1) % 3;
    if (rc_pick(r.d, r.kz) < 0.0) { const int s = r.kx; r.kx = r.ky; r.ky = s; }
    const double dz = r.ok ? rc_pick(r.d, r.kz) : 1.0;
    r.Sx = RC_DIV(rc_pick(r.d, r.kx), dz); r.Sy = RC_DIV(rc_pick(r.d, r.ky), dz); r.Sz = RC_DIV(1.0, dz);
    r.po[0] = rc_pick(r.o, r.kx); r.po[1] = rc_pick(r.o, r.ky); r.po[2] = rc_pick(r.o, r.kz);
    return r;
}

struct RcHit { double t, U, V, W, det; };

// one live triangle against one ray: whether it hits in [t_min, t_max], and t, U, V, W, det
RC_HD inline bool rc_test(const RcRay& r, const double v[3][3], double t_min, double t_max, RcHit* h) {
    double x[3], y[3], z[3];
    for (int k = 0; k < 3; ++k) {
        const double px = RC_SUB(rc_pick(v[k], r.kx), r.po[0]), py = RC_SUB(rc_pick(v[k], r.ky), r.po[1]), pz = RC_SUB(rc_pick(v[k], r.kz), r.po[2]);
        x[k] = RC_SUB(px, RC_MUL(r.Sx, pz));
        y[k] = RC_SUB(py, RC_MUL(r.Sy, pz));
        z[k] = RC_MUL(r.Sz, pz);
    }
    const double U = RC_SUB(RC_MUL(x[2], y[1]), RC_MUL(y[2], x[1]));
    const double V = RC_SUB(RC_MUL(x[0], y[2]), RC_MUL(y[0], x[2]));
    const double W = RC_SUB(RC_MUL(x[1], y[0]), RC_MUL(y[1], x[0]));
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return false;      // false for a NaN
    const double det = RC_ADD(RC_ADD(U, V), W);
    if (det == 0.0) return false;
    const double t = RC_DIV(RC_ADD(RC_ADD(RC_MUL(U, z[0]), RC_MUL(V, z[1])), RC_MUL(W, z[2])), det);
    if (!(isfinite(t) && t >= t_min && t <= t_max)) return false;
    h->t = t; h->U = U; h->V = V; h->W = W; h->det = det;
    return true;
}

RC_HD inline void rc_bary(const RcHit& h, float bary[3]) {
    bary[0] = (float)RC_DIV(h.U, h.det); bary[1] = (float)RC_DIV(h.V, h.det); bary[2] = (float)RC_DIV(h.W, h.det);
}

// (t, face) before (best_t, best_face) in the lexicographic order; best_face < 0: nothing yet
RC_HD inline bool rc_closer(double t, int32_t face, double best_t, int32_t best_face) {
    return best_face < 0 || t < best_t || (t == best_t && face < best_face);
}

// ---- the stepper ------------------------------------------------------------------------------------------------------------------
// The ray in cell units: g_c(t) = og[c] + t dg[c].  cell: where it is; next[c]: the parameter at which it crosses its cell's far
// boundary along c (+inf where dg[c] == 0); t_exit: min(t_max, where it leaves the box grown by PAD); left: steps it may still take.
struct RcWalk { double og[3], dg[3], next[3], t_exit; int cell[3], step[3], left; bool in; };

RC_HD inline double rc_cross(const RcWalk& w, int c) {
    if (w.dg[c] == 0.0) return INFINITY;
    const double boundary = (double)(w.cell[c] + (w.step[c] > 0 ? 1 : 0));
    return RC_DIV(RC_SUB(boundary, w.og[c]), w.dg[c]);
}

// in == false: the ray misses the grown box inside [t_min, t_max] and nothing can hit
RC_HD inline RcWalk rc_walk(const RcGrid& g, const RcRay& r, double t_min, double t_max) {
    RcWalk w;
    double t_in = t_min, t_out = t_max;
    w.in = true;
    for (int c = 0; c < 3; ++c) {
        w.og[c] = RC_MUL(RC_SUB(r.o[c], g.lo[c]), g.inv[c]);
        w.dg[c] = RC_MUL(r.d[c], g.inv[c]);
        w.step[c] = w.dg[c] > 0.0 ? 1 : w.dg[c] < 0.0 ? -1 : 0;
        const double low = -kRcPad, high = RC_ADD((double)g.dims[c], kRcPad);
        if (w.dg[c] == 0.0) {
            w.in = w.in && w.og[c] >= low && w.og[c] <= high;
        } else {
            const double a = RC_DIV(RC_SUB(low, w.og[c]), w.dg[c]), b = RC_DIV(RC_SUB(high, w.og[c]), w.dg[c]);
            t_in = fmax(t_in, fmin(a, b));
            t_out = fmin(t_out, fmax(a, b));
        }
    }
    w.in = w.in && t_in <= t_out && isfinite(t_in);                  // false for a NaN
    w.t_exit = t_out;
    w.left = g.dims[0] + g.dims[1] + g.dims[2] + 3;
    for (int c = 0; c < 3; ++c) {
        const double at = w.in ? RC_ADD(w.og[c], RC_MUL(t_in, w.dg[c])) : 0.0;
        w.cell[c] = rc_cell_clamp(floor(at), g.dims[c]);
    }
    for (int c = 0; c < 3; ++c) w.next[c] = rc_cross(w, c);
    return w;
}

RC_HD inline uint32_t rc_walk_cell(const RcGrid& g, const RcWalk& w) {
    return (uint32_t)(((int64_t)w.cell[2] * g.dims[1] + w.cell[1]) * g.dims[0] + w.cell[0]);
}

// the parameter at which the ray leaves its cell
RC_HD inline double rc_walk_leave(const RcWalk& w) { return fmin(fmin(w.next[0], w.next[1]), w.next[2]); }

// After the triangles of the cell: moves to the next cell; false where the walk is over -- the closest hit so far (have_hit, best_t)
// lies at or before the point where the ray leaves the cell, that point is beyond the exit, the step leaves the grid, or no step is
// left.  Every comparison is written so that a NaN ends the walk.
RC_HD inline bool rc_walk_step(const RcGrid& g, RcWalk& w, bool have_hit, double best_t) {
    const double leave = rc_walk_leave(w);
    if (have_hit && best_t <= leave) return false;
    if (!(leave <= w.t_exit)) return false;
    if (--w.left <= 0) return false;
    const int c = (w.next[0] <= w.next[1] && w.next[0] <= w.next[2]) ? 0 : (w.next[1] <= w.next[2] ? 1 : 2);
    bool inside = false;
    for (int a = 0; a < 3; ++a)                                      // (unrolled: every index a constant)
        if (a == c) {
            w.cell[a] += w.step[a];
            inside = w.step[a] != 0 && w.cell[a] >= 0 && w.cell[a] < g.dims[a];
            if (inside) w.next[a] = rc_cross(w, a);
        }
    return inside;
}
