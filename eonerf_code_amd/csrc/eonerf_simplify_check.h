// Host side of eonerf_simplify.h: the refusals of the two entry points in their documented order and the 64-bit size arithmetic of the
// workspace, in functions with no HIP call so that a stand-alone program can include them (tests/host/simplify_checks.cpp).
// The rule itself -- the quantisation of a vertex, the rounded mean, the key, the mean position, the class of a triangle -- is here too,
// as functions the kernels of eonerf_simplify.hip call per lane and the stand-alone program calls in a loop: one statement of the rule
// for the device and for the host check.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eonerf_simplify.h"

#if defined(__HIPCC__)
#define SIMP_HD __host__ __device__
#else
#define SIMP_HD
#endif
// one fp64 operation each, never contracted: the device intrinsics say so themselves, the host build has no fused form to contract to
#if defined(__HIP_DEVICE_COMPILE__)
#define SIMP_ADD(a, b) __dadd_rn((a), (b))
#define SIMP_SUB(a, b) __dadd_rn((a), -(b))
#define SIMP_MUL(a, b) __dmul_rn((a), (b))
#define SIMP_DIV(a, b) __ddiv_rn((a), (b))
#else
#define SIMP_ADD(a, b) ((a) + (b))
#define SIMP_SUB(a, b) ((a) - (b))
#define SIMP_MUL(a, b) ((a) * (b))
#define SIMP_DIV(a, b) ((a) / (b))
#endif

constexpr int kSimpBlock = 256;                                     // threads of every kernel of the group: four waves
constexpr int kSimpTile = EONERF_SIMPLIFY_TILE;                     // cells / triangles / sums one workgroup scans
constexpr int kSimpRounds = kSimpTile / kSimpBlock;
constexpr int kSimpSubBits = EONERF_SIMPLIFY_SUBCELL_BITS;
constexpr int64_t kSimpSub = (int64_t)1 << kSimpSubBits;            // sub-cells per cell and axis
constexpr int kSimpMaxLevels = 4;                                   // 1024^3 < 2^31 - 1 <= 1024^4: the tile sums of a call, level by level
static_assert(kSimpTile % kSimpBlock == 0 && kSimpTile <= (1 << 14), "the scan inside a tile shares a uint16 with the two class bits");
static_assert((uint64_t)INT32_MAX <= (uint64_t)kSimpTile * kSimpTile * kSimpTile * kSimpTile, "four scan levels cover a call");

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// number of cells, or 0 where dims is outside the limits
inline uint64_t simp_cells(const int* dims) {
    if (!dims) return 0;
    uint64_t n = 1;
    for (int c = 0; c < 3; ++c) {
        if (dims[c] < 1 || dims[c] > EONERF_SIMPLIFY_MAX_DIM) return 0;
        n *= (uint64_t)dims[c];                                     // at most 2^36
    }
    return n <= (uint64_t)EONERF_SIMPLIFY_MAX_CELLS ? n : 0;
}

// the sums above n scanned elements: m[0] = tiles, m[k + 1] = tiles of m[k], down to one; at least two levels, so that the last one
// always holds the grand total (n = 0: no level)
struct SimpLevels { int count; uint64_t m[kSimpMaxLevels]; size_t off[kSimpMaxLevels]; };

struct SimpCarve {
    uint64_t cells, n_vertices, n_triangles;
    size_t n_off, sum_off, key_off, cid_off, vcell_off, tflag_off, bytes;     // sum_off follows n_off directly: one memset clears both
    SimpLevels lc, lt;
};

inline size_t simp_align(size_t b) { return (b + 255) / 256 * 256; }

inline SimpLevels simp_levels(uint64_t n, size_t* at) {
    SimpLevels l;
    l.count = 0;
    for (int k = 0; k < kSimpMaxLevels; ++k) { l.m[k] = 0; l.off[k] = 0; }
    if (n == 0) return l;
    uint64_t m = (n + kSimpTile - 1) / kSimpTile;
    for (;;) {
        l.m[l.count] = m;
        l.off[l.count] = *at;
        *at += simp_align((size_t)m * sizeof(uint32_t));
        ++l.count;
        if (m == 1 && l.count >= 2) break;
        m = (m + kSimpTile - 1) / kSimpTile;
    }
    return l;
}

// cells > 0, 0 <= n_vertices, n_triangles <= INT32_MAX
inline SimpCarve simp_carve(uint64_t cells, uint64_t n_vertices, uint64_t n_triangles) {
    SimpCarve c;
    c.cells = cells; c.n_vertices = n_vertices; c.n_triangles = n_triangles;
    size_t at = 0;
    c.n_off = at;     at += (size_t)cells * sizeof(uint32_t);        // 4 * cells is a multiple of 8 or the last: S stays 8-aligned below
    at = (at + 7) / 8 * 8;
    c.sum_off = at;   at = simp_align(at + (size_t)cells * 3 * sizeof(uint64_t));
    c.key_off = at;   at = simp_align(at + (size_t)cells * sizeof(uint64_t));
    c.cid_off = at;   at = simp_align(at + (size_t)cells * sizeof(uint16_t));
    c.vcell_off = at; at = simp_align(at + (size_t)n_vertices * sizeof(int32_t));
    c.tflag_off = at; at = simp_align(at + (size_t)n_triangles * sizeof(uint16_t));
    c.lc = simp_levels(cells, &at);
    c.lt = simp_levels(n_triangles, &at);
    c.bytes = at;                                                    // below 2^27 * 38 + 2^31 * 6 + the sums: far inside size_t
    return c;
}

// ---- refusals ---------------------------------------------------------------------------------------------------------------------
// One order for both entry points.  any_null: one of the pointers the call may not have null is.
inline int simp_check(bool any_null, int64_t n_vertices, int64_t n_triangles, int64_t cap_vertices, int64_t cap_triangles, const float* origin,
                      const float* cell, const int* dims, size_t workspace_bytes, int representative) {
    if (any_null || !origin || !cell || !dims) return EONERF_E_ARG;
    if (n_vertices < 0 || n_triangles < 0 || cap_vertices < 0 || cap_triangles < 0) return EONERF_E_ARG;
    if (n_vertices > (int64_t)INT32_MAX || n_triangles > (int64_t)INT32_MAX) return EONERF_E_UNSUPPORTED;
    const uint64_t cells = simp_cells(dims);
    if (cells == 0) return EONERF_E_UNSUPPORTED;
    for (int c = 0; c < 3; ++c)
        if (!isfinite(origin[c]) || !isfinite(cell[c]) || !(cell[c] > 0.f)) return EONERF_E_ARG;
    if (workspace_bytes < simp_carve(cells, (uint64_t)n_vertices, (uint64_t)n_triangles).bytes) return EONERF_E_WORKSPACE;
    if (representative != EONERF_SIMPLIFY_MEAN && representative != EONERF_SIMPLIFY_NEAREST) return EONERF_E_ARG;
    return EONERF_OK;
}

inline int simp_check_count(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const float* origin,
                            const float* cell, const int* dims, const void* workspace, size_t workspace_bytes, const void* counts_dev) {
    return simp_check(!vertices || !triangles || !workspace || !counts_dev, n_vertices, n_triangles, 0, 0, origin, cell, dims, workspace_bytes,
                      EONERF_SIMPLIFY_MEAN);
}

inline int simp_check_emit(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const float* origin,
                           const float* cell, const int* dims, int representative, const void* workspace, size_t workspace_bytes,
                           const void* out_vertices, int64_t cap_vertices, const void* out_triangles, int64_t cap_triangles,
                           const void* status_dev) {
    return simp_check(!vertices || !triangles || !workspace || !out_vertices || !out_triangles || !status_dev, n_vertices, n_triangles,
                      cap_vertices, cap_triangles, origin, cell, dims, workspace_bytes, representative);
}

inline size_t simp_workspace_bytes(const int* dims, int64_t n_vertices, int64_t n_triangles) {
    const uint64_t cells = simp_cells(dims);
    if (cells == 0 || n_vertices < 0 || n_triangles < 0 || n_vertices > (int64_t)INT32_MAX || n_triangles > (int64_t)INT32_MAX) return 0;
    return simp_carve(cells, (uint64_t)n_vertices, (uint64_t)n_triangles).bytes;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
struct SimpGrid { double origin[3], cell[3]; int dims[3]; };

inline SimpGrid simp_grid(const float* origin, const float* cell, const int* dims) {
    SimpGrid g;
    for (int c = 0; c < 3; ++c) { g.origin[c] = (double)origin[c]; g.cell[c] = (double)cell[c]; g.dims[c] = dims[c]; }
    return g;
}

// a vertex in the grid: its cell id (-1: dropped) and its local coordinates
struct SimpVertex { int32_t cell; int32_t q[3]; int32_t L[3]; };

SIMP_HD inline SimpVertex simp_vertex(const SimpGrid& g, const float* v) {
    SimpVertex r;
    r.cell = -1;
    for (int c = 0; c < 3; ++c) { r.q[c] = 0; r.L[c] = 0; }
    // every comparison is false for a NaN
    if (!(fabsf(v[0]) <= 3.402823466e38f && fabsf(v[1]) <= 3.402823466e38f && fabsf(v[2]) <= 3.402823466e38f)) return r;
    for (int c = 0; c < 3; ++c) {
        const double u = SIMP_DIV(SIMP_SUB((double)v[c], g.origin[c]), g.cell[c]);
        double s = SIMP_MUL(u, (double)kSimpSub);
        const double top = (double)((int64_t)g.dims[c] * kSimpSub - 1);
        s = s < 0.0 ? 0.0 : s > top ? top : s;
        const int64_t F = (int64_t)llrint(s);
        r.q[c] = (int32_t)(F >> kSimpSubBits);
        r.L[c] = (int32_t)(F & (kSimpSub - 1));
    }
    r.cell = (r.q[2] * g.dims[1] + r.q[1]) * g.dims[0] + r.q[0];          // below 2^27
    return r;
}

// the rounded mean of a cell's local coordinates along one axis, n > 0
SIMP_HD inline int64_t simp_mean(uint64_t S, uint32_t n) { return (int64_t)((2 * S + n) / (2 * (uint64_t)n)); }

SIMP_HD inline uint64_t simp_key(const int32_t L[3], const uint64_t S[3], uint32_t n, uint32_t vertex) {
    uint64_t d2 = 0;
    for (int c = 0; c < 3; ++c) {
        const int64_t d = (int64_t)L[c] - simp_mean(S[c], n);
        d2 += (uint64_t)(d * d);
    }
    return (d2 << 32) | (uint64_t)vertex;
}

// the MEAN position of a cell along axis c
SIMP_HD inline float simp_mean_position(const SimpGrid& g, int c, int32_t q, uint64_t S, uint32_t n) {
    const double local = SIMP_DIV(SIMP_DIV((double)S, (double)n), (double)kSimpSub);
    return (float)SIMP_ADD(g.origin[c], SIMP_MUL(SIMP_ADD((double)q, local), g.cell[c]));
}

enum { SIMP_KEEP = 0, SIMP_DROPPED = 1, SIMP_COLLAPSED = 2 };

// the class of a triangle from the cell ids of the vertices (new ids are equal iff cell ids are); reads vcell only at valid indices
SIMP_HD inline int simp_classify(const int32_t* vcell, int64_t n_vertices, const int32_t* tri, int32_t cells[3]) {
    for (int k = 0; k < 3; ++k) {
        cells[k] = -1;
        if (tri[k] < 0 || (int64_t)tri[k] >= n_vertices) return SIMP_DROPPED;
        cells[k] = vcell[tri[k]];
        if (cells[k] < 0) return SIMP_DROPPED;
    }
    return (cells[0] == cells[1] || cells[1] == cells[2] || cells[2] == cells[0]) ? SIMP_COLLAPSED : SIMP_KEEP;
}
