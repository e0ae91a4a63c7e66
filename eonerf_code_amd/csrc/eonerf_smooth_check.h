// Host side of eonerf_smooth.h: the refusals of the two entry points in their documented order and the 64-bit size arithmetic of the
// workspace, in functions with no HIP call so that a stand-alone program can include them (tests/host/smooth_checks.cpp).
// The rule itself -- the quantisation of a vertex, rdiv, the step of one vertex given its sums, the dequantisation, the open test and
// the flags -- is here too, as functions the kernels of eonerf_smooth.hip call per lane and the stand-alone program calls in a loop:
// one statement of the rule for the device and for the host check.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eonerf_smooth.h"

#if defined(__HIPCC__)
#define SMOOTH_HD __host__ __device__
#else
#define SMOOTH_HD
#endif
// one fp64 operation each, never contracted: the device intrinsics say so themselves, the host build has no fused form to contract to
#if defined(__HIP_DEVICE_COMPILE__)
#define SMOOTH_ADD(a, b) __dadd_rn((a), (b))
#define SMOOTH_SUB(a, b) __dsub_rn((a), (b))
#define SMOOTH_MUL(a, b) __dmul_rn((a), (b))
#define SMOOTH_DIV(a, b) __ddiv_rn((a), (b))
#else
#define SMOOTH_ADD(a, b) ((a) + (b))
#define SMOOTH_SUB(a, b) ((a) - (b))
#define SMOOTH_MUL(a, b) ((a) * (b))
#define SMOOTH_DIV(a, b) ((a) / (b))
#endif

constexpr int kSmoothBlock = 256;                                   // threads of every kernel of the group: four waves
constexpr int kSmoothTile = EONERF_SMOOTH_TILE;                     // vertices / sums one workgroup scans
constexpr int kSmoothRounds = kSmoothTile / kSmoothBlock;
constexpr int kSmoothFracBits = EONERF_SMOOTH_FRAC_BITS;
constexpr int64_t kSmoothOne = (int64_t)1 << kSmoothFracBits;       // quanta per unit
constexpr int64_t kSmoothLim = ((int64_t)EONERF_SMOOTH_MAX_COORD << kSmoothFracBits) - 1;
constexpr int64_t kSmoothMaxVertices = (int64_t)INT32_MAX, kSmoothMaxTriangles = (int64_t)1 << 29;
constexpr int kSmoothMaxLevels = 4;                                 // 1024^3 < 2^31 - 1 <= 1024^4: the tile sums of a call, level by level
static_assert(kSmoothTile % kSmoothBlock == 0, "whole rounds");
static_assert((uint64_t)kSmoothMaxVertices <= (uint64_t)kSmoothTile * kSmoothTile * kSmoothTile * kSmoothTile, "four scan levels cover a call");
static_assert(3 * (uint64_t)kSmoothMaxTriangles <= (uint64_t)UINT32_MAX, "3 T, every corner count and every scanned sum fit a uint32");
static_assert(kSmoothLim == ((int64_t)1 << 29) - 1, "|Q| < 2^29: 2^30 corners of 2^30 each stay below 2^62");

// the flags of a vertex (the fourth word of its record)
enum { SMOOTH_FREE = 1, SMOOTH_QUANTISABLE = 2, SMOOTH_OPEN = 4 };

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// the sums above n scanned elements: m[0] = tiles, m[k + 1] = tiles of m[k], down to one; at least two levels, so that the last one
// always holds the grand total (n = 0: no level)
struct SmoothLevels { int count; uint64_t m[kSmoothMaxLevels]; size_t off[kSmoothMaxLevels]; };

struct SmoothCarve {
    uint64_t n_vertices, n_triangles;
    size_t q_off[3], cnt_off, cursor_off, start_off, corner_off, bytes;     // cursor_off follows cnt_off directly: one memset clears both
    SmoothLevels lv;
};

inline size_t smooth_align(size_t b) { return (b + 255) / 256 * 256; }

inline SmoothLevels smooth_levels(uint64_t n, size_t* at) {
    SmoothLevels l;
    l.count = 0;
    for (int k = 0; k < kSmoothMaxLevels; ++k) { l.m[k] = 0; l.off[k] = 0; }
    if (n == 0) return l;
    uint64_t m = (n + kSmoothTile - 1) / kSmoothTile;
    for (;;) {
        l.m[l.count] = m;
        l.off[l.count] = *at;
        *at += smooth_align((size_t)m * sizeof(uint32_t));
        ++l.count;
        if (m == 1 && l.count >= 2) break;
        m = (m + kSmoothTile - 1) / kSmoothTile;
    }
    return l;
}

// 0 <= n_vertices <= 2^31 - 1, 0 <= n_triangles <= 2^29
inline SmoothCarve smooth_carve(uint64_t n_vertices, uint64_t n_triangles) {
    SmoothCarve c;
    c.n_vertices = n_vertices; c.n_triangles = n_triangles;
    size_t at = 0;
    for (int k = 0; k < 3; ++k) { c.q_off[k] = at; at = smooth_align(at + (size_t)n_vertices * 16); }
    c.cnt_off = at;    at += smooth_align((size_t)n_vertices * sizeof(uint32_t));
    c.cursor_off = at; at += smooth_align((size_t)n_vertices * sizeof(uint32_t));
    c.start_off = at;  at += smooth_align((size_t)n_vertices * sizeof(uint32_t));
    c.corner_off = at; at += smooth_align((size_t)n_triangles * 3 * 2 * sizeof(uint32_t));
    c.lv = smooth_levels(n_vertices, &at);
    c.bytes = at > 0 ? at : 256;                                     // below 2^31 * 60 + 2^29 * 24 + the sums: far inside size_t; never 0
    return c;
}

// ---- refusals ---------------------------------------------------------------------------------------------------------------------
// One order for both entry points.  any_null: one of the pointers the call may not have null is.  lam_q == nullptr: the build call.
inline int smooth_check(bool any_null, int64_t n_vertices, int64_t n_triangles, const float* origin, const float* unit, const int32_t* lam_q,
                        int n_steps, size_t workspace_bytes) {
    if (any_null || !origin || !unit) return EONERF_E_ARG;
    if (n_vertices < 0 || n_triangles < 0) return EONERF_E_ARG;
    if (n_vertices > kSmoothMaxVertices || n_triangles > kSmoothMaxTriangles) return EONERF_E_UNSUPPORTED;
    for (int c = 0; c < 3; ++c)
        if (!isfinite(origin[c]) || !isfinite(unit[c]) || !(unit[c] > 0.f)) return EONERF_E_ARG;
    if (lam_q) {
        if (n_steps < 1 || n_steps > EONERF_SMOOTH_MAX_STEPS) return EONERF_E_ARG;
        for (int k = 0; k < n_steps; ++k)
            if (lam_q[k] > kSmoothOne || lam_q[k] < -kSmoothOne) return EONERF_E_ARG;
    }
    if (workspace_bytes < smooth_carve((uint64_t)n_vertices, (uint64_t)n_triangles).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

inline int smooth_check_build(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const float* origin,
                              const float* unit, const void* workspace, size_t workspace_bytes, const void* counts_dev) {
    return smooth_check(!vertices || !triangles || !workspace || !counts_dev, n_vertices, n_triangles, origin, unit, nullptr, 0, workspace_bytes);
}

inline int smooth_check_run(const void* vertices, int64_t n_vertices, int64_t n_triangles, const float* origin, const float* unit,
                            const int32_t* lam_q, int n_steps, const void* workspace, size_t workspace_bytes, const void* out_vertices,
                            const void* status_dev) {
    return smooth_check(!vertices || !lam_q || !workspace || !out_vertices || !status_dev, n_vertices, n_triangles, origin, unit, lam_q, n_steps,
                        workspace_bytes);
}

inline size_t smooth_workspace_bytes(int64_t n_vertices, int64_t n_triangles) {
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > kSmoothMaxVertices || n_triangles > kSmoothMaxTriangles) return 0;
    return smooth_carve((uint64_t)n_vertices, (uint64_t)n_triangles).bytes;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
struct SmoothGrid { double origin[3], unit[3]; };

inline SmoothGrid smooth_grid(const float* origin, const float* unit) {
    SmoothGrid g;
    for (int c = 0; c < 3; ++c) { g.origin[c] = (double)origin[c]; g.unit[c] = (double)unit[c]; }
    return g;
}

// Q[3] of a vertex; false (and Q = 0) where it is not quantisable
SMOOTH_HD inline bool smooth_quantise(const SmoothGrid& g, const float* v, int32_t Q[3]) {
    bool ok = true;
    double u[3];
    for (int c = 0; c < 3; ++c) {
        u[c] = SMOOTH_DIV(SMOOTH_SUB((double)v[c], g.origin[c]), g.unit[c]);
        ok = ok && fabs(u[c]) < (double)EONERF_SMOOTH_MAX_COORD;      // false for a NaN and for an infinity
    }
    for (int c = 0; c < 3; ++c) {
        int64_t q = ok ? (int64_t)llrint(SMOOTH_MUL(u[c], (double)kSmoothOne)) : 0;
        q = q > kSmoothLim ? kSmoothLim : q < -kSmoothLim ? -kSmoothLim : q;
        Q[c] = (int32_t)q;
    }
    return ok;
}

// floor(a / b) rounded half up, b > 0: C++ `/` truncates, so the remainder is brought to [0, b) by hand
SMOOTH_HD inline int64_t smooth_rdiv(int64_t a, int64_t b) {
    int64_t q, r;
    if (a == (int64_t)(int32_t)a && b <= (int64_t)INT32_MAX) {        // the same quotient from a 32-bit division, where both fit
        const int32_t a32 = (int32_t)a, b32 = (int32_t)b, q32 = a32 / b32;
        q = q32;
        r = (int64_t)a32 - (int64_t)q32 * b32;
    } else {
        q = a / b;
        r = a - q * b;
    }
    if (r < 0) { q -= 1; r += b; }
    return q + (r >= b - r ? 1 : 0);
}

// one axis of one free vertex: Q' from Q, S = the sum of Q[next] + Q[prev] over its corners, n = 2 c > 0
SMOOTH_HD inline int32_t smooth_step(int32_t Q, int64_t S, int64_t n, int32_t lam_q, bool* clamped) {
    const int64_t D = S - n * (int64_t)Q;
    const int64_t M = smooth_rdiv(D, n);                              // the neighbours' mean less Q: |M| < 2^30
    const int64_t delta = smooth_rdiv((int64_t)lam_q * M, kSmoothOne);
    int64_t moved = (int64_t)Q + delta;
    if (moved > kSmoothLim) { moved = kSmoothLim; *clamped = true; }
    if (moved < -kSmoothLim) { moved = -kSmoothLim; *clamped = true; }
    return (int32_t)moved;
}

SMOOTH_HD inline float smooth_dequantise(const SmoothGrid& g, int c, int32_t Q) {
    return (float)SMOOTH_ADD(g.origin[c], SMOOTH_MUL(SMOOTH_MUL((double)Q, 1.0 / (double)kSmoothOne), g.unit[c]));
}

// the two power sums of a vertex' corners, one corner at a time
SMOOTH_HD inline void smooth_balance(uint32_t next, uint32_t prev, int64_t* B1, uint64_t* B2) {
    *B1 += (int64_t)next - (int64_t)prev;
    *B2 += (uint64_t)next * next - (uint64_t)prev * prev;            // mod 2^64
}

SMOOTH_HD inline int smooth_flags(bool quantisable, uint32_t corners, int64_t B1, uint64_t B2, bool pinned, bool pin_open) {
    const bool open = B1 != 0 || B2 != 0;
    const bool free_ = quantisable && corners > 0 && !pinned && !(open && pin_open);
    return (free_ ? SMOOTH_FREE : 0) | (quantisable ? SMOOTH_QUANTISABLE : 0) | (open ? SMOOTH_OPEN : 0);
}

// which of counts_dev[0 .. 5) a vertex adds one to, as a bit set (bit k: counts[k])
SMOOTH_HD inline int smooth_count_bits(int flags, uint32_t corners, bool pinned) {
    const bool q = (flags & SMOOTH_QUANTISABLE) != 0;
    return ((flags & SMOOTH_FREE) ? 1 : 0) | ((flags & SMOOTH_OPEN) ? 2 : 0) | ((q && corners > 0 && pinned) ? 4 : 0) | ((q && corners == 0) ? 8 : 0) | (q ? 0 : 16);
}

// a face is live iff its indices are inside the mesh and its vertices quantisable; flags_of(v) reads the flags of vertex v
template <class F>
SMOOTH_HD inline bool smooth_live(const int32_t* tri, int64_t n_vertices, F flags_of) {
    for (int k = 0; k < 3; ++k) {
        if (tri[k] < 0 || (int64_t)tri[k] >= n_vertices) return false;
        if (!(flags_of(tri[k]) & SMOOTH_QUANTISABLE)) return false;
    }
    return true;
}
