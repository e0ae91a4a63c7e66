// Host side of eonerf_dual.h: the refusals of the entry points in their documented order, the size arithmetic (64-bit) and the
// workspace carve, in functions with no HIP call so that a stand-alone program can include them (tests/host/dual_checks.cpp).  Each
// check returns 0 or the EONERF_E_* the entry point returns before it launches anything.
// The rule itself -- the classification of one lattice point, the vertex of one cell, the quads of one point -- is here too, as
// functions the kernels of eonerf_dual.hip call per thread and the stand-alone program calls in a loop: one statement of the rule for
// the device and for the host check.  The lattice, the inside test, t and the coordinate rule are eonerf_mesh_check.h's own functions.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eonerf_dual.h"
#include "eonerf_mesh_check.h"

#if defined(__HIPCC__)
#define DUAL_HD __host__ __device__
#else
#define DUAL_HD
#endif
// one fp64 operation each, never contracted: the device intrinsics say so themselves, the host build has no fused form to contract to
#if defined(__HIP_DEVICE_COMPILE__)
#define DUAL_ADD(a, b) __dadd_rn((a), (b))
#define DUAL_SUB(a, b) __dsub_rn((a), (b))
#define DUAL_MUL(a, b) __dmul_rn((a), (b))
#define DUAL_DIV(a, b) __ddiv_rn((a), (b))
#else
#define DUAL_ADD(a, b) ((a) + (b))
#define DUAL_SUB(a, b) ((a) - (b))
#define DUAL_MUL(a, b) ((a) * (b))
#define DUAL_DIV(a, b) ((a) / (b))
#endif

// info byte of a point: bits 0 .. 2 the mask of its owned crossing axis edges, bit 3 its cell is active, bits 4 .. 5 its quads
constexpr unsigned kDualMask = 7u, kDualActive = 8u;
constexpr int kDualQuadShift = 4;

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// the workspace: per point lh, lc, lq (uint16 each) and info (uint8); per tile / per kMeshTile tiles / once the sums (four uint32 each)
struct DualCarve { uint64_t n, n1, n2; size_t lh_off, lc_off, lq_off, info_off, l1_off, l2_off, l3_off, bytes; };
inline DualCarve dual_carve(uint64_t n) {
    DualCarve c;
    c.n = n;
    c.n1 = (n + kMeshTile - 1) / kMeshTile;
    c.n2 = (c.n1 + kMeshTile - 1) / kMeshTile;             // <= kMeshTile while n <= kMeshTile^3: the third level is one sum
    uint64_t off = 0;
    auto take = [&off](uint64_t bytes) { const uint64_t at = off; off = (off + bytes + 255) & ~(uint64_t)255; return (size_t)at; };
    c.lh_off = take(2 * n);
    c.lc_off = take(2 * n);
    c.lq_off = take(2 * n);
    c.info_off = take(n);
    c.l1_off = take(16 * c.n1);
    c.l2_off = take(16 * c.n2);
    c.l3_off = take(16);
    c.bytes = (size_t)off;
    return c;
}
static_assert(3 * kMeshTile <= 65535, "the scans inside a tile are uint16");
static_assert(6 * (uint64_t)EONERF_MESH_MAX_POINTS <= 0xffffffffull, "two triangles per quad, three quads per point: a uint32 offset");

inline bool dual_regularisation_ok(float lambda) {
    return isfinite(lambda) && lambda >= ldexpf(1.f, EONERF_DUAL_MIN_REG_LOG2) && lambda <= ldexpf(1.f, EONERF_DUAL_MAX_REG_LOG2);
}

inline int dual_check_count(const void* f, int nx, int ny, int nz, float level, const void* counts_dev, const void* workspace,
                            size_t workspace_bytes) {
    if (!f || !counts_dev || !workspace) return EONERF_E_ARG;
    if (nx < 2 || ny < 2 || nz < 2) return EONERF_E_ARG;
    const uint64_t n = mesh_points(nx, ny, nz);
    if (!n) return EONERF_E_UNSUPPORTED;
    if (!isfinite(level)) return EONERF_E_ARG;
    if (workspace_bytes < dual_carve(n).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

inline int dual_check_lattice(int nx, int ny, int nz, float level, const float* origin, const float* spacing) {
    if (nx < 2 || ny < 2 || nz < 2) return EONERF_E_ARG;
    if (!mesh_points(nx, ny, nz)) return EONERF_E_UNSUPPORTED;
    if (!isfinite(level) || !mesh_finite3(origin) || !mesh_finite3(spacing)) return EONERF_E_ARG;
    if (spacing[0] == 0.f || spacing[1] == 0.f || spacing[2] == 0.f) return EONERF_E_ARG;
    return EONERF_OK;
}

inline int dual_check_hermite(const void* f, int nx, int ny, int nz, float level, const float* origin, const float* spacing,
                              const void* workspace, size_t workspace_bytes, const void* points, int64_t cap_h, const void* status_dev) {
    if (!f || !origin || !spacing || !workspace || !points || !status_dev) return EONERF_E_ARG;
    const int rc = dual_check_lattice(nx, ny, nz, level, origin, spacing);
    if (rc != EONERF_OK) return rc;
    if (cap_h < 0) return EONERF_E_ARG;
    if (workspace_bytes < dual_carve(mesh_points(nx, ny, nz)).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

inline int dual_check_emit(const void* f, int nx, int ny, int nz, float level, const float* origin, const float* spacing,
                           const void* gradient, int64_t n_gradient, float regularisation, const void* workspace, size_t workspace_bytes,
                           const void* vertices, int64_t cap_v, const void* triangles, int64_t cap_t, const void* report_dev,
                           const void* status_dev) {
    if (!f || !origin || !spacing || !gradient || !workspace || !vertices || !triangles || !report_dev || !status_dev) return EONERF_E_ARG;
    const int rc = dual_check_lattice(nx, ny, nz, level, origin, spacing);
    if (rc != EONERF_OK) return rc;
    if (!dual_regularisation_ok(regularisation)) return EONERF_E_ARG;
    if (cap_v < 0 || cap_t < 0 || n_gradient < 0) return EONERF_E_ARG;
    if (workspace_bytes < dual_carve(mesh_points(nx, ny, nz)).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// A corner of the unit cell is three bits, x = 1, y = 2, z = 4 (eonerf_mesh_check.h); the edge of slot a runs along the bit 1 << a.

// t on the edge from a to b: eonerf_mesh.h's rule (mesh_vertex forms the same expression)
DUAL_HD inline float dual_t(float fa, float fb, float level) {
    float t = 0.5f;
    if (mesh_is_finite(fa) && mesh_is_finite(fb)) {
        t = MESH_DIV(MESH_SUB(level, fa), MESH_SUB(fb, fa));
        if (!(t >= 0.f)) t = 0.f;
        if (t > 1.f) t = 1.f;
    }
    return t;
}

// whether the edge along axis a owned by point (i, j, k) has four cells around it
DUAL_HD inline bool dual_edge_quad(int a, int i, int j, int k, int nx, int ny, int nz) {
    const bool x = i >= 1 && i <= nx - 2, y = j >= 1 && j <= ny - 2, z = k >= 1 && k <= nz - 2;
    return a == 0 ? (y && z) : a == 1 ? (z && x) : (x && y);
}

// One lattice point (i, j, k) = p from the eight values at and above it: the mask of its owned crossing axis edges, how many of those
// have an end that is not finite, whether its cell is active and how many quads its edges give.  Reads no value outside the lattice.
struct DualPoint { unsigned mask, nonfinite, active, quads; };
DUAL_HD inline DualPoint dual_classify(const float* f, int nx, int ny, int nz, int i, int j, int k, unsigned p, float level) {
    const bool ex = i + 1 < nx, ey = j + 1 < ny, ez = k + 1 < nz;
    const unsigned unx = (unsigned)nx, nxy = (unsigned)nx * (unsigned)ny;
    float v[8];
    unsigned have = 0, in8 = 0;
    for (int c = 0; c < 8; ++c) {
        const bool ok = (!(c & 1) || ex) && (!(c & 2) || ey) && (!(c & 4) || ez);
        v[c] = 0.f;
        if (ok) {
            v[c] = f[p + mesh_corner_offset(c, unx, nxy)];
            have |= 1u << c;
            if (v[c] >= level) in8 |= 1u << c;
        }
    }
    DualPoint r;
    r.mask = r.nonfinite = r.quads = 0;
    r.active = (have == 0xffu && in8 != 0 && in8 != 0xffu) ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        const int d = 1 << a;
        if (((have >> d) & 1) && (((in8 >> d) ^ in8) & 1)) {
            r.mask |= 1u << a;
            if (!mesh_is_finite(v[0]) || !mesh_is_finite(v[d])) ++r.nonfinite;
            if (dual_edge_quad(a, i, j, k, nx, ny, nz)) ++r.quads;
        }
    }
    return r;
}

DUAL_HD inline unsigned dual_info(const DualPoint& r) { return r.mask | (r.active ? kDualActive : 0u) | (r.quads << kDualQuadShift); }

// the Hermite point on the edge that point (i, j, k) = p owns in slot a < 3: marching tetrahedra's own vertex, verbatim
DUAL_HD inline void dual_hermite_point(const float* f, int nx, int ny, int i, int j, int k, unsigned p, int a, float level, const float* origin,
                                       const float* spacing, float* out) {
    mesh_vertex(f, nx, ny, i, j, k, p, a, level, origin, spacing, out);
}

// cell edge e = 4a + 2v + u: the corner (three bits) of its owner in the cell
DUAL_HD inline int dual_edge_corner(int e) {
    const int a = e >> 2, v = (e >> 1) & 1, u = e & 1;
    const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;
    return (u << lo) | (v << hi);
}

DUAL_HD inline bool dual_is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }         // false for a NaN

// The vertex of the active cell whose lowest corner is p, in cell-local coordinates.  hermite_of(q, a): the id of the Hermite point on
// the edge point q owns in slot a.  A Hermite id outside [0, n_gradient) sets `beyond` and its plane is left out.
struct DualVertex { double x[3]; unsigned clamped, fallback, dropped, beyond; };
template <class HermiteOf>
DUAL_HD inline DualVertex dual_cell_vertex(const float* f, int nx, int ny, unsigned p, float level, const float* spacing, double lambda,
                                           const float* gradient, int64_t n_gradient, const HermiteOf& hermite_of) {
    const unsigned unx = (unsigned)nx, nxy = (unsigned)nx * (unsigned)ny;
    float v[8];
    unsigned in8 = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = f[p + mesh_corner_offset(c, unx, nxy)];
        if (v[c] >= level) in8 |= 1u << c;
    }
    DualVertex r;
    r.clamped = r.fallback = r.dropped = r.beyond = 0;
    double t[12], sum[3] = {0.0, 0.0, 0.0}, m[3];
    unsigned crossing = 0;
    int count = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int a = e >> 2, corner = dual_edge_corner(e), far = corner | (1 << a);
        t[e] = 0.0;
        if (((in8 >> corner) ^ (in8 >> far)) & 1) {
            crossing |= 1u << e;
            ++count;
            t[e] = (double)dual_t(v[corner], v[far], level);
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] = DUAL_ADD(sum[c], c == a ? t[e] : (double)((corner >> c) & 1));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = DUAL_DIV(sum[c], (double)count);
    const double lam2 = DUAL_MUL(lambda, lambda);
    double a00 = lam2, a01 = 0.0, a02 = 0.0, a11 = lam2, a12 = 0.0, a22 = lam2, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!((crossing >> e) & 1)) continue;
        const int a = e >> 2, corner = dual_edge_corner(e);
        const int64_t id = hermite_of(p + mesh_corner_offset(corner, unx, nxy), a);
        if (id < 0 || id >= n_gradient) { r.beyond = 1; continue; }
        const float g0 = gradient[3 * id], g1 = gradient[3 * id + 1], g2 = gradient[3 * id + 2];
        if (!mesh_is_finite(g0) || !mesh_is_finite(g1) || !mesh_is_finite(g2)) { ++r.dropped; continue; }
        const double G0 = DUAL_MUL((double)g0, (double)spacing[0]), G1 = DUAL_MUL((double)g1, (double)spacing[1]),
                     G2 = DUAL_MUL((double)g2, (double)spacing[2]);
        const double s = DUAL_ADD(DUAL_ADD(DUAL_MUL(G0, G0), DUAL_MUL(G1, G1)), DUAL_MUL(G2, G2));
        if (!(s > 0.0)) { ++r.dropped; continue; }
        const double d0 = DUAL_SUB(a == 0 ? t[e] : (double)(corner & 1), m[0]), d1 = DUAL_SUB(a == 1 ? t[e] : (double)((corner >> 1) & 1), m[1]),
                     d2 = DUAL_SUB(a == 2 ? t[e] : (double)((corner >> 2) & 1), m[2]);
        const double dot = DUAL_ADD(DUAL_ADD(DUAL_MUL(G0, d0), DUAL_MUL(G1, d1)), DUAL_MUL(G2, d2));
        a00 = DUAL_ADD(a00, DUAL_DIV(DUAL_MUL(G0, G0), s));
        a01 = DUAL_ADD(a01, DUAL_DIV(DUAL_MUL(G0, G1), s));
        a02 = DUAL_ADD(a02, DUAL_DIV(DUAL_MUL(G0, G2), s));
        a11 = DUAL_ADD(a11, DUAL_DIV(DUAL_MUL(G1, G1), s));
        a12 = DUAL_ADD(a12, DUAL_DIV(DUAL_MUL(G1, G2), s));
        a22 = DUAL_ADD(a22, DUAL_DIV(DUAL_MUL(G2, G2), s));
        b0 = DUAL_ADD(b0, DUAL_DIV(DUAL_MUL(G0, dot), s));
        b1 = DUAL_ADD(b1, DUAL_DIV(DUAL_MUL(G1, dot), s));
        b2 = DUAL_ADD(b2, DUAL_DIV(DUAL_MUL(G2, dot), s));
    }
    // LDL^T: no square root, no pivoting
    const double d0 = a00, l10 = DUAL_DIV(a01, d0), l20 = DUAL_DIV(a02, d0);
    const double d1 = DUAL_SUB(a11, DUAL_MUL(l10, a01));
    const double t21 = DUAL_SUB(a12, DUAL_MUL(l20, a01));
    const double l21 = DUAL_DIV(t21, d1);
    const double d2 = DUAL_SUB(DUAL_SUB(a22, DUAL_MUL(l20, a02)), DUAL_MUL(l21, t21));
    const double y0 = b0, y1 = DUAL_SUB(b1, DUAL_MUL(l10, y0));
    const double y2 = DUAL_SUB(DUAL_SUB(b2, DUAL_MUL(l20, y0)), DUAL_MUL(l21, y1));
    const double z0 = DUAL_DIV(y0, d0), z1 = DUAL_DIV(y1, d1), z2 = DUAL_DIV(y2, d2);
    const double x2 = z2, x1 = DUAL_SUB(z1, DUAL_MUL(l21, x2));
    const double x0 = DUAL_SUB(DUAL_SUB(z0, DUAL_MUL(l10, x1)), DUAL_MUL(l20, x2));
    r.x[0] = DUAL_ADD(m[0], x0);
    r.x[1] = DUAL_ADD(m[1], x1);
    r.x[2] = DUAL_ADD(m[2], x2);
    if (!dual_is_finite(r.x[0]) || !dual_is_finite(r.x[1]) || !dual_is_finite(r.x[2])) {
        r.fallback = 1;
        r.x[0] = m[0]; r.x[1] = m[1]; r.x[2] = m[2];
        return r;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (r.x[c] < 0.0) { r.x[c] = 0.0; r.clamped = 1; }
        if (r.x[c] > 1.0) { r.x[c] = 1.0; r.clamped = 1; }
    }
    return r;
}

// cell-local vertex -> position by the coordinate rule
DUAL_HD inline void dual_vertex_position(const DualVertex& r, int i, int j, int k, const float* origin, const float* spacing, float* out) {
    out[0] = mesh_position(origin[0], spacing[0], i, (float)r.x[0]);
    out[1] = mesh_position(origin[1], spacing[1], j, (float)r.x[1]);
    out[2] = mesh_position(origin[2], spacing[2], k, (float)r.x[2]);
}

// the quads of point (i, j, k) = p with edge mask `mask`, in slot order, as triangles from index tri0 on: put(index, a, b, c) with
// a, b, c = vertex_of(cell index); owner_inside: f[p] >= level
template <class VertexOf, class Put>
DUAL_HD inline void dual_point_quads(unsigned mask, bool owner_inside, int nx, int ny, int nz, int i, int j, int k, unsigned p, uint64_t tri0,
                                     const VertexOf& vertex_of, const Put& put) {
    const unsigned step[3] = {1u, (unsigned)nx, (unsigned)nx * (unsigned)ny};
    uint64_t at = tri0;
    for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1) || !dual_edge_quad(a, i, j, k, nx, ny, nz)) continue;
        const unsigned s1 = step[(a + 1) % 3], s2 = step[(a + 2) % 3];
        int32_t r0 = vertex_of(p - s1 - s2), r1 = vertex_of(p - s2), r2 = vertex_of(p), r3 = vertex_of(p - s1);
        if (!owner_inside) {
            int32_t w = r0; r0 = r3; r3 = w;
            w = r1; r1 = r2; r2 = w;
        }
        put(at, r0, r1, r2);
        put(at + 1, r0, r2, r3);
        at += 2;
    }
}
