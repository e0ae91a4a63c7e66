// Host side of include/eonerf_mesh_dsm.h: the refusals of the two entry points in their documented order, in a function with no HIP call
// so that a stand-alone program can include it (tests/host/mesh_dsm_checks.cpp).  It returns 0 or the EONERF_E_* the entry point returns
// before it launches anything.
// The rule itself -- the vertex snap, the drop test, the triangle setup, the bounding box, coverage and altitude at one sample, the key
// -- is here too, as functions the kernels of eonerf_mesh_dsm.hip call per lane and the stand-alone program calls in a loop: one
// statement of the rule for the device and for the host check.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_mesh_dsm.h"

#if defined(__HIPCC__)
#define MDSM_HD __host__ __device__
#else
#define MDSM_HD
#endif
// one fp64 operation each, never contracted: the device intrinsics say so themselves, the host build has no fused form to contract to
#if defined(__HIP_DEVICE_COMPILE__)
#define MDSM_ADD(a, b) __dadd_rn((a), (b))
#define MDSM_SUB(a, b) __dadd_rn((a), -(b))
#define MDSM_MUL(a, b) __dmul_rn((a), (b))
#define MDSM_DIV(a, b) __ddiv_rn((a), (b))
#else
#define MDSM_ADD(a, b) ((a) + (b))
#define MDSM_SUB(a, b) ((a) - (b))
#define MDSM_MUL(a, b) ((a) * (b))
#define MDSM_DIV(a, b) ((a) / (b))
#endif

constexpr int kMdsmBlock = 256;                                         // threads of every kernel of the group: four waves
constexpr int kMdsmSub = 1 << EONERF_MESH_DSM_SUBPIXEL_BITS;            // sub-pixels per cell
constexpr int kMdsmHalf = kMdsmSub / 2;                                 // a cell centre
constexpr int64_t kMdsmLaneCells = EONERF_MESH_DSM_LANE_CELLS;

// ---- refusals ---------------------------------------------------------------------------------------------------------------------
// One order for both entry points.  `required`: every pointer the call may not have null, any_null = one of them is.
inline int mdsm_check(bool any_null, int64_t n_vertices, int64_t n_triangles, const double* scale, const double* offset, double xoff,
                      double yoff, int xsize, int ysize, double res, int channels) {
    if (any_null || !scale || !offset) return EONERF_E_ARG;
    if (xsize < 1 || ysize < 1) return EONERF_E_ARG;
    if (n_vertices < 0 || n_triangles < 0) return EONERF_E_ARG;
    if (channels < 1 || channels > EONERF_MESH_DSM_MAX_CHANNELS) return EONERF_E_ARG;
    if (xsize > EONERF_MESH_DSM_MAX_SIZE || ysize > EONERF_MESH_DSM_MAX_SIZE || n_vertices > (int64_t)INT32_MAX || n_triangles > (int64_t)INT32_MAX)
        return EONERF_E_UNSUPPORTED;
    if (!isfinite(res) || !isfinite(xoff) || !isfinite(yoff) || !(res > 0.0)) return EONERF_E_ARG;
    for (int c = 0; c < 3; ++c)
        if (!isfinite(scale[c]) || !isfinite(offset[c]) || scale[c] == 0.0) return EONERF_E_ARG;
    return EONERF_OK;
}

inline int mdsm_check_rasterize(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* scale,
                                const double* offset, double xoff, double yoff, int xsize, int ysize, double res, const void* keys,
                                const void* dsm, const void* counts_dev) {
    return mdsm_check(!vertices || !triangles || !keys || !dsm || !counts_dev, n_vertices, n_triangles, scale, offset, xoff, yoff, xsize, ysize,
                      res, 1);
}

inline int mdsm_check_attributes(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double* scale,
                                 const double* offset, double xoff, double yoff, int xsize, int ysize, double res, const void* face,
                                 const void* attr, int channels, const void* out) {
    return mdsm_check(!vertices || !triangles || !face || !attr || !out, n_vertices, n_triangles, scale, offset, xoff, yoff, xsize, ysize, res,
                      channels);
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
struct MdsmGrid { double scale[3], offset[3], xoff, yoff, res; int xsize, ysize; };

MDSM_HD inline int64_t mdsm_floor_div(int64_t a, int64_t b) {          // b > 0
    const int64_t q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

// a vertex in fixed point; ok = false where it drops its triangles (X and Y are then 0)
struct MdsmVertex { int64_t X, Y; double z; bool ok; };
MDSM_HD inline MdsmVertex mdsm_vertex(const MdsmGrid& g, const float* v) {
    const double east = MDSM_ADD(MDSM_MUL((double)v[0], g.scale[0]), g.offset[0]);
    double north = MDSM_ADD(MDSM_MUL((double)v[1], g.scale[1]), g.offset[1]);
    const double alt = MDSM_ADD(MDSM_MUL((double)v[2], g.scale[2]), g.offset[2]);
    if (north < 0.0) north = MDSM_ADD(north, 10e6);
    const double fx = MDSM_MUL(MDSM_DIV(MDSM_SUB(east, g.xoff), g.res), (double)kMdsmSub);
    const double fy = MDSM_MUL(MDSM_DIV(MDSM_SUB(g.yoff, north), g.res), (double)kMdsmSub);
    MdsmVertex r;
    r.z = alt;
    // every comparison is false for a NaN: a coordinate that is not finite fails the first two, such an altitude the third
    r.ok = fabs(fx) <= (double)EONERF_MESH_DSM_MAX_COORD && fabs(fy) <= (double)EONERF_MESH_DSM_MAX_COORD && fabs(alt) < (double)EONERF_MESH_DSM_MAX_ALTITUDE;
    r.X = r.ok ? (int64_t)llrint(fx) : 0;
    r.Y = r.ok ? (int64_t)llrint(fy) : 0;
    return r;
}

enum { MDSM_KEEP = 0, MDSM_DROPPED = 1, MDSM_DEGENERATE = 2 };

// a triangle ready for its samples: the vertices, s * A2 = |A2| with s folded into `sign`, and its box of cells clamped to the grid
// (i0 > i1 or j0 > j1: no cell)
struct MdsmTri { int64_t X[3], Y[3]; double z[3]; int64_t area; int sign, state; int i0, i1, j0, j1; };

MDSM_HD inline int64_t mdsm_edge(int64_t xa, int64_t ya, int64_t xb, int64_t yb, int64_t px, int64_t py) {
    return (xb - xa) * (py - ya) - (yb - ya) * (px - xa);
}

MDSM_HD inline int64_t mdsm_min3(int64_t a, int64_t b, int64_t c) { const int64_t m = a < b ? a : b; return m < c ? m : c; }
MDSM_HD inline int64_t mdsm_max3(int64_t a, int64_t b, int64_t c) { const int64_t m = a > b ? a : b; return m > c ? m : c; }

MDSM_HD inline MdsmTri mdsm_setup(const MdsmGrid& g, const float* vertices, int64_t n_vertices, const int32_t* tri) {
    MdsmTri t;
    t.state = MDSM_DROPPED;
    t.area = 0; t.sign = 1; t.i0 = t.j0 = 0; t.i1 = t.j1 = -1;
    for (int k = 0; k < 3; ++k) { t.X[k] = t.Y[k] = 0; t.z[k] = 0.0; }
    const int32_t a = tri[0], b = tri[1], c = tri[2];
    if (a < 0 || b < 0 || c < 0 || (int64_t)a >= n_vertices || (int64_t)b >= n_vertices || (int64_t)c >= n_vertices) return t;
    const int32_t id[3] = {a, b, c};
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const MdsmVertex v = mdsm_vertex(g, vertices + (size_t)id[k] * 3);
        t.X[k] = v.X; t.Y[k] = v.Y; t.z[k] = v.z;
        ok = ok && v.ok;
    }
    if (!ok) return t;
    const int64_t a2 = mdsm_edge(t.X[0], t.Y[0], t.X[1], t.Y[1], t.X[2], t.Y[2]);
    if (a2 == 0) { t.state = MDSM_DEGENERATE; return t; }
    t.state = MDSM_KEEP;
    t.sign = a2 > 0 ? 1 : -1;
    t.area = a2 > 0 ? a2 : -a2;
    // columns whose centre 4096 i + 2048 lies in [min X, max X]: ceil((min X - 2048) / 4096) .. floor((max X - 2048) / 4096)
    const int64_t i0 = mdsm_floor_div(mdsm_min3(t.X[0], t.X[1], t.X[2]) + (kMdsmHalf - 1), kMdsmSub);
    const int64_t i1 = mdsm_floor_div(mdsm_max3(t.X[0], t.X[1], t.X[2]) - kMdsmHalf, kMdsmSub);
    const int64_t j0 = mdsm_floor_div(mdsm_min3(t.Y[0], t.Y[1], t.Y[2]) + (kMdsmHalf - 1), kMdsmSub);
    const int64_t j1 = mdsm_floor_div(mdsm_max3(t.Y[0], t.Y[1], t.Y[2]) - kMdsmHalf, kMdsmSub);
    t.i0 = (int)(i0 < 0 ? 0 : i0 > g.xsize ? g.xsize : i0);
    t.i1 = (int)(i1 >= g.xsize ? g.xsize - 1 : i1 < -1 ? -1 : i1);
    t.j0 = (int)(j0 < 0 ? 0 : j0 > g.ysize ? g.ysize : j0);
    t.j1 = (int)(j1 >= g.ysize ? g.ysize - 1 : j1 < -1 ? -1 : j1);
    return t;
}

// cells of the clamped box (0 where it is empty)
MDSM_HD inline int64_t mdsm_box_cells(const MdsmTri& t) {
    if (t.state != MDSM_KEEP || t.i1 < t.i0 || t.j1 < t.j0) return 0;
    return (int64_t)(t.i1 - t.i0 + 1) * (int64_t)(t.j1 - t.j0 + 1);
}

// the weights of the three vertices at the centre of cell (j, i); true iff the cell is covered
MDSM_HD inline bool mdsm_weights(const MdsmTri& t, int i, int j, int64_t w[3]) {
    const int64_t px = (int64_t)kMdsmSub * i + kMdsmHalf, py = (int64_t)kMdsmSub * j + kMdsmHalf;
    w[0] = t.sign * mdsm_edge(t.X[1], t.Y[1], t.X[2], t.Y[2], px, py);
    w[1] = t.sign * mdsm_edge(t.X[2], t.Y[2], t.X[0], t.Y[0], px, py);
    w[2] = t.sign * mdsm_edge(t.X[0], t.Y[0], t.X[1], t.Y[1], px, py);
    return w[0] >= 0 && w[1] >= 0 && w[2] >= 0;
}

// a per-vertex quantity at the sample
MDSM_HD inline double mdsm_interpolate(const int64_t w[3], int64_t area, double a0, double a1, double a2) {
    const double s = MDSM_ADD(MDSM_ADD(MDSM_MUL((double)w[0], a0), MDSM_MUL((double)w[1], a1)), MDSM_MUL((double)w[2], a2));
    return MDSM_DIV(s, (double)area);
}

MDSM_HD inline int64_t mdsm_quantise(double z) {
    const double f = MDSM_MUL(z, 65536.0);
    if (!(f > -2147483648.0)) return -2147483648LL;             // (a NaN cannot come from a kept triangle; it would land here)
    if (f >= 2147483647.0) return 2147483647LL;
    return (int64_t)llrint(f);
}

MDSM_HD inline uint64_t mdsm_key(int64_t q, uint32_t face) {
    return ((uint64_t)(uint32_t)(q + 2147483648LL) << 32) | (uint64_t)(0xFFFFFFFFu - face);
}
MDSM_HD inline float mdsm_key_altitude(uint64_t key) {
    const int64_t q = (int64_t)(key >> 32) - 2147483648LL;
    return (float)MDSM_DIV((double)q, 65536.0);
}
MDSM_HD inline int32_t mdsm_key_face(uint64_t key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu)); }

// the key of triangle `face` at cell (j, i), or 0 where it does not cover the cell
MDSM_HD inline uint64_t mdsm_sample(const MdsmTri& t, uint32_t face, int i, int j) {
    int64_t w[3];
    if (!mdsm_weights(t, i, j, w)) return 0;
    return mdsm_key(mdsm_quantise(mdsm_interpolate(w, t.area, t.z[0], t.z[1], t.z[2])), face);
}
