// Host side of include/eonerf_mesh.h: the refusals of the entry points in their documented order, the size arithmetic (64-bit) and the
// workspace carve, in functions with no HIP call so that a stand-alone program can include them (tests/host/mesh_checks.cpp).  Each
// check returns 0 or the EONERF_E_* the entry point returns before it launches anything.
// The rule itself -- the case table, the classification of one lattice point, one vertex, the triangles of one cell -- is here too, as
// functions the kernels of eonerf_mesh.hip call per thread and the stand-alone program calls in a loop: one statement of the rule for
// the device and for the host check.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_mesh.h"

#if defined(__HIPCC__)
#define MESH_HD __host__ __device__
#else
#define MESH_HD
#endif
// one fp32 operation each, never contracted: the device intrinsics say so themselves, the host build has no fused form to contract to
#if defined(__HIP_DEVICE_COMPILE__)
#define MESH_SUB(a, b) __fsub_rn((a), (b))
#define MESH_ADD(a, b) __fadd_rn((a), (b))
#define MESH_MUL(a, b) __fmul_rn((a), (b))
#define MESH_DIV(a, b) __fdiv_rn((a), (b))
#else
#define MESH_SUB(a, b) ((a) - (b))
#define MESH_ADD(a, b) ((a) + (b))
#define MESH_MUL(a, b) ((a) * (b))
#define MESH_DIV(a, b) ((a) / (b))
#endif

constexpr int kMeshBlock = 256;                       // threads of every mesh kernel
constexpr int kMeshTile = EONERF_MESH_TILE;           // points (or sums) one workgroup scans: kMeshBlock threads x kMeshRounds
constexpr int kMeshRounds = kMeshTile / kMeshBlock;

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// points of an nx x ny x nz lattice in 64 bits; 0 for a dimension below 2 or more points than a call takes (no product can wrap: each
// partial product is checked against the limit first)
inline uint64_t mesh_points(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const uint64_t lim = (uint64_t)EONERF_MESH_MAX_POINTS;
    if ((uint64_t)nx > lim || (uint64_t)ny > lim || (uint64_t)nz > lim) return 0;
    const uint64_t xy = (uint64_t)nx * (uint64_t)ny;
    if (xy > lim) return 0;
    const uint64_t n = xy * (uint64_t)nz;
    return n > lim ? 0 : n;
}

// the slab of eonerf_mesh_lattice_points: any dimension from 1 up
inline uint64_t mesh_slab_points(int64_t nx, int64_t ny, int64_t z0, int64_t nz) {
    if (nx < 1 || ny < 1 || nz < 1 || z0 < 0) return 0;
    const uint64_t lim = (uint64_t)EONERF_MESH_MAX_POINTS;
    if ((uint64_t)nx > lim || (uint64_t)ny > lim || (uint64_t)nz > lim || (uint64_t)z0 + (uint64_t)nz > lim) return 0;
    const uint64_t xy = (uint64_t)nx * (uint64_t)ny;
    if (xy > lim) return 0;
    const uint64_t n = xy * (uint64_t)nz;
    return n > lim ? 0 : n;
}

// the workspace: per point lv (uint16), lt (uint16), mask (uint8); per tile / per kMeshTile tiles / once the sums (two uint32 each)
struct MeshCarve { uint64_t n, n1, n2; size_t lv_off, lt_off, mask_off, l1_off, l2_off, l3_off, bytes; };
inline MeshCarve mesh_carve(uint64_t n) {
    MeshCarve c;
    c.n = n;
    c.n1 = (n + kMeshTile - 1) / kMeshTile;
    c.n2 = (c.n1 + kMeshTile - 1) / kMeshTile;             // <= kMeshTile while n <= kMeshTile^3: the third level is one sum
    uint64_t off = 0;
    auto take = [&off](uint64_t bytes) { const uint64_t at = off; off = (off + bytes + 255) & ~(uint64_t)255; return (size_t)at; };
    c.lv_off = take(2 * n);
    c.lt_off = take(2 * n);
    c.mask_off = take(n);
    c.l1_off = take(8 * c.n1);
    c.l2_off = take(8 * c.n2);
    c.l3_off = take(8);
    c.bytes = (size_t)off;
    return c;
}
static_assert((uint64_t)EONERF_MESH_MAX_POINTS <= (uint64_t)kMeshTile * kMeshTile * kMeshTile, "three scan levels cover a call");
static_assert(7 * kMeshTile <= 65535 && 12 * kMeshTile <= 65535, "the scans inside a tile are uint16");

inline bool mesh_finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

inline int mesh_check_lattice(const float* origin, const float* spacing, int nx, int ny, int z0, int nz, const void* xyz_out) {
    if (!origin || !spacing || !xyz_out) return EONERF_E_ARG;
    if (nx < 1 || ny < 1 || nz < 1 || z0 < 0) return EONERF_E_ARG;
    if (!mesh_slab_points(nx, ny, z0, nz)) return EONERF_E_UNSUPPORTED;
    if (!mesh_finite3(origin) || !mesh_finite3(spacing)) return EONERF_E_ARG;
    if (spacing[0] == 0.f || spacing[1] == 0.f || spacing[2] == 0.f) return EONERF_E_ARG;
    return EONERF_OK;
}

inline int mesh_check_count(const void* f, int nx, int ny, int nz, float level, const void* counts_dev, const void* workspace,
                            size_t workspace_bytes) {
    if (!f || !counts_dev || !workspace) return EONERF_E_ARG;
    if (nx < 2 || ny < 2 || nz < 2) return EONERF_E_ARG;
    const uint64_t n = mesh_points(nx, ny, nz);
    if (!n) return EONERF_E_UNSUPPORTED;
    if (!isfinite(level)) return EONERF_E_ARG;
    if (workspace_bytes < mesh_carve(n).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

inline int mesh_check_emit(const void* f, int nx, int ny, int nz, float level, const float* origin, const float* spacing,
                           const void* workspace, size_t workspace_bytes, const void* vertices, int64_t cap_v, const void* triangles,
                           int64_t cap_t, const void* status_dev) {
    if (!f || !origin || !spacing || !workspace || !vertices || !triangles || !status_dev) return EONERF_E_ARG;
    if (nx < 2 || ny < 2 || nz < 2) return EONERF_E_ARG;
    const uint64_t n = mesh_points(nx, ny, nz);
    if (!n) return EONERF_E_UNSUPPORTED;
    if (!isfinite(level) || !mesh_finite3(origin) || !mesh_finite3(spacing)) return EONERF_E_ARG;
    if (spacing[0] == 0.f || spacing[1] == 0.f || spacing[2] == 0.f) return EONERF_E_ARG;
    if (cap_v < 0 || cap_t < 0) return EONERF_E_ARG;
    if (workspace_bytes < mesh_carve(n).bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// A corner of the unit cell, and the direction of an edge, are three bits: x = 1, y = 2, z = 4.
MESH_HD inline int mesh_slot_dir(int slot) { return (0x7653421 >> (4 * slot)) & 7; }          // slots 0..6: 100 010 001 110 101 011 111
MESH_HD inline int mesh_dir_slot(int dir) { return (0x65423100u >> (4 * dir)) & 7; }

// corner[t][c]: corner c of tetrahedron t.  ref[t][m][3 * q + r]: vertex r of triangle q of tetrahedron t in case m (bit c of m: corner c
// is inside) as (owning corner) | (slot << 3); a case has 0 (m = 0, 15), 2 (two corners inside) or 1 triangle.
struct MeshTable { uint8_t corner[6][4]; uint8_t ref[6][16][6]; };

constexpr MeshTable mesh_make_table() {
    MeshTable T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int dir_slot[8] = {0, 0, 1, 3, 2, 4, 5, 6};
    for (int t = 0; t < 6; ++t) {
        T.corner[t][0] = 0;
        for (int c = 1; c < 4; ++c) T.corner[t][c] = (uint8_t)(T.corner[t][c - 1] | (1 << perm[t][c - 1]));
        for (int m = 1; m < 15; ++m) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int c = 0; c < 4; ++c) {
                if ((m >> c) & 1) in[ni++] = c;
                else out[no++] = c;
            }
            int tri[2][3][2] = {};          // [triangle][vertex][the two corners of its edge]
            int nt = 1;
            if (ni == 1) {
                for (int r = 0; r < 3; ++r) { tri[0][r][0] = in[0]; tri[0][r][1] = out[r]; }
            } else if (ni == 3) {
                for (int r = 0; r < 3; ++r) { tri[0][r][0] = out[0]; tri[0][r][1] = in[r]; }
            } else {
                nt = 2;
                const int p = in[0], q = in[1], r = out[0], s = out[1];
                tri[0][0][0] = p; tri[0][0][1] = r; tri[0][1][0] = p; tri[0][1][1] = s; tri[0][2][0] = q; tri[0][2][1] = s;
                tri[1][0][0] = p; tri[1][0][1] = r; tri[1][1][0] = q; tri[1][1][1] = s; tri[1][2][0] = q; tri[1][2][1] = r;
            }
            // from the outside corners towards the inside ones, times ni * no: no * sum(inside) - ni * sum(outside)
            int towards_in[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                for (int c = 0; c < ni; ++c) towards_in[a] += no * ((T.corner[t][in[c]] >> a) & 1);
                for (int c = 0; c < no; ++c) towards_in[a] -= ni * ((T.corner[t][out[c]] >> a) & 1);
            }
            for (int q = 0; q < nt; ++q) {
                int mid[3][3] = {};         // twice the midpoint of each vertex' edge
                for (int r = 0; r < 3; ++r)
                    for (int a = 0; a < 3; ++a)
                        mid[r][a] = ((T.corner[t][tri[q][r][0]] >> a) & 1) + ((T.corner[t][tri[q][r][1]] >> a) & 1);
                int e1[3] = {}, e2[3] = {};
                for (int a = 0; a < 3; ++a) { e1[a] = mid[1][a] - mid[0][a]; e2[a] = mid[2][a] - mid[0][a]; }
                const int nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                const int dot = nrm[0] * towards_in[0] + nrm[1] * towards_in[1] + nrm[2] * towards_in[2];
                uint8_t refs[3] = {};
                for (int r = 0; r < 3; ++r) {
                    const int u = tri[q][r][0] < tri[q][r][1] ? tri[q][r][0] : tri[q][r][1];
                    const int v = tri[q][r][0] < tri[q][r][1] ? tri[q][r][1] : tri[q][r][0];
                    const int owner = T.corner[t][u], dir = T.corner[t][v] ^ T.corner[t][u];
                    refs[r] = (uint8_t)(owner | (dir_slot[dir] << 3));
                }
                T.ref[t][m][3 * q] = refs[0];
                T.ref[t][m][3 * q + 1] = dot > 0 ? refs[2] : refs[1];
                T.ref[t][m][3 * q + 2] = dot > 0 ? refs[1] : refs[2];
            }
        }
    }
    return T;
}

MESH_HD inline bool mesh_is_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }           // false for a NaN
MESH_HD inline unsigned mesh_corner_offset(int corner, unsigned nx, unsigned nxy) {
    return (unsigned)(corner & 1) + (unsigned)((corner >> 1) & 1) * nx + (unsigned)((corner >> 2) & 1) * nxy;
}
// triangles of a tetrahedron whose case has `inside` corners inside
MESH_HD inline unsigned mesh_case_triangles(int inside) { return inside == 2 ? 2u : (inside == 1 || inside == 3) ? 1u : 0u; }

// the 4-bit case of tetrahedron t from the cell's 8-bit inside mask (bit = corner)
MESH_HD inline int mesh_tet_case(const MeshTable& T, int t, unsigned in8) {
    return (int)(((in8 >> T.corner[t][0]) & 1) | (((in8 >> T.corner[t][1]) & 1) << 1) | (((in8 >> T.corner[t][2]) & 1) << 2) |
                 (((in8 >> T.corner[t][3]) & 1) << 3));
}

// One lattice point (i, j, k) = p from the eight values at and above it: the mask of its owned crossing edges, how many of those have
// an end that is not finite, and the triangle count of its cell (0 where it has none).  Reads no value outside the lattice.
struct MeshPoint { unsigned mask, nonfinite, triangles, in8; bool cell; };
MESH_HD inline MeshPoint mesh_classify(const MeshTable& T, const float* f, int nx, int ny, int nz, int i, int j, int k, unsigned p, float level) {
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
    MeshPoint r;
    r.mask = r.nonfinite = r.triangles = 0;
    r.in8 = in8;
    r.cell = have == 0xffu;
    for (int s = 0; s < 7; ++s) {
        const int d = mesh_slot_dir(s);
        if (((have >> d) & 1) && (((in8 >> d) ^ in8) & 1)) {
            r.mask |= 1u << s;
            if (!mesh_is_finite(v[0]) || !mesh_is_finite(v[d])) ++r.nonfinite;
        }
    }
    if (r.cell && in8 != 0 && in8 != 0xffu)
        for (int t = 0; t < 6; ++t) r.triangles += mesh_case_triangles(__builtin_popcount((unsigned)mesh_tet_case(T, t, in8)));
    return r;
}

// lattice coordinate -> position: the one coordinate rule
MESH_HD inline float mesh_position(float origin, float spacing, int index, float t) {
    return MESH_ADD(origin, MESH_MUL(spacing, MESH_ADD((float)index, t)));
}

// the vertex on the edge that point (i, j, k) = p owns in `slot`
MESH_HD inline void mesh_vertex(const float* f, int nx, int ny, int i, int j, int k, unsigned p, int slot, float level, const float* origin,
                                const float* spacing, float* out) {
    const int d = mesh_slot_dir(slot);
    const float fa = f[p], fb = f[p + mesh_corner_offset(d, (unsigned)nx, (unsigned)nx * (unsigned)ny)];
    float t = 0.5f;
    if (mesh_is_finite(fa) && mesh_is_finite(fb)) {
        t = MESH_DIV(MESH_SUB(level, fa), MESH_SUB(fb, fa));
        if (!(t >= 0.f)) t = 0.f;
        if (t > 1.f) t = 1.f;
    }
    out[0] = mesh_position(origin[0], spacing[0], i, (d & 1) ? t : 0.f);
    out[1] = mesh_position(origin[1], spacing[1], j, (d & 2) ? t : 0.f);
    out[2] = mesh_position(origin[2], spacing[2], k, (d & 4) ? t : 0.f);
}

// the triangles of one cell, in order, from index tri0 on: put(index, a, b, c) with a, b, c = id_of(owning corner, slot)
template <class IdOf, class Put>
MESH_HD inline void mesh_cell_triangles(const MeshTable& T, unsigned in8, uint64_t tri0, const IdOf& id_of, const Put& put) {
    uint64_t at = tri0;
    for (int t = 0; t < 6; ++t) {
        const int m = mesh_tet_case(T, t, in8);
        const unsigned nt = mesh_case_triangles(__builtin_popcount((unsigned)m));
        for (unsigned q = 0; q < nt; ++q) {
            const uint8_t* r = T.ref[t][m] + 3 * q;
            const int32_t a = id_of(r[0] & 7, r[0] >> 3), b = id_of(r[1] & 7, r[1] >> 3), c = id_of(r[2] & 7, r[2] >> 3);
            put(at++, a, b, c);
        }
    }
}
