/* eonerf_raycast.h -- STAGED public header (it moves to include/ and its bindings into _lib.API in the follow-up that counts it among
 * the public headers; until then the bindings are _lib.API_STAGED_RAYCAST and tests/test_raycast_abi_cpu.py holds them to this file).
 *
 * Ray casting against a triangle mesh: per ray the closest hit (t, face, barycentric weights) or whether anything blocks it.  Entry
 * points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_smooth.h: plain C, raw DEVICE pointers, HOST double[3] / int[3] for the box and the grid, a
 * hipStream_t passed as void*, the caller owns every buffer, every call is asynchronous on `stream`, nothing is allocated, nothing
 * synchronises and nothing is read back.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.  The group is
 * stateless: it takes no context.  Every output but the order inside a cell list is a pure function of the arguments: the grid below
 * only decides which triangles a ray is tested against, and the result is DEFINED without it -- the minimum over all live triangles
 * (tests/raycast_restated.py is that brute force in numpy).  All arithmetic of the rule is fp64, one IEEE operation at a time, never
 * contracted.
 *
 * THE RULE.
 *   BOX  lo[3], hi[3]: HOST doubles, finite, lo < hi per axis.
 *   TRIANGLE  DROPPED (counted, never tested) iff an index is outside [0, n_vertices), a vertex coordinate is not finite, or a vertex
 *     lies outside the closed box (its fp32 coordinate widened to fp64 is < lo or > hi).  Every other triangle is LIVE.  Nothing else
 *     is special: zero-area triangles simply never hit.
 *   RAY  o, d: fp32 triples widened to fp64.  t_min, t_max: per-call HOST doubles, 0 <= t_min <= t_max, t_max possibly +inf.  A ray is
 *     REJECTED (counted, reported as a miss) iff a component of o or d is not finite or d is the zero vector; decided before any loop.
 *   AXES  kz = the axis of the largest |d_c|, ties to the smallest index; kx = (kz + 1) % 3, ky = (kx + 1) % 3, the two swapped if
 *     d[kz] < 0.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz], each correctly rounded.
 *   SHEAR  per vertex v: P = (double)v - o, one subtraction per axis; x = P[kx] - Sx * P[kz], y = P[ky] - Sy * P[kz], z = Sz * P[kz]
 *     -- one product and one subtraction each.
 *   EDGE FUNCTIONS  for the corners A, B, C in the order the face lists them: U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax
 *     -- two products and one subtraction each.
 *   COVER  the ray covers the triangle iff U, V, W are all >= 0 or all <= 0.  Then det = (U + V) + W; det == 0 is no hit.  Every edge
 *     is inclusive, and the two triangles that share an edge compute its function from the same two sheared vertices with exactly
 *     negated value: a closed mesh has no crack, and a double hit is harmless under a minimum.
 *   DEPTH  t = ((U Az + V Bz) + W Cz) / det.  A HIT iff t is finite and t_min <= t <= t_max.  t is the ray's own parameter
 *     (o + t d, d not normalised).
 *   CLOSEST  per ray the lexicographic minimum of (t, face) over the live triangles that hit.  t_out fp64 (NaN on a miss), face_out
 *     int32 (-1), bary_out fp32 x 3 = U / det, V / det, W / det, each rounded once to fp64 and once to fp32: the weights of A, B, C
 *     (NaN).
 *   OCCLUDED  per ray one byte: 1 iff some live triangle f != skip[r] hits in [t_min, t_max]; skip is an int32 per ray, or NULL.
 *   COUNTS  eonerf_raycast_count: counts_dev[2] = list entries of the grid, triangles dropped.  The casts: counts_dev[3] = rays cast
 *     (n_rays), rays rejected, hits (closest: rays with a hit; occluded: rays with a 1).  Atomic adds; they decide nothing.
 *
 * THE GRID.  dims = (nx, ny, nz) cells over the box, 1 <= each <= EONERF_RAYCAST_MAX_DIM, nx ny nz <= 2^27.  Cell units along axis c:
 *   g_c(p) = (p_c - lo_c) * (dims_c / (hi_c - lo_c)), one subtraction, one product by a quotient rounded once.  A live triangle is
 *   listed in every cell its bounding box overlaps: per axis floor(min g - PAD) .. floor(max g + PAD), clamped to [0, dims_c - 1],
 *   PAD = EONERF_RAYCAST_PAD = 2^-8.  A ray walks the cells from max(t_min, its entry into the box grown by PAD) to min(t_max, its
 *   exit) with an Amanatides-Woo stepper in fp64: the cell of the start point, clamped; per axis the parameter at which it crosses its
 *   cell's far boundary, (boundary - g_c(o)) / (d_c dims_c / (hi_c - lo_c)), formed anew from the boundary's integer after every step
 *   (nothing accumulates), +inf where d_c == 0; the smallest of the three is where the ray leaves the cell, and the axis it belongs to
 *   (ties: the smallest index; the other follows in the next round, at the same parameter) is stepped.  After the triangles of a cell
 *   the closest form stops iff its best t so far is <= the parameter at which the ray leaves that cell; the any-hit form stops at the
 *   first hit.  Both stop once that parameter is beyond the exit or the step leaves the grid.
 *   WHY THE PAD SUFFICES  A hit at t lies at o + t d inside the triangle's bounding box up to the rounding of the rule; the stepper
 *   places that point in a cell up to the rounding of g_c(o) + t d_c', a few 2^-53 of |g_c(o)| + |t d_c'| -- below 2^-30 of a cell for
 *   any origin within 2^20 cells of the box.  Where the two disagree about a boundary, or a hit sits on a lattice point or a cell face,
 *   the triangle is listed on both sides, 2^-8 of a cell being seven orders of magnitude more.  (The argument takes a hit point that lies
 *   inside its triangle's box: a ray coplanar with a triangle to within rounding, whose edge functions are noise of one sign, is outside it.)
 *   LOOP BOUNDS  at most nx + ny + nz + 3 cell steps per ray -- every step moves one axis one cell one way, and the loop counts them --
 *   and the stored length of a cell's list, limited to the entries the workspace holds.  No value of any input makes a kernel spin.
 *
 * LIMITS  n_vertices, n_triangles <= 2^31 - 1; list entries <= 2^31 - 1; strides in floats, 3 .. EONERF_RAYCAST_MAX_STRIDE.
 *
 * WORKSPACE (eonerf_raycast_workspace_bytes; tiles of EONERF_RAYCAST_TILE consecutive cells): per cell the start of its list inside
 *   its tile and the cursor that filled the list (uint32 each; after the build the cursor IS the list's length), the sums of the tiles,
 *   of EONERF_RAYCAST_TILE tiles and so on up to one (uint32 each), and the lists: one uint32 face index per entry.  8 bytes a cell and
 *   4 an entry.  It carries no copy of the triangles (no 48-byte record): a cast reads the three indices and the three vertices of a
 *   listed face from the caller's arrays.  eonerf_raycast_build fills it, the casts only read it, so one build feeds any number of
 *   casts.  It may arrive dirty.  The per-cell counts of eonerf_raycast_count live in a buffer of the caller's (uint32 per cell), since
 *   the workspace's size follows from their sum.
 *
 * Launches.  count: a memset of the cell counts and of counts_dev; a lane per triangle adds one to every cell of its padded box -- a
 *   box of more than EONERF_RAYCAST_LANE_CELLS cells is walked by the whole wave, 64 cells at a time.  build: a memset of the cursors;
 *   the plain blocked scan of eonerf_simplify.h over the counts; a lane per triangle (the wave for a large box) writes its index into
 *   each list through the atomic cursor -- the order inside a list depends on arrival and nothing depends on it.  casts: a memset of
 *   counts_dev and one launch, a lane per ray.  No kernel waits on another.
 */
#ifndef EONERF_RAYCAST_H
#define EONERF_RAYCAST_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_RAYCAST_VERSION 1
int eonerf_raycast_version(void);

/* Cells per axis at most; the pad of a triangle's box on every side, in cells (2^-8); cells one workgroup scans; the largest box one
 * lane walks alone. */
#define EONERF_RAYCAST_MAX_DIM 4096
#define EONERF_RAYCAST_PAD 0.00390625
#define EONERF_RAYCAST_TILE 1024
#define EONERF_RAYCAST_LANE_CELLS 64
/* Floats between two rays of a table at most. */
#define EONERF_RAYCAST_MAX_STRIDE 16777216

/* Bytes of workspace for a grid and its lists; 0 if a dims entry is outside 1 .. EONERF_RAYCAST_MAX_DIM, the cells exceed 2^27, or
 * n_triangles or entries is negative or above 2^31 - 1. */
size_t eonerf_raycast_workspace_bytes(const int dims[3], int64_t n_triangles, int64_t entries);

/* Counts, per cell, the live triangles whose padded box overlaps it; counts_dev[0] = their sum (the entries of the lists),
 * counts_dev[1] = the dropped triangles.  n_vertices == 0 and n_triangles == 0 are not refused (the pointers still may not be null).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / lo / hi / dims / cell_counts / counts_dev
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices or triangles
 *   EONERF_E_ARG          an entry of lo or hi that is not finite;  lo >= hi on an axis
 *   EONERF_E_ARG          a dims entry outside 1 .. EONERF_RAYCAST_MAX_DIM
 *   EONERF_E_UNSUPPORTED  more than 2^27 cells */
int eonerf_raycast_count(const void* vertices /* float[n_vertices][3] */, int64_t n_vertices, const void* triangles /* int32[n_triangles][3] */,
                         int64_t n_triangles, const double lo[3], const double hi[3], const int dims[3], void* cell_counts /* uint32[nx ny nz] */,
                         void* counts_dev /* int64[2] */, void* stream);

/* Scans the counts eonerf_raycast_count left for the same mesh, box and grid and fills the lists.  entries: counts_dev[0] of that call.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / lo / hi / dims / cell_counts / workspace
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices or triangles
 *   EONERF_E_ARG          an entry of lo or hi that is not finite;  lo >= hi on an axis
 *   EONERF_E_ARG          a dims entry outside 1 .. EONERF_RAYCAST_MAX_DIM
 *   EONERF_E_UNSUPPORTED  more than 2^27 cells
 *   EONERF_E_ARG          entries < 0
 *   EONERF_E_UNSUPPORTED  entries above 2^31 - 1
 *   EONERF_E_WORKSPACE    workspace_bytes below eonerf_raycast_workspace_bytes(dims, n_triangles, entries) */
int eonerf_raycast_build(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                         const int dims[3], const void* cell_counts /* uint32[nx ny nz] */, int64_t entries, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The closest hit of every ray, from what eonerf_raycast_build left in the workspace for the same mesh, box, grid and entries.
 * Ray r has its origin at origins[r * origin_stride + 0 .. 2] and its direction at dirs[r * dir_stride + 0 .. 2]: columns of a wider
 * table are read in place.  n_rays == 0 is not refused.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / lo / hi / dims / workspace / origins / dirs / t_out / face_out / bary_out /
 *                         counts_dev
 *   EONERF_E_ARG          n_vertices < 0, n_triangles < 0 or n_rays < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices, triangles or rays
 *   EONERF_E_ARG          an entry of lo or hi that is not finite;  lo >= hi on an axis
 *   EONERF_E_ARG          a dims entry outside 1 .. EONERF_RAYCAST_MAX_DIM
 *   EONERF_E_UNSUPPORTED  more than 2^27 cells
 *   EONERF_E_ARG          entries < 0
 *   EONERF_E_UNSUPPORTED  entries above 2^31 - 1
 *   EONERF_E_ARG          a stride below 3 or above EONERF_RAYCAST_MAX_STRIDE
 *   EONERF_E_ARG          t_min or t_max a NaN, t_min < 0, t_min > t_max or t_min infinite
 *   EONERF_E_WORKSPACE    workspace_bytes below eonerf_raycast_workspace_bytes(dims, n_triangles, entries) */
int eonerf_raycast_closest(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                           const int dims[3], int64_t entries, const void* workspace, size_t workspace_bytes, const float* origins,
                           int64_t origin_stride, const float* dirs, int64_t dir_stride, int64_t n_rays, double t_min, double t_max,
                           void* t_out /* double[n_rays] */, void* face_out /* int32[n_rays] */, void* bary_out /* float[n_rays][3] */,
                           void* counts_dev /* int64[3] */, void* stream);

/* Whether anything blocks each ray.  skip (int32[n_rays], or NULL): the face ray r does not see.  Refusals as eonerf_raycast_closest,
 * with occluded_out in the place of the three outputs. */
int eonerf_raycast_occluded(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_triangles, const double lo[3], const double hi[3],
                            const int dims[3], int64_t entries, const void* workspace, size_t workspace_bytes, const float* origins,
                            int64_t origin_stride, const float* dirs, int64_t dir_stride, int64_t n_rays, double t_min, double t_max,
                            const void* skip /* int32[n_rays] or NULL */, void* occluded_out /* uint8[n_rays] */, void* counts_dev /* int64[3] */,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
