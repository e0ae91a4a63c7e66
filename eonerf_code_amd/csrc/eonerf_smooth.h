/* eonerf_smooth.h -- STAGED public header (it moves to include/ and its bindings into _lib.API in the follow-up that counts it among
 * the public headers; until then the bindings are _lib.API_STAGED_SMOOTH and tests/test_smooth_abi_cpu.py holds them to this file).
 *
 * Mesh smoothing: Taubin's lambda|mu iteration of the face-weighted umbrella operator, on positions in fixed point.  It keeps every
 * vertex, every face and their order; only positions change.  Entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_simplify.h: plain C, raw DEVICE pointers, HOST float[3] for the grid and a HOST array for the step
 * factors, a hipStream_t passed as void*, the caller owns every buffer, every call is asynchronous on `stream`, nothing is allocated,
 * nothing synchronises and nothing is read back.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.  The group
 * is stateless: it takes no context.  The output is a pure function of (vertices, triangles, origin, unit, pinned, pin_open, the
 * factors): every sum is an integer sum, so it does not depend on the order in which lanes arrive or faces are listed, two calls give
 * the same bits, and so does a restatement of the rule below on the host (tests/smooth_restated.py).
 *
 * THE RULE.  Q below is a position in quanta of 2^-16 unit; LIM = (EONERF_SMOOTH_MAX_COORD << 16) - 1 = 2^29 - 1.
 *   rdiv(a, b), b > 0: floor division rounded half up -- q = floor(a / b), r = a - q b, the result q + (2 r >= b).
 *   QUANTISE  per axis c, in fp64 and not contracted: u = ((double)v_c - (double)origin_c) / (double)unit_c, one subtraction and one
 *     correctly rounded division.  A vertex is QUANTISABLE iff its three u are finite and |u| < EONERF_SMOOTH_MAX_COORD.  Then
 *     Q_c = llrint(u * 65536) (the product is exact), ties to even, limited to [-LIM, LIM] (which acts only on a u within 2^-17 of
 *     +-8192): |Q| < 2^29.
 *   FACES  a face is LIVE iff its three indices lie in [0, n_vertices) and its three vertices are quantisable; otherwise it is DEAD:
 *     counted, and it contributes nothing.  Nothing else is special: faces with repeated indices, duplicate faces and opposite twins
 *     are live like any other.
 *   CORNERS  a live face (a, b, c) gives vertex a the corner (next = b, prev = c), vertex b the corner (c, a), vertex c the corner
 *     (a, b).  Per vertex i: c_i = the number of its corners (at most 3 T), n_i = 2 c_i.
 *   OPEN  B1_i = the sum over the corners of (next - prev) in int64, B2_i = the sum of (next^2 - prev^2) mod 2^64.  Vertex i is OPEN iff
 *     B1_i != 0 or B2_i != 0.  A vertex all of whose edges are used as often in one direction as in the other is never open; one with
 *     at most two open fans always is (two power sums decide two unknowns).
 *   FREE  iff quantisable, c_i > 0, pinned == NULL or pinned[i] == 0, and not (open and pin_open != 0).  Every vertex that is not free
 *     returns its INPUT BITS.
 *   STEP  with factor lam_q (int32, |lam_q| <= 65536; lambda = lam_q / 65536).  Jacobi: every vertex reads the positions of the step
 *     before.  Per free vertex and axis: S = the sum over the corners of (Q[next] + Q[prev]); D = S - n_i Q_i (|D| < 2^62);
 *     M = rdiv(D, n_i); delta = rdiv(lam_q * M, 65536); Q_i' = Q_i + delta limited to [-LIM, LIM]; where the limit acted,
 *     EONERF_SMOOTH_STATUS_CLAMPED is set in *status_dev.  Vertices that are not free keep Q_i.
 *     This is the face-weighted umbrella: on a closed manifold every neighbour appears twice in S and twice in n_i, so it is the
 *     uniform umbrella there and no edge has to be found twice.
 *   STEPS  lam_q_host[0 .. n_steps), 1 <= n_steps <= EONERF_SMOOTH_MAX_STEPS, applied in order.  Taubin with k iterations is
 *     (lambda_q, mu_q) k times with mu < -lambda < 0; a plain Laplacian lambda_q k times.
 *   DEQUANTISE  free vertices only, per axis in fp64 and not contracted: (double)origin_c + ((double)Q_c * 2^-16) * (double)unit_c,
 *     rounded once to fp32.  (Under lam_q = 0 a free vertex therefore moves by at most 2^-17 unit, and the fp32 rounding.)
 *   COUNTS  counts_dev[6] = free vertices; open vertices (whatever pin_open and the mask say); vertices the mask alone holds
 *     (quantisable, c_i > 0, pinned[i] != 0); quantisable vertices without a corner; vertices that are not quantisable; dead faces.
 *
 * LIMITS  n_vertices <= 2^31 - 1 and n_triangles <= 2^29, so that 3 T, every c_i and every n_i fit 32 bits and |D| < 2^62.
 *
 * WORKSPACE (tiles of EONERF_SMOOTH_TILE consecutive vertices): three tables of 16-byte records (Q_x, Q_y, Q_z, flags) per vertex --
 *   what eonerf_smooth_build quantised, and the two buffers the steps alternate between --, per vertex its corner count, the start of
 *   its corner list inside its tile and the cursor that filled the list (uint32 each), per corner (next, prev) as two uint32 -- 24
 *   bytes a triangle --, and the sums of the tiles, of EONERF_SMOOTH_TILE tiles and so on up to one (uint32 each).  60 bytes a vertex
 *   and 24 a triangle.  eonerf_smooth_build fills it; eonerf_smooth_run reads the first table, the counts, the starts and the corners
 *   and writes only the two step buffers, so one build feeds any number of runs.  It may arrive dirty.
 *
 * Launches.  build: a memset of the corner counts, of the cursors and of counts_dev; a lane per vertex quantises; a lane per face
 *   counts its three corners (a 32-bit atomic add each); the plain blocked scan of eonerf_simplify.h over the counts; a lane per face
 *   writes its three corners through the cursors (the order inside a list depends on arrival; every quantity taken from a list is an
 *   integer sum); a lane per vertex forms B1, B2 and the flags from its own list and counts.  run: a memset of status_dev; per step
 *   one launch, a lane per vertex gathering the records of its corners (no atomics); one launch that dequantises.  No kernel waits on
 *   another.
 */
#ifndef EONERF_SMOOTH_H
#define EONERF_SMOOTH_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_SMOOTH_VERSION 1
int eonerf_smooth_version(void);

/* Fraction bits of a position; the largest |coordinate| in units; the most steps of a call. */
#define EONERF_SMOOTH_FRAC_BITS 16
#define EONERF_SMOOTH_MAX_COORD 8192
#define EONERF_SMOOTH_MAX_STEPS 4096
/* Vertices one workgroup scans. */
#define EONERF_SMOOTH_TILE 1024
/* *status_dev bit: a step left [-LIM, LIM] and was limited to it. */
#define EONERF_SMOOTH_STATUS_CLAMPED 1

/* Bytes of workspace for a mesh; 0 if a count is negative, n_vertices above 2^31 - 1 or n_triangles above 2^29. */
size_t eonerf_smooth_workspace_bytes(int64_t n_vertices, int64_t n_triangles);

/* Quantises, lists the corners of every vertex, decides open and free, writes counts_dev.  pinned may be NULL.  n_vertices == 0 and
 * n_triangles == 0 are not refused (the pointers still may not be null).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / origin / unit / workspace / counts_dev
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices or more than 2^29 triangles
 *   EONERF_E_ARG          an entry of origin or unit that is not finite;  a unit <= 0
 *   EONERF_E_WORKSPACE    workspace_bytes below eonerf_smooth_workspace_bytes(n_vertices, n_triangles) */
int eonerf_smooth_build(const void* vertices /* float[n_vertices][3] */, int64_t n_vertices, const void* triangles /* int32[n_triangles][3] */,
                        int64_t n_triangles, const float origin[3], const float unit[3], const void* pinned /* uint8[n_vertices] or NULL */,
                        int pin_open, void* workspace, size_t workspace_bytes, void* counts_dev /* int64[6] */, void* stream);

/* Applies the steps to what eonerf_smooth_build left in the workspace for the same vertices and grid, writes out_vertices
 * (float[n_vertices][3]: free vertices dequantised, every other one the bits of `vertices`) and *status_dev (int32).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / origin / unit / lam_q_host / workspace / out_vertices / status_dev
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices or more than 2^29 triangles
 *   EONERF_E_ARG          an entry of origin or unit that is not finite;  a unit <= 0
 *   EONERF_E_ARG          n_steps outside 1 .. EONERF_SMOOTH_MAX_STEPS
 *   EONERF_E_ARG          a |lam_q_host[k]| above 65536
 *   EONERF_E_WORKSPACE    workspace_bytes below eonerf_smooth_workspace_bytes(n_vertices, n_triangles) */
int eonerf_smooth_run(const void* vertices /* float[n_vertices][3] */, int64_t n_vertices, int64_t n_triangles, const float origin[3],
                      const float unit[3], const int32_t* lam_q_host /* [n_steps] */, int n_steps, void* workspace, size_t workspace_bytes,
                      void* out_vertices, void* status_dev /* int32 */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
