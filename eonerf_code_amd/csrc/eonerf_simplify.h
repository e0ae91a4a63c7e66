/* eonerf_simplify.h -- STAGED public header (it moves to include/ and its bindings into _lib.API in the follow-up that counts it among
 * the public headers; until then the bindings are _lib.API_STAGED and tests/test_simplify_abi_cpu.py holds them to this file).
 *
 * Mesh simplification by vertex clustering (Rossignac-Borrel): every vertex falls into a cell of a coarse grid, all vertices of a cell
 * become one vertex, triangles that lose a corner to a merge disappear.  Entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_mesh.h: plain C, raw DEVICE pointers, HOST float[3] / int[3] for the grid, a hipStream_t passed as
 * void*, the caller owns every buffer, every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.  Return
 * value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.  The group is stateless: it takes no context.
 * The output is a pure function of (vertices, triangles, origin, cell, dims, representative): every decision is taken in integers, the
 * only atomics are an integer sum and a 64-bit minimum, so it does not depend on the order in which lanes arrive, two calls give the
 * same bits, and so does a restatement of the rule below on the host (tests/simplify_restated.py).
 *
 * THE RULE.  Grid: cell (qx, qy, qz), 0 <= q_c < dims[c], covers origin_c + q_c * cell_c .. origin_c + (q_c + 1) * cell_c; its id is
 * (qz * gy + qy) * gx + qx with (gx, gy, gz) = dims.  Each of gx, gy, gz is in 1 .. EONERF_SIMPLIFY_MAX_DIM, their product is at most
 * EONERF_SIMPLIFY_MAX_CELLS.
 *   VERTEX  a vertex with a coordinate that is not finite is DROPPED: it belongs to no cell.  Otherwise, per axis c, in fp64 and not
 *     contracted: u = ((double)v_c - (double)origin_c) / (double)cell_c, one subtraction and one correctly rounded division;
 *     s = u * 16384 (exact; EONERF_SIMPLIFY_SUBCELL_BITS = 14), clamped in fp64 to [0, g_c * 16384 - 1]; F_c = llrint(s), ties to even.
 *     Cell coordinate q_c = F_c >> 14, local coordinate L_c = F_c & 16383.  Vertices outside the grid land in its border cells.
 *   CELL SUMS  per cell n = its vertices and S_c = the sum of their L_c: integer atomic adds, S_c < 2^45, exact whatever the order.
 *   OUTPUT VERTICES  the occupied cells (n > 0) in ascending cell id are numbered 0 .. V' - 1: an exclusive scan of the occupancy flags
 *     over the dense cell table.
 *   SOURCE  per occupied cell the rounded mean M_c = (2 S_c + n) / (2 n), an integer division, in [0, 16383].  Every vertex of the cell
 *     offers key = ((uint64)d2 << 32) | vertex id with d2 = sum over c of (L_c - M_c)^2 (< 2^30); one 64-bit unsigned atomic minimum
 *     per vertex.  source[new id] = the low word of the cell's smallest key: the input vertex nearest to the cell's mean, at equal
 *     distance the one with the smallest id.
 *   POSITION  EONERF_SIMPLIFY_NEAREST: the three fp32 words of vertices[source], copied.  EONERF_SIMPLIFY_MEAN: per axis, in fp64 and
 *     not contracted, (double)origin_c + ((double)q_c + ((double)S_c / (double)n) / 16384.0) * (double)cell_c, rounded once to fp32.
 *   MAP  vertex_map[v] = the new id of input vertex v, -1 for a dropped one.
 *   TRIANGLES  a triangle is DROPPED and counted if one of its indices is outside [0, n_vertices) or names a dropped vertex
 *     (eonerf_mesh_emit documents that after a capacity overflow triangles may name vertices that did not fit).  It is COLLAPSED and
 *     counted if two of its three new ids are equal.  Every other triangle is KEPT: its three ids are mapped in place, so orientation
 *     and rotation are preserved, and kept triangles stay in input order (an exclusive scan of the keep flags).  Duplicates are kept.
 *   COUNTS  counts_dev[4] = V', kept, dropped, collapsed.  The scans write V' and kept; dropped is a sum of its own and collapsed what
 *     is left of n_triangles; neither decides a value.
 *   CAPACITIES  nothing is written at or beyond out_vertices[cap_vertices], source[cap_vertices] or out_triangles[cap_triangles];
 *     an output that did not fit sets EONERF_SIMPLIFY_STATUS_CAPACITY in *status_dev.  The counts are always the true ones.
 *
 * WORKSPACE (n = gx * gy * gz cells; tiles of EONERF_SIMPLIFY_TILE consecutive cells / triangles): per cell n (uint32), S (3 uint64),
 *   the key (uint64) and the occupancy scan inside its tile (uint16) -- 38 bytes a cell, dense: 80 MB for the expected 128^3 cells and
 *   about 5 GiB at the refused limit of 2^27 -- per vertex its cell id (int32), per triangle its class and the keep scan inside its
 *   tile (uint16), and the sums of the tiles, of EONERF_SIMPLIFY_TILE tiles and so on up to one (uint32 each).  eonerf_simplify_count
 *   fills it, eonerf_simplify_emit reads it and uses the keys; it may arrive dirty.
 *
 * Launches.  count: a memset of the cell sums and of counts_dev; one launch over the vertices (quantise, the atomics on n and S, runs
 *   of equal cell ids inside a wave combined first by a segmented shuffle reduction -- integers, so no bit changes); the blocked scan
 *   over the cells; one launch over the triangles (classify, scan inside the tile); the blocked scan over the triangle tiles.
 *   emit: a memset of the keys and of status_dev; one launch over the vertices (key minimum, combined likewise; vertex_map), one over the cells (positions
 *   and source of the occupied ones), one over the triangles (kept ones at their scanned offsets).  No kernel waits on another.
 */
#ifndef EONERF_SIMPLIFY_H
#define EONERF_SIMPLIFY_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_SIMPLIFY_VERSION 1
int eonerf_simplify_version(void);

/* Sub-cell bits of the vertex quantisation. */
#define EONERF_SIMPLIFY_SUBCELL_BITS 14
/* Largest gx, gy, gz and largest gx * gy * gz of a call. */
#define EONERF_SIMPLIFY_MAX_DIM 4096
#define EONERF_SIMPLIFY_MAX_CELLS (1 << 27)
/* Cells / triangles one workgroup scans. */
#define EONERF_SIMPLIFY_TILE 1024
/* `representative`. */
#define EONERF_SIMPLIFY_MEAN 0
#define EONERF_SIMPLIFY_NEAREST 1
/* *status_dev bit: an output vertex or triangle did not fit its capacity. */
#define EONERF_SIMPLIFY_STATUS_CAPACITY 1

/* Bytes of workspace for a grid and a mesh; 0 if dims is null or outside the limits, or a count is negative or above 2^31 - 1. */
size_t eonerf_simplify_workspace_bytes(const int dims[3], int64_t n_vertices, int64_t n_triangles);

/* Quantises and accumulates, scans the cells, classifies the triangles and scans them; writes counts_dev.  It clears what it uses of
 * the workspace.  n_vertices == 0 and n_triangles == 0 are not refused (the pointers still may not be null).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / origin / cell / dims / workspace / counts_dev
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices or triangles
 *   EONERF_E_UNSUPPORTED  an entry of dims outside 1 .. EONERF_SIMPLIFY_MAX_DIM, or more than EONERF_SIMPLIFY_MAX_CELLS cells
 *   EONERF_E_ARG          an entry of origin or cell that is not finite;  a cell <= 0
 *   EONERF_E_WORKSPACE    workspace_bytes below eonerf_simplify_workspace_bytes(dims, n_vertices, n_triangles) */
int eonerf_simplify_count(const float* vertices /* [n_vertices][3] */, int64_t n_vertices, const int32_t* triangles /* [n_triangles][3] */,
                          int64_t n_triangles, const float origin[3], const float cell[3], const int dims[3], void* workspace,
                          size_t workspace_bytes, int64_t* counts_dev /* [4] */, void* stream);

/* Writes the simplified mesh from the workspace eonerf_simplify_count left for the same inputs.  source and vertex_map may be NULL.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / origin / cell / dims / workspace / out_vertices / out_triangles / status_dev
 *   EONERF_E_ARG          n_vertices < 0, n_triangles < 0, cap_vertices < 0 or cap_triangles < 0
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices or triangles
 *   EONERF_E_UNSUPPORTED  an entry of dims outside 1 .. EONERF_SIMPLIFY_MAX_DIM, or more than EONERF_SIMPLIFY_MAX_CELLS cells
 *   EONERF_E_ARG          an entry of origin or cell that is not finite;  a cell <= 0
 *   EONERF_E_WORKSPACE    workspace_bytes below eonerf_simplify_workspace_bytes(dims, n_vertices, n_triangles)
 *   EONERF_E_ARG          a representative that is neither EONERF_SIMPLIFY_MEAN nor EONERF_SIMPLIFY_NEAREST */
int eonerf_simplify_emit(const float* vertices /* [n_vertices][3] */, int64_t n_vertices, const int32_t* triangles /* [n_triangles][3] */,
                         int64_t n_triangles, const float origin[3], const float cell[3], const int dims[3], int representative,
                         void* workspace, size_t workspace_bytes, float* out_vertices /* [cap_vertices][3] */, int64_t cap_vertices,
                         int32_t* out_triangles /* [cap_triangles][3] */, int64_t cap_triangles, int32_t* source /* [cap_vertices] */,
                         int32_t* vertex_map /* [n_vertices] */, int32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
