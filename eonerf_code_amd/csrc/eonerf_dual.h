/* eonerf_dual.h -- STAGED public header (it moves to include/ and its bindings into _lib.API in the follow-up that counts it among
 * the public headers; until then the bindings are _lib.API_STAGED_DUAL and tests/test_dual_abi_cpu.py holds them to this file).
 *
 * Dual contouring of a level set of a sampled density volume from Hermite data: one vertex per surface cell, placed by minimising a
 * quadric built from the crossing points of the cell's edges and the field's gradient there, and one quad per sign-changing axis
 * edge.  The second mesher beside marching tetrahedra (include/eonerf_mesh.h): vertices can sit on ridges and corners inside a cell.
 * Entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_mesh.h: plain C, raw DEVICE pointers, HOST float[3] for origin and spacing, a hipStream_t passed as
 * void*, the caller owns every buffer (the workspace included), every call is asynchronous on `stream`, nothing is allocated and
 * nothing synchronises.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 * The group is stateless: it takes no context.  The output is a pure function of (f, level, origin, spacing, gradient,
 * regularisation): two calls give the same bits, and so does a restatement of the rule below on the host.
 *
 * THE RULE.
 *   INPUT  a volume f[nz][ny][nx] of fp32 values, x fastest, and a level.  Lattice point (i, j, k) has the linear index
 *     p = (k * ny + j) * nx + i.  Cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, has the linear index of its lowest corner.
 *   INSIDE  a point is inside iff `f >= level` is true: a NaN is outside.
 *   HERMITE POINTS  every lattice point OWNS the three axis edges that leave it: slot 0 = +x, 1 = +y, 2 = +z.  An edge exists only
 *     where its far end is inside the lattice.  An edge whose ends differ in "inside" carries exactly one Hermite point.  Hermite
 *     points are numbered by increasing KEY p * 8 + slot.
 *     With a the owning end and b the far end:  t = (level - f_a) / (f_b - f_a), one fp32 subtraction each and one correctly rounded
 *     fp32 division; then t = 0 unless t >= 0 (a NaN quotient, which needs both differences to overflow, gives 0), then t = 1 if t > 1.
 *     If f_a or f_b is not finite, t = 0.5 and the edge is counted (counts[3] below).
 *     Per axis c:  idx_c = float(index of a on c) + (the edge runs along c ? t : 0),  pos_c = origin_c + spacing_c * idx_c: one fp32
 *     multiply and one fp32 add, not contracted.  The Hermite points are therefore, bit for bit, the vertices eonerf_mesh_emit gives
 *     in slots 0 .. 2, under the same keys.
 *   ACTIVE CELLS  a cell is active iff its eight corners are not all on one side.  Each active cell carries one vertex; vertices are
 *     numbered by increasing cell index.
 *   NORMALS  the caller hands in g, fp32 [H][3]: the field's gradient at the Hermite points, in the volume's coordinates, row h for
 *     Hermite point h.  Its sign and its length do not matter.  In fp64:  G_c = g_c * spacing_c (the plane in lattice units) and
 *     s = (G_0 G_0 + G_1 G_1) + G_2 G_2.  A sample contributes a plane iff all three g_c are finite and s > 0; a sample that fails
 *     this is dropped and counted (report[2]).
 *   A CELL'S VERTEX, in fp64, in cell-local coordinates in [0, 1]^3.  Only +, -, *, / are used, each rounded once, nothing contracted.
 *     The cell's twelve edges are numbered e = 4a + 2v + u: a is the edge's axis, u and v its offsets (0 or 1) on the two other axes,
 *     u on the lower of the two.  The edge's owner is the cell's lowest corner plus those offsets, its slot is a.
 *     For every crossing edge, q_e has u and v on the two other axes and double(t) on a, t as above, computed again from f.
 *     m = (sum of the q_e in increasing e, from 0) / (their number): one division per coordinate.
 *     A = lambda^2 I + sum G G^T / s  and  b = sum G (G . (q_e - m)) / s  over the planes in increasing e, where lambda^2 =
 *     double(regularisation) * double(regularisation), every entry of A is  A_cd = A_cd + (G_c * G_d) / s  in the order 00 01 02 11 12 22,
 *     d = q_e - m per coordinate,  dot = (G_0 d_0 + G_1 d_1) + G_2 d_2  and  b_c = b_c + (G_c * dot) / s.
 *     x = m + A^-1 b through the LDL^T factorisation, with no square root and no pivoting (A - lambda^2 I is positive semi-definite):
 *         d0 = A00;  l10 = A01 / d0;  l20 = A02 / d0;  d1 = A11 - l10 * A01;  t21 = A12 - l20 * A01;  l21 = t21 / d1;
 *         d2 = (A22 - l20 * A02) - l21 * t21;
 *         y0 = b0;  y1 = b1 - l10 * y0;  y2 = (b2 - l20 * y0) - l21 * y1;   z_c = y_c / d_c;
 *         x2 = z2;  x1 = z1 - l21 * x2;  x0 = (z0 - l10 * x1) - l20 * x2;   x_c = m_c + x_c.
 *     If a coordinate of x is not finite, x = m and the vertex is counted (report[1]).  Otherwise every coordinate is clamped into
 *     [0, 1] (x_c < 0 gives 0, x_c > 1 gives 1), and a vertex with a clamped coordinate is counted once (report[0]).  A cell without a
 *     usable plane gives m exactly.
 *     Output:  idx_c = float(cell index on c) + float(x_c) in fp32, then pos_c = origin_c + spacing_c * idx_c as above.
 *   FACES  every Hermite point whose edge has four existing cells around it gives one quad, in key order: with the edge along axis a
 *     at owner P, and (o1, o2) the two axes that follow a cyclically (x -> y z, y -> z x, z -> x y), that is iff
 *     1 <= P_o1 <= n_o1 - 2 and 1 <= P_o2 <= n_o2 - 2.  Edges on the volume's boundary give none: the surface is open there, as
 *     marching tetrahedra's is.  The ring of cells is  P - e_o1 - e_o2,  P - e_o2,  P,  P - e_o1  (counter-clockwise seen from +a); if
 *     the owning end P is outside, the ring is read backwards (r3 r2 r1 r0).  The quad gives the triangles (r0, r1, r2) and
 *     (r0, r2, r3): a fixed diagonal.  Normals therefore point against increasing density, the convention of eonerf_normals.h and
 *     eonerf_mesh.h; a solid's signed volume is positive.
 *   Nothing is welded and degenerate triangles are kept.  Every undirected edge of the soup is shared by an even number of
 *   triangles, and wherever the surface does not touch the boundary of the volume every directed edge has as many opposite twins as
 *   copies (the mesh is edge-balanced).  Dual contouring does NOT promise a 2-manifold: a cell that two sheets of the surface cross
 *   still carries one vertex, and its triangles may intersect their neighbours.
 *
 * WORKSPACE, left by eonerf_dual_count for eonerf_dual_hermite and eonerf_dual_emit (n = nx * ny * nz points, tiles of
 *   EONERF_MESH_TILE = 1024 consecutive points, every part 256-byte aligned): per point the exclusive scans inside its tile of the
 *   Hermite points, of the active cells and of the quads (uint16 each) and one byte: bits 0 .. 2 the mask of its owned crossing axis
 *   edges, bit 3 whether its cell is active, bits 4 .. 5 the number of quads its edges give; per tile, per 1024 tiles and once more the
 *   exclusive scans of the tile totals (four uint32 each: Hermite points, cells, quads, edges with an end that is not finite).
 *   The id of the Hermite point at point p, slot a is scan[p] + popcount(mask[p] & ((1 << a) - 1)) with scan[p] = (offset of p's
 *   tile) + (scan inside the tile); a cell's vertex id and a quad's index follow likewise.  No id table is stored.  Every byte the later
 *   calls read is written by count: the workspace's earlier contents never matter.
 *
 * Launches.  count: one classify launch (everything above from one read of the volume) and three launches of a plain blocked scan
 *   over the tile totals (scan, scan, add; the last also writes the counts).  hermite: a memset of the status word and one launch, a
 *   thread per point.  emit: a memset of the report and one of the status word, and one launch, a workgroup per tile: its threads first
 *   write the quads of their points and gather the tile's active cells into a dense list (the scan inside the tile is each cell's
 *   place in it), then solve the listed cells side by side.  No kernel waits on another workgroup.  The only atomics are on the status
 *   word and on the report counters; they never decide an id or an order.
 */
#ifndef EONERF_DUAL_H
#define EONERF_DUAL_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"
#include "../../include/eonerf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_DUAL_VERSION 1
/* Bit 0 of *status_dev: a Hermite point, a vertex, a triangle or a gradient row did not fit its capacity. */
#define EONERF_DUAL_STATUS_CAPACITY 1
/* The range of `regularisation` (lambda) as powers of two: 2^-10 .. 2^4. */
#define EONERF_DUAL_MIN_REG_LOG2 -10
#define EONERF_DUAL_MAX_REG_LOG2 4
int eonerf_dual_version(void);

/* Bytes of the workspace of eonerf_dual_count / _hermite / _emit, computed in 64 bits.  0 for a refused shape: a dimension below 2 or
 * more than EONERF_MESH_MAX_POINTS points. */
size_t eonerf_dual_workspace_bytes(int nx, int ny, int nz);

/* Classifies the volume and scans the counts.  counts_dev[0] = number of Hermite points, [1] = number of vertices (active cells),
 * [2] = number of triangles (two per quad), [3] = number of crossing axis edges with an end that is not finite.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / counts_dev / workspace
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a level that is not finite
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_dual_workspace_bytes(nx, ny, nz) */
int eonerf_dual_count(const float* f, int nx, int ny, int nz, float level, int64_t* counts_dev /* [4] */, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Writes the positions of the Hermite points: where the caller evaluates the gradient.  Reads what eonerf_dual_count left in
 * `workspace` for the same (f, shape, level).  point_key (may be NULL) receives each point's key p * 8 + slot.  *status_dev is set to
 * 0 first; nothing is written at or beyond the capacity: a point id >= cap_h sets EONERF_DUAL_STATUS_CAPACITY in *status_dev, and
 * everything that fits is still written.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / origin / spacing / workspace / points / status_dev
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a level, origin or spacing entry that is not finite
 *   EONERF_E_ARG          a zero spacing
 *   EONERF_E_ARG          a negative capacity
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_dual_workspace_bytes(nx, ny, nz) */
int eonerf_dual_hermite(const float* f, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3],
                        const void* workspace, size_t workspace_bytes, float* points /* [cap_h][3] */, int64_t cap_h,
                        int64_t* point_key /* [cap_h] */, int32_t* status_dev, void* stream);

/* Writes the vertices and triangles of the mesh.  Reads what eonerf_dual_count left in `workspace` for the same (f, shape, level).
 * gradient: fp32 [n_gradient][3], row h for Hermite point h.  regularisation: lambda of the rule.  cell_key (may be NULL) receives each
 * vertex' cell index.  report_dev[0] = vertices with a clamped coordinate, [1] = vertices that fell back to m, [2] = dropped planes,
 * [3] = 0.  *status_dev and report_dev are set to 0 first; nothing is written at or beyond a capacity: a vertex id >= cap_v, a
 * triangle index >= cap_t or a Hermite id >= n_gradient sets EONERF_DUAL_STATUS_CAPACITY in *status_dev (such a plane is left out, not
 * counted), and everything that fits is still written (the triangles that fit may then name vertices that did not).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / origin / spacing / gradient / workspace / vertices / triangles / report_dev / status_dev
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a level, origin or spacing entry that is not finite
 *   EONERF_E_ARG          a zero spacing
 *   EONERF_E_ARG          a regularisation that is not finite or outside [2^-10, 16]
 *   EONERF_E_ARG          a negative capacity or n_gradient
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_dual_workspace_bytes(nx, ny, nz) */
int eonerf_dual_emit(const float* f, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3],
                     const float* gradient /* [n_gradient][3] */, int64_t n_gradient, float regularisation, const void* workspace,
                     size_t workspace_bytes, float* vertices /* [cap_v][3] */, int64_t cap_v, int64_t* cell_key /* [cap_v] */,
                     int32_t* triangles /* [cap_t][3] */, int64_t cap_t, int64_t* report_dev /* [4] */, int32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
