/* eonerf_mesh.h -- a triangle mesh of a level set of a sampled density volume: marching tetrahedra on the device, entry points of
 * libeonerf_hip.so.
 *
 * Conventions are those of eonerf_ortho.h: plain C, raw DEVICE pointers, HOST float[3] for origin and spacing, a hipStream_t passed as
 * void*, the caller owns every buffer (the workspace included), every call is asynchronous on `stream`, nothing is allocated and
 * nothing synchronises.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.
 * The group is stateless: it takes no context.  The output is a pure function of (f, level, origin, spacing): two calls give the same
 * bits, and so does a restatement of the rule below on the host.
 *
 * THE RULE.
 *   INPUT  a volume f[nz][ny][nx] of fp32 values, x fastest, and a level.  Lattice point (i, j, k) has the linear index
 *     p = (k * ny + j) * nx + i.  Cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, has the linear index of its lowest corner.
 *   INSIDE  a point is inside iff `f >= level` is true: a NaN is outside.
 *   TETRAHEDRA  a cell is split into six tetrahedra (the Kuhn / Freudenthal split), one per permutation of the axes, in lexicographic
 *     order of the permutation with x = 0, y = 1, z = 2: xyz, xzy, yxz, yzx, zxy, zyx.  The corners c0 .. c3 of a tetrahedron are the path
 *     from the cell's lowest corner to its highest that adds one to one axis at a time, in the permutation's order.  All six share the
 *     body diagonal.  The split is the same in every cell, so neighbouring cells agree on the diagonal of every shared face.
 *   EDGES AND VERTICES  every lattice point OWNS the seven edges that leave it in these directions (x y z):
 *         slot       0    1    2    3    4    5    6
 *         direction  100  010  001  110  101  011  111
 *     An edge exists only where its far end is inside the lattice.  An edge whose ends differ in "inside" carries exactly one vertex.
 *     Vertices are numbered by increasing KEY p * 8 + slot.
 *     With a the owning end and b the far end:  t = (level - f_a) / (f_b - f_a), one fp32 subtraction each and one correctly rounded
 *     fp32 division; then t = 0 unless t >= 0 (a NaN quotient, which needs both differences to overflow, gives 0), then t = 1 if t > 1.
 *     If f_a or f_b is not finite, t = 0.5 and the edge is counted (counts[2] below).
 *     Per axis c:  idx_c = float(index of a on c) + (the direction steps on c ? t : 0),  pos_c = origin_c + spacing_c * idx_c: one fp32
 *     multiply and one fp32 add, not contracted.  A lattice point's own position is the same formula with t = 0
 *     (eonerf_mesh_lattice_points), so vertices and lattice points share one coordinate rule.
 *   TRIANGLES  with I the inside and O the outside corners of a tetrahedron, each in path order, and (u, v) the vertex on the edge
 *     between corners u and v:
 *         |I| = 1                     one triangle   (I0,O0) (I0,O1) (I0,O2)
 *         |I| = 3                     one triangle   (O0,I0) (O0,I1) (O0,I2)
 *         |I| = 2, I = {p,q}, O = {r,s}   two triangles  (p,r) (p,s) (q,s)  and  (p,r) (q,s) (q,r)
 *     A triangle's last two vertices are swapped where its normal would otherwise point from the outside corners towards the inside
 *     ones; the normal is taken on the midpoints of its three edges in the unit cell, so the swap is a property of the (tetrahedron,
 *     case) pair, not of the values.  Normals therefore point against increasing density: the convention of eonerf_normals.h.
 *     Triangles are ordered by cell index, then tetrahedron, then the order above.
 *   Degenerate triangles (from values exactly equal to the level) are kept and nothing is welded.  Wherever the surface does not touch
 *   the boundary of the volume the mesh is a closed, consistently oriented 2-manifold.
 *
 * WORKSPACE, left by eonerf_mesh_count for eonerf_mesh_emit (n = nx * ny * nz points, tiles of EONERF_MESH_TILE = 1024 consecutive
 *   points, every part 256-byte aligned): per point the exclusive scan of the vertex counts inside its tile (uint16) and of the
 *   triangle counts inside its tile (uint16) and the 7-bit mask of its owned crossing edges (uint8); per tile, per 1024 tiles and once
 *   more the exclusive scans of the tile totals (two uint32 each).  The id of the vertex on the edge at point p, slot e is
 *   scan[p] + popcount(mask[p] & ((1 << e) - 1)) with scan[p] = (offset of p's tile) + (scan inside the tile): no vertex index table
 *   is stored.  Every byte emit reads is written by count: the workspace's earlier contents never matter.
 *
 * Launches.  count: a memset of counts_dev; one classify launch (mask, triangle count and the scan inside each tile from one read of
 *   the volume); three launches of a plain blocked scan over the tile totals (scan, scan, add; the last also writes the counts).  emit: a
 *   memset of the status word and one launch.  No kernel waits on another workgroup.  The only atomics are on the status word and on the
 *   non-finite counter; they never decide an id or an order.
 */
#ifndef EONERF_MESH_H
#define EONERF_MESH_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_MESH_VERSION 1
int eonerf_mesh_version(void);

/* Lattice points one call takes: seven vertices per point must stay an int32 triangle index. */
#define EONERF_MESH_MAX_POINTS (1 << 28)
/* Points per scan tile (one workgroup of the classify launch). */
#define EONERF_MESH_TILE 1024
/* Bit 0 of *status_dev: a vertex or a triangle did not fit its capacity. */
#define EONERF_MESH_STATUS_CAPACITY 1

/* Positions of the lattice points of the slab z0 .. z0 + nz - 1 by the coordinate rule above, point (i, j, z0 + k) at
 * xyz_out[(k * ny + j) * nx + i]: ready for eonerf_query_density.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null origin / spacing / xyz_out;  nx < 1, ny < 1, nz < 1 or z0 < 0
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points in the slab, or z0 + nz beyond EONERF_MESH_MAX_POINTS
 *   EONERF_E_ARG          an origin or spacing entry that is not finite;  a zero spacing */
int eonerf_mesh_lattice_points(const float origin[3], const float spacing[3], int nx, int ny, int z0, int nz,
                               float* xyz_out /* [nz * ny * nx][3] */, void* stream);

/* Bytes of the workspace of eonerf_mesh_count / eonerf_mesh_emit, computed in 64 bits.  0 for a refused shape: a dimension below 2 or
 * more than EONERF_MESH_MAX_POINTS points. */
size_t eonerf_mesh_workspace_bytes(int nx, int ny, int nz);

/* Classifies the volume and scans the counts.  counts_dev[0] = number of vertices, [1] = number of triangles, [2] = number of crossing
 * edges with an end that is not finite, [3] = 0.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / counts_dev / workspace
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a level that is not finite
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_mesh_workspace_bytes(nx, ny, nz) */
int eonerf_mesh_count(const float* f, int nx, int ny, int nz, float level, int64_t* counts_dev /* [4] */,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Writes the vertices and triangles of the mesh.  Reads what eonerf_mesh_count left in `workspace` for the same (f, shape, level).
 * vertex_key (may be NULL) receives each vertex' key p * 8 + slot.  *status_dev is set to 0 first; nothing is written at or beyond a
 * capacity: a vertex id >= cap_v or a triangle index >= cap_t sets EONERF_MESH_STATUS_CAPACITY in *status_dev, and everything that
 * fits is still written (the triangles that fit may then name vertices that did not).
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / origin / spacing / workspace / vertices / triangles / status_dev
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a level, origin or spacing entry that is not finite
 *   EONERF_E_ARG          a zero spacing
 *   EONERF_E_ARG          a negative capacity
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_mesh_workspace_bytes(nx, ny, nz) */
int eonerf_mesh_emit(const float* f, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3],
                     const void* workspace, size_t workspace_bytes, float* vertices /* [cap_v][3] */, int64_t cap_v,
                     int32_t* triangles /* [cap_t][3] */, int64_t cap_t, int64_t* vertex_key /* [cap_v] */, int32_t* status_dev,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
