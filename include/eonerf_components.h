/* eonerf_components.h -- the solids a marching-tetrahedra mesh encloses: connected components of a sampled density volume under the
 * connectivity of the mesher of eonerf_mesh.h, and an element-wise filter that drops small solids or fills cavities in front of
 * eonerf_mesh_count / eonerf_mesh_emit.  Entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_mesh.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer (the
 * workspace included), every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.  Return value: 0 = OK,
 * < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.  The group is stateless: it takes no context.
 *
 * THE RULE.
 *   INPUT  a volume f[nz][ny][nx] of fp32 values, x fastest, a level and a side.  Lattice point (i, j, k) has the linear index
 *     p = (k * ny + j) * nx + i, as in eonerf_mesh.h.
 *   SIDES  side 0 is the inside of eonerf_mesh.h: `f >= level` is true, so a NaN is outside.  side 1 is the complement.
 *   ADJACENCY  two points on the same side are adjacent iff they differ by one of the seven owned-edge directions of eonerf_mesh.h
 *     (x y z: 100 010 001 110 101 011 111) or by its negative: the 14 edges of the Kuhn split that meet in a lattice point.
 *     (1, -1, 0) is no edge.  Inside a tetrahedron the interpolant is linear, so the inside part of a tetrahedron is connected and holds
 *     its inside corners: the solids the mesh of eonerf_mesh.h encloses are exactly the components of side 0 under this adjacency, and
 *     the components of side 1 that do not reach the volume's boundary are its cavities.
 *   LABELS  labels[p] (int32) is the smallest linear index of p's component; -1 where p is not on `side`.
 *   INFO  info[r] (uint32) at a root r (labels[r] == r) holds the number of points of the component (at most 2^28) in bits 0 .. 30;
 *     bit 31 (EONERF_CC_BOUNDARY) is set iff the component holds a point of the volume's boundary, i.e. one with an index equal to 0 or
 *     to n - 1 on its axis.  info is 0 everywhere else.
 *   COUNTS  counts_dev[0] = number of components, [1] = number of points on `side`, [2] = size of the largest component,
 *     [3] = root of the largest component, the smallest root among ties (-1 where there is no component).
 *   FILTER  a component is dropped iff its count is below min_points and not (protect_boundary and bit 31 set).
 *     f_out[p] = f[p] but for the points of dropped components: -inf for side 0, +inf for side 1.  The mesh of f_out is the mesh of f
 *     without the dropped components' vertices and triangles: no crossing edge gains a non-finite end.
 *   PURITY  everything is a pure function of (f, level, side): two calls give the same bits, whatever the workspace held before, and
 *     so does a restatement of this rule on the host.
 *
 * Launches of eonerf_cc_label (256 threads each; no kernel waits on another workgroup: no spin, no flag, no look-back):
 *   a memset of counts_dev and of the workspace's one word;
 *   LOCAL    one workgroup per tile of EONERF_CC_TILE_X x _Y x _Z points (x longest: rows coalesce).  A union-find in LDS over the seven
 *            forward edges that stay inside the tile, flattened; labels[p] = global index of the tile-local root (the order (k, j, i) inside
 *            a tile is monotone in the global index, so the local minimum is the global one); the tile-local root's count and boundary
 *            flag go to info with plain stores (the tile owns those slots), 0 to the tile's other points.
 *   MERGE    one thread per point; for every forward edge that leaves the point's tile with both ends on `side`, a union on labels,
 *            which is the parent array: parent[x] <= x always.  Parents are read with relaxed agent-scope atomic loads only, and the
 *            union is right under stale reads: after old = atomicMin(&parent[hi], lo), if old != hi it goes on with the pair (old, lo);
 *            every iteration ends or moves to a strictly smaller index.  Edges that other edges imply are left out: a diagonal with a
 *            point on `side` between its ends, and a straight edge whose neighbour one step back along the tile face is the same edge
 *            between the same two tiles.  Walks halve their path: an entry is lowered (atomicMin) to its
 *            own grandparent, never to anything found through another entry's link.
 *   FLATTEN  a launch of its own, so all of MERGE is visible: labels[p] = find(p); each tile-local root that is not the global root
 *            adds its count (atomicAdd) and its flag (atomicOr) to info at the global root and clears its own: one pair of atomics per
 *            tile-local component, not per point.
 *   COUNTS   at most EONERF_CC_COUNT_BLOCKS workgroups stride over the points: per workgroup sums of the roots and the points, per wavefront a 64-bit
 *            atomicMax of (size << 32) | (0xFFFFFFFF - root) in the workspace;
 *   FINISH   one thread unpacks that word into counts_dev[2], [3].
 *   All atomics are on integers and none decides an id: minima, sums and maxima do not depend on the order.
 * eonerf_cc_filter: a memset of dropped_dev and one element-wise launch.
 */
#ifndef EONERF_COMPONENTS_H
#define EONERF_COMPONENTS_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"
#include "eonerf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_CC_VERSION 1
int eonerf_cc_version(void);

/* Points of one tile of the LOCAL launch (one workgroup of 256 threads, four points each). */
#define EONERF_CC_TILE_X 32
#define EONERF_CC_TILE_Y 8
#define EONERF_CC_TILE_Z 4
/* Workgroups (of 256 threads) of the COUNTS launch at most: beyond 256 times as many points each thread takes more than one. */
#define EONERF_CC_COUNT_BLOCKS 2048
/* Bit 31 of info at a root: the component touches the volume's boundary. */
#define EONERF_CC_BOUNDARY 0x80000000u

/* Bytes of the workspace of eonerf_cc_label.  0 for a refused shape: a dimension below 2 or more than EONERF_MESH_MAX_POINTS points. */
size_t eonerf_cc_workspace_bytes(int nx, int ny, int nz);

/* Labels the components of `side` (0 or 1) of the volume.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / labels / info / counts_dev / workspace
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a level that is not finite
 *   EONERF_E_ARG          a side that is neither 0 nor 1
 *   EONERF_E_WORKSPACE    workspace_bytes < eonerf_cc_workspace_bytes(nx, ny, nz) */
int eonerf_cc_label(const float* f, int nx, int ny, int nz, float level, int side, int32_t* labels /* [nz * ny * nx] */,
                    uint32_t* info /* [nz * ny * nx] */, int64_t* counts_dev /* [4] */, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Drops the components of `side` whose count is below min_points (see FILTER above) from the volume.  labels and info are what
 * eonerf_cc_label left for the same (f, shape, side).  f_out may be f itself.  dropped_dev[0] = components dropped, [1] = points dropped.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null f / labels / info / f_out / dropped_dev
 *   EONERF_E_ARG          a dimension below 2
 *   EONERF_E_UNSUPPORTED  more than EONERF_MESH_MAX_POINTS points
 *   EONERF_E_ARG          a side that is neither 0 nor 1;  protect_boundary neither 0 nor 1
 *   EONERF_E_ARG          a negative min_points
 *   EONERF_E_ARG          side 1 with protect_boundary 0: the outside world is not a cavity */
int eonerf_cc_filter(const float* f, const int32_t* labels, const uint32_t* info, int nx, int ny, int nz, int side, int64_t min_points,
                     int protect_boundary, float* f_out /* [nz * ny * nx] */, int64_t* dropped_dev /* [2] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
