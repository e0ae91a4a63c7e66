/* eonerf_mesh_dsm.h -- a triangle mesh seen straight from above: for every cell of a georeferenced grid the altitude of the highest
 * surface under the cell's centre (a DSM of the mesh), the triangle that gave it, and per-vertex attributes interpolated there.  Entry
 * points of libeonerf_hip.so.  The raster goes into eonerf_dsm_mask_water -> eonerf_dsm_register -> eonerf_dsm_mae unchanged, which
 * puts a mesh on the scale of the DSM MAE.
 *
 * Conventions are those of eonerf_mesh.h: plain C, raw DEVICE pointers, HOST double[3] for scale and offset, a hipStream_t passed as
 * void*, the caller owns every buffer, every call is asynchronous on `stream`, nothing is allocated and nothing synchronises.  Return
 * value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.  The group is stateless: it takes no context.
 * The grid is the quintuple of eonerf_dsm_rasterize: (xoff, yoff) = the raster's upper-left corner, xsize, ysize, res.  Rasters are
 * row-major [ysize][xsize]; cell (j, i) -- row j, column i -- is sampled at its centre.
 * The output is a pure function of (vertices, triangles, scale, offset, grid): it does not depend on the order in which triangles or
 * lanes arrive, two calls give the same bits, and so does a restatement of the rule below on the host.
 *
 * THE RULE.
 *   VERTEX  per axis c: pos_c = (double)v_c * scale_c + offset_c in fp64, one multiply and one add, not contracted; east = pos_0,
 *     north = pos_1, altitude = pos_2.  A negative northing gets + 10e6, as in eonerf_dsm_rasterize.
 *     u = (east - xoff) / res and v = (yoff - north) / res: one fp64 subtraction and one correctly rounded fp64 division each.
 *     The vertex snaps to fixed point with EONERF_MESH_DSM_SUBPIXEL_BITS = 12 sub-pixel bits: X = llrint(u * 4096), Y = llrint(v * 4096),
 *     ties to even (the product is exact).  The altitude stays fp64.
 *   DROPPED TRIANGLE  a triangle is dropped and counted, and never rasterised, if one of its indices is outside [0, n_vertices), or one
 *     of its vertices has a coordinate or an altitude that is not finite, |X| or |Y| above 2^29 (EONERF_MESH_DSM_MAX_COORD; decided on
 *     u * 4096 before the conversion, which is the same test), or |altitude| at or above 32768 m (EONERF_MESH_DSM_MAX_ALTITUDE).
 *     The bound keeps every coordinate difference below 2^30, so every edge function
 *         E_ab(P) = (Xb - Xa) * (Py - Ya) - (Yb - Ya) * (Px - Xa)
 *     is exact in int64 (below 2^61).  The index test matters because eonerf_mesh_emit documents that after a capacity overflow "the
 *     triangles that fit may then name vertices that did not".
 *   DEGENERATE TRIANGLE  A2 = E_01(vertex 2), twice the projected area.  A triangle with A2 = 0 (a vertical wall, a zero-size triangle)
 *     is skipped and counted; its neighbours cover its edges.
 *   COVERAGE  the sample point of cell (j, i) is P = (4096 i + 2048, 4096 j + 2048).  With s = sign(A2):
 *         w0 = s * E_12(P),  w1 = s * E_20(P),  w2 = s * E_01(P)        (w_k belongs to vertex k; w0 + w1 + w2 = |A2|)
 *     the cell is covered iff all three are >= 0.  Every edge is inclusive: two triangles that share an edge leave no crack, and a cell
 *     hit twice is harmless under a maximum.  Both orientations of a triangle give the same result.  The cells visited are those of the
 *     integer bounding box -- columns ceil((min X - 2048) / 4096) .. floor((max X - 2048) / 4096), rows likewise in Y, floor divisions in
 *     integers -- clamped to the grid.
 *   ALTITUDE AT THE SAMPLE  z = (((double)w0 * z0 + (double)w1 * z1) + (double)w2 * z2) / (double)|A2|: fp64, in this order, not
 *     contracted.  q = llrint(z * 65536), clamped to [-2^31, 2^31 - 1] (only a rounding at the very limit of the altitude range can
 *     reach the clamp).
 *   RESOLVE  one 64-bit unsigned atomic maximum per covered (cell, triangle) pair on
 *         key = ((uint64)(uint32)(q + 2^31) << 32) | (0xFFFFFFFF - face)
 *     The highest surface wins; at equal q the smallest face index wins.  0 is "empty": no real key is 0 (a face index is below 2^31).
 *   OUTPUTS  dsm = (double)q / 65536 rounded once to fp32, NaN where empty; face = the winning triangle's index, -1 where empty.
 *     counts[0] = triangles rasterised (neither dropped nor degenerate, whether or not they cover a cell), [1] = dropped,
 *     [2] = degenerate, [3] = covered cells.  The counters use atomics; they never decide a value.
 *
 * Launches.  rasterize: a memset of keys and of counts_dev; one launch over the triangles -- a wave takes 64 consecutive triangles, every
 *   lane sets one up and walks its own bounding box if that has at most EONERF_MESH_DSM_LANE_CELLS cells; larger triangles are walked by
 *   the whole wave, one after the other, 64 cells at a time -- and one element-wise launch that resolves keys into dsm and face.
 *   attributes: one element-wise launch.  No kernel waits on another workgroup.
 */
#ifndef EONERF_MESH_DSM_H
#define EONERF_MESH_DSM_H
#include <stddef.h>
#include <stdint.h>

#include "eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_MESH_DSM_VERSION 1
int eonerf_mesh_dsm_version(void);

/* Sub-pixel bits of the vertex snap. */
#define EONERF_MESH_DSM_SUBPIXEL_BITS 12
/* Largest |X|, |Y| of a vertex that is kept, in sub-pixels. */
#define EONERF_MESH_DSM_MAX_COORD (1 << 29)
/* |altitude| in metres at and above which a vertex drops its triangles. */
#define EONERF_MESH_DSM_MAX_ALTITUDE 32768
/* Largest xsize / ysize of a call. */
#define EONERF_MESH_DSM_MAX_SIZE 65536
/* Cells of a bounding box up to which one lane walks it alone. */
#define EONERF_MESH_DSM_LANE_CELLS 64
/* Largest `channels` of eonerf_mesh_dsm_attributes. */
#define EONERF_MESH_DSM_MAX_CHANNELS 8

/* Rasterises the mesh by the rule above.  keys is the call's scratch raster: cleared by the call, it may arrive dirty, and it holds
 * the winning keys afterwards.  face may be NULL.  n_triangles == 0 is not refused: it gives an all-NaN raster.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / scale / offset / keys / dsm / counts_dev
 *   EONERF_E_ARG          xsize < 1 or ysize < 1
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_UNSUPPORTED  xsize or ysize above EONERF_MESH_DSM_MAX_SIZE;  more than 2^31 - 1 vertices or triangles
 *   EONERF_E_ARG          res, xoff, yoff or an entry of scale or offset that is not finite;  res <= 0;  a zero scale */
int eonerf_mesh_dsm_rasterize(const float* vertices /* [n_vertices][3] */, int64_t n_vertices, const int32_t* triangles /* [n_triangles][3] */,
                              int64_t n_triangles, const double scale[3], const double offset[3], double xoff, double yoff, int xsize,
                              int ysize, double res, uint64_t* keys /* [ysize * xsize] */, float* dsm /* [ysize * xsize] */,
                              int32_t* face /* [ysize * xsize] */, int64_t* counts_dev /* [4] */, void* stream);

/* Per-vertex attributes at the cell centres.  For every cell with face >= 0 the three weights w0 .. w2 of that triangle are computed
 * again by the same integer rule and every channel is interpolated as the altitude is:
 *   out = (((double)w0 * a0 + (double)w1 * a1) + (double)w2 * a2) / (double)|A2|, rounded once to fp32.
 * A cell gets NaN in every channel if its face is negative (empty) or outside [0, n_triangles), if that triangle would be dropped or is
 * degenerate, or if it does not cover the cell's centre; nothing is dereferenced beyond the failing test.
 *
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / scale / offset / face / attr / out
 *   EONERF_E_ARG          xsize < 1 or ysize < 1
 *   EONERF_E_ARG          n_vertices < 0 or n_triangles < 0
 *   EONERF_E_ARG          channels outside 1 .. EONERF_MESH_DSM_MAX_CHANNELS
 *   EONERF_E_UNSUPPORTED  xsize or ysize above EONERF_MESH_DSM_MAX_SIZE;  more than 2^31 - 1 vertices or triangles
 *   EONERF_E_ARG          res, xoff, yoff or an entry of scale or offset that is not finite;  res <= 0;  a zero scale */
int eonerf_mesh_dsm_attributes(const float* vertices /* [n_vertices][3] */, int64_t n_vertices, const int32_t* triangles /* [n_triangles][3] */,
                               int64_t n_triangles, const double scale[3], const double offset[3], double xoff, double yoff, int xsize,
                               int ysize, double res, const int32_t* face /* [ysize * xsize] */, const float* attr /* [n_vertices][channels] */,
                               int channels, float* out /* [ysize * xsize][channels] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
