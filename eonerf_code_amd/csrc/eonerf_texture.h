/* eonerf_texture.h -- STAGED public header (it moves to include/ and its bindings into _lib.API in the follow-up that counts it among
 * the public headers; until then the bindings are _lib.API_STAGED_TEXTURE and tests/test_texture_abi_cpu.py holds them to this file).
 *
 * Texture baking: a per-face atlas over a triangle mesh, the ground point of every texel, and the input images gathered through
 * their RPCs and fused per texel in ONE launch that loops over the K images in registers.  Entry points of libeonerf_hip.so.
 *
 * Conventions are those of eonerf_ortho.h: plain C, raw DEVICE pointers, a hipStream_t passed as void*, the caller owns every buffer,
 * every call is asynchronous on `stream`, nothing is allocated, nothing synchronises and nothing is read back.  The calls are
 * stateless.  Return value: 0 = OK, < 0 = EONERF_E_* of eonerf_hip.h, > 0 = hipError_t.  One thread per face, texel or sample; no
 * atomics, so every result is run-to-run bit-identical.  All arithmetic is fp64 and unfused, with one cast per fp32 output.
 *
 * THE ATLAS.  T = texels per leg, 1 <= T <= EONERF_TEXTURE_MAX_TEXELS.  Every pair of faces owns one square cell of side S = T + 5:
 *   cell j holds face 2j (its lower triangle) and face 2j + 1 (its upper triangle).
 *   cells = ceil(F / 2), cells_per_row = ceil(sqrt(cells)) in exact integer arithmetic,
 *   atlas_w = cells_per_row * S, atlas_h = ceil(cells / cells_per_row) * S  (all three 0 for F == 0);
 *   cell j sits at column j mod cells_per_row and row j div cells_per_row; texels are numbered row-major, t = y * atlas_w + x.
 *   Texel (x, y) of a cell has its centre at (x + 0.5, y + 0.5) and belongs to the lower face iff x + y <= S - 1, else to the upper.
 *   Lower-face corners A, B, C lie at (1.5, 1.5), (T + 1.5, 1.5), (1.5, T + 1.5) in cell coordinates, upper-face corners at
 *   (S - 1.5, S - 1.5), (S - 1.5 - T, S - 1.5), (S - 1.5, S - 1.5 - T).
 *   Barycentric weights of a texel, from its centre (u, v) in fp64: b1 = (u - u_A) / (u_B - u_A), b2 = (v - v_A) / (v_C - v_A),
 *   b0 = (1 - b1) - b2; then each b_i = max(b_i, 0) and b_i / ((b0 + b1) + b2).  Gutter texels are so clamped onto their own face: a
 *   gutter texel carries the colour of the nearest point of its face along the clamp, and no bilinear tap of non-zero weight inside a
 *   face's UV triangle lands on a texel of another face (tests/test_texture_restated_cpu.py), so no dilation pass is needed.
 *   Texels of an odd last face's missing partner and of unused cells in the last row have face -1 and NaN everywhere.
 *   A face with an index outside [0, n_vertices) or a non-finite vertex keeps its texels (face, bary) but gives NaN xyz, lonlatalt
 *   and normal.
 *
 * LIMITS  atlas_w, atlas_h <= EONERF_TEXTURE_MAX_SIDE and atlas_w * atlas_h <= 2^31 - 1 (formed in 64 bits); n_vertices <= 2^31 - 1.
 */
#ifndef EONERF_TEXTURE_H
#define EONERF_TEXTURE_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EONERF_TEXTURE_VERSION 1
#define EONERF_TEXTURE_MAX_TEXELS 64
#define EONERF_TEXTURE_GUTTER 5         /* S = T + EONERF_TEXTURE_GUTTER */
#define EONERF_TEXTURE_MAX_SIDE 32768
#define EONERF_TEXTURE_MAX_MEDIAN 64    /* images the median takes (one sample's values live in private memory), as EONERF_ORTHO_MAX_MEDIAN */
#define EONERF_TEXTURE_MEAN 0           /* eonerf_ortho_fuse's EONERF_ORTHO_MEAN */
#define EONERF_TEXTURE_MEDIAN 1         /* eonerf_ortho_fuse's EONERF_ORTHO_MEDIAN */
#define EONERF_TEXTURE_BEST 2           /* the value of the image with the largest weight, ties to the smaller k */
int eonerf_texture_version(void);

/* HOST only: out[3] (a HOST array) = atlas_w, atlas_h, cells_per_row.
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null out;  n_faces < 0;  texels outside 1 .. EONERF_TEXTURE_MAX_TEXELS
 *   EONERF_E_UNSUPPORTED  atlas_w or atlas_h above EONERF_TEXTURE_MAX_SIDE, or more than 2^31 - 1 texels */
int eonerf_texture_layout(int64_t n_faces, int texels, int64_t out[3]);

/* uv_out float[n_faces][3][2]: per face corner (A, B, C) the atlas coordinate (u / atlas_w, 1 - v / atlas_h) of the rule above, formed in
 * fp64 and cast once -- OBJ's v-up convention.  n_faces == 0 succeeds and writes nothing.
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null uv_out;  n_faces < 0;  texels outside 1 .. EONERF_TEXTURE_MAX_TEXELS
 *   EONERF_E_UNSUPPORTED  the limits of eonerf_texture_layout */
int eonerf_texture_uv(int64_t n_faces, int texels, void* uv_out, void* stream);

/* The samples of the texels [first, first + n) of the atlas, row i of every output belonging to texel first + i:
 *   face_out      int32[n]      the owning face, or -1
 *   bary_out      float[n][3]   the clamped weights of A, B, C, fp64 cast once (NaN for face -1)
 *   xyz_out       float[n][3]   (b0 * A + b1 * B) + b2 * C in fp64 on the widened fp32 vertices (normalised scene frame), cast once
 *   lonlatalt_out double[n][3]  xyz (the fp64 value) * scene_scale + scene_offset, then the inverse UTM of (east, north), as
 *                               eonerf_ortho_ground: lon, lat in degrees, alt in metres
 *   normal_out    float[n][3]   the face's unit normal in the metric frame: n = ((B - A) * scene_scale) x ((C - A) * scene_scale) in fp64,
 *                               n / sqrt((nx^2 + ny^2) + nz^2), cast once; NaN where the length is zero or not finite
 * Each output may be NULL (not all five).  n == 0 succeeds and writes nothing.
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null vertices / triangles / scene_scale / scene_offset;  no output
 *   EONERF_E_ARG          n_vertices < 0, n_faces < 0, first < 0 or n < 0;  texels outside 1 .. EONERF_TEXTURE_MAX_TEXELS
 *   EONERF_E_ARG          a non-finite scale or offset;  a zone outside 1 .. 60
 *   EONERF_E_UNSUPPORTED  more than 2^31 - 1 vertices;  the limits of eonerf_texture_layout
 *   EONERF_E_ARG          first + n beyond atlas_w * atlas_h */
int eonerf_texture_samples(const void* vertices /* float[n_vertices][3] */, int64_t n_vertices, const void* triangles /* int32[n_faces][3] */,
                           int64_t n_faces, int texels, int64_t first, int64_t n, const float scene_scale[3], const float scene_offset[3],
                           int utm_zone, int south, void* face_out, void* bary_out, void* xyz_out, void* lonlatalt_out, void* normal_out,
                           void* stream);

/* The fused gather: per sample a loop over the K images, only the fused result is written.  All tables are DEVICE arrays:
 *   lonlatalt     double[n][3]      as eonerf_texture_samples or eonerf_ortho_ground wrote them
 *   normal        float[n][3]       metric unit normals, or NULL: no incidence test and no angle weight
 *   rpcs          eonerf_rpc[K]     each image's RPC at the image's downscale
 *   pixel_addresses uint64[K]       the device address of each image's fp32 [h, w, channels] pixels (row-major, channel-last, NaN = no data)
 *   shapes        int32[K][2]       h, w of each image
 *   gain, bias    float[K][channels]  the radiometry v_image = gain * v_common + bias
 *   to_satellite  double[K][3]      metric unit vectors from the ground towards each satellite; may be NULL iff normal is NULL
 *   blocked       uint8[K][n]       1 = the mesh occludes image k at sample i; NULL = no occlusion test
 * Per image k the projection, the pixel convention, the bilinear expression, (v - bias) / gain and the cast to fp32 are those of
 * eonerf_ortho_gather, verbatim.  The weight w_k (fp32) is 0 where eonerf_ortho_gather's is 0 (a non-finite point, a projection outside
 * [0, w - 1] x [0, h - 1], a non-finite tap), where h or w < 1, where blocked, where a gain of the image is zero or not finite or a bias
 * not finite, or -- with a normal -- unless cos = (n0 s0 + n1 s1) + n2 s2 >= min_cos (fp64 on the widened values; NaN fails).
 * Otherwise w_k = (float)cos when angle_weight is set and a normal is given, else 1.  An image counts iff w_k > 0.
 *   count_out int32[n]: the images that count;  weight_sum_out float[n]: the fp64 sum of their w_k in ascending k, cast;
 *   best_out int32[n]: the k of the largest w_k, ties to the smaller k, -1 where count is 0;
 *   colour_out float[n][channels]: mode EONERF_TEXTURE_MEAN and EONERF_TEXTURE_MEDIAN exactly as eonerf_ortho_fuse defines them on the
 *   fp32 values and weights (fp64, ascending k, numpy's median), EONERF_TEXTURE_BEST the value of image best; NaN where count is 0.
 * A sample with a NaN point or normal therefore gives a NaN colour and count 0.  Each output may be NULL (not all four).
 * Loops are bounded by K and by EONERF_TEXTURE_MAX_MEDIAN.  n == 0 succeeds and writes nothing.
 * Refused, in this order, with nothing written:
 *   EONERF_E_ARG          a null lonlatalt / rpcs / pixel_addresses / shapes / gain / bias;  a normal without to_satellite;  no output
 *   EONERF_E_ARG          n < 0, K < 1, channels outside 1 .. 4, a mode outside 0 .. 2, angle_weight outside 0 .. 1, a non-finite min_cos
 *   EONERF_E_UNSUPPORTED  EONERF_TEXTURE_MEDIAN with K > EONERF_TEXTURE_MAX_MEDIAN;  K * n * channels beyond 2^62;  n beyond 2^31 - 1
 *                         workgroups of 256 */
int eonerf_texture_bake(const void* lonlatalt, const void* normal, int64_t n, const void* rpcs, const void* pixel_addresses, const void* shapes,
                        int K, int channels, const void* gain, const void* bias, const void* to_satellite, const void* blocked, float min_cos,
                        int angle_weight, int mode, void* colour_out, void* weight_sum_out, void* count_out, void* best_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
