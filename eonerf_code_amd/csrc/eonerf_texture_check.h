// Host side of eonerf_texture.h: the atlas layout, the per-texel ownership and barycentric weights (shared, as __host__ __device__
// functions, with the kernels of eonerf_texture.hip) and the refusals of the entry points with their size arithmetic, in functions with
// no HIP call so that a stand-alone program can include them (tests/host/texture_checks.cpp).  Each check returns 0 or the EONERF_E_*
// the entry point returns before it launches anything.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eonerf_texture.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EO_TEX_HD __host__ __device__
#else
#define EO_TEX_HD
#endif

constexpr int kTextureBlock = 256;

struct TextureLayout {
    int64_t atlas_w, atlas_h, cells_per_row, cells;
    int texels, side;       // T and S = T + EONERF_TEXTURE_GUTTER
};

// ceil(sqrt(c)) for 0 <= c < 2^62 in exact integer arithmetic: the floating root is only a start
inline int64_t texture_ceil_sqrt(int64_t c) {
    if (c <= 0) return 0;
    int64_t r = (int64_t)sqrt((double)c);
    while (r * r < c) ++r;
    while (r > 0 && (r - 1) * (r - 1) >= c) --r;
    return r;
}

// the layout rule of eonerf_texture.h; EONERF_E_ARG / EONERF_E_UNSUPPORTED as eonerf_texture_layout documents them
inline int texture_layout(int64_t n_faces, int texels, TextureLayout* out) {
    if (!out || n_faces < 0 || texels < 1 || texels > EONERF_TEXTURE_MAX_TEXELS) return EONERF_E_ARG;
    TextureLayout l;
    l.texels = texels;
    l.side = texels + EONERF_TEXTURE_GUTTER;
    l.cells = n_faces / 2 + n_faces % 2;                                    // no n_faces + 1: it would wrap at INT64_MAX
    l.cells_per_row = texture_ceil_sqrt(l.cells);
    const int64_t rows = l.cells_per_row ? (l.cells + l.cells_per_row - 1) / l.cells_per_row : 0;
    // cells_per_row < 2^31.5 and side <= 69: the products stay far inside 64 bits
    l.atlas_w = l.cells_per_row * l.side;
    l.atlas_h = rows * l.side;
    if (l.atlas_w > EONERF_TEXTURE_MAX_SIDE || l.atlas_h > EONERF_TEXTURE_MAX_SIDE) return EONERF_E_UNSUPPORTED;
    if (l.atlas_w * l.atlas_h > (int64_t)0x7fffffff) return EONERF_E_UNSUPPORTED;
    *out = l;
    return EONERF_OK;
}

// The owner of texel (x, y) of the atlas: returns the face, or -1 for a texel no face owns, and the clamped weights of A, B, C.
EO_TEX_HD inline int64_t texture_texel(int64_t x, int64_t y, int64_t cells_per_row, int64_t cells, int64_t n_faces, int texels, double b[3]) {
    const int S = texels + EONERF_TEXTURE_GUTTER;
    const int64_t col = x / S, row = y / S;
    const int cx = (int)(x % S), cy = (int)(y % S);
    const int64_t j = row * cells_per_row + col;
    const bool lower = cx + cy <= S - 1;
    const int64_t face = 2 * j + (lower ? 0 : 1);
    if (j >= cells || face >= n_faces) {
        b[0] = b[1] = b[2] = __builtin_nan("");
        return -1;
    }
    const double u = (double)cx + 0.5, v = (double)cy + 0.5, T = (double)texels;
    // A and the two legs: (1.5, 1.5), +T, +T for the lower face; (S - 1.5, S - 1.5), -T, -T for the upper one
    const double ua = lower ? 1.5 : (double)S - 1.5, leg = lower ? T : -T;
    double b1 = (u - ua) / leg, b2 = (v - ua) / leg;
    double b0 = (1.0 - b1) - b2;
    b0 = b0 > 0.0 ? b0 : 0.0;
    b1 = b1 > 0.0 ? b1 : 0.0;
    b2 = b2 > 0.0 ? b2 : 0.0;
    const double s = (b0 + b1) + b2;                                        // >= 1/3 of the largest weight: never zero
    b[0] = b0 / s; b[1] = b1 / s; b[2] = b2 / s;
    return face;
}

// The atlas position (u, v), in texels from the top left, of corner c (0, 1, 2 = A, B, C) of a face.
EO_TEX_HD inline void texture_corner(int64_t face, int c, int64_t cells_per_row, int texels, double* u, double* v) {
    const int S = texels + EONERF_TEXTURE_GUTTER;
    const int64_t j = face / 2, col = j % cells_per_row, row = j / cells_per_row;
    const bool lower = face % 2 == 0;
    const double a = lower ? 1.5 : (double)S - 1.5, leg = lower ? (double)texels : -(double)texels;
    *u = (double)(col * S) + (c == 1 ? a + leg : a);
    *v = (double)(row * S) + (c == 2 ? a + leg : a);
}

// elements of a [K, n, channels] table in 64 bits; false where the product leaves 2^62
inline bool texture_elems(int64_t K, int64_t n, int64_t channels, uint64_t* out) {
    if (K < 0 || n < 0 || channels < 0) return false;
    const uint64_t lim = (uint64_t)1 << 62;
    uint64_t e = (uint64_t)K;
    if (n && e > lim / (uint64_t)n) return false;
    e *= (uint64_t)n;
    if (channels && e > lim / (uint64_t)channels) return false;
    *out = e * (uint64_t)channels;
    return true;
}

// workgroups of kTextureBlock threads over n items; 0 where the grid would leave 2^31 - 1
inline unsigned texture_blocks(int64_t n) {
    if (n <= 0) return 0;
    const uint64_t b = ((uint64_t)n + kTextureBlock - 1) / kTextureBlock;
    return b > 0x7fffffffull ? 0u : (unsigned)b;
}

inline int texture_check_uv(int64_t n_faces, int texels, const void* uv_out, TextureLayout* l) {
    if (!uv_out) return EONERF_E_ARG;
    return texture_layout(n_faces, texels, l);
}

inline int texture_check_samples(const void* vertices, int64_t n_vertices, const void* triangles, int64_t n_faces, int texels, int64_t first,
                                 int64_t n, const float* scene_scale, const float* scene_offset, int utm_zone, const void* face_out,
                                 const void* bary_out, const void* xyz_out, const void* lonlatalt_out, const void* normal_out, TextureLayout* l) {
    if (!vertices || !triangles || !scene_scale || !scene_offset) return EONERF_E_ARG;
    if (!face_out && !bary_out && !xyz_out && !lonlatalt_out && !normal_out) return EONERF_E_ARG;
    if (n_vertices < 0 || n_faces < 0 || first < 0 || n < 0 || texels < 1 || texels > EONERF_TEXTURE_MAX_TEXELS) return EONERF_E_ARG;
    for (int k = 0; k < 3; ++k)
        if (!isfinite(scene_scale[k]) || !isfinite(scene_offset[k])) return EONERF_E_ARG;
    if (utm_zone < 1 || utm_zone > 60) return EONERF_E_ARG;
    if (n_vertices > (int64_t)0x7fffffff) return EONERF_E_UNSUPPORTED;
    const int rc = texture_layout(n_faces, texels, l);
    if (rc != EONERF_OK) return rc;
    const int64_t total = l->atlas_w * l->atlas_h;                          // <= 2^31 - 1
    if (first > total || n > total - first) return EONERF_E_ARG;            // no first + n: it could wrap
    return EONERF_OK;
}

inline int texture_check_bake(const void* lonlatalt, const void* normal, int64_t n, const void* rpcs, const void* pixel_addresses,
                              const void* shapes, int K, int channels, const void* gain, const void* bias, const void* to_satellite,
                              float min_cos, int angle_weight, int mode, const void* colour_out, const void* weight_sum_out,
                              const void* count_out, const void* best_out) {
    if (!lonlatalt || !rpcs || !pixel_addresses || !shapes || !gain || !bias) return EONERF_E_ARG;
    if (normal && !to_satellite) return EONERF_E_ARG;
    if (!colour_out && !weight_sum_out && !count_out && !best_out) return EONERF_E_ARG;
    if (n < 0 || K < 1 || channels < 1 || channels > 4) return EONERF_E_ARG;
    if (mode < EONERF_TEXTURE_MEAN || mode > EONERF_TEXTURE_BEST || angle_weight < 0 || angle_weight > 1 || !isfinite(min_cos)) return EONERF_E_ARG;
    if (mode == EONERF_TEXTURE_MEDIAN && K > EONERF_TEXTURE_MAX_MEDIAN) return EONERF_E_UNSUPPORTED;
    uint64_t e;
    if (!texture_elems(K, n, channels, &e)) return EONERF_E_UNSUPPORTED;
    if (n > 0 && !texture_blocks(n)) return EONERF_E_UNSUPPORTED;
    return EONERF_OK;
}
