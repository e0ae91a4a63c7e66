// Host side of include/eonerf_ortho.h: the refusals of the three entry points and their size arithmetic, in functions with no HIP
// call so that a stand-alone program can include them (tests/host/ortho_checks.cpp).  Each returns 0 or the EONERF_E_* the entry
// point returns before it launches anything.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_ortho.h"

constexpr int kOrthoBlock = 256;

// elements of a [K, n, channels] table in 64 bits; false where the product leaves 2^62 (so that 4- and 8-byte offsets stay in a size_t)
inline bool ortho_elems(int64_t K, int64_t n, int64_t channels, uint64_t* out) {
    if (K < 0 || n < 0 || channels < 0) return false;
    const uint64_t lim = (uint64_t)1 << 62;
    uint64_t e = (uint64_t)K;
    if (n && e > lim / (uint64_t)n) return false;
    e *= (uint64_t)n;
    if (channels && e > lim / (uint64_t)channels) return false;
    *out = e * (uint64_t)channels;
    return true;
}

// workgroups of kOrthoBlock threads over n points; 0 where the grid would leave 2^31 - 1
inline unsigned ortho_blocks(int64_t n) {
    if (n <= 0) return 0;
    const uint64_t b = ((uint64_t)n + kOrthoBlock - 1) / kOrthoBlock;
    return b > 0x7fffffffull ? 0u : (unsigned)b;
}

inline int ortho_check_ground(const void* rays, int ray_stride, const void* depth, long n, const float* scene_scale,
                              const float* scene_offset, int utm_zone, const void* lonlatalt_out) {
    if (!rays || !depth || !scene_scale || !scene_offset || !lonlatalt_out) return EONERF_E_ARG;
    if (n < 0 || ray_stride < 6 || utm_zone < 1 || utm_zone > 60) return EONERF_E_ARG;
    for (int k = 0; k < 3; ++k)
        if (!isfinite(scene_scale[k]) || !isfinite(scene_offset[k])) return EONERF_E_ARG;
    if (n > 0 && !ortho_blocks(n)) return EONERF_E_UNSUPPORTED;
    return EONERF_OK;
}

inline int ortho_check_gather(const void* lonlatalt, long n, const void* rpc, const void* pixels, int h, int w, int channels,
                              const float* gain, const float* bias, float min_visibility, const void* layer_out, const void* weight_out,
                              const void* colrow_out) {
    if (!lonlatalt || !rpc || n < 0) return EONERF_E_ARG;
    if (!layer_out && !weight_out && !colrow_out) return EONERF_E_ARG;
    if (h < 1 || w < 1 || channels < 1 || channels > 4) return EONERF_E_ARG;
    if (!isfinite(min_visibility)) return EONERF_E_ARG;
    if (layer_out || weight_out) {
        if (!pixels || !gain || !bias) return EONERF_E_ARG;
    }
    if (gain)
        for (int c = 0; c < channels; ++c)
            if (!(gain[c] != 0.f) || !isfinite(gain[c])) return EONERF_E_ARG;
    if (bias)
        for (int c = 0; c < channels; ++c)
            if (!isfinite(bias[c])) return EONERF_E_ARG;
    uint64_t e;
    if (!ortho_elems(1, n, channels, &e) || !ortho_elems(h, w, channels, &e)) return EONERF_E_UNSUPPORTED;
    if (n > 0 && !ortho_blocks(n)) return EONERF_E_UNSUPPORTED;
    return EONERF_OK;
}

inline int ortho_check_fuse(const void* layers, const void* weights, int K, long n, int channels, int mode, const void* mosaic_out,
                            const void* weight_sum_out, const void* count_out) {
    if (!layers || !weights || n < 0 || K < 1 || channels < 1 || channels > 4) return EONERF_E_ARG;
    if (mode != EONERF_ORTHO_MEAN && mode != EONERF_ORTHO_MEDIAN) return EONERF_E_ARG;
    if (!mosaic_out && !weight_sum_out && !count_out) return EONERF_E_ARG;
    if (mode == EONERF_ORTHO_MEDIAN && K > EONERF_ORTHO_MAX_MEDIAN) return EONERF_E_UNSUPPORTED;
    uint64_t e;
    if (!ortho_elems(K, n, channels, &e)) return EONERF_E_UNSUPPORTED;
    if (n > 0 && !ortho_blocks(n)) return EONERF_E_UNSUPPORTED;
    return EONERF_OK;
}
