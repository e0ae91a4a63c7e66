// Host side of include/eonerf_normals.h: the refusals of eonerf_field_density_grad / eonerf_render_normals in their documented order and
// the size arithmetic (64-bit), in functions with no HIP call so that a stand-alone program can include them
// (tests/host/normals_checks.cpp).  Each check returns 0 or the EONERF_E_* the entry point returns before it launches anything.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_normals.h"

// sample capacity of `n` units of `per` samples each (points: per = 1; rays: per = n_samples - 1), as eonerf_carve.h's p_cap_of /
// field_p_cap_of form it, in 64 bits; 0 where a call does not take that many: four chain columns per sample must stay an int
inline uint64_t normals_p_cap(int64_t n, int per) {
    if (n < 0 || per < 1 || per > 255) return 0;
    const uint64_t units = n > 0 ? (uint64_t)n : 1;
    const uint64_t cap = (units * (uint64_t)per + 255) / 256 * 256;
    return cap > (uint64_t)EONERF_NORMALS_MAX_POINTS ? 0 : cap;
}
// rays one call takes: eonerf_render_forward's own bound (eonerf_ctx.h: rays_in_range) and the capacity above
inline bool normals_rays_ok(int64_t n_rays, int n_samples) {
    if (n_samples < 2 || n_samples > 256) return false;
    if (n_rays > (1 << 24) / (n_samples > 128 ? n_samples / 128 : 1)) return false;
    return normals_p_cap(n_rays, n_samples - 1) != 0;
}
inline int64_t normals_max_rays(int n_samples) {
    if (n_samples < 2 || n_samples > 256) return 0;
    const int64_t by_cap = (int64_t)EONERF_NORMALS_MAX_POINTS / (n_samples - 1);
    const int64_t by_fwd = (1 << 24) / (n_samples > 128 ? n_samples / 128 : 1);
    return by_cap < by_fwd ? by_cap : by_fwd;
}

// the gradient planes [3][p_cap] fp32 follow the pass' own layout (`pass_bytes` = its size, 256 bytes of slack included), 256-byte aligned
struct NormalsExt { size_t grad_off, bytes; };
inline NormalsExt normals_ext(size_t pass_bytes, uint64_t p_cap) {
    NormalsExt e;
    const uint64_t off = ((uint64_t)(pass_bytes - 256) + 255) & ~(uint64_t)255;
    e.grad_off = (size_t)off;
    e.bytes = (size_t)(off + 3 * p_cap * sizeof(float) + 256);
    return e;
}

inline bool normals_axis_ok(const float* axis_scale) {
    if (!axis_scale) return true;
    for (int k = 0; k < 3; ++k)
        if (!isfinite(axis_scale[k]) || axis_scale[k] == 0.0f) return false;
    return true;
}

// eonerf_field_density_grad, up to the workspace check.  *empty: n == 0, the call returns EONERF_OK without doing anything
inline int normals_points_refusal(const void* ctx, const void* flat, const void* xyz, const void* sigma, const void* grad, const void* ws,
                                  int n, bool weights_set, int precision, bool* empty) {
    *empty = false;
    if (!ctx || !flat || !xyz || !sigma || !grad || !ws || n < 0) return EONERF_E_ARG;
    if (!weights_set) return EONERF_E_STATE;
    if (precision == EONERF_BF16) return EONERF_E_UNSUPPORTED;
    if (n == 0) { *empty = true; return EONERF_OK; }
    if (!normals_p_cap(n, 1)) return EONERF_E_UNSUPPORTED;
    return EONERF_OK;
}

// eonerf_render_normals, up to the workspace check
inline int normals_render_refusal(const void* ctx, const void* flat, const void* rays, const void* zsteps, const void* out, const void* ws,
                                  int n_rays, bool weights_set, int n_exports /* of 5 */, const float* axis_scale, int precision,
                                  bool has_u_cam, bool has_u_retry, int n_samples, bool* empty) {
    *empty = false;
    if (!ctx || !flat || !rays || !zsteps || !out || !ws || n_rays < 0) return EONERF_E_ARG;
    if (!weights_set) return EONERF_E_STATE;
    if (n_exports != 0 && n_exports != 5) return EONERF_E_ARG;
    if (!normals_axis_ok(axis_scale)) return EONERF_E_ARG;
    if (precision == EONERF_BF16) return EONERF_E_UNSUPPORTED;
    if (n_rays == 0) { *empty = true; return EONERF_OK; }
    if (!has_u_cam && has_u_retry) return EONERF_E_ARG;
    if (!normals_rays_ok(n_rays, n_samples)) return EONERF_E_UNSUPPORTED;
    return EONERF_OK;
}

inline int normals_check_workspace(size_t ws_bytes, size_t need) { return ws_bytes < need ? EONERF_E_WORKSPACE : EONERF_OK; }
