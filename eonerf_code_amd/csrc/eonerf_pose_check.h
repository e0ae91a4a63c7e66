// Host side of include/eonerf_pose.h: the refusals of eonerf_render_origin_grad and its size arithmetic (64-bit), in functions with no
// HIP call so that a stand-alone program can include them (tests/host/pose_checks.cpp).  Each check returns 0 or the EONERF_E_* the
// entry point returns before it launches anything.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/eonerf_pose.h"

// sample capacity of a pass, as eonerf_carve.h's p_cap_of forms it, in 64 bits; 0 where it would leave an int
inline uint64_t pose_p_cap(int64_t n_rays, int n_samples) {
    if (n_rays < 0 || n_samples < 2 || n_samples > 256) return 0;
    const uint64_t rays = n_rays > 0 ? (uint64_t)n_rays : 1;
    const uint64_t cap = (rays * (uint64_t)(n_samples - 1) + 255) / 256 * 256;
    return cap > 0x7fffff00ull ? 0 : cap;
}

// scratch layout: [3][p_cap] fp32 d position of the camera samples, then [n_rays][3] fp32 per-ray sums (used when the caller passes
// no d_origins), each 256-byte aligned
struct PoseScratch { size_t g_pos_off, rays_off, bytes; };
inline bool pose_scratch(int64_t n_rays, int n_samples, PoseScratch* out) {
    const uint64_t cap = pose_p_cap(n_rays, n_samples);
    if (!cap) return false;
    const uint64_t a = 3 * cap * sizeof(float);
    const uint64_t rays_off = (a + 255) & ~(uint64_t)255;
    const uint64_t b = 3 * (uint64_t)n_rays * sizeof(float);
    out->g_pos_off = 0; out->rays_off = (size_t)rays_off; out->bytes = (size_t)(((rays_off + b + 255) & ~(uint64_t)255) + 256);
    return true;
}

inline int pose_check_args(const void* ctx, const void* flat, const void* rays, const void* img_idx, int n_rays, int flags, const void* ws,
                           const void* scratch, const void* d_origins, const void* d_offsets) {
    if (!ctx || !flat || !rays || !img_idx || !ws || !scratch || n_rays < 0) return EONERF_E_ARG;
    if (!d_origins && !d_offsets) return EONERF_E_ARG;
    if (!(flags & EONERF_F_TRAIN) || (flags & EONERF_F_ONLY_DEPTH)) return EONERF_E_STATE;
    return EONERF_OK;
}

// the order rule: the call must find the record of a completed backward with its own workspace, batch size, flags and sample count
inline int pose_check_record(bool valid, const void* rec_ws, int rec_n_rays, int rec_flags, int rec_n_samples,
                             const void* ws, int n_rays, int flags, int n_samples) {
    if (!valid || rec_ws != ws || rec_n_rays != n_rays || rec_flags != flags || rec_n_samples != n_samples) return EONERF_E_STATE;
    return EONERF_OK;
}

inline int pose_check_sizes(int n_rays, int n_samples, size_t ws_bytes, size_t ws_need, size_t scratch_bytes) {
    PoseScratch s;
    if (!pose_scratch(n_rays, n_samples, &s)) return EONERF_E_UNSUPPORTED;
    if (ws_bytes < ws_need || scratch_bytes < s.bytes) return EONERF_E_WORKSPACE;
    return EONERF_OK;
}
