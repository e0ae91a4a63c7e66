// Device helpers shared by the per-ray forward and backward kernels.
#pragma once
#include "eonerf_common.h"
#include "eonerf_rays.h"
#include <type_traits>

namespace {

constexpr int RAYS_PER_BLOCK = 4;   // 256 threads

// ---- wave helpers -------------------------------------------------------------------------------------------
EO_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scan across the 64 lanes
EO_DEV float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// inclusive SUFFIX scan (sum over lanes >= lane)
EO_DEV float wave_suffix_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float t = __shfl_down(v, o, 64);
        if (lane + o < 64) v += t;
    }
    return v;
}

// ---- Philox4x32-10 (Salmon et al. 2011, the generator behind torch.rand on GPUs): counter = (ray, lane, draw, call), key = seed;
//      24 random bits -> [0, 1) fp32, as torch.rand.  Draws 0 (camera), 1 (camera retry), 2 (sun): the sampler; 3: the occupancy
//      grid's per-cell sample point (eonerf_occ.hip, counter = (cell, 0, 3, call))
EO_DEV void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
}
EO_DEV void philox_u4(uint64_t seed, uint32_t ray, uint32_t lane, uint32_t draw, uint32_t call, float (&u)[4]) {
    uint32_t c[4] = {ray, lane, draw, call};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = (float)(c[k] >> 8) * 0x1p-24f;
}

// ---- occupancy grid (include/eonerf_occ.h): cell of a point, per axis min(r - 1, (int)(((x + 1) * 0.5f) * (float)r)) as three
//      separately rounded fp32 operations; the clamps keep the index inside [0, r) whatever x holds (x + 1 == 2.0f at x = 1 - 2^-24;
//      the lower clamp never acts on a cube-valid coordinate, |x| < 1) -----------------------------------------------------------
EO_DEV int occ_axis(float x, int r) {
    const int i = (int)__fmul_rn(__fmul_rn(__fadd_rn(x, 1.0f), 0.5f), (float)r);
    return i < 0 ? 0 : (i > r - 1 ? r - 1 : i);
}
EO_DEV bool occ_bit(const uint32_t* bits, int r, float x, float y, float z) {
    const uint32_t c = (uint32_t)((occ_axis(x, r) * r + occ_axis(y, r)) * r + occ_axis(z, r));      // < r^3 <= 2^24
    return (bits[c >> 5] >> (c & 31)) & 1u;
}

// ---- ambient head for one ray, computed by the whole wave (radiance_fields/eonerf.py:132-139,163-164) ------
struct AmbientRay { float out[3]; float hid[2]; float pre[3]; float enc[27]; };

EO_DEV void sun_encoding(float sx, float sy, float sz, float* enc) {   // mlp.py:190-208, L=4, fp32
    enc[0] = sx; enc[1] = sy; enc[2] = sz;
    const float c[3] = {sx, sy, sz};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float xb = c[d] * (float)(1 << k);
            enc[3 + 3 * k + d] = sinf(xb);
            enc[15 + 3 * k + d] = sinf(xb + EO_PI_2_F);
        }
}

// one encoding element per lane (lanes 0..26), broadcast with shuffles: same arithmetic as sun_encoding
EO_DEV void sun_encoding_wave(float sx, float sy, float sz, int lane, float* enc) {
    float v = 0.f;
    if (lane < 27) {
        if (lane < 3) v = lane == 0 ? sx : (lane == 1 ? sy : sz);
        else {
            const int q = (lane - 3) % 12, k = q / 3, d = q % 3;
            const float c = d == 0 ? sx : (d == 1 ? sy : sz);
            const float xb = c * (float)(1 << k);
            v = lane < 15 ? sinf(xb) : sinf(xb + EO_PI_2_F);
        }
    }
#pragma unroll
    for (int i = 0; i < 27; ++i) enc[i] = __shfl(v, i, 64);
}

EO_DEV AmbientRay ambient_forward(const AmbientW& w, float sx, float sy, float sz, int lane) {
    AmbientRay r;
    sun_encoding_wave(sx, sy, sz, lane, r.enc);
    float part[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        float acc = w.b1[j];
        for (int i = 0; i < 27; ++i) acc = fmaf(w.w1[j * 27 + i], r.enc[i], acc);
        r.hid[k] = fmaxf(acc, 0.f);
#pragma unroll
        for (int o = 0; o < 3; ++o) part[o] = fmaf(w.w2[o * 128 + j], r.hid[k], part[o]);
    }
#pragma unroll
    for (int o = 0; o < 3; ++o) { r.pre[o] = wave_sum(part[o]) + w.b2[o]; r.out[o] = sigmoid_f(r.pre[o]); }
    return r;
}

// ---- compositing forward ------------------------------------------------------------------------------------
//   sd = sigma*delta;  T = exp(-exclusive_sum(sd));  alpha = 1-exp(-sd);  w = T*alpha   (nerfacc v0.5.2 volrend,
//   call sites radiance_fields/eonerf.py:229-243)            per-ray sums of w*{mid, albedo, ts, tb, 1}
// SPL = samples per lane: a ray has n_samples - 1 = 64 SPL - 1 intervals at most (n_samples = int(2 / render_step_size) = 64, 128 or
// 256, sat_rendering.py:64), element i = lane + 64 k sits in slot k of its lane
template <int SPL> struct RayWeights { float w[SPL], T[SPL], sd[SPL]; float total; };

template <int SPL>
EO_DEV RayWeights<SPL> ray_weights(const float* sigma, const float* delta, int off, int n, int lane) {
    RayWeights<SPL> r;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        r.sd[k] = i < n ? sigma[off + i] * delta[off + i] : 0.f;
    }
    // exclusive prefix = inclusive prefix of the PREVIOUS lane (never "inclusive - self": the last interval has
    // sigma*delta ~ 1e10 and would cancel the whole prefix), plus the total of the 64-element groups in front
    float carry = 0.f, ex[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const float inc = wave_incl_scan(r.sd[k], lane);
        const float prev = __shfl_up(inc, 1, 64);
        ex[k] = lane == 0 ? carry : carry + prev;
        carry += __shfl(inc, 63, 64);
    }
    r.total = carry;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        r.T[k] = expf(-ex[k]);
        r.w[k] = i < n ? r.T[k] * (1.f - expf(-r.sd[k])) : 0.f;
    }
    return r;
}

// run f(std::integral_constant<int, SPL>) for the sample slots per lane n_samples needs (<= 64 -> 1, <= 128 -> 2, <= 256 -> 4)
template <class F> inline void eo_dispatch_spl(int n_samples, F&& f) {
    if (n_samples <= 64) f(std::integral_constant<int, 1>());
    else if (n_samples > 128) f(std::integral_constant<int, 4>());      // (129 .. 256: a three-slot instance would save a quarter of the per-ray work of kernels that are < 2 % of a step)
    else f(std::integral_constant<int, 2>());
}


}  // namespace
