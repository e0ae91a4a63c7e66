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

// ---- the SatNeRF sampler for one ray (sat_rendering.py:46-84), evaluated without FMA contraction so that
//      t values and the cube-filter decisions are bit-identical to the reference's fp32 torch ops ------------
template <int SPL> struct RaySamples {
    float ts[SPL], te[SPL], mid[SPL], x[SPL], y[SPL], z[SPL];
    bool valid[SPL];
};

EO_DEV float zval(const float* zsteps, float near, int i) {
    // near * (1 - s) + (near + 2) * s      (sat_rendering.py:60-68)
    const float s = zsteps[i];
    return __fadd_rn(__fmul_rn(near, __fsub_rn(1.0f, s)), __fmul_rn(__fadd_rn(near, 2.0f), s));
}
// ns = n_samples = int(2 / render_step_size) (sat_rendering.py:64); zsteps = linspace(0, 1, ns)
EO_DEV float zperturbed(const float* zsteps, float near, int i, float u, int ns) {
    const float zi = zval(zsteps, near, i);
    const float lower = i == 0 ? zi : __fmul_rn(0.5f, __fadd_rn(zval(zsteps, near, i - 1), zi));
    const float upper = i == ns - 1 ? zi : __fmul_rn(0.5f, __fadd_rn(zi, zval(zsteps, near, i + 1)));
    return __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), u));       // perturb_z_vals, :46-54
}

// ---- jitter source: caller-provided arrays (parity tests, torch.rand) or the in-kernel Philox4x32-10 stream (philox_u4, eonerf_rays_dev.h):
//      counter = (ray, lane, draw, call), key = seed; one counter gives the lane's (up to four) jitters (samples lane + 64 k)
// jitters of samples lane + 64 k of draw `draw` (0 camera, 1 camera retry, 2 sun) of ray `ray`
template <int SPL>
EO_DEV void jitter(const SampleArgs& a, const float* u_arr, int draw, int ray, int lane, float (&u)[SPL]) {
    if (u_arr) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) u[k] = lane + 64 * k < a.n_samples ? u_arr[(size_t)ray * a.n_samples + lane + 64 * k] : 0.f;      // [R][n_samples]
    } else {
        float u4[4];
        philox_u4(a.seed, (uint32_t)ray, (uint32_t)lane, (uint32_t)draw, a.call, u4);
#pragma unroll
        for (int k = 0; k < SPL; ++k) u[k] = u4[k];
    }
}

template <int SPL>
EO_DEV RaySamples<SPL> sample_ray(const float* zsteps, int ns, bool perturb, const float (&u)[SPL], float near, float ox, float oy, float oz,
                                  float dx, float dy, float dz, int lane) {
    RaySamples<SPL> s;
    float zs[SPL], zn[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {      // perturb=False: :70-71 skipped.  Slots beyond the last z value repeat it (never used: masked below)
        const int i = lane + 64 * k < ns ? lane + 64 * k : ns - 1;
        zs[k] = perturb ? zperturbed(zsteps, near, i, u[k], ns) : zval(zsteps, near, i);
    }
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        zn[k] = __shfl_down(zs[k], 1, 64);
        if (k + 1 < SPL) { const float z0 = __shfl(zs[k + 1 < SPL ? k + 1 : k], 0, 64); if (lane == 63) zn[k] = z0; }      // (last group, lane 63: interval NS - 1 does not exist)
    }
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        s.ts[k] = zs[k];
        s.te[k] = __fadd_rn(zs[k], __fsub_rn(zn[k], zs[k]));               // a + (b - a), :74
        s.mid[k] = __fdiv_rn(__fadd_rn(s.ts[k], s.te[k]), 2.0f);           // :79
        s.x[k] = __fadd_rn(ox, __fmul_rn(dx, s.mid[k]));                    // :80
        s.y[k] = __fadd_rn(oy, __fmul_rn(dy, s.mid[k]));
        s.z[k] = __fadd_rn(oz, __fmul_rn(dz, s.mid[k]));
        const bool inside = fabsf(s.x[k]) < 1.0f && fabsf(s.y[k]) < 1.0f && fabsf(s.z[k]) < 1.0f;   // :18-22
        s.valid[k] = inside && lane + 64 * k < ns - 1;      // interval i = [z_i, z_{i+1}], i < n_samples - 1 (:74-76)
    }
    return s;
}
template <int SPL> EO_DEV int count_valid(const RaySamples<SPL>& s) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < SPL; ++k) n += __popcll(__ballot(s.valid[k]));
    return n;
}

// ---- occupancy culling (include/eonerf_occ.h): of the cube-valid samples of a ray keep those whose cell's bit is set, and the LAST
//      cube-valid one whatever its cell says -- a ray has a sample exactly when it has one without the grid (the "resample if any ray
//      is empty" decision is the same decision) and patch_last's 1e10 interval lands on the same sample.  The last slot follows from
//      the ballots: the highest non-empty group, then 63 - clz.  Only cube-valid lanes look a bit up, with the clamped cell index
template <int SPL>
EO_DEV void cull_by_grid(RaySamples<SPL>& s, const uint32_t* bits, int r, int lane) {
    int top = -1, last_lane = -1;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const unsigned long long m = __ballot(s.valid[k]);
        if (m) { top = k; last_lane = 63 - __clzll(m); }
    }
#pragma unroll
    for (int k = 0; k < SPL; ++k)
        if (s.valid[k]) s.valid[k] = occ_bit(bits, r, s.x[k], s.y[k], s.z[k]) || (k == top && lane == last_lane);
}

struct RayGeom { float ox, oy, oz, dx, dy, dz, near; };

// camera rays come from the [R,11] table; sun rays start at the rendered surface point and look at the sun
// (sat_rendering.py:90-91: origin = o + depth*d, dir = -sundir, near = 0)
EO_DEV RayGeom sun_geom(const float* r, float depth) {
    RayGeom g;
    g.ox = __fadd_rn(r[0], __fmul_rn(depth, r[3]));
    g.oy = __fadd_rn(r[1], __fmul_rn(depth, r[4]));
    g.oz = __fadd_rn(r[2], __fmul_rn(depth, r[5]));
    g.dx = -r[8]; g.dy = -r[9]; g.dz = -r[10];
    g.near = 0.f;
    return g;
}
EO_DEV RayGeom ray_geom(const SampleArgs& a, int ray) {
    const float* r = a.rays + (size_t)ray * 11;
    RayGeom g;
    if (a.sun_pass) {
        g = sun_geom(r, a.depth[(size_t)ray * a.depth_stride]);
    } else {
        g.ox = r[0]; g.oy = r[1]; g.oz = r[2]; g.dx = r[3]; g.dy = r[4]; g.dz = r[5];
        g.near = r[6];
    }
    return g;
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
template <int SPL> struct RayWeights { float w[SPL], T[SPL], sd[SPL]; float total; float ex[SPL]; };      // ex: the exclusive prefix of sd (T = exp(-ex))

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
    float carry = 0.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const float inc = wave_incl_scan(r.sd[k], lane);
        const float prev = __shfl_up(inc, 1, 64);
        r.ex[k] = lane == 0 ? carry : carry + prev;
        carry += __shfl(inc, 63, 64);
    }
    r.total = carry;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int i = lane + 64 * k;
        r.T[k] = expf(-r.ex[k]);
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
