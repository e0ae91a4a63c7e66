// What the round-based passes share (eonerf_march.hip, eonerf_quantile.hip): the argument block of a round's launches, the launchers of
// the begin and windowed-emit kernels (defined in eonerf_march.hip) and the device helpers that form one window of a ray.  Include it
// from translation units built with -ffp-contract=off only: the sample arithmetic is sample_ray's, bit for bit.
#pragma once
#include "eonerf_carve.h"
#include "eonerf_rays_dev.h"

struct MarchArgs {
    SampleArgs s;              // geometry, noise, grid; the round's compact outputs, offsets / counts / n_pts; cnt_first / cnt_retry (full counts); flags
    int round, block;
    int decide;                // 1 (round 0 of the camera pass): the emit takes the "resample if any ray is empty" decision and leaves it in flags[0]
    int *win_a, *win_b;        // [R] valid slots of the ray's NEXT window, per draw (win_b: the retry draw, read by the deciding round only)
    int *last_a, *last_b;      // [R] the ray's last valid slot per draw, -1: none
    int* n_total;              // += the round's sample count (the caller's n_samples_dev), or nullptr
    int *alive, *kept; float *od, *acc;      // march state: still marching, kept samples, optical depth carried, [R][MARCH_ACC] sums (camera pass)
    float* geo;                // shadow pass: the ray record's RR_GEO column (stride RAY_REC), or nullptr
    float eps;
    const float *sigma, *albedo, *ts, *tb; int p_pad, depth_only;
};

// eonerf_march.hip: the begin of a pass (full counts, last valid slots, first window counts, march state) and one round's windowed emit
hipError_t eo_march_launch_begin(const MarchArgs& m, hipStream_t st);
hipError_t eo_march_launch_emit(const MarchArgs& m, hipStream_t st);

// the round buffers as a sampler's outputs
inline void round_outputs(SampleArgs& s, const MarchWs& w) {
    s.counts = w.round.counts; s.offsets = w.round.offsets; s.n_pts = w.round.n_pts; s.n_pts_copy = nullptr;
    s.px = w.round.px; s.py = w.round.py; s.pz = w.round.pz; s.tmid = w.round.tmid; s.delta = w.round.delta; s.simg = w.round.simg;
}

namespace {

// jitter of slot i of draw `draw` of ray `ray`: the value jitter<SPL> hands to lane i & 63, slot i >> 6
EO_DEV float jitter_at(const SampleArgs& a, const float* u_arr, int draw, int ray, int i) {
    if (u_arr) return u_arr[(size_t)ray * a.n_samples + i];      // i < n_samples
    float u4[4];
    philox_u4(a.seed, (uint32_t)ray, (uint32_t)(i & 63), (uint32_t)draw, a.call, u4);
    const int k = i >> 6;
    return k == 0 ? u4[0] : (k == 1 ? u4[1] : (k == 2 ? u4[2] : u4[3]));
}
EO_DEV float z_at(const SampleArgs& a, const float* u_arr, int draw, float near, int ray, int i) {
    return a.perturb ? zperturbed(a.zsteps, near, i, jitter_at(a, u_arr, draw, ray, i), a.n_samples) : zval(a.zsteps, near, i);
}

// slot i of a ray as sample_ray forms it (its own z value; the neighbour's by shuffle, the one beyond the window formed by its last lane), with cull_by_grid's rule from the
// ray's last cube-valid slot `last`.  in_win: the lane holds a slot of the window
struct WinSample { float ts, te, mid, x, y, z; bool valid; };
template <bool GRID>
EO_DEV WinSample window_sample(const SampleArgs& a, const float* u_arr, int draw, float near, const RayGeom& g, int ray, int i, bool in_win, bool last_of_win, int last) {
    WinSample s;
    s.ts = s.te = s.mid = s.x = s.y = s.z = 0.f; s.valid = false;
    // every lane of the wave comes here: z_i once per lane, the neighbour's by shuffle; only the window's last lane forms z_{i+1} itself
    const int ns = a.n_samples;
    const float zi = (in_win && i < ns) ? z_at(a, u_arr, draw, near, ray, i) : 0.f;
    float zn = __shfl_down(zi, 1, 64);
    if (last_of_win && i + 1 < ns) zn = z_at(a, u_arr, draw, near, ray, i + 1);
    if (in_win && i < ns - 1) {      // interval i = [z_i, z_{i+1}], i < n_samples - 1
        const float zs = zi;
        s.ts = zs;
        s.te = __fadd_rn(zs, __fsub_rn(zn, zs));
        s.mid = __fdiv_rn(__fadd_rn(s.ts, s.te), 2.0f);
        s.x = __fadd_rn(g.ox, __fmul_rn(g.dx, s.mid));
        s.y = __fadd_rn(g.oy, __fmul_rn(g.dy, s.mid));
        s.z = __fadd_rn(g.oz, __fmul_rn(g.dz, s.mid));
        s.valid = fabsf(s.x) < 1.0f && fabsf(s.y) < 1.0f && fabsf(s.z) < 1.0f;
        if constexpr (GRID) { if (s.valid) s.valid = occ_bit(a.occ_bits, a.occ_r, s.x, s.y, s.z) || i == last; }
    }
    return s;
}
EO_DEV int pass_draw(const SampleArgs& a, bool retry) { return retry ? 1 : (a.sun_pass ? 2 : 0); }

template <bool GRID>
EO_DEV WinSample window_of(const MarchArgs& m, int ray, int lane, int round, bool retry, int last) {
    const SampleArgs& a = m.s;
    const RayGeom g = ray_geom(a, ray);
    return window_sample<GRID>(a, retry ? a.u_retry : a.u, pass_draw(a, retry), retry ? 0.f : g.near, g, ray, round * m.block + lane, lane < m.block, lane == m.block - 1, last);
}
// valid slots of window `round` of a ray (0 without forming a sample when the ray's last valid slot lies in front of it)
template <bool GRID>
EO_DEV int window_count(const MarchArgs& m, int ray, int lane, int round, bool retry) {
    const int last = retry ? m.last_b[ray] : m.last_a[ray];
    if (last < round * m.block) return 0;
    return __popcll(__ballot(window_of<GRID>(m, ray, lane, round, retry, last).valid));
}

template <class F> void dispatch_grid(const uint32_t* bits, F&& f) { if (bits) f(std::true_type()); else f(std::false_type()); }

}  // namespace
