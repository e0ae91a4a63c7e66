// Host-only checks of eonerf_code_amd/csrc/eonerf_smooth.h (eonerf_smooth_check.h), built for the CPU under the address +
// undefined-behaviour sanitizers (tests/host/test_smooth_host.py): every refusal in its documented order, the 64-bit size arithmetic
// at the limits (2^31 - 1 vertices, 2^29 triangles), rdiv on negative numerators and at |D| near 2^62, ties-to-even of the
// quantisation, the limit at both ends, and the rule itself -- the functions the kernels of eonerf_smooth.hip call per lane, run here
// in a loop.  No HIP runtime call is made and no device pointer is dereferenced.
//   smooth_checks             the checks
//   smooth_checks IN OUT      also smooths the mesh in IN (int64 V T, int32 pin_open has_mask n_steps 0, float origin[3] unit[3],
//                             int32 lam_q[n_steps], float vertices[V][3], int32 triangles[T][3], uint8 pinned[V] if has_mask) and writes
//                             OUT (int64 counts[6], int32 status, float vertices[V][3])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_smooth_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers

struct Result { int64_t counts[6] = {0, 0, 0, 0, 0, 0}; int32_t status = 0; std::vector<float> vertices; };
struct Rec { int32_t q[3]; int flags; };

// build + run as the kernels do them, one vertex and one face after the other
static Result run(const SmoothGrid& g, const std::vector<float>& vertices, const std::vector<int32_t>& triangles, const uint8_t* pinned, bool pin_open,
                  const std::vector<int32_t>& steps) {
    const int64_t nv = (int64_t)vertices.size() / 3, nt = (int64_t)triangles.size() / 3;
    std::vector<Rec> a((size_t)nv), b((size_t)nv);
    std::vector<uint32_t> cnt((size_t)nv, 0), start((size_t)nv + 1, 0), cursor((size_t)nv, 0);
    Result r;
    for (int64_t v = 0; v < nv; ++v) a[(size_t)v].flags = smooth_quantise(g, &vertices[(size_t)v * 3], a[(size_t)v].q) ? SMOOTH_QUANTISABLE : 0;
    auto flags_of = [&a](int32_t v) { return a.at((size_t)v).flags; };
    for (int64_t t = 0; t < nt; ++t) {
        const int32_t* tri = &triangles[(size_t)t * 3];
        if (!smooth_live(tri, nv, flags_of)) { ++r.counts[5]; continue; }
        for (int k = 0; k < 3; ++k) ++cnt.at((size_t)tri[k]);
    }
    for (int64_t v = 0; v < nv; ++v) start[(size_t)v + 1] = start[(size_t)v] + cnt[(size_t)v];
    std::vector<uint32_t> next(start[(size_t)nv]), prev(start[(size_t)nv]);
    for (int64_t t = nt - 1; t >= 0; --t) {                                   // (backwards: the order inside a list may not matter)
        const int32_t* tri = &triangles[(size_t)t * 3];
        if (!smooth_live(tri, nv, flags_of)) continue;
        for (int k = 0; k < 3; ++k) {
            const size_t v = (size_t)tri[k], at = start[v] + cursor[v]++;
            next.at(at) = (uint32_t)tri[(k + 1) % 3];
            prev.at(at) = (uint32_t)tri[(k + 2) % 3];
        }
    }
    for (int64_t v = 0; v < nv; ++v) {
        int64_t B1 = 0;
        uint64_t B2 = 0;
        for (uint32_t k = start[(size_t)v]; k < start[(size_t)v + 1]; ++k) smooth_balance(next[k], prev[k], &B1, &B2);
        const bool held = pinned && pinned[v] != 0;
        Rec& rec = a[(size_t)v];
        rec.flags = smooth_flags((rec.flags & SMOOTH_QUANTISABLE) != 0, cnt[(size_t)v], B1, B2, held, pin_open);
        const int bits = smooth_count_bits(rec.flags, cnt[(size_t)v], held);
        for (int k = 0; k < 5; ++k) r.counts[k] += (bits >> k) & 1;
    }
    for (int32_t lam : steps) {
        bool clamped = false;
        for (int64_t v = 0; v < nv; ++v) {
            Rec rec = a[(size_t)v];
            if (rec.flags & SMOOTH_FREE) {
                int64_t S[3] = {0, 0, 0};
                for (uint32_t k = start[(size_t)v]; k < start[(size_t)v + 1]; ++k)
                    for (int c = 0; c < 3; ++c) S[c] += (int64_t)a.at(next[k]).q[c] + a.at(prev[k]).q[c];
                for (int c = 0; c < 3; ++c) rec.q[c] = smooth_step(rec.q[c], S[c], 2 * (int64_t)cnt[(size_t)v], lam, &clamped);
            }
            b[(size_t)v] = rec;
        }
        a.swap(b);
        if (clamped) r.status |= EONERF_SMOOTH_STATUS_CLAMPED;
    }
    r.vertices = vertices;
    for (int64_t v = 0; v < nv; ++v)
        if (a[(size_t)v].flags & SMOOTH_FREE)
            for (int c = 0; c < 3; ++c) r.vertices[(size_t)v * 3 + c] = smooth_dequantise(g, c, a[(size_t)v].q[c]);
    return r;
}

int main(int argc, char** argv) {
    const float nan_ = nanf(""), inf_ = INFINITY;
    const float org[3] = {-1.f, -1.f, -1.f}, uni[3] = {0.25f, 0.25f, 0.5f};
    const int64_t lim = kSmoothLim;

    // ---------------------------------------------------------------- sizes
    {
        const int64_t vmax = kSmoothMaxVertices, tmax = kSmoothMaxTriangles;
        const SmoothCarve c = smooth_carve((uint64_t)vmax, (uint64_t)tmax);
        CHECK(c.lv.count == 4 && c.lv.m[0] == 1u << 21 && c.lv.m[1] == 2048 && c.lv.m[2] == 2 && c.lv.m[3] == 1, "levels at the limit: %d", c.lv.count);
        CHECK(c.q_off[0] == 0 && c.q_off[1] >= (size_t)vmax * 16 && c.q_off[2] >= c.q_off[1] + (size_t)vmax * 16 && c.cnt_off >= c.q_off[2] + (size_t)vmax * 16, "three tables in 64 bits");
        CHECK(c.cursor_off >= c.cnt_off + (size_t)vmax * 4 && c.start_off >= c.cursor_off + (size_t)vmax * 4 && c.corner_off >= c.start_off + (size_t)vmax * 4, "per vertex");
        CHECK(c.lv.off[0] >= c.corner_off + (size_t)tmax * 24, "the corners: 24 bytes a triangle");
        CHECK(c.bytes > (size_t)vmax * 60 + (size_t)tmax * 24 && c.bytes < (size_t)vmax * 60 + (size_t)tmax * 24 + ((size_t)16 << 20), "%zu bytes at the limits", c.bytes);
        CHECK(c.bytes > ((size_t)1 << 37), "beyond 32 and 36 bits");
        CHECK(3 * (uint64_t)tmax <= UINT32_MAX, "3 T stays a uint32");
        CHECK(smooth_workspace_bytes(vmax, tmax) == c.bytes && smooth_workspace_bytes(vmax + 1, 0) == 0 && smooth_workspace_bytes(0, tmax + 1) == 0 &&
              smooth_workspace_bytes(-1, 0) == 0 && smooth_workspace_bytes(0, -1) == 0 && smooth_workspace_bytes(INT64_MAX, INT64_MAX) == 0, "the query");
        const SmoothCarve s = smooth_carve(0, 0);
        CHECK(s.lv.count == 0 && s.bytes == 256 && smooth_workspace_bytes(0, 0) == 256, "the smallest call: %zu", s.bytes);
        const SmoothCarve one = smooth_carve(1, 0);
        CHECK(one.lv.count == 2 && one.lv.m[0] == 1 && one.lv.m[1] == 1, "one vertex: two levels");
        const SmoothCarve t = smooth_carve(1024 * 1024 + 1, 3);
        CHECK(t.lv.count == 3 && t.lv.m[0] == 1025 && t.lv.m[1] == 2 && t.lv.m[2] == 1, "one beyond a tile of tiles");
        for (const SmoothCarve* k : {&c, &s, &one, &t}) {
            CHECK(k->q_off[1] % 256 == 0 && k->q_off[2] % 256 == 0 && k->cnt_off % 256 == 0 && k->cursor_off % 256 == 0 && k->start_off % 256 == 0 && k->corner_off % 256 == 0, "alignment");
            CHECK(k->cursor_off == k->cnt_off + smooth_align((size_t)k->n_vertices * 4) && k->start_off == k->cursor_off + smooth_align((size_t)k->n_vertices * 4), "one memset clears counts and cursors");
            size_t last = k->corner_off + (size_t)k->n_triangles * 24;
            for (int l = 0; l < k->lv.count; ++l) { CHECK(k->lv.off[l] >= last && k->lv.off[l] % 256 == 0, "level %d", l); last = k->lv.off[l] + (size_t)k->lv.m[l] * 4; }
            CHECK(k->bytes >= last, "the end");
        }
    }

    // ---------------------------------------------------------------- refusals
    const int32_t two[2] = {32768, -34734};
    struct Call {
        const void *v = dev, *t = dev, *ws = dev, *counts = dev, *out = dev, *status = dev;
        int64_t nv = 100, nt = 200; const float *o, *u; const int32_t* lam; int n_steps = 2; size_t bytes = 0;
        int build() const { return smooth_check_build(v, nv, t, nt, o, u, ws, bytes, counts); }
        int run() const { return smooth_check_run(v, nv, nt, o, u, lam, n_steps, ws, bytes, out, status); }
    };
    Call ok; ok.o = org; ok.u = uni; ok.lam = two; ok.bytes = smooth_workspace_bytes(100, 200);
    CHECK(ok.bytes > 0 && ok.build() == EONERF_OK && ok.run() == EONERF_OK, "plain calls");
    { Call e = ok; e.nv = 0; e.nt = 0; CHECK(e.build() == EONERF_OK && e.run() == EONERF_OK, "an empty mesh is a mesh"); }
    { Call e = ok; e.v = nullptr; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "null vertices"); }
    { Call e = ok; e.t = nullptr; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_OK, "null triangles: build only"); }
    { Call e = ok; e.o = nullptr; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "null origin"); }
    { Call e = ok; e.u = nullptr; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "null unit"); }
    { Call e = ok; e.ws = nullptr; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "null workspace"); }
    { Call e = ok; e.counts = nullptr; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_OK, "null counts: build only"); }
    { Call e = ok; e.out = nullptr; CHECK(e.run() == EONERF_E_ARG && e.build() == EONERF_OK, "null out_vertices"); }
    { Call e = ok; e.status = nullptr; CHECK(e.run() == EONERF_E_ARG, "null status"); }
    { Call e = ok; e.lam = nullptr; CHECK(e.run() == EONERF_E_ARG && e.build() == EONERF_OK, "null factors"); }
    { Call e = ok; e.nv = -1; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "negative vertices"); e = ok; e.nt = INT64_MIN; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "negative triangles"); }
    { Call e = ok; e.bytes = SIZE_MAX; e.nv = kSmoothMaxVertices + 1; CHECK(e.build() == EONERF_E_UNSUPPORTED && e.run() == EONERF_E_UNSUPPORTED, "one vertex beyond");
      e.nv = kSmoothMaxVertices; e.nt = kSmoothMaxTriangles; CHECK(e.build() == EONERF_OK && e.run() == EONERF_OK, "the largest mesh");
      e.nt = kSmoothMaxTriangles + 1; CHECK(e.build() == EONERF_E_UNSUPPORTED && e.run() == EONERF_E_UNSUPPORTED, "one triangle beyond");
      e.nt = INT64_MAX; CHECK(e.run() == EONERF_E_UNSUPPORTED, "far beyond"); }
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {0.25f, 0.25f, 0.5f};
        Call e = ok;
        bad[k] = inf_; e.o = bad; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "infinite origin %d", k);
        bad[k] = nan_; CHECK(e.build() == EONERF_E_ARG, "NaN origin %d", k);
        bad[k] = -3e38f; CHECK(e.build() == EONERF_OK, "any finite origin");
        e = ok; e.u = bad;
        bad[k] = nan_; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "NaN unit %d", k);
        bad[k] = inf_; CHECK(e.build() == EONERF_E_ARG, "infinite unit %d", k);
        bad[k] = 0.f; CHECK(e.run() == EONERF_E_ARG, "zero unit %d", k);
        bad[k] = -0.f; CHECK(e.build() == EONERF_E_ARG, "minus zero unit %d", k);
        bad[k] = -0.25f; CHECK(e.build() == EONERF_E_ARG, "negative unit %d", k);
        bad[k] = 1e-45f; CHECK(e.build() == EONERF_OK && e.run() == EONERF_OK, "the smallest unit");
    }
    { Call e = ok; e.n_steps = 0; CHECK(e.run() == EONERF_E_ARG && e.build() == EONERF_OK, "no step"); e.n_steps = -3; CHECK(e.run() == EONERF_E_ARG, "a negative number of steps");
      std::vector<int32_t> many(EONERF_SMOOTH_MAX_STEPS + 1, 7);
      e.lam = many.data(); e.n_steps = EONERF_SMOOTH_MAX_STEPS; CHECK(e.run() == EONERF_OK, "4096 steps");
      e.n_steps = EONERF_SMOOTH_MAX_STEPS + 1; CHECK(e.run() == EONERF_E_ARG, "4097 steps");
      many[4095] = 65537; e.n_steps = EONERF_SMOOTH_MAX_STEPS; CHECK(e.run() == EONERF_E_ARG, "the last factor above one");
      many[4095] = 65536; many[0] = -65536; CHECK(e.run() == EONERF_OK, "factors of one and minus one");
      many[17] = -65537; CHECK(e.run() == EONERF_E_ARG, "below minus one"); many[17] = INT32_MIN; CHECK(e.run() == EONERF_E_ARG, "INT32_MIN"); }
    { Call e = ok; e.bytes = ok.bytes - 1; CHECK(e.build() == EONERF_E_WORKSPACE && e.run() == EONERF_E_WORKSPACE, "a short workspace"); e.bytes = 0; CHECK(e.build() == EONERF_E_WORKSPACE, "none at all"); }
    // the order: each refusal with every later one also present
    { const float zero_unit[3] = {0.f, 1.f, 1.f}; const int32_t big[2] = {0, 70000};
      Call e = ok; e.out = nullptr; e.counts = nullptr; e.nv = -1; e.nt = INT64_MAX; e.u = zero_unit; e.n_steps = 0; e.lam = big; e.bytes = 0;
      CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "null first");
      e.out = dev; e.counts = dev; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "a negative count before the limits");
      e.nv = 100; CHECK(e.build() == EONERF_E_UNSUPPORTED && e.run() == EONERF_E_UNSUPPORTED, "the limits before the values");
      e.nt = 200; CHECK(e.build() == EONERF_E_ARG && e.run() == EONERF_E_ARG, "the values before the steps and the workspace");
      e.u = uni; CHECK(e.build() == EONERF_E_WORKSPACE && e.run() == EONERF_E_ARG, "the number of steps before the workspace");
      e.n_steps = 2; CHECK(e.run() == EONERF_E_ARG, "the factors before the workspace");
      e.lam = two; CHECK(e.run() == EONERF_E_WORKSPACE, "the workspace last");
      e.bytes = ok.bytes; CHECK(e.build() == EONERF_OK && e.run() == EONERF_OK, "and nothing left"); }

    // ---------------------------------------------------------------- rdiv
    {
        const int64_t a[14] = {-7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7}, want[14] = {-2, -1, -1, -1, -1, 0, 0, 0, 0, 1, 1, 1, 2, 2};
        for (int k = 0; k < 14; ++k) CHECK(smooth_rdiv(a[k], 4) == want[k], "rdiv(%lld, 4) = %lld", (long long)a[k], (long long)smooth_rdiv(a[k], 4));
        CHECK(smooth_rdiv(-3, 2) == -1 && smooth_rdiv(3, 2) == 2 && smooth_rdiv(-1, 2) == 0 && smooth_rdiv(1, 2) == 1 && smooth_rdiv(-5, 3) == -2 && smooth_rdiv(-4, 3) == -1, "halves go up");
        const int64_t top = ((int64_t)1 << 62) - 1;
        CHECK(smooth_rdiv(top, 2) == (int64_t)1 << 61 && smooth_rdiv(-top, 2) == -((int64_t)1 << 61) + 1, "|D| near 2^62 over 2");
        const int64_t n = (int64_t)3 << 30;                                   // the largest n: 2 * 3 * 2^29 corners
        CHECK(smooth_rdiv(top, n) == 1431655765 && smooth_rdiv(-top, n) == -1431655765, "|D| near 2^62 over the largest n: %lld", (long long)smooth_rdiv(top, n));
        CHECK(smooth_rdiv(n * lim, n) == lim && smooth_rdiv(-n * lim, n) == -lim && smooth_rdiv(n * lim - n / 2, n) == lim && smooth_rdiv(n * lim - n / 2 - 1, n) == lim - 1, "the largest mean");
        CHECK(smooth_rdiv(-32768, 65536) == 0 && smooth_rdiv(-32769, 65536) == -1 && smooth_rdiv(32767, 65536) == 0 && smooth_rdiv(32768, 65536) == 1, "the factor's 16 bits");
        // both sides of the 32-bit short cut give one function
        CHECK(smooth_rdiv((int64_t)INT32_MAX, 2) == ((int64_t)1 << 30) && smooth_rdiv((int64_t)INT32_MAX + 1, 2) == ((int64_t)1 << 30) && smooth_rdiv((int64_t)INT32_MIN, 2) == -((int64_t)1 << 30) &&
              smooth_rdiv((int64_t)INT32_MIN - 1, 2) == -((int64_t)1 << 30) && smooth_rdiv((int64_t)INT32_MIN, (int64_t)INT32_MAX) == -1 && smooth_rdiv(5, (int64_t)INT32_MAX + 1) == 0 &&
              smooth_rdiv((int64_t)INT32_MAX, (int64_t)INT32_MAX) == 1 && smooth_rdiv((int64_t)1 << 30, (int64_t)INT32_MAX) == 1 && smooth_rdiv(((int64_t)1 << 30) - 1, (int64_t)INT32_MAX) == 0, "at the edges of 32 bits");
    }
    // ---------------------------------------------------------------- the quantisation: ties to even, what is quantisable, the limit
    {
        const float o[3] = {0.f, 0.f, 0.f}, u1[3] = {1.f, 1.f, 1.f};
        const SmoothGrid g = smooth_grid(o, u1);
        const float q = 1.f / 65536.f;
        int32_t Q[3];
        const float a[3] = {0.5f * q, 1.5f * q, -2.5f * q};
        CHECK(smooth_quantise(g, a, Q) && Q[0] == 0 && Q[1] == 2 && Q[2] == -2, "x.5 quanta go to the even one: %d %d %d", Q[0], Q[1], Q[2]);
        const float b[3] = {8191.9995f, -8191.9995f, -0.f};
        CHECK(smooth_quantise(g, b, Q) && Q[0] == 536870880 && Q[1] == -536870880 && Q[2] == 0, "the last fp32 below 8192: %d", Q[0]);
        const float c[3] = {8192.f, 0.f, 0.f}, d[3] = {0.f, -8192.f, 0.f}, e[3] = {0.f, 0.f, 3.4e38f};
        CHECK(!smooth_quantise(g, c, Q) && Q[0] == 0 && !smooth_quantise(g, d, Q) && !smooth_quantise(g, e, Q), "|u| = 8192 and beyond are not quantisable");
        const float n1[3] = {nan_, 0.f, 0.f}, n2[3] = {0.f, inf_, 0.f}, n3[3] = {0.f, 0.f, -inf_};
        CHECK(!smooth_quantise(g, n1, Q) && !smooth_quantise(g, n2, Q) && !smooth_quantise(g, n3, Q), "vertices that are not finite are not quantisable");
        // an origin that makes u = 8192 - 2^-30: quantisable, and llrint gives 2^29, which the limit takes back to LIM
        const float o2[3] = {9.31322574615478515625e-10f, 0.f, 0.f};
        CHECK(smooth_quantise(smooth_grid(o2, u1), c, Q) && Q[0] == (int32_t)lim, "within 2^-17 of 8192: %d", Q[0]);
        const float o3[3] = {-9.31322574615478515625e-10f, 0.f, 0.f}, c2[3] = {-8192.f, 0.f, 0.f};
        CHECK(smooth_quantise(smooth_grid(o3, u1), c2, Q) && Q[0] == -(int32_t)lim, "and of -8192: %d", Q[0]);
        // a denormal unit: the quotient overflows or is huge -- not quantisable, no undefined conversion
        const float tiny[3] = {1e-45f, 1e-45f, 1e-45f}, f[3] = {3.4e38f, 1.f, -1.f};
        CHECK(!smooth_quantise(smooth_grid(o, tiny), f, Q), "the smallest unit");
        CHECK(smooth_dequantise(g, 0, 98304) == 1.5f && smooth_dequantise(smooth_grid(org, uni), 2, -65536) == -1.5f && smooth_dequantise(g, 1, (int32_t)lim) == 8192.f, "dequantise");
    }
    // ---------------------------------------------------------------- the step: the limit at both ends
    {
        bool clamped = false;
        CHECK(smooth_step(100, 2 * 300, 2, 32768, &clamped) == 200 && !clamped, "half way to the neighbours' mean");
        CHECK(smooth_step(100, 2 * 300, 2, 65536, &clamped) == 300 && smooth_step(100, 2 * 300, 2, 0, &clamped) == 100 && smooth_step(100, 2 * 300, 2, -65536, &clamped) == -100 && !clamped, "factors 1, 0, -1");
        CHECK(smooth_step(0, 3, 4, 65536, &clamped) == 1 && smooth_step(0, -3, 4, 65536, &clamped) == -1 && smooth_step(0, 2, 4, 65536, &clamped) == 1 && smooth_step(0, -2, 4, 65536, &clamped) == 0 && !clamped, "the mean rounds half up");
        CHECK(smooth_step(0, 2, 2, 32768, &clamped) == 1 && smooth_step(0, -2, 2, 32768, &clamped) == 0 && !clamped, "so does the factor");
        CHECK(smooth_step((int32_t)lim, -2 * lim, 2, -65536, &clamped) == (int32_t)lim && clamped, "limited at the top");
        clamped = false;
        CHECK(smooth_step(-(int32_t)lim, 2 * lim, 2, -65536, &clamped) == -(int32_t)lim && clamped, "and at the bottom");
        clamped = false;
        CHECK(smooth_step((int32_t)lim - 1, 2 * lim, 2, 65536, &clamped) == (int32_t)lim && !clamped && smooth_step(-(int32_t)lim, 2 * lim, 2, 65536, &clamped) == (int32_t)lim && !clamped, "reaching the limit is not exceeding it");
        const int64_t n = (int64_t)3 << 30;
        CHECK(smooth_step(-(int32_t)lim, n * lim, n, 65536, &clamped) == (int32_t)lim && !clamped, "the largest D: n (LIM - (-LIM)) < 2^62");
    }
    // ---------------------------------------------------------------- open, free, counts, live
    {
        int64_t B1 = 0; uint64_t B2 = 0;
        smooth_balance(5, 9, &B1, &B2); smooth_balance(9, 5, &B1, &B2);
        CHECK(B1 == 0 && B2 == 0, "a closed fan of two");
        smooth_balance(0xFFFFFFFFu, 0, &B1, &B2);
        CHECK(B1 == 0xFFFFFFFFll && B2 == 0xFFFFFFFE00000001ull, "the largest index squared stays inside 64 bits");
        smooth_balance(0, 0xFFFFFFFFu, &B1, &B2);
        CHECK(B1 == 0 && B2 == 0, "and comes back mod 2^64");
        CHECK(smooth_flags(true, 3, 0, 0, false, true) == (SMOOTH_FREE | SMOOTH_QUANTISABLE) && smooth_flags(true, 3, 1, 0, false, true) == (SMOOTH_QUANTISABLE | SMOOTH_OPEN) &&
              smooth_flags(true, 3, 0, 7, false, false) == (SMOOTH_FREE | SMOOTH_QUANTISABLE | SMOOTH_OPEN) && smooth_flags(true, 3, 0, 0, true, false) == SMOOTH_QUANTISABLE &&
              smooth_flags(true, 0, 0, 0, false, true) == SMOOTH_QUANTISABLE && smooth_flags(false, 0, 0, 0, false, true) == 0, "flags");
        CHECK(smooth_count_bits(SMOOTH_FREE | SMOOTH_QUANTISABLE, 3, false) == 1 && smooth_count_bits(SMOOTH_QUANTISABLE | SMOOTH_OPEN, 3, true) == 6 && smooth_count_bits(SMOOTH_QUANTISABLE, 0, true) == 8 &&
              smooth_count_bits(0, 0, true) == 16 && smooth_count_bits(SMOOTH_FREE | SMOOTH_QUANTISABLE | SMOOTH_OPEN, 1, false) == 3, "counts");
        const int fl[5] = {2, 2, 2, 0, 2};
        auto of = [&fl](int32_t v) { return fl[v]; };
        const int32_t keep[3] = {0, 2, 4}, same[3] = {4, 4, 4}, gone[3] = {0, 3, 2}, low[3] = {-1, 0, 2}, high[3] = {0, 2, 5}, top[3] = {INT32_MAX, 0, 2}, bottom[3] = {0, INT32_MIN, 2};
        CHECK(smooth_live(keep, 5, of) && smooth_live(same, 5, of) && !smooth_live(gone, 5, of) && !smooth_live(low, 5, of) && !smooth_live(high, 5, of) && !smooth_live(top, 5, of) &&
              !smooth_live(bottom, 5, of) && !smooth_live(keep, 4, of) && !smooth_live(keep, 0, of), "live and dead faces");
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int64_t n[2]; int32_t par[4]; float grid[6];
        bool good = fread(n, 8, 2, in) == 2 && fread(par, 4, 4, in) == 4 && fread(grid, 4, 6, in) == 6 && n[0] >= 0 && n[1] >= 0 && n[0] < (1 << 24) && n[1] < (1 << 24) &&
                    par[2] >= 1 && par[2] <= EONERF_SMOOTH_MAX_STEPS;
        std::vector<int32_t> steps(good ? (size_t)par[2] : 0);
        good = good && fread(steps.data(), 4, steps.size(), in) == steps.size();
        good = good && smooth_check_run(dev, n[0], n[1], grid, grid + 3, steps.data(), (int)steps.size(), dev, SIZE_MAX, dev, dev) == EONERF_OK;
        std::vector<float> v(good ? (size_t)n[0] * 3 : 0);
        std::vector<int32_t> t(good ? (size_t)n[1] * 3 : 0);
        std::vector<uint8_t> mask(good && par[1] ? (size_t)n[0] : 0);
        good = good && fread(v.data(), 4, v.size(), in) == v.size() && fread(t.data(), 4, t.size(), in) == t.size() && fread(mask.data(), 1, mask.size(), in) == mask.size();
        fclose(in);
        if (!good) { fprintf(stderr, "malformed mesh file\n"); return 2; }
        const Result r = run(smooth_grid(grid, grid + 3), v, t, par[1] ? mask.data() : nullptr, par[0] != 0, steps);
        FILE* out = fopen(argv[2], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        fwrite(r.counts, 8, 6, out);
        fwrite(&r.status, 4, 1, out);
        fwrite(r.vertices.data(), 4, r.vertices.size(), out);
        fclose(out);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("smooth checks ok\n");
    return 0;
}
