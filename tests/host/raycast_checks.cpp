// Host-only checks of eonerf_code_amd/csrc/eonerf_raycast.h (eonerf_raycast_check.h), built for the CPU under the address +
// undefined-behaviour sanitizers (tests/host/test_raycast_host.py): every refusal in its documented order, the 64-bit size arithmetic
// at the limits (2^27 cells, 2^31 - 1 entries, the strides), the padded cell range with negative and boundary coordinates, the stepper
// with zero direction components, and the GRID path itself -- the functions the kernels of eonerf_raycast.hip call per lane, run here
// in a loop.  No HIP runtime call is made and no device pointer is dereferenced.
//   raycast_checks             the checks
//   raycast_checks IN OUT      also casts the rays of IN (int64 V T N, int32 dims[3] has_skip, double lo[3] hi[3] t_min t_max,
//                              float vertices[V][3], int32 triangles[T][3], float origins[N][3], float dirs[N][3], int32 skip[N] if
//                              has_skip) through the grid and writes OUT (int64 entries dropped, int64 closest[3], int64 occluded[3],
//                              double t[N], int32 face[N], float bary[N][3], uint8 occluded[N])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_raycast_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers

struct Grid {
    RcGrid g;
    std::vector<uint32_t> start, list;                                       // start[cell] .. start[cell + 1]: the cell's list
    int64_t dropped = 0;
};

// count, scan and fill as the kernels do them, one triangle after the other
static Grid build(const RcGrid& g, const std::vector<float>& vertices, const std::vector<int32_t>& triangles) {
    const int64_t nv = (int64_t)vertices.size() / 3, nt = (int64_t)triangles.size() / 3;
    const size_t cells = (size_t)g.dims[0] * g.dims[1] * g.dims[2];
    Grid r;
    r.g = g;
    std::vector<uint32_t> cnt(cells, 0), cursor(cells, 0);
    for (int64_t t = 0; t < nt; ++t) {
        double v[3][3];
        int c0[3], c1[3];
        if (!rc_live(g, vertices.data(), nv, &triangles[(size_t)t * 3], v)) { ++r.dropped; continue; }
        rc_cell_range(g, v, c0, c1);
        for (int64_t k = 0; k < rc_range_cells(c0, c1); ++k) ++cnt.at(rc_range_cell(g, c0, c1, k));
    }
    r.start.assign(cells + 1, 0);
    for (size_t c = 0; c < cells; ++c) r.start[c + 1] = r.start[c] + cnt[c];
    r.list.assign(r.start[cells], 0);
    for (int64_t t = nt - 1; t >= 0; --t) {                                   // (backwards: the order inside a list may not matter)
        double v[3][3];
        int c0[3], c1[3];
        if (!rc_live(g, vertices.data(), nv, &triangles[(size_t)t * 3], v)) continue;
        rc_cell_range(g, v, c0, c1);
        for (int64_t k = 0; k < rc_range_cells(c0, c1); ++k) {
            const uint32_t c = rc_range_cell(g, c0, c1, k);
            r.list.at(r.start[c] + cursor[c]++) = (uint32_t)t;
        }
    }
    return r;
}

struct Cast { double t; int32_t face; float bary[3]; bool rejected, blocked; int steps; };

static Cast cast(const Grid& G, const std::vector<float>& vertices, const std::vector<int32_t>& triangles, const float* o, const float* d, double t_min,
                 double t_max, bool any_hit, bool has_skip, int32_t skip) {
    const int64_t nv = (int64_t)vertices.size() / 3;
    Cast out;
    out.t = NAN; out.face = -1; out.bary[0] = out.bary[1] = out.bary[2] = NAN; out.blocked = false; out.steps = 0;
    const RcRay r = rc_ray(o, d);
    out.rejected = !r.ok;
    if (!r.ok) return out;
    RcWalk w = rc_walk(G.g, r, t_min, t_max);
    if (!w.in) return out;
    RcHit best;
    best.t = best.U = best.V = best.W = best.det = 0.0;
    do {
        ++out.steps;
        const uint32_t cell = rc_walk_cell(G.g, w);
        for (uint32_t k = G.start.at(cell); k < G.start.at(cell + 1); ++k) {
            const int32_t f = (int32_t)G.list[k];
            double v[3][3];
            RcHit h;
            if (!rc_live(G.g, vertices.data(), nv, &triangles[(size_t)f * 3], v) || !rc_test(r, v, t_min, t_max, &h)) continue;
            if (any_hit) {
                if (!(has_skip && f == skip)) { out.blocked = true; return out; }
            } else if (rc_closer(h.t, f, best.t, out.face)) {
                best = h; out.face = f;
            }
        }
    } while (rc_walk_step(G.g, w, out.face >= 0, best.t));
    if (out.face >= 0) { out.t = best.t; rc_bary(best, out.bary); }
    return out;
}

int main(int argc, char** argv) {
    const double nan_ = NAN, inf_ = INFINITY;
    const double lo[3] = {-1.0, -2.0, 0.5}, hi[3] = {3.0, 1.0, 2.5};
    const int dims[3] = {4, 6, 2};

    // ---------------------------------------------------------------- sizes
    {
        const int big[3] = {512, 512, 512}, over[3] = {1024, 512, 257}, one[3] = {1, 1, 1}, wide[3] = {EONERF_RAYCAST_MAX_DIM, EONERF_RAYCAST_MAX_DIM, 8};
        const int zero[3] = {4, 0, 4}, neg[3] = {-1, 4, 4}, long_[3] = {EONERF_RAYCAST_MAX_DIM + 1, 1, 1}, third[3] = {128, 128, 65};
        CHECK(rc_cells(big) == kRcMaxCells && rc_cells(wide) == kRcMaxCells && rc_cells(over) == -2 && rc_cells(one) == 1 && rc_cells(zero) == -1 && rc_cells(neg) == -1 &&
              rc_cells(long_) == -1, "the cells of a grid");
        const RcCarve c = rc_carve((uint64_t)kRcMaxCells, (uint64_t)kRcMaxCount);
        CHECK(c.lv.count == 3 && c.lv.m[0] == 1u << 17 && c.lv.m[1] == 128 && c.lv.m[2] == 1, "levels at the limit: %d", c.lv.count);
        CHECK(c.start_off == 0 && c.cursor_off >= (size_t)kRcMaxCells * 4 && c.lv.off[0] >= c.cursor_off + (size_t)kRcMaxCells * 4, "per cell");
        CHECK(c.list_off >= c.lv.off[2] + 4 && c.bytes >= c.list_off + (size_t)kRcMaxCount * 4, "the lists: 4 bytes an entry");
        CHECK(c.bytes > ((size_t)1 << 33) && c.bytes < ((size_t)1 << 33) + ((size_t)1 << 30) + ((size_t)2 << 20), "%zu bytes at the limits: beyond 32 bits", c.bytes);
        CHECK(rc_workspace_bytes(big, kRcMaxCount, kRcMaxCount) == c.bytes && rc_workspace_bytes(big, kRcMaxCount, kRcMaxCount + 1) == 0 &&
              rc_workspace_bytes(big, kRcMaxCount + 1, 0) == 0 && rc_workspace_bytes(big, -1, 0) == 0 && rc_workspace_bytes(big, 0, -1) == 0 &&
              rc_workspace_bytes(over, 1, 1) == 0 && rc_workspace_bytes(zero, 1, 1) == 0 && rc_workspace_bytes(nullptr, 1, 1) == 0 &&
              rc_workspace_bytes(one, INT64_MAX, INT64_MAX) == 0, "the query");
        const RcCarve s = rc_carve(1, 0);
        CHECK(s.lv.count == 2 && s.lv.m[0] == 1 && s.lv.m[1] == 1 && s.bytes == 4 * 256 && rc_workspace_bytes(one, 0, 0) == s.bytes, "the smallest grid: %zu", s.bytes);
        const RcCarve t = rc_carve((uint64_t)rc_cells(third), 5);
        CHECK(t.lv.count == 3 && t.lv.m[0] == 1040 && t.lv.m[1] == 2 && t.lv.m[2] == 1, "one beyond a tile of tiles");
        const RcCarve e = rc_carve(1024 * 1024, 5);
        CHECK(e.lv.count == 2 && e.lv.m[0] == 1024 && e.lv.m[1] == 1, "exactly a tile of tiles");
        for (const RcCarve* k : {&c, &s, &t, &e}) {
            CHECK(k->cursor_off % 256 == 0 && k->list_off % 256 == 0 && k->cursor_off >= k->start_off + (size_t)k->cells * 4, "alignment");
            size_t last = k->cursor_off + (size_t)k->cells * 4;
            for (int l = 0; l < k->lv.count; ++l) { CHECK(k->lv.off[l] >= last && k->lv.off[l] % 256 == 0, "level %d", l); last = k->lv.off[l] + (size_t)k->lv.m[l] * 4; }
            CHECK(k->list_off >= last && k->bytes >= k->list_off + (size_t)k->entries * 4, "the end");
        }
    }

    // ---------------------------------------------------------------- refusals
    struct Call {
        const void *v = dev, *t = dev, *cc = dev, *counts = dev, *ws = dev, *o = dev, *d = dev;
        bool out_null = false;
        int64_t nv = 100, nt = 200, entries = 900; const double *lo, *hi; const int* dims; size_t bytes = 0;
        RcRays rays = {50, 3, 11, 0.0, INFINITY};
        int count() const { return rc_check_count(v, nv, t, nt, lo, hi, dims, cc, counts); }
        int build() const { return rc_check_build(v, nv, t, nt, lo, hi, dims, cc, entries, ws, bytes); }
        int cast() const { return rc_check_cast(v, nv, t, nt, lo, hi, dims, entries, ws, bytes, o, d, rays, out_null); }
        bool all(int rc) const { return count() == rc && build() == rc && cast() == rc; }
    };
    Call ok; ok.lo = lo; ok.hi = hi; ok.dims = dims; ok.bytes = rc_workspace_bytes(dims, 200, 900);
    CHECK(ok.bytes > 0 && ok.all(EONERF_OK), "plain calls");
    { Call e = ok; e.nv = 0; e.nt = 0; e.entries = 0; e.rays.n_rays = 0; CHECK(e.all(EONERF_OK), "an empty mesh is a mesh and no rays are rays"); }
    { Call e = ok; e.v = nullptr; CHECK(e.all(EONERF_E_ARG), "null vertices"); e = ok; e.t = nullptr; CHECK(e.all(EONERF_E_ARG), "null triangles"); }
    { Call e = ok; e.lo = nullptr; CHECK(e.all(EONERF_E_ARG), "null lo"); e = ok; e.hi = nullptr; CHECK(e.all(EONERF_E_ARG), "null hi"); e = ok; e.dims = nullptr; CHECK(e.all(EONERF_E_ARG), "null dims"); }
    { Call e = ok; e.cc = nullptr; CHECK(e.count() == EONERF_E_ARG && e.build() == EONERF_E_ARG && e.cast() == EONERF_OK, "null cell counts: count and build"); }
    { Call e = ok; e.counts = nullptr; CHECK(e.count() == EONERF_E_ARG && e.build() == EONERF_OK, "null counts"); }
    { Call e = ok; e.ws = nullptr; CHECK(e.count() == EONERF_OK && e.build() == EONERF_E_ARG && e.cast() == EONERF_E_ARG, "null workspace: build and casts"); }
    { Call e = ok; e.o = nullptr; CHECK(e.cast() == EONERF_E_ARG, "null origins"); e = ok; e.d = nullptr; CHECK(e.cast() == EONERF_E_ARG, "null dirs"); e = ok; e.out_null = true; CHECK(e.cast() == EONERF_E_ARG, "a null output"); }
    { Call e = ok; e.nv = -1; CHECK(e.all(EONERF_E_ARG), "negative vertices"); e = ok; e.nt = INT64_MIN; CHECK(e.all(EONERF_E_ARG), "negative triangles");
      e = ok; e.rays.n_rays = -1; CHECK(e.cast() == EONERF_E_ARG && e.build() == EONERF_OK, "negative rays"); }
    { Call e = ok; e.bytes = SIZE_MAX; e.nv = kRcMaxCount + 1; CHECK(e.all(EONERF_E_UNSUPPORTED), "one vertex beyond");
      e.nv = kRcMaxCount; e.nt = kRcMaxCount; e.rays.n_rays = kRcMaxCount; e.entries = kRcMaxCount; CHECK(e.all(EONERF_OK), "the largest call");
      e.nt = kRcMaxCount + 1; CHECK(e.all(EONERF_E_UNSUPPORTED), "one triangle beyond");
      e.nt = 5; e.rays.n_rays = kRcMaxCount + 1; CHECK(e.cast() == EONERF_E_UNSUPPORTED && e.build() == EONERF_OK, "one ray beyond");
      e.rays.n_rays = 5; e.entries = kRcMaxCount + 1; CHECK(e.cast() == EONERF_E_UNSUPPORTED && e.build() == EONERF_E_UNSUPPORTED && e.count() == EONERF_OK, "one entry beyond");
      e.entries = -1; CHECK(e.cast() == EONERF_E_ARG && e.build() == EONERF_E_ARG, "negative entries"); }
    for (int k = 0; k < 3; ++k) {
        double bad[3] = {lo[0], lo[1], lo[2]};
        Call e = ok; e.lo = bad;
        bad[k] = inf_; CHECK(e.all(EONERF_E_ARG), "infinite lo %d", k);
        bad[k] = -inf_; CHECK(e.all(EONERF_E_ARG), "minus infinite lo %d", k);
        bad[k] = nan_; CHECK(e.all(EONERF_E_ARG), "NaN lo %d", k);
        bad[k] = hi[k]; CHECK(e.all(EONERF_E_ARG), "lo == hi %d", k);
        bad[k] = hi[k] + 1; CHECK(e.all(EONERF_E_ARG), "lo > hi %d", k);
        bad[k] = nextafter(hi[k], -inf_); CHECK(e.all(EONERF_OK), "the thinnest box");
        double top[3] = {hi[0], hi[1], hi[2]};
        e = ok; e.hi = top;
        top[k] = nan_; CHECK(e.all(EONERF_E_ARG), "NaN hi %d", k);
        top[k] = inf_; CHECK(e.all(EONERF_E_ARG), "infinite hi %d", k);
        int dd[3] = {4, 6, 2};
        e = ok; e.dims = dd; e.bytes = SIZE_MAX;
        dd[k] = 0; CHECK(e.all(EONERF_E_ARG), "no cells %d", k);
        dd[k] = -7; CHECK(e.all(EONERF_E_ARG), "negative cells %d", k);
        dd[k] = EONERF_RAYCAST_MAX_DIM + 1; CHECK(e.all(EONERF_E_ARG), "too many cells on an axis %d", k);
        dd[k] = EONERF_RAYCAST_MAX_DIM; CHECK(e.all(EONERF_OK), "the longest axis %d", k);
    }
    { const int over[3] = {1024, 512, 257}; Call e = ok; e.dims = over; e.bytes = SIZE_MAX; CHECK(e.all(EONERF_E_UNSUPPORTED), "more than 2^27 cells"); }
    { Call e = ok;
      e.rays.origin_stride = 2; CHECK(e.cast() == EONERF_E_ARG, "an origin stride of 2"); e.rays.origin_stride = 0; CHECK(e.cast() == EONERF_E_ARG, "of 0");
      e.rays.origin_stride = -3; CHECK(e.cast() == EONERF_E_ARG, "negative"); e.rays.origin_stride = kRcMaxStride + 1; CHECK(e.cast() == EONERF_E_ARG, "beyond 2^24");
      e.rays.origin_stride = kRcMaxStride; CHECK(e.cast() == EONERF_OK, "the largest stride");
      e = ok; e.rays.dir_stride = 2; CHECK(e.cast() == EONERF_E_ARG, "a direction stride of 2"); e.rays.dir_stride = INT64_MAX; CHECK(e.cast() == EONERF_E_ARG, "INT64_MAX");
      // the address of the last ray: (2^31 - 2) * 2^24 floats stay far inside 64 bits
      CHECK((uint64_t)(kRcMaxCount - 1) * (uint64_t)kRcMaxStride * 4 < ((uint64_t)1 << 58), "the last ray's offset in bytes");
      e = ok; e.rays.t_min = nan_; CHECK(e.cast() == EONERF_E_ARG, "NaN t_min"); e = ok; e.rays.t_max = nan_; CHECK(e.cast() == EONERF_E_ARG, "NaN t_max");
      e = ok; e.rays.t_min = -1e-300; CHECK(e.cast() == EONERF_E_ARG, "negative t_min"); e = ok; e.rays.t_min = 2; e.rays.t_max = 1; CHECK(e.cast() == EONERF_E_ARG, "t_min > t_max");
      e = ok; e.rays.t_min = inf_; CHECK(e.cast() == EONERF_E_ARG, "infinite t_min"); e = ok; e.rays.t_min = e.rays.t_max = 1.5; CHECK(e.cast() == EONERF_OK, "t_min == t_max");
      e = ok; e.rays.t_min = -0.0; e.rays.t_max = 0.0; CHECK(e.cast() == EONERF_OK, "zero"); }
    { Call e = ok; e.bytes = ok.bytes - 1; CHECK(e.build() == EONERF_E_WORKSPACE && e.cast() == EONERF_E_WORKSPACE && e.count() == EONERF_OK, "a short workspace");
      e.bytes = 0; CHECK(e.build() == EONERF_E_WORKSPACE, "none at all"); }
    // the order: each refusal with every later one also present
    { const double flat[3] = {3.0, -2.0, 0.5}; const int none[3] = {0, 6, 2}, over[3] = {1024, 512, 257};
      Call e = ok; e.out_null = true; e.nv = -1; e.nt = INT64_MAX; e.lo = flat; e.dims = none; e.entries = -1; e.rays.origin_stride = 1; e.rays.t_min = nan_; e.bytes = 0;
      CHECK(e.cast() == EONERF_E_ARG, "null first");
      e.out_null = false; CHECK(e.cast() == EONERF_E_ARG && e.build() == EONERF_E_ARG, "a negative count before the limits");
      e.nv = 100; CHECK(e.all(EONERF_E_UNSUPPORTED), "the limits before the box");
      e.nt = 200; e.dims = over; CHECK(e.all(EONERF_E_ARG), "the box before the grid");
      e.lo = lo; CHECK(e.all(EONERF_E_UNSUPPORTED), "too many cells");
      e.dims = none; CHECK(e.all(EONERF_E_ARG), "a bad axis");
      e.dims = dims; CHECK(e.count() == EONERF_OK && e.build() == EONERF_E_ARG && e.cast() == EONERF_E_ARG, "the grid before the entries");
      e.entries = kRcMaxCount + 1; CHECK(e.build() == EONERF_E_UNSUPPORTED && e.cast() == EONERF_E_UNSUPPORTED, "the entries before the strides");
      e.entries = 900; CHECK(e.build() == EONERF_E_WORKSPACE && e.cast() == EONERF_E_ARG, "the strides before the range");
      e.rays.origin_stride = 3; CHECK(e.cast() == EONERF_E_ARG, "the range before the workspace");
      e.rays.t_min = 0; CHECK(e.cast() == EONERF_E_WORKSPACE, "the workspace last");
      e.bytes = ok.bytes; CHECK(e.all(EONERF_OK), "and nothing left"); }

    // ---------------------------------------------------------------- the padded cell range
    {
        const double l0[3] = {-4.0, 0.0, 0.0}, h0[3] = {4.0, 8.0, 2.0};
        const int d0[3] = {8, 8, 2};
        const RcGrid g = rc_grid(l0, h0, d0);
        CHECK(g.inv[0] == 1.0 && g.inv[2] == 1.0, "cells of one unit");
        int c0[3], c1[3];
        const double a[3][3] = {{-3.5, 0.5, 0.5}, {-3.25, 0.75, 0.5}, {-3.5, 0.75, 0.75}};
        rc_cell_range(g, a, c0, c1);
        CHECK(c0[0] == 0 && c1[0] == 0 && c0[1] == 0 && c1[1] == 0 && c0[2] == 0 && c1[2] == 0 && rc_range_cells(c0, c1) == 1, "inside one cell with negative coordinates");
        const double b[3][3] = {{-3.0, 1.0, 1.0}, {-3.0, 1.0, 1.0}, {-3.0, 1.0, 1.0}};
        rc_cell_range(g, b, c0, c1);
        CHECK(c0[0] == 0 && c1[0] == 1 && c0[1] == 0 && c1[1] == 1 && c0[2] == 0 && c1[2] == 1 && rc_range_cells(c0, c1) == 8, "a point on a lattice point: the eight cells around it");
        const double c[3][3] = {{-4.0, 0.0, 0.0}, {4.0, 8.0, 2.0}, {-4.0, 8.0, 0.0}};
        rc_cell_range(g, c, c0, c1);
        CHECK(c0[0] == 0 && c1[0] == 7 && c0[1] == 0 && c1[1] == 7 && c0[2] == 0 && c1[2] == 1 && rc_range_cells(c0, c1) == 128, "corner to corner: clamped to the grid at both ends");
        const double pad = kRcPad, e[3][3] = {{-3.0 + pad, 1.0 - pad, 0.5}, {-2.5, 0.5, 0.5}, {-2.5, 0.5, 0.5}};
        rc_cell_range(g, e, c0, c1);
        CHECK(c0[0] == 1 && c1[0] == 1 && c0[1] == 0 && c1[1] == 1, "exactly one pad from a boundary: below it stays out, above it the floor reaches the next cell");
        const double f[3][3] = {{-3.0 + pad / 2, 1.0 - pad / 2, 0.5}, {-2.5, 0.5, 0.5}, {-2.5, 0.5, 0.5}};
        rc_cell_range(g, f, c0, c1);
        CHECK(c0[0] == 0 && c1[0] == 1 && c0[1] == 0 && c1[1] == 1, "half a pad inside: both sides");
        CHECK(rc_range_cell(g, c0, c1, 0) == 0 && rc_range_cell(g, c0, c1, 1) == 1 && rc_range_cell(g, c0, c1, 2) == 8 && rc_range_cell(g, c0, c1, 3) == 9, "x fastest");
        CHECK(rc_cell_clamp(nan_, 8) == 0 && rc_cell_clamp(-inf_, 8) == 0 && rc_cell_clamp(inf_, 8) == 7 && rc_cell_clamp(-1.0, 8) == 0 && rc_cell_clamp(8.0, 8) == 7 && rc_cell_clamp(1e300, 1) == 0, "the clamp");
        const int dmax[3] = {EONERF_RAYCAST_MAX_DIM, EONERF_RAYCAST_MAX_DIM, EONERF_RAYCAST_MAX_DIM}, z0[3] = {0, 0, 0}, z1[3] = {dmax[0] - 1, dmax[1] - 1, dmax[2] - 1};
        CHECK(rc_range_cells(z0, z1) == (int64_t)1 << 36, "the largest range in 64 bits");
    }
    // ---------------------------------------------------------------- rays and the rule
    {
        const float o[3] = {0.f, 0.f, 0.f}, d1[3] = {1.f, -1.f, 1.f}, d2[3] = {0.5f, -2.f, 1.f}, d3[3] = {0.f, 0.f, -3.f}, zero[3] = {0.f, -0.f, 0.f};
        const float bad[3] = {0.f, NAN, 1.f}, far_[3] = {INFINITY, 0.f, 0.f};
        RcRay r = rc_ray(o, d1);
        CHECK(r.ok && r.kz == 0 && r.kx == 1 && r.ky == 2, "ties go to the smallest index");
        r = rc_ray(o, d2);
        CHECK(r.ok && r.kz == 1 && r.kx == 0 && r.ky == 2 && r.Sz == -0.5 && r.Sx == -0.25, "a negative largest component swaps the other two");
        r = rc_ray(o, d3);
        CHECK(r.ok && r.kz == 2 && r.kx == 1 && r.ky == 0 && r.Sx == 0.0 && r.Sy == 0.0, "straight down");
        CHECK(!rc_ray(o, zero).ok && !rc_ray(o, bad).ok && !rc_ray(bad, d1).ok && !rc_ray(far_, d1).ok && !rc_ray(o, far_).ok, "rejected rays");
        const double tri[3][3] = {{-1, -1, -2}, {1, -1, -2}, {0, 1, -2}}, flip[3][3] = {{-1, -1, -2}, {0, 1, -2}, {1, -1, -2}};
        RcHit h;
        CHECK(rc_test(r, tri, 0, inf_, &h) && fabs(h.t - 2.0 / 3.0) < 1e-15 && rc_test(r, flip, 0, inf_, &h) && fabs(h.t - 2.0 / 3.0) < 1e-15, "both orientations hit");
        CHECK(rc_test(r, tri, h.t, h.t, &h) && !rc_test(r, tri, 0, nextafter(h.t, 0), &h) && !rc_test(r, tri, nextafter(h.t, 1), inf_, &h), "both ends of the range are inclusive");
        const double edge[3][3] = {{0, -1, -2}, {0, 1, -2}, {-1, 0, -2}}, corner[3][3] = {{0, 0, -2}, {1, 0, -2}, {0, 1, -2}}, flat[3][3] = {{0, 0, -2}, {0, 0, -3}, {0, 0, -4}};
        CHECK(rc_test(r, edge, 0, inf_, &h) && rc_test(r, corner, 0, inf_, &h) && !rc_test(r, flat, 0, inf_, &h), "edges and corners are inside, zero area never hits");
        float bary[3];
        rc_test(r, tri, 0, inf_, &h); rc_bary(h, bary);
        CHECK(bary[0] == 0.25f && bary[1] == 0.25f && bary[2] == 0.5f, "weights of A, B, C: %g %g %g", bary[0], bary[1], bary[2]);
        CHECK(rc_closer(1.0, 5, 0.0, -1) && rc_closer(1.0, 5, 2.0, 3) && rc_closer(1.0, 2, 1.0, 3) && !rc_closer(1.0, 3, 1.0, 3) && !rc_closer(1.0, 4, 1.0, 3) && !rc_closer(nan_, 1, 1.0, 3), "(t, face) in order");
    }
    // ---------------------------------------------------------------- the stepper with zero direction components
    {
        const double l0[3] = {0, 0, 0}, h0[3] = {4, 4, 4};
        const int d0[3] = {4, 4, 4};
        const RcGrid g = rc_grid(l0, h0, d0);
        const float o[3] = {-2.f, 1.5f, 2.f}, dx[3] = {1.f, 0.f, 0.f};      // along +x, inside row 1, ON the cell face z = 2
        RcWalk w = rc_walk(g, rc_ray(o, dx), 0, inf_);
        CHECK(w.in && w.cell[0] == 0 && w.cell[1] == 1 && w.cell[2] == 2 && isinf(w.next[1]) && isinf(w.next[2]) && w.next[0] == 3.0, "enters at x = 0: %d %d %d", w.cell[0], w.cell[1], w.cell[2]);
        int steps = 1;
        while (rc_walk_step(g, w, false, 0)) { ++steps; CHECK(w.cell[1] == 1 && w.cell[2] == 2, "never leaves its row"); }
        CHECK(steps == 4 && w.cell[0] == 4, "four cells, then out of the grid: %d", steps);
        w = rc_walk(g, rc_ray(o, dx), 0, inf_);
        CHECK(rc_walk_step(g, w, true, 3.5) && !rc_walk_step(g, w, true, 3.5), "stops after the cell that holds the best hit");
        w = rc_walk(g, rc_ray(o, dx), 0, 3.5);
        CHECK(rc_walk_step(g, w, false, 0) && !rc_walk_step(g, w, false, 0), "stops at t_max");
        const float mx[3] = {-1.f, 0.f, 0.f}, in_[3] = {2.f, 2.f, 2.f}, out_[3] = {2.f, 5.f, 2.f}, on_[3] = {2.f, 4.f, 2.f}, dz[3] = {0.f, 0.f, -2.f};
        CHECK(!rc_walk(g, rc_ray(o, mx), 0, inf_).in && !rc_walk(g, rc_ray(out_, dx), 0, inf_).in && rc_walk(g, rc_ray(on_, dx), 0, inf_).in, "pointing away; beside the box; along its face");
        w = rc_walk(g, rc_ray(on_, dx), 0, inf_);
        CHECK(w.cell[1] == 3 && w.cell[0] == 2, "on the upper face: the last row");
        w = rc_walk(g, rc_ray(in_, dz), 0, inf_);                            // from a lattice point straight down
        CHECK(w.in && w.cell[0] == 2 && w.cell[1] == 2 && w.cell[2] == 2 && w.next[2] == 0.0, "starts on a boundary it is about to cross");
        steps = 1;
        while (rc_walk_step(g, w, false, 0)) ++steps;
        CHECK(steps == 3, "cells 2, 1, 0 below it: %d", steps);
        const float diag[3] = {1.f, 1.f, 1.f}, org[3] = {0.f, 0.f, 0.f};
        w = rc_walk(g, rc_ray(org, diag), 0, inf_);
        steps = 1;
        while (rc_walk_step(g, w, false, 0)) ++steps;
        CHECK(steps == 10 && w.left > 0, "the diagonal: three steps a lattice point, one axis at a time: %d", steps);
        w = rc_walk(g, rc_ray(org, diag), 0, inf_);
        w.next[0] = w.next[1] = w.next[2] = nan_;
        CHECK(!rc_walk_step(g, w, false, 0), "a NaN ends the walk");
        w = rc_walk(g, rc_ray(org, diag), 0, inf_);
        w.left = 1;
        CHECK(!rc_walk_step(g, w, false, 0), "and so does the bound");
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int64_t n[3]; int32_t par[4]; double box[8];
        bool good = fread(n, 8, 3, in) == 3 && fread(par, 4, 4, in) == 4 && fread(box, 8, 8, in) == 8 && n[0] >= 0 && n[1] >= 0 && n[2] >= 0 && n[0] < (1 << 24) &&
                    n[1] < (1 << 24) && n[2] < (1 << 24);
        const RcRays rays = {good ? n[2] : 0, 3, 3, box[6], box[7]};
        good = good && rc_check_cast(dev, n[0], dev, n[1], box, box + 3, par, 0, dev, SIZE_MAX, dev, dev, rays, false) == EONERF_OK && rc_cells(par) <= (1 << 22);
        std::vector<float> v(good ? (size_t)n[0] * 3 : 0), o(good ? (size_t)n[2] * 3 : 0), d(o.size());
        std::vector<int32_t> t(good ? (size_t)n[1] * 3 : 0), skip(good && par[3] ? (size_t)n[2] : 0);
        good = good && fread(v.data(), 4, v.size(), in) == v.size() && fread(t.data(), 4, t.size(), in) == t.size() && fread(o.data(), 4, o.size(), in) == o.size() &&
               fread(d.data(), 4, d.size(), in) == d.size() && fread(skip.data(), 4, skip.size(), in) == skip.size();
        fclose(in);
        if (!good) { fprintf(stderr, "malformed case file\n"); return 2; }
        const RcGrid g = rc_grid(box, box + 3, par);
        const Grid G = build(g, v, t);
        int64_t head[8] = {(int64_t)G.list.size(), G.dropped, n[2], 0, 0, n[2], 0, 0};
        std::vector<double> t_out((size_t)n[2]);
        std::vector<int32_t> face((size_t)n[2]);
        std::vector<float> bary((size_t)n[2] * 3);
        std::vector<uint8_t> occ((size_t)n[2]);
        const int bound = par[0] + par[1] + par[2] + 3;
        for (int64_t r = 0; r < n[2]; ++r) {
            const Cast c = cast(G, v, t, &o[(size_t)r * 3], &d[(size_t)r * 3], box[6], box[7], false, false, -1);
            const Cast a = cast(G, v, t, &o[(size_t)r * 3], &d[(size_t)r * 3], box[6], box[7], true, par[3] != 0, par[3] ? skip[(size_t)r] : -1);
            CHECK(c.steps <= bound && a.steps <= bound, "ray %lld: %d cell steps", (long long)r, c.steps);
            t_out[(size_t)r] = c.t; face[(size_t)r] = c.face; memcpy(&bary[(size_t)r * 3], c.bary, 12); occ[(size_t)r] = a.blocked ? 1 : 0;
            head[3] += c.rejected; head[4] += c.face >= 0; head[6] += a.rejected; head[7] += a.blocked;
        }
        FILE* out = fopen(argv[2], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        fwrite(head, 8, 8, out);
        fwrite(t_out.data(), 8, t_out.size(), out);
        fwrite(face.data(), 4, face.size(), out);
        fwrite(bary.data(), 4, bary.size(), out);
        fwrite(occ.data(), 1, occ.size(), out);
        fclose(out);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("raycast checks ok\n");
    return 0;
}
