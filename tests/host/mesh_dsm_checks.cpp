// Host-only checks of include/eonerf_mesh_dsm.h (eonerf_mesh_dsm_check.h), built for the CPU under the address + undefined-behaviour
// sanitizers (tests/host/test_mesh_dsm_host.py): every refusal in its documented order, the 64-bit arithmetic at the limits of the
// fixed-point range (coordinates at +-2^29 and one beyond), the floor-division box with negative coordinates, and the rule itself -- the
// functions the kernels of eonerf_mesh_dsm.hip call per lane, run here in a loop over the triangles and the cells of their boxes.
// No HIP runtime call is made and no device pointer is dereferenced.
//   mesh_dsm_checks             the checks
//   mesh_dsm_checks IN OUT      also rasterises the mesh in IN (int64 V T, int32 xsize ysize, double scale[3] offset[3] xoff yoff res,
//                               float vertices[V][3], int32 triangles[T][3]) and writes OUT (int64 counts[4], float dsm[ysize*xsize],
//                               int32 face[ysize*xsize])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_mesh_dsm_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers

struct Raster { std::vector<uint64_t> keys; std::vector<float> dsm; std::vector<int32_t> face; int64_t counts[4] = {0, 0, 0, 0}; };

// rasterize + resolve as the kernels do them, one triangle and one cell after the other
static Raster run(const MdsmGrid& g, const std::vector<float>& vertices, const std::vector<int32_t>& triangles) {
    const size_t n = (size_t)g.xsize * (size_t)g.ysize;
    Raster r;
    r.keys.assign(n, 0); r.dsm.resize(n); r.face.resize(n);
    const int64_t nv = (int64_t)vertices.size() / 3, nt = (int64_t)triangles.size() / 3;
    for (int64_t f = 0; f < nt; ++f) {
        const MdsmTri t = mdsm_setup(g, vertices.data(), nv, &triangles[(size_t)f * 3]);
        ++r.counts[t.state];
        if (mdsm_box_cells(t) == 0) continue;
        for (int j = t.j0; j <= t.j1; ++j)
            for (int i = t.i0; i <= t.i1; ++i) {
                const uint64_t key = mdsm_sample(t, (uint32_t)f, i, j);
                uint64_t& at = r.keys.at((size_t)j * g.xsize + i);
                if (key > at) at = key;
            }
    }
    for (size_t c = 0; c < n; ++c) {
        r.dsm[c] = r.keys[c] ? mdsm_key_altitude(r.keys[c]) : nanf("");
        r.face[c] = r.keys[c] ? mdsm_key_face(r.keys[c]) : -1;
        r.counts[3] += r.keys[c] != 0;
    }
    return r;
}

static MdsmGrid unit_grid(int xsize, int ysize) {
    MdsmGrid g;
    for (int c = 0; c < 3; ++c) { g.scale[c] = 1.0; g.offset[c] = 0.0; }
    g.xoff = 0.0; g.yoff = (double)ysize; g.res = 1.0; g.xsize = xsize; g.ysize = ysize;      // cell (j, i) covers east i .. i + 1, north ysize - j - 1 .. ysize - j
    return g;
}

int main(int argc, char** argv) {
    const double nan_ = nan(""), inf_ = INFINITY;
    const double sc[3] = {2.0, 2.0, 10.0}, of[3] = {500000.0, 4000000.0, 30.0};

    // ---------------------------------------------------------------- refusals
    struct Call {
        const void *v = dev, *t = dev, *keys = dev, *dsm = dev, *counts = dev, *face = dev, *attr = dev, *out = dev;
        int64_t nv = 100, nt = 200; const double *s, *o; double xoff = 499990.0, yoff = 4000020.0, res = 0.5; int xsize = 33, ysize = 17, channels = 3;
        int raster() const { return mdsm_check_rasterize(v, nv, t, nt, s, o, xoff, yoff, xsize, ysize, res, keys, dsm, counts); }
        int attrs() const { return mdsm_check_attributes(v, nv, t, nt, s, o, xoff, yoff, xsize, ysize, res, face, attr, channels, out); }
    };
    Call ok; ok.s = sc; ok.o = of;
    CHECK(ok.raster() == EONERF_OK && ok.attrs() == EONERF_OK, "plain calls");
    { Call e = ok; e.nt = 0; e.nv = 0; CHECK(e.raster() == EONERF_OK && e.attrs() == EONERF_OK, "an empty mesh is a mesh"); }
    { Call e = ok; e.v = nullptr; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "null vertices"); }
    { Call e = ok; e.t = nullptr; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "null triangles"); }
    { Call e = ok; e.s = nullptr; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "null scale"); }
    { Call e = ok; e.o = nullptr; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "null offset"); }
    { Call e = ok; e.keys = nullptr; CHECK(e.raster() == EONERF_E_ARG, "null keys"); }
    { Call e = ok; e.dsm = nullptr; CHECK(e.raster() == EONERF_E_ARG, "null dsm"); }
    { Call e = ok; e.counts = nullptr; CHECK(e.raster() == EONERF_E_ARG, "null counts"); }
    { Call e = ok; e.face = nullptr; CHECK(e.attrs() == EONERF_E_ARG && e.raster() == EONERF_OK, "null face: refused by attributes only"); }
    { Call e = ok; e.attr = nullptr; CHECK(e.attrs() == EONERF_E_ARG, "null attr"); }
    { Call e = ok; e.out = nullptr; CHECK(e.attrs() == EONERF_E_ARG, "null out"); }
    { Call e = ok; e.xsize = 0; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "xsize 0"); e = ok; e.ysize = -4; CHECK(e.raster() == EONERF_E_ARG, "ysize -4"); }
    { Call e = ok; e.nv = -1; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "negative vertices"); e = ok; e.nt = INT64_MIN; CHECK(e.raster() == EONERF_E_ARG, "negative triangles"); }
    { Call e = ok; e.channels = 0; CHECK(e.attrs() == EONERF_E_ARG && e.raster() == EONERF_OK, "channels 0"); e.channels = 9; CHECK(e.attrs() == EONERF_E_ARG, "channels 9");
      e.channels = 1; CHECK(e.attrs() == EONERF_OK, "channels 1"); e.channels = 8; CHECK(e.attrs() == EONERF_OK, "channels 8"); }
    { Call e = ok; e.xsize = 65536; e.ysize = 65536; CHECK(e.raster() == EONERF_OK, "the largest grid"); e.xsize = 65537; CHECK(e.raster() == EONERF_E_UNSUPPORTED, "one column beyond");
      e = ok; e.ysize = INT_MAX; CHECK(e.attrs() == EONERF_E_UNSUPPORTED, "rows beyond"); }
    { Call e = ok; e.nv = INT32_MAX; e.nt = INT32_MAX; CHECK(e.raster() == EONERF_OK, "the largest mesh"); e.nv = (int64_t)INT32_MAX + 1; CHECK(e.raster() == EONERF_E_UNSUPPORTED, "one vertex beyond");
      e = ok; e.nt = INT64_MAX; CHECK(e.attrs() == EONERF_E_UNSUPPORTED, "triangles beyond"); }
    { Call e = ok; e.res = 0.0; CHECK(e.raster() == EONERF_E_ARG, "res 0"); e.res = -0.5; CHECK(e.raster() == EONERF_E_ARG, "res < 0"); e.res = nan_; CHECK(e.raster() == EONERF_E_ARG, "res NaN");
      e.res = inf_; CHECK(e.attrs() == EONERF_E_ARG, "res inf"); }
    { Call e = ok; e.xoff = nan_; CHECK(e.raster() == EONERF_E_ARG, "xoff NaN"); e = ok; e.yoff = -inf_; CHECK(e.attrs() == EONERF_E_ARG, "yoff -inf"); }
    for (int k = 0; k < 3; ++k) {
        double bad[3] = {sc[0], sc[1], sc[2]};
        Call e = ok;
        bad[k] = inf_; e.o = bad; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "infinite offset %d", k);
        e = ok; bad[k] = nan_; e.s = bad; CHECK(e.raster() == EONERF_E_ARG, "NaN scale %d", k);
        bad[k] = 0.0; CHECK(e.raster() == EONERF_E_ARG, "zero scale %d", k);
        bad[k] = -0.0; CHECK(e.attrs() == EONERF_E_ARG, "minus zero scale %d", k);
        bad[k] = -3.0; CHECK(e.raster() == EONERF_OK, "a negative scale is a scale");
        e = ok; bad[k] = 0.0; e.o = bad; CHECK(e.raster() == EONERF_OK, "a zero offset is fine");
    }
    // the order: each refusal with every later one also present
    { const double zero_sc[3] = {0.0, 1.0, 1.0};
      Call e = ok; e.out = nullptr; e.keys = nullptr; e.xsize = 0; e.nv = -1; e.channels = 0; e.ysize = INT_MAX; e.res = nan_; e.s = zero_sc;
      CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "null first");
      e.out = dev; e.keys = dev; e.xsize = 70000; e.ysize = 0; e.nv = INT64_MAX; e.nt = -1;
      CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "an empty grid before the counts and the limits");
      e.ysize = 17; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "a negative count before the limits");
      e.nt = 5; CHECK(e.attrs() == EONERF_E_ARG && e.raster() == EONERF_E_UNSUPPORTED, "channels before the limits");
      e.channels = 3; CHECK(e.attrs() == EONERF_E_UNSUPPORTED, "the limits before the values");
      e.xsize = 33; e.nv = 100; CHECK(e.raster() == EONERF_E_ARG && e.attrs() == EONERF_E_ARG, "the values last");
      e.res = 0.5; CHECK(e.raster() == EONERF_E_ARG, "a zero scale");
      e.s = sc; CHECK(e.raster() == EONERF_OK && e.attrs() == EONERF_OK, "and nothing left"); }

    // ---------------------------------------------------------------- floor division and the box
    CHECK(mdsm_floor_div(0, 4096) == 0 && mdsm_floor_div(4095, 4096) == 0 && mdsm_floor_div(4096, 4096) == 1 && mdsm_floor_div(-1, 4096) == -1 &&
          mdsm_floor_div(-4096, 4096) == -1 && mdsm_floor_div(-4097, 4096) == -2 && mdsm_floor_div(-((int64_t)1 << 29) - 2048, 4096) == -131073, "floor, not truncation");
    {
        // east -2.75 .. 1.5, north 0.25 .. 3.0 on a 4 x 4 grid whose upper edge is north 4: columns -3 .. 1 clamp to 0 .. 1, rows 1 .. 3
        const MdsmGrid g = unit_grid(4, 4);
        const std::vector<float> v = {-2.75f, 0.25f, 1.f, 1.5f, 0.25f, 1.f, -2.75f, 3.0f, 1.f};
        const int32_t tri[3] = {0, 1, 2};
        const MdsmTri t = mdsm_setup(g, v.data(), 3, tri);
        CHECK(t.state == MDSM_KEEP && t.X[0] == -11264 && t.Y[0] == 15360 && t.X[1] == 6144 && t.Y[2] == 4096, "snap: %lld %lld", (long long)t.X[0], (long long)t.Y[0]);
        CHECK(t.i0 == 0 && t.i1 == 1 && t.j0 == 1 && t.j1 == 3, "box %d %d %d %d", t.i0, t.i1, t.j0, t.j1);
        // the same triangle far to the west: the box is empty, never negative
        const std::vector<float> far = {-12.75f, 0.25f, 1.f, -8.5f, 0.25f, 1.f, -12.75f, 3.0f, 1.f};
        const MdsmTri u = mdsm_setup(g, far.data(), 3, tri);
        CHECK(u.state == MDSM_KEEP && mdsm_box_cells(u) == 0 && u.i0 == 0 && u.i1 == -1, "a box wholly outside: %d %d", u.i0, u.i1);
        // a box between two centres: min X = 2049, max X = 6143 holds no centre
        const std::vector<float> thin = {2049.f / 4096.f, 0.5f, 0.f, 6143.f / 4096.f, 0.5f, 0.f, 1.f, 3.5f, 0.f};
        const MdsmTri w = mdsm_setup(g, thin.data(), 3, tri);
        CHECK(w.state == MDSM_KEEP && w.i0 == 1 && w.i1 == 0 && mdsm_box_cells(w) == 0, "no centre in 2049 .. 6143: %d %d", w.i0, w.i1);
        // centres exactly on min and max are inside
        const std::vector<float> on = {0.5f, 0.5f, 0.f, 2.5f, 0.5f, 0.f, 0.5f, 3.5f, 0.f};
        const MdsmTri x = mdsm_setup(g, on.data(), 3, tri);
        CHECK(x.i0 == 0 && x.i1 == 2 && x.j0 == 0 && x.j1 == 3, "inclusive box %d %d %d %d", x.i0, x.i1, x.j0, x.j1);
    }

    // ---------------------------------------------------------------- the limits of the fixed-point range
    {
        MdsmGrid g = unit_grid(65536, 65536);
        g.offset[1] = 1e6; g.yoff = 1e6 + 65536.0;                    // northings stay positive: Y = (65536 - v) * 4096
        const int64_t M = EONERF_MESH_DSM_MAX_COORD;
        const float lim = 131072.f;                                   // 2^29 sub-pixels = 2^17 cells
        const float beyond = 131072.015625f;                          // the next fp32: 2^29 + 64 sub-pixels
        const std::vector<float> v = {-lim, 65536.f + lim, -32767.99f,      // 0: X = -2^29, Y = -2^29
                                      lim, 65536.f + lim, 32767.99f,        // 1: X = +2^29, Y = -2^29
                                      -lim, 65536.f - lim, 0.f,             // 2: X = -2^29, Y = +2^29
                                      lim, 65536.f - lim, 1.f,              // 3: X = +2^29, Y = +2^29
                                      beyond, 0.f, 0.f,                     // 4: one step beyond in X
                                      0.f, 65536.f - beyond, 0.f,           // 5: one step beyond in Y
                                      0.f, 0.f, 32768.f, 0.f, 0.f, -32768.f,                     // 6, 7: the altitude bound itself
                                      (float)nan_, 0.f, 0.f, 0.f, (float)inf_, 0.f, 0.f, 0.f, (float)-inf_,      // 8, 9, 10
                                      3e38f, 3e38f, 0.f};                   // 11: far beyond every int64 once scaled
        const int64_t nv = (int64_t)v.size() / 3;
        const MdsmVertex a = mdsm_vertex(g, &v[0]), b = mdsm_vertex(g, &v[3]), c = mdsm_vertex(g, &v[6]), d = mdsm_vertex(g, &v[9]);
        CHECK(a.ok && b.ok && c.ok && d.ok && a.X == -M && a.Y == -M && b.X == M && b.Y == -M && c.X == -M && c.Y == M && d.X == M && d.Y == M,
              "the corners of the range: %lld %lld %lld %lld", (long long)a.X, (long long)a.Y, (long long)d.X, (long long)d.Y);
        for (int k = 4; k < nv; ++k) CHECK(!mdsm_vertex(g, &v[(size_t)k * 3]).ok, "vertex %d drops its triangles", k);
        for (int k = 4; k < nv; ++k) {
            const int32_t tri[3] = {0, 1, k};
            CHECK(mdsm_setup(g, v.data(), nv, tri).state == MDSM_DROPPED, "a triangle of vertex %d", k);
        }
        { const int32_t t1[3] = {0, 1, -1}, t2[3] = {0, (int32_t)nv, 1}, t3[3] = {INT32_MIN, 0, 1}, t4[3] = {0, 1, INT32_MAX};
          CHECK(mdsm_setup(g, v.data(), nv, t1).state == MDSM_DROPPED && mdsm_setup(g, v.data(), nv, t2).state == MDSM_DROPPED &&
                mdsm_setup(g, v.data(), nv, t3).state == MDSM_DROPPED && mdsm_setup(g, v.data(), nv, t4).state == MDSM_DROPPED, "indices outside the mesh"); }
        // the two halves of the whole range, in both orientations: every product is below 2^60, every edge function below 2^61
        const int32_t tris[4][3] = {{0, 1, 2}, {1, 3, 2}, {0, 2, 1}, {2, 3, 1}};
        for (int q = 0; q < 4; ++q) {
            const MdsmTri t = mdsm_setup(g, v.data(), nv, tris[q]);
            CHECK(t.state == MDSM_KEEP && t.area == (int64_t)1 << 60 && t.sign == (q < 2 ? 1 : -1) && t.i0 == 0 && t.i1 == 65535 && t.j0 == 0 && t.j1 == 65535 &&
                  mdsm_box_cells(t) == (int64_t)1 << 32, "half %d: area %lld sign %d", q, (long long)t.area, t.sign);
            const int cells[5][2] = {{0, 0}, {65535, 0}, {0, 65535}, {65535, 65535}, {32768, 32767}};
            for (const auto& ij : cells) {
                int64_t w[3];
                const bool in = mdsm_weights(t, ij[0], ij[1], w);
                CHECK(w[0] + w[1] + w[2] == t.area, "weights sum to the area at (%d, %d)", ij[0], ij[1]);
                const uint64_t key = mdsm_sample(t, 7u, ij[0], ij[1]);
                CHECK((key != 0) == in && (!in || mdsm_key_face(key) == 7), "key at (%d, %d)", ij[0], ij[1]);
                if (in) CHECK(fabs((double)mdsm_key_altitude(key)) < 32768.0, "altitude at (%d, %d)", ij[0], ij[1]);
            }
        }
        { const int32_t flat[3] = {0, 0, 1}, line[3] = {0, 3, 3};
          CHECK(mdsm_setup(g, v.data(), nv, flat).state == MDSM_DEGENERATE && mdsm_setup(g, v.data(), nv, line).state == MDSM_DEGENERATE, "zero area at the limits"); }
        // the key at the ends of the altitude range
        CHECK(mdsm_quantise(32767.99999999999) == 2147483647LL && mdsm_quantise(-32768.0) == -2147483648LL && mdsm_quantise(32768.0) == 2147483647LL &&
              mdsm_quantise(0.5 / 65536.0) == 0 && mdsm_quantise(1.5 / 65536.0) == 2 && mdsm_quantise(-0.5 / 65536.0) == 0 && mdsm_quantise(nan_) == -2147483648LL, "quantise: ties to even, clamped");
        CHECK(mdsm_key(-2147483648LL, (uint32_t)INT32_MAX) == 0x80000000ull && mdsm_key(2147483647LL, 0u) == UINT64_MAX, "the smallest and the largest key");
        CHECK(mdsm_key(5, 3u) > mdsm_key(5, 4u) && mdsm_key(6, 4u) > mdsm_key(5, 3u) && mdsm_key(-1, 0u) < mdsm_key(0, 9u), "higher first, then the smaller face");
        CHECK(mdsm_key_altitude(mdsm_key(-98304, 2u)) == -1.5f && mdsm_key_face(mdsm_key(-98304, 2u)) == 2, "a key back to its parts");
    }

    // ---------------------------------------------------------------- small rasters
    {
        // a 4 x 4 square of two triangles over a 6 x 6 grid at altitude 10 + east: centres on the outline are covered (inclusive edges),
        // the diagonal's cells are hit twice and keep the smaller face
        const MdsmGrid g = unit_grid(6, 6);
        const std::vector<float> v = {0.5f, 0.5f, 10.5f, 4.5f, 0.5f, 14.5f, 4.5f, 4.5f, 14.5f, 0.5f, 4.5f, 10.5f};
        const std::vector<int32_t> tris = {0, 1, 2, 0, 2, 3};
        const Raster r = run(g, v, tris);
        CHECK(r.counts[0] == 2 && r.counts[1] == 0 && r.counts[2] == 0 && r.counts[3] == 25, "counts %lld %lld %lld %lld", (long long)r.counts[0],
              (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3]);
        for (int j = 0; j < 6; ++j)
            for (int i = 0; i < 6; ++i) {
                const bool in = i <= 4 && j >= 1;                    // row j is north 5 - j + 0.5
                const float got = r.dsm[(size_t)j * 6 + i];
                CHECK(in ? got == 10.5f + (float)i : got != got, "cell (%d, %d) = %g", j, i, (double)got);
                CHECK(r.face[(size_t)j * 6 + i] == (!in ? -1 : (5 - j) > i ? 1 : 0), "face (%d, %d) = %d", j, i, r.face[(size_t)j * 6 + i]);
            }
        std::vector<int32_t> flipped = {0, 2, 1, 0, 3, 2};
        const Raster s = run(g, v, flipped);
        CHECK(s.keys == r.keys, "both orientations");
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int64_t n[2]; int32_t size[2]; double par[9];
        bool good = fread(n, 8, 2, in) == 2 && fread(size, 4, 2, in) == 2 && fread(par, 8, 9, in) == 9 && n[0] >= 0 && n[1] >= 0 && n[0] < (1 << 24) && n[1] < (1 << 24);
        MdsmGrid g;
        for (int c = 0; c < 3; ++c) { g.scale[c] = par[c]; g.offset[c] = par[3 + c]; }
        g.xoff = par[6]; g.yoff = par[7]; g.res = par[8]; g.xsize = size[0]; g.ysize = size[1];
        good = good && mdsm_check_rasterize(dev, n[0], dev, n[1], g.scale, g.offset, g.xoff, g.yoff, g.xsize, g.ysize, g.res, dev, dev, dev) == EONERF_OK &&
               g.xsize <= 4096 && g.ysize <= 4096;
        std::vector<float> v(good ? (size_t)n[0] * 3 : 0);
        std::vector<int32_t> t(good ? (size_t)n[1] * 3 : 0);
        good = good && fread(v.data(), 4, v.size(), in) == v.size() && fread(t.data(), 4, t.size(), in) == t.size();
        fclose(in);
        if (!good) { fprintf(stderr, "malformed mesh file\n"); return 2; }
        const Raster r = run(g, v, t);
        FILE* out = fopen(argv[2], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        fwrite(r.counts, 8, 4, out);
        fwrite(r.dsm.data(), 4, r.dsm.size(), out);
        fwrite(r.face.data(), 4, r.face.size(), out);
        fclose(out);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("mesh dsm checks ok\n");
    return 0;
}
