// Host-only checks of eonerf_code_amd/csrc/eonerf_simplify.h (eonerf_simplify_check.h), built for the CPU under the address +
// undefined-behaviour sanitizers (tests/host/test_simplify_host.py): every refusal in its documented order, the 64-bit size arithmetic
// at the limits (dims of 4096, 2^27 cells, 2^31 - 1 vertices and triangles), the clamp at both grid borders and ties-to-even at x.5
// sub-cells, and the rule itself -- the functions the kernels of eonerf_simplify.hip call per lane, run here in a loop.
// No HIP runtime call is made and no device pointer is dereferenced.
//   simplify_checks             the checks
//   simplify_checks IN OUT      also simplifies the mesh in IN (int64 V T, int32 dims[3] representative, float origin[3] cell[3],
//                               float vertices[V][3], int32 triangles[T][3]) and writes OUT (int64 counts[4], float vertices[V'][3],
//                               int32 source[V'], int32 vertex_map[V], int32 triangles[kept][3])
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_simplify_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const void* const dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);      // never dereferenced: stands for device pointers

struct Result { int64_t counts[4] = {0, 0, 0, 0}; std::vector<float> vertices; std::vector<int32_t> source, vertex_map, triangles; };

// count + emit as the kernels do them, one vertex, one cell and one triangle after the other
static Result run(const SimpGrid& g, int representative, const std::vector<float>& vertices, const std::vector<int32_t>& triangles) {
    const int64_t nv = (int64_t)vertices.size() / 3, nt = (int64_t)triangles.size() / 3;
    const size_t cells = (size_t)g.dims[0] * g.dims[1] * g.dims[2];
    std::vector<uint32_t> n(cells, 0), id(cells, 0);
    std::vector<uint64_t> sum(cells * 3, 0), key(cells, UINT64_MAX);
    std::vector<int32_t> vcell((size_t)nv, -1);
    Result r;
    for (int64_t v = 0; v < nv; ++v) {
        const SimpVertex q = simp_vertex(g, &vertices[(size_t)v * 3]);
        vcell[(size_t)v] = q.cell;
        if (q.cell < 0) continue;
        ++n.at((size_t)q.cell);
        for (int c = 0; c < 3; ++c) sum.at((size_t)q.cell * 3 + c) += (uint64_t)q.L[c];
    }
    for (size_t c = 0; c < cells; ++c) { id[c] = (uint32_t)r.counts[0]; r.counts[0] += n[c] != 0; }
    r.vertex_map.assign((size_t)nv, -1);
    for (int64_t v = 0; v < nv; ++v) {
        const int32_t cell = vcell[(size_t)v];
        if (cell < 0) continue;
        r.vertex_map[(size_t)v] = (int32_t)id[(size_t)cell];
        const SimpVertex q = simp_vertex(g, &vertices[(size_t)v * 3]);
        const uint64_t k = simp_key(q.L, &sum[(size_t)cell * 3], n[(size_t)cell], (uint32_t)v);
        if (k < key[(size_t)cell]) key[(size_t)cell] = k;
    }
    r.vertices.resize((size_t)r.counts[0] * 3);
    r.source.resize((size_t)r.counts[0]);
    for (size_t c = 0; c < cells; ++c) {
        if (!n[c]) continue;
        const uint32_t src = (uint32_t)(key[c] & 0xFFFFFFFFull);
        r.source.at(id[c]) = (int32_t)src;
        const int32_t q[3] = {(int32_t)(c % g.dims[0]), (int32_t)(c / g.dims[0] % g.dims[1]), (int32_t)(c / g.dims[0] / g.dims[1])};
        for (int k = 0; k < 3; ++k)
            r.vertices.at((size_t)id[c] * 3 + k) = representative == EONERF_SIMPLIFY_NEAREST ? vertices.at((size_t)src * 3 + k)
                                                                                             : simp_mean_position(g, k, q[k], sum[c * 3 + k], n[c]);
    }
    for (int64_t t = 0; t < nt; ++t) {
        int32_t c3[3];
        const int state = simp_classify(vcell.data(), nv, &triangles[(size_t)t * 3], c3);
        if (state == SIMP_DROPPED) ++r.counts[2];
        if (state == SIMP_COLLAPSED) ++r.counts[3];
        if (state != SIMP_KEEP) continue;
        ++r.counts[1];
        for (int k = 0; k < 3; ++k) r.triangles.push_back((int32_t)id.at((size_t)c3[k]));
    }
    return r;
}

int main(int argc, char** argv) {
    const float nan_ = nanf(""), inf_ = INFINITY;
    const float org[3] = {-1.f, -1.f, -1.f}, cel[3] = {0.25f, 0.25f, 0.5f};
    const int dm[3] = {8, 8, 4};

    // ---------------------------------------------------------------- sizes
    {
        const int one[3] = {1, 1, 1}, line[3] = {4096, 1, 1}, big[3] = {512, 512, 512}, over[3] = {1024, 512, 512}, wide[3] = {4097, 1, 1}, zero[3] = {8, 0, 8};
        const int neg[3] = {-1, -1, 1}, huge[3] = {4096, 4096, 4096};
        CHECK(simp_cells(one) == 1 && simp_cells(line) == 4096 && simp_cells(big) == (uint64_t)1 << 27, "cells inside the limits");
        CHECK(simp_cells(over) == 0 && simp_cells(wide) == 0 && simp_cells(zero) == 0 && simp_cells(neg) == 0 && simp_cells(huge) == 0 && simp_cells(nullptr) == 0, "cells outside");
        const SimpCarve c = simp_carve((uint64_t)1 << 27, INT32_MAX, INT32_MAX);
        CHECK(c.lc.count == 3 && c.lc.m[0] == 1u << 17 && c.lc.m[1] == 128 && c.lc.m[2] == 1, "cell levels at the limit: %d", c.lc.count);
        CHECK(c.lt.count == 4 && c.lt.m[0] == 1u << 21 && c.lt.m[1] == 2048 && c.lt.m[2] == 2 && c.lt.m[3] == 1, "triangle levels at the limit: %d", c.lt.count);
        CHECK(c.sum_off == ((size_t)1 << 29) && c.key_off >= c.sum_off + ((size_t)3 << 30) && c.cid_off >= c.key_off + ((size_t)1 << 30), "the cell table in 64 bits");
        CHECK(c.vcell_off >= c.cid_off + ((size_t)1 << 28) && c.tflag_off >= c.vcell_off + (size_t)INT32_MAX * 4 && c.lc.off[0] >= c.tflag_off + (size_t)INT32_MAX * 2, "per vertex and per triangle");
        CHECK(c.bytes > ((size_t)38 << 27) + (size_t)INT32_MAX * 6 && c.bytes < ((size_t)38 << 27) + (size_t)INT32_MAX * 6 + ((size_t)16 << 20), "%zu bytes at the limits", c.bytes);
        CHECK(simp_workspace_bytes(big, INT32_MAX, INT32_MAX) == c.bytes && simp_workspace_bytes(big, (int64_t)INT32_MAX + 1, 0) == 0 && simp_workspace_bytes(big, 0, -1) == 0 &&
              simp_workspace_bytes(over, 1, 1) == 0 && simp_workspace_bytes(nullptr, 1, 1) == 0, "the query");
        const SimpCarve s = simp_carve(1, 0, 0);
        CHECK(s.lc.count == 2 && s.lc.m[0] == 1 && s.lc.m[1] == 1 && s.lt.count == 0 && s.bytes > 0 && s.bytes <= 8 * 256, "the smallest call: %zu", s.bytes);
        const SimpCarve t = simp_carve(1025, 3, 1024 * 1024 + 1);
        CHECK(t.lc.count == 2 && t.lc.m[0] == 2 && t.lt.count == 3 && t.lt.m[0] == 1025 && t.lt.m[1] == 2 && t.lt.m[2] == 1, "one beyond a tile and beyond a tile of tiles");
        for (const SimpCarve* k : {&c, &s, &t}) {
            CHECK(k->sum_off % 8 == 0 && k->key_off % 256 == 0 && k->cid_off % 256 == 0 && k->vcell_off % 256 == 0 && k->tflag_off % 256 == 0, "alignment");
            size_t last = k->tflag_off + (size_t)k->n_triangles * 2;               // the end of what lies in front
            for (int l = 0; l < k->lc.count; ++l) { CHECK(k->lc.off[l] >= last && k->lc.off[l] % 256 == 0, "cell level %d", l); last = k->lc.off[l] + (size_t)k->lc.m[l] * 4; }
            for (int l = 0; l < k->lt.count; ++l) { CHECK(k->lt.off[l] >= last && k->lt.off[l] % 256 == 0, "triangle level %d", l); last = k->lt.off[l] + (size_t)k->lt.m[l] * 4; }
            CHECK(k->bytes >= last, "the end");
        }
    }

    // ---------------------------------------------------------------- refusals
    struct Call {
        const void *v = dev, *t = dev, *ws = dev, *counts = dev, *ov = dev, *ot = dev, *status = dev;
        int64_t nv = 100, nt = 200, cv = 50, ct = 60; const float *o, *c; const int* d; size_t bytes = 0; int rep = EONERF_SIMPLIFY_NEAREST;
        int count() const { return simp_check_count(v, nv, t, nt, o, c, d, ws, bytes, counts); }
        int emit() const { return simp_check_emit(v, nv, t, nt, o, c, d, rep, ws, bytes, ov, cv, ot, ct, status); }
    };
    Call ok; ok.o = org; ok.c = cel; ok.d = dm; ok.bytes = simp_workspace_bytes(dm, 100, 200);
    CHECK(ok.bytes > 0 && ok.count() == EONERF_OK && ok.emit() == EONERF_OK, "plain calls");
    { Call e = ok; e.nv = 0; e.nt = 0; e.cv = 0; e.ct = 0; CHECK(e.count() == EONERF_OK && e.emit() == EONERF_OK, "an empty mesh is a mesh"); }
    { Call e = ok; e.v = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null vertices"); }
    { Call e = ok; e.t = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null triangles"); }
    { Call e = ok; e.o = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null origin"); }
    { Call e = ok; e.c = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null cell"); }
    { Call e = ok; e.d = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null dims"); }
    { Call e = ok; e.ws = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null workspace"); }
    { Call e = ok; e.counts = nullptr; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_OK, "null counts: refused by count only"); }
    { Call e = ok; e.ov = nullptr; CHECK(e.emit() == EONERF_E_ARG && e.count() == EONERF_OK, "null out_vertices"); }
    { Call e = ok; e.ot = nullptr; CHECK(e.emit() == EONERF_E_ARG, "null out_triangles"); }
    { Call e = ok; e.status = nullptr; CHECK(e.emit() == EONERF_E_ARG, "null status"); }
    { Call e = ok; e.nv = -1; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "negative vertices"); e = ok; e.nt = INT64_MIN; CHECK(e.count() == EONERF_E_ARG, "negative triangles"); }
    { Call e = ok; e.cv = -1; CHECK(e.emit() == EONERF_E_ARG && e.count() == EONERF_OK, "a negative capacity"); e = ok; e.ct = -7; CHECK(e.emit() == EONERF_E_ARG, "the other one"); }
    { Call e = ok; e.nv = (int64_t)INT32_MAX + 1; CHECK(e.count() == EONERF_E_UNSUPPORTED && e.emit() == EONERF_E_UNSUPPORTED, "one vertex beyond"); e = ok; e.nt = INT64_MAX; CHECK(e.emit() == EONERF_E_UNSUPPORTED, "triangles beyond");
      e = ok; e.nv = INT32_MAX; e.nt = INT32_MAX; e.bytes = SIZE_MAX; CHECK(e.count() == EONERF_OK && e.emit() == EONERF_OK, "the largest mesh");
      e.cv = INT64_MAX; e.ct = INT64_MAX; CHECK(e.emit() == EONERF_OK, "any capacity"); }
    for (int k = 0; k < 3; ++k) {
        int bad[3] = {8, 8, 4};
        Call e = ok; e.d = bad; e.bytes = SIZE_MAX;
        bad[k] = 0; CHECK(e.count() == EONERF_E_UNSUPPORTED && e.emit() == EONERF_E_UNSUPPORTED, "dims[%d] = 0", k);
        bad[k] = -3; CHECK(e.count() == EONERF_E_UNSUPPORTED, "dims[%d] < 0", k);
        bad[k] = 4097; CHECK(e.emit() == EONERF_E_UNSUPPORTED, "dims[%d] = 4097", k);
        bad[k] = 4096; CHECK(e.count() == EONERF_OK, "dims[%d] = 4096", k);
        bad[0] = bad[1] = bad[2] = 512; CHECK(e.count() == EONERF_OK, "2^27 cells"); bad[k] = 513; CHECK(e.count() == EONERF_E_UNSUPPORTED, "more than 2^27 cells");
    }
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {0.25f, 0.25f, 0.5f};
        Call e = ok;
        bad[k] = inf_; e.o = bad; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "infinite origin %d", k);
        bad[k] = nan_; CHECK(e.count() == EONERF_E_ARG, "NaN origin %d", k);
        bad[k] = -3e38f; CHECK(e.count() == EONERF_OK, "any finite origin");
        e = ok; e.c = bad;
        bad[k] = nan_; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "NaN cell %d", k);
        bad[k] = inf_; CHECK(e.count() == EONERF_E_ARG, "infinite cell %d", k);
        bad[k] = 0.f; CHECK(e.count() == EONERF_E_ARG, "zero cell %d", k);
        bad[k] = -0.f; CHECK(e.emit() == EONERF_E_ARG, "minus zero cell %d", k);
        bad[k] = -0.25f; CHECK(e.count() == EONERF_E_ARG, "negative cell %d", k);
        bad[k] = 1e-45f; CHECK(e.count() == EONERF_OK, "the smallest cell");
    }
    { Call e = ok; e.bytes = ok.bytes - 1; CHECK(e.count() == EONERF_E_WORKSPACE && e.emit() == EONERF_E_WORKSPACE, "a short workspace"); e.bytes = 0; CHECK(e.count() == EONERF_E_WORKSPACE, "none at all"); }
    { Call e = ok; e.rep = 2; CHECK(e.emit() == EONERF_E_ARG && e.count() == EONERF_OK, "representative 2"); e.rep = -1; CHECK(e.emit() == EONERF_E_ARG, "representative -1");
      e.rep = EONERF_SIMPLIFY_MEAN; CHECK(e.emit() == EONERF_OK, "MEAN"); }
    // the order: each refusal with every later one also present
    { const float zero_cell[3] = {0.f, 1.f, 1.f}; const int wide[3] = {4097, 1, 1};
      Call e = ok; e.ot = nullptr; e.counts = nullptr; e.nv = -1; e.nt = INT64_MAX; e.d = wide; e.c = zero_cell; e.bytes = 0; e.rep = 9;
      CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "null first");
      e.ot = dev; e.counts = dev; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "a negative count before the limits");
      e.nv = 100; CHECK(e.count() == EONERF_E_UNSUPPORTED && e.emit() == EONERF_E_UNSUPPORTED, "too many triangles before the values");
      e.nt = 200; CHECK(e.count() == EONERF_E_UNSUPPORTED && e.emit() == EONERF_E_UNSUPPORTED, "dims before the values");
      e.d = dm; CHECK(e.count() == EONERF_E_ARG && e.emit() == EONERF_E_ARG, "the values before the workspace");
      e.c = cel; CHECK(e.count() == EONERF_E_WORKSPACE && e.emit() == EONERF_E_WORKSPACE, "the workspace before the representative");
      e.bytes = ok.bytes; CHECK(e.count() == EONERF_OK && e.emit() == EONERF_E_ARG, "the representative last");
      e.rep = 0; CHECK(e.emit() == EONERF_OK, "and nothing left"); }

    // ---------------------------------------------------------------- the quantisation: ties to even, the clamp at both borders
    {
        const float o[3] = {0.f, 0.f, 0.f}, c1[3] = {1.f, 1.f, 1.f};
        const int d[3] = {4, 2, 1};
        const SimpGrid g = simp_grid(o, c1, d);
        const float sub = 1.f / 16384.f;
        const float a[3] = {0.5f * sub, 1.5f * sub, 2.5f * sub};
        SimpVertex q = simp_vertex(g, a);
        CHECK(q.cell == 0 && q.L[0] == 0 && q.L[1] == 2 && q.L[2] == 2, "x.5 sub-cells go to the even one: %d %d %d", q.L[0], q.L[1], q.L[2]);
        const float b[3] = {-3.f, 7.f, -0.f};
        q = simp_vertex(g, b);
        CHECK(q.cell == 4 && q.q[0] == 0 && q.q[1] == 1 && q.L[0] == 0 && q.L[1] == 16383 && q.L[2] == 0, "below and above the grid: cell %d", q.cell);
        const float e[3] = {4.f, 2.f, 1.f};
        q = simp_vertex(g, e);
        CHECK(q.cell == 7 && q.L[0] == 16383 && q.L[1] == 16383 && q.L[2] == 16383, "the upper corner itself belongs to the last cell: %d", q.cell);
        const float f[3] = {3.99999f, 3.4e38f, -3.4e38f};
        q = simp_vertex(g, f);
        CHECK(q.cell == 7 && q.L[0] == 16383 && q.L[1] == 16383 && q.L[2] == 0, "far outside: %d", q.cell);
        const float below[3] = {-0.25f * sub, 1.f - 0.25f * sub, 0.5f};
        q = simp_vertex(g, below);
        CHECK(q.cell == 4 && q.L[0] == 0 && q.q[1] == 1 && q.L[1] == 0, "a quarter sub-cell below a cell's edge rounds into the cell above: %d %d", q.q[1], q.L[1]);
        const float n1[3] = {nan_, 0.f, 0.f}, n2[3] = {0.f, inf_, 0.f}, n3[3] = {0.f, 0.f, -inf_};
        CHECK(simp_vertex(g, n1).cell == -1 && simp_vertex(g, n2).cell == -1 && simp_vertex(g, n3).cell == -1, "vertices that are not finite are dropped");
        // the largest grid: the last sub-cell of cell 4095
        const int line[3] = {4096, 1, 1};
        const SimpGrid gl = simp_grid(o, c1, line);
        const float far[3] = {1e9f, 0.f, 0.f};
        q = simp_vertex(gl, far);
        CHECK(q.cell == 4095 && q.L[0] == 16383, "4096 cells in a row: %d", q.cell);
        // a denormal cell size: the quotient is finite in fp64 and clamps
        const float tiny[3] = {1e-45f, 1e-45f, 1e-45f};
        q = simp_vertex(simp_grid(o, tiny, d), f);
        CHECK(q.cell == 7, "the smallest cell size: %d", q.cell);
    }
    // ---------------------------------------------------------------- mean, key, position
    {
        CHECK(simp_mean(0, 1) == 0 && simp_mean(16383, 1) == 16383 && simp_mean(3, 2) == 2 && simp_mean(5, 2) == 3 && simp_mean(1, 3) == 0 && simp_mean(2, 3) == 1, "the rounded mean");
        CHECK(simp_mean((uint64_t)16383 * INT32_MAX, (uint32_t)INT32_MAX) == 16383, "every vertex of the largest mesh in one corner: below 2^45, exact");
        const int32_t L[3] = {16383, 0, 16383};
        const uint64_t S[3] = {0, 16383, 0};
        CHECK(simp_key(L, S, 1, 0xFFFFFFFFu) == ((((uint64_t)3 * 16383 * 16383) << 32) | 0xFFFFFFFFull), "the largest key");
        const int32_t L0[3] = {5, 6, 7};
        const uint64_t S0[3] = {10, 12, 14};
        CHECK(simp_key(L0, S0, 2, 9) == 9 && simp_key(L0, S0, 2, 3) < simp_key(L0, S0, 2, 4), "distance first, then the smaller id");
        const float o[3] = {-1.f, 2.f, 0.f}, c1[3] = {0.25f, 0.5f, 1.f};
        const int d[3] = {8, 8, 8};
        const SimpGrid g = simp_grid(o, c1, d);
        CHECK(simp_mean_position(g, 0, 3, 8192, 1) == -0.125f && simp_mean_position(g, 1, 7, 3 * 4096, 3) == 5.625f && simp_mean_position(g, 2, 0, 0, 5) == 0.f, "mean positions");
    }
    // ---------------------------------------------------------------- triangles
    {
        const int32_t vcell[5] = {3, 3, 7, -1, 9};
        int32_t c3[3];
        const int32_t keep[3] = {0, 2, 4}, flip[3] = {4, 2, 0}, coll[3] = {0, 1, 2}, coll2[3] = {2, 4, 2}, same[3] = {4, 4, 4}, gone[3] = {0, 3, 2}, low[3] = {-1, 0, 2}, high[3] = {0, 2, 5},
                      top[3] = {INT32_MAX, 0, 2}, bottom[3] = {0, INT32_MIN, 2};
        CHECK(simp_classify(vcell, 5, keep, c3) == SIMP_KEEP && c3[0] == 3 && c3[1] == 7 && c3[2] == 9 && simp_classify(vcell, 5, flip, c3) == SIMP_KEEP && c3[0] == 9, "kept, in place");
        CHECK(simp_classify(vcell, 5, coll, c3) == SIMP_COLLAPSED && simp_classify(vcell, 5, coll2, c3) == SIMP_COLLAPSED && simp_classify(vcell, 5, same, c3) == SIMP_COLLAPSED, "collapsed");
        CHECK(simp_classify(vcell, 5, gone, c3) == SIMP_DROPPED && simp_classify(vcell, 5, low, c3) == SIMP_DROPPED && simp_classify(vcell, 5, high, c3) == SIMP_DROPPED &&
              simp_classify(vcell, 5, top, c3) == SIMP_DROPPED && simp_classify(vcell, 5, bottom, c3) == SIMP_DROPPED, "dropped");
        CHECK(simp_classify(vcell, 4, keep, c3) == SIMP_DROPPED && simp_classify(nullptr, 0, keep, c3) == SIMP_DROPPED, "an index at n_vertices; no vertices at all");
    }

    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        int64_t n[2]; int32_t par[4]; float grid[6];
        bool good = fread(n, 8, 2, in) == 2 && fread(par, 4, 4, in) == 4 && fread(grid, 4, 6, in) == 6 && n[0] >= 0 && n[1] >= 0 && n[0] < (1 << 24) && n[1] < (1 << 24);
        good = good && simp_check_emit(dev, n[0], dev, n[1], grid, grid + 3, par, par[3], dev, SIZE_MAX, dev, 0, dev, 0, dev) == EONERF_OK && simp_cells(par) <= (1u << 24);
        std::vector<float> v(good ? (size_t)n[0] * 3 : 0);
        std::vector<int32_t> t(good ? (size_t)n[1] * 3 : 0);
        good = good && fread(v.data(), 4, v.size(), in) == v.size() && fread(t.data(), 4, t.size(), in) == t.size();
        fclose(in);
        if (!good) { fprintf(stderr, "malformed mesh file\n"); return 2; }
        const Result r = run(simp_grid(grid, grid + 3, par), par[3], v, t);
        FILE* out = fopen(argv[2], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        fwrite(r.counts, 8, 4, out);
        fwrite(r.vertices.data(), 4, r.vertices.size(), out);
        fwrite(r.source.data(), 4, r.source.size(), out);
        fwrite(r.vertex_map.data(), 4, r.vertex_map.size(), out);
        fwrite(r.triangles.data(), 4, r.triangles.size(), out);
        fclose(out);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("simplify checks ok\n");
    return 0;
}
