// Host-only checks of the texture entry points' refusals, layout and size arithmetic (eonerf_texture_check.h), built for the CPU under the
// address + undefined-behaviour sanitizers (tests/host/test_texture_host.py).  The checks are the functions the entry points of
// eonerf_texture.hip call before they launch anything, and texture_texel / texture_corner are the very functions its kernels call.  No HIP
// runtime call is made and no pointer is dereferenced except the host arrays (scale, offset).
// argv[1]: a file the numpy restatement wrote -- blocks of int64 {F, T, n}, then n records of {int64 face, double b[3]} for the texels
// 0 .. n - 1, then 3 F records of double {u, v} for the corners; every value must be reproduced bit for bit.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../eonerf_code_amd/csrc/eonerf_texture_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (isnan(a) && isnan(b)); }

static int layout_rc(int64_t F, int T, int64_t* w, int64_t* h, int64_t* cpr) {
    TextureLayout l;
    const int rc = texture_layout(F, T, &l);
    if (rc == EONERF_OK) { *w = l.atlas_w; *h = l.atlas_h; *cpr = l.cells_per_row; }
    return rc;
}

int main(int argc, char** argv) {
    // never dereferenced: stands for a device pointer
    const void* dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);
    const float nanf_ = nanf(""), inff_ = INFINITY;
    int64_t w = -1, h = -1, cpr = -1;
    TextureLayout l;

    // ---------------------------------------------------------------- layout
    CHECK(layout_rc(0, 4, &w, &h, &cpr) == EONERF_OK && w == 0 && h == 0 && cpr == 0, "F = 0: %lld %lld %lld", (long long)w, (long long)h, (long long)cpr);
    CHECK(layout_rc(1, 1, &w, &h, &cpr) == EONERF_OK && w == 6 && h == 6 && cpr == 1, "F = 1");
    CHECK(layout_rc(2, 4, &w, &h, &cpr) == EONERF_OK && w == 9 && h == 9 && cpr == 1, "F = 2");
    CHECK(layout_rc(3, 4, &w, &h, &cpr) == EONERF_OK && w == 18 && h == 9 && cpr == 2, "F = 3: a second cell");
    CHECK(layout_rc(19, 3, &w, &h, &cpr) == EONERF_OK && w == 32 && h == 24 && cpr == 4, "F = 2 * 3^2 + 1: a new row");
    CHECK(layout_rc(200000, 4, &w, &h, &cpr) == EONERF_OK && w == 317 * 9 && h == 316 * 9 && cpr == 317, "200 k faces");
    CHECK(layout_rc((int64_t)2 * 3276 * 3276, 5, &w, &h, &cpr) == EONERF_OK && w == 32760 && h == 32760, "just inside 32768");
    CHECK(layout_rc((int64_t)2 * 4096 * 4096, 3, &w, &h, &cpr) == EONERF_OK && w == 32768 && h == 32768, "32768 itself: 2^30 texels");
    CHECK(layout_rc((int64_t)2 * 4096 * 4096 + 1, 3, &w, &h, &cpr) == EONERF_E_UNSUPPORTED, "one face past the 32768 limit");
    CHECK(layout_rc((int64_t)2 * 3276 * 3276 + 1, 5, &w, &h, &cpr) == EONERF_E_UNSUPPORTED, "one face past 32760");
    CHECK(layout_rc(0x7fffffff, 1, &w, &h, &cpr) == EONERF_E_UNSUPPORTED, "F = 2^31 - 1");
    CHECK(layout_rc(INT64_MAX, 64, &w, &h, &cpr) == EONERF_E_UNSUPPORTED, "F = 2^63 - 1: nothing wraps");
    CHECK(layout_rc(-1, 4, &w, &h, &cpr) == EONERF_E_ARG && layout_rc(1, 0, &w, &h, &cpr) == EONERF_E_ARG && layout_rc(1, 65, &w, &h, &cpr) == EONERF_E_ARG, "arguments");
    CHECK(texture_layout(1, 1, nullptr) == EONERF_E_ARG, "null out");
    CHECK(texture_ceil_sqrt(0) == 0 && texture_ceil_sqrt(1) == 1 && texture_ceil_sqrt(2) == 2 && texture_ceil_sqrt(4) == 2 && texture_ceil_sqrt(5) == 3, "small roots");
    for (int64_t r : {(int64_t)3, (int64_t)94906266, (int64_t)2147483647, (int64_t)2147483648}) {       // around 2^53 and 2^62 the floating root is off
        CHECK(texture_ceil_sqrt(r * r) == r && texture_ceil_sqrt(r * r - 1) == r && texture_ceil_sqrt(r * r + 1) == r + 1, "root of %lld^2", (long long)r);
    }

    // ---------------------------------------------------------------- uv
    CHECK(texture_check_uv(3, 4, dev, &l) == EONERF_OK && texture_check_uv(0, 4, dev, &l) == EONERF_OK, "plain calls");
    CHECK(texture_check_uv(3, 4, nullptr, &l) == EONERF_E_ARG, "null output");
    CHECK(texture_check_uv(-1, 4, dev, &l) == EONERF_E_ARG && texture_check_uv(3, 0, dev, &l) == EONERF_E_ARG && texture_check_uv(3, 65, dev, &l) == EONERF_E_ARG, "arguments");
    CHECK(texture_check_uv(0x7fffffff, 1, dev, &l) == EONERF_E_UNSUPPORTED, "too many faces");
    CHECK(texture_check_uv(0x7fffffff, 1, nullptr, &l) == EONERF_E_ARG, "the null pointer is tested first");

    // ---------------------------------------------------------------- samples
    float sc[3] = {300.f, 300.f, 60.f}, off[3] = {436000.f, 3355000.f, 20.f};
    auto samples = [&](const void* v, int64_t nv, const void* t, int64_t F, int T, int64_t first, int64_t n, const float* s, const float* o, int zone,
                       const void* out) { return texture_check_samples(v, nv, t, F, T, first, n, s, o, zone, out, nullptr, nullptr, nullptr, nullptr, &l); };
    CHECK(samples(dev, 11, dev, 9, 5, 0, 600, sc, off, 17, dev) == EONERF_OK, "a plain call");
    CHECK(samples(dev, 11, dev, 9, 5, 300, 300, sc, off, 1, dev) == EONERF_OK && samples(dev, 11, dev, 9, 5, 600, 0, sc, off, 60, dev) == EONERF_OK, "ranges that end at the atlas' end");
    CHECK(samples(dev, 0, dev, 0, 5, 0, 0, sc, off, 17, dev) == EONERF_OK, "an empty mesh");
    CHECK(texture_check_samples(dev, 11, dev, 9, 5, 0, 600, sc, off, 17, nullptr, nullptr, nullptr, nullptr, dev, &l) == EONERF_OK, "any one output");
    CHECK(samples(nullptr, 11, dev, 9, 5, 0, 600, sc, off, 17, dev) == EONERF_E_ARG, "null vertices");
    CHECK(samples(dev, 11, nullptr, 9, 5, 0, 600, sc, off, 17, dev) == EONERF_E_ARG, "null triangles");
    CHECK(samples(dev, 11, dev, 9, 5, 0, 600, nullptr, off, 17, dev) == EONERF_E_ARG, "null scale");
    CHECK(samples(dev, 11, dev, 9, 5, 0, 600, sc, nullptr, 17, dev) == EONERF_E_ARG, "null offset");
    CHECK(samples(dev, 11, dev, 9, 5, 0, 600, sc, off, 17, nullptr) == EONERF_E_ARG, "no output");
    CHECK(samples(dev, -1, dev, 9, 5, 0, 600, sc, off, 17, dev) == EONERF_E_ARG && samples(dev, 11, dev, -1, 5, 0, 600, sc, off, 17, dev) == EONERF_E_ARG, "negative counts");
    CHECK(samples(dev, 11, dev, 9, 5, -1, 600, sc, off, 17, dev) == EONERF_E_ARG && samples(dev, 11, dev, 9, 5, 0, -1, sc, off, 17, dev) == EONERF_E_ARG, "a negative range");
    CHECK(samples(dev, 11, dev, 9, 0, 0, 600, sc, off, 17, dev) == EONERF_E_ARG && samples(dev, 11, dev, 9, 65, 0, 600, sc, off, 17, dev) == EONERF_E_ARG, "texels");
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {sc[0], sc[1], sc[2]};
        bad[k] = nanf_;
        CHECK(samples(dev, 11, dev, 9, 5, 0, 600, bad, off, 17, dev) == EONERF_E_ARG, "NaN scale %d", k);
        bad[k] = inff_;
        CHECK(samples(dev, 11, dev, 9, 5, 0, 600, sc, bad, 17, dev) == EONERF_E_ARG, "infinite offset %d", k);
    }
    CHECK(samples(dev, 11, dev, 9, 5, 0, 600, sc, off, 0, dev) == EONERF_E_ARG && samples(dev, 11, dev, 9, 5, 0, 600, sc, off, 61, dev) == EONERF_E_ARG, "zones 0 and 61");
    CHECK(samples(dev, (int64_t)1 << 31, dev, 9, 5, 0, 600, sc, off, 17, dev) == EONERF_E_UNSUPPORTED && samples(dev, 0x7fffffff, dev, 9, 5, 0, 600, sc, off, 17, dev) == EONERF_OK, "2^31 vertices");
    CHECK(samples(dev, 11, dev, 0x7fffffff, 1, 0, 600, sc, off, 17, dev) == EONERF_E_UNSUPPORTED, "too many faces");
    CHECK(samples(dev, 11, dev, 9, 5, 0, 601, sc, off, 17, dev) == EONERF_E_ARG && samples(dev, 11, dev, 9, 5, 600, 1, sc, off, 17, dev) == EONERF_E_ARG, "a range past the atlas");
    CHECK(samples(dev, 11, dev, 9, 5, 601, 0, sc, off, 17, dev) == EONERF_E_ARG, "a start past the atlas");
    CHECK(samples(dev, 11, dev, 9, 5, INT64_MAX, INT64_MAX, sc, off, 17, dev) == EONERF_E_ARG && samples(dev, 11, dev, 9, 5, 1, INT64_MAX, sc, off, 17, dev) == EONERF_E_ARG, "first + n never wraps");
    // the order: a bad argument is reported before a limit, a limit before the range
    CHECK(samples(dev, (int64_t)1 << 31, dev, 9, 5, 0, 600, sc, off, 0, dev) == EONERF_E_ARG, "zone before the vertex limit");
    CHECK(samples(dev, (int64_t)1 << 31, dev, 9, 5, 0, 601, sc, off, 17, dev) == EONERF_E_UNSUPPORTED, "the vertex limit before the range");

    // ---------------------------------------------------------------- bake
    auto bake = [&](const void* lla, const void* nrm, int64_t n, const void* rpcs, const void* addr, const void* shp, int K, int C, const void* g,
                    const void* b, const void* sat, float mc, int aw, int mode, const void* out) {
        return texture_check_bake(lla, nrm, n, rpcs, addr, shp, K, C, g, b, sat, mc, aw, mode, out, nullptr, nullptr, nullptr);
    };
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, EONERF_TEXTURE_MEDIAN, dev) == EONERF_OK, "a plain call");
    CHECK(bake(dev, nullptr, 600, dev, dev, dev, 3, 4, dev, dev, nullptr, 0.1f, 0, EONERF_TEXTURE_BEST, dev) == EONERF_OK, "no normal needs no view table");
    CHECK(bake(dev, dev, 0, dev, dev, dev, 1, 1, dev, dev, dev, -1.f, 0, EONERF_TEXTURE_MEAN, dev) == EONERF_OK, "n == 0");
    CHECK(texture_check_bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, 0, nullptr, nullptr, nullptr, dev) == EONERF_OK, "any one output");
    CHECK(bake(nullptr, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "null points");
    CHECK(bake(dev, dev, 600, nullptr, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "null rpcs");
    CHECK(bake(dev, dev, 600, dev, nullptr, dev, 3, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "null addresses");
    CHECK(bake(dev, dev, 600, dev, dev, nullptr, 3, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "null shapes");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, nullptr, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "null gain");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, nullptr, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "null bias");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, nullptr, 0.1f, 1, 0, dev) == EONERF_E_ARG, "a normal without a view table");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, 0, nullptr) == EONERF_E_ARG, "no output");
    CHECK(bake(dev, dev, -1, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "n < 0");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 0, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "K == 0");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 0, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG && bake(dev, dev, 600, dev, dev, dev, 3, 5, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_ARG, "channels");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, -1, dev) == EONERF_E_ARG && bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 1, 3, dev) == EONERF_E_ARG, "mode");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, 2, 0, dev) == EONERF_E_ARG && bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, 0.1f, -1, 0, dev) == EONERF_E_ARG, "angle_weight");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, nanf_, 1, 0, dev) == EONERF_E_ARG && bake(dev, dev, 600, dev, dev, dev, 3, 4, dev, dev, dev, inff_, 1, 0, dev) == EONERF_E_ARG, "min_cos");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 64, 3, dev, dev, dev, 0.1f, 1, EONERF_TEXTURE_MEDIAN, dev) == EONERF_OK, "K = 64 median");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 65, 3, dev, dev, dev, 0.1f, 1, EONERF_TEXTURE_MEDIAN, dev) == EONERF_E_UNSUPPORTED, "K = 65 median");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 65, 3, dev, dev, dev, 0.1f, 1, EONERF_TEXTURE_MEAN, dev) == EONERF_OK && bake(dev, dev, 600, dev, dev, dev, INT_MAX, 3, dev, dev, dev, 0.1f, 1, EONERF_TEXTURE_BEST, dev) == EONERF_OK, "the mean and the best take any K");
    CHECK(bake(dev, dev, 600, dev, dev, dev, 65, 3, dev, dev, dev, 0.1f, 1, 3, dev) == EONERF_E_ARG, "a bad mode before the K limit");
    CHECK(bake(dev, dev, INT64_MAX, dev, dev, dev, INT_MAX, 4, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_UNSUPPORTED, "K * n * C beyond 2^62");
    CHECK(bake(dev, dev, (int64_t)0x7fffffff * 256, dev, dev, dev, 1, 1, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_OK && bake(dev, dev, (int64_t)0x7fffffff * 256 + 1, dev, dev, dev, 1, 1, dev, dev, dev, 0.1f, 1, 0, dev) == EONERF_E_UNSUPPORTED, "the grid limit");

    // ---------------------------------------------------------------- the 64-bit size arithmetic
    uint64_t e = 0;
    CHECK(texture_elems(64, 1 << 20, 4, &e) && e == (uint64_t)1 << 28, "%llu", (unsigned long long)e);
    CHECK(texture_elems(65536, 65536, 4, &e) && e == (uint64_t)1 << 34, "a product that wraps an int: %llu", (unsigned long long)e);
    CHECK(texture_elems(1, (int64_t)1 << 60, 4, &e) && e == (uint64_t)1 << 62, "the limit itself");
    CHECK(!texture_elems(1, ((int64_t)1 << 60) + 1, 4, &e) && !texture_elems(INT_MAX, INT64_MAX, 4, &e) && !texture_elems(2, INT64_MAX, 1, &e), "past the limit, past 2^64");
    CHECK(!texture_elems(-1, 1, 1, &e) && !texture_elems(1, -1, 1, &e) && !texture_elems(1, 1, -1, &e), "negative factors");
    CHECK(texture_elems(0, INT64_MAX, 4, &e) && e == 0, "an empty table");
    CHECK(texture_blocks(0) == 0 && texture_blocks(1) == 1 && texture_blocks(256) == 1 && texture_blocks(257) == 2, "workgroups of 256");
    CHECK(texture_blocks((int64_t)0x7fffffff * 256) == 0x7fffffffu && texture_blocks((int64_t)0x7fffffff * 256 + 1) == 0 && texture_blocks(INT64_MAX) == 0, "the grid limit, no wrap at the top");

    // ---------------------------------------------------------------- ownership, weights and corners against the restatement's file
    CHECK(argc == 2, "usage: texture_checks <file of the restatement>");
    long blocks = 0, records = 0;
    if (argc == 2) {
        FILE* fh = fopen(argv[1], "rb");
        CHECK(fh != nullptr, "cannot open %s", argv[1]);
        int64_t head[3];
        while (fh && fread(head, sizeof head, 1, fh) == 1) {
            const int64_t F = head[0], n = head[2];
            const int T = (int)head[1];
            CHECK(texture_layout(F, T, &l) == EONERF_OK && l.atlas_w * l.atlas_h == n, "block %ld: F %lld T %d n %lld", blocks, (long long)F, T, (long long)n);
            if (g_fail) break;
            for (int64_t t = 0; t < n; ++t) {
                struct { int64_t face; double b[3]; } want;
                if (fread(&want, sizeof want, 1, fh) != 1) { CHECK(false, "short file"); break; }
                double b[3];
                const int64_t face = texture_texel(t % l.atlas_w, t / l.atlas_w, l.cells_per_row, l.cells, F, T, b);
                CHECK(face == want.face && same_bits(b[0], want.b[0]) && same_bits(b[1], want.b[1]) && same_bits(b[2], want.b[2]),
                      "F %lld T %d texel %lld: face %lld (%lld), b %.17g %.17g %.17g (%.17g %.17g %.17g)", (long long)F, T, (long long)t, (long long)face,
                      (long long)want.face, b[0], b[1], b[2], want.b[0], want.b[1], want.b[2]);
                ++records;
                if (g_fail > 20) break;
            }
            for (int64_t f = 0; f < F && g_fail <= 20; ++f)
                for (int c = 0; c < 3; ++c) {
                    double want[2], u, v;
                    if (fread(want, sizeof want, 1, fh) != 1) { CHECK(false, "short file"); break; }
                    texture_corner(f, c, l.cells_per_row, T, &u, &v);
                    CHECK(same_bits(u, want[0]) && same_bits(v, want[1]), "F %lld T %d face %lld corner %d: %.17g %.17g (%.17g %.17g)", (long long)F, T, (long long)f, c, u, v, want[0], want[1]);
                    ++records;
                }
            ++blocks;
        }
        if (fh) fclose(fh);
        CHECK(blocks >= 4 && records >= 1000, "%ld blocks, %ld records", blocks, records);
    }

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("texture checks ok (%ld blocks, %ld records)\n", blocks, records);
    return 0;
}
