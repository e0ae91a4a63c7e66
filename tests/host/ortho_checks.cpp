// Host-only checks of the true-orthophoto entry points' refusals and size arithmetic (eonerf_ortho_check.h), built for the CPU under the
// address + undefined-behaviour sanitizers (tests/host/test_ortho_host.py).  The checks are the functions the entry points of
// eonerf_ortho.hip call before they launch anything.  No HIP runtime call is made and no pointer is dereferenced except the
// host arrays (scale, offset, gain, bias).
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../eonerf_code_amd/csrc/eonerf_ortho_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main() {
    // never dereferenced: stands for a device pointer
    const void* dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);
    const float nanf_ = nanf(""), inff_ = INFINITY;

    // ---------------------------------------------------------------- ground
    float sc[3] = {300.f, 300.f, 60.f}, off[3] = {436000.f, 3355000.f, 20.f};
    CHECK(ortho_check_ground(dev, 11, dev, 257, sc, off, 17, dev) == EONERF_OK, "a plain call");
    CHECK(ortho_check_ground(dev, 6, dev, 0, sc, off, 1, dev) == EONERF_OK && ortho_check_ground(dev, 6, dev, 0, sc, off, 60, dev) == EONERF_OK, "n == 0, zones 1 and 60");
    CHECK(ortho_check_ground(nullptr, 11, dev, 1, sc, off, 17, dev) == EONERF_E_ARG, "null rays");
    CHECK(ortho_check_ground(dev, 11, nullptr, 1, sc, off, 17, dev) == EONERF_E_ARG, "null depth");
    CHECK(ortho_check_ground(dev, 11, dev, 1, nullptr, off, 17, dev) == EONERF_E_ARG, "null scale");
    CHECK(ortho_check_ground(dev, 11, dev, 1, sc, nullptr, 17, dev) == EONERF_E_ARG, "null offset");
    CHECK(ortho_check_ground(dev, 11, dev, 1, sc, off, 17, nullptr) == EONERF_E_ARG, "null output");
    CHECK(ortho_check_ground(dev, 11, dev, -1, sc, off, 17, dev) == EONERF_E_ARG, "n < 0");
    CHECK(ortho_check_ground(dev, 5, dev, 1, sc, off, 17, dev) == EONERF_E_ARG, "ray_stride 5");
    CHECK(ortho_check_ground(dev, 11, dev, 1, sc, off, 0, dev) == EONERF_E_ARG && ortho_check_ground(dev, 11, dev, 1, sc, off, 61, dev) == EONERF_E_ARG, "zones 0 and 61");
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {sc[0], sc[1], sc[2]};
        bad[k] = nanf_;
        CHECK(ortho_check_ground(dev, 11, dev, 1, bad, off, 17, dev) == EONERF_E_ARG, "NaN scale %d", k);
        bad[k] = inff_;
        CHECK(ortho_check_ground(dev, 11, dev, 1, sc, bad, 17, dev) == EONERF_E_ARG, "infinite offset %d", k);
    }
    CHECK(ortho_check_ground(dev, 11, dev, LONG_MAX, sc, off, 17, dev) == EONERF_E_UNSUPPORTED, "a grid beyond 2^31 - 1 workgroups");

    // ---------------------------------------------------------------- gather
    float gain[4] = {0.5f, 1.f, 1.5f, 2.f}, bias[4] = {0.f, 0.1f, -0.1f, 0.f};
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 3, gain, bias, 0.2f, dev, dev, dev) == EONERF_OK, "a plain call");
    CHECK(ortho_check_gather(dev, 33, dev, nullptr, 8, 9, 3, nullptr, nullptr, 0.2f, nullptr, nullptr, dev) == EONERF_OK, "colrow alone needs no pixels");
    CHECK(ortho_check_gather(dev, 0, dev, dev, 1, 1, 1, gain, bias, 0.2f, dev, nullptr, nullptr) == EONERF_OK, "n == 0");
    CHECK(ortho_check_gather(nullptr, 33, dev, dev, 8, 9, 3, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "null points");
    CHECK(ortho_check_gather(dev, 33, nullptr, dev, 8, 9, 3, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "null rpc");
    CHECK(ortho_check_gather(dev, -1, dev, dev, 8, 9, 3, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "n < 0");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 3, gain, bias, 0.2f, nullptr, nullptr, nullptr) == EONERF_E_ARG, "no output");
    CHECK(ortho_check_gather(dev, 33, dev, nullptr, 8, 9, 3, gain, bias, 0.2f, dev, nullptr, nullptr) == EONERF_E_ARG, "a layer without pixels");
    CHECK(ortho_check_gather(dev, 33, dev, nullptr, 8, 9, 3, gain, bias, 0.2f, nullptr, dev, nullptr) == EONERF_E_ARG, "a weight without pixels");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 3, nullptr, bias, 0.2f, dev, nullptr, nullptr) == EONERF_E_ARG, "a layer without gain");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 3, gain, nullptr, 0.2f, dev, nullptr, nullptr) == EONERF_E_ARG, "a layer without bias");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 0, 9, 3, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "h == 0");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 0, 3, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "w == 0");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 0, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "0 channels");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 5, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "5 channels");
    CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 3, gain, bias, nanf_, dev, dev, dev) == EONERF_E_ARG, "NaN min_visibility");
    for (int c = 0; c < 4; ++c) {
        float g[4] = {gain[0], gain[1], gain[2], gain[3]}, b[4] = {bias[0], bias[1], bias[2], bias[3]};
        g[c] = 0.f;
        CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 4, g, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "zero gain %d", c);
        g[c] = nanf_;
        CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 4, g, bias, 0.2f, dev, dev, dev) == EONERF_E_ARG, "NaN gain %d", c);
        // a channel past `channels` is not read
        if (c == 3) CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 3, g, bias, 0.2f, dev, dev, dev) == EONERF_OK, "gain[3] with 3 channels");
        b[c] = inff_;
        CHECK(ortho_check_gather(dev, 33, dev, dev, 8, 9, 4, gain, b, 0.2f, dev, dev, dev) == EONERF_E_ARG, "infinite bias %d", c);
    }
    CHECK(ortho_check_gather(dev, 33, dev, dev, 65536, 65536, 4, gain, bias, 0.2f, dev, dev, dev) == EONERF_OK, "an image of 2^34 floats");
    CHECK(ortho_check_gather(dev, 33, dev, dev, INT_MAX, INT_MAX, 4, gain, bias, 0.2f, dev, dev, dev) == EONERF_E_UNSUPPORTED, "h * w * C beyond 2^62");

    // ---------------------------------------------------------------- fuse
    CHECK(ortho_check_fuse(dev, dev, 3, 33, 4, EONERF_ORTHO_MEDIAN, dev, dev, dev) == EONERF_OK, "a plain call");
    CHECK(ortho_check_fuse(dev, dev, 3, 0, 4, EONERF_ORTHO_MEAN, dev, nullptr, nullptr) == EONERF_OK, "n == 0");
    CHECK(ortho_check_fuse(nullptr, dev, 3, 33, 4, 0, dev, dev, dev) == EONERF_E_ARG, "null layers");
    CHECK(ortho_check_fuse(dev, nullptr, 3, 33, 4, 0, dev, dev, dev) == EONERF_E_ARG, "null weights");
    CHECK(ortho_check_fuse(dev, dev, 0, 33, 4, 0, dev, dev, dev) == EONERF_E_ARG, "K == 0");
    CHECK(ortho_check_fuse(dev, dev, 3, -1, 4, 0, dev, dev, dev) == EONERF_E_ARG, "n < 0");
    CHECK(ortho_check_fuse(dev, dev, 3, 33, 0, 0, dev, dev, dev) == EONERF_E_ARG && ortho_check_fuse(dev, dev, 3, 33, 5, 0, dev, dev, dev) == EONERF_E_ARG, "channels");
    CHECK(ortho_check_fuse(dev, dev, 3, 33, 4, 2, dev, dev, dev) == EONERF_E_ARG && ortho_check_fuse(dev, dev, 3, 33, 4, -1, dev, dev, dev) == EONERF_E_ARG, "mode");
    CHECK(ortho_check_fuse(dev, dev, 3, 33, 4, 0, nullptr, nullptr, nullptr) == EONERF_E_ARG, "no output");
    CHECK(ortho_check_fuse(dev, dev, EONERF_ORTHO_MAX_MEDIAN, 33, 3, EONERF_ORTHO_MEDIAN, dev, dev, dev) == EONERF_OK, "K = 64 median");
    CHECK(ortho_check_fuse(dev, dev, EONERF_ORTHO_MAX_MEDIAN + 1, 33, 3, EONERF_ORTHO_MEDIAN, dev, dev, dev) == EONERF_E_UNSUPPORTED, "K = 65 median");
    CHECK(ortho_check_fuse(dev, dev, EONERF_ORTHO_MAX_MEDIAN + 1, 33, 3, EONERF_ORTHO_MEAN, dev, dev, dev) == EONERF_OK, "K = 65 mean");
    CHECK(ortho_check_fuse(dev, dev, INT_MAX, 33, 3, EONERF_ORTHO_MEAN, dev, dev, dev) == EONERF_OK, "the mean takes any K");

    // ---------------------------------------------------------------- K * n * C in 64 bits
    uint64_t e = 0;
    CHECK(ortho_elems(64, 1 << 20, 4, &e) && e == (uint64_t)1 << 28, "%llu", (unsigned long long)e);
    CHECK(ortho_elems(65536, 65536, 4, &e) && e == (uint64_t)1 << 34, "a product that wraps an int: %llu", (unsigned long long)e);
    CHECK(ortho_elems(INT_MAX, INT_MAX, 1, &e) && e == (uint64_t)INT_MAX * INT_MAX, "%llu", (unsigned long long)e);
    CHECK(ortho_elems(1, (int64_t)1 << 60, 4, &e) && e == (uint64_t)1 << 62, "the limit itself");
    CHECK(!ortho_elems(1, ((int64_t)1 << 60) + 1, 4, &e), "one past the limit");
    CHECK(!ortho_elems(INT_MAX, INT64_MAX, 4, &e) && !ortho_elems(2, INT64_MAX, 1, &e), "products beyond 2^64");
    CHECK(!ortho_elems(-1, 1, 1, &e) && !ortho_elems(1, -1, 1, &e) && !ortho_elems(1, 1, -1, &e), "negative factors");
    CHECK(ortho_elems(0, INT64_MAX, 4, &e) && e == 0 && ortho_elems(INT_MAX, 0, 4, &e) && e == 0, "an empty table");
    CHECK(ortho_check_fuse(dev, dev, INT_MAX, LONG_MAX, 4, EONERF_ORTHO_MEAN, dev, dev, dev) == EONERF_E_UNSUPPORTED, "K * n * C beyond 2^62");
    CHECK(ortho_blocks(0) == 0 && ortho_blocks(1) == 1 && ortho_blocks(256) == 1 && ortho_blocks(257) == 2, "workgroups of 256");
    CHECK(ortho_blocks((int64_t)0x7fffffff * 256) == 0x7fffffffu && ortho_blocks((int64_t)0x7fffffff * 256 + 1) == 0, "the grid limit");
    CHECK(ortho_blocks(INT64_MAX) == 0, "no wrap at the top");

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("ortho checks ok\n");
    return 0;
}
