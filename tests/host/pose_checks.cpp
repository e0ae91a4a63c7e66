// Host-only checks of eonerf_render_origin_grad's refusals and size arithmetic (eonerf_pose_check.h), built for the CPU under the
// address + undefined-behaviour sanitizers (tests/host/test_pose_host.py).  The checks are the functions the entry point of
// eonerf_pose.hip calls before it launches anything.  No HIP runtime call is made and no pointer is dereferenced.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../eonerf_code_amd/csrc/eonerf_pose_check.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main() {
    // never dereferenced: stand for device pointers
    const void* dev = reinterpret_cast<const void*>((uintptr_t)1 << 40);
    const void* dev2 = reinterpret_cast<const void*>((uintptr_t)3 << 40);
    const int T = EONERF_F_TRAIN, S = EONERF_F_SHADOWS;

    // ---------------------------------------------------------------- capacity and scratch sizes
    CHECK(pose_p_cap(1, 128) == 256 && pose_p_cap(0, 128) == 256, "one ray (and an empty batch) round up to one granule");
    CHECK(pose_p_cap(192, 128) == 24576 && pose_p_cap(193, 128) == 24576 && pose_p_cap(4096, 128) == 520192, "127 intervals per ray");
    CHECK(pose_p_cap(96, 37) == 3584 && pose_p_cap(3, 2) == 256, "other sample counts");
    CHECK(pose_p_cap(-1, 128) == 0 && pose_p_cap(1, 1) == 0 && pose_p_cap(1, 257) == 0, "refused shapes");
    CHECK(pose_p_cap(INT_MAX, 256) == 0 && pose_p_cap((int64_t)1 << 40, 128) == 0, "a capacity that leaves an int (no wrap in 64 bits)");
    CHECK(pose_p_cap(16909318, 128) == 2147483392ull && pose_p_cap(16909319, 128) == 0, "the last capacity that fits");
    PoseScratch s;
    CHECK(pose_scratch(192, 128, &s) && s.g_pos_off == 0 && s.rays_off == 3u * 24576 * 4 && s.bytes == s.rays_off + 2304 + 256, "192 rays");
    CHECK(pose_scratch(1, 128, &s) && s.rays_off == 3072 && s.bytes == 3072 + 256 + 256, "one ray: the per-ray block is rounded up to 256 B");
    CHECK(pose_scratch(0, 128, &s) && s.bytes == 3072 + 256, "an empty batch");
    CHECK(pose_scratch(16909318, 128, &s) && s.bytes > ((size_t)1 << 34), "the largest batch: sizes beyond 2^32 stay exact");
    CHECK(s.rays_off % 256 == 0 && s.bytes % 256 == 0, "alignment");
    CHECK(!pose_scratch(-1, 128, &s) && !pose_scratch(INT_MAX, 256, &s), "refused sizes");

    // ---------------------------------------------------------------- arguments
    CHECK(pose_check_args(dev, dev, dev, dev, 192, T | S, dev, dev, dev, dev) == EONERF_OK, "a plain call");
    CHECK(pose_check_args(dev, dev, dev, dev, 192, T, dev, dev, nullptr, dev) == EONERF_OK, "no d_origins");
    CHECK(pose_check_args(dev, dev, dev, dev, 192, T | EONERF_F_RGB_LOSS, dev, dev, dev, nullptr) == EONERF_OK, "no d_offsets");
    CHECK(pose_check_args(dev, dev, dev, dev, 0, T, dev, dev, dev, dev) == EONERF_OK, "n_rays == 0");
    CHECK(pose_check_args(nullptr, dev, dev, dev, 1, T, dev, dev, dev, dev) == EONERF_E_ARG, "null ctx");
    CHECK(pose_check_args(dev, nullptr, dev, dev, 1, T, dev, dev, dev, dev) == EONERF_E_ARG, "null flat");
    CHECK(pose_check_args(dev, dev, nullptr, dev, 1, T, dev, dev, dev, dev) == EONERF_E_ARG, "null rays");
    CHECK(pose_check_args(dev, dev, dev, nullptr, 1, T, dev, dev, dev, dev) == EONERF_E_ARG, "null img_idx");
    CHECK(pose_check_args(dev, dev, dev, dev, 1, T, nullptr, dev, dev, dev) == EONERF_E_ARG, "null workspace");
    CHECK(pose_check_args(dev, dev, dev, dev, 1, T, dev, nullptr, dev, dev) == EONERF_E_ARG, "null scratch");
    CHECK(pose_check_args(dev, dev, dev, dev, 1, T, dev, dev, nullptr, nullptr) == EONERF_E_ARG, "no output");
    CHECK(pose_check_args(dev, dev, dev, dev, -1, T, dev, dev, dev, dev) == EONERF_E_ARG, "n_rays < 0");
    CHECK(pose_check_args(dev, dev, dev, dev, 1, S, dev, dev, dev, dev) == EONERF_E_STATE, "not a training call");
    CHECK(pose_check_args(dev, dev, dev, dev, 1, T | EONERF_F_ONLY_DEPTH, dev, dev, dev, dev) == EONERF_E_STATE, "a depth-only call");

    // ---------------------------------------------------------------- the order rule
    CHECK(pose_check_record(true, dev, 192, T | S, 128, dev, 192, T | S, 128) == EONERF_OK, "behind its backward");
    CHECK(pose_check_record(false, dev, 192, T | S, 128, dev, 192, T | S, 128) == EONERF_E_STATE, "no backward");
    CHECK(pose_check_record(true, dev2, 192, T | S, 128, dev, 192, T | S, 128) == EONERF_E_STATE, "another workspace");
    CHECK(pose_check_record(true, dev, 191, T | S, 128, dev, 192, T | S, 128) == EONERF_E_STATE, "another n_rays");
    CHECK(pose_check_record(true, dev, 192, T, 128, dev, 192, T | S, 128) == EONERF_E_STATE, "other flags");
    CHECK(pose_check_record(true, dev, 192, T | S, 64, dev, 192, T | S, 128) == EONERF_E_STATE, "another sample count");

    // ---------------------------------------------------------------- sizes
    pose_scratch(192, 128, &s);
    CHECK(pose_check_sizes(192, 128, 1000, 1000, s.bytes) == EONERF_OK, "exact sizes");
    CHECK(pose_check_sizes(192, 128, 999, 1000, s.bytes) == EONERF_E_WORKSPACE, "a short workspace");
    CHECK(pose_check_sizes(192, 128, 1000, 1000, s.bytes - 1) == EONERF_E_WORKSPACE, "a short scratch");
    CHECK(pose_check_sizes(192, 128, 1000, 1000, 0) == EONERF_E_WORKSPACE, "no scratch");
    CHECK(pose_check_sizes(INT_MAX, 256, SIZE_MAX, 1000, SIZE_MAX) == EONERF_E_UNSUPPORTED, "a batch beyond the capacity");

    if (g_fail) { fprintf(stderr, "%d pose check(s) failed\n", g_fail); return 1; }
    printf("pose checks ok\n");
    return 0;
}
