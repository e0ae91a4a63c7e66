// Host-only checks of the march's host logic (include/eonerf_march.h), built for the CPU under the address + undefined-behaviour
// sanitizers (tests/host/test_march_host.py):
//   * carve_march (eonerf_carve.h), the layout behind eonerf_march_workspace_bytes: for every legal block size, n_samples-independent,
//     both slab widths, with and without the head outputs -- 256-byte alignment, no two buffers overlapping, everything inside the
//     reported size, measuring pass == carving pass, a round capacity of n_rays x block slots, a size monotone in n_rays and in block;
//   * march_refusal, the one refusal path: the documented order -- EONERF_F_TRAIN, early_stop_eps, block, workspace;
//   * carve_render's sizes are the ones recorded before the march existed (a table of 48 layouts).
// No HIP runtime call is made.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <limits>
#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_ctx.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Span { const char* name; size_t off, bytes; };

static void add(std::vector<Span>& v, const uint8_t* base, const char* name, const void* p, size_t bytes) {
    if (p) v.push_back(Span{name, (size_t)(reinterpret_cast<const uint8_t*>(p) - base), bytes});
}

static void check_spans(const char* what, std::vector<Span> v, size_t total) {
    std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.off < b.off; });
    size_t end = 0;
    for (const Span& s : v) {
        CHECK(s.off % 256 == 0, "%s: %s at %zu is not 256-byte aligned", what, s.name, s.off);
        CHECK(s.off >= end, "%s: %s at %zu overlaps its predecessor (ends at %zu)", what, s.name, s.off, end);
        end = s.off + s.bytes;
        CHECK(end <= total, "%s: %s ends at %zu beyond the reported %zu bytes", what, s.name, end, total);
    }
}

static void check_carve_march(int n_rays, int block, bool bf16, int flags) {
    CarveCfg cfg;
    cfg.bf16 = bf16;
    const MarchWs m = carve_march(cfg, nullptr, n_rays, flags, block);
    std::vector<uint8_t> mem(m.bytes);      // the sanitizer guards its ends: the writes below stay inside
    uint8_t* base = mem.data();
    const MarchWs w = carve_march(cfg, base, n_rays, flags, block);
    CHECK(w.bytes == m.bytes && w.p_cap == m.p_cap, "%d rays, block %d: measuring pass %zu / %d, carving pass %zu / %d", n_rays, block, m.bytes, m.p_cap, w.bytes, w.p_cap);
    CHECK(w.p_cap % 256 == 0 && w.p_cap >= n_rays * block && w.p_cap < n_rays * block + 256, "%d rays, block %d: capacity %d", n_rays, block, w.p_cap);
    const bool od = flags & EONERF_F_ONLY_DEPTH;
    CHECK((w.round.albedo != nullptr) == !od && (w.round.ts != nullptr) == !od && (w.round.tb != nullptr) == !od, "head outputs with flags %d", flags);
    CHECK(!w.round.act && !w.round.grd && !w.round.masks && !w.round.g_sigma, "an inference layout holds training buffers");
    const size_t R = (size_t)n_rays, p = (size_t)w.p_cap;
    std::vector<Span> v;
    for (auto q : {std::make_pair("cnt_first", w.cnt_first), {"cnt_retry", w.cnt_retry}, {"last_first", w.last_first}, {"last_retry", w.last_retry},
                   {"win_first", w.win_first}, {"win_retry", w.win_retry}, {"sun_cnt", w.sun_cnt}, {"sun_last", w.sun_last}, {"sun_win", w.sun_win},
                   {"alive", w.alive}, {"kept_cam", w.kept_cam}, {"kept_sun", w.kept_sun}, {"counts", w.round.counts}})
        add(v, base, q.first, q.second, R * sizeof(int));
    add(v, base, "flags", w.flags, 4 * sizeof(int)); add(v, base, "od", w.od, R * 4); add(v, base, "acc", w.acc, R * MARCH_ACC * 4);
    add(v, base, "ray_rec", w.ray_rec, R * RAY_REC * 4);
    add(v, base, "offsets", w.round.offsets, (R + 1) * sizeof(int)); add(v, base, "n_pts", w.round.n_pts, 4 * sizeof(int));
    add(v, base, "px", w.round.px, p * 4); add(v, base, "py", w.round.py, p * 4); add(v, base, "pz", w.round.pz, p * 4);
    add(v, base, "tmid", w.round.tmid, p * 4); add(v, base, "delta", w.round.delta, p * 4); add(v, base, "simg", w.round.simg, p * 4);
    add(v, base, "sigma", w.round.sigma, p * 4); add(v, base, "albedo", w.round.albedo, 3 * p * 4); add(v, base, "ts", w.round.ts, p * 4); add(v, base, "tb", w.round.tb, p * 4);
    CHECK(v.size() == (od ? 26u : 29u), "%zu buffers", v.size());
    check_spans("carve_march", v, w.bytes);
    // what the march's kernels write: every per-ray word, every slot of the round
    for (size_t r = 0; r < R; ++r) {
        w.cnt_first[r] = w.cnt_retry[r] = w.last_first[r] = w.last_retry[r] = w.win_first[r] = w.win_retry[r] = 0;
        w.sun_cnt[r] = w.sun_last[r] = w.sun_win[r] = w.alive[r] = w.kept_cam[r] = w.kept_sun[r] = w.round.counts[r] = 0;
        w.od[r] = 0.f;
        for (int j = 0; j < MARCH_ACC; ++j) w.acc[r * MARCH_ACC + j] = 0.f;
        for (int j = 0; j < RAY_REC; ++j) w.ray_rec[r * RAY_REC + j] = 0.f;
    }
    w.round.offsets[R] = 0; w.flags[0] = 0; w.round.n_pts[0] = 0;
    for (size_t i = 0; i < p; ++i) {
        w.round.px[i] = w.round.py[i] = w.round.pz[i] = w.round.tmid[i] = w.round.delta[i] = w.round.sigma[i] = 0.f; w.round.simg[i] = 0;
        if (!od) { w.round.albedo[2 * p + i] = 0.f; w.round.ts[i] = w.round.tb[i] = 0.f; }
    }
}

static void check_refusal_order() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const int T = EONERF_F_TRAIN;
    // every later defect is present as well: the earlier one answers
    CHECK(march_refusal(T, -1.f, 7, 0, 100) == EONERF_E_UNSUPPORTED, "EONERF_F_TRAIN comes first");
    CHECK(march_refusal(T | EONERF_F_SHADOWS, 0.1f, 32, 100, 100) == EONERF_E_UNSUPPORTED, "EONERF_F_TRAIN alone");
    for (float e : {-1e-6f, 1.0f, 2.0f, nan, -INFINITY, INFINITY}) CHECK(march_refusal(0, e, 7, 0, 100) == EONERF_E_ARG, "early_stop_eps %g", e);
    for (float e : {0.0f, 1e-5f, 0.6f, 0.99999994f})
        for (int b : {16, 32, 64}) CHECK(march_refusal(EONERF_F_SHADOWS, e, b, 100, 100) == EONERF_OK, "eps %g block %d", e, b);
    for (int b : {0, -16, 1, 8, 15, 17, 48, 128}) CHECK(march_refusal(0, 0.1f, b, 0, 100) == EONERF_E_ARG, "block %d", b);
    CHECK(march_refusal(0, 0.1f, 32, 99, 100) == EONERF_E_WORKSPACE && march_refusal(0, 0.1f, 32, 0, 100) == EONERF_E_WORKSPACE, "a short workspace");
    // eps and block are both EONERF_E_ARG: told apart by fixing one at a time
    CHECK(march_refusal(0, 1.5f, 32, 0, 100) == EONERF_E_ARG && march_refusal(0, 0.5f, 33, 0, 100) == EONERF_E_ARG, "argument checks before the workspace");
    CHECK(march_block_ok(16) && march_block_ok(32) && march_block_ok(64) && !march_block_ok(0) && !march_block_ok(24), "legal block sizes");
    CHECK(march_rounds(2, 16) == 1 && march_rounds(37, 16) == 3 && march_rounds(128, 32) == 4 && march_rounds(129, 32) == 4 && march_rounds(130, 32) == 5
          && march_rounds(255, 64) == 4 && march_rounds(256, 64) == 4, "rounds of a pass");
}

// carve_render(prec, n_samples, n_rays, flags).bytes as recorded before carve_march was added to the header
struct Recorded { int prec, ns, n_rays, flags; unsigned long long bytes; };
static const Recorded RECORDED[] = {
    {0, 37, 67, 0, 129024ull},  {0, 37, 67, 1, 201984ull},  {0, 37, 67, 8, 77824ull},  {0, 37, 67, 5, 102317824ull},
    {0, 37, 4096, 0, 7341056ull},  {0, 37, 4096, 1, 11503104ull},  {0, 37, 4096, 8, 4391936ull},  {0, 37, 4096, 5, 5878614784ull},
    {0, 128, 67, 0, 423936ull},  {0, 128, 67, 1, 668928ull},  {0, 128, 67, 8, 249856ull},  {0, 128, 67, 5, 347119360ull},
    {0, 128, 4096, 0, 25232384ull},  {0, 128, 4096, 1, 39831040ull},  {0, 128, 4096, 8, 14828544ull},  {0, 128, 4096, 5, 20729907968ull},
    {1, 37, 67, 0, 129024ull},  {1, 37, 67, 1, 201984ull},  {1, 37, 67, 8, 77824ull},  {1, 37, 67, 5, 52346624ull},
    {1, 37, 4096, 0, 7341056ull},  {1, 37, 4096, 1, 11503104ull},  {1, 37, 4096, 8, 4391936ull},  {1, 37, 4096, 5, 3000273664ull},
    {1, 128, 67, 0, 423936ull},  {1, 128, 67, 1, 668928ull},  {1, 128, 67, 8, 249856ull},  {1, 128, 67, 5, 177217280ull},
    {1, 128, 4096, 0, 25232384ull},  {1, 128, 4096, 1, 39831040ull},  {1, 128, 4096, 8, 14828544ull},  {1, 128, 4096, 5, 10575760128ull},
    {2, 37, 67, 0, 129024ull},  {2, 37, 67, 1, 201984ull},  {2, 37, 67, 8, 77824ull},  {2, 37, 67, 5, 102317824ull},
    {2, 37, 4096, 0, 7341056ull},  {2, 37, 4096, 1, 11503104ull},  {2, 37, 4096, 8, 4391936ull},  {2, 37, 4096, 5, 5878614784ull},
    {2, 128, 67, 0, 423936ull},  {2, 128, 67, 1, 668928ull},  {2, 128, 67, 8, 249856ull},  {2, 128, 67, 5, 347119360ull},
    {2, 128, 4096, 0, 25232384ull},  {2, 128, 4096, 1, 39831040ull},  {2, 128, 4096, 8, 14828544ull},  {2, 128, 4096, 5, 20729907968ull},
};

static void check_carve_render_unchanged() {
    for (const Recorded& q : RECORDED) {
        CarveCfg cfg;
        cfg.bf16 = q.prec == EONERF_BF16; cfg.n_samples = q.ns;
        const size_t got = carve_render(cfg, nullptr, q.n_rays, q.flags).bytes;
        CHECK(got == (size_t)q.bytes, "carve_render(prec %d, %d samples, %d rays, flags %d) = %zu, recorded %llu", q.prec, q.ns, q.n_rays, q.flags, got, q.bytes);
    }
}

int main() {
    for (int n_rays : {1, 5, 67, 300, 4096})
        for (int block : {16, 32, 64})
            for (int bf16 = 0; bf16 < 2; ++bf16)
                for (int flags : {0, (int)EONERF_F_SHADOWS, (int)EONERF_F_EVAL | (int)EONERF_F_SHADOWS, (int)EONERF_F_ONLY_DEPTH})
                    check_carve_march(n_rays, block, bf16 != 0, flags);
    {   // monotone in n_rays and in block; independent of n_samples; the shadow flag adds nothing (one round buffer serves both passes)
        CarveCfg cfg;
        size_t prev = 0;
        for (int n_rays = 0; n_rays <= 700; ++n_rays) {
            const size_t b = carve_march(cfg, nullptr, n_rays, 0, 32).bytes;
            CHECK(b >= prev, "carve_march shrinks from %d to %d rays", n_rays - 1, n_rays);
            prev = b;
        }
        CHECK(carve_march(cfg, nullptr, 300, 0, 16).bytes < carve_march(cfg, nullptr, 300, 0, 32).bytes
              && carve_march(cfg, nullptr, 300, 0, 32).bytes < carve_march(cfg, nullptr, 300, 0, 64).bytes, "not monotone in block");
        CarveCfg c2 = cfg; c2.n_samples = 255;
        CHECK(carve_march(cfg, nullptr, 300, 0, 32).bytes == carve_march(c2, nullptr, 300, 0, 32).bytes, "the layout depends on n_samples");
        CHECK(carve_march(cfg, nullptr, 300, 0, 32).bytes == carve_march(cfg, nullptr, 300, EONERF_F_SHADOWS, 32).bytes, "the shadow pass has buffers of its own");
        CHECK(carve_march(cfg, nullptr, 300, EONERF_F_ONLY_DEPTH, 32).bytes < carve_march(cfg, nullptr, 300, 0, 32).bytes, "a depth-only layout holds head outputs");
    }
    check_refusal_order();
    check_carve_render_unchanged();
    if (g_fail) { fprintf(stderr, "%d march host checks FAILED\n", g_fail); return 1; }
    printf("march host checks ok\n");
    return 0;
}
