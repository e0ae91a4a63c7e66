// Host-only checks of the occupancy grid's host logic, built for the CPU under the address + undefined-behaviour sanitizers
// (tests/host/test_occ_host.py):
//   * carve_occ (eonerf_carve.h), the layout behind eonerf_occ_workspace_bytes: for r = 1, 5, 128, 256 and every precision's slab width --
//     256-byte alignment, no two buffers overlapping, everything inside the reported size, measuring pass == carving pass, the field
//     part equal to carve_field of the chunk, and a size that stops growing with r at OCC_CHUNK cells;
//   * a grid set on a context (eonerf_ctx::occ_bits) changes nothing of carve_render / carve_sweep: the same offsets, the same size.
// No HIP runtime call is made.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
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

static void check_carve_occ(int r, bool bf16) {
    CarveCfg cfg;
    cfg.bf16 = bf16;
    const OccWs m = carve_occ(cfg, nullptr, r);
    std::vector<uint8_t> mem(m.bytes);      // the sanitizer guards its ends: the writes below stay inside
    uint8_t* base = mem.data();
    const OccWs w = carve_occ(cfg, base, r);
    CHECK(w.bytes == m.bytes && w.p_cap == m.p_cap, "r=%d: measuring pass %zu / %d, carving pass %zu / %d", r, m.bytes, m.p_cap, w.bytes, w.p_cap);
    const long long cells = (long long)r * r * r;
    const int chunk = (int)std::min<long long>(cells, OCC_CHUNK);
    CHECK(occ_chunk_cells(r) == chunk && w.p_cap == (chunk + 255) / 256 * 256 && w.p_cap >= chunk, "r=%d: chunk %d, capacity %d", r, chunk, w.p_cap);
    const FieldWs f = carve_field(cfg, base, w.p_cap);
    CHECK(f.b.px == w.b.px && f.b.sigma == w.b.sigma && f.b.simg == w.b.simg && f.b.n_pts == w.b.n_pts, "r=%d: the field part is not carve_field's", r);
    CHECK(w.bytes > f.bytes && w.bytes - f.bytes <= 4096, "r=%d: %zu bytes of reduction scratch", r, w.bytes - f.bytes);
    const size_t p = (size_t)w.p_cap;
    std::vector<Span> v;
    add(v, base, "counts", w.b.counts, sizeof(int)); add(v, base, "offsets", w.b.offsets, 2 * sizeof(int)); add(v, base, "n_pts", w.b.n_pts, 4 * sizeof(int));
    add(v, base, "px", w.b.px, p * 4); add(v, base, "py", w.b.py, p * 4); add(v, base, "pz", w.b.pz, p * 4);
    add(v, base, "tmid", w.b.tmid, p * 4); add(v, base, "delta", w.b.delta, p * 4); add(v, base, "simg", w.b.simg, p * 4);
    add(v, base, "sigma", w.b.sigma, p * 4); add(v, base, "albedo", w.b.albedo, 3 * p * 4); add(v, base, "ts", w.b.ts, p * 4); add(v, base, "tb", w.b.tb, p * 4);
    add(v, base, "partial", w.partial, OCC_SUM_BLOCKS * sizeof(double)); add(v, base, "result", w.result, 2 * sizeof(double));
    CHECK(v.size() == 15, "r=%d: %zu buffers", r, v.size());
    check_spans("carve_occ", v, w.bytes);
    // what the update's kernels write: every slot of the pass, every partial, the result pair
    for (size_t i = 0; i < p; ++i) { w.b.px[i] = w.b.py[i] = w.b.pz[i] = w.b.sigma[i] = 0.f; w.b.simg[i] = 0; }
    w.b.n_pts[0] = chunk;
    for (int i = 0; i < OCC_SUM_BLOCKS; ++i) w.partial[i] = 0.0;
    w.result[0] = 0.0; reinterpret_cast<float*>(w.result + 1)[0] = 0.f;
}

static std::vector<const void*> render_ptrs(const RenderWs& w) {
    std::vector<const void*> v = {w.cnt_first, w.cnt_retry, w.flags, w.ray_rec, w.g_ray, w.amb_save, w.m_bott, w.queue, w.enc_part, w.pipe.dy_in,
                                  w.pipe.rings, w.pipe.sync, w.det.pipe_part, w.det.wgrad_part, w.det.rad_rays, w.det.emb_rays};
    for (const PassBuffers* b : {&w.cam, &w.sun})
        for (const void* p : {(const void*)b->counts, (const void*)b->offsets, (const void*)b->n_pts, (const void*)b->px, (const void*)b->py,
                              (const void*)b->pz, (const void*)b->tmid, (const void*)b->delta, (const void*)b->sigma, (const void*)b->albedo,
                              (const void*)b->ts, (const void*)b->tb, (const void*)b->simg, (const void*)b->act, (const void*)b->grd,
                              (const void*)b->masks, (const void*)b->g_sigma, (const void*)b->g_albedo, (const void*)b->g_ts, (const void*)b->g_tb,
                              (const void*)b->g_emb, (const void*)b->g_pos})
            v.push_back(p);
    return v;
}

static void check_grid_leaves_the_layouts_alone() {
    eonerf_ctx ctx;
    memset(&ctx.cfg, 0, sizeof(ctx.cfg));
    ctx.n_cu = 256; ctx.n_pipes = 36;
    static uint32_t grid_words[4] = {0xFFFFFFFFu, 0, 0, 0};
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 20);      // (offsets only: never dereferenced)
    for (int prec = 0; prec < 3; ++prec)
        for (int pipe = 0; pipe < 2; ++pipe)
            for (int ns : {2, 37, 128, 255})
                for (int n_rays : {1, 5, 67, 300, 4096})
                    for (int flags : {0, (int)EONERF_F_SHADOWS, (int)EONERF_F_EVAL | (int)EONERF_F_SHADOWS, (int)EONERF_F_ONLY_DEPTH,
                                      (int)EONERF_F_TRAIN | (int)EONERF_F_SHADOWS}) {
                        ctx.prec = prec; ctx.bf16 = prec == EONERF_BF16; ctx.pipe = pipe && ctx.bf16; ctx.n_samples = ns;
                        ctx.occ_bits = nullptr; ctx.occ_r = 0;
                        const RenderWs a = carve_render(&ctx, base, n_rays, flags);
                        const SweepWs sa = carve_sweep(carve_cfg(&ctx), base, n_rays);
                        ctx.occ_bits = grid_words; ctx.occ_r = 5;
                        const RenderWs b = carve_render(&ctx, base, n_rays, flags);
                        const SweepWs sb = carve_sweep(carve_cfg(&ctx), base, n_rays);
                        CHECK(a.bytes == b.bytes && render_ptrs(a) == render_ptrs(b), "carve_render moves with a grid set (prec %d, %d samples, %d rays, flags %d)", prec, ns, n_rays, flags);
                        CHECK(sa.bytes == sb.bytes && sa.table == sb.table && render_ptrs(sa.r) == render_ptrs(sb.r), "carve_sweep moves with a grid set (prec %d, %d samples, %d rays)", prec, ns, n_rays);
                    }
}

int main() {
    for (int r : {1, 5, 128, 256})
        for (int bf16 = 0; bf16 < 2; ++bf16) check_carve_occ(r, bf16 != 0);
    {   // beyond OCC_CHUNK cells the workspace does not grow with r
        CarveCfg cfg;
        CHECK(carve_occ(cfg, nullptr, 64).bytes == carve_occ(cfg, nullptr, 128).bytes && carve_occ(cfg, nullptr, 128).bytes == carve_occ(cfg, nullptr, 256).bytes,
              "the workspace grows beyond one chunk");
        CHECK(carve_occ(cfg, nullptr, 5).bytes < carve_occ(cfg, nullptr, 64).bytes, "a small grid asks for a full chunk");
    }
    check_grid_leaves_the_layouts_alone();
    if (g_fail) { fprintf(stderr, "%d occupancy host checks FAILED\n", g_fail); return 1; }
    printf("occ host checks ok\n");
    return 0;
}
