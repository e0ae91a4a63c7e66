// Host-only checks of the sun sweep's workspace layout (carve_sweep, eonerf_carve.h) and its ray bound, built for the CPU under the
// address + undefined-behaviour sanitizers (tests/host/test_sweep_host.py).  The sweep's per-sun launches are the forward's launches on the
// forward's layout: what has to hold is that the first bytes of the sweep's carve ARE carve_render's, pointer for pointer, and that the
// table copy behind them overlaps nothing.  No HIP runtime call is made.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_carve.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Span { const char* name; size_t lo, hi; };
static void add(std::vector<Span>& v, const char* name, const void* p, size_t bytes, const uint8_t* base) {
    if (p) v.push_back(Span{name, (size_t)(reinterpret_cast<const uint8_t*>(p) - base), (size_t)(reinterpret_cast<const uint8_t*>(p) - base) + bytes});
}
static void add_pass(std::vector<Span>& v, const PassBuffers& b, int n_rays, size_t p_cap, bool full, const uint8_t* base) {
    add(v, "counts", b.counts, 4 * (size_t)n_rays, base); add(v, "offsets", b.offsets, 4 * (size_t)(n_rays + 1), base); add(v, "n_pts", b.n_pts, 16, base);
    add(v, "px", b.px, 4 * p_cap, base); add(v, "py", b.py, 4 * p_cap, base); add(v, "pz", b.pz, 4 * p_cap, base);
    add(v, "tmid", b.tmid, 4 * p_cap, base); add(v, "delta", b.delta, 4 * p_cap, base); add(v, "simg", b.simg, 4 * p_cap, base);
    add(v, "sigma", b.sigma, 4 * p_cap, base);
    if (full) { add(v, "albedo", b.albedo, 12 * p_cap, base); add(v, "ts", b.ts, 4 * p_cap, base); add(v, "tb", b.tb, 4 * p_cap, base); }
}

static void check_sweep(const CarveCfg& cfg, int n_rays) {
    CHECK(sweep_rays_addressable(n_rays, cfg.n_samples), "%d rays x %d samples", n_rays, cfg.n_samples);
    const SweepWs m = carve_sweep(cfg, nullptr, n_rays);                       // measuring pass
    // a fake, never dereferenced base: only differences of pointers are formed
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
    const SweepWs s = carve_sweep(cfg, base, n_rays);
    const RenderWs r = carve_render(cfg, base, n_rays, EONERF_F_SHADOWS);      // what eonerf_render_forward(EONERF_F_SHADOWS) carves
    CHECK(s.bytes == m.bytes && s.r.bytes == m.r.bytes, "measuring pass %zu != carving pass %zu", m.bytes, s.bytes);
    CHECK(m.table == nullptr && m.r.ray_rec == nullptr && m.r.cam.px == nullptr && m.r.sun.px == nullptr, "the measuring pass forms no pointer");
    const size_t p_cap = (size_t)p_cap_of(n_rays, cfg.n_samples);
    CHECK(p_cap % 256 == 0 && p_cap >= (size_t)n_rays * (cfg.n_samples - 1), "p_cap %zu", p_cap);

    // every sub-buffer inside [0, bytes), 256-byte aligned, disjoint from the others
    std::vector<Span> v;
    add(v, "cnt_first", s.r.cnt_first, 4 * (size_t)n_rays, base); add(v, "cnt_retry", s.r.cnt_retry, 4 * (size_t)n_rays, base); add(v, "flags", s.r.flags, 16, base);
    add(v, "ray_rec", s.r.ray_rec, 4 * (size_t)n_rays * RAY_REC, base);
    add_pass(v, s.r.cam, n_rays, p_cap, true, base);
    add_pass(v, s.r.sun, n_rays, p_cap, false, base);
    add(v, "table", s.table, 4 * (size_t)n_rays * 11, base);
    CHECK(v.size() == 4 + 13 + 10 + 1, "%zu sub-buffers", v.size());
    std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    for (size_t i = 0; i < v.size(); ++i) {
        CHECK(v[i].lo % 256 == 0, "%s not 256-byte aligned", v[i].name);
        CHECK(v[i].hi <= s.bytes, "%s ends at %zu beyond the workspace (%zu)", v[i].name, v[i].hi, s.bytes);
        if (i + 1 < v.size()) CHECK(v[i].hi <= v[i + 1].lo, "%s overlaps %s", v[i].name, v[i + 1].name);
    }

    // the first carve_render(...).bytes - 256 bytes: carve_render's layout, pointer for pointer (RenderWs holds pointers and sizes only)
    CHECK(s.r.bytes == r.bytes, "render part %zu, carve_render %zu", s.r.bytes, r.bytes);
    CHECK(s.r.cnt_first == r.cnt_first && s.r.cnt_retry == r.cnt_retry && s.r.flags == r.flags && s.r.ray_rec == r.ray_rec, "per-ray buffers");
    CHECK(s.r.g_ray == nullptr && s.r.amb_save == nullptr && s.r.m_bott == nullptr && s.r.queue == nullptr && s.r.enc_part == nullptr &&
          s.r.pipe.sync == nullptr && s.r.pipe.dy_in == nullptr && s.r.pipe.rings == nullptr && s.r.det.pipe_part == nullptr &&
          s.r.det.wgrad_part == nullptr && s.r.det.rad_rays == nullptr && s.r.det.emb_rays == nullptr, "an inference layout has no training buffer");
    CHECK(memcmp(&s.r.cam, &r.cam, sizeof(PassBuffers)) == 0, "camera pass buffers");
    CHECK(memcmp(&s.r.sun, &r.sun, sizeof(PassBuffers)) == 0, "sun pass buffers");
    CHECK(s.r.cam.albedo && s.r.cam.ts && s.r.cam.tb && s.r.sun.px && !s.r.sun.albedo && !s.r.cam.act && !s.r.sun.act, "full camera pass, density-only sun pass");

    // the table copy: R x 11 floats, behind everything carve_render laid out, in front of the tail pad
    const size_t t_lo = (size_t)(reinterpret_cast<uint8_t*>(s.table) - base);
    CHECK(t_lo >= r.bytes - 256 && t_lo < r.bytes, "table at %zu, carve_render's allocator stopped at %zu", t_lo, r.bytes - 256);
    CHECK(s.bytes == t_lo + 4 * (size_t)n_rays * 11 + 256, "table of %zu bytes", s.bytes - 256 - t_lo);
    for (const Span& sp : v) if (sp.name[0] != 't' || sp.name[1] != 'a') CHECK(sp.hi <= t_lo, "%s reaches into the table", sp.name);
}

int main() {
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int ns : {2, 3, 128, 256})
            for (int n_rays : {1, 37, 4096, 65536}) {
                CarveCfg c;
                c.bf16 = bf16 != 0; c.n_samples = ns;
                check_sweep(c, n_rays);
                // the training switches of a context do not reach an inference layout
                CarveCfg t = c;
                t.pipe = true; t.n_pipes = 36; t.deterministic = t.pipe_partials = true; t.enc_part_wgs = 256;
                CHECK(carve_sweep(t, nullptr, n_rays).bytes == carve_sweep(c, nullptr, n_rays).bytes, "switches change the sweep layout");
            }
    // the 64-bit ray bound: 2^24 rays x 199 intervals wrap an int (the forward's own bound, a multiple of 128 samples, admits them)
    CHECK(!sweep_rays_addressable(1 << 24, 200), "(1 << 24, 200) admitted");
    CHECK(sweep_rays_addressable(1 << 24, 128) && !sweep_rays_addressable(1 << 24, 129), "bound at 2^24 rays");
    CHECK(sweep_rays_addressable((INT_MAX - 255) / 255, 256) && !sweep_rays_addressable((INT_MAX - 255) / 255 + 1, 256), "bound at 256 samples");
    CHECK(sweep_rays_addressable(INT_MAX - 255, 2) && !sweep_rays_addressable(INT_MAX - 254, 2) && sweep_rays_addressable(0, 256), "bound at 2 samples");
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("sweep checks ok\n");
    return 0;
}
