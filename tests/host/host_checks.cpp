// Host-only checks of the C ABI's host logic, built for the CPU under the address + undefined-behaviour sanitizers (tests/test_host_sanitizers.py):
//   * eonerf_pack.cpp: the flat parameter layout and every packed weight stream (gather maps) for several image counts -- every
//     destination inside its stream, every source inside the flat buffer, no byte written twice, chunk tables consistent with the
//     grouping the chain kernels walk;
//   * eonerf_carve.h: the workspace layout for a set of (n_rays, flags, configuration) -- 256-byte alignment, no two buffers
//     overlapping, everything inside the reported size, measuring pass == carving pass; the same for the layouts of the eonerf_field_*
//     entry points (carve_field, carve_field_train).  What the kernels then touch inside and around these spans is the device side's
//     business: tests/test_workspace_contract.py.
//   * eonerf_wgrad_plan.h: the job table and slice plan of the weight-gradient GEMM launch for every reachable combination of precision,
//     backward path, pass set and switches -- the table fits, the items are a running sum that fits deterministic mode's partial buffer,
//     every operand stays inside the slab block it starts in, the wave grid covers the product, the riders sit on the right job.
//   * eonerf_layout_table.h (include/eonerf_layout.h): over the same enumeration of layouts, every offset eonerf_workspace_layout and eonerf_ray_layout report
//     is the carve's own pointer minus the base, a buffer the carve does not have is UINT64_MAX, and the refusals write nothing.
// No HIP runtime call is made (GPU sanitizers are not available on this pool; the device side is covered by the parity tests).
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../eonerf_code_amd/csrc/eonerf_pack.h"
#include "../../eonerf_code_amd/csrc/eonerf_carve.h"
#include "../../eonerf_code_amd/csrc/eonerf_wgrad_plan.h"
#include "../../eonerf_code_amd/csrc/eonerf_layout_table.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void check_stream(const char* name, const PackedStream& s, const ParamLayout& pl, bool chain) {
    std::vector<uint8_t> hit(s.bytes, 0);
    auto walk = [&](const std::vector<PackEntry>& e, int esz) {
        for (const PackEntry& pe : e) {
            CHECK((size_t)pe.dst + esz <= s.bytes, "%s: destination %u beyond the stream (%zu bytes)", name, pe.dst, s.bytes);
            // sources beyond the flat buffer index the fold buffer (ParamLayout::fold_w / fold_b, eonerf_pack.h)
            CHECK(pe.src >= -1 && (pe.src < 0 || (size_t)pe.src < pl.total + FOLD_FLOATS), "%s: source %d outside the flat + fold buffers (%zu + %d floats)", name, pe.src, pl.total, FOLD_FLOATS);
            CHECK(pe.dst % esz == 0, "%s: misaligned destination %u", name, pe.dst);
            if ((size_t)pe.dst + esz <= s.bytes)
                for (int k = 0; k < esz; ++k) { CHECK(!hit[pe.dst + k], "%s: byte %u written twice", name, pe.dst + k); hit[pe.dst + k] = 1; }
        }
    };
    walk(s.e16, 2);
    walk(s.e16lo, 2);
    walk(s.e32, 4);
    size_t covered = 0;
    for (uint8_t h : hit) covered += h;
    CHECK(covered == s.bytes, "%s: %zu of %zu bytes have a gather entry", name, covered, s.bytes);
    if (chain) {
        size_t off = 0;
        for (const ChunkDesc& c : s.chunks) {
            CHECK(c.off == off, "%s: chunk table not contiguous", name);
            const uint32_t slot = s.e16lo.empty() ? (uint32_t)(CHUNK_KG_TARGET * 1024 + 1024) : (uint32_t)(CHUNK_KG_TARGET_SPLIT * PH3::UNIT_B + 1024);
            CHECK(c.bytes <= slot, "%s: chunk of %u bytes exceeds the LDS slot", name, c.bytes);
            CHECK(c.bytes % 128 == 0, "%s: chunk size %u", name, c.bytes);
            off += c.bytes;
        }
        CHECK(off == s.bytes, "%s: chunks cover %zu of %zu bytes", name, off, s.bytes);
    }
}

static void check_layout(int n_img) {
    ParamLayout pl;
    pl.build(n_img);
    CHECK(pl.t.size() == 42, "parameter tensors: %zu", pl.t.size());      // the 44 state_dict entries minus the two int64 encoder buffers
    size_t end = 0;
    for (const ParamInfo& p : pl.t) {
        CHECK(p.offset % 4 == 0 && p.offset >= end, "%s overlaps its predecessor", p.name.c_str());
        end = p.offset + (size_t)p.rows * p.cols;
    }
    CHECK(end <= pl.total && pl.total - end < 4, "total %zu vs end %zu", pl.total, end);
    CHECK(pl.t[pl.trunk_w[5]].cols == 319 && pl.t[pl.t_w[0]].cols == 260 && pl.t[pl.emb].rows == n_img && pl.t[pl.rad].cols == 9, "shapes");
    for (int bf16 = 0; bf16 < 2; ++bf16) {
        const std::string tag = std::string(bf16 ? "bf16" : "fp32") + " n_img=" + std::to_string(n_img);
        check_stream(("fwd full " + tag).c_str(), build_fwd_stream(pl, bf16, true), pl, true);
        check_stream(("fwd dens " + tag).c_str(), build_fwd_stream(pl, bf16, false), pl, true);
        check_stream(("bwd full " + tag).c_str(), build_bwd_stream(pl, bf16, true, false), pl, true);
        check_stream(("bwd full ig " + tag).c_str(), build_bwd_stream(pl, bf16, true, true, true), pl, true);
        check_stream(("bwd rgb " + tag).c_str(), build_bwd_stream(pl, bf16, true, false, false), pl, true);
        check_stream(("bwd dens " + tag).c_str(), build_bwd_stream(pl, bf16, false, true), pl, true);
    }
    {   // fp16 x 3 split (inference): hi and lo halves of every unit, same sources
        const PackedStream sf = build_fwd_stream(pl, 2, true), sd = build_fwd_stream(pl, 2, false);
        check_stream("fwd full fp16x3", sf, pl, true);
        check_stream("fwd dens fp16x3", sd, pl, true);
        CHECK(sf.e16.size() == sf.e16lo.size() && sf.e16.size() == build_fwd_stream(pl, 1, true).e16.size(), "split stream: one hi and one lo entry per bf16-stream element");
        for (size_t k = 0; k < sf.e16.size(); ++k) CHECK(sf.e16lo[k].dst == sf.e16[k].dst + 1024 && sf.e16lo[k].src == sf.e16[k].src, "lo entry %zu", k);
    }
    check_stream("bwd full heads", build_bwd_stream(pl, true, true, false, true, 1), pl, true);
    check_stream("bwd rgb heads", build_bwd_stream(pl, true, true, false, false, 1), pl, true);
    {   // the fold: every element of the folded matrix and bias is a source of the full forward stream exactly once, and of the backward
        // streams (transient head in the graph) exactly once; the bottleneck layer's own weights are a source of NO chain stream
        const PackedStream ff = build_fwd_stream(pl, true, true), bf = build_bwd_stream(pl, true, true, false, true, 1), br = build_bwd_stream(pl, true, true, false, false, 1);
        std::vector<int> nf(FOLD_FLOATS, 0), nb(FOLD_FLOATS, 0), nr(FOLD_FLOATS, 0);
        const size_t bot_lo = pl.t[pl.bot_w].offset, bot_hi = pl.t[pl.bot_b].offset + 256;
        auto count = [&](const PackedStream& st, std::vector<int>& n) {
            for (const std::vector<PackEntry>* e : {&st.e16, &st.e32})
                for (const PackEntry& pe : *e) {
                    if (pe.src >= (int)pl.total) n[pe.src - pl.total]++;
                    CHECK(pe.src < 0 || (size_t)pe.src < bot_lo || (size_t)pe.src >= bot_hi, "bottleneck weight %d is a source of a chain stream", pe.src);
                }
        };
        count(ff, nf); count(bf, nb); count(br, nr);
        for (int k = 0; k < FOLD_FLOATS; ++k) {
            const bool bias = k >= 256 * 256, albedo = bias ? k - 256 * 256 < 128 : k < 128 * 256;
            CHECK(nf[k] == 1, "fold element %d: %d sources in the forward stream", k, nf[k]);
            CHECK(nb[k] == (bias ? 0 : 1), "fold element %d: %d sources in the backward stream", k, nb[k]);
            CHECK(nr[k] == ((bias || !albedo) ? 0 : 1), "fold element %d: %d sources in the rgb backward stream", k, nr[k]);
        }
    }
    check_stream("bwd dens heads", build_bwd_stream(pl, true, false, true, false, 1), pl, true);
    const PackedStream pw = build_pipe_stream(pl), iw = build_ig_tail_stream(pl);
    check_stream("pipe W^T", pw, pl, false);
    check_stream("ig tail W^T", iw, pl, false);
    CHECK(pw.bytes == (size_t)PIPE_STAGES * 8 * 16 * 1024, "pipe stream size");
    for (int s = 0; s < 64; ++s) {
        const int c16 = enc_col_of_slot(true, s), c32 = enc_col_of_slot(false, s);
        CHECK(c16 >= -1 && c16 < 63 && c32 >= -1 && c32 < 63, "encoding slot %d -> %d / %d", s, c16, c32);
    }
}

struct Span { const char* name; size_t lo, hi; };
static void add(std::vector<Span>& v, const char* name, const void* p, size_t bytes, const uint8_t* base) {
    if (p) v.push_back(Span{name, (size_t)(reinterpret_cast<const uint8_t*>(p) - base), (size_t)(reinterpret_cast<const uint8_t*>(p) - base) + bytes});
}
static void add_pass(std::vector<Span>& v, const PassBuffers& b, int n_rays, size_t p_cap, bool full, int ab, const uint8_t* base) {
    add(v, "counts", b.counts, 4 * (size_t)n_rays, base); add(v, "offsets", b.offsets, 4 * (size_t)(n_rays + 1), base); add(v, "n_pts", b.n_pts, 16, base);
    add(v, "px", b.px, 4 * p_cap, base); add(v, "py", b.py, 4 * p_cap, base); add(v, "pz", b.pz, 4 * p_cap, base);
    add(v, "tmid", b.tmid, 4 * p_cap, base); add(v, "delta", b.delta, 4 * p_cap, base); add(v, "simg", b.simg, 4 * p_cap, base);
    add(v, "sigma", b.sigma, 4 * p_cap, base); add(v, "albedo", b.albedo, 12 * p_cap, base); add(v, "ts", b.ts, 4 * p_cap, base); add(v, "tb", b.tb, 4 * p_cap, base);
    add(v, "act", b.act, (size_t)(full ? ACT_ROWS_FULL : ACT_ROWS_DENSITY) * p_cap * ab, base);
    add(v, "grd", b.grd, (size_t)(full ? GRD_ROWS_FULL : GRD_ROWS_DENSITY) * p_cap * ab, base);
    add(v, "masks", b.masks, (size_t)(full ? MASK_SLOTS_FULL : MASK_SLOTS_DENSITY) * p_cap * 32, base);
    add(v, "g_sigma", b.g_sigma, 4 * p_cap, base); add(v, "g_albedo", b.g_albedo, 12 * p_cap, base); add(v, "g_ts", b.g_ts, 4 * p_cap, base);
    add(v, "g_tb", b.g_tb, 4 * p_cap, base); add(v, "g_emb", b.g_emb, 16 * p_cap, base); add(v, "g_pos", b.g_pos, 12 * p_cap, base);
}

// 256-byte alignment, no two spans overlapping, every span inside the reported size
static void check_spans(std::vector<Span>& v, size_t bytes) {
    std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    for (size_t i = 0; i < v.size(); ++i) {
        CHECK(v[i].lo % 256 == 0, "%s not 256-byte aligned", v[i].name);
        CHECK(v[i].hi <= bytes, "%s ends at %zu beyond the workspace (%zu)", v[i].name, v[i].hi, bytes);
        if (i + 1 < v.size()) CHECK(v[i].hi <= v[i + 1].lo, "%s overlaps %s", v[i].name, v[i + 1].name);
    }
}

// include/eonerf_layout.h: entry k of the table against the carve's own pointer (null: the layout has no such buffer)
static void check_layout_pass(const char* what, const uint64_t* t, const PassBuffers& b, const uint8_t* base) {
    const void* m[EONERF_PASS_MEMBERS] = {b.counts, b.offsets, b.n_pts, b.px, b.py, b.pz, b.tmid, b.delta, b.sigma, b.albedo, b.ts, b.tb, b.simg,
                                          b.act, b.grd, b.masks, b.g_sigma, b.g_albedo, b.g_ts, b.g_tb, b.g_emb, b.g_pos};
    static_assert(EONERF_PASS_G_POS == 21 && EONERF_PASS_ACT == 13 && EONERF_PASS_SIMG == 12, "documented order of the pass members");
    for (int k = 0; k < EONERF_PASS_MEMBERS; ++k) {
        const uint64_t want = m[k] ? (uint64_t)(reinterpret_cast<const uint8_t*>(m[k]) - base) : UINT64_MAX;
        CHECK(t[k] == want, "%s member %d: layout query %llu, carve %llu", what, k, (unsigned long long)t[k], (unsigned long long)want);
    }
}
static uint64_t off_or_none(const void* p, const uint8_t* base) { return p ? (uint64_t)(reinterpret_cast<const uint8_t*>(p) - base) : UINT64_MAX; }

static void check_carve(const CarveCfg& cfg, int n_rays, int flags) {
    const RenderWs m = carve_render(cfg, nullptr, n_rays, flags);                 // measuring pass
    // a fake, never dereferenced base: only differences of pointers are formed
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
    const RenderWs w = carve_render(cfg, base, n_rays, flags);
    CHECK(w.bytes == m.bytes, "measuring pass %zu != carving pass %zu", m.bytes, w.bytes);
    const size_t p_cap = (size_t)p_cap_of(n_rays, cfg.n_samples);
    const bool od = flags & EONERF_F_ONLY_DEPTH;
    const int ab = cfg.bf16 ? 2 : 4;
    std::vector<Span> v;
    add(v, "cnt_first", w.cnt_first, 4 * (size_t)n_rays, base); add(v, "cnt_retry", w.cnt_retry, 4 * (size_t)n_rays, base); add(v, "flags", w.flags, 16, base);
    add(v, "ray_rec", w.ray_rec, 4 * (size_t)n_rays * RAY_REC, base); add(v, "g_ray", w.g_ray, 4 * (size_t)n_rays * RAY_REC, base);
    add(v, "amb_save", w.amb_save, 4 * (size_t)n_rays * 160, base);
    add(v, "m_bott+queue", w.m_bott, 4 * (BOTT_SCRATCH_F + 64), base);
    if (w.pipe.sync) {
        add(v, "sync", w.pipe.sync, PIPE_LAUNCHES * w.pipe.sync_bytes, base);
        add(v, "dy_in", w.pipe.dy_in, p_cap * 512, base);
        const size_t edges = (size_t)cfg.n_pipes * (PIPE_STAGES - 1);
        add(v, "rings", w.pipe.rings, edges * PIPE_RING * PIPE_UNIT_B, base);
        // the ONE memset of a backward call runs from m_bott to the end of the sync blocks: they must be adjacent
        CHECK(reinterpret_cast<uint8_t*>(w.pipe.sync) >= reinterpret_cast<uint8_t*>(w.m_bott) + 4 * (BOTT_SCRATCH_F + 64) &&
              reinterpret_cast<uint8_t*>(w.pipe.sync) - (reinterpret_cast<uint8_t*>(w.m_bott) + 4 * (BOTT_SCRATCH_F + 64)) < 256, "sync block not behind the GEMM queue");
        const size_t wgs = (size_t)cfg.n_pipes * PIPE_STAGES;
        CHECK(w.pipe.sync_bytes >= (64 + wgs * 32 + edges * 64) * 4, "sync block too small");
    }
    add(v, "pipe_part", w.det.pipe_part, (size_t)cfg.n_pipes * PIPE_STAGES * WGRAD_PART_F * 4, base);
    add(v, "wgrad_part", w.det.wgrad_part, (size_t)WGRAD_MAX_JOBS * 48 * WGRAD_PART_F * 4, base);
    add(v, "rad_rays", w.det.rad_rays, 24 * (size_t)n_rays, base); add(v, "emb_rays", w.det.emb_rays, 16 * (size_t)n_rays, base);
    add(v, "enc_part", w.enc_part, 4 * (size_t)cfg.enc_part_wgs * ENC_PART_F, base);
    add_pass(v, w.cam, n_rays, p_cap, !od, ab, base);
    add_pass(v, w.sun, n_rays, p_cap, false, ab, base);
    check_spans(v, w.bytes);
    const bool train = flags & EONERF_F_TRAIN;
    CHECK(p_cap % 256 == 0 && p_cap >= 256 && p_cap >= (size_t)n_rays * (cfg.n_samples - 1), "p_cap %zu for %d rays x %d samples", p_cap, n_rays, cfg.n_samples);
    CHECK((w.cam.act != nullptr) == train && (w.g_ray != nullptr) == train, "training buffers");
    CHECK((w.cam.g_pos != nullptr) == (train && od), "input-gradient buffer of a density-only training pass");
    CHECK((w.sun.px != nullptr) == ((flags & EONERF_F_SHADOWS) && !od), "sun pass buffers");
    CHECK((w.enc_part != nullptr) == (train && (flags & EONERF_F_SHADOWS) && !od && cfg.pipe && cfg.enc_part_wgs > 0), "encoding partials");
    // the layout query reports exactly this carve
    uint64_t t[EONERF_LAYOUT_ENTRIES + 1];
    t[EONERF_LAYOUT_ENTRIES] = 0x5a5a5a5a5a5a5a5aull;
    CHECK(workspace_layout_table(cfg, EONERF_LAYOUT_RENDER, n_rays, flags, t, EONERF_LAYOUT_ENTRIES) == EONERF_LAYOUT_ENTRIES, "layout query refused");
    CHECK(t[EONERF_LAYOUT_ENTRIES] == 0x5a5a5a5a5a5a5a5aull, "layout query wrote beyond its table");
    CHECK(t[EONERF_LAYOUT_P_CAP] == p_cap && t[EONERF_LAYOUT_BYTES] == w.bytes, "layout query: p_cap %llu bytes %llu", (unsigned long long)t[0], (unsigned long long)t[1]);
    CHECK(t[EONERF_LAYOUT_M_BOTT] == off_or_none(w.m_bott, base) && t[EONERF_LAYOUT_DY_IN] == off_or_none(w.pipe.dy_in, base) &&
          t[EONERF_LAYOUT_ENC_PART] == off_or_none(w.enc_part, base), "layout query: m_bott / dy_in / enc_part");
    check_layout_pass("render cam", t + EONERF_LAYOUT_CAM, w.cam, base);
    check_layout_pass("render sun", t + EONERF_LAYOUT_SUN, w.sun, base);
    for (int k = 0; k < EONERF_LAYOUT_ENTRIES; ++k)
        if (k != EONERF_LAYOUT_P_CAP && k != EONERF_LAYOUT_BYTES && t[k] != UINT64_MAX) CHECK(t[k] % 256 == 0 && t[k] < w.bytes, "layout entry %d = %llu", k, (unsigned long long)t[k]);
    // ... and the per-ray query the buffers in front of the passes
    uint64_t q[EONERF_RAY_ENTRIES + 1];
    q[EONERF_RAY_ENTRIES] = 0x5a5a5a5a5a5a5a5aull;
    CHECK(ray_layout_table(cfg, n_rays, flags, q, EONERF_RAY_ENTRIES) == EONERF_RAY_ENTRIES, "ray layout query refused");
    CHECK(q[EONERF_RAY_ENTRIES] == 0x5a5a5a5a5a5a5a5aull, "ray layout query wrote beyond its table");
    static_assert(EONERF_RAY_ENTRIES == 8 && EONERF_RAY_REC == 3 && EONERF_RAY_EMB_RAYS == 7, "documented order of the per-ray buffers");
    const void* rm[EONERF_RAY_ENTRIES] = {w.cnt_first, w.cnt_retry, w.flags, w.ray_rec, w.g_ray, w.amb_save, w.det.rad_rays, w.det.emb_rays};
    for (int k = 0; k < EONERF_RAY_ENTRIES; ++k) {
        CHECK(q[k] == off_or_none(rm[k], base), "ray layout entry %d: query %llu, carve %llu", k, (unsigned long long)q[k], (unsigned long long)off_or_none(rm[k], base));
        if (q[k] != UINT64_MAX) CHECK(q[k] % 256 == 0 && q[k] < w.bytes, "ray layout entry %d = %llu", k, (unsigned long long)q[k]);
    }
    CHECK((q[EONERF_RAY_G_RAY] != UINT64_MAX) == train && (q[EONERF_RAY_AMB_SAVE] != UINT64_MAX) == train &&
          (q[EONERF_RAY_RAD_RAYS] != UINT64_MAX) == (train && cfg.deterministic) && (q[EONERF_RAY_EMB_RAYS] != UINT64_MAX) == (train && cfg.deterministic),
          "ray layout query: training / deterministic buffers");
}

// eonerf_field_forward / eonerf_query_density (carve_field) and eonerf_field_forward_train / eonerf_field_backward (carve_field_train)
static void check_carve_field(const CarveCfg& cfg, int n) {
    const size_t p_cap = (size_t)field_p_cap_of(n);
    CHECK(p_cap % 256 == 0 && p_cap >= 256 && p_cap >= (size_t)n && p_cap < (size_t)std::max(n, 1) + 256, "field p_cap %zu for %d points", p_cap, n);
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
    const int ab = cfg.bf16 ? 2 : 4;
    {
        const FieldWs m = carve_field(cfg, nullptr, (int)p_cap), w = carve_field(cfg, base, (int)p_cap);
        CHECK(w.bytes == m.bytes, "field: measuring pass %zu != carving pass %zu", m.bytes, w.bytes);
        std::vector<Span> v;
        add_pass(v, w.b, 1, p_cap, true, ab, base);
        check_spans(v, w.bytes);
        CHECK(w.b.albedo && w.b.ts && w.b.tb && !w.b.act && !w.b.grd && !w.b.masks && !w.b.g_pos, "field inference buffers");
    }
    for (int density_only = 0; density_only < 2; ++density_only) {
        const bool full = !density_only;
        const FieldTrainWs m = carve_field_train(cfg, nullptr, (int)p_cap, full), w = carve_field_train(cfg, base, (int)p_cap, full);
        CHECK(w.bytes == m.bytes, "field train: measuring pass %zu != carving pass %zu", m.bytes, w.bytes);
        std::vector<Span> v;
        add_pass(v, w.b, 1, p_cap, full, ab, base);
        add(v, "m_bott", w.m_bott, 4 * (size_t)BOTT_SCRATCH_F, base);
        add(v, "queue", w.queue, 16, base);
        check_spans(v, w.bytes);
        CHECK(w.b.act && w.b.grd && w.b.masks && w.b.g_sigma && w.b.g_pos && w.m_bott && w.queue, "field training buffers");
        CHECK((w.b.albedo != nullptr) == full && (w.b.g_albedo != nullptr) == full && (w.b.g_emb != nullptr) == full, "field head buffers");
        CHECK(w.bytes > carve_field(cfg, nullptr, (int)p_cap).bytes || !full, "a training layout holds the inference layout and more");
        uint64_t t[EONERF_LAYOUT_ENTRIES];
        CHECK(workspace_layout_table(cfg, EONERF_LAYOUT_FIELD_TRAIN, n, density_only, t, EONERF_LAYOUT_ENTRIES) == EONERF_LAYOUT_ENTRIES, "field layout query refused");
        CHECK(t[EONERF_LAYOUT_P_CAP] == p_cap && t[EONERF_LAYOUT_BYTES] == w.bytes && t[EONERF_LAYOUT_M_BOTT] == off_or_none(w.m_bott, base), "field layout query: p_cap / bytes / m_bott");
        CHECK(t[EONERF_LAYOUT_DY_IN] == UINT64_MAX && t[EONERF_LAYOUT_ENC_PART] == UINT64_MAX, "field layout query: buffers of the render path");
        check_layout_pass("field train", t + EONERF_LAYOUT_CAM, w.b, base);
        for (int k = 0; k < EONERF_PASS_MEMBERS; ++k) CHECK(t[EONERF_LAYOUT_SUN + k] == UINT64_MAX, "field layout query: sun pass member %d", k);
    }
}

// ---- weight-gradient job planner (eonerf_wgrad_plan.h) ----
// the slab block an operand address starts in and its first row, decoded from the block-major layout ([block][sample tile][row][SEG_B],
// eonerf_common.h) independently of the planner; needs n_tiles >= the largest block (256 rows)
template <class Map> static bool operand_rows(const void* p, const void* slab, size_t n_tiles, int slab_rows, int rows, uint32_t stride, const char* what) {
    const size_t off = (size_t)(reinterpret_cast<const uint8_t*>(p) - reinterpret_cast<const uint8_t*>(slab));
    CHECK(p && slab && off % SEG_B == 0, "%s: operand not on a segment", what);
    const size_t q = off / SEG_B;
    for (int r = 0; r < slab_rows; r += Map::block(r).r) {
        const SlabBlk blk = Map::block(r);
        if (q < (size_t)blk.s * n_tiles || q >= (size_t)blk.s * n_tiles + blk.r) continue;
        const int row0 = blk.s + (int)(q - (size_t)blk.s * n_tiles);
        CHECK(row0 + rows <= blk.s + blk.r && blk.s + blk.r <= slab_rows, "%s: rows %d..%d leave block [%d, %d) of a %d-row slab", what, row0, row0 + rows, blk.s, blk.s + blk.r, slab_rows);
        CHECK(stride == (uint32_t)(blk.r * SEG_B), "%s: tile stride %u of a %d-row block", what, stride, blk.r);
        return true;
    }
    CHECK(false, "%s: operand at segment %zu is in no block of the slab", what, q);
    return false;
}

struct PlanCase { bool bf16, pipelined; int state; bool riders, det, enc_done; int n_cu; };      // state: 0 full + transient, 1 full rgb, 2 density only, 3 full + sun
static int check_wgrad_plan(const PlanCase& pc, const ParamLayout& pl) {
    char tag[160];
    snprintf(tag, sizeof(tag), "plan %s %s state %d riders %d det %d enc_done %d n_cu %d", pc.bf16 ? "bf16" : "fp32", pc.pipelined ? "pipe" : "gemm", pc.state,
             pc.riders, pc.det, pc.enc_done, pc.n_cu);
    CarveCfg cfg;
    cfg.bf16 = pc.bf16; cfg.pipe = pc.pipelined; cfg.n_pipes = pc.n_cu / PIPE_STAGES; cfg.deterministic = cfg.pipe_partials = pc.det;
    cfg.enc_part_wgs = pc.enc_done ? pc.n_cu : 0;
    const int n_rays = 128, flags = EONERF_F_TRAIN | (pc.state == 3 ? EONERF_F_SHADOWS : 0) | (pc.state == 2 ? EONERF_F_ONLY_DEPTH : 0);
    // fake, never dereferenced bases: the planner only forms addresses
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
    float* d_flat = reinterpret_cast<float*>((uintptr_t)1 << 41);
    const int* colmap = reinterpret_cast<const int*>((uintptr_t)1 << 42);
    const RenderWs w = carve_render(cfg, base, n_rays, flags);
    const int p_cap = p_cap_of(n_rays, cfg.n_samples);
    const size_t n_tiles = (size_t)p_cap / (pc.bf16 ? 32 : 16);
    CHECK(n_tiles >= 256, "%s: too few sample tiles to decode a block", tag);
    const PassBuffers* full = pc.state == 2 ? nullptr : &w.cam;
    const PassBuffers* dens = pc.state == 2 ? &w.cam : pc.state == 3 ? &w.sun : nullptr;
    WgradPlanOpts o;      // as camera_backward sets them (eonerf_render.hip); the chain + GEMM cases are eonerf_field_backward's as well
    o.transient = pc.state != 1;
    o.full_trunk_done = pc.pipelined; o.dens_trunk_done = pc.pipelined && dens; o.dens_enc_done = pc.enc_done; o.zeroed = pc.pipelined;
    o.riders = pc.riders; o.deterministic = pc.det;
    WgradJobTable tab;
    memset(&tab, 0xff, sizeof(tab));
    const bool ok = wgrad_plan(tab, full, dens, pc.bf16, p_cap, pc.n_cu, d_flat, pl, colmap, w.m_bott, o);
    CHECK(ok && tab.n >= 1 && tab.n <= WGRAD_MAX_JOBS, "%s: %d jobs", tag, tab.n);
    if (!ok || tab.n < 1 || tab.n > WGRAD_MAX_JOBS) return 0;
    int items = 0, bott_job = -1;
    for (int k = 0; k < tab.n; ++k) {
        const WgradJob& j = tab.j[k];
        CHECK(j.item0 == items && j.slices >= 1, "%s job %d: item0 %d after %d items, %d slices", tag, k, j.item0, items, j.slices);
        if (pc.det) CHECK(j.slices <= 48, "%s job %d: %d slices in deterministic mode", tag, k, j.slices);
        items += j.slices;
        CHECK(j.gm * j.wm * 32 >= j.m_rows && j.gn * j.wn * 32 >= j.n_rows && j.m_rows >= 1 && j.n_rows >= 1, "%s job %d: (%d x %d x 32) x (%d x %d x 32) waves for %d x %d", tag, k, j.gm, j.wm, j.gn, j.wn, j.m_rows, j.n_rows);
        const bool of_full = full && j.n_pts == full->n_pts;
        CHECK(of_full || (dens && j.n_pts == dens->n_pts), "%s job %d: sample count of no pass", tag, k);
        const PassBuffers& b = of_full ? *full : *dens;
        operand_rows<GrdMap>(j.a, b.grd, n_tiles, of_full ? GRD_ROWS_FULL : GRD_ROWS_DENSITY, j.m_rows, j.a_stride, tag);
        operand_rows<ActMap>(j.b, b.act, n_tiles, of_full ? ACT_ROWS_FULL : ACT_ROWS_DENSITY, j.n_rows, j.b_stride, tag);
        const bool to_scratch = j.dw >= w.m_bott && j.dw < w.m_bott + BOTT_SCRATCH_F;
        CHECK(to_scratch || (j.dw >= d_flat && j.dw + (size_t)(j.split - 1) * j.dw_ld < d_flat + pl.total), "%s job %d: destination outside the gradient buffer", tag, k);
        CHECK((j.split == j.m_rows) == (j.dw2 == nullptr) && j.split >= 1 && j.split <= j.m_rows, "%s job %d: split %d of %d rows", tag, k, j.split, j.m_rows);
        CHECK(j.a_units == ((pc.pipelined && j.n_rows == 64) ? 1 : 0), "%s job %d: a_units %d", tag, k, j.a_units);      // only dY_0 / dY_5 are left in unit order
        if (to_scratch) { CHECK(bott_job < 0 && j.dw == w.m_bott, "%s: two bottleneck-factor jobs", tag); bott_job = k; }
    }
    CHECK(tab.items == items, "%s: %d items, slices sum to %d", tag, tab.items, items);
    if (pc.det) CHECK(tab.items <= WGRAD_MAX_JOBS * 48, "%s: %d items beyond the partial buffer", tag, tab.items);
    CHECK((bott_job >= 0) == (full != nullptr), "%s: bottleneck-factor job %d", tag, bott_job);
    const bool riders = full && pc.riders && !pc.det;
    CHECK(tab.aux.job == (riders ? bott_job : -1), "%s: riders on job %d, bottleneck-factor job %d", tag, tab.aux.job, bott_job);
    if (riders) {
        operand_rows<GrdMap>(tab.aux.a2, full->grd, n_tiles, GRD_ROWS_FULL, 1, tab.aux.a2_stride, tag);
        CHECK((tab.aux.b2 != nullptr) == o.transient, "%s: embedding rider", tag);
        if (tab.aux.b2) operand_rows<ActMap>(tab.aux.b2, full->act, n_tiles, ACT_ROWS_FULL, 4, tab.aux.b2_stride, tag);
    }
    return tab.n;
}

static void check_wgrad_plans() {
    ParamLayout pl;
    pl.build(20);
    int most = 0;
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int pipelined = 0; pipelined <= bf16; ++pipelined)          // the pipelined backward is a bf16 path
            for (int state = 0; state < 4; ++state)
                for (int riders = 0; riders < 2; ++riders)
                    for (int det = 0; det < 2; ++det)
                        for (int enc_done = 0; enc_done <= (pipelined && state == 3 && !det ? 1 : 0); ++enc_done)      // eonerf_enc_pair.hip: shadow pass, pipelined, atomic mode
                            for (int n_cu : {256, 64, 7}) {
                                const PlanCase pc{bf16 != 0, pipelined != 0, state, riders != 0, det != 0, enc_done != 0, n_cu};
                                const int n = check_wgrad_plan(pc, pl);
                                most = std::max(most, n);
                                // anchors: the default bf16 states of the training step
                                if (bf16 && pipelined && riders && !det && state == 1) CHECK(n == 4, "rgb state plans %d jobs", n);
                                if (bf16 && pipelined && riders && !det && state == 3 && enc_done) CHECK(n == 9, "full step plans %d jobs", n);
                            }
    CHECK(most <= 31, "largest table: %d jobs", most);
    printf("wgrad plans: at most %d jobs\n", most);
}

int main() {
    for (int n_img : {1, 19, 20, 2048}) check_layout(n_img);
    CarveCfg cfgs[7];
    cfgs[0].bf16 = false;
    cfgs[1].pipe = true; cfgs[1].n_pipes = 36;
    cfgs[2] = cfgs[1]; cfgs[2].pipe_partials = true;
    cfgs[3] = cfgs[1]; cfgs[3].deterministic = cfgs[3].pipe_partials = true;
    cfgs[4] = cfgs[1]; cfgs[4].n_pipes = 1;
    cfgs[5] = cfgs[1]; cfgs[5].enc_part_wgs = 256;      // what a context on the pipelined path carves by default: one partial per CU (eonerf_enc_pair.hip)
    cfgs[6] = cfgs[4]; cfgs[6].enc_part_wgs = 1;
    // (EONERF_F_TRAIN | EONERF_F_ONLY_DEPTH: the layout of eonerf_rendering_train(depth_only) / eonerf_rendering_backward)
    const int flag_sets[] = {0, EONERF_F_SHADOWS, EONERF_F_ONLY_DEPTH, EONERF_F_TRAIN | EONERF_F_RGB_LOSS, EONERF_F_TRAIN | EONERF_F_SHADOWS,
                             EONERF_F_SHADOWS | EONERF_F_EVAL, EONERF_F_TRAIN | EONERF_F_SHADOWS | EONERF_F_EVAL, EONERF_F_TRAIN | EONERF_F_ONLY_DEPTH,
                             EONERF_F_TRAIN};
    for (const CarveCfg& c : cfgs)
        for (int n_rays : {1, 37, 4096, 66050})
            for (int f : flag_sets) check_carve(c, n_rays, f);
    // the other step sizes (eonerf_set_n_samples)
    // (version 502 admits 2 .. 256: n_samples = 2 leaves ONE interval per ray, the smallest p_cap_of)
    for (int ns : {2, 3, 37, 64, 255, 256})
        for (const CarveCfg& c0 : {cfgs[0], cfgs[1], cfgs[3], cfgs[5]}) {
            CarveCfg c = c0;
            c.n_samples = ns;
            for (int n_rays : {1, 37, 300, 4096, 16384})
                for (int f : flag_sets) check_carve(c, n_rays, f);
        }
    CHECK(p_cap_of(1, 2) == 256 && p_cap_of(256, 2) == 256 && p_cap_of(257, 2) == 512 && p_cap_of(0, 2) == 256 && p_cap_of(300, 255) == 76288, "p_cap_of corners");
    // the field entry points: one pass over round_up(n, 256) points, whatever the render configuration of the context
    for (const CarveCfg& c : {cfgs[0], cfgs[1], cfgs[3], cfgs[5]})
        for (int n : {0, 1, 255, 256, 257, 1000, 2097152}) check_carve_field(c, n);
    CHECK(slab_blocks_addressable(true, (size_t)p_cap_of(66050, 128)) && !slab_blocks_addressable(true, (size_t)p_cap_of(66051, 128)), "bf16 size guard");
    CHECK(slab_blocks_addressable(false, (size_t)p_cap_of(33024, 128)) && !slab_blocks_addressable(false, (size_t)p_cap_of(33025, 128)), "fp32 size guard");
    {   // the layout query's refusals leave the table alone
        uint64_t t[EONERF_LAYOUT_ENTRIES] = {7};
        CHECK(workspace_layout_table(cfgs[1], EONERF_LAYOUT_RENDER, 37, EONERF_F_TRAIN, t, EONERF_LAYOUT_ENTRIES - 1) == EONERF_E_ARG && t[0] == 7, "short table");
        CHECK(workspace_layout_table(cfgs[1], 2, 37, 0, t, EONERF_LAYOUT_ENTRIES) == EONERF_E_ARG && t[0] == 7, "unknown kind");
        CHECK(workspace_layout_table(cfgs[1], EONERF_LAYOUT_FIELD_TRAIN, -1, 0, t, EONERF_LAYOUT_ENTRIES) == EONERF_E_ARG && t[0] == 7, "negative n");
        CHECK(workspace_layout_table(cfgs[1], EONERF_LAYOUT_RENDER, 37, 0, nullptr, EONERF_LAYOUT_ENTRIES) == EONERF_E_ARG, "null table");
        uint64_t q[EONERF_RAY_ENTRIES] = {7};
        CHECK(ray_layout_table(cfgs[1], 37, EONERF_F_TRAIN, q, EONERF_RAY_ENTRIES - 1) == EONERF_E_ARG && q[0] == 7, "ray layout: short table");
        CHECK(ray_layout_table(cfgs[1], -1, 0, q, EONERF_RAY_ENTRIES) == EONERF_E_ARG && q[0] == 7, "ray layout: negative n");
        CHECK(ray_layout_table(cfgs[1], 37, 0, nullptr, EONERF_RAY_ENTRIES) == EONERF_E_ARG, "ray layout: null table");
    }
    check_wgrad_plans();
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("host checks ok\n");
    return 0;
}
