// Job table and slice plan of the weight-gradient GEMM launch (eonerf_wgrad.hip): plain host code, no HIP runtime calls -- shared by
// eo_run_weight_gradients (eonerf_render.hip) and the host-only sanitizer test (tests/host/host_checks.cpp), which enumerates the
// reachable option combinations.  Nothing here is dereferenced: the table only carries addresses.
#pragma once
#include <string.h>
#include <algorithm>
#include "eonerf_kernels.h"
#include "eonerf_pack.h"
#include "eonerf_carve.h"

struct WgradPlanOpts {
    bool transient = true;          // full pass: the transient head is in the graph
    bool full_trunk_done = false;   // layers 1..7 of the full pass were accumulated by the layer-pipelined trunk backward ...
    bool dens_trunk_done = false;   // ... of the density-only pass
    bool dens_enc_done = false;     // the density-only pass' two products against the encoding were formed by eo_launch_enc_pair
    bool riders = true;             // eonerf_ctx::wgrad_riders (in effect with a full pass outside deterministic mode)
    bool deterministic = false;     // the launch stores partials (DetWs::wgrad_part) instead of adding atomically
    bool zeroed = false;            // the bottleneck factors and the work queue are zero already (launch only: the plan does not depend on it)
};

// Weight gradients of up to two MLP passes as jobs of ONE split-K launch:
//   full: a pass through the whole field (camera pass / EONerfMLP.forward), with or without the transient head in the graph;
//   dens: a density-only pass (shadow pass / query_density).  Either may be null.  Gradients are ACCUMULATED into d_flat.
// false: a job did not fit WGRAD_MAX_JOBS (the table is not to be launched).
inline bool wgrad_plan(WgradJobTable& tab, const PassBuffers* full, const PassBuffers* dens, bool bf16, int p_cap, int n_cu, float* d_flat,
                       const ParamLayout& pl, const int* enc_colmap, float* m_bott, const WgradPlanOpts& o) {
    auto dptr = [&](int ti) { return d_flat + pl.t[ti].offset; };
    tab.n = 0; tab.items = 0;
    memset(&tab.aux, 0, sizeof(tab.aux));
    tab.aux.job = -1;
    bool fits = true;
    // riders of the bottleneck-factor job (WgradAux): the sigma row and the embedding columns of the camera pass travel with the job that
    // streams X_8 / dY_T1 anyway.  Not in deterministic mode (its partial-sum tiles have no room for them)
    const bool riders = full && !o.deterministic && o.riders;
    const size_t n_tiles = (size_t)p_cap / (bf16 ? 32 : 16);      // sample tiles of the slabs (block-major layout, eonerf_common.h)
    auto seg0 = [&](const void* slab, SlabBlk blk, int row) {           // (row, sample tile 0)
        return reinterpret_cast<const uint8_t*>(slab) + ((size_t)blk.s * n_tiles + (row - blk.s)) * SEG_B;
    };
    WgradJob spill;      // takes the writes of a job that did not fit
    auto add = [&](const PassBuffers& b, int grd_row, int m_rows, int act_row, int n_rows, float* dw, int dw_ld, float* db,
                   const int* cmap, int gm, int gn, int wm, int wn) -> WgradJob& {
        if (tab.n >= WGRAD_MAX_JOBS) fits = false;
        WgradJob& j = fits ? tab.j[tab.n++] : spill;
        const SlabBlk ba = GrdMap::block(grd_row), bb = ActMap::block(act_row);
        j.a = seg0(b.grd, ba, grd_row); j.b = seg0(b.act, bb, act_row); j.dw = dw; j.db = db; j.col_map = cmap; j.n_pts = b.n_pts;
        j.a_stride = (uint32_t)(ba.r * SEG_B);       // consecutive sample tiles of a block are contiguous
        j.b_stride = (uint32_t)(bb.r * SEG_B);
        j.m_rows = m_rows; j.n_rows = n_rows; j.dw_ld = dw_ld; j.gm = gm; j.gn = gn; j.wm = wm; j.wn = wn;
        j.dw2 = nullptr; j.db2 = nullptr; j.split = m_rows; j.dw2_ld = 0; j.a_units = 0;
        return j;
    };
    // pipelined: the 256 x 256 products of layers 1..7 (and their biases) were accumulated by the layer-pipelined trunk backward;
    // what is left are the two 256 x 64 products against the encoding (layer 0, skip columns of layer 5) and the sigma row
    auto trunk_jobs = [&](const PassBuffers& b, bool pipelined, bool sigma_job, bool enc_jobs) {
        // (pipelined: dY_0 and dY_5 lie in their slab tiles in unit order -- written once by the stages of layers 1 and 6)
        // (enc_jobs = false: the two products against the encoding were formed by eo_launch_enc_pair, with the pass' input-gradient tail)
        if (enc_jobs) add(b, GRD_ROW_Y0, 256, ACT_ROW_ENC, 64, dptr(pl.trunk_w[0]), 63, dptr(pl.trunk_b[0]), enc_colmap, 4, 2, 2, 1).a_units = pipelined;
        for (int l = 1; l < 8; ++l) {
            const int in_ld = l == 5 ? 319 : 256;
            if (!pipelined)
                add(b, GRD_ROW_Y0 + 256 * l, 256, ACT_ROW_X1 + 256 * (l - 1), 256, dptr(pl.trunk_w[l]), in_ld, dptr(pl.trunk_b[l]), nullptr, 2, 4, 4, 2);
            if (l == 5 && enc_jobs)   // skip columns 256..318 <- encoding slots
                add(b, GRD_ROW_Y0 + 256 * 5, 256, ACT_ROW_ENC, 64, dptr(pl.trunk_w[5]) + 256, 319, nullptr, enc_colmap, 4, 2, 2, 1).a_units = pipelined;
        }
        if (sigma_job) add(b, GRD_ROW_SIG, 1, ACT_ROW_X1 + 256 * 7, 256, dptr(pl.sig_w), 256, dptr(pl.sig_b), nullptr, 1, 8, 1, 1);
    };
    if (full) {
        const PassBuffers& c = *full;
        trunk_jobs(c, o.full_trunk_done, !riders, true);
        // bottleneck factors M_a = dA1^T X8 (and M_t = dT1^T X8) + the bias gradients db_A1 (db_T1), finished by eo_launch_bott_wgrad
        // into THREE weight gradients: the bottleneck layer's and the two head layers' that read the bottleneck output (which is
        // therefore never saved by the forward, nor read back here: see BottWgradArgs)
        float* db_at = m_bott + 2 * 128 * 256;
        // dY A1 and dY T1 are the two halves of one 256-row block of the gradient slab: with the transient head both factors are ONE job
        if (o.transient) add(c, GRD_ROW_A1, 256, ACT_ROW_X1 + 256 * 7, 256, m_bott, 256, db_at, nullptr, 2, 4, 4, 2);          // [M_a; M_t], [db_A1; db_T1]
        else add(c, GRD_ROW_A1, 128, ACT_ROW_X1 + 256 * 7, 256, m_bott, 256, db_at, nullptr, 2, 4, 2, 2);
        if (riders) {
            WgradAux& x = tab.aux;
            x.job = tab.n - 1;
            x.a2 = seg0(c.grd, GrdMap::block(GRD_ROW_SIG), GRD_ROW_SIG); x.a2_stride = (uint32_t)(GrdMap::block(GRD_ROW_SIG).r * SEG_B);
            x.dw_sig = dptr(pl.sig_w); x.db_sig = dptr(pl.sig_b);
            if (o.transient) {
                x.b2 = seg0(c.act, ActMap::block(ACT_ROW_EMB), ACT_ROW_EMB); x.b2_stride = (uint32_t)(ActMap::block(ACT_ROW_EMB).r * SEG_B);
                x.dw_emb = dptr(pl.t_w[0]) + 256; x.emb_ld = 260; x.emb_row0 = 128;
            }
        }
        add(c, GRD_ROW_A2, 3, ACT_ROW_A1, 128, dptr(pl.a2_w), 128, dptr(pl.a2_b), nullptr, 1, 4, 1, 1);
        if (o.transient) {
            if (!riders) add(c, GRD_ROW_T1, 128, ACT_ROW_EMB, 4, dptr(pl.t_w[0]) + 256, 260, nullptr, nullptr, 4, 1, 1, 1);
            for (int l = 1; l < 4; ++l)
                add(c, GRD_ROW_T1 + 128 * l, 128, ACT_ROW_T1 + 128 * (l - 1), 128, dptr(pl.t_w[l]), 128, dptr(pl.t_b[l]), nullptr, 2, 4, 2, 1);
            // row 0: d ts_pre, row 1: d tb_pre -- the second row goes to a second layer's gradient
            WgradJob& j = add(c, GRD_ROW_T5, 2, ACT_ROW_T1 + 384, 128, dptr(pl.tsc_w), 128, dptr(pl.tsc_b), nullptr, 1, 4, 1, 1);
            j.split = 1; j.dw2 = dptr(pl.tbe_w); j.dw2_ld = 128; j.db2 = dptr(pl.tbe_b);
        }
    }
    if (dens) trunk_jobs(*dens, o.dens_trunk_done, true, !o.dens_enc_done);
    if (!fits) return false;
    // every work item = one slice of one job's sample range, equal slices for every job; persistent workgroups pull items from one
    // counter.  Since the K loop is instantiated per tile shape the launch is HBM-bound (5.7 TB/s) and an item's time follows the
    // bytes its job moves per K step.  Measured rules (item-count sweeps through a switch removed after commit 38660b0; slices in
    // proportion to the bytes were tried twice and lost to equal slices at every item count):
    //   few jobs (the rgb state: 4): the HEAVY jobs' items (>= 45 % of the heaviest job's bytes per step) fill exactly one round,
    //     just under one item per CU, and the light jobs' items fill the gaps behind them: 0.227-0.238 ms at 288-320 items against
    //     0.26 at 512 and 0.28 at 352 (heavy items spill into a second round)
    //   many jobs (the full state with the pipelined trunk: 11): ~2.5 items per CU: flat (0.472-0.478 ms) from 650 to 830 items,
    //     0.49-0.50 at 512-600 and at 1,024
    double wmax = 0.0, wj[WGRAD_MAX_JOBS];
    for (int k = 0; k < tab.n; ++k) {
        wj[k] = (double)((tab.j[k].m_rows + 15) / 16 * 16 + (tab.j[k].n_rows + 15) / 16 * 16) * SEG_B;
        wmax = std::max(wmax, wj[k]);
    }
    int n_heavy = 0;
    for (int k = 0; k < tab.n; ++k) n_heavy += wj[k] >= 0.45 * wmax ? 1 : 0;
    for (int k = 0; k < tab.n; ++k) {
        WgradJob& j = tab.j[k];
        int fill = (int)(2.54 * n_cu / tab.n + 0.5);
        if (tab.n <= 8) fill = (n_cu - 1) / std::max(n_heavy, 1);
        int sl = tab.n > 16 ? std::max(fill, 48) : std::min(std::max(fill, 1), 256);
        if (o.deterministic && sl > 48) sl = 48;       // the partial buffer holds WGRAD_MAX_JOBS x 48 items
        j.slices = sl < 1 ? 1 : sl;
    }
    for (int k = 0; k < tab.n; ++k) { tab.j[k].item0 = tab.items; tab.items += tab.j[k].slices; }
    return true;
}
