// The tables behind eonerf_workspace_layout and eonerf_ray_layout (include/eonerf_layout.h): plain host code, no HIP runtime calls -- shared by the entry points
// (eonerf_field.hip) and the host-only test (tests/host/host_checks.cpp), which holds every entry to the carve's own pointers.
// The offsets are read off the carve itself: carve_field_train / carve_render on a base that is never dereferenced, minus that base
// (a null base is the carve's MEASURING mode and hands out null pointers only, so the base here is a fake non-null one, as in the host test).
#pragma once
#include "../../include/eonerf_layout.h"
#include "eonerf_carve.h"

inline void layout_pass(const PassBuffers& b, const uint8_t* base, uint64_t* out) {
    const void* m[EONERF_PASS_MEMBERS] = {b.counts, b.offsets, b.n_pts, b.px, b.py, b.pz, b.tmid, b.delta, b.sigma, b.albedo, b.ts, b.tb, b.simg,
                                          b.act, b.grd, b.masks, b.g_sigma, b.g_albedo, b.g_ts, b.g_tb, b.g_emb, b.g_pos};
    for (int k = 0; k < EONERF_PASS_MEMBERS; ++k) out[k] = m[k] ? (uint64_t)(reinterpret_cast<const uint8_t*>(m[k]) - base) : UINT64_MAX;
}

inline int workspace_layout_table(const CarveCfg& cfg, int kind, int n, int flags, uint64_t* out, int cap) {
    if (!out || n < 0 || cap < EONERF_LAYOUT_ENTRIES || (kind != EONERF_LAYOUT_FIELD_TRAIN && kind != EONERF_LAYOUT_RENDER)) return EONERF_E_ARG;
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
    auto off = [&](const void* p) { return p ? (uint64_t)(reinterpret_cast<const uint8_t*>(p) - base) : UINT64_MAX; };
    for (int k = 0; k < EONERF_LAYOUT_ENTRIES; ++k) out[k] = UINT64_MAX;
    if (kind == EONERF_LAYOUT_FIELD_TRAIN) {
        const int p_cap = field_p_cap_of(n);
        const FieldTrainWs w = carve_field_train(cfg, base, p_cap, !(flags & 1));
        out[EONERF_LAYOUT_P_CAP] = (uint64_t)p_cap; out[EONERF_LAYOUT_BYTES] = w.bytes;
        out[EONERF_LAYOUT_M_BOTT] = off(w.m_bott);
        layout_pass(w.b, base, out + EONERF_LAYOUT_CAM);
    } else {
        const RenderWs w = carve_render(cfg, base, n, flags);
        out[EONERF_LAYOUT_P_CAP] = (uint64_t)p_cap_of(n, cfg.n_samples); out[EONERF_LAYOUT_BYTES] = w.bytes;
        out[EONERF_LAYOUT_M_BOTT] = off(w.m_bott); out[EONERF_LAYOUT_DY_IN] = off(w.pipe.dy_in); out[EONERF_LAYOUT_ENC_PART] = off(w.enc_part);
        layout_pass(w.cam, base, out + EONERF_LAYOUT_CAM);
        layout_pass(w.sun, base, out + EONERF_LAYOUT_SUN);
    }
    return EONERF_LAYOUT_ENTRIES;
}

// The table behind eonerf_ray_layout: the per-ray buffers carve_render puts in front of the passes
inline int ray_layout_table(const CarveCfg& cfg, int n_rays, int flags, uint64_t* out, int cap) {
    if (!out || n_rays < 0 || cap < EONERF_RAY_ENTRIES) return EONERF_E_ARG;
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 40);
    const RenderWs w = carve_render(cfg, base, n_rays, flags);
    const void* m[EONERF_RAY_ENTRIES] = {w.cnt_first, w.cnt_retry, w.flags, w.ray_rec, w.g_ray, w.amb_save, w.det.rad_rays, w.det.emb_rays};
    for (int k = 0; k < EONERF_RAY_ENTRIES; ++k) out[k] = m[k] ? (uint64_t)(reinterpret_cast<const uint8_t*>(m[k]) - base) : UINT64_MAX;
    return EONERF_RAY_ENTRIES;
}
