"""CPU: the per-ray checks of tests/ray_checks.py accept a correct workspace and catch each seeded defect at the right check and at no
unrelated one -- a check that cannot fail is worth nothing.

The workspace is synthetic: the fp32 emulation of tests/ray_restated.py (arithmetic F32: the kernels' operations in their own order) run
on random per-sample sigma / albedo / ts / tb -- no MLP -- and laid out by ray_restated.build_image at made-up offsets, then decoded through
the same views the GPU file uses.  Also here, because it needs no GPU: the clip conditions of the GPU cases (both bounds reached, fewer
than 2 % of the rays ambiguous) on the float64 reference alone, for exactly the batches and the state dict the GPU file uses."""
import pytest
import torch

from oracle import eonerf_oracle as orc
import ray_checks as rc
import ray_restated as rr
import slab_checks as sc

F = rr.F32
SEEDS = (7, 61, 62)      # 7: the state dict's seed; 61, 62: batch seeds of the GPU file


def _pass_arrays(g, counts, ns, p_cap, camera):
    """Random per-sample arrays of one pass.  Per ray a density scale: 300 (opaque within a few samples), 1, or 1e-3 (nearly
    transparent); interval lengths around 2 / ns, the camera pass' last one 1e10."""
    R = len(counts)
    cnt = torch.tensor(counts)
    off = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    n = int(off[-1])
    scale = torch.tensor([300.0, 1.0, 1e-3])[torch.arange(R) % 3]
    ray_of = torch.repeat_interleave(torch.arange(R), cnt)
    a = {k: torch.zeros(r, p_cap) for k, r in (("sigma", 1), ("delta", 1), ("tmid", 1), ("albedo", 3), ("ts", 1), ("tb", 1))}
    a["sigma"][0, :n] = torch.rand(n, generator=g) * scale[ray_of]
    a["delta"][0, :n] = (0.5 + torch.rand(n, generator=g)) * (2.0 / ns)
    a["tmid"][0, :n] = torch.rand(n, generator=g) * 2
    a["albedo"][:, :n] = torch.rand(3, n, generator=g)
    a["ts"][0, :n] = torch.rand(n, generator=g)
    a["tb"][0, :n] = torch.rand(n, generator=g) * 0.5
    if camera:
        last = off[1:][cnt > 0] - 1
        a["delta"][0, last] = 1e10
    return cnt, off, n, a


def emulate(ns, seed, shadows=True, kind=1, defect=None, given_d_out=False, deterministic=False):
    k = rr.K()
    g = torch.Generator().manual_seed(seed)
    lst = rc.COUNTS_256 if ns > 128 else ([c for c in rc.COUNTS_128 if c < ns] if ns >= 128 else [0, 1, 2, ns - 2, ns - 1])
    cam_counts = lst + lst[::-1] + [5, 17, 33]
    sun_counts = lst[::-1] + lst + [0, 9, 40]
    R = len(cam_counts)
    p_cap = (R * (ns - 1) + 255) // 256 * 256
    cc, coff, cn, ca = _pass_arrays(g, cam_counts, ns, p_cap, True)
    sc_, soff, sn, sa = _pass_arrays(g, sun_counts, ns, p_cap, False)
    mk = lambda cnt, off, n, a, extra: dict(counts=cnt.int(), offsets=off.int(), n_pts=torch.tensor([n, 0, 0, 0], dtype=torch.int32),      # noqa: E731
                                            **{kk: v.float() for kk, v in a.items()}, **extra)
    nan = lambda *s: torch.full(s, float("nan"))      # noqa: E731
    cam_d = mk(cc, coff, cn, ca, dict(g_sigma=nan(1, p_cap), g_albedo=nan(3, p_cap), g_ts=nan(1, p_cap), g_tb=nan(1, p_cap)))
    sun_d = mk(sc_, soff, sn, {kk: sa[kk] for kk in ("sigma", "delta", "tmid")}, dict(g_sigma=nan(1, p_cap), g_pos=torch.randn(3, p_cap, generator=g))) if shadows else None
    ray_d = dict(cnt_first=cc.int(), cnt_retry=cc.int(), flags=torch.zeros(4, dtype=torch.int32), ray_rec=nan(R, k["RAY_REC"]), g_ray=nan(R, k["RAY_REC"]),
                 amb_save=nan(R, 160))
    if deterministic:
        ray_d["rad_rays"] = nan(R, 6)
    ws, roff, coff_, soff_ = rr.build_image(ray_d, cam_d, sun_d, p_cap)
    rv, cam = rr.RayView(ws, roff, R), rr.PassView(ws, coff_, p_cap, R, ns)
    sun = rr.PassView(ws, soff_, p_cap, R, ns) if shadows else None
    # ---- forward ----
    rays = torch.randn(R, 11, generator=g)
    rays[:, 8:11] = rays[:, 8:11] / rays[:, 8:11].norm(dim=1, keepdim=True)
    img = torch.randint(0, rc.N_IMG, (R,), generator=g)
    amb_t = {"ambient_mlp.hidden_layers.0.weight": torch.randn(128, 27, generator=g) * 0.3, "ambient_mlp.hidden_layers.0.bias": torch.randn(128, generator=g) * 0.1,
             "ambient_mlp.output_layer.weight": torch.randn(3, 128, generator=g) * 0.3, "ambient_mlp.output_layer.bias": torch.randn(3, generator=g) * 0.1}
    table = rc.clip_state_dict()["radiometricT_enc.weight"] + 0.05 * torch.randn(rc.N_IMG, 9, generator=g)
    rec = rv.rec()
    rw = rr.ray_weights(F, cam.dense("sigma"), cam.dense("delta"), cam.mask, defect)
    comp = rr.composite_record(F, rw, cam.dense("tmid"), [cam.dense("albedo", c, 3) for c in range(3)], cam.dense("ts"), cam.dense("tb"), defect=defect)
    for col, v in zip([k["RR_DEPTH"], k["RR_ALB"], k["RR_ALB"] + 1, k["RR_ALB"] + 2, k["RR_TS"], k["RR_TB"], k["RR_WSUM"]], comp):
        rec[:, col] = v
    rec[:, k["RR_GEO"]] = 1.0
    if shadows:
        rws = rr.ray_weights(F, sun.dense("sigma"), sun.dense("delta"), sun.mask)
        rec[:, k["RR_GEO"]] = rr.geo_shadow(F, rws, sun.counts, defect)
    enc = torch.stack(rr.ambient_encoding(F, [rays[:, 8 + d] for d in range(3)]), 1)
    hid = rr.ambient_hidden(F, enc, amb_t["ambient_mlp.hidden_layers.0.weight"], amb_t["ambient_mlp.hidden_layers.0.bias"])
    aout = rr.ambient_out(F, hid, amb_t["ambient_mlp.output_layer.weight"], amb_t["ambient_mlp.output_layer.bias"])
    sv = rv.f32("amb_save", 160)
    sv[:, :27], sv[:, 32:160] = enc, hid
    for o in range(3):
        rec[:, k["RR_AMB"] + o] = aout[o]
    cols = [rec[:, j].clone() for j in range(k["RAY_REC"])]
    tA, tb = [table[img][:, c] for c in range(3)], [table[img][:, 3 + c] for c in range(3)]
    o, _ = rr.shade(F, cols, tA, tb, shadows)
    out = torch.zeros(R, 21)
    for c, v in o.items():
        out[:, c] = v
    out[:, 3], out[:, 4:7], out[:, 10], out[:, 11], out[:, 12] = rec[:, k["RR_DEPTH"]], rec[:, k["RR_ALB"]:k["RR_ALB"] + 3], rec[:, k["RR_GEO"]] if shadows else 1.0, \
        rec[:, k["RR_TS"]], rec[:, k["RR_TB"]]
    out[:, 13], out[:, 14], out[:, 15], out[:, 16], out[:, 17] = 1.0, cc.float(), sun.counts.float() if shadows else 1.0, 1.0, 1.0
    # ---- loss and backward ----
    pix = torch.rand(R, 3, generator=g)
    part, go = rr.loss_terms(F, [out[:, c] for c in range(3)], out[:, 12], [pix[:, c] for c in range(3)], R, kind)
    loss = rr.loss_total(F, part, kind, defect)
    d_out = torch.zeros(R, 21)
    for c, v in go.items():
        d_out[:, c] = v
    if given_d_out:
        d_out = torch.randn(R, 21, generator=g)
        go = {c: d_out[:, c] for c in range(21)}
    gr, rad, _ = rr.shade_bwd(F, cols, go, tA, tb, shadows, defect)
    g_ray = rv.rec("g_ray")
    for col, v in gr.items():
        g_ray[:, col] = v
    radm = torch.stack(rad, 1)
    d_table = torch.zeros(rc.N_IMG, 9)
    if deterministic:
        rv.f32("rad_rays", 6)[:] = radm
        for r in range(R):
            d_table[img[r], :6] += radm[r]
    else:
        d_table[:, :6] = F.index_sum(radm, img, rc.N_IMG)
    gcols = [g_ray[:, j].clone() for j in range(k["RAY_REC"])]
    if shadows:
        sun.flat("g_sigma")[0][sun.idx[sun.mask]] = rr.sun_composite_bwd(F, gcols[k["RR_GEO"]], cols[k["RR_GEO"]], sun.dense("delta"), sun.mask, sun.counts, defect)[sun.mask]
    rwb = rr.ray_weights(F, cam.dense("sigma"), cam.dense("delta"), cam.mask)
    cb = rr.cam_composite_bwd(F, rwb, cam.mask, cam.dense("delta"), cam.dense("tmid"), [cam.dense("albedo", c, 3) for c in range(3)], cam.dense("ts"), cam.dense("tb"),
                              gcols, [rays[:, 3 + d] for d in range(3)] if shadows else None, [sun.dense("g_pos", d, 3) for d in range(3)] if shadows else None,
                              defect=defect)
    sel = cam.idx[cam.mask]
    cam.flat("g_sigma")[0][sel] = cb[0][cam.mask]
    for c in range(3):
        cam.flat("g_albedo", 3)[c][sel] = cb[1][c][cam.mask]
    cam.flat("g_ts")[0][sel], cam.flat("g_tb")[0][sel] = cb[2][cam.mask], cb[3][cam.mask]
    ab = rr.ambient_bwd(F, [gcols[k["RR_AMB"] + o_] for o_ in range(3)], aout, enc, hid, amb_t["ambient_mlp.output_layer.weight"], defect)
    grads = {"ambient_mlp.hidden_layers.0.weight": ab["w1"], "ambient_mlp.hidden_layers.0.bias": ab["b1"], "ambient_mlp.output_layer.weight": ab["w2"],
             "ambient_mlp.output_layer.bias": ab["b2"]}
    return dict(rv=rv, cam=cam, sun=sun, rays=rays, img=img, amb_t=amb_t, table=table, out=out, pix=pix, loss=loss, d_out=d_out, d_table=d_table, grads=grads,
                shadows=shadows, kind=kind, given=given_d_out, R=R)


def run_checks(e):
    """check name -> results, in the order of a training step."""
    res = {"ray record": rc.check_ray_record(e["cam"], e["rv"], geo_is_one=not e["shadows"])}
    if e["shadows"]:
        res["geo"] = rc.check_geo(e["sun"], e["rv"])
    res["ambient head"] = rc.check_ambient_forward(e["rv"], e["rays"], e["amb_t"])
    res["shading"] = rc.check_shade(e["rv"], e["out"], e["table"], e["img"], e["shadows"], e["sun"].counts if e["shadows"] else None)
    if e["given"]:
        go = {c: rr.Ref.inp(e["d_out"][:, c]) for c in range(21)}
    else:
        res["loss"] = rc.check_loss(e["out"], e["pix"], e["kind"], e["loss"], e["d_out"])
        go = rc.loss_reference(e["out"], e["pix"], e["kind"])[1]
    res["shading backward"], amb = rc.check_shade_bwd(e["rv"], e["table"], e["img"], e["shadows"], go, e["d_table"])
    assert float(amb.double().mean()) < rc.CLIP_CAP
    res["camera compositing backward"] = rc.check_cam_composite_bwd(e["cam"], e["rv"], e["rays"], e["sun"])
    if e["shadows"]:
        res["shadow compositing backward"] = rc.check_sun_composite_bwd(e["sun"], e["rv"])
        res["ambient head backward"] = rc.check_ambient_bwd(e["rv"], e["amb_t"], e["grads"])
    return res


def worst(results):
    return max(w.ratio for w in results)


@pytest.mark.parametrize("ns", [37, 128, 256])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mode", ["shadows-kind1", "noshadow-kind0", "shadows-given_d_out", "shadows-kind1-deterministic"])
def test_clean_emulation_passes_every_check(ns, seed, mode):
    e = emulate(ns, seed, shadows="noshadow" not in mode, kind=0 if "kind0" in mode else 1, given_d_out="given" in mode, deterministic="deterministic" in mode)
    out = e["out"]
    assert all(rc.clip_census(out)), rc.clip_census(out)
    for name, results in run_checks(e).items():
        for w in results:
            print(f"  ns{ns} seed{seed} {mode} {name}: {w!r}")
        assert worst(results) < 1.0, (name, sc.failures(results)[:1] or results)


# defect -> the ONE check that must report it
DEFECTS = {"inclusive_T": "ray record", "geo_late": "geo", "sun_last_nonzero": "shadow compositing backward", "clip_open": "shading backward",
           "no_beta_min": "ray record", "no_02_in_g_wsum": "shading backward", "no_sun_depth_term": "camera compositing backward",
           "no_three_halves": "loss", "relu_leak": "ambient head backward", "g_albedo_ulp": "camera compositing backward"}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_seeded_defect_fails_exactly_its_check(defect):
    res = run_checks(emulate(128, SEEDS[0], defect=defect))
    bad = {name for name, r in res.items() if sc.failures(r)}
    assert bad == {DEFECTS[defect]}, (defect, bad, [repr(w) for r in res.values() for w in sc.failures(r)])


def test_suffix_sum_without_the_carry_fails_at_65_samples_and_passes_at_64():
    e = emulate(128, SEEDS[0], defect="suffix_no_carry")
    res = run_checks(e)
    bad = {name for name, r in res.items() if sc.failures(r)}
    assert bad == {"camera compositing backward"}, bad
    cam, rv = e["cam"], e["rv"]
    A = rr.Ref
    x = rc._pass_inputs(cam, True)
    rw = rr.ray_weights(A, x["sigma"], x["delta"], cam.mask)
    ref = rr.cam_composite_bwd(A, rw, cam.mask, x["delta"], x["tmid"], x["albedo"], x["ts"], x["tb"], rc._rec_cols(rv.rec("g_ray")),
                               [A.inp(e["rays"][:, 3 + d]) for d in range(3)], [A.inp(e["sun"].dense("g_pos", d, 3)) for d in range(3)])[0]
    per_ray = ((cam.dense("g_sigma").double() - ref.v).abs() / ref.e.clamp_min(1e-300)).amax(1)
    r64, r65 = rc.COUNTS_128.index(64), rc.COUNTS_128.index(65)
    assert per_ray[r64] <= 1 and per_ray[r65] > 1, (float(per_ray[r64]), float(per_ray[r65]))


@pytest.mark.parametrize("epoch", [0, 3])
@pytest.mark.parametrize("batch", rc.RENDER_BATCHES)
def test_clip_conditions_hold_on_the_float64_reference_alone(batch, epoch):
    """The render cases of the GPU file, evaluated by the float64 reference only: some channel is clipped at 0, some at 1, some passes, and
    fewer than 2 % of the rays have a lin within the rounding of its expression of 0 or of 1."""
    rays, img, pix, u_cam, u_retry, u_sun, ns = rc.render_batch(batch)
    sd = rc.clip_state_dict()
    d = lambda t: t.double() if t.is_floating_point() else t      # noqa: E731
    field = orc.Field({k: d(v) for k, v in sd.items()})
    with torch.no_grad():
        out, _ = orc.render_rays(field, orc.define_satrays_from_tensors(d(rays), img.reshape(-1, 1)), d(u_cam), d(u_sun), epoch, 2.0 / ns, u_cam_retry=d(u_retry))
    assert all(rc.clip_census(out)), rc.clip_census(out)
    k = rr.K()
    A = rr.Ref
    R = out.shape[0]
    one = torch.ones(R, dtype=torch.float64)
    rec = [A.inp(one)] * k["RAY_REC"]
    rec[k["RR_WSUM"]], rec[k["RR_TS"]], rec[k["RR_GEO"]] = A.inp(one), A.inp(out[:, 11].float()), A.inp(out[:, 10].float())
    for c in range(3):
        rec[k["RR_ALB"] + c], rec[k["RR_AMB"] + c] = A.inp(out[:, 4 + c].float()), A.inp((out[:, 7 + c] / 0.2).float())
    tab = sd["radiometricT_enc.weight"][img]
    _, f = rr.shade(A, rec, [A.inp(tab[:, c]) for c in range(3)], [A.inp(tab[:, 3 + c]) for c in range(3)], epoch >= 2)
    frac = float(rc.clip_ambiguous(f["lin"]).double().mean())
    print(f"{batch} epoch {epoch}: ambiguous rays {frac:.4f}")
    assert frac < rc.CLIP_CAP
