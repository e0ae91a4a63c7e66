"""Per-kernel references for the per-ray kernels of a training step: each is held to the float64 evaluation of ITS OWN operation on the
bits it read -- the per-sample arrays of its pass, the ray record, the record's gradient -- as they lie in the workspace when the call
returns (tests/ray_restated.py decodes them and holds the operations).  No MLP enters a comparison.

Every check returns a list of slab_checks.Worst: name, row = ray, sample = sample slot (or column of a per-ray record), ratio =
|got - ref| / bound, got, ref, bound; ratio <= 1 passes, a bound of 0 demands equality.

The bounds.  The reference arithmetic (ray_restated.Ref) carries, next to every float64 value, a bound on what the fp32 kernel can be off
by, built from the kernel's own rounding steps: u = 2^-24 per fp32 operation on the magnitude of that operation's result, 8 u relative for
the device expf / logf / sinf (the project's allowance for expf / log1pf, tests/slab_checks.py), gamma(k) of the summed magnitudes for a
k-deep sum in the kernel's tree or scan order, and 2^-126 per operation for a result in the denormal range that the device may flush (so
flush-to-zero of T on an opaque ray is not pinned; multiplied on by the later factors, this is the floor "2^-126 times the element's
scale").  Each docstring below names the steps its kernel takes; the numbers follow from them, none is fitted to what a kernel returned.
"""
import torch

import ray_restated as rr
import slab_checks as sc

A = rr.Ref
F64 = torch.float64
CLIP_CAP = 0.02


def _cmp(name, got, ev, exact=None, keep=None):
    """got [R] or [R, C] against an EV; exact: bool mask where the bound is 0; keep: rows (rays) that take part."""
    v, e = ev.v, ev.e
    if exact is not None:
        e = torch.where(exact, torch.zeros_like(e), e)
    got = got.to(F64)
    if keep is not None:
        k = keep if got.dim() == 1 else keep[:, None].expand_as(got)
        got = torch.where(k, got, v)
    return sc.compare(name, got, v, e)


def _rec_cols(rec):
    return [A.inp(rec[:, j]) for j in range(rec.shape[1])]


def _pass_inputs(p, full):
    d = dict(sigma=A.inp(p.dense("sigma")), delta=A.inp(p.dense("delta")))
    if p.has("tmid"):
        d["tmid"] = A.inp(p.dense("tmid"))
    if full:
        d["albedo"] = [A.inp(p.dense("albedo", c, 3)) for c in range(3)]
        d["ts"], d["tb"] = A.inp(p.dense("ts")), A.inp(p.dense("tb"))
    return d


# ------------------------------------------------------------------------------------------------------------ compositing forward
def check_ray_record(cam, rv, depth_only=False, geo_is_one=False):
    """ray_weights + k_composite_fwd.  Steps: sd = fl(sigma delta) [u]; ex = exclusive prefix of sd by a 6-level scan per 64 samples plus
    the carry of the groups in front [gamma(6 + slots per lane) of the prefix, all terms >= 0]; T = expf(-ex) [8 u, and T inherits
    exp(err ex) - 1 ~ gamma(.) ex relative from the prefix]; e = expf(-sd) [8 u + u sd]; alpha = fl(1 - e) [u alpha + err e: ABSOLUTE
    ~8 u where sd is tiny and 1 - e cancels -- scaled by the terms 1 and e, not by alpha]; w = fl(T alpha) [u];  record = per lane
    w x summed over its slots, then a 6-level butterfly [gamma(6 + slots - 1) of sum |w x| plus the w errors times |x|]; tb + 0.05f [u].
    An empty ray: every sum is exactly 0 and tb exactly 0.05f (bound 0)."""
    k = rr.K()
    x = _pass_inputs(cam, not depth_only)
    rw = rr.ray_weights(A, x["sigma"], x["delta"], cam.mask)
    rec = rr.composite_record(A, rw, x["tmid"], x.get("albedo"), x.get("ts"), x.get("tb"), depth_only)
    cols = [k["RR_DEPTH"], k["RR_ALB"], k["RR_ALB"] + 1, k["RR_ALB"] + 2, k["RR_TS"], k["RR_TB"], k["RR_WSUM"]]
    got = rv.rec()[:, cols]
    ref = A.stack(rec, 1)
    empty = (cam.counts == 0)[:, None].expand_as(ref.v)
    res = [_cmp("ray_rec (depth alb3 ts tb wsum)", got, ref, exact=empty)]
    if geo_is_one:
        res.append(sc.compare("ray_rec[GEO] == 1 (no shadow pass)", rv.rec()[:, k["RR_GEO"]], torch.ones(rv.R, dtype=F64, device=got.device),
                              torch.zeros(rv.R, dtype=F64, device=got.device)))
    return res


def check_geo(sun, rv):
    """k_composite_fwd (shadow_only): geo = T at the last sample = expf(-sum_{j < n - 1} sd_j) of the SUN pass' arrays, steps as above;
    exactly 1.0f for an empty shadow ray (bound 0)."""
    x = _pass_inputs(sun, False)
    rw = rr.ray_weights(A, x["sigma"], x["delta"], sun.mask)
    ref = rr.geo_shadow(A, rw, sun.counts)
    return [_cmp("ray_rec[GEO]", rv.rec()[:, rr.K()["RR_GEO"]], ref, exact=sun.counts == 0)]


# ------------------------------------------------------------------------------------------------------------ ambient head
def _amb_weights(t):
    """t: name -> fp32 tensor of the four ambient tensors."""
    return (A.inp(t["ambient_mlp.hidden_layers.0.weight"]), A.inp(t["ambient_mlp.hidden_layers.0.bias"].reshape(-1)),
            A.inp(t["ambient_mlp.output_layer.weight"]), A.inp(t["ambient_mlp.output_layer.bias"].reshape(-1)))


def check_ambient_forward(rv, rays, t):
    """ambient_forward, stage by stage on what the kernel saved: (1) the 27 encoding values from rays[:, 8:11]: 2^k c exact, + fp32(pi/2)
    [u], sinf [8 u]; (2) the 128 hidden values from the SAVED encoding: b1 + 27 multiply-adds, ReLU [gamma(28) of |b1| + sum |w enc|];
    (3) ray_rec[AMB] from the SAVED hidden values: two products per lane, 6-level butterfly, + b2 [gamma], 1 / (1 + expf(-pre)) [8 u, u, u]."""
    k = rr.K()
    w1, b1, w2, b2 = _amb_weights(t)
    sv = rv.f32("amb_save", 160)
    enc = A.stack(rr.ambient_encoding(A, [A.inp(rays[:, 8 + d]) for d in range(3)]), 1)
    res = [_cmp("amb_save encoding", sv[:, :27], enc)]
    res.append(_cmp("amb_save hidden", sv[:, 32:160], rr.ambient_hidden(A, A.inp(sv[:, :27]), w1, b1)))
    out = A.stack(rr.ambient_out(A, A.inp(sv[:, 32:160]), w2, b2), 1)
    res.append(_cmp("ray_rec[AMB]", rv.rec()[:, k["RR_AMB"]:k["RR_AMB"] + 3], out))
    return res


def check_ambient_bwd(rv, t, grads, keep=None):
    """ambient_bwd_body (k_step_tail, the pipelined launch's spare workgroups, or the single deterministic block: the same per-ray code).
    Inputs: g_ray[AMB], ray_rec[AMB], amb_save, w2.  Per ray gpre = fl(fl(g out) fl(1 - out)) [3 u], ghid = 3 products summed [gamma(3)],
    masked where the SAVED hidden value is <= 0 (the kernel's own test on the same bits: no decision is ambiguous); each gradient element
    is the sum of its per-ray products over the rays in any order [gamma(R) of the summed magnitudes]."""
    k = rr.K()
    _, _, w2, _ = _amb_weights(t)
    sv, rec, g = rv.f32("amb_save", 160), rv.rec(), rv.rec("g_ray")
    ref = rr.ambient_bwd(A, [A.inp(g[:, k["RR_AMB"] + o]) for o in range(3)], [A.inp(rec[:, k["RR_AMB"] + o]) for o in range(3)],
                         A.inp(sv[:, :27]), A.inp(sv[:, 32:160]), w2)
    names = {"w1": "ambient_mlp.hidden_layers.0.weight", "b1": "ambient_mlp.hidden_layers.0.bias", "w2": "ambient_mlp.output_layer.weight",
             "b2": "ambient_mlp.output_layer.bias"}
    return [_cmp("d " + names[s], grads[names[s]].reshape(ref[s].shape), ref[s]) for s in ("w1", "b1", "w2", "b2")]


# ------------------------------------------------------------------------------------------------------------ shading, loss
def _table(table, img):
    rows = table[img]
    return [A.inp(rows[:, c]) for c in range(3)], [A.inp(rows[:, 3 + c]) for c in range(3)]


def check_shade(rv, out, table, img, use_shadow, sun_counts=None):
    """shade_ray on the bits of the record.  s = fl(geo ts); amb = fl(fl(wsum head) 0.2f); rgb = fl(fl(alb s) + fl(fl(1 - s) fl(amb alb)));
    lin = fl(fl(A rgb) + b), clamped to [0, 1] (a clamp does not enlarge an error); column 18.. = fl(fl(A alb) + b): one u per step on
    the step's own magnitude.  Copies (3, 4..6, 10, 11, 12) are bit-identical; 13, 16, 17 are exactly 1; 14 = cnt_first; 15 = the sun
    counts, or 1."""
    k = rr.K()
    rec = rv.rec()
    tA, tb = _table(table, img)
    ref, _ = rr.shade(A, _rec_cols(rec), tA, tb, use_shadow)
    z = lambda t: torch.zeros_like(t, dtype=F64)      # noqa: E731
    res = [_cmp("out rgb (0..2)", out[:, 0:3], A.stack([ref[c] for c in range(3)], 1)),
           _cmp("out ambient (7..9)", out[:, 7:10], A.stack([ref[7 + c] for c in range(3)], 1)),
           _cmp("out albedo-only rgb (18..20)", out[:, 18:21], A.stack([ref[18 + c] for c in range(3)], 1))]
    geo = rec[:, k["RR_GEO"]] if use_shadow else torch.ones_like(rec[:, 0])
    copies = torch.stack([rec[:, k["RR_DEPTH"]], rec[:, k["RR_ALB"]], rec[:, k["RR_ALB"] + 1], rec[:, k["RR_ALB"] + 2], geo, rec[:, k["RR_TS"]],
                          rec[:, k["RR_TB"]]], 1)
    res.append(sc.compare("out copies (3 4..6 10 11 12)", out[:, [3, 4, 5, 6, 10, 11, 12]], copies, z(copies)))
    c15 = sun_counts.to(F64) if use_shadow else torch.ones(rv.R, dtype=F64, device=out.device)
    consts = torch.stack([torch.ones_like(c15), rv.i32("cnt_first").to(F64), c15, torch.ones_like(c15), torch.ones_like(c15)], 1)
    res.append(sc.compare("out constants and counts (13..17)", out[:, 13:18], consts, z(consts)))
    return res


def loss_reference(out, pix, kind):
    n = out.shape[0]
    part, go = rr.loss_terms(A, [A.inp(out[:, c]) for c in range(3)], A.inp(out[:, 12]), [A.inp(pix[:, c]) for c in range(3)], n, kind)
    return rr.loss_total(A, part, kind), go


def check_loss(out, pix, kind, loss_got, d_out_got=None):
    """k_loss / the loss inside k_shade_bwd.  inv = fl(1 / fl(3 n)); kind 0: per ray fl(fl(df df) inv) over the channels from 0
    [gamma(2)], gradient fl(fl(2 df) inv); kind 1: ib2 = fl(1 / fl(beta beta)), sq = sum df^2, the term
    fl(fl(fl(fl(0.5 sq) ib2) inv) + fl(fl(0.5 logf(beta)) / n)) [logf: 8 u], gradient columns 0..2 fl(fl(df ib2) inv) and 12
    fl(fl(fl(fl(-sq ib2) / beta) inv) + fl(0.5 / fl(n beta))).  The mean: 6-level butterfly per 64 rays, two levels per block of 256, the
    blocks in order on top of the constant 3/2 of kind 1 [gamma(8 + blocks) of the summed magnitudes, 3/2 included]."""
    total, go = loss_reference(out, pix, kind)
    res = [_cmp(f"loss (kind {kind})", loss_got.reshape(1), EV1(total))]
    if d_out_got is not None:
        cols = sorted(go)
        res.append(_cmp(f"d_out of k_loss (kind {kind})", d_out_got[:, cols], A.stack([go[c] for c in cols], 1)))
        rest = [c for c in range(21) if c not in go]
        res.append(sc.compare("d_out zero columns", d_out_got[:, rest], torch.zeros_like(d_out_got[:, rest], dtype=F64),
                              torch.zeros_like(d_out_got[:, rest], dtype=F64)))
    return res


def EV1(ev):
    return rr.EV(ev.v.reshape(1), ev.e.reshape(1))


def clip_ambiguous(lin):
    """[R] bool: the float64 lin = A pre + b of some channel lies within the derived rounding of that expression of 0 or of 1 -- the fp32
    kernel may take the other side of torch.clip's inclusive bounds."""
    amb = torch.zeros_like(lin[0].v, dtype=torch.bool)
    for l in lin:
        amb |= (l.v.abs() <= l.e) | ((l.v - 1).abs() <= l.e)
    return amb


def check_shade_bwd(rv, table, img, use_shadow, go, d_table=None):
    """k_shade_bwd from the bits of ray_rec, the table and `go` = {column: EV} (the loss gradient as the same kernel forms it from out and
    the pixels, or the caller's d_out as exact inputs).  lin is recomputed as in the forward; the gradient passes for 0 <= lin <= 1.  A
    ray whose float64 lin is within its own rounding bound of 0 or 1 (clip_ambiguous) is left out of the g_ray and rad_rays comparisons;
    CLIP_CAP bounds how many may be (asserted by the caller).  Every column is a handful of fp32 products and sums: u per step.
    The table gradient, rows [img][0..5]: deterministic mode -- rad_rays per ray, and the table BIT-IDENTICAL to the fp32 sum of those
    rows in ray order (one thread per element, k_table_reduce); otherwise (LDS accumulation per block, then atomics) the sum over the
    image's rays in any order [gamma(rays of the image) of the summed magnitudes], where an ambiguous ray widens the bound by the whole
    effect of its decision (|go| |pre| on the gain, |go| on the offset).  Columns 6..8 of the table receive nothing.
    -> (results, ambiguous [R])."""
    k = rr.K()
    rec = rv.rec()
    tA, tb = _table(table, img)
    g, rad, lin = rr.shade_bwd(A, _rec_cols(rec), go, tA, tb, use_shadow)
    amb = clip_ambiguous(lin)
    keep = ~amb
    cols = [k["RR_DEPTH"], k["RR_ALB"], k["RR_ALB"] + 1, k["RR_ALB"] + 2, k["RR_TS"], k["RR_TB"], k["RR_WSUM"], k["RR_AMB"], k["RR_AMB"] + 1,
            k["RR_AMB"] + 2, k["RR_GEO"]]
    res = [_cmp("g_ray (shading backward)", rv.rec("g_ray")[:, cols], A.stack([g[c] for c in cols], 1), keep=keep)]
    if d_table is None:
        return res, amb
    radv = A.stack(rad, 1)
    n_img = table.shape[0]
    if rv.has("rad_rays"):
        got = rv.f32("rad_rays", 6)
        res.append(_cmp("rad_rays", got, radv, keep=keep))
        acc = torch.zeros(n_img, 6, dtype=torch.float32, device=got.device)
        for r in range(rv.R):
            acc[img[r]] += got[r]
        res.append(sc.compare("d radiometric == in-order sum of rad_rays", d_table[:, :6], acc, torch.zeros(n_img, 6, dtype=F64, device=got.device)))
    else:
        zero = torch.zeros_like(radv.e[:, 0])
        extra = []
        for c in range(3):
            _, f = rr.shade(A, _rec_cols(rec), tA, tb, use_shadow)
            gc = go[c].mag() if c in go else zero
            extra.append(torch.where(amb, gc * f["pre"][c].mag(), zero))
        for c in range(3):
            extra.append(torch.where(amb, go[c].mag() if c in go else zero, zero))
        radv = rr.EV(radv.v, radv.e + torch.stack(extra, 1))
        res.append(_cmp("d radiometric (sum over the image's rays)", d_table[:, :6], A.index_sum(radv, img, n_img)))
    z = torch.zeros(n_img, 3, dtype=F64, device=d_table.device)
    res.append(sc.compare("d radiometric columns 6..8 == 0", d_table[:, 6:9], z, z))
    return res, amb


# ------------------------------------------------------------------------------------------------------------ rendering outputs
def check_rendering_out(rv, outs, depth_only):
    """k_rendering_out: depth, albedo, beta, ts are copies of the record (bit-identical), ambient = fl(wsum head), entropy = 1."""
    k = rr.K()
    rec = rv.rec()
    z = lambda t: torch.zeros_like(t, dtype=F64)      # noqa: E731
    res = [sc.compare("rendering depth", outs["depth"], rec[:, k["RR_DEPTH"]], z(outs["depth"]))]
    if depth_only:
        return res
    copies = torch.cat([outs["albedo"], outs["beta"][:, None], outs["ts"][:, None], outs["entropy"][:, None]], 1)
    want = torch.cat([rec[:, k["RR_ALB"]:k["RR_ALB"] + 3], rec[:, k["RR_TB"]][:, None], rec[:, k["RR_TS"]][:, None], torch.ones_like(rec[:, :1])], 1)
    res.append(sc.compare("rendering copies (albedo beta ts entropy)", copies, want, z(want)))
    res.append(_cmp("rendering ambient", outs["ambient"], A.stack(rr.rendering_out(A, _rec_cols(rec)), 1)))
    return res


def check_rendering_out_bwd(rv, cot, depth_only):
    """k_rendering_out_bwd.  cot: name -> tensor or None (a NULL cotangent is zero; depth_only passes g_depth alone).  Copied columns
    (DEPTH, ALB, TS, TB) are bit-identical to the cotangents, GEO and the column behind it exactly 0; g[AMB + c] = fl(ga_c wsum),
    g[WSUM] = the three fl(ga_c head_c) summed from 0 [u per step]."""
    k = rr.K()
    rec, g = rv.rec(), rv.rec("g_ray")
    R, dev = rv.R, rec.device
    get = lambda name, c: (torch.zeros(R, c, device=dev) if (cot.get(name) is None or (depth_only and name != "g_depth")) else cot[name].reshape(R, c))      # noqa: E731
    want = torch.cat([get("g_depth", 1), get("g_albedo", 3), get("g_ts", 1), get("g_beta", 1), torch.zeros(R, 2, device=dev)], 1)
    cols = [k["RR_DEPTH"], k["RR_ALB"], k["RR_ALB"] + 1, k["RR_ALB"] + 2, k["RR_TS"], k["RR_TB"], k["RR_GEO"], k["RR_GEO"] + 1]
    res = [sc.compare("g_ray copies (rendering)", g[:, cols], want, torch.zeros_like(want, dtype=F64))]
    ga = get("g_ambient", 3)
    ref = rr.rendering_out_bwd(A, _rec_cols(rec), [A.inp(ga[:, c]) for c in range(3)])
    cols = [k["RR_AMB"], k["RR_AMB"] + 1, k["RR_AMB"] + 2, k["RR_WSUM"]]
    res.append(_cmp("g_ray AMB / WSUM (rendering)", g[:, cols], A.stack([ref[c] for c in cols], 1)))
    return res


# ------------------------------------------------------------------------------------------------------------ compositing backward
def check_cam_composite_bwd(cam, rv, rays, sun=None, depth_only=False):
    """k_cam_composite_bwd from the bits of g_ray and the pass' arrays.  w, T, e as in the forward (same ray_weights, same bounds).
    g_albedo, g_ts, g_tb = fl(w g) per sample [u, plus the error of w times |g|].  g_depth = g[DEPTH] + the butterfly sum over the ray's
    shadow samples of fl(fl(fl(gx dx) + fl(gy dy)) + fl(gz dz)) when the shadow pass ran.  gw_i = g_depth tmid + sum_c g_alb_c alb_c +
    g_ts ts + g_tb tb + g_wsum, left to right [u per step]; the exclusive suffix sum of fl(gw w) by a 6-level scan per 64 samples plus
    the carry of the groups behind [gamma(6 + slots) of sum_{j > i} |gw_j| w_j]; g_sigma_i = fl(delta_i fl(fl(fl(gw_i T_i) e_i) - suffix)):
    delta_i times the rounding of the two magnitudes |gw_i| T_i e_i and sum_{j > i} |gw_j| w_j, with the error T inherits from the
    fp32 prefix (relative exp(gamma(.) sum_{j < i} sd_j) - 1)."""
    x = _pass_inputs(cam, not depth_only)
    rw = rr.ray_weights(A, x["sigma"], x["delta"], cam.mask)
    g = _rec_cols(rv.rec("g_ray"))
    sun_gpos = view_d = None
    if sun is not None:
        sun_gpos = [A.inp(_gather_to(cam, sun, d)) for d in range(3)]
        view_d = [A.inp(rays[:, 3 + d]) for d in range(3)]
    ref = rr.cam_composite_bwd(A, rw, cam.mask, x["delta"], x["tmid"], x.get("albedo"), x.get("ts"), x.get("tb"), g, view_d, sun_gpos, depth_only)
    res = [_cmp("g_sigma (camera compositing backward)", cam.dense("g_sigma"), ref[0])]
    if not depth_only:
        for c in range(3):
            res.append(_cmp(f"g_albedo[{c}]", cam.dense("g_albedo", c, 3), ref[1][c]))
        res.append(_cmp("g_ts", cam.dense("g_ts"), ref[2]))
        res.append(_cmp("g_tb", cam.dense("g_tb"), ref[3]))
    return res


def _gather_to(cam, sun, d):
    """The sun pass' g_pos row d over each ray's shadow samples, as [R, cam.W] (both passes share the instance's width)."""
    assert sun.W == cam.W
    return sun.dense("g_pos", d, 3)


def check_sun_composite_bwd(sun, rv):
    """k_sun_composite_bwd: g_sigma_i = fl(fl(-g_geo geo) delta_i) for i < n - 1 [2 u], exactly 0.0f at i = n - 1 (bound 0)."""
    k = rr.K()
    ref = rr.sun_composite_bwd(A, A.inp(rv.rec("g_ray")[:, k["RR_GEO"]]), A.inp(rv.rec()[:, k["RR_GEO"]]), A.inp(sun.dense("delta")), sun.mask, sun.counts)
    return [_cmp("sun g_sigma (shadow compositing backward)", sun.dense("g_sigma"), ref)]


# ------------------------------------------------------------------------------------------------------------ cases shared by the CPU and GPU files
N_IMG, SEED = 6, 7
COUNTS_128 = [0, 1, 2, 63, 64, 65, 127]
COUNTS_256 = COUNTS_128 + [128, 129, 191, 192, 193, 254, 255]


def clip_state_dict():
    """The state dict of the GPU cases.  The synthetic batch alone never leaves [0, 1] (gains 1, offsets 0), so the radiometric rows are
    set by a fixed pattern, not tuned to any output: image i has gain 40 on channel i % 3 (lin > 1 wherever pre > 0.025), offset -1.5 on
    channel (i + 1) % 3 (lin < 0 always) and the identity on the third -- every ray with some colour clips at both bounds and passes in one
    channel."""
    from oracle import eonerf_oracle as orc
    sd = orc.random_state_dict(N_IMG, seed=SEED, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    rad = sd["radiometricT_enc.weight"].clone()
    for i in range(N_IMG):
        rad[i, i % 3] = 40.0
        rad[i, 3 + (i + 1) % 3] = -1.5
    sd["radiometricT_enc.weight"] = rad
    return sd


def render_batch(name):
    """-> rays [R, 11], img [R], pixels [R, 3], u_cam, u_retry, u_sun [R, n_samples], n_samples.  The batches of the render-step cases."""
    from oracle import eonerf_oracle as orc
    R, ns, seed = {"R1": (1, 128, 61), "R37": (37, 128, 62), "R300": (300, 128, 63), "R96-ns37": (96, 37, 64), "R12-ns256": (12, 256, 65),
                   "edges-retry": (192, 128, 52)}[name]
    rays, ts, rgbs, u_cam, u_sun = orc.synthetic_batch(R, N_IMG, seed=seed, n_samples=ns)
    u_retry = u_cam
    if name == "edges-retry":      # rays 5 and 7 of tests/test_origin_grad_gpu.py::test_edges_empty_ray_and_empty_shadow_ray
        rays = rays.clone()
        rays[5, 0], rays[5, 3:6] = 1.5, torch.tensor([1.0, 0.0, 0.0])
        d = torch.tensor([0.7, 0.7, -0.1])
        rays[7, 0:3], rays[7, 3:6] = torch.tensor([0.99, 0.99, 0.9995]), d / d.norm()
    return rays, ts.reshape(-1), rgbs, u_cam, u_retry, u_sun, ns


RENDER_BATCHES = ["R1", "R37", "R300", "R96-ns37", "R12-ns256", "edges-retry"]


def clip_census(out):
    """(some channel clipped at 0, some at 1, some strictly inside) over columns 0..2 of out."""
    rgb = out[:, :3]
    return bool((rgb == 0).any()), bool((rgb == 1).any()), bool(((rgb > 0) & (rgb < 1)).any())
