"""GPU: the per-ray kernels of a training step held to float64 references, ray by ray.

The kernels of csrc/eonerf_rays.hip / eonerf_rays_bwd.hip (compositing forward, shadow-ray transmittance, ambient head, shading, the loss,
the shading backward, both compositing backwards, the rendering outputs and their backward, the ambient-head backward, the radiometric
table gradient) read a few per-sample arrays and write a per-ray record or per-sample gradients, and all of that still lies in the
caller's workspace when the call returns.  These tests call the C ABI on guarded workspaces of exactly the reported size, prefilled with
0xFF, with fixed noise buffers, ask eonerf_ray_layout / eonerf_workspace_layout where the buffers are, and hold every kernel to the float64
evaluation of its own operation on the bits it read (tests/ray_checks.py: every bound is derived there; tests/ray_restated.py holds the
operations).  The float64 references run in torch on the card.  No MLP enters a comparison.

The per-ray code is the same for both precisions; what differs between the contexts is which launch hosts the ambient-head backward and
which reduction the table gradients take -- the ids name it:
  bf16-pipe   the ambient backward on the pipelined launch's spare workgroups (shadow pass on), the table through LDS accumulation + atomics
  fp32-gemm   chain + GEMM path: the ambient backward in k_step_tail, the table as above
  bf16-det    EONERF_DETERMINISTIC=1: the ambient backward in its single block, the table through rad_rays + k_table_reduce

Per check, the worst |got - ref| / bound over the cases of a run is printed at the end of the module (reported figures, not gates: the
gates are the bounds); DESIGN.md section 5 has the table recorded on MI355X: everything below 0.95, the margins nearest 1 being the one-,
two- and three-rounding products (rendering ambient 0.95, sun g_sigma 0.91).  49 items, 2.9 s."""
import ctypes as C
import functools
import os
import time

import pytest
import torch

from oracle import eonerf_oracle as orc
import ray_checks as rc
import ray_restated as rr
import slab_checks as sc
import slab_restated as sr
import workspace_guard as wg

pytestmark = pytest.mark.gpu
F32 = torch.float32
SHADOWS, TRAIN, ONLY_DEPTH = 1, 4, 8
KIND_RENDER = 1
RATIOS = {}
CONTEXTS = {"bf16-pipe": ("bf16", "1", "0"), "fp32-gemm": ("fp32", "0", "0"), "bf16-det": ("bf16", "1", "1")}
AMB = ["ambient_mlp.hidden_layers.0.weight", "ambient_mlp.hidden_layers.0.bias", "ambient_mlp.output_layer.weight", "ambient_mlp.output_layer.bias"]
RAD = "radiometricT_enc.weight"


def L():
    from eonerf_code_amd import _lib
    return _lib.lib()


def P(x):
    if x is None:
        return C.c_void_p(0)
    return C.c_void_p(x.ptr if isinstance(x, wg.Guarded) else x.data_ptr())


@functools.lru_cache(maxsize=None)
def _field(name):
    """One native context per entry of CONTEXTS; EONERF_PIPE and EONERF_DETERMINISTIC are read when the context is created, so they are
    set before the first _context() (as tests/test_origin_grad_gpu.py does)."""
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    precision, pipe, det = CONTEXTS[name]
    f = EONerfMLP(rc.N_IMG, radiometric_normalization=True, precision=precision)
    f.load_state_dict(rc.clip_state_dict(), strict=True)
    f = f.cuda()
    keys = {"EONERF_PIPE": pipe, "EONERF_DETERMINISTIC": det}
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    try:
        f._context()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    f._ensure_packed()
    return f


def layouts(ctx, R, flags):
    t = (C.c_uint64 * sr.LAYOUT_ENTRIES)()
    assert L().eonerf_layout_version() == 1
    assert L().eonerf_workspace_layout(ctx, KIND_RENDER, R, flags, t, sr.LAYOUT_ENTRIES) == sr.LAYOUT_ENTRIES
    q = (C.c_uint64 * rr.RAY_ENTRIES)()
    assert L().eonerf_ray_layout(ctx, R, flags, q, rr.RAY_ENTRIES) == rr.RAY_ENTRIES
    assert L().eonerf_ray_layout(ctx, R, flags, q, rr.RAY_ENTRIES - 1) == -1 and L().eonerf_ray_layout(None, R, flags, q, rr.RAY_ENTRIES) == -1
    return sr.layout_dict(list(t)) + (rr.ray_layout_dict(list(q)),)


def tensors(f, flat):
    return {name: flat[off:off + r * c].view(r, c) for name, off, r, c in f._layout}


def record(results, case, group):
    for w in results:
        print(f"  {case}: {w!r}")
        if w.ratio > RATIOS.get((group, w.name), (-1.0, ""))[0]:
            RATIOS[(group, w.name)] = (w.ratio, case)
    bad = sc.failures(results)
    assert not bad, f"{case}: {len(bad)} check(s) beyond their derived bound, first: {bad[0]!r}"


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print("\nworst |got - ref| / bound per check over the cases of this run:")
    for (group, name), (ratio, case) in sorted(RATIOS.items()):
        print(f"  {group:10s} {name:50s} {ratio:9.4f}   {case}")
    print(f"run time of this module's tests: {time.time() - t0:.1f} s")


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(*shape, device="cuda", generator=g) * (hi - lo) + lo).contiguous()


# ------------------------------------------------------------------------------------------------------------ render step
def check_sun_setup(sun, rv, rays, u_sun, ns):
    """sun_geom + the sun sampler: counts, offsets, positions, mid points and interval lengths of the sun pass are bit-identical to
    orc.satnerf_sampling in fp32 on o + depth d, depth = the bits of ray_rec[DEPTH] (explicit __fadd_rn / __fmul_rn in a unit built with
    -ffp-contract=off: identity is the bar).  No 1e10 patch on this pass."""
    R = rv.R
    depth = rv.rec()[:, rr.K()["RR_DEPTH"]][:, None]
    o = rays[:, 0:3] + torch.hstack([depth, depth, depth]) * rays[:, 3:6]
    d = -1.0 * rays[:, 8:11]
    assert int(2 / (2.0 / ns)) == ns
    ri, ts_, te_ = orc.satnerf_sampling(o, d, u_sun, 2.0 / ns)
    cnt = torch.bincount(ri, minlength=R)
    assert torch.equal(cnt, sun.counts), "sun counts"
    assert torch.equal(torch.cat([torch.zeros(1, dtype=torch.long, device="cuda"), cnt.cumsum(0)]), sun.offsets), "sun offsets"
    n = int(cnt.sum())
    assert n == sun.n
    mid = (ts_ + te_)[:, None] / 2.0
    pos = o[ri] + d[ri] * mid
    for name, want in (("px", pos[:, 0]), ("py", pos[:, 1]), ("pz", pos[:, 2]), ("tmid", mid[:, 0]), ("delta", te_ - ts_)):
        wg.assert_same_bits("sun ray set-up", name, sun.flat(name)[0][:n], want.contiguous())


def run_render_step(ctx_name, batch, flags, kind, two_call=False):
    f = _field(ctx_name)
    rays, img, pix, u_cam, u_retry, u_sun, ns = (t.cuda().contiguous() if torch.is_tensor(t) else t for t in rc.render_batch(batch))
    f.set_n_samples(ns)
    ctx, R, shadows = f._ctx, rays.shape[0], bool(flags & SHADOWS)
    nbytes = int(L().eonerf_render_workspace_bytes(ctx, R, flags))
    head, cam_off, sun_off, ray_off = layouts(ctx, R, flags)
    assert head["bytes"] == nbytes and ("rad_rays" in ray_off) == (ctx_name == "bf16-det")
    assert "dy_in" in head or ctx_name != "bf16-pipe", "the pipelined path"
    assert "dy_in" not in head or ctx_name != "fp32-gemm", "the chain + GEMM path"
    assert all(k in ray_off for k in ("cnt_first", "cnt_retry", "flags", "ray_rec", "g_ray", "amb_save")) and bool(sun_off) == shadows
    p_cap = head["p_cap"]
    ws = wg.Guarded("workspace", nbytes, "cuda", fill=0xFF)
    z = torch.linspace(0, 1, ns, device="cuda")
    out, n_dev, loss, loss2 = (wg.Guarded(n_, b, "cuda") for n_, b in (("out", 4 * R * 21), ("n_samples_dev", 4), ("loss", 4), ("loss2", 4)))
    d_out = wg.Guarded("d_out", 4 * R * 21, "cuda")
    d_flat = torch.zeros(int(L().eonerf_grad_floats(ctx)), device="cuda")
    w = C.c_void_p(ws.ptr)
    rc_ = L().eonerf_render_forward(ctx, P(f._flat), P(rays), P(img), P(z), P(u_cam), P(u_retry), P(u_sun if shadows else None), R, flags, P(out), P(n_dev), w, nbytes, None)
    assert rc_ == 0, rc_
    assert L().eonerf_train_loss(ctx, P(out), P(pix), R, kind, P(d_out), P(loss2), None) == 0
    if two_call:
        rc_ = L().eonerf_render_backward(ctx, P(f._flat), P(rays), P(img), R, flags, P(d_out), P(d_flat), w, nbytes, None)
    else:
        rc_ = L().eonerf_render_backward_loss(ctx, P(f._flat), P(rays), P(img), R, flags, P(out), P(pix), kind, None, P(loss), P(d_flat), w, nbytes, None)
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    assert L().eonerf_device_status(ctx, None) == 0
    wg.check_guards("render step", [ws, out, n_dev, loss, loss2, d_out])
    raw = ws.payload
    rv = rr.RayView(raw, ray_off, R)
    cam = rr.PassView(raw, cam_off, p_cap, R, ns)
    sun = rr.PassView(raw, sun_off, p_cap, R, ns) if shadows else None
    o21, do21 = out.view(F32, R, 21), d_out.view(F32, R, 21)
    par, grads = tensors(f, f._flat), tensors(f, d_flat)
    # what the case is: the retry draw, the counts the shading reports, clipping at both bounds
    # (flags[0] is the LAST sampler launch's word: the shadow pass' sampler, which never retries, overwrites the camera pass' bit)
    retried = bool((rv.i32("cnt_first") == 0).any())
    assert retried == (batch == "edges-retry") and (shadows or bool(int(rv.i32("flags", 4)[0]) & 1) == retried)
    assert cam.n == int(n_dev.view(torch.int32, 1)[0])
    if shadows:      # (the shadow rays' count kernel leaves ITS counts in cnt_retry)
        assert torch.equal(sun.counts, rv.i32("cnt_retry").long()) and (retried or torch.equal(cam.counts, rv.i32("cnt_first").long()))
    else:
        assert torch.equal(cam.counts, rv.i32("cnt_retry" if retried else "cnt_first").long())
    if batch == "edges-retry":
        assert int(cam.counts[5]) == 0 and int(cam.counts[7]) == 1 and (not shadows or int(sun.counts[7]) == 0)
    assert all(rc.clip_census(o21)), rc.clip_census(o21)
    res = rc.check_ray_record(cam, rv, geo_is_one=not shadows)
    if shadows:
        check_sun_setup(sun, rv, rays, u_sun, ns)
        res += rc.check_geo(sun, rv)
    res += rc.check_ambient_forward(rv, rays, par)
    res += rc.check_shade(rv, o21, par[RAD], img, shadows, sun.counts if shadows else None)
    lres = rc.check_loss(o21, pix, kind, loss2.view(F32, 1), do21)
    lres[0].name += " (k_loss)"
    res += lres
    if two_call:
        go = {c: rr.Ref.inp(do21[:, c]) for c in range(21)}
    else:
        res += rc.check_loss(o21, pix, kind, loss.view(F32, 1))
        wg.assert_same_bits("loss", "fused scalar against eonerf_train_loss", loss.view(F32, 1), loss2.view(F32, 1))
        go = rc.loss_reference(o21, pix, kind)[1]
    part, amb = rc.check_shade_bwd(rv, par[RAD], img, shadows, go, grads[RAD])
    frac = float(amb.double().mean())
    assert frac < rc.CLIP_CAP, f"{frac:.3f} of the rays have an ambiguous clip decision"
    res += part
    res += rc.check_cam_composite_bwd(cam, rv, rays, sun)
    if shadows:
        res += rc.check_sun_composite_bwd(sun, rv)
        res += rc.check_ambient_bwd(rv, par, grads)
    else:      # s = 1: the ambient head is outside the graph
        for name in AMB:
            assert not bool(grads[name].any()), name
    return res


STEP_MODES = {"shadows-kind1": (TRAIN | SHADOWS, 1), "noshadow-kind0": (TRAIN, 0)}


@pytest.mark.parametrize("batch", rc.RENDER_BATCHES)
@pytest.mark.parametrize("mode", sorted(STEP_MODES))
@pytest.mark.parametrize("ctx_name", sorted(CONTEXTS))
def test_render_step_per_ray_kernels(ctx_name, mode, batch):
    """eonerf_render_forward + eonerf_render_backward_loss: every per-ray kernel of the step on its own inputs.  Batches: R = 1, 37, 300 at
    128 samples; 96 rays at 37 samples (one slot per lane); 12 rays at 256 samples (four slots); and the batch with an empty camera ray (5)
    and a ray whose shadow ray is empty (7), in which the retry draw fires."""
    flags, kind = STEP_MODES[mode]
    record(run_render_step(ctx_name, batch, flags, kind), f"step[{ctx_name}-{mode}-{batch}]", ctx_name)


@pytest.mark.parametrize("ctx_name", sorted(CONTEXTS))
def test_render_step_two_calls_given_d_out(ctx_name):
    """eonerf_train_loss + eonerf_render_backward: the shading backward is held to the d_out it was given."""
    record(run_render_step(ctx_name, "R37", TRAIN | SHADOWS, 1, two_call=True), f"step[{ctx_name}-two calls-R37]", ctx_name)


# ------------------------------------------------------------------------------------------------------------ flattened samples
def flattened_samples(ns):
    """ray_indices / t_starts / t_ends with per-ray counts exactly COUNTS_128 (COUNTS_256 at 256 samples), three times over -- once per
    regime of interval lengths: 1e-6 .. 1e-5 (1 - exp(-sd) cancels), 0.01 .. 0.05, and 0.02 for three samples then 50 (T underflows
    along the ray)."""
    lst = rc.COUNTS_256 if ns > 128 else rc.COUNTS_128
    counts = lst * 3
    g = torch.Generator().manual_seed(70 + ns)
    ri, t0, t1 = [], [], []
    for r, n in enumerate(counts):
        regime = r // len(lst)
        u = torch.rand(n, generator=g)
        length = [1e-6 + 9e-6 * u, 0.01 + 0.04 * u, torch.where(torch.arange(n) < 3, torch.full((n,), 0.02), torch.full((n,), 50.0))][regime].float()
        start = (0.05 + torch.cat([torch.zeros(1), length.cumsum(0)[:-1]])).float() if n else torch.zeros(0)
        ri.append(torch.full((n,), r, dtype=torch.long)), t0.append(start), t1.append(start + length)
    return counts, torch.cat(ri), torch.cat(t0), torch.cat(t1)


FLAT_CASES = [(c, d, ns, False) for c in ("bf16-pipe", "fp32-gemm") for d in (0, 1) for ns in (128, 256)] + [(c, 0, 128, True) for c in ("bf16-pipe", "fp32-gemm")]


@pytest.mark.parametrize("ctx_name,depth_only,ns,null_cot", FLAT_CASES,
                         ids=[f"{c}-depth_only{d}-ns{ns}{'-null_cotangents' if nc else ''}" for c, d, ns, nc in FLAT_CASES])
def test_flattened_samples_per_ray_kernels(ctx_name, depth_only, ns, null_cot):
    """eonerf_rendering_train + eonerf_rendering_backward on samples the test builds: every count at which the scans change shape, interval
    lengths from 1e-6 to 50, random cotangents (null_cot: g_beta and g_ambient NULL, one run per context: a NULL pointer takes no other path at another size).  The ambient backward runs in k_step_tail on both
    contexts here.  At the C ABI t_ends is a const input: the 1e10 patch of the last interval of every ray shows in the workspace's
    delta (asserted bit for bit, with the mid points), and t_ends itself must come back unchanged."""
    from eonerf_code_amd.synthetic import synthetic_batch
    f = _field(ctx_name)
    f.set_n_samples(ns)
    counts, ri, t0, t1 = flattened_samples(ns)
    R, n = len(counts), int(ri.numel())
    rays, img, _ = (t.cuda().contiguous() for t in synthetic_batch(R, rc.N_IMG, seed=80 + ns))
    ri, t0, t1 = ri.cuda(), t0.cuda().contiguous(), t1.cuda().contiguous()
    t1_before = t1.clone()
    ctx, flags = f._ctx, TRAIN | (ONLY_DEPTH if depth_only else 0)
    nbytes = int(L().eonerf_render_workspace_bytes(ctx, R, flags))
    head, cam_off, sun_off, ray_off = layouts(ctx, R, flags)
    assert head["bytes"] == nbytes and not sun_off and ("albedo" in cam_off) == (not depth_only)
    p_cap = head["p_cap"]
    ws = wg.Guarded("workspace", nbytes, "cuda", fill=0xFF)
    names = ("albedo", "depth", "beta", "ts", "ambient", "entropy")
    outs = {k: wg.Guarded(k, 4 * R * c, "cuda") for k, c in zip(names, (3, 1, 1, 1, 3, 1))}
    po = lambda k: P(None) if (depth_only and k != "depth") else P(outs[k])      # noqa: E731
    w = C.c_void_p(ws.ptr)
    rc_ = L().eonerf_rendering_train(ctx, P(f._flat), P(rays), P(img), P(t0), P(t1), P(ri), n, R, depth_only, *(po(k) for k in names), w, nbytes, None)
    assert rc_ == 0, rc_
    cot = {"g_albedo": _rand((R, 3), 91), "g_depth": _rand((R,), 92), "g_beta": _rand((R,), 93), "g_ts": _rand((R,), 94), "g_ambient": _rand((R, 3), 95)}
    if null_cot:
        cot["g_beta"] = cot["g_ambient"] = None
    d_flat = torch.zeros(int(L().eonerf_grad_floats(ctx)), device="cuda")
    rc_ = L().eonerf_rendering_backward(ctx, P(f._flat), P(rays), P(img), R, depth_only, P(cot["g_albedo"]), P(cot["g_depth"]), P(cot["g_beta"]), P(cot["g_ts"]),
                                        P(cot["g_ambient"]), P(d_flat), w, nbytes, None)
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    assert L().eonerf_device_status(ctx, None) == 0
    wg.check_guards("rendering pair", [ws] + list(outs.values()))
    raw = ws.payload
    rv, cam = rr.RayView(raw, ray_off, R), rr.PassView(raw, cam_off, p_cap, R, ns)
    assert cam.counts.tolist() == counts and cam.n == n
    # k_packed_emit: mid points, and the 1e10 patch of every ray's last interval (in delta; the caller's t_ends is an input)
    assert torch.equal(t1, t1_before)
    last = torch.zeros(n, dtype=torch.bool, device="cuda")
    last[(cam.offsets[:R] + cam.counts - 1)[cam.counts > 0]] = True      # (offsets of a ray without samples is not a prefix sum here)
    wg.assert_same_bits("packed samples", "delta", cam.flat("delta")[0][:n], torch.where(last, torch.full_like(t1, 1e10), t1) - t0)
    wg.assert_same_bits("packed samples", "tmid", cam.flat("tmid")[0][:n], (t0 + t1) / 2.0)
    assert int(last.sum()) == sum(1 for c in counts if c > 0)
    par, grads = tensors(f, f._flat), tensors(f, d_flat)
    res = rc.check_ray_record(cam, rv, depth_only=bool(depth_only), geo_is_one=True)
    o = {k: outs[k].view(F32, R, c)[:, 0] if c == 1 else outs[k].view(F32, R, c) for k, c in zip(names, (3, 1, 1, 1, 3, 1))}
    res += rc.check_rendering_out(rv, o, bool(depth_only))
    res += rc.check_rendering_out_bwd(rv, cot, bool(depth_only))
    res += rc.check_cam_composite_bwd(cam, rv, rays, None, depth_only=bool(depth_only))
    if not depth_only:
        res += rc.check_ambient_forward(rv, rays, par)
        res += rc.check_ambient_bwd(rv, par, grads)
    record(res, f"flat[{ctx_name}-depth_only{depth_only}-ns{ns}{'-null cotangents' if null_cot else ''}]", ctx_name)
