"""GPU: the training kernels held to exact references on their own slabs.

Every chain / GEMM kernel of a training call reads its operands from the caller's workspace and writes its result to the workspace or to
the gradient buffer.  These tests call the C ABI on workspaces they own, ask eonerf_workspace_layout where the buffers are, decode them
(tests/slab_restated.py) and hold each kernel to a float64 evaluation of its own operation on the bits it read (tests/slab_checks.py, where
every bound is derived in the docstring of its check).  The float64 references run in torch on the card.  A failure names the tensor, the
row and the sample.

Per check, the worst |got - ref| / bound over all cases of a run is collected in RATIOS and printed at the end of the module (reported
figures, not gates: the gates are the bounds).  Recorded on MI355X (DESIGN.md section 5 has the table): every bf16-rounded tensor 0.97 .. 0.996
(the rounding itself), the accumulation-only checks (GEMM jobs, bottleneck factors and their products, g_emb, head outputs) 0.005 .. 0.06,
g_pos 0.11 (field) / 0.17 (render), the embedding table 0.10, fp32 mode below 0.6 everywhere; the narrowest margin is the sun pass'
encoding at 0.993 (__sinf near an argument of 500).  41 items, 3.4 s."""
import ctypes as C
import functools
import os
import time

import pytest
import torch

from oracle import eonerf_oracle as orc
import slab_checks as sc
import slab_restated as sr
import workspace_guard as wg

pytestmark = pytest.mark.gpu
N_IMG, SEED = 5, 7
F32 = torch.float32
KIND_FIELD_TRAIN, KIND_RENDER = 0, 1
RATIOS = {}


def L():
    from eonerf_code_amd import _lib
    return _lib.lib()


def P(x):
    if x is None:
        return C.c_void_p(0)
    return C.c_void_p(x.ptr if isinstance(x, wg.Guarded) else x.data_ptr())


@functools.lru_cache(maxsize=None)
def _field(precision, pipe=True):
    """One native context per (precision, backward path); the library reads EONERF_PIPE when the context is created (as
    tests/test_bwd_pipe.py does).  Default (atomic) summation mode."""
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    sd = orc.random_state_dict(N_IMG, seed=SEED, bias_scale=0.05)      # the ambiguity cap of this seed: tests/test_slab_checks_cpu.py
    sd["sigma_layer.output_layer.bias"] += 1.0
    f = EONerfMLP(N_IMG, radiometric_normalization=True, precision=precision)
    f.load_state_dict(sd, strict=True)
    f = f.cuda()
    keys = {"EONERF_PIPE": "1" if pipe else "0", "EONERF_DETERMINISTIC": "0"}
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


@functools.lru_cache(maxsize=None)
def _params(precision, pipe=True):
    f = _field(precision, pipe)
    pr = sc.Params.from_flat(f._flat, f._layout, precision)
    assert pr.fold()["amb_frac"] < 0.01, pr.fold()["amb_frac"]
    return pr


def layout(ctx, kind, n, flags):
    t = (C.c_uint64 * sr.LAYOUT_ENTRIES)()
    assert L().eonerf_layout_version() == 1
    assert L().eonerf_workspace_layout(ctx, kind, n, flags, t, sr.LAYOUT_ENTRIES) == sr.LAYOUT_ENTRIES
    return sr.layout_dict(list(t))


def grad_views(f, d_flat):
    return {name: d_flat[off:off + r * c].view(r, c) for name, off, r, c in f._layout}


def record(results, case, group):
    """group: the column of the report (field bf16 / field fp32 / render)."""
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
        print(f"  {group:12s} {name:36s} {ratio:9.4f}   {case}")
    print(f"run time of this module's tests: {time.time() - t0:.1f} s")


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(*shape, device="cuda", generator=g) * (hi - lo) + lo).contiguous()


# ------------------------------------------------------------------------------------------------------------ field pair
def run_field_pair(precision, density_only, n, live=None):
    """eonerf_field_forward_train + eonerf_field_backward on a guarded workspace of exactly the reported size, pre-filled with 0xFF (NaN:
    anything read but not written shows).  live: the samples with non-zero upstream gradients (None: all, dense and random)."""
    f = _field(precision)
    ctx = f._ctx
    nbytes = int(L().eonerf_field_train_workspace_bytes(ctx, n, density_only))
    head, off, sun = layout(ctx, KIND_FIELD_TRAIN, n, density_only)
    assert head["bytes"] == nbytes and head["p_cap"] == (n + 255) // 256 * 256 and not sun and "dy_in" not in head
    ws = wg.Guarded("workspace", nbytes, "cuda", fill=0xFF)
    x = _rand((n, 3), 11)
    sun_dir = _rand((n, 3), 12)
    img = torch.randint(0, N_IMG, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(13))
    shapes = [(n,)] if density_only else [(n,), (n, 3), (n, 3), (n,), (n,)]
    gs = [_rand(s, 20 + k) for k, s in enumerate(shapes)]
    if live is not None:
        keep = torch.zeros(n, device="cuda")
        keep[live] = 1.0
        gs = [g * (keep if g.dim() == 1 else keep[:, None]) for g in gs]
    gs = gs + [None] * (5 - len(gs))
    outs = [wg.Guarded(k, 4 * m, "cuda") for k, m in (("sigma", n), ("albedo", 3 * n), ("ambient", 3 * n), ("ts", n), ("tb", n))]
    heads = [None] * 4 if density_only else outs[1:]
    d_flat = torch.zeros(int(L().eonerf_grad_floats(ctx)), device="cuda")
    d_xyz = wg.Guarded("d_xyz", 12 * n, "cuda")
    rc = L().eonerf_field_forward_train(ctx, P(f._flat), P(x), P(None if density_only else sun_dir), P(None if density_only else img), n, density_only,
                                        P(outs[0]), *(P(h) for h in heads), C.c_void_p(ws.ptr), nbytes, None)
    assert rc == 0, rc
    rc = L().eonerf_field_backward(ctx, P(f._flat), P(None if density_only else sun_dir), n, density_only, *(P(g) for g in gs), P(d_flat), P(d_xyz),
                                   C.c_void_p(ws.ptr), nbytes, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert L().eonerf_device_status(ctx, None) == 0
    wg.check_guards("field pair", [ws, d_xyz] + outs)
    ps = sc.Pass(ws.payload, off, head["p_cap"], n, precision, not density_only)
    m_bott = ws.payload[head["m_bott"]:head["m_bott"] + 4 * sr.K()["BOTT_SCRATCH_F"]].view(F32)
    return f, ps, grad_views(f, d_flat), m_bott, (x, img, gs, d_xyz)


FIELD_N = [1, 31, 32, 33, 255, 256, 257, 300, 1000]


@pytest.mark.parametrize("n", FIELD_N)
@pytest.mark.parametrize("density_only", [0, 1])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_field_pair_exact(precision, density_only, n):
    """Training forward chain, the complete backward chain with the input-gradient tail, every GEMM job with the riders and the products
    that follow from the bottleneck factors: dense random upstream gradients, points in [-1, 1]^3, image indices over all images."""
    f, ps, grads, m_bott, (x, img, gs, d_xyz) = run_field_pair(precision, density_only, n)
    case = f"field[{precision}-density_only{density_only}-n{n}]"
    # the per-sample arrays the checks start from are the call's own inputs
    assert torch.equal(ps.xyz().t().float(), x) and (density_only or torch.equal(ps.simg(), img))
    assert torch.equal(ps.f32("g_sigma")[0].float(), gs[0])
    res = sc.check_field_pair(ps, _params(precision), grads, m_bott)
    res.append(sc.compare("d_xyz == g_pos", d_xyz.view(F32, n, 3).t(), ps.f32("g_pos", 3), torch.zeros(3, n, device="cuda", dtype=torch.float64)))
    record(res, case, "field " + precision)


def multi_round_samples(n):
    """More than the 65,536 samples one round of 256 workgroups covers (bf16: 256 samples per workgroup; fp32: 32,768 per round, so the
    same n is more than three rounds there), ending in the evenly dealt partial tail round of TileSched.  Samples with non-zero upstream
    gradients: 0 and n - 1, every sample of the last partial 32-sample tile, the first and last sample of the first and of the last
    256-sample tile of the second round, 64 random ones."""
    assert n > 65536 + 256 and n % 32
    last_tile = (n - 1) // 256 * 256
    chosen = {0, n - 1, 65536, 65536 + 255, last_tile, min(last_tile + 255, n - 1)} | set(range(n // 32 * 32, n))
    g = torch.Generator().manual_seed(5)
    chosen |= set(int(v) for v in torch.randint(0, n, (64,), generator=g))
    return torch.tensor(sorted(chosen), device="cuda")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_field_pair_multi_round(precision):
    """n = 100,037, full model.  The per-sample checks run on all samples.  For the weight gradients a dense upstream gradient would make
    the elementwise bound gamma(n + 257) S too slack to see one missing tile, so the upstream gradients are non-zero on ~100 chosen samples
    only: dY is then exactly zero elsewhere (asserted), n_nz is about a hundred, and a tile the GEMM skipped loses all of its contribution."""
    n = 100037
    live = multi_round_samples(n)
    f, ps, grads, m_bott, _ = run_field_pair(precision, 0, n, live)
    c = sr.K()
    allowed = torch.zeros(n, dtype=torch.bool, device="cuda")
    allowed[live] = True
    for row in list(range(0, c["GRD_ROW_SIG"], 256)) + [c["GRD_ROW_A1"], c["GRD_ROW_T1"] + 128, c["GRD_ROW_T1"] + 256, c["GRD_ROW_T1"] + 384]:
        blk = sr.grd_block(row)
        nz = (ps.grd(blk[0], blk[1]) != 0).any(0)
        assert not bool((nz & ~allowed).any()), f"dY rows {blk[0]}..: non-zero at a sample without an upstream gradient"
        assert int(nz.sum()) > live.numel() // 2
    for row, k in ((c["GRD_ROW_SIG"], 1), (c["GRD_ROW_A2"], 3), (c["GRD_ROW_T5"], 2)):
        assert not bool(((ps.grd(row, k) != 0).any(0) & ~allowed).any())
    record(sc.check_field_pair(ps, _params(precision), grads, m_bott), f"field[{precision}-n{n}-sparse upstream]", "field " + precision)


# ------------------------------------------------------------------------------------------------------------ render step, pipelined path
SHADOWS, TRAIN = 1, 4


@pytest.mark.parametrize("R", [1, 37, 300])
def test_render_step_pipelined_exact(R):
    """eonerf_render_forward + eonerf_render_backward_loss (kind 1: the uncertainty loss of epoch 3, with the shadow pass) on a bf16 context
    created with EONERF_PIPE=1, default atomic mode, 128 samples per ray, fixed noise buffers.

      * forward slab checks on the camera pass (full model) and on the sun pass (density only);
      * the camera heads chain (k_mlp_bwd PIPE 1): the head dY rows in the slab, and dY_7 as it lies in pipe.dy_in in unit order;
      * k_bwd_pipe where its operands exist.  The two pipelined launches of a backward call share pipe.dy_in and the camera's runs last:
        after the call dy_in holds the CAMERA pass' dY_7 only, while dW_7 in the gradient buffer is the sum of both passes -- the layout does
        not allow dW_7 = dY_7 X_7^T.  It allows the other route: dY_5 of both passes lies in its pass' slab (unit order), so
        dW_5[:, :256] = sum over the passes of dY_5 X_5^T and db_5 are checked;
      * k_enc_pair + k_step_tail: dW_0, db_0 and dW_5[:, 256:319] = the camera pass' product (a GEMM job on unit-order tiles) plus the sun
        pass' product (per-workgroup partials, summed by the tail kernel) against the encoding, and the sun pass' g_pos from its dY_0 / dY_5;
      * the remaining GEMM jobs of the camera pass (sigma rows of both passes, A2, the embedding columns, T2..T4, ts / tb), the bottleneck
        factors and what follows from them, the embedding table.
    Layers 6 and 4..1 of the pipeline stay with the 1e-4 tie to chain + GEMM (tests/test_bwd_pipe.py), which the field cases above anchor."""
    from eonerf_code_amd.synthetic import synthetic_batch
    f = _field("bf16", True)
    f.set_n_samples(128)
    ctx, flags = f._ctx, TRAIN | SHADOWS
    nbytes = int(L().eonerf_render_workspace_bytes(ctx, R, flags))
    head, cam, sun = layout(ctx, KIND_RENDER, R, flags)
    assert head["bytes"] == nbytes and "dy_in" in head and "enc_part" in head and "act" in sun and "g_pos" in sun and "g_pos" not in cam
    p_cap = head["p_cap"]
    ws = wg.Guarded("workspace", nbytes, "cuda", fill=0xFF)
    rays, img, pix = (t.cuda().contiguous() for t in synthetic_batch(R, N_IMG, seed=3))
    z = torch.linspace(0, 1, 128, device="cuda")
    u = [_rand((R, 128), 40 + k, 0.0, 1.0) for k in range(3)]
    out, n_dev, loss = wg.Guarded("out", 4 * R * 21, "cuda"), wg.Guarded("n_samples_dev", 4, "cuda"), wg.Guarded("loss", 4, "cuda")
    d_flat = torch.zeros(int(L().eonerf_grad_floats(ctx)), device="cuda")
    w = C.c_void_p(ws.ptr)
    rc = L().eonerf_render_forward(ctx, P(f._flat), P(rays), P(img), P(z), P(u[0]), P(u[1]), P(u[2]), R, flags, P(out), P(n_dev), w, nbytes, None)
    assert rc == 0, rc
    rc = L().eonerf_render_backward_loss(ctx, P(f._flat), P(rays), P(img), R, flags, P(out), P(pix), 1, None, P(loss), P(d_flat), w, nbytes, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert L().eonerf_device_status(ctx, None) == 0
    wg.check_guards("render step", [ws, out, n_dev, loss])
    raw = ws.payload
    n_cam = int(raw[cam["n_pts"]:cam["n_pts"] + 4].view(torch.int32)[0])
    n_sun = int(raw[sun["n_pts"]:sun["n_pts"] + 4].view(torch.int32)[0])
    assert 0 < n_cam <= p_cap and 0 < n_sun <= p_cap, (n_cam, n_sun, p_cap)
    y0 = sr.K()["GRD_ROW_Y0"]
    units = (y0, y0 + 5 * 256)      # dY_0 and dY_5 lie in unit order behind the pipelined launches
    pc = sc.Pass(raw, cam, p_cap, n_cam, "bf16", True, units)
    psun = sc.Pass(raw, sun, p_cap, n_sun, "bf16", False, units)
    pr = _params("bf16")
    case = f"render[bf16-pipe-R{R}]"
    res = []
    for tag, p in ((" (cam)", pc), (" (sun)", psun)):
        part = sc.check_encoding(p) + sc.check_forward(p, pr)
        for w_ in part:
            w_.name += tag
        res += part
    dy7 = sr.decode_units(raw, head["dy_in"], p_cap // 32)[:, :n_cam].double()
    part = sc.check_backward(pc, pr, dy7=dy7, stop_at_dy7=True)
    for w_ in part:
        w_.name += " (cam, heads chain)"
    res += part
    part = sc.check_input_grad(psun, pr)
    part[0].name += " (sun, enc_pair)"
    res += part
    grads = grad_views(f, d_flat)
    m_bott = raw[head["m_bott"]:head["m_bott"] + 4 * sr.K()["BOTT_SCRATCH_F"]].view(F32)
    res += sc.check_weight_gradients([pc, psun], pr, grads, m_bott, trunk=(5,), tag=" (render)")
    record(res, case, "render bf16")
