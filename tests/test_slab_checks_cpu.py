"""CPU: the per-kernel checks of tests/slab_checks.py accept a correct workspace and catch each seeded defect at the right tensor and
location -- a check that cannot fail is worth nothing.

The workspace is synthetic: a torch emulation of the chain (operands rounded to the slab's type, fp32 accumulation, one rounding per stored
value) for n = 300 points, encoded through tests/slab_restated.py at made-up 256-byte aligned offsets.  Also here, because it needs no GPU:
the cap on the folded matrix' ambiguous entries for the seed the GPU tests use."""

import pytest
import torch

from oracle import eonerf_oracle as orc
import slab_checks as sc
import slab_restated as sr

N, N_IMG, SEED = 300, 5, 7
F32 = torch.float32


def _state_dict():
    sd = orc.random_state_dict(N_IMG, seed=SEED, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    return sd


def emulate(sd, precision, n=N, seed=3):
    """Dense tensors of one full forward + backward pass as the kernels would leave them, and the synthetic workspace / gradients."""
    bf16 = precision == "bf16"
    pr = sc.Params.from_state_dict(sd, precision)
    r = (lambda t: t.to(torch.bfloat16).float()) if bf16 else (lambda t: t.float())      # rounding of a stored value / an operand
    op = lambda name: r(pr.t[name])      # noqa: E731
    bias = lambda name: pr.t[name].reshape(-1, 1)      # noqa: E731
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(3, n, generator=g) * 2 - 1).float()
    img = torch.randint(0, N_IMG, (n,), generator=g)
    c = sr.K()
    cols = sr.enc_col_of_row(precision)
    ref_cols = torch.zeros(63, n)
    for col, (d, k, half) in enumerate(sc._enc_dim_scale()):
        ref_cols[col] = xyz[d] if k < 0 else torch.sin(xyz[d] * float(1 << k) + (sc.PI_2_F if half else 0.0))
    E = r(ref_cols)
    enc_rows = torch.stack([E[k] if k >= 0 else torch.zeros(n) for k in cols])
    act, grd, pre = {}, {}, {}
    x1, y0 = c["ACT_ROW_X1"], c["GRD_ROW_Y0"]
    X = [None] * 9
    for l in range(8):
        inp = E if l == 0 else (torch.cat([X[5], E]) if l == 5 else X[l])
        pre[l] = op(sc.TRUNK % l + ".weight") @ inp + bias(sc.TRUNK % l + ".bias")
        X[l + 1] = r(pre[l].clamp_min(0))
        act[x1 + 256 * l] = X[l + 1]
    f = pr.fold()
    fw, fb = f["op"].float(), f["b"].float().reshape(-1, 1)
    softplus = lambda v: torch.where(v > 20, v, torch.log1p(torch.exp(v.clamp_max(20))))      # noqa: E731
    sigma = softplus(op(sc.SIG + ".weight") @ X[8] + bias(sc.SIG + ".bias"))
    A1 = r((fw[:128] @ X[8] + fb[:128]).clamp_min(0))
    albedo = torch.sigmoid(op(sc.A2 + ".weight") @ A1 + bias(sc.A2 + ".bias"))
    emb = r(pr.t[sc.EMB][img].t())
    T = [None, r((torch.cat([fw[128:], op(sc.TR % 0 + ".weight")[:, 256:260]], 1) @ torch.cat([X[8], emb]) + fb[128:]).clamp_min(0))]
    for l in range(1, 4):
        T.append(r((op(sc.TR % l + ".weight") @ T[l] + bias(sc.TR % l + ".bias")).clamp_min(0)))
    ts = torch.sigmoid(op(sc.TSC + ".weight") @ T[4] + bias(sc.TSC + ".bias"))
    tb = softplus(op(sc.TBE + ".weight") @ T[4] + bias(sc.TBE + ".bias"))
    act[c["ACT_ROW_ENC"]] = enc_rows
    act[c["ACT_ROW_A1"]] = A1
    for l in range(1, 5):
        act[c["ACT_ROW_T1"] + 128 * (l - 1)] = T[l]
    act[c["ACT_ROW_EMB"]] = torch.cat([emb, torch.zeros(28, n)])
    # ---- backward ----
    gs, ga, gts, gtb = (torch.rand(k, n, generator=g) * 2 - 1 for k in (1, 3, 1, 1))
    dsig = r(gs * (1 - torch.exp(-sigma)))
    dalb = r(ga * albedo * (1 - albedo))
    dt5 = r(torch.cat([gts * ts * (1 - ts), gtb * (1 - torch.exp(-tb))]))
    m = lambda t: (t > 0).float()      # noqa: E731
    dT = {4: r(torch.cat([op(sc.TSC + ".weight"), op(sc.TBE + ".weight")]).t() @ dt5 * m(T[4]))}
    for l in (3, 2, 1):
        dT[l] = r(op(sc.TR % l + ".weight").t() @ dT[l + 1] * m(T[l]))
    dA1 = r(op(sc.A2 + ".weight").t() @ dalb * m(A1))
    g_emb = op(sc.TR % 0 + ".weight")[:, 256:260].t() @ dT[1]
    dY = [None] * 8
    dY[7] = r(torch.cat([fw, op(sc.SIG + ".weight")]).t() @ torch.cat([dA1, dT[1], dsig]) * m(X[8]))
    for l in range(6, -1, -1):
        dY[l] = r(op(sc.TRUNK % (l + 1) + ".weight")[:, :256].t() @ dY[l + 1] * m(X[l + 1]))
    denc = op(sc.TRUNK % 5 + ".weight")[:, 256:].t() @ dY[5] + op(sc.TRUNK % 0 + ".weight").t() @ dY[0]
    g_pos = torch.zeros(3, n)
    for col, (d, k, half) in enumerate(sc._enc_dim_scale()):
        dv = torch.ones(n) if k < 0 else float(1 << k) * torch.cos(xyz[d] * float(1 << k) + (sc.PI_2_F if half else 0.0))
        g_pos[d] += denc[col] * dv
    for l in range(8):
        grd[y0 + 256 * l] = dY[l]
    grd[c["GRD_ROW_SIG"]] = torch.cat([dsig, torch.zeros(31, n)])
    grd[c["GRD_ROW_A2"]] = torch.cat([dalb, torch.zeros(29, n)])
    grd[c["GRD_ROW_A1"]] = torch.cat([dA1, dT[1]])
    for l in (2, 3, 4):
        grd[c["GRD_ROW_T1"] + 128 * (l - 1)] = dT[l]
    grd[c["GRD_ROW_T5"]] = torch.cat([dt5, torch.zeros(30, n)])
    # ---- weight gradients (fp32 sums of the stored operands) ----
    G = {}
    G[sc.TRUNK % 0 + ".weight"], G[sc.TRUNK % 0 + ".bias"] = dY[0] @ E.t(), dY[0].sum(1)[None]
    for l in range(1, 8):
        w = dY[l] @ X[l].t()
        G[sc.TRUNK % l + ".weight"], G[sc.TRUNK % l + ".bias"] = (torch.cat([w, dY[5] @ E.t()], 1) if l == 5 else w), dY[l].sum(1)[None]
    G[sc.SIG + ".weight"], G[sc.SIG + ".bias"] = dsig @ X[8].t(), dsig.sum(1)[None]
    G[sc.A2 + ".weight"], G[sc.A2 + ".bias"] = dalb @ A1.t(), dalb.sum(1)[None]
    for l in range(1, 4):
        G[sc.TR % l + ".weight"], G[sc.TR % l + ".bias"] = dT[l + 1] @ T[l].t(), dT[l + 1].sum(1)[None]
    G[sc.TSC + ".weight"], G[sc.TSC + ".bias"] = dt5[:1] @ T[4].t(), dt5[:1].sum(1)[None]
    G[sc.TBE + ".weight"], G[sc.TBE + ".bias"] = dt5[1:] @ T[4].t(), dt5[1:].sum(1)[None]
    dAT = torch.cat([dA1, dT[1]])
    M, db = dAT @ X[8].t(), dAT.sum(1)
    WAT = torch.cat([pr.t[sc.A1 + ".weight"], pr.t[sc.TR % 0 + ".weight"][:, :256]])
    Wb, bb = pr.t[sc.BOT + ".weight"], pr.t[sc.BOT + ".bias"].reshape(-1)
    G[sc.BOT + ".weight"], G[sc.BOT + ".bias"] = WAT.t() @ M, (WAT.t() @ db)[None]
    head = M @ Wb.t() + db[:, None] * bb[None]
    G[sc.A1 + ".weight"], G[sc.A1 + ".bias"] = head[:128], db[None, :128]
    G[sc.TR % 0 + ".weight"], G[sc.TR % 0 + ".bias"] = torch.cat([head[128:], dT[1] @ emb.t()], 1), db[None, 128:]
    G[sc.EMB] = torch.zeros(N_IMG, 4).index_add_(0, img, g_emb.t().contiguous())
    m_bott = torch.cat([M.reshape(-1), db])
    # ---- the synthetic workspace ----
    p_cap = (n + 255) // 256 * 256
    nt = p_cap // sr.seg_samples(precision)
    esz = 2 if bf16 else 4
    sizes = dict(px=4 * p_cap, py=4 * p_cap, pz=4 * p_cap, simg=4 * p_cap, sigma=4 * p_cap, albedo=12 * p_cap, ts=4 * p_cap, tb=4 * p_cap,
                 act=c["ACT_ROWS_FULL"] * p_cap * esz, grd=c["GRD_ROWS_FULL"] * p_cap * esz, g_sigma=4 * p_cap, g_albedo=12 * p_cap,
                 g_ts=4 * p_cap, g_tb=4 * p_cap, g_emb=16 * p_cap, g_pos=12 * p_cap)
    off, at = {}, 512
    for k, v in sizes.items():
        off[k], at = at, (at + v + 255) // 256 * 256 + 256
    ws = torch.full((at,), 0xFF, dtype=torch.uint8)

    def put(name, t):
        sr.soa(ws, off[name], t.shape[0], p_cap)[:, :n] = t
    for name, t in (("px", xyz[0:1]), ("py", xyz[1:2]), ("pz", xyz[2:3]), ("sigma", sigma), ("albedo", albedo), ("ts", ts), ("tb", tb),
                    ("g_sigma", gs), ("g_albedo", ga), ("g_ts", gts), ("g_tb", gtb), ("g_pos", g_pos)):
        put(name, t)
    sr.soa(ws, off["simg"], 1, p_cap, torch.int32)[0, :n] = img.int()
    ws[off["g_emb"]:off["g_emb"] + 16 * p_cap].view(F32).view(p_cap, 4)[:n] = g_emb.t()
    for which, rows, blk in (("act", act, sr.act_block), ("grd", grd, sr.grd_block)):
        for row, t in rows.items():
            s, nr = blk(row)
            dense = sr.decode_block(ws, off[which], s, nr, nt, precision).clone()
            dense[row - s:row - s + t.shape[0], :n] = t.to(dense.dtype)
            sr.encode_block(ws, off[which], s, nr, nt, precision, dense)
    return dict(ws=ws, off=off, p_cap=p_cap, n=n, precision=precision, pr=pr, grads=G, m_bott=m_bott, pre=pre, X=X, dY=dY)


@pytest.fixture(scope="module")
def clean_bf16():
    return emulate(_state_dict(), "bf16")


def _run(w):
    ps = sc.Pass(w["ws"], w["off"], w["p_cap"], w["n"], w["precision"], True)
    return sc.check_field_pair(ps, w["pr"], w["grads"], w["m_bott"])


def _seeded(clean):
    w = dict(clean)
    w["ws"] = clean["ws"].clone()
    w["grads"] = {k: v.clone() for k, v in clean["grads"].items()}
    return w


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_clean_workspace_passes(precision, clean_bf16):
    w = clean_bf16 if precision == "bf16" else emulate(_state_dict(), "fp32")
    res = _run(w)
    assert len(res) > 60
    assert not sc.failures(res), sc.failures(res)
    assert all(r.ratio == r.ratio for r in res)


def test_ambiguity_cap_holds_for_the_seeds_in_use():
    """Fewer than 1 % of the folded matrix is ambiguous (Params.fold) for the state dict of the GPU tests."""
    for seed in (SEED,):
        sd = orc.random_state_dict(N_IMG, seed=seed, bias_scale=0.05)
        f = sc.Params.from_state_dict(sd, "bf16").fold()
        assert 0 < f["amb_frac"] < 0.01, f["amb_frac"]
        # the emulated fp32 fold is the fp32 product up to summation order: within gamma(257) S of the float64 product
        L = torch.cat([sd[sc.A1 + ".weight"], sd[sc.TR % 0 + ".weight"][:, :256]]).double()
        assert bool(((f["W"] - L @ sd[sc.BOT + ".weight"].double()).abs() <= sc.gamma(257) * f["S"]).all())


def _named(res, name):
    hit = [r for r in sc.failures(res) if r.name == name]
    assert hit, (name, sc.failures(res)[:5])
    return hit[0]


def test_zeroed_segment_is_caught(clean_bf16):
    w, c = _seeded(clean_bf16), sr.K()
    row0, tile = c["ACT_ROW_X1"] + 256 * 2, 4                     # X_3, samples 128..159
    r = int(torch.argmax(clean_bf16["X"][3][:, 128:160].sum(1)))
    b = w["off"]["act"] + sr.segment_offset(sr.act_block(row0), row0 + r, tile, w["p_cap"] // 32)
    w["ws"][b:b + 64] = 0
    hit = _named(_run(w), "X_3")
    assert hit.row == row0 + r and 128 <= hit.sample < 160, hit


def test_four_rows_of_a_tile_from_another_tile_are_caught(clean_bf16):
    """Rows 28..31 of one 32-row tile of one sample tile overwritten (the defect csrc/eonerf_common.h records for the 128-bit slab store)."""
    w, c = _seeded(clean_bf16), sr.K()
    row0, nt = c["GRD_ROW_Y0"] + 256 * 3, w["p_cap"] // 32         # dY_3, m-tile 2, sample tile 5 <- sample tile 6
    for r in range(28, 32):
        dst = w["off"]["grd"] + sr.segment_offset(sr.grd_block(row0), row0 + 64 + r, 5, nt)
        src = w["off"]["grd"] + sr.segment_offset(sr.grd_block(row0), row0 + 64 + r, 6, nt)
        w["ws"][dst:dst + 64] = w["ws"][src:src + 64].clone()
    hit = _named(_run(w), "dY_3")
    assert row0 + 64 + 28 <= hit.row < row0 + 64 + 32 and 160 <= hit.sample < 192, hit


def test_missing_sample_and_missing_tile_in_a_weight_gradient_are_caught(clean_bf16):
    for lo, hi in ((77, 78), (256, 288)):
        w = _seeded(clean_bf16)
        name = sc.TRUNK % 2 + ".weight"
        w["grads"][name] -= clean_bf16["dY"][2][:, lo:hi] @ clean_bf16["X"][2][:, lo:hi].t()
        res = _run(w)
        _named(res, "dW 2")
        assert [r.name for r in sc.failures(res)] == ["dW 2"], sc.failures(res)


def test_two_bf16_ulps_are_caught(clean_bf16):
    w, c = _seeded(clean_bf16), sr.K()
    X6 = clean_bf16["X"][6]
    p = 201
    r = int(torch.argmax(X6[:, p]))
    row0 = c["ACT_ROW_X1"] + 256 * 5
    b = w["off"]["act"] + sr.segment_offset(sr.act_block(row0), row0 + r, p // 32, w["p_cap"] // 32) + 2 * (p % 32)
    w["ws"][b:b + 2].view(torch.int16).add_(2)                   # two ulps up (a positive bf16: the bit pattern is monotonic)
    hit = _named(_run(w), "X_6")
    assert (hit.row, hit.sample) == (row0 + r, p), hit


def test_flipped_relu_derivative_is_caught(clean_bf16):
    """An element of dY_4 whose ReLU' is 0 (pre-activation of layer 4 well below zero) receives the unmasked value."""
    w, c = _seeded(clean_bf16), sr.K()
    p = 150
    unmasked = (w["pr"].op(sc.TRUNK % 5 + ".weight")[:, :256].t() @ clean_bf16["dY"][5].double())[:, p]
    cand = torch.where(clean_bf16["pre"][4][:, p] < -0.05, unmasked.abs(), torch.zeros(256, dtype=torch.float64))
    r = int(torch.argmax(cand))
    assert cand[r] > 0 and clean_bf16["X"][5][r, p] == 0
    row0 = c["GRD_ROW_Y0"] + 256 * 4
    b = w["off"]["grd"] + sr.segment_offset(sr.grd_block(row0), row0 + r, p // 32, w["p_cap"] // 32) + 2 * (p % 32)
    w["ws"][b:b + 2].view(torch.bfloat16)[0] = float(unmasked[r])
    hit = _named(_run(w), "dY_4")
    assert (hit.row, hit.sample) == (row0 + r, p) and hit.bound == 0.0, hit


def test_scaled_input_gradient_is_caught(clean_bf16):
    w = _seeded(clean_bf16)
    p = 33
    sr.soa(w["ws"], w["off"]["g_pos"], 3, w["p_cap"])[:, p] *= 1.01
    res = _run(w)
    hit = _named(res, "g_pos")
    assert hit.sample == p and [r.name for r in sc.failures(res)] == ["g_pos"], sc.failures(res)


def test_unit_order_blocks_are_read_as_the_pipelined_path_leaves_them(clean_bf16):
    """dY_0 and dY_5 re-encoded in B-operand unit order (where the pipelined launches leave them): the checks that read them pass through
    Pass(unit_blocks=...), fail when the blocks are taken for feature-major ones, and catch two exchanged k-groups of one step."""
    w, c = _seeded(clean_bf16), sr.K()
    y0, nt = c["GRD_ROW_Y0"], clean_bf16["p_cap"] // 32
    for l in (0, 5):
        dense = sr.decode_block(w["ws"], w["off"]["grd"], y0 + 256 * l, 256, nt, "bf16").clone()
        dense[:, w["n"]:] = 0
        sr.encode_units(w["ws"], w["off"]["grd"] + (y0 + 256 * l) * nt * c["SEG_B"], nt, dense)

    def run(ws, units):
        ps = sc.Pass(ws, w["off"], w["p_cap"], w["n"], "bf16", True, units)
        return sc.check_input_grad(ps, w["pr"]) + sc.check_weight_gradients([ps], w["pr"], w["grads"], w["m_bott"], trunk=(5,))
    units = (y0, y0 + 5 * 256)
    assert not sc.failures(run(w["ws"], units))
    assert {"g_pos", "dW 0", "dW 5"} <= {r.name for r in sc.failures(run(w["ws"], ()))}
    bad = w["ws"].clone()
    step = w["off"]["grd"] + (y0 + 5 * 256) * nt * c["SEG_B"] + 3 * c["PIPE_UNIT_B"]      # dY_5, samples 96..127: k-groups 2 and 9 exchanged
    bad[step + 2 * 1024:step + 3 * 1024], bad[step + 9 * 1024:step + 10 * 1024] = w["ws"][step + 9 * 1024:step + 10 * 1024], w["ws"][step + 2 * 1024:step + 3 * 1024]
    res = run(bad, units)
    hit = _named(res, "g_pos")
    assert 96 <= hit.sample < 128, hit
    _named(res, "dW 5")
