"""GPU: eonerf_image_metrics (include/eonerf_metrics.h) through ctypes, against golden G6 (the reference's own outputs) and, for the
sizes G6 does not cover, against the numpy restatement of the contract (tests/metrics_restated.py).

Bounds.  Against G6: 2e-5 relative (fp32 sums of 120 terms in the reference: 120 x 2^-24 = 7e-6, times 3 for the per-term roundings),
1e-4 dB on psnr (10 / ln 10 times the mse bound).  Against the restatement: both sides form the same fp64 terms from the same fp32
inputs, only the order of the fp64 summation differs: n x 2^-53 < 6e-11 for n <= 3 x 131,073 positive terms -> 1e-10 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
import metrics_restated as M
import workspace_guard as wg

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_ARG, E_WORKSPACE = -1, -2
GUARD = 1 << 16                 # the kernels' coarsest step is one partial (32 B) / one packed row (84 B)
SIZES = [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073]      # wave, block and grid-stride boundaries, and a third trip
N_MAX = max(SIZES)


def lib():
    from eonerf_code_amd import _lib
    return _lib.lib()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, offset_floats=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_floats) if t is not None else C.c_void_p(0)


def ws_bytes():
    return lib().eonerf_metrics_workspace_bytes()


def run(pred, gt, beta, n=None, strides=(3, 1, 3), ws=None, result=None, nbytes=None):
    """One call on contiguous fp32 device tensors (or explicit strides) -> (rc, result tensor)."""
    n = pred.shape[0] if n is None else n
    ws = torch.empty(ws_bytes(), dtype=torch.uint8, device=DEV) if ws is None else ws
    result = torch.empty(6, dtype=torch.float64, device=DEV) if result is None else result
    rc = lib().eonerf_image_metrics(ptr(pred), strides[0], ptr(beta), strides[1], ptr(gt), strides[2], n, ptr(result), ptr(ws),
                                    ws.numel() if nbytes is None else nbytes, stream())
    return rc, result


@pytest.fixture(scope="module")
def cloud():
    """131,073 random rays, shared and never written: pred, gt in [0, 1), beta in [0.05, 1.05)."""
    rng = np.random.default_rng(61)
    pred = rng.random((N_MAX, 3), dtype=np.float32)
    gt = rng.random((N_MAX, 3), dtype=np.float32)
    beta = (rng.random((N_MAX, 1), dtype=np.float32) + np.float32(0.05)).astype(np.float32)
    assert beta.min() >= 0.05 and beta.max() < 1.05
    host = {"pred": pred, "gt": gt, "beta": beta}
    return host, {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}


def bits(t):
    return t.view(torch.int64)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
def test_device_matches_golden_g6():
    g = load_golden("g6_metrics")
    assert lib().eonerf_metrics_version() == 1
    pred, gt, beta = (torch.from_numpy(g[k]).to(DEV).contiguous() for k in ("pred", "gt", "beta"))
    rc, out = run(pred, gt, beta)
    assert rc == 0
    out = out.cpu().numpy()
    for k, name in ((0, "unc_loss"), (1, "unc_color"), (2, "unc_logbeta"), (3, "mse"), (3, "mse_torch")):
        r = abs(out[k] - float(g[name])) / abs(float(g[name]))
        print(f"{name}: device {out[k]:.9f}, reference {float(g[name]):.9f}, relative {r:.2e}")
        assert r <= 2e-5, name
    print(f"psnr: device {out[4]:.7f}, reference {float(g['psnr']):.7f}")
    assert abs(out[4] - float(g["psnr"])) <= 1e-4
    assert out[5] == 40
    rc, nob = run(pred, gt, None)
    assert rc == 0
    nob = nob.cpu().numpy()
    assert np.isnan(nob[:3]).all() and nob[3] == out[3] and nob[4] == out[4] and nob[5] == 40


# ---------------------------------------------------------------------------------------------------------------- 2. the contract
@pytest.mark.parametrize("n", SIZES)
def test_device_matches_the_restatement(cloud, n):
    host, dev = cloud
    want = M.image_metrics(host["pred"][:n], host["gt"][:n], host["beta"][:n])
    rc, out = run(dev["pred"], dev["gt"], dev["beta"], n=n)
    assert rc == 0
    out = out.cpu().numpy()
    r = np.abs(out - want) / np.abs(want)
    print(f"n={n}: device {out}, worst relative {r.max():.2e}")
    assert np.isfinite(out).all() and (r <= 1e-10).all()
    assert out[5] == n
    rc, nob = run(dev["pred"], dev["gt"], None, n=n)
    nob = nob.cpu().numpy()
    assert rc == 0 and np.isnan(nob[:3]).all() and (nob[3:] == out[3:]).all()


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_strided_inputs_give_the_same_bits(cloud, n):
    """The packed [n, 21] output of the renderer read in place (rgb = column 0, beta = column 12, stride 21) and a ground truth with a
    row stride of 5 against separate contiguous tensors of the same values."""
    _, dev = cloud
    g = torch.Generator(device=DEV).manual_seed(7)
    packed = torch.randn(n, 21, device=DEV, generator=g)
    packed[:, 0:3], packed[:, 12:13] = dev["pred"][:n], dev["beta"][:n]
    gt5 = torch.randn(n, 5, device=DEV, generator=g)
    gt5[:, 0:3] = dev["gt"][:n]
    rc, base = run(dev["pred"], dev["gt"], dev["beta"], n=n)
    assert rc == 0
    ws = torch.empty(ws_bytes(), dtype=torch.uint8, device=DEV)
    out = torch.empty(6, dtype=torch.float64, device=DEV)
    rc = lib().eonerf_image_metrics(ptr(packed), 21, ptr(packed, 12), 21, ptr(gt5), 5, n, ptr(out), ptr(ws), ws.numel(), stream())
    assert rc == 0
    assert torch.equal(bits(out), bits(base)), (out, base)


# ---------------------------------------------------------------------------------------------------------------- 3. the workspace
def guarded_case(cloud, n):
    _, dev = cloud
    bufs = {}
    for name, cols in (("pred", 3), ("gt", 3), ("beta", 1)):
        b = wg.Guarded(f"metrics:{name}", n * cols * 4, DEV, guard=GUARD)
        b.view(torch.float32, n, cols).copy_(dev[name][:n])
        bufs[name] = b
    bufs["result"] = wg.Guarded("metrics:result", 6 * 8, DEV, guard=GUARD)
    bufs["ws"] = wg.Guarded("metrics:workspace", ws_bytes(), DEV, guard=GUARD)
    return bufs


def guarded_call(b, n, nbytes=None):
    return lib().eonerf_image_metrics(C.c_void_p(b["pred"].ptr), 3, C.c_void_p(b["beta"].ptr), 1, C.c_void_p(b["gt"].ptr), 3, n,
                                      C.c_void_p(b["result"].ptr), C.c_void_p(b["ws"].ptr), b["ws"].nbytes if nbytes is None else nbytes,
                                      stream())


@pytest.mark.parametrize("n", [65, 65537])
def test_result_does_not_depend_on_the_workspace_contents(cloud, n):
    """Zeros, 0xFF bytes (NaN partials) and what a larger call left in the workspace: three runs, one result, no stray write."""
    _, dev = cloud
    b = guarded_case(cloud, n)
    outs = []
    for state in ("zeros", "ones", "stale"):
        if state == "stale":
            rc, _ = run(dev["pred"], dev["gt"], dev["beta"], n=N_MAX, ws=b["ws"].payload)
            assert rc == 0
        else:
            b["ws"].fill(0x00 if state == "zeros" else 0xFF)
        b["result"].fill(0xFF)
        assert guarded_call(b, n) == 0
        outs.append(b["result"].view(torch.float64, 6).clone())
        wg.check_guards(f"eonerf_image_metrics n={n} ({state})", list(b.values()))
    wg.assert_same_bits("eonerf_image_metrics", "result on a 0xFF workspace", outs[1], outs[0])
    wg.assert_same_bits("eonerf_image_metrics", "result on a stale workspace", outs[2], outs[0])
    rc, plain = run(dev["pred"], dev["gt"], dev["beta"], n=n)
    assert rc == 0 and torch.equal(bits(plain), bits(outs[0]))
    assert torch.equal(b["pred"].view(torch.float32, n, 3), dev["pred"][:n])          # inputs untouched


def test_refusals_write_nothing(cloud):
    n = 257
    b = guarded_case(cloud, n)
    b["result"].fill(0x5A)
    b["ws"].fill(0x5A)
    L = lib()
    assert L.eonerf_metrics_workspace_bytes() == 256 * 4 * 8
    assert guarded_call(b, n, nbytes=ws_bytes() - 1) == E_WORKSPACE
    assert guarded_call(b, 0) == E_ARG
    assert guarded_call(b, -5) == E_ARG
    p, be, g, r, w = (C.c_void_p(b[k].ptr) for k in ("pred", "beta", "gt", "result", "ws"))
    nb, st, null = b["ws"].nbytes, stream(), C.c_void_p(0)
    assert L.eonerf_image_metrics(p, 2, be, 1, g, 3, n, r, w, nb, st) == E_ARG           # a stride smaller than the row it addresses
    assert L.eonerf_image_metrics(p, 3, be, 1, g, 2, n, r, w, nb, st) == E_ARG
    assert L.eonerf_image_metrics(p, 3, be, 0, g, 3, n, r, w, nb, st) == E_ARG
    assert L.eonerf_image_metrics(null, 3, be, 1, g, 3, n, r, w, nb, st) == E_ARG
    assert L.eonerf_image_metrics(p, 3, be, 1, null, 3, n, r, w, nb, st) == E_ARG
    assert L.eonerf_image_metrics(p, 3, be, 1, g, 3, n, null, w, nb, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((b["result"].payload == 0x5A).all()) and bool((b["ws"].payload == 0x5A).all())      # nothing was launched
    wg.check_guards("eonerf_image_metrics (refused)", list(b.values()))
    assert L.eonerf_image_metrics(p, 3, null, 0, g, 3, n, r, w, nb, st) == 0             # no beta: its stride is not looked at
    assert guarded_call(b, n) == 0
    assert not bool((b["result"].payload == 0x5A).all())


# ---------------------------------------------------------------------------------------------------------------- 4. edge values
def torch_metrics(pred, gt, beta):
    """metrics.py:17-22,60-69 as the reference evaluates them: fp32 torch on the same tensors."""
    color = ((pred - gt) ** 2 / (2 * beta ** 2)).mean()
    logbeta = (3 + torch.log(beta).mean()) / 2
    mse = ((pred - gt) ** 2).mean()
    return torch.stack([color + logbeta, color, logbeta, mse, -10 * torch.log10(mse)]).cpu().numpy().astype(np.float64)


def pattern(v):
    return ["nan" if np.isnan(x) else "+inf" if x == np.inf else "-inf" if x == -np.inf else "finite" for x in v]


@pytest.mark.parametrize("case,want", [("identical", ["finite", "finite", "finite", "finite", "+inf"]),
                                       ("zero_beta", ["nan", "+inf", "-inf", "finite", "finite"]),
                                       ("nan_pixel", ["nan", "nan", "finite", "nan", "nan"])])
def test_edge_values_follow_torch(cloud, case, want):
    _, dev = cloud
    n = 300
    pred, gt, beta = dev["pred"][:n].clone(), dev["gt"][:n].clone(), dev["beta"][:n].clone()
    if case == "identical":
        pred = gt.clone()
    elif case == "zero_beta":
        beta[70, 0] = 0.0
    else:
        pred[260, 1] = float("nan")
    ref = torch_metrics(pred, gt, beta)
    rc, out = run(pred, gt, beta)
    assert rc == 0
    out = out.cpu().numpy()
    print(f"{case}: device {out[:5]}, torch {ref}")
    assert pattern(ref) == want                  # the fixture does what its name says
    assert pattern(out[:5]) == pattern(ref)
    assert out[5] == n
    if case == "identical":
        assert out[1] == 0.0 and out[3] == 0.0 and out[0] == out[2]
