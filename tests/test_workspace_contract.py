"""GPU: the workspace contract of the C ABI (include/eonerf_hip.h), checked from outside with the sizes the ABI itself reports.

  * "the caller must pass eonerf_*_workspace_bytes() bytes": every call runs on a workspace of EXACTLY that size, and on output buffers
    of exactly the documented capacity, each between two guards (tests/workspace_guard.py: [guard | payload | guard], guards of
    2,850,816 B -- one 256-sample granule of the widest slab, derived from the headers' constants in workspace_guard.guard_bytes).  After
    the call every guard byte still holds its fill: no kernel stores outside what the caller owns.
  * "nothing else is remembered between calls": every case runs three times, on a workspace of zero bytes (Z, the baseline), of 0xFF
    bytes (F: fp32 / bf16 / fp16 NaN, int -1) and on what a LARGER call of the same kind with another batch and another seed left behind
    (S; one allocation of the larger call's size serves both, and the part behind the smaller call's size must come back unchanged).
    F and S reproduce Z's outputs bit for bit.  Outputs are pre-filled with 0xFF (NaN / -1); everything the header says is written comes
    back finite.
  * a workspace one byte short is refused with EONERF_E_WORKSPACE before anything is launched: payloads and outputs keep their fill.

Gradients.  The render entry points run on contexts created under EONERF_DETERMINISTIC=1 (fixed-order sums): d_flat_params is bit
identical across Z / F / S.  One case per precision at the bench size runs in the default mode (atomic sums): finite, and each tensor within
1e-4 relative L2 of Z -- the project's bound for "summation order only" (tests/test_bwd_pipe.py, tests/test_oracle_fullsize.py).
eonerf_field_backward has no deterministic mode (its weight-gradient GEMM always adds its work items atomically; the switch only serves
the render path's partial buffers, which the field layout does not carve), so its d_flat_params is held to that same 1e-4 bound on every
context, and d_xyz -- one store per point, no sum -- to bit identity.

These tests do not aim at a fault: with correct kernels every access stays inside the test's own allocations and the poison is only data.
The cases are ordered smallest first; run the file with -x."""
import ctypes as C
import functools
import os

import pytest
import torch

from oracle import eonerf_oracle as orc
import workspace_guard as wg

pytestmark = pytest.mark.gpu
N_IMG = 19
E_WORKSPACE, E_STATE, E_UNSUPPORTED = -2, -3, -4
F32, I32, I64 = torch.float32, torch.int32, torch.int64


def P(x):
    if x is None:
        return C.c_void_p(0)
    return C.c_void_p(x.ptr if isinstance(x, wg.Guarded) else x.data_ptr())


def L():
    from eonerf_code_amd import _lib
    return _lib.lib()


def _field(precision, pipe=True, det=False):
    """One native context per (precision, backward path, summation mode); the library reads the switches when the context is created."""
    return _field_cached(precision, bool(pipe), bool(det))


@functools.lru_cache(maxsize=None)
def _field_cached(precision, pipe, det):
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    sd = orc.random_state_dict(N_IMG, seed=7, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    f = EONerfMLP(N_IMG, radiometric_normalization=True, precision=precision)
    f.load_state_dict(sd, strict=True)
    f = f.cuda()
    keys = {"EONERF_PIPE": "1" if pipe else "0", "EONERF_DETERMINISTIC": "1" if det else "0"}
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


class Case:
    """One call (or forward / backward pair) on buffers it owns: `run(ws_ptr, ws_bytes)` launches it and returns the return codes."""

    def __init__(self, call, f, nbytes):
        self.call, self.f, self.nbytes = call, f, int(nbytes)
        self.bufs, self.outs, self.grads, self.written = [], {}, {}, {}
        self.keep = []          # inputs (kept alive)
        self.expect = None      # return codes of run(); None: all zero

    def buf(self, name, dtype, *shape, fill=0xFF, out=True, grad=False, written=None):
        """A guarded buffer of exactly numel x itemsize bytes.  out: compared bit for bit with the baseline; grad: a gradient (mode-dependent
        comparison); written: the part the header says the call writes (default all of it), a function of the tensor."""
        n = 1
        for s in shape:
            n *= s
        b = wg.Guarded(f"{self.call}:{name}", n * torch.empty(0, dtype=dtype).element_size(), "cuda", fill=fill)
        self.bufs.append(b)
        t = b.view(dtype, *shape)
        if grad:
            self.grads[name] = t
        elif out:
            self.outs[name] = t
            self.written[name] = written if written is not None else (lambda x: x)
        return b


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(*shape, device="cuda", generator=g) * scale + shift).contiguous()


# ------------------------------------------------------------------------------------------------------------ the harness
def _finite(name, t):
    if t.dtype in (I32, I64):
        return bool((t >= 0).all())
    return bool(torch.isfinite(t).all())


def _status_clean(case):
    rc = L().eonerf_device_status(case.f._ctx, None)
    assert rc == 0, f"{case.call}: eonerf_device_status returned {rc}"


def contract(make, small, big, grad_mode="exact"):
    """make(*args) -> Case.  Runs make(*small) on Z, F and S workspaces (S: what make(*big) left) and holds F and S to Z."""
    base_outs = base_grads = None
    for state in "ZFS":
        case = make(*small)
        call = f"{case.call}[{state}]"
        extra = []
        if state == "S":
            stale = make(*big)
            assert stale.nbytes >= case.nbytes, (stale.nbytes, case.nbytes)
            ws = wg.Guarded(f"{case.call}:workspace", stale.nbytes, "cuda", fill=0)
            rcs = stale.run(ws.ptr, stale.nbytes)
            torch.cuda.synchronize()
            assert all(rc == 0 for rc in rcs), f"{stale.call} (stale contents): return codes {rcs}"
            _status_clean(stale)
            wg.check_guards(f"{stale.call} (stale contents)", stale.bufs + [ws])
            tail = ws.payload[case.nbytes:].clone()
            extra = stale.bufs
        else:
            ws = wg.Guarded(f"{case.call}:workspace", case.nbytes, "cuda", fill=0x00 if state == "Z" else 0xFF)
        rcs = case.run(ws.ptr, case.nbytes)
        torch.cuda.synchronize()
        if case.expect is not None:
            assert list(rcs) == list(case.expect), f"{call}: return codes {rcs}, documented {case.expect}"
        else:
            assert all(rc == 0 for rc in rcs), f"{call}: return codes {rcs}"
        _status_clean(case)
        wg.check_guards(call, case.bufs + [ws] + extra)
        if state == "S":
            wg.assert_same_bits(call, "the larger allocation behind workspace_bytes", ws.payload[case.nbytes:], tail)
        if case.expect is None:
            for name, t in case.outs.items():
                assert _finite(name, case.written[name](t)), f"{call}: {name} has elements the call did not write (or not finite)"
            for name, t in case.grads.items():
                assert bool(torch.isfinite(t).all()), f"{call}: gradient {name} is not finite"
        outs = {k: v.clone() for k, v in case.outs.items()}
        grads = {k: v.clone() for k, v in case.grads.items()}
        if base_outs is None:
            base_outs, base_grads = outs, grads
        else:
            for name in outs:
                wg.assert_same_bits(call, name, outs[name], base_outs[name])
            for name in grads:
                if grad_mode == "exact" or name.startswith("d_xyz"):
                    wg.assert_same_bits(call, name, grads[name], base_grads[name])
                else:       # atomic sums: summation order only, per parameter tensor
                    n_par = int(L().eonerf_param_floats(case.f._ctx))
                    for (pname, _), a, b in zip(case.f.named_parameters(), case.f.grad_views(base_grads[name][:n_par]), case.f.grad_views(grads[name][:n_par])):
                        err, ref = (a - b).norm().item(), a.norm().item()
                        assert err <= 1e-4 * ref + 1e-10, f"{call}: {name} / {pname}: |diff| {err:.3e} against |Z| {ref:.3e}"
                    wg.assert_same_bits(call, name + " control floats", grads[name][n_par:], base_grads[name][n_par:])
        del ws, case, extra
    torch.cuda.empty_cache()


def undersized(make, args, ws_fill=0x5A):
    """bytes - 1: EONERF_E_WORKSPACE from every call of the case, workspace and outputs exactly as filled (nothing was launched)."""
    case = make(*args)
    ws = wg.Guarded(f"{case.call}:workspace", case.nbytes, "cuda", fill=ws_fill)
    before = [b.payload.clone() for b in case.bufs]
    rcs = case.run(ws.ptr, case.nbytes - 1)
    torch.cuda.synchronize()
    assert rcs and all(rc == E_WORKSPACE for rc in rcs), f"{case.call} with workspace_bytes - 1: return codes {rcs}"
    _status_clean(case)
    wg.check_guards(case.call + " (undersized)", case.bufs + [ws])
    assert bool((ws.payload == ws_fill).all()), f"{case.call}: an undersized call wrote the workspace"
    for b, t in zip(case.bufs, before):
        wg.assert_same_bits(case.call + " (undersized)", b.name, b.payload, t)


# ------------------------------------------------------------------------------------------------------------ field
def _points(n, seed):
    x = _rand((n, 3), seed, 2.0, -1.0)
    sun = _rand((n, 3), seed + 1, 2.0, -1.0)
    g = torch.Generator(device="cuda").manual_seed(seed + 2)
    img = torch.randint(0, N_IMG, (n,), device="cuda", generator=g)
    return x, sun, img


def make_field_forward(precision, n, seed):
    f = _field(precision)
    c = Case(f"eonerf_field_forward[{precision}-n{n}]", f, L().eonerf_field_workspace_bytes(f._ctx, n))
    x, sun, img = c.keep = _points(n, seed)
    o = [c.buf("sigma", F32, n), c.buf("albedo", F32, n, 3), c.buf("ambient", F32, n, 3), c.buf("ts", F32, n), c.buf("tb", F32, n)]
    c.run = lambda ws, nb: [L().eonerf_field_forward(f._ctx, P(f._flat), P(x), P(sun), P(img), n, *(P(b) for b in o), C.c_void_p(ws), nb, None)]
    return c


def make_query_density(precision, n, seed):
    f = _field(precision)
    c = Case(f"eonerf_query_density[{precision}-n{n}]", f, L().eonerf_field_workspace_bytes(f._ctx, n))
    x, _, _ = c.keep = _points(n, seed)
    sigma = c.buf("sigma", F32, n)
    c.run = lambda ws, nb: [L().eonerf_query_density(f._ctx, P(f._flat), P(x), n, P(sigma), C.c_void_p(ws), nb, None)]
    return c


def make_field_autograd(precision, n, density_only, seed):
    f = _field(precision, det=True)
    ctx = f._ctx
    c = Case(f"eonerf_field_forward_train+backward[{precision}-n{n}-density_only{density_only}]", f,
             L().eonerf_field_train_workspace_bytes(ctx, n, density_only))
    x, sun, img = _points(n, seed)
    sigma = c.buf("sigma", F32, n)
    if density_only:
        heads, gs = [None] * 4, [_rand((n,), seed + 3, 2.0, -1.0)] + [None] * 4
    else:
        heads = [c.buf("albedo", F32, n, 3), c.buf("ambient", F32, n, 3), c.buf("ts", F32, n), c.buf("tb", F32, n)]
        gs = [_rand(s, seed + 3 + k, 2.0, -1.0) for k, s in enumerate([(n,), (n, 3), (n, 3), (n,), (n,)])]
    c.keep = (x, sun, img, gs)
    n_grad = int(L().eonerf_grad_floats(ctx))
    d_flat = c.buf("d_flat_params", F32, n_grad, fill=0, grad=True)      # gradients are ACCUMULATED: the message starts at zero
    d_xyz = c.buf("d_xyz", F32, n, 3, grad=True)

    def run(ws, nb):
        rc = [L().eonerf_field_forward_train(ctx, P(f._flat), P(x), P(None if density_only else sun), P(None if density_only else img), n, density_only,
                                             P(sigma), *(P(h) for h in heads), C.c_void_p(ws), nb, None)]
        rc.append(L().eonerf_field_backward(ctx, P(f._flat), P(None if density_only else sun), n, density_only, *(P(g) for g in gs),
                                            P(d_flat), P(d_xyz), C.c_void_p(ws), nb, None))
        return rc
    c.run = run
    return c


FIELD_N = [1, 255, 256, 257, 1000]


@pytest.mark.parametrize("n", FIELD_N)
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x3"])
def test_field_forward_and_query_density(precision, n):
    contract(make_field_forward, (precision, n, 5), (precision, 2 * n + 300, 105))
    contract(make_query_density, (precision, n, 5), (precision, 2 * n + 300, 105))


@pytest.mark.parametrize("n", FIELD_N)
@pytest.mark.parametrize("density_only", [0, 1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_field_autograd_pair(precision, density_only, n):
    contract(make_field_autograd, (precision, n, density_only, 5), (precision, 2 * n + 300, density_only, 105), grad_mode="atomic")


# ------------------------------------------------------------------------------------------------------------ rays
def _batch(R, seed, kind="plain"):
    """rays[R,11], img[R], pixels[R,3]; kind "mixed": every second ray keeps no sample, "empty": no ray keeps one (origins far outside the
    cube, what filter_pts_outside_cube can leave: tests/test_hip_forward.py, tests/test_bwd_pipe.py)."""
    from eonerf_code_amd.synthetic import synthetic_batch
    rays, img, pix = (t.cuda().contiguous() for t in synthetic_batch(R, N_IMG, seed=seed))
    if kind == "mixed":
        rays[::2, 0] = 5.0
    elif kind == "empty":
        rays[:, 0] = 5.0
    return rays.contiguous(), img, pix


def _zsteps(ns):
    return torch.linspace(0, 1, ns, device="cuda")


def _set_ns(f, ns):
    f.set_n_samples(ns)
    assert f._n_samples == ns


def make_sampler(R, ns, perturb, seed, kind="plain", noise=True):
    f = _field("fp32")
    _set_ns(f, ns)
    ctx = f._ctx
    c = Case(f"eonerf_sample_rays[R{R}-ns{ns}-perturb{perturb}-{kind}{'' if noise else '-philox'}]", f,
             L().eonerf_render_workspace_bytes(ctx, R, 8))      # EONERF_F_ONLY_DEPTH: the layout the entry point carves
    rays, _, _ = _batch(R, seed, kind)
    z, u = _zsteps(ns), (_rand((R, ns), seed + 1) if noise else None)
    c.keep = (rays, z, u)
    cap = R * (ns - 1)
    n_dev = c.buf("n_dev", I32, 1)
    live = lambda t: t[:int(n_dev.view(I32, 1)[0])]            # noqa: E731  (the first *n_dev of the capacity are written)
    ri, t0, t1 = c.buf("ray_indices", I64, cap, written=live), c.buf("t_starts", F32, cap, written=live), c.buf("t_ends", F32, cap, written=live)
    ppr = c.buf("pts_per_ray", F32, R)

    def run(ws, nb):
        _set_ns(f, ns)
        if not noise:
            assert L().eonerf_set_noise_seed(ctx, 1234) == 0
        return [L().eonerf_sample_rays(ctx, P(rays), P(z), P(u), perturb, R, P(ri), P(t0), P(t1), P(ppr), P(n_dev), C.c_void_p(ws), nb, None)]
    c.run = run
    c.samples = (rays, ri, t0, t1, n_dev)
    return c


@pytest.mark.parametrize("ns", [2, 3, 37, 128, 255, 256])
@pytest.mark.parametrize("R", [1, 37, 300])
def test_sampler(R, ns):
    for perturb in (0, 1):
        contract(make_sampler, (R, ns, perturb, 3), (R + 40, ns, perturb, 103))
    if R == 37:
        contract(make_sampler, (R, ns, 1, 3, "mixed"), (R + 40, ns, 1, 103))
        contract(make_sampler, (R, ns, 1, 3, "empty"), (R + 40, ns, 1, 103))
        contract(make_sampler, (R, ns, 1, 3, "plain", False), (R + 40, ns, 1, 103, "plain", False))      # jitter drawn in the kernel
        undersized(make_sampler, (R, ns, 1, 3))


def _samples(R, ns, seed, kind):
    """The sampler's own output for this batch (computed once, on a private workspace): the input of the rendering entry points."""
    s = make_sampler(R, ns, 1, seed, kind)
    ws = wg.Guarded("sampler workspace", s.nbytes, "cuda", fill=0)
    assert s.run(ws.ptr, s.nbytes) == [0]
    torch.cuda.synchronize()
    rays, ri, t0, t1, n_dev = s.samples
    n = int(n_dev.view(I32, 1)[0])
    return n, ri.view(I64, -1)[:n].clone(), t0.view(F32, -1)[:n].clone(), t1.view(F32, -1)[:n].clone()


def make_rendering(precision, R, ns, depth_only, train, seed, kind="plain"):
    f = _field(precision, det=True) if train else _field(precision)
    _set_ns(f, ns)
    ctx = f._ctx
    flags = (4 if train else 0) | (8 if depth_only else 0)
    name = "eonerf_rendering_train+backward" if train else "eonerf_rendering"
    c = Case(f"{name}[{precision}-R{R}-ns{ns}-depth_only{depth_only}-{kind}]", f, L().eonerf_render_workspace_bytes(ctx, R, flags))
    rays, img, _ = _batch(R, seed, kind)
    n, ri, t0, t1 = _samples(R, ns, seed, kind)
    _set_ns(f, ns)
    depth = c.buf("depth", F32, R)
    if depth_only:
        o, g = [None, depth, None, None, None, None], [None, _rand((R,), seed + 5, 2.0, -1.0), None, None, None]
    else:
        o = [c.buf("albedo", F32, R, 3), depth, c.buf("beta", F32, R), c.buf("transient_s", F32, R), c.buf("ambient", F32, R, 3), c.buf("entropy", F32, R)]
        g = [_rand(s, seed + 5 + k, 2.0, -1.0) for k, s in enumerate([(R, 3), (R,), (R,), (R,), (R, 3)])]
    c.keep = (rays, img, ri, t0, t1, g)
    d_flat = c.buf("d_flat_params", F32, int(L().eonerf_grad_floats(ctx)), fill=0, grad=True) if train else None

    def run(ws, nb):
        _set_ns(f, ns)
        fn = L().eonerf_rendering_train if train else L().eonerf_rendering
        rc = [fn(ctx, P(f._flat), P(rays), P(img), P(t0), P(t1), P(ri), n, R, depth_only, *(P(b) for b in o), C.c_void_p(ws), nb, None)]
        if train:
            rc.append(L().eonerf_rendering_backward(ctx, P(f._flat), P(rays), P(img), R, depth_only, *(P(t) for t in g), P(d_flat), C.c_void_p(ws), nb, None))
        return rc
    c.run = run
    return c


@pytest.mark.parametrize("R", [1, 37, 300])
@pytest.mark.parametrize("depth_only", [0, 1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rendering_on_the_samplers_output(precision, depth_only, R):
    for train in (0, 1):
        contract(make_rendering, (precision, R, 128, depth_only, train, 3), (precision, R + 40, 128, depth_only, train, 103))
    if R == 37:
        for kind in ("mixed", "empty"):
            for train in (0, 1):
                contract(make_rendering, (precision, R, 128, depth_only, train, 3, kind), (precision, R + 40, 128, depth_only, train, 103))
        for train in (0, 1):
            undersized(make_rendering, (precision, R, 128, depth_only, train, 3))


# ------------------------------------------------------------------------------------------------------------ render step
SHADOWS, EVAL, TRAIN, ONLY_DEPTH, RGB_LOSS = 1, 2, 4, 8, 16


def _flag_name(flags):
    return "|".join(n for b, n in ((TRAIN, "TRAIN"), (SHADOWS, "SHADOWS"), (EVAL, "EVAL"), (ONLY_DEPTH, "ONLY_DEPTH"), (RGB_LOSS, "RGB_LOSS")) if flags & b) or "0"


def _out_written(flags):
    # out[R,21] = rgb3 depth1 albedo3 ambient3 geo1 ts1 beta1 entropy1 pts1 sc_pts1 opacity2 shadowless3; ONLY_DEPTH: out[:,3] only
    return (lambda t: t[:, 3]) if flags & ONLY_DEPTH else (lambda t: t)


def make_render_forward(precision, R, ns, flags, seed, kind="plain", noise=True, presample=False, pipe=True, det=False):
    f = _field(precision, pipe, det)
    _set_ns(f, ns)
    ctx = f._ctx
    c = Case(f"eonerf_render_forward[{precision}-R{R}-ns{ns}-{_flag_name(flags)}-{kind}{'' if noise else '-philox'}{'-presample' if presample else ''}]", f,
             L().eonerf_render_workspace_bytes(ctx, R, flags))
    rays, img, pix = _batch(R, seed, kind)
    z = _zsteps(ns)
    u = [_rand((R, ns), seed + 1 + k) for k in range(3)] if noise else [None] * 3
    if noise and kind == "plain" and R % 2:
        u[1] = None                                            # u_retry may be NULL: the resample branch is not armed
    c.keep = (rays, img, pix, z, u)
    out = c.buf("out", F32, R, 21, written=_out_written(flags))
    n_dev = c.buf("n_samples_dev", I32, 1)
    c.io = (rays, img, pix, out)

    def run(ws, nb):
        _set_ns(f, ns)
        rc = []
        if not noise:
            assert L().eonerf_set_noise_seed(ctx, 4321) == 0
        if presample:
            rc.append(L().eonerf_presample(ctx, P(rays), P(img), P(z), R, flags, P(n_dev), C.c_void_p(ws), nb, None))
        rc.append(L().eonerf_render_forward(ctx, P(f._flat), P(rays), P(img), P(z), P(u[0]), P(u[1]), P(u[2]), R, flags, P(out), P(n_dev),
                                            C.c_void_p(ws), nb, None))
        return rc
    c.run = run
    return c


def make_render_step(precision, pipe, det, R, ns, flags, seed, kind="plain", noise=True, presample=False):
    """forward(TRAIN) -> eonerf_render_backward(d_out) -> eonerf_render_backward_loss(kind 0 [, kind 1 with the shadow pass]), each backward
    into a gradient message of its own; the backwards share the workspace their forward filled."""
    c = make_render_forward(precision, R, ns, flags, seed, kind, noise, presample, pipe, det)
    c.call = c.call.replace("eonerf_render_forward", f"render step, EONERF_PIPE={int(pipe)}{'' if det else ', atomic sums'}")
    f, ctx, fwd = c.f, c.f._ctx, c.run
    rays, img, pix, out = c.io
    d_out = torch.zeros(R, 21, device="cuda")
    d_out[:, 0:4] = _rand((R, 4), seed + 7, 2.0, -1.0) / R
    if flags & SHADOWS:
        d_out[:, 11:13] = _rand((R, 2), seed + 8, 2.0, -1.0) / R     # (without the shadow pass the ABI wants these two zero: EONERF_F_RGB_LOSS)
    c.keep += (d_out,)
    n_grad = int(L().eonerf_grad_floats(ctx))
    kinds = (0, 1) if flags & SHADOWS else (0,)
    g_plain = c.buf("d_flat_params(render_backward)", F32, n_grad, fill=0, grad=True)
    g_loss = [c.buf(f"d_flat_params(render_backward_loss kind {k})", F32, n_grad, fill=0, grad=True) for k in kinds]
    losses = [c.buf(f"loss kind {k}", F32, 1) for k in kinds]
    # beyond 65,536 rays eonerf_render_backward_loss is eonerf_train_loss + eonerf_render_backward behind each other and wants room for d out
    scratch = c.buf("d_out_scratch", F32, R, 21) if R > 65536 else None

    def run(ws, nb):
        rc = fwd(ws, nb)
        rc.append(L().eonerf_render_backward(ctx, P(f._flat), P(rays), P(img), R, flags, P(d_out), P(g_plain), C.c_void_p(ws), nb, None))
        for k, g, l in zip(kinds, g_loss, losses):
            rc.append(L().eonerf_render_backward_loss(ctx, P(f._flat), P(rays), P(img), R, flags, P(out), P(pix), k, P(scratch), P(l), P(g),
                                                      C.c_void_p(ws), nb, None))
        return rc
    c.run = run
    return c


def _bigger(R):
    return R + max(R // 8, 40)


INFER_FLAGS = [0, SHADOWS, SHADOWS | EVAL, ONLY_DEPTH]


@pytest.mark.parametrize("R", [1, 37, 300, 4096])
@pytest.mark.parametrize("flags", INFER_FLAGS, ids=_flag_name)
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x3"])
def test_render_forward_inference(precision, flags, R):
    contract(make_render_forward, (precision, R, 128, flags, 3), (precision, _bigger(R), 128, flags, 103))
    if R == 37:
        for kind in ("mixed", "empty"):
            contract(make_render_forward, (precision, R, 128, flags, 3, kind), (precision, _bigger(R), 128, flags, 103))
        undersized(make_render_forward, (precision, R, 128, flags, 3))
    if R == 300 and flags == SHADOWS:      # production noise: the sampler kernels draw the jitter themselves
        contract(make_render_forward, (precision, R, 128, flags, 3, "plain", False), (precision, _bigger(R), 128, flags, 103, "plain", False))


TRAIN_CTX = [("fp32", True), ("bf16", True), ("bf16", False)]
TRAIN_IDS = ["fp32", "bf16-pipe1", "bf16-pipe0"]


@pytest.mark.parametrize("R,ns", [(1, 128), (37, 2), (37, 37), (37, 128), (37, 256), (300, 128), (4096, 128)])
@pytest.mark.parametrize("flags", [TRAIN | RGB_LOSS, TRAIN | SHADOWS], ids=_flag_name)
@pytest.mark.parametrize("precision,pipe", TRAIN_CTX, ids=TRAIN_IDS)
def test_render_step_deterministic(precision, pipe, flags, R, ns):
    contract(make_render_step, (precision, pipe, True, R, ns, flags, 3), (precision, pipe, True, _bigger(R), ns, flags, 103))
    if (R, ns) == (37, 128):
        for kind in ("mixed", "empty"):
            contract(make_render_step, (precision, pipe, True, R, ns, flags, 3, kind), (precision, pipe, True, _bigger(R), ns, flags, 103))
        undersized(make_render_step, (precision, pipe, True, R, ns, flags, 3))
        undersized(make_render_step, (precision, pipe, True, R, ns, flags, 3, "plain", False, True))      # eonerf_presample takes workspace_bytes too
        # the production backward (atomic sums: GEMM riders, the shadow pass' encoding partials) on the small ragged batches
        for kind in ("mixed", "empty"):
            contract(make_render_step, (precision, pipe, False, R, ns, flags, 3, kind), (precision, pipe, False, _bigger(R), ns, flags, 103), grad_mode="atomic")
    if (R, ns) == (300, 128):
        # production noise (u_cam == NULL, the seed reset in front of every run), and eonerf_presample ahead of the forward
        contract(make_render_step, (precision, pipe, True, R, ns, flags, 3, "plain", False), (precision, pipe, True, _bigger(R), ns, flags, 103, "plain", False))
        contract(make_render_step, (precision, pipe, True, R, ns, flags, 3, "plain", False, True),
                 (precision, pipe, True, _bigger(R), ns, flags, 103, "plain", False, True))


@pytest.mark.parametrize("flags", [TRAIN | RGB_LOSS, TRAIN | SHADOWS], ids=_flag_name)
@pytest.mark.parametrize("precision,pipe", TRAIN_CTX, ids=TRAIN_IDS)
def test_two_call_loss_path_beyond_65536_rays(precision, pipe, flags):
    """65,537 rays at n_samples = 2 (one interval per ray: a small workspace): eonerf_render_backward_loss runs eonerf_train_loss, which
    writes d_out_scratch and *loss, in front of the backward.  A call the backward refuses -- the workspace one byte short -- must be
    refused before that launch too: d_out_scratch and the loss keep their fill."""
    R = 65537
    undersized(make_render_step, (precision, pipe, True, R, 2, flags, 3))
    if precision == "bf16" and pipe:
        contract(make_render_step, (precision, pipe, True, R, 2, flags, 3), (precision, pipe, True, _bigger(R), 2, flags, 103))


def test_two_call_loss_path_refuses_an_unaddressable_batch_before_the_loss_kernel():
    """fp32, 128 samples per ray: 65,537 rays are beyond the 33,024 a training call addresses (EONERF_E_UNSUPPORTED); nothing is written."""
    R, flags = 65537, TRAIN | RGB_LOSS
    f = _field("fp32", True, True)
    _set_ns(f, 128)
    ctx = f._ctx
    c = Case("eonerf_render_backward_loss[fp32-R65537-ns128]", f, 4096)
    rays, img, pix = _batch(R, 3)
    out = _rand((R, 21), 4)
    scratch, loss, d_flat = c.buf("d_out_scratch", F32, R, 21), c.buf("loss", F32, 1), c.buf("d_flat_params", F32, int(L().eonerf_grad_floats(ctx)))
    ws = wg.Guarded("workspace", c.nbytes, "cuda", fill=0x5A)
    before = [b.payload.clone() for b in c.bufs]
    rc = L().eonerf_render_backward_loss(ctx, P(f._flat), P(rays), P(img), R, flags, P(out), P(pix), 0, P(scratch), P(loss), P(d_flat),
                                         C.c_void_p(ws.ptr), c.nbytes, None)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED, rc
    _status_clean(c)
    wg.check_guards(c.call, c.bufs + [ws])
    assert bool((ws.payload == 0x5A).all())
    for b, t in zip(c.bufs, before):
        wg.assert_same_bits(c.call, b.name, b.payload, t)


def test_contexts_run_in_the_mode_they_were_asked_for():
    """The switches are read when a context is created; what it carves tells which it got: deterministic mode adds the partial-sum buffers,
    the pipelined path its rings, and the default pipelined path the encoding partials of the shadow pass."""
    def size(pipe, det, flags):
        f = _field("bf16", pipe, det)
        _set_ns(f, 128)
        return int(L().eonerf_render_workspace_bytes(f._ctx, 37, flags))

    c = wg.header_constants()
    for flags in (TRAIN | RGB_LOSS, TRAIN | SHADOWS):
        assert size(True, True, flags) > size(False, True, flags) > size(False, False, flags)
        assert size(True, False, flags) > size(False, False, flags)
        assert size(False, True, flags) - size(False, False, flags) >= 4 * c["WGRAD_MAX_JOBS"] * 48 * c["WGRAD_PART_F"]
    assert size(True, False, TRAIN | SHADOWS) - size(True, False, TRAIN | RGB_LOSS) > size(True, True, TRAIN | SHADOWS) - size(True, True, TRAIN | RGB_LOSS)
    # fp32 has no pipelined path: EONERF_PIPE changes nothing there
    assert L().eonerf_render_workspace_bytes(_field("fp32", True, True)._ctx, 37, TRAIN) > L().eonerf_render_workspace_bytes(_field("fp32", True, False)._ctx, 37, TRAIN)


@pytest.mark.parametrize("flags", [TRAIN | RGB_LOSS, TRAIN | SHADOWS], ids=_flag_name)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_render_step_default_mode_at_the_bench_size(precision, flags):
    """Atomic sums (what training runs): finite, and every tensor within 1e-4 relative L2 of the Z run."""
    contract(make_render_step, (precision, True, False, 4096, 128, flags, 3), (precision, True, False, _bigger(4096), 128, flags, 103), grad_mode="atomic")


@pytest.mark.parametrize("precision,pipe", TRAIN_CTX, ids=TRAIN_IDS)
def test_train_with_only_depth_is_refused_before_anything_is_written(precision, pipe):
    """EONERF_F_TRAIN | EONERF_F_ONLY_DEPTH: eonerf_render_forward returns EONERF_E_UNSUPPORTED, eonerf_presample and the backward calls
    EONERF_E_STATE (a depth-only pass under autograd is eonerf_rendering_train's business) -- workspace and outputs keep their fill."""
    R, flags = 37, TRAIN | ONLY_DEPTH
    f = _field(precision, pipe, True)
    _set_ns(f, 128)
    ctx = f._ctx
    rays, img, pix = _batch(R, 3)
    z, u = _zsteps(128), [_rand((R, 128), 4 + k) for k in range(3)]
    c = Case(f"render step[{precision}-TRAIN|ONLY_DEPTH]", f, L().eonerf_render_workspace_bytes(ctx, R, flags))
    assert c.nbytes > 0
    out, n_dev, loss = c.buf("out", F32, R, 21), c.buf("n_samples_dev", I32, 1), c.buf("loss", F32, 1)
    d_flat = c.buf("d_flat_params", F32, int(L().eonerf_grad_floats(ctx)))
    d_out = torch.zeros(R, 21, device="cuda")
    ws = wg.Guarded("workspace", c.nbytes, "cuda", fill=0x5A)
    before = [b.payload.clone() for b in c.bufs]
    w = C.c_void_p(ws.ptr)
    assert L().eonerf_render_forward(ctx, P(f._flat), P(rays), P(img), P(z), P(u[0]), P(u[1]), P(u[2]), R, flags, P(out), P(n_dev), w, c.nbytes, None) == E_UNSUPPORTED
    assert L().eonerf_presample(ctx, P(rays), P(img), P(z), R, flags, P(n_dev), w, c.nbytes, None) == E_STATE
    assert L().eonerf_render_backward(ctx, P(f._flat), P(rays), P(img), R, flags, P(d_out), P(d_flat), w, c.nbytes, None) == E_STATE
    assert L().eonerf_render_backward_loss(ctx, P(f._flat), P(rays), P(img), R, flags, P(out), P(pix), 0, None, P(loss), P(d_flat), w, c.nbytes, None) == E_STATE
    torch.cuda.synchronize()
    _status_clean(c)
    wg.check_guards(c.call, c.bufs + [ws])
    assert bool((ws.payload == 0x5A).all())
    for b, t in zip(c.bufs, before):
        wg.assert_same_bits(c.call, b.name, b.payload, t)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x3"])
def test_undersized_field_workspaces(precision):
    for n in (1, 257):
        undersized(make_field_forward, (precision, n, 5))
        undersized(make_query_density, (precision, n, 5))
        if precision != "fp16x3":
            for density_only in (0, 1):
                undersized(make_field_autograd, (precision, n, density_only, 5))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_field_call_on_what_a_render_step_left_and_the_other_way_round(precision):
    """S across entry points: the two layouts have nothing in common."""
    for first, second in ((make_render_step(precision, True, True, 77, 128, TRAIN | SHADOWS, 103), lambda: make_field_forward(precision, 1000, 5)),
                          (make_field_autograd(precision, 4000, 0, 105), lambda: make_render_step(precision, True, True, 37, 128, TRAIN | SHADOWS, 3))):
        results = []
        for state in "ZS":
            case = second()
            ws = wg.Guarded(f"{case.call}:workspace", max(first.nbytes, case.nbytes), "cuda", fill=0)
            if state == "S":
                assert all(rc == 0 for rc in first.run(ws.ptr, first.nbytes))
            rcs = case.run(ws.ptr, case.nbytes)
            torch.cuda.synchronize()
            assert all(rc == 0 for rc in rcs), (case.call, rcs)
            _status_clean(case)
            wg.check_guards(f"{case.call}[{state} after {first.call}]", case.bufs + first.bufs + [ws])
            results.append({k: v.clone() for k, v in list(case.outs.items()) + list(case.grads.items())})
        for name in results[0]:
            wg.assert_same_bits(f"{case.call}[S after {first.call}]", name, results[1][name], results[0][name])
