"""GPU: the sun sweep (include/eonerf_sweep.h, eonerf_code_amd/relight.py) -- K sun directions per view from ONE camera pass.

The contract is bit equality with the shipped path: out[k] of eonerf_render_sun_sweep holds the 21 x R words eonerf_render_forward
(EONERF_F_SHADOWS) writes for the ray table whose columns 8..10 are suns[k], in every precision.  The shipped renderer itself is anchored
to the reference arithmetic (tests/test_hip_forward.py: 1e-4 against the oracle); one case repeats that anchor for the sweep directly.

Inputs (checked on the CPU oracle, eval=True, epoch_idx=3): the closed-form field of golden G8 (sigma bias + 1.5), rays
orc.synthetic_batch(R, 5, seed=77, n_samples=S), five suns, shadow-ray noise torch.rand(R, S) under seed 1000 + k.
  (300, 16): shadow-ray sample counts span 0 .. 15 = S - 1, geo_shadows spans 0.034 .. 1.0
  (300, 3), (37, 2): camera rays WITHOUT samples (the retry branch) and shadow rays without samples
  (37, 37): counts 2 .. 36        (1, 16): one ray        (257, 128): the product's sample count, a partial wave tile in both passes
From S = 3 up rgb differs between suns by >= 0.05 somewhere: a sweep that ignored `suns` cannot pass.

These tests do not aim at a fault: with correct kernels every access stays inside the test's own allocations.  Smallest shapes first;
run the file with -x."""
import ctypes as C
import functools
import warnings

import pytest
import torch

from oracle import eonerf_oracle as orc
import workspace_guard as wg

pytestmark = pytest.mark.gpu
N_IMG = 5
SHADOWS, EVAL, TRAIN, ONLY_DEPTH = 1, 2, 4, 8
E_ARG, E_WORKSPACE, E_STATE, E_UNSUPPORTED = -1, -2, -3, -4
F32, I32 = torch.float32, torch.int32
# (elevation, azimuth): high, low, grazing, near-north, below the horizon
SUN_ANGLES = [(80.0, 120.0), (35.0, 200.0), (8.0, 300.0), (60.0, 10.0), (-20.0, 45.0)]
CAMERA_COLS = [3, 4, 5, 6, 11, 12, 13, 14]      # depth, albedo, transient_s, beta, entropy, pts_per_ray: no sun in them


def L():
    from eonerf_code_amd import _lib
    return _lib.lib()


def P(x):
    if x is None:
        return C.c_void_p(0)
    return C.c_void_p(x.ptr if isinstance(x, wg.Guarded) else x.data_ptr())


def _state():
    sd = orc.closed_form_state_dict(N_IMG)
    sd["sigma_layer.output_layer.bias"] = sd["sigma_layer.output_layer.bias"] + 1.5
    return sd


def _new_field(precision, eval_precision="same", sd=None, n_img=N_IMG):
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    f = EONerfMLP(n_img, radiometric_normalization=True, precision=precision, eval_precision=eval_precision)
    f.load_state_dict(sd if sd is not None else _state(), strict=True)
    f = f.cuda()
    f._context()
    f._ensure_packed()
    return f


@functools.lru_cache(maxsize=None)
def _field(precision):
    return _new_field(precision)


def _suns():
    s = torch.tensor([orc.get_dir_vec_from_el_az(90 - el, az) for el, az in SUN_ANGLES], dtype=F32)
    return (s / s.norm(dim=1, keepdim=True)).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(R, S):
    """(rays [R,11], img [R], u_cam, u_retry [R,S], u_sun [5,R,S]) on the device; computed once per shape and never written."""
    rays, ts, _, u_cam, _ = orc.synthetic_batch(R, N_IMG, seed=77, n_samples=S)
    u_retry = torch.rand(R, S, generator=torch.Generator().manual_seed(999))
    u_sun = torch.stack([torch.rand(R, S, generator=torch.Generator().manual_seed(1000 + k)) for k in range(len(SUN_ANGLES))])
    return tuple(t.cuda().contiguous() for t in (rays, ts.reshape(-1), u_cam, u_retry, u_sun))


def _zsteps(S):
    return torch.linspace(0, 1, S, device="cuda")


def _replaced(rays, sun):
    t = rays.clone()
    t[:, 8:11] = sun
    return t.contiguous()


def forward(f, S, table, img, u_cam, u_retry, u_sun, flags):
    """The shipped path: eonerf_render_forward(flags | EONERF_F_SHADOWS) on its own workspace -> (out [R,21], n_samples [1])."""
    f.set_n_samples(S)
    R = table.shape[0]
    nb = L().eonerf_render_workspace_bytes(f._ctx, R, flags | SHADOWS)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    out = torch.full((R, 21), float("nan"), device="cuda")
    n = torch.full((1,), -1, dtype=I32, device="cuda")
    rc = L().eonerf_render_forward(f._ctx, P(f._flat), P(table), P(img), P(_zsteps(S)), P(u_cam), P(u_retry), P(u_sun), R, flags | SHADOWS, P(out), P(n),
                                   P(ws), nb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, n


def sweep(f, S, rays, img, u_cam, u_retry, u_sun, suns, flags, ws=None, out=None, ws_bytes=None, n=None):
    """eonerf_render_sun_sweep on a workspace of exactly the reported size -> (return code, out [K,R,21], n_samples [1])."""
    f.set_n_samples(S)
    R, K = rays.shape[0], suns.shape[0]
    nb = L().eonerf_sun_sweep_workspace_bytes(f._ctx, R, K)
    assert nb > 0
    if ws is None:
        ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.full((K, R, 21), float("nan"), device="cuda")
    if n is None:
        n = torch.full((1,), -1, dtype=I32, device="cuda")
    rc = L().eonerf_render_sun_sweep(f._ctx, P(f._flat), P(rays), P(img), P(_zsteps(S)), P(u_cam), P(u_retry), P(u_sun), P(suns), K, R, flags, P(out), P(n),
                                     P(ws), nb if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, out, n


# ------------------------------------------------------------------------------------------------------------ 1. bit equality
BIT_CASES = [("fp32", 37, 2), ("fp32", 1, 16), ("fp32", 300, 3), ("fp32", 37, 37), ("fp32", 300, 16), ("bf16", 300, 16), ("fp16x3", 300, 16),
             ("fp32", 257, 128)]


@pytest.mark.parametrize("precision,R,S", BIT_CASES, ids=[f"{p}-R{r}-S{s}" for p, r, s in BIT_CASES])
def test_every_sun_of_a_sweep_is_the_shipped_forward_on_the_replaced_table_bit_for_bit(precision, R, S):
    f = _field(precision)
    rays, img, u_cam, u_retry, u_sun = _inputs(R, S)
    suns = _suns()
    for flags in (0, EVAL):
        rc, out, n = sweep(f, S, rays, img, u_cam, u_retry, u_sun, suns, flags)
        assert rc == 0, rc
        assert bool(torch.isfinite(out).all())
        for k in range(suns.shape[0]):
            want, n_want = forward(f, S, _replaced(rays, suns[k]), img, u_cam, u_retry, u_sun[k], flags)
            wg.assert_same_bits(f"sweep[{precision}-R{R}-S{S}-flags{flags}]", f"out[{k}]", out[k], want)
            wg.assert_same_bits(f"sweep[{precision}-R{R}-S{S}-flags{flags}]", "n_samples_dev", n, n_want)
        for k in range(1, suns.shape[0]):
            wg.assert_same_bits("camera columns across suns", f"out[{k}]", out[k][:, CAMERA_COLS], out[0][:, CAMERA_COLS])
        if S >= 3 and R > 1:
            spread = (out[:, :, 0:3].max(dim=0).values - out[:, :, 0:3].min(dim=0).values).max().item()
            assert spread >= 0.05, spread      # the suns really light the scene differently
        assert L().eonerf_range_status(f._ctx, None) == 0
    if (precision, R, S) == ("fp32", 300, 16):      # the coverage the inputs were chosen for
        sc = out[:, :, 15]
        assert sc.min().item() == 0 and sc.max().item() == S - 1
        assert out[:, :, 10].min().item() < 0.05 and out[:, :, 10].max().item() == 1.0
    if (R, S) in ((300, 3), (37, 2)):
        assert (out[0][:, 14] == 0).any(), "a camera ray without samples: the retry branch ran"


# ------------------------------------------------------------------------------------------------------------ 2. reference arithmetic
def test_sweep_matches_the_reference_arithmetic_per_sun():
    R, S = 37, 16
    f = _field("fp32")
    rays, img, u_cam, u_retry, u_sun = _inputs(R, S)
    suns = _suns()
    rc, out, n = sweep(f, S, rays, img, u_cam, u_retry, u_sun, suns, EVAL)
    assert rc == 0
    field = orc.Field(_state())
    for k in range(suns.shape[0]):
        table = _replaced(rays, suns[k]).cpu()
        with torch.no_grad():
            ref, n_ref = orc.render_rays(field, orc.define_satrays_from_tensors(table, img.cpu()[:, None]), u_cam.cpu(), u_sun[k].cpu(), 3, 2.0 / S,
                                         eval=True, u_cam_retry=u_retry.cpu())
        got = out[k].cpu()
        assert int(n[0]) == n_ref
        assert torch.equal(got[:, 14:16], ref[:, 14:16]), f"sun {k}: sample counts must be bit exact"
        err = (got - ref).abs().max(dim=0).values
        assert err.max().item() <= 1e-4, (k, err)


# ------------------------------------------------------------------------------------------------------------ 3. Philox
def test_philox_sweep_takes_one_call_number_and_its_first_sun_is_the_shipped_forward():
    R, S, seed = 300, 16, 20240611
    a, b = _new_field("fp32"), _new_field("fp32")      # twins: same weights, each with its own call counter
    rays, img, _, _, _ = _inputs(R, S)
    suns = _suns()[:3].contiguous()
    for f in (a, b):
        assert L().eonerf_set_noise_seed(f._ctx, seed) == 0
    rc, out, n = sweep(a, S, rays, img, None, None, None, suns, 0)
    assert rc == 0
    first, n_first = forward(b, S, _replaced(rays, suns[0]), img, None, None, None, 0)
    wg.assert_same_bits("philox sweep", "out[0] against the twin's first forward", out[0], first)
    wg.assert_same_bits("philox sweep", "n_samples_dev", n, n_first)
    for k in range(1, 3):
        wg.assert_same_bits("philox sweep", f"camera columns of out[{k}]", out[k][:, CAMERA_COLS], out[0][:, CAMERA_COLS])
        assert not torch.equal(out[k][:, 0:3], out[0][:, 0:3])
    # the sweep took exactly one call number: the forwards that follow are in step
    after, _ = forward(a, S, _replaced(rays, suns[1]), img, None, None, None, 0)
    second, _ = forward(b, S, _replaced(rays, suns[1]), img, None, None, None, 0)
    wg.assert_same_bits("philox sweep", "a forward after the sweep against the twin's second forward", after, second)
    assert not torch.equal(after[:, 3], first[:, 3])      # (another call number: another jitter)


# ------------------------------------------------------------------------------------------------------------ 4. workspace contract
def _guarded_sweep(f, S, R, K, fill, ws=None):
    """A sweep on guarded buffers of exactly the reported sizes (ws: a larger allocation to run in the front of) -> (ws, out, n, bytes)."""
    rays, img, u_cam, u_retry, u_sun = _inputs(R, S)
    suns = _suns()[:K].contiguous()
    f.set_n_samples(S)
    nb = L().eonerf_sun_sweep_workspace_bytes(f._ctx, R, K)
    if ws is None:
        ws = wg.Guarded("sweep:workspace", nb, "cuda", fill=fill)
    assert ws.nbytes >= nb
    out = wg.Guarded("sweep:out", K * R * 21 * 4, "cuda", fill=0xFF)
    n = wg.Guarded("sweep:n_samples_dev", 4, "cuda", fill=0xFF)
    rc = L().eonerf_render_sun_sweep(f._ctx, P(f._flat), P(rays), P(img), P(_zsteps(S)), P(u_cam), P(u_retry), P(u_sun[:K].contiguous()), P(suns), K, R, 0,
                                     P(out), P(n), C.c_void_p(ws.ptr), nb, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert L().eonerf_device_status(f._ctx, None) == 0
    wg.check_guards(f"sweep[R{R}-S{S}-K{K}]", [ws, out, n])
    return ws, out, n, nb


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x3"])
def test_workspace_contract_of_the_sweep(precision):
    """Workspace and outputs of exactly the reported size between guards; a workspace of zeros (Z), of 0xFF bytes (F) and what a larger
    sweep left behind (S) give the same bits, and no guard byte is dirtied."""
    f = _field(precision)
    R, S, K = 37, 16, 3
    base = None
    for state in "ZFS":
        stale = tail = None
        if state == "S":
            stale, _, _, big_nb = _guarded_sweep(f, S, 300, 5, 0x00)
            f.set_n_samples(S)
            small_nb = L().eonerf_sun_sweep_workspace_bytes(f._ctx, R, K)
            assert big_nb > small_nb
            tail = stale.payload[small_nb:].clone()
        ws, out, n, nb = _guarded_sweep(f, S, R, K, 0x00 if state == "Z" else 0xFF, ws=stale)
        if stale is not None:
            wg.assert_same_bits(f"sweep[{precision}][S]", "the larger allocation behind workspace_bytes", ws.payload[nb:], tail)
        got = (out.view(F32, K, R, 21).clone(), n.view(I32, 1).clone())
        assert bool(torch.isfinite(got[0]).all()) and int(got[1][0]) >= 0, "everything the header says is written comes back written"
        if base is None:
            base = got
        else:
            wg.assert_same_bits(f"sweep[{precision}][{state}]", "out", got[0], base[0])
            wg.assert_same_bits(f"sweep[{precision}][{state}]", "n_samples_dev", got[1], base[1])
    # K = 1 is the shipped forward
    rays, img, u_cam, u_retry, u_sun = _inputs(R, S)
    rc, one, n1 = sweep(f, S, rays, img, u_cam, u_retry, u_sun[:1].contiguous(), _suns()[:1].contiguous(), 0)
    want, n_want = forward(f, S, _replaced(rays, _suns()[0]), img, u_cam, u_retry, u_sun[0], 0)
    assert rc == 0
    wg.assert_same_bits(f"sweep[{precision}] K = 1", "out", one[0], want)
    wg.assert_same_bits(f"sweep[{precision}] K = 3", "out[0]", base[0][0], want)
    wg.assert_same_bits(f"sweep[{precision}] K = 1", "n_samples_dev", n1, n_want)


def test_every_refusal_of_the_sweep_leaves_its_buffers_untouched():
    f = _field("fp32")
    R, S, K = 37, 16, 3
    rays, img, u_cam, u_retry, u_sun = _inputs(R, S)
    u_sun = u_sun[:K].contiguous()
    suns = _suns()[:K].contiguous()
    f.set_n_samples(S)
    ctx, flat, z = f._ctx, f._flat, _zsteps(S)
    nb = L().eonerf_sun_sweep_workspace_bytes(ctx, R, K)
    assert nb == L().eonerf_sun_sweep_workspace_bytes(ctx, R, 24), "the layout does not depend on the number of suns"
    assert nb > L().eonerf_render_workspace_bytes(ctx, R, SHADOWS) and nb - L().eonerf_render_workspace_bytes(ctx, R, SHADOWS) <= R * 44 + 256
    assert L().eonerf_sun_sweep_workspace_bytes(ctx, -1, K) == 0 and L().eonerf_sun_sweep_workspace_bytes(ctx, R, 0) == 0
    ws = wg.Guarded("sweep:workspace", nb, "cuda", fill=0x5A)
    out = wg.Guarded("sweep:out", K * R * 21 * 4, "cuda", fill=0x5A)
    n = wg.Guarded("sweep:n_samples_dev", 4, "cuda", fill=0x5A)

    def call(ctx=ctx, flat=flat, rays=rays, img=img, z=z, u_cam=u_cam, u_retry=u_retry, u_sun=u_sun, suns=suns, K=K, R=R, flags=0, out=out, ws=ws, nbytes=nb):
        return L().eonerf_render_sun_sweep(ctx, P(flat), P(rays), P(img), P(z), P(u_cam), P(u_retry), P(u_sun), P(suns), K, R, flags, P(out), P(n), P(ws), nbytes, None)

    def untouched(what):
        torch.cuda.synchronize()
        wg.check_guards(what, [ws, out, n])
        for b in (ws, out, n):
            assert bool((b.payload == 0x5A).all()), f"{what}: {b.name} was written"

    for name in ("ctx", "flat", "rays", "img", "z", "suns", "out", "ws"):
        assert call(**{name: None}) == E_ARG, name
    assert call(K=0) == E_ARG and call(R=-1) == E_ARG
    assert call(u_sun=None) == E_ARG                                        # noise for the camera pass but none for the shadow passes
    assert call(u_cam=None, u_retry=None) == E_ARG                          # Philox mode with a u_sun
    assert call(u_cam=None, u_sun=None) == E_ARG                            # Philox mode with a u_retry
    untouched("EONERF_E_ARG")
    # weights not set: a context of its own, never handed any
    from eonerf_code_amd import _lib
    bare = C.c_void_p()
    cfg = _lib.EonerfConfig(N_IMG, _lib.EONERF_FP32, S, 1)
    _lib.check(L().eonerf_create(C.byref(bare), C.byref(cfg)))
    try:
        assert call(ctx=bare) == E_STATE
        assert call(ctx=bare, rays=None) == E_ARG                           # the argument check comes first
        assert call(ctx=bare, R=0) == E_STATE                               # ... and the state in front of the empty batch
    finally:
        L().eonerf_destroy(bare)
    untouched("EONERF_E_STATE")
    assert call(R=0) == 0 and call(R=0, flags=TRAIN) == 0                   # an empty batch: nothing to do, nothing to refuse
    untouched("n_rays == 0")
    for flags in (TRAIN, ONLY_DEPTH, TRAIN | EVAL, ONLY_DEPTH | SHADOWS):
        assert call(flags=flags) == E_UNSUPPORTED, flags
    assert call(flags=TRAIN, nbytes=nb - 1) == E_UNSUPPORTED                # the flags in front of the workspace
    untouched("EONERF_E_UNSUPPORTED (flags)")
    try:
        f.set_n_samples(200)                                                # 2^24 rays x 199 intervals wrap an int; the forward's own bound admits them
        assert call(R=1 << 24) == E_UNSUPPORTED
        assert L().eonerf_sun_sweep_workspace_bytes(ctx, 1 << 24, K) == 0
        f.set_n_samples(256)                                                # inside the 64-bit bound, beyond the forward's
        assert ((1 << 23) + 1) * 255 <= 2 ** 31 - 1 - 255
        assert call(R=(1 << 23) + 1) == E_UNSUPPORTED
    finally:
        f.set_n_samples(S)
    untouched("EONERF_E_UNSUPPORTED (ray bound)")
    assert call(nbytes=nb - 1) == E_WORKSPACE and call(nbytes=0) == E_WORKSPACE
    untouched("EONERF_E_WORKSPACE")
    assert L().eonerf_device_status(ctx, None) == 0
    assert call() == 0                                                      # and the same buffers serve a call that is in order
    torch.cuda.synchronize()
    wg.check_guards("sweep after the refusals", [ws, out, n])
    assert bool(torch.isfinite(out.view(F32, K, R, 21)).all())


# ------------------------------------------------------------------------------------------------------------ 5. render_sun_sweep
def _chunk_noise(u_cam, u_retry, u_sun, chunk):
    R = u_cam.shape[0]
    return [(u_cam[i:i + chunk], u_retry[i:i + chunk], u_sun[:, i:i + chunk]) for i in range(0, R, chunk)]


def test_render_sun_sweep_shapes_keys_chunking_and_equality_with_render_image():
    from eonerf_code_amd.relight import render_sun_sweep, SUN_KEYS
    from eonerf_code_amd.sat_rendering import render_image, RESULT_SLICES
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    R, S, K = 35, 16, 5
    f = _field("fp32")
    rays, img, u_cam, u_retry, u_sun = _inputs(R, S)
    suns = _suns()
    sr = define_satrays_from_tensors(rays, img[:, None])
    all_keys = tuple(k for k, _, _ in RESULT_SLICES)
    # eval=True takes the radiometric row of the CHUNK's first ray (sat_rendering.py:288-291), as render_image does: an export render is one
    # view, so its rays carry one image index; a training-style render (eval=False) runs on the batch's mixed indices
    for ev, im in ((False, img), (True, torch.full_like(img, 2))):
        sr_v = define_satrays_from_tensors(rays, im[:, None])
        res16, n16 = render_sun_sweep(f, sr_v, suns, chunk=16, render_step_size=2.0 / S, eval=ev, keys=all_keys, noise=_chunk_noise(u_cam, u_retry, u_sun, 16))
        res64, n64 = render_sun_sweep(f, sr_v, suns, chunk=64, render_step_size=2.0 / S, eval=ev, keys=all_keys, noise=_chunk_noise(u_cam, u_retry, u_sun, 64))
        assert set(res16) == set(all_keys)
        for k, a, b in RESULT_SLICES:
            assert tuple(res16[k].shape) == ((K, R, b - a) if k in SUN_KEYS else (R, b - a)), k
            assert not res16[k].requires_grad
        # K render_image calls with the sun columns replaced and the same per-chunk noise
        per16 = [render_image(f, None, define_satrays_from_tensors(_replaced(rays, suns[k]), im[:, None]), None, None, epoch_idx=3, chunk=16,
                              render_step_size=2.0 / S, eval=ev, noise=[(c, r, s[k]) for c, r, s in _chunk_noise(u_cam, u_retry, u_sun, 16)]) for k in range(K)]
        per64 = [render_image(f, None, define_satrays_from_tensors(_replaced(rays, suns[k]), im[:, None]), None, None, epoch_idx=3, chunk=64,
                              render_step_size=2.0 / S, eval=ev, noise=[(u_cam, u_retry, u_sun[k])]) for k in range(K)]
        for res, n, per in ((res16, n16, per16), (res64, n64, per64)):
            assert n == per[0][1]
            for key in all_keys:
                for k in range(K):
                    got = res[key][k] if key in SUN_KEYS else res[key]
                    wg.assert_same_bits(f"render_sun_sweep(eval={ev}) against render_image", f"{key}[{k}]", got, per[k][0][key])
        # every camera ray of this batch keeps samples (checked on the oracle): no chunk resamples, and the chunking is invisible
        assert (res64["pts_per_ray"] > 0).all() and n16 == n64
        for key in all_keys:
            wg.assert_same_bits(f"render_sun_sweep(eval={ev}) chunk 16 against chunk 64", key, res16[key], res64[key])
    # keys are honoured (default: rgb and geo_shadows), [H, W] rays keep their shape, Philox noise runs
    res, _ = render_sun_sweep(f, sr, suns[:2], chunk=16, render_step_size=2.0 / S)
    assert set(res) == {"rgb", "geo_shadows"} and tuple(res["rgb"].shape) == (2, R, 3) and tuple(res["geo_shadows"].shape) == (2, R, 1)
    hw = type(sr)(*(t.reshape(5, 7, -1) for t in sr))
    res, _ = render_sun_sweep(f, hw, suns[:2], chunk=16, render_step_size=2.0 / S, keys=("rgb", "depth"))
    assert tuple(res["rgb"].shape) == (2, 5, 7, 3) and tuple(res["depth"].shape) == (5, 7, 1)
    with pytest.raises(KeyError):
        render_sun_sweep(f, sr, suns, keys=("rgb", "shadows"))


def test_render_sun_sweep_falls_back_to_the_fp32_export_context_when_fp16x3_leaves_its_range():
    """The weights of tests/test_f16x3_range.py that push an activation beyond 65504."""
    from eonerf_code_amd.relight import render_sun_sweep
    from eonerf_code_amd.sat_rendering import render_image
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    n_img, R, S = 4, 64, 128
    sd = orc.random_state_dict(n_img, seed=5, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    for layer in (1, 2, 3):
        sd[f"base_mlp.hidden_layers.{layer}.weight"] *= 400.0
    f = _new_field("bf16", eval_precision="fp16x3", sd=sd, n_img=n_img)
    rays, ts, _, u_cam, _ = orc.synthetic_batch(R, n_img, seed=9)
    rays, img, u_cam = rays.cuda(), ts.reshape(-1).cuda(), u_cam.cuda()
    suns = _suns()[:2].contiguous()
    u_sun = torch.stack([torch.rand(R, S, generator=torch.Generator().manual_seed(1000 + k)) for k in range(2)]).cuda()
    sr = define_satrays_from_tensors(rays, img[:, None])
    keys = ("rgb", "depth", "geo_shadows", "sc_pts_per_ray")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got, n = render_sun_sweep(f, sr, suns, chunk=R, render_step_size=2.0 / S, eval=True, keys=keys, noise=[(u_cam, None, u_sun)])
    assert any("fp16x3" in str(x.message) for x in w), "the switch is announced"
    assert f.eval_precision == "fp32"
    f32 = _new_field("bf16", eval_precision="fp32", sd=sd, n_img=n_img)
    for k in range(2):
        want, n32 = render_image(f32, None, define_satrays_from_tensors(_replaced(rays, suns[k]), img[:, None]), None, None, epoch_idx=3, chunk=R,
                                 render_step_size=2.0 / S, eval=True, noise=[(u_cam, None, u_sun[k])])
        assert n == n32
        for key in keys:
            g = got[key][k] if key != "depth" else got[key]
            assert bool(torch.isfinite(g).all()), key
            wg.assert_same_bits("sweep after the range fallback against the fp32 export render", f"{key}[{k}]", g, want[key])


def test_a_sweep_between_two_training_steps_leaves_the_training_context_alone(monkeypatch):
    """bf16 module: the sweep runs on the export context, so the training context's jitter stream does not move -- the second step of a
    trainer that swept in between gives the loss of one that did not (fixed-order sums: bit for bit)."""
    monkeypatch.setenv("EONERF_DETERMINISTIC", "1")
    from eonerf_code_amd.relight import render_sun_sweep
    from eonerf_code_amd.trainer import FusedTrainer
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    R = 128
    rays, ts, rgbs, _, _ = orc.synthetic_batch(R, N_IMG, seed=78)
    rays, img, pix = rays.cuda(), ts.reshape(-1).cuda(), rgbs.cuda()
    losses = []
    for with_sweep in (True, False):
        f = _new_field("bf16", eval_precision="fp16x3")
        f.set_noise_seed(4242)
        tr = FusedTrainer(f, lr=5e-4, max_rays=R)
        first = float(tr.step(rays, img, pix, 3))
        if with_sweep:
            res, _ = render_sun_sweep(f, define_satrays_from_tensors(rays, img[:, None]), _suns()[:3], chunk=64, render_step_size=2.0 / 128)
            assert f._ctx_eval is not None and bool(torch.isfinite(res["rgb"]).all())
        second = float(tr.step(rays, img, pix, 3))
        tr.check_device_status()
        losses.append((first, second))
    assert losses[0] == losses[1], losses
    assert losses[0][0] != losses[0][1]      # (the two steps draw different jitter and run on different weights)
