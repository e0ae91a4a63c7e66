"""GPU: depth priors from an initial DSM (include/eonerf_prior.h, eonerf_code_amd/priors.py) against the reference's recorded outputs
(golden g13) and the numpy restatement of the contract (tests/prior_restated.py); the RayTable extras, the trainer's prior term and
the launcher's --init_dsm.

Bounds.  Reprojection: NaN pattern and values bit-equal -- both sides gather fp32 values, so the only way to differ is another winner.
A pixel may be left out only where a sample point's fp64 col / row lies within 1e-9 px of an integer (device and numpy sin / atanh
differ by an ulp, ~1e-12 px); the fixtures' seeds leave no such pixel (tests/test_prior_restated_cpu.py), which is asserted here too.
Depth: 1 fp32 ulp (fp64 inside, one cast)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import prior_restated as R
from oracle import eonerf_oracle as orc
from oracle import raygen_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_same_raster(got, want, skip):
    assert got.shape == want.shape and got.dtype == np.float32
    assert skip.sum() <= 0.001 * skip.size
    keep = ~skip
    np.testing.assert_array_equal(np.isnan(got)[keep], np.isnan(want)[keep])
    ok = keep & ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 1. reprojection
@pytest.mark.parametrize("name", list(R.CASES))
def test_reprojection_matches_the_reference_and_the_contract(name):
    from eonerf_code_amd import priors
    c = R.make_case(name)
    f = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], full=True)
    skip = R.ambiguous_pixels(f["cols"], f["rows"], c["out_h"], c["out_w"])
    assert skip.sum() == 0                                            # the seeds leave no pixel to rounding
    got = priors.reproject_dsm(cu(c["dsm"]), c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"]).cpu().numpy()
    assert_same_raster(got, f["raster"], skip)
    # the winner is the highest raveled index among the points of a pixel
    sel = f["winner"] > 0
    assert f["valid"].sum() > sel.sum()
    np.testing.assert_array_equal(got[sel], c["dsm"].ravel()[f["index1d"][f["winner"][sel] - 1]])
    g = load_golden("g13_prior")
    if name in R.GOLDEN_CASES:
        assert_same_raster(got, g[f"{name}.alt"], skip)
    if c["values"] is not None:
        want = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], values=c["values"])
        got = priors.reproject_dsm(cu(c["dsm"]), c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"],
                                   values=cu(c["values"])).cpu().numpy()
        assert_same_raster(got, want, skip)
        assert_same_raster(got, g[f"{name}.conf_raster"], skip)
    if name == "outside":                                             # the zone derived from the RPC's centre is the fixture's zone
        got = priors.reproject_dsm(cu(c["dsm"]), c["bounds"], c["rpc"], c["out_h"], c["out_w"]).cpu().numpy()
        assert_same_raster(got, f["raster"], skip)


# ---------------------------------------------------------------------------------------------------------------- 2. depth
@pytest.mark.parametrize("name", ["outside", "south", "conf"])
def test_fused_depth_matches_the_contract_and_is_reproducible(name):
    from eonerf_code_amd import priors
    c = R.make_case(name)
    n = c["out_h"] * c["out_w"]
    rays = np.concatenate([R.case_rays(c, 0), R.case_rays(c, 1)])    # two images with the same RPC and other rays
    alt = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"])
    want = np.concatenate([R.depth_prior(alt, rays[:n], R.Z_OFFSET, R.Z_SCALE), R.depth_prior(alt, rays[n:], R.Z_OFFSET, R.Z_SCALE)])
    args = (cu(c["dsm"]), c["bounds"], [c["rpc"], c["rpc"]], [[c["out_h"], c["out_w"]]] * 2, cu(rays), [0.0, 0.0, R.Z_OFFSET],
            [1.0, 1.0, R.Z_SCALE], c["zone"], c["south"])
    conf = cu(c["values"]) if c["values"] is not None else None
    d1, c1 = priors.depth_priors_from_dsm(*args, conf=conf)
    d2, c2 = priors.depth_priors_from_dsm(*args, conf=conf)
    assert d1.dtype == torch.float32 and d1.shape == (2 * n,)
    assert torch.equal(d1, d2)                                        # run to run bit-identical
    got = d1.cpu().numpy()
    empty = np.tile(np.isnan(alt).ravel(), 2)
    assert empty.any() and (got[empty] == -1.0).all() and (want[empty] == -1.0).all()
    worst = np.abs(got.astype(np.float64) - want)[~empty] / ulp32(want[~empty])
    print(f"{name}: depth worst {worst.max():.2f} ulp over {int((~empty).sum())} rays")
    assert (worst <= 1.0).all()
    g = load_golden("g13_prior")
    if name in R.GOLDEN_CASES:                                        # the reference's own depth of the first image
        want_g = g[f"{name}.depth"]
        assert ((got[:n] == -1.0) == (want_g == -1.0)).all()
        assert (np.abs(got[:n].astype(np.float64) - want_g) <= ulp32(want_g)).all()
    if conf is None:
        assert c1 is None
    else:
        want_c = R.conf_prior(R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], values=c["values"]))
        assert torch.equal(c1, c2)
        np.testing.assert_array_equal(c1.cpu().numpy(), np.tile(want_c, 2))
        np.testing.assert_array_equal(c1.cpu().numpy()[:n], g[f"{name}.conf"])
    with pytest.raises(ValueError, match="pixels"):
        priors.depth_priors_from_dsm(args[0], args[1], args[2], args[3], cu(rays[:-1]), *args[5:])


# ---------------------------------------------------------------------------------------------------------------- 3. geometry
def geometry_fixture(n_img=1, S=32, h=32, w=32):
    """A smooth terrain DSM under `n_img` synthetic cameras, with what a dataset would hold for them: RPCs at the image's scale, scene
    normalisation (whole numbers, as the fp32 values of a dataset are), altitude range."""
    lat0, lon0 = 30.33, -81.66
    zone = RO.utm_zone_number(lat0, lon0)
    rpcs = [RO.rescale_rpc(RO.synthetic_rpc(13 + k, lat0=lat0, lon0=lon0), S / 2048.0) for k in range(n_img)]
    e0, n0 = (float(v[0]) for v in RO.utm_forward(np.array([lat0]), np.array([lon0]), zone))
    gsd = 0.3 * 2048.0 / S * (1.1 / 1.05)
    half = round(0.45 * S * gsd)
    bounds = [round(e0) - half, round(n0) - half, round(e0) + half, round(n0) + half]
    yy, xx = np.mgrid[0:40, 0:40].astype(np.float64)
    dsm = (20 + 8 * np.sin(xx / 7.0) * np.cos(yy / 9.0)).astype(np.float32)
    offset, scale = [float(round(e0)), float(round(n0)), 25.0], [float(round(0.6 * S * gsd)), float(round(0.6 * S * gsd)), 40.0]
    return {"dsm": dsm, "bounds": bounds, "rpcs": rpcs, "shapes": [[h, w]] * n_img, "zone": zone, "south": False, "offset": offset,
            "scale": scale, "min_alt": -15.0, "max_alt": 65.0}


def test_prior_depth_agrees_with_the_localisation_kernel():
    """generate_rays (RPC localisation, forward UTM series) is independent code: a ray followed to its prior depth must come back to the
    reprojected altitude, at the ground position of the DSM sample point that won the pixel.
    Altitude: the depth is rounded once to fp32, so the altitude moves by at most 2^-24 of the ray's drop |alt - origin altitude|; the
    bound is 2^-23 of it.  Position: the winning point projects somewhere inside the pixel whose ray starts at the pixel's integer
    corner, so the two are at most one pixel's ground footprint (its diagonal, from the fixture's RPC) apart; plus half a DSM sample
    spacing, plus 0.25 m, the fp32 northing quantum of the reference's rays."""
    from eonerf_code_amd import priors
    from eonerf_code_amd.datasets.satellite import generate_rays, get_utmalt_from_nerf_prediction
    fx = geometry_fixture()
    (h, w), rpc = fx["shapes"][0], fx["rpcs"][0]
    rays = generate_rays(rpc, fx["min_alt"], fx["max_alt"], h=h, w=w, sun_elevation_deg=40.0, sun_azimuth_deg=150.0,
                         scene_offset=fx["offset"], scene_scale=fx["scale"], zone=fx["zone"], south=False)
    depth, _ = priors.depth_priors_from_dsm(cu(fx["dsm"]), fx["bounds"], [rpc], [[h, w]], rays, fx["offset"], fx["scale"], fx["zone"], False)
    f = R.reproject(fx["dsm"], fx["bounds"], rpc, h, w, fx["zone"], False, full=True)
    skip = R.ambiguous_pixels(f["cols"], f["rows"], h, w)
    assert skip.sum() == 0
    alt = priors.reproject_dsm(cu(fx["dsm"]), fx["bounds"], rpc, h, w, fx["zone"], False).cpu().numpy()
    assert_same_raster(alt, f["raster"], skip)
    has = ~np.isnan(alt).ravel()
    assert has.sum() > 0.5 * h * w and ((depth.cpu().numpy() >= 0) == has).all()
    e, n, a = (v.cpu().numpy() for v in get_utmalt_from_nerf_prediction(rays, depth, fx["offset"], fx["scale"]))
    origin_alt = rays[:, 2].double().cpu().numpy() * fx["scale"][2] + fx["offset"][2]
    err = np.abs(a - alt.ravel().astype(np.float64))[has]
    bound = 2.0 ** -23 * np.abs(alt.ravel().astype(np.float64) - origin_alt)[has] + 1e-9
    print(f"altitude: worst |diff| {err.max():.3e} m, worst diff / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    # one pixel's ground footprint: the diagonal between the localisations of (c, r) and (c + 1, r + 1) at mid altitude, worst corner
    cc, rr = np.array([0.0, w - 1.0, 0.0, w - 1.0]), np.array([0.0, 0.0, h - 1.0, h - 1.0])
    lon_a, lat_a = RO.localization(rpc, cc, rr, np.full(4, 20.0))
    lon_b, lat_b = RO.localization(rpc, cc + 1, rr + 1, np.full(4, 20.0))
    ea, na = RO.utm_forward(lat_a, lon_a, fx["zone"])
    eb, nb = RO.utm_forward(lat_b, lon_b, fx["zone"])
    footprint = float(np.hypot(eb - ea, nb - na).max())
    spacing = max((fx["bounds"][2] - fx["bounds"][0]) / (2 * 40 - 1), (fx["bounds"][3] - fx["bounds"][1]) / (2 * 40 - 1))
    win = f["winner"].ravel()[has] - 1
    dist = np.hypot(e[has] - f["easts"][win], n[has] - f["norths"][win])
    limit = footprint + 0.5 * spacing + 0.25
    print(f"position: worst distance {dist.max():.3f} m, limit {limit:.3f} m (footprint {footprint:.3f}, spacing {spacing:.3f})")
    assert (dist <= limit).all()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    import ctypes as C
    from eonerf_code_amd import _lib
    from eonerf_code_amd.datasets.satellite import _rpc_struct
    from eonerf_code_amd._lib import _ptr, _stream
    L = _lib.lib()
    assert L.eonerf_prior_version() == 1
    c = R.make_case("tiny")
    s, dsm = _rpc_struct(c["rpc"]), cu(c["dsm"])
    h, w = c["dsm"].shape
    b = (C.c_double * 4)(*c["bounds"])
    n = c["out_h"] * c["out_w"]
    out = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.full((n,), -1, dtype=torch.int32, device=DEV)            # 0xffffffff: no winner image holds it
    rays = cu(R.case_rays(c))

    def call(out_h=c["out_h"], out_w=c["out_w"], raster=out, depth=None, ws_bytes=4 * n, hh=h, ww=w):
        return L.eonerf_prior_reproject(_ptr(dsm), None, hh, ww, b, C.byref(s), c["zone"], 0, out_h, out_w, _ptr(raster), 0, _ptr(rays), 11,
                                        R.Z_OFFSET, R.Z_SCALE, _ptr(depth), _ptr(ws), ws_bytes, _stream())
    assert L.eonerf_prior_workspace_bytes(c["out_h"], c["out_w"]) == 4 * n
    assert L.eonerf_prior_workspace_bytes(1, 32768) == 0
    assert call(out_w=32768, ws_bytes=1 << 40) == -4                 # EONERF_E_UNSUPPORTED: int16 pixel indices of the reference
    assert call(out_h=32768, ws_bytes=1 << 40) == -4
    assert call(hh=1 << 15, ww=1 << 15) == -4                         # 4 * h * w = 2^32: the winner index
    assert call(ws_bytes=4 * n - 1) == -2                             # EONERF_E_WORKSPACE
    assert call(raster=None, depth=None) == -1                        # EONERF_E_ARG: no output
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == -1).all()                    # nothing was launched, nothing was cleared
    assert call() == 0
    assert not (ws == -1).any() and not (out == 7.0).any()


# ---------------------------------------------------------------------------------------------------------------- 5. RayTable extras
def test_ray_table_extras_follow_the_permutation():
    from eonerf_code_amd.trainer import RayTable
    n, b = 1000, 96
    g = torch.Generator().manual_seed(3)
    rays, ts, rgbs = torch.rand(n, 11, generator=g), torch.randint(0, 4, (n,), generator=g), torch.rand(n, 3, generator=g)
    prior, conf = torch.rand(n, generator=g), torch.randint(0, 8, (n,), generator=g).float()
    plain = RayTable(rays, ts, rgbs, DEV, seed=5, rank=1, world=2)
    table = RayTable(rays, ts, rgbs, DEV, seed=5, rank=1, world=2, extras={"prior_depth": prior, "prior_conf": conf})
    for epoch, step in ((0, 0), (0, 3), (1, 2)):
        out3 = plain.batch(epoch, step, b)
        assert len(out3) == 3 and len(table.batch(epoch, step, b)) == 3
        r, i, c, ex = table.batch(epoch, step, b, with_extras=True)
        lo = (step * 2 + 1) * b
        idx = table._perm[lo:lo + b]
        assert torch.equal(table._perm, plain._perm)
        assert torch.equal(r, out3[0]) and torch.equal(i, out3[1]) and torch.equal(c, out3[2])
        assert torch.equal(r, rays.to(DEV)[idx]) and torch.equal(ex["prior_depth"], prior.to(DEV)[idx])
        assert torch.equal(ex["prior_conf"], conf.to(DEV)[idx])
    assert plain.batch(0, 0, b, with_extras=True)[3] == {}
    with pytest.raises(ValueError, match="one row per ray"):
        RayTable(rays, ts, rgbs, DEV, extras={"prior_depth": prior[:-1]})


# ---------------------------------------------------------------------------------------------------------------- 6. trainer
def test_the_launchers_prior_term_is_the_reference_term(monkeypatch):
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    from eonerf_code_amd.train_dp import depth_prior_term
    from eonerf_code_amd.trainer import FusedTrainer
    monkeypatch.setenv("EONERF_DETERMINISTIC", "1")                   # fixed-order gradient sums: two backwards compare bit for bit
    n_img, n_rays = 4, 256
    sd = orc.random_state_dict(n_img, seed=91, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    f = EONerfMLP(n_img, radiometric_normalization=True, precision="bf16")
    f.load_state_dict(sd, strict=True)
    f = f.cuda()
    tr = FusedTrainer(f, lr=5e-4, max_rays=n_rays, n_samples=32)
    rays, ts, rgbs, u_cam, u_sun = orc.synthetic_batch(n_rays, n_img, seed=92, n_samples=32)
    rays, img, pix = rays.cuda(), ts.reshape(-1).cuda(), rgbs.cuda()
    noise = (u_cam.cuda(), None, u_sun.cuda())
    g = torch.Generator().manual_seed(5)
    prior = (0.2 + 1.2 * torch.rand(n_rays, generator=g))
    prior[::7] = -1.0
    conf = torch.randint(0, 8, (n_rays,), generator=g).float()
    prior, conf = prior.cuda(), conf.cuda()
    for extras in ({"prior_depth": prior, "prior_conf": conf}, {"prior_depth": prior}):
        record = [None]
        loss_a = tr.forward_backward(rays, img, pix, 1, noise, aux_loss=depth_prior_term(extras, 80.0, record)).clone()
        g_a = tr.d_flat.clone()
        loss_b = tr.forward_backward(rays, img, pix, 1, noise,
                                     aux_loss=lambda o: orc.depth_loss_L2(prior, o[:, 3], extras.get("prior_conf"), w=80.0)).clone()
        g_b = tr.d_flat.clone()
        tr.check_device_status()
        assert math.isfinite(float(record[0])) and float(record[0]) > 0
        assert torch.equal(loss_a, loss_b) and torch.equal(g_a, g_b)
        assert g_a.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 7. launcher
def run_launcher(tmp_path, extra):
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--rays", os.path.join(str(tmp_path), "table.pt"), "--n_images", "2",
           "--batch_size", "240", "--max_train_steps", "6", "--check_every", "1", "--n_samples", "32", "--logs_dir", str(tmp_path),
           "--exp_name", "t"] + extra
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_launcher_trains_with_depth_priors(tmp_path):
    from eonerf_code_amd.datasets.satellite import generate_rays
    fx = geometry_fixture(n_img=2, S=24, h=24, w=20)
    rays = torch.cat([generate_rays(rpc, fx["min_alt"], fx["max_alt"], h=24, w=20, sun_elevation_deg=40.0, sun_azimuth_deg=150.0,
                                    scene_offset=fx["offset"], scene_scale=fx["scale"], zone=fx["zone"], south=False)
                      for rpc in fx["rpcs"]]).cpu()
    ts = torch.arange(2).repeat_interleave(24 * 20)
    torch.save({"rays": rays, "ts": ts, "rgbs": torch.rand(960, 3, generator=torch.Generator().manual_seed(1))},
               os.path.join(str(tmp_path), "table.pt"))
    init = os.path.join(str(tmp_path), "init.pt")
    torch.save({"dsm": torch.from_numpy(fx["dsm"]), "bounds": fx["bounds"], "zone": fx["zone"], "south": False, "scene_offset": fx["offset"],
                "scene_scale": fx["scale"], "rpcs": fx["rpcs"], "shapes": torch.tensor(fx["shapes"])}, init)
    out = run_launcher(tmp_path, ["--init_dsm", init])
    terms = [float(m) for m in re.findall(r"train/depth_l2=([^\s|]+)", out)]
    weights = [float(m) for m in re.findall(r"depth_weight=([^\s|]+)", out)]
    # 960 rays / 240 per step = 4 steps per epoch: steps 0-3 in epoch 0, steps 4-6 in epoch 1
    assert len(terms) == 7 and all(math.isfinite(t) for t in terms), out
    assert any(t > 0 for t in terms), out
    assert weights == [100.0] * 4 + [80.0] * 3, out
    plain = run_launcher(tmp_path, [])
    assert "depth_l2" not in plain and "depth_weight" not in plain
    assert len(re.findall(r"step=\d+ \| loss=", plain)) == 7
