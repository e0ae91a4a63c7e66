"""CPU: the numpy restatement of the depth-prior contract (tests/prior_restated.py) against the reference's recorded outputs (golden
g13, tests/golden/make_golden_prior.py), the round trip of the restated inverse UTM series, and the product path's depth loss.

Bounds.  Reprojection: NaN pattern and values exact (both sides gather fp32 values; the lon / lat of the golden are the restatement's
own, recorded as inputs).  Depth: 1 fp32 ulp (fp64 inside, one cast).  Round trip: 1e-6 m -- ~500 fp64 ulps of a northing, five orders
under a DSM cell; the series' own truncation is in nanometres."""
import numpy as np
import pytest
import torch

from conftest import T, load_golden
import prior_restated as R
from oracle import eonerf_oracle as orc
from oracle import raygen_oracle as RO


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_equals_the_reference(name):
    g = load_golden("g13_prior")
    c = R.make_case(name)
    f = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], full=True)
    np.testing.assert_array_equal(f["lon"], g[f"{name}.lon"])                 # the golden's inputs are what the restatement computes today
    np.testing.assert_array_equal(f["lat"], g[f"{name}.lat"])
    want = g[f"{name}.alt"]
    assert f["raster"].dtype == np.float32 and f["raster"].shape == want.shape
    np.testing.assert_array_equal(np.isnan(f["raster"]), np.isnan(want))
    np.testing.assert_array_equal(f["raster"][~np.isnan(want)], want[~np.isnan(want)])
    # the winner image the kernels build (max of index + 1) selects what numpy's last-writer-wins assignment kept
    win = f["winner"]
    np.testing.assert_array_equal(win > 0, ~np.isnan(want))           # a NaN altitude is never valid, so it never wins
    sel = win > 0
    np.testing.assert_array_equal(c["dsm"].ravel()[f["index1d"][win[sel] - 1]], f["raster"][sel])
    depth = R.depth_prior(f["raster"], R.case_rays(c), R.Z_OFFSET, R.Z_SCALE)
    want_d = g[f"{name}.depth"]
    np.testing.assert_array_equal(depth == -1.0, want_d == -1.0)
    np.testing.assert_array_equal(np.isnan(want), (want_d == -1.0).reshape(want.shape))
    worst = np.abs(depth.astype(np.float64) - want_d) / ulp32(want_d)
    print(f"{name}: depth worst {worst.max():.2f} ulp")
    assert (worst <= 1.0).all()
    if c["values"] is not None:
        conf = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], values=c["values"])
        want_c = g[f"{name}.conf_raster"]
        np.testing.assert_array_equal(np.isnan(conf), np.isnan(want_c))
        np.testing.assert_array_equal(conf[~np.isnan(want_c)], want_c[~np.isnan(want_c)])
        np.testing.assert_array_equal(R.conf_prior(conf), g[f"{name}.conf"])
        assert np.isnan(want_c).sum() > np.isnan(want).sum()                  # NaN confidences on top of the empty pixels


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixtures_leave_no_pixel_to_rounding(name):
    """The GPU test may leave out pixels with a contributing point within 1e-9 px of an integer; the seeds are chosen so that there is none."""
    c = R.make_case(name)
    f = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], full=True)
    assert R.ambiguous_pixels(f["cols"], f["rows"], c["out_h"], c["out_w"]).sum() == 0
    assert f["valid"].sum() > (f["winner"] > 0).sum() > 0                      # collisions in every case


@pytest.mark.parametrize("south", [False, True])
def test_utm_round_trip(south):
    rng = np.random.default_rng(17)
    n = 200000
    lat = rng.uniform(0.0, 84.0, n) * (-1.0 if south else 1.0)
    lon = -81.0 + rng.uniform(-3.0, 3.0, n)                                   # zone 17: central meridian -81
    e, nn = RO.utm_forward(lat, lon, 17, south)
    lo, la = R.utm_inverse(e, nn, 17, south)
    e2, n2 = RO.utm_forward(la, lo, 17, south)
    worst = max(np.abs(e2 - e).max(), np.abs(n2 - nn).max())
    print(f"south={south}: worst round trip {worst:.3e} m, lon {np.abs(lo - lon).max():.3e} deg, lat {np.abs(la - lat).max():.3e} deg")
    assert worst < 1e-6


def test_depth_loss_matches_the_oracle_and_golden_g6():
    from eonerf_code_amd.priors import depth_loss_L2
    g = load_golden("g6_metrics")
    gd, pd, cf = T(g["gt_depth"]), T(g["pred_depth"]), T(g["conf"])
    for conf in (cf, None):
        got, want = depth_loss_L2(gd, pd, conf, 100), orc.depth_loss_L2(gd, pd, conf, 100)
        assert torch.equal(got, want)
        assert torch.allclose(got, T(g["depth_loss" if conf is not None else "depth_loss_noconf"]))
    # gradients too: the launcher's term must be the oracle's term bit for bit
    p1, p2 = pd.clone().requires_grad_(True), pd.clone().requires_grad_(True)
    depth_loss_L2(gd, p1, cf, 80.0).backward()
    orc.depth_loss_L2(gd, p2, cf, 80.0).backward()
    assert torch.equal(p1.grad, p2.grad)
    # the stated deviation: no valid prior -> 0 with a zero gradient (the reference's mean of an empty set is NaN)
    p3 = pd.clone().requires_grad_(True)
    z = depth_loss_L2(torch.full_like(gd, -1.0), p3, None, 100)
    z.backward()
    assert float(z.detach()) == 0.0 and torch.equal(p3.grad, torch.zeros_like(p3))
    assert torch.isnan(orc.depth_loss_L2(torch.full_like(gd, -1.0), pd, None, 100))
