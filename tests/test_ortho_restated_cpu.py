"""CPU: the numpy restatement of the true-orthophoto contract (tests/ortho_restated.py) checked on itself, on an analytic scene, and
for the tie margin the GPU comparisons (tests/test_ortho_gpu.py) rely on.  Needs no GPU and no library."""
import numpy as np
import pytest

import ortho_restated as OR


@pytest.fixture(scope="module")
def results():
    out = {}
    for name in OR.CASES:
        c = OR.make_case(name)
        out[name] = (c, OR.orthorectify(c, OR.MEAN), OR.orthorectify(c, OR.MEDIAN))
    return out


@pytest.mark.parametrize("name", list(OR.CASES))
def test_weight_and_nan_rules(results, name):
    c, mean, med = results[name]
    n = c["rays"].shape[0]
    for k, img in enumerate(c["images"]):
        h, w = img.shape[:2]
        lay, wgt, cr = mean["layers"][k], mean["weights"][k], mean["colrow"][k]
        assert lay.dtype == np.float32 and wgt.dtype == np.float32 and cr.dtype == np.float64
        zero = wgt == 0
        assert np.isnan(lay[zero]).all() and np.isfinite(lay[~zero]).all()          # NaN in every channel exactly where the weight is 0
        with np.errstate(invalid="ignore"):
            inside = (cr[:, 0] >= 0) & (cr[:, 0] <= w - 1) & (cr[:, 1] >= 0) & (cr[:, 1] <= h - 1)
        assert not (~inside & ~zero).any()
        if c["visibility"] is None:
            assert (wgt[~zero] == 1).all()
        else:
            v = c["visibility"][k]
            np.testing.assert_array_equal(wgt[~zero], v[~zero])
            assert (v[~zero] >= np.float32(c["min_visibility"])).all()
    for r in (mean, med):
        assert r["mosaic"].shape == (n, c["images"][0].shape[2]) and r["count"].dtype == np.int32
        np.testing.assert_array_equal(r["count"], (mean["weights"] > 0).sum(axis=0))
        assert np.isnan(r["mosaic"][r["count"] == 0]).all() and np.isfinite(r["mosaic"][r["count"] > 0]).all()
        assert (r["weight"][r["count"] == 0] == 0).all()
    assert (mean["count"] > 0).any()                                                # no case is empty


def test_the_cases_cover_what_their_table_says(results):
    c, mean, _ = results["tiny"]
    assert c["rays"].shape[0] == 1 and len(c["images"]) == 1 and c["images"][0].shape == (2, 2, 1) and mean["count"][0] == 1
    c, mean, _ = results["block"]
    assert c["rays"].shape[0] == 257 and (mean["count"] == 2).any()                 # an even median
    c, mean, _ = results["odd"]
    assert (mean["count"] == 3).any() and c["images"][0].shape[2] == 4
    c, mean, _ = results["cap"]
    assert len(c["images"]) == OR.MAX_MEDIAN and mean["count"].max() > 32
    assert results["south"][0]["south"] and (results["south"][1]["lonlatalt"][:, 1] < 0).all()
    c, mean, _ = results["edges"]
    for k, img in enumerate(c["images"]):
        h, w = img.shape[:2]
        col, row = mean["colrow"][k][:, 0], mean["colrow"][k][:, 1]
        with np.errstate(invalid="ignore"):
            assert (col < 0).any() and (col > w - 1).any() and (row < 0).any() and (row > h - 1).any()      # outside on all four sides
    assert np.isnan(mean["lonlatalt"][[OR.EDGE_NAN_DEPTH, OR.EDGE_INF_DEPTH]]).all()
    assert (mean["weights"][:, [OR.EDGE_NAN_DEPTH, OR.EDGE_INF_DEPTH, OR.EDGE_UNSEEN]] == 0).all()
    assert mean["weights"][0, OR.EDGE_NAN_VIS] == 0
    # the unseen cell projects inside every image: only its visibility keeps it out
    no_vis = OR.orthorectify(c, OR.MEAN, visibility=None)
    inside_unseen = [np.isfinite(no_vis["colrow"][k][OR.EDGE_UNSEEN]).all() for k in range(3)]
    assert all(inside_unseen) and mean["count"][OR.EDGE_UNSEEN] == 0
    # NaN pixels under some taps: a point inside the image, visible, and still weight 0
    hit = False
    for k, img in enumerate(c["images"]):
        h, w = img.shape[:2]
        cr, v = mean["colrow"][k], c["visibility"][k]
        with np.errstate(invalid="ignore"):
            inside = (cr[:, 0] >= 0) & (cr[:, 0] <= w - 1) & (cr[:, 1] >= 0) & (cr[:, 1] <= h - 1) & (v >= np.float32(0.2))
        hit |= bool((inside & (mean["weights"][k] == 0)).any())
    assert hit
    with np.errstate(invalid="ignore"):
        assert (c["visibility"] < 0.2).any() and (c["visibility"] > 0.2).any()


@pytest.mark.parametrize("name", list(OR.CASES))
def test_fusion_modes(results, name):
    c, mean, med = results[name]
    lay, wgt = mean["layers"].astype(np.float64), mean["weights"].astype(np.float64)
    seen = mean["count"] > 0
    # the median against numpy's, on the layers with the unseen images masked out
    masked = np.where((wgt > 0)[:, :, None], lay, np.nan)
    with np.errstate(all="ignore"):
        want = np.nanmedian(masked[:, seen], axis=0)
    np.testing.assert_allclose(med["mosaic"][seen], want.astype(np.float32), rtol=0, atol=1e-7)
    for p in np.nonzero(seen)[0][:5]:
        ks = wgt[:, p] > 0
        np.testing.assert_allclose(med["mosaic"][p], np.median(lay[ks, p], axis=0).astype(np.float32), rtol=0, atol=1e-7)
    # the weighted mean against a vectorised sum (another order of summation: a few fp64 ulps, then one fp32 rounding)
    w0 = np.where(wgt > 0, wgt, 0.0)
    with np.errstate(all="ignore"):
        want = (np.where((wgt > 0)[:, :, None], lay, 0.0) * w0[:, :, None]).sum(axis=0)[seen] / w0.sum(axis=0)[seen, None]
    np.testing.assert_allclose(mean["mosaic"][seen], want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(mean["weight"], w0.sum(axis=0), rtol=1e-6, atol=0)
    np.testing.assert_array_equal(mean["weight"], med["weight"])


def test_gain_and_bias_are_inverted():
    c = OR.make_case("odd")
    plain = dict(c, gain=np.ones_like(c["gain"]), bias=np.zeros_like(c["bias"]))
    a, b = OR.orthorectify(c, OR.MEAN), OR.orthorectify(plain, OR.MEAN)
    np.testing.assert_array_equal(a["weights"], b["weights"])
    for k in range(len(c["images"])):
        s = a["weights"][k] > 0
        np.testing.assert_allclose(a["layers"][k][s] * c["gain"][k] + c["bias"][k], b["layers"][k][s], rtol=0, atol=1e-6)


def test_conventions_on_an_analytic_plane():
    """Row / col order, north up, no half-pixel offset: the mosaic of two synthetic images of a plane with a linear pattern equals the
    pattern at the surface points within 0.1 * gsd * (|gE| + |gN|) = 1.26e-3.  Measured: 5.6e-8 in both modes -- the fp32 rounding of the
    images' pixels; a row / col swap measures 1.0e-1, a north flip 2.2e-1 and a half-pixel shift 6.5e-3 (5.2 times the bound)."""
    s = OR.plane_scene()
    assert abs(s["bound"] - 1.257e-3) < 1e-5
    for mode in (OR.MEAN, OR.MEDIAN):
        r = OR.orthorectify(s, mode)
        assert (r["count"] == 2).all()                                # inside both footprints
        err = np.abs(r["mosaic"][:, 0].astype(np.float64) - s["truth"]).max()
        print(f"plane scene, mode {mode}: max |mosaic - f| = {err:.3e} (bound {s['bound']:.3e})")
        assert err < s["bound"]
    assert s["truth"].min() < 0.3 and s["truth"].max() > 0.7          # the pattern varies over the grid
    # what the bound is for: each wrong convention errs by at least five times it
    r = OR.orthorectify(s, OR.MEAN)
    lla = r["lonlatalt"]
    img, rpc = s["images"][0], s["rpcs"][0]
    one, zero = np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
    wrong = {"swap": np.ascontiguousarray(img.transpose(1, 0, 2)), "flip": img[::-1].copy(), "half": None}
    for name, im in wrong.items():
        if im is None:                                                # pixel centres at +0.5
            half = dict(rpc, col_offset=rpc["col_offset"] - 0.5, row_offset=rpc["row_offset"] - 0.5)
            lay, wgt, _ = OR.gather(lla, half, img, one, zero)
        else:
            lay, wgt, _ = OR.gather(lla, rpc, im, one, zero)
        e = np.nanmax(np.abs(lay[:, 0].astype(np.float64) - s["truth"]))
        print(f"wrong convention '{name}': max error {e:.3e}")
        assert e > 5 * s["bound"], name


@pytest.mark.parametrize("name", list(OR.CASES))
def test_tie_margin(results, name):
    c, mean, _ = results[name]
    assert OR.tie_margin(c, mean) > 1e-6
