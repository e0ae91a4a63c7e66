"""CPU: tests/march_restated.py (the march rule of include/eonerf_march.h restated in numpy fp64) against scalar loops that follow the
rule's sentences slot by slot, and the rule's stated properties: eps = 0 is oracle/nerfacc_restated.py's weights on the same sample
list; the kept count never grows with eps; the camera bounds (2 eps on depth, eps on the unit-range sums, eps * max(tb) on beta); a
block that covers the whole ray is the dense result whatever eps is."""
import math

import numpy as np
import pytest
import torch

from oracle import nerfacc_restated as nv
import march_restated as mr

EPS = [0.0, 1e-3, 0.08, 0.25, 0.6]
BLOCKS = [16, 32, 64]


def layout(seed, R=23, n=127, fog=3.0):
    """Rays with 0, 1, n and random numbers of valid slots; densities from fog to wall; the last valid slot's interval is 1e10."""
    rng = np.random.default_rng(seed)
    valid = rng.random((R, n)) < rng.random((R, 1))
    valid[0] = False
    valid[1] = False
    valid[1, n // 2] = True
    valid[2] = True
    sigma = rng.random((R, n)) * fog * rng.random((R, 1)) ** 2
    delta = np.full((R, n), 2.0 / n) * (0.5 + rng.random((R, n)))
    for r in range(R):
        idx = np.nonzero(valid[r])[0]
        if idx.size:
            delta[r, idx[-1]] = 1e10
    tmid = np.sort(rng.random((R, n)) * 2.0, axis=1)
    alb = rng.random((R, n, 3))
    tb = rng.random((R, n)) * 3.0
    return valid, sigma * delta, {"depth": tmid, "albedo": alb, "ts": rng.random((R, n)), "tb": tb}


def scalar_march(valid, sd, eps, block, values):
    """The rule, one ray and one slot at a time."""
    R, n = valid.shape
    kept = np.zeros((R, n), dtype=bool)
    w = np.zeros((R, n))
    geo = np.ones(R)
    rounds = np.zeros(R, dtype=int)
    for r in range(R):
        slots = [i for i in range(n) if valid[r, i]]
        if not slots:
            continue
        last = slots[-1]
        alive, od_kept, j = True, 0.0, 0
        while j * block <= last:
            if j > 0:
                od_j = sum(sd[r, i] for i in slots if i < j * block)
                alive = alive and math.exp(-od_j) >= eps
                if not alive:
                    geo[r] = math.exp(-od_j)
                    break
            rounds[r] = j + 1
            for i in range(j * block, min((j + 1) * block, n)):
                if not valid[r, i]:
                    continue
                kept[r, i] = True
                if i == last:
                    geo[r] = math.exp(-od_kept)
                w[r, i] = math.exp(-od_kept) * (1.0 - math.exp(-sd[r, i]))
                od_kept += sd[r, i]
            j += 1
    sums = {}
    for name, v in values.items():
        v3 = v[:, :, None] if v.ndim == 2 else v
        s = np.zeros((R, v3.shape[2]))
        for r in range(R):
            for i in range(n):
                if kept[r, i]:
                    s[r] += w[r, i] * v3[r, i]
        sums[name] = s
    return kept, rounds, w, sums, geo


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("eps", EPS)
def test_restatement_against_scalar_loops(eps, block):
    for seed, n in ((1, 127), (2, 36), (3, 1), (4, 254)):
        valid, sd, values = layout(seed, n=n)
        got = mr.march(valid, sd, eps, block, values)
        kept, rounds, w, sums, geo = scalar_march(valid, sd, eps, block, values)
        assert np.array_equal(got["kept"], kept)
        assert np.array_equal(got["rounds"], rounds)
        assert np.allclose(got["weights"], w, rtol=1e-12, atol=1e-15)      # (1 - exp(-sd)) cancels: an ulp of 1 is its absolute error
        assert np.allclose(got["geo"], geo, rtol=1e-12, atol=1e-300)
        for name in values:
            assert np.allclose(got["sums"][name], sums[name], rtol=1e-10, atol=1e-14), name
        assert np.allclose(got["wsum"], w.sum(axis=1), rtol=1e-10)
        assert got["geo"][0] == 1.0 and got["rounds"][0] == 0 and got["rounds"][1] == (n // 2) // block + 1


@pytest.mark.parametrize("block", BLOCKS)
def test_eps_zero_is_nerfacc_on_the_same_list(block):
    valid, sd, values = layout(7)
    R, n = valid.shape
    got = mr.march(valid, sd, 0.0, block, values)
    assert np.array_equal(got["kept"], valid)
    ri, slot = np.nonzero(valid)
    t0 = torch.zeros(ri.size, dtype=torch.float64)
    w, trans, _ = nv.render_weight_from_density(t0, t0 + 1.0, torch.from_numpy(sd[ri, slot]), torch.from_numpy(ri), R)
    assert np.allclose(got["weights"][ri, slot], w.numpy(), rtol=1e-12, atol=1e-15)
    depth = nv.accumulate_along_rays(w, torch.from_numpy(values["depth"][ri, slot])[:, None], torch.from_numpy(ri), R)
    assert np.allclose(got["sums"]["depth"], depth.numpy(), rtol=1e-10, atol=1e-14)
    last = np.array([np.nonzero(valid[r])[0][-1] if valid[r].any() else -1 for r in range(R)])
    flat_last = np.cumsum(valid.sum(axis=1)) - 1
    for r in range(R):
        want = 1.0 if last[r] < 0 else float(trans[flat_last[r]])
        assert math.isclose(got["geo"][r], want, rel_tol=1e-12, abs_tol=1e-300)
    assert np.all(np.isinf(got["margin"]))


@pytest.mark.parametrize("block", BLOCKS)
def test_kept_is_monotone_and_the_bounds_hold(block):
    for seed in (11, 12, 13):
        valid, sd, values = layout(seed)
        ref = mr.march(valid, sd, 0.0, block, values)
        prev = ref["kept"].sum(axis=1)
        for eps in EPS[1:]:
            got = mr.march(valid, sd, eps, block, values)
            k = got["kept"].sum(axis=1)
            assert np.all(k <= prev)
            assert np.all(got["kept"] <= ref["kept"])
            prev = k
            tol = 1e-12
            assert np.abs(got["sums"]["depth"] - ref["sums"]["depth"]).max() <= 2 * eps + tol       # t < 2
            for name in ("albedo", "ts"):
                assert np.abs(got["sums"][name] - ref["sums"][name]).max() <= eps + tol
            assert np.abs(got["wsum"] - ref["wsum"]).max() <= eps + tol
            assert np.abs(got["sums"]["tb"] - ref["sums"]["tb"]).max() <= eps * values["tb"].max() + tol
            died = ~got["alive"][:, -1] & (got["kept"].sum(axis=1) < valid.sum(axis=1))
            assert np.all(got["geo"][died] < eps)
        assert (prev < ref["kept"].sum(axis=1)).any()      # the largest eps really drops samples


@pytest.mark.parametrize("eps", EPS)
def test_a_block_that_covers_the_ray_is_the_dense_result(eps):
    valid, sd, values = layout(21, n=63)
    ref = mr.march(valid, sd, 0.0, 16, values)
    got = mr.march(valid, sd, eps, 64, values)
    assert np.array_equal(got["kept"], valid)
    assert np.array_equal(got["weights"], ref["weights"]) and np.array_equal(got["geo"], ref["geo"])
    assert np.array_equal(got["rounds"], valid.any(axis=1).astype(int))


def test_dense_layout_scatters_a_sample_list():
    ri, slots = np.array([0, 0, 2]), np.array([1, 3, 0])
    valid, cols = mr.dense_layout(ri, slots, 3, 4, sd=np.array([1.0, 2.0, 3.0]), v=np.arange(9.0).reshape(3, 3))
    assert valid.tolist() == [[False, True, False, True], [False] * 4, [True, False, False, False]]
    assert cols["sd"][0, 3] == 2.0 and cols["sd"][2, 0] == 3.0 and cols["v"][2, 0].tolist() == [6.0, 7.0, 8.0] and cols["v"].shape == (3, 4, 3)
