"""CPU: tests/occ_restated.py (the occupancy grid of include/eonerf_occ.h restated in numpy / torch) against brute-force loops --
cell index, bit packing, the culling rule on a sample list, the update, the dilation -- at r = 1, 3, 5, 32; the cell index at the
edges of fp32; the keep-last rule on rays with 0, 1 and n_samples - 1 cube-valid samples."""
import math
import struct

import numpy as np
import pytest
import torch

import occ_restated as occ

RES = [1, 3, 5, 32]


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def brute_axis(x, r):
    a = f32(f32(x) + 1.0)
    b = f32(a * 0.5)
    c = f32(b * float(r))
    return min(r - 1, int(c))


@pytest.mark.parametrize("r", RES)
def test_cell_index_against_a_scalar_loop(r):
    rng = np.random.default_rng(r)
    pts = rng.uniform(-1, 1, size=(500, 3)).astype(np.float32)
    pts = pts[(np.abs(pts) < 1).all(axis=1)]
    got = occ.cell_index(pts, r)
    for p, c in zip(pts, got):
        ix, iy, iz = (brute_axis(float(v), r) for v in p)
        assert c == (ix * r + iy) * r + iz
        assert 0 <= c < r ** 3
    t = torch.from_numpy(pts)
    assert np.array_equal(occ.cell_index_torch(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(), r).numpy(), got)


@pytest.mark.parametrize("r", RES + [128, 256])
def test_cell_index_at_the_edges_of_fp32(r):
    edge = [-1 + 2.0 ** -24, -2.0 ** -149, 0.0, 1 - 2.0 ** -24]
    assert all(f32(e) == e for e in edge)      # all four are fp32 numbers
    want = [0, r // 2, r // 2, r - 1]          # x + 1 = 2^-24 | 1 | 1 | 2.0f: the last one needs the clamp
    got = occ.cell_axis(np.array(edge, dtype=np.float32), r)
    assert got.tolist() == want, (r, got)
    assert [brute_axis(e, r) for e in edge] == want
    assert f32(f32(1 - 2.0 ** -24) + 1.0) == 2.0      # why the clamp exists
    t = torch.tensor(edge, dtype=torch.float32)
    z = torch.zeros_like(t)
    assert (occ.cell_index_torch(z, z, t, r) - occ.cell_index_torch(z, z, z, r) + r // 2).tolist() == want


@pytest.mark.parametrize("r", RES)
def test_bit_packing_round_trip_and_zero_tail(r):
    n = r ** 3
    flags = np.random.default_rng(10 + r).random(n) < 0.5
    words = occ.pack_bits(flags)
    assert words.dtype == np.uint32 and words.size == (n + 31) // 32
    for c in range(n):
        assert bool((int(words[c >> 5]) >> (c & 31)) & 1) == bool(flags[c])
    for c in range(n, words.size * 32):
        assert (int(words[c >> 5]) >> (c & 31)) & 1 == 0
    assert np.array_equal(occ.unpack_bits(words, n), flags)
    assert np.array_equal(occ.unpack_bits(occ.pack_bits(np.ones(n, bool)), n), np.ones(n, bool))


def brute_keep(ray_indices, occupied):
    keep = []
    for p in range(len(ray_indices)):
        last = p == len(ray_indices) - 1 or ray_indices[p + 1] != ray_indices[p]
        keep.append(bool(occupied[p]) or last)
    return np.array(keep, dtype=bool)


@pytest.mark.parametrize("n_samples", [2, 37, 128, 255])
def test_keep_last_rule_on_rays_with_no_one_and_all_samples(n_samples):
    full = n_samples - 1
    counts = [0, 1, full, 0, 1, full]      # ray 0 and 3 have no sample at all: they get none
    ri = np.concatenate([np.full(c, k) for k, c in enumerate(counts)]).astype(np.int64)
    for name, occd in (("empty grid", np.zeros(ri.size, bool)), ("full grid", np.ones(ri.size, bool)),
                       ("random grid", np.random.default_rng(n_samples).random(ri.size) < 0.5)):
        keep = occ.keep_mask(ri, occd)
        assert np.array_equal(keep, brute_keep(ri, occd)), name
        kept = np.bincount(ri[keep], minlength=len(counts))
        assert ((kept > 0) == (np.array(counts) > 0)).all(), name      # a ray has a sample exactly when it has one without the grid
        for k, c in enumerate(counts):
            if c:      # the last cube-valid sample always survives
                assert keep[np.nonzero(ri == k)[0][-1]]
        if name == "empty grid":
            assert kept.tolist() == [min(c, 1) for c in counts]
        if name == "full grid":
            assert keep.all()
        assert np.array_equal(occ.keep_mask_torch(torch.from_numpy(ri), torch.from_numpy(occd)).numpy(), keep)
    assert occ.keep_mask(np.zeros(0, np.int64), np.zeros(0, bool)).size == 0


@pytest.mark.parametrize("r", RES)
def test_cull_looks_the_sample_cells_up(r):
    rng = np.random.default_rng(40 + r)
    flags = rng.random(r ** 3) < 0.5
    ri = np.sort(rng.integers(0, 7, size=200))
    xyz = rng.uniform(-0.999, 0.999, size=(200, 3)).astype(np.float32)
    occd = np.array([flags[(brute_axis(float(p[0]), r) * r + brute_axis(float(p[1]), r)) * r + brute_axis(float(p[2]), r)] for p in xyz])
    assert np.array_equal(occ.cull(ri, xyz, flags, r), brute_keep(ri, occd))


@pytest.mark.parametrize("r", RES)
def test_cell_points_lie_in_their_cells(r):
    for jitter in (False, True):
        p = occ.cell_points(r, seed=0x5eed5eed, call=3, jitter=jitter)
        assert p.shape == (r ** 3, 3) and p.dtype == np.float32
        c = 0
        for ix in range(min(r, 4)):
            for iy in range(min(r, 4)):
                for iz in range(min(r, 4)):
                    c = (ix * r + iy) * r + iz
                    lo = [2.0 * i / r - 1 for i in (ix, iy, iz)]
                    assert all(l - 1e-6 <= v <= l + 2.0 / r + 1e-6 for l, v in zip(lo, p[c].tolist()))
                    if not jitter:
                        want = [f32(f32(f32(f32(float(i) + 0.5) / float(r)) * 2.0) - 1.0) for i in (ix, iy, iz)]
                        assert p[c].tolist() == want
    a, b = occ.cell_points(r, seed=1, call=0), occ.cell_points(r, seed=1, call=1)
    assert np.array_equal(a, occ.cell_points(r, seed=1, call=0)) and not np.array_equal(a, b)


def test_philox_known_answer():
    """Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors): counter and key all zero / all ones."""
    def raw(seed, c):
        # undo the 24-bit conversion: the top 24 bits of every word
        return [int(v * 2 ** 24) for v in occ.philox_u4(seed, *c)[0]]
    assert raw(0, (0, 0, 0, 0)) == [w >> 8 for w in (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)]
    ones = 0xFFFFFFFF
    assert raw((ones << 32) | ones, (ones,) * 4) == [w >> 8 for w in (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)]


@pytest.mark.parametrize("r", RES)
def test_update_against_a_scalar_loop(r):
    rng = np.random.default_rng(70 + r)
    n = r ** 3
    occs = (rng.random(n) * 0.02).astype(np.float32)
    sigma = (rng.random(n) * 4 * (rng.random(n) < 0.3)).astype(np.float32)
    step, decay, thre = 2.0 / 128, 0.95, 1e-2
    new, mean, thr, flags = occ.update(occs, sigma, step, decay, thre)
    want = [max(f32(float(o) * f32(decay)), f32(float(s) * f32(step))) for o, s in zip(occs, sigma)]
    assert new.tolist() == want
    m = math.fsum(want) / n
    assert abs(mean - m) <= 1e-12 * max(abs(m), 1e-30)
    assert thr == min(f32(m), f32(thre))
    assert flags.tolist() == [w > thr for w in want]


@pytest.mark.parametrize("r", RES)
def test_dilation_against_a_scalar_loop(r):
    flags = np.random.default_rng(90 + r).random(r ** 3) < (0.5 if r < 32 else 0.02)
    got = occ.dilate(flags, r).reshape(r, r, r)
    g = flags.reshape(r, r, r)
    on = np.argwhere(g)
    want = np.zeros((r, r, r), dtype=bool)
    for x, y, z in on:      # every set cell switches its clipped 3 x 3 x 3 neighbourhood on
        for a in range(max(0, x - 1), min(r, x + 2)):
            for b in range(max(0, y - 1), min(r, y + 2)):
                for c in range(max(0, z - 1), min(r, z + 2)):
                    want[a, b, c] = True
    assert np.array_equal(got, want)
    assert not occ.dilate(np.zeros(r ** 3, bool), r).any() and occ.dilate(np.ones(r ** 3, bool), r).all()
