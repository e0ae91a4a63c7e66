"""GPU: the texture entry points (eonerf_code_amd/csrc/eonerf_texture.h) through the C ABI, against the fp64 numpy restatement of their
contract (tests/texture_restated.py), and the fused bake against the two kernels it fuses.

Bounds.  uv, face, bary and xyz are exact: integer arithmetic, and fp64 sums, products and quotients that IEEE 754 rounds the same
way on both sides (the unit is built unfused), cast once.  normal is held to one fp32 ulp: it is a cast of n / sqrt(n . n) in fp64, and
while the device's fp64 division is correctly rounded, HIP documents its fp64 sqrt to 1 ulp only -- an fp64 ulp moves the fp32 cast by
at most one fp32 ulp, where the value sits on a rounding boundary.  lon / lat within 1e-12 degrees, as tests/test_ortho_gpu.py holds the
same series (tests/geodesy_exact.py; device and numpy libm differ there); the altitude is plain unfused fp64 arithmetic and exact.
Colours within 1e-6 absolute, by test_ortho_gpu.py's own derivation: pixels in [0, 1], coordinates within 1e-9 px of the restatement's
(1e-12 degrees through the RPC), bilinear slope at most 1 per axis, gain at least 0.5 and one fp32 rounding (1.2e-7 for the values up to
2.2 that (v - b) / A reaches) give less than 2e-7; the median is 1-Lipschitz in the sup norm, the weighted mean a convex combination and
BEST one of the values, so all three modes keep the bound.  count and best are exact: no sample of a case lies within 1e-6 px of an
image edge, within 1e-6 of min_cos, or within 1e-9 of a weight tie (tests/test_texture_restated_cpu.py asserts it), and the cosine
itself is unfused fp64 arithmetic on the same bits.  The cross-check against eonerf_ortho_gather + eonerf_ortho_fuse has no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import ortho_restated as OR
import texture_cases as TC
import texture_restated as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-6
E_ARG, E_UNSUPPORTED = -1, -4
S = TC.SENTINEL
GUARD = 3                                   # sentinel rows before and after every output


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t, row=0):
    """The address of row `row` of a tensor (None: NULL)."""
    return C.c_void_p(t[row:].data_ptr() if row else t.data_ptr()) if t is not None else C.c_void_p(0)


def f32(v):
    v = [float(x) for x in v]
    return (C.c_float * len(v))(*v)


def lib():
    from eonerf_code_amd import _lib
    return _lib.lib()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a


def guarded(n, tail, dtype):
    """A sentinel-filled output of n rows between GUARD rows on either side."""
    return torch.full((n + 2 * GUARD,) + tail, S, dtype=dtype, device=DEV)


def inner(t):
    """The n rows between the guards, after checking that the guards kept the sentinel."""
    assert (t[:GUARD] == S).all() and (t[-GUARD:] == S).all()
    return t[GUARD:-GUARD].cpu().numpy()


def rpc_table(rpcs):
    """The K RPCs as one device array of eonerf_rpc."""
    from eonerf_code_amd._lib import EonerfRpc
    from eonerf_code_amd.datasets.satellite import _rpc_struct
    raw = b"".join(bytes(_rpc_struct(r)) for r in rpcs)
    assert len(raw) == len(rpcs) * C.sizeof(EonerfRpc)
    return cu(np.frombuffer(raw, dtype=np.uint8).copy())


class Device:
    """A case's tables on the device (kept alive for as long as the addresses are in use)."""

    def __init__(self, c):
        self.c = c
        self.vertices, self.faces = cu(c["vertices"]), cu(c["faces"])
        self.images = [cu(im) for im in c["images"]]
        self.rpcs = rpc_table(c["rpcs"])
        self.addresses = cu(np.array([im.data_ptr() for im in self.images], dtype=np.uint64).view(np.int64))
        self.shapes = cu(c["shapes"])
        self.gain, self.bias, self.sat = cu(c["gain"]), cu(c["bias"]), cu(c["to_satellite"])
        self.K, self.C = len(self.images), c["images"][0].shape[2]

    def samples(self, first, n, want=("face", "bary", "xyz", "lla", "normal")):
        c = self.c
        out = {"face": guarded(n, (), torch.int32), "bary": guarded(n, (3,), torch.float32), "xyz": guarded(n, (3,), torch.float32),
               "lla": guarded(n, (3,), torch.float64), "normal": guarded(n, (3,), torch.float32)}
        rc = lib().eonerf_texture_samples(ptr(self.vertices), self.vertices.shape[0], ptr(self.faces), self.faces.shape[0], c["texels"], first, n,
                                          f32(c["scene_scale"]), f32(c["scene_offset"]), c["zone"], 1 if c["south"] else 0,
                                          *[ptr(out[k], GUARD) if k in want else None for k in ("face", "bary", "xyz", "lla", "normal")], None)
        assert rc == 0
        return out

    def bake(self, lla, normal, blocked, mode, angle_weight=1, min_cos=TC.MIN_COS, want=("colour", "wsum", "count", "best"), K=None):
        n = lla.shape[0]
        out = {"colour": guarded(n, (self.C,), torch.float32), "wsum": guarded(n, (), torch.float32), "count": guarded(n, (), torch.int32),
               "best": guarded(n, (), torch.int32)}
        rc = lib().eonerf_texture_bake(ptr(lla), ptr(normal), n, ptr(self.rpcs), ptr(self.addresses), ptr(self.shapes), self.K if K is None else K,
                                       self.C, ptr(self.gain), ptr(self.bias), ptr(self.sat), ptr(blocked), min_cos, angle_weight, mode,
                                       *[ptr(out[k], GUARD) if k in want else None for k in ("colour", "wsum", "count", "best")], None)
        return rc, out


def assert_values(got, want, tol=TOL):
    """The same NaN cells, and the others within tol."""
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if ok.any():
        err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)).max()
        print("largest difference", err)
        assert err <= tol


def ulps32(got, want):
    """The largest distance in fp32 ulps between two fp32 arrays with the same NaNs."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return int(np.abs(bits(got[ok]).astype(np.int64) - bits(want[ok]).astype(np.int64)).max()) if ok.any() else 0


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name in TC.CASES:
        c = TC.make_case(name)
        s = TR.samples(c["vertices"], c["faces"], c["texels"], c["scene_offset"], c["scene_scale"], c["zone"], c["south"])
        out[name] = (c, s)
    return out


def test_version_and_layout():
    L = lib()
    assert L.eonerf_texture_version() == TR.VERSION
    out = (C.c_int64 * 3)(-1, -1, -1)
    for F, T in ((0, 4), (1, 1), (2, 64), (3, 2), (9, 5), (200000, 4), (2 * 3276 * 3276, 5)):
        assert L.eonerf_texture_layout(F, T, out) == 0
        assert tuple(out) == TR.layout(F, T)[:3], (F, T)
    assert TR.layout(2 * 3276 * 3276 + 1, 5) is None and L.eonerf_texture_layout(2 * 3276 * 3276 + 1, 5, out) == E_UNSUPPORTED
    assert L.eonerf_texture_layout((1 << 31) - 1, 1, out) == E_UNSUPPORTED
    for F, T in ((-1, 4), (1, 0), (1, 65)):
        assert L.eonerf_texture_layout(F, T, out) == E_ARG
    assert L.eonerf_texture_layout(1, 1, None) == E_ARG


@pytest.mark.parametrize("name", list(TC.CASES))
def test_uv_and_samples_match_the_contract(restated, name):
    c, want = restated[name]
    d = Device(c)
    F, T = c["faces"].shape[0], c["texels"]
    w, h, _, _ = TR.layout(F, T)
    uv = guarded(F, (3, 2), torch.float32)
    assert lib().eonerf_texture_uv(F, T, ptr(uv, GUARD), None) == 0
    np.testing.assert_array_equal(bits(inner(uv)), bits(TR.uv(F, T)))
    total = w * h
    # the whole atlas, then the block shapes: one sample, a short block, a block and one, and a range that starts inside the atlas
    for first, n in {(0, total), (0, 1), (0, min(255, total)), (min(300, total - 1), min(257, total - min(300, total - 1))), (total - 1, 1)}:
        got = d.samples(first, n)
        sl = slice(first, first + n)
        np.testing.assert_array_equal(inner(got["face"]), want["face"][sl])
        for key in ("bary", "xyz"):
            np.testing.assert_array_equal(bits(inner(got[key])), bits(want[key][sl]), err_msg=key)
        worst = ulps32(inner(got["normal"]), want["normal"][sl])
        print("normal: fp32 ulps", worst)
        assert worst <= 1
        lla, lla_want = inner(got["lla"]), want["lonlatalt"][sl]
        np.testing.assert_array_equal(np.isnan(lla), np.isnan(lla_want))
        ok = ~np.isnan(lla_want[:, 0])
        if ok.any():
            print("lon / lat: degrees", np.abs(lla[ok, :2] - lla_want[ok, :2]).max())
            assert np.abs(lla[ok, :2] - lla_want[ok, :2]).max() <= 1e-12
            np.testing.assert_array_equal(lla[ok, 2], lla_want[ok, 2])
    # outputs one by one: the others keep the sentinel
    for key in ("face", "bary", "xyz", "lla", "normal"):
        got = d.samples(0, total, want=(key,))
        for other, t in got.items():
            assert other == key or (t == S).all(), (key, other)
        assert not (got[key][GUARD:-GUARD] == S).all()


@pytest.mark.parametrize("name", list(TC.CASES))
def test_bake_matches_the_contract(restated, name):
    c, s = restated[name]
    d = Device(c)
    lla, normal = cu(s["lonlatalt"]), cu(s["normal"])
    blocked = cu(c["blocked"]) if c["blocked"] is not None else None
    n = lla.shape[0]
    for mode in (TR.MEAN, TR.MEDIAN, TR.BEST):
        for angle_weight, with_normal, with_blocked in ((1, True, True), (0, True, False), (0, False, True)):
            blk = blocked if with_blocked else None
            want = TR.bake(s["lonlatalt"], s["normal"] if with_normal else None, c["rpcs"], c["images"], c["gain"], c["bias"], c["to_satellite"],
                           c["blocked"] if with_blocked else None, c["min_cos"], angle_weight, mode)
            rc, got = d.bake(lla, normal if with_normal else None, blk, mode, angle_weight)
            assert rc == 0
            np.testing.assert_array_equal(inner(got["count"]), want["count"])
            np.testing.assert_array_equal(inner(got["best"]), want["best"])
            assert_values(inner(got["colour"]), want["colour"])
            np.testing.assert_allclose(inner(got["wsum"]), want["weight"], rtol=2e-7, atol=0)      # an fp64 sum, one fp32 rounding
    # a chunk: rows [first, first + m) of the tables, the occlusion table cut to match
    first, m = (n // 3, min(257, n - n // 3))
    want = TR.bake(s["lonlatalt"][first:first + m], s["normal"][first:first + m], c["rpcs"], c["images"], c["gain"], c["bias"], c["to_satellite"],
                   None if c["blocked"] is None else c["blocked"][:, first:first + m], c["min_cos"], True, TR.MEDIAN)
    blk = None if blocked is None else blocked[:, first:first + m].contiguous()
    rc, got = d.bake(lla[first:first + m].contiguous(), normal[first:first + m].contiguous(), blk, TR.MEDIAN)
    assert rc == 0
    np.testing.assert_array_equal(inner(got["count"]), want["count"])
    assert_values(inner(got["colour"]), want["colour"])
    # outputs one by one, and run to run
    rc, ref = d.bake(lla, normal, blocked, TR.MEDIAN)
    for key in ("colour", "wsum", "count", "best"):
        rc, got = d.bake(lla, normal, blocked, TR.MEDIAN, want=(key,))
        assert rc == 0
        for other, t in got.items():
            assert (t == S).all() if other != key else np.array_equal(bits(t.cpu().numpy()), bits(ref[key].cpu().numpy())), (key, other)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_fused_bake_equals_gather_then_fuse_bit_for_bit(restated, name):
    """normal = NULL: the fused kernel against eonerf_ortho_gather (visibility 1 - blocked, min_visibility 0.5) + eonerf_ortho_fuse on the
    same points.  An image with a zero gain, which the gather refuses on the host and the bake gives weight 0, enters as an all-zero
    visibility with gain 1."""
    from eonerf_code_amd.datasets.satellite import _rpc_struct
    c, s = restated[name]
    d = Device(c)
    L = lib()
    lla = cu(s["lonlatalt"])
    n, K, ch = lla.shape[0], d.K, d.C
    for with_blocked in (True, False):
        if with_blocked and c["blocked"] is None:
            continue
        blocked = cu(c["blocked"]) if with_blocked else None
        layers = torch.empty(K, n, ch, dtype=torch.float32, device=DEV)
        weights = torch.empty(K, n, dtype=torch.float32, device=DEV)
        for k in range(K):
            usable = bool((c["gain"][k] != 0).all())
            vis = (1.0 - blocked[k].float()) if with_blocked else torch.ones(n, dtype=torch.float32, device=DEV)
            if not usable:
                vis = torch.zeros_like(vis)
            vis = vis.contiguous()
            gain = c["gain"][k] if usable else np.ones(ch, dtype=np.float32)
            h, w = c["images"][k].shape[:2]
            rc = L.eonerf_ortho_gather(ptr(lla), n, C.byref(_rpc_struct(c["rpcs"][k])), ptr(d.images[k]), h, w, ch, f32(gain), f32(c["bias"][k]),
                                       ptr(vis), 0.5, ptr(layers[k]), ptr(weights[k]), None, None)
            assert rc == 0
        for mode in (OR.MEAN, OR.MEDIAN):
            mosaic = torch.empty(n, ch, dtype=torch.float32, device=DEV)
            wsum = torch.empty(n, dtype=torch.float32, device=DEV)
            count = torch.empty(n, dtype=torch.int32, device=DEV)
            assert L.eonerf_ortho_fuse(ptr(layers), ptr(weights), K, n, ch, mode, ptr(mosaic), ptr(wsum), ptr(count), None) == 0
            rc, got = d.bake(lla, None, blocked, mode, angle_weight=0)
            assert rc == 0
            assert (count > 0).any()
            np.testing.assert_array_equal(inner(got["count"]), count.cpu().numpy())
            np.testing.assert_array_equal(bits(inner(got["wsum"])), bits(wsum.cpu().numpy()))
            np.testing.assert_array_equal(bits(inner(got["colour"])), bits(mosaic.cpu().numpy()))


def test_k_limits_of_the_median(restated):
    c, s = restated["cap"]
    d = Device(c)
    assert d.K == TR.MAX_MEDIAN
    lla = cu(s["lonlatalt"])
    rc, got = d.bake(lla, None, None, TR.MEDIAN, K=65)               # refused on the host: the 64-entry tables are never read
    assert rc == E_UNSUPPORTED
    for t in got.values():
        assert (t == S).all()
    # the mean takes any K: 65 images, the last one the first again
    c65 = dict(c, rpcs=c["rpcs"] + c["rpcs"][:1], images=c["images"] + c["images"][:1], shapes=np.concatenate([c["shapes"], c["shapes"][:1]]),
               gain=np.concatenate([c["gain"], c["gain"][:1]]), bias=np.concatenate([c["bias"], c["bias"][:1]]),
               to_satellite=np.concatenate([c["to_satellite"], c["to_satellite"][:1]]))
    d65 = Device(c65)
    rc, got = d65.bake(lla, None, None, TR.MEAN)
    assert rc == 0
    want = TR.bake(s["lonlatalt"], None, c65["rpcs"], c65["images"], c65["gain"], c65["bias"], None, None, 0.1, False, TR.MEAN)
    assert want["count"].max() > 32                                  # (every other image has NaN pixels: not all 65 see a texel)
    np.testing.assert_array_equal(inner(got["count"]), want["count"])
    assert_values(inner(got["colour"]), want["colour"])


def test_refusals(restated):
    L = lib()
    c, s = restated["three"]
    d = Device(c)
    F, T = c["faces"].shape[0], c["texels"]
    w, h, _, _ = TR.layout(F, T)
    total = w * h
    sc, off = f32(c["scene_scale"]), f32(c["scene_offset"])
    face = torch.full((total,), int(S), dtype=torch.int32, device=DEV)
    uv = torch.full((F, 3, 2), S, dtype=torch.float32, device=DEV)
    assert L.eonerf_texture_uv(0, T, ptr(uv), None) == 0 and (uv == S).all()          # F == 0 succeeds and writes nothing
    for args in ((F, T, None), (-1, T, ptr(uv)), (F, 0, ptr(uv)), (F, 65, ptr(uv))):
        assert L.eonerf_texture_uv(*args, None) == E_ARG, args
    assert L.eonerf_texture_uv((1 << 31) - 1, 1, ptr(uv), None) == E_UNSUPPORTED

    def samples(v=d.vertices, nv=d.vertices.shape[0], t=d.faces, F=F, T=T, first=0, n=total, sc=sc, off=off, zone=c["zone"], face=face):
        return L.eonerf_texture_samples(ptr(v), nv, ptr(t), F, T, first, n, sc, off, zone, 0, ptr(face), None, None, None, None, None)
    assert samples() == 0
    face.fill_(int(S))
    assert samples(n=0) == 0 and samples(first=total, n=0) == 0 and (face == int(S)).all()
    for kw in (dict(v=None), dict(t=None), dict(sc=None), dict(off=None), dict(face=None), dict(nv=-1), dict(F=-1), dict(first=-1), dict(n=-1),
               dict(T=0), dict(T=65), dict(sc=f32([300, float("nan"), 60])), dict(off=f32([float("inf"), 0, 0])), dict(zone=0), dict(zone=61),
               dict(first=1), dict(first=total, n=1), dict(first=total + 1, n=0), dict(n=total + 1)):
        assert samples(**kw) == E_ARG, kw
    assert samples(nv=1 << 31) == E_UNSUPPORTED and samples(F=(1 << 31) - 1, T=1) == E_UNSUPPORTED
    assert (face == int(S)).all()

    lla = cu(s["lonlatalt"])
    colour = torch.full((total, d.C), S, dtype=torch.float32, device=DEV)

    def bake(lla=lla, normal=None, n=total, rpcs=d.rpcs, addr=d.addresses, shapes=d.shapes, K=d.K, ch=d.C, gain=d.gain, bias=d.bias, sat=d.sat,
             min_cos=0.1, aw=1, mode=0, colour=colour):
        return L.eonerf_texture_bake(ptr(lla), ptr(normal), n, ptr(rpcs), ptr(addr), ptr(shapes), K, ch, ptr(gain), ptr(bias), ptr(sat), None,
                                     min_cos, aw, mode, ptr(colour), None, None, None, None)
    assert bake() == 0
    colour.fill_(S)
    assert bake(n=0) == 0 and (colour == S).all()
    normal = cu(s["normal"])
    for kw in (dict(lla=None), dict(rpcs=None), dict(addr=None), dict(shapes=None), dict(gain=None), dict(bias=None), dict(normal=normal, sat=None),
               dict(colour=None), dict(n=-1), dict(K=0), dict(ch=0), dict(ch=5), dict(mode=-1), dict(mode=3), dict(aw=2), dict(aw=-1),
               dict(min_cos=float("nan")), dict(min_cos=float("inf"))):
        assert bake(**kw) == E_ARG, kw
    assert bake(K=65, mode=1) == E_UNSUPPORTED
    assert (colour == S).all()
    torch.cuda.synchronize()
