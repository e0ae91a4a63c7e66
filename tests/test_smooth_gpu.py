"""GPU, C ABI: the smoothing group (eonerf_code_amd/csrc/eonerf_smooth.h) against the numpy restatement of its rule
(tests/smooth_restated.py), bit for bit: out_vertices, the six counts and the status word.

Shapes (tests/smooth_cases.py): one triangle, a closed tetrahedron, hubs of 300 and of 1,100 corners (one lane loops over them all),
open and balanced vertices of every kind the rule names, faces with repeated indices, duplicates and twins, indices outside the mesh,
vertices that are not finite or lie at |u| = 8192, vertices without a face, no faces, no vertices; the 9^3, 17^3 and 33^3 spheres (more
than one tile of vertices), the cut sphere with its open rim, 1,025 vertices (one beyond a tile), the clamp, factors of 0, 1 and -1, 1
and 40 steps; more than 1024^2 corners and more than 1024^2 vertices (the third scan level).  The workspace arrives filled with 0x00
and with 0xFF, and every buffer sits between guards (workspace_guard.Guarded), checked after every call.

These tests do not aim at a fault: with correct kernels every access stays inside the test's own allocations."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import smooth_cases as sc
import smooth_restated as sm
import workspace_guard as wg

pytestmark = pytest.mark.gpu
E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
# The coarsest step a kernel of the group takes through a buffer is one 16-byte record; 64 KiB of guard on either side covers a store
# that misses by thousands of such steps.
GUARD = 1 << 16
CASES = sc.cases()
IDS = [c["name"].replace(" ", "_").replace(":", "").replace(",", "") for c in CASES]


@functools.lru_cache(maxsize=None)
def lib():
    from eonerf_code_amd import _lib
    return _lib.lib()


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def i32(v):
    return (C.c_int32 * max(len(v), 1))(*[int(x) for x in v])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(name, nbytes, fill=0xFF):
    return wg.Guarded(name, nbytes, "cuda", guard=GUARD, fill=fill)


def upload(name, array):
    array = np.ascontiguousarray(array)
    buf = guarded(name, max(array.nbytes, 4))
    if array.nbytes:
        buf.payload[:array.nbytes].copy_(torch.from_numpy(array.reshape(-1).view(np.uint8)))
    return buf


def rows(buf, dtype, n, width):
    t = buf.payload[:n * width * 4].view(dtype)
    return t.cpu().numpy().reshape(n, width)


class Built:
    """One eonerf_smooth_build of a case: the buffers, and run(steps) into a fresh guarded output."""

    def __init__(self, c, ws_fill=0xFF, pinned="case", pin_open=None):
        L = lib()
        self.c, self.n_v, self.n_t = c, len(c["vertices"]), len(c["triangles"])
        self.origin, self.unit = f3(c["origin"]), f3(c["unit"])
        mask = c["pinned"] if isinstance(pinned, str) else pinned
        self.nb = L.eonerf_smooth_workspace_bytes(self.n_v, self.n_t)
        assert self.nb > 0, c["name"]
        self.vert, self.tri = upload("vertices", c["vertices"]), upload("triangles", c["triangles"])
        self.mask = upload("pinned", mask) if mask is not None else None
        self.ws, self.counts = guarded("workspace", self.nb, ws_fill), guarded("counts", 48)
        self.bufs = [self.vert, self.tri, self.ws, self.counts] + ([self.mask] if self.mask is not None else [])
        rc = L.eonerf_smooth_build(self.vert.ptr, self.n_v, self.tri.ptr, self.n_t, self.origin, self.unit, self.mask.ptr if self.mask is not None else None,
                                   int(c["pin_open"] if pin_open is None else pin_open), self.ws.ptr, self.nb, self.counts.ptr, stream())
        assert rc == 0, (c["name"], rc)
        wg.check_guards("eonerf_smooth_build: " + c["name"], self.bufs)

    def run(self, steps):
        out, status = guarded("out_vertices", max(12 * self.n_v, 4)), guarded("status", 4)
        rc = lib().eonerf_smooth_run(self.vert.ptr, self.n_v, self.n_t, self.origin, self.unit, i32(steps), len(steps), self.ws.ptr, self.nb, out.ptr, status.ptr, stream())
        assert rc == 0, (self.c["name"], rc)
        wg.check_guards("eonerf_smooth_run: " + self.c["name"], self.bufs + [out, status])
        return {"vertices": rows(out, torch.float32, self.n_v, 3), "status": int(status.view(torch.int32, 1).item()),
                "counts": self.counts.view(torch.int64, 6).cpu().numpy()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def restate(c, steps=None, pinned="case", pin_open=None):
    return sm.smooth(c["vertices"], c["triangles"], c["origin"], c["unit"], c["steps"] if steps is None else steps, c["pinned"] if isinstance(pinned, str) else pinned,
                     c["pin_open"] if pin_open is None else pin_open)


@functools.lru_cache(maxsize=None)
def restated(index):
    return restate(CASES[index])


def check(got, want, name):
    assert got["counts"].tolist() == want["counts"].tolist(), (name, got["counts"].tolist(), want["counts"].tolist())
    assert got["status"] == want["status"], (name, got["status"])
    if not same_bits(got["vertices"], want["vertices"]):
        bad = np.nonzero((got["vertices"].view(np.uint32) != want["vertices"].view(np.uint32)).any(axis=1))[0]
        raise AssertionError((name, len(bad), bad[:5].tolist(), got["vertices"][bad[:3]].tolist(), want["vertices"][bad[:3]].tolist()))


def case_named(name):
    index = next(i for i, c in enumerate(CASES) if c["name"] == name)
    return index, CASES[index]


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_case_equals_the_restatement(index):
    c = CASES[index]
    got = Built(c, ws_fill=0xFF if index % 2 else 0x00).run(c["steps"])
    check(got, restated(index), c["name"])


def test_listed_counts():
    by_name = {c["name"]: restated(i) for i, c in enumerate(CASES) if not c["big"]}
    assert by_name["the 300-gon bipyramid"]["counts"].tolist() == [302, 0, 0, 0, 0, 0]
    assert by_name["a fan of 1100 faces around one vertex"]["counts"].tolist() == [1, 1100, 0, 0, 0, 0]
    assert by_name["a tetrahedron near +8191.9 units under lam_q = -65536: the clamp"]["status"] == sm.STATUS_CLAMPED
    assert by_name["sphere 33^3"]["counts"][0] > 1024 and by_name["vertices without a face"]["counts"][3] == 37
    assert by_name["no vertices"]["counts"].tolist() == [0, 0, 0, 0, 0, 2]
    cut = by_name["sphere 17^3 cut at z = 8"]["counts"]
    assert cut[1] > 0 and cut[0] + cut[1] == len(case_named("sphere 17^3 cut at z = 8")[1]["vertices"])


def test_permuted_faces_give_the_same_bits():
    index, c = case_named("sphere 33^3")
    rng = np.random.default_rng(7)
    base = Built(c).run(c["steps"])
    check(base, restated(index), c["name"])
    perm = rng.permutation(len(c["triangles"]))
    other = dict(c, name=c["name"] + ", faces permuted and rotated", triangles=np.ascontiguousarray(np.stack([np.roll(row, k % 3) for k, row in enumerate(c["triangles"][perm])])))
    got = Built(other).run(c["steps"])
    check(got, base, other["name"])


def test_one_build_feeds_three_runs_and_a_run_can_be_repeated():
    index, c = case_named("sphere 17^3 cut at z = 8")
    built = Built(c, ws_fill=0xA7)
    lists = [sm.taubin(2), [sm.lam_q(0.5)], sm.taubin(5, mu=None), sm.taubin(2)]
    runs = [built.run(steps) for steps in lists]
    for steps, got in zip(lists, runs):
        check(got, restate(c, steps), (c["name"], len(steps)))
    assert same_bits(runs[0]["vertices"], runs[3]["vertices"]) and not same_bits(runs[0]["vertices"], runs[1]["vertices"])


def test_two_builds_agree_whatever_the_workspace_held():
    index, c = case_named("sphere 17^3")
    runs = [Built(c, ws_fill=fill).run(c["steps"]) for fill in (0x00, 0xFF, 0xA7)]
    for got in runs:
        check(got, restated(index), c["name"])


def test_pinned_masks_and_pin_open():
    _, c = case_named("sphere 17^3 cut at z = 8")
    rng = np.random.default_rng(8)
    n_v = len(c["vertices"])
    for mask in (np.zeros(n_v, np.uint8), np.ones(n_v, np.uint8), (rng.uniform(0, 1, n_v) < 0.5).astype(np.uint8) * 255):
        for pin_open in (0, 1):
            got = Built(c, pinned=mask, pin_open=pin_open).run(c["steps"])
            want = restate(c, pinned=mask, pin_open=bool(pin_open))
            check(got, want, (c["name"], int(mask.sum()), pin_open))
            held = ~want["free"]
            assert same_bits(got["vertices"][held], c["vertices"][held])
    everything = Built(c, pinned=np.ones(n_v, np.uint8)).run(c["steps"])
    assert same_bits(everything["vertices"], c["vertices"]) and everything["counts"][0] == 0


def test_refusals_write_nothing():
    L = lib()
    _, c = case_named("sphere 9^3")
    n_v, n_t = len(c["vertices"]), len(c["triangles"])
    origin, unit = f3(c["origin"]), f3(c["unit"])
    nb = L.eonerf_smooth_workspace_bytes(n_v, n_t)
    vert, tri = upload("vertices", c["vertices"]), upload("triangles", c["triangles"])
    ws, counts, out, status = guarded("workspace", nb), guarded("counts", 48), guarded("out_vertices", 12 * n_v), guarded("status", 4)
    everything = [vert, tri, ws, counts, out, status]
    steps = i32(c["steps"])

    def build(v=vert.ptr, nv=n_v, t=tri.ptr, nt=n_t, o=origin, u=unit, w=ws.ptr, b=nb, cn=counts.ptr):
        return L.eonerf_smooth_build(v, nv, t, nt, o, u, None, 1, w, b, cn, stream())

    def run(v=vert.ptr, nv=n_v, nt=n_t, o=origin, u=unit, lam=steps, n=len(c["steps"]), w=ws.ptr, b=nb, ov=out.ptr, st=status.ptr):
        return L.eonerf_smooth_run(v, nv, nt, o, u, lam, n, w, b, ov, st, stream())

    def refused(call, want, **kw):
        assert call(**kw) == want, (call.__name__, kw)
        wg.check_guards(f"refused {call.__name__}({', '.join(kw)})", everything)
        for b in (ws, counts, out, status):
            assert bool((b.payload == 0xFF).all()), (b.name, kw)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(v=None), dict(o=None), dict(u=None), dict(w=None), dict(nv=-1), dict(nt=-5), dict(o=f3((nan, 0, 0))), dict(o=f3((0, inf, 0))), dict(u=f3((1, 0, 1))),
               dict(u=f3((1, 1, -2))), dict(u=f3((nan, 1, 1))), dict(u=f3((1, inf, 1)))):
        refused(build, E_ARG, **kw)
        refused(run, E_ARG, **kw)
    for kw in (dict(t=None), dict(cn=None)):
        refused(build, E_ARG, **kw)
    for kw in (dict(ov=None), dict(st=None), dict(lam=None), dict(n=0), dict(n=-1), dict(n=4097, lam=i32([0] * 4097)), dict(lam=i32([65537] + c["steps"][1:])),
               dict(lam=i32(c["steps"][:-1] + [-65537]))):
        refused(run, E_ARG, **kw)
    for kw in (dict(nv=1 << 31), dict(nt=(1 << 29) + 1), dict(nt=1 << 40)):
        refused(build, E_UNSUPPORTED, **kw)
        refused(run, E_UNSUPPORTED, **kw)
    for kw in (dict(b=nb - 1), dict(b=0)):
        refused(build, E_WORKSPACE, **kw)
        refused(run, E_WORKSPACE, **kw)
    # the order: nulls, negative counts, the limits, the values, the number of steps, the factors, the workspace
    refused(run, E_ARG, ov=None, nv=-1, u=f3((0, 1, 1)), n=0, b=0)
    refused(run, E_ARG, nv=-1, nt=1 << 40, u=f3((0, 1, 1)), n=0, b=0)
    refused(run, E_UNSUPPORTED, nt=1 << 40, u=f3((0, 1, 1)), n=0, b=0)
    refused(run, E_ARG, u=f3((0, 1, 1)), b=0)
    refused(run, E_ARG, n=0, b=0)
    refused(run, E_ARG, lam=i32([70000] * len(c["steps"])), b=0)
    refused(run, E_WORKSPACE, b=0)
    refused(build, E_UNSUPPORTED, nt=1 << 40, u=f3((0, 1, 1)), b=0)
    assert L.eonerf_smooth_workspace_bytes(-1, 1) == 0 and L.eonerf_smooth_workspace_bytes(1 << 31, 1) == 0 and L.eonerf_smooth_workspace_bytes(1, (1 << 29) + 1) == 0
    assert L.eonerf_smooth_workspace_bytes((1 << 31) - 1, 1 << 29) > 60 * ((1 << 31) - 1) + (24 << 29) and L.eonerf_smooth_workspace_bytes(0, 0) > 0
    assert build() == 0 and run() == 0
    wg.check_guards("build + run", everything)
    got = {"vertices": rows(out, torch.float32, n_v, 3), "status": int(status.view(torch.int32, 1).item()), "counts": counts.view(torch.int64, 6).cpu().numpy()}
    check(got, restate(c, pinned=None, pin_open=True), c["name"])
    assert L.eonerf_smooth_version() == 1
