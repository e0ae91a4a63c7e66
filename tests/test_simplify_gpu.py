"""GPU, C ABI: the simplification group (eonerf_code_amd/csrc/eonerf_simplify.h) against the numpy restatement of its rule
(tests/simplify_restated.py), bit for bit: out_vertices, out_triangles, source, vertex_map, the four counts and the status word, in both
modes.

Shapes (tests/simplify_cases.py): one cell holding all vertices, a 1 x 1 x 1 and a 4096 x 1 x 1 grid; the 9^3 and 33^3 spheres with cells
of 2 and 3 spacings; 65 vertices in one cell, 64 + 1, runs of equal cells that end at, cross and start at a wave boundary, alternate, and
are broken by dropped vertices (the pre-aggregation's corners); more than 1024 and more than 1024^2 occupied cells and triangles (every
scan level); vertices that are not finite or far outside the grid, indices outside the mesh, equal-distance ties, ties to even; no
vertices, no triangles; capacities one too small; the triangles and the vertices of the 33^3 sphere permuted.  The workspace arrives
filled with 0x00 and with 0xFF, and every buffer sits between guards (workspace_guard.Guarded), checked after every call.

These tests do not aim at a fault: with correct kernels every access stays inside the test's own allocations."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import simplify_cases as sc
import simplify_restated as sr
import workspace_guard as wg

pytestmark = pytest.mark.gpu
E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
STATUS_CAPACITY = 1
# The coarsest step a kernel of the group takes through a buffer is one row: 24 bytes of cell sums, 12 of a vertex or a triangle; 64 KiB
# of guard on either side covers a store that misses by thousands of such steps.
GUARD = 1 << 16
CASES = sc.cases()
IDS = [c["name"].replace(" ", "_").replace(":", "").replace(",", "") for c in CASES]


@functools.lru_cache(maxsize=None)
def lib():
    from eonerf_code_amd import _lib
    return _lib.lib()


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


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
    """The first n rows of a guarded buffer as numpy."""
    t = buf.payload[:n * width * 4].view(dtype)
    return t.cpu().numpy().reshape(n, width) if width > 1 else t.cpu().numpy().reshape(n)


def device_simplify(c, representative, ws_fill=0xFF, short_v=0, short_t=0, optional=True):
    """count, one read-back of the counts, emit into buffers of exactly the counted size (less short_v / short_t rows)."""
    L = lib()
    n_v, n_t = len(c["vertices"]), len(c["triangles"])
    origin, cell, dims = f3(c["origin"]), f3(c["cell"]), i3(c["dims"])
    nb = L.eonerf_simplify_workspace_bytes(dims, n_v, n_t)
    assert nb > 0, c["name"]
    vert, tri, ws, counts = upload("vertices", c["vertices"]), upload("triangles", c["triangles"]), guarded("workspace", nb, ws_fill), guarded("counts", 32)
    rc = L.eonerf_simplify_count(vert.ptr, n_v, tri.ptr, n_t, origin, cell, dims, ws.ptr, nb, counts.ptr, stream())
    assert rc == 0, (c["name"], rc)
    wg.check_guards("eonerf_simplify_count: " + c["name"], [vert, tri, ws, counts])
    got = {"counts": counts.view(torch.int64, 4).cpu().numpy()}
    cap_v, cap_t = max(int(got["counts"][0]) - short_v, 0), max(int(got["counts"][1]) - short_t, 0)
    out_v, out_t, status = guarded("out_vertices", max(12 * cap_v, 4)), guarded("out_triangles", max(12 * cap_t, 4)), guarded("status", 4)
    source = guarded("source", max(4 * cap_v, 4)) if optional else None
    vmap = guarded("vertex_map", max(4 * n_v, 4)) if optional else None
    rc = L.eonerf_simplify_emit(vert.ptr, n_v, tri.ptr, n_t, origin, cell, dims, representative, ws.ptr, nb, out_v.ptr, cap_v, out_t.ptr, cap_t,
                                source.ptr if optional else None, vmap.ptr if optional else None, status.ptr, stream())
    assert rc == 0, (c["name"], rc)
    bufs = [vert, tri, ws, counts, out_v, out_t, status] + ([source, vmap] if optional else [])
    wg.check_guards("eonerf_simplify_emit: " + c["name"], bufs)
    got.update(vertices=rows(out_v, torch.float32, cap_v, 3), triangles=rows(out_t, torch.int32, cap_t, 3), status=int(status.view(torch.int32, 1).item()),
               counts_after=counts.view(torch.int64, 4).cpu().numpy(), cap=(cap_v, cap_t), all=bufs)
    if optional:
        got.update(source=rows(source, torch.int32, cap_v, 1), vertex_map=rows(vmap, torch.int32, n_v, 1))
    return got


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def restated(index, representative):
    c = CASES[index]
    return sr.simplify(c["vertices"], c["triangles"], c["origin"], c["cell"], c["dims"], representative)


def check(got, want, name):
    cap_v, cap_t = got["cap"]
    assert got["counts"].tolist() == want["counts"].tolist() == got["counts_after"].tolist(), (name, got["counts"].tolist(), want["counts"].tolist())
    fits = cap_v >= want["counts"][0] and cap_t >= want["counts"][1]
    assert got["status"] == (0 if fits else STATUS_CAPACITY), (name, got["status"])
    assert same_bits(got["vertices"], want["vertices"][:cap_v]), name
    assert same_bits(got["triangles"], want["triangles"][:cap_t]), name
    if "source" in got:
        assert same_bits(got["source"], want["source"][:cap_v]), name
        assert same_bits(got["vertex_map"], want["vertex_map"]), name


@pytest.mark.parametrize("representative", [sr.MEAN, sr.NEAREST], ids=["mean", "nearest"])
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_case_equals_the_restatement(index, representative):
    c = CASES[index]
    got = device_simplify(c, representative, ws_fill=0xFF if representative == sr.MEAN else 0x00)
    check(got, restated(index, representative), c["name"])
    assert int(got["counts"][1:].sum()) == len(c["triangles"])


def test_listed_counts_and_scan_levels():
    by_name = {c["name"]: restated(i, sr.MEAN)["counts"].tolist() for i, c in enumerate(CASES)}
    assert by_name["sphere 9^3 k 2"][:2] == [50, 96] and by_name["sphere 33^3 k 2"][:2] == [654, 1304]
    assert by_name["sphere 9^3 in a 1 x 1 x 1 grid"] == [1, 0, 0, 940] and by_name["sphere 9^3 in one cell of 3 x 3 x 3"] == [1, 0, 0, 940]
    big = by_name["sphere 33^3 k 1: more than 1024 occupied cells and triangles"]
    assert big[0] > 1024 and big[1] > 1024
    assert by_name["sphere 33^3, its triangles 67 times"][1] > 1024 * 1024 // 16 and 67 * 15672 > 1024 * 1024
    assert by_name["sphere 33^3 in 129 x 129 x 65 cells"][0] > 1024 and 129 * 129 * 65 > 1024 * 1024


def case_named(name):
    index = next(i for i, c in enumerate(CASES) if c["name"] == name)
    return index, CASES[index]


@pytest.mark.parametrize("representative", [sr.MEAN, sr.NEAREST], ids=["mean", "nearest"])
def test_capacities_one_too_small(representative):
    index, c = case_named("sphere 9^3 k 2")
    want = restated(index, representative)
    for short_v, short_t in ((1, 0), (0, 1), (1, 1)):
        got = device_simplify(c, representative, short_v=short_v, short_t=short_t)
        assert got["status"] == STATUS_CAPACITY
        check(got, want, (c["name"], short_v, short_t))      # the rows that fit are the right ones; the guards saw nothing beyond them


def test_order_of_triangles_and_of_vertices_does_not_matter():
    index, c = case_named("sphere 33^3 k 2")
    rng = np.random.default_rng(7)
    for representative in (sr.MEAN, sr.NEAREST):
        base = device_simplify(c, representative)
        check(base, restated(index, representative), c["name"])
        perm = rng.permutation(len(c["triangles"]))
        other = dict(c, name=c["name"] + ", triangles permuted", triangles=np.ascontiguousarray(c["triangles"][perm]))
        got = device_simplify(other, representative)
        check(got, sr.simplify(other["vertices"], other["triangles"], c["origin"], c["cell"], c["dims"], representative), other["name"])
        assert same_bits(got["vertices"], base["vertices"]) and same_bits(got["source"], base["source"]) and same_bits(got["vertex_map"], base["vertex_map"])
        assert sorted(map(tuple, got["triangles"].tolist())) == sorted(map(tuple, base["triangles"].tolist()))
        # vertices permuted, triangles renamed: new vertex j is old vertex perm[j]
        perm = rng.permutation(len(c["vertices"]))
        inverse = np.empty_like(perm)
        inverse[perm] = np.arange(len(perm))
        other = dict(c, name=c["name"] + ", vertices permuted", vertices=np.ascontiguousarray(c["vertices"][perm]),
                     triangles=np.ascontiguousarray(inverse[c["triangles"]].astype(np.int32)))
        got = device_simplify(other, representative)
        check(got, sr.simplify(other["vertices"], other["triangles"], c["origin"], c["cell"], c["dims"], representative), other["name"])
        assert same_bits(got["triangles"], base["triangles"]) and same_bits(got["vertex_map"], base["vertex_map"][perm])
        cells = sr.quantise(c["vertices"], c["origin"], c["cell"], c["dims"])[0]
        assert (cells[perm[got["source"]]] == cells[base["source"]]).all()
        if representative == sr.MEAN:
            assert same_bits(got["vertices"], base["vertices"])


def test_two_calls_agree_whatever_the_workspace_held_and_the_optional_outputs_may_be_null():
    index, c = case_named("sphere 33^3 k 3")
    runs = [device_simplify(c, sr.MEAN, ws_fill=fill, optional=opt) for fill, opt in ((0x00, True), (0xFF, True), (0xA7, False), (0xFF, True))]
    for other in runs:
        check(other, restated(index, sr.MEAN), c["name"])
        assert same_bits(other["vertices"], runs[0]["vertices"]) and same_bits(other["triangles"], runs[0]["triangles"])


def test_emit_twice_from_one_count_in_both_modes():
    """One count call feeds a MEAN and then a NEAREST emit (and a MEAN one again): the workspace is left as the count call made it."""
    L = lib()
    index, c = case_named("sphere 9^3 k 3")
    n_v, n_t = len(c["vertices"]), len(c["triangles"])
    origin, cell, dims = f3(c["origin"]), f3(c["cell"]), i3(c["dims"])
    nb = L.eonerf_simplify_workspace_bytes(dims, n_v, n_t)
    vert, tri, ws, counts = upload("vertices", c["vertices"]), upload("triangles", c["triangles"]), guarded("workspace", nb), guarded("counts", 32)
    assert L.eonerf_simplify_count(vert.ptr, n_v, tri.ptr, n_t, origin, cell, dims, ws.ptr, nb, counts.ptr, stream()) == 0
    n_out, kept = counts.view(torch.int64, 4).cpu().numpy()[:2].tolist()
    for representative in (sr.MEAN, sr.NEAREST, sr.MEAN):
        want = restated(index, representative)
        out_v, out_t, status = guarded("out_vertices", 12 * n_out), guarded("out_triangles", 12 * kept), guarded("status", 4)
        assert L.eonerf_simplify_emit(vert.ptr, n_v, tri.ptr, n_t, origin, cell, dims, representative, ws.ptr, nb, out_v.ptr, n_out, out_t.ptr, kept, None, None,
                                      status.ptr, stream()) == 0
        wg.check_guards("eonerf_simplify_emit again", [vert, tri, ws, counts, out_v, out_t, status])
        assert same_bits(rows(out_v, torch.float32, n_out, 3), want["vertices"]) and same_bits(rows(out_t, torch.int32, kept, 3), want["triangles"])
        assert int(status.view(torch.int32, 1).item()) == 0


def test_refusals_write_nothing():
    L = lib()
    index, c = case_named("sphere 9^3 k 2")
    n_v, n_t = len(c["vertices"]), len(c["triangles"])
    origin, cell, dims = f3(c["origin"]), f3(c["cell"]), i3(c["dims"])
    nb = L.eonerf_simplify_workspace_bytes(dims, n_v, n_t)
    vert, tri = upload("vertices", c["vertices"]), upload("triangles", c["triangles"])
    ws, counts = guarded("workspace", nb), guarded("counts", 32)
    out_v, out_t, source, vmap, status = guarded("out_vertices", 12 * 50), guarded("out_triangles", 12 * 96), guarded("source", 4 * 50), guarded("vertex_map", 4 * n_v), guarded("status", 4)
    everything = [vert, tri, ws, counts, out_v, out_t, source, vmap, status]

    def count(v=vert.ptr, nv=n_v, t=tri.ptr, nt=n_t, o=origin, ce=cell, d=dims, w=ws.ptr, b=nb, cn=counts.ptr):
        return L.eonerf_simplify_count(v, nv, t, nt, o, ce, d, w, b, cn, stream())

    def emit(v=vert.ptr, nv=n_v, t=tri.ptr, nt=n_t, o=origin, ce=cell, d=dims, rep=sr.MEAN, w=ws.ptr, b=nb, ov=out_v.ptr, cv=50, ot=out_t.ptr, ct=96, st=status.ptr):
        return L.eonerf_simplify_emit(v, nv, t, nt, o, ce, d, rep, w, b, ov, cv, ot, ct, source.ptr, vmap.ptr, st, stream())

    def refused(call, want, **kw):
        assert call(**kw) == want, (call.__name__, kw)
        wg.check_guards(f"refused {call.__name__}({', '.join(kw)})", everything)
        for b in (ws, counts, out_v, out_t, source, vmap, status):
            assert bool((b.payload == 0xFF).all()), (b.name, kw)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(v=None), dict(t=None), dict(o=None), dict(ce=None), dict(d=None), dict(w=None), dict(nv=-1), dict(nt=-5), dict(o=f3((nan, 0, 0))),
               dict(o=f3((0, inf, 0))), dict(ce=f3((1, 0, 1))), dict(ce=f3((1, 1, -2))), dict(ce=f3((nan, 1, 1))), dict(ce=f3((1, inf, 1)))):
        refused(count, E_ARG, **kw)
        refused(emit, E_ARG, **kw)
    refused(count, E_ARG, cn=None)
    for kw in (dict(ov=None), dict(ot=None), dict(st=None), dict(cv=-1), dict(ct=-1), dict(rep=2), dict(rep=-1)):
        refused(emit, E_ARG, **kw)
    for kw in (dict(nv=1 << 31), dict(nt=1 << 40), dict(d=i3((4097, 1, 1))), dict(d=i3((0, 4, 4))), dict(d=i3((4, -1, 4))), dict(d=i3((1024, 512, 512)))):
        refused(count, E_UNSUPPORTED, **kw)
        refused(emit, E_UNSUPPORTED, **kw)
    for kw in (dict(b=nb - 1), dict(b=0)):
        refused(count, E_WORKSPACE, **kw)
        refused(emit, E_WORKSPACE, **kw)
    # the order: nulls, negative counts, the limits, dims, the values, the workspace, the representative
    refused(emit, E_ARG, ov=None, nv=-1, d=i3((4097, 1, 1)), b=0, rep=7)
    refused(emit, E_ARG, nv=-1, nt=1 << 40, d=i3((4097, 1, 1)), b=0, rep=7)
    refused(emit, E_UNSUPPORTED, nt=1 << 40, ce=f3((0, 1, 1)), b=0, rep=7)
    refused(emit, E_UNSUPPORTED, d=i3((4097, 1, 1)), ce=f3((0, 1, 1)), b=0, rep=7)
    refused(emit, E_ARG, ce=f3((0, 1, 1)), b=0)
    refused(emit, E_WORKSPACE, b=0, rep=7)
    refused(emit, E_ARG, rep=7)
    assert L.eonerf_simplify_workspace_bytes(i3((4097, 1, 1)), 1, 1) == 0 and L.eonerf_simplify_workspace_bytes(dims, -1, 1) == 0
    assert L.eonerf_simplify_workspace_bytes(None, 1, 1) == 0 and L.eonerf_simplify_workspace_bytes(i3((512, 512, 512)), 0, 0) > 38 << 27
    assert count() == 0 and emit() == 0
    wg.check_guards("count + emit", everything)
    want = restated(index, sr.MEAN)
    assert same_bits(rows(out_v, torch.float32, 50, 3), want["vertices"]) and same_bits(rows(vmap, torch.int32, n_v, 1), want["vertex_map"])
    assert L.eonerf_simplify_version() == 1
