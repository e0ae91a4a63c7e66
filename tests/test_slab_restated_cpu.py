"""CPU: tests/slab_restated.py against itself (encode / decode round trips) and against the headers (a stand-alone program that includes
csrc/eonerf_kernels.h and csrc/eonerf_wgrad_plan.h prints ActMap / GrdMap, the encoding column map, P::feat and the operand offsets of
every job of the weight-gradient plan; built host-only like the neighbouring host tests, without a sanitizer)."""
import os
import subprocess

import pytest
import torch

from conftest import REPO
import slab_restated as sr

HIPCC = "/opt/rocm/bin/hipcc"
P_CAPS = [256, 512, 1280]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("p_cap", P_CAPS)
def test_block_round_trip(precision, p_cap):
    """Every block of both slabs: encode o decode is the identity, blocks do not overlap, and a decoded element sits at the byte the
    segment formula names."""
    c = sr.K()
    nt = p_cap // sr.seg_samples(precision)
    esz = 2 if precision == "bf16" else 4
    g = torch.Generator().manual_seed(p_cap)
    for rows_total, blk in ((c["ACT_ROWS_FULL"], sr.act_block), (c["GRD_ROWS_FULL"], sr.grd_block)):
        ws = torch.zeros(rows_total * p_cap * esz + 512, dtype=torch.uint8)
        off = 256
        dense, r = {}, 0
        while r < rows_total:
            s, n = blk(r)
            assert s == r
            dense[s] = torch.randn(n, p_cap, generator=g).to(sr.act_dtype(precision))
            sr.encode_block(ws, off, s, n, nt, precision, dense[s])
            r += n
        assert not bool(ws[:off].any()) and not bool(ws[off + rows_total * p_cap * esz:].any())
        for s, d in dense.items():
            n = d.shape[0]
            back = sr.decode_block(ws, off, s, n, nt, precision)
            assert back.dtype == d.dtype and torch.equal(back, d)
            for row, p in ((s, 0), (s + n - 1, p_cap - 1), (s + n // 2, p_cap // 2 + 3)):
                ts = sr.seg_samples(precision)
                b = off + sr.segment_offset((s, n), row, p // ts, nt) + (p % ts) * esz
                assert torch.equal(ws[b:b + esz].view(d.dtype)[0], d[row - s, p])


@pytest.mark.parametrize("p_cap", P_CAPS)
def test_unit_order_round_trip(p_cap):
    g = torch.Generator().manual_seed(p_cap + 1)
    steps = p_cap // 32
    d = torch.randn(256, p_cap, generator=g).to(torch.bfloat16)
    ws = torch.zeros(steps * sr.K()["PIPE_UNIT_B"] + 512, dtype=torch.uint8)
    sr.encode_units(ws, 256, steps, d)
    assert torch.equal(sr.decode_units(ws, 256, steps), d)
    assert not bool(ws[:256].any()) and not bool(ws[256 + steps * sr.K()["PIPE_UNIT_B"]:].any())
    # element (feature f, sample p): step p / 32, k-group f / 16, lane 32 h + p % 32, element e with feat(kg, h, e) = f
    for f, p in ((0, 0), (5, 33), (255, p_cap - 1), (100, 77)):
        kg, rem = divmod(f, 16)
        h, e = (rem % 8) // 4, (rem // 8) * 4 + rem % 4
        b = 256 + ((p // 32) * 16 + kg) * 1024 + (32 * h + p % 32) * 16 + 2 * e
        assert torch.equal(ws[b:b + 2].view(torch.bfloat16)[0], d[f, p])


@pytest.fixture(scope="module")
def header_tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slab_tables") / "slab_tables")
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", os.path.join(REPO, "tests", "host", "slab_tables.cpp"),
           os.path.join(REPO, "eonerf_code_amd", "csrc", "eonerf_pack.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    out = {}
    for p_cap in P_CAPS:
        r = subprocess.run([exe, str(p_cap)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "slab tables ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        out[p_cap] = [ln.split() for ln in r.stdout.splitlines()]
    return out


def test_row_tables_match_the_headers(header_tables):
    c = sr.K()
    rows = header_tables[P_CAPS[0]]
    act = [(int(a), int(b), int(d)) for k, a, b, d in (x for x in rows if x[0] == "act")]
    grd = [(int(a), int(b), int(d)) for k, a, b, d in (x for x in rows if x[0] == "grd")]
    assert len(act) == c["ACT_ROWS_FULL"] and len(grd) == c["GRD_ROWS_FULL"]
    for r, s, n in act:
        assert sr.act_block(r) == (s, n), (r, s, n)
    for r, s, n in grd:
        assert sr.grd_block(r) == (s, n), (r, s, n)
    enc = {(int(x[1]), int(x[2])): int(x[3]) for x in rows if x[0] == "enc"}
    for prec, flag in (("bf16", 1), ("fp32", 0)):
        cols = sr.enc_col_of_row(prec)
        assert cols == [enc[(flag, s)] for s in range(64)]
        assert sorted(k for k in cols if k >= 0) == list(range(63)) and cols.count(-1) == 1
    feat = {(int(x[1]), int(x[2]), int(x[3]), int(x[4])): int(x[5]) for x in rows if x[0] == "feat"}
    idx = sr._unit_feature_index()
    for kg in range(16):
        for h in range(2):
            for e in range(8):
                assert int(idx[kg, h, e]) == feat[(1, kg, h, e)]
    # the encoding rows: slot q = kg * NE + e of half h is stored at row feat(kg, h, e)
    for prec, flag, ne in (("bf16", 1, 8), ("fp32", 0, 4)):
        for kg in range(64 // (2 * ne)):
            for h in range(2):
                for e in range(ne):
                    assert sr.enc_hq_of_row(prec, feat[(flag, kg, h, e)]) == (h, kg * ne + e)


def _plan_rows(full):
    """(gradient row, activation row) of the jobs of wgrad_plan in table order: chain + GEMM path, transient head in the graph, no riders."""
    c = sr.K()
    trunk = [(c["GRD_ROW_Y0"], c["ACT_ROW_ENC"])]
    for l in range(1, 8):
        trunk.append((c["GRD_ROW_Y0"] + 256 * l, c["ACT_ROW_X1"] + 256 * (l - 1)))
        if l == 5:
            trunk.append((c["GRD_ROW_Y0"] + 256 * 5, c["ACT_ROW_ENC"]))
    trunk.append((c["GRD_ROW_SIG"], c["ACT_ROW_X1"] + 256 * 7))
    if not full:
        return trunk
    heads = [(c["GRD_ROW_A1"], c["ACT_ROW_X1"] + 256 * 7), (c["GRD_ROW_A2"], c["ACT_ROW_A1"]), (c["GRD_ROW_T1"], c["ACT_ROW_EMB"])]
    heads += [(c["GRD_ROW_T1"] + 128 * l, c["ACT_ROW_T1"] + 128 * (l - 1)) for l in range(1, 4)]
    heads.append((c["GRD_ROW_T5"], c["ACT_ROW_T1"] + 384))
    return trunk + heads


@pytest.mark.parametrize("p_cap", P_CAPS)
def test_segment_offsets_match_the_weight_gradient_plan(header_tables, p_cap):
    jobs = [x for x in header_tables[p_cap] if x[0] == "job"]
    for prec, flag in (("bf16", 1), ("fp32", 0)):
        nt = p_cap // sr.seg_samples(prec)
        for full in (0, 1):
            mine = _plan_rows(full)
            theirs = [[int(v) for v in x[3:]] for x in jobs if int(x[1]) == flag and int(x[2]) == full]
            assert len(theirs) == len(mine), (len(theirs), len(mine))
            for (k, a_off, b_off, a_stride, b_stride, m_rows, n_rows), (grow, arow) in zip(theirs, mine):
                ga, ab = sr.grd_block(grow), sr.act_block(arow)
                assert a_off == sr.segment_offset(ga, grow, 0, nt) and b_off == sr.segment_offset(ab, arow, 0, nt), (prec, full, k)
                # the tile stride: segment (row, tile t) = segment (row, tile 0) + t x stride
                t = nt - 1
                assert a_off + t * a_stride == sr.segment_offset(ga, grow, t, nt) and b_off + t * b_stride == sr.segment_offset(ab, arow, t, nt)
                assert grow + m_rows <= ga[0] + ga[1] and arow + n_rows <= ab[0] + ab[1]


def test_layout_table_order_matches_the_header():
    import re
    hdr = open(os.path.join(REPO, "include", "eonerf_layout.h")).read()
    enums = re.findall(r"enum\s*\{(.*?)\};", hdr, re.S)
    assert len(enums) == 2
    members = [m.lower() for m in re.findall(r"EONERF_PASS_(\w+)", enums[0])]
    assert members == sr.LAYOUT_PASS + ["members"]
    head = [m.lower() for m in re.findall(r"EONERF_LAYOUT_(\w+)", enums[1])]
    assert head[:len(sr.LAYOUT_HEAD)] == sr.LAYOUT_HEAD and head[len(sr.LAYOUT_HEAD):len(sr.LAYOUT_HEAD) + 2] == ["cam", "sun"]
    assert sr.LAYOUT_ENTRIES == 5 + 2 * 22
