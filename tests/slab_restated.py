"""The layout INSIDE a training slab, restated in plain torch (device-agnostic): raw workspace bytes -> dense tensors and back.

WHERE a slab starts inside the workspace is not restated here: that is the library's bump allocator (csrc/eonerf_carve.h), asked through
eonerf_workspace_layout (include/eonerf_layout.h).  What is restated is DESIGN.md section 2 and the three places of the sources that define it:

  * feature-major blocks (csrc/eonerf_common.h "Saved-activation / saved-gradient slabs", wgrad_plan's seg0): a slab is
    [row block][sample tile][row in block][64 B]; segment (row, tile t) of block [s, s + r) lies at byte (s * NT + t * r + (row - s)) * 64
    from the slab's start, NT = p_cap / samples per segment; a segment holds 32 bf16 or 16 fp32 samples;
  * unit-order tiles (csrc/eonerf_mlp_bwd.hip PIPE 1, csrc/eonerf_bwd_pipe.hip, csrc/eonerf_enc_pair.hip): a 256-feature tensor as
    [step of 32 samples][k-group 16][lane 64][16 B] bf16 -- the B operand of v_mfma_f32_32x32x16_bf16: lane = 32 * h + sample, its 8
    elements e are features 16 * kg + 8 * (e >> 2) + 4 * h + (e & 3) (PBf16::feat);
  * the row tables ActMap / GrdMap (csrc/eonerf_kernels.h) and the encoding slot -> reference column map (enc_col_of_hq,
    csrc/eonerf_common.h; slot order: csrc/eonerf_pack.cpp slot_to_kghe).

Constants come from the headers through workspace_guard.header_constants(); tests/test_slab_restated_cpu.py holds the tables and a set of
segment offsets to a stand-alone program that includes the headers themselves."""
import functools

import torch

import workspace_guard as wg


@functools.lru_cache(maxsize=None)
def K():
    """The headers' layout constants (ACT_ROW_*, GRD_ROW_*, SEG_B, ENC_SLOTS, PIPE_UNIT_B, ...)."""
    c = wg.header_constants()
    for name in ("ACT_ROW_ENC", "ACT_ROW_X1", "ACT_ROW_A1", "ACT_ROW_T1", "ACT_ROW_EMB", "ACT_ROWS_FULL", "ACT_ROWS_DENSITY", "GRD_ROW_Y0",
                 "GRD_ROW_SIG", "GRD_ROW_A2", "GRD_ROW_A1", "GRD_ROW_T1", "GRD_ROW_T5", "GRD_ROWS_FULL", "GRD_ROWS_DENSITY", "SEG_B",
                 "ENC_SLOTS", "PIPE_UNIT_B", "PIPE_TS"):
        if name not in c:
            raise RuntimeError(f"slab_restated: {name} not found in the headers")
    return c


def act_dtype(precision):
    return {"bf16": torch.bfloat16, "fp32": torch.float32}[precision]


def seg_samples(precision):
    """Samples of one 64-byte segment."""
    return K()["SEG_B"] // torch.empty(0, dtype=act_dtype(precision)).element_size()


# ------------------------------------------------------------------------------------------------------------ row tables
def act_block(row):
    """ActMap::block: (first row, rows) of the block of a row of the activation slab."""
    c = K()
    if row < c["ACT_ROW_X1"]:
        return c["ACT_ROW_ENC"], 64
    if row < c["ACT_ROW_A1"]:
        return c["ACT_ROW_X1"] + (row - c["ACT_ROW_X1"]) // 256 * 256, 256
    if row < c["ACT_ROW_EMB"]:
        return c["ACT_ROW_A1"] + (row - c["ACT_ROW_A1"]) // 128 * 128, 128
    return c["ACT_ROW_EMB"], 32


def grd_block(row):
    """GrdMap::block."""
    c = K()
    if row < c["GRD_ROW_SIG"]:
        return row // 256 * 256, 256
    if row < c["GRD_ROW_A2"]:
        return c["GRD_ROW_SIG"], 32
    if row < c["GRD_ROW_A1"]:
        return c["GRD_ROW_A2"], 32
    if row < c["GRD_ROW_T1"] + 128:
        return c["GRD_ROW_A1"], 256
    if row < c["GRD_ROW_T5"]:
        return c["GRD_ROW_T1"] + (row - c["GRD_ROW_T1"]) // 128 * 128, 128
    return c["GRD_ROW_T5"], 32


def segment_offset(block, row, tile, n_tiles):
    """Byte offset, from the slab's start, of segment (row, sample tile) of block = (s, r)."""
    s, r = block
    assert s <= row < s + r and 0 <= tile < n_tiles
    return (s * n_tiles + tile * r + (row - s)) * K()["SEG_B"]


def enc_col_of_hq(h, q):
    """Reference encoding column (radiance_fields/mlp.py:190-208: [x, y, z, sin 30, cos 30]) of slot q of lane half h; -1 = the pad slot."""
    if q < 30:
        return 33 + q if h else 3 + q
    if q == 30:
        return 2 if h else 0
    return -1 if h else 1


def enc_hq_of_row(precision, row):
    """(h, q) of encoding row `row` of the activation slab: the forward stores slot q = kg * NE + e of half h at row P::feat(kg, h, e)."""
    if precision == "bf16":
        kg, rem = divmod(row, 16)
        return (rem % 8) // 4, kg * 8 + (rem // 8) * 4 + rem % 4
    kg, rem = divmod(row, 8)
    return rem // 4, kg * 4 + rem % 4


def enc_col_of_row(precision):
    """[64] reference column of every encoding row (-1: pad)."""
    return [enc_col_of_hq(*enc_hq_of_row(precision, r)) for r in range(K()["ENC_SLOTS"])]


# ------------------------------------------------------------------------------------------------------------ feature-major blocks
def _block_view(ws, slab_off, block_start, block_rows, n_tiles, precision):
    ts = seg_samples(precision)
    lo = slab_off + block_start * n_tiles * K()["SEG_B"]
    nbytes = n_tiles * block_rows * K()["SEG_B"]
    assert ws.dtype == torch.uint8 and ws.dim() == 1 and lo + nbytes <= ws.numel(), (lo, nbytes, ws.numel())
    return ws[lo:lo + nbytes].view(act_dtype(precision)).view(n_tiles, block_rows, ts)


def decode_block(ws, slab_off, block_start, block_rows, n_tiles, precision):
    """[block_rows, p_cap] (p_cap = n_tiles x samples per segment) of block [block_start, block_start + block_rows) of the slab at slab_off."""
    v = _block_view(ws, slab_off, block_start, block_rows, n_tiles, precision)
    return v.permute(1, 0, 2).reshape(block_rows, -1)


def encode_block(ws, slab_off, block_start, block_rows, n_tiles, precision, dense):
    """Inverse of decode_block: writes dense [block_rows, p_cap] (rounded to the slab's type) into the workspace."""
    v = _block_view(ws, slab_off, block_start, block_rows, n_tiles, precision)
    v.copy_(dense.to(act_dtype(precision)).reshape(block_rows, n_tiles, -1).permute(1, 0, 2))


# ------------------------------------------------------------------------------------------------------------ unit-order tiles (bf16)
@functools.lru_cache(maxsize=None)
def _unit_feature_index():
    """[kg 16][h 2][e 8] -> feature (PBf16::feat)."""
    kg = torch.arange(16).view(16, 1, 1)
    h = torch.arange(2).view(1, 2, 1)
    e = torch.arange(8).view(1, 1, 8)
    return (16 * kg + 8 * (e >> 2) + 4 * h + (e & 3)).expand(16, 2, 8).contiguous()


def _units_view(ws, off, n_steps):
    nbytes = n_steps * K()["PIPE_UNIT_B"]
    assert ws.dtype == torch.uint8 and off + nbytes <= ws.numel(), (off, nbytes, ws.numel())
    return ws[off:off + nbytes].view(torch.bfloat16).view(n_steps, 16, 2, 32, 8)      # [step][kg][h][sample][e]


def decode_units(ws, off, n_steps):
    """[256, n_steps * 32] bf16 of a 256-feature tensor in unit order at byte `off`."""
    v = _units_view(ws, off, n_steps).permute(1, 2, 4, 0, 3).reshape(256, n_steps * 32)      # rows in (kg, h, e) order
    out = torch.empty_like(v)
    out[_unit_feature_index().reshape(-1).to(v.device)] = v
    return out


def encode_units(ws, off, n_steps, dense):
    v = _units_view(ws, off, n_steps)
    src = dense.to(torch.bfloat16)[_unit_feature_index().reshape(-1).to(dense.device)]      # (kg, h, e) order
    v.copy_(src.reshape(16, 2, 8, n_steps, 32).permute(3, 0, 1, 4, 2))


def decode_unit_block(ws, slab_off, block_start, n_tiles):
    """A 256-row block of the gradient slab whose 16-KiB tiles are in unit order (dY_0 / dY_5 on the pipelined path): the tiles lie where
    the feature-major ones would."""
    return decode_units(ws, slab_off + block_start * n_tiles * K()["SEG_B"], n_tiles)


# ------------------------------------------------------------------------------------------------------------ per-sample arrays
def soa(ws, off, rows, p_cap, dtype=torch.float32):
    """[rows, p_cap] view of a per-sample array (fp32 / int32) at byte `off`."""
    return ws[off:off + rows * p_cap * 4].view(dtype).view(rows, p_cap)


# ------------------------------------------------------------------------------------------------------------ eonerf_workspace_layout
# the fixed order of include/eonerf_layout.h (held to the header's enums by tests/test_slab_restated_cpu.py)
LAYOUT_HEAD = ["p_cap", "bytes", "m_bott", "dy_in", "enc_part"]
LAYOUT_PASS = ["counts", "offsets", "n_pts", "px", "py", "pz", "tmid", "delta", "sigma", "albedo", "ts", "tb", "simg", "act", "grd", "masks",
               "g_sigma", "g_albedo", "g_ts", "g_tb", "g_emb", "g_pos"]
LAYOUT_ENTRIES = len(LAYOUT_HEAD) + 2 * len(LAYOUT_PASS)
LAYOUT_NONE = (1 << 64) - 1


def layout_dict(table):
    """The table eonerf_workspace_layout filled -> (head dict, camera pass dict, sun pass dict); a missing buffer is absent."""
    table = [int(v) for v in table]
    assert len(table) == LAYOUT_ENTRIES
    n_head, n_pass = len(LAYOUT_HEAD), len(LAYOUT_PASS)
    pick = lambda names, vals: {k: v for k, v in zip(names, vals) if v != LAYOUT_NONE}      # noqa: E731
    return (pick(LAYOUT_HEAD, table[:n_head]), pick(LAYOUT_PASS, table[n_head:n_head + n_pass]), pick(LAYOUT_PASS, table[n_head + n_pass:]))
