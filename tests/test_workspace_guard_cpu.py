"""CPU: the checker of the workspace contract test (tests/workspace_guard.py) can fail.  One dirtied guard byte, in front of the payload
or behind it, and one changed output byte are each reported with their offsets; clean buffers pass."""
import pytest
import torch

import workspace_guard as wg


def test_guard_size_follows_the_headers():
    c = wg.header_constants()
    assert c["ACT_ROWS_FULL"] == 2784 and c["GRD_ROWS_FULL"] == 2784 and c["SEG_B"] == 64 and c["PIPE_UNIT_B"] == 16384
    g = wg.guard_bytes()
    assert g == 2784 * 256 * 4 and g % 256 == 0 and g >= wg.MIN_GUARD
    assert g >= c["PIPE_RING"] * c["PIPE_UNIT_B"] and g >= 4 * c["BOTT_SCRATCH_F"] and g >= 4 * c["WGRAD_PART_F"]


def test_layout_of_a_guarded_buffer():
    b = wg.Guarded("out", 84, "cpu", guard=512, fill=0xFF)
    assert b.raw.numel() == 512 + 84 + 512 and b.payload.numel() == 84
    assert b.ptr == b.raw.data_ptr() + 512 and b.payload.data_ptr() == b.ptr
    assert bool((b.raw[:512] == wg.GUARD_FILL).all()) and bool((b.raw[-512:] == wg.GUARD_FILL).all()) and bool((b.payload == 0xFF).all())
    assert torch.isnan(b.view(torch.float32, 1, 21)).all()          # 0xFF bytes: fp32 NaN ...
    assert int(b.fill(0xFF).view(torch.int32, 21)[0]) == -1         # ... and int -1
    assert b.dirty() is None
    wg.check_guards("clean", [b])
    b.view(torch.float32, 21)[:] = 1.0                              # writing the whole payload is no stray write
    wg.check_guards("payload written", [b])


@pytest.mark.parametrize("where,offset", [("rear first byte", 0), ("rear last byte", 511), ("front last byte", -85), ("front first byte", -84 - 512)])
def test_one_dirtied_guard_byte_fails_with_its_offset(where, offset):
    clean, b = wg.Guarded("depth", 4, "cpu", guard=512), wg.Guarded("out", 84, "cpu", guard=512)
    b.raw[512 + 84 + offset] = 0                                    # (index of the byte at `offset` from the payload end)
    assert b.dirty() == (1, offset, offset)
    with pytest.raises(AssertionError) as e:
        wg.check_guards("render_forward R=1", [clean, b])
    msg = str(e.value)
    assert "render_forward R=1" in msg and "out (84 B payload" in msg and "depth" not in msg
    assert f"first at offset {offset:+d}" in msg and f"last at {offset:+d}" in msg


def test_a_dirtied_range_reports_first_and_last():
    b = wg.Guarded("ws", 1024, "cpu", guard=256)
    b.raw[256 + 1024 + 3:256 + 1024 + 67] = 0xFF                    # a 64-byte store that starts 3 bytes past the end
    b.raw[100] = 0                                                  # and one byte in the front guard
    assert b.dirty() == (65, -1024 - 156, 66)


def test_one_changed_output_byte_fails_with_its_offset():
    a = torch.arange(64, dtype=torch.float32).reshape(16, 4)
    b = a.clone()
    wg.assert_same_bits("case", "out", b, a)
    assert wg.first_difference(a, b) is None
    b.view(torch.uint8).reshape(-1)[4 * 37 + 1] ^= 0x10             # one bit of the second byte of element 37
    assert wg.first_difference(b, a) == (4 * 37 + 1, 1)
    with pytest.raises(AssertionError) as e:
        wg.assert_same_bits("field_forward[bf16-n257-F]", "sigma", b, a)
    assert "field_forward[bf16-n257-F]" in str(e.value) and "sigma" in str(e.value) and f"byte offset {4 * 37 + 1}" in str(e.value) and "element 37" in str(e.value)


def test_bit_comparison_sees_what_a_float_comparison_does_not():
    nan1 = torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)
    nan2 = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    wg.assert_same_bits("case", "nan", nan1, nan1.clone())          # the same NaN is the same bits
    with pytest.raises(AssertionError):
        wg.assert_same_bits("case", "nan", nan1, nan2)
    with pytest.raises(AssertionError):
        wg.assert_same_bits("case", "zero", torch.tensor([0.0]), torch.tensor([-0.0]))
