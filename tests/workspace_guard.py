"""Guarded buffers and bit comparisons of the workspace contract test (tests/test_workspace_contract.py).  Plain torch on whatever
device the caller names, so that the checker itself is tested on the CPU (tests/test_workspace_guard_cpu.py): a contract test whose
checker cannot fail is worth nothing."""
import os
import re

import torch

from conftest import REPO

CSRC = os.path.join(REPO, "eonerf_code_amd", "csrc")
GUARD_FILL = 0xA5          # not a poison byte (0x00, 0xFF), not a plausible float / count / offset either
MIN_GUARD = 1 << 20


GUARD_CONSTANTS = ("ACT_ROWS_FULL", "GRD_ROWS_FULL", "SEG_B", "PIPE_RING", "PIPE_UNIT_B", "BOTT_SCRATCH_F", "WGRAD_PART_F", "ENC_PART_F",
                   "WGRAD_MAX_JOBS")


def header_constants():
    """The `constexpr int NAME = <integer expression>;` definitions of the headers the carve is written in, evaluated.  Every constant
    the guard size rests on (GUARD_CONSTANTS) must resolve: a definition this cannot read is an error, not a smaller guard."""
    text = "".join(open(os.path.join(CSRC, h)).read() for h in ("eonerf_common.h", "eonerf_rays.h", "eonerf_kernels.h", "eonerf_carve.h"))
    todo = {m.group(1): m.group(2) for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*([\w\s+\-*/()]+);", text)}
    done, progress = {}, True
    while todo and progress:
        progress = False
        for name, expr in list(todo.items()):
            try:
                done[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(done)))
            except NameError:       # refers to a constant that is not resolved yet (or never: then it stays in todo)
                continue
            del todo[name]
            progress = True
    missing = [n for n in GUARD_CONSTANTS if n not in done]
    if missing:
        raise RuntimeError(f"workspace_guard: cannot evaluate {missing} from the headers in {CSRC}")
    return done


def guard_bytes():
    """Size of one guard.  It has to cover the largest single stride a kernel of these calls takes past the end (or in front of the
    start) of a sub-buffer, so that a store that misses its sub-buffer by one step lands in a guard and not beyond it:

      * every per-sample array is carved for p_cap samples, p_cap a multiple of 256 (p_cap_of, field_p_cap_of): the coarsest step of
        any kernel over the samples is one 256-sample granule.  In the widest slab (saved activations of the full model,
        ACT_ROWS_FULL = 2784 rows -- the gradient slab has as many) one granule is ACT_ROWS_FULL x 256 samples x 4 B (fp32 mode)
        = 2,850,816 B; the same number is 16 sample tiles of [2784 rows][64 B] in fp32 and 8 in bf16;
      * one 256-row block of a slab inside one sample tile (the operand unit of the GEMM and of the pipeline): 256 x SEG_B = 16 KiB;
      * the pipelined backward's rings: one unit is PIPE_UNIT_B = 16 KiB, a whole ring PIPE_RING units = 256 KiB;
      * the per-call scratch blocks: bottleneck factors (BOTT_SCRATCH_F floats = 263 KiB), one deterministic-mode partial
        (WGRAD_PART_F floats = 257 KiB), one encoding partial (ENC_PART_F floats = 129 KiB).

    The guard is the largest of these, not below 1 MiB, rounded up to 256 B (the carve's own alignment)."""
    c = header_constants()
    rows = max(c["ACT_ROWS_FULL"], c["GRD_ROWS_FULL"])
    strides = [rows * 256 * 4, 256 * c["SEG_B"], c["PIPE_RING"] * c["PIPE_UNIT_B"], 4 * c["BOTT_SCRATCH_F"], 4 * c["WGRAD_PART_F"],
               4 * c["ENC_PART_F"], MIN_GUARD]
    return (max(strides) + 255) // 256 * 256


class Guarded:
    """[guard | payload | guard] in ONE uint8 tensor; the payload is exactly `nbytes` long and starts a whole number of 256-byte units
    behind the start of the allocation, i.e. with the alignment the allocator gives."""

    def __init__(self, name, nbytes, device, guard=None, fill=0xFF):
        self.name, self.nbytes = name, int(nbytes)
        self.guard = guard_bytes() if guard is None else int(guard)
        assert self.guard % 256 == 0 and self.guard > 0
        self.raw = torch.empty(2 * self.guard + self.nbytes, dtype=torch.uint8, device=device)
        self.raw[:self.guard] = GUARD_FILL
        self.raw[self.guard + self.nbytes:] = GUARD_FILL
        self.payload = self.raw[self.guard:self.guard + self.nbytes]
        self.payload.fill_(fill)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.guard

    def fill(self, byte):
        self.payload.fill_(byte)
        return self

    def view(self, dtype, *shape):
        """The payload as a tensor of `dtype` (its start is 256-byte aligned; its length must be a whole number of elements)."""
        return self.payload.view(dtype).view(*shape)

    def dirty(self):
        """None, or (number of dirtied guard bytes, first and last dirtied offset RELATIVE TO THE PAYLOAD END: negative offsets below
        -nbytes are in the front guard, offsets >= 0 in the rear one)."""
        front, rear = self.raw[:self.guard], self.raw[self.guard + self.nbytes:]
        bad_f, bad_r = front != GUARD_FILL, rear != GUARD_FILL
        if not bool(bad_f.any()) and not bool(bad_r.any()):
            return None
        offs = torch.cat([torch.nonzero(bad_f).flatten() - self.guard - self.nbytes, torch.nonzero(bad_r).flatten()])
        return int(offs.numel()), int(offs.min()), int(offs.max())


def check_guards(call, buffers):
    """Every guard byte of every buffer still holds its fill; otherwise AssertionError naming the call, the buffer and the offsets."""
    flags = [(b.raw[:b.guard] != GUARD_FILL).any() | (b.raw[b.guard + b.nbytes:] != GUARD_FILL).any() for b in buffers]
    if not flags or not bool(torch.stack(flags).any()):
        return
    msgs = []
    for b in buffers:
        d = b.dirty()
        if d is not None:
            msgs.append(f"{b.name} ({b.nbytes} B payload, {b.guard} B guards): {d[0]} guard byte(s) dirtied, first at offset {d[1]:+d}, "
                        f"last at {d[2]:+d} relative to the payload end")
    raise AssertionError(f"{call}: stray write outside a caller-owned buffer -- " + "; ".join(msgs))


def first_difference(a, b):
    """None if the two tensors hold the same bits, else (byte offset of the first differing byte, number of differing bytes)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    ba, bb = a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)
    ne = ba != bb
    if not bool(ne.any()):
        return None
    return int(torch.nonzero(ne)[0]), int(ne.sum())


def assert_same_bits(call, name, got, want):
    """Bit-for-bit equality (NaN payloads and the sign of zero included)."""
    d = first_difference(got, want)
    if d is not None:
        k = d[0] // got.element_size()
        raise AssertionError(f"{call}: {name} differs from the baseline in {d[1]} byte(s), first at byte offset {d[0]} "
                             f"(element {k}: {got.reshape(-1)[k].item()!r} vs {want.reshape(-1)[k].item()!r})")
