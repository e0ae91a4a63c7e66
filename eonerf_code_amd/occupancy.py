"""Occupancy grid over libeonerf_hip.so (include/eonerf_occ.h): nerfacc's one-level OccGridEstimator over [-1,1]^3, updated on
the device from the field's density and USED by export renders -- render_image, validate_images, evaluate_dsm and render_sun_sweep
skip the samples of empty cells (the reference builds, saves and reloads the same grid but never samples with it,
sat_rendering.py:92-94).

State: `occs` fp32 [r^3] and a bit field `bits` int32 [ceil(r^3 / 32)] (cell c = (ix * r + iy) * r + iz is bit c & 31 of word
c >> 5: the uint32 words of the header, held in torch's int32).  `export_bits` is what renders cull by: `bits` dilated by one cell
(27 neighbours) unless `dilate` is off.  A new grid is all ones -- inert, and what checkpoints have always carried.
"""
import torch

from . import _lib
from ._lib import _ptr, _stream

AABB = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


def n_words(resolution):
    return (int(resolution) ** 3 + 31) // 32


def bits_from_binaries(binaries):
    """bool [1, r, r, r] (or anything with r^3 elements) -> int32 [ceil(r^3 / 32)]; the unused bits of the last word are zero."""
    flat = binaries.reshape(-1).to(torch.int64)
    n = flat.numel()
    pad = (-n) % 32
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    w = (flat.view(-1, 32) << torch.arange(32, dtype=torch.int64, device=flat.device)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def binaries_from_bits(bits, resolution):
    """int32 [ceil(r^3 / 32)] -> bool [1, r, r, r]."""
    r = int(resolution)
    b = (bits.to(torch.int64).unsqueeze(1) >> torch.arange(32, dtype=torch.int64, device=bits.device)) & 1
    return b.reshape(-1)[:r ** 3].view(1, r, r, r).to(torch.bool)


class OccupancyGrid:
    def __init__(self, resolution=128, device="cuda"):
        r = int(resolution)
        if not 1 <= r <= 256:
            raise ValueError(f"OccupancyGrid: resolution {r} outside 1 .. 256")
        self.resolution, self.device = r, torch.device(device)
        self.occs = torch.zeros(r ** 3, dtype=torch.float32, device=self.device)
        self.bits = bits_from_binaries(torch.ones(r ** 3, dtype=torch.bool, device=self.device))
        self.dilate = True
        self.render_step_size = None      # of the last update / build (None: never updated here, e.g. loaded from a checkpoint)
        self.threshold = torch.zeros(1, dtype=torch.float32, device=self.device)      # thr of the last update (device)
        self._export_bits = None
        self._calls = 0                   # the Philox call word of the next update

    # ------------------------------------------------------------------ state
    @property
    def binaries(self):
        """nerfacc's `binaries` buffer: bool [1, r, r, r] of the (undilated) bits."""
        return binaries_from_bits(self.bits, self.resolution)

    @property
    def export_bits(self):
        """The bit field export renders cull by (computed on the device on first use after a change)."""
        if self._export_bits is None:
            if self.dilate:
                out = torch.empty_like(self.bits)
                with torch.cuda.device(self.device):
                    _lib.check(_lib.lib().eonerf_occ_dilate(_ptr(self.bits), _ptr(out), self.resolution, _stream()))
                self._export_bits = out
            else:
                self._export_bits = self.bits
        return self._export_bits

    def state_dict(self):
        """The four persistent buffers of nerfacc v0.5.2's OccGridEstimator (checkpoint.occ_grid_state_dict's format)."""
        r = self.resolution
        return {"resolution": torch.tensor([r, r, r], dtype=torch.int32), "aabbs": torch.tensor([list(AABB)]),
                "occs": self.occs.detach().cpu().clone(), "binaries": self.binaries.cpu()}

    def load_state_dict(self, sd):
        res = [int(x) for x in sd["resolution"].reshape(-1).tolist()]
        if len(set(res)) != 1 or res[0] != self.resolution:
            raise ValueError(f"OccupancyGrid: checkpoint grid {res} against resolution {self.resolution}")
        aabb = sd["aabbs"].reshape(-1, 6)
        if aabb.shape[0] != 1 or not torch.equal(aabb[0].float().cpu(), torch.tensor(AABB)):
            raise ValueError("OccupancyGrid: one level over [-1,1]^3 is supported")
        if sd["occs"].numel() != self.resolution ** 3 or sd["binaries"].numel() != self.resolution ** 3:
            raise ValueError("OccupancyGrid: occs / binaries do not have resolution^3 elements")
        self.occs = sd["occs"].reshape(-1).to(self.device, torch.float32).clone()
        self.bits = bits_from_binaries(sd["binaries"].to(self.device))
        self._export_bits, self.render_step_size = None, None

    # ------------------------------------------------------------------ building
    def update(self, field, render_step_size, decay=0.95, occ_thre=1e-2, jitter=True, return_points=False):
        """One OccGridEstimator update over all cells on the field's own (training) context: one point per cell, jittered inside it,
        occs = max(occs * decay, density * render_step_size), bits = occs > min(mean(occs), occ_thre).  No host synchronisation."""
        if self.device.type != "cuda":
            raise RuntimeError("OccupancyGrid.update runs on an AMD GPU only (no CPU fallback)")
        L = _lib.lib()
        ctx = field._context()
        flat = field._ensure_packed()
        r = self.resolution
        nb = L.eonerf_occ_workspace_bytes(ctx, r)
        ws = field._workspace("occ", nb)
        pts = torch.empty(r ** 3, 3, dtype=torch.float32, device=self.device) if return_points else None
        with torch.cuda.device(self.device):
            _lib.check(L.eonerf_occ_update(ctx, _ptr(flat), _ptr(self.occs), _ptr(self.bits), r, float(render_step_size), float(decay),
                                           float(occ_thre), 1 if jitter else 0, self._calls & 0xFFFFFFFF, _ptr(pts), _ptr(self.threshold),
                                           _ptr(ws), ws.numel(), _stream()))
        self._calls += 1
        self._export_bits, self.render_step_size = None, float(render_step_size)
        return pts

    def update_every_n_steps(self, step, field, render_step_size, n=50, occ_thre=1e-2):
        """train_eonerf.py:112-119: an update every n steps (decay 0.95).  Returns whether one ran."""
        if step % n != 0:
            return False
        self.update(field, render_step_size, decay=0.95, occ_thre=occ_thre)
        return True

    def build(self, field, render_step_size, passes=8, occ_thre=1e-2, dilate=True):
        """The grid of a finished checkpoint: from zero occs, `passes` jittered updates at decay = 1 (the running maximum over the
        passes' points), then -- with dilate -- one cell of margin for the export bits."""
        self.occs.zero_()
        for _ in range(max(1, int(passes))):
            self.update(field, render_step_size, decay=1.0, occ_thre=occ_thre, jitter=True)
        self.dilate = bool(dilate)
        self._export_bits = None
        return self

    # ------------------------------------------------------------------ rendering
    def check_step_size(self, render_step_size):
        """Culling on a grid built for another step size is a silent quality loss: refuse beyond a factor of 2."""
        s = self.render_step_size
        if s is not None and not (0.5 <= float(render_step_size) / s <= 2.0):
            raise ValueError(f"OccupancyGrid: built for render_step_size {s:g}, asked to cull a render at {float(render_step_size):g} "
                             "(more than a factor of 2 apart): rebuild the grid")


class grid_on:
    """`with grid_on(native, grid):` -- the library calls enqueued inside cull by the grid (grid None: nothing happens).  The context
    only borrows the bit field: it is cleared on the way out, and the grid object outlives the calls."""

    def __init__(self, native, grid):
        self.native, self.grid = native, grid

    def __enter__(self):
        if self.grid is not None:
            _lib.check(_lib.lib().eonerf_set_occupancy(self.native, _ptr(self.grid.export_bits), self.grid.resolution))

    def __exit__(self, *exc):
        if self.grid is not None:
            _lib.check(_lib.lib().eonerf_set_occupancy(self.native, None, 0))
        return False
