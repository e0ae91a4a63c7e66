"""Camera offset refinement (include/eonerf_pose.h): a learned 3-D offset per image, added to that image's ray origins -- the
reference's --rpc_correction (opt.py:80).

apply_origin_offsets is the ONE definition of "corrected rays": render_image(origin_offsets=...), FusedTrainer(origin_offsets=True)
and train_dp.py's validation all render the table it returns.  origin_grad binds eonerf_render_origin_grad: d loss / d ray origin of
the training step whose backward has just run, and its per-image sum.  Only the origins are differentiated: view direction, near / far
and the sun direction are not."""
import torch

from . import _lib
from ._lib import _ptr, _stream


def apply_origin_offsets(rays, img_idx, offsets):
    """rays [n, 11] fp32 (origin3, dir3, near, far, sun3), img_idx [n] int64, offsets [n_images, 3] fp32 -> a NEW contiguous [n, 11]
    table whose origin columns are rays[:, :3] + offsets[img_idx]: one fp32 add per component; every other column is copied."""
    if rays.dim() != 2 or rays.shape[1] != 11:
        raise ValueError("rays must be an [n, 11] table")
    if offsets.dim() != 2 or offsets.shape[1] != 3:
        raise ValueError("offsets must be an [n_images, 3] table")
    out = rays.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
    q = offsets.detach().to(device=out.device, dtype=torch.float32)
    out[:, 0:3] = rays.detach()[:, 0:3].to(torch.float32) + q.index_select(0, img_idx.reshape(-1).to(out.device))
    return out


def max_offset(offsets):
    """Largest row norm of an offset table, in scene units (a device scalar: the status line of train_dp.py reads it)."""
    return offsets.detach().float().norm(dim=1).max()


def origin_grad(native, flat, table, img, flags, ws, n_images=None, d_offsets=None, want_origins=False):
    """Directly behind eonerf_render_backward / _backward_loss on (native, flat, table, img, flags, ws), same stream: returns
    (d_origins [n, 3] or None, d_offsets).  d_offsets [n_images, 3] is ACCUMULATED into when given, created from zeros when n_images is
    given, None otherwise.  The library refuses (RuntimeError, call sequence error) when anything used the context's workspaces since."""
    L = _lib.lib()
    n, dev = table.shape[0], table.device
    if d_offsets is None and n_images is not None:
        d_offsets = torch.zeros(n_images, 3, dtype=torch.float32, device=dev)
    d_origins = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_origins else None
    nb = L.eonerf_origin_grad_scratch_bytes(native, n, flags)
    scratch = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    _lib.check(L.eonerf_render_origin_grad(native, _ptr(flat), _ptr(table), _ptr(img), n, flags, _ptr(ws), ws.numel(),
                                           _ptr(scratch), nb, _ptr(d_origins), _ptr(d_offsets), _stream()))
    return d_origins, d_offsets
