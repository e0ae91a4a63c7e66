"""Depth priors from an initial DSM on the device (include/eonerf_prior.h): the producing end of the reference's depth supervision.

What the reference does before training with --init_dsm_path / --init_conf_path (SatelliteDataset.load_depth_priors_from_dsm,
datasets/satellite.py:620-709; sat_utils.reproject_dsm_alt_to_satellite_image, sat_utils.py:310-362) as a host loop over the images
-- pyproj, rpcm, a numpy scatter over 4*H*W points per image -- runs here as two kernels per image.  PyTorch owns the memory and the
stream; every arithmetic step runs in libeonerf_hip.so.  The consuming end is FusedTrainer.step(aux_loss=...): depth_loss_L2 below is
metrics.depth_loss_L2 (metrics.py:24-31) in plain PyTorch; no training kernel knows about the prior.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import _ptr, _stream
from .dsm import _raster as _dsm_raster


def _reproject(dsm, values, bounds, rpc_struct, zone, south, out_h, out_w, want_raster, nan_fill, rays, z_offset, z_scale, depth_out=None):
    L = _lib.lib()
    dev = dsm.device
    h, w = dsm.shape
    raster = torch.empty(out_h, out_w, dtype=torch.float32, device=dev) if want_raster else None
    ws = torch.empty(max(4, L.eonerf_prior_workspace_bytes(out_h, out_w)), dtype=torch.uint8, device=dev)
    b = (C.c_double * 4)(*[float(x) for x in bounds])
    with torch.cuda.device(dev):
        _lib.check(L.eonerf_prior_reproject(_ptr(dsm), _ptr(values), h, w, b, C.byref(rpc_struct), int(zone), 1 if south else 0,
                                            int(out_h), int(out_w), _ptr(raster), 1 if nan_fill else 0, _ptr(rays),
                                            int(rays.stride(0)) if rays is not None else 0, float(z_offset), float(z_scale),
                                            _ptr(depth_out), _ptr(ws), ws.numel(), _stream()))
    return raster


def _raster(t, like=None):
    t = _dsm_raster(t)
    if like is not None and t.shape != like.shape:
        raise ValueError("the second raster must have the DSM's size (sat_utils.py:353)")
    return t


def _zone(rpc_struct, zone, south):
    if zone is None:
        from .datasets.satellite import utm_zone_from_lonlat
        return utm_zone_from_lonlat(rpc_struct.lon_offset, rpc_struct.lat_offset)
    return int(zone), bool(south)


def reproject_dsm(dsm, bounds, rpc, out_h, out_w, zone=None, south=None, img_downscale=1.0, values=None):
    """sat_utils.reproject_dsm_alt_to_satellite_image (sat_utils.py:310-362): the DSM [h, w] (fp32, on the GPU; bounds = left, bottom,
    right, top in UTM metres of `zone`) seen from the image of `rpc` (an rpcm-format dict) -> fp32 [out_h, out_w], NaN where no DSM
    point lands.  values: a second raster of the DSM's size to reproject instead of the altitude (other_val_path: the confidence)."""
    from .datasets.satellite import _rpc_struct
    s = _rpc_struct(rpc, img_downscale)
    zone, south = _zone(s, zone, south)
    dsm = _raster(dsm)
    values = _raster(values, dsm) if values is not None else None
    return _reproject(dsm, values, bounds, s, zone, south, int(out_h), int(out_w), True, False, None, 0.0, 1.0)


def depth_priors_from_dsm(dsm, bounds, rpcs, shapes, rays, scene_offset, scene_scale, zone, south, conf=None):
    """SatelliteDataset.load_depth_priors_from_dsm (datasets/satellite.py:620-709) for a whole ray table.
    rays: fp32 [N, >= 6] normalised rays on the GPU whose rows are image-major, row-major pixels, as load_data stacks them
    (:406-481); rpcs: one rpcm-format dict per image, at the table's downscale; shapes: [h, w] per image; scene_offset / scene_scale:
    the dataset's fp32 X/Y/Z values.  conf: a second raster of the DSM's size (the reference's --init_conf_path).
    Returns (prior_depths [N] fp32, prior_confs [N] fp32 or None); -1 marks a ray without a prior.  One reprojection per image yields
    both.  Nothing is read back to the host."""
    from .datasets.satellite import _rpc_struct
    shapes = [(int(h), int(w)) for h, w in (shapes.tolist() if torch.is_tensor(shapes) else shapes)]
    if len(shapes) != len(rpcs):
        raise ValueError("one RPC and one shape per image")
    if rays.dim() != 2 or rays.shape[1] < 6 or rays.dtype != torch.float32 or rays.stride(1) != 1 or not rays.is_cuda:
        raise ValueError("rays must be fp32 [N, >= 6] on the GPU with contiguous rows")
    n = rays.shape[0]
    if sum(h * w for h, w in shapes) != n:
        raise ValueError(f"the images hold {sum(h * w for h, w in shapes)} pixels, the ray table {n} rows")
    dsm = _raster(dsm).to(rays.device)
    conf = _raster(conf, dsm).to(rays.device) if conf is not None else None
    z_offset = float(torch.as_tensor(scene_offset, dtype=torch.float32).reshape(-1)[2])
    z_scale = float(torch.as_tensor(scene_scale, dtype=torch.float32).reshape(-1)[2])
    depths = torch.empty(n, dtype=torch.float32, device=rays.device)
    confs = [] if conf is not None else None
    lo = 0
    for rpc, (h, w) in zip(rpcs, shapes):
        s = _rpc_struct(rpc)
        z, so = _zone(s, zone, south)
        r = _reproject(dsm, conf, bounds, s, z, so, h, w, conf is not None, True, rays[lo:lo + h * w], z_offset, z_scale,
                       depth_out=depths[lo:lo + h * w])
        if conf is not None:
            confs.append(r.reshape(-1))
        lo += h * w
    return depths, (torch.cat(confs) if conf is not None else None)


def depth_loss_L2(gt_depth, pred_depth, gt_conf=None, w=100):
    """metrics.depth_loss_L2 (metrics.py:24-31): w * mean((pred - gt)^2) over the rays with a prior (gt >= 0) and, given confidences,
    gt_conf >= 4.  One deviation: with no such ray in the batch the term is 0 (and so is its gradient), where the reference's mean of
    an empty set is NaN.  The boolean selection synchronises once, as it does in the reference."""
    valid = gt_depth >= 0
    if gt_conf is not None:
        valid = valid & (gt_conf >= 4)
    pred, gt = pred_depth[valid], gt_depth[valid]
    if pred.numel() == 0:
        return (pred_depth * 0).sum()
    return ((pred - gt) ** 2).mean() * w
