"""DSM evaluation on the device (include/eonerf_dsm.h): nadir rays -> depth render -> raster -> NCC registration -> MAE.

What the reference does after render_image on its evaluation path (eval_eonerf.py:78-95,130-249, datasets/satellite.py:545-610,
dsmr.py, sat_utils.py:133-256), without leaving the GPU: no GeoTIFF round trip, no gdal_translate, no host loop.  PyTorch owns the
memory and the stream; every arithmetic step runs in libeonerf_hip.so.  The DSM is rasterised directly on the ground truth's grid
(the roi_txt branch of get_dsm_from_nerf_prediction), so the reference's crop / resample step has nothing left to do.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import _ptr, _stream


def _d3(v):
    """Three doubles holding the dataset's fp32 values (scene.loc_utm is kept as fp32 tensors, datasets/satellite.py:303-307)."""
    t = torch.as_tensor(v, dtype=torch.float32).reshape(3).double().tolist()
    return (C.c_double * 3)(*t)


def _raster(t, dtype=torch.float32):
    if t.dim() != 2 or not t.is_cuda:
        raise ValueError("a raster is a 2-D tensor on the GPU")
    return t.to(dtype).contiguous()


def nadir_rays(h, w, scene_scale, sun_elevation_deg, sun_azimuth_deg, radius=2.0, elevation_deg=0.0, azimuth_deg=0.0, near=None,
               far=None, device="cuda"):
    """create_rays_from_nadir (eval_eonerf.py:78-95): fp32 [h*w, 11] rays of the virtual camera; h, w after int(h // img_downscale).
    sun_elevation_deg is the angle that function receives (the caller passes 90 - the JSON's sun_elevation, :289)."""
    near = max(0.0, radius - 2.0) if near is None else near
    far = near + 2.5 if far is None else far
    dev = torch.device(device)
    rays = torch.empty(int(h) * int(w), 11, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().eonerf_nadir_rays(int(h), int(w), float(radius), float(elevation_deg), float(azimuth_deg), float(near),
                                                float(far), _d3(scene_scale), float(sun_elevation_deg), float(sun_azimuth_deg),
                                                _ptr(rays), _stream()))
    return rays


def grid_from_roi(roi):
    """ROI quadruple (x, y, size, res) of a <aoi>_DSM.txt -> (xoff, yoff, xsize, ysize, res) with yoff the raster's UPPER edge
    (datasets/satellite.py:566-570)."""
    xoff, yoff, size, res = float(roi[0]), float(roi[1]), int(roi[2]), float(roi[3])
    return xoff, yoff + size * res, size, size, res


def rasterize_dsm(rays, depth, scene_offset, scene_scale, roi=None, grid=None, resolution=0.5, accumulators=None, return_grid=False):
    """get_dsm_from_nerf_prediction (datasets/satellite.py:545-610): rays [N,>=6] fp32, depth [N] or [N,1] fp32 -> fp32 [ysize, xsize].
    The grid is `grid` = (xoff, yoff, xsize, ysize, res), or comes from the ROI quadruple, or -- with neither -- from the cloud's
    extent as :572-577 derive it; only that last branch synchronises.  accumulators: an (int64, int32) pair of [ysize*xsize] tensors
    to reuse; they are cleared by the call."""
    if rays.dim() != 2 or rays.shape[1] < 6 or rays.dtype != torch.float32 or rays.stride(1) != 1:
        raise ValueError("rays must be fp32 [N, >= 6] with contiguous rows")
    depth = depth.reshape(-1).to(torch.float32).contiguous()
    if depth.numel() != rays.shape[0]:
        raise ValueError("one depth per ray")
    if grid is None and roi is not None:
        grid = grid_from_roi(roi)
    if grid is None:
        from .datasets.satellite import get_utmalt_from_nerf_prediction
        e, n, _ = get_utmalt_from_nerf_prediction(rays, depth, scene_offset, scene_scale)
        n = torch.where(n < 0, n + 10e6, n)
        keep = (depth >= 0) & torch.isfinite(depth) & torch.isfinite(e) & torch.isfinite(n)     # the rays the rasteriser keeps
        e, n = e[keep], n[keep]
        xmin, xmax, ymin, ymax = torch.stack([e.min(), e.max(), n.min(), n.max()]).tolist()
        import math
        xoff = math.floor(xmin / resolution) * resolution
        yoff = math.ceil(ymax / resolution) * resolution
        grid = (xoff, yoff, int(1 + math.floor((xmax - xoff) / resolution)), int(1 - math.floor((ymin - yoff) / resolution)), resolution)
    xoff, yoff, xsize, ysize, res = grid
    dev = rays.device
    if accumulators is None:
        accumulators = (torch.empty(ysize * xsize, dtype=torch.int64, device=dev), torch.empty(ysize * xsize, dtype=torch.int32, device=dev))
    acc_sum, acc_cnt = accumulators
    if acc_sum.dtype != torch.int64 or acc_cnt.dtype != torch.int32 or min(acc_sum.numel(), acc_cnt.numel()) < ysize * xsize:
        raise ValueError("accumulators: int64 and int32 tensors of ysize * xsize elements")
    dsm = torch.empty(ysize, xsize, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().eonerf_dsm_rasterize(_ptr(rays), int(rays.stride(0)), _ptr(depth), rays.shape[0], _d3(scene_scale),
                                                   _d3(scene_offset), float(xoff), float(yoff), int(xsize), int(ysize), float(res),
                                                   _ptr(acc_sum), _ptr(acc_cnt), _ptr(dsm), _stream()))
    return (dsm, grid) if return_grid else dsm


def mask_water(sec, water):
    """A copy of sec with NaN under the water mask (sat_utils.py:181-185, over the common top-left extent)."""
    out = _raster(sec).clone()
    water = _raster(water, torch.uint8)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().eonerf_dsm_mask_water(_ptr(out), out.shape[0], out.shape[1], _ptr(water), water.shape[0], water.shape[1], _stream()))
    return out


def register_dsm(ref, sec, scaling=False, water=None, return_workspace=False):
    """dsmr.compute_shift(ref, sec, scaling) -> device double[4] = dx, dy, a, b.  water: masks sec first, as the reference does before
    it registers.  return_workspace: also the workspace tensor (register_levels reads the per-level diagnostics from it)."""
    ref = _raster(ref)
    sec = mask_water(sec, water) if water is not None else _raster(sec)
    L = _lib.lib()
    shape = (ref.shape[0], ref.shape[1], sec.shape[0], sec.shape[1])
    ws = torch.empty(L.eonerf_dsm_register_workspace_bytes(*shape), dtype=torch.uint8, device=ref.device)
    out = torch.empty(4, dtype=torch.float64, device=ref.device)
    with torch.cuda.device(ref.device):
        _lib.check(L.eonerf_dsm_register(_ptr(ref), shape[0], shape[1], _ptr(sec), shape[2], shape[3], 1 if scaling else 0, _ptr(out),
                                         _ptr(ws), ws.numel(), _stream()))
    return (out, ws) if return_workspace else out


def register_levels(ws, ref_shape, sec_shape):
    """Per pyramid level (0 = full resolution) what eonerf_dsm_register left in its workspace: {"shift": int32[2], "scores":
    double[121] in scan order, "ref" / "sec": the fp64 level (None for level 0)} as views of `ws`."""
    L = _lib.lib()
    shape = (int(ref_shape[0]), int(ref_shape[1]), int(sec_shape[0]), int(sec_shape[1]))
    out = []
    for level in range(L.eonerf_dsm_register_levels(shape[0], shape[1])):
        dims, offs = (C.c_int * 4)(), (C.c_size_t * 4)()
        _lib.check(L.eonerf_dsm_register_level(*shape, level, dims, offs))

        def view(off, dtype, n, size):
            return ws[off:off + n * size].view(dtype)
        d = {"shift": view(offs[0], torch.int32, 2, 4), "scores": view(offs[1], torch.float64, 121, 8), "ref": None, "sec": None}
        if level:
            d["ref"] = view(offs[2], torch.float64, dims[0] * dims[1], 8).reshape(dims[0], dims[1])
            d["sec"] = view(offs[3], torch.float64, dims[2] * dims[3], 8).reshape(dims[2], dims[3])
        out.append(d)
    return out


def dsm_mae(gt, sec, transform, water=None, return_err=False):
    """The tail of dsm_pointwise_diff (sat_utils.py:198-207) + nanmean(|err|) (:255) -> device double[2] = MAE, n_valid
    (and the fp32 error raster over the common extent).  transform: device double[4] of register_dsm."""
    gt, sec = _raster(gt), _raster(sec)
    water = _raster(water, torch.uint8) if water is not None else None
    transform = transform.to(gt.device, torch.float64).contiguous()
    L = _lib.lib()
    h, w = min(gt.shape[0], sec.shape[0]), min(gt.shape[1], sec.shape[1])
    err = torch.empty(h, w, dtype=torch.float32, device=gt.device) if return_err else None
    ws = torch.empty(L.eonerf_dsm_mae_workspace_bytes(), dtype=torch.uint8, device=gt.device)
    out = torch.empty(2, dtype=torch.float64, device=gt.device)
    wh, ww = (water.shape if water is not None else (0, 0))
    with torch.cuda.device(gt.device):
        _lib.check(L.eonerf_dsm_mae(_ptr(gt), gt.shape[0], gt.shape[1], _ptr(sec), sec.shape[0], sec.shape[1], _ptr(water), wh, ww,
                                    _ptr(transform), _ptr(out), _ptr(err), _ptr(ws), ws.numel(), _stream()))
    return (out, err) if return_err else out


def evaluate_dsm(field, gt, roi, scene_offset, scene_scale, sun, chunk=5120, render_step_size=None, water=None, scaling=False,
                 h=None, w=None, noise=None, return_all=False, occupancy_grid=None, early_stop_eps=0.0, march_block=32, depth_quantile=None):
    """Validation DSM MAE of a field against a lidar DSM, as train_eonerf.py:197-282 / eval_eonerf.py:286-324 obtain it:
    nadir rays (h x w, default the GT's size) -> render_image(only_depth=True) in the field's export precision -> raster on the GT's
    grid (roi = x, y, size, res) -> water mask -> registration -> MAE.
    sun = (elevation_deg, azimuth_deg) as create_rays_from_nadir receives them.  Returns device tensors: double[2] = MAE, n_valid
    (return_all: a dict with the rays, depth, dsm, transform and error raster as well).  Nothing here reads a result back: the only
    host synchronisation is render_image's own sample count, and the caller's read of the MAE.
    occupancy_grid, early_stop_eps, march_block: handed to render_image.
    depth_quantile: None, or a quantile q in (0, 1): the raster is made from the depth at which the rays' accumulated opacity crosses q
    (0.5: the median surface; sat_rendering.render_depth_quantiles, include/eonerf_quantile.h) instead of the expected depth; with
    return_all the dict then also carries "depth_expected" and "od_front"."""
    from .datasets.satellite import define_satrays_from_tensors
    from .sat_rendering import render_depth_quantiles, render_image
    gt = _raster(gt)
    h, w = int(h or gt.shape[0]), int(w or gt.shape[1])
    rays = nadir_rays(h, w, scene_scale, sun[0], sun[1], device=gt.device)
    ts = torch.zeros(h * w, 1, dtype=torch.int64, device=gt.device)
    if render_step_size is None:       # the step whose int(2 / step) is the field's current sample count
        import math
        render_step_size = 2.0 / field._n_samples
        if int(2 / render_step_size) < field._n_samples:
            render_step_size = math.nextafter(render_step_size, 0.0)
    if depth_quantile is not None:
        res, _ = render_depth_quantiles(field, occupancy_grid, define_satrays_from_tensors(rays, ts), quantiles=(depth_quantile,), chunk=chunk,
                                        render_step_size=render_step_size, noise=noise, early_stop_eps=early_stop_eps, march_block=march_block)
        depth = res["depth_q"].reshape(-1)
    else:
        with torch.no_grad():
            res, _ = render_image(field, occupancy_grid, define_satrays_from_tensors(rays, ts), None, None, epoch_idx=None, chunk=chunk,
                                  render_step_size=render_step_size, only_depth=True, eval=True, noise=noise,
                                  early_stop_eps=early_stop_eps, march_block=march_block)
        depth = res["depth"].reshape(-1)
    dsm = rasterize_dsm(rays, depth, scene_offset, scene_scale, roi=roi)
    if water is not None:
        dsm = mask_water(dsm, water)
    transform = register_dsm(gt, dsm, scaling=scaling)
    out = dsm_mae(gt, dsm, transform, return_err=return_all)
    if not return_all:
        return out
    all_ = {"mae": out[0], "err": out[1], "rays": rays, "depth": depth, "dsm": dsm, "transform": transform}
    if depth_quantile is not None:
        all_["depth_expected"], all_["od_front"] = res["depth"].reshape(-1), res["od_front"].reshape(-1)
    return all_
