"""Surface normals of a trained field (include/eonerf_normals.h): the density gradient in forward mode, composited per ray.

The density-only inference chain carries every sample as four columns -- its value and the three partial derivatives -- through the
shipped packed weights, in the export precisions (fp16x3 with the fp32 retry, or fp32): no autograd, no saved activations, no weight
gradient.  render_normals composites -grad sigma / |grad sigma| with the render's own weights, beside the depth an export render gives
bit for bit.  PyTorch owns the memory and the stream; the arithmetic runs in libeonerf_hip.so.

Not here: march mode (early_stop_eps), bf16 derivative columns, incidence weights for ortho.orthorectify, a train_dp.py flag and any
loss on normals.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import _ptr, _stream
from .datasets.satellite import SatRays, namedtuple_map, satrays_to_table
from .occupancy import OccupancyGrid, grid_on
from .sat_rendering import _zsteps, n_samples_of


@torch.no_grad()
def density_gradient(field, xyz):
    """xyz [..., 3] -> (sigma [..., 1], grad [..., 3] = d sigma / d xyz), in the field's export precision (a bf16 field: its fp16x3
    or fp32 export context; never bf16).  sigma is what field.query_density gives on that context, bit for bit.  Takes no autograd
    and leaves none: for a differentiable gradient use query_density under autograd."""
    shape = xyz.shape[:-1]
    xs = xyz.detach().reshape(-1, 3).float().contiguous()
    n, dev = xs.shape[0], xs.device
    if n == 0:
        return xs.new_empty(*shape, 1), xs.new_empty(*shape, 3)
    L = _lib.lib()
    for _attempt in range(2):
        native, flat = field._native(True, no_bf16=True)
        sigma = torch.empty(n, dtype=torch.float32, device=dev)
        grad = torch.empty(n, 3, dtype=torch.float32, device=dev)
        nb = L.eonerf_density_grad_workspace_bytes(native, n)
        if n and not nb:
            raise ValueError(f"{n} points: more than one call takes; split the batch")
        ws = field._workspace("density_grad", max(nb, 256))
        _lib.check(L.eonerf_field_density_grad(native, _ptr(flat), _ptr(xs), n, _ptr(sigma), _ptr(grad), _ptr(ws), ws.numel(), _stream()))
        if field._export_range_ok():      # (fp16x3 export context: range check over all four columns, once more in fp32 if it fired)
            break
    return sigma.view(*shape, 1), grad.view(*shape, 3)


def _axis_scale(scene_scale):
    """1 / scene_scale as the three fp32 values the library reads: a gradient is a covector, so this puts it into the metric frame."""
    if scene_scale is None:
        return None
    s = torch.as_tensor(scene_scale, dtype=torch.float32).reshape(3).double()
    inv = (1.0 / s).tolist()
    arr = (C.c_float * 3)(*inv)
    for v in arr:
        if v == 0.0 or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"scene_scale={scene_scale!r}: every entry must be finite and non-zero, as must its reciprocal in fp32")
    return arr


@torch.no_grad()
def render_normals(field, occupancy_grid, rays: SatRays, chunk: int = 5120, render_step_size: float = 1e-3, scene_scale=None,
                   noise=None, return_samples=False):
    """Per-ray surface normal of an EXPORT render.  Returns ({"depth": [..., 1] the expected depth, bit-equal to
    render_image(only_depth=True, eval=True); "normal": [..., 3] unit length, 0 where normal_raw is 0; "normal_raw": [..., 3]
    N = -sum w u over the ray's samples (u = the unit density gradient; |N| <= acc, and |N| / acc tells how well the samples agree);
    "acc": [..., 1] sum w}, n_rendering_samples).
    scene_scale: the dataset's three scale factors -- the gradient is multiplied by 1 / scene_scale before it is normalised, which puts
    the normal into the metric east / north / up frame; None leaves the normalised cube's frame.
    Always under no_grad, with the context choice, grid handling, fp16x3 range retry, chunk loop and single host synchronisation of
    sat_rendering.render_depth_quantiles; a field whose export precision is bf16 runs on an fp32 context.
    noise: per chunk (u_cam, u_retry[, ...]) as render_image's.
    return_samples: the dict also carries "samples" = (ray_indices int64 [k], t_starts [k], t_ends [k], sigma [k], grad [k, 3] before
    the scale) of the composited samples, ray indices counted over the whole call."""
    axis = _axis_scale(scene_scale)
    field._context()
    field.set_n_samples(n_samples_of(render_step_size))
    grid = occupancy_grid if isinstance(occupancy_grid, OccupancyGrid) else None
    if grid is not None:
        grid.check_step_size(render_step_size)
    rays_shape = rays.origins.shape
    if len(rays_shape) == 3:
        height, width, _ = rays_shape
        num_rays = height * width
        rays = namedtuple_map(lambda r: r.reshape([num_rays] + list(r.shape[2:])), rays)
    else:
        num_rays, _ = rays_shape
    table, _ = satrays_to_table(rays)
    dev = table.device
    L = _lib.lib()
    for _attempt in range(2):
        native, flat = field._native(True, no_bf16=True)
        ns = field._n_samples
        zs = _zsteps(dev, ns)
        outs, counts, samples = [], [], []
        for k, i in enumerate(range(0, num_rays, chunk)):
            t = table[i:i + chunk]
            n = t.shape[0]
            u_cam = u_retry = None
            if noise is not None:
                u_cam, u_retry = (None if u is None else u.to(dev, torch.float32).contiguous() for u in noise[k][:2])
            nb = L.eonerf_normals_workspace_bytes(native, n)
            if n and not nb:
                raise ValueError(f"chunk={chunk}: more rays than one call takes at {ns} samples per ray")
            ws = field._workspace("normals", max(nb, 256))
            out = torch.empty(n, 5, dtype=torch.float32, device=dev)
            n_samples = torch.zeros(1, dtype=torch.int32, device=dev)
            s = None
            if return_samples:
                cap = max(n * (ns - 1), 1)
                s = (torch.empty(cap, dtype=torch.int64, device=dev),) + tuple(torch.empty(cap, dtype=torch.float32, device=dev) for _ in range(3)) \
                    + (torch.empty(cap, 3, dtype=torch.float32, device=dev),)
            sp = [None] * 5 if s is None else [_ptr(x) for x in s]
            with grid_on(native, grid):
                _lib.check(L.eonerf_render_normals(native, _ptr(flat), _ptr(t), _ptr(zs), _ptr(u_cam), _ptr(u_retry), n, axis, _ptr(out),
                                                   _ptr(n_samples), *sp, _ptr(ws), ws.numel(), _stream()))
            outs.append(out)
            counts.append(n_samples)
            samples.append((i, s))
        out = torch.cat(outs, dim=0) if len(outs) > 1 else outs[0]
        per_chunk = torch.stack(counts).reshape(-1).tolist()     # the only host sync of the call
        n_rendering_samples = int(sum(per_chunk))
        if field._export_range_ok():      # (fp16x3 export context: render_image's retry on its fp32 context)
            break
    lead = tuple(rays_shape[:-1])
    raw = out[:, 1:4]
    length = torch.linalg.vector_norm(raw, dim=1, keepdim=True)
    unit = torch.where(length > 0, raw / length, torch.zeros_like(raw))
    res = {"depth": out[:, 0:1].reshape(*lead, -1), "normal": unit.reshape(*lead, 3), "normal_raw": raw.reshape(*lead, 3),
           "acc": out[:, 4:5].reshape(*lead, -1)}
    if return_samples:
        parts = [[], [], [], [], []]
        for (i, s), kept in zip(samples, per_chunk):
            parts[0].append(s[0][:kept] + i)
            for j in range(1, 5):
                parts[j].append(s[j][:kept])
        res["samples"] = tuple(torch.cat(p, dim=0) for p in parts)
    return res, n_rendering_samples


def slope_aspect(normal):
    """normal [..., 3] in the east / north / up frame -> (slope_deg [...]: the angle between the normal and the vertical, 0 = flat;
    aspect_deg [...]: the compass bearing the surface faces, clockwise from north in [0, 360), NaN where the normal has no horizontal
    part).  A zero normal gives NaN in both."""
    e, n, u = normal[..., 0], normal[..., 1], normal[..., 2]
    length = torch.linalg.vector_norm(normal, dim=-1)
    nan = torch.full_like(length, float("nan"))
    slope = torch.where(length > 0, torch.rad2deg(torch.acos(torch.clamp(u / length, -1.0, 1.0))), nan)
    aspect = torch.rad2deg(torch.atan2(e, n))
    aspect = torch.where(aspect < 0, aspect + 360.0, aspect)
    aspect = torch.where((length > 0) & ((e != 0) | (n != 0)), aspect, nan)
    return slope, aspect


def nadir_normals(field, h, w, scene_scale, sun=(0.0, 0.0), occupancy_grid=None, chunk=5120, render_step_size=None, noise=None):
    """Normal, slope and aspect rasters of the field under the vertical camera of dsm.nadir_rays(h, w): (normal [h, w, 3] unit, metric
    east / north / up, slope_deg [h, w], aspect_deg [h, w]) on the raster ortho.nadir_geotransform(h, w, scene_offset, scene_scale)
    georeferences.  sun: what nadir_rays takes; the normals do not depend on it."""
    from .datasets.satellite import define_satrays_from_tensors
    from .dsm import nadir_rays
    field._context()
    dev = field.flat_params().device
    rays = nadir_rays(h, w, scene_scale, sun[0], sun[1], device=dev)
    ts = torch.zeros(int(h) * int(w), 1, dtype=torch.int64, device=dev)
    if render_step_size is None:       # the step whose int(2 / step) is the field's current sample count
        import math
        render_step_size = 2.0 / field._n_samples
        if int(2 / render_step_size) < field._n_samples:
            render_step_size = math.nextafter(render_step_size, 0.0)
    res, _ = render_normals(field, occupancy_grid, define_satrays_from_tensors(rays, ts), chunk=chunk, render_step_size=render_step_size,
                            scene_scale=scene_scale, noise=noise)
    normal = res["normal"].reshape(int(h), int(w), 3)
    slope, aspect = slope_aspect(normal)
    return normal, slope, aspect
