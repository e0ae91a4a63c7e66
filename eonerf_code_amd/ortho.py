"""True orthophoto on the device (include/eonerf_ortho.h): the input images themselves resampled onto the reconstructed surface
through their own RPCs, occluded cells left out, fused into one mosaic on the grid of a nadir render.

The nadir render's albedo is the field's opinion of the ground; the orthophoto is the data on the ground.  The chain is
surface point (ray + depth) -> UTM -> lon / lat (inverse Krueger series) -> each image's RPC -> bilinear gather -> mean or median
over the images that see the point -- the reference's get_lonlatalt_from_nerf_prediction (datasets/satellite.py:535-543) and
rpc_projection_differentiable (sat_utils.py:420-432), which it carries and never calls.  Whether image j sees a surface point is
asked of the field itself: a camera's view direction points from the satellite to the ground as sundirs points from the sun to the
ground, so the sun sweep (relight.render_sun_sweep) with the K view directions as its suns returns every point's transmittance
towards every satellite -- one camera pass and K shadow passes, no new rendering code.

PyTorch owns the memory and the stream; every arithmetic step runs in libeonerf_hip.so.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import _ptr, _stream

MAX_MEDIAN = 64      # EONERF_ORTHO_MAX_MEDIAN
_MODES = {"mean": 0, "median": 1}


def _f3(v):
    """Three floats holding the dataset's fp32 values (scene.loc_utm is kept as fp32 tensors, datasets/satellite.py:303-307)."""
    return (C.c_float * 3)(*torch.as_tensor(v, dtype=torch.float32).reshape(3).tolist())


def _ray_table(rays):
    if rays.dim() != 2 or rays.shape[1] < 6 or rays.dtype != torch.float32 or rays.stride(1) != 1 or not rays.is_cuda:
        raise ValueError("rays must be fp32 [n, >= 6] on the GPU with contiguous rows")
    return rays


def ground_points(rays, depth, scene_offset, scene_scale, zone, south):
    """Surface points of a render: rays [n, >= 6] fp32 normalised, depth [n] or [n, 1] -> fp64 [n, 3] = lon, lat (degrees), alt (m).
    get_lonlatalt_from_nerf_prediction in fp64; a non-finite depth gives three NaNs."""
    rays = _ray_table(rays)
    depth = depth.reshape(-1).to(rays.device, torch.float32).contiguous()
    if depth.numel() != rays.shape[0]:
        raise ValueError("one depth per ray")
    out = torch.empty(rays.shape[0], 3, dtype=torch.float64, device=rays.device)
    with torch.cuda.device(rays.device):
        _lib.check(_lib.lib().eonerf_ortho_ground(_ptr(rays), int(rays.stride(0)), _ptr(depth), rays.shape[0], _f3(scene_scale),
                                                  _f3(scene_offset), int(zone), 1 if south else 0, _ptr(out), _stream()))
    return out


def _points(lonlatalt):
    if lonlatalt.dim() != 2 or lonlatalt.shape[1] != 3 or not lonlatalt.is_cuda:
        raise ValueError("lonlatalt must be [n, 3] on the GPU")
    return lonlatalt.to(torch.float64).contiguous()


def _gather(lla, rpc_struct, pixels, gain, bias, visibility, min_visibility, layer, weight, colrow):
    h, w, c = (pixels.shape if pixels is not None else (1, 1, 1))
    g = (C.c_float * c)(*gain) if gain is not None else None
    b = (C.c_float * c)(*bias) if bias is not None else None
    with torch.cuda.device(lla.device):
        _lib.check(_lib.lib().eonerf_ortho_gather(_ptr(lla), lla.shape[0], C.byref(rpc_struct), _ptr(pixels), int(h), int(w), int(c), g, b,
                                                  _ptr(visibility), float(min_visibility), _ptr(layer), _ptr(weight), _ptr(colrow), _stream()))


def project_points(lonlatalt, rpc, img_downscale=1.0):
    """sat_utils.rpc_projection_differentiable on device points: lonlatalt fp64 [n, 3] (ground_points) and an rpcm-format dict ->
    fp64 [n, 2] = col, row in the image, inside it or not.  The integer coordinate (c, r) is pixel [r, c]."""
    from .datasets.satellite import _rpc_struct
    lla = _points(lonlatalt)
    out = torch.empty(lla.shape[0], 2, dtype=torch.float64, device=lla.device)
    _gather(lla, _rpc_struct(rpc, img_downscale), None, None, None, None, 0.0, None, None, out)
    return out


def view_directions(rpcs, shapes, min_alt, max_alt, scene_offset, scene_scale, zone, south, device="cuda"):
    """fp32 [K, 3]: per image the normalised ray direction of its centre pixel ((w - 1) / 2, (h - 1) / 2), from the satellite to the
    ground, through generate_rays -- the vector the sun sweep takes in place of a sun direction to ask for the visibility from that
    satellite.  ONE direction per image is an approximation: across a 256 m scene a 600 km orbit changes it by about 0.02 degrees,
    far below what moves a shadow edge by a cell."""
    from .datasets.satellite import generate_rays
    shapes = [(int(h), int(w)) for h, w in (shapes.tolist() if torch.is_tensor(shapes) else shapes)]
    if len(shapes) != len(rpcs):
        raise ValueError("one RPC and one shape per image")
    off = torch.as_tensor(scene_offset, dtype=torch.float32).reshape(3).tolist()
    sc = torch.as_tensor(scene_scale, dtype=torch.float32).reshape(3).tolist()
    rows = [generate_rays(rpc, min_alt, max_alt, cols=[(w - 1) / 2.0], rows=[(h - 1) / 2.0], scene_offset=off, scene_scale=sc,
                          zone=int(zone), south=bool(south), device=device)[0, 3:6] for rpc, (h, w) in zip(rpcs, shapes)]
    return torch.stack(rows).contiguous()


def _step_size(field, render_step_size):
    if render_step_size is not None:
        return render_step_size
    import math
    step = 2.0 / field._n_samples           # the step whose int(2 / step) is the field's current sample count
    return math.nextafter(step, 0.0) if int(2 / step) < field._n_samples else step


def surface_visibility(field, rays, view_dirs, chunk=5120, render_step_size=None, occupancy_grid=None, noise=None):
    """(depth [n], visibility [K, n]) of the ray table `rays` [n, 11]: the rendered depth and, per view direction, the transmittance
    from the surface point towards that satellite -- geo_shadows of one render_sun_sweep call with suns=view_dirs, an export render."""
    from .datasets.satellite import define_satrays_from_tensors
    from .relight import render_sun_sweep
    ts = torch.zeros(rays.shape[0], 1, dtype=torch.int64, device=rays.device)
    res, _ = render_sun_sweep(field, define_satrays_from_tensors(rays, ts), view_dirs, chunk=chunk,
                              render_step_size=_step_size(field, render_step_size), eval=True, keys=("depth", "geo_shadows"), noise=noise,
                              occupancy_grid=occupancy_grid)
    return res["depth"].reshape(-1), res["geo_shadows"].reshape(res["geo_shadows"].shape[0], -1)


def nadir_geotransform(h, w, scene_offset, scene_scale, radius=2.0):
    """(xoff, yoff, res_x, res_y) in UTM metres of the raster dsm.nadir_rays(h, w) spans (its default vertical camera): the rays of
    eval_eonerf.py:196-200 are a regular grid in normalised x, y -- x_i = (i - w / 2) / (w / radius), y_j = -(j - h / 2) / (h / radius).
    Pixel-is-area, north up: cell [j, i] of the mosaic is centred on its ray, at east = xoff + (i + 0.5) * res_x and
    north = yoff - (j + 0.5) * res_y; (xoff, yoff) is the upper left corner of cell [0, 0]."""
    off = torch.as_tensor(scene_offset, dtype=torch.float32).reshape(3).double().tolist()
    sc = torch.as_tensor(scene_scale, dtype=torch.float32).reshape(3).double().tolist()
    res_x, res_y = radius / int(w) * sc[0], radius / int(h) * sc[1]
    return off[0] - 0.5 * radius * sc[0] - 0.5 * res_x, off[1] + 0.5 * radius * sc[1] + 0.5 * res_y, res_x, res_y


def fuse_layers(layers, weights, fuse="median"):
    """K layers [K, n, C] and weights [K, n] (fp32, on the GPU) -> (mosaic [n, C] fp32, weight [n] fp32, count [n] int32).
    "mean": the weighted mean, summed in fp64 in ascending image order; "median": per channel, unweighted, over the images with a
    positive weight (at most 64 images) -- the mode that keeps one image's cars and clouds out of the mosaic."""
    if fuse not in _MODES:
        raise ValueError("fuse must be 'mean' or 'median'")
    K, n, c = layers.shape
    if fuse == "median" and K > MAX_MEDIAN:
        raise ValueError(f"fuse='median' takes at most {MAX_MEDIAN} images ({K} given): use fuse='mean', or fuse subsets")
    layers, weights = layers.to(torch.float32).contiguous(), weights.to(torch.float32).contiguous()
    dev = layers.device
    mosaic = torch.empty(n, c, dtype=torch.float32, device=dev)
    wsum = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().eonerf_ortho_fuse(_ptr(layers), _ptr(weights), int(K), int(n), int(c), _MODES[fuse], _ptr(mosaic), _ptr(wsum),
                                                _ptr(count), _stream()))
    return mosaic, wsum, count


def orthorectify(field, images, rpcs, scene_offset, scene_scale, zone, south, h, w, min_alt, max_alt, rays=None, fuse="median",
                 min_visibility=0.2, radiometric=True, depth=None, visibility=None, occupancy_grid=None, chunk=5120,
                 render_step_size=None, noise=None, return_all=False, image_indices=None):
    """True orthophoto: images (K tensors [h_k, w_k, C], fp32, NaN = no data) and their rpcm-format RPCs (at the images' downscale)
    -> {"mosaic": [h, w, C], "weight": [h, w] (sum of the weights), "count": [h, w] int32
    (images that see the cell)}; a cell no image sees is NaN.  nadir_geotransform(h, w, ...) georeferences the result.

    rays: the [n = h * w, 11] table the surface is rendered along; default dsm.nadir_rays(h, w).  Any table works: with image i's own
      rays the result is image j warped into image i's geometry.
    depth [n] / visibility [K, n]: given in place of a render.  With neither, ONE sun sweep (surface_visibility) renders the depth and,
      with the images' view directions (view_directions, from min_alt / max_alt) as its suns, each point's transmittance towards each
      satellite; with a depth alone the visibility is still rendered unless field is None -- then the call is a plain DSM-driven
      orthorectification without an occlusion test (the depth could come from a lidar DSM).
    min_visibility: a point counts as seen by an image from this transmittance on, and is weighted by it; 0.2 is the reference's own
      line between lit and shadowed (geo_shadows > 0.2, metrics.py:40).
    radiometric: undo each image's gain A and bias b of rgb_j = clip(A * rgb + b) (sat_rendering.py:288-306), (v - b) / A, with
      field.radiometricT_enc.weight[j, :6], so that all images are fused on the field's common radiometry; needs 3 channels and
      len(images) == the field's image count, or image_indices=; False (or a field without the embedding): the identity.
    fuse: "median" (at most 64 images) or "mean", see fuse_layers.
    return_all: the dict also holds depth, visibility [K, n], layers [K, n, C], weights [K, n], colrow [K, n, 2], lonlatalt [n, 3].
    No result is read back: the only host synchronisation is the sweep's own sample count, and one copy of the K x 6 radiometric
    parameters (the library validates gains on the host)."""
    from .datasets.satellite import _rpc_struct
    K = len(images)
    if K < 1 or len(rpcs) != K:
        raise ValueError("one RPC per image, at least one image")
    if fuse not in _MODES:
        raise ValueError("fuse must be 'mean' or 'median'")
    if fuse == "median" and K > MAX_MEDIAN:
        raise ValueError(f"fuse='median' takes at most {MAX_MEDIAN} images ({K} given): use fuse='mean', or fuse subsets")
    h, w = int(h), int(w)
    if rays is not None:
        dev = rays.device
    elif field is not None:
        dev = next(field.parameters()).device
    elif depth is not None and depth.is_cuda:
        dev = depth.device
    else:
        dev = torch.device("cuda")
    images = [im.to(dev, torch.float32).contiguous() for im in images]
    c = images[0].shape[2] if images[0].dim() == 3 else 0
    if any(im.dim() != 3 or im.shape[2] != c for im in images) or not 1 <= c <= 4:
        raise ValueError("images are [h, w, C] tensors with the same 1 <= C <= 4")
    if rays is None:
        from .dsm import nadir_rays
        rays = nadir_rays(h, w, scene_scale, 0.0, 0.0, device=dev)
    rays = _ray_table(rays)
    n = rays.shape[0]
    if n != h * w:
        raise ValueError(f"the ray table has {n} rows, the mosaic {h} x {w} cells")
    gains, biases = [[1.0] * c] * K, [[0.0] * c] * K
    if radiometric and field is not None and getattr(field, "radiometric_normalization", False):
        idx = list(range(K)) if image_indices is None else [int(j) for j in image_indices]
        if len(idx) != K or (image_indices is None and K != field.n_input_images):
            raise ValueError(f"radiometric=True: {K} images against the field's {field.n_input_images}: pass image_indices= (or radiometric=False)")
        if c != 3:
            raise ValueError("radiometric=True needs 3-channel images (the field's gain and bias are RGB)")
        ab = field.radiometricT_enc.weight.detach()[torch.as_tensor(idx, device=field.radiometricT_enc.weight.device), :6].double().cpu().tolist()
        gains, biases = [row[:3] for row in ab], [row[3:6] for row in ab]
    if depth is not None:
        depth = depth.reshape(-1).to(dev, torch.float32).contiguous()
    if visibility is not None:
        visibility = visibility.to(dev, torch.float32).reshape(K, n).contiguous()
    if field is not None and (depth is None or visibility is None):
        dirs = view_directions(rpcs, [im.shape[:2] for im in images], min_alt, max_alt, scene_offset, scene_scale, zone, south, device=dev)
        d, v = surface_visibility(field, rays, dirs, chunk=chunk, render_step_size=render_step_size, occupancy_grid=occupancy_grid, noise=noise)
        depth = d if depth is None else depth
        visibility = v.contiguous() if visibility is None else visibility
    if depth is None:
        raise ValueError("without a field a depth must be given")
    lla = ground_points(rays, depth, scene_offset, scene_scale, zone, south)
    layers = torch.empty(K, n, c, dtype=torch.float32, device=dev)
    weights = torch.empty(K, n, dtype=torch.float32, device=dev)
    colrow = torch.empty(K, n, 2, dtype=torch.float64, device=dev) if return_all else None
    for k in range(K):
        _gather(lla, _rpc_struct(rpcs[k]), images[k], gains[k], biases[k], None if visibility is None else visibility[k],
                min_visibility, layers[k], weights[k], None if colrow is None else colrow[k])
    mosaic, wsum, count = fuse_layers(layers, weights, fuse)
    out = {"mosaic": mosaic.reshape(h, w, c), "weight": wsum.reshape(h, w), "count": count.reshape(h, w)}
    if return_all:
        out.update(depth=depth, visibility=visibility, layers=layers, weights=weights, colrow=colrow, lonlatalt=lla)
    return out
