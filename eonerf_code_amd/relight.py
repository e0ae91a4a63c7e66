"""Sun sweep: a finished scene rendered under sun directions no input image had (shadow maps over a day, relit views,
sun-exposure maps on a DSM grid) over libeonerf_hip.so (include/eonerf_sweep.h).

Per chunk ONE library call runs the camera pass once -- sampler and the full forward chain with the albedo and transient heads,
none of which depends on the sun -- and then, per sun direction, what does: the ambient head, the shadow ray's sample count, the
shadow pass and the final shading.  Every sun's 21 output columns are bit-identical to what render_image gives for a ray table
whose columns 8..10 hold that sun.
"""
import torch

from . import _lib
from ._lib import _ptr, _stream
from .datasets.satellite import SatRays, namedtuple_map, satrays_to_table, sun_direction
from .occupancy import OccupancyGrid, grid_on
from .sat_rendering import RESULT_SLICES, _zsteps, n_samples_of

# the result keys that depend on the sun; every other key is the same for all suns and is returned once
SUN_KEYS = ("rgb", "ambient_rgb", "geo_shadows", "sc_pts_per_ray")


def sun_table(sun_elevation_deg, sun_azimuth_deg, scene_scale, device="cuda"):
    """fp32 [K,3]: exactly the values load_rays puts into columns 8..10 of the rays of an image whose JSON carries that
    sun_elevation / sun_azimuth (scalars or sequences of K): sun_direction, then the / scene_scale, normalise (fp64), cast of
    normalize_rays."""
    def seq(v):
        return [float(x) for x in v] if hasattr(v, "__len__") else [float(v)]
    el, az = seq(sun_elevation_deg), seq(sun_azimuth_deg)
    if len(el) != len(az):
        if len(el) != 1 and len(az) != 1:
            raise ValueError(f"{len(el)} elevations against {len(az)} azimuths")
        el, az = el * (len(az) if len(el) == 1 else 1), az * (len(el) if len(az) == 1 else 1)
    dev = torch.device(device)
    d = torch.tensor([sun_direction(e, a) for e, a in zip(el, az)], dtype=torch.float64, device=dev).reshape(-1, 3)
    sc = torch.as_tensor(scene_scale, dtype=torch.float32).to(dev, torch.float64)
    s = d / sc
    return (s / torch.linalg.norm(s, dim=1, keepdim=True)).to(torch.float32)


def render_sun_sweep(radiance_field, rays: SatRays, suns, chunk: int = 5120, render_step_size: float = 1e-3, eval: bool = False,
                     keys=("rgb", "geo_shadows"), noise=None, occupancy_grid=None):
    """Render the pixels of a view under K sun directions.  suns: [K,3] as sun_table gives them (rays.sundirs is not read).
    Always an export render: under no_grad, on the module's export context (EONerfMLP.eval_precision), with render_image's
    protocol -- one host sync for the sample count, then the fp16x3 range check, and once more on the fp32 export context if it
    fired.  Returns (results, n_rendering_samples): results[key] is [K, *lead, c] for the keys that depend on the sun (SUN_KEYS)
    and [*lead, c] for all others, lead = the rays' leading shape.  Only the requested keys are kept.
    noise: per chunk (u_cam [c,S], u_retry [c,S] or None, u_sun [K,c,S]), or None: the sampler kernels draw the jitter.
    occupancy_grid: an OccupancyGrid the camera pass and every shadow pass cull by (None or any other object: no culling)."""
    grid = occupancy_grid if isinstance(occupancy_grid, OccupancyGrid) else None
    if grid is not None:
        grid.check_step_size(render_step_size)
    slices = {k: (a, b) for k, a, b in RESULT_SLICES}
    keys = tuple(keys)
    for k in keys:
        if k not in slices:
            raise KeyError(f"render_sun_sweep: unknown result key {k!r} (one of {sorted(slices)})")
    with torch.no_grad():
        radiance_field._context()
        ns = n_samples_of(render_step_size)
        radiance_field.set_n_samples(ns)
        rays_shape = rays.origins.shape
        if len(rays_shape) == 3:
            num_rays = rays_shape[0] * rays_shape[1]
            rays = namedtuple_map(lambda r: r.reshape([num_rays] + list(r.shape[2:])), rays)
        else:
            num_rays = rays_shape[0]
        table, img = satrays_to_table(rays)
        dev = table.device
        suns = torch.as_tensor(suns).to(dev, torch.float32).reshape(-1, 3).contiguous()
        n_suns = suns.shape[0]
        if n_suns < 1:
            raise ValueError("render_sun_sweep: no sun direction")
        L = _lib.lib()
        flags = _lib.F_EVAL if eval else 0
        starts = list(range(0, num_rays, chunk))
        # the chunk's [K, c, 21] columns are reused from chunk to chunk: only the requested keys stay
        buf = torch.empty(n_suns * min(chunk, max(num_rays, 1)) * 21, dtype=torch.float32, device=dev)
        for _attempt in range(2):
            native, flat = radiance_field._native(True)
            results = {k: torch.empty(((n_suns,) if k in SUN_KEYS else ()) + (num_rays, slices[k][1] - slices[k][0]), dtype=torch.float32, device=dev)
                       for k in keys}
            counts = torch.zeros(max(len(starts), 1), dtype=torch.int32, device=dev)
            for j, i in enumerate(starts):
                n = min(chunk, num_rays - i)
                if noise is None:       # production: no noise buffers, the sampler kernels draw the jitter (Philox)
                    u_cam = u_retry = u_sun = None
                else:
                    u_cam, u_retry, u_sun = (None if t is None else t.to(dev, torch.float32).contiguous() for t in noise[j])
                    if u_sun is None or tuple(u_sun.shape) != (n_suns, n, ns):
                        raise ValueError(f"render_sun_sweep: u_sun of chunk {j} must be [{n_suns}, {n}, {ns}]")
                nb = L.eonerf_sun_sweep_workspace_bytes(native, n, n_suns)
                ws = radiance_field._workspace("render", nb)
                out = buf[:n_suns * n * 21].view(n_suns, n, 21)
                with grid_on(native, grid):
                    _lib.check(L.eonerf_render_sun_sweep(native, _ptr(flat), _ptr(table[i:i + n]), _ptr(img[i:i + n]), _ptr(_zsteps(dev, ns)),
                                                         _ptr(u_cam), _ptr(u_retry), _ptr(u_sun), _ptr(suns), n_suns, n, flags, _ptr(out),
                                                         _ptr(counts[j:j + 1]), _ptr(ws), ws.numel(), _stream()))
                for k in keys:
                    a, b = slices[k]
                    if k in SUN_KEYS:
                        results[k][:, i:i + n] = out[:, :, a:b]
                    else:
                        results[k][i:i + n] = out[0, :, a:b]
            n_rendering_samples = int(counts.sum().item())      # the only host sync of the call
            if radiance_field._export_range_ok():
                break
    lead = tuple(rays_shape[:-1])
    return {k: v.reshape(*(((n_suns,) if k in SUN_KEYS else ()) + lead), -1) for k, v in results.items()}, n_rendering_samples
