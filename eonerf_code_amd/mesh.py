"""Triangle mesh of a trained field (include/eonerf_mesh.h): the density sampled on a lattice, a level set of it extracted by marching
tetrahedra on the device, per-vertex normals and albedo, a binary PLY writer.

The density volume is filled slab by slab through the field's export context (fp16x3 with the fp32 retry, or fp32 -- the context
normals.density_gradient uses, so values and gradients of one mesh come from one arithmetic); the surface extraction is a pure,
bit-reproducible function of the volume (eonerf_mesh_count / eonerf_mesh_emit: classify, scan, emit; no vertex table, nothing welded).
PyTorch owns the memory and the stream; the arithmetic runs in libeonerf_hip.so.

Not here: marching cubes, vertex refinement along the gradient, floater filters, simplification and welding, textures, skipping empty
space through the occupancy grid while the volume is filled, volumes larger than one call, OBJ / glTF writers.
The default level of extract_mesh is a guess: it has not been measured on a converged scene, and neither has the quality of the mesh.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .radiance_fields.eonerf import _ptr, _stream

UNIT_CUBE = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
STATUS_CAPACITY = 1


def level_from_opacity(alpha, step):
    """The density at which one step of length `step` has opacity `alpha`: -log(1 - alpha) / step."""
    if not 0.0 < alpha < 1.0 or not step > 0.0:
        raise ValueError(f"alpha={alpha!r}, step={step!r}: need 0 < alpha < 1 and step > 0")
    return -math.log(1.0 - alpha) / step


def _f3(values, what):
    arr = (C.c_float * 3)(*[float(v) for v in values])
    if not all(math.isfinite(v) for v in arr):
        raise ValueError(f"{what}={tuple(values)!r}: every entry must be finite in fp32")
    return arr


def _shape3(shape):
    nz, ny, nx = (int(shape),) * 3 if isinstance(shape, int) else (int(s) for s in shape)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"shape={shape!r}: at least two lattice points per axis")
    return nz, ny, nx


def lattice_of(shape, bounds=UNIT_CUBE):
    """(origin, spacing) as the fp32 triples (x, y, z) the library reads, of a lattice of shape (nz, ny, nx) whose first and last
    points lie on `bounds` = ((x0, y0, z0), (x1, y1, z1))."""
    nz, ny, nx = _shape3(shape)
    lo, hi = bounds
    origin = _f3(lo, "bounds[0]")
    spacing = _f3([(float(h) - float(l)) / (n - 1) for l, h, n in zip(lo, hi, (nx, ny, nz))], "spacing")
    if any(v == 0.0 for v in spacing):
        raise ValueError(f"bounds={bounds!r}: an empty axis")
    return origin, spacing


@torch.no_grad()
def lattice_points(origin, spacing, nx, ny, z0, nz, device):
    """[nz, ny, nx, 3] fp32 positions of the slab z0 .. z0 + nz - 1 of the lattice, by the coordinate rule mesh vertices follow."""
    xyz = torch.empty(nz, ny, nx, 3, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().eonerf_mesh_lattice_points(origin, spacing, nx, ny, z0, nz, _ptr(xyz), _stream()))
    return xyz


@torch.no_grad()
def density_volume(field, shape, bounds=UNIT_CUBE, slab_points=1 << 22):
    """The field's density on a lattice: fp32 [nz, ny, nx] (shape = (nz, ny, nx), or one int for a cube), x fastest, first and last
    points on `bounds`.  Filled z-slab by z-slab (at most slab_points points per call, at least one layer): eonerf_mesh_lattice_points,
    then the density chain in the field's export precision on the context normals.density_gradient uses, with its range retry.  The values
    are what field.query_density gives at those positions in eval mode under no_grad, bit for bit (a bf16 field with eval_precision
    "same" is the exception: it has no bf16 gradient, so volume and normals both come from its fp32 export context)."""
    nz, ny, nx = _shape3(shape)
    origin, spacing = lattice_of((nz, ny, nx), bounds)
    field._context()
    dev = field.flat_params().device
    L = _lib.lib()
    layers = max(1, min(nz, int(slab_points) // (nx * ny)))
    for _attempt in range(2):
        native, flat = field._native(True, no_bf16=True)
        volume = torch.empty(nz, ny, nx, dtype=torch.float32, device=dev)
        for z0 in range(0, nz, layers):
            k = min(layers, nz - z0)
            xyz = lattice_points(origin, spacing, nx, ny, z0, k, dev)
            n = k * ny * nx
            nb = L.eonerf_field_workspace_bytes(native, n)
            ws = field._workspace("field", nb)
            _lib.check(L.eonerf_query_density(native, _ptr(flat), _ptr(xyz), n, _ptr(volume[z0:z0 + k]), _ptr(ws), ws.numel(), _stream()))
        if field._export_range_ok():      # (fp16x3 export context: range check, once more in fp32 if it fired)
            break
    return volume


@torch.no_grad()
def mesh_from_volume(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), return_keys=False):
    """Level set `level` of volume [nz, ny, nx] (fp32, on the device; lattice point (i, j, k) at origin + spacing * (i, j, k)) as
    (vertices fp32 [V, 3], faces int32 [T, 3]): marching tetrahedra by the rule of include/eonerf_mesh.h.  Inside is volume >= level;
    face normals point out of it.  Nothing is welded or dropped: where the surface stays off the volume's boundary the mesh is closed.
    One host synchronisation: the read-back of the two counts between the count and the emit call (this is an export).
    return_keys: also the int64 key (lattice point * 8 + edge slot) of every vertex."""
    if volume.dim() != 3 or volume.device.type != "cuda":
        raise ValueError("volume must be a [nz, ny, nx] tensor on the GPU (the extraction has no host form)")
    vol = volume.detach().float().contiguous()
    nz, ny, nx = vol.shape
    origin = origin if isinstance(origin, C.Array) else _f3(origin, "origin")
    spacing = spacing if isinstance(spacing, C.Array) else _f3(spacing, "spacing")
    level = float(level)
    dev = vol.device
    L = _lib.lib()
    nb = L.eonerf_mesh_workspace_bytes(nx, ny, nz)
    if not nb:
        raise ValueError(f"a {nz} x {ny} x {nx} volume: every dimension must be at least 2 and one call takes 2^28 points")
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    _lib.check(L.eonerf_mesh_count(_ptr(vol), nx, ny, nz, level, _ptr(counts), _ptr(ws), nb, _stream()))
    n_v, n_t, n_bad, _ = counts.tolist()           # the export's host synchronisation
    if n_bad:
        import warnings
        warnings.warn(f"mesh_from_volume: {n_bad} crossing edge(s) have an end that is not finite; their vertices sit at the edge's middle")
    vertices = torch.empty(max(n_v, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(n_t, 1), 3, dtype=torch.int32, device=dev)
    keys = torch.empty(max(n_v, 1), dtype=torch.int64, device=dev) if return_keys else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(L.eonerf_mesh_emit(_ptr(vol), nx, ny, nz, level, origin, spacing, _ptr(ws), nb, _ptr(vertices), n_v, _ptr(faces), n_t,
                                  _ptr(keys), _ptr(status), _stream()))
    if int(status.item()) & STATUS_CAPACITY:
        raise RuntimeError("mesh_from_volume: the emit call found more vertices or triangles than the count call (the volume changed in between?)")
    out = (vertices[:n_v], faces[:n_t])
    return out + (keys[:n_v],) if return_keys else out


def unit_normals(grad, axis_scale=None):
    """-grad / |grad| (grad first multiplied by axis_scale), 0 where the length is 0 or not finite: fp32, |g| = sqrt(gx gx + gy gy + gz gz)."""
    g = grad.float()
    if axis_scale is not None:
        g = g * torch.tensor(list(axis_scale), dtype=torch.float32, device=g.device)
    length = torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    ok = (length > 0) & torch.isfinite(length)
    return torch.where(ok[:, None], -g / length[:, None], torch.zeros_like(g))


@torch.no_grad()
def vertex_albedo(field, vertices, chunk=1 << 20):
    """The albedo head at the vertices [V, 3], through the field's forward in eval mode (its export context).  The sun direction and
    the image index the forward also takes (a vertical sun, image 0 here) do not enter the albedo head."""
    was_training = field.training
    field.train(False)
    try:
        out = []
        for i in range(0, vertices.shape[0], chunk):
            x = vertices[i:i + chunk]
            sun = torch.tensor([0.0, 0.0, 1.0], device=x.device).expand(x.shape[0], 3)
            img = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
            out.append(field(x, sun, img)[1])
    finally:
        field.train(was_training)
    return torch.cat(out, dim=0) if out else vertices.new_empty(0, 3)


@torch.no_grad()
def extract_mesh(field, resolution=256, level=None, bounds=UNIT_CUBE, scene_offset=None, scene_scale=None, normals=True, albedo=True,
                 slab_points=1 << 22, chunk=1 << 20):
    """Mesh of the level set `level` of the field's density on a resolution^3 lattice over `bounds` (scene coordinates: the normalised
    cube).  Returns a dict: "vertices" fp32 [V, 3] in scene coordinates; "faces" int32 [T, 3], normals out of the dense side; "level";
    "normals" fp32 [V, 3]: -grad sigma at the vertices (normals.density_gradient, times 1 / scene_scale when that is given: the metric
    east / north / up frame), unit length, 0 where the gradient is 0 or not finite; "albedo" fp32 [V, 3]; "vertices_utm" fp64 [V, 3] =
    vertices * scene_scale + scene_offset when both are given.
    level: a density.  The default, level_from_opacity(0.5, 2 / 128) -- half opacity over one step of a 128-sample render -- is a guess
    until it has been measured on a converged scene."""
    from .normals import _axis_scale, density_gradient
    if level is None:
        level = level_from_opacity(0.5, 2.0 / 128)
    shape = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(resolution)
    origin, spacing = lattice_of(shape, bounds)
    volume = density_volume(field, shape, bounds, slab_points=slab_points)
    vertices, faces = mesh_from_volume(volume, level, origin, spacing)
    del volume
    mesh = {"vertices": vertices, "faces": faces, "level": float(level)}
    if normals:
        axis = _axis_scale(scene_scale)
        grads = [density_gradient(field, vertices[i:i + chunk])[1] for i in range(0, vertices.shape[0], chunk)]
        grad = torch.cat(grads, dim=0) if grads else vertices.new_empty(0, 3)
        mesh["normals"] = unit_normals(grad, None if axis is None else list(axis))
    if albedo:
        mesh["albedo"] = vertex_albedo(field, vertices, chunk=chunk)
    if scene_offset is not None and scene_scale is not None:
        scale = torch.as_tensor(scene_scale, dtype=torch.float64).reshape(3).to(vertices.device)
        offset = torch.as_tensor(scene_offset, dtype=torch.float64).reshape(3).to(vertices.device)
        mesh["vertices_utm"] = vertices.double() * scale + offset
    return mesh


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def save_ply(path, mesh):
    """Binary little-endian PLY of a mesh dict: the vertices ("vertices_utm" where the dict has it, else "vertices") as float, or as
    double where they are fp64 (UTM metres do not fit a float); "normals" as nx ny nz (float) and "albedo" as uchar red green blue
    (clipped to [0, 1], times 255, rounded) where present; "faces" as lists of three int32."""
    xyz = _host(mesh["vertices_utm"] if mesh.get("vertices_utm") is not None else mesh["vertices"])
    faces = _host(mesh["faces"]).astype("<i4").reshape(-1, 3)
    double = xyz.dtype == np.float64
    real, name = ("<f8", "double") if double else ("<f4", "float")
    n = xyz.shape[0]
    fields = [("x", real), ("y", real), ("z", real)]
    header = ["ply", "format binary_little_endian 1.0", "comment marching tetrahedra of an EO-NeRF density level set",
              f"element vertex {n}"] + [f"property {name} {a}" for a in "xyz"]
    if mesh.get("normals") is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += [f"property float {a}" for a in ("nx", "ny", "nz")]
    if mesh.get("albedo") is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += [f"property uchar {a}" for a in ("red", "green", "blue")]
    header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vert = np.zeros(n, dtype=fields)
    for c, a in enumerate("xyz"):
        vert[a] = xyz[:, c]
    if mesh.get("normals") is not None:
        nrm = _host(mesh["normals"]).astype(np.float32)
        for c, a in enumerate(("nx", "ny", "nz")):
            vert[a] = nrm[:, c]
    if mesh.get("albedo") is not None:
        rgb = np.rint(np.clip(np.nan_to_num(_host(mesh["albedo"]).astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        for c, a in enumerate(("red", "green", "blue")):
            vert[a] = rgb[:, c]
    face = np.zeros(faces.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"] = 3
    face["v"] = faces
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
