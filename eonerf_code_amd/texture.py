"""Textured mesh export on the device (csrc/eonerf_texture.h): the input images baked onto the mesh through their own RPCs.

extract_mesh samples the field's albedo once per vertex -- one colour per lattice spacing, the field's opinion of the ground.  The
images are finer, and orthorectify only puts them on the nadir surface, where a facade is one pixel wide.  Here every face of the mesh
gets its own patch of an atlas (two faces to a square cell, see the header for the rule), every texel its ground point, and ONE kernel
per chunk of texels loops over the K images: projection through the image's RPC, bilinear gather, the image's gain and bias undone,
occlusion against the mesh itself (MeshRaycaster.occluded), a weight by how steeply the image looks at the face, and the mean, the
median or the best image written as the texel's colour.  No K x n x C table exists at any point.

PyTorch owns the memory and the stream; every arithmetic step runs in libeonerf_hip.so.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream
from .mesh import MeshRaycaster, _host, _mesh_arrays, vertex_visibility
from .ortho import _f3, ground_points, view_directions

MAX_TEXELS = 64      # EONERF_TEXTURE_MAX_TEXELS
MAX_MEDIAN = 64      # EONERF_TEXTURE_MAX_MEDIAN
_MODES = {"mean": 0, "median": 1, "best": 2}


def atlas_layout(n_faces, texels):
    """(atlas_w, atlas_h, cells_per_row) of the atlas of n_faces faces with `texels` texels per leg (host arithmetic only)."""
    if not 1 <= int(texels) <= MAX_TEXELS:
        raise ValueError(f"texels={texels!r}: 1 .. {MAX_TEXELS}")
    out = (C.c_int64 * 3)()
    rc = _lib.lib().eonerf_texture_layout(int(n_faces), int(texels), out)
    if rc == -4:
        raise ValueError(f"{n_faces} faces at {texels} texels a leg need an atlas of more than 32768 texels a side: use fewer texels, or a simpler mesh")
    _lib.check(rc)
    return int(out[0]), int(out[1]), int(out[2])


def _uv(n_faces, texels, device):
    uv = torch.empty(n_faces, 3, 2, dtype=torch.float32, device=device)
    if n_faces == 0:
        return uv                                # (an empty tensor has no address to pass)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().eonerf_texture_uv(n_faces, int(texels), _ptr(uv), _stream()))
    return uv


@torch.no_grad()
def texture_atlas(mesh, texels=4):
    """The parameterisation alone: {"uv": fp32 [F, 3, 2], per face corner (u, v) in [0, 1]^2 with v up as OBJ has it; "size": (h, w) of
    the atlas in texels; "texels"; "cells_per_row"}.  Every pair of faces owns one square cell of (texels + 5)^2 texels."""
    vertices, faces = _mesh_arrays(mesh)
    w, h, cpr = atlas_layout(faces.shape[0], texels)
    return {"uv": _uv(faces.shape[0], texels, vertices.device), "size": (h, w), "texels": int(texels), "cells_per_row": cpr}


def _tables(images, rpcs, dev, field, image_indices):
    """The per-image device tables of eonerf_texture_bake: images (kept alive by the caller), RPCs, addresses, shapes, gain, bias."""
    from .datasets.satellite import _rpc_struct
    K = len(images)
    if K < 1 or len(rpcs) != K:
        raise ValueError("one RPC per image, at least one image")
    images = [im.to(dev, torch.float32).contiguous() for im in images]
    c = images[0].shape[2] if images[0].dim() == 3 else 0
    if any(im.dim() != 3 or im.shape[2] != c for im in images) or not 1 <= c <= 4:
        raise ValueError("images are [h, w, C] tensors with the same 1 <= C <= 4")
    raw = np.frombuffer(b"".join(bytes(_rpc_struct(r)) for r in rpcs), dtype=np.uint8).copy()
    table = {"images": images, "channels": c, "rpcs": torch.from_numpy(raw).to(dev),
             "addresses": torch.tensor([im.data_ptr() for im in images], dtype=torch.int64).to(dev),
             "shapes": torch.tensor([[im.shape[0], im.shape[1]] for im in images], dtype=torch.int32).to(dev)}
    if field is not None and getattr(field, "radiometric_normalization", False):
        idx = list(range(K)) if image_indices is None else [int(j) for j in image_indices]
        if len(idx) != K or (image_indices is None and K != field.n_input_images):
            raise ValueError(f"field=: {K} images against the field's {field.n_input_images}: pass image_indices=")
        if c != 3:
            raise ValueError("field= needs 3-channel images (the field's gain and bias are RGB)")
        ab = field.radiometricT_enc.weight.detach().to(dev, torch.float32)[torch.as_tensor(idx, device=dev), :6]      # stays on the device
        table["gain"], table["bias"] = ab[:, :3].contiguous(), ab[:, 3:6].contiguous()
    else:
        table["gain"], table["bias"] = torch.ones(K, c, device=dev), torch.zeros(K, c, device=dev)
    return table


def _view_tables(table, rpcs, min_alt, max_alt, scene_offset, scene_scale, zone, south, dev):
    """(view_dirs fp32 [K, 3] as the rays take them, to_satellite fp64 [K, 3] in the metric frame)."""
    view = view_directions(rpcs, [im.shape[:2] for im in table["images"]], min_alt, max_alt, scene_offset, scene_scale, zone, south, device=dev)
    metric = -(view.double() * torch.as_tensor(scene_scale, dtype=torch.float32).reshape(3).double().to(dev))
    return view, (metric / metric.square().sum(dim=1, keepdim=True).sqrt()).contiguous()


def _bake(lla, normal, table, to_satellite, blocked, min_cos, angle_weight, mode, colour, weight, count, best):
    n, K = lla.shape[0], len(table["images"])
    with torch.cuda.device(lla.device):
        _lib.check(_lib.lib().eonerf_texture_bake(_ptr(lla), _ptr(normal), n, _ptr(table["rpcs"]), _ptr(table["addresses"]), _ptr(table["shapes"]), K,
                                                  table["channels"], _ptr(table["gain"]), _ptr(table["bias"]), _ptr(to_satellite), _ptr(blocked),
                                                  float(min_cos), 1 if angle_weight else 0, mode, _ptr(colour), _ptr(weight), _ptr(count), _ptr(best),
                                                  _stream()))


def _check_fuse(fuse, K):
    if fuse not in _MODES:
        raise ValueError("fuse must be 'mean', 'median' or 'best'")
    if fuse == "median" and K > MAX_MEDIAN:
        raise ValueError(f"fuse='median' takes at most {MAX_MEDIAN} images ({K} given): use fuse='mean' or 'best', or bake subsets")


@torch.no_grad()
def bake_texture(mesh, images, rpcs, scene_offset, scene_scale, zone, south, min_alt, max_alt, texels=4, fuse="median", occlusion=True,
                 angle_weight=True, min_cos=0.1, field=None, image_indices=None, raycaster=None, bias=None, chunk=1 << 20, return_all=False):
    """The images baked onto the mesh: images (K tensors [h_k, w_k, C], fp32, NaN = no data) and their rpcm-format RPCs (at the images'
    downscale) -> {"atlas": fp32 [H, W, C], NaN where no image sees the texel (and where no face owns it); "uv": fp32 [F, 3, 2] (texture_atlas);
    "count": int32 [H, W], the images that see the texel; "weight": fp32 [H, W], the sum of their weights; "best": int32 [H, W], the image
    with the largest weight, -1; "face": int32 [H, W], the face that owns the texel, -1; "size", "texels", "cells_per_row"}.  save_obj writes the result.

    The mesh is a dict of extract_mesh / simplify_mesh / smooth_mesh or a (vertices, faces) pair in the normalised scene frame;
    scene_offset / scene_scale / zone / south place it on the ground exactly as orthorectify's do.
    fuse: "median" (per channel, unweighted, at most 64 images: keeps one image's cars and clouds out), "mean" (weighted) or "best" (the
      image that looks at the face most steeply, ties to the first).
    occlusion: a texel counts for image k only if the ray from its point towards that satellite (ortho.view_directions, one direction
      per image) meets no other face of the mesh, from t = bias on.  raycaster: a MeshRaycaster of this mesh to reuse.
    angle_weight / min_cos: cos = face normal . direction to the satellite in the metric frame; an image below min_cos does not count,
      the others weigh cos (or 1 without angle_weight).
    field: with radiometric_normalization, each image's gain A and bias b of rgb_j = clip(A * rgb + b) are undone, (v - b) / A, as
      orthorectify does (image_indices: the field's image index of each image); otherwise the identity.  They stay on the device.
    chunk: texels per launch; per chunk one samples launch, K any-hit casts into one [K, chunk] byte table and one bake launch.  The
      result does not depend on it.
    return_all: the dict also holds xyz fp32 [H, W, 3], lonlatalt fp64 [H, W, 3], normal fp32 [H, W, 3],
      blocked uint8 [K, H * W] (with occlusion), view_dirs fp32 [K, 3], to_satellite fp64 [K, 3].
    The defaults texels=4, min_cos=0.1 and bias (MeshRaycaster.default_bias(), 1/64 of a lattice spacing) are guesses: none has been
    measured on a converged scene.  No result is read back."""
    vertices, faces = _mesh_arrays(mesh)
    dev = vertices.device
    _check_fuse(fuse, len(images))
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk: at least one texel")
    table = _tables(images, rpcs, dev, field, image_indices)
    K, c = len(table["images"]), table["channels"]
    n_v, n_f = vertices.shape[0], faces.shape[0]
    w, h, cpr = atlas_layout(n_f, texels)
    n = w * h
    view, to_sat = _view_tables(table, rpcs, min_alt, max_alt, scene_offset, scene_scale, zone, south, dev)
    caster = None
    if occlusion and n_f:
        caster = raycaster if raycaster is not None else MeshRaycaster(mesh)
        bias = caster.default_bias() if bias is None else float(bias)
    colour = torch.empty(n, c, dtype=torch.float32, device=dev)
    weight = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    best = torch.empty(n, dtype=torch.int32, device=dev)
    m = min(chunk, max(n, 1))
    face = torch.empty(n, dtype=torch.int32, device=dev)                    # kept whole: which texels a face owns is part of the result
    xyz = torch.empty(n if return_all else m, 3, dtype=torch.float32, device=dev)
    lla = torch.empty(n if return_all else m, 3, dtype=torch.float64, device=dev)
    normal = torch.empty(n if return_all else m, 3, dtype=torch.float32, device=dev)
    blocked = torch.empty(K, m, dtype=torch.uint8, device=dev) if caster is not None else None
    all_blocked = torch.empty(K, n, dtype=torch.uint8, device=dev) if (return_all and caster is not None) else None
    v_arg = vertices if n_v else torch.zeros(1, 3, dtype=torch.float32, device=dev)          # the library takes no null pointer
    sc, off = _f3(scene_scale), _f3(scene_offset)
    L = _lib.lib()
    for first in range(0, n, chunk):
        cur = min(chunk, n - first)
        rows = slice(first, first + cur) if return_all else slice(0, cur)
        own = face[first:first + cur]
        with torch.cuda.device(dev):
            _lib.check(L.eonerf_texture_samples(_ptr(v_arg), n_v, _ptr(faces), n_f, int(texels), first, cur, sc, off, int(zone), 1 if south else 0,
                                                _ptr(own), None, _ptr(xyz[rows]), _ptr(lla[rows]), _ptr(normal[rows]), _stream()))
        blk = None
        if caster is not None:
            blk = blocked if cur == m else blocked.reshape(-1)[:K * cur].view(K, cur)     # the kernel reads a dense [K, cur] table
            for k in range(K):
                blk[k].copy_(caster.occluded(xyz[rows], (-view[k]).expand(cur, 3).contiguous(), skip_face=own, t_min=bias))
            if all_blocked is not None:
                all_blocked[:, first:first + cur] = blk
        _bake(lla[rows], normal[rows], table, to_sat, blk, min_cos, angle_weight, _MODES[fuse], colour[first:first + cur],
              weight[first:first + cur], count[first:first + cur], best[first:first + cur])
    out = {"atlas": colour.reshape(h, w, c), "uv": _uv(n_f, texels, dev), "count": count.reshape(h, w), "weight": weight.reshape(h, w),
           "best": best.reshape(h, w), "face": face.reshape(h, w), "size": (h, w), "texels": int(texels), "cells_per_row": cpr}
    if return_all:
        out.update(xyz=xyz.reshape(h, w, 3), lonlatalt=lla.reshape(h, w, 3), normal=normal.reshape(h, w, 3),
                   view_dirs=view, to_satellite=to_sat, bias=bias)
        if all_blocked is not None:
            out["blocked"] = all_blocked
    return out


def _vertex_normals(vertices, faces, scene_scale):
    """Area-weighted face normals accumulated at the vertices, metric frame, unit length (NaN where nothing accumulates)."""
    v = vertices.double() * torch.as_tensor(scene_scale, dtype=torch.float32).reshape(3).double().to(vertices.device)
    f = faces.long()
    ok = ((f >= 0) & (f < v.shape[0])).all(dim=1)
    f = f[ok]
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)               # twice the area long
    n = torch.where(torch.isfinite(n).all(dim=1, keepdim=True), n, torch.zeros_like(n))
    acc = torch.zeros_like(v)
    for corner in range(3):
        acc.index_add_(0, f[:, corner], n)
    return (acc / acc.square().sum(dim=1, keepdim=True).sqrt()).float()


@torch.no_grad()
def color_vertices(mesh, images, rpcs, scene_offset, scene_scale, zone, south, min_alt, max_alt, fuse="median", occlusion=True,
                   angle_weight=True, min_cos=0.1, field=None, image_indices=None, raycaster=None, bias=None, return_all=False):
    """The same bake with the vertices as samples -> fp32 [V, C], NaN where no image sees the vertex: it fits the mesh dict's "albedo"
    slot for save_ply.  Normals are mesh["normals"] where the dict has them (extract_mesh's: the field's own, metric frame), otherwise
    area-weighted face normals; occlusion goes through vertex_visibility.  Arguments as bake_texture; return_all: a dict with "colour",
    "count", "weight", "best", "lonlatalt", "normal"."""
    vertices, faces = _mesh_arrays(mesh)
    dev = vertices.device
    _check_fuse(fuse, len(images))
    table = _tables(images, rpcs, dev, field, image_indices)
    K, c = len(table["images"]), table["channels"]
    n = vertices.shape[0]
    view, to_sat = _view_tables(table, rpcs, min_alt, max_alt, scene_offset, scene_scale, zone, south, dev)
    colour = torch.empty(n, c, dtype=torch.float32, device=dev)
    weight = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    best = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return {"colour": colour, "count": count, "weight": weight, "best": best} if return_all else colour
    rays = torch.cat([vertices, torch.zeros(n, 3, dtype=torch.float32, device=dev)], dim=1).contiguous()       # (vertex, zero direction), depth 0
    lla = ground_points(rays, torch.zeros(n, dtype=torch.float32, device=dev), scene_offset, scene_scale, zone, south)
    given = mesh.get("normals") if isinstance(mesh, dict) else None
    normal = given.detach().to(dev, torch.float32).contiguous() if given is not None else _vertex_normals(vertices, faces, scene_scale).contiguous()
    if normal.shape != (n, 3):
        raise ValueError(f"mesh['normals']: [{n}, 3], not {tuple(normal.shape)}")
    blocked = None
    if occlusion and faces.shape[0]:
        blocked = (~vertex_visibility(mesh, view, bias=bias, raycaster=raycaster)).t().contiguous().to(torch.uint8)
    _bake(lla, normal, table, to_sat, blocked, min_cos, angle_weight, _MODES[fuse], colour, weight, count, best)
    if return_all:
        return {"colour": colour, "count": count, "weight": weight, "best": best, "lonlatalt": lla, "normal": normal, "view_dirs": view,
                "to_satellite": to_sat}
    return colour


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, pixels):
    """An 8-bit PNG of uint8 [h, w] (grey) or [h, w, 3] (RGB), rows top to bottom, with the standard library alone."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    h, w, c = pixels.shape
    if c not in (1, 3) or h < 1 or w < 1:
        raise ValueError("write_png: [h, w] or [h, w, 3], at least one pixel")
    rows = np.concatenate([np.zeros((h, 1), dtype=np.uint8), pixels.reshape(h, w * c)], axis=1)      # filter type 0 in front of every row
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n")
        fh.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0)))
        fh.write(_png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        fh.write(_png_chunk(b"IEND", b""))


def atlas_bytes(atlas):
    """uint8 [H, W] or [H, W, 3] of an atlas [H, W, C]: NaN -> 0, clipped to [0, 1], times 255, rounded to nearest even.  C = 1 is grey; of
    four channels the first three are written."""
    a = _host(atlas).astype(np.float64)
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError("a texture of 1, 3 or 4 channels (four: the first three are written)")
    a = a[:, :, 0] if a.shape[2] == 1 else a[:, :, :3]
    return np.rint(np.clip(np.nan_to_num(a, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)


def save_obj(path, mesh, texture):
    """Wavefront OBJ of a mesh dict with the texture of bake_texture: three files, `path`, <stem>.mtl and <stem>.png beside it.
    v: "vertices_utm" where the dict has it (else "vertices") minus the offset written as `# origin E N Z` -- the floor of the smallest
    finite coordinate per axis -- so that the floats most readers keep suffice for UTM metres; vt: one per face corner, texture["uv"];
    f a/ta b/tb c/tc.  The PNG holds texture["atlas"] by atlas_bytes, rows top to bottom, so that v = 1 - row / H of the uvs lands on the
    right texel.  Returns the three paths."""
    xyz = _host(mesh["vertices_utm"] if isinstance(mesh, dict) and mesh.get("vertices_utm") is not None else (mesh["vertices"] if isinstance(mesh, dict) else mesh[0]))
    xyz = xyz.astype(np.float64).reshape(-1, 3)
    faces = _host(mesh["faces"] if isinstance(mesh, dict) else mesh[1]).astype(np.int64).reshape(-1, 3)
    uv = _host(texture["uv"]).astype(np.float64).reshape(-1, 3, 2)
    if uv.shape[0] != faces.shape[0]:
        raise ValueError(f"texture['uv'] has {uv.shape[0]} faces, the mesh {faces.shape[0]}")
    pixels = atlas_bytes(texture["atlas"])
    finite = xyz[np.isfinite(xyz).all(axis=1)]
    origin = np.floor(finite.min(axis=0)) if finite.shape[0] else np.zeros(3)
    stem = os.path.splitext(os.path.abspath(path))[0]
    name = os.path.basename(stem)
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    local = xyz - origin
    lines = ["# textured mesh of an EO-NeRF density level set", "# origin %.3f %.3f %.3f" % tuple(origin), f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %.6f %.6f %.6f" % tuple(p) for p in local]
    lines += ["vt %.8f %.8f" % tuple(t) for t in uv.reshape(-1, 2)]
    lines += ["f %d/%d %d/%d %d/%d" % (f[0] + 1, 3 * i + 1, f[1] + 1, 3 * i + 2, f[2] + 1, 3 * i + 3) for i, f in enumerate(faces)]
    with open(stem + ".obj" if not path.endswith(".obj") else path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    write_png(stem + ".png", pixels)
    return (stem + ".obj" if not path.endswith(".obj") else path), stem + ".mtl", stem + ".png"
