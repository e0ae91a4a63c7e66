"""Triangle mesh of a trained field (include/eonerf_mesh.h): the density sampled on a lattice, a level set of it extracted by marching
tetrahedra on the device, per-vertex normals and albedo, a binary PLY writer.

The density volume is filled slab by slab through the field's export context (fp16x3 with the fp32 retry, or fp32 -- the context
normals.density_gradient uses, so values and gradients of one mesh come from one arithmetic); the surface extraction is a pure,
bit-reproducible function of the volume (eonerf_mesh_count / eonerf_mesh_emit: classify, scan, emit; no vertex table, nothing welded).
PyTorch owns the memory and the stream; the arithmetic runs in libeonerf_hip.so.

Mesh clean-up (include/eonerf_components.h) works on the volume in front of the extraction: label_components finds the solids the mesh
encloses -- the connected components of the inside lattice points under the 14 edges of the mesher's own split -- or, on the outside,
the cavities; filter_components drops solids below a point count or all but the k largest and fills cavities, element-wise, so that
the mesh of the filtered volume is the mesh of the original one without those components, bit for bit; vertex_components gives every
vertex the id of its solid.  Every filter is off by default: what a good min_points is on a converged scene has not been measured.

rasterize_mesh (include/eonerf_mesh_dsm.h) looks straight down on a mesh: for every cell of a georeferenced grid the altitude of the highest
surface under the cell's centre, the face that gave it and per-vertex attributes interpolated there (an ortho view of albedo, normals or
component ids).  evaluate_mesh_dsm sends that raster through dsm.mask_water -> register_dsm -> dsm_mae, which puts a mesh -- and with it the
level and every clean-up filter -- on the scale of the validation DSM MAE.

simplify_mesh (csrc/eonerf_simplify.h, a staged header) clusters the vertices of a mesh on a coarse grid: all vertices of a cell become
one -- the cell's mean, or the input vertex nearest to it -- and triangles that lose a corner to a merge disappear.  A pure,
bit-reproducible function of its input; extract_mesh(simplify=k) runs it with cells of k lattice spacings in front of normals and albedo.
Off by default: what it costs in DSM MAE on a converged scene has not been measured.

smooth_mesh (csrc/eonerf_smooth.h, a staged header) runs Taubin's lambda|mu iteration of the face-weighted umbrella operator on positions
in fixed point (2^-16 of a unit -- for a mesh of extract_mesh a lattice spacing): a Laplacian step with factor lambda > 0, then one with
mu < -lambda, so the surface loses the roughness marching tetrahedra leave at the scale of one spacing without shrinking.  It keeps
every vertex, every face and their order, so every per-vertex table stays valid; vertices on an open boundary stay where they are unless
pin_open=False.  Every sum is an integer sum: a pure, bit-reproducible function of its input.  extract_mesh(smooth=k) runs k iterations
after the extraction and in front of simplify, normals and albedo.  Off by default: what it does to the DSM MAE of a trained field is
in profiles/smooth_ab.txt, not in a default.

MeshRaycaster, render_mesh and vertex_visibility (csrc/eonerf_raycast.h, a staged header) cast rays against a mesh: the closest hit
(t, face, barycentric weights) or whether anything blocks a ray, defined as the minimum over ALL triangles by a rule in fp64 and found
through a uniform grid that may not change a bit of it.  render_mesh gives the depth of a mesh through the camera of an input image on
the scale of render_image's depth, per-vertex tables interpolated there, and the hard shadow of that image's sun; vertex_visibility says
which vertices a sun or a satellite sees.  The default grid and both bias defaults are guesses (profiles/raycast_ab.txt has what was measured).

dual_contour (csrc/eonerf_dual.h, a staged header) is the second mesher: one vertex per cell the surface crosses, placed by minimising
the quadric of the planes through the crossing points of the cell's edges with the field's gradient there as normal, and one quad per
sign-changing lattice edge, so that vertices can sit on ridges and corners inside a cell and a surface takes about a third of marching
tetrahedra's triangles.  It returns the same kind of mesh, so everything above takes it as it is; extract_mesh(method="dual") runs it
with normals.density_gradient at the Hermite points.  Marching tetrahedra stay the default; the default regularisation 0.1 is a guess.

Not here: choosing a quad's diagonal by the Hermite normals, manifold dual contouring, per-vertex component ids of a dual mesh, adaptive
(octree) cells, intersection-free guarantees, a BVH or any structure for meshes that do not fit a uniform grid, perspective cameras other than ray tables, anti-aliasing, texture atlases, a loss on the
mesh's shadows, cotangent or area weights, bilateral or feature-preserving filters, implicit smoothing, re-projection onto the level set,
sliding open vertices along their boundary, marching cubes, vertex refinement along the gradient, filters on area or height above ground, labelling of the mesh graph
itself, edge collapse, quadric error representatives, welding by distance, removal of duplicate triangles, textures, skipping empty space through the occupancy grid while the volume is filled, volumes larger
than one call, OBJ / glTF writers.
The default level of extract_mesh is a guess: it has not been measured on a converged scene, and neither has the quality of the mesh.
So is the default regularisation of dual_contour and extract_mesh(method="dual"), 0.1 (profiles/dual_ab.txt has what was measured).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

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


DUAL_MIN_REGULARISATION, DUAL_MAX_REGULARISATION = 2.0 ** -10, 16.0      # EONERF_DUAL_MIN_REG_LOG2, EONERF_DUAL_MAX_REG_LOG2
DUAL_REGULARISATION = 0.1           # the default lambda of dual_contour and extract_mesh(method="dual"): a guess, not measured
DUAL_REPORT = ("clamped", "fallback", "dropped_planes")
MESH_METHODS = ("tetra", "dual")


@torch.no_grad()
def dual_contour(volume, level, gradient, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), regularisation=DUAL_REGULARISATION, return_keys=False,
                 chunk=1 << 20):
    """Level set `level` of volume [nz, ny, nx] (fp32, on the device; lattice point (i, j, k) at origin + spacing * (i, j, k)) by dual
    contouring, the rule of csrc/eonerf_dual.h (a staged header): one vertex per cell the surface crosses, placed in the cell by
    minimising the quadric of the planes through the crossing points of the cell's edges (the Hermite points) with the field's gradient
    there as normal, and two triangles per sign-changing lattice edge.  Vertices can therefore sit on a ridge or a corner inside a
    cell, which marching tetrahedra cut off.  Inside is volume >= level; face normals point out of it.  Nothing is welded; every edge
    is shared by an even number of triangles, but the mesh is NOT promised to be a 2-manifold.  Bit-reproducible.
    gradient: a callable points fp32 [n, 3] -> fp32 [n, 3] (asked in chunks of at most `chunk` Hermite points, in the volume's
    coordinates; for a field: lambda p: normals.density_gradient(field, p)[1]), or a tensor [H, 3], row h for Hermite point h.  Its
    sign and length do not matter; rows that are zero or not finite are left out of their cells' quadrics and counted.
    regularisation: lambda, the pull towards the mean of a cell's Hermite points in lattice spacings, in [2^-10, 16].  The default 0.1
    is a guess: it has not been measured on a converged scene.
    Returns (vertices fp32 [V, 3], faces int32 [T, 3], report): report = {"hermite", "vertices", "faces", "nonfinite_edges",
    "clamped" (vertices the solve put outside their cell, held on its wall), "fallback" (vertices left at the mean: a solve that was
    not finite), "dropped_planes", "regularisation"}.  return_keys: also (cell_keys int64 [V]: each vertex' cell index, hermite fp32
    [H, 3]: the Hermite points, hermite_keys int64 [H]: lattice point * 8 + axis).
    Two host synchronisations: the read-back of the counts between the count and the other calls, and of status and report at the end."""
    if volume.dim() != 3 or volume.device.type != "cuda":
        raise ValueError("volume must be a [nz, ny, nx] tensor on the GPU (the extraction has no host form)")
    lam = float(regularisation)
    if not (math.isfinite(lam) and DUAL_MIN_REGULARISATION <= lam <= DUAL_MAX_REGULARISATION):
        raise ValueError(f"regularisation={regularisation!r}: finite and in [2^-10, 16]")
    vol = volume.detach().float().contiguous()
    nz, ny, nx = vol.shape
    origin = origin if isinstance(origin, C.Array) else _f3(origin, "origin")
    spacing = spacing if isinstance(spacing, C.Array) else _f3(spacing, "spacing")
    level = float(level)
    dev = vol.device
    L = _lib.lib()
    nb = L.eonerf_dual_workspace_bytes(nx, ny, nz)
    if not nb:
        raise ValueError(f"a {nz} x {ny} x {nx} volume: every dimension must be at least 2 and one call takes 2^28 points")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.check(L.eonerf_dual_count(_ptr(vol), nx, ny, nz, level, _ptr(counts), _ptr(ws), nb, _stream()))
        n_h, n_v, n_t, n_bad = counts.tolist()         # the export's host synchronisation
        if n_bad:
            import warnings
            warnings.warn(f"dual_contour: {n_bad} crossing edge(s) have an end that is not finite; their Hermite points sit at the edge's middle")
        back = torch.zeros(6, dtype=torch.int64, device=dev)           # report[4], then the two status words in the low halves of two more
        points = torch.empty(max(n_h, 1), 3, dtype=torch.float32, device=dev)
        point_keys = torch.empty(max(n_h, 1), dtype=torch.int64, device=dev) if return_keys else None
        _lib.check(L.eonerf_dual_hermite(_ptr(vol), nx, ny, nz, level, origin, spacing, _ptr(ws), nb, _ptr(points), n_h, _ptr(point_keys),
                                         C.c_void_p(back.data_ptr() + 32), _stream()))
        if callable(gradient):
            parts = [gradient(points[i:i + chunk]) for i in range(0, n_h, chunk)]
            table = torch.cat(parts, dim=0) if parts else points.new_empty(0, 3)
        else:
            table = gradient
        table = torch.as_tensor(table).detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
        if table.shape[0] != n_h:
            raise ValueError(f"gradient: one row per Hermite point, {n_h} x 3, not {tuple(table.shape)}")
        g_in = table if n_h else torch.zeros(1, 3, dtype=torch.float32, device=dev)          # the library takes no null pointer
        vertices = torch.empty(max(n_v, 1), 3, dtype=torch.float32, device=dev)
        faces = torch.empty(max(n_t, 1), 3, dtype=torch.int32, device=dev)
        cell_keys = torch.empty(max(n_v, 1), dtype=torch.int64, device=dev) if return_keys else None
        _lib.check(L.eonerf_dual_emit(_ptr(vol), nx, ny, nz, level, origin, spacing, _ptr(g_in), n_h, lam, _ptr(ws), nb, _ptr(vertices), n_v,
                                      _ptr(cell_keys), _ptr(faces), n_t, _ptr(back), C.c_void_p(back.data_ptr() + 40), _stream()))
        numbers = back.tolist()                                        # the second host synchronisation
    if (numbers[4] | numbers[5]) & STATUS_CAPACITY:
        raise RuntimeError("dual_contour: a later call found more Hermite points, vertices or triangles than the count call (the volume changed in between?)")
    report = {"hermite": n_h, "vertices": n_v, "faces": n_t, "nonfinite_edges": n_bad, **dict(zip(DUAL_REPORT, numbers[:3])), "regularisation": lam}
    out = (vertices[:n_v], faces[:n_t], report)
    return out + (cell_keys[:n_v], points[:n_h], point_keys[:n_h]) if return_keys else out


SIDES = {"inside": 0, "outside": 1, 0: 0, 1: 1}
BOUNDARY_BIT = 0x80000000
COUNT_MASK = 0x7FFFFFFF
ALL_POINTS = 1 << 29            # a min_points above every count (one call takes 2^28 points)
SLOT_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))      # (dx, dy, dz) of the edge slots 0 .. 6


def _volume3(volume):
    if volume.dim() != 3 or volume.device.type != "cuda":
        raise ValueError("volume must be a [nz, ny, nx] tensor on the GPU (the component group has no host form)")
    vol = volume.detach().float().contiguous()
    nz, ny, nx = vol.shape
    if not _lib.lib().eonerf_cc_workspace_bytes(nx, ny, nz):
        raise ValueError(f"a {nz} x {ny} x {nx} volume: every dimension must be at least 2 and one call takes 2^28 points")
    return vol, nz, ny, nx


def _label(vol, level, side):
    """labels, info and the counts ON THE DEVICE (no read-back)."""
    nz, ny, nx = vol.shape
    L = _lib.lib()
    dev = vol.device
    nb = L.eonerf_cc_workspace_bytes(nx, ny, nz)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    labels = torch.empty(nz, ny, nx, dtype=torch.int32, device=dev)
    info = torch.empty(nz, ny, nx, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    _lib.check(L.eonerf_cc_label(_ptr(vol), nx, ny, nz, float(level), side, _ptr(labels), _ptr(info), _ptr(counts), _ptr(ws), nb, _stream()))
    return labels, info, counts


def _filter(vol, labels, info, side, min_points, protect_boundary, out):
    """eonerf_cc_filter into `out` (may be vol itself); the two dropped counts stay on the device."""
    nz, ny, nx = vol.shape
    dropped = torch.empty(2, dtype=torch.int64, device=vol.device)
    _lib.check(_lib.lib().eonerf_cc_filter(_ptr(vol), _ptr(labels), _ptr(info), nx, ny, nz, side, int(min_points), int(bool(protect_boundary)),
                                           _ptr(out), _ptr(dropped), _stream()))
    return dropped


@torch.no_grad()
def label_components(volume, level, side="inside"):
    """Connected components of one side of volume [nz, ny, nx] (fp32, on the device) by the rule of include/eonerf_components.h: inside
    is volume >= level (a NaN is outside), two points are adjacent iff they differ by one of the seven edge directions of the mesher's
    split or its negative -- so the inside components are exactly the solids mesh_from_volume encloses, and the outside components off
    the volume's boundary its cavities.  Returns (labels int32 [nz, ny, nx]: the smallest linear index of the point's component, -1 off
    the side; info int32 [nz, ny, nx]: at a root (labels[r] == r) the component's point count in bits 0 .. 30 and, in bit 31 (the sign),
    whether it touches the volume's boundary, 0 elsewhere; dict of "components", "points", "largest", "largest_root").  One read-back."""
    if side not in SIDES:
        raise ValueError(f"side={side!r}: 'inside' or 'outside'")
    vol, nz, ny, nx = _volume3(volume)
    labels, info, counts = _label(vol, level, SIDES[side])
    n_comp, n_points, largest, root = counts.tolist()
    return labels, info, {"components": n_comp, "points": n_points, "largest": largest, "largest_root": root}


@torch.no_grad()
def filter_components(volume, level, min_points=0, keep_largest=0, protect_boundary=False, fill_cavities=False):
    """volume [nz, ny, nx] without its small solids and / or its cavities: (filtered volume fp32, report).  The mesh of the result is
    the mesh of `volume` without the dropped components' vertices and triangles; everything else keeps its bits and its order.
    min_points: inside components with fewer lattice points are set to -inf.  keep_largest=k: so are those smaller than the k-th largest
    (a torch.topk over the counts on the device; ties with the k-th are kept, so the result does not depend on an order).  Both may be
    given: the larger threshold holds.  protect_boundary: components that touch the volume's boundary are never dropped.
    fill_cavities: afterwards, every outside component of the result that does not touch the boundary is set to +inf -- inside first, then
    cavities, so a floater inside a bubble goes with the bubble.
    report: "threshold" (the min_points applied), "components_dropped", "points_dropped", "cavities_filled", "points_filled"."""
    vol, nz, ny, nx = _volume3(volume)
    min_points, keep_largest = int(min_points), int(keep_largest)
    if min_points < 0 or keep_largest < 0:
        raise ValueError(f"min_points={min_points}, keep_largest={keep_largest}: neither may be negative")
    out = vol.clone() if vol.data_ptr() == volume.data_ptr() else vol
    zero = torch.zeros(2, dtype=torch.int64, device=vol.device)
    dropped, filled, threshold = zero, zero, min_points
    if min_points > 0 or keep_largest > 0:
        labels, info, _ = _label(out, level, 0)
        if keep_largest > 0:
            sizes = (info.reshape(-1) & COUNT_MASK)
            kth = int(torch.topk(sizes, min(keep_largest, sizes.numel()), sorted=True).values[-1])
            threshold = max(threshold, kth)
        dropped = _filter(out, labels, info, 0, threshold, protect_boundary, out)
    if fill_cavities:
        labels, info, _ = _label(out, level, 1)
        filled = _filter(out, labels, info, 1, ALL_POINTS, True, out)
    d, f = dropped.tolist(), filled.tolist()
    return out, {"threshold": threshold, "components_dropped": d[0], "points_dropped": d[1], "cavities_filled": f[0], "points_filled": f[1]}


def vertex_components(keys, labels):
    """The component of each mesh vertex: the label of the end of its edge that is on the labelled side.  keys: int64 [V] from
    mesh_from_volume(return_keys=True) (lattice point * 8 + edge slot); labels: int32 [nz, ny, nx] of label_components on the same
    volume and level.  Plain torch on the device; int32 [V]."""
    nz, ny, nx = labels.shape
    flat = labels.reshape(-1)
    p, slot = keys >> 3, keys & 7
    step = torch.tensor([dx + dy * nx + dz * nx * ny for dx, dy, dz in SLOT_OFFSETS] + [0], dtype=torch.int64, device=keys.device)
    near, far = flat[p], flat[p + step[slot]]
    return torch.where(near >= 0, near, far)


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


class MeshDict(dict):
    """The dict extract_mesh and simplify_mesh return.  Its keys are the mesh; what simplify_mesh(factor=...) needs to lay its grid over
    the lattice the mesh came from rides along as attributes, not as keys: `lattice` = {"origin": fp32 triple, "spacing": fp32 triple,
    "shape": (nz, ny, nx)} and `scene` = (scene_scale, scene_offset) as fp64 tensors, or None."""
    lattice = None
    scene = None


@torch.no_grad()
def extract_mesh(field, resolution=256, level=None, bounds=UNIT_CUBE, scene_offset=None, scene_scale=None, normals=True, albedo=True,
                 slab_points=1 << 22, chunk=1 << 20, min_component_points=0, keep_largest=0, protect_boundary=False, fill_cavities=False,
                 components=False, simplify=0, representative="mean", smooth=0, smooth_lambda=0.5, smooth_mu=-0.53, method="tetra",
                 dual_regularisation=DUAL_REGULARISATION):
    """Mesh of the level set `level` of the field's density on a resolution^3 lattice over `bounds` (scene coordinates: the normalised
    cube).  Returns a dict: "vertices" fp32 [V, 3] in scene coordinates; "faces" int32 [T, 3], normals out of the dense side; "level";
    "normals" fp32 [V, 3]: -grad sigma at the vertices (normals.density_gradient, times 1 / scene_scale when that is given: the metric
    east / north / up frame), unit length, 0 where the gradient is 0 or not finite; "albedo" fp32 [V, 3]; "vertices_utm" fp64 [V, 3] =
    vertices * scene_scale + scene_offset when both are given.
    level: a density.  The default, level_from_opacity(0.5, 2 / 128) -- half opacity over one step of a 128-sample render -- is a guess
    until it has been measured on a converged scene.
    min_component_points, keep_largest, protect_boundary, fill_cavities: filter_components on the volume in front of the extraction;
    the dict then also carries its "report".  All off by default (no component call is made, the result keeps today's bits): what a
    good min_component_points is has not been measured.  components: also "component" int32 [V], the root id of each vertex' solid
    (label_components of the volume that was meshed), and "component_points" int32 [V], that solid's lattice points.
    simplify=k > 0: simplify_mesh with cells of k lattice spacings and `representative` ("mean" or "nearest") runs on the extracted mesh
    BEFORE normals and albedo, which the field then gives at the V' new vertices (fewer points, and right for mean positions);
    "component" and "component_points" go through "source".  The dict then also carries "source" int64 [V'] (the extracted vertex each
    new one stands for) and "simplify" (simplify_mesh's report).  0: no simplify call is made and the result keeps today's bits.
    smooth=k > 0: k lambda|mu iterations of smooth_mesh (factors smooth_lambda, smooth_mu; units of one lattice spacing) move the
    extracted vertices after the component ids are taken and BEFORE simplify, normals and albedo, which the field then gives at the moved
    vertices.  The dict then also carries "smooth" (smooth_mesh's report).  0: no smoothing call is made and the result keeps today's
    bits and keys.
    method: "tetra" (the default, and what an omitted argument gives, bit for bit) -- marching tetrahedra, mesh_from_volume -- or "dual"
    -- dual_contour on the same (filtered) volume with normals.density_gradient at the Hermite points, asked in chunks of `chunk`, and
    lambda = dual_regularisation (default 0.1: a guess, not measured).  Everything behind the mesher runs unchanged on either mesh;
    the dict of "dual" also carries "dual" (dual_contour's report).  components=True with "dual" raises ValueError: a cell can touch
    two solids, so a per-vertex component id is not defined there."""
    from .normals import _axis_scale, density_gradient
    if method not in MESH_METHODS:
        raise ValueError(f"method={method!r}: one of {MESH_METHODS}")
    if method == "dual" and components:
        raise ValueError("components=True with method='dual': a dual-contouring vertex belongs to a cell, which can touch two solids; per-vertex ids are not defined")
    if level is None:
        level = level_from_opacity(0.5, 2.0 / 128)
    shape = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(resolution)
    origin, spacing = lattice_of(shape, bounds)
    volume = density_volume(field, shape, bounds, slab_points=slab_points)
    cleanup = {}
    if min_component_points or keep_largest or fill_cavities:
        volume, cleanup["report"] = filter_components(volume, level, min_component_points, keep_largest, protect_boundary, fill_cavities)
    if method == "dual":
        vertices, faces, cleanup["dual"] = dual_contour(volume, level, lambda points: density_gradient(field, points)[1], origin, spacing,
                                                        regularisation=dual_regularisation, chunk=chunk)
    elif components:
        vertices, faces, keys = mesh_from_volume(volume, level, origin, spacing, return_keys=True)
        labels, info, _ = label_components(volume, level)
        cleanup["component"] = vertex_components(keys, labels)
        cleanup["component_points"] = info.reshape(-1)[cleanup["component"].long()] & COUNT_MASK
        del keys, labels, info
    else:
        vertices, faces = mesh_from_volume(volume, level, origin, spacing)
    del volume
    mesh = MeshDict({"vertices": vertices, "faces": faces, "level": float(level), **cleanup})
    mesh.lattice = {"origin": tuple(origin), "spacing": tuple(spacing), "shape": tuple(int(n) for n in shape)}
    if scene_offset is not None and scene_scale is not None:
        mesh.scene = (torch.as_tensor(scene_scale, dtype=torch.float64).reshape(3).to(vertices.device),
                      torch.as_tensor(scene_offset, dtype=torch.float64).reshape(3).to(vertices.device))
    if smooth:
        moved = smooth_mesh(mesh, iterations=smooth, lam=smooth_lambda, mu=smooth_mu)
        mesh.update(vertices=moved["vertices"], smooth=moved["report"])
        vertices = mesh["vertices"]
    if simplify:
        small = simplify_mesh(mesh, factor=simplify, representative=representative)
        mesh.update(vertices=small["vertices"], faces=small["faces"], source=small["source"], simplify=small["report"])
        mesh.update({k: small[k] for k in ("component", "component_points") if k in small})
        vertices, faces = mesh["vertices"], mesh["faces"]
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


def _mesh_arrays(mesh):
    """(vertices fp32 [V, 3], faces int32 [T, 3]) in scene coordinates, contiguous, from a mesh dict or a pair."""
    vertices, faces = (mesh["vertices"], mesh["faces"]) if isinstance(mesh, dict) else mesh
    if vertices.device.type != "cuda" or faces.device != vertices.device:
        raise ValueError("the mesh must be on the GPU (the rasteriser has no host form)")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("vertices [V, 3] and faces [T, 3]")
    return vertices.detach().float().contiguous(), faces.detach().to(torch.int32).contiguous()


REPRESENTATIVES = {"mean": 0, "nearest": 1}
PER_VERTEX = ("normals", "albedo", "component", "component_points")        # tables simplify_mesh gathers through "source"
SIMPLIFY_MAX_DIM = 4096


def _triple(value, what):
    values = [float(value)] * 3 if isinstance(value, (int, float)) else [float(v) for v in value]
    if len(values) != 3:
        raise ValueError(f"{what}={value!r}: one number or three")
    return values


@torch.no_grad()
def simplify_mesh(mesh, cell=None, factor=None, origin=None, dims=None, representative="mean", return_map=False):
    """The mesh with its vertices clustered on a grid, by the rule of csrc/eonerf_simplify.h: all vertices of a cell become one, a
    triangle with two corners in one cell disappears, every other triangle keeps its place, orientation and rotation.  Bit-reproducible:
    the result does not depend on the order in which the device visits vertices or triangles.
    mesh: a dict of extract_mesh, or a (vertices, faces) pair, on the GPU.
    The grid: either factor=k with a dict of extract_mesh -- cells of k lattice spacings anchored on the lattice origin, one more per
    axis than reach the lattice's last point -- or cell= (one size or three) with origin= (default: the lower corner of the finite
    vertices' bounding box) and dims= (default: what covers the bounding box; at most 4096 per axis and 2^27 cells in all, vertices
    outside the grid fall into its border cells).
    representative: "mean" -- a new vertex is the mean of its cell's vertices (to 2^-14 of a cell) -- or "nearest" -- the input vertex
    nearest to that mean, copied, at equal distance the one with the smallest index.
    Returns a dict: "vertices" fp32 [V', 3]; "faces" int32 [T', 3]; "source" int64 [V']: the input vertex each new one stands for (the
    nearest to the mean in both modes); "report": the counts (vertices_in, faces_in, vertices, faces, dropped, collapsed) and the grid
    (origin, cell, dims, representative); with return_map "vertex_map" int32 [V]: the new index of every input vertex, -1 for one with a
    coordinate that is not finite.  Every per-vertex table of an input dict ("normals", "albedo", "component", "component_points") is
    gathered through "source"; "vertices_utm" too under "nearest", and under "mean" it is computed again from the new vertices (a dict
    of extract_mesh knows its scene transform); "level" is kept.  One host synchronisation: the read-back of the counts."""
    if representative not in REPRESENTATIVES:
        raise ValueError(f"representative={representative!r}: 'mean' or 'nearest'")
    vertices, faces = _mesh_arrays(mesh)
    dev = vertices.device
    n_v, n_t = vertices.shape[0], faces.shape[0]
    lattice = getattr(mesh, "lattice", None)
    if (cell is None) == (factor is None):
        raise ValueError("simplify_mesh needs exactly one of cell= and factor=")
    if factor is not None:
        if lattice is None or origin is not None or dims is not None:
            raise ValueError("factor= lays the grid over the lattice of an extract_mesh dict (and takes no origin= or dims=); give cell= for any other mesh")
        if not float(factor) > 0:
            raise ValueError(f"factor={factor!r}: a positive number of lattice spacings")
        origin = lattice["origin"]
        cell = [float(sp) * float(factor) for sp in lattice["spacing"]]
        nz, ny, nx = lattice["shape"]
        dims = [int(math.floor((n - 1) / float(factor))) + 1 for n in (nx, ny, nz)]
    cell = _f3(_triple(cell, "cell"), "cell")
    if not all(v > 0 for v in cell):
        raise ValueError(f"cell={tuple(cell)!r}: every cell size must be positive")
    if origin is None or dims is None:                      # the bounding box of the finite vertices: one more read-back
        finite = vertices[torch.isfinite(vertices).all(dim=1)]
        lo = finite.min(dim=0).values.tolist() if finite.shape[0] else [0.0, 0.0, 0.0]
        hi = finite.max(dim=0).values.tolist() if finite.shape[0] else lo
        if origin is None:
            origin = lo
        if dims is None:
            dims = [min(max(int(math.floor((h - float(o)) / c)) + 1, 1), SIMPLIFY_MAX_DIM) for h, o, c in zip(hi, _triple(origin, "origin"), cell)]
    origin = _f3(_triple(origin, "origin"), "origin")
    dims = (C.c_int * 3)(*[int(d) for d in dims])
    L = _lib.lib()
    nb = L.eonerf_simplify_workspace_bytes(dims, n_v, n_t)
    if not nb:
        raise ValueError(f"dims={tuple(dims)!r}: each of 1 .. {SIMPLIFY_MAX_DIM}, at most 2^27 cells in all (larger cells, or a grid of its own)")
    if n_v == 0:
        vertices = torch.zeros(1, 3, dtype=torch.float32, device=dev)          # the library takes no null pointer
    if n_t == 0:
        faces = torch.zeros(1, 3, dtype=torch.int32, device=dev)
    mode = REPRESENTATIVES[representative]
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.check(L.eonerf_simplify_count(_ptr(vertices), n_v, _ptr(faces), n_t, origin, cell, dims, _ptr(ws), nb, _ptr(counts), _stream()))
        n_out, kept, dropped, collapsed = counts.tolist()          # the host synchronisation
        out_v = torch.empty(max(n_out, 1), 3, dtype=torch.float32, device=dev)
        out_t = torch.empty(max(kept, 1), 3, dtype=torch.int32, device=dev)
        source = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)
        vertex_map = torch.empty(max(n_v, 1), dtype=torch.int32, device=dev) if return_map else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(L.eonerf_simplify_emit(_ptr(vertices), n_v, _ptr(faces), n_t, origin, cell, dims, mode, _ptr(ws), nb, _ptr(out_v), n_out, _ptr(out_t),
                                          kept, _ptr(source), _ptr(vertex_map), _ptr(status), _stream()))
        if int(status.item()) & STATUS_CAPACITY:
            raise RuntimeError("simplify_mesh: the emit call found more vertices or triangles than the count call (the mesh changed in between?)")
    source = source[:n_out].long()
    out = MeshDict({"vertices": out_v[:n_out], "faces": out_t[:kept], "source": source})
    out["report"] = {"vertices_in": n_v, "faces_in": n_t, "vertices": n_out, "faces": kept, "dropped": dropped, "collapsed": collapsed,
                     "origin": tuple(origin), "cell": tuple(cell), "dims": tuple(dims), "representative": representative}
    if return_map:
        out["vertex_map"] = vertex_map[:n_v]
    if isinstance(mesh, dict):
        out.lattice, out.scene = lattice, getattr(mesh, "scene", None)
        if "level" in mesh:
            out["level"] = mesh["level"]
        for name in PER_VERTEX:
            if mesh.get(name) is not None:
                out[name] = mesh[name][source]
        if mesh.get("vertices_utm") is not None:
            if mode == REPRESENTATIVES["nearest"]:
                out["vertices_utm"] = mesh["vertices_utm"][source]
            elif out.scene is not None:
                out["vertices_utm"] = out["vertices"].double() * out.scene[0] + out.scene[1]
            else:
                raise ValueError("simplify_mesh: 'vertices_utm' under representative='mean' has to be computed again from the new vertices, and only a dict of "
                                 "extract_mesh knows its scene transform; drop the key, or use representative='nearest'")
    return out


SMOOTH_ONE = 1 << 16                 # quanta per unit (EONERF_SMOOTH_FRAC_BITS)
SMOOTH_MAX_STEPS = 4096
SMOOTH_STATUS_CLAMPED = 1
SMOOTH_COUNTS = ("free", "open", "pinned", "no_corner", "not_quantisable", "dead_faces")


def _factor_q(value, what):
    value = float(value)
    if not abs(value) <= 1.0:
        raise ValueError(f"{what}={value!r}: a factor in [-1, 1]")
    return int(np.rint(np.float64(value) * SMOOTH_ONE))           # llrint: ties to even


@torch.no_grad()
def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, origin=None, unit=None, pinned=None, pin_open=True):
    """The mesh after `iterations` lambda|mu iterations of Taubin smoothing, by the rule of csrc/eonerf_smooth.h: per iteration a step
    of the face-weighted umbrella operator with factor lam, then one with factor mu (mu=None or 0: plain Laplacian, one step an
    iteration).  Positions are integers of 2^-16 unit on the grid (origin, unit), every sum is an integer sum: the result does not
    depend on the order of the faces or of the device's lanes.  Every vertex, every face and their order are kept.
    mesh: a dict of extract_mesh / simplify_mesh, or a (vertices, faces) pair, on the GPU.
    The grid: a dict that knows its lattice gives origin and unit (the lattice origin and spacing); otherwise unit= is one number or
    three, and the defaults cost one more read-back: origin the lower corner of the finite vertices' bounding box, unit its largest
    extent / 4096 on all axes.  A vertex further than 8192 units from the origin, or not finite, stays as it is and its faces count for
    nothing.
    pinned: a mask [V] (bool or bytes) of vertices that keep their bits.  pin_open: vertices on an open boundary keep theirs too.
    Returns a MeshDict: the same "faces" tensor, new "vertices", every other key of an input dict carried over ("vertices_utm" computed
    again from the new vertices: a dict of extract_mesh knows its scene transform), and "report": the counts ("free", "open", "pinned"
    by the mask, "no_corner", "not_quantisable", "dead_faces"), the grid ("origin", "unit"), "steps" (the factors in 2^-16), "iterations"
    and "clamped" (a step wanted to leave the 8192 units and was held).  iterations=0: no library call, the same bits.
    One host synchronisation: the read-back of the counts and the status."""
    vertices, faces = _mesh_arrays(mesh)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"iterations={iterations}: not negative")
    pair = [_factor_q(lam, "lam")] + ([_factor_q(mu, "mu")] if mu else [])
    steps = pair * iterations
    if len(steps) > SMOOTH_MAX_STEPS:
        raise ValueError(f"iterations={iterations}: {len(steps)} steps, and one call takes {SMOOTH_MAX_STEPS}")
    dev = vertices.device
    n_v, n_t = vertices.shape[0], faces.shape[0]
    lattice = getattr(mesh, "lattice", None)
    if unit is None and lattice is not None:
        unit = lattice["spacing"]
        if origin is None:
            origin = lattice["origin"]
    if unit is not None:
        unit = _triple(unit, "unit")
        if not all(math.isfinite(u) and u > 0 for u in unit):
            raise ValueError(f"unit={tuple(unit)!r}: every unit must be finite and positive")
    if pinned is not None:
        pinned = torch.as_tensor(pinned).to(dev).reshape(-1).ne(0).to(torch.uint8).contiguous()
        if pinned.shape[0] != n_v:
            raise ValueError(f"pinned: a mask of {n_v} vertices, not {pinned.shape[0]}")
    out = MeshDict(mesh) if isinstance(mesh, dict) else MeshDict({"vertices": vertices, "faces": faces})
    if isinstance(mesh, dict):
        out.lattice, out.scene = lattice, getattr(mesh, "scene", None)
    if not steps:
        return out
    if out.get("vertices_utm") is not None and out.scene is None:
        raise ValueError("smooth_mesh: 'vertices_utm' has to be computed again from the new vertices, and only a dict of extract_mesh knows its scene "
                         "transform; drop the key")
    if origin is None or unit is None:                      # the bounding box of the finite vertices: one more read-back
        finite = vertices[torch.isfinite(vertices).all(dim=1)]
        lo = finite.min(dim=0).values.tolist() if finite.shape[0] else [0.0, 0.0, 0.0]
        hi = finite.max(dim=0).values.tolist() if finite.shape[0] else lo
        if origin is None:
            origin = lo
        if unit is None:
            extent = max(h - l for h, l in zip(hi, lo))
            unit = [extent / 4096.0 if extent > 0 else 1.0] * 3
    origin, unit = _f3(_triple(origin, "origin"), "origin"), _f3(unit, "unit")
    if not all(u > 0 for u in unit):
        raise ValueError(f"unit={tuple(unit)!r}: every unit must be positive in fp32")
    L = _lib.lib()
    nb = L.eonerf_smooth_workspace_bytes(n_v, n_t)
    if not nb:
        raise ValueError(f"{n_v} vertices and {n_t} faces: one call takes 2^31 - 1 vertices and 2^29 faces")
    v_in = vertices if n_v else torch.zeros(1, 3, dtype=torch.float32, device=dev)          # the library takes no null pointer
    f_in = faces if n_t else torch.zeros(1, 3, dtype=torch.int32, device=dev)
    lam_q = (C.c_int32 * len(steps))(*steps)
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        back = torch.zeros(7, dtype=torch.int64, device=dev)           # the six counts and, in the low half of the seventh, the status word
        moved = torch.empty(max(n_v, 1), 3, dtype=torch.float32, device=dev)
        _lib.check(L.eonerf_smooth_build(_ptr(v_in), n_v, _ptr(f_in), n_t, origin, unit, _ptr(pinned), int(bool(pin_open)), _ptr(ws), nb, _ptr(back), _stream()))
        _lib.check(L.eonerf_smooth_run(_ptr(v_in), n_v, n_t, origin, unit, lam_q, len(steps), _ptr(ws), nb, _ptr(moved), C.c_void_p(back.data_ptr() + 48), _stream()))
        numbers = back.tolist()                                        # the host synchronisation
    out["vertices"] = moved[:n_v]
    out["faces"] = mesh["faces"] if isinstance(mesh, dict) else faces
    out["report"] = dict(zip(SMOOTH_COUNTS, numbers[:6]), vertices=n_v, faces=n_t, origin=tuple(origin), unit=tuple(unit), steps=list(steps), iterations=iterations,
                         lam=float(lam), mu=float(mu) if mu else 0.0, pin_open=bool(pin_open), clamped=bool(numbers[6] & SMOOTH_STATUS_CLAMPED))
    if out.get("vertices_utm") is not None:
        out["vertices_utm"] = out["vertices"].double() * out.scene[0] + out.scene[1]
    return out


@torch.no_grad()
def rasterize_mesh(mesh, scene_offset, scene_scale, roi=None, grid=None, attributes=None, return_face=False, return_counts=False):
    """The mesh seen straight from above by the rule of include/eonerf_mesh_dsm.h: fp32 [ysize, xsize], per cell the altitude of the
    highest surface under the cell's centre, NaN where there is none.  Vertices go to UTM as pos = v * scene_scale + scene_offset in fp64
    (the dataset's fp32 values, as dsm.rasterize_dsm takes them); the result does not depend on the order of the faces.
    mesh: a dict of extract_mesh (its "vertices" and "faces"), or a (vertices, faces) pair in scene coordinates, on the GPU.
    roi / grid: as in dsm.rasterize_dsm -- the ROI quadruple (x, y, size, res) of a lidar DSM, or (xoff, yoff, xsize, ysize, res) with
    (xoff, yoff) the upper-left corner.  One of the two is required.
    attributes: a dict of per-vertex fp32 tensors [V] or [V, C <= 8] (mesh["albedo"], mesh["normals"], ...), interpolated at the cell
    centres on the winning face: rasters [ysize, xsize, C], NaN where the DSM is.
    With none of attributes, return_face, return_counts the raster itself is returned; otherwise a dict: "dsm"; "attributes" (a dict
    under the names given); "face" int32 [ysize, xsize], rows of `faces`, -1 where empty; "counts" = {"rasterised", "dropped",
    "degenerate", "covered"} as ints.  Nothing is read back unless return_counts asks for it."""
    from .dsm import _d3, grid_from_roi
    vertices, faces = _mesh_arrays(mesh)
    if grid is None and roi is not None:
        grid = grid_from_roi(roi)
    if grid is None:
        raise ValueError("rasterize_mesh needs roi= or grid=")
    xoff, yoff, xsize, ysize, res = float(grid[0]), float(grid[1]), int(grid[2]), int(grid[3]), float(grid[4])
    dev = vertices.device
    n_v, n_t = vertices.shape[0], faces.shape[0]
    if n_v == 0:
        vertices = torch.zeros(1, 3, dtype=torch.float32, device=dev)          # the library takes no null pointer
    if n_t == 0:
        faces = torch.zeros(1, 3, dtype=torch.int32, device=dev)
    scale, offset = _d3(scene_scale), _d3(scene_offset)
    cells = max(xsize, 0) * max(ysize, 0)
    keys = torch.empty(max(cells, 1), dtype=torch.int64, device=dev)
    dsm = torch.empty(max(ysize, 0), max(xsize, 0), dtype=torch.float32, device=dev)
    want_face = return_face or bool(attributes)
    face = torch.empty(max(ysize, 0), max(xsize, 0), dtype=torch.int32, device=dev) if want_face else None
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    tables = {}
    for name, attr in (attributes or {}).items():
        a = attr.detach().to(dev, torch.float32)
        a = a.reshape(a.shape[0], -1).contiguous() if a.dim() else a.reshape(1, 1)
        if a.shape[0] != n_v or not 1 <= a.shape[1] <= 8:
            raise ValueError(f"attributes[{name!r}]: a per-vertex tensor [V] or [V, C <= 8] with V = {n_v}, not {tuple(attr.shape)}")
        tables[name] = a if n_v else torch.zeros(1, a.shape[1], dtype=torch.float32, device=dev)
    L = _lib.lib()
    rasters = {}
    with torch.cuda.device(dev):
        _lib.check(L.eonerf_mesh_dsm_rasterize(_ptr(vertices), n_v, _ptr(faces), n_t, scale, offset, xoff, yoff, xsize, ysize, res, _ptr(keys),
                                               _ptr(dsm), _ptr(face), _ptr(counts), _stream()))
        for name, a in tables.items():
            out = torch.empty(ysize, xsize, a.shape[1], dtype=torch.float32, device=dev)
            _lib.check(L.eonerf_mesh_dsm_attributes(_ptr(vertices), n_v, _ptr(faces), n_t, scale, offset, xoff, yoff, xsize, ysize, res,
                                                    _ptr(face), _ptr(a), a.shape[1], _ptr(out), _stream()))
            rasters[name] = out
    if not (attributes or return_face or return_counts):
        return dsm
    result = {"dsm": dsm}
    if attributes:
        result["attributes"] = rasters
    if return_face:
        result["face"] = face
    if return_counts:
        result["counts"] = dict(zip(("rasterised", "dropped", "degenerate", "covered"), counts.tolist()))
    return result


@torch.no_grad()
def evaluate_mesh_dsm(mesh, gt, roi, scene_offset, scene_scale, water=None, scaling=False, return_all=False):
    """DSM MAE of a mesh against a lidar DSM, on the scale of dsm.evaluate_dsm: rasterize_mesh on the GT's grid (roi = x, y, size, res)
    -> water mask -> registration -> MAE.  Returns device double[2] = MAE, n_valid (return_all: a dict with "mae", "err", "dsm",
    "transform").  Nothing is read back."""
    from .dsm import _raster, dsm_mae, mask_water, register_dsm
    gt = _raster(gt)
    dsm = rasterize_mesh(mesh, scene_offset, scene_scale, roi=roi)
    if water is not None:
        dsm = mask_water(dsm, water)
    transform = register_dsm(gt, dsm, scaling=scaling)
    out = dsm_mae(gt, dsm, transform, return_err=return_all)
    if not return_all:
        return out
    return {"mae": out[0], "err": out[1], "dsm": dsm, "transform": transform}


RAYCAST_MAX_DIM = 4096              # EONERF_RAYCAST_MAX_DIM
RAYCAST_MAX_CELLS = 1 << 27
RAYCAST_DEFAULT_DIM = 256           # cells per axis at most by default: the fastest of 32 .. 256 on the one scene measured (profiles/raycast_ab.txt)
RAYCAST_BIAS_SPACINGS = 1.0 / 64    # the default shadow / visibility bias in lattice spacings: a guess, not measured


def _ray_columns(a, what):
    """An fp32 [N, 3] view whose rows are contiguous (columns of a ray table are read in place) -> (tensor, row stride in floats)."""
    if a.dim() != 2 or a.shape[1] != 3:
        raise ValueError(f"{what}: [N, 3], not {tuple(a.shape)}")
    if a.dtype != torch.float32 or (a.shape[0] > 1 and a.stride(0) < 3) or a.stride(1) != 1:
        a = a.detach().float().contiguous()
    return a, (int(a.stride(0)) if a.shape[0] > 1 else 3)


class MeshRaycaster:
    """A mesh with the uniform grid of csrc/eonerf_raycast.h built over it: one build, any number of casts.  Every answer is the one a
    brute force over all triangles gives by the header's rule, bit for bit; the grid only makes it cheap.
    mesh: a dict of extract_mesh / simplify_mesh / smooth_mesh, or a (vertices, faces) pair, on the GPU.
    bounds: ((x0, y0, z0), (x1, y1, z1)), the box of the grid.  Default: the lattice a dict of extract_mesh came from, grown by half a
    spacing; otherwise the extent of the finite vertices (one read-back), grown by 2^-10 of its largest side.  A triangle with a vertex
    outside the box, a vertex that is not finite or an index outside the mesh is dropped: counted, never hit.
    dims: cells per axis, one int or (nx, ny, nz); at most 4096 each and 2^27 in all.  The default -- min(RAYCAST_DEFAULT_DIM,
    ceil(sqrt(faces / 2))) on every axis, a surface of T faces crossing about sqrt(T / 2) cells a side -- is a guess until it has been
    measured on a converged scene: RAYCAST_DEFAULT_DIM = 256 is the fastest of 32, 64, 128 and 256 for a 512 x 512 view of the 256^3
    extraction of a 2,000-step synthetic field (profiles/raycast_ab.txt), the only scene measured; the square-root rule is not measured at all.
    One host synchronisation at construction: the read-back of the number of list entries."""

    def __init__(self, mesh, dims=None, bounds=None):
        self.vertices, self.faces = _mesh_arrays(mesh)
        dev = self.vertices.device
        self.n_v, self.n_t = self.vertices.shape[0], self.faces.shape[0]
        self.lattice = getattr(mesh, "lattice", None)
        if bounds is None and self.lattice is not None:
            o, s, (nz, ny, nx) = self.lattice["origin"], self.lattice["spacing"], self.lattice["shape"]
            ends = [(float(o[c]), float(o[c]) + float(s[c]) * (n - 1)) for c, n in enumerate((nx, ny, nz))]
            bounds = ([min(a, b) - 0.5 * abs(float(s[c])) for c, (a, b) in enumerate(ends)], [max(a, b) + 0.5 * abs(float(s[c])) for c, (a, b) in enumerate(ends)])
        if bounds is None:
            finite = self.vertices[torch.isfinite(self.vertices).all(dim=1)]
            lo = finite.min(dim=0).values.double().tolist() if finite.shape[0] else [0.0, 0.0, 0.0]
            hi = finite.max(dim=0).values.double().tolist() if finite.shape[0] else lo
            grow = max(h - l for h, l in zip(hi, lo)) * 2.0 ** -10 or 1.0
            bounds = ([l - grow for l in lo], [h + grow for h in hi])
        lo, hi = _triple(bounds[0], "bounds[0]"), _triple(bounds[1], "bounds[1]")
        if not all(math.isfinite(l) and math.isfinite(h) and l < h for l, h in zip(lo, hi)):
            raise ValueError(f"bounds={bounds!r}: finite, with lo < hi on every axis")
        if dims is None:
            dims = min(RAYCAST_DEFAULT_DIM, max(1, math.ceil(math.sqrt(self.n_t / 2.0))))
        dims = [int(dims)] * 3 if isinstance(dims, int) else [int(n) for n in dims]
        if len(dims) != 3 or not all(1 <= n <= RAYCAST_MAX_DIM for n in dims) or dims[0] * dims[1] * dims[2] > RAYCAST_MAX_CELLS:
            raise ValueError(f"dims={dims!r}: three entries of 1 .. {RAYCAST_MAX_DIM} and at most 2^27 cells")
        self.bounds, self.dims = (tuple(lo), tuple(hi)), tuple(dims)
        self._lo, self._hi, self._dims = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi), (C.c_int * 3)(*dims)
        L = _lib.lib()
        self._v = self.vertices if self.n_v else torch.zeros(1, 3, dtype=torch.float32, device=dev)       # the library takes no null pointer
        self._f = self.faces if self.n_t else torch.zeros(1, 3, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            cell_counts = torch.empty(dims[0] * dims[1] * dims[2], dtype=torch.int32, device=dev)
            self._built = torch.zeros(2, dtype=torch.int64, device=dev)
            _lib.check(L.eonerf_raycast_count(_ptr(self._v), self.n_v, _ptr(self._f), self.n_t, self._lo, self._hi, self._dims, _ptr(cell_counts), _ptr(self._built), _stream()))
            self.entries, self.dropped = self._built.tolist()               # the host synchronisation
            nb = L.eonerf_raycast_workspace_bytes(self._dims, self.n_t, self.entries)
            if not nb:
                raise ValueError(f"{self.entries} list entries: one grid takes 2^31 - 1; use fewer cells")
            self._ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            _lib.check(L.eonerf_raycast_build(_ptr(self._v), self.n_v, _ptr(self._f), self.n_t, self._lo, self._hi, self._dims, _ptr(cell_counts), self.entries, _ptr(self._ws),
                                              nb, _stream()))
        self._cast = torch.zeros(2, 3, dtype=torch.int64, device=dev)       # the counters of the last closest / occluded call

    def _args(self, origins, dirs, t_min, t_max):
        o, so = _ray_columns(origins, "origins")
        d, sd = _ray_columns(dirs, "dirs")
        if o.shape[0] != d.shape[0] or o.device != self.vertices.device or d.device != o.device:
            raise ValueError("origins and dirs: one row per ray, on the mesh's device")
        t_min, t_max = float(t_min), float(t_max)
        if not (0.0 <= t_min <= t_max and math.isfinite(t_min)):
            raise ValueError(f"t_min={t_min!r}, t_max={t_max!r}: need 0 <= t_min <= t_max")
        head = (_ptr(self._v), self.n_v, _ptr(self._f), self.n_t, self._lo, self._hi, self._dims, self.entries, _ptr(self._ws), self._ws.numel())
        return o, d, head + (_ptr(o), so, _ptr(d), sd, o.shape[0], t_min, t_max)

    @torch.no_grad()
    def closest(self, origins, dirs, t_min=0.0, t_max=float("inf")):
        """The first triangle each ray o + t d meets with t_min <= t <= t_max (d is not normalised: t is in its units).  origins, dirs:
        fp32 [N, 3] on the GPU; columns of a wider table are read in place.  Returns {"t": fp64 [N], NaN on a miss; "face": int32 [N],
        rows of the mesh's faces, -1; "bary": fp32 [N, 3], the weights of the face's three corners, NaN; "hit": bool [N]}.  Nothing is
        read back."""
        o, d, args = self._args(origins, dirs, t_min, t_max)
        n, dev = o.shape[0], o.device
        t = torch.empty(n, dtype=torch.float64, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev)
        bary = torch.empty(n, 3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().eonerf_raycast_closest(*args, _ptr(t), _ptr(face), _ptr(bary), _ptr(self._cast[0]), _stream()))
        return {"t": t, "face": face, "bary": bary, "hit": face >= 0}

    @torch.no_grad()
    def occluded(self, origins, dirs, skip_face=None, t_min=0.0, t_max=float("inf")):
        """bool [N]: whether any triangle but skip_face[r] (int32 [N], or None) meets ray r with t_min <= t <= t_max."""
        o, d, args = self._args(origins, dirs, t_min, t_max)
        n, dev = o.shape[0], o.device
        if skip_face is not None:
            skip_face = skip_face.to(dev, torch.int32).reshape(-1).contiguous()
            if skip_face.shape[0] != n:
                raise ValueError(f"skip_face: one face per ray ({n}), not {skip_face.shape[0]}")
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().eonerf_raycast_occluded(*args, _ptr(skip_face), _ptr(out), _ptr(self._cast[1]), _stream()))
        return out.bool()

    def counts(self):
        """The counters as ints (one host synchronisation): the grid's "entries", "dropped" triangles, "faces", "dims"; of the last
        closest() call "cast", "rejected", "hits"; of the last occluded() call "shadow_cast", "shadow_rejected", "shadow_hits"."""
        near, block = self._cast.tolist()
        return dict(entries=self.entries, dropped=self.dropped, faces=self.n_t, dims=self.dims, cast=near[0], rejected=near[1], hits=near[2], shadow_cast=block[0],
                    shadow_rejected=block[1], shadow_hits=block[2])

    def default_bias(self):
        """RAYCAST_BIAS_SPACINGS of the smallest lattice spacing (without a lattice: of the smallest cell side).  A guess: far above the
        rounding of a hit point in fp32 for a scene in the unit cube, far below anything a mesh of that lattice resolves."""
        if self.lattice is not None:
            return RAYCAST_BIAS_SPACINGS * min(abs(float(s)) for s in self.lattice["spacing"])
        return RAYCAST_BIAS_SPACINGS * min((h - l) / n for l, h, n in zip(*self.bounds, self.dims))


def _table_of(rays):
    """The fp32 [N, 11] ray table of a SatRays or of a table."""
    if isinstance(rays, torch.Tensor):
        table = rays
    else:
        from .datasets.satellite import namedtuple_map, satrays_to_table
        if rays.origins.dim() == 3:
            rays = namedtuple_map(lambda r: r.reshape([-1] + list(r.shape[2:])), rays)
        table = satrays_to_table(rays)[0]
    if table.dim() != 2 or table.shape[1] < 6 or not table.is_cuda:
        raise ValueError("rays: a SatRays or an fp32 table [N, >= 6] on the GPU")
    return table.detach().float().contiguous()


@torch.no_grad()
def render_mesh(mesh, rays, attributes=("albedo", "normals"), shadows=True, shadow_bias=None, raycaster=None):
    """The mesh seen along the rays of a view, by the rule of csrc/eonerf_raycast.h.
    rays: a ray table [N, 11] (origins 0..2, directions 3..5, sun 8..10) or a SatRays, as render_image takes.
    Returns a dict: "depth" fp32 [N, 1], the ray parameter of the first surface -- the scale of render_image's "depth", so it goes into
    get_utmalt_from_nerf_prediction unchanged -- NaN on a miss; "hit" bool [N]; "face" int32 [N] (-1); "bary" fp32 [N, 3]; per name in
    `attributes` that the mesh dict carries, the per-vertex table interpolated with bary, fp32 [N, C], NaN on a miss.
    shadows: also "sun_visible" fp32 [N, 1]: 1 where the ray from the hit point towards the sun is free, 0 where the mesh blocks it,
    NaN on a miss.  Columns 8..10 hold the direction the sun's light travels (datasets.satellite.sun_direction: downwards), so the ray
    runs along their negation, as the field's own shadow pass does.  It starts at the hit point o + t d formed in fp64 and rounded once
    to fp32, skips the face it starts on and begins at t = shadow_bias (in units of the sun column: a unit vector of the scene for a
    dataset's table).  shadow_bias defaults to MeshRaycaster.default_bias(), 1/64 of a lattice spacing: a guess, not measured -- too small and a
    neighbouring face of a concave corner shades its own edge through fp32 rounding, too large and contact shadows thinner than it vanish.
    raycaster: a MeshRaycaster of this mesh to reuse; otherwise one is built (and returned under "raycaster")."""
    caster = raycaster if raycaster is not None else MeshRaycaster(mesh)
    table = _table_of(rays)
    o, d = table[:, 0:3], table[:, 3:6]
    near = caster.closest(o, d)
    hit, face, bary = near["hit"], near["face"], near["bary"]
    out = {"depth": near["t"].float().reshape(-1, 1), "hit": hit, "face": face, "bary": bary, "raycaster": caster}
    if isinstance(mesh, dict) and attributes:
        corners = caster.faces[face.clamp(min=0).long()].long()                        # [N, 3] vertex ids; face 0 stands in on a miss
        for name in attributes:
            a = mesh.get(name)
            if a is None:
                continue
            a = a.detach().to(table.device, torch.float32)
            a = a.reshape(a.shape[0], -1)
            if a.shape[0] != caster.n_v:
                raise ValueError(f"mesh[{name!r}]: a per-vertex table of {caster.n_v} rows, not {a.shape[0]}")
            if caster.n_t == 0:
                out[name] = torch.full((table.shape[0], a.shape[1]), float("nan"), device=table.device)
                continue
            value = (a[corners] * bary.unsqueeze(-1)).sum(dim=1)
            out[name] = torch.where(hit.unsqueeze(-1), value, torch.full_like(value, float("nan")))
    if shadows:
        if table.shape[1] < 11:
            raise ValueError("shadows=True reads the sun direction from columns 8..10 of the ray table")
        bias = caster.default_bias() if shadow_bias is None else float(shadow_bias)
        point = (o.double() + near["t"].unsqueeze(-1) * d.double()).float()            # NaN on a miss: that ray is rejected
        blocked = caster.occluded(point, -table[:, 8:11], skip_face=face, t_min=bias)
        nan = torch.full((table.shape[0],), float("nan"), device=table.device)
        out["sun_visible"] = torch.where(hit, (~blocked).float(), nan).reshape(-1, 1)
        out["shadow_bias"] = bias
    return out


@torch.no_grad()
def vertex_visibility(mesh, directions, bias=None, raycaster=None):
    """bool [V, K]: whether vertex v sees the sun or the satellite k -- the ray v - t directions[k], t >= bias, meets no triangle.
    directions: fp32 [K, 3] as a ray table holds them, pointing from the sun or the satellite TOWARDS the scene: a relight.sun_table, or
    the view directions of the satellites (columns 3..5 of a row of each image).  A vertex that is not finite sees nothing.  bias (default MeshRaycaster.default_bias(), a guess) keeps the ray off the faces that
    share the vertex: they all meet it at t = 0.  Visibility for colouring a mesh from the images, sun hours, a sky-view factor."""
    caster = raycaster if raycaster is not None else MeshRaycaster(mesh)
    directions = torch.as_tensor(directions, dtype=torch.float32, device=caster.vertices.device).reshape(-1, 3)
    bias = caster.default_bias() if bias is None else float(bias)
    finite = torch.isfinite(caster.vertices).all(dim=1)
    out = torch.zeros(caster.n_v, directions.shape[0], dtype=torch.bool, device=caster.vertices.device)
    if caster.n_v == 0:
        return out
    for k in range(directions.shape[0]):
        d = (-directions[k]).expand(caster.n_v, 3).contiguous()
        out[:, k] = finite & ~caster.occluded(caster.vertices, d, t_min=bias)
    return out


@torch.no_grad()
def mesh_view_metrics(field, mesh, images, chunk=5120, render_step_size=None, occupancy_grid=None, raycaster=None, shadow_bias=None):
    """A mesh judged through the cameras of held-out images: device double[4] = the mean |mesh depth - field depth| over the rays that
    hit the mesh (ray parameters: the scale of render_image's "depth"), the number of those rays, the share of them where the mesh's
    hard shadow agrees with the field's learned one (sun_visible == (geo_shadows >= 0.5)), the number of rays cast.
    images: dicts with "rays" [h * w, 11], as validation.validate_images takes.  The field depth comes from a depth-only export render
    of the same rays, geo_shadows from a full export render with the shadow pass on (epoch 2).  Nothing is read back beyond
    render_image's own sample count."""
    from .datasets.satellite import define_satrays_from_tensors
    from .sat_rendering import render_image
    from .validation import _step_size_of
    if render_step_size is None:
        render_step_size = _step_size_of(field)
    caster = raycaster if raycaster is not None else MeshRaycaster(mesh)
    dev = caster.vertices.device
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    was_training = field.training
    field.eval()
    try:
        for data in images:
            rays = data["rays"].to(dev, torch.float32).contiguous()
            sat = define_satrays_from_tensors(rays, torch.zeros(rays.shape[0], 1, dtype=torch.int64, device=dev))
            seen = render_mesh(mesh, rays, attributes=(), shadows=True, shadow_bias=shadow_bias, raycaster=caster)
            depth = render_image(field, occupancy_grid, sat, None, None, chunk=chunk, render_step_size=render_step_size, only_depth=True, eval=True)[0]["depth"]
            full = render_image(field, occupancy_grid, sat, None, None, epoch_idx=2, chunk=chunk, render_step_size=render_step_size, eval=True)[0]
            hit = seen["hit"]
            diff = (seen["depth"].reshape(-1).double() - depth.reshape(-1).double()).abs()
            agree = (seen["sun_visible"].reshape(-1) >= 0.5) == (full["geo_shadows"].reshape(-1) >= 0.5)
            sums += torch.stack([torch.where(hit, diff, torch.zeros_like(diff)).sum(), hit.sum().double(), (agree & hit).sum().double(),
                                 torch.tensor(float(rays.shape[0]), dtype=torch.float64, device=dev)])
    finally:
        field.train(was_training)
    n = sums[1].clamp(min=1.0)
    return torch.stack([sums[0] / n, sums[1], sums[2] / n, sums[3]])


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def save_ply(path, mesh):
    """Binary little-endian PLY of a mesh dict: the vertices ("vertices_utm" where the dict has it, else "vertices") as float, or as
    double where they are fp64 (UTM metres do not fit a float); "normals" as nx ny nz (float) and "albedo" as uchar red green blue
    (clipped to [0, 1], times 255, rounded) where present; "component" as int component; "faces" as lists of three int32."""
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
    if mesh.get("component") is not None:
        fields += [("component", "<i4")]
        header += ["property int component"]
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
    if mesh.get("component") is not None:
        vert["component"] = _host(mesh["component"]).astype("<i4")
    face = np.zeros(faces.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"] = 3
    face["v"] = faces
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
