"""The component rule (include/eonerf_components.h) restated in numpy: test infrastructure, written from the rule's text and not from
the library's kernels.  Labels are found by minimum-label propagation: every point on the side starts with its own linear index and
takes, sweep after sweep, the smallest label among itself and its neighbours in the seven directions and their negatives, until a sweep
changes nothing.  (Between sweeps every label is replaced by the label of the point it names -- a point of the same component with a
label that is no larger -- which changes no fixed point and shortens long paths.)  Then counts, boundary flags and the filter.
Imports nothing but numpy."""
import numpy as np

DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]      # (dx, dy, dz): the owned edges of the mesh rule
BOUNDARY = np.uint32(0x80000000)


def side_mask(f, level, side):
    """side 0: f >= level (a NaN is outside); side 1: the complement."""
    with np.errstate(invalid="ignore"):
        inside = np.asarray(f, dtype=np.float32) >= np.float32(level)
    return inside if side == 0 else ~inside


def label_mask(mask):
    """mask [nz, ny, nx] bool -> labels int32 [nz, ny, nx]: the smallest linear index of each point's component, -1 off the mask."""
    nz, ny, nx = mask.shape
    big = np.int64(mask.size)
    lab = np.where(mask, np.arange(mask.size, dtype=np.int64).reshape(mask.shape), big)
    while True:
        new = lab.copy()
        for dx, dy, dz in DIRS:
            lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
            hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
            both = mask[lo] & mask[hi]
            new[lo] = np.where(both, np.minimum(new[lo], lab[hi]), new[lo])
            new[hi] = np.where(both, np.minimum(new[hi], lab[lo]), new[hi])
        flat = new.reshape(-1)
        on = flat < big
        flat[on] = np.minimum(flat[on], flat[flat[on]])
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1).astype(np.int32)


def boundary_mask(shape):
    nz, ny, nx = shape
    b = np.zeros(shape, dtype=bool)
    b[0], b[-1], b[:, 0], b[:, -1], b[:, :, 0], b[:, :, -1] = True, True, True, True, True, True
    return b


def label(f, level, side=0):
    """f [nz, ny, nx] -> dict(labels int32, info uint32 (both [nz, ny, nx]), counts = (components, points, largest size, its root))."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    mask = side_mask(f, level, side)
    labels = label_mask(mask)
    flat = labels.reshape(-1)
    on = flat >= 0
    size = np.bincount(flat[on], minlength=flat.size).astype(np.uint32)
    touches = np.bincount(flat[on & boundary_mask(f.shape).reshape(-1)], minlength=flat.size) > 0
    info = size | np.where(touches, BOUNDARY, np.uint32(0))
    roots = np.nonzero(size)[0]
    if len(roots):
        largest = int(size[roots].max())
        root = int(roots[size[roots] == largest].min())
    else:
        largest, root = 0, -1
    return {"labels": labels, "info": info.astype(np.uint32).reshape(f.shape), "counts": (len(roots), int(on.sum()), largest, root)}


def dropped_roots(info, min_points, protect_boundary):
    """Roots of the components the filter drops: count below min_points and not (protect_boundary and boundary bit)."""
    flat = np.asarray(info, dtype=np.uint32).reshape(-1)
    count = (flat & ~BOUNDARY).astype(np.int64)
    drop = (count > 0) & (count < min_points)
    if protect_boundary:
        drop &= (flat & BOUNDARY) == 0
    return np.nonzero(drop)[0]


def filter_volume(f, labels, info, side, min_points, protect_boundary):
    """-> (f_out fp32, (components dropped, points dropped)): the points of dropped components set to -inf (side 0) or +inf (side 1)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    roots = dropped_roots(info, min_points, protect_boundary)
    hit = np.isin(labels, roots) & (labels >= 0)
    out = f.copy()
    out[hit] = np.float32(np.inf if side else -np.inf)
    return out, (len(roots), int(hit.sum()))


def vertex_components(keys, labels, shape):
    """The component of each mesh vertex (key = point * 8 + slot): the label of the end of its edge that is on side 0."""
    nz, ny, nx = shape
    flat = np.asarray(labels).reshape(-1)
    keys = np.asarray(keys, dtype=np.int64)
    p, slot = keys >> 3, keys & 7
    d = np.array(DIRS + [(0, 0, 0)], dtype=np.int64)[slot]
    far = p + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny
    return np.where(flat[p] >= 0, flat[p], flat[far]).astype(np.int32)


def same_partition(a, b):
    """Do two label arrays (any ids; `off` marks no component: -1 here, 0 for scipy) split the same points into the same groups?"""
    (a, off_a), (b, off_b) = a, b
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    on = a != off_a
    if not np.array_equal(on, b != off_b):
        return False
    pairs = np.unique(np.stack([a[on], b[on]], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs)


def structure14():
    """The 3x3x3 structuring element (z, y, x) of the adjacency: the centre, the seven directions and their negatives."""
    s = np.zeros((3, 3, 3), dtype=bool)
    s[1, 1, 1] = True
    for dx, dy, dz in DIRS:
        s[1 + dz, 1 + dy, 1 + dx] = True
        s[1 - dz, 1 - dy, 1 - dx] = True
    return s
