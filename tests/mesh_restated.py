"""The mesh rule (marching tetrahedra over the Kuhn split of every cell) restated in numpy: test infrastructure, written from the rule's
text and not from the library's header or kernels.  Coordinates are fp32 element by element -- one subtraction each, one division, one
multiply, one add, exactly the operations the rule names -- and the case table is derived here from the geometry of the unit cell: for
every (tetrahedron, case) the triangles the rule lists, turned so that the normal of the triangle on its edges' midpoints points from the
inside corners to the outside ones.  Imports nothing but numpy."""
import itertools

import numpy as np

SLOT_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]      # (dx, dy, dz) of slots 0..6
PERMS = list(itertools.permutations(range(3)))                                                # lexicographic, x = 0, y = 1, z = 2


def tet_corners(perm):
    """The path of four unit-cell corners (x, y, z) of the tetrahedron of one axis permutation."""
    c = [0, 0, 0]
    path = [tuple(c)]
    for axis in perm:
        c[axis] += 1
        path.append(tuple(c))
    return path


def _case_triangles(path, case):
    """Triangles of one tetrahedron in one case: a list of three (u, v) corner pairs each, oriented."""
    inside = [c for c in range(4) if (case >> c) & 1]
    outside = [c for c in range(4) if not (case >> c) & 1]
    if len(inside) == 1:
        tris = [[(inside[0], o) for o in outside]]
    elif len(inside) == 3:
        tris = [[(outside[0], i) for i in inside]]
    elif len(inside) == 2:
        (p, q), (r, s) = inside, outside
        tris = [[(p, r), (p, s), (q, s)], [(p, r), (q, s), (q, r)]]
    else:
        return []
    pts = np.array(path, dtype=np.float64)
    outward = pts[outside].mean(axis=0) - pts[inside].mean(axis=0)
    out = []
    for tri in tris:
        mid = [(pts[u] + pts[v]) / 2 for u, v in tri]
        normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        d = float(normal @ outward)
        assert d != 0.0
        out.append(tri if d > 0 else [tri[0], tri[2], tri[1]])
    return out


PATHS = [tet_corners(perm) for perm in PERMS]
TABLE = [[_case_triangles(path, case) for case in range(16)] for path in PATHS]


def inside_of(f, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(f, dtype=np.float32) >= np.float32(level)


def position(origin_c, spacing_c, index, t=None):
    """The coordinate rule on one axis, fp32: origin + spacing * (float(index) + t)."""
    idx = np.asarray(index).astype(np.float32)
    if t is not None:
        idx = (idx + np.asarray(t, dtype=np.float32)).astype(np.float32)
    return (np.float32(origin_c) + (np.float32(spacing_c) * idx).astype(np.float32)).astype(np.float32)


def lattice_points(origin, spacing, nx, ny, z0, nz):
    """[nz, ny, nx, 3] fp32 positions of the slab z0 .. z0 + nz - 1."""
    k, j, i = np.meshgrid(np.arange(z0, z0 + nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([position(origin[0], spacing[0], i), position(origin[1], spacing[1], j), position(origin[2], spacing[2], k)], axis=-1)


def extract(f, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """f [nz, ny, nx] -> dict(vertices fp32 [V, 3], keys int64 [V], triangles int32 [T, 3], nonfinite int)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    nz, ny, nx = f.shape
    level = np.float32(level)
    ins = inside_of(f, level)
    keys = []
    for slot, (dx, dy, dz) in enumerate(SLOT_DIRS):
        a, b = ins[:nz - dz, :ny - dy, :nx - dx], ins[dz:, dy:, dx:]
        k, j, i = np.nonzero(a != b)
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 8 + slot)
    keys = np.sort(np.concatenate(keys))
    p, slot = keys >> 3, keys & 7
    i, j, k = p % nx, (p // nx) % ny, p // (nx * ny)
    d = np.array(SLOT_DIRS, dtype=np.int64)[slot]
    fa, fb = f[k, j, i], f[k + d[:, 2], j + d[:, 1], i + d[:, 0]]
    with np.errstate(all="ignore"):
        t = ((level - fa).astype(np.float32) / (fb - fa).astype(np.float32)).astype(np.float32)
        t = np.where(t >= 0, t, np.float32(0))
        t = np.where(t > 1, np.float32(1), t)
    bad = ~(np.isfinite(fa) & np.isfinite(fb))
    t = np.where(bad, np.float32(0.5), t).astype(np.float32)
    zero = np.zeros_like(t)
    vertices = np.stack([position(origin[c], spacing[c], (i, j, k)[c], np.where(d[:, c] == 1, t, zero)) for c in range(3)], axis=1)
    vid = dict(zip(keys.tolist(), range(len(keys))))

    cnt = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int32)
    for oz, oy, ox in itertools.product((0, 1), repeat=3):
        cnt += ins[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox]
    triangles = []
    for ck, cj, ci in zip(*np.nonzero((cnt > 0) & (cnt < 8))):          # C order: increasing cell index
        for path, cases in zip(PATHS, TABLE):
            case = sum(int(ins[ck + z, cj + y, ci + x]) << c for c, (x, y, z) in enumerate(path))
            for tri in cases[case]:
                ids = []
                for u, v in tri:
                    lo, hi = path[min(u, v)], path[max(u, v)]
                    s = SLOT_DIRS.index((hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]))
                    ids.append(vid[(((int(ck) + lo[2]) * ny + int(cj) + lo[1]) * nx + int(ci) + lo[0]) * 8 + s])
                triangles.append(ids)
    return {"vertices": vertices.astype(np.float32).reshape(-1, 3), "keys": keys.astype(np.int64),
            "triangles": np.array(triangles, dtype=np.int32).reshape(-1, 3), "nonfinite": int(bad.sum())}


# ---- what the tests ask of a mesh ---------------------------------------------------------------------------------------------------
def rotate_smallest_first(tri):
    """Each triangle rotated (never flipped) so that its smallest id comes first."""
    tri = np.asarray(tri).reshape(-1, 3)
    if not len(tri):
        return tri
    r = np.argmin(tri, axis=1)
    idx = (r[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(tri, idx, axis=1)


def directed_edges(tri):
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]], axis=0)


def edge_report(tri):
    """(largest multiplicity of a directed edge, directed edges whose reverse is missing [m, 2])."""
    e = directed_edges(tri)
    if not len(e):
        return 0, e
    big = int(e.max()) + 1
    code, counts = np.unique(e[:, 0] * big + e[:, 1], return_counts=True)
    rev = e[:, 1] * big + e[:, 0]
    return int(counts.max()), e[~np.isin(rev, code)]


def euler_characteristic(n_vertices, tri):
    e = np.sort(directed_edges(tri), axis=1)
    return n_vertices - len(np.unique(e, axis=0)) + len(np.asarray(tri).reshape(-1, 3))


def signed_volume(vertices, tri):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(tri).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def face_normals(vertices, tri):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(tri).reshape(-1, 3)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])


def sphere_volume(n):
    """The issue's sphere on an n^3 lattice: f = R^2 - |x - c|^2, R = 0.37 (n - 1), c = (n - 1) / 2 + (0.137, 0.187, -0.073)."""
    radius = 0.37 * (n - 1)
    c = (n - 1) / 2 + np.array([0.137, 0.187, -0.073])
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    f = radius ** 2 - ((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    return f.astype(np.float32), radius


def read_ply(path):
    """A small reader of binary little-endian PLY files with a vertex and a face element (faces: lists of three int32 behind a uchar
    count): dict of one array per vertex property plus "faces" [T, 3]."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    types = {"float": "<f4", "double": "<f8", "uchar": "u1", "int": "<i4"}
    counts, props, current = {}, {"vertex": [], "face": []}, None
    for line in lines[2:]:
        word = line.split()
        if word[:1] == ["element"]:
            current = word[1]
            counts[current] = int(word[2])
        elif word[:1] == ["property"]:
            props[current].append(word[1:])
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]], props["face"]
    vdt = np.dtype([(name, types[kind]) for kind, name in props["vertex"]])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    vert = np.frombuffer(raw, vdt, counts["vertex"], end)
    face = np.frombuffer(raw, fdt, counts["face"], end + vdt.itemsize * counts["vertex"])
    assert end + vdt.itemsize * counts["vertex"] + fdt.itemsize * counts["face"] == len(raw)
    assert (face["n"] == 3).all()
    out = {name: vert[name].copy() for name in vdt.names}
    out["faces"] = face["v"].copy()
    return out
