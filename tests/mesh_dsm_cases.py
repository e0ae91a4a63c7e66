"""The meshes and grids the mesh-DSM tests share (tests/host/test_mesh_dsm_host.py on the CPU, tests/test_mesh_dsm_gpu.py on the device):
the smallest shapes at which the rasteriser of include/eonerf_mesh_dsm.h can go wrong.  A case is a dict: "name", "vertices" fp32 [V, 3],
"triangles" int32 [T, 3], "scale", "offset" (three doubles each), "grid" = (xoff, yoff, xsize, ysize, res).

Unless a case says otherwise scale = 1, res = 1, xoff = 0, the offset is 1000 m north (SHIFT: a northing below zero would get the
southern hemisphere's + 10e6) and yoff = ysize + 1000, so that a vertex written as (u, v, z) through uv() lies u cells right of and v
cells below the raster's upper-left corner: the centre of cell (j, i) is (i + 0.5, j + 0.5)."""
import numpy as np

ONE, ZERO, SHIFT = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 1000.0, 0.0)


def grid(xsize, ysize):
    return (0.0, float(ysize) + SHIFT[1], xsize, ysize, 1.0)


def uv(ysize, points):
    """(u, v, z) rows -> fp32 (east, north, z) on grid(xsize, ysize)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.stack([p[:, 0], ysize - p[:, 1], p[:, 2]], 1).astype(np.float32)


def case(name, vertices, triangles, g, scale=ONE, offset=SHIFT):
    return {"name": name, "vertices": np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3),
            "triangles": np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3), "scale": tuple(scale), "offset": tuple(offset), "grid": g}


def soup(ysize, tris):
    """Triangles given by their own three (u, v, z) corners: nothing shared."""
    pts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    return uv(ysize, pts), np.arange(len(pts), dtype=np.int32).reshape(-1, 3)


def small_random(n, seed, ysize):
    """n triangles of a few cells each, scattered over and a little around a 33 x 17 window, altitudes in -50 .. 50."""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-1.0, 34.0, n), rng.uniform(-1.0, 18.0, n)], 1)
    corners = centre[:, None, :] + rng.uniform(-2.0, 2.0, (n, 3, 2))
    z = rng.uniform(-50.0, 50.0, (n, 3, 1))
    return soup(ysize, np.concatenate([corners, z], 2))


def insert_big(vertices, triangles, at, ysize):
    """One triangle over the whole of a 70 x 70 grid, below the small ones' altitudes, as triangle number `at`."""
    big = uv(ysize, [(-10.0, -10.0, -90.0), (200.0, -10.0, -60.0), (-10.0, 200.0, -75.0)])
    n = len(vertices)
    vertices = np.concatenate([vertices, big])
    triangles = np.insert(triangles, at, np.array([n, n + 1, n + 2], dtype=np.int32), axis=0)
    return vertices, triangles


def sphere_volume():
    """The 9^3 sphere volume of tests/host/mesh_checks.cpp with its lattice: (f, level, origin, spacing)."""
    n = 9
    r, cx, cy, cz = 0.37 * (n - 1), (n - 1) / 2.0 + 0.137, (n - 1) / 2.0 + 0.187, (n - 1) / 2.0 - 0.073
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    f = (r * r - ((i - cx) ** 2 + (j - cy) ** 2 + (k - cz) ** 2)).astype(np.float32)
    return f, 0.0, (-1.0, -1.0, -1.0), (0.25, 0.25, 0.25)


SPHERE_SCALE, SPHERE_OFFSET = (20.0, 20.0, 10.0), (500000.3, 4100000.7, 35.0)
SPHERE_GRID = (499978.5, 4100022.2, 45, 43, 1.0)


def cases():
    out = []
    # ---- single triangles -------------------------------------------------------------------------------------------------------
    for xs, ys in ((1, 1), (3, 3), (5, 3)):
        tri = [(-0.3, -0.2, 3.0), (xs + 0.4, 0.1, 7.5), (0.2, ys + 0.3, -2.25)] if xs > 1 else [(0.1, 0.2, 3.0), (0.9, 0.3, 7.5), (0.4, 0.95, -2.25)]
        v, t = soup(ys, [tri])
        out.append(case(f"one triangle {xs}x{ys} ccw", v, t, grid(xs, ys)))
        out.append(case(f"one triangle {xs}x{ys} cw", v, t[:, ::-1], grid(xs, ys)))
    # the centre of a 1 x 1 grid exactly on the hypotenuse; vertices exactly on cell centres and the hypotenuse through (1.5, 1.5)
    for name, order in (("ccw", (0, 1, 2)), ("cw", (0, 2, 1))):
        v, t = soup(1, [[(0.0, 0.0, 1.0), (1.0, 0.0, 2.0), (0.0, 1.0, 4.0)]])
        out.append(case(f"centre on an edge 1x1 {name}", v, t[:, order], grid(1, 1)))
        v, t = soup(3, [[(0.5, 0.5, 1.0), (2.5, 0.5, 2.0), (0.5, 2.5, 4.0)]])
        out.append(case(f"centres on vertices and on an edge 3x3 {name}", v, t[:, order], grid(3, 3)))
        v, t = soup(3, [[(0.5, 0.5, 1.0), (4.5, 0.5, 2.0), (0.5, 2.5, 4.0)]])
        out.append(case(f"centres on vertices and on an edge 5x3 {name}", v, t[:, order], grid(5, 3)))
    # ---- wave and block boundaries ----------------------------------------------------------------------------------------------
    for n in (63, 64, 65, 257):
        v, t = small_random(n, 100 + n, 17)
        out.append(case(f"{n} small triangles 33x17", v, t, grid(33, 17)))
        v, t = small_random(n, 100 + n, 70)
        for name, where in (("lane 0", (0,)), ("lane 63", (63,)), ("twice in one wave", (5, 40))):
            bv, bt = v, t
            for at in where:
                bv, bt = insert_big(bv, bt, at, 70)
            out.append(case(f"{n} small triangles and a whole-grid one at {name} 70x70", bv, bt, grid(70, 70)))
    # ---- grid edges (8 x 6) -----------------------------------------------------------------------------------------------------
    v, t = soup(6, [[(-5.0, 1.0, 1.0), (-1.0, 2.0, 1.0), (-3.0, 5.0, 1.0)], [(9.0, 1.0, 2.0), (13.0, 2.0, 2.0), (10.0, 5.0, 2.0)],
                    [(1.0, -5.0, 3.0), (6.0, -4.0, 3.0), (3.0, -0.6, 3.0)], [(1.0, 6.6, 4.0), (6.0, 9.0, 4.0), (3.0, 12.0, 4.0)]])
    out.append(case("wholly outside on each side 8x6", v, t, grid(8, 6)))
    v, t = soup(6, [[(-2.0, 1.2, 1.0), (1.7, 2.9, 1.5), (-1.0, 4.1, 2.0)], [(6.2, 1.1, 3.0), (11.0, 3.0, 3.5), (6.4, 4.7, 4.0)],
                    [(2.2, -3.0, 5.0), (5.1, 1.8, 5.5), (3.0, 1.6, 6.0)], [(2.3, 4.2, 7.0), (5.9, 4.4, 7.5), (4.0, 9.0, 8.0)],
                    [(-3.0, -3.0, 9.0), (1.8, -0.5, 9.5), (-0.5, 1.9, 10.0)], [(6.1, -0.4, 11.0), (12.0, -4.0, 11.5), (8.7, 2.1, 12.0)],
                    [(-0.7, 4.1, 13.0), (1.9, 6.4, 13.5), (-4.0, 10.0, 14.0)], [(6.3, 6.2, 15.0), (8.4, 3.9, 15.5), (13.0, 11.0, 16.0)]])
    out.append(case("straddling each side and corner 8x6", v, t, grid(8, 6)))
    v, t = soup(6, [[(-20.0, -15.0, -3.0), (40.0, -15.0, 12.0), (-20.0, 45.0, 5.0)]])
    out.append(case("contains the whole grid 8x6", v, t, grid(8, 6)))
    # ---- layers and ties --------------------------------------------------------------------------------------------------------
    layer = lambda z, dz: [(0.2, 0.3, z), (6.7, 0.4, z + dz), (1.1, 4.9, z - dz)]       # noqa: E731
    v, t = soup(5, [layer(1.0, 0.25), layer(5.0, -0.5), layer(3.0, 0.125)])
    out.append(case("three stacked layers 7x5", v, t, grid(7, 5)))
    v, t = soup(5, [layer(2.0, 0.5), layer(-8.0, 0.0), layer(2.0, 0.5), layer(2.0, 0.5)[::-1]])
    out.append(case("coincident triangles 7x5", v, np.roll(t, 1, axis=0), grid(7, 5)))
    v, t = soup(5, [layer(-100.5, 3.0), layer(-7.0, 2.0)])
    out.append(case("negative altitudes 7x5", v, t, grid(7, 5)))
    v, t = soup(5, [layer(32767.9, 0.0), layer(32768.0, 0.0), [(3.0, 0.1, -32767.9), (6.9, 4.0, -32767.9), (3.2, 4.8, -32767.9)],
                    [(3.0, 0.1, -32768.0), (6.9, 4.0, -32768.0), (3.2, 4.8, -32768.0)], layer(-40000.0, 0.0), layer(1e30, 0.0)])
    out.append(case("altitudes at the bound 7x5", v, t, grid(7, 5)))
    # ---- degenerate and bad input -----------------------------------------------------------------------------------------------
    quad = uv(5, [(0.5, 0.5, 1.0), (5.5, 0.5, 2.0), (5.5, 4.5, 3.0), (0.5, 4.5, 4.0), (5.5, 0.5, 9.0), (3.0, 2.0, 2.5)])
    out.append(case("a vertical and a zero-size triangle between neighbours 7x5", quad,
                    [[0, 1, 2], [1, 4, 2], [0, 2, 3], [5, 5, 5], [0, 0, 2], [0, 5, 2]], grid(7, 5)))
    out.append(case("indices outside the mesh 7x5", quad, [[0, 1, 2], [-1, 1, 2], [0, 6, 2], [0, 2, 3], [0, 2, 2 ** 31 - 1], [-2 ** 31, 1, 2]], grid(7, 5)))
    bad = np.concatenate([quad, np.array([[np.nan, 2.0, 1.0], [2.0, np.inf, 1.0], [2.0, 2.0, -np.inf], [2.0, 2.0, np.nan],
                                          [131073.0, 2.0, 1.0], [2.0, -131080.0, 1.0], [-131073.0, 2.0, 1.0], [3e38, 3e38, 1.0]], dtype=np.float32)])
    out.append(case("vertices that are not finite or beyond the fixed-point range 7x5", bad,
                    [[0, 1, 2]] + [[0, 1, k] for k in range(6, 14)] + [[0, 2, 3]], grid(7, 5)))
    # the last kept coordinate: X = 2^29 exactly (u = 2^17 cells), and Y = -2^29
    edge = np.array([[131072.0, 5.0, 1.0], [-3.0, 5.0 + 131072.0, 2.0], [-3.0, -4.0, 3.0]], dtype=np.float32)
    out.append(case("coordinates exactly on the fixed-point bound 7x5", edge, [[0, 1, 2]], grid(7, 5)))
    # southern hemisphere: northings below zero get + 10e6
    v, t = small_random(40, 7, 17)
    out.append(case("negative northings 33x17", v, t, (0.0, 7000000.0 + 17.0, 33, 17, 1.0), offset=(0.0, -3000000.0, 0.0)))
    # a real georeference: res 0.5, UTM offsets, an anisotropic scale and a flipped axis
    v, t = small_random(90, 8, 17)
    v = (v / np.array([16.0, 8.0, 50.0], dtype=np.float32)).astype(np.float32)
    out.append(case("utm offsets and res 0.5 50x40", v, t, (368000.25, 3354020.5, 50, 40, 0.5), scale=(12.5, -9.75, 40.0), offset=(367995.1, 3354018.3, 12.0)))
    # ---- no triangles -----------------------------------------------------------------------------------------------------------
    out.append(case("no triangles 5x3", quad, np.zeros((0, 3), dtype=np.int32), grid(5, 3)))
    return out
