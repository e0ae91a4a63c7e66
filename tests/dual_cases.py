"""The cases the dual-contouring tests share (tests/test_dual_restated_cpu.py, tests/host/test_dual_host.py, tests/test_dual_gpu.py):
volumes, levels, lattices, gradient tables and regularisations, each a dict
    name, f [nz, ny, nx] fp32, level, origin, spacing, g fp32 [H, 3], lam, big (too large for the host program under the sanitizers).
The gradient table has one row per Hermite point of the restatement (tests/dual_restated.py), in key order.  Imports numpy only."""
import numpy as np

import dual_restated as dr

TILE = 1024                                        # EONERF_MESH_TILE: points per scan tile
BOX_LO, BOX_HI, BOX_N = 3.0, 9.0, 14               # the box's faces lie at BOX_LO - delta and BOX_HI + delta on every axis of a 14^3 lattice
SPHERE_R, SPHERE_C, SPHERE_N = 8.2, (11.3, 11.7, 12.1), 24


def _case(name, f, level, g, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), lam=0.1, big=False):
    f = np.ascontiguousarray(f, dtype=np.float32)
    h = dr.hermite(f, level, origin, spacing)
    table = g(h["points"], np.random.default_rng(len(h["keys"]) + 7)) if callable(g) else g
    table = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 3)
    assert table.shape[0] == len(h["keys"]), name
    return {"name": name, "f": f, "level": float(level), "origin": tuple(origin), "spacing": tuple(spacing), "g": table, "lam": float(lam), "big": big}


def random_gradient(points, rng):
    return rng.standard_normal((len(points), 3)).astype(np.float32)


def box_volume(delta):
    """f = min_c(h - |x_c - centre|) on 14^3 with the faces at 3 - delta and 9 + delta: positive inside."""
    centre, half = (BOX_LO + BOX_HI) / 2, (BOX_HI - BOX_LO) / 2 + delta
    z, y, x = np.meshgrid(*[np.arange(BOX_N, dtype=np.float64)] * 3, indexing="ij")
    return np.minimum(np.minimum(half - np.abs(x - centre), half - np.abs(y - centre)), half - np.abs(z - centre)).astype(np.float32)


def box_gradient(delta):
    """The analytic gradient of box_volume at points on its surface: minus the outward unit normal of the face the point lies on."""
    centre, half = (BOX_LO + BOX_HI) / 2, (BOX_HI - BOX_LO) / 2 + delta

    def g(points, rng=None):
        d = points.astype(np.float64) - centre
        axis = np.argmin(half - np.abs(d), axis=1)
        out = np.zeros((len(points), 3), dtype=np.float32)
        out[np.arange(len(points)), axis] = -np.sign(d[np.arange(len(points)), axis])
        return out
    return g


def box_case(delta, lam=0.1):
    return _case(f"box delta {delta}", box_volume(delta), 0.0, box_gradient(delta), lam=lam)


def sphere_volume():
    """f = R - |x - c| on 24^3: the signed distance, positive inside."""
    z, y, x = np.meshgrid(*[np.arange(SPHERE_N, dtype=np.float64)] * 3, indexing="ij")
    c = SPHERE_C
    return (SPHERE_R - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def sphere_gradient(points, rng=None):
    """Along the analytic gradient of sphere_volume (its length does not enter the rule)."""
    return (-(points.astype(np.float64) - np.array(SPHERE_C))).astype(np.float32)


def sphere_case(lam=0.1):
    return _case("sphere", sphere_volume(), 0.0, sphere_gradient, lam=lam)


def shell(f, value=-1.0):
    """f wrapped in one layer of outside points: no crossing edge lies on the boundary then."""
    out = np.full(tuple(n + 2 for n in f.shape), value, dtype=np.float32)
    out[1:-1, 1:-1, 1:-1] = f
    return out


def sparse_volume():
    """128 x 128 x 65 points (more than TILE^2: every scan level): -1 but for isolated inside points, some beside tile borders."""
    shape = (65, 128, 128)
    f = np.full(shape, -1.0, dtype=np.float32).reshape(-1)
    rng = np.random.default_rng(4)
    n = f.size
    assert n > TILE * TILE
    extra = [0, 1, TILE - 1, TILE, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, n - TILE, n - TILE - 1, n - 2, n - 1]
    idx = np.concatenate([rng.choice(n, 300, replace=False), np.array(extra, dtype=np.int64)])
    f[idx] = rng.uniform(0.5, 2.0, len(idx)).astype(np.float32)
    return f.reshape(shape)


def level_case():
    rng = np.random.default_rng(12)
    f = rng.standard_normal((5, 6, 7)).astype(np.float32)
    f.reshape(-1)[rng.choice(f.size, 40, replace=False)] = 0.25
    return _case("values equal to the level", f, 0.25, random_gradient)


def nonfinite_value_case():
    rng = np.random.default_rng(13)
    f = rng.standard_normal((5, 6, 7)).astype(np.float32)
    f.reshape(-1)[rng.choice(f.size, 18, replace=False)] = np.repeat(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 6)
    f.reshape(-1)[[100, 101]] = [3e38, -3e38]              # finite ends whose differences overflow under the level below: t = 0
    return _case("values that are not finite", f, -1e-3, random_gradient, origin=(0.5, -2.0, 3.0), spacing=(0.25, 0.5, -1.5))


def bad_gradient(points, rng):
    g = rng.standard_normal((len(points), 3)).astype(np.float32)
    rows = rng.permutation(len(points))
    k = len(points) // 8
    g[rows[:k]] = 0.0
    g[rows[k:2 * k], rng.integers(0, 3, k)] = np.nan
    g[rows[2 * k:3 * k], rng.integers(0, 3, k)] = np.inf
    g[rows[3 * k:4 * k], rng.integers(0, 3, k)] = -np.inf
    g[rows[4 * k:5 * k]] *= np.float32(1e-30)              # tiny but not zero: still a plane
    g[rows[5 * k:6 * k]] *= np.float32(1e30)
    return g


def bad_gradient_case():
    f = np.random.default_rng(15).standard_normal((6, 7, 8)).astype(np.float32)
    return _case("gradients that are zero, NaN or infinite", f, 0.1, bad_gradient, spacing=(0.5, 2.0, 1.25))


def no_plane_case():
    f = shell(np.random.default_rng(16).standard_normal((3, 3, 3)).astype(np.float32))
    return _case("no usable plane anywhere", f, 0.0, lambda points, rng: np.zeros((len(points), 3), dtype=np.float32))


SHAPES = [(2, 2, 2), (3, 3, 3), (2, 2, 65), (2, 65, 2), (65, 2, 2), (3, 4, 5), (9, 17, 33), (5, 5, 41)]       # (nz, ny, nx); 5 x 5 x 41 = TILE + 1 points


def random_case(shape, lam=0.1):
    f = np.random.default_rng(sum(shape) + 3 * shape[0]).standard_normal(shape).astype(np.float32)
    return _case("random " + "x".join(str(d) for d in shape[::-1]), f, 0.1, random_gradient, origin=(-1.0, -0.5, 0.25),
                 spacing=(2.0 / max(shape[2] - 1, 1), 0.37, -1.5), lam=lam)


def cases(big=True):
    for shape in SHAPES:
        yield random_case(shape)
    yield random_case((4, 5, 6), lam=dr.MIN_REGULARISATION)
    yield random_case((4, 5, 6), lam=dr.MAX_REGULARISATION)
    yield level_case()
    yield nonfinite_value_case()
    yield bad_gradient_case()
    yield no_plane_case()
    yield box_case(0.25)
    yield box_case(0.6)
    yield sphere_case()
    if big:
        yield _case("sparse 128x128x65", sparse_volume(), 0.0, random_gradient, origin=(-1.0, -1.0, -1.0), spacing=(2.0 / 127, 2.0 / 127, 2.0 / 64), big=True)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
