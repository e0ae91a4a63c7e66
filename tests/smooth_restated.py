"""The rule of eonerf_code_amd/csrc/eonerf_smooth.h (Taubin lambda|mu smoothing in fixed point) restated in numpy, int64 and fp64, from
the header's text and not from the kernels: the reference the host program and the device are compared with bit for bit.  Imports
nothing but numpy."""
import numpy as np

FRAC_BITS = 16
ONE = 1 << FRAC_BITS
MAX_COORD = 8192
MAX_STEPS = 4096
LIM = (MAX_COORD << FRAC_BITS) - 1
MAX_VERTICES, MAX_TRIANGLES = (1 << 31) - 1, 1 << 29
STATUS_CLAMPED = 1
COUNTS = ("free", "open", "pinned", "no_corner", "not_quantisable", "dead_faces")
# default Taubin pair of the Python layer
LAMBDA, MU = 0.5, -0.53


def lam_q(value):
    """A factor as the host computes it: llrint(value * 65536), ties to even."""
    q = int(np.rint(np.float64(value) * float(ONE)))
    assert abs(q) <= ONE, value
    return q


def taubin(iterations, lam=LAMBDA, mu=MU):
    """The step list of `iterations` lambda|mu iterations; mu None or 0: plain Laplacian."""
    pair = [lam_q(lam)] if not mu else [lam_q(lam), lam_q(mu)]
    return pair * int(iterations)


def grid_arrays(origin, unit):
    o = np.asarray(origin, dtype=np.float32).reshape(3).astype(np.float64)
    u = np.asarray(unit, dtype=np.float32).reshape(3).astype(np.float64)
    assert np.isfinite(o).all() and np.isfinite(u).all() and (u > 0).all(), (origin, unit)
    return o, u


def rdiv(a, b):
    """floor(a / b) rounded half up, b > 0: q = floor(a / b), r = a - q b, q + (2 r >= b).  int64 arrays (or Python ints)."""
    q = a // b                      # numpy's and Python's // are floor divisions
    r = a - q * b
    return q + (2 * r >= b)


def quantise(vertices, origin, unit):
    """(quantisable bool [V], Q int64 [V, 3], 0 where not quantisable)."""
    o, un = grid_arrays(origin, unit)
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (v.astype(np.float64) - o[None, :]) / un[None, :]
        ok = (np.isfinite(u) & (np.abs(u) < float(MAX_COORD))).all(axis=1)
    s = np.where(ok[:, None], u, 0.0) * float(ONE)
    q = np.clip(np.rint(s).astype(np.int64), -LIM, LIM)           # ties to even; the clip acts only within 2^-17 of +-8192
    return ok, q


def corners(vertices, triangles, origin, unit):
    """(quantisable [V], Q [V, 3], live bool [T], centre, nxt, prv int64 [3 * live])."""
    ok, q = quantise(vertices, origin, unit)
    n_v = len(ok)
    tri = np.asarray(triangles, dtype=np.int32).reshape(-1, 3).astype(np.int64)
    inside = ((tri >= 0) & (tri < n_v)).all(axis=1)
    live = inside & (ok[np.clip(tri, 0, max(n_v - 1, 0))].all(axis=1) if n_v else np.zeros(len(tri), dtype=bool))
    t = tri[live]
    centre = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    nxt = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    prv = np.concatenate([t[:, 2], t[:, 0], t[:, 1]])
    return ok, q, live, centre, nxt, prv


def classify(vertices, triangles, origin, unit, pinned=None, pin_open=True):
    """dict: "quantisable", "corners" int64 [V], "open", "free" bool [V], "counts" int64 [6], and the corner arrays."""
    ok, q, live, centre, nxt, prv = corners(vertices, triangles, origin, unit)
    n_v = len(ok)
    c = np.bincount(centre, minlength=n_v).astype(np.int64)[:n_v] if n_v else np.zeros(0, dtype=np.int64)
    b1 = np.zeros(n_v, dtype=np.int64)
    b2 = np.zeros(n_v, dtype=np.uint64)
    np.add.at(b1, centre, nxt - prv)
    np.add.at(b2, centre, (nxt * nxt - prv * prv).astype(np.uint64))      # mod 2^64
    is_open = (b1 != 0) | (b2 != 0)
    mask = np.zeros(n_v, dtype=bool) if pinned is None else (np.asarray(pinned).reshape(-1) != 0)
    assert len(mask) == n_v
    held = ok & (c > 0) & mask
    free = ok & (c > 0) & ~mask & ~(is_open & bool(pin_open))
    counts = np.array([free.sum(), is_open.sum(), held.sum(), (ok & (c == 0)).sum(), (~ok).sum(), (~live).sum()], dtype=np.int64)
    return {"quantisable": ok, "Q": q, "corners": c, "open": is_open, "free": free, "counts": counts, "live": live,
            "centre": centre, "next": nxt, "prev": prv}


def step(q, free, c, centre, nxt, prv, lam):
    """One Jacobi step: (Q' int64 [V, 3], clamped bool)."""
    s = np.zeros_like(q)
    np.add.at(s, centre, q[nxt] + q[prv])
    n = 2 * c
    d = s - n[:, None] * q
    assert (np.abs(d) < (1 << 62)).all()
    m = rdiv(d, np.maximum(n, 1)[:, None])
    delta = rdiv(int(lam) * m, ONE)
    moved = q + delta
    clamped = bool((free[:, None] & ((moved < -LIM) | (moved > LIM))).any())
    return np.where(free[:, None], np.clip(moved, -LIM, LIM), q), clamped


def dequantise(q, origin, unit):
    o, un = grid_arrays(origin, unit)
    return (o[None, :] + (q.astype(np.float64) * (1.0 / ONE)) * un[None, :]).astype(np.float32)


def smooth(vertices, triangles, origin, unit, steps, pinned=None, pin_open=True, return_q=False):
    """dict: "vertices" fp32 [V, 3], "counts" int64 [6] (free, open, pinned by the mask, without a corner, not quantisable, dead faces),
    "status" int, "free" / "open" bool [V].  steps: the factors lam_q, 1 .. MAX_STEPS of them, |lam_q| <= 65536."""
    steps = [int(x) for x in steps]
    assert 1 <= len(steps) <= MAX_STEPS and all(abs(x) <= ONE for x in steps), steps
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    k = classify(v, triangles, origin, unit, pinned, pin_open)
    q, status = k["Q"], 0
    for lam in steps:
        q, clamped = step(q, k["free"], k["corners"], k["centre"], k["next"], k["prev"], lam)
        status |= STATUS_CLAMPED if clamped else 0
    out = v.copy()
    moved = dequantise(q, origin, unit)
    out[k["free"]] = moved[k["free"]]
    result = {"vertices": out, "counts": k["counts"], "status": status, "free": k["free"], "open": k["open"]}
    if return_q:
        result["Q"] = q
    return result
