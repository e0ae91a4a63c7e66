"""The dual-contouring rule (csrc/eonerf_dual.h) restated in numpy: test infrastructure, written from the rule's text and not from the
library's kernels.  Vectorised over Hermite points, cells and quads.  The Hermite points follow the marching-tetrahedra coordinate
rule in fp32, one operation at a time; a cell's vertex is fp64 with one numpy operation per operation the rule names, in the rule's
order (a skipped term is added as +0.0, which changes no bit: no accumulator here is ever -0.0).  Imports numpy and mesh_restated."""
import numpy as np

import mesh_restated as mr

VERSION = 1
MIN_REGULARISATION = 2.0 ** -10
MAX_REGULARISATION = 16.0
STATUS_CAPACITY = 1
AXIS_DIRS = mr.SLOT_DIRS[:3]                    # slot a = the edge along axis a: (dx, dy, dz)
OTHER_AXES = ((1, 2), (0, 2), (0, 1))           # of edge axis a: the two other axes, the lower first (offsets u, v of e = 4a + 2v + u)
RING_AXES = ((1, 2), (2, 0), (0, 1))            # of edge axis a: (o1, o2), the two axes that follow a cyclically


def edge_of(e):
    """Cell edge e = 4a + 2v + u -> (axis a, offsets (ox, oy, oz) of its owning corner in the cell)."""
    a, v, u = e >> 2, (e >> 1) & 1, e & 1
    off = [0, 0, 0]
    off[OTHER_AXES[a][0]], off[OTHER_AXES[a][1]] = u, v
    return a, tuple(off)


def _t_of(fa, fb, level):
    with np.errstate(all="ignore"):
        t = ((level - fa).astype(np.float32) / (fb - fa).astype(np.float32)).astype(np.float32)
        t = np.where(t >= 0, t, np.float32(0))
        t = np.where(t > 1, np.float32(1), t)
    bad = ~(np.isfinite(fa) & np.isfinite(fb))
    return np.where(bad, np.float32(0.5), t).astype(np.float32), bad


def hermite(f, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """The crossing axis edges of f [nz, ny, nx] in key order: dict(points fp32 [H, 3], keys int64 [H], nonfinite int)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    nz, ny, nx = f.shape
    level = np.float32(level)
    ins = mr.inside_of(f, level)
    keys = []
    for slot, (dx, dy, dz) in enumerate(AXIS_DIRS):
        k, j, i = np.nonzero(ins[:nz - dz, :ny - dy, :nx - dx] != ins[dz:, dy:, dx:])
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 8 + slot)
    keys = np.sort(np.concatenate(keys))
    p, slot = keys >> 3, keys & 7
    idx = (p % nx, (p // nx) % ny, p // (nx * ny))
    d = np.array(AXIS_DIRS, dtype=np.int64)[slot]
    fa, fb = f[idx[2], idx[1], idx[0]], f[idx[2] + d[:, 2], idx[1] + d[:, 1], idx[0] + d[:, 0]]
    t, bad = _t_of(fa, fb, level)
    zero = np.zeros_like(t)
    points = np.stack([mr.position(origin[c], spacing[c], idx[c], np.where(d[:, c] == 1, t, zero)) for c in range(3)], axis=1)
    return {"points": points.astype(np.float32).reshape(-1, 3), "keys": keys.astype(np.int64), "nonfinite": int(bad.sum())}


def contour(f, level, gradient, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), regularisation=0.1):
    """f [nz, ny, nx], gradient fp32 [H, 3] (or a callable points -> [H, 3]) -> dict(points, keys, nonfinite as hermite(); vertices
    fp32 [V, 3]; cell_keys int64 [V]; triangles int32 [T, 3]; local fp64 [V, 3]: the vertex in its cell's [0, 1]^3;
    report = (clamped, fallback, dropped, 0))."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    nz, ny, nx = f.shape
    dims = (nx, ny, nz)
    level = np.float32(level)
    lam = np.float64(np.float32(regularisation))
    assert np.isfinite(lam) and MIN_REGULARISATION <= lam <= MAX_REGULARISATION, regularisation
    out = hermite(f, level, origin, spacing)
    keys = out["keys"]
    n_h = len(keys)
    g = gradient(out["points"]) if callable(gradient) else gradient
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1, 3)
    assert g.shape[0] == n_h, (g.shape, n_h)
    ins = mr.inside_of(f, level)
    sp = np.array([np.float32(s) for s in spacing], dtype=np.float32).astype(np.float64)

    # Hermite id of every lattice edge (-1: not crossing), per axis
    hid = np.full((3, nz * ny * nx), -1, dtype=np.int64)
    hid[keys & 7, keys >> 3] = np.arange(n_h)
    hid = hid.reshape(3, nz, ny, nx)

    # active cells in increasing cell index
    cnt = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int32)
    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                cnt += ins[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox]
    ck, cj, ci = np.nonzero((cnt > 0) & (cnt < 8))
    cell = (ci, cj, ck)
    n_v = len(ci)
    cell_keys = (ck.astype(np.int64) * ny + cj) * nx + ci

    cross = np.zeros((12, n_v), dtype=bool)
    q = np.zeros((12, n_v, 3), dtype=np.float64)
    ids = np.zeros((12, n_v), dtype=np.int64)
    for e in range(12):
        a, off = edge_of(e)
        o = [cell[c] + off[c] for c in range(3)]
        ids[e] = hid[a, o[2], o[1], o[0]]
        cross[e] = ids[e] >= 0
        d = AXIS_DIRS[a]
        t, _ = _t_of(f[o[2], o[1], o[0]], f[o[2] + d[2], o[1] + d[1], o[0] + d[0]], level)
        for c in range(3):
            q[e, :, c] = t.astype(np.float64) if c == a else float(off[c])
    total = np.zeros((n_v, 3), dtype=np.float64)
    for e in range(12):
        total = total + np.where(cross[e][:, None], q[e], 0.0)
    with np.errstate(all="ignore"):
        m = total / cross.sum(axis=0).astype(np.float64)[:, None]

    lam2 = lam * lam
    a00 = np.full(n_v, lam2); a11 = np.full(n_v, lam2); a22 = np.full(n_v, lam2)
    a01 = np.zeros(n_v); a02 = np.zeros(n_v); a12 = np.zeros(n_v)
    b = [np.zeros(n_v), np.zeros(n_v), np.zeros(n_v)]
    dropped = 0
    with np.errstate(all="ignore"):
        for e in range(12):
            ge = g[np.maximum(ids[e], 0)]
            G = [ge[:, c].astype(np.float64) * sp[c] for c in range(3)]
            s = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
            ok = cross[e] & np.isfinite(ge).all(axis=1) & (s > 0)
            dropped += int((cross[e] & ~ok).sum())
            dlt = [q[e, :, c] - m[:, c] for c in range(3)]
            dot = (G[0] * dlt[0] + G[1] * dlt[1]) + G[2] * dlt[2]

            def term(x):
                return np.where(ok, x / s, 0.0)
            a00 = a00 + term(G[0] * G[0]); a01 = a01 + term(G[0] * G[1]); a02 = a02 + term(G[0] * G[2])
            a11 = a11 + term(G[1] * G[1]); a12 = a12 + term(G[1] * G[2]); a22 = a22 + term(G[2] * G[2])
            for c in range(3):
                b[c] = b[c] + term(G[c] * dot)
        # LDL^T, no square root, no pivoting
        d0 = a00
        l10 = a01 / d0
        l20 = a02 / d0
        d1 = a11 - l10 * a01
        t21 = a12 - l20 * a01
        l21 = t21 / d1
        d2 = (a22 - l20 * a02) - l21 * t21
        y0 = b[0]
        y1 = b[1] - l10 * y0
        y2 = (b[2] - l20 * y0) - l21 * y1
        z0, z1, z2 = y0 / d0, y1 / d1, y2 / d2
        x2 = z2
        x1 = z1 - l21 * x2
        x0 = (z0 - l10 * x1) - l20 * x2
        x = np.stack([m[:, 0] + x0, m[:, 1] + x1, m[:, 2] + x2], axis=1)
    fallback = ~np.isfinite(x).all(axis=1)
    x = np.where(fallback[:, None], m, x)
    clamped = ((x < 0) | (x > 1)).any(axis=1) & ~fallback
    x = np.where(fallback[:, None], x, np.minimum(np.maximum(x, 0.0), 1.0))
    x32 = x.astype(np.float32)
    vertices = np.stack([mr.position(origin[c], spacing[c], cell[c], x32[:, c]) for c in range(3)], axis=1).astype(np.float32).reshape(-1, 3)

    # faces: one quad per crossing edge with four cells around it, in key order
    vid = np.full(nz * ny * nx, -1, dtype=np.int64)
    vid[cell_keys] = np.arange(n_v)
    p, a = keys >> 3, keys & 7
    idx = np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], axis=1)
    ring_axes = np.array(RING_AXES, dtype=np.int64)[a] if n_h else np.zeros((0, 2), dtype=np.int64)
    step = np.array([1, nx, nx * ny], dtype=np.int64)
    nd = np.array(dims, dtype=np.int64)
    rows = np.arange(n_h)
    i1, i2 = idx[rows, ring_axes[:, 0]], idx[rows, ring_axes[:, 1]]
    quad = (i1 >= 1) & (i1 <= nd[ring_axes[:, 0]] - 2) & (i2 >= 1) & (i2 <= nd[ring_axes[:, 1]] - 2)
    pq, s1, s2 = p[quad], step[ring_axes[quad, 0]], step[ring_axes[quad, 1]]
    ring = np.stack([vid[pq - s1 - s2], vid[pq - s2], vid[pq], vid[pq - s1]], axis=1)
    assert (ring >= 0).all()
    owner_in = ins.reshape(-1)[pq]
    ring = np.where(owner_in[:, None], ring, ring[:, ::-1])
    triangles = np.stack([ring[:, [0, 1, 2]], ring[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    out.update(vertices=vertices, cell_keys=cell_keys.astype(np.int64), triangles=triangles, local=x,
               report=(int(clamped.sum()), int(fallback.sum()), dropped, 0))
    return out


def counts_of(result):
    """counts_dev[4] of eonerf_dual_count for a result of contour()."""
    return (len(result["keys"]), len(result["cell_keys"]), len(result["triangles"]), result["nonfinite"])
