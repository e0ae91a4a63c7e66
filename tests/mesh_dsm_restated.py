"""The rule of include/eonerf_mesh_dsm.h restated in numpy: int64 and fp64, a loop over the triangles, vectorised over each triangle's
box of cells.  Nothing here is shared with the library: the constants are written out again, and every fp64 step is one numpy
operation (numpy does not fuse)."""
import numpy as np

SUB = 4096                  # sub-pixels per cell (12 bits)
HALF = 2048
MAX_COORD = 1 << 29
MAX_ALTITUDE = 32768.0
KEEP, DROPPED, DEGENERATE = 0, 1, 2


def snap(vertices, scale, offset, xoff, yoff, res):
    """vertices fp32 [V, 3] -> (X int64 [V], Y int64 [V], z fp64 [V], ok bool [V])."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    scale, offset = np.asarray(scale, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    with np.errstate(all="ignore"):
        pos = v * scale + offset
        east, north, alt = pos[:, 0], pos[:, 1].copy(), pos[:, 2]
        neg = north < 0
        north[neg] = north[neg] + 10e6
        fx = (east - np.float64(xoff)) / np.float64(res) * np.float64(SUB)
        fy = (np.float64(yoff) - north) / np.float64(res) * np.float64(SUB)
        ok = (np.abs(fx) <= MAX_COORD) & (np.abs(fy) <= MAX_COORD) & (np.abs(alt) < MAX_ALTITUDE)       # all false for a NaN
    X = np.where(ok, np.rint(np.where(ok, fx, 0.0)), 0.0).astype(np.int64)
    Y = np.where(ok, np.rint(np.where(ok, fy, 0.0)), 0.0).astype(np.int64)
    return X, Y, alt, ok


def edge(xa, ya, xb, yb, px, py):
    return (xb - xa) * (py - ya) - (yb - ya) * (px - xa)


def setup(tri, n_vertices, X, Y, z, ok, xsize, ysize):
    """One triangle (three indices) -> dict with "state" and, where it is kept, the vertices, |A2|, the sign and the clamped box."""
    a, b, c = (int(t) for t in tri)
    if min(a, b, c) < 0 or max(a, b, c) >= n_vertices or not (ok[a] and ok[b] and ok[c]):
        return {"state": DROPPED}
    xs, ys = [int(X[k]) for k in (a, b, c)], [int(Y[k]) for k in (a, b, c)]
    a2 = edge(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2])
    if a2 == 0:
        return {"state": DEGENERATE}
    i0, i1 = (min(xs) + HALF - 1) // SUB, (max(xs) - HALF) // SUB           # Python's // is a floor division
    j0, j1 = (min(ys) + HALF - 1) // SUB, (max(ys) - HALF) // SUB
    return {"state": KEEP, "x": xs, "y": ys, "z": [np.float64(z[k]) for k in (a, b, c)], "area": abs(a2), "sign": 1 if a2 > 0 else -1,
            "box": (max(i0, 0), min(i1, xsize - 1), max(j0, 0), min(j1, ysize - 1))}


def weights(t, ii, jj):
    """int64 weights of the three vertices at the centres of the cells (jj, ii), and the coverage mask."""
    px, py = SUB * ii.astype(np.int64) + HALF, SUB * jj.astype(np.int64) + HALF
    x, y, s = t["x"], t["y"], t["sign"]
    w0 = s * edge(x[1], y[1], x[2], y[2], px, py)
    w1 = s * edge(x[2], y[2], x[0], y[0], px, py)
    w2 = s * edge(x[0], y[0], x[1], y[1], px, py)
    return w0, w1, w2, (w0 >= 0) & (w1 >= 0) & (w2 >= 0)


def interpolate(w0, w1, w2, area, a0, a1, a2):
    return ((w0.astype(np.float64) * np.float64(a0) + w1.astype(np.float64) * np.float64(a1)) + w2.astype(np.float64) * np.float64(a2)) / np.float64(area)


def rasterize(vertices, triangles, scale, offset, xoff, yoff, xsize, ysize, res):
    """-> dict: "dsm" fp32 [ysize, xsize] (NaN where empty), "face" int32 (-1 where empty), "counts" int64 [4], "keys" uint64."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    X, Y, z, ok = snap(vertices, scale, offset, xoff, yoff, res)
    keys = np.zeros((ysize, xsize), dtype=np.uint64)
    counts = np.zeros(4, dtype=np.int64)
    for f, tri in enumerate(triangles):
        t = setup(tri, len(vertices), X, Y, z, ok, xsize, ysize)
        counts[t["state"]] += 1
        if t["state"] != KEEP:
            continue
        i0, i1, j0, j1 = t["box"]
        if i1 < i0 or j1 < j0:
            continue
        jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing="ij")
        w0, w1, w2, cov = weights(t, ii, jj)
        zz = interpolate(w0, w1, w2, t["area"], *t["z"])
        q = np.clip(np.rint(zz * np.float64(65536.0)), -2147483648.0, 2147483647.0).astype(np.int64)
        key = ((q + 2147483648).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - f)
        key = np.where(cov, key, np.uint64(0))
        keys[j0:j1 + 1, i0:i1 + 1] = np.maximum(keys[j0:j1 + 1, i0:i1 + 1], key)
    full = keys != 0
    counts[3] = int(full.sum())
    q = (keys >> np.uint64(32)).astype(np.int64) - 2147483648
    dsm = np.where(full, (q.astype(np.float64) / np.float64(65536.0)).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    face = np.where(full, (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64), -1).astype(np.int32)
    return {"dsm": dsm, "face": face, "counts": counts, "keys": keys}


def attributes(vertices, triangles, scale, offset, xoff, yoff, xsize, ysize, res, face, attr):
    """attr fp32 [V, C] at the cell centres through the face raster -> fp32 [ysize, xsize, C]; NaN where the header says so."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    attr = np.asarray(attr, dtype=np.float32).reshape(len(vertices), -1)
    face = np.asarray(face, dtype=np.int32).reshape(ysize, xsize)
    X, Y, z, ok = snap(vertices, scale, offset, xoff, yoff, res)
    out = np.full((ysize, xsize, attr.shape[1]), np.nan, dtype=np.float32)
    for f in np.unique(face):
        if f < 0 or f >= len(triangles):
            continue
        t = setup(triangles[f], len(vertices), X, Y, z, ok, xsize, ysize)
        if t["state"] != KEEP:
            continue
        jj, ii = np.nonzero(face == f)
        w0, w1, w2, cov = weights(t, ii, jj)
        a, b, c = (int(k) for k in triangles[f])
        for ch in range(attr.shape[1]):
            val = interpolate(w0, w1, w2, t["area"], attr[a, ch], attr[b, ch], attr[c, ch]).astype(np.float32)
            out[jj[cov], ii[cov], ch] = val[cov]
    return out
