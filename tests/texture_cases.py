"""TEST INFRASTRUCTURE ONLY -- the small texture cases shared by the CPU and the GPU tests, built on ortho_restated.make_case's RPCs
and scene frame, and the two analytic scenes.  tie_margin is a CONDITION on them (asserted in tests/test_texture_restated_cpu.py), not
a measurement: no sample of any case lies within 1e-6 px of an image edge, within 1e-6 of min_cos, or within 1e-9 of a weight tie in
BEST -- so two correct implementations decide every sample the same way."""
import numpy as np

import ortho_restated as OR
import texture_restated as TR
from oracle import raygen_oracle as RO

LAT0 = 30.33
MIN_COS = 0.1
SENTINEL = -7.0
#       name: (seed, F, T, K, C, image shapes (h, w) cycled, blocked?, zero gain?, broken faces?)
CASES = {
    "one": (41, 1, 1, 1, 1, [(8, 8)], False, False, False),                               # the smallest everything: one face, 36 texels
    "three": (42, 3, 2, 2, 3, [(12, 9), (32, 24)], True, False, False),                   # an odd last face, non-square images
    "row": (43, 9, 5, 3, 4, [(8, 8), (16, 11), (32, 24)], True, True, True),              # F = 2 * 2^2 + 1: a new row; 600 texels, three blocks
    "cap": (44, 3, 1, 64, 3, [(8, 8)], True, False, False),                               # the K limit of the median
}
ROW_BAD_INDEX, ROW_NAN_VERTEX, ROW_ZERO_AREA = 2, 4, 6                                    # faces of "row" broken by hand


def view_of(rpc, h, w, zone, south, scale, min_alt=-10.0, max_alt=50.0):
    """fp32 [3]: the normalised-scene direction of the centre pixel's ray, from the satellite to the ground (ortho.view_directions)."""
    raw = RO.get_rays([(w - 1) / 2.0], [(h - 1) / 2.0], rpc, min_alt, max_alt, zone, south)[0].astype(np.float64)
    d = raw[3:6] / np.asarray(scale, dtype=np.float32).astype(np.float64)
    return (d / np.linalg.norm(d)).astype(np.float32)


def make_case(name):
    """-> dict(vertices fp32 [V, 3], faces int32 [F, 3], texels, scene_offset, scene_scale, zone, south, rpcs [K], images [K] of fp32
    [h, w, C], shapes int32 [K, 2], gain / bias fp32 [K, C], view_dirs fp32 [K, 3], to_satellite fp64 [K, 3], blocked uint8 [K, n] | None,
    min_cos)."""
    seed, F, T, K, C, shapes, with_blocked, zero_gain, broken = CASES[name]
    rng = np.random.default_rng(seed)
    zone, south, offset = OR.scene_frame(LAT0)
    scale = np.array(OR.SCENE_SCALE, dtype=np.float32)
    V = F + 2
    vertices = np.column_stack([rng.uniform(-0.8, 0.8, V), rng.uniform(-0.8, 0.8, V), rng.uniform(-0.1, 0.1, V)]).astype(np.float32)
    faces = np.zeros((F, 3), dtype=np.int32)
    for f in range(F):
        a, b, c = rng.choice(V, 3, replace=False)
        A, B, Cc = vertices[[a, b, c]].astype(np.float64)
        if np.cross(B - A, Cc - A)[2] < 0:
            b, c = c, b                                              # facing up
        if f % 4 == 3:
            b, c = c, b                                              # ... but every fourth faces down: no image sees it from above
        faces[f] = a, b, c
    if broken:
        faces[ROW_BAD_INDEX, 1] = V                                  # an index outside the mesh
        vertices[faces[ROW_NAN_VERTEX, 0], 2] = np.nan               # (also breaks every other face on that vertex)
        faces[ROW_ZERO_AREA, 2] = faces[ROW_ZERO_AREA, 1]            # no area: a NaN normal
    rpcs, images = [], []
    for k in range(K):
        h, w = shapes[k % len(shapes)]
        rpcs.append(RO.rescale_rpc(RO.synthetic_rpc(seed * 100 + k, lat0=LAT0, lon0=OR.LON0), max(h, w) / 2048.0))
        img = rng.uniform(0.0, 1.0, (h, w, C)).astype(np.float32)
        if k % 2 == 1:
            img[rng.random((h, w)) < 0.1] = np.nan                   # NaN pixels under some taps
        images.append(img)
    gain = rng.uniform(0.5, 1.5, (K, C)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, (K, C)).astype(np.float32)
    if zero_gain:
        gain[K - 1, C - 1] = 0.0
    shp = np.array([im.shape[:2] for im in images], dtype=np.int32)
    view = np.stack([view_of(rpcs[k], shp[k, 0], shp[k, 1], zone, south, scale) for k in range(K)])
    w_, h_, _, _ = TR.layout(F, T)
    blocked = (rng.random((K, w_ * h_)) < 0.2).astype(np.uint8) if with_blocked else None
    return {"vertices": vertices, "faces": faces, "texels": T, "scene_offset": offset, "scene_scale": scale, "zone": zone, "south": south,
            "rpcs": rpcs, "images": images, "shapes": shp, "gain": gain, "bias": bias, "view_dirs": view,
            "to_satellite": TR.to_satellite(view, scale), "blocked": blocked, "min_cos": MIN_COS}


def restate(case, mode, normal=True, angle_weight=True, blocked="case"):
    """samples + bake of a case over the whole atlas -> (samples dict, bake dict with return_all)."""
    s = TR.samples(case["vertices"], case["faces"], case["texels"], case["scene_offset"], case["scene_scale"], case["zone"], case["south"])
    blk = case["blocked"] if isinstance(blocked, str) else blocked
    b = TR.bake(s["lonlatalt"], s["normal"] if normal else None, case["rpcs"], case["images"], case["gain"], case["bias"], case["to_satellite"],
                blk, case["min_cos"], angle_weight, mode, return_all=True)
    return s, b


def tie_margin(case, baked):
    """(px from an image edge, distance of a cosine from min_cos, gap between the two largest distinct weights of a sample): the smallest
    of each over the case; inf where nothing qualifies."""
    edge = cosd = gap = np.inf
    for k, img in enumerate(case["images"]):
        h, w = img.shape[:2]
        cr = baked["colrow"][k]
        cr = cr[np.isfinite(cr).all(axis=1)]
        for v, hi in ((cr[:, 0], w - 1), (cr[:, 1], h - 1)):
            if v.size:
                edge = min(edge, np.abs(v).min(), np.abs(v - hi).min())
    if baked["cos"] is not None:
        c = baked["cos"][np.isfinite(baked["cos"])]
        if c.size:
            cosd = np.abs(c - float(np.float32(case["min_cos"]))).min()
        wk = np.where(baked["weights"] > 0, baked["cos"], -np.inf)
        if wk.shape[0] > 1:
            top = np.sort(wk, axis=0)[-2:]
            with np.errstate(invalid="ignore"):
                d = top[1] - top[0]                                  # (-inf) - (-inf) where no image counts: NaN, left out below
            d = d[np.isfinite(d) & (d != 0)]                         # exactly equal weights are no ambiguity: the smaller k has it
            if d.size:
                gap = d.min()
    return edge, cosd, gap


# ----------------------------------------------------------------------------- analytic scene 1: a tilted, textured plane
PLANE_S = 64
PLANE_GE, PLANE_GN = 7.5e-4, -5.0e-4       # the pattern, per metre (ortho_restated.plane_scene's)
PLANE_SE, PLANE_SN = 0.04, -0.03           # the plane's slope, metres of altitude per metre


def plane_scene(texels=8):
    """Two triangles spanning a tilted plane alt(E, N) = ALT0 + sE (E - E0) + sN (N - N0) carrying f(E, N) = 0.5 + gE (E - E0) + gN (N - N0),
    seen by two synthetic images: pixel (c, r) holds f where its ray meets the plane (the altitude found by fixed-point iteration on
    the localisation).  -> a case dict plus "f" (the pattern as a function of east, north)."""
    zone, south, offset = OR.scene_frame(LAT0)
    scale = np.array([250.0, 250.0, 50.0], dtype=np.float32)
    E0, N0, A0 = (float(v) for v in offset)

    def f(E, N):
        return 0.5 + PLANE_GE * (E - E0) + PLANE_GN * (N - N0)

    def alt(E, N):
        return A0 + PLANE_SE * (E - E0) + PLANE_SN * (N - N0)
    rpcs, images = [], []
    cols, rows = np.meshgrid(np.arange(PLANE_S), np.arange(PLANE_S))
    cols, rows = cols.ravel().astype(np.float64), rows.ravel().astype(np.float64)
    for seed in (1, 2):
        rpc = RO.rescale_rpc(RO.synthetic_rpc(seed, lat0=LAT0, lon0=OR.LON0), PLANE_S / 2048.0)
        a = np.full(cols.size, A0)
        for _ in range(12):                                          # |d alt / d alt| is slope * tan(off-nadir) << 1: converges fast
            lon, lat = RO.localization(rpc, cols, rows, a)
            E, N = RO.utm_forward(lat, lon, zone, south)
            a = alt(E, N)
        rpcs.append(rpc)
        images.append(f(E, N).reshape(PLANE_S, PLANE_S, 1).astype(np.float32))
    xy = np.array([[-0.8, -0.8], [0.8, -0.8], [0.8, 0.8], [-0.8, 0.8]], dtype=np.float32)
    z = ((alt(xy[:, 0].astype(np.float64) * 250.0 + E0, xy[:, 1].astype(np.float64) * 250.0 + N0) - A0) / 50.0).astype(np.float32)
    vertices = np.column_stack([xy, z]).astype(np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    shp = np.array([[PLANE_S, PLANE_S]] * 2, dtype=np.int32)
    view = np.stack([view_of(rpcs[k], PLANE_S, PLANE_S, zone, south, scale) for k in range(2)])
    return {"vertices": vertices, "faces": faces, "texels": texels, "scene_offset": offset, "scene_scale": scale, "zone": zone, "south": south,
            "rpcs": rpcs, "images": images, "shapes": shp, "gain": np.ones((2, 1), dtype=np.float32), "bias": np.zeros((2, 1), dtype=np.float32),
            "view_dirs": view, "to_satellite": TR.to_satellite(view, scale), "blocked": None, "min_cos": MIN_COS, "f": f,
            "min_alt": -10.0, "max_alt": 50.0}


# ----------------------------------------------------------------------------- analytic scene 2: a roof plate over a floor
ROOF_S = 48
ROOF_COLOURS = (0.25, 0.75)
ROOF_TILT = 0.4                            # the altitude term of the column polynomial: about 45 degrees off nadir, east and west
ROOF_BIAS = 1.0 / 1024                     # where the occlusion rays start, in units of the (unit) view direction


def roof_scene(texels=32):
    """A floor (two triangles at z = -0.1) under a smaller roof plate (two triangles at z = +0.3), and two constant images -- 0.25 and
    0.75 in all three channels -- whose satellites look from the east and from the west at about 45 degrees: each sees under one side of the plate.
    -> a case dict; "blocked" is raycast_restated.occluded of the atlas' sample points towards each satellite."""
    zone, south, offset = OR.scene_frame(LAT0)
    scale = np.array(OR.SCENE_SCALE, dtype=np.float32)
    rpcs, images = [], []
    for k, tilt in enumerate((ROOF_TILT, -ROOF_TILT)):
        rpc = RO.synthetic_rpc(7 + k, lat0=LAT0, lon0=OR.LON0)
        rpc["col_num"] = list(rpc["col_num"])
        rpc["col_num"][3] = tilt
        rpcs.append(RO.rescale_rpc(rpc, ROOF_S / 2048.0))
        images.append(np.full((ROOF_S, ROOF_S, 3), ROOF_COLOURS[k], dtype=np.float32))
    fl, rf = 0.6, 0.2
    vertices = np.array([[-fl, -fl, -0.1], [fl, -fl, -0.1], [fl, fl, -0.1], [-fl, fl, -0.1],
                         [-rf, -rf, 0.3], [rf, -rf, 0.3], [rf, rf, 0.3], [-rf, rf, 0.3]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)
    shp = np.array([[ROOF_S, ROOF_S]] * 2, dtype=np.int32)
    view = np.stack([view_of(rpcs[k], ROOF_S, ROOF_S, zone, south, scale) for k in range(2)])
    case = {"vertices": vertices, "faces": faces, "texels": texels, "scene_offset": offset, "scene_scale": scale, "zone": zone, "south": south,
            "rpcs": rpcs, "images": images, "shapes": shp, "gain": np.ones((2, 3), dtype=np.float32), "bias": np.zeros((2, 3), dtype=np.float32),
            "view_dirs": view, "to_satellite": TR.to_satellite(view, scale), "min_cos": MIN_COS, "min_alt": -10.0, "max_alt": 50.0,
            "bounds": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "bias_t": ROOF_BIAS}
    s = TR.samples(vertices, faces, texels, offset, scale, zone, south)
    case["blocked"] = roof_blocked(case, s["xyz"], s["face"], view)
    return case


def roof_blocked(case, xyz, face, view_dirs):
    """uint8 [K, n]: the any-hit answer of the restated ray caster for rays from the sample points against each view direction."""
    import raycast_restated as RC
    lo, hi = case["bounds"]
    n = xyz.shape[0]
    rows = []
    for k in range(len(view_dirs)):
        d = np.tile(-np.asarray(view_dirs[k], dtype=np.float32), (n, 1))
        rows.append(RC.occluded(case["vertices"], case["faces"], lo, hi, xyz, d, skip=face, t_min=case["bias_t"])["occluded"])
    return np.stack(rows).astype(np.uint8)
