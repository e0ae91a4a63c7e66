"""CPU: the texture restatement (tests/texture_restated.py) against what it cannot get wrong by construction -- the atlas rule checked tap
by tap, and two analytic scenes -- and the condition on the shared cases (tests/texture_cases.py) that lets the GPU tests ask for exact
counts: no sample near an image edge, near min_cos or near a weight tie."""
import numpy as np
import pytest

import texture_cases as TC
import texture_restated as TR
from oracle import raygen_oracle as RO

TEXELS = (1, 2, 3, 4, 5, 8, 16)


@pytest.mark.parametrize("T", TEXELS)
def test_no_bilinear_tap_inside_a_face_reads_another_face(T):
    """On a dense barycentric lattice with all edges and corners, for the lower and the upper face of an inner cell and of the cells at
    the atlas' rim: every tap of non-zero weight lands inside the atlas on a texel the sampled face owns."""
    F = 2 * 9 + 1                                                    # 10 cells, four to a row: inner cells, rim cells, an odd last face
    w, h, cpr, cells = TR.layout(F, T)
    face, _ = TR.texels_of(F, T)
    face = face.reshape(h, w)
    corner = TR.corners(F, T)
    m = 4 * T + 3                                                    # lattice steps per leg: finer than the texels, no multiple of them
    checked = 0
    for f in range(F):
        A, B, C = corner[f]
        for i in range(m + 1):
            for j in range(m + 1 - i):
                b1, b2 = i / m, j / m
                u, v = A + b1 * (B - A) + b2 * (C - A)
                for x, y, wt in TR.bilinear_taps(u, v, w, h):
                    if wt > 0:
                        assert 0 <= x < w and 0 <= y < h, (T, f, b1, b2, x, y)
                        assert face[y, x] == f, (T, f, b1, b2, x, y)
                        checked += 1
    assert checked >= F * (m + 1) * (m + 2) // 2


@pytest.mark.parametrize("T", TEXELS)
def test_uv_corners_invert_to_barycentric_unit_vectors(T):
    F = 7
    w, h, cpr, cells = TR.layout(F, T)
    S = T + TR.GUTTER
    corner = TR.corners(F, T)
    uv = TR.uv(F, T)
    np.testing.assert_allclose(uv[..., 0] * w, corner[..., 0], rtol=0, atol=w * 6e-8)
    np.testing.assert_allclose((1.0 - uv[..., 1].astype(np.float64)) * h, corner[..., 1], rtol=0, atol=h * 6e-8)
    assert uv.min() >= 0 and uv.max() <= 1
    for f in range(F):
        A, B, C = corner[f]
        for c, P in enumerate((A, B, C)):
            b1 = (P[0] - A[0]) / (B[0] - A[0])                       # the header's expressions
            b2 = (P[1] - A[1]) / (C[1] - A[1])
            np.testing.assert_array_equal([1 - b1 - b2, b1, b2], np.eye(3)[c])
        # the texel whose centre is the corner carries exactly that corner
        face, b = TR.texels_of(F, T)
        for c, P in enumerate((A, B, C)):
            t = int(P[1] - 0.5) * w + int(P[0] - 0.5)
            assert face[t] == f
            np.testing.assert_array_equal(b[t], np.eye(3)[c])
        # both faces of a cell lie inside it
        j = f // 2
        x0, y0 = (j % cpr) * S, (j // cpr) * S
        assert (corner[f, :, 0] > x0 + 1).all() and (corner[f, :, 0] < x0 + S - 1).all()
        assert (corner[f, :, 1] > y0 + 1).all() and (corner[f, :, 1] < y0 + S - 1).all()


@pytest.mark.parametrize("F", [1, 2, 3, 2 * 3 * 3 + 1])
def test_face_counts_ownership_and_clamped_weights(F):
    T = 3
    S = T + TR.GUTTER
    w, h, cpr, cells = TR.layout(F, T)
    assert cells == (F + 1) // 2 and (cpr - 1) ** 2 < cells <= cpr ** 2
    assert w == cpr * S and h == -(-cells // cpr) * S
    if F == 19:
        assert cpr == 4 and h == 3 * S                               # 10 cells: one more than 3 x 3, a new row
    face, b = TR.texels_of(F, T)
    owned = face >= 0
    # every face owns the texels of its half cell: S (S + 1) / 2 for a lower, S (S - 1) / 2 for an upper one
    counts = np.bincount(face[owned], minlength=F)
    assert (counts[0::2] == S * (S + 1) // 2).all() and (counts[1::2] == S * (S - 1) // 2).all()
    assert (~owned).sum() == w * h - counts.sum()
    assert np.isnan(b[~owned]).all()
    assert (b[owned] >= 0).all() and np.abs(b[owned].sum(axis=1) - 1).max() <= 2.3e-16
    # inside the triangle the clamp changes nothing: the weights are the header's quotients
    lower = owned & (face % 2 == 0)
    t = np.nonzero(lower)[0]
    cx, cy = (t % w) % S, (t // w) % S
    inside = (cx >= 1) & (cy >= 1) & (cx + cy <= T + 2)
    np.testing.assert_allclose(b[t[inside], 1], (cx[inside] - 1) / T, rtol=0, atol=1e-15)
    np.testing.assert_allclose(b[t[inside], 2], (cy[inside] - 1) / T, rtol=0, atol=1e-15)
    # chunks see the same texels
    f2, b2 = TR.texels_of(F, T, first=5, n=min(40, w * h - 5))
    np.testing.assert_array_equal(f2, face[5:5 + len(f2)])
    np.testing.assert_array_equal(b2, b[5:5 + len(f2)])


def test_layout_limits():
    assert TR.layout(0, 4) == (0, 0, 0, 0)
    assert TR.layout(2 * 3276 * 3276, 5)[:3] == (32760, 32760, 3276)
    assert TR.layout(2 * 3276 * 3276 + 1, 5) is None and TR.layout((1 << 31) - 1, 1) is None


@pytest.mark.parametrize("name", list(TC.CASES))
def test_no_case_sits_on_a_decision(name):
    c = TC.make_case(name)
    for angle_weight in (True, False):
        _, b = TC.restate(c, TR.BEST, angle_weight=angle_weight)
        edge, cosd, gap = TC.tie_margin(c, b)
        print(name, edge, cosd, gap)
        assert edge > 1e-6 and cosd > 1e-6 and gap > 1e-9
    assert (b["count"] > 0).any()
    if c["blocked"] is not None:
        assert (TC.restate(c, TR.BEST, blocked=None)[1]["count"] != b["count"]).any()          # the occlusion table matters


def test_a_tilted_textured_plane_is_reproduced():
    """Analytic scene 1.  The atlas holds f at each texel's ground point within 1e-6, the bound tests/test_ortho_gpu.py derives for
    values: the images are samples of f through a near-affine map, so their bilinear interpolation errs by the map's curvature across
    one pixel (about 1e-8 here) plus the images' fp32 rounding (6e-8)."""
    p = TC.plane_scene()
    for mode in (TR.MEAN, TR.MEDIAN, TR.BEST):
        s, b = TC.restate(p, mode)
        owned = s["face"] >= 0
        assert owned.all() and (b["count"] == 2).all()               # two faces fill their one cell; both images see all of it
        lla = s["lonlatalt"]
        E, N = RO.utm_forward(lla[:, 1], lla[:, 0], p["zone"], p["south"])
        err = np.abs(b["colour"][:, 0].astype(np.float64) - p["f"](E, N)).max()
        print("tilted plane, mode", mode, err)
        assert err <= 1e-6
    # the ground points are the plane's: xyz in the metric frame, and a normal that is the plane's
    xyz = s["xyz64"] * p["scene_scale"].astype(np.float64) + p["scene_offset"].astype(np.float64)
    assert np.abs(E - xyz[:, 0]).max() < 1e-6 and np.abs(N - xyz[:, 1]).max() < 1e-6
    n = np.array([-TC.PLANE_SE, -TC.PLANE_SN, 1.0])
    np.testing.assert_allclose(s["normal64"], np.tile(n / np.linalg.norm(n), (len(E), 1)), rtol=0, atol=1e-6)       # fp32 vertices


def test_floor_texels_under_a_roof_take_the_image_that_looks_under_it():
    """Analytic scene 2: with the restated ray caster's occlusion table, a floor texel that the plate hides from one satellite has the
    other image's colour alone; one hidden from both has none; the rest of the floor has the mean of both."""
    r = TC.roof_scene()
    s, b = TC.restate(r, TR.MEAN, angle_weight=False)
    blk = r["blocked"]
    floor, roof = (s["face"] == 0) | (s["face"] == 1), s["face"] >= 2
    assert not blk[:, roof].any()                                    # nothing is above the plate
    lo, hi = TC.ROOF_COLOURS
    for k, other in ((0, hi), (1, lo)):
        only = floor & (blk[k] == 1) & (blk[1 - k] == 0)
        assert only.sum() >= 20
        assert (b["count"][only] == 1).all() and (b["best"][only] == 1 - k).all()
        np.testing.assert_array_equal(b["colour"][only], np.float32(other))
        # the satellite looks from the side the texel is hidden from: image 0 from the west (its to_satellite points west) hides the east
        side = np.sign(r["to_satellite"][k, 0])
        assert (np.sign(s["xyz"][only, 0]) == -side).all()
    both = floor & (blk[0] == 1) & (blk[1] == 1)
    assert both.sum() >= 20 and (b["count"][both] == 0).all() and np.isnan(b["colour"][both]).all() and (b["best"][both] == -1).all()
    free = floor & (blk[0] == 0) & (blk[1] == 0)
    assert free.sum() >= 100 and (b["count"][free] == 2).all()
    np.testing.assert_allclose(b["colour"][free], 0.5 * (lo + hi), rtol=0, atol=6e-8)
    # without the table the plate's shadow is gone
    assert (TC.restate(r, TR.MEAN, angle_weight=False, blocked=None)[1]["count"][floor] == 2).all()


def test_angle_weight_changes_a_mean_by_the_closed_form():
    r = TC.roof_scene(texels=4)
    s, flat = TC.restate(r, TR.MEAN, angle_weight=False, blocked=None)
    _, steep = TC.restate(r, TR.MEAN, angle_weight=True, blocked=None)
    owned = s["face"] >= 0
    cos = r["to_satellite"][:, 2]                                    # every face is horizontal: cos is the satellites' up component
    assert (cos > TC.MIN_COS).all() and abs(cos[0] - cos[1]) > 1e-3
    lo, hi = TC.ROOF_COLOURS
    c32 = cos.astype(np.float32).astype(np.float64)
    want = (c32[0] * lo + c32[1] * hi) / (c32[0] + c32[1])
    np.testing.assert_allclose(flat["colour"][owned], 0.5 * (lo + hi), rtol=0, atol=6e-8)
    np.testing.assert_allclose(steep["colour"][owned], want, rtol=0, atol=6e-8)
    np.testing.assert_allclose(steep["weight"][owned], c32.sum(), rtol=1.2e-7, atol=0)
    assert (steep["best"][owned] == int(np.argmax(c32))).all() and (flat["best"][owned] == 0).all()
    # an image below min_cos does not count at all
    _, cut = TC.restate(dict(r, min_cos=float(c32.min()) + 1e-3), TR.MEAN, angle_weight=True, blocked=None)
    assert (cut["count"][owned] == 1).all() and (cut["best"][owned] == int(np.argmax(c32))).all()
