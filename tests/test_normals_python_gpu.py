"""GPU: surface normals through the Python layer (eonerf_code_amd/normals.py).  The rules are pinned at the C ABI
(tests/test_normals_gpu.py); here: that the depth is render_image's, the chunk loop, the occupancy grid, the fp16x3 range retry, the
context a bf16 field runs on, and that neither entry point writes outside the buffers it is given (tests/workspace_guard.py)."""
import ctypes as C
import warnings

import pytest
import torch

import occ_restated as occ
import test_march_python_gpu as tmp_
import test_occ_python_gpu as top
import workspace_guard as wg

pytestmark = pytest.mark.gpu
S, STEP = tmp_.S, tmp_.STEP
SCALE = (6.0, 6.0, 40.0)


def _sat(n=300):
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    rays, ts, _, _, _ = tmp_._batch()
    rays = torch.cat([rays] * 5)[:n].contiguous()        # 300 rays: chunks of 64 and a ragged 44
    assert not bool(rays[:, 6].any())                    # near = 0: the retry draw of the same noise is the first draw
    u = torch.rand(n, S, generator=torch.Generator().manual_seed(4)).cuda()
    return define_satrays_from_tensors(rays, torch.zeros(n, 1, dtype=torch.int64, device="cuda")), u


def _noise(u, chunk):
    return [(u[i:i + chunk], u[i:i + chunk], None) for i in range(0, u.shape[0], chunk)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ("depth", "normal", "normal_raw", "acc"))


def test_depth_is_render_images_chunking_does_not_matter_and_normals_are_unit():
    from eonerf_code_amd.normals import render_normals
    from eonerf_code_amd.sat_rendering import render_image
    from eonerf_code_amd.datasets.satellite import namedtuple_map
    f = tmp_._field()
    sat, u = _sat()
    one, n_one = render_normals(f, None, sat, chunk=256, render_step_size=STEP, scene_scale=SCALE, noise=_noise(u, 256))
    many, n_many = render_normals(f, None, sat, chunk=64, render_step_size=STEP, scene_scale=SCALE, noise=_noise(u, 64))
    assert set(one) == {"depth", "normal", "normal_raw", "acc"}
    assert one["depth"].shape == (300, 1) and one["normal"].shape == (300, 3) and one["normal_raw"].shape == (300, 3) and one["acc"].shape == (300, 1)
    assert n_one == n_many > 0 and _same(one, many)
    assert all(bool(torch.isfinite(v).all()) for v in one.values())
    with torch.no_grad():
        img, n_img = render_image(f, None, sat, None, None, chunk=64, render_step_size=STEP, only_depth=True, eval=True, noise=_noise(u, 64))
    assert torch.equal(_bits(many["depth"]), _bits(img["depth"])) and n_many == n_img
    hit = many["acc"].reshape(-1) > 0
    length = torch.linalg.vector_norm(many["normal"], dim=1)
    assert int(hit.sum()) > 100 and bool(((length[hit] - 1).abs() <= 4 * 2.0 ** -24 * 3).all())      # three squares, a root and a quotient in fp32
    assert bool((many["normal"][~hit] == 0).all())
    raw_len = torch.linalg.vector_norm(many["normal_raw"], dim=1)
    assert bool((raw_len <= many["acc"].reshape(-1) + 1e-4).all()) and bool((many["acc"] <= 1 + 1e-4).all())
    # the scale acts before the normalisation: another frame, another direction; the depth does not move
    cube, _ = render_normals(f, None, sat, chunk=64, render_step_size=STEP, noise=_noise(u, 64))
    assert torch.equal(_bits(cube["depth"]), _bits(many["depth"])) and not torch.equal(cube["normal"], many["normal"])
    # an image-shaped ray set keeps its leading shape
    sat2 = namedtuple_map(lambda t: t.reshape(15, 20, *t.shape[1:]), sat)
    shaped, _ = render_normals(f, None, sat2, chunk=64, render_step_size=STEP, scene_scale=SCALE, noise=_noise(u, 64))
    assert shaped["normal"].shape == (15, 20, 3) and shaped["depth"].shape == (15, 20, 1)
    assert torch.equal(shaped["normal"].reshape(300, 3), many["normal"])


def test_an_all_ones_grid_is_the_identity_and_a_cleared_grid_drops_exactly_the_culled_samples():
    from eonerf_code_amd.datasets.satellite import satrays_to_table
    from eonerf_code_amd.normals import render_normals
    from eonerf_code_amd.occupancy import OccupancyGrid, binaries_from_bits
    f = tmp_._field()
    sat, u = _sat()
    kw = dict(chunk=64, render_step_size=STEP, scene_scale=SCALE, noise=_noise(u, 64), return_samples=True)
    plain, n_plain = render_normals(f, None, sat, **kw)
    ones, n_ones = render_normals(f, OccupancyGrid(5), sat, **kw)
    assert n_ones == n_plain and _same(ones, plain)
    for a, b in zip(ones["samples"], plain["samples"]):
        assert torch.equal(_bits(a), _bits(b))
    ri, t0, t1, sigma, grad = plain["samples"]
    assert ri.shape[0] == n_plain and grad.shape == (n_plain, 3) and int(ri.max()) > 64      # ray indices count over the whole call
    grid = top._slab_grid()
    culled, n_culled = render_normals(f, grid, sat, **kw)
    assert 0 < n_culled < n_plain
    # the rule of include/eonerf_occ.h restated (tests/occ_restated.py) on the ungridded list
    table, _ = satrays_to_table(sat)
    flags = binaries_from_bits(grid.export_bits, grid.resolution).reshape(-1)
    x, y, z = occ.mid_points_torch(table, ri, t0, t1)
    keep = occ.keep_mask_torch(ri, flags[occ.cell_index_torch(x, y, z, grid.resolution)])
    assert int(keep.sum()) == n_culled
    for got, want in zip(culled["samples"][:3], (ri[keep], t0[keep], t1[keep])):
        assert torch.equal(_bits(got), _bits(want))
    # the kept samples are evaluated at the same positions: the same densities and gradients, bit for bit
    assert torch.equal(_bits(culled["samples"][3]), _bits(sigma[keep])) and torch.equal(_bits(culled["samples"][4]), _bits(grad[keep]))
    assert _same(render_normals(f, None, sat, **kw)[0], plain)      # nothing stays on the context


def test_the_range_fallback_warns_switches_for_good_and_equals_the_fp32_context():
    import test_f16x3_range as tfr
    from eonerf_code_amd.normals import density_gradient, render_normals
    sd = tfr._scaled(tfr._state(), **tfr.CASES["activation_overflow"])
    sat, u = _sat(128)
    kw = dict(chunk=64, render_step_size=STEP, scene_scale=SCALE, noise=_noise(u, 64))
    f = tfr._field(sd)
    assert f.eval_precision == "fp16x3"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got, n = render_normals(f, None, sat, **kw)
    assert any("fp16x3" in str(x.message) for x in w), "the switch is announced"
    assert f.eval_precision == "fp32"
    want, n32 = render_normals(tfr._field(sd, eval_precision="fp32"), None, sat, **kw)
    assert n == n32 and _same(got, want) and all(bool(torch.isfinite(v).all()) for v in got.values())
    # density_gradient carries the same guard
    x = (torch.rand(100, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    f2 = tfr._field(sd)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s, g = density_gradient(f2, x)
    assert any("fp16x3" in str(x_.message) for x_ in w) and f2.eval_precision == "fp32"
    s32, g32 = density_gradient(tfr._field(sd, eval_precision="fp32"), x)
    assert torch.equal(_bits(s), _bits(s32)) and torch.equal(_bits(g), _bits(g32)) and s.shape == (100, 1) and g.shape == (100, 3)


def test_a_field_whose_export_precision_is_bf16_runs_on_an_fp32_context():
    from eonerf_code_amd.normals import density_gradient, render_normals
    sat, u = _sat(128)
    kw = dict(chunk=64, render_step_size=STEP, scene_scale=SCALE, noise=_noise(u, 64))
    bf = tmp_._field("bf16", eval_precision="same")
    got, n = render_normals(bf, None, sat, **kw)
    want, n32 = render_normals(tmp_._field("fp32"), None, sat, **kw)
    assert n == n32 and _same(got, want)
    x = (torch.rand(50, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    s, g = density_gradient(bf, x)
    f32 = tmp_._field("fp32").eval()
    s32, g32 = density_gradient(f32, x)
    assert torch.equal(_bits(s), _bits(s32)) and torch.equal(_bits(g), _bits(g32))
    with torch.no_grad():
        assert torch.equal(_bits(s), _bits(f32.query_density(x)))      # the value plane is query_density's
    # the bf16 field's own renders stay where they were
    with torch.no_grad():
        assert bf._native(True)[0] is bf._ctx


def test_density_gradient_takes_no_autograd_and_keeps_the_shape():
    from eonerf_code_amd.normals import density_gradient
    f = tmp_._field()
    x = (torch.rand(4, 5, 3, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda().requires_grad_(True)
    s, g = density_gradient(f, x)
    assert s.shape == (4, 5, 1) and g.shape == (4, 5, 3) and not s.requires_grad and not g.requires_grad
    s0, g0 = density_gradient(f, x[:0].reshape(0, 3))
    assert s0.shape == (0, 1) and g0.shape == (0, 3)


def test_nadir_normals_of_a_field_of_z_alone_are_vertical():
    import test_normals_gpu as tng
    from eonerf_code_amd.normals import nadir_normals
    f = tng.one_axis_field("fp32", 2)
    f.set_n_samples(S)
    normal, slope, aspect = nadir_normals(f, 6, 7, SCALE, chunk=16)
    assert normal.shape == (6, 7, 3) and slope.shape == (6, 7) and aspect.shape == (6, 7)
    hit = torch.linalg.vector_norm(normal, dim=2) > 0
    assert int(hit.sum()) > 0 and bool((normal[..., 0:2] == 0).all())
    assert bool(((slope[hit] == 0) | ((slope[hit] - 180).abs() <= 1e-3)).all()) and bool(torch.isnan(aspect).all())      # no horizontal part: no aspect
    from eonerf_code_amd.normals import slope_aspect
    n = torch.tensor([[1.0, 0.0, 1.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    sl, asp = slope_aspect(n)
    assert sl[:3].tolist() == pytest.approx([45.0, 90.0, 90.0]) and asp[:3].tolist() == pytest.approx([90.0, 180.0, 270.0])
    assert bool(torch.isnan(sl[3])) and bool(torch.isnan(asp[3]))


def test_neither_entry_point_writes_outside_its_buffers():
    import test_normals_gpu as tng
    L, P = tng.L, tng.P
    G = lambda name, nbytes: wg.Guarded(name, nbytes, "cuda")
    for precision in tng.PRECISIONS:
        f = tng.rays_field(precision)
        for R, S_ in ((37, 64), (67, 128)):
            rays, _, u_cam, u_retry, _ = tng.tmg.make_rays(R, S_)
            f.set_n_samples(S_)
            cap = R * (S_ - 1)
            nb = L().eonerf_normals_workspace_bytes(f._ctx, R)
            bufs = [G("workspace", nb), G("out", R * 5 * 4), G("n_samples_dev", 4), G("s_ray", cap * 8), G("s_ts", cap * 4), G("s_te", cap * 4),
                    G("s_sigma", cap * 4), G("s_grad", cap * 12)]
            ptr = [C.c_void_p(b.ptr) for b in bufs]
            axis = (C.c_float * 3)(1.0, 1.0, 0.5)
            rc = L().eonerf_render_normals(f._ctx, P(f._flat), P(rays), P(tng.tog._zsteps(S_)), P(u_cam), P(u_retry), R, axis, ptr[1], ptr[2],
                                           *ptr[3:], ptr[0], nb, None)
            assert rc == 0
            torch.cuda.synchronize()
            wg.check_guards(f"eonerf_render_normals[{precision}-R{R}-S{S_}]", bufs)
        for n in (1, 9, 257):
            x = tng.cube_points()[:n].cuda().contiguous()
            nb = L().eonerf_density_grad_workspace_bytes(f._ctx, n)
            bufs = [G("workspace", nb), G("sigma", n * 4), G("grad", n * 12)]
            rc = L().eonerf_field_density_grad(f._ctx, P(f._flat), P(x), n, C.c_void_p(bufs[1].ptr), C.c_void_p(bufs[2].ptr), C.c_void_p(bufs[0].ptr), nb, None)
            assert rc == 0
            torch.cuda.synchronize()
            wg.check_guards(f"eonerf_field_density_grad[{precision}-n{n}]", bufs)
            assert bool(torch.isfinite(bufs[1].view(torch.float32, n)).all()) and bool(torch.isfinite(bufs[2].view(torch.float32, n, 3)).all())
