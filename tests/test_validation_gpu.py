"""GPU: eonerf_code_amd.validation -- image_metrics on render outputs and the validation loop of train_eonerf.py:197-294.

One arithmetic is compared: an fp32 field with eval_precision="same", closed-form filler weights (as the G3 goldens build them), 16
samples per ray, jitter handed in through noise=.  A row of validate_images' table and the restatement (tests/metrics_restated.py)
applied to what render_image returns for the same image see the same fp32 pixels, so only the order of the fp64 summation differs:
n x 2^-53 for n <= 144 terms, held to 1e-10 relative."""
import numpy as np
import pytest
import torch

import metrics_restated as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_IMG, S, EPOCH = 5, 16, 3          # epoch >= 2: the shadow pass is on, as in every validation after the second epoch
STEP = 2.0 / S


@pytest.fixture(scope="module")
def field():
    from oracle import eonerf_oracle as orc
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    sd = orc.closed_form_state_dict(N_IMG)
    sd["sigma_layer.output_layer.bias"] = sd["sigma_layer.output_layer.bias"] + 1.5      # rays end inside the cube, as in G8
    f = EONerfMLP(N_IMG, radiometric_normalization=True, precision="fp32", eval_precision="same")
    f.load_state_dict(sd)
    f = f.cuda().eval()
    f.set_n_samples(S)
    f.flat_params()
    return f


def chunk_noise(n, chunk, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(min(chunk, n - i), S, generator=g), None, torch.rand(min(chunk, n - i), S, generator=g)) for i in range(0, n, chunk)]


def make_images(sizes, seed=31):
    """Synthetic held-out images: JAX_068-like rays and uniform target colours, one jitter set per image."""
    from oracle import eonerf_oracle as orc
    images, noise = [], []
    for k, (h, w) in enumerate(sizes):
        rays, _, rgbs, _, _ = orc.synthetic_batch(h * w, N_IMG, seed=seed + k, n_samples=S)
        images.append({"rays": rays.to(DEV), "rgbs": rgbs.to(DEV), "h": h, "w": w})
        noise.append(chunk_noise(h * w, CHUNK, 100 + k))
    return images, noise


CHUNK = 16
SIZES = [(8, 6), (5, 7), (1, 1)]        # 3 chunks, 2 chunks + a partial one (35 = 2 x 16 + 3), a one-ray image


def render(field, image, noise, index=0, chunk=CHUNK):
    """render_image as validate_images calls it, with image index `index` on every ray."""
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    from eonerf_code_amd.sat_rendering import render_image
    rays = image["rays"]
    ts = torch.full((rays.shape[0], 1), index, dtype=torch.int64, device=DEV)
    assert not field.training
    with torch.no_grad():
        res, _ = render_image(field, None, define_satrays_from_tensors(rays, ts), None, None, epoch_idx=EPOCH, chunk=chunk,
                              render_step_size=STEP, noise=noise)
    return res


def restated_row(res, image):
    return M.image_metrics(res["rgb"].cpu().numpy(), image["rgbs"].cpu().numpy(), res["beta"].cpu().numpy())


@pytest.fixture(scope="module")
def three(field):
    """The three images, their table and means, and the restatement of every row from a render by hand: computed once."""
    from eonerf_code_amd.validation import validate_images
    images, noise = make_images(SIZES)
    table, means = validate_images(field, images, EPOCH, chunk=CHUNK, render_step_size=STEP, noise=noise)
    want = np.stack([restated_row(render(field, im, nz), im) for im, nz in zip(images, noise)])
    return images, noise, table, means, want


def test_image_metrics_reads_the_packed_render_output_in_place(field):
    from eonerf_code_amd.validation import _rows, image_metrics
    images, noise = make_images([(5, 7)])
    res = render(field, images[0], noise[0])
    rgb, beta = res["rgb"], res["beta"]
    assert rgb.stride(0) == 21 and beta.stride(0) == 21                  # column views of the packed [R, 21] output
    t, n, stride = _rows(rgb, 3)
    assert t.data_ptr() == rgb.data_ptr() and (n, stride) == (35, 21)    # no copy
    t, n, stride = _rows(beta, 1)
    assert t.data_ptr() == beta.data_ptr() and (n, stride) == (35, 21)
    got = image_metrics(rgb, images[0]["rgbs"], beta)
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (6,)
    copied = image_metrics(rgb.contiguous(), images[0]["rgbs"], beta.contiguous())
    assert torch.equal(got.view(torch.int64), copied.view(torch.int64))
    # anything else goes through .contiguous(): an [h, w, 3] view, fp64 values, a transposed layout
    shaped = image_metrics(rgb.contiguous().view(5, 7, 3), images[0]["rgbs"].view(5, 7, 3), beta.contiguous().view(5, 7, 1))
    assert torch.equal(shaped.view(torch.int64), got.view(torch.int64))
    transposed = rgb.t().contiguous().t()
    assert transposed.stride(1) != 1
    assert torch.equal(image_metrics(transposed, images[0]["rgbs"].double(), beta).view(torch.int64), got.view(torch.int64))
    want = restated_row(res, images[0])
    assert (np.abs(got.cpu().numpy() - want) <= 1e-10 * np.abs(want)).all()
    nob = image_metrics(rgb, images[0]["rgbs"]).cpu().numpy()
    assert np.isnan(nob[:3]).all() and (nob[3:] == got.cpu().numpy()[3:]).all()


def test_every_row_is_the_restatement_of_its_render(three):
    images, _, table, _, want = three
    assert table.shape == (3, 7) and table.dtype == torch.float64 and table.is_cuda
    got = table.cpu().numpy()
    for i in range(3):
        row = got[i, [0, 1, 2, 3, 4, 6]]
        r = np.abs(row - want[i]) / np.abs(want[i])
        print(f"image {i} ({images[i]['h']}x{images[i]['w']}): {row}, worst relative {r.max():.2e}")
        assert np.isfinite(row).all() and (r <= 1e-10).all()
        assert row[5] == images[i]["h"] * images[i]["w"]
    assert np.isnan(got[:, 5]).all()                                     # no ground truth: no MAE


def test_means_leave_image_zero_out(field, three):
    from eonerf_code_amd.validation import validate_images
    images, noise, table, means, _ = three
    got = table.cpu().numpy()
    assert list(means) == ["loss", "coarse_color", "coarse_logbeta", "mse", "psnr", "mae"]
    for k, name in enumerate(means):
        assert means[name].is_cuda and means[name].dim() == 0 and means[name].dtype == torch.float64
        np.testing.assert_allclose(means[name].item(), (got[1, k] + got[2, k]) / 2, rtol=4e-16, atol=0, equal_nan=True)
    assert abs(means["loss"].item() - got[:, 0].mean()) > 1e-6           # the fixture can tell: image 0 would move the mean
    # a single image is its own mean; max_images cuts the list as the reference's min(5, len(val_dataset)) does
    t1, m1 = validate_images(field, images, EPOCH, chunk=CHUNK, render_step_size=STEP, noise=noise, max_images=1)
    assert t1.shape == (1, 7) and torch.equal(t1.view(torch.int64), table[:1].view(torch.int64))
    for k, name in enumerate(m1):
        np.testing.assert_array_equal(m1[name].item(), got[0, k])


def test_every_image_is_rendered_with_image_index_zero(field, three):
    """The reference's ts = zeros_like quirk: the rows are those of index 0 (the test above); the images' own indices give another
    beta on a field whose transient embedding rows differ."""
    images, noise, table, _, want = three
    emb = field.state_dict()["transient_encoder.weight"]
    assert not torch.equal(emb[0], emb[1]) and not torch.equal(emb[0], emb[2])
    got = table.cpu().numpy()
    for i in (1, 2):
        own = restated_row(render(field, images[i], noise[i], index=i), images[i])
        print(f"image {i}: coarse_logbeta {got[i, 2]:.9f} with index 0, {own[2]:.9f} with index {i}")
        assert abs(own[2] - want[i][2]) > 1e-6 * abs(want[i][2])
        assert abs(got[i, 2] - want[i][2]) <= 1e-10 * abs(want[i][2])


@pytest.mark.parametrize("training", [True, False])
def test_module_mode_and_parameters_are_left_alone(field, three, training):
    from eonerf_code_amd.validation import validate_images
    images, noise, table, _, _ = three
    field.train(training)
    try:
        assert all(p.requires_grad for p in field.parameters())
        versions = [p._version for p in field.parameters()]
        before = field.flat_params().clone()
        again, _ = validate_images(field, images, EPOCH, chunk=CHUNK, render_step_size=STEP, noise=noise)
        assert field.training is training and all(m.training is training for m in field.modules())
        assert all(p.grad is None for p in field.parameters())
        assert [p._version for p in field.parameters()] == versions
        assert torch.equal(before, field.flat_params())
        assert torch.equal(again.view(torch.int64), table.view(torch.int64))        # run-to-run bit-identical, whatever the mode was
    finally:
        field.eval()


def test_image_dsm_mae_is_the_chain_by_hand(field):
    """Two 24 x 24 images of nadir-like rays over the field's near-flat surface, a tilted plane as the lidar DSM: the mae column of
    image i is dsm_mae(register_dsm(rasterize_dsm(...))) on that image's own rays and rendered depth, bit for bit."""
    from eonerf_code_amd import dsm
    from eonerf_code_amd.validation import validate_images
    H, chunk = 24, 256
    scale, offset, roi = (6.0, 6.0, 40.0), (1006.0, 5006.0, 30.0), (1000.0, 5000.0, H, 0.5)
    g = torch.Generator().manual_seed(5)
    images = [{"rays": dsm.nadir_rays(H, H, scale, el, az), "rgbs": torch.rand(H * H, 3, generator=g).to(DEV), "h": H, "w": H}
              for el, az in ((35.0, 160.0), (50.0, 120.0))]
    noise = [chunk_noise(H * H, chunk, 200 + k) for k in range(2)]
    depths = [render(field, im, nz, chunk=chunk)["depth"].reshape(-1) for im, nz in zip(images, noise)]
    surface = dsm.rasterize_dsm(images[0]["rays"], depths[0], offset, scale, roi=roi)
    assert surface.shape == (H, H) and float(torch.isfinite(surface).float().mean()) > 0.9
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
    plane = (float(torch.nanmean(surface)) + 0.4 + 0.05 * xx - 0.03 * yy).to(DEV)
    water = torch.zeros(H, H, dtype=torch.uint8, device=DEV)
    water[15:20, 3:9] = 1
    base = {"dsm": plane, "roi": list(roi), "scene_offset": list(offset), "scene_scale": list(scale)}
    for gt in (base, dict(base, water=water)):
        table, means = validate_images(field, images, EPOCH, chunk=chunk, render_step_size=STEP, gt=gt, noise=noise)
        got = table.cpu().numpy()
        for i in range(2):
            d = dsm.rasterize_dsm(images[i]["rays"], depths[i], offset, scale, roi=roi)
            if "water" in gt:
                d = dsm.mask_water(d, water)
            want = dsm.dsm_mae(plane, d, dsm.register_dsm(plane, d, scaling=False))
            print(f"image {i} (water: {'water' in gt}): mae {got[i, 5]:.9f} m over {int(want[1].item())} cells")
            assert np.isfinite(got[i, 5]) and got[i, 5] > 0
            assert torch.equal(table[i, 5].view(torch.int64), want[0].view(torch.int64))
        assert torch.equal(means["mae"].view(torch.int64), table[1, 5].view(torch.int64))       # image 0 left out
    table, means = validate_images(field, images, EPOCH, chunk=chunk, render_step_size=STEP, noise=noise)
    assert torch.isnan(table[:, 5]).all() and torch.isnan(means["mae"])
    assert torch.equal(table[:, :5].view(torch.int64), torch.from_numpy(got[:, :5].copy()).to(DEV).view(torch.int64))
