"""CPU: the sun sweep's header against the ctypes mirror and the built library, and relight.sun_table against the dataset code."""
import ctypes
import os

import torch

# (elevation, azimuth) of the sweep tests: high, low, grazing, near-north, below the horizon
SUNS = [(80.0, 120.0), (35.0, 200.0), (8.0, 300.0), (60.0, 10.0), (-20.0, 45.0)]


def test_sweep_header_declares_exactly_the_mirrored_symbols_and_the_library_exports_them():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.eonerf_sweep_version.restype = ctypes.c_int
    assert L.eonerf_sweep_version() == 1
    L.eonerf_version.restype = ctypes.c_int
    assert L.eonerf_version() == 502
    # a null context has no layout: the size query answers 0 instead of reading it
    L.eonerf_sun_sweep_workspace_bytes.restype = ctypes.c_size_t
    L.eonerf_sun_sweep_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert L.eonerf_sun_sweep_workspace_bytes(None, 37, 5) == 0


def test_sun_table_is_what_normalize_rays_puts_into_columns_8_to_10():
    from eonerf_code_amd.datasets.satellite import normalize_rays, sun_direction
    from eonerf_code_amd.relight import sun_table
    offset, scale = [4.4e5, 3.35e6, 20.0], [317.25, 291.5, 52.125]      # anisotropic: the direction turns under the normalisation
    rows = torch.zeros(len(SUNS), 11, dtype=torch.float64)
    rows[:, 0:3] = torch.tensor(offset, dtype=torch.float64)
    rows[:, 3:6] = torch.tensor([0.1, -0.2, -0.97], dtype=torch.float64)
    rows[:, 7] = 120.0
    for k, (el, az) in enumerate(SUNS):
        rows[k, 8:11] = torch.tensor(sun_direction(el, az), dtype=torch.float64)      # as load_rays appends it
    want = normalize_rays(rows, offset, scale).to(torch.float32)[:, 8:11]
    got = sun_table([el for el, _ in SUNS], [az for _, az in SUNS], scale, device="cpu")
    assert got.dtype == torch.float32 and got.shape == (len(SUNS), 3)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    assert (got.norm(dim=1) - 1).abs().max().item() < 1e-6
    iso = sun_table([el for el, _ in SUNS], [az for _, az in SUNS], [1.0, 1.0, 1.0], device="cpu")
    assert (got - iso).abs().max().item() > 0.05                          # the anisotropic scale really moved them
    # scalars give one row; a scalar broadcasts against a sequence
    one = sun_table(35.0, 200.0, scale, device="cpu")
    assert one.shape == (1, 3) and torch.equal(one[0], got[1])
    two = sun_table(35.0, [200.0, 10.0], scale, device="cpu")
    assert two.shape == (2, 3) and torch.equal(two[0], got[1])
