#!/usr/bin/env python3
"""Generate tests/golden/g13_prior.npz by running the REFERENCE's own Python code (/root/reference, read-only) on the CPU in the build
container, in the manner of make_golden_dsm.py.  Never runs on the GPU box: only the .npz output travels.

g13: sat_utils.reproject_dsm_alt_to_satellite_image (sat_utils.py:310-362) and, through SatelliteDataset.load_depth_priors_from_dsm
     called on a stand-in `self`, the altitude -> depth lines datasets/satellite.py:644-653, on the fixtures of
     tests/prior_restated.py; the confidence raster through the same function with other_val_path, as :677 calls it.

Stand-ins supply only what is absent from the container (no arithmetic of the reference is replaced):
  rasterio.open              an object handing back the fixture arrays, their bounds, size and crs;
  pyproj.Transformer         .transform returns the lon / lat that tests/prior_restated.utm_inverse gives for the sample points; they
                             are recorded in the golden as INPUTS (pyproj itself is un-vendored: that step stays unpinned);
  rpcm.RPCModel              attributes from the rpcm dict; .projection delegates to the reference's in-tree
                             sat_utils.rpc_projection_differentiable on fp64 arrays;
  dataset.load_data          hands back the fixture rays.

Usage:  python tests/golden/make_golden_prior.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)          # must precede site-packages: a HuggingFace `datasets` package is installed
sys.path.insert(1, REPO)
sys.path.insert(2, os.path.join(REPO, "tests"))

MAX_BYTES = 200 * 1000


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Missing:
    def __init__(self, *a, **k):
        raise RuntimeError("placeholder for an un-vendored third-party symbol was called")


RASTERS = {}        # path -> (array, bounds, crs)
LONLAT = {}         # crs -> (lons, lats) of the sample points


class _Src:
    def __init__(self, path):
        self.arr, (left, bottom, right, top), crs = RASTERS[path]
        self.bounds = types.SimpleNamespace(left=left, bottom=bottom, right=right, top=top)
        self.height, self.width = self.arr.shape
        self.profile = {"crs": crs}

    def read(self, band):
        assert band == 1
        return self.arr.copy()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _Transformer:
    def __init__(self, crs_src):
        self.crs_src = crs_src

    @classmethod
    def from_crs(cls, crs_src, crs_dst):
        assert crs_dst == "+proj=latlon"
        return cls(crs_src)

    def transform(self, easts, norths):
        lons, lats, e, n = LONLAT[self.crs_src]
        assert np.array_equal(e, easts) and np.array_equal(n, norths)        # the reference built the very sample grid of the restatement
        return lons.copy(), lats.copy()


class _RPCModel:
    def __init__(self, d, dict_format="rpcm"):
        assert dict_format == "rpcm"
        self.__dict__.update(d)

    def projection(self, lon, lat, alt):
        import sat_utils
        return sat_utils.rpc_projection_differentiable(self, np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64),
                                                       np.asarray(alt, dtype=np.float64))


_placeholder("rasterio", open=lambda path, mode="r": _Src(path))
_placeholder("pyproj", Transformer=_Transformer, CRS=types.SimpleNamespace(from_proj4=lambda s: s))
_placeholder("rpcm", RPCModel=_RPCModel)
_placeholder("torchvision", transforms=_placeholder("torchvision.transforms"))
_placeholder("nerfacc", OccGridEstimator=_Missing, rendering=_Missing, render_transmittance_from_density=_Missing,
             accumulate_along_rays=_Missing)
try:
    import PIL  # noqa: F401
except ImportError:
    _placeholder("PIL", Image=_placeholder("PIL.Image"))

import sat_utils  # noqa: E402
from datasets import satellite as ref_sat  # noqa: E402

import prior_restated as R  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in R.GOLDEN_CASES:
            c = R.make_case(name)
            h, w = c["dsm"].shape
            crs = f"+proj=utm +zone={c['zone']}" + (" +south" if c["south"] else "")
            easts, norths, _ = R.sample_points(h, w, c["bounds"])
            lons, lats = R.utm_inverse(easts, norths, c["zone"], c["south"])
            LONLAT[crs] = (lons, lats, easts, norths)
            dsm_path, conf_path = os.path.join(tmp, name + "_dsm.tif"), os.path.join(tmp, name + "_conf.tif")
            open(dsm_path, "w").close()                     # the reference asserts that the paths exist
            RASTERS[dsm_path] = (c["dsm"], c["bounds"], crs)
            if c["values"] is not None:
                open(conf_path, "w").close()
                RASTERS[conf_path] = (c["values"], c["bounds"], crs)
            rpc = _RPCModel(c["rpc"])
            alt = sat_utils.reproject_dsm_alt_to_satellite_image(dsm_path, c["out_h"], c["out_w"], rpc)
            assert alt.dtype == np.float32 and alt.shape == (c["out_h"], c["out_w"])
            # load_depth_priors_from_dsm on a stand-in dataset: the JSON carries the fixture's RPC, load_data its rays
            rays = R.case_rays(c)
            json_path = os.path.join(tmp, name + ".json")
            with open(json_path, "w") as f:
                json.dump({"img": name + ".tif", "height": c["out_h"], "width": c["out_w"], "rpc": c["rpc"]}, f)
            ds = types.SimpleNamespace(json_files=[json_path], cache_dir=None, img_downscale=1, train=True,
                                       scene_offset=torch.tensor([0.0, 0.0, R.Z_OFFSET], dtype=torch.float32),
                                       scene_scale=torch.tensor([1.0, 1.0, R.Z_SCALE], dtype=torch.float32),
                                       load_data=lambda files, verbose=False, rays=rays: (torch.from_numpy(rays), None, None, None, None))
            has_conf = c["values"] is not None
            depths, _ = ref_sat.SatelliteDataset.load_depth_priors_from_dsm(ds, dsm_path, None)
            assert depths.dtype == torch.float32
            out[f"{name}.lon"], out[f"{name}.lat"] = lons, lats
            out[f"{name}.alt"], out[f"{name}.depth"] = alt, depths.numpy()
            if has_conf:
                # the method's confidence branch stops at :679 under this container's torch (np.isnan of a tensor is not a boolean mask
                # there), so the reference's function is called as :677 calls it and :678-679 are re-typed on its numpy result
                conf = sat_utils.reproject_dsm_alt_to_satellite_image(dsm_path, c["out_h"], c["out_w"], rpc, other_val_path=conf_path)
                out[f"{name}.conf_raster"] = conf
                conf = conf.ravel().copy()
                conf[np.isnan(conf)] = -1.0
                out[f"{name}.conf"] = conf
            print(f"  {name}: {int(np.isnan(alt).sum())} empty of {alt.size} pixels, {int((depths < 0).sum())} rays without a prior")
    path = os.path.join(HERE, "g13_prior.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(path)
    print(f"wrote g13_prior.npz, {size} bytes, {len(out)} arrays")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
