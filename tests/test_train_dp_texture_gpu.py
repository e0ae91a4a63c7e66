"""GPU: the launcher's textured mesh (eonerf_code_amd/train_dp.py --mesh_out PATH --mesh_texture FILE): after the mesh is saved rank 0 bakes
the images onto it, writes <PATH stem>.obj / .mtl / .png and prints mesh/texels= and mesh/textured=; the same run without the flag
writes none of the three, prints neither field, and leaves every other line and the PLY as they were.  The scene and the step count are
those of tests/test_train_dp_mesh_dsm_gpu.py."""
import os
import re
import zlib

import numpy as np
import pytest
import torch

import ortho_restated as OR
from oracle import raygen_oracle as RO
from test_train_dp_mesh_dsm_gpu import run

pytestmark = pytest.mark.gpu
RES, IMG, TEXELS = 9, 16, 2


def test_launcher_writes_the_textured_mesh_and_leaves_everything_else_alone(tmp_path):
    rng = np.random.default_rng(4)
    zone, south, offset = OR.scene_frame(30.33)
    rpcs = [RO.rescale_rpc(RO.synthetic_rpc(60 + k, lat0=30.33, lon0=OR.LON0), IMG / 2048.0) for k in range(2)]
    images = [torch.from_numpy(rng.uniform(0.1, 1, (IMG, IMG, 3)).astype(np.float32)) for _ in range(2)]
    src = os.path.join(str(tmp_path), "texture_in.pt")
    torch.save({"images": images, "rpcs": rpcs, "size": [4, 4], "min_alt": -10.0, "max_alt": 50.0, "scene_offset": offset.tolist(),
                "scene_scale": list(OR.SCENE_SCALE), "zone": zone, "south": south}, src)
    ply_a, ply_b = str(tmp_path / "a" / "scene.ply"), str(tmp_path / "b" / "scene.ply")
    mesh_flags = ["--mesh_res", str(RES), "--mesh_level", "0.3"]
    out = run(tmp_path / "with", ["--mesh_out", ply_a, "--mesh_texture", src, "--mesh_texels", str(TEXELS)] + mesh_flags)
    found = re.findall(r"mesh_obj=(\S+) \| mesh/texels=(\d+) \| mesh/textured=(\S+)", out)
    assert len(found) == 1, out
    obj, texels, textured = found[0][0], int(found[0][1]), float(found[0][2])
    print("mesh/texels=%d mesh/textured=%s" % (texels, found[0][2]))
    faces = int(re.search(r"mesh=\S+ \| vertices=\d+ \| faces=(\d+)", out).group(1))
    side = TEXELS + 5
    assert faces > 0 and texels == (faces + 1) // 2 * side * (side + 1) // 2 + faces // 2 * side * (side - 1) // 2       # what the faces own
    assert 0.0 <= textured <= 1.0
    stem = os.path.splitext(ply_a)[0]
    assert obj == stem + ".obj" and out.index("mesh=") < out.index("mesh_obj=")
    for ext in (".obj", ".mtl", ".png"):
        assert os.path.getsize(stem + ext) > 0, ext
    text = open(stem + ".obj").read()
    assert text.count("\nf ") == faces and text.count("\nvt ") == 3 * faces and "# origin" in text and "mtllib scene.mtl" in text
    png = open(stem + ".png", "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    idat = png[png.index(b"IDAT") + 4:png.index(b"IEND") - 8]
    pixels = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    assert (pixels.max() > 0) == (textured > 0)
    # without the flag: none of the three files, neither field, and every line and the PLY as they were
    without = run(tmp_path / "without", ["--mesh_out", ply_b] + mesh_flags)
    assert "mesh/texels" not in without and "mesh/textured" not in without and "mesh_obj" not in without
    for ext in (".obj", ".mtl", ".png"):
        assert not os.path.exists(os.path.splitext(ply_b)[0] + ext)
    assert open(ply_a, "rb").read() == open(ply_b, "rb").read()
    strip = lambda s: [re.sub(r"elapsed_time=\S+|rays/s=\S+", "", ln).replace(ply_a, "PLY").replace(ply_b, "PLY")       # noqa: E731
                       for ln in s.splitlines() if "mesh_obj=" not in ln]
    assert strip(out) == strip(without)
