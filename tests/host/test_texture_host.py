"""CPU: the texture group's refusals in their documented order, its layout at the limits, its 64-bit size arithmetic and the per-texel
ownership and barycentric functions the kernels call (csrc/eonerf_texture_check.h), checked by the stand-alone program
tests/host/texture_checks.cpp built host-only under the address and undefined-behaviour sanitizers, exactly as
tests/host/test_ortho_host.py builds ortho_checks.cpp, and run as a program.  The per-texel values come from the numpy restatement
(tests/texture_restated.py) through a file and must be reproduced bit for bit."""
import numpy as np

import sanitized
import texture_restated as TR

BLOCKS = ((1, 1), (3, 2), (9, 5), (19, 3), (7, 16), (2, 64), (5, 4))


def test_texture_host_logic_under_asan_ubsan(tmp_path):
    path = tmp_path / "texels.bin"
    with open(path, "wb") as fh:
        for F, T in BLOCKS:
            w, h, _, _ = TR.layout(F, T)
            face, b = TR.texels_of(F, T)
            rec = np.zeros(w * h, dtype=[("face", "<i8"), ("b", "<f8", (3,))])
            rec["face"], rec["b"] = face, b
            fh.write(np.array([F, T, w * h], dtype="<i8").tobytes())
            fh.write(rec.tobytes())
            fh.write(TR.corners(F, T).astype("<f8").tobytes())
    sanitized.run(sanitized.build(tmp_path / "texture_checks", "texture_checks.cpp"), "texture checks ok", args=(str(path),))
