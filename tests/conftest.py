import os
import sys

# MKL picks its sgemm code path by CPU model, and the fp32 gradients of the oracle-vs-golden tests amplify that rounding past their
# bounds; the COMPATIBLE branch gives the same bits on every x86 CPU (tests/golden/make_golden.py writes the goldens under it too).
# Read when MKL initialises, so it is set before torch is imported.
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="session")
def golden():
    return load_golden
