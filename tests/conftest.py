import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(ROOT, "tests", "data")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs the HIP path)")


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    def load(name):
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        if "grad_up_seed" in d:
            # the upstream gradient stored as its seed (make_golden.py draws it as N(0,1) in the
            # images' shape from RandomState(seed)): 1 MB of noise would put the file over 1 MiB
            seed = int(d.pop("grad_up_seed"))
            d["grad_up"] = np.random.RandomState(seed).normal(size=d["images"].shape).astype(np.float32)
        return d
    return load


@pytest.fixture(scope="session")
def oracle_mod():
    import build as oracle_build
    oracle_build.build()
    import oracle
    return oracle


@pytest.fixture(scope="session")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    return torch.device("cuda:0")
