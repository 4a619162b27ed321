"""pytest config: registers the `gpu` marker; puts the repo root on sys.path.

`-m "not gpu"`: oracle vs golden vectors, host logic, C-ABI symbol export (CPU only).
`-m gpu`     : HIP path vs oracle / golden vectors through the C-ABI (real MI355X).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.fixture(scope="session")
def golden():
    return load_golden


@pytest.fixture(scope="session")
def oracle():
    from oracle import cpu_ref

    cpu_ref.lib()
    return cpu_ref


@pytest.fixture
def golden_lobe_exp(oracle, monkeypatch):
    """The oracle's wavelength-lobe exp pinned to the values recorded with the golden vectors (tests/golden/lobe_exp.npz,
    tools/make_goldens.py::g_lobe_exp).  Float32 exp is not correctly rounded and torch-CPU hands it to MKL, whose code path
    (and last bit) depends on the host CPU; the golden vectors are compared bit for bit.  An exponent not in the table is a KeyError."""
    import torch

    g = load_golden("lobe_exp")
    table = dict(zip(g["x"].view(np.uint32).tolist(), g["exp"].tolist()))

    def exp(x):
        a = np.ascontiguousarray(x.numpy())
        return torch.from_numpy(np.array([table[k] for k in a.reshape(-1).view(np.uint32).tolist()], np.float32).reshape(a.shape))

    monkeypatch.setattr(oracle, "_lobe_exp", exp)
    return oracle
