import os
import sys

import pytest

# The golden fixtures pin the reference's torch statements bit for bit on the CPU.  MKL's vector math (torch.exp, log, ...)
# picks its code path by CPU vendor and ISA, torch's own kernels by ISA: both are fixed here, before any torch operation,
# to what tests/golden/_ref_harness.py fixes for the generators, so that the pins hold on every x86-64 test host.
os.environ["MKL_CBWR"] = "COMPATIBLE"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "hair-gs_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    import numpy as np
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_pins.npz"), allow_pickle=False)
