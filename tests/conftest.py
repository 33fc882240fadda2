import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "act-plus-plus_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: test needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


@pytest.fixture
def host_only(monkeypatch):
    """Hide the GPU from torch.cuda.is_available() for one test: eval_bc and dist_utils move to the GPU (and RCCL) whenever
    one is visible, while the host-logic tests drive them with CPU test doubles."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
