"""What the plan tests (eq, mix, delay; host and device) share.  A plain module: import what a test file needs; a test
file that imports `gab` gets the fixture."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def gab():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gpuaudiobench_amd as g
    return g


def dev(a):
    """A device tensor holding a copy of a (which may be read-only or strided)."""
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
