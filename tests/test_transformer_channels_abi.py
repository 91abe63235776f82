"""CPU-side checks of the multi-channel transformer entry points (air_transformer_nc_fwd, air_transformer_nc_bwd): argument and
limit errors reported on the host before any launch, the Python ops importable and without a CPU fallback.  (That a shape
with more channels than fit the LDS at once is accepted needs a launch: it is
tests/test_gpu_transformer_channels.py::test_more_channels_than_a_workgroup_holds.)"""
import ctypes as C

import pytest
import torch

import abi_check as abi

SIZES = ("B", "T", "Hi", "Wi", "C", "Ho", "Wo")
GOOD = dict(B=3, T=2, Hi=9, Wi=11, C=3, Ho=7, Wo=8)


@pytest.fixture(scope="module")
def H():
    return abi.hip()


@pytest.fixture()
def ptr():
    return abi.host_ptr()


def _sizes(**kw):
    s = dict(GOOD)
    s.update(kw)
    return [s[k] for k in SIZES]


def test_forward_argument_errors(H, ptr):
    lib = H.lib()
    for nul in range(3):                                           # U, theta, out
        args = [None if i == nul else ptr for i in range(3)]
        assert lib.air_transformer_nc_fwd(*args, *_sizes(), None) == -1, nul
    for k in SIZES:
        for v in (0, -1):
            assert lib.air_transformer_nc_fwd(ptr, ptr, ptr, *_sizes(**{k: v}), None) == -1, (k, v)


def test_backward_argument_errors(H, ptr):
    lib = H.lib()
    for nul in range(3):                                           # U, theta, d_out
        args = [None if i == nul else ptr for i in range(3)]
        assert lib.air_transformer_nc_bwd(*args, ptr, ptr, *_sizes(), None) == -1, nul
    assert lib.air_transformer_nc_bwd(ptr, ptr, ptr, None, None, *_sizes(), None) == -1          # both gradients null
    for outs in ((ptr, ptr), (ptr, None), (None, ptr)):
        for k in SIZES:
            for v in (0, -1):
                assert lib.air_transformer_nc_bwd(ptr, ptr, ptr, *outs, *_sizes(**{k: v}), None) == -1, (k, v)


def test_backward_limit_error_when_one_channel_cannot_fit(H, ptr):
    lib = H.lib()
    for outs in ((ptr, ptr), (ptr, None), (None, ptr)):
        for c in (1, 3, 64):
            assert lib.air_transformer_nc_bwd(ptr, ptr, ptr, *outs, *_sizes(Hi=256, Wi=256, C=c), None) == -2
    # an argument error is reported before a limit error
    assert lib.air_transformer_nc_bwd(ptr, ptr, ptr, None, None, *_sizes(Hi=256, Wi=256), None) == -1
    assert lib.air_transformer_nc_bwd(ptr, ptr, ptr, ptr, ptr, *_sizes(Hi=256, Wi=256, T=0), None) == -1


def test_python_ops_are_importable_and_refuse_cpu_tensors(H):
    from air.transformer import batch_transformer, batch_transformer_grad, transformer, transformer_grad  # noqa: F401
    with pytest.raises(H.AirHipError):
        transformer(torch.zeros(1, 5, 5, 3), torch.zeros(1, 6), (3, 3))
    with pytest.raises(H.AirHipError):
        batch_transformer(torch.zeros(1, 5, 5, 3), torch.zeros(1, 2, 6), (3, 3))
    with pytest.raises(H.AirHipError):
        batch_transformer(torch.zeros(1, 5, 5), torch.zeros(1, 2, 6), (3, 3))
