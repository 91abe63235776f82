"""CPU-side checks of the stand-alone Concrete and VAE pieces (include/air_hip.h) and of the public modules air.concrete /
air.vae: argument errors are answered on the host before any HIP call, the VAE's variable names are the reference
checkpoint's, and the Python ops refuse CPU tensors and unsupported configurations.  (What the kernels compute:
tests/test_gpu_concrete.py, tests/test_gpu_vae.py.)"""
import ctypes as C
import json
import os

import pytest
import torch

import abi_check as abi


@pytest.fixture(scope="module")
def H():
    return abi.hip()


@pytest.fixture()
def ptr():
    return abi.host_ptr()


def _scalars(H, ptr):
    """(good by value, good device scalar, good per element, stride 2)"""
    return (C.byref(H.Scalar(None, 1.0, 0)), C.byref(H.Scalar(ptr, 0.0, 0)), C.byref(H.Scalar(ptr, 0.0, 1)),
            C.byref(H.Scalar(ptr, 0.0, 2)))


def test_concrete_sample_argument_errors(H, ptr):
    lib = H.lib()
    val, dev, per, bad = _scalars(H, ptr)
    fwd, bwd = lib.air_concrete_sample_fwd, lib.air_concrete_sample_bwd
    assert fwd(None, ptr, val, 1e-9, 0, ptr, ptr, 4, None) == -1
    assert fwd(ptr, None, val, 1e-9, 0, ptr, ptr, 4, None) == -1
    assert fwd(ptr, ptr, None, 1e-9, 0, ptr, ptr, 4, None) == -1
    assert fwd(ptr, ptr, val, 1e-9, 0, None, None, 4, None) == -1          # (one of the two outputs may be absent, not both)
    assert fwd(ptr, ptr, val, 1e-9, 0, ptr, ptr, 0, None) == -1
    assert fwd(ptr, ptr, bad, 1e-9, 0, ptr, ptr, 4, None) == -1
    assert bwd(None, val, ptr, ptr, ptr, 4, None) == -1
    assert bwd(ptr, None, ptr, ptr, ptr, 4, None) == -1
    assert bwd(ptr, val, None, None, ptr, 4, None) == -1
    assert bwd(ptr, val, ptr, ptr, None, 4, None) == -1
    assert bwd(ptr, dev, ptr, ptr, ptr, 0, None) == -1
    assert bwd(ptr, bad, ptr, ptr, ptr, 4, None) == -1


def test_concrete_presigmoid_argument_errors(H, ptr):
    lib = H.lib()
    val, dev, per, bad = _scalars(H, ptr)
    fwd, bwd = lib.air_concrete_presigmoid_fwd, lib.air_concrete_presigmoid_bwd
    for nul in (0, 1, 4):
        args = [ptr, ptr, per, 1e-9, ptr, 4, None]
        args[nul] = None
        assert fwd(*args) == -1, nul
    assert fwd(ptr, ptr, None, 1e-9, ptr, 4, None) == -1
    assert fwd(ptr, ptr, val, 1e-9, ptr, 0, None) == -1
    assert fwd(ptr, ptr, val, 1e-9, ptr, -3, None) == -1
    assert fwd(ptr, ptr, bad, 1e-9, ptr, 4, None) == -1
    assert bwd(None, val, ptr, 4, None) == -1
    assert bwd(ptr, None, ptr, 4, None) == -1
    assert bwd(ptr, val, None, 4, None) == -1
    assert bwd(ptr, val, ptr, 0, None) == -1
    assert bwd(ptr, bad, ptr, 4, None) == -1


def test_concrete_kl_argument_errors(H, ptr):
    lib = H.lib()
    val, dev, per, bad = _scalars(H, ptr)
    fwd, bwd = lib.air_concrete_kl_fwd, lib.air_concrete_kl_bwd
    good = [ptr, val, dev, ptr, per, 1e-9, ptr, 4, None]
    for nul in (0, 1, 2, 3, 4, 6):
        args = list(good)
        args[nul] = None
        assert fwd(*args) == -1, nul
    for pos in (1, 2, 4):
        args = list(good)
        args[pos] = bad
        assert fwd(*args) == -1, pos
    assert fwd(*(good[:7] + [0, None])) == -1
    goodb = [ptr, ptr, per, dev, ptr, val, 1e-9, ptr, ptr, ptr, 4, None]
    for nul in (0, 1, 2, 3, 4, 5):
        args = list(goodb)
        args[nul] = None
        assert bwd(*args) == -1, nul
    for pos in (2, 3, 5):
        args = list(goodb)
        args[pos] = bad
        assert bwd(*args) == -1, pos
    assert bwd(*(goodb[:7] + [None, None, None, 4, None])) == -1               # no output at all
    assert bwd(*(goodb[:10] + [0, None])) == -1
    # a gradient per element of the prior exists only for a per-element prior
    for one_value in (val, dev):
        args = list(goodb)
        args[2] = one_value
        assert bwd(*args) == -1


def test_vae_piece_argument_errors(H, ptr):
    lib = H.lib()
    for nul in range(3):
        args = [None if i == nul else ptr for i in range(3)]
        assert lib.air_sigmoid_bwd(*args, 4, None) == -1, nul
    assert lib.air_sigmoid_bwd(ptr, ptr, ptr, 0, None) == -1
    good = [ptr, ptr, ptr, None, None, ptr, 2, 2, None]                     # (the two incoming gradients are nullable)
    for nul in (0, 1, 2, 5):
        args = list(good)
        args[nul] = None
        assert lib.air_reparam_bwd_plain(*args) == -1, nul
    assert lib.air_reparam_bwd_plain(*(good[:6] + [0, 2, None])) == -1
    assert lib.air_reparam_bwd_plain(*(good[:6] + [2, 0, None])) == -1      # Z = 0


def test_vae_variable_names_are_the_checkpoints(H, golden_dir):
    from air.vae import VAE
    listing = json.load(open(os.path.join(golden_dir, "tf_index_listing.json")))["entries"]
    ref = sorted(k[len("air/rnn/"):] for k in listing if k.startswith("air/rnn/vae/"))
    assert len(ref) == 14
    names = VAE.variable_names((512, 256), (256, 512))
    assert sorted(names) == ref
    assert names[0] == "vae/recognition_1/weights" and names[-1] == "vae/gen_mean/biases"


def test_no_cpu_fallback(H):
    from air import concrete as cc
    from air.vae import vae
    x = torch.zeros(5)
    with pytest.raises(H.AirHipError):
        cc.concrete_binary_sample(x, 1.0, u=x)
    with pytest.raises(H.AirHipError):
        cc.concrete_binary_pre_sigmoid_sample(x, 1.0, u=x)
    with pytest.raises(H.AirHipError):
        cc.concrete_binary_kl_mc_sample(x, -2.0, 1.0, x, 1.0)
    with pytest.raises(H.AirHipError):
        vae(torch.zeros(3, 36), 36, (24, 16), 6, (16, 24), 0.3)


def test_vae_refuses_what_the_library_cannot_do(H):
    from air.vae import VAE
    with pytest.raises(NotImplementedError, match="16"):
        VAE(8, (4,) * 8, 2, (4,) * 7, device="cpu")                         # 8 + 7 + 2 = 17 weight-gradient problems
    with pytest.raises(ValueError, match="activation"):
        VAE(8, (4,), 2, (4,), activation="tanh", device="cpu")
    with pytest.raises(ValueError, match="precision"):
        VAE(8, (4,), 2, (4,), precision="fp16", device="cpu")
    m = VAE(8, (4,) * 7, 2, (4,) * 7, device="cpu")                         # 16 problems: the limit itself is accepted
    assert len(list(m.parameters())) == 32
    assert sorted(m.variables()) == sorted(VAE.variable_names((4,) * 7, (4,) * 7))
