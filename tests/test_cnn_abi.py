"""CPU-side checks of the stand-alone CNN front-end (include/air_hip.h, air/cnn.py): argument errors are answered on the host
before any HIP call, the module's variables carry tf.layers.conv2d's names, and the Python op refuses CPU tensors and sizes
the library cannot hold.  (What the kernels compute: tests/test_gpu_cnn.py.)"""
import ctypes as C

import pytest
import torch

import abi_check as abi

FWD_REQUIRED = ("images", "k1", "b1", "k2", "b2", "k3", "b3", "out")
FWD_SAVED = ("pool1", "pool2", "arg1", "arg2")
BWD_REQUIRED = ("d_out", "out", "images", "pool1", "pool2", "arg1", "arg2", "k1", "k2", "k3", "workspace",
                "d_k1", "d_b1", "d_k2", "d_b2", "d_k3", "d_b3")


@pytest.fixture(scope="module")
def H():
    return abi.hip()


@pytest.fixture()
def ptr():
    return abi.host_ptr()


def _fwd(H, ptr, B=2, S=50, F=8, saved=True, **override):
    a = H.CnnFwd()
    for n in FWD_REQUIRED + (FWD_SAVED if saved else ()):
        setattr(a, n, ptr)
    a.B, a.S, a.F = B, S, F
    for k, v in override.items():
        setattr(a, k, v)
    return a


def _bwd(H, ptr, B=2, S=50, F=8, **override):
    a = H.CnnBwd()
    for n in BWD_REQUIRED + ("d_images",):
        setattr(a, n, ptr)
    a.B, a.S, a.F = B, S, F
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_forward_argument_errors(H, ptr):
    fwd = H.lib().air_cnn_fwd
    assert fwd(None, None) == -1
    for n in FWD_REQUIRED:
        assert fwd(C.byref(_fwd(H, ptr, **{n: None})), None) == -1, n
        assert fwd(C.byref(_fwd(H, ptr, saved=False, **{n: None})), None) == -1, n
    for n in FWD_SAVED:                                                  # the saved tensors: all four or none
        assert fwd(C.byref(_fwd(H, ptr, **{n: None})), None) == -1, n
        assert fwd(C.byref(_fwd(H, ptr, saved=False, **{n: ptr})), None) == -1, n
    for saved in (True, False):
        assert fwd(C.byref(_fwd(H, ptr, B=0, saved=saved)), None) == -1
        assert fwd(C.byref(_fwd(H, ptr, B=-3, saved=saved)), None) == -1
        assert fwd(C.byref(_fwd(H, ptr, S=3, saved=saved)), None) == -1
        assert fwd(C.byref(_fwd(H, ptr, F=0, saved=saved)), None) == -1
        assert fwd(C.byref(_fwd(H, ptr, F=9, saved=saved)), None) == -2
        assert fwd(C.byref(_fwd(H, ptr, S=78, saved=saved)), None) == -2   # 77 is the last canvas that fits at 8 filters
        assert fwd(C.byref(_fwd(H, ptr, S=129, F=1, saved=saved)), None) == -2
        assert fwd(C.byref(_fwd(H, ptr, S=4096, F=1, saved=saved)), None) == -2
    assert fwd(C.byref(_fwd(H, ptr, S=3, F=9)), None) == -1              # an invalid size is reported before a limit


def test_backward_argument_errors(H, ptr):
    bwd = H.lib().air_cnn_bwd
    assert bwd(None, None) == -1
    for n in BWD_REQUIRED:
        assert bwd(C.byref(_bwd(H, ptr, **{n: None})), None) == -1, n
        assert bwd(C.byref(_bwd(H, ptr, d_images=None, **{n: None})), None) == -1, n
    assert bwd(C.byref(_bwd(H, ptr, B=0)), None) == -1
    assert bwd(C.byref(_bwd(H, ptr, S=3)), None) == -1
    assert bwd(C.byref(_bwd(H, ptr, F=0)), None) == -1
    assert bwd(C.byref(_bwd(H, ptr, F=9)), None) == -2
    assert bwd(C.byref(_bwd(H, ptr, S=78)), None) == -2
    assert bwd(C.byref(_bwd(H, ptr, S=129, F=2)), None) == -2


def test_workspace_query_and_limits_agree(H):
    ws = H.lib().air_cnn_workspace_floats
    assert ws(64, 50, 8) == 64 * (25 * 8 + 50 * 64 + 3 * 8)
    assert ws(1, 4, 1) == 25 + 50 + 3
    assert ws(0, 50, 8) == -1 and ws(1, 3, 8) == -1 and ws(1, 50, 0) == -1
    assert ws(1, 50, 9) == -2 and ws(1, 129, 1) == -2
    # S from 4 to at least 64 and F from 1 to 8 are served; the stated last canvas per filter count
    for F in range(1, 9):
        for S in (4, 5, 50, 64):
            assert ws(3, S, F) > 0, (S, F)
    last = {8: 77, 7: 83, 6: 89, 5: 97, 4: 107, 3: 118, 2: 128, 1: 128}
    for F, S in last.items():
        assert ws(1, S, F) > 0 and ws(1, S + 1, F) == -2, (F, S)


def test_variable_names_and_output_dim(H):
    from air.cnn import CNN
    assert CNN.variable_names() == ["cnn/conv1/kernel", "cnn/conv1/bias", "cnn/conv2/kernel", "cnn/conv2/bias",
                                    "cnn/conv3/kernel", "cnn/conv3/bias"]
    m = CNN(device="cpu")
    assert m.output_dim == 1152 and m.canvas_size == 50 and m.filters == 8
    v = m.variables()
    assert list(v) == CNN.variable_names()
    assert [tuple(t.shape) for t in v.values()] == [(5, 5, 1, 8), (8,), (5, 5, 8, 8), (8,), (5, 5, 8, 8), (8,)]
    # Glorot-uniform over fan_in = 25 Cin, fan_out = 25 F; zero biases; the seed decides the values
    for i, cin in ((1, 1), (2, 8), (3, 8)):
        k, lim = v["cnn/conv%d/kernel" % i], (6.0 / (25 * cin + 25 * 8)) ** 0.5
        assert float(k.abs().max()) <= lim and float(k.abs().max()) > 0.8 * lim
        assert float(v["cnn/conv%d/bias" % i].abs().max()) == 0.0
    assert torch.equal(CNN(device="cpu", seed=3).k2, CNN(device="cpu", seed=3).k2)
    assert not torch.equal(CNN(device="cpu", seed=3).k2, CNN(device="cpu", seed=4).k2)
    assert CNN(13, 3, device="cpu").output_dim == 27


def test_load_variables_is_all_or_nothing(H):
    from air.cnn import CNN
    a, b = CNN(9, 3, device="cpu", seed=1), CNN(9, 3, device="cpu", seed=2)
    before = b.k1.detach().clone()
    src = dict(a.variables())
    del src["cnn/conv3/bias"]
    with pytest.raises(KeyError):
        b.load_variables(src)
    assert torch.equal(b.k1.detach(), before)
    b.load_variables({"air/" + k: v for k, v in a.variables().items()}, scope="air")
    assert all(torch.equal(x, y) for x, y in zip(a.variables().values(), b.variables().values()))


def test_no_cpu_fallback_and_refused_sizes(H):
    from air.cnn import CNN, cnn
    with pytest.raises(H.AirHipError):
        cnn(torch.zeros(2, 2500))
    with pytest.raises(H.AirHipError):
        CNN(device="cpu")(torch.zeros(2, 2500))
    with pytest.raises(NotImplementedError, match="200.*8"):
        CNN(200, 8, device="cpu")
    with pytest.raises(NotImplementedError, match="50.*9"):
        CNN(50, 9, device="cpu")
    with pytest.raises(ValueError):
        CNN(3, 8, device="cpu")
