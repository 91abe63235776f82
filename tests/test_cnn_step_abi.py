"""CPU-side checks of what AIRModel(cnn=True) adds below the model: the two entry points air_cnn_bwd_sq
/ air_cnn_num_sq_partials answer argument errors on the host before any HIP call, in the cases air_cnn_bwd does; the
VariableStore keeps every cnn=False offset, puts the six conv variables behind everything else and draws them first from its
one stream.  (What the step computes: tests/test_gpu_cnn_model.py.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import abi_check as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BWD_REQUIRED = ("d_out", "out", "images", "pool1", "pool2", "arg1", "arg2", "k1", "k2", "k3", "workspace",
                "d_k1", "d_b1", "d_k2", "d_b2", "d_k3", "d_b3")
HP = dict(canvas_size=50, windows_size=28, rnn_units=256, vae_latent_dimensions=50, vae_recognition_units=(512, 256),
          vae_generative_units=(256, 512), scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64)


@pytest.fixture(scope="module")
def H():
    return abi.hip()


@pytest.fixture()
def ptr():
    return abi.host_ptr()


def _bwd(H, ptr, B=2, S=50, F=8, **override):
    a = H.CnnBwd()
    for n in BWD_REQUIRED + ("d_images",):
        setattr(a, n, ptr)
    a.B, a.S, a.F = B, S, F
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_partial_count_depends_on_filters_only(H):
    count = H.lib().air_cnn_num_sq_partials
    for F in range(1, 9):
        elements = 25 * F + 50 * F * F + 3 * F                    # the six gradients, as air_cnn_workspace_floats counts them
        assert H.lib().air_cnn_workspace_floats(1, 50, F) == elements
        assert count(F) == (elements + 255) // 256 > 0            # one per 256-thread workgroup of the reduction
    assert count(8) == 14
    assert count(0) == -1 and count(-2) == -1 and count(9) == -2


def test_backward_sq_argument_errors_match_backward(H, ptr):
    sq, bwd = H.lib().air_cnn_bwd_sq, H.lib().air_cnn_bwd
    assert sq(None, ptr, None) == -1
    assert sq(C.byref(_bwd(H, ptr)), None, None) == -1                       # a null sq_partials
    cases = [{n: None} for n in BWD_REQUIRED]
    cases += [dict(B=0), dict(B=-3), dict(S=3), dict(F=0), dict(F=9), dict(S=78), dict(S=129, F=2), dict(S=4096, F=1),
              dict(S=3, F=9)]
    for kw in cases:
        for d_images in (ptr, None):
            a = _bwd(H, ptr, d_images=d_images, **kw)
            want = bwd(C.byref(a), None)
            assert want in (-1, -2), kw
            assert sq(C.byref(a), ptr, None) == want, kw


def _stores(cnn_hp):
    from air.air_model import VariableStore
    return VariableStore(dict(HP), torch.device("cpu"), 0), VariableStore(dict(HP, **cnn_hp), torch.device("cpu"), 0)


def test_store_layout(H):
    from air.cnn import CNN
    plain, conv = _stores(dict(cnn=True, cnn_filters=8))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "store_layout.json")))["default"]
    assert plain.dims["Din"] == plain.dims["D"] == 2500 and conv.dims["Din"] == 1152 and conv.dims["D"] == 2500
    assert tuple(conv.P["lstm_kernel"].shape) == (1152 + 256, 1024)
    assert plain.cnn_names == [] and list(plain.variables) == list(conv.variables)[:-6]
    # the conv variables come last, under the names the op module owns, everything 8-aligned
    names = CNN.variable_names()
    assert list(conv.offsets)[-6:] == names == list(conv.variables)[-6:] == conv.cnn_names
    assert all(off % 8 == 0 for off in conv.offsets.values()) and conv.n % 8 == 0
    assert [tuple(conv.variables[k].shape) for k in names] == [(5, 5, 1, 8), (8,), (5, 5, 8, 8), (8,), (5, 5, 8, 8), (8,)]
    end_of_rest = conv.offsets[names[0]]
    assert all(off < end_of_rest for k, off in conv.offsets.items() if k not in names)
    assert conv.n == end_of_rest + 200 + 8 + 1600 + 8 + 1600 + 8
    assert conv.num_trainable == sum(v.numel() for v in conv.variables.values())
    for views in (conv.gradients, conv.adam_m, conv.adam_v):
        assert list(views)[-6:] == names
    # Wx keeps its row-major shadow beside the panel twin (the data gradient of x.Wx reads it)
    assert plain.wx_exclusive and not conv.wx_exclusive and "Wx" in conv.panel_off
    # the pinned layout of a cnn=False store holds (tests/test_store_layout.py pins all of it), and the order of the entries a
    # cnn=True store shares with it is the same: only lstm_kernel's size, and with it the later offsets, differ
    assert [[k, v] for k, v in plain.offsets.items()] == golden["offsets"] and plain.n == golden["n"]
    assert list(conv.offsets)[:-6] == [k for k, _ in golden["offsets"]]
    small = _stores(dict(cnn=True, cnn_filters=3, canvas_size=21))[1]
    assert small.dims["Din"] == 75 and "Wx" not in small.panel_off          # Din % 4 != 0: no panel


def test_store_initialisation_order(H):
    plain, conv = _stores(dict(cnn=True, cnn_filters=8))
    again = _stores(dict(cnn=True, cnn_filters=8))[1]
    assert torch.equal(conv.params, again.params)
    # cnn=False consumes the stream as before: the first draw is the LSTM kernel
    rng = np.random.RandomState(0)
    lim = np.sqrt(6.0 / (2756 + 1024))
    assert np.array_equal(plain.variables["rnn/kernel"].numpy(), rng.uniform(-lim, lim, (2756, 1024)).astype(np.float32))
    # cnn=True: the three conv kernels first (Glorot-uniform over fan_in = 25 Cin, fan_out = 25 F), then the LSTM kernel
    rng = np.random.RandomState(0)
    for i, cin in ((1, 1), (2, 8), (3, 8)):
        lim = np.sqrt(6.0 / (25 * cin + 25 * 8))
        assert np.array_equal(conv.variables["cnn/conv%d/kernel" % i].numpy(), rng.uniform(-lim, lim, (5, 5, cin, 8)).astype(np.float32))
        assert float(conv.variables["cnn/conv%d/bias" % i].abs().max()) == 0.0
    lim = np.sqrt(6.0 / (1408 + 1024))
    assert np.array_equal(conv.variables["rnn/kernel"].numpy(), rng.uniform(-lim, lim, (1408, 1024)).astype(np.float32))


def test_state_dict_carries_the_conv_variables_and_refuses_a_plain_one(H):
    plain, conv = _stores(dict(cnn=True, cnn_filters=8))
    conv.m.uniform_(-1, 1)
    conv.v.uniform_(0, 1)
    sd = conv.state_dict()
    other = _stores(dict(cnn=True, cnn_filters=8))[1]
    other.initialize(5)
    other.load_state_dict(sd)
    for views in ("variables", "adam_m", "adam_v"):           # (per variable: the alignment pads between them are not state)
        for k, v in getattr(conv, views).items():
            assert torch.equal(v, getattr(other, views)[k]), (views, k)
    before = conv.params.clone()
    with pytest.raises((KeyError, ValueError)):
        conv.load_state_dict(plain.state_dict())
    assert torch.equal(conv.params, before)
    import tf_checkpoint as tfc
    shapes = {k: tuple(v.shape) for k, v in conv.variables.items()}
    tensors = tfc.model_to_tensors(sd, shapes)
    assert "air/cnn/conv2/kernel" in tensors and "air/training/air/cnn/conv2/kernel/Adam_1" in tensors
    assert "air/rnn/rnn/kernel" in tensors and not any(k.startswith("air/rnn/cnn") for k in tensors)
    back = tfc.tensors_to_state_dict(tensors)
    assert set(back) == set(sd)
    assert all(np.array_equal(np.asarray(back[k]).reshape(-1), np.asarray(sd[k]).reshape(-1)) for k in sd)
