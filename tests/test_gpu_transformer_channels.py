"""GPU tests of the spatial transformer on multi-channel inputs and of batch_transformer (air_transformer_nc_fwd /
air_transformer_nc_bwd, air/transformer.py).  Every reference is oracle.air_oracle applied per channel plane:
   * forward: channel c is the single-channel transformer of plane c -- bit for bit against the product's own
     air_transformer_fwd on every row and against the oracle on the rows without shear, 1e-6 on the sheared rows (as
     tests/test_gpu_kernels.py::test_transformer_generic_matches_oracle explains);
   * d U: bit for bit against oracle.transformer_backward on plane c; with T transforms per image the fp32 sum of the rows'
     gradients in ascending t (the descending order gives other bits: asserted below);
   * d theta: |got - sum_c d_theta64_c| <= 2e-5 * sum_c max|d_theta32_c| per row -- the single-channel band of
     test_transformer_bwd_generic_matches_oracle carried across the channels by the triangle inequality (d_theta64_c: the
     oracle in float64 on plane c, d_theta32_c: in float32).  A numpy model of the kernel's arithmetic with the contraction
     as one sequential fp32 chain stays within 0.19 of that band on these shapes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import abi_check as abi

pytestmark = pytest.mark.gpu

from oracle import air_oracle as ao  # noqa: E402

f32 = np.float32
#          Hi  Wi  Ho  Wo  C
SHAPES = [(9, 11, 7, 8, 3),          # non-square, fewer than 64 output pixels, odd C
          (28, 28, 50, 50, 4),       # 16-byte path
          (50, 50, 28, 28, 5),       # scalar path, Ho*Wo not a multiple of 64, a second channel group of one
          (50, 50, 28, 28, 12),      # three channel groups
          (16, 16, 12, 12, 1),       # the new entry points at C = 1
          (128, 128, 12, 12, 3)]     # two planes fit the LDS: groups of 2 + 1
BATCH_SHAPES = [(9, 11, 7, 8, 3), (28, 28, 50, 50, 4)]


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(*arrays):
    return tuple(torch.tensor(np.ascontiguousarray(a), device="cuda") for a in arrays)


@functools.lru_cache(maxsize=None)
def _case(Hi, Wi, Ho, Wo, Ch, B=3, T=1):
    """Inputs as in test_transformer_bwd_generic_matches_oracle and their per-plane oracle results (computed once, read-only)."""
    rng = np.random.RandomState(Hi * 7 + Wo + 13 * Ch + 101 * T)
    R = B * T
    U = rng.uniform(0, 1, (B, Hi, Wi, Ch)).astype(f32)
    base = np.array([[0.55, 0.25, 0.3], [-0.2, 0.6, -0.4]], f32)
    th = (np.tile(base, (R, 1, 1)) + rng.randn(R, 2, 3).astype(f32) * 0.15).astype(f32)
    th[0] = [[1.6, 0.0, 0.9], [0.0, 1.6, -0.9]]              # mostly out of range: border slots collect long chains
    d = (rng.randn(R, Ho, Wo, Ch) * np.where(rng.uniform(size=(R, Ho, Wo, Ch)) < 0.1, 1e6, 1.0)).astype(f32)
    Urep = np.repeat(U, T, axis=0)                           # row b*T+t samples image b
    out = np.empty((R, Ho, Wo, Ch), f32)
    dU_rows = np.empty((R, Hi, Wi, Ch), f32)
    dth64, band = np.zeros((R, 2, 3)), np.zeros((R, 1, 1))
    for c in range(Ch):
        Uc, dc = np.ascontiguousarray(Urep[..., c]), np.ascontiguousarray(d[..., c])
        out[..., c] = ao.transformer(Uc, th, (Ho, Wo))
        dU_rows[..., c], t32 = ao.transformer_backward(Uc, th, (Ho, Wo), dc)
        dth64 += ao.transformer_backward(Uc.astype(np.float64), th.astype(np.float64), (Ho, Wo), dc.astype(np.float64))[1]
        band += 2e-5 * np.abs(t32).max(axis=(1, 2), keepdims=True)
    # the gradient of the tf.gather replication: the rows of an image summed left to right in fp32
    rows = dU_rows.reshape(B, T, Hi, Wi, Ch)
    asc, desc = rows[:, 0].copy(), rows[:, T - 1].copy()
    for t in range(1, T):
        asc = asc + rows[:, t]
        desc = desc + rows[:, T - 1 - t]
    res = dict(U=U, th=th, d=d, out=out, dU=asc, dU_desc=desc, dth64=dth64, band=band)
    for v in res.values():
        v.setflags(write=False)
    return res


def _check_dtheta(got, case):
    got = got.cpu().numpy().reshape(case["dth64"].shape).astype(np.float64)
    err = np.abs(got - case["dth64"])
    print("d_theta: max |err| / band = %.3f" % (err / case["band"]).max())
    assert (err <= case["band"]).all(), (err / case["band"]).max()


def _planes_fwd(H, Ut, tht, Ho, Wo):
    """the product's single-channel air_transformer_fwd on every channel plane of Ut [R,Hi,Wi,C] -> [R,Ho,Wo,C]"""
    R, Hi, Wi, Ch = Ut.shape
    outs = []
    for c in range(Ch):
        plane, o = Ut[..., c].contiguous(), torch.empty(R, Ho, Wo, device="cuda")
        H.check(H.lib().air_transformer_fwd(_p(plane), _p(tht), _p(o), R, Hi, Wi, Ho, Wo, _stream()))
        outs.append(o)
    return torch.stack(outs, dim=3)


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,Ch", SHAPES + [(5, 5, 1, 3, 2)])         # (the last: the Ho == 1 meshgrid branch)
def test_forward_matches_oracle_and_single_channel_kernel_per_plane(H, Hi, Wi, Ho, Wo, Ch):
    from air.transformer import transformer
    case = _case(Hi, Wi, Ho, Wo, Ch)
    Ut, tht = _cuda(case["U"], case["th"])
    got_t = transformer(Ut, tht, (Ho, Wo))
    assert got_t.shape == (3, Ho, Wo, Ch)
    assert torch.equal(got_t, _planes_fwd(H, Ut, tht, Ho, Wo))                 # every row, every channel
    got, ref = got_t.cpu().numpy(), case["out"]
    plain = (case["th"][:, 0, 1] == 0) & (case["th"][:, 1, 0] == 0)             # the rows without shear
    assert plain[0] and not plain[1:].any()
    diff = np.abs(got - ref)
    print("forward: max |diff| without shear %.3g, with shear %.3g" % (diff[plain].max(), diff[~plain].max()))
    assert np.array_equal(got[plain], ref[plain])
    assert diff[~plain].max() <= 1e-6


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,Ch", SHAPES)
def test_backward_matches_oracle_per_plane(H, Hi, Wi, Ho, Wo, Ch):
    from air.transformer import transformer_grad
    case = _case(Hi, Wi, Ho, Wo, Ch)
    Ut, tht, dt = _cuda(case["U"], case["th"], case["d"])
    if Ch == 1:                                      # (the Python op keeps one channel on the single-channel entry points)
        dU, dth = torch.empty_like(Ut), torch.empty(3, 6, device="cuda")
        H.check(H.lib().air_transformer_nc_bwd(_p(Ut), _p(tht), _p(dt), _p(dU), _p(dth), 3, 1, Hi, Wi, 1, Ho, Wo, _stream()))
    else:
        dU, dth = transformer_grad(Ut, tht, (Ho, Wo), dt)
    torch.cuda.synchronize()
    assert dU.shape == (3, Hi, Wi, Ch) and dth.shape == (3, 6)
    assert np.array_equal(dU.cpu().numpy(), case["dU"])
    _check_dtheta(dth, case)
    # either gradient alone: the same bits
    for need_dU, need_dth in ((True, False), (False, True)):
        a = torch.empty_like(Ut) if need_dU else None
        b = torch.empty(3, 6, device="cuda") if need_dth else None
        H.check(H.lib().air_transformer_nc_bwd(_p(Ut), _p(tht), _p(dt), _p(a), _p(b), 3, 1, Hi, Wi, Ch, Ho, Wo, _stream()))
        assert (a is None or torch.equal(a, dU)) and (b is None or torch.equal(b, dth))


def test_new_entry_points_at_one_channel_give_the_single_channel_bits(H):
    Hi, Wi, Ho, Wo, Ch = SHAPES[4]
    case = _case(Hi, Wi, Ho, Wo, Ch)
    Ut, tht, dt = _cuda(case["U"], case["th"], case["d"])
    out = torch.empty(3, Ho, Wo, 1, device="cuda")
    H.check(H.lib().air_transformer_nc_fwd(_p(Ut), _p(tht), _p(out), 3, 1, Hi, Wi, 1, Ho, Wo, _stream()))
    assert torch.equal(out, _planes_fwd(H, Ut, tht, Ho, Wo))
    assert np.array_equal(out.cpu().numpy()[:1], case["out"][:1])
    dU, dth, dU1, dth1 = (torch.empty_like(Ut), torch.empty(3, 6, device="cuda"), torch.empty_like(Ut), torch.empty(3, 6, device="cuda"))
    H.check(H.lib().air_transformer_nc_bwd(_p(Ut), _p(tht), _p(dt), _p(dU), _p(dth), 3, 1, Hi, Wi, 1, Ho, Wo, _stream()))
    H.check(H.lib().air_transformer_bwd(_p(Ut), _p(tht), _p(dt), _p(dU1), _p(dth1), 3, Hi, Wi, Ho, Wo, _stream()))
    assert torch.equal(dU, dU1) and torch.equal(dth, dth1)


def test_more_channels_than_a_workgroup_holds(H):
    """Hi = Wi = 50, C = 64: sixteen channel groups per image; no size error, every plane the single-channel kernels' bits."""
    from air.transformer import transformer, transformer_grad
    rng = np.random.RandomState(64)
    B, Hi, Wi, Ho, Wo, Ch = 2, 50, 50, 7, 8, 64
    U = rng.uniform(0, 1, (B, Hi, Wi, Ch)).astype(f32)
    th = (np.tile(np.array([[0.55, 0.25, 0.3], [-0.2, 0.6, -0.4]], f32), (B, 1, 1)) + rng.randn(B, 2, 3).astype(f32) * 0.15).astype(f32)
    d = (rng.randn(B, Ho, Wo, Ch) * np.where(rng.uniform(size=(B, Ho, Wo, Ch)) < 0.1, 1e6, 1.0)).astype(f32)
    Ut, tht, dt = _cuda(U, th, d)
    assert torch.equal(transformer(Ut, tht, (Ho, Wo)), _planes_fwd(H, Ut, tht, Ho, Wo))
    dU, dth = transformer_grad(Ut, tht, (Ho, Wo), dt)
    for c in range(Ch):
        plane, g, ref = Ut[..., c].contiguous(), dt[..., c].contiguous(), torch.empty(B, Hi, Wi, device="cuda")
        H.check(H.lib().air_transformer_bwd(_p(plane), _p(tht), _p(g), _p(ref), None, B, Hi, Wi, Ho, Wo, _stream()))
        assert torch.equal(dU[..., c], ref), c
    assert bool(torch.isfinite(dth).all())


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,Ch", BATCH_SHAPES)
def test_batch_transformer_matches_oracle(H, Hi, Wi, Ho, Wo, Ch):
    from air.transformer import batch_transformer, batch_transformer_grad, transformer
    B, T = 2, 3
    case = _case(Hi, Wi, Ho, Wo, Ch, B=B, T=T)
    Ut, tht, dt = _cuda(case["U"], case["th"].reshape(B, T, 6), case["d"])
    out = batch_transformer(Ut, tht, (Ho, Wo))
    assert out.shape == (B * T, Ho, Wo, Ch)
    assert torch.equal(out, transformer(Ut.repeat_interleave(T, dim=0), tht.reshape(B * T, 6), (Ho, Wo)))
    assert torch.equal(batch_transformer(Ut, tht.reshape(B, T, 2, 3), (Ho, Wo)), out)
    dU, dth = batch_transformer_grad(Ut, tht, (Ho, Wo), dt)
    assert dU.shape == (B, Hi, Wi, Ch) and dth.shape == (B * T, 6)
    differ = int((case["dU"] != case["dU_desc"]).sum())
    print("d_U: ascending and descending t differ in %d of %d elements" % (differ, case["dU"].size))
    assert differ > 0                                         # the order of the sum over t is visible in these inputs
    assert np.array_equal(dU.cpu().numpy(), case["dU"])
    _check_dtheta(dth, case)


def test_batch_transformer_single_channel_input_without_channel_axis(H):
    from air.transformer import batch_transformer, batch_transformer_grad
    Hi, Wi, Ho, Wo, Ch = BATCH_SHAPES[0]
    B, T = 2, 3
    case = _case(Hi, Wi, Ho, Wo, Ch, B=B, T=T)
    Ut, tht, dt = _cuda(case["U"][..., 1], case["th"].reshape(B, T, 6), case["d"][..., 1])
    out = batch_transformer(Ut, tht, (Ho, Wo))
    assert out.shape == (B * T, Ho, Wo)
    assert np.array_equal(out.cpu().numpy()[:1], case["out"][:1, ..., 1])
    dU, _ = batch_transformer_grad(Ut, tht, (Ho, Wo), dt)
    assert dU.shape == (B, Hi, Wi) and np.array_equal(dU.cpu().numpy(), case["dU"][..., 1])


def test_batch_transformer_with_one_transform_is_transformer(H):
    from air.transformer import batch_transformer, batch_transformer_grad, transformer, transformer_grad
    Hi, Wi, Ho, Wo, Ch = SHAPES[0]
    case = _case(Hi, Wi, Ho, Wo, Ch)
    Ut, tht, dt = _cuda(case["U"], case["th"], case["d"])
    assert torch.equal(batch_transformer(Ut, tht.reshape(3, 1, 6), (Ho, Wo)), transformer(Ut, tht, (Ho, Wo)))
    dU, dth = transformer_grad(Ut, tht, (Ho, Wo), dt)
    dUb, dthb = batch_transformer_grad(Ut, tht.reshape(3, 1, 6), (Ho, Wo), dt)
    assert torch.equal(dUb, dU) and torch.equal(dthb, dth)


def test_autograd_carries_both_ops(H):
    from air.transformer import batch_transformer, batch_transformer_grad, transformer, transformer_grad
    Hi, Wi, Ho, Wo, Ch = SHAPES[0]
    case = _case(Hi, Wi, Ho, Wo, Ch)
    Ut, tht, dt = _cuda(case["U"], case["th"], case["d"])
    dU, dth = transformer_grad(Ut, tht, (Ho, Wo), dt)
    Ug, tg = Ut.clone().requires_grad_(True), tht.clone().requires_grad_(True)
    transformer(Ug, tg, (Ho, Wo)).backward(dt)
    assert torch.equal(Ug.grad, dU) and torch.equal(tg.grad.reshape(3, 6), dth)
    B, T = 2, 3
    case = _case(Hi, Wi, Ho, Wo, Ch, B=B, T=T)
    Ut, tht, dt = _cuda(case["U"], case["th"].reshape(B, T, 2, 3), case["d"])
    dU, dth = batch_transformer_grad(Ut, tht, (Ho, Wo), dt)
    Ug, tg = Ut.clone().requires_grad_(True), tht.clone().requires_grad_(True)
    batch_transformer(Ug, tg, (Ho, Wo)).backward(dt)
    assert tg.grad.shape == tht.shape
    assert torch.equal(Ug.grad, dU) and torch.equal(tg.grad.reshape(B * T, 6), dth)
    # theta alone: no d U is computed, the same d theta
    tg2 = tht.clone().requires_grad_(True)
    batch_transformer(Ut, tg2, (Ho, Wo)).backward(dt)
    assert torch.equal(tg2.grad, tg.grad)


def test_backward_is_deterministic(H):
    from air.transformer import batch_transformer_grad, transformer_grad
    Hi, Wi, Ho, Wo, Ch = SHAPES[3]
    case = _case(Hi, Wi, Ho, Wo, Ch)
    Ut, tht, dt = _cuda(case["U"], case["th"], case["d"])
    a, b = transformer_grad(Ut, tht, (Ho, Wo), dt), transformer_grad(Ut, tht, (Ho, Wo), dt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    thb = tht.reshape(1, 3, 6)                              # ... and with the sum over transforms
    a, b = batch_transformer_grad(Ut[:1], thb, (Ho, Wo), dt), batch_transformer_grad(Ut[:1], thb, (Ho, Wo), dt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_single_channel_inputs_stay_on_the_single_channel_entry_points(H, monkeypatch):
    from air.transformer import transformer, transformer_grad
    rng = np.random.RandomState(3)
    B, Hi, Wi, Ho, Wo = 3, 50, 50, 28, 28
    U = rng.uniform(0, 1, (B, Hi, Wi, 1)).astype(f32)
    th = (np.tile(np.array([[0.55, 0.25, 0.3], [-0.2, 0.6, -0.4]], f32), (B, 1, 1)) + rng.randn(B, 2, 3).astype(f32) * 0.15).astype(f32)
    d = rng.randn(B, Ho, Wo, 1).astype(f32)
    Ut, tht, dt = _cuda(U, th, d)

    def rerouted(*a):
        raise AssertionError("a single-channel input reached the multi-channel entry points")
    monkeypatch.setattr(H.lib(), "air_transformer_nc_fwd", rerouted)
    monkeypatch.setattr(H.lib(), "air_transformer_nc_bwd", rerouted)
    ref = torch.empty(B, Ho, Wo, device="cuda")
    H.check(H.lib().air_transformer_fwd(_p(Ut), _p(tht), _p(ref), B, Hi, Wi, Ho, Wo, _stream()))
    got = transformer(Ut, tht, (Ho, Wo))
    assert got.shape == (B, Ho, Wo, 1) and torch.equal(got[..., 0], ref)
    assert torch.equal(transformer(Ut[..., 0], tht, (Ho, Wo)), ref)
    dU_ref, dth_ref = torch.empty(B, Hi, Wi, device="cuda"), torch.empty(B, 6, device="cuda")
    H.check(H.lib().air_transformer_bwd(_p(Ut), _p(tht), _p(dt), _p(dU_ref), _p(dth_ref), B, Hi, Wi, Ho, Wo, _stream()))
    dU, dth = transformer_grad(Ut, tht, (Ho, Wo), dt)
    assert torch.equal(dth, dth_ref) and torch.equal(dU, dU_ref)


_FALLBACK_SCRIPT = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tf-attend-infer-repeat_amd"))
from air.transformer import batch_transformer_grad
z = np.load(sys.argv[2])
t = lambda a: torch.tensor(a, device="cuda")
dU, dth = batch_transformer_grad(t(z["U"]), t(z["th"]), (int(z["Ho"]), int(z["Wo"])), t(z["d"]))
torch.cuda.synchronize()
np.savez(sys.argv[3], dU=dU.cpu().numpy(), dth=dth.cpu().numpy())
'''


def test_single_lane_fallback_gives_the_same_bits(H, tmp_path):
    """AIR_LDS_ORDER=0 (a part whose LDS atomics do not apply lanes in order, decided once per process): one lane per channel
    walks the terms.  Same bits as the LDS-pipe path of this process, i.e. as the oracle."""
    import subprocess
    import sys
    from air.transformer import batch_transformer_grad
    Hi, Wi, Ho, Wo, Ch = BATCH_SHAPES[0]
    B, T = 2, 3
    case = _case(Hi, Wi, Ho, Wo, Ch, B=B, T=T)
    thetas = case["th"].reshape(B, T, 6)
    Ut, tht, dt = _cuda(case["U"], thetas, case["d"])
    dU, dth = batch_transformer_grad(Ut, tht, (Ho, Wo), dt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script, inp, out = tmp_path / "fallback.py", tmp_path / "in.npz", tmp_path / "out.npz"
    script.write_text(_FALLBACK_SCRIPT)
    np.savez(inp, U=case["U"], th=thetas, d=case["d"], Ho=Ho, Wo=Wo)
    env = dict(os.environ)
    env["AIR_LDS_ORDER"] = "0"
    r = subprocess.run([sys.executable, str(script), root, str(inp), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert np.array_equal(got["dU"], dU.cpu().numpy()) and np.array_equal(got["dU"], case["dU"])
    assert np.array_equal(got["dth"], dth.cpu().numpy())
