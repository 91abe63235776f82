"""GPU tests of air.concrete (air_concrete_* of include/air_hip.h): the binary Concrete sample, its pre-sigmoid form and the
one-sample KL of the reference's air/concrete.py as stand-alone differentiable ops.

  * bit for bit the z_pres columns of the model's own att record (the ops call the attend kernel's device functions);
  * values against the numpy functions of oracle.air_oracle, 2e-4 absolute -- the band tests/test_gpu_graph_golden.py
    applies to z_pres_kls against the executed graph;
  * gradients against float64 torch autograd of a restatement of the formulas written here, 16 fp32 ulp of the tensor's
    scale max|reference| -- the yardstick of the teacher-forced backward epilogues (tests/test_gpu_graph_golden.py::_ulps).
Sizes: n = 1 (tail only), 257 (64 vector groups + a tail of one), and 257 elements starting 4 bytes into an allocation (no
16-byte alignment: the scalar path)."""
import functools

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle.synth import blob_canvases

pytestmark = pytest.mark.gpu

f32 = np.float32
ULP = 2.0 ** -23
EPS = 10e-10
#         n, offset of the first element in its allocation
SIZES = [(1, 0), (257, 0), (257, 1)]
T_POST, T_PRIOR, PRIOR_LO = 0.7, 1.3, -2.0


@pytest.fixture(scope="module")
def cc():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import concrete
    return concrete


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(a, off=0):
    """a device copy of the 1-D array `a` whose first element lies `off` floats into its allocation"""
    buf = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
    buf[off:] = torch.tensor(np.asarray(a))
    return buf[off:].detach()


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """log-odds in [-6, 6], uniforms, incoming gradients.  The draw of 257 includes a uniform of exactly 0 and the largest
    float below 1.  The single element of n = 1 is an ordinary draw: at either extreme the sample saturates (sigmoid(-30) or
    1 - 6e-8), d sig_y / d log_odds is ~1e-13 or rounds to 0, and a one-element tensor has no other scale -- the "ulp of
    the tensor's scale" yardstick would then ask for exp(-30) to 16 ulp from an fp32 argument that carries half an ulp of 30
    (~8 ulp of the result) before the kernel has done anything.  In the 257 draw the two extremes sit among ordinary
    elements, which set the scale, as the yardstick intends."""
    rng = np.random.RandomState(100 + n)
    lo = rng.uniform(-6, 6, n).astype(f32)
    u = rng.uniform(0, 1, n).astype(f32)
    if n > 1:
        u[0], u[1] = 0.0, np.nextafter(f32(1.0), f32(0.0))
    g1, g2 = rng.randn(n).astype(f32), rng.randn(n).astype(f32)
    plo_full = rng.uniform(-3, 3, n).astype(f32)
    for a in (lo, u, g1, g2, plo_full):
        a.setflags(write=False)
    return lo, u, g1, g2, plo_full


# ---- the formulas in float64 torch (the gradient reference) --------------------------------------------------------
def _noise64(u, eps):
    return torch.log(u + eps) - torch.log(1.0 - u + eps)


def _sample64(lo, u, T, eps=EPS):
    y = lo + _noise64(u, eps)
    return y, torch.sigmoid(y / T)


def _log_density64(y, T, a, eps):
    return np.log(T + eps) - y * T + a - 2.0 * torch.log(1.0 + torch.exp(a - y * T) + eps)


def _kl64(y, plo, pT, qlo, qT, eps=EPS):
    return _log_density64(y, qT, qlo, eps) - _log_density64(y, pT, plo, eps)


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _ulps(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(_np(got).astype(np.float64) - ref).max() / (np.abs(ref).max() * ULP))


# ---- 1. the model's own bits ----------------------------------------------------------------------------------------
def test_presigmoid_and_kl_are_the_models_bits(cc):
    from air import _hip as H
    from air import air_model as am
    hp = dict(ao.DEFAULT_HP)
    B, N = 5, hp["max_steps"]
    images, targets = blob_canvases(B, hp["canvas_size"], hp["max_digits"], seed=3)
    am.reset_default_graph()
    model = am.AIRModel(torch.tensor(images.reshape(B, -1), device="cuda"), torch.tensor(targets, device="cuda"), cnn=False,
                        train=True, gemm_precision="fp32", **hp)
    model.set_noise(ao.make_noise(hp, B, 1))
    model.forward()
    lo = model.out7[..., 6]                                  # [N, B], a strided view
    T = model.dyn[H.DYN_TEMPERATURE]                         # 0-dim device views: read by the kernels, never by the host
    plo = model.dyn[H.DYN_PRIOR_LOG_ODDS]
    assert T.dim() == 0 and lo.shape == (N, B) and not lo.is_contiguous()
    ypre = cc.concrete_binary_pre_sigmoid_sample(lo, T, u=model.u)
    assert _same_bits(ypre, model.att[..., H.ATT_ZPRE])
    kl = cc.concrete_binary_kl_mc_sample(ypre, plo, T, lo, T)
    assert _same_bits(kl, model.att[..., H.ATT_KL_Z])
    assert float(kl.abs().max()) > 0.0
    am.reset_default_graph()


# ---- 2. values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", SIZES)
def test_values_match_the_numpy_functions(cc, n, off):
    lo, u, _, _, _ = _inputs(n)
    ref_y = ao.concrete_binary_pre_sigmoid_sample(lo, T_POST, u)
    ref_kl = ao.concrete_binary_kl_mc_sample(ref_y, PRIOR_LO, T_PRIOR, lo, T_POST)
    y = cc.concrete_binary_pre_sigmoid_sample(_dev(lo, off), T_POST, u=_dev(u, off))
    kl = cc.concrete_binary_kl_mc_sample(y, PRIOR_LO, T_PRIOR, _dev(lo, off), T_POST)
    assert y.shape == (n,) and kl.shape == (n,)
    ey, ek = np.abs(_np(y) - ref_y).max(), np.abs(_np(kl) - ref_kl).max()
    print("n=%d off=%d: |y - ref| %.3g, |kl - ref| %.3g" % (n, off, ey, ek))
    assert ey <= 2e-4 and ek <= 2e-4


# ---- 3. concrete_binary_sample --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", SIZES)
def test_sample_soft_and_hard(cc, n, off):
    lo, u, g1, g2, _ = _inputs(n)
    ref_pre = ao.concrete_binary_pre_sigmoid_sample(lo, T_POST, u)
    ref_y, ref_s = ref_pre * f32(T_POST), ao.sigmoid(ref_pre)
    y, s = cc.concrete_binary_sample(_dev(lo, off), T_POST, u=_dev(u, off))
    assert np.abs(_np(y) - ref_y).max() <= 2e-4 and np.abs(_np(s) - ref_s).max() <= 2e-4
    yh, sh = cc.concrete_binary_sample(_dev(lo, off), T_POST, hard=True, u=_dev(u, off))
    assert _same_bits(yh, y)
    assert set(np.unique(_np(sh))) <= {0.0, 1.0}
    assert np.array_equal(_np(sh), np.rint(_np(s)))
    # straight-through: the hard sample carries the soft one's gradient, bit for bit
    grads = []
    for hard in (False, True):
        x = _dev(lo, off).requires_grad_(True)
        yy, ss = cc.concrete_binary_sample(x, T_POST, hard=hard, u=_dev(u, off))
        (yy * _dev(g1, off)).sum().add((ss * _dev(g2, off)).sum()).backward()
        grads.append(x.grad)
    assert _same_bits(grads[0], grads[1])


def test_half_rounds_to_even(cc):
    z = torch.zeros(4, device="cuda")
    y, s = cc.concrete_binary_sample(z, 1.0, hard=True, u=torch.full((4,), 0.5, device="cuda"))
    assert torch.equal(y, z) and torch.equal(s, z)                      # sigmoid(0) = 0.5 -> 0
    _, soft = cc.concrete_binary_sample(z, 1.0, u=torch.full((4,), 0.5, device="cuda"))
    assert torch.equal(soft, torch.full((4,), 0.5, device="cuda"))


# ---- 4. gradients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", SIZES)
def test_gradients_match_float64_autograd(cc, n, off):
    lo, u, g1, g2, plo_full = _inputs(n)
    dv = lambda a: _dev(a, off)  # noqa: E731
    # the sample: both outputs, then each alone (the other incoming gradient is absent)
    for use_y, use_s in ((True, True), (True, False), (False, True)):
        l64 = _t64(lo, True)
        y64, s64 = _sample64(l64, _t64(u), T_POST)
        ((y64 * _t64(g1)).sum() * use_y + (s64 * _t64(g2)).sum() * use_s).backward()
        x = dv(lo).requires_grad_(True)
        y, s = cc.concrete_binary_sample(x, T_POST, u=dv(u))
        loss = (y * dv(g1)).sum() if use_y else 0.0
        loss = loss + ((s * dv(g2)).sum() if use_s else 0.0)
        loss.backward()
        e = _ulps(x.grad, l64.grad.numpy())
        print("n=%d off=%d sample(y=%d, sig=%d): %.2f ulp" % (n, off, use_y, use_s, e))
        assert e <= 16
    # the pre-sigmoid sample
    l64 = _t64(lo, True)
    ((l64 + _noise64(_t64(u), EPS)) / T_POST * _t64(g1)).sum().backward()
    x = dv(lo).requires_grad_(True)
    ypre = cc.concrete_binary_pre_sigmoid_sample(x, T_POST, u=dv(u))
    (ypre * dv(g1)).sum().backward()
    e = _ulps(x.grad, l64.grad.numpy())
    print("n=%d off=%d pre-sigmoid: %.2f ulp" % (n, off, e))
    assert e <= 16
    # the KL at the sample: to y, to the posterior log-odds, and to a per-element prior
    yv = _np(ypre)
    y64, q64, p64 = _t64(yv, True), _t64(lo, True), _t64(plo_full, True)
    (_kl64(y64, p64, T_PRIOR, q64, T_POST) * _t64(g2)).sum().backward()
    yt, qt, pt = dv(yv).requires_grad_(True), dv(lo).requires_grad_(True), dv(plo_full).requires_grad_(True)
    (cc.concrete_binary_kl_mc_sample(yt, pt, T_PRIOR, qt, T_POST) * dv(g2)).sum().backward()
    for name, got, ref in (("d_y", yt.grad, y64.grad), ("d_posterior", qt.grad, q64.grad), ("d_prior", pt.grad, p64.grad)):
        e = _ulps(got, ref.numpy())
        print("n=%d off=%d kl %s: %.2f ulp" % (n, off, name, e))
        assert e <= 16, name
    # a scalar prior: the same gradients to y and the posterior
    y64, q64 = _t64(yv, True), _t64(lo, True)
    (_kl64(y64, PRIOR_LO, T_PRIOR, q64, T_POST) * _t64(g2)).sum().backward()
    yt, qt = dv(yv).requires_grad_(True), dv(lo).requires_grad_(True)
    (cc.concrete_binary_kl_mc_sample(yt, PRIOR_LO, T_PRIOR, qt, T_POST) * dv(g2)).sum().backward()
    assert _ulps(yt.grad, y64.grad.numpy()) <= 16 and _ulps(qt.grad, q64.grad.numpy()) <= 16
    # only one input wants a gradient
    qt = dv(lo).requires_grad_(True)
    (cc.concrete_binary_kl_mc_sample(dv(yv), PRIOR_LO, T_PRIOR, qt, T_POST) * dv(g2)).sum().backward()
    assert _ulps(qt.grad, q64.grad.numpy()) <= 16


# ---- 5. the three forms of a scalar argument ------------------------------------------------------------------------
def test_scalar_forms_give_identical_bits(cc):
    n = 257
    lo, u, g1, _, _ = _inputs(n)
    dl, du = _dev(lo), _dev(u)
    forms = lambda v: (v, torch.tensor(v, device="cuda"), torch.full((n,), v, device="cuda"))  # noqa: E731
    ys = [cc.concrete_binary_pre_sigmoid_sample(dl, T, u=du) for T in forms(T_POST)]
    assert _same_bits(ys[0], ys[1]) and _same_bits(ys[0], ys[2])
    ss = [cc.concrete_binary_sample(dl, T, u=du)[1] for T in forms(T_POST)]
    assert _same_bits(ss[0], ss[1]) and _same_bits(ss[0], ss[2])
    kls, gys = [], []
    for plo, pT, qT in zip(forms(PRIOR_LO), forms(T_PRIOR), forms(T_POST)):
        y = ys[0].clone().requires_grad_(True)
        kl = cc.concrete_binary_kl_mc_sample(y, plo, pT, dl, qT)
        (kl * _dev(g1)).sum().backward()
        kls.append(kl)
        gys.append(y.grad)
    assert _same_bits(kls[0], kls[1]) and _same_bits(kls[0], kls[2])
    assert _same_bits(gys[0], gys[1]) and _same_bits(gys[0], gys[2])
    # a one-element tensor is read when the kernel runs: rewriting it in place changes the next call, no new descriptor
    T = torch.tensor(T_POST, device="cuda")
    T.fill_(1.1)
    assert _same_bits(cc.concrete_binary_pre_sigmoid_sample(dl, T, u=du), cc.concrete_binary_pre_sigmoid_sample(dl, 1.1, u=du))
    # eps is honoured as passed
    assert not _same_bits(cc.concrete_binary_pre_sigmoid_sample(dl, T_POST, 1e-3, u=du), ys[0])
    bad = torch.tensor(T_POST, device="cuda", requires_grad=True)
    with pytest.raises(ValueError):
        cc.concrete_binary_pre_sigmoid_sample(dl, bad, u=du)
    with pytest.raises(ValueError):
        cc.concrete_binary_sample(dl, bad, u=du)
    with pytest.raises(ValueError):
        cc.concrete_binary_kl_mc_sample(ys[0], PRIOR_LO, bad, dl, T_POST)
    with pytest.raises(ValueError):
        cc.concrete_binary_kl_mc_sample(ys[0], PRIOR_LO, T_PRIOR, dl, bad)


# ---- 6. drawn noise -------------------------------------------------------------------------------------------------
def test_drawn_noise_is_keyed_by_seed_and_call(cc):
    lo = _dev(_inputs(257)[0])
    cc.manual_seed(5)
    a = cc.concrete_binary_pre_sigmoid_sample(lo, T_POST)
    b = cc.concrete_binary_pre_sigmoid_sample(lo, T_POST)
    cc.manual_seed(5)
    a2 = cc.concrete_binary_pre_sigmoid_sample(lo, T_POST)
    b2, _ = cc.concrete_binary_sample(lo, T_POST)
    assert _same_bits(a, a2) and not _same_bits(a, b)
    assert _same_bits(b2, b * T_POST) or np.abs(_np(b2) - _np(b) * T_POST).max() <= 1e-5     # the same uniforms: call 1 again
    cc.manual_seed(6)
    assert not _same_bits(cc.concrete_binary_pre_sigmoid_sample(lo, T_POST), a)
    assert bool(torch.isfinite(a).all())


# ---- 7. shapes ------------------------------------------------------------------------------------------------------
def test_shapes_and_non_contiguous_inputs(cc):
    rng = np.random.RandomState(7)
    lo = torch.tensor(rng.uniform(-6, 6, (7, 3)).astype(f32), device="cuda").t()          # [3, 7], strides (1, 3)
    u = torch.tensor(rng.uniform(0, 1, (7, 3)).astype(f32), device="cuda").t()
    assert lo.shape == (3, 7) and not lo.is_contiguous()
    flat_lo, flat_u = lo.contiguous().view(-1), u.contiguous().view(-1)
    y = cc.concrete_binary_pre_sigmoid_sample(lo, T_POST, u=u)
    assert y.shape == (3, 7) and _same_bits(y.reshape(-1), cc.concrete_binary_pre_sigmoid_sample(flat_lo, T_POST, u=flat_u))
    yy, ss = cc.concrete_binary_sample(lo, T_POST, u=u)
    fy, fs = cc.concrete_binary_sample(flat_lo, T_POST, u=flat_u)
    assert yy.shape == ss.shape == (3, 7) and _same_bits(yy.reshape(-1), fy) and _same_bits(ss.reshape(-1), fs)
    kl = cc.concrete_binary_kl_mc_sample(y.t().contiguous().t(), PRIOR_LO, T_PRIOR, lo, T_POST)
    assert kl.shape == (3, 7)
    assert _same_bits(kl.reshape(-1), cc.concrete_binary_kl_mc_sample(y.reshape(-1), PRIOR_LO, T_PRIOR, flat_lo, T_POST))
    # gradients come back in the input's shape
    x = lo.clone().requires_grad_(True)
    cc.concrete_binary_pre_sigmoid_sample(x, T_POST, u=u).sum().backward()
    assert x.grad.shape == (3, 7)
