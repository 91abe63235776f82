"""GPU tests of air.vae (the VAE of the reference's air/vae.py as a differentiable torch module on the HIP kernels).

  * fp32 precision, the model's variables / glimpses / noise: the model's own ml and vrec bit for bit (same descriptors);
  * forward against oracle.air_oracle.vae in float32 numpy: 2e-5 absolute, the forward band of the parity tests;
  * gradients against float64 torch autograd of a restatement of vae.py written here, relative to each tensor's
    max |reference|.  Measured on the MI355X (worst over every parameter and d_inputs, both losses, M = 5 and 70,
    likelihood_std 0 and 0.3, softplus and relu):  fp32 precision MEASURED_FP32 below; asserted: 4 x that (room for another
    accumulation order after a tile change), capped at 1e-4 -- exact fp32 products at K <= 784 cannot be further than
    K * 2^-24 = 4.7e-5 from the reference, so anything beyond the cap is a bug;
  * bf16 precision: reconstruction within 3e-2 of the fp32-precision forward (the band of test_forward_parity_bf16);
    gradients relative to the fp32-precision ones: MEASURED_BF16 below, asserted 2 x that (rounding of fixed operands
    to bf16 is deterministic; the margin is for tile changes);
  * determinism (two eager forward + backward runs, the Concrete KL in the same pass, identical bits) and the variables
    round trip.
NOT tested: a torch.cuda.graph capture of forward + backward.  It was written (one stream, one eager warm-up, one replay
compared with the eager bits) and ended twice in a segmentation fault inside torch's capture_end on the MI355X, the second
time with the warm-up and the capture on the same stream and no earlier autograd graph alive; the cause is not known, so
the ops refuse to run under capture (air/vae.py, air/concrete.py) and the test is left out with them."""
import functools

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle.synth import blob_canvases

pytestmark = pytest.mark.gpu

f32 = np.float32
D, REC, Z, GEN = 36, (24, 16), 6, (16, 24)
# worst |gradient - reference| / max |reference| measured on the MI355X (printed by the tests below)
#   fp32 precision against float64: 4.95e-07 (vae/generative_1/weights, M = 5, likelihood_std 0, softplus; the ten cases lie
#   between 2.6e-07 and 4.95e-07)
#   bf16 precision against fp32 precision: 1.10e-02 at M = 5 (vae/generative_1/biases), 6.07e-03 at M = 70 (vae/rec_mean/weights)
MEASURED_FP32 = 4.95e-7
MEASURED_BF16 = 1.10e-2
FP32_GRAD_BOUND = min(4 * MEASURED_FP32, 1e-4)
BF16_GRAD_BOUND = 2 * MEASURED_BF16


@pytest.fixture(scope="module")
def V():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import vae
    return vae


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _names():
    layers = ["recognition_%d" % (i + 1) for i in range(len(REC))] + ["rec_mean", "rec_log_variance"] + \
             ["generative_%d" % (i + 1) for i in range(len(GEN))] + ["gen_mean"]
    return layers


@functools.lru_cache(maxsize=None)
def _params():
    """variables under their TF names: Glorot-sized weights and NON-zero biases (a zero bias hides a misplaced one)"""
    rng = np.random.RandomState(11)
    widths = (D,) + REC
    shapes = {}
    for i, u in enumerate(REC):
        shapes["recognition_%d" % (i + 1)] = (widths[i], u)
    shapes["rec_mean"] = shapes["rec_log_variance"] = (REC[-1], Z)
    prev = Z
    for i, u in enumerate(GEN):
        shapes["generative_%d" % (i + 1)] = (prev, u)
        prev = u
    shapes["gen_mean"] = (prev, D)
    P = {}
    for layer in _names():
        k, n = shapes[layer]
        lim = np.sqrt(6.0 / (k + n))
        P["vae/%s/weights" % layer] = rng.uniform(-lim, lim, (k, n)).astype(f32)
        P["vae/%s/biases" % layer] = rng.uniform(-0.3, 0.3, n).astype(f32)
    for a in P.values():
        a.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def _data(M):
    rng = np.random.RandomState(1000 + M)
    out = dict(x=rng.uniform(0, 1, (M, D)).astype(f32), eps_z=rng.randn(M, Z).astype(f32), eps_x=rng.randn(M, D).astype(f32),
               w1=rng.randn(M, D).astype(f32), w2=rng.randn(M, Z).astype(f32), w3=rng.randn(M, Z).astype(f32),
               w4=rng.randn(M, Z).astype(f32))
    for a in out.values():
        a.setflags(write=False)
    return out


def _act64(v, activation):
    return torch.nn.functional.softplus(v) if activation == "softplus" else torch.clamp(v, min=0.0)


def _vae64(x, P, eps_z, eps_x, std, activation):
    """vae.py in float64 torch: the encoder stack, the two linear heads, the sample, the decoder stack, the noisy sigmoid"""
    h = x
    for i in range(len(REC)):
        h = _act64(h @ P["vae/recognition_%d/weights" % (i + 1)] + P["vae/recognition_%d/biases" % (i + 1)], activation)
    mean = h @ P["vae/rec_mean/weights"] + P["vae/rec_mean/biases"]
    lv = h @ P["vae/rec_log_variance/weights"] + P["vae/rec_log_variance/biases"]
    h = mean + eps_z * torch.exp(0.5 * lv)
    for i in range(len(GEN)):
        h = _act64(h @ P["vae/generative_%d/weights" % (i + 1)] + P["vae/generative_%d/biases" % (i + 1)], activation)
    rec = torch.sigmoid(h @ P["vae/gen_mean/weights"] + P["vae/gen_mean/biases"] + std * eps_x)
    return rec, mean, lv, mean


@functools.lru_cache(maxsize=None)
def _reference_grads(M, std, activation, all_outputs):
    """float64 gradients of the test loss wrt every variable (TF names) and the inputs (key 'inputs')"""
    d = _data(M)
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)  # noqa: E731
    P = {k: t(v, True) for k, v in _params().items()}
    x = t(d["x"], True)
    rec, mean, lv, mean4 = _vae64(x, P, t(d["eps_z"]), t(d["eps_x"]), std, activation)
    loss = (t(d["w1"]) * rec).sum()
    if all_outputs:
        loss = loss + (t(d["w2"]) * mean).sum() + (t(d["w3"]) * lv).sum() + (t(d["w4"]) * mean4).sum()
    loss.backward()
    out = {k: v.grad.numpy() for k, v in P.items()}
    out["inputs"] = x.grad.numpy()
    return out


def _module(V, std, activation="softplus", precision="fp32"):
    m = V.VAE(D, REC, Z, GEN, likelihood_std=std, activation=activation, precision=precision)
    m.load_variables(_params())
    return m


def _cuda(d, *keys):
    return tuple(torch.tensor(d[k], device="cuda") for k in keys)


def _run(V, m, M, all_outputs, std):
    """one forward + backward on the HIP kernels: (outputs, {TF name or 'inputs': gradient})"""
    d = _data(M)
    x, eps_z, eps_x, w1, w2, w3, w4 = _cuda(d, "x", "eps_z", "eps_x", "w1", "w2", "w3", "w4")
    x.requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    rec, mean, lv, mean4 = V.vae(x, D, REC, Z, GEN, std, module=m, eps_z=eps_z, eps_x=(eps_x if std else None))
    assert mean4 is mean or _same_bits(mean4, mean)
    loss = (w1 * rec).sum()
    if all_outputs:
        loss = loss + (w2 * mean).sum() + (w3 * lv).sum() + (w4 * mean4).sum()
    loss.backward()
    Zl = m.latent_dim
    fused = {k: p.grad for k, p in m._fused().items()}
    grads = {}
    for i in range(len(REC)):
        grads["vae/recognition_%d/weights" % (i + 1)], grads["vae/recognition_%d/biases" % (i + 1)] = fused["rec%d_w" % i], fused["rec%d_b" % i]
    grads["vae/rec_mean/weights"], grads["vae/rec_mean/biases"] = fused["ml_w"][:, :Zl], fused["ml_b"][:Zl]
    grads["vae/rec_log_variance/weights"], grads["vae/rec_log_variance/biases"] = fused["ml_w"][:, Zl:], fused["ml_b"][Zl:]
    for i in range(len(GEN)):
        grads["vae/generative_%d/weights" % (i + 1)], grads["vae/generative_%d/biases" % (i + 1)] = fused["gen%d_w" % i], fused["gen%d_b" % i]
    grads["vae/gen_mean/weights"], grads["vae/gen_mean/biases"] = fused["out_w"], fused["out_b"]
    grads["inputs"] = x.grad
    # (detached: a caller that keeps the results must not keep the autograd graph, and with it the gradient accumulators of
    # the parameters, alive)
    return tuple(t.detach() for t in (rec, mean, lv, mean4)), {k: v.clone() for k, v in grads.items()}


def _worst_rel(got, ref):
    """max over the tensors of max |got - ref| / max |ref| (tensors whose reference is identically zero: absolute)"""
    worst, where = 0.0, None
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        scale = np.abs(r).max()
        e = float(np.abs(_np(got[k]).astype(np.float64) - r).max() / (scale if scale > 0 else 1.0))
        if e > worst:
            worst, where = e, k
    return worst, where


# ---- 1. the model's own bits ----------------------------------------------------------------------------------------
def test_fp32_reproduces_the_models_ml_and_vrec_bit_for_bit(V):
    from air import air_model as am
    hp = dict(ao.DEFAULT_HP)
    B, N = 4, hp["max_steps"]
    images, targets = blob_canvases(B, hp["canvas_size"], hp["max_digits"], seed=3)
    am.reset_default_graph()
    model = am.AIRModel(torch.tensor(images.reshape(B, -1), device="cuda"), torch.tensor(targets, device="cuda"), cnn=False,
                        train=True, gemm_precision="fp32", **hp)
    model.set_noise(ao.make_noise(hp, B, 1))
    model.forward()
    d, Zm = hp["windows_size"] ** 2, hp["vae_latent_dimensions"]
    m = V.VAE(d, hp["vae_recognition_units"], Zm, hp["vae_generative_units"], likelihood_std=hp["vae_likelihood_std"],
              precision="fp32")
    m.load_variables(model.variables, scope="")
    M = N * B
    with torch.no_grad():
        rec, mean, lv, mean4 = m(model.window.reshape(M, d), eps_z=model.eps_z.reshape(M, Zm), eps_x=model.eps_x.reshape(M, d))
    ml = model.ml.reshape(M, 2 * Zm)
    assert _same_bits(mean, ml[:, :Zm]) and _same_bits(lv, ml[:, Zm:]) and _same_bits(mean4, ml[:, :Zm])
    assert _same_bits(rec, model.vrec.reshape(M, d))
    assert float(rec.std()) > 0 and float(lv.abs().max()) > 0
    am.reset_default_graph()


# ---- 2. forward against the numpy oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("std", [0.0, 0.3])
@pytest.mark.parametrize("M", [5, 70])
def test_forward_matches_the_oracle(V, M, std):
    d = _data(M)
    hp = dict(vae_recognition_units=REC, vae_generative_units=GEN, vae_likelihood_std=std)
    ref = ao.vae(d["x"], _params(), hp, d["eps_z"], d["eps_x"])
    m = _module(V, std)
    x, eps_z, eps_x = _cuda(d, "x", "eps_z", "eps_x")
    with torch.no_grad():
        got = V.vae(x, D, REC, Z, GEN, std, module=m, eps_z=eps_z, eps_x=(eps_x if std else None))
    for name, g, r in zip(("reconstruction", "mean", "log_variance", "mean (4th)"), got, ref):
        e = float(np.abs(_np(g) - r).max())
        print("M=%d std=%.1f %s: |got - ref| %.3g" % (M, std, name, e))
        assert g.shape == r.shape and e <= 2e-5, name
    if std == 0.0:
        # no likelihood noise: eps_x is neither drawn nor read -- NaNs in it change nothing
        with torch.no_grad():
            again = m(x, eps_z=eps_z, eps_x=torch.full_like(eps_x, float("nan")))
        assert _same_bits(again[0], got[0])


# ---- 3. / 4. gradients, fp32 precision ------------------------------------------------------------------------------
@pytest.mark.parametrize("all_outputs", [True, False])
@pytest.mark.parametrize("M,std,activation", [(5, 0.0, "softplus"), (5, 0.3, "softplus"), (70, 0.0, "softplus"),
                                              (70, 0.3, "softplus"), (5, 0.3, "relu")])
def test_gradients_match_float64_autograd(V, M, std, activation, all_outputs):
    m = _module(V, std, activation)
    outs, grads = _run(V, m, M, all_outputs, std)
    ref = _reference_grads(M, std, activation, all_outputs)
    assert set(grads) == set(ref)
    worst, where = _worst_rel(grads, ref)
    print("M=%d std=%.1f %s all_outputs=%d: worst relative gradient error %.3g (%s)" % (M, std, activation, all_outputs, worst, where))
    assert worst <= FP32_GRAD_BOUND, where
    if activation == "relu":
        d = _data(M)
        t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
        ref_out = _vae64(t(d["x"]), {k: t(v) for k, v in _params().items()}, t(d["eps_z"]), t(d["eps_x"]), std, activation)
        for g, r in zip(outs, ref_out):
            assert float(np.abs(_np(g) - r.numpy()).max()) <= 2e-5


# ---- 5. bf16 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [5, 70])
def test_bf16_against_the_fp32_precision(V, M):
    std = 0.3
    out32, g32 = _run(V, _module(V, std, precision="fp32"), M, True, std)
    out16, g16 = _run(V, _module(V, std, precision="bf16"), M, True, std)
    e = float((out16[0] - out32[0]).abs().max())
    print("M=%d bf16 reconstruction: |bf16 - fp32| %.3g" % (M, e))
    assert e <= 3e-2
    assert not _same_bits(out16[0], out32[0])                           # (the precision switch reaches the products)
    worst, where = _worst_rel(g16, {k: _np(v) for k, v in g32.items()})
    print("M=%d bf16 gradients: worst deviation from fp32 relative to max |fp32| %.3g (%s)" % (M, worst, where))
    assert worst <= BF16_GRAD_BOUND, where


# ---- 6. determinism (the torch.cuda.graph capture the ops were meant to support is left out: module docstring) ------
def test_deterministic(V):
    from air import concrete as cc
    M, std = 70, 0.3
    m = _module(V, std)
    o1, g1 = _run(V, m, M, True, std)
    o2, g2 = _run(V, m, M, True, std)
    assert all(_same_bits(a, b) for a, b in zip(o1, o2)) and all(_same_bits(g1[k], g2[k]) for k in g1)

    # with the Concrete KL in the same backward pass: two eager runs, identical bits
    d = _data(M)
    x, eps_z, eps_x, w1, w2, w3, w4 = _cuda(d, "x", "eps_z", "eps_x", "w1", "w2", "w3", "w4")
    x.requires_grad_(True)
    lo = w2[:, 0].contiguous().requires_grad_(True)                     # [M] log-odds for the KL
    u = torch.tensor(np.random.RandomState(3).uniform(0, 1, M).astype(f32), device="cuda")
    dyn = torch.tensor([-2.0, 0.8], device="cuda")                      # prior log-odds, temperature: device scalars
    leaves = [x, lo] + list(m.parameters())

    def step():
        for t in leaves:
            t.grad = None
        rec, mean, lv, mean4 = m(x, eps_z=eps_z, eps_x=eps_x)
        ypre = cc.concrete_binary_pre_sigmoid_sample(lo, dyn[1], u=u)
        kl = cc.concrete_binary_kl_mc_sample(ypre, dyn[0], dyn[1], lo, dyn[1])
        loss = (w1 * rec).sum() + (w2 * mean).sum() + (w3 * lv).sum() + (w4 * mean4).sum() + (kl * w3[:, 0]).sum()
        loss.backward()
        return [t.detach().clone() for t in (rec, mean, lv, kl)] + [t.grad.clone() for t in leaves]

    first, second = step(), step()
    assert all(_same_bits(a, b) for a, b in zip(first, second))
    assert all(bool(torch.isfinite(t).all()) for t in first) and float(first[-1].abs().max()) > 0


# ---- 7. variables ---------------------------------------------------------------------------------------------------
def test_variables_round_trip_and_fused_halves(V):
    M, std = 5, 0.3
    d = _data(M)
    x, eps_z, eps_x = _cuda(d, "x", "eps_z", "eps_x")
    a = _module(V, std)
    b = V.VAE(D, REC, Z, GEN, likelihood_std=std, precision="fp32", seed=5)
    with torch.no_grad():
        oa = a(x, eps_z=eps_z, eps_x=eps_x)
        assert not _same_bits(b(x, eps_z=eps_z, eps_x=eps_x)[0], oa[0])
        b.load_variables(a.variables())
        ob = b(x, eps_z=eps_z, eps_x=eps_x)
    assert all(_same_bits(p, q) for p, q in zip(oa, ob))
    assert list(a.variables()) == V.VAE.variable_names(REC, GEN)
    for k, v in a.variables().items():
        assert np.array_equal(_np(v), _params()[k]), k
    # the two halves of the fused bottleneck matrix, loaded from different constants
    src = {k: np.array(v) for k, v in _params().items()}
    src["vae/rec_mean/weights"][:], src["vae/rec_mean/biases"][:] = 1.0, 3.0
    src["vae/rec_log_variance/weights"][:], src["vae/rec_log_variance/biases"][:] = 2.0, 4.0
    b.load_variables({"scope/" + k: v for k, v in src.items()}, scope="scope")
    assert b.ml_w.shape == (REC[-1], 2 * Z) and b.ml_b.shape == (2 * Z,)
    assert bool((b.ml_w[:, :Z] == 1.0).all()) and bool((b.ml_w[:, Z:] == 2.0).all())
    assert bool((b.ml_b[:Z] == 3.0).all()) and bool((b.ml_b[Z:] == 4.0).all())
    with pytest.raises(KeyError):
        b.load_variables({k: v for k, v in src.items() if "gen_mean" not in k})
    # drawn noise: the same seed and call give the same bits, the next call differs
    with torch.no_grad():
        a.manual_seed(9)
        r0, r1 = a(x)[0], a(x)[0]
        a.manual_seed(9)
        assert _same_bits(a(x)[0], r0) and not _same_bits(r0, r1)
