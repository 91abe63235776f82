"""AIRModel(likelihood="gaussian") -- the AIR paper's pixel likelihood, a Gaussian around the clipped canvas with the fixed
standard deviation vae_likelihood_std -- from the kernels up: the compose launch (write_fwd_gauss_kernel) and the un-fused
op (air_gauss_nll_fwd_bwd) against float64, the model's loss and gradients against the oracle and its fp64 twin, the
agreement of the three backward orders under it, launch plans and capture, the constructor, and a short training run.

Inputs, references and their conditions: tests/likelihood_cases.py (asserted on the CPU by tests/test_likelihood_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import likelihood_cases as lc
from oracle import air_oracle as ao
from oracle import air_oracle_torch as at
from oracle.synth import blob_canvases

pytestmark = pytest.mark.gpu

HP = dict(ao.TRAINING_HP)
SIGMA = np.float64(np.float32(HP["vae_likelihood_std"]))      # what dyn[AIR_DYN_LIK_STD] holds


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


@pytest.fixture(scope="module")
def am(H):
    from air import air_model
    return air_model


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. the compose launch ---------------------------------------------------------------------------------------------------

D_R = 2e-5       # the bound on the reconstruction itself, carried through the (linear) gradient formula below


@pytest.mark.parametrize("which", lc.COMPOSE_CASES + ["masked"], ids=lambda c: "masked" if c == "masked" else "%d-%d-%d" % c)
def test_write_fwd_gaussian_sixteen_steps_matches_fp64(H, which):
    """air_write_fwd with likelihood = AIR_LIK_GAUSSIAN at N = 16, B = 3 on the compose cases of tests/step_limit_cases.py
    (canvases on both sides of the image-prefetch threshold) and on the variant whose image 1 is masked out at every step.
    reconstruction, digit counts, KL_VAE and run_loss in the bands of test_write_fwd_sixteen_steps_matches_fp64; rec_loss =
    (0.5 / sigma^2) sum (x - r)^2 + D (log sigma + 0.5 log 2 pi) and loss_item rtol 1e-5 / atol 1e-3; d_recon exactly 0 at every
    compared pixel the clip does not pass, elsewhere within gsc * 2e-5 / sigma^2 (what the asserted bound on the reconstruction
    moves the linear formula by) + 1e-6 |ref| (the fp32 subtract, scale and divide); on the masked image d_recon ==
    -gsc * x / sigma^2 to 1e-6 relative at every pixel.  Nothing is filtered beyond in_band (<= 1 % of the pixels: CPU test).
    Measured on MI355X (largest over the four cases): reconstruction 2.2e-06, KL_VAE 7.9e-08 relative, run_loss 1.6e-07 /
    rec_loss 1.7e-07 / loss_item 1.6e-07 relative, d_recon error 0.105 of its allowance."""
    case, ref, g = lc.masked_case_and_reference() if which == "masked" else lc.compose_case_and_reference(*which)
    N, B, Cc, w, Z = case["N"], case["B"], case["C"], case["w"], case["Z"]
    att_in = case["att"].copy()
    att_in[..., H.ATT_KL_VAE] = np.nan
    vrec, ml, images, dyn, att = (_t(v) for v in (case["vrec"], case["ml"], case["images"], case["dyn"], att_in))
    recon, d_recon = torch.full((B, Cc * Cc), float("nan"), device="cuda"), torch.full((B, Cc * Cc), float("nan"), device="cuda")
    rec_loss, run_loss, loss_item = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    digits = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    order = torch.full((N * B,), -1, dtype=torch.int32, device="cuda")
    wf = H.WriteFwd(_p(vrec), _p(ml), _p(images), _p(dyn), _p(att), _p(recon), _p(rec_loss), _p(d_recon), _p(run_loss),
                    _p(digits), _p(loss_item), B, N, Cc, w, Z, _p(order), H.LIK_GAUSSIAN)
    H.check(H.lib().air_write_fwd(C.byref(wf), _stream()), "air_write_fwd")
    torch.cuda.synchronize()
    recon, d_recon, att_out, order = _np(recon), _np(d_recon), _np(att), _np(order)
    err = float(np.abs(recon - ref["recon"]).max())
    print("|d recon| %.2e" % err)
    assert err <= 2e-5
    assert np.array_equal(_np(digits), ref["run_digits"])
    kl = att_out[..., H.ATT_KL_VAE]
    kl_err = float(np.abs(kl - ref["kl_vae"]).max()) / max(1.0, float(np.abs(ref["kl_vae"]).max()))
    print("KL_VAE %.2e" % kl_err)
    assert np.isfinite(kl).all() and kl_err <= 1e-4
    want = dict(run_loss=ref["run_loss"], rec_loss=g["rec_loss"], loss_item=g["loss_item"])
    for name, got in (("run_loss", run_loss), ("rec_loss", rec_loss), ("loss_item", loss_item)):
        print("%s: relative error %.2e" % (name, float(np.abs(_np(got) - want[name]).max() / np.abs(want[name]).max())))
        np.testing.assert_allclose(_np(got), want[name], rtol=1e-5, atol=1e-3, err_msg=name)
    # d_recon
    cmp, passes = ~ref["in_band"], g["passes"]
    sel = cmp & passes
    assert not d_recon[cmp & ~passes].any()
    allow = g["gsc"] * D_R / g["sigma"] ** 2 + 1e-6 * np.abs(g["d_recon"])
    derr = np.abs(d_recon - g["d_recon"])
    print("d_recon: worst error / allowance %.2e over %d pixels" % (float((derr[sel] / allow[sel]).max()), int(sel.sum())))
    assert (derr[sel] <= allow[sel]).all()
    assert np.abs(d_recon).max() <= np.float32(g["gsc"] / g["sigma"] ** 2) * (1 + 1e-6)      # bounded on every canvas
    if which == "masked":
        b = lc.MASKED_IMAGE
        assert not recon[b].any()
        x = case["images"][b].astype(np.float64)
        np.testing.assert_allclose(d_recon[b], -g["gsc"] * x / g["sigma"] ** 2, rtol=1e-6, atol=0.0)
    # the longest-first list of the write backward rides in this launch as in the Bernoulli one
    assert np.array_equal(np.sort(order), np.arange(N * B))
    active = ref["active"].reshape(-1)[order]
    n_act = int(ref["active"].sum())
    assert active[:n_act].all() and not active[n_act:].any()


# ---- 2. the un-fused op -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D", [(5, 2500), (2, 1), (3, 257)])
def test_gauss_nll_fwd_bwd_matches_the_formula(H, B, D):
    """air_gauss_nll_fwd_bwd, the twin of air_bce_fwd_bwd (ties and just-outside values as its test has them): recon bit-equal
    to np.clip; rec_loss rtol 2e-5; d_recon rtol 2e-6 / atol 1e-9 (fewer than eight fp32 roundings, no difference of
    quotients); d_recon == NULL leaves the other outputs as they are."""
    rng = np.random.RandomState(3 + D)
    x = (rng.rand(B, D) * (rng.rand(B, D) > 0.8)).astype(np.float32)
    R = rng.uniform(-0.2, 1.3, size=(B, D)).astype(np.float32)
    ties = np.array([0.0, 1.0, -0.0, 0.5, 1.0000001, -1e-8, 0.25], np.float32)
    n = min(D, ties.size)
    R[0, :n] = ties[:n]
    dyn = np.zeros(H.DYN_COUNT, np.float32)
    dyn[H.DYN_GRAD_SCALE], dyn[H.DYN_LIK_STD] = 1.0 / B, 0.3
    xt, Rt, dt = _t(x), _t(R), _t(dyn)
    out = {}
    for with_grad in (True, False):
        rec = torch.full((B, D), float("nan"), device="cuda")
        loss = torch.full((B,), float("nan"), device="cuda")
        dR = torch.full((B, D), float("nan"), device="cuda")
        H.check(H.lib().air_gauss_nll_fwd_bwd(_p(xt), _p(Rt), _p(dt), _p(rec), _p(loss), _p(dR if with_grad else None), B, D,
                                              _stream()), "air_gauss_nll_fwd_bwd")
        torch.cuda.synchronize()
        out[with_grad] = (_np(rec), _np(loss), _np(dR))
    rec, loss, dR = out[True]
    f = np.float64
    sigma, gsc = f(dyn[H.DYN_LIK_STD]), f(dyn[H.DYN_GRAD_SCALE])
    r32 = np.clip(R, 0.0, 1.0)
    np.testing.assert_array_equal(rec, r32)
    want = lc.gaussian_nll(x.astype(f), r32.astype(f), sigma)
    print("rec_loss", loss, "relative error %.2e" % float(np.abs((loss - want) / want).max()))
    np.testing.assert_allclose(loss, want, rtol=2e-5)
    gd = gsc * (r32.astype(f) - x.astype(f)) / sigma ** 2
    gd[(R > 1.0) | (R < 0.0)] = 0.0                                     # clipped away: no gradient; ties pass
    print("d_recon: largest relative error %.2e" % float((np.abs(dR - gd) / np.maximum(np.abs(gd), 1e-30))[gd != 0].max(initial=0.0)))
    np.testing.assert_allclose(dR, gd, rtol=2e-6, atol=1e-9)
    assert np.array_equal(out[False][0], rec) and np.array_equal(out[False][1], loss) and np.isnan(out[False][2]).all()


# ---- 3 / 4. the model against the oracle and its fp64 twin ----------------------------------------------------------------------

def _make(am, B, train, prec="fp32", backward="exact", seed_img=3, seed_noise=1, likelihood="gaussian", **ctor_kw):
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=seed_img)
    params, noise = ao.init_params(HP, 0), ao.make_noise(HP, B, seed_noise)
    am.reset_default_graph()
    model = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=train,
                        gemm_precision=prec, backward=backward, likelihood=likelihood, **ctor_kw, **HP)
    model.load_state_dict(params)
    model.set_noise(noise)
    model.set_dynamic(z_pres_prior_log_odds=-2.0)
    return model, images, targets, params, noise


@pytest.mark.parametrize("train", [True, False])
def test_forward_loss_is_the_gaussian_of_the_models_own_reconstruction(am, train):
    """fp32, B = 4: reconstruction_loss against the fp64 formula on the device's own reconstruction (rtol 1e-5, atol 1e-4);
    loss against the oracle's loss_per_item - reconstruction_loss + gaussian(reconstruction) within the whole-model band
    elbo_rel <= 1e-2 of test_forward_parity_fp32 (no pole amplifies the canvas error here: the printed figure sits orders
    below it); everything but the loss is the Bernoulli model's."""
    model, images, targets, params, noise = _make(am, 4, train)
    assert model.likelihood == "gaussian"
    model.forward()
    torch.cuda.synchronize()
    o = ao.air_forward(params, images, targets, noise, HP, train, -2.0)
    x = images.astype(np.float64)
    own = lc.gaussian_nll(x, _np(model.reconstruction).astype(np.float64), SIGMA)
    np.testing.assert_allclose(_np(model.reconstruction_loss), own, rtol=1e-5, atol=1e-4)
    want_item = (o["loss_per_item"].astype(np.float64) - o["reconstruction_loss"].astype(np.float64)
                 + lc.gaussian_nll(x, o["reconstruction"].astype(np.float64), SIGMA))
    elbo_rel = abs(float(model.loss) - float(want_item.mean())) / abs(float(want_item.mean()))
    print("train=%s: loss %.4f, oracle %.4f, elbo_rel %.2e" % (train, float(model.loss), float(want_item.mean()), elbo_rel))
    assert elbo_rel <= 1e-2
    np.testing.assert_allclose(_np(model.loss_per_item), _np(model.reconstruction_loss) +
                               (o["loss_per_item"] - o["reconstruction_loss"]), rtol=1e-4, atol=1e-3)
    assert np.abs(_np(model.reconstruction) - o["reconstruction"]).max() <= 2e-5
    assert np.array_equal(_np(model.rec_num_digits), o["rec_num_digits"])


def _twin_gaussian_grads(params, images, targets, noise, matmul_mode):
    """d mean(loss_per_item - reconstruction_loss + gaussian_nll(reconstruction)) / d parameters in the fp64 twin"""
    f64 = torch.float64
    at.MATMUL_MODE = matmul_mode
    try:
        pt = at.to_torch(params, dtype=f64, requires_grad=True)
        x = torch.tensor(images, dtype=f64)
        out = at.air_forward(pt, x, torch.tensor(targets), at.to_torch(noise, dtype=f64), HP, True, -2.0)
        D = x.shape[1]
        nll = (0.5 / float(SIGMA) ** 2) * torch.sum((x - out["reconstruction"]) ** 2, dim=1) + \
            D * (float(np.log(SIGMA)) + 0.5 * float(np.log(2.0 * np.pi)))
        loss = (out["loss_per_item"] - out["reconstruction_loss"] + nll).mean()
        grads = torch.autograd.grad(loss, list(pt.values()))
    finally:
        at.MATMUL_MODE = "exact"
    return dict(zip(pt.keys(), grads))


@pytest.mark.parametrize("prec,B,loose", [("fp32", 4, ("z_pres", "rnn")), ("bf16", 16, ())])
def test_gradients_match_the_fp64_twin(am, prec, B, loose):
    """backward="exact" against autograd through the fp64 twin with the Gaussian term in place of the cross-entropy, per
    variable relative L2: fp32 at B = 4 in _grad_check's bands of tests/test_gpu_model.py (1e-2, ten times that for z_pres/*
    and rnn/*); bf16 at B = 16 against the twin that rounds the same GEMM operands (MATMUL_MODE = "bf16"): 1e-2, that file's
    inked band."""
    model, images, targets, params, noise = _make(am, B, True, prec=prec)
    s = model._stream()
    model._run_forward(s)
    model._run_backward(s)
    torch.cuda.synchronize()
    grads = _twin_gaussian_grads(params, images, targets, noise, "bf16" if prec == "bf16" else "exact")
    rep = {}
    for k, gref in grads.items():
        got = model.gradients[k].detach().cpu().double()
        rep[k] = float((got - gref.double()).norm() / max(float(gref.double().norm()), 1e-12))
        print("%s %-40s %.2e" % (prec, k, rep[k]))
    tol = 1e-2
    bad = {k: v for k, v in rep.items() if v > (tol * 10 if loose and k.startswith(loose) else tol)}
    assert not bad, bad


# ---- 5. the backward orders agree under the bounded gradient --------------------------------------------------------------------

def test_backward_orders_agree_under_the_gaussian_likelihood(am):
    """The property the option is wanted for.  On inked canvases (the inputs of
    test_reference_backward_carries_a_residue_the_exact_adjoint_does_not: B = 64, prior log-odds 9.21) the reference-order and
    the carried backward equal the exact adjoint per variable to relative L2 <= 2e-3 -- the band of
    test_reference_and_exact_backward_agree_without_residues, whose premise (d loss / d canvas stays O(1)) this likelihood
    provides on any canvas.  The Bernoulli figure on the same inputs is printed beside each."""
    B = 64
    import multi_mnist as mm
    ds = mm.generate_dataset(2, 100, 10)
    images, targets = ds["train_images"][:B], ds["train_digits"][:B]
    params, noise = ao.init_params(HP, 0), ao.make_noise(HP, B, 5)
    grads = {}
    for lik in ("gaussian", "bernoulli"):
        for mode in ("exact", "reference", "reference_carried"):
            am.reset_default_graph()
            m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False,
                            train=True, backward=mode, likelihood=lik, **HP)
            m.load_state_dict(params)
            m.set_noise(noise)
            m.set_dynamic(z_pres_prior_log_odds=9.21)
            s = m._stream()
            m._run_forward(s)
            m._run_backward(s)
            torch.cuda.synchronize()
            grads[lik, mode] = {k: v.detach().cpu().double().clone() for k, v in m.gradients.items()}
    bad = {}
    for k, ge in grads["gaussian", "exact"].items():
        be = grads["bernoulli", "exact"][k]
        for mode in ("reference", "reference_carried"):
            err = float((grads["gaussian", mode][k] - ge).norm() / (ge.norm() + 1e-30))
            bern = float((grads["bernoulli", mode][k] - be).norm() / (be.norm() + 1e-30))
            print("%-18s %-40s gaussian %.2e (|exact| %.2e)   bernoulli %.2e" % (mode, k, err, float(ge.norm()), bern))
            if err > 2e-3:
                bad[mode, k] = (err, float(ge.norm()))
    assert not bad, bad


# ---- 6. plans and capture -------------------------------------------------------------------------------------------------------

def _train_model(am, images, targets, **kw):
    am.reset_default_graph()
    return am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=True,
                       annealing_schedules=ao.TRAINING_ANNEALING, seed=0, noise_seed=0, gemm_precision="bf16", **kw, **HP)


def test_gaussian_plans_are_the_unfolded_bernoulli_plans_and_replays_equal_eager_steps(am):
    B = 8
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=3)
    params = ao.init_params(HP, 0)
    bern = _train_model(am, images, targets, compose_fold=False)
    bern_kernels = [op.kernel for op in bern.train_step_ops()]
    bern_names = [op.name for op in bern.train_step_ops()]

    res = {}
    for mode in ("eager", "graph"):
        model = _train_model(am, images, targets, likelihood="gaussian")
        model.load_state_dict(params)
        ops = model.train_step_ops()
        assert [op.name for op in ops] == bern_names and len(ops) == 23
        i = bern_names.index("compose_fwd")
        assert bern_kernels[i] == "write_fwd_kernel<1024>" and ops[i].kernel == "write_fwd_gauss_kernel<1024>"
        assert [op.kernel for j, op in enumerate(ops) if j != i] == [k for j, k in enumerate(bern_kernels) if j != i]
        if mode == "graph":
            model.capture_graph(steps=3)
            assert model._fold_op is None                     # the library refuses the fold: the two launches stay
            for step in range(3):
                cap = model.captured_step_ops(step)
                assert len(cap) == len(ops)
                assert "write_fwd_gauss_kernel<1024>" in [op.kernel for op in cap]
                assert "compose_write_bwd" not in [op.name for op in cap]
            model.training()
        else:
            for _ in range(3):
                model.training(eager=True)
        torch.cuda.synchronize()
        st = model.store
        assert int(model.global_step) == 3
        res[mode] = [st.params.clone(), st.m.clone(), st.v.clone(), st.params16.clone(), st.gnorm.clone(), model.scalars.clone()]
        assert bool(torch.isfinite(st.params).all())
    for a, b in zip(res["eager"], res["graph"]):
        assert torch.equal(a, b)


def test_generate_does_not_depend_on_the_likelihood(am):
    B = 8
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=3)
    params, noise = ao.init_params(HP, 0), ao.make_noise(HP, B, 4)
    scenes = {}
    for lik in ("bernoulli", "gaussian"):
        am.reset_default_graph()
        m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=False,
                        likelihood=lik, **HP)
        m.load_state_dict(params)
        m.set_dynamic(z_pres_prior_log_odds=0.0)
        m.set_generate_noise(noise)
        sc = m.generate(likelihood_noise=True)
        torch.cuda.synchronize()
        scenes[lik] = {k: getattr(sc, k).clone() for k in ("canvas", "num_digits", "scales", "shifts", "z_pres", "latents", "windows")}
        scenes[lik, "keys"] = sorted(m.state_dict())
    assert scenes["bernoulli", "keys"] == scenes["gaussian", "keys"]
    for k, v in scenes["bernoulli"].items():
        assert torch.equal(v, scenes["gaussian"][k]), k
    assert int(scenes["gaussian"]["num_digits"].sum()) > 0


# ---- 7. the constructor ---------------------------------------------------------------------------------------------------------

def test_constructor_validates_the_likelihood(am):
    images, targets = blob_canvases(4, HP["canvas_size"], HP["max_digits"], seed=3)
    xin, tin = torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda")
    am.reset_default_graph()
    with pytest.raises(ValueError, match="likelihood"):
        am.AIRModel(xin, tin, cnn=False, likelihood="poisson", **HP)
    for std in (0.0, -0.3):
        with pytest.raises(ValueError, match="vae_likelihood_std"):
            am.AIRModel(xin, tin, cnn=False, likelihood="gaussian", **dict(HP, vae_likelihood_std=std))
    # a refused constructor leaves no variable scope behind; the default is the reference's likelihood
    m = am.AIRModel(xin, tin, cnn=False, **HP)
    assert m.likelihood == "bernoulli"
    g = am.AIRModel(xin, tin, cnn=False, reuse=True, likelihood="gaussian", **HP)      # no variable of its own: it shares the scope
    assert g.likelihood == "gaussian" and g.store is m.store
    m.forward()
    g.forward()
    torch.cuda.synchronize()
    assert torch.equal(m.reconstruction, g.reconstruction)
    assert not torch.equal(m.reconstruction_loss, g.reconstruction_loss)


# ---- 8. training ----------------------------------------------------------------------------------------------------------------

def test_annealed_training_runs_and_loss_drops_under_the_gaussian_likelihood(am):
    am.reset_default_graph()
    B = 64
    images, targets = blob_canvases(B, 50, 2, seed=21)
    model = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False,
                        train=True, scope="air", annealing_schedules=ao.TRAINING_ANNEALING, likelihood="gaussian", **HP)
    losses = []
    for i in range(60):
        model.training()
        if i % 10 == 0 or i == 59:
            losses.append(float(model.loss))
    torch.cuda.synchronize()
    print("losses", losses)
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
