"""AIRModel(cnn=True) on the GPU: the conv front-end inside the step.

Cases (blob canvases of oracle.synth, noise injected with set_noise):
  A  the reference's shape: the constructor defaults, S = 50, F = 8 (Din = 1152: fused first step and panel twin in bf16), B = 6
  B  S = 21, F = 3 (Din = 75, no multiple of 4: no fusion, no Wx panel, padded twin rows), windows 11, R = 80, 2 steps, B = 5
  C  S = 33, F = 5 (Din = 320), R = 64, 4 steps, 3 digits, B = 37
Both precisions where the assertion does not say otherwise.

Bounds, none of them taken from what the code returns:
  * products (x.Wx at K = Din, d_rnn_input at K = 4R): |got - float64 product of the operands as the kernel rounds them|.max()
    / sqrt(K) < 2e-6 (fp32) / 2e-5 (bf16), the plain-product bound of tests/test_gpu_gemm_edges.py;
  * dWx: rtol 1e-5, atol 2e-6 sqrt(K) 4 max|ref| with K = B, the bound of test_wgrad_grouped (tests/test_gpu_kernels.py);
  * gnorm: 1e-5 relative to the float64 norm of the flat gradient (tests/test_gpu_kernels.py);
  * Adam: m rtol 1e-5 / atol 1e-9, v rtol 1e-5 / atol 1e-12, p atol 2e-7 (tests/test_gpu_optimizer_edges.py);
  * everything else is bit-equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import air_oracle as ao  # noqa: E402
from oracle.synth import blob_canvases  # noqa: E402

CASES = {
    "A": dict(B=6, F=8, hp={}),
    "B": dict(B=5, F=3, hp=dict(canvas_size=21, windows_size=11, rnn_units=80, max_steps=2)),
    "C": dict(B=37, F=5, hp=dict(canvas_size=33, rnn_units=64, max_steps=4, max_digits=3)),
}
PRECS = ("fp32", "bf16")
GEMM_TOL = {"fp32": 2e-6, "bf16": 2e-5}


@pytest.fixture(scope="module")
def am():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model
    return air_model


def _np(t):
    return t.detach().cpu().numpy()


def _bf16(x):
    return torch.as_tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _operand(x, prec):
    """the operand as the GEMM kernels round it on the way in"""
    return _bf16(x) if prec == "bf16" else np.asarray(x, np.float64)


def _hp(case):
    return dict(ao.DEFAULT_HP, **CASES[case]["hp"])


def _inputs(case):
    hp, B = _hp(case), CASES[case]["B"]
    images, targets = blob_canvases(B, hp["canvas_size"], hp["max_digits"], seed=11)
    return images, targets, ao.make_noise(hp, B, 1)


def _model(am, case, prec, train=True, scope="air", cnn=True, backward="exact", noise=True, reset=True, **kw):
    if reset:
        am.reset_default_graph()
    images, targets, nz = _inputs(case)
    m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=cnn,
                    cnn_filters=CASES[case]["F"], train=train, scope=scope, gemm_precision=prec, backward=backward, seed=3,
                    **dict(_hp(case), **kw))
    if noise:
        m.set_noise(nz)
    return m


def _fwd_bwd(m):
    """forward, loss and the whole backward into the flat gradient buffer; no optimizer"""
    m.forward()
    m._run_backward(m._stream())
    torch.cuda.synchronize()


def _reference_cnn(m):
    """air.cnn.CNN carrying the model's six variables"""
    from air.cnn import CNN
    ref = CNN(m.canvas_size, m.cnn_filters, device="cuda")
    ref.load_variables(m.variables)
    return ref


# ---------------------------------------------------------------------------------------------------------- 1. front-end
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_rnn_input_is_the_cnn_op(am, case, train):
    m = _model(am, case, "bf16", train=train)
    m.forward()
    torch.cuda.synchronize()
    S, F = m.canvas_size, m.cnn_filters
    assert tuple(m.rnn_input.shape) == (m.batch_size, (S // 4) ** 2 * F) and m.rnn_input is not m.input_images
    with torch.no_grad():
        ref = _reference_cnn(m)(m.input_images)
    assert float(ref.abs().max()) > 0
    assert torch.equal(m.rnn_input, ref)


# --------------------------------------------------------------------------------------------------------- 2. x.Wx at Din
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_first_step_gates_at_din(am, case, prec):
    m = _model(am, case, prec)
    m.forward()
    torch.cuda.synchronize()
    Din, R = m.store.dims["Din"], m.rnn_units
    Wx = _np(m.variables["rnn/kernel"])[:Din]
    bias = _np(m.variables["rnn/bias"]).astype(np.float64)
    ref = _operand(_np(m.rnn_input), prec) @ _operand(Wx, prec) + bias
    got = _np(m.xw).astype(np.float64).sum(0) + bias          # split-K slabs; ONE slab (the raw product) where step 0 is fused
    err = np.abs(got - ref).max() / np.sqrt(Din)
    print("x.Wx %s %s: Din %d, fused %s, error / sqrt(K) = %.3g (bound %.0e)" % (case, prec, Din, m._fuse_step0, err, GEMM_TOL[prec]))
    assert np.abs(ref - bias).max() > 1e-2                        # (a product, not zeros)
    assert err < GEMM_TOL[prec]
    if m._fuse_step0:
        # ... and what the fused epilogue made of it: acts[0] = sigmoid(i), tanh(j), sigmoid(f + 1), sigmoid(o), inverted
        a = _np(m.acts[0]).astype(np.float64)
        logit = lambda s: np.log(s) - np.log1p(-s)           # noqa: E731
        pre = np.concatenate([logit(a[:, :R]), np.arctanh(a[:, R:2 * R]), logit(a[:, 2 * R:3 * R]) - 1.0, logit(a[:, 3 * R:])], 1)
        assert np.abs(ref).max() < 6.0                            # (the inversion is well conditioned there)
        err = np.abs(pre - ref).max() / np.sqrt(Din)
        print("  acts[0] pre-image: error / sqrt(K) = %.3g" % err)
        assert err < GEMM_TOL[prec]


# ------------------------------------------------------------------------------------------- 3. downstream is untouched
def _zero_wx_pair(am, case, prec):
    """a cnn=False and a cnn=True model on the same images, noise and variables: Wh copied, Wx zero in both"""
    m0 = _model(am, case, prec, scope="plain", cnn=False)
    m1 = _model(am, case, prec, scope="conv", cnn=True, reset=False)
    D, Din = m0.store.dims["D"], m1.store.dims["Din"]
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, v in m0.variables.items():
            if v.dim() == 1:
                # (with zero biases and Wx = 0 the LSTM's state stays zero and no gradient reaches its gates)
                v.copy_((torch.rand(v.shape, generator=gen) * 0.6 - 0.3).to(v.device))
        for k, v in m0.variables.items():
            if k == "rnn/kernel":
                v[:D].zero_()
                m1.variables[k][:Din].zero_()
                m1.variables[k][Din:].copy_(v[D:])
            else:
                m1.variables[k].copy_(v)
    m0.store.touch()
    m1.store.touch()
    return m0, m1


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_downstream_of_the_lstm_input_is_untouched(am, case, prec):
    m0, m1 = _zero_wx_pair(am, case, prec)
    _fwd_bwd(m0)
    _fwd_bwd(m1)
    D, Din, B = m0.store.dims["D"], m1.store.dims["Din"], m1.batch_size
    bad = []
    for k in ("loss", "accuracy", "reconstruction", "reconstruction_loss", "rec_num_digits", "loss_per_item", "rec_scales",
              "rec_shifts", "rec_windows", "rec_latents", "z_pres_probs", "z_pres_kls", "scale_kls", "shift_kls", "vae_kls",
              "rec_st_back", "dgsum"):
        if not torch.equal(getattr(m0, k), getattr(m1, k)):
            bad.append(k)
    assert float(m1.dgsum.abs().max()) > 0
    for k, g0 in m0.gradients.items():
        g1 = m1.gradients[k]
        if k == "rnn/kernel":
            g0, g1 = g0[D:], g1[Din:]
        if not torch.equal(g0, g1):
            bad.append("d " + k)
    assert not bad, bad
    for k in m1.store.cnn_names:
        assert float(m1.gradients[k].abs().max()) == 0.0, k
    # dWx of the conv model from its own buffers
    A, dY = _operand(_np(m1.rnn_input), prec), _operand(_np(m1.dgsum), prec)
    ref = A.T @ dY
    got = _np(m1.gradients["rnn/kernel"])[:Din]
    print("dWx %s %s: max |got - ref| = %.3g, max |ref| = %.3g" % (case, prec, np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=2e-6 * np.sqrt(B) * 4 * np.abs(ref).max())


# ------------------------------------------------------------------------------------------ 4. backward into the CNN
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_backward_into_the_cnn(am, case, prec):
    m = _model(am, case, prec)
    _fwd_bwd(m)
    Din, R = m.store.dims["Din"], m.rnn_units
    Wx = _np(m.variables["rnn/kernel"])[:Din]
    ref = _operand(_np(m.dgsum), prec) @ _operand(Wx, prec).T
    got = _np(m.d_rnn_input).astype(np.float64)
    err = np.abs(got - ref).max() / np.sqrt(4 * R)
    print("d_rnn_input %s %s: error / sqrt(K) = %.3g (bound %.0e), max |ref| %.3g, max |dgsum| %.3g"
          % (case, prec, err, GEMM_TOL[prec], np.abs(ref).max(), float(m.dgsum.abs().max())))
    assert np.abs(ref).max() > 0
    assert err < GEMM_TOL[prec]
    # the six gradients in the flat buffer: the op's own backward of the same module with d_out = the model's d_rnn_input
    mod = _reference_cnn(m)
    out = mod(m.input_images)
    assert torch.equal(out.detach(), m.rnn_input)
    out.backward(m.d_rnn_input)
    torch.cuda.synchronize()
    for k, q in zip(m.store.cnn_names, mod._params()):
        assert float(q.grad.abs().max()) > 0, k
        assert torch.equal(m.gradients[k], q.grad), k


# -------------------------------------------------------------------------------------------------- 5. clip and Adam
WX_SCALE = 4.0     # Wx times this: the conv gradients (proportional to it) then carry a tenth of the squared norm and more


def _heavy_wx_model(am, prec, **kw):
    m = _model(am, "A", prec, **kw)
    with torch.no_grad():
        m.variables["rnn/kernel"][:m.store.dims["Din"]].mul_(WX_SCALE)
    m.store.touch()
    return m


def _flat_norms(m):
    g = m.store.grads[:m.store.n].double()
    conv = sum(float((m.gradients[k].double() ** 2).sum()) for k in m.store.cnn_names)
    return float(g.norm()), conv / float((g ** 2).sum())


@pytest.mark.parametrize("prec", PRECS)
def test_global_norm_counts_the_conv_gradients_and_adam_updates_them(am, prec):
    m = _heavy_wx_model(am, prec)
    before = {k: _np(v).astype(np.float64) for k, v in m.variables.items()}
    m.training(eager=True)
    torch.cuda.synchronize()
    norm, share = _flat_norms(m)
    got = float(m.store.gnorm)
    print("gnorm %s: %.6g against %.6g (float64), conv share of the squared norm %.3f, without it the norm would be %.6g"
          % (prec, got, norm, share, norm * np.sqrt(1 - share)))
    assert share >= 0.10                           # leaving the conv partials out moves the norm by >= 5 %: 5000 x the bound
    assert abs(got - norm) / norm < 1e-5
    # one step of the oracle's clip + Adam on the model's own gradients
    grads = {k: _np(v).astype(np.float64) for k, v in m.gradients.items()}
    f32 = lambda x: float(np.float32(x))                  # noqa: E731  (what the kernels receive, as float64)
    clipped, gn = ao.clip_by_global_norm(grads, f32(m.gradient_clipping_norm))
    assert abs(float(gn) - norm) / norm < 1e-12
    p64 = {k: v.copy() for k, v in before.items()}
    m64 = {k: np.zeros_like(v) for k, v in before.items()}
    v64 = {k: np.zeros_like(v) for k, v in before.items()}
    ao.adam_step(p64, clipped, m64, v64, 1, f32(m.learning_rate), f32(0.9), f32(0.999), f32(1e-8))
    for k in m.store.cnn_names:
        assert np.abs(p64[k]).max() <= 1.0
        np.testing.assert_allclose(_np(m.store.adam_m[k]), m64[k], rtol=1e-5, atol=1e-9, err_msg=k)
        np.testing.assert_allclose(_np(m.store.adam_v[k]), v64[k], rtol=1e-5, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(_np(m.variables[k]), p64[k], rtol=0, atol=2e-7, err_msg=k)
        if k.endswith("kernel"):
            assert np.abs(_np(m.variables[k]) - before[k]).max() > 1e-4, k       # (it moved)


def test_global_norm_on_the_data_parallel_path(am, tmp_path, monkeypatch):
    """AIR_DP_FORCE=1 on a process group of one rank: backward -> exchange -> air_grad_sqnorm over the flat buffer -> Adam"""
    import torch.distributed as dist
    monkeypatch.setenv("AIR_DP_FORCE", "1")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "pg"), 1), rank=0, world_size=1)
    try:
        m = _heavy_wx_model(am, "bf16")
        assert m._dp()
        m.training(eager=True)
        torch.cuda.synchronize()
        norm, share = _flat_norms(m)
        got = float(m.store.gnorm)
    finally:
        dist.destroy_process_group()
    print("gnorm on the data-parallel path: %.6g against %.6g, conv share %.3f" % (got, norm, share))
    assert share >= 0.10
    assert abs(got - norm) / norm < 1e-5


# ----------------------------------------------------------------------------------------------------------- 6. capture
def _train_state(m):
    st = m.store
    torch.cuda.synchronize()
    return {k: getattr(st, k).clone() for k in ("params", "m", "v", "grads", "gnorm", "istate")} | {"scalars": m.scalars.clone()}


@pytest.mark.parametrize("hook", [False, True])
@pytest.mark.parametrize("prec", PRECS)
def test_captured_steps_equal_eager_steps(am, prec, hook):
    """three eager steps against ONE replay of three captured steps from the same state: a replayed step that read a twin of
    rnn_input left by an earlier step (the conv variables have moved since) would differ from its eager self"""
    m = _model(am, "A", prec, backward="reference", noise=False, learning_rate=1e-2)    # (device RNG, keyed by global_step)
    sd0 = m.state_dict()
    for _ in range(3):
        m.training(eager=True)
    eager = _train_state(m)
    assert int(m.global_step) == 3
    m.load_state_dict(sd0)
    src = m.input_images.clone()
    m.capture_graph(steps=3, between_steps=(lambda i: m.input_images.copy_(src)) if hook else None)
    kernels = m.captured_xwx_kernels()
    m.training()
    replay = _train_state(m)
    bad = [k for k in eager if not torch.equal(eager[k], replay[k])]
    assert not bad, bad
    assert m._xwx_twin_op is None and len(kernels) == 3 and not any("glds" in k for k in kernels), kernels
    assert all(op.name.startswith("xWx") and "16" not in op.name.split("[")[0] for op in m.captured_xwx_ops())
    # (the conv variables did move between the steps, or the test above shows nothing)
    k1 = torch.as_tensor(np.asarray(sd0["cnn/conv1/kernel"])).to(m.variables["cnn/conv1/kernel"].device)
    assert float((m.variables["cnn/conv1/kernel"] - k1).abs().max()) > 1e-3


@pytest.mark.parametrize("prec", PRECS)
def test_inference_forward_graph_equals_eager(am, prec):
    m = _model(am, "A", prec, train=False, noise=False)
    m.forward()
    torch.cuda.synchronize()
    eager = {k: getattr(m, k).clone() for k in ("rnn_input", "reconstruction", "loss", "rec_num_digits", "att")}
    m.capture_graph()
    m.rnn_input.zero_()
    m.forward()
    torch.cuda.synchronize()
    assert m._graph is not None
    bad = [k for k in eager if not torch.equal(eager[k], getattr(m, k))]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------ 7. launch list
def _tags(m):
    return [op.name.split("[")[0] for op in m.train_step_ops()]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_steps", [3, 1])
def test_launch_list(am, prec, max_steps):
    plain = _tags(_model(am, "A", prec, cnn=False, backward="reference", noise=False, max_steps=max_steps))
    conv = _tags(_model(am, "A", prec, backward="reference", noise=False, max_steps=max_steps))
    at = plain.index("wgrad_grouped")
    assert plain[at - 1] == ("bptt_lstm_bwd" if max_steps > 1 else "dh_heads")
    assert conv == ["cnn_fwd"] + plain[:at] + ["dgrad_rnn_input", "cnn_bwd"] + plain[at:]
    if max_steps == 3 and prec == "bf16":                 # (the fp32 path does not fuse the first step: three launches more)
        assert len(plain) == 23 and len(conv) == 26


# ---------------------------------------------------------------------------------------- 8. persistence and refusals
def test_state_dict_and_tf_bundle_round_trip(am, tmp_path):
    m = _heavy_wx_model(am, "bf16")
    m.training(eager=True)                               # (non-trivial Adam slots and global_step)
    torch.cuda.synchronize()
    sd = m.state_dict()
    for k in m.store.cnn_names:
        assert k in sd and k + "/Adam" in sd and k + "/Adam_1" in sd
        assert float(sd[k + "/Adam_1"].abs().max()) > 0
    prefix = str(tmp_path / "air-model")
    m.save_tf_checkpoint(prefix)
    import tf_checkpoint as tfc
    names = set(tfc.load_checkpoint(prefix))
    for k in m.store.cnn_names:                          # the scope cnn/ sits beside rnn/, not under it
        assert {"air/" + k, "air/training/air/" + k + "/Adam", "air/training/air/" + k + "/Adam_1"} <= names, k
    assert "air/rnn/rnn/kernel" in names and not any(n.startswith("air/rnn/cnn") for n in names)
    for how in ("state_dict", "bundle"):
        m2 = _model(am, "A", "bf16", scope="restored_" + how, reset=False)
        if how == "state_dict":
            m2.load_state_dict(sd)
        else:
            m2.load_tf_checkpoint(prefix)
        for k in ("params", "m", "v"):
            assert torch.equal(getattr(m.store, k), getattr(m2.store, k)), (how, k)
        assert int(m2.global_step) == int(m.global_step) == 1
    # a cnn=False bundle into a cnn=True model: refused, nothing written
    plain = _model(am, "A", "bf16", scope="plain", cnn=False, reset=False)
    pprefix = str(tmp_path / "plain-model")
    plain.save_tf_checkpoint(pprefix)
    keep = m.store.params.clone()
    with pytest.raises((KeyError, ValueError)):
        m.load_tf_checkpoint(pprefix)
    assert torch.equal(m.store.params, keep)


def test_refusals_leave_no_scope_behind(am):
    am.reset_default_graph()
    images, targets, _ = _inputs("A")
    x, t = torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda")
    with pytest.raises(NotImplementedError, match="factors"):
        am.AIRModel(x, t, cnn=True, train=True, scope="r1", dp_exchange="factors")
    with pytest.raises(NotImplementedError, match="50.*9"):
        am.AIRModel(x, t, cnn=True, cnn_filters=9, scope="r2")
    big = torch.zeros(2, 78 * 78, device="cuda")
    with pytest.raises(NotImplementedError, match="78.*8"):
        am.AIRModel(big, None, cnn=True, canvas_size=78, scope="r3")
    with pytest.raises(ValueError):
        am.AIRModel(x, t, cnn=True, cnn_filters=0, scope="r4")
    assert not am._SCOPES
    with pytest.raises(NotImplementedError, match="cnn=True.*cnn=False"):
        am.AIRModel(x, t, scope="r5", train=True)            # `cnn` left out: refused as before, the caller chooses
    assert not am._SCOPES
    m = am.AIRModel(x, t, cnn=True, scope="r5", train=True)
    assert m.cnn and m.cnn_filters == 8 and m.store.dims["Din"] == 1152
    for kw in (dict(cnn=False), dict(cnn=True, cnn_filters=4)):
        with pytest.raises(ValueError, match="different"):
            am.AIRModel(x, t, scope="r5", reuse=True, **kw)
    for call in (m.var_summaries, m.grad_summaries, m.var_summary_names, m.grad_summary_names):
        with pytest.raises(NotImplementedError):
            call()
    m.forward()
    assert m.numeric_summaries().numel() == len(m.summary_names())
    scenes = m.generate()
    torch.cuda.synchronize()
    assert tuple(scenes.canvas.shape) == (m.batch_size, 2500)
