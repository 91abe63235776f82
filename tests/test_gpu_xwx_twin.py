"""The x.Wx + first-LSTM-step launch over the padded bf16 twin of the image batch (LDS-DMA staged,
gemm_xwx_glds_kernel) against the fp32-operand launch that writes that twin: bit-identical at the launch and at the
train step, never used where the twin could be stale."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi

pytestmark = pytest.mark.gpu

from oracle import air_oracle as ao  # noqa: E402
from oracle.synth import blob_canvases  # noqa: E402

HP = dict(ao.TRAINING_HP)
AF32_NAME = "gemm_bf16tw_kernel<1, 1, false, 6, true, 40>"
GLDS_NAME = "gemm_xwx_glds_kernel<40>"
REG_NAME = "gemm_bf16tw_kernel<1, 1, false, 6, false, 40>"
PADDED, PADDED_REGISTERS = 2, 3                  # air_gemm_t.i0 of AIR_EPI_LSTM_FWD0 with A16 (include/air_hip.h)


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


@pytest.fixture(scope="module")
def am():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model
    return air_model


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _name(H, g):
    buf = C.create_string_buffer(128)
    H.check(H.lib().air_gemm_kernel_name(C.byref(g), buf, 128))
    return buf.value.decode()


def _struct(H, A, B, Cc, M, N, K, lda, **kw):
    g = H.Gemm()
    g.A, g.B, g.C = A.data_ptr(), B.data_ptr(), Cc.data_ptr()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = M, N, K, lda, N, N
    g.precision = 1
    g.epi = H.EPI_LSTM_FWD0
    for k, v in kw.items():
        setattr(g, k, v.data_ptr() if torch.is_tensor(v) else v)
    return g


def _panels(H, W):
    K, N = W.shape
    out = torch.zeros(K * N, dtype=torch.int16, device="cuda")
    pd = (H.Panel * 1)(H.Panel(0, 0, K, N, 4, 0))
    H.check(H.lib().air_panel_shadow(_p(W), _p(out), pd, 1, _stream()))
    return out


# B = 64: the benchmark's batch; 50: ragged (not a multiple of 16 -- the last row tile has 2 rows); (37, 64, 1100): a
# shorter ragged contraction (18 images, K % 64 = 12, K % 8 = 4) on the same 40-image kernel.  The 16-image kernels:
# (48, 64, 516) one round of 9 images; (20, 64, 2700) 43 images = three rounds, the last one ragged
@pytest.mark.parametrize("Bn,R,D,rounds", [(64, 256, 2500, 40), (50, 256, 2500, 40), (37, 64, 1100, 40),
                                           (48, 64, 516, 16), (20, 64, 2700, 16)])
def test_twin_launches_bit_identical_to_the_fp32_operand_launch(H, Bn, R, D, rounds):
    af32_name, glds_name, reg_name = (n.replace("40>", "%d>" % rounds) for n in (AF32_NAME, GLDS_NAME, REG_NAME))
    lib = H.lib()
    rng = np.random.RandomState(Bn + D)
    f = lambda *s: torch.tensor(rng.uniform(-1, 1, s).astype(np.float32), device="cuda")  # noqa: E731
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    X, Wx, bias = f(Bn, D).abs(), f(D, 4 * R) * 0.05, f(4 * R) * 0.1
    WxP = _panels(H, Wx)
    Dp = (D + 7) & ~7
    assert Dp != D                                             # the cases are the ones a dense twin cannot serve
    twin = torch.full((Bn, Dp), 0x7fc1, dtype=torch.int16, device="cuda")      # (NaN patterns: the pad must be WRITTEN)

    def run(**kw):
        out = dict(xw=nan(Bn, 4 * R), acts=nan(Bn, 4 * R), c=nan(Bn, R), h=nan(Bn, R),
                   h16=torch.full((Bn, R), 0x7fc1, dtype=torch.int16, device="cuda"))
        lda = kw.pop("lda", D)
        g = _struct(H, X, Wx, out["xw"], Bn, 4 * R, D, lda, bias=bias, q0=out["acts"], q1=out["c"], q2=out["h"],
                    q2_16=out["h16"], B16p=WxP, **kw)
        name = _name(H, g)
        H.check(lib.air_gemm(C.byref(g), _stream()))
        torch.cuda.synchronize()
        return name, out

    name0, ref = run(C16=twin)
    assert name0 == af32_name, name0
    # the side output: RNE bf16 of the batch in columns < D, zeros in the pad
    assert torch.equal(twin[:, :D].view(torch.bfloat16), X.to(torch.bfloat16))
    assert bool((twin[:, D:] == 0).all())
    for v in ref.values():
        assert bool(torch.isfinite(v.float()).all()) if v.dtype != torch.int16 else True
    # ... and it changes nothing of the launch's own results
    name1, plain = run()
    assert name1 == af32_name
    for k in ref:
        assert torch.equal(ref[k], plain[k]), k
    for i0, want in ((PADDED, glds_name), (PADDED_REGISTERS, reg_name)):
        name, got = run(A16=twin, lda=Dp, i0=i0)
        assert name == want, name
        for k in ("xw", "acts", "c", "h", "h16"):
            assert torch.equal(ref[k], got[k]), (want, k)
    assert torch.equal(ref["h16"].view(torch.bfloat16), ref["h"].to(torch.bfloat16))


def test_padded_twin_needs_the_twin_kernel(H):
    """C16 of AIR_EPI_LSTM_FWD0 is only written by the fp32-A twin kernel: a descriptor that cannot take it is refused"""
    Bn, R, D = 16, 16, 64
    X, Wx = torch.zeros(Bn, D, device="cuda"), torch.zeros(D, 4 * R, device="cuda")
    o = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    twin = torch.zeros(Bn, D, dtype=torch.int16, device="cuda")
    g = _struct(H, X, Wx, o(Bn, 4 * R), Bn, 4 * R, D, D, q0=o(Bn, 4 * R), q1=o(Bn, R), q2=o(Bn, R), C16=twin)   # no bf16 B at all
    assert H.lib().air_gemm(C.byref(g), _stream()) != 0
    torch.cuda.synchronize()


# R = 100, 20: four-unit tiles exist (R % 4 == 0) but the twin kernels want R % 8 == 0; (64, None): no panel twin of Wx
@pytest.mark.parametrize("R,panels", [(100, True), (20, True), (64, False)])
def test_padded_twin_forms_are_refused_where_the_twin_kernels_do_not_serve_them(H, R, panels):
    """Both padded-twin forms of AIR_EPI_LSTM_FWD0 -- C16 out, A16 in with lda = the twin's stride -- are refused by the
    launch AND by the name query when the descriptor is not the twin kernels'; the plain descriptor of the same shape
    still runs on the fp32-operand kernel, and an ORDINARY A16 twin (no padded flag, lda = A's) still does too."""
    lib = H.lib()
    Bn, D = 32, 516
    Dp = (D + 7) & ~7
    rng = np.random.RandomState(R)
    f = lambda *s: torch.tensor(rng.uniform(-1, 1, s).astype(np.float32), device="cuda")  # noqa: E731
    X, Wx, bias = f(Bn, D).abs(), f(D, 4 * R) * 0.05, f(4 * R) * 0.1
    WxP = _panels(H, Wx) if panels else None
    twin = torch.zeros(Bn, Dp, dtype=torch.int16, device="cuda")
    twin[:, :D] = X.to(torch.bfloat16).view(torch.int16)
    buf = C.create_string_buffer(128)

    def desc(out, lda=D, **kw):
        if WxP is not None:
            kw["B16p"] = WxP
        return _struct(H, X, Wx, out[0], Bn, 4 * R, D, lda, bias=bias, q0=out[1], q1=out[2], q2=out[3], **kw)

    outs = lambda: [torch.full(s, float("nan"), device="cuda") for s in ((Bn, 4 * R), (Bn, 4 * R), (Bn, R), (Bn, R))]  # noqa: E731
    ref = outs()
    g = desc(ref)
    assert _name(H, g).startswith("gemm_bf16v2_kernel<1, 1, false, 6>")
    H.check(lib.air_gemm(C.byref(g), _stream()))
    torch.cuda.synchronize()
    for kw in (dict(C16=twin), dict(A16=twin, lda=Dp, i0=PADDED), dict(A16=twin, lda=Dp, i0=PADDED_REGISTERS)):
        got = outs()
        g = desc(got, **kw)
        assert lib.air_gemm_kernel_name(C.byref(g), buf, 128) == -3, kw.keys()
        assert lib.air_gemm(C.byref(g), _stream()) == -3, kw.keys()
        torch.cuda.synchronize()
        assert bool(torch.isnan(got[0]).all())                  # nothing ran
    # an ordinary twin of A (same leading dimension, no flag): served by the fp32-operand kernel from A itself
    dense = X.to(torch.bfloat16).view(torch.int16).contiguous()
    got = outs()
    g = desc(got, A16=dense)
    assert _name(H, g).startswith("gemm_bf16v2_kernel<1, 1, false, 6>")
    H.check(lib.air_gemm(C.byref(g), _stream()))
    torch.cuda.synchronize()
    for a0, a1 in zip(ref, got):
        assert torch.equal(a0, a1)


def _model(am, images, targets, scope="air", hp=HP, **kw):
    am.reset_default_graph()
    return am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=True,
                       scope=scope, annealing_schedules=ao.TRAINING_ANNEALING, seed=0, noise_seed=0, gemm_precision="bf16",
                       **kw, **hp)


def _state(model):
    torch.cuda.synchronize()
    st = model.store
    return dict(params=st.params.clone(), m=st.m.clone(), v=st.v.clone(), loss=model.loss.clone(),
                step=int(st.istate[0]))


def _same(a, b):
    for k in ("params", "m", "v", "loss"):
        assert torch.equal(a[k], b[k]), k
    assert a["step"] == b["step"]


def test_four_step_replay_equals_four_eager_steps_and_is_never_stale(am):
    B = 64
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=3)
    images2, _ = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=11)
    assert not np.array_equal(images, images2)
    params = ao.init_params(HP, 0)

    eager = _model(am, images, targets)
    eager.load_state_dict(params)
    for _ in range(4):
        eager.training(eager=True)
    e4 = _state(eager)
    assert eager.captured_xwx_kernels() is None

    graph = _model(am, images, targets)
    graph.load_state_dict(params)
    graph.capture_graph(steps=4)
    assert graph.captured_xwx_kernels() == [AF32_NAME] + [GLDS_NAME] * 3
    ops = graph.captured_xwx_ops()                          # the ops that were enqueued under capture, by identity
    assert ops[0] is graph._fwd[0] and all(op is graph._xwx_twin_op for op in ops[1:])
    graph.training()
    g4 = _state(graph)
    _same(e4, g4)
    assert g4["step"] == 4
    # the padded twin is the bf16 image of the batch, pad zero
    D = images.shape[1] * images.shape[2] if images.ndim == 3 else images.shape[1]
    tw = graph.images16p
    assert torch.equal(tw[:, :D].view(torch.bfloat16), graph.input_images.reshape(B, D).to(torch.bfloat16))
    assert bool((tw[:, D:] == 0).all())
    sd4 = graph.state_dict()

    # staleness: new images written in place from the host, then the next replay -- step 0 of it must read THEM
    graph.input_images.copy_(torch.tensor(images2, device="cuda").reshape(graph.input_images.shape))
    graph.training()
    g8 = _state(graph)
    assert g8["step"] == 8

    fresh = _model(am, images2, targets)
    fresh.load_state_dict(sd4)
    for _ in range(4):
        fresh.training(eager=True)
    _same(_state(fresh), g8)
    assert not torch.equal(g8["params"], g4["params"])


def test_dispatch_keeps_the_fp32_operand_launch_where_the_twin_is_not_provable(am):
    B = 16
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=5)
    model = _model(am, images, targets)
    model.load_state_dict(ao.init_params(HP, 0))
    # a between_steps hook may rewrite the batch between two steps of a replay: every step reads the fp32 batch
    model.capture_graph(steps=3, between_steps=lambda i: None)
    assert model.captured_xwx_kernels() == [AF32_NAME] * 3
    model.training()
    model.release_graph()
    # one-step graphs: step 0 only
    model.capture_graph(steps=1)
    assert model.captured_xwx_kernels() == [AF32_NAME]
    model.release_graph()
    # the eager list (bench --full, profiling tools) is the fp32-operand step
    assert model.train_step_ops()[0].kernel == AF32_NAME
    # the A/B arm: the same operands through registers
    reg = _model(am, images, targets, scope="air_reg", xwx_twin_staging="registers")
    reg.load_state_dict(ao.init_params(HP, 0))
    reg.capture_graph(steps=2)
    assert reg.captured_xwx_kernels() == [AF32_NAME, REG_NAME]
    assert reg.captured_xwx_ops()[1] is reg._xwx_twin_op
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        _model(am, images, targets, scope="air_bad", xwx_twin_staging="dma")
    # the fp32 path and train=False models have no twin op at all
    am.reset_default_graph()
    f32 = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=True,
                      scope="air", gemm_precision="fp32", **HP)
    assert f32._xwx_twin_op is None
    te = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=False,
                     reuse=True, scope="air", gemm_precision="fp32", **HP)
    assert te._xwx_twin_op is None and te.images16p is None


@pytest.mark.parametrize("R", [20, 100])
def test_models_the_twin_kernel_does_not_serve_train_on_the_fp32_operand_launch(am, R):
    """rnn_units % 8 == 4: the store still builds the gate-interleaved panel of Wx, but the fused x.Wx launch is the
    fp32-operand kernel's (gemm_bf16v2_kernel), which neither writes nor reads the padded twin.  Such a model trains as
    it did: eagerly and through a multi-step graph, bit-identically, with no twin kernel in the graph."""
    B = 16
    hp = dict(HP, rnn_units=R)
    images, targets = blob_canvases(B, hp["canvas_size"], hp["max_digits"], seed=7)
    params = ao.init_params(hp, 0)
    eager = _model(am, images, targets, hp=hp)
    eager.load_state_dict(params)
    assert eager._xwx_twin_op is None
    assert eager.train_step_ops()[0].kernel.startswith("gemm_bf16v2_kernel<1, 1, false, 6>")
    for _ in range(2):
        eager.training(eager=True)
    e2 = _state(eager)
    assert e2["step"] == 2 and bool(torch.isfinite(e2["loss"]))
    graph = _model(am, images, targets, hp=hp)
    graph.load_state_dict(params)
    graph.capture_graph(steps=2)
    names = graph.captured_xwx_kernels()
    assert len(names) == 2 and all(n.startswith("gemm_bf16v2_kernel<1, 1, false, 6>") for n in names), names
    graph.training()
    _same(e2, _state(graph))
