"""HIP path vs vectors produced by EXECUTING the reference's own saved graph
(tests/golden/graph_b64.npz, written by tests/golden/make_graph_golden.py from
/root/reference/model/air-model.meta; the reference itself does not travel to the GPU box).

  * whole model, fp32: forward outputs / ELBO vs the graph's (same tolerances as vs the oracle);
    backward="exact" gradients and the clipped Adam update vs the graph evaluated in fp64;
  * kernel level, identical inputs: `air_write_bwd(literal=2)` -- the default backward="reference" --
    reproduces the graph's UnsortedSegmentSum result (d loss / d vae_recon, rounding residue of the
    out-of-range taps included) BIT FOR BIT, and the gradients wrt (s, x, y, z_pres) to <= 1e-5;
    `air_attend_bwd(literal=2)`: gradients wrt the seven head outputs vs the graph's AddN_27..32;
  * whole model, backward="reference": per-variable gradient norms carry the same residue as the
    graph's fp32 backward (the two differ element-wise only because upstream expf/logf/GEMM rounding
    differs by an ulp, which the residue amplifies chaotically -- compared in magnitude).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_check as abi

pytestmark = pytest.mark.gpu

from oracle import air_oracle as ao  # noqa: E402
from oracle.synth import blob_canvases  # noqa: E402

HP = dict(ao.TRAINING_HP)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "graph_b64.npz")
GOLD_KERN = os.path.join(os.path.dirname(__file__), "golden", "graph_b64_kern.npz")   # its kern/* vectors (1 MiB per file)
SEEDS = dict(images=3, params=0, noise=1)            # tests/golden/make_graph_golden.py
KB, SUB = 16, 2048


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g.update(np.load(GOLD_KERN))
    return g


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _inputs(batch=64, seed_images=SEEDS["images"], seed_noise=SEEDS["noise"]):
    images, targets = blob_canvases(batch, HP["canvas_size"], HP["max_digits"], seed=seed_images)
    return images, targets, ao.init_params(HP, SEEDS["params"]), ao.make_noise(HP, batch, seed_noise)


def _subsample_index(name, numel):
    if numel <= 2 * SUB:
        return np.arange(numel)
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return np.sort(np.random.RandomState(abs(h) % (2 ** 31)).choice(numel, SUB, replace=False))


def _model(batch, train, lo, backward="exact", prec="fp32", **kw):
    from air import air_model as am
    images, targets, params, noise = _inputs(batch, **kw)
    am.reset_default_graph()
    m = am.AIRModel(_cuda(images), _cuda(targets, torch.int32), cnn=False, train=train, scope="air",
                    gemm_precision=prec, backward=backward, **HP)
    m.load_state_dict(params)
    m.set_noise(noise)
    m.set_dynamic(z_pres_prior_log_odds=float(lo))
    return m, images, params


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ whole model vs the graph

@pytest.mark.parametrize("tag,batch,train,kw", [("train0", 64, True, {}),
                                                ("train3000", 64, True, dict(seed_images=11, seed_noise=7)),
                                                ("test40000_b4", 4, False, {})])
def test_forward_matches_executed_graph(gold, tag, batch, train, kw):
    m, images, _ = _model(batch, train, gold[tag + "/z_pres_prior_log_odds"], **kw)
    m.forward()
    torch.cuda.synchronize()
    assert m.steps_executed == int(gold[tag + "/steps_executed"])
    assert np.array_equal(_np(m.rec_num_digits), gold[tag + "/rec_num_digits"])
    assert abs(float(m.accuracy) - float(gold[tag + "/accuracy"])) < 1e-6
    assert abs(float(m.loss) - float(gold[tag + "/loss"])) / abs(float(gold[tag + "/loss"])) <= 1e-2
    for k in ("z_pres_kls", "vae_kls"):
        np.testing.assert_allclose(_np(getattr(m, k)), gold[tag + "/" + k], rtol=2e-4, atol=2e-4)
    if tag != "train3000":
        assert np.abs(_np(m.reconstruction) - gold[tag + "/reconstruction"]).max() <= 2e-5
        for k in ("rec_scales", "rec_shifts", "rec_st_back", "z_pres_probs", "scale_kls", "shift_kls"):
            g = gold[tag + "/" + k]
            assert np.abs(_np(getattr(m, k)) - g).max() <= 5e-5 * max(1.0, np.abs(g).max()), k
    if tag == "train0":
        assert np.abs(_np(m.rec_windows)[:KB] - gold["train0/rec_windows_first"]).max() <= 5e-5
    if tag == "test40000_b4":
        assert np.abs(_np(m.rec_windows) - gold[tag + "/rec_windows"]).max() <= 5e-5


def test_exact_backward_and_adam_match_graph_fp64(gold):
    m, images, params = _model(64, True, gold["train0/z_pres_prior_log_odds"], backward="exact")
    p0 = {k: _np(v).astype(np.float64) for k, v in m.variables.items()}
    m.training()
    torch.cuda.synchronize()
    worst = {}
    for k, g in m.gradients.items():
        idx = _subsample_index(k, g.numel())
        got = _np(g).reshape(-1)[idx].astype(np.float64)
        ref = gold["train0/grad64_sub/" + k]
        worst[k] = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
        tol = 2e-2 if k.startswith(("z_pres/", "rnn/")) else 5e-3
        assert worst[k] < tol, (k, worst[k])
    gn = float(m.store.gnorm[0])
    assert abs(gn - float(gold["train0/global_norm_fp64"])) / float(gold["train0/global_norm_fp64"]) < 2e-3
    for k, v in m.variables.items():
        idx = _subsample_index(k, v.numel())
        d = (_np(v).astype(np.float64) - p0[k]).reshape(-1)[idx]
        ref = gold["train0/adam64_delta_sub/" + k]
        if np.linalg.norm(ref) > 0:
            # first Adam step: every element moves by ~lr * sign(g); elements with g ~ 0 may flip
            assert np.linalg.norm(d - ref) / np.linalg.norm(ref) < 5e-2, k


def test_reference_backward_carries_the_graphs_residue(gold):
    """backward="reference": same order of magnitude per variable as the graph's own fp32 backward
    (|g| 1.6e6 against 1.1e3 exact at initialisation), far above what the exact adjoint gives.

    Why only a magnitude band (0.2-5x per tensor) and not element-wise equality: the residue is
    ulp(partial sum ~1e11) of a cancellation, so a last-ulp difference in ANY upstream expf / logf / GEMM
    accumulation reshuffles it completely -- two correct fp32 evaluations of the same graph disagree
    element-wise.  The band is acceptable ONLY because the two kernels that create and consume the residue
    are teacher-forced on the graph's own tensors and compared exactly: air_write_bwd(literal=2) bit for
    bit against the graph's UnsortedSegmentSum output (test_write_bwd_reproduces_the_graphs_scatter_bit_for_bit,
    and at every canvas regime vs the graph-pinned oracle in
    test_gpu_kernels.py::test_write_bwd_graph_order_matches_oracle_all_canvas_sizes), air_attend_bwd(literal=2)
    <= 1e-4 against AddN_27..32 (test_attend_bwd_matches_graph_head_gradients)."""
    m, _, _ = _model(64, True, gold["train0/z_pres_prior_log_odds"], backward="reference")
    m.training()
    torch.cuda.synchronize()
    gn = float(m.store.gnorm[0])
    ref = float(gold["train0/global_norm_fp32"])
    print("reference |g| / graph sequential:", {"global": "%.2f" % (gn / ref), **{
        k: "%.2f" % (float(g.double().norm()) / float(gold["train0/grad32_norm/" + k])) for k, g in m.gradients.items() if g.numel() >= 16}})
    assert 0.25 < gn / ref < 4.0, (gn, ref)
    for k, g in m.gradients.items():
        if g.numel() < 16:
            continue                      # one- and two-element biases: a single residue realisation each
        a, b = float(g.double().norm()), float(gold["train0/grad32_norm/" + k])
        assert 0.2 < a / b < 5.0, (k, a, b)
    # the heads of z_pres see no sampler residue: they agree with the exact math
    for k in ("z_pres/log_odds/output/biases", "z_pres/log_odds/output/weights"):
        a, b = float(m.gradients[k].double().norm()), float(gold["train0/grad64_norm/" + k])
        assert abs(a - b) / b < 0.1, (k, a, b)


# ------------------------------------------------------------------ kernel level, identical inputs

def _att(H, gold, N):
    att = np.zeros((N, KB, H.ATT_STRIDE), np.float32)
    for t in range(N):
        k = "kern/t%d/" % t
        att[t, :, H.ATT_S], att[t, :, H.ATT_X], att[t, :, H.ATT_Y] = gold[k + "s"], gold[k + "x"], gold[k + "y"]
        att[t, :, H.ATT_Z], att[t, :, H.ATT_ZPRE] = gold[k + "z_pres"], gold[k + "z_pre"]
        att[t, :, H.ATT_MASK] = gold[k + "mask"].astype(np.float32)
        att[t, :, H.ATT_MASK_PREV] = gold[k + "mask_prev"].astype(np.float32)
    return att


@pytest.mark.parametrize("literal", [2, 4])
def test_write_bwd_reproduces_the_graphs_scatter_bit_for_bit(H, gold, golden_dir, literal):
    """literal 2 (backward="reference") against the executed graph's UnsortedSegmentSum; literal 4 ("reference_carried")
    against the SAME graph executed with that one kernel in the carried16 order (tests/golden/graph_b64_carried.npz,
    make_graph_golden.py --carried-only) -- both bit for bit.  literal 4 additionally equals literal 2's fixture on every
    window pixel whose four streams are short (the reference's own chain there), and its coordinate / z gradients
    (per-column thread sums in the graph's AddN order) are held to the graph's own tensors like literal 2's."""
    blk = np.load(os.path.join(golden_dir, "graph_b64_carried.npz"))
    N, Cc, w = int(gold["train0/steps_executed"]), HP["canvas_size"], HP["windows_size"]
    att = _cuda(_att(H, gold, N))
    # d loss / d running_recon is the same tensor at every step (the canvas is a running sum)
    g_sel = np.zeros((KB, Cc * Cc), np.float32)
    for t in range(N):
        act = gold["kern/t%d/mask" % t].astype(bool)
        g_sel[act] = gold["kern/t%d/g_select" % t].reshape(KB, -1)[act]
    d_recon = _cuda(g_sel)
    vrec = _cuda(np.stack([gold["kern/t%d/vae_recon" % t] for t in range(N)]))
    dgen = torch.full((N, KB, w * w), 7.0, device="cuda")
    dsx = torch.full((N, KB, 4), 7.0, device="cuda")
    wb = H.WriteBwd(_p(d_recon), _p(vrec), _p(att), _p(dgen), _p(dsx), KB, N, Cc, w, literal, None, None, None, None)
    H.check(H.lib().air_write_bwd(C.byref(wb), _stream()), "air_write_bwd")
    torch.cuda.synchronize()
    dgen, dsx = _np(dgen), _np(dsx)
    n_active = 0
    for t in range(N):
        k = "kern/t%d/" % t
        act = gold[k + "mask"].astype(bool)
        n_active += int(act.sum())
        ref = (gold if literal == 2 else blk)[k + "d_gen_pre"].reshape(KB, -1)
        # inactive items: Select(active, ., 0) passes no gradient
        assert not dgen[t][~act].any() and not dsx[t][~act].any()
        assert not ref[~act].any()
        # active items: the UnsortedSegmentSum accumulation order, bit for bit (residue included)
        assert np.array_equal(dgen[t][act], ref[act]), (t, float(np.abs(dgen[t][act] - ref[act]).max()))
        assert np.abs(ref[act]).max() > 1.0          # the residue is there: the exact gradient is ~1e-2
        if literal == 4:
            seq = gold[k + "d_gen_pre"].reshape(KB, -1)[act]
            same = (dgen[t][act] == seq).mean(0)                                     # per window pixel, over the active items
            interior = np.ones((w, w), bool)
            interior[0, :] = interior[-1, :] = interior[:, 0] = interior[:, -1] = False
            assert (same.reshape(w, w)[interior] == 1.0).all()                       # interior pixels: the reference's chain
        # theta_recon legs: reductions over 2500 pixels (order differs from numpy's matmul) -> 1e-5
        ds_ref = ((gold[k + "d_s_write_0"] + gold[k + "d_s_write_1"]) + gold[k + "d_s_write_2"]) + gold[k + "d_s_write_3"]
        for got, ref1, nm in ((dsx[t, :, 0], ds_ref, "ds"), (dsx[t, :, 1], gold[k + "d_x_write"], "dx"),
                              (dsx[t, :, 2], gold[k + "d_y_write"], "dy"), (dsx[t, :, 3], gold[k + "d_z_canvas"], "dz")):
            scale = np.abs(ref1[act]).max()
            assert np.abs(got[act] - ref1[act]).max() <= 2e-5 * scale, (t, nm, got[act], ref1[act])
    assert n_active >= KB


def test_attend_bwd_matches_graph_head_gradients(H, gold):
    N, Cc, w = int(gold["train0/steps_executed"]), HP["canvas_size"], HP["windows_size"]
    images, targets, params, noise = _inputs()
    Hs = Hh = Hz = 64
    HT = 2 * Hs + 2 * Hh + Hz
    att = _cuda(_att(H, gold, N))
    out7 = np.zeros((N, KB, H.OUT_STRIDE), np.float32)
    d_win = np.zeros((N, KB, w * w), np.float32)
    d_sxyw = np.zeros((N, KB, 4), np.float32)
    for t in range(N):
        k = "kern/t%d/" % t
        out7[t, :, 0], out7[t, :, 1] = gold[k + "out_scale_mean"][:, 0], gold[k + "out_scale_lv"][:, 0]
        out7[t, :, 2:4], out7[t, :, 4:6] = gold[k + "out_shift_mean"], gold[k + "out_shift_lv"]
        out7[t, :, 6] = gold[k + "out_z_log_odds"][:, 0]
        d_win[t] = gold[k + "d_window"].reshape(KB, -1)
        ds = ((gold[k + "d_s_write_0"] + gold[k + "d_s_write_1"]) + gold[k + "d_s_write_2"]) + gold[k + "d_s_write_3"]
        d_sxyw[t] = np.stack([ds, gold[k + "d_x_write"], gold[k + "d_y_write"], gold[k + "d_z_canvas"]], 1)
    dyn = np.zeros(H.DYN_COUNT, np.float32)
    dyn[H.DYN_PRIOR_LOG_ODDS] = gold["train0/z_pres_prior_log_odds"]
    dyn[H.DYN_TEMPERATURE], dyn[H.DYN_STOP_THRESHOLD] = HP["z_pres_temperature"], HP["stopping_threshold"]
    dyn[H.DYN_SCALE_PM], dyn[H.DYN_SCALE_PV] = HP["scale_prior_mean"], HP["scale_prior_variance"]
    dyn[H.DYN_SHIFT_PM], dyn[H.DYN_SHIFT_PV] = HP["shift_prior_mean"], HP["shift_prior_variance"]
    dyn[H.DYN_VAE_PM], dyn[H.DYN_VAE_PV] = HP["vae_prior_mean"], HP["vae_prior_variance"]
    dyn[H.DYN_GRAD_SCALE] = 1.0 / 64                     # the graph's batch: d mean / d item
    hid = torch.ones(N, KB, HT, device="cuda")
    wout = torch.zeros(7, 64, device="cuda")
    d_hid = torch.zeros(N, KB, HT, device="cuda")
    d_out7 = torch.zeros(N, KB, H.OUT_STRIDE, device="cuda")
    # (device tensors are kept in named variables: the ABI takes raw pointers)
    canvas, e_s, e_h = _cuda(images[:KB]), _cuda(noise["eps_scale"][:N, :KB]), _cuda(noise["eps_shift"][:N, :KB])
    dyn_d, out7_d, d_win_d, d_sxyw_d = _cuda(dyn), _cuda(out7), _cuda(d_win), _cuda(d_sxyw)
    ab = H.AttendBwd(_p(hid), _p(wout), _p(canvas), _p(e_s), _p(e_h), _p(dyn_d), _p(out7_d), _p(att),
                     _p(d_win_d), _p(d_sxyw_d), _p(d_hid), _p(d_out7), KB, N, Cc, w, Hs, Hh, Hz, 64, 2)
    H.check(H.lib().air_attend_bwd(C.byref(ab), _stream()), "air_attend_bwd")
    torch.cuda.synchronize()
    got = _np(d_out7)
    for t in range(N):
        k = "kern/t%d/" % t
        ref = np.concatenate([gold[k + "d_out_scale_mean"].reshape(KB, 1), gold[k + "d_out_scale_lv"].reshape(KB, 1),
                              gold[k + "d_out_shift_mean"].reshape(KB, 2), gold[k + "d_out_shift_lv"].reshape(KB, 2),
                              gold[k + "d_out_z_log_odds"].reshape(KB, 1)], axis=1)
        # totals wrt (s, x, y) first: the read's theta gradient + the write legs (AddN_23..25)
        for o in range(7):
            scale = max(np.abs(ref[:, o]).max(), 1e-6)
            assert np.abs(got[t, :, o] - ref[:, o]).max() <= 1e-4 * scale, (t, o, got[t, :, o], ref[:, o])


def test_compose_reproduces_the_graphs_canvas_bit_for_bit(H, gold, golden_dir):
    """air_write_fwd (compose) teacher-forced on the graph's OWN per-step tensors (s, x, y, z_pres, masks, vae_recon,
    posterior mean / log-variance, the three per-step KLs) for the first KB images of the train0 run:
      * `reconstruction` (write transformer st_backward, x z_pres, masked accumulation over the steps, clip;
        air_model.py:351-366, 429-439, 580-582; transformer.py:56-117) BIT FOR BIT against the graph's clipped_rec --
        out-of-range tap residues included;
      * `reconstruction_loss` (:586-593) <= 1e-5 relative ("BCE evaluated on the same reconstruction");
        the order of the 2500-term sum is the only freedom;
      * the VAE KL (:479-485) and the running loss / ELBO per item <= 1e-5 relative, digit counts exact;
      * d loss / d reconstruction against the graph's gradient at the canvas (what air_write_bwd is then fed)."""
    comp = np.load(os.path.join(golden_dir, "graph_b64_compose.npz"))
    N, Cc, w, Z = int(gold["train0/steps_executed"]), HP["canvas_size"], HP["windows_size"], HP["vae_latent_dimensions"]
    assert N == HP["max_steps"]
    images, _, _, _ = _inputs()
    att = _att(H, gold, N)
    for t in range(N):
        att[t, :, H.ATT_KL_Z] = gold["train0/z_pres_kls"][:KB, t]
        att[t, :, H.ATT_KL_SCALE] = gold["train0/scale_kls"][:KB, t]
        att[t, :, H.ATT_KL_SHIFT] = gold["train0/shift_kls"][:KB, t]
        att[t, :, H.ATT_KL_VAE] = 7.0                                  # written by the kernel
    ml = np.stack([np.concatenate([comp["kern/t%d/rec_mean" % t], comp["kern/t%d/rec_log_variance" % t]], 1) for t in range(N)])
    vrec = np.stack([gold["kern/t%d/vae_recon" % t] for t in range(N)])
    dyn = np.zeros(H.DYN_COUNT, np.float32)
    dyn[H.DYN_VAE_PM], dyn[H.DYN_VAE_PV] = HP["vae_prior_mean"], HP["vae_prior_variance"]
    dyn[H.DYN_VAE_PLV] = np.log(np.float32(HP["vae_prior_variance"]))
    dyn[H.DYN_GRAD_SCALE] = 1.0 / 64                                   # the graph's batch: d mean / d item
    att_d, ml_d, vrec_d, img_d, dyn_d = _cuda(att), _cuda(ml), _cuda(vrec), _cuda(images[:KB]), _cuda(dyn)
    recon = torch.full((KB, Cc * Cc), 7.0, device="cuda")
    d_recon = torch.full((KB, Cc * Cc), 7.0, device="cuda")
    rec_loss, run_loss, loss_item = (torch.full((KB,), 7.0, device="cuda") for _ in range(3))
    digits = torch.full((KB,), 7, dtype=torch.int32, device="cuda")
    wf = H.WriteFwd(_p(vrec_d), _p(ml_d), _p(img_d), _p(dyn_d), _p(att_d), _p(recon), _p(rec_loss), _p(d_recon),
                    _p(run_loss), _p(digits), _p(loss_item), KB, N, Cc, w, Z)
    H.check(H.lib().air_write_fwd(C.byref(wf), _stream()), "air_write_fwd")
    torch.cuda.synchronize()
    ref_rec = gold["train0/reconstruction"][:KB]
    assert np.array_equal(_np(recon), ref_rec), float(np.abs(_np(recon) - ref_rec).max())
    # the canvases are not trivial: ink was written, and residues of out-of-range taps survive the clip
    assert ref_rec.max() > 0.3 and ((ref_rec > 0) & (ref_rec < 1e-5)).sum() > 100
    rl, rl_ref = _np(rec_loss).astype(np.float64), gold["train0/reconstruction_loss"][:KB].astype(np.float64)
    assert np.abs(rl - rl_ref).max() / np.abs(rl_ref).max() <= 1e-5 and np.all(np.abs(rl - rl_ref) <= 1e-5 * np.abs(rl_ref))
    kv = _np(att_d)[:, :, H.ATT_KL_VAE].T
    np.testing.assert_allclose(kv, gold["train0/vae_kls"][:KB], rtol=1e-5)
    np.testing.assert_allclose(_np(run_loss), comp["train0/running_loss"], rtol=1e-5)
    np.testing.assert_allclose(_np(loss_item), comp["train0/loss_per_item"], rtol=1e-5)
    assert np.array_equal(_np(digits), gold["train0/rec_num_digits"][:KB])
    # the ELBO of these 16 items given the graph's own per-step tensors
    assert abs(_np(loss_item).astype(np.float64).mean() - comp["train0/loss_per_item"].astype(np.float64).mean()) \
        <= 1e-5 * abs(comp["train0/loss_per_item"].astype(np.float64).mean())
    # d loss / d reconstruction: the graph's gradient at the canvas, for items that were active at some step
    g_sel = np.zeros((KB, Cc * Cc), np.float32)
    ever = np.zeros(KB, bool)
    for t in range(N):
        act = gold["kern/t%d/mask" % t].astype(bool)
        g_sel[act] = gold["kern/t%d/g_select" % t].reshape(KB, -1)[act]
        ever |= act
    got = _np(d_recon)[ever]
    # (x / p1 - (1 - x) / p0 here, grad * reciprocal(p) in TensorFlow's LogGrad: last-ulp differences of the two quotients)
    assert np.abs(got - g_sel[ever]).max() <= 2e-6 * np.abs(g_sel[ever]).max()


# ------------------------------------------------------------------ the rest of the backward, kernel by kernel, on the graph's tensors

def _gemm(H, A, B, Cc, M, N, K, lda, ldb, ldc, **kw):
    g = H.Gemm()
    g.A, g.B, g.C = A.data_ptr(), B.data_ptr(), Cc.data_ptr()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = M, N, K, lda, ldb, ldc
    g.precision = 0                                   # exact-fp32 products: the reference's precision
    for k, v in kw.items():
        setattr(g, k, v.data_ptr() if torch.is_tensor(v) else v)
    H.check(H.lib().air_gemm(C.byref(g), _stream()), "air_gemm")


ULP = 2.0 ** -23


def _ulps(got, ref):
    """max |got - ref| in units of one fp32 ulp of the tensor's scale max|ref|"""
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / (np.abs(ref).max() * ULP))


def test_backward_chain_kernel_by_kernel_on_the_graphs_own_tensors(H, gold, golden_dir):
    """Every remaining launch of the default backward, TEACHER-FORCED: its inputs are the executed graph's own tensors at that
    interface (tests/golden/graph_b64_chain.npz, make_graph_golden.py --chain-only; first 8 images of the train0 run, all
    three steps), its outputs are compared with the graph's next tensors.  With write_bwd / attend_bwd / compose pinned
    bit for bit above, the whole backward of the fp32 path is pinned to the graph launch by launch:
      dgrad_gen x2   (d_gen_pre -> generative_2 -> generative_1: MatMul_grad/MatMul + SoftplusGrad; vae.py:32-35)
      bottleneck_bwd (exact-fp32 form: generative_1 -> d z -> (d mean, d log_var) incl. the KL -> recognition_2; vae.py:16-30)
      dgrad_rec, dgrad_win (recognition_2 -> recognition_1 -> d glimpse; vae.py:10-14)
      dh_heads + the LSTM backward epilogues (last step, then BPTT: the five hidden layers' ReluGrad -> d h' -> d gates,
      d c; BasicLSTMCell, air_model.py:286)
    Measured in ulps of each tensor's scale (max |ref|): the GEMMs sum K = 256..784 products in another order than the
    executor's BLAS, the pointwise parts use expf where the graph has its own kernels; bound asserted: 16 ulp."""
    ch = np.load(os.path.join(golden_dir, "graph_b64_chain.npz"))
    comp = np.load(os.path.join(golden_dir, "graph_b64_compose.npz"))
    N, Z, R = int(gold["train0/steps_executed"]), HP["vae_latent_dimensions"], HP["rnn_units"]
    D = HP["canvas_size"] ** 2
    K8 = ch["kern/t0/d_gen2"].shape[0]
    M = N * K8
    _, _, params, noise = _inputs()
    P = {k: _cuda(v) for k, v in params.items()}
    st = lambda key, src=ch: np.concatenate([src["kern/t%d/%s" % (t, key)][:K8].reshape(K8, -1) for t in range(N)])   # noqa: E731
    rep = {}
    # ---- decoder data gradients
    d_genpre, act2, act1 = _cuda(st("d_gen_pre", gold)), _cuda(st("gen_act2")), _cuda(st("gen_act1"))
    d_gen2 = torch.full((M, 512), 7.0, device="cuda")
    _gemm(H, d_genpre, P["vae/gen_mean/weights"], d_gen2, M, 512, 784, 784, 784, 512, transB=1, aux=act2, ldaux=512,
          actgrad=H.GRAD_SOFTPLUS)
    rep["dgrad_gen2"] = _ulps(_np(d_gen2), st("d_gen2"))
    d_gen2_ref = _cuda(st("d_gen2"))
    d_gen1 = torch.full((M, 256), 7.0, device="cuda")
    _gemm(H, d_gen2_ref, P["vae/generative_2/weights"], d_gen1, M, 256, 512, 512, 512, 256, transB=1, aux=act1, ldaux=256,
          actgrad=H.GRAD_SOFTPLUS)
    rep["dgrad_gen1"] = _ulps(_np(d_gen1), st("d_gen1"))
    # ---- the bottleneck in one exact-fp32 launch
    att = np.zeros((M, H.ATT_STRIDE), np.float32)
    att[:, H.ATT_MASK] = np.concatenate([gold["kern/t%d/mask" % t][:K8] for t in range(N)]).astype(np.float32)
    dyn = np.zeros(H.DYN_COUNT, np.float32)
    dyn[H.DYN_VAE_PM], dyn[H.DYN_VAE_PV], dyn[H.DYN_GRAD_SCALE] = HP["vae_prior_mean"], HP["vae_prior_variance"], 1.0 / 64
    ml = np.concatenate([st("rec_mean", comp), st("rec_log_variance", comp)], 1)
    Wml = torch.cat([P["vae/rec_mean/weights"], P["vae/rec_log_variance/weights"]], 1).contiguous()
    dG, ml_d, eps_d = _cuda(st("d_gen1")), _cuda(ml), _cuda(noise["eps_z"][:N, :K8].reshape(M, Z))
    att_d, dyn_d, x_d = _cuda(att), _cuda(dyn), _cuda(st("rec_act2"))
    d_ml = torch.full((M, 2 * Z), 7.0, device="cuda")
    d_rec2 = torch.full((M, 256), 7.0, device="cuda")
    bb = H.BottleneckBwd(_p(dG), _p(P["vae/generative_1/weights"]), _p(ml_d), _p(eps_d), _p(att_d), _p(dyn_d), _p(Wml), _p(x_d),
                         _p(d_ml), _p(d_rec2), M, 256, Z, 256, None, None, None, None, None, 1)
    H.check(H.lib().air_vae_bottleneck_bwd(C.byref(bb), _stream()), "air_vae_bottleneck_bwd")
    rep["bottleneck_bwd d(mean|log_var)"] = _ulps(_np(d_ml), np.concatenate([st("d_mean"), st("d_log_variance")], 1))
    # (d_rec2 continues from the kernel's OWN d_ml inside the launch: one more K = 100 product on top of its rounding)
    rep["bottleneck_bwd d_rec2"] = _ulps(_np(d_rec2), st("d_rec2"))
    # ---- encoder data gradients
    d_rec2_ref, rec1 = _cuda(st("d_rec2")), _cuda(st("rec_act1"))
    d_rec1 = torch.full((M, 512), 7.0, device="cuda")
    _gemm(H, d_rec2_ref, P["vae/recognition_2/weights"], d_rec1, M, 512, 256, 256, 256, 512, transB=1, aux=rec1, ldaux=512,
          actgrad=H.GRAD_SOFTPLUS)
    rep["dgrad_rec1"] = _ulps(_np(d_rec1), st("d_rec1"))
    d_rec1_ref = _cuda(st("d_rec1"))
    d_win = torch.full((M, 784), 7.0, device="cuda")
    _gemm(H, d_rec1_ref, P["vae/recognition_1/weights"], d_win, M, 784, 512, 512, 512, 784, transB=1)
    rep["dgrad_win"] = _ulps(_np(d_win), st("d_window_vae"))
    # ---- heads' hidden layers -> d h' -> the LSTM cell backward, last step first
    HEADS = ("scale/mean", "scale/log_variance", "shift/mean", "shift/log_variance", "z_pres/log_odds")
    whid = torch.cat([P[h + "/hidden/weights"] for h in HEADS], 1).contiguous()               # [R, HT]
    HT = whid.shape[1]
    Wh = P["rnn/kernel"][D:].contiguous()                                                       # [R, 4R]
    dc_next = None
    dgates_next = None
    for t in reversed(range(N)):
        k = "kern/t%d/" % t
        d_hid = _cuda(np.concatenate([ch[k + "d_hid/" + h] for h in HEADS], 1))                # [K8, HT]
        acts = _cuda(np.concatenate([ch[k + "lstm_i"], ch[k + "lstm_j"], ch[k + "lstm_f"], ch[k + "lstm_o"]], 1))
        c_prev, c_new = _cuda(ch[k + "c_prev"]), _cuda(ch[k + "c_new"])
        dgates = torch.full((K8, 4 * R), 7.0, device="cuda")
        dc_prev = torch.full((K8, R), 7.0, device="cuda")
        dgsum = torch.zeros(K8, 4 * R, device="cuda")
        dh = torch.full((K8, R), 7.0, device="cuda")
        if t == N - 1:
            # the GEMM that produces d h' of the heads also starts the chain: rows >= i0 take the LSTM backward of the last step
            assert not ch[k + "dh_rec"].any()                                                   # nothing flows back into the last h'
            _gemm(H, d_hid, whid, dh, K8, R, HT, HT, HT, R, transB=1, epi=H.EPI_LSTM_BWD_TAIL, i0=0,
                  p0=acts, p1=c_prev, p2=c_new, q0=dgates, q1=dc_prev, q2=dgsum)
        else:
            dh_heads = torch.full((K8, R), 7.0, device="cuda")
            _gemm(H, d_hid, whid, dh_heads, K8, R, HT, HT, HT, R, transB=1)
            _gemm(H, dgates_next, Wh, dh, K8, R, 4 * R, 4 * R, 4 * R, R, transB=1, addend=dh_heads, ldadd=R,
                  epi=H.EPI_LSTM_BWD, p0=acts, p1=c_prev, p2=c_new, p3=dc_next, q0=dgates, q1=dc_prev, q2=dgsum, i0=1)
        torch.cuda.synchronize()
        rep["lstm_bwd t=%d dgates" % t] = _ulps(_np(dgates), ch[k + "dgates"])
        rep["lstm_bwd t=%d dc_prev" % t] = _ulps(_np(dc_prev), ch[k + "dc_prev"])
        dgates_next, dc_next = _cuda(ch[k + "dgates"]), _cuda(ch[k + "dc_prev"])               # teacher forcing
    torch.cuda.synchronize()
    print("backward chain vs the executed graph, ulps of the tensor scale:", {k: round(v, 2) for k, v in rep.items()})
    for k, v in rep.items():
        assert v <= 16.0, (k, v)
