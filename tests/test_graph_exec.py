"""Pins the CPU oracle to the reference's OWN executed graph.

oracle/graphdef_exec.py evaluates the reference's model/air-model.meta (the MetaGraphDef TF 1.3
saved for the reference's training run) node by node in numpy: forward while-loop, loss, the whole
tf.gradients backward (gradient while-loop, Stack push/pop, AddN orders, UnsortedSegmentSum),
clip_by_global_norm and ApplyAdam.  The graph is not committed; what it returns is, as fixtures
(tests/golden/make_graph_golden.py, make_graph_runs.py).  Asserted here:

  * fp32: every output the reference's callers fetch is BIT-IDENTICAL between the executed graph
    and oracle/air_oracle.py (train model at B=64, test model at dynamic B, with annealing and the
    early loop exit) -- the restatement is the graph's dataflow, op for op;
  * fp64 (the graph's exact math): all 36 gradients, the global norm and the clipped ApplyAdam
    update equal the oracle's autograd twin / adam_step to <= 2e-4 (the graph's constants are
    fp32-rounded, the oracle's fp64 ones are not), on every gradient's norm and a fixed element subset;
  * the oracle reproduces the committed fixtures tests/golden/graph_b64*.npz.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle import air_oracle_torch as at
from oracle import graphdef_exec as gx

HP = dict(ao.TRAINING_HP)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "graph_b64.npz")
GOLD_KERN = os.path.join(os.path.dirname(__file__), "golden", "graph_b64_kern.npz")   # its kern/* vectors (1 MiB per file)
RUNS = os.path.join(os.path.dirname(__file__), "golden", "graph_runs.npz")      # tests/golden/make_graph_runs.py
STRIDE = 4                                                  # make_graph_runs.STRIDE


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g.update(np.load(GOLD_KERN))
    return g


@pytest.fixture(scope="module")
def runs():
    return np.load(RUNS)


def _digest(a):
    a = np.asarray(a)
    return "%s|%s|%s" % (a.dtype.str, a.shape, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def _mk():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_graph_golden", os.path.join(os.path.dirname(GOLD), "make_graph_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ATTRS = ("reconstruction", "reconstruction_loss", "rec_num_digits", "rec_scales", "rec_shifts", "rec_st_back",
         "rec_windows", "z_pres_probs", "z_pres_kls", "scale_kls", "shift_kls", "vae_kls", "loss", "accuracy")


# ------------------------------------------------------------------ op kernels in isolation

def test_kernel_semantics():
    class N:
        def __init__(self, **kw): self.kw = kw
        def a(self, k, d=None): return self.kw.get(k, d)
    K = gx.OPS
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    # x[:, 1, ::2]  == begin_mask/end_mask on axis 0, shrink on axis 1
    n = N(begin_mask=0b101, end_mask=0b101, shrink_axis_mask=0b010)
    np.testing.assert_array_equal(K["StridedSlice"](n, x, [0, 1, 0], [0, 2, 0], [1, 1, 2]), x[:, 1, ::2])
    g = K["StridedSliceGrad"](n, [2, 3, 4], [0, 1, 0], [0, 2, 0], [1, 1, 2], np.ones((2, 2), np.float32))
    assert g.shape == (2, 3, 4) and g.sum() == 4 and g[:, 1, ::2].sum() == 4
    r0, r1 = K["BroadcastGradientArgs"](N(), [64, 1], [64, 2500])
    assert list(r0) == [1] and list(r1) == []
    r0, r1 = K["BroadcastGradientArgs"](N(), [], [64, 3])
    assert list(r0) == [0, 1] and list(r1) == []
    # scatter-add runs in index order, like the TF 1.3 CPU kernel (matters in fp32)
    d = np.array([1e8, 1.0, -1e8, 1.0], np.float32)
    assert K["UnsortedSegmentSum"](N(), d, np.zeros(4, np.int32), 1)[0] == np.float32(1.0)
    d = np.array([1.0, 1e8, 1.0, -1e8], np.float32)
    assert K["UnsortedSegmentSum"](N(), d, np.zeros(4, np.int32), 1)[0] == np.float32(0.0)
    ls = K["LinSpace"](N(), np.float32(-1), np.float32(1), 28)
    assert ls.dtype == np.float32 and ls[0] == -1 and abs(ls[-1] - 1) < 2e-7
    np.testing.assert_array_equal(ls, ao._linspace(28, np.float32))
    sp = K["Softplus"](N(), np.array([-20.0, 0.0, 20.0], np.float32))
    np.testing.assert_allclose(sp, [np.exp(-20.0), np.log(2.0), 20.0], rtol=1e-6)
    np.testing.assert_array_equal(sp, ao.softplus(np.array([-20.0, 0.0, 20.0], np.float32)))
    st = K["DynamicStitch"](N(N=2), np.array([0, 2]), np.array([1]), np.array([10., 30.]), np.array([20.]))
    np.testing.assert_array_equal(st, [10., 20., 30.])
    assert K["AddN"](N(), np.float32(1e8), np.float32(1.0), np.float32(-1e8)) == np.float32(0.0)     # left to right


# ------------------------------------------------------------------ forward: bit-exact

def _assert_bit_equal(rec, prefix, o):
    """the oracle's outputs against the graph's, recorded as dtype | shape | sha256 of the bytes"""
    for k in ATTRS:
        assert _digest(o[k]) == str(rec[prefix + k]), (k, str(rec[prefix + k]))


@pytest.mark.parametrize("step,seed_images,seed_noise", [(0, 3, 1), (3000, 11, 7), (40000, 5, 2)])
def test_train_graph_forward_is_bit_identical_to_oracle(runs, step, seed_images, seed_noise):
    mk = _mk()
    images, targets, params, noise = mk.inputs(seed_images=seed_images, seed_noise=seed_noise)
    if step == 40000:
        noise["u"][0] = 1e-4          # Concrete sample z_pres ~ 1e-4 in step 1: every stopping sum passes 0.99
    p = "train/%d/" % step
    lo = runs[p + "z_pres_prior_log_odds"]
    assert lo == ao.annealed_value(ao.TRAINING_ANNEALING["z_pres_prior_log_odds"], step)       # air_model.py:94-121
    o = ao.air_forward(params, images, targets, noise, HP, True, lo, early_exit=True)
    assert int(runs[p + "trips"]) == o["steps_executed"]                                        # cond :271-275
    if step == 40000:
        assert o["steps_executed"] == 1            # the while_loop exits early (cond :271-275)
    _assert_bit_equal(runs, p, o)


@pytest.mark.parametrize("batch,step", [(4, 40000), (7, 0), (1, 2000)])
def test_test_graph_dynamic_batch_is_bit_identical_to_oracle(runs, batch, step):
    mk = _mk()
    images, targets, params, noise = mk.inputs(batch=batch)
    p = "test/%d_%d/" % (batch, step)
    o = ao.air_forward(params, images, targets, noise, HP, False, runs[p + "z_pres_prior_log_odds"], early_exit=True)
    assert int(runs[p + "trips"]) == o["steps_executed"]
    _assert_bit_equal(runs, p, o)
    # the saved graph predates vae.py:43: its latents array holds the SAMPLE (vae.py:22-24); the oracle
    # follows the source (the mean).  Both are pinned: sample == mean + eps * sqrt(exp(log_var)).
    Tn = o["steps_executed"]
    lat = runs[p + "latent_samples"]
    assert lat.shape == o["rec_latents"].shape and not np.array_equal(lat, o["rec_latents"])
    for t in range(Tn):
        win = o["_window_in"][:, t]
        _, mean, lv, _ = ao.vae(win, params, HP, noise["eps_z"][t], noise["eps_x"][t])
        np.testing.assert_array_equal(mean, o["rec_latents"][:, t])
        np.testing.assert_array_equal(lat[:, t], mean + noise["eps_z"][t] * np.sqrt(np.exp(lv)))


# ------------------------------------------------------------------ backward + optimizer: fp64

@pytest.mark.parametrize("step", [0, 40000])
def test_graph_backward_and_adam_match_oracle_fp64(runs, step):
    """the graph in fp64: every gradient's norm and a fixed element subset of it, the global norm and the clipped
    ApplyAdam update of those elements (recorded by tests/golden/make_graph_runs.py)"""
    mk = _mk()
    images, targets, params, noise = mk.inputs()
    if step == 40000:
        noise["u"][0] = 1e-4          # early loop exit after one step: the gradient loop runs once, too
    f64 = np.float64
    p = "bwd/%d/" % step
    names = list(params.keys())
    gn = float(runs[p + "global_norm"])
    lo = float(runs[p + "z_pres_prior_log_odds"])
    assert int(runs[p + "bwd_trips"]) == int(runs[p + "fwd_trips"]) == (3 if step == 0 else 1)
    pt = at.to_torch(params, dtype=torch.float64, requires_grad=True)
    out, g = at.loss_and_grads(pt, torch.tensor(images, dtype=torch.float64), torch.tensor(targets),
                               at.to_torch(noise, dtype=torch.float64), HP, lo)
    assert abs(float(runs[p + "loss"]) - float(out["loss"])) / abs(float(out["loss"])) < 1e-6
    idx = {k: mk.subsample_index(k, params[k].size)[::STRIDE] for k in names}
    for k in names:
        ref = g[k].detach().numpy()
        nref = np.linalg.norm(ref)
        assert abs(float(runs[p + "grad_norm/" + k]) - nref) / max(nref, 1e-30) < 2e-4, k
        sub, rsub = runs[p + "grad_sub/" + k], ref.reshape(-1)[idx[k]]
        assert np.linalg.norm(sub - rsub) / max(np.linalg.norm(rsub), 1e-30) < 2e-4, k
    gn_ref = np.sqrt(sum(float((v.detach() ** 2).sum()) for v in g.values()))
    assert abs(gn - gn_ref) / gn_ref < 1e-4
    assert abs(np.sqrt(sum(float(runs[p + "grad_norm/" + k]) ** 2 for k in names)) - gn) / gn < 1e-12
    # clip_by_global_norm + ApplyAdam + beta powers at this global_step (air_model.py:654-694), on the recorded elements:
    # the clip is one scale for every element, from the graph's global norm
    g_sub = {k: runs[p + "grad_sub/" + k] for k in names}
    scale = f64(HP["gradient_clipping_norm"]) * np.minimum(f64(1.0) / f64(gn), f64(1.0) / f64(HP["gradient_clipping_norm"]))
    clipped = {k: v * scale for k, v in g_sub.items()}
    p64 = {k: np.asarray(params[k], f64).reshape(-1)[idx[k]] for k in names}
    m0 = {k: np.zeros_like(v) for k, v in p64.items()}
    v0 = {k: np.zeros_like(v) for k, v in p64.items()}
    # the graph's Adam constants are fp32 Const nodes: hand the oracle the same (rounded) values
    r32 = lambda x: float(np.float32(x))                                                     # noqa: E731
    new_p, new_m, new_v = ao.adam_step({k: v.copy() for k, v in p64.items()}, clipped, m0, v0, step + 1,
                                       r32(HP["learning_rate"]), r32(0.9), r32(0.999), r32(1e-8))[:3]
    # at step 0 the beta powers are beta itself; later the graph's accumulators are fp32 product chains
    tol = 1e-9 if step == 0 else 1e-3
    for k in names:
        d_graph, d_ref = runs[p + "var_sub/" + k] - p64[k], new_p[k] - p64[k]
        if np.linalg.norm(d_ref) > 0:
            assert np.linalg.norm(d_graph - d_ref) / np.linalg.norm(d_ref) < tol, k
        np.testing.assert_allclose(runs[p + "m_sub/" + k], new_m[k], rtol=1e-9, atol=1e-30)
        np.testing.assert_allclose(runs[p + "v_sub/" + k], new_v[k], rtol=1e-9, atol=1e-30)


# ------------------------------------------------------------------ the committed fixture

def test_oracle_matches_committed_graph_fixture(gold):
    """runs anywhere (no reference needed): oracle vs the vectors the reference graph produced"""
    mk = _mk()
    images, targets, params, noise = mk.inputs()
    o = ao.air_forward(params, images, targets, noise, HP, True, gold["train0/z_pres_prior_log_odds"], early_exit=True)
    assert o["steps_executed"] == int(gold["train0/steps_executed"])
    for k in mk.FWD_KEYS:
        if k != "z_pres_prior_log_odds":
            assert np.array_equal(np.asarray(o[k]), gold["train0/" + k]), k
    assert np.array_equal(o["rec_windows"][:mk.KB], gold["train0/rec_windows_first"])
    images2, targets2, _, noise2 = mk.inputs(seed_images=11, seed_noise=7)
    o2 = ao.air_forward(params, images2, targets2, noise2, HP, True, gold["train3000/z_pres_prior_log_odds"], early_exit=True)
    for k in ("loss", "accuracy", "reconstruction_loss", "rec_num_digits", "z_pres_kls", "vae_kls"):
        assert np.array_equal(np.asarray(o2[k]), gold["train3000/" + k]), k
    images4, targets4, _, noise4 = mk.inputs(batch=4)
    o4 = ao.air_forward(params, images4, targets4, noise4, HP, False, gold["test40000_b4/z_pres_prior_log_odds"], early_exit=True)
    for k in mk.FWD_KEYS + ("rec_windows",):
        if k != "z_pres_prior_log_odds":
            assert np.array_equal(np.asarray(o4[k]), gold["test40000_b4/" + k]), k
    # fp64 gradients of the graph vs the autograd twin, on the stored element subsets
    pt = at.to_torch(params, dtype=torch.float64, requires_grad=True)
    _, g = at.loss_and_grads(pt, torch.tensor(images, dtype=torch.float64), torch.tensor(targets),
                             at.to_torch(noise, dtype=torch.float64), HP, float(gold["train0/z_pres_prior_log_odds"]))
    for k in params:
        ref = g[k].detach().numpy().reshape(-1)[mk.subsample_index(k, g[k].numel())]
        sub = gold["train0/grad64_sub/" + k]
        assert np.linalg.norm(sub - ref) / max(np.linalg.norm(ref), 1e-30) < 2e-4, k


# ------------------------------------------------------------------ transformer backward (generic op)

def test_oracle_transformer_backward_matches_graph_fixture_and_autograd(gold):
    """oracle.transformer_backward (graph op order) vs (a) the executed graph's st_backward gradient
    tensors -- bit-identical d U, d theta to 1e-6 -- and (b) torch autograd in fp64, any theta."""
    f = np.float32
    for t in range(int(gold["train0/steps_executed"])):
        k = "kern/t%d/" % t
        s, x, y = gold[k + "s"], gold[k + "x"], gold[k + "y"]
        n = len(s)
        th = np.zeros((n, 2, 3), f)
        th[:, 0, 0] = f(1) / s; th[:, 0, 2] = (-x) / s; th[:, 1, 1] = f(1) / s; th[:, 1, 2] = (-y) / s   # air_model.py:353-356
        dU, dth = ao.transformer_backward(gold[k + "vae_recon"].reshape(n, 28, 28), th, (50, 50),
                                          gold[k + "g_window_recon"].reshape(n, 50, 50))
        act = gold[k + "mask"].astype(bool)
        assert np.array_equal(dU.reshape(n, -1)[act], gold[k + "d_vae_recon"].reshape(n, -1)[act])
        ref = gold[k + "d_theta_recon"].reshape(n, 6)[act]
        assert np.abs(dth.reshape(n, 6)[act] - ref).max() <= 1e-6 * np.abs(ref).max()
    rng = np.random.RandomState(0)
    B, Hi, Wi, Ho, Wo = 3, 9, 11, 7, 8
    U = rng.uniform(0, 1, (B, Hi, Wi))
    th = np.tile(np.array([[0.7, 0.2, 0.1], [-0.15, 0.8, -0.05]]), (B, 1, 1)) + rng.randn(B, 2, 3) * 0.1
    d = rng.randn(B, Ho, Wo)
    dU, dth = ao.transformer_backward(U, th, (Ho, Wo), d)
    Ut, tt = torch.tensor(U, requires_grad=True), torch.tensor(th, requires_grad=True)
    at.transformer(Ut, tt, (Ho, Wo)).backward(torch.tensor(d))
    np.testing.assert_allclose(dU, Ut.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(dth, tt.grad.numpy(), atol=1e-12)


# ------------------------------------------------------------------ chunks from +0.0 (the order the carried one is NOT)

def _chunks_from_zero(streams, chunks=16, chunk_min=64):
    """ONE slot's four tap streams cut as order="carried16" cuts them, every chunk summed sequentially from +0.0 and the
    chunk sums added left to right -- the plain chunked order round 5 shipped as backward="reference_blocked" and removed
    (it does not keep the size of the cancellation residue, and training noticed: DESIGN.md section 10.1).  Kept here as
    the contrast the carried order is measured against."""
    f = np.float32
    acc = f(0)
    for t in streams:
        n = len(t)
        if n == 0:
            continue
        cs = max(-(-n // chunks), chunk_min)
        for k0 in range(0, n, cs):
            acc = f(acc + np.add.accumulate(np.concatenate([[f(0)], t[k0:k0 + cs]]).astype(f))[-1])
    return acc


# ------------------------------------------------------------------ the carried accumulation order

def _carried_rule_by_hand(streams, chunks=16, chunk_min=64):
    """order="carried16" for ONE slot, term by term (the definition, not the library form)"""
    f = np.float32
    if all(len(t) <= chunk_min for t in streams):
        acc = f(0)
        for t in streams:
            for v in t:
                acc = f(acc + v)
        return acc
    chunks_ = []
    for t in streams:
        n = len(t)
        if n == 0:
            continue
        cs = max(-(-n // chunks), chunk_min)
        chunks_ += [t[k0:k0 + cs] for k0 in range(0, n, cs)]
    P, Ps, Qs = f(0), [], []
    for ch in chunks_:
        C, Q = f(0), P
        for v in ch:
            C = f(C + v)
            Q = f(Q + v)
        Ps.append(P); Qs.append(Q)
        P = f(P + C)
    Ps.append(P)
    corr = f(0)
    for k in range(len(chunks_) - 1):
        corr = f(corr + f(Qs[k] - Ps[k + 1]))
    return f(Qs[-1] + corr)


def test_carried_segment_sum_is_the_stated_rule():
    """oracle.carried_segment_sum (the order of backward="reference_carried") against the rule applied term by term: slots
    with four short streams are the sequential sum; one stream above 64 terms switches the whole slot to the carried
    chunks; empty streams; a slot that receives nothing."""
    rng = np.random.RandomState(8)
    lens = [[3, 2, 3, 2], [64, 64, 64, 64], [65, 1, 65, 1], [3000, 2900, 3000, 2900], [0, 0, 70, 5], [0, 0, 0, 0], [1025, 0, 1025, 7]]
    ids4, vals4, want = [], [], []
    streams = [[None] * 4 for _ in lens]
    for k in range(4):
        ids = np.concatenate([np.full(l[k], s) for s, l in enumerate(lens)]).astype(np.int64)
        perm = rng.permutation(len(ids))
        ids = ids[perm]
        vals = (rng.randn(len(ids)) * 10.0 ** rng.randint(-3, 8, len(ids))).astype(np.float32)
        if k >= 2:                                            # c = -a, d = -b where the lengths allow: the sampler's cancellation
            pass
        ids4.append(ids); vals4.append(vals)
        for s in range(len(lens)):
            streams[s][k] = vals[ids == s]
    got = ao.carried_segment_sum(ids4, vals4, len(lens))
    want = np.array([_carried_rule_by_hand(st) for st in streams], np.float32)
    assert np.array_equal(got, want)
    seq = np.zeros(len(lens), np.float32)
    np.add.at(seq, np.concatenate(ids4), np.concatenate(vals4))
    assert np.array_equal(got[:2], seq[:2]) and got[5] == 0                      # short slots: the reference's chain
    assert not np.array_equal(got[2:5], seq[2:5])                                # long ones: another tree


def test_carried_order_keeps_the_size_of_the_cancellation_residue():
    """What the order is FOR: corner-slot streams as the sampler makes them (c = -a, d = -b term by term, rare huge terms)
    leave a residue of the same RMS as the reference's one chain -- chunks summed from +0.0 leave a third of it (120 random streams)."""
    rng = np.random.RandomState(0)
    f = np.float32
    seq, car, blk = [], [], []
    for _ in range(120):
        n = rng.randint(300, 2500)
        wx, wy0, wy1 = (rng.uniform(0, 70, n).astype(f) for _ in range(3))
        g = np.where(rng.uniform(size=n) < 0.08, -1e7 * rng.uniform(0.1, 1, n), 1e-2 * rng.randn(n)).astype(f)
        st = [(wx * wy0) * g, (wx * wy1) * g, ((-wx) * wy0) * g, ((-wx) * wy1) * g]
        ids = [np.zeros(n, np.int64)] * 4
        s0 = np.zeros(1, f)
        np.add.at(s0, np.concatenate(ids), np.concatenate(st))
        seq.append(float(s0[0]))
        car.append(float(ao.carried_segment_sum(ids, st, 1)[0]))
        blk.append(float(_chunks_from_zero(st)))
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))     # noqa: E731
    assert 0.75 < rms(car) / rms(seq) < 1.33, (rms(car), rms(seq))
    assert rms(blk) / rms(seq) < 0.6, (rms(blk), rms(seq))


def test_carried_fixture_residue_norms_against_the_sequential_graph(gold, golden_dir):
    """tests/golden/graph_b64_carried.npz = the saved graph executed with its ONE UnsortedSegmentSum in the carried16 order.
    One realisation of the residue each, and one 8 000-term corner stream carries most of this one's norm: per variable
    within 0.05x..6x of the sequential order's (the device's own sequential realisation sits at 2.7x of the graph's,
    tests/test_gpu_graph_golden.py; what the order does to the residue's SIZE is measured over 700 streams below), far
    above the exact gradient; the z_pres heads (no sampler residue) unchanged."""
    car = np.load(os.path.join(golden_dir, "graph_b64_carried.npz"))
    r = float(car["train0/global_norm_fp32"]) / float(gold["train0/global_norm_fp32"])
    assert 0.1 < r < 4.0, r
    assert float(car["train0/global_norm_fp32"]) > 100 * float(gold["train0/global_norm_fp64"])
    for k in car.files:
        if not k.startswith("train0/grad32_norm/"):
            continue
        ratio = float(car[k]) / float(gold[k])
        assert 0.05 < ratio < 6.0, (k, ratio)
        if "/z_pres/" in k:
            assert abs(ratio - 1.0) < 1e-3, (k, ratio)


def test_carried_oracle_reproduces_the_carried_fixture(gold, golden_dir):
    """oracle.transformer_backward(order="carried16") on the graph's own sampler inputs gives the d_gen_pre rows of
    graph_b64_carried.npz (the graph executed with SEGMENT_SUM_ORDER = "carried16") bit for bit"""
    car = np.load(os.path.join(golden_dir, "graph_b64_carried.npz"))
    f = np.float32
    trips = int(gold["train0/steps_executed"])
    for t in range(trips):
        k = "kern/t%d/" % t
        s, x, y = gold[k + "s"], gold[k + "x"], gold[k + "y"]
        n = len(s)
        th = np.zeros((n, 2, 3), f)
        th[:, 0, 0] = f(1) / s; th[:, 0, 2] = (-x) / s; th[:, 1, 1] = f(1) / s; th[:, 1, 2] = (-y) / s
        v = gold[k + "vae_recon"].reshape(n, -1)
        dU, _ = ao.transformer_backward(v.reshape(n, 28, 28), th, (50, 50), gold[k + "g_window_recon"].reshape(n, 50, 50),
                                        order="carried16")
        act = gold[k + "mask"].astype(bool)
        got = ((dU.reshape(n, -1) * v) * (f(1) - v)).astype(f)
        assert np.array_equal(got[act], car[k + "d_gen_pre"][act])


def test_carried_order_keeps_the_residue_of_real_corner_streams():
    """The corner streams of the write backward as the model makes them at initialisation (two batches of 64 blob canvases
    through the oracle forward; d loss / d canvas with the poles of the Bernoulli ELBO): the error of each order against the
    exact (fp64) sum.  carried16 leaves the sequential order's mean |error| (measured 1.0x over 2116 streams; asserted
    0.6x..1.6x over ~700), chunks summed from +0.0 do not keep the distribution (twice the mean, a 5x heavier tail)."""
    from oracle.synth import blob_canvases
    f = np.float32
    hp = dict(ao.TRAINING_HP)
    err = {"seq": [], "car": [], "blk": []}
    for seed in range(2):
        B = 64
        images, targets = blob_canvases(B, 50, 2, seed=100 + seed)
        o = ao.air_forward(ao.init_params(hp, seed), images, targets, ao.make_noise(hp, B, seed + 50), hp, True, 9.21)
        r = o["_running_recon"]
        rc = np.clip(r, 0, 1).astype(f)
        p1, p0 = rc + f(ao.EPS), (f(1) - rc) + f(ao.EPS)
        g = np.where((r <= 1) & (np.minimum(r, 1) >= 0), -(f(1) / f(B)) * (images / p1 - (f(1) - images) / p0), 0).astype(f)
        for t in range(o["rec_scales"].shape[1]):
            s, xs, ys = o["rec_scales"][:, t, 0], o["rec_shifts"][:, t, 0], o["rec_shifts"][:, t, 1]
            th = np.zeros((B, 2, 3), f)
            th[:, 0, 0] = th[:, 1, 1] = f(1) / s
            th[:, 0, 2], th[:, 1, 2] = (-xs) / s, (-ys) / s
            _, aux = ao.transformer(o["rec_windows"][:, t].reshape(B, 28, 28).astype(f), th, (50, 50), return_aux=True)
            X, Y, x0, x1, y0, y1 = (aux[q] for q in ("x", "y", "x0", "x1", "y0", "y1"))
            gg = (o["_z_pres"][:, t][:, None] * g).astype(f)
            wx0, wx1, wy0, wy1 = x1.astype(f) - X, X - x0.astype(f), y1.astype(f) - Y, Y - y0.astype(f)
            for b in range(B):
                idx = [y0[b] * 28 + x0[b], y1[b] * 28 + x0[b], y0[b] * 28 + x1[b], y1[b] * 28 + x1[b]]
                val = [(wx0[b] * wy0[b]) * gg[b], (wx0[b] * wy1[b]) * gg[b], (wx1[b] * wy0[b]) * gg[b], (wx1[b] * wy1[b]) * gg[b]]
                for sl in (0, 27, 756, 783):
                    st = [v[i == sl] for i, v in zip(idx, val)]
                    if max(len(q) for q in st) <= 64:
                        continue
                    ids = [np.zeros(len(q), np.int64) for q in st]
                    exact = float(np.concatenate(st).astype(np.float64).sum())
                    seq = np.zeros(1, f)
                    np.add.at(seq, np.concatenate(ids), np.concatenate(st))
                    err["seq"].append(float(seq[0]) - exact)
                    err["car"].append(float(ao.carried_segment_sum(ids, st, 1)[0]) - exact)
                    err["blk"].append(float(_chunks_from_zero(st)) - exact)
    mean = {k: float(np.mean(np.abs(v))) for k, v in err.items()}
    assert len(err["seq"]) > 500
    assert 0.6 < mean["car"] / mean["seq"] < 1.6, mean
