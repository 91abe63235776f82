"""GPU tests of the importance-weighted bound (air_importance_logw / air_importance_fold of include/air_hip.h,
AIRModel.forward_sampled, air.metrics.ImportanceBound).

The reference is the float64 restatement of tests/importance_cases.py.  air_importance_logw has no transcendental: logw,
digits and terms are compared BIT FOR BIT.  air_importance_fold: the integer counts, map, and the confusion matrix are exact;
the fp64 values go through the device's exp and log, held to 3 ulp, in sums of at most K + T terms, so they may differ from
the restatement by importance_cases.fold_bound(K, T) = 8 (K + T + 2) 2^-52 relative to max(1, |ref|) -- the largest gap seen
is printed (DESIGN.md section 47 records it).  Inputs and outputs sit between guard bands (NaN around the fp32 inputs,
sentinels around everything else) that must be intact afterwards; rows >= k of every input are NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import importance_cases as ic

pytestmark = pytest.mark.gpu

GUARD = 8                                    # sentinel elements in front of and behind every buffer
FILL_I32, FILL_I64, FILL_F64 = -5, -(2 ** 40) - 5, -7.25
F32_INPUTS = ("att", "out7", "ml", "z", "eps_scale", "eps_shift", "eps_z", "rec_loss", "dyn")
WORST = {"gap": 0.0, "where": None}


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """a device buffer of n elements between two rows of sentinels; `init` fills the payload"""

    def __init__(self, n, dtype, fill, init=None):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        if init is not None:
            self.buf[GUARD:GUARD + n] = init
        self.view = self.buf[GUARD:GUARD + n]

    def payload(self):
        """the payload as numpy, after checking the sentinels"""
        host = self.buf.cpu().numpy()
        for band in (host[:GUARD], host[GUARD + self.n:]):
            assert np.isnan(band).all() if self.fill != self.fill else (band == self.fill).all(), "a sentinel was overwritten"
        return host[GUARD:GUARD + self.n]


def _note(where, gap):
    if gap > WORST["gap"]:
        WORST["gap"], WORST["where"] = gap, where


# ------------------------------------------------------------------------------------------------------------- log-weights
def run_logw(H, inp, sample, with_terms=True):
    """one air_importance_logw call -> the three tables as numpy, [K, B(, 5)]; every table starts as sentinels"""
    B, k, T, Z, ldz, K = inp["shape"]
    ins = {key: Guarded(inp[key].size, torch.float32, float("nan"), init=_dev(inp[key].reshape(-1))) for key in F32_INPUTS}
    rd = Guarded(B, torch.int32, FILL_I32, init=_dev(inp["run_digits"]))
    out = dict(logw=Guarded(K * B, torch.float64, FILL_F64), digits=Guarded(K * B, torch.int32, FILL_I32),
               terms=Guarded(K * B * ic.TERMS, torch.float64, FILL_F64))
    p = lambda key: H.ptr(ins[key].view)                           # noqa: E731
    a = H.Importance(p("att"), p("out7"), p("ml"), p("z"), p("eps_scale"), p("eps_shift"), p("eps_z"), p("rec_loss"),
                     H.ptr(rd.view), p("dyn"), H.ptr(out["logw"].view), H.ptr(out["digits"].view),
                     H.ptr(out["terms"].view) if with_terms else None, T, B, k, Z, ldz, K)
    H.launch("air_importance_logw", torch.device("cuda"), C.byref(a), sample)
    torch.cuda.synchronize()
    for key in F32_INPUTS:
        assert ic.bits(ins[key].payload()) == ic.bits(inp[key].reshape(-1)), key
    assert (rd.payload() == inp["run_digits"]).all()
    return out["logw"].payload().reshape(K, B), out["digits"].payload().reshape(K, B), out["terms"].payload().reshape(K, B, ic.TERMS)


def check_logw(H, inp, sample, with_terms=True):
    B, k, T, Z, ldz, K = inp["shape"]
    want_w, want_d, want_t = ic.logw_reference(inp)
    logw, digits, terms = run_logw(H, inp, sample, with_terms)
    assert ic.bits(logw[sample, :k]) == ic.bits(want_w), np.flatnonzero(logw[sample, :k] != want_w)[:8]
    assert (digits[sample, :k] == want_d).all()
    if with_terms:
        assert ic.bits(terms[sample, :k]) == ic.bits(want_t)
        terms[sample, :k] = FILL_F64
    logw[sample, :k], digits[sample, :k] = FILL_F64, FILL_I32      # only that row, only columns < k, were written
    assert (logw == FILL_F64).all() and (digits == FILL_I32).all() and (terms == FILL_F64).all()


@pytest.mark.parametrize("shape", ic.LOGW_SHAPES, ids=ic.shape_name)
def test_logw_equals_the_restatement_bit_for_bit(H, shape):
    """(B, k, T, Z, ldz, K): 3 and 65 images, k < B, T = 1, 2, 16, Z = 1, 3, 50 in rows of 52, 256; image 0 stopped at step
    0, image 1 with every step active, NaN in every closed step and in rows >= k; the first and the last row of the tables"""
    inp = ic.logw_inputs(shape)
    for sample in sorted({0, shape[5] - 1}):
        check_logw(H, inp, sample)


def test_logw_without_the_terms_table_and_with_an_infinite_rec_loss(H):
    check_logw(H, ic.logw_inputs((65, 60, 2, 3, 3, 2)), 1, with_terms=False)
    for s, inp in enumerate(ic.degenerate_passes()):
        check_logw(H, inp, s)


# -------------------------------------------------------------------------------------------------------------------- fold
def run_fold(H, case, per_image=True, counts_in=None, sums_in=None, first=0, k=None):
    """one air_importance_fold call over the images [first, first + k) of `case` -> counts, sums, bound, ess, map as numpy"""
    T, B, K = case["T"], case["B"], case["K"]
    k = case["k"] - first if k is None else k
    ncounts = ic.COUNTS + (T + 1) * (T + 1)
    logw = Guarded(K * B, torch.float64, FILL_F64, init=_dev(case["logw"].reshape(-1)))
    digits = Guarded(K * B, torch.int32, FILL_I32, init=_dev(case["digits"].reshape(-1)))
    tg = None if case["targets"] is None else Guarded(case["k"], torch.int32, FILL_I32, init=_dev(case["targets"]))
    counts = Guarded(ncounts, torch.int64, FILL_I64, init=_dev(np.zeros(ncounts, np.int64) if counts_in is None else counts_in))
    sums = Guarded(ic.SUMS, torch.float64, FILL_F64, init=_dev(np.zeros(ic.SUMS) if sums_in is None else sums_in))
    out = dict(bound=Guarded(k, torch.float64, FILL_F64), ess=Guarded(k, torch.float64, FILL_F64), map=Guarded(k, torch.int32, FILL_I32))
    nbytes = H.lib().air_importance_fold_workspace_bytes(T, B, k, K)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = Guarded(nbytes // 8, torch.float64, FILL_F64)
    opt = (lambda key: H.ptr(out[key].view)) if per_image else (lambda key: None)
    a = H.ImportanceFold(H.ptr(logw.view[first:]), H.ptr(digits.view[first:]), H.ptr(tg.view[first:]) if tg else None,
                         opt("bound"), opt("ess"), opt("map"), H.ptr(counts.view), H.ptr(sums.view), T, B, k, K)
    H.launch("air_importance_fold", torch.device("cuda"), C.byref(a), H.ptr(ws.view))
    torch.cuda.synchronize()
    ws.payload()
    assert ic.bits(logw.payload()) == ic.bits(case["logw"].reshape(-1)) and (digits.payload() == case["digits"].reshape(-1)).all()
    assert tg is None or (tg.payload() == case["targets"]).all()
    got = {key: g.payload() for key, g in out.items()}
    if not per_image:
        assert (got["bound"] == FILL_F64).all() and (got["ess"] == FILL_F64).all() and (got["map"] == FILL_I32).all()
    got.update(counts=counts.payload(), sums=sums.payload())
    return got


def assert_fold(name, got, want, K, T, per_image=True):
    assert (got["counts"] == want["counts"]).all(), (name, got["counts"], want["counts"])
    keys = ("sums", "bound", "ess") if per_image else ("sums",)
    for key in keys:
        gap, ok = ic.close(got[key], want[key], K, T)
        print("%s: %s gap %.3e of %.3e allowed" % (name, key, gap, ic.fold_bound(K, T)))
        _note("%s/%s" % (name, key), gap)
        assert ok, (name, key, gap, ic.fold_bound(K, T))
    if per_image:
        assert (got["map"] == want["map"]).all(), (name, got["map"], want["map"])


@pytest.mark.parametrize("name", sorted(ic.fold_cases()))
def test_fold_equals_the_restatement(H, name):
    """counts, MAP counts and the confusion matrix exactly, the fp64 values within the derived bound: one sample, two, 64;
    k < B; 290 images (two groups of the sums); counts beyond [0, T] clamped; no targets; weights 800 apart; an exact tie of
    the count posterior; a degenerate image beside sound ones"""
    case = ic.fold_cases()[name]
    got = run_fold(H, case)
    assert_fold(name, got, ic.expected_fold(name), case["K"], case["T"])
    for i in ic.DEGENERATE_IMAGES.get(name, ()):
        assert np.isnan(got["bound"][i]) and np.isnan(got["ess"][i]) and got["map"][i] == -1


def test_fold_adds_to_its_accumulators_and_needs_no_optional_output(H):
    case, once = ic.fold_cases()["b65_t2_s2"], ic.expected_fold("b65_t2_s2")
    want = ic.fold_reference(case, once["counts"], once["sums"])
    got = run_fold(H, case, per_image=False, counts_in=once["counts"], sums_in=once["sums"])
    assert_fold("b65_t2_s2 (second call)", got, want, case["K"], case["T"], per_image=False)


def test_the_same_tables_give_the_same_bits_and_one_sample_is_exact(H):
    case = ic.fold_cases()["b300_t3_s16"]
    a, b = run_fold(H, case), run_fold(H, case)
    assert all(ic.bits(a[key]) == ic.bits(b[key]) for key in a)
    one = run_fold(H, ic.fold_cases()["b3_t1_s1"])
    assert ic.bits(one["bound"]) == ic.bits(ic.fold_cases()["b3_t1_s1"]["logw"][0, :3]) and (one["ess"] == 1.0).all()


def test_two_folds_over_halves_equal_one_over_the_whole(H):
    """the per-image values and every count are the same; the sums associate their additions differently (the header says
    so: the tree of a group depends on k), so they agree within the derived bound, not bit for bit"""
    case = ic.fold_cases()["b65_t2_s2"]
    T, K, k = case["T"], case["K"], case["k"]
    whole = run_fold(H, case)
    h = k // 2
    first = run_fold(H, case, first=0, k=h)
    second = run_fold(H, case, first=h, k=k - h, counts_in=first["counts"], sums_in=first["sums"])
    assert (second["counts"] == whole["counts"]).all()
    for key in ("bound", "ess", "map"):
        assert ic.bits(np.concatenate((first[key], second[key]))) == ic.bits(whole[key]), key
    gap, ok = ic.close(second["sums"], whole["sums"], K, T)
    print("halves against the whole: sums gap %.3e of %.3e allowed" % (gap, ic.fold_bound(K, T)))
    assert ok, gap


# ------------------------------------------------------------------------------------------------------------------- model
B_MODEL, K_MODEL = 4, 3


@pytest.fixture(scope="module")
def model(H):
    """a small fp32 test model: the hyper-parameters of test_gpu_step_limits' model with three steps, four blob canvases"""
    from air import air_model as am
    from oracle import air_oracle as ao
    from oracle.synth import blob_canvases
    from test_gpu_step_limits import LIMIT_HP
    hp = dict(LIMIT_HP, max_steps=3)
    images, targets = blob_canvases(B_MODEL, hp["canvas_size"], hp["max_digits"], seed=11)
    am.reset_default_graph()
    m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=False,
                    scope="air", gemm_precision="fp32", **hp)
    m.load_state_dict(ao.init_params(hp, 3))
    return m, np.asarray(targets, np.int32)


def _pass_of(m):
    """the buffers air_importance_logw reads, copied to the host as importance_cases.logw_inputs lays them out"""
    T, B, Z = int(m.max_steps), int(m.batch_size), int(m.vae_latent_dimensions)
    np_ = lambda t: t.detach().cpu().numpy().copy()                  # noqa: E731
    return dict(att=np_(m.att), out7=np_(m.out7), ml=np_(m.ml), z=np_(m.zs), eps_scale=np_(m.eps_scale).reshape(T, B),
                eps_shift=np_(m.eps_shift), eps_z=np_(m.eps_z), rec_loss=np_(m._rec_loss), run_digits=np_(m.run_digits),
                dyn=np_(m.dyn), shape=(B, B, T, Z, Z, K_MODEL))


def _snapshot(m):
    m.forward()
    torch.cuda.synchronize()
    return tuple(ic.bits(t.detach().cpu().numpy()) for t in (m.att, m.run_digits, m.scalars))


def test_the_instrument_on_a_model_equals_the_restatement_of_its_own_buffers(H, model):
    from air.metrics import ImportanceBound
    m, targets = model
    T = int(m.max_steps)
    before = _snapshot(m)
    iw = ImportanceBound(m, samples=K_MODEL, seed=5, keep=True)
    iw.reset()
    passes = []
    for s in range(K_MODEL):
        iw.add_sample()
        torch.cuda.synchronize()
        passes.append(_pass_of(m))
    iw.fold(targets)
    logw, digits, terms = (t.cpu().numpy() for t in (iw.logw, iw.digits, iw.terms))
    for s, p in enumerate(passes):
        want_w, want_d, want_t = ic.logw_reference(p)
        assert ic.bits(logw[s]) == ic.bits(want_w) and (digits[s] == want_d).all() and ic.bits(terms[s]) == ic.bits(want_t), s
        assert ic.bits(terms[s, :, ic.TERM_REC]) == ic.bits(p["rec_loss"].astype(np.float64))
        zp = np.zeros(B_MODEL)
        for t in range(T):
            zp = zp + np.where(p["att"][t, :, ic.ATT_MASK_PREV] != 0, p["att"][t, :, ic.ATT_KL_Z].astype(np.float64), 0.0)
        assert ic.bits(terms[s, :, ic.TERM_Z_PRES]) == ic.bits(zp)
    assert np.isfinite(logw).all()
    assert len({ic.bits(logw[s]) for s in range(K_MODEL)}) == K_MODEL             # fresh noise: the three rows differ
    case = dict(logw=logw, digits=digits, targets=targets, T=T, B=B_MODEL, k=B_MODEL, K=K_MODEL)
    want = ic.fold_reference(case)
    got = dict(counts=iw.counts.cpu().numpy(), sums=iw.sums.cpu().numpy(), bound=iw.bound.cpu().numpy(), ess=iw.ess.cpu().numpy(),
               map=iw.map.cpu().numpy())
    assert_fold("model", got, want, K_MODEL, T)
    res = iw.result()
    vals = ic.values_of(want["counts"], want["sums"], K_MODEL)
    for name, v in zip(ic.NAMES, vals):
        assert abs(res[name] - v) <= ic.fold_bound(K_MODEL, T) * max(1.0, abs(v)), (name, res[name], v)
    assert res["gap"] >= 0.0 and res["scored"] == B_MODEL and res["confusion"].sum() == B_MODEL and iw.calls == K_MODEL
    # the same (seed, first call) reproduces every bit, through evaluate(); the next evaluation draws other noise
    again = ImportanceBound(m, samples=K_MODEL, seed=5, keep=True)
    again.evaluate(targets)
    for key in ("logw", "digits", "terms", "counts", "sums", "bound", "ess", "map"):
        assert ic.bits(getattr(again, key).cpu().numpy()) == ic.bits(getattr(iw, key).cpu().numpy()), key
    again.evaluate(targets)
    assert again.calls == 2 * K_MODEL and ic.bits(again.logw.cpu().numpy()) != ic.bits(logw)
    other = ImportanceBound(m, samples=K_MODEL, seed=6)
    other.evaluate()
    assert ic.bits(other.logw.cpu().numpy()) != ic.bits(logw) and np.isnan(other.result()["count_accuracy"])
    # forward() gives what it gave before
    assert _snapshot(m) == before


def test_a_captured_evaluation_graph_is_left_alone(H, model):
    from air.metrics import ImportanceBound
    m, targets = model
    m.capture_graph()
    try:
        before = _snapshot(m)
        iw = ImportanceBound(m, samples=K_MODEL, seed=5)
        iw.evaluate(targets)
        assert np.isfinite(iw.logw.cpu().numpy()).all()
        assert _snapshot(m) == before
    finally:
        m.release_graph()


def test_the_driver_loop_writes_the_iw_keys_beside_the_loss(H, model, tmp_path):
    """training.py's SummaryWriter with the instrument in its list: two evaluations, rows with every iw_* key, gap >= 0, the
    second on other noise; the values are those of an instrument of the same seed run by hand"""
    import json
    import time
    import training
    from air.metrics import ImportanceBound
    m, targets = model
    tg = torch.tensor(targets, device="cuda")
    iw, byhand = ImportanceBound(m, samples=K_MODEL, seed=9), ImportanceBound(m, samples=K_MODEL, seed=9)
    seen = []
    writer = training.SummaryWriter(m, str(tmp_path / "scalars.jsonl"), time.perf_counter(), instruments=[(iw, (tg,))],
                                    on_values=lambda step, instrument, values: seen.append((step, instrument, values)))
    want = []
    for step in (0, 50):
        m.forward()
        writer.push(step)
        byhand.evaluate(tg)
        want.append(byhand.values().cpu().tolist())
    writer.flush()
    writer.file.close()
    rows = [json.loads(line) for line in open(str(tmp_path / "scalars.jsonl"))]
    assert [r["step"] for r in rows] == [0, 50] and [s for s, _, _ in seen] == [0, 50] and all(i is iw for _, i, _ in seen)
    for row, values in zip(rows, want):
        assert "loss" in row and [k for k in row if k.startswith("iw_")] == ["iw_" + n for n in ic.NAMES]
        assert [row["iw_" + n] for n in ic.NAMES] == [round(v, 5) for v in values]
        assert row["iw_gap"] >= 0.0 and 1.0 / K_MODEL <= row["iw_ess_share"] <= 1.0
    assert rows[0]["iw_nll_bound"] != rows[1]["iw_nll_bound"]


def test_the_largest_fold_gap_seen_is_within_the_bound(H):
    print("largest fold gap against the restatement: %.3e (%s)" % (WORST["gap"], WORST["where"]))
    assert WORST["gap"] <= ic.fold_bound(64, 16)
