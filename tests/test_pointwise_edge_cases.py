"""CPU side of tests/test_gpu_pointwise_edges.py: that the case tables of tests/pointwise_edge_cases.py reach the edges they are
there for, that the inputs are sized for the bounds (the fp32 restatement of every kernel lies within a quarter of each bound
of the float64 reference, for every case -- a condition on the inputs that holds without any kernel), that the slab order of
the first LSTM step shows in the bits, and the host-side argument checks of the seven entry points (no launch: every call
here carries an argument that is refused)."""
import numpy as np
import pytest
import torch

import abi_check as abi
import pointwise_edge_cases as pec

RATIOS = {}


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(r))


def _report(prefix):
    print("fp32 restatement, largest error / bound:", {k: "%.3f" % v for k, v in sorted(RATIOS.items()) if k.startswith(prefix)})
    over = {k: v for k, v in RATIOS.items() if k.startswith(prefix) and not v <= pec.QUARTER}
    assert not over, over


# ---- the tables ---------------------------------------------------------------------------------------------------------
def test_tables_reach_the_edges():
    T = pec.THREADS
    for shapes in (pec.LSTM_FWD_SHAPES, pec.LSTM_BWD_SHAPES, pec.REPARAM_SHAPES):
        n = [a * b for a, b in shapes]
        assert 1 in n and any(v % T for v in n if v > T) and any(v % T == 0 for v in n) and any(v < T for v in n)
        assert any(b == 1 and a >= T for a, b in shapes) and any(b % 2 and b > 1 for a, b in shapes)      # R = 1 with many rows; odd R
    assert (1, 256) in pec.LSTM_FWD_SHAPES and (2, 256) in pec.LSTM_FWD_SHAPES                             # one full block, two
    # the first step: every slab count the entry point accepts, with and without bias and twin, at every shape
    assert len(pec.FIRST_STEP_CASES) == 3 * 8 * 2 * 2
    assert {(c["nslabs"], c["bias"], c["h16"]) for c in pec.FIRST_STEP_CASES if c["B"] == 64} == \
        {(n, b, h) for n in range(1, 9) for b in (True, False) for h in (True, False)}
    assert len(pec.LSTM_BWD_CASES) == 5 * 2 * 3 and len(pec.PLAIN_CASES) == 4 * 4
    # the grid-stride loops take a second round, and only just
    cap = pec.GRID_CAP * T
    M, Z = pec.PLAIN_SHAPES[-1]
    assert cap < M * Z <= cap + T
    n = pec.SIGMOID_N[-1]
    assert n // 4 > cap and n // 4 <= cap + T and n % 4 == 3 and n * 4 <= 8 * 2 ** 20 + 64              # 8 MB: the largest array
    assert {n % 4 for n in pec.SIGMOID_N} == {0, 1, 3} and 1027 in pec.SIGMOID_N
    assert all(sum(1 for o in c["off"] if o) <= 1 for c in pec.SIGMOID_CASES) and len(pec.SIGMOID_CASES) == 6 * 4
    # one workgroup per image, 256 threads striding over D
    D = [d for _, d in pec.BCE_SHAPES]
    assert 1 in D and 255 in D and 256 in D and 257 in D and 2500 in D
    fc = pec.finalize_cases()
    for B in pec.FINALIZE_B:
        ks = [c["k"] for c in fc if c["B"] == B]
        assert ks[:2] == [B, 0]
        assert all(B % k for k in ks[2:]) and (len(ks) == 3 or B <= 2)
    assert [B for B in pec.FINALIZE_B if B > 2] == [255, 256, 257, 1000]


def test_bf16_bits_is_round_to_nearest_even():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.randn(4096).astype(np.float32), np.array([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0], np.float32)])  # ties
    assert np.array_equal(pec.bf16_bits(x), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy())


def test_mask_rows_and_nan_records():
    for B, Z in pec.REPARAM_SHAPES:
        x = pec.reparam_inputs(B, Z)
        assert B == 1 or (x["mask"].min() == 0.0 and x["mask"].max() == 1.0)
        assert int(np.isfinite(x["att"]).sum()) == B and int(np.isfinite(x["dyn"]).sum()) == 3
        assert np.isfinite(pec.reparam_bwd_ref(x)).all()
        lv = x["ml"][:, Z:]
        assert lv.min() >= -6 and lv.max() <= 2 and np.abs(x["ml"][:, :Z]).max() <= 2 and np.abs(x["eps"]).max() <= 3
        # a row with mask 0: exactly d on the mean leg
        ref = pec.reparam_bwd_f32(x)
        assert np.array_equal(ref[x["mask"] == 0][:, :Z], x["d_zs"][x["mask"] == 0])
    assert int(np.isfinite(pec.bce_inputs(3, 257)["dyn"]).sum()) == 1


def test_slab_order_shows_in_the_bits():
    """with three or more slabs the sum from the last slab to the first has other bits than the promised order, at every shape
    (two fp32 additions commute, so a case of 1 or 2 slabs cannot tell)"""
    for c in pec.FIRST_STEP_CASES:
        x = pec.first_step_inputs(c)
        bias = x["bias"] if c["bias"] else None
        fwd = pec.first_step_pre(x["slabs"], bias)
        rev = pec.first_step_pre(x["slabs"], bias, order=range(c["nslabs"] - 1, -1, -1))
        assert np.abs(fwd).max() < 6.0
        if c["nslabs"] >= 3:
            differ = int((fwd.view(np.int32) != rev.view(np.int32)).sum())
            assert differ >= max(1, fwd.size // 20), (pec.describe(c), differ)
            _, _, h_f = pec.lstm_fwd_f32(fwd, np.zeros((c["B"], c["R"]), np.float32))
            _, _, h_r = pec.lstm_fwd_f32(rev, np.zeros((c["B"], c["R"]), np.float32))
            assert not np.array_equal(h_f, h_r), pec.describe(c)


# ---- the inputs are sized for the bounds --------------------------------------------------------------------------------
def test_lstm_restatement_within_a_quarter_of_the_bounds():
    zero = lambda B, R: np.zeros((B, R), np.float32)  # noqa: E731
    runs = [(x["pre"], x["c_prev"]) for x in (pec.lstm_fwd_inputs(B, R) for B, R in pec.LSTM_FWD_SHAPES)]
    for c in pec.FIRST_STEP_CASES:
        x = pec.first_step_inputs(c)
        runs.append((pec.first_step_pre(x["slabs"], x["bias"] if c["bias"] else None), zero(c["B"], c["R"])))
    for pre, c_prev in runs:
        for name, got, ref in zip(("acts", "c", "h"), pec.lstm_fwd_f32(pre, c_prev), pec.lstm_fwd_ref(pre, c_prev)):
            _note("lstm_fwd/" + name, pec.ratio(got, ref, pec.LSTM_FWD_TOL))
    for c in pec.LSTM_BWD_CASES:
        x = pec.lstm_bwd_inputs(c["B"], c["R"])
        for name, got, ref in zip(("dgates", "dc_prev"), pec.lstm_bwd_f32(x, c["dc_in"]), pec.lstm_bwd_ref(x, c["dc_in"])):
            _note("lstm_bwd/" + name, pec.ratio(got, ref, pec.LSTM_BWD_TOL))
    _report("lstm")


def test_reparam_restatement_within_a_quarter_of_the_bounds():
    for B, Z in pec.REPARAM_SHAPES:
        x = pec.reparam_inputs(B, Z)
        _note("reparam_fwd/zs", pec.ratio(pec.reparam_fwd_f32(x), pec.reparam_fwd_ref(x), pec.REPARAM_FWD_TOL))
        got, ref = pec.reparam_bwd_f32(x), pec.reparam_bwd_ref(x)
        _note("reparam_bwd/d_mean", pec.ratio(got[:, :Z], ref[:, :Z], pec.REPARAM_BWD_TOL))
        _note("reparam_bwd/d_log_var", pec.ratio(got[:, Z:], ref[:, Z:], pec.REPARAM_BWD_TOL))
    for c in pec.PLAIN_CASES:
        x = pec.plain_inputs(c["M"], c["Z"])
        _note("reparam_bwd_plain/d_log_var", pec.ratio(pec.plain_lv_f32(x, c["d_lv_in"]), pec.plain_lv_ref(x, c["d_lv_in"]), pec.REPARAM_BWD_TOL))
        want = x["d_zs"].astype(np.float64) + (x["d_mean_in"] if c["d_mean_in"] else 0.0)
        assert np.array_equal(pec.plain_mean_bits(x, c["d_mean_in"]), want.astype(np.float32))
    _report("reparam")


def test_bce_restatement_within_a_quarter_of_the_bounds():
    for B, D in pec.BCE_SHAPES:
        x = pec.bce_inputs(B, D)
        k = min(pec.BCE_TIES.size, B * D)
        assert np.array_equal(x["R"].reshape(-1)[:k].view(np.int32), pec.BCE_TIES[:k].view(np.int32))
        (loss, g), (loss64, g64) = pec.bce_f32(x), pec.bce_ref(x)
        nz = loss64 != 0                                                    # (a lone pixel at a tie: the reference is exactly 0)
        _note("bce/rec_loss", pec.ratio(loss[nz], loss64[nz], pec.BCE_LOSS_TOL) if nz.any() else 0.0)
        assert not loss[~nz].any()
        _note("bce/d_recon", pec.ratio(g, g64, pec.BCE_GRAD_TOL))
        assert np.array_equal(pec.bce_recon_bits(x), np.clip(x["R"].astype(np.float64), 0.0, 1.0).astype(np.float32))
    _report("bce")


def test_finalize_restatement_and_the_bound_of_the_mean():
    assert pec.MEAN_FIXED_OPS == 11 and pec.mean_bound(1000, 1.0) == 15 * 2.0 ** -24 and pec.mean_bound(256, 2.0) == 12 * 2.0 ** -23
    for c in pec.finalize_cases():
        x = pec.finalize_inputs(c)
        assert int((x["targets"] == x["digits"]).sum()) == c["k"]
        assert 50 <= x["run_loss"].min() and x["run_loss"].max() <= 900 and 100 <= x["rec_loss"].min() and x["rec_loss"].max() <= 2000
        item, mean, acc = pec.finalize_f32(x)
        ref = pec.finalize_ref(x)
        _note("finalize/mean", abs(float(mean) - ref) / pec.mean_bound(c["B"], ref))
        # a sum of small integers is exact in any order: one division
        assert acc == np.float32(c["k"]) / np.float32(c["B"]) and acc.dtype == np.float32
        assert np.array_equal(item, (x["run_loss"].astype(np.float64) + x["rec_loss"]).astype(np.float32))
    _report("finalize")


def test_sigmoid_bits_are_the_float64_product_rounded_thrice():
    x = pec.sigmoid_inputs(1027)
    got = pec.sigmoid_bwd_bits(x)
    g, r = x["g"].astype(np.float64), x["r"].astype(np.float64)
    assert got.dtype == np.float32 and np.abs(got - g * r * (1 - r)).max() <= 3 * 2.0 ** -24 * np.abs(g).max()
    other = x["g"] * (x["r"] * (np.float32(1.0) - x["r"]))                # the other association has other bits
    assert (got.view(np.int32) != other.view(np.int32)).sum() > 50


# ---- argument checks (no launch) ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    return abi.hip()


# entry point -> its arguments without the stream (p: a required pointer, n: a nullable one, S: slab count, D: dimension, 0: flag)
_ENTRY = {
    "air_lstm_gates_fwd": "ppppp" "DD",
    "air_lstm_first_step": "pSnpppn" "DD",
    "air_lstm_gates_bwd": "pnpppppn" "0DD",
    "air_reparam_fwd": "ppp" "DD",
    "air_reparam_bwd": "pppppp" "DD",
    "air_bce_fwd_bwd": "pppppn" "DD",
    "air_finalize": "pppppp" "D",
}


def _good(spec, ptr):
    """p and n: a non-null pointer; S: a slab count; D: a dimension; 0: the accumulate flag"""
    return [ptr if k in "pn" else {"S": 4, "D": 3, "0": 0}[k] for k in spec]


@pytest.mark.parametrize("name", sorted(_ENTRY))
def test_argument_errors(H, name):
    fn, spec = getattr(H.lib(), name), _ENTRY[name]
    ptr = abi.host_ptr()
    # every required pointer in turn
    for i, k in enumerate(spec):
        if k == "p":
            args = _good(spec, ptr)
            args[i] = None
            assert fn(*args, None) == H.EINVAL, (name, i)
    # every dimension zero and negative, with the nullable pointers given and with them NULL: refused for the dimension alone,
    # before any launch (that a NULL there is ACCEPTED shows on the device, and below where another code tells)
    for i, k in enumerate(spec):
        if k == "D":
            for bad in (0, -3):
                for nullable in (ptr, None):
                    args = [nullable if kk == "n" else a for kk, a in zip(spec, _good(spec, ptr))]
                    args[i] = bad
                    assert fn(*args, None) == H.EINVAL, (name, i, bad)


def test_first_step_slab_count(H):
    fn, ptr = H.lib().air_lstm_first_step, abi.host_ptr()
    for n in (0, -1):
        assert fn(ptr, n, ptr, ptr, ptr, ptr, ptr, 3, 3, None) == H.EINVAL
    assert fn(ptr, 9, ptr, ptr, ptr, ptr, ptr, 3, 3, None) == H.ELIMIT
    # bias and h16 are nullable: with both NULL the call gets as far as the slab limit
    assert fn(ptr, 9, None, ptr, ptr, ptr, None, 3, 3, None) == H.ELIMIT
    # ... and a required pointer is missed before the limit is looked at
    assert fn(None, 9, ptr, ptr, ptr, ptr, ptr, 3, 3, None) == H.EINVAL
