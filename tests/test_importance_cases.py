"""CPU-side checks of tests/importance_cases.py: the case tables cover what they say, the inputs meet the conditions the GPU
tests rely on (no degenerate image and no near-tie of the count posterior but in the cases that name one), and the
float64 restatement of air_importance_logw / air_importance_fold has the properties of the quantities it restates."""
import numpy as np
import pytest

import importance_cases as ic


def test_the_shapes_cover_the_edges():
    B, k, T, Z, ldz, K = (set(col) for col in zip(*ic.LOGW_SHAPES))
    assert {3, 65} <= B and {1, 2, 16} <= T and {1, 3, 50, 256} <= Z and {1, 2, 64} <= K
    assert any(s[1] < s[0] for s in ic.LOGW_SHAPES) and (65, 65, 16, 50, 52, 64) in ic.LOGW_SHAPES
    assert max(T) == ic.MAX_STEPS and max(K) == ic.MAX_SAMPLES and max(Z) == ic.MAX_Z
    assert all(s[4] >= s[3] for s in ic.LOGW_SHAPES) and any(s[4] > s[3] for s in ic.LOGW_SHAPES)
    cases = ic.fold_cases()
    assert {c["B"] for c in cases.values()} >= {3, 65, 300} and {c["K"] for c in cases.values()} >= {1, 2, 64}
    assert {c["T"] for c in cases.values()} >= {1, 2, 16} and cases["no_targets"]["targets"] is None
    assert any(c["k"] > ic.GROUP for c in cases.values())                   # more than one group of the sums
    assert len(ic.shape_name(ic.LOGW_SHAPES[0])) and len({ic.shape_name(s) for s in ic.LOGW_SHAPES}) == len(ic.LOGW_SHAPES)


@pytest.mark.parametrize("shape", ic.LOGW_SHAPES, ids=ic.shape_name)
def test_the_logw_inputs_hold_what_the_cases_promise(shape):
    B, k, T, Z, ldz, K = shape
    inp = ic.logw_inputs(shape)
    att, n = inp["att"], inp["steps"]
    assert n[0] == 0 and att[0, 0, ic.ATT_MASK_PREV] == 1 and att[0, 0, ic.ATT_MASK] == 0       # stopped at step 0
    assert (att[1:, 0, ic.ATT_MASK_PREV] == 0).all() and np.isfinite(att[0, 0, ic.ATT_KL_Z])
    if k > 1:
        assert n[1] == T and (att[:, 1, ic.ATT_MASK] == 1).all() and (att[:, 1, ic.ATT_MASK_PREV] == 1).all()
    for key in ("att", "out7", "ml", "z", "eps_scale", "eps_shift", "eps_z"):
        assert np.isnan(inp[key][:, k:]).all(), key                          # rows >= k
    assert np.isnan(inp["rec_loss"][k:]).all() and (inp["run_digits"][k:] == -77).all()
    closed = att[:, :k, ic.ATT_MASK] == 0
    if closed.any():                                                         # NaN records in the steps a gate closes
        assert np.isnan(att[:, :k, ic.ATT_S][closed]).all() and np.isnan(inp["eps_z"][:, :k][closed]).all()
        assert np.isnan(inp["ml"][:, :k][closed]).all() and np.isnan(inp["out7"][:, :k][closed]).all()
    unreached = att[:, :k, ic.ATT_MASK_PREV] == 0
    assert not unreached.any() or np.isnan(att[:, :k, ic.ATT_KL_Z][unreached]).all()
    if ldz > Z:
        assert np.isnan(inp["z"][:, :, Z:]).all()
    logw, digits, terms = ic.logw_reference(inp)
    assert np.isfinite(logw).all() and np.isfinite(terms).all()             # no NaN of a closed step reaches a result
    assert (digits == n[:k]).all()
    # image 0: only rec_loss and the z_pres term of step 0
    assert logw[0] == -(np.float64(inp["rec_loss"][0]) + np.float64(att[0, 0, ic.ATT_KL_Z]))
    assert terms[0, ic.TERM_SCALE] == terms[0, ic.TERM_SHIFT] == terms[0, ic.TERM_WHAT] == 0.0
    # the terms add up to the loss to rounding (they are summed in another association)
    total = terms.sum(axis=1)
    assert np.allclose(-logw, total, rtol=1e-12, atol=0.0)


def test_only_the_named_cases_are_degenerate_or_tied():
    for name, case in ic.fold_cases().items():
        want = ic.expected_fold(name)
        assert tuple(np.flatnonzero(want["degenerate"])) == ic.DEGENERATE_IMAGES.get(name, ()), name
        assert np.isfinite(case["logw"][:, :case["k"]]).all() or name == "degenerate"
        for i in range(case["k"]):
            if want["degenerate"][i]:
                continue
            W = np.sort(want["W"][i][want["W"][i] > 0])[::-1]
            near = len(W) > 1 and (W[0] - W[1]) <= 1e-6 * W[0]
            assert near == (i in ic.TIED.get(name, ())), (name, i, W[:2])
            if near:
                assert W[0] == W[1]                                          # the tie is exact
        assert np.isnan(case["logw"][:, case["k"]:]).all()
    deg = ic.fold_cases()["degenerate"]
    assert (deg["logw"][:, 2] == -np.inf).all() and np.isfinite(deg["logw"][:, :2]).all()
    assert all(np.isinf(p["rec_loss"][2]) for p in ic.degenerate_passes())
    under = ic.fold_cases()["underflow"]
    assert (np.abs(under["logw"][0] - under["logw"][1])[[0, 2]] == 800.0).all() and np.exp(-800.0) == 0.0


@pytest.mark.parametrize("name", sorted(ic.fold_cases()))
def test_properties_of_the_fold_restatement(name):
    case, want = ic.fold_cases()[name], ic.expected_fold(name)
    T, k, K = case["T"], case["k"], case["K"]
    ok = ~want["degenerate"]
    assert (want["bound"][ok] - want["elbo"][ok] >= 0.0).all()               # gap_i >= 0: Jensen
    assert (want["ess"][ok] >= 1.0).all() and (want["ess"][ok] <= K).all()
    assert (want["entropy"][ok] >= 0.0).all() and (want["entropy"][ok] <= np.log(T + 1) + 1e-12).all()
    assert (want["map"][ok] >= 0).all() and (want["map"][ok] <= T).all() and (want["map"][~ok] == -1).all()
    c = want["counts"]
    assert c[ic.IMAGES] == k and c[ic.SCORED] + c[ic.DEGENERATE] == k and c[ic.SPLIT] == want["split"].sum()
    assert c[ic.COUNTS:].sum() == (c[ic.SCORED] if case["targets"] is not None else 0)
    assert c[ic.MAP_CORRECT] == np.trace(c[ic.COUNTS:].reshape(T + 1, T + 1))
    v = ic.values_of(c, want["sums"], K, case["targets"] is not None)
    assert v[2] >= 0.0 and 1.0 / K <= v[3] <= 1.0 and np.isnan(v[4]) == (case["targets"] is None)


def test_one_sample_is_its_own_bound():
    case, want = ic.fold_cases()["b3_t1_s1"], ic.expected_fold("b3_t1_s1")
    assert ic.bits(want["bound"]) == ic.bits(case["logw"][0, :3]) == ic.bits(want["elbo"])
    assert (want["ess"] == 1.0).all() and (want["entropy"] == 0.0).all() and not want["split"].any()


def test_underflow_tie_and_accumulation():
    under = ic.expected_fold("underflow")
    assert under["ess"][0] == 1.0 and under["ess"][2] == 1.0 and under["map"].tolist() == [1, 2, 1]
    assert under["W"][0].tolist() == [0.0, 1.0, 0.0] and under["entropy"][0] == 0.0
    tie = ic.expected_fold("tie")
    assert tie["map"].tolist() == [1, 0, 1] and tie["split"].tolist() == [True, True, False]
    assert (tie["ess"] == 4.0).all() and tie["entropy"][0] == tie["entropy"][1] == np.log(2.0)
    # a second call adds to the first
    case = ic.fold_cases()["b65_t2_s2"]
    once = ic.expected_fold("b65_t2_s2")
    twice = ic.fold_reference(case, once["counts"], once["sums"])
    assert (twice["counts"] == 2 * once["counts"]).all() and np.allclose(twice["sums"], 2 * once["sums"], rtol=1e-14)


def test_a_ratio_at_the_prior_is_exactly_zero():
    """eps = 0, the sample at the prior mean, the posterior's log-variance the prior's: log q - log p = 0, bit for bit"""
    for pm, pv in ic.PRIORS.values():
        pm, pv = np.float64(np.float32(pm)), np.float64(np.float32(pv))
        plv = np.float64(np.log(np.float32(pv)))
        assert ic.lr_gauss(pm, np.float64(0.0), plv, pm, pv, plv) == 0.0
    assert ic.fold_bound(64, 16) == 8 * 82 * 2.0 ** -52
