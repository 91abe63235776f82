"""CPU-side checks of the case table of the latent clusters (tests/latent_kmeans_cases.py): a cap only keeps a test honest
if the reference meets it, so every case has to show what it is there for -- the unconverged case stops at max_iters, the
duplicate case has a cluster without members, the tie is a tie, the start rows of a restart are distinct -- and the
restatement has to behave like k-means: the inertia does not rise from one iteration to the next, and the three scores do
not depend on how the clusters are numbered.  (What the kernels compute: tests/test_gpu_latent_kmeans.py.)"""
import numpy as np
import pytest

import latent_kmeans_cases as kc

CASES = kc.cases()


def test_the_table_holds_the_shapes_it_promises():
    Ms, Zs, ks, Rs = (set(s[i] for s in kc.SHAPES) for i in range(4))
    assert {1, 2, 63, 64, 65, 257, 700} <= Ms and {1, 3, 50} <= Zs and {1, 2, 3, 10} <= ks and {1, 8} <= Rs
    assert (65, kc.MAX_Z, kc.MAX_K, kc.MAX_RESTARTS) in kc.SHAPES
    for name, c in CASES.items():
        M, Z = c["x"].shape
        assert 1 <= M <= kc.MAX_ROWS and 1 <= Z <= kc.MAX_Z and 1 <= c["k"] <= kc.MAX_K and 1 <= c["classes"] <= kc.MAX_CLASSES, name
        assert 1 <= c["restarts"] <= kc.MAX_RESTARTS and 1 <= c["max_iters"] <= kc.MAX_ITERS, name
        me = kc.effective_rows(M, c["rows"])
        assert np.isnan(c["x"][me:]).all(), name                 # garbage beyond the cursor


@pytest.mark.parametrize("name", sorted(CASES))
def test_start_rows_are_distinct_valid_rows_and_the_inertia_does_not_rise(name):
    c, want = CASES[name], kc.expected(name)
    V = int(want["counts"][kc.VALID])
    if V == 0:
        assert np.isnan(want["restart_inertia"]).all() and not want["restart_iters"].any() and (want["assignment"] == -1).all()
        assert not want["counts"][kc.LABELLED:kc.COUNTS + c["k"]].any() and np.isnan(want["centroids"]).all()
        return
    ok = np.isfinite(c["x"][:kc.effective_rows(len(c["x"]), c["rows"])]).all(axis=1)
    for r, (start, trace) in enumerate(zip(want["starts"], want["traces"])):
        assert len(set(start)) == len(start) == min(c["k"], V) and all(ok[i] for i in start), (name, r)
        assert len(trace) == want["restart_iters"][r] and trace[-1] == want["restart_inertia"][r]
        for before, after in zip(trace, trace[1:]):
            assert after <= before * (1.0 + V * 2.0 ** -52), (name, r, before, after)
    best = int(want["counts"][kc.BEST])
    assert want["restart_inertia"][best] == want["restart_inertia"].min() == want["restart_inertia"][:best + 1].min()
    assert best == 0 or (want["restart_inertia"][:best] > want["restart_inertia"][best]).all()
    sizes, majority, table = kc.parts(want["counts"], c["k"], c["classes"])
    assert sizes.sum() == V == (want["assignment"] >= 0).sum() and want["counts"][kc.LIVE] == (sizes > 0).sum()
    assert table.sum() == want["counts"][kc.LABELLED] <= V and (table.sum(axis=1) <= sizes).all()


def test_three_blobs_tie_in_every_restart_and_are_pure():
    c, want = CASES["three_blobs"], kc.expected("three_blobs")
    assert len(set(want["restart_inertia"].tobytes()[8 * r:8 * r + 8] for r in range(8))) == 1       # all eight to the bit
    partitions = {tuple(sorted(np.bincount(a, minlength=3))) for a in [want["assignment"]]}
    assert partitions == {(21, 22, 22)}
    assert want["counts"][kc.BEST] == 0 and want["counts"][kc.RESTARTS_CONVERGED] == 8 and want["counts"][kc.CONVERGED] == 1
    assert 2 <= want["restart_iters"].min() and want["restart_iters"].max() <= 3
    assert all(len({i % 3 for i in s}) == 3 for s in want["starts"])
    assert want["counts"][kc.CORRECT] == want["counts"][kc.LABELLED] == 65
    assert len({tuple(s) for s in want["starts"]}) > 1          # the restarts did start from different rows
    assert kc.scores(kc.parts(want["counts"], 3, 3)[2]) == (1.0, 1.0, 1.0)


def test_the_unconverged_case_stops_at_max_iters_and_its_twin_converges():
    short, long_ = kc.expected("unconverged"), kc.expected("converged")
    assert short["restart_iters"].tolist() == [3, 3] and short["counts"][kc.CONVERGED] == 0 and short["counts"][kc.RESTARTS_CONVERGED] == 0
    assert short["counts"][kc.ITERS] == 3
    assert long_["counts"][kc.CONVERGED] == 1 and long_["counts"][kc.RESTARTS_CONVERGED] == 2
    assert (long_["restart_iters"] > 3).all() and (long_["restart_iters"] < 100).all(), long_["restart_iters"]
    # the traces of the two agree for the three iterations they share
    assert [t[:3] for t in long_["traces"]] == short["traces"]


def test_the_duplicate_case_has_a_cluster_without_members_that_keeps_its_centroid():
    c, want = CASES["duplicates"], kc.expected("duplicates")
    sizes = kc.parts(want["counts"], 3, 2)[0]
    assert want["counts"][kc.LIVE] == 2 and sorted(sizes.tolist()) == [0, 4, 4] and want["counts"][kc.VALID] == 8
    empty = int(np.argmin(sizes))
    start = want["starts"][int(want["counts"][kc.BEST])]
    assert want["centroids"][empty].tobytes() == c["x"][start[empty]].astype(np.float64).tobytes()       # never updated
    assert want["restart_inertia"][want["counts"][kc.BEST]] == 0.0 and want["counts"][kc.CORRECT] == 8


def test_the_exact_tie_goes_to_the_lower_cluster():
    c, want = CASES["exact_tie"], kc.expected("exact_tie")
    assert want["starts"][0] == [0, 1]
    mu = c["x"][[0, 1]].astype(np.float64)
    d2 = kc.distances(c["x"].astype(np.float64), mu)
    assert d2[2, 0] == d2[2, 1] == 1.0                           # the tie is a tie
    assert want["assignment"].tolist() == [0, 1, 0] and want["row_d2"].tolist() == [0.0, 0.0, 1.0]
    assert want["restart_iters"].tolist() == [1] and want["counts"][kc.CONVERGED] == 0


def test_edges_show_what_they_are_there_for():
    get = lambda name, key: int(kc.expected(name)["counts"][key])             # noqa: E731
    assert get("nan_row", kc.VALID) == 36 and kc.expected("nan_row")["assignment"][9] == -1
    assert get("inf_rows", kc.VALID) == 35
    assert get("labels_out_of_range", kc.VALID) == 37 and get("labels_out_of_range", kc.LABELLED) == 34
    assert (kc.expected("labels_out_of_range")["assignment"][9:12] >= 0).all()
    v2 = kc.expected("v_below_k")
    assert get("v_below_k", kc.VALID) == 2 and np.isnan(v2["centroids"][2:]).all() and np.isfinite(v2["centroids"][:2]).all()
    assert get("v_below_k", kc.LIVE) == 2 and sorted(v2["assignment"][[9, 20]].tolist()) == [0, 1]
    assert get("one_valid", kc.VALID) == 1 and get("one_valid", kc.LIVE) == 1
    assert get("all_invalid", kc.VALID) == 0 and get("all_invalid", kc.ROWS) == 37
    assert get("labels_null", kc.LABELLED) == 0 and get("labels_null", kc.VALID) == 37
    assert (kc.parts(kc.expected("labels_null")["counts"], 4, 4)[1] == -1).all()
    assert [get(n, kc.ROWS) for n in ("rows_zero", "rows_less", "rows_more", "rows_negative")] == [0, 21, 37, 0]


def test_scores_do_not_depend_on_the_numbering_of_the_clusters():
    rng = np.random.RandomState(5)
    for name in ("m257_z3_k10_r8", "m700_z50_k10_r1", "unconverged", "labels_out_of_range"):
        c = CASES[name]
        table = kc.parts(kc.expected(name)["counts"], c["k"], c["classes"])[2]
        want = kc.scores(table)
        assert all(v == v for v in want), (name, want)
        for _ in range(4):
            got = kc.scores(table[rng.permutation(len(table))])
            assert got[0] == want[0] and got[1] == want[1] and abs(got[2] - want[2]) <= kc.score_allowance(c["k"], c["classes"]), name
    assert kc.scores(np.zeros((3, 3), np.int64)) != kc.scores(np.zeros((3, 3), np.int64))       # NaN: nothing labelled
    one = kc.scores(np.asarray([[5, 0], [0, 0]]))
    assert one[0] == 1.0 and one[1] != one[1] and one[2] != one[2]              # one cluster, one class: zero denominators
    # hand-made: two clusters, two classes, one row misplaced
    acc, ari, nmi = kc.scores(np.asarray([[3, 1], [0, 4]]))
    assert acc == 7 / 8 and abs(ari - (9 - 13 * 12 / 28) / (12.5 - 13 * 12 / 28)) < 1e-15 and 0 < nmi < 1
