"""CPU checks of the latent probe's case table (tests/latent_probe_cases.py): the two restatements of include/air_hip.h's
"latent probe" section agree to the bit on every case, and the inputs have the properties the GPU test relies on -- ties at
the k-th neighbour that straddle reference tiles and splits, shared top votes, exact duplicates, a case without ties, and a
named case for every branch of the validity rule -- so that tests/test_gpu_latent_probe.py cannot pass vacuously."""
import numpy as np
import pytest

import latent_probe_cases as pc

CASES = pc.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_restatements_agree_to_the_bit(name):
    c = CASES[name]
    scalar = pc.probe_scalar(c["x"], c["labels"], c["k"], c["classes"], c["au_threshold"], c["rows"])
    assert pc.same_bits(pc.expected(name), scalar) == []


def test_the_table_holds_the_shapes_the_kernel_can_go_wrong_at():
    shapes = {(len(c["x"]), c["x"].shape[1], c["k"], c["classes"]) for c in CASES.values()}
    for M in (1, 2, 5, 6, 63, 64, 65, pc.QUERY_TILE - 1, pc.QUERY_TILE, pc.QUERY_TILE + 1, pc.REF_TILE - 1, pc.REF_TILE,
              pc.REF_TILE + 1, pc.MAX_SPLITS * pc.REF_TILE + 1, 16, 17):
        assert any(s[0] == M for s in shapes), M
    assert max(s[0] for s in shapes) <= 600
    assert {1, 2, 50, 51, 256} <= {s[1] for s in shapes} and {1, 5, 16} <= {s[2] for s in shapes}
    assert {1, 2, 10, 64} <= {s[3] for s in shapes}
    assert (5, 50, 5, 10) in shapes and (6, 50, 5, 10) in shapes and (16, 51, 16, 10) in shapes and (17, 256, 16, 64) in shapes
    # beyond the full set of splits a run holds more than one reference tile, and the last runs are empty
    M = pc.MAX_SPLITS * pc.REF_TILE + 1
    assert pc.splits(M) == pc.MAX_SPLITS and pc.split_of(M - 1, M) < pc.MAX_SPLITS - 1 and pc.split_of(pc.REF_TILE, M) == 0
    assert pc.splits(pc.REF_TILE) == 1 and pc.splits(pc.REF_TILE + 1) == 2


def test_the_tie_case_ties_across_tiles_and_splits():
    c = CASES["ties"]
    M = len(c["x"])
    assert (M, c["x"].shape[1], c["k"], c["classes"]) == (130, 3, 5, 10)
    assert set(np.unique(c["x"]).tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    ties = pc.boundary_ties(c)
    assert len(ties) == M
    tied = [i for i, (tie, _, _) in ties.items() if tie]
    across = [i for i in tied if pc.tile_of(ties[i][1]) != pc.tile_of(ties[i][2])
              and pc.split_of(ties[i][1], M) != pc.split_of(ties[i][2], M)]
    print("ties at the k-th neighbour: %d of %d queries, %d of them across reference tiles and splits" % (len(tied), M, len(across)))
    assert len(tied) * 4 >= M and len(across) >= 10
    # ... and inside one tile between the rows of two waves, whose lists the workgroup merges
    waves = [i for i in tied if pc.tile_of(ties[i][1]) == pc.tile_of(ties[i][2]) and pc.pass_of(ties[i][1]) != pc.pass_of(ties[i][2])]
    print("ties inside a tile across the rows of two waves: %d" % len(waves))
    assert len(waves) >= 10
    # among equal distances the smaller row wins: a neighbour list that is not sorted by row alone
    nb = pc.expected("ties")["neighbours"]
    assert any((np.diff(nb[i]) < 0).any() for i in tied)


def test_the_tie_case_shares_top_votes():
    shared = pc.shared_top_votes(CASES["ties"], pc.expected("ties"))
    print("rows whose top vote is shared: %d" % len(shared))
    assert len(shared) >= 10
    # and the earliest neighbour does not always win: some winner is not the nearest neighbour's class
    res, labels = pc.expected("ties"), CASES["ties"]["labels"]
    assert any(res["pred"][i] != labels[res["neighbours"][i, 0]] for i in range(130))
    assert any(res["pred"][i] == labels[res["neighbours"][i, 0]] for i in shared)


def test_the_duplicate_case_has_pairs_at_distance_zero():
    res = pc.expected("duplicates")
    zero = [(i, int(res["neighbours"][i, 0])) for i in range(40) if res["neighbour_d2"][i, 0] == 0.0 and res["neighbours"][i, 0] >= 0]
    pairs = {tuple(sorted(p)) for p in zero}
    assert len(pairs) >= 8 and all(res["neighbour_d2"][i, 0].tobytes() == np.float64(0.0).tobytes() for i, _ in zero)
    assert any(pc.tile_of(a) != pc.tile_of(b) for a, b in pairs)


def test_the_gaussian_case_has_no_ties():
    ties = pc.boundary_ties(CASES["gaussian"])
    assert len(ties) == 130 and not any(tie for tie, _, _ in ties.values())
    res = pc.expected("gaussian")
    Z = CASES["gaussian"]["x"].shape[1]
    assert 0 < res["counts"][pc.ACTIVE_UNITS] < Z                # some units move, some do not
    assert res["counts"][pc.SCORED] == 130 and 0 < res["counts"][pc.CORRECT] < 130


def test_every_branch_of_the_validity_rule_has_a_case():
    base = 37
    for kind in ("nan_row", "label_negative", "label_too_large"):
        res, at = pc.expected(kind), CASES[kind]["planted"][kind]
        assert res["counts"][pc.VALID] == base - 1 and res["pred"][at] == -1 and not (res["neighbours"] == at).any(), kind
        assert res["counts"][pc.SCORED] == base - 1
    res, at = pc.expected("inf_row"), CASES["inf_row"]["planted"]["inf_row"]
    assert res["counts"][pc.VALID] == base - 2 and not np.isin(res["neighbours"], (at, at + 20)).any()
    res = pc.expected("all_invalid")
    assert res["counts"][:pc.COUNTS].tolist() == [base, 0, 0, 0, 0] and np.isnan(res["moments"]).all() and (res["pred"] == -1).all()
    res, at = pc.expected("one_valid"), CASES["one_valid"]["planted"]["one_valid"]
    assert res["counts"][:pc.COUNTS - 1].tolist() == [base, 1, 0, 0] and (res["pred"] == -1).all()
    assert res["moments"][0] == 0.5 and (res["moments"][5:] == 0.0).all()


def test_the_rows_cases_clamp_and_hide_the_rest():
    want = {"rows_zero": 0, "rows_less": 41, "rows_more": 70, "rows_negative": 0}
    for name, me in want.items():
        c, res = CASES[name], pc.expected(name)
        assert res["counts"][pc.ROWS] == me and res["counts"][pc.VALID] == me, name
        assert np.isnan(c["x"][me:]).all() and (res["pred"][me:] == -1).all() and (res["neighbours"] < me).all()
    assert np.isnan(pc.expected("rows_zero")["moments"]).all()


def test_small_sets_keep_fewer_than_k_neighbours():
    assert (pc.expected("m1_z50_k5_c10")["pred"] == -1).all()                      # one row: nothing to compare with
    two = pc.expected("m2_z50_k5_c10")
    assert two["neighbours"][:, 0].tolist() == [1, 0] and (two["neighbours"][:, 1:] == -1).all()
    assert two["neighbour_d2"][0, 0] == two["neighbour_d2"][1, 0] and (two["neighbour_d2"][:, 1:] == 0.0).all()
    assert (pc.expected("m5_z50_k5_c10")["neighbours"][:, 4] == -1).all() and (pc.expected("m6_z50_k5_c10")["neighbours"] >= 0).all()


def test_derived_values():
    counts = np.zeros(pc.COUNTS + 4, np.int64)
    assert np.isnan(pc.derived(counts, 0, 0)[[0, 3]]).all() and pc.derived(counts, 0, 0)[[1, 2]].tolist() == [0.0, 0.0]
    counts[pc.SCORED], counts[pc.CORRECT], counts[pc.ACTIVE_UNITS] = 8, 6, 3
    assert pc.derived(counts, 9, 12).tolist() == [0.75, 3.0, 8.0, 0.75]
