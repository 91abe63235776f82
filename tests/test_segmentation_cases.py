"""The case tables of the segmentation tests hold what they claim (tests/segmentation_cases.py; CPU only): the planted
branches are there, and the restated FG-ARI is the adjusted Rand index."""
import numpy as np
import pytest

import segmentation_cases as sc


@pytest.fixture(scope="module")
def branches():
    case = sc.gpu_cases()["branches"]
    (pred, tables, ari, iou), counts, sums = sc.expected("branches")[0][0], *sc.expected("branches")[1:]
    return case, case["chunks"][0], pred, tables, ari, iou, counts, sums


def _terms(case, ch, i):
    return sc.step_terms(ch["att"], ch["vrec"], i, case["C"], case["w"])


def test_shapes_are_the_issue_table():
    assert sc.SHAPES == [(1, 1, 1, 1, 8, 4), (2, 2, 3, 4, 16, 8), (3, 2, 5, 8, 15, 7), (16, 16, 2, 2, 12, 6), (5, 4, 2, 2, 128, 32),
                         (3, 2, 257, 260, 10, 4)]
    for T, G, k, B, C, w in sc.SHAPES:
        assert T <= sc.MAX_STEPS and G <= sc.MAX_DIGITS and C <= sc.MAX_CANVAS and w <= sc.MAX_WINDOW and k <= B
    assert [(C * C) % 16 == 0 for (_, _, _, _, C, _) in sc.SHAPES] == [True, True, False, True, True, False]
    assert -(-257 // sc.GROUP) == 2


def test_overlap_off_canvas_and_inactive_step(branches):
    case, ch, pred, tables, *_ = branches
    at, C = case["planted"], case["C"]
    # overlapping windows: both of the first two steps are above the threshold on some pixel, and each wins somewhere
    terms, active = _terms(case, ch, at["overlap"])
    both = (terms[0] > 0.5) & (terms[1] > 0.5)
    assert active.all() and both.sum() > 4
    assert {1, 2} <= set(pred[at["overlap"]].reshape(C, C)[both].tolist())
    # a window partly off the canvas: taps clipped on the far side (both indices equal) for some columns, not for all
    rec = ch["att"][0, at["off_canvas"]]
    _, _, i0, i1 = sc.axis_taps(C, case["w"], sc.f32(1) / rec[sc.ATT_S], -rec[sc.ATT_X] / rec[sc.ATT_S])
    assert 0 < (i0 == i1).sum() < C
    # the inactive step would have taken pixels, takes none, and a later step is active
    terms, active = _terms(case, ch, at["inactive_between"])
    assert active.tolist() == [True, False, True, True]
    assert (terms[1] > np.maximum(np.maximum(terms[0], terms[2]), np.maximum(terms[3], 0.5))).sum() > 10
    assert 2 not in pred[at["inactive_between"]] and {3, 4} & set(pred[at["inactive_between"]].tolist())


def test_the_tie_exists_and_goes_to_the_smaller_step(branches):
    case, ch, pred, *_ = branches
    i = case["planted"]["tie"]
    terms, active = _terms(case, ch, i)
    assert active.all() and terms[1].tobytes() == terms[2].tobytes()
    lab = pred[i].reshape(case["C"], case["C"])
    tied_best = (terms[1] > 0.5) & (terms[1] > terms[0])
    assert tied_best.sum() > 10 and (lab[tied_best] == 2).all() and 3 not in lab


def test_nan_zero_presence_and_the_threshold_itself(branches):
    case, ch, pred, tables, ari, iou, *_ = branches
    at, C = case["planted"], case["C"]
    terms, _ = _terms(case, ch, at["nan_window"])
    nan = np.isnan(terms[0])
    assert 0 < nan.sum() < C * C and (pred[at["nan_window"]].reshape(C, C)[nan] != 1).all()
    assert 1 in pred[at["nan_window"]]                                      # ... and the step still takes other pixels
    terms, active = _terms(case, ch, at["z_zero"])
    assert active.all() and (terms == 0).all() and (pred[at["z_zero"]] == 0).all()
    terms, active = _terms(case, ch, at["at_threshold"])
    assert active.tolist() == [True, False, False, False]
    assert terms[0][0, 0] == sc.f32(0.5) == sc.f32(case["thr"]) and pred[at["at_threshold"]][0] == 0
    assert ch["gt_mask"][at["at_threshold"]][0] == 1                        # a foreground pixel nobody claims
    assert 1 in pred[at["at_threshold"]]


def test_m_equals_e_and_the_unscored_image(branches):
    case, ch, pred, tables, ari, iou, counts, sums = branches
    at = case["planted"]
    t = tables[at["z_zero"]]
    assert t[2, 0] == 30 and t[1:].sum() == 30                              # one truth label, one predicted cluster
    assert ari[at["z_zero"]] == 1.0 and iou[at["z_zero"]].tolist() == [0.0, 0.0, 0.0]
    assert tables[at["unscored"]][1:].sum() == 0 and np.isnan(ari[at["unscored"]])
    assert counts[sc.IMAGES] == 8 and counts[sc.SCORED] < 8
    assert counts[sc.FG_MISSED] > 0 and counts[sc.BG_CLAIMED] > 0 and counts[sc.PRESENT] > 0
    # a single foreground pixel is not enough either
    scored, a, _, _ = sc.scores_from_table([[5, 5], [1, 0]])
    assert not scored and np.isnan(a)
    # a label beyond G counts as background
    assert sc.table_of(np.asarray([0, 1, 2, 200], np.uint8), np.asarray([0, 1, 1, 1], np.uint8), 2, 1).tolist() == [[1, 1], [0, 1], [0, 1]]


def test_fg_ari_perfect_independent_and_degenerate():
    # a relabelled perfect partition: truth 1, 2, 3 predicted as 3, 1, 2; the background row is ignored whatever it holds
    n = np.asarray([[50, 7, 9, 11], [0, 0, 0, 40], [0, 25, 0, 0], [0, 0, 31, 0]])
    scored, ari, iou, tot = sc.scores_from_table(n)
    assert scored and ari == 1.0 and tot == dict(present=3, fg=96, missed=0, claimed=27)
    assert iou.tolist() == [40 / 51, 25 / 32, 31 / 40]
    # a split independent of the truth: every truth row spread over the clusters in the same proportions
    scored, ari, _, _ = sc.scores_from_table(np.asarray([[0, 0, 0], [0, 300, 300], [0, 200, 200]]))
    assert scored and abs(ari) < 2e-3
    # M == E: everything in one cluster and one truth label
    assert sc.scores_from_table([[3, 0], [0, 9]])[1] == 1.0
    # one cluster over two truth labels: E == Bs-side degenerate, ARI 0
    assert sc.scores_from_table([[0, 0], [0, 5], [0, 5]])[1] == 0.0


def test_fg_ari_agrees_with_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(4)
    for G, T in ((2, 3), (4, 2), (16, 16), (1, 1)):
        for _ in range(5):
            truth = rng.randint(0, G + 1, 400).astype(np.uint8)
            pred = rng.randint(0, T + 1, 400).astype(np.uint8)
            pred = np.where(rng.uniform(size=400) < 0.5, np.minimum(truth, T), pred)      # correlated, not equal
            scored, ari, _, _ = sc.scores_from_table(sc.table_of(truth, pred, G, T))
            fg = truth > 0
            assert scored and abs(ari - metrics.adjusted_rand_score(truth[fg], pred[fg])) <= 1e-12


def test_summation_tree_and_derived_values():
    v = np.arange(1, 258, dtype=np.float64) * 0.1
    want = np.float64(0.0) + sc.group_tree(v[:256])
    want = want + sc.group_tree(np.concatenate([v[256:], np.zeros(255)]))
    assert sc.batch_total(v) == want
    x = [np.float64(1e16), 1.0, 1.0, 1.0]                                     # the tree is not the running sum
    assert sc.group_tree(np.asarray(x + [0.0] * 252)) == (x[0] + x[1]) + (x[2] + x[3]) != ((x[0] + x[1]) + x[2]) + x[3]
    counts, sums = sc.empty_accumulators()
    assert np.isnan(sc.derived(counts, sums, 10)).all()
    counts[:] = [2, 1, 3, 40, 10, 16]
    sums[:] = [0.5, 1.5]
    assert sc.derived(counts, sums, 10).tolist() == [0.5, 0.5, 0.25, 0.1]


def test_scene_masks_smallest_digit_wins_on_hand_placed_glyphs():
    s = sc.hand_scene()
    C = s["C"]
    mask = sc.scene_masks(s["glyphs"], s["crops"], s["digits"], s["indices"], s["positions"], C).reshape(2, C, C)
    want = np.zeros((C, C), np.uint8)
    want[1:7, 1:7] = 3                                                        # the block, under ...
    want[2:6, 2:7:2] = 1                                                      # ... the comb of digit 0 ...
    want[2:6, 3:8:2] = 2                                                      # ... and that of digit 1 (one tooth beyond the block)
    assert mask[0].tolist() == want.tolist()
    # boxes of digits 0 and 1 intersect, their inks do not
    assert max(2, 3) < min(2 + 5, 3 + 5) and not ((want == 1) & (want == 2)).any()
    # scene 1: an index outside the table and a crop that leaves its frame label nothing; the slot past digits[b] neither
    only = np.zeros((C, C), np.uint8)
    only[5:9, 4:9:2] = 3
    assert mask[1].tolist() == only.tolist()
    # the threshold is strict, and above every value nothing is ink
    m = sc.scene_masks(s["glyphs"], s["crops"], s["digits"], s["indices"], s["positions"], C, ink_threshold=0.75).reshape(2, C, C)
    assert set(np.unique(m[0]).tolist()) == {0, 1} and not m[1].any()
