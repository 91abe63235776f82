"""CPU checks of tests/localization_cases.py: hand-checked boxes through the restatement, and every table the GPU tests use
(tests/test_gpu_localization.py) holds what it claims to exercise -- a table may not silently miss a branch."""
import math

import numpy as np
import pytest

import localization_cases as lc

C = 50


def _one(gt, rec):
    """(iou, cover) of one digit (x, y, w, h) against one record (s, x, y)"""
    return lc.pair(lc.inferred_box(*rec, C), *gt)


# --------------------------------------------------------------------------------------------------------- hand-checked
@pytest.mark.parametrize("gt", [(10, 12, 20, 20), (0, 0, 28, 28), (22, 22, 28, 28), (31, 3, 9, 9)])
def test_a_record_built_from_a_box_scores_it(gt):
    rec = lc.record_for_box(gt[0], gt[1], gt[2], C)
    assert all(isinstance(v, np.float32) for v in rec)
    l, r, t, b = lc.inferred_box(*rec, C)
    assert max(abs(l - gt[0]), abs(r - gt[0] - gt[2]), abs(t - gt[1]), abs(b - gt[1] - gt[3])) < 1e-4
    iou, cover = _one(gt, rec)
    assert 0.99 <= iou <= 1.0 and cover >= 0.99
    case = dict(T=1, B=1, G=1, canvas_size=C, tau=0.5)
    chunk = dict(k=1, att=np.zeros((1, 1, 16), np.float32), run_digits=np.ones(1, np.int32), gt_count=np.ones(1, np.int32),
                 gt_positions=np.asarray([[gt[:2]]], np.int32), gt_boxes=np.asarray([[gt[2:]]], np.int32))
    chunk["att"][0, 0, :3] = rec
    counts, sums = lc.empty_accumulators(case)
    match, ious = lc.apply_chunk(case, chunk, counts, sums)
    assert match.tolist() == [[0]] and ious[0, 0] == iou
    assert counts[:lc.COUNTS].tolist() == [1, 1, 1, 1, 1, 1] and lc.confusion(case, counts).tolist() == [[0, 0], [0, 1]]
    # (the record maps pixels by (C - 1.001) / 2, the reference's centre by (C - 1) / 2: up to 0.001 / 49 of a coordinate <= 2)
    assert sums[lc.IOU] == iou and sums[lc.COVER] == cover and sums[lc.DIST] < 1e-4
    assert lc.derived(counts, sums).tolist() == [iou, 1.0, 1.0, cover, sums[lc.DIST], 1.0]


def test_the_same_box_moved_by_its_width_scores_nothing():
    gt = (5, 12, 20, 20)
    rec = lc.record_for_box(25.01, 12, 20, C)                   # (a hair beyond: the float32 record rounds either way)
    assert _one(gt, rec) == (0.0, 0.0)
    assert lc.match_image([list(rec) + [0.0] * 13], 1, [gt[:2]], [gt[2:]], 1, C) == {}


def test_a_box_of_twice_the_side_covers_the_digit():
    gt = (15, 15, 14, 14)
    iou, cover = _one(gt, lc.record_for_box(8, 8, 28, C))
    assert cover == 1.0 and abs(iou - 0.25) < 1e-4


def test_a_window_outside_the_canvas_has_no_area():
    l, r, t, b = lc.inferred_box(0.2, 3.0, 0.0, C)
    assert l == r == float(C) and (r - l) * (b - t) == 0.0
    assert _one((30, 10, 20, 20), (0.2, 3.0, 0.0)) == (0.0, 0.0)
    l, r, t, b = lc.inferred_box(0.2, 0.0, -3.0, C)
    assert t == b == 0.0
    assert _one((10, 0, 20, 20), (0.2, 0.0, -3.0)) == (0.0, 0.0)


def test_nan_and_the_clip():
    assert math.isnan(lc.clip(float("nan"), 50.0)) and lc.clip(-0.0, 50.0) == 0.0 and lc.clip(51.0, 50.0) == 50.0
    for rec in ((lc.NAN, 0.0, 0.0), (0.4, lc.NAN, 0.0), (0.4, 0.0, lc.NAN)):
        assert _one((10, 10, 20, 20), rec) == (0.0, 0.0)
    assert lc.center_distance(0.0, 0.0, 11, 11, 28, 28, 50) == 0.0
    assert lc.center_distance(3 / 32, 4 / 32, 11, 11, 28, 28, 50) == 5 / 32


def test_the_group_tree_and_the_fold():
    v = [float(i) * 0.1 for i in range(lc.GROUP)]
    want = v
    for _ in range(8):
        want = [want[2 * m] + want[2 * m + 1] for m in range(len(want) // 2)]
    assert lc.group_tree(v) == want[0] and len(want) == 1
    assert lc.group_tree([0.0] * lc.GROUP) == 0.0
    nan = lc.derived(np.zeros(lc.COUNTS, np.int64), np.zeros(lc.SUMS))
    assert np.isnan(nan).all() and len(nan) == len(lc.NAMES)


# ------------------------------------------------------------------------------------------------------------ the tables
def _images(case):
    for ci, ch in enumerate(case["chunks"]):
        for i in range(ch["k"]):
            yield ci, ch, i


def test_the_shapes_are_the_issues():
    cases = lc.gpu_cases()
    got = {(c["T"], c["G"], c["chunks"][0]["k"], c["B"]) for c in cases.values() if len(c["chunks"]) == 1}
    assert {(1, 1, 1, 1), (3, 2, 5, 8), (16, 16, 7, 7), (3, 2, 64, 64), (3, 2, 65, 70), (3, 2, 257, 260), (4, 3, 32, 32)} <= got
    assert lc.GROUP == 256 and [ch["k"] for ch in cases["two_chunks"]["chunks"]] == [5, 3]
    for c in cases.values():
        for ch in c["chunks"]:
            assert ch["att"].shape == (c["T"], c["B"], 16) and ch["att"].dtype == np.float32
            assert ch["gt_positions"].shape == ch["gt_boxes"].shape == (ch["k"], c["G"], 2)
            assert ch["gt_positions"].dtype == ch["gt_boxes"].dtype == ch["gt_count"].dtype == ch["run_digits"].dtype == np.int32
            assert np.isnan(ch["att"][:, ch["k"]:]).all() and (ch["run_digits"][ch["k"]:] > 0).all()


def test_the_branch_table_holds_every_branch():
    case = lc.gpu_cases()["branches"]
    ch, T, G, tau = case["chunks"][0], case["T"], case["G"], case["tau"]
    at = case["planted"]
    assert sorted(at) == sorted(lc.PLANTED) and len(set(at.values())) == len(at)

    def scored(name):
        i = at[name]
        c, n, match, ious, p, hits = lc.score_image(case, ch, i)
        m = lc.iou_matrix(ch["att"][:, i], n, ch["gt_positions"][i], ch["gt_boxes"][i], c, case["canvas_size"])
        return c, n, match, ious, m, hits

    c, n, match, ious, m, _ = scored("tie_objects")              # an exact tie between two objects: the smaller t
    assert (c, n) == (1, 2) and m[0][0] == m[0][1] > 0 and match[0] == 0
    c, n, match, ious, m, _ = scored("tie_digits")               # and between two digits: the smaller g
    assert (c, n) == (2, 1) and m[0][0] == m[1][0] > 0 and match[:2] == [0, -1]
    c, n, match, ious, m, _ = scored("unmatched_digit")
    assert (c, n) == (2, 1) and match[:2] == [0, -1] and ious[1] == 0.0
    c, n, match, ious, m, _ = scored("unmatched_object")
    assert (c, n) == (1, 2) and match[0] == 0 and m[0][1] == 0.0
    assert scored("no_digits")[:2] == (0, 1) and scored("no_objects")[:2] == (1, 0) and scored("neither")[:2] == (0, 0)
    for name in ("no_digits", "no_objects", "neither"):
        assert scored(name)[2] == [-1] * G
    i = at["above_T"]
    assert ch["run_digits"][i] > T and scored("above_T")[1] == T and sorted(scored("above_T")[2][:2]) == [0, 3]
    i = at["below_zero"]
    assert ch["run_digits"][i] < 0 and scored("below_zero")[1] == 0 and scored("below_zero")[2] == [-1] * G
    c, n, match, ious, m, _ = scored("nan")                      # NaN records inside t < n: never taken, the rest goes on
    i = at["nan"]
    assert np.isnan(ch["att"][0, i, lc.ATT_S]) and np.isnan(ch["att"][1, i, lc.ATT_X]) and n == 3
    assert m[0] == [0.0, 0.0, 0.0] and match[:2] == [-1, 2]
    c, n, match, ious, m, hits = scored("at_tau")                # a pair exactly at tau is a hit
    assert ious[0] == tau == 0.5 and hits == 1
    c, n, match, ious, m, _ = scored("greedy")                   # the greedy choice is not the in-order one
    i = at["greedy"]
    in_order = lc.in_order_match(ch["att"][:, i], n, ch["gt_positions"][i], ch["gt_boxes"][i], c, case["canvas_size"])
    assert in_order == {0: 0} and match[:2] == [-1, 0] and m[1][0] > m[0][0] > 0
    c, n, match, ious, m, _ = scored("outside")
    assert (c, n) == (1, 1) and m == [[0.0]] and match[0] == -1


def test_the_random_tables_are_not_trivial():
    """matched, unmatched, hits, misses, clamped counts and a second group in the sums"""
    for name, case in lc.gpu_cases().items():
        _, counts, sums = lc.expected(name)
        assert counts[lc.IMAGES] == sum(ch["k"] for ch in case["chunks"])
        assert counts[lc.COUNTS:].sum() == counts[lc.IMAGES]
        if counts[lc.IMAGES] >= 5:
            assert 0 < counts[lc.HITS] < counts[lc.MATCHED] < min(counts[lc.PRESENT], counts[lc.INFERRED]), name
            assert counts[lc.COUNT_CORRECT] < counts[lc.IMAGES] and (counts[lc.COUNT_CORRECT] > 0 or counts[lc.IMAGES] < 32)
            assert 0 < sums[lc.IOU] < sums[lc.COVER] and sums[lc.DIST] > 0
    big = lc.gpu_cases()["t3_g2_k257_b260"]["chunks"][0]
    assert big["k"] == lc.GROUP + 1 and lc.clamp(big["gt_count"][256], 2) > 0    # the image of the second group counts
    out, _, _ = lc.expected("t3_g2_k257_b260")
    assert out[0][0][256].max() >= 0
    full = lc.gpu_cases()["t16_g16_k7_b7"]["chunks"][0]
    assert max(lc.clamp(v, 16) for v in full["run_digits"]) == 16 and full["gt_count"].max() == 16
    # the same inputs, the same bits: the restatement is a function
    case = lc.gpu_cases()["two_chunks"]
    counts, sums = lc.empty_accumulators(case)
    for chk in case["chunks"]:
        lc.apply_chunk(case, chk, counts, sums)
    _, want_c, want_s = lc.expected("two_chunks")
    assert counts.tobytes() == want_c.tobytes() and sums.tobytes() == want_s.tobytes()
