"""The localisation metrics restated in plain Python float64 (the "localisation metrics" section of include/air_hip.h:
inferred box, ground-truth box, IoU / cover / centre distance of a pair, the greedy match, the accumulators and their ONE
summation order, the derived numbers of air.metrics.Localization), and the builders of the cases
tests/test_localization_cases.py (CPU) and tests/test_gpu_localization.py (air_localization) share.  No torch, no GPU.

Every operation is a correctly rounded float64 add, subtract, multiply, divide, sqrt or comparison, written in the header's
order; Python's float is that type, so the kernel has to give the same BITS.

A case is a dict:
  T, B, G, canvas_size, tau
  chunks   a list of dicts, one per call of air_localization: k, att [T, B, 16] float32 (only the columns ATT_S = 0,
           ATT_X = 1 and ATT_Y = 2 matter), run_digits [B] int32 and the padded ground truth gt_count [k],
           gt_positions / gt_boxes [k, G, 2] int32
  planted  {name: image index in the first chunk} of the hand-built images, when the case has them
Batch rows >= k of a chunk hold junk (NaN records, run_digits > 0): they must not count."""
import functools
import math

import numpy as np

ATT_STRIDE, ATT_S, ATT_X, ATT_Y = 16, 0, 1, 2
MAX_STEPS = MAX_DIGITS = 16
GROUP = 256                                  # AIR_LOC_GROUP: images per group of the summation order
IMAGES, PRESENT, INFERRED, MATCHED, HITS, COUNT_CORRECT, COUNTS = range(7)
IOU, COVER, DIST, SUMS = range(4)
NAMES = ("mean_iou", "recall", "precision", "cover", "center_dist", "count_accuracy")


# ------------------------------------------------------------------------------------------------------ one pair, one image
def clip(v, C):
    return 0.0 if v < 0.0 else (C if v > C else v)             # a NaN fails both comparisons and passes through


def fmin(a, b):
    return a if a < b else b


def fmax(a, b):
    return a if a > b else b


def inferred_box(s, x, y, canvas_size):
    """(l1, r1, t1, b1) of one record; s, x, y are the float32 values widened"""
    C = float(canvas_size)
    q = (C - 1.001) / 2.0
    s, x, y = float(s), float(x), float(y)
    return (clip((x - s + 1.0) * q, C), clip((x + s + 1.0) * q + 1.0, C),
            clip((y - s + 1.0) * q, C), clip((y + s + 1.0) * q + 1.0, C))


def gt_box(x, y, w, h):
    x, y, w, h = float(int(x)), float(int(y)), float(int(w)), float(int(h))
    return (x, x + w, y, y + h), w * h


def pair(obox, x, y, w, h):
    """-> (iou, cover) of an inferred box and the ground-truth digit (x, y, w, h)"""
    (l2, r2, t2, b2), a_gt = gt_box(x, y, w, h)
    l1, r1, t1, b1 = obox
    iw = fmin(r1, r2) - fmax(l1, l2)
    ih = fmin(b1, b2) - fmax(t1, t2)
    if iw > 0.0 and ih > 0.0:
        inter = iw * ih
        a_inf = (r1 - l1) * (b1 - t1)
        uni = a_inf + a_gt - inter
        if uni > 0.0:
            return inter / uni, inter / a_gt
    return 0.0, 0.0


def center_distance(xa, ya, x, y, w, h, canvas_size):
    """embeddings.py:39-44, 113-114 with (canvas_size - 1) / 2 for 24.5"""
    half = (float(canvas_size) - 1.0) / 2.0
    cx = (float(int(x) + int(x) + int(w)) - 1.0) / 2.0
    cy = (float(int(y) + int(y) + int(h)) - 1.0) / 2.0
    x1, y1 = cx / half - 1.0, cy / half - 1.0
    dx, dy = float(xa) - x1, float(ya) - y1
    return math.sqrt(dx * dx + dy * dy)


def iou_matrix(rec, n, pos, box, c, canvas_size):
    """[c][n] IoU of every (digit, object) pair of one image; rec [T, 16], pos / box [G, 2]"""
    return [[pair(inferred_box(rec[t][ATT_S], rec[t][ATT_X], rec[t][ATT_Y], canvas_size), pos[g][0], pos[g][1], box[g][0],
                  box[g][1])[0] for t in range(n)] for g in range(c)]


def match_image(rec, n, pos, box, c, canvas_size):
    """the greedy match -> {g: t} (insertion order = round order)"""
    used_g, used_t, taken = set(), set(), {}
    for _ in range(min(n, c)):
        best, bg, bt = 0.0, -1, -1
        for g in range(c):
            if g in used_g:
                continue
            for t in range(n):
                if t in used_t:
                    continue
                obox = inferred_box(rec[t][ATT_S], rec[t][ATT_X], rec[t][ATT_Y], canvas_size)
                v = pair(obox, pos[g][0], pos[g][1], box[g][0], box[g][1])[0]
                if v > best:
                    best, bg, bt = v, g, t
        if bg < 0:
            break
        used_g.add(bg)
        used_t.add(bt)
        taken[bg] = bt
    return taken


def in_order_match(rec, n, pos, box, c, canvas_size):
    """what the greedy match is NOT: every digit in order takes its best unused object"""
    used_t, taken = set(), {}
    m = iou_matrix(rec, n, pos, box, c, canvas_size)
    for g in range(c):
        best, bt = 0.0, -1
        for t in range(n):
            if t not in used_t and m[g][t] > best:
                best, bt = m[g][t], t
        if bt >= 0:
            used_t.add(bt)
            taken[g] = bt
    return taken


def clamp(v, hi):
    return min(max(int(v), 0), hi)


def score_image(case, chunk, i):
    """-> (c, n, match [G], iou [G], (p_iou, p_cover, p_dist), hits) of image i of a chunk; p_*: step 1 of the order"""
    T, G, C = case["T"], case["G"], case["canvas_size"]
    c, n = clamp(chunk["gt_count"][i], G), clamp(chunk["run_digits"][i], T)
    rec, pos, box = chunk["att"][:, i], chunk["gt_positions"][i], chunk["gt_boxes"][i]
    taken = match_image(rec, n, pos, box, c, C)
    match, ious = [-1] * G, [0.0] * G
    p, hits = [0.0, 0.0, 0.0], 0
    for g in range(c):                                          # digits in order, an unmatched one skipped
        if g not in taken:
            continue
        t = taken[g]
        obox = inferred_box(rec[t][ATT_S], rec[t][ATT_X], rec[t][ATT_Y], C)
        v, cover = pair(obox, pos[g][0], pos[g][1], box[g][0], box[g][1])
        dist = center_distance(rec[t][ATT_X], rec[t][ATT_Y], pos[g][0], pos[g][1], box[g][0], box[g][1], C)
        match[g], ious[g] = t, v
        p[IOU] = p[IOU] + v
        p[COVER] = p[COVER] + cover
        p[DIST] = p[DIST] + dist
        hits += 1 if v >= case["tau"] else 0
    return c, n, match, ious, p, hits


# ------------------------------------------------------------------------------------------------------- the accumulators
def group_tree(values):
    """step 2: GROUP values folded by the adjacent pairwise tree"""
    v = list(values)
    assert len(v) == GROUP
    while len(v) > 1:
        v = [v[2 * m] + v[2 * m + 1] for m in range(len(v) // 2)]
    return v[0]


def empty_accumulators(case):
    return (np.zeros(COUNTS + (case["G"] + 1) * (case["T"] + 1), np.int64), np.zeros(SUMS, np.float64))


def apply_chunk(case, chunk, counts, sums):
    """one call of air_localization: adds to counts / sums in place -> (match [k, G] int32, iou [k, G] float64)"""
    T, G, k = case["T"], case["G"], chunk["k"]
    match, ious = np.full((k, G), -1, np.int32), np.zeros((k, G), np.float64)
    per_image = [[0.0] * (-(-k // GROUP) * GROUP) for _ in range(SUMS)]
    counts[IMAGES] += k
    for i in range(k):
        c, n, m, v, p, hits = score_image(case, chunk, i)
        match[i], ious[i] = m, v
        for j in range(SUMS):
            per_image[j][i] = p[j]
        counts[PRESENT] += c
        counts[INFERRED] += n
        counts[MATCHED] += sum(1 for t in m if t >= 0)
        counts[HITS] += hits
        counts[COUNT_CORRECT] += 1 if c == n else 0
        counts[COUNTS + c * (T + 1) + n] += 1
    for j in range(SUMS):
        total = 0.0                                             # step 3: the groups in order
        for g0 in range(0, len(per_image[j]), GROUP):
            total = total + group_tree(per_image[j][g0:g0 + GROUP])
        sums[j] = float(sums[j]) + total                        # step 4: the incoming value + the batch total
    return match, ious


@functools.lru_cache(maxsize=None)
def _expected(name, upto):
    case = gpu_cases()[name]
    counts, sums = empty_accumulators(case)
    out = [apply_chunk(case, ch, counts, sums) for ch in case["chunks"][:upto]]
    return out, counts, sums


def expected(name, upto=None):
    """the case through the restatement, chunk after chunk -> ([(match, iou)], counts, sums); computed once, do not modify"""
    return _expected(name, len(gpu_cases()[name]["chunks"]) if upto is None else upto)


def confusion(case, counts):
    return np.asarray(counts[COUNTS:]).reshape(case["G"] + 1, case["T"] + 1)


def derived(counts, sums):
    """Localization.values(): NAMES in order, NaN for a zero denominator"""
    def div(a, b):
        return float("nan") if b == 0 else float(a) / float(b)
    return np.asarray([div(sums[IOU], counts[PRESENT]), div(counts[HITS], counts[PRESENT]), div(counts[HITS], counts[INFERRED]),
                       div(sums[COVER], counts[PRESENT]), div(sums[DIST], counts[MATCHED]),
                       div(counts[COUNT_CORRECT], counts[IMAGES])], np.float64)


# ------------------------------------------------------------------------------------------------------------ case builders
def record_for_box(left, top, side, canvas_size=50):
    """(s, x, y) as float32 whose window spans [left, left + side) x [top, top + side): the header's edges solved for the
    record, l1 = (x - s + 1) q and r1 - 1 = (x + s + 1) q, then rounded to float32"""
    q = (canvas_size - 1.001) / 2.0
    s = (side - 1.0) / (2.0 * q)
    x = (2.0 * left + side - 1.0) / (2.0 * q) - 1.0
    y = (2.0 * top + side - 1.0) / (2.0 * q) - 1.0
    return np.float32(s), np.float32(x), np.float32(y)


NAN = float("nan")
# name -> (ground truth [(x, y, w, h)], records [(s, x, y)], run_digits); canvas 50, T = 4, G = 3
PLANTED = {
    "tie_objects": ([(10, 10, 20, 20)], [record_for_box(12, 12, 20)] * 2, 2),            # equal IoU: the smaller t
    "tie_digits": ([(10, 10, 20, 20)] * 2, [record_for_box(11, 11, 20)], 1),              # equal IoU: the smaller g
    "unmatched_digit": ([(2, 2, 14, 14), (30, 30, 14, 14)], [record_for_box(2, 2, 14)], 1),
    "unmatched_object": ([(2, 2, 14, 14)], [record_for_box(2, 2, 14), record_for_box(30, 30, 14)], 2),
    "no_digits": ([], [record_for_box(5, 5, 20)], 1),
    "no_objects": ([(5, 5, 20, 20)], [], 0),
    "neither": ([], [], 0),
    "above_T": ([(5, 5, 20, 20), (28, 28, 15, 15)],
                [record_for_box(29, 28, 15), record_for_box(40, 2, 8), record_for_box(1, 40, 8), record_for_box(6, 5, 20)], 9),
    "below_zero": ([(5, 5, 20, 20)], [record_for_box(5, 5, 20)], -3),
    "nan": ([(5, 5, 20, 20), (28, 28, 15, 15)],
            [(NAN,) + tuple(record_for_box(5, 5, 20)[1:]), (record_for_box(5, 5, 20)[0], NAN, record_for_box(5, 5, 20)[2]),
             record_for_box(28, 28, 15)], 3),
    # the window covers the whole canvas after the clip (exact edges 0 and 50); the digit is half of it: IoU = 1250 / 2500
    "at_tau": ([(0, 0, 25, 50)], [(2.0, 0.0, 0.0)], 1),
    # digit 1 has the best pair (object 0, 380 / 420); in order, digit 0 would take object 0 (300 / 500) first
    "greedy": ([(10, 10, 20, 20), (14, 10, 20, 20)], [record_for_box(15, 10, 20), record_for_box(40, 40, 8)], 2),
    "outside": ([(30, 10, 20, 20)], [(0.2, 3.0, 0.0)], 1),                                # clipped to area 0
}


def _random_image(rng, T, G, C, full=False):
    """-> gt [(x, y, w, h)] (c of them), records [(s, x, y)] (T of them), run_digits; full: c = G and run_digits = T"""
    c = G if full else int(rng.randint(0, G + 1))
    gt = []
    for _ in range(c):
        w, h = int(rng.randint(6, 29)), int(rng.randint(6, 29))
        gt.append((int(rng.randint(0, C - w + 1)), int(rng.randint(0, C - h + 1)), w, h))
    recs = []
    for _ in range(T):
        u = rng.rand()
        if gt and u < 0.65:                                     # a digit's box, moved and resized a little
            x, y, w, h = gt[int(rng.randint(len(gt)))]
            side = max(w, h) * rng.uniform(0.8, 1.3)
            recs.append(record_for_box(x + rng.uniform(-4, 4), y + rng.uniform(-4, 4), side, C))
        elif recs and u < 0.75:                                 # a copy of an earlier object: exact ties
            recs.append(recs[int(rng.randint(len(recs)))])
        else:
            recs.append((np.float32(rng.uniform(0.1, 0.9)), np.float32(rng.uniform(-1.2, 1.2)), np.float32(rng.uniform(-1.2, 1.2))))
    n = int(rng.randint(0, T + 1))
    if rng.rand() < 0.1:
        n = int(rng.choice([-2, T + 1, T + 5]))
    return gt, recs, T if full else n


def build_chunk(rng, k, T, B, G, C, planted=None):
    """planted: {image index: name of PLANTED}"""
    att = rng.uniform(-1.0, 1.0, (T, B, ATT_STRIDE)).astype(np.float32)
    run = rng.randint(0, T + 1, B).astype(np.int32)
    att[:, k:] = np.float32(NAN)                                # rows >= k: junk that would poison every sum
    run[k:] = T
    gt_count = np.zeros(k, np.int32)
    gt_positions = rng.randint(0, C, (k, G, 2)).astype(np.int32)   # slots behind gt_count hold junk boxes
    gt_boxes = rng.randint(1, C, (k, G, 2)).astype(np.int32)
    for i in range(k):
        # (image 0 of every chunk has all G digits and all T objects: the longest scan the shape allows)
        gt, recs, n = PLANTED[planted[i]] if planted and i in planted else _random_image(rng, T, G, C, full=i == 0)
        assert len(gt) <= G and len(recs) <= T
        gt_count[i], run[i] = len(gt), n
        for g, (x, y, w, h) in enumerate(gt):
            gt_positions[i, g], gt_boxes[i, g] = (x, y), (w, h)
        for t, r in enumerate(recs):
            att[t, i, ATT_S], att[t, i, ATT_X], att[t, i, ATT_Y] = r
    return dict(k=k, att=att, run_digits=run, gt_count=gt_count, gt_positions=gt_positions, gt_boxes=gt_boxes)


def random_case(seed, chunk_sizes, T, B, G, canvas_size=50, tau=0.5, planted=None):
    rng = np.random.RandomState(seed)
    return dict(T=T, B=B, G=G, canvas_size=canvas_size, tau=tau,
                chunks=[build_chunk(rng, k, T, B, G, canvas_size, planted) for k in chunk_sizes])


def branch_case():
    """(T, G, k, B) = (4, 3, 32, 32): every PLANTED image at a shuffled index, random images between them"""
    rng = np.random.RandomState(77)
    T, G, k, B, C = 4, 3, 32, 32, 50
    where = rng.permutation(k)[:len(PLANTED)]
    planted = {int(i): name for i, name in zip(where, sorted(PLANTED))}
    case = dict(T=T, B=B, G=G, canvas_size=C, tau=0.5, chunks=[build_chunk(rng, k, T, B, G, C, planted)])
    case["planted"] = {name: i for i, name in planted.items()}
    return case


# (T, G, k, B) of the single-chunk shapes; 257 crosses the group (= workgroup) size by one image
SHAPES = ((1, 1, 1, 1), (3, 2, 5, 8), (16, 16, 7, 7), (3, 2, 64, 64), (3, 2, 65, 70), (3, 2, GROUP + 1, GROUP + 4))


@functools.lru_cache(maxsize=None)
def gpu_cases():
    # (the one image of the second group is a planted one: it has a matched pair, so the group's partial is not zero)
    cases = {"t%d_g%d_k%d_b%d" % s: random_case(100 + n, (s[2],), s[0], s[3], s[1],
                                                planted={GROUP: "unmatched_object"} if s[2] > GROUP else None)
             for n, s in enumerate(SHAPES)}
    cases["branches"] = branch_case()
    cases["two_chunks"] = random_case(200, (5, 3), 3, 8, 2)     # accumulation: k1 + k2 rows in two calls
    return cases
