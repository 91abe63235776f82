"""The segmentation metrics of include/air_hip.h (air_scene_masks, air_segmentation) restated in numpy, and the case tables of
their tests.

Labels are computed in FLOAT32 in the header's order -- the taps of theta_recon, the reference's four-product expression,
z_pres times it -- so a label is a comparison of the very numbers the kernel compares; the table is integer; FG-ARI and the
mask IoU are python integers (exact) and float64 operations in the stated order; the sums use the stated tree.  Everything
the kernel leaves is therefore compared bit for bit (tests/test_gpu_segmentation.py).  Inputs are built from seeds, not from
a model; what the tables claim to contain is asserted by tests/test_segmentation_cases.py."""
import functools

import numpy as np

MAX_STEPS = MAX_DIGITS = 16
MAX_CANVAS, MAX_WINDOW, GROUP = 128, 32, 256
IMAGES, SCORED, PRESENT, FG_PIXELS, FG_MISSED, BG_CLAIMED, COUNTS = 0, 1, 2, 3, 4, 5, 6
ARI, MASK_IOU, SUMS = 0, 1, 2
WORKSPACE_BYTES_PER_IMAGE = 8 * (SUMS + COUNTS - 1)      # the two values and the five integer totals of an image
ATT_S, ATT_X, ATT_Y, ATT_Z, ATT_MASK, ATT_STRIDE = 0, 1, 2, 4, 11, 16
NAMES = ("fg_ari", "mask_iou", "fg_missed", "bg_claimed")
f32 = np.float32


# ---- the restatement --------------------------------------------------------------------------------------------------
def axis_taps(n_out, n_in, a, b):
    """axis_tap of csrc/air_sampler_common.h for every output coordinate of one axis, float32 -> (w0, w1, i0, i1)"""
    j = np.arange(n_out, dtype=f32)
    step = f32(2.0) / f32(n_out - 1)
    t = f32(-1.0) + step * j
    xs = a * t + b
    X = ((xs + f32(1.0)) * (f32(n_in) - f32(1.001))) / f32(2.0)
    f0 = np.floor(X)
    lim = f32(n_in - 1)
    c0 = np.fmin(np.fmax(f0, f32(0.0)), lim)                 # fminf / fmaxf: a NaN gives the other operand
    c1 = np.fmin(np.fmax(f0 + f32(1.0), f32(0.0)), lim)
    assert all(v.dtype == f32 for v in (t, xs, X, c0, c1))
    return c1 - X, X - c0, c0.astype(np.int64), c1.astype(np.int64)


def step_terms(att, vrec, i, C, w):
    """c_t [T, C, C] float32 of image i (NaN-free only where the inputs are) and the active flags [T]"""
    T = att.shape[0]
    terms, active = np.zeros((T, C, C), f32), np.zeros(T, bool)
    with np.errstate(all="ignore"):
        for t in range(T):
            rec = att[t, i]
            active[t] = bool(rec[ATT_MASK] != 0)
            s, x, y, z = (f32(rec[c]) for c in (ATT_S, ATT_X, ATT_Y, ATT_Z))
            ia, bx, by = f32(1.0) / s, (-x) / s, (-y) / s
            xw0, xw1, xi0, xi1 = axis_taps(C, w, ia, bx)        # over the canvas columns
            yw0, yw1, yi0, yi1 = axis_taps(C, w, ia, by)        # over the canvas rows
            win = vrec[t, i].reshape(w, w)
            Ia, Ib = win[yi0[:, None], xi0[None, :]], win[yi1[:, None], xi0[None, :]]
            Ic, Id = win[yi0[:, None], xi1[None, :]], win[yi1[:, None], xi1[None, :]]
            wa, wb = xw0[None, :] * yw0[:, None], xw0[None, :] * yw1[:, None]
            wc, wd = xw1[None, :] * yw0[:, None], xw1[None, :] * yw1[:, None]
            wr = ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id
            terms[t] = z * wr
            assert terms[t].dtype == f32 and wr.dtype == f32
    return terms, active


def predicted_labels(att, vrec, i, C, w, thr):
    """uint8 [C * C]: the first active step whose term is above thr and above every earlier one, + 1; 0: none"""
    terms, active = step_terms(att, vrec, i, C, w)
    best = np.full((C, C), f32(thr), f32)
    label = np.zeros((C, C), np.uint8)
    with np.errstate(invalid="ignore"):
        for t in range(att.shape[0]):
            if not active[t]:
                continue
            take = terms[t] > best                                   # a NaN never takes the pixel
            best = np.where(take, terms[t], best)
            label = np.where(take, np.uint8(t + 1), label)
    return label.reshape(-1)


def table_of(truth, pred, G, T):
    """int32 [G + 1, T + 1]: truth x prediction over the pixels; a truth label > G counts as 0"""
    truth = np.where(truth > G, 0, truth).astype(np.int64)
    return np.bincount(truth * (T + 1) + pred.astype(np.int64), minlength=(G + 1) * (T + 1)).astype(np.int32).reshape(G + 1, T + 1)


def scores_from_table(n):
    """-> (scored, ari float64 (NaN when unscored), mask_iou float64 [G], dict of the integer totals)"""
    n = [[int(v) for v in r] for r in np.asarray(n)]
    G, T = len(n) - 1, len(n[0]) - 1
    a = [sum(r) for r in n]
    b = [sum(n[r][c] for r in range(1, G + 1)) for c in range(T + 1)]
    colsum = [sum(n[r][c] for r in range(G + 1)) for c in range(T + 1)]
    N = sum(a[1:])
    S = sum(v * (v - 1) // 2 for r in range(1, G + 1) for v in n[r])
    A = sum(v * (v - 1) // 2 for v in a[1:])
    Bs = sum(v * (v - 1) // 2 for v in b)
    scored = N >= 2
    ari = np.float64("nan")
    if scored:
        P = N * (N - 1) // 2
        E = np.float64(A) * np.float64(Bs) / np.float64(P)
        M = (np.float64(A) + np.float64(Bs)) / np.float64(2.0)
        ari = np.float64(1.0) if M == E else (np.float64(S) - E) / (M - E)
    iou = np.zeros(G, np.float64)
    for r in range(1, G + 1):
        if a[r] > 0:
            v = np.float64(0.0)
            for c in range(1, T + 1):
                q = np.float64(n[r][c]) / np.float64(a[r] + colsum[c] - n[r][c])
                if q > v:
                    v = q
            iou[r - 1] = v
    totals = dict(present=sum(1 for v in a[1:] if v > 0), fg=N, missed=sum(n[r][0] for r in range(1, G + 1)),
                  claimed=sum(n[0][1:]))
    return scored, ari, iou, totals


def group_tree(values):
    """the adjacent pairwise tree over GROUP float64 values: v[m] = v[2 m] + v[2 m + 1], eight times"""
    v = np.asarray(values, np.float64)
    assert v.shape == (GROUP,)
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def batch_total(per_image):
    """(((+0.0 + group 0) + group 1) + ...) of the per-image values, +0.0 for an image beyond the last"""
    k = len(per_image)
    padded = np.zeros(-(-k // GROUP) * GROUP, np.float64)
    padded[:k] = per_image
    total = np.float64(0.0)
    for g in range(0, len(padded), GROUP):
        total = total + group_tree(padded[g:g + GROUP])
    return total


def empty_accumulators():
    return np.zeros(COUNTS, np.int64), np.zeros(SUMS, np.float64)


def apply_chunk(case, chunk, counts, sums):
    """one air_segmentation call: adds to counts / sums in place -> (pred_mask [k, C C] uint8, tables [k, G + 1, T + 1] int32,
    ari [k] float64, mask_iou [k, G] float64)"""
    T, G, C, w, k = case["T"], case["G"], case["C"], case["w"], chunk["k"]
    pred = np.zeros((k, C * C), np.uint8)
    tables = np.zeros((k, G + 1, T + 1), np.int32)
    ari, iou = np.zeros(k, np.float64), np.zeros((k, G), np.float64)
    v_ari, v_iou = np.zeros(k, np.float64), np.zeros(k, np.float64)
    for i in range(k):
        pred[i] = predicted_labels(chunk["att"], chunk["vrec"], i, C, w, case["thr"])
        tables[i] = table_of(chunk["gt_mask"][i], pred[i], G, T)
        scored, ari[i], iou[i], tot = scores_from_table(tables[i])
        v_ari[i] = ari[i] if scored else 0.0
        p = np.float64(0.0)
        for r in range(G):
            if tables[i][r + 1].sum() > 0:
                p = p + iou[i][r]
        v_iou[i] = p
        counts[IMAGES] += 1
        counts[SCORED] += int(scored)
        counts[PRESENT] += tot["present"]
        counts[FG_PIXELS] += tot["fg"]
        counts[FG_MISSED] += tot["missed"]
        counts[BG_CLAIMED] += tot["claimed"]
    sums[ARI] = sums[ARI] + batch_total(v_ari)
    sums[MASK_IOU] = sums[MASK_IOU] + batch_total(v_iou)
    return pred, tables, ari, iou


def derived(counts, sums, C):
    """the four numbers of NAMES, float64; a zero denominator gives NaN"""
    num = np.asarray([sums[ARI], sums[MASK_IOU], counts[FG_MISSED], counts[BG_CLAIMED]], np.float64)
    den = np.asarray([counts[SCORED], counts[PRESENT], counts[FG_PIXELS], counts[IMAGES] * (C * C) - counts[FG_PIXELS]], np.float64)
    with np.errstate(all="ignore"):
        return np.where(den == 0, np.float64("nan"), num / den)


def scene_masks(glyphs, crops, digits, indices, positions, C, ink_threshold=0.0):
    """air_scene_masks: uint8 [B, C * C]; glyphs [Gn, gd gd] float32, crops [Gn, 4], digits [B], indices [B, md],
    positions [B, 2 md]"""
    Gn, gd = glyphs.shape[0], int(round(glyphs.shape[1] ** 0.5))
    B, md = len(digits), indices.shape[1]
    mask = np.zeros((B, C, C), np.uint8)
    for b in range(B):
        for g in reversed(range(min(max(int(digits[b]), 0), md))):           # the smallest g is painted last: it wins
            idx = int(indices[b, g])
            if not 0 <= idx < Gn:
                continue
            x0, y0, w, h = (int(v) for v in crops[idx])
            if x0 < 0 or y0 < 0 or w < 0 or h < 0 or x0 + w > gd or y0 + h > gd:
                continue
            xg, yg = int(positions[b, 2 * g]), int(positions[b, 2 * g + 1])
            plane = glyphs[idx].reshape(gd, gd)
            for dy in range(h):
                for dx in range(w):
                    px, py = xg + dx, yg + dy
                    if 0 <= px < C and 0 <= py < C and plane[y0 + dy, x0 + dx] > f32(ink_threshold):
                        mask[b, py, px] = g + 1
    return mask.reshape(B, C * C)


# ---- the cases --------------------------------------------------------------------------------------------------------
# (T, G, k, B, C, w): one image; several, k < B; C * C no multiple of 16 (the byte-store path); the limits of T and G; the
# largest canvas and window (the LDS grant); one image beyond a group (a second group in the tree, the byte path again)
SHAPES = [(1, 1, 1, 1, 8, 4), (2, 2, 3, 4, 16, 8), (3, 2, 5, 8, 15, 7), (16, 16, 2, 2, 12, 6), (5, 4, 2, 2, 128, 32),
          (3, 2, 257, 260, 10, 4)]
READS = (ATT_S, ATT_X, ATT_Y, ATT_Z, ATT_MASK)


def shape_name(s):
    return "t%d_g%d_k%d_b%d_c%d_w%d" % s


def random_gt(rng, k, G, C, beyond=True):
    """label planes: up to G rectangles per image, later ones over earlier ones, some images empty; a few pixels carry a
    label > G (which counts as background)"""
    gt = np.zeros((k, C, C), np.uint8)
    for i in range(k):
        for g in range(rng.randint(0, G + 1)):
            x, y = rng.randint(0, C - 1, 2)
            ww, hh = rng.randint(1, max(2, C // 2), 2)
            gt[i, y:y + hh, x:x + ww] = rng.randint(1, G + 1)
        if beyond and G < 255:
            gt[i, rng.randint(0, C), rng.randint(0, C)] = rng.randint(G + 1, 256)
    return gt.reshape(k, C * C)


def random_chunk(rng, T, B, k, G, C, w):
    """records with overlapping windows (scale 0.3 .. 0.9 of the canvas, centres within +-0.6), z_pres 1 with a few 0, the
    last steps of some images inactive; NaN in every slot and every row (>= k) the kernel has no business with"""
    att = np.full((T, B, ATT_STRIDE), np.nan, f32)
    att[:, :k, ATT_S] = rng.uniform(0.3, 0.9, (T, k))
    att[:, :k, ATT_X] = rng.uniform(-0.6, 0.6, (T, k))
    att[:, :k, ATT_Y] = rng.uniform(-0.6, 0.6, (T, k))
    att[:, :k, ATT_Z] = (rng.uniform(0, 1, (T, k)) < 0.9).astype(f32)
    steps = rng.randint(0, T + 1, k)
    att[:, :k, ATT_MASK] = (np.arange(T)[:, None] < np.maximum(steps, 1)[None, :]).astype(f32)
    vrec = np.full((T, B, w * w), np.nan, f32)
    vrec[:, :k] = rng.uniform(0.0, 1.0, (T, k, w * w))
    return dict(k=k, att=att, vrec=vrec, gt_mask=random_gt(rng, k, G, C))


def branches_case():
    """(T, G, C, w) = (4, 3, 16, 8), eight images, each planted with what its name says (thr = 0.5)"""
    T, G, C, w, B = 4, 3, 16, 8, 8
    rng = np.random.RandomState(77)
    ch = random_chunk(rng, T, B, B, G, C, w)
    att, vrec = ch["att"], ch["vrec"]
    att[:, :, ATT_Z], att[:, :, ATT_MASK] = 1.0, 1.0
    planted = dict(overlap=0, off_canvas=1, inactive_between=2, tie=3, nan_window=4, z_zero=5, at_threshold=6, unscored=7)
    # 0: two large windows over the same part of the canvas
    att[0, 0, [ATT_S, ATT_X, ATT_Y]] = 0.7, -0.1, 0.0
    att[1, 0, [ATT_S, ATT_X, ATT_Y]] = 0.7, 0.1, 0.1
    # 1: a window that lies partly off the canvas (centre 0.9, half-width 0.5)
    att[0, 1, [ATT_S, ATT_X, ATT_Y]] = 0.5, 0.9, -0.9
    # 2: step 1 inactive between active ones (compose skips it; steps 0, 2, 3 run)
    att[1, 2, ATT_MASK] = 0.0
    vrec[1, 2] = 0.99                                                         # would take nearly every pixel it covers
    # 3: steps 1 and 2 have identical records and windows: an exact tie wherever either is the best
    att[2, 3], vrec[2, 3] = att[1, 3], vrec[1, 3]
    vrec[1, 3] = vrec[2, 3] = np.maximum(vrec[1, 3], f32(0.8))
    vrec[0, 3] = np.minimum(vrec[0, 3], f32(0.3))
    vrec[3, 3] = np.minimum(vrec[3, 3], f32(0.3))
    # 4: NaN values in a window
    vrec[0, 4, ::5] = np.nan
    # 5: z_pres = 0 on every step (nothing is claimed) under a single-label truth: A = Bs = P, the M == E branch
    att[:, 5, ATT_Z] = 0.0
    # 6: step 0 maps the canvas onto the whole window (s = 1, x = y = 0): canvas pixel (0, 0) reads window element (0, 0)
    # with weight exactly 1, and that element is the threshold
    att[0, 6, [ATT_S, ATT_X, ATT_Y]] = 1.0, 0.0, 0.0
    att[1:, 6, ATT_MASK] = 0.0
    vrec[0, 6, 0] = 0.5
    gt = random_gt(rng, B, G, C).reshape(B, C, C)
    gt[5] = 0
    gt[5, 3:9, 2:7] = 2
    gt[6, 0, 0] = 1
    gt[7] = 0                                                                 # 7: no foreground at all: unscored
    gt[7, 4, 4] = 200                                                         # (a label > G is background)
    ch["gt_mask"] = gt.reshape(B, C * C)
    return dict(T=T, G=G, B=B, C=C, w=w, thr=0.5, chunks=[ch], planted=planted)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    cases = {}
    for n, (T, G, k, B, C, w) in enumerate(SHAPES):
        rng = np.random.RandomState(100 + n)
        cases[shape_name(SHAPES[n])] = dict(T=T, G=G, B=B, C=C, w=w, thr=0.5, chunks=[random_chunk(rng, T, B, k, G, C, w)])
    cases["branches"] = branches_case()
    rng = np.random.RandomState(9)
    cases["two_chunks"] = dict(T=3, G=2, B=6, C=12, w=5, thr=0.25,
                               chunks=[random_chunk(rng, 3, 6, 5, 2, 12, 5), random_chunk(rng, 3, 6, 3, 2, 12, 5)])
    return cases


@functools.lru_cache(maxsize=None)
def expected(name, upto=None):
    """([(pred_mask, tables, ari, mask_iou)] per chunk, counts, sums) of a case -- computed once per process, read-only"""
    case = gpu_cases()[name]
    counts, sums = empty_accumulators()
    outs = [apply_chunk(case, ch, counts, sums) for ch in case["chunks"][:upto]]
    return outs, counts, sums


def hand_scene():
    """three glyphs placed by hand on a 12 x 12 canvas: the boxes of digits 0 and 1 intersect and their inks are disjoint
    (two interleaved combs); digit 2 lies over the ink of digit 0 (the smaller g must win); a fourth slot is past
    digits[b].  Scene 1 has an index outside the table and a crop that leaves its frame: both label nothing."""
    gd, C = 6, 12
    glyphs = np.zeros((4, gd, gd), f32)
    glyphs[0, 1:5, 0:6:2] = 1.0                    # comb on the even columns
    glyphs[1, 1:5, 1:6:2] = 0.75                   # comb on the odd columns
    glyphs[2, 0:6, 0:6] = 0.5                      # a full block
    glyphs[3, 2:4, 2:4] = 0.2
    crops = np.asarray([[0, 1, 5, 4], [1, 1, 5, 4], [0, 0, 6, 6], [2, 2, 5, 2]], np.int32)     # the last leaves the frame
    digits = np.asarray([3, 3], np.int32)
    indices = np.asarray([[0, 1, 2, 3], [7, 3, 1, 0]], np.int32)
    positions = np.asarray([[2, 2, 3, 2, 1, 1, 0, 0], [0, 0, 1, 1, 4, 5, 0, 0]], np.int32)
    return dict(glyphs=glyphs.reshape(4, gd * gd), crops=crops, digits=digits, indices=indices, positions=positions, C=C, gd=gd)
