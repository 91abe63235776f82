"""The projector export restated in plain Python and numpy float64 (embeddings.py:29-131 of the reference: ground-truth
centres, match, compaction in (image, digit) order, sprite sheet and matplotlib's grey levels), and the builders of the cases
tests/test_embedding_cases.py (CPU) and tests/test_gpu_embeddings.py (air_embed_collect / air_embed_sprites) share.  No
torch, no GPU.

A synthetic case is a dict:
  T, B, G, Z, w, canvas_size, max_distance
  chunks   a list of dicts, one per call of air_embed_collect: k, att [T, B, 16] float32 (only the columns ATT_X = 1 and
           ATT_Y = 2 matter), run_digits [B] int32, ml [T, B, 2 Z], vrec [T, B, w w] float32 and the padded ground truth
           gt_count [k], gt_positions / gt_boxes [k, G, 2], gt_labels / gt_ids [k, G] int32
  planted  {name: global image index} of the hand-worked images, when asked for
Batch rows >= k of a chunk hold junk with run_digits > 0: they must not count."""
import math

import numpy as np

ATT_STRIDE, ATT_X, ATT_Y = 16, 1, 2
FIVE_32 = 5.0 / 32.0                        # the planted tie: (3/32, 4/32) is at exactly 5/32 of the origin


def st_center(x, y, w, h, canvas_size=50):
    """embeddings.py:41-44 in float64; 24.5 = (canvas_size - 1) / 2 at 50"""
    half = (canvas_size - 1) / 2.0
    cx = (int(x) + int(x) + int(w) - 1.0) / 2.0
    cy = (int(y) + int(y) + int(h) - 1.0) / 2.0
    return cx / half - 1.0, cy / half - 1.0


def distance(x1, y1, x2, y2):
    return math.sqrt((x2 - x1) ** 2 + (y2 - y1) ** 2)


def candidate_distances(center, shifts):
    """float64 distances of one ground-truth centre to the (float32) shifts [n, 2] of the inferred objects"""
    return [distance(center[0], center[1], float(s[0]), float(s[1])) for s in shifts]


def match_image(centers, shifts, max_distance):
    """embeddings.py:90-108 for one image -> the matched object of every ground-truth digit, or -1"""
    taken, out = [], []
    for c in centers:
        closest, min_distance = -1, 3.0
        for k, dist in enumerate(candidate_distances(c, shifts)):
            if dist < min_distance:
                min_distance, closest = dist, k
        if closest >= 0 and min_distance <= max_distance and closest not in taken:
            taken.append(closest)
            out.append(closest)
        else:
            out.append(-1)
    return out


def collect_lists(digits, indices, positions, boxes, labels, rec_digits, rec_positions, rec_windows, rec_latents,
                  max_distance=0.2, canvas_size=50):
    """The reference's pipeline on the lists of read_test_data and of ModelWrapper.infer (rec_positions rows are (s, x, y))
    -> dict(ids, labels, latents, windows, present, inferred, matched)"""
    ids, labs, lats, wins = [], [], [], []
    for i in range(len(digits)):
        n = int(digits[i])
        centers = [st_center(positions[i][2 * j], positions[i][2 * j + 1], boxes[i][2 * j], boxes[i][2 * j + 1], canvas_size)
                   for j in range(n)]
        shifts = [rec_positions[i][k][1:] for k in range(int(rec_digits[i]))]
        for j, k in enumerate(match_image(centers, shifts, max_distance)):
            if k >= 0:
                ids.append(int(indices[i][j])); labs.append(int(labels[i][j]))
                lats.append(np.asarray(rec_latents[i][k], np.float32)); wins.append(np.asarray(rec_windows[i][k], np.float32))
    return dict(ids=np.asarray(ids, np.int32), labels=np.asarray(labs, np.int32),
                latents=np.stack(lats) if lats else np.zeros((0, 0), np.float32),
                windows=np.stack(wins) if wins else np.zeros((0, 0, 0), np.float32),
                present=int(sum(int(d) for d in digits)), inferred=int(sum(int(d) for d in rec_digits)), matched=len(ids))


# ---------------------------------------------------------------------------------------------------------------- sprites
def sprite_dim(m):
    return int(math.ceil(math.sqrt(m)))


def sprite_sheet_f64(windows):
    """embeddings.py:117-126: ones, tile i at column i % dim, row i // dim has window i subtracted"""
    windows = np.asarray(windows)
    m, w = windows.shape[0], windows.shape[1]
    dim = sprite_dim(m)
    sheet = np.ones((dim * w, dim * w))
    for i in range(m):
        x, y = i % dim, i // dim
        sheet[y * w:(y + 1) * w, x * w:(x + 1) * w] -= windows[i].reshape(w, w)
    return sheet


def grey_table():
    return (np.linspace(0.0, 1.0, 256) * 255).astype(np.uint8)


def sprite_levels(windows):
    """imsave(cmap='gray') of the sheet, as bytes"""
    sheet = sprite_sheet_f64(windows)
    lo, hi = sheet.min(), sheet.max()
    n = (sheet - lo) / (hi - lo) if hi > lo else np.zeros_like(sheet)
    return grey_table()[np.minimum((n * 256).astype(np.int64), 255)]


# ------------------------------------------------------------------------------------------------------- synthetic cases
PLANTED = ("tie", "shared", "no_objects", "no_digits", "too_far")


def _planted_image(name, T, G):
    """-> gt positions [(x, y)], boxes [(w, h)], inferred shifts [(x, y)] -- numbers exact in float64"""
    origin = ((11, 11), (28, 28))                                       # st_center = (0, 0) exactly
    if name == "tie":            # two objects at exactly 5/32: the first wins; accepted at max_distance = 5/32, not below
        return [origin[0]], [origin[1]], [(3 / 32, 4 / 32), (-3 / 32, -4 / 32)]
    if name == "shared":         # both digits are closest to object 0; the second is dropped although object 1 is in range
        return [origin[0], (12, 11)], [origin[1], (28, 28)], [(1 / 64, 0.0), (1 / 8, 0.0)]
    if name == "no_objects":
        return [origin[0]], [origin[1]], []
    if name == "no_digits":
        return [], [], [(0.0, 0.0), (0.25, 0.25)]
    if name == "too_far":
        return [origin[0]], [origin[1]], [(0.5, 0.5)]
    raise KeyError(name)


def synthetic_case(seed, chunk_sizes, T, B, G, Z, w, planted=False, max_distance=FIVE_32, canvas_size=50):
    rng = np.random.RandomState(seed)
    n = sum(chunk_sizes)
    slots = {}
    if planted:
        assert T >= 2 and G >= 2 and n >= len(PLANTED) + 2
        where = rng.permutation(n)[:len(PLANTED)]
        slots = {name: int(i) for name, i in zip(PLANTED, where)}
    by_index = {i: name for name, i in slots.items()}
    chunks, g0 = [], 0
    for k in chunk_sizes:
        assert 1 <= k <= B
        c = dict(k=k,
                 att=rng.uniform(-1.0, 1.0, (T, B, ATT_STRIDE)).astype(np.float32),
                 run_digits=rng.randint(0, T + 1, B).astype(np.int32),
                 ml=rng.standard_normal((T, B, 2 * Z)).astype(np.float32),
                 vrec=rng.uniform(0.0, 1.0, (T, B, w * w)).astype(np.float32),
                 gt_count=rng.randint(0, G + 1, k).astype(np.int32),
                 gt_positions=rng.randint(0, canvas_size - 27, (k, G, 2)).astype(np.int32),
                 gt_boxes=rng.randint(18, 29, (k, G, 2)).astype(np.int32),
                 gt_labels=rng.randint(0, 10, (k, G)).astype(np.int32),
                 gt_ids=rng.randint(0, 60000, (k, G)).astype(np.int32))
        c["run_digits"][k:] = T                                         # junk rows: must not be counted
        for i in range(k):
            # about half of the inferred objects sit near a ground-truth centre, so that matches, misses and contests all occur
            for t in range(T):
                if c["gt_count"][i] and rng.rand() < 0.6:
                    g = rng.randint(c["gt_count"][i])
                    cx, cy = st_center(*c["gt_positions"][i, g], *c["gt_boxes"][i, g], canvas_size)
                    c["att"][t, i, ATT_X] = np.float32(cx + rng.uniform(-0.2, 0.2))
                    c["att"][t, i, ATT_Y] = np.float32(cy + rng.uniform(-0.2, 0.2))
            name = by_index.get(g0 + i)
            if name is not None:
                pos, box, shifts = _planted_image(name, T, G)
                c["gt_count"][i], c["run_digits"][i] = len(pos), len(shifts)
                for g in range(len(pos)):
                    c["gt_positions"][i, g], c["gt_boxes"][i, g] = pos[g], box[g]
                for t, s in enumerate(shifts):
                    c["att"][t, i, ATT_X], c["att"][t, i, ATT_Y] = s
        chunks.append(c)
        g0 += k
    return dict(T=T, B=B, G=G, Z=Z, w=w, canvas_size=canvas_size, max_distance=max_distance, chunks=chunks, planted=slots)


def image_candidates(case, chunk, i):
    """-> (centres of the ground-truth digits of image i of the chunk, shifts [n, 2] float32 of its inferred objects)"""
    centers = [st_center(*chunk["gt_positions"][i, g], *chunk["gt_boxes"][i, g], case["canvas_size"])
               for g in range(int(chunk["gt_count"][i]))]
    n = int(chunk["run_digits"][i])
    return centers, chunk["att"][:n, i, ATT_X:ATT_Y + 1]


def margins(case, skip=()):
    """The smallest gap between two candidate distances of one digit, and between a candidate distance and max_distance, over
    the images of the case that are not in `skip` (global indices: the planted images tie on purpose, in exact numbers)"""
    pair, edge, g0 = math.inf, math.inf, 0
    for c in case["chunks"]:
        for i in range(c["k"]):
            if g0 + i in skip:
                continue
            centers, shifts = image_candidates(case, c, i)
            for ctr in centers:
                d = sorted(candidate_distances(ctr, shifts))
                pair = min([pair] + [b - a for a, b in zip(d, d[1:])])
                edge = min([edge] + [abs(x - case["max_distance"]) for x in d])
        g0 += c["k"]
    return pair, edge


def expected(case, capacity, rows, fill):
    """What air_embed_collect leaves after the chunks of `case`: per-chunk match [k, G]; the counters (matched, present,
    inferred, overflow); the four outputs with `rows` >= capacity rows, untouched rows holding fill[name]"""
    T, B, G, Z, w = (case[k] for k in ("T", "B", "G", "Z", "w"))
    assert rows >= capacity
    out = dict(latents=np.full((rows, Z), fill["latents"], np.float32), windows=np.full((rows, w * w), fill["windows"], np.float32),
               labels=np.full(rows, fill["labels"], np.int32), ids=np.full(rows, fill["ids"], np.int32))
    matches, row, present, inferred = [], 0, 0, 0
    for c in case["chunks"]:
        m = np.full((c["k"], G), -1, np.int32)
        for i in range(c["k"]):
            centers, shifts = image_candidates(case, c, i)
            present += len(centers); inferred += len(shifts)
            for g, t in enumerate(match_image(centers, shifts, case["max_distance"])):
                m[i, g] = t
                if t >= 0:
                    if row < capacity:
                        out["latents"][row], out["windows"][row] = c["ml"][t, i, :Z], c["vrec"][t, i]
                        out["labels"][row], out["ids"][row] = c["gt_labels"][i, g], c["gt_ids"][i, g]
                    row += 1
        matches.append(m)
    return matches, np.asarray([row, present, inferred, 1 if row > capacity else 0], np.int32), out


# the cases of tests/test_gpu_embeddings.py; the seeds were picked on the CPU so that margins() of the random images is
# above 1e-9 (tests/test_embedding_cases.py asserts it)
def gpu_cases():
    return {
        "chunks_z50_w28": synthetic_case(1, (5, 2), T=3, B=5, G=3, Z=50, w=28, planted=True),
        "chunks_z3_w5": synthetic_case(2, (5, 2), T=3, B=5, G=3, Z=3, w=5, planted=True),
        "below_tie_z3_w5": synthetic_case(2, (5, 2), T=3, B=5, G=3, Z=3, w=5, planted=True,
                                          max_distance=float(np.nextafter(FIVE_32, 0.0))),
        "b70": synthetic_case(3, (70,), T=3, B=70, G=2, Z=4, w=4),
        "b150_strided": synthetic_case(4, (150,), T=16, B=150, G=16, Z=4, w=4),
    }
