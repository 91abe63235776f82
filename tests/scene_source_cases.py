"""Shared by tests/test_scene_source_abi.py and tests/test_gpu_scene_source.py: a numpy restatement of
air_scene_source_compose (include/air_hip.h, csrc/air_scenes.hip) and the small glyph sets the tests use.

The kernel's decisions are integer arithmetic on Philox4x32-10 words, so the restatement reproduces every output bit for
bit: draw j of scene b in batch k is word j & 3 of philox(key = seed, counter = (b, j >> 2, k mod 2^32, 0x5343454E)); an
integer in [lo, lo + span) is lo + ((word * span) >> 32); draw 0 is the digit count (when it is drawn), then per digit the
glyph index and per attempt x, then y; j keeps counting across restarts."""
import numpy as np

from oracle.philox_ref import MASK, philox4x32_10

SALT = 0x5343454E


class Draws:
    """the draw stream of one scene; the words are made 64 quads at a time"""

    def __init__(self, b, batch, seed):
        self.b, self.batch, self.seed, self.j = int(b), int(batch) & MASK, int(seed), 0
        self.words = np.zeros((0, 4), np.uint32)

    def next(self):
        q = self.j >> 2
        while q >= len(self.words):
            qs = np.arange(len(self.words), len(self.words) + 64, dtype=np.uint64)
            w = philox4x32_10(self.b, qs, self.batch, SALT, self.seed & MASK, (self.seed >> 32) & MASK)
            self.words = np.concatenate([self.words, np.ascontiguousarray(w.T)])
        v = int(self.words[q, self.j & 3])
        self.j += 1
        return v

    def range(self, lo, span):
        return lo + ((self.next() * int(span)) >> 32)


def dilate(ink, gap):
    """bool [C, C]: within Chebyshev distance `gap` of a True pixel (nothing outside the canvas)"""
    C = ink.shape[0]
    out = np.zeros_like(ink)
    for dy in range(-gap, gap + 1):
        for dx in range(-gap, gap + 1):
            ya, yb, xa, xb = max(0, dy), min(C, C + dy), max(0, dx), min(C, C + dx)
            out[ya:yb, xa:xb] |= ink[ya - dy:yb - dy, xa - dx:xb - dx]
    return out


def touches(occ, glyph, x, y):
    """the device rule: an ink pixel of `glyph` (its crop box, placed with its top-left corner at x, y) on an occupied pixel"""
    h, w = glyph.shape
    return bool(np.any((glyph > 0) & occ[y:y + h, x:x + w]))


def compose_scene(b, batch, glyphs, crops, C, margin, gap, max_digits, max_attempts, max_restarts, seed, count=None, bg=None):
    """one scene -> (image [C * C] float32, digits, indices [max_digits], positions [2 max_digits], boxes [2 max_digits],
    status); glyphs [G, gd, gd] float32, crops [G, 4]"""
    d = Draws(b, batch, seed)
    gd = glyphs.shape[1]
    n = d.range(0, max_digits + 1) if count is None else min(max(int(count), 0), max_digits)
    ok, restarts = False, 0
    while restarts < max_restarts:
        canvas = np.zeros((C, C), np.float32)
        occ = np.zeros((C, C), bool)
        idx, pos, box = np.zeros(max_digits, np.int32), np.zeros(2 * max_digits, np.int32), np.zeros(2 * max_digits, np.int32)
        ok = True
        for i in range(n):
            g = d.range(0, len(glyphs))
            x0, y0, w, h = (int(v) for v in crops[g])
            if not (w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= gd and y0 + h <= gd) or w + 2 * margin > C or h + 2 * margin > C:
                ok = False
                break
            glyph = glyphs[g, y0:y0 + h, x0:x0 + w]
            found = False
            for _ in range(max_attempts):
                x = d.range(margin, C - w - 2 * margin + 1)           # [margin, C - w - margin]
                y = d.range(margin, C - h - 2 * margin + 1)
                found = i == 0 or not touches(occ, glyph, x, y)
                if found:
                    break
            if not found:
                ok = False
                break
            canvas[y:y + h, x:x + w] += glyph
            ink = np.zeros((C, C), bool)
            ink[y:y + h, x:x + w] = glyph > 0
            occ |= dilate(ink, gap)
            idx[i], pos[2 * i], pos[2 * i + 1], box[2 * i], box[2 * i + 1] = g, x, y, w, h
        if ok:
            break
        restarts += 1
    if not ok:
        canvas = np.zeros((C, C), np.float32)
        idx[:], pos[:], box[:] = 0, 0, 0
    if bg is not None:
        canvas = np.clip(canvas + np.asarray(bg, np.float32).reshape(C, C), np.float32(0), np.float32(1))
    return canvas.reshape(-1), (n if ok else 0), idx, pos, box, (restarts if ok else -1)


def compose_batch(B, batch, glyphs, crops, C, margin, gap, max_digits, max_attempts, max_restarts, seed, counts=None, bg=None):
    """dict of the six outputs of one launch"""
    rows = [compose_scene(b, batch, glyphs, crops, C, margin, gap, max_digits, max_attempts, max_restarts, seed,
                          None if counts is None else counts[b], bg) for b in range(B)]
    return dict(images=np.stack([r[0] for r in rows]), digits=np.asarray([r[1] for r in rows], np.int32),
                indices=np.stack([r[2] for r in rows]), positions=np.stack([r[3] for r in rows]),
                boxes=np.stack([r[4] for r in rows]), status=np.asarray([r[5] for r in rows], np.int32))


def crop_boxes(glyphs):
    """[G, 4] int32 x0, y0, w, h of the non-empty box of every glyph of [G, gd, gd] (crop_non_empty of the generator)"""
    out = np.zeros((len(glyphs), 4), np.int32)
    for i, g in enumerate(glyphs):
        cols, rows = np.nonzero(g.sum(0))[0], np.nonzero(g.sum(1))[0]
        out[i] = (cols[0], rows[0], cols[-1] - cols[0] + 1, rows[-1] - rows[0] + 1)
    return out


def ragged_glyphs(count=12, gd=8, lo=4, hi=7, seed=11):
    """[count, gd, gd] float32: filled rectangles of lo..hi pixels a side somewhere in the frame, fractional ink values
    (multiples of 1/16 in [0.25, 1]), a ragged right column and bottom row (pixels knocked out, never all of them, so the
    crop box is the rectangle)"""
    rng = np.random.RandomState(seed)
    out = np.zeros((count, gd, gd), np.float32)
    for g in out:
        w, h = rng.randint(lo, hi + 1), rng.randint(lo, hi + 1)
        x0, y0 = rng.randint(0, gd - w + 1), rng.randint(0, gd - h + 1)
        g[y0:y0 + h, x0:x0 + w] = rng.randint(4, 17, size=(h, w)) / 16.0
        g[y0 + 1:y0 + h, x0 + w - 1] *= rng.randint(0, 2, size=h - 1)        # the top pixel of the right column stays
        g[y0 + h - 1, x0 + 1:x0 + w - 1] *= rng.randint(0, 2, size=w - 2)    # the left pixel of the bottom row stays
    return out
