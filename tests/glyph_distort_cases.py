"""Shared by tests/test_glyph_distort_cases.py, tests/test_glyph_distort_abi.py, tests/test_gpu_glyph_distort.py and
tests/golden/make_glyph_distort.py: a numpy restatement of air_glyph_distort (include/air_hip.h, csrc/air_glyph_distort.hip)
in the kernel's operation order, and the small inputs the tests use.

Everything but cos / sin of the angle is an IEEE +, -, *, /, floor, min or max in fp64 (the build has -ffp-contract=off), so
the restatement reproduces every output bit for bit once it is given the kernel's own c, s.  Parameter stream: draw j of variant
v is word j & 3 of philox(key = seed, counter = (v, j >> 2, generation mod 2^32, 0x47445350)): word 0 picks the base glyph, then
two words per real -- angle, shear, sx, sy, each only when its bounds are not neutral -- and one word for the stroke.  Field
stream: element j of the two planes is word j & 3 of philox(same key, counter = (v, j >> 2, generation mod 2^32, 0x47445346))."""
import numpy as np

from oracle.philox_ref import MASK, philox4x32_10

SALT_P, SALT_F = 0x47445350, 0x47445346
MAX_PLANE, MAX_RADIUS, MAX_STROKE = 40, 64, 4
NEUTRAL = dict(max_ang=0.0, max_shear=0.0, min_scale=1.0, max_scale=1.0, min_stroke=0, max_stroke=0, lo=0.0, hi=1.0, sigma=1.0,
               alpha=0.0)
F32 = np.float32


def gaussian_taps(sigma, radius=None):
    """the normalised Gaussian of the host side: -> (taps [2 R + 1] float64, R); R = int(4 sigma + 0.5) unless given"""
    R = int(4.0 * float(sigma) + 0.5) if radius is None else int(radius)
    x = np.arange(-R, R + 1, dtype=np.float64)
    t = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return t / t.sum(), R


def field_gain(taps, alpha):
    """alpha / ((1 / sqrt 3) * sum taps^2): the smoothed field then has standard deviation alpha"""
    return float(alpha) / ((1.0 / np.sqrt(3.0)) * float(np.sum(taps * taps))) if alpha != 0.0 else 0.0


class Draws:
    """the parameter stream of one variant"""

    def __init__(self, v, generation, seed):
        self.words = philox4x32_10(int(v), np.arange(3, dtype=np.uint64), int(generation) & MASK, SALT_P, int(seed) & MASK,
                                   (int(seed) >> 32) & MASK).T.reshape(-1)
        self.j = 0

    def next(self):
        self.j += 1
        return int(self.words[self.j - 1])

    def index(self, span):
        return (self.next() * int(span)) >> 32

    def real(self, lo, hi):
        a, b = self.next(), self.next()
        u = (np.float64(a >> 5) * 67108864.0 + np.float64(b >> 6)) / 9007199254740992.0
        return np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u


def draw_variant(v, generation, seed, G, b):
    """-> (base glyph, angle, shear, sx, sy, n, words used); b: the bounds"""
    d = Draws(v, generation, seed)
    g = d.index(G)
    ang = k = np.float64(0.0)
    sx = sy = np.float64(1.0)
    n = 0
    if float(b["max_ang"]) != 0.0:
        ang = d.real(-np.float64(b["max_ang"]), b["max_ang"])
    if float(b["max_shear"]) != 0.0:
        k = d.real(-np.float64(b["max_shear"]), b["max_shear"])
    if float(b["min_scale"]) != 1.0 or float(b["max_scale"]) != 1.0:
        sx = d.real(b["min_scale"], b["max_scale"])
        sy = d.real(b["min_scale"], b["max_scale"])
    if int(b["min_stroke"]) != 0 or int(b["max_stroke"]) != 0:
        n = int(b["min_stroke"]) + d.index(int(b["max_stroke"]) - int(b["min_stroke"]) + 1)
    return g, ang, k, sx, sy, n, d.j


def uniform_of(words):
    """((word >> 8) + 0.5) * 2^-23 - 1: in (-1, 1), never 0"""
    return ((np.asarray(words, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -23 - 1.0


def field_uniforms(v, generation, seed, gd):
    """[2, gd, gd] float64: the two planes of uniform values of variant v"""
    n = 2 * gd * gd
    w = philox4x32_10(int(v), np.arange((n + 3) // 4, dtype=np.uint64), int(generation) & MASK, SALT_F, int(seed) & MASK,
                      (int(seed) >> 32) & MASK).T.reshape(-1)[:n]
    return uniform_of(w).reshape(2, gd, gd)


def smooth_axis(plane, taps, axis):
    """out[i] = sum over t ascending of taps[t] * in[i + t - R] along `axis`, zeros outside (adding +0 changes no bit)"""
    R = (len(taps) - 1) // 2
    a = np.moveaxis(np.asarray(plane, np.float64), axis, 0)
    n = a.shape[0]
    pad = np.zeros((n + 2 * R,) + a.shape[1:], np.float64)
    pad[R:R + n] = a
    acc = np.zeros_like(a)
    for t in range(2 * R + 1):
        acc = acc + np.float64(taps[t]) * pad[t:t + n]
    return np.moveaxis(acc, 0, axis)


def smooth(plane, taps, gain=1.0):
    """axis 0, then axis 1, the axis-1 sums times gain"""
    return smooth_axis(smooth_axis(plane, taps, 0) * 1.0, taps, 1) * np.float64(gain)


def warp(base, c, s, k, sx, sy, field=None):
    """stage 2 -> float32 [gd, gd]"""
    gd = base.shape[0]
    c, s, k = np.float64(c), np.float64(s), np.float64(k)
    isy, isx, ctr = 1.0 / np.float64(sy), 1.0 / np.float64(sx), (np.float64(gd) - 1.0) / 2.0
    a00, a01, a10, a11 = c * isy, (c * k + s) * isx, (-s) * isy, ((-s) * k + c) * isx
    y, x = np.meshgrid(np.arange(gd, dtype=np.float64), np.arange(gd, dtype=np.float64), indexing="ij")
    dy, dx = y - ctr, x - ctr
    qy, qx = ctr + (a00 * dy + a01 * dx), ctr + (a10 * dy + a11 * dx)
    if field is not None:
        qy, qx = qy + field[0], qx + field[1]
    with np.errstate(invalid="ignore"):
        inside = (qy > -1.0) & (qy < gd) & (qx > -1.0) & (qx < gd)
    qy, qx = np.where(inside, qy, 0.0), np.where(inside, qx, 0.0)
    fy, fx = np.floor(qy), np.floor(qx)
    ty, tx = qy - fy, qx - fx
    iy, ix = fy.astype(np.int64), fx.astype(np.int64)
    pad = np.zeros((gd + 2, gd + 2), np.float64)
    pad[1:-1, 1:-1] = base
    v00, v01, v10, v11 = pad[iy + 1, ix + 1], pad[iy + 1, ix + 2], pad[iy + 2, ix + 1], pad[iy + 2, ix + 2]
    uy, ux = 1.0 - ty, 1.0 - tx
    out = ((v00 * (uy * ux) + v01 * (uy * tx)) + v10 * (ty * ux)) + v11 * (ty * tx)
    return np.where(inside, out, 0.0).astype(F32)


def stroke(plane, n):
    """|n| passes of grey dilation (n > 0) / erosion (n < 0) over the 4-neighbour cross, neighbours outside left out"""
    p = np.array(plane, F32)
    op, fill = (np.maximum, -np.inf) if n > 0 else (np.minimum, np.inf)
    for _ in range(abs(int(n))):
        q = np.full((p.shape[0] + 2, p.shape[1] + 2), fill, F32)
        q[1:-1, 1:-1] = p
        p = op(op(op(op(q[1:-1, 1:-1], q[:-2, 1:-1]), q[2:, 1:-1]), q[1:-1, :-2]), q[1:-1, 2:])
    return p


def ramp(plane, lo, hi):
    t = (np.asarray(plane, F32).astype(np.float64) - np.float64(lo)) / (np.float64(hi) - np.float64(lo))
    r = np.minimum(np.maximum(t, 0.0), 1.0).astype(F32)
    return np.where(r < F32(0.05), F32(0), r)


def box_of(image):
    """(x0, y0, w, h) of the pixels > 0, or None"""
    ys, xs = np.nonzero(image > 0)
    if len(ys) == 0:
        return None
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def area_resample(a, n_out, axis):
    """float64: out[i] = (sum over j ascending of in[j] * overlap(i, j)) / r along `axis`, r = n_in / n_out"""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    n = a.shape[0]
    r = np.float64(n) / np.float64(n_out)
    i = np.arange(n_out, dtype=np.float64)
    lo, hi = i * r, (i + 1.0) * r
    acc = np.zeros((n_out,) + a.shape[1:], np.float64)
    for j in range(n):
        ov = np.maximum(np.minimum(np.float64(j + 1), hi) - np.maximum(np.float64(j), lo), 0.0)
        acc = acc + a[j][None] * ov.reshape((-1,) + (1,) * (a.ndim - 1))
    return np.moveaxis(acc / r, 0, axis)


def fit(image, ink):
    """stage 5 on the cropped h x w float32 image -> (f, float32 [h', w'] before the second crop)"""
    h, w = image.shape
    f = np.float64(ink) / np.float64(max(h, w))
    h2 = max(1, int(np.floor(np.float64(h) * f + 0.5)))
    w2 = max(1, int(np.floor(np.float64(w) * f + 0.5)))
    out = area_resample(area_resample(image, h2, 0), w2, 1).astype(F32)
    return f, np.where(out < F32(0.05), F32(0), out)


def centre(image, od):
    """stage 6 on the cropped float32 image -> (x0, y0, cx, cy)"""
    h, w = image.shape
    a = image.astype(np.float64)
    rm, rmx = np.zeros(h, np.float64), np.zeros(h, np.float64)
    for x in range(w):
        rm = rm + a[:, x]
        rmx = rmx + a[:, x] * np.float64(x)
    m = my = mx = np.float64(0.0)
    for r in range(h):
        m = m + rm[r]
        my = my + rm[r] * np.float64(r)
        mx = mx + rmx[r]
    cy, cx = my / m, mx / m
    mid = (np.float64(od) - 1.0) / 2.0
    y0 = int(min(max(np.floor(mid - cy + 0.5), 0.0), np.float64(od - h)))
    x0 = int(min(max(np.floor(mid - cx + 0.5), 0.0), np.float64(od - w)))
    return x0, y0, cx, cy


def finish(plane, n, lo, hi, ink, od):
    """stages 3 .. 6 on the warped plane -> (status, f, frame [od, od] or None, crop box (x0, y0, w, h))"""
    p = ramp(stroke(plane, n), lo, hi)
    b = box_of(p)
    if b is None:
        return 1, 0.0, None, (0, 0, 0, 0)
    f, fitted = fit(p[b[1]:b[1] + b[3], b[0]:b[0] + b[2]], ink)
    b = box_of(fitted)
    if b is None:
        return 1, f, None, (0, 0, 0, 0)
    glyph = fitted[b[1]:b[1] + b[3], b[0]:b[0] + b[2]]
    h, w = glyph.shape
    x0, y0, _, _ = centre(glyph, od)
    if h > od or w > od:
        return 2, f, None, (0, 0, 0, 0)
    frame = np.zeros((od, od), F32)
    frame[y0:y0 + h, x0:x0 + w] = glyph
    return 0, f, frame, (x0, y0, w, h)


def cosdg_sindg(angle):
    from scipy.special import cosdg, sindg
    return float(cosdg(angle)), float(sindg(angle))


def distort_bank(glyphs, V, od, ink, seed, generation=0, cs=None, radius=None, **bounds):
    """dict of the five outputs of one launch.  glyphs [G, gd, gd] float32; cs: None (cosdg / sindg of the drawn angles) or
    [V, 2], the kernel's own c, s; bounds: NEUTRAL's keys (sigma, alpha make the taps and the gain as the host side does)"""
    b = dict(NEUTRAL, **bounds)
    taps, _ = gaussian_taps(b["sigma"], radius)
    gain = field_gain(taps, b["alpha"])
    G, gd = len(glyphs), glyphs.shape[1]
    bank = np.zeros((V, od, od), F32)
    bank_crops, source, status = np.zeros((V, 4), np.int32), np.zeros(V, np.int32), np.zeros(V, np.int32)
    params = np.zeros((V, 8), np.float64)
    for v in range(V):
        g, ang, k, sx, sy, n, _ = draw_variant(v, generation, seed, G, b)
        c, s = (1.0, 0.0) if float(b["max_ang"]) == 0.0 else cosdg_sindg(ang) if cs is None else (float(cs[v][0]), float(cs[v][1]))
        field = None
        if gain != 0.0:
            u = field_uniforms(v, generation, seed, gd)
            field = (smooth(u[0], taps, gain), smooth(u[1], taps, gain))
        st, f, frame, box = finish(warp(np.asarray(glyphs[g], F32), c, s, k, sx, sy, field), n, b["lo"], b["hi"], ink, od)
        source[v], status[v], bank_crops[v] = g, st, box
        params[v] = (ang, k, sx, sy, c, s, n, f)
        if st == 0:
            bank[v] = frame
    return dict(bank=bank.reshape(V, od * od), bank_crops=bank_crops, source=source, params=params, status=status)


# ---- the inputs of the tests ------------------------------------------------------------------------------------------------
MNIST_LIKE = dict(max_ang=12.0, max_shear=0.2, min_scale=0.85, max_scale=1.15, min_stroke=-1, max_stroke=1, lo=0.3, hi=0.7,
                  sigma=6.0, alpha=1.5)
AFFINE = dict(max_ang=30.0, max_shear=0.3, min_scale=0.8, max_scale=1.25)


def blob_glyphs(G, gd, seed=7):
    """[G, gd, gd] float32 in [0, 1]: smooth random strokes with boxes of about 3 .. gd pixels (one touches the border)"""
    rng = np.random.RandomState(seed)
    out = np.zeros((G, gd, gd), F32)
    for i in range(G):
        h, w = rng.randint(3, gd + 1, 2) if i else (gd, gd)
        y0, x0 = rng.randint(0, gd - h + 1), rng.randint(0, gd - w + 1)
        out[i, y0:y0 + h, x0:x0 + w] = np.round(rng.uniform(0.3, 1.0, (h, w)) * (rng.uniform(size=(h, w)) < 0.7), 3)
        out[i, y0, x0] = out[i, y0 + h - 1, x0 + w - 1] = 1.0
    return out


def thin_glyphs(gd=8):
    """strokes one and two pixels thin, 1 x k and k x 1, a single pixel, and one block that survives two erosions"""
    g = np.zeros((7, gd, gd), F32)
    g[0, 3, 1:7] = (0.5, 1.0, 0.75, 1.0, 0.25, 0.9)        # 1 x 6
    g[1, 1:6, 4] = (1.0, 0.6, 1.0, 0.8, 0.3)               # 5 x 1
    g[2, 2:4, 1:7] = 1.0                                   # 2 x 6
    g[3, 1:7, 5:7] = 0.9                                   # 6 x 2
    g[4, 4, 4] = 1.0                                       # one pixel
    g[5, 0, 0:3] = (1.0, 1.0, 0.4)                         # 1 x 3 in the corner
    g[6, 1:7, 2:7] = 0.8                                   # 6 x 5: two erosions leave 2 x 1
    return g


GPU_V = 256
GPU_CASES = {                      # name: (glyph set, gd, od, ink, seed, generation, radius or None, bounds)
    "small": ("blobs", 8, 16, 10, 201, 0, 9, dict(MNIST_LIKE, sigma=2.0, alpha=0.6)),          # R >= gd; boxes 3 .. 8 -> 10
    "preset": ("blobs", 24, 28, 20, 202, 2, None, dict(MNIST_LIKE)),
    "one_tap": ("blobs", 8, 16, 10, 203, 0, 0, dict(AFFINE, sigma=1.0, alpha=0.5)),             # R = 0: a single tap of 1.0
    "affine": ("blobs", 8, 16, 10, 204, 1, None, dict(AFFINE)),                                 # alpha = 0
    "field": ("blobs", 8, 16, 10, 205, 0, None, dict(sigma=1.5, alpha=1.0)),
    "thin": ("thin", 8, 16, 10, 206, 0, None, dict(min_stroke=-2, max_stroke=-2, lo=0.0, hi=1.0)),
    "thick": ("thin", 8, 16, 6, 207, 0, None, dict(min_stroke=2, max_stroke=2, max_ang=20.0)),
    "lines": ("thin", 8, 16, 6, 208, 0, None, dict(min_stroke=0, max_stroke=1)),                # 1 x k and k x 1 crops
    "border": ("blobs", 8, 16, 10, 209, 0, None, dict(max_ang=45.0, min_scale=0.8, max_scale=1.4)),    # ink leaves the plane
    "clamped": ("blobs", 8, 12, 12, 210, 0, None, dict(AFFINE, min_stroke=-1, max_stroke=1)),   # od = ink
    "late": ("blobs", 8, 16, 10, 211, (1 << 32) + 5, None, dict(MNIST_LIKE, sigma=2.0, alpha=0.6)),
}


def gpu_glyphs(name, gd):
    return thin_glyphs(gd) if name == "thin" else blob_glyphs(12, gd)
