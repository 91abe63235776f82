"""Shared by tests/test_glyph_jitter_cases.py, tests/test_glyph_jitter_abi.py, tests/test_gpu_glyph_jitter.py and
tests/golden/make_glyph_jitter.py: a numpy restatement of air_glyph_jitter (include/air_hip.h, csrc/air_glyph_jitter.hip)
in the kernel's operation order, and the small inputs the tests use.

Everything but cos / sin of the angle is an IEEE +, -, *, / or floor in fp64 (the build has -ffp-contract=off), so the
restatement reproduces every output bit for bit once it is given the kernel's own c, s.  Draw j of variant v is word j & 3
of philox(key = seed, counter = (v, j >> 2, generation mod 2^32, 0x474A4954)): word 0 picks the base glyph, then two words
per real -- new_width, new_height (only when a scale bound is not 1.0), angle (only when an angle bound is not 0.0)."""
import numpy as np

from oracle.philox_ref import MASK, philox4x32_10

SALT = 0x474A4954
MAX_PLANE, MAX_ROTATED = 48, 64
Z1 = np.sqrt(67.5 - np.sqrt(4436.25)) + np.sqrt(26.25) - 6.5
Z2 = np.sqrt(67.5 + np.sqrt(4436.25)) - np.sqrt(26.25) - 6.5
POLES = (float(Z1), float(Z2))
GAIN = (1.0 * ((1.0 - POLES[0]) * (1.0 - 1.0 / POLES[0]))) * ((1.0 - POLES[1]) * (1.0 - 1.0 / POLES[1]))
NEUTRAL = dict(min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0)


class Draws:
    """the draw stream of one variant"""

    def __init__(self, v, generation, seed):
        self.words = philox4x32_10(int(v), np.arange(2, dtype=np.uint64), int(generation) & MASK, SALT, int(seed) & MASK,
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


def draw_variant(v, generation, seed, G, j):
    """-> (base glyph, new_width, new_height, angle, scaled?, rotated?); j: the six bounds"""
    d = Draws(v, generation, seed)
    g = d.index(G)
    scaled = any(float(j[k]) != 1.0 for k in ("min_w", "max_w", "min_h", "max_h"))
    rotated = float(j["min_ang"]) != 0.0 or float(j["max_ang"]) != 0.0
    nw = nh = np.float64(1.0)
    ang = np.float64(0.0)
    if scaled:
        nw = d.real(j["min_w"], j["max_w"])
        nh = d.real(j["min_h"], j["max_h"])
    if rotated:
        ang = d.real(j["min_ang"], j["max_ang"])
    return g, nw, nh, ang, scaled, rotated


def prefilter(plane):
    """the order-5 B-spline coefficients of a 2-D plane, mirror boundaries: axis 0, then axis 1; fp64"""
    c = np.array(plane, np.float64)
    for axis in (0, 1):
        c = np.moveaxis(c, axis, 0)                   # c[i]: element i of every line
        n = c.shape[0]
        if n > 1:
            c *= GAIN
            for z in POLES:
                zn = np.float64(1.0)
                for _ in range(n - 1):
                    zn = zn * z
                c0 = c[0] + zn * c[n - 1]
                zi = np.float64(z)
                for i in range(1, n - 1):
                    c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
                    zi = zi * z
                c[0] = c0 / (1.0 - zn * zn)
                for i in range(1, n):
                    c[i] = c[i] + z * c[i - 1]
                c[n - 1] = ((z * c[n - 2] + c[n - 1]) * z) / (z * z - 1.0)
                for i in range(n - 2, -1, -1):
                    c[i] = z * (c[i + 1] - c[i])
        c = np.moveaxis(c, 0, axis)
    return np.ascontiguousarray(c)


def weights(x):
    """the six order-5 B-spline weights of the taps floor - 2 .. floor + 3 at fraction x (arrays): [6, ...]"""
    t = x * x
    w2 = t * (t * (0.25 - x / 12.0) - 0.5) + 0.55
    y = 1.0 - x
    t = y * y
    w3 = t * (t * (0.25 - y / 12.0) - 0.5) + 0.55
    w0 = y * t * t / 120.0
    y = x + 1.0
    w1 = y * (y * (y * (y * (y / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425
    y = 2.0 - x
    w4 = y * (y * (y * (y * (y / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425
    w5 = 1.0 - ((((w0 + w1) + w2) + w3) + w4)
    return np.stack([w0, w1, w2, w3, w4, w5])


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def transform(image, m, off, out_shape, raw=False):
    """affine_transform(order=5, mode='constant', cval=0) of a float32 plane -> float32 [out_shape] (raw), then clipped to
    [0, 1] and values < 0.05 zeroed.  Coordinates (oy m00 + ox m01) + off0, (oy m10 + ox m11) + off1; the 36 products
    (coefficient * wy) * wx are summed row by row from the top-left tap."""
    h, w = image.shape
    coef = prefilter(image)
    oy, ox = np.meshgrid(np.arange(out_shape[0], dtype=np.float64), np.arange(out_shape[1], dtype=np.float64), indexing="ij")
    cy = (oy * m[0] + ox * m[1]) + off[0]
    cx = (oy * m[2] + ox * m[3]) + off[1]
    inside = ~((cy < 0) | (cy > h - 1) | (cx < 0) | (cx > w - 1))
    cy, cx = np.where(inside, cy, 0.0), np.where(inside, cx, 0.0)
    fy, fx = np.floor(cy), np.floor(cx)
    wy, wx = weights(cy - fy), weights(cx - fx)
    iy, ix = fy.astype(np.int64), fx.astype(np.int64)
    t = np.zeros(out_shape, np.float64)
    for ky in range(6):
        my = mirror(iy - 2 + ky, h)
        for kx in range(6):
            t = t + (coef[my, mirror(ix - 2 + kx, w)] * wy[ky]) * wx[kx]
    out = np.where(inside, t, 0.0).astype(np.float32)
    if raw:
        return out
    out = np.minimum(np.maximum(out, np.float32(0)), np.float32(1))
    return np.where(out < np.float32(0.05), np.float32(0), out)


def box_of(image):
    """(x0, y0, w, h) of the pixels > 0, or None"""
    ys, xs = np.nonzero(image > 0)
    if len(ys) == 0:
        return None
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def crop(image):
    b = box_of(image)
    return None if b is None else image[b[1]:b[1] + b[3], b[0]:b[0] + b[2]]


def scale_stage(image, gd, nw, nh, raw=False):
    """-> (status, image): 0 and the cropped result; 1 when it is empty; 2 when the plane leaves 1 .. MAX_PLANE"""
    OH, OW = int(np.float64(gd) * nh), int(np.float64(gd) * nw)
    if OH < 1 or OW < 1 or OH > MAX_PLANE or OW > MAX_PLANE:
        return 2, None
    out = transform(image, (1.0 / nh, 0.0, 0.0, 1.0 / nw), (0.0, 0.0), (OH, OW), raw)
    if raw:
        return 0, out
    out = crop(out)
    return (1, None) if out is None else (0, out)


def rotate_geometry(h, w, c, s):
    """scipy.ndimage.rotate(reshape=True): -> (OH, OW, offset y, offset x)"""
    c, s, hh, ww = np.float64(c), np.float64(s), np.float64(h), np.float64(w)
    r0 = (0.0, s * ww, c * hh, c * hh + s * ww)
    r1 = (0.0, c * ww, (-s) * hh, (-s) * hh + c * ww)
    OH, OW = int((max(r0) - min(r0)) + 0.5), int((max(r1) - min(r1)) + 0.5)
    a, b = (np.float64(OH) - 1.0) / 2.0, (np.float64(OW) - 1.0) / 2.0
    return OH, OW, (hh - 1.0) / 2.0 - (c * a + s * b), (ww - 1.0) / 2.0 - ((-s) * a + c * b)


def rotate_stage(image, c, s, raw=False):
    h, w = image.shape
    OH, OW, offy, offx = rotate_geometry(h, w, c, s)
    if OH < 1 or OW < 1 or OH > MAX_ROTATED or OW > MAX_ROTATED:
        return 2, None
    out = transform(image, (c, s, -s, c), (offy, offx), (OH, OW), raw)
    if raw:
        return 0, out
    out = crop(out)
    return (1, None) if out is None else (0, out)


def cosdg_sindg(angle):
    from scipy.special import cosdg, sindg
    return float(cosdg(angle)), float(sindg(angle))


def jitter_bank(glyphs, crops, V, od, seed, generation=0, cs=None, **bounds):
    """dict of the five outputs of one launch.  glyphs [G, gd, gd] float32, crops [G, 4]; cs: None (cosdg / sindg of the
    drawn angles) or [V, 2], the kernel's own c, s"""
    j = dict(NEUTRAL, **bounds)
    G, gd = len(glyphs), glyphs.shape[1]
    bank = np.zeros((V, od, od), np.float32)
    bank_crops, source, status = np.zeros((V, 4), np.int32), np.zeros(V, np.int32), np.zeros(V, np.int32)
    params = np.zeros((V, 6), np.float64)
    for v in range(V):
        g, nw, nh, ang, scaled, rotated = draw_variant(v, generation, seed, G, j)
        c, s = (1.0, 0.0) if not rotated else cosdg_sindg(ang) if cs is None else (float(cs[v][0]), float(cs[v][1]))
        source[v], params[v] = g, (nw, nh, ang, c, s, 0.0)
        x0, y0, w, h = (int(t) for t in crops[g])
        st = 0 if w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= gd and y0 + h <= gd else 1
        image = glyphs[g, y0:y0 + h, x0:x0 + w] if st == 0 else None
        if st == 0 and scaled:
            st, image = scale_stage(image, gd, nw, nh)
        if st == 0 and rotated:
            st, image = rotate_stage(image, c, s)
        if st == 0 and (image.shape[0] > od or image.shape[1] > od):
            st = 2
        status[v] = st
        if st == 0:
            bank[v, :image.shape[0], :image.shape[1]] = image
            bank_crops[v] = (0, 0, image.shape[1], image.shape[0])
    return dict(bank=bank.reshape(V, od * od), bank_crops=bank_crops, source=source, params=params, status=status)


# ---- the same pipeline on scipy -------------------------------------------------------------------------------------------
def scipy_variant(image, gd, nw, nh, ang, scaled, rotated, raws=None):
    """the reference's lines :113-135 on scipy.ndimage -> the final glyph, or None when a crop is empty; raws: a list that
    collects the values of both stages before clip and threshold"""
    import scipy.ndimage as nd
    image = np.asarray(image, np.float32)
    for stage in ("scale", "rotate"):
        if stage == "scale" and scaled:
            image = nd.affine_transform(image, matrix=np.array([[1.0 / nh, 0.0], [0.0, 1.0 / nw]]),
                                        output_shape=(int(gd * nh), int(gd * nw)), order=5)
        elif stage == "rotate" and rotated:
            image = nd.rotate(image, ang, order=5)
        else:
            continue
        if raws is not None:
            raws.append(image.copy())
        image = np.clip(image, 0.0, 1.0)
        image = np.where(image >= 0.05, image, np.zeros_like(image))
        if not image.any():
            return None
        image = crop(image)
    return image


def adjacent_or_equal(a, b):
    """float32 arrays of non-negative values: equal, or neighbours in float32"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= 1))


def thin_glyphs():
    """hand-made 8x8 glyphs whose crops are 1 x k, k x 1, 2 x 2 and a single pixel: the n = 1 line of the prefilter, the
    mirror at n = 2, and the plane where every coordinate but 0 is outside"""
    g = np.zeros((6, 8, 8), np.float32)
    g[0, 3, 1:7] = (0.5, 1.0, 0.75, 1.0, 0.25, 0.9)        # 1 x 6
    g[1, 1:6, 4] = (1.0, 0.6, 1.0, 0.8, 0.3)               # 5 x 1
    g[2, 2:4, 5:7] = ((1.0, 0.5), (0.7, 0.9))              # 2 x 2
    g[3, 4, 4] = 1.0                                       # one pixel
    g[4, 0, 0:3] = (1.0, 1.0, 0.4)                         # 1 x 3 in the corner
    g[5, 5:7, 2] = (0.8, 1.0)                              # 2 x 1
    return g


# ---- the inputs of tests/test_gpu_glyph_jitter.py and of the scipy fixture tests/golden/glyph_jitter_scipy.npz ---------------
SCALE = dict(min_w=0.8, max_w=1.25, min_h=0.8, max_h=1.25)
ANGLE = dict(min_ang=-30.0, max_ang=30.0)
GPU_V, GPU_GD, GPU_OD = 256, 8, 16
GPU_CASES = {                      # name: (glyph set, od, seed, generation, bounds)
    "scale": ("ragged", GPU_OD, 101, 0, SCALE),
    "rotate": ("ragged", GPU_OD, 102, 0, ANGLE),
    "both": ("ragged", GPU_OD, 103, 3, dict(SCALE, **ANGLE)),
    "late": ("ragged", GPU_OD, 104, (1 << 32) + 5, dict(SCALE, **ANGLE)),
    "crowded": ("mixed", 8, 105, 1, dict(min_w=0.5, max_w=1.5, min_h=0.5, max_h=1.5, min_ang=-45.0, max_ang=45.0)),
}
FIXTURE_CASES = ("scale", "rotate", "both")


def gpu_glyphs(name):
    """[12, 8, 8] float32 and its crop boxes.  ragged: scene_source_cases.ragged_glyphs(); mixed: eight of those and four thin
    ones (a row, a column, one pixel, two pixels) that a scale or a rotation can wipe out"""
    import scene_source_cases as sc
    g = sc.ragged_glyphs()
    if name == "mixed":
        g = np.concatenate([g[:8], thin_glyphs()[[0, 1, 3, 5]]])
    return g, sc.crop_boxes(g)


def scipy_bank(glyphs, crops, V, seed, generation, bounds, raws=None):
    """the final glyph of every variant on scipy.ndimage, for the restatement's draws: a list of arrays, None where empty"""
    j = dict(NEUTRAL, **bounds)
    out = []
    for v in range(V):
        g, nw, nh, ang, scaled, rotated = draw_variant(v, generation, seed, len(glyphs), j)
        x0, y0, w, h = (int(t) for t in crops[g])
        out.append(scipy_variant(glyphs[g, y0:y0 + h, x0:x0 + w], glyphs.shape[1], nw, nh, ang, scaled, rotated, raws))
    return out
