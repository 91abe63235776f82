"""The numpy restatement of air_glyph_distort (tests/glyph_distort_cases.py) against known answers: what every stage must
give where the answer can be written down without it (identity settings, scipy.ndimage, np.rot90, pair means), the draw
streams, and the geometry of a bank of the MNIST_LIKE preset.  The kernel is held to the restatement bit for bit by
tests/test_gpu_glyph_distort.py; this file is what makes the restatement worth being held to."""
import numpy as np
import pytest

import glyph_distort_cases as gd
from oracle.philox_ref import MASK, philox4x32_10

F32 = np.float32


def l_glyph():
    """an L in an 8 x 8 plane: a 6-pixel bar down the left, a 4-pixel foot along the bottom; box 4 wide, 6 high at (2, 1)"""
    g = np.zeros((8, 8), F32)
    g[1:7, 2] = (1.0, 0.875, 0.75, 0.625, 0.5, 1.0)
    g[6, 3:6] = 1.0
    return g


# ---------------------------------------------------------------------------------------------------- neutral settings
def test_neutral_bounds_give_the_cropped_glyph_back_bit_for_bit():
    """all bounds neutral, alpha = 0, ink = the larger side of the glyph's box: every stage is the identity on the values"""
    glyphs = gd.blob_glyphs(12, 8)
    for g, glyph in enumerate(glyphs):
        x0, y0, w, h = gd.box_of(np.where(glyph < F32(0.05), 0, glyph))
        out = gd.distort_bank(glyphs[g:g + 1], 1, 16, max(h, w), seed=3)
        assert out["status"][0] == 0 and out["source"][0] == 0
        bx, by, bw, bh = out["bank_crops"][0]
        assert (bw, bh) == (w, h)
        frame = out["bank"][0].reshape(16, 16)
        want = np.where(glyph < F32(0.05), F32(0), glyph)[y0:y0 + h, x0:x0 + w]
        assert np.array_equal(frame[by:by + bh, bx:bx + bw].view(np.uint32), want.view(np.uint32)), g
        rest = frame.copy()
        rest[by:by + bh, bx:bx + bw] = 0
        assert not rest.any() and not np.signbit(rest).any()                       # +0 elsewhere
        assert np.array_equal(out["params"][0], (0, 0, 1, 1, 1, 0, 0, 1.0))


def test_centring_of_an_l_by_hand():
    """the L's mass by rows: 1, .875, .75, .625, .5 and the foot's 4 -> m = 7.75, cy = (.875 + 1.5 + 1.875 + 2 + 20) / 7.75 =
    26.25 / 7.75 = 3.387..; by columns: 4.75, 1, 1, 1 -> cx = (1 + 2 + 3) / 7.75 = 0.774.. (every sum is exact in binary).
    od = 8: y0 = floor(3.5 - 3.387 + .5) = 0, x0 = floor(3.5 - .774 + .5) = 3, x free (od - w = 4).
    od = 6 = h: floor(2.5 - 3.387 + .5) = -1 is clamped to 0; x0 = floor(2.226) = 2 = od - w."""
    g = l_glyph()[1:7, 2:6]
    x0, y0, cx, cy = gd.centre(g, 8)
    assert (x0, y0) == (3, 0) and cy == 26.25 / 7.75 and cx == 6.0 / 7.75
    assert gd.centre(g, 6)[:2] == (2, 0)
    # both clamps along x: the mass at the right end asks for x0 = floor(3.5 - 5 / 1.1 + .5) = -1; at the left end for
    # floor(3.5 - .5 / 1.1 + .5) = 3 > od - w = 2.  A single row: y0 = floor(3.5 - 0 + .5) = 4
    r = np.zeros((1, 6), F32)
    r[0, 0], r[0, 5] = 0.1, 1.0
    assert gd.centre(r, 8)[:2] == (0, 4) and gd.centre(r[:, ::-1], 8)[:2] == (2, 4)
    out = gd.distort_bank(l_glyph()[None], 1, 6, 6, seed=1)
    assert tuple(out["bank_crops"][0]) == (2, 0, 4, 6) and out["status"][0] == 0
    assert np.array_equal(out["bank"][0].reshape(6, 6)[:, 2:], g) and not out["bank"][0].reshape(6, 6)[:, :2].any()


# ---------------------------------------------------------------------------------------------------------- the stages
def test_smoothing_is_scipys_constant_mode_convolution():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(0)
    for gdim, sigma, radius in ((8, 2.0, 9), (13, 1.5, None), (24, 6.0, None), (5, 1.0, 0), (7, 3.0, 40)):
        taps, R = gd.gaussian_taps(sigma, radius)
        assert len(taps) == 2 * R + 1 and abs(taps.sum() - 1.0) < 1e-15
        plane = rng.uniform(-1, 1, (gdim, gdim))
        want = nd.convolve1d(nd.convolve1d(plane, taps, axis=0, mode="constant"), taps, axis=1, mode="constant")
        got = gd.smooth(plane, taps, 1.0)
        assert np.abs(got - want).max() <= 16 * 2.0 ** -53, (gdim, R)             # sums of <= 2 * 81 terms of magnitude < 1
        assert np.array_equal(gd.smooth(plane, taps, 2.5), got * 2.5)
    assert np.array_equal(gd.smooth(plane, np.ones(1), 1.0), plane)               # a single tap of 1.0


def test_field_gain_gives_the_field_its_standard_deviation():
    """away from the border the smoothed field of uniform(-1, 1) values has standard deviation alpha"""
    taps, R = gd.gaussian_taps(1.5)
    gain = gd.field_gain(taps, 2.0)
    u = np.random.RandomState(1).uniform(-1, 1, (200, 200))
    f = gd.smooth(u, taps, gain)[R:-R, R:-R]
    assert abs(f.std() - 2.0) < 0.1
    assert gd.field_gain(taps, 0.0) == 0.0


def test_warp_identity_and_quarter_turn():
    base = gd.blob_glyphs(3, 9)[1]
    assert np.array_equal(gd.warp(base, 1.0, 0.0, 0.0, 1.0, 1.0), base)
    zero = (np.zeros((9, 9)), np.zeros((9, 9)))
    assert np.array_equal(gd.warp(base, 1.0, 0.0, 0.0, 1.0, 1.0, zero), base)
    for plane in (base, gd.blob_glyphs(3, 8)[2]):                                   # odd and even sides
        assert np.array_equal(gd.warp(plane, 0.0, 1.0, 0.0, 1.0, 1.0), np.rot90(plane))
        assert np.array_equal(gd.warp(plane, -1.0, 0.0, 0.0, 1.0, 1.0), np.rot90(plane, 2))
        assert np.array_equal(gd.warp(plane, 0.0, -1.0, 0.0, 1.0, 1.0), np.rot90(plane, 3))
    # a constant field of one pixel shifts the plane, zeros come in from outside
    one = (np.ones((9, 9)), np.zeros((9, 9)))
    want = np.zeros_like(base)
    want[:-1] = base[1:]
    assert np.array_equal(gd.warp(base, 1.0, 0.0, 0.0, 1.0, 1.0, one), want)
    # half a pixel: the mean of two rows, the last row with zero
    half = (np.full((9, 9), 0.5), np.zeros((9, 9)))
    want = ((base.astype(np.float64) + np.vstack([base[1:], np.zeros((1, 9))])) * 0.5).astype(F32)
    assert np.array_equal(gd.warp(base, 1.0, 0.0, 0.0, 1.0, 1.0, half), want)
    # coordinates that leave every range give zeros, not an error
    assert not gd.warp(base, 1.0, 0.0, 0.0, 1e-300, 1e-300).any()


def test_stroke_is_grey_dilation_and_erosion_over_the_cross():
    nd = pytest.importorskip("scipy.ndimage")
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    plane = np.random.RandomState(2).uniform(0, 1, (11, 9)).astype(F32)
    for n in (1, 2, 4):
        d, e = plane, plane
        for _ in range(n):
            d, e = nd.grey_dilation(d, footprint=cross), nd.grey_erosion(e, footprint=cross)
        assert np.array_equal(gd.stroke(plane, n)[n:-n, n:-n], d[n:-n, n:-n])
        assert np.array_equal(gd.stroke(plane, -n)[n:-n, n:-n], e[n:-n, n:-n])
    assert np.array_equal(gd.stroke(plane, 0), plane)
    # neighbours outside are left out: a constant plane stays constant under both
    const = np.full((5, 5), 0.5, F32)
    assert np.array_equal(gd.stroke(const, 2), const) and np.array_equal(gd.stroke(const, -2), const)
    dot = np.zeros((5, 5), F32)
    dot[0, 0] = 1.0
    assert gd.stroke(dot, 1).sum() == 3.0 and gd.stroke(dot, -1).sum() == 0.0


def test_ramp():
    v = np.array([[0.0, 0.3, 0.31, 0.33, 0.5, 0.7, 0.9, 1.0]], F32)
    r = gd.ramp(v, 0.3, 0.7)
    assert r.dtype == F32 and r[0, 0] == 0 and r[0, 1] == 0 and r[0, 2] == 0          # 0.025 < 0.05
    assert r[0, 3] == F32((np.float64(F32(0.33)) - 0.3) / (0.7 - 0.3)) > 0.07 and r[0, 5] == 1 and r[0, 7] == 1
    assert abs(r[0, 4] - 0.5) < 1e-6


def test_area_resample_conserves_the_sum_and_halves_by_pair_means():
    rng = np.random.RandomState(3)
    a = rng.uniform(0, 1, (12, 7)).astype(F32)
    for n_out in (1, 3, 5, 6, 11, 12, 13, 20, 29):
        for axis in (0, 1):
            out = gd.area_resample(a, n_out, axis)
            n_in = a.shape[axis]
            assert out.shape[axis] == n_out and out.dtype == np.float64
            # every output is an average: the sum scales with the number of cells, to rounding
            assert abs(out.sum() * n_in / n_out - a.astype(np.float64).sum()) <= 1e-12 * a.sum(), (n_out, axis)
    a64 = a.astype(np.float64)
    assert np.array_equal(gd.area_resample(a, 6, 0), (a64[0::2] + a64[1::2]) / 2.0)
    assert np.array_equal(gd.area_resample(a, 12, 0), a64) and np.array_equal(gd.area_resample(a, 7, 1), a64)
    assert np.array_equal(gd.area_resample(a, 24, 0), np.repeat(a64, 2, axis=0))     # doubling repeats
    f, fitted = gd.fit(a, 6)
    assert f == 0.5 and fitted.shape == (6, 4)                                        # floor(3.5 + 0.5) = 4
    f, fitted = gd.fit(a[:, :1], 20)
    assert fitted.shape == (20, 2)                                                    # floor(1 * 20 / 12 + 0.5) = 2
    assert gd.fit(a[:1, :1], 5)[1].shape == (5, 5) and gd.fit(a[:, :1], 3)[1].shape == (3, 1)    # max(1, floor(0.75)) = 1


# ---------------------------------------------------------------------------------------------------- the draw streams
def _words(v, generation, seed, salt, quads):
    return philox4x32_10(v, np.arange(quads, dtype=np.uint64), generation & MASK, salt, seed & MASK, (seed >> 32) & MASK).T.reshape(-1)


def test_parameter_stream_order_and_skipped_draws():
    seed, gen, v, G = 0x1234567890, 7, 11, 100
    w = [int(x) for x in _words(v, gen, seed, gd.SALT_P, 3)]
    real = lambda a, b, lo, hi: lo + (hi - lo) * ((np.float64(a >> 5) * 67108864.0 + np.float64(b >> 6)) / 9007199254740992.0)
    b = dict(gd.NEUTRAL, **gd.MNIST_LIKE)
    g, ang, k, sx, sy, n, used = gd.draw_variant(v, gen, seed, G, b)
    assert used == 10 and g == (w[0] * G) >> 32
    assert ang == real(w[1], w[2], -12.0, 12.0) and k == real(w[3], w[4], -0.2, 0.2)
    assert sx == real(w[5], w[6], 0.85, 1.15) and sy == real(w[7], w[8], 0.85, 1.15)
    assert n == -1 + ((w[9] * 3) >> 32) and n in (-1, 0, 1)
    # what is neutral is not drawn, and what follows moves up
    assert gd.draw_variant(v, gen, seed, G, gd.NEUTRAL) == (g, 0.0, 0.0, 1.0, 1.0, 0, 1)
    g2, ang2, k2, sx2, sy2, n2, used = gd.draw_variant(v, gen, seed, G, dict(gd.NEUTRAL, max_shear=0.2, min_stroke=0, max_stroke=2))
    assert used == 4 and ang2 == 0.0 and k2 == real(w[1], w[2], -0.2, 0.2) and (sx2, sy2) == (1.0, 1.0) and n2 == (w[3] * 3) >> 32
    g3, _, _, sx3, sy3, n3, used = gd.draw_variant(v, gen, seed, G, dict(gd.NEUTRAL, max_scale=1.5))
    assert used == 5 and sx3 == real(w[1], w[2], 1.0, 1.5) and sy3 == real(w[3], w[4], 1.0, 1.5) and n3 == 0
    # the generation enters through its low 32 bits; variant, seed and generation each change the stream
    assert gd.draw_variant(v, gen + (1 << 32), seed, G, b) == gd.draw_variant(v, gen, seed, G, b)
    for other in ((v + 1, gen, seed), (v, gen + 1, seed), (v, gen, seed + 1)):
        assert gd.draw_variant(*other, G, b)[1] != ang


def test_field_stream_and_the_one_word_uniform():
    assert gd.uniform_of([0])[0] == 2.0 ** -24 - 1.0 and gd.uniform_of([0xFFFFFFFF])[0] == 1.0 - 2.0 ** -24
    assert gd.uniform_of([0xFF])[0] == gd.uniform_of([0])[0] and gd.uniform_of([0x100])[0] == 3 * 2.0 ** -24 - 1.0
    assert gd.uniform_of([0x80000000])[0] == 2.0 ** -24                              # never 0
    seed, gen, v = 99, 3, 5
    u = gd.field_uniforms(v, gen, seed, 5)                                            # 50 elements: 13 quads, two words spare
    w = _words(v, gen, seed, gd.SALT_F, 13)
    assert u.shape == (2, 5, 5) and np.array_equal(u.reshape(-1), gd.uniform_of(w[:50]))
    assert u[1, 2, 3] == gd.uniform_of([w[25 + 2 * 5 + 3]])[0]
    assert np.abs(u).max() < 1.0 and not (u == 0).any()
    assert not np.array_equal(u, gd.field_uniforms(v, gen + 1, seed, 5))
    assert not np.array_equal(_words(v, gen, seed, gd.SALT_P, 13), w)


# ------------------------------------------------------------------------------------------------------------ geometry
def test_geometry_of_a_preset_bank():
    """256 variants of the preset on the base glyphs it is made for: the larger side of every usable box is ink, the box lies
    in the frame, and where no clamp acted the centre of mass is within half a pixel of the frame's middle.  (The fit's second
    threshold can empty an edge row of the fitted box, which then is ink - 1 on its larger side: 1 variant of 2 048 of the
    preset at another seed, none of these 256.)"""
    import multi_mnist as mm
    p = dict(mm.MNIST_LIKE)
    side, ink, od = p.pop("side"), p.pop("ink"), p.pop("od")
    assert p == gd.MNIST_LIKE and (side, ink, od) == (40, 20, 28)
    base, labels = mm.load_base_glyphs(side)
    assert base.shape == (1797, side * side) and base.dtype == F32 and base.min() >= 0.0 and base.max() <= 1.0 and len(labels) == 1797
    out = gd.distort_bank(base.reshape(-1, side, side), 256, od, ink, seed=5, **p)
    ok = out["status"] == 0
    print("status counts %s" % np.bincount(out["status"], minlength=3))
    assert ok.sum() >= 250
    free = 0
    for v in np.nonzero(ok)[0]:
        x0, y0, w, h = (int(t) for t in out["bank_crops"][v])
        assert max(h, w) == ink, (v, h, w)
        assert 0 <= x0 and x0 + w <= od and 0 <= y0 and y0 + h <= od
        frame = out["bank"][v].reshape(od, od).astype(np.float64)
        assert gd.box_of(frame) == (x0, y0, w, h) and frame.max() <= 1.0
        ys, xs = np.mgrid[0:od, 0:od]
        cy, cx = (frame * ys).sum() / frame.sum(), (frame * xs).sum() / frame.sum()
        if 0 < y0 < od - h:
            assert abs(cy - (od - 1) / 2.0) <= 0.5, (v, cy)
            free += 1
        if 0 < x0 < od - w:
            assert abs(cx - (od - 1) / 2.0) <= 0.5, (v, cx)
            free += 1
    assert free >= 256                                                               # the check did run
    assert not out["bank"][~ok].any() and not out["bank_crops"][~ok].any()
    assert set(np.unique(out["params"][:, 6])) == {-1.0, 0.0, 1.0}
