"""The numpy restatement of air_glyph_jitter (tests/glyph_jitter_cases.py) against scipy.ndimage itself -- the arithmetic the
kernel states is scipy's affine_transform / rotate at order 5 -- and its draw stream and status values.  No GPU: what the
kernel computes is compared with this restatement, bit for bit, in tests/test_gpu_glyph_jitter.py.

Pass rule against scipy: the final glyph of every variant has scipy's shape and its pixels are scipy's or the neighbouring
float32.  (Before the threshold the two agree to a few 1e-14; scipy's own matrix products may contract where the kernel and
the restatement round every operation.)  A value within 1e-6 of the 0.05 threshold could fall on either side of it for such
a difference: the seeds are chosen so that scipy has none, and the test asserts it."""
import numpy as np
import pytest
import scipy.ndimage as scipy_ndimage

import glyph_jitter_cases as gj
import scene_source_cases as sc

SCALE, ANGLE = gj.SCALE, dict(min_ang=-20.0, max_ang=20.0)
BOTH = dict(SCALE, **ANGLE)


def _standin():
    import multi_mnist as mm
    glyphs, _, source = mm.load_glyphs()
    return glyphs[:64].reshape(64, mm.IMAGE_SIZE, mm.IMAGE_SIZE)


def _glyph_set(name):
    g = {"ragged": sc.ragged_glyphs, "thin": gj.thin_glyphs, "standin": _standin}[name]()
    return g, sc.crop_boxes(g)


@pytest.mark.parametrize("name,V,seed,bounds", [
    ("ragged", 48, 1, SCALE), ("ragged", 48, 2, ANGLE), ("ragged", 48, 3, BOTH),
    ("thin", 40, 4, SCALE), ("thin", 40, 5, ANGLE), ("thin", 40, 6, BOTH),
    ("standin", 16, 7, SCALE), ("standin", 16, 8, ANGLE), ("standin", 24, 9, BOTH)],
    ids=lambda v: v if isinstance(v, str) else None)
def test_restatement_is_scipy(name, V, seed, bounds):
    """280 variants in all: the 8 x 8 rectangles of the scene tests, 64 glyphs of the stand-in set (28 x 28), and crops of
    1 x k, k x 1, 2 x 2 and one pixel (the n = 1 line, the mirror at n = 2, a plane where only coordinate 0 is inside)"""
    glyphs, crops = _glyph_set(name)
    od = 64
    out = gj.jitter_bank(glyphs, crops, V, od, seed, 0, **bounds)
    raws = []
    ref = gj.scipy_bank(glyphs, crops, V, seed, 0, bounds, raws)
    near = sum(int((np.abs(r.astype(np.float64) - 0.05) < 1e-6).sum()) for r in raws)
    assert near == 0, "scipy itself has %d values within 1e-6 of the threshold: choose another seed" % near
    exact = 0
    for v, r in enumerate(ref):
        if r is None:
            assert out["status"][v] == 1 and not out["bank_crops"][v].any() and not out["bank"][v].any(), v
            continue
        assert out["status"][v] == 0, v
        x0, y0, w, h = out["bank_crops"][v]
        assert (x0, y0, h, w) == (0, 0) + r.shape, (v, out["bank_crops"][v], r.shape)
        frame = out["bank"][v].reshape(od, od)
        assert gj.adjacent_or_equal(frame[:h, :w], r), v
        exact += np.array_equal(frame[:h, :w], r)
        assert not frame[h:].any() and not frame[:, w:].any()
    print("%s %s: %d variants, %d empty, %d of the others equal scipy in every bit" % (
        name, sorted(bounds), V, sum(r is None for r in ref), exact))
    if name != "thin":
        assert all(r is not None for r in ref)
    else:                                             # (a rotation wipes out some of the thin glyphs; a scale alone need not)
        assert any(r is not None for r in ref) and ("min_ang" not in bounds or any(r is None for r in ref))


def test_prefilter_is_scipys_spline_filter():
    """the coefficients themselves, on lines of 1, 2, 3 and more elements, to a few ulp of scipy's (whose z^(n-1) is pow)"""
    rng = np.random.RandomState(0)
    for shape in ((1, 1), (1, 6), (5, 1), (2, 2), (2, 7), (3, 3), (12, 9), (28, 28)):
        a = rng.rand(*shape).astype(np.float32)
        ref = scipy_ndimage.spline_filter(a.astype(np.float64), order=5, mode="mirror", output=np.float64)
        assert np.allclose(gj.prefilter(a), ref, rtol=0, atol=1e-13 * max(1.0, np.abs(ref).max())), shape
    assert np.array_equal(gj.prefilter(np.float32([[0.75]])), [[0.75]])              # n = 1 both ways: left alone


def test_rotation_geometry_is_scipys():
    for (h, w), ang in (((5, 7), 17.0), ((1, 6), -33.5), ((8, 8), 45.0), ((3, 1), 90.0), ((48, 48), 45.0)):
        c, s = gj.cosdg_sindg(ang)
        OH, OW, _, _ = gj.rotate_geometry(h, w, c, s)
        assert (OH, OW) == scipy_ndimage.rotate(np.ones((h, w), np.float32), ang, order=0).shape, (h, w, ang)
    assert gj.rotate_geometry(48, 48, *gj.cosdg_sindg(45.0))[0] == 68 > gj.MAX_ROTATED


def test_draw_stream():
    """word j & 3 of quad j >> 2; draw order glyph, new_width, new_height, angle; a neutral jitter takes no words; the real is
    53 bits of two words"""
    from oracle.philox_ref import philox4x32_10
    v, gen, seed = 7, (1 << 32) + 9, (5 << 32) + 11
    words = [int(philox4x32_10(v, j >> 2, 9, gj.SALT, 11, 5)[j & 3]) for j in range(7)]
    d = gj.Draws(v, gen, seed)
    assert [d.next() for _ in range(7)] == words
    real = lambda a, b, lo, hi: lo + (hi - lo) * (((a >> 5) * 2 ** 26 + (b >> 6)) / 2.0 ** 53)
    G = 12
    g, nw, nh, ang, scaled, rotated = gj.draw_variant(v, gen, seed, G, dict(gj.NEUTRAL, **BOTH))
    assert (scaled, rotated) == (True, True) and g == (words[0] * G) >> 32
    assert nw == real(words[1], words[2], 0.8, 1.25) and nh == real(words[3], words[4], 0.8, 1.25)
    assert ang == real(words[5], words[6], -20.0, 20.0)
    # rotation only: the angle takes the words the scale would have taken; scale only: no angle; neutral: the glyph alone
    g2, nw2, nh2, ang2, scaled2, rotated2 = gj.draw_variant(v, gen, seed, G, dict(gj.NEUTRAL, **ANGLE))
    assert (g2, nw2, nh2, scaled2, rotated2) == (g, 1.0, 1.0, False, True) and ang2 == real(words[1], words[2], -20.0, 20.0)
    g3, nw3, nh3, ang3, _, rotated3 = gj.draw_variant(v, gen, seed, G, dict(gj.NEUTRAL, **SCALE))
    assert (g3, nw3, nh3, ang3, rotated3) == (g, nw, nh, 0.0, False)
    assert gj.draw_variant(v, gen, seed, G, gj.NEUTRAL)[:4] == (g, 1.0, 1.0, 0.0)
    # one bound away from neutral is enough to draw, and the bound that is still neutral is drawn too
    one = gj.draw_variant(v, gen, seed, G, dict(gj.NEUTRAL, max_h=1.5))
    assert one[1] == 1.0 and one[2] == real(words[3], words[4], 1.0, 1.5) and one[4]
    # the 53-bit real: 0 at the all-zero words, 1 - 2^-53 at the all-one words, every bit of (a >> 5, b >> 6) counts
    class Fixed(gj.Draws):
        def __init__(self, *w):
            self.words, self.j = np.asarray(w, np.uint32), 0
    assert Fixed(0, 0).real(2.0, 3.0) == 2.0 and Fixed(31, 63).real(2.0, 3.0) == 2.0
    assert Fixed(0xFFFFFFFF, 0xFFFFFFFF).real(0.0, 1.0) == 1.0 - 2.0 ** -53
    assert Fixed(0, 64).real(0.0, 1.0) == 2.0 ** -53 and Fixed(32, 0).real(0.0, 1.0) == 2.0 ** -27
    assert all(0 <= gj.Draws(k, 0, 3).index(5) < 5 for k in range(20))


def test_the_three_status_values():
    """0: a plain glyph; 1: 0.06 pixels scaled by 0.5 so that nothing reaches the threshold; 2: a full 8 x 8 glyph at scale 1.5
    and 45 degrees, whose box cannot fit od = 8 -- and a plane that leaves its limit.

    (For status 1 a SINGLE 0.06 pixel does not do: its crop is 1 x 1, output pixel (0, 0) samples coordinate (0, 0), and an
    interpolating spline returns the sample there -- scipy keeps the 0.06 as well, asserted below.  Two 0.06 pixels on the
    anti-diagonal of a 2 x 2 crop do: at scale 0.5 the output samples coordinates 0, 2, 4, 6, of which only (0, 0) is inside,
    and that corner of the crop is empty.)"""
    half = dict(min_w=0.5, max_w=0.5, min_h=0.5, max_h=0.5)
    dot = np.zeros((1, 8, 8), np.float32)
    dot[0, 3, 4] = 0.06
    kept = scipy_ndimage.affine_transform(dot[0, 3:4, 4:5], np.diag([2.0, 2.0]), output_shape=(4, 4), order=5)
    out = gj.jitter_bank(dot, sc.crop_boxes(dot), 1, 8, 1, **half)
    assert kept[0, 0] == np.float32(0.06) and np.count_nonzero(kept) == 1
    assert out["status"][0] == 0 and np.array_equal(out["bank_crops"][0], (0, 0, 1, 1)) and out["bank"][0, 0] == np.float32(0.06)
    dot[0, 3, 4], dot[0, 3, 5], dot[0, 4, 4] = 0.0, 0.06, 0.06
    assert scipy_ndimage.affine_transform(dot[0, 3:5, 4:6], np.diag([2.0, 2.0]), output_shape=(4, 4), order=5).max() < 0.05
    out = gj.jitter_bank(dot, sc.crop_boxes(dot), 4, 8, 1, **half)
    assert (out["status"] == 1).all() and not out["bank"].any() and not out["bank_crops"].any()
    assert np.array_equal(out["params"][:, :3], np.tile([0.5, 0.5, 0.0], (4, 1))) and not out["source"].any()
    full = np.ones((1, 8, 8), np.float32)
    big = dict(min_w=1.5, max_w=1.5, min_h=1.5, max_h=1.5, min_ang=45.0, max_ang=45.0)
    out = gj.jitter_bank(full, sc.crop_boxes(full), 4, 8, 1, **big)
    assert (out["status"] == 2).all() and not out["bank"].any() and not out["bank_crops"].any()
    ok = gj.jitter_bank(full, sc.crop_boxes(full), 4, 32, 1, **big)                 # the same variants fit od = 32
    assert (ok["status"] == 0).all() and (ok["bank_crops"][:, 2:] > 12).all() and (ok["bank_crops"][:, 2:] <= 32).all()
    assert np.array_equal(ok["params"][:, 3:5], np.tile(gj.cosdg_sindg(45.0), (4, 1)))
    plain = gj.jitter_bank(full, sc.crop_boxes(full), 2, 8, 1)                      # neutral: the crop itself
    assert (plain["status"] == 0).all() and (plain["bank"] == 1).all() and np.array_equal(plain["bank_crops"][0], (0, 0, 8, 8))
    assert gj.scale_stage(full[0], 8, 6.25, 1.0)[0] == 2 and gj.scale_stage(full[0], 8, 6.0, 6.0)[0] == 0     # 50 > 48 >= 48
    assert gj.rotate_stage(np.ones((48, 48), np.float32), *gj.cosdg_sindg(45.0))[0] == 2                      # 68 > 64
    bad_box = gj.jitter_bank(full, np.int32([[4, 0, 8, 8]]), 2, 8, 1)              # a crop box that leaves its frame
    assert (bad_box["status"] == 1).all() and not bad_box["bank"].any()


def test_the_gpu_cases_reach_what_they_are_for():
    """the inputs of tests/test_gpu_glyph_jitter.py: the crowded case has all three status values, and the committed scipy
    fixture is what tests/golden/make_glyph_jitter.py writes with the installed scipy"""
    import os
    glyphs, crops = gj.gpu_glyphs("mixed")
    _, od, seed, gen, bounds = gj.GPU_CASES["crowded"]
    st = gj.jitter_bank(glyphs, crops, gj.GPU_V, od, seed, gen, **bounds)["status"]
    assert (np.bincount(st, minlength=3) > 0).all()
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyph_jitter_scipy.npz"))
    name = "both"
    glyph_set, _, seed, gen, bounds = gj.GPU_CASES[name]
    glyphs, crops = gj.gpu_glyphs(glyph_set)
    finals = gj.scipy_bank(glyphs, crops, gj.GPU_V, seed, gen, bounds)
    assert np.array_equal(fx[name + "_shapes"], [(0, 0) if f is None else f.shape for f in finals])
    assert gj.adjacent_or_equal(fx[name + "_pixels"], np.concatenate([f.reshape(-1) for f in finals if f is not None]))
