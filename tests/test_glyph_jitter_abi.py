"""CPU-side checks of the glyph bank (include/air_hip.h: air_glyph_jitter*, multi_mnist.DeviceGlyphBank): every refusal is
answered on the host before any launch, in the stated order (an invalid size before a limit, a limit before a null pointer),
with host pointers that are never dereferenced; the LDS query; the Python classes' refusals.  (What the kernel computes:
tests/test_gpu_glyph_jitter.py; the descriptor's layout and the signatures: tests/test_abi.py, with every other.)"""
import ctypes as C

import numpy as np
import pytest

import abi_check as abi
import scene_source_cases as sc

POINTERS = ("glyphs", "crops", "bank", "bank_crops", "source", "params", "status")      # counter is optional


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _desc(H, ptrs=True, **override):
    """a descriptor that passes every check (the model's shapes, the issue's jitter); ptrs: the required pointers set to a
    host address the checks never follow"""
    a = H.GlyphJitter()
    a.V, a.G, a.gd, a.od = 4096, 1797, 28, 32
    a.min_w, a.max_w, a.min_h, a.max_h, a.min_ang, a.max_ang = 0.9, 1.1, 0.9, 1.1, -15.0, 15.0
    if ptrs:
        for k in POINTERS:
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_the_limit_is_the_documented_one(H):
    assert H.JITTER_MAX_PLANE == 48 and H.SCENE_MAX_GLYPH == 32


def test_a_valid_descriptor_passes_the_checks(H):
    """prepare is the checks alone: 0, and nothing was launched (no device here); counter may be null"""
    assert H.lib().air_glyph_jitter_prepare(C.byref(_desc(H))) == 0
    assert H.lib().air_glyph_jitter_prepare(C.byref(_desc(H, counter=abi.host_ptr().value))) == 0
    neutral = _desc(H, min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0)
    assert H.lib().air_glyph_jitter_prepare(C.byref(neutral)) == 0
    # the limits themselves pass: 32 * 1.5 = 48, +-180 degrees, gd = od = 32, one variant of one glyph
    edge = _desc(H, V=1, G=1, gd=32, od=32, min_w=1.0 / 32, max_w=1.5, min_h=1.0 / 32, max_h=1.5, min_ang=-180.0, max_ang=180.0)
    assert H.lib().air_glyph_jitter_prepare(C.byref(edge)) == 0
    # just inside what the refusals of the next test are just outside of
    for kw in (dict(gd=8, od=8, min_h=0.125), dict(max_w=48.9 / 28), dict(min_ang=-180.0, max_ang=180.0)):
        assert H.lib().air_glyph_jitter_prepare(C.byref(_desc(H, **kw))) == 0, kw


def test_every_refusal_comes_before_a_launch(H):
    """(only refused descriptors go to air_glyph_jitter itself: one that passes would launch on host pointers)"""
    lib = H.lib()
    inf, nan = float("inf"), float("nan")
    for fn in (lambda a: lib.air_glyph_jitter(C.byref(a), None), lambda a: lib.air_glyph_jitter_prepare(C.byref(a))):
        for k in ("V", "G", "gd", "od"):
            assert fn(_desc(H, **{k: 0})) == H.EINVAL and fn(_desc(H, **{k: -3})) == H.EINVAL, k
        assert fn(_desc(H, gd=28, od=27)) == H.EINVAL                               # od < gd
        for k in ("min_w", "max_w", "min_h", "max_h", "min_ang", "max_ang"):
            assert fn(_desc(H, **{k: nan})) == H.EINVAL and fn(_desc(H, **{k: inf})) == H.EINVAL, k
            assert fn(_desc(H, **{k: -inf})) == H.EINVAL, k
        assert fn(_desc(H, min_w=1.2, max_w=1.1)) == H.EINVAL and fn(_desc(H, min_h=1.2, max_h=1.1)) == H.EINVAL
        assert fn(_desc(H, min_ang=20.0, max_ang=15.0)) == H.EINVAL
        assert fn(_desc(H, min_w=0.0)) == H.EINVAL and fn(_desc(H, min_h=-0.5)) == H.EINVAL
        assert fn(_desc(H, min_w=-2.0, max_w=-1.0)) == H.EINVAL
        assert fn(_desc(H, min_h=0.03)) == H.EINVAL and fn(_desc(H, min_w=0.03)) == H.EINVAL      # int(28 * 0.03) = 0
        assert fn(_desc(H, gd=8, od=8, min_h=0.124)) == H.EINVAL                    # int(8 * 0.124) = 0
        # limits
        assert fn(_desc(H, gd=33, od=33)) == H.ELIMIT and fn(_desc(H, od=33)) == H.ELIMIT
        assert fn(_desc(H, max_h=1.75)) == H.ELIMIT and fn(_desc(H, max_w=1.75)) == H.ELIMIT       # int(28 * 1.75) = 49
        assert fn(_desc(H, max_w=1e300)) == H.ELIMIT
        assert fn(_desc(H, max_ang=180.5)) == H.ELIMIT and fn(_desc(H, min_ang=-181.0)) == H.ELIMIT
        # the order: an invalid size before a limit, a limit before a null pointer, a null pointer before the alignment
        assert fn(_desc(H, V=0, od=33)) == H.EINVAL
        assert fn(_desc(H, min_w=nan, max_ang=200.0)) == H.EINVAL
        assert fn(_desc(H, min_w=0.03, max_h=1.75)) == H.EINVAL
        assert fn(_desc(H, ptrs=False, od=33)) == H.ELIMIT and fn(_desc(H, ptrs=False, max_ang=200.0)) == H.ELIMIT
        assert fn(_desc(H, ptrs=False)) == H.EINVAL
        assert fn(_desc(H, glyphs=None, crops=abi.host_ptr().value + 4)) == H.EINVAL
    assert lib.air_glyph_jitter(None, None) == H.EINVAL and lib.air_glyph_jitter_prepare(None) == H.EINVAL


def test_each_required_pointer_is_required_and_aligned(H):
    """prepare alone from here on: with every pointer set, air_glyph_jitter itself would launch"""
    prepare = H.lib().air_glyph_jitter_prepare
    for missing in POINTERS:
        assert prepare(C.byref(_desc(H, **{missing: None}))) == H.EINVAL, missing
    p = abi.host_ptr().value
    for k in ("crops", "bank_crops"):                                             # a crop box is one 16-byte access
        assert prepare(C.byref(_desc(H, **{k: p + 4}))) == H.EALIGN and prepare(C.byref(_desc(H, **{k: p + 8}))) == H.EALIGN, k
    assert prepare(C.byref(_desc(H, params=p + 4))) == H.EALIGN and prepare(C.byref(_desc(H, params=p + 8))) == 0
    assert prepare(C.byref(_desc(H, glyphs=p + 4, bank=p + 4, source=p + 4, status=p + 4))) == 0


def test_lds_query(H):
    lds = H.lib().air_glyph_jitter_lds
    want = 8 * 48 * 48 + 4 * 64 * 64 + 32                   # coefficients of a 48 x 48 plane, a 64 x 64 image, two boxes
    for gd, od in ((28, 32), (8, 16), (8, 8), (1, 1), (32, 32), (7, 9)):
        assert lds(gd, od) == want == 34848, (gd, od)
    assert want <= 48 * 1024                                 # no grant is needed: prepare has nothing to do but the checks
    assert lds(0, 8) == H.EINVAL and lds(8, 0) == H.EINVAL and lds(8, 7) == H.EINVAL
    assert lds(33, 33) == H.ELIMIT and lds(8, 33) == H.ELIMIT and lds(0, 33) == H.EINVAL


def test_python_bank_refuses_on_the_host(H):
    import multi_mnist as mm
    glyphs = sc.ragged_glyphs().reshape(12, 64)
    for kw, code in ((dict(min_w=1.2, max_w=1.1), "-1"), (dict(min_h=0.0), "-1"), (dict(max_ang=float("nan")), "-1"),
                     (dict(od=7), "-1"), (dict(od=33), "-2"), (dict(max_h=6.2), "-2"), (dict(min_ang=-200.0), "-2"),
                     (dict(variants=0), "-1")):
        args = dict(variants=16, od=16)
        args.update(kw)
        with pytest.raises(H.AirHipError, match="air_glyph_jitter_prepare failed with code %s" % code):
            mm.DeviceGlyphBank(glyphs, **args)
    with pytest.raises(ValueError, match="empty"):
        mm.DeviceGlyphBank(np.zeros((2, 64), np.float32), 16, od=16, min_w=0.9)
    with pytest.raises(ValueError, match=">= 0"):
        mm.DeviceGlyphBank(-glyphs, 16, od=16, min_w=0.9)
    with pytest.raises(ValueError, match="gd \\* gd"):
        mm.DeviceGlyphBank(glyphs[:, :63], 16, od=16, min_w=0.9)
    with pytest.raises(TypeError):
        mm.DeviceGlyphBank(glyphs, 16, shear=0.1)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):                  # valid arguments: what is missing is a GPU
        mm.DeviceGlyphBank(glyphs, 16, od=16, min_w=0.9, device="cpu")


def test_scene_source_still_refuses_jitter_keywords(H):
    """the jitter is the bank's: the scene source's own keywords stay refused, and the message still names the host generator"""
    import multi_mnist as mm
    glyphs = sc.ragged_glyphs().reshape(12, 64)
    with pytest.raises(NotImplementedError, match="Generator.multi_image") as e:
        mm.DeviceSceneSource(glyphs, 4, None, None, min_w=0.8)
    assert "DeviceGlyphBank" in str(e.value)
    for kw in (dict(max_h=1.2), dict(min_ang=-10.0), dict(max_ang=15.0)):
        with pytest.raises(NotImplementedError, match="Generator.multi_image"):
            mm.DeviceSceneSource(glyphs, 4, None, None, **kw)
    with pytest.raises(NotImplementedError, match="Generator.multi_image"):
        mm.DeviceSceneSource(glyphs, 4, None, None, use_pixel_overlap=False)
    assert mm.JITTER_NEUTRAL == dict(min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0)
