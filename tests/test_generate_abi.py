"""CPU-side checks of the generation entry points (air_philox_fill, air_scene_records, air_render): exported and bound,
argument and limit errors reported on the host before any launch."""
import ctypes as C

import pytest

import abi_check as abi


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def test_philox_fill_argument_errors(H):
    lib, p = H.lib(), abi.host_ptr()
    assert lib.air_philox_fill(None, 16, None, 16, 1, 0, None) == -1          # null buffers
    assert lib.air_philox_fill(p, 16, None, 16, 1, 0, None) == -1
    assert lib.air_philox_fill(None, 16, p, 0, 1, 0, None) == -1
    assert lib.air_philox_fill(p, 0, p, 0, 1, 0, None) == -1                  # nothing to fill
    assert lib.air_philox_fill(p, -4, p, 16, 1, 0, None) == -1                # negative counts
    assert lib.air_philox_fill(p, 16, p, -1, 1, 0, None) == -1


def _records(H, **kw):
    p = abi.host_ptr
    a = H.SceneRecords(p(), p(), p(), p(), p(), p(), p(), None, 4, 3, 50, 50, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_scene_records_argument_and_limit_errors(H):
    lib = H.lib()
    assert lib.air_scene_records(None, None) == -1
    assert lib.air_scene_records(C.byref(H.SceneRecords()), None) == -1
    for f in ("scale_src", "shift_src", "z_src", "pres_src", "dyn", "att", "z"):
        assert lib.air_scene_records(C.byref(_records(H, **{f: None})), None) == -1, f
    for f in ("B", "N", "Z"):
        for v in (0, -1):
            assert lib.air_scene_records(C.byref(_records(H, **{f: v})), None) == -1, (f, v)
    assert lib.air_scene_records(C.byref(_records(H, ldz=49)), None) == -1        # row stride below Z
    assert lib.air_scene_records(C.byref(_records(H, N=H.MAX_STEPS + 1)), None) == -2
    assert lib.air_scene_records(C.byref(_records(H, N=H.MAX_STEPS + 1, given=1)), None) == -2
    a = _records(H)
    a.att = a.att + 4                                                                    # records are written 16 bytes at a time
    assert lib.air_scene_records(C.byref(a), None) == -3


def _render(H, **kw):
    p = abi.host_ptr
    a = H.Render(p(), p(), p(), p(), 4, 3, 50, 28)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_render_argument_and_limit_errors(H):
    lib = H.lib()
    assert lib.air_render(None, None) == -1
    assert lib.air_render(C.byref(H.Render()), None) == -1
    for f in ("vrec", "att", "canvas", "num_digits"):
        assert lib.air_render(C.byref(_render(H, **{f: None})), None) == -1, f
    for f, bad in (("B", (0, -1)), ("N", (0, -1)), ("C", (1, 0, -3)), ("w", (1, 0, -3))):
        for v in bad:
            assert lib.air_render(C.byref(_render(H, **{f: v})), None) == -1, (f, v)
    assert lib.air_render(C.byref(_render(H, N=H.MAX_STEPS + 1)), None) == -2
    # the taps and windows of one image must fit the 160 KB of LDS: 16 steps of a 256 x 256 canvas do not
    assert lib.air_render(C.byref(_render(H, N=16, C=256, w=28)), None) == -2


def test_model_exposes_the_generation_methods(H):
    from air import air_model as am
    for name in ("generate", "decode", "set_generate_noise"):
        assert callable(getattr(am.AIRModel, name))
    assert set(am.GeneratedScenes.__slots__) >= {"canvas", "num_digits", "scales", "shifts", "z_pres", "latents", "windows", "st_back"}
