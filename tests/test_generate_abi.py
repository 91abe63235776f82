"""CPU-side checks of the generation entry points (air_philox_fill, air_scene_records, air_render): exported and bound,
argument and limit errors reported on the host before any launch, ctypes mirrors equal to the C layout."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("air_philox_fill", "air_scene_records", "air_render")


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("air_build", os.path.join(ROOT, "tf-attend-infer-repeat_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from air import _hip
    _hip.lib()
    return _hip


def _host_ptr(keep, nbytes=256):
    """a 16-byte aligned non-null address (never dereferenced: every call below returns before a launch)"""
    buf = (C.c_char * (nbytes + 16))()
    keep.append(buf)
    base = C.addressof(buf)
    return C.c_void_p(base + (-base) % 16)


def test_generation_entry_points_are_exported_and_bound(H):
    raw = C.CDLL(H.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in H.EXPORTED_SYMBOLS
        fn = getattr(H.lib(), name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    assert H.lib().air_abi_version() == H.ABI_VERSION == 6


def test_descriptor_layout_matches_c(H, tmp_path):
    """sizeof / offsetof from a C compile of the header == the ctypes mirrors (as tests/test_abi.py does for the others)."""
    fields = {"air_scene_records_t": (H.SceneRecords, [f[0] for f in H.SceneRecords._fields_]),
              "air_render_t": (H.Render, [f[0] for f in H.Render._fields_])}
    body, exp = [], []
    for cname, (cls, names) in fields.items():
        body.append('printf("%%zu\\n", sizeof(%s));' % cname)
        exp.append(C.sizeof(cls))
        for n in names:
            body.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, n))
            exp.append(getattr(cls, n).offset)
    body.append('printf("%d\\n", AIR_MAX_STEPS);')
    exp.append(H.MAX_STEPS)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "air_hip.h"\nint main(){%s return 0;}' % "".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == exp, (got, exp)


def test_philox_fill_argument_errors(H):
    lib, keep = H.lib(), []
    p = _host_ptr(keep)
    assert lib.air_philox_fill(None, 16, None, 16, 1, 0, None) == -1          # null buffers
    assert lib.air_philox_fill(p, 16, None, 16, 1, 0, None) == -1
    assert lib.air_philox_fill(None, 16, p, 0, 1, 0, None) == -1
    assert lib.air_philox_fill(p, 0, p, 0, 1, 0, None) == -1                  # nothing to fill
    assert lib.air_philox_fill(p, -4, p, 16, 1, 0, None) == -1                # negative counts
    assert lib.air_philox_fill(p, 16, p, -1, 1, 0, None) == -1


def _records(H, keep, **kw):
    p = lambda: _host_ptr(keep)  # noqa: E731
    a = H.SceneRecords(p(), p(), p(), p(), p(), p(), p(), None, 4, 3, 50, 50, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_scene_records_argument_and_limit_errors(H):
    lib, keep = H.lib(), []
    assert lib.air_scene_records(None, None) == -1
    assert lib.air_scene_records(C.byref(H.SceneRecords()), None) == -1
    for f in ("scale_src", "shift_src", "z_src", "pres_src", "dyn", "att", "z"):
        assert lib.air_scene_records(C.byref(_records(H, keep, **{f: None})), None) == -1, f
    for f in ("B", "N", "Z"):
        for v in (0, -1):
            assert lib.air_scene_records(C.byref(_records(H, keep, **{f: v})), None) == -1, (f, v)
    assert lib.air_scene_records(C.byref(_records(H, keep, ldz=49)), None) == -1        # row stride below Z
    assert lib.air_scene_records(C.byref(_records(H, keep, N=H.MAX_STEPS + 1)), None) == -2
    assert lib.air_scene_records(C.byref(_records(H, keep, N=H.MAX_STEPS + 1, given=1)), None) == -2
    a = _records(H, keep)
    a.att = a.att + 4                                                                    # records are written 16 bytes at a time
    assert lib.air_scene_records(C.byref(a), None) == -3


def _render(H, keep, **kw):
    p = lambda: _host_ptr(keep)  # noqa: E731
    a = H.Render(p(), p(), p(), p(), 4, 3, 50, 28)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_render_argument_and_limit_errors(H):
    lib, keep = H.lib(), []
    assert lib.air_render(None, None) == -1
    assert lib.air_render(C.byref(H.Render()), None) == -1
    for f in ("vrec", "att", "canvas", "num_digits"):
        assert lib.air_render(C.byref(_render(H, keep, **{f: None})), None) == -1, f
    for f, bad in (("B", (0, -1)), ("N", (0, -1)), ("C", (1, 0, -3)), ("w", (1, 0, -3))):
        for v in bad:
            assert lib.air_render(C.byref(_render(H, keep, **{f: v})), None) == -1, (f, v)
    assert lib.air_render(C.byref(_render(H, keep, N=H.MAX_STEPS + 1)), None) == -2
    # the taps and windows of one image must fit the 160 KB of LDS: 16 steps of a 256 x 256 canvas do not
    assert lib.air_render(C.byref(_render(H, keep, N=16, C=256, w=28)), None) == -2


def test_model_exposes_the_generation_methods(H):
    from air import air_model as am
    for name in ("generate", "decode", "set_generate_noise"):
        assert callable(getattr(am.AIRModel, name))
    assert set(am.GeneratedScenes.__slots__) >= {"canvas", "num_digits", "scales", "shifts", "z_pres", "latents", "windows", "st_back"}
