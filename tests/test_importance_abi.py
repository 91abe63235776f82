"""CPU-side checks of the importance-weighted bound (include/air_hip.h: air_importance_*, air/metrics.py ImportanceBound,
training.py --importance-samples): every refusal is answered on the host before any launch, in the stated order, with host
pointers that are never dereferenced -- no descriptor that would launch is passed; the workspace query; the constants of the
binding, the header and the cases module; the Python class's refusals; the driver's refusal of a bad sample count.  (What
the kernels compute: tests/test_gpu_importance.py; the descriptors' layouts and the signatures: tests/test_abi.py.)"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import abi_check as abi
import importance_cases as ic

LOGW_REQUIRED = ("att", "out7", "ml", "z", "eps_scale", "eps_shift", "eps_z", "rec_loss", "run_digits", "dyn", "logw", "digits")
FOLD_REQUIRED = ("logw", "digits", "counts", "sums")
FOLD_OPTIONAL = ("targets", "bound", "ess", "map")


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _logw(H, ptrs=True, **override):
    """a descriptor that would pass every check (so it is only ever sent with something wrong)"""
    a = H.Importance()
    a.T, a.B, a.k, a.Z, a.ldz, a.K = 3, 8, 8, 50, 52, 16
    if ptrs:
        for key in LOGW_REQUIRED + ("terms",):
            setattr(a, key, abi.host_ptr().value)
    for key, v in override.items():
        setattr(a, key, v)
    return a


def _fold(H, ptrs=True, **override):
    a = H.ImportanceFold()
    a.T, a.B, a.k, a.K = 3, 8, 8, 16
    if ptrs:
        for key in FOLD_REQUIRED + FOLD_OPTIONAL:
            setattr(a, key, abi.host_ptr().value)
    for key, v in override.items():
        setattr(a, key, v)
    return a


def test_the_limits_and_the_layout_are_the_documented_ones(H):
    assert (H.MAX_STEPS, H.IW_MAX_SAMPLES, H.IW_MAX_Z) == (16, 64, 256) == (ic.MAX_STEPS, ic.MAX_SAMPLES, ic.MAX_Z)
    assert H.LOC_GROUP == ic.GROUP == 256                                  # the summation group is air_localization's
    num = abi.compile_numbers()
    for name in ("TERM_REC", "TERM_Z_PRES", "TERM_SCALE", "TERM_SHIFT", "TERM_WHAT", "TERMS", "IMAGES", "SCORED", "DEGENERATE",
                 "MAP_CORRECT", "SPLIT", "COUNTS", "BOUND", "ELBO", "ESS", "ENTROPY", "SUMS", "MAX_SAMPLES", "MAX_Z"):
        assert num.values["AIR_IW_" + name] == getattr(ic, name) == getattr(H, "IW_" + name), name
    for name in ("ATT_S", "ATT_X", "ATT_Y", "ATT_KL_Z", "ATT_MASK_PREV", "ATT_MASK", "ATT_STRIDE", "OUT_STRIDE", "DYN_COUNT"):
        assert num.values["AIR_" + name] == getattr(ic, name) == getattr(H, name), name
    assert (ic.DYN_SCALE, ic.DYN_SHIFT, ic.DYN_VAE) == ((H.DYN_SCALE_PM, H.DYN_SCALE_PV, H.DYN_SCALE_PLV),
                                                        (H.DYN_SHIFT_PM, H.DYN_SHIFT_PV, H.DYN_SHIFT_PLV),
                                                        (H.DYN_VAE_PM, H.DYN_VAE_PV, H.DYN_VAE_PLV))
    h = abi.read_header()
    assert h.structs["air_importance_t"] == [f[0] for f in H.Importance._fields_]
    assert h.structs["air_importance_fold_t"] == [f[0] for f in H.ImportanceFold._fields_]
    assert h.prototypes["air_importance_logw"] == ("int", ["const air_importance_t*", "int", "void*"])
    assert h.prototypes["air_importance_fold"] == ("int", ["const air_importance_fold_t*", "void*", "void*"])
    assert h.prototypes["air_importance_fold_workspace_bytes"] == ("int64_t", ["int"] * 4)
    assert abi.check_abi(H) == []
    assert H.lib().air_abi_version() == 6                                  # additive


def test_the_kernels_have_rows_in_the_table_of_kernel_names(H):
    from air import air_model as am
    assert am.KERNEL_NAMES["air_importance_logw"] == "iw_logw_kernel"
    assert am.KERNEL_NAMES["air_importance_fold"] == "iw_image_kernel"


def test_every_logw_refusal_comes_before_a_launch(H):
    lib = H.lib()
    call = lambda a, sample=0: lib.air_importance_logw(C.byref(a), sample, None)      # noqa: E731
    assert lib.air_importance_logw(None, 0, None) == H.EINVAL
    for key in ("T", "B", "k", "Z", "K"):
        assert call(_logw(H, **{key: 0})) == H.EINVAL and call(_logw(H, **{key: -2})) == H.EINVAL, key
    assert call(_logw(H, k=9)) == H.EINVAL                                 # k > B
    assert call(_logw(H, ldz=49)) == H.EINVAL and call(_logw(H, ldz=-1)) == H.EINVAL
    assert call(_logw(H), -1) == H.EINVAL and call(_logw(H), 16) == H.EINVAL
    for key, v in (("T", 17), ("K", 65), ("Z", 257)):
        assert call(_logw(H, **{key: v, "ldz": 0})) == H.ELIMIT, key
    for missing in LOGW_REQUIRED:
        assert call(_logw(H, **{missing: None})) == H.EINVAL, missing
    assert call(_logw(H, ptrs=False)) == H.EINVAL
    # the order: a size before a limit, a limit before a null pointer
    assert call(_logw(H, T=17, Z=0)) == H.EINVAL and call(_logw(H, K=65), 70) == H.EINVAL
    assert call(_logw(H, ptrs=False, T=17)) == H.ELIMIT


def test_every_fold_refusal_comes_before_a_launch(H):
    lib, ws = H.lib(), abi.host_ptr()
    call = lambda a, w=ws: lib.air_importance_fold(C.byref(a), w, None)    # noqa: E731
    assert lib.air_importance_fold(None, ws, None) == H.EINVAL
    for key in ("T", "B", "k", "K"):
        assert call(_fold(H, **{key: 0})) == H.EINVAL and call(_fold(H, **{key: -2})) == H.EINVAL, key
    assert call(_fold(H, k=9)) == H.EINVAL
    assert call(_fold(H, T=17)) == H.ELIMIT and call(_fold(H, K=65)) == H.ELIMIT
    for missing in FOLD_REQUIRED:
        assert call(_fold(H, **{missing: None})) == H.EINVAL, missing
    assert call(_fold(H), None) == H.EINVAL                                # no workspace
    assert call(_fold(H, ptrs=False)) == H.EINVAL
    assert call(_fold(H, T=17, K=0)) == H.EINVAL and call(_fold(H, ptrs=False, K=65)) == H.ELIMIT
    assert call(_fold(H, T=17), None) == H.ELIMIT


def test_the_workspace_query_answers_as_the_entry_point(H):
    q = H.lib().air_importance_fold_workspace_bytes
    for k, groups in ((1, 1), (256, 1), (257, 2), (1000, 4)):
        assert q(3, 1000, k, 16) == groups * ic.SUMS * 8, k
    for bad in ((0, 8, 8, 16), (3, 0, 8, 16), (3, 8, 0, 16), (3, 8, 8, 0), (3, 8, 9, 16)):
        assert q(*bad) == H.EINVAL, bad
    assert q(17, 8, 8, 16) == H.ELIMIT and q(3, 8, 8, 65) == H.ELIMIT and q(17, 8, 0, 16) == H.EINVAL


def _stub(max_steps=3, batch_size=8, device_tensor=None, Z=50):
    return types.SimpleNamespace(max_steps=max_steps, batch_size=batch_size, canvas_size=50, windows_size=28,
                                 vae_latent_dimensions=Z,
                                 input_images=torch.zeros(batch_size, 2500) if device_tensor is None else device_tensor)


def test_python_class_refuses_on_the_host(H):
    from air.metrics import ImportanceBound, _Instrument
    assert ImportanceBound.names() == list(ic.NAMES) == list(ImportanceBound.reported)
    assert issubclass(ImportanceBound, _Instrument) and (ImportanceBound.prefix, ImportanceBound.group) == ("iw_", "importance/")
    for stub, kw in ((_stub(), dict(samples=65)), (_stub(max_steps=17), {}), (_stub(Z=257), {})):
        with pytest.raises(NotImplementedError, match="hold 16, 64 and 256"):
            ImportanceBound(stub, **kw)
    with pytest.raises(ValueError, match="samples"):
        ImportanceBound(_stub(), samples=0)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):           # valid arguments: what is missing is a device tensor
        ImportanceBound(_stub(), samples=4)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        ImportanceBound(_stub(device_tensor=np.zeros((8, 2500), np.float32)))


def test_forward_sampled_is_a_method_of_the_model_and_eager_only():
    import inspect
    from air.air_model import AIRModel
    sig = inspect.signature(AIRModel.forward_sampled)
    assert list(sig.parameters) == ["self", "call", "seed"] and sig.parameters["seed"].default is None
    src = inspect.getsource(AIRModel.forward_sampled)
    assert "_injected_noise" not in src and "_graph" not in src and "global_step" not in src.split('"""')[2]


def test_training_refuses_a_bad_sample_count(tmp_path):
    """parser.error (exit status 2) before anything touches a device or the results folder"""
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "training.py")
    for bad in ("65", "-1"):
        p = subprocess.run([sys.executable, script, "--importance-samples", bad, "-r", str(tmp_path / "out")], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "--importance-samples" in p.stderr, (p.returncode, p.stderr[-400:])
        assert not (tmp_path / "out").exists()
