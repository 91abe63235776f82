"""CPU-side checks of the latent probe (include/air_hip.h: air_latent_probe*, air/metrics.py LatentProbe, air/embeddings.py
probe, training.py --latent-probe): every refusal is answered on the host before any launch, in the stated order, with host
pointers that are never dereferenced -- no descriptor that would launch is passed; the workspace and the splits queries;
the constants of the binding, the header and the cases module; the Python class's refusals; the driver's refusal of a cache
without labels.  (What the kernels compute: tests/test_gpu_latent_probe.py; the descriptor's layout and the signatures:
tests/test_abi.py, with every other.)"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import abi_check as abi
import latent_probe_cases as pc

REQUIRED = ("latents", "labels", "counts", "moments")
OPTIONAL = ("rows", "pred", "neighbours", "neighbour_d2")


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _desc(H, ptrs=True, **override):
    """a descriptor that would pass every check (so it is only ever sent with something wrong)"""
    a = H.LatentProbe()
    a.M, a.Z, a.k, a.classes, a.au_threshold = 100, 50, 5, 10, 0.01
    if ptrs:
        for k in REQUIRED + OPTIONAL:
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_the_limits_and_the_layout_are_the_documented_ones(H):
    assert (H.PROBE_MAX_K, H.PROBE_MAX_CLASSES, H.PROBE_MAX_Z, H.PROBE_MAX_ROWS) == (16, 64, 256, 32768) == \
        (pc.MAX_K, pc.MAX_CLASSES, pc.MAX_Z, pc.MAX_ROWS)
    assert (H.PROBE_QUERY_TILE, H.PROBE_REF_TILE, H.PROBE_MAX_SPLITS, H.PROBE_PASS_ROWS) == \
        (pc.QUERY_TILE, pc.REF_TILE, pc.MAX_SPLITS, pc.PASS_ROWS)
    assert (H.PROBE_ROWS, H.PROBE_VALID, H.PROBE_SCORED, H.PROBE_CORRECT, H.PROBE_ACTIVE_UNITS, H.PROBE_COUNTS) == \
        (pc.ROWS, pc.VALID, pc.SCORED, pc.CORRECT, pc.ACTIVE_UNITS, pc.COUNTS)
    assert H.LOC_GROUP == pc.GROUP == 256                       # the summation group is air_localization's
    num = abi.compile_numbers()
    for name in ("MAX_K", "MAX_CLASSES", "MAX_Z", "MAX_ROWS", "QUERY_TILE", "REF_TILE", "MAX_SPLITS", "PASS_ROWS", "ROWS", "VALID", "SCORED",
                 "CORRECT", "ACTIVE_UNITS", "COUNTS"):
        assert num.values["AIR_PROBE_" + name] == getattr(pc, name) == getattr(H, "PROBE_" + name), name
    assert H.lib().air_abi_version() == 6                       # additive
    assert pc.QUERY_TILE % 64 == 0 and pc.MAX_SPLITS * pc.REF_TILE + 1 <= 600 and pc.REF_TILE % pc.PASS_ROWS == 0


def test_the_kernel_has_a_row_in_the_table_of_kernel_names(H):
    from air import air_model as am
    assert am.KERNEL_NAMES["air_latent_probe"] == "probe_pairs_kernel"


def test_every_refusal_comes_before_a_launch(H):
    lib, ws = H.lib(), abi.host_ptr()
    call = lambda a, w=ws: lib.air_latent_probe(C.byref(a), w, None)      # noqa: E731
    assert lib.air_latent_probe(None, ws, None) == H.EINVAL
    for k in ("M", "Z", "k", "classes"):
        assert call(_desc(H, **{k: 0})) == H.EINVAL and call(_desc(H, **{k: -2})) == H.EINVAL, k
    for au in (-0.01, float("nan"), -float("inf")):
        assert call(_desc(H, au_threshold=au)) == H.EINVAL, au
    for missing in REQUIRED:
        assert call(_desc(H, **{missing: None})) == H.EINVAL, missing
    assert call(_desc(H), None) == H.EINVAL                                # no workspace
    assert call(_desc(H, neighbours=None)) == H.EINVAL and call(_desc(H, neighbour_d2=None)) == H.EINVAL   # exactly one of the two
    assert call(_desc(H, ptrs=False)) == H.EINVAL
    for k, v in (("k", 17), ("classes", 65), ("Z", 257), ("M", 32769)):
        assert call(_desc(H, **{k: v})) == H.ELIMIT, k
    odd = abi.host_ptr().value + 4
    assert call(_desc(H, moments=odd)) == H.EALIGN and call(_desc(H, neighbour_d2=odd)) == H.EALIGN
    assert call(_desc(H), C.c_void_p(odd)) == H.EALIGN
    # the order: a size (the threshold with it) before a limit, a limit before a null pointer, a null pointer before alignment
    assert call(_desc(H, k=17, Z=0)) == H.EINVAL and call(_desc(H, M=32769, au_threshold=-1.0)) == H.EINVAL
    assert call(_desc(H, ptrs=False, k=17)) == H.ELIMIT and call(_desc(H, classes=65), None) == H.ELIMIT
    assert call(_desc(H, moments=odd, labels=None)) == H.EINVAL and call(_desc(H, neighbour_d2=odd, neighbours=None)) == H.EINVAL
    assert call(_desc(H, moments=odd), None) == H.EINVAL


def test_workspace_and_splits_queries_answer_as_the_entry_point(H):
    q, sp = H.lib().air_latent_probe_workspace_bytes, H.lib().air_latent_probe_splits
    pad8 = lambda n: -(-n // 8) * 8                                        # noqa: E731
    for M, Z, k in ((1, 1, 1), (2, 50, 5), (33, 7, 5), (257, 3, 16), (1000, 50, 5), (2000, 50, 5), (32768, 256, 16)):
        n = M * pc.splits(M) * k
        assert sp(M) == pc.splits(M), M
        assert q(M, Z, k) == 8 * n + pad8(4 * n) + pad8(4 * M), (M, Z, k)
    assert [sp(M) for M in (1, 32, 33, 64, 65, 256, 257, 1000)] == [1, 1, 2, 2, 3, 8, 8, 8]
    for bad in ((0, 50, 5), (100, 0, 5), (100, 50, 0), (-1, 50, 5)):
        assert q(*bad) == H.EINVAL, bad
    assert q(32769, 50, 5) == H.ELIMIT and q(100, 257, 5) == H.ELIMIT and q(100, 50, 17) == H.ELIMIT
    assert q(32769, 0, 5) == H.EINVAL                                      # a size before a limit
    assert sp(0) == H.EINVAL and sp(-4) == H.EINVAL and sp(32769) == H.ELIMIT


def _stub(max_steps=3, batch_size=8, device_tensor=None, Z=50):
    return types.SimpleNamespace(max_steps=max_steps, batch_size=batch_size, canvas_size=50, windows_size=28,
                                 vae_latent_dimensions=Z,
                                 input_images=torch.zeros(batch_size, 2500) if device_tensor is None else device_tensor)


def test_python_class_refuses_on_the_host(H):
    from air.metrics import LatentProbe
    assert LatentProbe.names() == list(pc.NAMES)
    for kw in (dict(k=17), dict(classes=65), dict(capacity=32769)):
        with pytest.raises(NotImplementedError, match="holds 16, 64, 256 and 32768"):
            LatentProbe(_stub(), 2, **kw)
    with pytest.raises(NotImplementedError, match="holds 16, 64, 256 and 32768"):
        LatentProbe(_stub(Z=257), 2)
    with pytest.raises(NotImplementedError, match="collector holds 16 and 16"):
        LatentProbe(_stub(max_steps=17), 2)
    with pytest.raises(NotImplementedError, match="collector holds 16 and 16"):
        LatentProbe(_stub(), 17)
    with pytest.raises(ValueError, match="max_gt_digits"):
        LatentProbe(_stub(), 0)
    for kw, what in ((dict(k=0), "positive"), (dict(classes=0), "positive"), (dict(capacity=0), "capacity"),
                     (dict(au_threshold=-0.5), "au_threshold"), (dict(au_threshold=float("nan")), "au_threshold"),
                     (dict(max_distance=0.0), "max_distance")):
        with pytest.raises(ValueError, match=what):
            LatentProbe(_stub(), 2, **kw)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):           # valid arguments: what is missing is a device tensor
        LatentProbe(_stub(), 2)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        LatentProbe(_stub(device_tensor=np.zeros((8, 2500), np.float32)), 2)


def test_embeddings_probe_refuses_on_the_host(H):
    from air import embeddings
    make = lambda lat, lab: embeddings.Embeddings(lat, None, lab, None, 0, 0, 0)      # noqa: E731
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        embeddings.probe(make(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)))


def test_training_refuses_the_probe_on_a_cache_without_labels(tmp_path):
    """parser.error (exit status 2) before anything touches a device or the results folder"""
    data = tmp_path / "multi_mnist_data"
    data.mkdir()
    zeros = np.zeros((4, 4), np.int32)
    np.savez(str(data / "common.npz"), images=np.zeros((4, 2500), np.float32), digits=np.zeros(4, np.int32))
    np.savez(str(data / "test.npz"), images=np.zeros((4, 2500), np.float32), digits=np.zeros(4, np.int32), positions=zeros, boxes=zeros)
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "training.py")
    p = subprocess.run([sys.executable, script, "--latent-probe", "-r", str(tmp_path / "out")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "holds none" in p.stderr and "labels" in p.stderr, (p.returncode, p.stderr[-400:])
    assert not (tmp_path / "out").exists()
    p = subprocess.run([sys.executable, script, "--latent-probe", "--latent-k", "17"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--latent-k" in p.stderr
