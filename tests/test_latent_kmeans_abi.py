"""CPU-side checks of the latent clusters (include/air_hip.h: air_latent_kmeans*, air/metrics.py LatentClusters,
air/embeddings.py cluster, training.py --latent-clusters, embeddings.py --kmeans): the descriptor's layout, the exports and
the constants against the header; every refusal answered on the host before any launch, in the stated order, with host
pointers that are never dereferenced -- no descriptor that would launch is passed; the workspace query; the Python class's
refusals; the drivers' refusals.  (What the kernels compute: tests/test_gpu_latent_kmeans.py.)"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import abi_check as abi
import latent_kmeans_cases as kc

REQUIRED = ("latents", "assignment", "centroids", "restart_inertia", "restart_iters", "counts")
OPTIONAL = ("labels", "rows", "row_d2")
SIZES = ("M", "Z", "k", "classes", "restarts", "max_iters")


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _desc(H, ptrs=True, **override):
    """a descriptor that would pass every check (so it is only ever sent with something wrong)"""
    a = H.LatentKmeans()
    a.M, a.Z, a.k, a.classes, a.restarts, a.max_iters, a.seed = 100, 50, 10, 10, 8, 50, 3
    if ptrs:
        for k in REQUIRED + OPTIONAL:
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_the_header_the_mirror_and_the_cases_agree(H):
    assert abi.check_abi(H) == []
    h, num = abi.read_header(), abi.compile_numbers()
    assert h.structs["air_latent_kmeans_t"] == [f[0] for f in H.LatentKmeans._fields_]
    assert num.sizeof["air_latent_kmeans_t"] == C.sizeof(H.LatentKmeans) == 9 * 8 + 6 * 4 + 8
    assert h.prototypes["air_latent_kmeans"] == ("int", ["const air_latent_kmeans_t*", "void*", "void*"])
    assert h.prototypes["air_latent_kmeans_workspace_bytes"] == ("int64_t", ["int"] * 4)
    for name in ("air_latent_kmeans", "air_latent_kmeans_workspace_bytes"):
        assert hasattr(H.lib(), name) and name in H.EXPORTED_SYMBOLS, name
    assert (H.KMEANS_MAX_K, H.KMEANS_MAX_RESTARTS, H.KMEANS_MAX_ITERS) == (64, 32, 1000) == (kc.MAX_K, kc.MAX_RESTARTS, kc.MAX_ITERS)
    assert (H.PROBE_MAX_CLASSES, H.PROBE_MAX_Z, H.PROBE_MAX_ROWS) == (kc.MAX_CLASSES, kc.MAX_Z, kc.MAX_ROWS)
    for name in ("MAX_K", "MAX_RESTARTS", "MAX_ITERS", "ROWS", "VALID", "LABELLED", "CORRECT", "LIVE", "BEST", "ITERS", "CONVERGED",
                 "RESTARTS_CONVERGED", "COUNTS"):
        assert num.values["AIR_KMEANS_" + name] == getattr(kc, name) == getattr(H, "KMEANS_" + name), name
    assert H.lib().air_abi_version() == 6                       # additive
    from air import air_model as am
    assert am.KERNEL_NAMES["air_latent_kmeans"] == "kmeans_restart_kernel"


def test_every_refusal_comes_before_a_launch(H):
    lib, ws = H.lib(), abi.host_ptr()
    call = lambda a, w=ws: lib.air_latent_kmeans(C.byref(a), w, None)     # noqa: E731
    assert lib.air_latent_kmeans(None, ws, None) == H.EINVAL
    for k in SIZES:
        assert call(_desc(H, **{k: 0})) == H.EINVAL and call(_desc(H, **{k: -2})) == H.EINVAL, k
    for k, v in (("k", 65), ("restarts", 33), ("max_iters", 1001), ("Z", 257), ("classes", 65), ("M", 32769)):
        assert call(_desc(H, **{k: v})) == H.ELIMIT, k
    for missing in REQUIRED:
        assert call(_desc(H, **{missing: None})) == H.EINVAL, missing
    assert call(_desc(H), None) == H.EINVAL                                # no workspace
    assert call(_desc(H, ptrs=False)) == H.EINVAL
    odd = abi.host_ptr().value + 4
    for k in ("row_d2", "centroids", "restart_inertia"):
        assert call(_desc(H, **{k: odd})) == H.EALIGN, k
    assert call(_desc(H), C.c_void_p(odd)) == H.EALIGN
    # the order: a size before a limit, a limit before a null pointer, a null pointer before alignment
    assert call(_desc(H, k=65, Z=0)) == H.EINVAL and call(_desc(H, M=32769, max_iters=0)) == H.EINVAL
    assert call(_desc(H, ptrs=False, k=65)) == H.ELIMIT and call(_desc(H, max_iters=1001), None) == H.ELIMIT
    assert call(_desc(H, centroids=odd, latents=None)) == H.EINVAL and call(_desc(H, row_d2=odd), None) == H.EINVAL


def test_workspace_query_answers_as_the_entry_point(H):
    q = H.lib().air_latent_kmeans_workspace_bytes
    for M, Z, k, R in ((1, 1, 1, 1), (2, 50, 10, 8), (65, 3, 3, 8), (257, 3, 10, 3), (2000, 50, 10, 8), (32768, 256, 64, 32)):
        assert q(M, Z, k, R) == kc.workspace_bytes(M, Z, k, R) and q(M, Z, k, R) % 8 == 0, (M, Z, k, R)
    for bad in ((0, 50, 5, 1), (100, 0, 5, 1), (100, 50, 0, 1), (100, 50, 5, 0), (-1, 50, 5, 1)):
        assert q(*bad) == H.EINVAL, bad
    for bad in ((32769, 50, 5, 1), (100, 257, 5, 1), (100, 50, 65, 1), (100, 50, 5, 33)):
        assert q(*bad) == H.ELIMIT, bad
    assert q(32769, 0, 5, 1) == H.EINVAL                                   # a size before a limit


def _stub(max_steps=3, batch_size=8, device_tensor=None, Z=50):
    return types.SimpleNamespace(max_steps=max_steps, batch_size=batch_size, canvas_size=50, windows_size=28,
                                 vae_latent_dimensions=Z,
                                 input_images=torch.zeros(batch_size, 2500) if device_tensor is None else device_tensor)


def test_python_class_refuses_on_the_host_and_declares_its_protocol(H):
    from air import metrics
    from air.metrics import LatentClusters
    assert LatentClusters.names() == list(kc.NAMES) == list(metrics.CLUSTER_NAMES)
    assert (LatentClusters.prefix, LatentClusters.group, tuple(LatentClusters.reported), LatentClusters.nan_in_events) == \
        ("clu_", "clusters/", kc.NAMES, False)
    assert issubclass(LatentClusters, metrics._Instrument) and issubclass(metrics.LatentProbe, metrics._LatentStore)
    assert LatentClusters.update is metrics.LatentProbe.update             # one collector call, shared
    for kw in (dict(clusters=65), dict(classes=65), dict(restarts=33), dict(max_iters=1001), dict(capacity=32769)):
        with pytest.raises(NotImplementedError, match="holds 64, 64, 32, 1000, 256 and 32768"):
            LatentClusters(_stub(), 2, **kw)
    with pytest.raises(NotImplementedError, match="holds 64, 64, 32, 1000, 256 and 32768"):
        LatentClusters(_stub(Z=257), 2)
    with pytest.raises(NotImplementedError, match="collector holds 16 and 16"):
        LatentClusters(_stub(max_steps=17), 2)
    with pytest.raises(ValueError, match="max_gt_digits"):
        LatentClusters(_stub(), 0)
    for kw, what in ((dict(clusters=0), "positive"), (dict(classes=0), "positive"), (dict(restarts=0), "positive"),
                     (dict(max_iters=0), "positive"), (dict(capacity=0), "capacity"), (dict(max_distance=0.0), "max_distance")):
        with pytest.raises(ValueError, match=what):
            LatentClusters(_stub(), 2, **kw)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):           # valid arguments: what is missing is a device tensor
        LatentClusters(_stub(), 2)


def test_embeddings_cluster_refuses_on_the_host(H):
    from air import embeddings
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        embeddings.cluster(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        embeddings.cluster(np.zeros((4, 3), np.float32), None)


def test_drivers_refuse_before_anything_touches_a_device(tmp_path):
    """parser.error (exit status 2) before the results folder exists"""
    data = tmp_path / "multi_mnist_data"
    data.mkdir()
    zeros = np.zeros((4, 4), np.int32)
    np.savez(str(data / "common.npz"), images=np.zeros((4, 2500), np.float32), digits=np.zeros(4, np.int32))
    np.savez(str(data / "test.npz"), images=np.zeros((4, 2500), np.float32), digits=np.zeros(4, np.int32), positions=zeros, boxes=zeros)
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "training.py")
    run = lambda *argv: subprocess.run([sys.executable, script] + list(argv), cwd=str(tmp_path), capture_output=True,    # noqa: E731
                                       text=True, timeout=300)
    p = run("--latent-clusters", "-r", str(tmp_path / "out"))
    assert p.returncode == 2 and "holds none" in p.stderr and "labels" in p.stderr, (p.returncode, p.stderr[-400:])
    assert not (tmp_path / "out").exists()
    p = run("--latent-clusters", "--cluster-count", "65")
    assert p.returncode == 2 and "--cluster-count" in p.stderr
    p = run("--latent-clusters", "--cluster-restarts", "0")
    assert p.returncode == 2 and "--cluster-restarts" in p.stderr
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "embeddings.py")
    p = subprocess.run([sys.executable, script, "--kmeans", "65"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--kmeans" in p.stderr
