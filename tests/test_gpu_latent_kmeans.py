"""GPU tests of the latent clusters (air_latent_kmeans of include/air_hip.h, air.metrics.LatentClusters,
air.embeddings.cluster, training.py --latent-clusters, embeddings.py --kmeans).

The reference is the float64 restatement of tests/latent_kmeans_cases.py.  Every output of the entry point is compared BIT
FOR BIT: the arithmetic and its order are fully stated, so there is no tolerance.  Inputs, outputs and the workspace sit
between guard bands that must be intact afterwards, and rows >= M_eff of the codes are NaN: reading one would show.  The one
float allowance is on ari and nmi of values(), whose logarithms are the device library's (latent_kmeans_cases.score_allowance
derives it; the largest gap seen is printed)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_check as abi
import latent_kmeans_cases as kc

pytestmark = pytest.mark.gpu

PKG = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd")
GUARD = 8                                    # sentinel elements in front of and behind every buffer
FILL_I32, FILL_I64, FILL_F64 = -5, -(2 ** 40) - 5, -7.25
CASES = kc.cases()


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """a device buffer of n elements between two rows of sentinels; `init` fills the payload, `skew` shifts it by that
    many elements (an address off the allocator's alignment)"""

    def __init__(self, n, dtype, fill, init=None, skew=0, bytes_ff=False):
        self.n, self.fill, self.at = n, fill, GUARD + skew
        self.buf = torch.full((n + 2 * GUARD + skew,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[self.at:self.at + n]
        if init is not None:
            self.view.copy_(init)
        elif bytes_ff:
            self.view.view(torch.uint8).fill_(0xFF)

    def payload(self):
        """the payload as numpy, after checking the sentinels"""
        host = self.buf.cpu().numpy()
        for band in (host[:self.at], host[self.at + self.n:]):
            assert np.isnan(band).all() if self.fill != self.fill else (band == self.fill).all(), "a sentinel was overwritten"
        return host[self.at:self.at + self.n]


def run_case(H, case, row_d2=True, skew=0, bytes_ff=False):
    """one air_latent_kmeans call -> the six outputs as numpy; every output starts as sentinels (or 0xFF bytes), so an
    element the call does not write shows"""
    x, labels, k, classes, R = case["x"], case["labels"], case["k"], case["classes"], case["restarts"]
    M, Z = x.shape
    lat = Guarded(M * Z, torch.float32, float("nan"), init=_dev(x.reshape(-1)), skew=skew)
    assert skew == 0 or H.ptr(lat.view).value % 16 == 4 * skew
    lab = None if labels is None else Guarded(M, torch.int32, FILL_I32, init=_dev(labels))
    rows = None if case["rows"] is None else torch.tensor([case["rows"]], dtype=torch.int32, device="cuda")
    nbytes = H.lib().air_latent_kmeans_workspace_bytes(M, Z, k, R)
    assert nbytes == kc.workspace_bytes(M, Z, k, R)
    ws = Guarded(nbytes // 8, torch.float64, FILL_F64)
    out = dict(assignment=Guarded(M, torch.int32, FILL_I32, bytes_ff=bytes_ff), row_d2=Guarded(M, torch.float64, FILL_F64, bytes_ff=bytes_ff),
               centroids=Guarded(k * Z, torch.float64, FILL_F64, bytes_ff=bytes_ff),
               restart_inertia=Guarded(R, torch.float64, FILL_F64, bytes_ff=bytes_ff),
               restart_iters=Guarded(R, torch.int32, FILL_I32, bytes_ff=bytes_ff),
               counts=Guarded(kc.COUNTS + 2 * k + k * classes, torch.int64, FILL_I64, bytes_ff=bytes_ff))
    a = H.LatentKmeans(H.ptr(lat.view), H.ptr(None if lab is None else lab.view), H.ptr(rows), H.ptr(out["assignment"].view),
                       H.ptr(out["row_d2"].view if row_d2 else None), H.ptr(out["centroids"].view),
                       H.ptr(out["restart_inertia"].view), H.ptr(out["restart_iters"].view), H.ptr(out["counts"].view),
                       M, Z, k, classes, R, case["max_iters"], case["seed"])
    H.launch("air_latent_kmeans", torch.device("cuda"), C.byref(a), H.ptr(ws.view))
    torch.cuda.synchronize()
    ws.payload(), lat.payload()
    if lab is not None:
        lab.payload()
    got = {key: g.payload() for key, g in out.items()}
    if not row_d2:
        assert bytes_ff or (got["row_d2"] == FILL_F64).all()
    got["centroids"] = got["centroids"].reshape(k, Z)
    return got


def check_case(H, name, **kw):
    want, got = kc.expected(name), run_case(H, CASES[name], **kw)
    print("%s: counts %s iters %s" % (name, got["counts"][:kc.COUNTS].tolist(), got["restart_iters"].tolist()))
    assert kc.same_bits(want, got) == [], (name, got["counts"][:kc.COUNTS], want["counts"][:kc.COUNTS], got["restart_iters"],
                                           want["restart_iters"])
    return got


@pytest.mark.parametrize("name", [kc.shape_name(s) for s in kc.SHAPES])
def test_kernel_equals_the_restatement(H, name):
    """(M, Z, k, R): M = 1, 2, 63, 64, 65, 257, 700; Z = 1, 3, 50; k = 1, 2, 3, 10 (one cluster of a dimension per thread, and
    several); R = 1, 8; V < k; and the limits together, Z = 256, k = 64, R = 32: 130 KiB of LDS"""
    check_case(H, name)


def test_three_blobs_tie_to_the_bit_and_the_first_restart_wins(H):
    got = check_case(H, "three_blobs")
    assert len({got["restart_inertia"][r].tobytes() for r in range(8)}) == 1 and got["counts"][kc.BEST] == 0
    assert got["counts"][kc.CORRECT] == got["counts"][kc.LABELLED] == 65


def test_the_iteration_cap_and_convergence(H):
    short, long_ = check_case(H, "unconverged"), check_case(H, "converged")
    assert short["restart_iters"].tolist() == [3, 3] and short["counts"][kc.CONVERGED] == 0
    assert long_["counts"][kc.CONVERGED] == 1 and long_["counts"][kc.RESTARTS_CONVERGED] == 2


def test_a_cluster_without_members_keeps_its_centroid_and_a_tie_goes_to_the_lower_cluster(H):
    got = check_case(H, "duplicates")
    assert got["counts"][kc.LIVE] == 2
    got = check_case(H, "exact_tie")
    assert got["assignment"].tolist() == [0, 1, 0]


@pytest.mark.parametrize("name", kc.EDGES)
def test_edges_of_validity_and_the_cursor(H, name):
    """NaN and Inf rows inside the set, labels out of range (clustered, not scored), V < k, V == 1, V == 0, labels null,
    *rows = 0, < M, > M and negative with NaN garbage beyond"""
    got = check_case(H, name)
    assert got["counts"][kc.ROWS] == kc.effective_rows(37, CASES[name]["rows"])


@pytest.mark.parametrize("name", ["m257_z3_k10_r8", "nan_row", "m63_z50_k10_r1"])
def test_without_row_d2_and_off_a_16_byte_boundary(H, name):
    """row_d2 null: the other outputs are the same; the latents one float off a 16-byte boundary: rows are read float by float"""
    want = kc.expected(name)
    got = run_case(H, CASES[name], row_d2=False)
    assert [key for key in kc.same_bits(want, got) if key != "row_d2"] == []
    got = run_case(H, CASES[name], skew=1)
    assert kc.same_bits(want, got) == []


def test_the_same_inputs_give_the_same_bits_into_dirty_buffers(H):
    for name in ("m257_z3_k10_r8", "all_invalid", "v_below_k"):
        a, b = run_case(H, CASES[name]), run_case(H, CASES[name], bytes_ff=True)
        assert kc.same_bits(a, b) == [] and kc.same_bits(kc.expected(name), b) == [], name


def test_properties_at_the_working_size(H):
    """M = 2000, Z = 50, k = 10, R = 8, from the outputs alone: every valid row's centroid is its nearest under the stated
    expression; the centroids of a converged winner are the stated means of its members; the winner's inertia is the first
    minimum and the stated sum"""
    case = kc.blobs(2000, 50, 10, restarts=8, max_iters=100, seed=77, sigma=3.0)
    got = run_case(H, case)
    x = case["x"].astype(np.float64)
    counts, a, mu = got["counts"], got["assignment"], got["centroids"]
    print("working size: counts %s iters %s" % (counts[:kc.COUNTS].tolist(), got["restart_iters"].tolist()))
    assert counts[kc.VALID] == 2000 and (a >= 0).all() and counts[kc.CONVERGED] == 1 and np.isfinite(mu).all()
    d2 = kc.distances(x, mu)
    assert np.array_equal(np.argmin(d2, axis=1), a)
    assert d2[np.arange(2000), a].tobytes() == got["row_d2"].tobytes()
    for c in range(10):
        members = x[a == c]
        assert len(members) == kc.parts(counts, 10, 10)[0][c]
        if len(members):
            mean = np.add.accumulate(np.concatenate((np.zeros((1, 50)), members)), axis=0)[-1] / np.float64(len(members))
            assert mean.tobytes() == mu[c].tobytes(), c
    best = int(counts[kc.BEST])
    assert best == int(np.argmin(got["restart_inertia"])) and got["restart_inertia"][best] == kc.seq_sum(got["row_d2"])
    assert counts[kc.ITERS] == got["restart_iters"][best]
    table = kc.parts(counts, 10, 10)[2]
    assert np.array_equal(table, np.bincount(a * 10 + case["labels"], minlength=100).reshape(10, 10))


# ------------------------------------------------------------------------------------------------------------- the module
def _real_model(scope):
    """AIRModel(cnn=False, train=False) at B = 8, T = 3 on scenes a DeviceSceneSource composed, as tests/test_gpu_latent_probe.py
    sets it up: the z_pres bias of a fresh model is raised until every image holds an object"""
    import multi_mnist as mm
    from air import air_model as am
    from oracle import air_oracle as ao
    hp = dict(ao.TRAINING_HP)
    B, G = 8, 2
    am.reset_default_graph()
    images = torch.zeros(B, hp["canvas_size"] ** 2, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    model = am.AIRModel(images, digits, cnn=False, train=False, scope=scope, gemm_precision="fp32", **hp)
    params = {k: np.array(v) for k, v in ao.init_params(hp, 0).items()}
    bias = "z_pres/log_odds/output/biases"
    glyphs, glyph_labels, _ = mm.load_glyphs()
    source = mm.DeviceSceneSource(glyphs, B, images, digits, canvas_dim=hp["canvas_size"], max_digits=G, seed=5)
    source.next_batch()
    for _ in range(12):
        model.load_state_dict(params)
        model.forward()
        if bool((model.run_digits > 0).all()):
            break
        params[bias] = params[bias] + np.float32(1.0)
    meta = source.meta()
    labels = torch.from_numpy(np.asarray(glyph_labels, np.int32)).cuda()[meta["indices"].long().clamp(min=0)].contiguous()
    return model, (digits, meta["positions"], meta["boxes"], labels), hp


def test_module_on_a_real_model_beside_the_probe(H):
    from air.metrics import LatentClusters, LatentProbe
    model, truth, hp = _real_model("clusters8")
    Z, k, classes = hp["vae_latent_dimensions"], 3, 10
    alone = LatentProbe(model, 2, k=3, max_distance=2.9)
    alone.evaluate(*truth)
    alone_bits = (alone.counts.cpu().numpy().tobytes(), alone.moments.cpu().numpy().tobytes(), alone.values().cpu().numpy().tobytes())
    clu = LatentClusters(model, 2, clusters=k, restarts=4, max_iters=20, seed=9, max_distance=2.9, per_row=True)
    probe = LatentProbe(model, 2, k=3, max_distance=2.9)
    assert clu.names() == list(kc.NAMES)
    assert np.isnan(clu.values().cpu().numpy()[:4]).all()                  # nothing scored yet: no number
    clu.evaluate(*truth)
    probe.evaluate(*truth)
    values = clu.values()
    assert values.is_cuda and values.dtype == torch.float64
    matched, present, inferred, overflow = clu.counters.tolist()
    assert matched >= 4 and not overflow and clu.counters.tolist() == probe.counters.tolist()
    assert (probe.counts.cpu().numpy().tobytes(), probe.moments.cpu().numpy().tobytes(), probe.values().cpu().numpy().tobytes()) == alone_bits
    x, lab = clu.latents.cpu().numpy(), clu.labels.cpu().numpy()
    assert x.tobytes() == probe.latents.cpu().numpy().tobytes() and lab.tobytes() == probe.labels.cpu().numpy().tobytes()
    # evaluate() is the entry point run on the instrument's own store
    want = kc.kmeans(x, lab, k, classes, 4, 20, seed=9, rows=matched)
    got = {key: getattr(clu, key).cpu().numpy() for key in kc.KEYS}
    assert kc.same_bits(want, got) == []
    again = run_case(H, dict(x=x, labels=lab, k=k, classes=classes, restarts=4, max_iters=20, seed=9, rows=matched))
    assert kc.same_bits(again, got) == []
    table = kc.parts(want["counts"], k, classes)[2]
    hc, hl = kc.entropies(table)
    print("real model: %d matched, table %s, H(c) %.3f H(l) %.3f" % (matched, table.tolist(), hc, hl))
    assert hc > 0.1 and hl > 0.1                                           # the quotient does not magnify the gap
    ref, val = kc.derived(want, k, classes), values.cpu().numpy()
    gap = np.abs(val[1:3] - ref[1:3])
    print("values %s restatement %s: largest gap on ari / nmi %.3g of %.3g allowed" % (val.tolist(), ref.tolist(), gap.max(),
                                                                                       kc.score_allowance(k, classes)))
    assert val[0] == ref[0] and val[3:].tobytes() == ref[3:].tobytes()     # accuracy, inertia, live, scored: exact
    assert (gap <= kc.score_allowance(k, classes)).all()
    into = torch.zeros(len(kc.NAMES), dtype=torch.float64, device="cuda")
    assert clu.values(into) is into and torch.equal(into, values)
    res = clu.result()
    assert [res[n] for n in kc.NAMES] == val.tolist() and res["table"].tobytes() == table.tobytes() and res["matched"] == matched
    assert res["centroids"].tobytes() == want["centroids"].tobytes() and res["restart_iters"].tobytes() == want["restart_iters"].tobytes()
    assert (res["best"], res["iters"], res["converged"], res["restarts_converged"]) == tuple(
        int(want["counts"][i]) for i in (kc.BEST, kc.ITERS, kc.CONVERGED, kc.RESTARTS_CONVERGED))
    clu.reset()
    assert clu.counters.tolist() == [0, 0, 0, 0] and not clu.counts.any()
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        clu.update(truth[0], truth[1].cpu(), truth[2], truth[3])


def test_embeddings_cluster_and_the_centroid_sheet(H, tmp_path):
    """cluster() on tensors equals the restatement; write_clusters() writes both files, and the sheet's tiles are a direct
    decode of the live centroids"""
    from air import embeddings
    case = CASES["m63_z50_k10_r1"]
    want = kc.expected("m63_z50_k10_r1")
    got = embeddings.cluster(_dev(case["x"]), _dev(case["labels"]), clusters=10, classes=10, restarts=1, max_iters=30, seed=case["seed"])
    assert got["table"].tobytes() == kc.parts(want["counts"], 10, 10)[2].tobytes()
    assert got["centroids"].tobytes() == want["centroids"].tobytes() and got["assignment"].tobytes() == want["assignment"].tobytes()
    assert got["accuracy"] == kc.derived(want, 10, 10)[0]
    unlabelled = embeddings.cluster(_dev(case["x"]), None, clusters=10, restarts=1, max_iters=30, seed=case["seed"])
    assert unlabelled["assignment"].tobytes() == want["assignment"].tobytes() and unlabelled["labelled"] == 0
    with pytest.raises(ValueError, match="nothing to cluster"):
        embeddings.cluster(_dev(case["x"])[:0], None)
    model, _, hp = _real_model("clusters_sheet")
    Z, w, B = hp["vae_latent_dimensions"], hp["windows_size"], 8
    assert case["x"].shape[1] == Z
    paths = embeddings.write_clusters(str(tmp_path), got, model)
    assert sorted(os.listdir(tmp_path)) == ["cluster_sprites.png", "clusters.npz"]
    back = np.load(paths["clusters"])
    assert back["centroids"].tobytes() == want["centroids"].tobytes() and back["table"].tobytes() == got["table"].tobytes()
    assert back["names"].tolist() == list(kc.NAMES) and back["values"][0] == got["accuracy"]
    live = np.nonzero(got["sizes"] > 0)[0]
    assert back["live"].tolist() == live.tolist() and len(live) > B        # more than one decode call
    windows = embeddings.centroid_windows(model, got["centroids"][live])
    direct = []
    for lo in range(0, len(live), B):
        take = min(B, len(live) - lo)
        latents = torch.zeros(B, 3, Z, device="cuda")
        latents[:take, 0] = _dev(got["centroids"][live[lo:lo + take]].astype(np.float32))
        z_pres = torch.zeros(B, 3, device="cuda")
        z_pres[:, 0] = 1.0
        scenes = model.decode(latents, torch.ones(B, 3, 1, device="cuda"), torch.zeros(B, 3, 2, device="cuda"), z_pres)
        direct.append(scenes.windows[:take, 0].reshape(take, w, w).clone())
    assert torch.equal(windows, torch.cat(direct))
    import tf_events
    sheet = embeddings.sprite_sheet(windows).cpu().numpy()
    assert open(paths["sprites"], "rb").read() == tf_events.encode_png(sheet)


# ------------------------------------------------------------------------------------------------------------ the drivers
def _train(tmp_path, name, *flags):
    out = tmp_path / name
    p = subprocess.run([sys.executable, "training.py", "--online-data", "--glyph-style", "mnist-like", "--latent-clusters",
                        "--cluster-restarts", "4", "--iterations", "200", "--print-every", "0", "--precision", "bf16",
                        "--jitter-bank", "256", "-r", str(out)] + list(flags), cwd=PKG, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-600:], p.stderr[-1500:])
    return p.stdout, [json.loads(ln) for ln in open(out / "summary" / "scalars.jsonl")]


def test_training_driver_carries_the_instrument(tmp_path):
    """training.py --latent-clusters for 200 iterations as 50-step replays and with --no-graph: every row carries the clu_*
    keys, both runs report the same rows, and the run ends with the cluster table"""
    out_g, rows_g = _train(tmp_path, "graph", "--graph-steps", "50")
    out_e, rows_e = _train(tmp_path, "eager", "--no-graph")
    keys = ["clu_" + k for k in kc.NAMES]
    for out, rows in ((out_g, rows_g), (out_e, rows_e)):
        assert len(rows) >= 4
        for r in rows:
            assert [k for k in r if k.startswith("clu_")] == keys
            assert all(r[k] is None or isinstance(r[k], (int, float)) for k in keys)
        assert rows[-1]["clu_scored"] is not None and rows[-1]["clu_live_clusters"] is not None
        assert "latent clusters, 10-means (4 restarts" in out and "cluster table (rows: cluster 0..9, columns: true class 0..9):" in out
    strip = lambda rows: [{k: v for k, v in r.items() if k != "wall_s"} for r in rows]       # noqa: E731
    by_step = {r["step"]: r for r in strip(rows_e)}
    assert all(by_step[r["step"]] == r for r in strip(rows_g) if r["step"] in by_step)


def test_embeddings_script_writes_both_files(H, tmp_path):
    """embeddings.py --kmeans 10 on 12 records in a fresh child process: clusters.npz and cluster_sprites.png beside the
    projector files"""
    import test_gpu_embeddings as tge
    from air import air_model as am
    from demo.model_wrapper import ModelWrapper
    from multi_mnist import write_to_records
    am.reset_default_graph()
    images, _ = tge.blob_canvases(12, 50, 2, seed=21)
    images = [np.asarray(im, np.float32).reshape(-1) for im in images]
    params = {k: np.array(v) for k, v in tge.ao.init_params(tge.HP, 0).items()}
    twin = am.AIRModel(torch.zeros(8, 2500, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"),
                       max_steps=3, rnn_units=256, canvas_size=50, windows_size=28,
                       vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                       vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                       z_pres_temperature=1.0, stopping_threshold=0.99, cnn=False,
                       train=False, reuse=False, scope="kmeans_twin", gemm_precision="fp32")
    for _ in range(12):
        twin.load_state_dict(params)
        rec = ModelWrapper(twin, None, None).infer(images)
        if sum(rec[0]) >= 6:
            break
        params[tge.BIAS] = params[tge.BIAS] + np.float32(1.0)
    assert sum(rec[0]) >= 6, rec[0]
    ckpt = str(tmp_path / "air-model.pt")
    torch.save(twin.state_dict(), ckpt)
    digits, indices, positions, boxes, labels = tge._ground_truth(rec[0], rec[1], np.random.RandomState(9))
    write_to_records(str(tmp_path / "test"), images, indices, positions, boxes, labels, digits, side=50)
    out = str(tmp_path / "embeddings")
    p = subprocess.run([sys.executable, "embeddings.py", "--model", ckpt, "--data", str(tmp_path / "test.tfrecords"), "--out", out,
                        "--batch-size", "8", "--kmeans", "10"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    files = os.listdir(out)
    assert "clusters.npz" in files and "cluster_sprites.png" in files and "mnist_sprites.png" in files
    assert "Clustering accuracy:" in p.stdout and "Cluster table (rows: cluster, columns: true digit):" in p.stdout
    back = np.load(os.path.join(out, "clusters.npz"))
    assert back["centroids"].shape == (10, 50) and back["table"].shape == (10, 10) and back["table"].sum() == (back["assignment"] >= 0).sum()
    assert open(os.path.join(out, "cluster_sprites.png"), "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"
