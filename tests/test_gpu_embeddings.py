"""GPU tests of the projector export (air_embed_collect / air_embed_sprites of include/air_hip.h, air/embeddings.py, the
embeddings.py script).

The reference is the float64 restatement of tests/embedding_cases.py.  Everything is compared bit for bit: the match is a
chain of decisions on correctly rounded float64 operations (subtract, multiply, add, sqrt, divide), the rows are copies, the
grey levels come from a correctly rounded float64 division -- and tests/test_embedding_cases.py asserts that no decision of
the random cases hangs on the last bits of a distance."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_check as abi
import embedding_cases as ec
from oracle import air_oracle as ao
from oracle.synth import blob_canvases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
CANARY_ROWS = 2
FILL = dict(latents=-7.5, windows=-3.25, labels=-77, ids=-99)
CASES = ec.gpu_cases()


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_collect(H, case, capacity):
    """the chunks of `case` through air_embed_collect, one call each, on outputs of capacity + CANARY_ROWS rows
    -> (per-chunk match, counters, outputs) as numpy"""
    T, B, G, Z, w = (case[k] for k in ("T", "B", "G", "Z", "w"))
    rows = capacity + CANARY_ROWS
    out = dict(latents=torch.full((rows, Z), FILL["latents"], device="cuda"),
               windows=torch.full((rows, w * w), FILL["windows"], device="cuda"),
               labels=torch.full((rows,), FILL["labels"], dtype=torch.int32, device="cuda"),
               ids=torch.full((rows,), FILL["ids"], dtype=torch.int32, device="cuda"))
    counters = torch.zeros(H.EMBED_COUNTERS, dtype=torch.int32, device="cuda")
    matches, keep = [], []
    for c in case["chunks"]:
        k = c["k"]
        n = H.lib().air_embed_collect_workspace_ints(T, B, k, G)
        assert n == k * G
        ws = torch.full((n + 4,), -5, dtype=torch.int32, device="cuda")
        match = torch.full((k * G + 4,), -5, dtype=torch.int32, device="cuda")
        d = {name: _dev(c[name]) for name in ("att", "run_digits", "ml", "vrec", "gt_count", "gt_positions", "gt_boxes",
                                              "gt_labels", "gt_ids")}
        a = H.EmbedCollect(*(H.ptr(d[name]) for name in ("att", "run_digits", "ml", "vrec", "gt_count", "gt_positions",
                                                          "gt_boxes", "gt_labels", "gt_ids")),
                           H.ptr(match), H.ptr(counters), H.ptr(out["latents"]), H.ptr(out["windows"]), H.ptr(out["labels"]),
                           H.ptr(out["ids"]), T, B, k, G, Z, w, capacity, case["canvas_size"], case["max_distance"])
        H.launch("air_embed_collect", torch.device("cuda"), C.byref(a), H.ptr(ws))      # stream-ordered: no sync between chunks
        matches.append(match)
        keep.append((d, ws))
    torch.cuda.synchronize()
    for m, (_, ws) in zip(matches, keep):
        assert m[-4:].tolist() == [-5] * 4 and ws[-4:].tolist() == [-5] * 4              # nothing behind match / workspace
    return [m[:-4].cpu().numpy().reshape(-1, G) for m in matches], counters.cpu().numpy(), \
        {k: v.cpu().numpy() for k, v in out.items()}


def check_collect(H, name, capacity=None):
    case = CASES[name]
    total = int(ec.expected(case, 10 ** 4, 10 ** 4, FILL)[1][0])
    capacity = total if capacity is None else capacity
    want_m, want_c, want_o = ec.expected(case, capacity, capacity + CANARY_ROWS, FILL)
    got_m, got_c, got_o = run_collect(H, case, capacity)
    print("%s: matched %d present %d inferred %d overflow %d (capacity %d)" % ((name,) + tuple(int(v) for v in got_c) + (capacity,)))
    for g, wnt in zip(got_m, want_m):
        assert g.tobytes() == wnt.tobytes(), (name, g, wnt)
    assert got_c.tobytes() == want_c.tobytes(), (name, got_c, want_c)
    for k in ("latents", "windows", "labels", "ids"):
        assert got_o[k].dtype == want_o[k].dtype and got_o[k].tobytes() == want_o[k].tobytes(), (name, k)
        assert (got_o[k][capacity:] == FILL[k]).all(), (name, k)                         # the canary rows
    return got_m, got_c


@pytest.mark.parametrize("name", ["chunks_z50_w28", "chunks_z3_w5", "below_tie_z3_w5"])
def test_collect_chunks_with_planted_cases(H, name):
    """T = 3, B = 5, G = 3, seven images in chunks of 5 and 2 (cursor carry, k < B); Z = 50 rows are 8-byte aligned, 25 floats
    of a 5 x 5 window are no multiple of four"""
    got_m, got_c = check_collect(H, name)
    p, flat = CASES[name]["planted"], np.concatenate(got_m)
    assert flat[p["tie"]][0] == (-1 if name.startswith("below") else 0) and flat[p["shared"]].tolist() == [0, -1, -1]


def test_collect_scan_across_waves_and_passes(H):
    """B = 70 in one chunk: two waves of the matching workgroup; B = 150 with T = G = 16: a second, strided pass as well"""
    check_collect(H, "b70")
    check_collect(H, "b150_strided")


def test_collect_overflow_is_guarded(H):
    """capacity two rows short: the overflow counter is set, the rows that fit are right, the canary rows intact"""
    for name in ("chunks_z50_w28", "b70"):
        total = int(ec.expected(CASES[name], 10 ** 4, 10 ** 4, FILL)[1][0])
        assert total > 2
        _, got_c = check_collect(H, name, capacity=total - 2)
        assert got_c[H.EMBED_OVERFLOW] == 1 and got_c[H.EMBED_MATCHED] == total


# ----------------------------------------------------------------------------------------------------------------- sprites
def test_sprites_equal_matplotlibs_plane(H, golden_dir):
    from air import embeddings
    levels = np.load(os.path.join(golden_dir, "sprite_levels.npz"))
    for c in range(5):
        windows, plane = levels["windows_%d" % c], levels["plane_%d" % c]
        got = embeddings.sprite_sheet(_dev(windows))
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == plane.shape
        assert got.cpu().numpy().tobytes() == plane.tobytes(), c
        flat = embeddings.sprite_sheet(_dev(windows.reshape(windows.shape[0], -1)))      # [M, w * w] is accepted too
        assert torch.equal(flat, got)
    A = _dev(np.zeros(16, np.float32))
    assert H.lib().air_embed_sprites(H.ptr(A), 0, 4, H.ptr(A), H.ptr(A), None) == -1     # M = 0: AIR_EINVAL
    with pytest.raises(ValueError):
        embeddings.sprite_sheet(torch.zeros(0, 4, 4, device="cuda"))
    # every grey level: a ramp that reaches all 256 indices, against the restatement
    ramp = (np.arange(1024, dtype=np.float32) / 1023.0).reshape(1, 32, 32)
    want = ec.sprite_levels(ramp)
    assert len(np.unique(want)) == len(np.unique(ec.grey_table())) == 232    # (the table repeats 24 of its levels)
    assert embeddings.sprite_sheet(_dev(ramp)).cpu().numpy().tobytes() == want.tobytes()


# -------------------------------------------------------------------------------------------------------------- the module
HP = dict(ao.TRAINING_HP)
N_IMAGES = 20
BIAS = "z_pres/log_odds/output/biases"


def _noise(B):
    """injected noise that is the same in every batch row: what the model makes of an image does not depend on the row (or
    the chunk) it lands in"""
    return {k: np.ascontiguousarray(np.repeat(v[:, :1], B, axis=1)) for k, v in ao.make_noise(HP, 1, seed=3).items()}


def _inference_model(B, params, scope):
    from air import air_model as am
    model = am.AIRModel(torch.zeros(B, HP["canvas_size"] ** 2, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
                        cnn=False, train=False, scope=scope, gemm_precision="fp32", **HP)
    model.load_state_dict(params)
    model.set_noise(_noise(B))
    model.set_dynamic(z_pres_prior_log_odds=-2.0)
    return model


def _ground_truth(rec_digits, rec_positions, rng):
    """ground truth from the inferred shifts, snapped to the integer grid (a box of 27 or 28 pixels, whichever centre is
    nearer: at most 0.0103 off in transformer coordinates, far inside 0.2), in shuffled order; plus, for some images, a digit
    placed far away from every object and, for images without objects, sometimes a digit nobody found"""
    digits, indices, positions, boxes, labels = [], [], [], [], []
    half, nid = (HP["canvas_size"] - 1) / 2.0, 1000
    for i, n in enumerate(rec_digits):
        entries = []
        for k in rng.permutation(n):
            pb = []
            for v in rec_positions[i][k][1:]:
                c = (float(v) + 1.0) * half                                  # centre in pixels: x + (w - 1) / 2
                cand = [(abs(round(c - (w - 1) / 2.0) + (w - 1) / 2.0 - c), int(round(c - (w - 1) / 2.0)), w) for w in (27, 28)]
                pb.append(min(cand)[1:])
            entries.append(((pb[0][0], pb[1][0]), (pb[0][1], pb[1][1])))
        if rng.rand() < 0.4:
            far = [e for e in (((0, 0), (12, 12)), ((38, 38), (12, 12)), ((0, 38), (12, 12))) if all(
                ec.distance(*ec.st_center(*e[0], *e[1]), float(p[1]), float(p[2])) > 0.3 for p in rec_positions[i][:n])]
            if far:
                entries.insert(int(rng.randint(len(entries) + 1)), far[0])
        digits.append(len(entries))
        positions.append(np.asarray([v for e in entries for v in e[0]], np.int32))
        boxes.append(np.asarray([v for e in entries for v in e[1]], np.int32))
        indices.append(np.arange(nid, nid + len(entries), dtype=np.int32))
        labels.append(rng.randint(0, 10, len(entries)).astype(np.int32))
        nid += len(entries)
    return np.asarray(digits), indices, positions, boxes, labels


@pytest.fixture(scope="module")
def scene(H):
    """a fresh model at B = 8 whose z_pres bias was raised until it finds objects, 20 canvases, the lists of
    ModelWrapper.infer and a ground truth built from them"""
    from air import air_model as am
    from demo.model_wrapper import ModelWrapper
    am.reset_default_graph()
    images, _ = blob_canvases(N_IMAGES, HP["canvas_size"], HP["max_digits"], seed=21)
    images = [np.asarray(im, np.float32).reshape(-1) for im in images]
    params = {k: np.array(v) for k, v in ao.init_params(HP, 0).items()}
    model = _inference_model(8, params, "emb8")
    for raised in range(12):
        rec = ModelWrapper(model, None, None).infer(images)
        counts = rec[0]
        if sum(c > 0 for c in counts) * 3 >= N_IMAGES and max(counts) >= 2:
            break
        params[BIAS] = params[BIAS] + np.float32(1.0)
        model.load_state_dict(params)
    print("z_pres bias raised %d times: inferred counts %s" % (raised, counts))
    assert sum(c > 0 for c in counts) * 3 >= N_IMAGES and max(counts) >= 2, counts
    gt = _ground_truth(counts, rec[1], np.random.RandomState(8))
    return dict(model=model, params=params, images=images, rec=rec, gt=gt)


def _check_against_lists(res, rec, gt, what):
    digits, indices, positions, boxes, labels = gt
    want = ec.collect_lists(digits, indices, positions, boxes, labels, rec[0], rec[1], rec[3], rec[4], max_distance=0.2)
    print("%s: present %d inferred %d matched %d" % (what, want["present"], want["inferred"], want["matched"]))
    assert (res.present, res.inferred, res.matched) == (want["present"], want["inferred"], want["matched"])
    assert 0 < want["matched"] < want["present"]                              # some digits were placed far away
    assert res.ids.cpu().numpy().tobytes() == want["ids"].tobytes()
    assert res.labels.cpu().numpy().tobytes() == want["labels"].tobytes()
    assert tuple(res.latents.shape) == want["latents"].shape and tuple(res.windows.shape) == want["windows"].shape
    assert res.latents.cpu().numpy().tobytes() == want["latents"].tobytes()
    assert res.windows.cpu().numpy().tobytes() == want["windows"].tobytes()
    return want


def test_module_equals_the_restatement(H, scene):
    """20 canvases at B = 8: chunks of 8, 8 and 4"""
    from air import embeddings
    digits, indices, positions, boxes, labels = scene["gt"]
    res = embeddings.collect(scene["model"], scene["images"], digits, indices, positions, boxes, labels, max_distance=0.2)
    want = _check_against_lists(res, scene["rec"], scene["gt"], "B = 8")
    # every inferred object has its snapped twin in the ground truth: all of them are matched
    assert want["matched"] == want["inferred"]
    sheet = embeddings.sprite_sheet(res.windows)
    assert sheet.cpu().numpy().tobytes() == ec.sprite_levels(want["windows"]).tobytes()
    with pytest.raises(ValueError):
        embeddings.collect(scene["model"], scene["images"], digits, indices, positions, boxes, labels, max_distance=0.0)
    scene["res8"] = want


def test_module_at_another_batch_size(H, scene):
    """B = 5: chunks of 5, 5, 5, 5, no padded chunk -- the same arrays"""
    from air import embeddings
    from demo.model_wrapper import ModelWrapper
    digits, indices, positions, boxes, labels = scene["gt"]
    model = _inference_model(5, scene["params"], "emb5")
    res = embeddings.collect(model, scene["images"], digits, indices, positions, boxes, labels, max_distance=0.2)
    rec = ModelWrapper(model, None, None).infer(scene["images"])
    want5 = _check_against_lists(res, rec, scene["gt"], "B = 5")
    want8 = scene.get("res8") or ec.collect_lists(digits, indices, positions, boxes, labels, scene["rec"][0], scene["rec"][1],
                                                  scene["rec"][3], scene["rec"][4], max_distance=0.2)
    for k in ("ids", "labels", "latents", "windows"):
        assert want5[k].tobytes() == want8[k].tobytes(), k


# -------------------------------------------------------------------------------------------------------------- the script
def test_script_writes_the_projector_files(H, scene, tmp_path):
    """embeddings.py on 12 records in a fresh child process: the six files and the event file, and the totals collect() gives
    for the same model, data and batch size (the script's model draws its noise from the device generator, seed 0: so does
    `twin`)"""
    from air import air_model as am
    from air import embeddings
    from demo.model_wrapper import ModelWrapper
    from multi_mnist import read_test_data, write_to_records
    images = scene["images"][:12]
    twin = am.AIRModel(torch.zeros(8, 2500, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"),
                       max_steps=3, rnn_units=256, canvas_size=50, windows_size=28,
                       vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                       vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                       z_pres_temperature=1.0, stopping_threshold=0.99, cnn=False,
                       train=False, reuse=False, scope="script_twin", gemm_precision="fp32")
    twin.load_state_dict(scene["params"])
    ckpt = str(tmp_path / "air-model.pt")
    torch.save(twin.state_dict(), ckpt)
    # the device generator is keyed by (seed, global step): an inference model draws the same noise in every forward, so the
    # ground truth snapped from this pass is found again by collect() here and by the script's model in the child process
    rec = ModelWrapper(twin, None, None).infer(images)
    digits, indices, positions, boxes, labels = _ground_truth(rec[0], rec[1], np.random.RandomState(9))
    write_to_records(str(tmp_path / "test"), images, indices, positions, boxes, labels, digits, side=HP["canvas_size"])
    data = str(tmp_path / "test.tfrecords")
    res = embeddings.collect(twin, *read_test_data(data), max_distance=0.2)
    assert res.matched > 0
    out = str(tmp_path / "embeddings")
    p = subprocess.run([sys.executable, "embeddings.py", "--model", ckpt, "--data", data, "--out", out, "--batch-size", "8"],
                       cwd=PKG, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    files = sorted(os.listdir(out))
    events = [f for f in files if f.startswith("events.out.tfevents.")]
    assert len(events) == 1
    assert [f for f in files if f not in events] == sorted(["mnist_metadata.tsv", "mnist_sprites.png", "embeddings.index",
                                                           "embeddings.data-00000-of-00001", "checkpoint",
                                                           "projector_config.pbtxt"])
    totals = {k: int(v) for k, v in re.findall(r"^(Present digits|Inferred digits|Matched inference boxes): (\d+)$", p.stdout, re.M)}
    assert totals == {"Present digits": res.present, "Inferred digits": res.inferred, "Matched inference boxes": res.matched}, p.stdout
    assert "Digit distribution (among matched digits):" in p.stdout
    hist = {d: 0 for d in range(10)}
    for label in res.labels.cpu().tolist():
        hist[label] += 1
    assert str(hist) in p.stdout
    import tf_checkpoint
    back = tf_checkpoint.load_checkpoint(os.path.join(out, "embeddings"))
    assert back["air_mnist"].tobytes() == res.latents.cpu().numpy().tobytes()
    assert len(open(os.path.join(out, "mnist_metadata.tsv")).read().splitlines()) == res.matched + 1
