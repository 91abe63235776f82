"""CPU-side checks of the projector export (include/air_hip.h "projector export", air/embeddings.py): argument errors are
answered on the host before any HIP call; the restatement of tests/embedding_cases.py gives the hand-worked answers and matplotlib's grey levels
(tests/golden/sprite_levels.npz, written by tests/golden/make_sprite_levels.py); write_projector's files read back; and the
random cases the GPU tests compare exactly keep clear of rounding ties.  (What the kernels compute:
tests/test_gpu_embeddings.py.)"""
import ctypes as C
import math
import os
import struct
import zlib

import numpy as np
import pytest

import abi_check as abi
import embedding_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZEROS = dict(latents=0, windows=0, labels=0, ids=0)


@pytest.fixture(scope="module")
def H():
    return abi.hip()


# ------------------------------------------------------------------------------------------------- the library's answers
def test_restatement_reads_the_record_slots_of_the_binding(H):
    """(which are the header's: tests/test_abi.py)"""
    assert (H.ATT_STRIDE, H.ATT_X, H.ATT_Y) == (ec.ATT_STRIDE, ec.ATT_X, ec.ATT_Y)


def _collect_args(H, **kw):
    """a valid descriptor over never-dereferenced addresses (every refusal comes before a launch)"""
    vals = dict(T=3, B=5, k=5, G=3, Z=50, w=28, capacity=10, canvas_size=50, max_distance=0.2)
    for i, (n, t) in enumerate(H.EmbedCollect._fields_):
        if t is C.c_void_p:
            vals[n] = (i + 1) << 20
    vals.update(kw)
    return H.EmbedCollect(**vals)


def test_argument_errors_without_gpu(H):
    lib = H.lib()
    ws = C.c_void_p(1 << 30)

    def call(**kw):
        return lib.air_embed_collect(C.byref(_collect_args(H, **kw)), ws, None)
    assert lib.air_embed_collect(None, ws, None) == -1
    assert lib.air_embed_collect(C.byref(_collect_args(H)), None, None) == -1
    for n, t in H.EmbedCollect._fields_:
        if t is C.c_void_p:
            assert call(**{n: None}) == -1, n
    for bad in (dict(T=0), dict(B=0), dict(k=0), dict(k=6), dict(G=0), dict(Z=0), dict(w=0), dict(capacity=0), dict(T=-1),
                dict(canvas_size=1), dict(max_distance=0.0), dict(max_distance=-0.2), dict(max_distance=float("nan"))):
        assert call(**bad) == -1, bad
    for bad in (dict(T=17), dict(G=17), dict(w=257)):
        assert call(**bad) == -2, bad
    assert lib.air_embed_collect_workspace_ints(3, 5, 5, 3) == 15 and lib.air_embed_collect_workspace_ints(16, 70, 2, 16) == 32
    assert lib.air_embed_collect_workspace_ints(3, 5, 6, 3) == -1 and lib.air_embed_collect_workspace_ints(3, 5, 0, 3) == -1
    assert lib.air_embed_collect_workspace_ints(17, 5, 5, 3) == -2 and lib.air_embed_collect_workspace_ints(3, 5, 5, 17) == -2
    # sprites
    A = C.c_void_p(1 << 20)
    assert lib.air_embed_sprites(A, 0, 28, A, A, None) == -1                     # an empty sheet cannot be saved
    assert lib.air_embed_sprites(A, 4, 0, A, A, None) == -1 and lib.air_embed_sprites(A, -3, 28, A, A, None) == -1
    for args in ((None, 4, 28, A, A), (A, 4, 28, None, A), (A, 4, 28, A, None)):
        assert lib.air_embed_sprites(*args, None) == -1
    assert lib.air_embed_sprites(A, (1 << 22) + 1, 28, A, A, None) == -2 and lib.air_embed_sprites(A, 4, 257, A, A, None) == -2
    assert lib.air_embed_sprites(A, 4, 28, C.c_void_p((1 << 20) + 4), A, None) == -3
    assert lib.air_embed_sprites(A, 4, 28, A, C.c_void_p((1 << 20) + 2), None) == -3
    assert lib.air_embed_sprites_workspace_doubles(0, 28) == -1 and lib.air_embed_sprites_workspace_doubles(4, 257) == -2
    assert lib.air_embed_sprites_workspace_doubles(1, 4) == 2 and lib.air_embed_sprites_workspace_doubles(2000, 28) == 512
    for m in (1, 2, 4, 5, 9, 10, 16, 17, 2000, 1 << 22):
        assert lib.air_embed_sprite_dim(m) == ec.sprite_dim(m) == math.isqrt(m - 1) + 1, m
    assert lib.air_embed_sprite_dim(0) == -1 and lib.air_embed_sprite_dim((1 << 22) + 1) == -2


def test_module_refuses_host_tensors(H):
    import torch
    from air import embeddings
    with pytest.raises(H.AirHipError):
        embeddings.sprite_sheet(torch.zeros(3, 4, 4))


# ------------------------------------------------------------------------------------------- hand-worked restatement
def test_hand_worked_match():
    assert ec.st_center(11, 11, 28, 28) == (0.0, 0.0)
    f = lambda rows: np.asarray(rows, np.float32)  # noqa: E731
    both = f([(3 / 32, 4 / 32), (-3 / 32, -4 / 32)])
    assert ec.candidate_distances((0.0, 0.0), both) == [5 / 32, 5 / 32]                    # exact
    assert ec.match_image([(0.0, 0.0)], both, 5 / 32) == [0]                                # the first: the minimum is strict; <=
    assert ec.match_image([(0.0, 0.0)], both[::-1], 5 / 32) == [0]
    assert ec.match_image([(0.0, 0.0)], both, float(np.nextafter(5 / 32, 0.0))) == [-1]
    # two digits share their closest object: the second is dropped although object 1 is within range of it
    centers = [ec.st_center(11, 11, 28, 28), ec.st_center(12, 11, 28, 28)]
    shifts = f([(1 / 64, 0.0), (1 / 8, 0.0)])
    d = ec.candidate_distances(centers[1], shifts)
    assert d[0] < d[1] < 5 / 32
    assert ec.match_image(centers, shifts, 5 / 32) == [0, -1]
    assert ec.match_image(centers[::-1], shifts, 5 / 32) == [0, -1]
    assert ec.match_image([(0.0, 0.0)], f(np.zeros((0, 2))), 5 / 32) == [-1]                # no inferred object
    assert ec.match_image([], both, 5 / 32) == []                                           # no digit
    assert ec.match_image([(0.0, 0.0)], f([(0.5, 0.5)]), 0.2) == [-1]                       # beyond max_distance
    assert ec.match_image([(0.0, 0.0)], f([(0.5, 0.5)]), 0.75) == [0]


def test_collect_lists_on_a_small_set():
    """image 0: two digits, both matched, in digit order; image 1: no digit; image 2: one digit, nothing inferred"""
    none = np.array([])
    rec_pos = [np.asarray([[0.5, 1 / 8, 0.0], [0.5, 0.0, 0.0]], np.float32), np.asarray([[0.5, 0.0, 0.0]], np.float32), none]
    lat = [np.asarray([[1.0, 2.0], [3.0, 4.0]], np.float32), np.asarray([[5.0, 6.0]], np.float32), none]
    win = [np.arange(8, dtype=np.float32).reshape(2, 2, 2), np.ones((1, 2, 2), np.float32), none]
    r = ec.collect_lists([2, 0, 1], [[70, 71], [], [72]], [[11, 11, 14, 11], [], [11, 11]], [[28, 28, 28, 28], [], [28, 28]],
                         [[7, 8], [], [9]], [2, 1, 0], rec_pos, win, lat, max_distance=0.2)
    assert r["ids"].tolist() == [70, 71] and r["labels"].tolist() == [7, 8]
    assert r["latents"].tolist() == [[3.0, 4.0], [1.0, 2.0]] and r["windows"][0].tolist() == [[4.0, 5.0], [6.0, 7.0]]
    assert (r["present"], r["inferred"], r["matched"]) == (3, 3, 2)


def test_planted_images_of_the_gpu_cases():
    cases = ec.gpu_cases()
    for name, below in (("chunks_z50_w28", False), ("chunks_z3_w5", False), ("below_tie_z3_w5", True)):
        case = cases[name]
        matches, counters, _ = ec.expected(case, 400, 400, ZEROS)
        flat = np.concatenate(matches)                     # [7, G]
        p = case["planted"]
        assert sorted(p) == sorted(ec.PLANTED) and len(set(p.values())) == 5
        assert flat[p["tie"]].tolist() == [-1 if below else 0, -1, -1]
        assert flat[p["shared"]].tolist() == [0, -1, -1]
        for k in ("no_objects", "no_digits", "too_far"):
            assert flat[p[k]].tolist() == [-1, -1, -1], k
        assert [c["k"] for c in case["chunks"]] == [5, 2] and counters[3] == 0 and counters[0] >= 2


def test_random_cases_keep_clear_of_rounding_ties():
    """The GPU tests compare with these cases bit for bit.  That is fair when no decision of the match hangs on the last bits
    of a distance: per digit no two candidate distances within 1e-9 of each other, none within 1e-9 of max_distance (the
    planted images tie on purpose, in numbers that are exact in float64)."""
    for name, case in ec.gpu_cases().items():
        pair, edge = ec.margins(case, skip=set(case["planted"].values()))
        print("%s: closest pair of distances %.3e, closest to max_distance %.3e" % (name, pair, edge))
        assert pair > 1e-9 and edge > 1e-9, name
        matches, counters, _ = ec.expected(case, 400, 400, ZEROS)
        assert 0 < counters[0] < counters[1] and counters[0] < counters[2], (name, counters)
    c = ec.gpu_cases()["b150_strided"]
    assert c["T"] == 16 and c["G"] == 16 and c["chunks"][0]["k"] == 150


# --------------------------------------------------------------------------------------------------------- grey levels
@pytest.fixture(scope="module")
def levels(golden_dir):
    return np.load(os.path.join(golden_dir, "sprite_levels.npz"))


def test_grey_levels_equal_matplotlibs(levels):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sprite_levels.npz")) < 100 * 1024
    table = levels["table"]
    assert table.dtype == np.uint8 and table.tobytes() == ec.grey_table().tobytes()
    off = np.nonzero(table != np.arange(256))[0]
    assert off[:3].tolist() == [33, 37, 41] and (table[off] == off - 1).all()           # not the identity
    shapes = []
    for c in range(5):
        windows, plane = levels["windows_%d" % c], levels["plane_%d" % c]
        shapes.append(windows.shape[:2])
        got = ec.sprite_levels(windows)
        assert got.dtype == np.uint8 and got.shape == plane.shape and got.tobytes() == plane.tobytes(), c
    assert shapes == [(1, 28), (5, 28), (9, 5), (10, 4), (3, 4)]
    assert not levels["windows_4"].any() and not levels["plane_4"].any()                 # hi == lo: all zeros
    assert (levels["plane_1"][56:, 56:] == 255).all()                                    # empty tiles are 1.0 = white


# ----------------------------------------------------------------------------------------------------- write_projector
def _decode_grey_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    i, idat, size = 8, b"", None
    while i < len(data):
        (n,), kind = struct.unpack(">I", data[i:i + 4]), data[i + 4:i + 8]
        body = data[i + 8:i + 8 + n]
        if kind == b"IHDR":
            w, h, depth, color = struct.unpack(">IIBB", body[:10])
            assert (depth, color) == (8, 0)
            size = (h, w)
        elif kind == b"IDAT":
            idat += body
        i += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], size[1] + 1)
    assert not rows[:, 0].any()                                # filter 0
    return rows[:, 1:]


def test_write_projector_on_host_arrays(tmp_path):
    from air import embeddings
    import tf_checkpoint
    import tf_events
    rng = np.random.RandomState(5)
    M, Z, w = 7, 50, 28
    windows = rng.uniform(0, 1, (M, w, w)).astype(np.float32)
    res = embeddings.Embeddings(rng.standard_normal((M, Z)).astype(np.float32), windows,
                                rng.randint(0, 10, M).astype(np.int32), np.arange(M, dtype=np.int32), 9, 8, M,
                                sprites=ec.sprite_levels(windows))
    folder = str(tmp_path / "proj")
    paths = embeddings.write_projector(folder, res)
    assert sorted(os.listdir(folder)) == sorted(["mnist_metadata.tsv", "mnist_sprites.png", "embeddings.index",
                                                 "embeddings.data-00000-of-00001", "checkpoint", "projector_config.pbtxt",
                                                 os.path.basename(paths["events"])])
    back = tf_checkpoint.load_checkpoint(os.path.join(folder, "embeddings"))
    assert list(back) == ["air_mnist"] and back["air_mnist"].dtype == np.float32 and back["air_mnist"].shape == (M, Z)
    assert back["air_mnist"].tobytes() == res.latents.tobytes()
    want = ('embeddings {\n  tensor_name: "air_mnist:0"\n  metadata_path: "%s/mnist_metadata.tsv"\n  sprite {\n'
            '    image_path: "%s/mnist_sprites.png"\n    single_image_dim: 28\n    single_image_dim: 28\n  }\n}\n' % (folder, folder))
    assert os.path.isabs(folder) and open(paths["config"]).read() == want
    tsv = open(paths["metadata"]).read().split("\n")
    assert tsv[0] == "Index\tLabel" and tsv[-1] == "" and len(tsv) - 1 == M + 1
    assert tsv[1:-1] == ["%d\t%d" % (i, l) for i, l in enumerate(res.labels)]
    png = open(paths["sprites"], "rb").read()
    assert _decode_grey_png(png).tobytes() == res.sprites.tobytes()
    assert 'model_checkpoint_path: "%s/embeddings"' % folder in open(paths["state"]).read()
    ev = tf_events.read_events(paths["events"])
    assert len(ev) == 1 and ev[0]["file_version"] == "brain.Event:2"
