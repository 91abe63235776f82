"""CPU-side checks of what carries the evaluation instruments (air/metrics.py's protocol, training.py's SummaryWriter /
TensorBoardWriter, the test-set record, multi_mnist.padded): what a driver reads from an instrument, the one rule that turns
its values into the fields of a row, what reaches the event file, the record load_data returns and its one permutation,
and the one padding helper against arrays written out by hand.  (The instruments through the driver loop on a device:
tests/test_gpu_eval_instruments.py; what each kernel computes and every refusal: the tests of each instrument.)"""
import types

import numpy as np
import pytest

import multi_mnist as mm
import tf_events

NAN = float("nan")
# class name -> row prefix, TensorBoard group, reported keys, whether a NaN is written to the event file
PROTOCOL = {
    "Localization": ("loc_", "localization/", ("mean_iou", "recall", "precision", "cover", "center_dist"), True),
    "Segmentation": ("seg_", "segmentation/", ("fg_ari", "mask_iou", "fg_missed", "bg_claimed"), True),
    "LatentProbe": ("lat_", "latents/", ("knn_accuracy", "active_units", "scored", "matched_share"), False),
}


@pytest.fixture(scope="module")
def training():
    import training
    return training


@pytest.mark.parametrize("name", sorted(PROTOCOL))
def test_protocol_is_the_declared_one(name):
    from air import metrics
    cls = getattr(metrics, name)
    prefix, group, reported, nan_in_events = PROTOCOL[name]
    assert (cls.prefix, cls.group, tuple(cls.reported), cls.nan_in_events) == (prefix, group, reported, nan_in_events)
    names = cls.names()
    assert isinstance(names, list) and set(reported) <= set(names)
    assert [k for k in names if k in reported] == list(reported)            # the same relative order
    assert names == list({"Localization": metrics.NAMES, "Segmentation": metrics.SEG_NAMES, "LatentProbe": metrics.PROBE_NAMES}[name])
    assert callable(cls.evaluate)
    assert "count_accuracy" in metrics.Localization.names() and "count_accuracy" not in metrics.Localization.reported


def test_row_fields_of_localization(training):
    from air.metrics import Localization
    got = training.row_fields(Localization, [0.123456, NAN, 1.0, 0.5, 2.0, 0.75])
    assert got == {"loc_mean_iou": 0.12346, "loc_recall": None, "loc_precision": 1.0, "loc_cover": 0.5, "loc_center_dist": 2.0}
    assert list(got) == ["loc_mean_iou", "loc_recall", "loc_precision", "loc_cover", "loc_center_dist"]
    assert "loc_count_accuracy" not in got


def test_event_file_takes_group_keys_and_the_nan_rule_from_the_instrument(training, tmp_path):
    from air.metrics import LatentProbe, Localization
    model = types.SimpleNamespace(max_steps=3, max_digits=2, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                                  scope="air")
    board = training.TensorBoardWriter(str(tmp_path), model, model)
    board.instrument(50, LatentProbe, [NAN, 7.0, 0.0, 0.25])
    board.instrument(100, Localization, [0.5, NAN, 1.0, 0.25, 2.0])
    board.close()
    ev = tf_events.read_events(board.events.path, verify=True)
    assert [e["step"] for e in ev[1:]] == [50, 100]
    probe, loc = ([(v["tag"], v["simple_value"]) for v in e["summary"]] for e in ev[1:])
    assert probe == [("latents/active_units", 7.0), ("latents/scored", 0.0), ("latents/matched_share", 0.25)]
    assert [t for t, _ in loc] == ["localization/" + k for k in ("mean_iou", "recall", "precision", "cover", "center_dist")]
    assert [v for _, v in loc if v == v] == [0.5, 1.0, 0.25, 2.0] and loc[1][1] != loc[1][1]      # the NaN as NaN


def _cache(folder, keys, G=2):
    """the 4-image cache of the refusal tests, and of positions, boxes and labels what `keys` names"""
    data = folder / "multi_mnist_data"
    data.mkdir()
    truth = dict(positions=np.arange(4 * 2 * G, dtype=np.int64).reshape(4, 2 * G), boxes=np.arange(4 * 2 * G).reshape(4, 2 * G) + 100,
                 labels=np.arange(4 * G, dtype=np.int64).reshape(4, G) % 10)
    for name in ("common.npz", "test.npz"):
        np.savez(str(data / name), images=np.zeros((4, 2500), np.float32), digits=np.asarray([1, 0, 2, 0], np.int32),
                 **{k: truth[k] for k in keys})
    return truth


def test_load_data_returns_the_cached_test_set_as_one_record(training, tmp_path, monkeypatch):
    truth = _cache(tmp_path, ("positions", "boxes", "labels"))
    monkeypatch.chdir(tmp_path)
    assert training.cache_without(("positions", "boxes", "labels")) is None
    train_images, train_digits, test = training.load_data(want=("positions", "boxes", "labels"))
    assert train_images.shape == (4, 2500) and train_digits.tolist() == [1, 0, 2, 0]
    assert set(test) == {"images", "digits", "positions", "boxes", "labels"}
    assert test["images"].shape == (4, 2500) and test["digits"].tolist() == [1, 0, 2, 0]
    for k in ("positions", "boxes"):
        assert test[k].shape == (4, 2, 2) and test[k].dtype == np.int32 and np.array_equal(test[k].reshape(4, -1), truth[k])
    assert test["labels"].shape == (4, 2) and test["labels"].dtype == np.int32 and np.array_equal(test["labels"], truth["labels"])
    assert set(training.load_data()[2]) == {"images", "digits"}
    assert set(training.load_data(want=("positions", "boxes"))[2]) == {"images", "digits", "positions", "boxes"}


def test_cache_without_names_the_file_that_lacks_a_key(training, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert training.cache_without(("positions", "boxes")) is None            # no cache at all: nothing to refuse
    _cache(tmp_path, ("positions", "boxes"))
    assert training.cache_without(("positions", "boxes")) is None and training.cache_without(()) is None
    assert training.cache_without(("positions", "boxes", "labels")) == training.TEST_DATA_FILE
    assert training.cache_without(("labels",)) == training.TEST_DATA_FILE


def test_every_entry_of_the_record_follows_the_one_permutation(training):
    digits = np.asarray([1, 0, 2, 0], np.int32)
    order = mm.shift_zero_digits_order(digits)
    assert order.tolist() == [1, 0, 2, 3]
    test = dict(images=np.arange(12, dtype=np.float32).reshape(4, 3), digits=digits,
                positions=np.arange(16, dtype=np.int32).reshape(4, 2, 2), boxes=np.arange(16, dtype=np.int32).reshape(4, 2, 2) + 50,
                labels=np.arange(8, dtype=np.int32).reshape(4, 2), masks=np.arange(20, dtype=np.uint8).reshape(4, 5))
    kept = {k: a.copy() for k, a in test.items()}
    got = training.shifted(test)
    assert set(got) == set(test)
    for k, a in got.items():
        assert np.array_equal(a, kept[k][[1, 0, 2, 3]]) and a.dtype == kept[k].dtype and a.flags["C_CONTIGUOUS"], k
        assert np.array_equal(test[k], kept[k]), k                             # the record handed in is left as it was
    images, shifted_digits = mm.shift_zero_digits_images(kept["images"], kept["digits"])
    assert np.array_equal(got["images"], images) and np.array_equal(got["digits"], shifted_digits)
    assert got["digits"].tolist() == [0, 1, 2, 0]
    # no empty image: the identity, for every entry
    full = dict(images=np.arange(6.0).reshape(3, 2), digits=np.asarray([2, 1, 1]))
    assert mm.shift_zero_digits_order(full["digits"]).tolist() == [0, 1, 2]
    assert all(np.array_equal(a, full[k]) for k, a in training.shifted(full).items())


def test_padded_is_the_three_helpers_it_replaces():
    """expected arrays written out by hand: what padded_truth (width 2), padded_labels and the projector export's helper
    (width 1 and 2, G given) returned"""
    pairs, singles, counts = [[1, 2, 3, 4], [], [5, 6]], [[7, 8], [], [9]], [2, 0, 1]
    want2 = [[[1, 2], [3, 4]], [[0, 0], [0, 0]], [[5, 6], [0, 0]]]
    want1 = [[[7], [8]], [[0], [0]], [[9], [0]]]
    for G in (None, 2):                                                        # the largest count | given
        got2, got1 = mm.padded(pairs, counts, 2, G), mm.padded(singles, counts, 1, G)
        assert got2.dtype == got1.dtype == np.int32 and got2.shape == (3, 2, 2) and got1.shape == (3, 2, 1)
        assert got2.tolist() == want2 and got1.tolist() == want1
        assert mm.padded_truth(pairs, counts, G).tolist() == want2
        assert mm.padded_labels(singles, counts, G).tolist() == [[7, 8], [0, 0], [9, 0]]
    # max_digits larger than the largest count: rows of zeros behind
    assert mm.padded(pairs, counts, 2, 3).tolist() == [row + [[0, 0]] for row in want2]
    assert mm.padded(singles, counts, 1, 4).tolist() == [row + [[0], [0]] for row in want1]
    assert mm.padded_labels(singles, counts, 3).tolist() == [[7, 8, 0], [0, 0, 0], [9, 0, 0]]
    # values behind an image's digits are not read; numpy arrays serve as lists
    assert mm.padded([np.asarray([1, 2, 3, 4, 9, 9], np.int32)], [2], 2).tolist() == [[[1, 2], [3, 4]]]
    assert mm.padded([np.asarray([7, 8, 9])], np.asarray([1]), 1).tolist() == [[[7]]]
    # a list shorter than the counts (the blank canvases that fill a last batch): only rows with a count are read
    assert mm.padded(pairs, counts + [0, 0], 2, 2).tolist() == want2 + [[[0, 0], [0, 0]]] * 2
    # no image at all, nothing but empty images, max_digits = 0: one column of zeros
    for width in (1, 2):
        assert mm.padded([], [], width).shape == (0, 1, width) and mm.padded([], [], width, 3).shape == (0, 3, width)
        assert mm.padded([[], []], [0, 0], width).tolist() == [[[0] * width]] * 2
        assert mm.padded([[], []], [0, 0], width, 0).shape == (2, 1, width)
    assert mm.padded_truth([], []).shape == (0, 1, 2) and mm.padded_labels([], []).shape == (0, 1)
    out = mm.padded_labels(singles, counts)
    assert out.flags["C_CONTIGUOUS"] and out.dtype == np.int32
