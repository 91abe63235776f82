"""CPU-side checks of air/sources.py as a module: multi_mnist re-exports its public names as the same objects and stays
importable without torch or the library; what each bank declares to the common constructor; the steps latch of the feed
protocol on stub feeds that launch nothing; the plain glyph array as the bank that never turns over.  (The constructors'
refusals, in their order: tests/test_glyph_jitter_abi.py, tests/test_glyph_distort_abi.py, tests/test_scene_source_abi.py;
the queue's picks: tests/test_shuffle_queue.py; the classes on a device: tests/test_gpu_data_sources.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_source_cases as sc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tf-attend-infer-repeat_amd")
REEXPORTED = ("DeviceSceneSource", "DeviceGlyphBank", "DeviceHandwritingBank", "ShuffleBatchQueue", "crop_boxes",
              "gaussian_taps", "JITTER_NEUTRAL", "MNIST_LIKE")


def test_multi_mnist_reexports_the_same_objects():
    import multi_mnist as mm
    from air import sources
    for name in REEXPORTED:
        assert getattr(mm, name) is getattr(sources, name), name


def test_import_multi_mnist_loads_neither_torch_nor_the_library():
    code = ("import sys; import multi_mnist; "
            "print([m for m in ('torch', 'air._hip') if m in sys.modules]); print('air.sources' in sys.modules)")
    p = subprocess.run([sys.executable, "-c", code], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-500:]
    assert p.stdout.split("\n")[:2] == ["[]", "True"], p.stdout


def test_each_bank_declares_what_differs():
    from air import _hip as H
    from air import sources
    jitter, writing = sources.DeviceGlyphBank, sources.DeviceHandwritingBank
    assert (jitter.params_width, writing.params_width) == (6, 8)
    assert (jitter.extra, writing.extra) == ("crops", "taps")
    assert (jitter.struct, jitter.entry, jitter.prepare) == ("GlyphJitter", "air_glyph_jitter", "air_glyph_jitter_prepare")
    assert (writing.struct, writing.entry, writing.prepare) == ("GlyphDistort", "air_glyph_distort", "air_glyph_distort_prepare")
    for bank in (jitter, writing):
        assert issubclass(bank, sources._Bank) and "refresh" not in vars(bank) and "labels" not in vars(bank)
        fields = [k for k, _ in getattr(H, bank.struct)._fields_]
        assert bank.extra in fields and "counter" in fields                     # the names _make fills exist in the descriptor
        assert bank.entry in H._SIGNATURES and bank.prepare in H._SIGNATURES


class _StubFeed:
    """mixed into a feed base subclass below: launches nothing, counts what would have been launched"""
    def __init__(self):
        self.eager, self.hooked = 0, []

    def _eager(self):
        self.eager += 1

    def _between(self, steps):
        self.hooked.append(steps)
        return lambda i: None


def _stub(noun):
    from air import sources
    return type("Stub", (_StubFeed, sources._Feed), {"noun": noun})()


@pytest.mark.parametrize("noun", ["queue", "source", "stub"])
def test_the_steps_latch_on_a_stub_feed(noun):
    feed = _stub(noun)
    feed.next_batch()
    feed.next_batch(3)                                                           # (the step index a driver may pass is ignored)
    assert feed.eager == 2
    for steps in (0, -1):
        with pytest.raises(ValueError, match="steps per replay must be positive"):
            feed.graph_hooks(steps)
    feed.next_batch()                                                            # a refused graph_hooks latched nothing
    assert feed.eager == 3 and feed.hooked == []
    between, after = feed.graph_hooks(5)
    assert callable(between) and after is None and feed.hooked == [5]
    with pytest.raises(ValueError, match="graph_hooks was set up for 5 steps per replay"):
        feed.graph_hooks(4)
    with pytest.raises(ValueError, match="positive"):
        feed.graph_hooks(0)
    feed.graph_hooks(5)                                                          # the same steps again: hooks again
    assert feed.hooked == [5, 5]
    with pytest.raises(RuntimeError, match="this %s feeds a captured graph \\(graph_hooks\\)" % noun):
        feed.next_batch()
    assert feed.eager == 3


def test_the_two_feeds_keep_their_nouns():
    from air import sources
    assert sources.ShuffleBatchQueue.noun == "queue" and sources.DeviceSceneSource.noun == "source"
    for feed in (sources.ShuffleBatchQueue, sources.DeviceSceneSource):
        assert issubclass(feed, sources._Feed) and "next_batch" not in vars(feed) and "graph_hooks" not in vars(feed)


def test_a_plain_glyph_array_is_the_bank_that_never_turns_over():
    from air import sources
    glyphs = sc.ragged_glyphs()                                                  # 12 glyphs of 8 x 8, boxes of 4 .. 7 pixels a side
    flat = glyphs.reshape(12, 64)
    crops = sources.crop_boxes(flat, 8)
    inline = lambda canvas_dim, margin: bool(np.any((crops[:, 2] + 2 * margin <= canvas_dim) & (crops[:, 3] + 2 * margin <= canvas_dim)))
    for given in (flat, glyphs):                                                 # [G, gd * gd], or anything that reshapes to it
        fixed = sources._FixedBank(given, "cpu")
        assert (fixed.variants, fixed.od) == (12, 8)
        assert fixed.bank.shape == (12, 64) and fixed.bank.dtype.is_floating_point and np.array_equal(fixed.bank.numpy(), flat)
        assert np.array_equal(fixed.bank_crops.numpy(), crops) and fixed.bank_crops.numpy().dtype == np.int32
        assert fixed.fits(16, 0) is True and inline(16, 0) is True
        assert fixed.fits(16, 7) is False and inline(16, 7) is False             # 16 - 14 = 2 pixels of room, the smallest box is 4
        smallest = int(np.maximum(crops[:, 2], crops[:, 3]).min())               # the threshold itself, from both sides
        assert fixed.fits(smallest, 0) is True and fixed.fits(smallest - 1, 0) is False
        for canvas_dim in range(3, 12):
            for margin in range(0, 3):
                assert fixed.fits(canvas_dim, margin) == inline(canvas_dim, margin), (canvas_dim, margin)
        assert fixed.refresh() is None
    with pytest.raises(ValueError, match="empty"):
        sources._FixedBank(np.zeros((2, 64), np.float32), "cpu")
    with pytest.raises(ValueError, match="gd \\* gd"):
        sources._FixedBank(flat[:, :63], "cpu")


def test_the_8x8_digits_have_one_loader():
    import multi_mnist as mm
    small, labels = mm.load_digits8x8()
    assert small.shape == (1797, 8, 8) and small.dtype == np.float32 and 0.0 <= small.min() and small.max() == 1.0
    assert labels.shape == (1797,) and labels.dtype == np.int64 and set(labels) == set(range(10))
    base, base_labels = mm.load_base_glyphs(16)
    assert base.shape == (1797, 256) and np.array_equal(base_labels, labels)
    if not any(os.path.exists(os.path.join(mm.MNIST_FOLDER, n)) for n in ("train-images-idx3-ubyte", "train-images-idx3-ubyte.gz")):
        standin, standin_labels, source = mm.load_glyphs()
        assert source == "digits8x8" and standin.shape == (1797, 784) and np.array_equal(standin_labels, labels)
