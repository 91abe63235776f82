"""The contract the two banks and the scene source share (air/sources.py: _Bank, _Feed, _FixedBank), on the GPU, at the smallest
shapes that exercise them: 12 ragged 8 x 8 glyphs, V = 8 variants in 16 x 16 frames (ink = 10 for the handwriting bank),
non-neutral bounds, scenes of B = 4 canvases of 24 x 24.  What the kernels compute is pinned elsewhere
(tests/test_gpu_glyph_jitter.py, tests/test_gpu_glyph_distort.py, tests/test_gpu_scene_source.py); here a batch is held against
the scene restatement of tests/scene_source_cases.py fed the glyph table the source itself read."""
import numpy as np
import pytest
import torch

import glyph_distort_cases as gd
import scene_source_cases as sc

pytestmark = pytest.mark.gpu

V, OD, INK, B, CANVAS, MD, SEED = 8, 16, 10, 4, 24, 2, 77
BANKS = {       # name: (class name, params width, extra input, constructor keywords)
    "jitter": ("DeviceGlyphBank", 6, "crops", dict(min_w=0.9, max_w=1.1, min_h=0.9, max_h=1.1, min_ang=-15.0, max_ang=15.0)),
    "handwriting": ("DeviceHandwritingBank", 8, "taps", dict(gd.MNIST_LIKE, sigma=2.0, alpha=0.6, ink=INK)),
}


def _glyphs():
    return sc.ragged_glyphs().reshape(12, 64)


def _source(sources, table, seed=SEED):
    dev = torch.device("cuda", 0)
    images, digits = torch.zeros(B, CANVAS * CANVAS, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    return sources.DeviceSceneSource(table, B, images, digits, canvas_dim=CANVAS, max_digits=MD, gap=1, seed=seed), images, digits


def _batch_is_the_restatements(src, images, digits, batch):
    """the source's output buffers and meta() against compose_batch on the glyph table the source read; -> the digits"""
    torch.cuda.synchronize()
    frames, crops = src.glyphs.cpu().numpy(), src.crops.cpu().numpy()
    side = int(round(np.sqrt(frames.shape[1])))
    ref = sc.compose_batch(B, batch, frames.reshape(len(frames), side, side), crops, CANVAS, 0, 1, MD, 100, 32, SEED)
    got = dict(images=images.cpu().numpy(), digits=digits.cpu().numpy(), **{k: v.cpu().numpy() for k, v in src.meta().items()})
    for k in ("images", "digits", "indices", "positions", "boxes", "status"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (batch, k)
    assert (got["status"] >= 0).all() and (got["images"].any(1) == (got["digits"] > 0)).all()
    return got["digits"]


def _refuses_eager_batches_after_graph_hooks(src):
    between, after = src.graph_hooks(2)
    assert callable(between) and after is None
    with pytest.raises(RuntimeError, match="this source feeds a captured graph"):
        src.next_batch()
    with pytest.raises(RuntimeError, match="this source feeds a captured graph"):
        src.fresh_batch()
    with pytest.raises(ValueError, match="set up for 2 steps"):
        src.graph_hooks(3)


@pytest.mark.parametrize("kind", sorted(BANKS))
def test_bank_contract(kind):
    from air import sources
    name, width, extra, kw = BANKS[kind]
    dev = torch.device("cuda", 0)
    bank = getattr(sources, name)(_glyphs(), V, od=OD, seed=SEED, device=dev, **kw)
    assert (bank.variants, bank.gd, bank.od, bank.device) == (V, 8, OD, dev) and type(bank).params_width == width
    assert bank.params.shape == (V, width) and bank.params.dtype == torch.float64
    assert bank.bank.shape == (V, OD * OD) and bank.bank.dtype == torch.float32
    assert bank.bank_crops.shape == (V, 4) and bank.source.shape == (V,) and bank.status.shape == (V,)
    assert all(t.dtype == torch.int32 for t in (bank.bank_crops, bank.source, bank.status)) and bank.counter.dtype == torch.int64
    assert bank.glyphs.shape == (12, 64) and torch.is_tensor(getattr(bank, extra)) and getattr(bank, extra).device == dev
    assert bank.status_counts().tolist() == [0, V, 0] and int(bank.counter) == 0      # nothing is usable before the first refresh
    bank.refresh()
    first = bank.bank.clone()
    bank.refresh()
    torch.cuda.synchronize()
    assert int(bank.counter) == 2 and not torch.equal(first, bank.bank)               # every generation is another bank
    counts = bank.status_counts()
    assert counts.shape == (3,) and int(counts.sum()) == V and int(counts[0]) > 0
    assert np.array_equal(counts.cpu().numpy(), np.bincount(bank.status.cpu().numpy(), minlength=3))
    base = np.arange(100, 112)
    source = bank.source.cpu().numpy()
    assert ((0 <= source) & (source < 12)).all() and np.array_equal(bank.labels(base), base[source])
    assert bank.fits(CANVAS, 0) is True and bank.fits(CANVAS, 12) is False

    src, images, digits = _source(sources, bank)
    assert src.bank is bank and src.glyphs is bank.bank and src.crops is bank.bank_crops
    src.next_batch()                                                                  # (does not refresh)
    _batch_is_the_restatements(src, images, digits, 0)
    assert int(bank.counter) == 2 and int(src.counter) == 1
    src.fresh_batch()                                                                 # the bank turned over, then a batch of it
    _batch_is_the_restatements(src, images, digits, 1)
    assert int(bank.counter) == 3 and int(src.counter) == 2 and int(src.gave_up()) == 0
    _refuses_eager_batches_after_graph_hooks(src)
    assert int(bank.counter) == 3 and int(src.counter) == 2                           # a refusal launched nothing


def test_plain_glyph_array_under_the_same_source():
    """the same seed on the plain array: the one constructor path, no bank to show, and the scenes' digit counts -- the first
    draw of every scene -- are those of a source on a bank"""
    from air import sources
    dev = torch.device("cuda", 0)
    src, images, digits = _source(sources, _glyphs())
    assert src.bank is None and src.glyphs.shape == (12, 64) and src.glyphs.dtype == torch.float32
    assert np.array_equal(src.crops.cpu().numpy(), sources.crop_boxes(_glyphs(), 8)) and src.crops.dtype == torch.int32
    src.next_batch()
    plain = _batch_is_the_restatements(src, images, digits, 0)
    src.fresh_batch()                                                                 # nothing to turn over: next_batch()
    _batch_is_the_restatements(src, images, digits, 1)
    assert int(src.counter) == 2 and int(src.gave_up()) == 0

    bank = sources.DeviceGlyphBank(_glyphs(), V, od=OD, seed=SEED, device=dev, **BANKS["jitter"][3])
    on_bank, bank_images, bank_digits = _source(sources, bank)
    on_bank.fresh_batch()
    assert np.array_equal(_batch_is_the_restatements(on_bank, bank_images, bank_digits, 0), plain)
    _refuses_eager_batches_after_graph_hooks(src)
    with pytest.raises(ValueError, match="no glyph fits a 24 x 24 canvas with margin 11"):
        sources.DeviceSceneSource(_glyphs(), B, images, digits, canvas_dim=CANVAS, max_digits=MD, margin=11)
