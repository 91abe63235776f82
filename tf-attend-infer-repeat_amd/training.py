"""Training driver -- counterpart of the reference's training.py on the HIP AIRModel.

Same constants (training.py:13-31), same CLI flags (-r/-o/-t, :35-39), same results-folder
layout (:41-61), the same constructor call (:100-122), train + test models sharing variables
(:95-123), periodic evaluation on the fixed 1 000-image test set with the
shift_zero_digits_images ordering (:143-156, 169-200), checkpoints every 10 000 iterations
(:203-207) and the same stdout line (:226).  TensorBoard summaries become JSONL scalars
(summary/scalars.jsonl): loss, accuracy and the per-digit-count breakdown of
AIRModel._summarize_by_digit_count (air_model.py:160-182, 614-617).  With --tensorboard the reference's four summary
groups are also written to summary/events.out.tfevents.* (TensorBoardWriter; tf_events.py) at its cadences (:165-218).

The whole dataset lives in HBM.  A batch comes out of tf.train.shuffle_batch's queue, kept on the
device (air.sources.ShuffleBatchQueue; multi_mnist.py:240-249: capacity 10 000 + 10 * batch, min_after_dequeue
10 000, over the epoch-repeating record stream of training.py:76-81) and is gathered into the train model's input
buffer; with --print-every 0 fifty train steps and their batches are one hipGraph replay (the queue's picks for the
fifty batches in its first launch, a row gather in front of every step), and the evaluation every 50 iterations is one replay of the
test model's forward + one summaries launch whose numbers are fetched without blocking (SummaryWriter).

--online-data replaces the queue and the train set by air.sources.DeviceSceneSource: the generator's default path as one
launch per step that composes a fresh batch into the train model's input buffers (inside the replay when there is one), so
no canvas is trained on twice; the evaluation set stays the fixed one.  The run ends with a line that says how many
batches were composed and how many canvases the bounded rejection sampler gave up on.  With the generator's scale /
rotation flags (--min-width-scale ... --max-rotation-angle) the digits come from a bank of --jitter-bank jittered glyphs
(air.sources.DeviceGlyphBank), remade on the device every --graph-steps steps -- by the replay itself when there is one, so
the batches are the same with and without --no-graph; the last line then also counts the banks and the unusable variants.
--glyph-style mnist-like takes the digits from an air.sources.DeviceHandwritingBank instead (the 8x8 handwritten digits
distorted on the device into MNIST's 20-in-28 geometry), remade at the same steps; the evaluation set is then 1 000 scenes
composed once on the device from a bank with a seed of its own, and the host generator does not run at all.
"""
import argparse
import json
import os
import shutil
import time

import numpy as np
import torch

from multi_mnist import (JITTER_NEUTRAL, DeviceGlyphBank, DeviceSceneSource, ShuffleBatchQueue, generate_dataset, handwriting_bank,
                         load_glyphs, padded_labels, padded_truth, shift_zero_digits_order)
from air.air_model import AIRModel

EPOCHS = 300
BATCH_SIZE = 64
CANVAS_SIZE = 50

NUM_SUMMARIES_EACH_ITERATIONS = 50
VAR_SUMMARIES_EACH_ITERATIONS = 250
IMG_SUMMARIES_EACH_ITERATIONS = 500
GRAD_SUMMARIES_EACH_ITERATIONS = 100
SAVE_PARAMS_EACH_ITERATIONS = 10000
NUM_IMAGES_TO_SAVE = 60

MIN_AFTER_DEQUEUE = 10000                 # multi_mnist.py:246-247 (capacity = this + 10 * batch)
DEFAULT_READER_THREADS = 4
ONLINE_TRAIN_SET_SIZE = 3 * 20000 - 1000   # generate_dataset's defaults: what an epoch counts where there is no train set
TEST_SET_SIZE = 1000
DEFAULT_RESULTS_FOLDER = "air_results"
TRAIN_DATA_FILE = "multi_mnist_data/common.npz"
TEST_DATA_FILE = "multi_mnist_data/test.npz"
# The test set is one record (load_data, device_test_set): `images` and `digits`, and what was asked for by name (`want`) --
# `positions` (x, y) and `boxes` (w, h) as int32 [n, G, 2], `labels` (the digits' classes) as int32 [n, G], zeros behind an
# image's digits, and the instance `masks` as uint8 [n, CANVAS_SIZE^2], which only a test set composed on the device has


def load_background(bg_path="", bg_max_intensity=1.0):
    """clutter (multi_mnist.py --bg-path / --bg-max-intensity): a png, or "<file>.npz:<key>", an already decoded background"""
    if not bg_path:
        return None
    if ".npz:" in bg_path:
        f, key = bg_path.rsplit(":", 1)
        bg = np.load(f)[key].astype(np.float32)
        if bg.max() > 0:
            bg = bg / bg.max() * min(bg_max_intensity, 1.0)
        return bg
    from multi_mnist import read_image
    return read_image(bg_path, bg_max_intensity)


def cache_without(keys):
    """the cached data set load_data would read, when its test file lacks one of `keys`; None otherwise"""
    if os.path.exists(TRAIN_DATA_FILE) and os.path.exists(TEST_DATA_FILE):
        with np.load(TEST_DATA_FILE) as te:
            if any(k not in te.files for k in keys):
                return TEST_DATA_FILE
    return None


def load_data(bg_path="", bg_max_intensity=1.0, want=()):
    """-> train images, train digits, the test-set record; want: which of positions, boxes and labels it also holds"""
    if os.path.exists(TRAIN_DATA_FILE) and os.path.exists(TEST_DATA_FILE):
        tr, te = np.load(TRAIN_DATA_FILE), np.load(TEST_DATA_FILE)
        test = dict(images=te["images"], digits=te["digits"])
        n = len(test["digits"])
        test.update({k: te[k].astype(np.int32).reshape((n, -1) if k == "labels" else (n, -1, 2)) for k in want})
        return tr["images"], tr["digits"], test
    rec_tr, rec_te = TRAIN_DATA_FILE.replace(".npz", ".tfrecords"), TEST_DATA_FILE.replace(".npz", ".tfrecords")
    if os.path.exists(rec_tr) and os.path.exists(rec_te):
        # the reference's own files (training.py:23-24: multi_mnist_data/common.tfrecords, test.tfrecords)
        from multi_mnist import read_test_data
        print("Reading the reference's TFRecord files...")
        tri, trd, *_ = read_test_data(rec_tr)
        tei, ted, _, *lists = read_test_data(rec_te)
        test = dict(images=tei, digits=ted.astype(np.int32))
        for k, lst in zip(("positions", "boxes", "labels"), lists):
            if k in want:
                test[k] = padded_labels(lst, ted) if k == "labels" else padded_truth(lst, ted)
        return tri, trd.astype(np.int32), test
    print("Generating multi-digit dataset in memory (multi_mnist.py defaults)...")
    ds = generate_dataset(bg=load_background(bg_path, bg_max_intensity))
    return ds["train_images"], ds["train_digits"], {k: ds["test_" + k] for k in ("images", "digits", *want)}


def device_test_set(dev, variants, seed, max_digits, margin, gap, bg, want=()):
    """--glyph-style mnist-like: TEST_SET_SIZE scenes composed once on the device from one handwriting bank with a seed of its
    own -> the test-set record as numpy arrays; the bank and the source are dropped.  want: which of these it also holds --
    source.meta()'s positions and boxes, int32 [n, max_digits, 2]; masks, the scenes' instance labels, uint8 [n,
    CANVAS_SIZE^2] (air.metrics.Segmentation.scene_masks: made here, while the bank's glyph table is still the one the scenes
    came from); labels, the classes of the scenes' digits, int32 [n, max_digits] (the base glyph of every variant the scenes
    drew, read here for the same reason; 0 behind an image's digits)"""
    images = torch.zeros(TEST_SET_SIZE, CANVAS_SIZE ** 2, device=dev)
    digits = torch.zeros(TEST_SET_SIZE, dtype=torch.int32, device=dev)
    bank, base_labels = handwriting_bank(variants, 0x54455354 + seed, dev)
    source = DeviceSceneSource(bank, TEST_SET_SIZE, images, digits, canvas_dim=CANVAS_SIZE, max_digits=max_digits, margin=margin,
                               gap=gap, bg=bg, seed=0x5445535453 + seed)
    source.fresh_batch()
    test = dict(images=images.cpu().numpy(), digits=digits.cpu().numpy())
    for k in ("positions", "boxes"):
        if k in want:
            test[k] = source.meta()[k].cpu().numpy().reshape(TEST_SET_SIZE, -1, 2)
    if "labels" in want:
        indices = source.meta()["indices"].cpu().numpy().reshape(TEST_SET_SIZE, -1)
        of_variant = bank.labels(base_labels).astype(np.int32)
        used = np.arange(indices.shape[1])[None, :] < test["digits"][:, None]
        test["labels"] = np.where(used, of_variant[np.clip(indices, 0, len(of_variant) - 1)], 0).astype(np.int32)
    if "masks" in want:
        from air.metrics import Segmentation
        test["masks"] = Segmentation.scene_masks(source, digits).cpu().numpy()
    return test


def shifted(test):
    """a test-set record in the order of shift_zero_digits_images: every entry follows the one permutation"""
    order = shift_zero_digits_order(test["digits"])
    return {k: np.ascontiguousarray(a[order]) for k, a in test.items()}


def reported_values(instrument, values):
    """{name: value} of the names an instrument reports, from its `values` (names() order)"""
    got = dict(zip(instrument.names(), values))
    return {k: got[k] for k in instrument.reported}


def row_fields(instrument, values):
    """what a row of scalars.jsonl gains from an instrument's `values`: the reported ones under its prefix, rounded, a NaN
    as null"""
    return {instrument.prefix + k: (round(v, 5) if v == v else None) for k, v in reported_values(instrument, values).items()}


class SummaryWriter:
    """The reference's numeric summaries (air_model.py:160-209, 608-625; training.py:171-180 evaluates them on the test
    model every NUM_SUMMARIES_EACH_ITERATIONS) as rows of summary/scalars.jsonl.  AIRModel.numeric_summaries() is one
    launch into a device vector; the vector is copied into a pinned host ring without blocking and a row is written
    when the NEXT evaluation has been enqueued, so the host never waits for the step it has just launched."""

    def __init__(self, model, path, t0, slots=2, on_row=None, instruments=(), on_values=None):
        """instruments: [(an air.metrics instrument of `model`, its ground truth on the device: evaluate()'s arguments)] --
        every evaluation is then also scored by each (a few launches behind the summaries one, the values fetched through
        a pinned ring of the instrument's own) and the row gains row_fields() of each, in list order;
        on_values(step, instrument, the values of its reported names) is called for each after on_row"""
        self.model, self.t0, self.on_row, self.on_values = model, t0, on_row, on_values
        self.names = model.summary_names()
        self.dev = torch.empty(len(self.names), dtype=torch.float32, device=model.input_images.device)
        self.host = torch.empty(slots, len(self.names), dtype=torch.float32).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(slots)]
        self.pending, self.k, self.file = [], 0, open(path, "w")
        self.instruments = [(instrument, truth, torch.empty(slots, len(instrument.names()), dtype=torch.float64).pin_memory())
                            for instrument, truth in instruments]

    def push(self, step):
        slot = self.k % len(self.events)
        self.k += 1
        self.model.numeric_summaries(self.dev)
        self.host[slot].copy_(self.dev, non_blocking=True)
        for instrument, truth, ring in self.instruments:
            instrument.evaluate(*truth)
            ring[slot].copy_(instrument.values(), non_blocking=True)
        self.events[slot].record()
        self.pending.append((slot, step))
        while len(self.pending) > 1:
            self._drain_one()

    def _drain_one(self):
        slot, step = self.pending.pop(0)
        self.events[slot].synchronize()
        row = {"step": step, "wall_s": round(time.perf_counter() - self.t0, 3)}
        row.update({k: (round(v, 5) if v == v else None) for k, v in zip(self.names, self.host[slot].tolist())})
        scored = [(instrument, ring[slot].tolist()) for instrument, _, ring in self.instruments]
        for instrument, values in scored:
            row.update(row_fields(instrument, values))
        self.file.write(json.dumps(row) + "\n")
        self.file.flush()
        if self.on_row is not None:
            self.on_row(step, self.host[slot].tolist())
        if self.on_values is not None:
            for instrument, values in scored:
                self.on_values(step, instrument, list(reported_values(instrument, values).values()))

    def flush(self):
        while self.pending:
            self._drain_one()


class TensorBoardWriter:
    """--tensorboard: the reference's four summary groups (training.py:144-149) as a TensorBoard event file in summary/,
    under its tags (air.summaries.summary_tags) and at its cadences and steps (:165-218):
      numeric    every 50 iterations, the numbers SummaryWriter has fetched anyway (its on_row hook; loss and accuracy, which
                 the reference does not summarise, are left out);
      variables  every 250: test_model.var_summaries(), one air_histograms call;
      image      every 500: the first num_summary_images reconstructions with their attention boxes (air/visualize.py);
      gradients  every 100: train_model.grad_summaries() after the train step, under the global step AFTER that step
                 (the `step` the reference fetches beside the train op, :212-218); with several steps per hipGraph replay
                 it is taken after the replay that contains the step and describes -- and is written under -- the LAST
                 step of that replay.
    Nothing blocks: every group is one or a few launches into a device buffer, a non-blocking copy into a pinned host
    buffer and an event; the bytes are decoded and written when a later fetch is enqueued (or at flush())."""

    def __init__(self, logdir, train_model, test_model, depth=2):
        import tf_events
        from air.summaries import summary_tags
        self.train_model, self.test_model, self.depth = train_model, test_model, depth
        m = test_model
        self.tags = summary_tags(m.max_steps, m.max_digits, m.vae_recognition_units, m.vae_generative_units, m.scope)
        self.events = tf_events.EventFileWriter(logdir)
        self.pending, self.slots, self.dev = [], {}, {}

    def _fetch(self, kind, dev, done):
        """`dev` -> a pinned host buffer of `kind` without blocking; done(host tensor) runs once the copy has landed"""
        if kind not in self.slots:
            self.slots[kind] = ([torch.empty(dev.shape, dtype=dev.dtype).pin_memory() for _ in range(self.depth)], [0])
        hosts, k = self.slots[kind]
        slot = k[0] % len(hosts)
        k[0] += 1
        while any(p[0] == (kind, slot) for p in self.pending):       # (the slot's previous fetch has to be written first)
            self._drain_one()
        hosts[slot].copy_(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append(((kind, slot), ev, done, hosts[slot]))
        while len(self.pending) > self.depth:
            self._drain_one()

    def _drain_one(self):
        _, ev, done, host = self.pending.pop(0)
        ev.synchronize()
        done(host)

    def numeric(self, step, values):
        """SummaryWriter's row of `step` (AIRModel.summary_names() order: loss, accuracy, then the reference's scalars)"""
        self.events.add_scalars(step, zip(self.tags.numeric, values[2:]))

    def instrument(self, step, instrument, values):
        """--localization, --segmentation, --latent-probe, --latent-clusters: the reported values of the evaluation at `step`, under the
        instrument's group (SummaryWriter's on_values hook); whether a NaN is written is the instrument's to say"""
        self.events.add_scalars(step, [(instrument.group + k, v) for k, v in zip(instrument.reported, values)
                                       if v == v or instrument.nan_in_events])

    def variables(self, step):
        from air.summaries import decode_histograms
        buf = self.dev["var"] = self.test_model.var_summaries(self.dev.get("var"))
        self._fetch("var", buf, lambda h: self.events.add_histograms(step, decode_histograms(h, self.tags.variables)))

    def image(self, step):
        from air import _hip as H
        from air.air_model import st_matrices
        from air.visualize import visualize_reconstructions
        m = self.test_model
        n = min(m.num_summary_images, m.batch_size)
        # every max_steps record (no read of T' on the host): a step the loop did not reach draws no box, no image has
        # more digits than steps were run (air_model.py:224-231 pads those steps with zeros)
        st_back = st_matrices(m.att[:, :n, H.ATT_ST_BACK:H.ATT_ST_BACK + 3].transpose(0, 1))
        img = visualize_reconstructions(m.input_images[:n], m.reconstruction[:n], st_back, m.rec_num_digits[:n],
                                        m.canvas_size, m.windows_size, m.max_steps, zoom=2).contiguous()
        tag = self.tags.image[0]
        self._fetch("img", img, lambda h: self.events.add_images(step, tag, h.numpy(), max_outputs=m.num_summary_images,
                                                                 png_level=1))

    def gradients(self, step):
        from air.summaries import decode_histograms, gradient_summaries
        buf = self.dev["grad"] = self.train_model.grad_summaries(self.dev.get("grad"))
        names = self.tags.gradients[::3]
        self._fetch("grad", buf, lambda h: self.events.add_summary(step, gradient_summaries(decode_histograms(h, names))))

    def flush(self):
        while self.pending:
            self._drain_one()
        self.events.flush()

    def close(self):
        self.flush()
        self.events.close()


def instruments(args, model, test):
    """--localization, --segmentation, --latent-probe, --latent-clusters -> [(the air.metrics instrument of `model`, its ground truth out of the
    test-set record on the device, headline)], in that order; headline(result()) -> what the run's last line about the
    instrument says in front of and behind its reported values, and the title of its confusion matrix (None: it has none)"""
    from air import metrics
    out = []
    if args.localization:
        loc = metrics.Localization(model, int(test["positions"].shape[1]), args.localization_iou)
        out.append((loc, (test["digits"], test["positions"], test["boxes"]), lambda res: (
            "localization at IoU {:g}: ".format(loc.iou_threshold), "",
            "count confusion (rows: digits present 0..{}, columns: objects inferred 0..{}):".format(loc.G, loc.T))))
    if args.segmentation:
        seg = metrics.Segmentation(model, args.online_max_digits, args.segmentation_threshold)
        out.append((seg, (test["masks"],), lambda res: ("segmentation at {:g}: ".format(seg.pred_threshold), "", None)))
    if args.latent_probe:
        lat = metrics.LatentProbe(model, int(test["labels"].shape[1]), k=args.latent_k)
        out.append((lat, (test["digits"], test["positions"], test["boxes"], test["labels"]), lambda res: (
            "latent probe, {}-NN over {} matched digits: ".format(lat.k, res["scored"]),
            "  (the store overflowed)" if res["overflow"] else "",
            "digit confusion (rows: true class 0..{}, columns: predicted):".format(lat.classes - 1))))
    if args.latent_clusters:
        clu = metrics.LatentClusters(model, int(test["labels"].shape[1]), clusters=args.cluster_count,
                                     restarts=args.cluster_restarts, seed=args.seed)
        out.append((clu, (test["digits"], test["positions"], test["boxes"], test["labels"]), lambda res: (
            "latent clusters, {}-means ({} restarts, best {} after {} iterations{}) over {} matched digits: ".format(
                clu.clusters, clu.restarts, res["best"], res["iters"], "" if res["converged"] else ", not converged", res["scored"]),
            "  (the store overflowed)" if res["overflow"] else "",
            "cluster table (rows: cluster 0..{}, columns: true class 0..{}):".format(clu.clusters - 1, clu.classes - 1))))
    if args.importance_samples:                 # LAST: its sampled passes replace the buffers the others read
        iw = metrics.ImportanceBound(model, args.importance_samples, seed=args.seed)
        out.append((iw, (test["digits"],), lambda res: (
            "importance bound, {} samples over {} images ({} degenerate): ".format(iw.K, res["scored"], res["degenerate"]), "",
            "count confusion (rows: digits present 0..{}, columns: the posterior's most likely count 0..{}):".format(iw.T, iw.T))))
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("-r", "--results-folder", default=DEFAULT_RESULTS_FOLDER)
    parser.add_argument("-o", "--overwrite-results", type=int, choices=[0, 1], default=0)
    parser.add_argument("-t", "--reader-threads", type=int, default=DEFAULT_READER_THREADS)   # kept for CLI parity
    parser.add_argument("--iterations", type=int, default=0, help="stop after this many iterations (0 = EPOCHS)")
    parser.add_argument("--print-every", type=int, default=1)
    parser.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    parser.add_argument("--no-graph", action="store_true")
    parser.add_argument("--tf-checkpoints", action="store_true",
                        help="also write TensorFlow bundles models/air-model-<step>.{index,data-00000-of-00001} (tf.train.Saver layout)")
    parser.add_argument("--bg-path", default="", help="clutter background for the in-memory dataset (png, or file.npz:key)")
    parser.add_argument("--bg-max-intensity", type=float, default=1.0)
    parser.add_argument("--graph-steps", type=int, default=50,
                        help="train steps per hipGraph replay when --print-every 0 (a divisor of 50)")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--tensorboard", action="store_true",
                        help="also write the reference's TensorBoard summaries to summary/events.out.tfevents.*: 88 scalars every "
                             "50 iterations, 36 variable histograms every 250, 60 reconstruction images every 500 (all at the "
                             "iteration's step, from the test model) and 216 gradient summaries every 100, taken after the train "
                             "step and written under the global step after it.  With --graph-steps > 1 (--print-every 0) the "
                             "gradient summary is taken after the replay that contains its step: it describes, and is written "
                             "under, the last step of that replay")
    parser.add_argument("--backward", default="reference", choices=["reference", "reference_carried", "exact"],
                        help="sampler backward: the reference graph's op order, the same streams with the long ones in 16 "
                             "carried chunks per tap, or the exact adjoint")
    parser.add_argument("--late-backward", default="", choices=["", "reference", "reference_carried", "exact"],
                        help="switch the sampler backward to this order from iteration --late-backward-from on "
                             "(AIRModel(backward=(first, late, iteration)))")
    parser.add_argument("--late-backward-from", type=int, default=5000,
                        help="(opt-in: over 48 seeds per precision no switch point keeps the reference order's success rate within 60 000 "
                             "iterations; over the full 276 300 the two end alike and this saves ~3 s -- DESIGN.md section 11.1)")
    parser.add_argument("--likelihood", default="bernoulli", choices=["bernoulli", "gaussian"],
                        help="pixel likelihood of the reconstruction loss: the reference's Bernoulli cross-entropy, or the AIR "
                             "paper's Gaussian around the clipped canvas with the fixed standard deviation vae_likelihood_std "
                             "(AIRModel(likelihood=...); the reported loss is then a density and may be negative)")
    parser.add_argument("--cnn", action="store_true",
                        help="the reference's conv front-end in front of the LSTM (AIRModel(cnn=True); the reference's own "
                             "training.py passes cnn=False)")
    parser.add_argument("--cnn-filters", type=int, default=8)
    parser.add_argument("--online-data", action="store_true",
                        help="compose every train batch on the device (air.sources.DeviceSceneSource: the generator's default "
                             "path, a fresh batch per step, no canvas seen twice) instead of drawing it from the fixed train set; "
                             "--bg-path applies; the evaluation set stays the fixed one")
    parser.add_argument("--online-max-digits", type=int, default=2, help="--online-data: scenes hold 0 .. this many digits")
    parser.add_argument("--digit-gap", type=int, default=0, help="--online-data: empty pixels kept between two digits")
    parser.add_argument("--canvas-margin", type=int, default=0, help="--online-data: empty border of the canvas")
    # --online-data: the generator's six jitter flags (multi_mnist.py:322-327); neutral values leave the run as it is
    parser.add_argument("--min-width-scale", type=float, default=1.0)
    parser.add_argument("--max-width-scale", type=float, default=1.0)
    parser.add_argument("--min-height-scale", type=float, default=1.0)
    parser.add_argument("--max-height-scale", type=float, default=1.0)
    parser.add_argument("--min-rotation-angle", type=float, default=0.0)
    parser.add_argument("--max-rotation-angle", type=float, default=0.0)
    parser.add_argument("--jitter-bank", type=int, default=4096, metavar="V",
                        help="--online-data with jitter: digits are drawn from a bank of V jittered glyphs made on the device "
                             "(air.sources.DeviceGlyphBank), a fresh bank every --graph-steps steps")
    parser.add_argument("--glyph-style", default="standin", choices=["standin", "mnist-like"],
                        help="--online-data: mnist-like draws the digits from a bank of --jitter-bank handwritten digits "
                             "distorted on the device into MNIST's geometry (air.sources.DeviceHandwritingBank: a 20-pixel "
                             "box centred in a 28-pixel frame), a fresh bank every --graph-steps steps; the evaluation set is "
                             "composed on the device too")
    parser.add_argument("--localization", action="store_true",
                        help="score the test model's attention boxes against the test set's ground-truth boxes at every "
                             "evaluation (air.metrics.Localization: box IoU, recall, precision, cover, centre distance): the "
                             "rows of summary/scalars.jsonl gain loc_* keys, --tensorboard gains localization/* scalars, and the "
                             "run ends with the confusion matrix of the counts")
    parser.add_argument("--localization-iou", type=float, default=0.5, help="--localization: the IoU from which a matched box is a hit")
    parser.add_argument("--segmentation", action="store_true",
                        help="score the test model's decomposition per pixel at every evaluation (air.metrics.Segmentation: "
                             "foreground adjusted Rand index, best mask IoU per digit, ink missed, background claimed) against "
                             "the instance masks of the test set: the rows of summary/scalars.jsonl gain seg_* keys and "
                             "--tensorboard gains segmentation/* scalars.  Needs --glyph-style mnist-like: the masks come from "
                             "the glyph table of the source that composes the test set on the device")
    parser.add_argument("--segmentation-threshold", type=float, default=0.5,
                        help="--segmentation: an object claims a pixel where its part of the reconstruction is above this")
    parser.add_argument("--latent-probe", action="store_true",
                        help="score the what-codes of the test model at every evaluation (air.metrics.LatentProbe: the leave-one-"
                             "out k-nearest-neighbour digit accuracy of the latent means of the matched digits, and the active "
                             "units): the rows of summary/scalars.jsonl gain lat_* keys, --tensorboard gains latents/* scalars, "
                             "and the run ends with the confusion matrix of the digits.  Needs the boxes and labels of the test set")
    parser.add_argument("--latent-k", type=int, default=5, help="--latent-probe: the neighbours that vote (1 .. 16)")
    parser.add_argument("--latent-clusters", action="store_true",
                        help="cluster the what-codes of the test model at every evaluation (air.metrics.LatentClusters: exact "
                             "k-means over the latent means of the matched digits, every cluster mapped to its majority class: "
                             "clustering accuracy, adjusted Rand index, NMI): the rows of summary/scalars.jsonl gain clu_* keys, "
                             "--tensorboard gains clusters/* scalars, and the run ends with the cluster x class table.  Needs "
                             "the boxes and labels of the test set, as --latent-probe does")
    parser.add_argument("--cluster-count", type=int, default=10, metavar="K", help="--latent-clusters: the clusters (1 .. 64)")
    parser.add_argument("--cluster-restarts", type=int, default=8, metavar="R",
                        help="--latent-clusters: the seeded starts of which the lowest inertia wins (1 .. 32)")
    parser.add_argument("--importance-samples", type=int, default=0, metavar="K",
                        help="score every evaluation by K passes of the test model on fresh noise as well (air.metrics."
                             "ImportanceBound; 0: off, at most 64): the K-sample importance-weighted bound on the negative "
                             "log-likelihood, the effective sample size and the posterior over the object count.  The rows of "
                             "summary/scalars.jsonl gain iw_* keys, --tensorboard gains importance/* scalars, and the run ends "
                             "with the confusion matrix of the most likely counts")
    args = parser.parse_args()
    if not 0 <= args.importance_samples <= 64:
        parser.error("--importance-samples must lie in 0 .. 64")
    if args.latent_probe and not 1 <= args.latent_k <= 16:
        parser.error("--latent-k must lie in [1, 16]")
    if args.latent_clusters and not 1 <= args.cluster_count <= 64:
        parser.error("--cluster-count must lie in [1, 64]")
    if args.latent_clusters and not 1 <= args.cluster_restarts <= 32:
        parser.error("--cluster-restarts must lie in [1, 32]")
    if args.latent_clusters and args.glyph_style != "mnist-like" and cache_without(("positions", "boxes", "labels")):
        parser.error("--latent-clusters needs the ground-truth boxes and digit labels of the test set, and %s holds none (no "
                     "'positions' / 'boxes' / 'labels'): regenerate the cache with multi_mnist.py (or multi_mnist.py --device N), "
                     "which writes them, or remove it to have the data set generated in memory"
                     % cache_without(("positions", "boxes", "labels")))
    if args.latent_probe and args.glyph_style != "mnist-like" and cache_without(("positions", "boxes", "labels")):
        parser.error("--latent-probe needs the ground-truth boxes and digit labels of the test set, and %s holds none (no "
                     "'positions' / 'boxes' / 'labels'): regenerate the cache with multi_mnist.py (or multi_mnist.py --device N), "
                     "which writes them, or remove it to have the data set generated in memory"
                     % cache_without(("positions", "boxes", "labels")))
    if args.segmentation and not 0.0 <= args.segmentation_threshold < 1.0:
        parser.error("--segmentation-threshold must lie in [0, 1)")
    if args.segmentation and args.glyph_style != "mnist-like":
        parser.error("--segmentation needs a test set composed on the device (--online-data --glyph-style mnist-like): the "
                     "instance masks come from the glyph table of the composing source, which a host-generated or cached "
                     "test set does not have")
    if args.localization and not 0.0 < args.localization_iou <= 1.0:
        parser.error("--localization-iou must lie in (0, 1]")
    if args.localization and args.glyph_style != "mnist-like" and cache_without(("positions", "boxes")):
        parser.error("--localization needs the ground-truth boxes of the test set, and %s holds none (no 'positions' / 'boxes'): "
                     "regenerate the cache with multi_mnist.py (or multi_mnist.py --device N), which writes them, or remove it "
                     "to have the data set generated in memory" % cache_without(("positions", "boxes")))
    jitter = dict(min_w=args.min_width_scale, max_w=args.max_width_scale, min_h=args.min_height_scale,
                  max_h=args.max_height_scale, min_ang=args.min_rotation_angle, max_ang=args.max_rotation_angle)
    mnist_like = args.glyph_style == "mnist-like"
    if mnist_like and not args.online_data:
        parser.error("--glyph-style mnist-like is made on the device: give --online-data")
    if mnist_like and jitter != JITTER_NEUTRAL:
        parser.error("--glyph-style mnist-like distorts the glyphs itself: leave the scale / rotation flags neutral")
    if args.cnn and args.tensorboard:
        parser.error("--tensorboard writes histogram summaries, which a --cnn model does not have yet")

    # results folder handling, training.py:41-61
    if os.path.exists(args.results_folder):
        if args.overwrite_results:
            shutil.rmtree(args.results_folder, ignore_errors=True)
        else:
            folder, i = args.results_folder, 0
            args.results_folder = "{}_{}".format(folder, i)
            while os.path.exists(args.results_folder):
                i += 1
                args.results_folder = "{}_{}".format(folder, i)
    models_folder = args.results_folder + "/models/"
    summaries_folder = args.results_folder + "/summary/"
    for d in (args.results_folder, models_folder, summaries_folder):
        os.makedirs(d)

    dev = torch.device("cuda", 0)
    want = (("positions", "boxes") if args.localization or args.latent_probe or args.latent_clusters else ()) + \
        (("labels",) if args.latent_probe or args.latent_clusters else ()) + (("masks",) if args.segmentation else ())
    print("Creating input pipeline...")
    if mnist_like:                                                   # no host generator: the test set is device work too
        test = device_test_set(dev, args.jitter_bank, args.seed, args.online_max_digits, args.canvas_margin, args.digit_gap,
                               load_background(args.bg_path, args.bg_max_intensity), want)
    else:
        tr_im, tr_dg, test = load_data(args.bg_path, args.bg_max_intensity, want)
    test = shifted(test)                                             # the ground truth follows the images' permutation
    test["digits"] = test["digits"].astype(np.int32)
    test = {k: torch.tensor(a, device=dev) for k, a in test.items()}
    if not args.online_data:
        train_images = torch.tensor(tr_im, device=dev)
        train_digits = torch.tensor(tr_dg.astype(np.int32), device=dev)
    test_data, test_targets = test["images"], test["digits"]
    train_data = torch.zeros(BATCH_SIZE, CANVAS_SIZE ** 2, device=dev)
    train_targets = torch.zeros(BATCH_SIZE, dtype=torch.int32, device=dev)

    backward = args.backward
    if args.late_backward and args.late_backward != args.backward:
        if args.late_backward_from < 0:
            parser.error("--late-backward-from must be >= 0")
        backward = (args.backward, args.late_backward, args.late_backward_from)
    models = []
    model_inputs = [[train_data, train_targets], [test_data, test_targets]]
    for i in range(2):
        print("Creating {0} model...".format("training" if i == 0 else "testing"))
        models.append(
            AIRModel(
                model_inputs[i][0], model_inputs[i][1],
                max_steps=3, max_digits=2, rnn_units=256, canvas_size=CANVAS_SIZE, windows_size=28,
                vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                scale_prior_mean=-1.0, scale_prior_variance=0.05, shift_prior_mean=0.0, shift_prior_variance=1.0,
                vae_prior_mean=0.0, vae_prior_variance=1.0, vae_likelihood_std=0.3,
                scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                z_pres_prior_log_odds=-0.01, z_pres_temperature=1.0, stopping_threshold=0.99,
                learning_rate=1e-4, gradient_clipping_norm=1.0, cnn=args.cnn, cnn_filters=args.cnn_filters,
                num_summary_images=NUM_IMAGES_TO_SAVE, train=(i == 0), reuse=(i == 1), scope="air",
                annealing_schedules={
                    "z_pres_prior_log_odds": {
                        "init": 10000.0, "min": 0.000000001,
                        "factor": 0.1, "iters": 3000,
                        "staircase": False, "log": True
                    },
                },
                seed=args.seed, gemm_precision=args.precision, backward=backward, likelihood=args.likelihood,
            )
        )
    train_model, test_model = models
    n_train = ONLINE_TRAIN_SET_SIZE if mnist_like else tr_im.shape[0]
    total = args.iterations if args.iterations > 0 else (n_train // BATCH_SIZE) * EPOCHS

    # The input queue is device work too (read_and_decode, multi_mnist.py:228-249): the RandomShuffleQueue's resident
    # record indices and the stream position live in HBM.  When nothing is printed per step, --graph-steps train steps
    # are captured per hipGraph replay together with their batches: one launch at the head of the replay makes the picks of
    # all its batches, one row gather sits in front of every step.
    # --online-data: no queue and no train set -- one launch in front of every step composes the step's batch from the
    # glyphs (same hooks: next_batch() eagerly, graph_hooks() inside the replay).
    bank = None
    if args.online_data:
        if mnist_like:
            bank, _ = handwriting_bank(args.jitter_bank, 0x4A4954 + args.seed, dev)
        elif jitter != JITTER_NEUTRAL:
            bank = DeviceGlyphBank(load_glyphs()[0], args.jitter_bank, seed=0x4A4954 + args.seed, device=dev, **jitter)
        batches = DeviceSceneSource(load_glyphs()[0] if bank is None else bank, BATCH_SIZE, train_data, train_targets, canvas_dim=CANVAS_SIZE,
                                    max_digits=args.online_max_digits, margin=args.canvas_margin, gap=args.digit_gap,
                                    bg=load_background(args.bg_path, args.bg_max_intensity), seed=0x5343454E45 + args.seed)
    else:
        batches = ShuffleBatchQueue(train_images, train_digits, BATCH_SIZE, train_data, train_targets,
                                    seed=0x5348554646 + args.seed, min_after_dequeue=MIN_AFTER_DEQUEUE)
    gsteps = 1
    if not args.no_graph:
        if args.print_every == 0 and NUM_SUMMARIES_EACH_ITERATIONS % args.graph_steps == 0 and args.graph_steps > 1:
            gsteps = args.graph_steps

    def capture():
        if args.no_graph:
            return
        if gsteps > 1:
            between, after = batches.graph_hooks(gsteps)
            train_model.capture_graph(steps=gsteps, between_steps=between, after_steps=after)
        else:
            train_model.capture_graph(steps=1)
    capture()
    if not args.no_graph:
        test_model.capture_graph()                                   # the evaluation pass: one replay

    print("Training...")
    print()
    step = 0
    order = train_model.backward
    t0 = time.perf_counter()
    board = TensorBoardWriter(summaries_folder, train_model, test_model) if args.tensorboard else None
    scored = instruments(args, test_model, test)
    writer = SummaryWriter(test_model, summaries_folder + "scalars.jsonl", t0, on_row=board.numeric if board else None,
                           instruments=[(instrument, truth) for instrument, truth, _ in scored],
                           on_values=board.instrument if board else None)
    while step < total:
        if step % NUM_SUMMARIES_EACH_ITERATIONS == 0:
            test_model.forward()
            writer.push(step)
            if board and step % VAR_SUMMARIES_EACH_ITERATIONS == 0:
                if step % IMG_SUMMARIES_EACH_ITERATIONS == 0:
                    if args.importance_samples:                       # (the model holds the last SAMPLED pass: the images are
                        test_model.forward()                          # those of the pass the other summaries describe)
                    board.image(step)
                board.variables(step)
        if step % SAVE_PARAMS_EACH_ITERATIONS == 0:
            torch.save(train_model.state_dict(), models_folder + "air-model-%d.pt" % step)
            if args.tf_checkpoints:                                   # training.py:203-207 saver.save(..., global_step)
                train_model.save_tf_checkpoint(models_folder + "air-model-%d" % step)
        if train_model.backward != order:                            # (a backward schedule: the model switched by itself)
            order = train_model.backward
            print("iteration {}: sampler backward order -> {}".format(step - gsteps, order))
        if gsteps == 1:
            if bank is not None and step % max(args.graph_steps, 1) == 0:      # (a replay of --graph-steps steps does it itself)
                bank.refresh()
            batches.next_batch()
        train_model.training()
        if board and step % GRAD_SUMMARIES_EACH_ITERATIONS == 0:
            board.gradients(step + gsteps)
        step += gsteps
        if args.print_every and step % args.print_every == 0:
            print("iteration {}\tloss {:.3f}\taccuracy {:.2f}".format(
                int(train_model.global_step), float(train_model.loss), float(train_model.accuracy)))
    torch.cuda.synchronize()
    writer.flush()
    if board:
        board.close()
    test_model.forward()
    print()
    print("training has ended")
    print("test accuracy {:.4f}  test loss {:.3f}  ({} iterations, {:.1f} s)".format(
        float(test_model.accuracy), float(test_model.loss), step, time.perf_counter() - t0))
    for instrument, truth, headline in scored:                       # the evaluation just made, the last of the run
        instrument.evaluate(*truth)
        res = instrument.result()
        lead, tail, matrix = headline(res)
        print(lead + "  ".join("{} {:.4f}".format(k, res[k]) for k in instrument.reported) + tail)
        if matrix:
            print(matrix)
            for row in res["confusion"]:
                print("  " + " ".join("{:6d}".format(int(v)) for v in row))
    if args.online_data:
        print("online data: {} batches composed on the device, {} canvases given up".format(
            int(batches.counter), int(batches.gave_up())) + ("" if bank is None else
            ", {} glyph banks of {} variants, {} unusable in the last".format(
                int(bank.counter), bank.variants, int(bank.status_counts()[1:].sum()))))
    torch.save(train_model.state_dict(), models_folder + "air-model-%d.pt" % step)
    if args.tf_checkpoints:
        train_model.save_tf_checkpoint(models_folder + "air-model-%d" % step)


if __name__ == "__main__":
    main()
