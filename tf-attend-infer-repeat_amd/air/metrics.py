"""Localisation metrics on the device: does the model ATTEND to the digits?

``Localization(model, max_gt_digits)`` scores the attention boxes of the model's last pass (``att``, ``run_digits``, where
the forward left them) against ground-truth boxes: ONE call of air_localization (include/air_hip.h has the semantics: box
IoU in fp64, a greedy match per image, fixed-order sums) per ``update()``, into int64 / fp64 accumulators that live on the
device, so the chunks of a data set add up.  ``values()`` derives the numbers of ``names()`` on the device without
blocking; ``result()`` is the one method that synchronises.

    loc = Localization(test_model, max_gt_digits=2)
    test_model.forward()
    loc.update(gt_count, gt_positions, gt_boxes)        # device int32 tensors, or numpy arrays (copied)
    loc.values()                                        # float64 [6] on the device, names() order
    loc.result()                                        # dict of floats + "confusion" [G + 1, T + 1] (truth x inferred)

The ground truth has the layouts of air_embed_collect and of air.sources.DeviceSceneSource: positions (x, y) and boxes
(w, h) as [k, G, 2] or [k, 2 G], so ``source.meta()`` can be passed straight in.  There is no CPU fallback.

``Segmentation(model, max_gt_digits)`` is the per-pixel instrument beside it: which object explains which ink?  One call of
air_segmentation per ``update()`` derives the predicted instance labels of the pass (``att`` and the decoded windows
``vrec``; the step whose compose term is the largest above ``pred_threshold``) and scores them against uint8 label planes:
the foreground adjusted Rand index and the best mask IoU of every ground-truth object, accumulated as above.

    seg = Segmentation(test_model, max_gt_digits=2)
    masks = Segmentation.scene_masks(source, digits)    # uint8 [B, C * C] from the glyph table of a DeviceSceneSource
    test_model.forward()
    seg.update(masks)
    seg.values()                                        # float64 [4] on the device: fg_ari, mask_iou, fg_missed, bg_claimed

``LatentProbe(model, max_gt_digits)`` asks the third question: do the what-codes say WHAT the digits are?  ``update()`` collects
the latent means of the digits the pass matched (one air_embed_collect call), ``score()`` is one air_latent_probe call over
them: exact leave-one-out k-nearest-neighbour digit accuracy with its confusion matrix, and the active units.

    probe = LatentProbe(test_model, max_gt_digits=2)
    test_model.forward()
    probe.update(gt_count, gt_positions, gt_boxes, gt_labels)
    probe.score()
    probe.values()                                      # float64 [4] on the device: knn_accuracy, active_units, scored, matched_share

``LatentClusters(model, max_gt_digits)`` asks the same store a question that needs no labelled neighbours: do digit classes
emerge in the what-codes ON THEIR OWN?  ``update()`` is LatentProbe's (the two share the store and the collector call),
``score()`` is one air_latent_kmeans call: exact k-means with seeded restarts, every cluster mapped to its majority class.

    clu = LatentClusters(test_model, max_gt_digits=2)
    test_model.forward()
    clu.update(gt_count, gt_positions, gt_boxes, gt_labels)
    clu.score()
    clu.values()                                        # float64 [6] on the device: accuracy, ari, nmi, inertia, live_clusters, scored

All of them are one protocol (_Instrument): ``evaluate(*truth)`` is reset() + update(*truth) (+ score() for the two above), the
model's last pass scored alone; ``prefix``, ``group``, ``reported`` and ``nan_in_events`` say how a driver names and writes
the values, so training.py carries a list of instruments without knowing which they are.

``ImportanceBound(model, samples=K)`` is the fourth, and the one that runs passes of its own: HOW LIKELY is the data, and how
sure is the model of the count?  ``evaluate(targets)`` runs K passes on fresh noise (AIRModel.forward_sampled), turns each
into a row of log-weights (air_importance_logw) and folds the rows (air_importance_fold) into the K-sample
importance-weighted bound, the effective sample size and the posterior over the object count.

    iw = ImportanceBound(test_model, samples=16)
    iw.evaluate(targets)                                # K x (forward_sampled, air_importance_logw), one fold
    iw.values()                                         # float64 [7] on the device: nll_bound, sample_loss, gap, ...

It leaves the buffers of its LAST SAMPLED pass in the model: instruments that score forward()'s pass go before it."""
import ctypes as C

import numpy as np
import torch

from . import _hip as H

NAMES = ("mean_iou", "recall", "precision", "cover", "center_dist", "count_accuracy")


class _Instrument:
    """What the three instruments share, and what a driver reads to carry one without knowing which it is (training.py):
    ``prefix`` of its keys in a row of scalars.jsonl, ``group`` of its TensorBoard tags, ``reported``: the names() that are
    written, ``nan_in_events``: whether a NaN value is written to the event file or left out.  evaluate(*truth) scores the
    model's last pass from zero: the arguments are update()'s."""
    NAMES = reported = ()
    prefix = group = None
    nan_in_events = True

    def __init__(self, model, max_gt_digits):
        self.op = type(self).__name__
        self.model, self.T, self.B, self.G = model, int(model.max_steps), int(model.batch_size), int(max_gt_digits)
        if self.G < 1:
            raise ValueError("%s: max_gt_digits must be positive" % self.op)

    def _refuse_beyond(self, a, b, most_a, most_b, what):
        if a > most_a or b > most_b:
            raise NotImplementedError("%s: %s: the kernel holds %d and %d" % (self.op, what, most_a, most_b))

    def _on_device(self, capture_too=False):
        """the device of the model's input buffer, once it is known to be one"""
        H.require_device(self.model.input_images, "the model's input buffer", self.op, capture_too=capture_too)
        dev = self.device = self.model.input_images.device
        self._nan = torch.full((len(self.NAMES),), float("nan"), dtype=torch.float64, device=dev)
        return dev

    def _accumulators(self, query, counts, sums):
        """the workspace `query` sizes for a whole batch, then ``counts`` int64 and ``sums`` float64 on the model's device"""
        nbytes = getattr(H.lib(), query)(self.T, self.B, self.B, self.G)
        if nbytes < 0:
            H.check(int(nbytes), query)
        dev = self._on_device()
        self.counts = torch.zeros(counts, dtype=torch.int64, device=dev)
        self.sums = torch.zeros(sums, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(int(nbytes) // 8, dtype=torch.float64, device=dev)
        return dev

    @classmethod
    def names(cls):
        return list(cls.NAMES)

    def reset(self):
        """zeroes the accumulators on the current stream"""
        self.counts.zero_()
        self.sums.zero_()

    def evaluate(self, *truth):
        """reset() and update(*truth): the model's last pass alone, on the current stream"""
        self.reset()
        self.update(*truth)

    def _images(self, k, first):
        """update()'s k: by default all rows of the first ground-truth array, and at most the model's batch"""
        if k is None:
            k = int(first.shape[0]) if hasattr(first, "shape") else len(first)
        k = int(k)
        if not 1 <= k <= self.B:
            raise ValueError("%s.update: k = %d images, the model's batch holds %d" % (self.op, k, self.B))
        return k

    def _truth(self, t, what, k, width):
        """`t` as a contiguous int32 device tensor of `width` values for each of at least k images (numpy is copied)"""
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype=np.int32)).to(self.device)
        H.require_device(t, what, self.op + ".update")
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device:
            raise ValueError("%s.update: %s must be a contiguous int32 tensor on %s" % (self.op, what, self.device))
        if t.dim() < 1 or int(t.shape[0]) < k or t.numel() != int(t.shape[0]) * width:
            raise ValueError("%s.update: %s must hold %d values for each of at least %d images, got %r"
                             % (self.op, what, width, k, tuple(t.shape)))
        return t

    def _ratios(self, num, den, out):
        """values()'s tail: num / den, NaN where den is 0, into `out` when there is one"""
        v = torch.where(den == 0, self._nan, num / den)
        if out is None:
            return v
        out.copy_(v)
        return out


class Localization(_Instrument):
    """mean_iou = IOU / PRESENT (an unmatched digit counts 0), recall = HITS / PRESENT, precision = HITS / INFERRED,
    cover = COVER / PRESENT, center_dist = DIST / MATCHED (transformer units), count_accuracy = COUNT_CORRECT / IMAGES; a
    zero denominator gives NaN.  per_digit=True also keeps ``match`` [B, G] int32 (the object matched to every digit, or
    -1) and ``iou`` [B, G] float64 of the last update (rows >= k are not written)."""
    NAMES = NAMES
    prefix, group = "loc_", "localization/"
    reported = NAMES[:5]                    # the sixth, count_accuracy, is the `accuracy` the model summarises itself

    def __init__(self, model, max_gt_digits, iou_threshold=0.5, per_digit=False):
        super().__init__(model, max_gt_digits)
        T, B, G = self.T, self.B, self.G
        self._refuse_beyond(T, G, H.LOC_MAX_STEPS, H.LOC_MAX_DIGITS, "%d steps, %d digits in one image" % (T, G))
        tau = self.iou_threshold = float(iou_threshold)
        if not 0.0 < tau <= 1.0:
            raise ValueError("Localization: iou_threshold must lie in (0, 1]")
        dev = self._accumulators("air_localization_workspace_bytes", H.LOC_COUNTS + (G + 1) * (T + 1), H.LOC_SUMS)
        self.match = torch.full((B, G), -1, dtype=torch.int32, device=dev) if per_digit else None
        self.iou = torch.zeros(B, G, dtype=torch.float64, device=dev) if per_digit else None

    def update(self, gt_count, gt_positions, gt_boxes, k=None):
        """One air_localization call over the model's last pass: its first k images (default: all rows of gt_count) against
        gt_count [>= k], gt_positions / gt_boxes [>= k, G, 2] or [>= k, 2 G]."""
        m = self.model
        m._ensure()
        H.require_device(m.att, "the model's records", "Localization.update")
        k = self._images(k, gt_count)
        gt = (self._truth(gt_count, "gt_count", k, 1), self._truth(gt_positions, "gt_positions", k, 2 * self.G),
              self._truth(gt_boxes, "gt_boxes", k, 2 * self.G))
        a = H.Localization(H.ptr(m.att), H.ptr(m.run_digits), *(H.ptr(t) for t in gt), H.ptr(self.match), H.ptr(self.iou),
                           H.ptr(self.counts), H.ptr(self.sums), self.T, self.B, k, self.G, m.canvas_size, self.iou_threshold)
        H.launch("air_localization", self.device, C.byref(a), H.ptr(self.workspace))

    def values(self, out=None):
        """float64 [len(names())] on the device, from the accumulators as they stand on the current stream; never blocks"""
        c, s = self.counts, self.sums
        num = torch.stack((s[H.LOC_IOU], c[H.LOC_HITS].double(), c[H.LOC_HITS].double(), s[H.LOC_COVER], s[H.LOC_DIST],
                           c[H.LOC_COUNT_CORRECT].double()))
        den = torch.stack((c[H.LOC_PRESENT], c[H.LOC_PRESENT], c[H.LOC_INFERRED], c[H.LOC_PRESENT], c[H.LOC_MATCHED],
                           c[H.LOC_IMAGES])).double()
        return self._ratios(num, den, out)

    def confusion(self):
        """int64 [G + 1, T + 1] view of the accumulators: rows the true count, columns the inferred one"""
        return self.counts[H.LOC_COUNTS:].view(self.G + 1, self.T + 1)

    def result(self):
        """the values as a dict of floats, the raw totals and the confusion matrix as numpy -- synchronises"""
        values, counts, sums = self.values().cpu().tolist(), self.counts.cpu().numpy(), self.sums.cpu().numpy()
        out = dict(zip(NAMES, values))
        out.update(images=int(counts[H.LOC_IMAGES]), present=int(counts[H.LOC_PRESENT]), inferred=int(counts[H.LOC_INFERRED]),
                   matched=int(counts[H.LOC_MATCHED]), hits=int(counts[H.LOC_HITS]),
                   confusion=counts[H.LOC_COUNTS:].reshape(self.G + 1, self.T + 1).copy(), sums=sums)
        return out


SEG_NAMES = ("fg_ari", "mask_iou", "fg_missed", "bg_claimed")


class Segmentation(_Instrument):
    """fg_ari = ARI / SCORED (images with at least two foreground pixels), mask_iou = MASK_IOU / PRESENT (the best IoU of a
    predicted mask with every ground-truth object), fg_missed = FG_MISSED / FG_PIXELS (ink no object claims), bg_claimed =
    BG_CLAIMED / (IMAGES * C * C - FG_PIXELS) (background an object claims); a zero denominator gives NaN.  keep=True also
    keeps ``pred_mask`` [B, C * C] uint8, ``tables`` [B, G + 1, T + 1] int32 (truth x prediction), ``ari`` [B] and
    ``mask_iou`` [B, G] float64 of the last update (rows >= k are not written)."""

    NAMES = reported = SEG_NAMES
    prefix, group = "seg_", "segmentation/"

    def __init__(self, model, max_gt_digits, pred_threshold=0.5, keep=False):
        super().__init__(model, max_gt_digits)
        T, B, G = self.T, self.B, self.G
        Cc, w = self.C, self.w = int(model.canvas_size), int(model.windows_size)
        self._refuse_beyond(T, G, H.SEG_MAX_STEPS, H.SEG_MAX_DIGITS, "%d steps, %d digits in one image" % (T, G))
        self._refuse_beyond(Cc, w, H.SEG_MAX_CANVAS, H.SEG_MAX_WINDOW, "a %d x %d canvas, %d x %d windows" % (Cc, Cc, w, w))
        thr = self.pred_threshold = float(pred_threshold)
        if not 0.0 <= thr < 1.0:
            raise ValueError("Segmentation: pred_threshold must lie in [0, 1)")
        dev = self._accumulators("air_segmentation_workspace_bytes", H.SEG_COUNTS, H.SEG_SUMS)
        self.pred_mask = torch.zeros(B, Cc * Cc, dtype=torch.uint8, device=dev) if keep else None
        self.tables = torch.zeros(B, G + 1, T + 1, dtype=torch.int32, device=dev) if keep else None
        self.ari = torch.full((B,), float("nan"), dtype=torch.float64, device=dev) if keep else None
        self.mask_iou = torch.zeros(B, G, dtype=torch.float64, device=dev) if keep else None

    def update(self, gt_mask, k=None):
        """One air_segmentation call over the model's last pass: its first k images (default: all rows of gt_mask) against
        gt_mask [>= k, C * C] or [>= k, C, C] uint8 (a device tensor, or a numpy array: copied), 0 the background."""
        m = self.model
        m._ensure()
        H.require_device(m.att, "the model's records", "Segmentation.update")
        H.require_device(m.vrec, "the model's decoded windows", "Segmentation.update")
        if not torch.is_tensor(gt_mask):
            gt_mask = torch.from_numpy(np.ascontiguousarray(np.asarray(gt_mask), dtype=np.uint8)).to(self.device)
        H.require_device(gt_mask, "gt_mask", "Segmentation.update")
        if gt_mask.dtype != torch.uint8 or not gt_mask.is_contiguous() or gt_mask.device != self.device:
            raise ValueError("Segmentation.update: gt_mask must be a contiguous uint8 tensor on %s" % self.device)
        k = self._images(k, gt_mask if gt_mask.dim() else ())        # (a scalar has no rows)
        if gt_mask.dim() < 2 or int(gt_mask.shape[0]) < k or gt_mask.numel() != int(gt_mask.shape[0]) * self.C * self.C:
            raise ValueError("Segmentation.update: gt_mask must hold %d labels for each of at least %d images, got %r"
                             % (self.C * self.C, k, tuple(gt_mask.shape)))
        a = H.Segmentation(H.ptr(m.att), H.ptr(m.vrec), H.ptr(gt_mask), H.ptr(self.pred_mask), H.ptr(self.tables),
                           H.ptr(self.ari), H.ptr(self.mask_iou), H.ptr(self.counts), H.ptr(self.sums),
                           self.T, self.B, k, self.G, self.C, self.w, self.pred_threshold)
        H.launch("air_segmentation", self.device, C.byref(a), H.ptr(self.workspace))

    def values(self, out=None):
        """float64 [len(names())] on the device, from the accumulators as they stand on the current stream; never blocks"""
        c, s = self.counts, self.sums
        num = torch.stack((s[H.SEG_ARI], s[H.SEG_MASK_IOU], c[H.SEG_FG_MISSED].double(), c[H.SEG_BG_CLAIMED].double()))
        den = torch.stack((c[H.SEG_SCORED], c[H.SEG_PRESENT], c[H.SEG_FG_PIXELS],
                           c[H.SEG_IMAGES] * (self.C * self.C) - c[H.SEG_FG_PIXELS])).double()
        return self._ratios(num, den, out)

    def result(self):
        """the values as a dict of floats and the raw totals -- synchronises"""
        values, counts, sums = self.values().cpu().tolist(), self.counts.cpu().numpy(), self.sums.cpu().numpy()
        out = dict(zip(SEG_NAMES, values))
        out.update(images=int(counts[H.SEG_IMAGES]), scored=int(counts[H.SEG_SCORED]), present=int(counts[H.SEG_PRESENT]),
                   fg_pixels=int(counts[H.SEG_FG_PIXELS]), fg_missed_pixels=int(counts[H.SEG_FG_MISSED]),
                   bg_claimed_pixels=int(counts[H.SEG_BG_CLAIMED]), sums=sums)
        return out

    @staticmethod
    def scene_masks(source_or_arrays, digits, ink_threshold=0.0):
        """uint8 [B, C * C] instance labels of composed scenes, one air_scene_masks launch on the current stream: pixel p of
        scene b is g + 1 for the first digit g < digits[b] whose glyph has ink (a value > ink_threshold) there, 0 elsewhere.
        source_or_arrays: an air.sources.DeviceSceneSource (its glyphs, crops and meta() of the last batch), or a dict of
        device tensors glyphs [Gn, gd * gd] float32, crops [Gn, 4], indices [B, max_digits], positions [B, 2 max_digits]
        int32 and the int canvas_dim.  digits: int32 [B] on the device."""
        src = source_or_arrays
        if isinstance(src, dict):
            glyphs, crops, indices, positions, Cc = (src[key] for key in ("glyphs", "crops", "indices", "positions", "canvas_dim"))
        else:
            meta = src.meta()
            glyphs, crops, indices, positions, Cc = src.glyphs, src.crops, meta["indices"], meta["positions"], src.canvas_dim
        for t, what, dtype in ((glyphs, "glyphs", torch.float32), (crops, "crops", torch.int32), (digits, "digits", torch.int32),
                               (indices, "indices", torch.int32), (positions, "positions", torch.int32)):
            H.require_device(t, what, "Segmentation.scene_masks")
            if t.dtype != dtype or not t.is_contiguous() or t.device != glyphs.device:
                raise ValueError("Segmentation.scene_masks: %s must be a contiguous %s tensor on %s" % (what, dtype, glyphs.device))
        if glyphs.dim() != 2 or crops.dim() != 2 or tuple(crops.shape) != (int(glyphs.shape[0]), 4):
            raise ValueError("Segmentation.scene_masks: glyphs must be [Gn, gd * gd] and crops [Gn, 4]")
        Gn, gd, Cc, B = int(glyphs.shape[0]), int(round(float(glyphs.shape[1]) ** 0.5)), int(Cc), int(digits.numel())
        if gd * gd != int(glyphs.shape[1]):
            raise ValueError("Segmentation.scene_masks: a glyph must be a square plane, got %d values" % int(glyphs.shape[1]))
        md = indices.numel() // B if B else 0
        if B < 1 or md < 1 or indices.numel() != B * md or positions.numel() != 2 * B * md:
            raise ValueError("Segmentation.scene_masks: indices [B, max_digits] and positions [B, 2 max_digits] must go with digits "
                             "[B], got %r, %r and %r" % (tuple(indices.shape), tuple(positions.shape), tuple(digits.shape)))
        mask = torch.empty(B, Cc * Cc, dtype=torch.uint8, device=glyphs.device)
        a = H.SceneMasks(H.ptr(glyphs), H.ptr(crops), H.ptr(digits), H.ptr(indices), H.ptr(positions), H.ptr(mask),
                         B, Gn, gd, Cc, md, float(ink_threshold))
        H.launch("air_scene_masks", glyphs.device, C.byref(a))
        return mask


PROBE_NAMES = ("knn_accuracy", "active_units", "scored", "matched_share")


class _ProbeBuffers:
    """the outputs and the workspace of air_latent_probe for up to M rows of Z dimensions, and the one call"""

    def __init__(self, op, dev, M, Z, k, classes, au_threshold, per_row):
        k, classes, au = int(k), int(classes), float(au_threshold)
        if k < 1 or classes < 1 or M < 1 or Z < 1:
            raise ValueError("%s: k, classes, the rows and their dimensions must be positive" % op)
        if not au >= 0.0:
            raise ValueError("%s: au_threshold must not be negative" % op)
        if k > H.PROBE_MAX_K or classes > H.PROBE_MAX_CLASSES or Z > H.PROBE_MAX_Z or M > H.PROBE_MAX_ROWS:
            raise NotImplementedError("%s: %d neighbours, %d classes, %d dimensions, %d rows: the kernel holds %d, %d, %d and %d"
                                      % (op, k, classes, Z, M, H.PROBE_MAX_K, H.PROBE_MAX_CLASSES, H.PROBE_MAX_Z, H.PROBE_MAX_ROWS))
        nbytes = H.lib().air_latent_probe_workspace_bytes(M, Z, k)
        if nbytes < 0:
            H.check(int(nbytes), "air_latent_probe_workspace_bytes")
        self.op, self.device, self.M, self.Z, self.k, self.classes, self.au_threshold = op, dev, M, Z, k, classes, au
        self.nbytes = int(nbytes)
        self.per_row = bool(per_row)

    def allocate(self):
        dev, M = self.device, self.M
        self.counts = torch.zeros(H.PROBE_COUNTS + self.classes * self.classes, dtype=torch.int64, device=dev)
        self.moments = torch.full((2 * self.Z,), float("nan"), dtype=torch.float64, device=dev)
        self.workspace = torch.empty(self.nbytes // 8, dtype=torch.float64, device=dev)
        self.pred = torch.full((M,), -1, dtype=torch.int32, device=dev) if self.per_row else None
        self.neighbours = torch.full((M, self.k), -1, dtype=torch.int32, device=dev) if self.per_row else None
        self.neighbour_d2 = torch.zeros(M, self.k, dtype=torch.float64, device=dev) if self.per_row else None
        return self

    def run(self, latents, labels, rows=None):
        """one air_latent_probe call on the current stream; rows: a device int32 tensor whose first element says how many
        rows are in use, or None for all M"""
        a = H.LatentProbe(H.ptr(latents), H.ptr(labels), H.ptr(rows), H.ptr(self.pred), H.ptr(self.neighbours),
                          H.ptr(self.neighbour_d2), H.ptr(self.counts), H.ptr(self.moments), self.M, self.Z, self.k, self.classes,
                          self.au_threshold)
        H.launch("air_latent_probe", self.device, C.byref(a), H.ptr(self.workspace))

    def summary(self):
        """the counts, the confusion matrix, the per-class recall and the moments as a dict of host values -- synchronises"""
        counts, moments, n = self.counts.cpu().numpy(), self.moments.cpu().numpy(), self.classes
        confusion = counts[H.PROBE_COUNTS:].reshape(n, n).copy()
        truth = confusion.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            recall = np.where(truth == 0, np.nan, np.diag(confusion) / truth.astype(np.float64))
        scored, correct = int(counts[H.PROBE_SCORED]), int(counts[H.PROBE_CORRECT])
        return dict(knn_accuracy=correct / scored if scored else float("nan"), active_units=int(counts[H.PROBE_ACTIVE_UNITS]),
                    scored=scored, correct=correct, rows=int(counts[H.PROBE_ROWS]), valid=int(counts[H.PROBE_VALID]),
                    k=self.k, classes=n, au_threshold=self.au_threshold, confusion=confusion, recall=recall,
                    mean=moments[:self.Z].copy(), variance=moments[self.Z:].copy())


class _LatentStore(_Instrument):
    """What the instruments over the what-codes share (LatentProbe, LatentClusters): the store ``latents`` [capacity, Z] /
    ``labels`` [capacity] of the matched digits' posterior means, with the collector's device counters as the cursor, and the
    one air_embed_collect call that appends a pass to it.  A subclass holds ``counts``, which reset() zeroes, and score()."""

    def _store_sizes(self, capacity, max_distance):
        """the sizes of the store, checked on the host: capacity defaults to batch_size * max_gt_digits (one pass)"""
        self.Z, self.w = int(self.model.vae_latent_dimensions), int(self.model.windows_size)
        capacity = self.B * self.G if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError("%s: capacity must be positive" % self.op)
        if not float(max_distance) > 0.0:
            raise ValueError("%s: max_distance must be positive" % self.op)
        self.capacity, self.max_distance = capacity, float(max_distance)
        return capacity

    def _store_allocate(self):
        """the collector's workspace query, then the store on the model's device (which is returned)"""
        T, B, G, Z, w, capacity = self.T, self.B, self.G, self.Z, self.w, self.capacity
        nints = H.lib().air_embed_collect_workspace_ints(T, B, B, G)
        if nints < 0:
            raise NotImplementedError("%s: %d steps, %d digits in one image: the collector holds %d and %d"
                                      % (self.op, T, G, H.EMBED_MAX_STEPS, H.EMBED_MAX_DIGITS))
        dev = self._on_device(capture_too=True)
        self.latents = torch.zeros(capacity, Z, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(capacity, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(H.EMBED_COUNTERS, dtype=torch.int32, device=dev)
        self._windows = torch.empty(capacity, w * w, dtype=torch.float32, device=dev)       # the collector writes them: unused
        self._ids = torch.empty(capacity, dtype=torch.int32, device=dev)
        self._match = torch.empty(B, G, dtype=torch.int32, device=dev)
        self._workspace = torch.empty(int(nints), dtype=torch.int32, device=dev)
        self._one = torch.ones(1, dtype=torch.float64, device=dev)
        return dev

    def reset(self):
        """zeroes the row cursor and the counts on the current stream"""
        self.counters.zero_()
        self.counts.zero_()

    def evaluate(self, *truth):
        """reset(), update(*truth) and score()"""
        super().evaluate(*truth)
        self.score()

    def update(self, gt_count, gt_positions, gt_boxes, gt_labels, k=None):
        """One air_embed_collect call over the model's last pass: the digits of its first k images (default: all rows of
        gt_count) matched to the inferred objects by centre distance, the latent means of the matched ones appended to the
        store with gt_labels [>= k, G] as their labels.  gt_positions / gt_boxes: [>= k, G, 2] or [>= k, 2 G]."""
        m = self.model
        m._ensure()
        H.require_device(m.att, "the model's records", self.op + ".update", capture_too=True)
        k = self._images(k, gt_count)
        gt = (self._truth(gt_count, "gt_count", k, 1), self._truth(gt_positions, "gt_positions", k, 2 * self.G),
              self._truth(gt_boxes, "gt_boxes", k, 2 * self.G), self._truth(gt_labels, "gt_labels", k, self.G))
        a = H.EmbedCollect(H.ptr(m.att), H.ptr(m.run_digits), H.ptr(m.ml), H.ptr(m.vrec), *(H.ptr(t) for t in gt), H.ptr(gt[3]),
                           H.ptr(self._match), H.ptr(self.counters), H.ptr(self.latents), H.ptr(self._windows),
                           H.ptr(self.labels), H.ptr(self._ids), self.T, self.B, k, self.G, self.Z, self.w, self.capacity,
                           m.canvas_size, self.max_distance)
        H.launch("air_embed_collect", self.device, C.byref(a), H.ptr(self._workspace))

    def _collected(self):
        """the collector's totals as a dict of host values -- synchronises"""
        counters = self.counters.cpu().tolist()
        return dict(matched=counters[H.EMBED_MATCHED], present=counters[H.EMBED_PRESENT], inferred=counters[H.EMBED_INFERRED],
                    overflow=bool(counters[H.EMBED_OVERFLOW]), capacity=self.capacity)


class LatentProbe(_LatentStore):
    """Do the what-codes say WHAT the digits are?  The latent codes (posterior means) of the matched digits of an evaluation
    set, scored by air_latent_probe (include/air_hip.h has the semantics): the leave-one-out k-nearest-neighbour accuracy of
    their labels with its confusion matrix, and the active units (dimensions whose mean varies over the set, variance >
    au_threshold).  fp64 in a fixed order; nothing blocks but result().

        probe = LatentProbe(test_model, max_gt_digits=2)
        test_model.forward()
        probe.update(gt_count, gt_positions, gt_boxes, gt_labels)   # one air_embed_collect call: the projector export's match
        probe.score()                                               # one air_latent_probe call over the rows collected so far
        probe.values()                                              # float64 [4] on the device, names() order

    knn_accuracy = CORRECT / SCORED, active_units and scored as counted, matched_share = MATCHED / PRESENT (the share of the
    ground-truth digits that were matched to an inferred object, and so probed); a zero denominator gives NaN.  The rows
    live in the probe's own store ``latents`` [capacity, Z] / ``labels`` [capacity] with the collector's device counters as
    the cursor; capacity defaults to batch_size * max_gt_digits (one pass), and digits beyond it set the overflow flag that
    result() reports.  per_row=True keeps ``pred`` [capacity], ``neighbours`` and ``neighbour_d2`` [capacity, k] of the last
    score()."""
    NAMES = reported = PROBE_NAMES
    prefix, group = "lat_", "latents/"
    nan_in_events = False                     # (nothing scored yet: the scalar is left out, not written as NaN)

    def __init__(self, model, max_gt_digits, classes=10, k=5, capacity=None, au_threshold=0.01, per_row=False, max_distance=0.2):
        super().__init__(model, max_gt_digits)
        capacity = self._store_sizes(capacity, max_distance)
        self.buffers = _ProbeBuffers("LatentProbe", None, capacity, self.Z, k, classes, au_threshold, per_row)
        self.buffers.device = self._store_allocate()
        self.k, self.classes = self.buffers.k, self.buffers.classes
        self.buffers.allocate()
        self.counts, self.moments = self.buffers.counts, self.buffers.moments
        self.pred, self.neighbours, self.neighbour_d2 = self.buffers.pred, self.buffers.neighbours, self.buffers.neighbour_d2

    def score(self):
        """One air_latent_probe call over the rows collected so far (the device cursor says how many: no host read)"""
        H.require_device(self.latents, "the store", "LatentProbe.score", capture_too=True)
        self.buffers.run(self.latents, self.labels, self.counters[H.EMBED_MATCHED:])

    def values(self, out=None):
        """float64 [len(names())] on the device, from the counts of the last score() and the collector's counters as they
        stand on the current stream; never blocks"""
        c, n = self.counts.double(), self.counters.double()
        num = torch.stack((c[H.PROBE_CORRECT], c[H.PROBE_ACTIVE_UNITS], c[H.PROBE_SCORED], n[H.EMBED_MATCHED]))
        den = torch.stack((c[H.PROBE_SCORED], self._one[0], self._one[0], n[H.EMBED_PRESENT]))
        return self._ratios(num, den, out)

    def confusion(self):
        """int64 [classes, classes] view of the counts: rows the true class, columns the predicted one"""
        return self.counts[H.PROBE_COUNTS:].view(self.classes, self.classes)

    def result(self):
        """the values as a dict of floats, the totals, the confusion matrix, the per-class recall and the moments as numpy
        -- synchronises"""
        values = self.values().cpu().tolist()
        out = self.buffers.summary()
        out.update(zip(PROBE_NAMES, values))
        out.update(self._collected())
        return out


CLUSTER_NAMES = ("accuracy", "ari", "nmi", "inertia", "live_clusters", "scored")


class _KMeansBuffers:
    """the outputs and the workspace of air_latent_kmeans for up to M rows of Z dimensions, the one call, and the numbers
    derived from its counts"""

    def __init__(self, op, dev, M, Z, k, classes, restarts, max_iters, seed, per_row):
        k, classes, R, iters = int(k), int(classes), int(restarts), int(max_iters)
        if k < 1 or classes < 1 or R < 1 or iters < 1 or M < 1 or Z < 1:
            raise ValueError("%s: clusters, classes, restarts, max_iters, the rows and their dimensions must be positive" % op)
        if k > H.KMEANS_MAX_K or classes > H.PROBE_MAX_CLASSES or R > H.KMEANS_MAX_RESTARTS or iters > H.KMEANS_MAX_ITERS \
                or Z > H.PROBE_MAX_Z or M > H.PROBE_MAX_ROWS:
            raise NotImplementedError(
                "%s: %d clusters, %d classes, %d restarts, %d iterations, %d dimensions, %d rows: the kernel holds %d, %d, %d, %d, "
                "%d and %d" % (op, k, classes, R, iters, Z, M, H.KMEANS_MAX_K, H.PROBE_MAX_CLASSES, H.KMEANS_MAX_RESTARTS,
                               H.KMEANS_MAX_ITERS, H.PROBE_MAX_Z, H.PROBE_MAX_ROWS))
        nbytes = H.lib().air_latent_kmeans_workspace_bytes(M, Z, k, R)
        if nbytes < 0:
            H.check(int(nbytes), "air_latent_kmeans_workspace_bytes")
        self.op, self.device, self.M, self.Z, self.k, self.classes, self.restarts, self.max_iters = op, dev, M, Z, k, classes, R, iters
        self.seed, self.nbytes, self.per_row = int(seed) & 0xFFFFFFFFFFFFFFFF, int(nbytes), bool(per_row)

    def allocate(self):
        dev, M, k = self.device, self.M, self.k
        self.counts = torch.zeros(H.KMEANS_COUNTS + 2 * k + k * self.classes, dtype=torch.int64, device=dev)
        self.assignment = torch.full((M,), -1, dtype=torch.int32, device=dev)
        self.row_d2 = torch.zeros(M, dtype=torch.float64, device=dev) if self.per_row else None
        self.centroids = torch.full((k, self.Z), float("nan"), dtype=torch.float64, device=dev)
        self.restart_inertia = torch.full((self.restarts,), float("nan"), dtype=torch.float64, device=dev)
        self.restart_iters = torch.zeros(self.restarts, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(self.nbytes // 8, dtype=torch.float64, device=dev)
        self._nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        self._zero = torch.zeros((), dtype=torch.float64, device=dev)
        return self

    def run(self, latents, labels=None, rows=None):
        """one air_latent_kmeans call on the current stream; labels: None clusters without scoring; rows: a device int32
        tensor whose first element says how many rows are in use, or None for all M"""
        a = H.LatentKmeans(H.ptr(latents), H.ptr(labels), H.ptr(rows), H.ptr(self.assignment), H.ptr(self.row_d2),
                           H.ptr(self.centroids), H.ptr(self.restart_inertia), H.ptr(self.restart_iters), H.ptr(self.counts),
                           self.M, self.Z, self.k, self.classes, self.restarts, self.max_iters, self.seed)
        H.launch("air_latent_kmeans", self.device, C.byref(a), H.ptr(self.workspace))

    def table(self):
        """int64 [k, classes] view of the counts: rows the cluster, columns the class"""
        return self.counts[H.KMEANS_COUNTS + 2 * self.k:].view(self.k, self.classes)

    def values(self):
        """float64 [6] on the device in CLUSTER_NAMES order, fp64 torch ops over the integer counts; never blocks"""
        c, nan = self.counts, self._nan
        t = self.table().double()
        n = t.sum()
        pairs = lambda v: (v * (v - 1.0) / 2.0).sum()            # noqa: E731  (integers below 2^53: exact)
        rows_, cols = t.sum(dim=1), t.sum(dim=0)
        I, A, B, N = pairs(t), pairs(rows_), pairs(cols), n * (n - 1.0) / 2.0
        E = torch.where(N == 0, nan, A * B / N)
        den = (A + B) / 2.0 - E
        ari = torch.where(den == 0, nan, (I - E) / den)
        plogp = lambda v: torch.where(v > 0, (v / n) * torch.log(v / n), self._zero).sum()      # noqa: E731
        hc, hl, hcl = -plogp(rows_), -plogp(cols), -plogp(t.reshape(-1))
        nmi = torch.where((hc + hl == 0) | (n == 0), nan, 2.0 * (hc + hl - hcl) / (hc + hl))
        ari = torch.where(n == 0, nan, ari)
        labelled, valid = c[H.KMEANS_LABELLED].double(), c[H.KMEANS_VALID].double()
        inertia = self.restart_inertia.index_select(0, c[H.KMEANS_BEST:H.KMEANS_BEST + 1])[0]
        num = torch.stack((c[H.KMEANS_CORRECT].double(), ari, nmi, inertia, c[H.KMEANS_LIVE].double(), labelled))
        one = torch.ones_like(valid)
        den = torch.stack((labelled, one, one, valid, one, one))
        return torch.where(den == 0, nan, num / den)

    def summary(self):
        """the values, the counts, the table, sizes, majority, centroids and every restart's inertia and iterations as a dict
        of host values -- synchronises"""
        values, counts, k, n = self.values().cpu().tolist(), self.counts.cpu().numpy(), self.k, self.classes
        at = H.KMEANS_COUNTS
        table = counts[at + 2 * k:].reshape(k, n).copy()
        out = dict(zip(CLUSTER_NAMES, values))
        out.update(rows=int(counts[H.KMEANS_ROWS]), valid=int(counts[H.KMEANS_VALID]), labelled=int(counts[H.KMEANS_LABELLED]),
                   correct=int(counts[H.KMEANS_CORRECT]), live=int(counts[H.KMEANS_LIVE]), best=int(counts[H.KMEANS_BEST]),
                   iters=int(counts[H.KMEANS_ITERS]), converged=bool(counts[H.KMEANS_CONVERGED]),
                   restarts_converged=int(counts[H.KMEANS_RESTARTS_CONVERGED]), clusters=k, classes=n, restarts=self.restarts,
                   max_iters=self.max_iters, seed=self.seed, table=table, confusion=table,
                   sizes=counts[at:at + k].copy(), majority=counts[at + k:at + 2 * k].copy(),
                   centroids=self.centroids.cpu().numpy(), assignment=self.assignment.cpu().numpy(),
                   restart_inertia=self.restart_inertia.cpu().numpy(), restart_iters=self.restart_iters.cpu().numpy())
        return out


class LatentClusters(_LatentStore):
    """Do digit classes emerge in the what-codes ON THEIR OWN?  The store of LatentProbe (the posterior means of the matched
    digits), clustered without their labels by air_latent_kmeans (include/air_hip.h has the semantics: exact k-means, fp64 in
    a fixed order, `restarts` seeded starts, the lowest inertia wins), then every cluster mapped to its majority class.

        clu = LatentClusters(test_model, max_gt_digits=2)
        test_model.forward()
        clu.update(gt_count, gt_positions, gt_boxes, gt_labels)     # LatentProbe's: one air_embed_collect call
        clu.score()                                                 # one air_latent_kmeans call over the rows collected so far
        clu.values()                                                # float64 [6] on the device, names() order

    accuracy = CORRECT / LABELLED (clustering accuracy, or purity: the rows that carry their cluster's majority class),
    ari = the adjusted Rand index of the cluster x class table, (I - E) / ((A + B) / 2 - E) over its pair counts,
    nmi = 2 I(c; l) / (H(c) + H(l)), inertia = the best restart's, per valid row, live_clusters and scored (the labelled
    rows) as counted; a zero denominator gives NaN.  Derived on the device in fp64 from the integer counts; nothing blocks but
    result().  ``centroids`` [clusters, Z] float64 are what-codes: AIRModel.decode draws what each cluster looks like.
    per_row=True keeps ``row_d2`` [capacity] of the last score() beside ``assignment`` [capacity]."""
    NAMES = reported = CLUSTER_NAMES
    prefix, group = "clu_", "clusters/"
    nan_in_events = False

    def __init__(self, model, max_gt_digits, classes=10, clusters=None, restarts=8, max_iters=50, seed=0, capacity=None,
                 max_distance=0.2, per_row=False):
        super().__init__(model, max_gt_digits)
        capacity = self._store_sizes(capacity, max_distance)
        self.buffers = _KMeansBuffers("LatentClusters", None, capacity, self.Z, classes if clusters is None else clusters, classes,
                                      restarts, max_iters, seed, per_row)
        self.buffers.device = self._store_allocate()
        b = self.buffers.allocate()
        self.clusters, self.classes, self.restarts, self.max_iters, self.seed = b.k, b.classes, b.restarts, b.max_iters, b.seed
        self.counts, self.assignment, self.row_d2, self.centroids = b.counts, b.assignment, b.row_d2, b.centroids
        self.restart_inertia, self.restart_iters = b.restart_inertia, b.restart_iters

    def score(self):
        """One air_latent_kmeans call over the rows collected so far (the device cursor says how many: no host read)"""
        H.require_device(self.latents, "the store", "LatentClusters.score", capture_too=True)
        self.buffers.run(self.latents, self.labels, self.counters[H.EMBED_MATCHED:])

    def values(self, out=None):
        """float64 [len(names())] on the device, from the counts of the last score() as they stand on the current stream;
        never blocks"""
        v = self.buffers.values()
        if out is None:
            return v
        out.copy_(v)
        return out

    def table(self):
        """int64 [clusters, classes] view of the counts: rows the cluster, columns the true class"""
        return self.buffers.table()

    def result(self):
        """the values as a dict of floats, the totals, the cluster x class table (also under "confusion"), sizes, majority,
        centroids, every restart's inertia and iterations and the converged flags as numpy -- synchronises"""
        out = self.buffers.summary()
        out.update(self._collected())
        return out


IW_NAMES = ("nll_bound", "sample_loss", "gap", "ess_share", "count_accuracy", "count_entropy", "count_split")
_IW_SALT = 0x4957                                  # the instrument's noise is not the generator's at the same call number


class ImportanceBound(_Instrument):
    """How likely is the data, and how sure is the model of the count?  K passes on fresh noise, each turned into a row of
    log-weights log p(x, z) - log q(z | x) by air_importance_logw, and the rows folded by air_importance_fold
    (include/air_hip.h has the semantics of both) into fp64 accumulators on the device, so the chunks of a test set add up.

        iw = ImportanceBound(test_model, samples=16)
        iw.evaluate(targets)                  # reset(), K x add_sample(), fold(targets)
        iw.values()                           # float64 [7] on the device, names() order; never blocks
        iw.result()                           # dict of floats + "confusion" [T + 1, T + 1] (true count x MAP count)

    nll_bound = -BOUND / SCORED (the K-sample importance-weighted bound on -log p(x): it tightens with K), sample_loss =
    -ELBO / SCORED (the mean one-sample bound of the same K passes), gap = sample_loss - nll_bound (>= 0), ess_share = ESS /
    (K SCORED) (1: the weights are equal; 1 / K: one sample carries the image), count_accuracy = MAP_CORRECT / SCORED (the
    count with the largest posterior weight against `targets`; NaN without), count_entropy = ENTROPY / SCORED (nats, of the
    count posterior), count_split = SPLIT / SCORED (images whose K passes did not agree on the count); a zero denominator
    gives NaN.  An image without a finite weight is counted as degenerate and left out of SCORED.

    The noise of pass n is air_philox_fill's under (seed, n): ``calls`` runs on across evaluations, so successive
    evaluations see different noise, and the same (seed, calls) reproduces every bit.  The model keeps the buffers of the
    last sampled pass; forward() afterwards gives what it gave before.  keep=True also keeps ``terms`` [K, B, 5] float64
    (rec, z_pres, scale, shift, what of every weight) and ``bound``, ``ess`` [B] float64, ``map`` [B] int32 of the last
    fold (rows >= k are not written)."""
    NAMES = reported = IW_NAMES
    prefix, group = "iw_", "importance/"

    def __init__(self, model, samples=16, seed=0, keep=False):
        self.op = "ImportanceBound"
        self.model, self.T, self.B = model, int(model.max_steps), int(model.batch_size)
        K = self.K = self.G = int(samples)            # (G: where _accumulators passes the fourth size of the workspace query)
        T, B, Z = self.T, self.B, int(model.vae_latent_dimensions)
        if K < 1:
            raise ValueError("ImportanceBound: samples must be positive")
        if T > H.MAX_STEPS or K > H.IW_MAX_SAMPLES or Z > H.IW_MAX_Z:
            raise NotImplementedError("ImportanceBound: %d steps, %d samples, %d latent dimensions: the kernels hold %d, %d and %d"
                                      % (T, K, Z, H.MAX_STEPS, H.IW_MAX_SAMPLES, H.IW_MAX_Z))
        self.Z, self.seed, self.calls, self._sample, self._targets = Z, int(seed), 0, 0, False
        dev = self._accumulators("air_importance_fold_workspace_bytes", H.IW_COUNTS + (T + 1) * (T + 1), H.IW_SUMS)
        self.logw = torch.full((K, B), float("nan"), dtype=torch.float64, device=dev)
        self.digits = torch.zeros(K, B, dtype=torch.int32, device=dev)
        self.terms = torch.full((K, B, H.IW_TERMS), float("nan"), dtype=torch.float64, device=dev) if keep else None
        self.bound = torch.full((B,), float("nan"), dtype=torch.float64, device=dev) if keep else None
        self.ess = torch.full((B,), float("nan"), dtype=torch.float64, device=dev) if keep else None
        self.map = torch.full((B,), -1, dtype=torch.int32, device=dev) if keep else None

    def reset(self):
        """zeroes the accumulators on the current stream and forgets the passes sampled so far (not the call counter)"""
        super().reset()
        self._sample = 0

    def add_sample(self, k=None):
        """One pass of the model on fresh noise and one air_importance_logw call: the next row of the tables, for the first k
        images (default: the whole batch).  K of them, then fold()."""
        if self._sample >= self.K:
            raise RuntimeError("ImportanceBound.add_sample: all %d samples are drawn -- fold() them first" % self.K)
        k = self._images(self.B if k is None else k, None)
        m = self.model
        m.forward_sampled(self.calls, (self.seed ^ _IW_SALT) & 0xFFFFFFFFFFFFFFFF)
        self.calls += 1
        a = H.Importance(H.ptr(m.att), H.ptr(m.out7), H.ptr(m.ml), H.ptr(m.zs), H.ptr(m.eps_scale), H.ptr(m.eps_shift),
                         H.ptr(m.eps_z), H.ptr(m._rec_loss), H.ptr(m.run_digits), H.ptr(m.dyn), H.ptr(self.logw),
                         H.ptr(self.digits), H.ptr(self.terms), self.T, self.B, k, self.Z, int(m.zs.stride(1)), self.K)
        H.launch("air_importance_logw", self.device, C.byref(a), self._sample)
        self._sample += 1

    def fold(self, targets=None, k=None):
        """One air_importance_fold call over the K rows drawn since the last fold, added to the accumulators.  targets: the
        true counts of at least k images (a device int32 tensor, or a numpy array: copied), or None."""
        if self._sample != self.K:
            raise RuntimeError("ImportanceBound.fold: %d of %d samples are drawn" % (self._sample, self.K))
        k = self._images(self.B if k is None else k, None)
        if targets is not None:
            targets = self._truth(targets, "targets", k, 1)
        self._targets = targets is not None
        a = H.ImportanceFold(H.ptr(self.logw), H.ptr(self.digits), H.ptr(targets), H.ptr(self.bound), H.ptr(self.ess),
                             H.ptr(self.map), H.ptr(self.counts), H.ptr(self.sums), self.T, self.B, k, self.K)
        H.launch("air_importance_fold", self.device, C.byref(a), H.ptr(self.workspace))
        self._sample = 0

    def evaluate(self, targets=None, k=None):
        """reset(), K x add_sample() and fold(targets): the model's current batch scored from zero, on the current stream"""
        self.reset()
        for _ in range(self.K):
            self.add_sample(k)
        self.fold(targets, k)

    def values(self, out=None):
        """float64 [len(names())] on the device, from the accumulators as they stand on the current stream; never blocks"""
        c, s = self.counts, self.sums
        scored = c[H.IW_SCORED].double()
        correct = c[H.IW_MAP_CORRECT].double() if self._targets else self._nan[0]
        num = torch.stack((-s[H.IW_BOUND], -s[H.IW_ELBO], s[H.IW_BOUND] - s[H.IW_ELBO], s[H.IW_ESS], correct, s[H.IW_ENTROPY],
                           c[H.IW_SPLIT].double()))
        den = torch.stack((scored, scored, scored, scored * self.K, scored, scored, scored))
        return self._ratios(num, den, out)

    def confusion(self):
        """int64 [T + 1, T + 1] view of the accumulators: rows the true count, columns the MAP count"""
        return self.counts[H.IW_COUNTS:].view(self.T + 1, self.T + 1)

    def result(self):
        """the values as a dict of floats, the raw totals and the confusion matrix as numpy -- synchronises"""
        values, counts, sums = self.values().cpu().tolist(), self.counts.cpu().numpy(), self.sums.cpu().numpy()
        out = dict(zip(IW_NAMES, values))
        out.update(images=int(counts[H.IW_IMAGES]), scored=int(counts[H.IW_SCORED]), degenerate=int(counts[H.IW_DEGENERATE]),
                   samples=self.K, calls=self.calls,
                   confusion=counts[H.IW_COUNTS:].reshape(self.T + 1, self.T + 1).copy(), sums=sums)
        return out
