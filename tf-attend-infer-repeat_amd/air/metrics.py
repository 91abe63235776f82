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

The ground truth has the layouts of air_embed_collect and of multi_mnist.DeviceSceneSource: positions (x, y) and boxes
(w, h) as [k, G, 2] or [k, 2 G], so ``source.meta()`` can be passed straight in.  There is no CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _hip as H

NAMES = ("mean_iou", "recall", "precision", "cover", "center_dist", "count_accuracy")


class Localization:
    """mean_iou = IOU / PRESENT (an unmatched digit counts 0), recall = HITS / PRESENT, precision = HITS / INFERRED,
    cover = COVER / PRESENT, center_dist = DIST / MATCHED (transformer units), count_accuracy = COUNT_CORRECT / IMAGES; a
    zero denominator gives NaN.  per_digit=True also keeps ``match`` [B, G] int32 (the object matched to every digit, or
    -1) and ``iou`` [B, G] float64 of the last update (rows >= k are not written)."""

    def __init__(self, model, max_gt_digits, iou_threshold=0.5, per_digit=False):
        T, B, G = int(model.max_steps), int(model.batch_size), int(max_gt_digits)
        if G < 1:
            raise ValueError("Localization: max_gt_digits must be positive")
        if T > H.LOC_MAX_STEPS or G > H.LOC_MAX_DIGITS:
            raise NotImplementedError("Localization: %d steps, %d digits in one image: the kernel holds %d and %d"
                                      % (T, G, H.LOC_MAX_STEPS, H.LOC_MAX_DIGITS))
        tau = float(iou_threshold)
        if not 0.0 < tau <= 1.0:
            raise ValueError("Localization: iou_threshold must lie in (0, 1]")
        nbytes = H.lib().air_localization_workspace_bytes(T, B, B, G)
        if nbytes < 0:
            H.check(int(nbytes), "air_localization_workspace_bytes")
        H.require_device(model.input_images, "the model's input buffer", "Localization")
        dev = self.device = model.input_images.device
        self.model, self.T, self.B, self.G, self.iou_threshold = model, T, B, G, tau
        self.counts = torch.zeros(H.LOC_COUNTS + (G + 1) * (T + 1), dtype=torch.int64, device=dev)
        self.sums = torch.zeros(H.LOC_SUMS, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(int(nbytes) // 8, dtype=torch.float64, device=dev)
        self.match = torch.full((B, G), -1, dtype=torch.int32, device=dev) if per_digit else None
        self.iou = torch.zeros(B, G, dtype=torch.float64, device=dev) if per_digit else None
        self._nan = torch.full((len(NAMES),), float("nan"), dtype=torch.float64, device=dev)

    @staticmethod
    def names():
        return list(NAMES)

    def reset(self):
        """zeroes the accumulators on the current stream"""
        self.counts.zero_()
        self.sums.zero_()

    def _truth(self, t, what, k, width):
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype=np.int32)).to(self.device)
        H.require_device(t, what, "Localization.update")
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device:
            raise ValueError("Localization.update: %s must be a contiguous int32 tensor on %s" % (what, self.device))
        if t.dim() < 1 or int(t.shape[0]) < k or t.numel() != int(t.shape[0]) * width:
            raise ValueError("Localization.update: %s must hold %d values for each of at least %d images, got %r"
                             % (what, width, k, tuple(t.shape)))
        return t

    def update(self, gt_count, gt_positions, gt_boxes, k=None):
        """One air_localization call over the model's last pass: its first k images (default: all rows of gt_count) against
        gt_count [>= k], gt_positions / gt_boxes [>= k, G, 2] or [>= k, 2 G]."""
        m = self.model
        m._ensure()
        H.require_device(m.att, "the model's records", "Localization.update")
        if k is None:
            k = int(gt_count.shape[0]) if hasattr(gt_count, "shape") else len(gt_count)
        k = int(k)
        if not 1 <= k <= self.B:
            raise ValueError("Localization.update: k = %d images, the model's batch holds %d" % (k, self.B))
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
        v = torch.where(den == 0, self._nan, num / den)
        if out is None:
            return v
        out.copy_(v)
        return out

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
