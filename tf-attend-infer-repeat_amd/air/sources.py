"""The device data sources.  Feeds put batches into the train model's input buffers without the host: ShuffleBatchQueue (the
reference's input queue over a resident train set) and DeviceSceneSource (scenes composed from glyphs) are one protocol, _Feed.
Banks are glyph tables remade on the device that a scene source draws from: DeviceGlyphBank (scale and rotation jitter) and
DeviceHandwritingBank (MNIST's geometry) share _Bank; a plain glyph array is the bank that never turns over (_FixedBank).
multi_mnist.py re-exports the public names.  Importing this module loads neither torch nor the library: a constructor binds
them (_Device._bind), so the host generator stays importable without either.  There is no CPU fallback anywhere here."""
import numpy as np

JITTER_NEUTRAL = dict(min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0)

# The handwriting bank's starting values (a CPU prototype of the recipe read as MNIST at a glance with them): 40-pixel base
# planes, a 20-pixel box in a 28-pixel frame, an elastic field of sigma 6 / alpha 1.5 base pixels (Simard's 4 / 34 at 28
# pixels is a far stronger field; this one is judged at 40 and halved by the fit), +-12 degrees, shear +-0.2, scale
# 0.85 .. 1.15 per axis, one pass of erosion or dilation at the most, and an ink ramp that saturates the strokes.
MNIST_LIKE = dict(side=40, ink=20, od=28, sigma=6.0, alpha=1.5, max_ang=12.0, max_shear=0.2, min_scale=0.85, max_scale=1.15,
                  min_stroke=-1, max_stroke=1, lo=0.3, hi=0.7)


def crop_boxes(glyphs, image_dim):
    """[G, 4] int32 (x0, y0, w, h): the box crop_non_empty keeps of every glyph of [G, image_dim * image_dim]"""
    g = np.asarray(glyphs, np.float32).reshape(len(glyphs), image_dim, image_dim)
    out = np.zeros((len(g), 4), np.int32)
    for i, im in enumerate(g):
        cols = np.nonzero(np.sum(im, axis=0))[0]
        rows = np.nonzero(np.sum(im, axis=1))[0]
        if len(cols) == 0:
            raise ValueError("glyph %d is empty: crop_non_empty has no box for it" % i)
        out[i] = (cols[0], rows[0], cols[-1] - cols[0] + 1, rows[-1] - rows[0] + 1)
    return out


def gaussian_taps(sigma, radius=None):
    """-> (taps [2 R + 1] float64, a normalised Gaussian; R = int(4 sigma + 0.5) unless given)"""
    R = int(4.0 * float(sigma) + 0.5) if radius is None else int(radius)
    x = np.arange(-R, R + 1, dtype=np.float64)
    t = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return t / t.sum(), R


def _glyph_array(glyphs):
    """-> ([G, gd * gd] float32 contiguous numpy, gd)"""
    import torch
    g = glyphs.detach().cpu().numpy() if torch.is_tensor(glyphs) else np.asarray(glyphs)
    g = np.ascontiguousarray(g.reshape(len(g), -1), np.float32)
    gd = int(round(np.sqrt(g.shape[1])))
    if gd * gd != g.shape[1]:
        raise ValueError("glyphs must be [G, gd * gd]")
    if g.min() < 0:
        raise ValueError("glyph values must be >= 0")
    return g, gd


class _Device:
    """what every class here starts with: torch and the library, bound by the constructor, not by importing the module"""

    def _bind(self):
        import ctypes as C
        import torch
        from air import _hip as H
        self._C, self._torch, self._H = C, torch, H
        return C, torch, H

    def _s(self):
        return self._H.stream(self.device)


# ----------------------------------------------------------------------------- the banks
class _Bank(_Device):
    """A glyph table remade on the device by ONE launch per refresh.  A bank declares `struct` (its descriptor in air._hip),
    `entry` and `prepare` (its launch and the host-only checks of it), `params_width`, `extra` (the name of its second input
    tensor) and fits(); its constructor checks its own arguments, then _make() gets that input and the scalar fields."""

    def _make(self, g, gd, variants, od, seed, device, extra, scalars):
        """the descriptor by field name, checked on placeholder pointers; the device; the tensors; the checks again"""
        torch, H = self._torch, self._H
        V, name = int(variants), type(self).__name__
        self.variants, self.gd, self.od = V, gd, int(od)
        self._a = getattr(H, self.struct)(V=V, G=len(g), gd=gd, od=self.od, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, **scalars)
        required = ("glyphs", self.extra, "bank", "bank_crops", "source", "params", "status")       # counter may be null
        # the argument checks first, before anything is allocated: they need no device (the pointers are placeholders that
        # the checks only compare with null and test for alignment)
        for k in required:
            setattr(self._a, k, 16)
        self._checks()
        if device is None and not torch.cuda.is_available():
            raise H.AirHipError("%s: needs a GPU (no CPU fallback)" % name)
        dev = self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise H.AirHipError("%s: device must be a GPU (no CPU fallback)" % name)
        self.glyphs = torch.tensor(g, device=dev)
        setattr(self, self.extra, torch.tensor(extra, device=dev))
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)           # the bank generation (device: replays move it)
        self.bank = torch.zeros(V, self.od * self.od, device=dev)
        self.bank_crops = torch.zeros(V, 4, dtype=torch.int32, device=dev)
        self.source = torch.zeros(V, dtype=torch.int32, device=dev)
        self.params = torch.zeros(V, self.params_width, dtype=torch.float64, device=dev)
        self.status = torch.ones(V, dtype=torch.int32, device=dev)             # (nothing is usable before the first refresh)
        for k in required + ("counter",):
            setattr(self._a, k, getattr(self, k).data_ptr())
        with torch.cuda.device(dev):
            self._checks()

    def _checks(self):
        H = self._H
        H.check(getattr(H.lib(), self.prepare)(self._C.byref(self._a)), self.prepare)

    def refresh(self):
        H = self._H
        s = self._s()
        H.check(getattr(H.lib(), self.entry)(self._C.byref(self._a), s), self.entry)
        H.check(H.lib().air_scene_source_advance(self.counter.data_ptr(), 1, s), "air_scene_source_advance")

    def labels(self, base_labels):
        """[V]: the label of the base glyph of every variant of the last refresh (a read-back)"""
        return np.asarray(base_labels)[self.source.cpu().numpy()]

    def status_counts(self):
        """device tensor [3]: the variants of the last refresh that are usable / empty / too large"""
        return self._torch.bincount(self.status, minlength=3)[:3]


class DeviceGlyphBank(_Bank):
    """The scale and rotation jitter of generate_multi_image (:113-135) on the device, as a bank: ONE launch
    (air_glyph_jitter, one workgroup per variant) turns the base `glyphs` [G, gd * gd] into `variants` jittered glyphs --
    base glyph, new_width, new_height and angle drawn per variant -- each cropped into the top-left of an od x od frame, with
    its crop box.  The arithmetic is scipy's affine_transform / rotate at order 5 in fp64 (include/air_hip.h states it), so a
    variant is the glyph Generator.multi_image would have placed for the same draws.  DeviceSceneSource takes the bank in
    place of a glyph array and draws its digits from the variants.

    refresh(): the launch, then the generation counter advanced by one -- on the current stream, nothing synchronises; every
    generation is another bank (its draws are keyed by (seed; variant, draw, generation)).  The tensors bank [V, od * od],
    bank_crops [V, 4], source [V] (the base glyph of each variant), params [V, 6] (new_width, new_height, angle, cos, sin, 0)
    and status [V] hold the last refresh.  status: 0 usable, 1 nothing left after the threshold, 2 larger than a plane limit
    or than od -- such a variant has an all-zero crop box, and a scene that draws it restarts (the reference's IndexError
    path, :177).  labels(base_labels): the label of every variant; status_counts(): a device tensor [3]."""
    struct, entry, prepare = "GlyphJitter", "air_glyph_jitter", "air_glyph_jitter_prepare"
    extra, params_width = "crops", 6

    def __init__(self, glyphs, variants, od=32, seed=0, min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0,
                 device=None):
        self._bind()
        g, gd = _glyph_array(glyphs)
        self.base_crops = crop_boxes(g, gd)
        self.bounds = dict(min_w=float(min_w), max_w=float(max_w), min_h=float(min_h), max_h=float(max_h),
                           min_ang=float(min_ang), max_ang=float(max_ang))
        self._make(g, gd, variants, od, seed, device, self.base_crops, self.bounds)

    def fits(self, canvas_dim, margin):
        """whether some base glyph, at the smallest scale that may be drawn, fits the canvas"""
        w = np.floor(self.base_crops[:, 2] * self.bounds["min_w"]) + 2 * margin
        h = np.floor(self.base_crops[:, 3] * self.bounds["min_h"]) + 2 * margin
        return bool(np.any((w <= canvas_dim) & (h <= canvas_dim)))


class DeviceHandwritingBank(_Bank):
    """Base glyphs distorted into MNIST's geometry on the device, as a bank: ONE launch (air_glyph_distort, one workgroup per
    variant) turns the whole planes `base_glyphs` [G, gd * gd] (values in [0, 1], gd <= 40) into `variants` glyphs -- base
    glyph, angle, shear, two scales and stroke passes drawn per variant, an elastic displacement field of standard deviation
    `alpha` base pixels smoothed by a Gaussian of `sigma` -- each with its box fitted to `ink` pixels a side and put by its
    centre of mass into an od x od frame.  include/air_hip.h states every operation; tests/glyph_distort_cases.py restates
    them in numpy, bit for bit.  The taps (a normalised Gaussian of radius int(4 sigma + 0.5), or `radius`) and the field's
    gain alpha / ((1 / sqrt 3) * sum taps^2) are made here, on the host.

    The attributes and methods are DeviceGlyphBank's, and DeviceSceneSource takes either; here params is [V, 8] (angle, shear,
    sx, sy, cos, sin, stroke passes, fit factor) and status 1 is nothing left after the ramp or the fit, 2 larger than od."""
    struct, entry, prepare = "GlyphDistort", "air_glyph_distort", "air_glyph_distort_prepare"
    extra, params_width = "taps", 8

    def __init__(self, base_glyphs, variants, od=28, ink=20, seed=0, max_ang=0.0, max_shear=0.0, min_scale=1.0, max_scale=1.0,
                 min_stroke=0, max_stroke=0, lo=0.0, hi=1.0, sigma=1.0, alpha=0.0, radius=None, device=None):
        self._bind()
        g, gd = _glyph_array(base_glyphs)
        if g.max() > 1:
            raise ValueError("glyph values must be <= 1")
        if not (np.isfinite(sigma) and sigma > 0 and np.isfinite(alpha)):
            raise ValueError("sigma must be positive, sigma and alpha finite")
        self.ink = int(ink)
        fields = dict(max_ang=float(max_ang), max_shear=float(max_shear), min_scale=float(min_scale), max_scale=float(max_scale),
                      min_stroke=int(min_stroke), max_stroke=int(max_stroke), lo=float(lo), hi=float(hi))
        self.bounds = dict(fields, sigma=float(sigma), alpha=float(alpha))
        taps, self.radius = gaussian_taps(sigma, radius)
        self.field_gain = float(alpha) / ((1.0 / np.sqrt(3.0)) * float(np.sum(taps * taps))) if alpha != 0.0 else 0.0
        self._make(g, gd, variants, od, seed, device, taps,
                   dict(fields, ink=self.ink, radius=self.radius, field_gain=self.field_gain))

    def fits(self, canvas_dim, margin):
        """whether a usable variant, whose larger side is at most `ink` pixels, fits the canvas"""
        return self.ink + 2 * margin <= canvas_dim


class _FixedBank:
    """a plain glyph array [G, gd * gd] as the bank that never turns over: what DeviceSceneSource reads of a bank"""

    def __init__(self, glyphs, device):
        import torch
        g, self.od = _glyph_array(glyphs)
        self.boxes = crop_boxes(g, self.od)
        self.variants, self.device = len(g), device
        self.bank, self.bank_crops = torch.tensor(g, device=device), torch.tensor(self.boxes, device=device)

    def fits(self, canvas_dim, margin):
        return bool(np.any((self.boxes[:, 2] + 2 * margin <= canvas_dim) & (self.boxes[:, 3] + 2 * margin <= canvas_dim)))

    def refresh(self):
        pass


# ----------------------------------------------------------------------------- the feeds
class _Feed(_Device):
    """next_batch() / graph_hooks(steps): a batch on the current stream, or the hook that AIRModel.capture_graph(steps,
    between_steps=) records into its replay.  One object feeds one way: once graph_hooks has been taken -- for a positive
    `steps`, the same at every call -- an eager batch is refused.  A feed gives `noun`, _eager() and _between(steps)."""
    _steps = None               # steps per replay once graph_hooks has been taken

    def next_batch(self, _i=0):
        if self._steps is not None:
            raise RuntimeError("this %s feeds a captured graph (graph_hooks): batches come out of its replays" % self.noun)
        self._eager()

    def graph_hooks(self, steps):
        """-> (between_steps, after_steps) for AIRModel.capture_graph"""
        if steps < 1:
            raise ValueError("steps per replay must be positive")
        if self._steps is None:
            self._steps = steps
        elif self._steps != steps:
            raise ValueError("graph_hooks was set up for %d steps per replay" % self._steps)
        return self._between(steps), None


class ShuffleBatchQueue(_Feed):
    """read_and_decode (:228-249) on the device: tf.train.shuffle_batch([image, digits], batch_size,
    capacity=10000 + 10 * batch_size, min_after_dequeue=10000) over the epoch-repeating record stream of ONE reader
    (training.py:76-81), the decoded records resident in HBM.  `images` [n, D] float32 / `digits` [n] int32 are device
    tensors; every batch lands in the caller's `out_images` [B, D] / `out_digits` [B] (the train model's input buffers).

    next_batch(): dequeue + gather on the current stream (two launches in front of the step that consumes the batch).
    graph_hooks(steps): the form for AIRModel.capture_graph(steps, between_steps=): the captured replay starts with ONE
    launch that makes the picks of all its `steps` batches into a device table (air_shuffle_batch_dequeue_many, the queue
    staged in LDS once) and holds one more launch per step, the row gather of that step's batch.  The batches are the same
    sequence either way, pick for pick the numpy model of the reference's queue that tests/test_shuffle_queue.py holds.
    (Measured on one MI355X, 50 steps per replay, ms per train step: no input work 0.1774; a gather per step 0.1801; this
    form 0.1815; a serial dequeue + gather in front of every step 0.186-0.190; a dequeue_many concurrent with the steps --
    on a forked branch of the graph or on a second stream -- 0.2085: DESIGN.md section 11.3.)"""
    noun = "queue"

    def __init__(self, images, digits, batch_size, out_images, out_digits, seed=0, min_after_dequeue=10000):
        C, torch, H = self._bind()
        dev = self.device = images.device
        self.images, self.digits, self.out_images, self.out_digits = images, digits, out_images, out_digits
        self.batch, self.D = int(batch_size), int(images.shape[1])
        self.capacity = min_after_dequeue + 10 * self.batch                       # :246
        self.queue = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)
        self.picks = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self._sq = H.ShuffleBatch(self.queue.data_ptr(), self.state.data_ptr(), self.picks.data_ptr(), self.capacity,
                                  self.batch, min_after_dequeue, int(images.shape[0]), seed)
        self._table = None          # [steps, batch] picks of the replay about to run (read by the captured gathers)
        H.check(H.lib().air_shuffle_batch_init(C.byref(self._sq), self._s()), "air_shuffle_batch_init")

    def _gather(self, picks):
        H = self._H
        H.check(H.lib().air_batch_gather(self.images.data_ptr(), self.digits.data_ptr(), picks.data_ptr(),
                                         self.out_images.data_ptr(), self.out_digits.data_ptr(), self.batch, self.D, self._s()),
                "air_batch_gather")

    def _eager(self):
        H = self._H
        H.check(H.lib().air_shuffle_batch_dequeue(self._C.byref(self._sq), self._s()), "air_shuffle_batch_dequeue")
        self._gather(self.picks)

    def _between(self, steps):
        if self._table is None:
            self._table = self._torch.zeros(steps, self.batch, dtype=self._torch.int32, device=self.device)

        def between_steps(i):
            H = self._H
            if i == 0:                                   # the picks of the replay's batches: the replay's first launch
                H.check(H.lib().air_shuffle_batch_dequeue_many(self._C.byref(self._sq), steps, self._table.data_ptr(), self._s()),
                        "air_shuffle_batch_dequeue_many")
            self._gather(self._table[i])
        return between_steps


class DeviceSceneSource(_Feed):
    """generate_multi_image (:82-183) on the device, default path only (pixel overlap with the optional gap buffer, margin,
    background): every batch is COMPOSED by one launch (air_scene_source_compose, one workgroup per canvas) straight into
    the caller's `out_images` [B, canvas_dim^2] float32 / `out_digits` [B] int32 -- the train model's input buffers -- so a
    run needs no data set and never sees a canvas twice.  `glyphs` [G, gd * gd] (numpy or tensor, values >= 0, gd <= 32);
    `bg` [canvas_dim, canvas_dim] or None; `counts` [B] int32 fixes the digit count of every slot of a batch (None: drawn
    uniformly from 0 .. max_digits, the mix of the strata of generate_dataset).

    The methods of ShuffleBatchQueue, with its contracts: next_batch() makes one batch on the current stream (compose +
    the one-thread launch that advances the device batch counter); graph_hooks(steps) is the form for
    AIRModel.capture_graph(steps, between_steps=): one compose in front of every step, the counter advanced by `steps`
    behind the last, so replays continue the sequence without the host.  Batch k holds the same scenes either way: its
    draws are Philox4x32-10 words keyed by (seed; slot, draw, k) -- include/air_hip.h has the draw order.
    meta(): the device tensors indices / positions / boxes / status of the last batch (status: restarts of the rejection
    sampler, -1 = given up after max_restarts: an empty canvas with 0 digits).  gave_up(): a device scalar, the number of
    such canvases over all batches so far; nothing here synchronises.

    `glyphs` may be a DeviceGlyphBank or a DeviceHandwritingBank instead: the source then draws from the bank's variants (its
    frames and crop boxes, gd = the bank's od; meta()['indices'] are bank indices, bank.source maps them to base glyphs), and
    graph_hooks(steps) enqueues bank.refresh() in front of the first compose of every replay.  next_batch() does not
    refresh: the caller decides when the bank turns over; fresh_batch() is the two together, a batch from a bank of its own.

    Against the host generator: glyph indices are drawn uniformly instead of walking a permutation, and the restart loop
    is bounded.  Jitter keywords here are refused (the jitter is the bank's); bounding-box overlap exists only in
    Generator.multi_image."""
    noun = "source"

    def __init__(self, glyphs, batch_size, out_images, out_digits, canvas_dim=50, max_digits=2, margin=0, gap=0,
                 bg=None, counts=None, seed=0, max_attempts=100, max_restarts=32, use_pixel_overlap=True, **jitter):
        C, torch, H = self._bind()
        unknown = sorted(set(jitter) - set(JITTER_NEUTRAL))
        if unknown:
            raise TypeError("unexpected arguments: %s" % ", ".join(unknown))
        if any(float(jitter[k]) != v for k, v in JITTER_NEUTRAL.items() if k in jitter):
            raise NotImplementedError("scale / rotation jitter is not an option of the scene source: pass a DeviceGlyphBank built "
                                      "with these bounds as `glyphs`, or use the host generator, "
                                      "multi_mnist.Generator.multi_image")
        if not use_pixel_overlap:
            raise NotImplementedError("bounding-box overlap is not composed on the device: use the host generator, "
                                      "multi_mnist.Generator.multi_image(use_pixel_overlap=False)")
        H.require_device(out_images, "out_images", "DeviceSceneSource")
        H.require_device(out_digits, "out_digits", "DeviceSceneSource")
        dev = self.device = out_images.device
        self.bank = glyphs if isinstance(glyphs, _Bank) else None
        table = self._glyph_table = _FixedBank(glyphs, dev) if self.bank is None else self.bank
        if table.device != dev:
            raise ValueError("the glyph bank lives on %s, out_images on %s" % (table.device, dev))
        self.batch, self.canvas_dim, self.max_digits = int(batch_size), int(canvas_dim), int(max_digits)
        B, D, md = self.batch, self.canvas_dim ** 2, self.max_digits
        if tuple(out_images.shape) != (B, D) or out_images.dtype != torch.float32 or not out_images.is_contiguous():
            raise ValueError("out_images must be a contiguous float32 [%d, %d]" % (B, D))
        if tuple(out_digits.shape) != (B,) or out_digits.dtype != torch.int32:
            raise ValueError("out_digits must be an int32 [%d]" % B)
        if not table.fits(canvas_dim, margin):
            raise ValueError("no glyph fits a %d x %d canvas with margin %d" % (canvas_dim, canvas_dim, margin))
        self.out_images, self.out_digits = out_images, out_digits
        self.glyphs, self.crops = table.bank, table.bank_crops
        self.bg = None if bg is None else torch.tensor(np.ascontiguousarray(bg, np.float32).reshape(-1), device=dev)
        if self.bg is not None and self.bg.numel() != D:
            raise ValueError("bg must be [%d, %d]" % (canvas_dim, canvas_dim))
        self.counts = None
        if counts is not None:
            self.counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
            if tuple(self.counts.shape) != (B,):
                raise ValueError("counts must be [%d]" % B)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)          # batches made so far (device: replays move it)
        self.indices = torch.zeros(B, md, dtype=torch.int32, device=dev)
        self.positions = torch.zeros(B, 2 * md, dtype=torch.int32, device=dev)
        self.boxes = torch.zeros(B, 2 * md, dtype=torch.int32, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self._gave_up = torch.zeros(B, dtype=torch.int32, device=dev)         # per slot; gave_up() sums it
        self._a = H.SceneSource(
            self.glyphs.data_ptr(), self.crops.data_ptr(), self.bg.data_ptr() if self.bg is not None else None,
            self.counts.data_ptr() if self.counts is not None else None, self.counter.data_ptr(),
            out_images.data_ptr(), out_digits.data_ptr(), self.indices.data_ptr(), self.positions.data_ptr(),
            self.boxes.data_ptr(), self.status.data_ptr(), self._gave_up.data_ptr(),
            B, table.variants, table.od, self.canvas_dim, int(margin), int(gap), md, int(max_attempts), int(max_restarts),
            int(seed) & 0xFFFFFFFFFFFFFFFF)
        # the argument checks and the LDS grant now: the first compose may be enqueued under stream capture
        with torch.cuda.device(dev):
            H.check(H.lib().air_scene_source_prepare(C.byref(self._a)), "air_scene_source_prepare")

    def _compose(self, step_in_replay):
        H = self._H
        H.check(H.lib().air_scene_source_compose(self._C.byref(self._a), step_in_replay, self._s()), "air_scene_source_compose")

    def _advance(self, by):
        H = self._H
        H.check(H.lib().air_scene_source_advance(self.counter.data_ptr(), by, self._s()), "air_scene_source_advance")

    def _eager(self):
        self._compose(0)
        self._advance(1)

    def _between(self, steps):
        def between_steps(i):
            if i == 0:                                   # a fresh bank for every replay, made by the replay itself
                self._glyph_table.refresh()
            self._compose(i)
            if i == steps - 1:                           # behind the last compose of the replay: the next replay goes on
                self._advance(steps)
        return between_steps

    def fresh_batch(self):
        """the bank turned over (a plain glyph array has nothing to turn over), then next_batch()"""
        if self._steps is None:                          # (otherwise next_batch() refuses, and the bank is left as it is)
            self._glyph_table.refresh()
        self.next_batch()

    def meta(self):
        return dict(indices=self.indices, positions=self.positions, boxes=self.boxes, status=self.status)

    def gave_up(self):
        return self._gave_up.sum()
