"""Multi-digit canvas generator -- restatement of the DEFAULT path of the reference's
multi_mnist.py (generate_multi_image :82-183 with use_pixel_overlap=True, the __main__
driver :299-414) in numpy, writing .npz instead of TFRecords.

Glyph source: real MNIST idx files are used if present under ``mnist_data/`` (the reference
downloads them, :336 -- impossible here, no network); otherwise the 1 797 8x8 glyphs of
sklearn's ``load_digits`` (committed as data/digits8x8.npz), up-sampled (cubic) to 12x12 inside a
28x28 frame with the ink ramp stretched so that strokes saturate like MNIST's (the rendering
that trains most reliably of those tried: with 16x16 or larger glyphs most seeds stall on an
over-counting plateau, with 12x12 every fp32 seed ends at 96-99 % digit-count accuracy --
profiles/r01_glyph_sweep*_60k.jsonl, profiles/r01_seed_sweep_12px_120k.jsonl).  Everything downstream (cropping, rejection sampling of
non-overlapping positions, strata of 0..max_digits digits, shuffling, 1 000-image test split)
follows the reference.

  python multi_mnist.py [--max-digits 2] [--images-per-digit 20000] [--test-set-size 1000]
                        [--digit-gap 0] [--canvas-margin 0] [--bg-path X --bg-max-intensity 1.0]
  python multi_mnist.py --device 60000 [--seed 0] [...]     the same files, composed on the GPU (DeviceSceneSource; with
                        --min-width-scale ... --max-rotation-angle from a DeviceGlyphBank remade for every batch; with
                        --glyph-style mnist-like from a DeviceHandwritingBank remade for every batch)

DeviceSceneSource is that default path as device work: one HIP launch composes a fresh batch of canvases into the train
model's input buffers (training.py --online-data), eagerly or inside a captured replay.  DeviceGlyphBank is the scale and
rotation jitter (:113-135) as device work: one launch makes a bank of jittered variants of the glyphs, with scipy's order-5
spline arithmetic, and a scene source built on the bank draws from those.  DeviceHandwritingBank is a bank of another kind
(--glyph-style mnist-like): the 8x8 handwritten digits up-sampled to 40x40 (load_base_glyphs) and distorted on the device
into MNIST's geometry -- elastic field, affine map, stroke width, ink ramp, a 20-pixel box centred by its centre of mass in a
28x28 frame -- by one launch per bank (air_glyph_distort).
"""
import argparse
import gzip
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CANVAS_SIZE = 50
IMAGE_SIZE = 28
MNIST_FOLDER = "mnist_data/"
MULTI_MNIST_FOLDER = "multi_mnist_data/"


def load_glyphs():
    """[n, 28*28] float32 in [0,1] + labels; MNIST if available, else up-sampled 8x8 digits."""
    for name in ("train-images-idx3-ubyte", "train-images-idx3-ubyte.gz"):
        p = os.path.join(MNIST_FOLDER, name)
        if os.path.exists(p):
            op = gzip.open if p.endswith(".gz") else open
            with op(p, "rb") as f:
                _, n, r, c = struct.unpack(">IIII", f.read(16))
                imgs = np.frombuffer(f.read(), np.uint8).reshape(n, r * c).astype(np.float32) / 255.0
            lp = p.replace("images-idx3", "labels-idx1")
            with op(lp, "rb") as f:
                f.read(8)
                labels = np.frombuffer(f.read(), np.uint8).astype(np.int64)
            return imgs, labels, "mnist"
    import scipy.ndimage as nd
    d = np.load(os.path.join(HERE, "data", "digits8x8.npz"))
    small = d["images"].astype(np.float32) / 16.0
    out = np.zeros((small.shape[0], IMAGE_SIZE, IMAGE_SIZE), np.float32)
    zoom = float(os.environ.get("AIR_GLYPH_ZOOM", "1.5"))                 # 8x8 -> 12x12: fits the scale prior (sigmoid(-1) * 50 = 13.4 px)
    order = int(os.environ.get("AIR_GLYPH_ORDER", "3"))                   # spline order of the up-sampling
    lo, hi = (float(v) for v in os.environ.get("AIR_GLYPH_CONTRAST", "0.25,0.65").split(","))   # ink ramp: MNIST strokes saturate
    for i, g in enumerate(small):
        big = np.clip(nd.zoom(g, zoom, order=order), 0.0, 1.0)
        big = np.clip((big - lo) / (hi - lo), 0.0, 1.0)
        big = np.where(big >= 0.15, big, 0.0)
        o = (IMAGE_SIZE - big.shape[0]) // 2
        out[i, o:o + big.shape[0], o:o + big.shape[1]] = big
    return out.reshape(-1, IMAGE_SIZE * IMAGE_SIZE), d["labels"].astype(np.int64), "digits8x8"


def load_base_glyphs(side=40):
    """[n, side * side] float32 in [0, 1] + labels: the committed 8x8 handwritten digits up-sampled (cubic) to side x side
    and clipped -- the base planes of DeviceHandwritingBank, which gives them stroke, ramp, size and place itself"""
    import scipy.ndimage as nd
    d = np.load(os.path.join(HERE, "data", "digits8x8.npz"))
    small = d["images"].astype(np.float32) / 16.0
    out = np.stack([np.clip(nd.zoom(g, side / 8.0, order=3), 0.0, 1.0) for g in small]).astype(np.float32)
    return out.reshape(-1, side * side), d["labels"].astype(np.int64)


def read_image(path, max_intensity):
    """multi_mnist.py:17-33 (backgrounds)."""
    from PIL import Image
    image = np.asarray(Image.open(path).convert("L"), dtype=np.float32) / 255.0
    img_min, img_max = image.min(), image.max()
    if img_min != img_max:
        if img_min > 0.0:
            image = image - img_min
        if img_max > 0.0:
            image = image / img_max
        if max_intensity < 1.0:
            image = image * max_intensity
    else:
        if img_max > max_intensity:
            image = np.ones_like(image) * max_intensity
    return image


def crop_non_empty(image):
    """:36-43"""
    cols = np.nonzero(np.sum(image, axis=0))[0]
    rows = np.nonzero(np.sum(image, axis=1))[0]
    return image[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]


def add_buffer(image, buffer_width):
    """:44-58 -- every empty pixel within `buffer_width` (Chebyshev) of an ink pixel becomes 1:
    a dilation by a (2b+1)^2 square, used to keep a gap between digits under pixel overlap."""
    import scipy.ndimage as nd
    b = buffer_width
    near = nd.maximum_filter((image > 0).astype(np.uint8), size=2 * b + 1, mode="constant", cval=0) > 0
    return np.where((image == 0) & near, np.float32(1.0), image).astype(image.dtype)


def pixels_overlap(canvas, image, x, y):
    """:61-65"""
    h, w = image.shape
    window = canvas[y:y + h, x:x + w]
    return not np.array_equal(np.maximum(image, window), image + window)


def bounding_boxes_overlap(x, y, w, h, positions, boxes, gap):
    """:68-79, with the reference's exact tests: a candidate is rejected as soon as its
    gap-inflated x-extent intersects a placed box's x-extent (whatever the rows), and also in the
    (degenerate) case l1y >= r2y and l2y >= r1y."""
    l1x, l1y, r1x, r1y = x - gap, y - gap, x + w + gap - 1, y + h + gap - 1
    for i in range(len(positions) // 2):
        px, py = positions[2 * i], positions[2 * i + 1]
        bw, bh = boxes[2 * i], boxes[2 * i + 1]
        l2x, l2y, r2x, r2y = px, py, px + bw - 1, py + bh - 1
        if l1x <= r2x and l2x <= r1x:
            return True
        if l1y >= r2y and l2y >= r1y:
            return True
    return False


class Generator:
    """State of the reference's module-level globals (digit_ids, next_digit_id :82-85, :343-346)."""

    def __init__(self, glyphs, rng):
        self.glyphs = glyphs
        self.rng = rng
        self.digit_ids = rng.permutation(len(glyphs))
        self.next = 0

    def multi_image(self, num_images, canvas_dim=CANVAS_SIZE, image_dim=IMAGE_SIZE, bg=None,
                    min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0,
                    gap=0, margin=0, use_pixel_overlap=True):
        """generate_multi_image :82-183: scale / rotation jitter with order-5 splines (:117-139),
        rejection sampling of positions (up to 100 attempts, then the whole image is restarted)
        under pixel overlap (with an optional gap buffer) or bounding-box overlap."""
        import scipy.ndimage as nd
        rng = self.rng
        while True:
            canvas = np.zeros([canvas_dim, canvas_dim], np.float32)
            canvas_with_buffer = canvas
            ids, positions, boxes = [], [], []
            if num_images == 0:
                break
            ok = True
            for i in range(num_images):
                idx = self.digit_ids[self.next]
                self.next += 1
                if self.next >= len(self.digit_ids):
                    self.digit_ids = rng.permutation(self.digit_ids)
                    self.next = 0
                image = crop_non_empty(self.glyphs[idx].reshape(image_dim, image_dim))
                if min_w != 1.0 or max_w != 1.0 or min_h != 1.0 or max_h != 1.0:
                    new_width = rng.uniform(min_w, max_w)
                    new_height = rng.uniform(min_h, max_h)
                    image = nd.affine_transform(image, matrix=np.array([[1.0 / new_height, 0.0], [0.0, 1.0 / new_width]]),
                                                output_shape=(int(image_dim * new_height), int(image_dim * new_width)),
                                                order=5)
                    image = np.clip(image, 0.0, 1.0)
                    image = crop_non_empty(np.where(image >= 0.05, image, np.zeros_like(image)))
                if min_ang != 0.0 or max_ang != 0.0:
                    image = nd.rotate(image, rng.uniform(min_ang, max_ang), order=5)
                    image = np.clip(image, 0.0, 1.0)
                    image = crop_non_empty(np.where(image >= 0.05, image, np.zeros_like(image)))
                h, w = image.shape
                if w + 2 * margin > canvas_dim or h + 2 * margin > canvas_dim:
                    ok = False                                   # (the reference's IndexError path :166)
                    break
                found = False
                for _ in range(100):
                    x = rng.randint(margin, canvas_dim - w - margin + 1)
                    y = rng.randint(margin, canvas_dim - h - margin + 1)
                    if i == 0:
                        found = True
                    elif use_pixel_overlap:
                        found = not pixels_overlap(canvas_with_buffer, image, x, y)
                    else:
                        found = not bounding_boxes_overlap(x, y, w, h, positions, boxes, gap)
                    if found:
                        break
                if not found:
                    ok = False
                    break
                canvas[y:y + h, x:x + w] += image
                if use_pixel_overlap and num_images > 1:
                    canvas_with_buffer = add_buffer(canvas, gap) if gap > 0 else canvas
                positions.extend([x, y])
                boxes.extend([w, h])
                ids.append(idx)
            if ok:
                break
        if bg is not None:
            canvas = np.clip(canvas + bg, 0.0, 1.0)
        return canvas, ids, positions, boxes


def generate_strata(max_digits=2, images_per_digit=20000, seed=0, bg=None, canvas_dim=CANVAS_SIZE, verbose=False,
                    **jitter):
    """__main__ :341-381: one stratum of `images_per_digit` canvases per digit count, with the
    metadata the reference stores (glyph indices, positions, boxes, labels)."""
    glyphs, labels, source = load_glyphs()
    rng = np.random.RandomState(seed)                                   # np.random.seed(0) :341
    gen = Generator(glyphs, rng)
    strata = []
    for nd_ in range(max_digits + 1):
        st = dict(images=[], indices=[], positions=[], boxes=[], labels=[], digits=[])
        for item in range(images_per_digit):
            img, ids, pos, box = gen.multi_image(nd_, canvas_dim=canvas_dim, bg=bg, **jitter)
            st["images"].append(img.reshape(-1))
            st["indices"].append(list(ids)); st["positions"].append(list(pos)); st["boxes"].append(list(box))
            st["labels"].append([int(labels[i]) for i in ids]); st["digits"].append(nd_)
            if verbose and (item + 1) % 5000 == 0:
                print("%d digits: %d done" % (nd_, item + 1), flush=True)
        strata.append(st)
    return strata, rng, source


def generate_dataset(max_digits=2, images_per_digit=20000, test_set_size=1000, seed=0, bg=None, margin=0,
                     canvas_dim=CANVAS_SIZE, verbose=False, **jitter):
    """__main__ :341-413: strata of 0..max_digits digits, shuffled together, first
    `test_set_size` images -> test, the rest -> train.  Returns dict of arrays."""
    strata, rng, source = generate_strata(max_digits, images_per_digit, seed, bg, canvas_dim, verbose,
                                          margin=margin, **jitter)
    images = np.stack([im for st in strata for im in st["images"]]).astype(np.float32)
    digits = np.asarray([d for st in strata for d in st["digits"]], np.int32)
    perm = rng.permutation(len(images))                                 # shuffle_lists :215-225
    images, digits = images[perm], digits[perm]
    # the ground truth of the test rows, carried through the same shuffle: [test_set_size, max(max_digits, 1), 2] int32
    test = perm[:test_set_size]
    positions, boxes, labels = ([lst for st in strata for lst in st[k]] for k in ("positions", "boxes", "labels"))
    return dict(test_labels=padded_labels([labels[i] for i in test], digits[:test_set_size], max_digits),
                train_images=images[test_set_size:], train_digits=digits[test_set_size:],
                test_images=images[:test_set_size], test_digits=digits[:test_set_size], source=source,
                test_positions=padded_truth([positions[i] for i in test], digits[:test_set_size], max_digits),
                test_boxes=padded_truth([boxes[i] for i in test], digits[:test_set_size], max_digits))


def padded(lists, digits, width, max_digits=None):
    """per-image flat lists of `width` values per digit -> int32 [n, G, width], zeros behind digits[i]; G = max_digits (at
    least 1), or the largest count when None: the layout air_embed_collect and air_localization read"""
    digits = np.asarray(digits, np.int64).reshape(-1)
    G = max(1, int(digits.max()) if max_digits is None and len(digits) else int(max_digits or 1))
    out = np.zeros((len(digits), G, width), np.int32)
    for i, n in enumerate(digits):
        if n:
            out[i, :n] = np.asarray(lists[i], np.int32).reshape(-1)[:width * n].reshape(n, width)
    return out


def padded_truth(lists, digits, max_digits=None):
    """per-image flat lists [x0, y0, x1, y1, ...] (positions, or boxes as w, h) -> int32 [n, G, 2]"""
    return padded(lists, digits, 2, max_digits)


def padded_labels(lists, digits, max_digits=None):
    """per-image label lists -> int32 [n, G]"""
    out = padded(lists, digits, 1, max_digits)
    return out.reshape(out.shape[:2])


# ----------------------------------------------------------------------------- reference file format
def write_to_records(filename, images, indices, positions, boxes, labels, digits, side=None):
    """:186-212 -- `filename`.tfrecords with the reference's feature set (height, width, digits as
    int64; indices / positions / boxes / labels as raw int32 bytes; image as raw float32 bytes)."""
    import tfrecord
    recs = []
    for k in range(len(images)):
        img = np.asarray(images[k], np.float32)
        rows = cols = side if side is not None else (img.shape[0] if img.ndim == 2 else int(round(np.sqrt(img.size))))
        recs.append(tfrecord.encode_example({
            "height": ("int64", [rows]), "width": ("int64", [cols]), "digits": ("int64", [int(digits[k])]),
            "indices": ("bytes", [np.asarray(indices[k], np.int32).tobytes()]),
            "positions": ("bytes", [np.asarray(positions[k], np.int32).tobytes()]),
            "boxes": ("bytes", [np.asarray(boxes[k], np.int32).tobytes()]),
            "labels": ("bytes", [np.asarray(labels[k], np.int32).tobytes()]),
            "image": ("bytes", [np.ravel(img).tobytes()]),
        }))
    return tfrecord.write_records(filename + ".tfrecords", recs)


class ShuffleBatchQueue:
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

    def __init__(self, images, digits, batch_size, out_images, out_digits, seed=0, min_after_dequeue=10000):
        import ctypes as C
        import torch
        from air import _hip as H
        self._C, self._torch, self._H = C, torch, H
        dev = images.device
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

    def _s(self):
        return self._H.stream(self.images.device)

    def _gather(self, picks):
        H = self._H
        H.check(H.lib().air_batch_gather(self.images.data_ptr(), self.digits.data_ptr(), picks.data_ptr(),
                                         self.out_images.data_ptr(), self.out_digits.data_ptr(), self.batch, self.D, self._s()),
                "air_batch_gather")

    def next_batch(self, _i=0):
        H = self._H
        if self._table is not None:
            raise RuntimeError("this queue feeds a captured graph (graph_hooks): batches come out of its replays")
        H.check(H.lib().air_shuffle_batch_dequeue(self._C.byref(self._sq), self._s()), "air_shuffle_batch_dequeue")
        self._gather(self.picks)

    def graph_hooks(self, steps):
        """-> (between_steps, after_steps) for AIRModel.capture_graph"""
        if steps < 1:
            raise ValueError("steps per replay must be positive")
        if self._table is None:
            self._table = self._torch.zeros(steps, self.batch, dtype=self._torch.int32, device=self.images.device)
        elif self._table.shape[0] != steps:
            raise ValueError("graph_hooks was set up for %d steps per replay" % self._table.shape[0])

        def between_steps(i):
            H = self._H
            if i == 0:                                   # the picks of the replay's batches: the replay's first launch
                H.check(H.lib().air_shuffle_batch_dequeue_many(self._C.byref(self._sq), steps, self._table.data_ptr(), self._s()),
                        "air_shuffle_batch_dequeue_many")
            self._gather(self._table[i])
        return between_steps, None


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


JITTER_NEUTRAL = dict(min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0)


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


class DeviceGlyphBank:
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

    def __init__(self, glyphs, variants, od=32, seed=0, min_w=1.0, max_w=1.0, min_h=1.0, max_h=1.0, min_ang=0.0, max_ang=0.0,
                 device=None):
        import ctypes as C
        import torch
        from air import _hip as H
        self._C, self._torch, self._H = C, torch, H
        g, gd = _glyph_array(glyphs)
        self.base_crops = crop_boxes(g, gd)
        self.variants, self.gd, self.od = int(variants), gd, int(od)
        self.bounds = dict(min_w=float(min_w), max_w=float(max_w), min_h=float(min_h), max_h=float(max_h),
                           min_ang=float(min_ang), max_ang=float(max_ang))
        V = self.variants
        # the argument checks first, before anything is allocated: they need no device (the pointers are placeholders that
        # the checks only compare with null and test for alignment)
        self._a = H.GlyphJitter(16, 16, None, 16, 16, 16, 16, 16, V, len(g), gd, self.od,
                                *[self.bounds[k] for k in ("min_w", "max_w", "min_h", "max_h", "min_ang", "max_ang")],
                                int(seed) & 0xFFFFFFFFFFFFFFFF)
        H.check(H.lib().air_glyph_jitter_prepare(C.byref(self._a)), "air_glyph_jitter_prepare")
        if device is None and not torch.cuda.is_available():
            raise H.AirHipError("DeviceGlyphBank: needs a GPU (no CPU fallback)")
        dev = self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise H.AirHipError("DeviceGlyphBank: device must be a GPU (no CPU fallback)")
        self.glyphs = torch.tensor(g, device=dev)
        self.crops = torch.tensor(self.base_crops, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)           # the bank generation (device: replays move it)
        self.bank = torch.zeros(V, self.od * self.od, device=dev)
        self.bank_crops = torch.zeros(V, 4, dtype=torch.int32, device=dev)
        self.source = torch.zeros(V, dtype=torch.int32, device=dev)
        self.params = torch.zeros(V, 6, dtype=torch.float64, device=dev)
        self.status = torch.ones(V, dtype=torch.int32, device=dev)             # (nothing is usable before the first refresh)
        for k in ("glyphs", "crops", "counter", "bank", "bank_crops", "source", "params", "status"):
            setattr(self._a, k, getattr(self, k).data_ptr())
        H.check(H.lib().air_glyph_jitter_prepare(C.byref(self._a)), "air_glyph_jitter_prepare")

    def refresh(self):
        H = self._H
        s = H.stream(self.device)
        H.check(H.lib().air_glyph_jitter(self._C.byref(self._a), s), "air_glyph_jitter")
        H.check(H.lib().air_scene_source_advance(self.counter.data_ptr(), 1, s), "air_scene_source_advance")

    def labels(self, base_labels):
        """[V]: the label of the base glyph of every variant of the last refresh (a read-back)"""
        return np.asarray(base_labels)[self.source.cpu().numpy()]

    def status_counts(self):
        """device tensor [3]: the variants of the last refresh that are usable / empty / too large"""
        return self._torch.bincount(self.status, minlength=3)[:3]

    def fits(self, canvas_dim, margin):
        """whether some base glyph, at the smallest scale that may be drawn, fits the canvas"""
        w = np.floor(self.base_crops[:, 2] * self.bounds["min_w"]) + 2 * margin
        h = np.floor(self.base_crops[:, 3] * self.bounds["min_h"]) + 2 * margin
        return bool(np.any((w <= canvas_dim) & (h <= canvas_dim)))


# The handwriting bank's starting values (a CPU prototype of the recipe read as MNIST at a glance with them): 40-pixel base
# planes, a 20-pixel box in a 28-pixel frame, an elastic field of sigma 6 / alpha 1.5 base pixels (Simard's 4 / 34 at 28
# pixels is a far stronger field; this one is judged at 40 and halved by the fit), +-12 degrees, shear +-0.2, scale
# 0.85 .. 1.15 per axis, one pass of erosion or dilation at the most, and an ink ramp that saturates the strokes.
MNIST_LIKE = dict(side=40, ink=20, od=28, sigma=6.0, alpha=1.5, max_ang=12.0, max_shear=0.2, min_scale=0.85, max_scale=1.15,
                  min_stroke=-1, max_stroke=1, lo=0.3, hi=0.7)


def gaussian_taps(sigma, radius=None):
    """-> (taps [2 R + 1] float64, a normalised Gaussian; R = int(4 sigma + 0.5) unless given)"""
    R = int(4.0 * float(sigma) + 0.5) if radius is None else int(radius)
    x = np.arange(-R, R + 1, dtype=np.float64)
    t = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return t / t.sum(), R


class DeviceHandwritingBank:
    """Base glyphs distorted into MNIST's geometry on the device, as a bank: ONE launch (air_glyph_distort, one workgroup per
    variant) turns the whole planes `base_glyphs` [G, gd * gd] (values in [0, 1], gd <= 40) into `variants` glyphs -- base
    glyph, angle, shear, two scales and stroke passes drawn per variant, an elastic displacement field of standard deviation
    `alpha` base pixels smoothed by a Gaussian of `sigma` -- each with its box fitted to `ink` pixels a side and put by its
    centre of mass into an od x od frame.  include/air_hip.h states every operation; tests/glyph_distort_cases.py restates
    them in numpy, bit for bit.  The taps (a normalised Gaussian of radius int(4 sigma + 0.5), or `radius`) and the field's
    gain alpha / ((1 / sqrt 3) * sum taps^2) are made here, on the host.

    The attributes and methods are DeviceGlyphBank's, and DeviceSceneSource takes either: refresh() (the launch, then the
    generation counter advanced by one, on the current stream), bank [V, od * od], bank_crops [V, 4] = (x0, y0, w, h) inside
    the frame, source [V], params [V, 8] (angle, shear, sx, sy, cos, sin, stroke passes, fit factor), status [V] (0 usable,
    1 nothing left after the ramp or the fit, 2 larger than od), counter, labels(), status_counts(), fits()."""

    def __init__(self, base_glyphs, variants, od=28, ink=20, seed=0, max_ang=0.0, max_shear=0.0, min_scale=1.0, max_scale=1.0,
                 min_stroke=0, max_stroke=0, lo=0.0, hi=1.0, sigma=1.0, alpha=0.0, radius=None, device=None):
        import ctypes as C
        import torch
        from air import _hip as H
        self._C, self._torch, self._H = C, torch, H
        g, gd = _glyph_array(base_glyphs)
        if g.max() > 1:
            raise ValueError("glyph values must be <= 1")
        if not (np.isfinite(sigma) and sigma > 0 and np.isfinite(alpha)):
            raise ValueError("sigma must be positive, sigma and alpha finite")
        self.variants, self.gd, self.od, self.ink = int(variants), gd, int(od), int(ink)
        self.bounds = dict(max_ang=float(max_ang), max_shear=float(max_shear), min_scale=float(min_scale),
                           max_scale=float(max_scale), min_stroke=int(min_stroke), max_stroke=int(max_stroke), lo=float(lo),
                           hi=float(hi), sigma=float(sigma), alpha=float(alpha))
        taps, self.radius = gaussian_taps(sigma, radius)
        self.field_gain = float(alpha) / ((1.0 / np.sqrt(3.0)) * float(np.sum(taps * taps))) if alpha != 0.0 else 0.0
        V = self.variants
        # the argument checks first, before anything is allocated: they need no device (the pointers are placeholders that
        # the checks only compare with null and test for alignment)
        b = self.bounds
        self._a = H.GlyphDistort(16, None, 16, 16, 16, 16, 16, 16, V, len(g), gd, self.od, self.ink, self.radius,
                                 b["min_stroke"], b["max_stroke"], self.field_gain, b["max_ang"], b["max_shear"], b["min_scale"],
                                 b["max_scale"], b["lo"], b["hi"], int(seed) & 0xFFFFFFFFFFFFFFFF)
        H.check(H.lib().air_glyph_distort_prepare(C.byref(self._a)), "air_glyph_distort_prepare")
        if device is None and not torch.cuda.is_available():
            raise H.AirHipError("DeviceHandwritingBank: needs a GPU (no CPU fallback)")
        dev = self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise H.AirHipError("DeviceHandwritingBank: device must be a GPU (no CPU fallback)")
        self.glyphs = torch.tensor(g, device=dev)
        self.taps = torch.tensor(taps, dtype=torch.float64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)           # the bank generation (device: replays move it)
        self.bank = torch.zeros(V, self.od * self.od, device=dev)
        self.bank_crops = torch.zeros(V, 4, dtype=torch.int32, device=dev)
        self.source = torch.zeros(V, dtype=torch.int32, device=dev)
        self.params = torch.zeros(V, 8, dtype=torch.float64, device=dev)
        self.status = torch.ones(V, dtype=torch.int32, device=dev)             # (nothing is usable before the first refresh)
        for k in ("glyphs", "taps", "counter", "bank", "bank_crops", "source", "params", "status"):
            setattr(self._a, k, getattr(self, k).data_ptr())
        with torch.cuda.device(dev):
            H.check(H.lib().air_glyph_distort_prepare(C.byref(self._a)), "air_glyph_distort_prepare")

    def refresh(self):
        H = self._H
        s = H.stream(self.device)
        H.check(H.lib().air_glyph_distort(self._C.byref(self._a), s), "air_glyph_distort")
        H.check(H.lib().air_scene_source_advance(self.counter.data_ptr(), 1, s), "air_scene_source_advance")

    labels = DeviceGlyphBank.labels
    status_counts = DeviceGlyphBank.status_counts

    def fits(self, canvas_dim, margin):
        """whether a usable variant, whose larger side is at most `ink` pixels, fits the canvas"""
        return self.ink + 2 * margin <= canvas_dim


_BANKS = (DeviceGlyphBank, DeviceHandwritingBank)


class DeviceSceneSource:
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
    refresh: the caller decides when the bank turns over.

    Against the host generator: glyph indices are drawn uniformly instead of walking a permutation, and the restart loop
    is bounded.  Jitter keywords here are refused (the jitter is the bank's); bounding-box overlap exists only in
    Generator.multi_image."""

    def __init__(self, glyphs, batch_size, out_images, out_digits, canvas_dim=CANVAS_SIZE, max_digits=2, margin=0, gap=0,
                 bg=None, counts=None, seed=0, max_attempts=100, max_restarts=32, use_pixel_overlap=True, **jitter):
        import ctypes as C
        import torch
        from air import _hip as H
        neutral = JITTER_NEUTRAL
        unknown = sorted(set(jitter) - set(neutral))
        if unknown:
            raise TypeError("unexpected arguments: %s" % ", ".join(unknown))
        if any(float(jitter[k]) != v for k, v in neutral.items() if k in jitter):
            raise NotImplementedError("scale / rotation jitter is not an option of the scene source: pass a DeviceGlyphBank built "
                                      "with these bounds as `glyphs`, or use the host generator, "
                                      "multi_mnist.Generator.multi_image")
        if not use_pixel_overlap:
            raise NotImplementedError("bounding-box overlap is not composed on the device: use the host generator, "
                                      "multi_mnist.Generator.multi_image(use_pixel_overlap=False)")
        H.require_device(out_images, "out_images", "DeviceSceneSource")
        H.require_device(out_digits, "out_digits", "DeviceSceneSource")
        self._C, self._torch, self._H = C, torch, H
        dev = self.device = out_images.device
        self.bank = glyphs if isinstance(glyphs, _BANKS) else None
        if self.bank is not None:
            if self.bank.device != dev:
                raise ValueError("the glyph bank lives on %s, out_images on %s" % (self.bank.device, dev))
            G, gd = self.bank.variants, self.bank.od
        else:
            g, gd = _glyph_array(glyphs)
            G = len(g)
        self.batch, self.canvas_dim, self.max_digits = int(batch_size), int(canvas_dim), int(max_digits)
        B, D, md = self.batch, self.canvas_dim ** 2, self.max_digits
        if tuple(out_images.shape) != (B, D) or out_images.dtype != torch.float32 or not out_images.is_contiguous():
            raise ValueError("out_images must be a contiguous float32 [%d, %d]" % (B, D))
        if tuple(out_digits.shape) != (B,) or out_digits.dtype != torch.int32:
            raise ValueError("out_digits must be an int32 [%d]" % B)
        if self.bank is not None:
            fits = self.bank.fits(canvas_dim, margin)
        else:
            crops = crop_boxes(g, gd)
            fits = np.any((crops[:, 2] + 2 * margin <= canvas_dim) & (crops[:, 3] + 2 * margin <= canvas_dim))
        if not fits:
            raise ValueError("no glyph fits a %d x %d canvas with margin %d" % (canvas_dim, canvas_dim, margin))
        self.out_images, self.out_digits = out_images, out_digits
        if self.bank is not None:
            self.glyphs, self.crops = self.bank.bank, self.bank.bank_crops
        else:
            self.glyphs = torch.tensor(g, device=dev)
            self.crops = torch.tensor(crops, device=dev)
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
        self._steps = None          # steps per replay once graph_hooks has been taken
        self._a = H.SceneSource(
            self.glyphs.data_ptr(), self.crops.data_ptr(), self.bg.data_ptr() if self.bg is not None else None,
            self.counts.data_ptr() if self.counts is not None else None, self.counter.data_ptr(),
            out_images.data_ptr(), out_digits.data_ptr(), self.indices.data_ptr(), self.positions.data_ptr(),
            self.boxes.data_ptr(), self.status.data_ptr(), self._gave_up.data_ptr(),
            B, G, gd, self.canvas_dim, int(margin), int(gap), md, int(max_attempts), int(max_restarts),
            int(seed) & 0xFFFFFFFFFFFFFFFF)
        # the argument checks and the LDS grant now: the first compose may be enqueued under stream capture
        with torch.cuda.device(dev):
            H.check(H.lib().air_scene_source_prepare(C.byref(self._a)), "air_scene_source_prepare")

    def _s(self):
        return self._H.stream(self.device)

    def _compose(self, step_in_replay):
        H = self._H
        H.check(H.lib().air_scene_source_compose(self._C.byref(self._a), step_in_replay, self._s()), "air_scene_source_compose")

    def _advance(self, by):
        H = self._H
        H.check(H.lib().air_scene_source_advance(self.counter.data_ptr(), by, self._s()), "air_scene_source_advance")

    def next_batch(self, _i=0):
        if self._steps is not None:
            raise RuntimeError("this source feeds a captured graph (graph_hooks): batches come out of its replays")
        self._compose(0)
        self._advance(1)

    def graph_hooks(self, steps):
        """-> (between_steps, after_steps) for AIRModel.capture_graph"""
        if steps < 1:
            raise ValueError("steps per replay must be positive")
        if self._steps is None:
            self._steps = steps
        elif self._steps != steps:
            raise ValueError("graph_hooks was set up for %d steps per replay" % self._steps)

        def between_steps(i):
            if i == 0 and self.bank is not None:         # a fresh bank for every replay, made by the replay itself
                self.bank.refresh()
            self._compose(i)
            if i == steps - 1:                           # behind the last compose of the replay: the next replay goes on
                self._advance(steps)
        return between_steps, None

    def meta(self):
        return dict(indices=self.indices, positions=self.positions, boxes=self.boxes, status=self.status)

    def gave_up(self):
        return self._gave_up.sum()


def handwriting_bank(variants, seed, device, **override):
    """the DeviceHandwritingBank of the MNIST_LIKE preset on load_base_glyphs -> (bank, base labels)"""
    kw = dict(MNIST_LIKE, **override)
    base, labels = load_base_glyphs(kw.pop("side"))
    return DeviceHandwritingBank(base, variants, seed=seed, device=device, **kw), labels


def compose_on_device(num_images, max_digits=2, canvas_dim=CANVAS_SIZE, bg=None, gap=0, margin=0, seed=0, batch_size=1000,
                      variants=4096, glyph_style="standin", **generator_options):
    """`num_images` canvases from DeviceSceneSource (cuda:0), with the metadata generate_strata keeps: -> (dict of numpy
    arrays images [n, canvas_dim^2], digits, indices, positions, boxes, labels [n, max_digits] (slots behind digits[i] are
    0) and status [n], glyph source).  generator_options: scale / rotation bounds that are not neutral put a DeviceGlyphBank
    of `variants` jittered glyphs under the source, refreshed before every batch (`indices` are then indices into that
    batch's bank; `labels` are mapped through it); what the device does not compose is refused by the source.
    glyph_style "mnist-like": the digits come from a DeviceHandwritingBank of the MNIST_LIKE preset instead, remade before
    every batch in the same way; it has distortions of its own, so it is refused together with scale / rotation bounds."""
    import torch
    if glyph_style not in ("standin", "mnist-like"):
        raise ValueError("glyph_style must be 'standin' or 'mnist-like'")
    dev = torch.device("cuda", 0)
    B = min(batch_size, num_images)
    images = torch.zeros(B, canvas_dim * canvas_dim, device=dev)
    digits = torch.zeros(B, dtype=torch.int32, device=dev)
    jitter = {k: float(generator_options.pop(k)) for k in JITTER_NEUTRAL if k in generator_options}
    bank = glyphs = None
    jittered = any(v != JITTER_NEUTRAL[k] for k, v in jitter.items())
    if glyph_style == "mnist-like":
        if jittered:
            raise ValueError("glyph_style='mnist-like' distorts the glyphs itself: leave the scale / rotation bounds neutral")
        bank, labels = handwriting_bank(variants, seed, dev)
        source = "digits8x8, mnist-like"
    else:
        glyphs, labels, source = load_glyphs()
        if jittered:
            bank = DeviceGlyphBank(glyphs, variants, seed=seed, device=dev, **jitter)
    src = DeviceSceneSource(glyphs if bank is None else bank, B, images, digits, canvas_dim=canvas_dim, max_digits=max_digits,
                            margin=margin, gap=gap, bg=bg, seed=seed, **generator_options)
    out = {k: [] for k in ("images", "digits", "indices", "positions", "boxes", "status", "labels")}
    for _ in range((num_images + B - 1) // B):
        if bank is not None:
            bank.refresh()
        src.next_batch()
        out["images"].append(images.cpu().numpy())
        out["digits"].append(digits.cpu().numpy())
        for k, v in src.meta().items():
            out[k].append(v.cpu().numpy())
        out["labels"].append((labels if bank is None else bank.labels(labels))[out["indices"][-1]])
    out = {k: np.concatenate(v)[:num_images] for k, v in out.items()}
    used = np.arange(max_digits)[None, :] < out["digits"][:, None]
    out["labels"] = np.where(used, out["labels"], 0).astype(np.int32)
    return out, source


def read_test_data(filename, shift_zero_digits_images=False):
    """:254-296 -- reads a .tfrecords file written by the reference (or by write_to_records)."""
    import tfrecord
    images_list, digits_list = [], []
    indices_list, positions_list, boxes_list, labels_list = [], [], [], []
    for rec in tfrecord.read_records(filename):
        ex = tfrecord.parse_example(rec)
        n = int(ex["digits"][0])
        images_list.append(np.frombuffer(ex["image"][0], np.float32))
        digits_list.append(n)
        i32 = lambda k: np.frombuffer(ex[k][0], np.int32) if k in ex and ex[k] else np.zeros(0, np.int32)
        indices_list.append(i32("indices")[:n])
        positions_list.append(i32("positions")[:n * 2])
        boxes_list.append(i32("boxes")[:n * 2])
        labels_list.append(i32("labels")[:n])
    images_list, digits_list = np.array(images_list), np.array(digits_list)
    if shift_zero_digits_images:
        images_list, digits_list = _shift_zero(images_list, digits_list)
    return images_list, digits_list, indices_list, positions_list, boxes_list, labels_list


def shift_zero_digits_images(images, digits):
    """read_test_data(..., shift_zero_digits_images=True) :284-294: one empty image first,
    then all non-empty ones, then the remaining empty ones."""
    order = shift_zero_digits_order(digits)
    return images[order], digits[order]


def shift_zero_digits_order(digits):
    """the permutation shift_zero_digits_images applies, as an index array (the identity where no image is empty): whatever
    belongs to the images (ground-truth boxes) follows them by a[order]"""
    empty = [i for i in range(len(digits)) if digits[i] == 0]
    non_empty = [i for i in range(len(digits)) if digits[i] > 0]
    if not empty:
        return np.arange(len(digits))
    return np.asarray([empty[0]] + non_empty + empty[1:], np.int64)


_shift_zero = shift_zero_digits_images        # read_test_data's flag shadows the function name


if __name__ == "__main__":
    parser = argparse.ArgumentParser()                                  # flag surface of multi_mnist.py:312-329
    parser.add_argument("--max-digits", type=int, choices=list(range(7)), default=2)
    parser.add_argument("--max-in-common", type=int, choices=list(range(7)), default=2)
    parser.add_argument("--images-per-digit", type=int, default=20000)
    parser.add_argument("--test-set-size", type=int, default=1000)
    parser.add_argument("--digit-gap", type=int, default=0)
    parser.add_argument("--canvas-margin", type=int, default=0)
    parser.add_argument("--bg-path", default="")
    parser.add_argument("--bg-max-intensity", type=float, default=1.0)
    parser.add_argument("--min-width-scale", type=float, default=1.0)
    parser.add_argument("--max-width-scale", type=float, default=1.0)
    parser.add_argument("--min-height-scale", type=float, default=1.0)
    parser.add_argument("--max-height-scale", type=float, default=1.0)
    parser.add_argument("--min-rotation-angle", type=float, default=0.0)
    parser.add_argument("--max-rotation-angle", type=float, default=0.0)
    parser.add_argument("--use-bounding-box-overlap", action="store_true")
    parser.add_argument("--canvas-size", type=int, default=CANVAS_SIZE)
    parser.add_argument("--tfrecords", action="store_true",
                        help="also write the reference's files: <n>.tfrecords per stratum, common.tfrecords, test.tfrecords")
    parser.add_argument("--device", type=int, default=0, metavar="N",
                        help="compose N canvases on the GPU instead (DeviceSceneSource: 0 .. --max-digits digits each, drawn "
                             "uniformly) and write them with their metadata to common.npz / test.npz")
    parser.add_argument("--seed", type=int, default=0, help="--device: the seed of the scene source")
    parser.add_argument("--glyph-style", default="standin", choices=["standin", "mnist-like"],
                        help="--device: mnist-like draws the digits from a DeviceHandwritingBank (the 8x8 digits up-sampled to "
                             "40 pixels and distorted on the device into a 20-pixel box centred in a 28-pixel frame)")
    args = parser.parse_args()
    jitter = dict(min_w=args.min_width_scale, max_w=args.max_width_scale, min_h=args.min_height_scale,
                  max_h=args.max_height_scale, min_ang=args.min_rotation_angle, max_ang=args.max_rotation_angle)
    if args.glyph_style != "standin" and not args.device:
        parser.error("--glyph-style %s is made on the device: give --device N" % args.glyph_style)
    if args.glyph_style == "mnist-like" and jitter != JITTER_NEUTRAL:
        parser.error("--glyph-style mnist-like distorts the glyphs itself: leave the scale / rotation flags neutral")
    os.makedirs(MULTI_MNIST_FOLDER, exist_ok=True)
    bg = read_image(args.bg_path, args.bg_max_intensity) if args.bg_path else None
    if args.device:
        ds, source = compose_on_device(args.device, max_digits=args.max_digits, canvas_dim=args.canvas_size, bg=bg,
                                       gap=args.digit_gap, margin=args.canvas_margin, seed=args.seed,
                                       use_pixel_overlap=not args.use_bounding_box_overlap,
                                       glyph_style=args.glyph_style, **jitter)
        T = min(args.test_set_size, args.device)
        np.savez(MULTI_MNIST_FOLDER + "common.npz", **{k: v[T:] for k, v in ds.items()})
        np.savez(MULTI_MNIST_FOLDER + "test.npz", **{k: v[:T] for k, v in ds.items()})
        print("glyph source: %s; composed on the device: wrote %d train / %d test images, %d given up" % (
            source, args.device - T, T, int((ds["status"] < 0).sum())))
        raise SystemExit(0)
    strata, rng, source = generate_strata(
        args.max_digits, args.images_per_digit, bg=bg, canvas_dim=args.canvas_size, verbose=True,
        min_w=args.min_width_scale, max_w=args.max_width_scale, min_h=args.min_height_scale, max_h=args.max_height_scale,
        min_ang=args.min_rotation_angle, max_ang=args.max_rotation_angle, gap=args.digit_gap,
        margin=args.canvas_margin, use_pixel_overlap=not args.use_bounding_box_overlap)
    keys = ("images", "indices", "positions", "boxes", "labels", "digits")
    common = {k: [] for k in keys}
    for nd_, st in enumerate(strata):                                   # :347-413
        if args.tfrecords:
            write_to_records(MULTI_MNIST_FOLDER + str(nd_), *[st[k] for k in keys], side=args.canvas_size)
        if nd_ <= args.max_in_common:
            for k in keys:
                common[k].extend(st[k])
    perm = rng.permutation(len(common["images"]))                       # shuffle_lists :215-225
    common = {k: [common[k][i] for i in perm] for k in keys}
    T = args.test_set_size
    if args.tfrecords:
        write_to_records(MULTI_MNIST_FOLDER + "common", *[common[k][T:] for k in keys], side=args.canvas_size)
        write_to_records(MULTI_MNIST_FOLDER + "test", *[common[k][:T] for k in keys], side=args.canvas_size)
    np.savez(MULTI_MNIST_FOLDER + "common.npz", images=np.stack(common["images"][T:]).astype(np.float32),
             digits=np.asarray(common["digits"][T:], np.int32))
    np.savez(MULTI_MNIST_FOLDER + "test.npz", images=np.stack(common["images"][:T]).astype(np.float32),
             digits=np.asarray(common["digits"][:T], np.int32),
             # the test set's ground truth, [n, 2 * max_digits] as --device writes it (training.py --localization reads it)
             positions=padded_truth(common["positions"][:T], common["digits"][:T], args.max_digits).reshape(-1, 2 * max(args.max_digits, 1)),
             boxes=padded_truth(common["boxes"][:T], common["digits"][:T], args.max_digits).reshape(-1, 2 * max(args.max_digits, 1)),
             labels=padded_labels(common["labels"][:T], common["digits"][:T], args.max_digits))   # (training.py --latent-probe)
    print("glyph source: %s; wrote %d train / %d test images" % (source, len(perm) - T, T))
