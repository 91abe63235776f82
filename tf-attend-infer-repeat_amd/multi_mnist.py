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

The device classes -- that default path, the scale and rotation jitter (:113-135) and MNIST-geometry digits as device work,
and the input queue -- live in air/sources.py and are re-exported here; this file joins its loaders to them (handwriting_bank,
compose_on_device) and imports neither torch nor the library until one of them is built.
"""
import argparse
import gzip
import os
import struct

import numpy as np

from air.sources import (JITTER_NEUTRAL, MNIST_LIKE, DeviceGlyphBank, DeviceHandwritingBank, DeviceSceneSource,  # noqa: F401
                         ShuffleBatchQueue, crop_boxes, gaussian_taps)

HERE =os.path.dirname(os.path.abspath(__file__))
CANVAS_SIZE = 50
IMAGE_SIZE = 28
MNIST_FOLDER = "mnist_data/"
MULTI_MNIST_FOLDER = "multi_mnist_data/"


def load_digits8x8():
    """the committed 8x8 handwritten digits: [n, 8, 8] float32 in [0, 1] + labels"""
    d = np.load(os.path.join(HERE, "data", "digits8x8.npz"))
    return d["images"].astype(np.float32) / 16.0, d["labels"].astype(np.int64)


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
    small, labels = load_digits8x8()
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
    return out.reshape(-1, IMAGE_SIZE * IMAGE_SIZE), labels, "digits8x8"


def load_base_glyphs(side=40):
    """[n, side * side] float32 in [0, 1] + labels: the committed 8x8 handwritten digits up-sampled (cubic) to side x side
    and clipped -- the base planes of DeviceHandwritingBank, which gives them stroke, ramp, size and place itself"""
    import scipy.ndimage as nd
    small, labels = load_digits8x8()
    out = np.stack([np.clip(nd.zoom(g, side / 8.0, order=3), 0.0, 1.0) for g in small]).astype(np.float32)
    return out.reshape(-1, side * side), labels


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


# ----------------------------------------------------------------------------- the loaders joined to the device sources
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
    jittered = any(v != JITTER_NEUTRAL[k] for k, v in jitter.items())
    if glyph_style == "mnist-like":
        if jittered:
            raise ValueError("glyph_style='mnist-like' distorts the glyphs itself: leave the scale / rotation bounds neutral")
        table, labels = handwriting_bank(variants, seed, dev)
        source = "digits8x8, mnist-like"
    else:
        table, labels, source = load_glyphs()
        if jittered:
            table = DeviceGlyphBank(table, variants, seed=seed, device=dev, **jitter)
    src = DeviceSceneSource(table, B, images, digits, canvas_dim=canvas_dim, max_digits=max_digits, margin=margin, gap=gap, bg=bg,
                            seed=seed, **generator_options)
    out = {k: [] for k in ("images", "digits", "indices", "positions", "boxes", "status", "labels")}
    for _ in range((num_images + B - 1) // B):
        src.fresh_batch()
        out["images"].append(images.cpu().numpy())
        out["digits"].append(digits.cpu().numpy())
        for k, v in src.meta().items():
            out[k].append(v.cpu().numpy())
        out["labels"].append((labels if src.bank is None else src.bank.labels(labels))[out["indices"][-1]])
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
