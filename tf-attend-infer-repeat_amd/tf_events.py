"""TensorBoard event files without TensorFlow -- what tf.summary.FileWriter writes for the reference (training.py:140-218):
TFRecord-framed Event protos, hand-encoded on tfrecord.py's wire helpers.

    Event           wall_time = 1 double, step = 2 int64, file_version = 3 string, summary = 5 Summary
    Summary         value = 1 repeated Value
    Value           tag = 1 string, simple_value = 2 float, image = 4 Image, histo = 5 HistogramProto
    HistogramProto  min, max, num, sum, sum_squares = 1..5 double, bucket_limit = 6, bucket = 7 (packed double)
    Image           height = 1, width = 2, colorspace = 3 (varint), encoded_image_string = 4 bytes

Scalar fields that hold their default (0, 0.0, "") are left out, as proto3 serialises them.  The graph-def record, audio and
tensor summaries are not written."""
import os
import socket
import struct
import time
import zlib

import numpy as np

from tfrecord import _fields, _ld, _varint, crc32c, masked, read_records

FILE_VERSION = "brain.Event:2"


# ----------------------------------------------------------------------------- encoding
def _double(field, v):
    b = struct.pack("<d", float(v))
    return b"" if b == b"\0" * 8 else _varint((field << 3) | 1) + b


def _int(field, v):
    return _varint((field << 3) | 0) + _varint(int(v)) if int(v) else b""


def _packed_doubles(field, values):
    values = np.asarray(values, dtype="<f8")
    return _ld(field, values.tobytes()) if values.size else b""


def compress_buckets(limits, counts):
    """TF's Histogram::EncodeToProto: walk the buckets; a run of buckets with count <= 0 becomes ONE entry carrying the limit
    and the count of the run's last bucket, every non-empty bucket is its own entry.  -> (limits, counts), float64."""
    limits, counts = np.asarray(limits, np.float64), np.asarray(counts, np.float64)
    if limits.shape != counts.shape or limits.ndim != 1:
        raise ValueError("one limit per bucket")
    n = counts.size
    if n == 0:
        return limits, counts
    # bucket i is emitted unless it is empty AND followed by another empty bucket (then it is inside a run)
    empty = counts <= 0
    keep = ~(empty & np.append(empty[1:], False))
    return limits[keep], counts[keep]


def encode_histogram(h, limits):
    """h: min, max, num, sum, sum_squares, counts (dense, one per limit) as attributes or keys"""
    get = (lambda k: h[k]) if isinstance(h, dict) else (lambda k: getattr(h, k))
    lim, cnt = compress_buckets(limits, get("counts"))
    return b"".join(_double(i + 1, get(k)) for i, k in enumerate(("min", "max", "num", "sum", "sum_squares"))) + \
        _packed_doubles(6, lim) + _packed_doubles(7, cnt)


def encode_png(pixels, level=6):
    """uint8 [H, W, 3] (or [H, W, 1] / [H, W]: greyscale) -> PNG bytes (8 bits per channel, no interlace, filter 0)"""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    if c not in (1, 3):
        raise ValueError("1 or 3 channels")

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * c)], axis=1)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + chunk(b"IEND", b"")


def image_to_uint8(image):
    """tf.summary.image's conversion of ONE float image whose minimum is >= 0 (the reference's picture: values in [0, 1], the
    white stripe is 1.0): uint8(v * scale), truncating, scale = 255 / max in fp32 (0 for an all-zero image) -- v * 255 when
    the maximum is 1.  An image with negative values takes TF's other branch (an offset of 127): refused, not guessed."""
    v = np.asarray(image, dtype=np.float32)
    if not np.isfinite(v).all():
        raise ValueError("image summary of non-finite values")
    if v.size and v.min() < 0:
        raise ValueError("image summary of negative values is not implemented (TF rescales around 127)")
    mx = np.float32(v.max()) if v.size else np.float32(0)
    scale = np.float32(0) if mx < np.float32(1e-6) else np.float32(255) / mx
    return (v * scale).astype(np.uint8)


def encode_image(pixels, png_level=6):
    a = np.asarray(pixels)
    if a.ndim == 2:
        a = a[:, :, None]
    return _int(1, a.shape[0]) + _int(2, a.shape[1]) + _int(3, a.shape[2]) + _ld(4, encode_png(a, png_level))


def _value(tag, payload):
    return _ld(1, _ld(1, tag.encode()) + payload)


def encode_event(wall_time, step=0, values=b"", file_version=None):
    body = _double(1, wall_time) + _int(2, step)
    if file_version is not None:
        body += _ld(3, file_version.encode())
    if values:
        body += _ld(5, values)
    return body


class EventFileWriter:
    """tf.summary.FileWriter's file: <logdir>/events.out.tfevents.<seconds>.<hostname>, its first record
    Event{wall_time, file_version: "brain.Event:2"}, then one Event{wall_time, step, summary} per add_* call."""

    def __init__(self, logdir, filename_suffix=""):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s%s" % (int(now), socket.gethostname(), filename_suffix))
        self._file = open(self.path, "wb")
        self._limits = None
        self._write(encode_event(now, file_version=FILE_VERSION))
        self._file.flush()

    def _write(self, record):
        head = struct.pack("<Q", len(record))
        self._file.write(head + struct.pack("<I", int(masked(crc32c(head)))) + record +
                         struct.pack("<I", int(masked(crc32c(record)))))

    def _add(self, step, values, wall_time=None):
        self._write(encode_event(time.time() if wall_time is None else wall_time, step, values))

    def add_scalars(self, step, scalars, wall_time=None):
        """scalars: {tag: float} or (tag, float) pairs -- one Summary with a simple_value per tag (NaN is written as NaN)"""
        items = scalars.items() if hasattr(scalars, "items") else scalars
        # (simple_value is written even when 0.0 would be elided: a Value without a payload reads as "no value" in TensorBoard)
        self._add(step, b"".join(_value(t, _varint((2 << 3) | 5) + struct.pack("<f", float(v))) for t, v in items), wall_time)

    def add_histograms(self, step, histograms, limits=None, wall_time=None):
        """histograms: {tag: h} with h.min, .max, .num, .sum, .sum_squares and the DENSE .counts over `limits` (TF 1.3's
        bucket limits, air.summaries.histogram_limits(), when None)"""
        if limits is None:
            if self._limits is None:
                from air.summaries import histogram_limits
                self._limits = histogram_limits()
            limits = self._limits
        items = histograms.items() if hasattr(histograms, "items") else histograms
        self._add(step, b"".join(_value(t, _ld(5, encode_histogram(h, limits))) for t, h in items), wall_time)

    def add_images(self, step, tag, images, max_outputs=3, wall_time=None, png_level=6):
        """tf.summary.image(tag, images, max_outputs): float [N, H, W, C] (C = 1 or 3), the first max_outputs of them, each
        normalised on its own (image_to_uint8) and PNG-encoded; tags <tag>/image/<i>, or <tag>/image when max_outputs is 1"""
        images = np.asarray(images)
        if images.ndim != 4:
            raise ValueError("images must be [N, H, W, C]")
        n = min(int(max_outputs), images.shape[0])
        vals = b""
        for i in range(n):
            t = "%s/image" % tag if max_outputs == 1 else "%s/image/%d" % (tag, i)
            vals += _value(t, _ld(4, encode_image(image_to_uint8(images[i]), png_level)))
        self._add(step, vals, wall_time)

    def add_summary(self, step, items, limits=None, wall_time=None):
        """a mixed Summary, (tag, float | histogram) pairs in order (the reference's gradient group)"""
        if limits is None:
            if self._limits is None:
                from air.summaries import histogram_limits
                self._limits = histogram_limits()
            limits = self._limits
        items = items.items() if hasattr(items, "items") else items
        vals = b""
        for t, v in items:
            if isinstance(v, (int, float, np.floating)):
                vals += _value(t, _varint((2 << 3) | 5) + struct.pack("<f", float(v)))
            else:
                vals += _value(t, _ld(5, encode_histogram(v, limits)))
        self._add(step, vals, wall_time)

    def flush(self):
        self._file.flush()

    def close(self):
        if not self._file.closed:
            self._file.close()


# ----------------------------------------------------------------------------- decoding
def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def _doubles(w, v):
    return list(struct.unpack("<%dd" % (len(v) // 8), v)) if w == 2 else [struct.unpack("<d", v)[0]]


def decode_event(b):
    ev = {"wall_time": 0.0, "step": 0}
    for f, w, v in _fields(b):
        if f == 1:
            ev["wall_time"] = struct.unpack("<d", v)[0]
        elif f == 2:
            ev["step"] = _signed(v)
        elif f == 3:
            ev["file_version"] = bytes(v).decode()
        elif f == 5:
            ev["summary"] = [_decode_value(val) for f2, _, val in _fields(v) if f2 == 1]
    return ev


def _decode_value(b):
    val = {"tag": ""}
    for f, w, v in _fields(b):
        if f == 1:
            val["tag"] = bytes(v).decode()
        elif f == 2:
            val["simple_value"] = struct.unpack("<f", v)[0]
        elif f == 4:
            img = {"height": 0, "width": 0, "colorspace": 0, "encoded_image_string": b""}
            for f2, _, x in _fields(v):
                if f2 in (1, 2, 3):
                    img[("height", "width", "colorspace")[f2 - 1]] = x
                elif f2 == 4:
                    img["encoded_image_string"] = bytes(x)
            val["image"] = img
        elif f == 5:
            h = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
            for f2, w2, x in _fields(v):
                if 1 <= f2 <= 5:
                    h[("min", "max", "num", "sum", "sum_squares")[f2 - 1]] = struct.unpack("<d", x)[0]
                elif f2 == 6:
                    h["bucket_limit"] += _doubles(w2, x)
                elif f2 == 7:
                    h["bucket"] += _doubles(w2, x)
            val["histo"] = h
    return val


def read_events(path, verify=True):
    """-> the Events of the file as dicts: wall_time, step, file_version (first record) or summary = [Value dicts], each with
    tag and one of simple_value / histo / image.  verify: check the CRC-32C of every record."""
    return [decode_event(r) for r in read_records(path, verify)]
