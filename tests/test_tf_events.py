"""tf_events.py: TensorBoard event files without TensorFlow.  A file with scalars, two histograms and an image reads back
equal through read_events, its framing verifies through tfrecord.read_records, it parses with protobuf message classes built
here from the field numbers of TensorFlow's event.proto / summary.proto (an independent decoder: an encoder / decoder pair
that agree on a wrong wire format fails), and the PNG decodes with PIL.  TF's run-merging rule of Histogram::EncodeToProto is
pinned on a hand-written case."""
import glob
import io
import os
import re
import socket
from collections import namedtuple

import numpy as np
import pytest

import tf_events
import tfrecord

Hist = namedtuple("Hist", "min max num sum sum_squares counts")

LIMITS = np.array([-10.0, -1.0, -0.1, 0.0, 0.1, 1.0, 10.0, 1e300])
# empty runs at both ends and in the middle | a single bucket
H_RUNS = Hist(-0.5, 5.0, 4.0, 5.25, 25.3125, np.array([0, 0, 3, 0, 0, 0, 1, 0], dtype=np.uint32))
H_ONE = Hist(0.0, 0.0, 7.0, 0.0, 0.0, np.array([7], dtype=np.uint32))
SCALARS = [("air_1/summaries/steps_0_dig", 1.5), ("air_1/summaries/empty_group", float("nan")), ("zero", 0.0), ("neg", -2.25)]
IMAGE = np.linspace(0.0, 1.0, 3 * 5 * 3, dtype=np.float32).reshape(1, 3, 5, 3)


def test_run_merging_rule():
    lim, cnt = tf_events.compress_buckets(np.arange(8.0), [0, 0, 3, 0, 0, 0, 1, 0])
    assert lim.tolist() == [1.0, 2.0, 5.0, 6.0, 7.0] and cnt.tolist() == [0.0, 3.0, 0.0, 1.0, 0.0]
    lim, cnt = tf_events.compress_buckets([5.0], [7])
    assert lim.tolist() == [5.0] and cnt.tolist() == [7.0]
    lim, cnt = tf_events.compress_buckets(np.arange(4.0), [0, 0, 0, 0])
    assert lim.tolist() == [3.0] and cnt.tolist() == [0.0]
    lim, cnt = tf_events.compress_buckets(np.arange(5.0), [2, 0, 1, 1, 0])
    assert lim.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and cnt.tolist() == [2.0, 0.0, 1.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        tf_events.compress_buckets(np.arange(3.0), [1, 2])


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    logdir = str(tmp_path_factory.mktemp("summary"))
    w = tf_events.EventFileWriter(logdir)
    w.add_scalars(0, SCALARS, wall_time=100.5)
    w.add_histograms(250, {"h/runs": H_RUNS}, limits=LIMITS, wall_time=101.0)
    w.add_histograms(250, [("h/one", H_ONE)], limits=[1e-12], wall_time=101.25)
    w.add_images(500, "air_1/summaries/reconstruction", IMAGE.repeat(2, axis=0), max_outputs=60, wall_time=102.0)
    w.add_summary(1, [("g", H_RUNS), ("g_norm", 5.03), ("g_avg", 1.3125)], limits=LIMITS, wall_time=103.0)
    w.flush()
    w.close()
    w.close()
    return logdir, w.path


def test_file_name_and_framing(written):
    logdir, path = written
    assert glob.glob(os.path.join(logdir, "*")) == [path]
    assert re.fullmatch(r"events\.out\.tfevents\.\d{10}\.%s" % re.escape(socket.gethostname()), os.path.basename(path))
    recs = tfrecord.read_records(path, verify=True)
    assert len(recs) == 6
    raw = bytearray(open(path, "rb").read())
    raw[-6] ^= 1                                                     # a flipped payload bit is caught by the record's CRC
    bad = path + ".bad"
    open(bad, "wb").write(bytes(raw))
    try:
        with pytest.raises(IOError):
            tf_events.read_events(bad, verify=True)
    finally:
        os.remove(bad)


def test_round_trip(written):
    ev = tf_events.read_events(written[1], verify=True)
    assert ev[0]["file_version"] == "brain.Event:2" and ev[0]["wall_time"] > 1e9 and "summary" not in ev[0]
    assert [(e["step"], e["wall_time"]) for e in ev[1:]] == [(0, 100.5), (250, 101.0), (250, 101.25), (500, 102.0), (1, 103.0)]
    sc = ev[1]["summary"]
    assert [v["tag"] for v in sc] == [t for t, _ in SCALARS]
    assert sc[0]["simple_value"] == 1.5 and sc[1]["simple_value"] != sc[1]["simple_value"]
    assert sc[2]["simple_value"] == 0.0 and sc[3]["simple_value"] == -2.25
    h = ev[2]["summary"][0]
    assert h["tag"] == "h/runs"
    assert h["histo"] == dict(min=-0.5, max=5.0, num=4.0, sum=5.25, sum_squares=25.3125,
                              bucket_limit=[-1.0, -0.1, 1.0, 10.0, 1e300], bucket=[0.0, 3.0, 0.0, 1.0, 0.0])
    one = ev[3]["summary"][0]
    assert one["tag"] == "h/one" and one["histo"] == dict(min=0.0, max=0.0, num=7.0, sum=0.0, sum_squares=0.0,
                                                          bucket_limit=[1e-12], bucket=[7.0])
    im = ev[4]["summary"]
    assert [v["tag"] for v in im] == ["air_1/summaries/reconstruction/image/0", "air_1/summaries/reconstruction/image/1"]
    assert all((v["image"]["height"], v["image"]["width"], v["image"]["colorspace"]) == (3, 5, 3) for v in im)
    assert im[0]["image"]["encoded_image_string"][:8] == b"\x89PNG\r\n\x1a\n"
    mixed = ev[5]["summary"]
    assert [v["tag"] for v in mixed] == ["g", "g_norm", "g_avg"] and mixed[0]["histo"] == dict(h["histo"])
    assert mixed[1]["simple_value"] == np.float32(5.03) and mixed[2]["simple_value"] == 1.3125


def test_png_decodes_to_the_truncated_bytes(written):
    Image = pytest.importorskip("PIL.Image")
    ev = tf_events.read_events(written[1])
    want = (IMAGE[0] * np.float32(255)).astype(np.uint8)             # max = 1: uint8(v * 255), truncating
    assert want.max() == 255 and want.min() == 0 and int(want[0, 0, 1]) == int(255 / 44)
    for v in ev[4]["summary"]:
        px = np.asarray(Image.open(io.BytesIO(v["image"]["encoded_image_string"])).convert("RGB"))
        assert px.dtype == np.uint8 and np.array_equal(px, want)
    grey = tf_events.encode_png(want[:, :, :1])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(grey))), want[:, :, 0])


def test_image_conversion_rules():
    assert tf_events.image_to_uint8(np.array([[0.0, 0.5, 0.999, 1.0]])).tolist() == [[0, 127, 254, 255]]
    assert tf_events.image_to_uint8(np.zeros((2, 2))).tolist() == [[0, 0], [0, 0]]
    with pytest.raises(ValueError, match="negative"):
        tf_events.image_to_uint8(np.array([[0.5, -1e-3]]))
    with pytest.raises(ValueError):
        tf_events.image_to_uint8(np.array([[0.5, np.nan]]))
    with pytest.raises(ValueError):
        tf_events.EventFileWriter.add_images(None, 0, "t", np.zeros((3, 5, 3)))


def _message_classes():
    """Event / Summary / HistogramProto / Image built from descriptor_pb2 with TensorFlow's field numbers"""
    pytest.importorskip("google.protobuf")
    from google.protobuf import descriptor_pb2, descriptor_pool
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="air_test_event.proto", package="air_test", syntax="proto3")

    def message(name, fields):
        m = fd.message_type.add(name=name)
        for fname, number, ftype, label, type_name in fields:
            f = m.field.add(name=fname, number=number, type=ftype, label=label)
            if type_name:
                f.type_name = ".air_test." + type_name
    one, rep = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    message("HistogramProto", [(n, i + 1, F.TYPE_DOUBLE, one, None) for i, n in enumerate(("min", "max", "num", "sum", "sum_squares"))] +
            [("bucket_limit", 6, F.TYPE_DOUBLE, rep, None), ("bucket", 7, F.TYPE_DOUBLE, rep, None)])
    message("Image", [("height", 1, F.TYPE_INT32, one, None), ("width", 2, F.TYPE_INT32, one, None),
                      ("colorspace", 3, F.TYPE_INT32, one, None), ("encoded_image_string", 4, F.TYPE_BYTES, one, None)])
    message("Value", [("tag", 1, F.TYPE_STRING, one, None), ("simple_value", 2, F.TYPE_FLOAT, one, None),
                      ("image", 4, F.TYPE_MESSAGE, one, "Image"), ("histo", 5, F.TYPE_MESSAGE, one, "HistogramProto")])
    message("Summary", [("value", 1, F.TYPE_MESSAGE, rep, "Value")])
    message("Event", [("wall_time", 1, F.TYPE_DOUBLE, one, None), ("step", 2, F.TYPE_INT64, one, None),
                      ("file_version", 3, F.TYPE_STRING, one, None), ("summary", 5, F.TYPE_MESSAGE, one, "Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    desc = pool.FindMessageTypeByName("air_test.Event")
    try:
        from google.protobuf import message_factory
        return message_factory.GetMessageClass(desc)
    except (ImportError, AttributeError):
        from google.protobuf import message_factory
        return message_factory.MessageFactory(pool).GetPrototype(desc)


def test_parses_with_an_independent_protobuf_decoder(written):
    Event = _message_classes()
    recs = tfrecord.read_records(written[1], verify=True)
    evs = []
    for r in recs:
        e = Event()
        e.ParseFromString(bytes(r))
        evs.append(e)
    assert evs[0].file_version == "brain.Event:2" and evs[0].step == 0 and len(evs[0].summary.value) == 0
    assert [e.step for e in evs[1:]] == [0, 250, 250, 500, 1] and evs[2].wall_time == 101.0
    sc = evs[1].summary.value
    assert [v.tag for v in sc] == [t for t, _ in SCALARS]
    assert sc[0].simple_value == 1.5 and sc[1].simple_value != sc[1].simple_value and sc[3].simple_value == -2.25
    h = evs[2].summary.value[0]
    assert h.tag == "h/runs" and (h.histo.min, h.histo.max, h.histo.num, h.histo.sum, h.histo.sum_squares) == (-0.5, 5.0, 4.0, 5.25, 25.3125)
    assert list(h.histo.bucket_limit) == [-1.0, -0.1, 1.0, 10.0, 1e300] and list(h.histo.bucket) == [0.0, 3.0, 0.0, 1.0, 0.0]
    one = evs[3].summary.value[0].histo
    assert (one.min, one.num, list(one.bucket_limit), list(one.bucket)) == (0.0, 7.0, [1e-12], [7.0])
    im = evs[4].summary.value
    assert len(im) == 2 and im[1].tag.endswith("/image/1") and (im[1].image.height, im[1].image.width, im[1].image.colorspace) == (3, 5, 3)
    assert im[1].image.encoded_image_string[:4] == b"\x89PNG"
    mixed = evs[5].summary.value
    assert mixed[0].histo.num == 4.0 and mixed[1].simple_value == np.float32(5.03) and not mixed[1].HasField("histo")
    # and the bytes are what that encoder would write itself, field order and default elision included (not the scalars:
    # TensorFlow's Value keeps its payload in a oneof, so a simple_value of 0.0 IS written, as here)
    for i in (0, 2, 3):
        assert evs[i].SerializeToString(deterministic=True) == bytes(recs[i]), i
