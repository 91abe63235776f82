"""CPU-side checks of the histogram summaries (include/air_hip.h "histogram summaries", air/summaries.py): the bucket limits
are TensorFlow 1.3's bit for bit, argument errors are answered on the host before any HIP call and alike by all three
descriptor-taking calls, and
the tag function gives the four tag lists of the reference's graph (tests/golden/summary_tags.json, written by
tests/golden/make_summary_tags.py).  (What the kernels compute: tests/test_gpu_histograms.py.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import abi_check as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def test_limits_are_tensorflows(H):
    pos, v = [], 1e-12
    while v < 1e20:                                   # core/lib/histogram/histogram.cc: InitDefaultBucketsInner
        pos.append(v)
        v *= 1.1
    assert len(pos) == 774 and pos[-1] == 9.920775621859783e+19
    pos.append(sys.float_info.max)
    want = np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)
    n = H.lib().air_histogram_num_buckets()
    assert n == len(want) == 1551
    buf = (C.c_double * n)()
    assert H.lib().air_histogram_limits(buf) == 0
    got = np.frombuffer(buf, dtype=np.float64)
    assert got.tobytes() == want.tobytes()            # bit for bit
    assert (np.diff(got) > 0).all() and np.array_equal(got, -got[::-1]) and got[n // 2] == 0.0
    assert H.lib().air_histogram_limits(None) == -1
    from air.summaries import histogram_limits
    assert histogram_limits().tobytes() == want.tobytes()
    assert H.lib().air_histogram_record_bytes() == 48 + 4 * (n + 1) and H.lib().air_histogram_record_bytes() % 8 == 0
    assert H.lib().air_histogram_chunk() % 4 == 0 and H.lib().air_histogram_chunk() >= 256


def test_descriptor_is_24_bytes(H):
    assert C.sizeof(H.HistogramDesc) == 24            # the documented size (its layout: tests/test_abi.py, with every other)


def _descs(H, n=2, **override):
    """n valid descriptors over a never-dereferenced address; `override` changes the LAST one"""
    d = [H.HistogramDesc(1 << 20, 3, 5, 8, 0) for _ in range(n)]
    for k, v in override.items():
        setattr(d[-1], k, v)
    return (H.HistogramDesc * n)(*d)


def _all_three(H, descs, count):
    """the answer of the three descriptor-taking calls (every call returns before a launch: nothing is dereferenced)"""
    lib = H.lib()
    a = H.Histograms(descs, count, 1.0, C.c_void_p(1 << 21), C.c_void_p(1 << 22), C.c_void_p(1 << 23), C.c_void_p(1 << 24),
                     1 << 40, 1 << 40)
    return lib.air_histograms_output_bytes(descs, count), lib.air_histograms_workspace_bytes(descs, count), \
        lib.air_histograms(C.byref(a), None)


def test_argument_errors_without_gpu(H):
    lib = H.lib()
    assert lib.air_histograms(None, None) == -1
    assert _all_three(H, None, 1) == (-1, -1, -1)
    assert _all_three(H, _descs(H), 0) == (-1, -1, -1)
    assert _all_three(H, _descs(H), -5) == (-1, -1, -1)
    assert _all_three(H, _descs(H, 129), 129) == (-2, -2, -2)
    for bad in (dict(base=None), dict(rows=0), dict(rows=-1), dict(cols=0), dict(ld=4), dict(scale_kind=3), dict(scale_kind=-1)):
        assert _all_three(H, _descs(H, 3, **bad), 3) == (-1, -1, -1), bad
        assert _all_three(H, _descs(H, 128, **bad), 128) == (-1, -1, -1), bad
    assert _all_three(H, _descs(H, base=(1 << 20) + 2), 2) == (-3, -3, -3)              # AIR_EALIGN: not a float address
    assert _all_three(H, _descs(H, rows=1 << 20, cols=1 << 13, ld=1 << 13), 2) == (-2, -2, -2)   # 2^33 elements: uint32 counts
    # the launch alone: null buffers, a short buffer, scale_kind 2 without its device scalars, misaligned buffers
    d = _descs(H, scale_kind=2)

    def call(**kw):
        a = H.Histograms(d, 2, 1.0, C.c_void_p(1 << 21), C.c_void_p(1 << 22), C.c_void_p(1 << 23), C.c_void_p(1 << 24),
                         1 << 40, 1 << 40)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.air_histograms(C.byref(a), None)
    for k in ("out", "workspace", "dyn", "gnorm"):
        assert call(**{k: None}) == -1, k
    assert call(out_bytes=2 * lib.air_histogram_record_bytes() - 1) == -1 and call(workspace_bytes=95) == -1
    assert call(out=C.c_void_p((1 << 23) + 4)) == -3 and call(workspace=C.c_void_p((1 << 24) + 4)) == -3


def test_sizes(H):
    lib = H.lib()
    chunk, rec = lib.air_histogram_chunk(), lib.air_histogram_record_bytes()
    for n, items in ((1, 1), (chunk - 1, 1), (chunk, 1), (chunk + 1, 2), (2 * chunk + 5, 3)):
        d = _descs(H, 1, rows=1, cols=n, ld=n)
        assert lib.air_histograms_workspace_bytes(d, 1) == items * 48 and lib.air_histograms_output_bytes(d, 1) == rec
    d = _descs(H, 128, rows=2756, cols=1024, ld=1024)
    assert lib.air_histograms_output_bytes(d, 128) == 128 * rec
    assert lib.air_histograms_workspace_bytes(d, 128) == 48 * (127 + -(-2756 * 1024 // chunk))


def test_tags_equal_the_references_graph():
    from air.summaries import numeric_names, summary_tags, variable_order
    from oracle.air_oracle import TRAINING_HP as hp
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "summary_tags.json")))
    got = summary_tags(hp["max_steps"], hp["max_digits"], hp["vae_recognition_units"], hp["vae_generative_units"], scope="air")
    assert [len(want[k]) for k in ("numeric", "variables", "image", "gradients")] == [88, 36, 1, 216]
    for k in ("numeric", "variables", "image", "gradients"):
        assert getattr(got, k) == want[k], k
    assert got.gradients[0] == "air/training/air/rnn/rnn/kernel_0_grad_original"
    assert got.gradients[-1] == "air/training/air/rnn/z_pres/log_odds/output/biases_0_grad_applied_avg"
    assert len(numeric_names(3, 2)) == 88 and len(variable_order()) == 36
    other = summary_tags(2, 1, (32,), (16, 8, 4), scope="m", test_scope="eval")
    assert len(other.numeric) == (4 + 6 * 2) * 3 and other.numeric[0] == "eval/summaries/steps_0_dig"
    assert len(other.variables) == 22 + 2 * 7 and other.variables[0] == "eval/summaries/m/rnn/rnn/kernel_0"
    assert other.image == ["eval/summaries/reconstruction"] and len(other.gradients) == 6 * len(other.variables)


def test_views_as_they_lie_in_memory():
    """VariableStore's TF-named views -> (rows, cols, ld): column slices of whid, transposed row slices of wout, the column
    halves of ml_w"""
    from air.summaries import view_2d
    whid, wout, ml = torch.zeros(256, 320), torch.zeros(7, 64), torch.zeros(256, 100)
    assert view_2d(whid[:, 64:128]) == (256, 64, 320)
    assert view_2d(wout[0:1, :64].t()) == (1, 64, 64)
    assert view_2d(wout[2:4, :48].t()) == (2, 48, 64)
    assert view_2d(ml[:, 50:]) == (256, 50, 100)
    assert view_2d(torch.zeros(8)[2:4]) == (1, 2, 2) and view_2d(torch.zeros(5, 7)) == (5, 7, 7)
    assert view_2d(torch.zeros(1, 7)) == (1, 7, 7) and view_2d(torch.zeros(1)) == (1, 1, 1)
    with pytest.raises(ValueError):
        view_2d(torch.zeros(8, 8)[::2, ::2])
    with pytest.raises(ValueError):
        view_2d(torch.zeros(2, 2, 2))


def test_decode_checks_its_input(H):
    from air.summaries import decode_histograms, gradient_summaries
    rec, nb = H.lib().air_histogram_record_bytes(), H.lib().air_histogram_num_buckets()
    raw = np.zeros(2 * rec, dtype=np.uint8)
    for h, bad in ((0, 0.0), (1, 2.0)):
        raw[h * rec:h * rec + 48].view(np.float64)[:] = [-1.5, 2.0, 3.0, 0.5, 6.25, bad]
        raw[h * rec + 48:h * rec + 48 + 4 * nb].view(np.uint32)[[10, 800]] = [1, 2]
    out = decode_histograms(raw[:rec], ["a"])
    assert out["a"].min == -1.5 and out["a"].num == 3.0 and out["a"].counts[800] == 2 and out["a"].counts.size == nb
    s = gradient_summaries(out)
    assert list(s) == ["a", "a_norm", "a_avg"] and s["a_norm"] == 2.5 and s["a_avg"] == 0.5 / 3.0
    with pytest.raises(H.AirHipError, match="b/grad.*2 non-finite"):
        decode_histograms(raw, ["a", "b/grad"])
    with pytest.raises(ValueError):
        decode_histograms(raw, ["a"])
