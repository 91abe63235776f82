"""The reference's TensorBoard summaries, host side: their tags, and the decoding of what air_histograms leaves in a buffer.

Pure host code (no GPU, no model instance).  The reference builds four merged groups (training.py:144-149):
  numeric    88 scalars of the test model             air_model.py:160-209, 613-625
  variables  36 histograms of the trainable variables :642-649
  image      1 image summary ("reconstruction")       :627-640
  gradients  216 summaries of the train model: histogram, norm and mean of every gradient, original then applied, :657-687
A tf.summary node is named after its tag inside the model's name scope, and that name is what TensorBoard shows: the train
model (built first) owns the name scope "<scope>", the variable-sharing test model "<scope>_1"; a variable's name
"<scope>/rnn/<name>:0" becomes "<scope>/rnn/<name>_0"."""
from collections import OrderedDict, namedtuple

import numpy as np

from ._layers import VaeLayers

SummaryTags = namedtuple("SummaryTags", "numeric variables image gradients")
Histogram = namedtuple("Histogram", "min max num sum sum_squares counts")

_HEADS = ("scale/mean", "scale/log_variance", "shift/mean", "shift/log_variance")


def variable_order(n_rec=2, n_gen=2):
    """The TF names (relative to "<scope>/rnn/", the keys of VariableStore.variables) of the trainable variables in the
    reference's creation order -- tf.trainable_variables(): the LSTM cell, the scale and shift heads, the VAE, and z_pres
    last (air_model.py:286-376: z_pres is computed after the glimpse has been encoded)."""
    names = ["rnn/kernel", "rnn/bias"]
    for head in _HEADS:
        names += ["%s/%s/%s" % (head, layer, kind) for layer in ("hidden", "output") for kind in ("weights", "biases")]
    names += VaeLayers.tf_names_of(n_rec, n_gen)
    names += ["z_pres/log_odds/%s/%s" % (layer, kind) for layer in ("hidden", "output") for kind in ("weights", "biases")]
    return names


def numeric_names(max_steps, max_digits):
    """the reference's 4 + 6 * max_steps quantities x (max_digits + 2) digit-count groups, in its order, without a scope"""
    names = []

    def by_digit(name):
        names.extend("%s_%d_dig" % (name, i) for i in range(max_digits + 1))
        names.append(name + "_all_dig")
    for n in ("steps", "rec_loss", "digit_acc", "total_loss"):
        by_digit(n)
    for n in ("scale", "z_pres_prob", "z_pres_kl", "scale_kl", "shift_kl", "vae_kl"):
        for i in range(max_steps):
            by_digit("%s_%d_step" % (n, i + 1))
    return names


def summary_tags(max_steps=3, max_digits=2, vae_recognition_units=(512, 256), vae_generative_units=(256, 512), scope="air",
                 test_scope=None):
    """The four tag lists of the reference, in its order and under its name scopes: numeric, variables and image are fetched
    from the test model (name scope `test_scope`, "<scope>_1" by default), gradients from the train model (`scope`)."""
    test_scope = scope + "_1" if test_scope is None else test_scope
    variables = ["%s/rnn/%s_0" % (scope, n) for n in variable_order(len(vae_recognition_units), len(vae_generative_units))]
    numeric = ["%s/summaries/%s" % (test_scope, n) for n in numeric_names(max_steps, max_digits)]
    var_tags = ["%s/summaries/%s" % (test_scope, v) for v in variables]
    image = ["%s/summaries/reconstruction" % test_scope]
    grads = []
    for which in ("original", "applied"):
        for v in variables:
            t = "%s/training/%s_grad_%s" % (scope, v, which)
            grads += [t, t + "_norm", t + "_avg"]
    return SummaryTags(numeric, var_tags, image, grads)


def view_2d(t):
    """(rows, cols, ld) of a 1-D or 2-D tensor view as it lies in memory (a transposed view by the rows of its base)"""
    if t.dim() == 1:
        if t.numel() > 1 and t.stride(0) != 1:
            raise ValueError("a strided vector is not a row")
        return 1, t.numel(), t.numel()
    if t.dim() != 2:
        raise ValueError("a histogram view is 1-D or 2-D")
    r, c = t.shape
    sr, sc = t.stride()
    if c == 1 or sc == 1:                                     # row-major (a single column: one element per row)
        if c == 1 and r > 1 and sr == 1:
            return 1, r, r                                    # a contiguous column vector is a row
        return r, c, (max(sr, c) if r > 1 else c)
    if r == 1 or sr == 1:                                     # transposed: the rows of the base are its columns
        return c, r, (max(sc, r) if c > 1 else r)
    raise ValueError("neither dimension of the view is contiguous")


_LIMITS = None


def histogram_limits():
    """the bucket limits of TF 1.3's histogram (float64, ascending), from the library's host function"""
    global _LIMITS
    if _LIMITS is None:
        import ctypes as C
        from . import _hip as H
        n = H.lib().air_histogram_num_buckets()
        buf = (C.c_double * n)()
        H.check(H.lib().air_histogram_limits(buf), "air_histogram_limits")
        _LIMITS = np.frombuffer(buf, dtype=np.float64).copy()
    return _LIMITS


def decode_histograms(buffer, tags):
    """{tag: Histogram} from the bytes air_histograms wrote for len(tags) descriptors (a uint8 tensor or array fetched to the
    host).  AirHipError naming the tag when a histogram met a non-finite value -- where TensorFlow fails the summary op."""
    from . import _hip as H
    raw = np.ascontiguousarray(buffer.numpy() if hasattr(buffer, "numpy") else buffer).view(np.uint8).reshape(-1)
    rec, nb = int(H.lib().air_histogram_record_bytes()), int(H.lib().air_histogram_num_buckets())
    if raw.size != rec * len(tags):
        raise ValueError("%d bytes for %d histograms of %d bytes" % (raw.size, len(tags), rec))
    out = OrderedDict()
    for i, tag in enumerate(tags):
        r = raw[i * rec:(i + 1) * rec]
        mn, mx, num, s, sq, bad = (float(v) for v in r[:48].view(np.float64))
        if bad != 0:
            raise H.AirHipError("histogram summary %s: %d non-finite values" % (tag, int(bad)))
        out[tag] = Histogram(mn, mx, num, s, sq, r[48:48 + 4 * nb].view(np.uint32).copy())
    return out


def gradient_summaries(histograms):
    """The reference's gradient group from the decoded histograms of AIRModel.grad_summaries(): every histogram followed by
    its two derived scalars, tag -> Histogram | float in the reference's order:
    <tag>_norm = sqrt(sum_squares) (tf.norm), <tag>_avg = sum / num (tf.reduce_mean)."""
    out = OrderedDict()
    for tag, h in histograms.items():
        out[tag] = h
        out[tag + "_norm"] = float(np.sqrt(h.sum_squares))
        out[tag + "_avg"] = h.sum / h.num
    return out
