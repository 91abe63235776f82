"""The reference's TensorBoard summaries, host side: their tags, the two launches that compute them for a model
(air_summaries, air_histograms), and the decoding of what air_histograms leaves in a buffer.

The tags, view_2d and the decoding are pure host code (no GPU, no model instance); numeric_summaries() and histograms()
take a built AIRModel -- its public methods of those names are thin calls of them -- and import torch and the library
when they run, not when this module is imported.  The reference builds four merged groups (training.py:144-149):
  numeric    88 scalars of the test model             air_model.py:160-209, 613-625
  variables  36 histograms of the trainable variables :642-649
  image      1 image summary ("reconstruction")       :627-640
  gradients  216 summaries of the train model: histogram, norm and mean of every gradient, original then applied, :657-687
A tf.summary node is named after its tag inside the model's name scope, and that name is what TensorBoard shows: the train
model (built first) owns the name scope "<scope>", the variable-sharing test model "<scope>_1"; a variable's name
"<scope>/rnn/<name>:0" becomes "<scope>/rnn/<name>_0"."""
import ctypes as C
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


# ---- the launches, for a built AIRModel `m` (AIRModel.numeric_summaries / var_summaries / grad_summaries) ---------------
def numeric_summaries(m, out=None):
    """air_summaries on the model's stream over the records of its last pass, into `out` (allocated when None)"""
    import torch
    from . import _hip as H
    n = m.lib.air_summaries_count(m.max_steps, m.max_digits)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=m.input_images.device)
    if out.numel() != n or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 vector of %d elements" % n)
    a = H.Summaries(H.ptr(m.att), H.ptr(m.target_num_digits), H.ptr(m.run_digits), H.ptr(m._rec_loss),
                    H.ptr(m._loss_item), H.ptr(m.scalars), H.ptr(out), m.batch_size, m.max_steps, m.max_digits)
    H.check(m.lib.air_summaries(C.byref(a), m._stream()), "air_summaries")
    return out


def _histogram_plan(m, which):
    """descriptors + workspace of one of the two launches ("var" / "grad"), built once per model (the views never move)"""
    import torch
    from . import _hip as H
    if which not in m._hist_plans:
        order = variable_order(len(m.vae_recognition_units), len(m.vae_generative_units))
        views = m.store.variables if which == "var" else m.store.gradients
        kinds = (0,) if which == "var" else (1, 2)
        descs = []
        for kind in kinds:
            for name in order:
                v = views[name]
                rows, cols, ld = view_2d(v)
                descs.append(H.HistogramDesc(v.data_ptr(), rows, cols, ld, kind))
        arr = (H.HistogramDesc * len(descs))(*descs)
        nout = m.lib.air_histograms_output_bytes(arr, len(descs))
        nws = m.lib.air_histograms_workspace_bytes(arr, len(descs))
        if nout < 0 or nws < 0:
            H.check(int(min(nout, nws)), "air_histograms_workspace_bytes")
        ws = torch.empty(int(nws), dtype=torch.uint8, device=m.input_images.device)
        m._hist_plans[which] = (arr, int(nout), ws)
    return m._hist_plans[which]


def histograms(m, which, out=None):
    """air_histograms on the model's stream over the strided views of its flat variable ("var") or gradient ("grad")
    buffer, into the uint8 device vector `out` (allocated when None) that decode_histograms() reads once fetched"""
    import torch
    from . import _hip as H
    arr, nout, ws = _histogram_plan(m, which)
    if out is None:
        out = torch.empty(nout, dtype=torch.uint8, device=m.input_images.device)
    if out.numel() != nout or out.dtype != torch.uint8 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous uint8 device vector of %d bytes" % nout)
    a = H.Histograms(arr, len(arr), 1.0 / m._world(), H.ptr(m.dyn), H.ptr(m.store.gnorm), H.ptr(out), H.ptr(ws),
                     nout, ws.numel())
    H.check(m.lib.air_histograms(C.byref(a), m._stream()), "air_histograms")
    return out
