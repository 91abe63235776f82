"""Binary Concrete (Gumbel-Softmax) ops -- mirror of the reference's air/concrete.py:4-43.

``concrete_binary_sample``, ``concrete_binary_pre_sigmoid_sample`` and ``concrete_binary_kl_mc_sample`` keep the
reference's names, positional arguments and return values.  Tensors are float32 device tensors of any shape (the result
has the input's shape; a non-contiguous input is made contiguous); the ops run as hand-written HIP kernels
(air_concrete_* of include/air_hip.h), there is no CPU fallback.  The pre-sigmoid sample and the KL are the device code
of the model's attend kernel, so they reproduce its ``att`` record bit for bit.

Noise: the reference draws its uniforms inside the op (tf.random_uniform, unseeded).  Here ``u=`` takes the caller's
uniforms; with ``u=None`` they are drawn on the device by air_philox_fill under the key (module seed, call counter):
``manual_seed(s)`` sets the seed and rewinds the counter, every drawing call advances it.

Scalar arguments (the temperatures, ``prior_log_odds``) may be a Python float (passed by value), a 0-dim / one-element
device tensor (READ ON THE DEVICE when the kernel runs -- no ``.item()``, no synchronisation; e.g. the view
``model.dyn[H.DYN_TEMPERATURE]`` that a schedule rewrites every step) or a tensor of the full shape.  ``eps`` is a float.

Gradients (torch.autograd, hand-written backward kernels): the samples to ``log_odds``; the KL to ``y``,
``posterior_log_odds`` and a full-shape ``prior_log_odds``.  Temperatures get none (the reference feeds constants or
global_step schedules there): one that requires a gradient is a ValueError.  Everything is enqueued on the current
stream and nothing synchronises or reads a device value on the host.

Stream capture is NOT supported yet: a torch.cuda.graph capture of a forward + backward through these ops and air.vae ended
in a segmentation fault inside the runtime's end of capture on the MI355X, so the ops refuse to run
while the current stream is capturing."""
import ctypes as C

import torch

from . import _hip as H

_SALT = 0x434F4E43        # keeps this module's stream apart from others keyed by the same user seed
_state = {"seed": 0, "calls": 0}


def manual_seed(seed):
    """Seed of the uniforms drawn when ``u=None``; rewinds the call counter."""
    _state["seed"], _state["calls"] = int(seed), 0


def _device_f32(t, what, op):
    H.require_device(t, what, op, capture_too=True)
    return t.detach().contiguous().float()


def _scalar(v, like, what, op):
    """(air_scalar_t, the tensor it points into or None) of a float / one-element tensor / full-shape tensor"""
    if not torch.is_tensor(v):
        return H.Scalar(None, float(v), 0), None
    if not v.is_cuda:
        raise H.AirHipError("%s: %s must be a float or a device tensor (no CPU fallback)" % (op, what))
    t = v.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if tuple(t.shape) == tuple(like.shape):                  # (the full shape, also when that is one element)
        t = t.contiguous()
        return H.Scalar(t.data_ptr(), 0.0, 1), t
    if t.numel() == 1:
        return H.Scalar(t.data_ptr(), 0.0, 0), t
    raise ValueError("%s: %s has shape %r; a scalar, one element or the full shape %r is needed"
                     % (op, what, tuple(t.shape), tuple(like.shape)))


def _no_grad_scalar(v, what, op):
    if torch.is_tensor(v) and v.requires_grad:
        raise ValueError("%s: %s requires a gradient, which this op does not compute (the reference feeds it constants "
                         "or global_step schedules)" % (op, what))


def _uniforms(like, u, op):
    if u is not None:
        uu = _device_f32(u, "u", op)
        if uu.numel() != like.numel():
            raise ValueError("%s: u has %d elements, log_odds %d" % (op, uu.numel(), like.numel()))
        return uu
    uu = torch.empty_like(like)
    H.launch("air_philox_fill", like.device, None, 0, H.ptr(uu), uu.numel(), C.c_uint64(_state["seed"] ^ _SALT),
             C.c_uint64(_state["calls"]))
    _state["calls"] += 1
    return uu


# ---- the samples ----------------------------------------------------------------------------------------------------
def _sample_fwd(lo, u, T, eps, hard):
    y, s = torch.empty_like(lo), torch.empty_like(lo)
    H.launch("air_concrete_sample_fwd", lo.device, H.ptr(lo), H.ptr(u), C.byref(T[0]), eps, 1 if hard else 0, H.ptr(y), H.ptr(s),
             lo.numel())
    return y, s


def _presigmoid_fwd(lo, u, T, eps):
    y = torch.empty_like(lo)
    H.launch("air_concrete_presigmoid_fwd", lo.device, H.ptr(lo), H.ptr(u), C.byref(T[0]), eps, H.ptr(y), lo.numel())
    return y


class _SampleFn(torch.autograd.Function):
    """(The scalar descriptors travel as plain attributes of ctx: a device scalar is a view the caller rewrites in place --
    saved as an autograd tensor that would be an error at backward -- and it is read at backward as it then is.)"""
    @staticmethod
    def forward(ctx, log_odds, lo, u, T, eps, hard):
        y, s = _sample_fwd(lo, u, T, eps, hard)
        ctx.set_materialize_grads(False)
        ctx.y, ctx.T = y, T
        return y.view(log_odds.shape), s.view(log_odds.shape)

    @staticmethod
    def backward(ctx, d_y, d_s):
        if d_y is None and d_s is None:
            return None, None, None, None, None, None
        y, T = ctx.y, ctx.T
        gy = d_y.contiguous().float() if d_y is not None else None
        gs = d_s.contiguous().float() if d_s is not None else None
        d_lo = torch.empty_like(y)
        H.launch("air_concrete_sample_bwd", y.device, H.ptr(y), C.byref(T[0]), H.ptr(gy), H.ptr(gs), H.ptr(d_lo), y.numel())
        return d_lo, None, None, None, None, None


class _PresigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_odds, lo, u, T, eps):
        ctx.T = T
        return _presigmoid_fwd(lo, u, T, eps).view(log_odds.shape)

    @staticmethod
    def backward(ctx, d_y):
        g = d_y.contiguous().float()
        d_lo = torch.empty_like(g)
        H.launch("air_concrete_presigmoid_bwd", g.device, H.ptr(g), C.byref(ctx.T[0]), H.ptr(d_lo), g.numel())
        return d_lo, None, None, None, None


def concrete_binary_sample(log_odds, temperature, hard=False, eps=10e-10, *, u=None):
    """concrete.py:4-17: (y, sig_y) with y = log_odds + noise, sig_y = sigmoid(y / temperature); hard=True rounds the value
    (half to even, tf.round) and keeps the gradient of the soft one."""
    op = "concrete_binary_sample"
    lo = _device_f32(log_odds, "log_odds", op)
    _no_grad_scalar(temperature, "temperature", op)
    T = _scalar(temperature, lo, "temperature", op)
    uu = _uniforms(lo, u, op)
    if torch.is_grad_enabled() and log_odds.requires_grad:
        return _SampleFn.apply(log_odds, lo, uu, T, float(eps), bool(hard))
    return _sample_fwd(lo, uu, T, float(eps), bool(hard))


def concrete_binary_pre_sigmoid_sample(log_odds, temperature, eps=10e-10, *, u=None):
    """concrete.py:20-27: y = (log_odds + noise) / temperature."""
    op = "concrete_binary_pre_sigmoid_sample"
    lo = _device_f32(log_odds, "log_odds", op)
    _no_grad_scalar(temperature, "temperature", op)
    T = _scalar(temperature, lo, "temperature", op)
    uu = _uniforms(lo, u, op)
    if torch.is_grad_enabled() and log_odds.requires_grad:
        return _PresigmoidFn.apply(log_odds, lo, uu, T, float(eps))
    return _presigmoid_fwd(lo, uu, T, float(eps))


# ---- the one-sample KL ----------------------------------------------------------------------------------------------
def _kl_fwd(y, plo, pT, qlo, qT, eps):
    kl = torch.empty_like(y)
    H.launch("air_concrete_kl_fwd", y.device, H.ptr(y), C.byref(plo[0]), C.byref(pT[0]), H.ptr(qlo), C.byref(qT[0]), eps, H.ptr(kl),
             y.numel())
    return kl


class _KlFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_in, plo_in, qlo_in, y, plo, pT, qlo, qT, eps):
        ctx.args = (y, plo, pT, qlo, qT, eps)
        ctx.shapes = (y_in.shape, plo_in.shape if torch.is_tensor(plo_in) else None, qlo_in.shape)
        return _kl_fwd(y, plo, pT, qlo, qT, eps).view(y_in.shape)

    @staticmethod
    def backward(ctx, d_kl):
        y, plo, pT, qlo, qT, eps = ctx.args
        need_y, need_p, need_q = ctx.needs_input_grad[:3]
        g = d_kl.contiguous().float()
        d_y = torch.empty_like(y) if need_y else None
        d_p = torch.empty_like(y) if need_p else None
        d_q = torch.empty_like(y) if need_q else None
        H.launch("air_concrete_kl_bwd", y.device, H.ptr(g), H.ptr(y), C.byref(plo[0]), C.byref(pT[0]), H.ptr(qlo), C.byref(qT[0]), eps,
                 H.ptr(d_y), H.ptr(d_q), H.ptr(d_p), y.numel())
        sy, sp, sq = ctx.shapes
        return (d_y.view(sy) if need_y else None, d_p.view(sp) if need_p else None, d_q.view(sq) if need_q else None,
                None, None, None, None, None, None)


def concrete_binary_kl_mc_sample(y, prior_log_odds, prior_temperature, posterior_log_odds, posterior_temperature, eps=10e-10):
    """concrete.py:30-43: log q(y) - log p(y) of the pre-sigmoid sample y under the posterior and the prior Concrete."""
    op = "concrete_binary_kl_mc_sample"
    yc = _device_f32(y, "y", op)
    _no_grad_scalar(prior_temperature, "prior_temperature", op)
    _no_grad_scalar(posterior_temperature, "posterior_temperature", op)
    plo = _scalar(prior_log_odds, yc, "prior_log_odds", op)
    pT = _scalar(prior_temperature, yc, "prior_temperature", op)
    qT = _scalar(posterior_temperature, yc, "posterior_temperature", op)
    qlo = _device_f32(posterior_log_odds, "posterior_log_odds", op)
    if tuple(qlo.shape) != tuple(yc.shape):
        raise ValueError("%s: posterior_log_odds has shape %r, y %r" % (op, tuple(qlo.shape), tuple(yc.shape)))
    p_grad = torch.is_tensor(prior_log_odds) and prior_log_odds.requires_grad
    if p_grad and plo[0].stride != 1:
        raise ValueError("%s: a prior_log_odds that requires a gradient must have the full shape %r" % (op, tuple(yc.shape)))
    if torch.is_grad_enabled() and (y.requires_grad or posterior_log_odds.requires_grad or p_grad):
        return _KlFn.apply(y, prior_log_odds, posterior_log_odds, yc, plo, pT, qlo, qT, float(eps))
    return _kl_fwd(yc, plo, pT, qlo, qT, float(eps))
