"""The CNN front-end of the reference -- the inline block air/air_model.py:510-533 as an op of its own.

Three 5x5 SAME convolutions + ReLU with a 2x2 / stride-2 max-pool after the first two, one input channel, ``filters``
output channels each, fp32, NHWC: ``[B, S*S]`` or ``[B, S, S, 1]`` images in, ``[B, (S//4)**2 * filters]`` out, flattened in
(y, x, channel) order like the reference's tf.reshape (1152 columns at the reference's 50 x 50 canvas and 8 filters).

``CNN`` is a torch.nn.Module that owns the variables tf.layers.conv2d creates under the scope ``cnn/``
(``cnn/conv{1,2,3}/kernel`` [5, 5, Cin, F], ``cnn/conv{1,2,3}/bias`` [F]; Glorot-uniform kernels with fan_in = 25 Cin and
fan_out = 25 F, zero biases, from a generator of this module); ``cnn(...)`` is the functional form.

The forward is ONE launch of air_cnn_fwd, the backward one air_cnn_bwd (a per-image launch plus the batch reduction of the
variable gradients, in ascending image order: no atomics, the same inputs give the same bits).  Both are enqueued on the
current stream; nothing synchronises and no device value is read on the host.  The gradient of the images is computed only
when the input requires one; under torch.no_grad() the tensors the backward needs (the pooled planes and their argmax
codes) are not allocated and the launch is the inference forward -- same bits.  There is no CPU fallback.

Stream capture is NOT supported, for the reason air.vae gives: the op refuses to run while the
current stream is capturing.

AIRModel(cnn=True) does not go through this module: its launch lists call air_cnn_fwd and air_cnn_bwd_sq themselves, from the
thread that captures the step, and own the six variables in the model's flat buffer under the names variable_names() gives
(DESIGN.md section 25).  CNN.load_variables(model.variables) reproduces the model's rnn_input bit for bit."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _hip as H
from ._layers import load_variables

_SALT = 0x434E4E31            # keeps this module's initial values apart from others keyed by the same user seed


def _check_sizes(canvas_size, filters):
    """the library's own answer for (S, F) -- no GPU is touched"""
    S, F = int(canvas_size), int(filters)
    rc = H.lib().air_cnn_workspace_floats(1, S, F)
    if rc == H.ELIMIT:
        raise NotImplementedError("cnn: canvas_size = %d with filters = %d is beyond what the kernels hold in LDS "
                                  "(filters <= 8; canvas_size <= 77 at 8 filters, <= 128 at 1 or 2)" % (S, F))
    if rc < 0:
        raise ValueError("cnn: canvas_size must be >= 4 and filters >= 1, got %d and %d" % (S, F))


class _CnnFn(torch.autograd.Function):
    """forward(ctx, module, images [B, S*S], k1, b1, k2, b2, k3, b3) -> out [B, S2*S2*F]"""

    @staticmethod
    def forward(ctx, mod, images, *params):
        dev = images.device
        x = images.detach().contiguous().float()
        P = [q.detach().contiguous() for q in params]
        B, S, F = int(x.shape[0]), mod.canvas_size, mod.filters
        S1, S2 = S // 2, S // 4
        out = torch.empty(B, S2 * S2 * F, dtype=torch.float32, device=dev)
        train = any(ctx.needs_input_grad[1:])       # all False under torch.no_grad(): the inference forward
        pool1 = pool2 = arg1 = arg2 = None
        if train:
            pool1 = torch.empty(B, S1, S1, F, dtype=torch.float32, device=dev)
            pool2 = torch.empty(B, S2, S2, F, dtype=torch.float32, device=dev)
            arg1 = torch.empty(B, S1, S1, F, dtype=torch.uint8, device=dev)
            arg2 = torch.empty(B, S2, S2, F, dtype=torch.uint8, device=dev)
        a = H.CnnFwd(H.ptr(x), H.ptr(P[0]), H.ptr(P[1]), H.ptr(P[2]), H.ptr(P[3]), H.ptr(P[4]), H.ptr(P[5]), H.ptr(out),
                     H.ptr(pool1), H.ptr(pool2), H.ptr(arg1), H.ptr(arg2), B, S, F)
        with torch.cuda.device(dev):                 # the launch belongs to the input's device, whichever is current
            H.launch("air_cnn_fwd", dev, C.byref(a))
        ctx.set_materialize_grads(False)
        # the input, the variables and the output through save_for_backward: an in-place change of any of them between
        # forward and backward is an error of autograd's, not a silently wrong gradient.  x and P are the same storage
        # unless a copy had to be made (a non-contiguous or non-fp32 input); the four tensors below never leave this class.
        ctx.save_for_backward(images, *params, out)
        ctx.mod, ctx.x, ctx.P = mod, x, P
        ctx.saved = (pool1, pool2, arg1, arg2)
        ctx.in_shape, ctx.in_dtype = images.shape, images.dtype
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        if d_out is None:
            return (None,) * 8
        out = ctx.saved_tensors[-1]                  # (raises if the input, a variable or the output was changed in place)
        mod, x, P = ctx.mod, ctx.x, ctx.P
        pool1, pool2, arg1, arg2 = ctx.saved
        dev = out.device
        B, S, F = int(x.shape[0]), mod.canvas_size, mod.filters
        d_out = d_out.contiguous().float()
        ws = torch.empty(int(H.lib().air_cnn_workspace_floats(B, S, F)), dtype=torch.float32, device=dev)
        grads = [torch.empty_like(q) for q in P]
        d_images = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        a = H.CnnBwd(H.ptr(d_out), H.ptr(out), H.ptr(x), H.ptr(pool1), H.ptr(pool2), H.ptr(arg1), H.ptr(arg2),
                     H.ptr(P[0]), H.ptr(P[2]), H.ptr(P[4]), H.ptr(ws), *[H.ptr(g) for g in grads], H.ptr(d_images), B, S, F)
        with torch.cuda.device(dev):
            H.launch("air_cnn_bwd", dev, C.byref(a))
        if d_images is not None:
            d_images = d_images.view(ctx.in_shape).to(ctx.in_dtype)
        return (None, d_images) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class CNN(torch.nn.Module):
    """air_model.py:510-533 as a module: conv1 -> pool1 -> conv2 -> pool2 -> conv3 on a canvas_size x canvas_size canvas."""

    def __init__(self, canvas_size=50, filters=8, device="cuda", seed=0):
        super().__init__()
        _check_sizes(canvas_size, filters)
        self.canvas_size, self.filters = int(canvas_size), int(filters)
        self.output_dim = (self.canvas_size // 4) ** 2 * self.filters
        F = self.filters
        gen = torch.Generator(device="cpu")
        gen.manual_seed((int(seed) ^ _SALT) & 0x7FFFFFFFFFFFFFFF)
        cin = 1
        for i in (1, 2, 3):
            # the tf.layers.conv2d default: glorot_uniform over fan_in = 25 Cin, fan_out = 25 F; zero bias
            lim = float(np.sqrt(6.0 / (25 * cin + 25 * F)))
            k = (torch.rand(5, 5, cin, F, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * lim
            setattr(self, "k%d" % i, torch.nn.Parameter(k.to(device)))
            setattr(self, "b%d" % i, torch.nn.Parameter(torch.zeros(F, dtype=torch.float32, device=device)))
            cin = F

    def _params(self):
        return [self.k1, self.b1, self.k2, self.b2, self.k3, self.b3]

    @staticmethod
    def variable_names():
        """the TF variable names of the block under the scope cnn/, in creation order"""
        return ["cnn/conv%d/%s" % (i, kind) for i in (1, 2, 3) for kind in ("kernel", "bias")]

    def variables(self):
        """TF name -> tensor (views of the parameters)"""
        return OrderedDict(zip(self.variable_names(), (q.detach() for q in self._params())))

    def load_variables(self, mapping, scope=""):
        """Copies every variable from mapping[scope + name] (tensors or arrays).  All of them must be there with the right
        number of elements: nothing is written otherwise."""
        load_variables(self.variables(), mapping, scope)

    def forward(self, input_images):
        H.require_device(input_images, "input_images", "cnn", capture_too=True)
        S = self.canvas_size
        shp = tuple(int(d) for d in input_images.shape)
        if not (len(shp) >= 2 and shp[0] >= 1 and shp[1:] in ((S * S,), (S, S, 1))):
            raise ValueError("cnn: input_images must be [B, %d] or [B, %d, %d, 1], got %r" % (S * S, S, S, shp))
        if self.k1.device != input_images.device:
            raise H.AirHipError("cnn: the module's variables live on %s, input_images on %s" % (self.k1.device, input_images.device))
        return _CnnFn.apply(self, input_images, *self._params())


def cnn(input_images, canvas_size=50, cnn_filters=8, *, module=None):
    """air_model.py:510-533.  With `module` (a CNN) that module's variables are used -- the variable scope of the reference;
    without one a module with freshly initialised variables is built on the device of `input_images`."""
    H.require_device(input_images, "input_images", "cnn")
    if module is None:
        module = CNN(canvas_size, cnn_filters, device=input_images.device)
    return module(input_images)
