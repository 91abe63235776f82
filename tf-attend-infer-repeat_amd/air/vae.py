"""The variational auto-encoder of the glimpses -- mirror of the reference's air/vae.py:5-43.

``VAE`` is a torch.nn.Module that owns the variables the reference creates under the scope ``vae/``; ``vae(...)`` is the
function with the reference's signature.  Both return the reference's 4-tuple (reconstruction, recognition_mean,
recognition_log_variance, recognition_mean): the fourth value is the MEAN, not the sample (vae.py:43) -- the decoder is
fed the sample.

Every product runs as an air_gemm launch with the descriptors of the model's own forward and backward (AIRModel.
_build_forward / _build_backward: both walk the layer table of air/_layers.py, each building its own descriptors), over
the M rows of ``inputs``: bias + activation per recognition layer, ONE product with the
re-parameterisation in its epilogue for rec_mean | rec_log_variance (stored as one fused [K, 2Z] matrix, like the
model's ml_w), bias + activation per generative layer, sigmoid(. + likelihood_std * eps_x) for gen_mean.  With the
model's variables, glimpses and noise the fp32 path reproduces the model's ``ml`` and ``vrec`` bit for bit.  The fused
bottleneck launches of the model are not used (their shape limits and the KL they fold in belong to the model).

Differentiable through torch.autograd with hand-written kernels behind it: air_sigmoid_bwd, air_gemm (transB, the saved
activation as ``aux``) for the data gradients, air_reparam_bwd_plain for the sample, and ONE air_wgrad_grouped launch for
all weight and bias gradients.  Everything is enqueued on the current stream, nothing synchronises and no device value is
read on the host.  There is no CPU fallback.

Stream capture is NOT supported yet: a torch.cuda.graph capture of a forward + backward through this module and the
air.concrete ops ended in a segmentation fault inside the runtime's end of capture on the MI355X,
so the module refuses to run while the current stream is capturing.

Noise: ``eps_z`` [M, Z] and ``eps_x`` [M, input_dim] are the caller's standard normals; with None they are drawn on the
device by air_philox_fill under the key (module seed, call counter).  With likelihood_std == 0 no eps_x is drawn or read."""
import ctypes as C
from collections import OrderedDict

import torch

from . import _hip as H
from ._hip import MAX_WGRAD_PROBLEMS  # noqa: F401  -- (this module's public name of the limit; _hip.py owns the value)
from ._layers import VaeLayers, load_variables
from ._store import xavier_uniform_

_ACTIVATIONS = {"softplus": (H.ACT_SOFTPLUS, H.GRAD_SOFTPLUS), "relu": (H.ACT_RELU, H.GRAD_RELU)}
_SALT = 0x56414531            # keeps this module's noise apart from others keyed by the same user seed


def _gemm(prec, A, Bm, Cm, M, N, K, lda, ldb, ldc, tb=0, bias=None, aux=None, ldaux=0, aux_scale=0.0, act=H.ACT_NONE,
          actgrad=H.GRAD_NONE, epi=H.EPI_GENERIC, p0=None, q0=None):
    """one air_gemm launch on the current stream; the fields AIRModel._gemm fills for the same layer, without twins"""
    g = H.Gemm(A=H.ptr(A), B=H.ptr(Bm), C=H.ptr(Cm), M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, transB=tb, bias=H.ptr(bias),
               aux=H.ptr(aux), ldaux=ldaux, aux_scale=aux_scale, act=act, actgrad=actgrad, precision=prec, epi=epi,
               p0=H.ptr(p0), q0=H.ptr(q0))
    H.launch("air_gemm", Cm.device, C.byref(g))


class _VaeFn(torch.autograd.Function):
    """forward(ctx, module, inputs, eps_z, eps_x, *parameters) -> (reconstruction, mean, log_variance); the parameters in
    the order of VAE._fused().  Both directions walk the module's layer table (air/_layers.py)."""

    @staticmethod
    def forward(ctx, mod, inputs, eps_z, eps_x, *params):
        dev = inputs.device
        P = OrderedDict(zip(mod._fused(), (q.detach() for q in params)))
        x = inputs.detach().contiguous().float()
        L, M, Z, prec = mod._layers, int(x.shape[0]), mod.latent_dim, mod._prec
        act, _ = _ACTIVATIONS[mod.activation]
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        xs = [x]                               # the input of every product, in layer order (the A of its weight gradient)
        for l in L.rec:
            xs.append(f(M, l.N))
            _gemm(prec, xs[-2], P[l.w], xs[-1], M, l.N, l.K, l.K, l.N, l.N, bias=P[l.b], act=act)
        l = L.ml
        ml, zs = f(M, l.N), f(M, Z)
        _gemm(prec, xs[-1], P[l.w], ml, M, l.N, l.K, l.K, l.N, l.N, bias=P[l.b], epi=H.EPI_REPARAM_FWD, p0=eps_z, q0=zs)
        xs.append(zs)
        for l in L.gen:
            xs.append(f(M, l.N))
            _gemm(prec, xs[-2], P[l.w], xs[-1], M, l.N, l.K, l.K, l.N, l.N, bias=P[l.b], act=act)
        l = L.out
        rec = f(M, l.N)
        # (AIR_ACT_SIGMOID_NOISE wants its noise operand: without likelihood noise it reads zeros, never eps_x)
        noise = eps_x if eps_x is not None else torch.zeros(M, l.N, dtype=torch.float32, device=dev)
        _gemm(prec, xs[-1], P[l.w], rec, M, l.N, l.K, l.K, l.N, l.N, bias=P[l.b], act=H.ACT_SIGMOID_NOISE, aux=noise, ldaux=l.N,
              aux_scale=float(mod.likelihood_std) if eps_x is not None else 0.0)
        ctx.set_materialize_grads(False)
        ctx.mod, ctx.P, ctx.xs = mod, P, xs
        ctx.ml, ctx.eps_z, ctx.rec = ml, eps_z, rec
        ctx.in_shape = inputs.shape
        return rec, ml[:, :Z], ml[:, Z:]

    @staticmethod
    def backward(ctx, d_rec, d_mean, d_lv):
        mod, P, xs = ctx.mod, ctx.P, ctx.xs
        rec, ml = ctx.rec, ctx.ml
        dev = rec.device
        L, M, Z, prec = mod._layers, int(rec.shape[0]), mod.latent_dim, mod._prec
        _, actgrad = _ACTIVATIONS[mod.activation]
        n_enc = len(L.encoder)
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        c = lambda t: None if t is None else t.contiguous().float()  # noqa: E731
        d_rec = c(d_rec) if d_rec is not None else torch.zeros_like(rec)
        d_mean, d_lv = c(d_mean), c(d_lv)

        def data_grad(l, dy, saved=None):
            """dX = dY . W^T of product l, times the activation's derivative from the saved output X where one is given"""
            g = f(M, l.K)
            _gemm(prec, dy, P[l.w], g, M, l.K, l.N, l.N, l.N, l.K, tb=1, aux=saved, ldaux=l.K if saved is not None else 0,
                  actgrad=actgrad if saved is not None else H.GRAD_NONE)
            return g
        # d loss / d (pre-activation) of every product, in layer order (the dY of its weight gradient)
        dys = [None] * len(xs)
        dys[-1] = f(M, L.out.N)
        H.launch("air_sigmoid_bwd", dev, H.ptr(d_rec), H.ptr(rec), H.ptr(dys[-1]), M * L.out.N)
        for i in reversed(range(len(L.gen))):                  # decoder[i + 1] read the activation of gen[i], xs[n_enc + i + 1]
            dys[n_enc + i] = data_grad(L.decoder[i + 1], dys[n_enc + i + 1], xs[n_enc + i + 1])
        d_z = data_grad(L.decoder[0], dys[n_enc])
        dys[n_enc - 1] = f(M, 2 * Z)
        H.launch("air_reparam_bwd_plain", dev, H.ptr(d_z), H.ptr(ml), H.ptr(ctx.eps_z), H.ptr(d_mean), H.ptr(d_lv),
                 H.ptr(dys[n_enc - 1]), M, Z)
        for i in reversed(range(len(L.rec))):                  # encoder[i + 1] read the activation of rec[i], xs[i + 1]
            dys[i] = data_grad(L.encoder[i + 1], dys[i + 1], xs[i + 1])
        d_in = None
        if ctx.needs_input_grad[1]:
            d_in = data_grad(L.encoder[0], dys[0]).view(ctx.in_shape)
        grads = [None] * len(P)
        if any(ctx.needs_input_grad[4:]):
            # all dW = X^T . dY and db = column sums of dY in ONE launch; problem i is layer i
            grads = [torch.empty_like(q) for q in P.values()]
            probs = [H.Wgrad(A=H.ptr(xin), dY=H.ptr(dy), dW=H.ptr(grads[2 * i]), db=H.ptr(grads[2 * i + 1]),
                             M=l.K, N=l.N, K=M, lda=l.K, ldb=l.N, ldc=l.N)
                     for i, (l, xin, dy) in enumerate(zip(L.products(), xs, dys))]
            arr = (H.Wgrad * len(probs))(*probs)
            H.launch("air_wgrad_grouped", dev, arr, len(probs), prec, None, None)
        return (None, d_in, None, None) + tuple(grads)


class VAE(torch.nn.Module):
    """vae.py:5-43 as a module.  precision: "fp32" (exact-fp32 MFMA), "bf16" (operands rounded to bf16 on their way into LDS,
    fp32 accumulate) or None for the package default (GEMM_PRECISION of air._hip; air_model reads the same)."""

    def __init__(self, input_dim, rec_hidden_units, latent_dim, gen_hidden_units, likelihood_std=0.0, activation="softplus",
                 precision=None, device="cuda", seed=0):
        super().__init__()
        rec, gen = tuple(int(u) for u in rec_hidden_units), tuple(int(u) for u in gen_hidden_units)
        if activation not in _ACTIVATIONS:
            raise ValueError("activation must be one of %s (the activations air_gemm has), got %r"
                             % (sorted(_ACTIVATIONS), activation))
        prec = precision or H.GEMM_PRECISION
        if prec not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32', 'bf16' or None")
        if len(rec) + len(gen) + 2 > H.MAX_WGRAD_PROBLEMS:
            raise NotImplementedError("len(rec_hidden_units) + len(gen_hidden_units) + 2 = %d weight-gradient problems exceed the "
                                      "limit of %d of the grouped weight-gradient launch" % (len(rec) + len(gen) + 2, H.MAX_WGRAD_PROBLEMS))
        if int(input_dim) < 1 or int(latent_dim) < 1 or any(u < 1 for u in rec + gen):
            raise ValueError("input_dim, latent_dim and the hidden widths must be positive")
        self.input_dim, self.latent_dim = int(input_dim), int(latent_dim)
        self.rec_hidden_units, self.gen_hidden_units = rec, gen
        self.likelihood_std = float(likelihood_std)
        self.activation = activation
        self.precision = prec
        self._prec = 1 if prec == "bf16" else 0
        self._seed, self._calls = int(seed), 0
        self._layers = VaeLayers(self.input_dim, rec, self.latent_dim, gen)
        shapes = self._layers.shapes()
        for k, shp in shapes.items():
            setattr(self, k, torch.nn.Parameter(torch.zeros(*shp, dtype=torch.float32, device=device)))
        self._names = tuple(shapes)
        xavier_uniform_(self.variables(), seed)

    def _fused(self):
        """the parameters under their fused names (rec<i>_w/_b, ml_w/_b, gen<i>_w/_b, out_w/_b), in layer order"""
        return OrderedDict((k, getattr(self, k)) for k in self._names)

    @staticmethod
    def variable_names(rec_hidden_units, gen_hidden_units):
        """the TF variable names of vae.py under the scope vae/, in creation order"""
        return VaeLayers.tf_names_of(len(rec_hidden_units), len(gen_hidden_units))

    def variables(self):
        """TF name -> tensor (views of the parameters; rec_mean / rec_log_variance are the column halves of ml_w / ml_b)"""
        return self._layers.tf_views(OrderedDict((k, v.detach()) for k, v in self._fused().items()))

    def load_variables(self, mapping, scope=""):
        """Copies every variable from mapping[scope + name] (tensors or arrays; e.g. AIRModel.variables, whose keys are these
        names).  All of them must be there with the right number of elements: nothing is written otherwise."""
        load_variables(self.variables(), mapping, scope)

    def manual_seed(self, seed):
        """Seed of the normals drawn when eps_z / eps_x are None; rewinds the call counter."""
        self._seed, self._calls = int(seed), 0

    def _draw(self, M, dev):
        """(eps_z, eps_x or None) from one air_philox_fill launch"""
        nz = (M * self.latent_dim + 7) & ~7                     # eps_x starts 32-byte aligned
        nx = M * self.input_dim if self.likelihood_std != 0.0 else 0
        buf = torch.empty(nz + nx, dtype=torch.float32, device=dev)
        H.launch("air_philox_fill", dev, H.ptr(buf), buf.numel(), None, 0, C.c_uint64(self._seed ^ _SALT), C.c_uint64(self._calls))
        self._calls += 1
        return buf[:M * self.latent_dim].view(M, self.latent_dim), (buf[nz:].view(M, self.input_dim) if nx else None)

    def forward(self, inputs, eps_z=None, eps_x=None):
        H.require_device(inputs, "inputs", "vae", capture_too=True)
        if inputs.dim() != 2 or int(inputs.shape[1]) != self.input_dim or int(inputs.shape[0]) < 1:
            raise ValueError("vae: inputs must be [M, %d], got %r" % (self.input_dim, tuple(inputs.shape)))
        if self.out_w.device != inputs.device:
            raise H.AirHipError("vae: the module's variables live on %s, inputs on %s" % (self.out_w.device, inputs.device))
        M = int(inputs.shape[0])
        noisy = self.likelihood_std != 0.0
        if eps_z is None or (noisy and eps_x is None):
            dz, dx = self._draw(M, inputs.device)
            eps_z = dz if eps_z is None else eps_z
            eps_x = dx if eps_x is None else eps_x
        eps_z = eps_z.detach().to(inputs.device).reshape(M, self.latent_dim).contiguous().float()
        eps_x = eps_x.detach().to(inputs.device).reshape(M, self.input_dim).contiguous().float() if noisy else None
        rec, mean, lv = _VaeFn.apply(self, inputs, eps_z, eps_x, *self._fused().values())
        return rec, mean, lv, mean


def vae(inputs, input_dim, rec_hidden_units, latent_dim, gen_hidden_units, likelihood_std=0.0, activation="softplus", *,
        module=None, eps_z=None, eps_x=None):
    """vae.py:5-43.  With `module` (a VAE) that module's variables are used -- the variable scope of the reference; without
    one a module with freshly initialised variables is built on the device of `inputs`."""
    H.require_device(inputs, "inputs", "vae")
    if module is None:
        module = VAE(input_dim, rec_hidden_units, latent_dim, gen_hidden_units, likelihood_std, activation, device=inputs.device)
    return module(inputs, eps_z=eps_z, eps_x=eps_x)
