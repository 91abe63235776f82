"""The variational auto-encoder of the glimpses -- mirror of the reference's air/vae.py:5-43.

``VAE`` is a torch.nn.Module that owns the variables the reference creates under the scope ``vae/``; ``vae(...)`` is the
function with the reference's signature.  Both return the reference's 4-tuple (reconstruction, recognition_mean,
recognition_log_variance, recognition_mean): the fourth value is the MEAN, not the sample (vae.py:43) -- the decoder is
fed the sample.

Every product runs as an air_gemm launch with the descriptors of the model's own forward and backward (AIRModel.
_build_programs), over the M rows of ``inputs``: bias + activation per recognition layer, ONE product with the
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

import numpy as np
import torch

from . import _hip as H
from . import air_model as _am

MAX_WGRAD_PROBLEMS = 16       # air_wgrad_grouped takes that many problems in one launch
_ACTIVATIONS = {"softplus": (H.ACT_SOFTPLUS, H.GRAD_SOFTPLUS), "relu": (H.ACT_RELU, H.GRAD_RELU)}
_SALT = 0x56414531            # keeps this module's noise apart from others keyed by the same user seed


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _gemm(prec, A, Bm, Cm, M, N, K, lda, ldb, ldc, tb=0, bias=None, aux=None, ldaux=0, aux_scale=0.0, act=H.ACT_NONE,
          actgrad=H.GRAD_NONE, epi=H.EPI_GENERIC, p0=None, q0=None):
    """one air_gemm launch on the current stream; the fields AIRModel._gemm fills for the same layer, without twins"""
    g = H.Gemm(_p(A), _p(Bm), _p(Cm), M, N, K, lda, ldb, ldc, 0, tb, _p(bias), None, 0, _p(aux), ldaux, aux_scale, act, actgrad,
               0, prec, epi, 0, 0, 0, 0, 0, _p(p0), None, None, None, _p(q0), None, None, None,
               None, None, None, None, None, None)
    H.check(H.lib().air_gemm(C.byref(g), _stream(Cm.device)), "air_gemm")


class _VaeFn(torch.autograd.Function):
    """forward(ctx, module, inputs, eps_z, eps_x, *parameters) -> (reconstruction, mean, log_variance); the parameters in
    the order of VAE._fused()."""

    @staticmethod
    def forward(ctx, mod, inputs, eps_z, eps_x, *params):
        dev = inputs.device
        P = OrderedDict(zip(mod._fused(), (q.detach() for q in params)))
        x = inputs.detach().contiguous().float()
        M, d, Z, prec = int(x.shape[0]), mod.input_dim, mod.latent_dim, mod._prec
        act, _ = _ACTIVATIONS[mod.activation]
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        xs = [x]                               # the input of every product, in layer order (the A of its weight gradient)
        k = d
        rec_act, gen_act = [], []
        for i, u in enumerate(mod.rec_hidden_units):
            rec_act.append(f(M, u))
            _gemm(prec, xs[-1], P["rec%d_w" % i], rec_act[i], M, u, k, k, u, u, bias=P["rec%d_b" % i], act=act)
            xs.append(rec_act[i]); k = u
        ml, zs = f(M, 2 * Z), f(M, Z)
        _gemm(prec, xs[-1], P["ml_w"], ml, M, 2 * Z, k, k, 2 * Z, 2 * Z, bias=P["ml_b"], epi=H.EPI_REPARAM_FWD, p0=eps_z, q0=zs)
        xs.append(zs); k = Z
        for i, u in enumerate(mod.gen_hidden_units):
            gen_act.append(f(M, u))
            _gemm(prec, xs[-1], P["gen%d_w" % i], gen_act[i], M, u, k, k, u, u, bias=P["gen%d_b" % i], act=act)
            xs.append(gen_act[i]); k = u
        rec = f(M, d)
        # (AIR_ACT_SIGMOID_NOISE wants its noise operand: without likelihood noise it reads zeros, never eps_x)
        noise = eps_x if eps_x is not None else torch.zeros(M, d, dtype=torch.float32, device=dev)
        _gemm(prec, xs[-1], P["out_w"], rec, M, d, k, k, d, d, bias=P["out_b"], act=H.ACT_SIGMOID_NOISE, aux=noise, ldaux=d,
              aux_scale=float(mod.likelihood_std) if eps_x is not None else 0.0)
        ctx.set_materialize_grads(False)
        ctx.mod, ctx.P, ctx.xs = mod, P, xs
        ctx.rec_act, ctx.gen_act, ctx.ml, ctx.eps_z, ctx.rec = rec_act, gen_act, ml, eps_z, rec
        ctx.in_shape = inputs.shape
        return rec, ml[:, :Z], ml[:, Z:]

    @staticmethod
    def backward(ctx, d_rec, d_mean, d_lv):
        mod, P, xs = ctx.mod, ctx.P, ctx.xs
        rec, ml = ctx.rec, ctx.ml
        dev = rec.device
        M, d, Z, prec = int(rec.shape[0]), mod.input_dim, mod.latent_dim, mod._prec
        _, actgrad = _ACTIVATIONS[mod.activation]
        rec_u, gen_u = mod.rec_hidden_units, mod.gen_hidden_units
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        lib, s = H.lib(), _stream(dev)
        c = lambda t: None if t is None else t.contiguous().float()  # noqa: E731
        d_rec = c(d_rec) if d_rec is not None else torch.zeros_like(rec)
        d_mean, d_lv = c(d_mean), c(d_lv)
        # d loss / d (pre-activation) of every product, in layer order (the dY of its weight gradient)
        dys = [None] * (len(rec_u) + len(gen_u) + 2)
        d_pre = f(M, d)
        H.check(lib.air_sigmoid_bwd(_p(d_rec), _p(rec), _p(d_pre), M * d, s), "air_sigmoid_bwd")
        dys[-1] = d_pre
        # decoder data gradients: dX = dY . W^T, times the activation's derivative from the saved output
        dy, n_out, wname = d_pre, d, "out_w"
        for i in reversed(range(len(gen_u))):
            u = gen_u[i]
            g = f(M, u)
            _gemm(prec, dy, P[wname], g, M, u, n_out, n_out, n_out, u, tb=1, aux=ctx.gen_act[i], ldaux=u, actgrad=actgrad)
            dys[len(rec_u) + 1 + i] = g
            dy, n_out, wname = g, u, "gen%d_w" % i
        d_z = f(M, Z)
        _gemm(prec, dy, P[wname], d_z, M, Z, n_out, n_out, n_out, Z, tb=1)
        d_ml = f(M, 2 * Z)
        H.check(lib.air_reparam_bwd_plain(_p(d_z), _p(ml), _p(ctx.eps_z), _p(d_mean), _p(d_lv), _p(d_ml), M, Z, s),
                "air_reparam_bwd_plain")
        dys[len(rec_u)] = d_ml
        dy, n_out, wname = d_ml, 2 * Z, "ml_w"
        for i in reversed(range(len(rec_u))):
            u = rec_u[i]
            g = f(M, u)
            _gemm(prec, dy, P[wname], g, M, u, n_out, n_out, n_out, u, tb=1, aux=ctx.rec_act[i], ldaux=u, actgrad=actgrad)
            dys[i] = g
            dy, n_out, wname = g, u, "rec%d_w" % i
        d_in = None
        if ctx.needs_input_grad[1]:
            d_in = f(M, d)
            _gemm(prec, dy, P[wname], d_in, M, d, n_out, n_out, n_out, d, tb=1)
            d_in = d_in.view(ctx.in_shape)
        grads = [None] * len(P)
        if any(ctx.needs_input_grad[4:]):
            # all dW = X^T . dY and db = column sums of dY in ONE launch; problem i is layer i
            names = list(P)
            grads = [torch.empty_like(P[n]) for n in names]
            probs = []
            for i, (xin, dyi) in enumerate(zip(xs, dys)):
                K_, N_ = int(xin.shape[1]), int(dyi.shape[1])
                probs.append(H.Wgrad(_p(xin), _p(dyi), _p(grads[2 * i]), _p(grads[2 * i + 1]), K_, N_, M, K_, N_, N_, 0, 0, 0, 0,
                                     None, None))
            arr = (H.Wgrad * len(probs))(*probs)
            H.check(lib.air_wgrad_grouped(arr, len(probs), prec, None, None, s), "air_wgrad_grouped")
        return (None, d_in, None, None) + tuple(grads)


class VAE(torch.nn.Module):
    """vae.py:5-43 as a module.  precision: "fp32" (exact-fp32 MFMA), "bf16" (operands rounded to bf16 on their way into LDS,
    fp32 accumulate) or None for the package default (air_model.GEMM_PRECISION)."""

    def __init__(self, input_dim, rec_hidden_units, latent_dim, gen_hidden_units, likelihood_std=0.0, activation="softplus",
                 precision=None, device="cuda", seed=0):
        super().__init__()
        rec, gen = tuple(int(u) for u in rec_hidden_units), tuple(int(u) for u in gen_hidden_units)
        if activation not in _ACTIVATIONS:
            raise ValueError("activation must be one of %s (the activations air_gemm has), got %r"
                             % (sorted(_ACTIVATIONS), activation))
        prec = precision or _am.GEMM_PRECISION
        if prec not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32', 'bf16' or None")
        if len(rec) + len(gen) + 2 > MAX_WGRAD_PROBLEMS:
            raise NotImplementedError("len(rec_hidden_units) + len(gen_hidden_units) + 2 = %d weight-gradient problems exceed the "
                                      "limit of %d of the grouped weight-gradient launch" % (len(rec) + len(gen) + 2, MAX_WGRAD_PROBLEMS))
        if int(input_dim) < 1 or int(latent_dim) < 1 or any(u < 1 for u in rec + gen):
            raise ValueError("input_dim, latent_dim and the hidden widths must be positive")
        self.input_dim, self.latent_dim = int(input_dim), int(latent_dim)
        self.rec_hidden_units, self.gen_hidden_units = rec, gen
        self.likelihood_std = float(likelihood_std)
        self.activation = activation
        self.precision = prec
        self._prec = 1 if prec == "bf16" else 0
        self._seed, self._calls = int(seed), 0
        Z = self.latent_dim
        shapes = OrderedDict()
        prev = self.input_dim
        for i, u in enumerate(rec):
            shapes["rec%d_w" % i], shapes["rec%d_b" % i] = (prev, u), (u,)
            prev = u
        shapes["ml_w"], shapes["ml_b"] = (prev, 2 * Z), (2 * Z,)
        prev = Z
        for i, u in enumerate(gen):
            shapes["gen%d_w" % i], shapes["gen%d_b" % i] = (prev, u), (u,)
            prev = u
        shapes["out_w"], shapes["out_b"] = (prev, self.input_dim), (self.input_dim,)
        for k, shp in shapes.items():
            setattr(self, k, torch.nn.Parameter(torch.zeros(*shp, dtype=torch.float32, device=device)))
        self._names = tuple(shapes)
        _am.xavier_uniform_(self.variables(), seed)

    def _fused(self):
        """the parameters under their fused names (rec<i>_w/_b, ml_w/_b, gen<i>_w/_b, out_w/_b), in layer order"""
        return OrderedDict((k, getattr(self, k)) for k in self._names)

    @staticmethod
    def variable_names(rec_hidden_units, gen_hidden_units):
        """the TF variable names of vae.py under the scope vae/, in creation order"""
        layers = ["recognition_%d" % (i + 1) for i in range(len(rec_hidden_units))] + ["rec_mean", "rec_log_variance"] + \
                 ["generative_%d" % (i + 1) for i in range(len(gen_hidden_units))] + ["gen_mean"]
        return ["vae/%s/%s" % (layer, kind) for layer in layers for kind in ("weights", "biases")]

    def variables(self):
        """TF name -> tensor (views of the parameters; rec_mean / rec_log_variance are the column halves of ml_w / ml_b)"""
        Z, P = self.latent_dim, OrderedDict((k, v.detach()) for k, v in self._fused().items())
        out = OrderedDict()
        for i in range(len(self.rec_hidden_units)):
            out["vae/recognition_%d/weights" % (i + 1)], out["vae/recognition_%d/biases" % (i + 1)] = P["rec%d_w" % i], P["rec%d_b" % i]
        out["vae/rec_mean/weights"], out["vae/rec_mean/biases"] = P["ml_w"][:, :Z], P["ml_b"][:Z]
        out["vae/rec_log_variance/weights"], out["vae/rec_log_variance/biases"] = P["ml_w"][:, Z:], P["ml_b"][Z:]
        for i in range(len(self.gen_hidden_units)):
            out["vae/generative_%d/weights" % (i + 1)], out["vae/generative_%d/biases" % (i + 1)] = P["gen%d_w" % i], P["gen%d_b" % i]
        out["vae/gen_mean/weights"], out["vae/gen_mean/biases"] = P["out_w"], P["out_b"]
        return out

    def load_variables(self, mapping, scope=""):
        """Copies every variable from mapping[scope + name] (tensors or arrays; e.g. AIRModel.variables, whose keys are these
        names).  All of them must be there with the right number of elements: nothing is written otherwise."""
        prefix = scope if (not scope or scope.endswith("/")) else scope + "/"
        mine = self.variables()
        src = {}
        for name, v in mine.items():
            if prefix + name not in mapping:
                raise KeyError("missing variable %s" % (prefix + name))
            t = mapping[prefix + name]
            t = t.detach() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
            if t.numel() != v.numel():
                raise ValueError("variable %s has %r elements, expected %r" % (prefix + name, tuple(t.shape), tuple(v.shape)))
            src[name] = t
        with torch.no_grad():
            for name, v in mine.items():
                v.copy_(src[name].to(device=v.device, dtype=v.dtype).reshape(v.shape))

    def manual_seed(self, seed):
        """Seed of the normals drawn when eps_z / eps_x are None; rewinds the call counter."""
        self._seed, self._calls = int(seed), 0

    def _draw(self, M, dev):
        """(eps_z, eps_x or None) from one air_philox_fill launch"""
        nz = (M * self.latent_dim + 7) & ~7                     # eps_x starts 32-byte aligned
        nx = M * self.input_dim if self.likelihood_std != 0.0 else 0
        buf = torch.empty(nz + nx, dtype=torch.float32, device=dev)
        H.check(H.lib().air_philox_fill(_p(buf), buf.numel(), None, 0, C.c_uint64(self._seed ^ _SALT), C.c_uint64(self._calls),
                                        _stream(dev)), "air_philox_fill")
        self._calls += 1
        return buf[:M * self.latent_dim].view(M, self.latent_dim), (buf[nz:].view(M, self.input_dim) if nx else None)

    def forward(self, inputs, eps_z=None, eps_x=None):
        if not (torch.is_tensor(inputs) and inputs.is_cuda):
            raise H.AirHipError("vae: inputs must be a device tensor (no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise H.AirHipError("vae: not supported under stream capture (torch.cuda.graph); run it eagerly")
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
    if not (torch.is_tensor(inputs) and inputs.is_cuda):
        raise H.AirHipError("vae: inputs must be a device tensor (no CPU fallback)")
    if module is None:
        module = VAE(input_dim, rec_hidden_units, latent_dim, gen_hidden_units, likelihood_std, activation, device=inputs.device)
    return module(inputs, eps_z=eps_z, eps_x=eps_x)
