"""The variables of a scope: ONE flat fp32 buffer with its gradients, Adam slots and bf16 shadows (VariableStore), the
registry of scopes that AIRModel(reuse=True) looks them up in, and the Glorot initialiser air.vae shares.

Nothing here knows of launch lists or of AIRModel: a store is built from a dict of hyper-parameters and a device
(tests/golden/make_store_layout.py, tests/test_cnn_step_abi.py).  air_model imports every name of this module back,
so `air_model.VariableStore`, `air_model._SCOPES`, ... are these objects.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _hip as H
from ._hip import ptr as _ptr
from ._layers import VaeLayers

_SCOPES = {}


def reset_default_graph():
    """Drops all variable scopes (the tf.reset_default_graph() of this runtime)."""
    _SCOPES.clear()


def saved_cnn_arguments(path):
    """dict(cnn=, cnn_filters=) of the model saved at `path` -- a torch.save'd state dict, or the prefix of a TensorFlow
    bundle --, read off its conv variables (cnn/conv1/bias holds one element per filter).  cnn=False for a model saved
    without the front-end, which is every checkpoint written before it existed."""
    if os.path.exists(path + ".index"):
        import tf_checkpoint as tfc
        entry = tfc.read_index(path + ".index")[1].get(tfc.CNN_SCOPE + "conv1/bias")
        filters = int(np.prod(entry["shape"])) if entry is not None else 0
    else:
        bias = torch.load(path, map_location="cpu").get("cnn/conv1/bias")
        filters = int(np.prod(np.shape(bias))) if bias is not None else 0
    return dict(cnn=filters > 0, cnn_filters=filters if filters > 0 else 8)


def _align8(n):
    return (n + 7) & ~7


def xavier_uniform_(variables, seed=0, rng=None):
    """Fills every 2-D tensor of the name -> tensor mapping with Glorot-uniform values, limit sqrt(6 / (fan_in + fan_out)), from
    ONE numpy stream seeded by `seed` (or the stream `rng`, continued), in the mapping's order (layers.xavier_initializer, the
    TF 1.3 default of fully_connected and BasicLSTMCell); 1-D tensors (biases: zeros) are left alone, and so are the 4-D
    conv kernels (VariableStore.initialize draws them)."""
    if rng is None:
        rng = np.random.RandomState(seed)
    with torch.no_grad():
        for v in variables.values():
            if v.dim() == 2:
                limit = math.sqrt(6.0 / (v.shape[0] + v.shape[1]))
                v.copy_(torch.from_numpy(rng.uniform(-limit, limit, size=tuple(v.shape)).astype(np.float32)))


class VariableStore:
    """All trainable variables of one scope in ONE flat fp32 buffer (+ grads,
    Adam m/v) so that the optimizer and the data-parallel all-reduce are a
    single pass / a single collective.  TF variable names (model/air-model.index,
    SURVEY appendix B) are exposed as views."""

    def __init__(self, hp, device, seed=0):
        self.hp = hp
        self.device = device
        D, d = hp["canvas_size"] ** 2, hp["windows_size"] ** 2
        R, Z = hp["rnn_units"], hp["vae_latent_dimensions"]
        Hs, Hh, Hz = hp["scale_hidden_units"], hp["shift_hidden_units"], hp["z_pres_hidden_units"]
        HT, Hmax = 2 * Hs + 2 * Hh + Hz, max(Hs, Hh, Hz)
        # the LSTM's input: the canvas, or the [S // 4, S // 4, F] output of the conv front-end (reference :510-535)
        cnn, F = bool(hp.get("cnn", False)), int(hp.get("cnn_filters", 0))
        Din = (hp["canvas_size"] // 4) ** 2 * F if cnn else D
        self.dims = dict(D=D, d=d, R=R, Z=Z, Hs=Hs, Hh=Hh, Hz=Hz, HT=HT, Hmax=Hmax, Din=Din)
        self.vae_layers = VaeLayers(d, hp["vae_recognition_units"], Z, hp["vae_generative_units"])

        fused = OrderedDict()           # fused device tensors: name -> shape
        fused["lstm_kernel"] = (Din + R, 4 * R)
        fused["lstm_bias"] = (4 * R,)
        fused["whid"] = (R, HT)
        fused["bhid"] = (HT,)
        fused["wout"] = (7, Hmax)
        fused["bout"] = (8,)
        fused.update(self.vae_layers.shapes())
        # the conv variables BEHIND every other entry: the offsets of a cnn=False store are those of every earlier build
        self.cnn_names = []
        if cnn:
            from .cnn import CNN
            self.cnn_names = CNN.variable_names()
            for i, name in enumerate(self.cnn_names):
                fused[name] = (5, 5, (1 if i < 2 else F), F) if i % 2 == 0 else (F,)

        self.offsets = OrderedDict()
        off = 0
        for k, shp in fused.items():
            self.offsets[k] = off
            off += _align8(int(np.prod(shp)))               # every tensor 32-byte aligned in fp32, 16-byte in the bf16 shadow
        self.n = off                                        # multiple of 8
        # +4 tail floats: loss / accuracy ride along in the gradient all-reduce
        self.params = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.n + 4, dtype=torch.float32, device=device)
        self.m = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.v = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.istate = torch.zeros(H.IST_COUNT, dtype=torch.int32, device=device)
        # global-norm partial sums: air_grad_sqnorm's fixed count, or one per weight-gradient workgroup
        self.partials = torch.zeros(max(H.lib().air_optim_num_partials(self.n), 16384), dtype=torch.float32, device=device)
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=device)
        self.synced_world = 1            # world size the replicas were last made identical for (AIRModel.sync_parameters)
        # bf16 shadow of the whole flat variable buffer (same offsets): the weight operand of every bf16 GEMM.
        # Adam rewrites it with the variables (air_adam_clip_step's bf16_shadow); any host-side change of the
        # variables (initialize / load_state_dict / sync / checkpoint load) marks it stale and the next
        # forward() / training() re-derives it with one air_bf16_twin launch.  Code that writes into
        # `variables[...]` views directly must call touch().
        self.params16 = torch.zeros(self.n, dtype=torch.int16, device=device)
        self.shadow_stale = True
        # PANEL-BLOCKED bf16 twins (air_panel_t) of the weights the forward (untransposed) products read: 16-column
        # panels of [K][16], so that a 16-column GEMM tile fetches whole cache lines; the LSTM kernel in gate-interleaved
        # panels (the four gates of four units in 32 contiguous bytes per row), in two pieces (Wx rows, Wh rows).
        # Maintained by Adam next to the row-major shadow (which the transposed data-gradient products keep reading);
        # Wx has no other reader than the hoisted x.Wx, so its row-major shadow is dropped ("exclusive") unless the
        # canvas is large (the throughput tiling of D > 4096 reads row-major lines) or the shape cannot fuse the first step --
        # or the conv front-end is on: the data gradient d rnn_input = dgsum . Wx^T reads the row-major shadow of Wx.
        pan, poff = [], 0
        self.panel_off = {}

        def add_panel(key, src_off, K, N, gates, exclusive=False):
            nonlocal poff
            if N % 8 or src_off % 4 or (gates and (N // 4) % 4):
                return
            self.panel_off[key] = poff
            pan.append(H.Panel(src_off, poff, K, N, 4 if gates else 0, 1 if exclusive else 0))
            poff += _align8(K * N if gates else ((N + 15) // 16) * 16 * K)
        o = self.offsets["lstm_kernel"]
        # (its one reader is the x.Wx launch that also runs the first step -- which needs D % 4 == 0 and R % 4 == 0: a shape that
        # cannot fuse keeps the row-major shadow of Wx; the throughput tiling of a large canvas reads row-major lines: no panel)
        if Din <= 4096 and Din % 4 == 0 and R % 4 == 0:
            add_panel("Wx", o, Din, 4 * R, True, exclusive=not cnn)
        add_panel("Wh", o + Din * 4 * R, R, 4 * R, True)
        for k, shp in fused.items():
            if k.endswith("_w") and k not in ("ml_w", "gen0_w") or k == "whid":
                add_panel(k, self.offsets[k], shp[0], shp[1], False)
        pan = pan[:H.MAX_PANELS]
        self.panels = (H.Panel * len(pan))(*pan)
        self.panel_off = {k: v for k, v in self.panel_off.items() if any(q.dst_off == v for q in pan)}
        # True: params16 is NOT maintained over the Wx rows of the LSTM kernel (only its panel twin is)
        self.wx_exclusive = "Wx" in self.panel_off and bool(pan[0].exclusive)
        self.params16p = torch.zeros(max(poff, 8), dtype=torch.int16, device=device)

        def views(buf):
            return OrderedDict((k, buf[self.offsets[k]:self.offsets[k] + int(np.prod(s))].view(*s))
                               for k, s in fused.items())
        self.P, self.G = views(self.params), views(self.grads)
        self.P16 = views(self.params16)

        # TF-named views (air-model.index names, relative to scope "<scope>/rnn/")
        def named(V):
            o = OrderedDict()
            o["rnn/kernel"], o["rnn/bias"] = V["lstm_kernel"], V["lstm_bias"]
            seg = 0
            rows = (0, 1, (2, 4), (4, 6), 6)
            for hi, (head, wid, k) in enumerate((("scale/mean", Hs, 1), ("scale/log_variance", Hs, 1),
                                                 ("shift/mean", Hh, 2), ("shift/log_variance", Hh, 2),
                                                 ("z_pres/log_odds", Hz, 1))):
                o[head + "/hidden/weights"] = V["whid"][:, seg:seg + wid]
                o[head + "/hidden/biases"] = V["bhid"][seg:seg + wid]
                r = rows[hi]
                r0, r1 = (r, r + 1) if isinstance(r, int) else r
                o[head + "/output/weights"] = V["wout"][r0:r1, :wid].t()
                o[head + "/output/biases"] = V["bout"][r0:r1]
                seg += wid
            o.update(self.vae_layers.tf_views(V))
            for name in self.cnn_names:                  # scope cnn/ sits beside rnn/ (reference :511 against :537)
                o[name] = V[name]
            return o
        self.variables = named(self.P)
        self.gradients = named(self.G)
        self.adam_m, self.adam_v = named(views(self.m)), named(views(self.v))   # TF slots <var>/Adam, <var>/Adam_1
        self.num_trainable = sum(v.numel() for v in self.variables.values())
        self.initialize(seed)

    def initialize(self, seed=0):
        """Xavier/Glorot-uniform weights, zero biases -- TF1.3 defaults of
        BasicLSTMCell / layers.fully_connected (limits sqrt(6/(in+out)) as in
        air-model.meta's initializer constants); zero Adam slots, step 0."""
        self.params.zero_()
        rng = np.random.RandomState(seed)
        # the reference creates the conv layers first (:511-533): their kernels come first from the store's one stream,
        # Glorot-uniform over fan_in = 25 Cin, fan_out = 25 F (tf.layers.conv2d's default), zero biases
        for name in self.cnn_names[::2]:
            k = self.variables[name]
            limit = math.sqrt(6.0 / (25 * k.shape[2] + 25 * k.shape[3]))
            k.copy_(torch.from_numpy(rng.uniform(-limit, limit, size=tuple(k.shape)).astype(np.float32)))
        xavier_uniform_(self.variables, rng=rng)
        self.m.zero_(); self.v.zero_(); self.grads.zero_(); self.istate.zero_()
        self.shadow_stale = True

    def touch(self):
        """The variables were changed from the host side: the bf16 shadow has to be re-derived."""
        self.shadow_stale = True

    def refresh_shadow(self, stream=None):
        if stream is None:
            stream = H.stream(self.device)
        H.check(H.lib().air_bf16_twin(_ptr(self.params), _ptr(self.params16), self.n, stream), "air_bf16_twin")
        if len(self.panels):
            H.check(H.lib().air_panel_shadow(_ptr(self.params), _ptr(self.params16p), self.panels, len(self.panels), stream),
                    "air_panel_shadow")
        self.shadow_stale = False

    def panel(self, key):
        """device pointer (as int16 tensor view) of the panel-blocked twin of matrix `key`, or None"""
        if key not in self.panel_off:
            return None
        return self.params16p[self.panel_off[key]:]

    def state_dict(self):
        sd = OrderedDict((k, v.detach().cpu().contiguous().clone()) for k, v in self.variables.items())
        sd["global_step"] = self.istate[H.IST_GLOBAL_STEP].cpu().clone()
        # Adam slots per variable under TensorFlow's slot names (<var>/Adam, <var>/Adam_1): independent of the
        # alignment / order of the flat buffers, which is an implementation detail that has changed between rounds
        for k in self.variables:
            sd[k + "/Adam"] = self.adam_m[k].detach().cpu().contiguous().clone()
            sd[k + "/Adam_1"] = self.adam_v[k].detach().cpu().contiguous().clone()
        return sd

    def load_state_dict(self, sd, strict=True, load_optimizer=True):
        """Variables (+ global_step, + the Adam slots when the dict carries them per variable).  The dict is validated BEFORE
        anything is written: a caller that catches the error keeps its old state.  load_optimizer=False takes the
        variables and global_step only -- the way to use checkpoints whose optimizer state cannot be read (flat slots
        written by an earlier build) for evaluation / demo.py."""
        missing = [k for k in self.variables if k not in sd]
        if strict and missing:
            raise KeyError("missing variable %s" % missing[0])
        for k, v in self.variables.items():
            if k in sd and int(np.prod(np.shape(sd[k]))) != v.numel():
                raise ValueError("variable %s has %r elements, expected %r" % (k, np.shape(sd[k]), tuple(v.shape)))
        slots = [k for k in self.variables if k + "/Adam" in sd or k + "/Adam_1" in sd]
        if load_optimizer:
            half = [k for k in slots if not (k + "/Adam" in sd and k + "/Adam_1" in sd)]
            if half:
                raise ValueError("state dict carries only one of the two Adam slots (<var>/Adam, <var>/Adam_1) of %s" % half[0])
            if "_adam_m" in sd and not slots:
                # flat slots written by an older build: their offsets are those of THAT build's buffer layout (the alignment
                # of the flat buffers has changed since) -- refuse loudly rather than load shifted slots
                raise ValueError("state dict carries flat Adam slots (_adam_m / _adam_v) of an unknown buffer layout; it needs "
                                 "per-variable slots (<var>/Adam, <var>/Adam_1) -- or load_state_dict(sd, load_optimizer=False) "
                                 "for the variables alone")
            for k in slots:
                for slot in ("/Adam", "/Adam_1"):
                    if int(np.prod(np.shape(sd[k + slot]))) != self.variables[k].numel():
                        raise ValueError("slot %s has %r elements, expected %r" % (k + slot, np.shape(sd[k + slot]),
                                                                                   tuple(self.variables[k].shape)))
        global_step = int(sd["global_step"]) if "global_step" in sd else None       # (converted before the first write too)
        for k, v in self.variables.items():
            if k in sd:
                v.copy_(torch.as_tensor(np.asarray(sd[k])).to(v.dtype).reshape(v.shape))
        if global_step is not None:
            self.istate[H.IST_GLOBAL_STEP] = global_step
        if load_optimizer:
            for k in slots:
                v = self.variables[k]
                self.adam_m[k].copy_(torch.as_tensor(np.asarray(sd[k + "/Adam"])).to(v.dtype).reshape(v.shape))
                self.adam_v[k].copy_(torch.as_tensor(np.asarray(sd[k + "/Adam_1"])).to(v.dtype).reshape(v.shape))
        self.shadow_stale = True
