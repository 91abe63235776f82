"""AIRModel on MI355X -- host side of the Attend-Infer-Repeat hot path.

Mirrors the constructor and output attributes of the reference class
(/root/reference/air/air_model.py:11-92, outputs :568-611, train op :651-694)
but executes the per-timestep loop as hand-written HIP kernels behind the C ABI
of libair_hip.so (include/air_hip.h).  PyTorch is used for device memory,
streams and torch.distributed only; there is no torch autograd, no torch math
and NO CPU fallback on this path.

Differences forced by the runtime (TF1 graph/session -> eager device buffers):
  * ``input_images`` / ``target_num_digits`` are device tensors that act as the
    placeholders: the kernels read them in place every time the model runs;
  * output attributes are device tensors refreshed by ``forward()`` /
    ``training()`` (``training`` is the callable train op, reference :692);
  * the loop runs a fixed ``max_steps`` iterations (numerically identical to the
    reference's early exit); the stacked ``rec_*`` outputs
    are sliced to the T' <= max_steps iterations the reference would have run;
  * every RNG op of the reference graph is unseeded; here noise comes from a
    device Philox stream (``seed``) or is injected with ``set_noise`` (parity).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _hip as H
from . import summaries as _summaries
from ._generate import GeneratedScenes, Generator, st_matrices
from ._hip import GEMM_PRECISION, ptr as _ptr
from ._store import (VariableStore, _SCOPES, _align8, reset_default_graph,  # noqa: F401  -- (re-exported: every name
                     saved_cnn_arguments, xavier_uniform_)                  # callers read from this module stays here)

_st_matrices = st_matrices      # (the name this module had for it)

# The sampler-backward order the training driver and the benchmark run (training.py, bench.py).  Round 6 gated the schedule
# ("reference", "reference_carried", N) -- the reference graph's own accumulation order up to iteration N, the faster carried
# order after it -- on 48 seeds x 60 000 iterations per precision and switch point (N = 2 000 .. 20 000): no N keeps the
# reference order's success rate within that window in both precisions (a run resting on the 0.67 plateau at the switch leaves
# it later; over the full 276 300 iterations the two end alike), so the reference's order stays the default for every iteration
# and schedules stay opt-in.
TRAINING_BACKWARD = "reference"

_ANNEALABLE = {
    "z_pres_prior_log_odds": H.DYN_PRIOR_LOG_ODDS, "z_pres_temperature": H.DYN_TEMPERATURE,
    "stopping_threshold": H.DYN_STOP_THRESHOLD, "learning_rate": H.DYN_LEARNING_RATE,
    "gradient_clipping_norm": H.DYN_CLIP_NORM,
    "scale_prior_mean": H.DYN_SCALE_PM, "scale_prior_variance": H.DYN_SCALE_PV,
    "shift_prior_mean": H.DYN_SHIFT_PM, "shift_prior_variance": H.DYN_SHIFT_PV,
    "vae_prior_mean": H.DYN_VAE_PM, "vae_prior_variance": H.DYN_VAE_PV,
}


class _Op:
    """One enqueued C-ABI call: callable(stream) + algorithmic bytes/flops for rooflines."""
    __slots__ = ("name", "fn", "nbytes", "flops", "kernel")

    def __init__(self, name, fn, nbytes=0, flops=0, kernel=None):
        self.name, self.fn, self.nbytes, self.flops = name, fn, nbytes, flops
        self.kernel = kernel or name          # kernel function name as rocprofv3 prints it

    def __call__(self, stream):
        self.fn(stream)


def _enqueue(plan, stream):
    for op in plan:
        op(stream)


# Entry point of the library -> the kernel it launches, as rocprofv3 prints it: every entry point AIRModel._call takes
# (air_gemm's kernels come from air_gemm_kernel_name, _gemm).  A template names the instantiation by a model attribute,
# filled in by _call; None: the library names the kernel of the descriptor (air_*_kernel_name, _build_backward).
# tests/test_kernel_names.py holds every name against the symbols of the built library.
KERNEL_NAMES = {
    "air_step_begin": "step_begin_kernel",
    "air_lstm_first_step": "lstm_first_step_kernel<{slabs}>",           # <4> split-K slabs, or <0>: a run-time count
    "air_attend_fwd": "attend_fwd_kernel",
    "air_vae_bottleneck_fwd": "bottleneck_fwd_kernel<256, {twins}>",    # (bf16 path only) per operand form: bf16 twins or fp32
    "air_write_fwd": "write_fwd{gauss}_kernel<1024>",                   # (a __global__ per likelihood over one body)
    "air_finalize": "finalize_kernel",
    "air_write_bwd": None,
    "air_write_fwd_bwd": None,
    "air_vae_bottleneck_bwd": "bottleneck_bwd_kernel<256, {twins}>",
    "air_attend_bwd": "attend_bwd_kernel",
    "air_wgrad_grouped": "wgrad_grouped{bf16}_kernel",
    "air_colsum": "colsum_kernel",
    "air_grad_sqnorm": "grad_sqnorm_kernel",
    "air_adam_clip_step": "adam_clip_kernel",
    "air_adam_clip_step_panels": "adam_panels_kernel",
    "air_cnn_fwd": "cnn_fwd_kernel<{filters}>",
    "air_cnn_bwd_sq": "cnn_bwd_kernel<{filters}>",                      # (its second launch is cnn_reduce_sq_kernel)
    "air_philox_fill": "philox_fill_kernel",
    "air_scene_records": "scene_records_kernel",
    "air_render": "render_kernel",
    "air_glyph_distort": "glyph_distort_kernel",                        # (air.sources.DeviceHandwritingBank launches it)
    "air_localization": "loc_match_kernel",                             # (air.metrics.Localization; then loc_fold_kernel)
    "air_segmentation": "seg_image_kernel",                             # (air.metrics.Segmentation; then seg_fold_kernel)
    "air_scene_masks": "scene_masks_kernel",                            # (Segmentation.scene_masks)
    "air_latent_probe": "probe_pairs_kernel",                           # (air.metrics.LatentProbe; probe_valid / probe_moments
    #                                                                      before, probe_merge after; the *16_kernel pair for k > 8)
    "air_importance_logw": "iw_logw_kernel",                            # (air.metrics.ImportanceBound, once per sampled pass)
    "air_importance_fold": "iw_image_kernel",                           # (then iw_fold_kernel)
    "air_latent_kmeans": "kmeans_restart_kernel",                       # (air.metrics.LatentClusters; kmeans_valid before,
    #                                                                      kmeans_pick after)
}


def _step_lds(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld):
    """air_step_lds_t of these hyper-parameters: the library's own sizing functions answer (no GPU is touched)"""
    lds = H.StepLds()
    H.check(H.lib().air_step_lds(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld, C.byref(lds)), "air_step_lds")
    return lds


def step_lds_bytes(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld, literals=()):
    """Dynamic LDS, in bytes, of every launch of the step whose need grows with the hyper-parameters: [(launch, bytes)],
    as the functions that size the launches give it (air_step_lds, csrc/air_sampler_common.h).  `literals`: the
    air_write_bwd_t.literal values of the sampler-backward orders a train model runs (none for a test model)."""
    lds = _step_lds(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld)
    need = [("air_attend_fwd", lds.attend_fwd), ("air_write_fwd", lds.write_fwd), ("air_render", lds.render)]
    if literals:
        need.append(("air_attend_bwd", lds.attend_bwd))
    for lit in sorted(set(literals)):
        need.append(("air_write_bwd (literal %d)" % lit, lds.write_bwd_graph) if lit >= 2 else
                    ("air_write_bwd (literal 0)", lds.write_bwd_exact))
    return need


def check_step_lds(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld, literals=()):
    """NotImplementedError when a launch of the step would need more LDS than a workgroup can hold"""
    limit = _step_lds(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld).limit
    for launch, nbytes in step_lds_bytes(max_steps, canvas_size, windows_size, Hs, Hh, Hz, wout_ld, literals):
        if nbytes > limit:
            raise NotImplementedError(
                "canvas_size = %d with max_steps = %d and windows_size = %d exceeds the HIP path's limits: %s would need %d bytes of "
                "LDS per workgroup, a workgroup holds %d (the taps and windows of all steps of an image, or a whole canvas, "
                "live in LDS) -- reduce canvas_size or max_steps" % (canvas_size, max_steps, windows_size, launch, nbytes, limit))


# the weight-gradient problems AIRModel._build_wgrad appends beside the VAE's: Wh, whid, wout (head pack), Wx
_NON_VAE_WGRAD_PROBLEMS = 4
_NOISE_KEYS = ("eps_scale", "eps_shift", "eps_z", "eps_x", "u")


def _carve_noise(normals, uniforms, N, B, Z, d):
    """(eps_scale [N,B,1], eps_shift [N,B,2], eps_z [N,B,Z], eps_x [N,B,d], u [N,B]): views of one normals / uniforms pair
    (one contiguous buffer each: one Philox launch fills them)"""
    sizes = (N * B, 2 * N * B, N * B * Z, N * B * d)
    assert normals.numel() == sum(sizes) and uniforms.numel() == N * B
    es, exy, ez, ex = torch.split(normals, sizes)
    return es.view(N, B, 1), exy.view(N, B, 2), ez.view(N, B, Z), ex.view(N, B, d), uniforms.view(N, B)


def _row16(t, i):
    """block i of a bf16 twin buffer (None when the twins are off)"""
    return None if t is None else t[i]


def _copy_noise(noise, dst):
    """copies the five noise tensors of the dict `noise` (tensors or arrays) into the buffers dst(key)"""
    for k in _NOISE_KEYS:
        buf = dst(k)
        buf.copy_(torch.as_tensor(np.asarray(noise[k]), dtype=torch.float32).reshape(buf.shape))


class AIRModel:

    def __init__(self, input_images, target_num_digits,
                 max_steps=3, max_digits=2, rnn_units=256, canvas_size=50, windows_size=28,
                 vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                 scale_prior_mean=-1.0, scale_prior_variance=0.1, shift_prior_mean=0.0, shift_prior_variance=1.0,
                 vae_prior_mean=0.0, vae_prior_variance=1.0, vae_likelihood_std=0.3,
                 scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                 z_pres_prior_log_odds=-2.0, z_pres_temperature=1.0, stopping_threshold=0.99,
                 learning_rate=1e-3, gradient_clipping_norm=100.0, cnn=None, cnn_filters=8,
                 num_summary_images=60, train=False, reuse=False, scope="air",
                 annealing_schedules=None, seed=0, gemm_precision=None, backward="reference", noise_seed=None,
                 bf16_twins=None, dp_exchange=None, xw_tile=None, xwx_twin_staging="lds_dma", step0_fusion=None,
                 compose_fold=True, likelihood="bernoulli"):
        if cnn is None:
            # The reference's default is cnn=True (:21) and every caller of the reference passes cnn=False.  A call that leaves
            # `cnn` out has always been refused here, and still is: which LSTM input a model has (and with it the layout of
            # its variables and checkpoints) is chosen by the caller, not met by accident.  cnn=True builds the front-end.
            raise NotImplementedError("pass cnn explicitly: cnn=True (the reference's default: the conv front-end in front of the "
                                      "LSTM) or cnn=False (what the reference's training.py, demo.py and embeddings.py pass)")
        if not (torch.is_tensor(input_images) and input_images.is_cuda):
            raise H.AirHipError("input_images must be a CUDA/HIP device tensor: this path has no CPU fallback")
        self.lib = H.lib()
        self.input_images = input_images
        self.target_num_digits = target_num_digits
        self.batch_size = int(input_images.shape[0])
        # the shape limits of the kernels, checked HERE with the limit in the message (a caller never meets them as an
        # error code of a launch): include/air_hip.h.  The LDS each launch needs follows below, once the backward order is
        # known (check_step_lds)
        limits = (("max_steps", max_steps, 16, "the per-image records of the compose / attend kernels hold 16 steps"),
                  ("windows_size", windows_size, 32, "the sampler backward gives every glimpse pixel a thread of a 1024-thread workgroup"),
                  # (the VAE's products beside its two fixed ones, ml and out: VaeLayers.products)
                  ("len(vae_recognition_units) + len(vae_generative_units)", len(vae_recognition_units) + len(vae_generative_units),
                   H.MAX_WGRAD_PROBLEMS - _NON_VAE_WGRAD_PROBLEMS - 2,
                   "the grouped weight-gradient launch takes %d problems" % H.MAX_WGRAD_PROBLEMS))
        for name, val, cap, why in limits:
            if val > cap:
                raise NotImplementedError("%s = %d exceeds the HIP path's limit of %d (%s)" % (name, val, cap, why))
        # the pixel likelihood of the reconstruction loss (air_write_fwd_t.likelihood, include/air_hip.h): "bernoulli", the
        # reference's cross-entropy on the clipped canvas (:586-589), or "gaussian", the AIR paper's Gaussian around the
        # clipped canvas with the fixed standard deviation vae_likelihood_std.  A per-model argument, not part of the
        # variable scope's shapes: it owns no variable, so a checkpoint of either kind loads into either.
        if likelihood not in self._LIKELIHOODS:
            raise ValueError("likelihood must be one of %s" % sorted(self._LIKELIHOODS))
        if likelihood == "gaussian" and not float(vae_likelihood_std) > 0.0:
            raise ValueError("likelihood='gaussian' needs vae_likelihood_std > 0, got %r" % (vae_likelihood_std,))
        self.likelihood = likelihood
        cnn = bool(cnn)
        if cnn:
            # the conv front-end (reference :510-533): the limits of its kernels, as the library answers them
            rc = self.lib.air_cnn_workspace_floats(self.batch_size, int(canvas_size), int(cnn_filters))
            if rc == H.ELIMIT:
                raise NotImplementedError("cnn=True: canvas_size = %d with cnn_filters = %d exceeds the HIP path's limits (cnn_filters "
                                          "<= 8; canvas_size <= 77 at 8 filters .. <= 128 at 1 or 2: the planes of an image live "
                                          "in LDS)" % (canvas_size, cnn_filters))
            if rc < 0:
                raise ValueError("cnn=True needs canvas_size >= 4 and cnn_filters >= 1, got %d and %d" % (canvas_size, cnn_filters))

        self.max_steps = max_steps
        self.max_digits = max_digits
        self.rnn_units = rnn_units
        self.canvas_size = canvas_size
        self.windows_size = windows_size
        self.vae_latent_dimensions = vae_latent_dimensions
        self.vae_recognition_units = tuple(vae_recognition_units)
        self.vae_generative_units = tuple(vae_generative_units)
        self.scale_prior_mean = scale_prior_mean
        self.scale_prior_variance = scale_prior_variance
        self.shift_prior_mean = shift_prior_mean
        self.shift_prior_variance = shift_prior_variance
        self.vae_prior_mean = vae_prior_mean
        self.vae_prior_variance = vae_prior_variance
        self.vae_likelihood_std = vae_likelihood_std
        self.scale_hidden_units = scale_hidden_units
        self.shift_hidden_units = shift_hidden_units
        self.z_pres_hidden_units = z_pres_hidden_units
        self.z_pres_prior_log_odds = z_pres_prior_log_odds
        self.z_pres_temperature = z_pres_temperature
        self.stopping_threshold = stopping_threshold
        self.learning_rate = learning_rate
        self.gradient_clipping_norm = gradient_clipping_norm
        self.num_summary_images = num_summary_images
        self.cnn = cnn
        self.cnn_filters = cnn_filters
        self.train = train
        self.scope = scope
        self.annealing_schedules = annealing_schedules
        self.rnn_input = self.input_images            # reference :535 (cnn=True: the conv block's output, _alloc)
        # (the reference's var_summaries / grad_summaries lists of summary ops are the methods of that name here)
        self.num_summaries, self.img_summaries = [], []
        self._hist_plans = {}
        prec = gemm_precision or GEMM_PRECISION
        if prec not in ("fp32", "bf16"):
            raise ValueError("gemm_precision must be 'fp32' or 'bf16'")
        self.gemm_precision = prec
        # "reference": the sampler backward in the op order of the reference's saved graph
        #   (model/air-model.meta, executed node by node by tests/test_graph_exec.py): one fp32 accumulator per window
        #   pixel through the four concatenated Gather gradients (UnsortedSegmentSum order), AddN_10/11
        #   order for the coordinate gradients -- keeps the out-of-range rounding residue the
        #   reference's training signal carries; bit-identical to the graph at kernel level.
        # "reference_carried": the reference's order for every window pixel whose streams are short (all but the four corners
        #   and a few borders); the long streams in 16 chunks per tap, every chunk walked from a carried stand-in for the
        #   reference's accumulator, so that every add rounds at the reference's magnitude (the order tests call "carried16").
        # "exact": the mathematical adjoint (the fp64-gradient tests; the model does not learn to localise with it).
        # (first, second, N): `first` while global_step < N, `second` from then on -- e.g. ("reference", "reference_carried",
        #   5000): the reference's own order at the start of training, the faster carried order for the rest of the run.  The
        #   switch is made by training() between two steps (launch lists rebuilt, a captured graph captured again); forward
        #   outputs are not affected.  Opt-in: no switch iteration passed the learning gate of DESIGN.md section 11.1.
        self._schedule = None
        if isinstance(backward, (tuple, list)):
            if len(backward) != 3 or backward[0] not in self._ORDERS or backward[1] not in self._ORDERS or int(backward[2]) < 0:
                raise ValueError("a backward schedule is (first order, second order, switch iteration >= 0)")
            self._schedule = (backward[0], backward[1], int(backward[2]))
            backward = backward[0]
        if backward not in self._ORDERS:
            raise ValueError("backward must be one of %s or a (first, second, iteration) schedule" % sorted(self._ORDERS))
        self.backward = backward
        self._literal = self._ORDERS[backward]
        self._host_step = None                    # global_step as the host follows it (schedules only; None: read it once)
        self._capture_args = None
        self._prec = 1 if prec == "bf16" else 0
        # bf16 path: every GEMM operand also exists as a bf16 twin in memory (written by the producing kernel /
        # by Adam), so the GEMMs read 2-byte operands and convert nothing -- bit-identical results (the twin IS
        # the rounding the fp32-operand kernels apply on the way into LDS).  bf16_twins=False keeps fp32 operands.
        self._twins = (True if bf16_twins is None else bool(bf16_twins)) and self._prec == 1
        self._xw_tile_arg = xw_tile
        self._step0_fusion_arg = step0_fusion
        # (before the variables exist: a refused shape leaves no variable scope behind)
        self._dp_exchange = dp_exchange or os.environ.get("AIR_DP_EXCHANGE", "flat")
        if self._dp_exchange not in ("flat", "factors"):
            raise ValueError("dp_exchange must be 'flat' or 'factors'")
        if cnn and self._dp_exchange == "factors":
            # (the factors of dWx would be rnn_input and sum_t dgates; the conv gradients would still need the all-reduce)
            raise NotImplementedError("dp_exchange='factors' is not implemented for cnn=True; use dp_exchange='flat'")
        self._check_lds((self._schedule[:2] if self._schedule else (backward,)) if train else ())

        dev = input_images.device
        if tuple(input_images.shape) != (self.batch_size, canvas_size * canvas_size) or \
                input_images.dtype != torch.float32 or not input_images.is_contiguous():
            raise ValueError("input_images must be contiguous float32 [B, canvas_size**2]")
        if target_num_digits is None:
            self.target_num_digits = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)
        if self.target_num_digits.dtype != torch.int32 or tuple(self.target_num_digits.shape) != (self.batch_size,):
            raise ValueError("target_num_digits must be int32 [B]")

        hp = dict(canvas_size=canvas_size, windows_size=windows_size, rnn_units=rnn_units,
                  vae_latent_dimensions=vae_latent_dimensions,
                  vae_recognition_units=self.vae_recognition_units, vae_generative_units=self.vae_generative_units,
                  scale_hidden_units=scale_hidden_units, shift_hidden_units=shift_hidden_units,
                  z_pres_hidden_units=z_pres_hidden_units, cnn=cnn, cnn_filters=int(cnn_filters) if cnn else 0)
        # tf.variable_scope(scope, reuse=reuse), reference :68
        if reuse:
            if scope not in _SCOPES:
                raise ValueError("reuse=True but variable scope %r does not exist" % scope)
            self.store = _SCOPES[scope]
            if self.store.hp != hp:
                raise ValueError("variable scope %r was created with different shapes" % scope)
        else:
            if scope in _SCOPES:
                raise ValueError("variable scope %r already exists; pass reuse=True" % scope)
            self.store = _SCOPES[scope] = VariableStore(hp, dev, seed)
        self.variables = self.store.variables
        self.gradients = self.store.gradients

        # `seed` initialises the variables (identical on every data-parallel rank); `noise_seed`
        # (default: seed) keys the device Philox stream -- DP ranks pass different ones, otherwise
        # every shard would draw the same noise
        self._seed = (seed if noise_seed is None else noise_seed) + (0 if train else 7919)
        # data parallel, what crosses xGMI per step.  "flat" (default): ONE all_reduce of the whole flat gradient
        # (16 MB at the default shapes).  "factors": the LSTM input-weight gradient dWx = X^T.(sum_t dgates) -- 64 % of
        # the gradient elements, rank <= B per GPU -- is never reduced: its FACTORS (X and sum_t dgates, 0.9 MB per
        # rank) are all-gathered and every rank contracts the gathered rows itself; only the other 36 % is
        # all-reduced.  Same sum up to the fp32 order of the contraction (tests/test_gpu_dp.py).
        self._dp_factor_ops = None
        # test hook: run the data-parallel protocol (gradient exchange + separate norm pass + Adam) on a process group of
        # ONE rank -- all a 1-GPU box can give RCCL -- so that its captured form is exercised on hardware
        self._dp_force = os.environ.get("AIR_DP_FORCE") == "1"
        self._injected_noise = False
        # how the twin-operand x.Wx launch stages its panels: "lds_dma" (gemm_xwx_glds_kernel) or "registers" (the same
        # operands through VGPRs and ds_write, air_gemm_t.i0 bit 0): an A/B handle for the tools, results are bit-identical
        if xwx_twin_staging not in ("lds_dma", "registers"):
            raise ValueError("xwx_twin_staging must be 'lds_dma' or 'registers'")
        self._xwx_twin_staging = xwx_twin_staging
        # captured train steps run compose inside the write-backward launch where the library has that form
        # (air_write_fwd_bwd; same results); False keeps the two launches: the A/B arm within one build
        self._compose_fold = bool(compose_fold)
        self._fold_op = None
        self._graph = None
        self._dirty = True
        self._steps_executed = None
        self._generator = Generator(self)         # generate() / decode(): buffers + launch lists, built at their first call
        self._alloc()
        self._build_programs()

    # ------------------------------------------------------------------ buffers
    def _f32(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.input_images.device)

    def _i16(self, *shape):
        """a bf16 twin buffer (None when the twins are off)"""
        return torch.zeros(*shape, dtype=torch.int16, device=self.input_images.device) if self._twins else None

    def _alloc(self):
        st, dv = self.store, self.input_images.device
        dm = st.dims
        B, N = self.batch_size, self.max_steps
        D, d, R, Z, HT = dm["D"], dm["d"], dm["R"], dm["Z"], dm["HT"]
        Din = dm["Din"]                                      # the LSTM's input width: D, or the conv block's output
        f, h16 = self._f32, self._i16

        # dynamic scalars + annealing table (reference :76-82, 94-121)
        dyn = np.zeros(H.DYN_COUNT, np.float32)
        dyn[H.DYN_PRIOR_LOG_ODDS] = self.z_pres_prior_log_odds if not isinstance(self.z_pres_prior_log_odds, dict) else 0
        dyn[H.DYN_TEMPERATURE] = self.z_pres_temperature
        dyn[H.DYN_STOP_THRESHOLD] = self.stopping_threshold
        dyn[H.DYN_LEARNING_RATE] = self.learning_rate
        dyn[H.DYN_CLIP_NORM] = self.gradient_clipping_norm if self.gradient_clipping_norm is not None else 0.0
        dyn[H.DYN_SCALE_PM], dyn[H.DYN_SCALE_PV] = self.scale_prior_mean, self.scale_prior_variance
        dyn[H.DYN_SHIFT_PM], dyn[H.DYN_SHIFT_PV] = self.shift_prior_mean, self.shift_prior_variance
        dyn[H.DYN_VAE_PM], dyn[H.DYN_VAE_PV] = self.vae_prior_mean, self.vae_prior_variance
        dyn[H.DYN_LIK_STD] = self.vae_likelihood_std
        # tf.log of the constructor values, taken before any schedule replaces the attribute (:72-82)
        dyn[H.DYN_SCALE_PLV] = np.log(np.float32(self.scale_prior_variance))
        dyn[H.DYN_SHIFT_PLV] = np.log(np.float32(self.shift_prior_variance))
        dyn[H.DYN_VAE_PLV] = np.log(np.float32(self.vae_prior_variance))
        dyn[H.DYN_GRAD_SCALE] = 1.0 / B
        self.dyn = torch.from_numpy(dyn).to(dv)
        sched = []
        for param, s in (self.annealing_schedules or {}).items():
            if param not in _ANNEALABLE:
                raise NotImplementedError("annealing of %r is not supported on the HIP path" % param)
            flags = (H.SCHED_STAIRCASE if s.get("staircase", False) else 0) | \
                    (H.SCHED_HAS_MIN if "min" in s else 0) | (H.SCHED_HAS_MAX if "max" in s else 0) | \
                    (H.SCHED_LOG if s.get("log", False) else 0)
            sched.append((_ANNEALABLE[param], flags, s["init"], s["iters"], s["factor"],
                          s.get("min", 0.0), s.get("max", 0.0)))
        self._nsched = len(sched)
        arr = np.zeros(max(1, len(sched)), dtype=[("slot", "<i4"), ("flags", "<i4"), ("init", "<f4"),
                                                 ("iters", "<f4"), ("factor", "<f4"), ("vmin", "<f4"), ("vmax", "<f4")])
        for i, srow in enumerate(sched):
            arr[i] = srow
        self.sched = torch.from_numpy(arr.view(np.uint8).copy()).to(dv)

        # noise: normals then uniforms, one contiguous buffer each (one Philox launch)
        self.normals = f(N * B * (1 + 2 + Z + d))
        self.uniforms = f(N * B)
        self.eps_scale, self.eps_shift, self.eps_z, self.eps_x, self.u = _carve_noise(self.normals, self.uniforms, N, B, Z, d)

        # per-image results of the compose kernel (no running state lives across kernels any more)
        self.run_loss = f(B)
        self.run_digits = torch.zeros(B, dtype=torch.int32, device=dv)
        self.c = f(N + 1, B, R); self.h = f(N + 1, B, R)         # [0] stays zero (zero_state :540)

        # the hoisted x.Wx: 4 split-K slabs (the LSTM epilogues sum them); 32x32 tiles at D = 2500 (0.1977 ->
        # 0.1968 ms per step against 8 slabs), 64x32 for the 128x128 canvases (0.923 -> 0.898 ms) -- measured sweeps
        # (bf16 twins, large canvases: 64x64 tiles -- the image batch is re-read by 16 instead of 32 column tiles and the
        # row-major Wx shadow is fetched in whole 128-byte lines: [256x1024x16384] 59.6 -> 42.2 us, tools/exp/gemm_twin_bench.py)
        self._xw_ksplit, self._xw_tile = 4, ((2, 2) if Din <= 4096 else ((4, 4) if self._twins else (4, 2)))
        if self._twins and Din > 4096 and B % 64 == 0 and R % 16 == 0 and Din % 512 == 0:
            # full batches of a large canvas: the throughput tiling (64 x 64 per workgroup, 8 K-slabs), gemm_xw_tp_kernel
            self._xw_ksplit, self._xw_tile = 8, (8, 4)
        xw_tile = self._xw_tile_arg
        if xw_tile is not None:                              # (tile_m, tile_n, ksplit <= 8) in 16-row / 16-column units: the split-K
            tm_, tn_, ks_ = (int(v) for v in xw_tile)        # product on THAT tiling (tests: a common tiling for bit-identity)
            self._xw_ksplit, self._xw_tile = ks_, (tm_, tn_)
        # ONE launch computes x.Wx (no split-K) and, in its epilogue, the first LSTM step (zero state: no h.Wh) --
        # AIR_EPI_LSTM_FWD0 on four-unit x four-gate tiles.  On the row-major shadow of Wx such a tile reads 8-byte pieces
        # of every row (one sixteenth of each cache line it pulls through the CU): 16.0 us against 7.8 + 3.4 us for the
        # split-K product + the pointwise first step, which is why round 2 kept it off.  On the gate-interleaved PANEL twin
        # (VariableStore.panels) the tile's rows are 32 contiguous bytes: default for the bf16 path now (and for its
        # twins-off form, so that the two stay bit-identical); the fp32 path keeps the split-K product.
        # AIRModel(step0_fusion=False / True) forces it off / on, where the shape allows it.
        want0 = (self._prec == 1 and Din <= 4096) if self._step0_fusion_arg is None else bool(self._step0_fusion_arg)
        self._fuse_step0 = want0 and R % 4 == 0 and Din % 4 == 0 and xw_tile is None
        self._xw_slabs = 1 if self._fuse_step0 else self.lib.air_gemm_slabs(Din, self._xw_ksplit)
        self.xw = f(self._xw_slabs, B, 4 * R)            # x.Wx (split-K slabs when not fused)
        self.gates_pre = f(B, 4 * R)
        self.acts = f(N, B, 4 * R)
        self.hid = f(N, B, HT)
        self.out7 = f(N, B, H.OUT_STRIDE)
        self.att = f(N, B, H.ATT_STRIDE)
        self.window = f(N, B, d)
        self.rec_act = [f(N, B, u) for u in self.vae_recognition_units]
        self.ml = f(N, B, 2 * Z)
        # z rows are padded to a multiple of 4 (Z = 50 -> 52) where the fused bottleneck writes them (air_bottleneck_fwd_t.ldz):
        # the weight gradient of the first generative layer then reads z's twin in 8-byte pieces instead of taking the
        # fp32-operand tiles (35 -> 15 us for that problem at 128 x 128).  self.zs is the [N, B, Z] view either way.
        self._zs_ld = (Z + 3) & ~3
        self._zs_pad = f(N, B, self._zs_ld)
        self.zs = f(N, B, Z)
        self.gen_act = [f(N, B, u) for u in self.vae_generative_units]
        self.vrec = f(N, B, d)
        self._recon = f(B, D)
        self._rec_loss = f(B)
        self._loss_item = f(B)
        self.scalars = self.store.grads[self.store.n:self.store.n + 4] if self.train else f(4)
        # arrival count of air_write_fwd_bwd (the captured steps' compose + write backward launch): zero between launches
        self._arrive = torch.zeros(1, dtype=torch.int32, device=self.input_images.device) if self.train else None

        self.h16 = h16(N + 1, B, R)                     # [0] stays zero like h[0]
        self.hid16 = h16(N, B, HT)
        self.window16 = h16(N, B, d)
        self.rec_act16 = [h16(N, B, u) for u in self.vae_recognition_units]
        self.zs16 = h16(N, B, Z)
        self._zs16_pad = h16(N, B, self._zs_ld)
        self.gen_act16 = [h16(N, B, u) for u in self.vae_generative_units]
        self.images16 = None
        self.images16p = None
        if self.train:
            self.d_genpre16 = h16(N, B, d)
            self.d_gen16 = [h16(N, B, u) for u in self.vae_generative_units]
            self.d_ml16 = h16(N, B, 2 * Z)
            self.d_rec16 = [h16(N, B, u) for u in self.vae_recognition_units]
            self.d_hid16 = h16(N, B, HT)
            self.dgates16 = h16(N, B, 4 * R)
            self.dgsum16 = h16(B, 4 * R)
            # twin of the LSTM's input (the caller's fp32 image batch, or rnn_input): written by the step prologue, read by the
            # input-weight gradient
            self.images16 = h16(B, Din)
            # a SECOND twin of the batch with rows padded to a multiple of 8 elements (every row 16-byte aligned, pad
            # columns zero): side output of the fp32-operand x.Wx launch, A operand of the x.Wx launches that follow it
            # inside one captured replay (capture_graph)
            # (not with the conv front-end: the LSTM's input is recomputed by every step)
            self.images16p = None if self.cnn else h16(B, (Din + 7) & ~7)
        if self.train:
            self.d_recon = f(B, D)
            self.d_genpre = f(N, B, d)
            self.d_gen = [f(N, B, u) for u in self.vae_generative_units]
            self.d_ml = f(N, B, 2 * Z)
            self.d_rec = [f(N, B, u) for u in self.vae_recognition_units]
            self.d_window = f(N, B, d)
            self.d_sxyw = f(N, B, 4)
            self.dh_heads = f(N, B, R)
            self.d_hid = f(N, B, HT)
            self.d_out7 = f(N, B, H.OUT_STRIDE)
            self.dh_cur = f(B, R)                       # scratch C of the fused LSTM-backward GEMM
            self.dc = [f(B, R), f(B, R)]
            self.dgates = f(N, B, 4 * R)
            self.dgsum = f(B, 4 * R)
        if self.cnn:
            # the conv front-end (reference :510-533): its output is the LSTM's input; a train model keeps what the backward
            # reads (the pooled planes and their argmax codes) and the per-image partials of the six gradients
            S, F = self.canvas_size, self.cnn_filters
            self.rnn_input = f(B, Din)
            self._cnn_saved = (None,) * 4
            if self.train:
                u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=dv)
                S1, S2 = S // 2, S // 4
                self._cnn_saved = (f(B, S1, S1, F), f(B, S2, S2, F), u8(B, S1, S1, F), u8(B, S2, S2, F))
                self._cnn_ws = f(int(self.lib.air_cnn_workspace_floats(B, S, F)))
                self.d_rnn_input = f(B, Din)

    # ------------------------------------------------------------- launch lists
    def _gemm(self, A, Bm, Cm, M, N, K, lda, ldb, ldc, ta=0, tb=0, bias=None, addend=None, ldadd=0,
              aux=None, ldaux=0, aux_scale=0.0, act=H.ACT_NONE, actgrad=H.GRAD_NONE, accumulate=0, tag="gemm",
              epi=H.EPI_GENERIC, tile=(0, 0), ksplit=0, addend_slabs=0, i0=0, p=(), q=(), extra_bytes=0, step_job=None,
              A16=None, B16=None, C16=None, q0_16=None, q2_16=None, B16p=None):
        p = list(p) + [None] * (4 - len(p))
        q = list(q) + [None] * (3 - len(q))
        g = H.Gemm(A=_ptr(A), B=_ptr(Bm), C=_ptr(Cm), M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, transA=ta, transB=tb,
                   bias=_ptr(bias), addend=_ptr(addend), ldadd=ldadd, aux=_ptr(aux), ldaux=ldaux, aux_scale=aux_scale,
                   act=act, actgrad=actgrad, accumulate=accumulate, precision=self._prec,
                   epi=epi, tile_m=tile[0], tile_n=tile[1], ksplit=ksplit, addend_slabs=addend_slabs, i0=i0,
                   p0=_ptr(p[0]), p1=_ptr(p[1]), p2=_ptr(p[2]), p3=_ptr(p[3]), q0=_ptr(q[0]), q1=_ptr(q[1]), q2=_ptr(q[2]),
                   step_job=C.pointer(step_job) if step_job is not None else None,
                   A16=_ptr(A16), B16=_ptr(B16), C16=_ptr(C16), q0_16=_ptr(q0_16), q2_16=_ptr(q2_16), B16p=_ptr(B16p))
        fn = self.lib.air_gemm
        kbuf = C.create_string_buffer(96)
        H.check(self.lib.air_gemm_kernel_name(C.byref(g), kbuf, 96), "air_gemm_kernel_name")
        extra = (addend is not None) * max(1, addend_slabs) + (aux is not None) + (1 if accumulate else 0)
        return _Op("%s[%dx%dx%d%s]" % (tag, M, N, K, "t" if ta else ("n" + ("t" if tb else "n"))),
                   lambda s, g=g, fn=fn, keep=step_job: H.check(fn(C.byref(g), s), "air_gemm"),
                   nbytes=(2 if A16 is not None else 4) * M * K + (2 if (B16 is not None or B16p is not None) else 4) * K * N
                   + 4 * M * N * (1 + extra) + (0 if C16 is None else 2 * M * (((K + 7) & ~7) if epi == H.EPI_LSTM_FWD0 else N))
                   + (4 * N if bias is not None else 0) + extra_bytes,
                   flops=2 * M * N * K, kernel=kbuf.value.decode())

    def _call(self, name, *args, nbytes=0, flops=0, tag=None):
        fn = getattr(self.lib, name)
        kernel = KERNEL_NAMES[name]
        if kernel is not None:
            kernel = kernel.format(slabs=4 if self._xw_slabs == 4 else 0, twins="true" if self._twins else "false",
                                   bf16="_bf16" if self._prec else "", filters=self.cnn_filters,
                                   gauss="_gauss" if self.likelihood == "gaussian" else "")
        return _Op(tag or name, lambda s, fn=fn, args=args, name=name: H.check(fn(*args, s), name),
                   nbytes=nbytes, flops=flops, kernel=kernel)

    # bf16 twins of the weights (None when the twins are off): the activations carry their own twin buffers
    def _T(self, name):
        """the row-major bf16 shadow of a fused variable"""
        return self.store.P16[name] if self._twins else None

    def _TP(self, name):
        """its panel-blocked twin (forward products only; None for a matrix the store built no panel of: row-major shadow)"""
        return self.store.panel(name) if self._twins else None

    def _lstm_weights(self):
        """(Wx, Wh, Wx16, Wh16): the input and the recurrent rows of the LSTM kernel and of its row-major bf16 shadow"""
        Din, K = self.store.dims["Din"], self.store.P["lstm_kernel"]
        K16 = self._T("lstm_kernel")
        return (K[:Din], K[Din:]) + ((K16[:Din], K16[Din:]) if K16 is not None else (None, None))

    def _generative_ops(self, x, x16, act, act16, out, eps_x, aux_scale, first=0):
        """The generative layers from index `first` on and gen_mean (vae.py:26-41), reading x (twin x16), the input of layer
        `first`: softplus layers into act[i] / act16[i], then sigmoid(. + aux_scale * eps_x) into out.  The forward and the
        generation lists are built from this one set of descriptors."""
        P, T, TP, L = self.store.P, self._T, self._TP, self.store.vae_layers
        NB = self.max_steps * self.batch_size
        ops = []
        for i in range(first, len(L.gen)):
            l = L.gen[i]
            ops.append(self._gemm(x, P[l.w], act[i], NB, l.N, l.K, l.K, l.N, l.N,
                                  bias=P[l.b], act=H.ACT_SOFTPLUS, tag="vae_gen",
                                  A16=x16, B16=T(l.w), C16=act16[i], B16p=TP(l.w)))
            x, x16 = act[i], act16[i]
        l = L.out
        ops.append(self._gemm(x, P[l.w], out, NB, l.N, l.K, l.K, l.N, l.N, bias=P[l.b],
                              act=H.ACT_SIGMOID_NOISE, aux=eps_x, ldaux=l.N, aux_scale=aux_scale, tag="vae_out",
                              A16=x16, B16=T(l.w), B16p=TP(l.w)))
        return ops

    def _build_programs(self):
        self._keep = []                 # ctypes structs referenced by the closures
        self._build_forward()
        if not self.train:
            self._bwd, self._opt, self._wgrad_plain = [], [], None
            return
        self._build_wgrad()
        self._build_backward()
        self._opt = None
        self._opt_world = None

    def _build_forward(self):
        st, P, L = self.store, self.store.P, self.store.vae_layers
        dm = st.dims
        B, N = self.batch_size, self.max_steps
        D, d, R, Z, HT = dm["D"], dm["d"], dm["R"], dm["Z"], dm["HT"]
        Hs, Hh, Hz, Hmax = dm["Hs"], dm["Hh"], dm["Hz"], dm["Hmax"]
        Cc, w = self.canvas_size, self.windows_size
        tw, T, TP = self._twins, self._T, self._TP
        Wx, Wh, Wx16, Wh16 = self._lstm_weights()
        imgs = self.input_images                # the canvas side: attend, compose
        xin, Din = self.rnn_input, dm["Din"]    # the LSTM side: the same tensor unless the conv front-end is on
        keep = self._keep

        NB = N * B
        fwd = []
        self._xwx_twin_op = None
        # the conv front-end, an op of its own IN FRONT of the list (self._fwd[0] stays the x.Wx launch): fp32 in both precisions
        self._cnn_fwd = None
        if self.cnn:
            S, F = self.canvas_size, self.cnn_filters
            cv = [P[k] for k in st.cnn_names]
            cf = H.CnnFwd(_ptr(imgs), *[_ptr(v) for v in cv], _ptr(xin), *[_ptr(t) for t in self._cnn_saved], B, S, F)
            keep.append(cf)
            self._cnn_fwd = self._call("air_cnn_fwd", C.byref(cf), nbytes=4 * (B * (D + Din) + sum(v.numel() for v in cv)),
                                       flops=2 * 25 * B * F * (S * S + F * ((S // 2) ** 2 + (S // 4) ** 2)), tag="cnn_fwd")
        self._generator.drop_ops()              # (the generation launch lists are rebuilt with these; its buffers stay)

        def gemm(*args, **kw):
            fwd.append(self._gemm(*args, **kw))

        def xwx(tag, lda=Din, **kw):                # one form of the x.Wx launch (lda: the row stride of the A16 twin given)
            return self._gemm(xin, Wx, self.xw, B, 4 * R, Din, lda, 4 * R, 4 * R, tag=tag, **kw)
        # hoisted x.W_x (the reference recomputes it every step, :286); split-K slabs
        job = H.StepJob(_ptr(self.sched), self._nsched, _ptr(self.dyn), _ptr(st.istate),
                        _ptr(self.normals), self.normals.numel(), _ptr(self.uniforms), self.uniforms.numel(),
                        self._seed, _ptr(xin if self.images16 is not None else None), _ptr(self.images16),
                        xin.numel() if self.images16 is not None else 0)
        noise_bytes = 4 * (self.normals.numel() + self.uniforms.numel())
        if tw and st.wx_exclusive and not self._fuse_step0:
            # the store keeps ONLY the panel twin of Wx (VariableStore: "exclusive"), and this model cannot read it: its
            # largest operand is converted from fp32 inside the kernel -- correct, and a silent perf cliff otherwise
            import warnings
            warnings.warn("AIRModel(scope=%r): bf16 twins are on but x.Wx reads the fp32 Wx (the scope's store maintains only the "
                          "panel twin of Wx; this model does not fuse the first step: xw_tile or step0_fusion=False given?)"
                          % self.scope, RuntimeWarning, stacklevel=4)
        if self._fuse_step0:
            # the first step rides in the x.Wx launch: h_0 = c_0 = 0 (zero_state, :540), so its gates are x.Wx + b
            # (twins: the panel twin of Wx is the ONLY bf16 form of Wx that is maintained when the store made it exclusive)
            wx_pan = TP("Wx")
            step0 = dict(bias=P["lstm_bias"], epi=H.EPI_LSTM_FWD0, q=(self.acts[0], self.c[1], self.h[1]),
                         extra_bytes=4 * B * R * 6, q2_16=_row16(self.h16, 1), B16p=wx_pan,
                         B16=(Wx16 if (wx_pan is None and not st.wx_exclusive) else None))
            # (panel twin + train: the launch also leaves the padded bf16 twin of the batch behind -- air_gemm_t.C16 of this
            # epilogue -- and a second op reads it in place of the fp32 batch: capture_graph decides where that is allowed)
            # Only the bf16-twin kernel of this launch writes the twin, and only it has the twin-operand form (R % 8 == 0, a
            # 16-byte aligned batch, ...: twin_rounds in csrc/air_gemm_bf16.hip).  The library is asked, not second-guessed:
            # the plain descriptor is built first, and the twin is offered only where THAT dispatches to the twin kernel.
            op0 = xwx("xWx+lstm0", **step0)
            # (not with the conv front-end: its output changes with every step of a replay, so no step may read a twin an
            # earlier step left behind -- every x.Wx launch is the fp32-operand one)
            if wx_pan is not None and self.train and not self.cnn and op0.kernel.startswith("gemm_bf16tw_kernel<1, 1, false, %d, true," % H.EPI_LSTM_FWD0):
                x16p = self.images16p
                op0 = xwx("xWx+lstm0", C16=x16p, **step0)
                self._xwx_twin_op = xwx("xWx16+lstm0", lda=x16p.shape[1], A16=x16p,
                                        i0=(3 if self._xwx_twin_staging == "registers" else 2), **step0)
            fwd.append(op0)
            step0["extra_bytes"] += noise_bytes
            self._begin_host = (0, xwx("xWx+lstm0+step_begin", step_job=job, **step0))
        else:
            if st.wx_exclusive:
                Wx16 = None         # (the row-major shadow of Wx is not maintained on this scope: fp32 operand)
            plain = dict(ksplit=self._xw_ksplit, tile=self._xw_tile, B16=Wx16)
            fwd.append(xwx("xWx", **plain))
            # the same launch carrying the step prologue (schedules + Philox noise) as an extra plane of
            # workgroups: x.Wx reads neither, so the train step needs no prologue launch of its own
            self._begin_host = (0, xwx("xWx+step_begin", step_job=job, extra_bytes=noise_bytes, **plain))
            # step 0 starts from zero_state (:540): h_0 . Wh = 0, the gates are x.Wx + b -- a pointwise launch
            fwd.append(self._call("air_lstm_first_step", _ptr(self.xw), self._xw_slabs, _ptr(P["lstm_bias"]),
                                  _ptr(self.acts[0]), _ptr(self.c[1]), _ptr(self.h[1]), _ptr(_row16(self.h16, 1)), B, R,
                                  nbytes=4 * B * R * (4 * self._xw_slabs + 6) + 16 * R, tag="lstm_fwd0"))
        # the recurrence: the remaining LSTM steps, chained (the only sequential part of the loop -- the LSTM
        # sees the same image every step and nothing downstream feeds back into it, :286/:535)
        for t in range(1, N):
            lstm_kw = dict(bias=P["lstm_bias"], addend=self.xw, ldadd=4 * R, addend_slabs=self._xw_slabs,
                           epi=H.EPI_LSTM_FWD, p=(self.c[t],), q=(self.acts[t], self.c[t + 1], self.h[t + 1]),
                           extra_bytes=4 * B * R * 7, tag="lstm_fwd",
                           A16=_row16(self.h16, t), B16=Wh16, q2_16=_row16(self.h16, t + 1), B16p=TP("Wh"))
            gemm(self.h[t], Wh, self.gates_pre, B, 4 * R, R, R, 4 * R, 4 * R, **lstm_kw)
            if t == 1 and self._fuse_step0 and tw:
                # With the first step fused into it, x.Wx is ONE round of 160 KB of LDS per workgroup: prologue workgroups in
                # that launch would each take a whole CU.  The LSTM steps read neither the noise, nor dyn, nor the image
                # twin (their first consumer is attend_fwd): the prologue rides in the first of them instead (16 KB of LDS)
                lstm_kw = dict(lstm_kw, extra_bytes=lstm_kw["extra_bytes"] + noise_bytes, tag="lstm_fwd+step_begin")
                self._begin_host = (len(fwd) - 1, self._gemm(self.h[t], Wh, self.gates_pre, B, 4 * R, R, R, 4 * R, 4 * R,
                                                             step_job=job, **lstm_kw))
        # everything else runs ONCE over all N*B (step, image) rows
        gemm(self.h[1], P["whid"], self.hid, NB, HT, R, R, HT, HT, bias=P["bhid"],
             act=H.ACT_RELU, tag="heads_hid", A16=_row16(self.h16, 1), B16=T("whid"), C16=self.hid16, B16p=TP("whid"))
        a = H.AttendFwd(_ptr(self.hid), _ptr(P["wout"]), _ptr(P["bout"]), _ptr(imgs),
                        _ptr(self.eps_scale), _ptr(self.eps_shift), _ptr(self.u), _ptr(self.dyn),
                        _ptr(self.out7), _ptr(self.att), _ptr(self.window),
                        B, N, Cc, w, Hs, Hh, Hz, Hmax, 1 if self.train else 0, _ptr(self.window16))
        keep.append(a)
        fwd.append(self._call("air_attend_fwd", C.byref(a), nbytes=NB * ((D + d + HT) * 4 + 12), tag="attend_fwd"))
        x, x16 = self.window, self.window16
        for i, l in enumerate(L.rec):
            gemm(x, P[l.w], self.rec_act[i], NB, l.N, l.K, l.K, l.N, l.N,
                 bias=P[l.b], act=H.ACT_SOFTPLUS, tag="vae_rec",
                 A16=x16, B16=T(l.w), C16=self.rec_act16[i], B16p=TP(l.w))
            x, x16 = self.rec_act[i], self.rec_act16[i]
        # the bottleneck (last recognition product -> reparameterised sample -> first generative layer) is
        # ONE launch where the fused kernel's limits hold (bf16 operands; vae.py:16-30); else two GEMMs
        # bf16 path: on.  fp32 path (the parity precision): OFF -- its exact-fp32 form is 3e-6 from the two launches (another
        # fp32 order of a K = 256 sum) and saves 7 us, but over 32 seeds x 60 k iterations 4 runs never separate one count
        # class with it against 0 of 32 with two launches (profiles/r04_seed_sweep_fp32_bottleneck_*, r05_sweep_fp32_bottleneck_*).
        # (the library keeps the exact-fp32 form of the two kernels, air_bottleneck_*_t.exact_fp32 = 1: the model does not use it)
        ml = L.ml
        fuse_f = self._prec == 1 and len(L.gen) >= 1 and ml.K == 256 and Z <= 64 and Z % 2 == 0 and L.gen[0].N % 4 == 0
        self._zs_fused = fuse_f
        if fuse_f:
            g0 = L.gen[0]
            self.zs = self._zs_pad[:, :, :Z]                 # (the sample lives in the padded rows)
            bf = H.BottleneckFwd(_ptr(x), _ptr(P[ml.w]), _ptr(P[ml.b]), _ptr(self.eps_z), _ptr(P[g0.w]),
                                 _ptr(P[g0.b]), _ptr(self.ml), _ptr(self._zs_pad), _ptr(self.gen_act[0]), NB, ml.K, Z, g0.N, ml.K,
                                 _ptr(self._zs16_pad), _ptr(self.gen_act16[0]), _ptr(x16), _ptr(T(ml.w)), _ptr(T(g0.w)),
                                 0, self._zs_ld)
            keep.append(bf)
            fwd.append(self._call("air_vae_bottleneck_fwd", C.byref(bf),
                                  nbytes=4 * (NB * (ml.K + 4 * Z + g0.N) + ml.K * 2 * Z + Z * g0.N),
                                  flops=2 * NB * (ml.K * 2 * Z + Z * g0.N), tag="vae_bottleneck"))
            fwd += self._generative_ops(self.gen_act[0], self.gen_act16[0], self.gen_act, self.gen_act16, self.vrec,
                                        self.eps_x, float(self.vae_likelihood_std), first=1)
        else:
            fwd.append(self._gemm(x, P[ml.w], self.ml, NB, ml.N, ml.K, ml.K, ml.N, ml.N, bias=P[ml.b],
                                  epi=H.EPI_REPARAM_FWD, p=(self.eps_z,), q=(self.zs,),
                                  extra_bytes=8 * NB * Z, tag="ml_reparam", q0_16=self.zs16))
            fwd += self._generative_ops(self.zs, self.zs16, self.gen_act, self.gen_act16, self.vrec,
                                        self.eps_x, float(self.vae_likelihood_std))
        # more (image, step) items than CUs: the graph-order write backward takes them longest first (one extra workgroup of
        # the compose launch sorts them; air_write_fwd_t.wb_order)
        self._wb_order = (torch.arange(NB, dtype=torch.int32, device=imgs.device)
                          if (self.train and self._literal >= 2 and 256 < NB <= 4096) else None)
        wf = H.WriteFwd(_ptr(self.vrec), _ptr(self.ml), _ptr(imgs), _ptr(self.dyn), _ptr(self.att),
                        _ptr(self._recon), _ptr(self._rec_loss), _ptr(self.d_recon if self.train else None),
                        _ptr(self.run_loss), _ptr(self.run_digits), _ptr(self._loss_item), B, N, Cc, w, Z, _ptr(self._wb_order),
                        self._LIKELIHOODS[self.likelihood])
        keep.append(wf)
        self._write_fwd_desc = wf
        fwd.append(self._call("air_write_fwd", C.byref(wf),
                              nbytes=NB * (d + 2 * Z) * 4 + B * D * 4 * (3 if self.train else 2), tag="compose_fwd"))
        # batch means: their own launch after a plain forward; inside air_write_bwd in a train step
        self._finalize = self._call("air_finalize", _ptr(self.run_loss), _ptr(self._rec_loss),
                                    _ptr(self.target_num_digits), _ptr(self.run_digits), _ptr(self._loss_item),
                                    _ptr(self.scalars), B)
        self._fwd = fwd
        twin_job = ((_ptr(xin), _ptr(self.images16), xin.numel()) if self.images16 is not None else (None, None, 0))
        self._begin_sched_only = self._call(
            "air_step_begin", _ptr(self.sched), self._nsched, _ptr(self.dyn), _ptr(st.istate),
            None, 0, None, 0, C.c_uint64(self._seed), *twin_job)

    def _build_wgrad(self):
        """The weight-gradient problems: dW = A^T . dY for every variable; weights are shared across the time steps, so
        every dW contracts over all N*B rows, the LSTM input weights over sum_t dgates.  Order = tile numbering = order
        of the global-norm partials."""
        # (Round 4 let the VAE tiles RIDE as trailing workgroups of dh_heads and the BPTT steps -- their operands exist once
        # the data gradient has reached the glimpse.  Bit-identical, and slower: 0.1912 vs 0.1762 ms per step, 0.86 vs 0.70
        # at 128 x 128 -- a launch lasts as long as its slowest workgroup, a K = 192 tile needs 5.5 us, the carriers 3-4 us.
        # Removed)
        st, G, L = self.store, self.store.G, self.store.vae_layers
        dm = st.dims
        B, NB = self.batch_size, self.max_steps * self.batch_size
        Din, R, HT = dm["Din"], dm["R"], dm["HT"]
        Gx, Gh = G["lstm_kernel"][:Din], G["lstm_kernel"][Din:]
        probs = []

        def wg(A, dY, dW, db, M, Nn, K, A16=None, dY16=None, lda=None):
            probs.append(H.Wgrad(A=_ptr(A), dY=_ptr(dY), dW=_ptr(dW), db=_ptr(db), M=M, N=Nn, K=K, lda=lda or M, ldb=Nn, ldc=Nn,
                                 A16=_ptr(A16), dY16=_ptr(dY16)))
        wg(self.h[0], self.dgates, Gh, None, R, 4 * R, NB, _row16(self.h16, 0), self.dgates16)
        wg(self.h[1], self.d_hid, G["whid"], G["bhid"], R, HT, NB, _row16(self.h16, 1), self.d_hid16)
        # the VAE's products in layer order: the input of each (the fused bottleneck leaves z in padded rows) and the
        # gradient of its pre-activation
        z, z16, zl = (self._zs_pad, self._zs16_pad, self._zs_ld) if self._zs_fused else (self.zs, self.zs16, None)
        xs = [(self.window, self.window16)] + list(zip(self.rec_act, self.rec_act16)) + \
             [(z, z16)] + list(zip(self.gen_act, self.gen_act16))
        dys = list(zip(self.d_rec, self.d_rec16)) + [(self.d_ml, self.d_ml16)] + \
              list(zip(self.d_gen, self.d_gen16)) + [(self.d_genpre, self.d_genpre16)]
        for l, (x, x16), (dy, dy16) in zip(L.products(), xs, dys):
            wg(x, dy, G[l.w], G[l.b], l.K, l.N, NB, x16, dy16, lda=(zl if l is L.decoder[0] else None))
        probs.append(H.Wgrad(A=_ptr(self.d_out7), dY=_ptr(self.hid), dW=_ptr(G["wout"]), db=_ptr(G["bout"]),
                             M=H.OUT_STRIDE, N=HT, K=NB, lda=H.OUT_STRIDE, ldb=HT, ldc=dm["Hmax"],
                             head_pack=1, Hs=dm["Hs"], Hh=dm["Hh"], Hz=dm["Hz"]))
        # the input-weight gradient contracts over B rows only (sum_t dgates): its many light
        # workgroups go LAST so that they fill the tail of the launch behind the K = N*B ones
        wg(self.rnn_input, self.dgsum, Gx, G["lstm_bias"], Din, 4 * R, B, self.images16, self.dgsum16)
        assert len(probs) == _NON_VAE_WGRAD_PROBLEMS + len(L.products()) <= H.MAX_WGRAD_PROBLEMS      # (constructor: the limit)
        arr = (H.Wgrad * len(probs))(*probs)
        self._keep.append(arr)
        self._wgrad_arr = arr

        # weight + bias grads of all variables: ONE grouped launch (weights are shared across the
        # time steps, so every dW contracts over all N*B rows; the LSTM input weights over sum_t dgates)
        wbytes = sum(4 * q.M * q.N + (2 if (q.A16 and q.dY16) else 4) * q.K * (q.M + q.N) for q in probs)
        wflops = sum(2 * q.M * q.N * q.K for q in probs)
        self._wgrad_plain = self._call("air_wgrad_grouped", arr, len(probs), self._prec, None, None,
                                       nbytes=wbytes, flops=wflops, tag="wgrad_grouped")
        # single-GPU train step: the same launch also leaves the global-norm partial sums and counts
        # the step, so no separate pass over the 16 MB gradient is needed before Adam
        self._wgrad_blocks = self.lib.air_wgrad_num_blocks(arr, len(probs))
        if self._wgrad_blocks <= 0:
            H.check(self._wgrad_blocks, "air_wgrad_num_blocks")
        # (the conv gradients come from a launch of their own: its partials sit directly behind this launch's)
        self._cnn_sq = self.lib.air_cnn_num_sq_partials(self.cnn_filters) if self.cnn else 0
        if self._cnn_sq < 0:
            H.check(self._cnn_sq, "air_cnn_num_sq_partials")
        if st.partials.numel() < self._wgrad_blocks + self._cnn_sq:
            raise NotImplementedError("weight-gradient launch of %d workgroups%s exceeds the partial-sum buffer"
                                      % (self._wgrad_blocks, " + %d of the conv gradients" % self._cnn_sq if self.cnn else ""))
        # (Adam rebuilding dWx = X^T.(sum_t dgates) from its factors instead of reading the stored 10 MB -- bit-identical, the
        # tiles rebuilt inside Adam cost ~7 us against ~1 us saved in this launch -- was an option until round 5: removed)
        self._wgrad_fused = self._call("air_wgrad_grouped", arr, len(probs), self._prec, _ptr(st.partials),
                                       _ptr(st.istate), nbytes=wbytes, flops=wflops, tag="wgrad_grouped")
        self._sqnorm = self._call("air_grad_sqnorm", _ptr(st.grads), st.n, _ptr(st.partials), _ptr(st.istate),
                                  nbytes=4 * st.n, tag="grad_sqnorm")

    def _build_backward(self):
        st, P, L = self.store, self.store.P, self.store.vae_layers
        dm = st.dims
        B, N = self.batch_size, self.max_steps
        D, d, R, Z, HT = dm["D"], dm["d"], dm["R"], dm["Z"], dm["HT"]
        Hs, Hh, Hz, Hmax = dm["Hs"], dm["Hh"], dm["Hz"], dm["Hmax"]
        Cc, w = self.canvas_size, self.windows_size
        T = self._T
        _, Wh, _, Wh16 = self._lstm_weights()
        imgs, keep, NB = self.input_images, self._keep, N * B

        bwd = []
        lit = self._literal
        wb = H.WriteBwd(_ptr(self.d_recon), _ptr(self.vrec), _ptr(self.att), _ptr(self.d_genpre),
                        _ptr(self.d_sxyw), B, N, Cc, w, lit, None, None, None, None, _ptr(self.d_genpre16),
                        _ptr(self._wb_order))
        wbf = H.WriteBwd(_ptr(self.d_recon), _ptr(self.vrec), _ptr(self.att), _ptr(self.d_genpre),
                         _ptr(self.d_sxyw), B, N, Cc, w, lit, _ptr(self._loss_item), _ptr(self.target_num_digits),
                         _ptr(self.run_digits), _ptr(self.scalars), _ptr(self.d_genpre16), _ptr(self._wb_order))
        keep += [wb, wbf]
        kbuf = C.create_string_buffer(96)
        H.check(self.lib.air_write_bwd_kernel_name(C.byref(wb), kbuf, 96), "air_write_bwd_kernel_name")
        # (algorithmic bytes as SURVEY 8(d) counts them: the write's (d + D) * 4 + 16 again + 12 bytes of theta gradient = 13 164 per
        # (image, step) at 50 x 50 -- the bf16 twin and the second read of the window are traffic, not algorithm)
        bwd.append(self._call("air_write_bwd", C.byref(wb), nbytes=NB * ((D + d) * 4 + 16 + 12), tag="write_bwd"))
        self._write_bwd_fin = self._call("air_write_bwd", C.byref(wbf), nbytes=NB * ((D + d) * 4 + 16 + 12), tag="write_bwd")
        bwd[-1].kernel = self._write_bwd_fin.kernel = kbuf.value.decode()
        # compose + write backward (+ batch means) as one launch, for the captured steps: the library says whether this pair
        # of descriptors has that form (a refusal keeps the two launches; anything else is an error)
        self._fold_op = None
        if self._compose_fold:
            rc = self.lib.air_write_fwd_bwd_kernel_name(C.byref(self._write_fwd_desc), C.byref(wbf), kbuf, 96)
            if rc == 0:
                self._fold_op = self._call("air_write_fwd_bwd", C.byref(self._write_fwd_desc), C.byref(wbf), _ptr(self._arrive),
                                           nbytes=self._fwd[-1].nbytes + self._write_bwd_fin.nbytes - NB * D * 4,
                                           tag="compose_write_bwd")
                self._fold_op.kernel = kbuf.value.decode()
            elif rc not in (H.EINVAL, H.ELIMIT):
                H.check(rc, "air_write_fwd_bwd_kernel_name")

        def dgrad(l, dy, dy16, out, out16, saved=None, tag="dgrad_win"):
            """dX = dY . W^T of product l; times softplus'(saved activation X) where one is given"""
            bwd.append(self._gemm(dy, P[l.w], out, NB, l.K, l.N, l.N, l.N, l.K, tb=1, aux=saved,
                                  ldaux=l.K if saved is not None else 0,
                                  actgrad=H.GRAD_SOFTPLUS if saved is not None else H.GRAD_NONE, tag=tag,
                                  A16=dy16, B16=T(l.w), C16=out16))
            return out, out16
        # decoder data-grads over all N*B rows: decoder[i + 1] is the product that read the activation of gen[i]
        dy, dy16 = self.d_genpre, self.d_genpre16
        for i in reversed(range(len(L.gen))):
            dy, dy16 = dgrad(L.decoder[i + 1], dy, dy16, self.d_gen[i], self.d_gen16[i], self.gen_act[i], "dgrad_gen")
        fuse_b = self._prec == 1 and len(L.gen) >= 1 and len(L.rec) >= 1 and L.gen[0].N == 256 and Z <= 64 and Z % 2 == 0
        last_rec = len(L.rec)
        if fuse_b:
            # d_gen[0] -> d_z -> (d_mean | d_lv) -> d_rec[last] in ONE launch (vae.py:22-24 and the KL, backwards)
            g0, ml = L.gen[0], L.ml
            bb = H.BottleneckBwd(_ptr(dy), _ptr(P[g0.w]), _ptr(self.ml), _ptr(self.eps_z), _ptr(self.att), _ptr(self.dyn),
                                 _ptr(P[ml.w]), _ptr(self.rec_act[-1]), _ptr(self.d_ml), _ptr(self.d_rec[-1]),
                                 NB, ml.K, Z, g0.N, _ptr(self.d_ml16), _ptr(self.d_rec16[-1]),
                                 _ptr(dy16), _ptr(T(g0.w)), _ptr(T(ml.w)), 0)
            keep.append(bb)
            bwd.append(self._call("air_vae_bottleneck_bwd", C.byref(bb),
                                  nbytes=4 * (NB * (g0.N + 5 * Z + 2 * ml.K) + Z * g0.N + ml.K * 2 * Z),
                                  flops=2 * NB * (g0.N * Z + 2 * Z * ml.K), tag="vae_bottleneck_bwd"))
            dy, dy16, last_rec = self.d_rec[-1], self.d_rec16[-1], len(L.rec) - 1
        else:
            l = L.decoder[0]
            bwd.append(self._gemm(dy, P[l.w], self.d_ml, NB, l.K, l.N, l.N, l.N, 2 * Z, tb=1,
                                  epi=H.EPI_REPARAM_BWD, p=(self.ml, self.eps_z, self.att, self.dyn),
                                  extra_bytes=16 * NB * Z, tag="dz_reparam", C16=self.d_ml16))
            dy, dy16 = self.d_ml, self.d_ml16
        # ... and the encoder's: encoder[i + 1] is the product that read the activation of rec[i]
        for i in reversed(range(last_rec)):
            dy, dy16 = dgrad(L.encoder[i + 1], dy, dy16, self.d_rec[i], self.d_rec16[i], self.rec_act[i], "dgrad_rec")
        dgrad(L.encoder[0], dy, dy16, self.d_window, None)
        ab = H.AttendBwd(_ptr(self.hid), _ptr(P["wout"]), _ptr(imgs), _ptr(self.eps_scale),
                         _ptr(self.eps_shift), _ptr(self.dyn), _ptr(self.out7), _ptr(self.att),
                         _ptr(self.d_window), _ptr(self.d_sxyw), _ptr(self.d_hid), _ptr(self.d_out7),
                         B, N, Cc, w, Hs, Hh, Hz, Hmax, min(lit, 2), _ptr(self.d_hid16))
        keep.append(ab)
        bwd.append(self._call("air_attend_bwd", C.byref(ab), nbytes=NB * ((D + d + 2 * HT) * 4 + 64), tag="attend_bwd"))
        # heads' contribution to d loss / d h'[t] for every step
        # ... whose last-step rows go straight through the LSTM cell backward (start of the BPTT chain)
        tl = N - 1
        bwd.append(self._gemm(self.d_hid, P["whid"], self.dh_heads, NB, R, HT, HT, HT, R, tb=1,
                              epi=H.EPI_LSTM_BWD_TAIL, i0=tl * B,
                              p=(self.acts[tl], self.c[tl], self.c[tl + 1]),
                              q=(self.dgates[tl], self.dc[tl % 2], self.dgsum),
                              extra_bytes=4 * B * R * 15, tag="dh_heads", A16=self.d_hid16, B16=T("whid"),
                              q0_16=_row16(self.dgates16, tl), q2_16=(self.dgsum16 if N == 1 else None)))
        # back-propagation through time: the only sequential part of the backward
        for t in reversed(range(N - 1)):
            # d h'[t] = heads[t] + dgates[t+1] . Wh^T, LSTM pointwise backward fused in the epilogue
            bwd.append(self._gemm(self.dgates[t + 1], Wh, self.dh_cur, B, R, 4 * R, 4 * R, 4 * R, R, tb=1,
                                  addend=self.dh_heads[t], ldadd=R, epi=H.EPI_LSTM_BWD,
                                  p=(self.acts[t], self.c[t], self.c[t + 1], self.dc[(t + 1) % 2]),
                                  q=(self.dgates[t], self.dc[t % 2], self.dgsum), i0=1,
                                  extra_bytes=4 * B * R * 15, tag="bptt_lstm_bwd",
                                  A16=_row16(self.dgates16, t + 1), B16=Wh16, q0_16=_row16(self.dgates16, t),
                                  q2_16=(self.dgsum16 if t == 0 else None)))
        if self.cnn:
            # dgsum = sum_t dgates is complete: d loss / d rnn_input = dgsum . Wx^T (the row-major shadow of Wx on the twin path),
            # then the conv block's backward straight into the flat gradient buffer, with its global-norm partials
            Wx, _, Wx16, _ = self._lstm_weights()
            Din, S, F = dm["Din"], self.canvas_size, self.cnn_filters
            bwd.append(self._gemm(self.dgsum, Wx, self.d_rnn_input, B, Din, 4 * R, 4 * R, 4 * R, Din, tb=1,
                                  tag="dgrad_rnn_input", A16=self.dgsum16, B16=Wx16))
            cv, cg = [P[k] for k in st.cnn_names], [st.G[k] for k in st.cnn_names]
            cb = H.CnnBwd(_ptr(self.d_rnn_input), _ptr(self.rnn_input), _ptr(imgs), *[_ptr(t) for t in self._cnn_saved],
                          _ptr(cv[0]), _ptr(cv[2]), _ptr(cv[4]), _ptr(self._cnn_ws), *[_ptr(g) for g in cg], None, B, S, F)
            keep.append(cb)
            bwd.append(self._call("air_cnn_bwd_sq", C.byref(cb), _ptr(st.partials[self._wgrad_blocks:]),
                                  nbytes=4 * (B * (D + 2 * Din) + (B + 1) * sum(g.numel() for g in cg)), tag="cnn_bwd"))
        self._bwd = bwd

    # ------------------------------------------------------------------ running
    def _stream(self):
        return H.stream(self.input_images.device)

    def set_noise(self, noise):
        """Inject the noise tensors of one pass (parity tests): dict with eps_scale
        [N,B,1], eps_shift [N,B,2], eps_z [N,B,Z], eps_x [N,B,d], u [N,B]."""
        _copy_noise(noise, lambda k: getattr(self, k))
        self._injected_noise = True
        self._dirty = True

    _ORDERS = {"reference_carried": 4, "reference": 2, "exact": 0}      # air_write_bwd_t.literal
    _LIKELIHOODS = {"bernoulli": H.LIK_BERNOULLI, "gaussian": H.LIK_GAUSSIAN}      # air_write_fwd_t.likelihood

    def set_backward(self, backward):
        """Switches the sampler-backward order of a built train model (AIRModel(backward=...)): the launch lists are rebuilt,
        a captured graph is released and has to be captured again.  The variables, the Adam slots and global_step are
        untouched.  (training.py --late-backward: the reference's order while the out-of-range residue rules the gradient,
        a chunked order once ink is explained -- DESIGN.md section 10.1.)"""
        if backward not in self._ORDERS:
            raise ValueError("backward must be one of %s" % sorted(self._ORDERS))
        self._schedule = None                     # an explicit order ends a schedule
        self._set_order(backward)

    def _check_lds(self, orders):
        Hs, Hh, Hz = self.scale_hidden_units, self.shift_hidden_units, self.z_pres_hidden_units
        check_step_lds(self.max_steps, self.canvas_size, self.windows_size, Hs, Hh, Hz, max(Hs, Hh, Hz),
                       [self._ORDERS[o] for o in orders])

    def _set_order(self, backward):
        if backward == self.backward:
            return False
        self._check_lds((backward,))
        self.release_graph()
        self.backward = backward
        self._literal = self._ORDERS[backward]
        self._build_programs()
        return True

    @property
    def backward_schedule(self):
        """(first order, second order, switch iteration) or None"""
        return self._schedule

    def _follow_schedule(self, recapture=True):
        """AIRModel(backward=(first, second, N)): the order global_step asks for, before a train step is launched.  The host
        follows global_step by counting the steps it launches (one read of the device counter after construction / a
        checkpoint load); with a multi-step graph the switch happens at the first replay that starts at or after N."""
        if self._schedule is None:
            return
        if self._host_step is None:
            self._host_step = int(self.store.istate[H.IST_GLOBAL_STEP])
        first, second, n = self._schedule
        args = self._capture_args if self._graph is not None else None
        if self._set_order(first if self._host_step < n else second) and args is not None and recapture:
            self.capture_graph(**args)

    def use_device_rng(self, seed=None):
        if seed is not None:
            self._seed = seed
            self._build_programs()
        self._injected_noise = False

    def set_dynamic(self, **kw):
        """Overrides dynamic scalars (e.g. z_pres_prior_log_odds=-2.0) -- only meaningful
        for parameters without an annealing schedule."""
        plv = {"scale_prior_variance": H.DYN_SCALE_PLV, "shift_prior_variance": H.DYN_SHIFT_PLV,
               "vae_prior_variance": H.DYN_VAE_PLV}
        for k, v in kw.items():
            self.dyn[_ANNEALABLE[k]] = float(v)
            if k in plv:
                # an override of a prior variance is a new CONSTRUCTOR value, not a schedule: the log-variance the KL
                # uses (air_model.py:72-74, tf.log taken at construction) follows it; schedules leave that slot alone
                self.dyn[plv[k]] = float(np.log(np.float32(v)))
        self._dirty = True

    def _fresh_shadow(self):
        """bf16 shadow of the variables, re-derived (outside any captured graph) after a host-side change"""
        if self._twins and self.store.shadow_stale:
            self.store.refresh_shadow(self._stream())

    # The launch plans decide which built ops make up a forward, a backward, an update -- here and nowhere else.  They hand
    # out the built _Op objects, enqueue nothing and set nothing: the runners, the public lists and capture_graph read them.
    def _forward_plan(self, finalize=True, twin_x=False, fold=False, injected=None):
        """twin_x: x.Wx reads the padded bf16 twin of the image batch (capture_graph knows where an earlier step left it).
        fold: without the compose launch, the last of the list -- the backward that follows opens with air_write_fwd_bwd.
        injected (default: set_noise was called): the prologue is a launch of its own, the schedules only (parity tests)."""
        fwd = list(self._fwd[:-1] if fold else self._fwd)
        if twin_x:
            if self._xwx_twin_op is None:
                raise RuntimeError("this model has no twin-operand x.Wx launch")
            fwd[0] = self._xwx_twin_op
        head = [self._cnn_fwd] if self._cnn_fwd is not None else []   # (first: x.Wx and the prologue's bf16 twin read its output)
        if self._injected_noise if injected is None else injected:
            head.append(self._begin_sched_only)
        else:
            hi, hop = self._begin_host               # the launch that carries the prologue (schedules + Philox noise, as extra
            fwd[hi] = hop                            # workgroups) in the place of its plain form
        return head + fwd + ([self._finalize] if finalize else [])

    def _xwx_of(self, plan):
        """the x.Wx launch of a forward plan: the first behind the conv front-end and the schedules-only prologue"""
        i = int(self._cnn_fwd is not None)
        return plan[i + (plan[i] is self._begin_sched_only)]

    def _backward_plan(self, for_update=False, fused_finalize=False, fold=False, dp=None):
        """for_update: this backward is followed by the optimizer of a train step -- on a single GPU the weight-gradient
        launch then also publishes the global-norm partials and counts the step.  dp: self._dp() unless given.
        fold: the forward before it ran without its compose launch (_forward_plan): air_write_fwd_bwd opens the list."""
        first = self._fold_op if fold else (self._write_bwd_fin if fused_finalize else self._bwd[0])
        # (tried: the VAE weight gradients as their own launch on a side stream beside attend_bwd ->
        # dh_heads -> BPTT.  The big launch takes the CUs the latency-critical chain needs: 217 -> 257 us.)
        if for_update and not (self._dp() if dp is None else dp):
            tail = [self._wgrad_fused]
        elif for_update and self._dp_exchange == "factors":
            tail = [self._dp_factors()[k] for k in ("local", "bias")]
        else:
            tail = [self._wgrad_plain]
        return [first] + self._bwd[1:] + tail

    def _update_plan(self, dp=None):
        """global-norm clip + TF-style Adam + global_step += 1 (after the all-reduce); with the factor exchange
        dWx from the gathered factors first, identically on every rank"""
        factors = (self._dp() if dp is None else dp) and self._dp_exchange == "factors"
        return ([self._dp_factors()["dwx"]] if factors else []) + list(self._optimizer_ops())

    def forward_ops(self):
        """The launches of one uncaptured forward(), in order (profiling tools): the forward side of train_step_ops()."""
        return self._forward_plan()

    def train_step_ops(self):
        """The launches of one single-GPU train step on device noise, in order (bench / profiling tools): the EAGER step, whose
        x.Wx reads the caller's fp32 image batch.  Steps 1 .. G-1 of a captured G-step replay without a between_steps hook run
        the same list with the twin-operand x.Wx launch (gemm_xwx_glds_kernel, captured_xwx_kernels()) in its first place."""
        return self._forward_plan(finalize=False, twin_x=False, fold=False, injected=False) + \
            self._backward_plan(for_update=True, fused_finalize=True, fold=False, dp=False) + self._update_plan(dp=False)

    def _run_forward(self, s, finalize=True, twin_x=False, fold=False):
        self._fresh_shadow()
        _enqueue(self._forward_plan(finalize, twin_x, fold), s)

    def forward(self):
        """Evaluates the model on the current contents of the input buffers."""
        self._fresh_shadow()
        if self._graph is not None and not self.train and not self._injected_noise:
            self._graph[0].replay()
        else:
            self._run_forward(self._stream())
        self._dirty = False
        self._steps_executed = None
        return self

    def forward_sampled(self, call, seed=None):
        """One evaluation pass on FRESH noise (air.metrics.ImportanceBound): air_philox_fill under the key (seed or the
        model's seed, call) into the model's own noise buffers, then the forward launches that read them as given.  A test
        model's global_step never moves, so forward() draws the same noise every time; here the caller counts its calls.
        Eager only, on the current stream: the injected-noise flag, a captured graph and global_step are not touched, and a
        forward() afterwards draws its own noise again and gives what it gave before."""
        H.require_device(self.input_images, "the model's input buffer", "AIRModel.forward_sampled", capture_too=True)
        self._fresh_shadow()
        seed = self._seed if seed is None else int(seed)
        H.launch("air_philox_fill", self.input_images.device, _ptr(self.normals), self.normals.numel(), _ptr(self.uniforms),
                 self.uniforms.numel(), C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(call)))
        _enqueue(self._forward_plan(injected=True), self._stream())
        self._dirty = False
        self._steps_executed = None
        return self

    def _world(self):
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            return torch.distributed.get_world_size()
        return 1

    def _dp(self):
        """True when a train step runs the data-parallel protocol: backward -> gradient exchange -> norm of the
        exchanged gradient -> clip + Adam (world > 1; or forced on a one-rank group, AIR_DP_FORCE=1)"""
        if self._world() > 1:
            return True
        return self._dp_force and torch.distributed.is_available() and torch.distributed.is_initialized()

    def _collectives_capturable(self):
        """RCCL collectives are stream work and can be recorded into a hipGraph (torch.cuda.graph captures NCCL calls);
        gloo moves device tensors through the host and cannot.  AIR_DP_GRAPH_COLLECTIVE=0 keeps the collective outside."""
        return (self._dp() and torch.distributed.get_backend() == "nccl"
                and os.environ.get("AIR_DP_GRAPH_COLLECTIVE", "1") != "0")

    def sync_parameters(self, src=0):
        """Data parallel: every rank continues from rank `src`'s variables, Adam slots and global_step
        (one broadcast each; DESIGN section 6 needs clip + Adam to run on identical state everywhere).
        Called by capture_graph() / the first training() after the process group exists."""
        world = self._world()
        if world > 1:
            st = self.store
            for buf in (st.params, st.m, st.v, st.istate):
                torch.distributed.broadcast(buf, src)
        self.store.synced_world = world
        self.store.touch()
        self._dirty = True

    def _optimizer_ops(self):
        world = self._world()
        if self._opt_world != (world, self._dp()):
            st = self.store
            fused = not self._dp()
            npart = self._wgrad_blocks + self._cnn_sq if fused else self.lib.air_optim_num_partials(st.n)
            if self._twins and len(st.panels):
                # (with the panels whether or not THIS model reads them: another model on the scope may)
                adam = self._call("air_adam_clip_step_panels", _ptr(st.params), _ptr(st.grads), _ptr(st.m), _ptr(st.v),
                                  st.n, _ptr(st.partials), npart, _ptr(self.dyn), _ptr(st.istate), 1.0 / world,
                                  0.9, 0.999, 1e-8, _ptr(st.params16), st.panels, len(st.panels), _ptr(st.params16p),
                                  _ptr(st.gnorm), nbytes=30 * st.n, tag="adam_clip")
            else:
                adam = self._call("air_adam_clip_step", _ptr(st.params), _ptr(st.grads), _ptr(st.m), _ptr(st.v),
                                  st.n, _ptr(st.partials), npart, _ptr(self.dyn), _ptr(st.istate), 1.0 / world,
                                  0.9, 0.999, 1e-8, _ptr(st.params16) if self._twins else None, _ptr(st.gnorm),
                                  nbytes=(30 if self._twins else 28) * st.n, tag="adam_clip")
            # data parallel: the norm is that of the all-reduced gradient -> separate pass after the collective
            self._opt = [adam] if fused else [self._sqnorm, adam]
            self._opt_world = (world, self._dp())
        return self._opt

    def _dp_factors(self):
        """Launch lists of the factor exchange (dp_exchange="factors", world > 1): local weight gradients WITHOUT
        dWx (its bias gradient, the column sums of sum_t dgates, by air_colsum), and -- after the collectives -- dWx
        from the gathered factors: ONE weight-gradient problem with K = world * B rows."""
        world = self._world()
        if self._dp_factor_ops is not None and self._dp_factor_ops["world"] == world:
            return self._dp_factor_ops
        st, G, dm = self.store, self.store.G, self.store.dims
        B, D, R = self.batch_size, dm["D"], dm["R"]
        dv = self.input_images.device
        n_local = len(self._wgrad_arr) - 1                       # the input-weight problem is the last one
        local = (H.Wgrad * n_local)(*[self._wgrad_arr[i] for i in range(n_local)])
        x_all = torch.zeros(world * B, D, dtype=torch.float32, device=dv)
        dg_all = torch.zeros(world * B, 4 * R, dtype=torch.float32, device=dv)
        Gx = G["lstm_kernel"][:D]
        fac = (H.Wgrad * 1)(H.Wgrad(A=_ptr(x_all), dY=_ptr(dg_all), dW=_ptr(Gx), M=D, N=4 * R, K=world * B, lda=D, ldb=4 * R,
                                    ldc=4 * R))
        cs = (H.Colsum * 1)(H.Colsum(_ptr(self.dgsum), _ptr(G["lstm_bias"]), B, 4 * R, 4 * R, 0))
        self._keep += [local, fac, cs]
        ops = dict(world=world, x_all=x_all, dg_all=dg_all, tail=st.grads[D * 4 * R:],
                   local=self._call("air_wgrad_grouped", local, n_local, self._prec, None, None, tag="wgrad_grouped_local"),
                   bias=self._call("air_colsum", cs, 1, tag="lstm_bias_colsum"),
                   dwx=self._call("air_wgrad_grouped", fac, 1, self._prec, None, None, tag="wgrad_dWx_gathered"))
        self._dp_factor_ops = ops
        return ops

    def _dp_exchange_gradients(self):
        """The collectives of one data-parallel step (between the two captured graphs)."""
        dist = torch.distributed
        if self._dp_exchange == "flat":
            dist.all_reduce(self.store.grads)                    # ONE collective: grads + loss/accuracy tail
            return
        f = self._dp_factors()
        world, B = f["world"], self.batch_size
        for out, inp in ((f["x_all"], self.input_images), (f["dg_all"], self.dgsum)):
            if dist.get_backend() == "nccl":
                dist.all_gather_into_tensor(out, inp)
            else:
                # gloo moves device tensors only through broadcast / all_reduce: x + 0 is exact, so a zero-padded
                # all_reduce delivers the same rows an all_gather would
                r = dist.get_rank()
                out.zero_()
                out[r * B:(r + 1) * B].copy_(inp)
                dist.all_reduce(out)
        dist.all_reduce(f["tail"])                               # everything but dWx (+ loss / accuracy)

    def _run_backward(self, s, for_update=False, fused_finalize=False, fold=False):
        _enqueue(self._backward_plan(for_update, fused_finalize, fold), s)

    def captured_xwx_kernels(self):
        """Kernel name of the x.Wx launch of every step of the captured replay, in order (None: no train graph): the names
        of the ops that were enqueued under capture (captured_xwx_ops())."""
        ops = self.captured_xwx_ops()
        return None if ops is None else [op.kernel for op in ops]

    def captured_xwx_ops(self):
        return None if self._graph is None or not self.train else [xwx for xwx, _ in self._graph_record]

    def captured_step_ops(self, step=0):
        """The launches of train step `step` of the captured replay, in order (None: no train graph): the plan that was
        enqueued under capture.  Where the library has the form, compose and the write backward are ONE of them
        (air_write_fwd_bwd: compose_fold), so the list is one shorter than train_step_ops(), the eager step.
        After set_noise that includes the schedules-only prologue launch (air_step_begin): always captured then, not listed before.
        Data parallel over a backend whose collectives cannot be captured: the ops of the FIRST graph, prologue to weight
        gradients -- the optimizer is replayed from a graph of its own after the exchange and is not listed."""
        return None if self._graph is None or not self.train else list(self._graph_record[step][1])

    def _train_phase_a(self, s, twin_x=False, fold=False):
        """step prologue + forward + loss + backward (+ weight grads) into the flat grad buffer"""
        self._run_forward(s, finalize=False, twin_x=twin_x, fold=fold)
        self._run_backward(s, for_update=True, fused_finalize=True, fold=fold)

    def _train_phase_b(self, s):
        _enqueue(self._update_plan(), s)

    def _warm_up(self, run):
        """run() on a side stream before a capture: lazy module loads, LDS attributes, communicators -- never under capture"""
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def capture_graph(self, steps=1, between_steps=None, after_steps=None):
        """Captures the train step into hipGraphs (fixed N, no host sync, no allocation inside).
        Single GPU: ONE graph of `steps` consecutive train steps.  Data parallel over RCCL: the same -- the gradient
        exchange is stream work and is recorded between the backward and the optimizer of every step,
        ([fwd+bwd] -> all_reduce -> [sqnorm + clip + Adam]) x steps in ONE replay, the protocol of the 1-GPU number.
        Data parallel over a backend whose collectives cannot be captured (gloo): [fwd+bwd] | collective | [clip+Adam],
        one step per replay.  Noise and schedules are keyed by the device-side global_step, so the steps of a replay
        differ as they would in separate replays; `between_steps(i)` (optional, graph-capturable device work such as
        the next batch's gather) is captured before step i, `after_steps()` after the last one (e.g. the join of a branch
        that between_steps forked: air.sources.ShuffleBatchQueue.graph_hooks).  training() then advances `steps` steps."""
        if not self.train:
            return self._capture_forward_graph()
        self._capture_args = dict(steps=steps, between_steps=between_steps, after_steps=after_steps)
        self._follow_schedule(recapture=False)        # (this call is the capture)
        world = self._world()
        if self.store.synced_world != world:
            self.sync_parameters()
        self._fresh_shadow()
        dp = self._dp()
        in_graph = self._collectives_capturable()
        if steps < 1 or (steps > 1 and dp and not in_graph):
            raise ValueError("multi-step graphs need world_size 1 or a backend whose collectives can be captured (nccl)")
        self._graph_steps = steps
        factors = dp and self._dp_exchange == "factors"
        self._update_plan()                      # (the lazily built ops and buffers exist before anything is captured)

        def warm():
            s = self._stream()
            _enqueue(self._forward_plan() + self._backward_plan(for_update=factors), s)
            if dp:
                self._dp_exchange_gradients()    # also the first collective of the communicator: never under capture
                if factors:
                    self._dp_factors()["dwx"](s)
            if self._fold_op is not None:
                self._fold_op(s)                 # (its LDS grant, like every launch's, is a driver call: never under capture)
        self._warm_up(warm)
        # Step 0 of a replay reads the caller's fp32 image batch (the host may have rewritten it since the last replay) and
        # leaves its padded bf16 twin behind; nothing inside the graph writes the batch unless a between_steps hook does, so
        # the steps behind it read the twin: half the A bytes of x.Wx, both operands by LDS-DMA.  (Not where the x.Wx launch
        # itself carries the step prologue -- max_steps == 1: that launch is the fp32-operand one.)
        # (Nor with the conv front-end, whose model builds no twin-operand launch: Adam moves the conv variables, so the LSTM's
        # input differs from step to step.)
        can_twin = between_steps is None and self._xwx_twin_op is not None and self._begin_host[0] != 0
        # Every captured step runs compose inside the write-backward launch where the library has that form for this model
        # (air_write_fwd_bwd: one launch fewer, same results) -- with or without hooks: nothing it reads can be stale.
        fold = self._fold_op is not None
        record = []                              # per step: (its x.Wx op, the plan that was enqueued)
        ga = torch.cuda.CUDAGraph()
        # (thread_local: RCCL's watchdog thread may touch the runtime while this thread captures)
        with torch.cuda.graph(ga, **({"capture_error_mode": "thread_local"} if dp else {})):
            for i in range(steps):
                if between_steps is not None:
                    between_steps(i)
                s = self._stream()
                fwd = self._forward_plan(finalize=False, twin_x=i >= 1 and can_twin, fold=fold)
                bwd = self._backward_plan(for_update=True, fused_finalize=True, fold=fold)
                # (a backend whose collectives cannot be captured: the optimizer is recorded into the second graph, below)
                update = [] if (dp and not in_graph) else self._update_plan()
                _enqueue(fwd + bwd, s)
                if dp and in_graph:
                    self._dp_exchange_gradients()
                    s = self._stream()
                _enqueue(update, s)
                record.append((self._xwx_of(fwd), fwd + bwd + update))
            if after_steps is not None:
                after_steps()
            if dp and in_graph and world > 1:
                self.scalars[:2].mul_(1.0 / world)       # loss / accuracy rode in the all-reduce as sums over ranks
        gb = None
        if dp and not in_graph:
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb):
                self._train_phase_b(self._stream())
        self._graph = (ga, gb)
        self._graph_record = record
        self._graph_dp = (dp, in_graph)
        return self

    def _capture_forward_graph(self):
        """train=False models (the demo / evaluation call, demo/model_wrapper.py:19-30): the whole
        forward -- schedules + noise, hoisted x.Wx, N x (LSTM, heads, read, VAE), compose, batch means --
        as ONE hipGraph; forward() then is a single replay."""
        self._fresh_shadow()
        self._warm_up(lambda: self._run_forward(self._stream()))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._run_forward(self._stream())
        self._graph = (g, None)
        self._graph_steps = 1
        return self

    def release_graph(self):
        self._graph = None

    def training(self, eager=False):
        """The train op (reference :692): forward, loss, backward, clip, Adam, global_step += 1.
        With a captured graph one call advances `steps` train steps (capture_graph); eager=True
        runs exactly one step through plain launches even then."""
        if not self.train:
            raise RuntimeError("model was built with train=False")
        world = self._world()
        if self.store.synced_world != world:
            self.sync_parameters()
        self._follow_schedule()
        self._fresh_shadow()
        dp = self._dp()
        if self._host_step is not None:
            self._host_step += self._graph_steps if (self._graph is not None and not eager) else 1
        if self._graph is not None and not eager:
            ga, gb = self._graph
            if self._graph_dp[0] != dp:
                raise RuntimeError("the captured graph was recorded for another process-group state; capture_graph() again")
            ga.replay()
            if gb is not None:
                self._dp_exchange_gradients()
                gb.replay()
                if world > 1:
                    self.scalars[:2].mul_(1.0 / world)
        else:
            s = self._stream()
            self._train_phase_a(s)
            if dp:
                self._dp_exchange_gradients()
            self._train_phase_b(s)
            if world > 1:
                self.scalars[:2].mul_(1.0 / world)
        if not self._twins:
            # this model's Adam launch does not maintain the bf16 shadow of the (shared) variables: whoever reads it
            # next -- e.g. a reuse=True model with bf16 twins on the same scope -- has to re-derive it first
            self.store.shadow_stale = True
        self._dirty = False
        self._steps_executed = None

    __call__ = forward

    # ------------------------------------------------- generation (air/_generate.py)
    def generate_ops(self, likelihood_noise=False, given=False, fill=True):
        """The launches of one generate() (given=False) or decode() call, in order (profiling tools)."""
        return self._generator.launch_list(likelihood_noise, given, fill)

    def set_generate_noise(self, noise):
        """Injects eps_scale [N,B,1], eps_shift [N,B,2], eps_z [N,B,Z], eps_x [N,B,d], u [N,B] (the dict of set_noise) for
        ONE generate() / decode() call; the device RNG is back after it."""
        self._generator.set_noise(noise)

    def generate(self, likelihood_noise=False):
        """Draws batch_size scenes from the model's priors and renders them: z_pres from the Concrete prior (rounded, as at
        test time), scale / shift / z_what from their Gaussian priors -- all read from the live dynamic scalars, so
        set_dynamic() and annealed values apply --, the stopping rule of the loop, the decoder as forward() runs it and the
        compose kernel's canvas.  likelihood_noise=False renders the decoder's mean image, True adds vae_likelihood_std
        noise before the sigmoid (vae.py:36-41).  Noise comes from the device Philox stream keyed by (seed, number of
        earlier drawing calls): the same seed and call index give the same scenes, successive calls differ.  Works on train
        and test models; returns a GeneratedScenes.  No gradients flow through it."""
        return self._generator.run(False, bool(likelihood_noise), True)

    def decode(self, latents, scales, shifts, z_pres, likelihood_noise=False):
        """Renders the scenes described by the caller's DEVICE tensors latents [B,N,Z], scales [B,N,1] (or [B,N]), shifts
        [B,N,2] and z_pres [B,N] (used as given -- it may be relaxed; the masks are re-derived by the stopping rule), the
        way generate() renders its own.  likelihood_noise=True draws eps_x (or takes set_generate_noise's)."""
        return self._generator.decode(latents, scales, shifts, z_pres, likelihood_noise)

    # ------------------------------------------------------------------ outputs
    def _ensure(self):
        if self._dirty:
            self.forward()

    @property
    def steps_executed(self):
        """T' of the reference's while_loop (cond :271-275) for the last pass."""
        self._ensure()
        if self._steps_executed is None:
            alive = (self.att[:, :, H.ATT_MASK] > 0).any(dim=1).cpu().tolist()
            tprime = 1
            for t in range(self.max_steps - 1):
                if alive[t]:
                    tprime += 1
                else:
                    break
            self._steps_executed = tprime
        return self._steps_executed

    def _stack(self, x):
        return x[:self.steps_executed].transpose(0, 1)

    loss = property(lambda self: (self._ensure(), self.scalars[0])[1])
    accuracy = property(lambda self: (self._ensure(), self.scalars[1])[1])
    global_step = property(lambda self: self.store.istate[H.IST_GLOBAL_STEP])
    reconstruction = property(lambda self: (self._ensure(), self._recon)[1])
    reconstruction_loss = property(lambda self: (self._ensure(), self._rec_loss)[1])
    rec_num_digits = property(lambda self: (self._ensure(), self.run_digits)[1])
    loss_per_item = property(lambda self: (self._ensure(), self._loss_item)[1])     # air_model.py:598-600, before the mean
    rec_scales = property(lambda self: self._stack(self.att[:, :, H.ATT_S:H.ATT_S + 1]))
    rec_shifts = property(lambda self: self._stack(self.att[:, :, H.ATT_X:H.ATT_Y + 1]))
    rec_windows = property(lambda self: self._stack(self.vrec))
    rec_latents = property(lambda self: self._stack(self.ml[:, :, :self.vae_latent_dimensions]))
    z_pres_probs = property(lambda self: self._stack(self.att[:, :, H.ATT_ZPROB]))
    z_pres_kls = property(lambda self: self._stack(self.att[:, :, H.ATT_KL_Z]))
    scale_kls = property(lambda self: self._stack(self.att[:, :, H.ATT_KL_SCALE]))
    shift_kls = property(lambda self: self._stack(self.att[:, :, H.ATT_KL_SHIFT]))
    vae_kls = property(lambda self: self._stack(self.att[:, :, H.ATT_KL_VAE]))

    def summary_names(self):
        """Names of the reference's numeric summaries (self.num_summaries of air_model.py:160-209, 608-625), in its order."""
        return ["loss", "accuracy"] + _summaries.numeric_names(self.max_steps, self.max_digits)

    def numeric_summaries(self, out=None):
        """The values of summary_names() for the last pass, as ONE launch on the current stream (air_summaries,
        include/air_hip.h) into the float32 device vector `out` (allocated when None) -- what sess.run(num_summaries)
        evaluates at training.py:171-180.  No host synchronisation: the caller copies `out` when it wants the numbers."""
        self._ensure()
        return _summaries.numeric_summaries(self, out)

    # ---- histogram summaries (air_model.py:642-687): air_histograms over strided views of the flat buffers (air/summaries.py)
    def _summary_tags(self):
        return _summaries.summary_tags(self.max_steps, self.max_digits, self.vae_recognition_units, self.vae_generative_units,
                                       self.scope)

    def _no_cnn_histograms(self):
        if self.cnn:
            raise NotImplementedError("the histogram summaries of a cnn=True model are not implemented (its tag lists are a "
                                      "follow-up: DESIGN.md section 25); numeric_summaries() works")

    def var_summary_names(self):
        """Tags of var_summaries(), the reference's 36 at its shapes: "<scope>_1/summaries/<scope>/rnn/<variable>_0" in
        tf.trainable_variables() order (the name scope of the variable-sharing test model, which training.py fetches
        them from)."""
        self._no_cnn_histograms()
        return self._summary_tags().variables

    def grad_summary_names(self):
        """Tags of the histograms of grad_summaries(): "<scope>/training/<scope>/rnn/<variable>_0_grad_original" for every
        variable, then "..._grad_applied" (air_model.py:657-687).  air.summaries.gradient_summaries() adds the _norm / _avg
        scalars the reference writes beside each."""
        self._no_cnn_histograms()
        return self._summary_tags().gradients[::3]

    def var_summaries(self, out=None):
        """TensorFlow's histograms of the variables (tf.summary.histogram(v.name, v.value()), air_model.py:642-649), tags
        var_summary_names(), as ONE call of air_histograms (include/air_hip.h) on the current stream over the strided views
        of the flat variable buffer -- nothing is copied out variable by variable.  `out`: a uint8 device vector
        (allocated when None) that air.summaries.decode_histograms() reads once fetched.  No host synchronisation."""
        self._no_cnn_histograms()
        return _summaries.histograms(self, "var", out)

    def grad_summaries(self, out=None):
        """The histograms of the gradients, original and applied (air_model.py:657-687), tags grad_summary_names(), as ONE
        call of air_histograms over the flat gradient buffer: original = g / world, applied = that times the
        clip_by_global_norm factor air_adam_clip_step used, from the global norm it left on the device.  Describes the
        gradient left by the LAST train step: after a captured replay of several steps that is the last step of the replay.
        Train models only.  No host synchronisation."""
        if not self.train:
            raise H.AirHipError("grad_summaries: the model was built with train=False and has no gradients")
        self._no_cnn_histograms()
        return _summaries.histograms(self, "grad", out)

    @property
    def rec_st_back(self):
        return st_matrices(self._stack(self.att[:, :, H.ATT_ST_BACK:H.ATT_ST_BACK + 3]))   # [B,T',3] = 1/s, -x/s, -y/s

    def state_dict(self):
        return self.store.state_dict()

    def save_tf_checkpoint(self, prefix):
        """Writes `<prefix>.index` + `<prefix>.data-00000-of-00001` in TensorFlow's bundle format
        with the reference graph's variable names (what tf.train.Saver writes at training.py:203-207),
        Adam slots included -- restorable by the reference's demo.py:33 / training.py."""
        import tf_checkpoint as tfc
        shapes = {k: tuple(v.shape) for k, v in self.store.variables.items()}
        return tfc.save_checkpoint(prefix, tfc.model_to_tensors(self.store.state_dict(), shapes))

    def load_tf_checkpoint(self, prefix, verify=True):
        """Restores variables (and Adam slots / global_step when present) from a TensorFlow bundle
        written by the reference (`model/air-model`, `air_results/model/air-model-<step>`).  The bundle goes through
        load_state_dict: it is validated before anything is written, so a malformed one -- a variable missing, only one of
        a variable's two Adam slots -- is refused with the model's state untouched."""
        import tf_checkpoint as tfc
        self.load_state_dict(tfc.tensors_to_state_dict(tfc.load_checkpoint(prefix, verify)))
        return self

    def load_state_dict(self, sd, strict=True, load_optimizer=True):
        self.store.load_state_dict(sd, strict, load_optimizer)
        self._dirty = True
        self._host_step = None
