"""ctypes binding of libair_hip.so (C ABI declared in include/air_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol
cannot be resolved the import fails loudly.  Build it with
``python tf-attend-infer-repeat_amd/build.py`` (hipcc --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- FIRST: torch brings its own libamdhip64; loading libair_hip.so before it binds the library to a
#                              second HIP runtime that sees no device ("no ROCm-capable device is detected" at the first launch)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AIR_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libair_hip.so")   # override: A/B builds in tools/
# the package default of air_gemm_t.precision -- "fp32": exact-fp32 MFMA (parity path); "bf16": bf16 operands, fp32 accumulate
GEMM_PRECISION = os.environ.get("AIR_GEMM_PRECISION", "fp32")

# Every upper-case integer constant X below is AIR_X of include/air_hip.h, and every Structure the CamelCase of its
# air_*_t: tests/test_abi.py compares all of them, and _SIGNATURES, with the header.
ABI_VERSION = 6
EINVAL, ELIMIT, EALIGN = -1, -2, -3
DYN_PRIOR_LOG_ODDS, DYN_TEMPERATURE, DYN_STOP_THRESHOLD, DYN_LEARNING_RATE, DYN_CLIP_NORM = 0, 1, 2, 3, 4
DYN_SCALE_PM, DYN_SCALE_PV, DYN_SHIFT_PM, DYN_SHIFT_PV, DYN_VAE_PM, DYN_VAE_PV = 5, 6, 7, 8, 9, 10
DYN_LIK_STD, DYN_GRAD_SCALE, DYN_COUNT = 11, 12, 16
DYN_SCALE_PLV, DYN_SHIFT_PLV, DYN_VAE_PLV = 13, 14, 15
IST_GLOBAL_STEP, IST_COUNT = 0, 4
ATT_S, ATT_X, ATT_Y, ATT_ZPRE, ATT_Z, ATT_ZPROB = 0, 1, 2, 3, 4, 5
ATT_KL_Z, ATT_KL_SCALE, ATT_KL_SHIFT, ATT_KL_VAE, ATT_MASK_PREV, ATT_MASK, ATT_ST_BACK = 6, 7, 8, 9, 10, 11, 12
ATT_STRIDE, OUT_STRIDE = 16, 8
ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_SIGMOID_NOISE = 0, 1, 2, 3
GRAD_NONE, GRAD_RELU, GRAD_SOFTPLUS = 0, 1, 2
EPI_GENERIC, EPI_LSTM_FWD, EPI_REPARAM_FWD, EPI_LSTM_BWD, EPI_REPARAM_BWD, EPI_LSTM_BWD_TAIL, EPI_LSTM_FWD0 = 0, 1, 2, 3, 4, 5, 6
SCHED_STAIRCASE, SCHED_HAS_MIN, SCHED_HAS_MAX, SCHED_LOG = 1, 2, 4, 8
LIK_BERNOULLI, LIK_GAUSSIAN = 0, 1

_p = C.c_void_p
_i = C.c_int32
_f = C.c_float


class Schedule(C.Structure):
    _fields_ = [("slot", _i), ("flags", _i), ("init", _f), ("iters", _f), ("factor", _f),
                ("vmin", _f), ("vmax", _f)]


class StepJob(C.Structure):
    _fields_ = [("sched", _p), ("nsched", _i), ("dyn", _p), ("istate", _p),
                ("normals", _p), ("n_normal", C.c_int64), ("uniforms", _p), ("n_uniform", C.c_int64),
                ("seed", C.c_uint64), ("twin_src", _p), ("twin_dst", _p), ("twin_n", C.c_int64)]


class Gemm(C.Structure):
    _fields_ = [("A", _p), ("B", _p), ("C", _p),
                ("M", _i), ("N", _i), ("K", _i), ("lda", _i), ("ldb", _i), ("ldc", _i),
                ("transA", _i), ("transB", _i),
                ("bias", _p), ("addend", _p), ("ldadd", _i), ("aux", _p), ("ldaux", _i),
                ("aux_scale", _f), ("act", _i), ("actgrad", _i), ("accumulate", _i), ("precision", _i),
                ("epi", _i), ("tile_m", _i), ("tile_n", _i), ("ksplit", _i), ("addend_slabs", _i), ("i0", _i),
                ("p0", _p), ("p1", _p), ("p2", _p), ("p3", _p), ("q0", _p), ("q1", _p), ("q2", _p),
                ("step_job", C.POINTER(StepJob)),
                ("A16", _p), ("B16", _p), ("C16", _p), ("q0_16", _p), ("q2_16", _p), ("B16p", _p)]


class Panel(C.Structure):
    """air_panel_t: one row-major [K, N] matrix of the flat variable buffer and where its panel-blocked bf16 twin lives"""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("K", _i), ("N", _i), ("gates", _i), ("exclusive", _i)]


MAX_PANELS = 16
MAX_WGRAD_PROBLEMS = 16       # air_wgrad_grouped takes that many problems in one launch


class Colsum(C.Structure):
    _fields_ = [("src", _p), ("dst", _p), ("rows", _i), ("cols", _i), ("ld", _i), ("accumulate", _i)]


class Wgrad(C.Structure):
    _fields_ = [("A", _p), ("dY", _p), ("dW", _p), ("db", _p),
                ("M", _i), ("N", _i), ("K", _i), ("lda", _i), ("ldb", _i), ("ldc", _i),
                ("head_pack", _i), ("Hs", _i), ("Hh", _i), ("Hz", _i), ("A16", _p), ("dY16", _p)]


class AttendFwd(C.Structure):
    _fields_ = [("hid", _p), ("wout", _p), ("bout", _p), ("canvas", _p),
                ("eps_scale", _p), ("eps_shift", _p), ("u", _p), ("dyn", _p),
                ("out7", _p), ("att", _p), ("window", _p),
                ("B", _i), ("N", _i), ("C", _i), ("w", _i), ("Hs", _i), ("Hh", _i), ("Hz", _i),
                ("wout_ld", _i), ("train", _i), ("window16", _p)]


class AttendBwd(C.Structure):
    _fields_ = [("hid", _p), ("wout", _p), ("canvas", _p), ("eps_scale", _p), ("eps_shift", _p),
                ("dyn", _p), ("out7", _p), ("att", _p), ("d_window", _p), ("d_sxy_write", _p),
                ("d_hid", _p), ("d_out7", _p),
                ("B", _i), ("N", _i), ("C", _i), ("w", _i), ("Hs", _i), ("Hh", _i), ("Hz", _i), ("wout_ld", _i),
                ("literal", _i), ("d_hid16", _p)]


class WriteFwd(C.Structure):
    _fields_ = [("vrec", _p), ("ml", _p), ("images", _p), ("dyn", _p), ("att", _p), ("recon", _p),
                ("rec_loss", _p), ("d_recon", _p), ("run_loss", _p), ("run_digits", _p), ("loss_item", _p),
                ("B", _i), ("N", _i), ("C", _i), ("w", _i), ("Z", _i), ("wb_order", _p), ("likelihood", _i)]


class WriteBwd(C.Structure):
    _fields_ = [("d_recon", _p), ("vrec", _p), ("att", _p), ("d_gen_pre", _p), ("d_sxy_write", _p),
                ("B", _i), ("N", _i), ("C", _i), ("w", _i), ("literal", _i),
                ("fin_loss_item", _p), ("fin_targets", _p), ("fin_digits", _p), ("fin_scalars", _p), ("d_gen_pre16", _p),
                ("order", _p)]


class BottleneckFwd(C.Structure):
    _fields_ = [("X", _p), ("Wml", _p), ("bml", _p), ("eps", _p), ("Wg", _p), ("bg", _p), ("ml", _p), ("z", _p), ("g", _p),
                ("M", _i), ("K1", _i), ("Z", _i), ("H", _i), ("ldx", _i), ("z16", _p), ("g16", _p),
                ("X16", _p), ("Wml16", _p), ("Wg16", _p), ("exact_fp32", _i), ("ldz", _i)]


class BottleneckBwd(C.Structure):
    _fields_ = [("dG", _p), ("Wg", _p), ("ml", _p), ("eps", _p), ("att", _p), ("dyn", _p), ("Wml", _p), ("x", _p),
                ("d_ml", _p), ("d_x", _p), ("M", _i), ("K1", _i), ("Z", _i), ("H", _i), ("d_ml16", _p), ("d_x16", _p),
                ("dG16", _p), ("Wg16", _p), ("Wml16", _p), ("exact_fp32", _i)]


class ShuffleBatch(C.Structure):
    _fields_ = [("queue", _p), ("state", _p), ("picks", _p), ("capacity", _i), ("batch", _i), ("min_after_dequeue", _i),
                ("n_records", _i), ("seed", C.c_uint64)]


class Summaries(C.Structure):
    _fields_ = [("att", _p), ("targets", _p), ("digits", _p), ("rec_loss", _p), ("loss_item", _p), ("scalars", _p),
                ("out", _p), ("B", _i), ("N", _i), ("max_digits", _i)]


class SceneRecords(C.Structure):
    """air_scene_records_t: the four sources are noise (given = 0) or the caller's scales / shifts / latents / z_pres"""
    _fields_ = [("scale_src", _p), ("shift_src", _p), ("z_src", _p), ("pres_src", _p), ("dyn", _p), ("att", _p),
                ("z", _p), ("z16", _p), ("B", _i), ("N", _i), ("Z", _i), ("ldz", _i), ("given", _i)]


class Render(C.Structure):
    _fields_ = [("vrec", _p), ("att", _p), ("canvas", _p), ("num_digits", _p), ("B", _i), ("N", _i), ("C", _i), ("w", _i)]


MAX_STEPS = 16


class StepLds(C.Structure):
    """air_step_lds_t: dynamic LDS per workgroup, in bytes, of the sampler launches of a step, and the limit"""
    _fields_ = [(k, C.c_int64) for k in ("attend_fwd", "attend_bwd", "write_fwd", "render", "write_bwd_exact",
                                         "write_bwd_graph", "limit")]


class Scalar(C.Structure):
    """air_scalar_t: a float by value (ptr NULL), one device float read by the kernel (stride 0), or one per element (stride 1)"""
    _fields_ = [("ptr", _p), ("value", _f), ("stride", _i)]


class CnnFwd(C.Structure):
    """air_cnn_fwd_t: the four saved tensors (pool1, pool2, arg1, arg2) come together or not at all"""
    _fields_ = [("images", _p), ("k1", _p), ("b1", _p), ("k2", _p), ("b2", _p), ("k3", _p), ("b3", _p), ("out", _p),
                ("pool1", _p), ("pool2", _p), ("arg1", _p), ("arg2", _p), ("B", _i), ("S", _i), ("F", _i)]


class CnnBwd(C.Structure):
    _fields_ = [("d_out", _p), ("out", _p), ("images", _p), ("pool1", _p), ("pool2", _p), ("arg1", _p), ("arg2", _p),
                ("k1", _p), ("k2", _p), ("k3", _p), ("workspace", _p),
                ("d_k1", _p), ("d_b1", _p), ("d_k2", _p), ("d_b2", _p), ("d_k3", _p), ("d_b3", _p), ("d_images", _p),
                ("B", _i), ("S", _i), ("F", _i)]


HISTOGRAM_MAX = 128


class HistogramDesc(C.Structure):
    """air_histogram_desc_t: a 2-D view as it lies in memory, element (r, c) = base[r * ld + c]; scale_kind 0 stored value,
    1 x * prescale, 2 x * (prescale * clip factor)"""
    _fields_ = [("base", _p), ("rows", _i), ("cols", _i), ("ld", _i), ("scale_kind", _i)]


class Histograms(C.Structure):
    """air_histograms_t: `descs` is a HOST array; out / workspace are device buffers of out_bytes / workspace_bytes"""
    _fields_ = [("descs", C.POINTER(HistogramDesc)), ("count", _i), ("prescale", _f), ("dyn", _p), ("gnorm", _p),
                ("out", _p), ("workspace", _p), ("out_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


EMBED_MAX_STEPS = EMBED_MAX_DIGITS = 16
EMBED_MATCHED, EMBED_PRESENT, EMBED_INFERRED, EMBED_OVERFLOW, EMBED_COUNTERS = 0, 1, 2, 3, 4


class EmbedCollect(C.Structure):
    """air_embed_collect_t: one inference chunk of the projector export -- the model's buffers, the chunk's padded ground
    truth, the dataset-level outputs and the device counters that carry the row cursor from chunk to chunk"""
    _fields_ = [("att", _p), ("run_digits", _p), ("ml", _p), ("vrec", _p),
                ("gt_count", _p), ("gt_positions", _p), ("gt_boxes", _p), ("gt_labels", _p), ("gt_ids", _p),
                ("match", _p), ("counters", _p), ("out_latents", _p), ("out_windows", _p), ("out_labels", _p), ("out_ids", _p),
                ("T", _i), ("B", _i), ("k", _i), ("G", _i), ("Z", _i), ("w", _i), ("capacity", _i), ("canvas_size", _i),
                ("max_distance", C.c_double)]


SCENE_MAX_CANVAS, SCENE_MAX_GLYPH, SCENE_MAX_DIGITS, SCENE_MAX_GAP, SCENE_MAX_ATTEMPTS, SCENE_MAX_RESTARTS = 128, 32, 6, 4, 100, 64


class SceneSource(C.Structure):
    """air_scene_source_t: glyphs and their crop boxes in, one composed batch (canvases, counts, metadata, status) out;
    batch_counter is a device int64 that air_scene_source_advance moves"""
    _fields_ = [("glyphs", _p), ("crops", _p), ("bg", _p), ("counts", _p), ("batch_counter", _p),
                ("images", _p), ("digits", _p), ("indices", _p), ("positions", _p), ("boxes", _p), ("status", _p),
                ("gave_up", _p),
                ("B", _i), ("G", _i), ("gd", _i), ("C", _i), ("margin", _i), ("gap", _i), ("max_digits", _i),
                ("max_attempts", _i), ("max_restarts", _i), ("seed", C.c_uint64)]


JITTER_MAX_PLANE = 48


class GlyphJitter(C.Structure):
    """air_glyph_jitter_t: base glyphs and their crop boxes in, a bank of V jittered variants (frames, crop boxes, base glyph,
    drawn parameters, status) out; counter is a nullable device int64, the bank generation"""
    _fields_ = [("glyphs", _p), ("crops", _p), ("counter", _p), ("bank", _p), ("bank_crops", _p), ("source", _p),
                ("params", _p), ("status", _p), ("V", _i), ("G", _i), ("gd", _i), ("od", _i),
                ("min_w", C.c_double), ("max_w", C.c_double), ("min_h", C.c_double), ("max_h", C.c_double),
                ("min_ang", C.c_double), ("max_ang", C.c_double), ("seed", C.c_uint64)]


DISTORT_MAX_PLANE, DISTORT_MAX_RADIUS, DISTORT_MAX_STROKE = 40, 64, 4


class GlyphDistort(C.Structure):
    """air_glyph_distort_t: base glyphs (whole planes) and the host-made Gaussian taps in, a bank of V distorted variants
    (frames, boxes, base glyph, drawn parameters, status) out; counter is a nullable device int64, the bank generation"""
    _fields_ = [("glyphs", _p), ("counter", _p), ("taps", _p), ("bank", _p), ("bank_crops", _p), ("source", _p),
                ("params", _p), ("status", _p), ("V", _i), ("G", _i), ("gd", _i), ("od", _i), ("ink", _i), ("radius", _i),
                ("min_stroke", _i), ("max_stroke", _i),
                ("field_gain", C.c_double), ("max_ang", C.c_double), ("max_shear", C.c_double), ("min_scale", C.c_double),
                ("max_scale", C.c_double), ("lo", C.c_double), ("hi", C.c_double), ("seed", C.c_uint64)]


LOC_MAX_STEPS = LOC_MAX_DIGITS = 16
LOC_GROUP = 256
LOC_IMAGES, LOC_PRESENT, LOC_INFERRED, LOC_MATCHED, LOC_HITS, LOC_COUNT_CORRECT, LOC_COUNTS = 0, 1, 2, 3, 4, 5, 6
LOC_IOU, LOC_COVER, LOC_DIST, LOC_SUMS = 0, 1, 2, 3


class Localization(C.Structure):
    """air_localization_t: the records of an inference pass and the padded ground truth of its first k images in, the
    optional per-digit match / IoU out, and the int64 / fp64 accumulators a call adds to"""
    _fields_ = [("att", _p), ("run_digits", _p), ("gt_count", _p), ("gt_positions", _p), ("gt_boxes", _p),
                ("match", _p), ("iou", _p), ("counts", _p), ("sums", _p),
                ("T", _i), ("B", _i), ("k", _i), ("G", _i), ("canvas_size", _i), ("iou_threshold", C.c_double)]


SEG_MAX_STEPS = SEG_MAX_DIGITS = 16
SEG_MAX_CANVAS, SEG_MAX_WINDOW = 128, 32
SEG_IMAGES, SEG_SCORED, SEG_PRESENT, SEG_FG_PIXELS, SEG_FG_MISSED, SEG_BG_CLAIMED, SEG_COUNTS = 0, 1, 2, 3, 4, 5, 6
SEG_ARI, SEG_MASK_IOU, SEG_SUMS = 0, 1, 2


class SceneMasks(C.Structure):
    """air_scene_masks_t: the scene source's glyph table and the metadata of a composed batch in, the uint8 instance labels
    of its canvases out"""
    _fields_ = [("glyphs", _p), ("crops", _p), ("digits", _p), ("indices", _p), ("positions", _p), ("mask", _p),
                ("B", _i), ("G", _i), ("gd", _i), ("C", _i), ("max_digits", _i), ("ink_threshold", _f)]


class Segmentation(C.Structure):
    """air_segmentation_t: the records and decoded windows of an inference pass and the label planes of its first k images
    in, the optional per-image outputs out, and the int64 / fp64 accumulators a call adds to"""
    _fields_ = [("att", _p), ("vrec", _p), ("gt_mask", _p), ("pred_mask", _p), ("tables", _p), ("ari", _p), ("mask_iou", _p),
                ("counts", _p), ("sums", _p),
                ("T", _i), ("B", _i), ("k", _i), ("G", _i), ("C", _i), ("w", _i), ("pred_threshold", _f)]


PROBE_MAX_K, PROBE_MAX_CLASSES, PROBE_MAX_Z, PROBE_MAX_ROWS = 16, 64, 256, 32768
PROBE_QUERY_TILE, PROBE_REF_TILE, PROBE_MAX_SPLITS, PROBE_PASS_ROWS = 64, 32, 8, 8     # facts of the pairs launch
PROBE_ROWS, PROBE_VALID, PROBE_SCORED, PROBE_CORRECT, PROBE_ACTIVE_UNITS, PROBE_COUNTS = 0, 1, 2, 3, 4, 5


class LatentProbe(C.Structure):
    """air_latent_probe_t: latent codes and their labels in (rows: a nullable device int32, how many are in use), the
    optional per-row outputs, the int64 counts with the confusion matrix and the fp64 moments out -- all written whole"""
    _fields_ = [("latents", _p), ("labels", _p), ("rows", _p), ("pred", _p), ("neighbours", _p), ("neighbour_d2", _p),
                ("counts", _p), ("moments", _p), ("M", _i), ("Z", _i), ("k", _i), ("classes", _i),
                ("au_threshold", C.c_double)]


IW_MAX_SAMPLES, IW_MAX_Z = 64, 256
IW_TERM_REC, IW_TERM_Z_PRES, IW_TERM_SCALE, IW_TERM_SHIFT, IW_TERM_WHAT, IW_TERMS = 0, 1, 2, 3, 4, 5
IW_IMAGES, IW_SCORED, IW_DEGENERATE, IW_MAP_CORRECT, IW_SPLIT, IW_COUNTS = 0, 1, 2, 3, 4, 5
IW_BOUND, IW_ELBO, IW_ESS, IW_ENTROPY, IW_SUMS = 0, 1, 2, 3, 4


class Importance(C.Structure):
    """air_importance_t: the records, posterior parameters, samples and noise one pass left on the device in, row `sample`
    of the log-weight, count and (nullable) term tables out"""
    _fields_ = [("att", _p), ("out7", _p), ("ml", _p), ("z", _p), ("eps_scale", _p), ("eps_shift", _p), ("eps_z", _p),
                ("rec_loss", _p), ("run_digits", _p), ("dyn", _p), ("logw", _p), ("digits", _p), ("terms", _p),
                ("T", _i), ("B", _i), ("k", _i), ("Z", _i), ("ldz", _i), ("K", _i)]


class ImportanceFold(C.Structure):
    """air_importance_fold_t: the [K, B] tables and the nullable true counts in, the optional per-image outputs out, and the
    int64 / fp64 accumulators a call adds to"""
    _fields_ = [("logw", _p), ("digits", _p), ("targets", _p), ("bound", _p), ("ess", _p), ("map", _p),
                ("counts", _p), ("sums", _p), ("T", _i), ("B", _i), ("k", _i), ("K", _i)]


KMEANS_MAX_K, KMEANS_MAX_RESTARTS, KMEANS_MAX_ITERS = 64, 32, 1000
KMEANS_ROWS, KMEANS_VALID, KMEANS_LABELLED, KMEANS_CORRECT, KMEANS_LIVE, KMEANS_BEST, KMEANS_ITERS = 0, 1, 2, 3, 4, 5, 6
KMEANS_CONVERGED, KMEANS_RESTARTS_CONVERGED, KMEANS_COUNTS = 7, 8, 9


class LatentKmeans(C.Structure):
    """air_latent_kmeans_t: latent codes and their nullable labels in (rows: a nullable device int32, how many are in use),
    the best restart's assignment, optional d2 and centroids, every restart's inertia and iterations and the int64 counts
    (scalars, sizes[k], majority[k], table[k x classes]) out -- all written whole"""
    _fields_ = [("latents", _p), ("labels", _p), ("rows", _p), ("assignment", _p), ("row_d2", _p), ("centroids", _p),
                ("restart_inertia", _p), ("restart_iters", _p), ("counts", _p),
                ("M", _i), ("Z", _i), ("k", _i), ("classes", _i), ("restarts", _i), ("max_iters", _i), ("seed", C.c_uint64)]


_SIGNATURES = {
    "air_abi_version": (C.c_int, []),
    "air_strerror": (C.c_char_p, [C.c_int]),
    "air_gemm": (C.c_int, [C.POINTER(Gemm), _p]),
    "air_gemm_kernel_name": (C.c_int, [C.POINTER(Gemm), C.c_char_p, C.c_int]),
    "air_gemm_slabs": (C.c_int, [C.c_int, C.c_int]),
    "air_bf16_twin": (C.c_int, [_p, _p, C.c_int64, _p]),
    "air_panel_shadow": (C.c_int, [_p, _p, C.POINTER(Panel), C.c_int, _p]),
    "air_adam_clip_step_panels": (C.c_int, [_p, _p, _p, _p, C.c_int64, _p, C.c_int, _p, _p, _f, _f, _f, _f, _p,
                                            C.POINTER(Panel), C.c_int, _p, _p, _p]),
    "air_colsum": (C.c_int, [C.POINTER(Colsum), C.c_int, _p]),
    "air_wgrad_num_blocks": (C.c_int, [C.POINTER(Wgrad), C.c_int]),
    "air_wgrad_num_workgroups": (C.c_int, [C.POINTER(Wgrad), C.c_int, C.c_int]),
    "air_wgrad_grouped": (C.c_int, [C.POINTER(Wgrad), C.c_int, C.c_int, _p, _p, _p]),
    "air_lstm_gates_fwd": (C.c_int, [_p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_lstm_first_step": (C.c_int, [_p, C.c_int, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_lstm_gates_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, _p]),
    "air_transformer_fwd": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p]),
    "air_transformer_bwd": (C.c_int, [_p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p]),
    "air_transformer_nc_fwd": (C.c_int, [_p, _p, _p] + [C.c_int] * 7 + [_p]),
    "air_transformer_nc_bwd": (C.c_int, [_p, _p, _p, _p, _p] + [C.c_int] * 7 + [_p]),
    "air_attend_fwd": (C.c_int, [C.POINTER(AttendFwd), _p]),
    "air_attend_bwd": (C.c_int, [C.POINTER(AttendBwd), _p]),
    "air_heads_out_wgrad": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p]),
    "air_reparam_fwd": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, _p]),
    "air_reparam_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_write_fwd": (C.c_int, [C.POINTER(WriteFwd), _p]),
    "air_write_bwd": (C.c_int, [C.POINTER(WriteBwd), _p]),
    "air_bce_fwd_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_gauss_nll_fwd_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_finalize": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, _p]),
    "air_step_begin": (C.c_int, [_p, C.c_int, _p, _p, _p, C.c_int64, _p, C.c_int64, C.c_uint64, _p, _p, C.c_int64, _p]),
    "air_optim_num_partials": (C.c_int, [C.c_int64]),
    "air_grad_sqnorm": (C.c_int, [_p, C.c_int64, _p, _p, _p]),
    "air_write_bwd_kernel_name": (C.c_int, [C.POINTER(WriteBwd), C.c_char_p, C.c_int]),
    "air_write_fwd_bwd": (C.c_int, [C.POINTER(WriteFwd), C.POINTER(WriteBwd), _p, _p]),
    "air_write_fwd_bwd_kernel_name": (C.c_int, [C.POINTER(WriteFwd), C.POINTER(WriteBwd), C.c_char_p, C.c_int]),
    "air_vae_bottleneck_fwd": (C.c_int, [C.POINTER(BottleneckFwd), _p]),
    "air_vae_bottleneck_bwd": (C.c_int, [C.POINTER(BottleneckBwd), _p]),
    "air_adam_clip_step": (C.c_int, [_p, _p, _p, _p, C.c_int64, _p, C.c_int, _p, _p, _f, _f, _f, _f, _p, _p, _p]),
    "air_shuffle_batch_init": (C.c_int, [C.POINTER(ShuffleBatch), _p]),
    "air_shuffle_batch_dequeue": (C.c_int, [C.POINTER(ShuffleBatch), _p]),
    "air_shuffle_batch_dequeue_many": (C.c_int, [C.POINTER(ShuffleBatch), C.c_int, _p, _p]),
    "air_batch_gather": (C.c_int, [_p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_summaries_count": (C.c_int, [C.c_int, C.c_int]),
    "air_summaries": (C.c_int, [C.POINTER(Summaries), _p]),
    "air_scene_records": (C.c_int, [C.POINTER(SceneRecords), _p]),
    "air_render": (C.c_int, [C.POINTER(Render), _p]),
    "air_philox_fill": (C.c_int, [_p, C.c_int64, _p, C.c_int64, C.c_uint64, C.c_uint64, _p]),
    "air_step_lds": (C.c_int, [C.c_int] * 7 + [C.POINTER(StepLds)]),
    "air_concrete_sample_fwd": (C.c_int, [_p, _p, C.POINTER(Scalar), _f, C.c_int, _p, _p, C.c_int64, _p]),
    "air_concrete_sample_bwd": (C.c_int, [_p, C.POINTER(Scalar), _p, _p, _p, C.c_int64, _p]),
    "air_concrete_presigmoid_fwd": (C.c_int, [_p, _p, C.POINTER(Scalar), _f, _p, C.c_int64, _p]),
    "air_concrete_presigmoid_bwd": (C.c_int, [_p, C.POINTER(Scalar), _p, C.c_int64, _p]),
    "air_concrete_kl_fwd": (C.c_int, [_p, C.POINTER(Scalar), C.POINTER(Scalar), _p, C.POINTER(Scalar), _f, _p, C.c_int64, _p]),
    "air_concrete_kl_bwd": (C.c_int, [_p, _p, C.POINTER(Scalar), C.POINTER(Scalar), _p, C.POINTER(Scalar), _f, _p, _p, _p,
                                      C.c_int64, _p]),
    "air_sigmoid_bwd": (C.c_int, [_p, _p, _p, C.c_int64, _p]),
    "air_reparam_bwd_plain": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p]),
    "air_cnn_fwd": (C.c_int, [C.POINTER(CnnFwd), _p]),
    "air_cnn_bwd": (C.c_int, [C.POINTER(CnnBwd), _p]),
    "air_cnn_workspace_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "air_cnn_bwd_sq": (C.c_int, [C.POINTER(CnnBwd), _p, _p]),
    "air_cnn_num_sq_partials": (C.c_int, [C.c_int]),
    "air_histogram_num_buckets": (C.c_int, []),
    "air_histogram_limits": (C.c_int, [C.POINTER(C.c_double)]),
    "air_histogram_chunk": (C.c_int, []),
    "air_histogram_record_bytes": (C.c_int64, []),
    "air_histograms_output_bytes": (C.c_int64, [C.POINTER(HistogramDesc), C.c_int]),
    "air_histograms_workspace_bytes": (C.c_int64, [C.POINTER(HistogramDesc), C.c_int]),
    "air_histograms": (C.c_int, [C.POINTER(Histograms), _p]),
    "air_embed_collect": (C.c_int, [C.POINTER(EmbedCollect), _p, _p]),
    "air_embed_collect_workspace_ints": (C.c_int64, [C.c_int] * 4),
    "air_embed_sprites": (C.c_int, [_p, C.c_int, C.c_int, _p, _p, _p]),
    "air_embed_sprite_dim": (C.c_int, [C.c_int]),
    "air_embed_sprites_workspace_doubles": (C.c_int64, [C.c_int, C.c_int]),
    "air_scene_source_compose": (C.c_int, [C.POINTER(SceneSource), C.c_int, _p]),
    "air_scene_source_advance": (C.c_int, [_p, C.c_int, _p]),
    "air_scene_source_prepare": (C.c_int, [C.POINTER(SceneSource)]),
    "air_scene_source_lds": (C.c_int64, [C.c_int, C.c_int]),
    "air_glyph_jitter": (C.c_int, [C.POINTER(GlyphJitter), _p]),
    "air_glyph_jitter_prepare": (C.c_int, [C.POINTER(GlyphJitter)]),
    "air_glyph_jitter_lds": (C.c_int64, [C.c_int, C.c_int]),
    "air_glyph_distort": (C.c_int, [C.POINTER(GlyphDistort), _p]),
    "air_glyph_distort_prepare": (C.c_int, [C.POINTER(GlyphDistort)]),
    "air_glyph_distort_lds": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "air_localization": (C.c_int, [C.POINTER(Localization), _p, _p]),
    "air_localization_workspace_bytes": (C.c_int64, [C.c_int] * 4),
    "air_scene_masks": (C.c_int, [C.POINTER(SceneMasks), _p]),
    "air_segmentation": (C.c_int, [C.POINTER(Segmentation), _p, _p]),
    "air_segmentation_workspace_bytes": (C.c_int64, [C.c_int] * 4),
    "air_latent_probe": (C.c_int, [C.POINTER(LatentProbe), _p, _p]),
    "air_latent_probe_workspace_bytes": (C.c_int64, [C.c_int] * 3),
    "air_latent_probe_splits": (C.c_int, [C.c_int]),
    "air_importance_logw": (C.c_int, [C.POINTER(Importance), C.c_int, _p]),
    "air_importance_fold": (C.c_int, [C.POINTER(ImportanceFold), _p, _p]),
    "air_importance_fold_workspace_bytes": (C.c_int64, [C.c_int] * 4),
    "air_latent_kmeans": (C.c_int, [C.POINTER(LatentKmeans), _p, _p]),
    "air_latent_kmeans_workspace_bytes": (C.c_int64, [C.c_int] * 4),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class AirHipError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    if not os.path.exists(path):
        raise AirHipError(
            "libair_hip.so not found at %s -- the AIR hot path has no CPU fallback. "
            "Build it: python tf-attend-infer-repeat_amd/build.py" % path)
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise AirHipError("libair_hip.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    if lib.air_abi_version() != ABI_VERSION:
        raise AirHipError("libair_hip.so ABI %d != binding ABI %d" % (lib.air_abi_version(), ABI_VERSION))
    return lib


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = load()
    return _LIB


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().air_strerror(rc)
        raise AirHipError("%s failed with code %d: %s" % (what or "libair_hip call", rc,
                                                          msg.decode() if msg else "?"))


# ---- host helpers of every module that calls the library ---------------------------------------------------------------
def ptr(t):
    """device pointer of a tensor; NULL for None"""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream(device):
    """the current stream of `device`, as the hipStream_t every entry point takes last"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def launch(name, device, *args):
    """one eager call of the entry point `name` on the current stream of `device`"""
    check(getattr(lib(), name)(*args, stream(device)), name)


def require_device(t, what, op, capture_too=False):
    """AirHipError unless `t` is a device tensor; capture_too: also while the current stream is capturing (the op modules
    that refuse to run under torch.cuda.graph: DESIGN.md section 18.5)"""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise AirHipError("%s: %s must be a device tensor (no CPU fallback)" % (op, what))
    if capture_too and torch.cuda.is_current_stream_capturing():
        raise AirHipError("%s: not supported under stream capture (torch.cuda.graph); run it eagerly" % op)
