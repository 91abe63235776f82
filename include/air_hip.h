/*
 * air_hip.h -- C ABI of libair_hip.so, the MI355X (gfx950) implementation of the
 * Attend-Infer-Repeat hot path (aakhundov/tf-attend-infer-repeat).
 *
 * The reference has no FFI: its seam is the TensorFlow graph that
 * air/air_model.py builds.  Every entry point below replaces a group of TF ops
 * the reference instantiates per time step; the reference file:line each one
 * replaces is cited.  INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a CALLER-OWNED DEVICE pointer, contiguous row-major fp32
 *     unless stated; the library never allocates or frees, keeps no state but two per-device caches (the LDS grant of a
 *     kernel function, the lane-order probe below), is re-entrant, and does not synchronise -- with ONE exception: the
 *     first EAGER air_write_bwd(literal 2) / air_transformer_bwd / air_transformer_nc_bwd of a process on a device probes the lane order of the LDS
 *     atomic pipe (one tiny kernel, an 8-byte copy back, one stream synchronise).  Under stream capture nothing is probed:
 *     a capture-first caller takes the register-chain accumulator (same bits, slower; a message on stderr).  Every other
 *     call is hipGraph-capture safe from the first call;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 on success, a positive hipError_t from the launch, or a
 *     negative AIR_E* argument error; no C++ exception crosses the boundary.
 */
#ifndef AIR_HIP_H
#define AIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: air_gemm_t / air_wgrad_t carry bf16 twins; `literal` of the sampler backward: 0 exact, 1 per-tap order, 2 the
 * reference graph's order (version 1 headers of round 1 called the per-tap order "reference")
 * 3: panel-blocked bf16 shadows of the weights (air_panel_t, air_gemm_t.B16p, air_panel_shadow,
 *    air_adam_clip_step_panels)
 * 4: measured-negative paths removed (DESIGN.md sections 8-10 keep the record): the deferred Adam slices
 *    (air_step_job_t.ad_*, air_adam_clip_step_blocks), the banded compose (air_write_fwd_t.rec_part / bands,
 *    air_finalize_parts, air_write_bwd_t.fin_rec_part ..), air_adam_clip_step_factored; added: `literal` 3 / 4 of air_write_bwd, air_shuffle_batch_*
 * 5: added air_shuffle_batch_dequeue_many, air_batch_gather, air_summaries; removed `literal` 1 and 3 of the sampler
 *    backward (backward="taps" / "reference_blocked")
 * 6: added air_step_lds (the dynamic LDS of the sampler launches, answered by the functions that size them) */
#define AIR_ABI_VERSION 6

#define AIR_EINVAL   (-1)   /* bad dimension / null pointer            */
#define AIR_ELIMIT   (-2)   /* size exceeds what the kernel supports    */
#define AIR_EALIGN   (-3)   /* pointer / leading dimension misaligned   */

int air_abi_version(void);
const char* air_strerror(int code);

/* ---- dynamic scalars --------------------------------------------------
 * Kernels read the float hyper-parameters that the reference allows to be
 * annealed (air_model.py:76-82) from a device array `dyn` so that a captured
 * hipGraph sees new values without re-capture. */
enum {
    AIR_DYN_PRIOR_LOG_ODDS = 0,  /* z_pres_prior_log_odds          air_model.py:50,405 */
    AIR_DYN_TEMPERATURE    = 1,  /* z_pres_temperature             :51,381             */
    AIR_DYN_STOP_THRESHOLD = 2,  /* stopping_threshold             :52,274,412         */
    AIR_DYN_LEARNING_RATE  = 3,  /* learning_rate                  :54,654             */
    AIR_DYN_CLIP_NORM      = 4,  /* gradient_clipping_norm         :55,673             */
    AIR_DYN_SCALE_PM = 5, AIR_DYN_SCALE_PV = 6,   /* scale prior mean / variance  :38-39 */
    AIR_DYN_SHIFT_PM = 7, AIR_DYN_SHIFT_PV = 8,   /* shift prior                  :40-41 */
    AIR_DYN_VAE_PM   = 9, AIR_DYN_VAE_PV   = 10,  /* vae prior                    :42-43 */
    AIR_DYN_LIK_STD  = 11,                        /* vae_likelihood_std           :44    */
    AIR_DYN_GRAD_SCALE = 12,     /* d(loss)/d(per-item loss) = 1/B (reduce_mean, :610) */
    /* log of the prior variances AS PASSED TO THE CONSTRUCTOR (air_model.py:72-74: tf.log(...) is taken
     * before any annealing schedule replaces the attribute, :76-82) -- never written by a schedule */
    AIR_DYN_SCALE_PLV = 13, AIR_DYN_SHIFT_PLV = 14, AIR_DYN_VAE_PLV = 15,
    AIR_DYN_COUNT    = 16
};

/* int state words (device int32 array `istate`) */
enum {
    AIR_IST_GLOBAL_STEP = 0,     /* air/global_step, air_model.py:69 */
    AIR_IST_COUNT = 4
};

/* one annealing schedule (air_model.py:94-121), evaluated on device each step */
typedef struct {
    int32_t slot;        /* AIR_DYN_* written                               */
    int32_t flags;       /* AIR_SCHED_* bits                                 */
    float init, iters, factor, vmin, vmax;
} air_schedule_t;
enum { AIR_SCHED_STAIRCASE = 1, AIR_SCHED_HAS_MIN = 2, AIR_SCHED_HAS_MAX = 4, AIR_SCHED_LOG = 8 };

/* ---- per-step records ---------------------------------------------------
 * att[t][b][AIR_ATT_STRIDE] -- per-item scalars of one time step. */
enum {
    AIR_ATT_S = 0, AIR_ATT_X = 1, AIR_ATT_Y = 2,     /* scale, shift  :301,318      */
    AIR_ATT_ZPRE = 3,                                /* z_pres_pre_sigmoid :380     */
    AIR_ATT_Z = 4,                                   /* z_pres (rounded if !train)  */
    AIR_ATT_ZPROB = 5,                               /* sigmoid(log_odds) :395      */
    AIR_ATT_KL_Z = 6, AIR_ATT_KL_SCALE = 7, AIR_ATT_KL_SHIFT = 8, AIR_ATT_KL_VAE = 9,
    AIR_ATT_MASK_PREV = 10,                          /* stopping_sum(old) < thr :412 */
    AIR_ATT_MASK = 11,                               /* stopping_sum(new) < thr :427 */
    AIR_ATT_ST_BACK = 12,                            /* 1/s, -x/s, -y/s  :353-356   */
    AIR_ATT_STRIDE = 16
};
/* out7[t][b][8]: scale_mean, scale_lv, shift_mean.x, .y, shift_lv.x, .y, z_log_odds, pad */
#define AIR_OUT_STRIDE 8

/* ---- GEMM (K1/K2/K5: LSTM, head and VAE MatMul + BiasAdd + activation) --------
 * C[M,N] (+)= epilogue( op(A)[M,K] . op(B)[K,N] )
 *   op(A)(m,k) = transA ? A[k*lda+m] : A[m*lda+k];  op(B)(k,n) = transB ? B[n*ldb+k] : B[k*ldb+n]
 * epilogue, in this order:  v = acc; v += bias[n]; v += addend[m*ldadd+n];
 *   v = act(v); v *= actgrad(aux[m*ldaux+n]); if (ACCUM) v += C[m*ldc+n].
 * Replaces tf.matmul + BiasAdd + Relu/Softplus/Sigmoid nodes of
 * layers.fully_connected (air_model.py:292-316, 374-376; vae.py:13-34), the
 * BasicLSTMCell MatMul (:286) and their MatMul_grad nodes.
 * Leading dimensions may be padded; one below the row it strides is AIR_EINVAL: lda < K (M with transA), ldb < N (K with
 * transB), ldc < N (2N for AIR_EPI_REPARAM_BWD, which writes 2N columns), and ldadd / ldaux < N when that operand is given.
 * (lda of the padded-A16 form of AIR_EPI_LSTM_FWD0 is the twin's stride and has its own rule, see A16 below.)
 * Pad columns are never read into the result and never written.
 * precision: 0 = exact-fp32 MFMA (v_mfma_f32_16x16x4_f32);
 *            1 = bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16). */
enum {
    AIR_ACT_NONE = 0, AIR_ACT_RELU = 1, AIR_ACT_SOFTPLUS = 2,
    AIR_ACT_SIGMOID_NOISE = 3   /* sigmoid(v + aux*aux_scale): vae.py:36-41 */
};
enum {
    AIR_GRAD_NONE = 0,
    AIR_GRAD_RELU = 1,          /* v *= (aux > 0)                        */
    AIR_GRAD_SOFTPLUS = 2       /* v *= 1 - exp(-aux)  (aux = softplus output) */
};
/* fused epilogues (the pointwise ops the reference runs right after the MatMul) */
enum {
    AIR_EPI_GENERIC = 0,
    /* BasicLSTMCell pointwise part (air_model.py:286): N = 4R gate columns i,j,f,o (groups of R);
     * pre-activation = acc + sum(addend slabs) + bias.  p0 = c_prev [M,R];
     * q0 = acts [M,4R] (sigmoid i, tanh j, sigmoid(f+1), sigmoid o), q1 = c [M,R], q2 = h [M,R]. */
    AIR_EPI_LSTM_FWD = 1,
    /* vae.py:16-24: N = 2Z (mean | log_var); C = ml [M,2Z]; p0 = eps [M,Z]; q0 = sample [M,Z]. */
    AIR_EPI_REPARAM_FWD = 2,
    /* LSTM backward: acc (+ addend) = d loss/d h' [M,R]; p0 = acts, p1 = c_prev, p2 = c,
     * p3 = d c' from the next step (nullable); q0 = dgates [M,4R], q1 = d c_prev [M,R],
     * q2 = running sum of dgates (nullable), i0 = accumulate into q2. */
    AIR_EPI_LSTM_BWD = 3,
    /* re-parameterisation backward + VAE-KL gradient (air_model.py:481-493): acc = d loss/d z;
     * p0 = ml [M,2Z], p1 = eps [M,Z], p2 = att, p3 = dyn; C = d_ml [M,2Z]. */
    AIR_EPI_REPARAM_BWD = 4,
    /* rows [0, i0): plain store of acc into C; rows [i0, M): AIR_EPI_LSTM_BWD of the LAST time step
     * (no d c' from a later step, q2 is stored not accumulated), with p0..p2 / q0..q2 indexed by
     * (row - i0).  Lets the GEMM that produces d h' of all steps also start the BPTT chain. */
    AIR_EPI_LSTM_BWD_TAIL = 5,
    /* The FIRST step of the recurrence in the GEMM that hoists x.Wx (zero_state, air_model.py:540: h_0 = c_0 = 0,
     * so [x, h].kernel = x.Wx): N = 4R; C [M,4R] receives the raw product (the addend of the later steps,
     * one slab), and q0 = acts, q1 = c, q2 = h of step 0 from acc + bias.  16-column tiles of four units x
     * four gates (untransposed operands, no split-K, no addend). */
    AIR_EPI_LSTM_FWD0 = 6
};
/* air_step_begin's work as a descriptor, so that a GEMM launch can carry it (air_gemm_t.step_job) */
typedef struct {
    const air_schedule_t* sched /*device*/; int32_t nsched; float* dyn; const int32_t* istate;
    float* normals; int64_t n_normal; float* uniforms; int64_t n_uniform; uint64_t seed;
    const float* twin_src; uint16_t* twin_dst; int64_t twin_n;   /* see air_step_begin */
} air_step_job_t;
typedef struct {
    const float* A; const float* B; float* C;
    int32_t M, N, K, lda, ldb, ldc;
    int32_t transA, transB;
    const float* bias;             /* [N] or NULL                        */
    const float* addend; int32_t ldadd;   /* [M,N] or NULL               */
    const float* aux;    int32_t ldaux;   /* [M,N] or NULL               */
    float   aux_scale;
    int32_t act;                   /* AIR_ACT_*                          */
    int32_t actgrad;               /* AIR_GRAD_*                         */
    int32_t accumulate;            /* C += result                        */
    int32_t precision;             /* 0 fp32, 1 bf16                     */
    int32_t epi;                   /* AIR_EPI_*                          */
    int32_t tile_m, tile_n;        /* output tile in units of 16 (0 = auto): (1,1)(1,2)(1,4)(2,2)(2,4)(4,1)(4,2)(4,4); (8,4) = the
                                      throughput tiling for a deep split-K product of an fp32 A with a bf16 B16 (M % 128, N % 64, K-slab % 64 == 0,
                                      ksplit > 1, generic epilogue; AIR_EINVAL / AIR_EALIGN otherwise -- callers fall back to (4,4)) */
    int32_t ksplit;                /* > 1: split K over grid.z; C receives `air_gemm_slabs()` slabs of
                                      [M,ldc] (plain stores, generic epilogue skipped)            */
    int32_t addend_slabs;          /* addend is that many [M,ldadd] slabs (0/1 = one)            */
    int32_t i0;                    /* AIR_EPI_LSTM_BWD_TAIL: first row.  AIR_EPI_LSTM_FWD0 with A16, a bit set: bit 1 (value 2) = A16 is the
                                      PADDED twin and lda ITS row stride (see A16 below); bit 0 (value 1) = with bit 1, stage the operands
                                      through registers instead of by 16-byte LDS-DMA (gemm_xwx_glds_kernel).  0 = an ordinary twin */
    const float* p0; const float* p1; const float* p2; const float* p3;
    float* q0; float* q1; float* q2;
    /* optional (HOST pointer, read during the call): the step prologue of air_step_begin is run by
     * an extra plane of workgroups of THIS launch.  Only for a GEMM that reads neither the noise nor
     * dyn (the hoisted x.Wx): the train step then has no separate prologue launch. */
    const air_step_job_t* step_job;
    /* bf16 TWINS (precision 1 only; each nullable).  A twin is the RNE-rounded bf16 copy of an fp32 array with the
     * same shape and leading dimension -- exactly what the kernel would have produced on the operand's way into
     * LDS, so results are bit-identical with and without them.  A16 / B16: twins of A / B; when B16 (and A16, or an
     * fp32 A) are given and aligned to 16 bytes the operands are read as bf16 (half the bytes through the CU,
     * no conversion; row-major weights through the LDS transpose read).  C16 / q0_16 / q2_16: twins the epilogue
     * writes next to C / q0 / q2 for the next consumer (q2_16 of AIR_EPI_LSTM_BWD: pass it with the LAST
     * accumulation into q2 only).
     * AIR_EPI_LSTM_FWD0 (its C, the raw x.Wx, has no consumer that wants a twin) REUSES two of these fields.  Both forms
     * exist in the bf16-twin kernels only: precision 1, untransposed operands, B16p (16-byte aligned), R = N/4 a
     * multiple of 8.  A descriptor that asks for one of them and does not meet this is REFUSED with AIR_EALIGN by
     * air_gemm and by air_gemm_kernel_name -- never served by another kernel:
     *   - with an fp32 A (A16 == NULL), C16 (nullable, 16-byte aligned) receives the PADDED bf16 twin of A as a side
     *     output: M rows of ldp = K rounded up to a multiple of 8 elements, element (m, k) = bf16(A[m, k]) (RNE), the
     *     columns K .. ldp - 1 zero -- every row starts 16-byte aligned although K % 8 != 0.  Also required: A 16-byte
     *     aligned, lda and K multiples of 4;
     *   - with A16 != NULL and i0 bit 1 (value 2) set, A16 IS such a padded twin and lda is ITS row stride, not A's (a
     *     multiple of 8, >= K rounded up to 8; A16 16-byte aligned; the pad columns must be zero): K itself may be
     *     ragged.  A must still be a valid pointer; it is not read.  C16 is ignored.
     * Without i0 bit 1 an A16 is an ordinary twin (same leading dimension as A, K % 8 == 0 for the twin kernels).
     * Results are bit-identical between all forms. */
    const uint16_t* A16; const uint16_t* B16;
    uint16_t* C16; uint16_t* q0_16; uint16_t* q2_16;
    /* PANEL-BLOCKED bf16 twin of an untransposed B = [K, N] (precision 1, nullable; air_panel_t below describes the
     * layout and who writes it): the same bf16 values as B16, stored as N/16 panels of [K rows][16 columns], so that a
     * 16-column output tile reads ONE contiguous 32*K-byte block instead of a 32-byte piece of every 2*ldb-byte row
     * (a quarter of each cache line it pulls through the CU).  For AIR_EPI_LSTM_FWD / AIR_EPI_LSTM_FWD0 (N = 4R gate
     * columns) the panels are the gate-interleaved ones (air_panel_t.gates = 4): panel p holds units 4p..4p+3, column
     * gate*4 + u%4 -- the four gates of four units in 32 contiguous bytes per row.  Read instead of B16 by the 16- and
     * 32-column tiles; results are bit-identical.  B16 may be NULL when B16p is given and the tile supports it. */
    const uint16_t* B16p;
} air_gemm_t;
/* number of K-slabs a ksplit request produces for contraction depth K */
int air_gemm_slabs(int K, int ksplit);
int air_gemm(const air_gemm_t* g, void* stream);
/* name of the kernel function `g` dispatches to, as rocprofv3 prints it.  Host-only, and the SAME decision as the launch:
 * both read one dispatch plan, so a descriptor air_gemm refuses (AIR_EINVAL / AIR_EALIGN / AIR_ELIMIT) gets that code here
 * instead of a name, and a name returned here is the kernel air_gemm launches */
int air_gemm_kernel_name(const air_gemm_t* g, char* buf, int n);

/* dst[i] = bf16(src[i]), round to nearest even: the twin of an array whose producer could not write it (the flat
 * variable buffer after a host-side load -- air_adam_clip_step keeps its shadow fresh afterwards). */
int air_bf16_twin(const float* src, uint16_t* dst, int64_t n, void* stream);

/* ---- panel-blocked bf16 shadows of row-major [K, N] weight matrices that live in a flat fp32 buffer ----------
 * Element (k, n) of the matrix at flat offset src_off goes to
 *   gates == 0:  dst_off + (n / 16) * (K * 16) + k * 16 + n % 16                  (ceil(N / 16) * K * 16 elements)
 *   gates == 4:  N = 4R gate columns (BasicLSTMCell's i, j, f, o blocks, air_model.py:286), gate = n / R, u = n % R:
 *                dst_off + (u / 4) * (K * 16) + k * 16 + gate * 4 + u % 4          (K * N elements, R % 4 == 0)
 * of the panel shadow (what air_gemm_t.B16p points into).  N % 4 == 0, src_off % 4 == 0, dst_off % 4 == 0.
 * `exclusive` != 0: the row-major bf16 shadow of this range is NOT maintained by air_adam_clip_step_panels (no kernel
 * reads it: the hoisted x.Wx is the only consumer of Wx and takes the panels). */
typedef struct {
    int64_t src_off, dst_off;
    int32_t K, N, gates, exclusive;
} air_panel_t;
#define AIR_MAX_PANELS 16
/* panel_shadow <- bf16(params), for every described matrix (after a host-side change of the variables) */
int air_panel_shadow(const float* params, uint16_t* panel_shadow, const air_panel_t* panels /*HOST array, <= 16, ascending src_off*/,
                     int count, void* stream);

/* ---- grouped weight gradients: every dW = A^T . dY (+ db = column sums of dY) of the
 * step in ONE launch (MatMul_grad / BiasAdd_grad nodes of all variables; weights are shared
 * across time steps so K = N_steps * B rows).  head_pack = 1 handles the 7 head output units:
 * A = d_out7 [K,8], dY = hid [K,HT], dW = wout [7][ldc] (unit o keeps only its head's hidden
 * segment), db = bout [7]. */
typedef struct {
    const float* A; const float* dY; float* dW; float* db /*nullable*/;
    int32_t M, N, K, lda, ldb, ldc;
    int32_t head_pack, Hs, Hh, Hz;
    /* bf16 twins of A / dY (precision 1, nullable, same leading dimensions; see air_gemm_t): a problem that has both
     * (8-byte aligned, lda/ldb/N multiples of 4, M a multiple of 4 or lda >= M rounded up to 4 -- padded rows --, not
     * head_pack) reads its operands as bf16 -- bit-identical dW.  Padded rows (M % 4 != 0, lda >= M rounded up to 4): the pad
     * columns of A and A16 must be READABLE but may hold anything, NaN included -- a piece that straddles M only feeds output
     * rows >= M, which are neither stored nor counted in sq_partials (tests/test_gpu_kernels.py::
     * test_wgrad_twins_of_padded_rows_ignore_what_the_pad_holds).
     * db is always summed from the fp32 dY. */
    const uint16_t* A16; const uint16_t* dY16;
} air_wgrad_t;
/* precision: 0 = fp32 MFMA (exact fp32 products), 1 = operands rounded to bf16, fp32 accumulate.
 * sq_partials (nullable): [air_wgrad_num_blocks()] floats receiving the sum of squares of every
 * gradient element each workgroup stored -- the tf.global_norm terms (air_model.py:673), handed to
 * air_adam_clip_step instead of a separate air_grad_sqnorm pass (single-GPU path; with data
 * parallelism the norm is taken after the all-reduce).  istate (nullable, only with sq_partials):
 * istate[GLOBAL_STEP] += 1, as air_grad_sqnorm does.  A plain problem may have dW == NULL when
 * sq_partials is given: its tiles are computed and squared but not stored (a caller that rebuilds the
 * gradient from its factors elsewhere). */
/* air_wgrad_num_blocks(): the number of global-norm partials = 64 x 64 tiles of all problems + one per bias column tile of
 * the problems with K >= 384 (their db is summed by workgroups of their own, the launch's first, instead of by a tile). */
int air_wgrad_num_blocks(const air_wgrad_t* probs, int count);
/* Workgroups air_wgrad_grouped(precision) launches for these problems: air_wgrad_num_blocks() unless a problem runs in
 * STRIPS -- at precision 1 a twin problem of >= 512 tiles (K = 64, 128, 192 or 256; 16-byte dY rows; M % 4 == 0) gives each
 * workgroup 2 (from 2048 tiles: 4) consecutive column tiles of a block-row, its A block fetched once and its MFMA fragments
 * kept in registers.  Values, db and the partials (still one per tile, at the same index) are bit-identical either way.
 * For a problem of >= 512 tiles (any precision) the tile that sums db of column tile nt is the one in block-row
 * nt % min(16, block-rows), not block-row 0.  Diagnostic. */
int air_wgrad_num_workgroups(const air_wgrad_t* probs, int count, int precision);
#define AIR_MAX_WGRAD_PROBLEMS 16
int air_wgrad_grouped(const air_wgrad_t* probs /*HOST array, <= AIR_MAX_WGRAD_PROBLEMS*/, int count, int precision,
                      float* sq_partials, int32_t* istate, void* stream);

/* column sums db[n] = sum_r dY[r*ld + n]  (BiasAdd_grad nodes) for `count` problems */
typedef struct { const float* src; float* dst; int32_t rows, cols, ld, accumulate; } air_colsum_t;
int air_colsum(const air_colsum_t* probs /*HOST array*/, int count, void* stream);

/* ---- LSTM gates (K1c) -- BasicLSTMCell pointwise part, air_model.py:286 -------
 * gates_pre [B,4R] = [x,h].kernel + bias, split order i,j,f,o; forget_bias 1.0.
 * acts [B,4R] receives sigmoid(i), tanh(j), sigmoid(f+1), sigmoid(o). */
int air_lstm_gates_fwd(const float* gates_pre, const float* c_prev, float* acts,
                       float* c, float* h, int B, int R, void* stream);
/* The first step of the loop: the LSTM starts from zero_state (air_model.py:540), so [x, h].kernel is the
 * hoisted x.Wx alone -- no MatMul.  xw_slabs: `nslabs` split-K slabs [B,4R] of x.Wx (air_gemm ksplit);
 * pre-activation = slab sum (in slab order) + bias, i.e. AIR_EPI_LSTM_FWD with a zero accumulator. */
int air_lstm_first_step(const float* xw_slabs, int nslabs, const float* bias /*nullable*/, float* acts,
                        float* c, float* h, uint16_t* h16 /*bf16 twin of h, nullable*/, int B, int R, void* stream);
/* dgates [B,4R] (pre-activation grads), dc_prev [B,R]; dgsum (+)= dgates when given */
int air_lstm_gates_bwd(const float* dh, const float* dc_in /*nullable*/, const float* acts,
                       const float* c_prev, const float* c, float* dgates, float* dc_prev,
                       float* dgsum /*nullable*/, int dgsum_accumulate, int B, int R, void* stream);

/* ---- spatial transformer, generic (transformer.py:18-175) ---------------------
 * out[B,Ho,Wo] = transformer(U[B,Hi,Wi,1], theta[B,2,3], (Ho,Wo)); literal
 * 4-product / add_n op order, indices clipped before the weights. */
int air_transformer_fwd(const float* U, const float* theta, float* out,
                        int B, int Hi, int Wi, int Ho, int Wo, void* stream);
/* its gradient (what tf.gradients builds for transformer.py:56-171): d_U [B,Hi,Wi] and / or d_theta [B,2,3]
 * (either may be NULL) from d_out [B,Ho,Wo].
 *   d_U: ONE fp32 accumulator per input pixel that receives the a-, b-, c-, d-tap terms in output-pixel order -- the
 *        graph's single UnsortedSegmentSum over the concatenated Gather gradients -- BIT-IDENTICAL to the executed
 *        reference graph (oracle.transformer_backward, tests/test_gpu_kernels.py).
 *   d_theta: per output pixel the graph's AddN order for the coordinate gradients; the contraction over the output
 *        pixels with (x_t, y_t, 1) (MatMul_grad) is a per-thread strided sum followed by a fixed-order block reduction,
 *        i.e. it matches the graph up to the reduction order of that one sum: tested to 2e-5 of the largest element.
 * Hi*Wi <= ~20 000 (U and d_U of one image live in LDS). */
int air_transformer_bwd(const float* U, const float* theta, const float* d_out, float* d_U, float* d_theta,
                        int B, int Hi, int Wi, int Ho, int Wo, void* stream);

/* ---- spatial transformer on multi-channel inputs, several transforms per image (transformer.py:18-175 with
 * num_channels = C, and batch_transformer :178-195) -----------------------------
 * U [B,Hi,Wi,C], channels innermost and contiguous as the reference lays it out; theta [B*T,2,3]; out [B*T,Ho,Wo,C].
 * Row b*T+t samples image b with theta[b*T+t]: T = 1 is transformer, T > 1 is batch_transformer, whose tf.gather copy of
 * the input (:193-194) is never made.  Any C >= 1, T >= 1.
 * The tap coordinates and the four weights of an output pixel are computed once, in the op sequence of
 * air_transformer_fwd (indices clipped before the weights, no contraction); every channel then gets
 * ((wa*Ia + wb*Ib) + wc*Ic) + wd*Id.  Channel c of `out` is BIT-IDENTICAL to air_transformer_fwd on the channel-c plane.
 * 16-byte loads and stores when C % 4 == 0 and U / out are 16-byte aligned, scalar ones otherwise. */
int air_transformer_nc_fwd(const float* U, const float* theta, float* out,
                           int B, int T, int Hi, int Wi, int C, int Ho, int Wo, void* stream);
/* its gradient: d_U [B,Hi,Wi,C] and / or d_theta [B*T,2,3] (either may be NULL) from d_out [B*T,Ho,Wo,C].
 *   d_U, T = 1: im_flat is [B*H*W, C] (:100) and the four Gather gradients carry rows of C values into ONE
 *        UnsortedSegmentSum: per channel, one fp32 accumulator per input pixel that receives its a-terms in output-pixel
 *        order, then b, c, d.  Channel c of d_U is BIT-IDENTICAL to air_transformer_bwd on plane c, and so to the executed
 *        reference graph.
 *   d_U, T > 1: the gradient of the tf.gather replication is one more sequential UnsortedSegmentSum over the rows: each
 *        row's d_U is first completed from zero as above, then d_U[b] = ((row b*T+0) + row b*T+1) + ... in fp32,
 *        ascending t.  NOT one accumulator carried across the transforms (the two orders differ in the last bits).
 *   d_theta: the weights are shared by the channels, so the graph reduces g*I over the channel axis before the AddN legs:
 *        ga = sum_c g_c*Ia_c in fp32 in ascending c, starting from the c = 0 product (gb, gc, gd alike); then the
 *        dX / dY / truediv / mul sequence and the contraction with (x_t, y_t, 1) of air_transformer_bwd -- at C = 1 the same
 *        bits, and like it equal to the graph up to the reduction order of that one contraction.
 * Deterministic: no global atomics.  Hi*Wi keeps the bound of air_transformer_bwd (~20 000 pixels: AIR_ELIMIT beyond, when a
 * single channel's planes cannot fit); the channels are taken in groups whose planes fit the LDS at once, one wave per
 * channel, so any C works.  AIR_EINVAL: a null U / theta / d_out, both outputs null, a size < 1.  Both are answered on the
 * host before any launch.  The lane-order probe and its behaviour under stream capture are air_transformer_bwd's. */
int air_transformer_nc_bwd(const float* U, const float* theta, const float* d_out,
                           float* d_U /*nullable*/, float* d_theta /*nullable*/,
                           int B, int T, int Hi, int Wi, int C, int Ho, int Wo, void* stream);

/* ---- "attend": heads output layer + sampling + KLs + stop logic + ST read -----
 * air_model.py:288-333 (scale/shift heads, theta, transformer canvas->window) and
 * :368-427 (z_pres head, Concrete sample, z KL, stopping_sum masks), :441-477
 * (scale/shift KL) for ALL N time steps at once: one workgroup per (image, step).
 * The LSTM input is the same image every step (:286, :535), so h' of every step
 * exists before the heads run; the stopping sum is re-derived per block in step
 * order (bitwise equal to the sequential loop).
 * hid [N,B,HT] = ReLU hidden activations of the 5 heads, concatenated in the order
 * scale/mean, scale/log_variance, shift/mean, shift/log_variance, z_pres/log_odds
 * with widths Hs,Hs,Hh,Hh,Hz (HT = 2Hs+2Hh+Hz).  wout [7][wout_ld] holds one row
 * per output unit, bout [7].
 * wout_ld is the row stride of wout in floats: wout_ld >= max(Hs, Hh, Hz), AIR_EINVAL otherwise (air_attend_fwd,
 * air_attend_bwd and air_heads_out_wgrad alike).  It may be padded beyond the widest head: the pad is copied with the
 * rows but never enters a product, whatever it holds.  air_attend_fwd keeps all 7 * wout_ld floats in LDS next to
 * 17 * HT + 8 * w + ~40 floats and, for C * C <= 2560, the canvas: AIR_ELIMIT beyond 160 KB. */
typedef struct {
    const float* hid; const float* wout; const float* bout;
    const float* canvas;                 /* input_images [B,C*C]            */
    const float* eps_scale; const float* eps_shift; const float* u;   /* [N,B,1],[N,B,2],[N,B] */
    const float* dyn;                    /* AIR_DYN_* device array          */
    float* out7;                         /* [N,B,8]                         */
    float* att;                          /* [N,B,AIR_ATT_STRIDE]            */
    float* window;                       /* [N,B,w*w]                       */
    int32_t B, N, C, w, Hs, Hh, Hz, wout_ld, train;
    uint16_t* window16;                  /* bf16 twin of window (nullable): A operand of the first recognition GEMM */
} air_attend_fwd_t;
int air_attend_fwd(const air_attend_fwd_t* a, void* stream);

typedef struct {
    const float* hid; const float* wout;
    const float* canvas; const float* eps_scale; const float* eps_shift;
    const float* dyn; const float* out7; const float* att;
    const float* d_window;               /* [N,B,w*w] grad wrt the glimpse  */
    const float* d_sxy_write;            /* [N,B,4]: ds,dx,dy,dz from the write path */
    float* d_hid;                        /* [N,B,HT] grad wrt pre-ReLU hidden */
    float* d_out7;                       /* [N,B,8]                         */
    int32_t B, N, C, w, Hs, Hh, Hz, wout_ld;
    int32_t literal;                     /* 0: exact adjoint.
                                            2: the op order of the reference's saved graph (model/air-model.meta):
                                               AddN_10/11 (AddN_20/21) input order for the coordinate gradients and,
                                               in air_write_bwd, ONE fp32 accumulator per window pixel through the four
                                               concatenated Gather gradients (the graph's single UnsortedSegmentSum) --
                                               keeps the out-of-range rounding residue, bit-identical to the executed graph.
                                            (air_attend_bwd: any non-zero value selects the graph order)               */
    uint16_t* d_hid16;                   /* bf16 twin of d_hid (nullable)   */
} air_attend_bwd_t;
int air_attend_bwd(const air_attend_bwd_t* a, void* stream);

/* grads of the 7 output units: dwout[o][j] = sum_{r} d_out7[r][o]*hid[r][seg(o)+j],
 * dbout[o] = sum_r d_out7[r][o]; rows = N*B */
int air_heads_out_wgrad(const float* d_out7, const float* hid, float* dwout, float* dbout,
                        int rows, int Hs, int Hh, int Hz, int wout_ld, void* stream);

/* ---- VAE re-parameterisation (vae.py:22-24) ---------------------------------- */
int air_reparam_fwd(const float* ml /*[B,2Z] mean|log_var*/, const float* eps_z, float* zs,
                    int B, int Z, void* stream);
/* d_ml [B,2Z] from d_zs [B,Z] plus the VAE-KL gradient (air_model.py:481-493) */
int air_reparam_bwd(const float* d_zs, const float* ml, const float* eps_z, const float* att,
                    const float* dyn, float* d_ml, int B, int Z, void* stream);

/* ---- "write"/compose: ST window->canvas for all N steps + z_pres scaling + masked
 * accumulate (in step order, in registers) + VAE KL + running loss + digit count +
 * reconstruction loss and its gradient.  air_model.py:351-366 (theta_recon,
 * transformer), :409-439 (masks, running_recon), :479-496 (VAE KL), :580-593 (loss).
 * One workgroup per image. */
/* the pixel likelihood of the reconstruction loss (air_write_fwd_t.likelihood; additive to ABI 6).  With R the running
 * reconstruction of a pixel, r = min(max(R, 0), 1) the reported reconstruction, x the image pixel, gsc = dyn[AIR_DYN_GRAD_SCALE]
 * and pass = (R <= 1 && min(R, 1) >= 0) (Minimum / Maximum pass their gradient at ties):
 *   AIR_LIK_BERNOULLI  the reference's cross-entropy :586-589:  rec_loss = -sum_p x log(r + 1e-9) + (1 - x) log(1 - r + 1e-9),
 *                      d_recon = pass ? -gsc * (x / (r + 1e-9) - (1 - x) / (1 - r + 1e-9)) : 0
 *   AIR_LIK_GAUSSIAN   the AIR paper's Gaussian with mean r and fixed sigma = dyn[AIR_DYN_LIK_STD] (> 0; read on the device):
 *                      rec_loss = (0.5 / sigma^2) * sum_p (x - r)^2 + C * C * (log sigma + 0.5 log 2 pi)   -- a density: may be < 0;
 *                      d_recon = pass ? gsc * (r - x) / sigma^2 : 0, so |d_recon| <= gsc / sigma^2 on every canvas */
enum { AIR_LIK_BERNOULLI = 0, AIR_LIK_GAUSSIAN = 1 };
typedef struct {
    const float* vrec;                   /* vae reconstructions [N,B,w*w]   */
    const float* ml;                     /* [N,B,2Z] mean | log_var         */
    const float* images;                 /* [B,C*C]                         */
    const float* dyn;
    float* att;                          /* [N,B,16]: reads s,x,y,z,masks,KLs; writes KL_VAE */
    float* recon;                        /* [B,C*C] clipped reconstruction  */
    float* rec_loss;                     /* [B]                             */
    float* d_recon;                      /* [B,C*C] d loss/d running_recon, nullable */
    float* run_loss;                     /* [B] sum of masked KLs (running_loss) */
    int32_t* run_digits;                 /* [B] rec_num_digits              */
    float* loss_item;                    /* [B] run_loss + rec_loss         */
    int32_t B, N, C, w, Z;
    /* nullable, [N*B] (N*B <= 4096): one extra workgroup of this launch sorts the (image, step) items by the work the
     * graph-order write backward will have with them (its corner terms; inactive items last) and leaves the permutation
     * here -- air_write_bwd_t.order.  Worth it when there are more items than CUs (128 x 128, b = 256: 1280 items). */
    int32_t* wb_order;
    int32_t likelihood;                  /* AIR_LIK_*; 0 (a zero-filled field) is the Bernoulli path, AIR_LIK_GAUSSIAN launches
                                            write_fwd_gauss_kernel; any other value: AIR_EINVAL */
} air_write_fwd_t;
int air_write_fwd(const air_write_fwd_t* a, void* stream);

/* one workgroup per (image, step): all steps see the same d loss / d canvas */
typedef struct {
    const float* d_recon;                /* [B,C*C]                         */
    const float* vrec; const float* att; /* [N,B,w*w], [N,B,16]             */
    float* d_gen_pre;                    /* [N,B,w*w] grad wrt gen_mean pre-sigmoid input */
    float* d_sxy_write;                  /* [N,B,4]: ds,dx,dy (via theta_recon), dz */
    int32_t B, N, C, w;
    int32_t literal;                     /* 0, 2: see air_attend_bwd_t.  air_write_bwd only:
                                            4: as 2 for every window pixel whose four term streams have at most 64 terms each
                                               (all but the four corners and a few long borders); a pixel with a longer stream
                                               has every tap's stream cut into at most 16 chunks of at least 64 terms and walks
                                               each chunk TWICE -- C_k from +0.0, Q_k from P_k = the running sum of the earlier
                                               C's -- and returns Q_last + sum_{k < last} (Q_k - P_k+1), the (exact) differences
                                               added left to right: every add of the Q chains rounds at the magnitude it has in
                                               the one long chain of 2, and nothing else does (backward="reference_carried"; no
                                               LDS atomics, no probe).  The coordinate / z gradients d_sxy_write of 4 are
                                               per-column thread sums in the graph's AddN order per pixel (rows whose y taps clip
                                               to one index are exact zeros and skipped): equal to 2's to ~1e-7 relative, not bit
                                               for bit -- pinned against the executed graph's tensors by
                                               tests/test_gpu_graph_golden.py.
                                            (1, the per-tap order, and 3, chunks from +0.0 added left to right, were removed
                                             with ABI 5: measured to train worse, DESIGN.md section 10.1.  AIR_EINVAL.)      */
    /* optional: workgroup (0,0) also does air_finalize's batch means (train step: saves a launch).
     * fin_scalars == NULL disables; loss_item is the [B] output of air_write_fwd */
    const float* fin_loss_item; const int32_t* fin_targets; const int32_t* fin_digits;
    float* fin_scalars;
    uint16_t* d_gen_pre16;               /* bf16 twin of d_gen_pre (nullable) */
    /* nullable (literals 2 and 4; AIR_EINVAL with literal 0): workgroup i of the launch computes item order[i] = t * B + b instead of item i -- the
     * longest-first permutation of air_write_fwd_t.wb_order (the hardware hands workgroups out in launch order).  Results
     * do not depend on it.  With `order` the batch-mean finisher is the LAST workgroup of the launch. */
    const int32_t* order;
} air_write_bwd_t;
int air_write_bwd(const air_write_bwd_t* a, void* stream);
/* the kernel function air_write_bwd dispatches this descriptor to, as rocprofv3 prints it (profiling tools) */
int air_write_bwd_kernel_name(const air_write_bwd_t* a, char* buf, int n);

/* air_write_fwd(f) followed by air_write_bwd(b) as ONE launch, every output bit for bit that of the two: a workgroup of
 * the write backward builds d loss / d canvas of its image itself, the workgroup of step 0 stores the image's forward
 * outputs (d_recon included), and the owner workgroup that finishes last computes the batch means.  The pair must describe
 * one train step: b->d_recon / vrec / att / fin_loss_item / fin_digits are f's d_recon / vrec / att / loss_item /
 * run_digits, equal B, N, C, w, f->d_recon and all four b->fin_* given (AIR_EINVAL otherwise, and for b->literal != 2).
 * The form exists where all four taps' terms of the write backward are resident in LDS, compose's scratch fits over
 * them, N * B <= 256 without f->wb_order / b->order, and f->likelihood == AIR_LIK_BERNOULLI (the fold has not been taught
 * another likelihood): AIR_ELIMIT otherwise -- the caller keeps its two launches.
 * N * B <= 256 is an ASSUMPTION about placement, not a guarantee: the hand-off of the batch means uses agent-scope
 * relaxed stores and loads in place of a release / acquire pair, a form measured with one workgroup per CU on a 256-CU
 * part.  The launch asks for under half a CU's LDS, so on a part with fewer CUs, or beside another stream's work, two of
 * its workgroups can share a CU -- a setting that form has not been measured in.
 * `arrive`: one device word, zero before the first call; every call leaves it zero.  Calls that share it must not overlap.
 * Like air_write_bwd, call it once eagerly before capturing it (the accumulator probe). */
int air_write_fwd_bwd(const air_write_fwd_t* f, const air_write_bwd_t* b, int32_t* arrive, void* stream);
/* the kernel function air_write_fwd_bwd dispatches this pair to, as rocprofv3 prints it; the code air_write_fwd_bwd
 * returns for a pair it refuses (both read one host-side plan: no GPU is touched) */
int air_write_fwd_bwd_kernel_name(const air_write_fwd_t* f, const air_write_bwd_t* b, char* buf, int n);

/* ---- VAE bottleneck, one launch per direction (vae.py:16-34) ------------------
 * Forward = the last recognition product and the first generative layer:
 *   ml [M,2Z] = X [M,K1].Wml [K1,2Z] + bml  (mean | log-variance, vae.py:16-20)
 *   z  [M,Z]  = mean + eps * sqrt(exp(lv))                          (vae.py:22-24)
 *   g  [M,H]  = softplus(z.Wg [Z,H] + bg)                           (vae.py:26-30)
 * i.e. air_gemm(AIR_EPI_REPARAM_FWD) followed by air_gemm(bias, AIR_ACT_SOFTPLUS) without the second
 * launch and without z's round trip through memory.  Operands are rounded to bf16 for the MFMAs
 * (as air_gemm precision 1 does), accumulation is fp32.
 * Backward = their data gradients:
 *   d_z = dG [M,H].Wg^T; d_ml [M,2Z] as AIR_EPI_REPARAM_BWD writes it (ml, eps, att mask, dyn);
 *   d_x [M,K1] = (d_ml.Wml^T) * softplus'(x)    (x = the saved activation X, AIR_GRAD_SOFTPLUS)
 * Limits: K1 == 256 (forward) / H == 256 (backward), Z <= 64 and even, 16-byte aligned operands;
 * AIR_ELIMIT / AIR_EALIGN otherwise (callers fall back to the two air_gemm launches). */
typedef struct {
    const float* X; const float* Wml; const float* bml; const float* eps; const float* Wg; const float* bg;
    float* ml; float* z; float* g;
    int32_t M, K1, Z, H, ldx;
    uint16_t* z16; uint16_t* g16;        /* bf16 twins of z / g written next to them (nullable) */
    const uint16_t* X16; const uint16_t* Wml16; const uint16_t* Wg16;   /* bf16 twins of the three operands (all or none;
                                          * X16 16-byte aligned with ldx % 8 == 0, the weights 8-byte aligned): read instead of
                                          * the fp32 arrays, same results */
    int32_t exact_fp32;                  /* 1: exact fp32 products (v_mfma_f32_16x16x4_f32) on the fp32 operands -- the fp32
                                          * path; twins ignored / not written; additionally 2 Z <= 104 */
    int32_t ldz;                         /* row stride of z and z16 in elements; 0 = Z.  A stride that is a multiple of 4
                                          * (Z = 50 -> 52) lets the weight gradient of the first generative layer read z's
                                          * twin in 8-byte pieces (air_wgrad_t: lda % 4 == 0, lda >= M rounded up to 4).  Only
                                          * columns < Z of a row are written: the pad keeps what the caller put there */
} air_bottleneck_fwd_t;
typedef struct {
    const float* dG; const float* Wg; const float* ml; const float* eps;
    const float* att;                    /* [M, AIR_ATT_STRIDE]: AIR_ATT_MASK gates the KL gradient */
    const float* dyn; const float* Wml; const float* x;
    float* d_ml; float* d_x;
    int32_t M, K1, Z, H;
    uint16_t* d_ml16; uint16_t* d_x16;   /* bf16 twins of d_ml / d_x written next to them (nullable) */
    const uint16_t* dG16; const uint16_t* Wg16; const uint16_t* Wml16;  /* bf16 twins of the three operands (all or none) */
    int32_t exact_fp32;                  /* as in air_bottleneck_fwd_t */
} air_bottleneck_bwd_t;
int air_vae_bottleneck_fwd(const air_bottleneck_fwd_t* a, void* stream);
int air_vae_bottleneck_bwd(const air_bottleneck_bwd_t* a, void* stream);

/* ---- reconstruction loss (air_model.py:580-593) + its gradient ---------------- */
int air_bce_fwd_bwd(const float* images, const float* run_recon, const float* dyn,
                    float* recon /*clipped [B,D]*/, float* rec_loss /*[B]*/,
                    float* d_recon /*[B,D] nullable*/, int B, int D, void* stream);
/* its twin under AIR_LIK_GAUSSIAN (the formulas above air_write_fwd_t; sigma = dyn[AIR_DYN_LIK_STD]); additive to ABI 6 */
int air_gauss_nll_fwd_bwd(const float* images, const float* run_recon, const float* dyn,
                          float* recon /*clipped [B,D]*/, float* rec_loss /*[B]*/,
                          float* d_recon /*[B,D] nullable*/, int B, int D, void* stream);
/* loss = mean(run_loss + rec_loss), accuracy = mean(target == digits)  (:597-611)
 * scalars[0] = loss, scalars[1] = accuracy */
int air_finalize(const float* run_loss, const float* rec_loss, const int32_t* targets,
                 const int32_t* digits, float* loss_per_item, float* scalars, int B, void* stream);

/* ---- step prologue: annealing schedules + Philox noise ------------------------
 * Evaluates `nsched` schedules at istate[GLOBAL_STEP] into dyn, and fills
 * normals[n_normal] ~ N(0,1), uniforms[n_uniform] ~ U[0,1) from
 * Philox4x32-10(key = seed, counter = (index, global_step + call_salt)).  Optionally also writes
 * twin_dst[i] = bf16(twin_src[i]), i < twin_n: the bf16 twin of the image batch (the caller's fp32 tensor; it has no
 * producing kernel of ours) that the input-weight gradient reads at the end of the step (air_wgrad_t.A16). */
int air_step_begin(const air_schedule_t* sched /*device*/, int nsched, float* dyn,
                   const int32_t* istate, float* normals, int64_t n_normal,
                   float* uniforms, int64_t n_uniform, uint64_t seed,
                   const float* twin_src /*nullable*/, uint16_t* twin_dst, int64_t twin_n, void* stream);

/* ---- optimizer (air_model.py:651-694): clip_by_global_norm + TF1.3 ApplyAdam --
 * partials: scratch [>= air_optim_num_partials(n)] floats.
 * air_grad_sqnorm also increments istate[GLOBAL_STEP] (apply_gradients, :692). */
int air_optim_num_partials(int64_t n);
int air_grad_sqnorm(const float* grads, int64_t n, float* partials, int32_t* istate, void* stream);
int air_adam_clip_step(float* params, const float* grads, float* m, float* v, int64_t n,
                       const float* partials, int npartials, const float* dyn, const int32_t* istate,
                       float grad_prescale /* e.g. 1/world_size */, float beta1, float beta2,
                       float epsilon, uint16_t* bf16_shadow /*nullable*/, float* gnorm_out /*nullable*/,
                       void* stream);
/* air_adam_clip_step that ALSO maintains the panel-blocked shadows: every updated variable that lies
 * in a described matrix is written to its panel position (and to bf16_shadow unless the matrix is `exclusive`). */
int air_adam_clip_step_panels(float* params, const float* grads, float* m, float* v, int64_t n,
                              const float* partials, int npartials, const float* dyn, const int32_t* istate,
                              float grad_prescale, float beta1, float beta2, float epsilon,
                              uint16_t* bf16_shadow /*nullable*/, const air_panel_t* panels /*HOST array*/, int npanels,
                              uint16_t* panel_shadow, float* gnorm_out /*nullable*/, void* stream);

/* ---- input pipeline: tf.train.shuffle_batch on the device (the reference's multi_mnist.py:228-249) -------------
 * A RandomShuffleQueue of `capacity` record indices resident in HBM over the epoch-repeating record stream
 * 0, 1, .., n_records-1, 0, 1, ..  (string_input_producer([file], num_epochs) + ONE TFRecordReader: file order, every
 * epoch the same -- training.py:76-81).  The reader threads are far faster than a train step, so the queue is modelled AT
 * CAPACITY whenever a batch is taken.  air_shuffle_batch_dequeue then does what RandomShuffleQueue::TryDequeueMany does
 * for each of the `batch` elements in turn:  index = r_k mod size;  emit queue[index];  queue[index] = queue[size-1];
 * size -= 1  (uniform pick, swap with the back, pop) -- and the `batch` freed slots at the back are refilled from the
 * stream in order (enqueue appends at the back).  r_k = word k mod 4 of Philox4x32-10(key = seed, counter = (dequeue
 * number lo, hi, k / 4, 0x53485546)).  TF's own queue is unseeded here (seed 0 -> nondeterministic): the distribution is
 * the contract, and tests/test_shuffle_queue.py holds a numpy model of the queue that this kernel matches pick for pick.
 * state[0] = records enqueued so far (the stream position), state[1] = batches dequeued so far.
 * One workgroup per call; the picks of a batch are resolved in parallel (the content of a slot at pick k is found by walking
 * the earlier picks of the batch backwards: csrc/air_input.hip), the same picks as the sequential queue.  Limits:
 * capacity * 4 + batch * 8 <= 48 KB (capacity 10 640, batch 64: 43 KB -- air_shuffle_batch_dequeue_many stages the queue
 * in LDS), batch a multiple of 4 and <= 1024, capacity - batch >= min_after_dequeue >= 0 (the reference: 10 000).  No
 * allocation, no synchronisation;
 * both calls are stream work and capturable. */
typedef struct {
    int32_t* queue;            /* [capacity] record indices in the queue */
    int64_t* state;            /* [2] */
    int32_t* picks;            /* [batch] out: the records of this batch, in dequeue order */
    int32_t capacity, batch, min_after_dequeue, n_records;
    uint64_t seed;
} air_shuffle_batch_t;
/* queue <- the first `capacity` records of the stream, state <- (capacity, 0) */
int air_shuffle_batch_init(const air_shuffle_batch_t* q, void* stream);
int air_shuffle_batch_dequeue(const air_shuffle_batch_t* q, void* stream);
/* `n_batches` consecutive dequeues in one launch, pick for pick what n_batches calls of air_shuffle_batch_dequeue make:
 * picks_out[k * batch + i] = pick i of the k-th of them (q->picks is not written).  In training.py it is the first launch
 * of every hipGraph replay of n_batches train steps, whose row gathers read picks_out (multi_mnist.ShuffleBatchQueue). */
int air_shuffle_batch_dequeue_many(const air_shuffle_batch_t* q, int n_batches, int32_t* picks_out, void* stream);
/* the decoded tensors of a dequeued batch (read_and_decode, multi_mnist.py:228-238, after the queue):
 * out_images[i] = images[picks[i]] ([batch, D] fp32 rows, D % 4 == 0, 16-byte aligned), out_digits[i] = digits[picks[i]]
 * (out_digits / digits nullable together). */
int air_batch_gather(const float* images, const int32_t* digits, const int32_t* picks, float* out_images,
                     int32_t* out_digits, int batch, int D, void* stream);

/* ---- numeric summaries (the reference's air_model.py:160-209, 608-632; evaluated by training.py:169-200 on the test
 * model every 50 iterations) as one launch over the outputs of a forward pass --------------------------------------
 * out[0] = loss, out[1] = accuracy (copies of `scalars`), then one ROW of max_digits + 2 masked means per summarised
 * quantity -- the images with exactly 0 .. max_digits target digits, then all images ("_<i>_dig", "_all_dig"; an empty
 * group is NaN as tf.reduce_mean of an empty tensor) -- in the order the reference appends them:
 *   rows 0..3          steps (= rec_num_digits as float), rec_loss, digit_acc (digits == targets), total_loss (loss_item)
 *   rows 4 + q * N + i quantity q of step i + 1, q = scale, z_pres_prob (all_steps=True), z_pres_kl (one_more_step=True),
 *                      scale_kl, shift_kl, vae_kl; masked to the images with rec_num_digits > i (> i - 1: one_more_step; no
 *                      mask: all_steps); a step the while_loop did not reach (i >= T', derived from AIR_ATT_MASK) is the
 *                      zero padding of :187.
 * air_summaries_count(N, max_digits) = 2 + (4 + 6 N)(max_digits + 2) floats.  N <= 16, max_digits <= 6.  Stream work,
 * capturable, deterministic (fp64 sums in a fixed order, rounded once). */
#define AIR_MAX_STEPS_SUMMARY 16
typedef struct {
    const float* att;            /* [N,B,AIR_ATT_STRIDE] of the pass */
    const int32_t* targets;      /* [B] target_num_digits */
    const int32_t* digits;       /* [B] rec_num_digits */
    const float* rec_loss;       /* [B] reconstruction_loss */
    const float* loss_item;      /* [B] loss before the batch mean (:598-600) */
    const float* scalars;        /* [2] loss, accuracy (air_finalize) */
    float* out;                  /* [air_summaries_count(N, max_digits)] */
    int32_t B, N, max_digits;
} air_summaries_t;
int air_summaries_count(int N, int max_digits);
int air_summaries(const air_summaries_t* a, void* stream);

/* ---- generation: scenes from the priors, or from latents the caller supplies (additive to ABI 5) -----------------
 * The generative half of the reference's loop body with the posterior heads replaced by the priors: no image, no LSTM, no
 * recognition network.  Three launches around the decoder GEMMs (air_gemm with the forward's descriptors: the generative
 * layers, then gen_mean with AIR_ACT_SIGMOID_NOISE, vae.py:26-41):
 *   air_philox_fill -> air_scene_records -> [air_gemm ...] -> air_render.
 *
 * air_scene_records: ONE launch writes the att records of all (step, image) pairs and the latents the first generative
 * GEMM reads.  given == 0 (sample): the four sources are NOISE, eps_scale [N,B], eps_shift [N,B,2], eps_z [N,B,Z] ~ N(0,1)
 * and u [N,B] ~ U[0,1), and
 *   scale = sigmoid(SCALE_PM + sqrt(SCALE_PV) * eps)         (air_model.py:300-303 on the prior of :441-447)
 *   shift = tanh(SHIFT_PM + sqrt(SHIFT_PV) * eps)            (:317-320, :460-466)
 *   z_what = VAE_PM + sqrt(VAE_PV) * eps                     (vae.py:22-24 on the prior of air_model.py:479-485)
 *   z_pres = round(sigmoid((PRIOR_LOG_ODDS + log(u + 1e-9) - log(1 - u + 1e-9)) / TEMPERATURE))
 *            (concrete.py:20-27 on the prior the KL of air_model.py:398-407 is taken against, rounded as :389-390)
 * with the prior parameters read from the live `dyn` slots.  given != 0: the sources ARE scales [N,B], shifts [N,B,2],
 * latents [N,B,Z] and z_pres [N,B] (used as given: it may be relaxed); AIR_ATT_ZPRE is 0.  Either way the stopping sum is
 * re-derived per image in step order (:409-427: S += 1 - z_pres; MASK_PREV / MASK = S < STOP_THRESHOLD before / after),
 * AIR_ATT_ST_BACK is (1/s, -x/s, -y/s, 0) (:353-356), and AIR_ATT_ZPROB and the four KL slots are 0.
 * z [N,B,ldz] (ldz >= Z; columns Z .. ldz-1 are written as 0) and its bf16 twin z16 (nullable, same stride). */
#define AIR_MAX_STEPS 16
typedef struct {
    const float* scale_src;              /* [N,B]   eps_scale | scales   */
    const float* shift_src;              /* [N,B,2] eps_shift | shifts   */
    const float* z_src;                  /* [N,B,Z] eps_z     | latents  */
    const float* pres_src;               /* [N,B]   u         | z_pres   */
    const float* dyn;                    /* AIR_DYN_* device array       */
    float* att;                          /* [N,B,AIR_ATT_STRIDE], 16-byte aligned */
    float* z;                            /* [N,B,ldz]                    */
    uint16_t* z16;                       /* bf16 twin of z (nullable)    */
    int32_t B, N, Z, ldz, given;
} air_scene_records_t;
int air_scene_records(const air_scene_records_t* a, void* stream);

/* air_render: the compose kernel without a loss -- canvas [B,C*C] = clip(sum_t [MASK_t] z_pres_t *
 * transformer(window_t, theta_recon_t, [C,C]), 0, 1) in step order (air_model.py:351-366, 429-439, 582), num_digits [B] =
 * sum_t MASK_t (:427), from the records `att` and the decoded windows vrec [N,B,w*w].  One workgroup per image; the
 * per-pixel arithmetic IS air_write_fwd's (shared device code): on the same att / vrec the canvas equals its `recon` bit
 * for bit.  N <= AIR_MAX_STEPS; the taps and windows of one image live in LDS (<= 160 KB: AIR_ELIMIT beyond). */
typedef struct {
    const float* vrec;                   /* [N,B,w*w]                    */
    const float* att;                    /* [N,B,AIR_ATT_STRIDE]         */
    float* canvas;                       /* [B,C*C]                      */
    int32_t* num_digits;                 /* [B]                          */
    int32_t B, N, C, w;
} air_render_t;
int air_render(const air_render_t* a, void* stream);

/* normals[n_normal] ~ N(0,1), uniforms[n_uniform] ~ U[0,1) from the generator of air_step_begin, Philox4x32-10(key = seed,
 * counter = (index, call)) under a salt of its own: no schedules, no global_step (a test model's never moves) -- the
 * caller counts its calls.  The same (seed, call) gives the same numbers; either count may be 0, not both. */
int air_philox_fill(float* normals, int64_t n_normal, float* uniforms, int64_t n_uniform,
                    uint64_t seed, uint64_t call, void* stream);

/* Dynamic LDS, in bytes per workgroup, of the launches of a step whose need grows with the hyper-parameters, from the
 * functions the entry points themselves size their launches with (no GPU is touched): N steps, a C x C canvas, w x w
 * windows, head widths Hs / Hh / Hz, wout_ld the row stride of wout (>= the widest head).  write_bwd_exact: literal 0 of
 * air_write_bwd; write_bwd_graph: literals 2 and 4, with as many tap phases resident as the entry point would choose.
 * limit: what a workgroup may hold -- an entry point answers AIR_ELIMIT beyond it.  AIR_EINVAL: null out, a size < 1,
 * wout_ld below a head width. */
typedef struct {
    int64_t attend_fwd, attend_bwd, write_fwd, render, write_bwd_exact, write_bwd_graph, limit;
} air_step_lds_t;
int air_step_lds(int N, int C, int w, int Hs, int Hh, int Hz, int wout_ld, air_step_lds_t* out);

/* ---- stand-alone Concrete and VAE pieces (additive to ABI 6) ----------------------------------------------------------
 * The ops of the reference's air/concrete.py and the pointwise gradients of air/vae.py as launches of their own, for
 * callers that compose them with torch.autograd (air/concrete.py, air/vae.py of this package) -- the train step keeps
 * computing them inside air_attend_fwd / air_attend_bwd and the GEMM epilogues.  Plain element-wise kernels over n fp32
 * elements (any n >= 1): a grid-stride loop, 16-byte loads and stores when every array of the call is 16-byte aligned
 * (4-byte ones otherwise) and a scalar tail, no LDS, no atomics; fp32 in the reference's op order, one rounding per op.
 *
 * air_scalar_t: an argument the reference takes as a scalar OR a tensor (temperatures, prior log-odds).
 *   ptr == NULL:             `value`, by value;
 *   ptr != NULL, stride 0:   ONE device float, read by the kernel when it runs (a slot of `dyn` that a schedule
 *                            rewrites every step: no host read, a captured graph sees the new value);
 *   ptr != NULL, stride 1:   [n], one value per element.
 * AIR_EINVAL (all entry points below, answered on the host before any HIP call): a null descriptor or required pointer,
 * n < 1, a stride other than 0 or 1, Z < 1. */
typedef struct { const float* ptr; float value; int32_t stride; } air_scalar_t;

/* concrete.py:4-17 with the uniform sample u [n] given: noise = log(u + eps) - log(1 - u + eps); y = log_odds + noise;
 * sig_y = sigmoid(y / temperature), and with hard != 0 its tf.round (half to even).  y / sig_y: either may be NULL. */
int air_concrete_sample_fwd(const float* log_odds, const float* u, const air_scalar_t* temperature, float eps, int hard,
                            float* y /*nullable*/, float* sig_y /*nullable*/, int64_t n, void* stream);
/* its gradient: d_log_odds = d_y + (d_sig_y * s * (1 - s)) / temperature with s = sigmoid(y / temperature), the SOFT value
 * also when the forward was hard (the stop_gradient of concrete.py:15: straight-through).  d_y / d_sig_y: either may be
 * NULL (a zero gradient), not both. */
int air_concrete_sample_bwd(const float* y, const air_scalar_t* temperature, const float* d_y /*nullable*/,
                            const float* d_sig_y /*nullable*/, float* d_log_odds, int64_t n, void* stream);
/* concrete.py:20-27: y = (log_odds + noise) / temperature -- the expression of air_attend_fwd (AIR_ATT_ZPRE), same bits */
int air_concrete_presigmoid_fwd(const float* log_odds, const float* u, const air_scalar_t* temperature, float eps,
                                float* y, int64_t n, void* stream);
/* d_log_odds = d_y / temperature */
int air_concrete_presigmoid_bwd(const float* d_y, const air_scalar_t* temperature, float* d_log_odds, int64_t n, void* stream);
/* concrete.py:30-43: kl = log q(y) - log p(y), log r(y) = log(T_r + eps) - y T_r + a_r - 2 log(1 + exp(-y T_r + a_r) + eps)
 * for the prior (prior_log_odds, prior_temperature) and the posterior (posterior_log_odds [n], posterior_temperature) --
 * the expression of air_attend_fwd (AIR_ATT_KL_Z; shared device code), same bits. */
int air_concrete_kl_fwd(const float* y, const air_scalar_t* prior_log_odds, const air_scalar_t* prior_temperature,
                        const float* posterior_log_odds, const air_scalar_t* posterior_temperature, float eps,
                        float* kl, int64_t n, void* stream);
/* its exact derivatives: with e = exp(-y T + a), D = 1 + e + eps:  d log r / d a = 1 - 2 e / D,  d log r / d y = -T (1 - 2 e / D);
 * d_y = d_kl (d log q / d y - d log p / d y), d_posterior_log_odds = d_kl d log q / d a, d_prior_log_odds = -d_kl d log p / d a.
 * Each output may be NULL (not all three); d_prior_log_odds [n] only with a per-element prior_log_odds (stride 1). */
int air_concrete_kl_bwd(const float* d_kl, const float* y, const air_scalar_t* prior_log_odds,
                        const air_scalar_t* prior_temperature, const float* posterior_log_odds,
                        const air_scalar_t* posterior_temperature, float eps, float* d_y /*nullable*/,
                        float* d_posterior_log_odds /*nullable*/, float* d_prior_log_odds /*nullable*/, int64_t n, void* stream);

/* gradient of the sigmoid that ends the decoder (vae.py:39-41): d_pre = (d_rec * rec) * (1 - rec) from the saved output */
int air_sigmoid_bwd(const float* d_rec, const float* rec, float* d_pre, int64_t n, void* stream);
/* gradient of the re-parameterisation (vae.py:22-24) ALONE -- air_reparam_bwd / AIR_EPI_REPARAM_BWD add the VAE-KL term of
 * the model from att and dyn; this one takes what arrives at the mean and the log-variance from outside instead:
 *   d_ml[m, j]     = d_z[m, j] + d_mean_in[m, j]
 *   d_ml[m, Z + j] = ((d_z[m, j] * eps[m, j]) * 0.5) * sqrt(exp(ml[m, Z + j])) + d_lv_in[m, j]
 * ml / d_ml [M, 2Z] (mean | log_var), d_z / eps / d_mean_in / d_lv_in [M, Z]; the two incoming gradients are nullable
 * (nothing is added). */
int air_reparam_bwd_plain(const float* d_z, const float* ml, const float* eps, const float* d_mean_in /*nullable*/,
                          const float* d_lv_in /*nullable*/, float* d_ml, int M, int Z, void* stream);

/* ---- stand-alone CNN front-end (additive to ABI 6) --------------------------------------------------------------------
 * air_model.py:510-533, the block in front of the LSTM when cnn=True, generalised from the 50 x 50 canvas to S x S:
 *   conv1 (5x5, stride 1, SAME, 1 -> F, + bias, ReLU) -> pool1 (2x2, stride 2, VALID: S1 = S / 2, an odd last row and column
 *   are dropped) -> conv2 (F -> F, ReLU) -> pool2 (S2 = S1 / 2) -> conv3 (F -> F, ReLU) -> [B, S2 * S2 * F], (y, x, channel).
 * fp32 throughout, NHWC tensors, kernels [5, 5, Cin, F] and biases [F] as tf.layers.conv2d stores them.  air/cnn.py calls
 * air_cnn_fwd / air_cnn_bwd; the train step of AIRModel(cnn=True) calls air_cnn_fwd in front of x.Wx and air_cnn_bwd_sq
 * behind the data gradient of x.Wx.
 *
 * Max-pool routing: the pooled value is the maximum of the four ReLU outputs of its window, its code 2 dy + dx names the
 * FIRST maximum in row-major window order (what TF's MaxPoolGrad and torch's CPU max_pool2d route the gradient to), one
 * byte per pooled element.  ReLU's gradient (pre > 0) is read off the saved pooled value: pool(relu(x)) = relu(pool(x)).
 *
 * Launches: the forward is ONE launch (a workgroup per image; the un-pooled conv outputs never reach memory), the backward
 * one launch per image plus one that sums the per-image partials of the variable gradients in ascending image order.  No
 * atomics: the same inputs give the same bits.  Every inner product is one chain of fmaf in a fixed order, written out at
 * the top of csrc/air_cnn.hip.
 *
 * Limits: 1 <= F <= 8, 4 <= S <= 128, and the LDS of BOTH kernels must fit a workgroup's 160 KiB (S <= 77, 83, 89, 97, 107,
 * 118 at F = 8 .. 3, S <= 128 at F <= 2); the three entry points give the same answer for the same (B, S, F).
 * AIR_EINVAL (before any HIP call): a null descriptor or required pointer, some but not all of the four saved tensors,
 * B < 1, S < 4, F < 1.  AIR_ELIMIT (before any HIP call): F or S beyond the limits above. */
typedef struct {
    const float* images;                 /* [B, S * S] (= [B, S, S, 1])                                                */
    const float* k1; const float* b1;    /* [5, 5, 1, F], [F]                                                          */
    const float* k2; const float* b2;    /* [5, 5, F, F], [F]                                                          */
    const float* k3; const float* b3;    /* [5, 5, F, F], [F]                                                          */
    float* out;                          /* [B, S2 * S2 * F]                                                           */
    float* pool1; float* pool2;          /* nullable: [B, S1, S1, F], [B, S2, S2, F], what the backward needs ...       */
    uint8_t* arg1; uint8_t* arg2;        /* ... with their argmax codes; all four or none (the inference forward: `out`
                                            has the same bits)                                                         */
    int32_t B, S, F;
} air_cnn_fwd_t;
int air_cnn_fwd(const air_cnn_fwd_t* args, void* stream);

typedef struct {
    const float* d_out; const float* out;           /* [B, S2 * S2 * F]: the incoming gradient, the forward's output   */
    const float* images;                            /* the forward's input                                             */
    const float* pool1; const float* pool2;         /* the forward's saved tensors                                     */
    const uint8_t* arg1; const uint8_t* arg2;
    const float* k1; const float* k2; const float* k3;
    float* workspace;                               /* [>= air_cnn_workspace_floats(B, S, F)] floats of scratch        */
    float* d_k1; float* d_b1; float* d_k2; float* d_b2; float* d_k3; float* d_b3;    /* overwritten, not accumulated    */
    float* d_images;                                /* nullable: [B, S * S], computed only when given                  */
    int32_t B, S, F;
} air_cnn_bwd_t;
int air_cnn_bwd(const air_cnn_bwd_t* args, void* stream);
/* floats of `workspace` (the per-image partials of the six variable gradients), or AIR_EINVAL / AIR_ELIMIT for a
 * (B, S, F) the entry points refuse -- no GPU is touched */
int64_t air_cnn_workspace_floats(int B, int S, int F);
/* air_cnn_bwd whose batch reduction ALSO leaves sums of squares for the global-norm clip: workgroup i of the reduction
 * writes sq_partials[i] = the sum of the squares of the gradient elements it stored (the last workgroup counts nothing
 * past the last element), i in [0, air_cnn_num_sq_partials(F)).  The six gradients have the bits air_cnn_bwd gives; the
 * sums are taken in a fixed order without atomics (the same inputs give the same bits), so air_adam_clip_step can read
 * them behind air_wgrad_grouped's partials.  Errors as air_cnn_bwd, plus AIR_EINVAL for a null sq_partials. */
int air_cnn_bwd_sq(const air_cnn_bwd_t* args, float* sq_partials, void* stream);
/* how many floats air_cnn_bwd_sq writes: a function of F alone (AIR_EINVAL for F < 1, AIR_ELIMIT for F > 8); no GPU is touched */
int air_cnn_num_sq_partials(int F);

/* ---- histogram summaries (additive to ABI 6) --------------------------------------------------------------------------
 * tf.summary.histogram of the reference's variables and gradients (air_model.py:642-687, written by training.py:144-218):
 * TensorFlow 1.3's HistogramSummary (core/lib/histogram/histogram.cc) of up to AIR_HISTOGRAM_MAX strided views in ONE call.
 *
 * Buckets.  Positive limits: v = 1e-12; while (v < 1e20) { push v; v *= 1.1; } in double, then DBL_MAX.  All limits,
 * ascending: the negated positive limits in reverse, 0.0, the positive limits -- air_histogram_num_buckets() of them
 * (air_histogram_limits writes them; a host call, no GPU is touched).  A value x is cast to double and counted in bucket
 * upper_bound(limits, x), the index of the first limit strictly greater than x: +-0.0 and positive denormals land in the
 * bucket whose limit is 1e-12, |x| >= 9.92e19 in a DBL_MAX bucket.  The index is exact for every fp32 value.
 *
 * Values.  scale_kind 0: the element as stored; 1: x * prescale; 2: x * (prescale * s), s = clip * min(1 / gnorm, 1 / clip)
 * with clip = dyn[AIR_DYN_CLIP_NORM] (s = 1 when clip <= 0) and gnorm = *gnorm read on the device -- the factor
 * air_adam_clip_step applies to the gradient, ONE fp32 multiply per element.  A non-finite value (after the multiply) is
 * counted in `nonfinite` and left out of every other field (TF fails the op instead; the host side raises).
 *
 * A descriptor is a 2-D view as it lies in memory: element (r, c) is base[r * ld + c], r < rows, c < cols <= ld.  The
 * floats between cols and ld are never read into a result.  base: 4-byte aligned (AIR_EALIGN); 16-byte loads are used when
 * base is 16-byte aligned and cols and ld are multiples of 4, scalar loads otherwise.  rows * cols < 2^32 (AIR_ELIMIT).
 *
 * Output: record h at (char*)out + h * air_histogram_record_bytes():
 *   double min, max, num, sum, sum_squares, nonfinite;       (num == 0: min = +inf, max = -inf)
 *   uint32_t count[air_histogram_num_buckets()];             dense, in limit order
 *   uint32_t pad;                                            (0: keeps the next record 8-byte aligned)
 * out and workspace: 8-byte aligned device buffers (AIR_EALIGN) of at least air_histograms_output_bytes /
 * air_histograms_workspace_bytes bytes (out_bytes / workspace_bytes say what the caller allocated: AIR_EINVAL when short).
 * The call initialises everything it reports: both buffers may hold garbage.  sum and sum_squares are fp64 sums in a fixed
 * order and the counts integer sums: the same input gives the same bits.  Stream work (three kernels), no synchronisation,
 * no device value is read by the host.
 *
 * AIR_EINVAL / AIR_ELIMIT, from all three descriptor-taking calls alike and before any HIP call: null descs, count < 1
 * (EINVAL) or > AIR_HISTOGRAM_MAX (ELIMIT), a null base, rows or cols < 1, ld < cols, a scale_kind outside 0..2.
 * air_histograms also: a null descriptor, out or workspace, and null dyn / gnorm when a descriptor has scale_kind 2. */
#define AIR_HISTOGRAM_MAX 128
typedef struct {
    const float* base;                   /* DEVICE pointer */
    int32_t rows, cols, ld, scale_kind;
} air_histogram_desc_t;
typedef struct {
    const air_histogram_desc_t* descs;   /* HOST array [count], read during the call only */
    int32_t count;
    float prescale;                      /* scale_kind 1 and 2 */
    const float* dyn;                    /* AIR_DYN_* device array (scale_kind 2) */
    const float* gnorm;                  /* one device float: the global norm air_adam_clip_step wrote (scale_kind 2) */
    void* out;
    void* workspace;
    int64_t out_bytes, workspace_bytes;
} air_histograms_t;
int air_histogram_num_buckets(void);
int air_histogram_limits(double* out /* HOST, [air_histogram_num_buckets()] */);
int air_histogram_chunk(void);           /* elements per work item: a view of n elements is ceil(n / chunk) work items */
int64_t air_histogram_record_bytes(void);
int64_t air_histograms_output_bytes(const air_histogram_desc_t* descs, int count);
int64_t air_histograms_workspace_bytes(const air_histogram_desc_t* descs, int count);
int air_histograms(const air_histograms_t* a, void* stream);

/* ---- projector export (additive to ABI 6) ------------------------------------------------------------------------------
 * The middle of the reference's embeddings.py: the ground truth of a test set matched to the objects the model inferred
 * (embeddings.py:29-59, 86-114), the matched latents and windows gathered into dataset-level arrays, and the sprite sheet
 * of the windows as matplotlib's grey levels (embeddings.py:117-131).  air/embeddings.py is the caller.
 *
 * Ground truth of digit g of image i: the integer top-left corner (x, y) = gt_positions[i][g], the box (w, h) =
 * gt_boxes[i][g].  In fp64:  cx = (x + x + w - 1.0) / 2.0,  st_cx = cx / ((canvas_size - 1) / 2.0) - 1.0,  cy / st_cy alike
 * (x + x + w is an int32 sum, as numpy forms it).
 *
 * Match, per image, its ground-truth digits in order: over the inferred objects t = 0 .. run_digits[i] - 1 (clamped to T)
 *   dist = sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1))     fp64; (x2, y2) = att[t][i][AIR_ATT_X, AIR_ATT_Y] widened
 * keep the FIRST strict minimum below min_distance = 3.0; accept it when min_distance <= max_distance and no earlier digit
 * of the image took that object.  A digit whose closest object is taken gets no second choice.  A digit of an image without
 * inferred objects is never accepted (the reference's script would index an empty list there when max_distance >= 3).
 * match[i][g] = the step t, or -1.
 *
 * Rows.  The accepted pairs of the chunk, in (image, digit) order, take the rows counters[AIR_EMBED_MATCHED] + 0, 1, ... of
 * the four outputs: out_latents[row] = ml[t][i][0 .. Z) (the means: what rec_latents returns), out_windows[row] =
 * vrec[t][i], out_labels / out_ids[row] = gt_labels / gt_ids[i][g].  A row >= capacity is not written; the call sets
 * counters[AIR_EMBED_OVERFLOW] = 1 instead.  The call then advances the int32 counters, which live on the device across the
 * chunks of a dataset (the caller zeroes them once): MATCHED (also the row cursor of the next chunk) by the accepted pairs,
 * PRESENT by the sum of gt_count, INFERRED by the sum of run_digits over the k real images.
 *
 * k <= B: the last chunk of a dataset fills only its first k batch rows; the ground-truth arrays have k rows, padded to G
 * digits per image (gt_count[i] <= G says how many are real).  Two launches (one workgroup that matches and scans, one
 * workgroup per (image, digit) slot that copies), stream-ordered, no host read, no floating-point atomics; 16-byte copies
 * where both rows are 16-byte aligned.  The same inputs give the same bits.
 *
 * AIR_EINVAL (before any HIP call): a null descriptor, pointer or workspace; T, B, k, G, Z, w or capacity < 1; k > B;
 * canvas_size < 2; max_distance <= 0 (or NaN).  AIR_ELIMIT: T > AIR_EMBED_MAX_STEPS, G > AIR_EMBED_MAX_DIGITS, w > 256. */
#define AIR_EMBED_MAX_STEPS 16
#define AIR_EMBED_MAX_DIGITS 16
enum { AIR_EMBED_MATCHED = 0, AIR_EMBED_PRESENT = 1, AIR_EMBED_INFERRED = 2, AIR_EMBED_OVERFLOW = 3, AIR_EMBED_COUNTERS = 4 };
typedef struct {
    const float* att;                    /* [T, B, AIR_ATT_STRIDE] of the inference pass                                */
    const int32_t* run_digits;           /* [B] inferred object counts                                                  */
    const float* ml;                     /* [T, B, 2 Z]: mean | log-variance                                            */
    const float* vrec;                   /* [T, B, w * w] decoded windows                                               */
    const int32_t* gt_count;             /* [k]                                                                         */
    const int32_t* gt_positions;         /* [k, G, 2] (x, y)                                                            */
    const int32_t* gt_boxes;             /* [k, G, 2] (w, h)                                                            */
    const int32_t* gt_labels;            /* [k, G]                                                                      */
    const int32_t* gt_ids;               /* [k, G]                                                                      */
    int32_t* match;                      /* out [k, G]                                                                  */
    int32_t* counters;                   /* in / out [AIR_EMBED_COUNTERS]                                               */
    float* out_latents;                  /* [capacity, Z]                                                               */
    float* out_windows;                  /* [capacity, w * w]                                                           */
    int32_t* out_labels;                 /* [capacity]                                                                  */
    int32_t* out_ids;                    /* [capacity]                                                                  */
    int32_t T, B, k, G, Z, w, capacity, canvas_size;
    double max_distance;
} air_embed_collect_t;
/* `workspace`: a device buffer of at least air_embed_collect_workspace_ints(T, B, k, G) int32 (the row of every slot) */
int air_embed_collect(const air_embed_collect_t* args, void* workspace, void* stream);
/* int32 elements of `workspace`, or AIR_EINVAL / AIR_ELIMIT for a (T, B, k, G) the entry point refuses -- no GPU is touched */
int64_t air_embed_collect_workspace_ints(int T, int B, int k, int G);

/* The sprite sheet of windows [M, w * w] as grey levels, uint8 plane [dim * w, dim * w], dim = ceil(sqrt(M))
 * (air_embed_sprite_dim).  The fp64 sheet is 1.0 everywhere, tile i (column i % dim, row i / dim) has window i subtracted;
 * lo and hi are its minimum and maximum (an empty tile's 1.0 included when dim * dim > M); then, as matplotlib's
 * imsave(cmap='gray') does:  n = (v - lo) / (hi - lo) in fp64 (0 when hi == lo), index = min(int(n * 256), 255),
 * grey = uint8(linspace(0, 1, 256)[index] * 255), truncating -- a 256-byte table that is not the identity.
 * Two launches (per-workgroup min / max partials; fold + plane, four pixels per 32-bit store when dim * w is a multiple of
 * 4).  workspace: 8-byte aligned, plane: 4-byte aligned (AIR_EALIGN).  AIR_EINVAL: M < 1 (the reference cannot save an empty
 * sheet either), w < 1, a null pointer.  AIR_ELIMIT: M > 2^22, w > 256. */
int air_embed_sprites(const float* windows, int M, int w, void* workspace, uint8_t* plane, void* stream);
int air_embed_sprite_dim(int M);
/* doubles of `workspace`, or AIR_EINVAL / AIR_ELIMIT -- no GPU is touched */
int64_t air_embed_sprites_workspace_doubles(int M, int w);

/* ---- scene source (additive to ABI 6) -----------------------------------------------------------------------------------
 * The default path of the reference's generate_multi_image (multi_mnist.py:82-183: use_pixel_overlap=True, no scale or
 * rotation jitter) as ONE launch that composes a fresh batch of B canvases straight into the caller's buffers -- the train
 * model's inputs -- so that a run needs no data set.  multi_mnist.DeviceSceneSource is the caller.
 *
 * Inputs.  glyphs [G, gd * gd] fp32, values >= 0 (ink is value > 0).  crops [G, 4] int32: x0, y0, w, h of each glyph's
 * non-empty box, computed once on the host (crop_non_empty, multi_mnist.py:36-43).  bg, nullable [C * C].  counts, nullable
 * [B] int32: the number of digits of each scene (clamped to 0 .. max_digits); null: drawn uniformly from 0 .. max_digits.
 *
 * One scene, by one workgroup, the canvas and an occupancy plane in LDS:
 *   for each of its n digits in turn: draw a glyph index g; then up to max_attempts times draw x uniform in
 *   [margin, C - w - margin] and y uniform in [margin, C - h - margin].  The first digit takes its first draw.  A later digit
 *   is accepted when no ink pixel of the glyph lies within Chebyshev distance `gap` of an ink pixel already on the canvas
 *   (the reference's max(image, window) == image + window against the add_buffer-dilated canvas, :44-65).  An accepted
 *   glyph's box is added to the canvas: inks are disjoint and everything else adds zero, so the sums are exact.
 *   A digit that finds no place in max_attempts draws, or whose box does not fit (w + 2 margin > C or h + 2 margin > C; also
 *   a crop box that is empty or leaves its gd x gd frame), RESTARTS the scene with an empty canvas.  status[b] is the number
 *   of restarts.  At the end, with bg: image = min(max(canvas + bg, 0), 1) (:189-190); without: the canvas as it is.
 * Two deviations from the reference:
 *   - the glyph index is drawn uniformly from 0 .. G-1 instead of walking a permutation of the glyph set (:84-85, 108-112);
 *   - the reference restarts without a bound; here, when the restart count reaches max_restarts (the scene has failed
 *     max_restarts times) the scene is written as an EMPTY canvas (bg alone), digits = 0, status = -1, its metadata zero.
 *
 * Random numbers: integers only.  Draw j of scene b is word j & 3 of Philox4x32-10(key = (seed low, seed high), counter =
 * (b, j >> 2, (uint32_t)batch, 0x5343454E)); an integer in [lo, hi) is lo + umulhi(word, hi - lo).  Draw 0 is the count
 * (only when counts is null); then per digit the glyph index and, per attempt, x then y.  j keeps counting across restarts.
 * A scene makes at most 1 + max_restarts * max_digits * (1 + 2 * max_attempts) draws: every loop of the kernel has a trip
 * count bounded by a range-checked argument, control flow is uniform across the workgroup (every thread computes the same
 * draws, the overlap test ends in a workgroup-wide OR), and there are no global atomics and no grid-wide waits.
 * batch = *batch_counter + step_in_replay: air_scene_source_advance (one thread: *counter += by) runs once per eager batch,
 * or once behind the last compose of a captured replay with by = its steps, so replays continue the sequence without the
 * host and batch k is the same scene set however it was made.
 *
 * Outputs (every element is written): images [B, C * C]; digits [B] (the glyphs on the canvas); indices [B, max_digits];
 * positions [B, 2 * max_digits] (x, y of each box's top-left corner); boxes [B, 2 * max_digits] (w, h); status [B]; slots
 * behind digits[b] are zero.  gave_up, nullable [B] int32: gave_up[b] += (status[b] == -1) -- a running per-slot count
 * (its sum is the number of scenes given up so far), read and written by workgroup b alone.
 *
 * Limits, answered on the host before any HIP call.  AIR_EINVAL: a null descriptor; B, G, gd, C or max_digits < 1; margin,
 * gap or step_in_replay < 0; max_attempts or max_restarts < 1; 2 * margin + 1 > C (no glyph can fit); then a null required
 * pointer.  AIR_ELIMIT: C > 128, gd > 32, max_digits > 6, gap > 4, max_attempts > 100, max_restarts > 64.  An invalid size
 * is reported before a limit, a limit before a null pointer; AIR_EALIGN: crops not 16-byte aligned.  Dynamic LDS: air_scene_source_lds(C, gd) = 4 C C (canvas) +
 * 4 gd gd (the glyph being placed) + C C (occupancy), each part rounded up to 16 bytes, + 160 (metadata): 86 176 bytes at
 * the limits, granted once per device (air_scene_source_prepare does it without a launch: call it before a capture whose
 * first compose would otherwise be the first). */
typedef struct {
    const float* glyphs;                 /* [G, gd * gd]                                                                */
    const int32_t* crops;                /* [G, 4] x0, y0, w, h                                                         */
    const float* bg;                     /* nullable [C * C]                                                            */
    const int32_t* counts;               /* nullable [B]                                                                */
    const int64_t* batch_counter;        /* one device int64: batches made before this replay / this eager batch        */
    float* images;                       /* out [B, C * C]                                                              */
    int32_t* digits;                     /* out [B]                                                                     */
    int32_t* indices;                    /* out [B, max_digits]                                                         */
    int32_t* positions;                  /* out [B, 2 * max_digits]                                                     */
    int32_t* boxes;                      /* out [B, 2 * max_digits]                                                     */
    int32_t* status;                     /* out [B]: restarts, or -1                                                    */
    int32_t* gave_up;                    /* in / out, nullable [B]                                                      */
    int32_t B, G, gd, C, margin, gap, max_digits, max_attempts, max_restarts;
    uint64_t seed;
} air_scene_source_t;
#define AIR_SCENE_MAX_CANVAS 128
#define AIR_SCENE_MAX_GLYPH 32
#define AIR_SCENE_MAX_DIGITS 6
#define AIR_SCENE_MAX_GAP 4
#define AIR_SCENE_MAX_ATTEMPTS 100
#define AIR_SCENE_MAX_RESTARTS 64
int air_scene_source_compose(const air_scene_source_t* a, int step_in_replay, void* stream);
int air_scene_source_advance(int64_t* counter, int by, void* stream);    /* AIR_EINVAL: null counter, by < 0 */
/* the checks and the LDS grant of air_scene_source_compose(a, 0, ..) without its launch */
int air_scene_source_prepare(const air_scene_source_t* a);
/* bytes of dynamic LDS per workgroup, or AIR_EINVAL / AIR_ELIMIT for a (C, gd) the entry point refuses -- no GPU is touched */
int64_t air_scene_source_lds(int C, int gd);

/* ---- glyph bank: scale and rotation jitter (additive to ABI 6) -----------------------------------------------------------
 * The two jitter options of the reference's generate_multi_image (multi_mnist.py:113-135) as ONE launch that turns the base
 * glyphs into V jittered variants with their crop boxes: a bank the scene source draws from in place of the glyph set
 * (bank / bank_crops are its glyphs / crops, with gd = od).  multi_mnist.DeviceGlyphBank is the caller.
 *
 * One variant, by one workgroup, its planes in LDS.  The bank generation is *counter (null: 0; air_scene_source_advance
 * moves it).  Draw j of variant v is word j & 3 of Philox4x32-10(key = (seed low, seed high), counter = (v, j >> 2,
 * (uint32_t)generation, 0x474A4954)).  Word 0 picks the base glyph g = umulhi(word, G).  A real takes two words:
 * u = ((a >> 5) * 2^26 + (b >> 6)) / 2^53, value = lo + (hi - lo) * u in fp64.  Only when one of the four scale bounds is
 * not 1.0: new_width, then new_height.  Then, only when one of the two angle bounds is not 0.0: angle (degrees).
 *   Scale (:117-126): the base glyph's crop box (h x w) through the transform below with matrix diag(1 / new_height,
 *   1 / new_width), offset 0, onto a plane of int(gd * new_height) x int(gd * new_width).
 *   Rotation (:128-135, scipy.ndimage.rotate(reshape=True)): c, s = cos, sin of the angle (fp64, on the device: the angle
 *   less its nearest multiple of 90 is exact, sincospi of that / 180, the quadrant put back by sign and swap);
 *   R = (c s; -s c); plane = int(ptp(R (0 0 h h; 0 w 0 w), axis 1) + 0.5); offset = (in - 1) / 2 - R ((plane - 1) / 2).
 *   Each stage's result is rounded to float32, clipped to [0, 1], values < 0.05 set to 0, cropped to its non-empty box.
 * status[v]: 0 usable; 1 a stage left nothing (or the base crop box is empty or leaves its gd x gd frame); 2 a plane outside
 * its limit (scaled side not in 1 .. AIR_JITTER_MAX_PLANE, rotated side not in 1 .. 64) or a final box larger than od.  A
 * non-zero status writes an all-zero frame and an all-zero crop box: the scene kernel restarts a scene that draws it, which
 * is what the reference's IndexError path does (:177).
 *
 * The transform is scipy's affine_transform(order=5, mode='constant', cval=0, prefilter=True), fp64 throughout:
 *   prefilter: along axis 0, then axis 1; a line of n = 1 is left alone; poles z1 = sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25)
 *   - 6.5, z2 = sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5 (computed on the host); the line times
 *   gain = prod (1 - z)(1 - 1 / z); then per pole: zn = z^(n-1) by repeated multiplication, c0 = c[0] + zn c[n-1], for
 *   i = 1 .. n-2: c0 += z^i (c[i] + zn c[n-1-i]), c[0] = c0 / (1 - zn zn); c[i] += z c[i-1]; c[n-1] = (z c[n-2] + c[n-1]) z /
 *   (z z - 1); c[i] = z (c[i+1] - c[i]) from n-2 down to 0.
 *   evaluation: cc = (oy m00 + ox m01) + offset per axis; a coordinate < 0 or > len - 1 gives 0; taps floor(cc) - 2 .. + 3
 *   per axis, mirrored with period 2n - 2; weights at x = cc - floor(cc): w2 = t (t (0.25 - x / 12) - 0.5) + 0.55, t = x x;
 *   w3 the same in 1 - x; w1 = y (y (y (y (y / 24 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425, y = x + 1; w4 the same in 2 - x;
 *   w0 = y t t / 120, y = 1 - x, t = y y; w5 = 1 - ((((w0 + w1) + w2) + w3) + w4).
 *   SUMMATION ORDER of the 36 products: t = 0; for tap row 0 .. 5 (top first), for tap column 0 .. 5 (left first):
 *   t = t + (coefficient * wy[row]) * wx[column].
 *
 * Outputs (every element is written): bank [V, od * od] float32, the variant's final crop at the top-left of its od x od
 * frame, +0 elsewhere; bank_crops [V, 4] = (0, 0, w, h), or zeros; source [V], the base glyph; params [V, 6] fp64: new_width,
 * new_height, angle, c, s, 0 (1, 1, 0, 1, 0 for what was not drawn); status [V].
 *
 * Limits, answered on the host before any HIP call, an invalid size before a limit, a limit before a null pointer.
 * AIR_EINVAL: a null descriptor; V, G, gd or od < 1; od < gd; a bound that is not finite; min > max; a scale bound <= 0;
 * int(gd * min_h) or int(gd * min_w) < 1; then a null pointer (counter may be null).  AIR_ELIMIT: gd or od >
 * AIR_SCENE_MAX_GLYPH; int(gd * max_h) or int(gd * max_w) > AIR_JITTER_MAX_PLANE; |angle bound| > 180.  AIR_EALIGN: crops
 * or bank_crops not 16-byte aligned, params not 8-byte aligned.  Dynamic LDS: air_glyph_jitter_lds(gd, od) = 8 * 48 * 48
 * (coefficients) + 4 * 64 * 64 (the image so far) + 32 (boxes) = 34 848 bytes at every accepted (gd, od): below 48 KiB, so
 * no grant and nothing for air_glyph_jitter_prepare to do but the checks. */
typedef struct {
    const float* glyphs;                 /* [G, gd * gd]                                                                */
    const int32_t* crops;                /* [G, 4] x0, y0, w, h                                                         */
    const int64_t* counter;              /* nullable: one device int64, the bank generation                             */
    float* bank;                         /* out [V, od * od]                                                            */
    int32_t* bank_crops;                 /* out [V, 4]                                                                  */
    int32_t* source;                     /* out [V]                                                                     */
    double* params;                      /* out [V, 6]                                                                  */
    int32_t* status;                     /* out [V]                                                                     */
    int32_t V, G, gd, od;
    double min_w, max_w, min_h, max_h, min_ang, max_ang;
    uint64_t seed;
} air_glyph_jitter_t;
#define AIR_JITTER_MAX_PLANE 48
int air_glyph_jitter(const air_glyph_jitter_t* a, void* stream);
/* the checks of air_glyph_jitter without its launch */
int air_glyph_jitter_prepare(const air_glyph_jitter_t* a);
/* bytes of dynamic LDS per workgroup, or AIR_EINVAL / AIR_ELIMIT for a (gd, od) the entry point refuses -- no GPU is touched */
int64_t air_glyph_jitter_lds(int gd, int od);

/* ---- handwriting bank: base glyphs distorted into MNIST's geometry (additive to ABI 6) ------------------------------------
 * ONE launch that turns base glyphs (whole gd x gd planes, values in [0, 1]) into V distorted variants: an elastic field
 * (Simard et al. 2003) and an affine map, a stroke of drawn width, an ink ramp, the box fitted to `ink` pixels a side and the
 * glyph put by its centre of mass into an od x od frame -- MNIST's 20-in-28 layout at ink = 20, od = 28.  The outputs have the
 * shapes and the meaning of air_glyph_jitter's: a bank the scene source draws from.  multi_mnist.DeviceHandwritingBank is
 * the caller; it makes taps and field_gain.
 *
 * One variant, by one workgroup of 256 threads, its planes in LDS; every intermediate is fp64 unless said otherwise, the build
 * has -ffp-contract=off, and tests/glyph_distort_cases.py restates every operation below.  generation = *counter (null: 0).
 * Parameter stream: draw j of variant v is word j & 3 of Philox4x32-10(key = (seed low, seed high), counter = (v, j >> 2,
 * (uint32_t)generation, 0x47445350)).  Word 0 picks the base glyph g = umulhi(word, G).  A real takes two words,
 * u = ((a >> 5) * 2^26 + (b >> 6)) / 2^53, value = lo + (hi - lo) * u.  In this order, each only when its bounds are not
 * neutral: angle in [-max_ang, max_ang] (degrees; when max_ang != 0), shear k in [-max_shear, max_shear] (when max_shear !=
 * 0), sx then sy in [min_scale, max_scale] (when one of the two is not 1.0), and one word for the stroke,
 * n = min_stroke + umulhi(word, max_stroke - min_stroke + 1) (when the two are not both 0).
 * Field stream (only when field_gain != 0): element j = plane * gd * gd + y * gd + x of the two planes is word j & 3 of
 * Philox4x32-10(same key, counter = (v, j >> 2, (uint32_t)generation, 0x47445346)); value = ((word >> 8) + 0.5) * 2^-23 - 1.
 *
 *   1. Field.  Each plane is smoothed along axis 0, then along axis 1: out[i] = sum over t = 0 .. 2 radius, ascending, of
 *      taps[t] * in[i + t - radius], the terms whose pixel lies outside the plane left out (zeros outside); the axis-1 sums are
 *      multiplied by field_gain.  Plane 0 displaces y, plane 1 displaces x.  With taps a normalised Gaussian and
 *      field_gain = alpha / ((1 / sqrt 3) * sum taps^2) the field has standard deviation alpha pixels away from the border.
 *   2. Warp.  c, s = cos, sin of the angle (the angle less its nearest multiple of 90 is exact, sincospi of that / 180, the
 *      quadrant put back by sign and swap -- air_glyph_jitter's).  isy = 1 / sy, isx = 1 / sx; A = R (1 k; 0 1) diag(isy, isx)
 *      with R = (c s; -s c) over (y, x):  a00 = c isy, a01 = (c k + s) isx, a10 = (-s) isy, a11 = ((-s) k + c) isx.
 *      ctr = (gd - 1) / 2, dy = y - ctr, dx = x - ctr;  qy = (ctr + (a00 dy + a01 dx)) + field0[y, x],
 *      qx = (ctr + (a10 dy + a11 dx)) + field1[y, x] (the field terms only when field_gain != 0).  fy = floor(qy), ty = qy - fy,
 *      uy = 1 - ty, likewise in x; v00 .. v11 the base plane at (fy, fx), (fy, fx + 1), (fy + 1, fx), (fy + 1, fx + 1), zero
 *      outside the plane;  value = float32(((v00 (uy ux) + v01 (uy tx)) + v10 (ty ux)) + v11 (ty tx)).
 *   3. Stroke.  |n| passes, each behind a barrier: every pixel becomes the maximum (n > 0) or the minimum (n < 0) of itself
 *      and its upper, lower, left and right neighbours, those outside the plane left out.
 *   4. Ramp.  t = (value - lo) / (hi - lo), clipped to [0, 1], rounded to float32; values < 0.05 become 0.  h x w = the box of
 *      what is left; status 1 when nothing is.
 *   5. Fit.  f = ink / max(h, w); h' = max(1, floor(h f + 0.5)), w' likewise.  Area average along axis 0 (h -> h'), then along
 *      axis 1 (w -> w'): with r = h / h', out[i] = (sum over j = 0 .. h - 1, ascending, of in[j] * max(0, min(j + 1, (i + 1) r)
 *      - max(j, i r))) / r.  The axis-1 result is rounded to float32, values < 0.05 become 0, and the box of what is left is
 *      taken again (it may be smaller than h' x w'; status 1 when nothing is left): from here on h' x w' is that box.
 *   6. Centre.  Per row of the box, m_r = sum of v and mx_r = sum of v * x, x ascending from the box's left edge (x = 0);
 *      then m = sum m_r, my = sum m_r * r, mx = sum mx_r, rows ascending; cy = my / m, cx = mx / m.
 *      y0 = clamp(floor((od - 1) / 2 - cy + 0.5), 0, od - h'), x0 likewise.
 *
 * Outputs (every element is written): bank [V, od * od] float32, the glyph with its box's corner at (x0, y0), +0 elsewhere;
 * bank_crops [V, 4] = (x0, y0, w', h'); source [V], the base glyph; params [V, 8] fp64: angle, shear, sx, sy, c, s, n, f
 * (0, 0, 1, 1, 1, 0, 0 for what was not drawn; f = 0 when the ramp left nothing); status [V]: 0 usable, 1 nothing left
 * after the ramp or the fit, 2 a box larger than od (ink <= od rules it out; checked before the frame is written).  A
 * non-zero status writes an all-zero frame and an all-zero box: the scene kernel restarts a scene that draws it.
 *
 * Limits, answered on the host before any HIP call: an invalid size before a limit, a limit before a null pointer, a null
 * pointer before the alignment.  AIR_EINVAL: a null descriptor; V, G, gd, od or ink < 1; radius < 0; ink > od; field_gain or
 * a real bound that is not finite; min_scale > max_scale; min_stroke > max_stroke; lo >= hi; min_scale <= 0; then a null
 * pointer (counter may be null).  AIR_ELIMIT: gd > AIR_DISTORT_MAX_PLANE; od > AIR_SCENE_MAX_GLYPH; radius >
 * AIR_DISTORT_MAX_RADIUS (a tap line may be wider than the plane); |max_ang| > 180; a stroke bound outside +-
 * AIR_DISTORT_MAX_STROKE.  AIR_EALIGN: bank_crops not 16-byte aligned; params or taps not 8-byte aligned.
 * Dynamic LDS: air_glyph_distort_lds(gd, od, radius) = 3 * 8 S S (field planes) + 8 (2 radius + 1) (taps) + 4 S S (the base
 * plane, then the fitted glyph) + 32 (boxes) with S = max(gd, od): 45 864 bytes at the limits, 45 224 at the preset (gd 40,
 * radius 24) -- below 48 KiB, so air_glyph_distort_prepare is the checks (and would take the grant if the limits grew). */
typedef struct {
    const float* glyphs;                 /* [G, gd * gd]                                                                */
    const int64_t* counter;              /* nullable: one device int64, the bank generation                             */
    const double* taps;                  /* device [2 * radius + 1]                                                     */
    float* bank;                         /* out [V, od * od]                                                            */
    int32_t* bank_crops;                 /* out [V, 4]                                                                  */
    int32_t* source;                     /* out [V]                                                                     */
    double* params;                      /* out [V, 8]                                                                  */
    int32_t* status;                     /* out [V]                                                                     */
    int32_t V, G, gd, od, ink, radius, min_stroke, max_stroke;
    double field_gain, max_ang, max_shear, min_scale, max_scale, lo, hi;
    uint64_t seed;
} air_glyph_distort_t;
#define AIR_DISTORT_MAX_PLANE 40
#define AIR_DISTORT_MAX_RADIUS 64
#define AIR_DISTORT_MAX_STROKE 4
int air_glyph_distort(const air_glyph_distort_t* a, void* stream);
/* the checks and the LDS grant of air_glyph_distort without its launch */
int air_glyph_distort_prepare(const air_glyph_distort_t* a);
/* bytes of dynamic LDS per workgroup, or AIR_EINVAL / AIR_ELIMIT for sizes the entry point refuses -- no GPU is touched */
int64_t air_glyph_distort_lds(int gd, int od, int radius);

/* ---- localisation metrics (additive to ABI 6) ---------------------------------------------------------------------------
 * The attention boxes of an inference pass scored against the ground-truth boxes of its images: box IoU, recall, cover,
 * centre distance and the confusion matrix of the counts.  air/metrics.py (Localization) is the caller; the first seven
 * fields are those of air_embed_collect_t, in its layouts, so one set of device arrays serves both.
 *
 * All arithmetic is fp64 in exactly the order written here (the translation unit has -ffp-contract=off), and
 * tests/localization_cases.py restates every operation below.  C = canvas_size; n_i = run_digits[i] clamped to [0, T];
 * c_i = gt_count[i] clamped to [0, G]; i < k.
 *
 * Inferred box of object t < n_i of image i.  q = (C - 1.001) / 2.0 (the transformer's pixel map, transformer.py:75-76, in
 * fp64); (s, x, y) = att[t][i][AIR_ATT_S, AIR_ATT_X, AIR_ATT_Y] widened;
 *   l1 = (x - s + 1.0) * q     r1 = (x + s + 1.0) * q + 1.0     t1 = (y - s + 1.0) * q     b1 = (y + s + 1.0) * q + 1.0
 * (the sample points of the window span the pixel indices l1 .. r1 - 1; pixel j is the cell [j, j + 1)), then every edge v
 * is clipped:  v < 0 ? 0 : (v > C ? C : v)  -- a NaN passes through.  a_inf = (r1 - l1) * (b1 - t1).
 * Ground-truth box of digit g < c_i: (x, y) = gt_positions[i][g], (w, h) = gt_boxes[i][g], widened one by one:
 *   l2 = x     r2 = x + w     t2 = y     b2 = y + h     a_gt = w * h
 * Pair (g, t):  iw = min(r1, r2) - max(l1, l2),  ih = min(b1, b2) - max(t1, t2)  (min(a, b) = a < b ? a : b, max alike with
 * >).  When iw > 0 && ih > 0:  inter = iw * ih,  uni = a_inf + a_gt - inter,  and when uni > 0:  iou = inter / uni,
 * cover = inter / a_gt.  In every other case (a NaN anywhere among them) iou = cover = 0.
 * dist, the reference's centre distance in transformer units (embeddings.py:39-44, 113-114, as air_embed_collect has it):
 *   cx = ((x + x + w) - 1.0) / 2.0 (an int32 sum, widened),  x1 = cx / ((C - 1) / 2.0) - 1.0,  cy / y1 alike,
 *   dist = sqrt((xa - x1) * (xa - x1) + (ya - y1) * (ya - y1)),  (xa, ya) = att[t][i][AIR_ATT_X, AIR_ATT_Y] widened.
 *
 * Match, per image: greedy on IoU, at most min(n_i, c_i) rounds.  A round scans the pairs of unused digits and unused
 * objects, g outer and t inner, and keeps the first pair whose iou is strictly greater than the best so far (the best
 * starts at 0): a tie goes to the smaller g, then the smaller t, and a pair with iou 0 is never taken.  The round takes the
 * kept pair (digit and object are used from then on); the first round that keeps none ends the image.
 * match[i][g] = the object taken with digit g, or -1; iou[i][g] = the iou of that pair, or 0.  g in [c_i, G) gets -1 and 0.
 *
 * Accumulators: the caller zeroes them once; a call ADDS, so the chunks of a data set add up.
 *   counts[AIR_LOC_IMAGES] += k, [PRESENT] += sum c_i, [INFERRED] += sum n_i, [MATCHED] += taken pairs, [HITS] += taken
 *   pairs with iou >= iou_threshold, [COUNT_CORRECT] += images with n_i == c_i, and the confusion matrix
 *   counts[AIR_LOC_COUNTS + c_i * (T + 1) + n_i] += 1  ((G + 1) rows of (T + 1)).  Integer atomics: any order, the same sums.
 *   sums[AIR_LOC_IOU / COVER / DIST] += the iou / cover / dist of the taken pairs, each of the three in this ONE order,
 *   which depends on (k, G) alone:
 *     1. image i:  p_i = (((+0.0 + v_0) + v_1) + ...) over its digits g = 0 .. c_i - 1 in order, v_g the value of digit g's
 *        pair, an unmatched digit skipped;
 *     2. group j = images [AIR_LOC_GROUP * j, AIR_LOC_GROUP * (j + 1)): its AIR_LOC_GROUP values p (+0.0 for an image >= k)
 *        are folded by the adjacent pairwise tree -- v[m] = v[2 m] + v[2 m + 1], eight times, 256 values to one;
 *     3. the batch total = (((+0.0 + group 0) + group 1) + ...) in group order;
 *     4. sums[.] = incoming sums[.] + the batch total.
 * No floating-point atomics: the same inputs (and incoming accumulators) give the same bits.
 *
 * Two launches on the caller's stream (a thread per image in workgroups of AIR_LOC_GROUP, which leave one partial triple
 * per group in the workspace; one small fold), no synchronisation, no host read.  Rows >= k of att / run_digits are never
 * read, the ground truth has k rows, and match / iou rows >= k are never written.  match and iou are nullable TOGETHER.
 *
 * Refusals, on the host before any HIP call, in this order.  AIR_EINVAL: a null descriptor; T, B, k or G < 1; k > B.
 * AIR_ELIMIT: T > AIR_LOC_MAX_STEPS, G > AIR_LOC_MAX_DIGITS.  AIR_EINVAL: canvas_size < 2; iou_threshold not in (0, 1]
 * (NaN included); a null att, run_digits, gt_count, gt_positions, gt_boxes, counts, sums or workspace; exactly one of
 * match / iou null. */
#define AIR_LOC_MAX_STEPS 16
#define AIR_LOC_MAX_DIGITS 16
#define AIR_LOC_GROUP 256
enum { AIR_LOC_IMAGES = 0, AIR_LOC_PRESENT = 1, AIR_LOC_INFERRED = 2, AIR_LOC_MATCHED = 3, AIR_LOC_HITS = 4,
       AIR_LOC_COUNT_CORRECT = 5, AIR_LOC_COUNTS = 6 };
enum { AIR_LOC_IOU = 0, AIR_LOC_COVER = 1, AIR_LOC_DIST = 2, AIR_LOC_SUMS = 3 };
typedef struct {
    const float* att;                    /* [T, B, AIR_ATT_STRIDE] of the pass just run                                 */
    const int32_t* run_digits;           /* [B] inferred object counts                                                  */
    const int32_t* gt_count;             /* [k]                                                                         */
    const int32_t* gt_positions;         /* [k, G, 2] (x, y): the memory layout of DeviceSceneSource.positions          */
    const int32_t* gt_boxes;             /* [k, G, 2] (w, h)                                                            */
    int32_t* match;                      /* out [k, G], nullable with iou                                               */
    double* iou;                         /* out [k, G], nullable with match                                             */
    int64_t* counts;                     /* in / out [AIR_LOC_COUNTS + (G + 1) * (T + 1)]                               */
    double* sums;                        /* in / out [AIR_LOC_SUMS]                                                     */
    int32_t T, B, k, G, canvas_size;
    double iou_threshold;
} air_localization_t;
/* `workspace`: a device buffer of at least air_localization_workspace_bytes(T, B, k, G) bytes, 8-byte aligned (the
 * per-group partial sums) */
int air_localization(const air_localization_t* args, void* workspace, void* stream);
/* bytes of `workspace`, or AIR_EINVAL / AIR_ELIMIT for a (T, B, k, G) the entry point refuses -- no GPU is touched */
int64_t air_localization_workspace_bytes(int T, int B, int k, int G);

/* ---- segmentation metrics (additive to ABI 6) -----------------------------------------------------------------------------
 * The decomposition of an inference pass scored per pixel: which object explains which ink.  Two entry points:
 * air_scene_masks builds the ground-truth instance labels of composed scenes from the scene source's metadata, and
 * air_segmentation derives the predicted instance labels of a pass from its records and decoded windows and scores them
 * against a label plane -- the foreground adjusted Rand index (FG-ARI) and the best mask IoU of every ground-truth object.
 * air/metrics.py (Segmentation) is the caller; tests/segmentation_cases.py restates every operation below.
 *
 * air_scene_masks.  glyphs [Gn, gd * gd] and crops [Gn, 4] (x0, y0, w, h) are the arrays air_scene_source_compose reads;
 * digits [B], indices [B, max_digits] and positions [B, 2 * max_digits] (x, y) are its outputs.  One workgroup per scene.
 * mask [B, C * C] uint8, every element written: pixel (py, px) of scene b gets the label g + 1 of the SMALLEST
 * g < clamp(digits[b], 0, max_digits) with, for idx = indices[b][g], (x0, y0, w, h) = crops[idx], (x_g, y_g) =
 * positions[b][g]:
 *   0 <= px - x_g < w  and  0 <= py - y_g < h  and  glyphs[idx][(y0 + py - y_g) * gd + (x0 + px - x_g)] > ink_threshold,
 * and 0 where there is none.  A digit whose idx lies outside [0, Gn), or whose crop box leaves its gd x gd frame (x0 < 0,
 * y0 < 0, w < 0, h < 0, x0 + w > gd or y0 + h > gd), labels nothing.  (A NaN glyph value is not ink.)
 * Refusals, on the host before any HIP call, in this order.  AIR_EINVAL: a null descriptor; B, G, gd, C or max_digits < 1;
 * ink_threshold < 0 or NaN.  AIR_ELIMIT: C > AIR_SCENE_MAX_CANVAS, gd > AIR_SCENE_MAX_GLYPH, max_digits >
 * AIR_SCENE_MAX_DIGITS.  AIR_EINVAL: a null pointer.  16-byte stores where C * C is a multiple of 16 and mask is 16-byte
 * aligned, byte stores otherwise.
 *
 * air_segmentation.  One workgroup per image i < k; the taps and windows of all T steps are staged in LDS exactly as
 * air_render stages them (the same device code), <= 160 KB: AIR_ELIMIT beyond.
 * Predicted label of canvas pixel (py, px).  The term of step t is the one compose adds for it:
 *   c_t = z_pres_t * (((wa * Ia + wb * Ib) + wc * Ic) + wd * Id)
 * -- the window -> canvas taps of theta_recon, fp32, the same operations in the same order (the translation unit has
 * -ffp-contract=off) -- taken only for ACTIVE steps (att[t][i][AIR_ATT_MASK] != 0).  Walk t = 0 .. T - 1 with
 * best = pred_threshold, label = 0:  if (c_t > best) { best = c_t; label = t + 1; }.  A tie keeps the smaller t, a NaN never
 * takes the pixel, and a pixel no step lifts above pred_threshold is background (label 0).
 * Table of image i: n[r][c] = the number of its C * C pixels with truth r and prediction c, int32, r = 0 .. G, c = 0 .. T;
 * the truth of a pixel is gt_mask[i][p], a value > G counting as 0.
 * FG-ARI, over the rows r >= 1 only, in int64:  a_r = sum_c n[r][c],  b_c = sum_{r>=1} n[r][c],  N = sum_{r>=1} a_r,
 *   S = sum_{r>=1,c} n (n - 1) / 2,  A = sum_{r>=1} a_r (a_r - 1) / 2,  Bs = sum_c b_c (b_c - 1) / 2,  P = N (N - 1) / 2.
 * The image is SCORED only when N >= 2; then in fp64, in this order:
 *   E = (double)A * (double)Bs / (double)P;   M = ((double)A + (double)Bs) / 2.0;
 *   ari = (M == E) ? 1.0 : ((double)S - E) / (M - E).
 * Mask IoU.  Digit r >= 1 is PRESENT when a_r > 0.  With colsum_c = sum_{r>=0} n[r][c]:  v = 0.0; for c = 1 .. T in order:
 *   q = (double)n[r][c] / (double)(a_r + colsum_c - n[r][c]);  if (q > v) v = q.     An absent digit has v = 0.
 * Outputs, each nullable on its own: pred_mask [k, C * C] uint8; tables [k, (G + 1) * (T + 1)] int32; ari [k] fp64 (NaN for
 * an unscored image); mask_iou [k, G] fp64 (digit r at column r - 1).
 * Accumulators: the caller zeroes them once; a call ADDS.
 *   counts[AIR_SEG_IMAGES] += k, [SCORED] += scored images, [PRESENT] += present digits, [FG_PIXELS] += sum N,
 *   [FG_MISSED] += sum_{r>=1} n[r][0], [BG_CLAIMED] += sum_{c>=1} n[0][c].  Integers: any order, the same sums.
 *   sums[AIR_SEG_ARI / AIR_SEG_MASK_IOU] += in the ONE order of air_localization, with its group AIR_LOC_GROUP:
 *     1. image i:  ARI: its ari, +0.0 for an unscored image.  MASK_IOU: (((+0.0 + v_1) + v_2) + ...) over its present digits
 *        in order;
 *     2. the adjacent pairwise tree over each group of AIR_LOC_GROUP images (+0.0 for an image >= k);
 *     3. the batch total = (((+0.0 + group 0) + group 1) + ...) in group order;
 *     4. sums[.] = incoming sums[.] + the batch total.
 * Two launches on the caller's stream (the per-image kernel, which leaves the images' two values and five integer totals in
 * the workspace; one small fold), no synchronisation, no host read, no atomics on memory: the same inputs give the same bits.  Rows >= k of
 * att / vrec are never read, gt_mask has k rows, and rows >= k of the outputs are never written.  pred_mask is stored 16
 * bytes at a time where C * C is a multiple of 16 and pred_mask is 16-byte aligned, byte by byte otherwise.
 * Refusals, on the host before any HIP call, in this order.  AIR_EINVAL: a null descriptor; T, B, k or G < 1; k > B.
 * AIR_ELIMIT: T > AIR_SEG_MAX_STEPS, G > AIR_SEG_MAX_DIGITS.  AIR_EINVAL: C < 2, w < 2.  AIR_ELIMIT: C > AIR_SEG_MAX_CANVAS,
 * w > AIR_SEG_MAX_WINDOW, more than 160 KB of LDS.  AIR_EINVAL: pred_threshold not in [0, 1) (NaN included); a null att,
 * vrec, gt_mask, counts, sums or workspace. */
typedef struct {
    const float* glyphs;                 /* [G, gd * gd]                                                                */
    const int32_t* crops;                /* [G, 4] x0, y0, w, h                                                         */
    const int32_t* digits;               /* [B]                                                                         */
    const int32_t* indices;              /* [B, max_digits]                                                             */
    const int32_t* positions;            /* [B, 2 * max_digits] (x, y)                                                  */
    uint8_t* mask;                       /* out [B, C * C]                                                              */
    int32_t B, G, gd, C, max_digits;
    float ink_threshold;
} air_scene_masks_t;
int air_scene_masks(const air_scene_masks_t* args, void* stream);

#define AIR_SEG_MAX_STEPS 16
#define AIR_SEG_MAX_DIGITS 16
#define AIR_SEG_MAX_CANVAS 128
#define AIR_SEG_MAX_WINDOW 32
enum { AIR_SEG_IMAGES = 0, AIR_SEG_SCORED = 1, AIR_SEG_PRESENT = 2, AIR_SEG_FG_PIXELS = 3, AIR_SEG_FG_MISSED = 4,
       AIR_SEG_BG_CLAIMED = 5, AIR_SEG_COUNTS = 6 };
enum { AIR_SEG_ARI = 0, AIR_SEG_MASK_IOU = 1, AIR_SEG_SUMS = 2 };
typedef struct {
    const float* att;                    /* [T, B, AIR_ATT_STRIDE] of the pass just run                                 */
    const float* vrec;                   /* [T, B, w * w] the decoded windows of the pass                               */
    const uint8_t* gt_mask;              /* [k, C * C] instance labels, 0 the background                                */
    uint8_t* pred_mask;                  /* out, nullable [k, C * C]                                                    */
    int32_t* tables;                     /* out, nullable [k, (G + 1) * (T + 1)]                                        */
    double* ari;                         /* out, nullable [k]                                                           */
    double* mask_iou;                    /* out, nullable [k, G]                                                        */
    int64_t* counts;                     /* in / out [AIR_SEG_COUNTS]                                                   */
    double* sums;                        /* in / out [AIR_SEG_SUMS]                                                     */
    int32_t T, B, k, G, C, w;
    float pred_threshold;
} air_segmentation_t;
/* `workspace`: a device buffer of at least air_segmentation_workspace_bytes(T, B, k, G) bytes, 8-byte aligned (the two
 * values and the five integer totals of every image: 56 k bytes) */
int air_segmentation(const air_segmentation_t* args, void* workspace, void* stream);
/* bytes of `workspace`, or AIR_EINVAL / AIR_ELIMIT for a (T, B, k, G) the entry point refuses -- no GPU is touched */
int64_t air_segmentation_workspace_bytes(int T, int B, int k, int G);

/* ---- latent probe (additive to ABI 6) --------------------------------------------------------------------------------------
 * What do the what-codes say?  Two label-based, training-free measurements of a set of latent codes (the posterior means
 * air_embed_collect gathers): the leave-one-out k-nearest-neighbour accuracy of their labels with its confusion matrix, and
 * the number of ACTIVE UNITS, the dimensions whose value varies over the set (Burda et al., Importance Weighted Autoencoders:
 * variance > 0.01).  air/metrics.py (LatentProbe) and air/embeddings.py (probe) are the callers;
 * tests/latent_probe_cases.py restates every operation below.  All arithmetic is fp64 in exactly the order written here (the
 * translation unit has -ffp-contract=off).
 *
 * Rows.  M_eff = rows ? clamp(*rows, 0, M) : M -- `rows` points to ONE device int32 (a collector's cursor,
 * counters[AIR_EMBED_MATCHED], can be passed without a host read).  Rows >= M_eff of latents and labels are never read; the
 * launches are sized by M.  x[i][z] = latents[i * Z + z]; rows are only 4-byte aligned and are read float by float.
 * Row i < M_eff is VALID when all its Z values are finite and 0 <= labels[i] < classes.  An invalid row is neither a query
 * nor a neighbour.  V = the number of valid rows.
 *
 * Squared distance of two valid rows:  d2(i, j) = (((+0.0 + e_0 * e_0) + e_1 * e_1) + ...), z ascending,
 *   e_z = (double)x[i][z] - (double)x[j][z].
 * No square root (the order is defined on d2), never the |a|^2 + |b|^2 - 2 a.b form; d2(i, j) == d2(j, i) bit for bit.
 *
 * Neighbours of a valid row i: the valid rows j != i ordered by (d2 ascending, then j ascending); the first
 * kk = min(k, V - 1) are kept.  kk == 0: the row is UNSCORED.  The order is total, so the result does not depend on how the
 * kernels partition the rows (AIR_PROBE_QUERY_TILE, AIR_PROBE_REF_TILE, AIR_PROBE_PASS_ROWS and air_latent_probe_splits are
 * facts of the launch, exported for the tests, not of the result).
 * Vote: votes[c] = the neighbours with label c; the class with the most votes wins, a tie goes to the tied class whose first
 * member comes earliest in the neighbour order.  pred[i] = that class.
 *
 * Outputs: EVERY element is written on EVERY call (nothing accumulates: k-NN is a whole-set operation).
 *   pred [M] (nullable): the class, -1 for an invalid row, an unscored row and a row >= M_eff.
 *   neighbours [M, k], neighbour_d2 [M, k] (nullable TOGETHER): the kept rows in order and their d2, then -1 and +0.0.
 *   counts[AIR_PROBE_ROWS] = M_eff, [VALID] = V, [SCORED] = scored rows, [CORRECT] = those with pred == label,
 *   [ACTIVE_UNITS] (below), then counts[AIR_PROBE_COUNTS + label * classes + pred] = the scored rows with that label and that
 *   prediction (truth x predicted).  Integer atomics: any order, the same sums.
 *   moments [2 Z]: mean_z at [z], var_z at [Z + z], over the valid rows:
 *     S_z = the sum of (double)x[i][z] in the ONE order of air_localization's sums: rows in groups of AIR_LOC_GROUP, each folded
 *     by the adjacent pairwise tree (v[m] = v[2 m] + v[2 m + 1], eight times), +0.0 for an absent or invalid row; the group
 *     totals added one by one from +0.0 in group order.   mean_z = S_z / (double)V.
 *     Q_z = the sum of (x - mean_z) * (x - mean_z) in the same order (+0.0 for an absent or invalid row).  var_z = Q_z / V.
 *   counts[AIR_PROBE_ACTIVE_UNITS] = the z with var_z > au_threshold.  V == 0: every mean and variance is the quiet NaN
 *   0x7FF8000000000000 and ACTIVE_UNITS is 0.
 * No floating-point atomics anywhere: the same inputs give the same bits.
 *
 * Four launches on the caller's stream, no synchronisation, no host read: validity flags (a thread per row; zeroes counts);
 * moments (a workgroup per dimension); pairs (a workgroup per AIR_PROBE_QUERY_TILE queries x one of
 * air_latent_probe_splits(M) contiguous runs of AIR_PROBE_REF_TILE-row reference tiles; each of its four waves takes
 * AIR_PROBE_PASS_ROWS rows of every tile for all the queries, the four lists are merged in the workgroup, and each query's k
 * best of the run go to the workspace); merge, vote and count (a thread per row).
 *
 * Refusals, on the host before any HIP call, in this order.  AIR_EINVAL: a null descriptor; M, Z, k or classes < 1;
 * au_threshold negative or NaN.  AIR_ELIMIT: k > AIR_PROBE_MAX_K, classes > AIR_PROBE_MAX_CLASSES, Z > AIR_PROBE_MAX_Z,
 * M > AIR_PROBE_MAX_ROWS.  AIR_EINVAL: a null latents, labels, counts, moments or workspace; exactly one of neighbours /
 * neighbour_d2 null.  AIR_EALIGN: moments, neighbour_d2 or the workspace not 8-byte aligned. */
#define AIR_PROBE_MAX_K 16
#define AIR_PROBE_MAX_CLASSES 64
#define AIR_PROBE_MAX_Z 256
#define AIR_PROBE_MAX_ROWS 32768
#define AIR_PROBE_QUERY_TILE 64
#define AIR_PROBE_REF_TILE 32
#define AIR_PROBE_MAX_SPLITS 8
#define AIR_PROBE_PASS_ROWS 8
enum { AIR_PROBE_ROWS = 0, AIR_PROBE_VALID = 1, AIR_PROBE_SCORED = 2, AIR_PROBE_CORRECT = 3, AIR_PROBE_ACTIVE_UNITS = 4,
       AIR_PROBE_COUNTS = 5 };
typedef struct {
    const float* latents;                /* [M, Z]                                                                      */
    const int32_t* labels;               /* [M]                                                                         */
    const int32_t* rows;                 /* nullable: ONE device int32, the rows in use (clamped to [0, M])             */
    int32_t* pred;                       /* out [M], nullable                                                           */
    int32_t* neighbours;                 /* out [M, k], nullable with neighbour_d2                                      */
    double* neighbour_d2;                /* out [M, k], nullable with neighbours                                        */
    int64_t* counts;                     /* out [AIR_PROBE_COUNTS + classes * classes]                                  */
    double* moments;                     /* out [2 Z]: means, then variances                                            */
    int32_t M, Z, k, classes;
    double au_threshold;
} air_latent_probe_t;
/* `workspace`: a device buffer of at least air_latent_probe_workspace_bytes(M, Z, k) bytes, 8-byte aligned (the partial
 * neighbour lists of every split and the validity flags) */
int air_latent_probe(const air_latent_probe_t* args, void* workspace, void* stream);
/* bytes of `workspace`, or AIR_EINVAL / AIR_ELIMIT for an (M, Z, k) the entry point refuses -- no GPU is touched */
int64_t air_latent_probe_workspace_bytes(int M, int Z, int k);
/* the reference runs the pairs launch splits M rows into: min(AIR_PROBE_MAX_SPLITS, ceil(M / AIR_PROBE_REF_TILE)); run s
 * holds the reference tiles [s * tps, (s + 1) * tps), tps = ceil(tiles / splits).  AIR_EINVAL: M < 1; AIR_ELIMIT: M >
 * AIR_PROBE_MAX_ROWS -- no GPU is touched */
int air_latent_probe_splits(int M);

/* ---- importance-weighted evaluation bound (additive to ABI 6) ----------------------------------------------------------------
 * The K-sample importance-weighted bound of a variational scene model, log (1/K) sum_k w_k, its effective sample size and
 * the posterior over the object count, from K passes of a test model on fresh noise (AIRModel.forward_sampled).  Two entry
 * points: air_importance_logw turns the buffers one pass left on the device into one row of log-weights, and
 * air_importance_fold reduces the K rows to per-image numbers and adds them to accumulators.  air/metrics.py
 * (ImportanceBound) is the caller; tests/importance_cases.py restates every operation below.
 *
 * All arithmetic is fp64 in exactly the order written here (the translation unit has -ffp-contract=off); every fp32 input
 * is widened first, one by one.  i < k is an image, t < T a step, j < Z a latent dimension.
 *
 * air_importance_logw -- row `sample` of the tables, ONE launch.  The weight of a sample is p(x, z) / q(z | x) at the
 * sample: log w = -(rec_loss + the log-ratios log q - log p of every latent the pass drew).
 *   lr(z, eps, lv, pm, pv, plv) = 0.5 * ((((z - pm) * (z - pm)) / pv + plv) - eps * eps - lv)
 * is that log-ratio of a Gaussian posterior N(mean, exp(lv)) against the prior N(pm, pv) (plv = log pv, the dyn slot the
 * loss reads), at the sample the noise eps gave: log q(z) = -0.5 (eps^2 + lv) and log p(z) = -0.5 ((z - pm)^2 / pv + plv) up
 * to the same constant.  It has no transcendental.  The pixel noise eps_x is drawn from ITS prior under q as well (the
 * likelihood noise of vae.py:37 is no latent of the posterior): its ratio is 1 and it has no term.
 *   scale_t = lr(att[t][i][AIR_ATT_S], eps_scale[t][i], out7[t][i][1], dyn[AIR_DYN_SCALE_PM], [SCALE_PV], [SCALE_PLV])
 *   shift_t = lr(att[t][i][AIR_ATT_X], eps_shift[t][i][0], out7[t][i][4], dyn[AIR_DYN_SHIFT_PM], [SHIFT_PV], [SHIFT_PLV])
 *           + lr(att[t][i][AIR_ATT_Y], eps_shift[t][i][1], out7[t][i][5], the same three)                     (x first)
 *   what_t  = (((+0.0 + l_0) + l_1) + ...) over j = 0 .. Z - 1 IN ORDER, l_j = lr(z[t][i][j], eps_z[t][i][j],
 *             ml[t][i][Z + j], dyn[AIR_DYN_VAE_PM], [VAE_PV], [VAE_PLV]); z is addressed with ldz (0 = Z) as in
 *             air_bottleneck_fwd_t.  The sum is SEQUENTIAL: one lane owns an (image, step) and runs the Z loop alone.
 *   a_t = att[t][i][AIR_ATT_MASK_PREV] != 0 ? (double)att[t][i][AIR_ATT_KL_Z] : 0.0     (the Monte-Carlo z_pres log-ratio)
 *   b_t = att[t][i][AIR_ATT_MASK] != 0 ? (scale_t + shift_t) + what_t : 0.0
 *   loss_i = ((((double)rec_loss[i] + (a_0 + b_0)) + (a_1 + b_1)) + ...) over t = 0 .. T - 1 in order;   logw_i = -loss_i
 * The gates are SELECTS: whatever the records of a step hold that the gate closes (a NaN included) never reaches a result.
 * logw[sample][i] = logw_i;  digits[sample][i] = run_digits[i];  when terms is given, terms[sample][i][AIR_IW_TERM_*] =
 * (double)rec_loss[i], then the four sums (((+0.0 + v_0) + v_1) + ...) over t in order of a_t (Z_PRES) and of the gated
 * scale_t, shift_t and what_t (MASK_t != 0 ? v : 0.0).  The tables have K rows of B columns; only row `sample`, columns
 * < k, is written, and rows >= k of the inputs are never read.
 * Refusals, on the host before any HIP call, in this order.  AIR_EINVAL: a null descriptor; T, B, k, Z or K < 1; k > B;
 * ldz not 0 and < Z; sample not in [0, K).  AIR_ELIMIT: T > AIR_MAX_STEPS, K > AIR_IW_MAX_SAMPLES, Z > AIR_IW_MAX_Z.
 * AIR_EINVAL: a null att, out7, ml, z, eps_scale, eps_shift, eps_z, rec_loss, run_digits, dyn, logw or digits. */
#define AIR_IW_MAX_SAMPLES 64
#define AIR_IW_MAX_Z 256
enum { AIR_IW_TERM_REC = 0, AIR_IW_TERM_Z_PRES = 1, AIR_IW_TERM_SCALE = 2, AIR_IW_TERM_SHIFT = 3, AIR_IW_TERM_WHAT = 4,
       AIR_IW_TERMS = 5 };
typedef struct {
    const float* att;                    /* [T, B, AIR_ATT_STRIDE] of the pass just run                                 */
    const float* out7;                   /* [T, B, AIR_OUT_STRIDE]: the posterior parameters of scale and shift         */
    const float* ml;                     /* [T, B, 2 Z]: mean | log-variance of the what-code                           */
    const float* z;                      /* [T, B, ldz]: the what-code samples                                          */
    const float* eps_scale;              /* [T, B]                                                                      */
    const float* eps_shift;              /* [T, B, 2]                                                                   */
    const float* eps_z;                  /* [T, B, Z]                                                                   */
    const float* rec_loss;               /* [B]                                                                         */
    const int32_t* run_digits;           /* [B]                                                                         */
    const float* dyn;                    /* AIR_DYN_* device array                                                      */
    double* logw;                        /* in / out [K, B]                                                             */
    int32_t* digits;                     /* in / out [K, B]                                                             */
    double* terms;                       /* in / out [K, B, AIR_IW_TERMS], nullable                                     */
    int32_t T, B, k, Z, ldz, K;
} air_importance_t;
int air_importance_logw(const air_importance_t* args, int sample, void* stream);

/* air_importance_fold -- the [K, k] tables folded into per-image numbers and the accumulators.  Per image i < k, with
 * l_s = logw[s][i] and d_s = digits[s][i] clamped to [0, T], s = 0 .. K - 1 in order everywhere:
 *   m = the first maximum: m = l_0; then s = 1 ..: if (l_s > m || l_s != l_s) m = l_s  (a NaN stays).  An image whose m is
 *   not finite (every weight zero, an infinite one, a NaN) is DEGENERATE: it adds 1 to counts[AIR_IW_DEGENERATE] and nothing
 *   else to any sum or count but IMAGES; its optional outputs are NaN, NaN and -1.  Otherwise, e_s = exp(l_s - m):
 *   S = (((+0.0 + e_0) + e_1) + ...),  S2 = (((+0.0 + e_0 * e_0) + e_1 * e_1) + ...),  L = (((+0.0 + l_0) + l_1) + ...)
 *   bound_i = m + log(S / K)     elbo_i = L / K     ess_i = (S * S) / S2          (K widened)
 *   W_c = (((+0.0 + [d_0 == c] e_0) + ...), the terms of other counts skipped, for c = 0 .. T: the count posterior
 *   map_i = the first c with the largest W_c (W_c > best, best starts at W_0)
 *   entropy_i = -(((+0.0 + p_0 log p_0) + ...) over c in order, p_c = W_c / S, a c with W_c == 0 skipped
 *   split_i = any d_s != d_0
 * exp and log are the device library's fp64 functions (within 3 ulp: the tests allow 8 (K + T + 2) 2^-52 on the sums).
 * Accumulators: the caller zeroes them once; a call ADDS, so the chunks of a test set add up.
 *   counts[AIR_IW_IMAGES] += k, [DEGENERATE] += the degenerate ones, [SCORED] += the others, [SPLIT] += sum split_i and,
 *   when targets is given (g_i = targets[i] clamped to [0, T]): [MAP_CORRECT] += images with map_i == g_i, and the confusion
 *   matrix counts[AIR_IW_COUNTS + g_i * (T + 1) + map_i] += 1  ((T + 1) rows, truth, of (T + 1), MAP).  Integer atomics.
 *   sums[AIR_IW_BOUND / ELBO / ESS / ENTROPY] += bound_i / elbo_i / ess_i / entropy_i, each in the ONE order of
 *   air_localization's sums with its group AIR_LOC_GROUP: the values of a group (+0.0 for an image >= k or degenerate)
 *   folded by the adjacent pairwise tree, the group totals added in group order from +0.0, then sums[.] = incoming + the
 *   batch total.  The order depends on k alone, so the same tables give the same bits; two calls over the halves of a
 *   batch associate the additions differently from one call over the whole and agree with it to rounding only.
 * bound, ess [k] fp64 and map [k] int32 are nullable, each on its own.  Two launches, no synchronisation, no host read.
 * Refusals, in this order.  AIR_EINVAL: a null descriptor; T, B, k or K < 1; k > B.  AIR_ELIMIT: T > AIR_MAX_STEPS,
 * K > AIR_IW_MAX_SAMPLES.  AIR_EINVAL: a null logw, digits, counts, sums or workspace. */
enum { AIR_IW_IMAGES = 0, AIR_IW_SCORED = 1, AIR_IW_DEGENERATE = 2, AIR_IW_MAP_CORRECT = 3, AIR_IW_SPLIT = 4,
       AIR_IW_COUNTS = 5 };
enum { AIR_IW_BOUND = 0, AIR_IW_ELBO = 1, AIR_IW_ESS = 2, AIR_IW_ENTROPY = 3, AIR_IW_SUMS = 4 };
typedef struct {
    const double* logw;                  /* [K, B]                                                                      */
    const int32_t* digits;               /* [K, B]                                                                      */
    const int32_t* targets;              /* [k] true counts, nullable                                                   */
    double* bound;                       /* out [k], nullable                                                           */
    double* ess;                         /* out [k], nullable                                                           */
    int32_t* map;                        /* out [k], nullable                                                           */
    int64_t* counts;                     /* in / out [AIR_IW_COUNTS + (T + 1) * (T + 1)]                                */
    double* sums;                        /* in / out [AIR_IW_SUMS]                                                      */
    int32_t T, B, k, K;
} air_importance_fold_t;
/* `workspace`: a device buffer of at least air_importance_fold_workspace_bytes(T, B, k, K) bytes, 8-byte aligned (the
 * per-group partial sums) */
int air_importance_fold(const air_importance_fold_t* args, void* workspace, void* stream);
/* bytes of `workspace`, or AIR_EINVAL / AIR_ELIMIT for a (T, B, k, K) the entry point refuses -- no GPU is touched */
int64_t air_importance_fold_workspace_bytes(int T, int B, int k, int K);

/* ---- latent clusters (additive to ABI 6) -------------------------------------------------------------------------------------
 * Do classes emerge in the what-codes ON THEIR OWN?  Exact k-means (Lloyd's loop, R restarts from seeded draws) over a set of
 * latent codes, and -- where labels are given -- the cluster x class table of the best restart with each cluster's majority
 * class, from which the caller derives clustering accuracy (purity), the adjusted Rand index and the normalised mutual
 * information.  air/metrics.py (LatentClusters) and air/embeddings.py (cluster) are the callers;
 * tests/latent_kmeans_cases.py restates every operation below.  All arithmetic is fp64 in exactly the order written here (the
 * translation unit has -ffp-contract=off); no floating-point atomics, no grid-wide wait: the same inputs give the same bits.
 *
 * Rows.  M_eff = rows ? clamp(*rows, 0, M) : M, as for the latent probe; rows >= M_eff of latents and labels are never read.
 * x[i][z] = latents[i * Z + z], read float by float (rows are only 4-byte aligned).  Row i < M_eff is VALID when all its Z
 * values are finite -- the label plays no part.  A valid row is LABELLED when labels is not null and 0 <= labels[i] < classes.
 * V = the number of valid rows, k_eff = min(k, V).  Clusters c >= k_eff do not exist.
 *
 * Squared distance of a valid row and a centroid:  d2(i, c) = (((+0.0 + e_0 * e_0) + e_1 * e_1) + ...), z ascending,
 *   e_z = (double)x[i][z] - mu[c][z].
 *
 * Start of restart r < R.  idx[0 .. V - 1] = the valid rows in ascending order.  For t = 0 .. k_eff - 1:
 *   j = t + umulhi(word_t, V - t) (the high 32 bits of the 64-bit product), swap idx[t] and idx[j]; then mu[t][z] =
 *   (double)x[idx[t]][z].  word_t is word t & 3 of Philox4x32-10 (csrc/air_philox.h) with key (seed & 0xffffffff, seed >> 32)
 *   and counter (r, t >> 2, 0, 0x4B4D4E53).  Integers only; the k_eff start rows of a restart are distinct rows.
 *
 * Lloyd's loop of a restart.  a[i] = -1 for every row; for it = 1 .. max_iters:
 *   assign  a'[i] = the c < k_eff with the smallest d2(i, c), a tie to the lowest c, for every valid row;
 *           changed = the valid rows with a'[i] != a[i];  a = a'.
 *   stop    when changed == 0 (CONVERGED, restart_iters[r] = it) or it == max_iters (not converged unless changed == 0).
 *   update  otherwise, for every cluster with n_c > 0 members: mu[c][z] = S / (double)n_c, S = the sum of (double)x[i][z]
 *           over its members added one by one from +0.0 in ascending row order.  A cluster without members keeps its
 *           centroid (and may win rows later).
 * The restart's assignment, its per-row d2, its centroids and its inertia are those of the LAST assign step (so the centroids
 * of a converged restart are the stated means of its members).  restart_inertia[r] = the sum of d2(i, a[i]) over the valid
 * rows, added one by one from +0.0 in ascending row order.
 * Best restart: the lowest inertia, a tie to the lowest r (restarts that find the same partition under permuted cluster
 * indices tie to the bit).
 *
 * Outputs: EVERY element is written on EVERY call.
 *   assignment [M]: the cluster of the best restart; -1 for an invalid row and a row >= M_eff.
 *   row_d2 [M] (nullable): d2(i, assignment[i]); +0.0 where the assignment is -1.
 *   centroids [k, Z]: of the best restart; clusters >= k_eff hold the quiet NaN 0x7FF8000000000000.
 *   restart_inertia [R], restart_iters [R].
 *   counts[AIR_KMEANS_ROWS] = M_eff, [VALID] = V, [LABELLED] = labelled rows, [CORRECT] = sum over c of max_l table[c][l],
 *   [LIVE] = clusters of the best restart with members, [BEST] = its index, [ITERS] = its iterations, [CONVERGED] = 0 / 1 for
 *   it, [RESTARTS_CONVERGED] = how many restarts converged; then sizes[k] (valid members per cluster), majority[k] (the first
 *   maximum of table[c][.], -1 for a cluster without labelled members) and table[k x classes] (the labelled rows by
 *   cluster x label) at counts[AIR_KMEANS_COUNTS], [AIR_KMEANS_COUNTS + k] and [AIR_KMEANS_COUNTS + 2 k].
 * V == 0: no restart runs.  restart_inertia is the quiet NaN, restart_iters 0, every centroid NaN, every assignment -1, and
 * every count but ROWS is 0 (majority: -1).
 *
 * Three launches on the caller's stream, no synchronisation, no host read: validity flags (a thread per row); the restarts (a
 * workgroup per restart, its whole loop inside the kernel, the centroids in up to 130 KiB of LDS); the pick (one workgroup:
 * the winner copied out, the table and the counts).  Call it eagerly once before capturing it (the LDS grant).
 *
 * Refusals, on the host before any HIP call, in this order.  AIR_EINVAL: a null descriptor; M, Z, k, classes, restarts or
 * max_iters < 1.  AIR_ELIMIT: k > AIR_KMEANS_MAX_K, restarts > AIR_KMEANS_MAX_RESTARTS, max_iters > AIR_KMEANS_MAX_ITERS,
 * Z > AIR_PROBE_MAX_Z, classes > AIR_PROBE_MAX_CLASSES, M > AIR_PROBE_MAX_ROWS.  AIR_EINVAL: a null latents, assignment,
 * centroids, restart_inertia, restart_iters, counts or workspace.  AIR_EALIGN: row_d2, centroids, restart_inertia or the
 * workspace not 8-byte aligned. */
#define AIR_KMEANS_MAX_K 64
#define AIR_KMEANS_MAX_RESTARTS 32
#define AIR_KMEANS_MAX_ITERS 1000
enum { AIR_KMEANS_ROWS = 0, AIR_KMEANS_VALID = 1, AIR_KMEANS_LABELLED = 2, AIR_KMEANS_CORRECT = 3, AIR_KMEANS_LIVE = 4,
       AIR_KMEANS_BEST = 5, AIR_KMEANS_ITERS = 6, AIR_KMEANS_CONVERGED = 7, AIR_KMEANS_RESTARTS_CONVERGED = 8,
       AIR_KMEANS_COUNTS = 9 };
typedef struct {
    const float* latents;                /* [M, Z]                                                                      */
    const int32_t* labels;               /* [M], nullable: clustering needs none                                        */
    const int32_t* rows;                 /* nullable: ONE device int32, the rows in use (clamped to [0, M])             */
    int32_t* assignment;                 /* out [M]                                                                     */
    double* row_d2;                      /* out [M], nullable                                                           */
    double* centroids;                   /* out [k, Z]                                                                  */
    double* restart_inertia;             /* out [restarts]                                                              */
    int32_t* restart_iters;              /* out [restarts]                                                              */
    int64_t* counts;                     /* out [AIR_KMEANS_COUNTS + 2 k + k * classes]                                 */
    int32_t M, Z, k, classes, restarts, max_iters;
    uint64_t seed;
} air_latent_kmeans_t;
/* `workspace`: a device buffer of at least air_latent_kmeans_workspace_bytes(M, Z, k, restarts) bytes, 8-byte aligned (the
 * assignment, d2 and centroids of every restart, the validity flags) */
int air_latent_kmeans(const air_latent_kmeans_t* args, void* workspace, void* stream);
/* bytes of `workspace`: 8 R M + 8 R k Z + pad8(4 R M) + pad8(4 M) + pad8(4 R), or AIR_EINVAL / AIR_ELIMIT for an
 * (M, Z, k, restarts) the entry point refuses -- no GPU is touched */
int64_t air_latent_kmeans_workspace_bytes(int M, int Z, int k, int restarts);

#ifdef __cplusplus
}
#endif
#endif /* AIR_HIP_H */
