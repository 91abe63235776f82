"""Case tables, inputs and references for the kernels AROUND the train step (tests/test_gpu_around_step.py, pinned on the CPU
by tests/test_around_step_cases.py): the input queue and the row gather of csrc/air_input.hip, air_summaries
(csrc/air_summaries.hip), air_scene_records and air_render (csrc/air_generate.hip).

They decide which records a model trains on, what generate() draws and what TensorBoard shows; a fault in them gives no NaN
and no crash.  So every reference here is the plainest statement of the operation: the literal pop-and-swap queue
(oracle.shuffle_queue.literal_dequeue) started from any state, numpy indexing for the gather, oracle/summaries.py on [B, T']
stacks sliced from the record array, the formulas of include/air_hip.h (the generation block) in float64 on the fp32 inputs,
and step_limit_cases.running_recon64 for the canvas.

Where a comparison could sit on a discontinuity (round(z_pres), S < threshold, the clip of a tap) the INPUTS are built away
from it; the margins are computed from the float64 reference alone and asserted on the CPU.  No result is filtered."""
import functools

import numpy as np

import pointwise_edge_cases as pec
import step_limit_cases as slc
from air import _hip as H
from oracle import air_oracle as ao
from oracle import shuffle_queue as sq
from oracle import summaries as osum

# ---- 1. the shuffle queue ---------------------------------------------------------------------------------------------
# (capacity, batch, min_after_dequeue, n_records)
QUEUE_GEOMETRIES = [
    (132, 128, 0, 1000),           # the generic branch (64 < batch), almost every slot a back that moves
    (128, 128, 0, 50),             # capacity == batch: every slot a back, the modulus runs down to 1, the stream wraps inside one refill
    (72, 68, 0, 7),                # just past one wave
    (68, 64, 0, 7),                # the wave branch, an event in every batch
    (4, 4, 0, 1),                  # the smallest of everything
    (10, 4, 6, 3),                 # one drawing thread
    (3000, 256, 100, 60000),       # the generic branch at a mid-size batch
    (10240, 1024, 9000, 60000),    # capacity * 4 + batch * 8 == 48 KB at the largest batch: all 1024 threads pick
    (12160, 64, 12000, 60000),     # the same limit at the reference's batch
]
QUEUE_SEED = 5
# what every geometry runs: (kind, count) -- single dequeues, one air_shuffle_batch_dequeue_many, single ones again
QUEUE_SCHEDULE = (("single", 12), ("many", 5), ("single", 3))
LDS_LIMIT = 48 * 1024
WAVE = 64

# a stream position and a dequeue number beyond 2^32: four single dequeues cross the point where the low word of the
# counter wraps (dequeue numbers 2^32 - 2 .. 2^32 + 1), one dequeue_many of 3 follows
LARGE_GEOMETRY = (100, 8, 50, 37)
LARGE_STATE = (2 ** 32 + 5, 2 ** 32 - 2)
LARGE_SEED = 0x1234567890AB
LARGE_SCHEDULE = (("single", 4), ("many", 3))


def schedule_batches(schedule):
    return sum(n for _, n in schedule)


def initial_queue(geometry):
    """what air_shuffle_batch_init leaves: the first `capacity` records of the stream"""
    cap, _, _, n_rec = geometry
    return [i % n_rec for i in range(cap)]


def large_state_queue():
    """an arbitrary valid queue image of LARGE_GEOMETRY: record indices with repeats, in no order"""
    cap, _, _, n_rec = LARGE_GEOMETRY
    return [int(v) for v in np.random.RandomState(32).randint(0, n_rec, cap)]


@functools.lru_cache(maxsize=None)
def queue_model(geometry, seed, schedule, start=None):
    """the literal queue through a schedule: (picks [batches, batch] int32, queue image int32, (stream position, dequeues)).
    start: (state, queue image as a tuple); None: the state after air_shuffle_batch_init"""
    cap, batch, mad, n_rec = geometry
    assert cap - batch >= mad
    (pos, n), q = ((cap, 0), initial_queue(geometry)) if start is None else (start[0], list(start[1]))
    picks = []
    for _ in range(schedule_batches(schedule)):
        p, q = sq.literal_dequeue(q, batch, sq.device_draws(seed, n, batch), pos, n_rec)
        picks.append(p)
        pos, n = pos + batch, n + 1
    return np.asarray(picks, np.int32), np.asarray(q, np.int32), (pos, n)


def wave_events(geometry, seed, batches, first=0):
    """per dequeue number, from the draws alone: does the wave-level resolver of dequeue_batch (batch <= 64) see an EVENT --
    two picks on one slot, or a pick among the last `batch` slots -- and walk, or does it take the short way"""
    cap, batch = geometry[:2]
    out = []
    for n in range(first, first + batches):
        idx = [r % (cap - k) for k, r in enumerate(sq.device_draws(seed, n, batch))]
        out.append(len(set(idx)) < batch or max(idx) >= cap - batch)
    return out


# ---- 2. air_batch_gather ----------------------------------------------------------------------------------------------
GATHER_D = [4, 8, 1020, 4096, 4100, 16388]       # one float4; two; D / 4 = 1024 is one slice of a row, 1025 two; 4097 five
GATHER_BATCH = [1, 3, 64]
GATHER_RECORDS = [1, 5, 300]
GATHER_MODES = ["both", "digits_only", "none"]   # digits and out_digits; digits with out_digits NULL; both NULL
GATHER_SLICE = 4 * 256                           # float4s per (row, slice) workgroup
GATHER_CASES = [dict(D=D, batch=b, records=GATHER_RECORDS[(i + j) % 3], mode=GATHER_MODES[(i + 2 * j) % 3])
                for i, D in enumerate(GATHER_D) for j, b in enumerate(GATHER_BATCH)]


def gather_inputs(c):
    """images [records, D] in (0, 1), digits in 0 .. 9, picks [batch] with the last record first, then the first, and the
    last pick a repeat of pick 0 (batch >= 3; batch 1 picks the last record)"""
    rng = pec._seed(21, c["D"], c["batch"], c["records"])
    n, b = c["records"], c["batch"]
    picks = rng.randint(0, n, b).astype(np.int32)
    picks[0] = n - 1
    if b >= 3:
        picks[1], picks[-1] = 0, picks[0]
    return dict(images=rng.rand(n, c["D"]).astype(np.float32), digits=rng.randint(0, 10, n).astype(np.int32), picks=picks)


# ---- 3. air_summaries -------------------------------------------------------------------------------------------------
SUMMARY_B = [1, 63, 64, 65, 257, 1000]
SUMMARY_CONFIGS = [(1, 0, 1), (3, 2, 1), (3, 2, 3), (16, 6, 16), (16, 6, 9), (16, 0, 2)]     # (N, max_digits, T')
# not the full product: every configuration with a B below one wave and a B past one workgroup, and every B
_SUMMARY_BS = [(1, 257, 64), (63, 1000), (1, 257, 65), (63, 1000, 64), (1, 257, 65), (63, 1000)]
SUMMARY_CASES = [dict(B=B, N=N, max_digits=md, T=T) for (N, md, T), Bs in zip(SUMMARY_CONFIGS, _SUMMARY_BS) for B in Bs]
SUMMARY_TOL = (2e-7, 0.0)                        # tests/test_summaries.py: rtol 2e-7, atol 0, NaN where the reference is NaN
SUMMARY_SLOTS = ("S", "ZPROB", "KL_Z", "KL_SCALE", "KL_SHIFT", "KL_VAE")       # the rows of the launch, in its order
SUMMARY_GROUPS_MAX = 6                           # max_digits the entry point admits


def summary_inputs(c):
    """att [N, B, 16]: NaN in the nine slots the kernel has no business with; the six value slots positive in rows < T' and
    NaN in rows >= T' (the reference pads those columns with zeros: the kernel must not read them into a mean); MASK 1 for
    some images -- at one step for a single one -- at every step < T' - 1 and 0 from step T' - 1 on.
    digits in 0 .. N, targets in 0 .. max_digits + 2 (above max_digits: counted in _all_dig only).  Two kinds of empty
    group: the images of target group `lone` all have digits 0, so the group is empty in every masked row and not in the
    others; with max_digits >= 2 and B >= 63 no image has target max_digits, so that group is empty in every row"""
    B, N, md, T = c["B"], c["N"], c["max_digits"], c["T"]
    rng = pec._seed(22, B, N, md, T)
    att = np.full((N, B, H.ATT_STRIDE), np.nan, np.float32)
    for name in SUMMARY_SLOTS:
        att[:T, :, getattr(H, "ATT_" + name)] = rng.uniform(0.05, 3.0, (T, B))
    mask = np.zeros((N, B), np.float32)
    for t in range(T - 1):
        mask[t] = rng.uniform(size=B) < 0.3
        if t == 0:
            mask[t] = 0.0                                   # one image alone keeps the loop going, in the last stride of the batch
        mask[t, (B - 1 - 7 * t) % B] = 1.0
    att[..., H.ATT_MASK] = mask
    allowed = [g for g in range(md + 3) if not (md >= 2 and B >= 63 and g == md)]
    targets = rng.choice(allowed, B).astype(np.int32)
    digits = rng.randint(0, N + 1, B).astype(np.int32)
    lone = md // 2
    digits[targets == lone] = 0
    return dict(att=att, targets=targets, digits=digits, lone=lone,
                rec_loss=rng.uniform(100.0, 2000.0, B).astype(np.float32), loss_item=rng.uniform(150.0, 2900.0, B).astype(np.float32),
                scalars=rng.uniform(0.1, 900.0, 2).astype(np.float32))


def summary_reference(c, x):
    """oracle.summaries.summaries on the [B, T'] stacks sliced from the same fp32 arrays"""
    T = c["T"]
    stacks = [x["att"][:T, :, getattr(H, "ATT_" + name)].T for name in SUMMARY_SLOTS]
    return osum.summaries(x["scalars"][0], x["scalars"][1], x["targets"], x["digits"], x["rec_loss"], x["loss_item"],
                          *stacks, c["N"], c["max_digits"])


def summary_ratio(got, ref):
    """largest |got - ref| / (2e-7 |ref|) over the finite entries; inf where the NaN positions differ, where a value is
    infinite or where the reference is 0 and the value is not"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.inf
    k = ~np.isnan(ref)
    g, r = got[k], ref[k]
    if not np.isfinite(g).all() or (g[r == 0] != 0).any():
        return np.inf
    nz = r != 0
    return float((np.abs(g[nz] - r[nz]) / (SUMMARY_TOL[0] * np.abs(r[nz]))).max()) if nz.any() else 0.0


# ---- 4. air_scene_records ---------------------------------------------------------------------------------------------
# (B, N, Z, ldz, z16)
SCENE_SHAPES = [
    (1, 1, 1, 1, False),           # the smallest launch
    (4, 16, 50, 56, True),         # 16 steps, padded latent rows, the twin
    (3, 5, 50, 50, False),         # N < 16, tight rows
    (300, 1, 1, 1, False),         # the grid sized by B (N B ldz = B): two workgroups
    (257, 16, 65, 72, True),       # B past one workgroup with everything on
]
SCENE_CASES = [dict(B=B, N=N, Z=Z, ldz=ldz, z16=z16, given=g) for (B, N, Z, ldz, z16) in SCENE_SHAPES for g in (0, 1)]
SCENE_DYN = ("TEMPERATURE", "STOP_THRESHOLD", "PRIOR_LOG_ODDS", "SCALE_PM", "SCALE_PV", "SHIFT_PM", "SHIFT_PV", "VAE_PM", "VAE_PV")
ATT_TOL = 5e-5                                   # x max(1, |ref|max): _assert_attend's bound (tests/test_gpu_step_limits.py)
ATT_CLOSE = ("S", "X", "Y", "ZPRE")              # + the three ST_BACK values
ATT_ZERO = (H.ATT_ZPROB, H.ATT_KL_Z, H.ATT_KL_SCALE, H.ATT_KL_SHIFT, H.ATT_KL_VAE, H.ATT_ST_BACK + 3)
S_MARGIN, ROUND_MARGIN = slc.S_MARGIN, slc.ROUND_MARGIN


def scene_stops(B, N):
    """step_limit_cases.STOPS_B4 at any N, repeated over B: alive through all steps, stopping at step 0, (N - 1) // 2, N - 1
    (N = 16: None, 0, 7, 15)"""
    base = (None, 0, (N - 1) // 2, N - 1)
    return tuple(base[b % 4] for b in range(B))


def _phase(stops, N):
    """[N, B]: +1 while an image is alive, 0 at its stopping step, -1 behind it"""
    ph = np.ones((N, len(stops)), np.int64)
    for b, k in enumerate(stops):
        if k is not None:
            ph[k, b], ph[k + 1:, b] = 0, -1
    return ph


def scene_inputs(c):
    """the four sources, fp32, and dyn (NaN but for the nine slots the kernel reads).
    given = 0: eps clipped at +-2.5 (+-3 for the latents); u = sigmoid(T y - prior log-odds) of a PLANNED pre-sigmoid value
    y -- 1.5 .. 5 while the image is alive, -5 .. -1.5 at its stopping step, either side behind it -- so that round() is
    never near its tie.  given = 1: scales, shifts, latents and a RELAXED z_pres: 1 - 1e-5 .. 1 - 5e-4 while alive (the image
    that stops last: 0.96 .. 0.98, a stopping sum of 0.3 .. 0.6 by step 15), 0.002 .. 0.006 at the stopping step, 0.1 .. 0.9
    behind it"""
    B, N, Z, given = c["B"], c["N"], c["Z"], c["given"]
    rng = pec._seed(23, B, N, Z, given)
    stops = scene_stops(B, N)
    ph = _phase(stops, N)
    dyn = pec.dyn_only(B, *(getattr(H, "DYN_" + k) for k in SCENE_DYN))
    if not given:
        mag = rng.uniform(1.5, 5.0, (N, B))
        y = np.where(ph > 0, mag, np.where(ph == 0, -mag, mag * rng.choice([-1.0, 1.0], (N, B))))
        T, plo = np.float64(dyn[H.DYN_TEMPERATURE]), np.float64(dyn[H.DYN_PRIOR_LOG_ODDS])
        src = dict(scale_src=np.clip(rng.standard_normal((N, B)), -2.5, 2.5), shift_src=np.clip(rng.standard_normal((N, B, 2)), -2.5, 2.5),
                   z_src=np.clip(rng.standard_normal((N, B, Z)), -3.0, 3.0), pres_src=1.0 / (1.0 + np.exp(-(y * T - plo))))
    else:
        last = np.array([k is not None and k == N - 1 and N > 1 for k in stops])
        alive = np.where(last[None, :], rng.uniform(0.96, 0.98, (N, B)), 1.0 - rng.uniform(1e-5, 5e-4, (N, B)))
        z = np.where(ph > 0, alive, np.where(ph == 0, rng.uniform(0.002, 0.006, (N, B)), rng.uniform(0.1, 0.9, (N, B))))
        src = dict(scale_src=rng.uniform(0.2, 0.95, (N, B)), shift_src=rng.uniform(-0.8, 0.8, (N, B, 2)),
                   z_src=rng.standard_normal((N, B, Z)), pres_src=z)
    return dict({k: v.astype(np.float32) for k, v in src.items()}, dyn=dyn, stops=stops)


def scene_reference(c, x, t=np.float64):
    """the generation block of include/air_hip.h in type t on the fp32 inputs (t = float64: the reference; float32: the
    kernel's expressions in its order).  att [N, B, 16], z [N, B, ldz] with zero pad columns, and what the margins need:
    S_before / S_after [N, B], z_sigmoid [N, B] (before the round; given = 0)"""
    B, N, Z, ldz, given = c["B"], c["N"], c["Z"], c["ldz"], c["given"]
    d = {k: t(x["dyn"][getattr(H, "DYN_" + k)]) for k in SCENE_DYN}
    sc, sh, zs, pr = (x[k].astype(t) for k in ("scale_src", "shift_src", "z_src", "pres_src"))
    att = np.zeros((N, B, H.ATT_STRIDE), t)
    z = np.zeros((N, B, ldz), t)
    S = np.zeros(B, t)
    S_before, S_after, zsig = np.zeros((N, B), t), np.zeros((N, B), t), np.full((N, B), np.nan, t)
    for k in range(N):
        if given:
            s, px, py, zp, ypre = sc[k], sh[k, :, 0], sh[k, :, 1], pr[k], np.zeros(B, t)
        else:
            s = ao.sigmoid(d["SCALE_PM"] + sc[k] * np.sqrt(d["SCALE_PV"]))
            px, py = (np.tanh(d["SHIFT_PM"] + sh[k, :, i] * np.sqrt(d["SHIFT_PV"])) for i in (0, 1))
            ypre = ao.concrete_binary_pre_sigmoid_sample(np.full(B, d["PRIOR_LOG_ODDS"], t), d["TEMPERATURE"], pr[k])
            zsig[k] = ao.sigmoid(ypre)
            zp = np.round(zsig[k])                                      # tf.round: half to even, as numpy's
        S_before[k] = S
        mask_prev = S < d["STOP_THRESHOLD"]
        S = S + (t(1.0) - zp)
        S_after[k] = S
        mask = S < d["STOP_THRESHOLD"]
        a = att[k]
        a[:, H.ATT_S], a[:, H.ATT_X], a[:, H.ATT_Y], a[:, H.ATT_ZPRE], a[:, H.ATT_Z] = s, px, py, ypre, zp
        a[:, H.ATT_MASK_PREV], a[:, H.ATT_MASK] = mask_prev, mask
        a[:, H.ATT_ST_BACK], a[:, H.ATT_ST_BACK + 1], a[:, H.ATT_ST_BACK + 2] = t(1.0) / s, -px / s, -py / s
        z[k, :, :Z] = zs[k] if given else d["VAE_PM"] + zs[k] * np.sqrt(d["VAE_PV"])
    return dict(att=att, z=z, S_before=S_before, S_after=S_after, z_sigmoid=zsig)


def scene_margins(c, x, ref):
    thr = np.float64(x["dyn"][H.DYN_STOP_THRESHOLD])
    m = dict(S=float(min(np.abs(ref["S_before"] - thr).min(), np.abs(ref["S_after"] - thr).min())))
    if c["given"]:
        p = x["pres_src"].astype(np.float64)
        m["relaxed"] = float(np.minimum(p, 1.0 - p).min())             # > 0: no z_pres is 0 or 1
    else:
        m["round"] = float(np.abs(ref["z_sigmoid"] - 0.5).min())
    return m


def att_close_columns():
    """(name, column) of the record slots compared within ATT_TOL"""
    return [(n, getattr(H, "ATT_" + n)) for n in ATT_CLOSE] + [("ST_BACK%d" % i, H.ATT_ST_BACK + i) for i in range(3)]


def att_ratio(got, ref):
    """largest |got - ref| / (5e-5 max(1, |ref|max)) of one slot"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - ref).max() / (ATT_TOL * max(1.0, float(np.abs(ref).max()))))


# ---- 5. air_render ----------------------------------------------------------------------------------------------------
RENDER_FROM_WRITE = [(C, w) for (C, w, Z) in slc.WRITE_CASES[:5]]          # (50, 28), (51, 28), (64, 32), (65, 32), (33, 7)
# C * C < 1024 (one pass of the 1024-thread pixel walk, most threads idle), 1024 % C != 0 (the j >= C carry), and the
# smallest canvas and window the entry point admits
RENDER_ADDED = [(7, 2), (2, 2), (31, 5)]
RENDER_CASES = RENDER_FROM_WRITE + RENDER_ADDED
RENDER_THREADS = 1024
RENDER_TOL = 2e-5                                # test_write_fwd_sixteen_steps_matches_fp64's bound on the reconstruction
RENDER_READS = (H.ATT_S, H.ATT_X, H.ATT_Y, H.ATT_Z, H.ATT_MASK)


@functools.lru_cache(maxsize=None)
def render_case_and_reference(C, w):
    """({att [16, 3, 16], vrec [16, 3, w w]}, {canvas: the clipped float64 running reconstruction, digits, tap: the tap margin})
    -- built once per process and shared: read-only.  The shapes of slc.WRITE_CASES are its cases; an added one is built the
    same way (section-0 records, windows in (0.02, 0.45)) and drawn again while a tap coordinate of an active step lies
    within WRITE_TAP_MARGIN of a clip edge"""
    if (C, w) in RENDER_FROM_WRITE:
        case, ref = slc.write_case_and_reference(C, w, 50)
        return (dict(C=C, w=w, N=case["N"], B=case["B"], att=case["att"], vrec=case["vrec"]),
                dict(canvas=ref["recon"], digits=ref["run_digits"], tap=ref["tap"]))
    B, N = 3, slc.N_STEPS
    for attempt in range(16):
        att, _ = slc._att_for_write(B, 31 * attempt)
        vrec = pec._seed(24, C, w, attempt).uniform(0.02, 0.45, (N, B, w * w)).astype(np.float32)
        R, taps = slc.running_recon64(att, vrec, C, w, return_taps=True)
        tap = min(min(slc.tap_margin(tx, w), slc.tap_margin(ty, w)) for tx, ty in taps if tx.size)
        if tap >= slc.WRITE_TAP_MARGIN:
            digits = (att[..., H.ATT_MASK] != 0).sum(0).astype(np.int32)
            return dict(C=C, w=w, N=N, B=B, att=att, vrec=vrec), dict(canvas=np.clip(R, 0.0, 1.0), digits=digits, tap=tap)
    raise AssertionError("no draw meets the tap margin: change the builder")


def render_att(att):
    """the records as air_render gets them: NaN in every slot it has no business with"""
    return pec.nan_record(att.shape[:2] + (H.ATT_STRIDE,), {k: att[..., k] for k in RENDER_READS})
