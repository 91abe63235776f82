"""The step prologue (air_step_job_run, csrc/air_philox.h) number for number: alone (air_step_begin), as air_philox_fill, and
carried as extra grid.z planes by every GEMM kernel family (air_gemm_t.step_job; carriers: tests/step_prologue_cases.py,
pinned on the CPU by tests/test_step_prologue_cases.py).

Reference: oracle/philox_ref.py, a numpy restatement of Philox4x32-10 and of the index map of the noise planes.
  * uniforms: bit-identical ((x >> 8) * 2^-24 is exact in fp32);
  * normals: absolute error against float64 Box-Muller on the same words below NORMAL_BOUND (the kernel runs on the hardware
    log / sin / cos; DESIGN.md records the measurement the bound comes from);
  * the bf16 twin: bit-identical to torch's .to(torch.bfloat16) on a source with ties, signed zeros, denormals, infinities and a
    NaN (the NaN's pattern against torch's device conversion: torch's CPU code has two answers for it);
  * schedules: oracle.annealed_value at the bound of test_annealing_schedule_variants_match_oracle; a slot no schedule names
    keeps its sentinel.
Every output carries PAD sentinel elements behind its length, bit-identical afterwards.

A carried job writes what air_step_begin writes with the same arguments, bit for bit, and leaves the product alone: C and every
other output of the launch are bit-identical to the launch without the job wherever air_gemm_kernel_name reports the same
kernel for both, and pass the float64 checks of tests/test_gpu_gemm_edges.py (its runners launch the carriers) either way."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import step_prologue_cases as spc
import test_gpu_gemm_edges as tge
from oracle import air_oracle as ao
from oracle import philox_ref as pr

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64
SENT32 = np.int32(0x7FC5A5A5)                     # a quiet NaN with a payload no arithmetic produces
SENT16 = np.int16(0x7FC5)
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15            # a non-zero high word: key word 1
STEPS = (0, 39000)
# |normal - float64 Box-Muller|: measured 6.67e-7 at worst over the 2 100 003 normals of the largest case (6.30e-7 at step 0,
# 6.67e-7 at step 39000, |x| up to 5.30), x 4 = 2.67e-6, rounded up to one significant digit
NORMAL_BOUND = 3e-6
SIZES = [(0, 5), (5, 0), (1, 1), (4, 4), (7, 9), (2100003, 50001)]       # the last: 537 501 quads > 2048 x 256, the loop wraps
SCHED_DTYPE = [("slot", "<i4"), ("flags", "<i4"), ("init", "<f4"), ("iters", "<f4"), ("factor", "<f4"), ("vmin", "<f4"), ("vmax", "<f4")]


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def schedules(H, count):
    """`count` schedules as (slot, oracle dict): distinct slots, flags = every combination of staircase / min / max / log in turn"""
    slots = [H.DYN_PRIOR_LOG_ODDS, H.DYN_TEMPERATURE, H.DYN_LEARNING_RATE, H.DYN_LIK_STD, H.DYN_VAE_PLV] if count == 5 else \
        [(7 * i + 3) % H.DYN_COUNT for i in range(count)]
    assert len(set(slots)) == count
    out = []
    for i, slot in enumerate(slots):
        flags = (3 * i + 8) % 16 if count == 5 else i                    # (5: log+min.., 11, 14, 1, 4; DYN_COUNT: all sixteen)
        s = dict(init=[10000.0, 1.0, 2.0, 5.0][i % 4], iters=[3000, 1000, 500, 700, 5000][i % 5], factor=[0.1, 0.5, 1.2, 0.9][(i // 2) % 4],
                 staircase=bool(flags & 1), log=bool(flags & 8))
        if flags & 2:
            s["min"] = [1e-9, 0.3][i % 2]
        if flags & 4:
            s["max"] = [40.0, 2.0][i % 2]
        out.append((slot, s))
    return out


def sched_table(H, scheds):
    arr = np.zeros(len(scheds), dtype=SCHED_DTYPE)
    for i, (slot, s) in enumerate(scheds):
        flags = (H.SCHED_STAIRCASE if s["staircase"] else 0) | (H.SCHED_HAS_MIN if "min" in s else 0) | \
                (H.SCHED_HAS_MAX if "max" in s else 0) | (H.SCHED_LOG if s["log"] else 0)
        arr[i] = (slot, flags, s["init"], s["iters"], s["factor"], s.get("min", 0.0), s.get("max", 0.0))
    return torch.from_numpy(arr.view(np.uint8).copy()).to(DEV)


SPECIALS = np.array([0x3F808000, 0x3F818000, 0x80000000, 0x00018000, 0x7F800000, 0x7FC00000, 0xFF800000,      # tie -> even (down), tie -> even (up),
                     0x00000000, 0x00000001, 0x00008000, 0x807FFFFF, 0x007FFFFF, 0x3F808001, 0x3F807FFF,      # -0, denormal tie, inf, NaN, -inf, +0,
                     0xBF808000, 0xBF818000, 0x7F7FFFFF, 0x33800000, 0x00010000], np.uint32)                   # denormals, next to a tie, -ties, max


def twin_source(n):
    """n floats: the special bit patterns first, then uniform (-1, 1); + PAD more behind them (readable, never converted)"""
    rng = np.random.RandomState(3)
    v = rng.uniform(-1, 1, n + PAD).astype(np.float32)
    k = min(n, SPECIALS.size)
    v[:k] = SPECIALS[:k].view(np.float32)
    return v


class Job:
    """the arguments of one prologue and its sentinel-filled outputs"""

    def __init__(self, H, nn, nu, nt, step, scheds, seed=SEED):
        self.H, self.nn, self.nu, self.nt, self.step, self.scheds, self.seed = H, nn, nu, nt, step, scheds, seed
        self.table = sched_table(H, scheds) if scheds else None
        self.ist = torch.tensor([step, 0, 0, 0], dtype=torch.int32, device=DEV)
        self.src_host = twin_source(nt)
        self.src = torch.from_numpy(self.src_host).to(DEV)
        full = lambda n, s, dt: torch.from_numpy(np.full(n + PAD, s, dt)).to(DEV)  # noqa: E731
        self.out = dict(dyn=full(H.DYN_COUNT, SENT32, np.int32), normals=full(nn, SENT32, np.int32), uniforms=full(nu, SENT32, np.int32),
                        twin=full(nt, SENT16, np.int16))
        self.struct = H.StepJob(sched=self.table.data_ptr() if scheds else None, nsched=len(scheds), dyn=self.out["dyn"].data_ptr(),
                                istate=self.ist.data_ptr(), normals=self.out["normals"].data_ptr(), n_normal=nn,
                                uniforms=self.out["uniforms"].data_ptr(), n_uniform=nu, seed=seed,
                                twin_src=self.src.data_ptr() if nt else None, twin_dst=self.out["twin"].data_ptr() if nt else None, twin_n=nt)

    def step_begin(self):
        o = self.out
        return self.H.lib().air_step_begin(_p(self.table), len(self.scheds), _p(o["dyn"]), _p(self.ist), _p(o["normals"]), self.nn,
                                           _p(o["uniforms"]), self.nu, C.c_uint64(self.seed), _p(self.src) if self.nt else None,
                                           _p(o["twin"]) if self.nt else None, self.nt, _stream())

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def check(self, snap, bound=None):
        """sentinels, then every plane against its reference; returns the largest normal error"""
        H = self.H
        sizes = dict(dyn=H.DYN_COUNT, normals=self.nn, uniforms=self.nu, twin=self.nt)
        for k, n in sizes.items():
            sent = SENT16 if k == "twin" else SENT32
            assert (snap[k][n:] == sent).all(), "%s: the %d elements behind its length were written" % (k, PAD)
            if k != "dyn":
                assert not (snap[k][:n] == sent).any(), "%s: %d elements not written" % (k, int((snap[k][:n] == sent).sum()))
        named = {slot for slot, _ in self.scheds}
        for slot in range(H.DYN_COUNT):
            if slot not in named:
                assert snap["dyn"][slot] == SENT32, "dyn[%d] was written and no schedule names it" % slot
        for slot, s in self.scheds:
            got, ref = float(snap["dyn"][slot:slot + 1].view(np.float32)[0]), float(ao.annealed_value(s, self.step))
            assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (slot, s, self.step, got, ref)
        normals, uniforms = pr.step_planes(self.nn, self.nu, self.step, self.seed)
        assert np.array_equal(snap["uniforms"][:self.nu].view(np.float32), uniforms), "uniforms differ from the reference"
        got = snap["normals"][:self.nn].view(np.float32)
        err = float(np.abs(got - normals).max()) if self.nn else 0.0
        assert np.isfinite(got).all()
        if self.nn:
            print("normals: n %d step %d max |x| %.3f, max |error| against float64 %.3e" % (self.nn, self.step, np.abs(normals).max(), err))
        assert err < (NORMAL_BOUND if bound is None else bound), err
        src, got = self.src_host[:self.nt], snap["twin"][:self.nt]
        want = torch.from_numpy(src.copy()).to(torch.bfloat16).view(torch.int16).numpy()
        nan = np.isnan(src)
        assert np.array_equal(got[~nan], want[~nan]), "the twin is not torch's bf16 of its source"
        # torch's own conversions disagree on the bit pattern of a NaN (0x7FC0 from its scalar and device code, 0xFFFF from its
        # vectorised CPU code; IEEE leaves the payload open): on the host a NaN has to stay a NaN, and the whole twin, NaN
        # included, equals torch's conversion on the device bit for bit
        g = got[nan].view(np.uint16)
        assert ((g & 0x7F80) == 0x7F80).all() and ((g & 0x007F) != 0).all(), "a NaN did not stay one"
        dev = self.src[:self.nt].to(torch.bfloat16).view(torch.int16).cpu().numpy()
        assert np.array_equal(got, dev), "the twin is not torch's bf16 (device conversion) of its source"
        return err


# ---- air_step_begin ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nn,nu", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_noise_planes_match_the_reference(H, nn, nu):
    """uniforms bit for bit, normals within NORMAL_BOUND of float64, at both steps; the planes of the two steps differ"""
    snaps = []
    for step in STEPS:
        job = Job(H, nn, nu, 0, step, [])
        H.check(job.step_begin(), "air_step_begin")
        snaps.append(job.snapshot())
        job.check(snaps[-1])
    for k, n in (("normals", nn), ("uniforms", nu)):
        if n:
            assert not np.array_equal(snaps[0][k][:n], snaps[1][k][:n]), k
            # ... in every quad, not merely somewhere (a counter word that ignores the step only in part)
            if n >= 64:
                assert (snaps[0][k][:n] != snaps[1][k][:n]).mean() > 0.99


@pytest.mark.parametrize("nt", [1, 3, 4, 7, 4099])
def test_twin_is_torchs_bf16_with_noise_planes_in_front(H, nt):
    """the twin's quads come behind those of both noise planes: (7, 9) puts them at quad 5"""
    job = Job(H, 7, 9, nt, 39000, [])
    H.check(job.step_begin(), "air_step_begin")
    job.check(job.snapshot())
    # ... and alone
    job = Job(H, 0, 0, nt, 0, [])
    H.check(job.step_begin(), "air_step_begin")
    job.check(job.snapshot())


@pytest.mark.parametrize("count", [5, 16])
def test_schedules_write_their_slots_and_no_other(H, count):
    assert H.DYN_COUNT == 16
    for step in STEPS + (1, 2999, 3000):
        job = Job(H, 4, 4, 0, step, schedules(H, count))
        H.check(job.step_begin(), "air_step_begin")
        job.check(job.snapshot())


def test_more_schedules_than_threads_are_refused(H):
    job = Job(H, 4, 4, 0, 0, schedules(H, 5))
    big = torch.zeros(257 * 28, dtype=torch.uint8, device=DEV)
    o = job.out
    lib = H.lib()
    rc = lib.air_step_begin(_p(big), 257, _p(o["dyn"]), _p(job.ist), _p(o["normals"]), 4, _p(o["uniforms"]), 4, C.c_uint64(SEED), None, None, 0,
                            _stream())
    assert rc == -1
    snap = job.snapshot()
    assert all((v == (SENT16 if k == "twin" else SENT32)).all() for k, v in snap.items())      # nothing ran


@pytest.mark.parametrize("seed,call,nn,nu", [(SEED, 7, 50003, 20001), (0x1234, (3 << 32) | 0xFFFFFFFF, 9, 6)])
def test_philox_fill_matches_the_reference(H, seed, call, nn, nu):
    full = lambda n: torch.from_numpy(np.full(n + PAD, SENT32, np.int32)).to(DEV)  # noqa: E731
    normals, uniforms = full(nn), full(nu)
    H.check(H.lib().air_philox_fill(_p(normals), nn, _p(uniforms), nu, C.c_uint64(seed), C.c_uint64(call), _stream()), "air_philox_fill")
    torch.cuda.synchronize()
    gn, gu = normals.cpu().numpy(), uniforms.cpu().numpy()
    assert (gn[nn:] == SENT32).all() and (gu[nu:] == SENT32).all()
    rn, ru = pr.fill_planes(nn, nu, seed, call)
    assert np.array_equal(gu[:nu].view(np.float32), ru)
    err = np.abs(gn[:nn].view(np.float32) - rn).max()
    print("air_philox_fill: max |error| of the normals against float64 %.3e" % err)
    assert err < NORMAL_BOUND
    # the step prologue's salt is another one: the same (seed, counter) there gives other numbers
    assert not np.array_equal(pr.step_planes(nn, nu, call & 0xffffffff, seed)[1], ru)


# ---- the job carried by a GEMM -----------------------------------------------------------------------------------------------

CARRIED_STEP = 39000


def _job(H, job):
    _, nn, nu, nt = job
    return Job(H, nn, nu, nt, CARRIED_STEP, schedules(H, 5))


@pytest.fixture(scope="module")
def standalone(H):
    """what air_step_begin writes for each job of the table: computed once, checked against the references, never changed"""
    out = {}
    for job in spc.JOBS:
        j = _job(H, job)
        H.check(j.step_begin(), "air_step_begin")
        out[job[0]] = j.snapshot()
        j.check(out[job[0]])
    return out


def _run_fwd0(H, c, rng):
    """the hoisted x.Wx + first LSTM step (AIR_EPI_LSTM_FWD0) on the edge tests' guarded outputs, against float64"""
    M, R, K = c["M"], c["R"], c["K"]
    Kp = (K + 7) & ~7
    X = np.abs(rng.uniform(-1, 1, (M, K))).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, 4 * R)) * 0.05).astype(np.float32)
    bias = (rng.uniform(-1, 1, 4 * R) * 0.1).astype(np.float32)
    Xd, Wd, bd = (torch.from_numpy(v).to(DEV) for v in (X, W, bias))
    keep = [tge._panels(H, (Wd, True))]
    x16 = np.zeros((M, Kp), np.int16)
    x16[:, :K] = tge._twin_of(X)
    keep.append(torch.from_numpy(x16).to(DEV))
    outs = dict(C=tge._Out(M, 4 * R, 4 * R), q0=tge._Out(M, 4 * R, 4 * R), q1=tge._Out(M, R, R), q2=tge._Out(M, R, R),
                q2_16=tge._Out(M, R, R, bits=16))
    if c["C16"]:
        outs["C16"] = tge._Out(M, Kp, Kp, bits=16)
    ptr = dict(A=Xd.data_ptr(), B=Wd.data_ptr(), bias=bd.data_ptr(), B16p=keep[0].data_ptr(), A16=keep[1].data_ptr())
    ptr.update({k: o.ptr for k, o in outs.items()})
    tge._launch(H, spc.descriptor(H, c, ptr))
    tge._sync()
    bad = []
    for k, o in outs.items():
        bad += ["%s: %s" % (k, b) for b in o.check()[0]]
    if bad:
        return bad
    acc = tge._bf16_round(X) @ tge._bf16_round(W)
    pre = acc + bias
    gi, gj, gf, go = tge._sig(pre[:, :R]), np.tanh(pre[:, R:2 * R]), tge._sig(pre[:, 2 * R:3 * R] + 1.0), tge._sig(pre[:, 3 * R:])
    cn = gi * gj                                                          # zero_state: c_0 = 0
    for k, ref in dict(C=acc, q0=np.concatenate([gi, gj, gf, go], axis=1), q1=cn, q2=np.tanh(cn) * go).items():
        tge._compare(bad, "%s[epi 6]" % k, outs[k].body().view(np.float32)[0], ref)
    bad += tge._twin_problems("q2_16", outs["q2_16"], outs["q2"])
    if c["C16"] and not np.array_equal(outs["C16"].body()[0], x16):
        bad.append("C16 is not the zero-padded bf16 twin of the batch")
    return bad


def _runner(c):
    return _run_fwd0 if c["group"] == "fwd0" else tge._run_fused if c["group"] == "fused" else tge._run_plain


def _carry(H, monkeypatch, c, job):
    """launch carrier c through its runner, every launch of it carrying `job` (None: none).  Returns the runner's findings, the
    kernel name of every launch, and every output array of the runner (guards and pads included), in creation order."""
    names, outs = [], []

    class Recorded(tge._Out):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            outs.append(self)

    def launch(H_, g):
        if job is not None:
            g.step_job = C.pointer(job.struct)
        buf = C.create_string_buffer(128)
        H_.check(H_.lib().air_gemm_kernel_name(C.byref(g), buf, 128), "air_gemm_kernel_name")
        names.append(buf.value.decode())
        H_.check(H_.lib().air_gemm(C.byref(g), _stream()), "air_gemm")

    with monkeypatch.context() as mp:
        mp.setattr(tge, "_Out", Recorded)
        mp.setattr(tge, "_launch", launch)
        bad = _runner(c)(H, c, np.random.RandomState(911))
    return bad, names, [o.host() for o in outs]


@pytest.mark.parametrize("c", spc.CARRIERS, ids=[spc.carrier_id(c) for c in spc.CARRIERS])
def test_a_carried_job_equals_step_begin_and_leaves_the_product_alone(H, monkeypatch, standalone, c):
    bad0, names0, outs0 = _carry(H, monkeypatch, c, None)
    assert not bad0, bad0
    assert names0[-1] == c["name"]
    for job in spc.JOBS:
        j = _job(H, job)
        bad, names, outs = _carry(H, monkeypatch, c, j)
        snap = j.snapshot()
        assert names[-1] == c["job_name"], names
        # the job's outputs: air_step_begin's, bit for bit (sentinels included: the snapshots hold the pads)
        for k, want in standalone[job[0]].items():
            diff = np.flatnonzero(snap[k] != want)
            assert diff.size == 0, "%s job on %s: %s differs from air_step_begin at %d elements, first %d" % (
                job[0], c["carrier"], k, diff.size, diff[0])
        # the launch's own outputs: guards intact, written, the float64 reference at the edge tests' bounds ...
        assert not bad, (job[0], bad)
        # ... and bit-identical to the launch without the job, every split-K slab, pad and guard row included
        assert len(outs) == len(outs0) and len(names) == len(names0)
        if names == names0:
            for i, (a, b) in enumerate(zip(outs0, outs)):
                assert np.array_equal(a, b), "%s job on %s: output %d of the launch differs from the launch without a job" % (job[0], c["carrier"], i)
        else:
            assert (c["name"], c["job_name"]) == ("gemm_f32v2_kernel<1, 1, false, 100>", "gemm_f32v2_kernel<1, 4, false, 1>")
