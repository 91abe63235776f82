"""The optimizer launches of a train step -- air_grad_sqnorm, then air_adam_clip_step or air_adam_clip_step_panels -- against
oracle.clip_by_global_norm + oracle.adam_step evaluated in float64 ON THE KERNELS' INPUTS (the fp32 arrays and the fp32 values
of lr, clip, beta1, beta2 and epsilon, widened), at the sizes where the kernels change path:

  n < 4 and n % 4 != 0      the scalar tails of all three kernels (the model's flat buffer never has one)
  n / 4 = 524288 -+ 1       one grid pass of adam_clip_kernel (2048 workgroups x 256 float4) and the first prefetched quad of a
  n / 4 = 2 x 524288        second; two full passes.  grad_sqnorm_kernel (1024 x 256) wraps at all three.

and under the conditions the one-size test of tests/test_gpu_kernels.py never sets: clipping inactive, clipping disabled
(clip = 0), a prescaled gradient, a zero gradient, and the first step (t = 1).

Bounds are that test's: gnorm relative 1e-5; m rtol 1e-5 / atol 1e-9; v rtol 1e-5 / atol 1e-12; p atol 2e-7 with |p| <= 1 and
lr = 1e-2.  The inputs are sized for those bounds by the precision of fp32, not by what the kernels return:
  * m and v enter as moments of one stream, v0 >= m0^2, so that the update of p stays below lr;
  * where the new m = m0 + (g' - m0)(1 - beta1) cancels, rtol buys nothing and atol = 1e-9 has to hold the rounding of g' and of
    g' - m0 (half an ulp each, times 0.1), of the product, and the error of the clip scale (a chain of five fp32 operations,
    <= 3e-7 relative) times 0.1 |g'|.  Half an ulp is 9.3e-10 for |x| < 2^-5: gradients of 0.004 N(0, 1) keep |g'| below 0.025 over
    4.2 M draws and the sum of those terms near 6e-10.  (At 0.05 N(0, 1), the scale of the one-size test, two of 4 194 307
    elements with |g'| = 0.09 and |m| = 1e-5 sat 1.6e-9 off: fp32 itself, at 40 028 elements such a pair does not occur.)
Every array carries 64 sentinel elements behind its length, which must be bit-identical afterwards; two runs are bit-identical."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
from oracle import air_oracle as ao
from test_gpu_kernels import _panel_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64
SENT32 = np.int32(0x7FC5A5A5)                     # a quiet NaN with a payload no arithmetic produces
SENT16 = np.int16(0x7FC5)
ISENT = np.int32(0x5A5A5A5A)
PASS = 524288                                     # float4 per grid pass of adam_clip_kernel: 2048 workgroups x 256 threads
SIZES = [1, 2, 3, 5, 4099, 4 * PASS - 1, 4 * PASS + 5, 4 * (PASS + 2048 * 256) + 3]
NMAX = max(SIZES)
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-2, 0.9, 0.999, 1e-8))      # what the kernels receive, as float64


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


@pytest.fixture(scope="module")
def pool():
    """one stream of inputs for every case (a case takes the first n of each): p in (-0.98, 0.98), g ~ 0.004 N(0, 1),
    m0 ~ 0.01 N(0, 1), v0 = m0^2 + (0.5 .. 1.5) e-4"""
    rng = np.random.RandomState(77)
    f = np.float32
    m0 = (rng.standard_normal(NMAX) * 0.01).astype(f)
    return dict(p=rng.uniform(-0.98, 0.98, NMAX).astype(f), g=(rng.standard_normal(NMAX) * 0.004).astype(f), m=m0,
                v=(m0.astype(np.float64) ** 2 + rng.uniform(0.5e-4, 1.5e-4, NMAX)).astype(f))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(values, sent=SENT32):
    """device copy of a host array with PAD sentinel elements behind it"""
    host = np.full(values.size + PAD, sent, values.dtype if values.dtype.kind == "i" else np.int32)
    host[:values.size] = values.view(host.dtype)
    return torch.from_numpy(host).to(DEV)


def _bf16_bits(x32):
    return torch.from_numpy(np.ascontiguousarray(x32)).to(torch.bfloat16).view(torch.int16).numpy()


class _Run:
    """one air_grad_sqnorm + Adam launch pair on fresh padded buffers; `panels` = (descriptor array, count, panel elements)"""

    def __init__(self, H, n, data, step0, clip, prescale, panels=None):
        lib = H.lib()
        self.n = n
        self.p, self.g, self.m, self.v = (_padded(data[k][:n]) for k in ("p", "g", "m", "v"))
        dyn = np.zeros(H.DYN_COUNT, np.float32)
        dyn[H.DYN_LEARNING_RATE], dyn[H.DYN_CLIP_NORM] = LR, clip
        self.dyn_host = dyn
        self.dyn = _padded(dyn)
        ist = np.full(H.IST_COUNT, ISENT, np.int32)
        ist[H.IST_GLOBAL_STEP] = step0
        self.ist = _padded(ist, ISENT)
        self.npart = lib.air_optim_num_partials(n)
        self.part = _padded(np.zeros(self.npart, np.float32))
        self.gn = _padded(np.zeros(1, np.float32))
        self.sh = _padded(np.full(n, SENT16, np.int16), SENT16)
        self.pan = None
        H.check(lib.air_grad_sqnorm(_p(self.g), n, _p(self.part), _p(self.ist), _stream()), "air_grad_sqnorm")
        if panels is None:
            H.check(lib.air_adam_clip_step(_p(self.p), _p(self.g), _p(self.m), _p(self.v), n, _p(self.part), self.npart, _p(self.dyn),
                                           _p(self.ist), prescale, B1, B2, EPS, _p(self.sh), _p(self.gn), _stream()), "air_adam_clip_step")
        else:
            pans, count, ptotal = panels
            self.pan = _padded(np.full(ptotal, SENT16, np.int16), SENT16)
            H.check(lib.air_adam_clip_step_panels(_p(self.p), _p(self.g), _p(self.m), _p(self.v), n, _p(self.part), self.npart, _p(self.dyn),
                                                  _p(self.ist), prescale, B1, B2, EPS, _p(self.sh), pans, count, _p(self.pan), _p(self.gn),
                                                  _stream()), "air_adam_clip_step_panels")
        torch.cuda.synchronize()
        self.host = {k: getattr(self, k).cpu().numpy() for k in ("p", "g", "m", "v", "dyn", "ist", "part", "gn", "sh")}
        if self.pan is not None:
            self.host["pan"] = self.pan.cpu().numpy()

    def f32(self, k):
        size = {"gn": 1, "part": self.npart}.get(k, self.n)
        return self.host[k][:size].view(np.float32)

    def pads_intact(self, data, step0):
        h, n = self.host, self.n
        for k in ("p", "m", "v", "g"):
            assert (h[k][n:] == SENT32).all(), "the pad behind %s was written" % k
        assert np.array_equal(h["g"][:n].view(np.float32), data["g"][:n])
        assert (h["sh"][n:] == SENT16).all() and (h["gn"][1:] == SENT32).all() and (h["part"][self.npart:] == SENT32).all()
        assert np.array_equal(h["dyn"][:self.dyn_host.size].view(np.float32), self.dyn_host) and (h["dyn"][self.dyn_host.size:] == SENT32).all()
        # apply_gradients(global_step=...): incremented exactly once, by air_grad_sqnorm; nothing else of istate moves
        assert h["ist"][0] == step0 + 1 and (h["ist"][1:] == ISENT).all()
        if "pan" in h:
            assert (h["pan"][-PAD:] == SENT16).all()


def _reference(data, n, step0, clip, prescale):
    """float64: (gnorm, p, m, v) of clip_by_global_norm + ApplyAdam on the prescaled gradient; clip = 0 disables clipping"""
    g = data["g"][:n].astype(np.float64) * float(np.float32(prescale))
    with np.errstate(divide="ignore"):                                   # a zero gradient: 1 / gnorm = inf, min(inf, 1 / clip) is the finite one
        grads, gnorm = ao.clip_by_global_norm({"w": g}, float(np.float32(clip)) if clip > 0 else 1.0)
    if not clip > 0:
        grads = {"w": g}
    pp, mm, vv = ao.adam_step({"w": data["p"][:n].astype(np.float64)}, grads, {"w": data["m"][:n].astype(np.float64)},
                              {"w": data["v"][:n].astype(np.float64)}, step0 + 1, LR, B1, B2, EPS)
    return float(gnorm), pp["w"], mm["w"], vv["w"]


def _small_panels(H, n):
    """descriptors for the size sweep: an exclusive 1 x 4 matrix at the front; from 4099 on also a gate-interleaved 60 x 64 one"""
    mats = [(0, 0, 1, 4, 0, 1)] + ([(128, 16, 60, 64, 4, 0)] if n >= 4099 else [])
    pans = (H.Panel * len(mats))(*[H.Panel(*m) for m in mats])
    return mats, (pans, len(mats), 16 + (3840 if n >= 4099 else 0) + 8)


def _check(H, data, n, step0=4, clip_of_norm=0.37, prescale=1.0, zero_grad=False):
    """one case: the plain kernel twice, the panel kernel once (n >= 4: a described matrix holds at least four elements)"""
    if zero_grad:
        data = dict(data, g=np.zeros(n, np.float32))
    norm = float(np.sqrt((data["g"][:n].astype(np.float64) ** 2).sum())) * prescale
    # clip_of_norm < 1: clipping active; > 1: inactive (gnorm below clip); 0: disabled.  (A zero gradient keeps clip = 1.)
    clip = float(np.float32(clip_of_norm * norm)) if norm > 0 else float(bool(clip_of_norm))
    gnorm, p64, m64, v64 = _reference(data, n, step0, clip, prescale)
    a = _Run(H, n, data, step0, clip, prescale)
    b = _Run(H, n, data, step0, clip, prescale)
    runs = [("plain", a)]
    if n >= 4:
        mats, panels = _small_panels(H, n)
        runs.append(("panels", _Run(H, n, data, step0, clip, prescale, panels)))
    else:
        pans = (H.Panel * 1)(H.Panel(0, 0, 1, 4, 0, 0))                 # no matrix fits in fewer than four elements: refused
        assert H.lib().air_adam_clip_step_panels(_p(a.p), _p(a.g), _p(a.m), _p(a.v), n, _p(a.part), a.npart, _p(a.dyn), _p(a.ist), 1.0,
                                                 B1, B2, EPS, None, pans, 1, _p(a.sh), None, _stream()) == -1
    for k in ("p", "m", "v", "sh", "gn", "part", "ist"):
        assert np.array_equal(a.host[k], b.host[k]), "two runs differ in %s" % k
    for name, r in runs:
        r.pads_intact(data, step0)
        got_gn = float(r.f32("gn")[0])
        err = {"gnorm": abs(got_gn - gnorm) / gnorm if gnorm > 0 else abs(got_gn),
               "m": np.abs(r.f32("m") - m64).max(), "v": np.abs(r.f32("v") - v64).max(), "p": np.abs(r.f32("p") - p64).max()}
        print("n %d %s step %d clip %.3g prescale %g: gnorm %.9g (ref %.9g) errors %s" %
              (n, name, step0 + 1, clip, prescale, got_gn, gnorm, {k: "%.2e" % v for k, v in err.items()}))
        if zero_grad:
            assert got_gn == 0.0
        else:
            assert err["gnorm"] < 1e-5, (name, got_gn, gnorm)
        for k in ("p", "m", "v"):
            assert np.isfinite(r.f32(k)).all(), (name, k)
        np.testing.assert_allclose(r.f32("m"), m64, rtol=1e-5, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(r.f32("v"), v64, rtol=1e-5, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(r.f32("p"), p64, rtol=0, atol=2e-7, err_msg=name)
        assert np.abs(p64).max() <= 1.0
    # the row-major bf16 shadow of the plain call: bf16(p) everywhere, the tail included
    assert np.array_equal(a.host["sh"][:n], _bf16_bits(a.f32("p")))
    if n >= 4:
        r = runs[1][1]
        for k in ("p", "m", "v", "gn"):
            assert np.array_equal(a.host[k], r.host[k]), "the panel kernel differs from the plain one in %s" % k
        keep = np.ones(n, bool)
        for off, doff, K, N, gates, excl in mats:
            ref = _panel_ref(r.f32("p")[off:off + K * N].reshape(K, N), gates)
            sl = r.host["pan"][doff:doff + ref.size]
            w = np.zeros((K, (N + 15) // 16 * 16), bool)
            w[:, :N] = True
            w = w.reshape(-1) if gates else w.reshape(K, -1, 16).transpose(1, 0, 2).reshape(-1)      # the pad columns are never written
            assert np.array_equal(sl[w], ref[w]) and (sl[~w] == SENT16).all(), (K, N)
            if excl:
                keep[off:off + K * N] = False
        flat16 = _bf16_bits(r.f32("p"))
        assert np.array_equal(r.host["sh"][:n][keep], flat16[keep]) and (r.host["sh"][:n][~keep] == SENT16).all()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_across_tails_and_grid_passes(H, pool, n):
    """clipping active (clip = 0.37 gnorm), t = 5"""
    _check(H, pool, n)


SMALL, WRAPS = 4099, 4 * PASS + 5


@pytest.mark.parametrize("n", [SMALL, WRAPS])
@pytest.mark.parametrize("cond", ["gnorm_below_clip", "clip_disabled", "prescale_1_64", "zero_gradient", "first_step"])
def test_conditions(H, pool, cond, n):
    kw = {"gnorm_below_clip": dict(clip_of_norm=3.0), "clip_disabled": dict(clip_of_norm=0.0), "prescale_1_64": dict(prescale=1.0 / 64),
          "zero_gradient": dict(zero_grad=True), "first_step": dict(step0=0)}[cond]
    _check(H, pool, n, **kw)


# ---- panels: chunk ownership of adam_panels_kernel (a workgroup owns 1024 consecutive quads = 4096 variables) ----------------

CHUNK = 4096
# (offset, K, N, gates, exclusive), offsets in variables.  Three small matrices and a fourth inside chunk 0, exclusive and
# shared mixed; one that starts mid-chunk and crosses the borders at 4096 and 8192; one right behind it (no gap) that ENDS on
# the border at 12288 and one that STARTS there; nine more, 16 descriptors in all; then a region no matrix owns.
PANEL_LAYOUT = [(8, 4, 8, 0, 0), (48, 3, 16, 4, 1), (104, 5, 12, 0, 1), (200, 2, 4, 0, 0),
                (2000, 150, 64, 0, 0), (11600, 43, 16, 4, 1), (12288, 8, 32, 4, 0),
                (12560, 1, 4, 0, 1), (12600, 7, 20, 0, 0), (12800, 2, 48, 4, 1), (12900, 16, 16, 0, 0), (13200, 3, 8, 0, 1),
                (13300, 9, 36, 0, 0), (13700, 4, 64, 4, 0), (14000, 6, 4, 0, 1), (14100, 1, 16, 4, 1)]
PANEL_N = 14100 + 16 + 5000 + 3                   # a trailing unowned region (one whole chunk and more), n % 4 == 3


def test_panel_layout_is_what_its_comment_says():
    """(no GPU work: the table itself)"""
    assert len(PANEL_LAYOUT) == 16 and PANEL_N % 4 == 3
    ends = [off + K * N for off, K, N, _, _ in PANEL_LAYOUT]
    assert all(o % 4 == 0 and N % 4 == 0 for o, _, N, _, _ in PANEL_LAYOUT)
    assert all(PANEL_LAYOUT[i + 1][0] >= ends[i] for i in range(15)) and ends[-1] + CHUNK < PANEL_N
    assert sum(1 for e in ends if e <= CHUNK) == 4 and {x[4] for x in PANEL_LAYOUT[:4]} == {0, 1}
    off, end = PANEL_LAYOUT[4][0], ends[4]
    assert off % CHUNK and off // CHUNK == 0 and end // CHUNK == 2 and PANEL_LAYOUT[5][0] == end
    assert ends[5] == 3 * CHUNK == PANEL_LAYOUT[6][0]


def test_panels_across_chunk_borders_with_a_tail(H, pool):
    rng = np.random.RandomState(5)
    n = PANEL_N
    data = {k: pool[k][:n] for k in pool}
    doff, mats = 8, []
    for off, K, N, gates, excl in PANEL_LAYOUT:
        mats.append((off, doff, K, N, 4 if gates else 0, excl))
        doff += (K * N if gates else (N + 15) // 16 * 16 * K) + int(rng.randint(1, 4)) * 8         # a gap behind every panel twin
    pans = (H.Panel * 16)(*[H.Panel(*m) for m in mats])
    norm = float(np.sqrt((data["g"].astype(np.float64) ** 2).sum()))
    clip = float(np.float32(0.37 * norm))
    gnorm, p64, m64, v64 = _reference(data, n, 4, clip, 1.0)
    plain = _Run(H, n, data, 4, clip, 1.0)
    r = _Run(H, n, data, 4, clip, 1.0, (pans, 16, doff))
    plain.pads_intact(data, 4)
    r.pads_intact(data, 4)
    for k in ("p", "m", "v", "gn"):
        assert np.array_equal(plain.host[k], r.host[k]), "the panel kernel differs from the plain one in %s" % k
    assert abs(float(r.f32("gn")[0]) - gnorm) / gnorm < 1e-5
    np.testing.assert_allclose(r.f32("m"), m64, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(r.f32("v"), v64, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(r.f32("p"), p64, rtol=0, atol=2e-7)
    pn, sh, pp = r.host["pan"], r.host["sh"][:n], r.f32("p")
    written = np.zeros(pn.size, bool)
    keep = np.ones(n, bool)
    for off, d, K, N, gates, excl in mats:
        ref = _panel_ref(pp[off:off + K * N].reshape(K, N), gates)
        w = np.zeros((K, (N + 15) // 16 * 16), bool)
        w[:, :N] = True
        w = w.reshape(-1) if gates else w.reshape(K, -1, 16).transpose(1, 0, 2).reshape(-1)
        assert np.array_equal(pn[d:d + ref.size][w], ref[w]), ("panel twin", off, K, N, gates)
        written[d:d + ref.size] = w
        if excl:
            keep[off:off + K * N] = False
    # the sentinel in every gap of the panel buffer (and in the never-written pad columns), and over the exclusive ranges of the
    # row-major shadow; everywhere else -- gaps between matrices, the unowned region, the n % 4 tail -- that shadow is bf16(p)
    assert (pn[~written] == SENT16).all()
    flat16 = _bf16_bits(pp)
    assert (sh[~keep] == SENT16).all() and np.array_equal(sh[keep], flat16[keep])
    assert np.array_equal(plain.host["sh"][:n], flat16)
