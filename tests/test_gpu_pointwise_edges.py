"""The pointwise kernels of csrc/air_pointwise.hip through the C ABI at their shape edges: air_lstm_gates_fwd, air_lstm_first_step,
air_lstm_gates_bwd, air_reparam_fwd, air_reparam_bwd, air_reparam_bwd_plain, air_sigmoid_bwd, air_bce_fwd_bwd and air_finalize
(case tables, inputs and references: tests/pointwise_edge_cases.py, pinned on the CPU by tests/test_pointwise_edge_cases.py;
air_colsum and air_heads_out_wgrad of the same file: tests/test_gpu_wgrad_edges.py).

Every launch runs on poisoned buffers (the helpers of tests/test_gpu_gemm_edges.py).  An input lies between NaN pads, and where
a kernel reads one field of a record every other field is NaN (att[b, AIR_ATT_MASK]; GRAD_SCALE, VAE_PV and VAE_PM of dyn): a
finite result proves that nothing else was read.  An output starts as sentinels between guard bands, which must be
bit-identical afterwards, while every element of the written region must have been written.  No input changes.  Each launch
runs twice, each time on buffers of its own, and the two results are bit-identical.

Values: float64 on the kernel's own fp32 inputs, with the suite's bounds (pointwise_edge_cases.py names the test each comes
from); bit for bit where the operation leaves no freedom -- the first LSTM step against air_lstm_gates_fwd on the numpy fp32
slab sum, the bf16 twin, dgsum, the mean half of air_reparam_bwd_plain, air_sigmoid_bwd, the clipped reconstruction, the
per-item loss and the accuracy.  The inputs of a backward case come from the float64 forward, never from a launch.

Each test collects its failing cases and asserts at the end that there are none, and prints the largest error / bound per
kernel and quantity (recorded in DESIGN.md section 37)."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import pointwise_edge_cases as pec
from test_gpu_gemm_edges import DEV, GUARD, SENT32, _In, _Out

pytestmark = pytest.mark.gpu

PAD = 16                                          # NaN floats in front of and behind every input (64 bytes: alignment is kept)
MAXERR = {}                                       # kernel/quantity -> largest error / bound seen


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _note(key, ratio):
    MAXERR[key] = max(MAXERR.get(key, 0.0), float(ratio))


def _report(failures, prefix):
    print("largest error / bound:", {k: "%.3f" % v for k, v in sorted(MAXERR.items()) if k.startswith(prefix)})
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))


class _Dense(_In):
    """a dense fp32 input between NaN pads, its first value `off` bytes behind a 16-byte boundary; adr: that value's address"""

    def __init__(self, values, off=0):
        v = np.ascontiguousarray(values, np.float32).reshape(1, -1)
        super().__init__(v, v.shape[1] + PAD, 4 * PAD + off)
        self.adr = self.ptr + self.off
        self.before = self.t.cpu().numpy().view(np.int32).copy()

    def changed(self):
        return not np.array_equal(self.t.cpu().numpy().view(np.int32), self.before)


class _Ints:
    """an int32 input between pads of one value (the same for targets and digits: an element read past the end counts as a hit)"""

    def __init__(self, values, pad=-7):
        host = np.full(values.size + 2 * PAD, pad, np.int32)
        host[PAD:PAD + values.size] = values
        self.before = host
        self.t = torch.from_numpy(host).to(DEV)
        self.adr = self.t.data_ptr() + 4 * PAD

    def changed(self):
        return not np.array_equal(self.t.cpu().numpy(), self.before)


class _Flat:
    """n fp32 outputs, the first `off` bytes behind a 16-byte boundary, with GUARD sentinels directly in front and behind (an
    _Out of one row would carry 2 GUARD rows of n: too much for the long case)"""

    def __init__(self, n, off=0):
        self.n, self.e = n, GUARD + off // 4
        self.t = torch.from_numpy(np.full(self.e + n + GUARD, SENT32, np.int32)).to(DEV)
        self.ptr = self.t.data_ptr() + 4 * self.e
        self._host = None

    def host(self):
        if self._host is None:
            self._host = self.t.cpu().numpy()
        return self._host

    def check(self):
        h = self.host()
        body = h[self.e:self.e + self.n]
        bad = []
        if (h[:self.e] != SENT32).any():
            bad.append("the sentinels in front written")
        if (h[self.e + self.n:] != SENT32).any():
            bad.append("the sentinels behind written")
        if (body == SENT32).any():
            bad.append("%d elements not written" % int((body == SENT32).sum()))
        return bad, body.view(np.float32)


def _mat(rows, width, bits=32, init=None):
    return _Out(rows, width, width, bits=bits, init=init)


def _adr(x):
    return None if x is None else (x.adr if hasattr(x, "adr") else x.ptr)


def _twice(launch):
    """launch() -> ({name: output or None}, inputs), every buffer made by that call: run twice; (the first run's outputs, what
    differs between the two runs + whether an input changed)"""
    (a, ina), (b, inb) = launch(), launch()
    torch.cuda.synchronize()
    bad = ["%s: two launches differ in their bits" % k for k in a if a[k] is not None and not np.array_equal(a[k].host(), b[k].host())]
    if any(x is not None and x.changed() for x in list(ina) + list(inb)):
        bad.append("an input was written")
    return a, bad


def _values(bad, name, out, mask=None):
    """the written region [rows, width] of an _Out (fp32, or the int16 of a twin); its guard problems go to bad"""
    problems, vals = out.check(mask)
    bad += ["%s: %s" % (name, p) for p in problems]
    return vals[0, :, :out.width]


def _close(bad, key, got, ref, tol):
    r = pec.ratio(got, ref, tol)
    _note(key, r)
    if not r <= 1.0:
        bad.append("%s: error / bound = %.3g" % (key, r))


def _same_bits(bad, name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32)
    if got.shape != want.shape or not np.array_equal(got, want):
        d = np.flatnonzero(got.ravel() != want.ravel()) if got.shape == want.shape else []
        bad.append("%s: %d elements with other bits%s" % (name, len(d), ", first at %d" % d[0] if len(d) else ""))


def _tagged(c, bad):
    tag = c if isinstance(c, str) else pec.describe(c)
    return ["%s: %s" % (tag, b) for b in bad]


# ---- the LSTM cell ------------------------------------------------------------------------------------------------------
def _gates_fwd(H, pre, c_prev):
    B, R = c_prev.shape

    def launch():
        gin, cin = _Dense(pre), _Dense(c_prev)
        o = dict(acts=_mat(B, 4 * R), c=_mat(B, R), h=_mat(B, R))
        H.check(H.lib().air_lstm_gates_fwd(gin.adr, cin.adr, o["acts"].ptr, o["c"].ptr, o["h"].ptr, B, R, _stream()), "air_lstm_gates_fwd")
        return o, (gin, cin)
    out, bad = _twice(launch)
    return {k: _values(bad, k, v) for k, v in out.items()}, bad


def _against_float64(bad, key, got, pre, c_prev):
    for name, ref in zip(("acts", "c", "h"), pec.lstm_fwd_ref(pre, c_prev)):
        _close(bad, "%s/%s" % (key, name), got[name], ref, pec.LSTM_FWD_TOL)


def test_lstm_gates_fwd_at_block_edges(H):
    """B R = 1, below, at, twice and past 256; R = 1 with 257 rows; odd R: acts, c and h against float64"""
    failures = []
    for B, R in pec.LSTM_FWD_SHAPES:
        x = pec.lstm_fwd_inputs(B, R)
        got, bad = _gates_fwd(H, x["pre"], x["c_prev"])
        _against_float64(bad, "lstm_gates_fwd", got, x["pre"], x["c_prev"])
        failures += _tagged("B=%d R=%d" % (B, R), bad)
    _report(failures, "lstm_gates_fwd")


@pytest.mark.parametrize("B,R", pec.FIRST_STEP_SHAPES)
def test_lstm_first_step_every_slab_count_bias_and_twin(H, B, R):
    """nslabs 1 .. 8 (4: the compile-time body of the train step; the rest: the run-time body) x bias or NULL x h16 or NULL, on
    exactly nslabs slabs.  (a) acts, c and h have the bits of air_lstm_gates_fwd on c_prev = 0 and the numpy fp32 sum
    ((0 + s0) + s1) ... + bias; (b) they agree with float64 of that pre-activation; (c) h16 is bf16(RNE) of the h that was
    written, and without h16 no other bit changes"""
    failures, zero = [], np.zeros((B, R), np.float32)
    with_twin = {}
    for c in (c for c in pec.FIRST_STEP_CASES if (c["B"], c["R"]) == (B, R)):
        x = pec.first_step_inputs(c)
        n = c["nslabs"]
        assert x["slabs"].shape == (n, B, 4 * R)

        def launch():
            sin, bin_ = _Dense(x["slabs"]), (_Dense(x["bias"]) if c["bias"] else None)
            o = dict(acts=_mat(B, 4 * R), c=_mat(B, R), h=_mat(B, R), h16=_mat(B, R, bits=16) if c["h16"] else None)
            H.check(H.lib().air_lstm_first_step(sin.adr, n, _adr(bin_), o["acts"].ptr, o["c"].ptr, o["h"].ptr, _adr(o["h16"]), B, R,
                                                _stream()), "air_lstm_first_step")
            return o, (sin, bin_)
        out, bad = _twice(launch)
        got = {k: _values(bad, k, out[k]) for k in ("acts", "c", "h")}
        pre = pec.first_step_pre(x["slabs"], x["bias"] if c["bias"] else None)
        if c["h16"]:
            unfused, ubad = _gates_fwd(H, pre, zero)
            bad += ["air_lstm_gates_fwd on the fp32 slab sum: " + b for b in ubad]
            with_twin[n, c["bias"]] = (got, unfused)
            _same_bits(bad, "h16 against bf16 of the written h", _values(bad, "h16", out["h16"]), pec.bf16_bits(got["h"]))
        else:
            twin_got, unfused = with_twin[n, c["bias"]]
            for k in got:
                _same_bits(bad, k + " without h16 against the launch with it", got[k], twin_got[k])
        for k in got:
            _same_bits(bad, k + " against air_lstm_gates_fwd on the fp32 slab sum", got[k], unfused[k])
        _against_float64(bad, "lstm_first_step", got, pre, zero)
        failures += _tagged(c, bad)
    _report(failures, "lstm_first_step")


def test_lstm_gates_bwd_every_optional_argument(H):
    """dc_in given or NULL x dgsum absent, stored or accumulated onto random values: dgates and dc_prev against float64; a stored
    dgsum has the bits of dgates, an accumulated one those of fp32(initial + dgates)"""
    failures = []
    for c in pec.LSTM_BWD_CASES:
        B, R = c["B"], c["R"]
        x = pec.lstm_bwd_inputs(B, R)

        def launch():
            ins = {k: _Dense(x[k]) for k in ("dh", "acts", "c_prev", "c")}
            dcin = _Dense(x["dc_in"]) if c["dc_in"] else None
            o = dict(dgates=_mat(B, 4 * R), dc_prev=_mat(B, R), dgsum=None)
            if c["dgsum"] != "absent":
                o["dgsum"] = _mat(B, 4 * R, init=x["dgsum0"] if c["dgsum"] == "accumulated" else None)
            H.check(H.lib().air_lstm_gates_bwd(ins["dh"].adr, _adr(dcin), ins["acts"].adr, ins["c_prev"].adr, ins["c"].adr, o["dgates"].ptr,
                                               o["dc_prev"].ptr, _adr(o["dgsum"]), int(c["dgsum"] == "accumulated"), B, R, _stream()),
                    "air_lstm_gates_bwd")
            return o, [dcin] + list(ins.values())
        out, bad = _twice(launch)
        dgates, dc_prev = _values(bad, "dgates", out["dgates"]), _values(bad, "dc_prev", out["dc_prev"])
        ref_g, ref_c = pec.lstm_bwd_ref(x, c["dc_in"])
        _close(bad, "lstm_gates_bwd/dgates", dgates, ref_g, pec.LSTM_BWD_TOL)
        _close(bad, "lstm_gates_bwd/dc_prev", dc_prev, ref_c, pec.LSTM_BWD_TOL)
        if c["dgsum"] == "stored":
            _same_bits(bad, "dgsum against dgates", _values(bad, "dgsum", out["dgsum"]), dgates)
        elif c["dgsum"] == "accumulated":
            _same_bits(bad, "dgsum against fp32(initial + dgates)", _values(bad, "dgsum", out["dgsum"]), x["dgsum0"] + dgates)
        failures += _tagged(c, bad)
    _report(failures, "lstm_gates_bwd")


# ---- re-parameterisation ------------------------------------------------------------------------------------------------
def test_reparam_fwd_and_bwd_at_block_edges(H):
    """Z = 1, even, odd and 257; B Z at 256 and past it; mask rows 0 and 1; att and dyn NaN but for the mask and the three
    scalars: the sample, the mean leg d + klg (mean - pm) / pv and the log-variance leg d eps sd / 2 + klg (var / pv - 1) / 2
    against float64; a row with mask 0 gives exactly d on the mean leg"""
    failures = []
    for B, Z in pec.REPARAM_SHAPES:
        x = pec.reparam_inputs(B, Z)

        def fwd():
            ins = {k: _Dense(x[k]) for k in ("ml", "eps")}
            o = dict(zs=_mat(B, Z))
            H.check(H.lib().air_reparam_fwd(ins["ml"].adr, ins["eps"].adr, o["zs"].ptr, B, Z, _stream()), "air_reparam_fwd")
            return o, ins.values()

        def bwd():
            ins = {k: _Dense(x[k]) for k in ("ml", "eps", "d_zs", "att", "dyn")}
            o = dict(d_ml=_mat(B, 2 * Z))
            H.check(H.lib().air_reparam_bwd(ins["d_zs"].adr, ins["ml"].adr, ins["eps"].adr, ins["att"].adr, ins["dyn"].adr, o["d_ml"].ptr,
                                            B, Z, _stream()), "air_reparam_bwd")
            return o, ins.values()
        (of, bad), (ob, bad_b) = _twice(fwd), _twice(bwd)
        bad += bad_b
        _close(bad, "reparam_fwd/zs", _values(bad, "zs", of["zs"]), pec.reparam_fwd_ref(x), pec.REPARAM_FWD_TOL)
        d_ml, ref = _values(bad, "d_ml", ob["d_ml"]), pec.reparam_bwd_ref(x)
        _close(bad, "reparam_bwd/d_mean", d_ml[:, :Z], ref[:, :Z], pec.REPARAM_BWD_TOL)
        _close(bad, "reparam_bwd/d_log_var", d_ml[:, Z:], ref[:, Z:], pec.REPARAM_BWD_TOL)
        off = x["mask"] == 0
        _same_bits(bad, "mean leg of the rows with mask 0 against d_zs", d_ml[off][:, :Z], x["d_zs"][off])
        failures += _tagged("B=%d Z=%d" % (B, Z), bad)
    _report(failures, "reparam_")


def test_reparam_bwd_plain_nullable_inputs_and_second_grid_pass(H):
    """d_mean_in and d_lv_in given or NULL, up to 2049 x 256 elements (256 past one pass of the capped grid): the mean half is
    one fp32 addition or a copy, bit for bit; the log-variance half against float64"""
    failures = []
    for M, Z in pec.PLAIN_SHAPES:
        x = pec.plain_inputs(M, Z)
        for c in (c for c in pec.PLAIN_CASES if (c["M"], c["Z"]) == (M, Z)):
            def launch():
                ins = {k: _Dense(x[k]) for k in ("d_zs", "ml", "eps")}
                dm, dl = (_Dense(x["d_mean_in"]) if c["d_mean_in"] else None), (_Dense(x["d_lv_in"]) if c["d_lv_in"] else None)
                o = dict(d_ml=_mat(M, 2 * Z))
                H.check(H.lib().air_reparam_bwd_plain(ins["d_zs"].adr, ins["ml"].adr, ins["eps"].adr, _adr(dm), _adr(dl), o["d_ml"].ptr,
                                                      M, Z, _stream()), "air_reparam_bwd_plain")
                return o, [dm, dl] + list(ins.values())
            out, bad = _twice(launch)
            d_ml = _values(bad, "d_ml", out["d_ml"])
            _same_bits(bad, "mean half", d_ml[:, :Z], pec.plain_mean_bits(x, c["d_mean_in"]))
            _close(bad, "reparam_bwd_plain/d_log_var", d_ml[:, Z:], pec.plain_lv_ref(x, c["d_lv_in"]), pec.REPARAM_BWD_TOL)
            failures += _tagged(c, bad)
    _report(failures, "reparam_bwd_plain")


# ---- SigmoidGrad --------------------------------------------------------------------------------------------------------
def test_sigmoid_bwd_vector_body_scalar_body_and_tails(H):
    """n = 1, 3, 4, 5, 1027 and 4 x 524288 + 7 (a second grid pass of the 16-byte body, then a scalar tail), all arrays 16-byte
    aligned and each in turn 4 bytes off (the scalar body): (g r) (1 - r) bit for bit, sentinels directly around d_pre"""
    failures = []
    for n in pec.SIGMOID_N:
        x = pec.sigmoid_inputs(n)
        want = pec.sigmoid_bwd_bits(x)
        for c in (c for c in pec.SIGMOID_CASES if c["n"] == n):
            og, orr, oo = c["off"]

            def launch():
                gin, rin = _Dense(x["g"], og), _Dense(x["r"], orr)
                o = dict(d_pre=_Flat(n, oo))
                assert gin.adr % 16 == og and rin.adr % 16 == orr and o["d_pre"].ptr % 16 == oo
                H.check(H.lib().air_sigmoid_bwd(gin.adr, rin.adr, o["d_pre"].ptr, n, _stream()), "air_sigmoid_bwd")
                return o, (gin, rin)
            out, bad = _twice(launch)
            problems, got = out["d_pre"].check()
            bad += problems
            _same_bits(bad, "d_pre", got, want)
            failures += _tagged(c, bad)
    _report(failures, "sigmoid_bwd")


# ---- Bernoulli cross-entropy and the batch means ------------------------------------------------------------------------
def test_bce_fwd_bwd_at_row_edges_with_and_without_gradient(H):
    """D = 1, 255, 256, 257 and 2500 (one workgroup per image, 256 threads striding over D), d_recon given or NULL, the ties and
    just-outside values of test_bce_fwd_bwd_matches_oracle_formula, dyn NaN but for GRAD_SCALE: recon has the bits of numpy's
    clip up to the sign of a zero (R = -0.0 is one of the ties: the device's fmaxf gives +0, numpy keeps -0, C allows both),
    loss and gradient that test's bounds; without d_recon, recon and rec_loss keep their bits"""
    failures = []
    with_grad = {}
    for c in pec.BCE_CASES:
        B, D = c["B"], c["D"]
        x = pec.bce_inputs(B, D)

        def launch():
            ins = {k: _Dense(x[k]) for k in ("x", "R", "dyn")}
            o = dict(recon=_mat(B, D), rec_loss=_mat(1, B), d_recon=_mat(B, D) if c["d_recon"] else None)
            H.check(H.lib().air_bce_fwd_bwd(ins["x"].adr, ins["R"].adr, ins["dyn"].adr, o["recon"].ptr, o["rec_loss"].ptr, _adr(o["d_recon"]),
                                            B, D, _stream()), "air_bce_fwd_bwd")
            return o, ins.values()
        out, bad = _twice(launch)
        recon, loss = _values(bad, "recon", out["recon"]), _values(bad, "rec_loss", out["rec_loss"])[0]
        ref_loss, ref_g = pec.bce_ref(x)
        # (+ 0: fmaxf(-0, +0) may return either zero, and the device returns +0 where numpy keeps the -0 of the ties)
        _same_bits(bad, "recon against numpy's clip", recon + np.float32(0.0), pec.bce_recon_bits(x) + np.float32(0.0))
        nz = ref_loss != 0                                                  # (a lone pixel at a tie: the reference is exactly 0)
        if nz.any():
            _close(bad, "bce_fwd_bwd/rec_loss", loss[nz], ref_loss[nz], pec.BCE_LOSS_TOL)
        if (loss[~nz] != 0).any():
            bad.append("rec_loss is not 0 where the reference is")
        if c["d_recon"]:
            _close(bad, "bce_fwd_bwd/d_recon", _values(bad, "d_recon", out["d_recon"]), ref_g, pec.BCE_GRAD_TOL)
            with_grad[B, D] = (recon, loss)
        else:
            _same_bits(bad, "recon without d_recon against the launch with it", recon, with_grad[B, D][0])
            _same_bits(bad, "rec_loss without d_recon against the launch with it", loss, with_grad[B, D][1])
        failures += _tagged(c, bad)
    _report(failures, "bce_fwd_bwd")


def test_finalize_means_on_both_sides_of_one_pass(H):
    """B = 1, 2, 255, 256, 257, 1000 (one workgroup: up to four items per thread); every target its digit, none, k of them for a
    k that does not divide B: loss_per_item has the bits of the fp32 sum, the accuracy is fp32(k) / fp32(B) exactly, the mean
    loss lies within (ceil(B / 256) + 11) 2^-24 of the float64 mean (pointwise_edge_cases.mean_bound), entries 2 and 3 of
    the four-float scalars keep their sentinel"""
    failures = []
    for c in pec.finalize_cases():
        B, k = c["B"], c["k"]
        x = pec.finalize_inputs(c)

        def launch():
            fin = [_Dense(x["run_loss"]), _Dense(x["rec_loss"]), _Ints(x["targets"]), _Ints(x["digits"])]
            o = dict(item=_mat(1, B), scalars=_mat(1, 4))
            H.check(H.lib().air_finalize(fin[0].adr, fin[1].adr, fin[2].adr, fin[3].adr, o["item"].ptr, o["scalars"].ptr, B, _stream()),
                    "air_finalize")
            return o, fin
        out, bad = _twice(launch)
        _same_bits(bad, "loss_per_item", _values(bad, "loss_per_item", out["item"])[0], x["run_loss"] + x["rec_loss"])
        sc = _values(bad, "scalars", out["scalars"], out["scalars"].mask(width=2))[0]
        _same_bits(bad, "accuracy against fp32(k) / fp32(B)", sc[1:2], np.array([np.float32(k) / np.float32(B)], np.float32))
        ref = pec.finalize_ref(x)
        r = abs(float(sc[0]) - ref) / pec.mean_bound(B, ref) if np.isfinite(sc[0]) else np.inf
        _note("finalize/mean loss", r)
        if not r <= 1.0:
            bad.append("mean loss %.9g, float64 %.9g: error / bound = %.3g" % (sc[0], ref, r))
        failures += _tagged(c, bad)
    _report(failures, "finalize")
