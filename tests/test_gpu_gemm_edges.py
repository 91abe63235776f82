"""air_gemm at tile edges, with padded leading dimensions, offset base pointers and guard bands, for every kernel family the
dispatch reaches (case tables: tests/gemm_edge_cases.py; which kernel each case launches is pinned on the CPU by
tests/test_gemm_edge_cases.py).

Every launch runs on poisoned buffers: the pad columns of A, B, addend and aux hold NaN (the ABI defines op(A)(m, k) for k < K
only: a kernel that reads a pad into its result shows a NaN); the pads of every output, BM-and-more guard rows around it and the
split-K slabs beyond air_gemm_slabs() hold a NaN-payload sentinel that must be bit-identical afterwards, while every element of
the written region must have been written (no sentinel left) and match the float64 reference.

Tolerances are the suite's own: plain products |got - ref|.max() / sqrt(K) < 2e-6 (exact fp32) / 2e-5 (bf16 operands, rounded
first in the reference), operands uniform in (-1, 1) (test_gemm_plain); generic epilogues 1e-5 / 2e-4 absolute with B / 8
(test_gemm_epilogues); fused epilogues 2e-5 absolute with weights x 0.1 and slabs x 0.3 against a float64 restatement of the
formulas of include/air_hip.h (test_gemm_fused_lstm_and_reparam_match_unfused).  Twin launches are bit-identical to the
fp32-operand launch of the same descriptor, and every bf16 twin a launch writes equals bf16(RNE) of its fp32 array bit for bit.

Each test collects its failing cases and asserts at the end that there are none: one bad shape does not hide the others."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import gemm_edge_cases as gec
from test_gpu_kernels import _bf16_round, _ref_gemm

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT32 = np.int32(0x7FC5A5A5)                     # a quiet NaN with a payload no arithmetic produces
SENT16 = np.int16(0x7FC5)                         # the same as bf16
GUARD = 64                                        # rows before and after every output: BM of the largest tile
MAXERR = {}                                       # group -> largest error / tolerance seen (printed per test, recorded in DESIGN.md)


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(H, g):
    H.check(H.lib().air_gemm(C.byref(g), _stream()), "air_gemm")


def _sync():
    torch.cuda.synchronize()


class _In:
    """an input matrix [rows, width] stored with leading dimension ld behind `off` bytes of NaN: every pad element is NaN"""

    def __init__(self, values, ld, off=0):
        rows, width = values.shape
        e = off // 4
        host = np.full(e + rows * ld, np.nan, np.float32)
        host[e:].reshape(rows, ld)[:, :width] = values
        self.values, self.ld, self.off = values, ld, off
        self.t = torch.from_numpy(host).to(DEV)
        self.ptr = self.t.data_ptr()              # + a_off / b_off is added by gec.descriptor

    def twin(self):
        """bf16 twin of the whole padded array (RNE, what air_bf16_twin writes): the pads stay NaN"""
        return self.t.to(torch.bfloat16).view(torch.int16)


class _Out:
    """an output of `slabs` x [rows, width] with leading dimension ld between GUARD rows, all sentinel; init: values of the
    written region before the launch (accumulating epilogues)"""

    def __init__(self, rows, width, ld, bits=32, slabs=1, init=None):
        self.rows, self.width, self.ld, self.slabs, self.bits = rows, width, ld, slabs, bits
        self.sent = SENT32 if bits == 32 else SENT16
        host = np.full((2 * GUARD + slabs * rows, ld), self.sent, np.int32 if bits == 32 else np.int16)
        if init is not None:
            host[GUARD:GUARD + rows, :width] = init.astype(np.float32).view(np.int32)
        self.t = torch.from_numpy(host).to(DEV)
        self.ptr = self.t.data_ptr() + GUARD * ld * (bits // 8)
        self._host = None

    def host(self):
        if self._host is None:
            self._host = self.t.cpu().numpy()
        return self._host

    def body(self):
        """[slabs, rows, ld] as stored (int32 / int16)"""
        return self.host()[GUARD:GUARD + self.slabs * self.rows].reshape(self.slabs, self.rows, self.ld)

    def mask(self, rows=None, width=None, slabs=None):
        m = np.zeros((self.slabs, self.rows, self.ld), bool)
        m[:self.slabs if slabs is None else slabs, :self.rows if rows is None else rows, :self.width if width is None else width] = True
        return m

    def check(self, mask=None):
        """(problems, values): guards, pads and unwritten slabs bit-identical to the sentinel; the written region fully written"""
        mask = self.mask() if mask is None else mask
        h, b = self.host(), self.body()
        bad = []
        if (h[:GUARD] != self.sent).any() or (h[GUARD + self.slabs * self.rows:] != self.sent).any():
            bad.append("guard rows written")
        if (b[~mask] != self.sent).any():
            bad.append("%d pad / unwritten-slab elements written" % int((b[~mask] != self.sent).sum()))
        if (b[mask] == self.sent).any():
            bad.append("%d elements of the written region not written" % int((b[mask] == self.sent).sum()))
        return bad, (b.view(np.float32) if self.bits == 32 else b)


def _twin_of(values32):
    """bf16(RNE) bit patterns of an fp32 array"""
    return torch.from_numpy(np.ascontiguousarray(values32)).to(torch.bfloat16).view(torch.int16).numpy()


def _twin_problems(name, out16, out32, mask=None):
    bad, b16 = out16.check(mask)
    mask = out16.mask() if mask is None else mask
    v32 = out32.body().view(np.float32)
    if not bad and not np.array_equal(b16[mask], _twin_of(v32)[mask]):
        bad.append("is not bf16 of its fp32 array")
    return ["%s: %s" % (name, b) for b in bad]


def _panels(H, B):
    """panel-blocked twin of a dense device matrix [K, N] through the ABI (air_panel_shadow); gates: the LSTM's interleaved form"""
    def build(W, gates):
        K, N = W.shape
        size = K * N if gates else (N + 15) // 16 * 16 * K
        out = torch.zeros(size, dtype=torch.int16, device=DEV)
        pd = (H.Panel * 1)(H.Panel(0, 0, K, N, 4 if gates else 0, 0))
        H.check(H.lib().air_panel_shadow(C.c_void_p(W.data_ptr()), C.c_void_p(out.data_ptr()), pd, 1, _stream()))
        return out
    return build(*B)


def _operands(c, rng, b_scale=1.0):
    M, N, K = c["M"], c["N"], c["K"]
    A = rng.uniform(-1, 1, (K, M) if c["ta"] else (M, K)).astype(np.float32)
    B = (rng.uniform(-1, 1, (N, K) if c["tb"] else (K, N)) * b_scale).astype(np.float32)
    return A, B, _In(A, c["lda"], c["a_off"]), _In(B, c["ldb"], c["b_off"])


def _twin_ptrs(H, c, Ain, Bin, keep, gates=False):
    """pointers of the twins a case passes (kept alive in `keep`)"""
    ptr = {}
    if c["A16"]:
        keep.append(Ain.twin())
        ptr["A16"] = keep[-1].data_ptr()
    if c["B16"]:
        keep.append(Bin.twin())
        ptr["B16"] = keep[-1].data_ptr()
    if c["B16p"]:
        keep.append(_panels(H, (torch.from_numpy(Bin.values).to(DEV), gates)))
        ptr["B16p"] = keep[-1].data_ptr()
    return ptr


def _note(group, err, tol):
    MAXERR[group] = max(MAXERR.get(group, 0.0), float(err) / tol)


def _forms(c):
    """the launches of a case: the descriptor itself, and for a twin case also the fp32-operand launch it must match bit for bit"""
    return [c] if c["family"] != "bf16tw" else [dict(c, A16=False, B16=False, B16p=False), c]


# ------------------------------------------------------------------------------------------------ plain products, split-K

def _run_plain(H, c, rng):
    """a plain product or split-K slabs of one; returns the problems found"""
    M, N, K = c["M"], c["N"], c["K"]
    A, B, Ain, Bin = _operands(c, rng)
    slabs = c["ksplit"] if c["ksplit"] > 1 else 1
    written = H.lib().air_gemm_slabs(K, c["ksplit"]) if c["ksplit"] > 1 else 1
    outs, keep = [], []
    for form in _forms(c):
        Cout = _Out(M, N, c["ldc"], slabs=slabs)
        ptr = dict(A=Ain.ptr, B=Bin.ptr, C=Cout.ptr)
        ptr.update(_twin_ptrs(H, form, Ain, Bin, keep))
        _launch(H, gec.descriptor(H, form, ptr))
        outs.append(Cout)
    _sync()
    bad = []
    for Cout in outs:
        pb, vals = Cout.check(Cout.mask(slabs=written))
        bad += pb
    got = outs[-1].body().view(np.float32)[:written, :, :N]
    if not bad:
        if np.isnan(got).any():
            bad.append("NaN in the result: a pad was read")
        else:
            ref = _ref_gemm(A, B, c["ta"], c["tb"], c["prec"])
            tol = 2e-5 if c["prec"] else 2e-6
            err = np.abs(got.astype(np.float64).sum(0) - ref).max() / np.sqrt(K)
            _note(c["group"] + "/" + c["family"], err, tol)
            if not err < tol:
                bad.append("error / sqrt(K) = %.3g (bound %.0e)" % (err, tol))
        if len(outs) == 2 and not np.array_equal(outs[0].body()[:written, :, :N], outs[1].body()[:written, :, :N]):
            bad.append("twin launch differs from the fp32-operand launch")
    return bad


def _run_cases(H, cases, run, seed):
    failures = []
    for i, c in enumerate(cases):
        for b in run(H, c, np.random.RandomState(seed + i)):
            failures.append("%s: %s" % (gec.describe(c), b))
    return failures


def _report(failures, group_prefix):
    worst = {k: v for k, v in MAXERR.items() if k.startswith(group_prefix)}
    print("largest error / bound so far:", {k: "%.3f" % v for k, v in sorted(worst.items())})
    assert not failures, "%d failing cases:\n%s" % (len(failures), "\n".join(failures[:40]))


PLAIN = gec.plain_groups()


@pytest.mark.parametrize("cases", [g[1] for g in PLAIN], ids=[g[0] for g in PLAIN])
def test_plain_products_at_tile_edges(H, cases):
    """M = 1, BM -+ 1, N = BN -+ 2, K from below one MFMA depth to a round boundary -+ one piece, all four alignment arms of the
    lean K loop, each way into the fallback kernels, the twin kernels with row-major and panel B twins: one (family, tile, layout)"""
    _report(_run_cases(H, cases, _run_plain, 1000), "plain")


def test_split_k_slabs_short_counts_and_short_last_slab(H):
    """ksplit slabs are allocated; only air_gemm_slabs() of them may be written, and their float64 sum is the product"""
    _report(_run_cases(H, gec.splitk_cases(), _run_plain, 2000), "splitk")


# ------------------------------------------------------------------------------------------------ generic epilogues

def _run_epilogue(H, c, rng):
    M, N, K = c["M"], c["N"], c["K"]
    kw = gec.EPI_KW[c["kw"]]
    A, B, Ain, Bin = _operands(c, rng, 1.0 / 8)
    bias = rng.uniform(-1, 1, N).astype(np.float32) if kw.get("bias") else None
    nadd = kw.get("addend", 0)
    addend = rng.uniform(-1, 1, (nadd, M, N)).astype(np.float32) if nadd else None
    aux = None
    if kw.get("aux"):
        aux = rng.uniform(0.01, 2, (M, N)).astype(np.float32) - (1.0 if kw["aux"] == "signed" else 0.0)
        aux = aux.astype(np.float32)
    c0 = rng.uniform(-1, 1, (M, N)).astype(np.float32) if kw.get("accumulate") else None
    keep, outs = [], []
    ptr0 = dict(A=Ain.ptr, B=Bin.ptr)
    if bias is not None:
        keep.append(torch.from_numpy(bias).to(DEV))
        ptr0["bias"] = keep[-1].data_ptr()
    if addend is not None:
        keep.append(_In(addend.reshape(nadd * M, N), c["ldadd"]))            # slab stride = M * ldadd
        ptr0["addend"] = keep[-1].ptr
    if aux is not None:
        keep.append(_In(aux, c["ldaux"]))
        ptr0["aux"] = keep[-1].ptr
    for form in _forms(c):
        Cout = _Out(M, N, c["ldc"], init=c0)
        C16 = _Out(M, N, c["ldc"], bits=16) if kw.get("C16") else None
        ptr = dict(ptr0, C=Cout.ptr)
        if C16 is not None:
            ptr["C16"] = C16.ptr
        ptr.update(_twin_ptrs(H, form, Ain, Bin, keep))
        _launch(H, gec.descriptor(H, form, ptr))
        outs.append((Cout, C16))
    _sync()
    bad = []
    for Cout, C16 in outs:
        bad += Cout.check()[0]
        if C16 is not None:
            bad += _twin_problems("C16", C16, Cout)
    got = outs[-1][0].body().view(np.float32)[0, :, :N]
    if not bad:
        if np.isnan(got).any():
            bad.append("NaN in the result: a pad was read")
        else:
            ref = _ref_gemm(A, B, c["ta"], c["tb"], c["prec"], bias=bias, addend=None if addend is None else addend.astype(np.float64).sum(0),
                            aux=aux, act=kw.get("act", 0), actgrad=kw.get("actgrad", 0), aux_scale=kw.get("aux_scale", 0.0),
                            accumulate=kw.get("accumulate", 0), c_init=c0)
            tol = 2e-4 if c["prec"] else 1e-5
            err = np.abs(got - ref).max()
            _note("epi/" + c["family"], err, tol)
            if not err < tol:
                bad.append("error %.3g (bound %.0e)" % (err, tol))
        if len(outs) == 2 and not np.array_equal(outs[0][0].body()[0, :, :N], outs[1][0].body()[0, :, :N]):
            bad.append("twin launch differs from the fp32-operand launch")
    return bad


@pytest.mark.parametrize("tile", gec.EPI_TILES, ids=lambda t: "%dx%d" % t)
def test_generic_epilogues_with_padded_addend_and_aux(H, tile):
    """every keyword set of test_gemm_epilogues + 2 and 8 addend slabs + a C16 twin, at the base shape of each family and layout:
    bias / addend / aux are indexed with n, ldadd and ldaux -- none of which equals ldc or N here"""
    cases = [c for c in gec.epilogue_cases() if tuple(c["tile"]) == tile]
    _report(_run_cases(H, cases, _run_epilogue, 3000), "epi")


# ------------------------------------------------------------------------------------------------ fused epilogues

def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _product64(A, B, c):
    """float64 acc of the case: operands rounded to bf16 first at precision 1"""
    A64 = _bf16_round(A) if c["prec"] else A.astype(np.float64)
    B64 = _bf16_round(B) if c["prec"] else B.astype(np.float64)
    return A64 @ (B64.T if c["tb"] else B64)


def _dense_in(keep, values):
    keep.append(torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(DEV))
    return keep[-1].data_ptr()


def _cell_backward64(dh, acts, c_prev, c_new, dc_in, R):
    """LSTM cell backward of air_gemm_common.h in float64: (dgates [M, 4R], dc_prev [M, R])"""
    si, tj, sf, so = (acts[:, j * R:(j + 1) * R].astype(np.float64) for j in range(4))
    tc = np.tanh(c_new.astype(np.float64))
    dc = (0.0 if dc_in is None else dc_in.astype(np.float64)) + dh * so * (1.0 - tc * tc)
    dg = np.concatenate([dc * tj * si * (1.0 - si), dc * si * (1.0 - tj * tj), dc * c_prev.astype(np.float64) * sf * (1.0 - sf),
                         dh * tc * so * (1.0 - so)], axis=1)
    return dg, dc * sf


def _cell_inputs(rng, rows, R):
    acts = np.concatenate([rng.uniform(0.05, 0.95, (rows, R)), rng.uniform(-0.9, 0.9, (rows, R)), rng.uniform(0.05, 0.95, (rows, 2 * R))], axis=1)
    return acts.astype(np.float32), rng.uniform(-1, 1, (rows, R)).astype(np.float32), rng.uniform(-1, 1, (rows, R)).astype(np.float32)


def _compare(bad, name, got, ref, tol=2e-5):
    if np.isnan(got).any():
        bad.append("%s: NaN in the result: a pad was read" % name)
        return
    err = np.abs(got - ref).max() if got.size else 0.0
    _note("fused/" + name.split("[")[0], err, tol)
    if not err < tol:
        bad.append("%s: error %.3g (bound %.0e)" % (name, err, tol))


def _run_fused(H, c, rng):
    M, N, K, e = c["M"], c["N"], c["K"], c["epi"]
    A, B, Ain, Bin = _operands(c, rng, 0.1)
    acc = _product64(A, B, c)
    keep, runs, bad = [], [], []
    ptr0 = dict(A=Ain.ptr, B=Bin.ptr)
    refs = {}
    if e == gec.EPI_LSTM_FWD:
        R, ns = c["R"], c["addend_slabs"]
        bias, c_prev = (rng.uniform(-1, 1, N) * 0.1).astype(np.float32), rng.uniform(-1, 1, (M, R)).astype(np.float32)
        ptr0.update(bias=_dense_in(keep, bias), p0=_dense_in(keep, c_prev))
        pre = acc.copy()
        if ns:
            slabs = (rng.uniform(-1, 1, (ns, M, N)) * 0.3).astype(np.float32)
            keep.append(_In(slabs.reshape(ns * M, N), c["ldadd"]))
            ptr0["addend"] = keep[-1].ptr
            pre += slabs.astype(np.float64).sum(0)
        pre += bias
        gi, gj, gf, go = _sig(pre[:, :R]), np.tanh(pre[:, R:2 * R]), _sig(pre[:, 2 * R:3 * R] + 1.0), _sig(pre[:, 3 * R:])
        cn = c_prev * gf + gi * gj
        refs = dict(q0=np.concatenate([gi, gj, gf, go], axis=1), q1=cn, q2=np.tanh(cn) * go)
        shapes = dict(C=(M, 0, c["ldc"]), q0=(M, 4 * R, 4 * R), q1=(M, R, R), q2=(M, R, R))
        twins = dict(q2_16="q2") if c["q2_16"] else {}
    elif e == gec.EPI_REPARAM_FWD:
        Z = c["Z"]
        bias, eps = (rng.uniform(-1, 1, N) * 0.1).astype(np.float32), rng.uniform(-1, 1, (M, Z)).astype(np.float32)
        ptr0.update(bias=_dense_in(keep, bias), p0=_dense_in(keep, eps))
        ml = acc + bias
        refs = dict(C=ml, q0=ml[:, :Z] + eps * np.sqrt(np.exp(ml[:, Z:])))
        shapes = dict(C=(M, N, c["ldc"]), q0=(M, Z, Z))
        twins = dict(q0_16="q0")
    elif e in (gec.EPI_LSTM_BWD, gec.EPI_LSTM_BWD_TAIL):
        R = c["R"]
        i0 = c["i0"] if e == gec.EPI_LSTM_BWD_TAIL else 0
        rows = M - i0                                                    # rows of the step's own arrays
        acts, c_prev, c_new = _cell_inputs(rng, max(rows, 1), R)
        # (the step's arrays hold M - i0 rows; i0 rows of NaN behind them: a row index that forgets i0 shows in the result)
        nanrows = lambda v: np.concatenate([v, np.full((i0, v.shape[1]), np.nan, np.float32)])  # noqa: E731
        ptr0.update(p0=_dense_in(keep, nanrows(acts)), p1=_dense_in(keep, nanrows(c_prev)), p2=_dense_in(keep, nanrows(c_new)))
        dh = acc.copy()
        if c["addend"]:
            add = rng.uniform(-1, 1, (M, N)).astype(np.float32)
            keep.append(_In(add, c["ldadd"]))
            ptr0["addend"] = keep[-1].ptr
            dh += add
        dc_in = None
        if c["p3"]:
            dc_in = rng.uniform(-1, 1, (M, R)).astype(np.float32)
            ptr0["p3"] = _dense_in(keep, dc_in)
        dg, dcp = _cell_backward64(dh[i0:], acts[:rows], c_prev[:rows], c_new[:rows], dc_in, R)
        refs = dict(q0=dg, q1=dcp)
        shapes = dict(C=(M, N if i0 else 0, c["ldc"]), q0=(max(rows, 1), 4 * R, 4 * R), q1=(max(rows, 1), R, R))
        ds0 = None
        if c["q2"]:
            shapes["q2"] = (max(rows, 1), 4 * R, 4 * R)
            ds0 = rng.uniform(-1, 1, (rows, 4 * R)).astype(np.float32) if c["q2"] == "acc" else None
            refs["q2"] = dg + (ds0 if ds0 is not None else 0.0)
        if i0:
            refs["C"] = dh[:i0]
        twins = {k: k[:2] for k in ("q0_16", "q2_16") if c[k]}
    else:
        Z = c["Z"]
        ml = np.concatenate([rng.uniform(-1, 1, (M, Z)), rng.uniform(-1, 0.5, (M, Z))], axis=1).astype(np.float32)
        eps = rng.uniform(-1, 1, (M, Z)).astype(np.float32)
        att = rng.uniform(-1, 1, (M, H.ATT_STRIDE)).astype(np.float32)
        att[:, H.ATT_MASK] = (np.arange(M) % 3 != 1).astype(np.float32)               # a mixed 0 / 1 mask
        dyn = rng.uniform(0.5, 1.5, H.DYN_COUNT).astype(np.float32)
        dyn[H.DYN_VAE_PV], dyn[H.DYN_VAE_PM], dyn[H.DYN_GRAD_SCALE] = 0.9, 0.1, 1.0 / max(M, 2)
        ptr0.update(p0=_dense_in(keep, ml), p1=_dense_in(keep, eps), p2=_dense_in(keep, att), p3=_dense_in(keep, dyn))
        klg = att[:, H.ATT_MASK:H.ATT_MASK + 1].astype(np.float64) * np.float64(dyn[H.DYN_GRAD_SCALE])
        pv, pm = np.float64(dyn[H.DYN_VAE_PV]), np.float64(dyn[H.DYN_VAE_PM])
        var = np.exp(ml[:, Z:].astype(np.float64))
        dmean = acc + klg * (ml[:, :Z] - pm) / pv
        dlv = acc * eps * 0.5 * np.sqrt(var) + klg * 0.5 * (var / pv - 1.0)
        refs = dict(C=np.concatenate([dmean, dlv], axis=1))
        shapes = dict(C=(M, 2 * Z, c["ldc"]))
        twins = dict(C16="C")
    for form in _forms(c):
        outs = {}
        for name, (rows, width, ld) in shapes.items():
            init = ds0 if (name == "q2" and e == gec.EPI_LSTM_BWD and c["q2"] == "acc") else None
            outs[name] = _Out(rows, width, ld, init=init)
        for t16, src in twins.items():
            rows, width, ld = shapes[src]
            outs[t16] = _Out(rows, width, ld, bits=16)
        ptr = dict(ptr0)
        ptr.update({name: o.ptr for name, o in outs.items()})
        ptr.update(_twin_ptrs(H, form, Ain, Bin, keep, gates=(e == gec.EPI_LSTM_FWD)))
        _launch(H, gec.descriptor(H, form, ptr))
        runs.append(outs)
    _sync()
    nrows = {name: refs[name].shape[0] for name in refs}
    for outs in runs:
        for name in shapes:
            o = outs[name]
            mask = o.mask(rows=nrows.get(name, 0)) if name in refs else o.mask(rows=0)
            bad += ["%s: %s" % (name, b) for b in o.check(mask)[0]]
        for t16, src in twins.items():
            bad += _twin_problems(t16, outs[t16], outs[src], outs[t16].mask(rows=nrows[src]))
    if not bad:
        last = runs[-1]
        for name, ref in refs.items():
            got = last[name].body().view(np.float32)[0, :ref.shape[0], :ref.shape[1]]
            _compare(bad, "%s[epi %d]" % (name, e), got, ref)
        if len(runs) == 2:
            for name, ref in refs.items():
                a, b = (r[name].body()[0, :ref.shape[0], :ref.shape[1]] for r in runs)
                if not np.array_equal(a, b):
                    bad.append("%s: twin launch differs from the fp32-operand launch" % name)
    return bad


FUSED = gec.fused_cases()


@pytest.mark.parametrize("epi", [gec.EPI_LSTM_FWD, gec.EPI_REPARAM_FWD, gec.EPI_LSTM_BWD, gec.EPI_REPARAM_BWD, gec.EPI_LSTM_BWD_TAIL],
                         ids=["lstm_fwd", "reparam_fwd", "lstm_bwd", "reparam_bwd", "lstm_bwd_tail"])
@pytest.mark.parametrize("prec", [0, 1])
def test_fused_epilogues_at_ragged_rows_and_unit_counts(H, prec, epi):
    """M = 1, 17, 37; R and Z odd (the fallback kernels' run-time epilogue), even, and multiples of 4 (four-unit tiles);
    addend slab counts 0, 1, 3, 4, 8; i0 of AIR_EPI_LSTM_BWD_TAIL at 0, inside a tile, at a tile edge and at M; nullable
    operands absent and present -- against the float64 formulas of include/air_hip.h"""
    cases = [c for c in FUSED if c["prec"] == prec and c["epi"] == epi]
    assert cases
    _report(_run_cases(H, cases, _run_fused, 4000 + 100 * epi), "fused")
