"""air_wgrad_grouped, air_colsum and air_heads_out_wgrad at tile, chunk and image edges, with padded leading dimensions, offset
base pointers, every optional output and guard bands (case tables: tests/wgrad_edge_cases.py; which device function each case
runs, and that the tables reach all of them, is pinned on the CPU by tests/test_wgrad_edge_cases.py).

Every launch runs on poisoned buffers (the helpers of tests/test_gpu_gemm_edges.py): the pad columns of A, dY, A16 and dY16 and
the bytes in front of an offset base hold NaN (fp32 or bf16) -- the ABI defines A(k, m) for m < M only, so a kernel that lets a
pad into its result shows a NaN; dW lies between guard rows with sentinel pads, db and the partials between sentinel guards, all
of which must be bit-identical afterwards, while every element of the written region must have been written.  In head_pack the
cells of wout[o] beyond unit o's segment keep the sentinel.

Values: dW against the float64 product of the operands (rounded to bf16 first at precision 1), db against the float64 column
sums of the fp32 dY, with test_wgrad_grouped's bound |got - ref| <= 2e-6 sqrt(K) 4 max|ref| + 1e-5 |ref|, randn operands, the
rows of dY scaled by 10^(-2 .. 2) as in the twin test.  Partials ONE BY ONE: partial[first_part + mb * tiles_n + nt] is the
float64 sum of squares of the tile's stored block (of the block it would have stored: norm-only) plus the squares of its db
block if, and only if, the restated owner rule names that tile; the bias workgroups' partials follow all tiles in table order;
relative bound 1e-5.  Twin and strip launches are bit-identical to the fp32-operand launch of the same descriptors; norm-only
problems publish the partials of their stored form bit for bit.

Each test collects its failing cases and asserts at the end that there are none."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import wgrad_edge_cases as wec
from test_gpu_gemm_edges import DEV, GUARD, SENT32, _In, _Out
from test_gpu_kernels import _bf16_round

pytestmark = pytest.mark.gpu

NAN16 = np.int16(0x7FC0)                          # bf16 NaN
MAXERR = {}                                       # group/quantity -> largest error / tolerance seen (recorded in DESIGN.md)


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


class _In16:
    """the bf16 twin (RNE) of an input matrix, stored with leading dimension ld behind `off` bytes: pads and front hold bf16 NaN"""

    def __init__(self, values, ld, off=0):
        rows, width = values.shape
        e = off // 2
        host = np.full(e + rows * ld, NAN16, np.int16)
        host[e:].reshape(rows, ld)[:, :width] = torch.from_numpy(np.ascontiguousarray(values)).to(torch.bfloat16).view(torch.int16).numpy()
        self.t = torch.from_numpy(host).to(DEV)
        self.ptr = self.t.data_ptr()              # + a16_off / y16_off is added by wec.descriptor


class _OutW(_Out):
    """an _Out of one fp32 slab whose first element lies `off` bytes behind a 256-byte aligned address, those bytes sentinel too"""

    def __init__(self, rows, width, ld, off=0):
        self.rows, self.width, self.ld, self.slabs, self.bits, self.sent = rows, width, ld, 1, 32, SENT32
        self.e = off // 4
        self.t = torch.from_numpy(np.full(self.e + (2 * GUARD + rows) * ld, SENT32, np.int32)).to(DEV)
        self.ptr = self.t.data_ptr() + GUARD * ld * 4          # + w_off is added by wec.descriptor
        self._host = None

    def host(self):
        if self._host is None:
            flat = self.t.cpu().numpy()
            self.front, self._host = flat[:self.e], flat[self.e:].reshape(-1, self.ld)
        return self._host

    def check(self, mask=None):
        bad, vals = super().check(mask)
        if (self.front != SENT32).any():
            bad.append("the bytes in front of the base written")
        return bad, vals


def _vec(n):
    """n floats between sentinel guards"""
    return _Out(1, n, n)


def _operands(c, rng):
    """(A, dY, device buffers) of a problem"""
    M, N, K = c["M"], c["N"], c["K"]
    A = rng.randn(K, M).astype(np.float32)
    dY = rng.randn(K, N).astype(np.float32)
    if not c["head_pack"]:
        dY = (dY * 10.0 ** rng.randint(-2, 3, (K, 1))).astype(np.float32)
    op = dict(A=A, dY=dY, Ain=_In(A, c["lda"], c["a_off"]), Yin=_In(dY, c["ldb"], c["y_off"]))
    if c["twins"]:
        op.update(A16=_In16(A, c["lda"], c["a16_off"]), Y16=_In16(dY, c["ldb"], c["y16_off"]))
    return op


def _reference(c, op):
    """(dW [M, N] or the 7 head rows as [8, HT], db) in float64"""
    if "ref" not in op:
        A64 = _bf16_round(op["A"]) if c["prec"] else op["A"].astype(np.float64)
        Y64 = _bf16_round(op["dY"]) if c["prec"] else op["dY"].astype(np.float64)
        op["ref"] = (A64.T @ Y64, (op["A"] if c["head_pack"] else op["dY"]).astype(np.float64).sum(0))
    return op["ref"]


def _wmask(c, out):
    """the cells of dW a problem writes: [M, N], or per head unit its segment's width"""
    if not c["head_pack"]:
        return out.mask()
    m = np.zeros((1, out.rows, out.ld), bool)
    for o, (off, wd) in enumerate(wec.head_segments(c["head_pack"])):
        m[0, o, :wd] = True
    return m


def _block_sums(sq, M, N):
    """[tiles_m, tiles_n] sums of a [M, N] array over 64 x 64 tiles"""
    tm, tn = -(-M // wec.BT), -(-N // wec.BT)
    P = np.zeros((tm * wec.BT, tn * wec.BT))
    P[:M, :N] = sq
    return P.reshape(tm, wec.BT, tn, wec.BT).sum((1, 3))


def _cols_sq(v, tn):
    """[tiles_n] sums of squares of a vector over 64-column blocks"""
    P = np.zeros(tn * wec.BT)
    P[:v.size] = v.astype(np.float64) ** 2
    return P.reshape(tn, wec.BT).sum(1)


def _bound_ratio(got, ref, K):
    """largest |got - ref| / (2e-6 sqrt(K) 4 max|ref| + 1e-5 |ref|): test_wgrad_grouped's bound"""
    atol = 2e-6 * np.sqrt(K) * 4 * np.abs(ref).max()
    return float((np.abs(got - ref) / (atol + 1e-5 * np.abs(ref))).max())


class _Form:
    """one launch of a table: its outputs"""

    def __init__(self, H, ln, ops, twins):
        cases = [c if twins else wec.without_twins(c) for c in ln["cases"]]
        self.cases, self.partials = cases, ln["partials"]
        self.dW = [(_OutW(7 if c["head_pack"] else c["M"], max(c["head_pack"]) if c["head_pack"] else c["N"], c["ldc"], c["w_off"])
                    if c["dW"] else None) for c in cases]
        self.db = [(_vec(7 if c["head_pack"] else c["N"]) if c["db"] else None) for c in cases]
        probs = []
        for c, op, w, b in zip(cases, ops, self.dW, self.db):
            ptr = dict(A=op["Ain"].ptr, dY=op["Yin"].ptr, dW=w.ptr if w else 0, db=b.ptr if b else 0)
            if c["twins"]:
                ptr.update(A16=op["A16"].ptr, dY16=op["Y16"].ptr)
            probs.append(wec.descriptor(H, c, ptr))
        arr = (H.Wgrad * len(probs))(*probs)
        self.nblk = H.lib().air_wgrad_num_blocks(arr, len(probs))
        assert self.nblk == wec.num_partials(cases)
        self.part = _vec(self.nblk)
        self.ist = torch.zeros(8, dtype=torch.int32, device=DEV)
        H.check(H.lib().air_wgrad_grouped(arr, len(probs), ln["prec"], C.c_void_p(self.part.ptr if self.partials else 0),
                                          C.c_void_p(self.ist.data_ptr() if self.partials else 0), _stream()), "air_wgrad_grouped")

    def stored(self, i):
        """[rows, width] fp32 of problem i as stored"""
        w = self.dW[i]
        return w.body().view(np.float32)[0, :, :w.width]

    def check(self, H, ops, group):
        bad = []
        first, bias_part = wec.partial_layout(self.cases)
        pb, pv = self.part.check(self.part.mask(width=self.nblk if self.partials else 0))
        bad += ["partials: " + b for b in pb]
        parts = pv[0, 0, :self.nblk].astype(np.float64)
        ist = self.ist.cpu().numpy()
        if int(ist[H.IST_GLOBAL_STEP]) != (1 if self.partials else 0) or ist[1:].any():
            bad.append("istate = %s" % ist.tolist())
        for i, c in enumerate(self.cases):
            name = "problem %d (%s): " % (i, wec.describe(c))
            M, N, K = c["M"], c["N"], c["K"]
            ref_w, ref_b = _reference(c, ops[i])
            tn = wec.tiles_n(c)
            ok = True
            # ---- dW
            if c["dW"]:
                pw, _ = self.dW[i].check(_wmask(c, self.dW[i]))
                bad += [name + "dW: " + b for b in pw]
                ok = not pw
                got = self.stored(i).astype(np.float64)
                if ok and c["head_pack"]:
                    sq_cols = np.zeros(N)                                       # per hidden column: squares of the cells it fed
                    ratio = 0.0
                    for o, (off, wd) in enumerate(wec.head_segments(c["head_pack"])):
                        if np.isnan(got[o, :wd]).any():
                            ok = False
                            continue
                        ratio = max(ratio, _bound_ratio(got[o, :wd], ref_w[o, off:off + wd], K))
                        sq_cols[off:off + wd] += got[o, :wd] ** 2
                    block = _block_sums(sq_cols[None, :], 1, N)
                elif ok:
                    ok = not np.isnan(got).any()
                    ratio = _bound_ratio(got, ref_w, K) if ok else 0.0
                    block = _block_sums(got ** 2, M, N)
                if not ok and not pw:
                    bad.append(name + "NaN in dW: a pad was read")
                elif ok:
                    _note("%s/p%d/dW" % (group, c["prec"]), ratio)
                    if not ratio <= 1.0:
                        bad.append(name + "dW error / bound = %.3g" % ratio)
            else:
                s = c["stored_as"]
                got = self.stored(s).astype(np.float64)
                ok = not np.isnan(got).any()
                block = _block_sums(got ** 2, M, N)
            # ---- db
            dbsq = np.zeros(tn)
            if c["db"]:
                nb = 7 if c["head_pack"] else N
                pd, dv = self.db[i].check()
                bad += [name + "db: " + b for b in pd]
                gb = dv[0, 0, :nb].astype(np.float64)
                if not pd:
                    if np.isnan(gb).any():
                        bad.append(name + "NaN in db: a pad was read")
                        ok = False
                    else:
                        ratio = _bound_ratio(gb, ref_b[:nb], K)
                        _note("%s/p%d/db" % (group, c["prec"]), ratio)
                        if not ratio <= 1.0:
                            bad.append(name + "db error / bound = %.3g" % ratio)
                        dbsq = _cols_sq(gb, tn) if not c["head_pack"] else np.array([(gb ** 2).sum()] + [0.0] * (tn - 1))
                else:
                    ok = False
            # ---- the partials, one by one
            if self.partials and ok and not pb:
                tm = 1 if c["head_pack"] else wec.tiles_m(c)
                owner = np.array([[wec.owns_bias(c, mb, nt) for nt in range(tn)] for mb in range(tm)])
                want = block[:tm] + owner * dbsq[None, :]
                gotp = parts[first[i]:first[i] + tm * tn].reshape(tm, tn)
                rel = np.abs(gotp - want) / np.maximum(want, 1e-300)
                _note("%s/p%d/partial" % (group, c["prec"]), np.nanmax(rel) / 1e-5 if not np.isnan(rel).all() else np.inf)
                if not (rel <= 1e-5).all():
                    mb, nt = np.argwhere(~(rel <= 1e-5))[0]
                    bad.append(name + "%d tile partials off, first at (%d, %d): %.9g, expected %.9g" % (int((~(rel <= 1e-5)).sum()), mb, nt,
                                                                                                    gotp[mb, nt], want[mb, nt]))
                if bias_part[i] is not None:
                    gotb = parts[bias_part[i]:bias_part[i] + tn]
                    relb = np.abs(gotb - dbsq) / np.maximum(dbsq, 1e-300)
                    _note("%s/p%d/partial" % (group, c["prec"]), relb.max() / 1e-5)
                    if not (relb <= 1e-5).all():
                        bad.append(name + "bias-workgroup partials off: %s, expected %s" % (gotb.tolist(), dbsq.tolist()))
        return bad

    def differences(self, other):
        """what is not bit-identical between two forms of a launch"""
        bad = []
        for i, c in enumerate(self.cases):
            if c["dW"] and not np.array_equal(self.dW[i].host(), other.dW[i].host()):
                bad.append("problem %d (%s): dW differs from the fp32-operand launch" % (i, wec.describe(c)))
            if c["db"] and not np.array_equal(self.db[i].host(), other.db[i].host()):
                bad.append("problem %d (%s): db differs from the fp32-operand launch" % (i, wec.describe(c)))
        if not np.array_equal(self.part.host(), other.part.host()):
            d = np.flatnonzero(self.part.body().ravel() != other.part.body().ravel())
            bad.append("%d partials differ from the fp32-operand launch, first at %d" % (d.size, d[0]))
        return bad


def _run_launch(H, ln, rng, group):
    """runs a launch as its cases describe it and, at precision 1 when a case has twins, again without any; returns the problems"""
    ops = []
    for c in ln["cases"]:
        ops.append(ops[c["stored_as"]] if c["stored_as"] is not None else _operands(c, rng))
    forms = [_Form(H, ln, ops, True)]
    if ln["prec"] == 1 and any(c["twins"] for c in ln["cases"]):
        forms.append(_Form(H, ln, ops, False))
    torch.cuda.synchronize()
    bad = []
    for f in forms:
        bad += f.check(H, ops, group)
    if len(forms) == 2:
        bad += forms[0].differences(forms[1])
    # a norm-only problem publishes the partials of its stored form, bit for bit
    f = forms[0]
    first, _ = wec.partial_layout(f.cases)
    for i, c in enumerate(f.cases):
        if c["stored_as"] is not None and f.partials:
            n, p = wec.tiles(c), f.part.body().ravel()
            if not np.array_equal(p[first[i]:first[i] + n], p[first[c["stored_as"]]:first[c["stored_as"]] + n]):
                bad.append("problem %d (%s): partials differ from those of its stored form" % (i, wec.describe(c)))
    tag = ln["id"] or wec.describe(ln["cases"][0])
    return ["%s: %s" % (tag, b) if ln["id"] else b for b in bad], forms


GROUPS = wec.wgrad_launches()


@pytest.mark.parametrize("launches", [g[1] for g in GROUPS if not g[0].startswith("head_pack")],
                         ids=[g[0] for g in GROUPS if not g[0].startswith("head_pack")])
def test_weight_gradients_at_edges_strides_and_guards(H, launches):
    """fp32 operands at both precisions around every chunk, image and round depth with each 16-byte arm on its scalar side; twins
    in 16- and 8-byte pieces and twins that must be ignored; problems of >= 512 tiles through every strip width, A-block form
    and block-row map and with bias owners nt % 1, 2, 7, 8, 16; 16 problems in one launch; norm-only problems next to their
    stored form; db and the partials absent"""
    group = launches[0]["cases"][0]["group"]
    failures = []
    for i, ln in enumerate(launches):
        failures += _run_launch(H, ln, np.random.RandomState(5000 + 17 * i + ln["prec"]), group)[0]
    _report(failures, group)


def _seventeen(struct, one):
    return (struct * 17)(*([one] * 17))


def test_seventeen_problems_are_refused(H):
    """AIR_MAX_WGRAD_PROBLEMS = 16 and air_colsum's 16: one more is AIR_ELIMIT, and nothing is launched"""
    c = wec.f32_operand_cases(0)[0]
    op = _operands(c, np.random.RandomState(1))
    dW, db, part = _OutW(c["M"], c["N"], c["ldc"]), _vec(c["N"]), _vec(17 * wec.tiles(c))
    one = wec.descriptor(H, c, dict(A=op["Ain"].ptr, dY=op["Yin"].ptr, dW=dW.ptr, db=db.ptr))
    for prec in (0, 1):
        assert H.lib().air_wgrad_grouped(_seventeen(H.Wgrad, one), 17, prec, C.c_void_p(part.ptr), None, _stream()) == H.ELIMIT
    src, dst = _In(op["dY"], c["ldb"]), _vec(c["N"])
    assert H.lib().air_colsum(_seventeen(H.Colsum, H.Colsum(src.ptr, dst.ptr, c["K"], c["N"], c["ldb"], 0)), 17, _stream()) == H.ELIMIT
    torch.cuda.synchronize()
    for out in (dW, db, part, dst):
        assert out.check(out.mask(rows=0))[0] == []


@pytest.mark.parametrize("prec", [0, 1])
def test_head_pack_segments_inside_across_and_wider_than_a_tile(H, prec):
    """head widths (64, 48, 16), (5, 17, 33), (100, 70, 130); K = 5, 192, 200, 390 (no bias workgroups: head_pack); ldc = Hmax and
    Hmax + 3; at precision 1 with twins, which are ignored bit for bit; at precision 0 against air_heads_out_wgrad, which sums
    in another order: its own test's bound, rtol 1e-4 and atol 2e-4"""
    failures = []
    for i, c in enumerate(wec.head_pack_cases(prec)):
        bad, forms = _run_launch(H, wec.launch("", [c]), np.random.RandomState(6000 + i), "head_pack")
        failures += bad
        if prec == 0 and not bad:
            op_rng = np.random.RandomState(6000 + i)                            # the same operands again
            op = _operands(c, op_rng)
            dw, db = _OutW(7, max(c["head_pack"]), c["ldc"]), _vec(7)
            Hs, Hh, Hz = c["head_pack"]
            H.check(H.lib().air_heads_out_wgrad(C.c_void_p(op["Ain"].ptr), C.c_void_p(op["Yin"].ptr), C.c_void_p(dw.ptr), C.c_void_p(db.ptr),
                                                c["K"], Hs, Hh, Hz, c["ldc"], _stream()), "air_heads_out_wgrad")
            torch.cuda.synchronize()
            a, b = forms[0].stored(0).astype(np.float64), dw.body().view(np.float32)[0, :, :dw.width].astype(np.float64)
            m = _wmask(c, dw)[0, :, :dw.width]
            ratio = float((np.abs(a[m] - b[m]) / (2e-4 + 1e-4 * np.abs(b[m]))).max())
            _note("head_pack/p0/against air_heads_out_wgrad", ratio)
            if dw.check(_wmask(c, dw))[0] or not ratio <= 1.0:
                failures.append("%s: differs from air_heads_out_wgrad: error / bound = %.3g" % (wec.describe(c), ratio))
    _report(failures, "head_pack")


def test_colsum_at_the_unroll_boundary_with_padded_rows(H):
    """rows on both sides of r + 28 < rows for every wave, cols around the 64-column strip, ld = cols and cols + 3 (NaN pads),
    overwrite and accumulate, 16 problems of different widths in a launch: test_colsum_problems' bound (rtol 1e-5, atol 1e-4)"""
    failures = []
    rng = np.random.RandomState(7000)
    for ln in wec.colsum_launches():
        keep, probs = [], []
        for c in ln:
            src = rng.randn(c["rows"], c["cols"]).astype(np.float32)
            init = rng.randn(c["cols"]).astype(np.float32) if c["accumulate"] else None
            sin, dst = _In(src, c["ld"]), _Out(1, c["cols"], c["cols"], init=None if init is None else init[None, :])
            keep.append((c, sin, dst, src.astype(np.float64).sum(0) + (0.0 if init is None else init)))
            probs.append(H.Colsum(sin.ptr, dst.ptr, c["rows"], c["cols"], c["ld"], c["accumulate"]))
        H.check(H.lib().air_colsum((H.Colsum * len(probs))(*probs), len(probs), _stream()), "air_colsum")
        torch.cuda.synchronize()
        for c, sin, dst, ref in keep:
            bad, vals = dst.check()
            got = vals[0, 0, :c["cols"]].astype(np.float64)
            ratio = float((np.abs(got - ref) / (1e-4 + 1e-5 * np.abs(ref))).max())
            if not bad:
                _note("colsum", ratio)
            if bad or not ratio <= 1.0:
                failures.append("%s: %s error / bound = %.3g" % (c, bad, ratio))
    _report(failures, "colsum")


def test_heads_out_wgrad_at_every_head_width(H):
    """segments wider than 64 (several rounds of 64 columns behind barriers), wout_ld = Hmax and Hmax + 3 (the pad keeps the
    sentinel, as do the cells of a row beyond its head's width), rows on both sides of the unroll boundary: the float64
    contraction within rtol 1e-4, atol 2e-4; bout within rtol 1e-5, atol 1e-4 (test_heads_out_wgrad_matches_grouped_launch)"""
    failures = []
    for i, c in enumerate(wec.heads_out_cases()):
        rng = np.random.RandomState(8000 + i)
        Hs, Hh, Hz = c["hp"]
        HT = 2 * Hs + 2 * Hh + Hz
        d7, hid = rng.randn(c["rows"], 8).astype(np.float32), rng.randn(c["rows"], HT).astype(np.float32)
        din, hin = _In(d7, 8), _In(hid, HT)
        dw, db = _OutW(7, max(c["hp"]), c["ld"]), _vec(7)
        H.check(H.lib().air_heads_out_wgrad(C.c_void_p(din.ptr), C.c_void_p(hin.ptr), C.c_void_p(dw.ptr), C.c_void_p(db.ptr),
                                            c["rows"], Hs, Hh, Hz, c["ld"], _stream()), "air_heads_out_wgrad")
        torch.cuda.synchronize()
        mask = _wmask(dict(head_pack=c["hp"]), dw)
        bad = dw.check(mask)[0] + db.check()[0]
        full = d7.astype(np.float64).T @ hid.astype(np.float64)
        got = dw.body().view(np.float32)[0].astype(np.float64)
        ratio = 0.0
        for o, (off, wd) in enumerate(wec.head_segments(c["hp"])):
            ref = full[o, off:off + wd]
            ratio = max(ratio, float((np.abs(got[o, :wd] - ref) / (2e-4 + 1e-4 * np.abs(ref))).max()))
        refb = d7.astype(np.float64).sum(0)[:7]
        rb = float((np.abs(db.body().view(np.float32)[0, 0, :7] - refb) / (1e-4 + 1e-5 * np.abs(refb))).max())
        if not bad:
            _note("heads_out/dwout", ratio)
            _note("heads_out/dbout", rb)
        if bad or not ratio <= 1.0 or not rb <= 1.0:
            failures.append("%s: %s dwout error / bound = %.3g, dbout %.3g" % (c, bad, ratio, rb))
    _report(failures, "heads_out")
