"""CPU checks of tests/gemm_edge_cases.py, the case tables of tests/test_gpu_gemm_edges.py: air_gemm_kernel_name is host-only
code, so with made-up pointers of the right alignment every case is asked which kernel it would launch.  This is what keeps the
GPU suite from testing only the fallback kernels: a case that drifts to another family, tile or epilogue fails HERE."""
import collections
import ctypes as C
import json
import os
import sys

import pytest

import gemm_edge_cases as gec
from air import _hip as H

BASE = 1 << 20                                   # made-up addresses, 1 MiB apart: every operand 256-byte aligned before its offset
NAMES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_edge_kernel_names.json")


def _name(c):
    ptr = {n: BASE * (i + 1) for i, n in enumerate(("A", "B", "C", "bias", "addend", "aux", "p0", "p1", "p2", "p3", "q0", "q1", "q2",
                                                      "A16", "B16", "C16", "q0_16", "q2_16", "B16p"))}
    buf = C.create_string_buffer(128)
    rc = H.lib().air_gemm_kernel_name(C.byref(gec.descriptor(H, c, ptr)), buf, 128)
    assert rc == 0, (rc, gec.describe(c))
    return buf.value.decode()


CASES = gec.all_cases()


def test_every_case_reaches_the_kernel_it_was_written_for():
    for c in CASES:
        name = _name(c)
        fam, tile, ta, tb, epi = gec.parse_kernel_name(name)
        assert (fam, tile, ta, tb, epi) == (c["family"], tuple(c["ktile"]), bool(c["ta"]), bool(c["tb"]), c["kepi"]), (name, gec.describe(c))
        # the same descriptor without its twins is the fp32-operand launch the twin one is compared with bit for bit: a lean kernel
        if c["family"] == "bf16tw":
            plain = dict(c, A16=False, B16=False, B16p=False)
            assert gec.parse_kernel_name(_name(plain))[0] == "bf16v2", gec.describe(c)
        # every leading dimension strictly wider than the row it strides, every twin flag only where the precision reads twins
        assert c["lda"] > (c["M"] if c["ta"] else c["K"]) and c["ldb"] > (c["K"] if c["tb"] else c["N"]), gec.describe(c)
        assert c["ldc"] > (2 * c["N"] if c["epi"] == gec.EPI_REPARAM_BWD else c["N"]) and c["ldadd"] > c["N"] and c["ldaux"] > c["N"]
        assert c["prec"] == 1 or not (c["A16"] or c["B16"] or c["B16p"])


def test_the_tables_cover_every_family_tile_layout_and_alignment_arm():
    plain = [c for c in CASES if c["group"] == "plain"]
    seen = collections.Counter((c["family"], tuple(c["tile"]), c["layout"]) for c in plain)
    for tile in gec.TILES:
        for fam in ("bf16v2", "f32v2"):
            for layout in ("nn", "nt"):
                assert seen[(fam, tile, layout)] >= 30, (fam, tile, layout)
                arms = collections.Counter(gec.lean_arms(c) for c in plain if (c["family"], tuple(c["tile"]), c["layout"]) == (fam, tile, layout))
                assert all(arms[(ha, hb)] >= 2 for ha in (False, True) for hb in (False, True)) and arms[(False, False)] >= 10, (fam, tile, layout, arms)
        for fam in ("bf16", "f32"):
            for layout in ("nn", "nt", "tn"):
                assert seen[(fam, tile, layout)] >= 17, (fam, tile, layout)
    # each way into the fallback kernels, once per (family, tile): by that condition ALONE
    for c in plain:
        if c.get("trigger"):
            even = c["K"] % 2 == 0 and c["lda"] % 2 == 0 and c["ldb"] % 2 == 0 and c["a_off"] % 8 == 0 and c["b_off"] % 8 == 0 and not c["ta"]
            only = {"odd K": c["K"] % 2 == 1 and c["lda"] % 2 == 0 and c["ldb"] % 2 == 0, "odd lda": c["lda"] % 2 == 1 and c["ldb"] % 2 == 0 and c["K"] % 2 == 0,
                    "A+4": c["a_off"] == 4 and c["lda"] % 2 == 0 and c["K"] % 2 == 0, "B+4": c["b_off"] == 4 and c["ldb"] % 2 == 0 and c["K"] % 2 == 0,
                    "transA": c["ta"] == 1 and c["lda"] % 2 == 0 and c["K"] % 2 == 0}[c["trigger"]]
            assert only and not even, gec.describe(c)
    trig = collections.Counter((c["family"], tuple(c["tile"]), c["trigger"]) for c in plain if c.get("trigger"))
    assert len(trig) == 2 * 8 * 5 and set(trig.values()) == {1, 2}                     # (NN and NT both carry the four operand triggers)
    # the twin combinations twin_rounds admits for the generic epilogue
    for tile, layout, a16, panel in gec.TWIN_COMBOS:
        got = [c for c in plain if c["family"] == "bf16tw" and (tuple(c["tile"]), c["layout"], c["A16"], c["B16p"]) == (tile, layout, a16, panel)]
        assert len(got) >= 18, (tile, layout, a16, panel)
    # tile grids whose workgroup count is not a multiple of 8 (xcd_tile's remainder branch) and ones beyond 8
    for fam in ("bf16v2", "f32v2", "bf16", "f32", "bf16tw"):
        counts = {gec.tile_count(c) for c in plain if c["family"] == fam}
        assert {1, 2, 4, 6, 9} <= counts, (fam, sorted(counts))             # 6 = 3 x 2: not square; 9: one chunk of 2, seven of 1
    # split-K: the short slab counts and a short last slab
    assert [gec.gemm_slabs(K, ks) for K, ks in gec.SPLITK] == [3, 4, 3, 4]
    assert all(H.lib().air_gemm_slabs(K, ks) == gec.gemm_slabs(K, ks) for K, ks in gec.SPLITK + gec.SPLITK_TWIN_A)
    assert {c["family"] for c in CASES if c["group"] == "splitk"} == {"bf16v2", "f32v2", "bf16tw"}
    # fused epilogues: every ABI epilogue through a lean kernel AND through the fallbacks' run-time choice, and through the twins
    fused = collections.Counter((c["epi"], c["family"]) for c in CASES if c["group"] == "fused")
    for epi in (gec.EPI_LSTM_FWD, gec.EPI_REPARAM_FWD, gec.EPI_LSTM_BWD, gec.EPI_REPARAM_BWD):
        for fam in ("bf16v2", "f32v2", "bf16", "f32"):
            assert fused[(epi, fam)] >= 3, (epi, fam)
    assert fused[(gec.EPI_LSTM_BWD_TAIL, "bf16v2")] == 8 and fused[(gec.EPI_LSTM_BWD_TAIL, "f32v2")] == 8
    assert all(fused[(epi, "bf16tw")] >= 2 for epi in (gec.EPI_LSTM_FWD, gec.EPI_LSTM_BWD, gec.EPI_LSTM_BWD_TAIL))
    assert {c["kepi"] for c in CASES if c["epi"] == gec.EPI_LSTM_FWD} == {None, 1, gec.EPI_LSTM_FWD_Q}


def test_the_whole_table_stays_a_few_thousand_launches():
    launches = sum(c["launches"] for c in CASES)
    per = collections.Counter()
    for c in CASES:
        per[(c["group"], c["family"])] += c["launches"]
    print("%d cases, %d launches" % (len(CASES), launches))
    for k in sorted(per):
        print("  %-8s %-8s %5d" % (k[0], k[1], per[k]))
    assert launches < 4100


def coverage_rows():
    cnt = collections.Counter()
    for c in CASES:
        if c["group"] != "plain":
            continue
        if c["family"] in ("bf16v2", "f32v2"):
            ha, hb = gec.lean_arms(c)
            arm = "A%d/B%d" % (8 if ha else 16, 8 if hb else 16)
        elif c["family"] == "bf16tw":
            arm = ("A16" if c["A16"] else "Af32") + "/" + ("B16p" if c["B16p"] else "B16")
        else:
            arm = "-"
        cnt[(c["family"], "%dx%d" % tuple(c["tile"]), c["layout"], arm)] += 1
    return [k + (v,) for k, v in sorted(cnt.items())]


@pytest.mark.parametrize("field,value", [("ldc", -1), ("ldb", -1), ("lda", -1), ("ldadd", -1), ("ldaux", -1)])
@pytest.mark.parametrize("layout", ["nn", "nt", "tn"])
def test_a_leading_dimension_below_the_row_width_is_refused(layout, field, value):
    """fill_args (air_gemm and air_gemm_kernel_name share it): AIR_EINVAL for ldc < N, lda / ldb below the stored row of A / B,
    ldadd / ldaux < N when the operand is given -- and the width itself is accepted"""
    ta, tb = gec.LAYOUTS[layout]
    M, N, K = 17, 18, 66
    width = dict(lda=M if ta else K, ldb=K if tb else N, ldc=N, ldadd=N, ldaux=N)
    buf = C.create_string_buffer(128)

    def rc(**ld):
        g = H.Gemm()
        g.A, g.B, g.C, g.addend, g.aux = BASE, 2 * BASE, 3 * BASE, 4 * BASE, 5 * BASE
        g.M, g.N, g.K, g.transA, g.transB = M, N, K, ta, tb
        for k, v in dict(width, **ld).items():
            setattr(g, k, v)
        named = H.lib().air_gemm_kernel_name(C.byref(g), buf, 128)
        # (air_gemm itself only once the host-only query has refused the descriptor: these pointers are made up)
        return named, H.lib().air_gemm(C.byref(g), None) if named == -1 else 0

    assert rc() == (0, 0)
    assert rc(**{field: width[field] + value}) == (-1, -1)
    # an absent addend / aux carries no leading dimension
    g = H.Gemm()
    g.A, g.B, g.C = BASE, 2 * BASE, 3 * BASE
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.transA, g.transB = M, N, K, width["lda"], width["ldb"], N, ta, tb
    assert H.lib().air_gemm_kernel_name(C.byref(g), buf, 128) == 0


def test_leading_dimension_checks_follow_the_epilogue():
    buf = C.create_string_buffer(128)
    M, Z, K = 17, 10, 64
    # AIR_EPI_REPARAM_BWD writes d_mean | d_log_var: 2N columns of C
    g = H.Gemm()
    g.A, g.B, g.C, g.p0, g.p1, g.p2, g.p3 = (BASE * i for i in range(1, 8))
    g.M, g.N, g.K, g.lda, g.ldb, g.transB, g.epi = M, Z, K, K, K, 1, H.EPI_REPARAM_BWD
    g.ldc = 2 * Z
    assert H.lib().air_gemm_kernel_name(C.byref(g), buf, 128) == 0
    g.ldc = 2 * Z - 1
    assert H.lib().air_gemm_kernel_name(C.byref(g), buf, 128) == -1
    # the padded-A16 form of AIR_EPI_LSTM_FWD0: lda is the TWIN's stride, twin_rounds owns its check (here K = 20 -> 24 fits, 16 does
    # not and is refused as a misalignment of that form, not by the new check) -- while an ordinary lda < K is AIR_EINVAL
    g = H.Gemm()
    g.A, g.B, g.C, g.q0, g.q1, g.q2, g.A16, g.B16p = (BASE * i for i in range(1, 9))
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.epi, g.precision, g.i0 = M, 32, 20, 24, 32, 32, H.EPI_LSTM_FWD0, 1, 2
    assert H.lib().air_gemm_kernel_name(C.byref(g), buf, 128) == 0 and buf.value.decode().startswith("gemm_xwx_glds_kernel")
    g.lda = 16
    assert H.lib().air_gemm_kernel_name(C.byref(g), buf, 128) == -3
    g.i0 = 0
    assert H.lib().air_gemm_kernel_name(C.byref(g), buf, 128) == -1


def _fwd0(prec, K, lda, **more):
    g = H.Gemm()
    g.A, g.B, g.C, g.q0, g.q1, g.q2 = (BASE * i for i in range(1, 7))
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.epi, g.precision = 17, 32, K, lda, 32, 32, H.EPI_LSTM_FWD0, prec
    for k, v in more.items():
        setattr(g, k, v)
    return g


def _tp(N, ksplit):
    g = H.Gemm()
    g.A, g.B, g.C, g.B16 = (BASE * i for i in range(1, 5))
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.precision, g.tile_m, g.tile_n, g.ksplit = 64, N, 128, 128, N, N, 1, 8, 4, ksplit
    return g


def _tiled(tile, job=False):
    g = H.Gemm()
    g.A, g.B, g.C = (BASE * i for i in range(1, 4))
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.tile_m, g.tile_n = 17, 32, 64, 64, 32, 32, tile[0], tile[1]
    if job:
        g.step_job = C.pointer(H.StepJob(dyn=4 * BASE, istate=5 * BASE))
    return g


REFUSED = [
    # the four-unit column map of AIR_EPI_LSTM_FWD0 only exists in the lean kernels: odd K keeps a descriptor out of them
    ("fwd0 odd K fp32", _fwd0(0, 21, 21), -3),
    ("fwd0 odd K bf16", _fwd0(1, 21, 21), -3),
    # C16 of AIR_EPI_LSTM_FWD0 is the padded image twin only the twin kernels write; without a twin of B none of them serves it
    ("fwd0 C16 without twins", _fwd0(1, 64, 64, C16=7 * BASE), -3),
    # the padded-A16 form: lda is the twin's stride and has to hold K rounded up to 8
    ("fwd0 padded A16 lda 16 K 20", _fwd0(1, 20, 16, A16=7 * BASE, B16p=8 * BASE, i0=2), -3),
    # tile (8, 4), the throughput kernel: split-K only, whole 64-column tiles only
    ("tile 8x4 ksplit 1", _tp(128, 1), -1),
    ("tile 8x4 N 96", _tp(96, 2), -3),
    # a tile outside the instantiated ones is refused before the grid or the carried job's planes are sized by it
    ("tile -1x1", _tiled((-1, 1)), -1),
    ("tile -1x1 with a step job", _tiled((-1, 1), job=True), -1),
    ("tile 2x1", _tiled((2, 1)), -1),
]


@pytest.mark.parametrize("what,g,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_the_name_and_the_launch_refuse_alike(what, g, code):
    """air_gemm_kernel_name formats the plan air_gemm launches, so a descriptor the launch refuses gets the same code and no name"""
    buf = C.create_string_buffer(128)
    named = H.lib().air_gemm_kernel_name(C.byref(g), buf, 128)
    assert named != 0, (what, buf.value)
    # (air_gemm itself only once the host-only query has refused the descriptor: these pointers are made up)
    assert H.lib().air_gemm(C.byref(g), None) == named == code, what


def test_the_reported_names_are_the_pinned_ones():
    """tests/golden/gemm_edge_kernel_names.json pins, for every kernel name, how many of the edge cases report it"""
    with open(NAMES_JSON) as f:
        pinned = json.load(f)
    assert dict(collections.Counter(_name(c) for c in CASES)) == pinned


if __name__ == "__main__":
    if "--write-names" in sys.argv:                  # the pin of test_the_reported_names_are_the_pinned_ones: rewrite it on purpose only
        with open(NAMES_JSON, "w") as f:
            json.dump(dict(sorted(collections.Counter(_name(c) for c in CASES).items())), f, indent=1)
            f.write("\n")
    print("| family | tile | layout | arm | cases |\n|---|---|---|---|---|")
    for r in coverage_rows():
        print("| %s | %s | %s | %s | %d |" % r)
