"""CPU checks of tests/wgrad_edge_cases.py, the case tables of tests/test_gpu_wgrad_edges.py.  Which device function a
weight-gradient workgroup runs is decided by the problem's shape, strides and alignment alone; the case module restates
those rules (each next to the name of the C it restates) and every case names the path it was written for.  Here: every
case reaches the path it names, every path is reached, and the restated tile and workgroup counts are those of
air_wgrad_num_blocks / air_wgrad_num_workgroups -- host-only entry points, asked with made-up pointers of the case's alignment."""
import collections
import ctypes as C

import wgrad_edge_cases as wec
from air import _hip as H

BASE = 1 << 28                                   # made-up addresses, 256 MiB apart: every operand 256-byte aligned before its offset


def _table(cases):
    probs = []
    for i, c in enumerate(cases):
        ptr = {n: BASE * (1 + len(wec.OPERANDS) * i + j) for j, n in enumerate(wec.OPERANDS)}
        probs.append(wec.descriptor(H, c, ptr))
    return (H.Wgrad * len(probs))(*probs)


LAUNCHES = [(gid, ln) for gid, launches in wec.wgrad_launches() for ln in launches]
CASES = wec.all_cases()


def test_every_case_reaches_the_path_it_names():
    for gid, ln in LAUNCHES:
        assert 1 <= len(ln["cases"]) <= wec.MAXP and ln["prec"] in (0, 1)
        for c in ln["cases"]:
            assert c["prec"] == ln["prec"] and c["partials"] == ln["partials"], wec.describe(c)
            got = wec.path_of(c)
            assert all(got.get(k) == v for k, v in c["path"].items()), (got, wec.describe(c))
            assert wec.bias_of(c) == c["bias"], (wec.bias_of(c), wec.describe(c))
            # a twin or strip case is compared with the fp32-operand launch of the same descriptor: tile_bf16
            if got["kind"] in ("tile_bf16_tw", "strip"):
                assert wec.path_of(wec.without_twins(c))["kind"] == "tile_bf16", wec.describe(c)
            assert c["lda"] >= c["M"] and c["ldb"] >= c["N"] and (c["dW"] or c["stored_as"] is not None), wec.describe(c)
            assert c["ldc"] >= (max(c["head_pack"]) if c["head_pack"] else c["N"])
            assert c["dW"] or (ln["partials"] and not c["head_pack"])          # what fill_table asks of a norm-only problem
            if c["stored_as"] is not None:
                s = ln["cases"][c["stored_as"]]
                assert s["dW"] and all(s[k] == c[k] for k in ("M", "N", "K", "lda", "ldb", "ldc", "twins", "db", "a_off", "y_off"))


def test_the_restated_counts_are_the_librarys():
    lib = H.lib()
    for gid, ln in LAUNCHES:
        for cases in (ln["cases"], [wec.without_twins(c) for c in ln["cases"]]):
            arr = _table(cases)
            what = (gid, [wec.describe(c) for c in cases])
            assert lib.air_wgrad_num_blocks(arr, len(cases)) == wec.num_partials(cases), what
            for prec in (0, 1):
                assert lib.air_wgrad_num_workgroups(arr, len(cases), prec) == wec.num_workgroups(cases, prec), (prec, what)
    # the limit of the table
    c = CASES[0]
    arr = _table([c] * (wec.MAXP + 1))
    assert wec.MAXP == H.MAX_WGRAD_PROBLEMS
    assert lib.air_wgrad_num_blocks(arr, wec.MAXP + 1) == H.ELIMIT and lib.air_wgrad_num_workgroups(arr, wec.MAXP + 1, 1) == H.ELIMIT
    assert lib.air_wgrad_num_blocks(arr, wec.MAXP) == wec.MAXP * wec.tiles(c)


def test_dense_problems_of_the_kernel_tests():
    """dense_case() is what tests/test_gpu_kernels.py asks for its strip expectation: the shapes it launches, against the library"""
    lib = H.lib()
    for M, N, K, strip in [(2500, 1024, 64, 2), (8192, 1024, 256, 4), (4096, 2048, 128, 4), (2048, 1024, 192, 2), (2052, 1024, 64, 2),
                           (2500, 1024, 512, 0), (16384, 1024, 2048, 0), (256, 1024, 192, 0), (50, 256, 192, 0), (2048, 4224, 64, 2),
                           (2048, 4160, 64, 0)]:
        c = wec.dense_case(M, N, K)
        assert wec.strip_of(c) == strip and wec.path_of(c) == c["path"], (M, N, K)
        arr = _table([c])
        assert lib.air_wgrad_num_workgroups(arr, 1, 1) == wec.num_workgroups([c], 1) == wec.bias_workgroups(c) + wec.tiles(c) // max(strip, 1)
        assert lib.air_wgrad_num_workgroups(_table([wec.dense_case(M, N, K, twins=False)]), 1, 1) == wec.num_partials([c])


def test_every_path_is_reached():
    """path -> case count: printed (run with -s), recorded in DESIGN.md"""
    seen = collections.Counter()
    for c in CASES:
        p = wec.path_of(c)
        key = {"tile_bf16_tw": lambda: "tile_bf16_tw a16=%d b16=%d" % (p["a16"], p["b16"]),
               "strip": lambda: "strip G=%d A8=%d xcd_map=%d" % (p["G"], p["A8"], p["xcd_map"])}.get(p["kind"], lambda: p["kind"])()
        seen[key] += 1
        seen["bias: %s" % wec.bias_of(c)] += 1
        if p["kind"] in ("tile_f32", "tile_bf16"):
            seen["%s vec(A,dY,dW)=%d%d%d" % ((p["kind"],) + tuple(int(v) for v in wec.vec_arms(c)))] += 1
        if not c["dW"]:
            seen["norm-only"] += 1
        if c["head_pack"]:
            seen["head_pack p%d" % c["prec"]] += 1
    for k in sorted(seen):
        print("%-40s %d" % (k, seen[k]))
    want = ["tile_f32", "tile_bf16", "norm-only", "head_pack p0", "head_pack p1"]
    want += ["tile_bf16_tw a16=%d b16=%d" % (a, b) for a in (8, 16) for b in (8, 16)]
    # every strip width the dispatch has (4, 2), every (A8, map) combination
    want += ["strip G=2 A8=%d xcd_map=%d" % (a, x) for a in (0, 1) for x in (0, 1)] + ["strip G=4 A8=0 xcd_map=1", "strip G=4 A8=1 xcd_map=0"]
    want += ["bias: %s" % b for b in (None, wec.ROW0, wec.ROWMOD, wec.BIASWG)]
    # each 16-byte arm alone on its scalar side, all on the vector side, all on the scalar side
    want += ["%s vec(A,dY,dW)=%s" % (k, v) for k in ("tile_f32", "tile_bf16") for v in ("111", "011", "101", "110", "000")]
    assert [k for k in want if not seen[k]] == []
    # bias owners spread by nt % 1, 2, 7, 8 and 16; strips that fall back (4 -> 2 -> none) do so by N alone
    big = [c for c in CASES if wec.bias_mod(c)]
    assert {wec.bias_mod(c) for c in big} >= {1, 2, 7, 8, 16}
    assert any(wec.tiles(c) >= 2048 and wec.strip_of(c) == 2 for c in big) and any(wec.tiles(c) >= 2048 and c["twins"] and c["K"] == 64 and
                                                                                  wec.twin_ok(c) and wec.strip_of(c) == 0 for c in big)
    assert {c["K"] for c in big if wec.strip_of(c)} == {64, 128, 192, 256}
    # A8 through a ragged M, through lda % 8 != 0 and through an 8-byte aligned A16, each alone
    a8 = [c for c in big if wec.strip_of(c) and wec.strip_a8(c)]
    assert any(c["M"] % 64 and c["lda"] % 8 == 0 and not c["a16_off"] for c in a8)
    assert any(c["M"] % 64 == 0 and c["lda"] % 8 and not c["a16_off"] for c in a8)
    assert any(c["M"] % 64 == 0 and c["lda"] % 8 == 0 and c["a16_off"] == 8 for c in a8)
    # twins unusable through alignment alone and through a stride alone
    tw = [c for c in CASES if c["group"] == "twins" and not wec.twin_ok(c)]
    assert any(c["a16_off"] == 2 and c["lda"] % 4 == 0 and c["ldb"] % 4 == 0 and c["N"] % 4 == 0 for c in tw)
    assert any(c["y16_off"] == 2 and c["lda"] % 4 == 0 and c["ldb"] % 4 == 0 and c["N"] % 4 == 0 for c in tw)
    assert any(c["lda"] % 4 and not c["a16_off"] and not c["y16_off"] for c in tw)


def test_the_pointwise_tables():
    launches = wec.colsum_launches()
    cases = [c for ln in launches for c in ln]
    assert sorted(map(repr, cases)) == sorted(map(repr, wec.colsum_cases())) and all(len(ln) <= wec.COLSUM_MAX for ln in launches)
    assert {c["rows"] for c in cases} == set(wec.COLSUM_ROWS) and {c["cols"] for c in cases} == set(wec.COLSUM_COLS)
    # both sides of the unroll boundary r + 28 < rows for wave 0 (rows 28 / 29) and for wave 3 (rows 31 / 32: 32 / 33 are past it)
    assert {28, 29, 32, 33} <= set(wec.COLSUM_ROWS) and {29, 33} <= set(wec.HEADS_ROWS)
    hp = wec.heads_out_cases()
    assert {c["hp"] for c in hp} == set(wec.HEAD_WIDTHS) and any(max(c["hp"]) > 64 for c in hp) and any(c["ld"] > max(c["hp"]) for c in hp)
    # head segments inside one tile, crossing a tile boundary, wider than a tile; HT a multiple of 4 and not
    kinds = set()
    for widths in wec.HEAD_WIDTHS:
        for off, wd in wec.head_segments(widths):
            kinds.add("wide" if wd > wec.BT else "crossing" if off // wec.BT != (off + wd - 1) // wec.BT else "inside")
    assert kinds == {"wide", "crossing", "inside"}
    assert {(2 * a + 2 * b + c) % 4 == 0 for a, b, c in wec.HEAD_WIDTHS} == {True, False}
