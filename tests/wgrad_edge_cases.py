"""Case tables of tests/test_gpu_wgrad_edges.py: air_wgrad_grouped, air_colsum and air_heads_out_wgrad descriptors at tile,
chunk and image edges, with padded leading dimensions, offset base pointers and every optional output (pure Python: no torch,
no GPU).

A weight-gradient case is a plain dict:
  group    the test it belongs to; prec; M, N, K of dW[M, N] = A[K, M]^T . dY[K, N]
  pads     (pa, pb, pc), added to the widths: lda = M + pa, ldb = N + pb, ldc = N + pc
  a_off / y_off / w_off / a16_off / y16_off   byte offsets of the A, dY, dW, A16 and dY16 bases from a 256-byte aligned allocation
  twins    the launch is given A16 / dY16; db; dW (False: a norm-only problem); partials (False: sq_partials and istate NULL)
  head_pack  None or (Hs, Hh, Hz): the 7 head output units (M = 8, N = 2 Hs + 2 Hh + Hz, dW = wout [7][ldc])
  path     what the case is WRITTEN FOR: dict(kind='tile_f32' | 'tile_bf16' | 'tile_bf16_tw' | 'strip') and, where the author
           pins them, a16 / b16 (piece widths in bytes of a twin tile) or G / A8 / xcd_map (of a strip)
  bias     who sums db: None (no db) | ROW0 | ROWMOD | BIASWG
  stored_as  (norm-only problems) index, in the same launch, of the same problem with dW stored: it shares its operands

A launch is dict(id, prec, partials, cases).  path_of() / bias_of() restate the dispatch of csrc/air_wgrad.hip;
tests/test_wgrad_edge_cases.py checks on the CPU that every case reaches the path it names and that the restated tile and
workgroup counts are those of air_wgrad_num_blocks / air_wgrad_num_workgroups."""

BT = 64                      # BT of air_wgrad.hip: the output tile
BIG_TILES = 512              # BIG_TILES
MAXP = 16                    # AIR_MAX_WGRAD_PROBLEMS
ROW0, ROWMOD, BIASWG = "tile row 0", "tile row nt % bias_mod", "bias workgroup"
HEAD_OF_UNIT = [0, 1, 2, 2, 3, 3, 4]         # air_out_head (air_common.h)


# ---- the dispatch of air_wgrad.hip, restated --------------------------------------------------------------------------------
def rows8(off, ld):
    """rows8(): rows of a bf16 twin start 8-byte aligned (ld in elements, off: byte offset of the base)"""
    return ld % 4 == 0 and off % 8 == 0


def rows16(off, ld):
    """rows16()"""
    return ld % 8 == 0 and off % 16 == 0


def tiles_m(c):
    return -(-c["M"] // BT)


def tiles_n(c):
    """Prob::tiles_n"""
    return -(-c["N"] // BT)


def tiles(c):
    return tiles_m(c) * tiles_n(c)


def twin_ok(c):
    """twin_ok(): both twins, usable in 8-byte pieces at least"""
    M, lda = c["M"], c["lda"]
    return bool(c["twins"] and not c["head_pack"] and rows8(c["a16_off"], lda) and rows8(c["y16_off"], c["ldb"]) and
                (M % 4 == 0 or lda >= (M + 3) // 4 * 4) and c["N"] % 4 == 0)


def twin_pieces(c):
    """a16 / b16 of tile_bf16_tw: the piece width in bytes of each operand"""
    a16 = rows16(c["a16_off"], c["lda"]) and c["M"] % 8 == 0
    b16 = rows16(c["y16_off"], c["ldb"]) and c["N"] % 8 == 0
    return (16 if a16 else 8), (16 if b16 else 8)


def strip_of(c, allow=True):
    """strip_of(): column tiles per strip workgroup, 0: one tile per workgroup.  allow: precision 1"""
    if not allow or not c["twins"] or not c["dW"] or c["head_pack"]:
        return 0
    if c["K"] not in (64, 128, 192, 256):
        return 0
    if not rows8(c["a16_off"], c["lda"]) or c["M"] % 4 != 0:
        return 0
    if not rows16(c["y16_off"], c["ldb"]):
        return 0
    if tiles(c) < BIG_TILES:
        return 0
    w = 4 if tiles(c) >= 2048 else 2
    while w > 1 and c["N"] % (BT * w) != 0:
        w >>= 1
    return w if w > 1 else 0


def strip_a8(c):
    """the A8 choice of run_tile_bf16: the A block of a strip in masked 8-byte pieces"""
    return not (rows16(c["a16_off"], c["lda"]) and c["M"] % BT == 0)


def strip_xcd_map(c):
    """find_tile(): block-rows of a strip problem are dealt per XCD when their number is a multiple of 8"""
    return tiles_m(c) % 8 == 0


def bias_mod(c):
    """Prob::bias_mod (fill_table): 0 -> block-row 0 owns every bias column"""
    return 0 if c["head_pack"] or tiles(c) < BIG_TILES else min(tiles_m(c), 16)


def bias_workgroups(c):
    """the K >= 384 rule of fill_table: how many workgroups of their own sum this problem's db"""
    return tiles_n(c) if (c["db"] and not c["head_pack"] and c["K"] >= 384) else 0


def owns_bias(c, mb, nt):
    """owns_bias(): does the tile (mb, nt) store db[nt * 64 ..] and count its squares?  (head_pack: tile_f32 / tile_bf16, n0 == 0)"""
    if not c["db"]:
        return False
    if c["head_pack"]:
        return nt == 0
    if bias_workgroups(c):
        return False
    return mb == nt % bias_mod(c) if bias_mod(c) > 0 else mb == 0


def path_of(c, prec=None):
    """what run_tile_bf16 / wgrad_grouped_kernel run for the tiles of the case"""
    prec = c["prec"] if prec is None else prec
    if prec == 0:
        return dict(kind="tile_f32")
    g = strip_of(c)
    if g:
        return dict(kind="strip", G=g, A8=strip_a8(c), xcd_map=strip_xcd_map(c))
    if twin_ok(c):
        a16, b16 = twin_pieces(c)
        return dict(kind="tile_bf16_tw", a16=a16, b16=b16)
    return dict(kind="tile_bf16")


def bias_of(c):
    if not c["db"]:
        return None
    if c["head_pack"]:
        return ROW0
    if bias_workgroups(c):
        return BIASWG
    return ROWMOD if bias_mod(c) > 0 else ROW0


def num_partials(cases):
    """air_wgrad_num_blocks: one partial per tile, then one per bias workgroup"""
    return sum(tiles(c) for c in cases) + sum(bias_workgroups(c) for c in cases)


def num_workgroups(cases, prec):
    """air_wgrad_num_workgroups: the bias workgroups, then tiles or strips"""
    n = sum(bias_workgroups(c) for c in cases)
    for c in cases:
        g = strip_of(c, prec == 1)
        n += tiles(c) // g if g else tiles(c)
    return n


def partial_layout(cases):
    """([Prob::first_part], [Prob::bias_part or None]) of a launch"""
    first, at = [], 0
    for c in cases:
        first.append(at)
        at += tiles(c)
    bias = []
    for c in cases:
        bias.append(at if bias_workgroups(c) else None)
        at += bias_workgroups(c)
    return first, bias


def head_segments(hp):
    """per output unit (offset, width) of its head's hidden segment: air_head_off / air_head_wid"""
    Hs, Hh, Hz = hp
    offs = [0, Hs, 2 * Hs, 2 * Hs + Hh, 2 * Hs + 2 * Hh]
    wid = [Hs, Hs, Hh, Hh, Hz]
    return [(offs[h], wid[h]) for h in HEAD_OF_UNIT]


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _case(group, prec, M, N, K, pads=(0, 0, 0), path=None, bias=ROW0, **kw):
    pa, pb, pc = pads
    c = dict(group=group, prec=prec, M=M, N=N, K=K, pads=tuple(pads), lda=M + pa, ldb=N + pb, ldc=N + pc,
             a_off=0, y_off=0, w_off=0, a16_off=0, y16_off=0, twins=False, db=True, dW=True, partials=True, head_pack=None,
             path=dict(kind=path) if isinstance(path, str) else dict(path), bias=bias, stored_as=None, note="")
    c.update(kw)
    if not c["db"]:
        c["bias"] = None
    return c


def dense_case(M, N, K, prec=1, twins=True):
    """a problem on dense, aligned operands (lda = M, ldb = ldc = N), as the tests of tests/test_gpu_kernels.py launch them"""
    c = _case("dense", prec, M, N, K, path="", twins=twins)
    c["path"], c["bias"] = path_of(c), bias_of(c)
    return c


def launch(lid, cases, prec=None, partials=None):
    prec = cases[0]["prec"] if prec is None else prec
    return dict(id=lid, prec=prec, cases=list(cases), partials=all(c["partials"] for c in cases) if partials is None else partials)


def _star(base, lists):
    """vary each dimension of base = (M, N, K) alone through its list, then the all-min and all-max corners; no duplicates"""
    out = [base]
    for axis, vals in enumerate(lists):
        for v in vals:
            s = list(base)
            s[axis] = v
            out.append(tuple(s))
    out.append(tuple(min(v) for v in lists))
    out.append(tuple(max(v) for v in lists))
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def _vec_pads(M, N, extra=(4, 4, 4)):
    """pads that make every leading dimension a multiple of 4 and strictly wider than its row: the 16-byte arms (vecA, vecB, vecC)
    with quads that straddle M or N when those are no multiples of 4"""
    return (-M % 4 + extra[0], -N % 4 + extra[1], -N % 4 + extra[2])


F32_BASE = (65, 66, 66)
F32_MN = [1, 63, 64, 65, 127, 129]
F32_K = {0: [1, 31, 32, 33, 191, 192, 193, 383, 384, 385],              # 32-row chunks, 192-row rounds of tile_f32<6>
         1: [1, 7, 8, 9, 63, 64, 65, 191, 192, 193, 383, 384, 385]}     # 8-row k-runs, 64-row images, 192-row rounds of tile_bf16
ARM_SHAPES = [F32_BASE, (64, 64, 64), (68, 60, 40)]                     # (64, 64, 64): `plain` / interior; (68, 60, 40): K % 32 != 0
ARM_PADS = [(0, 0, 0), (4, 4, 4), (1, 4, 4), (4, 1, 4), (4, 4, 1)]


def _kind32(prec):
    return "tile_bf16" if prec else "tile_f32"


def f32_operand_cases(prec):
    """fp32 operands at either precision: the star, then pads and 4-byte-offset bases at three shapes"""
    out = []
    for M, N, K in _star(F32_BASE, (F32_MN, F32_MN, F32_K[prec])):
        out.append(_case("f32ops", prec, M, N, K, _vec_pads(M, N), _kind32(prec), BIASWG if K >= 384 else ROW0))
    for M, N, K in ARM_SHAPES:
        for pads in ARM_PADS:
            out.append(_case("f32ops", prec, M, N, K, pads, _kind32(prec), note="pads"))
        for off in ("a_off", "y_off", "w_off"):
            out.append(_case("f32ops", prec, M, N, K, (4, 4, 4), _kind32(prec), note=off + "+4", **{off: 4}))
    return out


def vec_arms(c):
    """(vecA, vecB, vecC) of tile_f32 / tile_bf16 / store_tile"""
    return (c["lda"] % 4 == 0 and c["a_off"] % 16 == 0, c["ldb"] % 4 == 0 and c["y_off"] % 16 == 0,
            c["ldc"] % 4 == 0 and c["w_off"] % 16 == 0)


TWIN_BASE = (68, 72, 72)
TWIN_M = [4, 60, 64, 68, 124, 132]
TWIN_N = [4, 36, 40, 64, 68, 136]
TWIN_K = [8, 56, 64, 72, 192, 200, 384, 392]


def _tw(M, N, K, pads, a16=None, b16=None, **kw):
    path = dict(kind="tile_bf16_tw")
    if a16:
        path["a16"] = a16
    if b16:
        path["b16"] = b16
    return _case("twins", 1, M, N, K, pads, path, BIASWG if K >= 384 else ROW0, twins=True, **kw)


def twin_cases():
    """precision 1 with A16 / dY16 (every case is also launched without them)"""
    out = []
    for pads, wide in (((8, 8, 4), True), ((4, 4, 4), False)):
        for M, N, K in _star(TWIN_BASE, (TWIN_M, TWIN_N, TWIN_K)):
            # + 8 keeps 16-byte rows (16-byte pieces where the width is made of whole ones), + 4 leaves 8-byte rows
            out.append(_tw(M, N, K, pads, a16=16 if wide and M % 8 == 0 else 8, b16=16 if wide and N % 8 == 0 else 8))
    out.append(_tw(64, 72, 72, (8, 8, 4), a16=16, b16=16, note="all 16-byte pieces"))
    out.append(_tw(64, 72, 72, (8, 8, 4), a16=8, b16=16, a16_off=8, note="A16+8"))
    out.append(_tw(64, 72, 72, (8, 8, 4), a16=16, b16=8, y16_off=8, note="dY16+8"))
    out.append(_tw(64, 72, 200, (8, 8, 4), a16=8, b16=8, a16_off=8, y16_off=8, note="A16+8 dY16+8"))
    out.append(_tw(50, 72, 72, (2, 8, 4), a16=8, note="padded rows: M = 50, lda = 52"))
    out.append(_tw(50, 256, 192, (2, 0, 0), a16=8, b16=16, note="padded rows: M = 50, lda = 52"))
    # twins the launch is given and must silently ignore: it runs, and equals, the fp32-operand launch
    un = dict(twins=True)
    out.append(_case("twins", 1, 64, 72, 72, (8, 8, 4), "tile_bf16", a16_off=2, note="A16+2: unusable by alignment", **un))
    out.append(_case("twins", 1, 64, 72, 72, (8, 8, 4), "tile_bf16", y16_off=2, note="dY16+2: unusable by alignment", **un))
    out.append(_case("twins", 1, 64, 72, 72, (8, 8, 4), "tile_bf16", a16_off=4, note="A16+4: unusable by alignment", **un))
    out.append(_case("twins", 1, 50, 72, 72, (0, 8, 4), "tile_bf16", note="M = 50, lda = 50: unusable by stride", **un))
    out.append(_case("twins", 1, 68, 72, 72, (8, 2, 4), "tile_bf16", note="ldb % 4 != 0: unusable by stride", **un))
    out.append(_case("twins", 1, 68, 66, 72, (8, 6, 2), "tile_bf16", note="N % 4 != 0", **un))
    out.append(_case("twins", 1, 68, 70, 200, (8, 2, 2), "tile_bf16", note="N % 4 != 0", **un))
    return out


def _strip(G, A8, xcd):
    return dict(kind="strip", G=G, A8=A8, xcd_map=xcd)


def big_cases():
    """problems of >= 512 tiles: strips of 4 and 2 and their fall-backs, every (A8, map) combination, bias owners nt % 1 .. 16"""
    tw = dict(twins=True, bias=ROWMOD)
    P = (8, 8, 4)
    out = [
        _case("big", 1, 448, 4736, 64, P, _strip(2, False, False), note="7 x 74 tiles, bias_mod 7", **tw),
        _case("big", 1, 452, 4096, 64, P, _strip(2, True, True), note="ragged M, bias_mod 8", **tw),
        _case("big", 1, 512, 4096, 64, (4, 8, 4), _strip(2, True, True), note="lda = 516", **tw),
        _case("big", 1, 512, 4096, 64, P, _strip(2, True, True), a16_off=8, note="A16+8", **tw),
        _case("big", 1, 64, 32768, 64, P, _strip(2, False, False), note="bias_mod 1", **tw),
        _case("big", 1, 128, 16384, 64, P, _strip(2, False, False), note="bias_mod 2", **tw),
        _case("big", 1, 2048, 4096, 64, P, _strip(4, False, True), note="strips of 4", **tw),
        _case("big", 1, 2052, 4096, 64, (4, 8, 4), _strip(4, True, False), note="strips of 4, ragged M", **tw),
        _case("big", 1, 2048, 4224, 64, P, _strip(2, False, True), note="N % 256 != 0: strips of 2", **tw),
        _case("big", 1, 2048, 4160, 64, P, dict(kind="tile_bf16_tw", a16=16, b16=16), note="N % 128 != 0: no strip", **tw),
        _case("big", 1, 512, 4096, 64, P, dict(kind="tile_bf16_tw", a16=16, b16=8), y16_off=8, note="dY16+8: no strip", **tw),
        _case("big", 1, 452, 4096, 128, P, _strip(2, True, True), note="K = 128", **tw),
        _case("big", 1, 512, 4096, 192, (4, 8, 4), _strip(2, True, True), note="K = 192, lda = 516", **tw),
        _case("big", 1, 128, 16384, 256, P, _strip(2, False, False), note="K = 256", **tw),
        _case("big", 1, 580, 3328, 64, P, _strip(2, True, False), note="10 block-rows, ragged M: A8 on the plain map", **tw),
        _case("big", 1, 448, 4736, 96, P, dict(kind="tile_bf16_tw", a16=16, b16=16), note="K = 96: not a strip depth", **tw),
        # the owner rule is by shape alone: without twins, at either precision
        _case("big", 0, 448, 4736, 64, P, "tile_f32", ROWMOD, note="no twins"),
        _case("big", 1, 448, 4736, 64, P, "tile_bf16", ROWMOD, note="no twins"),
    ]
    return out


def _norm_only(c, stored_as):
    return dict(c, dW=False, stored_as=stored_as, w_off=0, path=dict(c["path"]), note="norm-only")


def norm_only_launches():
    """three problems with dW = NULL, each next to the same problem with dW stored; at both precisions (twins: precision 1 reads them)"""
    out = []
    for prec in (0, 1):
        stored = [_case("norm", prec, 70, 33, 40, (2, 3, 3), _kind32(prec), note="ragged"),
                  _case("norm", prec, 68, 72, 72, (8, 8, 4), "tile_bf16_tw" if prec else "tile_f32", twins=True, note="twin"),
                  _case("norm", prec, 65, 136, 392, (3, 4, 4), _kind32(prec), BIASWG, note="K >= 384 with db")]
        cases = []
        for c in stored:
            cases += [c, _norm_only(c, len(cases))]
        out.append(launch("norm-p%d" % prec, cases))
    return out


def optional_output_launches():
    out = []
    for prec in (0, 1):
        k = _kind32(prec)
        # db = NULL on some problems of a launch and not on others (a K >= 384 one among each)
        cases = [_case("optional", prec, 65, 66, 66, _vec_pads(65, 66), k, db=False),
                 _case("optional", prec, 65, 130, 66, _vec_pads(65, 130), k),
                 _case("optional", prec, 33, 70, 390, _vec_pads(33, 70), k, db=False),
                 _case("optional", prec, 70, 130, 390, _vec_pads(70, 130), k, BIASWG),
                 _case("optional", prec, 64, 64, 64, (4, 4, 4), k, db=False)]
        out.append(launch("some-db-p%d" % prec, cases))
        # sq_partials = NULL with istate = NULL on a non-strip launch
        cases = [_case("optional", prec, 65, 66, 66, _vec_pads(65, 66), k, partials=False),
                 _case("optional", prec, 70, 130, 390, _vec_pads(70, 130), k, BIASWG, partials=False),
                 _case("optional", prec, 68, 72, 72, (8, 8, 4), "tile_bf16_tw" if prec else "tile_f32", twins=True, partials=False),
                 _case("optional", prec, 64, 64, 64, (4, 4, 4), k, db=False, partials=False)]
        out.append(launch("no-partials-p%d" % prec, cases))
    return out


HEAD_WIDTHS = [(64, 48, 16), (5, 17, 33), (100, 70, 130)]     # segments inside one tile, crossing tile edges, wider than a tile
HEAD_K = [5, 192, 200, 390]


def head_case(prec, hp, K, pc, twins=False, group="head_pack"):
    Hs, Hh, Hz = hp
    HT = 2 * Hs + 2 * Hh + Hz
    c = _case(group, prec, 8, HT, K, (0, 0, 0), _kind32(prec), ROW0, head_pack=tuple(hp), twins=twins)
    c["ldc"] = max(hp) + pc                                   # dW = wout [7][ldc]
    c["pads"] = (0, 0, pc)
    return c


def head_pack_cases(prec):
    """head_pack: K < one chunk, a whole round, past it, past the K >= 384 switch (which head_pack must NOT take); ldc = Hmax, + 3"""
    return [head_case(prec, hp, K, pc, twins=bool(prec)) for hp in HEAD_WIDTHS for K in HEAD_K for pc in (0, 3)]


def table_launches():
    """16 problems in one launch, mixing the paths above; two K >= 384 problems that are not adjacent"""
    out = []
    for prec in (0, 1):
        k = _kind32(prec)
        tw = "tile_bf16_tw" if prec else "tile_f32"
        cases = [
            _case("table", prec, 65, 66, 66, _vec_pads(65, 66), k),
            _case("table", prec, 68, 72, 72, (8, 8, 4), tw, twins=True),
            _case("table", prec, 70, 130, 390, _vec_pads(70, 130), k, BIASWG),
            _case("table", prec, 1, 1, 1, (3, 3, 3), k),
            head_case(prec, (5, 17, 33), 40, 3, twins=True, group="table"),
            _case("table", prec, 64, 64, 64, (4, 4, 4), k, db=False),
            _case("table", prec, 64, 32768, 64, (8, 8, 4), _strip(2, False, False) if prec else "tile_f32", ROWMOD, twins=True),
            _case("table", prec, 129, 65, 33, (3, 3, 3), k, a_off=4, w_off=4),
            _case("table", prec, 50, 72, 72, (2, 8, 4), tw, twins=True),
            _case("table", prec, 64, 136, 384, (8, 8, 4), tw, BIASWG, twins=True),
            _case("table", prec, 127, 63, 193, (1, 1, 1), k),
        ]
        cases.append(_norm_only(cases[0], 0))
        cases += [
            _case("table", prec, 64, 72, 72, (8, 8, 4), k, twins=True, a16_off=2),
            _case("table", prec, 4, 4, 8, (4, 4, 4), tw, twins=True),
            _case("table", prec, 63, 129, 7, (1, 3, 3), k, y_off=4),
            _case("table", prec, 132, 136, 200, (4, 4, 4), tw, twins=True),
        ]
        assert len(cases) == MAXP
        out.append(launch("table-p%d" % prec, cases))
    return out


def wgrad_launches():
    """every launch of the GPU suite, single problems included: [(group id, [launch])]"""
    groups = []
    for prec in (0, 1):
        groups.append(("f32ops-p%d" % prec, [launch("", [c]) for c in f32_operand_cases(prec)]))
    groups.append(("twins", [launch("", [c]) for c in twin_cases()]))
    for i, c in enumerate(big_cases()):
        groups.append(("big-%02d-%dx%dx%d-%s" % (i, c["M"], c["N"], c["K"], c["path"]["kind"]), [launch("", [c])]))
    groups.append(("table", table_launches()))
    groups.append(("norm-only", norm_only_launches()))
    groups.append(("optional", optional_output_launches()))
    for prec in (0, 1):
        groups.append(("head_pack-p%d" % prec, [launch("", [c]) for c in head_pack_cases(prec)]))
    return groups


def all_cases():
    return [c for _, launches in wgrad_launches() for ln in launches for c in ln["cases"]]


def without_twins(c):
    """the fp32-operand launch of the same descriptor"""
    return dict(c, twins=False)


def describe(c):
    keys = ("a_off", "y_off", "w_off", "a16_off", "y16_off")
    extra = " ".join("%s=%s" % (k, c[k]) for k in keys if c[k])
    flags = " ".join(n for n, on in (("twins", c["twins"]), ("no-db", not c["db"]), ("norm-only", not c["dW"]), ("no-partials", not c["partials"])) if on)
    hp = " head_pack%s" % (c["head_pack"],) if c["head_pack"] else ""
    return "%s p%d M%d N%d K%d ld(%d,%d,%d)%s %s %s [%s] %s" % (c["group"], c["prec"], c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"], hp,
                                                          extra, flags, c["path"]["kind"], c["note"])


OPERANDS = ("A", "dY", "dW", "db", "A16", "dY16")
_OFFSET = dict(A="a_off", dY="y_off", dW="w_off", A16="a16_off", dY16="y16_off")


def descriptor(H, c, ptr):
    """the air_wgrad_t (H.Wgrad of air/_hip.py) of a case; ptr: operand name -> address of a 256-byte aligned allocation whose
    first logical element lies the case's byte offset further.  The CPU table check and the GPU test both build their launches
    here, so they are the same descriptors."""
    g = H.Wgrad()
    g.A, g.dY = ptr["A"] + c["a_off"], ptr["dY"] + c["y_off"]
    if c["dW"]:
        g.dW = ptr["dW"] + c["w_off"]
    if c["db"]:
        g.db = ptr["db"]
    if c["twins"]:
        g.A16, g.dY16 = ptr["A16"] + c["a16_off"], ptr["dY16"] + c["y16_off"]
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"]
    if c["head_pack"]:
        g.head_pack, (g.Hs, g.Hh, g.Hz) = 1, c["head_pack"]
    return g


# ---- air_colsum, air_heads_out_wgrad ----------------------------------------------------------------------------------------
COLSUM_ROWS = [1, 3, 4, 5, 28, 29, 32, 33, 61, 192]           # 4 waves on interleaved rows; the 8-deep unroll runs while r + 28 < rows
COLSUM_COLS = [1, 63, 64, 65, 130]
COLSUM_MAX = 16                                               # problems of one air_colsum launch


def colsum_cases():
    """dict(rows, cols, ld, accumulate)"""
    return [dict(rows=r, cols=c, ld=c + pad, accumulate=acc) for r in COLSUM_ROWS for c in COLSUM_COLS for pad in (0, 3) for acc in (0, 1)]


def colsum_launches():
    """<= 16 problems each, consecutive cases dealt round-robin so that every launch mixes widths (workgroups past a narrow
    problem's columns return early); the first launch: 16 problems with a width of every kind"""
    cases = colsum_cases()
    n = -(-len(cases) // COLSUM_MAX)
    out = [cases[i::n] for i in range(n)]
    assert all(len({c["cols"] for c in ln}) >= 3 for ln in out) and len(out[0]) == COLSUM_MAX
    return out


HEADS_ROWS = [1, 5, 29, 33, 192, 200]


def heads_out_cases():
    """dict(hp, rows, ld): air_heads_out_wgrad at the three width triples"""
    return [dict(hp=hp, rows=r, ld=max(hp) + pad) for hp in HEAD_WIDTHS for r in HEADS_ROWS for pad in (0, 3)]
