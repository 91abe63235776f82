"""Case tables of tests/test_gpu_gemm_edges.py: air_gemm descriptors at tile edges, with padded leading dimensions and offset
base pointers, for every kernel family the dispatch of air_gemm.hip reaches (pure Python: no torch, no GPU).

A case is a plain dict:
  group    'plain' | 'splitk' | 'epi' | 'fused'
  family   'bf16v2' | 'f32v2' (lean) | 'bf16' | 'f32' (fallback) | 'bf16tw' (twin): the kernel it is written for,
  ktile    the kernel's tile template arguments, kepi its epilogue template argument (None: fallback, chosen at run time)
  tile     air_gemm_t.tile_m / tile_n; ta / tb; prec; M, N, K; lda, ldb, ldc, ldadd, ldaux (all strictly wider than the
           logical rows); a_off / b_off: byte offsets of the A / B base pointers from a 256-byte aligned allocation
  A16 / B16 / B16p  which bf16 twins the launch is given; ksplit; epi and its operands (see the generators)
  launches how many kernel launches the GPU test spends on it (the twin cases also run the fp32-operand form)

Star design: the base shape of a tile (TM, TN) is (BM + 1, BN + 2, 66) with BM = 16 TM, BN = 16 TN; every dimension is varied
alone through its list, then three corners (all minima, all maxima, (1, base N, largest K)).  tests/test_gemm_edge_cases.py
checks on the CPU, through air_gemm_kernel_name, that every case reaches the kernel it names."""

TILES = [(1, 1), (1, 2), (1, 4), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4)]
EPI_GENERIC, EPI_LSTM_FWD, EPI_REPARAM_FWD, EPI_LSTM_BWD, EPI_REPARAM_BWD, EPI_LSTM_BWD_TAIL = 0, 1, 2, 3, 4, 5
EPI_LSTM_FWD_Q = 100                       # the kernels' internal id of AIR_EPI_LSTM_FWD on four-unit tiles (air_gemm_common.h)
LAYOUTS = {"nn": (0, 0), "nt": (0, 1), "tn": (1, 0)}

LEAN_K = [2, 6, 30, 62, 64, 66, 126, 130, 254, 258, 510, 514, 1030]       # every round depth R * 64, R in 1 2 4 8 16, -+ 8 bytes
FALLBACK_K = [1, 3, 5, 63, 65, 127, 129, 1025]
TWIN_K = [8, 56, 64, 72, 248, 264, 504, 520, 1016, 1032, 2056]
TWIN_K_F32A = [4, 60, 64, 68, 252, 260, 508, 516, 1020, 1028, 2052]      # the multiples of 4 next to them (fp32 A)
SPLITK = [(10, 8), (66, 4), (200, 3), (1030, 4)]                            # (K, ksplit); (10, 8) gives 3 slabs, not 8
SPLITK_TWIN_A = [(88, 3)]          # none of those leaves K-slabs of whole 8s, which a twin A needs: slabs of 32, 32 and a short 24
EPI_TILES = [(1, 1), (2, 4), (4, 2)]
# keyword sets of test_gemm_epilogues + addend slabs + a C16 twin
EPI_SETS = ["bias", "bias_relu", "bias_softplus", "bias_sigmoid_noise", "addend", "grad_relu", "grad_softplus", "bias_accumulate",
            "addend_slabs2", "addend_slabs8", "bias_softplus_c16"]


def gemm_slabs(K, ksplit):
    """air_gemm_slabs, restated"""
    ks = max(ksplit, 1)
    kslab = ((K + ks - 1) // ks + 3) & ~3
    return (K + kslab - 1) // kslab


def lean_arms(c):
    """(HA, HB) of k_loop in the lean kernels: the a8 / b8 expressions of gemm_bf16v2_kernel / gemm_f32v2_kernel for a
    generic (ungrouped) launch.  A half arm reads its 16 bytes as two 8-byte pieces with a mask each."""
    a8 = not (c["lda"] % 4 == 0 and c["a_off"] % 16 == 0 and c["K"] % 4 == 0)
    b8 = not (c["ldb"] % 4 == 0 and c["b_off"] % 16 == 0 and (c["K"] % 4 == 0 if c["tb"] else c["N"] % 4 == 0))
    return a8, b8


def tile_count(c):
    """workgroups of the (x, y) grid: what xcd_tile remaps"""
    tm, tn = c["ktile"]
    return -(-c["M"] // (16 * tm)) * -(-c["N"] // (16 * tn))


def _case(group, family, tile, layout, prec, M, N, K, pads, **kw):
    ta, tb = LAYOUTS[layout]
    pa, pb, pc = pads
    c = dict(group=group, family=family, tile=tile, ktile=tile, kepi=None if family in ("bf16", "f32") else 0, layout=layout,
             ta=ta, tb=tb, prec=prec, M=M, N=N, K=K, lda=(M if ta else K) + pa, ldb=(K if tb else N) + pb, ldc=N + pc,
             ldadd=N + pc, ldaux=N + pc + (1 if family in ("bf16", "f32") else 2), a_off=0, b_off=0, A16=False, B16=False,
             B16p=False, ksplit=0, epi=EPI_GENERIC, kw=None, launches=1)
    c.update(kw)
    return c


def _star(base, lists, corners=True):
    """vary each dimension of `base` = (M, N, K) alone through its list, then the three corners; no duplicates, order kept"""
    out = [base]
    for axis, vals in enumerate(lists):
        for v in vals:
            s = list(base)
            s[axis] = v
            out.append(tuple(s))
    if corners:
        out.append(tuple(min(v) for v in lists))
        out.append(tuple(max(v) for v in lists))
        out.append((1, base[1], max(lists[2])))
    seen, uniq = set(), []
    for s in out:
        if s not in seen and min(s) > 0:
            seen.add(s)
            uniq.append(s)
    return uniq


def lean_cases(tile, layout, prec):
    """gemm_bf16v2_kernel / gemm_f32v2_kernel: even K and leading dimensions, 8-byte aligned operands, NN with an even N"""
    tm, tn = tile
    BM, BN = 16 * tm, 16 * tn
    fam = "bf16v2" if prec else "f32v2"
    Ns = [2, BN - 2, BN, BN + 2, 2 * BN + 6] + ([1, BN - 1, BN + 1] if layout == "nt" else [])
    shapes = _star((BM + 1, BN + 2, 66), ([1, BM - 1, BM, BM + 1, 2 * BM + 3], Ns, LEAN_K))
    # pads + 4: the leading dimensions keep the residue mod 4 of the widths, so the arms follow from K and N
    out = [_case("plain", fam, tile, layout, prec, M, N, K, (4, 4, 2)) for M, N, K in shapes]
    # the four k_loop(HA, HB) arms, each reached through each condition of a8 / b8: shape (BM + 1, BN + 4, 64) takes the
    # full 16-byte loads on both operands; one change at a time sends A, B or both to the 8-byte halves
    M, N, K = BM + 1, BN + 4, 64
    for pa in (4, 2):
        for pb in (4, 2):
            out.append(_case("plain", fam, tile, layout, prec, M, N, K, (pa, pb, 2), arm="ld%d%d" % (pa, pb)))
    # ... and a small star of its own for that full arm, the one every launch of the train step takes: no shape of the lists
    # above has K, N and both leading dimensions all multiples of 4
    for Mf, Nf, Kf in _star((M, N, K), ([1, BM - 1], [4, BN - 4, 2 * BN + 8], [4, 60, 68, 252, 260, 1028]), corners=False)[1:]:
        out.append(_case("plain", fam, tile, layout, prec, Mf, Nf, Kf, (4, 4, 2), arm="full"))
    out.append(_case("plain", fam, tile, layout, prec, M, N, 66, (2, 4, 2), arm="K%4"))             # lda % 4 == 0, K % 4 == 2
    # (the fp32 lean kernel reads k-runs of 8 as two 16-byte pieces: with halves, K = 4 mod 8 ends inside the FIRST piece)
    for Kh in (60, 68):
        out.append(_case("plain", fam, tile, layout, prec, M, N, Kh, (2, 2, 2), arm="half K%8"))
    out.append(_case("plain", fam, tile, layout, prec, M, N, K, (4, 4, 2), a_off=8, arm="A+8"))
    out.append(_case("plain", fam, tile, layout, prec, M, N, K, (4, 4, 2), b_off=8, arm="B+8"))
    if layout == "nn":
        out.append(_case("plain", fam, tile, layout, prec, M, BN + 2, K, (4, 2, 2), arm="N%4"))        # ldb % 4 == 0, N % 4 == 2
    return out


def fallback_cases(tile, layout, prec):
    """gemm_bf16_kernel / gemm_f32_kernel: odd K, an odd leading dimension, a 4-byte aligned operand or a transposed A"""
    tm, tn = tile
    BM, BN = 16 * tm, 16 * tn
    fam = "bf16" if prec else "f32"
    # (at the base depth 66 it is the odd lda that keeps the lean kernels away, along the K list the odd K)
    # (2 BM + 3 and 2 BN + 5: three tiles a side, so that these families too see a 3 x 2 and a 9-workgroup grid)
    shapes = _star((BM + 1, BN + 2, 66), ([1, BM - 1, BM, BM + 1, 2 * BM + 3], [1, BN - 1, BN, BN + 1, 2 * BN + 5], FALLBACK_K))
    out = [_case("plain", fam, tile, layout, prec, M, N, K, (3, 1, 5)) for M, N, K in shapes]
    # each way into these kernels alone, everything else as the lean kernels want it
    M, N = BM + 1, BN + 2
    if layout == "tn":
        out.append(_case("plain", fam, tile, layout, prec, M + 1, N, 66, (2, 2, 2), trigger="transA"))
    else:
        out.append(_case("plain", fam, tile, layout, prec, M, N, 65, (3, 2, 2) if layout == "nn" else (3, 3, 2), trigger="odd K"))
        out.append(_case("plain", fam, tile, layout, prec, M, N, 66, (3, 2, 2), trigger="odd lda"))
        out.append(_case("plain", fam, tile, layout, prec, M, N, 66, (2, 2, 2), a_off=4, trigger="A+4"))
        out.append(_case("plain", fam, tile, layout, prec, M, N, 66, (2, 2, 2), b_off=4, trigger="B+4"))
    return out


# (tile, layout, A as a bf16 twin?, B as the panel twin?): exactly what twin_rounds admits for the generic epilogue,
# + the fp32-A forms of the 64-row tiles (the split-K x.Wx of large canvases runs them)
TWIN_COMBOS = [((1, 1), "nn", True, False), ((1, 1), "nn", True, True), ((1, 1), "nt", True, False),
               ((2, 2), "nn", True, False), ((2, 2), "nn", True, True), ((2, 2), "nt", True, False),
               ((2, 2), "nn", False, False), ((2, 2), "nn", False, True),
               ((4, 2), "nn", True, False), ((4, 4), "nn", True, False), ((4, 2), "nn", False, False), ((4, 4), "nn", False, False)]


def twin_cases(tile, layout, a16, panel):
    """gemm_bf16tw_kernel: whole 16-byte pieces of bf16 (K, N and the leading dimensions multiples of 8; 4 for an fp32 A)"""
    tm, tn = tile
    BM, BN = 16 * tm, 16 * tn
    Ns = [8, BN - 8, BN + 8, 2 * BN + 8] + ([1, BN - 1, BN + 1] if layout == "nt" else [])
    Ks = TWIN_K if (a16 or layout == "nt") else TWIN_K_F32A
    shapes = _star((BM + 1, BN + 8, 72), ([1, BM - 1, BM + 1, 2 * BM + 3], Ns, Ks))
    return [_case("plain", "bf16tw", tile, layout, 1, M, N, K, (8 if a16 else 4, 8, 2), A16=a16, B16=not panel, B16p=panel, launches=2)
            for M, N, K in shapes]


def splitk_cases():
    out = []
    for tile in ((1, 1), (2, 2), (4, 2)):
        BM, BN = 16 * tile[0], 16 * tile[1]
        for K, ks in SPLITK + SPLITK_TWIN_A:
            for prec in (0, 1):
                for layout in ("nn", "nt"):
                    out.append(_case("splitk", "bf16v2" if prec else "f32v2", tile, layout, prec, BM + 1, BN + 2, K, (4, 4, 2), ksplit=ks))
            # twins: an fp32 A (K % 4 == 0 and a K-slab of whole 4s always holds) with a row-major B16; (1, 1) has no fp32-A form
            if K % 4 == 0 and tile != (1, 1):
                out.append(_case("splitk", "bf16tw", tile, "nn", 1, BM + 1, BN + 8, K, (4, 8, 2), B16=True, ksplit=ks, launches=2))
            # ... and a twin A: K and the K-slab multiples of 8
            kslab = ((K + ks - 1) // ks + 3) & ~3
            if K % 8 == 0 and kslab % 8 == 0:
                out.append(_case("splitk", "bf16tw", tile, "nn", 1, BM + 1, BN + 8, K, (8, 8, 2), A16=True, B16=True, ksplit=ks, launches=2))
    return out


def epilogue_cases():
    """generic epilogues at the base shape of each family and layout; K <= 256 and B / 8 as in test_gemm_epilogues"""
    out = []
    for tile in EPI_TILES:
        BM, BN = 16 * tile[0], 16 * tile[1]
        for kw in EPI_SETS:
            for prec in (0, 1):
                for layout in ("nn", "nt"):
                    out.append(_case("epi", "bf16v2" if prec else "f32v2", tile, layout, prec, BM + 1, BN + 2, 66, (4, 4, 2), kw=kw))
                for layout in ("nn", "nt", "tn"):
                    out.append(_case("epi", "bf16" if prec else "f32", tile, layout, prec, BM + 1, BN + 2, 65, (3, 1, 5), kw=kw))
            if tile == (1, 1):
                out.append(_case("epi", "bf16tw", tile, "nn", 1, BM + 1, BN + 8, 72, (8, 8, 2), A16=True, B16=True, kw=kw, launches=2))
                out.append(_case("epi", "bf16tw", tile, "nt", 1, BM + 1, BN + 1, 72, (8, 8, 2), A16=True, B16=True, kw=kw, launches=2))
            if tile == (4, 2):
                out.append(_case("epi", "bf16tw", tile, "nn", 1, BM + 1, BN + 8, 72, (8, 8, 2), A16=True, B16=True, kw=kw, launches=2))
    return out


FUSED_M = [1, 17, 37]


def _fused(epi, family, ktile, kepi, layout, prec, M, N, K, pads, **kw):
    tile = {EPI_LSTM_FWD: (1, 4), EPI_REPARAM_FWD: (1, 2)}.get(epi, (1, 1))
    c = _case("fused", family, (0, 0), layout, prec, M, N, K, pads, epi=epi)
    c.update(ktile=ktile if family != "bf16" and family != "f32" else tile, kepi=kepi, ldc=N + pads[2], ldadd=N + max(pads[2], 2), ldaux=N + 3)
    if epi == EPI_REPARAM_BWD:
        c["ldc"] = 2 * N + 4
    c.update(kw)
    return c


def _fam(prec, lean):
    return ("bf16v2" if prec else "f32v2") if lean else ("bf16" if prec else "f32")


def fused_cases():
    out = []
    for prec in (0, 1):
        for M in FUSED_M:
            # ---- AIR_EPI_LSTM_FWD: N = 4R, K = R.  R = 3: odd, the fallback's run-time epilogue; 6: the grouped 64-column lean
            # tile; 20, 36: four-unit tiles at precision 0 (the lean bf16 kernel has the grouped tile only)
            for R in (3, 6, 20, 36):
                lean = R % 2 == 0
                quad = lean and prec == 0 and R % 4 == 0
                pads = (2, 4, 2) if lean else (3, 1, 3)
                slab_list = (None, 1, 3, 4, 8)
                for slabs in slab_list:
                    out.append(_fused(EPI_LSTM_FWD, _fam(prec, lean), (1, 1) if quad else (1, 4), None if not lean else (EPI_LSTM_FWD_Q if quad else 1),
                                      "nn", prec, M, 4 * R, R, pads, R=R, addend_slabs=slabs, q2_16=True))
            if prec == 1:
                for panel in (False, True):
                    out.append(_fused(EPI_LSTM_FWD, "bf16tw", (1, 1), EPI_LSTM_FWD_Q, "nn", 1, M, 96, 24, (8, 8, 2), R=24, addend_slabs=4, q2_16=True,
                                      A16=True, B16=not panel, B16p=panel, launches=2))
            # ---- AIR_EPI_REPARAM_FWD: N = 2Z, K = 64; an odd Z takes the fallback
            for Z in (1, 2, 9, 18, 50):
                lean = Z % 2 == 0
                out.append(_fused(EPI_REPARAM_FWD, _fam(prec, lean), (1, 2), None if not lean else 2, "nn", prec, M, 2 * Z, 64,
                                  (4, 2, 2) if lean else (4, 1, 3), Z=Z, q0_16=True))
            # ---- AIR_EPI_LSTM_BWD (NT): N = R, K = 4R.  B^T has k-contiguous rows, so an odd R still runs lean with even leading
            # dimensions; R = 3 is taken both ways (odd ones: the fallback)
            for R, lean in ((3, False), (3, True), (6, True), (20, True)):
                pads = (4, 4, 2) if lean else (3, 3, 2)
                base = dict(R=R, p3=True, q2="acc", addend=True, q0_16=True, q2_16=True)
                for var in (dict(), dict(p3=False), dict(q2=None, q2_16=False), dict(q2="store"), dict(addend=False, q0_16=False, q2_16=False)):
                    kw = dict(base)
                    kw.update(var)
                    out.append(_fused(EPI_LSTM_BWD, _fam(prec, lean), (1, 1), None if not lean else 3, "nt", prec, M, R, 4 * R, pads, **kw))
                if prec == 1 and R in (6, 20):
                    out.append(_fused(EPI_LSTM_BWD, "bf16tw", (1, 1), 3, "nt", 1, M, R, 4 * R, (8, 8, 2), A16=True, B16=True, launches=2, **base))
            # ---- AIR_EPI_REPARAM_BWD (NT as the train step runs it): N = Z, ldc = 2Z + 4, C16 given
            for Z in (1, 2, 9, 50):
                for lean in ((True, False) if Z % 2 else (True,)):
                    out.append(_fused(EPI_REPARAM_BWD, _fam(prec, lean), (1, 1), None if not lean else 4, "nt", prec, M, Z, 64,
                                      (4, 4, 0) if lean else (4, 3, 0), Z=Z, C16=True))
        # ---- AIR_EPI_LSTM_BWD_TAIL: rows [0, i0) are plain stores into C, rows [i0, M) the cell backward on arrays of M - i0 rows
        for R in (6, 20):
            for i0 in (0, 5, 16, 37):
                out.append(_fused(EPI_LSTM_BWD_TAIL, _fam(prec, True), (1, 1), 5, "nt", prec, 37, R, 4 * R, (4, 4, 2), R=R, i0=i0, p3=False,
                                  q2="store", addend=False, q0_16=True, q2_16=False))
                if prec == 1 and i0 == 5:
                    out.append(_fused(EPI_LSTM_BWD_TAIL, "bf16tw", (1, 1), 5, "nt", 1, 37, R, 4 * R, (8, 8, 2), R=R, i0=i0, p3=False, q2="store",
                                      addend=False, q0_16=True, q2_16=False, A16=True, B16=True, launches=2))
    return out


def plain_groups():
    """[(id, cases)] of the plain-product tests: one entry per (family, tile, layout)"""
    out = []
    for tile in TILES:
        for prec in (0, 1):
            for layout in ("nn", "nt"):
                out.append(("%s-%dx%d-%s" % ("bf16v2" if prec else "f32v2", tile[0], tile[1], layout), lean_cases(tile, layout, prec)))
            for layout in ("nn", "nt", "tn"):
                out.append(("%s-%dx%d-%s" % ("bf16" if prec else "f32", tile[0], tile[1], layout), fallback_cases(tile, layout, prec)))
    for tile, layout, a16, panel in TWIN_COMBOS:
        out.append(("bf16tw-%dx%d-%s-%s-%s" % (tile[0], tile[1], layout, "A16" if a16 else "Af32", "B16p" if panel else "B16"),
                    twin_cases(tile, layout, a16, panel)))
    return out


def all_cases():
    out = []
    for _, cases in plain_groups():
        out += cases
    return out + splitk_cases() + epilogue_cases() + fused_cases()


def describe(c):
    """one line that names a failing case"""
    keys = ("arm", "trigger", "kw", "ksplit", "a_off", "b_off", "R", "Z", "i0", "addend_slabs", "p3", "q2", "A16", "B16p")
    extra = " ".join("%s=%s" % (k, c[k]) for k in keys if c.get(k) not in (None, 0, False))
    return "%s %s %dx%d %s p%d M%d N%d K%d ld(%d,%d,%d) %s" % (c["group"], c["family"], c["ktile"][0], c["ktile"][1], c["layout"], c["prec"],
                                                              c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"], extra)


# generic-epilogue keyword sets: bias / addend (slab count) / aux ('pos': in (0.01, 2), 'signed': that minus 1) / act / actgrad
EPI_KW = {
    "bias": dict(bias=1), "bias_relu": dict(bias=1, act=1), "bias_softplus": dict(bias=1, act=2),
    "bias_sigmoid_noise": dict(bias=1, act=3, aux="pos", aux_scale=0.3), "addend": dict(addend=1),
    "grad_relu": dict(actgrad=1, aux="signed"), "grad_softplus": dict(actgrad=2, aux="pos"),
    "bias_accumulate": dict(bias=1, accumulate=1), "addend_slabs2": dict(addend=2), "addend_slabs8": dict(addend=8),
    "bias_softplus_c16": dict(bias=1, act=2, C16=1),
}


def operands(c):
    """names of the air_gemm_t pointer fields the case passes"""
    names = ["A", "B", "C"] + [k for k in ("A16", "B16", "B16p") if c[k]]
    e = c["epi"]
    if e == EPI_GENERIC:
        kw = EPI_KW.get(c["kw"], {})
        names += [k for k in ("bias", "addend", "aux", "C16") if kw.get(k)]
    elif e == EPI_LSTM_FWD:
        names += ["bias", "p0", "q0", "q1", "q2"] + (["addend"] if c["addend_slabs"] else []) + (["q2_16"] if c["q2_16"] else [])
    elif e == EPI_REPARAM_FWD:
        names += ["bias", "p0", "q0", "q0_16"]
    elif e in (EPI_LSTM_BWD, EPI_LSTM_BWD_TAIL):
        names += ["p0", "p1", "p2", "q0", "q1"] + [k for k in ("p3", "addend", "q2", "q0_16", "q2_16") if c[k]]
    elif e == EPI_REPARAM_BWD:
        names += ["p0", "p1", "p2", "p3", "C16"]
    return names


def descriptor(H, c, ptr):
    """the air_gemm_t (H.Gemm of air/_hip.py) of a case; ptr: operand name -> address of its first logical element, before
    a_off / b_off.  The CPU table check and the GPU test build their launches here, so they are the same descriptors."""
    g = H.Gemm()
    for name in operands(c):
        setattr(g, name, ptr[name] + (c["a_off"] if name == "A" else c["b_off"] if name == "B" else 0))
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"]
    g.transA, g.transB, g.precision, g.epi = c["ta"], c["tb"], c["prec"], c["epi"]
    g.tile_m, g.tile_n = c["tile"]
    g.ksplit, g.ldadd, g.ldaux = c["ksplit"], c["ldadd"], c["ldaux"]
    e = c["epi"]
    if e == EPI_GENERIC:
        kw = EPI_KW.get(c["kw"], {})
        g.act, g.actgrad, g.accumulate, g.aux_scale = kw.get("act", 0), kw.get("actgrad", 0), kw.get("accumulate", 0), kw.get("aux_scale", 0.0)
        g.addend_slabs = kw.get("addend", 0) if kw.get("addend", 0) > 1 else 0
    elif e == EPI_LSTM_FWD:
        g.addend_slabs = c["addend_slabs"] or 0
    elif e == EPI_LSTM_BWD:
        g.i0 = 1 if c["q2"] == "acc" else 0
    elif e == EPI_LSTM_BWD_TAIL:
        g.i0 = c["i0"]
    return g


def parse_kernel_name(name):
    """'gemm_bf16v2_kernel<1, 4, false, 1>' -> ('bf16v2', (1, 4), ta, tb, epi or None)"""
    fam = name[len("gemm_"):name.index("_kernel")]
    args = [a.strip() for a in name[name.index("<") + 1:name.rindex(">")].split(",")]
    tile = (int(args[0]), int(args[1]))
    if fam in ("bf16", "f32"):
        return fam, tile, args[2] == "true", args[3] == "true", None
    return fam, tile, False, args[2] == "true", int(args[3])
