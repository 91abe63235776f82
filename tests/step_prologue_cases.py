"""Case table of the carried step prologue in tests/test_gpu_step_prologue.py: one air_gemm descriptor per way a kernel family
carries an air_step_job_t (air_gemm_t.step_job), at the smallest shapes that reach it, and the jobs each one carries
(pure Python: no torch, no GPU).

A carrier is a case dict of tests/gemm_edge_cases.py (the descriptors are the edge tables' own, built by the same functions)
with three more keys:
  carrier   its name in the table of DESIGN.md
  name      the kernel air_gemm_kernel_name reports for the descriptor WITHOUT a job
  job_name  ... and WITH one (differs where the job switches the four-unit fp32 LSTM kernel off)
  wraps     whether the largest job of JOBS has more quads than the carrier's job planes have threads
The two AIR_EPI_LSTM_FWD0 carriers (group 'fwd0': the hoisted x.Wx of the train step, the launch that carries the job in
the model) are not in the edge tables; their descriptor is the one of tests/test_gpu_xwx_twin.py.

tests/test_step_prologue_cases.py checks on the CPU, through air_gemm_kernel_name, that every carrier reaches the kernel it
names with and without a job, and -- by restating plan_gemm's sizing of the job's planes -- that the largest job wraps the
grid-stride loop on every carrier."""
import re

import gemm_edge_cases as gec

EPI_LSTM_FWD0 = 6
PADDED = 2                                     # air_gemm_t.i0 of AIR_EPI_LSTM_FWD0: A16 is the padded twin, lda its stride

# (n_normal, n_uniform, twin_n): schedules only; tails on every plane; 12 501 + 5 001 + 2 502 = 20 004 quads, more than the
# 16 384 that cap x workgroups x 256 covers on these grids (16 planes of 4 workgroups; 64 planes of 1 on the throughput tile)
JOBS = [("schedules", 0, 0, 0), ("tails", 5, 3, 7), ("wraps", 50001, 20003, 10007)]


def _fwd0(carrier, M, R, K, **kw):
    """AIR_EPI_LSTM_FWD0 at precision 1 with the gate-interleaved panel twin of B: N = 4R, four-unit tiles, one K slab"""
    c = dict(group="fwd0", family=None, tile=(0, 0), ktile=(1, 1), layout="nn", ta=0, tb=0, prec=1, M=M, N=4 * R, K=K, R=R,
             lda=K, ldb=4 * R, ldc=4 * R, epi=EPI_LSTM_FWD0, i0=0, A16=False, B16=False, B16p=True, C16=False, ksplit=0, carrier=carrier)
    c.update(kw)
    return c


def _carriers():
    out = []

    def add(carrier, name, job_name, c):
        out.append(dict(dict(wraps=True), **dict(c, carrier=carrier, name=name, job_name=job_name or name)))

    for prec, fam in ((0, "f32"), (1, "bf16")):
        # the fallback kernels: an odd K (and lda) keeps the lean ones away
        add("%s fallback 1x1 K65" % fam, "gemm_%s_kernel<1, 1, false, false>" % fam, None,
            gec._case("plain", fam, (1, 1), "nn", prec, 17, 18, 65, (3, 2, 2)))
        # the lean kernels: both tiles, both layouts, K = 66 (one round and a 2-deep tail)
        for tile in ((1, 1), (2, 2)):
            for layout in ("nn", "nt"):
                add("%sv2 lean %dx%d %s K66" % (fam, tile[0], tile[1], layout),
                    "gemm_%sv2_kernel<%d, %d, %s, 0>" % (fam, tile[0], tile[1], "true" if layout == "nt" else "false"), None,
                    gec._case("plain", fam + "v2", tile, layout, prec, 16 * tile[0] + 1, 16 * tile[1] + 2, 66, (4, 4, 2)))
        # split-K: 4 slabs of 20, 20, 20 and 6 behind the job's planes
        add("%sv2 lean 1x1 split-K (66, 4)" % fam, "gemm_%sv2_kernel<1, 1, false, 0>" % fam, None,
            gec._case("splitk", fam + "v2", (1, 1), "nn", prec, 17, 18, 66, (4, 4, 2), ksplit=4))
    # the twin kernels: a generic product with both twins ...
    add("bf16tw 1x1 A16 B16 K64", "gemm_bf16tw_kernel<1, 1, false, 0, false, 4>", None,
        gec._case("plain", "bf16tw", (1, 1), "nn", 1, 17, 24, 64, (8, 8, 2), A16=True, B16=True, launches=2))
    # ... and the four-unit LSTM forward, whose grid.x is widened AFTER the job's planes were sized (plan_gemm rescales them)
    add("bf16tw four-unit AIR_EPI_LSTM_FWD", "gemm_bf16tw_kernel<1, 1, false, 100, false, 4>", None,
        gec._fused(gec.EPI_LSTM_FWD, "bf16tw", (1, 1), gec.EPI_LSTM_FWD_Q, "nn", 1, 17, 96, 24, (8, 8, 2), R=24, addend_slabs=4, q2_16=True,
                   A16=True, B16=True, launches=2))
    # fp32 lean AIR_EPI_LSTM_FWD: four-unit tiles without a job, the grouped 64-column tile with one
    add("f32v2 AIR_EPI_LSTM_FWD (job: no four-unit tiles)", "gemm_f32v2_kernel<1, 1, false, 100>", "gemm_f32v2_kernel<1, 4, false, 1>",
        gec._fused(gec.EPI_LSTM_FWD, "f32v2", (1, 1), gec.EPI_LSTM_FWD_Q, "nn", 0, 17, 80, 20, (2, 4, 2), R=20, addend_slabs=3, q2_16=True))
    # the hoisted x.Wx + first LSTM step: the fp32-A twin kernel that WRITES the padded twin of the batch (the carrier of a
    # model's first captured step), then the LDS-DMA kernel that reads it (the carrier of the later ones)
    add("bf16tw fp32-A AIR_EPI_LSTM_FWD0 (writes C16)", "gemm_bf16tw_kernel<1, 1, false, 6, true, 16>", None,
        _fwd0("fwd0-af32", 17, 8, 20, C16=True))
    add("xwx_glds padded A16 AIR_EPI_LSTM_FWD0", "gemm_xwx_glds_kernel<16>", None,
        _fwd0("fwd0-glds", 17, 8, 20, A16=True, lda=24, i0=PADDED))
    # the throughput tile: job planes LAST; 2 slabs (the pair map: 2 pairs, no remap) and 8 slabs (the slab-per-XCD map)
    for K, ks in ((128, 2), (512, 8)):
        add("xw_tp 64x64x%d ksplit %d" % (K, ks), "gemm_xw_tp_kernel<64>", None,
            gec._case("splitk", "xw_tp", (8, 4), "nn", 1, 64, 64, K, (4, 8, 2), B16=True, ksplit=ks))
    # ... and a 2 x 2 grid of its tiles: on a single tile the blockIdx.x / blockIdx.y terms of the job's workgroup index are 0
    # whatever their factors.  (20 planes of 4 workgroups hold the largest job in one pass: `wraps` False, this one alone.)
    add("xw_tp 128x128x128 ksplit 2", "gemm_xw_tp_kernel<64>", None,
        dict(gec._case("splitk", "xw_tp", (8, 4), "nn", 1, 128, 128, 128, (4, 8, 2), B16=True, ksplit=2), wraps=False))
    return out


CARRIERS = _carriers()


def carrier_id(c):
    return re.sub(r"[^A-Za-z0-9]+", "_", c["carrier"]).strip("_")


def operands(c):
    if c["group"] != "fwd0":
        return gec.operands(c)
    return ["A", "B", "C", "bias", "q0", "q1", "q2", "q2_16", "B16p"] + [k for k in ("A16", "C16") if c[k]]


def descriptor(H, c, ptr):
    """the air_gemm_t of a carrier, without a job (the caller sets step_job)"""
    if c["group"] != "fwd0":
        return gec.descriptor(H, c, ptr)
    g = H.Gemm()
    for name in operands(c):
        setattr(g, name, ptr[name])
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"]
    g.precision, g.epi, g.i0 = 1, EPI_LSTM_FWD0, c["i0"]
    return g


def job_quads(job):
    _, nn, nu, nt = job
    return (nn + 3) // 4 + (nu + 3) // 4 + (nt + 3) // 4


def job_grid_xy(c, with_job_name):
    """(grid.x, grid.y) of carrier c as plan_gemm launches it with a job"""
    return _grid(c, with_job_name)[1:]


def _grid(c, with_job_name):
    """(cap, grid.x when the job's planes are sized, grid.x and grid.y of the launch)"""
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    if tuple(c["tile"]) == (8, 4):
        gx, gy = c["N"] // 64, c["M"] // 64                                # (64-column tiles: far from 256 workgroups)
        return 64, gx, gx, gy
    e = c["epi"]
    tm, tn = {gec.EPI_LSTM_FWD: (1, 4), EPI_LSTM_FWD0: (1, 1)}.get(e, tuple(c["tile"]))
    grouped = e in (gec.EPI_LSTM_FWD, EPI_LSTM_FWD0)
    ncols = c["R"] if grouped else c["N"]
    tile_cols = 4 if e == EPI_LSTM_FWD0 else (16 if grouped else 16 * tn)
    gx, gy = ceil(ncols, tile_cols), ceil(c["M"], 16 * tm)
    four_unit = e == gec.EPI_LSTM_FWD and ", 100" in with_job_name       # grid.x widens AFTER the planes were sized
    return 16, gx, ceil(c["R"], 4) if four_unit else gx, gy


def job_grid(c, job, with_job_name):
    """(planes, workgroups per plane) of the job on carrier c: job_planes and the four-unit rescale of plan_gemm, restated"""
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    cap, gx0, gx, gy = _grid(c, with_job_name)
    planes = min(max(ceil(job_quads(job), gx0 * gy * 256), 1), cap)
    if gx != gx0:
        planes = ceil(planes * gx0, gx)                                   # the same number of workgroups on the wider grid
    return planes, gx * gy
