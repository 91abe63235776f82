"""CPU checks of tests/step_prologue_cases.py, the carriers of tests/test_gpu_step_prologue.py: air_gemm_kernel_name is
host-only code, so with made-up pointers every carrier is asked which kernel it launches, without and with a step job."""
import ctypes as C

import gemm_edge_cases as gec
import step_prologue_cases as spc
from air import _hip as H

BASE = 1 << 20
FAMILIES = ("f32", "bf16", "f32v2", "bf16v2", "bf16tw", "xwx_glds", "xw_tp")       # the seven that branch on Args::job_on


def _name(c, job=None):
    names = ("A", "B", "C", "bias", "addend", "aux", "p0", "p1", "p2", "p3", "q0", "q1", "q2", "A16", "B16", "C16", "q0_16", "q2_16", "B16p")
    g = spc.descriptor(H, c, {n: BASE * (i + 1) for i, n in enumerate(names)})
    if job is not None:
        _, nn, nu, nt = job
        sj = H.StepJob(sched=30 * BASE, nsched=5, dyn=31 * BASE, istate=32 * BASE, normals=33 * BASE, n_normal=nn,
                       uniforms=34 * BASE, n_uniform=nu, seed=1, twin_src=35 * BASE, twin_dst=36 * BASE, twin_n=nt)
        g.step_job = C.pointer(sj)
    buf = C.create_string_buffer(128)
    rc = H.lib().air_gemm_kernel_name(C.byref(g), buf, 128)
    assert rc == 0, (rc, c["carrier"])
    return buf.value.decode()


def _family(name):
    return name[len("gemm_"):name.index("_kernel")]


def test_every_carrier_reaches_the_kernel_it_names_with_and_without_a_job():
    for c in spc.CARRIERS:
        assert _name(c) == c["name"], c["carrier"]
        for job in spc.JOBS:
            assert _name(c, job) == c["job_name"], (c["carrier"], job[0])
        if c["family"] is not None:
            assert _family(c["name"]) == c["family"], c["carrier"]
    # the twin cases' fp32-operand form (launched by the edge tests' runner next to the twin one) is a lean kernel, job or not
    for c in spc.CARRIERS:
        if c["family"] == "bf16tw":
            plain = dict(c, A16=False, B16=False, B16p=False)
            assert _family(_name(plain)) == "bf16v2" and _family(_name(plain, spc.JOBS[2])) == "bf16v2", c["carrier"]


def test_the_carriers_cover_every_family_that_branches_on_the_job():
    with_job = {_family(c["job_name"]) for c in spc.CARRIERS}
    assert with_job == set(FAMILIES), sorted(with_job)
    names = {c["job_name"] for c in spc.CARRIERS}
    # both lean tiles in both layouts, at both precisions
    for fam in ("f32v2", "bf16v2"):
        for tile in ("1, 1", "2, 2"):
            for tb in ("false", "true"):
                assert "gemm_%s_kernel<%s, %s, 0>" % (fam, tile, tb) in names
    # split-K behind the job's planes: lean and throughput; the 8-slab throughput arm
    assert {(_family(c["name"]), c["K"], c["ksplit"]) for c in spc.CARRIERS if c["ksplit"] > 1} == \
        {("f32v2", 66, 4), ("bf16v2", 66, 4), ("xw_tp", 128, 2), ("xw_tp", 512, 8)}
    assert [c["carrier"] for c in spc.CARRIERS if not c["wraps"]] == ["xw_tp 128x128x128 ksplit 2"]
    # every family's job index has non-zero blockIdx.x and blockIdx.y terms somewhere: a grid of at least 2 x 2
    for fam in FAMILIES:
        assert any(_family(c["job_name"]) == fam and min(spc.job_grid_xy(c, c["job_name"])) >= 2 for c in spc.CARRIERS), fam
    assert all(gec.gemm_slabs(c["K"], c["ksplit"]) == c["ksplit"] for c in spc.CARRIERS if c["ksplit"] > 1)
    # the job changes the kernel of exactly one carrier: the fp32 four-unit LSTM forward
    assert [c["carrier"] for c in spc.CARRIERS if c["name"] != c["job_name"]] == ["f32v2 AIR_EPI_LSTM_FWD (job: no four-unit tiles)"]
    # the four-unit rescale of the job's planes is reached with a widened grid
    c = next(c for c in spc.CARRIERS if c["carrier"] == "bf16tw four-unit AIR_EPI_LSTM_FWD")
    assert spc.job_grid(c, spc.JOBS[2], c["job_name"]) == (6, 12)          # 16 planes of 4 workgroups -> 6 of 12


def test_the_largest_job_wraps_the_grid_stride_loop_on_every_carrier():
    jobs = {j[0]: j for j in spc.JOBS}
    assert spc.job_quads(jobs["wraps"]) == 20004 and spc.job_quads(jobs["tails"]) == 5 and spc.job_quads(jobs["schedules"]) == 0
    for c in spc.CARRIERS:
        planes, wgs = spc.job_grid(c, jobs["wraps"], c["job_name"])
        assert (planes * wgs * 256 < 20004) == c["wraps"], (c["carrier"], planes, wgs)
        assert planes * wgs > 1                                          # ... on more than one workgroup
        # the small jobs get one plane, most of whose workgroups find nothing to do
        assert spc.job_grid(c, jobs["tails"], c["job_name"])[0] == 1 and spc.job_grid(c, jobs["schedules"], c["job_name"])[0] == 1


if __name__ == "__main__":
    print("| carrier | kernel without a job | kernel with a job | planes x workgroups of the largest job |\n|---|---|---|---|")
    for c in spc.CARRIERS:
        p, w = spc.job_grid(c, spc.JOBS[2], c["job_name"])
        print("| %s | `%s` | `%s` | %d x %d |" % (c["carrier"], _name(c), _name(c, spc.JOBS[2]), p, w))
