"""Times the multi-channel spatial transformer (air_transformer_nc_fwd / air_transformer_nc_bwd, both gradients) against what
a caller had to do without it: C launches of the single-channel entry points on contiguous per-channel copies, the copies
(and the copy of the gradient planes back into [B,H,W,C]) included.  200 back-to-back calls between two device events
after a warm-up, three repeats alternating the two versions; prints one line per shape with the median of the repeats.
    python tools/bench_transformer_channels.py [B]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch
from air import _hip as H

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
lib = H.lib()


def timeit(fn, n=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def shape(Hi, Wi, Ho, Wo, Ch):
    g = torch.Generator(device="cuda").manual_seed(Hi + Ch)
    U = torch.rand(B, Hi, Wi, Ch, device="cuda", generator=g)
    th = torch.tensor([[0.55, 0.25, 0.3], [-0.2, 0.6, -0.4]], device="cuda").repeat(B, 1, 1) + 0.15 * torch.randn(B, 2, 3, device="cuda", generator=g)
    th = th.reshape(B, 6).contiguous()
    d = torch.randn(B, Ho, Wo, Ch, device="cuda", generator=g)
    out, dU, dth = torch.empty(B, Ho, Wo, Ch, device="cuda"), torch.empty_like(U), torch.empty(B, 6, device="cuda")
    o1, dU1, dth1 = torch.empty(B, Ho, Wo, device="cuda"), torch.empty(B, Hi, Wi, device="cuda"), torch.empty(B, 6, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        H.check(lib.air_transformer_nc_fwd(p(U), p(th), p(out), B, 1, Hi, Wi, Ch, Ho, Wo, s))

    def bwd():
        H.check(lib.air_transformer_nc_bwd(p(U), p(th), p(d), p(dU), p(dth), B, 1, Hi, Wi, Ch, Ho, Wo, s))

    def fwd_planes():
        for c in range(Ch):
            plane = U[..., c].contiguous()
            H.check(lib.air_transformer_fwd(p(plane), p(th), p(o1), B, Hi, Wi, Ho, Wo, s))
            out[..., c] = o1

    def bwd_planes():
        dth.zero_()
        for c in range(Ch):
            plane, gp = U[..., c].contiguous(), d[..., c].contiguous()
            H.check(lib.air_transformer_bwd(p(plane), p(th), p(gp), p(dU1), p(dth1), B, Hi, Wi, Ho, Wo, s))
            dU[..., c] = dU1
            dth.add_(dth1)

    U0, g0 = U[..., 0].contiguous(), d[..., 0].contiguous()

    def one_plane_bwd():                     # ONE single-channel backward, no copies
        H.check(lib.air_transformer_bwd(p(U0), p(th), p(g0), p(dU1), p(dth1), B, Hi, Wi, Ho, Wo, s))

    res = {k: [] for k in ("fwd", "fwd_planes", "bwd", "bwd_planes", "one_plane_bwd")}
    for _ in range(3):
        for k, fn in (("fwd", fwd), ("fwd_planes", fwd_planes), ("bwd", bwd), ("bwd_planes", bwd_planes), ("one_plane_bwd", one_plane_bwd)):
            res[k].append(timeit(fn))
    med = {k: sorted(v)[1] for k, v in res.items()}
    spread = max((max(v) - min(v)) / sorted(v)[1] for v in res.values())
    print("B=%d %dx%d -> %dx%d C=%d: forward %.1f us (per-plane calls %.1f), backward %.1f us (per-plane calls %.1f; one "
          "single-channel backward %.1f); largest spread over 3 repeats %.0f%%" %
          (B, Hi, Wi, Ho, Wo, Ch, med["fwd"], med["fwd_planes"], med["bwd"], med["bwd_planes"], med["one_plane_bwd"], 100 * spread), flush=True)


for Ch in (3, 8):
    shape(50, 50, 28, 28, Ch)
    shape(28, 28, 50, 50, Ch)
