"""The six kernels of csrc/air_bottleneck.hip, launched on their own: bench.py's models run only the two bf16-twin instances.

  python tools/bench_bottleneck.py [M] [launches]

M (default 192) = rows of the bottleneck = batch x steps: 192 for configs[1] (64 x 3), 1280 for configs[3] (256 x 5);
Z = 50, H = K1 = 256, z in rows of 52 with the twin outputs written, as the train step calls them.  Each of the forms
(forward / backward x fp32 operands, bf16 twins, exact fp32) is launched `launches` (default 300) times back to back and
nothing else, so that a `rocprofv3 --kernel-trace --stats` run of this command (a process of its own;
tools/rocprof_summary.py) has exactly that many calls per kernel name.  Prints the HIP-event time per launch, which at
these sizes is the launch rate of an eager loop, not the kernel time."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch

from air import _hip as H

Z, K = 50, 256
LDZ = 52


def main(M, n):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    twin = lambda t: t.to(torch.bfloat16).view(torch.int16)  # noqa: E731
    p, lib, stream = H.ptr, H.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Wml, bml, eps, Wg, bg = rnd(M, K).abs(), rnd(K, 2 * Z) * 0.05, rnd(2 * Z) * 0.05, rnd(M, Z), rnd(Z, K) * 0.2, rnd(K) * 0.05
    dG, ml, x = rnd(M, K) * 0.1, rnd(M, 2 * Z) * 0.5, rnd(M, K).abs() + 0.01
    att = torch.zeros(M, H.ATT_STRIDE, device=dev)
    att[:, H.ATT_MASK] = 1.0
    dyn = torch.zeros(32, device=dev)
    dyn[H.DYN_GRAD_SCALE], dyn[H.DYN_VAE_PV], dyn[H.DYN_VAE_PM] = 1.0 / 64, 1.0, 0.0
    o_ml, o_z, o_g = torch.empty(M, 2 * Z, device=dev), torch.zeros(M, LDZ, device=dev), torch.empty(M, K, device=dev)
    o_z16, o_g16 = torch.zeros(M, LDZ, dtype=torch.int16, device=dev), torch.empty(M, K, dtype=torch.int16, device=dev)
    d_ml, d_x = torch.empty(M, 2 * Z, device=dev), torch.empty(M, K, device=dev)
    d_ml16, d_x16 = torch.empty(M, 2 * Z, dtype=torch.int16, device=dev), torch.empty(M, K, dtype=torch.int16, device=dev)
    X16, Wml16, Wg16, dG16 = twin(X), twin(Wml), twin(Wg), twin(dG)
    for form in ("fp32 operands", "bf16 twins", "exact fp32"):
        tw, ex = form == "bf16 twins", int(form == "exact fp32")
        f = H.BottleneckFwd(p(X), p(Wml), p(bml), p(eps), p(Wg), p(bg), p(o_ml), p(o_z), p(o_g), M, K, Z, K, K, p(o_z16), p(o_g16),
                            p(X16 if tw else None), p(Wml16 if tw else None), p(Wg16 if tw else None), ex, LDZ)
        b = H.BottleneckBwd(p(dG), p(Wg), p(ml), p(eps), p(att), p(dyn), p(Wml), p(x), p(d_ml), p(d_x), M, K, Z, K, p(d_ml16), p(d_x16),
                            p(dG16 if tw else None), p(Wg16 if tw else None), p(Wml16 if tw else None), ex)
        for name, fn, arg in (("forward", lib.air_vae_bottleneck_fwd, f), ("backward", lib.air_vae_bottleneck_bwd, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                H.check(fn(C.byref(arg), stream), name)
            e1.record()
            torch.cuda.synchronize()
            print("M = %4d  %-8s %-13s %7.2f us per launch (%d eager launches, HIP events)" % (M, name, form, e0.elapsed_time(e1) * 1e3 / n, n),
                  flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bench_bottleneck.py needs the GPU: a CPU run gives no time")
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    main(arg(1, 192), arg(2, 300))
