"""Times the fused CNN front-end (air.cnn: air_cnn_fwd, air_cnn_bwd) against the only thing a caller could do before it:
torch's own conv2d / relu / max_pool2d on the device, the same arithmetic (NCHW, fp32), forward and forward + backward of
sum(w * out) with gradients for the six variables (not for the images, as in the model).  200 back-to-back calls between
two device events after a warm-up, three repeats alternating the versions; prints the median of the repeats, the spread,
and one JSON line.
    python tools/bench_cnn.py [B [S [F]]]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch
import torch.nn.functional as TF
from air.cnn import CNN

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 50
F = int(sys.argv[3]) if len(sys.argv) > 3 else 8


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


g = torch.Generator(device="cuda").manual_seed(S + F)
m = CNN(S, F, device="cuda", seed=1)
x = torch.rand(B, S * S, device="cuda", generator=g)
w = torch.randn(B, m.output_dim, device="cuda", generator=g)
# the torch chain on its own copies of the variables, in the layout conv2d wants ([F, Cin, 5, 5])
tk = [k.detach().permute(3, 2, 0, 1).contiguous().requires_grad_(True) for k in (m.k1, m.k2, m.k3)]
tb = [b.detach().clone().requires_grad_(True) for b in (m.b1, m.b2, m.b3)]
x4 = x.view(B, 1, S, S)
w4 = w.view(B, S // 4, S // 4, F).permute(0, 3, 1, 2).contiguous()


def torch_chain():
    h = TF.max_pool2d(TF.relu(TF.conv2d(x4, tk[0], tb[0], padding=2)), 2, 2)
    h = TF.max_pool2d(TF.relu(TF.conv2d(h, tk[1], tb[1], padding=2)), 2, 2)
    return TF.relu(TF.conv2d(h, tk[2], tb[2], padding=2))


def hip_fwd():
    with torch.no_grad():
        m(x)


def torch_fwd():
    with torch.no_grad():
        torch_chain()


def hip_fwd_bwd():
    torch.autograd.grad((m(x) * w).sum(), list(m.parameters()))


def torch_fwd_bwd():
    torch.autograd.grad((torch_chain() * w4).sum(), tk + tb)


# the two entry points alone, on buffers made once: what the launches cost without the autograd plumbing around them
import ctypes as C
from air import _hip as H
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
S1, S2 = S // 2, S // 4
o = torch.empty(B, m.output_dim, device="cuda")
sv = [torch.empty(B, S1, S1, F, device="cuda"), torch.empty(B, S2, S2, F, device="cuda"),
      torch.empty(B, S1, S1, F, dtype=torch.uint8, device="cuda"), torch.empty(B, S2, S2, F, dtype=torch.uint8, device="cuda")]
V = [q.detach() for q in m._params()]
gr = [torch.empty_like(q) for q in V]
ws = torch.empty(H.lib().air_cnn_workspace_floats(B, S, F), device="cuda")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
fa = H.CnnFwd(p(x), *[p(q) for q in V], p(o), *[p(t) for t in sv], B, S, F)
ba = H.CnnBwd(p(w), p(o), p(x), *[p(t) for t in sv], p(V[0]), p(V[2]), p(V[4]), p(ws), *[p(t) for t in gr], None, B, S, F)


def abi_fwd():
    H.check(H.lib().air_cnn_fwd(C.byref(fa), st))


def abi_bwd():
    H.check(H.lib().air_cnn_bwd(C.byref(ba), st))


with torch.no_grad():
    ref = torch_chain().permute(0, 2, 3, 1).reshape(B, -1)
    err = float((m(x) - ref).abs().max() / ref.abs().max())
runs = (("hip_fwd", hip_fwd), ("torch_fwd", torch_fwd), ("hip_fwd_bwd", hip_fwd_bwd), ("torch_fwd_bwd", torch_fwd_bwd),
        ("abi_fwd", abi_fwd), ("abi_bwd", abi_bwd))
res = {k: [] for k, _ in runs}
for _ in range(3):
    for k, fn in runs:
        res[k].append(timeit(fn))
med = {k: sorted(v)[1] for k, v in res.items()}
spread = {k: (max(v) - min(v)) / sorted(v)[1] for k, v in res.items()}
print("B=%d S=%d F=%d: forward %.1f us fused, %.1f us torch chain; forward + backward %.1f us fused, %.1f us torch chain; "
      "the entry points alone: air_cnn_fwd %.1f us, air_cnn_bwd %.1f us; largest spread over 3 repeats %.0f%%; fused vs torch forward, max |diff| / max |ref| = %.2g" %
      (B, S, F, med["hip_fwd"], med["torch_fwd"], med["hip_fwd_bwd"], med["torch_fwd_bwd"], med["abi_fwd"], med["abi_bwd"], 100 * max(spread.values()), err), flush=True)
print(json.dumps({"B": B, "S": S, "F": F, "median_us": med, "spread": spread, "forward_rel_diff": err}))
