"""Generation on a built AIRModel: scenes drawn from the priors (generate) or rendered from given latents (decode).

The generative half of the loop body (reference :288-439, 582; vae.py:26-41) with the posterior heads replaced by
the priors: no image, no LSTM, no recognition network.  Own noise / record / output buffers, own RNG call counter:
a forward() / training() result, the model's noise buffers, global_step, the schedules and a captured graph are not
touched.  Launches: [air_philox_fill ->] air_scene_records -> the generative GEMMs and gen_mean with the forward's
descriptors -> air_render (include/air_hip.h).

AIRModel.generate / decode / set_generate_noise / generate_ops are the public face; a Generator reads from its model
store.dims, dyn, the live _seed, _call, _generative_ops, _f32 / _i16, _fresh_shadow and _stream.
"""
import ctypes as C

import torch

from . import _hip as H
from ._hip import ptr as _ptr


class GeneratedScenes:
    """What AIRModel.generate() / decode() return: device tensors, image-major like the rec_* attributes, all max_steps
    steps (a step is an object of scene b while masks[b, t] == 1: the first num_digits[b] of them).  They are VIEWS of the
    model's generation buffers: the next generate() / decode() call overwrites them."""
    __slots__ = ("canvas", "num_digits", "scales", "shifts", "z_pres", "masks", "latents", "windows", "st_back")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def st_back_matrices(self):
        """[B, N, 2, 3] window -> canvas matrices (air_model.py:353-356), the form air.visualize draws boxes from"""
        return st_matrices(self.st_back)


def st_matrices(a):
    """[..., 3] = (1/s, -x/s, -y/s) -> [..., 2, 3] axis-aligned spatial-transformer matrices"""
    z = torch.zeros_like(a[..., 0])
    return torch.stack([torch.stack([a[..., 0], z, a[..., 1]], -1),
                        torch.stack([z, a[..., 0], a[..., 2]], -1)], -2)


class Generator:
    """The generation state of one AIRModel: buffers (allocated at the first call, kept for the model's life), launch
    lists (built at the first call and again after drop_ops()), the device RNG's call counter and the injected-noise flag."""

    def __init__(self, model):
        self.model = model
        self.calls = 0                  # the device RNG's call counter of generate() (never global_step)
        self.injected = False           # set_noise() filled the noise buffers for the next call
        self.buf = None
        self.ops = None
        self._keep = []                 # ctypes structs referenced by the closures

    def drop_ops(self):
        """The model rebuilt its programs: the launch lists are rebuilt with them at the next call; the buffers stay."""
        self.ops = None
        self._keep = []

    def _state(self):
        from .air_model import _carve_noise
        m, g = self.model, self.buf
        if g is None:
            dm, dv = m.store.dims, m.input_images.device
            B, N = m.batch_size, m.max_steps
            D, d, Z = dm["D"], dm["d"], dm["Z"]
            f, h16 = m._f32, m._i16
            g = self.buf = {}
            g["normals"], g["uniforms"] = f(N * B * (1 + 2 + Z + d)), f(N * B)
            g["eps_scale"], g["eps_shift"], g["eps_z"], g["eps_x"], g["u"] = _carve_noise(g["normals"], g["uniforms"], N, B, Z, d)
            # decode(): the caller's tensors, step-major
            g["in_s"], g["in_xy"], g["in_z"], g["in_p"] = f(N, B), f(N, B, 2), f(N, B, Z), f(N, B)
            g["att"] = f(N, B, H.ATT_STRIDE)
            # (rows of Z elements: the operand layout of the forward's unfused first generative GEMM, lda = K = Z)
            g["z"], g["z16"] = f(N, B, Z), h16(N, B, Z)
            g["act"] = [f(N, B, u) for u in m.vae_generative_units]
            g["act16"] = [h16(N, B, u) for u in m.vae_generative_units]
            g["vrec"] = f(N, B, d)
            g["canvas"] = f(B, D)
            g["digits"] = torch.zeros(B, dtype=torch.int32, device=dv)
        if self.ops is None:
            self.ops = self._build(g)
        return g

    def _build(self, g):
        """The generation launch lists; the decoder's GEMMs are the forward's (_generative_ops) on the generation buffers."""
        m = self.model
        dm = m.store.dims
        B, N, NB = m.batch_size, m.max_steps, m.max_steps * m.batch_size
        d, Z = dm["d"], dm["Z"]
        ops = {}
        for mode, srcs in (("sample", ("eps_scale", "eps_shift", "eps_z", "u")), ("given", ("in_s", "in_xy", "in_z", "in_p"))):
            r = H.SceneRecords(*[_ptr(g[k]) for k in srcs], _ptr(m.dyn), _ptr(g["att"]), _ptr(g["z"]), _ptr(g["z16"]),
                               B, N, Z, Z, 1 if mode == "given" else 0)
            self._keep.append(r)
            ops[mode] = m._call("air_scene_records", C.byref(r), nbytes=NB * (4 * (4 + 2 * Z) + 64), tag="scene_records_" + mode)
        for name, sigma in (("out_noise", float(m.vae_likelihood_std)), ("out_mean", 0.0)):
            dec = m._generative_ops(g["z"], g["z16"], g["act"], g["act16"], g["vrec"], g["eps_x"], sigma)
            ops["decoder"], ops[name] = dec[:-1], dec[-1]          # (the layers' descriptors do not depend on sigma)
        rd = H.Render(_ptr(g["vrec"]), _ptr(g["att"]), _ptr(g["canvas"]), _ptr(g["digits"]), B, N,
                      m.canvas_size, m.windows_size)
        self._keep.append(rd)
        ops["render"] = m._call("air_render", C.byref(rd), nbytes=NB * (d * 4 + 64) + B * dm["D"] * 4, tag="render")
        return ops

    def launch_list(self, likelihood_noise=False, given=False, fill=True):
        """AIRModel.generate_ops()"""
        self._state()
        o = self.ops
        ops = [self._fill_op()] if fill else []
        return ops + [o["given" if given else "sample"]] + o["decoder"] + [o["out_noise" if likelihood_noise else "out_mean"], o["render"]]

    def _fill_op(self):
        g, seed, call = self.buf, self.model._seed, self.calls
        return self.model._call("air_philox_fill", _ptr(g["normals"]), g["normals"].numel(), _ptr(g["uniforms"]), g["uniforms"].numel(),
                                C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint64(call),
                                nbytes=4 * (g["normals"].numel() + g["uniforms"].numel()), tag="philox_fill")

    def run(self, given, likelihood_noise, needs_noise):
        g = self._state()
        self.model._fresh_shadow()
        s = self.model._stream()
        fill = needs_noise and not self.injected
        for op in self.launch_list(likelihood_noise, given, fill):
            op(s)
        if fill:
            self.calls += 1
        self.injected = False
        a = g["att"]
        return GeneratedScenes(canvas=g["canvas"], num_digits=g["digits"],
                               scales=a[:, :, H.ATT_S:H.ATT_S + 1].transpose(0, 1), shifts=a[:, :, H.ATT_X:H.ATT_Y + 1].transpose(0, 1),
                               z_pres=a[:, :, H.ATT_Z].t(), masks=a[:, :, H.ATT_MASK].t(), latents=g["z"].transpose(0, 1),
                               windows=g["vrec"].transpose(0, 1), st_back=a[:, :, H.ATT_ST_BACK:H.ATT_ST_BACK + 3].transpose(0, 1))

    def set_noise(self, noise):
        """AIRModel.set_generate_noise()"""
        from .air_model import _copy_noise
        g = self._state()
        _copy_noise(noise, g.__getitem__)
        self.injected = True

    def decode(self, latents, scales, shifts, z_pres, likelihood_noise=False):
        """AIRModel.decode()"""
        m, g = self.model, self._state()
        B, N, Z = m.batch_size, m.max_steps, m.vae_latent_dimensions
        for name, t, shape, dst in (("latents", latents, (B, N, Z), g["in_z"]), ("scales", scales, (B, N, 1), g["in_s"]),
                                    ("shifts", shifts, (B, N, 2), g["in_xy"]), ("z_pres", z_pres, (B, N, 1), g["in_p"])):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise H.AirHipError("%s must be a CUDA/HIP device tensor: this path has no CPU fallback" % name)
            if t.dtype != torch.float32 or t.numel() != B * N * shape[2] or tuple(t.shape[:2]) != (B, N):
                raise ValueError("%s must be float32 %r" % (name, shape))
            dst.copy_(t.reshape(shape).transpose(0, 1).reshape(dst.shape))
        return self.run(True, bool(likelihood_noise), bool(likelihood_noise))
