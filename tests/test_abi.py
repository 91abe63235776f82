"""CPU-side checks of the C-ABI boundary: the library builds for gfx950, loads and exports every symbol include/air_hip.h
declares; the WHOLE of the ctypes mirror air/_hip.py -- every struct, field, constant and signature -- equals the header
(tests/abi_check.py reads it), and that comparison reports a doctored header or mirror by name; argument errors are
reported without touching a GPU, and the product path refuses to run without the HIP library / on CPU tensors (no
fallback)."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import pytest
import torch

import abi_check as abi

ROOT = abi.ROOT


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def test_every_declared_symbol_is_exported_and_bound(H):
    """declared == exported == bound, and load() gave every function the restype and argtypes of its _SIGNATURES row"""
    declared = sorted(abi.read_header().prototypes)
    src = re.sub(r"/\*.*?\*/", "", open(abi.HEADER).read(), flags=re.S)
    assert declared == sorted(set(re.findall(r"\b(air_[a-z0-9_]+)\s*\(", src)))      # the reader misses no air_*( of the header
    assert len(declared) >= 74
    lib = C.CDLL(H.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(H.EXPORTED_SYMBOLS) == declared
    for name, (res, args) in H._SIGNATURES.items():
        fn = getattr(H.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_abi_version_and_strerror(H):
    assert H.lib().air_abi_version() == H.ABI_VERSION == 6           # every feature since has been additive: the version stays
    assert b"invalid argument" in H.lib().air_strerror(H.EINVAL)
    assert H.lib().air_strerror(0) == b"success"
    assert (H.EINVAL, H.ELIMIT, H.EALIGN) == (-1, -2, -3)


# ---- the mirror equals the header ---------------------------------------------------------------------------------------
def test_the_reader_finds_the_whole_header():
    h, num = abi.read_header(), abi.compile_numbers()
    assert len(h.structs) >= 24 and len(h.prototypes) >= 74 and len(h.constants) >= 74
    assert len(num.sizeof) == len(h.structs) and len(num.fields) == sum(len(f) for f in h.structs.values()) >= 350
    assert sorted(num.values) == sorted(h.constants)
    assert h.structs["air_schedule_t"] == ["slot", "flags", "init", "iters", "factor", "vmin", "vmax"]
    assert h.prototypes["air_bf16_twin"] == ("int", ["const float*", "uint16_t*", "int64_t", "void*"])
    assert h.prototypes["air_strerror"] == ("const char*", ["int"]) and h.prototypes["air_abi_version"] == ("int", [])
    assert num.values["AIR_MAX_PANELS"] == 16 and num.values["AIR_EINVAL"] == -1


def test_structs_fields_and_layout_match_the_header(H):
    """both directions of the struct set; per struct the field names in order and the size; per field its offset and size"""
    assert abi.check_structs(abi.read_header(), abi.compile_numbers(), H) == []


def test_constants_match_the_header(H):
    """every upper-case integer X of _hip.py is AIR_X with the compiled value: ABI_VERSION and the error codes included, and
    no list of exceptions"""
    assert len(abi.constants(H)) >= 73 and {"ABI_VERSION", "EINVAL", "ELIMIT", "EALIGN", "DYN_COUNT"} <= set(abi.constants(H))
    assert abi.check_constants(abi.read_header(), abi.compile_numbers(), H) == []


def test_signatures_match_the_prototypes(H):
    """per prototype the restype and, element by element, the argtypes (abi_check.ctypes_of is the mapping)"""
    assert abi.check_signatures(abi.read_header(), H) == []


def _swap_wgrad_fields(src):
    assert "int32_t head_pack, Hs, Hh, Hz;" in src
    return src.replace("int32_t head_pack, Hs, Hh, Hz;", "int32_t head_pack, Hh, Hs, Hz;")


def _append_render_field(src):
    assert "    int32_t B, N, C, w;\n} air_render_t;" in src
    return src.replace("    int32_t B, N, C, w;\n} air_render_t;", "    int32_t B, N, C, w;\n    int32_t extra;\n} air_render_t;")


def _renumber_clip_norm(src):
    assert "AIR_DYN_CLIP_NORM      = 4," in src
    return src.replace("AIR_DYN_CLIP_NORM      = 4,", "AIR_DYN_CLIP_NORM      = 12,")


def _narrow_twin_count(src):
    assert "int air_bf16_twin(const float* src, uint16_t* dst, int64_t n, void* stream);" in src
    return src.replace("int air_bf16_twin(const float* src, uint16_t* dst, int64_t n, void* stream);",
                       "int air_bf16_twin(const float* src, uint16_t* dst, int n, void* stream);")


def _add_prototype(src):
    return src.replace("int air_abi_version(void);", "int air_abi_version(void);\nint air_new_thing(int x, void* stream);")


@pytest.mark.parametrize("doctor, item, names", [
    (_swap_wgrad_fields, "air_wgrad_t", ["air_wgrad_t: field 11 is Hh in the header, Hs in Wgrad",
                                         "air_wgrad_t.Hs: (offset, size) (64, 4) in C, (60, 4) in Wgrad",
                                         "air_wgrad_t.Hh: (offset, size) (60, 4) in C, (64, 4) in Wgrad"]),
    (_append_render_field, "air_render_t", ["air_render_t: field 8 is extra in the header, nothing in Render",
                                            "air_render_t: sizeof 56 in C, 48 in Render"]),
    (_renumber_clip_norm, "DYN_CLIP_NORM", ["DYN_CLIP_NORM = 4: AIR_DYN_CLIP_NORM is 12 in the header"]),
    (_narrow_twin_count, "air_bf16_twin", ["air_bf16_twin: argument 2 is int, bound as c_long"]),
    (_add_prototype, "air_new_thing", ["air_new_thing: declared in the header, no _SIGNATURES row"])])
def test_a_doctored_header_is_reported_by_name(H, tmp_path, doctor, item, names):
    """the checker catches what it is for: a copy of the header with one change gives exactly the mismatches of the changed
    item, each naming it (the repository's header is read, never written)"""
    path = tmp_path / "air_hip.h"
    path.write_text(doctor(open(abi.HEADER).read()))
    got = abi.check_abi(H, str(path))
    assert sorted(got) == sorted(names) and all(msg.startswith(item) for msg in got)


def test_a_doctored_mirror_is_reported_by_name(H):
    class Render(C.Structure):                                   # one field renamed
        _fields_ = [(n if n != "canvas" else "image", t) for n, t in H.Render._fields_]
    sigs = dict(H._SIGNATURES, air_render=(C.c_int, [C.POINTER(Render), C.c_void_p]))
    sigs["air_colsum"] = (C.c_int, sigs["air_colsum"][1][:-1])   # one argument dropped
    patched = types.SimpleNamespace(**dict(vars(H), Render=Render, _SIGNATURES=sigs))
    assert abi.check_abi(patched) == ["air_render_t: field 2 is canvas in the header, image in Render",
                                      "air_colsum: 3 parameters in the header, 2 argtypes"]
    assert abi.check_abi(types.SimpleNamespace(**dict(vars(H), NEW_LIMIT=5))) == ["NEW_LIMIT = 5: the header has no AIR_NEW_LIMIT"]


def test_argument_errors_without_gpu(H):
    lib = H.lib()
    assert lib.air_gemm(C.byref(H.Gemm()), None) == -1
    assert lib.air_gemm(None, None) == -1
    assert lib.air_attend_fwd(C.byref(H.AttendFwd()), None) == -1
    assert lib.air_write_bwd(C.byref(H.WriteBwd()), None) == -1
    assert lib.air_lstm_gates_fwd(None, None, None, None, None, 4, 4, None) == -1
    assert lib.air_grad_sqnorm(None, 10, None, None, None) == -1
    assert lib.air_colsum(None, 0, None) == -1
    assert lib.air_vae_bottleneck_fwd(C.byref(H.BottleneckFwd()), None) == -1
    assert lib.air_vae_bottleneck_bwd(None, None) == -1
    A = abi.host_ptr()
    # a norm-only weight-gradient problem (dW NULL) needs the partial-sum output
    nul = (H.Wgrad * 1)(H.Wgrad(A, A, None, None, 2, 4, 2, 2, 4, 4, 0, 0, 0, 0))
    assert lib.air_wgrad_grouped(nul, 1, 1, None, None, None) == -1
    assert lib.air_wgrad_num_blocks(nul, 1) == 1
    assert lib.air_wgrad_num_workgroups(nul, 1, 1) == 1 and lib.air_wgrad_num_workgroups(nul, 1, 0) == 1
    assert lib.air_wgrad_num_workgroups(nul, 1, 2) == -1 and lib.air_wgrad_num_workgroups(None, 1, 1) == -1
    # strips are a property of the problem table: >= 512 tiles with twins at precision 1 (2 column tiles per workgroup,
    # 4 from 2048 tiles), never at precision 0 or without twins
    T = C.c_void_p(64)
    big = (H.Wgrad * 1)(H.Wgrad(A, A, A, None, 2048, 1024, 128, 2048, 1024, 1024, 0, 0, 0, 0, T, T))
    assert lib.air_wgrad_num_blocks(big, 1) == 512 and lib.air_wgrad_num_workgroups(big, 1, 1) == 256
    assert lib.air_wgrad_num_workgroups(big, 1, 0) == 512
    big4 = (H.Wgrad * 1)(H.Wgrad(A, A, A, None, 16384, 1024, 256, 16384, 1024, 1024, 0, 0, 0, 0, T, T))
    assert lib.air_wgrad_num_workgroups(big4, 1, 1) == 1024
    notw = (H.Wgrad * 1)(H.Wgrad(A, A, A, None, 2048, 1024, 128, 2048, 1024, 1024, 0, 0, 0, 0))
    assert lib.air_wgrad_num_workgroups(notw, 1, 1) == 512
    assert lib.air_optim_num_partials(1000) > 0
    # panel-blocked twins: null buffers, bad descriptors
    one = (H.Panel * 1)(H.Panel(0, 0, 4, 8, 0, 0))
    assert lib.air_panel_shadow(None, A, one, 1, None) == -1
    assert lib.air_panel_shadow(A, A, one, 0, None) == -1
    assert lib.air_adam_clip_step_panels(A, A, A, A, 32, A, 1, A, A, 1.0, 0.9, 0.999, 1e-8, None, one, 1, None, None, None) == -1
    assert lib.air_adam_clip_step_panels(A, A, A, A, 16, A, 1, A, A, 1.0, 0.9, 0.999, 1e-8, None, one, 1, A, None, None) == -1   # 4 x 8 > 16


def test_no_cpu_fallback(H):
    from air import air_model as am
    am.reset_default_graph()
    with pytest.raises(H.AirHipError):
        am.AIRModel(torch.zeros(4, 2500), torch.zeros(4, dtype=torch.int32), cnn=False)
    with pytest.raises(H.AirHipError):
        H.load("/nonexistent/libair_hip.so")
    from air.transformer import transformer
    with pytest.raises(H.AirHipError):
        transformer(torch.zeros(1, 5, 5, 1), torch.zeros(1, 6), (3, 3))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, fn)).read()
                assert "oracle" not in txt.replace("no oracle", ""), os.path.join(dp, fn)
                assert "/root/reference" not in txt or fn.endswith(".py") and "import" not in \
                    [ln for ln in txt.splitlines() if "/root/reference" in ln][0]


def test_gemm_dispatch_is_pinned_per_shape(H):
    """Which kernel family an air_gemm descriptor reaches (air_gemm_kernel_name is host-only code, no launch):
      * bf16 twins supplied, whole 16-byte pieces          -> gemm_bf16tw_kernel (air_gemm_bf16.hip)
      * fp32 operands, even K / leading dimensions, row-major A  -> the lean kernels gemm_bf16v2 / gemm_f32v2
      * transposed A, or an odd K / leading dimension / 4-byte-aligned operand -> the general fallback kernels
        gemm_bf16_kernel / gemm_f32_kernel (air_gemm.hip; the only users are ragged test shapes and the transA form
        of the ABI -- no launch of the train step at any BASELINE configuration reaches them)."""
    lib = H.lib()
    buf = C.create_string_buffer(128)

    def name(M, N, K, ta=0, tb=0, prec=1, lda=None, ldb=None, twins=False, a_off=0, epi=0, tile=(0, 0)):
        g = H.Gemm()
        base = 1 << 20
        g.A, g.B, g.C = base + a_off, base * 2, base * 3
        g.M, g.N, g.K = M, N, K
        g.lda = lda if lda is not None else (M if ta else K)
        g.ldb = ldb if ldb is not None else (K if tb else N)
        g.ldc, g.transA, g.transB, g.precision, g.epi = N, ta, tb, prec, epi
        g.tile_m, g.tile_n = tile
        if twins:
            g.A16, g.B16 = base * 4, base * 5
        assert lib.air_gemm_kernel_name(C.byref(g), buf, 128) == 0
        return buf.value.decode()

    # the train step's shapes (Cfg-A and the stress batch): twins -> twin kernels, otherwise the lean ones
    for M, N, K, tb in ((192, 320, 256, 0), (192, 512, 784, 0), (192, 784, 512, 1), (64, 256, 1024, 1), (1280, 512, 784, 0)):
        assert name(M, N, K, tb=tb, twins=True).startswith("gemm_bf16tw_kernel<")
        assert name(M, N, K, tb=tb).startswith("gemm_bf16v2_kernel<")
        assert name(M, N, K, tb=tb, prec=0).startswith("gemm_f32v2_kernel<")
    # even-but-not-multiple-of-4 dimensions (Z = 50): still the lean kernels (8-byte loads)
    assert name(192, 100, 256).startswith("gemm_bf16v2_kernel<") and name(192, 256, 50).startswith("gemm_bf16v2_kernel<")
    assert name(192, 100, 256, twins=True).startswith("gemm_bf16v2_kernel<")          # N % 8 != 0: twins unusable
    assert name(192, 256, 50, twins=True).startswith("gemm_bf16v2_kernel<")           # K % 8 != 0
    # the general fallback kernels: transposed A, odd K, odd leading dimension, 4-byte aligned operand
    for kw in (dict(ta=1), dict(K=333), dict(lda=257), dict(a_off=4)):
        args = dict(M=70, N=150, K=256)
        args.update(kw)
        n1, n0 = name(**args), name(prec=0, **args)
        assert n1.startswith("gemm_bf16_kernel<") and n0.startswith("gemm_f32_kernel<"), (kw, n1, n0)


def test_no_undefined_names_in_the_gpu_only_code():
    """The model's code paths need a GPU and never run in the build container: a static pass over the product, the bench
    and the entry points for names that are bound nowhere (tools/undefined_names.py) -- the NameError class of mistakes."""
    import glob
    files = (glob.glob(os.path.join(ROOT, "tf-attend-infer-repeat_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tf-attend-infer-repeat_amd", "*", "*.py")) +
             [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")] + glob.glob(os.path.join(ROOT, "tests", "*.py")))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "undefined_names.py")] + files, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout
