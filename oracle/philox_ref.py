"""Test infrastructure only: a numpy restatement of the noise planes of the step prologue (csrc/air_philox.h) and of
air_philox_fill (csrc/air_generate.hip), so that the kernels can be compared number for number.

Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) over arrays of counters, in uint64 arithmetic: the two
32 x 32 -> 64-bit products of a round are one multiplication each.

The index map, as the header documents it:
  * quad q of a call has counter (q & 0xffffffff, q >> 32, c2, c3) and key (seed & 0xffffffff, seed >> 32);
  * quads q < ceil(n_normal / 4) give normals 4q .. 4q + 3; the uniforms start at a FRESH quad behind them: quad
    ceil(n_normal / 4) + j gives uniforms 4j .. 4j + 3;
  * the step prologue uses c2 = global_step, c3 = 0x41495221; air_philox_fill uses c2 = call & 0xffffffff,
    c3 = 0x47454E31 + (call >> 32) (mod 2^32).

Uniforms are (x >> 8) * 2^-24, exact in fp32.  Normals are Box-Muller on two pairs of words, here in float64:
r = sqrt(-2 ln(((x >> 8) + 1) * 2^-24)), angle 2 pi (y >> 8) 2^-24, (r cos, r sin) of words (0, 1) and of words (2, 3)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STEP_SALT = 0x41495221                       # c3 of the step prologue
FILL_SALT = 0x47454E31                       # c3 of air_philox_fill, + the high word of the call counter
TWO_M24 = 2.0 ** -24


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """arrays (or scalars) of counter words and key words -> uint32 array [4, ...] of the four output words"""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m0, m1, mask, s32 = np.uint64(M0), np.uint64(M1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                # < 2^64: no wrap
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c).astype(np.uint32)


def quads(q0, count, c2, c3, seed):
    """the words of quads q0 .. q0 + count - 1: uint32 [count, 4]"""
    q = np.arange(q0, q0 + count, dtype=np.uint64)
    w = philox4x32_10(q & np.uint64(MASK), q >> np.uint64(32), int(c2) & MASK, int(c3) & MASK, int(seed) & MASK, (int(seed) >> 32) & MASK)
    return np.ascontiguousarray(w.T)


def uniforms_of(words):
    """[0, 1): (x >> 8) * 2^-24 -- float32, exactly what the kernel stores"""
    return ((words >> np.uint32(8)).astype(np.float64) * TWO_M24).astype(np.float32)


def normals_of(words):
    """Box-Muller on words (0, 1) and (2, 3) of each quad, float64: [count, 4]"""
    w = (words >> np.uint32(8)).astype(np.float64)
    out = np.empty(w.shape, np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log((w[:, a] + 1.0) * TWO_M24))
        ang = 2.0 * np.pi * w[:, a + 1] * TWO_M24
        out[:, a], out[:, a + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


def noise_planes(n_normal, n_uniform, c2, c3, seed):
    """(normals float64 [n_normal], uniforms float32 [n_uniform]) of one call"""
    qn, qu = (n_normal + 3) // 4, (n_uniform + 3) // 4
    normals = normals_of(quads(0, qn, c2, c3, seed)).reshape(-1)[:n_normal]
    uniforms = uniforms_of(quads(qn, qu, c2, c3, seed)).reshape(-1)[:n_uniform]
    return normals, uniforms


def step_planes(n_normal, n_uniform, global_step, seed):
    """what air_step_begin (or a GEMM that carries the job) writes at istate[GLOBAL_STEP] = global_step"""
    return noise_planes(n_normal, n_uniform, global_step, STEP_SALT, seed)


def fill_planes(n_normal, n_uniform, seed, call):
    """what air_philox_fill(seed, call) writes"""
    return noise_planes(n_normal, n_uniform, call & MASK, (FILL_SALT + (call >> 32)) & MASK, seed)
