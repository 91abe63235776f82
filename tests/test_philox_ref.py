"""CPU checks of oracle/philox_ref.py, the numpy reference tests/test_gpu_step_prologue.py holds the noise planes against:
the generator itself against the Random123 known answers and the scalar model of oracle/shuffle_queue.py, and the index map
and number conversions against their statement in csrc/air_philox.h."""
import numpy as np

from oracle import philox_ref as pr
from oracle import shuffle_queue as sq

KAT = [  # Random123 kat_vectors, philox4x32-10: counter, key, output (the three quoted in tests/test_shuffle_queue.py)
    ((0, 0, 0, 0), (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = pr.philox4x32_10(*ctr, *key)
        assert got.dtype == np.uint32 and got.tolist() == want
    # ... and as three lanes of ONE vectorised call (same key only: the key is per call)
    ctr = np.array([KAT[0][0], (1, 2, 3, 4), (0xffffffff, 0, 0xffffffff, 0)], np.uint64)
    got = pr.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], 0, 0)
    assert got.shape == (4, 3) and got[:, 0].tolist() == KAT[0][2]


def test_vectorised_generator_agrees_with_the_scalar_model_on_scattered_counters():
    rng = np.random.RandomState(7)
    for key in ((0, 0), (0xdeadbeef, 0x12345678), (0xffffffff, 1)):
        ctr = rng.randint(0, 1 << 32, (64, 4), dtype=np.uint64)
        ctr[:4] = [(0, 0, 0, 0), (0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0, 0, 0), (0, 1, 39000, pr.STEP_SALT)]
        got = pr.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key)
        for i in range(len(ctr)):
            assert got[:, i].tolist() == sq.philox4x32_10(ctr[i].tolist(), key), (key, ctr[i])


def test_quads_carry_the_documented_counter_and_key():
    seed = (0x9abcdef1 << 32) | 0x01234567
    w = pr.quads(5, 3, 39000, pr.STEP_SALT, seed)
    assert w.shape == (3, 4)
    for i in range(3):
        assert w[i].tolist() == sq.philox4x32_10((5 + i, 0, 39000, pr.STEP_SALT), (0x01234567, 0x9abcdef1))
    # a quad index beyond 32 bits spills into the second counter word
    big = (3 << 32) + 9
    assert pr.quads(big, 1, 1, 2, seed)[0].tolist() == sq.philox4x32_10((9, 3, 1, 2), (0x01234567, 0x9abcdef1))
    # air_philox_fill: c2 = the low word of the call counter, the high word moves the salt
    call = (2 << 32) | 17
    n, u = pr.fill_planes(4, 4, seed, call)
    n2, u2 = pr.noise_planes(4, 4, 17, pr.FILL_SALT + 2, seed)
    assert np.array_equal(n, n2) and np.array_equal(u, u2)


def test_index_map_uniforms_start_at_a_fresh_quad():
    seed, step = (7 << 32) | 11, 3
    for nn, nu in ((0, 5), (5, 0), (1, 1), (4, 4), (7, 9)):
        normals, uniforms = pr.step_planes(nn, nu, step, seed)
        assert normals.shape == (nn,) and normals.dtype == np.float64 and uniforms.shape == (nu,) and uniforms.dtype == np.float32
        qn = (nn + 3) // 4
        for i in range(nu):
            x = sq.philox4x32_10((qn + i // 4, 0, step, pr.STEP_SALT), (11, 7))[i % 4]
            assert uniforms[i] == np.float32((x >> 8) * 2.0 ** -24)
        for i in range(nn):
            w = sq.philox4x32_10((i // 4, 0, step, pr.STEP_SALT), (11, 7))
            a = (i % 4) & 2
            r = np.sqrt(-2.0 * np.log(((w[a] >> 8) + 1) * 2.0 ** -24))
            ang = 2.0 * np.pi * (w[a + 1] >> 8) * 2.0 ** -24
            assert abs(normals[i] - (r * np.sin(ang) if i % 2 else r * np.cos(ang))) < 1e-14
    # the planes of another step or seed differ
    a = pr.step_planes(8, 8, 0, seed)
    for b in (pr.step_planes(8, 8, 39000, seed), pr.step_planes(8, 8, 0, seed + (1 << 32))):
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])


def test_number_conversions_at_the_ends_of_the_range():
    words = np.array([[0, 0, 0xffffffff, 0xffffffff], [0xff, 0xff, 0x100, 0x80000000]], np.uint32)
    u = pr.uniforms_of(words)
    assert u[0, 0] == 0.0 and u[0, 2] == np.float32(1.0 - 2.0 ** -24) and u[1, 0] == 0.0 and u[1, 3] == 0.5
    n = pr.normals_of(words)
    assert np.isfinite(n).all()
    assert abs(n[0, 0] - np.sqrt(-2.0 * np.log(2.0 ** -24))) < 1e-14 and n[0, 1] == 0.0        # the largest radius, angle 0: 5.768
    assert abs(n[0, 2]) < 1e-15 and n[0, 3] == 0.0                                   # ln 1 = 0: radius 0
    # moments of a large plane: a Gaussian and a uniform
    normals, uniforms = pr.step_planes(200000, 50000, 5, 1234)
    assert abs(normals.mean()) < 0.01 and abs(normals.std() - 1.0) < 0.01 and abs((normals ** 4).mean() - 3.0) < 0.1
    assert uniforms.min() >= 0.0 and uniforms.max() < 1.0 and abs(uniforms.mean() - 0.5) < 0.01
