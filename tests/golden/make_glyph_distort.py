"""Writes tests/golden/glyph_distort_cs.npz: per case of glyph_distort_cases.GPU_CASES <case>_cs [V, 2] float64,
scipy.special.cosdg and sindg of the angles of the restatement's draws (1, 0 where no angle is drawn), which the kernel's own
cos / sin are held to in tests/test_gpu_glyph_distort.py.

    python tests/golden/make_glyph_distort.py        (scipy 1.15.3 wrote the committed file)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import glyph_distort_cases as gd  # noqa: E402


def main():
    out = {}
    for name, (glyph_set, gdim, _, _, seed, generation, _, bounds) in gd.GPU_CASES.items():
        b = dict(gd.NEUTRAL, **bounds)
        G = len(gd.gpu_glyphs(glyph_set, gdim))
        angles = [gd.draw_variant(v, generation, seed, G, b)[1] for v in range(gd.GPU_V)]
        out[name + "_cs"] = np.asarray([gd.cosdg_sindg(a) if b["max_ang"] != 0.0 else (1.0, 0.0) for a in angles], np.float64)
    path = os.path.join(HERE, "glyph_distort_cs.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
