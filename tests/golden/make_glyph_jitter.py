"""Writes tests/golden/glyph_jitter_scipy.npz: what scipy.ndimage makes of the inputs of tests/test_gpu_glyph_jitter.py, so
that the GPU test needs no scipy.  Per case of glyph_jitter_cases.FIXTURE_CASES the final glyph of every variant -- the
reference's lines multi_mnist.py:113-135 (affine_transform / rotate at order 5, clip, threshold, crop) for the parameters of
the restatement's draws -- as <case>_shapes [V, 2] int32 (h, w; 0, 0 where nothing is left) and <case>_pixels, the glyphs'
float32 pixels one after the other (rotate takes the angle: its c, s are scipy.special.cosdg / sindg); and per case of
glyph_jitter_cases.GPU_CASES <case>_cs [V, 2] float64, cosdg and sindg of the drawn angles.

    python tests/golden/make_glyph_jitter.py        (scipy 1.15.3 wrote the committed file)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import glyph_jitter_cases as gj  # noqa: E402


def main():
    out = {}
    for name in gj.FIXTURE_CASES:
        glyph_set, _, seed, generation, bounds = gj.GPU_CASES[name]
        glyphs, crops = gj.gpu_glyphs(glyph_set)
        finals = gj.scipy_bank(glyphs, crops, gj.GPU_V, seed, generation, bounds)
        out[name + "_shapes"] = np.asarray([(0, 0) if f is None else f.shape for f in finals], np.int32)
        out[name + "_pixels"] = np.concatenate([np.zeros(0, np.float32)] + [f.reshape(-1) for f in finals if f is not None])
    for name, (glyph_set, _, seed, generation, bounds) in gj.GPU_CASES.items():
        draws = [gj.draw_variant(v, generation, seed, len(gj.gpu_glyphs(glyph_set)[0]), dict(gj.NEUTRAL, **bounds))
                 for v in range(gj.GPU_V)]
        out[name + "_cs"] = np.asarray([gj.cosdg_sindg(d[3]) for d in draws], np.float64)
    path = os.path.join(HERE, "glyph_jitter_scipy.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
