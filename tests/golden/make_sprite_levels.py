"""Writes tests/golden/sprite_levels.npz: what matplotlib's imsave(cmap='gray') makes of the reference's sprite sheets
(embeddings.py:117-131) -- needs matplotlib and PIL; the tests only read the file.

  python tests/golden/make_sprite_levels.py

Per case c: windows_c float32 [M, w, w] and plane_c uint8 [dim w, dim w], the red channel of the PNG (red = green = blue,
alpha = 255); `table`: the 256 grey levels of the colormap as bytes.  Cases: (M, w) = (1, 28), (5, 28), (9, 5), (10, 4) with
random windows, and an all-zero (3, 4) sheet (hi == lo)."""
import io
import math
import os

import matplotlib
matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

CASES = [(1, 28), (5, 28), (9, 5), (10, 4)]


def sheet_of(windows):
    m, w = windows.shape[0], windows.shape[1]
    dim = int(math.ceil(math.sqrt(m)))
    sheet = np.ones((dim * w, dim * w))
    for i in range(m):
        x, y = i % dim, i // dim
        sheet[y * w:(y + 1) * w, x * w:(x + 1) * w] -= windows[i]
    return sheet


def saved(sheet):
    buf = io.BytesIO()
    plt.imsave(buf, sheet, cmap="gray", format="png")
    rgba = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGBA"))
    assert (rgba[..., 0] == rgba[..., 1]).all() and (rgba[..., 0] == rgba[..., 2]).all() and (rgba[..., 3] == 255).all()
    return np.ascontiguousarray(rgba[..., 0])


def main():
    rng = np.random.RandomState(13)
    out = {"table": np.ascontiguousarray(matplotlib.colormaps["gray"](np.arange(256), bytes=True)[:, 0])}
    sets = [(rng.uniform(0.0, hi, (m, w, w)).astype(np.float32)) for (m, w), hi in zip(CASES, (0.9, 1.0, 1.0, 0.6))]
    sets.append(np.zeros((3, 4, 4), np.float32))
    for c, windows in enumerate(sets):
        out["windows_%d" % c] = windows
        out["plane_%d" % c] = saved(sheet_of(windows))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sprite_levels.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes), matplotlib %s" % (path, os.path.getsize(path), matplotlib.__version__))


if __name__ == "__main__":
    main()
