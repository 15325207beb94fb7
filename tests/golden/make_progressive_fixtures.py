"""Writes tests/golden/progressive/: one 131 x 83 gradient-plus-noise image saved by libjpeg (through PIL) as a PROGRESSIVE file and as a BASELINE
file (optimize=False) with the same quality and sampling. libjpeg codes the same quantised coefficients either way, so the baseline file is the
progressive file's twin: tests/test_progressive_decode.py asks that the product's decode of the progressive file equals the oracle's decode of the
baseline one. Run once, by hand, where PIL is installed; the files are committed (each under 8 KB)."""
import os

import numpy as np
from PIL import Image

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "progressive")
W, H = 131, 83
# name: (PIL subsampling or None for grey, quality)
FILES = {"444_q75": (0, 75), "422_q75": (1, 75), "420_q75": (2, 75), "420_q30": (2, 30), "420_q95": (2, 95), "grey_q75": (None, 75)}


def picture():
    rng = np.random.default_rng(131083)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + 2 * yy) * 255 // (W + 2 * H)], -1).astype(np.float64)
    rgb += rng.normal(0, 5, rgb.shape)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def main():
    os.makedirs(HERE, exist_ok=True)
    rgb = picture()
    for name, (sub, q) in FILES.items():
        im = Image.fromarray(rgb).convert("L") if sub is None else Image.fromarray(rgb)
        kw = {} if sub is None else {"subsampling": sub}
        im.save(os.path.join(HERE, name + "_progressive.jpg"), "JPEG", quality=q, progressive=True, **kw)
        im.save(os.path.join(HERE, name + "_baseline.jpg"), "JPEG", quality=q, optimize=False, **kw)
        a = np.asarray(Image.open(os.path.join(HERE, name + "_progressive.jpg")))
        b = np.asarray(Image.open(os.path.join(HERE, name + "_baseline.jpg")))
        sizes = [os.path.getsize(os.path.join(HERE, name + s)) for s in ("_progressive.jpg", "_baseline.jpg")]
        print(name, sizes, "PIL decodes both to the same pixels:", bool(np.array_equal(a, b)))
        assert max(sizes) < 8192 and np.array_equal(a, b)


if __name__ == "__main__":
    main()
