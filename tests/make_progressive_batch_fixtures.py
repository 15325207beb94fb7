"""Writes tests/golden/progressive_batch/: three DIFFERENT 83 x 131 pictures, each saved by libjpeg (through PIL) at quality 75, 4:2:0, as a
PROGRESSIVE file and as a BASELINE file (optimize=False). libjpeg codes the same quantised coefficients either way, so the baseline file is the
progressive file's twin. The three progressive files share size, sampling and quantisation tables and nothing else: libjpeg writes optimised Huffman
tables into every progressive file, so no two of their headers are byte-equal -- tests/test_progressive_batch.py asks that they form ONE group of
dec_opt_batch_progressive all the same, and that every frame equals the oracle's decode of its baseline save. Run once, by hand, where PIL is
installed; the files are committed (a few KB each)."""
import os

import numpy as np
from PIL import Image

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive_batch")
W, H = 83, 131
NAMES = ["gradient", "rings", "blocks"]


def picture(name):
    rng = np.random.default_rng(83131 + NAMES.index(name))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if name == "gradient":
        rgb = np.stack([xx * 255 / (W - 1), yy * 255 / (H - 1), (xx + 2 * yy) * 255 / (W + 2 * H)], -1)
    elif name == "rings":
        r = np.hypot(xx - W / 3, yy - H / 2)
        rgb = np.stack([127 + 120 * np.sin(r / 3), 127 + 120 * np.cos(r / 5), 255 - r * 2], -1)
    else:
        rgb = np.stack([((xx // 9 + yy // 7) % 2) * 200 + 20, ((xx // 5) % 3) * 100 + 30, ((yy // 11) % 4) * 60 + 40], -1)
    rgb = rgb + rng.normal(0, 4, rgb.shape)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def main():
    os.makedirs(HERE, exist_ok=True)
    total = 0
    for name in NAMES:
        im = Image.fromarray(picture(name))
        im.save(os.path.join(HERE, name + "_progressive.jpg"), "JPEG", quality=75, subsampling=2, progressive=True)
        im.save(os.path.join(HERE, name + "_baseline.jpg"), "JPEG", quality=75, subsampling=2, optimize=False)
        a = np.asarray(Image.open(os.path.join(HERE, name + "_progressive.jpg")))
        b = np.asarray(Image.open(os.path.join(HERE, name + "_baseline.jpg")))
        sizes = [os.path.getsize(os.path.join(HERE, name + s)) for s in ("_progressive.jpg", "_baseline.jpg")]
        total += sum(sizes)
        print(name, sizes, "PIL decodes both to the same pixels:", bool(np.array_equal(a, b)))
        assert max(sizes) < 8192 and np.array_equal(a, b)
    print("total", total)


if __name__ == "__main__":
    main()
