"""Writes tests/golden/generator_resize.npz: two float32 128 x 128 planes in [0, 255] (what ``generated_samples`` hands to the
resize after scaling the generator's output) and their Pillow ``Image.BICUBIC`` resizes to the radar arena's projections
(22, 176), (31, 176) and (22, 31) -- sizes that shrink one axis and stretch or shrink the other.  Run with Pillow installed:
``python tests/golden/make_golden_generator.py``."""
import os

import numpy as np
from PIL import Image

SIZES = {"xz": (176, 22), "yz": (176, 31), "xy": (31, 22)}          # Pillow's (cols, rows)


def main():
    rng = np.random.default_rng(20)
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64)
    smooth = 127.5 * (1.0 + np.tanh(2.0 * np.sin(xx / 9.0) * np.cos(yy / 5.0) + 0.5 * np.sin((xx + yy) / 3.0)))
    noisy = rng.uniform(0.0, 255.0, (128, 128))
    noisy[40:60, 30:90] = 255.0
    noisy[100:, :10] = 0.0
    # a short mantissa keeps the compressed fixture small; the values are ordinary float32 either way
    planes = np.stack([np.round(smooth * 16.0) / 16.0, np.round(noisy * 16.0) / 16.0]).astype(np.float32)
    out = {"planes": planes}
    for name, size in SIZES.items():
        out[name] = np.stack([np.asarray(Image.fromarray(p).resize(size, resample=Image.BICUBIC)) for p in planes]).astype(np.float32)
        assert out[name].shape == (2, size[1], size[0])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "generator_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
