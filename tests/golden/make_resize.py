"""Writes tests/golden/g14_resize.npz: small uint8 inputs and what ``PIL.Image.resize`` makes of them, so that the GPU test
of the resize kernels has a reference that does not depend on the Pillow installed where it runs.

    python tests/golden/make_resize.py

Inputs: 37 x 53 x 3 uniform noise (seed 14), its first channel, and the 200 x 313 crop [100:300, 200:513] of the decoded
sample photo (stored decoded: the fixture does not depend on the JPEG decoder either).  Keys: ``in_<name>``,
``out_<name>_<H>x<W>_<filter>``, ``pillow_version``."""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
SIZES = {"noise": [(17, 53), (37, 96), (129, 7), (1, 1), (64, 40)],
         "grey": [(29, 20)],
         "crop": [(128, 96), (5, 3), (64, 128)]}


def inputs():
    noise = np.random.default_rng(14).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    photo = np.asarray(Image.open(os.path.join(HERE, "canny_input_yoga.jpeg")).convert("RGB"))
    return {"noise": noise, "grey": noise[:, :, 0].copy(), "crop": photo[100:300, 200:513].copy()}


def main():
    data = {"pillow_version": np.array(PIL.__version__)}
    for name, img in inputs().items():
        data[f"in_{name}"] = img
        for H, W in SIZES[name]:
            for fname, f in FILTERS.items():
                data[f"out_{name}_{H}x{W}_{fname}"] = np.asarray(Image.fromarray(img).resize((W, H), f))
    path = os.path.join(HERE, "g14_resize.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {len(data)} arrays, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
