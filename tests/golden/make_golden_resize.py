"""Writes tests/golden/resize_eval.npz: small uint8 images and what Pillow's resize followed by the
centre crop makes of them (the transform of the reference's build_eval_transform, utils.py:593-607).

Run on a CPU with Pillow installed (the fixture in the tree was written with Pillow 12.2.0):

    python tests/golden/make_golden_resize.py

Per case the file holds the input `in_<name>` [H, W, C] and, per filter, `out_<name>_<filter>`
[S, S, C]; `cases` is a JSON list of {name, h, w, c, resize, size}. Geometry is torchvision's
(Resize(R) then CenterCrop(S)), restated here because torchvision is not a dependency.

3 channels go through mode "RGB", 1 through "L". 4 channels go through "CMYK": four plain 8-bit
bands. "RGBA" would not do: Image.resize premultiplies alpha there, and the library's contract
resamples every channel on its own.

What each case is for (a Resize keeps the aspect ratio, so both axes always scale the same way, and
an axis keeps its size only when R equals the short side, and then both do):
  down_tall / down_wide   53 x 37 and 37 x 53, R 36, S 32: both orientations of the short-side
                          rule, down-scaling. The long side becomes 51, so its crop offset is
                          round(9.5) = 10: half to even with an ODD integer part (9 would be floor).
  up                      16 x 16 -> 36: fs = 1, at most 5 taps.
  up_down                 20 x 64, R 24, S 20: 24 x 76, and a 60-byte output row: the row tail
                          that is no multiple of 16 bytes.
  same                    36 x 48, R 36, S 32: no axis changes size, so Pillow makes no pass and
                          the result is the crop alone; the kernel applies its identity tables.
  ratio                   24 x 300, R 18, S 16: 18 x 225; the crop offset is round(104.5) = 104:
                          half to even with an EVEN integer part (105 would be half-up). Smooth
                          content with 0 / 255 specks, so that it compresses.
  big_ratio               96 x 100, R 9, S 8: 9 x 9, a reduction of 10.7 and 11.1 with up to 45 and
                          47 taps (the aspect ratio is kept, so `ratio` above has 7-tap tables);
                          crop offsets round(0.5) = 0. The one case above 64 px besides `ratio`.
  checker / binary        0 / 255 images, so both clamps fire (bicubic overshoots).
  *_c1 / *_c4             1 and 4 channels, one down and one up case each.
"""
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def geometry(h, w, resize, size):
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    assert oh >= size and ow >= size
    return oh, ow, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


def to_pil(a):
    h, w, c = a.shape
    if c == 1:
        return Image.fromarray(a[:, :, 0])
    if c == 3:
        return Image.fromarray(a)
    return Image.frombytes("CMYK", (w, h), a.tobytes())


def transform(a, resize, size, resample):
    h, w, c = a.shape
    oh, ow, top, left = geometry(h, w, resize, size)
    r = np.asarray(to_pil(a).resize((ow, oh), resample)).reshape(oh, ow, c)
    return np.ascontiguousarray(r[top:top + size, left:left + size])


def content(kind, h, w, c, rng):
    if kind == "random":
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        a.reshape(-1)[:2] = (0, 255)
        return a
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], c, axis=2)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    if kind == "smooth":  # compressible: a gradient with sparse 0 / 255 specks
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(yy * 7 + xx * (k + 1)) % 256 for k in range(c)], -1).astype(np.uint8)
        speck = rng.random((h, w, c)) < 0.03
        a[speck] = rng.integers(0, 2, int(speck.sum())).astype(np.uint8) * 255
        return a
    raise ValueError(kind)


# name, h, w, c, resize, size, content
CASES = [
    ("down_tall", 53, 37, 3, 36, 32, "random"),
    ("down_wide", 37, 53, 3, 36, 32, "random"),
    ("up", 16, 16, 3, 36, 32, "random"),
    ("up_down", 20, 64, 3, 24, 20, "random"),
    ("same", 36, 48, 3, 36, 32, "random"),
    ("ratio", 24, 300, 3, 18, 16, "smooth"),
    ("big_ratio", 96, 100, 3, 9, 8, "smooth"),
    ("checker", 53, 37, 3, 36, 32, "checker"),
    ("binary", 37, 53, 3, 36, 32, "binary"),
    ("down_c1", 53, 37, 1, 36, 32, "random"),
    ("up_c1", 16, 16, 1, 36, 32, "random"),
    ("down_c4", 37, 53, 4, 36, 32, "random"),
    ("up_c4", 16, 16, 4, 36, 32, "binary"),
]


def main():
    rng = np.random.default_rng(20261020)
    arrays, cases = {}, []
    for name, h, w, c, resize, size, kind in CASES:
        a = content(kind, h, w, c, rng)
        arrays[f"in_{name}"] = a
        for fname, resample in FILTERS.items():
            arrays[f"out_{name}_{fname}"] = transform(a, resize, size, resample)
        cases.append(dict(name=name, h=h, w=w, c=c, resize=resize, size=size))
    arrays["cases"] = np.array(json.dumps(cases))
    import PIL
    arrays["pillow_version"] = np.array(PIL.__version__)
    path = os.path.join(HERE, "resize_eval.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
