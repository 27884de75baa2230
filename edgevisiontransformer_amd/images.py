"""uint8 image input: the binding of include/evt_image.h.

A decoder, PIL / OpenCV or a data loader deliver uint8 interleaved HWC images; the reference's
accuracy path (utils.py:593-606) resizes, crops and then applies
`Normalize(IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)`. Wrapped in `Uint8Images`, such a batch
goes to every mirror class as it is, and the first kernel of the forward normalises it on the way
in (a quarter of the fp32 bytes over the host link and out of HBM):

    batch = Uint8Images(u8)                      # [B, S, S, C] uint8, torch or numpy
    logits = model(batch)                        # also features(...), capture_graph(...)

The device value of a pixel is fmaf(float(u), scale[c], shift[c]) with scale = 1 / (255 std) and
shift = -mean / std (fp64, rounded once to fp32); `to_float` gives exactly those values, so
`model(batch)` equals `model(batch.to_float(native layout))` bit for bit. A bare uint8 tensor
keeps its old meaning (`.float()`, values 0..255, no normalisation).
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

# timm.data.constants, as the reference imports them at utils.py:596
IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)
EVT_IMG_F32, EVT_IMG_U8_NHWC = 0, 1


class evt_image_args(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("format", ctypes.c_int32),
                ("scale", ctypes.c_float * 4), ("shift", ctypes.c_float * 4)]


def affine_constants(mean: Sequence[float], std: Sequence[float]):
    """(scale, shift) fp32 arrays: 1 / (255 std) and -mean / std, computed in fp64 and rounded
    once."""
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    if m.shape != s.shape or m.ndim != 1 or not 1 <= m.size <= 4:
        raise ValueError("mean and std must be sequences of the same length, 1 to 4 channels")
    if not (np.all(np.isfinite(m)) and np.all(np.isfinite(s)) and np.all(s != 0)):
        raise ValueError("mean and std must be finite, std non-zero")
    return (1.0 / (255.0 * s)).astype(np.float32), (-m / s).astype(np.float32)


class Uint8Images:
    """A uint8 NHWC batch [B, S, S, C] (torch.uint8 tensor or np.uint8 array, C <= 4) with the
    per-channel normalisation the forward applies to it."""

    def __init__(self, data, mean: Sequence[float] = IMAGENET_DEFAULT_MEAN,
                 std: Sequence[float] = IMAGENET_DEFAULT_STD):
        import torch
        if isinstance(data, np.ndarray):
            ok = data.dtype == np.uint8
        elif isinstance(data, torch.Tensor):
            ok = data.dtype == torch.uint8
        else:
            raise TypeError("data must be a torch.uint8 tensor or a numpy uint8 array")
        if not ok:
            raise TypeError(f"data must be uint8, got {data.dtype}")
        if data.ndim != 4:
            raise ValueError(f"data must be [B, S, S, C], got {tuple(data.shape)}")
        self.data = data
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._scale, self._shift = affine_constants(self.mean, self.std)
        if data.shape[3] != self._scale.size:
            raise ValueError(f"data has {data.shape[3]} channels, mean / std have {self._scale.size}")

    @property
    def scale(self) -> np.ndarray:
        return self._scale.copy()

    @property
    def shift(self) -> np.ndarray:
        return self._shift.copy()

    @property
    def shape(self):
        return tuple(self.data.shape)

    @property
    def is_numpy(self) -> bool:
        return isinstance(self.data, np.ndarray)

    def _like(self, data) -> "Uint8Images":
        out = Uint8Images.__new__(Uint8Images)
        out.data, out.mean, out.std = data, self.mean, self.std
        out._scale, out._shift = self._scale, self._shift
        return out

    def to(self, device) -> "Uint8Images":
        """The same batch as a contiguous torch tensor on `device`."""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(self.data)) if self.is_numpy else self.data
        return self._like(t.to(device).contiguous())

    def to_float(self, layout: str = "nchw"):
        """The exact fp32 image the device computes, float32(float64(u) * float64(scale[c]) +
        float64(shift[c])), as "nchw" [B, C, S, S] or "nhwc" [B, S, S, C]; numpy for numpy data,
        else a torch tensor on the data's device (a 256 x C table looked up per pixel)."""
        if layout not in ("nchw", "nhwc"):
            raise ValueError('layout must be "nchw" or "nhwc"')
        lut = (np.arange(256, dtype=np.float64)[:, None] * self._scale.astype(np.float64)[None]
               + self._shift.astype(np.float64)[None]).astype(np.float32)  # [256, C]
        chan = np.arange(self._scale.size)
        if self.is_numpy:
            out = lut[self.data, chan]
            return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if layout == "nchw" else out
        import torch
        lut_t = torch.from_numpy(lut).to(self.data.device)
        out = lut_t[self.data.long(), torch.from_numpy(chan).to(self.data.device)]
        return out.permute(0, 3, 1, 2).contiguous() if layout == "nchw" else out

    def image_args(self) -> evt_image_args:
        """The evt_image_args of a device-resident batch (keep `self` alive while it is in use)."""
        if self.is_numpy or not self.data.is_cuda or not self.data.is_contiguous():
            raise ValueError("image_args needs a contiguous device tensor: use .to(device) first")
        a = evt_image_args()
        a.data, a.format = self.data.data_ptr(), EVT_IMG_U8_NHWC
        for c in range(self._scale.size):
            a.scale[c], a.shift[c] = float(self._scale[c]), float(self._shift[c])
        return a
