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


# ---- the eval transform in front of it (include/evt_preprocess.h) -------------------------------
# Resize(R, bicubic) + CenterCrop(S) of the reference's build_eval_transform (utils.py:593-607) on
# decoded uint8 images of any size. Pillow resamples 8-bit images in integer arithmetic (22-bit
# fixed-point coefficients, a horizontal then a vertical pass, each rounded and clamped to uint8);
# only the coefficient tables need floating point. `resize_geometry`, `resize_coefficients` and
# `EvalTransform.reference` restate that on the host and ARE the contract; the library computes the
# same tables in C++ and the kernel applies them, so the device result equals `reference` bit for
# bit.
RESIZE_FILTERS = {"bilinear": 2, "bicubic": 3}  # Pillow's codes (the reference passes 3)
_PRECISION_BITS = 22


def default_resize(size: int) -> int:
    """The reference's Resize argument for a crop of `size`: int((256 / 224) * size)."""
    return int((256 / 224) * size)


def resize_geometry(h: int, w: int, resize: int, size: int):
    """(oh, ow, top, left) of torchvision's Resize(resize) + CenterCrop(size) on an h x w image:
    the short side becomes `resize`, the other int(resize * long / short); the crop window starts
    at int(round((o - size) / 2.0)) (Python's round: half to even). Padding is not done."""
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    if oh < size or ow < size:
        raise ValueError(f"the resized image {oh} x {ow} is smaller than the crop {size}")
    return oh, ow, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


def _filter_value(code: int, x: float) -> float:
    x = abs(x)
    if code == 2:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_coefficients(in_size: int, out_size: int, interpolation: str = "bicubic",
                        first: int = 0, count: int = None):
    """(bounds [count, 2] int32 of (xmin, n), kk [count, ksize] int32) for output indices
    first .. first+count-1 of one axis: Pillow's precompute_coeffs and normalize_coeffs_8bpc in
    Python floats (fp64, every operation rounded on its own)."""
    code = RESIZE_FILTERS[interpolation]
    count = out_size - first if count is None else count
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    support = (1.0 if code == 2 else 2.0) * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((count, 2), np.int32)
    kk = np.zeros((count, ksize), np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_filter_value(code, (x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[i, x] = int(-0.5 + v * (1 << _PRECISION_BITS)) if v < 0 \
                else int(0.5 + v * (1 << _PRECISION_BITS))
        bounds[i] = (xmin, n)
    return bounds, kk


def _resample_axis1(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass along axis 1 of a uint8 [H, W, C] image; int32-exact (sums stay below 2^31)."""
    out = np.empty((img.shape[0], kk.shape[0], img.shape[2]), np.uint8)
    wide = img.astype(np.int64)
    for i in range(kk.shape[0]):
        xmin, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << (_PRECISION_BITS - 1)) + np.tensordot(
            wide[:, xmin:xmin + n, :], kk[i, :n].astype(np.int64), axes=([1], [0]))
        out[:, i, :] = np.clip(acc >> _PRECISION_BITS, 0, 255)
    return out


class EvalTransform:
    """Resize + centre crop of uint8 HWC images on the device, feeding `Uint8Images`:

        pre = EvalTransform(224)                       # Resize(256, bicubic), CenterCrop(224)
        logits = model(pre(decoded_images, model.device))

    `images` is a list of uint8 [H, W, C] torch tensors (on the device already, views with a row
    pitch included, or on the host and copied) or numpy arrays, of any mix of sizes. The result is
    a `Uint8Images` [B, size, size, C] on the device carrying `mean` / `std`; the normalisation
    stays in the forward's first kernel. Plans (the device tables of one (H, W, C)) are cached, at
    most `max_plans` of them; past that the least recently used plan is destroyed, after a
    synchronisation of the stream it was last launched on (rare: it takes more than `max_plans`
    distinct image shapes; a single call with more shapes than that keeps all its plans until it
    is launched and trims the cache afterwards). `reference` is the same transform in numpy on the host, the contract
    the device result equals bit for bit."""

    def __init__(self, size: int = 224, resize: int = None, interpolation: str = "bicubic",
                 mean: Sequence[float] = IMAGENET_DEFAULT_MEAN,
                 std: Sequence[float] = IMAGENET_DEFAULT_STD, max_plans: int = 1024):
        if interpolation not in RESIZE_FILTERS:
            raise ValueError(f"interpolation must be one of {sorted(RESIZE_FILTERS)}")
        if size < 1 or max_plans < 1:
            raise ValueError("size and max_plans must be positive")
        self.size = int(size)
        self.resize = default_resize(self.size) if resize is None else int(resize)
        if self.resize < 1:
            raise ValueError("resize must be positive")
        self.interpolation = interpolation
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        affine_constants(self.mean, self.std)  # validates
        self.max_plans = int(max_plans)
        from collections import OrderedDict
        self._plans = OrderedDict()  # (device index, H, W, C) -> [plan pointer, last stream]

    # -- host side: the contract -------------------------------------------------------------
    def reference(self, img) -> np.ndarray:
        """The transform of one uint8 [H, W, C] image in numpy integers, [size, size, C]."""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3:
            raise ValueError("img must be a uint8 [H, W, C] array")
        h, w, _ = img.shape
        oh, ow, top, left = resize_geometry(h, w, self.resize, self.size)
        x = img[:, :, :]
        if ow != w:
            x = _resample_axis1(x, *resize_coefficients(w, ow, self.interpolation, left, self.size))
        else:
            x = x[:, left:left + self.size]
        if oh != h:
            t = _resample_axis1(x.transpose(1, 0, 2),
                                *resize_coefficients(h, oh, self.interpolation, top, self.size))
            x = t.transpose(1, 0, 2)
        else:
            x = x[top:top + self.size]
        return np.ascontiguousarray(x)

    def geometry(self, h: int, w: int) -> dict:
        """evt_resize_geometry of an h x w image: oh, ow, top, left and the two table widths
        (host only; raises EvtError for what the library rejects)."""
        from . import _lib
        lib = _lib.load_library()
        v = [ctypes.c_int() for _ in range(6)]
        _lib.check(lib.evt_resize_geometry(h, w, self.resize, self.size,
                                           RESIZE_FILTERS[self.interpolation],
                                           *[ctypes.byref(x) for x in v]))
        return dict(zip(("oh", "ow", "top", "left", "ksize_h", "ksize_v"), (x.value for x in v)))

    # -- device side ----------------------------------------------------------------------------
    def _evict(self, keep=()) -> None:
        """Destroy least recently used plans until at most `max_plans` are left, sparing `keep`
        (the plans of a call that has not been launched yet); each after a synchronisation of the
        stream it was last launched on."""
        from . import _lib
        lib = _lib.load_library()
        for key in [k for k in self._plans if k not in keep]:  # least recently used first
            if len(self._plans) <= self.max_plans:
                break
            old, last = self._plans.pop(key)
            last.synchronize()
            _lib.check(lib.evt_resize_plan_destroy(ctypes.c_void_p(old)))

    def _plan(self, dev_index: int, h: int, w: int, c: int, stream, in_use: set):
        from . import _lib
        key = (dev_index, h, w, c)
        in_use.add(key)
        hit = self._plans.get(key)
        if hit is not None:
            self._plans.move_to_end(key)
            hit[1] = stream
            return hit[0]
        plan = ctypes.c_void_p()
        _lib.check(_lib.load_library().evt_resize_plan_create(
            h, w, c, self.resize, self.size, RESIZE_FILTERS[self.interpolation],
            ctypes.byref(plan)))
        self._plans[key] = [plan.value, stream]
        self._evict(keep=in_use)  # never a plan of the call being assembled
        return plan.value

    def into(self, images, out) -> "Uint8Images":
        """The transform of `images` into `out`, a contiguous uint8 [B, size, size, C] device
        tensor (its first len(images) images when it is larger); returns the `Uint8Images` of
        that part. Launches on torch's current stream of out's device; no synchronisation."""
        import torch
        from . import _lib
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_cuda
                and out.is_contiguous() and out.ndim == 4):
            raise ValueError("out must be a contiguous uint8 [B, size, size, C] device tensor")
        images = list(images)
        B, C = len(images), out.shape[3]
        if B < 1 or B > out.shape[0] or tuple(out.shape[1:3]) != (self.size, self.size):
            raise ValueError(f"out is {tuple(out.shape)}: {B} images of crop {self.size} do not fit")
        if C != len(self.mean):
            raise ValueError(f"out has {C} channels, mean / std have {len(self.mean)}")
        dev = out.device
        _lib.ensure_device(dev.index if dev.index is not None else torch.cuda.current_device())
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            items = (_lib.evt_resize_item * B)()
            keep, in_use = [], set()
            for i, im in enumerate(images):
                t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.ndim != 3:
                    raise TypeError(f"image {i}: need a uint8 [H, W, C] torch tensor or numpy array")
                if t.shape[2] != C:
                    raise ValueError(f"image {i} has {t.shape[2]} channels, the batch {C}")
                if t.device != dev:
                    t = t.contiguous().to(dev, non_blocking=True)
                h, w = int(t.shape[0]), int(t.shape[1])
                # a view keeps its pitch; anything but interleaved pixels in whole rows is copied
                if not ((t.stride(2) == 1 or C == 1) and (t.stride(1) == C or w == 1)
                        and (t.stride(0) >= w * C or h == 1)):
                    t = t.contiguous()
                keep.append(t)
                items[i].src = t.data_ptr()
                items[i].pitch = t.stride(0) if h > 1 else w * C
                items[i].plan = self._plan(dev.index, h, w, C, stream, in_use)
            _lib.check(_lib.load_library().evt_resize_crop_u8(
                items, B, C, self.size, ctypes.c_void_p(out.data_ptr()),
                ctypes.c_void_p(stream.cuda_stream)))
            if len(self._plans) > self.max_plans:  # a call with more shapes than max_plans
                self._evict()
            # the sources may be released now: torch's allocator orders reuse after this stream
        return Uint8Images(out[:B], self.mean, self.std)

    def __call__(self, images, device) -> "Uint8Images":
        import torch
        images = list(images)
        if not images:
            raise ValueError("images is empty")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((len(images), self.size, self.size, int(images[0].shape[2])),
                          dtype=torch.uint8, device=device)
        return self.into(images, out)

    def close(self) -> None:
        """Destroy the cached plans (after a synchronisation of the streams they ran on)."""
        from . import _lib
        while self._plans:
            _, (plan, last) = self._plans.popitem()
            last.synchronize()
            _lib.check(_lib.load_library().evt_resize_plan_destroy(ctypes.c_void_p(plan)))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
