"""What the model mirrors share: the image helpers and `ModelHandle`, the owner of a libevt_hip.so
model handle (include/evt.h) with the forward, HIP-graph and lane plumbing around it.

A model class (vit.py, t2t_vit.py, swin.py) adds its constructor, its descriptor (`_desc`), the
names of its four C functions and its geometry (`_image_dims`, `_feature_geometry`).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Union

import numpy as np
import torch

from ... import _lib
from ...images import Uint8Images


def _to_device_image(img, device):
    """(device batch, input was numpy). A `Uint8Images` stays one (its bytes moved to the device):
    the forward then goes through evt_forward_image, which normalises in its first kernel."""
    if isinstance(img, Uint8Images):
        return img.to(device), img.is_numpy
    if isinstance(img, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(device), True
    if not isinstance(img, torch.Tensor):
        raise TypeError("img must be a torch.Tensor or numpy.ndarray")
    if img.dtype != torch.float32:
        img = img.float()
    if img.device != device:
        img = img.to(device)
    return img.contiguous(), False


def _check_image_shape(x, native_dims, nhwc_dims) -> None:
    """ValueError unless x is [B, *native_dims] (fp32) or, a Uint8Images, [B, *nhwc_dims]."""
    u8 = isinstance(x, Uint8Images)
    want = tuple(nhwc_dims) if u8 else tuple(native_dims)
    if len(x.shape) != 4 or tuple(x.shape[1:]) != want:
        raise ValueError(f"expected {'uint8 NHWC ' if u8 else ''}[B, {', '.join(map(str, want))}], "
                         f"got {tuple(x.shape)}")


class ModelHandle:
    """Base of ViT, T2T_ViT and SwinTransformer. A subclass sets `cfg` and the class attributes
    below, provides `_desc(max_batch)` and `_image_dims()`, and in its constructor calls
    `_open_device`, appends its device tensors to `_weights` in the C order, then `_open_handle`."""

    _C_NUM_WEIGHTS = _C_CREATE = _C_FORWARD = _C_QUERY_WORKSPACE = ""  # C function names
    _DEFAULT_LANES_KW: dict = {}  # further keywords of _lib.default_lanes

    def _open_device(self, dtype: str, device) -> None:
        if dtype not in _lib.DTYPE:
            raise ValueError(f"dtype must be one of {sorted(_lib.DTYPE)}")
        self.dtype = dtype
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        _lib.ensure_device(self.device.index or 0)
        self._weights: List[torch.Tensor] = []

    def _open_handle(self, lanes: Optional[int], max_batch: int) -> None:
        self._handle: Optional[int] = None
        self._max_batch = 0
        # batch lanes (evt_model_set_lanes): None = _lib.default_lanes
        self._lanes = lanes
        if max_batch:
            self._build(max_batch)

    # -- C ABI plumbing ---------------------------------------------------------------------
    def _ptr(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(self._handle)

    def _stream(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(_lib.stream_ptr(self.device))

    def _build(self, max_batch: int) -> None:
        lib = _lib.load_library()
        self.close()
        self._graph_io = None
        desc = self._desc(max_batch)
        n = getattr(lib, self._C_NUM_WEIGHTS)(ctypes.byref(desc))
        if n != len(self._weights):
            raise RuntimeError(f"library expects {n} weights, mirror has {len(self._weights)}")
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self._weights])
        out = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(lib, self._C_CREATE)(ctypes.byref(desc), ptrs, n, self._stream(),
                                                    ctypes.byref(out)))
            self._handle = out.value
            self._max_batch = max_batch
            self._lane_streams = _lib.set_lanes(
                self._handle, self._lanes if self._lanes is not None
                else _lib.default_lanes(self.dtype, max_batch, **self._DEFAULT_LANES_KW),
                self.device)

    def lanes(self) -> int:
        """Batch lanes of the handle (include/evt.h evt_model_set_lanes; 1 = none)."""
        out = ctypes.c_int()
        _lib.check(_lib.load_library().evt_model_lanes(self._ptr(), ctypes.byref(out)))
        return out.value

    def tail_mode(self) -> int:
        """How the last forward ran its last encoder block (include/evt_tail.h
        evt_model_tail_mode): bit 0 the CLS tail, bit 1 the full-row block; 0 for Swin and MX8."""
        out = ctypes.c_int()
        _lib.check(_lib.load_library().evt_model_tail_mode(self._ptr(), ctypes.byref(out)))
        return out.value

    def workspace_bytes(self, batch: int) -> int:
        out = ctypes.c_size_t()
        _lib.check(getattr(_lib.load_library(), self._C_QUERY_WORKSPACE)(
            ctypes.byref(self._desc(batch)), batch, ctypes.byref(out)))
        return out.value

    def allocated_workspace_bytes(self) -> int:
        """Bytes this handle's workspace, lanes included, asked for (include/evt_workspace.h)."""
        out = ctypes.c_size_t()
        _lib.check(_lib.load_library().evt_model_workspace_bytes(self._ptr(), ctypes.byref(out)))
        return out.value

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _lib.load_library().evt_model_destroy(self._ptr())
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- forward ------------------------------------------------------------------------------
    def _fit(self, img) -> int:
        """The batch of `img`, the handle rebuilt first if it is too small for it."""
        b = img.shape[0]
        if b > self._max_batch:
            self._build(b)
        return b

    @staticmethod
    def _image_args(img) -> _lib.evt_image_args:
        """The evt_image_args (include/evt_image.h) of a device-resident batch: a `Uint8Images`'
        own, or the fp32 tensor's data pointer."""
        if isinstance(img, Uint8Images):
            return img.image_args()
        args = _lib.evt_image_args()
        args.data, args.format = img.data_ptr(), 0  # EVT_IMG_F32
        return args

    def _forward_image(self, img: Uint8Images, out) -> None:
        """evt_forward_image of a device-resident Uint8Images with the outputs `out`
        (evt_features_args); logits alone run over the handle's lanes like the fp32 forward."""
        b, args = self._fit(img), self._image_args(img)
        _lib.check(_lib.load_library().evt_forward_image(
            self._ptr(), ctypes.byref(args), b, ctypes.byref(out), self._stream()))

    def forward_into(self, img: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
        """Enqueue the forward of a device-resident fp32 batch in the model's layout (or a
        device-resident `Uint8Images`, uint8 NHWC) into `logits` (no allocation)."""
        if isinstance(img, Uint8Images):
            out = _lib.evt_features_args()
            out.logits = logits.data_ptr()
            self._forward_image(img, out)
            return logits
        b = self._fit(img)
        _lib.check(getattr(_lib.load_library(), self._C_FORWARD)(
            self._ptr(), ctypes.c_void_p(img.data_ptr()), b, ctypes.c_void_p(logits.data_ptr()),
            self._stream()))
        return logits

    def _checked_image(self, img):
        x, was_numpy = _to_device_image(img, self.device)
        c, s = self.cfg.in_chans, self.cfg.image_size
        _check_image_shape(x, self._image_dims(), (s, s, c))  # a Uint8Images is NHWC everywhere
        return x, was_numpy

    def __call__(self, img: Union[torch.Tensor, np.ndarray, Uint8Images]):
        x, was_numpy = self._checked_image(img)
        logits = torch.empty((x.shape[0], self.cfg.num_classes), dtype=torch.float32,
                             device=self.device)
        with torch.cuda.device(self.device):
            self.forward_into(x, logits)
        # stream-ordered, as every torch op: a numpy input gets numpy logits (.cpu() waits for
        # them), a device tensor gets device logits without a host sync
        return logits.cpu().numpy() if was_numpy else logits

    call = __call__

    # -- HIP graph ----------------------------------------------------------------------------
    def capture_graph(self, img, logits: torch.Tensor) -> None:
        """Record one forward of the device buffers (img, logits) as a HIP graph
        (evt_graph_capture[_image]); replay_graph() re-runs it after the caller refills img (a
        Uint8Images: img.data) in place."""
        b = self._fit(img)
        lib = _lib.load_library()
        stream = torch.cuda.Stream(self.device)  # capture needs a non-default stream
        stream.wait_stream(torch.cuda.current_stream(self.device))
        out, s = ctypes.c_void_p(logits.data_ptr()), ctypes.c_void_p(stream.cuda_stream)
        with torch.cuda.stream(stream):
            if isinstance(img, Uint8Images):
                args = img.image_args()
                _lib.check(lib.evt_graph_capture_image(self._ptr(), ctypes.byref(args), b, out, s))
            else:
                _lib.check(lib.evt_graph_capture(self._ptr(), ctypes.c_void_p(img.data_ptr()), b,
                                                 out, s))
        torch.cuda.current_stream(self.device).wait_stream(stream)
        self._graph_io = (img, logits, b)  # keep the captured buffers alive

    def replay_graph(self) -> None:
        if not getattr(self, "_graph_io", None):
            raise RuntimeError("no captured graph: call capture_graph(img, logits) first")
        _lib.check(_lib.load_library().evt_graph_launch(self._ptr(), self._stream()))
