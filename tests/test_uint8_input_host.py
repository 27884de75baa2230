"""CPU: the uint8 image input (include/evt_image.h, edgevisiontransformer_amd/images.py) without a
device.

  * `Uint8Images.to_float` against exact rational arithmetic: for every constant set the GPU tests
    use and all 256 x C byte values, u * scale + shift (scale, shift the fp32 constants) is exactly
    representable in fp64, so rounding it once to fp32 is what an fmaf returns, and `to_float` is
    that value bit for bit, in both layouts, for numpy and torch data;
  * header = `_lib.IMAGE_SIGNATURES` = exported symbols, and evt.h includes the header;
  * the EVT_EINVAL paths of evt_forward_image, evt_graph_capture_image, evt_patchify_u8 and
    evt_unfold_u8 that need no model, each before any launch;
  * `tools.py gpu_benchmark --dtype uint8` parses, and maps --input_shape to the NHWC byte shape.
"""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import (IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, Uint8Images,
                                       _lib, tools)
from edgevisiontransformer_amd.images import (EVT_IMG_F32, EVT_IMG_U8_NHWC, affine_constants,
                                              evt_image_args)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["evt_forward_image", "evt_graph_capture_image", "evt_patchify_u8", "evt_unfold_u8"]
# scale (1, 2, 4) / 255 and shift (0, -10, 100) as (mean, std): std = 1 / (255 scale),
# mean = -shift std; channel-distinct, so a swapped channel cannot hide
DISTINCT_STD = (1.0, 0.5, 0.25)
DISTINCT_MEAN = (0.0, 5.0, -25.0)
CONSTANT_SETS = {
    "imagenet": (IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD),
    "distinct": (DISTINCT_MEAN, DISTINCT_STD),
    "one_channel": ((0.5,), (0.25,)),
    "four_channels": ((0.485, 0.456, 0.406, 0.0), (0.229, 0.224, 0.225, 1.0)),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def all_bytes(C):
    """[1, 16, 16, C]: every byte value in every channel."""
    return np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1),
                           (1, 16, 16, C)).copy()


def test_constants_are_the_reference_ones():
    assert IMAGENET_DEFAULT_MEAN == (0.485, 0.456, 0.406)
    assert IMAGENET_DEFAULT_STD == (0.229, 0.224, 0.225)
    scale, shift = affine_constants(IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    assert scale.dtype == shift.dtype == np.float32
    for c in range(3):  # fp64, rounded once
        assert scale[c] == np.float32(1.0 / (255.0 * IMAGENET_DEFAULT_STD[c]))
        assert shift[c] == np.float32(-IMAGENET_DEFAULT_MEAN[c] / IMAGENET_DEFAULT_STD[c])
    scale, shift = affine_constants(DISTINCT_MEAN, DISTINCT_STD)
    assert np.array_equal(scale, (np.array([1, 2, 4]) / 255.0).astype(np.float32))
    assert np.array_equal(shift, np.array([0, -10, 100], np.float32))


@pytest.mark.parametrize("name", sorted(CONSTANT_SETS))
def test_to_float_is_the_exact_fma(name):
    mean, std = CONSTANT_SETS[name]
    C = len(mean)
    u8 = Uint8Images(all_bytes(C), mean, std)
    scale, shift = u8.scale, u8.shift
    nhwc, nchw = u8.to_float("nhwc"), u8.to_float("nchw")
    assert nhwc.dtype == nchw.dtype == np.float32
    assert nhwc.shape == (1, 16, 16, C) and nchw.shape == (1, C, 16, 16)
    assert np.array_equal(nchw.view(np.int32), nhwc.transpose(0, 3, 1, 2).view(np.int32))
    for c in range(C):
        fs, fh = Fraction(float(scale[c])), Fraction(float(shift[c]))
        for u in range(256):
            exact = u * fs + fh
            as_double = float(exact)
            # exact in fp64 without anyone's help, so one rounding to fp32 is the fmaf's result
            assert Fraction(as_double) == exact, (name, c, u)
            want = np.float32(as_double)
            got = nhwc[0, u // 16, u % 16, c]
            assert got.view(np.int32) == want.view(np.int32), (name, c, u, got, want)
    t = Uint8Images(torch.from_numpy(all_bytes(C)), mean, std)
    assert torch.equal(t.to_float("nhwc").view(torch.int32), torch.from_numpy(nhwc).view(torch.int32))
    assert torch.equal(t.to_float("nchw").view(torch.int32), torch.from_numpy(nchw).view(torch.int32))


def test_uint8images_argument_checks():
    ok = all_bytes(3)
    with pytest.raises(TypeError):
        Uint8Images(ok.astype(np.float32))
    with pytest.raises(TypeError):
        Uint8Images(torch.zeros((1, 4, 4, 3)))
    with pytest.raises(ValueError):
        Uint8Images(ok[0])
    with pytest.raises(ValueError):
        Uint8Images(all_bytes(4))  # 4 channels, 3 constants
    with pytest.raises(ValueError):
        Uint8Images(ok, std=(0.229, 0.0, 0.225))
    with pytest.raises(ValueError):
        Uint8Images(ok).to_float("hwc")
    with pytest.raises(ValueError):
        Uint8Images(ok).image_args()  # host data: .to(device) first


def test_header_binding_and_exports_agree(lib):
    txt = open(os.path.join(REPO, "include", "evt_image.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.IMAGE_SIGNATURES) == ENTRY_POINTS
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) |
                                set(_lib.FEATURE_SIGNATURES))
    assert '#include "evt_image.h"' in open(os.path.join(REPO, "include", "evt.h")).read()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.IMAGE_SIGNATURES[name][1]
    assert "#define EVT_IMG_F32     0" in txt and "#define EVT_IMG_U8_NHWC 1" in txt
    assert (EVT_IMG_F32, EVT_IMG_U8_NHWC) == (0, 1)
    # the struct the binding passes is the header's: pointer, int32, 2 x float[4], padded to 8
    assert ctypes.sizeof(evt_image_args) == 48
    assert (evt_image_args.format.offset, evt_image_args.scale.offset,
            evt_image_args.shift.offset) == (8, 12, 28)
    from edgevisiontransformer_amd import build
    assert any(h.endswith("evt_image.h") for h in build.HEADERS)


def _einval(lib, rc, *words):
    assert rc == _lib.EVT_EINVAL
    msg = lib.evt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_forward_image_rejects_before_any_launch(lib):
    """NULL descriptor / outputs / data / model and an unknown format need no device."""
    out = _lib.evt_features_args()
    out.logits = 64
    img = evt_image_args()
    img.data, img.format = 64, EVT_IMG_U8_NHWC
    model = ctypes.c_void_p(0)
    _einval(lib, lib.evt_forward_image(model, None, 1, ctypes.byref(out), None), b"NULL")
    _einval(lib, lib.evt_forward_image(model, ctypes.byref(img), 1, None, None), b"non-null")
    _einval(lib, lib.evt_forward_image(model, ctypes.byref(img), 1, ctypes.byref(out), None),
            b"model is NULL")
    _einval(lib, lib.evt_graph_capture_image(model, ctypes.byref(img), 1, None, None),
            b"model is NULL")
    img.data = None
    _einval(lib, lib.evt_forward_image(model, ctypes.byref(img), 1, ctypes.byref(out), None),
            b"data is NULL")
    _einval(lib, lib.evt_graph_capture_image(model, ctypes.byref(img), 1, None, None),
            b"data is NULL")
    img.data = 64
    for fmt in (2, -1):
        img.format = fmt
        _einval(lib, lib.evt_forward_image(model, ctypes.byref(img), 1, ctypes.byref(out), None),
                b"unknown image format")
        _einval(lib, lib.evt_graph_capture_image(model, ctypes.byref(img), 1, None, None),
                b"unknown image format")


def test_patchify_u8_rejects_before_any_launch(lib):
    one = (ctypes.c_float * 4)(1, 1, 1, 1)
    zero = (ctypes.c_float * 4)()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected on the host

    def call(dtype=1, img=p, B=1, C=3, HW=28, ps=14, out=p, ldo=640, x=p, cls=p, pos=p, D=192,
             scale=one, shift=zero):
        return lib.evt_patchify_u8(dtype, img, B, C, HW, ps, out, ldo, x, cls, pos, D, None,
                                   scale, shift, None)
    _einval(lib, call(dtype=2), b"dtype")
    _einval(lib, call(C=5), b"1 to 4 channels")
    _einval(lib, call(C=0), b"1 to 4 channels")
    _einval(lib, call(scale=None), b"non-null")
    for bad in (float("nan"), float("inf"), -float("inf")):
        _einval(lib, call(scale=(ctypes.c_float * 4)(1, bad, 1, 1)), b"finite")
        _einval(lib, call(shift=(ctypes.c_float * 4)(0, 0, bad, 0)), b"finite")
    # a non-finite constant past the first C is not read
    _einval(lib, call(C=1, HW=28, ldo=192, scale=(ctypes.c_float * 4)(1, float("nan"), 1, 1)),
            b"bad shape")
    _einval(lib, call(C=1, HW=6, ps=3, ldo=16), b"bad shape")   # ps*HW*C = 18: not a multiple of 4
    _einval(lib, call(HW=30), b"bad shape")                      # HW % ps
    _einval(lib, call(ldo=584), b"bad shape")                    # ldo < pd
    _einval(lib, call(ldo=644), b"bad shape")                    # ldo % 8
    _einval(lib, call(HW=1022, ps=14), b"bad shape")             # strip beyond 160 KiB
    _einval(lib, call(D=0), b"bad shape")
    _einval(lib, call(img=None), b"non-null")
    _einval(lib, call(out=None), b"non-null")
    _einval(lib, call(img=ctypes.c_void_p(4098)), b"aligned")
    _einval(lib, call(out=ctypes.c_void_p(4104)), b"aligned")


def test_unfold_u8_rejects_before_any_launch(lib):
    one = (ctypes.c_float * 4)(1, 1, 1, 1)
    zero = (ctypes.c_float * 4)()
    p = ctypes.c_void_p(4096)

    def call(dtype=1, img=p, B=1, H=16, W=16, C=3, k=7, s=4, pad=2, out=p, ldo=192, scale=one,
             shift=zero):
        return lib.evt_unfold_u8(dtype, img, B, H, W, C, k, s, pad, out, ldo, None, 0, scale,
                                 shift, None)
    _einval(lib, call(dtype=3), b"dtype")
    _einval(lib, call(C=5, ldo=256), b"1 to 4 channels")
    _einval(lib, call(shift=None), b"non-null")
    _einval(lib, call(scale=(ctypes.c_float * 4)(float("nan"), 1, 1, 1)), b"finite")
    _einval(lib, call(shift=(ctypes.c_float * 4)(0, 0, float("inf"), 0)), b"finite")
    _einval(lib, call(img=None), b"bad shape")
    _einval(lib, call(out=None), b"bad shape")
    _einval(lib, call(ldo=144), b"bad shape")          # ldo < k*k*C
    _einval(lib, call(H=2, W=2), b"bad shape")         # window larger than the padded image
    _einval(lib, call(s=0), b"bad shape")
    _einval(lib, call(C=4, ldo=196, img=ctypes.c_void_p(4098)), b"bad shape")  # C = 4: 4-B words


def test_gpu_benchmark_accepts_uint8():
    a = tools.parse_server_args(["gpu_benchmark", "--model", "deit_base", "--dtype", "uint8",
                                 "--input_shape", "8,3,224,224"])
    assert a.dtype == "uint8" and "uint8" in tools.INPUT_DTYPES
    assert tools.parse_server_args(["gpu_benchmark", "--model", "deit_base"]).dtype == "float32"
    with pytest.raises(ValueError, match="input dtype"):
        tools.parse_server_args(["gpu_benchmark", "--model", "deit_base", "--dtype", "float16"])
    # --input_shape keeps the family's fp32 meaning; the bytes are NHWC for every family
    assert tools.uint8_shape("deit_base", [8, 3, 224, 224]) == [8, 224, 224, 3]
    assert tools.uint8_shape("swin_tiny", [4, 3, 224, 224]) == [4, 224, 224, 3]
    assert tools.uint8_shape("t2t_vit_14", [2, 224, 224, 3]) == [2, 224, 224, 3]
    assert tools._image_size("deit_base", [8, 3, 224, 224]) == 224
