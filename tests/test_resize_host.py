"""CPU: the uint8 eval transform (include/evt_preprocess.h, EvalTransform) without a device.

  * `EvalTransform.reference` equals every golden of tests/golden/resize_eval.npz (Pillow 12.2.0's
    resize + the centre crop; tests/golden/make_golden_resize.py) bit for bit: no tolerance, no
    case left out. Where Pillow is importable the same comparison runs against the live library.
  * the library's tables (evt_resize_coefficients, the C++ that plan creation runs) equal the
    Python restatement's integer for integer, and |kk| < 2^23, for every fixture geometry and the
    workload's 500 x 375 -> 224;
  * evt_resize_geometry against the Python formulas over a hypothesis sweep, and its EVT_EINVALs;
  * the EVT_EINVALs of evt_resize_plan_create and evt_resize_crop_u8 that precede any device work;
  * header = `_lib.PREPROCESS_SIGNATURES` = exported symbols; evt.h includes the header;
    build.SOURCES / HEADERS list the new files;
  * `tools.py gpu_benchmark --raw_shape` parses and needs --dtype uint8.

Which golden covers which rounding of the crop offset: down_tall / down_wide have (51 - 32) / 2 =
9.5 -> 10 (odd integer part, half-even rounds up), ratio has (225 - 16) / 2 = 104.5 -> 104 (even
integer part, rounds down), big_ratio has 0.5 -> 0.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from edgevisiontransformer_amd import EvalTransform, _lib
from edgevisiontransformer_amd.images import (RESIZE_FILTERS, default_resize, resize_coefficients,
                                              resize_geometry)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "resize_eval.npz"))
CASES = json.loads(str(GOLDEN["cases"]))
FILTERS = ("bicubic", "bilinear")
ENTRY_POINTS = ["evt_resize_coefficients", "evt_resize_crop_u8", "evt_resize_geometry",
                "evt_resize_plan_create", "evt_resize_plan_destroy"]
# name -> the shape the issue sets for it
REQUIRED = {"down_tall": (53, 37, 3, 36, 32), "down_wide": (37, 53, 3, 36, 32),
            "up": (16, 16, 3, 36, 32), "up_down": (20, 64, 3, 24, 20), "same": (36, 48, 3, 36, 32),
            "ratio": (24, 300, 3, 18, 16)}


def transform_for(case, interpolation):
    c = case["c"]
    return EvalTransform(case["size"], case["resize"], interpolation, mean=(0.5,) * c,
                         std=(0.25,) * c)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def test_the_fixture_holds_the_cases_it_should():
    by_name = {c["name"]: c for c in CASES}
    for name, (h, w, c, r, s) in REQUIRED.items():
        k = by_name[name]
        assert (k["h"], k["w"], k["c"], k["resize"], k["size"]) == (h, w, c, r, s), name
    for chans in (1, 4):  # one down and one up case each
        scales = {k["resize"] > min(k["h"], k["w"]) for k in CASES if k["c"] == chans}
        assert scales == {True, False}, chans
    assert max(by_name["big_ratio"]["h"], by_name["big_ratio"]["w"]) / by_name["big_ratio"]["resize"] > 10
    for k in CASES:
        a = GOLDEN["in_" + k["name"]]
        assert a.dtype == np.uint8 and a.shape == (k["h"], k["w"], k["c"])
        if k["name"] not in ("ratio", "big_ratio"):
            assert max(a.shape[:2]) <= 64
    for name in ("checker", "binary", "up_c4"):  # 0 / 255 content
        assert set(np.unique(GOLDEN["in_" + name])) == {0, 255}
    out = GOLDEN["out_binary_bicubic"]
    assert (out == 0).any() and (out == 255).any()  # both clamps fire
    # the half-even crop offsets, both parities
    assert resize_geometry(53, 37, 36, 32) == (51, 36, 10, 2)
    assert resize_geometry(24, 300, 18, 16) == (18, 225, 1, 104)
    assert resize_geometry(96, 100, 9, 8) == (9, 9, 0, 0)


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_equals_the_golden(case, interpolation):
    got = transform_for(case, interpolation).reference(GOLDEN["in_" + case["name"]])
    want = GOLDEN[f"out_{case['name']}_{interpolation}"]
    assert got.dtype == np.uint8 and got.shape == want.shape == (case["size"], case["size"], case["c"])
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


def test_an_unchanged_axis_is_the_crop_alone_and_identity_tables():
    case = next(c for c in CASES if c["name"] == "same")
    a = GOLDEN["in_same"]
    for f in FILTERS:
        assert np.array_equal(transform_for(case, f).reference(a), a[2:34, 8:40])
        bounds, kk = resize_coefficients(48, 48, f)
        for i in range(48):  # one coefficient of exactly 2^22 on the pixel itself
            taps = {int(bounds[i, 0]) + x: int(v) for x, v in enumerate(kk[i]) if v}
            assert taps == {i: 1 << 22}


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_equals_live_pillow(case, interpolation):
    Image = pytest.importorskip("PIL.Image")
    a = GOLDEN["in_" + case["name"]]
    h, w, c = a.shape
    oh, ow, top, left = resize_geometry(h, w, case["resize"], case["size"])
    pil = (Image.fromarray(a[:, :, 0]) if c == 1 else Image.fromarray(a) if c == 3
           else Image.frombytes("CMYK", (w, h), a.tobytes()))  # CMYK: 4 plain bands, no alpha
    code = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[interpolation]
    r = np.asarray(pil.resize((ow, oh), code)).reshape(oh, ow, c)
    s = case["size"]
    assert np.array_equal(transform_for(case, interpolation).reference(a),
                          r[top:top + s, left:left + s])


def _c_tables(lib, in_size, out_size, first, count, interpolation, ksize):
    bounds = np.full((count, 2), -1, np.int32)
    kk = np.full((count, ksize), -1, np.int32)
    rc = lib.evt_resize_coefficients(in_size, out_size, first, count, RESIZE_FILTERS[interpolation],
                                     bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     kk.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0, lib.evt_last_error()
    return bounds, kk


GEOMETRIES = sorted({(c["h"], c["w"], c["resize"], c["size"]) for c in CASES} | {(500, 375, 256, 224),
                                                                               (375, 500, 256, 224)})


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("h,w,resize,size", GEOMETRIES)
def test_library_tables_equal_the_python_ones(lib, h, w, resize, size, interpolation):
    oh, ow, top, left = resize_geometry(h, w, resize, size)
    g = EvalTransform(size, resize, interpolation).geometry(h, w)
    assert (g["oh"], g["ow"], g["top"], g["left"]) == (oh, ow, top, left)
    for in_size, out_size, first, ksize in ((w, ow, left, g["ksize_h"]), (h, oh, top, g["ksize_v"])):
        bounds, kk = resize_coefficients(in_size, out_size, interpolation, first, size)
        assert kk.shape[1] == ksize
        cb, ck = _c_tables(lib, in_size, out_size, first, size, interpolation, ksize)
        assert np.array_equal(cb, bounds) and np.array_equal(ck, kk)
        assert int(np.abs(kk.astype(np.int64)).max()) < 1 << 23
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all()
        assert (bounds.sum(1) <= in_size).all() and (bounds[:, 1] <= ksize).all()
        # normalised: the integer coefficients of a row sum to 2^22 within one unit per tap
        assert (np.abs(kk.sum(1) - (1 << 22)) <= bounds[:, 1]).all()


@settings(max_examples=300, deadline=None)
@given(h=st.integers(1, 3000), w=st.integers(1, 3000), resize=st.integers(1, 600),
       size=st.integers(1, 600))
def test_geometry_against_the_python_formulas(h, w, resize, size):
    lib = _lib.load_library()
    v = [ctypes.c_int(-7) for _ in range(6)]
    rc = lib.evt_resize_geometry(h, w, resize, size, 3, *[ctypes.byref(x) for x in v])
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    if oh < size or ow < size or max(oh, ow) > 16 * _lib.RESIZE_MAX_SIDE:
        assert rc == _lib.EVT_EINVAL
        return
    assert rc == 0, lib.evt_last_error()
    top, left = int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))
    assert [x.value for x in v[:4]] == [oh, ow, top, left]
    for (i, o), ks in (((w, ow), v[4].value), ((h, oh), v[5].value)):
        assert ks == int(np.ceil(2.0 * max(i / o, 1.0))) * 2 + 1


def test_geometry_default_resize_and_optional_outputs(lib):
    assert default_resize(224) == 256 and default_resize(384) == 438 and default_resize(32) == 36
    oh, ow = ctypes.c_int(), ctypes.c_int()
    none = [None] * 4
    for size in (224, 384, 32, 7):
        assert lib.evt_resize_geometry(500, 375, 0, size, 3, ctypes.byref(oh), ctypes.byref(ow),
                                       *none) == 0
        assert ow.value == default_resize(size) and oh.value == int(default_resize(size) * 500 / 375)
    assert lib.evt_resize_geometry(500, 375, 256, 224, 2, *([None] * 6)) == 0
    assert EvalTransform(224).geometry(375, 500) == dict(oh=256, ow=341, top=16, left=58,
                                                         ksize_h=7, ksize_v=7)


def _einval(lib, rc, *words):
    assert rc == _lib.EVT_EINVAL
    msg = lib.evt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_geometry_rejects(lib):
    def call(h=500, w=375, r=256, s=224, f=3):
        return lib.evt_resize_geometry(h, w, r, s, f, *([None] * 6))
    assert call() == 0
    big = _lib.RESIZE_MAX_SIDE + 1
    for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(h=big), dict(w=big)):
        _einval(lib, call(**kw), b"image sides")
    for kw in (dict(s=0), dict(s=-1), dict(s=big)):
        _einval(lib, call(**kw), b"crop")
    for kw in (dict(r=-1), dict(r=big)):
        _einval(lib, call(**kw), b"resize_short")
    for f in (0, 1, 4, -1):
        _einval(lib, call(f=f), b"filter")
    _einval(lib, call(r=200), b"smaller than the crop")           # both sides short
    _einval(lib, call(h=100, w=400, r=64, s=100), b"smaller than the crop")  # only the short side
    _einval(lib, call(h=1, w=32768, r=32768, s=1), b"beyond")     # 32768^2 on the long side


def test_coefficients_rejects(lib):
    buf = (ctypes.c_int32 * 4096)()
    _einval(lib, lib.evt_resize_coefficients(10, 5, 0, 5, 3, None, buf), b"non-null")
    _einval(lib, lib.evt_resize_coefficients(10, 5, 0, 5, 3, buf, None), b"non-null")
    _einval(lib, lib.evt_resize_coefficients(0, 5, 0, 5, 3, buf, buf), b"sizes")
    _einval(lib, lib.evt_resize_coefficients(10, 0, 0, 0, 3, buf, buf), b"sizes")
    _einval(lib, lib.evt_resize_coefficients(10, 5, 1, 5, 3, buf, buf), b"window")
    _einval(lib, lib.evt_resize_coefficients(10, 5, -1, 2, 3, buf, buf), b"window")
    _einval(lib, lib.evt_resize_coefficients(10, 5, 0, 5, 1, buf, buf), b"filter")


def test_plan_create_rejects_before_any_device_work(lib):
    plan = ctypes.c_void_p(123)

    def call(h=500, w=375, c=3, r=256, s=224, f=3, out=ctypes.byref(plan)):
        return lib.evt_resize_plan_create(h, w, c, r, s, f, out)
    _einval(lib, call(out=None), b"NULL")
    for c in (0, 5, -1):
        _einval(lib, call(c=c), b"1 to 4 channels")
        assert plan.value is None  # cleared on failure
        plan.value = 123
    _einval(lib, call(h=0), b"image sides")
    _einval(lib, call(f=7), b"filter")
    _einval(lib, call(r=200), b"smaller than the crop")
    _einval(lib, call(s=222, r=254), b"multiple of 4")           # 666 bytes per row
    _einval(lib, call(c=1, s=30, r=36), b"multiple of 4")
    # the LDS band: ksize_v * round_up(S*C, 16) <= 65536. 224 x 3 rows are 672 bytes, so 97 taps:
    # a reduction of 24 fits (ksize 97), 24.5 does not (ksize 99)
    g = EvalTransform(224, 256).geometry(6272, 6272)
    assert g["ksize_v"] == 99 and 99 * 672 > _lib.RESIZE_LDS_BYTES >= 97 * 672
    _einval(lib, call(h=6272, w=6272), b"LDS band")
    assert lib.evt_resize_plan_destroy(None) == 0


def test_crop_rejects_before_any_launch(lib):
    items = (_lib.evt_resize_item * 2)()
    out = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected on the host

    def call(it=items, batch=1, c=3, s=224, o=out):
        return lib.evt_resize_crop_u8(it, batch, c, s, o, None)
    _einval(lib, call(it=None), b"non-null")
    _einval(lib, call(o=None), b"non-null")
    _einval(lib, call(batch=-1), b"negative")
    for c in (0, 5):
        _einval(lib, call(c=c), b"1 to 4 channels")
    _einval(lib, call(s=222), b"multiple of 4")
    _einval(lib, call(s=0), b"multiple of 4")
    _einval(lib, call(o=ctypes.c_void_p(4104)), b"16-byte aligned")
    _einval(lib, call(), b"item 0", b"non-null")                  # NULL src and plan
    items[0].src = 4096
    _einval(lib, call(), b"item 0", b"non-null")                  # NULL plan
    assert call(batch=0) == 0                                      # nothing to do, nothing read


def test_header_binding_and_exports_agree(lib):
    txt = open(os.path.join(REPO, "include", "evt_preprocess.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.PREPROCESS_SIGNATURES) == ENTRY_POINTS
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) |
                                set(_lib.FEATURE_SIGNATURES) | set(_lib.IMAGE_SIGNATURES))
    assert '#include "evt_preprocess.h"' in open(os.path.join(REPO, "include", "evt.h")).read()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.PREPROCESS_SIGNATURES[name][1]
    for name, value in (("EVT_RESIZE_BILINEAR", _lib.RESIZE_BILINEAR),
                        ("EVT_RESIZE_BICUBIC", _lib.RESIZE_BICUBIC),
                        ("EVT_RESIZE_MAX_SIDE", _lib.RESIZE_MAX_SIDE),
                        ("EVT_RESIZE_LDS_BYTES", _lib.RESIZE_LDS_BYTES),
                        ("EVT_RESIZE_CHUNK", _lib.RESIZE_CHUNK)):
        assert re.search(rf"#define {name}\s+{value}\b", txt), name
    assert RESIZE_FILTERS == {"bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC}
    # pointer, int64, pointer
    assert ctypes.sizeof(_lib.evt_resize_item) == 24
    assert (_lib.evt_resize_item.pitch.offset, _lib.evt_resize_item.plan.offset) == (8, 16)
    from edgevisiontransformer_amd import build
    assert "preprocess.hip" in build.SOURCES
    assert any(h.endswith("evt_preprocess.h") for h in build.HEADERS)


def test_python_argument_checks():
    with pytest.raises(ValueError):
        EvalTransform(224, interpolation="nearest")
    with pytest.raises(ValueError):
        EvalTransform(0)
    with pytest.raises(ValueError):
        EvalTransform(224, mean=(0.5,), std=(0.5, 0.5))
    t = EvalTransform(32)
    assert (t.size, t.resize, t.interpolation) == (32, 36, "bicubic")
    with pytest.raises(ValueError):
        t.reference(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="smaller than the crop"):
        EvalTransform(32, resize=20).reference(np.zeros((20, 20, 3), np.uint8))


def test_gpu_benchmark_raw_shape_flag():
    from edgevisiontransformer_amd import tools
    a = tools.parse_server_args(["gpu_benchmark", "--model", "deit_base", "--dtype", "uint8",
                                 "--raw_shape", "500,375"])
    assert a.raw_shape == [500, 375]
    assert tools.parse_server_args(["gpu_benchmark", "--model", "deit_base"]).raw_shape is None
    with pytest.raises(ValueError, match="uint8"):
        tools.parse_server_args(["gpu_benchmark", "--model", "deit_base", "--raw_shape", "500,375"])
    for bad in ("500", "500,0", "1,2,3"):
        with pytest.raises(ValueError, match="raw_shape"):
            tools.parse_server_args(["gpu_benchmark", "--model", "deit_base", "--dtype", "uint8",
                                     "--raw_shape", bad])
