"""The uint8 eval transform on the GPU (include/evt_preprocess.h, EvalTransform): the kernel does
integer work on tables the host computed, so every comparison here is bit for bit against
`EvalTransform.reference` (which tests/test_resize_host.py proves equal to Pillow's output).

Output buffers are prefilled with 0xAA and one image longer than the batch, so a byte that was not
written, or one written past the batch, shows.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import EvalTransform, Uint8Images, _lib
from tests.test_gpu_uint8_input import MODELS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "resize_eval.npz"))
CASES = json.loads(str(GOLDEN["cases"]))
FILTERS = ("bicubic", "bilinear")
FILL = 0xAA


def _transform(size, resize, interpolation, c):
    return EvalTransform(size, resize, interpolation, mean=(0.5,) * c, std=(0.25,) * c)


@functools.lru_cache(maxsize=None)
def _want(name, interpolation):
    case = next(c for c in CASES if c["name"] == name)
    ref = _transform(case["size"], case["resize"], interpolation, case["c"]).reference(
        GOLDEN["in_" + name])
    assert np.array_equal(ref, GOLDEN[f"out_{name}_{interpolation}"])  # the host test's gate
    return ref


def _run(pre, images, gpu, extra=1):
    """pre.into on a 0xAA buffer `extra` images longer than the batch: (result, spare part)."""
    c = int(images[0].shape[2])
    out = torch.full((len(images) + extra, pre.size, pre.size, c), FILL, dtype=torch.uint8, device=gpu)
    u8 = pre.into(images, out)
    torch.cuda.synchronize()
    assert isinstance(u8, Uint8Images) and u8.shape == (len(images), pre.size, pre.size, c)
    assert u8.data.data_ptr() == out.data_ptr()
    assert (out[len(images):] == FILL).all()
    return u8.data.cpu().numpy(), out


def _rand(h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    a.reshape(-1)[:2] = (0, 255)
    return a


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_fixture_singly(gpu, case, interpolation):
    pre = _transform(case["size"], case["resize"], interpolation, case["c"])
    a = GOLDEN["in_" + case["name"]]
    want = _want(case["name"], interpolation)
    got, _ = _run(pre, [a], gpu)                                   # numpy, copied
    assert np.array_equal(got[0], want), f"{int((got[0] != want).sum())} bytes differ"
    got, _ = _run(pre, [torch.from_numpy(a).to(gpu)], gpu)        # already on the device
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize("interpolation", FILTERS)
def test_fixtures_in_mixed_size_batches(gpu, interpolation):
    groups = {}
    for c in CASES:
        groups.setdefault((c["c"], c["size"], c["resize"]), []).append(c["name"])
    assert max(len(v) for v in groups.values()) >= 6  # the 3-channel crop-32 group: 4 image shapes
    for (chans, size, resize), names in groups.items():
        pre = _transform(size, resize, interpolation, chans)
        names = names + names[::-1]  # every plan twice, in another order
        got, _ = _run(pre, [GOLDEN["in_" + n] for n in names], gpu)
        for i, n in enumerate(names):
            assert np.array_equal(got[i], _want(n, interpolation)), (n, i)


def test_a_batch_one_larger_than_the_descriptor_chunk(gpu):
    """65 images of 9 x 7 (and a few 7 x 9): the second launch runs, for its one image."""
    n = _lib.RESIZE_CHUNK + 1
    pre = _transform(4, 5, "bicubic", 3)
    images = [_rand(*((7, 9) if i % 5 == 3 else (9, 7)), 3, 100 + i) for i in range(n)]
    got, _ = _run(pre, images, gpu)
    for i, a in enumerate(images):
        assert np.array_equal(got[i], pre.reference(a)), i
    assert not np.array_equal(got[n - 1], got[n - 2])


@pytest.mark.parametrize("name", ["down_tall", "up_down", "down_c1", "up_c4"])
def test_pitched_and_misaligned_sources(gpu, name):
    """Sources as views: a padded row pitch, and byte offsets 1, 2, 3 from an allocation start."""
    case = next(c for c in CASES if c["name"] == name)
    a = GOLDEN["in_" + name]
    h, w, c = a.shape
    pre = _transform(case["size"], case["resize"], "bicubic", c)
    want = _want(name, "bicubic")
    wide = torch.full((h, w + 5, c), 0x55, dtype=torch.uint8, device=gpu)
    wide[:, :w] = torch.from_numpy(a).to(gpu)
    view = wide[:, :w]
    assert view.stride(0) == (w + 5) * c and not view.is_contiguous()
    images = [view]
    for off in (1, 2, 3):
        flat = torch.full((h * w * c + 3,), 0x55, dtype=torch.uint8, device=gpu)
        flat[off:off + h * w * c] = torch.from_numpy(a).reshape(-1).to(gpu)
        t = flat[off:off + h * w * c].view(h, w, c)
        assert t.data_ptr() % 4 == (flat.data_ptr() + off) % 4
        images.append(t)
    got, _ = _run(pre, images, gpu)
    for i in range(4):
        assert np.array_equal(got[i], want), i


def test_the_same_call_twice_on_the_same_buffers(gpu):
    pre = _transform(32, 36, "bicubic", 3)
    names = ["down_tall", "binary", "up", "same"]
    images = [torch.from_numpy(GOLDEN["in_" + n]).to(gpu) for n in names]
    first, out = _run(pre, images, gpu)
    pre.into(images, out)
    torch.cuda.synchronize()
    second = out[:4].cpu().numpy()
    assert np.array_equal(first, second) and (out[4:] == FILL).all()
    for i, n in enumerate(names):
        assert np.array_equal(second[i], _want(n, "bicubic"))


def test_one_workload_sized_image(gpu):
    """500 x 375 -> Resize(256) -> 224: the reference's eval transform at its own size."""
    pre = EvalTransform(224)
    a = _rand(500, 375, 3, 7)
    yy, xx = np.mgrid[0:500, 0:375]
    a[:250] = np.stack([(yy + xx) % 256, (2 * xx) % 256, (yy * 3) % 256], -1)[:250]  # half smooth
    assert pre.geometry(500, 375) == dict(oh=341, ow=256, top=58, left=16, ksize_h=7, ksize_v=7)
    got, _ = _run(pre, [a], gpu)
    want = pre.reference(a)
    assert np.array_equal(got[0], want), f"{int((got[0] != want).sum())} bytes differ"


def test_a_reduction_that_shrinks_the_row_band(gpu):
    """1000 x 1100 x 4 -> Resize(73) -> 64: 13.7x, 57 taps of 256-byte rows; 16 output rows would
    need 70 KB of LDS, so the plan takes a lower band (the path the small fixtures do not reach)."""
    pre = _transform(64, 73, "bicubic", 4)
    g = pre.geometry(1000, 1100)
    assert g["ksize_v"] == 57 and (16 * 1000 // 73 + g["ksize_v"] - 2) * 256 > _lib.RESIZE_LDS_BYTES
    a = _rand(1000, 1100, 4, 11)
    got, _ = _run(pre, [a, a[:, ::-1].copy()], gpu)
    assert np.array_equal(got[0], pre.reference(a))
    assert np.array_equal(got[1], pre.reference(a[:, ::-1]))


def test_plan_cache_evicts_the_least_recently_used(gpu):
    pre = EvalTransform(32, 36, max_plans=2)
    names = ["down_tall", "down_wide", "up", "down_tall", "same"]
    for n in names:  # one shape per call: the third and every later call evicts
        got, _ = _run(pre, [GOLDEN["in_" + n]], gpu)
        assert np.array_equal(got[0], _want(n, "bicubic")), n
        assert len(pre._plans) <= 2
    got, _ = _run(pre, [GOLDEN["in_" + n] for n in names], gpu)  # more shapes than plans in a call
    for i, n in enumerate(names):
        assert np.array_equal(got[i], _want(n, "bicubic")), n
    pre.close()
    assert not pre._plans


@pytest.mark.parametrize("name", ["vit_ref_32", "swin_56"])
def test_end_to_end_equals_the_forward_of_the_reference_batch(gpu, name):
    make, size, _ = MODELS[name]
    m = make(1, gpu, 3)
    pre = EvalTransform(size, mean=(0.0, 5.0, -25.0), std=(1.0, 0.5, 0.25))
    shapes = [(size + 13, size + 40), (2 * size, 2 * size - 7), (size // 2 + 5, size // 2 + 9)]
    batches = [[_rand(h, w, 3, 10 * k + i) for i, (h, w) in enumerate(shapes)] for k in (0, 1)]
    refs = [np.stack([pre.reference(a) for a in b]) for b in batches]
    u8 = pre(batches[0], gpu)
    assert u8.mean == pre.mean and u8.std == pre.std
    got = m(u8).clone()
    want = [m(Uint8Images(torch.from_numpy(r).to(gpu), pre.mean, pre.std)).clone() for r in refs]
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    assert torch.isfinite(want[0]).all() and float(want[0].abs().max()) > 0
    assert torch.equal(bits(got), bits(want[0])) and not torch.equal(bits(want[0]), bits(want[1]))
    feats = m.features(u8, logits=True)
    assert torch.equal(bits(feats["logits"]), bits(want[0]))
    # a captured graph of the forward on the transformed batch; then the next batch transformed
    # into the captured bytes and replayed
    logits = torch.full((3, m.num_classes), float("nan"), device=gpu)
    m.capture_graph(u8, logits)
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(bits(logits), bits(want[0]))
    pre.into(batches[1], u8.data)
    m.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(bits(logits), bits(want[1]))
    m.close()


def test_the_call_is_capturable_in_a_graph(gpu):
    """No allocation, copy or synchronisation: evt_resize_crop_u8 records into a torch graph."""
    pre = _transform(32, 36, "bicubic", 3)
    names = ["down_tall", "up"]
    images = [torch.from_numpy(GOLDEN["in_" + n]).to(gpu) for n in names]
    out = torch.full((2, 32, 32, 3), FILL, dtype=torch.uint8, device=gpu)
    pre.into(images, out)  # plans exist before the capture
    out.fill_(FILL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pre.into(images, out)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        assert np.array_equal(out[i].cpu().numpy(), _want(n, "bicubic"))


def test_crop_rejects_before_any_launch_with_live_plans(gpu):
    lib = _lib.load_library()
    a = torch.from_numpy(GOLDEN["in_down_tall"]).to(gpu)  # 53 x 37 x 3
    plans = {}
    for key, (c, size) in dict(ok=(3, 32), c4=(4, 32), s28=(3, 28)).items():
        p = ctypes.c_void_p()
        _lib.check(lib.evt_resize_plan_create(53, 37, c, 36, size, 3, ctypes.byref(p)))
        plans[key] = p
    out = torch.full((2, 32, 32, 3), FILL, dtype=torch.uint8, device=gpu)

    def call(plan="ok", pitch=37 * 3, src=a.data_ptr(), c=3, size=32, o=out.data_ptr(), batch=2):
        items = (_lib.evt_resize_item * 2)()
        items[0].src, items[0].pitch, items[0].plan = a.data_ptr(), 37 * 3, plans["ok"].value
        items[1].src, items[1].pitch, items[1].plan = src, pitch, plans[plan].value
        return lib.evt_resize_crop_u8(items, batch, c, size, ctypes.c_void_p(o),
                                      ctypes.c_void_p(_lib.stream_ptr(gpu)))

    def einval(rc, *words):
        assert rc == _lib.EVT_EINVAL
        assert all(w in lib.evt_last_error() for w in words), lib.evt_last_error()
    einval(call(plan="c4"), b"item 1", b"channels")
    einval(call(c=4), b"item 0", b"channels")
    einval(call(plan="s28"), b"item 1", b"crop")
    einval(call(size=28), b"item 0", b"crop")
    einval(call(pitch=37 * 3 - 1), b"item 1", b"pitch")
    einval(call(src=None), b"item 1", b"non-null")
    einval(call(o=out.data_ptr() + 4), b"16-byte aligned")
    torch.cuda.synchronize()
    assert (out == FILL).all()  # nothing was launched, not even for the valid first item
    _lib.check(call())
    torch.cuda.synchronize()
    want = _want("down_tall", "bicubic")
    assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(out[1].cpu().numpy(), want)
    for p in plans.values():
        _lib.check(lib.evt_resize_plan_destroy(p))
    einval(lib.evt_resize_plan_create(53, 37, 3, 36, 32, 3, None), b"NULL")
