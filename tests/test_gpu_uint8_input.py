"""uint8 image input on the GPU (include/evt_image.h): every uint8 reader deposits the fp32 values
`Uint8Images.to_float` gives (tests/test_uint8_input_host.py proves those are the exact fmaf
results), and everything after the loader is the fp32 path's code, so every comparison here is
bit for bit:

  * evt_patchify_u8 against evt_patchify_ld on to_float("nchw") (and evt_patchify_cm when
    ldo == pd): rows, zero tail, CLS rows, statistics;
  * evt_unfold_u8 against evt_unfold(in_f32=1) on to_float("nhwc"): rows with their zero padding
    and tail, statistics, on both the k7 s4 C3 band kernel and the generic kernel's element paths;
  * model(Uint8Images(u8)) against model(to_float(native layout)) for every family and first
    kernel, over 1 and 2 lanes at an unevenly split batch; features; a captured graph replayed
    after refilling the bytes in place; a second call.

Output buffers are NaN-filled; the bytes are seeded and include 0 and 255.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT, ViT_Pruned
from tests._ops import TDT, _p, _s, patchify

pytestmark = pytest.mark.gpu

# channel-distinct constants (scale (1, 2, 4) / 255, shift (0, -10, 100)): a swapped channel shows
DISTINCT = dict(mean=(0.0, 5.0, -25.0), std=(1.0, 0.5, 0.25))
CONSTANTS = {1: dict(mean=(0.5,), std=(0.25,)), 3: DISTINCT,
             4: dict(mean=(0.485, 0.456, 0.406, 0.0), std=(0.229, 0.224, 0.225, 1.0))}
NAN = float("nan")


def _bytes(shape, seed):
    u = np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)
    u.reshape(-1)[:2] = (0, 255)
    u.reshape(-1)[-2:] = (255, 0)
    return u


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _f4(a):
    return (ctypes.c_float * 4)(*[float(v) for v in a], *([0.0] * (4 - len(a))))


# ---- evt_patchify_u8 -------------------------------------------------------------------------
# ps, HW, B, C, ldo
PATCH_SHAPES = [
    (14, 28, 2, 3, 640),
    (14, 42, 3, 3, 640),    # odd patch count
    (14, 70, 1, 1, 256),    # C = 1, the last chunk straddles pd
    (16, 32, 2, 3, 768),    # ldo == pd: also evt_patchify_cm
    (8, 24, 1, 4, 256),     # C = 4
    (16, 224, 2, 3, 768),   # the real 16-B path
    (14, 518, 1, 3, 640),   # the 4-B-aligned path (span 21756 = 12 mod 16), the largest strip
]
WIDTHS = (192, 1536)


def _slots(D):
    return 2 * ((D + 255) // 256)


def _patch_buffers(dtype, B, P, ldo, D, gpu):
    return (torch.full((B * P, ldo), NAN, dtype=TDT[dtype], device=gpu),
            torch.full((B * (P + 1), D), NAN, dtype=TDT[dtype], device=gpu),
            torch.full((B * (P + 1), _slots(D), 2), NAN, device=gpu))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("ps,HW,B,C,ldo", PATCH_SHAPES)
def test_patchify_u8(gpu, dtype, ps, HW, B, C, ldo):
    lib = _lib.load_library()
    u8 = Uint8Images(torch.from_numpy(_bytes((B, HW, HW, C), ps * 1000 + HW)).to(gpu), **CONSTANTS[C])
    img = u8.to_float("nchw")
    assert tuple(img.shape) == (B, C, HW, HW) and img.is_contiguous()
    pd, P = ps * ps * C, (HW // ps) ** 2
    scale, shift = _f4(u8.scale), _f4(u8.shift)
    for D in WIDTHS:
        g = torch.Generator().manual_seed(D)
        cls, pos = torch.randn(D, generator=g).to(gpu), torch.randn(4, D, generator=g).to(gpu)
        want = _patch_buffers(dtype, B, P, ldo, D, gpu)
        _lib.check(lib.evt_patchify_ld(_lib.DTYPE[dtype], _p(img), B, C, HW, ps, _p(want[0]), ldo,
                                       _p(want[1]), _p(cls), _p(pos), D, _p(want[2]), _s()))
        got = _patch_buffers(dtype, B, P, ldo, D, gpu)
        _lib.check(lib.evt_patchify_u8(_lib.DTYPE[dtype], _p(u8.data), B, C, HW, ps, _p(got[0]),
                                       ldo, _p(got[1]), _p(cls), _p(pos), D, _p(got[2]), scale,
                                       shift, _s()))
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "x", "stats"), got, want):
            assert _same(a, b), (name, D)  # NaN fill included: nothing else was touched
        assert not torch.isnan(got[0].float()).any()
        if ldo > pd:
            assert (got[0][:, pd:] == 0).all()
        if ldo == pd and ps % 8 == 0:
            cm, x, st = patchify(dtype, img, ps, cls, pos, D, channel_major=True)
            torch.cuda.synchronize()
            rows = torch.arange(B, device=gpu) * (P + 1)
            assert _same(got[0], cm) and _same(got[1][rows], x[rows])
            assert _same(got[2][rows], st[rows])


# ---- evt_unfold_u8 ---------------------------------------------------------------------------
# B, H, W, C, ldo: the first three are the k7 s4 p2 band kernel at the model's ldo; the rest take
# the generic kernel (pair path straddling a pixel, single-element path, C = 1, C = 4 words)
UNFOLD_SHAPES = [
    (2, 16, 16, 3, 192),
    (1, 20, 12, 3, 192),   # non-square
    (3, 32, 32, 3, 192),
    (2, 16, 16, 3, 148),   # VW = 2
    (1, 20, 12, 3, 147),   # VW = 1
    (1, 12, 12, 1, 64),    # C = 1
    (2, 12, 8, 4, 196),    # C = 4: VW = 4
]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B,H,W,C,ldo", UNFOLD_SHAPES)
def test_unfold_u8(gpu, dtype, B, H, W, C, ldo):
    lib = _lib.load_library()
    u8 = Uint8Images(torch.from_numpy(_bytes((B, H, W, C), 100 * H + W + C)).to(gpu), **CONSTANTS[C])
    img = u8.to_float("nhwc")
    k, s, p = 7, 4, 2
    rows = B * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    nslots = 2
    new = lambda: (torch.full((rows, ldo), NAN, dtype=TDT[dtype], device=gpu),  # noqa: E731
                   torch.full((rows, nslots, 2), NAN, device=gpu))
    want, got = new(), new()
    _lib.check(lib.evt_unfold(_lib.DTYPE[dtype], 1, _p(img), B, H, W, C, k, s, p, _p(want[0]), ldo,
                              _p(want[1]), nslots, _s()))
    _lib.check(lib.evt_unfold_u8(_lib.DTYPE[dtype], _p(u8.data), B, H, W, C, k, s, p, _p(got[0]),
                                 ldo, _p(got[1]), nslots, _f4(u8.scale), _f4(u8.shift), _s()))
    torch.cuda.synchronize()
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert not torch.isnan(got[0].float()).any() and not torch.isnan(got[1]).any()
    # the first output row's window starts at (-2, -2): its padded border is 0, not shift[c]
    first = got[0][0, :k * k * C].float().view(k, k, C)
    assert (first[:2] == 0).all() and (first[:, :2] == 0).all()
    assert (got[0][:, k * k * C:] == 0).all()
    assert (first[2:, 2:] != 0).any()


# ---- models -----------------------------------------------------------------------------------
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3"


def _swin(image, window, embed, heads, dtype, lanes, gpu, batch):
    return SwinTransformer(img_size=image, patch_size=4, num_classes=19, embed_dim=embed,
                           depths=(2, 2), num_heads=heads, window_size=window, dtype=dtype, seed=3,
                           device=gpu, max_batch=batch, lanes=lanes)


# name -> (factory(lanes, gpu, batch), image size, native layout)
MODELS = {
    "vit_ref_32": (lambda l, g, b: ViT(image_size=32, patch_size=16, num_classes=16, dim=192,
                                       depth=2, heads=3, mlp_dim=768, dtype="bf16", seed=1,
                                       device=g, max_batch=b, lanes=l), 32, "nchw"),
    "vit_ref_32_f32": (lambda l, g, b: ViT(image_size=32, patch_size=16, num_classes=16, dim=192,
                                           depth=2, heads=3, mlp_dim=768, dtype="f32", seed=1,
                                           device=g, max_batch=b, lanes=l), 32, "nchw"),
    "std_28_p14": (lambda l, g, b: StandardViT(image_size=28, patch_size=14, num_classes=16,
                                               dim=384, depth=2, heads=6, dtype="bf16", seed=2,
                                               device=g, max_batch=b, lanes=l), 28, "nchw"),
    "pruned_64": (lambda l, g, b: ViT_Pruned(image_size=64, patch_size=16, num_classes=16, dim=192,
                                             depth=3, heads=3, mlp_dim=768,
                                             prune_encoding=PRUNED, dtype="bf16", seed=4,
                                             device=g, max_batch=b, lanes=l), 64, "nchw"),
    "mx8_32": (lambda l, g, b: ViT(image_size=32, patch_size=16, num_classes=16, dim=192, depth=2,
                                   heads=3, mlp_dim=768, dtype="mx8", seed=5, device=g,
                                   max_batch=b, lanes=l), 32, "nchw"),
    "t2t": (lambda l, g, b: T2T_ViT(hidden_size=256, depth=2, num_heads=4, mlp_ratio=2,
                                    dtype="bf16", seed=6, device=g, max_batch=b, lanes=l),
            224, "nhwc"),
    "t2t_f32": (lambda l, g, b: T2T_ViT(hidden_size=256, depth=2, num_heads=4, mlp_ratio=2,
                                        dtype="f32", seed=6, device=g, max_batch=b, lanes=l),
                224, "nhwc"),
    # embed 96, patch 4, window 7, bf16: the fused stem (swin_embed96_kernel) where the image size
    # is a multiple of 16, so at 112 px; at 56 px and in f32 the generic im2col path
    "swin_stem96": (lambda l, g, b: _swin(112, 7, 96, (3, 6), "bf16", l, g, b), 112, "nchw"),
    "swin_56": (lambda l, g, b: _swin(56, 7, 96, (3, 6), "bf16", l, g, b), 56, "nchw"),
    "swin_f32": (lambda l, g, b: _swin(56, 7, 96, (3, 6), "f32", l, g, b), 56, "nchw"),
    "swin_w12": (lambda l, g, b: _swin(96, 12, 128, (4, 8), "bf16", l, g, b), 96, "nchw"),
}
BATCH = 3  # splits 1 + 2 over two lanes


@functools.lru_cache(maxsize=None)
def _batch_bytes(size, seed=0):
    return _bytes((BATCH, size, size, 3), 7000 + size + seed)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_uint8_equals_fp32_of_the_normalised_image(gpu, name, lanes):
    make, size, layout = MODELS[name]
    m = make(lanes, gpu, BATCH)
    assert m.lanes() == lanes
    u8 = Uint8Images(torch.from_numpy(_batch_bytes(size)).to(gpu), **DISTINCT)
    want = m(u8.to_float(layout)).clone()
    got = m(u8).clone()
    again = m(u8).clone()
    host = m(Uint8Images(_batch_bytes(size), **DISTINCT))  # numpy in, numpy out
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert _same(got, want) and _same(again, want)
    assert isinstance(host, np.ndarray) and np.array_equal(host.view(np.int32),
                                                           want.cpu().numpy().view(np.int32))
    # the ImageNet constants (the default) on the same handle
    u8i = Uint8Images(u8.data)
    assert _same(m(u8i), m(u8i.to_float(layout)))
    with pytest.raises(ValueError, match="uint8 NHWC"):
        m(Uint8Images(u8.data[:, :-4]))
    m.close()


def test_the_stem96_case_takes_the_fused_stem(gpu):
    """A profiled forward of the 112 px case launches nothing under "patchify" (the generic path's
    im2col) and one kernel under "patch_embed"; the 56 px case launches the im2col."""
    lib = _lib.load_library()
    roles = _lib.PROF_ROLES
    for name, fused in (("swin_stem96", True), ("swin_56", False)):
        make, size, _ = MODELS[name]
        m = make(1, gpu, BATCH)
        u8 = Uint8Images(torch.from_numpy(_batch_bytes(size)).to(gpu), **DISTINCT)
        logits = torch.empty((BATCH, m.num_classes), device=gpu)
        m.forward_into(u8, logits)
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 1))
        m.forward_into(u8, logits)
        us, n = (ctypes.c_float * len(roles))(), (ctypes.c_int * len(roles))()
        _lib.check(lib.evt_model_profile_read(ctypes.c_void_p(m._handle), us, n))
        gflop, gbytes = (ctypes.c_double * len(roles))(), (ctypes.c_double * len(roles))()
        _lib.check(lib.evt_model_profile_work(ctypes.c_void_p(m._handle), gflop, gbytes))
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 0))
        assert (n[roles.index("patchify")], n[roles.index("patch_embed")]) == \
            ((0, 1) if fused else (1, 1)), name
        if fused:  # 1 byte per input element + the bf16 stream rows + their statistics
            rows = BATCH * (size // 4) ** 2
            want = (BATCH * 3 * size * size + rows * 96 * 2 + rows * 2 * 8) * 1e-9
            assert abs(gbytes[roles.index("patch_embed")] - want) <= 1e-12
        m.close()


@pytest.mark.parametrize("name", ["vit_ref_32", "std_28_p14", "t2t", "swin_stem96", "swin_f32"])
def test_features_uint8(gpu, name):
    make, size, layout = MODELS[name]
    m = make(2, gpu, BATCH)
    u8 = Uint8Images(torch.from_numpy(_batch_bytes(size)).to(gpu), **DISTINCT)
    want = m.features(u8.to_float(layout), tokens=True, taps=(0, -1), logits=True)
    got = m.features(u8, tokens=True, taps=(0, -1), logits=True)
    torch.cuda.synchronize()
    for key in ("pooled", "tokens", "logits"):
        assert _same(got[key], want[key]), key
    assert len(got["taps"]) == 2 and all(_same(a, b) for a, b in zip(got["taps"], want["taps"]))
    assert _same(m.forward_features(u8), want["pooled"])
    assert _same(got["logits"], m(u8))  # the features forward's logits are the plain forward's
    m.close()


@pytest.mark.parametrize("name", ["vit_ref_32", "t2t", "swin_stem96"])
@pytest.mark.parametrize("lanes", [1, 2])
def test_graph_replay_uint8(gpu, name, lanes):
    make, size, layout = MODELS[name]
    m = make(lanes, gpu, BATCH)
    first, second = _batch_bytes(size), _batch_bytes(size, seed=1)
    u8 = Uint8Images(torch.from_numpy(first).to(gpu), **DISTINCT)
    want = [m(Uint8Images(torch.from_numpy(b).to(gpu), **DISTINCT).to_float(layout)).clone()
            for b in (first, second)]
    logits = torch.full((BATCH, m.num_classes), NAN, device=gpu)
    m.capture_graph(u8, logits)
    m.replay_graph()
    torch.cuda.synchronize()
    assert _same(logits, want[0])
    u8.data.copy_(torch.from_numpy(second))  # refill the captured byte buffer in place
    m.replay_graph()
    torch.cuda.synchronize()
    assert _same(logits, want[1]) and not _same(want[0], want[1])
    m.close()


def test_forward_image_validation_on_a_handle(gpu):
    """The EVT_EINVAL cases that need a model: batch range, a non-finite constant among the first
    in_chans (one past them is ignored), misaligned bytes; EVT_IMG_F32 routes to the fp32 path."""
    lib = _lib.load_library()
    make, size, layout = MODELS["swin_stem96"]
    m = make(1, gpu, BATCH)
    u8 = Uint8Images(torch.from_numpy(_batch_bytes(size)).to(gpu), **DISTINCT)
    logits = torch.full((BATCH, m.num_classes), NAN, device=gpu)
    out = _lib.evt_features_args()
    out.logits = logits.data_ptr()
    h, s = ctypes.c_void_p(m._handle), _s()

    def call(args, batch=BATCH):
        return lib.evt_forward_image(h, ctypes.byref(args), batch, ctypes.byref(out), s)
    for batch in (0, BATCH + 1):
        assert call(u8.image_args(), batch) == _lib.EVT_EINVAL and b"batch" in lib.evt_last_error()
    a = u8.image_args()
    a.shift[1] = NAN
    assert call(a) == _lib.EVT_EINVAL and b"finite" in lib.evt_last_error()
    a = u8.image_args()
    a.data += 4  # the fused stem reads 16-B chunks
    assert call(a) == _lib.EVT_EINVAL and b"aligned" in lib.evt_last_error()
    empty = _lib.evt_features_args()
    assert lib.evt_forward_image(h, ctypes.byref(u8.image_args()), BATCH, ctypes.byref(empty),
                                 s) == _lib.EVT_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(logits).all()  # nothing was launched
    a = u8.image_args()
    a.scale[3] = NAN  # past in_chans = 3: not read
    _lib.check(call(a))
    want = m(u8.to_float(layout))
    torch.cuda.synchronize()
    assert _same(logits, want)
    f32 = u8.to_float(layout)
    a = u8.image_args()
    a.data, a.format = f32.data_ptr(), 0
    logits.fill_(NAN)
    _lib.check(call(a))
    torch.cuda.synchronize()
    assert _same(logits, want)
    m.close()


def test_bare_uint8_tensor_keeps_its_meaning(gpu):
    """A uint8 tensor that is not wrapped is still `.float()`: values 0..255, no normalisation."""
    make, size, _ = MODELS["vit_ref_32"]
    m = make(1, gpu, BATCH)
    raw = torch.from_numpy(_batch_bytes(size)).permute(0, 3, 1, 2).contiguous().to(gpu)
    assert _same(m(raw), m(raw.float()))
    m.close()
