"""evt_patchify_ld (patch vectors of any patch size at a padded row stride) against the torch
rearrangement of the image: columns [0, pd) in the documented K order k = (c ps + p1) ps + p2 (f32
bit for bit, bf16 equal to .bfloat16() of it), columns [pd, ldo) exactly 0 over NaN-filled
buffers, the CLS rows and their statistics equal to what evt_patchify writes, twice the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import _lib
from tests._ops import TDT, _p, _s, patchify

pytestmark = pytest.mark.gpu

# ps, HW, B, C, ldo
SHAPES = [
    (14, 28, 2, 3, 640),    # smallest np > 1
    (14, 42, 3, 3, 640),    # odd np
    (14, 70, 1, 1, 256),    # pd = 196 (the last chunk of 8 straddles pd), C != 3
    (16, 32, 2, 3, 832),    # stride wider than a 64-multiple pd
    (14, 518, 1, 3, 640),   # largest strip (87 KB of LDS), one image
]
WIDTHS = (192, 1280, 1536)  # 2, 10 and 12 statistics slots


def _slots(D):
    return 2 * ((D + 255) // 256)


def _run(dtype, img, ps, ldo, cls, pos, D):
    B, C, HW, _ = img.shape
    P = (HW // ps) ** 2
    nan = float("nan")
    out = torch.full((B * P, ldo), nan, dtype=TDT[dtype], device=img.device)
    x = torch.full((B * (P + 1), D), nan, dtype=TDT[dtype], device=img.device)
    stats = torch.full((B * (P + 1), _slots(D), 2), nan, device=img.device)
    _lib.check(_lib.load_library().evt_patchify_ld(
        _lib.DTYPE[dtype], _p(img), B, C, HW, ps, _p(out), ldo, _p(x), _p(cls), _p(pos), D,
        _p(stats), _s()))
    return out, x, stats


def _reference_rows(img, ps):
    """einops 'b c (h p1) (w p2) -> (b h w) (p1 p2 c)' (reference vit.py:31-32)."""
    B, C, HW, _ = img.shape
    n = HW // ps
    return img.reshape(B, C, n, ps, n, ps).permute(0, 2, 4, 3, 5, 1).reshape(B * n * n, ps * ps * C)


def _k_of_reference_column(ps, C):
    """Column k of evt_patchify_ld that holds element f = (p1 ps + p2) C + c of the reference."""
    f = np.arange(ps * ps * C)
    return torch.from_numpy((f % C) * ps * ps + f // C)


@pytest.fixture(scope="module")
def cls_rows(gpu):
    """The CLS rows and statistics evt_patchify writes at patch 16 (one 32 x 32 image per batch
    entry), per (dtype, D, B): the shared code the new kernel must reproduce."""
    cache = {}

    def get(dtype, D, B):
        if (dtype, D, B) not in cache:
            g = torch.Generator().manual_seed(1000 + D)
            cls = torch.randn(D, generator=g).to(gpu)
            pos = torch.randn(8, D, generator=g).to(gpu)
            img = torch.zeros((B, 3, 32, 32), device=gpu)
            _, x, st = patchify(dtype, img, 16, cls, pos, D)
            cache[(dtype, D, B)] = (cls, pos, x[::5].clone(), st[::5].clone())  # rows b * (4 + 1)
        return cache[(dtype, D, B)]
    return get


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("ps,HW,B,C,ldo", SHAPES)
def test_patchify_ld(gpu, cls_rows, dtype, ps, HW, B, C, ldo):
    g = torch.Generator().manual_seed(ps * 1000 + HW)
    img = torch.randn((B, C, HW, HW), generator=g).to(gpu)
    pd, P = ps * ps * C, (HW // ps) ** 2
    ref = _reference_rows(img, ps)
    kcol = _k_of_reference_column(ps, C).to(gpu)
    for D in WIDTHS:
        cls, pos, x16, st16 = cls_rows(dtype, D, B)
        out, x, stats = _run(dtype, img, ps, ldo, cls, pos, D)
        again = _run(dtype, img, ps, ldo, cls, pos, D)
        torch.cuda.synchronize()
        # patch columns, un-permuted by the documented K order
        got = out[:, :pd].index_select(1, kcol)
        want = ref if dtype == "f32" else ref.bfloat16()
        assert torch.equal(got.view(torch.int32 if dtype == "f32" else torch.int16),
                           want.view(torch.int32 if dtype == "f32" else torch.int16))
        # the padding: exactly +0 over the NaN fill
        pad = out[:, pd:]
        assert pad.numel() == B * P * (ldo - pd)
        assert torch.equal(pad, torch.zeros_like(pad)) and not torch.signbit(pad).any()
        # CLS rows and all statistics slots as evt_patchify writes them; nothing else touched
        rows = torch.arange(B, device=gpu) * (P + 1)
        assert torch.equal(x[rows], x16)
        assert torch.equal(stats[rows], st16)
        assert (st16[:, 1:] == 0).all() and (st16[:, 0, 1] > 0).all()
        other = torch.ones(B * (P + 1), dtype=torch.bool, device=gpu)
        other[rows] = False
        assert torch.isnan(x[other]).all() and torch.isnan(stats[other]).all()
        # a second launch over fresh NaN-filled buffers: the same bits
        for a, b in zip((out, x[rows], stats[rows]), (again[0], again[1][rows], again[2][rows])):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_patchify_ld_feeds_the_gemm(gpu):
    """The padded rows as a GEMM A operand (K-tiles of 64 over ldo = 640) against the fp64 product
    of the (p1 p2 c) vectors with the unpermuted weight: the K order and the zero weight rows of
    the padding cancel (f32 path)."""
    from tests._ops import dense, pack
    ps, HW, B, C, N = 14, 28, 2, 3, 64
    g = torch.Generator().manual_seed(5)
    img = torch.randn((B, C, HW, HW), generator=g).to(gpu)
    W = (torch.randn((ps * ps * C, N), generator=g) / 24).to(gpu)
    cls, pos = torch.zeros(N, device=gpu), torch.zeros((8, N), device=gpu)
    out, _, _ = _run("f32", img, ps, 640, cls, pos, N)
    kcol = _k_of_reference_column(ps, C).to(gpu)
    Wk = torch.empty_like(W)
    Wk[kcol] = W  # row k of the packed weight = reference row f
    wp, kpad, npad = pack(Wk, "f32")
    assert kpad == 640
    y = dense("f32", 0, out, wp, kpad, npad, out.shape[0], N)
    torch.cuda.synchronize()
    want = _reference_rows(img, ps).double() @ W.double()
    assert float((y.double() - want).abs().max()) <= 1e-4
