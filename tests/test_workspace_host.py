"""CPU: the workspace queries against the workspace itself, buffer by buffer.

evt_{,t2t_,swin_}query_workspace sum the list of buffers the create call allocates (csrc/model.h
`WsLayout`; the `Workspace` comments name every buffer). Here the same sums are written out by
hand for one small config per family, at two batches, in bf16 and fp32 (the ViT also in MX8).
Also: the queries never decrease with the batch, and include/evt_workspace.h = its binding = the
exported symbol, with its NULL checks.
"""
import ctypes
import os
import re

import pytest

from edgevisiontransformer_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = 4096 + 256 * 256 * 256 * 4  # stream-K scratch of a bf16 handle: flags + 256 partial tiles
F32 = 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def _up(x, m):
    return (x + m - 1) // m * m


def _slots(width):  # statistics slots of a LayerNorm of this width (one per 128 of a 256-padded row)
    return 2 * ((width + 255) // 256)


def _encoder(B, T, D, inner, ffn_st, hbuf, es, bf16, mx8=False):
    """The encoder's buffers (ViT and T2T-ViT) in allocation order."""
    rows = B * T
    return [SK if bf16 else 0,                 # sk
            (rows * D + 64) * es,              # x (+ 64 zeroed slack elements)
            (rows * D + 64) * es,              # xm
            rows * _slots(D) * 2 * F32,        # sx
            rows * _slots(D) * 2 * F32,        # sm
            rows * 3 * inner * es,             # qkv
            (rows * inner + 64) * es,          # o
            hbuf,                              # hbuf
            0 if mx8 else B * ffn_st * es]     # hc (the CLS tail; none on an MX8 model)


# ---- ViT: D = 192, 3 heads of 64, depth 2, 224 / 16, FFN and head hidden 768 -----------------------
def _vit_desc(dtype, batch):
    arr = lambda v: (ctypes.c_int32 * 2)(v, v)  # noqa: E731
    return _lib.evt_vit_desc(224, 16, 3, 1000, 192, 2, 768, arr(3), arr(64), arr(768),
                             _lib.DTYPE[dtype], batch, _lib.VIT_REFERENCE, 0.0)


def _vit_sum(dtype, B):
    mx8 = dtype == "mx8"
    es = 4 if dtype == "f32" else 2
    T, P, D, inner, ffn_st, head_st, pdst = 197, 196, 192, 192, 768, 768, 768
    rows = B * T
    hbuf = max(rows * ffn_st, B * P * pdst) * es   # the patch matrix aliases it
    bufs = _encoder(B, T, D, inner, ffn_st, hbuf, es, dtype != "f32", mx8)
    bufs.append(B * head_st * es)                  # hh
    if mx8:
        qa_ld, qh_ld = max(_up(D, 128), _up(inner, 128)), _up(768, 128)
        bufs += [rows * qa_ld, rows * (qa_ld // 128) * 4,   # qa, sa
                 rows * qh_ld, rows * (qh_ld // 128) * 4,   # qh, shd
                 rows * 2 * F32]                            # lnst
    return sum(bufs)


# ---- T2T-ViT-7: 224 px, dim 256, depth 7, 4 heads, MLP 512 -----------------------------------------
def _t2t_desc(dtype, batch):
    return _lib.evt_t2t_desc(224, 3, 1000, 256, 7, 4, 512, 64, _lib.DTYPE[dtype], batch)


def _t2t_sum(dtype, B):
    es = 4 if dtype == "f32" else 2
    t1, t2, t3 = 56 * 56, 28 * 28, 14 * 14
    din1, din2 = 49 * 3, 9 * 64
    bufs = [B * max(t1 * _up(din1, 64), t2 * din2, t3 * din2) * es,            # u
            B * max(t1 * _slots(din1), t2 * _slots(din2)) * 2 * F32,          # su
            B * t1 * 3 * 64 * es,                                             # kqvb
            B * t1 * 64 * es,                                                 # pout
            B * t1 * 2 * F32,                                                 # tstats
            256,                                                              # zrow
            B * (t1 // 196 + 1) * (64 * 32 + 32) * F32]                       # part
    T, D, ffn_st = t3 + 1, 256, 512
    bufs += _encoder(B, T, D, D, ffn_st, B * T * ffn_st * es, es, dtype != "f32")
    return sum(bufs)


# ---- Swin: 56 px, patch 4, window 7, stages (96, 3 heads, depth 2), (192, 6 heads, depth 2) ------
def _swin_desc(dtype, batch):
    d = _lib.evt_swin_desc()
    d.image_size, d.patch_size, d.in_chans, d.num_classes = 56, 4, 3, 37
    d.embed_dim, d.num_stages, d.window_size, d.mlp_ratio = 96, 2, 7, 4.0
    for i, (dp, h) in enumerate(zip((2, 2), (3, 6))):
        d.depths[i], d.num_heads[i] = dp, h
    d.dtype, d.max_batch = _lib.DTYPE[dtype], batch
    return d


def _swin_sum(dtype, B):
    es = 4 if dtype == "f32" else 2
    stages = [(14 * 14, 96, 384), (7 * 7, 192, 768)]  # tokens, width, MLP width
    stream = max(B * t * c for t, c, _ in stages)
    stats = max(B * t * _slots(c) * 2 for t, c, _ in stages)
    qkv = max(B * t * 3 * c for t, c, _ in stages)
    # hbuf: the MLP hidden, the merge gather (4 x 96 columns of stage 2's rows), the patch matrix
    hbuf = max(max(B * t * m for t, _, m in stages), B * 49 * 4 * 96, B * 196 * _up(48, 64))
    bufs = [(stream + 64) * es, (stream + 64) * es,  # x, xm (+ 64 zeroed slack elements)
            stats * F32, stats * F32,                # sx, sm
            qkv * es,                                # qkv
            (stream + 64) * es,                      # o
            hbuf * es,                               # hbuf
            B * 192 * es,                            # pooled
            SK if dtype == "bf16" else 0]            # sk
    return sum(bufs)


FAMILIES = {"vit": ("evt_query_workspace", _vit_desc, _vit_sum),
            "t2t": ("evt_t2t_query_workspace", _t2t_desc, _t2t_sum),
            "swin": ("evt_swin_query_workspace", _swin_desc, _swin_sum)}
CASES = [(f, dt) for f in FAMILIES for dt in ("bf16", "f32")] + [("vit", "mx8")]


def _query(lib, family, dtype, batch):
    fn, desc, _ = FAMILIES[family]
    d, out = desc(dtype, batch), ctypes.c_size_t()
    assert getattr(lib, fn)(ctypes.byref(d), batch, ctypes.byref(out)) == _lib.EVT_OK, \
        lib.evt_last_error()
    return out.value


@pytest.mark.parametrize("family,dtype", CASES)
@pytest.mark.parametrize("batch", [1, 3])
def test_query_is_the_sum_of_the_buffers(lib, family, dtype, batch):
    assert _query(lib, family, dtype, batch) == FAMILIES[family][2](dtype, batch)


@pytest.mark.parametrize("family,dtype", CASES)
def test_query_never_decreases_with_the_batch(lib, family, dtype):
    got = [_query(lib, family, dtype, b) for b in range(1, 10)]
    assert got == sorted(got)


def test_header_binding_and_exports_agree(lib):
    txt = open(os.path.join(REPO, "include", "evt_workspace.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.WORKSPACE_SIGNATURES) == ["evt_model_workspace_bytes"]
    assert '#include "evt_workspace.h"' in open(os.path.join(REPO, "include", "evt.h")).read()
    from edgevisiontransformer_amd import build
    assert any(h.endswith("evt_workspace.h") for h in build.HEADERS)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.WORKSPACE_SIGNATURES[name][1]


def test_null_arguments(lib):
    out = ctypes.c_size_t(7)
    assert lib.evt_model_workspace_bytes(None, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert out.value == 7
    assert lib.evt_model_workspace_bytes(None, None) == _lib.EVT_EINVAL
