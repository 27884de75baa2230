"""Kernel-level parity on the GPU: each HIP kernel vs an fp64 CPU restatement of the same op on
the same (dtype-rounded) inputs. Tolerances are stated per dtype in each test."""
import math

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import _lib
from oracle import vit_ref
from tests import _ops

pytestmark = pytest.mark.gpu

# bf16 output rounding is 2^-9 relative; fp32 MFMA is an exact f32 fmaf chain.
TOL = {"bf16": dict(rtol=1.6e-2, atol=1.6e-2), "f32": dict(rtol=5e-5, atol=5e-5)}


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _q(t64, dtype):
    """Round an fp64 CPU tensor to the kernel dtype and back (what the kernel actually sees)."""
    return t64.to(_ops.TDT[dtype]).to(torch.float64)


def _gelu(x):
    return x * 0.5 * (1.0 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("M,K,N", [(197, 192, 576), (394, 768, 2304), (131, 320, 37 * 4),
                                   (1000, 576, 192), (64, 64, 1000), (257, 3072, 768),
                                   (300, 128, 200)])
@pytest.mark.parametrize("flags", [0, 3, 21, 17])
@pytest.mark.parametrize("variant", [1, 2, 8, 9, 0])
def test_dense(gpu, dtype, M, K, N, flags, variant):
    """variant 1: 128x128-tile kernel; 2: 256x256-tile kernel (bf16 only; f32 ignores it)."""
    with _ops.gemm_variant(variant):
        _dense_case(gpu, dtype, M, K, N, flags)


def _dense_case(gpu, dtype, M, K, N, flags):
    A64 = _rand((M, K), 1)
    W64 = _rand((K, N), 2, scale=1.0 / math.sqrt(K))
    b64 = _rand((N,), 3, scale=0.1)
    R64 = _rand((M, N), 4)
    A = A64.to(_ops.TDT[dtype]).to(gpu)
    W = W64.float().to(gpu)
    wp, kpad, npad = _ops.pack(W, dtype)
    kw = {}
    if flags & _lib.EPI_BIAS:
        bias = torch.zeros(npad, dtype=torch.float32, device=gpu)
        bias[:N] = b64.float().to(gpu)
        kw["bias"] = bias
    if flags & _lib.EPI_RESID:
        kw["resid"] = R64.to(_ops.TDT[dtype]).to(gpu)
    if kpad != K:
        Ap = torch.zeros((M, kpad), dtype=A.dtype, device=gpu)
        Ap[:, :K] = A
        A = Ap
    C = _ops.dense(dtype, flags, A, wp, kpad, npad, M, N, **kw)
    torch.cuda.synchronize()
    ref = _q(A64, dtype) @ _q(W64.float().double(), dtype)
    if flags & _lib.EPI_BIAS:
        ref = ref + b64.float().double()
    if flags & _lib.EPI_GELU:
        ref = _gelu(ref)
    if flags & _lib.EPI_RESID:
        ref = ref + _q(R64, dtype)
    got = C.double().cpu()
    tol = TOL["f32"] if (dtype == "f32") else (TOL["bf16"] if not (flags & _lib.EPI_OUT_F32)
                                                else dict(rtol=1e-3, atol=1e-3))
    torch.testing.assert_close(got, ref, **tol)


@pytest.mark.parametrize("variant", [0, 9])
@pytest.mark.parametrize("resid", [False, True])
def test_dense_huge_leading_dims(gpu, variant, resid):
    """Leading dimensions past the big kernels' 32-bit in-tile offsets (gemm.hip BIG_MAX_LD:
    ~2.8M elements; the LDS-DMA lane offsets wrap past 8.4M, the epilogue ranges past 4.2M) take
    the 128 x 128 kernel, even under a forced persistent variant (9): A, C (and the residual)
    rows 9M elements apart; bias + GELU into bf16, or bias + residual into fp32."""
    M, K, N, LD = 300, 768, 768, 9_000_000
    A64, W64 = _rand((M, K), 11), _rand((K, N), 12, scale=1.0 / math.sqrt(K))
    b64, R64 = _rand((N,), 13, scale=0.1), _rand((M, N), 14)
    A = torch.empty((M, LD), dtype=torch.bfloat16, device=gpu)
    A[:, :K] = A64.to(torch.bfloat16).to(gpu)
    wp, kpad, npad = _ops.pack(W64.float().to(gpu), "bf16")
    bias = torch.zeros(npad, dtype=torch.float32, device=gpu)
    bias[:N] = b64.float().to(gpu)
    kw = {}
    if resid:
        flags = _lib.EPI_BIAS | _lib.EPI_RESID | _lib.EPI_OUT_F32
        R = torch.empty((M, LD), dtype=torch.bfloat16, device=gpu)
        R[:, :N] = R64.to(torch.bfloat16).to(gpu)
        kw["resid"] = R
        C = torch.zeros((M, LD), dtype=torch.float32, device=gpu)
    else:
        flags = _lib.EPI_BIAS | _lib.EPI_GELU
        C = torch.zeros((M, LD), dtype=torch.bfloat16, device=gpu)
    with _ops.gemm_variant(variant):
        _ops.dense("bf16", flags, A, wp, kpad, npad, M, N, ldc=LD, bias=bias, C=C, **kw)
    ref = _q(A64, "bf16") @ _q(W64, "bf16") + b64
    ref = ref + _q(R64, "bf16") if resid else _gelu(ref)
    got = C[:, :N].double().cpu()
    torch.testing.assert_close(got, ref, **(dict(rtol=1e-3, atol=1e-3) if resid else TOL["bf16"]))
    assert not C[:, N:N + 64].any()  # nothing written past the N columns


# only the valid (K, splits) pairs: the padded K must split into whole 64-deep K-tiles
_SPLITK_SHAPES = [(M, K, N, s) for (M, K, N) in [(1, 768, 3072), (37, 3072, 1000), (130, 768, 148),
                                                  (257, 1536, 200)]
                  for s in (2, 4, 8) if K % (s * 64) == 0]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("M,K,N,splits", _SPLITK_SHAPES)
@pytest.mark.parametrize("flags", [_lib.EPI_BIAS | _lib.EPI_GELU, _lib.EPI_BIAS | _lib.EPI_OUT_F32,
                                   _lib.EPI_BIAS | _lib.EPI_GELU | _lib.EPI_OUT_F32])
def test_dense_splitk(gpu, dtype, M, K, N, flags, splits):
    """evt_dense_splitk (the classifier head path, vit.py:38-39,55): S K-slices with fp32 partials
    and a fixed-order reduce + bias / GELU, against the plain Dense on the same operands (the only
    difference is the fp32 summation order: within one output rounding) and an fp64 reference;
    M edges (1, 37, 130, 257 rows) and N not a multiple of the 128-column tile."""
    A64, W64, b64 = _rand((M, K), 31), _rand((K, N), 32, 1 / math.sqrt(K)), _rand((N,), 33, 0.1)
    A = A64.to(_ops.TDT[dtype]).to(gpu)
    wp, kpad, npad = _ops.pack(W64.float().to(gpu), dtype)
    bias = torch.zeros(npad, device=gpu)
    bias[:N] = b64.float().to(gpu)
    got = _ops.dense_splitk(dtype, flags, A, wp, kpad, npad, M, N, splits, bias=bias)
    # GELU with fp32 output exists only on the split-K path (evt_dense has no such flag set)
    plain = None if flags == _lib.EPI_BIAS | _lib.EPI_GELU | _lib.EPI_OUT_F32 else \
        _ops.dense(dtype, flags, A, wp, kpad, npad, M, N, bias=bias)
    torch.cuda.synchronize()
    ref = _q(A64, dtype) @ _q(W64.float().double(), dtype) + b64.float().double()
    if flags & _lib.EPI_GELU:
        ref = _gelu(ref)
    out_f32 = bool(flags & _lib.EPI_OUT_F32)
    tol = TOL["f32"] if dtype == "f32" or out_f32 else TOL["bf16"]
    if dtype == "bf16" and out_f32:
        tol = dict(rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(got.double().cpu(), ref, **tol)
    if plain is not None:
        same = dict(rtol=1e-5, atol=1e-5) if out_f32 or dtype == "f32" else dict(rtol=8e-3, atol=8e-3)
        torch.testing.assert_close(got.float(), plain.float(), **same)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_dense_patch_embed_remap(gpu, dtype):
    B, P, K, N = 3, 196, 768, 192
    A64, W64, b64 = _rand((B * P, K), 5), _rand((K, N), 6, 1 / 28.0), _rand((N,), 7, 0.1)
    pos64 = _rand((P + 1, N), 8, 0.05)
    A = A64.to(_ops.TDT[dtype]).to(gpu)
    wp, kpad, npad = _ops.pack(W64.float().to(gpu), dtype)
    bias = torch.zeros(npad, device=gpu)
    bias[:N] = b64.float().to(gpu)
    pos = pos64.float().to(gpu)
    C = torch.full((B * (P + 1), N), 7.0, device=gpu)
    _ops.dense(dtype, _lib.EPI_BIAS | _lib.EPI_POS | _lib.EPI_OUT_F32, A, wp, kpad, npad, B * P, N,
               bias=bias, pos=pos, P=P, C=C)
    torch.cuda.synchronize()
    ref = (_q(A64, dtype) @ _q(W64.float().double(), dtype) + b64.float().double()).reshape(B, P, N)
    ref = ref + pos64.float().double()[1:]
    got = C.double().cpu().reshape(B, P + 1, N)
    assert torch.all(got[:, 0] == 7.0), "CLS rows must be left untouched by the patch GEMM"
    torch.testing.assert_close(got[:, 1:], ref, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("B", [120, 131])
def test_dense_patch_embed_persistent(gpu, B):
    """The model's bf16 patch GEMM at a batch that takes the persistent kernel (EPI_POS with the
    bf16 position table in resid): + bias + pos[t+1], rows remapped past the CLS rows, statistics
    of the stored rows; CLS rows and their statistics untouched. B = 131: an M edge mid-image."""
    P, K, N = 196, 768, 768
    A64, W64, b64 = _rand((B * P, K), 15), _rand((K, N), 16, 1 / 28.0), _rand((N,), 17, 0.1)
    pos64 = _rand((P + 1, N), 18, 0.05)
    A = A64.to(torch.bfloat16).to(gpu)
    wp, kpad, npad = _ops.pack(W64.float().to(gpu), "bf16")
    bias = torch.zeros(npad, device=gpu)
    bias[:N] = b64.float().to(gpu)
    pos = pos64.float().to(gpu)
    pos_h = pos.to(torch.bfloat16)
    C = torch.full((B * (P + 1), N), 7.0, dtype=torch.bfloat16, device=gpu)
    st = torch.full((B * (P + 1), _nslots(N), 2), float("nan"), device=gpu)
    _ops.dense("bf16", _lib.EPI_BIAS | _lib.EPI_POS | _lib.EPI_STATS, A, wp, kpad, npad, B * P, N,
               bias=bias, pos=pos, P=P, C=C, resid=pos_h, stats_out=st, ln_width=N)
    torch.cuda.synchronize()
    ref = (_q(A64, "bf16") @ _q(W64.float().double(), "bf16") + b64.float().double()).reshape(B, P, N)
    ref = ref + _q(pos64.float().double(), "bf16")[1:]
    got = C.double().cpu().reshape(B, P + 1, N)
    assert torch.all(got[:, 0] == 7.0), "CLS rows must be left untouched by the patch GEMM"
    torch.testing.assert_close(got[:, 1:], ref, rtol=2e-2, atol=2e-2)
    stc = st.cpu().reshape(B, P + 1, -1, 2)
    assert torch.isnan(stc[:, 0]).all(), "CLS-row statistics must be left untouched"
    rows = got[:, 1:].reshape(B * P, N)
    torch.testing.assert_close(stc[:, 1:].double().sum(2).reshape(B * P, 2), _stats32(rows).double().sum(1),
                               rtol=1e-4, atol=1e-2)


def _attn_ref(qkv64, B, N, H):
    q, k, v = qkv64.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * 0.125
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhij,bhjd->bhid", p, v).permute(0, 2, 1, 3).reshape(B * N, H * 64)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (1, 197, 12), (3, 50, 2), (2, 256, 1),
                                   (1, 1, 2), (2, 129, 4), (1, 224, 6)])
def test_attention(gpu, dtype, B, N, H):
    """Random inputs at a few N. Both sides of every kernel / tile boundary, with inputs on which
    one miscounted key shows: tests/test_gpu_attn_probes.py."""
    qkv64 = _rand((B * N, 3 * H * 64), 11, scale=1.5)
    qkv = qkv64.to(_ops.TDT[dtype]).to(gpu)
    out = _ops.attention(dtype, qkv, B, N, H)
    torch.cuda.synchronize()
    ref = _attn_ref(_q(qkv64, dtype), B, N, H)
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == "bf16" else dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.double().cpu(), ref, **tol)


def _attn_ref_hd(qkv64, B, N, H, hd):
    q, k, v = qkv64.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * hd ** -0.5
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhij,bhjd->bhid", p, v).permute(0, 2, 1, 3).reshape(B * N, H * hd)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B,N,H,hd", [(2, 197, 1, 96), (1, 197, 8, 96), (2, 197, 6, 32),
                                      (2, 197, 8, 10), (1, 50, 3, 128), (3, 129, 2, 48),
                                      (1, 256, 2, 72), (2, 1, 4, 24), (1, 64, 5, 100),
                                      (2, 197, 2, 64)])
def test_attention_any_head_size(gpu, dtype, B, N, H, hd):
    """evt_attention_hd against a torch fp64 attention of the same rounded inputs: h_k other than
    64 (the generic kernels, features zero-padded to 32 / 64; odd sizes take the element-wise
    paths), 64 (the tuned kernels through the same entry point)."""
    qkv64 = _rand((B * N, 3 * H * hd), 13, scale=1.5)
    qkv = qkv64.to(_ops.TDT[dtype]).to(gpu)
    full = torch.full((B * N, H * hd + 8), 7.0, dtype=_ops.TDT[dtype], device=gpu)
    out = full[:, : H * hd]
    _ops.attention_hd(dtype, qkv, B, N, H, hd, out=out)
    torch.cuda.synchronize()
    ref = _attn_ref_hd(_q(qkv64, dtype), B, N, H, hd)
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == "bf16" else dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.double().cpu(), ref, **tol)
    assert torch.all(full[:, H * hd:] == 7.0), "columns past H * h_k must stay untouched"


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_attention_peaked_softmax(gpu, dtype):
    """One key dominates every query (scores ~ +40): exercises the max-subtraction path."""
    B, N, H = 1, 197, 2
    qkv64 = _rand((B * N, 3 * H * 64), 12, scale=0.2)
    qkv64[:, : H * 64] += 1.0   # q
    qkv64[5, H * 64: 2 * H * 64] += 5.0  # key 5 spikes
    qkv = qkv64.to(_ops.TDT[dtype]).to(gpu)
    out = _ops.attention(dtype, qkv, B, N, H)
    torch.cuda.synchronize()
    ref = _attn_ref(_q(qkv64, dtype), B, N, H)
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == "bf16" else dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.double().cpu(), ref, **tol)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("rows,D", [(197, 192), (394, 384), (1000, 768), (3, 64), (5, 1024)])
def test_layernorm(gpu, dtype, rows, D):
    x64 = _rand((rows, D), 21, 3.0) + 0.5
    g64, b64 = 1.0 + _rand((D,), 22, 0.1), _rand((D,), 23, 0.1)
    y = _ops.layernorm(dtype, x64.float().to(gpu), g64.float().to(gpu), b64.float().to(gpu))
    torch.cuda.synchronize()
    ref = torch.from_numpy(vit_ref.layer_norm(x64.float().double().numpy(), g64.float().double().numpy(),
                                              b64.float().double().numpy()))
    tol = TOL["bf16"] if dtype == "bf16" else dict(rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(y.double().cpu(), ref, **tol)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("channel_major", [False, True])
def test_patchify(gpu, dtype, channel_major):
    """evt_patchify: the reference (p1 p2 c) vectors; evt_patchify_cm (the model's layout): the
    same vectors with K permuted to (c p1 p2), bit-exact either way."""
    B, C, HW, ps, D = 2, 3, 224, 16, 192
    img = _rand((B, C, HW, HW), 31).float()
    cls, pos = _rand((D,), 32).float(), _rand((197, D), 33).float()
    out, x, stats = _ops.patchify(dtype, img.to(gpu), ps, cls.to(gpu), pos.to(gpu), D,
                                  channel_major=channel_major)
    torch.cuda.synchronize()
    ref = vit_ref.patchify_nchw(img.numpy(), ps).reshape(B * 196, -1)
    if channel_major:  # (p1 p2 c) -> (c p1 p2)
        ref = ref.reshape(B * 196, ps, ps, C).transpose(0, 3, 1, 2).reshape(B * 196, -1)
    exp = torch.from_numpy(ref).to(_ops.TDT[dtype])
    assert torch.equal(out.cpu(), exp), "patchify is a pure permutation: must be bit-exact"
    xr = x.cpu().reshape(B, 197, D)
    cls_row = (cls + pos[0]).to(_ops.TDT[dtype])
    assert torch.equal(xr[:, 0], cls_row.expand(B, D))
    q = cls_row.double()
    st = stats.cpu().reshape(B, 197, -1, 2)[:, 0].double()
    torch.testing.assert_close(st[:, 0, 0], q.sum().expand(B), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(st[:, 0, 1], (q * q).sum().expand(B), rtol=1e-5, atol=1e-4)
    assert torch.all(st[:, 1:] == 0)


def _ln64(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def _nslots(D):
    return 2 * ((D + 255) // 256)


def _stats32(xq):
    """[rows][S][2] slot statistics with the whole row in slot 0 (include/evt.h layout)."""
    S = _nslots(xq.shape[-1])
    st = torch.zeros((xq.shape[0], S, 2), dtype=torch.float32)
    st[:, 0, 0], st[:, 0, 1] = xq.sum(-1).float(), (xq * xq).sum(-1).float()
    return st


def _accepted(variant):
    """The variant these cases run under. 10 was a number of the removed diagnostic build: the library
    must reject it, and its cases exercise the automatic selection (0), which is what they have
    always run. Every other variant is passed on for _ops.gemm_variant to assert."""
    if variant != 10:
        return variant
    assert _lib.load_library().evt_set_gemm_variant(10) == _lib.EVT_EINVAL
    return 0


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("variant", [1, 2, 8, 9, 10, 0, 30, 31])  # 10: see _accepted
@pytest.mark.parametrize("M,D,N,gelu", [(300, 768, 2304, False), (600, 384, 1536, True),
                                        (197, 192, 537, True), (2900, 768, 3072, True)])
def test_dense_layernorm_folded_input(gpu, dtype, variant, M, D, N, gelu):
    """QKV / FC1 as run in the model: A = raw stream x, LayerNorm applied per row in the epilogue
    from (sum, sumsq) statistics, gamma folded into the packed weights (gemm.hip header)."""
    x64 = _rand((M, D), 41, 1.3) + 0.3
    g64, be64 = 1.0 + _rand((D,), 42, 0.1), _rand((D,), 43, 0.1)
    W64, bias64 = _rand((D, N), 44, 1 / math.sqrt(D)), _rand((N,), 45, 0.05)
    xq = _q(x64, dtype)
    W = W64.float().to(gpu)
    g, be, bias = g64.float().to(gpu), be64.float().to(gpu), bias64.float().to(gpu)
    wp, kpad, npad = _ops.pack(W, dtype, row_scale=g)
    colsum, cvec = _ops.ln_fold(dtype, wp, kpad, npad, W, be, bias)
    flags = _lib.EPI_LNIN | _lib.EPI_BIAS | (_lib.EPI_GELU if gelu else 0)
    with _ops.gemm_variant(_accepted(variant)):
        C = _ops.dense(dtype, flags, xq.to(_ops.TDT[dtype]).to(gpu), wp, kpad, npad, M, N,
                       bias=cvec, colsum=colsum, stats_in=_stats32(xq).to(gpu), ln_width=D)
    ref = _ln64(xq, g64.float().double(), be64.float().double()) @ W64.float().double() \
        + bias64.float().double()
    if gelu:
        ref = _gelu(ref)
    tol = dict(rtol=2.5e-2, atol=2.5e-2) if dtype == "bf16" else dict(rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(C.double().cpu(), ref, **tol)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("variant", [1, 2, 8, 9, 10, 0, 30, 31])  # 10: see _accepted
@pytest.mark.parametrize("M,K,D", [(300, 768, 768), (513, 3072, 384), (197, 576, 192),
                                   (2900, 768, 768), (12608, 3072, 768), (1, 384, 384),
                                   (129, 1152, 384), (50432, 384, 384)])
def test_dense_layernorm_residual_and_stats(gpu, dtype, variant, M, K, D):
    """out-proj / FC2 as run in the model: + bias + LN(resid) residual (the reference's quirk:
    the residual is the normalised input), storing the new stream and its row statistics."""
    A64, W64, b64 = _rand((M, K), 51), _rand((K, D), 52, 1 / math.sqrt(K)), _rand((D,), 53, 0.1)
    x64 = _rand((M, D), 54, 1.1) - 0.2
    g64, be64 = 1.0 + _rand((D,), 55, 0.1), _rand((D,), 56, 0.1)
    Aq, xq = _q(A64, dtype), _q(x64, dtype)
    wp, kpad, npad = _ops.pack(W64.float().to(gpu), dtype)
    bias = torch.zeros(npad, device=gpu)
    bias[:D] = b64.float().to(gpu)
    stats_out = torch.full((M, _nslots(D), 2), float("nan"), device=gpu)
    with _ops.gemm_variant(_accepted(variant)):
        C = _ops.dense(dtype, _lib.EPI_BIAS | _lib.EPI_RESID | _lib.EPI_RESLN | _lib.EPI_STATS,
                       Aq.to(_ops.TDT[dtype]).to(gpu), wp, kpad, npad, M, D, bias=bias,
                       resid=xq.to(_ops.TDT[dtype]).to(gpu), rstats=_stats32(xq).to(gpu),
                       rgamma=g64.float().to(gpu), rbeta=be64.float().to(gpu),
                       stats_out=stats_out, ln_width=D)
    ref = Aq @ _q(W64.float().double(), dtype) + b64.float().double() \
        + _ln64(xq, g64.float().double(), be64.float().double())
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == "bf16" else dict(rtol=1e-4, atol=1e-4)
    got = C.double().cpu()
    torch.testing.assert_close(got, ref, **tol)
    # statistics are of the values as stored
    torch.testing.assert_close(stats_out.double().cpu().sum(1), _stats32(got).double().sum(1),
                               rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("M,K,N", [(513, 384, 384), (3000, 1536, 384), (12608, 768, 768), (1, 128, 1152),
                                   (777, 768, 200)])
@pytest.mark.parametrize("variant", [30, 0])
def test_dense_residual_plain_stats(gpu, M, K, N, variant):
    """The Swin proj / FC2 form (BIAS|RESID|STATS: x + f(LN(x)) with the plain residual) on the
    128 x 384 persistent tiles (variant 30) and the automatic choice: values and the row
    statistics of the stored values (every slot written, the slots past 3 * N / 384 zero)."""
    A64, W64, b64 = _rand((M, K), 61), _rand((K, N), 62, 1 / math.sqrt(K)), _rand((N,), 63, 0.1)
    R64 = _rand((M, N), 64)
    Aq, Rq = _q(A64, "bf16"), _q(R64, "bf16")
    wp, kpad, npad = _ops.pack(W64.float().to(gpu), "bf16")
    bias = torch.zeros(npad, device=gpu)
    bias[:N] = b64.float().to(gpu)
    st = torch.full((M, _nslots(N), 2), float("nan"), device=gpu)
    with _ops.gemm_variant(variant):
        C = _ops.dense("bf16", _lib.EPI_BIAS | _lib.EPI_RESID | _lib.EPI_STATS,
                       Aq.to(torch.bfloat16).to(gpu), wp, kpad, npad, M, N, bias=bias,
                       resid=Rq.to(torch.bfloat16).to(gpu), stats_out=st, ln_width=N)
    ref = Aq @ _q(W64.float().double(), "bf16") + b64.float().double() + Rq
    got = C.double().cpu()
    torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(st.double().cpu().sum(1), _stats32(got).double().sum(1),
                               rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("flags,variant", [("resln", 30), ("lnin_gelu", 30), ("resln", 0),
                                           ("resln_k3072", 0)])
def test_dense_rows_independent_of_position(gpu, flags, variant):
    """128 x 384 tiles (variant 30) and the automatic 256 x 256 persistent kernel (K = 768 and
    3072): a row's outputs (and statistics) are the same bits wherever it sits in the batch (tile
    offsets, neighbours, last partial panel): the product contract's batch-position independence
    for a fixed kernel selection."""
    M, K, N, shift = 1000, 768, 768, 37
    if flags == "resln_k3072":
        flags, K = "resln", 3072
    A64 = _rand((M + shift, K), 71)
    W64, b64 = _rand((K, N), 72, 1 / math.sqrt(K)), _rand((N,), 73, 0.1)
    x64 = _rand((M + shift, N), 74)
    g64, be64 = 1.0 + _rand((N,), 75, 0.1), _rand((N,), 76, 0.1)
    outs = []
    with _ops.gemm_variant(variant):
        for off in (0, shift):
            Aq = _q(A64[off:off + M], "bf16").to(torch.bfloat16).to(gpu)
            xq = _q(x64[off:off + M], "bf16")
            if flags == "resln":
                wp, kpad, npad = _ops.pack(W64.float().to(gpu), "bf16")
                bias = torch.zeros(npad, device=gpu)
                bias[:N] = b64.float().to(gpu)
                st = torch.full((M, _nslots(N), 2), float("nan"), device=gpu)
                C = _ops.dense("bf16", _lib.EPI_BIAS | _lib.EPI_RESID | _lib.EPI_RESLN | _lib.EPI_STATS,
                               Aq, wp, kpad, npad, M, N, bias=bias,
                               resid=xq.to(torch.bfloat16).to(gpu), rstats=_stats32(xq).to(gpu),
                               rgamma=g64.float().to(gpu), rbeta=be64.float().to(gpu),
                               stats_out=st, ln_width=N)
            else:
                g = g64.float().to(gpu)
                wp, kpad, npad = _ops.pack(W64.float().to(gpu), "bf16", row_scale=g)
                colsum, cvec = _ops.ln_fold("bf16", wp, kpad, npad, W64.float().to(gpu),
                                            be64.float().to(gpu), b64.float().to(gpu))
                C = _ops.dense("bf16", _lib.EPI_LNIN | _lib.EPI_BIAS | _lib.EPI_GELU,
                               xq.to(torch.bfloat16).to(gpu), wp, kpad, npad, M, N, bias=cvec,
                               colsum=colsum, stats_in=_stats32(xq).to(gpu), ln_width=N)
                st = None
            torch.cuda.synchronize()
            outs.append((C.cpu(), None if st is None else st.cpu()))
    (c0, s0), (c1, s1) = outs
    assert torch.equal(c0[shift:], c1[:M - shift])
    if s0 is not None:
        assert torch.equal(s0[shift:], s1[:M - shift])
