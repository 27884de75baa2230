"""Attention past 256 tokens per image (the streaming kernels of csrc/attention.hip): op-level
parity against an fp64 torch attention of the same rounded inputs, at the tolerances of
tests/test_gpu_ops.py (bf16 rtol = atol = 2e-2, f32 1e-4), the online-softmax edge cases, batch
independence and the limits. The head-major slice layout is reached the way the existing layout
tests reach it, through the model (tests/test_gpu_long_models.py, EVT_QKV_LAYOUT)."""
import ctypes
import functools

import pytest
import torch

from edgevisiontransformer_amd import _lib
from tests import _ops

pytestmark = pytest.mark.gpu

TOL = {"bf16": dict(rtol=2e-2, atol=2e-2), "f32": dict(rtol=1e-4, atol=1e-4)}
MAX_TOKENS = 4096  # EVT_ATTN_MAX_TOKENS (include/evt.h: N <= 4096)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _q(t64, dtype):
    return t64.to(_ops.TDT[dtype]).to(torch.float64)


def _ref(qkv64, B, N, H, hd):
    q, k, v = qkv64.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * hd ** -0.5
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhij,bhjd->bhid", p, v).permute(0, 2, 1, 3).reshape(B * N, H * hd)


@functools.lru_cache(maxsize=None)
def _case(dtype, B, N, H, hd):
    """(fp64 qkv as the kernel sees it, fp64 reference), computed once per shape and dtype."""
    qkv64 = _q(_rand((B * N, 3 * H * hd), 100 + N + hd, scale=1.5), dtype)
    return qkv64, _ref(qkv64, B, N, H, hd)


def _run(dtype, qkv64, B, N, H, hd, gpu):
    qkv = qkv64.to(_ops.TDT[dtype]).to(gpu)
    if hd == 64:
        out = _ops.attention(dtype, qkv, B, N, H)
    else:
        out = _ops.attention_hd(dtype, qkv, B, N, H, hd)
    torch.cuda.synchronize()
    return out


def _check(out, ref, dtype):
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref, **TOL[dtype])


# (2, 257, 2): one key and one query past the old limit, a last block with one valid row;
# (1, 272, 3): an exact multiple of 16; (1, 577, 2): DeiT-384; (2, 785, 1): patch 8 at 224 px;
# (1, 1025, 1): 512 px at patch 16; (1, 4096, 1): the documented limit
SHAPES = [(2, 257, 2), (1, 272, 3), (1, 577, 2), (2, 785, 1), (1, 1025, 1), (1, MAX_TOKENS, 1)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B,N,H", SHAPES)
def test_long_attention(gpu, dtype, B, N, H):
    qkv64, ref = _case(dtype, B, N, H, 64)
    _check(_run(dtype, qkv64, B, N, H, 64, gpu), ref, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("hd", [32, 40, 96, 128])
@pytest.mark.parametrize("N", [290, 577])
def test_long_attention_head_sizes(gpu, dtype, hd, N):
    B, H = 2, 2
    qkv64, ref = _case(dtype, B, N, H, hd)
    _check(_run(dtype, qkv64, B, N, H, hd, gpu), ref, dtype)


def _edge_qkv(kind, N, H):
    """qkv with q = 1 + noise, so that a key row raised by 5 a scores about +40 a."""
    qkv = _rand((N, 3 * H * 64), 7, scale=0.2)
    qkv[:, : H * 64] += 1.0
    k = qkv[:, H * 64: 2 * H * 64]
    if kind == "first":
        k[5] += 5.0
    elif kind == "last":       # the running sum and O of every earlier block rescale to 0
        k[N - 1] += 5.0
    elif kind == "rising":     # a larger spike in every 64-key block: the max moves each step
        nb = (N + 63) // 64
        for i in range(nb):
            k[min(64 * i + 7, N - 1)] += 5.0 * (i + 1) / nb
    elif kind == "equal":      # every key the same: every score of a query is equal
        k[:] = k[0].clone()
    return qkv


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["first", "last", "rising", "equal"])
def test_online_softmax_edges(gpu, dtype, kind):
    B, N, H = 1, 577, 2
    qkv64 = _q(_edge_qkv(kind, N, H), dtype)
    ref = _ref(qkv64, B, N, H, 64)
    if kind != "equal":  # the case is what it claims: one key takes nearly all the weight
        s = (qkv64[:, :64] @ qkv64[:, H * 64: H * 64 + 64].T) * 0.125
        assert float(s.max()) > 30.0
    _check(_run(dtype, qkv64, B, N, H, 64, gpu), ref, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_batch_independence_bitwise(gpu, dtype):
    B, N, H = 3, 577, 2
    qkv64 = _q(_rand((B * N, 3 * H * 64), 31, scale=1.5), dtype)
    full = _run(dtype, qkv64, B, N, H, 64, gpu)
    for b in range(B):
        one = _run(dtype, qkv64[b * N:(b + 1) * N], 1, N, H, 64, gpu)
        assert torch.equal(one, full[b * N:(b + 1) * N]), f"image {b}"


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_256_tokens_within_tolerance(gpu, dtype):
    """The last size below the streaming kernels still holds the op tolerance (that it keeps the
    one-pass kernels is attention_launch's `N > 256` test, which no output can show)."""
    qkv64, ref = _case(dtype, 2, 256, 2, 64)
    _check(_run(dtype, qkv64, 2, 256, 2, 64, gpu), ref, dtype)


def test_limits(gpu):
    lib = _lib.load_library()
    N = MAX_TOKENS + 1
    qkv = torch.zeros((N, 192), dtype=torch.bfloat16, device=gpu)
    out = torch.zeros((N, 64), dtype=torch.bfloat16, device=gpu)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dt in (0, 1):
        assert lib.evt_attention(dt, ctypes.c_void_p(qkv.data_ptr()), 192,
                                 ctypes.c_void_p(out.data_ptr()), 64, 1, N, 1, 0.125,
                                 s) == _lib.EVT_EINVAL
    assert lib.evt_attention_hd(1, ctypes.c_void_p(qkv.data_ptr()), 192,
                                ctypes.c_void_p(out.data_ptr()), 64, 1, N, 2, 32, 0.125,
                                s) == _lib.EVT_EINVAL
    with pytest.raises(_lib.EvtError) as e:
        _ops.attention_mx8(torch.zeros((257, 192), dtype=torch.bfloat16, device=gpu), 1, 257, 1)
    assert e.value.code == _lib.EVT_EINVAL
    torch.cuda.synchronize()
