"""Op-level parity for the Dense epilogues, statistics layouts, strides and attention arguments that
only whole models reached before: flag sets 289 (LN-folded FC1 + erf GELU), 161 (LN-folded
patch-merge reduction + statistics) and 49 with stats_step (the classifier on the CLS rows), padded
row pitches, statistics spread over the slots as a preceding EPI_STATS GEMM leaves them, a
non-default LayerNorm epsilon, rows that are hard for the folded LayerNorm, the GELU forms point by
point, and ldq / ldo / scale of evt_attention(_hd).

Every reference is fp64 torch on the operands as the kernel sees them: activations rounded to the
kernel dtype, LN-folded weights as evt_pack_weight rounds them (fp32 W * gamma, then the dtype).
f32 has one GEMM kernel (evt_set_gemm_variant selects among the bf16 ones), so f32 cases run once."""
import functools
import math

import pytest
import torch

from edgevisiontransformer_amd import _lib
from tests import _ops
from tests.test_gpu_ops import _ln64, _nslots, _q, _rand, _stats32

pytestmark = pytest.mark.gpu

F33 = _lib.EPI_LNIN | _lib.EPI_BIAS
F35 = F33 | _lib.EPI_GELU
F49 = F33 | _lib.EPI_OUT_F32
F161 = F33 | _lib.EPI_STATS
F289 = F33 | _lib.EPI_GELU_ERF
F197 = _lib.EPI_BIAS | _lib.EPI_RESID | _lib.EPI_RESLN | _lib.EPI_STATS
# tolerances of test_dense_layernorm_folded_input / test_dense_layernorm_residual_and_stats
LNIN_TOL = {"bf16": dict(rtol=2.5e-2, atol=2.5e-2), "f32": dict(rtol=2e-4, atol=2e-4)}
RESLN_TOL = {"bf16": dict(rtol=2e-2, atol=2e-2), "f32": dict(rtol=1e-4, atol=1e-4)}
STATS_TOL = dict(rtol=1e-4, atol=1e-2)


def _dv(variants):
    """(dtype, variant) pairs: every bf16 kernel variant, the one f32 kernel."""
    return [("bf16", v) for v in variants] + [("f32", 0)]


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_tanh(x):
    return x * 0.5 * (1.0 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def _stats_spread(xq):
    """[rows][S][2] slot statistics as an EPI_STATS GEMM leaves them: slot j holds the exact (sum,
    sumsq) of columns [128 j, 128 j + 128), slots past the last slab zero."""
    rows, D = xq.shape
    st = torch.zeros((rows, _nslots(D), 2), dtype=torch.float32)
    for j in range((D + 127) // 128):
        slab = xq[:, 128 * j: 128 * (j + 1)]
        st[:, j, 0], st[:, j, 1] = slab.sum(-1).float(), (slab * slab).sum(-1).float()
    return st


HARD_MEAN = {"bf16": 32.0, "f32": 8.0}  # over sigma 0.5: ratios 64 and 16 (test_hard_rows)


def _rows(x64, kind, dtype):
    """plain: as drawn. small: the first half of the rows scaled to sigma ~ 2e-3 (variance ~ 4e-6,
    where eps 1e-6 and 1e-5 give r = 447 and 267). hard: rows 0..6 with a large mean against
    their spread, row 7 constant 3.0."""
    x64 = x64.clone()
    if kind == "small":
        h = x64.shape[0] // 2
        x64[:h] = _rand((h, x64.shape[1]), 991, 2e-3)
    elif kind == "hard":
        x64[:7] = HARD_MEAN[dtype] + _rand((7, x64.shape[1]), 992, 0.5)
        x64[7] = 3.0
    return x64


@functools.lru_cache(maxsize=None)
def _lnin_host(dtype, M, K, N, kind="plain"):
    """fp64 host operands of an LN-folded Dense (all fp32-representable; x rounded to dtype)."""
    xq = _q(_rows(_rand((M, K), 41, 1.3) + 0.3, kind, dtype), dtype)
    g = (1.0 + _rand((K,), 42, 0.1)).float().double()
    be = _rand((K,), 43, 0.1).float().double()
    W = _rand((K, N), 44, 1 / math.sqrt(K)).float().double()
    bias = _rand((N,), 45, 0.05).float().double()
    return xq, g, be, W, bias


def _packed64(W, g, dtype):
    """The folded weights as evt_pack_weight stores them: fp32 W[k][n] * gamma[k], then the dtype."""
    return _q((W.float() * g.float()[:, None]).double(), dtype)


def _lnin_ref_of(xq, g, be, W, bias, dtype, eps):
    mu = xq.mean(-1, keepdim=True)
    var = ((xq - mu) ** 2).mean(-1, keepdim=True)
    return (xq - mu) / torch.sqrt(var + eps) @ _packed64(W, g, dtype) + (be @ W + bias)


@functools.lru_cache(maxsize=None)
def _lnin_ref(dtype, M, K, N, kind="plain", eps=1e-5):
    return _lnin_ref_of(*_lnin_host(dtype, M, K, N, kind), dtype, eps)


def _lnin_weights(gpu, dtype, g, be, W, bias):
    Wd = W.float().to(gpu)
    wp, kpad, npad = _ops.pack(Wd, dtype, row_scale=g.float().to(gpu))
    colsum, cvec = _ops.ln_fold(dtype, wp, kpad, npad, Wd, be.float().to(gpu), bias.float().to(gpu))
    return wp, kpad, npad, colsum, cvec


def _act_rows(gpu, dtype, xq, kpad):
    """xq on the device in the kernel dtype, zero-padded to the packed K."""
    A = torch.zeros((xq.shape[0], kpad), dtype=_ops.TDT[dtype], device=gpu)
    A[:, : xq.shape[1]] = xq.to(_ops.TDT[dtype]).to(gpu)
    return A


def _run_lnin(gpu, dtype, variant, flags, M, K, N, kind="plain", eps=1e-5, stats=_stats32,
              stats_out=None):
    xq, g, be, W, bias = _lnin_host(dtype, M, K, N, kind)
    wp, kpad, npad, colsum, cvec = _lnin_weights(gpu, dtype, g, be, W, bias)
    A = _act_rows(gpu, dtype, xq, kpad)
    with _ops.gemm_variant(variant):
        C = _ops.dense(dtype, flags, A, wp, kpad, npad, M, N, bias=cvec, colsum=colsum,
                       stats_in=stats(xq).to(gpu), stats_out=stats_out, ln_width=K, ln_eps=eps)
    return C.double().cpu()


# ---- A. the three flag sets, across kernels ---------------------------------------------------

@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 2, 9, 31]))
@pytest.mark.parametrize("M,K,N", [(197, 96, 384), (300, 384, 1536), (131, 192, 200),
                                   (260, 768, 3072)])
def test_set_289_erf_gelu(gpu, dtype, variant, M, K, N):
    """LNIN|BIAS|GELU_ERF (Swin FC1) against gelu_exact(LN(x) @ W' + c) in fp64. Variant 30 is
    left out: p384_fl (gemm.hip) does not instantiate this flag set, so the 128 x 384 kernel never
    takes it (N = 384, 1536 and 3072 would otherwise qualify)."""
    got = _run_lnin(gpu, dtype, variant, F289, M, K, N)
    torch.testing.assert_close(got, _gelu_erf(_lnin_ref(dtype, M, K, N)), **LNIN_TOL[dtype])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 2, 9, 31]))
@pytest.mark.parametrize("M,K,N", [(196, 384, 192), (147, 768, 384), (300, 1536, 768)])
def test_set_161_merge_reduction_stats(gpu, dtype, variant, M, K, N):
    """LNIN|BIAS|STATS (Swin patch-merge reduction): the input LayerNorm is K wide, the stored row
    N = K / 2, and stats_in / stats_out both have S(K) slots per row. As read from the code: the
    128 x 128 kernel writes slot n0 / 128 of every column tile of the packed width, the 256 x 256
    kernels slots 2 tn and 2 tn + 1 of every tile, i.e. both write slots [0, 2 ceil(N / 256)) (zeros
    for a slab wholly past N) and leave slots [2 ceil(N / 256), S(K)) alone; hence the zero prefill.
    K = 1536 has 12 slots, more than the persistent kernel takes (8). Variant 30 is left out:
    p384_fl does not instantiate this flag set (N = 384 and 768 would otherwise qualify)."""
    st = torch.zeros((M, _nslots(K), 2), device=gpu)
    got = _run_lnin(gpu, dtype, variant, F161, M, K, N, stats_out=st)
    torch.testing.assert_close(got, _lnin_ref(dtype, M, K, N), **LNIN_TOL[dtype])
    stc = st.double().cpu()
    torch.testing.assert_close(stc.sum(1), _stats32(got).double().sum(1), **STATS_TOL)
    assert not stc[:, 2 * ((N + 255) // 256):].any(), "slots past the stored width were written"


@functools.lru_cache(maxsize=None)
def _cls_host(dtype, B, T, D, N):
    xq = _q(_rand((B * T, D), 81, 1.3) + 0.3, dtype)
    g = (1.0 + _rand((D,), 82, 0.1)).float().double()
    be = _rand((D,), 83, 0.1).float().double()
    W = _rand((D, N), 84, 1 / math.sqrt(D)).float().double()
    bias = _rand((N,), 85, 0.05).float().double()
    return xq, g, be, W, bias, _lnin_ref_of(xq[::T], g, be, W, bias, dtype, 1e-5)


@pytest.mark.parametrize("dtype,variant", _dv([0, 1]))
@pytest.mark.parametrize("N", [1000, 37])
@pytest.mark.parametrize("B,T,D", [(1, 197, 192), (5, 50, 384), (130, 17, 768)])
def test_set_49_classifier_on_cls_rows(gpu, dtype, variant, B, T, D, N):
    """LNIN|BIAS|OUT_F32 as the DeiT / T2T classifier calls it: A = the token stream with
    lda = T * D (row b of A is token 0 of image b), stats_step = T. The other tokens hold other
    data and NaN statistics: reading statistics row m instead of m * T poisons row m >= 1."""
    xq, g, be, W, bias, ref = _cls_host(dtype, B, T, D, N)
    wp, kpad, npad, colsum, cvec = _lnin_weights(gpu, dtype, g, be, W, bias)
    assert kpad == D
    st = _stats32(xq)
    st[torch.arange(B * T) % T != 0] = float("nan")
    x = xq.to(_ops.TDT[dtype]).to(gpu)
    with _ops.gemm_variant(variant):
        C = _ops.dense(dtype, F49, x.view(B, T * D)[:, :D], wp, kpad, npad, B, N, bias=cvec,
                       colsum=colsum, stats_in=st.to(gpu), ln_width=D, stats_step=T)
    assert C.dtype == torch.float32
    tol = dict(rtol=1e-3, atol=1e-3) if dtype == "bf16" else dict(rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(C.double().cpu(), ref, **tol)


def _padded(gpu, t64, dtype, pad, fill):
    """t64 on the device in a tensor `pad` columns wider (filled with `fill`); the column slice."""
    full = torch.full((t64.shape[0], t64.shape[1] + pad), fill, dtype=_ops.TDT[dtype], device=gpu)
    full[:, : t64.shape[1]] = t64.to(_ops.TDT[dtype]).to(gpu)
    return full[:, : t64.shape[1]]


@functools.lru_cache(maxsize=None)
def _resln_host(dtype, M, K, D, kind="plain", eps=1e-5):
    """Operands and fp64 reference of the out-proj / FC2 form (BIAS|RESID|RESLN|STATS)."""
    Aq = _q(_rand((M, K), 51), dtype)
    W = _rand((K, D), 52, 1 / math.sqrt(K)).float().double()
    b = _rand((D,), 53, 0.1).float().double()
    xq = _q(_rows(_rand((M, D), 54, 1.1) - 0.2, kind, dtype), dtype)
    g = (1.0 + _rand((D,), 55, 0.1)).float().double()
    be = _rand((D,), 56, 0.1).float().double()
    ref = Aq @ _q(W, dtype) + b + _ln64(xq, g, be, eps)
    return Aq, W, b, xq, g, be, ref


def _run_resln(gpu, dtype, variant, M, K, D, kind="plain", eps=1e-5, stats=_stats32, pitch=None):
    """-> (C [M, ldc] fp64 on the host, stats_out fp64 on the host); pitch = (lda - K, ldr - D,
    ldc - D) pads the rows of A / resid (1e4 in the pad columns) and C (7.0)."""
    Aq, W, b, xq, g, be, _ = _resln_host(dtype, M, K, D, kind, eps)
    wp, kpad, npad = _ops.pack(W.float().to(gpu), dtype)
    assert kpad == K
    bias = torch.zeros(npad, device=gpu)
    bias[:D] = b.float().to(gpu)
    pa, pr, pc = pitch or (0, 0, 0)
    C = torch.full((M, D + pc), 7.0, dtype=_ops.TDT[dtype], device=gpu)
    st = torch.full((M, _nslots(D), 2), float("nan"), device=gpu)
    with _ops.gemm_variant(variant):
        _ops.dense(dtype, F197, _padded(gpu, Aq, dtype, pa, 1e4), wp, kpad, npad, M, D, ldc=D + pc,
                   C=C, bias=bias, resid=_padded(gpu, xq, dtype, pr, 1e4),
                   rstats=stats(xq).to(gpu), rgamma=g.float().to(gpu), rbeta=be.float().to(gpu),
                   stats_out=st, ln_width=D, ln_eps=eps)
    return C.double().cpu(), st.double().cpu()


def _check_resln(dtype, C, st, ref):
    D = ref.shape[1]
    torch.testing.assert_close(C[:, :D], ref, **RESLN_TOL[dtype])
    torch.testing.assert_close(st.sum(1), _stats32(C[:, :D]).double().sum(1), **STATS_TOL)
    assert torch.all(C[:, D:] == 7.0), "columns of C past N were written"


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
@pytest.mark.parametrize("ldc_pad", [8, 4])
def test_padded_pitches_resln(gpu, dtype, variant, ldc_pad):
    """BIAS|RESID|RESLN|STATS with lda = K + 64, ldr = N + 8 and ldc = N + 8 (multiples of 8: the
    persistent kernel still applies) or N + 4 (vec_ok = 1: the 4-column epilogue of the 128 x 128
    kernel); pad columns of A / resid hold 1e4, those of C 7.0 and must stay."""
    M, K, D = 300, 768, 768
    C, st = _run_resln(gpu, dtype, variant, M, K, D, pitch=(64, 8, ldc_pad))
    _check_resln(dtype, C, st, _resln_host(dtype, M, K, D)[-1])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
@pytest.mark.parametrize("ldc_pad", [8, 4])
def test_padded_pitches_lnin(gpu, dtype, variant, ldc_pad):
    """LNIN|BIAS with lda = K + 64 and ldc = N + 8 / N + 4, as test_padded_pitches_resln."""
    M, K, N = 300, 384, 768
    xq, g, be, W, bias = _lnin_host(dtype, M, K, N)
    wp, kpad, npad, colsum, cvec = _lnin_weights(gpu, dtype, g, be, W, bias)
    assert kpad == K
    C = torch.full((M, N + ldc_pad), 7.0, dtype=_ops.TDT[dtype], device=gpu)
    with _ops.gemm_variant(variant):
        _ops.dense(dtype, F33, _padded(gpu, xq, dtype, 64, 1e4), wp, kpad, npad, M, N,
                   ldc=N + ldc_pad, C=C, bias=cvec, colsum=colsum, stats_in=_stats32(xq).to(gpu),
                   ln_width=K)
    C = C.double().cpu()
    torch.testing.assert_close(C[:, :N], _lnin_ref(dtype, M, K, N), **LNIN_TOL[dtype])
    assert torch.all(C[:, N:] == 7.0), "columns of C past N were written"


# ---- B. statistics as the models produce them -------------------------------------------------

@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
@pytest.mark.parametrize("flags,M,K,N", [(F33, 300, 768, 1536), (F35, 300, 384, 1536)])
def test_spread_slots_lnin(gpu, dtype, variant, flags, M, K, N):
    """stats_in spread over one slot per 128-column slab (what a preceding EPI_STATS GEMM leaves),
    not all in slot 0: same tolerances. A kernel summing fewer than all S slots fails."""
    got = _run_lnin(gpu, dtype, variant, flags, M, K, N, stats=_stats_spread)
    ref = _lnin_ref(dtype, M, K, N)
    torch.testing.assert_close(got, _gelu_tanh(ref) if flags == F35 else ref, **LNIN_TOL[dtype])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
def test_spread_slots_resln(gpu, dtype, variant):
    M, K, D = 300, 768, 768
    C, st = _run_resln(gpu, dtype, variant, M, K, D, stats=_stats_spread)
    _check_resln(dtype, C, st, _resln_host(dtype, M, K, D)[-1])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
@pytest.mark.parametrize("M,D", [(300, 768), (197, 192)])
def test_chained_stats(gpu, dtype, variant, M, D):
    """An out-proj form GEMM (set 197) writes the stream and its stats_out; that buffer, unchanged,
    is stats_in of the set-33 GEMM on the stored stream (the model's data flow). The second output
    against fp64 LayerNorm of the stream as stored."""
    Aq, W1, b1, xq, g1, be1, _ = _resln_host(dtype, M, D, D)
    wp1, kpad, npad = _ops.pack(W1.float().to(gpu), dtype)
    bias1 = torch.zeros(npad, device=gpu)
    bias1[:D] = b1.float().to(gpu)
    _, g, be, W, bias = _lnin_host(dtype, M, D, D)
    wp, kpad2, npad2, colsum, cvec = _lnin_weights(gpu, dtype, g, be, W, bias)
    assert kpad == D and kpad2 == D
    st = torch.full((M, _nslots(D), 2), float("nan"), device=gpu)
    with _ops.gemm_variant(variant):
        X = _ops.dense(dtype, F197, Aq.to(_ops.TDT[dtype]).to(gpu), wp1, kpad, npad, M, D,
                       bias=bias1, resid=xq.to(_ops.TDT[dtype]).to(gpu),
                       rstats=_stats32(xq).to(gpu), rgamma=g1.float().to(gpu),
                       rbeta=be1.float().to(gpu), stats_out=st, ln_width=D)
        C = _ops.dense(dtype, F33, X, wp, kpad2, npad2, M, D, bias=cvec, colsum=colsum,
                       stats_in=st, ln_width=D)
    ref = _lnin_ref_of(X.double().cpu(), g, be, W, bias, dtype, 1e-5)
    torch.testing.assert_close(C.double().cpu(), ref, **LNIN_TOL[dtype])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
def test_ln_eps_1e6_lnin(gpu, dtype, variant):
    """ln_eps = 1e-6 (the standard models) on rows whose variance is ~4e-6, where the epsilon
    decides the result (1e-5 instead scales those rows by 0.6)."""
    M, K, N = 300, 384, 768
    got = _run_lnin(gpu, dtype, variant, F33, M, K, N, kind="small", eps=1e-6)
    torch.testing.assert_close(got, _lnin_ref(dtype, M, K, N, "small", 1e-6), **LNIN_TOL[dtype])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
def test_ln_eps_1e6_resln(gpu, dtype, variant):
    M, K, D = 300, 768, 768
    C, st = _run_resln(gpu, dtype, variant, M, K, D, kind="small", eps=1e-6)
    _check_resln(dtype, C, st, _resln_host(dtype, M, K, D, "small", 1e-6)[-1])


def _coef32(xq):
    """The kernels' LayerNorm coefficients (ln_coef / pers_coef, gemm.hip) emulated in fp32 from
    fp64 statistics cast to fp32: mu = s1 / D, r = rsqrt(max(s2 / D - mu^2, 0) + eps)."""
    D = xq.shape[1]
    inv_d = torch.tensor(1.0 / D, dtype=torch.float32)
    s1, s2 = xq.sum(-1).float(), (xq * xq).sum(-1).float()
    mu = s1 * inv_d
    var = torch.clamp(s2 * inv_d - mu * mu, min=0.0)
    r = 1.0 / torch.sqrt(var + torch.tensor(1e-5, dtype=torch.float32))
    return mu.double()[:, None], r.double()[:, None]


def hard_rows_emulation(dtype, M=300, K=768, N=768):
    """Host-only: (max error ratio of the fp32-coefficient form, max error ratio with colsum taken
    from the unrounded weights), both as |out - ref| / (atol + rtol |ref|) over the 8 hard rows."""
    xq, g, be, W, bias = _lnin_host(dtype, M, K, N, "hard")
    ref = _lnin_ref(dtype, M, K, N, "hard")[:8]
    tol = LNIN_TOL[dtype]
    mu, r = _coef32(xq[:8])
    Wp = _packed64(W, g, dtype)
    acc, cvec = xq[:8] @ Wp, be @ W + bias
    folded = r * acc - r * mu * Wp.sum(0) + cvec
    unrounded = r * acc - r * mu * (W * g[:, None]).sum(0) + cvec
    ratio = lambda out: float(((out - ref).abs() / (tol["atol"] + tol["rtol"] * ref.abs())).max())
    return ratio(folded), ratio(unrounded)


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
def test_hard_rows_lnin(gpu, dtype, variant):
    """Rows 0..6: mean 32 (bf16) / 8 (f32) over sigma 0.5 (mean / sigma = 64 and 16, the values first
    tried, kept), where r acc - r mu colsum cancels 64 (16) times the result and is exact only
    because colsum is summed from the packed, rounded weights. hard_rows_emulation (the reference
    pushed through the kernel's fp32 mu / r), worst error over rows 0..7 in units of the tolerance:
    bf16 0.011, f32 0.088 (both under 0.25); with colsum taken from the unrounded weights bf16 is
    at 201 times the tolerance (f32, whose weights are not rounded, at 0.33; the f32 kernel does
    not use colsum, it centres the A rows instead)."""
    M, K, N = 300, 768, 768
    got = _run_lnin(gpu, dtype, variant, F33, M, K, N, kind="hard")
    ref = _lnin_ref(dtype, M, K, N, "hard")
    torch.testing.assert_close(got[:7], ref[:7], **LNIN_TOL[dtype])
    torch.testing.assert_close(got[8:], ref[8:], **LNIN_TOL[dtype])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
def test_constant_row_lnin(gpu, dtype, variant):
    """Row 7 of the same batch: every element 3.0, variance 0 (the fmaxf clamp), LN(x) = beta, so
    the output is cvec = beta . W + bias while r = 1 / sqrt(eps) = 316 multiplies whatever the
    kernel has left of (x - mu) . W'. The folded form r acc - r mu colsum leaves the difference of
    two differently ordered fp32 sums there: in f32 it measured max |out - ref| = 1.99e-3 on this
    row (tolerance 2e-4), which is why the f32 kernel now centres the A rows before the product
    (gemm_nt_kernel) and returns cvec here. bf16 keeps the folded form (tolerance 2.5e-2)."""
    M, K, N = 300, 768, 768
    got = _run_lnin(gpu, dtype, variant, F33, M, K, N, kind="hard")
    torch.testing.assert_close(got[7], _lnin_ref(dtype, M, K, N, "hard")[7], **LNIN_TOL[dtype])


@pytest.mark.parametrize("dtype,variant", _dv([0, 1, 9]))
def test_hard_rows_resln(gpu, dtype, variant):
    """The same rows as the LayerNorm residual of the out-proj / FC2 form ((x - mu) r gamma + beta
    with mu, r from fp32 statistics)."""
    M, K, D = 300, 768, 768
    C, st = _run_resln(gpu, dtype, variant, M, K, D, kind="hard")
    _check_resln(dtype, C, st, _resln_host(dtype, M, K, D, "hard")[-1])


# ---- C. activations point by point ------------------------------------------------------------

# c of |got - x Phi(x)| <= c |x| + output rounding: twice the maximum measured on an MI355X against
# the fp64 reference (test_activation_pointwise docstring), within the caps the issue sets: 4 x
# the bound common.h states (fast fit 8.0e-5; A&S 1.05e-7 + 1e-6 evaluation slack), 1e-5 for the
# fp32 tanh form.
ACT_CAP = {("bf16", "erf"): 4 * 8.0e-5, ("f32", "erf"): 4 * (1.05e-7 + 1e-6), ("f32", "tanh"): 1e-5,
           ("bf16", "tanh"): math.inf}
ACT_C = {("bf16", "erf"): 2 * 2.453e-5, ("f32", "erf"): 2 * 9.336e-8, ("f32", "tanh"): 2 * 3.935e-9,
         ("bf16", "tanh"): 2 * 2.271e-17}
OUT_ROUND = {"bf16": 2.0 ** -8, "f32": 2.0 ** -22}


def _act_grid(dtype):
    pts = [8.0, -8.0, 8.5, -8.5, 20.0, -20.0, 50.0, -50.0, 300.0, -300.0, 0.0, -0.0]
    x = torch.cat([torch.linspace(-10, 10, 4096, dtype=torch.float64),
                   torch.tensor(pts, dtype=torch.float64)])
    x = torch.cat([x, torch.zeros(-len(x) % 64, dtype=torch.float64)])
    return _q(x, dtype).reshape(-1, 64)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("form", ["tanh", "erf"])
def test_activation_pointwise(gpu, dtype, form):
    """The GELU epilogues on their own: K = N = 64, W = I and A a grid of x (4096 points in
    [-10, 10], +-8, +-8.5, +-20, +-50, +-300, +-0; rounded to bf16 first for bf16), so the
    accumulator is x exactly. tanh: flag set 3 (bias 0). erf: flag set 289 with the LayerNorm a
    no-op (statistics (0, 64), eps 0, colsum 0, bias 0: mu = 0, r = rsqrt(1)); f32 runs the A&S
    form, bf16 the fast fit. The same call without the GELU (set 33) must return x bit for bit,
    i.e. r is exactly 1. Bound per element: c |x| + 2^-8 |ref| (bf16 out) / 2^-22 |ref| (f32).
    Measured on an MI355X, max of (|got - ref| - output rounding) / |x|: bf16 fast erf fit
    2.453e-5 (common.h states 8.0e-5 on x Phi(x); the fit's own fp64 error is 4.2e-5 on Phi),
    f32 A&S erf 9.336e-8 (stated 1.05e-7 + evaluation), f32 tanh form 3.935e-9, bf16 tanh form
    2.271e-17 (output rounding is all there is). ACT_C holds twice these."""
    x = _act_grid(dtype)
    M = x.shape[0]
    wp, kpad, npad = _ops.pack(torch.eye(64, device=gpu), dtype)
    A = x.to(_ops.TDT[dtype]).to(gpu)
    zero = torch.zeros(npad, device=gpu)
    if form == "tanh":
        got = _ops.dense(dtype, _lib.EPI_BIAS | _lib.EPI_GELU, A, wp, kpad, npad, M, 64, bias=zero)
        ref = _gelu_tanh(x)
    else:
        st = torch.zeros((M, _nslots(64), 2), device=gpu)
        st[:, 0, 1] = 64.0
        kw = dict(bias=zero, colsum=zero, stats_in=st, ln_width=64, ln_eps=0.0)
        same = _ops.dense(dtype, F33, A, wp, kpad, npad, M, 64, **kw)
        got = _ops.dense(dtype, F289, A, wp, kpad, npad, M, 64, **kw)
        torch.cuda.synchronize()
        assert torch.equal(same.double().cpu(), x), "the no-op LayerNorm must return x (r == 1)"
        ref = _gelu_erf(x)
    torch.cuda.synchronize()
    got = got.double().cpu()
    assert not torch.isnan(got).any()
    ax = x.abs()
    rounding = OUT_ROUND[dtype] * ref.abs()
    err = (got - ref).abs()
    measured = float(((err - rounding).clamp(min=0)[ax > 0] / ax[ax > 0]).max())
    c = ACT_C[(dtype, form)]
    print(f"activation {dtype} {form}: measured c = {measured:.3e} (bound c = {c:.3e}, "
          f"cap {ACT_CAP[(dtype, form)]:.3e}), max |err| = {float(err.max()):.3e}")
    assert c <= ACT_CAP[(dtype, form)]
    neg, pos = x <= -8.0, x >= 8.0
    assert torch.all(got[neg] <= 0) and torch.all(got[neg] >= -1e-6 * ax[neg])
    assert torch.all((got[pos] - x[pos]).abs() <= OUT_ROUND[dtype] * ax[pos])
    assert torch.all(got[ax == 0] == 0)
    bad = err > c * ax + rounding
    assert not bad.any(), f"{int(bad.sum())} points outside the bound, first x = {float(x[bad][0])}"


# ---- D. attention arguments -------------------------------------------------------------------

ATTN_TOL = {"bf16": dict(rtol=2e-2, atol=2e-2), "f32": dict(rtol=1e-4, atol=1e-4)}
ATTN_BH = (2, 3)


@functools.lru_cache(maxsize=None)
def _attn_host(dtype, N, hd):
    B, H = ATTN_BH
    return _q(_rand((B * N, 3 * H * hd), 13, scale=1.5), dtype)


@functools.lru_cache(maxsize=None)
def _attn_ref(dtype, N, hd, scale):
    B, H = ATTN_BH
    q, k, v = _attn_host(dtype, N, hd).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax(torch.einsum("bhid,bhjd->bhij", q, k) * scale, dim=-1)
    return torch.einsum("bhij,bhjd->bhid", p, v).permute(0, 2, 1, 3).reshape(B * N, H * hd)


def _attn_run(gpu, dtype, entry, N, scale, ldq_pad=0, ldo_pad=0):
    """entry: 'attn' (evt_attention), 'hd64' / 'hd32' (evt_attention_hd). -> the whole out tensor
    [B*N, H*hd + ldo_pad] on the host (pad columns of qkv hold 1e4, of out 7.0)."""
    B, H = ATTN_BH
    hd = 32 if entry == "hd32" else 64
    qkv = _padded(gpu, _attn_host(dtype, N, hd), dtype, ldq_pad, 1e4)
    full = torch.full((B * N, H * hd + ldo_pad), 7.0, dtype=_ops.TDT[dtype], device=gpu)
    out = full[:, : H * hd]
    if entry == "attn":
        _ops.attention(dtype, qkv, B, N, H, scale=scale, out=out)
    else:
        _ops.attention_hd(dtype, qkv, B, N, H, hd, scale=scale, out=out)
    torch.cuda.synchronize()
    return full.double().cpu()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("entry", ["attn", "hd64", "hd32"])
@pytest.mark.parametrize("N", [50, 197, 256, 290])
def test_attention_padded_pitches(gpu, dtype, entry, N):
    """ldq = 3 H h_k + 64 and ldo = H h_k + 8 at head sizes 64 (both entry points) and 32, below
    and above the 256-token switch to the streaming kernels."""
    hd = 32 if entry == "hd32" else 64
    full = _attn_run(gpu, dtype, entry, N, hd ** -0.5, ldq_pad=64, ldo_pad=8)
    W = ATTN_BH[1] * hd
    torch.testing.assert_close(full[:, :W], _attn_ref(dtype, N, hd, hd ** -0.5), **ATTN_TOL[dtype])
    assert torch.all(full[:, W:] == 7.0), "columns of out past H * h_k were written"


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("entry", ["attn", "hd32"])
@pytest.mark.parametrize("scale", [0.3, 0.05, 0.0, -0.125])
@pytest.mark.parametrize("N", [50, 197, 256, 290])
def test_attention_scale(gpu, dtype, entry, N, scale):
    """`scale` other than h_k^-0.5. Up to 256 tokens zero and negative scales are allowed
    (include/evt.h): scale 0 gives the mean of V over the N keys (keys past N in the last 16-key
    tile must still weigh 0). Above 256 tokens a non-positive scale is refused with EVT_EINVAL."""
    hd = 32 if entry == "hd32" else 64
    if N > 256 and scale <= 0:
        with pytest.raises(_lib.EvtError) as e:
            _attn_run(gpu, dtype, entry, N, scale)
        assert e.value.code == _lib.EVT_EINVAL
        return
    got = _attn_run(gpu, dtype, entry, N, scale)
    assert not torch.isnan(got).any()
    torch.testing.assert_close(got, _attn_ref(dtype, N, hd, scale), **ATTN_TOL[dtype])
    if scale == 0:
        B, H = ATTN_BH
        v = _attn_host(dtype, N, hd).reshape(B, N, 3, H * hd)[:, :, 2]
        mean = v.mean(1, keepdim=True).expand(B, N, H * hd).reshape(B * N, H * hd)
        torch.testing.assert_close(got, mean, **ATTN_TOL[dtype])
