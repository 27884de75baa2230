"""GPU parity of Swin-L (stage widths up to 1536): the LayerNorm-consuming GEMMs with 10 / 12
statistics slots on the persistent 256 x 256 kernel (two statistics rounds, gemm.hip PERS_ACC),
the final LayerNorm + pool and the embedding LayerNorm at width 1536, and the swin_large configs.

Models run against the numpy fp64 oracle (oracle/swin_ref.py) on seeded parameters; gates are those
of tests/test_gpu_swin.py / test_gpu_swin_w12.py: f32 logits max-abs <= 1e-3, bf16 max-abs <= 3e-2
and per-row cosine >= 0.9995. Op-level tolerances are those of tests/test_gpu_dense_epilogues.py.

Which GEMM kernel runs: the automatic rule (use_big, gemm.hip) keeps the 128 x 128 kernel for
problems of one tile round, which covers every GEMM of the small models here, so each model and
op case also runs under evt_set_gemm_variant(9), which forces the 256 x 256 kernels (persistent
where the epilogue has one), and the op-level cases add M = 2816, where the automatic rule itself
picks the persistent kernel. No existing hook reports which GEMM kernel a default forward
launched (the per-role profile names roles, not kernels), so "the default run did not fall back"
is NOT asserted here; variant 9 against variant 1 is the check that both paths agree.

The errors each test prints, as measured on an MI355X, are recorded in its docstring.
"""
import functools

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import _lib
from edgevisiontransformer_amd.modeling.models.swin import (SwinTransformer, get_swin,
                                                            swin_config_from_name)
from edgevisiontransformer_amd.weights import make_images, make_swin_params, swin_config
from oracle import swin_ref
from tests import _ops
from tests.test_gpu_dense_epilogues import (F33, F197, F289, LNIN_TOL, _check_resln, _gelu_erf,
                                            _lnin_ref, _resln_host, _run_lnin, _run_resln)
from tests.test_gpu_ops import _nslots
from tests.test_swin_large import two_stage_cfg

pytestmark = pytest.mark.gpu


def _model(cfg, dtype, params, gpu, **kw):
    return SwinTransformer(img_size=cfg.image_size, patch_size=cfg.patch_size,
                           num_classes=cfg.num_classes, embed_dim=cfg.embed_dim,
                           depths=cfg.depths, num_heads=cfg.num_heads,
                           window_size=cfg.window_size, dtype=dtype, weights=params, device=gpu,
                           **kw)


def _cos_rows(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _gate(out, ref, dtype, what):
    err = np.abs(out - ref).max()
    cos = _cos_rows(out, ref).min()
    print(f"{what} {dtype}: max-abs {err:.3e} min row cosine {cos:.6f}")
    if dtype == "f32":
        assert err <= 1e-3, f"{what} f32 max-abs {err:.3e}"
    else:
        assert err <= 3e-2, f"{what} bf16 max-abs {err:.3e}"
        assert cos >= 0.9995, f"{what} bf16 row cosine {cos:.6f}"


# ---- the two-stage model: 768 -> 1536 at R = 14 -> 7, batch 11 (539 rows at stage 1) -----------

@functools.lru_cache(maxsize=None)
def _two_stage(batch):
    cfg = two_stage_cfg()
    params = make_swin_params(cfg, seed=21)
    img = make_images(batch, seed=22, image_size=56)
    return cfg, params, img


@functools.lru_cache(maxsize=None)
def _two_stage_ref():
    cfg, params, img = _two_stage(11)
    return swin_ref.swin_forward(params, cfg, img)


def _two_stage_run(gpu, dtype, variant, batch=11):
    cfg, params, img = _two_stage(batch)
    m = _model(cfg, dtype, params, gpu, max_batch=batch)
    with _ops.gemm_variant(variant):
        out = m(torch.from_numpy(img).to(gpu)).cpu()
    m.close()
    return out


@pytest.mark.parametrize("dtype,variant", [("f32", 0), ("bf16", 0), ("bf16", 9)])
def test_two_stage_1536_against_oracle(gpu, dtype, variant):
    """Merge gather 3072 -> 1536 writing 12 slots, QKV / FC1 reading them, proj / FC2 writing
    them, ln_pool at D = 1536; three 256-row tiles at stage 1, the last partial. Variant 9 forces
    the persistent kernel onto every one of these GEMMs.

    Measured: f32 1.5e-6; bf16 5.3e-3 (row cosine 0.999977) with the automatic kernel choice,
    bf16 6.1e-3 (0.999973) under variant 9."""
    out = _two_stage_run(gpu, dtype, variant).numpy().astype(np.float64)
    _gate(out, _two_stage_ref(), dtype, f"two-stage 1536 variant {variant}")


def test_two_stage_1536_gemm_variants_bf16(gpu):
    """Variants 0 and 36 differ in grid balancing only: bitwise. Variant 1 (the 128 x 128 kernel,
    which took 12 slots before) and variant 9 (persistent kernel forced) agree within the bf16
    gate: the two-round statistics path computes what the unchanged path computes.

    Measured: variant 1 against 0 max-abs 2.7e-3 (row cosine 0.999994), variant 9 against 1
    3.0e-3 (0.999994)."""
    out = {v: _two_stage_run(gpu, "bf16", v) for v in (0, 36, 1, 9)}
    assert torch.equal(out[0], out[36])
    f = lambda v: out[v].numpy().astype(np.float64)  # noqa: E731
    _gate(f(1), f(0), "bf16", "variant 1 against 0")
    _gate(f(9), f(1), "bf16", "variant 9 against 1")


@pytest.mark.parametrize("dtype,variant", [("bf16", 0), ("bf16", 9), ("f32", 0)])
def test_two_stage_1536_batch_independence_and_graph(gpu, dtype, variant):
    """Image i's logits do not depend on its batch neighbours (bitwise) and a HIP-graph replay
    reproduces the eager forward bitwise, at batch 5 (245 rows at stage 1: one partial tile)."""
    cfg, params, img = _two_stage(5)
    x = torch.from_numpy(img).to(gpu)
    m = _model(cfg, dtype, params, gpu, max_batch=5)
    with _ops.gemm_variant(variant):
        full = m(x)
        part = m(x[2:4].contiguous())
        assert torch.equal(full[2:4], part)
        logits = torch.empty_like(full)
        m.capture_graph(x, logits)
        m.replay_graph()
        torch.cuda.synchronize()
        assert torch.equal(logits, full)


# ---- op level: statistics split unevenly over 10 / 12 slots ------------------------------------

# slot edges as fractions of the row: some slots empty, 40 % of the row in slots 8 and up
EDGES = {12: [0, .10, .10, .25, .26, .40, .40, .55, .60, .75, .75, .90, 1.0],
         10: [0, .10, .10, .25, .26, .40, .40, .55, .60, .80, 1.0],
         6: [0, .10, .10, .30, .50, .80, 1.0]}


def _stats_uneven(xq):
    """[rows][S][2]: slot j holds the exact (sum, sumsq) of columns [e_j D, e_j+1 D)."""
    rows, D = xq.shape
    S = _nslots(D)
    e = [int(round(f * D)) for f in EDGES[S]]
    st = torch.zeros((rows, S, 2), dtype=torch.float32)
    for j in range(S):
        part = xq[:, e[j]: e[j + 1]]
        st[:, j, 0], st[:, j, 1] = part.sum(-1).float(), (part * part).sum(-1).float()
    assert not st[:, 1].any() and st[:, S - 1].any()
    return st


@pytest.mark.parametrize("variant", [0, 1, 9])
@pytest.mark.parametrize("flags", [F33, F289])
@pytest.mark.parametrize("M,K,N", [(300, 1536, 384), (300, 1280, 384), (2816, 1536, 1536)])
def test_lnin_wide_rows_uneven_slots(gpu, variant, flags, M, K, N):
    """LNIN (33, 289) in bf16 with ln_width 1536 (12 slots) and 1280 (10) against the fp64
    restatement; a kernel reading 8 slots loses 40 % of every row's sums. M = 300: the issue's
    shape (persistent under variant 9); M = 2816, N = 1536: the automatic rule takes the
    persistent kernel (66 tiles of 256 x 256 against 264 of 128 x 128)."""
    got = _run_lnin(gpu, "bf16", variant, flags, M, K, N, stats=_stats_uneven)
    ref = _lnin_ref("bf16", M, K, N)
    torch.testing.assert_close(got, _gelu_erf(ref) if flags == F289 else ref, **LNIN_TOL["bf16"])


@pytest.mark.parametrize("variant", [0, 1, 9])
@pytest.mark.parametrize("M,K,D", [(300, 1536, 1536), (300, 1280, 1280), (2816, 1536, 1536)])
def test_resln_wide_rows_uneven_slots(gpu, variant, M, K, D):
    """RESLN (197) with the residual rows 1536 / 1280 wide, EVT_EPI_STATS out (12 / 10 slots)."""
    C, st = _run_resln(gpu, "bf16", variant, M, K, D, stats=_stats_uneven)
    _check_resln("bf16", C, st, _resln_host("bf16", M, K, D)[-1])


@pytest.mark.parametrize("flags", [F33, F289, F197])
@pytest.mark.parametrize("M", [300, 2816])
def test_six_slots_bitwise_with_variant_36(gpu, flags, M):
    """ln_width 768 (6 slots, the one-round path): variant 36 gives the bits of variant 0."""
    K = 768
    if flags == F197:
        a, b = (_run_resln(gpu, "bf16", v, M, K, K, stats=_stats_uneven)[0] for v in (0, 36))
    else:
        a, b = (_run_lnin(gpu, "bf16", v, flags, M, K, 1536 if M > 300 else 384,
                          stats=_stats_uneven) for v in (0, 36))
    assert torch.equal(a, b)


def test_twelve_slots_bitwise_with_variant_36(gpu):
    """12 slots at a shape where the automatic rule takes the persistent kernel: variant 36 (no
    grid balancing, another tile -> block assignment) gives the bits of variant 0."""
    a, b = (_run_lnin(gpu, "bf16", v, F33, 2816, 1536, 1536, stats=_stats_uneven) for v in (0, 36))
    assert torch.equal(a, b)


# ---- ln_rows / ln_pool_long above 1024 columns --------------------------------------------------

def test_single_stage_1536_window12_f32(gpu):
    """embed_dim 1536, one block, window 12 at 96 px (576 tokens: ln_pool_long), batch 2, f32: the
    embedding LayerNorm (ln_rows) and the pooled final LayerNorm at width 1536. Gate 2e-5 as the
    window-12 single-stage test. Measured: 4.7e-7."""
    cfg = swin_config("large", embed_dim=1536, depths=(1,), num_heads=(48,), window_size=12,
                      image_size=96, num_classes=11)
    params = make_swin_params(cfg, seed=31)
    img = make_images(2, seed=32, image_size=96)
    ref = swin_ref.swin_forward(params, cfg, img)
    out = _model(cfg, "f32", params, gpu)(torch.from_numpy(img).to(gpu)).cpu().numpy()
    err = np.abs(out.astype(np.float64) - ref).max()
    print(f"single stage 1536 / window 12 f32: max-abs {err:.3e}")
    assert err <= 2e-5


def test_single_stage_1536_window12_bf16(gpu):
    """The same model in bf16 (ln_rows / ln_pool_long<bf16> at 1536 columns) on the model gate.
    Measured: 1.4e-3, row cosine 0.999992."""
    cfg = swin_config("large", embed_dim=1536, depths=(1,), num_heads=(48,), window_size=12,
                      image_size=96, num_classes=11)
    params = make_swin_params(cfg, seed=31)
    img = make_images(2, seed=32, image_size=96)
    ref = swin_ref.swin_forward(params, cfg, img)
    out = _model(cfg, "bf16", params, gpu)(torch.from_numpy(img).to(gpu)).cpu().numpy()
    _gate(out.astype(np.float64), ref, "bf16", "single stage 1536 / window 12")


def test_stage_wider_than_1536_is_refused(gpu):
    cfg = swin_config("large", embed_dim=1568, depths=(1,), num_heads=(49,), image_size=28)
    with pytest.raises(_lib.EvtError, match="stage width must be <= 1536") as e:
        _model(cfg, "bf16", make_swin_params(cfg, seed=1), gpu, max_batch=1)
    assert e.value.code == _lib.EVT_EINVAL


def test_swin_large_max_batch_limits(gpu):
    """The 2^31-byte rule at Swin-L widths (include/evt.h): 384 px takes 151 bf16 / 75 f32 images,
    224 px 445 / 222; one more is EVT_EINVAL. Checked through the workspace query (no allocation)."""
    for name, dtype, ok in (("swin_large_patch4_window12_384", "bf16", 151),
                            ("swin_large_patch4_window12_384", "f32", 75),
                            ("swin_large_patch4_window7_224", "bf16", 445),
                            ("swin_large_patch4_window7_224", "f32", 222)):
        c = swin_config_from_name(name)
        m = SwinTransformer.__new__(SwinTransformer)
        m.cfg, m.dtype = c, dtype
        assert m.workspace_bytes(ok) > 0
        with pytest.raises(_lib.EvtError) as e:
            m.workspace_bytes(ok + 1)
        assert e.value.code == _lib.EVT_EINVAL


# ---- all four Swin-L widths, depth-trimmed ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trimmed(image_size, window, batch):
    cfg = swin_config("large", depths=(1, 1, 2, 1), num_classes=17, image_size=image_size,
                      window_size=window)
    params = make_swin_params(cfg, seed=51)
    img = make_images(batch, seed=52, image_size=image_size)
    return cfg, params, img, swin_ref.swin_forward(params, cfg, img)


@pytest.mark.parametrize("dtype,variant", [("f32", 0), ("bf16", 0), ("bf16", 9)])
@pytest.mark.parametrize("image_size,window,batch", [(224, 7, 2), (384, 12, 1)])
def test_swin_large_trimmed_against_oracle(gpu, dtype, variant, image_size, window, batch):
    """Widths 192 / 384 / 768 / 1536 with depths (1, 1, 2, 1): stage 3 is one unshifted window of
    7 (224 px) or 12 (384 px) with 48 heads.

    Measured: 224 px f32 1.8e-6, bf16 6.3e-3 (cosine 0.999992), bf16 variant 9 6.3e-3
    (0.999993); 384 px f32 7.9e-7, bf16 5.1e-3 (0.999995), bf16 variant 9 4.4e-3 (0.999996)."""
    cfg, params, img, ref = _trimmed(image_size, window, batch)
    assert [cfg.window(i) for i in range(4)] == [window] * 4
    m = _model(cfg, dtype, params, gpu, max_batch=batch)
    with _ops.gemm_variant(variant):
        out = m(torch.from_numpy(img).to(gpu)).cpu().numpy().astype(np.float64)
    m.close()
    _gate(out, ref, dtype, f"swin_large trimmed {image_size} px variant {variant}")


def test_swin_large_patch4_window7_224_bf16_against_f32(gpu):
    """The published shape on two images, bf16 against f32 on the bf16 gate (no oracle run at full
    depth). Measured: max-abs 2.0e-2, row cosine 0.999981."""
    name = "swin_large_patch4_window7_224"
    params = make_swin_params(swin_config_from_name(name), seed=7)
    x = torch.from_numpy(make_images(2, seed=8, image_size=224)).to(gpu)
    out = {}
    for dtype in ("f32", "bf16"):
        m = get_swin(name, dtype=dtype, weights=params, device=gpu, max_batch=2)
        assert m.num_features == 1536 and [m.cfg.window(i) for i in range(4)] == [7] * 4
        out[dtype] = m(x).cpu().numpy().astype(np.float64)
        m.close()
    assert np.isfinite(out["f32"]).all()
    _gate(out["bf16"], out["f32"], "bf16", name)
