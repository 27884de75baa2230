"""CPU: libevt_hip.so loads and exports every entry point include/evt.h declares; host-only
validation paths return the documented error codes without touching a GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "evt.h")


def _declared():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    from edgevisiontransformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def test_header_and_binding_agree():
    from edgevisiontransformer_amd import _lib
    assert _declared() == sorted(_lib.SIGNATURES)
    assert len(_declared()) == 44


def test_every_declared_symbol_is_exported(lib):
    for name in _declared():
        assert hasattr(lib, name), name


def test_host_validation_codes(lib):
    from edgevisiontransformer_amd import _lib
    arr = (ctypes.c_int32 * 12)(*([12] * 12))
    hd = (ctypes.c_int32 * 12)(*([64] * 12))
    ffn = (ctypes.c_int32 * 12)(*([3072] * 12))
    d = _lib.evt_vit_desc(224, 16, 3, 1000, 768, 12, 3072, arr, hd, ffn, 1, 512)
    assert lib.evt_vit_num_weights(ctypes.byref(d)) == 4 + 11 * 12 + 4
    out = ctypes.c_size_t()
    assert lib.evt_query_workspace(ctypes.byref(d), 512, ctypes.byref(out)) == 0
    assert 1.5e9 < out.value < 3e9  # ~1.9 GB of activations for DeiT-base bs512 bf16
    bad = _lib.evt_vit_desc(225, 16, 3, 1000, 768, 12, 3072, arr, hd, ffn, 1, 512)
    assert lib.evt_query_workspace(ctypes.byref(bad), 512, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert b"divisible by the patch size" in lib.evt_last_error()
    hd2 = (ctypes.c_int32 * 12)(*([32] * 12))  # any head size in [1, 128] is accepted
    ok2 = _lib.evt_vit_desc(224, 16, 3, 1000, 768, 12, 3072, arr, hd2, ffn, 1, 512)
    assert lib.evt_query_workspace(ctypes.byref(ok2), 1, ctypes.byref(out)) == 0
    hd3 = (ctypes.c_int32 * 12)(*([160] * 12))
    bad2 = _lib.evt_vit_desc(224, 16, 3, 1000, 768, 12, 3072, arr, hd3, ffn, 1, 512)
    assert lib.evt_query_workspace(ctypes.byref(bad2), 1, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert b"head size" in lib.evt_last_error()
    bad3 = _lib.evt_vit_desc(224, 16, 3, 1000, 100, 12, 3072, arr, hd, ffn, 1, 512)
    assert lib.evt_query_workspace(ctypes.byref(bad3), 1, ctypes.byref(out)) == _lib.EVT_EINVAL
    out_h = ctypes.c_void_p()
    assert lib.evt_vit_create(ctypes.byref(d), None, 0, None, ctypes.byref(out_h)) == _lib.EVT_EINVAL
    assert lib.evt_model_destroy(None) == 0
    assert lib.evt_set_gemm_variant(20) == _lib.EVT_EINVAL  # a former ablation variant
    msg = lib.evt_last_error()
    assert b"0, 1, 2, 6, 8, 9, 16, 30, 31 or 36" in msg and b"lab" not in msg  # the supported set
    for v in (32, 33, 34, 35):  # removed in round 5 (measured-slower lab variants)
        assert lib.evt_set_gemm_variant(v) == _lib.EVT_EINVAL
    # the ablation / timeline / A-B numbers of the former diagnostic build
    for v in (10, 11, 13, 15, 17, 18, 19, 21, 22, 23, 24, 25, 106, 108):
        assert lib.evt_set_gemm_variant(v) == _lib.EVT_EINVAL
    for v in (1, 2, 6, 8, 9, 16, 30, 31, 36, 0):
        assert lib.evt_set_gemm_variant(v) == 0
    assert lib.evt_graph_launch(None, None) == _lib.EVT_EINVAL
    assert lib.evt_graph_capture(None, None, 1, None, None) == _lib.EVT_EINVAL


def test_op_entry_points_validate_before_launch(lib):
    from edgevisiontransformer_amd import _lib
    assert lib.evt_attention(1, None, 0, None, 0, 1, 197, 3, 0.125, None) == _lib.EVT_EINVAL
    assert lib.evt_layernorm(1, None, 0, None, 0, None, None, 1, 7, 1e-5, None) == _lib.EVT_EINVAL
    assert lib.evt_pack_weight(1, None, None, 1, 1, None, 64, 128, None) == _lib.EVT_EINVAL
    assert lib.evt_dense(1, None, None) == _lib.EVT_EINVAL
    # MX8 kernel-level entry points: shape checks before any launch
    assert lib.evt_mx8_layernorm(None, 4, 100, 128, None, None, 1e-5, None, None, None,
                                 None) == _lib.EVT_EINVAL
    assert lib.evt_attention_mx8(None, 2304, None, 768, None, 394, 2, 197, 12, 0.125,
                                 None) == _lib.EVT_EINVAL
    a = _lib.evt_dense_mx8_args()
    a.flags = _lib.EPI_BIAS | _lib.EPI_RESID | _lib.EPI_RESLN  # RESLN without rstats / gamma
    assert lib.evt_dense_mx8(ctypes.byref(a), None) == _lib.EVT_EINVAL


def test_t2t_host_validation(lib):
    from edgevisiontransformer_amd import _lib
    from edgevisiontransformer_amd.weights import t2t_config, t2t_param_shapes
    d = _lib.evt_t2t_desc(224, 3, 1000, 384, 14, 6, 1152, 64, 1, 256)
    n = lib.evt_t2t_num_weights(ctypes.byref(d))
    assert n == len(t2t_param_shapes(t2t_config(384, 14, 6, 3))) == 2 * 13 + 4 + 11 * 14 + 4
    out = ctypes.c_size_t()
    assert lib.evt_t2t_query_workspace(ctypes.byref(d), 256, ctypes.byref(out)) == 0
    assert 0.5e9 < out.value < 3e9
    for bad, msg in ((_lib.evt_t2t_desc(200, 3, 1000, 384, 14, 6, 1152, 64, 1, 8), b"multiple of 16"),
                     (_lib.evt_t2t_desc(224, 3, 1000, 384, 14, 5, 1152, 64, 1, 8), b"num_heads"),
                     (_lib.evt_t2t_desc(224, 3, 1000, 384, 14, 6, 1152, 32, 1, 8), b"token_size")):
        assert lib.evt_t2t_query_workspace(ctypes.byref(bad), 8, ctypes.byref(out)) == _lib.EVT_EINVAL
        assert msg in lib.evt_last_error()
    h = ctypes.c_void_p()
    assert lib.evt_t2t_create(ctypes.byref(d), None, 0, None, ctypes.byref(h)) == _lib.EVT_EINVAL
    assert lib.evt_unfold(1, 1, None, 1, 8, 8, 3, 7, 4, 2, None, 147, None, 0, None) == _lib.EVT_EINVAL
    assert lib.evt_performer(1, None, 192, 1, 16, *([None] * 10), None, 64, None) == _lib.EVT_EINVAL
    # per image: one (kptv, ksum) partial per 196-token chunk + their sum (t2t.hip performer_t)
    assert lib.evt_performer_scratch(2, 3136) == 2 * (16 + 1) * (64 * 32 + 32)
    assert lib.evt_performer_scratch(3, 784) == 3 * (4 + 1) * (64 * 32 + 32)


def test_performer_diagnostics_host_validation(lib):
    """include/evt_performer.h: evt_performer's checks, and the two extras are bf16 only."""
    from edgevisiontransformer_amd import _lib
    nul = [None] * 10   # w .. fc2_b, part
    assert lib.evt_performer_ex(1, None, 192, 1, 16, *nul, None, 64, 0, None, None) == _lib.EVT_EINVAL
    buf = (ctypes.c_float * 64)()
    arr = ctypes.cast(buf, ctypes.c_void_p)
    ok = [arr] * 10
    for ldq, ldo, T in ((188, 64, 16), (192, 60, 16), (194, 64, 16), (192, 66, 16), (192, 64, 0)):
        assert lib.evt_performer_ex(1, arr, ldq, 1, T, *ok, arr, ldo, 0, None, None) == _lib.EVT_EINVAL
        assert lib.evt_performer(1, arr, ldq, 1, T, *ok, arr, ldo, None) == _lib.EVT_EINVAL
    # f32 with either extra; the permuted path with ldq % 8 != 0 or a kqv off 16 bytes
    assert lib.evt_performer_ex(0, arr, 192, 1, 16, *ok, arr, 64, 1, None, None) == _lib.EVT_EINVAL
    assert b"bf16 only" in lib.evt_last_error()
    assert lib.evt_performer_ex(0, arr, 192, 1, 16, *ok, arr, 64, 0, arr, None) == _lib.EVT_EINVAL
    assert lib.evt_performer_ex(1, arr, 196, 1, 16, *ok, arr, 64, 1, None, None) == _lib.EVT_EINVAL
    assert b"ldq % 8" in lib.evt_last_error()
    off = ctypes.c_void_p(arr.value + (8 if arr.value % 16 == 0 else 0))   # 8 mod 16
    assert lib.evt_performer_ex(1, off, 192, 1, 16, *ok, arr, 64, 1, None, None) == _lib.EVT_EINVAL
    assert lib.evt_unfold_stats(None, 1, 4, None, 2, None) == _lib.EVT_EINVAL
    assert lib.evt_unfold_stats(arr, 1, 0, arr, 2, None) == _lib.EVT_EINVAL
    assert lib.evt_unfold_stats(arr, 1, 4, arr, 0, None) == _lib.EVT_EINVAL
    assert lib.evt_unfold_stats(arr, -1, 4, arr, 2, None) == _lib.EVT_EINVAL


def test_swin_host_validation(lib):
    from edgevisiontransformer_amd import _lib
    from edgevisiontransformer_amd.modeling.models.swin import swin_config_from_name
    from edgevisiontransformer_amd.weights import swin_param_shapes
    cfg = swin_config_from_name("swin_tiny_patch4_window7_224")
    d = _lib.evt_swin_desc()
    d.image_size, d.patch_size, d.in_chans, d.num_classes = 224, 4, 3, 1000
    d.embed_dim, d.num_stages, d.window_size, d.mlp_ratio = 96, 4, 7, 4.0
    for i, (dp, h) in enumerate(zip((2, 2, 6, 2), (3, 6, 12, 24))):
        d.depths[i], d.num_heads[i] = dp, h
    d.dtype, d.max_batch = 1, 256
    assert lib.evt_swin_num_weights(ctypes.byref(d)) == len(swin_param_shapes(cfg))
    out = ctypes.c_size_t()
    assert lib.evt_swin_query_workspace(ctypes.byref(d), 256, ctypes.byref(out)) == 0
    assert 1e9 < out.value < 4e9
    d.num_heads[0] = 4  # head size 24
    assert lib.evt_swin_query_workspace(ctypes.byref(d), 256, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert b"head size" in lib.evt_last_error()
    d.num_heads[0], d.image_size = 3, 192  # 48 -> stage resolutions not multiples of 7
    assert lib.evt_swin_query_workspace(ctypes.byref(d), 256, ctypes.byref(out)) == _lib.EVT_EINVAL


def test_mx8_dtype_host_validation(lib):
    """EVT_DTYPE_MX8 (2): accepted for the reference semantics, workspace includes the MX8
    operand buffers (qa, qh, their scales, the LayerNorm row statistics) and, the MX8 encoder
    having no CLS tail, leaves out its hidden rows ([B, ffn_st], bf16); rejected for STANDARD."""
    from edgevisiontransformer_amd import _lib
    arr = (ctypes.c_int32 * 12)(*([12] * 12))
    hd = (ctypes.c_int32 * 12)(*([64] * 12))
    ffn = (ctypes.c_int32 * 12)(*([3072] * 12))
    out_bf, out_8 = ctypes.c_size_t(), ctypes.c_size_t()
    d = _lib.evt_vit_desc(224, 16, 3, 1000, 768, 12, 3072, arr, hd, ffn, 1, 512)
    assert lib.evt_query_workspace(ctypes.byref(d), 512, ctypes.byref(out_bf)) == 0
    d8 = _lib.evt_vit_desc(224, 16, 3, 1000, 768, 12, 3072, arr, hd, ffn, 2, 512)
    assert lib.evt_query_workspace(ctypes.byref(d8), 512, ctypes.byref(out_8)) == 0
    rows = 512 * 197
    extra = rows * (768 + 768 // 32 + 3072 + 3072 // 32 + 8)
    assert out_8.value - out_bf.value == extra - 512 * 3072 * 2
    d8.semantics = _lib.VIT_STANDARD
    assert lib.evt_query_workspace(ctypes.byref(d8), 512, ctypes.byref(out_8)) == _lib.EVT_EINVAL
    assert b"MX8" in lib.evt_last_error()
    d8.semantics, d8.dtype = _lib.VIT_REFERENCE, 3
    assert lib.evt_query_workspace(ctypes.byref(d8), 512, ctypes.byref(out_8)) == _lib.EVT_EINVAL
