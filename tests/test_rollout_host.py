"""CPU: the attention-rollout interface (include/evt_rollout.h) without a device.

  * `rollout_reference` on closed forms (uniform maps, one-head permutation maps, `start`, row sums);
  * header = `_lib.ROLLOUT_SIGNATURES` = exported symbols, evt.h includes the header and declares
    none of it itself; the struct and the constants the binding passes are the header's;
  * host-only validation of the C entry points (EVT_EINVAL with a message, nothing launched);
  * the mirrors carry the interface, `rollout_shape` comes from the config alone, Swin and "mx8" raise;
  * the probe module of tests/_rollout_probes.py keeps what its docstring promises: a positive
    bound, the uniform closed form, and the chain re-evaluated in fp32 inside the bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from edgevisiontransformer_amd import _lib
from edgevisiontransformer_amd.modeling.models.head_stats import HeadStats
from edgevisiontransformer_amd.modeling.models.classify import Classification
from edgevisiontransformer_amd.modeling.models.rollout import (AttentionRollout, resolve_mode,
                                                               rollout_reference)
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import (StandardViT, ViT, ViT_Pruned,
                                                           pruned_config)
from tests import _rollout_probes as rp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["evt_attention_rollout_step", "evt_forward_rollout", "evt_rollout_scratch_bytes",
                "evt_rollout_shape"]
PRUNED = "layerwise_h1-d0.5_h3-d1.0_h2-d0.3"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def _bare(cls, cfg, dtype="bf16"):
    m = cls.__new__(cls)
    m.cfg, m.dtype, m._handle = cfg, dtype, None
    return m


# ---- the fp64 reference on closed forms ---------------------------------------------------------
@pytest.mark.parametrize("t,heads,steps", [(5, (1, 1, 1), 3), (17, (3, 2, 1, 4), 4), (64, (2,), 1)])
def test_reference_uniform(t, heads, steps):
    maps = [np.full((2, h, t, t), 1.0 / t) for h in heads]
    got = rollout_reference(maps)
    want = 2.0 ** -steps * np.eye(t) + (1 - 2.0 ** -steps) / t * np.ones((t, t))
    assert got.shape == (2, t, t)
    np.testing.assert_allclose(got, np.broadcast_to(want, got.shape), rtol=1e-14, atol=1e-17)
    np.testing.assert_allclose(rp.uniform_closed_form(t, steps), want, rtol=0, atol=0)


def test_reference_permutation_start_and_row_sums():
    t, rng = 13, np.random.default_rng(13)
    perms = [rng.permutation(t) for _ in range(4)]
    mats = []
    for pi in perms:
        p = np.zeros((t, t))
        p[np.arange(t), pi] = 1.0
        mats.append(p)
    maps = [m[None] for m in mats]                          # one head each: [1, T, T]
    want = np.eye(t)
    for m in mats:
        want = 0.5 * (np.eye(t) + m) @ want
    np.testing.assert_array_equal(rollout_reference(maps), want)   # dyadic values: exact
    # start selects the suffix; a negative start counts from the last block
    for start in range(4):
        suffix = np.eye(t)
        for m in mats[start:]:
            suffix = 0.5 * (np.eye(t) + m) @ suffix
        np.testing.assert_array_equal(rollout_reference(maps, start=start), suffix)
    np.testing.assert_array_equal(rollout_reference(maps, start=-1), 0.5 * (np.eye(t) + mats[-1]))
    # rows sum to 1 and stay non-negative for any row-stochastic maps, ragged heads included
    ragged = []
    for h in (3, 1, 2):
        a = rng.random((2, h, t, t))
        ragged.append(a / a.sum(-1, keepdims=True))
    r = rollout_reference(ragged)
    assert r.shape == (2, t, t) and (r >= 0).all()
    np.testing.assert_allclose(r.sum(-1), 1.0, rtol=1e-14)
    for bad in (dict(maps=[]), dict(maps=maps, start=4), dict(maps=maps, start=-5),
                dict(maps=[np.zeros((3, 4))]), dict(maps=[np.zeros((1, 3, 3)), np.zeros((1, 4, 4))])):
        with pytest.raises(ValueError):
            rollout_reference(**bad)


# ---- header, binding, exports -----------------------------------------------------------------------
def test_header_binding_and_exports_agree(lib):
    txt = open(os.path.join(REPO, "include", "evt_rollout.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.ROLLOUT_SIGNATURES) == ENTRY_POINTS
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.FEATURE_SIGNATURES) |
              set(_lib.IMAGE_SIGNATURES) | set(_lib.PREPROCESS_SIGNATURES) |
              set(_lib.ATTENTION_SIGNATURES) | set(_lib.WINDOW_ATTENTION_SIGNATURES) |
              set(_lib.TAIL_SIGNATURES) | set(_lib.CLASSIFY_SIGNATURES) |
              set(_lib.WORKSPACE_SIGNATURES) | set(_lib.PERFORMER_SIGNATURES) |
              set(_lib.HEAD_STATS_SIGNATURES))
    assert not set(declared) & others
    evt_h = open(os.path.join(REPO, "include", "evt.h")).read()
    assert '#include "evt_rollout.h"' in evt_h
    assert not re.search(r"^int\s+evt_\w*rollout", evt_h, re.M)
    for name in declared:
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.ROLLOUT_SIGNATURES[name][1]
    assert re.search(r"#define EVT_ROLLOUT_CLS 0\b", txt) and _lib.ROLLOUT_CLS == 0
    assert re.search(r"#define EVT_ROLLOUT_ALL 1\b", txt) and _lib.ROLLOUT_ALL == 1
    assert resolve_mode("cls") == 0 and resolve_mode("all") == 1 and resolve_mode(1) == 1
    for bad in ("CLS", 2, True, None):
        with pytest.raises(ValueError):
            resolve_mode(bad)
    # 2 x int32, 2 pointers, size_t
    a = _lib.evt_rollout_args
    assert ctypes.sizeof(a) == 32
    assert (a.start.offset, a.mode.offset, a.out.offset, a.scratch.offset,
            a.scratch_bytes.offset) == (0, 4, 8, 16, 24)
    fields = re.search(r"typedef struct evt_rollout_args \{(.*?)\}", txt, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in a._fields_]
    # the op-level entry point takes evt_attention_probs' arguments up to the scale
    probs = _lib.ATTENTION_SIGNATURES["evt_attention_probs"][1]
    mine = _lib.ROLLOUT_SIGNATURES["evt_attention_rollout_step"][1]
    assert mine[:11] == probs[:11] and mine[-1] == probs[-1]


def test_build_lists_the_header_and_the_sources():
    from edgevisiontransformer_amd import build
    assert any(h.endswith("evt_rollout.h") for h in build.HEADERS)
    assert "rollout.hip" in build.SOURCES
    assert "head_mean_kernel" in open(os.path.join(build.CSRC, "attn_maps.hip")).read()
    assert "rollout_step_kernel" in open(os.path.join(build.CSRC, "rollout.hip")).read()


def test_null_arguments_are_einval_with_a_message(lib):
    a, img = _lib.evt_rollout_args(), _lib.evt_image_args()
    assert lib.evt_forward_rollout(None, ctypes.byref(img), 1, None, ctypes.byref(a),
                                   None) == _lib.EVT_EINVAL
    assert b"non-null" in lib.evt_last_error()
    assert lib.evt_forward_rollout(None, None, 1, None, None, None) == _lib.EVT_EINVAL
    t = ctypes.c_int()
    assert lib.evt_rollout_shape(None, ctypes.byref(t), ctypes.byref(t)) == _lib.EVT_EINVAL
    assert lib.evt_last_error()
    n = ctypes.c_size_t()
    assert lib.evt_rollout_scratch_bytes(None, 1, 0, ctypes.byref(n)) == _lib.EVT_EINVAL
    assert lib.evt_last_error()


def test_rollout_step_validates_before_launch(lib):
    """Every rejected argument set is EVT_EINVAL with a message; the pointers are never followed
    (they are not device memory)."""
    buf = (ctypes.c_float * 256)()
    ok = ctypes.addressof(buf)
    ok += (-ok) % 16  # a 16-byte aligned non-null address
    P = ctypes.c_void_p
    nn = 5 * 5 * 4    # bytes of one [1, 5, 5] buffer

    def call(dtype=1, qkv=ok, ldq=3 * 2 * 64, sb=0, sh=0, ko=0, B=1, N=5, H=2, hd=64, scale=0.125,
             r_in=ok + 128, r_out=ok + 256, scratch=ok + 384, scratch_bytes=nn):
        rc = lib.evt_attention_rollout_step(dtype, P(qkv), ldq, sb, sh, ko, B, N, H, hd, scale,
                                            P(r_in), P(r_out), P(scratch), scratch_bytes, None)
        return rc, lib.evt_last_error()

    bad = {
        "dtype": dict(dtype=2), "NULL qkv": dict(qkv=None), "NULL r_out": dict(r_out=None),
        "NULL scratch": dict(scratch=None), "N 0": dict(N=0),
        "N 4097": dict(N=4097, scratch_bytes=1 << 40), "H 0": dict(H=0),
        "H 255": dict(H=255, ldq=3 * 255 * 64),
        "head size 0": dict(hd=0), "head size 129": dict(hd=129, ldq=3 * 2 * 129),
        "negative batch": dict(B=-1),
        "scale 0": dict(scale=0.0), "scale negative": dict(scale=-0.125),
        "scale inf": dict(scale=float("inf")), "scale nan": dict(scale=float("nan")),
        "r_out misaligned": dict(r_out=ok + 260), "r_in misaligned": dict(r_in=ok + 132),
        "scratch misaligned": dict(scratch=ok + 388), "qkv misaligned": dict(qkv=ok + 4),
        "scratch one float short": dict(scratch_bytes=nn - 4), "scratch 0": dict(scratch_bytes=0),
        "r_in is r_out": dict(r_in=ok + 256), "r_in overlaps r_out": dict(r_in=ok + 256 - 16),
        "r_out overlaps r_in": dict(r_in=ok + 256 + 16),
        "ldq short": dict(ldq=3 * 2 * 64 - 8), "ldq unaligned": dict(ldq=3 * 2 * 64 + 4),
        "slice layout in f32": dict(dtype=0, sb=3 * 2 * 5 * 64, sh=3 * 5 * 64, ldq=64, ko=5 * 64),
        "slice layout, head size 32": dict(hd=32, sb=3 * 2 * 5 * 64, sh=3 * 5 * 64, ldq=64, ko=5 * 64),
        "negative slice stride": dict(sb=-8, sh=3 * 5 * 64, ldq=64, ko=5 * 64),
    }
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == _lib.EVT_EINVAL and b"attention_rollout_step" in msg, what


# ---- the mirrors ----------------------------------------------------------------------------------
def test_mirror_classes_carry_the_interface():
    assert issubclass(AttentionRollout, HeadStats) and issubclass(Classification, AttentionRollout)
    for cls in (ViT, ViT_Pruned, StandardViT, T2T_ViT, SwinTransformer):
        assert issubclass(cls, AttentionRollout)
        for name in ("attention_rollout", "attention_rollout_into", "rollout_shape"):
            assert hasattr(cls, name), (cls.__name__, name)


def test_rollout_shape_is_host_only():
    from edgevisiontransformer_amd.weights import swin_config, t2t_config, vit_config
    v = _bare(StandardViT, vit_config(384, 3, 6, 1536, image_size=224, patch_size=14))
    assert v.rollout_shape() == (257, 3)
    geo = dict(dim=192, depth=3, heads=3, mlp_dim=768, image_size=64, patch_size=16, num_classes=16)
    assert _bare(ViT_Pruned, pruned_config(PRUNED, **geo)).rollout_shape() == (17, 3)
    assert _bare(T2T_ViT, t2t_config(256, 2, 4, 2)).rollout_shape() == (197, 2)
    s = _bare(SwinTransformer, swin_config("tiny", image_size=56, depths=(2, 2), num_heads=(3, 6)))
    m8 = _bare(ViT, vit_config(128, 2, 2, 256, image_size=32, patch_size=16), dtype="mx8")
    img = np.zeros((1, 3, 32, 32), np.float32)
    for model, pat in ((s, "windowed"), (m8, "mx8")):
        with pytest.raises(ValueError, match=pat):
            model.rollout_shape()
        with pytest.raises(ValueError, match=pat):
            model.attention_rollout(img)
        with pytest.raises(ValueError, match=pat):
            model.attention_rollout_into(img, out=None)
    with pytest.raises(ValueError, match="window_attention_maps"):
        s.attention_rollout(img)
    v2 = _bare(ViT, vit_config(128, 2, 2, 256, image_size=32, patch_size=16))
    for kw in (dict(start=2), dict(start=-3), dict(start=1.5), dict(start=True),
               dict(queries="rows"), dict(queries=2)):
        with pytest.raises(ValueError):
            v2.attention_rollout(img, **kw)
    with pytest.raises(ValueError, match="out must be"):
        v2.attention_rollout_into(img, out=None)


# ---- the probes keep their docstring's promises ---------------------------------------------------
@pytest.mark.parametrize("n,hd", [(n, 64) for n in rp.NS] + list(rp.HD_CASES))
def test_probe_cases(n, hd):
    u = rp.case("uniform", n, hd, "bf16")
    for s in range(rp.STEPS):
        want = rp.uniform_closed_form(n, s + 1)
        np.testing.assert_allclose(u["ref"][s], np.broadcast_to(want, u["ref"][s].shape),
                                   rtol=1e-13, atol=1e-16)
    # at y = 0: eps = (2 + 3 nkb) u, every step adds 2 eps + (H + N + 2) u
    nkb = -(-n // 64) if n > 64 else 0
    e = rp.STEPS * (2 * (2 + 3 * nkb) + rp.H + n + 2) * rp.U
    np.testing.assert_allclose(u["bound"][-1], u["ref"][-1] * e / (1 - e) + rp.TINY, rtol=1e-9)
    for kind in rp.INPUTS:
        c = rp.case(kind, n, hd, "bf16")
        assert len(c["rows"]) == rp.STEPS and c["rows"][0].shape == (rp.B * n, 3 * rp.H * hd)
        assert not any(np.array_equal(c["rows"][0], r) for r in c["rows"][1:])   # independent draws
        for s in range(rp.STEPS):
            ref, bound = c["ref"][s], c["bound"][s]
            assert ref.shape == bound.shape == (rp.B, n, n)
            assert np.isfinite(ref).all() and (ref >= 0).all() and (bound > 0).all()
            np.testing.assert_allclose(ref.sum(-1), 1.0, rtol=1e-13)
            assert (bound <= 1e-3 * ref + rp.TINY).all()            # a gate, not a formality
            # the chain re-evaluated in fp32 lies inside the bound
            err = np.abs(rp.fp32_chain(c["maps"][:s + 1]).astype(np.float64) - ref)
            assert (err <= bound).all(), (kind, s, (err / bound).max())


def test_probe_big_cases_are_single_image_single_head():
    for n in rp.BIG:
        c = rp.case("normal", n, 64, "bf16", 1, 1)
        assert c["rows"][0].shape == (n, 3 * 64) and c["ref"][-1].shape == (1, n, n)
        assert (c["bound"][-1] > 0).all()
