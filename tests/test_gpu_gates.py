"""GPU: structured gates (include/evt_gates.h; csrc/gates.hip, model.cpp set_gates,
modeling/models/gates.py).

Op level: evt_gate_weights is bitwise `(w0.float() * g).to(dtype)`, the sign of zero included, inside
sentinel-guarded buffers, and leaves w0 alone.

Model level, on the small ViT / ViT_Pruned / StandardViT of tests/test_gpu_head_stats.py at batch 2:
a gated model is bitwise a fresh model created from `gates_reference` parameters, for every output
the library has; its logits are held to the fp64 oracle run on those parameters under the
project's gates (F32_TOL, BF16_ABS, BF16_COS of tests/test_gpu_model.py; the oracle has no pooled
output for the reference ViT, so pooled is held bitwise to the fresh model only); all-ones gates
and clear_gates() restore the untouched model bitwise; the invariances (lanes, token-major QKV,
uint8 input, batch position, a second call, a graph captured before the set), the composition with
token pruning and the analysis outputs, no compounding, the refusals and head_ablation.

A lane child is refused by the library (EVT_EINVAL, "lane of another model"), but no public call
hands a child handle out, so that refusal is not reachable from a test.
"""
import ctypes

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib, evaluate
from edgevisiontransformer_amd.evaluate import head_ablation
from edgevisiontransformer_amd.modeling.models.gates import gates_reference
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT, ViT_Pruned
from edgevisiontransformer_amd.pruning import (build_pruned_vit, gates_from_kept,
                                               importance_from_head_ablation, prune_vit_params)
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_swin_params,
                                               make_vit_params, swin_config)
from oracle import vit_ref
from tests._ops import TDT, _p, _s
from tests.test_gpu_features import _cos_rows
from tests.test_gpu_head_stats import PRUNED, _pruned, _std, _t2t, _vit
from tests.test_gpu_model import BF16_ABS, BF16_COS, F32_TOL
from tests.test_gpu_token_pruning import _guarded, _intact

pytestmark = pytest.mark.gpu
GATE_VALUES = np.array([0.0, 1.0, 0.5, -1.0, 1e-3, 3.0], dtype=np.float32)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- op level -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(128, 64), (128, 192), (256, 3072)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gate_weights_op(gpu, shape, dtype):
    npad, kpad = shape
    rng = np.random.default_rng(npad + kpad)
    w_host = torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * 0.05).to(TDT[dtype])
    g_host = rng.choice(GATE_VALUES, kpad).astype(np.float32)
    g_host[:6] = GATE_VALUES  # every value occurs
    g_host[7] = 0.0
    w_host[:, 7] = -w_host[:, 7].abs() - 0.01  # negative weights under gate 0: -0.0
    w_host[:, 0] = -w_host[:, 0].abs() - 0.01
    f0, w0 = _guarded(shape, TDT[dtype], gpu, w_host)
    fg, g = _guarded((kpad,), torch.float32, gpu, torch.from_numpy(g_host))
    fw, w = _guarded(shape, TDT[dtype], gpu)
    _lib.check(_lib.load_library().evt_gate_weights(_lib.DTYPE[dtype], _p(w0), _p(w), _p(g), npad,
                                                    kpad, _s()))
    torch.cuda.synchronize()
    assert _intact(fw) and _intact(f0) and _intact(fg), "guard elements overwritten or output not filled"
    want = (w0.float() * g).to(TDT[dtype])
    assert torch.equal(_bits(w), _bits(want))
    assert bool((_bits(w[:, 7]) == _bits(torch.tensor(-0.0, dtype=TDT[dtype], device=gpu))).all())
    assert bool((_bits(w[:, 0]) == _bits(torch.tensor(-0.0, dtype=TDT[dtype], device=gpu))).all())
    assert torch.equal(_bits(w0), _bits(w_host.to(gpu))) and torch.equal(g, torch.from_numpy(g_host).to(gpu))
    # all-ones gates copy the pristine bits; a second launch writes the same
    g.fill_(1.0)
    _lib.check(_lib.load_library().evt_gate_weights(_lib.DTYPE[dtype], _p(w0), _p(w), _p(g), npad,
                                                    kpad, _s()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(w), _bits(w0)) and _intact(fw)


# ---- model level ----------------------------------------------------------------------------------
# name -> (factory, class, constructor keywords, parameter generator, seed, image size, oracle)
_STD_ORACLE = lambda p, c, x: vit_ref.std_vit_forward(p, c, x, eps=1e-6)  # noqa: E731
SPEC = {
    "vit": (_vit, ViT, dict(dim=192, depth=3, heads=3, mlp_dim=768, image_size=32, patch_size=4,
                            num_classes=16), make_vit_params, 71, 32, vit_ref.vit_forward),
    "pruned": (_pruned, ViT_Pruned, dict(prune_encoding=PRUNED, dim=192, depth=3, heads=3,
                                         mlp_dim=768, image_size=64, patch_size=16, num_classes=16),
               make_vit_params, 72, 64, vit_ref.vit_forward),
    "std": (_std, StandardViT, dict(dim=192, depth=2, heads=3, image_size=64, patch_size=8,
                                    num_classes=16), make_std_vit_params, 73, 64, _STD_ORACLE),
}


def _image(name, gpu, batch=2):
    return torch.from_numpy(make_images(batch, seed=75, image_size=SPEC[name][5])).to(gpu)


def _fresh(name, dtype, gpu, params, lanes=1, **kw):
    return SPEC[name][1](**SPEC[name][2], dtype=dtype, weights=params, device=gpu, max_batch=2,
                         lanes=lanes, **kw)


def _mixed(n, seed):
    g = np.random.default_rng(seed).choice(GATE_VALUES, n).astype(np.float32)
    g[:min(n, 6)] = GATE_VALUES[:min(n, 6)]
    return g


def _gate_sets(m):
    """Two gate sets on a middle block and on the last block (the CLS tail path): a binary head
    mask alone; fractional / negative head gates with mixed FFN gates."""
    depth, heads, ffn = m.cfg.depth, list(m.cfg.heads), list(m.cfg.ffn)
    mid, last = depth - 2, depth - 1
    binary = {b: np.array([float(h % 2) for h in range(heads[b])], dtype=np.float32)
              for b in (mid, last)}
    if heads[mid] == 1:
        binary[mid] = np.zeros(1, dtype=np.float32)
    frac = {mid: np.array([0.5, 1.0, -1.25][:heads[mid]], dtype=np.float32),
            -1: np.array([3.0, 1e-3, 0.25][:heads[last]], dtype=np.float32)}
    return [(binary, None), (frac, {mid: _mixed(ffn[mid], 1), -1: _mixed(ffn[last], 2)})]


def _all_outputs(m, x):
    """Every output the library has for a ViT, as a flat list of tensors."""
    nb = m.num_blocks
    f = m.features(x, tokens=True, taps=range(nb), logits=True)
    out = [m(x).clone(), f["pooled"], f["tokens"], f["logits"], *f["taps"]]
    out += m.attention_maps(x, blocks=range(nb), queries="all")["maps"]
    out += m.head_stats(x)["stats"] + m.ffn_stats(x)["stats"]
    out.append(m.attention_rollout(x, queries="all")["rollout"])
    out.append(m.classify(x, topk=3)["indices"])
    torch.cuda.synchronize()
    return out


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _oracle_gate(what, dtype, got, ref):
    got = got.double().cpu().numpy()
    err, cos = np.abs(got - ref).max(), _cos_rows(got, ref).min()
    print(f"GATES-ORACLE {what} {dtype}: max-abs {err:.3e} min cos {cos:.6f}")
    if dtype == "f32":
        assert err <= F32_TOL, f"{what}: f32 max-abs {err:.3e}"
    else:
        assert err <= BF16_ABS and cos >= BF16_COS, f"{what}: bf16 max-abs {err:.3e}, min cos {cos:.6f}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SPEC))
def test_identity_and_clear_restore_bitwise(gpu, name, dtype):
    m = SPEC[name][0](dtype, 1, gpu)
    x = _image(name, gpu)
    base = [m(x).clone(), m.forward_features(x).clone()]
    run = lambda: [m(x), m.forward_features(x)]  # noqa: E731
    ones_h = {b: np.ones(h, dtype=np.float32) for b, h in enumerate(m.cfg.heads)}
    ones_f = {b: np.ones(f, dtype=np.float32) for b, f in enumerate(m.cfg.ffn)}
    ws = m.allocated_workspace_bytes()
    m.set_head_gates(ones_h)
    m.set_ffn_gates(ones_f)
    assert _equal(run(), base)
    heads, ffn = _gate_sets(m)[1]
    m.set_head_gates(heads)
    m.set_ffn_gates(ffn)
    assert not torch.equal(m(x), base[0])
    m.set_head_gates(ones_h)  # all ones through the kernel, from the pristine copies
    m.set_ffn_gates(ones_f)
    assert _equal(run(), base)
    m.set_head_gates(heads)
    m.set_ffn_gates(ffn)
    m.clear_gates()
    assert _equal(run(), base) and m.allocated_workspace_bytes() == ws
    assert all((g == 1).all() for g in m.head_gates() + m.ffn_gates())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SPEC))
def test_gated_model_is_the_fresh_model_of_gated_parameters(gpu, name, dtype):
    make, _, _, gen, seed, _, oracle = SPEC[name]
    m = make(dtype, 1, gpu)
    x = _image(name, gpu)
    params = gen(m.cfg, seed=seed)
    plain = _fresh(name, dtype, gpu, params)
    assert torch.equal(plain(x), m(x))  # the factory's model is the one these parameters give
    del plain
    for k, (heads, ffn) in enumerate(_gate_sets(m)):
        m.clear_gates()
        m.set_head_gates(heads)
        m.set_ffn_gates(ffn)
        got = _all_outputs(m, x)
        fresh = _fresh(name, dtype, gpu, gates_reference(params, m.cfg, heads, ffn, dtype=dtype))
        want = _all_outputs(fresh, x)
        bad = [i for i, (u, v) in enumerate(zip(got, want)) if not torch.equal(u, v)]
        assert not bad and len(got) == len(want), f"gate set {k}: outputs {bad} differ"
        ref = oracle(gates_reference(params, m.cfg, heads, ffn), m.cfg, x.cpu().numpy())
        _oracle_gate(f"{name} set {k}", dtype, got[0], ref)
        del fresh


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_binary_mask_against_build_pruned_vit(gpu, dtype):
    """Not bitwise: the pruned model's K extent differs, so its sums run in another order. Both are
    held to the one oracle, and in f32 to each other within F32_TOL."""
    m = _vit(dtype, 1, gpu)
    x = _image("vit", gpu)
    cfg, params = m.cfg, make_vit_params(m.cfg, seed=71)
    rng = np.random.default_rng(9)
    kept_heads = [[0, 2], [1], [0, 1]]
    kept_ffn = [sorted(int(i) for i in rng.choice(768, k, replace=False)) for k in (500, 64, 333)]
    hg, fg = gates_from_kept(kept_heads, 3), gates_from_kept(kept_ffn, list(cfg.ffn))
    m.set_head_gates(hg)
    m.set_ffn_gates(fg)
    pruned = build_pruned_vit(params, cfg, kept_heads, kept_ffn, dtype=dtype, device=gpu,
                              max_batch=2, lanes=1)
    a, b = m(x), pruned(x)
    ref = vit_ref.vit_forward(gates_reference(params, cfg, hg, fg), cfg, x.cpu().numpy())
    pp, pc = prune_vit_params(params, cfg, kept_heads, kept_ffn)
    assert np.abs(vit_ref.vit_forward(pp, pc, x.cpu().numpy()) - ref).max() < 1e-9  # one oracle
    _oracle_gate("masked", dtype, a, ref)
    _oracle_gate("pruned", dtype, b, ref)
    if dtype == "f32":
        err = float((a - b).abs().max())
        print(f"GATES-PRUNED f32: masked against pruned max-abs {err:.3e}")
        assert err <= F32_TOL


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bitwise_invariances(gpu, dtype, monkeypatch):
    m = _vit(dtype, 1, gpu)
    x = _image("vit", gpu)
    base = m(x).clone()
    heads, ffn = _gate_sets(m)[1]

    def gate(model):
        model.set_head_gates(heads)
        model.set_ffn_gates(ffn)
        return model

    want = gate(m)(x).clone()
    assert not torch.equal(want, base)
    assert torch.equal(m(x), want)  # a second call
    assert torch.equal(m(x[:1].contiguous())[0], want[0])  # one image alone
    m2 = gate(_vit(dtype, 2, gpu))  # two lanes: the children read the parent's gated weights
    assert m2.lanes() == 2 and torch.equal(m2(x), want)
    m2.clear_gates()
    assert torch.equal(m2(x), base)
    monkeypatch.setenv("EVT_QKV_LAYOUT", "token")
    mt = gate(_vit(dtype, 1, gpu))
    monkeypatch.delenv("EVT_QKV_LAYOUT")
    assert torch.equal(mt(x), want) and mt.qkv_headmajor_layers() == 0
    # uint8 input
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    assert torch.equal(m(u8), m(u8.to_float("nchw")))
    # a handle rebuilt for a larger batch keeps its gates
    small = gate(SPEC["vit"][1](**SPEC["vit"][2], dtype=dtype, seed=71, device=gpu, max_batch=1, lanes=1))
    assert torch.equal(small(x), want)
    # a graph captured before the set, replayed after it with no recapture
    mg = _vit(dtype, 1, gpu)
    xin, logits = x.clone(), torch.empty_like(base)
    mg.capture_graph(xin, logits)
    mg.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, base)
    gate(mg)
    mg.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, want)
    mg.clear_gates()
    mg.replay_graph()
    torch.cuda.synchronize()
    assert torch.equal(logits, base)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_composition_with_token_pruning_and_analysis_outputs(gpu, dtype):
    m = _vit(dtype, 1, gpu)
    x = _image("vit", gpu)
    params = make_vit_params(m.cfg, seed=71)
    maps0 = m.attention_maps(x, blocks=range(3), queries="all")["maps"]
    hs0, fs0 = m.head_stats(x)["stats"], m.ffn_stats(x)["stats"]
    ro0 = m.attention_rollout(x, start=1)["rollout"]
    heads = {1: np.array([0.0, 1.0, 0.5], dtype=np.float32)}
    m.set_head_gates(heads)
    maps1 = m.attention_maps(x, blocks=range(3), queries="all")["maps"]
    hs1, fs1 = m.head_stats(x)["stats"], m.ffn_stats(x)["stats"]
    # block 1's own head gates: its probabilities are what it computed; block 2 sees the gated stream
    assert torch.equal(maps1[0], maps0[0]) and torch.equal(maps1[1], maps0[1])
    assert not torch.equal(maps1[2], maps0[2])
    assert torch.equal(hs1[1], hs0[1]) and not torch.equal(hs1[2], hs0[2])
    assert not torch.equal(fs1[1], fs0[1])  # the FFN of block 1 already reads the gated attention
    assert not torch.equal(m.attention_rollout(x, start=1)["rollout"], ro0)  # block 2's term moved
    m.clear_gates()
    m.set_head_gates({2: heads[1]})  # the last block's gates: no map, statistic or rollout moves
    assert _equal(m.attention_maps(x, blocks=range(3), queries="all")["maps"], maps0)
    assert _equal(m.head_stats(x)["stats"], hs0)
    assert torch.equal(m.attention_rollout(x, start=1)["rollout"], ro0)
    m.clear_gates()
    ffn = {1: _mixed(768, 3)}
    m.set_ffn_gates(ffn)
    fs2 = m.ffn_stats(x)["stats"]
    assert torch.equal(fs2[0], fs0[0]) and torch.equal(fs2[1], fs0[1])  # what FC1 stored
    assert not torch.equal(fs2[2], fs0[2])
    # with a token schedule: the fresh gated model with the same schedule
    schedule = {0: 40, 1: 17}
    m.set_head_gates(heads)
    m.set_token_pruning(schedule)
    got = m.token_pruning_outputs(x, logits=True, pooled=True)
    fresh = _fresh("vit", dtype, gpu, gates_reference(params, m.cfg, heads, ffn, dtype=dtype),
                   token_keep=schedule)
    want = fresh.token_pruning_outputs(x, logits=True, pooled=True)
    torch.cuda.synchronize()
    assert torch.equal(got["logits"], want["logits"]) and torch.equal(got["pooled"], want["pooled"])
    assert _equal(got["scores"], want["scores"]) and _equal(got["kept"], want["kept"])
    assert torch.equal(m(x), want["logits"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_successive_sets_do_not_compound(gpu, dtype):
    m = _vit(dtype, 1, gpu)
    x = _image("vit", gpu)
    first, second = _gate_sets(m)[1], ({1: np.array([0.3, 0.7, 1.1], dtype=np.float32)},
                                       {1: _mixed(768, 5) * np.float32(0.37)})
    m.set_head_gates(first[0])
    m.set_ffn_gates(first[1])
    m.set_head_gates({1: np.full(3, 1.0 / 3.0, dtype=np.float32)})
    m.set_head_gates(second[0])
    m.set_ffn_gates(second[1])
    m.set_head_gates({-1: np.ones(3)})
    m.set_ffn_gates({-1: np.ones(768)})
    twice = m(x).clone()
    alone = _vit(dtype, 1, gpu)
    alone.set_head_gates(second[0])
    alone.set_ffn_gates(second[1])
    assert torch.equal(alone(x), twice)
    # the library's record is the last set
    n = ctypes.c_int()
    rec = (ctypes.c_float * 768)()
    lib = _lib.load_library()
    _lib.check(lib.evt_model_get_head_gates(m._ptr(), 1, rec, 768, ctypes.byref(n)))
    assert n.value == 3 and np.array_equal(np.array(rec[:3], dtype=np.float32), second[0][1])
    _lib.check(lib.evt_model_get_ffn_gates(m._ptr(), -2, rec, 768, ctypes.byref(n)))
    assert n.value == 768 and np.array_equal(np.array(rec[:768], dtype=np.float32), second[1][1])
    _lib.check(lib.evt_model_get_head_gates(m._ptr(), 0, rec, 2, ctypes.byref(n)))
    assert n.value == 3 and list(rec[:2]) == [1.0, 1.0]
    assert np.array_equal(m.head_gates()[1], second[0][1])


def test_refusals(gpu):
    lib = _lib.load_library()
    E = _lib.EVT_EINVAL
    g3 = (ctypes.c_float * 3)(1, 0, 1)
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    sw = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                         embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                         window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                         device=gpu, max_batch=1, lanes=1)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    t2t = _t2t("bf16", 1, gpu)
    n = ctypes.c_int()
    for model, py_msg, c_msg in ((t2t, "no structured gates", "T2T-ViT"),
                                 (sw, "no structured gates", "Swin"), (m8, "mx8", "MX8")):
        with pytest.raises(ValueError, match=py_msg):
            model.mask_heads({0: [0]})
        with pytest.raises(ValueError, match=py_msg):
            model.set_ffn_gates({0: np.ones(4)})
        for rc in (lib.evt_model_set_head_gates(model._ptr(), 0, g3, 3, None),
                   lib.evt_model_set_ffn_gates(model._ptr(), 0, g3, 3, None),
                   lib.evt_model_clear_gates(model._ptr(), None),
                   lib.evt_model_get_head_gates(model._ptr(), 0, None, 0, ctypes.byref(n))):
            assert rc == E and c_msg in _lib.last_error()
    m = _vit("bf16", 1, gpu)
    x = _image("vit", gpu)
    base = m(x).clone()
    assert lib.evt_model_set_head_gates(m._ptr(), 0, g3, 2, None) == E
    assert "n is 2" in _lib.last_error() and "3 heads" in _lib.last_error()
    assert lib.evt_model_set_ffn_gates(m._ptr(), 0, g3, 3, None) == E
    assert "768 FFN neurons" in _lib.last_error()
    assert lib.evt_model_set_head_gates(m._ptr(), 3, g3, 3, None) == E and "block 3" in _lib.last_error()
    assert lib.evt_model_set_head_gates(m._ptr(), -4, g3, 3, None) == E
    assert lib.evt_model_set_head_gates(m._ptr(), 0, None, 3, None) == E
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.evt_model_set_head_gates(m._ptr(), 0, (ctypes.c_float * 3)(1, bad, 1), 3, None) == E
        assert "not finite" in _lib.last_error()
    with pytest.raises(ValueError, match="has 3 heads"):
        m.set_head_gates({0: [1, 1]})
    with pytest.raises(ValueError, match="finite"):
        m.set_head_gates({0: [1, float("nan"), 1]})
    with pytest.raises(ValueError, match="outside"):
        m.mask_heads({3: [0]})
    # while the stream is capturing: refused, by name, before anything is allocated or enqueued
    m.set_head_gates({0: [1.0, 0.5, 1.0]})
    gated = m(x).clone()
    buf = torch.zeros(8, device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.add_(1.0)
        with pytest.raises(ValueError, match="capturing"):
            m.set_head_gates({1: [0.0, 1.0, 1.0]})
        with pytest.raises(ValueError, match="capturing"):
            m.set_ffn_gates({1: np.zeros(768)})
        rc = lib.evt_model_clear_gates(m._ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == E and "capturing" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(m(x), gated)  # every refusal above left the model as it was
    assert [g.tolist() for g in m.head_gates()] == [[1.0, 0.5, 1.0], [1.0] * 3, [1.0] * 3]
    m.clear_gates()
    assert torch.equal(m(x), base)


def test_head_ablation_is_four_manual_runs(gpu):
    m = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=8, num_classes=8,
            dtype="bf16", seed=81, device=gpu, max_batch=4, lanes=1)
    rng = np.random.default_rng(4)
    loader = [(torch.from_numpy(make_images(4, seed=90 + i, image_size=32)).to(gpu),
               rng.integers(0, 8, 4)) for i in range(2)]
    m.set_head_gates({0: [1.0, 0.5]})  # the sweep runs on top of the gates the model has
    before = [g.copy() for g in m.head_gates()]
    res = head_ablation(m, loader, topk=3)
    assert [np.array_equal(a, b) for a, b in zip(m.head_gates(), before)] == [True, True]
    base = evaluate(m, loader, topk=3)
    assert res["base"] == base and base["seen"] == 8 and res["blocks"] == [0, 1]
    for l in range(2):
        for h in range(2):
            g = before[l].copy()
            g[h] = 0.0
            m.set_head_gates({l: g})
            r = evaluate(m, loader, topk=3)
            m.set_head_gates({l: before[l]})
            assert res["acc1"][l][h] == r["acc1"] and res["acck"][l][h] == r["acck"], (l, h)
    assert evaluate(m, loader, topk=3) == base
    imp = importance_from_head_ablation(res)
    assert imp.shape == (2, 2) and np.array_equal(imp, base["acc1"] - np.array(res["acc1"]))
    one = head_ablation(m, loader, topk=3, blocks=(-1,))
    assert one["blocks"] == [1] and one["acc1"] == [res["acc1"][1]]
