"""GPU: activation Grams (include/evt_gram.h; gram_kernel / gram_reduce_kernel in csrc/gram.hip).

Op level (evt_gram, f32 and bf16). The kernel as built: 128-wide tiles, row pieces of 64 (bf16) /
32 (fp32), row chunks of a multiple of 64 rows from 512 rows on (tests/_gram_ref.py lists the
shapes that follow: WIDTHS 8, 120, 128, 136, 256, 264, 776; ROWS 1, 2, 31, 32, 33, 63, 64, 65, 197,
511, 512, 513, 788; one 16 * 197 x 3072), each with ld = F and ld = F + 24, NaN in the padding
columns and around every buffer. Per element |G - Ghat| <= 8 R 2^-24 sum_r |a_ri a_rj| and the same
for the sums against the fp64 result of the stored values; integer probes bit for bit; the Gram
bitwise symmetric, a second call bitwise equal, the input untouched.

Model level (activation_grams / activation_grams_into / evt_forward_grams): the four tiny models of
tests/test_gpu_ffn_stats.py; logits and pooled bitwise the plain forward's; diag(G) and the sums
against ffn_stats of the same model; G and the sums against the fp64 forward's rows (f32: 1e-3 of
max|G|; bf16: the mean_sq gate of test_gpu_ffn_stats.py); refusals; profiling; and the end-to-end
repair of a ViT whose FC1 columns are duplicated.

Measured on an MI355X (the GRAM-* lines of a run): see DESIGN.md, "Activation Grams and
reconstruction".
"""
import ctypes

import numpy as np
import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib, collect_grams, pruning
from edgevisiontransformer_amd.modeling.models.grams import gram_reference
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.vit import StandardViT, ViT
from edgevisiontransformer_amd.weights import (make_images, make_std_vit_params, make_swin_params,
                                               make_t2t_params, make_vit_params, swin_config,
                                               vit_config)
from tests import _gram_ref as gr
from tests._ops import TDT, _p, _s
from tests.test_gpu_features import _buffer, _untouched, _written
from tests.test_gpu_ffn_stats import BF16_REL_GATE, MODELS, _host_image, _vit

pytestmark = pytest.mark.gpu
PAD = 64  # NaN elements before and after the input matrix


# ---- op level -------------------------------------------------------------------------------------
def _scratch(rows, width, gpu):
    n = ctypes.c_size_t()
    _lib.check(_lib.load_library().evt_gram_scratch_bytes(rows, width, ctypes.byref(n)))
    # all-ones bytes: NaN wherever a partial is read before it is written
    return torch.full((n.value,), 255, dtype=torch.uint8, device=gpu) if n.value else None


def _gram(dtype, a, ld, gpu):
    """evt_gram of the float32 host values a [R, F], stored with a pitch of ld and NaN padding ->
    (gram [F, F], sums [F]) on the device; checks the guards and that the input is untouched."""
    rows, f = a.shape
    host = torch.full((rows, ld), float("nan"), dtype=torch.float32)
    host[:, :f] = torch.from_numpy(np.ascontiguousarray(a))
    flat = torch.full((rows * ld + 2 * PAD,), float("nan"), dtype=TDT[dtype], device=gpu)
    flat[PAD:PAD + rows * ld] = host.reshape(-1).to(TDT[dtype]).to(gpu)
    before = flat.clone()
    dev = flat[PAD:PAD + rows * ld]
    gflat, g = _buffer((f, f), gpu)
    sflat, s = _buffer((f,), gpu)
    scratch = _scratch(rows, f, gpu)
    _lib.check(_lib.load_library().evt_gram(_lib.DTYPE[dtype], _p(dev), ld, rows, f, _p(g), _p(s),
                                            _p(scratch), scratch.numel() if scratch is not None else 0,
                                            _s()))
    torch.cuda.synchronize()
    assert _written(gflat) and _written(sflat), "NaN in gram / sums (padding read?) or a guard hit"
    bits = torch.int16 if dtype == "bf16" else torch.int32
    assert torch.equal(flat.view(bits), before.view(bits)), "the input was written"
    return g, s


def _check(dtype, a, ld, gpu, exact=False):
    """One matrix through the kernel and every op-level claim; the largest fraction of the gate."""
    g, s = _gram(dtype, a, ld, gpu)
    assert torch.equal(g, g.T.contiguous()), "gram is not bitwise symmetric"
    g2, s2 = _gram(dtype, a, ld, gpu)
    assert torch.equal(g, g2) and torch.equal(s, s2), "a second call differs"
    got_g, got_s = g.cpu().numpy(), s.cpu().numpy()
    if exact:
        want_g, want_s = gr.exact(a)
        assert np.array_equal(got_g, want_g) and np.array_equal(got_s, want_s)
        return 0.0
    ref = gr.reference(a)
    eg = np.abs(got_g.astype(np.float64) - ref["gram"])
    es = np.abs(got_s.astype(np.float64) - ref["sum"])
    assert (eg <= ref["gram_gate"]).all() and (es <= ref["sum_gate"]).all()
    tiny = np.finfo(np.float64).tiny
    return max((eg / np.maximum(ref["gram_gate"], tiny)).max(),
               (es / np.maximum(ref["sum_gate"], tiny)).max())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("f", gr.WIDTHS)
def test_gram_op(gpu, f, dtype):
    worst = 0.0
    for rows in gr.ROWS:
        a = gr.normal(rows, f, dtype, seed=rows + f)
        for ld in (f, f + gr.PAD_COLS):
            worst = max(worst, _check(dtype, a, ld, gpu))
    print(f"GRAM-OP-MAX {dtype} F{f}: {worst:.4f} of the gate")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("f", gr.WIDTHS)
def test_gram_op_exact_probes(gpu, f, dtype):
    for ld in (f, f + gr.PAD_COLS):
        for rows in (65, 788):
            _check(dtype, gr.probe_single(rows, f), ld, gpu, exact=True)
            _check(dtype, gr.probe_dense(rows, f, seed=f), ld, gpu, exact=True)
        _check(dtype, gr.probe_pairs(f), ld, gpu, exact=True)
        _check(dtype, gr.probe_pairs(f, repeat=8 if f > 128 else 300), ld, gpu, exact=True)  # also in row chunks


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gram_op_big(gpu, dtype):
    """16 * 197 rows of 3072 columns (300 tiles, one chunk); the fp64 reference on the device."""
    rows, f = gr.BIG
    gen = torch.Generator(device="cpu").manual_seed(5)
    a = (torch.randn((rows, f), generator=gen) * 0.5 + 0.25).to(TDT[dtype]).to(gpu)
    gflat, g = _buffer((f, f), gpu)
    sflat, s = _buffer((f,), gpu)
    assert _scratch(rows, f, gpu) is None
    _lib.check(_lib.load_library().evt_gram(_lib.DTYPE[dtype], _p(a), f, rows, f, _p(g), _p(s),
                                            None, 0, _s()))
    torch.cuda.synchronize()
    assert _written(gflat) and _written(sflat)
    assert torch.equal(g, g.T.contiguous())
    x = a.double()
    scale = gr.MARGIN * rows * 2.0 ** -24
    eg = (g.double() - x.T @ x).abs() / (scale * (x.abs().T @ x.abs()))
    es = (s.double() - x.sum(0)).abs() / (scale * x.abs().sum(0))
    print(f"GRAM-OP-BIG {dtype}: {max(eg.max().item(), es.max().item()):.4f} of the gate")
    assert eg.max().item() <= 1.0 and es.max().item() <= 1.0


def test_gram_op_errors_write_nothing(gpu):
    lib = _lib.load_library()
    a = torch.zeros((600 * 64 + 16,), dtype=torch.bfloat16, device=gpu)
    gflat, g = _buffer((64, 64), gpu)
    sflat, s = _buffer((64,), gpu)
    scratch = _scratch(600, 64, gpu)
    assert scratch is not None
    P = ctypes.c_void_p
    ok = dict(dtype=1, a=a.data_ptr(), ld=64, rows=600, width=64, gram=g.data_ptr(),
              sums=s.data_ptr(), scratch=scratch.data_ptr(), nbytes=scratch.numel())
    assert lib.evt_gram(*[P(v) if k in ("a", "gram", "sums", "scratch") else v
                          for k, v in ok.items()], _s()) == _lib.EVT_OK
    torch.cuda.synchronize()
    g.fill_(float("nan"))
    s.fill_(float("nan"))
    for kw in (dict(dtype=2), dict(a=None), dict(gram=None), dict(sums=None), dict(rows=0),
               dict(rows=2 ** 31), dict(width=0), dict(width=60), dict(width=6152, ld=6152),
               dict(ld=56), dict(ld=68), dict(a=a.data_ptr() + 8), dict(gram=g.data_ptr() + 4),
               dict(sums=s.data_ptr() + 8), dict(scratch=scratch.data_ptr() + 8),
               dict(scratch=None), dict(nbytes=scratch.numel() - 1), dict(nbytes=0)):
        c = {**ok, **kw}
        rc = lib.evt_gram(c["dtype"], P(c["a"]), c["ld"], c["rows"], c["width"], P(c["gram"]),
                          P(c["sums"]), P(c["scratch"]), c["nbytes"], _s())
        assert rc == _lib.EVT_EINVAL and b"gram" in lib.evt_last_error(), kw
    # fp32 takes a multiple of 4, bf16 does not
    f32 = torch.zeros((4, 12), dtype=torch.float32, device=gpu)
    assert lib.evt_gram(1, P(f32.data_ptr()), 16, 4, 12, P(g.data_ptr()), P(s.data_ptr()), None, 0,
                        _s()) == _lib.EVT_EINVAL
    torch.cuda.synchronize()
    assert _untouched(gflat) and _untouched(sflat)


# ---- model level ----------------------------------------------------------------------------------
_ROWS = {}


def _reference_rows(name, cfg):
    """{"ffn": [...], "attn": [...]}: gram_reference of every block's fp64 rows of the model `name`
    on its image; computed once on the CPU, shared by the f32 and bf16 tests, read-only."""
    if name not in _ROWS:
        img, seed = _host_image(name), MODELS[name][3]
        if name == "std":
            hidden, ctx, _ = gr.std_vit_rows(make_std_vit_params(cfg, seed=seed), cfg, img)
        elif name == "t2t":
            hidden, ctx = gr.t2t_rows(make_t2t_params(cfg, seed=seed), cfg, img)
        else:
            hidden, ctx, _ = gr.vit_rows(make_vit_params(cfg, seed=seed), cfg, img)
        _ROWS[name] = {"ffn": [gram_reference(h) for h in hidden],
                       "attn": [gram_reference(c) for c in ctx]}
    return _ROWS[name]


def _run(m, x, what, blocks=None, logits=True, pooled=False):
    """activation_grams_into on guarded buffers -> {"gram": [...], "sum": [...], "logits", ...}."""
    b, gpu = x.shape[0], m.device
    blocks = list(range(m.num_blocks)) if blocks is None else list(blocks)
    widths = [m.gram_shape(i, what)[0] for i in blocks]
    gb = [_buffer((f, f), gpu) for f in widths]
    sb = [_buffer((f,), gpu) for f in widths]
    extra = {}
    if logits:
        extra["logits"] = _buffer((b, m.num_classes), gpu)
    if pooled:
        extra["pooled"] = _buffer((b, m.feature_dim), gpu)
    m.activation_grams_into(x, blocks=blocks, what=what, gram_tensors=[v for _, v in gb],
                            sum_tensors=[v for _, v in sb], **{k: v for k, (_, v) in extra.items()})
    torch.cuda.synchronize()
    for flat, _ in gb + sb + list(extra.values()):
        assert _written(flat), "NaN left in an output or guard words overwritten"
    out = {k: v for k, (_, v) in extra.items()}
    out["gram"], out["sum"] = [v for _, v in gb], [v for _, v in sb]
    return out


def _same(u, v):
    return all(torch.equal(a, b) for k in ("gram", "sum") for a, b in zip(u[k], v[k]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("what,name", [("ffn", n) for n in MODELS] +
                         [("attn", n) for n in MODELS])
def test_model_grams(gpu, name, what, dtype):
    m = MODELS[name][0](dtype, 1, gpu)
    x = torch.from_numpy(_host_image(name)).to(gpu)
    plain = m(x).clone()
    pooled = m.forward_features(x).clone()
    out = _run(m, x, what, pooled=True)  # every block, the last one included
    assert torch.equal(out["logits"], plain) and torch.equal(out["pooled"], pooled)
    assert torch.equal(m(x), plain)  # a plain forward after a Gram forward is unchanged
    tokens = m.gram_shape(0, what)[1]
    rows = x.shape[0] * tokens
    if what == "ffn":  # diag(G) and the sums against the other kernel that reads the same rows
        stats = [s.double().cpu().numpy() for s in m.ffn_stats(x)["stats"]]
        scale = gr.MARGIN * rows * 2.0 ** -24
        for g, s, st in zip(out["gram"], out["sum"], stats):
            sq, sm, ab = (tokens * st[:, :, k].sum(0) for k in (2, 0, 1))
            dg, ds = np.diag(g.double().cpu().numpy()), s.double().cpu().numpy()
            assert (np.abs(dg - sq) <= scale * sq).all() and (np.abs(ds - sm) <= scale * ab).all()
    ref = _reference_rows(name, m.cfg)[what]
    worst = [0.0, 0.0]
    for i, (g, s, r) in enumerate(zip(out["gram"], out["sum"], ref)):
        width = m.gram_shape(i, what)[0]
        assert tuple(g.shape) == (width, width) == r["gram"].shape and r["rows"] == rows
        assert torch.equal(g, g.T.contiguous())
        rel = [np.abs(g.double().cpu().numpy() - r["gram"]).max() / np.abs(r["gram"]).max(),
               np.abs(s.double().cpu().numpy() - r["sum"]).max() / np.abs(r["sum"]).max()]
        print(f"GRAM-MODEL {name} {what} {dtype} block {i} F{width} R{rows}: gram {rel[0]:.3e} "
              f"sum {rel[1]:.3e}")
        worst = [max(a, b) for a, b in zip(worst, rel)]
    print(f"GRAM-MODEL-MAX {name} {what} {dtype}: gram {worst[0]:.3e} sum {worst[1]:.3e}")
    gate = 1e-3 if dtype == "f32" else BF16_REL_GATE[2]
    assert max(worst) <= gate, f"{worst} against the gate {gate}"
    if name == "pruned" and what == "ffn":
        assert [g.shape[0] for g in out["gram"]] == [384, 768, 230]  # ragged; 230 < its pitch 256
    # a second call, a single late block and the order given; no logits: no classifier head
    late = m.activation_grams(x, blocks=(-1, 0), what=what)
    assert sorted(late) == ["gram", "rows", "sum"] and late["rows"] == rows
    assert torch.equal(late["gram"][0], out["gram"][-1]) and torch.equal(late["sum"][1], out["sum"][0])
    # the last block alone, with logits and pooled: still bitwise the plain forward's
    last = _run(m, x, what, blocks=(m.num_blocks - 1,), pooled=True)
    assert torch.equal(last["logits"], plain) and torch.equal(last["pooled"], pooled)
    assert torch.equal(last["gram"][0], out["gram"][-1])
    # lanes = 2: the call runs as one lane on the handle's own workspace
    m2 = MODELS[name][0](dtype, 2, gpu)
    assert m2.lanes() == 2 and _same(_run(m2, x, what, logits=False), out)


def test_grams_uint8_and_numpy(gpu):
    m = _vit("bf16", 1, gpu)
    rng = np.random.default_rng(7)
    u8 = Uint8Images(torch.from_numpy(rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)).to(gpu))
    for what in ("ffn", "attn"):
        want = _run(m, u8.to_float("nchw"), what)
        got = _run(m, u8, what)
        assert torch.equal(got["logits"], want["logits"]) and _same(got, want)
        host = m.activation_grams(u8.to_float("nchw").cpu().numpy(), what=what, logits=True)
        assert isinstance(host["logits"], np.ndarray) and len(host["gram"]) == m.num_blocks
        assert all(np.array_equal(u, v.cpu().numpy()) for u, v in zip(host["gram"], want["gram"]))


def test_grams_head_major_layout(gpu, monkeypatch):
    """The QKV GEMM stores head-major only from the batch at which it takes the persistent kernel:
    20 images of a 384-wide StandardViT at 224 px reach it in both layers (asserted; the recipe of
    tests/test_gpu_depth.py). The attention writes the same context rows from either layout, so
    the attention Grams, the FFN Grams behind them and the logits are bitwise those of an
    EVT_QKV_LAYOUT=token handle."""
    cfg = vit_config(384, 2, 6, 1536, image_size=224, patch_size=16, num_classes=16)
    params = make_std_vit_params(cfg, seed=63)
    x = torch.from_numpy(make_images(20, seed=69, image_size=224)).to(gpu)
    build = lambda: StandardViT(image_size=224, patch_size=16, num_classes=16, dim=384, depth=2,  # noqa: E731
                                heads=6, dtype="bf16", weights=params, device=gpu, max_batch=20, lanes=1)

    def run(m, layers):
        out = [_run(m, x, what) for what in ("attn", "ffn")]
        assert m.qkv_headmajor_layers() == layers
        return out

    head = run(build(), 2)
    assert torch.equal(head[0]["logits"], head[1]["logits"])
    monkeypatch.setenv("EVT_QKV_LAYOUT", "token")
    mt = build()
    monkeypatch.delenv("EVT_QKV_LAYOUT")
    token = run(mt, 0)
    for u, v in zip(head, token):
        assert _same(u, v) and torch.equal(u["logits"], v["logits"])


def test_grams_under_profile_count_as_head(gpu):
    m = _vit("bf16", 1, gpu)
    x = torch.from_numpy(_host_image("vit")).to(gpu)
    lib = _lib.load_library()
    head = _lib.PROF_ROLES.index("head")
    us = (ctypes.c_float * len(_lib.PROF_ROLES))()
    n = (ctypes.c_int * len(_lib.PROF_ROLES))()

    def launches(run):
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 1))
        run()
        torch.cuda.synchronize()
        _lib.check(lib.evt_model_profile_read(ctypes.c_void_p(m._handle), us, n))
        _lib.check(lib.evt_model_profile(ctypes.c_void_p(m._handle), 0))
        return list(n)

    others = lambda c: [v for i, v in enumerate(c) if i != head]  # noqa: E731
    plain = launches(lambda: m(x))
    one = launches(lambda: _run(m, x, "ffn", blocks=(1,)))
    every = launches(lambda: _run(m, x, "attn"))
    tapped = launches(lambda: m.features(x, taps=(-1,), logits=True))
    assert one[head] == plain[head] + 1 and every[head] == plain[head] + 3
    assert others(one) == others(plain) and others(every) == others(tapped)
    assert launches(lambda: m(x)) == plain


def test_grams_refusals(gpu):
    cfg = swin_config("tiny", image_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6),
                      num_classes=11)
    s = SwinTransformer(img_size=56, patch_size=cfg.patch_size, num_classes=11,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=7, dtype="bf16", weights=make_swin_params(cfg, seed=3),
                        device=gpu, max_batch=1, lanes=1)
    xs = torch.zeros((1, 3, 56, 56), device=gpu)
    m8 = ViT(dim=128, depth=2, heads=2, mlp_dim=256, image_size=32, patch_size=16, num_classes=16,
             dtype="mx8", device=gpu, max_batch=1, lanes=1)
    x8 = torch.zeros((1, 3, 32, 32), device=gpu)
    for what in ("ffn", "attn"):
        with pytest.raises(ValueError, match="no activation Grams"):
            s.activation_grams(xs, what=what)
        with pytest.raises(ValueError, match="mx8"):
            m8.activation_grams(x8, what=what)
    lib = _lib.load_library()
    m = _vit("bf16", 1, gpu)
    x = torch.from_numpy(_host_image("vit")).to(gpu)
    gflat, g = _buffer((768, 768), gpu)
    sflat, sm = _buffer((768,), gpu)

    def call(model, img, blocks, which=0, grams=None, sums=None, batch=2, n_blocks=None):
        a = _lib.evt_gram_args()
        a.n_blocks = len(blocks) if n_blocks is None else n_blocks
        a.which = which
        k = max(1, len(blocks))
        keep = ((ctypes.c_int32 * k)(*blocks),
                (ctypes.c_void_p * k)(*(grams if grams is not None else [g.data_ptr()] * len(blocks))),
                (ctypes.c_void_p * k)(*(sums if sums is not None else [sm.data_ptr()] * len(blocks))))
        a.blocks, a.grams, a.sums = keep
        args = _lib.evt_image_args()
        args.data = img.data_ptr()
        rc = lib.evt_forward_grams(ctypes.c_void_p(model._handle), ctypes.byref(args), batch, None,
                                   ctypes.byref(a), _s())
        return rc, lib.evt_last_error()

    bad = {
        "swin": dict(model=s, img=xs, blocks=[0], batch=1),
        "mx8": dict(model=m8, img=x8, blocks=[0], batch=1),
        "which": dict(blocks=[0], which=2),
        "n_blocks 65": dict(blocks=[0], n_blocks=65),
        "nothing requested": dict(blocks=[]),
        "NULL gram pointer": dict(blocks=[0], grams=[None]),
        "NULL sums pointer": dict(blocks=[0], sums=[None]),
        "block out of range": dict(blocks=[3]),
        "blocks not increasing": dict(blocks=[1, 0]),
        "gram misaligned": dict(blocks=[0], grams=[g.data_ptr() + 4]),
        "sums misaligned": dict(blocks=[0], sums=[sm.data_ptr() + 8]),
        "batch over max_batch": dict(blocks=[0], batch=3),
    }
    for what, kw in bad.items():
        rc, msg = call(**{"model": m, "img": x, **kw})
        assert rc == _lib.EVT_EINVAL and msg, what
    w, t = ctypes.c_int(), ctypes.c_int()
    for model, blk, which in ((s, 0, 0), (m8, 0, 0), (m, 3, 0), (m, 0, 2)):
        assert lib.evt_gram_shape(ctypes.c_void_p(model._handle), blk, which, ctypes.byref(w),
                                  ctypes.byref(t)) == _lib.EVT_EINVAL
    _lib.check(lib.evt_gram_shape(ctypes.c_void_p(m._handle), 2, 1, ctypes.byref(w), ctypes.byref(t)))
    assert (w.value, t.value) == (192, 65) == m.gram_shape(2, "attn")
    assert m.gram_shape(-1, "ffn") == (768, 65)
    # a token schedule and a skipped sublayer: ValueError with the library's message
    m.set_token_pruning({0: 32})
    with pytest.raises(ValueError, match="token schedule"):
        m.activation_grams(x, blocks=(0,))
    m.set_token_pruning(None)
    m.skip_sublayers({1: "ffn", 2: "attn"})
    with pytest.raises(ValueError, match="FFN sublayer is skipped"):
        m.activation_grams(x, blocks=(1,), what="ffn")
    with pytest.raises(ValueError, match="attention sublayer is skipped"):
        m.activation_grams(x, blocks=(2,), what="attn")
    ok = m.activation_grams(x, blocks=(1,), what="attn")  # block 1's attention still runs
    assert torch.isfinite(ok["gram"][0]).all()
    m.clear_skips()
    torch.cuda.synchronize()
    assert _untouched(gflat) and _untouched(sflat)
    for kw in (dict(blocks=(3,)), dict(blocks=(0, 0)), dict(what="mlp")):
        with pytest.raises(ValueError):
            m.activation_grams(x, **kw)
    with pytest.raises(ValueError):
        m.activation_grams_into(x, blocks=(0,), gram_tensors=(torch.empty((768, 767), device=gpu),),
                                sum_tensors=(torch.empty((768,), device=gpu),))


def test_repair_of_duplicated_neurons_end_to_end(gpu):
    """f32 tiny ViT whose FC1 neurons 384 .. 767 copy neurons 0 .. 383: collect_grams over 16 images
    (1040 rows for 384 kept neurons), reconstruct_vit_params, build_pruned_vit. The repaired model
    must be strictly closer to the dense one than the plain cut on the calibration images."""
    cfg = vit_config(192, 3, 3, 768, image_size=32, patch_size=4, num_classes=16)
    params = {k: np.array(v, copy=True) for k, v in make_vit_params(cfg, seed=71).items()}
    for i in range(cfg.depth):
        params[f"l{i}.fc1_w"][:, 384:] = params[f"l{i}.fc1_w"][:, :384]
        params[f"l{i}.fc1_b"][384:] = params[f"l{i}.fc1_b"][:384]
    kw = dict(dtype="f32", device=gpu, max_batch=8, lanes=1)
    dense = ViT(dim=192, depth=3, heads=3, mlp_dim=768, image_size=32, patch_size=4, num_classes=16,
                weights=params, **kw)
    images = make_images(16, seed=9, image_size=32)
    loader = [images[:8], images[8:]]
    grams = collect_grams(dense, loader, what="ffn")
    assert grams["rows"] == 1040 and grams["gram"][0].shape == (768, 768)
    kept_heads, kept_ffn = [[0, 1, 2]] * 3, [list(range(384))] * 3
    fixed = pruning.reconstruct_vit_params(params, cfg, kept_ffn=kept_ffn, ffn_grams=grams)
    want = np.concatenate([dense(b) for b in loader])
    err = []
    for p in (fixed, params):
        pruned = pruning.build_pruned_vit(p, cfg, kept_heads, kept_ffn, **kw)
        got = np.concatenate([pruned(b) for b in loader])
        err.append(float(((got - want) ** 2).mean()))
    print(f"GRAM-REPAIR mean squared logit difference: repaired {err[0]:.3e} plain cut {err[1]:.3e} "
          f"ratio {err[0] / err[1]:.3e}")
    assert err[0] < err[1]
