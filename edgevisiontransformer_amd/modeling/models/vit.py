"""MI355X mirror of the reference `modeling/models/vit.py` (ViT, ViT_Pruned, get_deit_*).

Same public names, constructor keywords and prune-encoding grammar as the reference; the Keras
graph is replaced by one call into libevt_hip.so (`evt_vit_forward`, include/evt.h), which runs
the whole forward as hand-written gfx950 kernels on the caller's HIP stream.

    model = get_deit_base(dtype="bf16")          # reference: get_deit_base()  vit.py:100-101
    logits = model(img)                          # reference: ViT.call          vit.py:41-55

Differences that are deliberate and documented:
  * Weights. The reference random-initialises Keras variables (vit.py:18-39) and never loads a
    checkpoint on this path. Here `seed=` selects the deterministic generator of
    `edgevisiontransformer_amd.weights` (same init families); `weights=` accepts an explicit
    {name: array} dict in the Keras [in, out] layout instead.
  * `dtype`: "bf16" (bf16 MFMA, fp32 accumulate/statistics; the throughput path) or "f32" (exact
    fp32 MFMA; logits within 1e-3 of the fp64 oracle).
  * Input: fp32 NCHW [B, 3, H, W] torch tensor on the GPU (or a numpy array, copied in).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from .depth import DepthAxis
from ...weights import (ViTConfig, make_std_vit_params, make_vit_params, std_vit_param_shapes,
                        vit_config, vit_param_shapes)


def decode_prune_encoding(prune_encoding: str):
    """Reference `ViT_Pruned.decode_prune_encoding` (vit.py:77-97), same grammar and asserts.

    'all_head{N}_ffn{F}'                  -> ('all', N, F)
    'layerwise_h{N}-d{F}_h{N}-d{F}_...'   -> ('layerwise', [N...], [F...])
    """
    tokens = prune_encoding.split("_")
    prune_setting = tokens[0]
    assert prune_setting in ["layerwise", "all"]
    if prune_setting == "all":
        head_setting = tokens[1]
        ffn_setting = tokens[2]
        num_heads = int(head_setting.replace("head", ""))
        ffn_threshold = float(ffn_setting.replace("ffn", ""))
        return prune_setting, num_heads, ffn_threshold
    num_heads_list = []
    ffn_threshold_list = []
    for token in tokens[1:]:
        hx, dx = token.split("-")
        num_heads_list.append(int(hx.replace("h", "")))
        ffn_threshold_list.append(float(dx.replace("d", "")))
    return prune_setting, num_heads_list, ffn_threshold_list


class ViT(DepthAxis):
    """Vision Transformer forward on MI355X (reference `ViT`, vit.py:9-55).

    `image_size` / `patch_size`: any pair with (image_size / patch_size)^2 + 1 <= 4096 tokens per
    image (224 px: 197; 384 px as `get_torch_deit`, utils.py:52-62: 577; patch 14: 257 at 224 px,
    1370 at 518 px; "mx8": <= 256 tokens); the factories (`get_deit_*`, `build_named`) pass
    `image_size=` through. `dim`: a multiple of 8 up to 1536 ("mx8": of 64, up to 1024).
    `token_keep`: a token schedule `{block: keep}` (token_pruning.py `set_token_pruning`)."""

    SEMANTICS = _lib.VIT_REFERENCE
    _TOKEN_PRUNING_OK = True
    _GATES_OK = True
    _DEPTH_OK = True
    _param_shapes = staticmethod(vit_param_shapes)
    _make_params = staticmethod(make_vit_params)
    layer_norm_eps = 0.0  # 0: the library default 1e-5 (reference norm.py:6)

    def __init__(self, *, image_size=224, patch_size=16, num_classes=1000, dim=768, depth=12,
                 heads=12, mlp_dim=3072, dtype: str = "bf16", seed: int = 0,
                 weights: Optional[Dict[str, np.ndarray]] = None, device=None, max_batch: int = 0,
                 lanes: Optional[int] = None, token_keep=None,
                 _cfg: Optional[ViTConfig] = None):
        assert image_size % patch_size == 0, "image dimensions must be divisible by the patch size"
        if _cfg is None:
            if dim % heads != 0:  # reference Attention raises ValueError (attention.py:8-9)
                raise ValueError(f"hidden_size {dim} must be a multiple of num_heads {heads}.")
            _cfg = vit_config(dim, depth, heads, mlp_dim, image_size=image_size,
                              patch_size=patch_size, num_classes=num_classes)
        self.cfg = _cfg
        self.image_size, self.patch_size = image_size, patch_size
        self.num_classes, self.dim, self.depth, self.mlp_dim = num_classes, dim, depth, mlp_dim
        self._open_device(dtype, device)
        self.set_token_pruning(token_keep)  # {block: keep} (token_pruning.py); applied by _build
        params = weights if weights is not None else self._make_params(self.cfg, seed=seed)
        for name, shape in self._param_shapes(self.cfg):
            a = np.asarray(params[name], dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                if a.size == int(np.prod(shape)) and name == "cls":
                    a = a.reshape(shape)
                else:
                    raise ValueError(f"weight {name}: shape {a.shape}, expected {shape}")
            self._weights.append(torch.from_numpy(np.ascontiguousarray(a)).to(self.device))
        self._arrays = None
        self._open_handle(lanes, max_batch)

    # -- C ABI plumbing (the handle itself: _handle.py) ----------------------------------------
    _C_NUM_WEIGHTS, _C_CREATE = "evt_vit_num_weights", "evt_vit_create"
    _C_FORWARD, _C_QUERY_WORKSPACE = "evt_vit_forward", "evt_query_workspace"
    _DEFAULT_LANES_KW = {"vit": True}

    def _desc(self, max_batch: int):
        c = self.cfg
        arr = lambda v: (ctypes.c_int32 * max(1, len(v)))(*v)  # noqa: E731
        heads, hd, ffn = arr(list(c.heads)), arr(list(c.head_dim)), arr(list(c.ffn))
        self._arrays = (heads, hd, ffn)  # keep alive
        return _lib.evt_vit_desc(c.image_size, c.patch_size, c.in_chans, c.num_classes, c.dim,
                                 c.depth, c.mlp_dim, heads, hd, ffn, _lib.DTYPE[self.dtype],
                                 max_batch, self.SEMANTICS, self.layer_norm_eps)

    def qkv_headmajor_layers(self) -> int:
        """Encoder layers whose QKV output was stored head-major in the last forward
        (evt_model_qkv_layout; diagnostics for the layout-equality tests)."""
        out = ctypes.c_int()
        _lib.check(_lib.load_library().evt_model_qkv_layout(self._ptr(), ctypes.byref(out)))
        return out.value

    # -- feature outputs (features.py: forward_features, features, features_into) -------------
    _TAP_NORM_OK = False  # no final LayerNorm (vit.py:54); StandardViT has one

    def _feature_geometry(self):
        c = self.cfg
        return c.dim, c.tokens, [(c.tokens, c.dim)] * c.depth

    def _image_dims(self):
        c = self.cfg
        return c.in_chans, c.image_size, c.image_size

    # -- attention maps (attention_maps.py): a pruned model's heads differ per block ------------
    def _attn_geometry(self):
        c = self.cfg
        return [(int(h), c.tokens) for h in list(c.heads)[:c.depth]]

    # -- head statistics (head_stats.py): token 0 is the CLS token, the rest the patch grid ------
    def _patch_grid_w(self):
        return self.cfg.image_size // self.cfg.patch_size

    # -- FFN statistics (ffn_stats.py): a pruned model's FFN widths differ per block ------------
    def _ffn_geometry(self):
        c = self.cfg
        return [(int(f), c.tokens) for f in list(c.ffn)[:c.depth]]

    # -- activation Grams (grams.py): the attention context is heads * head_dim wide -------------
    def _attn_context_geometry(self):
        c = self.cfg
        return [(int(h) * int(d), c.tokens)
                for h, d in zip(list(c.heads)[:c.depth], list(c.head_dim)[:c.depth])]


class ViT_Pruned(ViT):
    """Head/FFN-pruned ViT (reference `ViT_Pruned`, vit.py:58-75)."""

    def __init__(self, *, image_size=224, patch_size=16, num_classes=1000, dim=768, depth=12,
                 heads=12, mlp_dim=3072, head_size=64, prune_encoding="all_head12_ffn1.0",
                 **kw):
        prune_setting, num_remain_heads, ffn_thresholds = self.decode_prune_encoding(prune_encoding)
        if prune_setting == "all":
            num_remain_heads_list = [num_remain_heads for _ in range(depth)]
            intermediate_size_list = [int(ffn_thresholds * mlp_dim) for _ in range(depth)]
        else:
            assert len(num_remain_heads) == depth and len(ffn_thresholds) == depth
            num_remain_heads_list = num_remain_heads
            intermediate_size_list = [int(ffn_thresholds[i] * mlp_dim) for i in range(depth)]
        self.prune_encoding = prune_encoding
        self.num_remain_heads_list = num_remain_heads_list
        self.intermediate_size_list = intermediate_size_list
        cfg = vit_config(dim, depth, heads, mlp_dim, image_size=image_size, patch_size=patch_size,
                         num_classes=num_classes, head_size=head_size,
                         heads_list=num_remain_heads_list, ffn_list=intermediate_size_list)
        super().__init__(image_size=image_size, patch_size=patch_size, num_classes=num_classes,
                         dim=dim, depth=depth, heads=heads, mlp_dim=mlp_dim, _cfg=cfg, **kw)

    @staticmethod
    def decode_prune_encoding(prune_encoding: str):
        return decode_prune_encoding(prune_encoding)


def get_deit_base(**kw) -> ViT:
    return ViT(dim=768, depth=12, **kw)


def get_deit_small(**kw) -> ViT:
    return ViT(dim=384, heads=6, mlp_dim=384 * 4, **kw)


def get_deit_tiny(**kw) -> ViT:
    return ViT(dim=192, heads=3, mlp_dim=192 * 4, **kw)


def pruned_config(prune_encoding: str, *, dim: int, depth: int, heads: int, mlp_dim: int,
                  head_size: int = 64, image_size=224, patch_size=16, num_classes=1000) -> ViTConfig:
    """The ViTConfig a `ViT_Pruned(...)` builds (host-only; no GPU needed)."""
    setting, nh, thr = decode_prune_encoding(prune_encoding)
    if setting == "all":
        hl, fl = [nh] * depth, [int(thr * mlp_dim)] * depth
    else:
        assert len(nh) == depth and len(thr) == depth
        hl, fl = nh, [int(t * mlp_dim) for t in thr]
    return vit_config(dim, depth, heads, mlp_dim, image_size=image_size, patch_size=patch_size,
                      num_classes=num_classes, head_size=head_size, heads_list=hl, ffn_list=fl)


class StandardViT(ViT):
    """The published DeiT / ViT architecture (timm `VisionTransformer`, HF `ViTForImageClassification`
    — what the reference evaluates for accuracy via `get_torch_deit`, utils.py:52-62): pre-norm
    residual x + f(LN(x)), QKV with bias, exact GELU, final LayerNorm, Linear head on the CLS token.
    Load real checkpoints with `params_from_timm_state_dict` / `params_from_hf_state_dict`."""

    SEMANTICS = _lib.VIT_STANDARD
    _TAP_NORM_OK = True
    _param_shapes = staticmethod(std_vit_param_shapes)
    _make_params = staticmethod(make_std_vit_params)

    def __init__(self, *, image_size=224, patch_size=16, num_classes=1000, dim=768, depth=12,
                 heads=12, mlp_ratio=4.0, layer_norm_eps=1e-6, **kw):
        self.layer_norm_eps = float(layer_norm_eps)
        super().__init__(image_size=image_size, patch_size=patch_size, num_classes=num_classes,
                         dim=dim, depth=depth, heads=heads, mlp_dim=int(dim * mlp_ratio), **kw)


def deit_tiny_patch16_224(**kw) -> StandardViT:
    return StandardViT(dim=192, heads=3, **kw)


def deit_small_patch16_224(**kw) -> StandardViT:
    return StandardViT(dim=384, heads=6, **kw)


def deit_base_patch16_224(**kw) -> StandardViT:
    return StandardViT(dim=768, heads=12, **kw)


# The large published ViTs (timm vit_large_patch16_224, vit_large_patch14_224,
# vit_huge_patch14_224; the MAE / CLIP / DINOv2 backbones): L = 1024 wide, 24 layers, 16 heads of
# 64; H = 1280 wide, 32 layers, 16 heads of 80; MLP ratio 4. Patch 14 gives 16 x 16 + 1 = 257
# tokens at 224 px (518 px: 1370).
STD_VIT_NAMED = {
    "vit_large_patch16_224": dict(dim=1024, depth=24, heads=16, patch_size=16),
    "vit_large_patch14_224": dict(dim=1024, depth=24, heads=16, patch_size=14),
    "vit_huge_patch14_224": dict(dim=1280, depth=32, heads=16, patch_size=14),
}


def _std_named(name: str, kw: dict) -> StandardViT:
    return StandardViT(**{**STD_VIT_NAMED[name], **kw})  # a keyword of the caller's wins (depth=2)


def vit_large_patch16_224(**kw) -> StandardViT:
    return _std_named("vit_large_patch16_224", kw)


def vit_large_patch14_224(**kw) -> StandardViT:
    return _std_named("vit_large_patch14_224", kw)


def vit_huge_patch14_224(**kw) -> StandardViT:
    return _std_named("vit_huge_patch14_224", kw)


def build_std_named(name: str, **kw) -> StandardViT:
    return _std_named(name, kw)


def _patch_rows(conv_w: np.ndarray) -> np.ndarray:
    """Conv2d kernel [D, C, p, p] -> patch_w [p*p*C, D] in this build's (p1 p2 c) vector order
    (the reference's einops pattern, vit.py:31-32), for any patch size p (14: 588 rows; the
    library's own K order and row padding are internal to evt_vit_create)."""
    d = conv_w.shape[0]
    return np.ascontiguousarray(conv_w.transpose(2, 3, 1, 0).reshape(-1, d))


def params_from_timm_state_dict(sd: Dict[str, np.ndarray], depth: int) -> Dict[str, np.ndarray]:
    """timm `VisionTransformer` / `deit_*_patch16_224` state dict -> StandardViT parameters."""
    a = lambda k: np.asarray(sd[k], dtype=np.float32)  # noqa: E731
    p = {"patch_w": _patch_rows(a("patch_embed.proj.weight")), "patch_b": a("patch_embed.proj.bias"),
         "cls": a("cls_token").reshape(-1), "pos": a("pos_embed")[0],
         "norm_g": a("norm.weight"), "norm_b": a("norm.bias"),
         "head_w": a("head.weight").T, "head_b": a("head.bias")}
    for i in range(depth):
        s = f"blocks.{i}."
        p.update({f"l{i}.ln1_g": a(s + "norm1.weight"), f"l{i}.ln1_b": a(s + "norm1.bias"),
                  f"l{i}.qkv_w": a(s + "attn.qkv.weight").T, f"l{i}.qkv_b": a(s + "attn.qkv.bias"),
                  f"l{i}.out_w": a(s + "attn.proj.weight").T, f"l{i}.out_b": a(s + "attn.proj.bias"),
                  f"l{i}.ln2_g": a(s + "norm2.weight"), f"l{i}.ln2_b": a(s + "norm2.bias"),
                  f"l{i}.fc1_w": a(s + "mlp.fc1.weight").T, f"l{i}.fc1_b": a(s + "mlp.fc1.bias"),
                  f"l{i}.fc2_w": a(s + "mlp.fc2.weight").T, f"l{i}.fc2_b": a(s + "mlp.fc2.bias")})
    return {k: np.ascontiguousarray(v) for k, v in p.items()}


def params_from_hf_state_dict(sd: Dict[str, np.ndarray], depth: int) -> Dict[str, np.ndarray]:
    """HF `ViTForImageClassification` (facebook/deit-*-patch16-224) state dict -> parameters."""
    a = lambda k: np.asarray(sd[k], dtype=np.float32)  # noqa: E731
    e = "vit.embeddings."
    p = {"patch_w": _patch_rows(a(e + "patch_embeddings.projection.weight")),
         "patch_b": a(e + "patch_embeddings.projection.bias"),
         "cls": a(e + "cls_token").reshape(-1), "pos": a(e + "position_embeddings")[0],
         "norm_g": a("vit.layernorm.weight"), "norm_b": a("vit.layernorm.bias"),
         "head_w": a("classifier.weight").T, "head_b": a("classifier.bias")}
    for i in range(depth):
        s = f"vit.layers.{i}."
        q, k, v = (a(s + f"attention.{n}_proj.weight") for n in "qkv")
        qb, kb, vb = (a(s + f"attention.{n}_proj.bias") for n in "qkv")
        p.update({f"l{i}.ln1_g": a(s + "layernorm_before.weight"),
                  f"l{i}.ln1_b": a(s + "layernorm_before.bias"),
                  f"l{i}.qkv_w": np.concatenate([q, k, v], 0).T,
                  f"l{i}.qkv_b": np.concatenate([qb, kb, vb]),
                  f"l{i}.out_w": a(s + "attention.o_proj.weight").T,
                  f"l{i}.out_b": a(s + "attention.o_proj.bias"),
                  f"l{i}.ln2_g": a(s + "layernorm_after.weight"),
                  f"l{i}.ln2_b": a(s + "layernorm_after.bias"),
                  f"l{i}.fc1_w": a(s + "mlp.fc1.weight").T, f"l{i}.fc1_b": a(s + "mlp.fc1.bias"),
                  f"l{i}.fc2_w": a(s + "mlp.fc2.weight").T, f"l{i}.fc2_b": a(s + "mlp.fc2.bias")})
    return {k: np.ascontiguousarray(v) for k, v in p.items()}


_NAMED = {
    "deit_base": dict(dim=768, depth=12, heads=12, mlp_dim=3072),   # vit.py:100-101
    "deit_small": dict(dim=384, depth=12, heads=6, mlp_dim=1536),   # vit.py:104-105
    "deit_tiny": dict(dim=192, depth=12, heads=3, mlp_dim=768),     # vit.py:108-109
}


def _cfg_for(name: str) -> ViTConfig:
    """Host-only config of a named DeiT (no GPU needed)."""
    return vit_config(**_NAMED[name])


def build_named(name: str, **kw) -> ViT:
    return ViT(**_NAMED[name], **kw)
