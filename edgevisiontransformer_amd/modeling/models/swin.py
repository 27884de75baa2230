"""MI355X Swin Transformer: the model the reference benchmarks through `get_swin`.

The reference does not implement Swin itself: `utils.py:14-47` (`get_swin(config_file_name,
swin_root_path)`) imports `SwinTransformer` from an external microsoft/Swin-Transformer checkout
and builds it from `configs/{config_file_name}.yaml`; `tools.py:272-282` benchmarks
`swin_tiny_patch4_window7_224` on NCHW [B, 3, 224, 224]. This module keeps that interface:

    model = get_swin("swin_tiny_patch4_window7_224", dtype="bf16")  # reference utils.py:14
    logits = model(img)                                             # SwinTransformer.forward
    model = get_swin("swin_base_patch4_window12_384", dtype="bf16")  # the 384 px configurations

`SwinTransformer(...)` takes the constructor keywords get_swin passes (utils.py:28-43). The yaml
files are not available offline, so the four published configs (tiny, small, base, large) are
built in (`edgevisiontransformer_amd.weights.SWIN_VARIANTS`), each at window 7 / 224 px and at
window 12 / 384 px, with the `_22k` / `_22kto1k` / `_22kto1k_finetune` name suffixes (21841 or
1000 classes); `swin_root_path` is accepted and ignored. Stage widths go up to 1536 (Swin-L).
The forward is one call into libevt_hip.so (`evt_swin_forward`, include/evt.h). Deliberate
differences: `seed=` / `weights=` select the parameters (Keras [in, out] dict, or
`params_from_state_dict` of a microsoft checkpoint), `dtype` selects bf16 MFMA or exact fp32;
inference only (dropout / drop-path are identity, as in eval mode). Unsupported options raise
ValueError: window_size other than 7 or 12, head size != 32, ape=True, patch_norm=False,
qkv_bias=False, qk_scale != None, a stage whose window (min(window_size, resolution), the
reference's clamp) is not 7 or 12 or does not divide its resolution.
"""
from __future__ import annotations

import re
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ...weights import SwinConfig, make_swin_params, swin_config, swin_param_shapes
from .depth import DepthAxis


class SwinTransformer(DepthAxis):
    """Swin Transformer forward on MI355X (microsoft `SwinTransformer`, built by reference
    `utils.py:28-43`). Stage widths (embed_dim * 2^i) up to 1536: Swin-T / S / B / L."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, num_classes=1000, embed_dim=96,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4.,
                 qkv_bias=True, qk_scale=None, drop_rate=0., drop_path_rate=0.1, ape=False,
                 patch_norm=True, use_checkpoint=False, *, dtype: str = "bf16", seed: int = 0,
                 weights: Optional[Dict[str, np.ndarray]] = None, device=None,
                 max_batch: int = 0, lanes: Optional[int] = None):
        if window_size not in (7, 12):
            raise ValueError("window_size must be 7 or 12 in this build")
        if ape or not patch_norm or not qkv_bias or qk_scale is not None:
            raise ValueError("this build supports ape=False, patch_norm=True, qkv_bias=True, "
                             "qk_scale=None (the published Swin configs)")
        if len(depths) != len(num_heads) or not 1 <= len(depths) <= _lib.SWIN_MAX_STAGES:
            raise ValueError("depths and num_heads must have the same length (1..8)")
        self.cfg: SwinConfig = SwinConfig(image_size=img_size, patch_size=patch_size,
                                          in_chans=in_chans, num_classes=num_classes,
                                          embed_dim=embed_dim, depths=tuple(depths),
                                          num_heads=tuple(num_heads), window_size=window_size,
                                          mlp_ratio=float(mlp_ratio))
        for i in range(self.cfg.num_stages):
            if self.cfg.dim(i) % num_heads[i] or self.cfg.dim(i) // num_heads[i] != 32:
                raise ValueError(f"stage {i}: head size {self.cfg.dim(i)}/{num_heads[i]} must be 32")
            w = self.cfg.window(i)
            if w not in (7, 12) or self.cfg.res(i) % w:
                raise ValueError(f"stage {i}: resolution {self.cfg.res(i)} is not a multiple of "
                                 f"{window_size} (window {w}; windows are 7 or 12)")
        self.num_classes = num_classes
        self.num_features = self.cfg.num_features
        self._open_device(dtype, device)
        params = weights if weights is not None else make_swin_params(self.cfg, seed=seed)
        for name, shape in swin_param_shapes(self.cfg):
            a = np.asarray(params[name], dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError(f"weight {name}: shape {a.shape}, expected {shape}")
            self._weights.append(torch.from_numpy(np.ascontiguousarray(a)).to(self.device))
        self._open_handle(lanes, max_batch)

    # -- C ABI plumbing (the handle itself: _handle.py) ----------------------------------------
    _C_NUM_WEIGHTS, _C_CREATE = "evt_swin_num_weights", "evt_swin_create"
    _C_FORWARD, _C_QUERY_WORKSPACE = "evt_swin_forward", "evt_swin_query_workspace"

    def _desc(self, max_batch: int) -> _lib.evt_swin_desc:
        c = self.cfg
        d = _lib.evt_swin_desc()
        d.image_size, d.patch_size, d.in_chans = c.image_size, c.patch_size, c.in_chans
        d.num_classes, d.embed_dim, d.num_stages = c.num_classes, c.embed_dim, c.num_stages
        for i in range(c.num_stages):
            d.depths[i] = c.depths[i]
            d.num_heads[i] = c.num_heads[i]
        d.window_size, d.mlp_ratio = c.window_size, c.mlp_ratio
        d.dtype, d.max_batch = _lib.DTYPE[self.dtype], max_batch
        return d

    forward = DepthAxis.__call__  # the microsoft name

    # -- feature outputs (features.py): forward_features = mean over tokens of LN(x) ----------
    def _feature_geometry(self):
        c = self.cfg
        last = c.num_stages - 1
        return c.num_features, c.res(last) ** 2, [(c.res(i) ** 2, c.dim(i))
                                                  for i in range(c.num_stages)
                                                  for _ in range(c.depths[i])]

    # -- window attention maps (window_attention_maps.py) --------------------------------------
    def _window_geometry(self):
        c = self.cfg
        return [(c.res(i), c.window(i), c.shift(i, j), c.num_heads[i])
                for i in range(c.num_stages) for j in range(c.depths[i])]

    def _image_dims(self):
        c = self.cfg
        return c.in_chans, c.image_size, c.image_size


_CONFIG_RE = re.compile(r"swin_(tiny|small|base|large)_patch(\d+)_window(\d+)_(\d+)"
                        r"(_22k|_22kto1k|_22kto1k_finetune)?$")
_CLASSES_22K = 21841  # ImageNet-22K head of the microsoft `_22k` configs


def swin_config_from_name(config_file_name: str, num_classes: Optional[int] = None) -> SwinConfig:
    """The SwinConfig of a microsoft config name (configs/swin_{tiny,small,base,large}_patch4_
    window7_224 or _window12_384, optionally with the `_22k` suffix: 21841 classes unless
    `num_classes` is given, or `_22kto1k` / `_22kto1k_finetune`: 1000 classes)."""
    m = _CONFIG_RE.match(config_file_name)
    if not m:
        raise NotImplementedError(f"Unkown model: {config_file_name}")  # utils.py:45 wording
    variant, patch, window, size = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
    if num_classes is None:
        num_classes = _CLASSES_22K if m.group(5) == "_22k" else 1000
    return swin_config(variant, patch_size=patch, window_size=window, image_size=size,
                       num_classes=num_classes)


def get_swin(config_file_name: str = "swin_tiny_patch4_window7_224", swin_root_path: str = "",
             **kw) -> SwinTransformer:
    """Reference `utils.py:14-47` (`get_swin`), with the published configs built in: swin_{tiny,
    small,base,large}_patch4_window7_224 / _window12_384 (+ `_22k`, `_22kto1k[_finetune]`)."""
    c = swin_config_from_name(config_file_name, kw.pop("num_classes", None))
    return SwinTransformer(img_size=c.image_size, patch_size=c.patch_size, in_chans=c.in_chans,
                           num_classes=c.num_classes, embed_dim=c.embed_dim, depths=c.depths,
                           num_heads=c.num_heads, window_size=c.window_size,
                           mlp_ratio=c.mlp_ratio, **kw)


def params_from_state_dict(sd: Dict[str, np.ndarray], cfg: SwinConfig) -> Dict[str, np.ndarray]:
    """Map a microsoft Swin-Transformer state dict (`model.state_dict()` / checkpoint['model'],
    torch [out, in] Linear weights) onto this module's Keras-layout parameter names."""
    a = lambda k: np.asarray(sd[k], dtype=np.float32)  # noqa: E731
    e = cfg.embed_dim
    p = {"patch_w": a("patch_embed.proj.weight").reshape(e, -1).T,
         "patch_b": a("patch_embed.proj.bias"),
         "pnorm_g": a("patch_embed.norm.weight"), "pnorm_b": a("patch_embed.norm.bias"),
         "norm_g": a("norm.weight"), "norm_b": a("norm.bias"),
         "head_w": a("head.weight").T, "head_b": a("head.bias")}
    for i in range(cfg.num_stages):
        if i > 0:  # microsoft attaches the merge of stage i to layers[i-1].downsample
            src = f"layers.{i - 1}.downsample."
            p[f"s{i}.merge_g"] = a(src + "norm.weight")
            p[f"s{i}.merge_b"] = a(src + "norm.bias")
            p[f"s{i}.merge_w"] = a(src + "reduction.weight").T
        for j in range(cfg.depths[i]):
            src, dst = f"layers.{i}.blocks.{j}.", f"s{i}.b{j}."
            p[dst + "ln1_g"], p[dst + "ln1_b"] = a(src + "norm1.weight"), a(src + "norm1.bias")
            p[dst + "qkv_w"], p[dst + "qkv_b"] = a(src + "attn.qkv.weight").T, a(src + "attn.qkv.bias")
            p[dst + "rpb"] = a(src + "attn.relative_position_bias_table")
            p[dst + "proj_w"], p[dst + "proj_b"] = a(src + "attn.proj.weight").T, a(src + "attn.proj.bias")
            p[dst + "ln2_g"], p[dst + "ln2_b"] = a(src + "norm2.weight"), a(src + "norm2.bias")
            p[dst + "fc1_w"], p[dst + "fc1_b"] = a(src + "mlp.fc1.weight").T, a(src + "mlp.fc1.bias")
            p[dst + "fc2_w"], p[dst + "fc2_b"] = a(src + "mlp.fc2.weight").T, a(src + "mlp.fc2.bias")
    return {k: np.ascontiguousarray(v) for k, v in p.items()}


def build_named(name: str, **kw) -> SwinTransformer:
    """'swin_tiny' | 'swin_small' | 'swin_base' | 'swin_large' (patch 4, window 7, 224)."""
    return get_swin(f"{name}_patch4_window7_224", **kw)
