"""MI355X mirror of the reference `modeling/models/t2t_vit.py` (T2T_ViT, get_t2t_vit_*).

Same public names and constructor keywords as the reference; the Keras graph is replaced by one
call into libevt_hip.so (`evt_t2t_forward`, include/evt.h): soft splits (unfold), the two
TokenPerformers, the project Dense, the shared encoder and the LayerNorm-folded classifier run
as gfx950 kernels on the caller's stream.

    model = get_t2t_vit_14(dtype="bf16")   # reference: get_t2t_vit_14()    t2t_vit.py:147-148
    logits = model(img)                    # reference: T2T_ViT.call       t2t_vit.py:132-135

Input is channel-last like the reference (tf_Unfold is built with channel_last=True,
t2t_vit.py:50-52): fp32 NHWC [B, S, S, 3]. Deliberate differences, as for ViT: `seed=` /
`weights=` select the parameters (the reference random-initialises, t2t_vit.py:116-118), and
`dtype` selects the bf16 MFMA path or the exact fp32 path. Unsupported reference options fail
loudly: tokens_type other than 'performer' raises NotImplementedError (t2t_vit.py:58-59),
token_size must be 64, the head size hidden_size // num_heads at most 128.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ...weights import T2TConfig, make_t2t_params, t2t_config, t2t_param_shapes
from .depth import DepthAxis


class T2T_ViT(DepthAxis):
    """Tokens-to-Token ViT forward on MI355X (reference `T2T_ViT`, t2t_vit.py:91-135).
    `image_size`: a multiple of 16 with (image_size / 16)^2 + 1 <= 4096 tokens."""

    def __init__(self, image_size=224, tokens_type="performer", in_channels=3, num_classes=1000,
                 hidden_size=768, depth=12, num_heads=12, mlp_ratio=4., token_size=64,
                 qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., *, dtype: str = "bf16", seed: int = 0,
                 weights: Optional[Dict[str, np.ndarray]] = None, device=None,
                 max_batch: int = 0, lanes: Optional[int] = None):
        if tokens_type != "performer":  # t2t_vit.py:58-59
            raise NotImplementedError(
                "T2T_module with token_type other than performer is not supported")
        if hidden_size % num_heads != 0:  # Attention (attention.py:8-9)
            raise ValueError(f"hidden_size {hidden_size} must be a multiple of num_heads {num_heads}.")
        # qkv_bias / qk_scale / drop rates are accepted and unused, as in the reference (:92-94)
        self.cfg: T2TConfig = t2t_config(hidden_size, depth, num_heads, mlp_ratio,
                                         image_size=image_size, num_classes=num_classes,
                                         token_size=token_size, in_channels=in_channels)
        self.num_classes = num_classes
        self.num_features = self.hidden_size = hidden_size
        self._open_device(dtype, device)
        params = weights if weights is not None else make_t2t_params(self.cfg, seed=seed)
        for name, shape in t2t_param_shapes(self.cfg):
            a = np.asarray(params[name], dtype=np.float32)
            if a.size != int(np.prod(shape)):
                raise ValueError(f"weight {name}: shape {a.shape}, expected {shape}")
            self._weights.append(torch.from_numpy(np.ascontiguousarray(a.reshape(shape)))
                                 .to(self.device))
        self._open_handle(lanes, max_batch)

    _C_NUM_WEIGHTS, _C_CREATE = "evt_t2t_num_weights", "evt_t2t_create"
    _C_FORWARD, _C_QUERY_WORKSPACE = "evt_t2t_forward", "evt_t2t_query_workspace"

    def _desc(self, max_batch: int):
        c = self.cfg
        return _lib.evt_t2t_desc(c.image_size, c.in_chans, c.num_classes, c.dim, c.depth, c.heads,
                                 c.mlp_dim, c.token_size, _lib.DTYPE[self.dtype], max_batch)

    # -- feature outputs (features.py): forward_features = LN(x)[:, 0], t2t_vit.py:120-130 ------
    _TAP_NORM_OK = True

    def _feature_geometry(self):
        c = self.cfg
        return c.dim, c.tokens, [(c.tokens, c.dim)] * c.depth

    def _image_dims(self):
        c = self.cfg
        return c.image_size, c.image_size, c.in_chans

    # -- attention maps (attention_maps.py): the encoder blocks, not the token performers -------
    def _attn_geometry(self):
        c = self.cfg
        return [(c.heads, c.tokens)] * c.depth

    # -- head statistics (head_stats.py): the S/16 token grid of soft_split2 behind the CLS token -
    def _patch_grid_w(self):
        return self.cfg.image_size // 16

    # -- FFN statistics (ffn_stats.py): the encoder blocks' MLPs, not the token performers' -----
    def _ffn_geometry(self):
        c = self.cfg
        return [(c.mlp_dim, c.tokens)] * c.depth

    # -- activation Grams (grams.py): the encoder blocks' attention context is `dim` wide --------
    def _attn_context_geometry(self):
        c = self.cfg
        return [(c.dim, c.tokens)] * c.depth


def get_t2t_vit_7(**kw) -> T2T_ViT:
    return T2T_ViT(hidden_size=256, depth=7, num_heads=4, mlp_ratio=2, **kw)


def get_t2t_vit_10(**kw) -> T2T_ViT:
    return T2T_ViT(hidden_size=256, depth=10, num_heads=4, mlp_ratio=2, **kw)


def get_t2t_vit_12(**kw) -> T2T_ViT:
    return T2T_ViT(hidden_size=256, depth=12, num_heads=4, mlp_ratio=2, **kw)


def get_t2t_vit_14(**kw) -> T2T_ViT:
    return T2T_ViT(hidden_size=384, depth=14, num_heads=6, mlp_ratio=3, **kw)


_NAMED = {  # t2t_vit.py:138-148
    "t2t_vit_7": (256, 7, 4, 2),
    "t2t_vit_10": (256, 10, 4, 2),
    "t2t_vit_12": (256, 12, 4, 2),
    "t2t_vit_14": (384, 14, 6, 3),
}


def t2t_cfg_for(name: str) -> T2TConfig:
    """Host-only config of a named T2T-ViT (no GPU needed)."""
    return t2t_config(*_NAMED[name])


def build_named(name: str, **kw) -> T2T_ViT:
    h, d, nh, r = _NAMED[name]
    return T2T_ViT(hidden_size=h, depth=d, num_heads=nh, mlp_ratio=r, **kw)
