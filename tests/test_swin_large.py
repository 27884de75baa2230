"""Swin-L on the host: the swin_large config names (with the microsoft `_22k` / `_22kto1k`
suffixes), the state-dict mapping at Swin-L widths, and the numpy oracle at stage width 1536 (the
shape the GPU tests of tests/test_gpu_swin_large.py lean on)."""
import numpy as np
import pytest

from edgevisiontransformer_amd.modeling.models.swin import (params_from_state_dict,
                                                            swin_config_from_name)
from edgevisiontransformer_amd.weights import (SWIN_VARIANTS, make_images, make_swin_params,
                                               swin_config, swin_param_shapes)
from oracle import swin_ref

# the two-stage model of the GPU tests: stage 0 at R = 14 (2 x 2 windows), stage 1 at R = 7, 1536 wide
TWO_STAGE = dict(embed_dim=768, depths=(1, 2), num_heads=(24, 48), window_size=7, image_size=56,
                 num_classes=13)


def two_stage_cfg():
    return swin_config("large", **TWO_STAGE)


@pytest.mark.parametrize("name,window,size", [("swin_large_patch4_window7_224", 7, 224),
                                              ("swin_large_patch4_window12_384", 12, 384)])
def test_swin_large_config_names(name, window, size):
    c = swin_config_from_name(name)
    assert c.embed_dim == 192 and tuple(c.depths) == (2, 2, 18, 2)
    assert tuple(c.num_heads) == (6, 12, 24, 48)
    assert [c.dim(i) for i in range(4)] == [192, 384, 768, 1536]
    assert (c.window_size, c.image_size, c.patch_size, c.num_classes) == (window, size, 4, 1000)
    assert all(c.dim(i) // c.num_heads[i] == 32 for i in range(4))
    assert SWIN_VARIANTS["large"]["embed_dim"] == 192


@pytest.mark.parametrize("variant", ["tiny", "small", "base", "large"])
def test_swin_22k_suffixes(variant):
    base = f"swin_{variant}_patch4_window7_224"
    assert swin_config_from_name(base + "_22k").num_classes == 21841
    assert swin_config_from_name(base + "_22k", num_classes=5).num_classes == 5
    assert swin_config_from_name(base + "_22kto1k").num_classes == 1000
    assert swin_config_from_name(base + "_22kto1k_finetune").num_classes == 1000
    c = swin_config_from_name(f"swin_{variant}_patch4_window12_384_22kto1k_finetune")
    assert (c.window_size, c.image_size, c.num_classes) == (12, 384, 1000)
    assert c.embed_dim == SWIN_VARIANTS[variant]["embed_dim"]


@pytest.mark.parametrize("name", ["swin_huge_patch4_window7_224", "swin_large_patch4_window7_224_21k",
                                  "swin_large_patch4_window7", "large_patch4_window7_224",
                                  "swin_large_patch4_window7_224_22kto1k_finetuned"])
def test_swin_junk_names_raise(name):
    with pytest.raises(NotImplementedError, match="Unkown model"):
        swin_config_from_name(name)


def test_tools_names_swin_large():
    from edgevisiontransformer_amd import tools
    assert "swin_large" in tools.SWIN_NAMED


def test_swin_large_state_dict_round_trip():
    """A synthetic microsoft-style state dict (torch [out, in] Linear weights, the merge under
    layers[i - 1].downsample) of a depth-trimmed Swin-L maps back onto the seeded parameters."""
    cfg = swin_config("large", depths=(1, 1, 2, 1), num_classes=17)
    params = make_swin_params(cfg, seed=3)
    sd = {"patch_embed.proj.weight": params["patch_w"].T.reshape(192, 3, 4, 4),
          "patch_embed.proj.bias": params["patch_b"],
          "patch_embed.norm.weight": params["pnorm_g"], "patch_embed.norm.bias": params["pnorm_b"],
          "norm.weight": params["norm_g"], "norm.bias": params["norm_b"],
          "head.weight": params["head_w"].T, "head.bias": params["head_b"]}
    for i in range(cfg.num_stages):
        if i > 0:
            d = f"layers.{i - 1}.downsample."
            sd[d + "norm.weight"], sd[d + "norm.bias"] = params[f"s{i}.merge_g"], params[f"s{i}.merge_b"]
            sd[d + "reduction.weight"] = params[f"s{i}.merge_w"].T
        for j in range(cfg.depths[i]):
            s, p = f"layers.{i}.blocks.{j}.", f"s{i}.b{j}."
            sd[s + "norm1.weight"], sd[s + "norm1.bias"] = params[p + "ln1_g"], params[p + "ln1_b"]
            sd[s + "attn.qkv.weight"], sd[s + "attn.qkv.bias"] = params[p + "qkv_w"].T, params[p + "qkv_b"]
            sd[s + "attn.relative_position_bias_table"] = params[p + "rpb"]
            sd[s + "attn.proj.weight"], sd[s + "attn.proj.bias"] = params[p + "proj_w"].T, params[p + "proj_b"]
            sd[s + "norm2.weight"], sd[s + "norm2.bias"] = params[p + "ln2_g"], params[p + "ln2_b"]
            sd[s + "mlp.fc1.weight"], sd[s + "mlp.fc1.bias"] = params[p + "fc1_w"].T, params[p + "fc1_b"]
            sd[s + "mlp.fc2.weight"], sd[s + "mlp.fc2.bias"] = params[p + "fc2_w"].T, params[p + "fc2_b"]
    back = params_from_state_dict(sd, cfg)
    shapes = swin_param_shapes(cfg)
    assert dict(shapes)["s3.b0.qkv_w"] == (1536, 4608) and dict(shapes)["s3.merge_w"] == (3072, 1536)
    assert set(back) == {n for n, _ in shapes}
    for name, shape in shapes:
        assert back[name].shape == tuple(shape), name
        assert np.array_equal(back[name], params[name]), name


def test_oracle_at_width_1536():
    """swin_ref.swin_forward on the two-stage model (stage 1 at width 1536): finite logits, and an
    image's logits do not depend on its batch neighbours."""
    cfg = two_stage_cfg()
    assert [cfg.dim(i) for i in range(2)] == [768, 1536] and [cfg.res(i) for i in range(2)] == [14, 7]
    params = make_swin_params(cfg, seed=21)
    img = make_images(3, seed=22, image_size=56)
    full = swin_ref.swin_forward(params, cfg, img)
    assert full.shape == (3, 13) and np.isfinite(full).all()
    one = swin_ref.swin_forward(params, cfg, img[1:2])
    assert np.allclose(full[1:2], one, rtol=0, atol=1e-9)
