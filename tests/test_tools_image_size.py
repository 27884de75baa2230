"""The image size the benchmark CLI derives from --input_shape (edgevisiontransformer_amd/tools.py):
NCHW for the DeiT / Swin models, NHWC for T2T-ViT, square shapes only, 224 by default. Host only."""
import inspect

import pytest

from edgevisiontransformer_amd import tools


def test_input_shape_parsing_and_defaults():
    assert tools._input_shape("deit_base", "64,3,384,384") == [64, 3, 384, 384]
    assert tools._input_shape("deit_base", None) == [1, 3, 224, 224]
    assert tools._input_shape("t2t_vit_14", None) == [1, 224, 224, 3]


def test_image_size_nchw():
    assert tools._image_size("deit_base", tools._input_shape("deit_base", "64,3,384,384")) == 384
    assert tools._image_size("swin_tiny", [2, 3, 224, 224]) == 224


def test_image_size_nhwc_t2t():
    assert tools._image_size("t2t_vit_7", tools._input_shape("t2t_vit_7", "1,272,272,3")) == 272


@pytest.mark.parametrize("name", ["deit_tiny", "t2t_vit_7", "swin_tiny"])
def test_default_is_224(name):
    assert tools._image_size(name, tools._input_shape(name, None)) == 224
    assert inspect.signature(tools.build_model).parameters["image_size"].default == 224


@pytest.mark.parametrize("name,spec", [("deit_base", "1,3,384,224"), ("t2t_vit_7", "1,224,272,3"),
                                       ("deit_tiny", "1,3,3,224")])
def test_non_square_raises(name, spec):
    with pytest.raises(ValueError):
        tools._image_size(name, tools._input_shape(name, spec))


def test_not_four_dimensions_raises():
    with pytest.raises(ValueError):
        tools._image_size("deit_tiny", [3, 224, 224])


def test_swin_is_224_only():
    # refused before any model is built (no GPU involved)
    with pytest.raises(ValueError, match="224"):
        tools.build_model("swin_tiny", "bf16", image_size=384)
