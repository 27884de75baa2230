"""GPU: what a live handle's workspace asked for (include/evt_workspace.h) is what the query says.

One small config per family (the ones of tests/test_workspace_host.py) at max_batch 4, in bf16 and
fp32: with one lane evt_model_workspace_bytes equals the query for 4 images; with two lanes the
two children's workspaces for 2 images each come on top; back at one lane they are gone. A forward
runs in every state. The one-lane forwards before and after are the same launches on the same
handle: bitwise equal. The laned forward splits 4 images into 2 + 2, where a part may take other
kernels than the whole batch (tests/test_gpu_lanes.py): within that file's 3e-2 of the one-lane
logits, and bitwise each part's own one-lane forward.
"""
import ctypes

import pytest
import torch

from edgevisiontransformer_amd import _lib
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import get_t2t_vit_7
from edgevisiontransformer_amd.modeling.models.vit import ViT
from edgevisiontransformer_amd.weights import make_images

pytestmark = pytest.mark.gpu
B = 4


def _build(family, dtype, gpu):
    kw = dict(dtype=dtype, seed=0, max_batch=B, lanes=1, device=gpu)
    if family == "vit":
        return ViT(dim=192, depth=2, heads=3, mlp_dim=768, **kw), dict()
    if family == "t2t":
        return get_t2t_vit_7(**kw), dict(layout="NHWC")
    return SwinTransformer(img_size=56, depths=(2, 2), num_heads=(3, 6), num_classes=37,
                           **kw), dict(image_size=56)


@pytest.mark.parametrize("family", ["vit", "t2t", "swin"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_handle_workspace_is_the_query(gpu, family, dtype):
    m, img_kw = _build(family, dtype, gpu)
    img = torch.from_numpy(make_images(B, seed=44, **img_kw)).to(gpu)
    lib, s = _lib.load_library(), ctypes.c_void_p(_lib.stream_ptr(gpu))
    q4, q2 = m.workspace_bytes(4), m.workspace_bytes(2)
    assert m.lanes() == 1 and m.allocated_workspace_bytes() == q4
    one = m(img)
    parts = [m(img[:2].contiguous()), m(img[2:].contiguous())]
    torch.cuda.synchronize()
    assert torch.isfinite(one).all()

    _lib.check(lib.evt_model_set_lanes(m._ptr(), 2, s))
    assert m.lanes() == 2 and m.allocated_workspace_bytes() == q4 + 2 * q2
    two = m(img)
    torch.cuda.synchronize()
    assert torch.equal(two, torch.cat(parts))
    assert float((two - one).abs().max()) <= 3e-2

    _lib.check(lib.evt_model_set_lanes(m._ptr(), 1, s))
    assert m.lanes() == 1 and m.allocated_workspace_bytes() == q4
    assert torch.equal(m(img), one)
    assert lib.evt_model_workspace_bytes(m._ptr(), None) == _lib.EVT_EINVAL
