"""Every kind of forward back to back on ONE handle with two lanes: nothing of a call may outlive
it. The other GPU suites pin the paths against each other bitwise, each on a fresh or single-purpose
handle; a tap list, a uint8 pointer or a lane slice left behind by one call would only show in the
next call on the same handle, which is what runs here.

Batch 3 over 2 lanes splits 1 + 2 (both the fp32 and the uint8 input offsets are scaled); batch 1
is below the lane count and runs on the parent; a profiled forward runs one lane on the parent.
Everything is compared bit for bit; the uint8 oracle is the fp32 forward of the normalised image
(tests/test_gpu_uint8_input.py).
"""
import ctypes

import pytest
import torch

from edgevisiontransformer_amd import Uint8Images, _lib
from tests.test_gpu_uint8_input import BATCH, DISTINCT, MODELS, NAN, _batch_bytes, _same

pytestmark = pytest.mark.gpu

# One image alone against its row of the batch, bit for bit: asserted for these families under the
# automatic GEMM selection (tests/test_gpu_t2t.py test_t2t_batch_independence, tests/test_gpu_swin.py
# test_swin_batch_independence_and_graph); a ViT is pinned to it only with the GEMM kernel fixed
# (tests/test_gpu_model.py test_batch_independence), so its batch of 1 is checked against a handle
# without lanes instead.
ROWS_INDEPENDENT = {"vit_ref_32": False, "t2t": True, "swin_stem96": True}


@pytest.mark.parametrize("name", sorted(ROWS_INDEPENDENT))
def test_back_to_back_on_one_laned_handle(gpu, name):
    lib = _lib.load_library()
    make, size, layout = MODELS[name]
    m = make(2, gpu, BATCH)
    assert m.lanes() == 2
    h, roles = ctypes.c_void_p(m._handle), _lib.PROF_ROLES
    u8 = Uint8Images(torch.from_numpy(_batch_bytes(size)).to(gpu), **DISTINCT)
    x = u8.to_float(layout)

    first = m(x).clone()                                              # 1: fp32, lanes 1 + 2
    feats = m.features(x, tokens=True, taps=(0, -1), logits=True)     # 2: features, two taps
    feats8 = m.features(u8, taps=(-1,), logits=True)                  # 3: uint8 features, a tap
    got8 = m(u8).clone()                                              # 4: uint8, lanes 1 + 2
    # 5: a tap past the last block, through the C ABI (the mirror refuses it on the host)
    guard = torch.full((BATCH, *m.tap_shape(-1)), NAN, device=gpu)
    bad = _lib.evt_features_args()
    blocks, taps = (ctypes.c_int32 * 1)(m.num_blocks), (ctypes.c_void_p * 1)(guard.data_ptr())
    bad.n_taps, bad.tap_blocks, bad.taps = 1, blocks, taps
    rc = lib.evt_forward_features(h, ctypes.c_void_p(x.data_ptr()), BATCH, ctypes.byref(bad),
                                  ctypes.c_void_p(_lib.stream_ptr(gpu)))
    assert rc == _lib.EVT_EINVAL and b"tap block" in lib.evt_last_error()
    last = m(x).clone()                                               # 6: fp32 again
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    assert _same(last, first)
    assert _same(got8, first)  # the oracle: the fp32 forward of the normalised image
    assert _same(feats["logits"], first) and _same(feats8["logits"], first)
    assert _same(feats8["pooled"], feats["pooled"]) and _same(feats8["taps"][0], feats["taps"][1])
    assert torch.isnan(guard).all()  # the refused call wrote nothing

    # a profiled forward runs one lane, on the parent (whose events these are), to the same bits
    _lib.check(lib.evt_model_profile(h, 1))
    for img in (x, u8):
        prof = m(img).clone()
        us, n = (ctypes.c_float * len(roles))(), (ctypes.c_int * len(roles))()
        _lib.check(lib.evt_model_profile_read(h, us, n))
        assert sum(n) > 0 and n[roles.index("head")] >= 1
        assert _same(prof, first)
    _lib.check(lib.evt_model_profile(h, 0))

    # batch 1 < 2 lanes: on the parent; fp32 and uint8
    one = m(x[:1].contiguous()).clone()
    one8 = m(Uint8Images(u8.data[:1], **DISTINCT)).clone()
    after = m(u8).clone()
    if ROWS_INDEPENDENT[name]:
        want1 = first[:1]
    else:
        single = make(1, gpu, BATCH)
        want1 = single(x[:1].contiguous()).clone()
        single.close()
    torch.cuda.synchronize()
    assert _same(one, want1) and _same(one8, want1)
    assert _same(after, first)
    m.close()
