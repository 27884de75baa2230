"""CPU: the CLS-tail interface (include/evt_tail.h) without a device.

  * header = `_lib.TAIL_SIGNATURES` = exported symbols, and evt.h includes the header;
  * the build tracks the header;
  * evt_model_tail_mode refuses null arguments before touching anything;
  * evt_query_workspace counts the tail's hidden rows ([B, ffn_st], ws.hc).
"""
import ctypes
import os
import re

import pytest

from edgevisiontransformer_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["evt_model_tail_mode"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from edgevisiontransformer_amd.build import build
        build()
    return _lib.load_library()


def test_header_binding_and_exports_agree(lib):
    txt = open(os.path.join(REPO, "include", "evt_tail.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(evt_\w+)\(", txt, re.M)))
    assert declared == sorted(_lib.TAIL_SIGNATURES) == ENTRY_POINTS
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.FEATURE_SIGNATURES) |
              set(_lib.IMAGE_SIGNATURES) | set(_lib.PREPROCESS_SIGNATURES) |
              set(_lib.ATTENTION_SIGNATURES))
    assert not set(declared) & others
    assert '#include "evt_tail.h"' in open(os.path.join(REPO, "include", "evt.h")).read()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.TAIL_SIGNATURES[name][1]


def test_build_tracks_the_header():
    from edgevisiontransformer_amd import build
    assert any(h.endswith("evt_tail.h") for h in build.HEADERS)


def test_null_arguments(lib):
    out = ctypes.c_int(7)
    assert lib.evt_model_tail_mode(None, ctypes.byref(out)) == _lib.EVT_EINVAL
    assert out.value == 7
    assert lib.evt_model_tail_mode(None, None) == _lib.EVT_EINVAL


def test_workspace_query_counts_the_hidden_rows(lib):
    """Everything else in the workspace is per token row; the tail's hidden rows are per image, so
    a query for B images is at least B * ffn_st elements above the token-row buffers' sum."""
    arr = (ctypes.c_int32 * 12)(*([12] * 12))
    hd = (ctypes.c_int32 * 12)(*([64] * 12))
    ffn = (ctypes.c_int32 * 12)(*([3072] * 12))
    d = _lib.evt_vit_desc(224, 16, 3, 1000, 768, 12, 3072, arr, hd, ffn, 1, 512)
    out = ctypes.c_size_t()
    assert lib.evt_query_workspace(ctypes.byref(d), 512, ctypes.byref(out)) == 0
    rows, es = 512 * 197, 2
    token_rows = rows * (2 * 768 * es + 2 * 6 * 8 + 3 * 768 * es + 768 * es + 3072 * es)
    assert out.value >= token_rows + 512 * 3072 * es + 512 * 3072 * es  # + hc + the head's hidden
