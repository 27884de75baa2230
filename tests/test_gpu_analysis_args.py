"""The argument checks and the launch sequence of the analysis forwards (evt_forward_features,
_image, _attention, _head_stats, _ffn_stats, _rollout, _window_attention, _token_pruning and
_classify), pinned on the smallest model of each family.

  * every rejected argument set is EVT_EINVAL with the full evt_last_error() text, the doubly-bad
    sets fix the order the checks fire in, and a valid call after the rejected ones still gives
    bitwise the logits of `model(img)`: a rejected call launches nothing and leaves nothing behind;
  * under evt_model_profile every analysis forward of the first and the last block makes the
    launches written down here, role by role (evt_model_profile_read counts the event pairs of a
    role: the full-row and the CLS-tail launch of a last block share their role's pair), and
    `tail_mode()` is 3 when the call exports the last block's rows (a tap, FFN statistics), else 1.

The messages are literals: the text is part of the interface.
"""
import ctypes

import pytest
import torch

from edgevisiontransformer_amd import _lib
from edgevisiontransformer_amd.modeling.models.swin import SwinTransformer
from edgevisiontransformer_amd.modeling.models.t2t_vit import T2T_ViT
from edgevisiontransformer_amd.modeling.models.vit import StandardViT

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
B = 2           # the batch of every valid call, and every handle's max_batch
WORDS = 1 << 19  # fp32 words of an output buffer: more than any single output of these models

BATCH = "batch must be in [1, max_batch=2]"
SCHEDULE = (" is not available while a token schedule is set: the stream drops tokens between "
            "blocks (clear it with evt_model_set_token_schedule(m, 0, ...))")
NO_FEAT = "no output requested: logits, pooled and tokens are NULL, n_taps is 0"
# the block list of each entry point: (args struct, its count / blocks / pointers fields) and the
# messages of the list checks
TAPS = dict(
    struct=(_lib.evt_features_args, "n_taps", "tap_blocks", "taps"),
    count="n_taps must be in [0, 64]", none=NO_FEAT,
    arrays="n_taps > 0 needs the tap_blocks and taps arrays",
    block="tap block {} is outside [0, {})", rising="tap_blocks must be strictly increasing",
    null="tap pointer {} is NULL", align="feature outputs must be 16-byte aligned",
    align_last=True)  # one alignment check after the loop: a later bad block is reported first
MAPS = dict(
    struct=(_lib.evt_attn_args, "n_maps", "blocks", "maps"),
    count="n_maps must be in [0, 64]", none="no output requested: n_maps is 0 and feat is NULL",
    arrays="n_maps > 0 needs the blocks and maps arrays",
    block="map block {} is outside [0, {})", rising="map blocks must be strictly increasing",
    null="map pointer {} is NULL", align="attention maps must be 16-byte aligned", align_last=False)
HSTATS = dict(
    struct=(_lib.evt_head_stats_args, "n_blocks", "blocks", "stats"),
    count="n_blocks must be in [0, 64]", none="no output requested: n_blocks is 0 and feat is NULL",
    arrays="n_blocks > 0 needs the blocks and stats arrays",
    block="head statistics block {} is outside [0, {})",
    rising="head statistics blocks must be strictly increasing",
    null="stats pointer {} is NULL", align="head statistics must be 16-byte aligned",
    align_last=False)
FSTATS = dict(HSTATS, struct=(_lib.evt_ffn_stats_args, "n_blocks", "blocks", "stats"),
              block="FFN statistics block {} is outside [0, {})",
              rising="FFN statistics blocks must be strictly increasing",
              align="FFN statistics must be 16-byte aligned")
LISTS = {"evt_forward_features": TAPS, "evt_forward_image": TAPS, "evt_forward_classify": TAPS,
         "evt_forward_rollout": TAPS, "evt_forward_token_pruning": TAPS,
         "evt_forward_attention": MAPS, "evt_forward_window_attention": MAPS,
         "evt_forward_head_stats": HSTATS, "evt_forward_ffn_stats": FSTATS}
# who refuses which family: {entry point: {family: message}}
WRONG_FAMILY = {
    "evt_forward_attention": {"swin": "attention maps: Swin's windowed, biased attention is not exported"},
    "evt_forward_head_stats": {"swin": "attention maps: Swin's windowed, biased attention is not exported"},
    "evt_forward_ffn_stats": {"swin": "FFN statistics: Swin's fused MLP does not store its hidden rows"},
    "evt_forward_rollout": {"swin": "attention rollout: Swin's windowed attention does not compose this "
                                    "way (per-window maps: evt_forward_window_attention)"},
    "evt_forward_window_attention": {
        f: "window attention maps are Swin's: this model's maps are evt_forward_attention's"
        for f in ("vit", "t2t")},
    "evt_forward_token_pruning": {
        "swin": "token pruning: Swin's windows need the whole token grid",
        "t2t": "token pruning: T2T-ViT is not supported yet (ViT handles only)"},
}
NO_SCHEDULE = ("forward_token_pruning: the model has no token schedule "
               "(evt_model_set_token_schedule first)")


class Handle:
    """A built mirror with a batch, its plain logits and the device buffers the calls name."""

    def __init__(self, family, model, shape, gpu):
        self.family, self.m, self.h = family, model, P(model._handle)
        g = torch.Generator().manual_seed(5)
        self.img = torch.randn((B, *shape), generator=g).to(gpu)
        self.want = model(self.img).clone()
        self.blocks = model.num_blocks
        self.logits = torch.full((B, model.num_classes), float("nan"), device=gpu)
        self.pooled = torch.empty((B, model.feature_dim), device=gpu)
        self.out = [torch.empty(WORDS, device=gpu) for _ in range(3)]
        self.ints = torch.empty((B, 4), dtype=torch.int32, device=gpu)
        self.p = [t.data_ptr() for t in self.out]
        assert all(p % 16 == 0 for p in self.p)


@pytest.fixture(scope="module")
def handles(gpu):
    kw = dict(dtype="bf16", device=gpu, max_batch=B, lanes=1)
    return {
        "vit": Handle("vit", StandardViT(dim=64, depth=2, heads=1, mlp_ratio=2.0, image_size=32,
                                         patch_size=16, num_classes=8, seed=1, **kw), (3, 32, 32), gpu),
        "t2t": Handle("t2t", T2T_ViT(hidden_size=256, depth=2, num_heads=4, mlp_ratio=2,
                                     num_classes=8, seed=2, **kw), (224, 224, 3), gpu),
        "swin": Handle("swin", SwinTransformer(img_size=56, num_classes=8, depths=(2, 2),
                                               num_heads=(3, 6), seed=3, **kw), (3, 56, 56), gpu),
    }


def _stream(gpu):
    return P(_lib.stream_ptr(gpu))


def _fill(struct, blocks, ptrs, n=None, null_arrays=False, **fields):
    """(args, what keeps its arrays alive) of one block list."""
    cls, count, blk, ptr = struct
    a = cls()
    setattr(a, count, len(blocks) if n is None else n)
    keep = ((ctypes.c_int32 * max(1, len(blocks)))(*blocks), (P * max(1, len(ptrs)))(*ptrs))
    if not null_arrays:
        setattr(a, blk, keep[0])
        setattr(a, ptr, keep[1])
    for k, v in fields.items():
        setattr(a, k, v)
    return a, keep


def call(H, fn, lst=None, batch=B, logits=False, pooled=False, tokens=False, feat=None):
    """(return code, evt_last_error()) of entry point `fn` on handle H. `lst`: the keywords of
    `_fill` for fn's own block list (LISTS[fn]; the feature outputs' tap list where that is the
    list). `logits` / `pooled` / `tokens`: the feature outputs asked for beside it."""
    lib = _lib.load_library()
    spec = LISTS[fn]
    own_taps = spec is TAPS
    lst = dict(lst or dict(blocks=(), ptrs=()))
    f, keep_f = _fill(TAPS["struct"], **(lst if own_taps else dict(blocks=(), ptrs=())))
    f.logits = H.logits.data_ptr() if logits else None
    f.pooled = H.pooled.data_ptr() if pooled else None
    f.tokens = H.out[2].data_ptr() if tokens else None
    has_feat = own_taps or logits or pooled or tokens if feat is None else feat
    fp = ctypes.byref(f) if has_feat else None
    img = _lib.evt_image_args()
    img.data, img.format = H.img.data_ptr(), 0
    s = _stream(H.img.device)
    if fn == "evt_forward_features":
        rc = lib.evt_forward_features(H.h, P(H.img.data_ptr()), batch, fp, s)
    elif fn == "evt_forward_image":
        rc = lib.evt_forward_image(H.h, ctypes.byref(img), batch, fp, s)
    elif fn == "evt_forward_classify":
        c = _lib.evt_classify_args()
        c.k, c.values, c.indices = 1, _lib.CLASSIFY_PROB, H.ints.data_ptr()
        rc = lib.evt_forward_classify(H.h, ctypes.byref(img), batch, fp, ctypes.byref(c), s)
    elif fn == "evt_forward_rollout":
        r = _lib.evt_rollout_args()
        r.start, r.mode, r.out = 0, _lib.ROLLOUT_CLS, H.p[2]
        r.scratch, r.scratch_bytes = H.p[1], WORDS * 4
        rc = lib.evt_forward_rollout(H.h, ctypes.byref(img), batch, fp, ctypes.byref(r), s)
    elif fn == "evt_forward_token_pruning":
        rc = lib.evt_forward_token_pruning(H.h, ctypes.byref(img), batch, fp, None, s)
    else:
        extra = dict(queries=_lib.ATTN_ALL) if spec is MAPS else {}
        a, keep_a = _fill(spec["struct"], **lst, **extra)
        rc = getattr(lib, fn)(H.h, ctypes.byref(img), batch, fp, ctypes.byref(a), s)
    return rc, lib.evt_last_error().decode()


def rejected(H, fn, message, **kw):
    rc, msg = call(H, fn, **kw)
    assert (rc, msg) == (_lib.EVT_EINVAL, message), (H.family, fn, kw)


def check_valid(H, fn, want=None, **kw):
    """A valid call of fn with logits: EVT_OK and bitwise the plain forward's logits."""
    H.logits.fill_(float("nan"))
    rc, msg = call(H, fn, logits=True, **kw)
    assert rc == _lib.EVT_OK, (H.family, fn, msg)
    torch.cuda.synchronize()
    assert torch.equal(H.logits, H.want if want is None else want), (H.family, fn)


def list_cases(H, fn, needs_logits=False):
    """Every bad block list of fn on H, alone and in the doubly-bad pairs that fix the order."""
    spec, nb, (p0, p1, _) = LISTS[fn], H.blocks, H.p
    kw = dict(logits=True) if needs_logits else {}
    two = dict(blocks=(0, nb - 1), ptrs=(p0, p1))
    for n in (-1, 65):
        rejected(H, fn, spec["count"], lst=dict(two, n=n), **kw)
        rejected(H, fn, spec["count"], lst=dict(two, n=n), batch=0, **kw)  # the count, then the batch
    if not needs_logits:
        rejected(H, fn, spec["none"], lst=dict(blocks=(), ptrs=()))
        rejected(H, fn, spec["none"], lst=dict(blocks=(), ptrs=()), batch=0)
    for batch in (0, B + 1):
        rejected(H, fn, BATCH, lst=two, batch=batch, **kw)
        rejected(H, fn, BATCH, lst=dict(blocks=(nb,), ptrs=(p0 + 4,)), batch=batch, **kw)
    rejected(H, fn, spec["arrays"], lst=dict(blocks=(0,), ptrs=(p0,), null_arrays=True), **kw)
    rejected(H, fn, spec["block"].format(-1, nb), lst=dict(blocks=(-1,), ptrs=(p0,)), **kw)
    rejected(H, fn, spec["block"].format(nb, nb), lst=dict(blocks=(nb,), ptrs=(p0,)), **kw)
    rejected(H, fn, spec["block"].format(nb, nb), **kw,  # 64 entries pass the count check
             lst=dict(blocks=tuple(range(64)), ptrs=(p0,) * 64))
    rejected(H, fn, spec["rising"], lst=dict(blocks=(0, 0), ptrs=(p0, p1)), **kw)
    rejected(H, fn, spec["rising"], lst=dict(blocks=(nb - 1, 0), ptrs=(p0, p1)), **kw)
    rejected(H, fn, spec["null"].format(1), lst=dict(blocks=(0, nb - 1), ptrs=(p0, None)), **kw)
    rejected(H, fn, spec["null"].format(0), lst=dict(blocks=(0, nb - 1), ptrs=(None, p1 + 4)), **kw)
    rejected(H, fn, spec["align"], lst=dict(blocks=(0, nb - 1), ptrs=(p0, p1 + 4)), **kw)
    # a bad block and a misaligned pointer: in one entry the block; the pointer of an earlier
    # entry where the list checks alignment entry by entry, the later block where it checks it
    # once after the loop (the feature outputs)
    rejected(H, fn, spec["block"].format(nb, nb), lst=dict(blocks=(nb,), ptrs=(p0 + 4,)), **kw)
    first = spec["block"].format(nb, nb) if spec["align_last"] else spec["align"]
    rejected(H, fn, first, lst=dict(blocks=(0, nb), ptrs=(p0 + 4, p1)), **kw)
    rejected(H, fn, spec["rising"], lst=dict(blocks=(0, 0), ptrs=(p0, p1 + 4)), **kw)


LIST_FNS = {"vit": ("evt_forward_features", "evt_forward_image", "evt_forward_attention",
                    "evt_forward_head_stats", "evt_forward_ffn_stats", "evt_forward_rollout"),
            "t2t": ("evt_forward_features", "evt_forward_image", "evt_forward_attention",
                    "evt_forward_head_stats", "evt_forward_ffn_stats", "evt_forward_rollout"),
            "swin": ("evt_forward_features", "evt_forward_image", "evt_forward_window_attention")}


@pytest.mark.parametrize("family", ["vit", "t2t", "swin"])
def test_bad_lists_are_rejected_in_order(handles, family):
    H = handles[family]
    one = dict(blocks=(0,), ptrs=(H.p[0],))
    for fn in LIST_FNS[family]:
        list_cases(H, fn)
        check_valid(H, fn, lst=one)
    # evt_forward_classify needs feat->logits, so its list never comes without an output
    list_cases(H, "evt_forward_classify", needs_logits=True)
    rejected(H, "evt_forward_classify", "forward_classify: feat->logits is required (the caller "
             "owns the logits the classification reads)", lst=dict(blocks=(0,), ptrs=(H.p[0],), n=65))
    check_valid(H, "evt_forward_classify", lst=one)
    # the feature outputs' own alignment: pooled and the taps are checked together, after the loop
    H.pooled = H.out[2][1:1 + H.pooled.numel()].view_as(H.pooled)
    try:
        for fn in ("evt_forward_features", "evt_forward_attention"
                   if family != "swin" else "evt_forward_window_attention"):
            lst = dict(blocks=(H.blocks,), ptrs=(H.p[0],))
            spec = LISTS[fn]
            if spec is TAPS:  # the tap's bad block, ahead of pooled's alignment
                rejected(H, fn, spec["block"].format(H.blocks, H.blocks), lst=lst, pooled=True)
                rejected(H, fn, spec["align"], lst=one, pooled=True)
            else:  # feat is validated ahead of the entry point's own list
                rejected(H, fn, TAPS["align"], lst=lst, pooled=True)
    finally:
        H.pooled = torch.empty_like(H.pooled)
    check_valid(H, "evt_forward_features", lst=one, pooled=True)


def test_wrong_family_and_missing_arguments(handles):
    for fn, families in WRONG_FAMILY.items():
        for family, message in families.items():
            H = handles[family]
            good = dict(blocks=(0,), ptrs=(H.p[0],))
            rejected(H, fn, message, lst=good, logits=True)
            # the family is refused ahead of the list, the outputs and the batch
            rejected(H, fn, message, lst=dict(good, n=65), logits=True)
            rejected(H, fn, message, lst=good, logits=True, batch=0)
            rejected(H, fn, message)
    lib = _lib.load_library()
    V = handles["vit"]
    img, f = _lib.evt_image_args(), _lib.evt_features_args()
    img.data = V.img.data_ptr()
    null = {"evt_forward_attention": "model, image descriptor and attn must be non-null",
            "evt_forward_window_attention": "model, image descriptor and attn must be non-null",
            "evt_forward_head_stats": "model, image descriptor and hs must be non-null",
            "evt_forward_ffn_stats": "model, image descriptor and fs must be non-null",
            "evt_forward_rollout": "model, image descriptor and ro must be non-null"}
    for fn, message in null.items():
        assert getattr(lib, fn)(V.h, ctypes.byref(img), B, None, None, None) == _lib.EVT_EINVAL
        assert lib.evt_last_error().decode() == message
        assert getattr(lib, fn)(V.h, None, 0, ctypes.byref(f), None, None) == _lib.EVT_EINVAL
        assert lib.evt_last_error().decode() == message
    assert lib.evt_forward_token_pruning(V.h, ctypes.byref(img), B, None, None, None) == _lib.EVT_EINVAL
    assert lib.evt_last_error().decode() == "model, image descriptor and feat must be non-null"
    assert lib.evt_forward_features(V.h, P(V.img.data_ptr()), 0, None, None) == _lib.EVT_EINVAL
    assert lib.evt_last_error().decode() == "model, img and args must be non-null"
    assert lib.evt_forward_image(V.h, ctypes.byref(img), 0, None, None) == _lib.EVT_EINVAL
    assert lib.evt_last_error().decode() == "image descriptor, outputs and model must be non-null"
    assert lib.evt_forward_classify(V.h, ctypes.byref(img), 0, ctypes.byref(f), None, None) == _lib.EVT_EINVAL
    assert lib.evt_last_error().decode() == "forward_classify: feat and cls must be non-null"
    # the image descriptor is checked ahead of everything a model adds
    img.data = None
    for fn in null:
        a = LISTS[fn]["struct"][0]() if fn != "evt_forward_rollout" else _lib.evt_rollout_args()
        assert getattr(lib, fn)(V.h, ctypes.byref(img), 0, None, ctypes.byref(a), None) == _lib.EVT_EINVAL
        assert lib.evt_last_error().decode() == "image data is NULL"
    # rollout and token pruning have no block list of their own: feat or the batch, then theirs
    for H in (handles["vit"], handles["t2t"]):
        for batch in (0, B + 1):
            rejected(H, "evt_forward_rollout", BATCH, batch=batch, feat=False)
        check_valid(H, "evt_forward_rollout")
    rejected(V, "evt_forward_token_pruning", NO_SCHEDULE, logits=True, batch=0)
    for H in handles.values():
        for fn in LIST_FNS[H.family]:
            check_valid(H, fn, lst=dict(blocks=(H.blocks - 1,), ptrs=(H.p[1],)))


def test_token_schedule_is_refused_in_order(handles):
    V = handles["vit"]
    good = dict(blocks=(0,), ptrs=(V.p[0],))
    V.m.set_token_pruning({0: 2})
    try:
        pruned = V.m(V.img).clone()
        for fn in ("evt_forward_attention", "evt_forward_head_stats", "evt_forward_ffn_stats",
                   "evt_forward_rollout"):
            rejected(V, fn, fn + SCHEDULE, lst=good, logits=True)
            if fn != "evt_forward_rollout":  # the schedule, then the list, the outputs, the batch
                rejected(V, fn, fn + SCHEDULE, lst=dict(good, n=65))
                rejected(V, fn, fn + SCHEDULE)
            rejected(V, fn, fn + SCHEDULE, lst=good, batch=0)
        for fn in ("evt_forward_features", "evt_forward_image", "evt_forward_classify",
                   "evt_forward_token_pruning"):
            lg = fn == "evt_forward_classify"
            rejected(V, fn, "a block tap" + SCHEDULE, lst=good, logits=True)
            rejected(V, fn, "the final token map (tokens)" + SCHEDULE, lst=good, tokens=True, logits=lg)
            # the count, the outputs and the batch are checked ahead of the schedule
            rejected(V, fn, TAPS["count"], lst=dict(good, n=-1), logits=lg)
            rejected(V, fn, BATCH, lst=good, batch=B + 1, logits=lg)
            # ... and the schedule ahead of the list's entries
            rejected(V, fn, "a block tap" + SCHEDULE, lst=dict(blocks=(9,), ptrs=(V.p[0] + 4,)), logits=lg)
            check_valid(V, fn, want=pruned)  # logits alone: the scheduled forward
        rejected(V, "evt_forward_token_pruning", NO_FEAT)
        rejected(V, "evt_forward_token_pruning", NO_FEAT, batch=0)
    finally:
        V.m.set_token_pruning(None)
    rejected(V, "evt_forward_token_pruning", NO_SCHEDULE, logits=True)
    rejected(V, "evt_forward_token_pruning", NO_SCHEDULE, lst=dict(good, n=65), batch=0)
    for fn in LIST_FNS["vit"]:
        check_valid(V, fn, lst=good)


# ---- the launch sequence ----------------------------------------------------------------------------
ROLES = _lib.PROF_ROLES


def _launches(H, run):
    """{role: event pairs} of the forward `run` enqueues under evt_model_profile."""
    lib = _lib.load_library()
    us, n = (ctypes.c_float * len(ROLES))(), (ctypes.c_int * len(ROLES))()
    _lib.check(lib.evt_model_profile(H.h, 1))
    try:
        run()
        torch.cuda.synchronize()
        _lib.check(lib.evt_model_profile_read(H.h, us, n))
    finally:
        _lib.check(lib.evt_model_profile(H.h, 0))
    return {r: c for r, c in zip(ROLES, n) if c}


def test_launches_of_the_vit_analysis_forwards(handles):
    """StandardViT, depth 2: a plain forward is patchify, the patch embedding, five roles per block
    and the head; every export of a block is one EVT_PROF_HEAD pair more (a rollout step's two
    launches share one, a scheduled block's scores / select / gather are three)."""
    V = handles["vit"]
    m, x, gpu = V.m, V.img, V.img.device
    enc = {"patchify": 1, "patch_embed": 1, "qkv": 2, "attention": 2, "out_proj": 2, "fc1": 2, "fc2": 2}
    new = lambda *shape: torch.empty(shape, device=gpu)  # noqa: E731
    lg = new(B, 8)
    t = m.attn_shape(0)[1]
    assert (t, m.num_blocks) == (5, 2)
    calls = {  # name: (the call of blocks `bl`, exports per block)
        "features": lambda bl: m.features_into(x, logits=lg, taps=bl, tap_tensors=[new(B, 5, 64) for _ in bl]),
        "attention": lambda bl: m.attention_maps_into(x, blocks=bl, logits=lg,
                                                      map_tensors=[new(B, 1, 5) for _ in bl]),
        "head_stats": lambda bl: m.head_stats_into(x, blocks=bl, logits=lg,
                                                   stat_tensors=[new(B, 1, 4) for _ in bl]),
        "ffn_stats": lambda bl: m.ffn_stats_into(x, blocks=bl, logits=lg,
                                                 stat_tensors=[new(B, 128, 4) for _ in bl]),
    }
    assert _launches(V, lambda: m.forward_into(x, lg)) == dict(enc, head=1)
    assert m.tail_mode() == 1
    for name, run in calls.items():
        exports_rows = name in ("features", "ffn_stats")
        assert _launches(V, lambda: run((0, 1))) == dict(enc, head=3), name
        assert m.tail_mode() == (3 if exports_rows else 1), name
        assert torch.equal(lg, V.want), name
        assert _launches(V, lambda: run((0,))) == dict(enc, head=2), name
        assert m.tail_mode() == 1, name
        assert _launches(V, lambda: run((1,))) == dict(enc, head=2), name
        assert m.tail_mode() == (3 if exports_rows else 1), name
    assert _launches(V, lambda: m.features_into(x, logits=lg, tokens=new(B, 5, 64))) == dict(enc, head=2)
    assert m.tail_mode() == 3
    assert _launches(V, lambda: m.attention_rollout_into(x, out=new(B, 5), logits=lg)) == dict(enc, head=3)
    assert m.tail_mode() == 1
    assert _launches(V, lambda: m.attention_rollout_into(x, out=new(B, 5), start=1)) == dict(enc, head=1)
    idx = torch.empty((B, 1), dtype=torch.int32, device=gpu)
    assert _launches(V, lambda: m.classify_into(x, logits=lg, indices=idx, topk=1)) == dict(enc, head=2)
    assert m.tail_mode() == 1
    m.set_token_pruning({0: 2})
    try:
        got = _launches(V, lambda: m.token_pruning_outputs_into(x, logits=lg))
    finally:
        m.set_token_pruning(None)
    assert got == dict(enc, head=4) and m.tail_mode() == 1
    assert _launches(V, lambda: m.forward_into(x, lg)) == dict(enc, head=1)
    assert torch.equal(lg, V.want)


def test_launches_of_the_swin_analysis_forwards(handles):
    """Swin 56 px, depths (2, 2), bf16: the two blocks of stage 1 are the fused attention sublayer
    and the fused MLP, the two of stage 2 the five GEMM-path roles. A window map of a fused block
    is two EVT_PROF_HEAD pairs (the QKV GEMM the fused sublayer does not store, then the map), of
    a GEMM-path block one; a tap is one."""
    S = handles["swin"]
    m, x, gpu = S.m, S.img, S.img.device
    enc = {"patchify": 1, "patch_embed": 1, "attn_sublayer": 2, "mlp": 2, "merge": 1, "qkv": 2,
           "attention": 2, "out_proj": 2, "fc1": 2, "fc2": 2}
    new = lambda *shape: torch.empty(shape, device=gpu)  # noqa: E731
    lg = new(B, 8)
    assert m.num_blocks == 4
    maps = lambda bl: m.window_attention_maps_into(  # noqa: E731
        x, blocks=bl, logits=lg, map_tensors=[new(B, *m.window_attn_shape(i), m.window_attn_shape(i)[2])
                                              for i in bl])
    taps = lambda bl: m.features_into(x, logits=lg, taps=bl,  # noqa: E731
                                      tap_tensors=[new(B, *m.tap_shape(i)) for i in bl])
    assert _launches(S, lambda: m.forward_into(x, lg)) == dict(enc, head=1)
    assert _launches(S, lambda: maps((0, 3))) == dict(enc, head=4)
    assert torch.equal(lg, S.want)
    assert _launches(S, lambda: maps((0,))) == dict(enc, head=3)
    assert _launches(S, lambda: maps((3,))) == dict(enc, head=2)
    assert _launches(S, lambda: maps((3, 0))) == dict(enc, head=4)  # the order given: sorted for the ABI
    assert _launches(S, lambda: taps((0, 3))) == dict(enc, head=3)
    assert torch.equal(lg, S.want) and m.tail_mode() == 0
    assert _launches(S, lambda: m.forward_into(x, lg)) == dict(enc, head=1)
