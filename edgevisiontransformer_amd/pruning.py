"""Pruned-checkpoint ingestion: turn the reference's pruning outputs into `ViT_Pruned` models.

The reference prunes DeiT in two places and benchmarks the result through `ViT_Pruned`'s
layerwise encoding (`modeling/models/vit.py:58-97`, `experiments.py:171-204`), which only carries
head COUNTS and FFN fractions. A real pruned checkpoint also says WHICH heads / neurons survive;
this module maps both reference sources onto exact per-layer shapes and sliced weights:

  * nn_pruning (`deit_pruning/vendor/nn_pruning_v1/nn_pruning/patch_coordinator.py:397-406`
    `parse_layerwise_sparsity`; `inference_model_patcher.py:26-89` `get_pruned_heads`): per-layer
    thresholds "h_{head}_d_{ffn}-h_..." and head selection by the count of non-zero rows of the
    q / k / v blocks of each head (lowest scores pruned, at least one head kept).
  * are_16_heads (`are_16_heads/deit_{tiny,small,base}_head_importance.txt`): a [layers, heads]
    importance table (whitespace separated); heads are kept by importance.

`prune_vit_params` slices a Keras-layout parameter dict (weights.vit_param_shapes) to the kept
heads / FFN neurons (q, k, v columns and out-proj rows of the kept heads in their original order;
fc1 columns / fc2 rows of the kept neurons); `build_pruned_vit` makes the MI355X model with those
exact shapes. Host-only (numpy); the forward runs on the GPU like any ViT_Pruned.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .weights import ViTConfig, vit_config


def parse_layerwise_thresholds(spec: str) -> List[Dict[str, float]]:
    """patch_coordinator.py:397-406: "h_0.5_d_0.3-h_..." -> [{'head': 0.5, 'ffn': 0.3}, ...]."""
    out = []
    for item in spec.split("-"):
        parts = item.split("_")
        out.append({"head": float(parts[1]), "ffn": float(parts[-1])})
    return out


def thresholds_to_encoding(thresholds: Sequence[Dict[str, float]], num_heads: int) -> str:
    """The ViT_Pruned layerwise encoding (vit.py:77-97) with the head counts nn_pruning keeps:
    int(threshold * heads) (inference_model_patcher.py: to_prune = heads - int(thr * heads), at
    least one head kept)."""
    toks = []
    for t in thresholds:
        keep = max(1, int(t["head"] * num_heads))
        toks.append(f"h{keep}-d{t['ffn']}")
    return "layerwise_" + "_".join(toks)


def head_scores_nonzero(qkv_w: np.ndarray, heads: int, head_size: int) -> np.ndarray:
    """inference_model_patcher.py `analyze_head` summed over q, k, v: for each head, how many of
    the three [head_size, D] weight blocks have any non-zero entry (0..3). `qkv_w` is the Keras
    [D, 3 * heads * head_size] kernel, columns (qkv h d)."""
    d = qkv_w.shape[0]
    w = qkv_w.reshape(d, 3, heads, head_size)
    return (w != 0).any(axis=(0, 3)).sum(axis=0).astype(np.int64)


def select_heads_nn_pruning(scores: np.ndarray, threshold: float) -> List[int]:
    """Kept heads as get_pruned_heads computes them: prune the H - int(thr * H) lowest-scoring
    heads (stable ascending sort, torch.sort order for ties), never all of them (head 0 stays)."""
    h = len(scores)
    n_prune = h - int(threshold * h)
    order = np.argsort(scores, kind="stable")
    pruned = set(int(i) for i in order[:n_prune])
    if len(pruned) == h:
        pruned.discard(0)
    return [i for i in range(h) if i not in pruned]


def load_head_importance(path: str) -> np.ndarray:
    """are_16_heads/deit_*_head_importance.txt -> float [layers, heads]."""
    rows = [[float(v) for v in line.split()] for line in open(path) if line.strip()]
    return np.asarray(rows, dtype=np.float64)


def importance_from_head_stats(stats: Sequence[np.ndarray], kind: str = "confidence") -> np.ndarray:
    """The [layers, heads] importance table `heads_from_importance` takes, from per-block head
    statistics: `stats[l]` is a [H, 4] array (`collect_head_stats`) or a [B, H, 4] one (`head_stats`,
    averaged over its images here), `kind` one of HEAD_STATS (modeling/models/head_stats.py). The
    value is the statistic itself: with "confidence" (Voita et al.) a higher value is a more
    important head. ValueError: an unknown `kind`, no blocks, or blocks whose head counts differ (a
    pruned model: a table has one width)."""
    names = ("confidence", "entropy", "distance", "cls_mass")
    if kind not in names:
        raise ValueError(f"kind must be one of {names}, got {kind!r}")
    rows = []
    for l, s in enumerate(stats):
        a = np.asarray(s, dtype=np.float64)
        if a.ndim == 3:
            a = a.mean(axis=0)
        if a.ndim != 2 or a.shape[1] != len(names):
            raise ValueError(f"stats[{l}] must be [H, 4] or [B, H, 4], got {a.shape}")
        rows.append(a[:, names.index(kind)])
    if not rows:
        raise ValueError("no blocks given")
    if len({len(r) for r in rows}) != 1:
        raise ValueError(f"head counts differ between blocks ({[len(r) for r in rows]}): an "
                         "importance table needs the same number of heads in every layer")
    return np.stack(rows)


def importance_from_head_ablation(result: Dict[str, object]) -> np.ndarray:
    """The [layers, heads] importance table `heads_from_importance` takes, from `head_ablation`'s
    result (evaluate.py): base top-1 accuracy minus the top-1 accuracy with that head masked, so
    the head whose removal costs most is the most important (a head whose removal helps is
    negative). ValueError: no rows, or rows whose head counts differ (a pruned model, or a sweep
    of some blocks of one: a table has one width)."""
    rows = [np.asarray(r, dtype=np.float64) for r in result["acc1"]]
    if not rows or any(r.ndim != 1 or r.size < 1 for r in rows):
        raise ValueError("the ablation result has no rows")
    if len({r.size for r in rows}) != 1:
        raise ValueError(f"head counts differ between blocks ({[r.size for r in rows]}): an "
                         "importance table needs the same number of heads in every layer")
    return float(result["base"]["acc1"]) - np.stack(rows)


def gates_from_kept(kept: Sequence[Sequence[int]], n) -> Dict[int, np.ndarray]:
    """Binary gates `{layer: float32 [n_l]}` of per-layer keep-lists (`heads_from_importance`,
    `ffn_keep_from_importance`): 1 for the kept indices, 0 for the rest; `n` is the layers' head /
    neuron count, one int for all or one per layer. What `set_head_gates` / `set_ffn_gates` take:
    masking with them checks a keep-list on the loaded model before `build_pruned_vit` cuts it.
    ValueError: an index outside [0, n_l), a count list of another length."""
    counts = [int(n)] * len(kept) if isinstance(n, (int, np.integer)) else [int(v) for v in n]
    if len(counts) != len(kept):
        raise ValueError("one count per layer")
    out = {}
    for l, (k, c) in enumerate(zip(kept, counts)):
        idx = np.asarray(list(k), dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= c):
            raise ValueError(f"layer {l}: kept indices {list(k)} out of range 0..{c - 1}")
        g = np.zeros(c, dtype=np.float32)
        g[idx] = 1.0
        out[l] = g
    return out


def heads_from_importance(importance: np.ndarray, keep_per_layer: Optional[Sequence[int]] = None,
                          keep_total: Optional[int] = None) -> List[List[int]]:
    """Kept heads per layer, most important first kept: either a per-layer count, or a global
    budget (the are-16-heads iterative scheme: the least important heads of the whole model go
    first; every layer keeps at least one head). Returned indices are sorted."""
    layers, heads = importance.shape
    if keep_per_layer is not None:
        return [sorted(int(i) for i in np.argsort(-importance[l], kind="stable")[:max(1, k)])
                for l, k in enumerate(keep_per_layer)]
    if keep_total is None:
        raise ValueError("give keep_per_layer or keep_total")
    order = np.argsort(importance.reshape(-1), kind="stable")  # least important first
    alive = np.ones((layers, heads), dtype=bool)
    to_remove = layers * heads - keep_total
    for flat in order:
        if to_remove <= 0:
            break
        l, h = divmod(int(flat), heads)
        if alive[l].sum() > 1:
            alive[l, h] = False
            to_remove -= 1
    return [[int(h) for h in np.nonzero(alive[l])[0]] for l in range(layers)]


def ffn_keep_by_norm(params: Dict[str, np.ndarray], layer: int, keep: int) -> List[int]:
    """FFN neurons to keep when only a fraction is known: the `keep` largest by
    ||fc1 column|| * ||fc2 row|| (a magnitude proxy; nn_pruning zeroes whole rows/columns, for
    which this picks exactly the non-zero neurons)."""
    w1, w2 = params[f"l{layer}.fc1_w"], params[f"l{layer}.fc2_w"]
    score = np.linalg.norm(w1, axis=0) * np.linalg.norm(w2, axis=1)
    return sorted(int(i) for i in np.argsort(-score, kind="stable")[:keep])


def ffn_importance_from_stats(stats: Sequence[np.ndarray],
                              params: Optional[Dict[str, np.ndarray]] = None,
                              kind: str = "energy") -> List[np.ndarray]:
    """Per-layer FFN neuron importances (one fp64 [F_l] array per layer; the widths may differ) from
    the activation statistics of every block: `stats[l]` is a [F, 4] array (`collect_ffn_stats`) or
    a [B, F, 4] one (`ffn_stats`: mean, mean_abs and mean_sq are averaged over its images, max_abs
    is their maximum), columns in FFN_STATS order (modeling/models/ffn_stats.py). `kind`:

        "energy"    mean_sq_j * ||params["l{l}.fc2_w"][j, :]||^2: the mean squared norm of what the
                    neuron adds to the block's output
        "mean_abs"  the statistic itself
        "max_abs"   the statistic itself (0: a neuron dead on the whole sample)

    A higher value is a more important neuron. ValueError: an unknown `kind`, no blocks, a
    malformed array, "energy" without `params` or with an FC2 of another width."""
    kinds = ("energy", "mean_abs", "max_abs")
    if kind not in kinds:
        raise ValueError(f"kind must be one of {kinds}, got {kind!r}")
    if kind == "energy" and params is None:
        raise ValueError('kind "energy" needs the parameter dict (the FC2 row norms)')
    out = []
    for l, s in enumerate(stats):
        a = np.asarray(s, dtype=np.float64)
        if a.ndim == 3 and a.shape[0] > 0:
            a = np.concatenate([a[..., :3].mean(axis=0), a[..., 3:].max(axis=0)], axis=-1)
        if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1:
            raise ValueError(f"stats[{l}] must be [F, 4] or [B, F, 4], got {np.shape(s)}")
        if kind == "energy":
            w2 = np.asarray(params[f"l{l}.fc2_w"], dtype=np.float64)
            if w2.ndim != 2 or w2.shape[0] != a.shape[0]:
                raise ValueError(f"layer {l}: fc2_w has {w2.shape[0]} rows, the statistics "
                                 f"{a.shape[0]} neurons")
            out.append(a[:, 2] * (w2 * w2).sum(axis=1))
        else:
            out.append(a[:, 1 if kind == "mean_abs" else 3].copy())
    if not out:
        raise ValueError("no blocks given")
    return out


def ffn_keep_from_importance(importance: Sequence[np.ndarray],
                             keep_per_layer: Optional[Sequence[int]] = None,
                             fraction: Optional[float] = None) -> List[List[int]]:
    """Kept FFN neurons per layer, as sorted index lists ready to be `kept_ffn` of
    `prune_vit_params`: the most important `keep_per_layer[l]` of layer l, or
    int(fraction * F_l) of them (the `d{fraction}` of a prune encoding), at least one per layer
    either way. Ties go to the lower index. Exactly one of the two forms must be given."""
    if (keep_per_layer is None) == (fraction is None):
        raise ValueError("give exactly one of keep_per_layer and fraction")
    layers = [np.asarray(v, dtype=np.float64) for v in importance]
    if not layers or any(v.ndim != 1 or v.size < 1 for v in layers):
        raise ValueError("importance must be a non-empty sequence of non-empty 1-D arrays")
    if any(np.isnan(v).any() for v in layers):
        raise ValueError("importance holds NaN")
    if keep_per_layer is not None:
        counts = [int(k) for k in keep_per_layer]
        if len(counts) != len(layers):
            raise ValueError("one keep count per layer")
        if any(k < 0 or k > v.size for k, v in zip(counts, layers)):
            raise ValueError(f"keep counts {counts} outside 0 .. the layers' widths")
    else:
        if not 0.0 <= fraction <= 1.0:
            raise ValueError(f"fraction must be in [0, 1], got {fraction!r}")
        counts = [int(fraction * v.size) for v in layers]
    return [sorted(int(i) for i in np.argsort(-v, kind="stable")[:max(1, k)])
            for k, v in zip(counts, layers)]


def sublayer_importance_from_stats(means: Sequence[np.ndarray], kind: str = "cosine") -> np.ndarray:
    """The [layers, 2] sublayer importance table (columns: attention, FFN) from the stream
    statistics of every block: `means[l]` is a [2, 4] array (`collect_block_stats`) or a [B, 2, 4]
    one (`block_stats`, averaged over its images here), columns in DEPTH_STATS order. `kind`:

        "cosine"      1 - cosine: how far the sublayer turns the stream (0: it leaves the direction)
        "rel_update"  the statistic itself: the size of the update relative to the stream

    A higher value is a more important sublayer; a skipped sublayer scores 0 either way. ValueError:
    an unknown `kind`, no blocks, a malformed array."""
    if kind not in ("cosine", "rel_update"):
        raise ValueError(f'kind must be "cosine" or "rel_update", got {kind!r}')
    rows = []
    for l, s in enumerate(means):
        a = np.asarray(s, dtype=np.float64)
        if a.ndim == 3 and a.shape[0] > 0:
            a = a.mean(axis=0)
        if a.shape != (2, 4):  # (attention, FFN) x DEPTH_STATS of modeling/models/depth.py
            raise ValueError(f"means[{l}] must be [2, 4] or [B, 2, 4], got {np.shape(s)}")
        rows.append(1.0 - a[:, 0] if kind == "cosine" else a[:, 1].copy())
    if not rows:
        raise ValueError("no blocks given")
    return np.stack(rows)


def importance_from_sublayer_ablation(result: Dict[str, object]) -> np.ndarray:
    """The [rows, 2] sublayer importance table from `sublayer_ablation`'s result (evaluate.py): base
    top-1 accuracy minus the top-1 accuracy with that sublayer skipped; row i is block
    result["blocks"][i]. A sublayer that was skipped already (NaN in the result) scores 0: it can
    be dropped at no further cost. ValueError: no rows, or rows that are not (attention, FFN)."""
    rows = np.asarray(result["acc1"], dtype=np.float64)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] != 2:
        raise ValueError(f"the ablation result must have [blocks, 2] accuracies, got {rows.shape}")
    return np.where(np.isnan(rows), 0.0, float(result["base"]["acc1"]) - rows)


def sublayers_from_importance(importance, drop: int,
                              blocks: Optional[Sequence[int]] = None) -> Dict[int, str]:
    """The `{block: "attn" | "ffn" | "block"}` dict `skip_sublayers` takes: the `drop` least
    important sublayers of a [layers, 2] table (ties go to the earlier block, attention before
    FFN); a block that loses both is "block". Row i is block `blocks[i]` (default: i). ValueError: a
    malformed table, NaN, `drop` outside [0, 2 * layers]."""
    imp = np.asarray(importance, dtype=np.float64)
    if imp.ndim != 2 or imp.shape[1] != 2 or imp.shape[0] < 1:
        raise ValueError(f"importance must be [layers, 2], got {imp.shape}")
    if np.isnan(imp).any():
        raise ValueError("importance holds NaN")
    if isinstance(drop, bool) or not 0 <= int(drop) <= imp.size:
        raise ValueError(f"drop must be in [0, {imp.size}], got {drop!r}")
    idx = list(range(imp.shape[0])) if blocks is None else [int(b) for b in blocks]
    if len(idx) != imp.shape[0]:
        raise ValueError("one block index per row")
    bits: Dict[int, int] = {}
    for flat in np.argsort(imp.reshape(-1), kind="stable")[:int(drop)]:
        l, sub = divmod(int(flat), 2)
        bits[idx[l]] = bits.get(idx[l], 0) | (1 << sub)
    return {b: ("attn", "ffn", "block")[v - 1] for b, v in sorted(bits.items())}


def drop_blocks(params: Dict[str, np.ndarray], cfg: ViTConfig,
                blocks: Sequence[int]) -> Tuple[Dict[str, np.ndarray], ViTConfig]:
    """(params, config) of the shallower model without the layers `blocks` (negative: from the
    last), the remaining layers renumbered l0, l1, ... in their order: what a model with these
    blocks skipped whole (`skip_sublayers({b: "block"})`) is cut to, bitwise. Everything that is not
    a layer's (`l{i}.*`) is the input's own array. ValueError: a block out of range or named twice."""
    import dataclasses
    depth = cfg.depth
    gone = set()
    for b in blocks:
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)):
            raise ValueError(f"blocks must be integers, got {b!r}")
        i = int(b) + depth if b < 0 else int(b)
        if not 0 <= i < depth:
            raise ValueError(f"block {b} is outside the model's {depth} blocks")
        if i in gone:
            raise ValueError(f"block {i} is named twice")
        gone.add(i)
    kept = [i for i in range(depth) if i not in gone]
    new_index = {old: new for new, old in enumerate(kept)}
    out: Dict[str, np.ndarray] = {}
    for name, value in params.items():
        layer, dot, rest = name.partition(".")
        if dot and layer[:1] == "l" and layer[1:].isdigit():
            old = int(layer[1:])
            if old in new_index:
                out[f"l{new_index[old]}.{rest}"] = value
        else:
            out[name] = value
    pick = lambda v: tuple(list(v)[i] for i in kept)  # noqa: E731
    new_cfg = dataclasses.replace(cfg, depth=len(kept), heads=pick(cfg.heads),
                                  head_dim=pick(cfg.head_dim), ffn=pick(cfg.ffn))
    return out, new_cfg


def prune_vit_params(params: Dict[str, np.ndarray], cfg: ViTConfig, kept_heads: List[List[int]],
                     kept_ffn: Optional[List[List[int]]] = None,
                     head_size: int = 64) -> Tuple[Dict[str, np.ndarray], ViTConfig]:
    """Slice an unpruned parameter dict to the kept heads / FFN neurons -> (params, config)."""
    depth = cfg.depth
    if len(kept_heads) != depth or (kept_ffn is not None and len(kept_ffn) != depth):
        raise ValueError("one kept list per layer")
    out = dict(params)
    heads_l, ffn_l = [], []
    for i in range(depth):
        h_all = cfg.heads[i]
        kh = list(kept_heads[i])
        if not kh or min(kh) < 0 or max(kh) >= h_all:
            raise ValueError(f"layer {i}: kept heads {kh} out of range 0..{h_all - 1}")
        d = params[f"l{i}.qkv_w"].shape[0]
        qkv = params[f"l{i}.qkv_w"].reshape(d, 3, h_all, head_size)[:, :, kh, :]
        out[f"l{i}.qkv_w"] = np.ascontiguousarray(qkv.reshape(d, 3 * len(kh) * head_size))
        ow = params[f"l{i}.out_w"].reshape(h_all, head_size, -1)[kh]
        out[f"l{i}.out_w"] = np.ascontiguousarray(ow.reshape(len(kh) * head_size, -1))
        heads_l.append(len(kh))
        if kept_ffn is not None:
            kf = list(kept_ffn[i])
            out[f"l{i}.fc1_w"] = np.ascontiguousarray(params[f"l{i}.fc1_w"][:, kf])
            out[f"l{i}.fc1_b"] = np.ascontiguousarray(params[f"l{i}.fc1_b"][kf])
            out[f"l{i}.fc2_w"] = np.ascontiguousarray(params[f"l{i}.fc2_w"][kf, :])
            ffn_l.append(len(kf))
        else:
            ffn_l.append(cfg.ffn[i])
    new_cfg = vit_config(cfg.dim, depth, max(cfg.heads), cfg.mlp_dim, image_size=cfg.image_size,
                         patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                         head_size=head_size, heads_list=heads_l, ffn_list=ffn_l)
    return out, new_cfg


# Default ridge of reconstruct_linear, relative to the mean eigenvalue of C_SS. The Grams come from
# fp32 sums over R = 10^5 .. 10^6 token rows: their entries carry a relative error of the order of
# sqrt(R) 2^-24 (2e-5 .. 6e-5), and forming C = G / R - mu mu^T cancels part of the leading digits.
# Directions of C_SS whose eigenvalue is below about 1e-4 of the mean are therefore noise, and an
# unregularised solve would divide by them; 1e-4 damps exactly those and changes a well-conditioned
# solve by a relative 1e-4, well under the bf16 rounding (2^-9) of the weights it produces. The
# value follows from that error estimate; it was not tuned on a dataset.
DEFAULT_RIDGE = 1e-4


def _checked_keep(keep, n: int, what: str) -> np.ndarray:
    k = np.asarray(list(keep), dtype=np.int64).reshape(-1)
    if k.size == 0:
        raise ValueError(f"{what}: keep is empty")
    if k.min() < 0 or k.max() >= n:
        raise ValueError(f"{what}: keep has an index outside [0, {n})")
    if np.unique(k).size != k.size:
        raise ValueError(f"{what}: keep has a repeated index")
    return k


def reconstruct_linear(W, b, keep, gram, sums, rows, ridge: float = DEFAULT_RIDGE
                       ) -> Tuple[np.ndarray, np.ndarray]:
    """Least-squares repair of a linear layer y = h W + b (W [F, D], b [D]) whose input is cut to
    the columns `keep` of h, from the second moments of h over a calibration set: `gram` = H^T H
    [F, F], `sums` = the column sums [F], `rows` = the rows of H (`collect_grams`). With

        mu = sums / rows          C = gram / rows - mu mu^T       S = keep

    the weights that minimise E |h W + b - (h_S W'_S + b')|^2 over the calibration rows are

        W'_S = (C_SS + lambda I)^-1 C_S,: W        b' = b + mu^T W - mu_S^T W'_S

    with lambda = ridge * trace(C_SS) / |S| (`ridge` = 0: the plain least-squares solution; the
    default is DEFAULT_RIDGE, see there). Returns (W', b') in fp64, W' full size [F, D] with the
    rows outside `keep` zero, so that `prune_vit_params` slices it like the dense weights. All of
    the dropped columns' mean and of what the kept columns predict of them moves into W'_S and b';
    keep = all returns W and b. Pure numpy fp64: a Cholesky solve, `lstsq` when C_SS + lambda I is
    not positive definite."""
    W = np.asarray(W, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    G = np.asarray(gram, dtype=np.float64)
    sm = np.asarray(sums, dtype=np.float64)
    if W.ndim != 2:
        raise ValueError(f"W must be [F, D], got {W.shape}")
    F, D = W.shape
    if b.shape != (D,):
        raise ValueError(f"b must be [{D}], got {b.shape}")
    if G.shape != (F, F) or sm.shape != (F,):
        raise ValueError(f"gram must be [{F}, {F}] and sums [{F}], got {G.shape} and {sm.shape}")
    if not rows >= 1:
        raise ValueError("rows must be at least 1")
    if ridge < 0:
        raise ValueError("ridge must be non-negative")
    S = _checked_keep(keep, F, "reconstruct_linear")
    if S.size == F and np.array_equal(np.sort(S), np.arange(F)):
        return W.copy(), b.copy()
    mu = sm / float(rows)
    C = G / float(rows) - np.outer(mu, mu)
    css = C[np.ix_(S, S)]
    rhs = C[S, :] @ W
    lam = float(ridge) * float(np.trace(css)) / S.size
    A = css + lam * np.eye(S.size)
    try:
        L = np.linalg.cholesky(A)
        ws = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    except np.linalg.LinAlgError:
        ws = np.linalg.lstsq(A, rhs, rcond=None)[0]
    Wn = np.zeros_like(W)
    Wn[S] = ws
    bn = b + mu @ W - mu[S] @ ws
    return Wn, bn


def _block_grams(grams, depth: int, what: str):
    if not isinstance(grams, dict) or not {"gram", "sum", "rows"} <= set(grams):
        raise ValueError(f"{what} must be the {{'gram', 'sum', 'rows'}} dict of collect_grams")
    if len(grams["gram"]) != depth or len(grams["sum"]) != depth:
        raise ValueError(f"{what} must hold one Gram and one sum per layer ({depth})")
    return grams["gram"], grams["sum"], grams["rows"]


def reconstruct_vit_params(params: Dict[str, np.ndarray], cfg: ViTConfig,
                           kept_heads: Optional[List[List[int]]] = None,
                           kept_ffn: Optional[List[List[int]]] = None, ffn_grams=None,
                           attn_grams=None, ridge: float = DEFAULT_RIDGE) -> Dict[str, np.ndarray]:
    """A copy of the FULL-SIZE parameter dict whose FC2 (`l{i}.fc2_w` / `fc2_b`, for `kept_ffn`)
    and out-projection (`l{i}.out_w` / `out_b`, for `kept_heads`; a kept head is its head_dim rows
    of out_w) are repaired by `reconstruct_linear` for the cut the kept lists describe, from the
    Grams of every block of the unpruned model: `ffn_grams` = collect_grams(model, loader, "ffn"),
    `attn_grams` = collect_grams(model, loader, "attn"). The rows of the dropped neurons / heads
    are zero, so the result feeds `prune_vit_params` / `build_pruned_vit` with the same kept lists
    unchanged. Calibration is one pass on the unpruned model: block i's repair does not see the
    repairs of the blocks before it. Entries keep the dtype of `params`."""
    depth = cfg.depth
    out = {k: np.array(v, copy=True) for k, v in params.items()}
    jobs = []
    if kept_ffn is not None:
        if len(kept_ffn) != depth:
            raise ValueError("one kept list per layer")
        g, s, r = _block_grams(ffn_grams, depth, "ffn_grams")
        jobs += [(f"l{i}.fc2_w", f"l{i}.fc2_b", list(kept_ffn[i]), g[i], s[i], r)
                 for i in range(depth)]
    if kept_heads is not None:
        if len(kept_heads) != depth:
            raise ValueError("one kept list per layer")
        g, s, r = _block_grams(attn_grams, depth, "attn_grams")
        for i in range(depth):
            hd = int(cfg.head_dim[i])
            kh = _checked_keep(kept_heads[i], int(cfg.heads[i]), f"layer {i} heads")
            rows_kept = (kh[:, None] * hd + np.arange(hd)[None, :]).reshape(-1)
            jobs.append((f"l{i}.out_w", f"l{i}.out_b", rows_kept, g[i], s[i], r))
    for wn, bn, keep, g, s, r in jobs:
        w, b = reconstruct_linear(params[wn], params[bn], keep, g, s, r, ridge)
        out[wn] = w.astype(np.asarray(params[wn]).dtype)
        out[bn] = b.astype(np.asarray(params[bn]).dtype)
    return out


def build_pruned_vit(params: Dict[str, np.ndarray], cfg: ViTConfig, kept_heads: List[List[int]],
                     kept_ffn: Optional[List[List[int]]] = None, **kw):
    """The MI355X ViT of a pruned checkpoint (exact per-layer shapes; needs the GPU)."""
    from .modeling.models.vit import ViT
    p, c = prune_vit_params(params, cfg, kept_heads, kept_ffn)
    return ViT(image_size=c.image_size, patch_size=c.patch_size, num_classes=c.num_classes,
               dim=c.dim, depth=c.depth, heads=max(cfg.heads), mlp_dim=c.mlp_dim, weights=p,
               _cfg=c, **kw)
