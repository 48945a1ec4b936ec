"""Video label propagation (include/hbird_hip_propagate.h) restated in plain numpy, and the worlds the tests run it on.  No engine code.

Candidate lists are built per query in ascending id and scored by oracle.knn_chain_f32 on exactly the allowed rows (the chain's bits and the
lower-id tie rule); the aggregation is float64; the upsampling, the channel norm and the argmax step through fp32 as depth_refs.py does; the
boundary maps, the dilation (by shifts) and the six counts are integers.  `variant=` switches ONE definition to a plausible wrong one
(tests/test_propagate_cpu.py holds each to a named check that it must fail):
  "round_window"       a disk dy^2 + dx^2 <= r^2 instead of the square window
  "per_frame_topk"     k neighbours per context frame instead of k over the union
  "tie_high"           equal scores go to the higher id
  "norm_on_grid"       the channel norm on the label grid, before the upsampling
  "bmap_no_edge_rule"  the last row and column of a boundary map treated like the interior of a zero-padded mask
  "square_dilation"    dilation by the square |dy|, |dx| <= bound instead of the disk
"""
import math

import numpy as np

import oracle
from depth_refs import source_index

F32 = np.float32
VARIANTS = ("round_window", "per_frame_topk", "tie_high", "norm_on_grid", "bmap_no_edge_rule", "square_dilation")
COUNTS = ("inter", "union", "nfg", "ngt", "fg_match", "gt_match")       # HB_JF_*


# ---- candidates, lists, aggregation --------------------------------------------------------------------------------------------------------
def candidates(gh, gw, radii, y, x, variant=None):
    """The ids f * N + cell' a query cell (y, x) may retrieve, ascending."""
    N = gh * gw
    yy, xx = np.mgrid[0:gh, 0:gw]
    ids = []
    for f, r in enumerate(radii):
        if r < 0:
            ok = np.ones((gh, gw), dtype=bool)
        elif variant == "round_window":
            ok = (yy - y) ** 2 + (xx - x) ** 2 <= r * r
        else:
            ok = (np.abs(yy - y) <= r) & (np.abs(xx - x) <= r)
        ids.append(f * N + np.flatnonzero(ok.ravel()))
    return np.concatenate(ids).astype(np.int64)


def _topk(qrow, rows, ids, k, tie_high):
    """(ids, scores) of the k best of `rows` (ids ascending): chain scores, ties to the lower id (to the higher one with tie_high)."""
    if tie_high:
        rows, ids = rows[::-1], ids[::-1]
    pos, sc = oracle.knn_chain_f32(qrow[None], np.ascontiguousarray(rows), k)
    pos, sc = pos[0], sc[0]
    out = np.where(pos >= 0, ids[np.maximum(pos, 0)], -1)
    return out.astype(np.int64), sc.astype(F32)


def lists(q, feat_pool, slots, radii, grid, k, variant=None):
    """-> (idx [N, K] int64, score [N, K] fp32), K = k (n_ctx * k for "per_frame_topk"): descending score, -1 / -inf past the candidates."""
    gh, gw = grid
    N = gh * gw
    q = np.asarray(q, dtype=F32)
    feat_pool = np.asarray(feat_pool, dtype=F32)
    ctx = np.concatenate([feat_pool[s] for s in slots], axis=0)          # row id = f * N + cell
    K = k * len(slots) if variant == "per_frame_topk" else k
    idx = np.full((N, K), -1, dtype=np.int64)
    score = np.full((N, K), -np.inf, dtype=F32)
    for i in range(N):
        ids = candidates(gh, gw, radii, i // gw, i % gw, variant)
        if variant == "per_frame_topk":
            got_i, got_s = [], []
            for f in range(len(slots)):
                sub = ids[ids // N == f]
                a, b = _topk(q[i], ctx[sub], sub, k, False)
                got_i.append(a); got_s.append(b)
            a, b = np.concatenate(got_i), np.concatenate(got_s)
            order = np.lexsort((np.where(a < 0, np.iinfo(np.int64).max, a), -b.astype(np.float64)))
            idx[i], score[i] = a[order], b[order]
        else:
            idx[i], score[i] = _topk(q[i], ctx[ids], ids, k, variant == "tie_high")
    return idx, score


def aggregate(idx, score, label_pool, slots, N, temperature):
    """The softmax(score / temperature)-weighted sum of the listed label rows, float64 -> [n, c]; an empty list gives zeros."""
    label_pool = np.asarray(label_pool, dtype=np.float64)
    T = float(F32(temperature))
    out = np.zeros((idx.shape[0], label_pool.shape[2]), dtype=np.float64)
    for i in range(idx.shape[0]):
        keep = idx[i] >= 0
        if not keep.any():
            continue
        logit = score[i][keep].astype(np.float64) / T
        e = np.exp(logit - logit[0])
        w = e / e.sum()
        ids = idx[i][keep]
        rows = np.stack([label_pool[slots[j // N], j % N] for j in ids])
        out[i] = (w[:, None] * rows).sum(0)
    return out


def aggregate_bound(idx, score, label_pool, temperature):
    """Per query: max|label| * U * (2 max|logit| + 2 spread + 2 k + 6), U = 2^-24 (tests/test_propagate_gpu.py derives it)."""
    U = 2.0 ** -24
    T = float(F32(temperature))
    k = idx.shape[1]
    lmax = float(np.abs(np.asarray(label_pool, dtype=np.float64)).max())
    out = np.zeros(idx.shape[0])
    for i in range(idx.shape[0]):
        keep = idx[i] >= 0
        if not keep.any():
            continue
        logit = score[i][keep].astype(np.float64) / T
        out[i] = lmax * U * (2 * np.abs(logit).max() + 2 * (logit.max() - logit.min()) + 2 * k + 6)
    return out


def propagate(q, feat_pool, label_pool, slots, radii, grid, k, temperature, variant=None):
    idx, score = lists(q, feat_pool, slots, radii, grid, k, variant)
    return aggregate(idx, score, label_pool, slots, grid[0] * grid[1], temperature), idx, score


# ---- the label map -------------------------------------------------------------------------------------------------------------------------
def upsample(labels, grid, h, w):
    """labels [B, gh * gw, c] -> [B, c, h, w] fp32: K6's four taps in their order, every operation rounded to fp32."""
    gh, gw = grid
    labels = np.asarray(labels, dtype=F32)
    B, _, c = labels.shape
    g = labels.reshape(B, gh, gw, c).transpose(0, 3, 1, 2)
    y0, y1, ly0, ly1 = source_index(h, gh)
    x0, x1, lx0, lx1 = source_index(w, gw)
    with np.errstate(invalid="ignore", over="ignore"):
        top = ((lx0 * g[:, :, y0][:, :, :, x0]).astype(F32) + (lx1 * g[:, :, y0][:, :, :, x1]).astype(F32)).astype(F32)
        bot = ((lx0 * g[:, :, y1][:, :, :, x0]).astype(F32) + (lx1 * g[:, :, y1][:, :, :, x1]).astype(F32)).astype(F32)
        return ((ly0[:, None] * top).astype(F32) + (ly1[:, None] * bot).astype(F32)).astype(F32)


def channel_norm(v):
    """v [B, c, ...] fp32: (v - mn) / (mx - mn) per (b, channel) where mx > 0 and mx > mn, unchanged elsewhere."""
    v = np.asarray(v, dtype=F32)
    axes = tuple(range(2, v.ndim))
    mn = v.min(axis=axes, keepdims=True)
    mx = v.max(axis=axes, keepdims=True)
    on = (mx > 0) & (mx > mn)
    span = np.where(on, (mx - mn).astype(F32), F32(1))
    return np.where(on, ((v - mn).astype(F32) / span).astype(F32), v).astype(F32)


def label_map(labels, grid, h, w, norm=True, variant=None):
    """-> [B, h, w] int64: the argmax over channels (first maximum wins) of the upsampled, optionally channel-normalised rows."""
    gh, gw = grid
    labels = np.asarray(labels, dtype=F32)
    if norm and variant == "norm_on_grid":
        B, _, c = labels.shape
        g = channel_norm(labels.reshape(B, gh * gw, c).transpose(0, 2, 1))
        return np.argmax(upsample(g.transpose(0, 2, 1), grid, h, w), axis=1).astype(np.int64)
    v = upsample(labels, grid, h, w)
    if norm:
        v = channel_norm(v)
    return np.argmax(v, axis=1).astype(np.int64)


# ---- boundary maps, dilation, counts -------------------------------------------------------------------------------------------------------
def bmap(M, variant=None):
    """The toolkit's seg2bmap at equal size.  M [h, w] bool -> bool."""
    M = np.asarray(M, dtype=bool)
    E = np.zeros_like(M); S = np.zeros_like(M); SE = np.zeros_like(M)
    E[:, :-1] = M[:, 1:]; S[:-1, :] = M[1:, :]; SE[:-1, :-1] = M[1:, 1:]
    if variant == "bmap_no_edge_rule":
        return (M ^ E) | (M ^ S) | (M ^ SE)
    b = (M ^ E) | (M ^ S) | (M ^ SE)
    b[-1, :] = M[-1, :] ^ E[-1, :]
    b[:, -1] = M[:, -1] ^ S[:, -1]
    b[-1, -1] = False
    return b


def dilate(b, R, variant=None):
    """Dilation by the disk dy^2 + dx^2 <= R^2, by shifts."""
    b = np.asarray(b, dtype=bool)
    h, w = b.shape
    out = np.zeros_like(b)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if variant != "square_dilation" and dy * dy + dx * dx > R * R:
                continue
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            if h - abs(dy) <= 0 or w - abs(dx) <= 0:
                continue
            out[yd, xd] |= b[ys, xs]
    return out


def jf_counts(pred, gt, n_objects, R, variant=None):
    """pred, gt [B, h, w] -> [B, n_objects, 6] int64 in the order of COUNTS."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = np.zeros((pred.shape[0], n_objects, 6), dtype=np.int64)
    for b in range(pred.shape[0]):
        for o in range(1, n_objects + 1):
            P, G = pred[b] == o, gt[b] == o
            bp, bg = bmap(P, variant), bmap(G, variant)
            out[b, o - 1] = ((P & G).sum(), (P | G).sum(), bp.sum(), bg.sum(), (bp & dilate(bg, R, variant)).sum(), (bg & dilate(bp, R, variant)).sum())
    return out


# ---- host metrics --------------------------------------------------------------------------------------------------------------------------
def bound_px(h, w):
    return int(math.ceil(0.008 * math.hypot(h, w)))


def jf_from_counts(counts):
    """counts [..., 6] -> (J, F) float64 with the toolkit's empty cases."""
    c = np.asarray(counts, dtype=np.float64)
    inter, union, nfg, ngt, fgm, gtm = (c[..., i] for i in range(6))
    J = np.where(union == 0, 1.0, inter / np.maximum(union, 1))
    p = np.where(nfg > 0, fgm / np.maximum(nfg, 1), 1.0)
    r = np.where(ngt > 0, gtm / np.maximum(ngt, 1), 1.0)
    p = np.where((nfg > 0) & (ngt == 0), 0.0, p)
    r = np.where((nfg == 0) & (ngt > 0), 0.0, r)
    F = np.where(p + r == 0, 0.0, 2 * p * r / np.where(p + r == 0, 1.0, p + r))
    return J, F


def video_metrics(per_sequence_counts):
    """{name: counts [T - 2, n_obj, 6]} (frames 1 .. T - 2) -> the five headline figures over all objects of all sequences."""
    Jm, Jr, Fm, Fr = [], [], [], []
    for counts in per_sequence_counts.values():
        J, F = jf_from_counts(counts)
        Jm += list(J.mean(0)); Jr += list((J > 0.5).mean(0)); Fm += list(F.mean(0)); Fr += list((F > 0.5).mean(0))
    out = {"J_mean": float(np.mean(Jm)), "J_recall": float(np.mean(Jr)), "F_mean": float(np.mean(Fm)), "F_recall": float(np.mean(Fr))}
    out["J&F"] = 0.5 * (out["J_mean"] + out["F_mean"])
    return out


def ring_context(t, n_last):
    """Context of frame t >= 1 as (frames, slots): the first frame, then the last min(t - 1, n_last) frames, oldest first; frame u >= 1 lives
    in slot 1 + (u - 1) % n_last."""
    frames = [0] + list(range(max(1, t - n_last), t))
    return frames, [0 if u == 0 else 1 + (u - 1) % n_last for u in frames]


# ---- worlds --------------------------------------------------------------------------------------------------------------------------------
def unit_rows(rng, *shape):
    x = rng.standard_normal(shape).astype(F32)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F32)


def small_world(seed=0, grid=(3, 4), d=8, c=3, pool=3):
    """A committed small world for the variant checks: a pool of frames with soft label rows, one query frame."""
    rng = np.random.default_rng(seed)
    N = grid[0] * grid[1]
    feat = unit_rows(rng, pool, N, d)
    lab = rng.random((pool, N, c)).astype(F32)
    lab /= lab.sum(-1, keepdims=True)
    q = unit_rows(rng, N, d)
    return q, feat, lab.astype(F32)


def blobs(rng, B, h, w, n_objects, n_blobs=6):
    """Random label maps [B, h, w] int64 in 0 .. n_objects: rectangles and disks painted over each other."""
    out = np.zeros((B, h, w), dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for b in range(B):
        for _ in range(n_blobs):
            o = int(rng.integers(1, n_objects + 1))
            cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
            ry, rx = int(rng.integers(2, max(3, h // 3))), int(rng.integers(2, max(3, w // 3)))
            if rng.random() < 0.5:
                out[b][(abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)] = o
            else:
                out[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = o
    return out
