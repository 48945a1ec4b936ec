"""Device-side operators of the hot path: thin ctypes wrappers over the C ABI (include/hbird_hip.h).

All tensors are CUDA tensors on the current device; work is enqueued on torch's current stream.  torch is
used for memory and streams only -- every arithmetic step below runs in libhbird_hip.so.
"""
from __future__ import annotations

import ctypes

from typing import Optional

import torch

from hbird_mi import _lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("hbird_mi.ops: CUDA tensors required (the HIP path has no CPU fallback)")


def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    """x / ||x|| over the last dim, no eps (reference hbird_eval.py:324, 335)."""
    _need_cuda(x)
    x2 = x.contiguous().float().view(-1, x.shape[-1])
    out = torch.empty_like(x2)
    _lib.check(_lib.lib().hb_normalize_rows(_p(x2), x2.shape[0], x2.shape[1], _p(out), _stream(x2)))
    return out.view(x.shape)


def patch_label_hist(y: torch.Tensor, patch_size: int, num_classes: int, map255: bool = False) -> torch.Tensor:
    """y [B,1,H,W] int64 -> soft labels [B, H/ps, W/ps, C] (reference hbird_eval.py:310, 317-320)."""
    _need_cuda(y)
    if y.dim() != 4 or y.shape[1] != 1:
        raise ValueError(f"expected a [B,1,H,W] mask, got {tuple(y.shape)}")
    y = y.contiguous().to(torch.int64)
    B, _, H, W = y.shape
    out = torch.empty((B, H // patch_size, W // patch_size, num_classes), dtype=torch.float32, device=y.device)
    rc = _lib.lib().hb_patch_label_hist(_p(y), B, H, W, int(patch_size), int(num_classes), int(map255), _p(out), _stream(y))
    if rc != 0 and "out-of-range class" in _lib.last_error():
        raise _lib.HbirdClassRangeError(_lib.last_error())     # F.one_hot raises here (hbird_eval.py:319)
    _lib.check(rc)
    return out


def patch_scores(label: torch.Tensor):
    """label [B, SS, C] -> (scores [B,SS] fp32, nonempty [B,SS] int32, nz_count [B] int32)
    (reference hbird_eval.py:471-493)."""
    _need_cuda(label)
    label = label.contiguous()
    B, SS, C = label.shape
    scores = torch.empty((B, SS), dtype=torch.float32, device=label.device)
    nonempty = torch.empty((B, SS), dtype=torch.int32, device=label.device)
    nz = torch.empty((B,), dtype=torch.int32, device=label.device)
    _lib.check(_lib.lib().hb_patch_scores(_p(label), B, SS, C, _p(scores), _p(nonempty), _p(nz), _stream(label)))
    return scores, nonempty, nz


def patch_select(scores: torch.Tensor, nonempty: torch.Tensor, r: torch.Tensor, r_off: torch.Tensor, K: int,
                 want_scores: bool = False):
    """noise multiply + K smallest per image, ascending (reference hbird_eval.py:497-511)."""
    # the C entry takes bare pointers: a tensor of another dtype would be read as noise, so dtypes and shapes are checked here (and
    # before the device check, so that the refusal does not need a GPU)
    for name, t, dt in (("scores", scores, torch.float32), ("nonempty", nonempty, torch.int32), ("r", r, torch.float32),
                        ("r_off", r_off, torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"patch_select: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
    if scores.dim() != 2 or tuple(nonempty.shape) != tuple(scores.shape):
        raise ValueError(f"patch_select: scores and nonempty must both be [B, SS], got {tuple(scores.shape)} and {tuple(nonempty.shape)}")
    if tuple(r_off.shape) != (scores.shape[0],):
        raise ValueError(f"patch_select: r_off must be [B] = [{scores.shape[0]}], got {tuple(r_off.shape)}")
    if r.dim() != 1:
        raise ValueError(f"patch_select: r must be one-dimensional, got {tuple(r.shape)}")
    _need_cuda(scores, nonempty, r, r_off)
    B, SS = scores.shape
    out = torch.empty((B, K), dtype=torch.int64, device=scores.device)
    osc = torch.empty((B, SS), dtype=torch.float32, device=scores.device) if want_scores else None
    _lib.check(_lib.lib().hb_patch_select(_p(scores.contiguous()), _p(nonempty.contiguous()), _p(r.contiguous()),
                                          _p(r_off.contiguous()), B, SS, int(K), _p(out), _p(osc), _stream(scores)))
    return (out, osc) if want_scores else out


def gather_rows(src: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """src [R, W] fp32, ids [n] int64 -> [n, W]."""
    _need_cuda(src, ids)
    src = src.contiguous()
    ids = ids.contiguous().to(torch.int64).view(-1)
    out = torch.empty((ids.numel(), src.shape[1]), dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().hb_gather_rows(_p(src), src.shape[0], src.shape[1], _p(ids), ids.numel(), _p(out),
                                         _stream(src)))
    return out


def upsample_argmax(label_hat: torch.Tensor, S: int, h: int, w: int) -> torch.Tensor:
    """label_hat [B, S*S, C] -> hard prediction [B,1,h,w] int64 (reference hbird_eval.py:235-243)."""
    _need_cuda(label_hat)
    label_hat = label_hat.contiguous().float()
    B, N, C = label_hat.shape
    if N != S * S:
        raise ValueError(f"label_hat has {N} patches, expected {S}x{S}")
    out = torch.empty((B, 1, h, w), dtype=torch.int64, device=label_hat.device)
    _lib.check(_lib.lib().hb_upsample_argmax(_p(label_hat), B, int(S), C, int(h), int(w), _p(out),
                                             _stream(label_hat)))
    return out


def upsample_argmax_confusion(label_hat: torch.Tensor, S: int, gt: torch.Tensor, conf: torch.Tensor, ignore_index,
                              want_map: bool = False) -> Optional[torch.Tensor]:
    """K6 + K7 fused: label_hat [B, S*S, C] upsampled to gt's [B,1,h,w], its argmax counted into conf [G,P] int64 against gt
    (reference hbird_eval.py:235-243 + eval_metrics.py:73-104).  The class map is only materialised when `want_map`."""
    _need_cuda(label_hat, gt, conf)
    label_hat = label_hat.contiguous().float()
    gt = gt.contiguous().to(torch.int64)
    B, N, C = label_hat.shape
    if N != S * S:
        raise ValueError(f"label_hat has {N} patches, expected {S}x{S}")
    if gt.dim() != 4 or gt.shape[0] != B or gt.shape[1] != 1:
        raise ValueError(f"gt must be [B,1,h,w] with B = {B}, got {tuple(gt.shape)}")
    h, w = int(gt.shape[2]), int(gt.shape[3])
    G, P = conf.shape
    has = ignore_index is not None
    out = torch.empty((B, 1, h, w), dtype=torch.int64, device=label_hat.device) if want_map else None
    _lib.check(_lib.lib().hb_upsample_argmax_confusion(_p(label_hat), B, int(S), C, h, w, _p(gt), G, P, int(ignore_index) if has else 0,
                                                       int(has), _p(conf), _p(out) if want_map else None, _stream(label_hat)))
    return out


def upsample_accumulate(label_hat: torch.Tensor, S: int, acc: torch.Tensor, y0: int, x0: int, win_h: int,
                        win_w: int) -> None:
    """Sliding windows: acc[B,H,W,C] (fp32, channels last) += bilinear upsample of one window's label_hat
    [B, S*S, C] to win_h x win_w, placed at (y0, x0) (the per-image upsample of hbird_eval.py:235-240)."""
    _need_cuda(label_hat)
    _need_cuda(acc)
    label_hat = label_hat.contiguous().float()
    B, N, C = label_hat.shape
    if N != S * S:
        raise ValueError(f"label_hat has {N} patches, expected {S}x{S}")
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.dim() != 4 or acc.shape[0] != B or acc.shape[3] != C:
        raise ValueError("acc must be a contiguous float32 [B, H, W, C] tensor matching label_hat")
    _lib.check(_lib.lib().hb_upsample_accumulate(_p(label_hat), B, int(S), C, int(win_h), int(win_w), _p(acc),
                                                 acc.shape[1], acc.shape[2], int(y0), int(x0), _stream(label_hat)))


def argmax_channels(acc: torch.Tensor) -> torch.Tensor:
    """acc [B,H,W,C] float32 -> [B,1,H,W] int64 class map (first maximum wins, hbird_eval.py:243)."""
    _need_cuda(acc)
    acc = acc.contiguous().float()
    B, H, W, C = acc.shape
    out = torch.empty((B, 1, H, W), dtype=torch.int64, device=acc.device)
    _lib.check(_lib.lib().hb_argmax_channels(_p(acc), B * H * W, C, _p(out), _stream(acc)))
    return out


def confusion_update(conf: torch.Tensor, gt: torch.Tensor, pred: torch.Tensor, ignore_index) -> None:
    """conf [G,P] int64 (CUDA) += confusion counts (reference eval_metrics.py:73-104)."""
    _need_cuda(conf, gt, pred)
    gt = gt.contiguous().to(torch.int64).view(-1)
    pred = pred.contiguous().to(torch.int64).view(-1)
    if gt.numel() != pred.numel():
        raise ValueError("gt and pred must have the same number of elements")
    G, P = conf.shape
    has = ignore_index is not None
    _lib.check(_lib.lib().hb_confusion_update(_p(gt), _p(pred), gt.numel(), G, P, int(ignore_index) if has else 0,
                                              int(has), _p(conf), _stream(conf)))


# ---- paired bootstrap over images (include/hbird_hip_bootstrap.h, csrc/hbird_bootstrap.hip) ---------------------------------------------
def image_class_counts(gt: torch.Tensor, pred: torch.Tensor, num_classes: int, ignore_index, out: Optional[torch.Tensor] = None,
                       row_stride: Optional[int] = None) -> torch.Tensor:
    """gt, pred [B,1,h,w] int64 -> per-image (tp, fp, fn) under the identity matching, int32 [B, G, 3].
    With `out` (a contiguous int32 CUDA tensor) image b's [G][3] block is written at out.view(-1)[b * row_stride:] and nothing else is
    touched: the blocks of one configuration inside an image-major table."""
    _need_cuda(gt, pred, out)
    if gt.shape != pred.shape or gt.dim() != 4 or gt.shape[1] != 1:
        raise ValueError(f"gt and pred must both be [B,1,h,w], got {tuple(gt.shape)} and {tuple(pred.shape)}")
    gt = gt.contiguous().to(torch.int64)
    pred = pred.contiguous().to(torch.int64)
    B, _, h, w = gt.shape
    G = int(num_classes)
    if out is None:
        out = torch.empty((B, G, 3), dtype=torch.int32, device=gt.device)
        row_stride = 3 * G
    else:
        if out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 tensor")
        if row_stride is None:
            raise ValueError("row_stride is required with out")
        if B and (int(row_stride) < 3 * G or (B - 1) * int(row_stride) + 3 * G > out.numel()):
            raise ValueError("out is too small for B blocks of 3 G counts at this row_stride")
    has = ignore_index is not None
    _lib.check(_lib.lib().hb_image_class_counts(_p(gt), _p(pred), B, int(h), int(w), G, int(ignore_index) if has else 0, int(has), _p(out),
                                                int(row_stride), _stream(gt)))
    return out


def bootstrap_multiplicities(n_img: int, seed: int, R: int, r0: int = 0, device=None) -> torch.Tensor:
    """Rows r0 .. r0 + R - 1 of the resampler's multiplicities W, int32 [R, n_img]: W[r][i] = #{j : draw(seed, r, j) == i}."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("hbird_mi.ops: CUDA tensors required (the HIP path has no CPU fallback)")
    out = torch.empty((max(int(R), 0), max(int(n_img), 0)), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().hb_bootstrap_multiplicities(int(n_img), int(seed) & 0xFFFFFFFFFFFFFFFF, int(r0), int(R), _p(out), _stream(out)))
    return out


def bootstrap_counts(stats: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """stats [n_img, cols] int32, W [R, n_img] int32 -> W @ stats in int64 [R, cols], exact."""
    _need_cuda(stats, W)
    if stats.dtype != torch.int32 or W.dtype != torch.int32 or stats.dim() != 2 or W.dim() != 2 or W.shape[1] != stats.shape[0]:
        raise ValueError("bootstrap_counts: stats [n_img, cols] and W [R, n_img] must be int32 with matching n_img")
    stats, W = stats.contiguous(), W.contiguous()
    out = torch.empty((W.shape[0], stats.shape[1]), dtype=torch.int64, device=stats.device)
    _lib.check(_lib.lib().hb_bootstrap_counts(_p(stats), stats.shape[0], stats.shape[1], _p(W), W.shape[0], _p(out), _stream(stats)))
    return out


def bootstrap_miou(stats: torch.Tensor, n_cfg: int, num_classes: int, seed: int, R: int, _chunk_replicates: int = 0):
    """stats [n_img, n_cfg * 3 G] int32 -> (point float64 [n_cfg], samples float64 [R, n_cfg]): the identity-matching mIoU of every
    configuration on all images and on R paired bootstrap replicates.  `_chunk_replicates` (tests): replicates per pass, 0 = automatic."""
    _need_cuda(stats)
    G, n_cfg = int(num_classes), int(n_cfg)
    if stats.dtype != torch.int32 or stats.dim() != 2 or stats.shape[1] != n_cfg * 3 * G:
        raise ValueError(f"bootstrap_miou: stats must be int32 [n_img, {n_cfg * 3 * G}], got {stats.dtype} {tuple(stats.shape)}")
    stats = stats.contiguous()
    point = torch.empty((n_cfg,), dtype=torch.float64, device=stats.device)
    samples = torch.empty((int(R), n_cfg), dtype=torch.float64, device=stats.device)
    _lib.check(_lib.lib().hb_bootstrap_miou(_p(stats), stats.shape[0], n_cfg, G, int(seed) & 0xFFFFFFFFFFFFFFFF, int(R), _p(point), _p(samples),
                                            int(_chunk_replicates), _stream(stats)))
    return point, samples


# ---- depth estimation by retrieval (include/hbird_hip_depth.h, csrc/hbird_depth.hip) -----------------------------------------------------
def patch_depth_targets(y: torch.Tensor, patch_size: int, target_grid: int = 1, min_depth: float = 1e-3, max_depth: float = 10.0):
    """y [B,H,W] fp32 metres -> (rows [B, H/ps, W/ps, 2 r^2] fp32: per-cell sums of valid depth and valid shares, both over the cell's area;
    nonempty [B, H/ps, W/ps] int32: the patch holds a valid pixel)."""
    if not isinstance(y, torch.Tensor) or y.dim() != 3 or y.dtype != torch.float32:
        raise ValueError(f"patch_depth_targets: y must be a float32 [B,H,W] tensor, got {getattr(y, 'dtype', type(y))} {tuple(getattr(y, 'shape', ()))}")
    B, H, W = y.shape
    ps, r = int(patch_size), int(target_grid)
    if ps < 1 or r < 1 or H % ps or W % ps or ps % r:
        raise ValueError(f"patch_depth_targets: patch_size={patch_size} must divide H={H} and W={W}, and target_grid={target_grid} the patch size")
    _need_cuda(y)
    y = y.contiguous()
    rows = torch.empty((B, H // ps, W // ps, 2 * r * r), dtype=torch.float32, device=y.device)
    nonempty = torch.empty((B, H // ps, W // ps), dtype=torch.int32, device=y.device)
    _lib.check(_lib.lib().hb_patch_depth_targets(_p(y), B, H, W, ps, r, float(min_depth), float(max_depth), _p(rows), _p(nonempty), _stream(y)))
    return rows, nonempty


def depth_upsample_metrics(agg: torch.Tensor, S: int, target_grid: int, gt: torch.Tensor, min_depth: float = 1e-3, max_depth: float = 10.0,
                           want_map: bool = False):
    """agg [B, S*S, 2 r^2] (the aggregated rows) against gt [B,h,w] fp32 -> (sums [B, DEPTH_NSUMS] float64 in the order of _lib.DEPTH_SUMS,
    pred [B,h,w] fp32 with NaN where there is no prediction -- or None unless `want_map`).  Synchronises the current stream."""
    _need_cuda(agg, gt)
    r = int(target_grid)
    if agg.dim() != 3 or agg.dtype != torch.float32 or agg.shape[1] != S * S or agg.shape[2] != 2 * r * r:
        raise ValueError(f"depth_upsample_metrics: agg must be float32 [B, {S * S}, {2 * r * r}], got {agg.dtype} {tuple(agg.shape)}")
    if gt.dim() != 3 or gt.dtype != torch.float32 or gt.shape[0] != agg.shape[0]:
        raise ValueError(f"depth_upsample_metrics: gt must be float32 [B,h,w] with B = {agg.shape[0]}, got {gt.dtype} {tuple(gt.shape)}")
    agg, gt = agg.contiguous(), gt.contiguous()
    B, h, w = gt.shape
    sums = torch.empty((B, _lib.DEPTH_NSUMS), dtype=torch.float64, device=agg.device)
    pred = torch.empty((B, h, w), dtype=torch.float32, device=agg.device) if want_map else None
    _lib.check(_lib.lib().hb_depth_upsample_metrics(_p(agg), B, int(S), r, h, w, _p(gt), float(min_depth), float(max_depth), _p(sums), _p(pred),
                                                    _stream(agg)))
    return sums, pred


# ---- depth grids (include/hbird_hip_depth_grid.h, csrc/hbird_depth_grid.hip) ------------------------------------------------------------------
def depth_upsample_metrics_grid(agg: torch.Tensor, S: int, target_grid: int, gt: torch.Tensor, min_depth: float = 1e-3, max_depth: float = 10.0,
                                want_map: bool = False):
    """agg [n_cfg, B, S*S, 2 r^2] (what `search_aggregate_grid` returns on a depth bank, viewed per image) against gt [B,h,w] fp32 ->
    (sums [n_cfg, B, DEPTH_NSUMS] float64, pred [n_cfg, B, h, w] fp32 -- or None unless `want_map`): slab c has the bits of
    `depth_upsample_metrics(agg[c], ...)`.  More than DEPTH_GRID_MAX_CONFIGS configurations go through in chunks of that many.
    Synchronises the current stream."""
    _need_cuda(agg, gt)
    r = int(target_grid)
    if agg.dim() != 4 or agg.dtype != torch.float32 or agg.shape[0] < 1 or agg.shape[2] != S * S or agg.shape[3] != 2 * r * r:
        raise ValueError(f"depth_upsample_metrics_grid: agg must be float32 [n_cfg >= 1, B, {S * S}, {2 * r * r}], got {agg.dtype} {tuple(agg.shape)}")
    if gt.dim() != 3 or gt.dtype != torch.float32 or gt.shape[0] != agg.shape[1]:
        raise ValueError(f"depth_upsample_metrics_grid: gt must be float32 [B,h,w] with B = {agg.shape[1]}, got {gt.dtype} {tuple(gt.shape)}")
    agg, gt = agg.contiguous(), gt.contiguous()
    n_cfg, (B, h, w) = agg.shape[0], gt.shape
    sums = torch.empty((n_cfg, B, _lib.DEPTH_NSUMS), dtype=torch.float64, device=agg.device)
    pred = torch.empty((n_cfg, B, h, w), dtype=torch.float32, device=agg.device) if want_map else None
    for c0 in range(0, n_cfg, _lib.DEPTH_GRID_MAX_CONFIGS):
        c1 = min(n_cfg, c0 + _lib.DEPTH_GRID_MAX_CONFIGS)
        _lib.check(_lib.lib().hb_depth_upsample_metrics_grid(_p(agg[c0:c1]), c1 - c0, B, int(S), r, h, w, _p(gt), float(min_depth), float(max_depth),
                                                             _p(sums[c0:c1]), _p(pred[c0:c1]) if want_map else None, _stream(agg)))
    return sums, pred


def bootstrap_weighted_sums(table: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """table [n_img, cols] float64, W [R, n_img] int32 (rows of `bootstrap_multiplicities`) -> out [R, cols] float64 with
    out[r][col] = the chain acc = 0.0; for i ascending: acc = acc + (double)W[r][i] * table[i][col] -- the same bits however R is cut."""
    _need_cuda(table, W)
    if table.dtype != torch.float64 or W.dtype != torch.int32 or table.dim() != 2 or W.dim() != 2 or W.shape[1] != table.shape[0]:
        raise ValueError("bootstrap_weighted_sums: table [n_img, cols] must be float64 and W [R, n_img] int32 with matching n_img")
    table, W = table.contiguous(), W.contiguous()
    out = torch.empty((W.shape[0], table.shape[1]), dtype=torch.float64, device=table.device)
    _lib.check(_lib.lib().hb_bootstrap_weighted_sums(_p(table), table.shape[0], table.shape[1], _p(W), W.shape[0], _p(out), _stream(table)))
    return out


# ---- video label propagation (include/hbird_hip_propagate.h, csrc/hbird_propagate.hip, csrc/hbird_maskmetrics.hip) ----------------------------
def propagate_labels(q: torch.Tensor, feat_pool: torch.Tensor, label_pool: torch.Tensor, slots, radii, grid, k: int = 5, temperature: float = 0.1,
                     want_neighbours: bool = False):
    """q [N, d] (the target frame's normalised tokens, N = gh * gw row-major) against the context frames `slots` of feat_pool [P, N, d] /
    label_pool [P, N, c], context position f restricted to the square window of radius radii[f] around the query's cell (< 0: unrestricted)
    -> labels [N, c] fp32: the softmax(score / temperature)-weighted sum of the k best candidates' label rows.  With `want_neighbours` also
    (idx [N, k] int64 with id = f * N + cell and -1 past the candidates, score [N, k] fp32 with -inf there)."""
    for name, t in (("q", q), ("feat_pool", feat_pool), ("label_pool", label_pool)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"propagate_labels: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    gh, gw = (int(g) for g in grid)
    N = gh * gw
    if q.dim() != 2 or q.shape[0] != N:
        raise ValueError(f"propagate_labels: q must be [gh * gw, d] = [{N}, d], got {tuple(q.shape)}")
    d = q.shape[1]
    if feat_pool.dim() != 3 or tuple(feat_pool.shape[1:]) != (N, d):
        raise ValueError(f"propagate_labels: feat_pool must be [slots, {N}, {d}], got {tuple(feat_pool.shape)}")
    if label_pool.dim() != 3 or tuple(label_pool.shape[:2]) != (feat_pool.shape[0], N):
        raise ValueError(f"propagate_labels: label_pool must be [{feat_pool.shape[0]}, {N}, c], got {tuple(label_pool.shape)}")
    slots, radii = [int(s) for s in slots], [int(r) for r in radii]
    if len(slots) != len(radii) or not slots:
        raise ValueError(f"propagate_labels: slots and radii must be non-empty and of one length, got {len(slots)} and {len(radii)}")
    if q.device != feat_pool.device or q.device != label_pool.device:
        raise ValueError("propagate_labels: q, feat_pool and label_pool must be on one device")
    _need_cuda(q, feat_pool, label_pool)
    q, feat_pool, label_pool = q.contiguous(), feat_pool.contiguous(), label_pool.contiguous()
    c, n_ctx = label_pool.shape[2], len(slots)
    out = torch.empty((N, c), dtype=torch.float32, device=q.device)
    idx = torch.empty((N, int(k)), dtype=torch.int64, device=q.device) if want_neighbours else None
    score = torch.empty((N, int(k)), dtype=torch.float32, device=q.device) if want_neighbours else None
    IntArr = ctypes.c_int * n_ctx
    _lib.check(_lib.lib().hb_propagate_labels(_p(q), _p(feat_pool), _p(label_pool), feat_pool.shape[0], IntArr(*slots), IntArr(*radii), n_ctx, gh, gw,
                                              d, c, int(k), float(temperature), _p(out), _p(idx), _p(score), _stream(q)))
    return (out, idx, score) if want_neighbours else out


def mask_upsample_argmax(labels: torch.Tensor, grid, h: int, w: int, channel_norm: bool = True) -> torch.Tensor:
    """labels [B, gh * gw, c] fp32 -> the label map [B, h, w] int64: bilinear upsampling (align_corners=False, K6's four taps), with
    `channel_norm` every (image, channel) rescaled to [0, 1] by its own extrema over the frame (DINO's norm_mask), argmax with the first
    maximum winning.  The channel-norm form synchronises the current stream."""
    gh, gw = (int(g) for g in grid)
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.float32 or labels.dim() != 3 or labels.shape[1] != gh * gw:
        raise ValueError(f"mask_upsample_argmax: labels must be float32 [B, {gh * gw}, c], got {getattr(labels, 'dtype', type(labels))} "
                         f"{tuple(getattr(labels, 'shape', ()))}")
    _need_cuda(labels)
    labels = labels.contiguous()
    B, _, c = labels.shape
    out = torch.empty((B, int(h), int(w)), dtype=torch.int64, device=labels.device)
    _lib.check(_lib.lib().hb_mask_upsample_argmax(_p(labels), B, gh, gw, c, int(h), int(w), int(bool(channel_norm)), _p(out), _stream(labels)))
    return out


def mask_jf_counts(pred: torch.Tensor, gt: torch.Tensor, n_objects: int, bound_px: int) -> torch.Tensor:
    """pred, gt [B, h, w] int64 -> counts [B, n_objects, 6] int64 in the order of _lib.JF_COUNTS, for the objects 1 .. n_objects: region
    intersection and union, the sizes of both boundary maps, and each map's pixels within bound_px (a disk) of the other."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 3:
            raise ValueError(f"mask_jf_counts: {name} must be an int64 [B,h,w] tensor, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if tuple(pred.shape) != tuple(gt.shape) or pred.device != gt.device:
        raise ValueError(f"mask_jf_counts: pred and gt must have one shape and device, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    _need_cuda(pred, gt)
    pred, gt = pred.contiguous(), gt.contiguous()
    B, h, w = pred.shape
    counts = torch.empty((B, int(n_objects), len(_lib.JF_COUNTS)), dtype=torch.int64, device=pred.device)
    _lib.check(_lib.lib().hb_mask_jf_counts(_p(pred), _p(gt), B, h, w, int(n_objects), int(bound_px), _p(counts), _stream(pred)))
    return counts


# ---- image-level k-NN classification (include/hbird_hip_vote.h, csrc/hbird_vote.hip) ---------------------------------------------------------
def _vote_grid(who: str, ks, temps):
    ks, temps = [int(k) for k in ks], [float(t) for t in temps]
    if not ks or not temps:
        raise ValueError(f"{who}: ks and temps must not be empty")
    return ks, temps


def knn_vote(idx: torch.Tensor, score: torch.Tensor, labels: torch.Tensor, C: int, ks, temps, topn: int = 5, id_base: int = 0,
             want_votes: bool = False):
    """The weighted vote of a (k, T) grid over one neighbour list per query: idx [nq, k_list] int64 / score [nq, k_list] fp32 as `search`
    leaves them on an inner-product index (best first, -1 / -inf padding), labels [n_rows] int32 (one class in [0, C) per bank row, -1 =
    unlabelled).  Configuration (k, T) votes over the first k list positions with weights exp(score / T); `ks` strictly ascending.
    -> pred [len(ks) * len(temps), nq, topn] int32 (configuration ik * len(temps) + it; classes by descending vote, ties to the lower class,
    -1 past the classes present) -- and with `want_votes` the votes [.., topn] fp32 beside it."""
    for name, t, dt in (("idx", idx, torch.int64), ("score", score, torch.float32), ("labels", labels, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"knn_vote: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
    if idx.dim() != 2 or tuple(idx.shape) != tuple(score.shape) or labels.dim() != 1:
        raise ValueError(f"knn_vote: idx and score must be [nq, k_list] alike and labels [n_rows], got {tuple(idx.shape)}, {tuple(score.shape)}, "
                         f"{tuple(labels.shape)}")
    if idx.device != score.device or idx.device != labels.device:
        raise ValueError("knn_vote: idx, score and labels must be on one device")
    ks, temps = _vote_grid("knn_vote", ks, temps)
    _need_cuda(idx, score, labels)
    idx, score, labels = idx.contiguous(), score.contiguous(), labels.contiguous()
    nq, k_list = idx.shape
    n_cfg = len(ks) * len(temps)
    pred = torch.empty((n_cfg, nq, int(topn)), dtype=torch.int32, device=idx.device)
    votes = torch.empty((n_cfg, nq, int(topn)), dtype=torch.float32, device=idx.device) if want_votes else None
    if nq == 0:                                               # an empty call (an empty tensor has no address to hand over)
        return (pred, votes) if want_votes else pred
    _lib.check(_lib.lib().hb_knn_vote(_p(idx), _p(score), nq, k_list, int(id_base), _p(labels), labels.shape[0], int(C),
                                      (ctypes.c_int * len(ks))(*ks), len(ks), (ctypes.c_float * len(temps))(*temps), len(temps), int(topn),
                                      _p(pred), _p(votes), _stream(idx)))
    return (pred, votes) if want_votes else pred


def vote_counts(pred: torch.Tensor, qlabels: torch.Tensor, C: int, counts: torch.Tensor, n: torch.Tensor,
                class_counts: Optional[torch.Tensor] = None) -> None:
    """ADDS a batch to the count tables: pred [n_cfg, nq, topn] int32 (`knn_vote`), qlabels [nq] int32 (-1: counted nowhere) ->
    counts [n_cfg, topn] int64 (slot t += 1 where the label is among pred[..., :t + 1]), n [1] int64 += the labelled queries, and where given
    class_counts [n_cfg, C, 2] int64 ([c][0] += 1 per labelled query of class c, [c][1] += 1 where its first prediction is c).  A query label
    outside [-1, C) raises ValueError before anything is counted (a flag read: the call synchronises the stream)."""
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.int32 or pred.dim() != 3:
        raise ValueError(f"vote_counts: pred must be an int32 [n_cfg, nq, topn] tensor, got {getattr(pred, 'dtype', type(pred))} {tuple(getattr(pred, 'shape', ()))}")
    n_cfg, nq, topn = pred.shape
    if not isinstance(qlabels, torch.Tensor) or qlabels.dtype != torch.int32 or tuple(qlabels.shape) != (nq,):
        raise ValueError(f"vote_counts: qlabels must be an int32 [{nq}] tensor, got {getattr(qlabels, 'dtype', type(qlabels))} {tuple(getattr(qlabels, 'shape', ()))}")
    for name, t, shape in (("counts", counts, (n_cfg, topn)), ("n", n, (1,)), ("class_counts", class_counts, (n_cfg, int(C), 2))):
        if t is None and name == "class_counts":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"vote_counts: {name} must be a contiguous int64 {list(shape)} tensor, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
        if t.device != pred.device:
            raise ValueError(f"vote_counts: {name} must be on the device of pred")
    if qlabels.device != pred.device:
        raise ValueError("vote_counts: qlabels must be on the device of pred")
    _need_cuda(pred, qlabels, counts, n, class_counts)
    pred, qlabels = pred.contiguous(), qlabels.contiguous()
    if nq == 0:
        return
    _lib.check(_lib.lib().hb_vote_counts(_p(pred), _p(qlabels), nq, n_cfg, topn, int(C), _p(counts), _p(class_counts), _p(n), _stream(pred)),
               ValueError)


def logits_topn(logits: torch.Tensor, topn: int = 5) -> torch.Tensor:
    """hb_logits_topn: logits [nq, C] fp32 -> pred [nq, topn] int32 -- the classes by descending logit, ties to the lower class id; a NaN
    logit ranks below every number and is never written; the tail holds -1 where C < topn or fewer than topn logits are numbers.  The form
    `vote_counts` takes is pred[None]."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError(f"logits_topn: logits must be a float32 [nq, C] tensor, got {getattr(logits, 'dtype', type(logits))} "
                         f"{tuple(getattr(logits, 'shape', ()))}")
    if isinstance(topn, bool) or not isinstance(topn, int) or not 1 <= topn <= _lib.VOTE_MAX_TOP:
        raise ValueError(f"logits_topn: topn={topn!r} must be an integer in [1, {_lib.VOTE_MAX_TOP}]")
    nq, C = logits.shape
    if not 1 <= C <= _lib.LINPROBE_CLASS_MAX_C:
        raise ValueError(f"logits_topn: C must be in [1, {_lib.LINPROBE_CLASS_MAX_C}], got {C}")
    _need_cuda(logits)
    logits = logits.contiguous()
    pred = torch.empty((nq, topn), dtype=torch.int32, device=logits.device)
    if nq == 0:                                               # an empty call (an empty tensor has no address to hand over)
        return pred
    _lib.check(_lib.lib().hb_logits_topn(_p(logits), nq, C, topn, _p(pred), _stream(logits)), ValueError)
    return pred
