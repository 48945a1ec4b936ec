"""numpy / Python-integer restatements of the bootstrap's definitions (include/hbird_hip_bootstrap.h, DESIGN.md section 4 "Bootstrap
intervals"), written from the definitions and sharing nothing with the kernels.  Each has the wrong variants the CPU tests hold it against."""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
SEED = 20240229          # hbird_mi.bootstrap.DEFAULT_SEED


# ---- per-image class counts -------------------------------------------------------------------------------------------------------------
def image_counts(gt: np.ndarray, pred: np.ndarray, G: int, ignore=None, fp_on_gt: bool = False) -> np.ndarray:
    """gt, pred [B,1,h,w] int64 -> int32 [B, G, 3] = (tp, fp, fn) per image.  `fp_on_gt`: the wrong variant that charges a false positive
    to the ground-truth class."""
    B = gt.shape[0]
    out = np.zeros((B, G, 3), dtype=np.int64)
    for b in range(B):
        g, p = gt[b].reshape(-1), pred[b].reshape(-1)
        ok = (g >= 0) & (g < G) & (p >= 0) & (p < G)
        if ignore is not None:
            ok &= g != ignore
        g, p = g[ok], p[ok]
        hit = g == p
        out[b, :, 0] = np.bincount(g[hit], minlength=G)
        out[b, :, 1] = np.bincount((g if fp_on_gt else p)[~hit], minlength=G)
        out[b, :, 2] = np.bincount(g[~hit], minlength=G)
    return out.astype(np.int32)


def maps(B: int, h: int, w: int, G: int, kind: str, seed: int):
    """(gt, pred) [B,1,h,w] int64 with everything the counting rule has to drop: ignore = 255 pixels, out-of-range gt (G, -3), a negative
    pred and a pred >= G, and image 1 entirely ignored.  kind: 'noise' (every pixel its own pair) or 'blocks' (piecewise constant)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        gt = rng.integers(0, G, size=(B, 1, h, w))
        pred = rng.integers(0, G, size=(B, 1, h, w))
    else:
        by, bx = (h + 7) // 8, (w + 11) // 12
        gt = np.kron(rng.integers(0, G, size=(B, 1, by, bx)), np.ones((8, 12), dtype=np.int64))[:, :, :h, :w]
        pred = np.roll(gt, 3, axis=3).copy()                                    # mostly right, wrong along the region borders
        pred[:, :, ::5, :] = rng.integers(0, G, size=(B, 1, (h + 4) // 5, 1))
    gt, pred = gt.astype(np.int64), pred.astype(np.int64)
    gt[:, :, 0, ::3] = 255
    gt[:, :, 1, ::4] = G
    gt[:, :, 2, ::5] = -3
    pred[:, :, 3, ::2] = -1
    pred[:, :, 4, ::2] = G
    pred[:, :, 5, 1::2] = G + 7
    if B > 1:
        gt[1] = 255
    return np.ascontiguousarray(gt), np.ascontiguousarray(pred)


# ---- the resampler -----------------------------------------------------------------------------------------------------------------------
def splitmix_int(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_int(seed: int, r: int, j: int, N: int) -> int:
    """Python integers only: the definition, one draw at a time."""
    return (splitmix_int((splitmix_int(seed) + (r << 32) + j) & M64) * N) >> 64


def _splitmix_u64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draws(seed: int, r: int, N: int, cfg=None) -> np.ndarray:
    """draw(seed, r, j) for j = 0 .. N - 1 (uint64 arithmetic; N < 2^32: the high word of z * N from 32-bit halves).
    `cfg`: the wrong variant whose draws depend on a configuration index."""
    base = splitmix_int(seed)
    if cfg is not None:
        base = (base + 0x1000000 * cfg) & M64
    with np.errstate(over="ignore"):
        z = _splitmix_u64(np.uint64((base + (r << 32)) & M64) + np.arange(N, dtype=np.uint64))
        n = np.uint64(N)
        return (((z >> np.uint64(32)) * n + (((z & np.uint64(0xFFFFFFFF)) * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def multiplicities(seed: int, r0: int, R: int, N: int, cfg=None) -> np.ndarray:
    return np.stack([np.bincount(draws(seed, r, N, cfg), minlength=N) for r in range(r0, r0 + R)]).astype(np.int32)


# ---- replicate counts and mIoU ------------------------------------------------------------------------------------------------------------
def counts(W: np.ndarray, stats: np.ndarray, acc32: bool = False) -> np.ndarray:
    """W [R, N] @ stats [N, cols] in int64.  `acc32`: the wrong variant with a 32-bit accumulator (wraps)."""
    out = W.astype(np.int64) @ stats.astype(np.int64)
    return out.astype(np.int32).astype(np.int64) if acc32 else out


def miou_rows(cnt: np.ndarray, n_cfg: int, G: int, pairwise: bool = False) -> np.ndarray:
    """cnt int64 [R, n_cfg * 3 G] -> float64 [R, n_cfg]: (sum over g ascending of tp / max(tp + fp + fn, 1e-8)) / G, the sum sequential.
    `pairwise`: the variant with numpy's mean (pairwise summation) -- PredsmIoU._miou_from_counts."""
    c = cnt.reshape(cnt.shape[0], n_cfg, G, 3).astype(np.float64)
    tp, fp, fn = c[..., 0], c[..., 1], c[..., 2]
    iou = tp / np.maximum(tp + fp + fn, 1e-8)
    if pairwise:
        return iou.mean(axis=-1)
    s = np.zeros(iou.shape[:2], dtype=np.float64)
    for g in range(G):
        s = s + iou[..., g]
    return s / np.float64(G)


def stats_table(N: int, n_cfg: int, G: int, seed: int, absent_class=None, pixels: int = 4096) -> np.ndarray:
    """A plausible image-major table int32 [N, n_cfg * 3 G]: per image and configuration a random split of `pixels` into (tp, fp, fn) over
    a few classes.  `absent_class`: that class has no count anywhere."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, pixels // G + 1, size=(N, n_cfg, G, 3)).astype(np.int32)
    t[rng.random((N, 1, G, 1)).repeat(n_cfg, 1).repeat(3, 3) < 0.5] = 0          # most classes are absent from most images
    if absent_class is not None:
        t[:, :, absent_class, :] = 0
    return np.ascontiguousarray(t.reshape(N, n_cfg * 3 * G))
