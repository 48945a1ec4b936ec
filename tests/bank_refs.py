"""Definitions of the bank-build, row-access and merge operations, in numpy (float64 / integers, no GPU).

Every function restates one operation from its definition (SURVEY.md 2.3 and the comments above the kernels), independently of the
kernels' own structure: no chunks, no waves, no prefix counts.  tests/test_bank_paths_gpu.py holds the kernels to these on bits;
tests/test_bank_paths_cpu.py holds these to `oracle` and to each other, and shows that deliberately wrong variants disagree with them
on the committed cases.
"""
from __future__ import annotations

import numpy as np

import oracle

F32 = np.float32
SENTINEL = np.float32(1e6)          # score of an empty patch
SUM_EPS = 2.3e-16                   # two orders of a double sum of D non-negative terms differ by at most D * 2.3e-16 (relative)


class ClassRange(ValueError):
    """A mask holds a class outside [0, C) (after the optional 255 -> 0)."""


# ---------------------------------------------------------------- K2

def label_counts(y, ps: int, C: int, map255: bool = False) -> np.ndarray:
    """Integer class counts per patch: y [B,1,H,W] or [B,H,W] int64 -> [B, H/ps, W/ps, C] int64."""
    y = np.asarray(y, dtype=np.int64)
    if y.ndim == 4:
        assert y.shape[1] == 1
        y = y[:, 0]
    B, H, W = y.shape
    if ps <= 0 or H % ps or W % ps:
        raise ValueError("H and W must be multiples of the patch size")
    if map255:
        y = np.where(y == 255, 0, y)
    if ((y < 0) | (y >= C)).any():
        raise ClassRange(f"class outside [0, {C})")
    Sh, Sw = H // ps, W // ps
    pix = y.reshape(B, Sh, ps, Sw, ps).transpose(0, 1, 3, 2, 4).reshape(B * Sh * Sw, ps * ps)
    counts = np.zeros((B * Sh * Sw, C), dtype=np.int64)
    np.add.at(counts, (np.arange(B * Sh * Sw)[:, None], pix), 1)
    return counts.reshape(B, Sh, Sw, C)


def label_hist(y, ps: int, C: int, map255: bool = False) -> np.ndarray:
    """Soft labels: float32(j) / float32(P) for the integer count j of each class among the patch's P pixels."""
    return label_counts(y, ps, C, map255).astype(F32) / F32(ps * ps)


# ---------------------------------------------------------------- K3a

def patch_scores(label):
    """label [B, SS, C] fp32 -> (scores [B,SS] fp32, nonempty [B,SS] int32, nz_count [B] int32, class_freq [B,C] int64).
    presence = label > 0 in IEEE arithmetic: -0.0, negatives and NaN are absent, the smallest denormal is present."""
    label = np.asarray(label, dtype=F32)
    with np.errstate(invalid="ignore"):
        pres = label > 0
    freq = pres.sum(axis=1, dtype=np.int64)                                   # patches of the image that hold the class
    score = np.stack([pres[b].astype(np.int64) @ freq[b] for b in range(label.shape[0])])
    nonempty = pres.any(axis=2)
    scores = np.where(nonempty, score.astype(F32), SENTINEL).astype(F32)
    return scores, nonempty.astype(np.int32), nonempty.sum(axis=1).astype(np.int32), freq


# ---------------------------------------------------------------- K3b

def noisy_scores(scores, nonempty, r, r_off) -> np.ndarray:
    """float32(score) * float32(r[r_off[b] + rank among the image's non-empty patches]); empty patches unmultiplied."""
    scores = np.asarray(scores, dtype=F32)
    r = np.asarray(r, dtype=F32)
    out = scores.copy()
    for b in range(scores.shape[0]):
        ne = np.flatnonzero(np.asarray(nonempty[b]) != 0)
        out[b, ne] = scores[b, ne] * r[int(r_off[b]) + np.arange(len(ne))]
    return out


def patch_select(scores, nonempty, r, r_off, K: int):
    """-> (indices [B,K] int64 of the K smallest noisy scores, ascending, ties to the lower patch index; noisy scores [B,SS])."""
    noisy = noisy_scores(scores, nonempty, r, r_off)
    return np.argsort(noisy, axis=1, kind="stable")[:, :K].astype(np.int64), noisy


# ---------------------------------------------------------------- rows: normalise, K1

def _sq(x) -> np.ndarray:
    return (np.asarray(x, dtype=F32).astype(np.float64) ** 2).sum(axis=1)


def norm32(x) -> np.ndarray:
    """n32 = float32(sqrt(sum_k float64(x_k)^2))."""
    return np.sqrt(_sq(x)).astype(F32)


def normalized(x) -> np.ndarray:
    """float32(x_k) / n32 in IEEE fp32 division, no eps: a zero row gives NaN."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (x / norm32(x)[:, None]).astype(F32)


def stored_rows(x, normalize: bool) -> np.ndarray:
    return normalized(x) if normalize else np.asarray(x, dtype=F32).copy()


def stored_norm(x, normalize: bool) -> np.ndarray:
    """bnorm of an append: the norm (same definition) of the STORED row; an unnormalised append stores x, so bnorm = n32."""
    return norm32(stored_rows(x, normalize))


def _ambiguous_sum(s, D: int) -> np.ndarray:
    return np.sqrt(s * (1.0 - D * SUM_EPS)).astype(F32) != np.sqrt(s * (1.0 + D * SUM_EPS)).astype(F32)


def ambiguous(x, normalize: bool = True) -> np.ndarray:
    """Rows where the order of a double sum could change a rounded norm: float32(sqrt(s (1 - D 2.3e-16))) != float32(sqrt(s (1 + D
    2.3e-16))), for the sum of the row and -- a normalised append rounds a second norm -- of the stored row."""
    x = np.asarray(x, dtype=F32)
    D = x.shape[1]
    a = _ambiguous_sum(_sq(x), D)
    if normalize:
        a |= _ambiguous_sum(_sq(normalized(x)), D)
    return a


def ulp_distance(a, b) -> np.ndarray:
    """Distance in units in the last place between two finite fp32 arrays (sign-magnitude -> ordered integers)."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------- merge

def merge(dist_parts, idx_parts, metric: int):
    """[parts, nq, k] lists -> the k best of each query's parts * k candidates: present entries (id >= 0) first; then the better
    score (metric 0: larger; metric 1: smaller distance; -0.0 == +0.0); then the lower id; then the lower position (part, then
    slot -- an id that two parts hold stays twice, in part order).  Missing entries come out as id -1 with -inf / +inf."""
    d = np.asarray(dist_parts, dtype=F32)
    i = np.asarray(idx_parts, dtype=np.int64)
    parts, nq, k = d.shape
    cd = d.transpose(1, 0, 2).reshape(nq, parts * k)
    ci = i.transpose(1, 0, 2).reshape(nq, parts * k)
    missing = ci < 0
    key = np.where(missing, F32(0), cd if metric == 1 else -cd).astype(F32) + F32(0)      # (+ 0: -0.0 -> +0.0, the two compare equal anyway)
    pos = np.broadcast_to(np.arange(parts * k), ci.shape)
    order = np.lexsort((pos, np.where(missing, 0, ci), key, missing), axis=-1)[:, :k]
    oi = np.take_along_axis(ci, order, axis=1)
    od = np.take_along_axis(cd, order, axis=1)
    om = oi < 0
    return np.where(om, -1, oi), np.where(om, F32(np.inf) if metric == 1 else F32(-np.inf), od).astype(F32)


# ---------------------------------------------------------------- scores -> squared L2 distances

def fma_f32(a, b, c) -> np.ndarray:
    """Correctly rounded fp32 a * b + c: the product of two fp32 values is exact in float64; the float64 sum is rounded to odd (its
    error term from TwoSum), which makes the final rounding to fp32 the rounding of the exact value."""
    p = np.asarray(a, dtype=F32).astype(np.float64) * np.asarray(b, dtype=F32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=F32).astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p + c
        bb = t - p
        e = (p - (t - bb)) + (c - bb)
        fix = np.isfinite(t) & np.isfinite(e) & (e != 0) & ((t.view(np.int64) & 1) == 0)
        t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
        return t.astype(F32)


def scores_to_l2(scores, q) -> np.ndarray:
    """max(0, fma(-2, s, |q|^2)) with |q|^2 the k-ascending fmaf chain (oracle.chain_sqnorm); a missing neighbour (-inf) -> +inf."""
    s = np.asarray(scores, dtype=F32)
    qn2 = oracle.chain_sqnorm(q)[:, None]
    d2 = fma_f32(F32(-2.0), s, qn2)
    with np.errstate(invalid="ignore"):
        d2 = np.where(d2 > 0, d2, F32(0.0)).astype(F32)
    return np.where(s == -np.inf, F32(np.inf), d2).astype(F32)
