"""K6 (upsample + argmax), K6 + K7 fused (the confusion counts in the same kernel) and K7 (confusion_update), csrc/hbird_post.hip,
on every launch path against the oracle -- bit for bit and count for count.

K6 evaluates the per-pixel fp32 formula of oracle.upsample_argmax with contraction off, in the same order of operations, so the class
maps must be identical, not nearly so.  The shapes below reach every rows-per-chunk instantiation R, bands taller than R (several
chunks), classes staged in several LDS passes, S = 1, maps narrower than a wave and maps smaller than the token grid; the fused cases
reach the LDS histogram, both hash-table sizes, probe overflow to global atomics and the noise shortcut.
tests/test_post_agg_coverage_cpu.py restates the launch arithmetic and checks that these lists reach every path.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import pytest

import golden_inputs as gi
import oracle

pytestmark = pytest.mark.gpu

# label_hat [B, S*S, C] -> class maps [B, 1, h, w];  C * h * w <= 4e7 per oracle call (it materialises the upsampled tensor)
K6Case = namedtuple("K6Case", "B S C h w")
K6_CASES = [
    K6Case(2, 1, 1, 5, 5),            # S = 1, one class, a map narrower than a wave
    K6Case(1, 1, 2, 40, 63),          # one band of 40 rows: R = 10, four chunks
    K6Case(2, 2, 151, 63, 65),        # R = 16, band 0 of 47 rows (three chunks), a second wave of one column
    K6Case(1, 2, 2, 65, 1),           # w = 1 < S
    K6Case(2, 7, 151, 98, 99),        # h = 14 S: R = 14; w = 14 S + 1
    K6Case(1, 7, 2, 84, 64),          # h = 12 S: R = 12
    K6Case(1, 7, 151, 280, 5),        # h = 40 S: R = 10, six chunks; w < S
    K6Case(1, 37, 1000, 128, 128),    # ncols = 37: 221 classes per LDS pass, five passes
    K6Case(1, 37, 151, 5, 518),       # h < S, w = 14 S
    K6Case(2, 37, 151, 519, 63),      # h = 14 S + 1, w < S
    K6Case(1, 37, 2, 1, 37),          # a single output row, w = S
    K6Case(1, 64, 151, 63, 64),       # h < S; ncols = 64: 128 classes per pass, two passes
    K6Case(1, 64, 1000, 5, 896),      # w = 14 S: 390 classes per pass, three passes
    K6Case(1, 64, 151, 896, 65),      # h = 14 S: R = 14, two chunks
]

# fused K6 + K7: conf[G, P] counts (gt, argmax) pairs; pattern of the gt map (see gt_map); ignore_index
FusedCase = namedtuple("FusedCase", "B S C h w G P pattern ignore")
FUSED_CASES = [
    FusedCase(2, 7, 21, 98, 99, 21, 21, "rects", 255),           # LDS histogram
    FusedCase(1, 2, 64, 63, 65, 64, 64, "noise", None),          # LDS histogram, every lane its own pair
    FusedCase(1, 37, 65, 128, 128, 65, 65, "rects", 0),          # hash table of 2^9; ignore_index inside the class range
    FusedCase(1, 1, 151, 40, 63, 151, 151, "noise", 255),        # hash table of 2^8 (small staging area), noise shortcut
    FusedCase(1, 37, 5, 518, 518, 1000, 5, "noise", None),       # 2^8 entries (5 classes staged), more distinct pairs than entries: probe overflow
    FusedCase(1, 7, 300, 280, 5, 300, 300, "checker", 0),        # 2^9, period-3 checkerboard across wave boundaries
    FusedCase(1, 64, 300, 65, 896, 300, 300, "one", 255),        # one (gt, pred) pair over the whole map
    FusedCase(1, 37, 151, 5, 518, 21, 151, "noise", 255),        # num_gt < num_pred: gt out of range
    FusedCase(2, 7, 151, 98, 99, 151, 64, "rects", 0),           # num_gt > num_pred: predictions out of range
    FusedCase(1, 64, 151, 63, 64, 64, 151, "checker", None),     # num_gt < num_pred, two staging passes
    FusedCase(1, 37, 1000, 128, 128, 300, 1000, "noise", 255),   # five staging passes, 300 x 1000 matrix
]

# standalone K7: below and at / above its 120 KiB LDS histogram (G * P * 4 bytes)
K7_CASES = [(175, 175), (176, 176), (120, 256), (121, 256)]


def k6_id(c):
    return f"B{c.B}-S{c.S}-C{c.C}-{c.h}x{c.w}"


def fused_id(c):
    return f"S{c.S}-C{c.C}-{c.h}x{c.w}-G{c.G}-P{c.P}-{c.pattern}-ign{c.ignore}"


def label_hat(B, S, C, seed):
    return np.random.default_rng(seed).random((B, S * S, C), dtype=np.float32)


def gt_map(c, seed):
    """int64 [B, 1, h, w] ground truth of pattern c.pattern:
      one      one class over the whole map (label_hat then favours one class: one (gt, pred) pair)
      rects    a few large rectangles (golden_inputs.random_masks)
      noise    even rows: a random class per pixel (as many pairs as pixels: the noise shortcut); odd rows: runs of two pixels
               (groups of two -- no shortcut -- with more distinct pairs than a table holds: probe overflow)
      checker  3 x 3 cells of three classes: the period does not divide the 64-pixel wave
    Except `one`, every map also holds ignore_index (when set), gt values outside [0, G) (negative and >= G) and 255."""
    B, h, w, G = c.B, c.h, c.w, c.G
    rng = np.random.default_rng(seed)
    if c.pattern == "one":
        return np.full((B, 1, h, w), G // 2, np.int64)
    if c.pattern == "rects":
        y = gi.random_masks(B, h, w, G, seed=seed, with_255=True)
    elif c.pattern == "noise":
        y = rng.integers(0, G, (B, 1, h, w))
        runs = np.repeat(rng.integers(0, G, (B, 1, h, (w + 1) // 2)), 2, axis=3)[..., :w]
        y[:, :, 1::2] = runs[:, :, 1::2]
    else:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        y = np.broadcast_to((((yy // 3) + (xx // 3)) % 3) * max(1, G // 3), (B, 1, h, w)).copy()
    y = y.astype(np.int64)
    flat = y.reshape(-1)
    n = flat.size
    spots = rng.choice(n, size=min(n, 4 + n // 50), replace=False)
    flat[spots[0::4]] = G + rng.integers(0, 5, spots[0::4].shape)     # out of range above
    flat[spots[1::4]] = -1 - rng.integers(0, 3, spots[1::4].shape)    # out of range below
    flat[spots[2::4]] = 255
    if c.ignore is not None:
        flat[spots[3::4]] = c.ignore
    return y


def fused_inputs(c, seed):
    lh = label_hat(c.B, c.S, c.C, seed)
    if c.pattern == "one":
        lh[..., min(c.C, c.P) // 3] += 2.0
    return lh, gt_map(c, seed + 1)


# ---------------------------------------------------------------- K6

@pytest.mark.parametrize("c", K6_CASES, ids=k6_id)
def test_k6_class_map_is_the_oracle_bit_for_bit(cuda_device, c):
    import torch
    from hbird_mi import ops
    lh = label_hat(c.B, c.S, c.C, K6_CASES.index(c))
    got = ops.upsample_argmax(torch.from_numpy(lh).cuda(), c.S, c.h, c.w).cpu().numpy()
    ref = oracle.upsample_argmax(lh, c.S, c.h, c.w)
    assert got.shape == (c.B, 1, c.h, c.w)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{len(bad)} pixels differ, first (b, 0, y, x) {bad[:4].tolist()}"


def _k6(lh, S, h, w):
    import torch
    from hbird_mi import ops
    got = ops.upsample_argmax(torch.from_numpy(lh).cuda(), S, h, w).cpu().numpy()
    assert np.array_equal(got, oracle.upsample_argmax(lh, S, h, w))
    return got


def test_k6_ties_go_to_the_lowest_class(cuda_device):
    """Equal channels interpolate to equal values (same fp32 steps), and the first maximum must win -- within one LDS pass, across
    passes, and when every class ties."""
    lh = label_hat(2, 7, 3, 11)
    lh[..., 1] = lh[..., 0]                                     # class 1 a copy of class 0: never predicted
    got = _k6(lh, 7, 98, 99)
    assert not (got == 1).any() and (got == 0).any()
    lh = label_hat(2, 37, 1000, 12)                             # 221 classes per pass at 128 x 128
    lh[0, :, 700] = lh[0, :, 5] = lh[0, :, 5] + 10.0            # pass 0 against pass 3
    lh[1, :, 442] = lh[1, :, 221] = lh[1, :, 221] + 10.0        # the first classes of passes 1 and 2
    got = _k6(lh, 37, 128, 128)
    assert (got[0] == 5).all() and (got[1] == 221).all()
    lh = np.repeat(label_hat(1, 64, 1, 13), 1000, axis=2)      # all classes equal (varying over the tokens), three passes
    assert not _k6(lh, 64, 5, 896).any()
    assert not _k6(np.full((2, 4, 151), 0.25, np.float32), 2, 63, 65).any()   # a constant label_hat


# ---------------------------------------------------------------- K6 + K7

@pytest.mark.parametrize("c", FUSED_CASES, ids=fused_id)
def test_k6_k7_fused_counts_are_the_oracle(cuda_device, c):
    import torch
    from hbird_mi import ops
    lh, gt = fused_inputs(c, 100 + FUSED_CASES.index(c))
    lt, gtt = torch.from_numpy(lh).cuda(), torch.from_numpy(gt).cuda()
    ref_map = oracle.upsample_argmax(lh, c.S, c.h, c.w)
    ref = oracle.confusion_matrix(gt, ref_map, c.G, c.P, c.ignore)
    conf = torch.zeros((c.G, c.P), dtype=torch.int64, device="cuda")
    out = ops.upsample_argmax_confusion(lt, c.S, gtt, conf, c.ignore, want_map=True)
    assert np.array_equal(out.cpu().numpy(), ref_map)
    assert np.array_equal(out.cpu().numpy(), ops.upsample_argmax(lt, c.S, c.h, c.w).cpu().numpy())
    got = conf.cpu().numpy()
    assert got.sum() == ref.sum() and np.array_equal(got, ref), f"{int((got != ref).sum())} bins differ (counted {got.sum()}, want {ref.sum()})"
    conf2 = torch.zeros((c.G, c.P), dtype=torch.int64, device="cuda")
    assert ops.upsample_argmax_confusion(lt, c.S, gtt, conf2, c.ignore) is None
    assert np.array_equal(conf2.cpu().numpy(), ref)


# ---------------------------------------------------------------- K7

@pytest.mark.parametrize("G,P", K7_CASES, ids=lambda v: str(v))
def test_k7_confusion_update_around_the_lds_limit(cuda_device, G, P):
    import torch
    from hbird_mi import ops
    rng = np.random.default_rng(G * 1000 + P)
    n = 300_000
    gt = np.repeat(rng.integers(-2, G + 3, n // 4), 4)                 # runs of four: grouped and single counting
    pred = rng.integers(-1, P + 2, n)
    gt[rng.choice(n, 5000, replace=False)] = 255
    for ign in (None, 255, 3):
        ref = oracle.confusion_matrix(gt, pred, G, P, ign)
        conf = torch.zeros((G, P), dtype=torch.int64, device="cuda")
        ops.confusion_update(conf, torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), ign)
        assert np.array_equal(conf.cpu().numpy(), ref), (G, P, ign)
