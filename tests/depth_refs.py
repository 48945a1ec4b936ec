"""Depth estimation by retrieval (include/hbird_hip_depth.h) restated in plain numpy, and the worlds the tests run it on.  No engine code.

Rows and predictions step through fp32 explicitly (every numpy operation below is on float32 arrays and rounds once, as the kernels' uncontracted
operations do); the sums are float64.  `variant=` switches ONE definition to a plausible wrong one (tests/test_depth_cpu.py holds each to a
named check that it must fail):
  "den_ignored"      the prediction is the upsampled numerator alone (holes bias the mean)
  "ratio_first"      the bilinear of the per-cell ratios instead of the ratio of the bilinears
  "no_clamp"         the clamp to [min_depth, max_depth] omitted
  "align_corners"    the source index of align_corners=True
  "invalid_gt"       pixels with invalid ground truth counted
"""
import numpy as np

F32 = np.float32
MIN_DEPTH, MAX_DEPTH = 1e-3, 10.0
SUMS = ("n", "n_nopred", "sq", "abs_rel", "sq_rel", "log_sq", "log", "log10", "d1", "d2", "d3")      # HB_DEPTH_SUM_*
NAN_BITS = np.uint32(0x7FC00000)                                                                      # "no prediction" in pred_out
METRICS = ("rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "log10", "d1", "d2", "d3")
VARIANTS = ("den_ignored", "ratio_first", "no_clamp", "align_corners", "invalid_gt")


def valid(v, lo=MIN_DEPTH, hi=MAX_DEPTH):
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v >= F32(lo)) & (v <= F32(hi))


# ---- target rows ---------------------------------------------------------------------------------------------------------------------------
def target_rows(y, ps, r, lo=MIN_DEPTH, hi=MAX_DEPTH):
    """y [B,H,W] fp32 -> (rows [B, H/ps, W/ps, 2 r^2] fp32, nonempty [B, H/ps, W/ps] int32)."""
    y = np.asarray(y, dtype=F32)
    B, H, W = y.shape
    assert H % ps == 0 and W % ps == 0 and ps % r == 0
    Sh, Sw, s = H // ps, W // ps, ps // r
    # [b, py, cy, u, px, cx, v] -> [b, py, px, cy, cx, u * s + v]: a cell's pixels in row-major order
    px = y.reshape(B, Sh, r, s, Sw, r, s).transpose(0, 1, 4, 2, 5, 3, 6).reshape(B, Sh, Sw, r * r, s * s)
    ok = valid(px, lo, hi)
    acc = np.zeros(px.shape[:-1], dtype=F32)
    for i in range(s * s):                                   # the chain: plain fp32 adds from 0.0f, an invalid pixel adds nothing
        acc = np.where(ok[..., i], acc + np.where(ok[..., i], px[..., i], F32(0)), acc).astype(F32)
    area = F32(s * s)
    num = (acc / area).astype(F32)
    den = (ok.sum(-1).astype(F32) / area).astype(F32)
    return np.concatenate([num, den], axis=-1), ok.any(axis=(-1, -2)).astype(np.int32)


# ---- prediction ----------------------------------------------------------------------------------------------------------------------------
def source_index(n_out, G, align_corners=False):
    """ATen's area_pixel_compute_source_index in fp32 -> (i0, i1, l0, l1)."""
    dst = np.arange(n_out, dtype=F32)
    if align_corners:
        scale = F32(G - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        f = (scale * dst).astype(F32)
    else:
        scale = F32(G) / F32(n_out)
        f = np.maximum((scale * (dst + F32(0.5))).astype(F32) - F32(0.5), F32(0)).astype(F32)
    i0 = np.minimum(np.floor(f).astype(np.int64), G - 1)
    i1 = np.minimum(i0 + 1, G - 1)
    l1 = (f - i0.astype(F32)).astype(F32)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def cell_grids(agg, S, r):
    """agg [B, S*S, 2 r^2] -> (Ngrid, Dgrid) [B, S r, S r] with gy = py r + cy, gx = px r + cx."""
    agg = np.asarray(agg, dtype=F32)
    B = agg.shape[0]
    a = agg.reshape(B, S, S, 2, r, r).transpose(3, 0, 1, 4, 2, 5).reshape(2, B, S * r, S * r)      # [which, b, py, cy, px, cx]
    return a[0], a[1]


def bilinear(grid, h, w, align_corners=False):
    """K6's four-tap formula in its order, fp32."""
    G = grid.shape[-1]
    y0, y1, ly0, ly1 = source_index(h, G, align_corners)
    x0, x1, lx0, lx1 = source_index(w, G, align_corners)
    with np.errstate(invalid="ignore", over="ignore"):
        top = ((lx0 * grid[:, y0][:, :, x0]).astype(F32) + (lx1 * grid[:, y0][:, :, x1]).astype(F32)).astype(F32)
        bot = ((lx0 * grid[:, y1][:, :, x0]).astype(F32) + (lx1 * grid[:, y1][:, :, x1]).astype(F32)).astype(F32)
        return ((ly0[:, None] * top).astype(F32) + (ly1[:, None] * bot).astype(F32)).astype(F32)


def predict(agg, S, r, h, w, lo=MIN_DEPTH, hi=MAX_DEPTH, variant=None):
    """-> (pred [B,h,w] fp32 with the NaN 0x7FC00000 where there is no prediction, has [B,h,w] bool)."""
    assert variant in (None,) + VARIANTS
    ac = variant == "align_corners"
    Ng, Dg = cell_grids(agg, S, r)
    Dn = bilinear(Dg, h, w, ac)
    has = Dn > F32(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if variant == "ratio_first":
            ratio = np.where(Dg > 0, Ng / np.where(Dg > 0, Dg, F32(1)), F32(0)).astype(F32)
            q = bilinear(ratio, h, w, ac)
        elif variant == "den_ignored":
            q = bilinear(Ng, h, w, ac)
        else:
            q = (bilinear(Ng, h, w, ac) / Dn).astype(F32)
        p = q if variant == "no_clamp" else np.fmin(np.fmax(q, F32(lo)), F32(hi)).astype(F32)   # fmaxf / fminf: a NaN quotient takes the bound
    pred = np.where(has, p, F32(0)).astype(F32)
    bits = pred.view(np.uint32).copy()
    bits[~has] = NAN_BITS
    return bits.view(F32), has


# ---- sums and metrics ----------------------------------------------------------------------------------------------------------------------
def sums(pred, has, gt, lo=MIN_DEPTH, hi=MAX_DEPTH, variant=None):
    """-> float64 [B, 11] in the order of SUMS, and float64 [B, 3]: the scales the errors of the three log-based sums (log_sq, log, log10) are
    held to.  A term ln p - ln g carries the rounding of two logarithms, about u (|ln p| + |ln g|) =: u L, whatever its own size -- where the
    prediction is good, p ~ g and the term is far smaller than its error.  So the scales are sum L for the signed log sum,
    sum (2 |dl| L + dl^2) for the squares, and sum (|log10 p| + |log10 g|) for the log10 sum."""
    gt = np.asarray(gt, dtype=F32)
    B = gt.shape[0]
    out = np.zeros((B, len(SUMS)), dtype=np.float64)
    scales = np.zeros((B, 3))
    for b in range(B):
        gok = valid(gt[b], lo, hi) if variant != "invalid_gt" else np.ones(gt[b].shape, dtype=bool)
        out[b, 1] = np.count_nonzero(gok & ~has[b])
        m = gok & has[b]
        p, g = pred[b][m].astype(np.float64), gt[b][m].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d = p - g
            dl = np.log(p) - np.log(g)
            ratio = np.fmax(p / g, g / p)
            out[b, 0] = p.size
            out[b, 2], out[b, 3], out[b, 4] = (d * d).sum(), (np.abs(d) / g).sum(), (d * d / g).sum()
            out[b, 5], out[b, 6], out[b, 7] = (dl * dl).sum(), dl.sum(), np.abs(np.log10(p) - np.log10(g)).sum()
            out[b, 8], out[b, 9], out[b, 10] = (ratio < 1.25).sum(), (ratio < 1.25 ** 2).sum(), (ratio < 1.25 ** 3).sum()
            L = np.abs(np.log(p)) + np.abs(np.log(g))
            scales[b] = (2 * np.abs(dl) * L + dl * dl).sum(), L.sum(), (np.abs(np.log10(p)) + np.abs(np.log10(g))).sum()
    return out, scales


def finish(s):
    """One float64 row of SUMS -> the metrics (None when n == 0).  silog is Eigen's scale-invariant log error with lambda = 1:
    sqrt(mean(dl^2) - mean(dl)^2), not multiplied by 100."""
    s = np.asarray(s, dtype=np.float64)
    n = s[0]
    if n <= 0:
        return None
    return {"rmse": float(np.sqrt(s[2] / n)), "abs_rel": float(s[3] / n), "sq_rel": float(s[4] / n), "rmse_log": float(np.sqrt(s[5] / n)),
            "silog": float(np.sqrt(max(0.0, s[5] / n - (s[6] / n) ** 2))), "log10": float(s[7] / n), "d1": float(s[8] / n), "d2": float(s[9] / n),
            "d3": float(s[10] / n)}


def metrics(all_sums):
    """[n_img, 11] -> (headline: the mean of the per-image metrics over images with n > 0, pooled: the metrics of the totals, per_image: a list
    with None for images with n == 0, n_nopred: total, empty_images: the indices with n == 0)."""
    all_sums = np.asarray(all_sums, dtype=np.float64).reshape(-1, len(SUMS))
    per = [finish(s) for s in all_sums]
    kept = [m for m in per if m is not None]
    head = {k: float(np.mean([m[k] for m in kept])) for k in METRICS} if kept else None
    return head, finish(all_sums.sum(0)), per, int(all_sums[:, 1].sum()), [i for i, m in enumerate(per) if m is None]


# ---- worlds ----------------------------------------------------------------------------------------------------------------------------------
TARGET_SHAPES = [(8, 1), (8, 2), (8, 8), (14, 1), (14, 7), (14, 14), (16, 4)]       # (ps, r); with B = 2, S in {2, 3}


def depth_maps(B, S, ps, r, seed):
    """[B, S ps, S ps] fp32 with every kind of invalid value sprinkled in, a wholly invalid cell (patch (0, 0, 0), cell (0, 0)), a wholly
    invalid patch (the last one) and a wholly valid patch (0, 0, 1)."""
    rng = np.random.default_rng(seed)
    H, s = S * ps, ps // r
    y = rng.uniform(0.5, 9.5, (B, H, H)).astype(F32)
    m = rng.random((B, H, H))
    for lo, hi, v in ((0.00, 0.04, 0.0), (0.04, 0.07, np.nan), (0.07, 0.09, np.inf), (0.09, 0.11, -np.inf), (0.11, 0.14, 12.0), (0.14, 0.16, 1e-4),
                      (0.16, 0.18, -2.0)):
        y[(m >= lo) & (m < hi)] = v
    y[0, :ps, ps:2 * ps] = rng.uniform(0.5, 9.5, (ps, ps)).astype(F32)
    y[0, :s, :s] = 0.0
    y[B - 1, H - ps:, H - ps:] = np.nan
    return y


def agg_world(B, S, r, h, w, seed):
    """(agg [B, S*S, 2 r^2], gt [B,h,w]): rows as an aggregation leaves them -- den in (0, 1], num = depth x den with depths from below
    min_depth to beyond max_depth (the clamp acts) -- with den = 0 cells, isolated everywhere and as one block in image 0 that covers more
    than half the grid (pixels without a prediction; the whole image at S r = 1); gt with every kind of invalid value."""
    rng = np.random.default_rng(seed)
    G = S * r
    den = rng.uniform(0.05, 1.0, (B, G, G)).astype(F32)
    depth = rng.uniform(0.2, 12.0, (B, G, G)).astype(F32)
    depth[rng.random((B, G, G)) < 0.05] = 1e-4
    den[rng.random((B, G, G)) < 0.12] = 0.0
    k = G // 2 + 1
    den[0, :k, :k] = 0.0
    num = (depth * den).astype(F32)
    a = np.stack([num, den]).reshape(2, B, S, r, S, r).transpose(1, 2, 4, 0, 3, 5).reshape(B, S * S, 2 * r * r)      # [b, py, px, which, cy, cx]
    gt = rng.uniform(0.3, 9.9, (B, h, w)).astype(F32)
    m = rng.random((B, h, w))
    for lo, hi, v in ((0.00, 0.05, 0.0), (0.05, 0.08, np.nan), (0.08, 0.10, np.inf), (0.10, 0.12, 11.0), (0.12, 0.13, -1.0)):
        gt[(m >= lo) & (m < hi)] = v
    return np.ascontiguousarray(a, dtype=F32), gt


def prediction_cases(ps=8):
    """(S, r, h, w) of the prediction tests: S in {1, 2, 3, 16} x r in {1, 2, ps} x {native, (37, 53), (5, 300), a downsampling size}."""
    out = []
    for S in (1, 2, 3, 16):
        for r in (1, 2, ps):
            G = S * r
            for h, w in ((S * ps, S * ps), (37, 53), (5, 300), (max(1, G // 2), max(1, (2 * G) // 3))):
                out.append((S, r, h, w))
    return out
