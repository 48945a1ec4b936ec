"""Depth grids (include/hbird_hip_depth_grid.h, hbird_mi/depth.py) restated in plain numpy.  No engine code.

`weighted_sums` is the resampling chain itself: numpy's elementwise float64 multiply and add round once each, exactly as the kernel's
uncontracted product and add do, so it is bit-exact.  `depth_bootstrap` is the estimator on per-image sums: per-image metrics from
depth_refs.finish, resampled with SHARED multiplicities, headline = resampled metric / resampled kept count, pooled = the metrics of the
resampled sums.  `variant=` switches ONE definition to a plausible wrong one (tests/test_depth_grid_cpu.py holds each to a named check that it
must fail):
  "descending"       the images are added in descending order
  "divide_by_n_img"  the headline is divided by the image count instead of the count of resampled images that scored a pixel
  "per_config_draws" every configuration draws multiplicities of its own (the replicates are no longer paired)
"""
import numpy as np

import depth_refs as R

VARIANTS = ("descending", "divide_by_n_img", "per_config_draws")
NM, NS = len(R.METRICS), len(R.SUMS)
COLS = NM + 1 + NS                 # per configuration: nine per-image metrics, the kept flag, the eleven raw sums


def weighted_sums(table, W, variant=None):
    """table [n_img, cols] float64, W [R, n_img] integers -> [R, cols] float64: acc = 0.0; for i ascending: acc = acc + (double)W[r][i] * table[i][col]."""
    table, W = np.asarray(table, dtype=np.float64), np.asarray(W)
    acc = np.zeros((W.shape[0], table.shape[1]), dtype=np.float64)
    order = range(table.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (reversed(order) if variant == "descending" else order):
            acc = acc + W[:, i].astype(np.float64)[:, None] * table[i][None, :]
    return acc


def table_of(sums):
    """sums [n_cfg, n_img, 11] -> the image-major table [n_img, n_cfg * COLS]."""
    sums = np.asarray(sums, dtype=np.float64)
    n_cfg, n_img, _ = sums.shape
    t = np.zeros((n_img, n_cfg, COLS))
    for c in range(n_cfg):
        for i in range(n_img):
            m = R.finish(sums[c, i])
            if m is not None:
                t[i, c, :NM] = [m[k] for k in R.METRICS]
                t[i, c, NM] = 1.0
        t[:, c, NM + 1:] = sums[c]
    return t.reshape(n_img, -1)


def finish_arrays(s):
    """depth_refs.finish on arrays [..., 11] -> {metric: [...]}, NaN where n <= 0; one float64 rounding per operation."""
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(s[..., 0] > 0, s[..., 0], np.nan)
        ml = s[..., 6] / n
        return {"rmse": np.sqrt(s[..., 2] / n), "abs_rel": s[..., 3] / n, "sq_rel": s[..., 4] / n, "rmse_log": np.sqrt(s[..., 5] / n),
                "silog": np.sqrt(np.maximum(0.0, s[..., 5] / n - ml * ml)), "log10": s[..., 7] / n, "d1": s[..., 8] / n, "d2": s[..., 9] / n,
                "d3": s[..., 10] / n}


def depth_bootstrap(sums, W, variant=None):
    """sums [n_cfg, n_img, 11] float64, W [R, n_img] -> (samples, pooled): {metric: float64 [R, n_cfg]} each."""
    assert variant in (None,) + VARIANTS
    sums, W = np.asarray(sums, dtype=np.float64), np.asarray(W)
    n_cfg, n_img, _ = sums.shape
    table = table_of(sums)
    if variant == "per_config_draws":         # configuration c takes the replicates' rows rotated by c
        out = np.concatenate([weighted_sums(table[:, c * COLS:(c + 1) * COLS], np.roll(W, c, axis=0)) for c in range(n_cfg)], axis=1)
    else:
        out = weighted_sums(table, W, variant)
    out = out.reshape(-1, n_cfg, COLS)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.float64(n_img) if variant == "divide_by_n_img" else out[:, :, NM]
        samples = {m: out[:, :, i] / den for i, m in enumerate(R.METRICS)}
    return samples, finish_arrays(out[:, :, NM + 1:])


def multiplicities(n_img, R_, seed):
    """Some rows of multiplicities that sum to n_img (numpy's generator: the CPU tests need no particular resampler)."""
    rng = np.random.default_rng(seed)
    return np.stack([np.bincount(rng.integers(0, n_img, n_img), minlength=n_img) for _ in range(R_)]).astype(np.int32)


def spread_table(n_img, cols, seed):
    """float64 [n_img, cols] with magnitudes spread over about 1e12 and both signs: a sum whose bits depend on the order of its terms."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_img, cols)) * 10.0 ** rng.uniform(-6, 6, (n_img, cols))


def grid_world(n_cfg, B, S, r, h, w, seed, nopred_slab=None):
    """(agg [n_cfg, B, S*S, 2 r^2], gt [B, h, w]): every configuration's slab is depth_refs.agg_world at a seed of its own -- each with image
    0's hole block --, one ground truth (the first slab's).  Slab `nopred_slab` has den == 0 everywhere: no pixel has a prediction."""
    slabs, gt = [], None
    for c in range(n_cfg):
        a, g = R.agg_world(B, S, r, h, w, seed=seed + 101 * c)
        gt = g if gt is None else gt
        if c == nopred_slab:
            a[:, :, r * r:] = 0.0
        slabs.append(a)
    return np.ascontiguousarray(np.stack(slabs), dtype=np.float32), gt
