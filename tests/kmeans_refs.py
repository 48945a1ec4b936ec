"""The k-means of include/hbird_hip_kmeans.h restated in plain numpy, and the worlds the tests run it on.  No engine code.

  quantise(x)          Q(x) = rint(x * 2^30) as int64 (round-half-even of the exact float64 product)
  update(x, a, K, prev) the integer update: S[c] = sum of Q(x[r]) over a[r] == c, n[c] their count, the centroid
                        (float32)(S / (n * 2^30)); an empty cluster keeps prev[c]
  assign(x, cent)      float64 squared distances, the lower id on ties, -1 for a row with a non-finite component; also the best and the
                        second-best distance of every row
  fit(x, init, max_iter) the loop with its history

fit calls the four pieces through the module's names (quantise, assign, update, count_changed), so a test can swap one for a wrong variant.

Every world generator asserts its own condition: at every iteration of the model every assigned row's best and second-best float64 squared
distances differ by more than 1e-3 of the best (and, stricter than asked, by more than 1e-4 outright), so that fp32 arithmetic cannot flip an
assignment and the model alone decides what the engine must return.  The tie worlds are the exception: their ties are exactly equal centroids.
"""
import functools

import numpy as np

TWO30 = float(2 ** 30)
MARGIN_REL, MARGIN_ABS = 1e-3, 1e-4


def quantise(x):
    return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * TWO30).astype(np.int64)


def integer_sums(x, a, K):
    """(S int64 [K, d], n int64 [K]) over the rows with a >= 0."""
    a = np.asarray(a)
    m = a >= 0
    S = np.zeros((K, x.shape[1]), dtype=np.int64)
    np.add.at(S, a[m], quantise(x[m]))
    n = np.bincount(a[m], minlength=K).astype(np.int64)
    return S, n


def centroids_from_sums(S, n, prev):
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (S.astype(np.float64) / (n.astype(np.float64)[:, None] * TWO30)).astype(np.float32)
    return np.where((n > 0)[:, None], c, np.asarray(prev, dtype=np.float32))


def update(x, a, K, prev):
    """-> (centroids float32 [K, d], n int64 [K], empty clusters)."""
    S, n = integer_sums(x, a, K)
    return centroids_from_sums(S, n, prev), n, int((n == 0).sum())


def assign(x, cent):
    """-> (a int32 [rows], best float64 [rows], second float64 [rows]); second is +inf with one centroid, both are +inf where a == -1."""
    x64, c64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(cent, dtype=np.float32).astype(np.float64)
    d2 = ((x64[:, None, :] - c64[None, :, :]) ** 2).sum(axis=2)
    finite = np.isfinite(x64).all(axis=1)
    d2[~finite] = np.inf
    a = d2.argmin(axis=1).astype(np.int32)             # the first minimum: the lower id
    rows = np.arange(x64.shape[0])
    best = d2[rows, a].copy()
    rest = d2.copy()
    rest[rows, a] = np.inf
    second = rest.min(axis=1)
    a[~finite] = -1
    return a, best, second


def count_changed(a, history_of_a):
    """Rows whose assignment differs from the previous iteration's; at the first iteration the rows with a >= 0."""
    if not history_of_a:
        return int((a >= 0).sum())
    return int((a != history_of_a[-1]).sum())


def min_margin(best, second, a):
    """(smallest (second - best) / best, smallest second - best) over the assigned rows (inf where there is no second centroid)."""
    m = a >= 0
    if not m.any():
        return np.inf, np.inf
    gap = second[m] - best[m]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(best[m] > 0, gap / best[m], np.where(gap > 0, np.inf, 0.0))
    return float(rel.min()), float(gap.min())


def fit(x, init, max_iter):
    """-> dict(centroids, counts, assign, history [{changed, empty, unassigned, inertia}], n_iter, converged, margins [(rel, abs)]).
    inertia here is the SQUARED distance sum in float64 (what an L2 search reports as its distance)."""
    x = np.asarray(x, dtype=np.float32)
    cent = np.asarray(init, dtype=np.float32).copy()
    K = cent.shape[0]
    counts = np.zeros(K, dtype=np.int64)
    seen, history, margins = [], [], []
    empty, converged = K, False
    for it in range(1, max_iter + 1):
        a, best, second = assign(x, cent)
        margins.append(min_margin(best, second, a))
        changed = count_changed(a, seen)
        seen.append(a)
        row = dict(changed=changed, empty=empty, unassigned=int((a < 0).sum()), inertia=float(best[a >= 0].sum()))
        history.append(row)
        if changed == 0:
            converged = True
            break
        cent, counts, empty = update(x, a, K, cent)
        row["empty"] = empty
    return dict(centroids=cent, counts=counts, assign=seen[-1], history=history, n_iter=len(history), converged=converged, margins=margins)


def assert_margins(model):
    for it, (rel, gap) in enumerate(model["margins"], 1):
        assert rel > MARGIN_REL and gap > MARGIN_ABS, (it, rel, gap)


# ---- worlds -------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = v.astype(np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _draw_blobs(K, D, rows, seed, sigma):
    g = np.random.default_rng(seed)
    centres = _unit(g.standard_normal((K, D)))
    blob = np.concatenate([np.arange(K), g.integers(0, K, rows - K)])
    g.shuffle(blob)
    return _unit(centres[blob].astype(np.float64) + sigma * g.standard_normal((rows, D))), blob


def blob_world(K, D, rows, seed, sigma=0.05, max_iter=10):
    """K planted blobs of unit-norm rows around random unit centres, rows dealt to the blobs in random order; init: the first row of every blob.
    -> (x float32 [rows, D], init float32 [K, D], init_rows int64 [K], model)."""
    x, blob = _draw_blobs(K, D, rows, seed, sigma)
    init_rows = np.array([int(np.flatnonzero(blob == c)[0]) for c in range(K)], dtype=np.int64)
    model = fit(x, x[init_rows], max_iter)
    assert_margins(model)
    assert model["converged"] and model["history"][-1]["changed"] == 0 and model["history"][0]["changed"] == rows
    return x, x[init_rows].copy(), init_rows, model


# (K, D, rows, seed): the committed seeds pass the margin condition (checked by tests/test_kmeans_cpu.py on every run)
BLOB_WORLDS = [(3, 16, 600, 11), (33, 16, 4000, 12), (3, 72, 4000, 13), (33, 72, 600, 14)]

# The bank-size seams (the arithmetic is spelled out in tests/linprobe_refs.py at BIG_ROWS, and asserted by tests/test_kmeans_cpu.py):
# 4,100 row tiles in 128 segments of 33 -- all four slots of a wave, a second trip, a segment of 8 tiles and three empty ones --, 33 workgroups
# of kmeans_counts_kernel and kmeans_changed_kernel, rows with j = 1 and 2 in the inertia tree, two default staging chunks (131,072 + 123).
BIG_ROWS = 131195
BIG_HOLE = 100003                                  # the one non-finite row: past row 65,536
BIG_BLOB_WORLD = (5, 16, BIG_ROWS, 15)
SEG_TILES_MIN, MAX_SEGS, WAVES, UNROLL = 16, 128, 8, 4      # KM_SEG_TILES, KM_MAX_SEGS, KM_WAVES, KM_UNROLL of csrc/hbird_kmeans.hip


def km_segments(row0, n):
    """km_accumulate's launch arithmetic -> (rt_begin, rt_end, segs, seg_tiles): the row tiles [rt_begin, rt_end) of rows row0 .. row0 + n - 1,
    segs = min(128, ceil(tiles / 16)) workgroups per column group, each of seg_tiles = ceil(tiles / segs) tiles."""
    rt_begin, rt_end = row0 >> 5, (row0 + n + 31) >> 5
    nt = rt_end - rt_begin
    segs = max(1, min(MAX_SEGS, -(-nt // SEG_TILES_MIN)))
    return rt_begin, rt_end, segs, -(-nt // segs)


def walked_tiles(row0, n, trips=None, slots=UNROLL):
    """[(tile, segment, wave, slot, trip)] of every row tile kmeans_accumulate_kernel reads: in segment s, wave w and slot u of trip p take
    tile t0 + w + 8 u + 32 p while it is below the segment's end.  `trips` and `slots` cut the walk short: WRONG variants for
    tests/test_bank_task_seams_cpu.py."""
    rt_begin, rt_end, segs, seg_tiles = km_segments(row0, n)
    out = []
    for s in range(segs):
        t0 = rt_begin + s * seg_tiles
        t1 = min(rt_end, t0 + seg_tiles)
        for w in range(WAVES):
            p = 0
            while t0 + w + WAVES * UNROLL * p < t1 and (trips is None or p < trips):
                for u in range(slots):
                    t = t0 + w + WAVES * u + WAVES * UNROLL * p
                    if t < t1:
                        out.append((t, s, w, u, p))
                p += 1
    return out


def walked_sums(x, a, K, row0=0, n=None, trips=None, slots=UNROLL):
    """integer_sums over the rows of the tiles that walked_tiles visits (the whole range when the walk is the kernel's)."""
    n = x.shape[0] - row0 if n is None else n
    keep = np.zeros(x.shape[0], dtype=bool)
    for t, *_ in walked_tiles(row0, n, trips, slots):
        keep[max(row0, t * 32):min(row0 + n, (t + 1) * 32)] = True
    return integer_sums(x, np.where(keep, np.asarray(a), -1), K)[0]


@functools.lru_cache(maxsize=None)
def big_blob_world(max_iter=10):
    """BIG_BLOB_WORLD: blob_world's draw with row BIG_HOLE made non-finite (it stays unassigned); the margins are asserted.
    -> (x, init, init_rows, model)."""
    K, D, rows, seed = BIG_BLOB_WORLD
    x, blob = _draw_blobs(K, D, rows, seed, 0.05)
    init_rows = np.array([int(np.flatnonzero(blob == c)[0]) for c in range(K)], dtype=np.int64)
    assert BIG_HOLE not in set(init_rows.tolist())
    x[BIG_HOLE, 2] = np.nan
    model = fit(x, x[init_rows], max_iter)
    assert_margins(model)
    assert model["converged"] and model["history"][0]["changed"] == rows - 1 and all(h["unassigned"] == 1 for h in model["history"])
    return x, x[init_rows].copy(), init_rows, model


def drift_world(K, D, rows, seed, sigma=0.12, max_iter=20):
    """Blobs wide enough to touch, init at the first K rows whatever their blobs: several iterations of real movement.
    -> (x, init, model); the seed is kept only when the model's margins hold at every iteration."""
    g = np.random.default_rng(seed)
    centres = _unit(g.standard_normal((K, D)))
    blob = g.integers(0, K, rows)
    x = _unit(centres[blob].astype(np.float64) + sigma * g.standard_normal((rows, D)))
    model = fit(x, x[:K], max_iter)
    assert_margins(model)
    return x, x[:K].copy(), model


# (K, D, rows, seed, iterations of the model): of the seeds 100 .. 139 these two hold the margins at every iteration
DRIFT_WORLDS = [(5, 16, 600, 110, 8), (5, 16, 600, 124, 5)]


def small_integer_world(D, rows, K, seed):
    """Entries in {-2 .. 2} / 2: every fp32 product, sum and difference of the engine's scores is exact, so the float64 argmin with the
    first minimum is the engine's answer, ties included.  -> (x float32 [rows, D], cent float32 [K, D])."""
    g = np.random.default_rng(seed)
    return (g.integers(-2, 3, (rows, D)) / 2.0).astype(np.float32), (g.integers(-2, 3, (K, D)) / 2.0).astype(np.float32)
