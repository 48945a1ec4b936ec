"""References for excluding searches on the certified fp16 screen (csrc/hbird_exclude_screen.hip): the IMAGE WORLD, a bank whose queries find
their own image at the top of their lists; a host model of the route's three levels on it; and the numpy restatement of what the excluding
re-rank kernel (hb_index_exclude_rerank) must return for given candidate lists.  Plain numpy; nothing here knows of tiles, pools or waves.
tests/test_exclude_screen_gpu.py holds the kernel and the route to these; tests/test_exclude_screen_cpu.py pins the model's counts and shows
which wrong kernels the restatement catches.

The restatement, per query: the candidates that are ALLOWED (row >= 0, and not: query group >= 0, row inside the table, same group), ranked by
(exact score descending, row ascending); the first k are the answer, the tail is -1 / the missing value.  Certificate: the k-th allowed exact
score strictly above (pass score of the LAST list entry, allowed or not) + E; a full list with fewer than k allowed candidates is never
certified; a list that ends in -1 is certified when the bank holds fewer than kc rows.
"""
from __future__ import annotations

import functools

import numpy as np

import f16_pass_refs as fr

METRIC_NAME = {0: "dot_product", 1: "l2"}


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def image_world():
    """6,000 x 64 rows in 36 contiguous "images" (12 of 300 rows, 24 of 100), 20 classes; a row = its class centre + a[g] x its image's offset
    + noise, normalised: with a = 0 an image is invisible, with a = 2.5 its rows are each other's nearest neighbours by far.  240 queries: the
    first four rows of every image, then 96 random rows, each plus a little noise.  -> rows, groups, q, qg (read-only)."""
    rng = np.random.default_rng(0)
    D, C = 64, 20
    sizes = [300] * 12 + [100] * 24
    N, G = 6000, 36
    assert sum(sizes) == N and len(sizes) == G
    groups = np.repeat(np.arange(G), sizes)
    centres = unit(rng.standard_normal((C, D)))
    off = unit(rng.standard_normal((G, D)))
    a = np.array([(0.0, 0.15, 0.5, 2.5)[g % 4] for g in range(G)])
    cls = rng.integers(0, C, N)
    nz = unit(rng.standard_normal((N, D)))
    rows = unit(centres[cls] + a[groups][:, None] * off[groups] + 0.6 * nz).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    src = np.concatenate([(starts[:, None] + np.arange(4)[None, :]).reshape(-1), rng.integers(0, N, 96)])
    q = (rows[src] + 0.05 * unit(rng.standard_normal((240, D)))).astype(np.float32)
    qg = groups[src].astype(np.int32)
    groups = groups.astype(np.int32)
    for arr in (rows, groups, q, qg):
        arr.setflags(write=False)
    return rows, groups, q, qg


@functools.lru_cache(maxsize=None)
def small_world():
    """A second small bank with d = 40 (no multiple of 8): 1,400 rows in 7 images of 200, 70 queries (no multiple of 4), same construction."""
    rng = np.random.default_rng(1)
    D, C, G, per = 40, 8, 7, 200
    N = G * per
    groups = np.repeat(np.arange(G), per)
    centres = unit(rng.standard_normal((C, D)))
    off = unit(rng.standard_normal((G, D)))
    a = np.array([(0.0, 0.5, 2.5)[g % 3] for g in range(G)])
    cls = rng.integers(0, C, N)
    rows = unit(centres[cls] + a[groups][:, None] * off[groups] + 0.6 * unit(rng.standard_normal((N, D)))).astype(np.float32)
    src = rng.integers(0, N, 70)
    q = (rows[src] + 0.05 * unit(rng.standard_normal((70, D)))).astype(np.float32)
    qg = groups[src].astype(np.int32)
    groups = groups.astype(np.int32)
    for arr in (rows, groups, q, qg):
        arr.setflags(write=False)
    return rows, groups, q, qg


@functools.lru_cache(maxsize=None)
def tiny_world():
    """50 rows (fewer than any candidate list holds) in 5 images of 10: the first rows and queries of the small world."""
    rows, _, q, _ = small_world()
    groups = (np.arange(50) // 10).astype(np.int32)
    rows, q, qg = rows[:50].copy(), q[:10].copy(), (np.arange(10) % 5).astype(np.int32)
    for arr in (rows, groups, q, qg):
        arr.setflags(write=False)
    return rows, groups, q, qg


def world(name):
    """rows, groups, q, qg of "image", "small" or "tiny"."""
    return {"image": image_world, "small": small_world, "tiny": tiny_world}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, metric):
    """f16_pass_refs.float_reference of a world: s16, s (float64), qn, E, ..."""
    rows, _, q, _ = world(name)
    return fr.float_reference(q, rows, metric)


@functools.lru_cache(maxsize=None)
def chain_ranking(name, metric):
    """The full fp32 chain ranking of every query (oracle.knn_chain_f32 at k = N): ids [nq, N] and distances [nq, N] -- THE order and the
    distance bits of the fp32 search."""
    import oracle
    rows, _, q, _ = world(name)
    idx, dist = oracle.knn_chain_f32(q, rows, rows.shape[0], METRIC_NAME[metric])
    idx.setflags(write=False); dist.setflags(write=False)
    return idx, dist


def allowed_mask(cand, groups, qg):
    """bool [nq, kc]: candidate c of query i is allowed (the kernel's rule; rows at or beyond the table are never excluded)."""
    cand = np.asarray(cand)
    n = len(groups)
    inside = (cand >= 0) & (cand < n)
    g = np.where(inside, np.asarray(groups)[np.clip(cand, 0, max(n - 1, 0))], -2)
    qg = np.asarray(qg)[:, None]
    return (cand >= 0) & ~((qg >= 0) & inside & (g == qg))


# ---- the host model of the route ---------------------------------------------------------------------------------------------------------
def _level(s16, s, E, groups, qg, k, kc, floor=None):
    """One pass of the model for every query: the kc best rows by s16 among those with s16 >= floor -> (certified, kth, n_allowed, margin): margin =
    (k-th allowed exact score - threshold) / E, the threshold being the last pass score + E of a full list and floor + E of a list that did not
    fill up (hb_rerank_finish's seed rule); nan where fewer than k candidates are allowed."""
    nq, N = s16.shape
    cert = np.zeros(nq, dtype=bool); kth = np.full(nq, -np.inf); n_allowed = np.zeros(nq, dtype=np.int64); margin = np.full(nq, np.nan)
    for i in range(nq):
        order = np.argsort(-s16[i], kind="stable")
        if floor is not None:
            order = order[s16[i, order] >= floor[i]]
        cand = order[:kc]
        ok = groups[cand] != qg[i] if qg[i] >= 0 else np.ones(len(cand), dtype=bool)
        n_allowed[i] = int(ok.sum())
        if n_allowed[i] < k:
            cert[i] = len(cand) < kc and N < kc         # (every row was a candidate)
            continue
        kth[i] = -np.sort(-s[i, cand[ok]])[k - 1]
        thr = (s16[i, cand[kc - 1]] if len(cand) == kc else floor[i]) + E[i]
        margin[i] = (kth[i] - thr) / E[i]
        cert[i] = kth[i] > thr
    return cert, kth, n_allowed, margin


@functools.lru_cache(maxsize=None)
def route_model(k, metric, escalation=True):
    """The route's three levels on the image world by the host model: fp16 images of both operands, float64 sums, E by the shipped formula;
    level 0 at kc = kc_of(k), the second pass at 256 from the floor kth - 1.001 E (-inf where level 0 held fewer than k allowed candidates).
    Pools and phases are absent.  -> dict: level [nq] (0, 1: second pass, 2: the rungs), counts (n0, n1, n2), margins (all finite ones, in
    units of E), all_excluded: queries whose 256 second-pass candidates are all excluded."""
    rows, groups, q, qg = image_world()
    ref = reference("image", metric)
    s16, s, E = ref["s16"], ref["s"], ref["E"]
    kc = fr.kc_of(k)
    c0, kth0, _, m0 = _level(s16, s, E, groups, qg, k, kc)
    level = np.where(c0, 0, 2)
    margins = [m0[np.isfinite(m0)]]
    all_excl = 0
    if escalation and kc < 256:
        bad = np.flatnonzero(~c0)
        floor = np.where(np.isfinite(kth0[bad]), kth0[bad] - 1.001 * E[bad], -np.inf)
        c1, _, na1, m1 = _level(s16[bad], s[bad], E[bad], groups, qg[bad], k, 256, floor)
        level[bad[c1]] = 1
        margins.append(m1[np.isfinite(m1)])
        all_excl = int((na1 == 0).sum())
    counts = tuple(int((level == v).sum()) for v in (0, 1, 2))
    return {"level": level, "counts": counts, "margins": np.concatenate(margins), "all_excluded": all_excl}


def tail_excluded_lists(metric, k, kc):
    """Hand-made lists on the image world, one per query, excluding the image AFTER the query's own: the k best allowed rows by s16, then the
    kc - k rows of the excluded image that score lowest (excluded entries up to position kc - 1), sorted as a pass leaves them; pass scores =
    s16.  -> cand int64 [nq, kc], scores float32 [nq, kc], qg int32 [nq]."""
    rows, groups, q, qg = image_world()
    s16 = reference("image", metric)["s16"]
    qg2 = ((qg + 1) % 36).astype(np.int32)
    cand = np.empty((len(q), kc), dtype=np.int64)
    for i in range(len(q)):
        order = np.argsort(-s16[i], kind="stable")
        out = groups[order] == qg2[i]
        cand[i] = np.concatenate([order[~out][:k], order[out][-(kc - k):]])
        assert (np.diff(s16[i, cand[i]]) <= 0).all()
    return cand, np.take_along_axis(s16, cand, axis=1).astype(np.float32), qg2


# ---- the restatement of the excluding re-rank -------------------------------------------------------------------------------------------
def rerank_expected(cand, pass_scores, groups, qg, k, rank_ids, rank_dist, s64, E, qn, ntotal, metric, id_base=0, variant=None):
    """What hb_index_exclude_rerank must return for the lists cand / pass_scores [nq, kc].
    rank_ids / rank_dist [nq, N]: the full chain ranking (chain_ranking); s64 [nq, N]: exact float64 scores; E, qn [nq].
    -> idx int64 [nq, k], dist float32 [nq, k], (must_be_1, must_be_0, in_band) bool [nq], have_kth bool [nq], kth_pos int64 [nq] (the position
    in rank_ids of the k-th allowed candidate, -1: none).
    variant: None, or one of the WRONG kernels tests/test_exclude_screen_cpu.py shows the restatement to catch (WRONG_KERNELS)."""
    cand = np.asarray(cand); pass_scores = np.asarray(pass_scores)
    nq, kc = cand.shape
    N = rank_ids.shape[1]
    missing = np.float32(np.inf if metric == 1 else -np.inf)
    ok = allowed_mask(cand, groups, qg) & (cand < ntotal)
    idx = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), missing, dtype=np.float32)
    kth64 = np.full(nq, -np.inf); have = np.zeros(nq, dtype=bool); kth_pos = np.full(nq, -1, dtype=np.int64)
    one = np.zeros(nq, dtype=bool); zero = np.zeros(nq, dtype=bool); band = np.zeros(nq, dtype=bool)
    for i in range(nq):
        rows_ok = cand[i][ok[i]]
        counted = cand[i][cand[i] >= 0] if variant == "excluded_counted" else rows_ok
        member = np.zeros(N, dtype=bool); member[rows_ok] = True
        pos = np.flatnonzero(member[rank_ids[i]])           # the allowed candidates in the fp32 search's order (a row listed twice counts once)
        take = pos[:k]
        idx[i, :len(take)] = rank_ids[i, take] + id_base
        dist[i, :len(take)] = rank_dist[i, take]
        full = cand[i, kc - 1] >= 0
        if variant == "not_full_after_exclusion":
            full = full and ok[i, kc - 1]
        if variant == "excluded_counted":                    # the rank k - 1 among ALL valid candidates
            cm = np.zeros(N, dtype=bool); cm[counted] = True
            cpos = np.flatnonzero(cm[rank_ids[i]])
            have[i] = len(cpos) >= k and bool(member[rank_ids[i, cpos[k - 1]]])      # (an excluded candidate at rank k - 1: "none" decides)
            if have[i]:
                kth_pos[i] = cpos[k - 1]
        else:
            have[i] = len(pos) >= k
            if have[i]:
                kth_pos[i] = pos[k - 1]
        if have[i]:
            kth64[i] = s64[i, rank_ids[i, kth_pos[i]]]
        if not full:
            c = ntotal < kc and qn[i] <= fr.F16_LIMIT
            one[i], zero[i] = c, not c
            continue
        if not have[i]:
            zero[i] = True
            continue
        last = float(pass_scores[i, kc - 1])
        if variant == "threshold_last_allowed":
            last = float(pass_scores[i, np.flatnonzero(ok[i])[-1]])
        o, z, b = fr.flag_band(kth64[i:i + 1], np.array([last]), E[i:i + 1], qn[i:i + 1])
        one[i], zero[i], band[i] = o[0], z[0], b[0]
    return idx, dist, (one, zero, band), have, kth_pos


def skip_cut_positions(cand, pass_scores, groups, qg, k, E, variant=None):
    """Which candidates the skip rule leaves unscored: position c > p_k with pass score < pass_scores[p_k] - 2 E, p_k = the list position of
    the k-th allowed candidate (none: nothing is skipped).  variant "cut_from_k_minus_1": the plain re-rank's rule, p_k = k - 1, which on a
    list with excluded entries ahead of k - 1 cuts candidates the answer needs.  -> bool [nq, kc]."""
    cand = np.asarray(cand); pass_scores = np.asarray(pass_scores)
    nq, kc = cand.shape
    ok = allowed_mask(cand, groups, qg)
    out = np.zeros((nq, kc), dtype=bool)
    for i in range(nq):
        if variant == "cut_from_k_minus_1":
            pk = k - 1 if cand[i, k - 1] >= 0 else -1
        else:
            p = np.flatnonzero(ok[i])
            pk = int(p[k - 1]) if len(p) >= k else -1
        if pk < 0 or not np.isfinite(E[i]):
            continue
        cut = np.float32(pass_scores[i, pk]) - np.float32(2.0) * np.float32(E[i])
        out[i] = (np.arange(kc) > pk) & (pass_scores[i] < cut)
    return out


WRONG_KERNELS = ("threshold_last_allowed", "excluded_counted", "cut_from_k_minus_1", "not_full_after_exclusion")
