"""References for excluding searches on the certified fp16 screen (csrc/hbird_exclude_screen.hip): the IMAGE WORLD, a bank whose queries find
their own image at the top of their lists; a host model of the route's three levels on it; and the numpy restatement of what the excluding
re-rank kernel (hb_index_exclude_rerank) must return for given candidate lists.  Plain numpy; nothing here knows of tiles, pools or waves.
tests/test_exclude_screen_gpu.py holds the kernel and the route to these; tests/test_exclude_screen_cpu.py pins the model's counts and shows
which wrong kernels the restatement catches.

Further down: the references of what a served excluding search leaves BEHIND its passes (HipFlatIndex.last_screen / last_screen_seeds /
last_exclusion_seeds) -- the chain of tests/f16_second_pass_refs.py with every k-th score taken over the allowed entries of the unmasked lists,
the gathered groups, and the hand-over to the rungs -- and the cases that reach its regimes (ECASES).  tests/test_exclude_seeds_gpu.py holds the
route to them, tests/test_exclude_seeds_cpu.py holds a host model to them and shows which wrong chains they catch.

The restatement, per query: the candidates that are ALLOWED (row >= 0, and not: query group >= 0, row inside the table, same group), ranked by
(exact score descending, row ascending); the first k are the answer, the tail is -1 / the missing value.  Certificate: the k-th allowed exact
score strictly above (pass score of the LAST list entry, allowed or not) + E; a full list with fewer than k allowed candidates is never
certified; a list that ends in -1 is certified when the bank holds fewer than kc rows.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import f16_centre_refs as CR
import f16_pass_refs as fr
import f16_second_pass_refs as SR

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


# ---- what a served excluding search leaves behind its passes --------------------------------------------------------------------------------
# The chain is that of f16_second_pass_refs.py (SR), and so are its checks: SR.check_seeds on the level-0 lists with the excluded entries
# struck (-1: kth0 is the k-th best chain score among the ALLOWED candidates), SR.check_level1 with the allowed entries handed in for kth1 --
# its list checks and its certificate rules read the unmasked lists, as the kernel does, and a k-th score of -inf (fewer than k allowed) pins
# the flag at 0 on both branches.  New here: the first certificates (rerank_expected's rule through flag_band), the gathered groups, the queries
# left to the rungs, and the answer.  Every value is a function of the previous stage's READ-OUT.
EXCL_NAMES = ("flag0_one", "flag0_zero", "groups1", "left", "n2", "answer_ids", "answer_bits")
# (the level-0 lists: the names of fr.check_float / fr.check_exact / fr.check_centred with this prefix -- check_level0_lists)
LISTS0 = "lists0_"
GROUP_ROWS = 150          # rows per group of the cases' tables: k + gmax = 180 > 128, the route serves the search
ECase = collections.namedtuple("ECase", "name base table metric")
# base: a case of SR.CASES (its world, k, metric, centred) or "image" (image_world, its own table); table: "block" (GROUP_ROWS consecutive
# rows), "interleaved" (row % G) or "edited" (block; every 7th row in no group, every 3rd query excludes nothing, query 1 names the group
# without rows).  qg[i]: the group of query i's best-scoring row.  Which regime each case reaches BY THE REFERENCE ALONE is recomputed and
# held by tests/test_exclude_seeds_cpu.py (REGIMES there).
ECASES = [
    ECase("rounding100", "rounding100", "block", None),
    ECase("rounding100-l2", "rounding100-l2", "interleaved", None),
    ECase("rounding300", "rounding300", "block", None),
    ECase("gather", "gather", "interleaved", None),
    ECase("tight-tokens", "tight-tokens", "block", None),
    ECase("one-failing", "one-failing", "interleaved", None),
    ECase("centred-clusters-neg", "centred-clusters-neg", "block", None),
    ECase("massive-128", "massive-128", "interleaved", None),
    ECase("exact", "exact", "block", None),
    ECase("exact-l2", "exact-l2", "interleaved", None),
    ECase("non-finite", "non-finite", "block", None),
    ECase("edited", "rounding100", "edited", None),
    ECase("image", "image", "own", 0),
    ECase("image-l2", "image", "own", 1),
]
ECASE = {c.name: c for c in ECASES}
_SRCASE = {c.name: c for c in SR.CASES}


@functools.lru_cache(maxsize=None)
def excl_case(name):
    """-> (c: the SR.Case the chain runs as, W: bank / queries [/ the exact world's fields], groups int32 [N], n_groups (one more than the table
    names: a group without rows), qg int32 [nq]); read-only."""
    ec = ECASE[name]
    if ec.base == "image":
        rows, groups, q, qg = image_world()
        c = SR.Case(name, "image", 64, 6000, 240, 30, ec.metric, False, ())
        return c, {"bank": rows, "queries": q}, groups, 37, qg
    c = _SRCASE[ec.base]
    W = SR.case_world(c)
    G = -(-c.N // GROUP_ROWS)
    groups = (np.arange(c.N) % G if ec.table == "interleaved" else np.arange(c.N) // GROUP_ROWS).astype(np.int32)
    b64 = W["bank"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = W["queries"].astype(np.float64) @ b64.T - (0.5 * (b64 * b64).sum(axis=1) if c.metric == 1 else 0.0)
    qg = groups[np.argmax(np.where(np.isfinite(s), s, -np.inf), axis=1)].astype(np.int32)
    if ec.table == "edited":
        groups[::7] = -1
        qg[::3] = -1
        qg[1] = G
    for arr in (groups, qg):
        arr.setflags(write=False)
    return c, W, groups, G + 1, qg


def bounds(q, bank, D, metric):
    """(qn, bmax, E [nq]) of the PLAIN pass: SR.plain_bounds with E by the library's own constants (fr.replay_bounds) wherever the norm is finite."""
    qn, bmax, E = SR.plain_bounds(q, bank, D, metric)
    E = np.array(E, np.float64)
    for i in np.flatnonzero(np.isfinite(qn)):
        E[i] = fr.replay_bounds(D, metric, float(qn[i]), bmax)[0]
    return qn, bmax, E


# What each case is there for -- a subset of what it reaches BY THE REFERENCE ALONE (tests/test_exclude_seeds_cpu.py recomputes it) and on the
# device (tests/test_exclude_seeds_gpu.py):
#   finite_seed        a second-pass query seeded from the k-th ALLOWED exact score
#   not_full_excluded  a second list that does not fill up, holds an excluded row and is certified by the seed rule
#   full_failing       a full second list with at least k allowed candidates that fails: to the rungs
#   fewer_than_k       a list with fewer than k allowed candidates (no seed; never certified)
#   all_excluded       a full second list of 256 excluded rows
#   n1_one / n1_many   one second-pass query / more than 256 (two query tiles of the second pass)
#   centred            the centred form;  centred_neg: with c_q < 0 and seeded second-pass queries
#   exact              an exact world with twins in the second lists (list bits)
#   non_finite         a NaN query and one beyond the fp16 range: no seed, through both levels to the rungs
#   no_group           queries that exclude nothing, a group without rows, rows in no group
REGIMES = {
    "rounding100": ("finite_seed", "not_full_excluded", "block", "dot"),
    "rounding100-l2": ("finite_seed", "not_full_excluded", "interleaved", "l2"),
    "rounding300": ("finite_seed", "full_failing", "block"),
    "gather": ("finite_seed", "full_failing", "interleaved"),
    "tight-tokens": ("n1_many", "full_failing"),
    "one-failing": ("n1_one", "not_full_excluded"),
    "centred-clusters-neg": ("centred", "centred_neg", "finite_seed", "not_full_excluded", "fewer_than_k"),
    "massive-128": ("centred",),
    "exact": ("exact",),
    "exact-l2": ("exact", "l2"),
    "non-finite": ("non_finite",),
    "edited": ("no_group", "finite_seed"),
    "image": ("fewer_than_k", "all_excluded"),
    "image-l2": ("fewer_than_k", "all_excluded", "l2"),
}
ALL_REGIMES = {"finite_seed", "not_full_excluded", "full_failing", "fewer_than_k", "all_excluded", "n1_one", "n1_many", "centred", "centred_neg", "exact",
               "non_finite", "no_group", "block", "interleaved", "dot", "l2"}


def regimes_reached(name, S, left, fig, cq, E):
    """The regimes a chain reached, from its read-out S, the queries left to the rungs and check_excl_chain's figures (cq / E: the centred
    pass' c_q and bound, or None) -> set.  The same rule for the host model and for the device."""
    c, W, groups, n_groups, qg = excl_case(name)
    table = ECASE[name].table
    out = {"block" if table in ("block", "edited") else table, "l2" if c.metric else "dot"}
    flags = {"finite_seed": fig["finite_seeds"] > 0, "not_full_excluded": fig["not_full_certified_with_excluded"] > 0,
             "full_failing": fig["full_failing_k_allowed"] > 0 and len(left) > 0, "fewer_than_k": fig["fewer_than_k0"] > 0,
             "all_excluded": fig["full_all_excluded"] > 0, "n1_one": S["n1"] == 1, "n1_many": S["n1"] > 256,
             "centred": c.centred and bool(np.isfinite(S["floor0"]).any()),
             "centred_neg": c.centred and cq is not None and fig["finite_seeds"] > 0 and bool((cq < -100 * E).all()),
             "exact": c.world == "exact" and S["n1"] > 0 and bool(W["dup"][S["rows1"][S["rows1"] >= 0]].any()),
             "non_finite": c.world == "nonfinite" and S["n1"] > 0 and bool(np.isin([7, 23], left).all()) and bool(np.isneginf(S["kth0"][[7, 23]]).all())
                           and bool(np.isneginf(S["seed1"][np.searchsorted(S["queries1"], [7, 23])]).all()),
             "no_group": bool((qg == -1).any() and (groups == -1).any() and (qg == n_groups - 1).any())}
    return out | {n for n, v in flags.items() if v}


def check_level0_lists(rows, scores, q, bank, metric, k, exact=None, centre_info=None):
    """The level-0 lists and pass scores of a served excluding search, which know nothing of groups: H1 / H2 as fr.check_float has them on a
    float world (over the queries with finite fp16 operands), fr.check_exact's bits on an exact world, fr.check_centred's H1 / H2 for the
    centred pass (centre_info: fp16_centre_info(), or the same fields of SR.centred_pass).  No flags: the excluding certificates are
    check_excl_chain's.  -> ({LISTS0 + name: message}, figures)."""
    kc = rows.shape[1]
    if exact is not None:
        bad, fig = fr.check_exact(rows, scores, exact, metric, kc), {}
    elif centre_info is not None:
        bad, fig = fr.check_centred(rows, scores, None, q, bank, metric, k, kc, centre_info)
    else:
        fin = SR.query_norms(q) <= fr.F16_LIMIT
        bad, fig = fr.check_float(rows[fin], scores[fin], None, fr.float_reference(np.asarray(q, np.float32)[fin], bank, metric), k, kc)
    return {LISTS0 + n: f"{LISTS0}{n}: {m}" for n, m in bad.items()}, {LISTS0 + n: v for n, v in fig.items()}


def check_excl_chain(S, L0, X1, stats, groups, qg, q, bank, metric, k, E, ref=None, exact=None, cq=None, skip=None):
    """Everything a served excluding search left -> ({name: message}, figures).  S: last_screen_seeds(); L0: last_screen() of the same search run
    WITHOUT its second pass (the level-0 lists; a dict with rows / scores / certified); X1: last_exclusion_seeds(); stats: last_exclusion_screen()
    or None; groups [N] / qg [nq]: the table and the queries' groups; the rest as SR.check_seeds / SR.check_level1 take it.
    Names: SR.SEED_NAMES, SR.LEVEL1_NAMES, EXCL_NAMES (answers: check_answer)."""
    nq, N = S["nq"], bank.shape[0]
    rows0, kc0 = L0["rows"], L0["rows"].shape[1]
    ok0 = allowed_mask(rows0, groups, qg)
    bad, fig = SR.check_seeds(S, np.where(ok0, rows0, -1), L0["certified"], q, bank, metric, k, E, cq)
    # the first certificates, from both sides outside the 0.1 % band, as a function of the read-out kth0 (held on bits above) and the list
    qn = SR.query_norms(q)
    add = cq.astype(np.float64) if cq is not None else 0.0
    full0 = rows0[:, kc0 - 1] >= 0
    with np.errstate(invalid="ignore"):
        thr = L0["scores"][:, kc0 - 1].astype(np.float64) + add
        one, zero, band = fr.flag_band(S["kth0"].astype(np.float64), thr, E, qn)
        nonfin = ~(qn <= fr.F16_LIMIT) | ~np.isfinite(E) | ~np.isfinite(thr)
    one, zero = one & ~nonfin & full0, zero | nonfin | ~full0 | (ok0.sum(axis=1) < k)       # (N >= kc0: a list that is not full has lost rows)
    one &= ~zero
    assert N >= kc0
    fig["band_share0"] = float((~one & ~zero).mean())
    f0 = S["certified0"].astype(bool)
    if (one & ~f0).any():
        i = int(np.flatnonzero(one & ~f0)[0])
        SR._note(bad, "flag0_one", f"query {i} ({int(ok0[i].sum())} allowed of {kc0}): not certified although its k-th allowed exact score lies {(S['kth0'][i] - thr[i]) / E[i]:.4f} E above the last pass score")
    if (zero & f0).any():
        i = int(np.flatnonzero(zero & f0)[0])
        SR._note(bad, "flag0_zero", f"query {i} ({int(ok0[i].sum())} allowed of {kc0}, list {'full' if full0[i] else 'not full'}): certified although its k-th allowed exact score ({S['kth0'][i]!r}) lies {(S['kth0'][i] - thr[i]) / E[i]:.4f} E above the last pass score")
    # the gather of the groups, and the second pass with the groups AS GATHERED
    n1 = S["n1"]
    g1 = np.asarray(X1["groups1"])
    want_g1 = np.asarray(qg)[S["queries1"]] if n1 else np.zeros(0, np.int32)
    if g1.shape != want_g1.shape or (g1 != want_g1).any():
        j = 0 if g1.shape != want_g1.shape else int(np.flatnonzero(g1 != want_g1)[0])
        SR._note(bad, "groups1", f"{g1.size} groups gathered for {n1} second-pass queries; second-pass query {j}" + (f" (query {S['queries1'][j]}) got group {g1[j]}, its own is {want_g1[j]}" if g1.shape == want_g1.shape else ""))
    ok1 = allowed_mask(S["rows1"], groups, g1 if g1.shape == want_g1.shape else want_g1) if n1 else np.zeros((0, SR.KC1), bool)
    bad1, fig1 = SR.check_level1(S, q, bank, metric, k, E, ref=ref, exact=exact, cq=cq, skip=skip, allowed=ok1)
    bad.update({n: m for n, m in bad1.items() if n not in bad})
    fig.update(fig1)
    # the hand-over to the rungs
    want_left = S["queries1"][S["certified1"] == 0] if n1 else np.flatnonzero(S["certified0"] == 0)
    left = np.asarray(X1["left"])
    if left.shape != want_left.shape or (left != want_left).any():
        SR._note(bad, "left", f"{left[:8]} ... ({left.size}) handed to the rungs, the last certificates failed for {want_left[:8]} ... ({want_left.size})")
    if S["n2"] != left.size or (stats is not None and stats["rung_queries"] != left.size):
        SR._note(bad, "n2", f"n2 = {S['n2']}, rung_queries = {None if stats is None else stats['rung_queries']}, {left.size} queries named")
    n_have = (S["rows1"] >= 0).sum(axis=1) if n1 else np.zeros(0, int)
    fig.update(n1=int(n1), n_left=int(left.size), excluded0=[int((~ok0 & (rows0 >= 0)).sum(axis=1).min()), int((~ok0 & (rows0 >= 0)).sum(axis=1).max())],
               fewer_than_k0=int((ok0.sum(axis=1) < k).sum()), finite_seeds=int(np.isfinite(S["seed1"]).sum()),
               not_full_certified_with_excluded=int(((n_have < SR.KC1) & (S["certified1"] == 1) & ((~ok1) & (S["rows1"] >= 0)).any(axis=1)).sum()) if n1 else 0,
               full_failing_k_allowed=int(((n_have == SR.KC1) & (S["certified1"] == 0) & (ok1.sum(axis=1) >= k)).sum()) if n1 else 0,
               full_all_excluded=int(((n_have == SR.KC1) & (ok1.sum(axis=1) == 0)).sum()) if n1 else 0,
               not_full_rows=[int(n_have[n_have < SR.KC1].min()), int(n_have[n_have < SR.KC1].max())] if (n_have < SR.KC1).any() else [],
               rule_margin_over_E=_rule_margins(S, n_have, E, cq) if n1 else [])
    return bad, fig


def _rule_margins(S, n_have, E, cq):
    """[min, max] over the second-pass queries with a finite k-th score of (kth1 [- c_q] - threshold) / E, the threshold being the last pass
    score of a full list and the seed of one that did not fill up: the certificates' distance from their decision."""
    Q1 = S["queries1"]
    add = cq[Q1].astype(np.float64) if cq is not None else 0.0
    thr = np.where(n_have == SR.KC1, S["scores1"][:, SR.KC1 - 1].astype(np.float64), S["seed1"].astype(np.float64))
    with np.errstate(invalid="ignore"):
        m = (S["kth1"].astype(np.float64) - add - thr) / E[Q1] - 1.0
    m = m[np.isfinite(m)]
    return [float(m.min()), float(m.max())] if m.size else []


def allowed_ranking(rank_ids, rank_dist, groups, qg, k, metric):
    """The fp32 chain ranking (oracle.knn_chain_f32 at k + gmax or more) restricted to the allowed rows -> idx int64 [nq, k], dist float32 [nq, k]."""
    nq = rank_ids.shape[0]
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf if metric == 1 else -np.inf, np.float32)
    g = np.asarray(groups)
    for i in range(nq):
        keep = np.flatnonzero((rank_ids[i] >= 0) & ~((qg[i] >= 0) & (g[np.maximum(rank_ids[i], 0)] == qg[i])))[:k]
        idx[i, :keep.size], dist[i, :keep.size] = rank_ids[i, keep], rank_dist[i, keep]
    return idx, dist


def check_answer(got_idx, got_dist, want_idx, want_dist, which=None, what=""):
    """ids and distance bits of the answer over the queries `which` (all) -> {name: message}"""
    bad = {}
    w = np.ones(len(got_idx), bool) if which is None else which
    m = w & (got_idx != want_idx).any(axis=1)
    if m.any():
        i = int(np.flatnonzero(m)[0]); c = int(np.flatnonzero(got_idx[i] != want_idx[i])[0])
        SR._note(bad, "answer_ids", f"{what}query {i}: neighbour {c} is row {got_idx[i, c]}, the fp32 chain ranking of the allowed rows has {want_idx[i, c]}")
    m = w & ~CR.same_bits(got_dist, want_dist).all(axis=1) & ~m
    if m.any():
        i = int(np.flatnonzero(m)[0]); c = int(np.flatnonzero(~CR.same_bits(got_dist[i], want_dist[i]))[0])
        SR._note(bad, "answer_bits", f"{what}query {i}: neighbour {c} (row {got_idx[i, c]}) at distance {got_dist[i, c]!r}, the chain gives {want_dist[i, c]!r}")
    return bad
