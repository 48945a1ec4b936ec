"""References for the OUTPUT of the fp16 candidate pass (csrc/hbird_knn_f16.hip: knn_f16v2_kernel + the merge of its pools), which
HipFlatIndex.last_screen() reads out: per query the k' candidate rows and the kernel's own scores, and the first certificates.  Plain numpy;
nothing here knows of tiles, pools, slots or phases.  tests/test_f16_candidates_gpu.py holds the kernel to these, and
tests/test_f16_candidates_cpu.py holds these to what they promise and shows on the host which wrong kernels they catch.

The certificate of the screen rests on two statements about the pass:
    H1  every candidate's pass score is within E of its exact score;
    H2  every row outside a query's k' candidates has a pass score no greater than the k'-th candidate's.

EXACT worlds: integer components in [-3, 3] (optionally times 2^-5), D <= 1024.  Every operand is an fp16 number, every product an integer
(times 2^-10), every partial sum of a row -- in ANY order, the L2 row init -|b|^2 / 2 included -- a multiple of 1/2 below 2^15 in magnitude
(9 x 1024 x 1.5 = 13,824), hence an fp32 number: whatever the MFMA's summation order, the pass score of every row is determined to the bit,
and so are the lists: the k' best by (score descending, row ascending).

FLOAT worlds: the pass score is compared with s16, the float64 sum of the products of the fp16 images plus the fp32 row init, within the
ACCUMULATION share A of the certificate's bound E (hbird_certificate.h):
    E = R + A + S + 1e-30,   R = qn bmax 1.05/1024            both operands rounded to fp16
                             A = qn bmax D 2.4e-7 [+ L2: D 1.2e-7 0.5 bmax^2]      fp32 accumulation (and the row init in the sums)
                             S = (qn + bmax) sqrt(D) 6e-8      fp16 subnormal inputs
A_r: A with the norm of row r in place of bmax -- what bounds the accumulation error of THAT row's sum.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import f16_screen_worlds as fw

F16_LIMIT = 65504.0


def kc_of(k):
    """k' of the first candidate pass (hb_knn_plan_shape)."""
    return min(256, max(64, (2 * k + 7) // 8 * 8))


def klw_of(kc):
    """Pool capacity per query and slot (hb_knn_plan_shape)."""
    return min(512, (max(2 * kc, kc + 128) + 63) // 64 * 64)


# ---- exact worlds ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_world(N, D, nq, kc, seed, scale_log2=0, dup_share=0.45):
    """-> dict: bank [N, D], queries [nq, D] float32 with components in {-3..3} x 2^scale_log2; bank_i / queries_i the integers (int64);
    `heavy`: the rows of the planted tie group (min(N, kc + 40) copies of one row with every component +-3, spread over the whole bank:
    query 0 IS that row, so for it these rows share the best score of the bank under both metrics -- kc + 40 of them where N >= 2 kc + 80);
    dup: bool [N], the row has a bit-identical twin."""
    assert D <= 1024 and scale_log2 in (0, -5)
    rng = np.random.default_rng([seed, N, D, nq])
    bank = rng.integers(-3, 4, size=(N, D), dtype=np.int64)
    q = rng.integers(-3, 4, size=(nq, D), dtype=np.int64)
    # copies: dup_share of the rows take the values of an ORIGINAL row anywhere in the bank (so copies straddle every boundary a kernel has)
    n_dup = int(np.ceil(dup_share * N))
    perm = rng.permutation(N)
    dst, orig = perm[:n_dup], perm[n_dup:]
    bank[dst] = bank[orig[rng.integers(0, orig.size, n_dup)]]
    # the planted tie group: more than kc rows tied at the best score of query 0, wherever the bank has room for them beside other rows
    proto = 3 * rng.choice([-1, 1], D).astype(np.int64)
    n_heavy = kc + 40 if N >= 2 * kc + 80 else N // 3
    heavy = np.sort(rng.choice(N, n_heavy, replace=False))
    bank[heavy] = proto
    q[0] = proto
    _, inv, cnt = np.unique(bank, axis=0, return_inverse=True, return_counts=True)
    dup = cnt[inv.reshape(-1)] > 1
    sc = np.float32(2.0 ** scale_log2)
    return {"bank": (bank.astype(np.float32) * sc), "queries": (q.astype(np.float32) * sc), "bank_i": bank, "queries_i": q, "heavy": heavy, "dup": dup,
            "scale_log2": scale_log2, "N": N, "D": D, "nq": nq}


def exact_scores2(W, metric):
    """TWICE the pass score of every (query, row) in units of 4^scale, as int64 [nq, N]: 2 q.b [- |b|^2].  (float64 matmul of small integers
    is exact: every entry is below 2^15.)"""
    qi, bi = W["queries_i"].astype(np.float64), W["bank_i"].astype(np.float64)
    s2 = 2.0 * (qi @ bi.T)
    if metric == 1:
        s2 -= (bi * bi).sum(axis=1)[None, :]
    out = s2.astype(np.int64)
    assert np.array_equal(out.astype(np.float64), s2)
    return out


def exact_lists(W, metric, kc):
    """-> rows int64 [nq, kc] (-1 at the tail when N < kc), scores float32 [nq, kc] (-inf there): the kc best by (score desc, row asc)."""
    if ("lists", metric, kc) in W:      # (computed once per world: the GPU cases and the host mutations share it)
        return W[("lists", metric, kc)]
    s2 = exact_scores2(W, metric)
    nq, N = s2.shape
    rows = np.full((nq, kc), -1, dtype=np.int64)
    scores = np.full((nq, kc), -np.inf, dtype=np.float32)
    unit = 0.5 * 4.0 ** W["scale_log2"]
    n = min(N, kc)
    for i in range(nq):
        order = np.lexsort((np.arange(N), -s2[i]))[:n]
        rows[i, :n] = order
        v = s2[i, order].astype(np.float64) * unit
        scores[i, :n] = v.astype(np.float32)
        assert np.array_equal(scores[i, :n].astype(np.float64), v), "an exact world's score must be an fp32 number"
    W[("lists", metric, kc)] = (rows, scores, s2)
    return rows, scores, s2


def check_exact(got_rows, got_scores, W, metric, kc):
    """The assertions of the exact worlds -> {name: message}: EMPTY when the lists are right.  Names (what tests/test_f16_candidates_cpu.py records):
    rows, score_bits, tail, no_repeats, sorted, low_ids_on_ties."""
    ref_rows, ref_scores, s2 = exact_lists(W, metric, kc)
    nq, N = s2.shape
    bad = {}

    def note(name, msg):
        bad.setdefault(name, msg)
    unit = 0.5 * 4.0 ** W["scale_log2"]
    for i in range(nq):
        r, s = got_rows[i], got_scores[i]
        n = min(N, kc)
        # -1 with -inf only at the tail, and only when the bank has fewer than kc rows
        if not ((r[:n] >= 0).all() and (r[n:] == -1).all() and np.isneginf(s[n:]).all() and np.isfinite(s[:n]).all() and (r < N).all()):
            note("tail", f"query {i}: missing entries {np.nonzero(r < 0)[0][:4]} of {kc} with {N} rows in the bank")
            continue
        rv = r[:n]
        if np.unique(rv).size != n:
            note("no_repeats", f"query {i}: a row appears twice")
        sv = s[:n].astype(np.float64)
        if not ((sv[:-1] > sv[1:]) | ((sv[:-1] == sv[1:]) & (rv[:-1] < rv[1:]))).all():
            note("sorted", f"query {i}: the list is not sorted by (score descending, row ascending) at {np.nonzero(~((sv[:-1] > sv[1:]) | ((sv[:-1] == sv[1:]) & (rv[:-1] < rv[1:]))))[0][:4]}")
        # among the rows tied with the kc-th score (by the REFERENCE's scores), the lowest ids are present
        last2 = s2[i, ref_rows[i, n - 1]]
        tied = np.nonzero(s2[i] == last2)[0]
        n_in = int((s2[i, ref_rows[i, :n]] == last2).sum())
        if not np.isin(tied[:n_in], rv).all():
            note("low_ids_on_ties", f"query {i}: of the {tied.size} rows tied at rank {kc} the {n_in} lowest ids belong to the list; missing {tied[:n_in][~np.isin(tied[:n_in], rv)][:4]}")
        if not np.array_equal(rv, ref_rows[i, :n]):
            j = int(np.nonzero(rv != ref_rows[i, :n])[0][0])
            note("rows", f"query {i}: candidate {j} is row {rv[j]} (score x2 {s2[i, rv[j]]}), the reference has row {ref_rows[i, j]} (score x2 {s2[i, ref_rows[i, j]]})")
        want = (s2[i, rv].astype(np.float64) * unit).astype(np.float32)       # the score of the row the kernel NAMES: a wrong row with its right score fails `rows` only
        if not np.array_equal(s[:n].view(np.uint32), want.view(np.uint32)):
            j = int(np.nonzero(s[:n].view(np.uint32) != want.view(np.uint32))[0][0])
            note("score_bits", f"query {i}: candidate {j} (row {rv[j]}, bank tile {rv[j] // 256}) has pass score {s[j]!r}, exactly {want[j]!r}")
    return bad


# ---- float worlds ----------------------------------------------------------------------------------------------------------------------------
def replay_bounds(D, metric, qn, bmax, qcn=0.0, cmax=0.0, mun=0.0, t=0.0):
    """(E, E') of hb_certificate_bound_replay: the shipped constants in float, as the re-rank kernels compile them."""
    from hbird_mi import _lib
    a = (ctypes.c_double * 8)(D, metric, qn, bmax, qcn, cmax, mun, t)
    o = (ctypes.c_double * 2)()
    assert _lib.lib().hb_certificate_bound_replay(a, 8, o, 2) == 0
    return o[0], o[1]


def shares(qn, bnorm, D, metric):
    """(R, A, S) of E as written in hbird_certificate.h, float64; bnorm: bmax, or the rows' norms for A_r (broadcasts against qn)."""
    R = qn * bnorm * (1.05 / 1024.0)
    A = qn * bnorm * D * 2.4e-7 + (D * 1.2e-7 * 0.5 * bnorm * bnorm if metric == 1 else 0.0)
    S = (qn + bnorm) * np.sqrt(float(D)) * 6e-8
    return R, A, S


def float_reference(q, bank, metric):
    """-> dict: s16 [nq, N] (float64 sum of the products of the fp16 images + the fp32 row init), s [nq, N] (the exact float64 score of the
    fp32 values), qn [nq], bn [N], bmax, E [nq] (the shipped constants), R / A / S [nq] with R + A + S + 1e-30 = E up to float rounding."""
    q = np.ascontiguousarray(q, dtype=np.float32); bank = np.ascontiguousarray(bank, dtype=np.float32)
    nq, D = q.shape
    q64, b64 = q.astype(np.float64), bank.astype(np.float64)
    q16, b16 = q.astype(np.float16).astype(np.float64), bank.astype(np.float16).astype(np.float64)
    assert np.isfinite(q16).all() and np.isfinite(b16).all()
    init = -0.5 * (b64 * b64).sum(axis=1) if metric == 1 else np.zeros(bank.shape[0])
    init32 = init.astype(np.float32).astype(np.float64)
    s = q64 @ b64.T + init[None, :]
    s16 = q16 @ b16.T + init32[None, :]
    qn, bn = np.sqrt((q64 * q64).sum(axis=1)), np.sqrt((b64 * b64).sum(axis=1))
    bmax = float(bn.max())
    E = np.array([replay_bounds(D, metric, float(x), bmax)[0] for x in qn])
    R, A, S = shares(qn, bmax, D, metric)
    return {"s16": s16, "s": s, "qn": qn, "bn": bn, "bmax": bmax, "E": E, "R": R, "A": A, "S": S, "D": D, "metric": metric}


def reference_candidates(score, kc):
    """rows [nq, kc] of the kc best of every query by (score desc, row asc)."""
    return np.argsort(-score, axis=1, kind="stable")[:, :kc]


def kth_best(vals, k):
    """the k-th largest of every row of vals [nq, n]"""
    return -np.sort(-vals, axis=1)[:, k - 1]


def flag_band(kth64, pass_last, E, qn):
    """The certificate decision the reference can pin -> (must_be_1, must_be_0, in_band), bool [nq].  A query whose norm exceeds the fp16 range
    fails by the certificate's own precondition (hbird_rerank_dev.h: finite operands); within 1e-6 of that limit nothing is pinned."""
    over = qn > F16_LIMIT * (1.0 + 1e-6)
    near = (np.abs(qn - F16_LIMIT) <= F16_LIMIT * 1e-6)
    one = (kth64 > pass_last + 1.001 * E) & ~over & ~near
    zero = (kth64 < pass_last + 0.999 * E) | over
    band = ~one & ~zero
    return one, zero, band


def reference_band_share(ref, k, kc):
    """Share of the queries inside the 0.1 % band by the reference alone: s16's candidates, their exact k-th best, s16's kc-th score."""
    cand = reference_candidates(ref["s16"], kc)
    kth64 = kth_best(np.take_along_axis(ref["s"], cand, axis=1), k)
    last = np.take_along_axis(ref["s16"], cand[:, kc - 1:kc], axis=1)[:, 0]
    return float(flag_band(kth64, last, ref["E"], ref["qn"])[2].mean())


def check_float(got_rows, got_scores, got_flags, ref, k, kc, subnormal=False):
    """The assertions of the float worlds -> ({name: message}, figures).  Names: valid, sorted, accumulation (|pass - s16| <= A [+ S]), H1
    (|pass - s| <= E), H2 (outside rows: s16[r] <= pass[kc-1] + A_r), clear_candidates (reference candidates more than 2 A above the
    reference's kc-th are in the list), flag_one / flag_zero (the certificate decision outside the 0.1 % band), band_cap (at most 1 % inside).
    got_flags may be None (no decision to check).  figures: max |pass - s16| / A, max |pass - s| / E, band share."""
    s16, s, E, A, S, qn, bn = ref["s16"], ref["s"], ref["E"], ref["A"], ref["S"], ref["qn"], ref["bn"]
    nq, N = s16.shape
    assert N >= kc
    bad = {}

    def note(name, msg):
        bad.setdefault(name, msg)
    tolA = A + S if subnormal else A
    fig = {"acc_over_A": 0.0, "err_over_E": 0.0, "band_share": 0.0}
    ok_rows = (got_rows >= 0).all() and (got_rows < N).all() and np.isfinite(got_scores).all()
    if not ok_rows:
        i = int(np.nonzero(((got_rows < 0) | (got_rows >= N) | ~np.isfinite(got_scores)).any(axis=1))[0][0])
        note("valid", f"query {i}: a missing entry, a row outside the bank or a non-finite pass score in a bank of {N} >= {kc} rows")
        return bad, fig
    srt = np.sort(got_rows, axis=1)
    if (srt[:, 1:] == srt[:, :-1]).any():
        note("valid", f"query {int(np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0][0])}: a row appears twice")
        return bad, fig
    p = got_scores.astype(np.float64)
    ordered = (p[:, :-1] > p[:, 1:]) | ((p[:, :-1] == p[:, 1:]) & (got_rows[:, :-1] < got_rows[:, 1:]))
    if not ordered.all():
        i, j = [int(v[0]) for v in np.nonzero(~ordered)]
        note("sorted", f"query {i}: the list is not sorted by (pass score descending, row ascending) at {j}")
    c16 = np.take_along_axis(s16, got_rows, axis=1)
    cs = np.take_along_axis(s, got_rows, axis=1)
    acc = np.abs(p - c16) / tolA[:, None]
    fig["acc_over_A"] = float((np.abs(p - c16) / A[:, None]).max())
    if (acc > 1.0).any():
        i, j = np.unravel_index(np.argmax(acc), acc.shape)
        note("accumulation", f"query {i} candidate {j} (row {got_rows[i, j]}, bank tile {got_rows[i, j] // 256}): |pass - s16| = {abs(p[i, j] - c16[i, j]):.4g} = {acc[i, j]:.3f} x the allowance")
    h1 = np.abs(p - cs) / E[:, None]
    fig["err_over_E"] = float(h1.max())
    if (h1 > 1.0).any():
        i, j = np.unravel_index(np.argmax(h1), h1.shape)
        note("H1", f"query {i} candidate {j} (row {got_rows[i, j]}, bank tile {got_rows[i, j] // 256}): |pass - s| = {h1[i, j]:.3f} E")
    last = p[:, kc - 1]
    inside = np.zeros((nq, N), bool)
    np.put_along_axis(inside, got_rows, True, axis=1)
    _, A_r, _ = shares(qn[:, None], bn[None, :], ref["D"], ref["metric"])
    lim = last[:, None] + A_r + (S[:, None] if subnormal else 0.0)
    over = ~inside & (s16 > lim)
    if over.any():
        i, r = [int(v[0]) for v in np.nonzero(over)]
        note("H2", f"query {i}: row {r} (bank tile {r // 256}) is no candidate, its s16 {s16[i, r]:.9g} exceeds the kc-th pass score {last[i]:.9g} by {(s16[i, r] - last[i]) / A_r[i, r]:.3f} A_r")
    ref_c = reference_candidates(s16, kc)
    rc16 = np.take_along_axis(s16, ref_c, axis=1)
    clear = rc16 > (rc16[:, kc - 1] + 2.0 * tolA)[:, None]
    lost = clear & ~np.take_along_axis(inside, ref_c, axis=1)
    if lost.any():
        i, j = [int(v[0]) for v in np.nonzero(lost)]
        note("clear_candidates", f"query {i}: row {ref_c[i, j]} (bank tile {ref_c[i, j] // 256}), rank {j} by s16 and {(rc16[i, j] - rc16[i, kc - 1]) / tolA[i]:.2f} A above rank {kc}, is no candidate")
    if got_flags is not None:
        kth64 = kth_best(cs, k)
        one, zero, band = flag_band(kth64, last, E, qn)
        fig["band_share"] = float(band.mean())
        f = np.asarray(got_flags).astype(bool)
        if (one & ~f).any():
            i = int(np.nonzero(one & ~f)[0][0])
            note("flag_one", f"query {i}: not certified although its exact k-th best lies {(kth64[i] - last[i]) / E[i]:.4f} E above the kc-th pass score")
        if (zero & f).any():
            i = int(np.nonzero(zero & f)[0][0])
            note("flag_zero", f"query {i}: certified although its exact k-th best lies {(kth64[i] - last[i]) / E[i]:.4f} E above the kc-th pass score (||q|| = {qn[i]:.6g})")
        if band.mean() > 0.01:
            note("band_cap", f"{band.mean():.4f} of the queries lie inside the 0.1 % band")
    return bad, fig


def model_lists(score, kc, dtype=np.float32):
    """What a RIGHT pass would leave for the scores `score` [nq, N]: rows and fp32 scores of the kc best by (score desc, row asc)."""
    sc = score.astype(dtype)
    rows = np.empty((sc.shape[0], kc), dtype=np.int64)
    for i in range(sc.shape[0]):
        rows[i] = np.lexsort((np.arange(sc.shape[1]), -sc[i]))[:kc]
    return rows, np.take_along_axis(sc, rows, axis=1)


# ---- the float worlds of the GPU cases ---------------------------------------------------------------------------------------------------------
def normal_world(N, D, nq, seed=0, normalised=True):
    rng = np.random.default_rng([seed, 20])
    bank = rng.standard_normal((N, D), dtype=np.float32)
    q = rng.standard_normal((nq, D), dtype=np.float32)
    if normalised:
        bank /= np.sqrt(np.einsum("ij,ij->i", bank, bank))[:, None]
        q *= np.float32(3.0) / np.sqrt(np.einsum("ij,ij->i", q, q))[:, None]
    return {"bank": bank, "queries": q}


@functools.lru_cache(maxsize=None)
def float_world(name, N, D, nq, k, metric, seed=0):
    """One of the float worlds by name -> dict bank, queries.  rounding: fw.rounding_world with 10 planted groups, the rest background."""
    kc = kc_of(k)
    if name == "rounding":
        n_decoys = kc + 44
        W = fw.rounding_world(D, k, kc, 10, n_decoys, (0.5, 0.7, 0.8, 0.9, 0.95), metric=metric, seed=seed, n_background=N - 10 * n_decoys - 19,      # (a group has n_decoys + h rows, h = 1, 2, 3, 1, ...)
                              n_queries_background=nq - 10)
    elif name == "normal":
        W = normal_world(N, D, nq, seed, True)
    elif name == "normal_raw":
        W = normal_world(N, D, nq, seed, False)
    else:
        W = fw.VIT_WORLDS[name](N, D, nq, seed=seed)
    assert W["bank"].shape == (N, D) and W["queries"].shape == (nq, D)
    return W


@functools.lru_cache(maxsize=None)
def float_world_reference(name, N, D, nq, k, metric, seed=0):
    W = float_world(name, N, D, nq, k, metric, seed)
    return float_reference(W["queries"], W["bank"], metric)


# ---- the centred form ------------------------------------------------------------------------------------------------------------------------
def check_centred(got_rows, got_scores, got_flags, q, bank, metric, k, kc, info):
    """H1 / H2 / the flags of the CENTRED pass, in the form the re-rank uses (hbird_rerank_dev.h): with mu the bank's column mean (float64,
    here), t / cmax / ||mu|| from fp16_centre_info() and E' from the shipped constants:
        |pass + q.mu - s| <= E' for candidates,   s[r] <= pass[kc-1] + q.mu + E' for outside rows,
    and the certificate decision outside its 0.1 % band (got_flags None: the lists only).  No bits, no A-level tolerance: one ulp of mu between this mean and the library's
    is 2^-14 of E'.  -> ({name: message}, figures)."""
    q64, b64 = np.asarray(q, np.float64), np.asarray(bank, np.float64)
    nq, D = q64.shape
    N = b64.shape[0]
    mu = b64.mean(axis=0)
    init = -0.5 * (b64 * b64).sum(axis=1) if metric == 1 else np.zeros(N)
    s = q64 @ b64.T + init[None, :]
    cq = q64 @ mu
    qn, bmax = np.sqrt((q64 * q64).sum(axis=1)), float(np.sqrt((b64 * b64).sum(axis=1)).max())
    qcn = np.sqrt(((q64 - info["t"] * mu[None, :]) ** 2).sum(axis=1))
    E = np.array([replay_bounds(D, metric, float(qn[i]), bmax, float(qcn[i]), info["cmax"], info["mu_norm"], info["t"])[1] for i in range(nq)])
    bad = {}

    def note(name, msg):
        bad.setdefault(name, msg)
    fig = {"err_over_E": 0.0, "band_share": 0.0, "E_centred_over_E_plain": float(np.median(E / np.array([replay_bounds(D, metric, float(x), bmax)[0] for x in qn])))}
    if not ((got_rows >= 0).all() and (got_rows < N).all() and np.isfinite(got_scores).all()):
        note("valid", "a missing entry or a non-finite pass score")
        return bad, fig
    srt = np.sort(got_rows, axis=1)
    if (srt[:, 1:] == srt[:, :-1]).any():
        note("valid", "a row appears twice")
        return bad, fig
    p = got_scores.astype(np.float64) + cq[:, None]
    cs = np.take_along_axis(s, got_rows, axis=1)
    h1 = np.abs(p - cs) / E[:, None]
    fig["err_over_E"] = float(h1.max())
    if (h1 > 1.0).any():
        i, j = np.unravel_index(np.argmax(h1), h1.shape)
        note("H1", f"query {i} candidate {j} (row {got_rows[i, j]}): |pass + q.mu - s| = {h1[i, j]:.3f} E'")
    last = p[:, kc - 1]
    inside = np.zeros((nq, N), bool)
    np.put_along_axis(inside, got_rows, True, axis=1)
    over = ~inside & (s > (last + E)[:, None])
    if over.any():
        i, r = [int(v[0]) for v in np.nonzero(over)]
        note("H2", f"query {i}: row {r} is no candidate, its exact score exceeds the kc-th pass score + q.mu by {(s[i, r] - last[i]) / E[i]:.3f} E'")
    if got_flags is None:      # (no decision to check: the lists of an excluding search, tests/excl_screen_refs.py)
        return bad, fig
    kth64 = kth_best(cs, k)
    one, zero, band = flag_band(kth64, last, E, np.maximum(qn, qcn))
    fig["band_share"] = float(band.mean())
    f = np.asarray(got_flags).astype(bool)
    if (one & ~f).any():
        i = int(np.nonzero(one & ~f)[0][0])
        note("flag_one", f"query {i}: not certified although its exact k-th best lies {(kth64[i] - last[i]) / E[i]:.4f} E' above the kc-th pass score")
    if (zero & f).any():
        i = int(np.nonzero(zero & f)[0][0])
        note("flag_zero", f"query {i}: certified although its exact k-th best lies {(kth64[i] - last[i]) / E[i]:.4f} E' above the kc-th pass score")
    if band.mean() > 0.01:
        note("band_cap", f"{band.mean():.4f} of the queries lie inside the 0.1 % band")
    return bad, fig
