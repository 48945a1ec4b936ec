"""References for what the certified fp16 screen leaves BEHIND its first candidate pass (HipFlatIndex.last_screen_seeds()): the seeds level 0
hands on (hb_rerank_finish, csrc/hbird_rerank_dev.h), the gather of the failing queries, the second pass' lists, pass scores, certificates and
k-th scores; and for the plain fp16 copy (HipFlatIndex.last_fp16_copy()).  Plain numpy; nothing here knows of pools, slots or gathers, and
every quantity is a function of the previous stage's READ-OUT (as in f16_centre_refs.py): a wrong stage fails its own assertion and no later one.

The chain: a query whose first certificate fails gets a second fp16 pass with k' = 256 whose pools start from
    floor0 = kth0 - 1.001 E  (and a hair; centred: kth0 - c_q - 1.001 E', the pass' units)
with kth0 the exact k-th best among the first pass' candidates.  Every row that can still enter the top k scores above floor0 in fp16, so a
second list that does NOT fill up holds every such row and is certified by the seed rule  kth1 > seed + (c_q) + E ; a full list by the usual
rule; what fails again goes to the fp32 kernel with kth1 as its floor.  A floor that is too HIGH by less than the gap to the next row loses
rows, the list does not fill up, and the not-full rule certifies an incomplete answer: sound results then rest on the fp32 search alone.

tests/test_f16_second_pass_gpu.py and tests/test_f16_copy_gpu.py hold the library to these; tests/test_f16_second_pass_cpu.py holds a host
model of the chain to them, shows which wrong variants they catch, and guards the case list.

Assertion names: SEED_NAMES, LEVEL1_NAMES, COPY_NAMES below."""
from __future__ import annotations

import collections
import functools

import numpy as np

import bank_refs
import f16_centre_refs as CR
import f16_pass_refs as R
import f16_screen_worlds as fw

F32 = np.float32
KC1 = 256                 # k' of the second pass
SEED_NAMES = ("kth0_bits", "kth0_inf", "floor0_high", "floor0_low", "floor0_inf", "queries1", "seed1", "n2")
LEVEL1_NAMES = ("valid1", "sorted1", "rows1", "score_bits1", "H1", "H2", "not_full", "flag1_one", "flag1_zero", "kth1_bits")
COPY_NAMES = ("tiles", "tile_padding", "row_padding", "flag", "flag_host", "rows")


def _note(bad, name, msg):
    bad.setdefault(name, f"{name}: {msg}")


def same(a, b) -> np.ndarray:
    """Elementwise equality of two read-out arrays: floats on bits (CR.same_bits), integers and flags by value; different shapes: all False."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return np.zeros(1, bool)
    return CR.same_bits(a, b) if a.dtype.kind == "f" else a == b


def bound_E_centred(qn, qcn, bmax, cmax, mun, t, D, metric):
    """E' of csrc/hbird_certificate.h (hb_certificate_bound_centred), restated in float64 (tests/test_f16_centre_cpu.py holds the same
    restatement to the compiled constants)."""
    qn, qcn = np.asarray(qn, np.float64), np.asarray(qcn, np.float64)
    du = (D + 4) * 1.2e-7
    return (qcn * cmax * (1.05 / 1024.0 + du) + du * (qn * bmax + qn * mun + 2.0 * abs(t) * mun * cmax + (bmax * bmax if metric == 1 else 0.0))
            + (qcn + cmax) * np.sqrt(float(D)) * 6e-8 + 1e-30)


# ---- the exact side: fp32 chain scores of named rows -----------------------------------------------------------------------------------------
def chain_scores(q, bank, rows, metric) -> np.ndarray:
    """float32 [n, kc]: per query i and candidate rows[i, j] the fp32 chain score of the library's exact kernels (oracle/hbird_oracle.c):
    acc = binit[row]; acc = fmaf(q_k, b_k, acc), k ascending.  -inf where rows is -1."""
    q, bank = np.asarray(q, F32), np.asarray(bank, F32)
    r = np.maximum(rows, 0)
    acc = CR.binit_ref(bank, metric)[r]
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(q.shape[1]):
            acc = bank_refs.fma_f32(np.broadcast_to(q[:, d:d + 1], r.shape), bank[:, d][r], acc)
    return np.where(rows < 0, F32(-np.inf), acc).astype(F32)


def kth_of(chain, k) -> np.ndarray:
    """the k-th best of every row of chain (missing entries are -inf: fewer than k candidates give -inf)"""
    with np.errstate(invalid="ignore"):
        return (-np.sort(-chain, axis=1))[:, k - 1].astype(F32)


def query_norms(q) -> np.ndarray:
    q64 = np.asarray(q, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((q64 * q64).sum(axis=1))


def seedless(qn, E, cq=None) -> np.ndarray:
    """Queries that get NO seed: the certificate's precondition fails (||q|| not within the fp16 range -- NaN and inf included), or E / c_q is
    not finite."""
    with np.errstate(invalid="ignore"):
        bad = ~(qn <= R.F16_LIMIT) | ~np.isfinite(E)
        if cq is not None:
            bad |= ~np.isfinite(cq)
    return bad


def check_seeds(S, rows0, cert0, q, bank, metric, k, E, cq=None):
    """Level 0's seeds and the gather -> ({name: message}, figures).  S: last_screen_seeds(); rows0 / cert0: the level-0 lists and first
    certificates (last_screen() of the same search run without its second pass); E [nq]: the bound by the Python restatement (E' when cq, the
    centred pass' c_q [nq], is given)."""
    bad, fig = {}, {}
    nq = S["nq"]
    qn = query_norms(q)
    off = seedless(qn, E, cq)
    chain0 = chain_scores(q, bank, rows0, metric)
    kth = kth_of(chain0, k)
    want_inf = off | np.isneginf(kth) | ~np.isfinite(kth)
    got = S["kth0"]
    m = np.isneginf(got) != want_inf
    if m.any():
        i = int(np.flatnonzero(m)[0])
        _note(bad, "kth0_inf", f"query {i}: kth0 {got[i]!r}, the reference expects {'-inf' if want_inf[i] else repr(kth[i])} (||q|| = {qn[i]!r}, E = {E[i]!r})")
    live = ~want_inf & ~np.isneginf(got)
    m = live & ~CR.same_bits(got, kth)
    if m.any():
        i = int(np.flatnonzero(m)[0])
        _note(bad, "kth0_bits", f"query {i}: kth0 {got[i]!r}, the k-th best chain score of its {int((rows0[i] >= 0).sum())} candidates is {kth[i]!r}")
    fl = S["floor0"].astype(np.float64)
    m = np.isneginf(S["floor0"]) != np.isneginf(got)
    if m.any():
        i = int(np.flatnonzero(m)[0])
        _note(bad, "floor0_inf", f"query {i}: floor0 {S['floor0'][i]!r} with kth0 {got[i]!r}")
    base = got.astype(np.float64) - (cq.astype(np.float64) if cq is not None else 0.0)
    with np.errstate(invalid="ignore"):
        hi = live & ~(fl < base - E)
        lo = live & ~(fl >= base - 1.002 * E - 1e-37)
    if live.any():
        with np.errstate(invalid="ignore"):
            margin = ((base - fl) / E)[live]
        fig["floor_margin_over_E"] = [float(margin.min()), float(margin.max())]
    if hi.any():
        i = int(np.flatnonzero(hi)[0])
        _note(bad, "floor0_high", f"query {i}: floor0 {fl[i]!r} is not below kth0 [- c_q] - E = {base[i] - E[i]!r} ((kth - floor) / E = {(base[i] - fl[i]) / E[i]:.6f})")
    if lo.any():
        i = int(np.flatnonzero(lo)[0])
        _note(bad, "floor0_low", f"query {i}: floor0 {fl[i]!r} lies below kth0 [- c_q] - 1.002 E ((kth - floor) / E = {(base[i] - fl[i]) / E[i]:.6f})")
    if not np.array_equal(S["certified0"], cert0):
        _note(bad, "queries1", "the first certificates of the search with its second pass differ from those of the search without")
    want_q1 = np.flatnonzero(S["certified0"] == 0)
    if S["n1"]:
        if not np.array_equal(S["queries1"], want_q1):
            _note(bad, "queries1", f"{S['queries1'][:8]} ..., the queries with certified0 == 0 are {want_q1[:8]} ... ({want_q1.size})")
        elif not CR.same_bits(S["seed1"], S["floor0"][S["queries1"]]).all():
            j = int(np.flatnonzero(~CR.same_bits(S["seed1"], S["floor0"][S["queries1"]]))[0])
            _note(bad, "seed1", f"second-pass query {j} (query {S['queries1'][j]}) was seeded with {S['seed1'][j]!r}, its floor0 is {S['floor0'][S['queries1'][j]]!r}")
    return bad, fig


# ---- the second pass ---------------------------------------------------------------------------------------------------------------------------
def exact_level1_lists(W, metric, queries1, seed1):
    """Exact worlds: rows int64 [n1, 256] / scores float32 of the best 256 by (score desc, row asc) of {rows: pass score >= seed}."""
    s2 = R.exact_scores2(W, metric)
    unit = 0.5 * 4.0 ** W["scale_log2"]
    n1 = len(queries1)
    rows = np.full((n1, KC1), -1, np.int64)
    scores = np.full((n1, KC1), -np.inf, F32)
    for j, qi in enumerate(queries1):
        sc = s2[qi].astype(np.float64) * unit
        keep = np.flatnonzero(sc >= float(seed1[j]))
        order = keep[np.lexsort((keep, -sc[keep]))][:KC1]
        rows[j, :order.size] = order
        scores[j, :order.size] = sc[order].astype(F32)
    return rows, scores


def check_level1(S, q, bank, metric, k, E, ref=None, exact=None, cq=None, skip=None, allowed=None):
    """The second pass' lists, certificates and k-th scores -> ({name: message}, figures).  ref: R.float_reference of (q, bank) for a float
    world (plain pass only); exact: the exact world W.  E [nq], cq [nq] or None as in check_seeds.  skip: bool [nq], queries whose lists are
    not looked at (non-finite operands).  allowed: bool [n1, 256] or None -- an excluding search (tests/excl_screen_refs.py): the entries of
    rows1 that kth1 is taken over; the lists and the certificates' thresholds are those of the unmasked lists."""
    bad, fig = {}, {"acc_over_A": 0.0, "undecided_share": 0.0, "band_share1": 0.0, "not_full": 0, "full": 0}
    n1 = S["n1"]
    if n1 == 0:
        return bad, fig
    Q1, seed = S["queries1"], S["seed1"].astype(np.float64)
    rows, p32 = S["rows1"], S["scores1"]
    N = bank.shape[0]
    sk = np.zeros(n1, bool) if skip is None else skip[Q1]
    ok = ~sk
    have = rows >= 0
    n_have = have.sum(axis=1)
    full = n_have == KC1
    fig["full"], fig["not_full"] = int((full & ok).sum()), int((~full & ok).sum())
    # the shape of a list: entries first, -1 / -inf behind them, rows of the bank, none twice, sorted by (pass score desc, row asc)
    shape_ok = np.array([have[j, :n_have[j]].all() for j in range(n1)]) & (rows < N).all(axis=1) \
        & np.array([np.isneginf(p32[j, n_have[j]:]).all() and np.isfinite(p32[j, :n_have[j]]).all() for j in range(n1)])
    srt = np.sort(np.where(have, rows, -1 - np.arange(KC1)[None, :]), axis=1)
    shape_ok &= ~(srt[:, 1:] == srt[:, :-1]).any(axis=1)
    if (ok & ~shape_ok).any():
        j = int(np.flatnonzero(ok & ~shape_ok)[0])
        _note(bad, "valid1", f"second-pass query {j} (query {Q1[j]}): a gap, a row outside the bank, a repeated row or a non-finite pass score in its list of {n_have[j]}")
        return bad, fig
    p = p32.astype(np.float64)
    for j in np.flatnonzero(ok):
        n = n_have[j]
        pv, rv = p[j, :n], rows[j, :n]
        if not ((pv[:-1] > pv[1:]) | ((pv[:-1] == pv[1:]) & (rv[:-1] < rv[1:]))).all():
            _note(bad, "sorted1", f"second-pass query {j} (query {Q1[j]}): the list is not sorted by (pass score descending, row ascending)")
            break
    if exact is not None:
        wr, ws = exact_level1_lists(exact, metric, Q1, S["seed1"])
        m = ok & (rows != wr).any(axis=1)
        if m.any():
            j = int(np.flatnonzero(m)[0]); c = int(np.flatnonzero(rows[j] != wr[j])[0])
            _note(bad, "rows1", f"second-pass query {j} (query {Q1[j]}): entry {c} is row {rows[j, c]}, the reference has {wr[j, c]} (list of {n_have[j]}, reference {int((wr[j] >= 0).sum())}, seed {seed[j]!r})")
        m = ok & ~CR.same_bits(p32, ws).all(axis=1) & ~m
        if m.any():
            j = int(np.flatnonzero(m)[0]); c = int(np.flatnonzero(~CR.same_bits(p32[j], ws[j]))[0])
            _note(bad, "score_bits1", f"second-pass query {j} (query {Q1[j]}): entry {c} (row {rows[j, c]}) has pass score {p32[j, c]!r}, exactly {ws[j, c]!r}")
    if ref is not None:
        s16, A = ref["s16"][Q1], ref["A"][Q1]
        inside = np.zeros((n1, N), bool)
        for j in range(n1):
            inside[j, rows[j, :n_have[j]]] = True
        c16 = np.take_along_axis(s16, np.maximum(rows, 0), axis=1)
        acc = np.where(have & ok[:, None], np.abs(p - c16), 0.0) / A[:, None]
        fig["acc_over_A"] = float(acc.max())
        if (acc > 1.0).any():
            j, c = np.unravel_index(np.argmax(acc), acc.shape)
            _note(bad, "H1", f"second-pass query {j} (query {Q1[j]}) entry {c} (row {rows[j, c]}): |pass - s16| = {acc[j, c]:.3f} A")
        last = p[:, KC1 - 1]
        over = ~inside & (full & ok)[:, None] & (s16 > (last + 2.0 * A)[:, None])
        if over.any():
            j, r = [int(v[0]) for v in np.nonzero(over)]
            _note(bad, "H2", f"second-pass query {j} (query {Q1[j]}): row {r} is no candidate, its s16 exceeds the last entry's pass score by {(s16[j, r] - last[j]) / A[j]:.3f} A")
        lost = ~inside & (~full & ok)[:, None] & (s16 >= (seed + A)[:, None])
        if lost.any():
            j, r = [int(v[0]) for v in np.nonzero(lost)]
            _note(bad, "not_full", f"second-pass query {j} (query {Q1[j]}): its list holds {n_have[j]} < 256 rows and lacks row {r}, whose s16 lies {(s16[j, r] - seed[j]) / A[j]:.3f} A above the seed")
        undecided = (np.abs(s16 - seed[:, None]) < A[:, None]).any(axis=1) & ok
        fig["undecided_share"] = float(undecided.sum() / max(1, ok.sum()))
    # the certificates, from both sides outside the 0.1 % band, as a function of the read-out kth1 (held on bits below), the read-out list
    # and seed: the device compares in fp32 with its own evaluation of E, the band takes both up
    kth64 = S["kth1"].astype(np.float64)
    E1, qn1 = E[Q1], query_norms(q)[Q1]
    add = cq[Q1].astype(np.float64) if cq is not None else 0.0
    with np.errstate(invalid="ignore"):
        thr = np.where(full, p[:, KC1 - 1], seed) + add
        one, zero, band = R.flag_band(kth64, thr, E1, qn1)
        nonfin = ~(qn1 <= R.F16_LIMIT) | ~np.isfinite(E1) | ~np.isfinite(thr)
    one, zero = one & ~nonfin, zero | nonfin
    if N < KC1:
        one, zero = ~nonfin, nonfin
    band = ~one & ~zero
    fig["band_share1"] = float(band.mean())
    f = S["certified1"].astype(bool)
    if (one & ~f).any():
        j = int(np.flatnonzero(one & ~f)[0])
        _note(bad, "flag1_one", f"second-pass query {j} (query {Q1[j]}, list of {n_have[j]}): not certified although its exact k-th best lies {(kth64[j] - thr[j]) / E1[j]:.4f} E above the {'last pass score' if full[j] else 'seed'}")
    if (zero & f).any():
        j = int(np.flatnonzero(zero & f)[0])
        _note(bad, "flag1_zero", f"second-pass query {j} (query {Q1[j]}, list of {n_have[j]}): certified although its exact k-th best lies {(kth64[j] - thr[j]) / E1[j]:.4f} E above the {'last pass score' if full[j] else 'seed'} (||q|| = {qn1[j]!r})")
    # kth1, on bits: as kth0, over the second pass' candidates
    kth = kth_of(chain_scores(np.asarray(q, F32)[Q1], bank, rows if allowed is None else np.where(allowed, rows, -1), metric), k)
    want_inf = seedless(qn1, E1, None if cq is None else cq[Q1]) | ~np.isfinite(kth)
    got = S["kth1"]
    m = (np.isneginf(got) != want_inf) | (~want_inf & ~CR.same_bits(got, kth))
    if m.any():
        j = int(np.flatnonzero(m)[0])
        _note(bad, "kth1_bits", f"second-pass query {j} (query {Q1[j]}): kth1 {got[j]!r}, the reference has {'-inf' if want_inf[j] else repr(kth[j])}")
    return bad, fig


def check_n2(S):
    bad = {}
    want = int((S["certified1"] == 0).sum()) if S["n1"] else int((S["certified0"] == 0).sum())
    if S["n2"] != want:
        _note(bad, "n2", f"{S['n2']} queries reached the fp32 kernel, {want} certificates of the last fp16 pass failed")
    return bad


# ---- the plain fp16 copy -----------------------------------------------------------------------------------------------------------------------
def f16_rne(x32) -> np.ndarray:
    """uint16 bits of the round-to-nearest-even fp16 image of fp32 values (subnormals kept, overflow to inf)."""
    return CR.f16_bits(x32)


def copy_flag_ref(converted) -> int:
    """The sticky flag: some FINITE |x| > 65504 was converted since the last reset (converted: every fp32 value handed to the conversion)."""
    x = np.abs(np.asarray(converted, F32).astype(np.float64))
    return int((np.isfinite(x) & (x > R.F16_LIMIT)).any())


def check_copy(C, bank, flag_ref, what="", key="bank16"):
    """The tiles of the plain copy (or, key='q16', of the query tiles) against astype(float16), on bits -> {name: message}."""
    bad = {}
    bank = np.asarray(bank, F32)
    N, D = bank.shape
    dp16 = C["dp16"]
    if key == "bank16" and C["rows"] != N:
        _note(bad, "rows", f"{what}{C['rows']} rows converted, the bank has {N}")
        return bad
    n_pad = C[key].size // dp16
    want_pad = (N + 31) // 32 * 32 if key == "bank16" else (N + 255) // 256 * 256
    if dp16 != (D + 127) // 128 * 128 or n_pad != want_pad:
        _note(bad, "rows", f"{what}{n_pad} rows of {dp16} halves read out for {N} x {D}")
        return bad
    got = CR.detile16(C[key], n_pad, dp16)
    want = f16_rne(bank)
    m = ~CR.same_bits(got[:N, :D].view(np.float16), want.view(np.float16))
    if m.any():
        r, c = [int(v[0]) for v in np.nonzero(m)]
        _note(bad, "tiles", f"{what}row {r} component {c}: {got[r, c]:#06x} for {bank[r, c]!r}, round-to-nearest-even gives {want[r, c]:#06x}")
    if (got[:N, D:] != 0).any():
        _note(bad, "tile_padding", f"{what}a padding component [{D}, {dp16}) of a real row is not zero")
    if (got[N:] != 0).any():
        _note(bad, "row_padding", f"{what}a row behind the last real one is not zero")
    if flag_ref is not None:
        if C["flag"] != flag_ref:
            _note(bad, "flag", f"{what}device flag {C['flag']}, the values converted since the last reset give {flag_ref}")
        if C["flag_host"] != flag_ref:
            _note(bad, "flag_host", f"{what}host image {C['flag_host']} of the flag, expected {flag_ref}")
    return bad


EDGE_VALUES = (65504.0, -65504.0, 65519.0, 65520.0, 1e5, np.inf, -np.inf, np.nan, -0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6e-8,
               1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25)
EDGE_FLAGGED = (65519.0, 65520.0, 1e5)          # finite and beyond the fp16 range -- 65519 ROUNDS to 65504 and still counts: |x| > 65504 is the rule


def copy_world(N, D, seed=0, edges=()):
    """Normal rows of scale 1 with sub-normal-range and large components mixed in, and the given edge values planted at known places:
    value e of `edges` at row 37 * (e + 1) % N, column 5 * e % D.  -> (bank float32, [(row, col, value)])"""
    rng = np.random.default_rng([seed, N, D, 40])
    bank = rng.standard_normal((N, D), dtype=F32)
    scale = rng.choice(np.array([1.0, 2.0 ** -16, 2.0 ** -20, 300.0], F32), size=(N, D))      # fp16 subnormals and values near the top binades
    bank *= scale
    planted = []
    for e, v in enumerate(edges):
        r, c = 37 * (e + 1) % N, 5 * e % D
        bank[r, c] = F32(v)
        planted.append((r, c, F32(v)))
    return bank, planted


# ---- the worlds of the second-pass cases ---------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name world D N nq k metric centred regime")
# regime: what the case must reach BY THE REFERENCE ALONE (tests/test_f16_second_pass_cpu.py restates and checks it):
#   not_full_certified  some second-pass list does not fill up and the seed rule certifies it
#   full_failing        some second-pass list is full, fails again and reaches the fp32 kernel
#   all_level1          every query fails its first certificate, n1 > 256 (two query tiles of the second pass)
#   one_failing         exactly one query fails its first certificate
#   exact               an exact world: bit checks of the second pass' lists
#   centred             the centred form: seeds in the pass' units
#   second_pass_centred the centred form with a second pass over a part of the queries: the seed rule with c_q
#   non_finite          a NaN query and a query of norm > 65504: no seed, straight through both levels
#   no_second_pass      k' = 256 at level 0: n1 = 0
#   gather              interleaved query norms 1 and 8, at least two of each reach the fp32 kernel
CASES = [
    Case("rounding100", "rounding100", 64, 4400, 64, 30, 0, False, ("not_full_certified",)),
    Case("rounding100-l2", "rounding100", 384, 4400, 64, 30, 1, False, ("not_full_certified",)),
    Case("rounding300", "rounding300", 128, 7000, 64, 30, 0, False, ("full_failing",)),
    Case("rounding300-l2", "rounding300", 64, 7000, 64, 30, 1, False, ("full_failing",)),
    Case("tight-tokens", "tight", 64, 4096, 300, 30, 0, False, ("all_level1", "full_failing")),
    Case("one-failing", "one", 128, 4300, 70, 30, 0, False, ("one_failing", "not_full_certified")),
    Case("exact", "exact", 64, 4096, 33, 30, 0, False, ("exact",)),
    Case("exact-l2", "exact", 384, 5000, 33, 30, 1, False, ("exact",)),
    Case("massive-128", "massive_activation", 128, 4096, 257, 30, 0, True, ("centred",)),
    Case("massive-768", "massive_activation", 768, 4096, 64, 30, 1, True, ("centred",)),
    Case("centred-clusters", "centred_clusters", 64, 5000, 64, 30, 0, True, ("centred", "second_pass_centred")),
    Case("centred-clusters-neg", "centred_clusters_neg", 64, 5000, 64, 30, 0, True, ("centred", "second_pass_centred")),
    Case("non-finite", "nonfinite", 64, 4096, 40, 30, 0, False, ("non_finite",)),
    Case("k128", "rounding300k128", 64, 8192, 64, 128, 0, False, ("no_second_pass",)),
    Case("gather", "gather", 64, 7000, 64, 30, 0, False, ("gather", "full_failing")),
]
GAPS = (0.5, 0.7, 0.8, 0.9, 0.95)
# (seeds chosen by tests/test_f16_second_pass_cpu.py's guard: at most 10 % of a case's second-pass queries have a row within A of their seed)
WORLD_SEEDS = {"rounding100": 4004, "gather": 4004}


@functools.lru_cache(maxsize=None)
def case_world(c):
    """-> dict bank, queries (float32) [, the exact world's fields]"""
    kc = R.kc_of(c.k)
    if c.world in ("rounding100", "rounding300", "one", "gather", "rounding300k128"):
        n_dec = {"rounding100": 100, "one": 100, "rounding300k128": 300}.get(c.world, 300)
        n_groups = 1 if c.world == "one" else 10
        n_rows = sum(n_dec + 1 + g % 3 for g in range(n_groups))
        W = fw.rounding_world(c.D, c.k, kc, n_groups, n_dec, GAPS, metric=c.metric, seed=WORLD_SEEDS.get(c.name, 4000 + c.D + c.metric), n_background=c.N - n_rows,
                              n_queries_background=c.nq - n_groups)
        bank, q = W["bank"], W["queries"].copy()
        if c.world == "one":                      # the failing query in the middle of the list, not at its head
            q[[0, 41]] = q[[41, 0]]
        if c.world == "gather":                   # the groups' queries interleaved with background ones; every other query 8 times as long
            order = np.empty(c.nq, np.int64)
            order[0:20:2] = np.arange(10); order[1:20:2] = np.arange(10, 20); order[20:] = np.arange(20, c.nq)
            q = q[order]
            q[1::2] *= F32(8.0)
            q[0:20:4] *= F32(8.0)                 # ... and of the groups' queries (even places below 20) every other one: norms 8, 1, 8, 1, ...
        W = {"bank": bank, "queries": np.ascontiguousarray(q)}
    elif c.world == "tight":
        rng = np.random.default_rng([77, c.D, c.N])
        protos = rng.standard_normal((8, c.D), dtype=F32)
        protos /= np.sqrt((protos * protos).sum(axis=1))[:, None]
        bank = np.repeat(protos, c.N // 8, axis=0) + F32(2e-5) * rng.standard_normal((c.N, c.D), dtype=F32)
        bank = bank[rng.permutation(c.N)]
        q = protos[rng.integers(0, 8, c.nq)] * F32(3.0) + F32(0.05) * rng.standard_normal((c.nq, c.D), dtype=F32)
        W = {"bank": np.ascontiguousarray(bank), "queries": np.ascontiguousarray(q)}
    elif c.world == "exact":
        W = dict(R.exact_world(c.N, c.D, c.nq, kc, 23, 0 if c.metric == 0 else -5))
    elif c.world == "nonfinite":
        W = dict(R.normal_world(c.N, c.D, c.nq, seed=3, normalised=True))
        q = W["queries"].copy()
        q[7, 11] = np.nan
        q[23] = F32(1.0e4)                        # 64 components of 1e4: every one an fp16 number, the norm 8e4 is beyond the range
        W["queries"] = q
    elif c.world in ("centred_clusters", "centred_clusters_neg"):
        W = dict(CR.second_pass_world())
        if c.world.endswith("neg"):               # the queries' share of the common component with the other sign: c_q = q.mu < 0, t < 0
            q = W["queries"].copy()
            q[:, [1, c.D // 2, c.D - 2]] -= F32(40.0)
            W["queries"] = q
    else:
        W = dict(fw.VIT_WORLDS[c.world](c.N, c.D, c.nq, seed=5))
    assert W["bank"].shape == (c.N, c.D) and W["queries"].shape == (c.nq, c.D), (c, W["bank"].shape, W["queries"].shape)
    return W


def plain_bounds(q, bank, D, metric):
    """(qn [nq], bmax, E [nq]) by the Python restatement (fw.bound_E)"""
    qn = query_norms(q)
    bmax = float(np.sqrt((np.asarray(bank, np.float64) ** 2).sum(axis=1)).max())
    with np.errstate(invalid="ignore", over="ignore"):
        return qn, bmax, fw.bound_E(qn, bmax, D, metric)


def centred_pass(q, bank, metric):
    """The centred pass by the references of f16_centre_refs.py -> dict: pass_scores float64 [nq, N] (the pass' units: without c_q), cq
    float32 [nq], E float64 [nq] (E' by the restatement), mu, t, cmax, mu_norm, qcn."""
    q, bank = np.asarray(q, F32), np.asarray(bank, F32)
    nq, D = q.shape
    mu = CR.mean_ref(bank)[0]
    mu2, mun = CR.mu_scalars(mu)
    d = CR.differences(bank, mu)
    cq = CR.chain_dot(q, mu)
    t = CR.t_ref(cq, nq, mu2)[0]
    qc = CR.centred_queries(q, mu, t)
    init16 = CR.init16_ref(t, CR.chain_dot(d, mu), CR.binit_ref(bank, metric))
    cmax, qcn = CR.cmax_ref(d), CR.row_norms_up(qc)
    ps = qc.astype(np.float16).astype(np.float64) @ d.astype(np.float16).astype(np.float64).T + init16.astype(np.float64)[None, :]
    qn, bmax, _ = plain_bounds(q, bank, D, metric)
    E = bound_E_centred(qn, qcn.astype(np.float64), bmax, float(cmax), float(mun), float(t), D, metric)
    return {"pass_scores": ps, "cq": cq, "E": E, "mu": mu, "t": t, "cmax": cmax, "mu_norm": mun, "qcn": qcn, "init16": init16,
            "A": centred_A(qcn, cmax, init16, D)}


def centred_A(qcn, cmax, init16, D):
    """The accumulation allowance of the CENTRED pass' sums, per query: an fp32 sum of D exact products that starts from the row init has
    partial sums below ||q - t mu|| max ||b - mu|| + max |init16| and rounds each of its D additions to 2^-24 of one; as for the plain A
    (D 2.4e-7 ||q|| bmax = four times D 2^-24) the factor is 2.4e-7.  Within E': |init16| <= |binit| + |t| ||mu|| cmax, which its du terms hold."""
    fin = np.asarray(init16, np.float64)
    top = float(np.abs(fin[np.isfinite(fin)]).max()) if np.isfinite(fin).any() else 0.0
    return D * 2.4e-7 * (np.asarray(qcn, np.float64) * float(cmax) + top)


def readout_centred_reference(C1, queries1, nq, N, D):
    """The reference of a CENTRED second pass from what the conversion left (HipFlatIndex.last_centre() after that pass: level 1): s16 =
    the float64 sum of the products of the read-out fp16 tiles of the second pass' queries and of the bank + the read-out row init, A =
    centred_A of the read-out norms -> {"s16" [nq, N], "A" [nq]} with the rows of queries1 filled (check_level1 reads no other)."""
    n1 = len(queries1)
    assert C1["level"] == 1 and C1["n"] == n1
    q16 = CR.detile16(C1["q16"], C1["q16"].size // C1["dp16"], C1["dp16"])[:n1, :D].view(np.float16).astype(np.float64)
    b16 = CR.detile16(C1["bank16"], C1["bank16"].size // C1["dp16"], C1["dp16"])[:N, :D].view(np.float16).astype(np.float64)
    s16, A = np.zeros((nq, N)), np.ones(nq)
    s16[queries1] = q16 @ b16.T + C1["init16"][:N].astype(np.float64)[None, :]
    A[queries1] = centred_A(C1["qcn"], C1["cmax"], C1["init16"][:N], D)
    return {"s16": s16, "A": A}


def finite_reference(q, bank, metric, skip):
    """R.float_reference over the queries that are not skipped (finite fp16 operands) -> {"s16" [nq, N], "A" [nq]}, other rows unused."""
    ref = R.float_reference(np.asarray(q, F32)[~skip], bank, metric)
    s16, A = np.zeros((q.shape[0], bank.shape[0])), np.ones(q.shape[0])
    s16[~skip], A[~skip] = ref["s16"], ref["A"]
    return {"s16": s16, "A": A}


@functools.lru_cache(maxsize=None)
def model_inputs(name):
    """The inputs of the host model of a case (the CPU tests of both chains)
    -> (W, kwargs of host_chain: pass_scores / E / cq, the float reference or None, the exact world or None)"""
    c = next(x for x in CASES if x.name == name)
    W = case_world(c)
    if c.centred:
        P = centred_pass(W["queries"], W["bank"], c.metric)
        return W, {"pass_scores": P["pass_scores"], "E": P["E"], "cq": P["cq"]}, {"s16": P["pass_scores"], "A": P["A"]}, None
    E = plain_bounds(W["queries"], W["bank"], c.D, c.metric)[2]
    if c.world == "exact":
        s2 = R.exact_scores2(W, c.metric)
        return W, {"pass_scores": s2.astype(np.float64) * (0.5 * 4.0 ** W["scale_log2"]), "E": E}, None, W
    if c.world == "nonfinite":
        q16 = W["queries"].astype(np.float16).astype(np.float64)
        with np.errstate(invalid="ignore"):
            ps = q16 @ W["bank"].astype(np.float16).astype(np.float64).T
        skip = ~(query_norms(W["queries"]) <= R.F16_LIMIT)
        return W, {"pass_scores": np.where(np.isfinite(ps), ps, -np.inf), "E": E}, finite_reference(W["queries"], W["bank"], c.metric, skip), None
    ref = R.float_reference(W["queries"], W["bank"], c.metric)
    return W, {"pass_scores": ref["s16"], "E": E}, ref, None


# ---- the host model of the chain: level 0 -> seeds -> gather -> level 1 -> flags ------------------------------------------------------------------
def host_chain(q, bank, metric, k, variant="", prev_floor=None, cq=None, E=None, pass_scores=None, seed_override=None, groups=None, qg=None):
    """What a RIGHT chain leaves (variant ''), as a last_screen_seeds() dict plus rows0, or a chain with one thing wrong.  The pass scores are
    the fp32 roundings of s16 (float worlds) or given (pass_scores [nq, N]: exact worlds, the centred pass).  E / cq as in check_seeds.
    variants: floor_half_E, floor_rank_k_minus_2, floor_without_cq, seeds_identity_order, stale_seeds (prev_floor), pool_drops_ties,
    not_full_rule_on_full, seed_rule_without_cq, kth_from_pass_scores.
    groups [N] / qg [nq] (int32): the EXCLUDING chain (csrc/hbird_exclude_screen.hip; tests/excl_screen_refs.py) -- every k-th score is taken
    over the ALLOWED entries of the unmasked lists, the second pass takes its queries' groups along, and what fails last is left to the rungs
    (S gains groups1 and left).  Its variants: kth_counts_excluded (every k-th score over all entries), floor_counts_excluded (the floor only),
    not_full_when_tail_excluded, groups_identity_order, groups_not_gathered, left_misses_one, left_holds_certified."""
    excl = groups is not None
    q, bank = np.asarray(q, F32), np.asarray(bank, F32)
    nq, N = q.shape[0], bank.shape[0]
    kc0 = R.kc_of(k)
    if pass_scores is None:
        pass_scores = R.float_reference(q, bank, metric)["s16"]
    ps = pass_scores.astype(F32)
    if E is None:
        E = plain_bounds(q, bank, q.shape[1], metric)[2]
    cqv = np.zeros(nq) if cq is None else cq.astype(np.float64)
    qn = query_norms(q)

    def lists(sc, n, floor=None, drop_ties=False):
        rows = np.full((sc.shape[0], n), -1, np.int64)
        out = np.full((sc.shape[0], n), -np.inf, F32)
        for i in range(sc.shape[0]):
            keep = np.arange(sc.shape[1]) if floor is None or not np.isfinite(floor[i]) else np.flatnonzero(sc[i] > floor[i] if drop_ties else sc[i] >= floor[i])
            order = keep[np.lexsort((keep, -sc[i, keep].astype(np.float64)))][:n]
            rows[i, :order.size] = order
            out[i, :order.size] = sc[i, order]
        return rows, out

    def level(qs, psl, rows, seed, Es, cqs, qns, qgs=None):
        n = rows.shape[1]
        chain_all = chain_scores(qs, bank, rows, metric)
        ok = np.ones(rows.shape, bool)
        if excl:      # (the kernel's rule: a row >= 0 of the query's group, the query naming one)
            ok = ~((rows >= 0) & (qgs[:, None] >= 0) & (np.asarray(groups)[np.maximum(rows, 0)] == qgs[:, None]))
        chain = chain_all if variant == "kth_counts_excluded" else np.where(ok, chain_all, F32(-np.inf)).astype(F32)
        src = np.where((rows >= 0) & ok, np.take_along_axis(psl, np.maximum(rows, 0), axis=1) + cqs[:, None].astype(F32), F32(-np.inf)) if variant == "kth_from_pass_scores" else chain
        kk = k - 2 if variant == "floor_rank_k_minus_2" else k
        kth_true = kth_of(chain, k)
        kth_seed = kth_of(src, kk) if variant in ("kth_from_pass_scores", "floor_rank_k_minus_2") else kth_true
        if variant == "floor_counts_excluded":
            kth_seed = kth_of(chain_all, k)
        off = seedless(qns, Es, None if cq is None else cqs) | ~np.isfinite(kth_true)
        kth_out = np.where(off, F32(-np.inf), kth_of(src, k) if variant == "kth_from_pass_scores" else kth_true).astype(F32)
        f = 0.5 if variant == "floor_half_E" else 1.001
        sub = 0.0 if variant == "floor_without_cq" else cqs
        with np.errstate(invalid="ignore", over="ignore"):
            fl = kth_seed.astype(np.float64) - sub - f * Es
            fl = (fl - np.abs(fl) * 2.4e-7 - 1e-37).astype(F32)
        fl = np.where(off, F32(-np.inf), fl).astype(F32)
        full = rows[:, n - 1] >= 0
        if variant == "not_full_when_tail_excluded":
            full = full & ok[:, n - 1]
        last = psl[np.arange(rows.shape[0]), np.maximum(rows[:, n - 1], 0)].astype(np.float64)
        with np.errstate(invalid="ignore"):
            okq = (qns <= R.F16_LIMIT) & np.isfinite(kth_true)
            cert = np.where(full, kth_true.astype(np.float64) > last + cqs + Es, N < n) & okq
            if seed is not None:
                add = 0.0 if variant == "seed_rule_without_cq" else cqs
                rule = (kth_true.astype(np.float64) > seed.astype(np.float64) + add + Es) & okq & np.isfinite(seed)
                cert = np.where(full & (variant != "not_full_rule_on_full"), cert, cert | rule)
        return kth_out, fl, cert.astype(np.uint8)

    rows0, _ = lists(ps, kc0)
    qgv = np.asarray(qg, np.int32) if excl else None
    kth0, floor0, cert0 = level(q, ps, rows0, None, E, cqv, qn, qgv)
    S = {"nq": nq, "kc0": kc0, "n1": 0, "kc1": 0, "centred": cq is not None, "kth0": kth0, "floor0": floor0, "certified0": cert0, "rows0": rows0,
         "queries1": np.zeros(0, np.int64), "seed1": np.zeros(0, F32), "rows1": np.zeros((0, 0), np.int64), "scores1": np.zeros((0, 0), F32),
         "certified1": np.zeros(0, np.uint8), "kth1": np.zeros(0, F32), "n2": int((cert0 == 0).sum())}
    Q1 = np.flatnonzero(cert0 == 0)
    if excl:
        S.update(scores0=np.where(rows0 >= 0, np.take_along_axis(ps, np.maximum(rows0, 0), axis=1), F32(-np.inf)).astype(F32), groups1=np.zeros(0, np.int32), left=Q1)
    if kc0 >= KC1 or N < 4096 or Q1.size == 0:
        return S
    seed = floor0[Q1]
    if variant == "seeds_identity_order":
        seed = floor0[:Q1.size]
    if variant == "stale_seeds":
        seed = prev_floor[Q1]
    if seed_override is not None:             # (second-pass query -> seed: a seed placed ON a row's pass score, for the pools' tie rule)
        seed = seed.copy()
        for j, v in seed_override.items():
            seed[j] = v
    rows1, sc1 = lists(ps[Q1], KC1, seed, drop_ties=variant == "pool_drops_ties")
    groups1 = None
    if excl:
        groups1 = qgv[:Q1.size] if variant == "groups_identity_order" else np.full(Q1.size, -1, np.int32) if variant == "groups_not_gathered" else qgv[Q1]
    kth1, _, cert1 = level(q[Q1], ps[Q1], rows1, seed, E[Q1], cqv[Q1], qn[Q1], groups1)
    S.update(n1=int(Q1.size), kc1=KC1, queries1=Q1, seed1=seed.astype(F32), rows1=rows1, scores1=sc1, certified1=cert1, kth1=kth1, n2=int((cert1 == 0).sum()))
    if excl:
        left = Q1[cert1 == 0]
        if variant == "left_misses_one":
            left = left[1:]
        if variant == "left_holds_certified":
            left = np.sort(np.concatenate([left, Q1[cert1 == 1][:1]]))
        S.update(groups1=groups1.astype(np.int32), left=left, n2=int(left.size))
    return S


def copy_model(chunks, D, variant="", resets=()):
    """The host model of the plain copy: chunks (a list of [n, D] float32 arrays, converted one after the other; resets: indices of chunks
    BEFORE which the bank was reset) -> a last_fp16_copy() dict without q16.  variants: truncate, flush_subnormals, flag_not_sticky, flag_on_inf."""
    dp16 = (D + 127) // 128 * 128
    rows, flag = np.zeros((0, D), F32), 0
    for i, ch in enumerate(chunks):
        if i in resets:
            rows, flag = np.zeros((0, D), F32), 0
        ch = np.asarray(ch, F32)
        rows = np.concatenate([rows, ch])
        a = np.abs(ch.astype(np.float64))
        with np.errstate(invalid="ignore"):
            now = int(((a > R.F16_LIMIT) & (np.isfinite(a) | (variant == "flag_on_inf"))).any())
        flag = now if variant == "flag_not_sticky" else (flag | now)
    bits = f16_rne(rows)
    if variant == "truncate":
        with np.errstate(over="ignore", invalid="ignore"):
            h = rows.astype(np.float16)
            too_big = np.abs(h.astype(np.float64)) > np.abs(rows.astype(np.float64))
            h = np.where(too_big & np.isfinite(h), np.nextafter(h, np.float16(0)), h)
        bits = h.view(np.uint16)
    if variant == "flush_subnormals":
        bits = np.where((bits & 0x7C00) == 0, bits & 0x8000, bits).astype(np.uint16)
    N = rows.shape[0]
    n_g = (N + 31) // 32 * 32
    full = np.zeros((n_g, dp16), np.uint16)
    full[:N, :D] = bits
    tiled = full.reshape(n_g // 32, 32, dp16 // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    return {"rows": N, "dp16": dp16, "flag": flag, "flag_host": flag, "n": 0, "level": -1, "bank16": np.ascontiguousarray(tiled)}, rows
