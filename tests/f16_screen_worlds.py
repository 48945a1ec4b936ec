"""Banks and queries that put the certified fp16 screen (csrc/hbird_knn_f16.hip) where its certificate can be WRONG, and a CPU model of the
screen.  Pure numpy, seeded, no GPU: tests/test_f16_certificate_cpu.py holds the worlds to what they promise, tests/test_f16_certificate_gpu.py
runs them through the kernels, tests/lowprec_certificate_report.py tabulates them.

The certificate rests on E >= |fp16 score - exact score| (include/hbird_hip.h):

    E = ||q|| bmax (1.05/1024 + D 2.4e-7) + (||q|| + bmax) sqrt(D) 6e-8 + [L2] D 1.2e-7 0.5 bmax^2 + 1e-30

`rounding_world` builds rows whose fp16 error is close to E and whose score gaps are of the order of E; the other worlds are shaped like ViT
features (shared mean, massive activations, duplicated background tokens) or sit at the ends of the fp16 range (subnormal, near 65504).

rounding_world, the arithmetic
------------------------------
A group lives on 54 of the D dimensions (all other components of its query and rows are exact zeros): 52 adversarial ones and two tuning ones.
  * adversarial dimension j: sign s_j, exponent e_j in {-1, 0, 1} (16 / 28 / 8 of them: sum 4^e = 64, so every group's rows have the same norm).
    query  s_j 2^e_j Q m_lo,  hidden row  s_j 2^e_j B m_lo,  decoy  s_j 2^e_j B m_hi  with  m_lo = 1 + 2^-11 (1 - 2^-6)  just BELOW an fp16
    rounding midpoint and  m_hi = 1 + 2^-11 (1 + 2^-6)  just above it.  In fp16 a hidden row's product loses 2^-10 (1 - 2^-6) of itself, a
    decoy's 2^-22; query and hidden row are parallel, so Cauchy-Schwarz is tight and the loss is that share of ||q|| ||b||.
  * tuning dimensions: query Q and Q 2^-10, row n1 u and n2 u with u = B 2^-12 and integers 16 <= n <= 2047 -- all exact in fp16 and normal, so
    they move a row's score by the same amount in every precision, in steps below 2e-7 of the score.
With S = sum |q_j b_j| of a hidden row, U = 2^-10 S and the spacing delta (below), the ordering scores (L2: with the row init -|b|^2 / 2, in
float64) of a group with h hidden rows are placed at
    T + j delta             hidden row j < h        (the k-th best, ..., (k-h+1)-th best of the query)
    T + (h + i) delta       decoy i < k - h         (the best k - h)
    T - delta, T - 2 delta  two decoys              (rank k+1, k+2: what the re-rank finds as "k-th best" when the hidden rows are missing)
    T - g U                 every other decoy, bit-identical copies (ties by id)
fp16 drops the hidden rows by 0.98 U and leaves the decoys where they are: for g <= 0.95 every decoy ranks above them, and with n_decoys >= k'
the hidden rows are no candidates.  A certificate with bound f E then compares (T - delta) with (T - g U) + f E; E > U, so f = 1 fails for every
g < 1 (sound), and an f small enough that g U - delta > f E certifies an answer that lacks a true neighbour.

Spacing: two placed scores are at least 4 x the worst-case difference between two fp32 summation orders apart, so that neither the MFMA's
summation order nor the chain's can change a candidate set or a rank.  For dense rows that difference is D 2^-23 sum |q_j b_j|.  A group's query has 54 non-zero components whatever D is, and adding a product that is exactly zero rounds nothing, so that worst case is
54 2^-23 S here: delta = 1.02 x 4 x 54 x 2^-23 x S = 2.6e-5 S at every D (the 2 % cover the placement steps).  (With D in place of 54 the spacing would be 3.7e-4 S at D = 768, a
third of E: the rank-(k+1) row would sit so far below T that no mutation of E above 0.46 E could be told from the true bound.)
"""
from __future__ import annotations

import numpy as np

M_LO = 1.0 + 2.0 ** -11 * (1.0 - 2.0 ** -6)
M_HI = 1.0 + 2.0 ** -11 * (1.0 + 2.0 ** -6)
_EXPS = np.array([-1] * 16 + [0] * 28 + [1] * 8)       # sum 4^e = 64
N_ADV = 52
NNZ = N_ADV + 2
_N_LO, _N_HI = 16, 2047                                # integer range of a tuning component (n u: exact in fp16, never subnormal)


def bound_E(qn, bmax, D, metric, c16=1.05):
    """The documented bound, restated (float64).  c16: the factor on 2^-10 (1.05 as shipped)."""
    qn = np.asarray(qn, dtype=np.float64)
    return (qn * bmax * (c16 / 1024.0 + D * 2.4e-7) + (qn + bmax) * np.sqrt(float(D)) * 6e-8
            + (D * 1.2e-7 * 0.5 * bmax * bmax if metric == 1 else 0.0) + 1e-30)


def _unit_rows(rng, n, D, norm):
    x = rng.standard_normal((n, D), dtype=np.float32)
    x *= (np.float32(norm) / np.sqrt(np.einsum("ij,ij->i", x, x)))[:, None]
    return x


def rounding_world(D, k, kc, n_groups, n_decoys, gap_fracs, metric=0, seed=0, n_background=4096, n_queries_background=0, bank_scale=1.0,
                   query_scale=1.0):
    """-> dict: bank [N, D] float32, queries [n_groups + n_queries_background, D] float32 (the groups' queries first), hidden_ids (one int64
    array per group), group_ids (all rows of a group), g (one gap fraction per group, gap_fracs cycled), delta / U / S / T (per group, float64), min_spacing = 4 x 54 x 2^-23 x S: what two
    placed scores are apart at least.
    bank_scale / query_scale: powers of two; the same seed gives the same queries and the same group geometry at every bank_scale."""
    assert D >= NNZ and n_decoys >= (k - 1) + 2 + 1 and kc >= k
    for s in (bank_scale, query_scale):
        assert s > 0 and np.log2(s) == int(np.log2(s)), "scales are powers of two (the mantissas must survive)"
    rng = np.random.default_rng([seed, 0])
    B, Q = 2.0 ** -3 * bank_scale, 2.0 ** -3 * query_scale
    u = B * 2.0 ** -12
    q1, q2 = Q, Q * 2.0 ** -10
    assert q2 >= 2.0 ** -14 and _N_LO * u >= 2.0 ** -14, "a tuning component would be an fp16 subnormal"
    n = np.arange(_N_LO, _N_HI + 1, dtype=np.float64)
    l2 = 0.5 if metric == 1 else 0.0
    f1 = q1 * u * n - l2 * (u * n) ** 2                 # what tuning component n adds to the ordering score (exact in float64: <= 35 bits)
    f2 = q2 * u * n - l2 * (u * n) ** 2
    assert np.all(np.diff(f1) > 0), "the coarse tuning term must grow with n (L2: the query's scale below half the bank's)"
    # the fine term: every n for the inner product (steps of q2 u); L2: n <= 128, where -|b|^2 / 2 moves it by at most 128 u^2 per step
    fine = np.arange(len(n)) if metric == 0 else np.arange(128 - _N_LO + 1)
    fine = fine[np.argsort(f2[fine], kind="stable")]
    f2s = f2[fine]
    assert f2s[-1] - f2s[0] >= np.diff(f1).max() and np.diff(f2s).max() <= 2e-7 * 64.0 * Q * B, "the fine term must span a coarse step, finely"
    rows, queries, group_rows, hidden_rows, gs, meta = [], [], [], [], [], []
    for gi in range(n_groups):
        g = float(gap_fracs[gi % len(gap_fracs)])
        h = 1 + gi % 3
        dims = rng.permutation(D)[:NNZ]
        adv, t1, t2 = dims[:N_ADV], dims[N_ADV], dims[N_ADV + 1]
        p = rng.choice([-1.0, 1.0], N_ADV) * 2.0 ** rng.permutation(_EXPS)
        q = np.zeros(D); q[adv] = p * M_LO * Q; q[t1] = q1; q[t2] = q2
        b_h = np.zeros(D); b_h[adv] = p * M_LO * B
        b_d = np.zeros(D); b_d[adv] = p * M_HI * B
        base_h = float(q @ b_h) - l2 * float(b_h @ b_h)
        base_d = float(q @ b_d) - l2 * float(b_d @ b_d)
        S = float(np.abs(q[adv] * b_d[adv]).sum()) + q1 * u * _N_HI + q2 * u * _N_HI     # >= sum |q_j b_j| of every row of the group
        U = 2.0 ** -10 * S
        delta = 1.02 * 4.0 * NNZ * 2.0 ** -23 * S
        n0 = _N_LO + int(np.ceil((U + 3.0 * delta) / (q1 * u))) + 8
        T = base_h + f1[n0 - _N_LO] + f2[64 - _N_LO]
        assert g * U >= 3.0 * delta, "the bulk of the decoys must lie below the two rank-(k+1, k+2) decoys"
        targets = [(base_h, b_h, T + j * delta) for j in range(h)]
        targets += [(base_d, b_d, T + (h + i) * delta) for i in range(k - h)]
        targets += [(base_d, b_d, T - delta), (base_d, b_d, T - 2.0 * delta)]
        n_rest = n_decoys - (k - h) - 2
        targets += [(base_d, b_d, T - g * U)]
        out = []
        for base, proto, tgt in targets:
            r = tgt - base
            i1 = int(np.searchsorted(f1, r - f2s[0], side="right")) - 1                 # the largest n1 that leaves the fine term its range
            assert 0 <= i1 < len(n), "target outside the tuning range"
            i2 = int(fine[np.argmin(np.abs(f2s - (r - f1[i1])))])
            assert abs(r - f1[i1] - f2[i2]) <= 1e-7 * S, "target not reached within one fine step"
            row = proto.copy(); row[t1] = n[i1] * u; row[t2] = n[i2] * u
            out.append(row)
        out += [out[-1]] * (n_rest - 1)
        start = sum(len(r_) for r_ in rows)
        rows.append(np.asarray(out))
        queries.append(q)
        group_rows.append(np.arange(start, start + len(out)))
        hidden_rows.append(np.arange(start, start + h))
        gs.append(g)
        meta.append((delta, U, S, T))
    grp = np.concatenate(rows)
    grp32 = grp.astype(np.float32)
    assert np.array_equal(grp32.astype(np.float64), grp), "every planted value is an fp32 number"
    norm = float(np.sqrt((grp[hidden_rows[0][0]] ** 2).sum()))
    rb = np.random.default_rng([seed, 1])
    bank = np.concatenate([grp32, _unit_rows(rb, n_background, D, norm)])
    perm = np.random.default_rng([seed, 2]).permutation(bank.shape[0])
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)                          # row i of `bank` lands at inv[i]
    bank = bank[perm]
    qs = np.asarray(queries).astype(np.float32)
    assert np.array_equal(qs.astype(np.float64), np.asarray(queries))
    if n_queries_background:
        qs = np.concatenate([qs, _unit_rows(np.random.default_rng([seed, 3]), n_queries_background, D, float(np.sqrt((queries[0] ** 2).sum())))])
    m = np.asarray(meta)
    return {"bank": np.ascontiguousarray(bank), "queries": np.ascontiguousarray(qs), "hidden_ids": [np.sort(inv[r_]) for r_ in hidden_rows],
            "group_ids": [np.sort(inv[r_]) for r_ in group_rows], "g": np.asarray(gs), "delta": m[:, 0], "U": m[:, 1], "S": m[:, 2], "T": m[:, 3], "min_spacing": m[:, 0] / 1.02,
            "n_groups": n_groups, "k": k, "kc": kc, "metric": metric}


# ---- ViT-shaped worlds ----------------------------------------------------------------------------------------------------------------------
def _normalised(x):
    x = x.astype(np.float32, copy=False)
    x /= np.sqrt(np.einsum("ij,ij->i", x, x))[:, None]
    return x


def shared_mean_world(N, D, nq, seed=0, cosine=0.45):
    """Rows mu + sigma noise, normalised: the mean pairwise cosine is `cosine` (0.3 .. 0.6 for ViT patch features)."""
    rng = np.random.default_rng([seed, 10])
    mu = rng.standard_normal(D); mu /= np.linalg.norm(mu)
    a, s = np.sqrt(cosine), np.sqrt((1.0 - cosine) / D)
    def make(n):
        x = rng.standard_normal((n, D), dtype=np.float32)
        x *= np.float32(s); x += (a * mu).astype(np.float32)
        return _normalised(x)
    bank, q = make(N), np.float32(3.0) * make(nq)
    return {"bank": bank, "queries": q}


def massive_activation_world(N, D, nq, seed=0, n_massive=3, lo=30.0, hi=100.0):
    """N(0,1) features with 2-4 dimensions at 30-100 x the rest, the same sign on every row; normalised rows."""
    rng = np.random.default_rng([seed, 11])
    dims = rng.permutation(D)[:n_massive]
    amp = rng.uniform(lo, hi, n_massive) * rng.choice([-1.0, 1.0], n_massive)

    def make(n):
        x = rng.standard_normal((n, D), dtype=np.float32)
        x[:, dims] = (amp * (1.0 + 0.1 * rng.standard_normal((n, n_massive)))).astype(np.float32)
        return x
    return {"bank": _normalised(make(N)), "queries": np.float32(3.0) * _normalised(make(nq)), "dims": dims}


def duplicate_background_world(N, D, nq, seed=0, blocks=(100, 1000, 317), near=64):
    """Normalised random rows; `blocks`: runs of bit-identical rows scattered over the bank, each followed by `near` copies that differ by one
    ulp in one component; a third of the queries sit next to a duplicated row, so that ties by id decide whole answers."""
    rng = np.random.default_rng([seed, 12])
    bank = _normalised(rng.standard_normal((N, D), dtype=np.float32))
    ids = rng.permutation(N)
    at, protos = 0, []
    for n_dup in blocks:
        proto = bank[ids[at]].copy()
        protos.append(proto)
        bank[ids[at:at + n_dup]] = proto
        at += n_dup
        nd = bank[ids[at:at + near]]
        nd[:] = proto
        j = rng.integers(0, D, near)
        nd[np.arange(near), j] = np.nextafter(nd[np.arange(near), j], np.float32(np.inf) * rng.choice([-1.0, 1.0], near).astype(np.float32))
        bank[ids[at:at + near]] = nd
        at += near
    q = np.float32(3.0) * _normalised(rng.standard_normal((nq, D), dtype=np.float32))
    for i in range(0, nq, 3):
        q[i] = np.float32(3.0) * protos[(i // 3) % len(protos)] + np.float32(0.05) * rng.standard_normal(D, dtype=np.float32)
    return {"bank": bank, "queries": q}


def subnormal_world(N, D, nq, seed=0):
    """Every bank component has a magnitude in [6e-8, 6e-5], log-uniform -- all of them fp16 subnormals -- and the queries are noisy multiples of
    bank rows with ||q|| of about 3e4 (< 65504).  A pass that flushes fp16 subnormals scores every row 0."""
    rng = np.random.default_rng([seed, 13])
    mag = np.exp(rng.uniform(np.log(6.1e-8), np.log(5.9e-5), (N, D)))
    bank = (mag * rng.choice([-1.0, 1.0], (N, D))).astype(np.float32)
    src = rng.integers(0, N, nq)
    q = bank[src].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True) + 0.5 * rng.standard_normal((nq, D)) / np.sqrt(D)
    q = 3.0e4 * q / np.linalg.norm(q, axis=1, keepdims=True)
    return {"bank": bank, "queries": q.astype(np.float32)}


def near_limit_world(N, D, nq, seed=0):
    """Bank and query components up to exactly +-65504 (the largest fp16 number); nothing in (65504, 65520), which rounds to 65504 in fp16 but is
    no fp16 number.  Half of the queries keep ||q|| < 65504 (the certificate can pass), the others carry one component at the limit.  Scores stay
    below 1e13: finite in fp32."""
    rng = np.random.default_rng([seed, 14])
    bank = np.clip(2000.0 * rng.standard_normal((N, D), dtype=np.float32), -65504.0, 65504.0)
    hot = rng.integers(0, N, max(8, N // 50))
    bank[hot, rng.integers(0, D, hot.size)] = (65504.0 * rng.choice([-1.0, 1.0], hot.size)).astype(np.float32)
    q = rng.standard_normal((nq, D), dtype=np.float32)
    q *= (3.0e4 / np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))).astype(np.float32)[:, None]
    odd = np.arange(1, nq, 2)
    q[odd, rng.integers(0, D, odd.size)] = (65504.0 * rng.choice([-1.0, 1.0], odd.size)).astype(np.float32)
    assert np.abs(bank).max() == 65504.0 and np.abs(q).max() == 65504.0
    return {"bank": bank, "queries": q}


VIT_WORLDS = {"shared_mean": shared_mean_world, "massive_activation": massive_activation_world, "duplicate_background": duplicate_background_world,
              "subnormal": subnormal_world, "near_limit": near_limit_world}


# ---- the CPU model of the screen -----------------------------------------------------------------------------------------------------------
def _top(scores, n):
    """Ids of the n best of one score vector (score descending, ties by ascending id)."""
    return np.argsort(-scores, kind="stable")[:n]


def _f32_orders(q16, b16, init32):
    """One query's fp16-operand scores accumulated in fp32 in three orders (the products of two fp16 numbers are exact in fp32):
    ascending, blocks of 16 (each summed ascending, then the block sums ascending), pairwise."""
    prod = b16 * q16[None, :]                                     # float32 [N, D], exact
    N, D = prod.shape
    asc = init32.copy()
    for j in range(D):
        asc += prod[:, j]
    pad = (-D) % 16
    pb = np.pad(prod, ((0, 0), (0, pad))).reshape(N, -1, 16)
    blk = np.zeros(pb.shape[:2], dtype=np.float32)
    for j in range(16):
        blk += pb[:, :, j]
    b16s = init32.copy()
    for j in range(blk.shape[1]):
        b16s += blk[:, j]
    n2 = 1 << int(np.ceil(np.log2(D)))
    tree = np.pad(prod, ((0, 0), (0, n2 - D)))
    while tree.shape[1] > 1:
        tree = tree[:, 0::2] + tree[:, 1::2]
    return {"ascending": asc, "blocks16": b16s, "pairwise": init32 + tree[:, 0]}


def screen_model(q, bank, k, kc, metric=0, factors=(1.0,), flush_subnormals=False, orders=False):
    """What the screen would do with operands rounded to fp16 (astype(float16): round to nearest even, subnormals kept; flush_subnormals:
    bank components below 2^-14 become zero, the model of an MFMA that flushes them).  Per query:
      err_over_E       max over rows of |s16 - s| / E; s16: products summed in float64, s: the float64 score of the fp32 values
      E                the documented bound
      cand             the fp16 top-kc (ids, best first, ties by id)
      contained        the true top-k (float64, ties by id) lies within cand
      certified[f]     a single pass whose certificate uses f E: exact k-th best of the candidates > kc-th candidate's fp16 score + f E
      wrong[f]         certified[f] and not contained: the pass would return an answer that lacks a true neighbour
    orders=True adds err_over_E_f32 (the worst of three fp32 summation orders) and same_candidates (all three give the candidate SET of the
    float64 sum)."""
    q = np.ascontiguousarray(q, dtype=np.float32); bank = np.ascontiguousarray(bank, dtype=np.float32)
    nq, D = q.shape
    N = bank.shape[0]
    assert N >= kc >= k
    q64, b64 = q.astype(np.float64), bank.astype(np.float64)
    q16 = q.astype(np.float16).astype(np.float32)
    b16 = bank.astype(np.float16).astype(np.float32)
    assert np.isfinite(q16).all() and np.isfinite(b16).all(), "the model assumes finite fp16 operands"
    if flush_subnormals:
        b16 = np.where(np.abs(b16) < 2.0 ** -14, np.float32(0.0), b16)
    init = -0.5 * (b64 ** 2).sum(axis=1) if metric == 1 else np.zeros(N)
    init32 = init.astype(np.float32)
    s = q64 @ b64.T + init[None, :]
    s16 = q16.astype(np.float64) @ b16.astype(np.float64).T + init32.astype(np.float64)[None, :]
    E = bound_E(np.sqrt((q64 ** 2).sum(axis=1)), float(np.sqrt((b64 ** 2).sum(axis=1)).max()), D, metric)
    res = {"E": E, "err_over_E": np.abs(s16 - s).max(axis=1) / E, "cand": [], "contained": np.zeros(nq, bool), "true_topk": [],
           "certified": {f: np.zeros(nq, bool) for f in factors}, "wrong": {f: np.zeros(nq, bool) for f in factors},
           "gap_over_E": np.zeros(nq)}
    if orders:
        res["err_over_E_f32"] = np.zeros(nq); res["same_candidates"] = np.ones(nq, bool)
    for i in range(nq):
        cand = _top(s16[i], kc)
        true = _top(s[i], k)
        res["cand"].append(cand); res["true_topk"].append(true)
        res["contained"][i] = np.isin(true, cand).all()
        kth = np.sort(s[i][cand])[::-1][k - 1]
        res["gap_over_E"][i] = (np.sort(s[i])[::-1][k - 1] - np.sort(s[i])[::-1][kc - 1]) / E[i]
        for f in factors:
            res["certified"][f][i] = kth > s16[i][cand[kc - 1]] + f * E[i]
            res["wrong"][f][i] = res["certified"][f][i] and not res["contained"][i]
        if orders:
            for name, so in _f32_orders(q16[i], b16, init32).items():
                res["err_over_E_f32"][i] = max(res["err_over_E_f32"][i], float(np.abs(so.astype(np.float64) - s[i]).max() / E[i]))
                res["same_candidates"][i] &= np.array_equal(np.sort(_top(so, kc)), np.sort(cand))
    return res
