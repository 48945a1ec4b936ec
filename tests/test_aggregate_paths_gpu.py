"""K5 (label aggregation, csrc/hbird_aggregate.hip; the body is k5_body of csrc/hbird_k5_dev.h) on every code path against a float64 restatement of its contract.

hb_launch_aggregate (its table: hb_k5_table_choose) picks one of three bodies of aggregate_kernel: the (neighbour group, class) form for C <= 32, the 16-byte gather
of uint16 count rows (32 < C <= 512, P <= 2048, row stride a multiple of 8, 16-byte aligned base) and the generic loop over 64-class
chunks.  Every case below names the body it is meant to reach; tests/test_post_agg_coverage_cpu.py checks each name against the
dispatch predicates and that the list reaches every body with every table form.

The neighbour lists are given, not searched, so a case does not depend on K4: bank rows of norms 0.5 .. 2 (stored unnormalised),
unnormalised queries of norm |q|, and scores built so that the cosines of one list lie in a band of width 2 beta (every neighbour
carries real weight).  Label rows are dense random multiples of 1 / P.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
D = 16                  # feature width (only the query norms reach K5)
NQ_PATTERNS = 7         # neighbour-list patterns, see _neighbours
NQ = 8 * NQ_PATTERNS

# form: where the label rows live and in which storage
#   own_f32       the index's own fp32 rows (add_labels)
#   own_u16_196   the index's own uint16 counts, P = 196 (set_label_denominator; rows padded to 16 bytes)
#   own_u16_4096  the same with P = 4096: beyond the three-instruction quotient, K5 divides in place
#   ext_f32       a borrowed fp32 table (set_label_table)
#   ext_u16       a borrowed dense count table (set_label_count_table), P = 196: row stride C
#   ext_u16_mis   the same, its base 8 bytes off a 16-byte boundary (a view into a larger int16 buffer)
# branch: the body of aggregate_kernel the case is meant to reach (grouped / wide / generic)
AggCase = namedtuple("AggCase", "branch form C k metric beta qs id_base")
FORM_P = {"own_f32": 196, "own_u16_196": 196, "own_u16_4096": 4096, "ext_f32": 196, "ext_u16": 196, "ext_u16_mis": 196}

CASES = [
    # C <= 32: (neighbour group, class) lanes
    AggCase("grouped", "own_f32", 1, 7, "ip", 0.02, 1, 0),
    AggCase("grouped", "own_f32", 21, 256, "ip", 0.07, 1000, 0),
    AggCase("grouped", "own_f32", 31, 9, "l2", 1.0, 1000, 0),
    AggCase("grouped", "own_u16_196", 2, 64, "l2", 0.02, 1, 3000),
    AggCase("grouped", "own_u16_196", 32, 90, "ip", 0.02, 30, 0),
    AggCase("grouped", "own_u16_196", 3, 200, "ip", 1.0, 300, 0),
    AggCase("grouped", "own_u16_4096", 21, 8, "ip", 0.07, 30, 0),
    AggCase("grouped", "own_u16_4096", 3, 65, "l2", 1.0, 30, 777),
    AggCase("grouped", "ext_f32", 2, 63, "ip", 0.07, 1, 0),
    AggCase("grouped", "ext_f32", 31, 1, "l2", 0.02, 30, 0),
    AggCase("grouped", "ext_u16", 21, 30, "l2", 0.07, 1, 0),
    AggCase("grouped", "ext_u16", 32, 256, "ip", 0.02, 300, 0),
    AggCase("grouped", "ext_u16_mis", 32, 7, "l2", 1.0, 300, 0),
    AggCase("grouped", "ext_u16_mis", 1, 90, "ip", 0.07, 1000, 0),
    # 16-byte gather of count rows
    AggCase("wide", "own_u16_196", 33, 9, "ip", 0.02, 1, 0),
    AggCase("wide", "own_u16_196", 64, 256, "ip", 0.02, 1000, 0),
    AggCase("wide", "own_u16_196", 65, 63, "l2", 0.07, 30, 0),
    AggCase("wide", "own_u16_196", 151, 8, "l2", 0.02, 1, 4096),
    AggCase("wide", "own_u16_196", 152, 200, "ip", 1.0, 30, 0),
    AggCase("wide", "own_u16_196", 512, 65, "ip", 0.07, 300, 0),
    AggCase("wide", "ext_u16", 64, 1, "ip", 0.07, 30, 0),
    AggCase("wide", "ext_u16", 152, 90, "l2", 0.07, 1, 0),
    AggCase("wide", "ext_u16", 512, 9, "l2", 1.0, 1000, 0),
    # generic loop over 64-class chunks
    AggCase("generic", "own_f32", 33, 64, "ip", 1.0, 1, 0),
    AggCase("generic", "own_f32", 151, 30, "l2", 0.02, 1, 0),
    AggCase("generic", "own_f32", 513, 7, "ip", 0.02, 30, 12345),
    AggCase("generic", "own_f32", 1000, 256, "ip", 0.07, 1, 0),
    AggCase("generic", "own_f32", 65, 8, "l2", 1.0, 300, 0),
    AggCase("generic", "own_u16_196", 513, 90, "ip", 0.02, 300, 0),
    AggCase("generic", "own_u16_196", 1000, 9, "l2", 0.07, 30, 0),
    AggCase("generic", "own_u16_4096", 151, 63, "ip", 0.07, 1000, 0),
    AggCase("generic", "own_u16_4096", 1000, 1, "l2", 1.0, 1, 0),
    AggCase("generic", "own_u16_4096", 64, 64, "ip", 1.0, 30, 500),
    AggCase("generic", "ext_f32", 152, 256, "ip", 0.02, 30, 0),
    AggCase("generic", "ext_f32", 1000, 65, "l2", 0.07, 1, 0),
    AggCase("generic", "ext_u16", 33, 200, "l2", 1.0, 1, 0),
    AggCase("generic", "ext_u16", 151, 7, "ip", 0.02, 1000, 0),
    AggCase("generic", "ext_u16", 513, 64, "ip", 0.07, 300, 0),
    AggCase("generic", "ext_u16", 1000, 8, "ip", 1.0, 30, 0),
    AggCase("generic", "ext_u16_mis", 64, 30, "ip", 0.02, 1, 0),
    AggCase("generic", "ext_u16_mis", 152, 9, "l2", 1.0, 1000, 0),
    AggCase("generic", "ext_u16_mis", 512, 63, "ip", 0.07, 30, 0),
    AggCase("generic", "ext_u16_mis", 1000, 1, "ip", 0.02, 300, 0),
]

# label-sharded partial sums: one table over three indices (uneven row counts, one empty), each index's own storage
ShardCase = namedtuple("ShardCase", "branch form C k metric beta qs")
SHARD_CASES = [
    ShardCase("grouped", "own_f32", 21, 64, "ip", 0.02, 30),
    ShardCase("wide", "own_u16_196", 151, 200, "l2", 0.07, 1),
    ShardCase("generic", "own_u16_196", 1000, 30, "ip", 1.0, 300),
]
SHARD_ROWS = (410, 0, 190)

# search_aggregate (K4 -> K5 in one call) against aggregate on the neighbours it returns
FUSED_CASES = [(C, k) for C in (21, 151, 1000) for k in (30, 256)]


def case_id(c):
    return f"{c.branch}-{c.form}-C{c.C}-k{c.k}-{c.metric}-b{c.beta}-q{c.qs}" + (f"-base{c.id_base}" if getattr(c, "id_base", 0) else "")


# ---------------------------------------------------------------- inputs

def _rows(n, rng):
    """Bank rows: random directions, norms spread over 0.5 .. 2 (stored as they are, no normalisation)."""
    b = rng.standard_normal((n, D))
    b *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(b, axis=1, keepdims=True)
    return b.astype(np.float32)


def _labels(n, C, P, rng):
    """Dense label rows j / P (fp32, as K2 produces them), j uniform in 0 .. P: every class non-zero in most rows."""
    j = rng.integers(0, P + 1, (n, C))
    return (j.astype(np.float32) / np.float32(P)).astype(np.float32), j.astype(np.uint16)


def _queries(qs, rng):
    q = rng.standard_normal((NQ, D))
    q *= qs / np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def _neighbours(rng, k, n_rows, base, beta, metric, q, norms):
    """(idx, dist) for NQ queries; query i follows pattern i % NQ_PATTERNS:
    0 plain, 1 / 2 / 3: a run of -1 at the head / middle / tail, 4: only -1, 5: ids outside the norm table (above its end and
    below its start), 6: repeated ids.  Scores: cosines in [c0 - beta, c0 + beta] (clipped to [-1, 1]), IP = cos |q| |b|,
    L2 = qn2 + |b|^2 - 2 IP with the fp32 chain |q|^2 the kernel uses."""
    qn = np.linalg.norm(q.astype(np.float64), axis=1)
    qn2 = oracle.chain_sqnorm(q).astype(np.float64)
    idx = np.empty((NQ, k), np.int64)
    dist = np.empty((NQ, k), np.float32)
    g = max(1, k // 8)
    for i in range(NQ):
        rows = rng.choice(n_rows, k, replace=k > n_rows)
        ids = base + rows
        pat = i % NQ_PATTERNS
        if pat == 1:
            ids[:g] = -1
        elif pat == 2:
            ids[k // 3:k // 3 + g] = -1
        elif pat == 3:
            ids[k - g:] = -1
        elif pat == 4:
            ids[:] = -1
        elif pat == 5:
            ids[0::3] = base + n_rows + rng.integers(0, 50, ids[0::3].shape)
            ids[1::5] = base - 1 - rng.integers(0, 50, ids[1::5].shape)
        elif pat == 6:
            ids[1::2] = ids[0:k - 1:2][: len(ids[1::2])]
            ids[-(k // 3):] = ids[0]
        c0 = rng.uniform(-0.6, 0.8) * max(0.0, 1.0 - beta)
        cos = np.clip(c0 + beta * rng.uniform(-1.0, 1.0, k), -1.0, 1.0)
        r = ids - base
        inside = (ids >= 0) & (r >= 0) & (r < n_rows)
        bn = np.where(inside, norms[np.clip(r, 0, n_rows - 1)], 1.0)
        ip = cos * qn[i] * bn
        d = ip if metric == "ip" else qn2[i] + bn * bn - 2.0 * ip
        miss = ids < 0
        d = np.where(miss, -np.inf if metric == "ip" else np.inf, d)      # what a search reports for a missing neighbour
        idx[i] = ids
        dist[i] = d.astype(np.float32)
    return idx, dist


# ---------------------------------------------------------------- float64 restatement of K5's contract

def reference(q, idx, dist, norms, norm_base, labels, label_base, beta, metric):
    """label_hat[i] = sum_j w_ij label[id_ij] in float64 with
         w_ij = softmax_j(cos_ij / beta) over the neighbours that take part (an id inside the norm table [norm_base, + len(norms))),
         cos_ij = ip_ij / (max(|q_i|, 1e-12) max(|b_j|, 1e-12)),  ip = dist (inner product) or (qn2 + |b|^2 - dist) / 2 (L2),
       the sum running over the rows of the label table [label_base, + len(labels)) only (label-sharded partial sums).
    -> (label_hat [nq, C], weights [nq, k] (0 where not taking part), logits [nq, k] (nan where not taking part))"""
    q64 = q.astype(np.float64)
    qn = np.maximum(np.linalg.norm(q64, axis=1), 1e-12)[:, None]
    qn2 = oracle.chain_sqnorm(q).astype(np.float64)[:, None]
    nrm = norms.astype(np.float64)
    rn = idx - norm_base
    part = (idx >= 0) & (rn >= 0) & (rn < len(nrm))
    b = np.where(part, nrm[np.clip(rn, 0, len(nrm) - 1)], 1.0)
    d = np.where(part, dist.astype(np.float64), 0.0)
    ip = d if metric == "ip" else 0.5 * (qn2 + b * b - d)
    logit = np.where(part, ip / (qn * np.maximum(b, 1e-12)) / beta, -np.inf)
    mx = logit.max(axis=1, keepdims=True)
    e = np.where(part, np.exp(logit - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
    den = e.sum(axis=1, keepdims=True)
    w = np.divide(e, den, out=np.zeros_like(e), where=den > 0)
    rl = idx - label_base
    own = part & (rl >= 0) & (rl < len(labels))
    lab = labels.astype(np.float64)
    wo = np.where(own, w, 0.0)
    rows = np.clip(rl, 0, max(len(labels) - 1, 0))
    out = np.zeros((idx.shape[0], labels.shape[1]))
    if len(labels):
        for i in range(idx.shape[0]):
            out[i] = wo[i] @ lab[rows[i]]
    return out, w, np.where(part, logit, np.nan)


def tolerance(q, idx, dist, norms, norm_base, logits, k, beta, metric, max_label):
    """Per-query bound on |K5 - reference|, first order in U (derivation):
      * logit_j = (ip_j / (qn bn_j)) / beta: three fp32 roundings and the fp32 |q| (sqrt of a double sum) -- relative 4 U, i.e.
        4 U |logit_j|; beta's own conversion to fp32 is a common relative factor, inside the same 4 U.
      * e_j = expf(logit_j - mx): the subtraction rounds at U |logit_j - mx| <= U spread, expf adds about 2 U (relative), its argument
        reduction another U spread: 2 U spread + 2 U.
        A perturbation delta_j of the logits moves label_hat by sum_j w_j (delta_j - mean delta) label_j, at most
        max|delta| max|label| for labels >= 0.
      * den: ceil(k / 64) additions per lane and a 6-level butterfly, 1 / den and w = e / den: (ceil(k / 64) + 8) U relative on every
        weight alike, a relative error of label_hat.
      * sum_j w_j label_j: at most k fmaf steps (the grouped form fewer): k U sum_j w_j |label_j| <= k U max|label|.
      * L2 only: ip = 0.5 (qn2 + bn * bn - dist) rounds bn^2, qn2 + bn^2 and the difference: delta ip <= U (qn2 / 2 + bn^2 + |ip|), a
        logit error delta ip / (|q| bn beta) -- it grows with |q| (qn2 / |q| = |q|) and with 1 / beta.
    The count quotients are exact (test_ops_gpu.py::test_count_quotients_are_exact), so the table form adds nothing.
      tol = max|label| (U (4 max|logit| + 2 spread + k + ceil(k / 64) + 10) + L2 term)
    which is (c1 U / beta + c2 k U) max|label| with c1 <= 4 + 4 = 8 (|logit| <= 1 / beta, spread <= 2 / beta), c2 ~ 1."""
    live = ~np.isnan(logits)
    lmax = np.where(live, np.abs(logits), 0.0).max(axis=1)
    spread = np.where(live.any(axis=1), np.where(live, logits, -np.inf).max(axis=1) - np.where(live, logits, np.inf).min(axis=1), 0.0)
    tol = U * (4.0 * lmax + 2.0 * spread + k + math.ceil(k / 64) + 10)
    if metric == "l2":
        qn = np.linalg.norm(q.astype(np.float64), axis=1)[:, None]
        qn2 = oracle.chain_sqnorm(q).astype(np.float64)[:, None]
        rn = idx - norm_base
        part = (idx >= 0) & (rn >= 0) & (rn < len(norms))
        b = np.where(part, norms.astype(np.float64)[np.clip(rn, 0, len(norms) - 1)], 1.0)
        ip = 0.5 * (qn2 + b * b - np.where(part, dist.astype(np.float64), 0.0))
        t = np.where(part, U * (qn2 / 2 + b * b + np.abs(ip)) / (np.maximum(qn, 1e-12) * b * beta), 0.0)
        tol = tol + t.max(axis=1)
    return tol * max_label


def _sensitivity(q, idx, dist, norms, norm_base, labels, label_base, beta, metric, P, ref, w, tol):
    """float64 only: the comparison must see (a) the least-weighted neighbour of each list dropped and (b) one class's label one count
    off in every row -- the smallest change a wrong class stride or offset makes (a single count in one of 256 rows moves label_hat by
    far less than the rounding bound; the list check (a) stands for the per-row errors).  Both must move a typical query (the median)
    by more than 20 x its tolerance."""
    live = (w > 0).any(axis=1)
    wd = np.where(w > 0, w, np.inf)
    drop = idx.copy()
    drop[np.arange(len(idx)), wd.argmin(axis=1)] = -1
    r_drop = reference(q, drop, dist, norms, norm_base, labels, label_base, beta, metric)[0]
    shifted = labels.astype(np.float64).copy()
    shifted[:, -1] += 1.0 / P
    r_shift = reference(q, idx, dist, norms, norm_base, shifted, label_base, beta, metric)[0]
    m_drop = np.abs(r_drop - ref).max(axis=1)[live] / tol[live]
    m_shift = np.abs(r_shift - ref).max(axis=1)[live] / tol[live]
    return float(np.median(m_drop)), float(np.median(m_shift))


def make_case(c, seed):
    """Everything a case needs on the host: table rows, norms, labels, queries and neighbour lists."""
    rng = np.random.default_rng(seed)
    P = FORM_P[c.form]
    n = 300
    bank = _rows(n, rng)
    labels, counts = _labels(n, c.C, P, rng)
    q = _queries(c.qs, rng)
    return dict(rng=rng, P=P, n=n, bank=bank, labels=labels, counts=counts, q=q)


# ---------------------------------------------------------------- tests

def _run_case(c, seed):
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    h = make_case(c, seed)
    rng, P, n, labels = h["rng"], h["P"], h["n"], h["labels"]
    metric = 0 if c.metric == "ip" else 1
    ix = HipFlatIndex(D, metric, 0)
    call_base = c.id_base
    keep = []
    if c.form.startswith("own"):
        if c.form.startswith("own_u16"):
            ix.set_label_denominator(P)
        ix.add(torch.from_numpy(h["bank"]).cuda())
        ix.add_labels(torch.from_numpy(labels).cuda())
        ix.set_num_classes(c.C)
        norms = ix.copy_norms().cpu().numpy()
        base = c.id_base
    else:
        norms = np.linalg.norm(h["bank"].astype(np.float64), axis=1).astype(np.float32)
        base = 4321                                        # the table's own id_base: it overrides the call's
        call_base = 99
        nt = torch.from_numpy(norms).cuda()
        if c.form == "ext_f32":
            ix.set_label_table(torch.from_numpy(labels).cuda(), nt, base)
        else:
            flat = torch.from_numpy(h["counts"].view(np.int16)).cuda().reshape(-1)
            if c.form == "ext_u16_mis":
                buf = torch.zeros(flat.numel() + 16, dtype=torch.int16, device="cuda")
                off = (-(buf.data_ptr() // 2) + 4) % 8                  # element offset: base = 8 (mod 16) bytes
                buf[off:off + flat.numel()] = flat
                tab = buf[off:off + flat.numel()].view(n, c.C)
                assert tab.data_ptr() % 16 == 8 and tab.is_contiguous()
                keep.append(buf)
            else:
                tab = flat.view(n, c.C)
                assert tab.data_ptr() % 16 == 0
            ix.set_label_count_table(tab, nt, P, base)
    idx, dist = _neighbours(rng, c.k, n, base, c.beta, c.metric, h["q"], norms.astype(np.float64))
    got = ix.aggregate(torch.from_numpy(h["q"]).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda(),
                       beta=c.beta, id_base=call_base).cpu().numpy()
    ref, w, logits = reference(h["q"], idx, dist, norms, base, labels, base, c.beta, c.metric)
    tol = tolerance(h["q"], idx, dist, norms, base, logits, c.k, c.beta, c.metric, float(labels.max()))
    return got, ref, w, tol, h, idx, dist, norms, base


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_k5_path_against_float64(cuda_device, c):
    seed = CASES.index(c) + 1
    got, ref, w, tol, h, idx, dist, norms, base = _run_case(c, seed)
    s_drop, s_shift = _sensitivity(h["q"], idx, dist, norms, base, h["labels"], base, c.beta, c.metric, h["P"], ref, w, tol)
    assert s_drop > 20 and s_shift > 20, f"the case cannot see a dropped neighbour ({s_drop:.1f} x tol) or a count off by one ({s_shift:.1f} x tol)"
    empty = ~(w > 0).any(axis=1)
    assert empty.any() and np.array_equal(got[empty].view(np.uint32), np.zeros_like(got[empty]).view(np.uint32)), "a list of only -1 must give exactly 0"
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)
    ratio = err / tol
    i = int(ratio.argmax())
    print(f"K5 {case_id(c)}: max err {err.max():.3e}, max err / bound {ratio.max():.3f} (query {i}: err {err[i]:.3e}, bound {tol[i]:.3e})")
    assert ratio.max() <= 1.0, f"query {i} (pattern {i % NQ_PATTERNS}): |K5 - float64| = {err[i]:.3e} > bound {tol[i]:.3e} (ratio {ratio.max():.2f})"


@pytest.mark.parametrize("c", SHARD_CASES, ids=case_id)
def test_k5_label_sharded_partial_sums(cuda_device, c):
    """aggregate_partial on three indices that split one table (row counts SHARD_ROWS, one shard empty): each partial against the float64
    partial sum, and the float64 sum of the three partials against the full reference."""
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(1000 + SHARD_CASES.index(c))
    P = FORM_P[c.form]
    n = sum(SHARD_ROWS)
    bank = _rows(n, rng)
    labels, _ = _labels(n, c.C, P, rng)
    q = _queries(c.qs, rng)
    metric = 0 if c.metric == "ip" else 1
    shards, lo = [], 0
    for rows in SHARD_ROWS:
        ix = HipFlatIndex(D, metric, 0)
        if c.form.startswith("own_u16"):
            ix.set_label_denominator(P)
        if rows:
            ix.add(torch.from_numpy(bank[lo:lo + rows]).cuda())
            ix.add_labels(torch.from_numpy(labels[lo:lo + rows]).cuda())
        ix.set_num_classes(c.C)
        shards.append((ix, lo, rows))
        lo += rows
    norms_all = torch.cat([ix.copy_norms() for ix, _, _ in shards])
    norms = norms_all.cpu().numpy()
    idx, dist = _neighbours(rng, c.k, n, 0, c.beta, c.metric, q, norms.astype(np.float64))
    qt, it, dt = torch.from_numpy(q).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()
    full, w, logits = reference(q, idx, dist, norms, 0, labels, 0, c.beta, c.metric)
    tol = tolerance(q, idx, dist, norms, 0, logits, c.k, c.beta, c.metric, float(labels.max()))
    total = np.zeros_like(full)
    for ix, lo, rows in shards:
        got = ix.aggregate_partial(qt, it, dt, norms_all, beta=c.beta, id_base=lo).cpu().numpy()
        part = reference(q, idx, dist, norms, 0, labels[lo:lo + rows], lo, c.beta, c.metric)[0]
        err = np.abs(got - part).max(axis=1)
        assert (err <= tol).all(), f"shard at {lo} ({rows} rows): max err / bound {(err / tol).max():.2f}"
        if rows == 0:
            assert not got.any()
        total += got
    err = np.abs(total - full).max(axis=1)
    assert (err <= 3 * tol).all(), f"sum of the partials: max err / bound {(err / (3 * tol)).max():.2f}"


def test_k5_rejects_k_above_256_and_nonpositive_beta(cuda_device):
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(7)
    n, C = 300, 21
    bank = _rows(n, rng)
    labels, _ = _labels(n, C, 196, rng)
    ix = HipFlatIndex(D, 0, 0)
    ix.add(torch.from_numpy(bank).cuda()); ix.add_labels(torch.from_numpy(labels).cuda()); ix.set_num_classes(C)
    q = torch.from_numpy(_queries(1.0, rng)[:4]).cuda()
    idx = torch.randint(0, n, (4, 257), device="cuda")
    dist = torch.rand((4, 257), device="cuda")
    with pytest.raises(RuntimeError, match=r"k must be (<= 256|in \[1, 256\])"):
        ix.aggregate(q, idx, dist)
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 256\]"):
        ix.search_aggregate(q, 257)
    with pytest.raises(RuntimeError, match=r"k must be (<= 256|in \[1, 256\])"):
        ix.aggregate_partial(q, idx, dist, ix.copy_norms())
    for beta in (0.0, -0.02):
        with pytest.raises(RuntimeError, match="beta must be positive"):
            ix.aggregate(q, idx[:, :30], dist[:, :30], beta=beta)
        with pytest.raises(RuntimeError, match="beta must be positive"):
            ix.search_aggregate(q, 30, beta=beta)
        with pytest.raises(RuntimeError, match="beta must be positive"):
            ix.aggregate_partial(q, idx[:, :30], dist[:, :30], ix.copy_norms(), beta=beta)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("C,k", FUSED_CASES)
def test_k5_fused_search_equals_aggregate(cuda_device, C, k, metric):
    """search_aggregate (K4 -> K5 in one call) gives the bits of aggregate on the neighbours it returns."""
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(C * 1000 + k)
    n = 2000
    bank = _rows(n, rng)
    labels, _ = _labels(n, C, 196, rng)
    ix = HipFlatIndex(D, 0 if metric == "ip" else 1, 0)
    ix.add(torch.from_numpy(bank).cuda()); ix.add_labels(torch.from_numpy(labels).cuda()); ix.set_num_classes(C)
    q = torch.from_numpy(_queries(3.0, rng)).cuda()
    lh, idx, dist = ix.search_aggregate(q, k, want_neighbours=True)
    again = ix.aggregate(q, idx, dist)
    assert torch.equal(lh.view(torch.int32), again.view(torch.int32))
    assert int((idx >= 0).sum()) == NQ * k
