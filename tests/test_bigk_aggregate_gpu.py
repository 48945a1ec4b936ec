"""K5 beyond 256 neighbours (aggregate_bigk_kernel, csrc/hbird_aggregate.hip: k5_body of csrc/hbird_k5_dev.h on dynamic LDS) through HipFlatIndex.aggregate_bigk / aggregate_partial_bigk /
search_aggregate_bigk.

Inputs, the float64 reference and its bound are those of tests/test_aggregate_paths_gpu.py: `_run_case` builds the index of a case in
its table form and calls `aggregate`; here it runs with a HipFlatIndex whose `aggregate` also remembers the call, so the very same
index and device tensors reach `aggregate_bigk`.

 (a) k <= 256: aggregate_bigk's bits are aggregate's (the arithmetic order is part of the new kernel's contract).
 (b) k > 256: within tolerance(...) of reference(...).
 (c) a condition on (b)'s inputs, checked on the host before the GPU is asked: the float64 reference of the list cut at every multiple
     of 256 below k is more than 10 x the bound away from the full one in some row -- a kernel that loses a chunk cannot pass (b).
     `_neighbours` puts a list's cosines in a band of 2 beta, so every neighbour carries weight; beta and |q| are chosen so that the bound
     stays near k U (small logits, no large |q| / beta term in the L2 conversion).
"""
from __future__ import annotations

import numpy as np
import pytest

import test_aggregate_paths_gpu as A
from test_aggregate_paths_gpu import AggCase, SHARD_ROWS, _labels, _neighbours, _queries, _rows, reference, tolerance

pytestmark = pytest.mark.gpu

# (body, table form, C): every body of the kernel with own / borrowed tables in fp32 / uint16 storage (the wide body exists for counts only)
TABLES = [
    ("grouped", "own_f32", 21), ("grouped", "own_u16_196", 21), ("grouped", "ext_f32", 19), ("grouped", "ext_u16", 32),
    ("wide", "own_u16_196", 151), ("wide", "ext_u16", 64),
    ("generic", "own_f32", 151), ("generic", "ext_f32", 65), ("generic", "own_u16_4096", 70), ("generic", "ext_u16_mis", 100),
]
SMALL_K = (1, 30, 64, 200, 256)
BIG_K = (257, 300, 512, 1000, 2048)
BETA, QS = 0.07, 1      # logits up to 1 / 0.07, |q| = 1: the bound is (k + ...) U, the L2 term 1e-5


def _cases(ks):
    return [AggCase(b, f, C, k, m, BETA, QS, 0) for (b, f, C) in TABLES for m in ("ip", "l2") for k in ks]


def _recording_index(monkeypatch, before=None):
    """HipFlatIndex for `_run_case`: `aggregate` keeps its arguments and serves k > 256 from aggregate_bigk (the old entry refuses them),
    after `before(norms, base, idx, dist)` has seen the inputs on the host -- norms and id range of the table the kernel will read."""
    from hbird_mi.nn import search_hip

    class Recording(search_hip.HipFlatIndex):
        calls = []
        _ext = None

        def set_label_table(self, labels, norms, id_base=0):
            self._ext = (norms.cpu().numpy(), id_base)
            super().set_label_table(labels, norms, id_base)

        def set_label_count_table(self, counts, norms, P, id_base=0):
            self._ext = (norms.cpu().numpy(), id_base)
            super().set_label_count_table(counts, norms, P, id_base)

        def aggregate(self, q, idx, dist, beta=0.02, id_base=0):
            Recording.calls.append((self, q, idx, dist, beta, id_base))
            if before is not None:
                norms, base = self._ext if self._ext is not None else (self.copy_norms().cpu().numpy(), id_base)
                before(norms, base, idx.cpu().numpy(), dist.cpu().numpy())
            if idx.shape[1] > 256:
                return self.aggregate_bigk(q, idx, dist, beta=beta, id_base=id_base)
            return super().aggregate(q, idx, dist, beta=beta, id_base=id_base)

    monkeypatch.setattr(search_hip, "HipFlatIndex", Recording)
    return Recording


def test_the_grid_reaches_every_body_and_table_form():
    assert {b for b, _, _ in TABLES} == {"grouped", "wide", "generic"}
    forms = {f for _, f, _ in TABLES}
    assert {"own_f32", "ext_f32"} <= forms and any(f.startswith("own_u16") for f in forms) and any(f.startswith("ext_u16") for f in forms)
    for b, f, C in TABLES:      # the dispatch of hb_launch_aggregate_bigk (hb_launch_aggregate's)
        wide = f in ("own_u16_196", "ext_u16") and 32 < C <= 512 and (f.startswith("own") or C % 8 == 0)
        assert b == ("grouped" if C <= 32 else "wide" if wide else "generic"), (b, f, C)


@pytest.mark.parametrize("c", _cases(SMALL_K), ids=A.case_id)
def test_bigk_bits_equal_the_old_kernel_up_to_256(cuda_device, monkeypatch, c):
    rec = _recording_index(monkeypatch)
    old = A._run_case(c, 5000 + c.k)[0]
    ix, q, idx, dist, beta, id_base = rec.calls[-1]
    new = ix.aggregate_bigk(q, idx, dist, beta=beta, id_base=id_base).cpu().numpy()
    assert np.isfinite(old).all() and np.abs(old).max() > 0
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), f"{(new != old).sum()} of {old.size} values differ, max |diff| {np.abs(new - old).max():.3e}"


@pytest.mark.parametrize("c", _cases(BIG_K), ids=A.case_id)
def test_bigk_against_float64_beyond_256(cuda_device, monkeypatch, c):
    seed = 7000 + c.k
    host = A.make_case(c, seed)           # the table `_run_case` builds from the same seed
    seen = {}

    def inputs_see_a_lost_chunk(norms, base, idx, dist):
        """(c), on the host before the kernel is launched: the list cut at every multiple of 256 below k moves some row of the float64
        reference by more than 10 x that row's bound."""
        ref, _, logits = reference(host["q"], idx, dist, norms, base, host["labels"], base, c.beta, c.metric)
        tol = tolerance(host["q"], idx, dist, norms, base, logits, c.k, c.beta, c.metric, float(host["labels"].max()))
        for m in range(256, c.k, 256):
            cut = reference(host["q"], idx[:, :m], dist[:, :m], norms, base, host["labels"], base, c.beta, c.metric)[0]
            seen[m] = float((np.abs(cut - ref).max(axis=1) / tol).max())
        print(f"K5 bigk {A.case_id(c)}: the list cut at m moves the reference by (x bound) {seen}")
        assert seen and min(seen.values()) > 10, f"the inputs cannot see a list cut at {min(seen, key=seen.get)}: {seen}"

    rec = _recording_index(monkeypatch, before=inputs_see_a_lost_chunk)
    got, ref, w, tol, h, idx, dist, norms, base = A._run_case(c, seed)
    assert seen and rec.calls[-1][2].shape[1] == c.k and np.array_equal(h["labels"], host["labels"])
    empty = ~(w > 0).any(axis=1)
    assert empty.any() and not got[empty].any(), "a list of only -1 must give exactly 0"
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)
    ratio = err / tol
    i = int(ratio.argmax())
    print(f"K5 bigk {A.case_id(c)}: max err {err.max():.3e}, max err / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0, f"query {i} (pattern {i % A.NQ_PATTERNS}): |K5 - float64| = {err[i]:.3e} > bound {tol[i]:.3e}"


@pytest.mark.parametrize("form,C,metric", [("own_f32", 21, "ip"), ("own_u16_196", 151, "l2"), ("own_u16_196", 1000, "ip")])
def test_bigk_label_sharded_partial_sums(cuda_device, form, C, metric):
    """aggregate_partial_bigk at k = 600 over three indices that split one table (SHARD_ROWS, one empty): the partials sum to the full
    float64 result within 3 x the bound; the empty shard gives zeros."""
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    k = 600
    rng = np.random.default_rng(9000 + C)
    P = A.FORM_P[form]
    n = sum(SHARD_ROWS)
    bank = _rows(n, rng)
    labels, _ = _labels(n, C, P, rng)
    q = _queries(QS, rng)
    shards, lo = [], 0
    for rows in SHARD_ROWS:
        ix = HipFlatIndex(A.D, 0 if metric == "ip" else 1, 0)
        if form.startswith("own_u16"):
            ix.set_label_denominator(P)
        if rows:
            ix.add(torch.from_numpy(bank[lo:lo + rows]).cuda())
            ix.add_labels(torch.from_numpy(labels[lo:lo + rows]).cuda())
        ix.set_num_classes(C)
        shards.append((ix, lo, rows))
        lo += rows
    norms_all = torch.cat([ix.copy_norms() for ix, _, _ in shards])
    norms = norms_all.cpu().numpy()
    idx, dist = _neighbours(rng, k, n, 0, BETA, metric, q, norms.astype(np.float64))
    qt, it, dt = torch.from_numpy(q).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()
    full, w, logits = reference(q, idx, dist, norms, 0, labels, 0, BETA, metric)
    tol = tolerance(q, idx, dist, norms, 0, logits, k, BETA, metric, float(labels.max()))
    total = np.zeros_like(full)
    for ix, lo, rows in shards:
        got = ix.aggregate_partial_bigk(qt, it, dt, norms_all, beta=BETA, id_base=lo).cpu().numpy()
        part = reference(q, idx, dist, norms, 0, labels[lo:lo + rows], lo, BETA, metric)[0]
        err = np.abs(got - part).max(axis=1)
        assert (err <= tol).all(), f"shard at {lo} ({rows} rows): max err / bound {(err / tol).max():.2f}"
        if rows == 0:
            assert not got.any()
        total += got
    err = np.abs(total - full).max(axis=1)
    assert np.abs(full).max() > 0.1
    assert (err <= 3 * tol).all(), f"sum of the partials: max err / bound {(err / (3 * tol)).max():.2f}"


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("C,k,n", [(21, 300, 2000), (151, 1000, 2000), (21, 600, 450), (1000, 257, 200)])
def test_bigk_fused_search_equals_search_then_aggregate(cuda_device, C, k, n, metric):
    """search_aggregate_bigk (K4's passes -> K5 in one call) gives the bits of search + aggregate_bigk; banks with more rows than k and
    with fewer (the tail of every list is missing: id -1, weight 0)."""
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(C * 1000 + k)
    bank = _rows(n, rng)
    labels, _ = _labels(n, C, 196, rng)
    ix = HipFlatIndex(A.D, 0 if metric == "ip" else 1, 0)
    ix.add(torch.from_numpy(bank).cuda()); ix.add_labels(torch.from_numpy(labels).cuda()); ix.set_num_classes(C)
    q = torch.from_numpy(_queries(3.0, rng)).cuda()
    lh, idx, dist = ix.search_aggregate_bigk(q, k, want_neighbours=True)
    sidx, sdist = ix.search(q, k)
    assert torch.equal(idx, sidx) and torch.equal(dist.view(torch.int32), sdist.view(torch.int32))
    again = ix.aggregate_bigk(q, sidx, sdist)
    assert torch.equal(lh.view(torch.int32), again.view(torch.int32))
    assert torch.equal(ix.search_aggregate_bigk(q, k).view(torch.int32), lh.view(torch.int32))
    assert int((idx >= 0).sum()) == A.NQ * min(k, n) and bool((idx[:, min(k, n):] == -1).all())
    ref = reference(q.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), ix.copy_norms().cpu().numpy(), 0, labels, 0, 0.02, metric)[0]
    assert np.abs(lh.cpu().numpy() - ref).max() < 1e-3 and np.abs(ref).max() > 0.1     # (the bits above carry the claim; this guards against two equal wrongs)


def test_bigk_error_surface(cuda_device):
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(7)
    n, C = 300, 21
    ix = HipFlatIndex(A.D, 0, 0)
    ix.add(torch.from_numpy(_rows(n, rng)).cuda()); ix.add_labels(torch.from_numpy(_labels(n, C, 196, rng)[0]).cuda()); ix.set_num_classes(C)
    q = torch.from_numpy(_queries(1.0, rng)[:4]).cuda()
    idx = torch.randint(0, n, (4, 2049), device="cuda")
    dist = torch.rand((4, 2049), device="cuda")
    norms = ix.copy_norms()
    for k in (0, 2049):
        with pytest.raises(RuntimeError, match=r"hb_bigk_aggregate: k must be in \[1, 2048\]"):
            ix.aggregate_bigk(q, idx[:, :k], dist[:, :k])
        with pytest.raises(RuntimeError, match=r"hb_bigk_search_aggregate: k must be in \[1, 2048\]"):
            ix.search_aggregate_bigk(q, k)
        with pytest.raises(RuntimeError, match=r"hb_bigk_aggregate_partial: k must be in \[1, 2048\]"):
            ix.aggregate_partial_bigk(q, idx[:, :k], dist[:, :k], norms)
    for beta in (0.0, -0.02, float("nan")):
        with pytest.raises(RuntimeError, match="beta must be positive"):
            ix.aggregate_bigk(q, idx[:, :300], dist[:, :300], beta=beta)
        with pytest.raises(RuntimeError, match="beta must be positive"):
            ix.search_aggregate_bigk(q, 300, beta=beta)
        with pytest.raises(RuntimeError, match="beta must be positive"):
            ix.aggregate_partial_bigk(q, idx[:, :300], dist[:, :300], norms, beta=beta)
    bare = HipFlatIndex(A.D, 0, 0)
    bare.add(torch.from_numpy(_rows(n, rng)).cuda()); bare.set_num_classes(C)
    with pytest.raises(RuntimeError, match="label rows missing"):
        bare.search_aggregate_bigk(q, 300)
    with pytest.raises(RuntimeError, match="label rows missing"):
        bare.aggregate_bigk(q, idx[:, :300], dist[:, :300])
