"""The fp16 screen's certificate on the GPU, on banks built to break it (tests/f16_screen_worlds.py; what those banks promise is checked on
the CPU in tests/test_f16_certificate_cpu.py).  Every check compares indices and distance BITS with oracle.knn_chain_f32 for the planted (or the
first few) queries and with the same index held at set_fp16(0) for all queries.  rounding_world's hidden rows are true neighbours that the
fp16 pass ranks below more than k' decoys, by a margin of 0.79 - 0.91 E: a certificate whose bound were 25 % too small (35 % at D = 768) passes
some of these queries and returns a decoy in a hidden row's place, so equality here is a statement about E, the skip rule `cut`, the second
pass's floor and its "a list that does not fill up is complete" rule.  The counts hold the other side: every query whose hidden neighbour is no
candidate (by the CPU model) must have failed its first certificate.  (The skip rule: with n_decoys < k' -- and in every second pass -- a
hidden row IS a candidate, at a list position beyond k and an fp16 score 0.79 - 0.91 E below the k-th candidate's.  That is as far below as one
query's rows can fall against each other -- both roundings of the row, the query's are shared --, so `cut`'s 2 E itself cannot be met.)

Each world prints one line `F16WORLD {json}` with the escalated / fallback shares (profiles/r08/fp16_certificate_worlds.json keeps them)."""
import json

import numpy as np
import pytest
import torch

import f16_screen_worlds as fw
import oracle
from hbird_mi.nn.search_hip import HipFlatIndex, merge_topk

pytestmark = pytest.mark.gpu

GAPS = (0.5, 0.7, 0.8, 0.9, 0.95)
METRIC_NAME = {0: "dot_product", 1: "l2"}
NQ_BIG = 21_904       # 86 query tiles: 300,000 x 768 is a "big" search for the automatic state (tests/test_exact_screen_gpu.py)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _index(bank, metric, fp16=None, rerank=None, escalation=None):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.add(bank)
    if fp16 is not None:
        ix.set_fp16(fp16)
    if rerank is not None:
        ix.set_rerank_copy(rerank)
    if escalation is not None:
        ix.set_fp16_escalation(escalation)
    return ix


def _assert_oracle(got, q_np, bank_np, k, metric, rows, what):
    """got: (idx, dist) CUDA tensors of ALL queries; the oracle answers for the queries `rows`."""
    ridx, rdist = oracle.knn_chain_f32(q_np[rows], bank_np, k, METRIC_NAME[metric])
    gi_, gd = got[0][rows].cpu().numpy(), got[1][rows].cpu().numpy()
    bad = np.nonzero((gi_ != ridx).any(axis=1))[0]
    assert bad.size == 0, f"{what}: query {rows[bad[0]]} returns ids that differ from the fp32 definition: got {sorted(set(gi_[bad[0]]) - set(ridx[bad[0]]))} " \
                          f"in place of {sorted(set(ridx[bad[0]]) - set(gi_[bad[0]]))}"
    assert np.array_equal(gd.view(np.uint32), rdist.view(np.uint32)), f"{what}: distance bits differ from the oracle's"


def _model_failures(W, k, kc, metric, bank=None):
    """Planted queries whose true top-k is NOT within the fp16 top-kc (CPU model): a sound first certificate fails each of them."""
    G = W["n_groups"]
    m = fw.screen_model(W["queries"][:G], W["bank"] if bank is None else bank, k, kc, metric)
    return int((~m["contained"]).sum())


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k", [30, 90])
@pytest.mark.parametrize("D", [64, 384, 768])
def test_rounding_world_through_the_forced_screen(cuda_device, D, k, metric):
    kc = min(256, max(64, (2 * k + 7) // 8 * 8))
    assert kc == {30: 64, 90: 184}[k]
    for n_decoys in (100, 200, 300):
        W = fw.rounding_world(D, k, kc, 10, n_decoys, GAPS, metric=metric, seed=1000 + D + 7 * k + metric + n_decoys, n_background=2500,
                              n_queries_background=54)
        G = W["n_groups"]
        need = _model_failures(W, k, kc, metric)
        assert need == (G if n_decoys >= kc else 0)          # (the CPU file holds the builder to this)
        bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
        held = _index(bank, metric, fp16=0)
        want = held.search(q, k)
        assert held.last_search_path()["path"] == "fp32"
        _assert_oracle(want, W["queries"], W["bank"], k, metric, np.arange(G), "fp32 kernel")
        for rerank in (1, 2):
            for escalation in (True, False):
                what = f"D={D} k={k} metric={metric} n_decoys={n_decoys} rerank_copy={rerank} escalation={escalation}"
                ix = _index(bank, metric, fp16=1, rerank=rerank, escalation=escalation)
                got = ix.search(q, k)
                assert ix.last_search_path() == {"path": "fp16_chain", "reason": "explicit_fp16"}, what
                assert (ix.rerank_copy_bytes() > 0) == (rerank == 1), what
                esc, fb = ix.last_fp16_escalated(), ix.last_fp16_fallbacks()
                _assert_oracle(got, W["queries"], W["bank"], k, metric, np.arange(G), what)
                assert _same(got, want), f"{what}: differs from the fp32 kernel's answer"
                assert esc >= need, f"{what}: {esc} first certificates failed, {need} queries have a true neighbour outside the candidates"
                if n_decoys == 300 or not escalation:
                    assert fb >= need, f"{what}: {fb} queries reached the fp32 kernel, {need} cannot be certified by any fp16 pass"
                ix.close()
        held.close()


def _planted_big_bank(dev, D, k, kc, metric, M, seed):
    """A rounding_world's groups scattered over a bank of M rows whose background is drawn on the device (same law as the builder's: N(0,1) rows
    at the groups' norm) -> (bank CUDA, queries CUDA [NQ_BIG], W with the ids of the big bank, bank on the host)."""
    W = fw.rounding_world(D, k, kc, 16, 300, GAPS, metric=metric, seed=seed, n_background=0)
    G, n_grp = W["n_groups"], W["bank"].shape[0]
    norm = float(np.sqrt((W["bank"][W["hidden_ids"][0][0]].astype(np.float64) ** 2).sum()))
    g = torch.Generator(device=dev); g.manual_seed(seed)
    bank = torch.nn.functional.normalize(torch.randn((M, D), generator=g, device=dev), dim=1) * norm
    pos = np.sort(np.random.default_rng(seed).permutation(M)[:n_grp])
    bank[torch.from_numpy(pos).to(dev)] = torch.from_numpy(W["bank"]).to(dev)
    q = torch.nn.functional.normalize(torch.randn((NQ_BIG, D), generator=g, device=dev), dim=1)
    where = np.random.default_rng(seed + 1).permutation(NQ_BIG)[:G]                       # the planted queries, spread over the query tiles
    q[torch.from_numpy(where).to(dev)] = torch.from_numpy(W["queries"][:G]).to(dev)
    W = dict(W, hidden_ids=[pos[h] for h in W["hidden_ids"]], group_ids=[pos[r] for r in W["group_ids"]])
    return bank, q, W, where


def test_rounding_world_under_the_automatic_state(cuda_device):
    D, k, kc, M = 768, 30, 64, 300_000
    bank, q, W, where = _planted_big_bank(cuda_device, D, k, kc, 0, M, seed=4242)
    bank_np, q_np = bank.cpu().numpy(), q.cpu().numpy()
    m = fw.screen_model(q_np[where], bank_np[np.concatenate(W["group_ids"])], k, kc, 0)      # (the background is far below: asserted via the oracle)
    need = int((~m["contained"]).sum())
    assert need == W["n_groups"]
    auto, held = _index(bank, 0), _index(bank, 0, fp16=0)
    want = held.search(q, k)
    _assert_oracle(want, q_np, bank_np, k, 0, where, "fp32 kernel")
    for i, hid in enumerate(W["hidden_ids"]):
        assert np.isin(hid, want[0][where[i]].cpu().numpy()).all()
    seen = []
    for n in range(4):
        got = auto.search(q, k)
        seen.append((auto.last_search_path(), auto.last_fp16_escalated(), auto.last_fp16_fallbacks()))
        if n == 0:
            assert auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"}
            assert auto.last_fp16_escalated() >= need and auto.last_fp16_fallbacks() >= need
        assert _same(got, want), f"search {n} ({seen}) differs from the fp32 kernel's answer"
    print("F16WORLD " + json.dumps({"world": "rounding_world", "rows": M, "dim": D, "queries": NQ_BIG, "state": "auto", "planted": need, "searches": seen}))


def test_bmax_follows_the_bank(cuda_device):
    """E takes the largest row norm of the bank: rows of 8 x the norm arrive with add() -- a stale bmax would make E eight times too small for
    them -- and leave with reset()."""
    D, k, kc = 384, 30, 64
    small = fw.rounding_world(D, k, kc, 10, 300, GAPS, seed=77, n_background=6000, n_queries_background=54)
    large = fw.rounding_world(D, k, kc, 10, 300, GAPS, seed=77, n_background=6000, n_queries_background=54, bank_scale=8.0)
    assert np.array_equal(small["queries"], large["queries"])
    G = small["n_groups"]
    both = np.concatenate([small["bank"], large["bank"]])
    need_small = _model_failures(small, k, kc, 0)
    need_both = _model_failures(small, k, kc, 0, bank=both)
    assert need_small == G and need_both == G
    q = torch.from_numpy(small["queries"]).to(cuda_device)
    for rerank in (1, 2):
        ix, held = HipFlatIndex(D, 0, 0), HipFlatIndex(D, 0, 0)
        ix.set_fp16(1); ix.set_rerank_copy(rerank); held.set_fp16(0)
        for step, (rows, ref, need) in enumerate(((small["bank"], small["bank"], need_small), (large["bank"], both, need_both), (None, small["bank"], need_small))):
            if rows is None:
                ix.reset(); held.reset()
                rows = small["bank"]
            ix.add(torch.from_numpy(rows).to(cuda_device)); held.add(torch.from_numpy(rows).to(cuda_device))
            assert ix.ntotal == ref.shape[0]
            got, want = ix.search(q, k), held.search(q, k)
            what = f"step {step} rerank_copy={rerank}"
            assert ix.last_search_path()["path"] == "fp16_chain"
            _assert_oracle(got, small["queries"], ref, k, 0, np.arange(G), what)
            assert _same(got, want), what
            assert ix.last_fp16_escalated() >= need and ix.last_fp16_fallbacks() >= need, (what, ix.last_fp16_escalated(), ix.last_fp16_fallbacks())
            if step == 1:      # the answers are rows of the appended world
                assert (got[0][:G].cpu().numpy() >= small["bank"].shape[0]).all()
        ix.close(); held.close()


def _vit_case(dev, name, W, metric, fp16, k=30, searches=1):
    (N, D), nq = W["bank"].shape, W["queries"].shape[0]
    bank, q = torch.from_numpy(W["bank"]).to(dev), torch.from_numpy(W["queries"]).to(dev)
    held = _index(bank, metric, fp16=0)
    want = held.search(q, k)
    _assert_oracle(want, W["queries"], W["bank"], k, metric, np.arange(16), f"{name}: fp32 kernel")
    ix = _index(bank, metric, fp16=fp16)
    seen = []
    for n in range(searches):
        got = ix.search(q, k)
        seen.append((ix.last_search_path(), ix.last_fp16_escalated(), ix.last_fp16_fallbacks()))
        assert _same(got, want), f"{name} {N} x {D} metric={metric} search {n} {seen}: differs from the fp32 kernel's answer"
    print("F16WORLD " + json.dumps({"world": name, "rows": N, "dim": D, "queries": nq, "metric": METRIC_NAME[metric], "state": "auto" if fp16 is None else "set_fp16(1)",
                                    "escalated_share": seen[0][1] / nq, "fallback_share": seen[0][2] / nq, "searches": seen}))
    ix.close(); held.close()
    return seen


@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("name", sorted(fw.VIT_WORLDS))
def test_vit_shaped_worlds_through_the_forced_screen(cuda_device, name, D):
    W = fw.VIT_WORLDS[name](60_000, D, 1024, seed=31)
    for metric in (0, 1):
        seen = _vit_case(cuda_device, name, W, metric, fp16=1)
        assert seen[0][0] == {"path": "fp16_chain", "reason": "explicit_fp16"}


def test_a_vit_shaped_world_under_the_automatic_state(cuda_device):
    seen = _vit_case(cuda_device, "massive_activation", fw.massive_activation_world(300_000, 768, NQ_BIG, seed=31), 0, fp16=None, searches=4)
    assert seen[0][0] == {"path": "fp16_chain", "reason": "auto"}


@pytest.mark.parametrize("metric", [0, 1])
def test_rounding_world_cut_into_row_shards(cuda_device, metric):
    """Hidden rows and decoys of a group in different shards; each shard its own index at set_fp16(1) with successive ids, the per-shard ordering
    scores merged by hb_merge_topk: the single index's bits."""
    D, k, kc = 384, 30, 64
    W = fw.rounding_world(D, k, kc, 10, 300, GAPS, metric=metric, seed=5150 + metric, n_background=20_000, n_queries_background=54)
    M, G = W["bank"].shape[0], W["n_groups"]
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    single = _index(torch.from_numpy(W["bank"]).to(cuda_device), metric, fp16=1)
    ref = single.search(q, k)
    _assert_oracle(ref, W["queries"], W["bank"], k, metric, np.arange(G), "single index")
    assert single.last_fp16_escalated() >= G
    for parts in (2, 4):
        per = (M + parts - 1) // parts
        for i in range(G):      # the world does what the test is about
            assert len(set((W["group_ids"][i] // per).tolist())) == parts, "a group's decoys must lie in every shard"
        idxs, scs = [], []
        for p in range(parts):
            lo, hi = p * per, min(M, (p + 1) * per)
            sh = _index(torch.from_numpy(W["bank"][lo:hi]).to(cuda_device), metric, fp16=1)
            i_, s_ = sh.search_scores(q, k, id_base=lo)
            assert sh.last_search_path()["path"] == "fp16_chain"
            idxs.append(i_); scs.append(s_)
            sh.close()
        im, dm = merge_topk(torch.stack(scs), torch.stack(idxs), 0)
        dm = single.distances_from_scores(q, dm.contiguous())
        assert _same((im, dm), ref), f"{parts} shards"
    single.close()
