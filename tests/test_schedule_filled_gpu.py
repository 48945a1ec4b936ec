"""The filled clustered work list (hb_index_set_cluster_sharing(ix, 3)) under the fp16 candidate kernel: segments of one launch stride by
1, 2, 4 or 8 bank tiles and the members of a cluster change their query and bank ways from row to row.  A stride or clock error names wrong
rows or drops pairs, so HipFlatIndex.last_screen() is held to the exact worlds of tests/f16_pass_refs.py (rows and score BITS of the kc best,
ties by lower row) for every query, and every search to the fp32 kernel's ids and distance bits.

Bank 20,000 x 64 (79 bank tiles), 64 workgroups; 1,553 queries (7 query tiles: as 4 x 2 one full group, a 2 x 4 row and a 1 x 8 row; as
8 x 1 fewer tiles than query ways: the list of old), 2,816 (11: r = 3), 3,584 (14: r = 6 as 8 x 1, r = 2 as 4 x 2), 512 (2: the list of old);
k = 30 (k' = 64: <4>) and 90 (k' = 184: <8>); phases on and off; both metrics.  One 300,000 x 768 x 21,904-query search (86 query tiles) with
the sharing mode left automatic."""
import collections
import functools

import numpy as np
import pytest
import torch

import f16_pass_refs as R
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

N, D, G = 20_000, 64, 64
Case = collections.namedtuple("Case", "nq shape k metric phases filled")
CASES = [
    Case(1553, (4, 2), 30, 1, True, 1),
    Case(1553, (4, 2), 90, 0, False, 1),
    Case(1553, (8, 1), 30, 0, True, 0),
    Case(2816, (8, 1), 90, 1, True, 1),
    Case(2816, (4, 2), 30, 0, False, 1),
    Case(3584, (8, 1), 30, 0, True, 1),
    Case(3584, (8, 1), 90, 1, False, 1),
    Case(3584, (4, 2), 90, 1, True, 1),
    Case(512, (8, 1), 30, 1, True, 0),
    Case(512, (4, 2), 90, 0, False, 0),
]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@functools.lru_cache(maxsize=None)
def _world(nq, kc):
    return R.exact_world(N, D, nq, kc, 31, 0, 0.0)


@functools.lru_cache(maxsize=None)
def _reference(nq, kc, metric, dev):
    """The kc best of every query by (score descending, row ascending) on the world's integers -> rows [nq, kc], pass scores float32 [nq, kc]:
    R.exact_scores2 / R.exact_lists in one stable sort on the device (float64 products of small integers are exact)."""
    W = _world(nq, kc)
    qi = torch.from_numpy(W["queries_i"]).to(dev).double()
    bi = torch.from_numpy(W["bank_i"]).to(dev).double()
    s2 = 2.0 * (qi @ bi.T)
    if metric == 1:
        s2 -= (bi * bi).sum(dim=1)[None, :]
    assert float(s2.abs().max()) < 2 ** 15
    val, rows = torch.sort(-s2, dim=1, stable=True)
    return rows[:, :kc].cpu().numpy(), (-0.5 * val[:, :kc]).float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fp32_answer(nq, kc, k, metric, dev):
    W = _world(nq, kc)
    held = HipFlatIndex(D, metric, 0)
    held.set_fp16(False)
    held.add(torch.from_numpy(W["bank"]).to(dev))
    want = held.search(torch.from_numpy(W["queries"]).to(dev), k)
    assert held.last_search_path()["path"] == "fp32"
    held.close()
    return want


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"nq{c.nq}-{c.shape[0]}x{c.shape[1]}-k{c.k}-m{c.metric}-{'phased' if c.phases else 'unphased'}")
def test_filled_lists_rows_score_bits_and_the_fp32_answer(cuda_device, c):
    kc = R.kc_of(c.k)
    W = _world(c.nq, kc)
    dev = str(cuda_device)
    ix = HipFlatIndex(D, c.metric, 0)
    ix.set_fp16(True); ix.set_fp16_escalation(False)
    ix.set_tuning(workgroups=G)
    ix.set_cluster(*c.shape); ix.set_cluster_sharing(3)
    if not c.phases:
        ix.set_search_options(phases=False)
    ix.add(torch.from_numpy(W["bank"]).to(cuda_device))
    got = ix.search(torch.from_numpy(W["queries"]).to(cuda_device), c.k)
    L = ix.last_screen()
    info = ix.schedule_info()
    print("FILLED", c, info)
    assert ix.last_search_path()["path"] == "fp16_chain"
    assert (L["nq"], L["kc"], L["klw"]) == (c.nq, kc, {30: 192, 90: 384}[c.k])
    nqt = (c.nq + 255) // 256
    assert info["workgroups"] == G and info["cluster"] == list(c.shape) and info["query_tiles"] == nqt and info["bank_tiles"] == 79
    assert info["filled"] == c.filled and "fill_refused" not in info, info
    CS = c.shape[0] * c.shape[1]
    if c.filled:      # a partial last unit per leftover row: fewer idle member ticks than the ragged group's ways alone would be
        assert info["idle_member_ticks"] < CS * 3 and info["member_ticks"] < (-(-nqt // c.shape[0]) * c.shape[0]) * 79
    else:
        assert info["idle_member_ticks"] >= (c.shape[0] - nqt % c.shape[0]) % c.shape[0] * 79 // c.shape[1]
    rows, scores = _reference(c.nq, kc, c.metric, dev)
    assert np.array_equal(L["rows"], rows), f"{c}: {int((L['rows'] != rows).any(axis=1).sum())} queries with other candidate rows, first {np.argwhere(L['rows'] != rows)[:3].tolist()}"
    assert np.array_equal(np.asarray(L["scores"]).view(np.uint32), scores.view(np.uint32)), f"{c}: pass score bits differ"
    assert _same(got, _fp32_answer(c.nq, kc, c.k, c.metric, dev)), f"{c}: the screened search differs from the fp32 kernel's answer"
    ix.close()


def test_headline_query_tiles_fill_by_themselves(cuda_device):
    """86 query tiles as 8 x 1 with the sharing mode left automatic: the candidate pass shares and fills (a 4 x 2 and a 2 x 4 row), and the
    answer is the fp32 kernel's.  (300,000 rows are below the size from which the clusters come by themselves: the shape is given.)"""
    M, Dh, nq, k = 300_000, 768, 21_904, 30
    g = torch.Generator(device=cuda_device); g.manual_seed(17)
    bank = torch.nn.functional.normalize(torch.randn((M, Dh), generator=g, device=cuda_device), dim=1)
    q = torch.randn((nq, Dh), generator=g, device=cuda_device)
    held = HipFlatIndex(Dh, 0, 0); held.set_fp16(False); held.add(bank)
    want = held.search(q, k)
    held.close()
    ix = HipFlatIndex(Dh, 0, 0)
    ix.set_fp16(True)
    ix.set_cluster(8, 1)
    ix.add(bank)
    got = ix.search(q, k)
    info = ix.schedule_info()
    print("FILLED headline tiles", info, ix.last_search_path())
    assert ix.last_search_path()["path"] == "fp16_chain"
    assert info["query_tiles"] == 86 and info["cluster"] == [8, 1] and info["workgroups"] == 256
    assert info["filled"] == 1 and info["idle_member_ticks"] * 500 < info["member_ticks"], info
    assert info["max_slots_per_qtile"] == 16
    assert _same(got, want)
    ix.close()
