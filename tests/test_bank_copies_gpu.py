"""The lazy copies of the bank (csrc/hbird_mirror.h: the plain fp16 tiles of the candidate pass, the re-rank's row copy) through every event
of a bank's life, on the plain (uncentred) copy: appends that end inside a 32-row tile and that cross a 256-row bank tile, a capacity change
without rows, an append beyond the capacity, a reset with another bank, the row copy and the centred form switched off and on, views.
Index A (set_fp16(1), set_rerank_copy(1)) is held after every step, as ids and distance bits, to index B, which is pinned to the fp32 kernel
and receives the same rows; every search of A must have taken the candidate pass.

A 4,352 x 64 bank (17 bank tiles; from the first append on the row count is no multiple of 256 or 32), 300 queries, k = 10: 4,096 rows
are the least at which the second fp16 pass exists.  Near-duplicates of three query directions lie among the rows that steps 2, 3 and 5
append: a copy left behind -- those rows are zero in a stale fp16 copy -- loses neighbours at the head of the list, not far down it; that
the planted rows ARE the head is checked with a numpy fp32 top-k."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

M, D, K, NQ = 4352, 64, 10, 300
CAP = 5120
STEP2 = list(range(4352, 4357))                                   # the planted rows, by the step that appends them
STEP3 = list(range(4357, 4361)) + list(range(4606, 4610))


def _near(c, n, rng):
    v = c[None, :] + 1e-2 * rng.standard_normal((n, D)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _world():
    rng = np.random.default_rng(31)
    dirs = gi.unit_bank(3, D, seed=32)
    q = gi.vit_like_queries(NQ, D, seed=33)
    for j in range(3):      # queries 10 j .. 10 j + 9 aim at direction j
        q[10 * j:10 * j + 10] = 4.0 * dirs[j] + 1e-3 * rng.standard_normal((10, D)).astype(np.float32)
    bank = gi.unit_bank(M, D, seed=34)
    step2 = _near(dirs[0], 5, rng)                                            # 4,352 -> 4,357: inside row tile 136
    # -> 4,657: planted rows in the tile step 2 left partly filled (4,357 ..) and on both sides of bank tile 18's start (4,608)
    step3 = gi.unit_bank(300, D, seed=35); step3[0:4] = _near(dirs[1], 4, rng); step3[249:253] = _near(dirs[1], 4, rng)
    step5 = gi.unit_bank(6000, D, seed=36); step5[5579:5587] = _near(dirs[2], 8, rng)   # -> 10,657 > 10,240: the planted rows across the old capacity
    other = -gi.unit_bank(4400, D, seed=37); other[4395:4400] = _near(dirs[0], 5, rng)  # the bank after the reset
    return q, bank, step2, step3, step5, other


def _same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def _head(rows_h, q_h, j):
    """numpy fp32 top-k (inner product) of the queries that aim at direction j -> the set of row ids in their lists"""
    s = q_h[10 * j:10 * j + 10] @ np.concatenate(rows_h).T
    return set(np.argsort(-s, axis=1, kind="stable")[:, :K].ravel().tolist())


def test_the_copies_follow_the_bank_through_its_life(cuda_device):
    q_h, bank_h, step2, step3, step5, other = _world()
    q = torch.from_numpy(q_h).to(cuda_device)
    a, b = HipFlatIndex(D, 0, 0), HipFlatIndex(D, 0, 0)
    opened = [a, b]
    try:
        a.set_fp16(1); a.set_rerank_copy(1)
        b.set_fp16(False)
        rows_h = []

        def add(x):
            rows_h.append(x)
            t = torch.from_numpy(x).to(cuda_device)
            a.add(t); b.add(t)

        def held(what, ia=a, ib=b):
            got, want = ia.search(q, K), ib.search(q, K)
            assert _same(got, want), what
            assert ia.last_search_path()["path"] == "fp16_chain", (what, ia.last_search_path())
            return got

        def planted(j, rows, what):
            """the planted rows are in the numpy lists of direction j's queries, and in A's"""
            want = set(rows)
            assert want <= _head(rows_h, q_h, j), what
            assert want <= set(a.search(q[10 * j:10 * j + 10], K)[0].cpu().numpy().ravel().tolist()), what

        # 1: build and search
        for x in (a, b):
            x.reserve(CAP)
        add(bank_h)
        held("1: built")
        assert a.rerank_copy_bytes() == CAP * D * 4
        # 2: five rows inside the capacity, ending inside a 32-row tile
        add(step2)
        assert a.ntotal == 4357
        held("2: 5 rows")
        planted(0, STEP2, "2")
        # 3: 300 more inside the capacity, crossing a 256-row bank tile
        add(step3)
        assert a.ntotal == 4657 and a.ntotal < CAP
        held("3: 300 rows")
        planted(1, STEP3, "3")
        planted(0, STEP2, "3: the rows of step 2")
        # 4: twice the capacity, no rows added: the copies are made anew for it by the next search
        for x in (a, b):
            x.reserve(2 * CAP)
        held("4: reserve")
        assert a.rerank_copy_bytes() == 2 * CAP * D * 4
        planted(0, STEP2, "4"); planted(1, STEP3, "4")
        # 5: an append beyond that capacity
        add(step5)
        assert a.ntotal == 10657 and a.ntotal > 2 * CAP
        held("5: beyond the capacity")
        assert a.rerank_copy_bytes() >= a.ntotal * D * 4
        planted(2, range(4657 + 5579, 4657 + 5587), "5")
        planted(0, STEP2, "5: the rows of step 2"); planted(1, STEP3, "5: the rows of step 3")
        # 6: reset, then another bank: the answers are rows of the new bank
        a.reset(); b.reset()
        rows_h.clear()
        add(other)
        got = held("6: another bank after reset")
        assert int(got[0].max()) < 4400 and int(got[0].min()) >= 0
        planted(0, range(4395, 4400), "6")
        # 7: the row copy off, then on
        a.set_rerank_copy(2)
        held("7a: without the row copy")
        assert a.rerank_copy_bytes() == 0
        a.set_rerank_copy(1)
        held("7b: with the row copy again")
        assert a.rerank_copy_bytes() > 0
        # 8: the centred form on, then off
        a.set_fp16_centre(True)
        held("8a: centred")
        a.set_fp16_centre(False)
        held("8b: plain again")
        assert a.last_search_path().get("centred", False) is False
        planted(0, range(4395, 4400), "8")
        # 9: a view of every second row, then the rest appended to it in two parts
        even = torch.arange(0, 4400, 2, device=cuda_device)
        odd = torch.arange(1, 4400, 2, device=cuda_device)
        va, vb = a.select_rows(even), b.select_rows(even)
        opened += [va, vb]
        va.set_fp16(1); va.set_rerank_copy(1); vb.set_fp16(False)
        # (2,200 rows: below the 4,096 of a second pass, the candidate pass runs all the same under set_fp16(1))
        held("9a: view", va, vb)
        for part in (odd[:777], odd[777:]):
            va.add_from(a, part); vb.add_from(b, part)
            held("9b: view after add_from", va, vb)
        assert va.ntotal == 4400
        order = torch.cat([even, odd]).cpu().numpy()
        got = va.search(q[:10], K)[0].cpu().numpy()
        assert set(range(4395, 4400)) <= set(order[got.ravel()].tolist())      # the planted rows, by their ids in the source
    finally:
        for x in opened:
            x.close()
