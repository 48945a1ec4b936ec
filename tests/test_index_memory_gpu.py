"""Every device allocation of an index is a member of one owning type (csrc/hbird_devbuf.h), and hb_debug_live_allocations counts what is
live, exact to the byte.  Indexes on a 16,384 x 64 bank are taken through every site that allocates, grows, moves or drops a buffer -- the
fp16 candidate pass with its second pass and the fp32 search of what is left (fb, fb1, stamp_keep, cand, q16, copy16.tiles, row_copy.rows), the centred
copy on and off, k > 256, a larger query batch, an append beyond the capacity, label rows as counts, as fp32 and of another width, an
excluding search through its second rung, views, dropping the re-rank copy -- and every search is held, as int32 words of ids and
distances, to an index pinned to the fp32 kernel that is taken through the same appends.  After close() on every index, views included,
the live count and the live bytes are exactly what they were before the first index."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import golden_inputs as gi
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

M, D, K = 16_384, 64, 10


def _live():
    count, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.lib().hb_debug_live_allocations(ctypes.byref(count), ctypes.byref(nbytes)))
    return int(count.value), int(nbytes.value)


def _world():
    """Unit rows with two planted near-duplicate clusters: 150 rows (wider than the first pass's k' = 64: settled by the second fp16 pass) and
    300 rows (wider than k' = 256: the fp32 kernel, and -- as one row group -- more than a first rung of 256 holds: the second rung).  The
    first 40 queries aim at the first cluster, the next 20 at the second."""
    rng = np.random.default_rng(21)
    bank = gi.unit_bank(M, D, seed=23)
    c1, c2 = bank[7].copy(), bank[8].copy()
    for r in range(1000, 1150):
        v = c1 + 1e-4 * rng.standard_normal(D).astype(np.float32); bank[r] = v / np.linalg.norm(v)
    for r in range(9000, 9300):
        v = c2 + 1e-4 * rng.standard_normal(D).astype(np.float32); bank[r] = v / np.linalg.norm(v)
    q = gi.vit_like_queries(3300, D, seed=24)
    q[:40] = 4.0 * c1 + 1e-3 * rng.standard_normal((40, D)).astype(np.float32)
    q[40:60] = 4.0 * c2 + 1e-3 * rng.standard_normal((20, D)).astype(np.float32)
    more = gi.unit_bank(5000, D, seed=25)
    return bank, more, q


def _same(got, want, what):
    assert torch.equal(got[0], want[0]), what
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), what


def test_every_owning_site_and_nothing_left_after_close(cuda_device):
    gc.collect()      # (an index another test left to the collector goes now, not between the two readings)
    count0, bytes0 = _live()
    bank_h, more_h, q_h = _world()
    bank, q = torch.from_numpy(bank_h).cuda(), torch.from_numpy(q_h).cuda()
    q300, q3000 = q[:300], q[300:]

    ref = HipFlatIndex(D, 0, 0); ref.set_fp16(False); ref.add(bank)      # the oracle: the fp32 kernel, whatever the search
    ix = HipFlatIndex(D, 0, 0); ix.set_fp16(1); ix.set_rerank_copy(1); ix.set_timing(True); ix.add(bank)
    opened = [ref, ix]
    try:
        count1, bytes1 = _live()
        assert count1 > count0 and bytes1 - bytes0 >= 2 * M * D * 4

        def step(what, k=K, queries=q300):
            _same(ix.search(queries, k), ref.search(queries, k), what)

        # the candidate pass, its second pass (the 150-row cluster) and the fp32 search of what is left (the 300-row cluster)
        step("1: fp16 chain")
        assert ix.last_search_path()["path"] == "fp16_chain"
        assert ix.last_fp16_escalated() > 0 and ix.last_fp16_fallbacks() > 0
        assert ix.rerank_copy_bytes() > 0
        ix.set_fp16_centre(True); step("2a: centred copy")
        ix.set_fp16_centre(False); step("2b: plain copy again")
        step("3: k = 300", k=300)
        step("4: 3,000 queries after 300", queries=q3000)
        step("4b: ... and the 300 again")
        ix.add(more_h); ref.add(more_h)      # host rows, beyond the capacity: the bank moves, the copies follow at the next search
        assert ix.ntotal == M + 5000
        step("5: after the append")
        _same(tuple(torch.from_numpy(a) for a in ix.search(q_h[:50], K)), tuple(t.cpu() for t in ref.search(q300[:50], K)), "5b: host queries")

        # label rows: counts of values j / 16, then the same rows as fp32
        C = 5
        lab = torch.from_numpy(gi.labels_from_masks(M + 5000, C, 16, seed=26)).cuda()
        for x in (ix, ref):
            x.set_label_denominator(16); x.add_labels(lab); x.set_num_classes(C)

        def step_labels(what):
            got, want = ix.search_aggregate(q300, K, want_neighbours=True), ref.search_aggregate(q300, K, want_neighbours=True)
            _same(got[1:], want[1:], what)
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), what
            return got[0]

        as_counts = step_labels("6a: count rows")
        ids = torch.arange(0, M + 5000, 97)
        assert np.array_equal(ix.gather_labels(ids.numpy()), lab[ids.cuda()].cpu().numpy())
        ix.labels_to_fp32(); ref.labels_to_fp32()
        assert ix.label_denominator == 0
        as_fp32 = step_labels("6b: the same rows as fp32")
        assert torch.allclose(as_counts, as_fp32, rtol=0.0, atol=1e-6)      # (the stored values are the same fp32 numbers; K5 adds them in another order)

        # an emptied index takes label rows of another width
        C = 7
        lab = torch.from_numpy(gi.labels_from_masks(M, C, 16, seed=27)).cuda()
        for x in (ix, ref):
            x.reset(); x.add(bank); x.add_labels(lab); x.set_num_classes(C)
        step_labels("7: after reset, C = 7")

        # one excluded row group per query: the 300-row cluster as ONE group sends its queries to the second rung
        groups = (np.arange(M, dtype=np.int32) // 64) + 1
        groups[9000:9300] = 0
        qg = torch.full((300,), -1, dtype=torch.int32); qg[40:60] = 0; qg[100:200] = torch.arange(100, 200, dtype=torch.int32)
        for x in (ix, ref):
            x.set_row_groups(groups)
        _same(ix.search_excluding(q300, K, qg.cuda()), ref.search_excluding(q300, K, qg.cuda()), "8: excluding")
        info = ix.last_exclusion()
        assert info["rungs"] == 2 and info["rung1_queries"] >= 20 and info["gmax"] == 300, info

        # views: rows gathered into a new index, then appended beyond its capacity
        first, second = torch.arange(0, M, 2).cuda(), torch.arange(1, M, 4).cuda()
        view, ref_view = ix.select_rows(first), ref.select_rows(first)
        opened += [view, ref_view]
        view.set_fp16(1); ref_view.set_fp16(False)
        _same(view.search(q300, K), ref_view.search(q300, K), "9a: view")
        view.add_from(ix, second); ref_view.add_from(ref, second)
        assert view.ntotal == M // 2 + M // 4
        got, want = view.search_aggregate(q300, K, want_neighbours=True), ref_view.search_aggregate(q300, K, want_neighbours=True)
        _same(got[1:], want[1:], "9b: view after add_from")
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))

        # the re-rank's row copy goes; the searches go on without it
        ix.set_rerank_copy(2)
        assert ix.rerank_copy_bytes() == 0
        step("10: without the row copy")
        assert _live()[1] > bytes0
    finally:
        for x in opened:
            x.close()
    assert _live() == (count0, bytes0)
