"""What one search tells its nested searches travels in a per-call context (knn_call, csrc/hbird_knn.hip), not in fields of the index: ONE index
is taken through every nested path in turn -- the escalation of uncertified queries through a second fp16 pass into the fp32 kernel, the
passes of a search with k > 256 behind their ceilings, timed and untimed, ordering scores on and off -- and every result is held, as int32
words of ids and distances, to a second index pinned to the fp32 kernel.  A context that leaks from one call (a level, a seed, a ceiling, the
fp16 setting or the timing of a nested search, another call's ||q||^2) shows in the next.

After every search the index's reports (last_fp16_escalated, last_fp16_fallbacks, hb_last_search_path) are those of a fresh index given only
that search.  The one exception is the empty query set: hb_index_search returns for nq = 0 before it reaches the launcher, so that call must
leave the reports of the search before it untouched (a fresh index would report zeros; so it was before the context existed)."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(cuda_device):
    """The world of test_knn_gpu.py::test_use_fp16_escalation_second_pass_then_fp32: 60,000 x 128, planted near-duplicate clusters of 150 rows
    (wider than the first pass's k' = 64, settled by the second pass) and of 400 rows (wider than k' = 256: the fp32 kernel), 700 queries."""
    M, D = 60_000, 128
    rng = np.random.default_rng(11)
    bank = gi.unit_bank(M, D, seed=13)
    c1, c2 = bank[7].copy(), bank[8].copy()
    for r in range(1000, 1150):
        v = c1 + 1e-4 * rng.standard_normal(D).astype(np.float32); bank[r] = v / np.linalg.norm(v)
    for r in range(30_000, 30_400):
        v = c2 + 1e-4 * rng.standard_normal(D).astype(np.float32); bank[r] = v / np.linalg.norm(v)
    bank[40_000:40_003] = bank[1000]
    q = gi.vit_like_queries(700, D, seed=14)
    q[:60] = 4.0 * c1 + 1e-3 * rng.standard_normal((60, D)).astype(np.float32)
    q[60:100] = 4.0 * c2 + 1e-3 * rng.standard_normal((40, D)).astype(np.float32)
    return torch.from_numpy(bank).cuda(), torch.from_numpy(q).cuda()


def _reports(ix):
    return {"escalated": ix.last_fp16_escalated(), "fallbacks": ix.last_fp16_fallbacks(), "path": ix.last_search_path()}


@pytest.mark.parametrize("metric", ["dot_product", "l2"])
def test_nested_searches_leave_nothing_behind_in_the_index(world, metric):
    bank, q = world
    D, m = bank.shape[1], 0 if metric == "dot_product" else 1

    def index(fp16, timing=False):
        ix = HipFlatIndex(D, m, 0)
        ix.add(bank)
        ix.set_fp16(fp16)
        ix.set_timing(timing)
        return ix

    ix, ref = index(True), index(False)

    def step(what, k, queries=q, scores=False, timing=False, escalates=False):
        """One search on the index under test: bits against the pinned fp32 index, reports (and, timed, the work list) against a fresh index."""
        run = (lambda x: x.search_scores(queries, k)) if scores else (lambda x: x.search(queries, k))
        ix.set_timing(timing)
        gi_, gd = run(ix)
        ri, rd = run(ref)
        assert torch.equal(gi_, ri), what
        assert torch.equal(gd.view(torch.int32), rd.view(torch.int32)), what
        fresh = index(True, timing)
        run(fresh)
        got = _reports(ix)
        assert got == _reports(fresh), (what, got, _reports(fresh))
        if timing:
            assert ix.schedule_info() == fresh.schedule_info(), what
            assert ix.last_knn_ms() > 0.0, what
        if escalates:      # (what this world is known to do: both clusters fail the first certificate, the wide one the second too)
            assert 100 <= got["escalated"] <= 200 and got["fallbacks"] >= 40, (what, got)
            assert got["path"]["path"] == "fp16_chain", (what, got)
        fresh.close()
        return got

    step("1: k = 30, through levels 1 and 2", 30, escalates=True)
    step("2: k = 5", 5)
    big = step("3: k = 300, two passes behind a ceiling, timed", 300, timing=True)
    assert big["path"] == {"path": "fp32", "reason": "ceiling"} and big["escalated"] == 0 and big["fallbacks"] == 0, big
    step("4: k = 30 again, timed", 30, timing=True, escalates=True)
    step("5a: ordering scores", 30, scores=True, escalates=True)
    before = step("5b: ... and distances again", 30, escalates=True)
    gi_, gd = ix.search(q[:0], 30)                                      # 6: nq = 0 never reaches the launcher
    assert tuple(gi_.shape) == tuple(gd.shape) == (0, 30)
    assert _reports(ix) == before
    step("7: k = 30 once more", 30, escalates=True)
    ix.close(); ref.close()
