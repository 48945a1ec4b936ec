"""The conversion behind the centred fp16 screen (csrc/hbird_f16_centre.hip: centre_row_valid / _colsum / _mean / _bank / _query_dot / _t /
_query / _init16) held to the definitions of tests/f16_centre_refs.py on its OWN output, read through HipFlatIndex.last_centre()
(hb_index_last_centre): mu, mu.mu, ||mu||, g, cmax, the fp16 tiles of bank and queries, c_q, t, ||q - t mu|| and init16 -- bits wherever the
definition determines them, the derived float64 summation tolerance for mu and t on float worlds.  Final ids and distance bits come out
right whatever the conversion did (an uncertified query is searched again), so every search here is ALSO compared with an index held at
set_fp16(0): a failure says which layer broke.

Everything runs in mode set_fp16(True) with set_fp16_centre(True).  The scenarios are those of f16_centre_refs.py -- the ones
tests/test_f16_centre_readout_cpu.py runs on its host model and on the wrong variants of it:

    fresh            1,000 x 40 | 1,000 x 128 | 5,000 x 136 | 20,000 x 64; a massive-activation-like float world and an exact world each
                     (what each shape reaches: the case-list guard of the CPU file)
    invalid rows     NaN rows (row 0, first tile, last tile): skipped by mean and count, nothing for cmax; one +inf component: cmax = +inf
    append, capacity, reset     rows behind an existing copy under the same mu (a partial tile converted again, rows of 8 x the norm);
                     mu anew beyond the reservation and after reset(); no cmax left over from the big rows
    two searches     t, init16 and the query side after the second search are the second search's
    query shapes     nq = 1, 70, 300; one query with a NaN component
    second pass      level 1, n = the failing queries, their c_q and ||q - t mu|| gathered in ascending order, t and init16 untouched
    zero mean        no centred copy: the read-out refuses
    view             a select_rows view derives the mean of ITS rows
    shards           a HipMultiIndex over two and three unequal row shards: every shard's conversion against ITS rows"""
import numpy as np
import pytest
import torch

import f16_centre_refs as R
import f16_pass_refs as P
import test_f16_centre_cpu as cm
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu


class _Screened:
    """A centred screened index and its twin held at set_fp16(0), behind the interface the scenarios drive."""

    def __init__(self, dev, D, metric, pair=None):
        self.dev = dev
        self.ix, self.held = pair if pair else (HipFlatIndex(D, metric, 0), HipFlatIndex(D, metric, 0))
        self.ix.set_fp16(True); self.ix.set_fp16_centre(True)
        self.held.set_fp16(0)
        self.expect_centred = True

    def _t(self, x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dev)

    def reserve(self, n):
        self.ix.reserve(n); self.held.reserve(n)

    def add(self, rows):
        t = self._t(rows)
        self.ix.add(t); self.held.add(t)

    def reset(self):
        self.ix.reset(); self.held.reset()

    def set_escalation(self, on):
        self.ix.set_fp16_escalation(on)

    def search(self, q, k):
        t = self._t(q)
        got, want = self.ix.search(t, k), self.held.search(t, k)
        path = self.ix.last_search_path()
        assert path["path"] == "fp16_chain" and path["centred"] is self.expect_centred, path
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), \
            "the centred screened search differs from the fp32 kernel's answer"
        return got

    def certified(self):
        return self.ix.last_screen()["certified"]

    def last_centre(self, queries=True):
        return self.ix.last_centre(queries)

    def select_rows(self, ids):
        return _Screened(self.dev, None, None, pair=(self.ix.select_rows(ids), self.held.select_rows(ids)))

    def close(self):
        self.ix.close(); self.held.close()


def _make(dev):
    return lambda D, metric: _Screened(dev, D, metric)


def _no_complaints(bad, what):
    assert not bad, f"{what}: " + " | ".join(f"[{k}] {v}" for k, v in bad.items())


@pytest.mark.parametrize("c", R.FRESH_CASES, ids=lambda c: f"{c.N}x{c.D}-m{c.metric}-{c.kind}")
def test_fresh_conversion(cuda_device, c):
    _no_complaints(R.run_fresh(_make(cuda_device), c), c)


@pytest.mark.parametrize("metric", [0, 1])
def test_invalid_rows(cuda_device, metric):
    _no_complaints(R.run_invalid_rows(_make(cuda_device), metric), f"invalid rows, metric={metric}")


@pytest.mark.parametrize("metric", [0, 1])
def test_append_capacity_change_and_reset(cuda_device, metric):
    _no_complaints(R.run_append_capacity_reset(_make(cuda_device), metric), f"append / capacity / reset, metric={metric}")


@pytest.mark.parametrize("metric", [0, 1])
def test_two_searches_of_one_index(cuda_device, metric):
    _no_complaints(R.run_two_searches(_make(cuda_device), metric), f"two searches, metric={metric}")


@pytest.mark.parametrize("metric", [0, 1])
def test_query_shapes(cuda_device, metric):
    _no_complaints(R.run_query_shapes(_make(cuda_device), metric), f"query shapes, metric={metric}")


@pytest.mark.parametrize("metric", [0, 1])
def test_second_pass_keeps_t_and_init16_and_gathers_its_queries(cuda_device, metric):
    s, W = R.SECOND_PASS, R.second_pass_world()
    m = cm.centred_model(W["queries"], W["bank"], s["k"], P.kc_of(s["k"]), metric)      # the condition on the world, by the reference alone
    share = 1.0 - float(m["certified"][1.05].mean())
    assert 0.10 <= share <= 0.90 and s["N"] >= 4096 and P.kc_of(s["k"]) < 256, share
    _no_complaints(R.run_second_pass(_make(cuda_device), metric), f"second pass, metric={metric}")


def test_a_view_derives_the_mean_of_its_rows(cuda_device):
    _no_complaints(R.run_view(_make(cuda_device), 0), "view")


def test_zero_mean_bank_and_the_refusals(cuda_device):
    W = R.zero_mean_world()
    ix = _Screened(cuda_device, W["bank"].shape[1], 0)
    ix.expect_centred = False
    with pytest.raises(_lib.HbirdHipError, match="no active centred copy"):      # nothing searched yet
        ix.last_centre()
    ix.add(W["bank"]); ix.search(W["queries"], R.K)                              # (still equals fp32: _Screened.search)
    assert ix.ix.fp16_centre_info()["centred"] is False
    with pytest.raises(_lib.HbirdHipError, match="no active centred copy"):
        ix.last_centre()
    ix.close()
    # the query side goes with the search it belongs to
    F = R.world("float", 1000, 40, 70)
    jx = _Screened(cuda_device, 40, 0)
    jx.add(F["bank"]); jx.search(F["queries"], R.K)
    assert jx.last_centre()["level"] == 0
    jx.add(F["bank"][:5])                                                        # add: the bank side stays readable, the query side does not
    bank_side = jx.last_centre(queries=False)
    assert bank_side["rows"] == 1000 and bank_side["n"] == 0 and bank_side["level"] == -1
    with pytest.raises(_lib.HbirdHipError, match="did not run centred"):
        jx.last_centre()
    jx.ix.set_fp16(0); jx.ix.search(jx._t(F["queries"]), R.K)                    # an fp32 search: not centred
    with pytest.raises(_lib.HbirdHipError, match="did not run centred"):
        jx.last_centre()
    jx.ix.set_fp16(True); jx.search(F["queries"], R.K)
    assert jx.last_centre()["rows"] == 1005
    jx.reset()
    with pytest.raises(_lib.HbirdHipError, match="no active centred copy"):
        jx.last_centre(queries=False)
    jx.close()


@pytest.mark.parametrize("parts", [2, 3])
def test_every_shard_of_a_multi_index_converts_with_its_own_mean(cuda_device, parts):
    """A HipMultiIndex over [0, 0] and [0, 0, 0], planned for 4,000 rows and given 5,003: unequal shards (2,000 + 3,003; 1,334 + 1,334 + 2,335),
    the last one ending inside a row tile.  Each shard derives mu, g, cmax and its tiles from ITS rows and t, c_q, the query tiles from the
    search's queries: last_centre() per shard against the same references as a single index; the merged result is the fp32 search's."""
    from hbird_mi.nn.search_hip import HipMultiIndex
    N, D = 5003, 136
    for metric, kind in ((0, "float"), (1, "exact")):
        W = R.world(kind, N, D, 70)
        bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
        held = HipFlatIndex(D, metric, 0); held.set_fp16(0); held.add(bank)
        want = held.search(q, R.K)
        multi = HipMultiIndex(D, metric, [0] * parts, shard=True)
        multi.reserve(4000); multi.add(bank); multi.set_fp16(1); multi.set_fp16_centre(True)
        for ix in multi.indexes:
            ix.set_fp16_escalation(False)         # (no second pass: every shard's query side stays the caller's)
        got = multi.search(q, R.K)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), f"{parts} shards, metric={metric}"
        sizes = [ix.ntotal for ix in multi.indexes]
        per = (4000 + parts - 1) // parts
        assert sizes == [per] * (parts - 1) + [N - per * (parts - 1)] and sizes[-1] % 32 != 0 and len(set(sizes)) > 1, sizes
        lo, mus = 0, []
        for s, ix in enumerate(multi.indexes):
            C = ix.last_centre()
            rows = W["bank"][lo:lo + sizes[s]]
            assert (C["rows"], C["n"], C["level"]) == (sizes[s], 70, 0), (s, C["rows"], C["n"], C["level"])
            bad = R.check_conversion(C, rows, metric, exact=W["exact"], what=f"shard {s}: ")
            bad.update(R.check_queries(C, W["queries"], exact=W["exact"], what=f"shard {s}: "))
            _no_complaints(bad, f"{parts} shards, metric={metric}, shard {s}")
            mus.append(C["mu"].copy())
            lo += sizes[s]
        assert all(not np.array_equal(mus[0], m) for m in mus[1:]), "every shard derives its own mu"
        multi.close(); held.close()
