"""Seeded random lives of an index (tests/index_life.py) against HipFlatIndex on the GPU: about 40 mutators, readers and refusals per life on
ONE index, every reader held to the numpy model -- neighbour ids and distance words to oracle.knn_chain_f32, label_hat to the same call on a
fresh index (bit for bit) and to the float64 K5 restatement within its bound, rows and label rows to the model's bits.  What a life is for
(the workspaces re-carved at another size, the cached work list, the lazy copies, the sticky records) is asserted from the generator alone
in tests/test_index_life_cpu.py.

After every life the live device allocations of the library (hb_debug_live_allocations) are what they were before its first index, count
and bytes.  The last test holds the lives together to every path name a search with k <= 128 can report."""
import ctypes
import gc
import time

import numpy as np
import pytest
import torch

import index_life as L
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

pytestmark = pytest.mark.gpu

RESULTS = {}          # name of a life (or pair) -> {path name: readers served}


def _live():
    count, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.lib().hb_debug_live_allocations(ctypes.byref(count), ctypes.byref(nbytes)))
    return int(count.value), int(nbytes.value)


class GpuEnv(L.Env):
    """Device tensors on cuda:0.  Every copy in and every call is followed by a synchronisation: an index that follows a side stream
    (use_current_stream) and a fresh one on its own stream read the same tensors."""

    def __init__(self):
        self.paths, self.side, self.on_side = [], None, False

    def dev(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.current_stream().synchronize()
        return t

    def sync(self):
        torch.cuda.synchronize()

    def stream(self, side):
        if side and self.side is None:
            self.side = torch.cuda.Stream()
        self.on_side = bool(side)
        torch.cuda.set_stream(self.side if side else torch.cuda.default_stream())

    def step(self, i):          # (an interleaved life finds the current stream where the other life left it)
        torch.cuda.set_stream(self.side if self.on_side else torch.cuda.default_stream())


def _held(name, run):
    """run() between two readings of the live allocations; its histogram(s) and wall time are kept and printed"""
    gc.collect()
    torch.cuda.set_device(0)
    before = _live()
    t0 = time.perf_counter()
    try:
        hists = run()
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())
    secs = time.perf_counter() - t0
    gc.collect()
    assert _live() == before, f"{name}: live device allocations (count, bytes) {_live()} after every index was closed, {before} before the first"
    total = {}
    for h in hists if isinstance(hists, list) else [hists]:
        for p, n in h.items():
            total[p] = total.get(p, 0) + n
    RESULTS[name] = total
    print(f"index life {name}: {secs:.2f} s, paths {total}")
    return total


def _single(seed, steered):
    return _held(str(seed), lambda: L.run_life(HipFlatIndex, L.generate(seed, steered=steered), GpuEnv()))


def _pair(seeds):
    lives = [L.generate(s, big=False, length=L.PAIR_LENGTH) for s in seeds]
    return _held("%d+%d" % seeds, lambda: L.run_interleaved(HipFlatIndex, lives, [GpuEnv() for _ in lives]))


@pytest.mark.parametrize("seed", L.PLAIN_SEEDS)
def test_plain_life(cuda_device, seed):
    _single(seed, False)


@pytest.mark.parametrize("seed", L.STEERED_SEEDS)
def test_steered_life(cuda_device, seed):
    _single(seed, True)


@pytest.mark.parametrize("seeds", L.PAIR_SEEDS, ids=lambda s: "%d+%d" % s)
def test_two_lives_interleaved(cuda_device, seeds):
    """Two lives of different D alternate operation by operation on cuda:0: per-device and process-wide state, and the thread-local error
    text after a refusal on the other index."""
    _pair(seeds)


def _op(op, kind=None, **kw):
    return dict(op=op, kind=kind or op, **kw)


def _search(nq, k, host=False, **kw):
    return _op("search", nq=nq, k=k, host=host, id_base=0, aim=False, **kw)


def test_a_view_of_an_index_whose_group_table_is_behind_its_rows(cuda_device):
    """Regression (a stale record found while the lives were written): set_row_groups, an append, then select_rows -- the view took
    groups[ids] from the Python-side copy of a table that no longer covered the rows, an index beyond its end.  The view now comes
    without a table, as the library's own (hb_index_select_rows) does."""
    head = dict(seed=401, D=48, metric=0, C=5, P=0, fp16=False, steered=False, big=False)
    ops = [_op("reserve", n=300, above=True),
           _op("add", n=300, host=False, normalize=False, spread=False, plant=False),
           _op("set_row_groups", big=False),
           _op("add", n=33, host=True, normalize=True, spread=False, plant=False),
           _op("select_rows", m=333, host=False),
           _search(37, 10), _op("ntotal"),
           _op("add_from", n_src=300, m=200, host=False),
           _search(257, 33, host=True), _op("reconstruct", m=37, host=False, foreign=True)]
    _held("view-behind-groups", lambda: L.run_life(HipFlatIndex, (head, ops), GpuEnv()))


def test_k_zero_is_refused_by_its_name_on_the_device_path(cuda_device):
    """Regression (life 101, step 22 -- refuse[k_zero] with device I/O): an [nq, 0] output tensor has no address, and hb_index_search
    looked at the pointers first: "output pointers are NULL" for a caller whose mistake was the k.  Both sides now name the range, and the
    next search is right."""
    head = dict(seed=402, D=20, metric=1, C=5, P=L.P_COUNTS, fp16=False, steered=False, big=False)
    ops = [_op("reserve", n=100, above=True),
           _op("add", n=257, host=True, normalize=False, spread=True, plant=False),
           _op("refuse", "k_zero", nq=37, k=0, host=False), _search(37, 10),
           _op("refuse", "k_zero", nq=37, k=0, host=True), _search(37, 33, host=True),
           _op("refuse", "k_2049", nq=37, k=2049, host=False), _search(1, 300)]
    _held("k-zero", lambda: L.run_life(HipFlatIndex, (head, ops), GpuEnv()))


MULTI_ENTRIES = ("search_excluding", "search_aggregate_excluding")


def test_a_life_through_two_shards_on_one_device(cuda_device):
    """HipMultiIndex([0, 0], shard=True) through the operations it supports -- reserve, add, add_labels, search, search_scores,
    search_aggregate, search_aggregate_grid, reconstruct, gather_labels, reset -- with the exclusion calls as refusals.  Left out, because a
    sharded bank has none: aggregate / aggregate_grid on given lists are reached through the fused forms only, search_aggregate_bigk (a
    multi index routes k > 256 itself), every excluding form, copy_norms against a fresh index, views, row groups and the mode settings
    other than set_fp16."""
    head = dict(seed=501, D=64, metric=1, C=21, P=L.P_COUNTS, fp16=False, steered=False, big=False)
    agg = dict(beta=0.02, id_base=0, aim=False)
    ops = [_op("reserve", n=2300, above=True),
           _op("add", n=1000, host=False, normalize=True, spread=False, plant=False),
           _op("add", n=1000, host=True, normalize=False, spread=True, plant=False),
           _op("add", n=257, host=False, normalize=False, spread=False, plant=False),       # (2,257 rows: 1,150 + 1,107)
           _search(300, 33), _search(37, 10, host=True), _search(257, 300),
           _op("search_scores", nq=257, k=90, host=False, id_base=0, aim=False),
           _op("search_aggregate", nq=300, k=30, host=False, **agg), _op("search_aggregate", nq=37, k=130, host=True, **agg),
           _op("search_aggregate_grid", nq=37, ks=(1, 10, 30), betas=(0.02, 0.07), host=False, id_base=0, aim=False),
           _op("reconstruct", m=300, host=False, foreign=True), _op("gather_labels", m=37, host=True, foreign=True)]
    for entry in MULTI_ENTRIES:
        ops += [_op("refuse", "multi_excluding", nq=37, entry=entry), _search(37, 32)]
    ops += [_op("set_fp16", mode=1), _search(300, 10),
            _op("add", n=500, host=False, normalize=False, spread=False, plant=False),       # beyond the plan: the last shard takes it
            _search(700, 33), _op("search_aggregate", nq=257, k=90, host=False, **agg),
            _op("reset", n=300, C=5, P=0, other=True, smaller=True, plant=False, host=True, normalize=False),
            _search(37, 10, host=True), _op("search_aggregate", nq=300, k=32, host=False, **agg),
            _op("gather_labels", m=37, host=False, foreign=True), _op("ntotal")]
    _held("multi", lambda: L.run_life(lambda d, metric, device: HipMultiIndex(d, metric, [0, 0], shard=True), (head, ops), GpuEnv()))


def test_every_search_path_served_a_reader(cuda_device):
    """Every path name a search with k <= 128 can report (HipFlatIndex.SEARCH_PATHS) served at least one reader of the committed lives."""
    for seed in L.PLAIN_SEEDS:
        if str(seed) not in RESULTS:
            _single(seed, False)
    for seed in L.STEERED_SEEDS:
        if str(seed) not in RESULTS:
            _single(seed, True)
    for seeds in L.PAIR_SEEDS:
        if "%d+%d" % seeds not in RESULTS:
            _pair(seeds)
    total = {}
    for name, h in RESULTS.items():
        if name[0].isdigit():         # (the committed lives, not the hand-written cases)
            for p, n in h.items():
                total[p] = total.get(p, 0) + n
    print(f"index lives: readers with k <= 128 by path: {total}")
    assert set(total) == set(HipFlatIndex.SEARCH_PATHS), total
