"""k-means over the resident bank on the GPU (include/hbird_hip_kmeans.h, hbird_mi/kmeans.py) against the numpy model of tests/kmeans_refs.py:
the assignment step against the public k = 1 search and, on worlds whose fp32 arithmetic is exact, against the float64 argmin; the integer
update on bits; the loop on assignments, centroid bits and the integers of its history.  Shapes are the smallest at which a path can go wrong:
one row, rows around a tile (31, 33), several tiles and segments (257, 1000, 4000), a padded width (72 -> 80), K = 1 and K = 2048; and
R.BIG_ROWS = 131,195 rows, the smallest bank that crosses every row-count seam at once (tests/linprobe_refs.py spells out the arithmetic,
tests/test_bank_task_seams_cpu.py holds the lists below to it): all four slots of an accumulating wave, a second trip, empty trailing segments,
33 workgroups of the counting kernels, j = 1 and 2 in the inertia tree, a default staging chunk that splits the bank."""
import ctypes
import math

import numpy as np
import pytest
import torch

import kmeans_refs as R
from hbird_mi import _lib
from hbird_mi import kmeans as KM
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

pytestmark = pytest.mark.gpu


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _bank(x):
    ix = HipFlatIndex(x.shape[1], 0, 0)
    ix.add(torch.from_numpy(np.ascontiguousarray(x)).cuda(), normalize=False)
    return ix


def _cent(c):
    ix = HipFlatIndex(c.shape[1], 1, 0)
    ix.set_fp16(0)
    ix.add(torch.from_numpy(np.ascontiguousarray(c)).cuda(), normalize=False)
    return ix


def _live():
    c, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hb_debug_live_allocations(ctypes.byref(c), ctypes.byref(b)))
    return c.value, b.value


def _randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---- assign ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 72, 384])
def test_assign_equals_the_public_search_on_a_separately_built_index(cuda_device, D):
    cents = {K: _randn((K, D), 100 + K) for K in (1, 2, 33, 257)}
    mine = {K: _cent(c) for K, c in cents.items()}
    theirs = {K: _cent(c) for K, c in cents.items()}
    for rows in (1, 31, 33, 257, 1000):
        x = _randn((rows, D), rows)
        bank = _bank(x)
        stored = bank.reconstruct(torch.arange(rows, device="cuda"))
        assert np.array_equal(_bits(stored), _bits(x))
        for K in cents:
            a, d = KM.assign_rows(bank, mine[K])
            idx, dist = theirs[K].search(stored, 1)
            assert a.dtype == torch.int32 and torch.equal(a.long(), idx.view(-1)) and np.array_equal(_bits(d), _bits(dist.view(-1))), (rows, K)
            if rows == 1000:
                # a range off the tile boundaries, and chunks of 64 rows against the automatic chunk
                a2, d2 = KM.assign_rows(bank, mine[K], row0=5, n=70)
                assert torch.equal(a2, a[5:75]) and np.array_equal(_bits(d2), _bits(d[5:75]))
                a3, d3 = KM.assign_rows(bank, mine[K], chunk_rows=64)
                assert torch.equal(a3, a) and np.array_equal(_bits(d3), _bits(d))
                a4, none = KM.assign_rows(bank, mine[K], row0=937, n=63, chunk_rows=7, want_dist=False)
                assert none is None and torch.equal(a4, a[937:])
        bank.close()
    for ix in list(mine.values()) + list(theirs.values()):
        ix.close()


@pytest.mark.parametrize("D, rows, K", [(16, 257, 33), (72, 1000, 257), (384, 33, 2)])
def test_assign_on_small_integer_worlds_is_the_float64_argmin_with_the_lower_id_on_ties(cuda_device, D, rows, K):
    x, c = R.small_integer_world(D, rows, K, seed=D + K)
    c[K - 1] = c[0]                                           # an exact twin of centroid 0: it never wins
    want, best, second = R.assign(x, c)
    assert (best == second).any() or K == 2                  # the world holds ties (exact ones)
    bank, cent = _bank(x), _cent(c)
    a, d = KM.assign_rows(bank, cent)
    assert np.array_equal(a.cpu().numpy(), want) and not (a == K - 1).any()
    assert np.array_equal(d.cpu().numpy(), best.astype(np.float32))      # (exact in fp32: the L2 search reports squared distances)
    bank.close(); cent.close()


def test_assign_identical_centroids_and_rows_that_are_not_finite(cuda_device):
    x = _randn((70, 16), 3)
    x[11, 4], x[40, 0], x[69, 15] = np.nan, np.inf, -np.inf
    c = np.repeat(_randn((1, 16), 4), 5, axis=0)
    bank, cent = _bank(x), _cent(c)
    a, d = KM.assign_rows(bank, cent)
    want = np.zeros(70, dtype=np.int32); want[[11, 40, 69]] = -1
    assert np.array_equal(a.cpu().numpy(), want)
    assert np.array_equal(a.cpu().numpy(), R.assign(x, c)[0])
    for bad in (dict(row0=-1, n=3), dict(row0=60, n=11), dict(row0=0, n=71)):
        with pytest.raises(ValueError, match="outside the bank"):
            KM.assign_rows(bank, cent, **bad)
    with pytest.raises(ValueError, match="HB_METRIC_L2"):
        KM.assign_rows(bank, _bank(c))
    with pytest.raises(ValueError, match="width"):
        KM.assign_rows(bank, _cent(_randn((3, 8), 1)))
    bank.close(); cent.close()


# ---- accumulate + centroids ----------------------------------------------------------------------------------------------------------------------
def _check_update(x, a, K, seed=0):
    """The engine's sums, counts and centroids of (x, a) against the model, on bits; -> (sums, counts) tensors."""
    bank = _bank(x)
    at = torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()
    sums, counts = KM.accumulate(bank, at, K)
    S, n = R.integer_sums(x, a, K)
    assert np.array_equal(sums.cpu().numpy(), S) and np.array_equal(counts.cpu().numpy(), n)
    prev = _randn((K, x.shape[1]), 1000 + seed)
    cent, empty = KM.centroids_from_sums(sums, counts, torch.from_numpy(prev).cuda())
    want = R.centroids_from_sums(S, n, prev)
    assert np.array_equal(_bits(cent), _bits(want)) and empty == int((n == 0).sum())
    if (n == 0).any():                                        # an empty cluster keeps its previous centroid
        assert np.array_equal(_bits(cent)[n == 0], _bits(prev)[n == 0])
    # again: the same bits (integer sums do not depend on the order the atomics arrive in)
    sums2, counts2 = KM.accumulate(bank, at, K)
    assert torch.equal(sums2, sums) and torch.equal(counts2, counts)
    bank.close()
    return sums, counts


@pytest.mark.parametrize("pattern", ["one_cluster", "round_robin", "random", "some_unassigned"])
def test_accumulate_and_centroids_equal_the_integer_model_on_bits(cuda_device, pattern):
    rows, D, K = 1000, 16, 7
    g = np.random.default_rng(5)
    x = (g.uniform(-1, 1, (rows, D))).astype(np.float32)
    a = {"one_cluster": np.full(rows, 3), "round_robin": np.arange(rows) % K, "random": g.integers(0, K - 1, rows),      # (random: cluster 6 stays empty)
         "some_unassigned": np.where(g.random(rows) < 0.2, -1, g.integers(0, K, rows))}[pattern].astype(np.int32)
    _check_update(x, a, K)


def test_accumulate_rounds_half_to_even_on_the_quantisers_grid(cuda_device):
    vals = np.array([1.0, -1.0, 2.0 ** -31, -(2.0 ** -31), 3 * 2.0 ** -31, -3 * 2.0 ** -31, 2.0, -2.0, 0.0, 5 * 2.0 ** -31], dtype=np.float32)
    g = np.random.default_rng(6)
    x = vals[g.integers(0, len(vals), (257, 16))]
    x[0, :10] = vals
    a = np.zeros(257, dtype=np.int32); a[1:] = g.integers(0, 3, 256)
    a[0] = 4                                                  # a cluster of its own: its sums are the quantised values themselves
    sums, _ = _check_update(x, a, 5)
    assert sums[4, :10].tolist() == [2 ** 30, -(2 ** 30), 0, 0, 2, -2, 2 ** 31, -(2 ** 31), 0, 2]


@pytest.mark.parametrize("K, D, rows", [(2048, 16, 4000), (7, 384, 1000), (33, 72, 257), (1, 16, 1)])
def test_accumulate_shapes_the_largest_table_a_wide_bank_a_padded_width_one_row(cuda_device, K, D, rows):
    g = np.random.default_rng(K + D)
    x = g.uniform(-1, 1, (rows, D)).astype(np.float32)
    a = g.integers(0, K, rows).astype(np.int32)
    a[rows - 1] = K - 1
    _check_update(x, a, K, seed=K)


def test_accumulate_over_split_row_ranges_equals_one_call(cuda_device):
    rows, D, K = 1000, 72, 9
    g = np.random.default_rng(8)
    x = g.uniform(-1, 1, (rows, D)).astype(np.float32)
    a = np.where(g.random(rows) < 0.1, -1, g.integers(0, K, rows)).astype(np.int32)
    bank, at = _bank(x), torch.from_numpy(a).cuda()
    whole = KM.accumulate(bank, at, K)
    sums, counts = KM.accumulate(bank, at[:333], K)
    KM.accumulate(bank, at[333:970], K, row0=333, sums=sums, counts=counts)
    KM.accumulate(bank, at[970:], K, row0=970, sums=sums, counts=counts)
    assert torch.equal(sums, whole[0]) and torch.equal(counts, whole[1])
    S, n = R.integer_sums(x, a, K)
    assert np.array_equal(sums.cpu().numpy(), S) and np.array_equal(counts.cpu().numpy(), n)
    with pytest.raises(ValueError, match="outside the bank"):
        KM.accumulate(bank, at, K, row0=1)
    bank.close()


# ---- past the first bank-size seams (R.BIG_ROWS; the lists are held to the launch arithmetic by tests/test_bank_task_seams_cpu.py) -----------------
BIG_D = 16
BIG_UPDATE_K = (5, 2048)
# (row0, n) of the calls that together cover the bank: cuts off the tile edges, the last range ending inside the last tile
BIG_SPLITS = [(0, 65541), (65541, R.BIG_ROWS - 10 - 65541), (R.BIG_ROWS - 10, 10)]
BIG_ASSIGN_CHUNKS = (0, 64 * 1024)              # the default staging chunk (131,072 rows: two chunks) against chunks of 65,536 (three)
BIG_SAMPLE = (R.BIG_ROWS - 4096, 4096)          # rows of the sample held to the public search: both sides of the default chunk's edge, 131,072


def _big_uniform(seed):
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, (R.BIG_ROWS, BIG_D)).astype(np.float32), g


@pytest.mark.parametrize("K", BIG_UPDATE_K)
def test_accumulate_on_the_big_bank_every_slot_a_second_trip_and_empty_segments(cuda_device, K):
    x, g = _big_uniform(20 + K)
    a = np.where(g.random(R.BIG_ROWS) < 0.1, -1, g.integers(0, K, R.BIG_ROWS)).astype(np.int32)
    a[R.BIG_ROWS - 1] = K - 1
    _check_update(x, a, K, seed=K)


def test_accumulate_over_split_row_ranges_of_the_big_bank_equals_one_call(cuda_device):
    K = 9
    x, g = _big_uniform(30)
    a = np.where(g.random(R.BIG_ROWS) < 0.1, -1, g.integers(0, K, R.BIG_ROWS)).astype(np.int32)
    assert BIG_SPLITS[0][0] == 0 and all(p[0] + p[1] == q[0] for p, q in zip(BIG_SPLITS, BIG_SPLITS[1:])) and sum(BIG_SPLITS[-1]) == R.BIG_ROWS
    bank, at = _bank(x), torch.from_numpy(a).cuda()
    whole = KM.accumulate(bank, at, K)
    sums = counts = None
    for row0, n in BIG_SPLITS:
        sums, counts = KM.accumulate(bank, at[row0:row0 + n], K, row0=row0, sums=sums, counts=counts)
    assert torch.equal(sums, whole[0]) and torch.equal(counts, whole[1])
    S, cnt = R.integer_sums(x, a, K)
    assert np.array_equal(sums.cpu().numpy(), S) and np.array_equal(counts.cpu().numpy(), cnt)
    # a range that ends inside the last tile, on its own, against the model
    row0, n = BIG_SPLITS[1][0], R.BIG_ROWS - 10 - BIG_SPLITS[1][0]
    part = KM.accumulate(bank, at[row0:row0 + n], K, row0=row0)
    masked = np.full(R.BIG_ROWS, -1, dtype=np.int32); masked[row0:row0 + n] = a[row0:row0 + n]
    S, cnt = R.integer_sums(x, masked, K)
    assert np.array_equal(part[0].cpu().numpy(), S) and np.array_equal(part[1].cpu().numpy(), cnt)
    bank.close()


def test_assign_on_the_big_bank_the_default_staging_chunk_splits_it(cuda_device):
    x, init, init_rows, model = R.big_blob_world()
    bank, cent, theirs = _bank(x), _cent(model["centroids"]), _cent(model["centroids"])
    got = {c: KM.assign_rows(bank, cent, chunk_rows=c) for c in BIG_ASSIGN_CHUNKS}
    a, d = got[0]
    assert torch.equal(got[64 * 1024][0], a) and np.array_equal(_bits(got[64 * 1024][1]), _bits(d))
    assert np.array_equal(a.cpu().numpy(), model["assign"]) and a[R.BIG_HOLE].item() == -1      # (the margins hold: the model decides)
    row0, n = BIG_SAMPLE
    idx, dist = theirs.search(torch.from_numpy(x[row0:row0 + n]).cuda(), 1)
    assert torch.equal(a[row0:row0 + n].long(), idx.view(-1)) and np.array_equal(_bits(d[row0:row0 + n]), _bits(dist.view(-1)))
    bank.close(); cent.close(); theirs.close()


def test_fit_on_the_big_blob_world_equals_the_model(cuda_device):
    x, init, init_rows, model = R.big_blob_world()
    res = _check_fit(x, init, model, max_iter=10)
    assert res.converged and res.n_iter == model["n_iter"] and all(h["unassigned"] == 1 for h in res.history)


def test_accumulate_refuses_rows_outside_the_quantisers_range(cuda_device):
    x = np.random.default_rng(9).uniform(-1, 1, (70, 16)).astype(np.float32)
    x[37, 9] = 2.5
    a = np.zeros(70, dtype=np.int32)
    bank = _bank(x)
    with pytest.raises(ValueError, match=r"outside \[-2, 2\]"):
        KM.accumulate(bank, torch.from_numpy(a).cuda(), 2)
    a[37] = -1                                                # unassigned: the row is not read into any sum
    sums, counts = KM.accumulate(bank, torch.from_numpy(a).cuda(), 2)
    S, n = R.integer_sums(x, a, 2)
    assert np.array_equal(sums.cpu().numpy(), S) and counts.tolist() == [69, 0]
    a[3] = 2
    with pytest.raises(ValueError, match="not below K"):
        KM.accumulate(bank, torch.from_numpy(a).cuda(), 2)
    for K in (0, 2049):
        with pytest.raises(ValueError, match="2048"):
            KM.accumulate(bank, torch.from_numpy(a).cuda(), K)
    bank.close()


# ---- fit ---------------------------------------------------------------------------------------------------------------------------------------
def _check_fit(x, init, model, max_iter, **kw):
    bank = _bank(x)
    before = _live()
    res = KM.kmeans_fit(bank, init.shape[0], init=torch.from_numpy(init), max_iter=max_iter, return_assignments=True, **kw)
    assert _live() == before                                  # the centroid index and every buffer of the call are gone
    K = init.shape[0]
    a = res.assignments.cpu().numpy()
    assert np.array_equal(a, model["assign"])
    assert np.array_equal(_bits(res.centroids), _bits(model["centroids"])) and np.array_equal(res.counts.cpu().numpy(), model["counts"])
    assert res.n_iter == model["n_iter"] and res.converged == model["converged"]
    for got, want in zip(res.history, model["history"]):
        assert (got["changed"], got["empty"], got["unassigned"]) == (want["changed"], want["empty"], want["unassigned"])
        assert abs(got["inertia"] - want["inertia"]) <= 1e-4 * want["inertia"]      # (the model's distances are float64: reported only)
    if res.converged:
        assert res.history[-1]["changed"] == 0
    # independently of the model: the returned centroids are the integer update of the returned assignment
    cent, n, empty = R.update(x, a, K, res.centroids.cpu().numpy())
    assert np.array_equal(_bits(res.centroids), _bits(cent)) and np.array_equal(res.counts.cpu().numpy(), n)
    # the last inertia is the float64 sum of the distances the final assignment's search returns (first-order bound of a float64 sum, doubled)
    if res.converged:
        ids, d = res.assign(bank.reconstruct(torch.arange(x.shape[0], device="cuda")), return_distances=True)
        assert np.array_equal(ids.cpu().numpy(), a)
        exact = math.fsum(d.cpu().numpy().astype(np.float64)[a >= 0])
        assert abs(res.history[-1]["inertia"] - exact) <= x.shape[0] * 2.0 ** -52 * exact
        res.close()
    bank.close()
    return res


@pytest.mark.parametrize("world", R.BLOB_WORLDS, ids=str)
def test_fit_on_planted_blobs_equals_the_model(cuda_device, world):
    x, init, init_rows, model = R.blob_world(*world)
    res = _check_fit(x, init, model, max_iter=10)
    assert res.converged and res.n_iter == 2


@pytest.mark.parametrize("world", R.DRIFT_WORLDS, ids=str)
def test_fit_through_several_iterations_equals_the_model(cuda_device, world):
    K, D, rows, seed, iters = world
    x, init, model = R.drift_world(K, D, rows, seed)
    res = _check_fit(x, init, model, max_iter=20)
    assert res.n_iter == iters
    same = _check_fit(x, init, model, max_iter=20, chunk_rows=64)          # the staging chunks do not show
    assert np.array_equal(_bits(same.centroids), _bits(res.centroids))
    short = R.fit(x, init, 3)                                  # stopped early: unconverged, the invariant still holds
    assert not short["converged"]
    _check_fit(x, init, short, max_iter=3)


def test_fit_one_iteration_duplicated_init_rows_and_rows_that_are_not_finite(cuda_device):
    x, init, init_rows, model = R.blob_world(*R.BLOB_WORLDS[0])
    one = R.fit(x, init, 1)
    assert not one["converged"] and one["n_iter"] == 1
    _check_fit(x, init, one, max_iter=1)
    # a duplicated init row: the lower id takes all, the twin is empty in the history and keeps its centroid
    dup = np.concatenate([init, init[1:2]])
    res = _check_fit(x, dup, R.fit(x, dup, 1), max_iter=1)
    assert res.history[0]["empty"] == 1 and res.counts[3].item() == 0 and np.array_equal(_bits(res.centroids[3]), _bits(dup[3]))
    # rows that are not finite stay unassigned in every iteration and enter no sum
    bad = x.copy()
    holes = [r for r in (5, 77, 300) if r not in set(init_rows.tolist())]
    bad[holes, 2] = np.nan
    res = _check_fit(bad, init, R.fit(bad, init, 10), max_iter=10)
    assert res.converged and all(h["unassigned"] == len(holes) for h in res.history) and torch.isfinite(res.centroids).all()


def test_fit_default_init_row_ids_and_refusals(cuda_device):
    x, init, init_rows, model = R.blob_world(*R.BLOB_WORLDS[0])
    bank = _bank(x)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(7))[:3]
    assert np.array_equal(_bits(KM.initial_centroids(bank, 3, None, 7)), _bits(x[perm.numpy()]))
    by_seed = KM.kmeans_fit(bank, 3, seed=7, max_iter=10)
    by_rows = KM.kmeans_fit(bank, 3, init=perm, max_iter=10)
    by_tensor = KM.kmeans_fit(bank, 3, init=torch.from_numpy(x[perm.numpy()]), max_iter=10)
    assert by_seed.assignments is None and by_seed.history == by_rows.history == by_tensor.history
    assert torch.equal(by_seed.centroids, by_rows.centroids) and torch.equal(by_seed.centroids, by_tensor.centroids)
    by_blob = KM.kmeans_fit(bank, 3, init=init_rows, max_iter=10)
    assert np.array_equal(_bits(by_blob.centroids), _bits(model["centroids"]))
    for K in (0, 2049, x.shape[0] + 1):
        with pytest.raises(ValueError, match="n_clusters"):
            KM.kmeans_fit(bank, K)
    for bad in (dict(max_iter=0), dict(init=torch.zeros(3, 15)), dict(init=[0, 1]), dict(init=[0, 1, x.shape[0]]), dict(init=[0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            KM.kmeans_fit(bank, 3, **bad)
    # the C entry refuses the same before anything is launched
    L, z = _lib.lib(), ctypes.c_int(0)
    hist = (ctypes.c_double * 4)()
    c = torch.zeros(3, 16, device="cuda"); n = torch.zeros(3, dtype=torch.int64, device="cuda")
    for K, msg in ((0, "[1, 2048]"), (2049, "[1, 2048]"), (601, "exceeds the bank's 600 rows")):
        assert L.hb_kmeans_fit(bank._h, K, ctypes.c_void_p(c.data_ptr()), 1, 0, ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(n.data_ptr()), None,
                               hist, ctypes.byref(z), ctypes.byref(z)) != 0 and msg in _lib.last_error()
    multi = HipMultiIndex(16, 0, [0, 0], shard=True)
    with pytest.raises(ValueError, match="HipMultiIndex"):
        KM.kmeans_fit(multi, 3)
    multi.close(); bank.close()
