"""Excluding searches on the GPU (csrc/hbird_exclude.hip): the filter kernel against the numpy restatement of its definition
(test_exclude_cpu.filter_reference), and HipFlatIndex.search_excluding and its fused forms against the thing they stand for -- `search` /
`search_aggregate` on `select_rows(the allowed rows, ascending)`, ids mapped back.  Every comparison is on bits and integers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import oracle
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex
from test_exclude_cpu import filter_reference

pytestmark = pytest.mark.gpu

METRIC_NAME = {0: "dot_product", 1: "l2"}


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().cpu().view(torch.int32).numpy()


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same(got, want):
    """(idx, dist) pairs: equal ids, equal distance bits."""
    assert np.array_equal(_np(got[0]), _np(want[0]))
    assert np.array_equal(_bits(got[1]), _bits(want[1]))


# ---- 1. the filter alone ----------------------------------------------------------------------------------------------------------------
F_NQ, F_ROWS, F_BASE, F_GROUPS = 70, 5000, 1000, 8


@functools.lru_cache(maxsize=None)
def _filter_lists(k_list):
    """70 hand-made lists of k_list entries over a table of 5,000 rows (id_base 1,000) in 8 groups and -1."""
    rng = np.random.default_rng(1000 + k_list)
    groups = rng.integers(-1, F_GROUPS, size=F_ROWS).astype(np.int32)
    qg = rng.integers(0, F_GROUPS, size=F_NQ).astype(np.int32)
    by_group = {g: np.flatnonzero(groups == g) for g in range(-1, F_GROUPS)}
    idx = np.empty((F_NQ, k_list), dtype=np.int64)
    for i in range(F_NQ):
        idx[i] = F_BASE + rng.choice(F_ROWS, size=k_list, replace=False)
        if i % 2 == 0:               # excluded entries at the chunk edges
            for p in (0, 63, 64, 127, k_list - 1):
                if p < k_list:
                    idx[i, p] = F_BASE + rng.choice(by_group[int(qg[i])])
    idx[1] = F_BASE + rng.choice(by_group[int(qg[1])], size=k_list)               # all excluded (ids repeat)
    idx[3] = -1                                                                    # all missing
    outside = np.concatenate([np.arange(0, F_BASE), np.arange(F_BASE + F_ROWS, F_BASE + F_ROWS + 3000)])
    idx[5] = rng.choice(outside, size=k_list, replace=False)                       # ids outside the table: kept, never looked up
    idx[7, ::2] = rng.choice(outside, size=len(idx[7, ::2]), replace=False)
    qg[9] = -1                                                                     # exclude nothing
    idx[11, k_list // 2:] = -1                                                     # a missing tail (the bank ran out)
    idx[13] = F_BASE + rng.choice(by_group[-1], size=k_list)                       # rows in no group are never excluded ...
    qg[15] = -1; idx[15] = idx[13]                                                 # ... also not by a query that excludes nothing
    idx[17, :-1] = F_BASE + rng.choice(by_group[int(qg[17])], size=k_list - 1)     # only the last entry survives
    dist = rng.standard_normal((F_NQ, k_list)).astype(np.float32)
    dist[19, 0] = -0.0
    return groups, qg, idx, dist


@pytest.mark.parametrize("k_list", [1, 63, 64, 65, 256, 2048])
def test_filter_kernel_equals_the_restatement(cuda_device, k_list):
    groups, qg, idx, dist = _filter_lists(k_list)
    d_groups, d_qg = torch.from_numpy(groups).cuda(), torch.from_numpy(qg).cuda()
    d_idx, d_dist = torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()
    L = _lib.lib()
    for k in sorted({1, 63, 64, 65, k_list}):
        for pad in (-np.inf, np.inf):
            want_i, want_d, want_c = filter_reference(idx, dist, F_BASE, groups, qg, k, np.float32(pad))
            out_i = torch.full((F_NQ, k), -77, dtype=torch.int64, device="cuda")
            out_d = torch.full((F_NQ, k), 77.0, dtype=torch.float32, device="cuda")
            out_c = torch.full((F_NQ,), -77, dtype=torch.int32, device="cuda")
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(L.hb_exclude_filter(d_idx.data_ptr(), d_dist.data_ptr(), F_NQ, k_list, F_BASE, d_groups.data_ptr(), F_ROWS, d_qg.data_ptr(),
                                           k, float(pad), out_i.data_ptr(), out_d.data_ptr(), out_c.data_ptr(), stream))
            torch.cuda.synchronize()
            assert np.array_equal(out_i.cpu().numpy(), want_i), (k_list, k)
            assert np.array_equal(_bits(out_d), _bits(want_d)), (k_list, k)
            assert np.array_equal(out_c.cpu().numpy(), want_c), (k_list, k)


# ---- 2. against views -------------------------------------------------------------------------------------------------------------------
V_D, V_N, V_NQ = 64, 1500, 300
V_SIZES = [1, 2, 7, 40, 230, 300] + [51] * 16 + [52] * 2          # 24 groups, 1,500 rows; group 24 has no rows
V_EMPTY = len(V_SIZES)


@functools.lru_cache(maxsize=None)
def _world():
    """Rows = their group's centre + small noise, dealt to the groups in a random order (a group is not a row range); queries = a row + smaller
    noise, so a query's own group fills the top of its list."""
    assert sum(V_SIZES) == V_N
    rng = np.random.default_rng(42)
    groups = np.repeat(np.arange(len(V_SIZES)), V_SIZES).astype(np.int32)
    rng.shuffle(groups)
    centres = rng.standard_normal((len(V_SIZES), V_D)).astype(np.float32)
    rows = (centres[groups] + 0.05 * rng.standard_normal((V_N, V_D))).astype(np.float32)
    src = np.concatenate([[int(np.flatnonzero(groups == g)[0]) for g in range(len(V_SIZES))],        # one query of every group ...
                          np.flatnonzero(groups == 5)[:40], np.flatnonzero(groups == 4)[:40],         # ... more of the two big ones
                          rng.integers(0, V_N, size=V_NQ - len(V_SIZES) - 80)])
    q = (rows[src] + 0.01 * rng.standard_normal((V_NQ, V_D))).astype(np.float32)
    qg = groups[src].copy()
    qg[10::17] = -1                       # exclude nothing
    qg[11::17] = V_EMPTY                  # a group without rows
    qg[12::17] = (qg[12::17] + 1) % len(V_SIZES)      # another group than the query's own
    return rows, groups, q, qg


@functools.lru_cache(maxsize=None)
def _index(metric, label_P=None, regroup=None):
    """The bank of _world() with its table (regroup = n: groups of n consecutive rows instead); label_P None: no labels, 0: fp32, else counts."""
    rows, groups, _, _ = _world()
    ix = HipFlatIndex(V_D, metric, 0)
    if label_P:
        ix.set_label_denominator(label_P)
    ix.add(torch.from_numpy(rows).cuda())
    if label_P is not None:
        ix.add_labels(torch.from_numpy(gi.labels_from_masks(V_N, 21, 64, seed=5)).cuda()); ix.set_num_classes(21)
    if regroup:
        ix.set_row_groups(torch.arange(V_N) // regroup)
    else:
        ix.set_row_groups(groups, V_EMPTY + 1)
    return ix


def _by_views(ix, groups, q, qg, call):
    """`call(view, queries)` -> tensors whose dim 0 is the query (a tuple of them), for every distinct query group on the view of its allowed
    rows (ascending); -> the per-query results in the queries' order, and per distinct group its allowed ids."""
    parts, allowed_of, order = [], {}, []
    for g in np.unique(qg):
        sel = np.flatnonzero(qg == g)
        allowed = np.flatnonzero(groups != g) if g >= 0 else np.arange(len(groups))
        view = ix.select_rows(torch.from_numpy(allowed))
        parts.append(call(view, torch.from_numpy(q[sel]).cuda(), torch.from_numpy(allowed).cuda()))
        view.close()
        order.append(sel); allowed_of[int(g)] = allowed
    order = np.concatenate(order)
    inv = torch.from_numpy(np.argsort(order)).cuda()
    return tuple(torch.cat([p[j] for p in parts])[inv] for j in range(len(parts[0]))), allowed_of


def _view_search(k, scores=False):
    def call(view, qq, allowed):
        vi, vd = (view.search_scores if scores else view.search)(qq, k)
        return torch.where(vi >= 0, allowed[vi.clamp(min=0)], vi), vd
    return call


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k", [1, 30, 33, 200])
def test_search_excluding_has_the_bits_of_search_on_the_view_of_the_allowed_rows(cuda_device, metric, k):
    rows, groups, q, qg = _world()
    ix = _index(metric)
    got = ix.search_excluding(torch.from_numpy(q).cuda(), k, torch.from_numpy(qg).cuda())
    info = ix.last_exclusion()
    want, allowed_of = _by_views(ix, groups, q, qg, _view_search(k))
    _same(got, want)
    # nothing excluded comes back, and every list is full (1,200 allowed rows at least)
    gi_, gg = got[0].cpu().numpy(), groups
    assert (gi_ >= 0).all() and all((gg[gi_[i]] != qg[i]).all() for i in range(V_NQ))
    assert info["gmax"] == 300
    if k == 30:          # rungs [256, 330]: the queries of the groups of 230 and 300 rows do not get 30 allowed rows out of 256
        assert info["rungs"] == 2 and 0 < info["rung1_queries"] < V_NQ and info["kf"] == 330
    if k == 200:         # r0 = 512 >= 500: one rung, no flag read
        assert info == {"rungs": 1, "rung1_queries": 0, "kf": 500, "gmax": 300}
    # the host path returns the same lists
    hi, hd = ix.search_excluding(q, k, qg)
    assert isinstance(hi, np.ndarray) and np.array_equal(hi, gi_) and np.array_equal(_bits(hd), _bits(got[1]))
    if k == 30:          # ... and so does the fp32 chain of the oracle on the allowed rows
        for g, allowed in allowed_of.items():
            sel = np.flatnonzero(qg == g)
            oi, od = oracle.knn_chain_f32(q[sel], rows[allowed], k, METRIC_NAME[metric])
            assert np.array_equal(allowed[oi], gi_[sel]) and np.array_equal(_bits(od), _bits(got[1][torch.from_numpy(sel).cuda()]))


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_world():
    """D = 16, components in {-1, 0, 1}, 1,200 rows.  Group 0 (300 rows) = 20 copies each of a base vector b and of 14 variants with one
    component zeroed: against b they score 16 (20 rows) and 15 (280 rows, one tie run across the rung-0 cut at 256).  The other 900 rows --
    30 groups of 30 -- are 5 more copies of b and of one variant (duplicates across groups) and 20 copies each of 44 random vectors plus 10
    of a 45th, dealt round-robin, so that copies of one vector sit in different groups and integer scores tie everywhere, the k cut included."""
    rng = np.random.default_rng(7)
    b = rng.choice([-1.0, 1.0], size=16).astype(np.float32)
    variants = []
    for j in range(14):
        v = b.copy(); v[j] = 0.0
        variants.append(v)
    rnd = rng.integers(-1, 2, size=(45, 16)).astype(np.float32)
    rows_a = np.concatenate([np.repeat(b[None], 20, 0)] + [np.repeat(v[None], 20, 0) for v in variants])
    rows_o = np.concatenate([np.repeat(b[None], 5, 0), np.repeat(variants[0][None], 5, 0), np.repeat(rnd[:44], 20, 0), np.repeat(rnd[44:], 10, 0)])
    assert rows_a.shape[0] == 300 and rows_o.shape[0] == 900
    rows = np.concatenate([rows_a, rows_o])
    groups = np.concatenate([np.zeros(300, dtype=np.int32), 1 + (np.arange(900) % 30).astype(np.int32)])
    perm = rng.permutation(1200)
    rows, groups = rows[perm], groups[perm]
    q = np.concatenate([np.repeat(b[None], 4, 0), np.stack(variants[:6]), rnd[:20], rnd[:20]])
    qg = np.concatenate([[0, 0, -1, 3], [0] * 6, np.zeros(20), 1 + np.arange(20) % 30]).astype(np.int32)
    return rows, groups, q, qg


@pytest.mark.parametrize("metric", [0, 1])
def test_ties_across_the_k_cut_and_the_rung_cut(cuda_device, metric):
    rows, groups, q, qg = _tie_world()
    ix = HipFlatIndex(16, metric, 0)
    ix.add(torch.from_numpy(rows).cuda())
    ix.set_row_groups(groups)
    # the total order in exact integer arithmetic (scores are small integers or halves): score descending, id ascending
    score = q.astype(np.float64) @ rows.T.astype(np.float64) - (0.5 * (rows.astype(np.float64) ** 2).sum(1) if metric == 1 else 0.0)
    top256 = np.lexsort((np.broadcast_to(np.arange(1200), score.shape), -score), axis=1)[:, :256]
    for k in (30, 5):
        got = ix.search_excluding(torch.from_numpy(q).cuda(), k, torch.from_numpy(qg).cuda())
        info = ix.last_exclusion()
        want, _ = _by_views(ix, groups, q, qg, _view_search(k))
        _same(got, want)
        # the queries whose 256 best rows hold fewer than k allowed ones go on to rung 1: b and its variants excluding group 0 at least
        short = [(groups[top256[i]] != qg[i]).sum() < k for i in range(len(q))]
        assert info["rung1_queries"] == sum(short) and info["gmax"] == 300
        assert (info["rungs"], info["kf"]) == ((2, k + 300) if sum(short) else (1, 256))
        assert sum(short) >= 8 or k == 5          # (k = 5: the flag is read and nobody goes on)
        d = got[1].cpu().numpy()
        assert (d[:, :-1] == d[:, 1:]).any(axis=1).sum() > len(q) // 2          # the lists are full of ties
    # the plain search's list of b ties across position 256 (the rung-0 cut): score 15 on both sides
    _, pd = ix.search(torch.from_numpy(q[:1]).cuda(), 300)
    assert pd[0, 255] == pd[0, 256]
    ix.close()


# ---- 4. missing tail --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_fewer_allowed_rows_than_k_leave_a_missing_tail(cuda_device, metric):
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((40, 24)).astype(np.float32)
    groups = np.array([0] * 25 + [1] * 15, dtype=np.int32)
    q = rng.standard_normal((5, 24)).astype(np.float32)
    qg = np.array([0, 1, -1, 0, 1], dtype=np.int32)
    ix = HipFlatIndex(24, metric, 0)
    ix.add(torch.from_numpy(rows).cuda()); ix.set_row_groups(groups)
    idx, dist = ix.search_excluding(torch.from_numpy(q).cuda(), 30, torch.from_numpy(qg).cuda(), id_base=500)
    assert ix.last_exclusion() == {"rungs": 1, "rung1_queries": 0, "kf": 55, "gmax": 25}
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    missing = np.inf if metric == 1 else -np.inf
    for i, n_allowed in enumerate([15, 25, 40, 15, 25]):
        n = min(30, n_allowed)
        assert (idx[i, :n] >= 500).all() and (idx[i, n:] == -1).all() and (dist[i, n:] == missing).all() and np.isfinite(dist[i, :n]).all()
        if qg[i] >= 0:
            assert (groups[idx[i, :n] - 500] != qg[i]).all()
    want, _ = _by_views(ix, groups, q, qg, _view_search(30))
    _same((torch.from_numpy(np.where(idx >= 0, idx - 500, idx)), dist), want)
    # ordering scores: the missing value is -inf for both metrics
    _lib.check(_lib.lib().hb_index_set_score_output(ix._h, 1))
    try:
        sidx, sdist = ix.search_excluding(torch.from_numpy(q).cuda(), 30, torch.from_numpy(qg).cuda())
    finally:
        _lib.check(_lib.lib().hb_index_set_score_output(ix._h, 0))
    want, _ = _by_views(ix, groups, q, qg, _view_search(30, scores=True))
    _same((sidx, sdist), want)
    assert (sdist.cpu().numpy()[0, 15:] == -np.inf).all()
    ix.close()


# ---- 5. k beyond 256 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,regroup,rungs", [(300, 100, [400]), (255, None, [512, 555])])
def test_k_beyond_one_pool_pass(cuda_device, k, regroup, rungs):
    rows, groups, q, qg = _world()
    if regroup:
        groups = (np.arange(V_N) // regroup).astype(np.int32)
        qg = np.where(qg >= 0, qg % (V_N // regroup), qg).astype(np.int32)
    ix = _index(0, None, regroup)
    got = ix.search_excluding(torch.from_numpy(q).cuda(), k, torch.from_numpy(qg).cuda())
    info = ix.last_exclusion()
    want, _ = _by_views(ix, groups, q, qg, _view_search(k))
    _same(got, want)
    assert info["gmax"] == (regroup or 300) and info["rungs"] == len(rungs) and info["kf"] == rungs[-1]
    assert (info["rung1_queries"] > 0) == (len(rungs) > 1)


# ---- 6. paths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_paths_no_exclusion_fp16_screen_and_score_output(cuda_device, metric):
    rows, groups, q, qg = _world()
    ix = _index(metric)
    qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
    for k in (8, 30):        # nothing excluded: the search's own bits (its first k of k + gmax)
        _same(ix.search_excluding(qd, k, torch.full((V_NQ,), -1, dtype=torch.int32, device="cuda")), ix.search(qd, k))
    try:                     # the certified fp16 screen gives the fp32 search's result, so the excluding search does not see it
        ix.set_fp16(0)
        want = ix.search_excluding(qd, 8, qgd)
        ix.set_fp16(1)
        got = ix.search_excluding(qd, 8, qgd)
        path = ix.last_search_path()
    finally:
        ix.set_fp16("auto")
    _same(got, want)
    assert path["path"] == "fp32"          # k + gmax = 308 > 128 leaves the screen
    # ordering scores
    _lib.check(_lib.lib().hb_index_set_score_output(ix._h, 1))
    try:
        got = ix.search_excluding(qd, 30, qgd)
    finally:
        _lib.check(_lib.lib().hb_index_set_score_output(ix._h, 0))
    want, _ = _by_views(ix, groups, q, qg, _view_search(30, scores=True))
    _same(got, want)
    if metric == 1:          # (L2 scores are not the distances: the mode was really on)
        assert not np.array_equal(_bits(got[1]), _bits(ix.search_excluding(qd, 30, qgd)[1]))


def test_fp16_screen_serves_a_small_need(cuda_device):
    """k = 8 with groups of at most 40 rows: need = 48 <= 128 stays inside the screen's range; set_fp16(1) forces it."""
    rows, _, q, _ = _world()
    groups = (np.arange(V_N) // 40).astype(np.int32)
    qg = (np.arange(V_NQ) % 38).astype(np.int32)
    ix = HipFlatIndex(V_D, 0, 0)
    ix.add(torch.from_numpy(rows).cuda()); ix.set_row_groups(groups)
    qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
    ix.set_fp16(0)
    want = ix.search_excluding(qd, 8, qgd)
    assert ix.last_search_path()["path"] == "fp32"
    ix.set_fp16(1)
    got = ix.search_excluding(qd, 8, qgd)
    assert ix.last_search_path()["path"] != "fp32" and ix.last_exclusion() == {"rungs": 1, "rung1_queries": 0, "kf": 48, "gmax": 40}
    _same(got, want)
    view_want, _ = _by_views(ix, groups, q, qg, _view_search(8))
    _same(got, view_want)
    ix.close()


# ---- 7. fused forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_P", [0, 64])
def test_fused_forms_have_the_bits_of_their_parts_and_of_the_views(cuda_device, label_P):
    rows, groups, q, qg = _world()
    ix = _index(0, label_P)
    qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
    for k, beta in ((30, 0.02), (7, 0.1), (300, 0.02)):
        out, idx, dist = ix.search_aggregate_excluding(qd, k, qgd, beta=beta, want_neighbours=True)
        lists = ix.search_excluding(qd, k, qgd)
        _same((idx, dist), lists)
        parts = (ix.aggregate if k <= 256 else ix.aggregate_bigk)(qd, lists[0], lists[1], beta=beta)
        assert np.array_equal(_bits(out), _bits(parts))
        (want,), _ = _by_views(ix, groups, q, qg, lambda view, qq, allowed: ((view.search_aggregate if k <= 256 else view.search_aggregate_bigk)(qq, k, beta=beta),))
        assert np.array_equal(_bits(out), _bits(want))
        assert np.array_equal(_bits(ix.search_aggregate_excluding(q, k, qg, beta=beta)), _bits(out))          # host in, host out
    ks, betas = [1, 30, 33, 300], [0.02, 0.1]
    grid, gidx, gdist = ix.search_aggregate_grid_excluding(qd, ks, betas, qgd, want_neighbours=True)
    _same((gidx, gdist), ix.search_excluding(qd, 300, qgd))
    assert tuple(grid.shape) == (8, V_NQ, 21)
    for ik, k in enumerate(ks):
        for ib, beta in enumerate(betas):
            assert np.array_equal(_bits(grid[ik * 2 + ib]), _bits(ix.search_aggregate_excluding(qd, k, qgd, beta=beta))), (k, beta)


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------------
def _raw(ix, q, k, qg, on_device=True):
    """The C entry on sentinel-filled outputs -> (status, outputs untouched)."""
    nq = q.shape[0]
    if on_device:
        idx = torch.full((nq, k), -77, dtype=torch.int64, device="cuda"); dist = torch.full((nq, k), 77.0, device="cuda")
        rc = _lib.lib().hb_index_search_excluding(ix._h, q.data_ptr(), nq, k, 0, qg.data_ptr(), idx.data_ptr(), dist.data_ptr(), 1)
        torch.cuda.synchronize()
        return rc, bool((idx == -77).all()) and bool((dist == 77.0).all())
    idx = np.full((nq, k), -77, dtype=np.int64); dist = np.full((nq, k), 77.0, dtype=np.float32)
    rc = _lib.lib().hb_index_search_excluding(ix._h, q.ctypes.data, nq, k, 0, qg.ctypes.data, idx.ctypes.data, dist.ctypes.data, 0)
    return rc, bool((idx == -77).all()) and bool((dist == 77.0).all())


def test_errors_are_raised_before_anything_is_searched_or_written(cuda_device):
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((2100, 16)).astype(np.float32)
    q = rng.standard_normal((6, 16)).astype(np.float32)
    qd = torch.from_numpy(q).cuda()
    qg = torch.zeros(6, dtype=torch.int32, device="cuda")
    ix = HipFlatIndex(16, 0, 0)
    ix.add(torch.from_numpy(rows).cuda())
    # no table
    with pytest.raises(ValueError, match="no row-group table"):
        ix.search_excluding(qd, 30, qg)
    # a group of 2,030 rows with k = 30: need = 2,060 > 2,048
    ix.set_row_groups(np.array([0] * 2030 + [1] * 70, dtype=np.int32))
    ok = ix.search_excluding(qd, 18, qg)              # need = 2,048 is served
    before = ix.last_exclusion()
    assert before["gmax"] == 2030 and before["kf"] == 2048 and (ok[0].cpu().numpy() >= 2030).all()
    with pytest.raises(ValueError, match=r"k = 30.*gmax = 2030.*2048.*memory_size"):
        ix.search_excluding(qd, 30, qg)
    rc, untouched = _raw(ix, qd, 30, qg)
    assert rc != 0 and untouched and "gmax = 2030" in _lib.last_error() and ix.last_exclusion() == before
    rc, untouched = _raw(ix, q, 30, qg.cpu().numpy(), on_device=False)
    assert rc != 0 and untouched
    # a query group outside the range: device and host query groups
    for bad in (2, -2):
        qb = qg.clone(); qb[4] = bad
        with pytest.raises(ValueError, match=r"outside \[-1, 2\)"):
            ix.search_excluding(qd, 5, qb)
        rc, untouched = _raw(ix, qd, 5, qb)
        assert rc != 0 and untouched and ix.last_exclusion() == before
        rc, untouched = _raw(ix, q, 5, qb.cpu().numpy(), on_device=False)
        assert rc != 0 and untouched and "query 4" in _lib.last_error()
    # a row group outside the range: refused, the table in place stays
    for bad in (2, -2):
        g = np.array([0] * 2030 + [1] * 70, dtype=np.int32); g[77] = bad
        with pytest.raises(ValueError, match=r"outside \[-1, 2\)"):
            ix.set_row_groups(g, 2)
    _same(ix.search_excluding(qd, 18, qg), ok)
    with pytest.raises(ValueError, match="integers"):
        ix.set_row_groups(np.zeros(2100, dtype=np.float32))
    # a table shorter than the bank after add
    ix.add(torch.from_numpy(rows[:10]).cuda())
    with pytest.raises(ValueError, match=r"covers 2100 rows, the bank holds 2110"):
        ix.search_excluding(qd, 5, qg)
    rc, untouched = _raw(ix, qd, 5, qg)
    assert rc != 0 and untouched
    _same(ix.search(qd, 5), ix.search(qd, 5))         # the plain search does not care
    # reset clears the table
    ix.reset()
    assert ix.row_groups is None
    ix.add(torch.from_numpy(rows).cuda())
    with pytest.raises(ValueError, match="no row-group table"):
        ix.search_excluding(qd, 5, qg)
    ix.set_row_groups(np.zeros(2100, dtype=np.int32)); ix.set_row_groups(None)
    with pytest.raises(ValueError, match="no row-group table"):
        ix.search_excluding(qd, 5, qg)
    with pytest.raises(ValueError, match="6 query groups|5 query groups"):
        ix.search_excluding(qd, 5, qg[:5])
    ix.close()
    # sharded and replicated banks have no excluding search
    multi = HipMultiIndex(16, 0, [0, 0], shard=True)
    multi.reserve(100)
    multi.add(torch.from_numpy(rows[:100]).cuda())
    for call in (lambda: multi.search_excluding(qd, 5, qg), lambda: multi.search_aggregate_excluding(qd, 5, qg),
                 lambda: multi.search_aggregate_grid_excluding(qd, [5], [0.02], qg), lambda: multi.set_row_groups(np.zeros(100, dtype=np.int32))):
        with pytest.raises(ValueError, match="single-index"):
            call()
    multi.close()


def test_views_carry_their_rows_groups(cuda_device):
    """select_rows / add_from hand the view groups[ids]: an excluding search on a view equals the one on an index built from those rows."""
    rows, groups, q, qg = _world()
    ix = _index(0)
    ids = np.sort(np.random.default_rng(1).choice(V_N, size=900, replace=False))
    view = ix.select_rows(torch.from_numpy(ids))
    assert np.array_equal(view.row_groups.cpu().numpy(), groups[ids])
    qd, qgd = torch.from_numpy(q[:64]).cuda(), torch.from_numpy(qg[:64]).cuda()
    got = view.search_excluding(qd, 30, qgd)
    fresh = HipFlatIndex(V_D, 0, 0)
    fresh.add(torch.from_numpy(rows[ids]).cuda()); fresh.set_row_groups(groups[ids], V_EMPTY + 1)
    _same(got, fresh.search_excluding(qd, 30, qgd))
    # add_from appends the groups of the rows it appends
    more = np.setdiff1d(np.arange(V_N), ids)[:100]
    view.add_from(ix, torch.from_numpy(more))
    assert np.array_equal(view.row_groups.cpu().numpy(), np.concatenate([groups[ids], groups[more]]))
    view.search_excluding(qd, 30, qgd)
    view.close(); fresh.close()
