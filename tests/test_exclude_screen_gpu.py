"""Excluding searches on the certified fp16 screen, on the GPU (csrc/hbird_exclude_screen.hip):
  1. the excluding re-rank kernel alone (hb_index_exclude_rerank) on the candidate pass' own lists against the numpy restatement of
     tests/excl_screen_refs.py: ids and distance bits of the fp32 chain ranking restricted to the allowed candidates, the certificate by
     f16_pass_refs.flag_band, the k-th score and the floor;
  2. the route (set_exclusion_screen) on the image world against the same call with the route off, and against views;
  3. the searches the route does not serve, and the entry's refusals;
  4. HbirdEvaluation.evaluate_leave_one_out(screen=True) against screen=False.
Every comparison of lists is on ids and distance bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import excl_screen_refs as X
import f16_pass_refs as R
import oracle
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex
from test_exclude_gpu import _bits, _by_views, _same, _view_search, _world as _shuffled_world

pytestmark = pytest.mark.gpu

EMPTY_GROUP = {"image": 36, "small": 7, "tiny": 5}        # a group id without rows, inside every table


def _table(name, edited):
    """The world's group table; edited: every 7th row in no group (-1)."""
    groups = X.world(name)[1].copy()
    if edited:
        groups[::7] = -1
    return groups


def _make_index(name, metric, edited=False):
    rows, _, _, _ = X.world(name)
    ix = HipFlatIndex(rows.shape[1], metric, 0)
    ix.add(torch.from_numpy(rows).cuda())
    ix.set_row_groups(_table(name, edited), EMPTY_GROUP[name] + 1)
    ix.set_fp16(1)
    return ix


@functools.lru_cache(maxsize=None)
def _index(name, metric, edited=False):
    return _make_index(name, metric, edited)


@functools.lru_cache(maxsize=None)
def _pass_lists(name, metric, k_search):
    """The level-0 candidate lists and pass scores of search(q, k_search) under set_fp16(1) (kc = kc_of(k_search)), read with last_screen()."""
    ix = _index(name, metric)
    q = X.world(name)[2]
    ix.set_fp16_escalation(False)          # (a second pass would reuse the lists)
    try:
        ix.search(torch.from_numpy(q).cuda(), k_search)
        sc = ix.last_screen()
    finally:
        ix.set_fp16_escalation(True)
    assert sc["kc"] == R.kc_of(k_search) and sc["nq"] == len(q) and not sc["centred"]
    return sc["rows"], sc["scores"]


def _entry(ix, q, cand, sc, qg, k, id_base=0):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ix.exclude_rerank(dev(q), dev(cand), dev(sc), dev(np.asarray(qg, dtype=np.int32)), k, id_base)
    return tuple(t.cpu().numpy() for t in out)


def _check_kernel(name, metric, cand, sc, qg, k, edited=False, id_base=0):
    """The entry on the lists cand / sc with query groups qg against the restatement."""
    rows, _, q, _ = X.world(name)
    groups = _table(name, edited)
    ref = X.reference(name, metric)
    ids, dist = X.chain_ranking(name, metric)
    ntotal = len(rows)
    want_i, want_d, (one, zero, band), have, pos = X.rerank_expected(cand, sc, groups, qg, k, ids, dist, ref["s"], ref["E"], ref["qn"], ntotal, metric, id_base)
    got_i, got_d, cert, kth, flo = _entry(_index(name, metric, edited), q, cand, sc, qg, k, id_base)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_d), _bits(want_d))
    assert band.mean() <= 0.01, band.mean()
    assert (cert[one] == 1).all() and (cert[zero] == 0).all(), (np.flatnonzero(one & (cert != 1)), np.flatnonzero(zero & (cert != 0)))
    # the k-th allowed exact score: its bits where the flag is pinned at 1 (L2: through the distance it gives), -inf without k allowed candidates
    pin = np.flatnonzero(have & one)
    kth_dist = dist[pin, pos[pin]]
    if metric == 0:
        assert np.array_equal(_bits(kth[pin]), _bits(kth_dist))
    else:
        qn2 = oracle.chain_sqnorm(q)[pin]
        d2 = np.maximum(qn2 - np.float32(2.0) * kth[pin], np.float32(0.0)).astype(np.float32)      # (fmaf(-2, s, qn2): 2 s is exact, one rounding)
        assert np.array_equal(_bits(d2), _bits(kth_dist))
    E = ref["E"][pin]
    assert (flo[pin] < kth[pin] - E).all() and (flo[pin] >= kth[pin] - 1.01 * E - 1e-30).all()
    assert np.isneginf(kth[~have]).all() and np.isneginf(flo[~have]).all()
    return {"one": one, "zero": zero, "have": have, "allowed": X.allowed_mask(cand, groups, qg)}


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k_search,k", [(30, 30), (33, 33), (64, 64), (128, 30), (128, 120), (1, 1), (30, 1)])
def test_kernel_on_the_pass_lists_of_the_image_world(cuda_device, metric, k_search, k):
    """kc = 64, 72, 128 and 256 (the wide-first size: the lists of a search at k = 128), k from 1 to 120."""
    cand, sc = _pass_lists("image", metric, k_search)
    qg = X.image_world()[3]
    r = _check_kernel("image", metric, cand, sc, qg, k)
    assert r["one"].sum() >= 8 and r["zero"].sum() >= 8                  # both decisions occur ...
    assert (r["allowed"].sum(axis=1) == 0).any()                         # ... and lists that are excluded whole
    assert (~r["have"]).sum() >= 8


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k_search,k", [(30, 30), (33, 20)])
def test_kernel_with_d_40_and_70_queries(cuda_device, metric, k_search, k):
    """d is no multiple of 8 (the tiles' last block is guarded), the query count no multiple of the workgroup's four."""
    cand, sc = _pass_lists("small", metric, k_search)
    assert cand.shape[0] == 70
    r = _check_kernel("small", metric, cand, sc, X.small_world()[3], k)
    assert r["one"].sum() >= 1 and r["zero"].sum() >= 1


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k_search", [30, 128])
def test_kernel_on_edited_groups(cuda_device, metric, k_search):
    """The pass' lists with the groups chosen per query so that the excluded entries sit at positions 0, 63, 64 and kc - 1; a query that
    excludes nothing (-1), one that names a group without rows, rows in no group (-1 in the table: never excluded), and an id_base."""
    cand, sc = _pass_lists("image", metric, k_search)
    kc = cand.shape[1]
    groups = _table("image", True)
    qg = X.image_world()[3].copy()
    for i in range(len(qg)):
        p = (0, 63, 64, kc - 1)[i % 4]
        g = groups[cand[i, min(p, kc - 1)]]
        qg[i] = g if g >= 0 else qg[i]
    qg[9] = -1
    qg[11] = EMPTY_GROUP["image"]
    allowed = X.allowed_mask(cand, groups, qg)
    for p in (0, 63, min(64, kc - 1), kc - 1):
        assert (~allowed[:, p]).any(), p
    assert allowed[9].all() and allowed[11].all()
    assert (allowed & (groups[cand] == -1)).any()
    _check_kernel("image", metric, cand, sc, qg, 30, edited=True, id_base=1000)


@pytest.mark.parametrize("metric", [0, 1])
def test_kernel_on_lists_whose_tail_is_excluded(cuda_device, metric):
    """k allowed candidates followed by excluded ones only (excl_screen_refs.tail_excluded_lists): the threshold is the LIST's last pass score,
    and every query certifies."""
    cand, sc, qg = X.tail_excluded_lists(metric, 30, 64)
    r = _check_kernel("image", metric, cand, sc, qg, 30)
    assert r["one"].all()


@pytest.mark.parametrize("metric", [0, 1])
def test_kernel_on_a_bank_smaller_than_its_lists(cuda_device, metric):
    """50 rows: every list ends in -1 and every row was a candidate -- certified, with a missing tail where fewer than k rows are allowed."""
    cand, sc = _pass_lists("tiny", metric, 45)
    assert cand.shape[1] == R.kc_of(45) and (cand[:, 50:] == -1).all() and (cand[:, :50] >= 0).all()
    qg = X.tiny_world()[3]
    r = _check_kernel("tiny", metric, cand, sc, qg, 45)              # 40 allowed rows: the tail is missing
    assert r["one"].all() and not r["have"].any()
    r = _check_kernel("tiny", metric, cand, sc, qg, 8)
    assert r["one"].all() and r["have"].all()


# ---- 2. the route -----------------------------------------------------------------------------------------------------------------------
def _levels_ok(s, nq, second_pass=True, model=None):
    """model = (k, metric) of a PLAIN pass: the level counts EQUAL the host model's, (184, 31, 25) with the second pass and (184, 0, 56) without
    (tests/test_exclude_screen_cpu.py pins them; no decision of the model lies within 5 % of E of its threshold).  The centred pass has a bound
    of its own and no model here: its counts are held to their sums."""
    assert s["served"] == 1 and s["reason"] == "served"
    assert s["certified0"] >= 8 and s["rung_queries"] >= 8
    if second_pass:
        assert s["second_pass"] == nq - s["certified0"] and s["certified1"] >= 8
    else:
        assert s["second_pass"] == 0 and s["certified1"] == 0
    assert s["certified0"] + s["certified1"] + s["rung_queries"] == nq
    if model is not None:
        want = X.route_model(*model, escalation=second_pass)["counts"]
        assert (s["certified0"], s["certified1"], s["rung_queries"]) == want == ((184, 31, 25) if second_pass else (184, 0, 56)), (s, want)


@functools.lru_cache(maxsize=None)
def _route_off(metric, k):
    """search_excluding on the image world with the route off (the default): what test_exclude_gpu.py pins against views."""
    rows, groups, q, qg = X.image_world()
    ix = _index("image", metric)
    got = ix.search_excluding(torch.from_numpy(q).cuda(), k, torch.from_numpy(qg).cuda())
    return got, ix.last_exclusion(), ix.last_exclusion_screen(), ix.last_search_path()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k", [8, 30, 64])
def test_route_has_the_bits_of_the_rungs(cuda_device, metric, k):
    rows, groups, q, qg = X.image_world()
    want, excl_off, screen_off, path_off = _route_off(metric, k)
    # the default: not served, the parent's rule (gmax = 300: rung 0 at 256, rung 1 at k + 300)
    assert screen_off["served"] == 0 and screen_off["reason"] == "off" and path_off["path"] == "fp32"
    assert excl_off["rungs"] == 2 and excl_off["kf"] == k + 300 and excl_off["gmax"] == 300
    ix = _index("image", metric)
    qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
    ix.set_exclusion_screen(True)
    try:
        got = ix.search_excluding(qd, k, qgd)
        path, s, le = ix.last_search_path(), ix.last_exclusion_screen(), ix.last_exclusion()
        host = ix.search_excluding(q, k, qg)                            # host-memory inputs
        s_host = ix.last_exclusion_screen()
    finally:
        ix.set_exclusion_screen(False)
    _same(got, want)
    _same(host, want)
    assert path["path"] != "fp32"
    assert s["kc"] == R.kc_of(k) and s["centred"] == 0 and s_host == s
    _levels_ok(s, len(q), model=(k, metric))
    assert le["gmax"] == 300 and le["kf"] == k + 300 and le["rungs"] >= 1       # the leftover's rung run
    if k == 30:
        view_want, _ = _by_views(ix, groups, q, qg, _view_search(30))
        _same(got, view_want)


@pytest.mark.parametrize("metric", [0, 1])
def test_route_variants_keep_the_bits(cuda_device, metric):
    """Without the second pass, on the centred copy, with ordering scores and an id_base: the bits of the route off under the same setting."""
    rows, groups, q, qg = X.image_world()
    qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
    ix = _make_index("image", metric)
    try:
        want = ix.search_excluding(qd, 30, qgd)
        ix.set_exclusion_screen(True)
        # the second pass switched off: its queries go to the rungs
        ix.set_fp16_escalation(False)
        _same(ix.search_excluding(qd, 30, qgd), want)
        s = ix.last_exclusion_screen()
        _levels_ok(s, len(q), second_pass=False, model=(30, metric))
        ix.set_fp16_escalation(True)
        full = None
        _same(ix.search_excluding(qd, 30, qgd), want)
        full = ix.last_exclusion_screen()
        _levels_ok(full, len(q), model=(30, metric))
        assert full["certified0"] == s["certified0"] and full["rung_queries"] < s["rung_queries"]
        # ordering scores and an id_base
        _lib.check(_lib.lib().hb_index_set_score_output(ix._h, 1))
        try:
            got = ix.search_excluding(qd, 30, qgd, id_base=5000)
            assert ix.last_exclusion_screen()["served"] == 1
            ix.set_exclusion_screen(False)
            want_sc = ix.search_excluding(qd, 30, qgd, id_base=5000)
            ix.set_exclusion_screen(True)
        finally:
            _lib.check(_lib.lib().hb_index_set_score_output(ix._h, 0))
        _same(got, want_sc)
        assert np.array_equal(got[0].cpu().numpy(), np.where(want[0].cpu().numpy() >= 0, want[0].cpu().numpy() + 5000, -1))
        # the centred copy
        ix.set_fp16_centre(True)
        _same(ix.search_excluding(qd, 30, qgd), want)
        s = ix.last_exclusion_screen()
        assert s["centred"] == 1 and ix.last_search_path()["path"] != "fp32"
        _levels_ok(s, len(q))
    finally:
        ix.close()


# ---- 3. not served ----------------------------------------------------------------------------------------------------------------------
def test_searches_the_route_does_not_serve_are_the_rungs(cuda_device):
    rows, groups, q, qg = X.image_world()
    qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
    ix = _make_index("image", 0)
    try:
        for setting, k, reason in ((0, 30, "path"), (1, 129, "k")):
            ix.set_fp16(setting)
            ix.set_exclusion_screen(False)
            want, le = ix.search_excluding(qd, k, qgd), ix.last_exclusion()
            assert ix.last_exclusion_screen() == {"served": 0, "reason": "off", "kc": 0, "certified0": 0, "second_pass": 0, "certified1": 0,
                                                  "rung_queries": 0, "centred": 0}
            ix.set_exclusion_screen(True)
            _same(ix.search_excluding(qd, k, qgd), want)
            s = ix.last_exclusion_screen()
            assert s["served"] == 0 and s["reason"] == reason and ix.last_exclusion() == le
            assert ix.last_search_path()["path"] == "fp32"
    finally:
        ix.close()
    # need = k + gmax <= 128: the single rung is on the screen already (the 40-row groups of test_fp16_screen_serves_a_small_need)
    rows, _, q, _ = _shuffled_world()
    groups = (np.arange(len(rows)) // 40).astype(np.int32)
    qg = (np.arange(len(q)) % 38).astype(np.int32)
    ix = HipFlatIndex(rows.shape[1], 0, 0)
    try:
        ix.add(torch.from_numpy(rows).cuda()); ix.set_row_groups(groups); ix.set_fp16(1)
        qd, qgd = torch.from_numpy(q).cuda(), torch.from_numpy(qg).cuda()
        want, le = ix.search_excluding(qd, 8, qgd), ix.last_exclusion()
        ix.set_exclusion_screen(True)
        _same(ix.search_excluding(qd, 8, qgd), want)
        s = ix.last_exclusion_screen()
        assert s["served"] == 0 and s["reason"] == "need"
        assert ix.last_exclusion() == le == {"rungs": 1, "rung1_queries": 0, "kf": 48, "gmax": 40}
        assert ix.last_search_path()["path"] != "fp32"
    finally:
        ix.close()


def test_refusals_of_the_entry_leave_the_outputs_untouched(cuda_device):
    rows, groups, q, qg = X.image_world()
    cand, sc = _pass_lists("image", 0, 30)
    ix = _index("image", 0)
    L = _lib.lib()
    nq, k = len(q), 30
    qd, cd, sd, gd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, cand, sc, qg))
    oi = torch.full((nq, k), -77, dtype=torch.int64, device="cuda")
    od = torch.full((nq, k), 77.0, dtype=torch.float32, device="cuda")
    oc = torch.full((nq,), 77, dtype=torch.uint8, device="cuda")
    ok_, of_ = torch.full((nq,), 77.0, device="cuda"), torch.full((nq,), 77.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(h=ix._h, q_=qd, c_=cd, s_=sd, kc=64, g_=gd, k_=k, oi_=oi):
        return L.hb_index_exclude_rerank(h, p(q_) if q_ is not None else None, nq, p(c_) if c_ is not None else None, p(s_), kc,
                                         p(g_) if g_ is not None else None, k_, 0, p(oi_) if oi_ is not None else None, p(od), p(oc), p(ok_), p(of_))
    bare = HipFlatIndex(64, 0, 0)
    bare.add(torch.from_numpy(rows).cuda())
    try:
        for what, rc in (("kc % 8", call(kc=60)), ("kc < k", call(kc=24)), ("kc > 256", call(kc=264)), ("k < 1", call(k_=0)),
                         ("NULL q", call(q_=None)), ("NULL lists", call(c_=None)), ("NULL groups", call(g_=None)), ("NULL out", call(oi_=None)),
                         ("no table", call(h=bare._h))):
            assert rc != 0 and L.hb_last_error(), what
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (oi == -77).all() and (od == 77.0).all() and (oc == 77).all() and (ok_ == 77.0).all() and (of_ == 77.0).all()
    assert call() == 0                      # ... and the same buffers take a good call
    torch.cuda.synchronize()
    assert not (oi == -77).all() and not (oc == 77).any()


# ---- 4. the evaluator -------------------------------------------------------------------------------------------------------------------
def test_leave_one_out_on_the_screen_gives_the_same_floats(cuda_device):
    """Six training images of 64 px at patch 4: 256 rows per image, so k + gmax > 128 and the screen serves the pass."""
    from hbird_mi.data.synthetic import SyntheticSegDataModule
    from hbird_mi.hbird_eval import HbirdEvaluation
    from hbird_mi.models import FeatureExtractor
    from tiny_vit import TinyQKVViT
    C, PX, PS, D, N_IMG = 5, 64, 4, 16, 6
    S = PX // PS
    train = SyntheticSegDataModule(batch_size=4, input_size=PX, num_classes=C, n_train=N_IMG, n_val=2, seed=5).train_dataloader()
    fe = FeatureExtractor(TinyQKVViT(d=D, ps=PS, seed=3).cuda().eval(), eval_spatial_resolution=S, d_model=D)
    torch.manual_seed(1234)
    ev = HbirdEvaluation(fe, train, num_classes=C, n_neighbours=10, augmentation_epoch=1, device="cuda", nn_method="hip", nn_params={},
                         memory_size=None, dataset_size=N_IMG)
    ev.index.set_fp16(1)
    ks, betas = (3, 30), (0.02, 0.1)
    off = ev.evaluate_leave_one_out(train, S, n_neighbours=ks, betas=betas, screen=False)
    assert ev.loo_screen_served == 0 and ev.index.last_exclusion_screen()["reason"] == "off"
    on = ev.evaluate_leave_one_out(train, S, n_neighbours=ks, betas=betas, screen=True)
    assert ev.loo_screen_served >= 1 and ev.index.last_exclusion()["gmax"] == S * S
    assert on == off and list(on) == [(k, b) for k in ks for b in betas]
    same = ev.evaluate_leave_one_out(train, S, n_neighbours=ks, betas=betas)           # None: the indexes as they are (on)
    assert ev.loo_screen_served >= 1 and same == off
    ev.index.close()
