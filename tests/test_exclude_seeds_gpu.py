"""An excluding search on the certified fp16 screen (set_exclusion_screen) BEHIND its passes, on its own intermediate values -- last_screen(),
last_screen_seeds() and last_exclusion_seeds() after the search, the leftover's rungs notwithstanding -- against tests/excl_screen_refs.py:
the level-0 lists and pass scores, which know nothing of groups (H1 / H2 as f16_pass_refs.check_float has them, bits on exact worlds,
the centred H1 / H2), kth0 on bits over the ALLOWED candidates of the unmasked level-0 list, floor0 between kth0 [- c_q] - 1.002 E and
kth0 [- c_q] - E, the first certificates from both sides outside the 0.1 % band, the gather of the failing queries, their seeds and their GROUPS, the second lists (bits
on exact worlds; H1 / H2 / the not-full rule within A on float worlds), kth1 on bits over the allowed entries, the second certificates (full
and at least k allowed: kth1 > last + E; full and fewer: 0; not full: the seed rule; non-finite: 0), the queries handed to the rungs, and the
answer: ids and distance bits of the fp32 chain ranking restricted to the allowed rows -- on its own for the queries the not-full rule
certified, where it is the soundness statement.  A query that fails wrongly goes to the rungs and a floor that is too high hides behind the
not-full rule: neither shows in a result of the worlds searched so far.

Every case runs two indexes on one bank, both with the route on: without the second pass (its level-0 lists stay readable: the reference of
kth0) and with it (the read-out under test).  Each case prints `EXCLSEEDS {json}` with its figures (profiles/r24/README.md keeps them)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import excl_screen_refs as X
import f16_pass_refs as R
import f16_second_pass_refs as SR
import oracle
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu
KEYS0 = ("kth0", "floor0", "certified0")
KEYS1 = ("queries1", "seed1", "rows1", "scores1", "certified1", "kth1")


def _index(dev, name, escalation, rerank=0, route=True):
    c, W, groups, n_groups, qg = X.excl_case(name)
    ix = HipFlatIndex(c.D, c.metric, 0)
    ix.set_fp16(1)
    ix.set_fp16_escalation(escalation)
    if c.centred:
        ix.set_fp16_centre(True)
    if rerank:
        ix.set_rerank_copy(rerank)
    ix.add(torch.from_numpy(W["bank"]).to(dev))
    ix.set_row_groups(groups, n_groups)
    ix.set_exclusion_screen(route)
    return ix


def _bounds(c, W, ix0):
    """(E [nq], c_q [nq] or None): the bound by the library's constants (X.bounds); centred: the Python restatement of E' on what the
    conversion left (HipFlatIndex.last_centre(), which tests/test_f16_centre_readout_gpu.py pins on its own references)."""
    qn, bmax, E = X.bounds(W["queries"], W["bank"], c.D, c.metric)
    if not c.centred:
        return E, None
    C = ix0.last_centre()
    assert C["level"] == 0 and C["n"] == c.nq
    return SR.bound_E_centred(qn, C["qcn"].astype(np.float64), bmax, float(C["cmax"]), float(C["mu_norm"]), float(C["t"]), c.D, c.metric), C["cq"]


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _run(dev, name, rerank=0):
    c, W, groups, n_groups, qg = X.excl_case(name)
    q, qgd = torch.from_numpy(W["queries"]).to(dev), torch.from_numpy(qg).to(dev)
    ix0 = _index(dev, name, False, rerank)
    got0 = _np(ix0.search_excluding(q, c.k, qgd))
    r = {"s0": ix0.last_exclusion_screen(), "L0": ix0.last_screen(), "S0": ix0.last_screen_seeds(), "X0": ix0.last_exclusion_seeds(), "got0": got0}
    r["E"], r["cq"] = _bounds(c, W, ix0)       # (centred: last_centre() answers behind the rungs as well)
    r["centre_info"] = ix0.fp16_centre_info() if c.centred else None
    if not c.centred and r["s0"]["rung_queries"]:      # ... and so does the query side of last_fp16_copy(): the fp32 rungs write no fp16 tiles
        C = ix0.last_fp16_copy()
        assert C["n"] == c.nq and C["level"] == 0, (name, C["n"], C["level"])
        fin = SR.query_norms(W["queries"]) <= R.F16_LIMIT
        if fin.all():
            assert not SR.check_copy(C, W["queries"], None, key="q16"), name
    ix0.close()
    ix1 = _index(dev, name, True, rerank)
    r["got1"] = _np(ix1.search_excluding(q, c.k, qgd))
    r.update(s1=ix1.last_exclusion_screen(), S=ix1.last_screen_seeds(), X1=ix1.last_exclusion_seeds(), path=ix1.last_search_path(), fallbacks=ix1.last_fp16_fallbacks())
    r["C1"] = ix1.last_centre() if c.centred and r["S"]["n1"] else None
    ix1.set_exclusion_screen(False)
    r["rungs"] = _np(ix1.search_excluding(q, c.k, qgd))
    assert ix1.last_exclusion_screen()["served"] == 0
    with pytest.raises(_lib.HbirdHipError, match="not an excluding one served"):
        ix1.last_exclusion_seeds()
    ix1.close()
    return r


def _check(name, r):
    c, W, groups, n_groups, qg = X.excl_case(name)
    L0, S0, S, X0, X1, E, cq = r["L0"], r["S0"], r["S"], r["X0"], r["X1"], r["E"], r["cq"]
    kc0 = R.kc_of(c.k)
    for s in (r["s0"], r["s1"]):
        assert s["served"] == 1 and s["kc"] == kc0 and s["centred"] == int(c.centred), (name, s)
    assert r["path"]["path"] == "fp16_chain" and (S["nq"], S["kc0"], S0["kc0"], L0["kc"]) == (c.nq, kc0, kc0, kc0) and S["centred"] == c.centred == L0["centred"], name
    q, bank = W["queries"], W["bank"]
    skip = ~(SR.query_norms(q) <= R.F16_LIMIT)
    # without the second pass: the same seeds behind the same certificates, and every failing query named for the rungs
    assert S0["n1"] == 0 and X0["n1"] == 0 and r["s0"]["second_pass"] == 0 and r["s0"]["certified1"] == 0, name
    for key in KEYS0:
        assert SR.same(S0[key], S[key]).all(), f"{name}: {key} differs between the searches with and without the second pass"
    bad0, _ = X.check_excl_chain(S0, L0, X0, r["s0"], groups, qg, q, bank, c.metric, c.k, E, cq=cq, skip=skip)
    assert not bad0, f"{name} without the second pass: " + " | ".join(bad0.values())
    # the level-0 lists and pass scores themselves, read behind the rungs
    exact = W if c.world == "exact" else None
    badl, figl = X.check_level0_lists(L0["rows"], L0["scores"], q, bank, c.metric, c.k, exact=exact, centre_info=r["centre_info"])
    assert not badl, f"{name}: " + " | ".join(badl.values())
    if name == "centred-clusters-neg":
        assert r["s0"]["rung_queries"] > 0, name      # (its centred read-out, last_centre() in _bounds, came after a rung run)
    assert np.array_equal(X0["left"], np.flatnonzero(L0["certified"] == 0)), name
    # with it
    if exact is not None or (c.centred and not S["n1"]):
        ref = None
    elif c.centred:
        ref = SR.readout_centred_reference(r["C1"], S["queries1"], c.nq, c.N, c.D)
    else:
        ref = SR.finite_reference(q, bank, c.metric, skip)
    bad, fig = X.check_excl_chain(S, L0, X1, r["s1"], groups, qg, q, bank, c.metric, c.k, E, ref=ref, exact=exact, cq=cq, skip=skip)
    counts = (int(S["certified0"].sum()), int(S["certified1"].sum()), int(X1["left"].size))
    # the answer: the fp32 chain ranking restricted to the allowed rows (the best k allowed rows lie among the best k + gmax)
    gmax = int(np.bincount(groups[groups >= 0]).max())
    fin = ~skip
    ids, dist = oracle.knn_chain_f32(np.ascontiguousarray(q[fin]), bank, c.k + gmax, X.METRIC_NAME[c.metric])
    want = X.allowed_ranking(ids, dist, groups, qg[fin], c.k, c.metric)
    n_have = (S["rows1"] >= 0).sum(axis=1) if S["n1"] else np.zeros(0, int)
    by_seed_rule = np.zeros(c.nq, bool)
    by_seed_rule[S["queries1"][(n_have < SR.KC1) & (S["certified1"] == 1)]] = True
    for label, got in (("", r["got1"]), ("without the second pass: ", r["got0"])):
        bad.update({n: m for n, m in X.check_answer(got[0][fin], got[1][fin], *want, what=label).items() if n not in bad})
        assert np.array_equal(got[0], r["rungs"][0]) and SR.same(got[1], r["rungs"][1]).all(), f"{name}: {label}the route's answer differs from the rungs'"
    sound = X.check_answer(r["got1"][0][fin], r["got1"][1][fin], *want, which=by_seed_rule[fin], what="certified by the not-full rule: ")
    print("EXCLSEEDS " + json.dumps(dict(name=name, D=c.D, N=c.N, nq=c.nq, k=c.k, metric=c.metric, centred=c.centred, table=X.ECASE[name].table, counts=counts,
                                         by_seed_rule=int(by_seed_rule.sum()), **fig, **figl)))
    assert not sound, f"{name}: " + " | ".join(sound.values())
    assert not bad, f"{name}: " + " | ".join(bad.values())
    assert (r["s1"]["certified0"], r["s1"]["certified1"], r["s1"]["rung_queries"], r["s1"]["second_pass"]) == counts + (S["n1"],), (name, r["s1"], counts)
    assert r["fallbacks"] == counts[2] and sum(counts) == c.nq, name
    if S["n1"]:
        assert (S["kc1"], S["klw1"]) == (256, 512) and S["rows1"].shape == (S["n1"], 256) and X1["n1"] == S["n1"], name
    # the regimes the case is there for, reached on the device as by the reference (tests/test_exclude_seeds_cpu.py)
    reached = X.regimes_reached(name, S, X1["left"], fig, cq, E)
    assert set(X.REGIMES[name]) <= reached, f"{name} is there for {X.REGIMES[name]} and reaches {sorted(reached)} on the device: {fig}"
    return counts, fig


@pytest.mark.parametrize("name", [n for n in X.ECASE if not n.startswith("image")])
def test_seeds_groups_second_pass_flags_and_hand_over(cuda_device, name):
    _check(name, _run(cuda_device, name))


@pytest.mark.parametrize("name,metric", [("image", 0), ("image-l2", 1)])
def test_the_image_world_has_the_model_counts_on_the_device(cuda_device, name, metric):
    """The unseeded regime and the lists of 256 excluded rows; no decision of the model lies within 5 % of E of its threshold
    (tests/test_exclude_screen_cpu.py), so the device's level counts EQUAL the model's."""
    r = _run(cuda_device, name)
    counts, fig = _check(name, r)
    assert counts == X.route_model(30, metric)["counts"] == (184, 31, 25), counts
    s0 = r["s0"]
    assert (s0["certified0"], s0["certified1"], s0["rung_queries"]) == X.route_model(30, metric, escalation=False)["counts"] == (184, 0, 56), s0
    assert fig["band_share0"] == 0.0 and fig["band_share1"] == 0.0 and np.isneginf(r["S"]["seed1"]).all()


def test_the_rerank_row_copy_changes_nothing(cuda_device):
    """An excluding re-rank reads the tiles whether or not the index keeps the row copy."""
    a, b = _run(cuda_device, "rounding100", rerank=1), _run(cuda_device, "rounding100", rerank=2)
    _check("rounding100", a)
    for key in KEYS0 + KEYS1:
        assert SR.same(a["S"][key], b["S"][key]).all(), f"{key} differs with and without the re-rank's row copy"
    for key in ("groups1", "left"):
        assert np.array_equal(a["X1"][key], b["X1"][key]), key
    assert np.array_equal(a["got1"][0], b["got1"][0]) and SR.same(a["got1"][1], b["got1"][1]).all() and a["s1"] == b["s1"]


def test_queries_that_exclude_nothing_leave_the_plain_chain(cuda_device):
    """The `edited` case: every third query names no group (-1) and query 1 a group without rows.  Their whole chain -- seeds, certificates,
    second lists, k-th scores -- equals, on bits, what a plain search of the same queries leaves."""
    c, W, groups, n_groups, qg = X.excl_case("edited")
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    ix = _index(cuda_device, "edited", True)
    ix.search_excluding(q, c.k, torch.from_numpy(qg).to(cuda_device))
    S = ix.last_screen_seeds()
    ix.search(q, c.k)
    P = ix.last_screen_seeds()
    ix.close()
    free = np.flatnonzero((qg == -1) | (qg == n_groups - 1))
    assert free.size >= 20 and P["n1"] > 0 and S["n1"] > 0
    for key in KEYS0:
        assert SR.same(S[key][free], P[key][free]).all(), key
    both = free[S["certified0"][free] == 0]
    assert both.size >= 2 and np.isin(both, S["queries1"]).all() and np.isin(both, P["queries1"]).all()
    js, jp = np.searchsorted(S["queries1"], both), np.searchsorted(P["queries1"], both)
    for key in KEYS1[1:]:
        assert SR.same(S[key][js], P[key][jp]).all(), key
    # ... while a query that does name a group differs from its plain self somewhere
    named = np.flatnonzero((qg >= 0) & (qg < n_groups - 1))
    assert (~SR.same(S["kth0"][named], P["kth0"][named])).any()


def test_last_exclusion_seeds_refusals_and_the_life_of_the_record(cuda_device):
    c, W, groups, n_groups, qg = X.excl_case("rounding300")
    q, qgd = torch.from_numpy(W["queries"]).to(cuda_device), torch.from_numpy(qg).to(cuda_device)
    lib = _lib.lib()
    info = (ctypes.c_int64 * 2)(7, 7)
    ix = _index(cuda_device, "rounding300", True)
    assert lib.hb_index_last_exclusion_seeds(ix._h, None, None, 0, 0, None) != 0 and "info is NULL" in _lib.last_error()
    with pytest.raises(_lib.HbirdHipError, match="not an excluding one served"):                # nothing searched yet
        ix.last_exclusion_seeds()
    ix.search(q, c.k)                                                                           # a plain screened search
    with pytest.raises(_lib.HbirdHipError, match="not an excluding one served"):
        ix.last_exclusion_seeds()
    ix.search_excluding(q, c.k, qgd)
    S, X1, s = ix.last_screen_seeds(), ix.last_exclusion_seeds(), ix.last_exclusion_screen()
    assert s["rung_queries"] == X1["n_left"] == S["n2"] >= 10 and ix.last_exclusion()["rungs"] >= 1      # the rungs ran, the record is back
    with pytest.raises(_lib.HbirdHipError, match="second fp16 pass"):                           # (the level-0 lists are gone, as after a plain search)
        ix.last_screen()
    # the sizes alone need no room; too small a capacity is refused before anything is written
    assert lib.hb_index_last_exclusion_seeds(ix._h, None, None, 0, 0, info) == 0 and list(info) == [S["n1"], X1["n_left"]]
    g = np.full(S["n1"], -7, np.int32); left = np.full(X1["n_left"], -7, np.int64)
    pg, pl = g.ctypes.data_as(ctypes.c_void_p), left.ctypes.data_as(ctypes.c_void_p)
    assert lib.hb_index_last_exclusion_seeds(ix._h, pg, None, S["n1"] - 1, 0, info) != 0 and "of the second pass" in _lib.last_error() and (g == -7).all()
    assert lib.hb_index_last_exclusion_seeds(ix._h, None, pl, 0, X1["n_left"] - 1, info) != 0 and "of the rungs" in _lib.last_error() and (left == -7).all()
    assert lib.hb_index_last_exclusion_seeds(ix._h, pg, pl, S["n1"], X1["n_left"], info) == 0
    assert np.array_equal(g, X1["groups1"]) and np.array_equal(left, X1["left"])
    # the record goes with the bank, with the next search, and with a search the route does not serve
    ix.add(torch.from_numpy(W["bank"][:10]).to(cuda_device))
    for read in (ix.last_exclusion_seeds, ix.last_screen_seeds):
        with pytest.raises(_lib.HbirdHipError):
            read()
    ix.set_row_groups(np.concatenate([groups, groups[:10]]), n_groups)
    ix.search_excluding(q, c.k, qgd); ix.last_exclusion_seeds(); ix.last_screen_seeds()
    ix.set_fp16(0)
    ix.search_excluding(q, c.k, qgd)
    assert ix.last_exclusion_screen()["reason"] == "path"
    for read in (ix.last_exclusion_seeds, ix.last_screen_seeds):
        with pytest.raises(_lib.HbirdHipError):
            read()
    ix.close()
