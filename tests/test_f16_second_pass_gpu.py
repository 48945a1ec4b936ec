"""The certified fp16 screen BEHIND its first candidate pass, on its own intermediate values (HipFlatIndex.last_screen_seeds()) against
tests/f16_second_pass_refs.py: the seeds level 0 hands on (kth0 on bits, floor0 between kth0 - 1.002 E and kth0 - E), the gather of the
failing queries and their seeds, the second pass' lists and pass scores (bits on exact worlds; H1 / H2 / the not-full rule within the
accumulation share A on float worlds), its certificates from both sides outside a 0.1 % band of E, and kth1 on bits.  A screened search
returns the fp32 search's bits whatever these are -- a failing certificate is searched again -- so none of them shows in a result.

Every case runs three indexes on one bank: set_fp16(1) without the second pass (its level-0 lists stay readable: the reference of kth0),
set_fp16(1) with it (the read-out under test), and set_fp16(0), whose ids and distance bits both screened searches must return.
Each case prints `F16SECOND {json}` with its figures (profiles/r23/README.md keeps them)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import f16_pass_refs as R
import f16_second_pass_refs as SR
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _index(dev, bank, metric, fp16, escalation=True, centre=False, rerank=0):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.set_fp16(fp16)
    if fp16:
        ix.set_fp16_escalation(escalation)
    if centre:
        ix.set_fp16_centre(True)
    if rerank:
        ix.set_rerank_copy(rerank)
    ix.add(torch.from_numpy(bank).to(dev))
    return ix


def _no_complaints(bad, c):
    assert not bad, f"{c.name}: " + " | ".join(bad.values())


def _bounds(c, W, ix0):
    """(E [nq], c_q [nq] or None): the bound by the Python restatement, from the norms of the world and -- centred -- from what the conversion
    left (HipFlatIndex.last_centre(), which tests/test_f16_centre_readout_gpu.py pins on its own references)."""
    qn, bmax, E = SR.plain_bounds(W["queries"], W["bank"], c.D, c.metric)
    if not c.centred:
        return E, None
    C = ix0.last_centre()
    assert C["level"] == 0 and C["n"] == c.nq
    return SR.bound_E_centred(qn, C["qcn"].astype(np.float64), bmax, float(C["cmax"]), float(C["mu_norm"]), float(C["t"]), c.D, c.metric), C["cq"]


def _run_case(dev, c, rerank=0):
    W = SR.case_world(c)
    q = torch.from_numpy(W["queries"]).to(dev)
    held = _index(dev, W["bank"], c.metric, 0)
    want = held.search(q, c.k)
    assert held.last_search_path()["path"] == "fp32"
    ix0 = _index(dev, W["bank"], c.metric, 1, escalation=False, centre=c.centred, rerank=rerank)
    got0 = ix0.search(q, c.k)
    L0, S0 = ix0.last_screen(), ix0.last_screen_seeds()
    E, cq = _bounds(c, W, ix0)
    ix1 = _index(dev, W["bank"], c.metric, 1, escalation=True, centre=c.centred, rerank=rerank)
    got1 = ix1.search(q, c.k)
    S = ix1.last_screen_seeds()
    C1 = ix1.last_centre() if c.centred and S["n1"] else None      # (the second pass' query side: its fp16 tiles, c_q, norms; the bank side as it is)
    assert ix1.last_search_path()["path"] == "fp16_chain" and bool(L0["centred"]) == c.centred == S["centred"], (c.name, ix1.last_search_path())
    assert _same(got0, want), f"{c.name}: the screened search without its second pass differs from the fp32 kernel's answer"
    assert _same(got1, want), f"{c.name}: the screened search with its second pass differs from the fp32 kernel's answer"
    out = {"W": W, "L0": L0, "S0": S0, "S": S, "E": E, "cq": cq, "C1": C1, "escalated": ix1.last_fp16_escalated(), "fallbacks": ix1.last_fp16_fallbacks()}
    held.close(); ix0.close(); ix1.close()
    return out


def _check_case(c, r):
    W, L0, S0, S, E, cq = r["W"], r["L0"], r["S0"], r["S"], r["E"], r["cq"]
    kc0 = R.kc_of(c.k)
    assert (S["nq"], S["kc0"], S["klw0"]) == (c.nq, kc0, R.klw_of(kc0)) == (S0["nq"], S0["kc0"], S0["klw0"]), c.name
    # without a second pass the same seeds lie behind the same certificates
    assert S0["n1"] == 0 and S0["queries1"].size == 0 and S0["n2"] == int((L0["certified"] == 0).sum()), c.name
    for name in ("kth0", "floor0", "certified0"):
        assert SR.same(S0[name], S[name]).all(), f"{c.name}: {name} differs between the searches with and without the second pass"
    assert np.array_equal(S0["certified0"], L0["certified"]), c.name
    skip = ~(SR.query_norms(W["queries"]) <= R.F16_LIMIT)
    bad, fig = SR.check_seeds(S, L0["rows"], L0["certified"], W["queries"], W["bank"], c.metric, c.k, E, cq)
    exact = W if c.world == "exact" else None
    # the list checks' reference: s16 of the plain pass (over the queries with finite fp16 operands), or -- centred -- the same sum over the
    # fp16 tiles and the row init that the conversion left, which tests/test_f16_centre_readout_gpu.py pins
    if exact is not None or (c.centred and not S["n1"]):
        ref = None
    elif c.centred:
        ref = SR.readout_centred_reference(r["C1"], S["queries1"], c.nq, c.N, c.D)
    else:
        ref = SR.finite_reference(W["queries"], W["bank"], c.metric, skip)
    bad1, fig1 = SR.check_level1(S, W["queries"], W["bank"], c.metric, c.k, E, ref=ref, exact=exact, cq=cq, skip=skip)
    bad.update({n: m for n, m in bad1.items() if n not in bad})
    bad.update(SR.check_n2(S))
    print("F16SECOND " + json.dumps(dict(name=c.name, D=c.D, N=c.N, nq=c.nq, k=c.k, metric=c.metric, centred=c.centred, n1=S["n1"], n2=S["n2"],
                                         certified1=int(S["certified1"].sum()), **fig, **fig1)))
    _no_complaints(bad, c)
    assert r["escalated"] == int((S["certified0"] == 0).sum()) and r["fallbacks"] == S["n2"], c.name
    if S["n1"]:
        assert (S["kc1"], S["klw1"]) == (256, 512) and S["rows1"].shape == (S["n1"], 256), c.name
    # the regime the case names, reached on the device as by the reference (tests/test_f16_second_pass_cpu.py)
    n_have = (S["rows1"] >= 0).sum(axis=1) if S["n1"] else np.zeros(0, int)
    if "not_full_certified" in c.regime:
        assert ((n_have < 256) & (S["certified1"] == 1)).any(), c.name
    if "full_failing" in c.regime:
        assert ((n_have == 256) & (S["certified1"] == 0)).any() and S["n2"] > 0, c.name
    if "all_level1" in c.regime:
        assert S["n1"] == c.nq > 256, (c.name, S["n1"])
    if "one_failing" in c.regime:
        assert S["n1"] == 1 and S["queries1"][0] == 41, (c.name, S["queries1"])
    if "centred" in c.regime:
        assert S["centred"] and np.isfinite(S["floor0"]).all(), c.name
    if "no_second_pass" in c.regime:
        assert S["kc0"] == 256 and S["n1"] == 0 and S["n2"] >= 10, (c.name, S["n1"], S["n2"])
    if "non_finite" in c.regime:
        assert np.isin([7, 23], S["queries1"]).all() and np.isneginf(S["kth0"][[7, 23]]).all() and np.isneginf(S["floor0"][[7, 23]]).all(), c.name
        j = np.searchsorted(S["queries1"], [7, 23])
        assert np.isneginf(S["seed1"][j]).all() and (S["certified1"][j] == 0).all() and np.isneginf(S["kth1"][j]).all() and S["n2"] >= 2, c.name
    if "gather" in c.regime:
        qn = SR.query_norms(W["queries"])
        at = (S["certified1"] == 0) & np.isin(S["queries1"], np.arange(0, 20, 2))      # the planted groups' queries (even places below 20)
        sent, k1 = S["queries1"][at], S["kth1"][at]
        short, long_ = (qn[sent] < 2.0).sum(), (qn[sent] > 2.0).sum()
        assert short >= 2 and long_ >= 2, f"{c.name}: {short} planted queries of norm 1 and {long_} of norm 8 reached the fp32 kernel"
        assert k1[qn[sent] > 2.0].min() > 4.0 * k1[qn[sent] < 2.0].max(), (c.name, k1)      # their k-th scores differ 8-fold: a seed handed to the wrong query changes results


@pytest.mark.parametrize("c", SR.CASES, ids=lambda c: c.name)
def test_seeds_gather_second_pass_and_flags(cuda_device, c):
    _check_case(c, _run_case(cuda_device, c))


@pytest.mark.parametrize("name", ["rounding100", "rounding300-l2"])
def test_the_rerank_row_copy_changes_nothing_behind_the_first_pass(cuda_device, name):
    c = next(x for x in SR.CASES if x.name == name)
    a, b = _run_case(cuda_device, c, rerank=1), _run_case(cuda_device, c, rerank=2)
    _check_case(c, a)
    for key in ("kth0", "floor0", "certified0", "queries1", "seed1", "rows1", "scores1", "certified1", "kth1"):
        assert SR.same(a["S"][key], b["S"][key]).all(), f"{name}: {key} differs with and without the re-rank's row copy"
    assert a["S"]["n2"] == b["S"]["n2"]


def test_last_screen_seeds_refusals(cuda_device):
    c = next(x for x in SR.CASES if x.name == "rounding100")
    W = SR.case_world(c)
    bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
    lib = _lib.lib()
    info = (ctypes.c_int64 * 8)(*([7] * 8))
    assert lib.hb_index_last_screen_seeds(None, *([None] * 9), 0, 0, info) != 0 and "NULL" in _lib.last_error() and list(info) == [7] * 8
    ix = HipFlatIndex(c.D, 0, 0)
    ix.add(bank)
    assert lib.hb_index_last_screen_seeds(ix._h, *([None] * 9), 0, 0, None) != 0 and "info is NULL" in _lib.last_error()
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):      # nothing searched yet
        ix.last_screen_seeds()
    ix.set_fp16(0); ix.search(q, c.k)
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen_seeds()
    ix.set_fp16(1); ix.set_fp16_escalation(True); ix.search(q, c.k)
    S = ix.last_screen_seeds()
    assert S["n1"] >= 10 and S["nq"] == c.nq
    with pytest.raises(_lib.HbirdHipError, match="second fp16 pass"):                          # the level-0 lists are gone, the seeds are not
        ix.last_screen()
    # info alone needs no room; too small a capacity is refused before anything is written, for either level
    assert lib.hb_index_last_screen_seeds(ix._h, *([None] * 9), 0, 0, info) == 0
    assert list(info) == [c.nq, 64, S["n1"], 256, 512, 0, S["n2"], 192]
    kth = np.full(c.nq, -7.0, np.float32)
    p = kth.ctypes.data_as(ctypes.c_void_p)
    assert lib.hb_index_last_screen_seeds(ix._h, p, *([None] * 8), c.nq - 1, 0, info) != 0 and f"room for {c.nq - 1} queries" in _lib.last_error()
    assert (kth == -7.0).all()
    seed = np.full(S["n1"], -7.0, np.float32)
    ps = seed.ctypes.data_as(ctypes.c_void_p)
    assert lib.hb_index_last_screen_seeds(ix._h, None, None, None, None, ps, None, None, None, None, 0, S["n1"] - 1, info) != 0
    assert "of the second pass" in _lib.last_error() and (seed == -7.0).all()
    assert lib.hb_index_last_screen_seeds(ix._h, p, None, None, None, ps, None, None, None, None, c.nq, S["n1"], info) == 0
    assert SR.same(kth, S["kth0"]).all() and SR.same(seed, S["seed1"]).all()
    # the record goes with the bank: add, reset, a capacity change; and with the next search
    ix.add(bank[:10])
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen_seeds()
    ix.search(q, c.k); ix.last_screen_seeds()
    ix.reserve(3 * c.N)
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen_seeds()
    ix.search(q, c.k); ix.last_screen_seeds()
    ix.reset()
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen_seeds()
    ix.add(bank); ix.search(q, c.k)
    S2 = ix.last_screen_seeds()
    for key in ("kth0", "floor0", "queries1", "seed1", "rows1", "scores1", "certified1", "kth1"):
        assert SR.same(S2[key], S[key]).all(), key
    ix.search(q, 200)                                                                           # k > 128: the fp32 kernel's
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen_seeds()
    ix.close()
