"""The 16x16x32 stage loop of the fp16 candidate kernel (csrc/hbird_knn_f16.hip) on its own output: HipFlatIndex.last_screen() against
tests/f16_pass_refs.py.  What this loop can get wrong that the 32x32x16 loop could not: the row permutation rho of the bank-fragment reads,
the lane swap at a tile's end, the pre-swap layout of the row-init values, the query fragments' lane offsets and the hand count of the
outstanding requests.  A wrong rho or swap names wrong rows; a wrong row-init layout shows only where the inits differ from row to row, so
the L2 metric (init -|b|^2 / 2) carries most cases -- inner product has all-zero inits.

EXACT worlds (integers in [-3, 3], optionally x 2^-5, no copied rows: dup_share = 0, so apart from the planted tie group every row of a
tile is its own): rows and score BITS equal the reference's, ties by lower row.  FLOAT worlds: |pass - s16| <= A, H1, H2 and the
certificate flags as tests/test_f16_candidates_gpu.py checks them (the summation order inside a k32 differs from the 32x32x16 loop's, the
bound does not).  CENTRED: H1 / H2 / flags under E'.  Every search is also compared with the fp32 kernel's ids and distance bits.

Shapes: D = 64 (one unrolled group of four stages per tile), 136 (zero padding up to 256), 384, 768 (three laps of the ring per tile); banks
of 200, 1,000 and 5,000 rows (ragged last tiles); 1, 70 and 300 queries (padding queries, two query tiles); k = 30 (k' = 64: <4>) and 90
(k' = 184: <8>); 3 and 64 workgroups, phases on and off; one 8 x 1 clustered case with sharing at 20,000 x 64."""
import collections
import json

import numpy as np
import pytest
import torch

import f16_pass_refs as R
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

Exact = collections.namedtuple("Exact", "D N nq k metric scale G opt")
EXACT_CASES = [
    Exact(64, 200, 1, 30, 1, 0, 0, ""),
    Exact(64, 1000, 70, 90, 1, -5, 3, ""),
    Exact(64, 5000, 300, 30, 0, 0, 64, ""),
    Exact(136, 200, 70, 90, 1, 0, 0, ""),
    Exact(136, 1000, 300, 30, 1, -5, 3, "phases_off"),
    Exact(136, 5000, 1, 90, 0, 0, 64, ""),
    Exact(384, 200, 300, 30, 1, 0, 0, ""),
    Exact(384, 1000, 1, 90, 1, 0, 64, "phases_off"),
    Exact(384, 5000, 70, 30, 1, -5, 3, ""),
    Exact(768, 200, 70, 30, 0, -5, 0, ""),
    Exact(768, 1000, 300, 90, 1, 0, 3, ""),
    Exact(768, 5000, 300, 30, 1, 0, 64, ""),
    Exact(768, 5000, 70, 90, 1, 0, 3, "phases_off"),
    Exact(64, 20000, 300, 30, 1, 0, 64, "cluster"),
]

Float = collections.namedtuple("Float", "world D N nq k metric G")
FLOAT_CASES = [
    Float("normal", 64, 5000, 70, 30, 1, 3),
    Float("normal", 136, 1000, 300, 90, 0, 0),
    Float("normal", 384, 5000, 70, 30, 1, 64),
    Float("normal", 768, 5000, 300, 90, 1, 3),
    Float("rounding", 768, 5000, 64, 30, 1, 8),
]

Centred = collections.namedtuple("Centred", "world D N nq k metric")
CENTRED_CASES = [
    Centred("shared_mean", 64, 5000, 70, 30, 1),
    Centred("shared_mean", 136, 1000, 70, 30, 1),
    Centred("massive_activation", 384, 5000, 70, 30, 1),
    Centred("massive_activation", 768, 1000, 300, 90, 1),
]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _screened(dev, bank, metric, G=0, opt="", centre=False):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.set_fp16(True); ix.set_fp16_escalation(False)
    if centre:
        ix.set_fp16_centre(True)
    if G:
        ix.set_tuning(workgroups=G)
    if opt == "phases_off":
        ix.set_search_options(phases=False)
    if opt == "cluster":
        ix.set_cluster(8, 1); ix.set_cluster_sharing(2)
    ix.add(torch.from_numpy(bank).to(dev))
    return ix


def _held(dev, bank, metric):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.set_fp16(False)
    ix.add(torch.from_numpy(bank).to(dev))
    return ix


def _regime(ix, L, c, kc):
    """The case reached what it names: the fp16 path, k' and the pools' capacity (hence the instantiation), the work list's shape."""
    assert ix.last_search_path()["path"] == "fp16_chain", (c, ix.last_search_path())
    assert (L["nq"], L["kc"], L["klw"]) == (c.nq, kc, R.klw_of(kc)) and L["rows"].shape == (c.nq, kc), (c, L["nq"], L["kc"], L["klw"])
    assert (kc, L["klw"]) == {30: (64, 192), 90: (184, 384)}[c.k]            # 192 <= 256: <4>; 384: <8>
    info = ix.schedule_info()
    assert info["query_tiles"] == (c.nq + 255) // 256 and info["bank_tiles"] == (c.N + 255) // 256, (c, info)
    G = getattr(c, "G", 0)
    if G:
        assert info["workgroups"] == G or info["query_tiles"] * info["bank_tiles"] < G, (c, info)
    if getattr(c, "opt", "") == "cluster":
        assert info["cluster"] == [8, 1], (c, info)


def _no_complaints(bad, c):
    assert not bad, f"{c}: " + " | ".join(f"[{n}] {m}" for n, m in bad.items())


@pytest.mark.parametrize("c", EXACT_CASES, ids=lambda c: f"D{c.D}-N{c.N}-nq{c.nq}-k{c.k}-m{c.metric}-s{c.scale}-G{c.G}{'-' + c.opt if c.opt else ''}")
def test_exact_worlds_rows_and_score_bits(cuda_device, c):
    kc = R.kc_of(c.k)
    W = R.exact_world(c.N, c.D, c.nq, kc, 23, c.scale, 0.0)
    twins = np.nonzero(W["dup"])[0]
    assert np.isin(twins, W["heavy"]).all(), "apart from the planted tie group no row has a twin: a permuted tile names other rows"
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    held = _held(cuda_device, W["bank"], c.metric)
    want = held.search(q, c.k)
    assert held.last_search_path()["path"] == "fp32"
    ix = _screened(cuda_device, W["bank"], c.metric, c.G, c.opt)
    got = ix.search(q, c.k)
    L = ix.last_screen()
    _regime(ix, L, c, kc)
    _no_complaints(R.check_exact(L["rows"], L["scores"], W, c.metric, kc), c)
    assert _same(got, want), f"{c}: the screened search differs from the fp32 kernel's answer"
    ix.close(); held.close()


@pytest.mark.parametrize("c", FLOAT_CASES, ids=lambda c: f"{c.world}-D{c.D}-N{c.N}-nq{c.nq}-k{c.k}-m{c.metric}-G{c.G}")
def test_float_worlds_accumulation_h1_h2_and_flags(cuda_device, c):
    kc = R.kc_of(c.k)
    W = R.float_world(c.world, c.N, c.D, c.nq, c.k, c.metric)
    ref = R.float_world_reference(c.world, c.N, c.D, c.nq, c.k, c.metric)
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    ix, held = _screened(cuda_device, W["bank"], c.metric, c.G), _held(cuda_device, W["bank"], c.metric)
    got, want = ix.search(q, c.k), held.search(q, c.k)
    L = ix.last_screen()
    _regime(ix, L, c, kc)
    bad, fig = R.check_float(L["rows"], L["scores"], L["certified"], ref, c.k, kc)
    print("F16PASS " + json.dumps(dict(c._asdict(), kc=kc, certified_share=float(L["certified"].mean()), **fig)))
    _no_complaints(bad, c)
    assert ix.last_fp16_escalated() == int((L["certified"] == 0).sum()) == ix.last_fp16_fallbacks(), c
    assert _same(got, want), f"{c}: the screened search differs from the fp32 kernel's answer"
    ix.close(); held.close()


@pytest.mark.parametrize("c", CENTRED_CASES, ids=lambda c: f"{c.world}-D{c.D}-N{c.N}-nq{c.nq}-k{c.k}-m{c.metric}")
def test_centred_form_h1_h2_and_flags(cuda_device, c):
    kc = R.kc_of(c.k)
    W = R.float_world(c.world, c.N, c.D, c.nq, c.k, c.metric)
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    ix, held = _screened(cuda_device, W["bank"], c.metric, centre=True), _held(cuda_device, W["bank"], c.metric)
    got, want = ix.search(q, c.k), held.search(q, c.k)
    L, info = ix.last_screen(), ix.fp16_centre_info()
    assert ix.last_search_path()["path"] == "fp16_chain" and L["centred"] and info["centred"] and info["last_search_centred"], (c, info)
    _regime(ix, L, c, kc)
    bad, fig = R.check_centred(L["rows"], L["scores"], L["certified"], W["queries"], W["bank"], c.metric, c.k, kc, info)
    print("F16PASS " + json.dumps(dict(c._asdict(), kc=kc, centred=True, certified_share=float(L["certified"].mean()), **fig)))
    _no_complaints(bad, c)
    assert ix.last_fp16_escalated() == int((L["certified"] == 0).sum()), c
    assert _same(got, want), f"{c}: the screened search differs from the fp32 kernel's answer"
    ix.close(); held.close()
