"""The fp16 candidate pass on its OWN output (HipFlatIndex.last_screen(): candidate rows, pass scores, first certificates) against
tests/f16_pass_refs.py.  A screened search returns the fp32 search's bits whatever the candidate kernel delivers -- failed certificates are
searched again -- so a kernel that loses rows or mis-scores them shows in no (idx, dist); here it shows as "candidate j of query i, bank
tile t".  Every index runs at set_fp16(1) with set_fp16_escalation(False): failures go straight to the fp32 kernel and the first pass's
lists stay in place.

EXACT worlds (integers in [-3, 3], optionally x 2^-5): rows and score BITS equal the reference's, ties by lower row.
FLOAT worlds: |pass - s16| <= A (the accumulation share of E; + S on the subnormal world), H1 |pass - s| <= E, H2 through the reference
(outside rows: s16[r] <= pass[kc-1] + A_r), clear reference candidates present, and the certificate flags from both sides outside a 0.1 %
band of E (the device's fp32 evaluation of E and of the comparison; queries inside it are skipped, at most 1 % of a case).
CENTRED form: H1 / H2 / flags with E' as the re-rank states them.

Each float case prints `F16PASS {json}` with max |pass - s16| / A, max |pass - s| / E and the band share (profiles/r17/README.md keeps them).

The cases are the smallest that reach each regime of the kernel: D = 64 (four k32 stages per tile: every unrolled iteration ends a tile), 200
(zero padding inside a k16 group), 384, 768 (24 stages: three laps of the 8-slot ring per tile), 1024; banks of 200 (< k' = 256), 256, 257,
2,049, 5,000 and 20,000 rows; 1 .. 700 queries; k = 1 / 30 / 90 / 128 (k' = 64 / 64 / 184 / 256: both instantiations, pools of 192 / 384 / 512)."""
import collections
import ctypes
import json

import numpy as np
import pytest
import torch

import f16_centre_refs as CR
import f16_pass_refs as R
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

Exact = collections.namedtuple("Exact", "D N nq k metric scale G opt")
# G: set_tuning(workgroups) (0: the default); opt: what else the case turns on
EXACT_CASES = [
    Exact(64, 200, 33, 128, 0, 0, 0, ""),               # fewer rows than k' = 256: -1 / -inf at the tail, every query certified
    Exact(64, 200, 1, 1, 1, -5, 0, ""),
    Exact(64, 256, 1, 90, 1, 0, 0, ""),                 # exactly one bank tile
    Exact(200, 257, 33, 30, 0, -5, 0, ""),              # one row in the second tile
    Exact(200, 2049, 257, 128, 1, 0, 0, ""),            # two query tiles, nine bank tiles, <8>
    Exact(384, 2049, 256, 1, 0, 0, 0, ""),
    Exact(1024, 257, 257, 90, 0, 0, 0, ""),
    Exact(768, 5000, 700, 90, 1, -5, 3, ""),            # three workgroups walk multi-tile strided segments
    Exact(1024, 5000, 257, 30, 0, 0, 8, ""),            # several slots share a query tile
    Exact(64, 5000, 700, 128, 0, 0, 64, ""),            # more workgroups than (query tile, bank tile) pairs
    Exact(384, 5000, 33, 30, 1, 0, 8, ""),
    Exact(768, 20000, 700, 90, 0, 0, 8, ""),            # phases on (the default) ...
    Exact(768, 20000, 700, 90, 0, 0, 8, "phases_off"),  # ... and off
    Exact(64, 20000, 257, 30, 1, -5, 3, "phases_off"),
    Exact(384, 20000, 700, 128, 1, 0, 64, "cluster"),   # 8 x 1 clusters, XCD-level sharing on
    Exact(64, 20000, 257, 30, 1, 0, 64, "xcd"),         # given, uneven XCD shares
    Exact(200, 20000, 257, 128, 0, 0, 64, "xcd"),
    Exact(200, 20000, 256, 128, 0, -5, 8, "rerank"),    # with and without the re-rank's row copy: the candidates do not change
    Exact(1024, 20000, 33, 90, 1, 0, 8, "append"),      # rows appended after the fp16 copy exists
    Exact(384, 20000, 1, 1, 0, 0, 64, ""),              # one query, 79 bank tiles over 64 workgroups
]

Float = collections.namedtuple("Float", "world D N nq k metric G")
FLOAT_CASES = [
    Float("rounding", 64, 5000, 64, 30, 0, 0),
    Float("rounding", 768, 5000, 64, 90, 1, 8),
    Float("rounding", 384, 5000, 64, 30, 1, 3),
    Float("shared_mean", 384, 5000, 257, 30, 1, 8),
    Float("shared_mean", 200, 2049, 33, 128, 0, 0),
    Float("massive_activation", 768, 5000, 257, 90, 0, 8),
    Float("massive_activation", 200, 2049, 256, 1, 1, 0),       # (at D = 64 this world has 1.2 % of its queries inside the flag band, by the reference alone)
    Float("duplicate_background", 200, 5000, 257, 128, 0, 64),
    Float("duplicate_background", 1024, 5000, 33, 30, 1, 3),
    Float("subnormal", 64, 2049, 33, 30, 0, 0),
    Float("subnormal", 384, 2049, 33, 90, 1, 0),
    Float("near_limit", 1024, 2049, 33, 30, 1, 0),
    Float("near_limit", 200, 5000, 64, 128, 0, 8),
    Float("normal", 64, 20000, 257, 1, 0, 8),
    Float("normal", 768, 20000, 257, 90, 1, 64),
    Float("normal_raw", 768, 20000, 257, 128, 1, 64),
    Float("normal_raw", 1024, 5000, 33, 30, 0, 3),
    Float("normal_raw", 384, 257, 1, 30, 0, 0),
]

Centred = collections.namedtuple("Centred", "world D N nq k metric")
CENTRED_CASES = [
    Centred("massive_activation", 384, 5000, 257, 30, 0),
    Centred("massive_activation", 384, 5000, 257, 30, 1),
    Centred("massive_activation", 768, 2049, 33, 90, 0),
    Centred("shared_mean", 768, 20000, 257, 90, 0),
    Centred("shared_mean", 64, 5000, 256, 128, 1),
]


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _screened(dev, bank, metric, G=0, opt="", centre=False):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.set_fp16(1); ix.set_fp16_escalation(False)
    if centre:
        ix.set_fp16_centre(True)
    if G:
        ix.set_tuning(workgroups=G)
    if opt == "phases_off":
        ix.set_search_options(phases=False)
    if opt == "cluster":
        ix.set_cluster(8, 1); ix.set_cluster_sharing(2)
    if opt == "xcd":
        ix.set_xcd_weights(2, np.random.default_rng(5).uniform(0.8, 1.25, size=8).tolist())
    if bank.shape[0]:
        ix.add(torch.from_numpy(bank).to(dev))
    return ix


def _held(dev, bank, metric):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.set_fp16(0)
    ix.add(torch.from_numpy(bank).to(dev))
    return ix


def _regime(ix, L, c, kc, N):
    """The case reached what it names: the fp16 path, k' and the pools' capacity (hence the instantiation), the work list's shape."""
    assert ix.last_search_path()["path"] == "fp16_chain", (c, ix.last_search_path())
    assert (L["nq"], L["kc"], L["klw"]) == (c.nq, kc, R.klw_of(kc)) and L["rows"].shape == (c.nq, kc), (c, L["nq"], L["kc"], L["klw"])
    assert kc == {1: 64, 30: 64, 90: 184, 128: 256}[c.k] and L["klw"] == {64: 192, 184: 384, 256: 512}[kc]
    info = ix.schedule_info()
    assert info["query_tiles"] == (c.nq + 255) // 256 and info["bank_tiles"] == (N + 255) // 256, (c, info)
    pairs = info["query_tiles"] * info["bank_tiles"]
    if c.G:
        assert info["workgroups"] == c.G or pairs < c.G, (c, info)
    if c.G == 3:
        assert pairs >= 4 * c.G and info["segments"] >= c.G, (c, info)                    # every workgroup walks several tiles
    if c.G == 8 and N >= 5000:
        assert info["max_slots_per_qtile"] > 1, (c, info)                                  # several slots share a query tile
    if c.G == 64 and N == 5000:
        assert pairs < 64, (c, info)                                                       # more workgroups than pairs
    if getattr(c, "opt", "") == "cluster":
        assert info["cluster"] == [8, 1], (c, info)


def _no_complaints(bad, c):
    assert not bad, f"{c}: " + " | ".join(f"[{n}] {m}" for n, m in bad.items())


@pytest.mark.parametrize("c", EXACT_CASES, ids=lambda c: f"D{c.D}-N{c.N}-nq{c.nq}-k{c.k}-m{c.metric}-s{c.scale}-G{c.G}{'-' + c.opt if c.opt else ''}")
def test_exact_worlds_rows_and_score_bits(cuda_device, c):
    kc = R.kc_of(c.k)
    W = R.exact_world(c.N, c.D, c.nq, kc, 17, c.scale)
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    held = _held(cuda_device, W["bank"], c.metric)
    want = held.search(q, c.k)
    assert held.last_search_path()["path"] == "fp32"
    first = None
    for leg in ((1, 2) if c.opt == "rerank" else (0,)):
        if c.opt == "append":                       # a search on the first 15,000 rows makes the fp16 copy; the rest arrives behind it
            ix = _screened(cuda_device, W["bank"][:15000], c.metric, c.G, c.opt)
            ix.search(q, c.k)
            assert ix.last_screen()["nq"] == c.nq
            ix.add(torch.from_numpy(W["bank"][15000:]).to(cuda_device))
            with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
                ix.last_screen()
        else:
            ix = _screened(cuda_device, W["bank"], c.metric, c.G, c.opt)
        if leg:
            ix.set_rerank_copy(leg)
        got = ix.search(q, c.k)
        L = ix.last_screen()
        _regime(ix, L, c, kc, c.N)
        assert not L["centred"] and (leg == 0 or (ix.rerank_copy_bytes() > 0) == (leg == 1))
        _no_complaints(R.check_exact(L["rows"], L["scores"], W, c.metric, kc), c)
        if c.N < kc:
            assert L["certified"].all(), f"{c}: every row was a candidate, every query is certified"
        assert ix.last_fp16_escalated() == int((L["certified"] == 0).sum()) == ix.last_fp16_fallbacks(), c
        assert _same(got, want), f"{c}: the screened search differs from the fp32 kernel's answer"
        if first is None:
            first = L
        else:
            assert np.array_equal(first["rows"], L["rows"]) and np.array_equal(first["scores"].view(np.uint32), L["scores"].view(np.uint32)) \
                and np.array_equal(first["certified"], L["certified"]), f"{c}: the re-rank's row copy changed the candidates"
        ix.close()
    held.close()


@pytest.mark.parametrize("c", FLOAT_CASES, ids=lambda c: f"{c.world}-D{c.D}-N{c.N}-nq{c.nq}-k{c.k}-m{c.metric}-G{c.G}")
def test_float_worlds_accumulation_h1_h2_and_flags(cuda_device, c):
    kc = R.kc_of(c.k)
    W = R.float_world(c.world, c.N, c.D, c.nq, c.k, c.metric)
    ref = R.float_world_reference(c.world, c.N, c.D, c.nq, c.k, c.metric)
    q = torch.from_numpy(W["queries"]).to(cuda_device)
    ix, held = _screened(cuda_device, W["bank"], c.metric, c.G), _held(cuda_device, W["bank"], c.metric)
    got, want = ix.search(q, c.k), held.search(q, c.k)
    L = ix.last_screen()
    _regime(ix, L, c, kc, c.N)
    bad, fig = R.check_float(L["rows"], L["scores"], L["certified"], ref, c.k, kc, subnormal=c.world == "subnormal")
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
    assert ix.last_search_path()["path"] == "fp16_chain" and L["centred"] and info["centred"] and info["last_search_centred"] and info["rows"] == c.N, (c, info)
    assert (L["nq"], L["kc"], L["klw"]) == (c.nq, kc, R.klw_of(kc))
    # the cmax, ||mu|| and t that enter E' below are the reference's (tests/f16_centre_refs.py), computed from the read-out mu: the theorem is
    # checked under a bound this test has verified, not one it was handed
    C = ix.last_centre()
    u32 = lambda v: np.asarray(v, np.float32).view(np.uint32)
    assert (info["cmax"], info["mu_norm"], info["t"]) == (float(C["cmax"]), float(C["mu_norm"]), float(C["t"])), (c, info)
    mu2_ref, mu_norm_ref = CR.mu_scalars(C["mu"])
    cmax_ref = CR.cmax_ref(CR.differences(W["bank"], C["mu"]))
    assert u32(C["cmax"]) == u32(cmax_ref), f"{c}: cmax {C['cmax']!r}, max ||fl32(b - mu)|| rounded up is {cmax_ref!r}"
    assert u32(C["mu_norm"]) == u32(mu_norm_ref), f"{c}: ||mu|| {C['mu_norm']!r}, rounded up from the read-out mu {mu_norm_ref!r}"
    t_ref, t_tol = CR.t_ref(CR.chain_dot(W["queries"], C["mu"][:c.D]), c.nq, mu2_ref)
    assert abs(float(C["t"]) - float(t_ref)) <= t_tol, f"{c}: t {C['t']!r}, sum c_q / (nq mu.mu) = {t_ref!r} (tolerance {t_tol:.3g})"
    bad, fig = R.check_centred(L["rows"], L["scores"], L["certified"], W["queries"], W["bank"], c.metric, c.k, kc, info)
    print("F16PASS " + json.dumps(dict(c._asdict(), kc=kc, centred=True, certified_share=float(L["certified"].mean()), **fig)))
    _no_complaints(bad, c)
    assert ix.last_fp16_escalated() == int((L["certified"] == 0).sum()), c
    assert _same(got, want), f"{c}: the screened search differs from the fp32 kernel's answer"
    ix.close(); held.close()


def test_last_screen_refusals(cuda_device):
    k, kc = 30, 64
    W = R.float_world("rounding", 5000, 64, 64, k, 0)
    bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
    ix = HipFlatIndex(64, 0, 0)
    ix.add(bank)
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):      # nothing searched yet
        ix.last_screen()
    ix.set_fp16(0); ix.search(q, k)
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen()
    # escalation on: the planted queries fail their first certificate and the second pass (k' = 256) merges into the same buffers
    ix.set_fp16(1); ix.set_fp16_escalation(True); ix.search(q, k)
    assert ix.last_fp16_escalated() >= 10
    with pytest.raises(_lib.HbirdHipError, match="second fp16 pass"):
        ix.last_screen()
    ix.set_fp16_escalation(False); ix.search(q, k)
    L = ix.last_screen()
    assert (L["nq"], L["kc"]) == (64, kc) and int((L["certified"] == 0).sum()) == ix.last_fp16_escalated() >= 10
    # too small a capacity: refused before anything is written
    lib = _lib.lib()
    info = (ctypes.c_int64 * 4)()
    rows = np.full((63, kc), -7, dtype=np.int64)
    assert lib.hb_index_last_screen(ix._h, rows.ctypes.data_as(ctypes.c_void_p), None, None, 63, info) != 0 and "room for 63 queries" in _lib.last_error()
    assert (rows == -7).all()
    assert lib.hb_index_last_screen(ix._h, None, None, None, 0, info) == 0 and list(info) == [64, kc, 0, 192]       # info alone needs no room
    only = np.empty(64, dtype=np.uint8)
    assert lib.hb_index_last_screen(ix._h, None, None, only.ctypes.data_as(ctypes.c_void_p), 64, info) == 0 and np.array_equal(only, L["certified"])
    # a search with k > 128 is the fp32 kernel's
    ix.search(q, 200)
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen()
    ix.search(q, k); ix.last_screen()
    ix.reset()
    with pytest.raises(_lib.HbirdHipError, match="did not take the fp16 candidate pass"):
        ix.last_screen()
    ix.add(bank); ix.search(q, k)
    assert np.array_equal(ix.last_screen()["rows"], L["rows"])
    ix.close()
