"""The references of tests/f16_second_pass_refs.py on the host: a numpy model of the chain level 0 -> seeds -> gather -> level 1 -> flags
(SR.host_chain) and of the plain fp16 copy (SR.copy_model) passes every assertion on the GPU cases' own inputs, every wrong variant of either
fails the assertion NAMED for it, and the case list reaches -- by the reference alone -- the regime each case is there for, within the caps on
the undecided band around the seed (10 % of a float case's second-pass queries) and on the certificate's 0.1 % band (0.1 % of all flags)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import f16_pass_refs as R
import f16_second_pass_refs as SR
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = {c.name: c for c in SR.CASES}


_inputs = SR.model_inputs      # (shared with tests/test_exclude_seeds_cpu.py)


@functools.lru_cache(maxsize=None)
def _model(name, variant="", stale=False):
    c = CASE[name]
    W, kw, ref, exact = _inputs(name)
    prev = np.roll(_model(name)["floor0"], 1) if stale else None
    return SR.host_chain(W["queries"], W["bank"], c.metric, c.k, variant=variant, prev_floor=prev, **kw)


def _complaints(name, S):
    c = CASE[name]
    W, kw, ref, exact = _inputs(name)
    right = _model(name)
    skip = ~(SR.query_norms(W["queries"]) <= R.F16_LIMIT)
    bad, fig = SR.check_seeds(S, right["rows0"], right["certified0"], W["queries"], W["bank"], c.metric, c.k, kw["E"], kw.get("cq"))
    bad1, fig1 = SR.check_level1(S, W["queries"], W["bank"], c.metric, c.k, kw["E"], ref=ref, exact=exact, cq=kw.get("cq"), skip=skip)
    bad.update({n: m for n, m in bad1.items() if n not in bad})
    bad.update(SR.check_n2(S))
    return bad, dict(fig, **fig1)


# ---------------------------------------------------------------- the case-list guard
@pytest.mark.parametrize("name", list(CASE))
def test_the_right_model_passes_and_the_case_reaches_its_regime(name):
    c = CASE[name]
    W, kw, ref, exact = _inputs(name)
    S = _model(name)
    bad, fig = _complaints(name, S)
    assert not bad, f"{name}: " + " | ".join(bad.values())
    assert 4096 <= c.N <= 8192 and c.nq <= 300 and c.D in (64, 128, 384, 768)
    n_have = (S["rows1"] >= 0).sum(axis=1) if S["n1"] else np.zeros(0, int)
    regimes = set()
    if ((n_have < 256) & (S["certified1"] == 1)).any():
        regimes.add("not_full_certified")
    if ((n_have == 256) & (S["certified1"] == 0)).any():
        regimes.add("full_failing")
    if S["n1"] == c.nq > 256:
        regimes.add("all_level1")
    if S["n1"] == 1 and S["queries1"][0] == 41:
        regimes.add("one_failing")
    if exact is not None and S["n1"] > 0 and exact["dup"][S["rows1"][S["rows1"] >= 0]].any():
        regimes.add("exact")
    if c.centred and np.isfinite(S["floor0"]).all():
        regimes.add("centred")
        if 0 < S["n1"] < c.nq and (np.abs(kw["cq"]) > 100 * kw["E"]).all():
            regimes.add("second_pass_centred")
    if c.world == "nonfinite" and np.isin([7, 23], S["queries1"]).all() and np.isneginf(S["seed1"][np.searchsorted(S["queries1"], [7, 23])]).all():
        regimes.add("non_finite")
    if S["kc0"] == 256 and S["n1"] == 0 and S["n2"] >= 10:
        regimes.add("no_second_pass")
    if S["n1"]:
        sent = S["queries1"][(S["certified1"] == 0) & np.isin(S["queries1"], np.arange(0, 20, 2))]      # the planted groups' queries
        qn = SR.query_norms(W["queries"])[sent]
        if c.world == "gather" and (qn < 2).sum() >= 2 and (qn > 2).sum() >= 2 and np.all((SR.query_norms(W["queries"])[:20:2] > 2) == (np.arange(10) % 2 == 0)):
            regimes.add("gather")
    assert set(c.regime) <= regimes, f"{name} is there for {c.regime}, the reference reaches {sorted(regimes)} (n1 = {S['n1']}, lists {np.bincount(n_have // 64, minlength=5)}, certified1 {int(S['certified1'].sum())})"
    if ref is not None:
        assert fig["undecided_share"] <= 0.10, f"{name}: {fig['undecided_share']:.3f} of the second-pass queries have a row within A of the seed"


def test_the_band_cap_over_all_flags():
    """At most 0.1 % of the flags the float cases check -- first and second certificates -- lie inside the 0.1 % band, by the reference alone."""
    inside = total = 0
    for name, c in CASE.items():
        W, kw, ref, exact = _inputs(name)
        if exact is not None:
            continue
        S = _model(name)
        ps = kw["pass_scores"]
        cq = kw["cq"].astype(np.float64) if "cq" in kw else 0.0
        last0 = np.take_along_axis(ps, S["rows0"][:, -1:], axis=1)[:, 0].astype(np.float32).astype(np.float64)
        kth0 = SR.kth_of(SR.chain_scores(W["queries"], W["bank"], S["rows0"], c.metric), c.k).astype(np.float64)
        with np.errstate(invalid="ignore"):
            band0 = R.flag_band(kth0, last0 + cq, kw["E"], SR.query_norms(W["queries"]))[2]
        inside += int(band0.sum()); total += c.nq
        if S["n1"]:
            fig = _complaints(name, S)[1]
            inside += int(round(fig["band_share1"] * S["n1"])); total += S["n1"]
    assert inside <= 0.001 * total, f"{inside} of {total} flags lie inside the band"


# ---------------------------------------------------------------- wrong variants
VARIANTS = [      # (variant of SR.host_chain, the case whose inputs show it, the assertion that must fail)
    ("floor_half_E", "rounding100", "floor0_high"),
    ("floor_rank_k_minus_2", "rounding100", "floor0_high"),
    ("floor_without_cq", "centred-clusters", "floor0_high"),
    ("floor_without_cq", "centred-clusters-neg", "floor0_low"),
    ("seeds_identity_order", "gather", "seed1"),
    ("stale_seeds", "gather", "seed1"),
    ("not_full_rule_on_full", "rounding300", "flag1_zero"),
    ("seed_rule_without_cq", "centred-clusters-neg", "flag1_one"),
    ("kth_from_pass_scores", "rounding100-l2", "kth0_bits"),
    ("kth_from_pass_scores", "rounding300", "kth1_bits"),
]


@pytest.mark.parametrize("variant,name,assertion", VARIANTS, ids=[f"{v}-{n}" for v, n, _ in VARIANTS])
def test_a_wrong_chain_fails_its_named_assertion(variant, name, assertion):
    assert assertion in SR.SEED_NAMES + SR.LEVEL1_NAMES
    S = _model(name, variant, stale=variant == "stale_seeds")
    bad, _ = _complaints(name, S)
    assert assertion in bad, f"{variant} on {name}: expected [{assertion}], got {sorted(bad)}"


@pytest.mark.parametrize("name", ["exact", "exact-l2"])
def test_a_pool_that_drops_rows_equal_to_the_seed_loses_them(name):
    """A seed placed ON the pass score of the 100th best row of a second-pass query (exact worlds: scores are determined to the bit, and 45 % of
    the rows have twins): the right pool offers the rows AT the seed, one that compares with > does not -- [rows1]."""
    c = CASE[name]
    W, kw, ref, exact = _inputs(name)
    S0 = _model(name)
    assert S0["n1"] > 0
    ps = kw["pass_scores"][S0["queries1"][0]]
    at = np.sort(ps)[::-1][99]
    assert (ps == at).sum() >= 1
    over = {0: np.float32(at)}
    for variant, fails in (("", False), ("pool_drops_ties", True)):
        S = SR.host_chain(W["queries"], W["bank"], c.metric, c.k, variant=variant, seed_override=over, **kw)
        bad, _ = SR.check_level1(S, W["queries"], W["bank"], c.metric, c.k, kw["E"], exact=exact)
        assert ("rows1" in bad) == fails, (variant, sorted(bad))


def _copy_chunks():
    a, _ = SR.copy_world(1000, 40, seed=1, edges=SR.EDGE_VALUES)
    b, _ = SR.copy_world(200, 40, seed=2)
    return a, b


@pytest.mark.parametrize("variant,assertion", [("truncate", "tiles"), ("flush_subnormals", "tiles"), ("flag_not_sticky", "flag"), ("flag_on_inf", "flag")])
def test_a_wrong_copy_fails_its_named_assertion(variant, assertion):
    a, b = _copy_chunks()
    if variant == "flag_on_inf":      # +-inf and NaN alone raise no flag
        a = np.where(np.isfinite(a) & (np.abs(a) > R.F16_LIMIT), np.float32(1.0), a).astype(np.float32)
        assert SR.copy_flag_ref(a) == 0 and np.isinf(a).any()
    want_flag = SR.copy_flag_ref(a)                      # sticky: the second chunk has nothing beyond the range
    assert SR.copy_flag_ref(b) == 0
    C, rows = SR.copy_model([a, b], 40)
    assert not SR.check_copy(C, rows, want_flag), "the right copy must pass"
    assert C["flag"] == (0 if variant == "flag_on_inf" else 1)
    Cw, rows = SR.copy_model([a, b], 40, variant=variant)
    bad = SR.check_copy(Cw, rows, want_flag)
    assert assertion in bad and assertion in SR.COPY_NAMES, (variant, sorted(bad))
    # a reset clears flag and rows
    C2, rows2 = SR.copy_model([a, b], 40, resets=(1,))
    assert C2["flag"] == 0 and C2["rows"] == 200 and not SR.check_copy(C2, rows2, 0)


def test_the_edge_values_round_as_the_reference_says():
    x = np.array(SR.EDGE_VALUES, np.float32)
    bits = SR.f16_rne(x)
    want = {65504.0: 0x7BFF, -65504.0: 0xFBFF, 65519.0: 0x7BFF, 65520.0: 0x7C00, 1e5: 0x7C00, np.inf: 0x7C00, -np.inf: 0xFC00, -0.0: 0x8000,
            2.0 ** -24: 0x0001, 2.0 ** -25: 0x0000, 3 * 2.0 ** -25: 0x0002, 6e-8: 0x0001, 1 + 2.0 ** -11: 0x3C00, 1 + 3 * 2.0 ** -11: 0x3C02,
            -(1 + 2.0 ** -11): 0xBC00, 2.0 ** -14: 0x0400, 2.0 ** -14 - 2.0 ** -25: 0x0400}
    for v, b in zip(SR.EDGE_VALUES, bits):
        if not np.isnan(v):
            assert b == want[v], (v, hex(b))
    assert (bits[np.isnan(x)] & 0x7C00 == 0x7C00).all() and (bits[np.isnan(x)] & 0x03FF != 0).all()
    assert [SR.copy_flag_ref([v]) for v in SR.EDGE_VALUES] == [int(v in SR.EDGE_FLAGGED) for v in SR.EDGE_VALUES]


def test_the_restated_centred_bound_is_the_shipped_one():
    for D, metric, qn, bmax, qcn, cmax, mun, t in ((128, 0, 3.0, 1.0, 0.4, 0.2, 0.98, 2.9), (768, 1, 3.0, 1.0, 0.5, 0.3, 0.95, -3.1), (64, 0, 70.0, 70.0, 12.0, 9.0, 69.0, 0.5)):
        E = float(SR.bound_E_centred(qn, qcn, bmax, cmax, mun, t, D, metric))
        assert abs(E - R.replay_bounds(D, metric, qn, bmax, qcn, cmax, mun, t)[1]) <= 1e-5 * E


# ---------------------------------------------------------------- the C ABI
def test_the_read_outs_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_screen.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {n: [a.strip() for a in args.split(",")] for _, n, args in re.findall(r"^\s*(\w+)\s+(hb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.M)}
    assert decl["hb_index_last_screen_seeds"] == ["hb_index_t* ix", "float* kth0", "float* floor0", "unsigned char* certified0", "int64_t* queries1", "float* seed1",
                                                  "int64_t* cand_rows1", "float* pass_scores1", "unsigned char* certified1", "float* kth1",
                                                  "int64_t capacity_queries", "int64_t capacity_queries1", "int64_t info[8]"]
    assert decl["hb_index_last_fp16_copy"] == ["hb_index_t* ix", "uint16_t* bank16", "uint16_t* q16", "int64_t info[8]"]
    V, I64 = ctypes.c_void_p, ctypes.c_int64
    want = {"hb_index_last_screen_seeds": [V] * 10 + [I64, I64, ctypes.POINTER(I64)], "hb_index_last_fp16_copy": [V, V, V, ctypes.POINTER(I64)]}
    main, integration, design = (open(os.path.join(ROOT, *p)).read() for p in (("include", "hbird_hip.h"), ("INTEGRATION.md",), ("DESIGN.md",)))
    for name, argtypes in want.items():
        res, got = _lib.SIGNATURES_SCREEN[name]
        fn = getattr(_lib.lib(), name)
        assert res is ctypes.c_int and got == argtypes and fn.argtypes == argtypes and fn.restype is res
        assert name in main and not re.search(name + r"\s*\(", main) and f"`{name}`" in integration and name in design, name
    assert callable(HipFlatIndex.last_screen_seeds) and callable(HipFlatIndex.last_fp16_copy)
    info = (I64 * 8)(*([7] * 8))
    L = _lib.lib()
    assert L.hb_index_last_screen_seeds(None, *([None] * 9), 0, 0, info) != 0 and b"NULL" in L.hb_last_error() and list(info) == [7] * 8
    assert L.hb_index_last_fp16_copy(None, None, None, info) != 0 and b"NULL" in L.hb_last_error() and list(info) == [7] * 8


def test_the_read_outs_are_copies_and_launch_nothing():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    src = open(os.path.join(csrc, "hbird_readout.hip")).read()      # (both live in the read-outs' unit, whose shared helper synchronises)
    assert "<<<" not in src and "hb_launch" not in src and "hipMemcpyAsync" not in src and src.count("hipStreamSynchronize") == 1
    assert "HostToDevice" not in src and "hipMemset" not in src
    for start in ('extern "C" int hb_index_last_screen_seeds(', 'extern "C" int hb_index_last_fp16_copy('):
        body = src[src.index(start):]
        body = body[:body.index("\n}\n")]
        assert "ro.sync()" in body and body.index("ro.sync()") < body.index("ro.copy("), start
