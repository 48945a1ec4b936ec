"""What a served excluding search leaves behind its passes, without a GPU (references: tests/excl_screen_refs.py, further down): a host model
of the excluding chain (SR.host_chain with a group table) passes every assertion on the GPU cases' own inputs; every wrong variant fails the
assertion NAMED for it; the case list reaches -- by the reference alone, with E by the library's own constants -- every regime of the chain,
within the caps on the undecided band around the seed (10 % of a case's second-pass queries) and on the certificates' 0.1 % band (1 % of a
case's flags, none on the image world); and the C ABI of the new read-out."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import excl_screen_refs as X
import f16_pass_refs as R
import f16_second_pass_refs as SR
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REGIMES, ALL_REGIMES = X.REGIMES, X.ALL_REGIMES


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """-> (c, W, groups, qg, kwargs of SR.host_chain: pass_scores / E / cq, the float reference or None, the exact world or None)"""
    c, W, groups, n_groups, qg = X.excl_case(name)
    if c.world == "image":
        ref = X.reference("image", c.metric)
        return c, W, groups, qg, {"pass_scores": ref["s16"], "E": ref["E"]}, ref, None
    _, kw, ref, exact = SR.model_inputs(X.ECASE[name].base)
    if not c.centred:
        kw = dict(kw, E=X.bounds(W["queries"], W["bank"], c.D, c.metric)[2])
    return c, W, groups, qg, kw, ref, exact


@functools.lru_cache(maxsize=None)
def _model(name, variant="", stale=False):
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    prev = np.roll(_model(name)["floor0"], 1) if stale else None
    return SR.host_chain(W["queries"], W["bank"], c.metric, c.k, variant=variant, prev_floor=prev, groups=groups, qg=qg, **kw)


def _complaints(name, S):
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    right = _model(name)
    skip = ~(SR.query_norms(W["queries"]) <= R.F16_LIMIT)
    L0 = {"rows": right["rows0"], "scores": right["scores0"], "certified": right["certified0"]}
    bad, fig = X.check_excl_chain(S, L0, {"groups1": S["groups1"], "left": S["left"]}, None, groups, qg, W["queries"], W["bank"], c.metric, c.k, kw["E"],
                                  ref=ref, exact=exact, cq=kw.get("cq"), skip=skip)
    bad0, fig0 = _lists0(name, S["rows0"], S["scores0"])
    bad.update(bad0); fig.update(fig0)
    return bad, fig


@functools.lru_cache(maxsize=None)
def _centre_info(name):
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    if not c.centred:
        return None
    P = SR.centred_pass(W["queries"], W["bank"], c.metric)
    return {"t": float(P["t"]), "cmax": float(P["cmax"]), "mu_norm": float(P["mu_norm"])}


def _lists0(name, rows0, scores0):
    """The level-0 lists through the calls the GPU test makes on the device's (X.check_level0_lists)."""
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    return X.check_level0_lists(rows0, scores0, W["queries"], W["bank"], c.metric, c.k, exact=exact, centre_info=_centre_info(name))


def _reached(name):
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    S = _model(name)
    bad, fig = _complaints(name, S)
    assert not bad, f"{name}: " + " | ".join(bad.values())
    out = X.regimes_reached(name, S, S["left"], fig, kw.get("cq"), kw["E"])
    return out, S, fig


# ---------------------------------------------------------------- the case-list guard
@pytest.mark.parametrize("name", list(X.ECASE))
def test_the_right_model_passes_and_the_case_reaches_its_regimes(name):
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    out, S, fig = _reached(name)
    assert set(REGIMES[name]) <= out, f"{name} is there for {REGIMES[name]}, the reference reaches {sorted(out)}: {fig}"
    assert c.N <= 7000 and c.nq <= 300 and c.k + np.bincount(groups[groups >= 0]).max() > 128 >= c.k
    excl0 = fig["excluded0"]
    if c.world != "image":
        assert np.bincount(groups[groups >= 0]).max() <= X.GROUP_ROWS and (excl0[1] >= 1), (name, excl0)
    if ref is not None:
        assert fig["undecided_share"] <= 0.10, f"{name}: {fig['undecided_share']:.3f} of the second-pass queries have a row within A of the seed"
    cap = 0.0 if c.world == "image" else 0.01
    assert fig["band_share0"] <= cap and fig["band_share1"] <= cap, (name, fig["band_share0"], fig["band_share1"])


def test_the_case_list_reaches_every_regime():
    assert set(REGIMES) == set(X.ECASE)
    assert set().union(*REGIMES.values()) == ALL_REGIMES


@pytest.mark.parametrize("name,metric", [("image", 0), ("image-l2", 1)])
def test_the_chain_model_counts_the_image_world_as_the_route_model_does(name, metric):
    """(184, 31, 25): the unseeded regime (every failing query holds fewer than k allowed candidates) and the lists of 256 excluded rows."""
    S = _model(name)
    m = X.route_model(30, metric)
    assert (int(S["certified0"].sum()), int(S["certified1"].sum()), int(S["left"].size)) == m["counts"] == (184, 31, 25)
    assert np.isneginf(S["seed1"]).all() and np.array_equal(np.flatnonzero(m["level"] == 2), S["left"])


# ---------------------------------------------------------------- wrong variants
VARIANTS = [      # (variant of SR.host_chain, the case whose inputs show it, the assertion that must fail)
    ("kth_counts_excluded", "rounding100", "kth0_bits"),            # kth0 and the floor from the k-th best of ALL candidates: too high
    ("floor_counts_excluded", "rounding100-l2", "floor0_high"),     # ... the floor alone
    ("floor_without_cq", "centred-clusters-neg", "floor0_low"),
    ("groups_identity_order", "gather", "groups1"),
    ("groups_not_gathered", "rounding300", "groups1"),
    ("stale_seeds", "gather", "seed1"),
    ("not_full_when_tail_excluded", "tight-tokens", "flag1_zero"),  # a full list whose last entry is excluded read as "ran out of rows"
    ("kth_counts_excluded", "rounding100-l2", "kth1_bits"),         # the seed rule (and kth1) on the k-th of all candidates, on lists that do not fill up
    ("kth_from_pass_scores", "gather", "kth1_bits"),
    ("left_misses_one", "rounding300", "left"),
    ("left_holds_certified", "rounding100", "left"),
]


@pytest.mark.parametrize("variant,name,assertion", VARIANTS, ids=[f"{v}-{n}" for v, n, _ in VARIANTS])
def test_a_wrong_chain_fails_its_named_assertion(variant, name, assertion):
    """The seed rule itself cannot be told from its wrong form by a flag: the second list holds the first one's k allowed candidates, so
    kth1 >= kth0 > seed + E whichever k-th is compared.  What the rule compares is the k-th score that is handed out, held on bits."""
    assert assertion in SR.SEED_NAMES + SR.LEVEL1_NAMES + X.EXCL_NAMES
    S = _model(name, variant, stale=variant == "stale_seeds")
    bad, _ = _complaints(name, S)
    assert assertion in bad, f"{variant} on {name}: expected [{assertion}], got {sorted(bad)}"


@pytest.mark.parametrize("name,assertion", [("rounding100", "lists0_H2"), ("exact-l2", "lists0_rows"), ("centred-clusters-neg", "lists0_H2"),
                                            ("rounding300", "lists0_accumulation")])
def test_wrong_level0_lists_fail_their_named_assertion(name, assertion):
    """A list that lost its best row to the next one outside (H2; on an exact world: rows), and pass scores off by 2 A of the bound."""
    c, W, groups, qg, kw, ref, exact = _inputs(name)
    S = _model(name)
    rows, scores = S["rows0"].copy(), S["scores0"].copy()
    assert not _lists0(name, rows, scores)[0]
    if assertion == "lists0_accumulation":
        scores = (scores.astype(np.float64) + 2.0 * ref["A"][:, None]).astype(np.float32)
    else:
        ps = kw["pass_scores"].astype(np.float32).astype(np.float64)      # (the order host_chain's lists are in)
        for i in range(rows.shape[0]):
            nxt = np.lexsort((np.arange(ps.shape[1]), -ps[i]))[rows.shape[1]]
            rows[i] = np.concatenate([rows[i, 1:], [nxt]]); scores[i] = np.concatenate([scores[i, 1:], [np.float32(ps[i, nxt])]])
    bad, _ = _lists0(name, rows, scores)
    assert assertion in bad, (name, sorted(bad))


def test_a_wrong_answer_fails_its_named_assertion():
    c, W, groups, qg, kw, ref, exact = _inputs("image")
    ids, dist = X.chain_ranking("image", 0)
    want = X.allowed_ranking(ids, dist, groups, qg, 30, 0)
    assert not X.check_answer(*want, *want)
    own = X.allowed_ranking(ids, dist, groups, np.full(len(qg), -1, np.int32), 30, 0)       # nothing excluded: the query's own image on top
    assert "answer_ids" in X.check_answer(*own, *want)
    off = want[1].copy(); off[5, 3] = np.nextafter(off[5, 3], np.float32(0))
    assert "answer_bits" in X.check_answer(want[0], off, *want)
    assert not X.check_answer(want[0], off, *want, which=np.arange(len(qg)) != 5)


# ---------------------------------------------------------------- the C ABI
def test_the_read_out_is_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_exclude_screen.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {n: [a.strip() for a in args.split(",")] for _, n, args in re.findall(r"^\s*(\w+)\s+(hb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.M)}
    name = "hb_index_last_exclusion_seeds"
    assert decl[name] == ["hb_index_t* ix", "int32_t* groups1", "int64_t* left", "int64_t capacity_queries1", "int64_t capacity_left", "int64_t info[2]"]
    V, I64 = ctypes.c_void_p, ctypes.c_int64
    res, got = _lib.SIGNATURES_EXCLUDE_SCREEN[name]
    fn = getattr(_lib.lib(), name)
    assert res is ctypes.c_int and got == [V, V, V, I64, I64, ctypes.POINTER(I64)] and fn.argtypes == got and fn.restype is res
    main, integration, design, screen = (open(os.path.join(ROOT, *p)).read() for p in (("include", "hbird_hip.h"), ("INTEGRATION.md",), ("DESIGN.md",),
                                                                                        ("include", "hbird_hip_screen.h")))
    assert name in main and not re.search(name + r"\s*\(", main) and f"`{name}`" in integration and name in design and name in screen
    assert "ALLOWED" in screen and "unmasked" in screen and "handed to the rungs" in screen
    assert callable(HipFlatIndex.last_exclusion_seeds) and HipMultiIndex.last_exclusion_seeds is HipMultiIndex._no_exclusion
    info = (I64 * 2)(7, 7)
    L = _lib.lib()
    assert L.hb_index_last_exclusion_seeds(None, None, None, 0, 0, info) != 0 and b"NULL" in L.hb_last_error() and list(info) == [7, 7]


def test_the_read_out_is_copies_and_launches_nothing():
    src = open(os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc", "hbird_readout.hip")).read()      # (the read-outs' unit, whose shared helper synchronises)
    assert "<<<" not in src and "hb_launch" not in src and "hipMemcpyAsync" not in src and src.count("hipStreamSynchronize") == 1
    assert "HostToDevice" not in src and "hipMemset" not in src
    body = src[src.index('extern "C" int hb_index_last_exclusion_seeds('):]
    body = body[:body.index("\n}\n")]
    assert "ro.sync()" in body and body.index("ro.sync()") < body.index("ro.copy(")
    seeds = src[src.index('extern "C" int hb_index_last_screen_seeds('):]
    assert "excluding" not in seeds[:seeds.index("\n}\n")]          # the refusal is gone
