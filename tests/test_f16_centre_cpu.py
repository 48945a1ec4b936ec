"""The mean-centred form of the certified fp16 screen (csrc/hbird_f16_centre.hip), restated in numpy and held to its bound on the
CPU.  `centred_model` shares no code with the library: it centres with q - t mu and b - mu in float32, rounds both to fp16, sums in float64, adds
the per-row term t g (through init16, rounded like the library's fmaf) and the per-query term c_q, and compares with the float64 score of the
fp32 values.  The bound is the shipped one, restated in float64:

    E' = ||q - t mu|| cmax (1.05 / 1024 + D' 1.2e-7)
         + D' 1.2e-7 (||q|| bmax + ||q|| ||mu|| + 2 |t| ||mu|| cmax + [L2] bmax^2)
         + (||q - t mu|| + cmax) sqrt(D) 6e-8 + 1e-30,          D' = D + 4, cmax = max ||b - mu||, bmax = max ||b||

What is asserted:
  (a) max |centred fp16 score + constants - exact| <= E' on every query and row of every world below;
  (b) no query is certified whose true top k is not inside the candidates;
  (c) every query of the two massive-activation worlds (20,000 rows, D = 128 / 768, inner product, k = 30) is certified at k' = 64 -- a condition
      on the bound's TIGHTNESS: a bound that is sound but too wide buys nothing on the banks this form exists for;
  (d) with 1.05 read as 0.75 the restated bound is caught: on rounding worlds shifted by a common vector (bank rows + v, queries + v) (a) or (b)
      fails.  v lives on four dimensions that the group leaves at exact zero, so q.v = b.v = 0 for the planted query and rows: their scores all
      move by v.v and the planted ranking survives (a v that overlaps the group moves every row by its own b.v and re-ranks the group); with
      mu = v and t = 1 the centred operands ARE the unshifted world's, whose fp16 error reaches 0.9 of 2^-10 ||q|| ||b||.  ||v|| = 2 (twice a
      row's norm) at D = 64 and 0.25 at D = 384: the fp32 terms of E' belong to the EXACT chain on the uncentred rows and grow with D ||v||^2 --
      at D = 384, ||v|| = 2 they are 0.6 of the fp16 term and no factor on it down to 0.75 could be told from 1.05; at ||v|| = 30 they are 17 x it.

Measured by the builder (worst |err| / E' over queries and rows, inner product / L2):
    massive_activation 20,000 x 128   0.196 / 0.186   certified 100 % / 100 % at k' = 64 (uncentred: 0 %), worst margin 0.90 / 0.78 E', E'/E 0.069
    massive_activation 20,000 x 768   0.049 / 0.045   certified 100 % / 100 %,                                worst margin 0.21 / 0.11 E', E'/E 0.28
    shared_mean 5,000 x 128 0.114 / 0.113 (E'/E 0.69), isotropic 5,000 x 128 0.122 / 0.122 (E'/E 1.005): certified 100 % as without centring
    shifted rounding worlds, mu = v, t = 1:  D = 64 0.833 / 0.805,  D = 384 0.822 / 0.789;  no group certified, every hidden row outside the candidates
    0.75 for 1.05: (a) fails at D = 64 (1.120 / 1.070 of the mutated bound) and at D = 384 (1.100 / 1.042); (b) fails as well at D = 64 for
    g >= 0.9 (L2: g = 0.95) and at D = 384, inner product, g = 0.95 -- all four (D, metric) cases are caught.
(The figures come from the tests' print statements; the assertions were fixed before any of them was seen.)
"""
import ctypes
import os
import re

import numpy as np
import pytest

import f16_screen_worlds as fw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAPS = (0.5, 0.7, 0.8, 0.9, 0.95)


def bound_E_centred(qn, qcn, bmax, cmax, mun, t, D, metric, c16=1.05):
    """E' of csrc/hbird_certificate.h (hb_certificate_bound_centred), restated in float64.  c16: the factor on 2^-10 (1.05 as shipped)."""
    qn, qcn = np.asarray(qn, np.float64), np.asarray(qcn, np.float64)
    du = (D + 4) * 1.2e-7
    return (qcn * cmax * (c16 / 1024.0 + du)
            + du * (qn * bmax + qn * mun + 2.0 * abs(t) * mun * cmax + (bmax * bmax if metric == 1 else 0.0))
            + (qcn + cmax) * np.sqrt(float(D)) * 6e-8 + 1e-30)


def centred_model(q, bank, k, kc, metric=0, mu=None, t=None, factors=(1.05,)):
    """The centred screen on fp16-rounded centred operands with float64 sums.  mu / t default to what the library derives: the bank's column
    mean (float64 sums, rounded to float32) and sum(q.mu) / (nq mu.mu).  Per query: err_over_E (worst row, per factor), certified[f], wrong[f],
    contained, margin[f] = (exact k-th best of the candidates - (k'-th pass score + c_q + E'_f)) / E'_f."""
    q = np.ascontiguousarray(q, np.float32); bank = np.ascontiguousarray(bank, np.float32)
    nq, D = q.shape
    N = bank.shape[0]
    q64, b64 = q.astype(np.float64), bank.astype(np.float64)
    mu32 = (b64.mean(axis=0) if mu is None else np.asarray(mu, np.float64)).astype(np.float32)
    mu64 = mu32.astype(np.float64)
    m2 = float(mu64 @ mu64)
    if t is None:
        t = float((q64 @ mu64).sum() / (nq * m2)) if m2 > 0 else 0.0
    t32 = np.float32(t); t64 = float(t32)
    bc32 = bank - mu32[None, :]                                          # fl32(b - mu)
    qc32 = (q64 - t64 * mu64[None, :]).astype(np.float32)                # fl32(q - t mu) (t mu is exact in float64)
    bc16 = bc32.astype(np.float16).astype(np.float64); qc16 = qc32.astype(np.float16).astype(np.float64)
    assert np.isfinite(bc16).all() and np.isfinite(qc16).all(), "the model assumes finite fp16 operands"
    g32 = (bc32.astype(np.float64) @ mu64).astype(np.float32)            # the per-row term, one fp32 rounding
    init64 = -0.5 * (b64 ** 2).sum(axis=1) if metric == 1 else np.zeros(N)
    init32 = init64.astype(np.float32)
    init16 = (t64 * g32.astype(np.float64) + init32.astype(np.float64)).astype(np.float32)     # fmaf(t, g, binit)
    cq32 = (q64 @ mu64).astype(np.float32)
    s = q64 @ b64.T + init64[None, :]
    p16 = qc16 @ bc16.T + init16.astype(np.float64)[None, :]             # the pass' scores (its own units: without c_q)
    full = p16 + cq32.astype(np.float64)[:, None]
    norms = dict(qn=np.sqrt((q64 ** 2).sum(axis=1)), qcn=np.sqrt((qc32.astype(np.float64) ** 2).sum(axis=1)),
                 bmax=float(np.sqrt((b64 ** 2).sum(axis=1)).max()), cmax=float(np.sqrt((bc32.astype(np.float64) ** 2).sum(axis=1)).max()),
                 mun=float(np.sqrt(m2)), t=t64)
    res = {"norms": norms, "E": {}, "err_over_E": {}, "certified": {}, "wrong": {}, "margin": {}, "contained": np.zeros(nq, bool), "cand": []}
    for f in factors:
        res["E"][f] = bound_E_centred(D=D, metric=metric, c16=f, **norms)
        res["err_over_E"][f] = np.abs(full - s).max(axis=1) / res["E"][f]
        res["certified"][f] = np.zeros(nq, bool); res["wrong"][f] = np.zeros(nq, bool); res["margin"][f] = np.zeros(nq)
    for i in range(nq):
        cand = np.argsort(-p16[i], kind="stable")[:kc]
        true = np.argsort(-s[i], kind="stable")[:k]
        res["cand"].append(cand)
        res["contained"][i] = np.isin(true, cand).all()
        kth = np.sort(s[i][cand])[::-1][k - 1]
        for f in factors:
            E = res["E"][f][i]
            res["margin"][f][i] = (kth - (p16[i][cand[kc - 1]] + float(cq32[i]) + E)) / E
            res["certified"][f][i] = res["margin"][f][i] > 0
            res["wrong"][f][i] = res["certified"][f][i] and not res["contained"][i]
    return res


def _isotropic(N, D, nq, seed):
    rng = np.random.default_rng([seed, 20])
    x = rng.standard_normal((N + nq, D), dtype=np.float32)
    x /= np.sqrt(np.einsum("ij,ij->i", x, x))[:, None]
    return {"bank": x[:N], "queries": np.float32(3.0) * x[N:]}


def _rounding(D, metric):
    return fw.rounding_world(D, 30, 64, 10, 300, GAPS, metric=metric, seed=D + metric, n_background=1024)


V_NORM = {64: 2.0, 384: 0.25}     # ||v|| of the common shift (module docstring, (d))


def shifted_rounding_worlds(D, metric):
    """One single-group rounding world per gap fraction, bank rows + v and queries + v.  v lives on four dimensions that the group leaves at
    exact zero, so q.v = b.v = 0 for the group's query and rows: every score of the group moves by v.v, the L2 row terms by v.v / 2 -- the
    planted ranking survives, and with mu = v, t = 1 the centred operands ARE the unshifted world's."""
    out = []
    for gi, gap in enumerate(GAPS):
        W = fw.rounding_world(D, 30, 64, 1, 300, (gap,), metric=metric, seed=100 * D + 10 * metric + gi, n_background=0)
        free = np.flatnonzero((W["bank"] == 0).all(axis=0) & (W["queries"] == 0).all(axis=0))
        assert free.size >= 4
        v = np.zeros(D, np.float32)
        v[free[:4]] = np.float32(V_NORM[D] / 2.0) * np.array([1, -1, 1, -1], np.float32)
        bank, q = W["bank"] + v[None, :], W["queries"] + v[None, :]
        assert np.array_equal((bank - v[None, :]), W["bank"]) and np.array_equal(q - v[None, :], W["queries"]), "the shift is not exact in fp32"
        out.append(dict(W, bank=bank, queries=q, v=v))
    return out


def _report(name, m, f=1.05):
    print(f"{name}: max err/E' {m['err_over_E'][f].max():.4f}, certified {m['certified'][f].mean():.3f}, wrong {int(m['wrong'][f].sum())}, "
          f"worst margin {m['margin'][f].min():+.3f} E', E'/E {np.median(m['E'][f] / fw.bound_E(m['norms']['qn'], m['norms']['bmax'], m['D'], m['metric'])):.3f}, "
          f"t {m['norms']['t']:.4f} ||mu|| {m['norms']['mun']:.4f} cmax {m['norms']['cmax']:.4f}")


def _run(W, metric, k=30, kc=64, **kw):
    m = centred_model(W["queries"], W["bank"], k, kc, metric, **kw)
    m["D"], m["metric"] = W["bank"].shape[1], metric
    return m


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [128, 768])
def test_massive_activation_worlds_hold_the_bound_and_certify(D, metric):
    W = fw.massive_activation_world(20000, D, 128, seed=31)
    m = _run(W, metric)
    _report(f"massive_activation 20000x{D} metric={metric}", m)
    assert m["err_over_E"][1.05].max() <= 1.0, "(a) the centred bound does not hold"
    assert not m["wrong"][1.05].any(), "(b) a query is certified although a true neighbour is no candidate"
    plain = fw.screen_model(W["queries"], W["bank"], 30, 64, metric)
    print(f"    uncentred: certified {plain['certified'][1.0].mean():.3f}")
    if metric == 0:
        assert m["certified"][1.05].all(), "(c) the centred certificate does not reach every query of the massive-activation world"
        assert not plain["certified"][1.0].any(), "the world no longer defeats the uncentred certificate"


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", ["shared_mean", "isotropic"])
def test_shared_mean_and_isotropic_rows_hold_the_bound(name, metric):
    W = fw.shared_mean_world(5000, 128, 48, seed=5) if name == "shared_mean" else _isotropic(5000, 128, 48, seed=5)
    m = _run(W, metric)
    _report(f"{name} 5000x128 metric={metric}", m)
    assert m["err_over_E"][1.05].max() <= 1.0 and not m["wrong"][1.05].any()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [64, 384])
def test_rounding_world_holds_the_bound_and_is_never_certified_wrongly(D, metric):
    """A world built to defeat the certificate: every group hides a true neighbour from the fp16 top-k'.  With the library's own mu and t (the
    mean of sparse rows with random signs: nearly zero) and with the shift taken out again (mu = v, t = 1)."""
    W = _rounding(D, metric)
    m = _run(W, metric)
    _report(f"rounding_world D={D} metric={metric}, mu = mean", m)
    assert m["err_over_E"][1.05].max() <= 1.0 and not m["wrong"][1.05].any()
    for S in shifted_rounding_worlds(D, metric):
        for label, kw in (("mu = mean", {}), ("mu = v, t = 1", {"mu": S["v"], "t": 1.0})):
            ms = _run(S, metric, **kw)
            _report(f"shifted rounding_world D={D} metric={metric} g={S['g'][0]}, {label}", ms)
            assert ms["err_over_E"][1.05].max() <= 1.0, "(a)"
            assert not ms["wrong"][1.05].any(), "(b)"
        assert not ms["contained"].any(), "the shifted world no longer hides its neighbour from the centred pass"


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [64, 384])
def test_a_bound_with_075_is_caught_on_the_shifted_rounding_world(D, metric):
    """(d): the tests above have teeth.  1.05 -> 0.75 in the restated bound, nothing else changed."""
    a_fails, b_fails = [], []
    for S in shifted_rounding_worlds(D, metric):
        m = _run(S, metric, mu=S["v"], t=1.0, factors=(1.05, 0.75))
        assert m["err_over_E"][1.05].max() <= 1.0 and not m["wrong"][1.05].any()
        a_fails.append(bool(m["err_over_E"][0.75].max() > 1.0)); b_fails.append(bool(m["wrong"][0.75].any()))
        print(f"shifted rounding_world D={D} metric={metric} g={S['g'][0]}: with 0.75 max err/E' {m['err_over_E'][0.75].max():.4f} ((a) "
              f"{'fails' if a_fails[-1] else 'holds'}), certified wrongly: {b_fails[-1]}; with 1.05: {m['err_over_E'][1.05].max():.4f}, "
              f"certificate margin {m['margin'][1.05].max():+.3f} E'")
    assert any(a_fails) or any(b_fails), "a bound with 0.75 in place of 1.05 passes (a) and (b): the shifted rounding world has lost its teeth"


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("hb_index_set_fp16_centre", "hb_index_fp16_centre_info", "hb_multi_set_fp16_centre", "hb_index_last_centre")


def test_the_four_centre_entries_are_declared_exported_and_bound():
    from hbird_mi import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hbird_hip_centre.h")).read()
    declared = set(re.findall(r"^int (hb_[a-z0-9_]+)\(", header, flags=re.M))
    assert declared == set(NEW_ENTRIES) == set(_lib.SIGNATURES_CENTRE)
    assert '#include "hbird_hip_centre.h"' in open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    c_int, c_void_p, dp, ip = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    want = {"hb_index_set_fp16_centre": (c_int, [c_void_p, c_int]), "hb_index_fp16_centre_info": (c_int, [c_void_p, dp]),
            "hb_multi_set_fp16_centre": (c_int, [c_void_p, c_int]),
            "hb_index_last_centre": (c_int, [c_void_p] * 9 + [ip])}      # the handle, eight host arrays (each may be NULL), info[8]
    for name in NEW_ENTRIES:
        fn = getattr(L, name)                       # AttributeError: not exported
        assert fn.restype is want[name][0] and list(fn.argtypes) == want[name][1], name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert not [n for n in NEW_ENTRIES if n not in doc], "entries missing from INTEGRATION.md's map"


def test_the_centre_entries_reject_null_handles_and_bad_values_without_a_gpu():
    from hbird_mi import _lib
    L = _lib.lib()
    out, info = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
    for name, args in {"hb_index_set_fp16_centre": (None, 1), "hb_index_fp16_centre_info": (None, out), "hb_multi_set_fp16_centre": (None, 1),
                       "hb_index_last_centre": (None,) + (None,) * 8 + (info,)}.items():
        assert getattr(L, name)(*args) != 0 and b"NULL" in L.hb_last_error(), name


def test_the_python_surface_has_the_switches():
    from hbird_mi.nn import search_hip
    for cls in (search_hip.HipFlatIndex, search_hip.HipMultiIndex):
        assert callable(getattr(cls, "set_fp16_centre")) and callable(getattr(cls, "fp16_centre_info"))
    assert callable(search_hip.HipFlatIndex.last_centre)
    import inspect
    src = inspect.getsource(search_hip.NearestNeighborSearchHIP.__init__)
    assert 'kwargs.pop("fp16_centre", False)' in src
