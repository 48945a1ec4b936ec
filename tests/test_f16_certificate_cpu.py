"""The worlds of tests/f16_screen_worlds.py, held to what they promise -- on the CPU, with the model of the screen (screen_model): the bound E
of the fp16 certificate holds on all of them, rounding_world comes close to it, and its groups are where a certificate that is too generous
returns a wrong neighbour.  These facts are what lets tests/test_f16_certificate_gpu.py conclude from "the fp32 bits came back" that the
kernels' certificate is sound; they are conditions on the INPUTS: if a seed or a D breaks one, the builder gets fixed, no bound moves.

Measured by the builder (max over groups of |s16 - s| / E, s16 summed in float64; n_decoys = 300, 10 groups, gap fractions below):
    D      inner product   L2        floor (0.9 x what the construction's first script reached: 0.92 / 0.86 / 0.79)
    64     0.9145          0.9116    0.83
    384    0.8507          0.8340    0.77
    768    0.7854          0.7571    0.71
(the share of E that no fp16 rounding can use grows with D: the fp32-accumulation term D 2.4e-7 is 17 % of E at D = 768; L2 adds its own term.)

Model mutation (a single pass whose certificate uses f E; groups at g = 0.5 / 0.7 / 0.8 / 0.9 / 0.95, two of each):
    f = 1.0   certifies no group at any D (every hidden neighbour is outside the candidates: all ten must fail, all ten do)
    f = 0.75  D = 64: certifies 3 groups, D = 384: 3 (L2: 2) -- every one of them with a true neighbour missing;  D = 768: none
    f = 0.65  D = 768: certifies 3 groups, all wrong
"""
import ctypes
import itertools

import numpy as np
import pytest

import f16_screen_worlds as fw
import oracle
from test_f16_centre_cpu import bound_E_centred

GAPS = (0.5, 0.7, 0.8, 0.9, 0.95)
FLOOR = {64: 0.83, 384: 0.77, 768: 0.71}
METRIC_NAME = {0: "dot_product", 1: "l2"}


def _world(D, k, kc, metric, n_decoys=300, seed=None):
    return fw.rounding_world(D, k, kc, 10, n_decoys, GAPS, metric=metric, seed=D + metric if seed is None else seed, n_background=1024)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [64, 384, 768])
def test_rounding_world_reaches_the_bound_and_never_exceeds_it(D, metric):
    W = _world(D, 30, 64, metric)
    m = fw.screen_model(W["queries"], W["bank"], 30, 64, metric, orders=True)
    print(f"rounding_world D={D} metric={metric}: max err/E {m['err_over_E'].max():.4f} (fp32 orders {m['err_over_E_f32'].max():.4f})")
    assert m["err_over_E"].max() <= 1.0 and m["err_over_E_f32"].max() <= 1.0, "the bound E does not hold"
    assert m["err_over_E"].max() >= FLOOR[D], "the construction no longer comes close to E"
    assert m["same_candidates"].all(), "an fp32 summation order changes a candidate set: the spacing is too small"
    # the placed scores are what the builder says, at least the spacing apart, and the fp32 chain arithmetic (the kernels' definition of the
    # answer) ranks the hidden rows where float64 does
    ridx, _ = oracle.knn_chain_f32(W["queries"], W["bank"], 30, METRIC_NAME[metric])
    b64, q64 = W["bank"].astype(np.float64), W["queries"].astype(np.float64)
    for i in range(W["n_groups"]):
        s = b64[W["group_ids"][i]] @ q64[i] - (0.5 * (b64[W["group_ids"][i]] ** 2).sum(axis=1) if metric else 0.0)
        lv = np.unique(s)[::-1]
        assert np.all(-np.diff(lv) >= W["min_spacing"][i]), "placed scores closer than the spacing"
        assert len(lv) == 30 + 2 + 1
        assert np.isin(W["hidden_ids"][i], m["true_topk"][i]).all() and np.isin(W["hidden_ids"][i], ridx[i]).all()
        assert np.array_equal(np.sort(ridx[i]), np.sort(m["true_topk"][i]))
        outside = np.delete(np.arange(W["bank"].shape[0]), W["group_ids"][i])
        so = b64[outside] @ q64[i] - (0.5 * (b64[outside] ** 2).sum(axis=1) if metric else 0.0)
        assert so.max() < s.min() - 2.0 * m["E"][i], "a row from outside the group reaches into its scores"


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k,kc", [(30, 64), (30, 256), (90, 184)])
@pytest.mark.parametrize("D", [64, 384, 768])
def test_rounding_world_bites(D, k, kc, metric):
    """Every group at g <= 0.95 hides a true neighbour from the fp16 top-k': a sound certificate fails all of them, one with 0.75 E (D <= 384)
    or 0.65 E (D = 768) passes some and returns a wrong answer."""
    W = _world(D, k, kc, metric)
    f_bad = 0.65 if D == 768 else 0.75
    m = fw.screen_model(W["queries"], W["bank"], k, kc, metric, factors=(1.0, f_bad))
    assert W["g"].max() <= 0.95
    for i in range(W["n_groups"]):
        assert not np.isin(W["hidden_ids"][i], m["cand"][i]).all(), f"group {i} (g = {W['g'][i]}): every hidden row is a candidate"
    assert not m["contained"].any()
    assert not m["certified"][1.0].any(), "the documented bound certifies a query whose true neighbour is no candidate"
    print(f"D={D} k={k} kc={kc} metric={metric}: {f_bad} E certifies {int(m['certified'][f_bad].sum())} of {W['n_groups']} groups, all wrong")
    assert m["wrong"][f_bad].any(), f"a certificate with {f_bad} E is not caught by this world"


def test_a_short_decoy_list_leaves_the_hidden_rows_among_the_candidates():
    """n_decoys < k': what the GPU test's escalation counts rely on (the model then predicts no failure for that case)."""
    W = _world(64, 90, 184, 0, n_decoys=100)
    m = fw.screen_model(W["queries"], W["bank"], 90, 184, 0)
    assert m["contained"].all()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", sorted(fw.VIT_WORLDS))
def test_the_bound_holds_on_the_vit_shaped_worlds(name, metric):
    W = fw.VIT_WORLDS[name](3000, 128, 48, seed=5)
    m = fw.screen_model(W["queries"], W["bank"], 30, 64, metric, orders=True)
    print(f"{name} metric={metric}: max err/E {m['err_over_E'].max():.4f} (fp32 orders {m['err_over_E_f32'].max():.4f}), certified "
          f"{m['certified'][1.0].mean():.2f}, gap/E median {np.median(m['gap_over_E']):.2f}")
    assert m["err_over_E"].max() <= 1.0 and m["err_over_E_f32"].max() <= 1.0
    assert not m["wrong"][1.0].any()


def test_world_shapes():
    W = fw.shared_mean_world(2000, 128, 8, seed=1, cosine=0.45)
    c = W["bank"].astype(np.float64) @ W["bank"].astype(np.float64).T
    assert 0.3 <= (c.sum() - np.trace(c)) / (c.size - c.shape[0]) <= 0.6
    W = fw.massive_activation_world(2000, 128, 8, seed=1)
    b = np.abs(W["bank"]); rest = np.delete(b, W["dims"], axis=1)
    assert 2 <= len(W["dims"]) <= 4 and (b[:, W["dims"]].min(axis=0) > 20 * np.sqrt((rest ** 2).mean())).all()
    assert (np.sign(W["bank"][:, W["dims"]]) == np.sign(W["bank"][0, W["dims"]])).all()
    W = fw.duplicate_background_world(4000, 64, 9, seed=1)
    _, counts = np.unique(W["bank"], axis=0, return_counts=True)
    assert sorted(counts)[-3:] == [100, 317, 1000]
    W = fw.subnormal_world(1000, 64, 8, seed=1)
    assert 6e-8 <= np.abs(W["bank"]).min() and np.abs(W["bank"]).max() <= 6e-5
    assert np.sqrt((W["queries"].astype(np.float64) ** 2).sum(axis=1)).max() < 65504
    W = fw.near_limit_world(1000, 64, 8, seed=1)
    for x in (W["bank"], W["queries"]):
        assert np.abs(x).max() == 65504.0 and np.isfinite(x.astype(np.float16)).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_subnormal_world_needs_the_subnormals(metric):
    """With fp16 subnormals kept the bound holds; an MFMA that flushed them would lose the ranking, outside E: the GPU test of this world
    can tell the two apart."""
    W = fw.subnormal_world(3000, 128, 48, seed=7)
    kept = fw.screen_model(W["queries"], W["bank"], 30, 64, metric)
    assert kept["err_over_E"].max() <= 1.0
    assert kept["contained"].all()
    flushed = fw.screen_model(W["queries"], W["bank"], 30, 64, metric, flush_subnormals=True)
    print(f"subnormal_world metric={metric}: err/E kept {kept['err_over_E'].max():.3f}, flushed {flushed['err_over_E'].max():.1f}")
    assert flushed["err_over_E"].max() > 1.0
    assert not flushed["contained"].all()


# ---- the restated bounds against the constants the kernels compile ----------------------------------------------------------------------------
NORMS = [float(np.float32(v)) for v in (2.0 ** -14, 1e-3, 1.0, 30.0, 6e4)]      # fp32 numbers: what the replay computes with


def _shipped_bounds(D, metric, qn, bmax, qcn, cmax, mun, t):
    """hb_certificate_bound_replay: (E, E') in float, by the code of csrc/hbird_certificate.h that the re-rank kernels call."""
    from hbird_mi import _lib
    a = (ctypes.c_double * 8)(D, metric, qn, bmax, qcn, cmax, mun, t)
    o = (ctypes.c_double * 2)()
    assert _lib.lib().hb_certificate_bound_replay(a, 8, o, 2) == 0
    return o[0], o[1]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [24, 33, 384, 768])
def test_restated_bounds_are_the_shipped_constants(D, metric):
    """bound_E (this folder's worlds) and bound_E_centred (test_f16_centre_cpu.py) restate E and E' in float64; the CPU proofs that "E is a bound"
    hold for the kernels only while the restatements ARE the kernels' expressions.  Norms from the smallest normal fp16 number to the end of its
    range.  Tolerance 1e-5 relative: a bound is about ten fp32 operations on positive terms, each within 6e-8.  With 0.75 for 1.05 on the
    Python side the comparison fails: it can tell a changed constant."""
    worst = worst_c = mut = mut_c = 0.0
    for qn, bmax in itertools.product(NORMS, NORMS):
        E, _ = _shipped_bounds(D, metric, qn, bmax, 0.0, 0.0, 0.0, 0.0)
        ref = float(fw.bound_E(qn, bmax, D, metric))
        worst = max(worst, abs(E - ref) / ref)
        mut = max(mut, abs(E - float(fw.bound_E(qn, bmax, D, metric, c16=0.75))) / ref)
        for qcn, cmax, mun, t in itertools.product(NORMS[::2], NORMS[::2], (0.0, NORMS[0], 1.0, NORMS[-1]), (0.0, -0.5, 3.0)):
            _, Ec = _shipped_bounds(D, metric, qn, bmax, qcn, cmax, mun, t)
            ref = float(bound_E_centred(qn, qcn, bmax, cmax, mun, t, D, metric))
            worst_c = max(worst_c, abs(Ec - ref) / ref)
            mut_c = max(mut_c, abs(Ec - float(bound_E_centred(qn, qcn, bmax, cmax, mun, t, D, metric, c16=0.75))) / ref)
    print(f"D={D} metric={metric}: worst relative difference E {worst:.2e}, E' {worst_c:.2e}; with 0.75 for 1.05: {mut:.3f}, {mut_c:.3f}")
    assert worst <= 1e-5 and worst_c <= 1e-5
    assert mut > 1e-5 and mut_c > 1e-5, "a mutated constant went unnoticed"


def test_bound_replay_rejects_bad_arguments():
    from hbird_mi import _lib
    L = _lib.lib()
    a, o = (ctypes.c_double * 8)(64, 0, 1, 1, 1, 1, 1, 1), (ctypes.c_double * 2)()
    assert L.hb_certificate_bound_replay(None, 8, o, 2) < 0 and L.hb_certificate_bound_replay(a, 7, o, 2) < 0
    assert L.hb_certificate_bound_replay(a, 8, o, 1) < 0 and L.hb_certificate_bound_replay(a, 8, None, 2) < 0
    a[0] = 0
    assert L.hb_certificate_bound_replay(a, 8, o, 2) < 0
