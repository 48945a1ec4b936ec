"""tests/f16_pass_refs.py held to what it promises, hb_index_last_screen's C ABI against its binding and documents, and -- on the host, before
any GPU time is spent -- the proof that the assertions of tests/test_f16_candidates_gpu.py can see the errors they are meant to catch: for each
of seven wrong candidate passes, modelled on the committed inputs, the table below records WHICH assertion fails.

The wrong passes (the only code in this suite that speaks of tiles: a bank tile is 256 rows, a k16 group 16 dimensions, as csrc/hbird_knn_f16.hip
walks them):
    init_prev_tile     one bank tile's row-init values are the previous tile's (a stale parity of the row-init buffer)
    k16_dropped        one k16 group of one bank tile is left out of the sums (a fragment that never arrived)
    k16_twice          ... or added twice (a fragment of the wrong ring slot)
    kc_minus_1_later   the best kc - 1 plus a later row (k - 1 handed to the epilogue)
    reversed_ties      ties by HIGHER row
    row_lost_per_slot  the first row behind every 1,024-row boundary is never offered to a pool
    off_by_3A          every score 3 A too high (exact worlds: 3 units)
"""
import ctypes
import os
import re

import numpy as np
import pytest

import f16_pass_refs as R
import f16_screen_worlds as fw
import test_f16_candidates_gpu as G
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT = 256


# ---------------------------------------------------------------- the C ABI
def test_screen_entry_is_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_screen.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    inc = '#include "hbird_hip_screen.h"'
    assert inc in main and main.index(inc) > main.index('#include "hbird_hip_exclude.h"')
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.findall(r"^\s*(\w+)\s+(hb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.M)
    names = ["hb_index_last_screen", "hb_index_last_screen_seeds", "hb_index_last_fp16_copy"]      # (the two later read-outs: tests/test_f16_second_pass_cpu.py)
    assert [(r, n) for r, n, _ in decl] == [("int", n) for n in names] and set(_lib.SIGNATURES_SCREEN) == set(names)
    args = [a.strip() for a in decl[0][2].split(",")]
    assert args == ["hb_index_t* ix", "int64_t* cand_rows", "float* pass_scores", "unsigned char* certified", "int64_t capacity_queries", "int64_t info[4]"]
    res, argtypes = _lib.SIGNATURES_SCREEN["hb_index_last_screen"]
    assert res is ctypes.c_int and argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    assert "hb_index_last_screen" in main and not re.search(r"hb_index_last_screen\s*\(", main)      # hbird_hip.h points at the entry
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
    assert "hb_index_last_screen" not in others
    fn = _lib.lib().hb_index_last_screen
    assert fn.argtypes == argtypes and fn.restype is res
    assert "`hb_index_last_screen`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hb_index_last_screen" in open(os.path.join(ROOT, "DESIGN.md")).read()
    mk = open(os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc", "Makefile")).read()
    assert "hbird_hip_screen.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    assert callable(HipFlatIndex.last_screen)


def test_last_screen_refuses_a_null_handle_with_a_message():
    L = _lib.lib()
    info = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    assert L.hb_index_last_screen(None, None, None, None, 0, info) != 0 and b"NULL" in L.hb_last_error()
    assert list(info) == [7, 7, 7, 7]


def test_the_read_out_is_host_bookkeeping_and_no_kernel_changed():
    """The read-out adds no kernel and no launch: its code is copies; the state is set and cleared where the issue of record says -- since the
    report of a search became one type (csrc/hbird_report.h) by its transitions: the searches and the index name no state themselves."""
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    capi = open(os.path.join(csrc, "hbird_capi.hip")).read()
    unit = open(os.path.join(csrc, "hbird_readout.hip")).read()      # the read-outs' unit: no launch anywhere in it
    assert "<<<" not in unit and "hb_launch" not in unit and unit.count("hipStreamSynchronize(ix->stream)") == 1
    body = unit[unit.index('extern "C" int hb_index_last_screen('):]
    body = body[:body.index("\n}\n")]
    assert "ro.sync()" in body and body.index("ro.sync()") < body.index("ro.copy(")
    knn = open(os.path.join(csrc, "hbird_knn.hip")).read()
    report = open(os.path.join(csrc, "hbird_report.h")).read()
    assert "HB_SCREEN_" not in knn and knn.count("level0_finished(") == 1 and knn.count("sent_to_second_pass(") == 1 and knn.count("->begin(") == 1
    for transition, state in (("level0_finished", "HB_SCREEN_VALID"), ("sent_to_second_pass", "HB_SCREEN_OVERWRITTEN"), ("bank_changed", "HB_SCREEN_BANK_CHANGED")):
        t = report[report.index("void %s(" % transition):]
        assert "state = %s" % state in t[:t.index("}")], transition
    f16 = knn[knn.index("static int knn_search_f16"):knn.index("static int knn_search_f32")]
    assert "level0_finished(" in f16 and f16.index("level0_finished(") > f16.index("hb_launch_rerank")
    # every change of the bank clears it in ONE place, hb_index::bank_changed: reset, add, a capacity change, and hb_index_add_from (hbird_select.hip)
    hook = capi[capi.index("int hb_index::bank_changed("):]
    hook = hook[:hook.index("\n}\n")]
    assert "HB_SCREEN_" not in capi and capi.count("last.bank_changed()") == 1 and "last.bank_changed()" in hook
    for entry, event in (("hb_index_reset", "HB_BANK_EMPTIED"), ("hb_index_reserve", "HB_BANK_MOVED"), ("hb_index_add", "HB_BANK_APPENDED")):
        body = capi[capi.index('extern "C" int %s(' % entry):]
        assert body[:body.index("\n}\n")].count("bank_changed(%s)" % event) == 1, entry
    select = open(os.path.join(csrc, "hbird_select.hip")).read()
    body = select[select.index('extern "C" int hb_index_add_from('):]
    assert body[:body.index("\n}\n")].count("bank_changed(HB_BANK_APPENDED)") == 1 and "HB_SCREEN_NONE" not in select


# ---------------------------------------------------------------- the exact worlds
def _exact(c):
    kc = R.kc_of(c.k)
    return R.exact_world(c.N, c.D, c.nq, kc, 17, c.scale), kc


def test_exact_worlds_are_exact_in_every_summation_order():
    """Operands are fp16 numbers; sum |q_j b_j| + |init| stays below 2^24 units, so every partial sum in any order is an fp32 number; three fp32
    summation orders (fw._f32_orders) reproduce the integer reference's bits."""
    seen = set()
    for c in G.EXACT_CASES:
        W, kc = _exact(c)
        key = (c.N, c.D, c.nq, kc, c.scale, c.metric)
        if key in seen:
            continue
        seen.add(key)
        for x in (W["bank"], W["queries"]):
            assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
            assert np.abs(x).max() <= 3 * 2.0 ** c.scale
        assert np.array_equal(W["bank"], (W["bank_i"] * 2.0 ** c.scale).astype(np.float32)) and np.abs(W["bank_i"]).max() <= 3
        # in units of 4^scale / 2 (L2: the init is a half-integer): 2 sum |q_j b_j| + |b|^2 < 2^24
        worst = 2 * (np.abs(W["queries_i"]).sum(axis=1).max() * 3) + (W["bank_i"] ** 2).sum(axis=1).max()
        assert worst <= 3 * 9 * 1024 < 2 ** 24
        rows, scores, s2 = R.exact_lists(W, c.metric, kc)
        unit = 0.5 * 4.0 ** c.scale
        init32 = (-(W["bank_i"] ** 2).sum(axis=1) * unit).astype(np.float32) if c.metric == 1 else np.zeros(c.N, np.float32)
        m = min(c.N, 1100)      # (the sums are per row: the first rows of a big bank say as much as all of them)
        for i in sorted({0, c.nq - 1}):
            for name, so in fw._f32_orders(W["queries"][i], W["bank"][:m], init32[:m]).items():
                assert np.array_equal(so.astype(np.float64), s2[i, :m] * unit), (c, name)
        if c.N <= 5000:
            assert not R.check_exact(rows, scores, W, c.metric, kc)      # (the reference meets its own assertions)


def test_exact_worlds_tie_structure():
    """>= 40 % of the rows have a bit-identical twin; wherever the bank has room (N >= 2 k' + 80) query 0 has more than k' rows tied at its
    k'-th score; ties at rank k' straddle bank-tile boundaries and 1,024-row boundaries; and over the case list some query's tie group is cut
    by rank k' (some of its rows in the list, some outside)."""
    cut_somewhere = 0
    for c in G.EXACT_CASES:
        W, kc = _exact(c)
        assert W["dup"].mean() >= 0.40, c
        if c.N < kc:
            continue
        rows, scores, s2 = R.exact_lists(W, c.metric, kc)
        last = s2[np.arange(c.nq), rows[:, kc - 1]]
        tied = s2 == last[:, None]
        if c.N >= 2 * kc + 80:
            assert tied[0].sum() == kc + 40 > kc and np.array_equal(np.nonzero(tied[0])[0], W["heavy"]), c
            assert np.array_equal(rows[0], W["heavy"][:kc]), c
            assert len(set((W["heavy"] // BT).tolist())) >= min(5, c.N // BT), c
        inside = np.zeros_like(tied)
        np.put_along_axis(inside, rows, True, axis=1)
        cut = (tied & inside).any(axis=1) & (tied & ~inside).any(axis=1)
        cut_somewhere += int(cut.sum())
        if c.N >= 2049 and c.nq >= 33:
            assert cut.sum() >= 2, (c, cut.sum())
            i = int(np.nonzero(cut)[0][-1])
            t = np.nonzero(tied[i])[0]
            assert len(set((t // BT).tolist())) > 1, c
    assert cut_somewhere >= 20


# ---------------------------------------------------------------- the float worlds
def test_float_worlds_keep_the_band_cap_by_the_reference_alone():
    """At most 1 % of a case's queries inside the certificate's 0.1 % band, by s16's candidates; and the reference's own pass -- s16 rounded to
    fp32 -- meets every assertion of the GPU test."""
    for c in G.FLOAT_CASES:
        kc = R.kc_of(c.k)
        ref = R.float_world_reference(c.world, c.N, c.D, c.nq, c.k, c.metric)
        assert R.reference_band_share(ref, c.k, kc) <= 0.01, c
        assert np.allclose(ref["R"] + ref["A"] + ref["S"] + 1e-30, ref["E"], rtol=1e-5, atol=0), c      # the three shares ARE the shipped E
        rows, p = R.model_lists(ref["s16"], kc)
        kth = R.kth_best(np.take_along_axis(ref["s"], rows, 1), c.k)
        flags = (kth > p[:, kc - 1].astype(np.float64) + ref["E"]) & (ref["qn"] <= R.F16_LIMIT)
        bad, fig = R.check_float(rows, p, flags, ref, c.k, kc, subnormal=c.world == "subnormal")
        assert not bad, (c, bad)
        assert fig["acc_over_A"] < 0.01 and fig["err_over_E"] <= 1.0


def test_flag_band_pins_both_sides():
    E = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    kth = np.array([2.0, 1.0005, 0.5, 2.0, 2.0])
    qn = np.array([1.0, 1.0, 1.0, 7e4, R.F16_LIMIT])
    one, zero, band = R.flag_band(kth, np.zeros(5), E, qn)
    assert one.tolist() == [True, False, False, False, False] and zero.tolist() == [False, False, True, True, False] and band.tolist() == [False, True, False, False, True]


# ---------------------------------------------------------------- the wrong passes
def _tile_of_a_candidate(rows):
    """a bank tile >= 1 that holds candidates of several queries (the mutation must be visible)"""
    t, n = np.unique(rows[rows >= BT] // BT, return_counts=True)
    return int(t[np.argmax(n)])


def _wrong_passes(score, kc, q, bank, init, three_A):
    """score [nq, N] float64: the right pass scores.  -> {name: (rows, fp32 scores)} of the seven wrong passes."""
    nq, N = score.shape
    right_rows, _ = R.model_lists(score, kc)
    t = _tile_of_a_candidate(right_rows)
    lo, hi = t * BT, min(N, (t + 1) * BT)
    out = {}
    s = score.copy(); s[:, lo:hi] += (init[lo - BT:lo - BT + (hi - lo)] - init[lo:hi])[None, :]
    out["init_prev_tile"] = R.model_lists(s, kc)
    g = 3
    part = q[:, 16 * g:16 * g + 16].astype(np.float16).astype(np.float64) @ bank[lo:hi, 16 * g:16 * g + 16].astype(np.float16).astype(np.float64).T
    s = score.copy(); s[:, lo:hi] -= part
    out["k16_dropped"] = R.model_lists(s, kc)
    s = score.copy(); s[:, lo:hi] += part
    out["k16_twice"] = R.model_lists(s, kc)
    rows, p = R.model_lists(score, kc + 4)
    out["kc_minus_1_later"] = (np.concatenate([rows[:, :kc - 1], rows[:, kc + 3:kc + 4]], axis=1), np.concatenate([p[:, :kc - 1], p[:, kc + 3:kc + 4]], axis=1))
    sc32 = score.astype(np.float32)
    rows = np.stack([np.lexsort((-np.arange(N), -sc32[i]))[:kc] for i in range(nq)])
    out["reversed_ties"] = (rows, np.take_along_axis(sc32, rows, axis=1))
    s = score.copy(); s[:, 1024::1024] = -np.inf
    out["row_lost_per_slot"] = R.model_lists(s, kc)
    out["off_by_3A"] = R.model_lists(score + three_A, kc)
    return out


# which assertions of the GPU test fail for which wrong pass, on the committed inputs below (recorded; profiles/r17/README.md has the table)
CAUGHT_EXACT = {
    "init_prev_tile": {"rows", "score_bits", "low_ids_on_ties"},
    "k16_dropped": {"rows", "score_bits", "low_ids_on_ties"},
    "k16_twice": {"rows", "score_bits", "low_ids_on_ties"},
    "kc_minus_1_later": {"rows", "low_ids_on_ties"},
    "reversed_ties": {"rows", "sorted", "low_ids_on_ties"},
    "row_lost_per_slot": {"rows", "low_ids_on_ties"},
    "off_by_3A": {"score_bits"},
}
CAUGHT_FLOAT = {
    "init_prev_tile": {"accumulation", "H1", "H2", "clear_candidates"},
    "k16_dropped": {"accumulation", "H1", "H2", "clear_candidates"},
    "k16_twice": {"accumulation", "H1", "H2", "clear_candidates"},
    "kc_minus_1_later": {"H2"},
    "reversed_ties": {"sorted"},
    "row_lost_per_slot": {"H2", "clear_candidates"},
    "off_by_3A": {"accumulation"},
}


def test_wrong_passes_break_the_exact_assertions():
    c = G.Exact(200, 2049, 257, 128, 1, 0, 0, "")
    assert c in G.EXACT_CASES
    W, kc = _exact(c)
    _, _, s2 = R.exact_lists(W, c.metric, kc)
    unit = 0.5 * 4.0 ** c.scale
    init = -(W["bank_i"] ** 2).sum(axis=1) * unit
    seen = {}
    for name, (rows, p) in _wrong_passes(s2 * unit, kc, W["queries"], W["bank"], init, 3 * unit).items():
        seen[name] = set(R.check_exact(rows, p, W, c.metric, kc))
    assert seen == CAUGHT_EXACT, seen
    assert all(seen.values())


def test_wrong_passes_break_the_float_assertions():
    """Every wrong pass fails at least one float assertion (reversed ties: on the duplicated rows of duplicate_background, whose pass scores are
    equal in any arithmetic)."""
    c = G.Float("duplicate_background", 200, 5000, 257, 128, 0, 64)
    assert c in G.FLOAT_CASES
    kc = R.kc_of(c.k)
    W = R.float_world(c.world, c.N, c.D, c.nq, c.k, c.metric)
    ref = R.float_world_reference(c.world, c.N, c.D, c.nq, c.k, c.metric)
    # (metric 0 has no row init: the init mutation is shown on the L2 case below)
    seen = {}
    wrong = _wrong_passes(ref["s16"], kc, W["queries"], W["bank"], np.zeros(c.N), 3.0 * ref["A"][:, None])
    for name, (rows, p) in wrong.items():
        if name != "init_prev_tile":
            seen[name] = set(R.check_float(rows, p, None, ref, c.k, kc)[0])
    c1 = G.Float("near_limit", 1024, 2049, 33, 30, 1, 0)
    assert c1 in G.FLOAT_CASES
    kc1 = R.kc_of(c1.k)
    W1 = R.float_world(c1.world, c1.N, c1.D, c1.nq, c1.k, c1.metric)
    ref1 = R.float_world_reference(c1.world, c1.N, c1.D, c1.nq, c1.k, c1.metric)
    init1 = -0.5 * (W1["bank"].astype(np.float64) ** 2).sum(axis=1)
    rows, p = _wrong_passes(ref1["s16"], kc1, W1["queries"], W1["bank"], init1, 0.0)["init_prev_tile"]
    seen["init_prev_tile"] = set(R.check_float(rows, p, None, ref1, c1.k, kc1)[0])
    assert seen == CAUGHT_FLOAT, seen
    assert all(seen.values())
