"""Excluding searches on the certified fp16 screen, without a GPU: the C ABI of include/hbird_hip_exclude_screen.h against its bindings and
INTEGRATION.md, the host model's counts on the image world (tests/excl_screen_refs.py), and the proof that the numpy restatement of the
excluding re-rank -- what tests/test_exclude_screen_gpu.py holds the kernel to -- sees the wrong kernels it is meant to catch.

The wrong kernels (excl_screen_refs.WRONG_KERNELS), each caught by a named assertion below:
    threshold_last_allowed     the certificate's pass score taken from the last ALLOWED candidate instead of the list's last entry
    excluded_counted           excluded candidates counted into the rank (the lane at rank k - 1 among all candidates decides)
    cut_from_k_minus_1         the skip rule's cut taken from list position k - 1 (the plain re-rank's) instead of the k-th allowed candidate's
    not_full_after_exclusion   the not-full rule applied to a list that exclusion shortened (its last entry excluded = "the list ran out")
"""
import ctypes
import os
import re

import numpy as np
import pytest

import excl_screen_refs as X
import f16_pass_refs as R
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_index_set_exclude_screen", "hb_index_last_exclusion_screen", "hb_index_exclude_rerank", "hb_index_last_exclusion_seeds"}
V, I64 = ctypes.c_void_p, ctypes.c_int64


# ---------------------------------------------------------------- the C ABI
def test_entries_are_declared_in_the_new_header_only_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_exclude_screen.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    inc = '#include "hbird_hip_exclude_screen.h"'
    assert inc in main and main.index(inc) > main.index('#include "hbird_hip_screen.h"')
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {n: (r, [a.strip() for a in args.split(",")]) for r, n, args in re.findall(r"^\s*(\w+)\s+(hb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.M)}
    assert set(decl) == NAMES == set(_lib.SIGNATURES_EXCLUDE_SCREEN)
    assert decl["hb_index_set_exclude_screen"] == ("int", ["hb_index_t* ix", "int on"])
    assert decl["hb_index_last_exclusion_screen"] == ("int", ["const hb_index_t* ix", "int64_t out[8]"])
    assert decl["hb_index_exclude_rerank"] == ("int", ["hb_index_t* ix", "const float* q", "int64_t nq", "const int64_t* cand_rows", "const float* pass_scores",
                                                       "int kc", "const int32_t* qgroups", "int k", "int64_t id_base", "int64_t* out_idx", "float* out_dist",
                                                       "unsigned char* out_certified", "float* out_kth", "float* out_floor"])
    want = {"hb_index_set_exclude_screen": [V, ctypes.c_int], "hb_index_last_exclusion_screen": [V, ctypes.POINTER(I64)],
            "hb_index_exclude_rerank": [V, V, I64, V, V, ctypes.c_int, V, ctypes.c_int, I64, V, V, V, V, V],
            "hb_index_last_exclusion_seeds": [V, V, V, I64, I64, ctypes.POINTER(I64)]}      # (its declaration: tests/test_exclude_seeds_cpu.py)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
              | set(_lib.SIGNATURES_SCREEN))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        res, argtypes = _lib.SIGNATURES_EXCLUDE_SCREEN[name]
        assert res is ctypes.c_int and argtypes == want[name], name
        fn = getattr(_lib.lib(), name)                  # exported
        assert fn.argtypes == argtypes and fn.restype is res
        assert name in main and not re.search(name + r"\s*\(", main), name       # hbird_hip.h names the entry and does not declare it
        assert name not in others
        assert f"`{name}`" in integration, name
        for part in ("hbird_hip_exclude.h", "hbird_hip_screen.h"):      # (hbird_hip_screen.h names the read-out of the rungs' queries, and declares none of these)
            assert not re.search(name + r"\s*\(", open(os.path.join(ROOT, "include", part)).read()), (name, part)
    mk = open(os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc", "Makefile")).read()
    assert "hbird_hip_exclude_screen.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_exclude_screen.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert callable(HipFlatIndex.set_exclusion_screen) and callable(HipFlatIndex.last_exclusion_screen) and callable(HipFlatIndex.last_exclusion_seeds)
    assert HipMultiIndex.set_exclusion_screen is HipMultiIndex._no_exclusion and HipMultiIndex.last_exclusion_screen is HipMultiIndex._no_exclusion


def test_the_kernel_keeps_its_name_rule_and_the_shared_pieces():
    """The new kernel stays outside the families whose names existing tests hold to a baseline, and ranks, certifies and writes through the
    shared tail."""
    src = open(os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc", "hbird_exclude_screen.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src)
    assert "excl_screen_rerank_kernel" in kernels
    assert not [k for k in kernels if k.startswith(("rerank_", "knn_", "aggregate_"))]
    for piece in ("hb_rerank_query_of<CENTRED>", "hb_rerank_tail<CENTRED>", "__launch_bounds__(256)"):
        assert piece in src, piece


def test_null_handles_are_refused_without_a_gpu():
    L = _lib.lib()
    out = (I64 * 8)(*[7] * 8)
    assert L.hb_index_set_exclude_screen(None, 1) != 0 and b"NULL" in L.hb_last_error()
    assert L.hb_index_last_exclusion_screen(None, out) != 0 and b"NULL" in L.hb_last_error()
    assert list(out) == [7] * 8
    assert L.hb_index_exclude_rerank(None, None, 1, None, None, 64, None, 1, 0, None, None, None, None, None) != 0 and b"NULL" in L.hb_last_error()


# ---------------------------------------------------------------- the host model on the image world
def test_the_image_world_is_the_recipe():
    rows, groups, q, qg = X.image_world()
    assert rows.shape == (6000, 64) and q.shape == (240, 64) and rows.dtype == q.dtype == np.float32
    assert np.array_equal(np.bincount(groups), [300] * 12 + [100] * 24) and (np.diff(groups) >= 0).all()
    assert np.array_equal(qg[:144], np.repeat(np.arange(36), 4))
    assert np.allclose(np.linalg.norm(rows.astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k", [8, 30, 64])
def test_model_counts_are_pinned_and_no_query_sits_at_a_threshold(k, metric):
    """184 queries certify at level 0, 31 at the second pass, 25 are left for the rungs (all 256 second-pass candidates excluded) -- at every
    k of the GPU tests and under both metrics.  No certificate decision of the model lies within 5 % of E of its threshold, let alone inside
    flag_band's 0.1 % band: a change of the recipe that empties a level, or moves a query onto a threshold, shows here."""
    m = X.route_model(k, metric)
    assert m["counts"] == (184, 31, 25), m["counts"]
    assert m["all_excluded"] == 25
    assert sum(m["counts"]) == 240 and min(m["counts"]) >= 8
    assert np.abs(m["margins"]).min() > 0.05, np.abs(m["margins"]).min()
    assert X.route_model(k, metric, escalation=False)["counts"] == (184, 0, 56)


# ---------------------------------------------------------------- the restatement catches wrong kernels
def _model_lists(metric, kc):
    """The model's candidate lists of the image world: the kc best by s16, and s16 as pass scores."""
    ref = X.reference("image", metric)
    cand = R.reference_candidates(ref["s16"], kc)
    return cand.astype(np.int64), np.take_along_axis(ref["s16"], cand, axis=1).astype(np.float32)


def _expected(metric, k, kc, variant=None):
    rows, groups, q, qg = X.image_world()
    ref = X.reference("image", metric)
    cand, sc = _model_lists(metric, kc)
    ids, dist = X.chain_ranking("image", metric)
    return X.rerank_expected(cand, sc, groups, qg, k, ids, dist, ref["s"], ref["E"], ref["qn"], 6000, metric, variant=variant)


@pytest.mark.parametrize("metric", [0, 1])
def test_restatement_catches_the_threshold_of_the_last_allowed_candidate(metric):
    """Lists whose k allowed candidates are followed by excluded rows only (excl_screen_refs.tail_excluded_lists): the last ALLOWED candidate is
    the k-th itself, and no exact score exceeds its own pass score + E -- the wrong kernel fails every query, the right one compares with
    the list's last entry, far below, and certifies."""
    rows, groups, q, qg = X.image_world()
    ref = X.reference("image", metric)
    cand, sc, qg2 = X.tail_excluded_lists(metric, 30, 64)
    ids, dist = X.chain_ranking("image", metric)
    args = (cand, sc, groups, qg2, 30, ids, dist, ref["s"], ref["E"], ref["qn"], 6000, metric)
    _, _, (one, zero, band), have, _ = X.rerank_expected(*args)
    _, _, (w_one, w_zero, _), _, _ = X.rerank_expected(*args, variant="threshold_last_allowed")
    assert have.all() and one.all() and not band.any()
    assert (one & w_zero).sum() == len(one), "threshold_last_allowed: a query pinned at 1 is not failed by the wrong kernel"
    # ... and on the pass' own lists the two thresholds differ wherever the tail is excluded
    _, _, _, have64, _ = _expected(metric, 30, 64)
    cand64, sc64 = _model_lists(metric, 64)
    ok64 = X.allowed_mask(cand64, groups, qg)
    moved = [i for i in np.flatnonzero(have64 & ~ok64[:, -1]) if sc64[i, np.flatnonzero(ok64[i])[-1]] > sc64[i, -1]]
    assert len(moved) >= 1


@pytest.mark.parametrize("metric", [0, 1])
def test_restatement_catches_excluded_candidates_counted_into_the_rank(metric):
    """With the query's own image at the top of the list, rank k - 1 among ALL candidates is an excluded one or a better allowed one than the
    k-th: the wrong kernel loses the certificate or takes the wrong k-th score."""
    _, _, (one, _, _), have, pos = _expected(metric, 30, 64)
    _, _, (w_one, w_zero, _), w_have, w_pos = _expected(metric, 30, 64, "excluded_counted")
    assert (have & ~w_have).sum() >= 1, "excluded_counted: no query loses its k-th allowed candidate"
    assert (have & w_have & (pos != w_pos)).sum() >= 1, "excluded_counted: no query's k-th score moves"
    assert (one & w_zero).sum() >= 1


@pytest.mark.parametrize("metric", [0, 1])
def test_restatement_catches_the_cut_from_list_position_k_minus_1(metric):
    """The plain re-rank's cut (position k - 1) sits ahead of the k-th allowed candidate where the query's image fills the top: it skips
    candidates of the right answer, which the comparison of ids and distance bits then misses."""
    rows, groups, q, qg = X.image_world()
    ref = X.reference("image", metric)
    k, kc = 30, 256
    cand, sc = _model_lists(metric, kc)
    idx, _, _, have, _ = _expected(metric, k, kc)
    right = X.skip_cut_positions(cand, sc, groups, qg, k, ref["E"])
    wrong = X.skip_cut_positions(cand, sc, groups, qg, k, ref["E"], "cut_from_k_minus_1")
    lost_right = lost_wrong = 0
    for i in np.flatnonzero(have):
        lost_right += np.isin(idx[i], cand[i][right[i]]).sum()
        lost_wrong += np.isin(idx[i], cand[i][wrong[i]]).sum()
    assert lost_right == 0, "the skip rule cuts a candidate of the answer"
    assert lost_wrong >= 1, "cut_from_k_minus_1: no answer row is skipped"
    assert right.sum() >= 1                   # (the rule does skip something on these lists)


@pytest.mark.parametrize("metric", [0, 1])
def test_restatement_catches_the_not_full_rule_on_a_list_that_exclusion_shortened(metric):
    """A full list whose last entry is excluded has not run out of rows: the wrong kernel reads it as "not full" and certifies (the bank has
    fewer rows than kc) or refuses on that ground; the right one compares with the last entry's pass score."""
    rows, groups, q, qg = X.image_world()
    cand, _ = _model_lists(metric, 64)
    tail_excluded = ~X.allowed_mask(cand, groups, qg)[:, -1]
    _, _, (one, zero, _), have, _ = _expected(metric, 30, 64)
    _, _, (w_one, w_zero, _), _, _ = _expected(metric, 30, 64, "not_full_after_exclusion")
    caught = tail_excluded & have & one & w_zero
    assert caught.sum() >= 1, "not_full_after_exclusion: no certified query ends in an excluded entry"
    assert np.array_equal(one[~tail_excluded], w_one[~tail_excluded])


def test_every_wrong_kernel_has_its_test():
    src = open(os.path.abspath(__file__)).read()
    for name in X.WRONG_KERNELS:
        assert src.count(f'"{name}"') >= 1, name
