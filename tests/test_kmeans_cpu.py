"""k-means over the resident bank, without a GPU: the C ABI of include/hbird_hip_kmeans.h against its bindings, the documents and the build;
the numpy model of tests/kmeans_refs.py against exact means; and five wrong variants of that model, each of which must fail a named check on
the committed worlds (a model that cannot tell them apart would hold the engine to nothing)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import kmeans_refs as R
from hbird_mi import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_kmeans_assign", "hb_kmeans_accumulate", "hb_kmeans_centroids", "hb_kmeans_fit"}
C_TYPES = {"hb_index_t*": ctypes.c_void_p, "const hb_index_t*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int,
           "int64_t": ctypes.c_int64, "int32_t*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "const float*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p}
HOST_OUT = {("hb_kmeans_centroids", "n_empty_host"): ctypes.POINTER(ctypes.c_int64), ("hb_kmeans_fit", "history"): ctypes.POINTER(ctypes.c_double),
            ("hb_kmeans_fit", "iters"): ctypes.POINTER(ctypes.c_int), ("hb_kmeans_fit", "converged"): ctypes.POINTER(ctypes.c_int)}


def _declarations(header):
    out = {}
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for ret, name, args in re.findall(r"^\s*(\w+)\s+(hb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.M):
        params = []
        for a in args.split(","):
            typ, arg = a.strip().rsplit(" ", 1)
            params.append((re.sub(r"\s*\*", "*", typ.strip()), arg))
        out[name] = (ret, params)
    return out


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_kmeans_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_kmeans.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_KMEANS)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
              | set(_lib.SIGNATURES_SCREEN) | set(_lib.SIGNATURES_EXCLUDE_SCREEN) | set(_lib.SIGNATURES_BOOTSTRAP))
    assert not NAMES & others
    # included by hbird_hip.h, after hbird_hip_exclude_screen.h and inside its extern "C" block
    inc, before = '#include "hbird_hip_kmeans.h"', '#include "hbird_hip_exclude_screen.h"'
    assert main.count(inc) == 1 and main.index(before) < main.index(inc) < main.rindex("#ifdef __cplusplus")
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_KMEANS[name]
        assert ret == "int" and res is ctypes.c_int
        want = [HOST_OUT[(name, arg)] if (name, arg) in HOST_OUT else C_TYPES[typ] for typ, arg in params]      # (host outputs: typed pointers)
        assert want == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_kmeans_assign"][1]] == ["bank", "cent", "row0", "n", "chunk_rows", "assign", "dist_opt"]
    assert [a for _, a in decl["hb_kmeans_accumulate"][1]] == ["bank", "assign", "row0", "n", "K", "sums", "counts"]
    assert [a for _, a in decl["hb_kmeans_centroids"][1]] == ["sums", "counts", "K", "d", "prev", "out", "n_empty_host", "stream"]
    assert [a for _, a in decl["hb_kmeans_fit"][1]] == ["bank", "K", "init", "max_iter", "chunk_rows", "centroids", "counts", "assign_opt", "history",
                                                        "iters", "converged"]
    assert int(re.search(r"#define HB_KMEANS_MAX_K (\d+)", header).group(1)) == _lib.KMEANS_MAX_K == 2048
    assert int(re.search(r"#define HB_KMEANS_CHUNK_ROWS (\d+)", header).group(1)) == _lib.KMEANS_CHUNK_ROWS == 131072
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_kmeans.h" in doc and all(n in doc for n in NAMES)


def test_kmeans_unit_is_built_outside_the_pinned_units_and_names_its_kernels_apart():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hbird_kmeans.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_kmeans.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_kmeans" not in re.search(r"^KNN_UNITS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_kmeans" not in re.search(r"^K5_UNITS\s*=(.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(csrc, "hbird_kmeans.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src)
    assert {"kmeans_accumulate_kernel", "kmeans_counts_kernel", "kmeans_centroids_kernel", "kmeans_changed_kernel", "kmeans_inertia_partial_kernel",
            "kmeans_inertia_final_kernel"} <= set(kernels)
    assert all(k.startswith("kmeans_") for k in kernels)
    assert "rocblas" not in src.lower() and "hipblas" not in src.lower()
    # integer atomics only: no atomic of this unit names a floating-point operand
    code = re.sub(r"//.*", "", src)
    atomics = [line for line in code.splitlines() if re.search(r"\batomic\w*\s*\(", line)]
    assert atomics and not [line for line in atomics if re.search(r"\b(float|double)\b", line)]
    assert "unsafeAtomicAdd" not in code and "atomicAdd_f" not in code


def test_kmeans_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    for call in (lambda: L.hb_kmeans_assign(None, None, 0, 1, 0, None, None), lambda: L.hb_kmeans_accumulate(None, None, 0, 1, 3, None, None),
                 lambda: L.hb_kmeans_fit(None, 3, None, 1, 0, None, None, None, None, None, None)):
        assert call() != 0 and "NULL index handle" in _lib.last_error()
    assert L.hb_kmeans_centroids(None, None, 0, 4, None, None, None, None) != 0 and "[1, 2048]" in _lib.last_error()
    assert L.hb_kmeans_centroids(None, None, 2049, 4, None, None, None, None) != 0 and "2049" in _lib.last_error()
    assert L.hb_kmeans_centroids(None, None, 3, 0, None, None, None, None) != 0 and "d must be positive" in _lib.last_error()
    assert L.hb_kmeans_centroids(None, None, 3, 4, None, None, None, None) != 0 and "NULL pointer" in _lib.last_error()


# ---- the model against exact arithmetic ------------------------------------------------------------------------------------------------------
def test_quantiser_rounds_half_to_even_and_is_exact_on_the_grid():
    x = np.array([1.0, -1.0, 2.0 ** -31, -(2.0 ** -31), 3 * 2.0 ** -31, 5 * 2.0 ** -31, 2.0 ** -30, 0.0, 2.0, -2.0], dtype=np.float32)
    assert R.quantise(x).tolist() == [2 ** 30, -(2 ** 30), 0, 0, 2, 2, 1, 0, 2 ** 31, -(2 ** 31)]
    g = np.random.default_rng(1)
    v = g.standard_normal(1000).astype(np.float32)
    q = R.quantise(v)
    assert np.abs(q.astype(np.float64) / R.TWO30 - v.astype(np.float64)).max() <= 2.0 ** -31


@pytest.mark.parametrize("world", R.BLOB_WORLDS[:2] + [w[:4] for w in R.DRIFT_WORLDS[:1]], ids=str)
def test_model_centroids_are_the_means_to_2_pow_minus_31_and_one_fp32_rounding(world):
    x, model = (R.blob_world(*world)[0::3] if world in R.BLOB_WORLDS else R.drift_world(*world)[0::2])
    a, cent = model["assign"], model["centroids"]
    assert np.array_equal(model["counts"], np.bincount(a, minlength=cent.shape[0]))
    for c in range(cent.shape[0]):
        rows = x[a == c].astype(np.float64)
        for j in range(0, x.shape[1], 5):
            mean = math.fsum(rows[:, j]) / rows.shape[0]
            half_ulp = float(np.spacing(np.float32(abs(mean)))) / 2
            assert abs(float(cent[c, j]) - mean) <= 2.0 ** -31 + half_ulp, (c, j)


def test_committed_worlds_hold_their_margins_and_their_histories():
    for w in R.BLOB_WORLDS:
        x, init, init_rows, model = R.blob_world(*w)
        assert model["n_iter"] == 2 and [h["changed"] for h in model["history"]] == [w[2], 0]
        assert all(h["empty"] == 0 and h["unassigned"] == 0 for h in model["history"])
    for K, D, rows, seed, iters in R.DRIFT_WORLDS:
        x, init, model = R.drift_world(K, D, rows, seed)
        assert model["converged"] and model["n_iter"] == iters >= 5
    assert [h["changed"] for h in R.drift_world(*R.DRIFT_WORLDS[0][:4])[2]["history"]] == [600, 68, 13, 6, 3, 4, 4, 0]
    # a world that breaks the condition is refused by its generator: two centroids a hair apart
    x = np.zeros((4, 16), dtype=np.float32); x[:, 0] = 1.0
    c = np.zeros((2, 16), dtype=np.float32); c[0, 0] = 0.5; c[1, 0] = 0.5 + 2.0 ** -20
    with pytest.raises(AssertionError):
        R.assert_margins(R.fit(x, c, 3))


def test_the_big_blob_world_crosses_the_row_count_seams_and_holds_its_margins():
    n = R.BIG_ROWS
    rt_begin, rt_end, segs, seg_tiles = R.km_segments(0, n)
    assert (rt_begin, rt_end, segs, seg_tiles) == (0, 4100, 128, 33)
    full, rest = divmod(4100, 33)
    assert (full, rest) == (124, 8) and segs - full - 1 == 3            # 124 full segments, one of 8 tiles, three empty ones
    walk = R.walked_tiles(0, n)
    assert sorted(t for t, *_ in walk) == list(range(4100))             # every tile once
    assert {u for _, _, _, u, _ in walk} == {0, 1, 2, 3} and {p for *_, p in walk} == {0, 1}
    assert {s for _, s, *_ in walk} == set(range(125))
    assert R.km_segments(0, 4000) == (0, 125, 8, 16) and R.km_segments(5, 70) == (0, 3, 1, 3) and R.km_segments(65541, 10) == (2048, 2049, 1, 1)
    assert n > 2 * 65536 and n > 131072 == 131072                       # the inertia tree at j = 1 and 2; the default staging chunk splits the bank
    x, init, init_rows, model = R.big_blob_world()                      # (asserts the margins at every iteration)
    assert x.shape == (n, 16) and init.shape == (5, 16) and model["converged"] and model["n_iter"] <= 10
    assert np.flatnonzero(~np.isfinite(x).all(axis=1)).tolist() == [R.BIG_HOLE] and 65536 < R.BIG_HOLE and model["assign"][R.BIG_HOLE] == -1
    a = model["assign"]
    S, cnt = R.integer_sums(x, a, 5)
    assert np.array_equal(R.walked_sums(x, a, 5), S) and cnt.sum() == n - 1


# ---- named checks of the model, and the wrong variants that must fail them -----------------------------------------------------------------------
def check_half_even():
    q = R.quantise(np.array([2.0 ** -31, 3 * 2.0 ** -31, -3 * 2.0 ** -31], dtype=np.float32)).tolist()
    assert q == [0, 2, -2], "half_even"
    x = np.array([[3 * 2.0 ** -31], [3 * 2.0 ** -31]], dtype=np.float32)
    cent, n, empty = R.update(x, np.zeros(2, dtype=np.int32), 1, np.zeros((1, 1), dtype=np.float32))
    assert cent[0, 0] == np.float32(2.0 ** -29) and n.tolist() == [2], "half_even"


def check_ties_to_lower_id():
    x, _ = R.small_integer_world(16, 40, 1, 5)
    cent = np.stack([x[3], x[7], x[3], x[7]])                 # two pairs of exactly equal centroids
    a, best, second = R.assign(x, cent)
    assert set(a.tolist()) <= {0, 1} and a[3] == 0 and a[7] == 1, "ties_low"
    model = R.fit(x, cent, 1)                                 # (one iteration: a twin that kept its centroid may win rows later)
    assert model["counts"][2] == 0 and model["counts"][3] == 0 and model["history"][0]["empty"] == 2, "ties_low"


def check_empty_keeps_previous():
    x, init, init_rows, _ = R.blob_world(*R.BLOB_WORLDS[0])
    dup = np.concatenate([init, init[1:2]])                   # cluster 3 duplicates cluster 1: the lower id takes all
    model = R.fit(x, dup, 1)                                  # (one iteration: the twin keeps its centroid and may win rows once cluster 1 has moved)
    assert model["history"][0]["empty"] == 1 and model["counts"][3] == 0, "empty_keeps_prev"
    assert np.array_equal(model["centroids"][3].view(np.uint32), dup[3].view(np.uint32)), "empty_keeps_prev"


def check_unassigned_rows_are_left_out():
    x, init, init_rows, clean = R.blob_world(*R.BLOB_WORLDS[0])
    bad = x.copy()
    holes = [r for r in (5, 77, 300) if r not in set(init_rows.tolist())]
    bad[holes, 2] = np.nan
    model = R.fit(bad, init, 5)
    assert (model["assign"][holes] == -1).all() and model["history"][0]["unassigned"] == len(holes), "unassigned_left_out"
    assert model["counts"].sum() == x.shape[0] - len(holes) and model["history"][0]["changed"] == x.shape[0] - len(holes), "unassigned_left_out"
    assert np.isfinite(model["centroids"]).all(), "unassigned_left_out"
    keep = np.ones(x.shape[0], dtype=bool); keep[holes] = False
    assert np.array_equal(model["centroids"].view(np.uint32), R.fit(x[keep], init, 5)["centroids"].view(np.uint32)), "unassigned_left_out"


def check_changed_against_previous():
    K, D, rows, seed, iters = R.DRIFT_WORLDS[0]
    model = R.drift_world(K, D, rows, seed)[2]
    assert [h["changed"] for h in model["history"]] == [600, 68, 13, 6, 3, 4, 4, 0] and model["n_iter"] == iters, "changed_previous"


CHECKS = [check_half_even, check_ties_to_lower_id, check_empty_keeps_previous, check_unassigned_rows_are_left_out, check_changed_against_previous]


def test_the_model_passes_its_named_checks():
    for check in CHECKS:
        check()


def _truncating_quantiser(x):
    return np.trunc(np.asarray(x, dtype=np.float32).astype(np.float64) * R.TWO30).astype(np.int64)


def _ties_to_higher_id(x, cent):
    a, best, second = ORIGINAL["assign"](x, cent[::-1])
    return np.where(a >= 0, cent.shape[0] - 1 - a, -1).astype(np.int32), best, second


def _empty_cluster_zeroed(x, a, K, prev):
    cent, n, empty = ORIGINAL["update"](x, a, K, prev)
    cent = cent.copy(); cent[n == 0] = 0.0
    return cent, n, empty


def _minus_one_rows_counted(x, a, K, prev):
    a = np.where(np.asarray(a) < 0, K - 1, a)                 # what indexing a table with -1 does
    return ORIGINAL["update"](np.nan_to_num(x), a, K, prev)


def _changed_against_the_first_iteration(a, seen):
    return ORIGINAL["count_changed"](a, seen[:1])


ORIGINAL = {name: getattr(R, name) for name in ("quantise", "assign", "update", "count_changed")}
MUTANTS = [("quantise", _truncating_quantiser, check_half_even, "half_even"),
           ("assign", _ties_to_higher_id, check_ties_to_lower_id, "ties_low"),
           ("update", _empty_cluster_zeroed, check_empty_keeps_previous, "empty_keeps_prev"),
           ("update", _minus_one_rows_counted, check_unassigned_rows_are_left_out, "unassigned_left_out"),
           ("count_changed", _changed_against_the_first_iteration, check_changed_against_previous, "changed_previous")]


@pytest.mark.parametrize("target, wrong, check, name", MUTANTS, ids=[m[1].__name__.lstrip("_") for m in MUTANTS])
def test_a_wrong_variant_fails_its_named_check(monkeypatch, target, wrong, check, name):
    monkeypatch.setattr(R, target, wrong)
    with pytest.raises(AssertionError, match=name):
        check()
    monkeypatch.undo()
    check()
