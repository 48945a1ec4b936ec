"""Image-level k-NN classification without a GPU: the C ABI of include/hbird_hip_vote.h against its bindings, the documents and the build; the
refusals of the two entries through ctypes (nothing is launched, no device pointer is dereferenced); the numpy restatement of
tests/vote_refs.py against hand-computed cases and five wrong variants of it, each of which must fail a named check; the host logic of
hbird_mi/classify.py (`KnnClassMetrics` from a counts table, the settings it refuses), the data modules of hbird_mi/data/classify.py
(`ClassFolderDataModule` on files written into tmp_path) and the eval.py --task knn-classify parser with its refusals."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import propagate_refs as PR
import vote_refs as R
from hbird_mi import _lib, ops
from hbird_mi import classify as hclassify
from hbird_mi.data import classify as cdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
NAMES = {"hb_knn_vote", "hb_vote_counts"}
V = ctypes.c_void_p
C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float*": V, "const float*": V, "int64_t*": V, "const int64_t*": V, "void*": V,
           "int32_t*": V, "const int32_t*": V, "const int*": ctypes.POINTER(ctypes.c_int)}
HOST_ARRAYS = {"ks": ctypes.POINTER(ctypes.c_int), "temps": ctypes.POINTER(ctypes.c_float)}


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


def _cli():
    spec = importlib.util.spec_from_file_location("hbird_cli_vote", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_vote.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_VOTE)
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    assert "hbird_hip_vote.h" not in main and not any(n in main for n in NAMES)                  # the header stands on its own
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "hbird_hip.h" not in code and "hb_index_t" not in code and 'extern "C"' in header
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_VOTE[name]
        assert ret == "int" and res is ctypes.c_int
        assert [HOST_ARRAYS.get(arg) or C_TYPES[typ] for typ, arg in params] == argtypes, (name, params)
        assert params[-1] == ("void*", "hip_stream")
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_knn_vote"][1]] == ["idx", "score", "nq", "k_list", "id_base", "labels", "n_rows", "C", "ks", "nk", "temps", "nt", "topn",
                                                       "pred", "votes_opt", "hip_stream"]
    assert [a for _, a in decl["hb_vote_counts"][1]] == ["pred", "qlabels", "nq", "n_cfg", "topn", "C", "counts_io", "class_io_opt", "n_io", "hip_stream"]
    for macro, value in (("HB_VOTE_MAX_CONFIGS", _lib.VOTE_MAX_CONFIGS), ("HB_VOTE_MAX_TOP", _lib.VOTE_MAX_TOP), ("HB_VOTE_MAX_K", _lib.VOTE_MAX_K),
                         ("HB_VOTE_MAX_CLASSES", _lib.VOTE_MAX_CLASSES)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert (_lib.VOTE_MAX_CONFIGS, _lib.VOTE_MAX_TOP, _lib.VOTE_MAX_K) == (16, 8, 2048) and _lib.VOTE_MAX_CLASSES >= 32768
    assert "NO LIMIT" in header                                                                 # the class count: a leader scan, no bins
    for words in ("THIS ENGINE'S OWN", "restated from memory", "no accuracy of this engine", "TAKES PART", "first k POSITIONS", "LOWER class id",
                  "IEEE fp32 division", "prefix", "No floating-point atomic".lower(), "ACCUMULATES"):
        assert words in header or words in header.lower(), words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_vote.h" in doc and all(n in doc for n in NAMES) and "HbirdKnnClassification" in doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k-NN classification" in design and all(n in design for n in NAMES) and "knn_vote_kernel" in design and "prefix" in design
    assert "positions" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--task knn-classify" in readme and "round 33" in readme and "restated from memory" in readme and "HB_BOOTSTRAP_MAX_IMAGES" in readme
    assert "exp_vote.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_unit_is_built_outside_the_pinned_units_and_has_no_float_atomic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hbird_vote.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_vote.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    for units in ("KNN_UNITS", "K5_UNITS", "RES_UNITS"):
        assert "hbird_vote" not in re.search(rf"^{units}\s*=(.*)$", mk, flags=re.M).group(1)
    src = re.sub(r"//.*", "", open(os.path.join(CSRC, "hbird_vote.hip")).read())
    assert set(re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src, flags=re.S)) == {"knn_vote_kernel", "vote_check_kernel", "vote_counts_kernel"}
    assert "#pragma clang fp contract(off)" in src and "unsafeAtomicAdd" not in src and "mfma" not in src.lower()
    assert "hbird_hip.h" not in src                                                              # no hb_index_t on this path
    # every atomic works on an integer: the first position, the flag, the LDS hit counters, the 64-bit counts
    calls = re.findall(r"\b(atomic\w+)\s*\(\s*([^,]+),", src)
    assert calls and {c for c, _ in calls} <= {"atomicMin", "atomicOr", "atomicAdd"}
    for _, target in calls:
        assert target.strip() in ("&s_first", "flag", "&hit[HB_VOTE_MAX_TOP]", "&hit[t]", "cell", "cell + 1", "n_io") or target.strip().startswith("counts +"), target
    assert "__shared__ int s_first" in src and "__shared__ unsigned hit[" in src and "unsigned long long* cell" in src
    assert "int32_t* __restrict__ flag" in src and "unsigned long long* __restrict__ n_io" in src


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _floats(*v):
    return (ctypes.c_float * len(v))(*v)


def test_every_entry_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = V(4096)                       # never dereferenced: every call below is refused first
    names = ("idx", "score", "nq", "k_list", "id_base", "labels", "n_rows", "C", "ks", "nk", "temps", "nt", "topn", "pred", "votes", "stream")
    good = (p, p, 10, 200, 0, p, 1000, 1000, _ints(10, 20, 100, 200), 4, _floats(0.07), 1, 5, p, None, None)

    def vote(**kw):
        assert set(kw) <= set(names)
        return tuple(kw.get(n, v) for n, v in zip(names, good))
    nan, inf = float("nan"), float("inf")
    cases = [(vote(idx=None), "NULL"), (vote(score=None), "NULL"), (vote(labels=None), "NULL"), (vote(pred=None), "NULL"),
             (vote(ks=_ints(10, 10, 100, 200)), "ascending"), (vote(ks=_ints(20, 10, 100, 200)), "ascending"), (vote(ks=_ints(0, 10, 100, 200)), "ascending"),
             (vote(ks=_ints(10, 20, 100, 201)), "exceeds k_list"), (vote(k_list=2049, ks=_ints(1, 2, 3, 4)), "limit"), (vote(k_list=0), "limit"),
             (vote(ks=_ints(*range(1, 18)), nk=17), "configurations"), (vote(temps=_floats(*([0.1] * 5)), nt=5), "configurations"), (vote(nk=0), "positive"),
             (vote(temps=_floats(0.0)), "temperature"), (vote(temps=_floats(-1.0)), "temperature"), (vote(temps=_floats(nan)), "temperature"),
             (vote(temps=_floats(inf)), "temperature"), (vote(topn=0), "topn"), (vote(topn=9), "topn"), (vote(C=0), "C must"), (vote(C=-3), "C must"),
             (vote(nq=-1), "negative"), (vote(n_rows=-1), "negative")]
    for args, word in cases:
        assert L.hb_knn_vote(*args) == -1, args
        assert word in _lib.last_error() and "hb_knn_vote" in _lib.last_error(), (args, _lib.last_error())
    assert L.hb_knn_vote(*vote(nq=0)) == 0                                                       # an empty call
    assert L.hb_knn_vote(*vote(C=_lib.VOTE_MAX_CLASSES, nq=0)) == 0                              # no limit on the class count
    good_c = (p, p, 10, 4, 5, 1000, p, None, p, None)
    for at, value, word in ((0, None, "NULL"), (1, None, "NULL"), (6, None, "NULL"), (8, None, "NULL"), (2, -1, "negative"), (3, 0, "configurations"),
                            (3, 17, "configurations"), (4, 0, "topn"), (4, 9, "topn"), (5, 0, "C must")):
        args = good_c[:at] + (value,) + good_c[at + 1:]
        assert L.hb_vote_counts(*args) == -1, args
        assert word in _lib.last_error() and "hb_vote_counts" in _lib.last_error(), (args, _lib.last_error())
    assert L.hb_vote_counts(*(good_c[:2] + (0,) + good_c[3:])) == 0


def test_wrappers_check_shapes_and_dtypes_without_a_gpu():
    idx, score, labels = torch.zeros((4, 6), dtype=torch.int64), torch.zeros((4, 6)), torch.zeros(9, dtype=torch.int32)
    for bad in (dict(idx=idx.int()), dict(score=score.double()), dict(labels=labels.long()), dict(score=score[:, :5]), dict(labels=labels[None]), dict(ks=())):
        kw = dict(idx=idx, score=score, labels=labels, ks=(1, 5))
        kw.update(bad)
        with pytest.raises(ValueError, match="knn_vote"):
            ops.knn_vote(kw["idx"], kw["score"], kw["labels"], 3, kw["ks"], (0.07,))
    pred, ql = torch.zeros((2, 4, 5), dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    counts, n, per = torch.zeros((2, 5), dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros((2, 3, 2), dtype=torch.int64)
    for bad in (dict(pred=pred.long()), dict(ql=ql[:3]), dict(ql=ql.long()), dict(counts=counts[:, :4]), dict(n=n.int()), dict(per=per[:, :2])):
        kw = dict(pred=pred, ql=ql, counts=counts, n=n, per=per)
        kw.update(bad)
        with pytest.raises(ValueError, match="vote_counts"):
            ops.vote_counts(kw["pred"], kw["ql"], 3, kw["counts"], kw["n"], kw["per"])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.knn_vote(idx, score, labels, 3, (1, 5), (0.07,))


# ---- the model against hand-computed cases -------------------------------------------------------------------------------------------------
# bank rows 0 .. 7 with classes 2 0 2 -1 1 0 1 2 (row 3 unlabelled); the one query's list, best first:
HAND_LABELS = np.array([2, 0, 2, -1, 1, 0, 1, 2], dtype=np.int32)
HAND_IDX = np.array([[3, 4, 0, 1, 9, 6, 2, -1]], dtype=np.int64)                   # row 3 unlabelled, id 9 outside the bank, a -1 tail
HAND_SCORE = np.array([[0.9, 0.8, 0.7, 0.7, 0.65, 0.6, 0.5, -np.inf]], dtype=np.float32)


def test_votes_and_ranking_by_hand():
    assert R.classes(HAND_IDX, HAND_LABELS).tolist() == [[-1, 1, 2, 0, -1, 1, 2, -1]]
    assert R.classes(HAND_IDX + 100, HAND_LABELS, id_base=100).tolist() == [[-1, 1, 2, 0, -1, 1, 2, -1]]        # (the tail, -1 + 100, lands outside too)
    T = float(np.float32(0.1))
    s = HAND_SCORE[0].astype(np.float64)
    e = np.exp((s - s[1]) / T)                                                   # mx is the logit of position 1: the first that takes part
    # k = 1: position 0 does not take part -- nothing does
    pred, v = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 1, 0.1, 3)
    assert pred.tolist() == [[-1, -1, -1]] and v.tolist() == [[0.0, 0.0, 0.0]]
    # k = 4: positions 1, 2, 3 -> classes 1, 2, 0 with e = 1, exp(-1), exp(-1): the tie of classes 2 and 0 goes to the LOWER class id
    pred, v = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 4, 0.1, 3)
    assert pred.tolist() == [[1, 0, 2]] and np.allclose(v, [[1.0, e[2], e[3]]], atol=1e-15) and v[0, 1] == v[0, 2]
    # k = 7: class 1 = e1 + e5, class 2 = e2 + e6, class 0 = e3; position 4 (id 9) is outside the bank
    pred, v = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 7, 0.1, 2)
    assert pred.tolist() == [[1, 2]] and np.allclose(v, [[e[1] + e[5], e[2] + e[6]]], atol=1e-15)
    # k beyond the list is the whole list; topn beyond the classes present leaves a -1 / 0 tail
    pred, v = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 8, 0.1, 5)
    assert pred.tolist() == [[1, 2, 0, -1, -1]] and v[0, 3:].tolist() == [0.0, 0.0]
    # the fp32 restatement agrees here, and its votes lie within the bound of the model's
    p32, v32 = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 7, 0.1, 3, dtype=np.float32)
    pred, v = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 7, 0.1, 3)
    assert v32.dtype == np.float32 and np.array_equal(p32, pred) and (np.abs(v32 - v) <= R.vote_bound(HAND_IDX, HAND_SCORE, HAND_LABELS, 7, 0.1)[0]).all()
    # grid order: cfg = ik * nt + it
    g = R.grid(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, (4, 7), (0.1, 1.0), 3)
    assert len(g) == 4 and np.array_equal(g[1][0], R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 4, 1.0, 3)[0])
    assert np.array_equal(g[2][1], R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 7, 0.1, 3)[1])


def test_counts_by_hand():
    pred = np.array([[1, 2, 0], [0, 1, -1], [2, 0, 1], [1, -1, -1], [0, 2, 1]], dtype=np.int32)
    qlabels = np.array([2, 0, 1, -1, 2])                                           # query 3 is counted nowhere
    c, per, n = R.counts(pred, qlabels, 3)
    assert n == 4 and c.tolist() == [1, 3, 4] and per.tolist() == [[1, 1], [1, 0], [2, 0]]
    top1, topn, mpc = R.metrics(c, per, n)
    assert (top1, topn) == (0.25, 1.0) and abs(mpc - (1.0 + 0.0 + 0.0) / 3) < 1e-15
    m = hclassify.KnnClassMetrics([(4, 0.1)], c[None], per[None], n, skipped=1)
    assert (m.top1[(4, 0.1)], m.topn[(4, 0.1)], m.n, m.skipped, m.n_top) == (0.25, 1.0, 4, 1, 3) and abs(m.mean_per_class[(4, 0.1)] - mpc) < 1e-15


def test_the_bound_is_aggregate_bound_with_unit_labels():
    bank, labels, q, _ = R.gaussian_world(1)
    idx, score = R.lists(q[:40], bank, 70)
    ones = np.ones((1, bank.shape[0], 1))
    for k in (1, 5, 70):
        for T in (0.07, 1.0):
            want = PR.aggregate_bound(idx[:, :k], score[:, :k], ones, T)
            assert np.array_equal(R.vote_bound(idx, score, labels, k, T), want)


# ---- five wrong variants, each against a named check ---------------------------------------------------------------------------------------
def check_ties_to_the_lower_class(variant):
    pred, _ = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 4, 0.1, 3, variant=variant)
    assert pred.tolist() == [[1, 0, 2]]


def check_weights_follow_the_scores(variant):
    # two far neighbours of class 1 against one near neighbour of class 0: at T = 0.07 the near one wins
    idx, score = np.array([[1, 4, 6]], dtype=np.int64), np.array([[0.9, 0.6, 0.6]], dtype=np.float32)
    pred, _ = R.predict(idx, score, HAND_LABELS, 3, 3, 0.07, 1, variant=variant)
    assert pred.tolist() == [[0]]


def check_k_counts_list_positions(variant):
    # k = 2 looks at positions 0 and 1 whatever takes part: class 1 alone
    pred, _ = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 2, 0.1, 3, variant=variant)
    assert pred.tolist() == [[1, -1, -1]]


def check_an_unlabelled_row_does_not_vote(variant):
    pred, _ = R.predict(HAND_IDX, HAND_SCORE, HAND_LABELS, 3, 1, 0.1, 3, variant=variant)
    assert pred.tolist() == [[-1, -1, -1]]


def check_the_temperature_divides(variant):
    # a small T sharpens: at T = 0.01 one neighbour at 0.9 outvotes five at 0.8
    idx, score = np.array([[1, 4, 6, 4, 6, 4]], dtype=np.int64), np.array([[0.9, 0.8, 0.8, 0.8, 0.8, 0.8]], dtype=np.float32)
    pred, _ = R.predict(idx, score, HAND_LABELS, 3, 6, 0.01, 1, variant=variant)
    assert pred.tolist() == [[0]]


CHECKS = {"tie_high_class": check_ties_to_the_lower_class, "uniform_weights": check_weights_follow_the_scores,
          "k_counts_labelled": check_k_counts_list_positions, "unlabelled_is_class0": check_an_unlabelled_row_does_not_vote,
          "temperature_multiplies": check_the_temperature_divides}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_each_wrong_variant_fails_its_check(variant):
    assert set(CHECKS) == set(R.VARIANTS)
    for check in CHECKS.values():
        check(None)                                              # the definitions pass every check
    with pytest.raises(AssertionError):
        CHECKS[variant](variant)


def test_worlds_are_what_the_gpu_tests_assume():
    for seed in (1, 2, 3):
        bank, labels, q, qlabels = R.gaussian_world(seed)
        again = R.gaussian_world(seed)
        assert bank.shape == (600, 32) and q.shape == (203, 32) and labels.dtype == qlabels.dtype == np.int32 and set(labels) == set(range(10))
        assert all(np.array_equal(a, b) for a, b in zip((bank, labels, q, qlabels), again))
        assert np.allclose(np.linalg.norm(bank, axis=1), 1, atol=1e-6)
    idx, score, labels = R.counting_world(7, 37, 70, 3, id_base=1000)
    live = idx >= 0
    assert (score[live] == np.repeat(score[:, :1], 70, axis=1)[live]).all() and np.isneginf(score[~live]).all()      # one score per query
    assert (labels < 0).any() and (R.classes(idx, labels, 1000)[3] == -1).all() and (idx[5] == -1).all()


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------
def test_metrics_from_a_counts_table():
    configs = [(10, 0.07), (10, 1.0), (20, 0.07), (20, 1.0)]
    counts = np.array([[6, 8, 9], [7, 8, 10], [7, 9, 9], [5, 9, 10]])
    per = np.zeros((4, 4, 2), dtype=np.int64)                                      # class 3 has no queries
    per[:, :3, 0] = [5, 3, 2]
    per[0, :3, 1], per[1, :3, 1], per[2, :3, 1], per[3, :3, 1] = [4, 1, 1], [5, 2, 0], [3, 2, 2], [2, 2, 1]
    m = hclassify.KnnClassMetrics(configs, counts, per, n=10, skipped=2)
    assert m.top1 == {(10, 0.07): 0.6, (10, 1.0): 0.7, (20, 0.07): 0.7, (20, 1.0): 0.5}
    assert m.topn[(20, 1.0)] == 1.0 and m.topn[(10, 0.07)] == 0.9 and (m.n, m.skipped, m.n_top) == (10, 2, 3)
    assert abs(m.mean_per_class[(10, 0.07)] - (4 / 5 + 1 / 3 + 1 / 2) / 3) < 1e-15 and abs(m.mean_per_class[(20, 0.07)] - (3 / 5 + 2 / 3 + 1) / 3) < 1e-15
    assert m.best() == ((10, 1.0), 0.7)                                            # the first of the two best in grid order
    for i, key in enumerate(configs):
        want = R.metrics(counts[i], per[i], 10)
        assert (m.top1[key], m.topn[key]) == want[:2] and abs(m.mean_per_class[key] - want[2]) < 1e-15
    empty = hclassify.KnnClassMetrics(configs, np.zeros((4, 3)), np.zeros((4, 4, 2)), n=0, skipped=5)
    assert np.isnan(empty.top1[(10, 0.07)]) and np.isnan(empty.mean_per_class[(10, 0.07)]) and empty.skipped == 5
    with pytest.raises(ValueError):
        empty.best()
    with pytest.raises(ValueError):
        hclassify.KnnClassMetrics(configs, counts[:3], per, 10)
    with pytest.raises(ValueError):
        hclassify.KnnClassMetrics(configs, counts, per[:, :, :1], 10)


def test_classifier_refuses_bad_settings_without_a_gpu():
    fn = lambda x: x.flatten(1)                                                    # noqa: E731
    for kw in (dict(n_neighbours=0), dict(n_neighbours=(5, 2049)), dict(n_neighbours=()), dict(temperatures=0.0), dict(temperatures=(0.07, float("nan"))),
               dict(topn=0), dict(topn=9), dict(nn_params={"distance_measure": "l2"}), dict(nn_params={"distance_measure": "euclidean"}),
               dict(nn_params={"idx_shard": True}), dict(nn_params={"gpu_ids": [0, 1]}), dict(device="cpu"), dict(pool="cls"), dict(pool="mean")):
        with pytest.raises(ValueError):
            hclassify.HbirdKnnClassification(fn, 10, **kw)
    with pytest.raises(ValueError, match="cosine"):
        hclassify.HbirdKnnClassification(fn, 10, nn_params={"distance_measure": "l2"})
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            hclassify.HbirdKnnClassification(fn, bad)
    with pytest.raises(ValueError):
        hclassify.HbirdKnnClassification(3, 10)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            hclassify.HbirdKnnClassification(fn, 10)


def test_synthetic_classify_world():
    w = cdata.SyntheticClassifyDataModule(batch_size=16, n_train=40, n_val=20, seed=3)
    again = cdata.SyntheticClassifyDataModule(batch_size=16, n_train=40, n_val=20, seed=3)
    other = cdata.SyntheticClassifyDataModule(batch_size=16, n_train=40, n_val=20, seed=4)
    tr = list(w.train_dataloader())
    assert [x.shape[0] for x, _ in tr] == [16, 16, 8] and w.get_train_dataset_size() == 40 and w.get_num_classes() == 12
    for (x, y), (x2, y2), (x3, _) in zip(tr, again.train_dataloader(), other.train_dataloader()):
        assert x.shape[1:] == (3, 32, 32) and x.dtype == torch.float32 and y.dtype == torch.int64 and 0 <= int(y.min()) and int(y.max()) < 12
        assert torch.equal(x, x2) and torch.equal(y, y2) and not torch.equal(x, x3)
    # colour and frequency determine the class: without noise the mean colour tells classes 0 .. 5 apart, the row spectrum class c from c + 6
    clean = cdata.SyntheticClassifyDataModule(batch_size=64, n_train=64, n_val=1, noise=0.0, seed=1)
    x, y = next(iter(clean.train_dataloader()))
    assert (x.mean(dim=(2, 3)).round().argmax(1)[y < 3] == y[y < 3]).all()
    rows = x.mean(dim=(1, 3)) - x.mean(dim=(1, 2, 3))[:, None]
    period = torch.fft.rfft(rows, dim=1).abs().argmax(1)
    assert (period == 1 + y // 6).all()
    noisy = cdata.SyntheticClassifyDataModule(batch_size=64, n_train=64, n_val=1, noise=2.0, seed=1)
    assert float((next(iter(noisy.train_dataloader()))[0] - x).std()) > 1.5
    assert isinstance(cdata.get_classify_dataset("synthetic-classify", input_size=32), cdata.SyntheticClassifyDataModule)
    assert cdata.get_classify_dataset("synthetic-classify*0.5", input_size=32).get_train_dataset_size() == 96
    with pytest.raises(ValueError):
        cdata.get_classify_dataset("imagenet")
    with pytest.raises(ValueError):
        cdata.SyntheticClassifyDataModule(noise=-1.0)
    with pytest.raises(ValueError):
        cdata.SyntheticClassifyDataModule(num_classes=500)


def test_class_folder_on_written_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    layout = {"train": {"zebra": 3, "ant": 2, "bee": 1}, "val": {"ant": 1, "bee": 2, "zebra": 1}}
    for split, classes in layout.items():
        for name, n in classes.items():
            os.makedirs(tmp_path / split / name)
            for i in range(n):
                if name == "bee":
                    np.save(tmp_path / split / name / f"{i}.npy", rng.random((3, 20, 20)).astype(np.float32))
                else:
                    Image.fromarray(rng.integers(0, 256, (24, 30, 3), dtype=np.uint8)).save(tmp_path / split / name / f"{i}.{'png' if i % 2 else 'jpg'}")
    (tmp_path / "train" / "ant" / "notes.txt").write_text("not an image")
    dm = cdata.get_classify_dataset("class-folder", str(tmp_path), batch_size=4, num_workers=0, input_size=16)
    assert dm.classes == ["ant", "bee", "zebra"] and dm.get_num_classes() == 3 and dm.get_train_dataset_size() == 6
    assert [c for _, c in dm.train.samples] == [0, 0, 1, 2, 2, 2] and [c for _, c in dm.val.samples] == [0, 1, 1, 2]
    batches = list(dm.train_dataloader())
    assert [tuple(x.shape) for x, _ in batches] == [(4, 3, 16, 16), (2, 3, 16, 16)] and torch.cat([y for _, y in batches]).tolist() == [0, 0, 1, 2, 2, 2]
    assert batches[0][0].dtype == torch.float32 and batches[0][1].dtype == torch.int64
    os.makedirs(tmp_path / "val" / "wasp")
    np.save(tmp_path / "val" / "wasp" / "0.npy", np.zeros((3, 16, 16), dtype=np.float32))
    with pytest.raises(RuntimeError, match="'wasp' is present in val only"):
        cdata.ClassFolderDataModule(str(tmp_path), 4, 0, 16)
    os.makedirs(tmp_path / "train" / "wasp")
    with pytest.raises(RuntimeError, match="no train images|not found"):
        cdata.ClassFolderDataModule(str(tmp_path / "train"), 4, 0, 16)
    np.save(tmp_path / "train" / "wasp" / "0.npy", np.zeros((16, 16, 3), dtype=np.float32))
    dm = cdata.ClassFolderDataModule(str(tmp_path), 4, 0, 16)
    assert dm.classes == ["ant", "bee", "wasp", "zebra"] and dm.train.samples[3] == ("train/wasp/0.npy", 2)
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        dm.train[3]


def test_cli_knn_classify_parser_and_refusals(capsys):
    cli = _cli()
    base = ["--dataset-name", "synthetic-classify", "--data-dir", "", "--d-model", "3", "--patch-size", "8"]
    a = cli.build_parser().parse_args(base + ["--task", "knn-classify"])
    assert (a.task, a.grid_k, a.grid_temperature, a.top_n, a.leave_one_out) == ("knn-classify", None, None, None, False)      # 10 20 100 200 / 0.07 / 5 in main_knn_classify
    a = cli.build_parser().parse_args(base + ["--task", "knn-classify", "--grid-k", "1", "5", "--grid-temperature", "0.07", "1", "--top-n", "3", "--leave-one-out"])
    assert (a.grid_k, a.grid_temperature, a.top_n, a.leave_one_out) == ([1, 5], [0.07, 1.0], 3, True)
    assert cli.classify_key(20, 0.07) == "k=20,T=0.07" and cli.classify_key(1, 1) == "k=1,T=1.0"
    for bad in (["--grid-temperature", "0"], ["--grid-temperature", "-1"], ["--top-n", "0"], ["--grid-k", "0"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + ["--task", "knn-classify"] + bad)
    for bad, word in ((["--memory-sizes", "100"], "--memory-sizes is not available"), (["--grid-beta", "0.02"], "--grid-beta"), (["--bootstrap", "100"], "--bootstrap"),
                      (["--memory-size", "100"], "--memory-size"), (["--linear-probe"], "--linear-probe"), (["--nn-method", "faiss"], "--nn-method"),
                      (["--target-grid", "2"], "--target-grid"), (["--frame-size", "64", "64"], "--frame-size"), (["--n-neighbours", "30"], "--n-neighbours"),
                      (["--video-radius", "3"], "needs --task video"), (["--top-n", "9"], "--top-n"), (["--leave-one-out-images", "5"], "--leave-one-out-images"),
                      (["--overclustering", "10"], "--overclustering"), (["--train-fs", "x.txt"], "--train-fs")):
        with pytest.raises(SystemExit):
            cli.main(base + ["--task", "knn-classify"] + bad)
        assert word in capsys.readouterr().err, word
    for task in ([], ["--task", "depth"], ["--task", "video"]):
        for opt in (["--grid-temperature", "0.5"], ["--top-n", "3"]):
            with pytest.raises(SystemExit):
                cli.main(base + task + opt)
            assert "needs --task knn-classify" in capsys.readouterr().err
