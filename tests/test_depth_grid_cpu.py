"""Depth grids without a GPU: the C ABI of include/hbird_hip_depth_grid.h against its bindings, the documents and the build; the refusals of both
entries through ctypes (nothing is launched); the numpy restatement of tests/depth_grid_refs.py against hand-computed cases and three wrong
variants of it, each of which must fail a named check; `DepthBootstrap` on hand-made sums; the eval.py --task depth-grid parser and the
argument errors of hbird_depth_grid_evaluation."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import depth_grid_refs as G
import depth_refs as R
from hbird_mi import _lib
from hbird_mi import depth as hdepth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_depth_upsample_metrics_grid", "hb_bootstrap_weighted_sums"}
C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "float*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
           "double*": ctypes.c_void_p, "const double*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "void*": ctypes.c_void_p}


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
def test_depth_grid_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_depth_grid.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_DEPTH_GRID)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
              | set(_lib.SIGNATURES_SCREEN) | set(_lib.SIGNATURES_EXCLUDE_SCREEN) | set(_lib.SIGNATURES_BOOTSTRAP) | set(_lib.SIGNATURES_KMEANS)
              | set(_lib.SIGNATURES_LINPROBE) | set(_lib.SIGNATURES_DEPTH))
    assert not NAMES & others
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    assert "hbird_hip_depth_grid.h" not in main and not any(n in main for n in NAMES)          # the header stands on its own
    assert "hbird_hip.h" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S) and 'extern "C"' in header
    # the older depth header keeps exactly its two entries
    assert set(_declarations(open(os.path.join(ROOT, "include", "hbird_hip_depth.h")).read())) == set(_lib.SIGNATURES_DEPTH) and len(_lib.SIGNATURES_DEPTH) == 2
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_DEPTH_GRID[name]
        assert ret == "int" and res is ctypes.c_int
        assert [C_TYPES[typ] for typ, _ in params] == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_depth_upsample_metrics_grid"][1]] == ["agg", "n_cfg", "B", "S", "r", "h", "w", "gt", "min_depth", "max_depth",
                                                                         "sums_out", "pred_out_opt", "stream"]
    assert [a for _, a in decl["hb_bootstrap_weighted_sums"][1]] == ["table", "n_img", "cols", "W", "R", "out", "stream"]
    assert int(re.search(r"#define HB_DEPTH_GRID_MAX_CONFIGS (\d+)", header).group(1)) == _lib.DEPTH_GRID_MAX_CONFIGS == _lib.GRID_MAX_CONFIGS
    grid_header = open(os.path.join(ROOT, "include", "hbird_hip_grid.h")).read()
    assert int(re.search(r"#define HB_GRID_MAX_CONFIGS (\d+)", grid_header).group(1)) == _lib.DEPTH_GRID_MAX_CONFIGS
    assert header.count("DEFINITION") == 2 and "acc = acc + (double)W[r][i] * table[i][col]" in header
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_depth_grid.h" in doc and all(n in doc for n in NAMES)
    assert all(word in doc for word in ("evaluate_grid", "evaluate_leave_one_out", "DepthBootstrap", "hbird_depth_grid_evaluation"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Depth grids" in design and all(n in design for n in NAMES)
    assert "depth_grid_metrics_kernel" in design and "bootstrap_weighted_sums_kernel" in design
    assert "--task depth-grid" in open(os.path.join(ROOT, "README.md")).read()
    assert "exp_depth_grid.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_depth_grid_unit_is_built_outside_the_pinned_units_and_has_no_atomic():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hbird_depth_grid.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_depth_grid.h" in hdrs and "hbird_depth_dev.h" in hdrs
    for units in ("KNN_UNITS", "K5_UNITS", "RES_UNITS"):
        assert "hbird_depth_grid" not in re.search(rf"^{units}\s*=(.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(csrc, "hbird_depth_grid.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src, flags=re.S)
    assert set(kernels) == {"depth_grid_metrics_kernel", "bootstrap_weighted_sums_kernel"}
    assert not any(k.startswith(("knn_", "aggregate_", "rerank_")) for k in kernels)             # those prefixes are held to a committed baseline
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\batomic\w*\s*\(", code) and "unsafeAtomicAdd" not in code
    assert "#pragma clang fp contract(off)" in code and "mfma" not in code.lower()
    assert "#pragma clang fp contract(off)" in open(os.path.join(csrc, "hbird_depth_dev.h")).read()


def test_both_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused first
    good = (p, 3, 1, 2, 2, 16, 16, p, 1e-3, 10.0, p, None, None)
    def grid(**kw):
        names = ("agg", "n_cfg", "B", "S", "r", "h", "w", "gt", "lo", "hi", "sums", "pred", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, good))
    for args, word in ((grid(agg=None), "NULL"), (grid(gt=None), "NULL"), (grid(sums=None), "NULL"), (grid(n_cfg=0), "n_cfg"), (grid(n_cfg=17), "n_cfg"),
                       (grid(n_cfg=-1), "n_cfg"), (grid(B=-1), "negative"), (grid(S=0), "positive"), (grid(r=-2), "positive"), (grid(h=0), "positive"),
                       (grid(w=0), "positive"), (grid(lo=0.0), "bounds"), (grid(lo=5.0, hi=1.0), "bounds"), (grid(hi=float("inf")), "bounds"),
                       (grid(lo=float("nan")), "bounds"), (grid(S=1024, r=8), "exceeds"), (grid(S=4097, r=1), "exceeds")):
        assert L.hb_depth_upsample_metrics_grid(*args) == -1, args
        assert word in _lib.last_error() and "hb_depth_upsample_metrics_grid" in _lib.last_error(), (args, _lib.last_error())
    # the words are the single entry's
    for kw in (dict(B=-1), dict(S=0), dict(lo=0.0), dict(S=1024, r=8), dict(gt=None)):
        a = grid(**kw)
        assert L.hb_depth_upsample_metrics_grid(*a) == -1
        mine = _lib.last_error().split(": ", 1)[1]
        assert L.hb_depth_upsample_metrics(a[0], *a[2:]) == -1 and _lib.last_error().split(": ", 1)[1] == mine
    assert L.hb_depth_upsample_metrics_grid(*grid(agg=None, gt=None, sums=None, B=0)) == 0        # an empty call
    assert L.hb_depth_upsample_metrics_grid(*grid(agg=None, gt=None, sums=None, B=0, n_cfg=0)) == -1
    for args, word in (((None, 4, 3, p, 2, p, None), "NULL"), ((p, 4, 3, None, 2, p, None), "NULL"), ((p, 4, 3, p, 2, None, None), "NULL"),
                       ((p, 4, 0, p, 2, p, None), "cols"), ((p, 4, -1, p, 2, p, None), "cols"), ((p, 0, 3, p, 2, p, None), "images"),
                       ((p, _lib.BOOTSTRAP_MAX_IMAGES + 1, 3, p, 2, p, None), "images"), ((p, 4, 3, p, -1, p, None), "R must"),
                       ((p, 4, 3, p, _lib.BOOTSTRAP_MAX_REPLICATES + 1, p, None), "R must")):
        assert L.hb_bootstrap_weighted_sums(*args) == -1, args
        assert word in _lib.last_error() and "hb_bootstrap_weighted_sums" in _lib.last_error(), (args, _lib.last_error())
    assert L.hb_bootstrap_weighted_sums(None, 4, 3, None, 0, None, None) == 0                     # an empty call
    assert L.hb_bootstrap_weighted_sums(None, _lib.BOOTSTRAP_MAX_IMAGES, 1, None, 0, None, None) == 0


# ---- the restatement: by hand, and wrong variants against named checks ---------------------------------------------------------------------
def _python_chain(table, W):
    """The definition with Python floats (IEEE doubles), element by element."""
    out = np.zeros((len(W), table.shape[1]))
    for r, w in enumerate(W):
        for c in range(table.shape[1]):
            acc = 0.0
            for i in range(table.shape[0]):
                acc = acc + float(int(w[i])) * float(table[i, c])
            out[r, c] = acc
    return out


def check_images_are_added_in_ascending_order(weighted_sums):
    table, W = G.spread_table(40, 6, seed=1), G.multiplicities(40, 5, seed=2)
    return bool(np.array_equal(weighted_sums(table, W).view(np.int64), _python_chain(table, W).view(np.int64)))


def _hand_sums(n_cfg=3, n_img=6, seed=0, empty=(2,)):
    """[n_cfg, n_img, 11] from the numpy model on small worlds; the images in `empty` have no valid ground truth (n == 0)."""
    out = []
    for c in range(n_cfg):
        agg, gt = R.agg_world(n_img, 3, 1, 20, 24, seed=seed + 7 * c)
        if c:
            gt = first_gt
        else:
            for i in empty:
                gt[i] = np.nan
            first_gt = gt
        pred, has = R.predict(agg, 3, 1, 20, 24)
        out.append(R.sums(pred, has, gt)[0])
    return np.stack(out)


def check_headline_is_the_mean_over_images_that_scored(boot):
    sums = _hand_sums(n_cfg=1, n_img=3, empty=(1,))
    per = [R.finish(s) for s in sums[0]]
    assert per[1] is None and per[0] is not None and per[2] is not None
    samples, _ = boot(sums, np.array([[1, 2, 0], [1, 1, 1], [0, 3, 0]], dtype=np.int32))
    ok = samples["rmse"][0, 0] == per[0]["rmse"] and samples["d1"][0, 0] == per[0]["d1"]                     # one kept image, drawn once
    ok = ok and samples["rmse"][1, 0] == (per[0]["rmse"] + per[2]["rmse"]) / 2.0                              # two kept of three
    return bool(ok and np.isnan(samples["rmse"][2, 0]))                                                       # none kept: NaN, never 0


def check_replicates_are_paired_across_configurations(boot):
    one = _hand_sums(n_cfg=1, n_img=6)
    sums = np.concatenate([one, one, one])
    samples, pooled = boot(sums, G.multiplicities(6, 9, seed=5))
    return all(np.array_equal(s[:, 0], s[:, c], equal_nan=True) for s in list(samples.values()) + list(pooled.values()) for c in (1, 2))


def test_the_model_passes_every_named_check_and_the_order_shows_on_its_input():
    assert check_images_are_added_in_ascending_order(G.weighted_sums)
    assert check_headline_is_the_mean_over_images_that_scored(G.depth_bootstrap)
    assert check_replicates_are_paired_across_configurations(G.depth_bootstrap)
    # the condition on the input of the order check -- here and in tests/test_depth_grid_gpu.py: ascending and descending differ somewhere
    for n_img, cols, seed in ((40, 6, 1), (7, 21, 11), (300, 337, 13), (33, 256, 17)):
        table, W = G.spread_table(n_img, cols, seed), G.multiplicities(n_img, 4, seed + 1)
        mags = np.abs(table)
        assert mags.max() / mags.min() > 1e9
        assert not np.array_equal(G.weighted_sums(table, W), G.weighted_sums(table, W, variant="descending")), (n_img, cols)
    assert G.weighted_sums(np.array([[1.5], [2.0 ** 60], [-2.0 ** 60]]), np.array([[2, 1, 1]])).tolist() == [[0.0]]      # 3 is lost at 2^60 ...
    assert G.weighted_sums(np.array([[2.0 ** 60], [-2.0 ** 60], [1.5]]), np.array([[1, 1, 2]])).tolist() == [[3.0]]      # ... and kept after it
    assert np.isnan(G.weighted_sums(np.array([[np.inf], [1.0]]), np.array([[0, 1]]))[0, 0])                              # 0 * inf, as IEEE says


@pytest.mark.parametrize("variant,check", [("descending", check_images_are_added_in_ascending_order),
                                           ("divide_by_n_img", check_headline_is_the_mean_over_images_that_scored),
                                           ("per_config_draws", check_replicates_are_paired_across_configurations)])
def test_wrong_variants_fail_their_check(variant, check):
    if variant == "descending":
        assert not check(lambda t, w: G.weighted_sums(t, w, variant=variant))
    else:
        assert not check(lambda s, w: G.depth_bootstrap(s, w, variant=variant))


# ---- DepthBootstrap on hand-made sums (the device reduction replaced by the numpy chain) ------------------------------------------------------
def _bootstrap(sums, W, keys=None, seed=7):
    keys = keys or [(k, 0.02) for k in range(1, len(sums) + 1)]
    metrics = {key: hdepth.DepthMetrics(s) for key, s in zip(keys, sums)}
    table = hdepth.bootstrap_table([metrics[k] for k in keys])
    assert table.shape == (sums.shape[1], len(keys) * hdepth.BOOT_COLS) and hdepth.BOOT_COLS == G.COLS == 21
    assert np.array_equal(table.view(np.int64), G.table_of(sums).view(np.int64))
    return hdepth.finish_bootstrap(keys, metrics, G.weighted_sums(table, W), seed), metrics


def test_bootstrap_equals_the_restatement_and_one_image_gives_the_point_value():
    sums = _hand_sums()
    W = G.multiplicities(6, 50, seed=3)
    boot, metrics = _bootstrap(sums, W)
    want, want_pooled = G.depth_bootstrap(sums, W)
    for m in R.METRICS:
        assert boot.samples[m].shape == (50, 3) and np.array_equal(boot.samples[m].view(np.int64), want[m].view(np.int64))
        assert np.array_equal(boot.pooled_samples[m].view(np.int64), want_pooled[m].view(np.int64))
    assert boot.seed == 7 and boot.n_images == 6 and boot.keys == list(metrics) and all(boot.metrics[k] is metrics[k] for k in metrics)
    lo, hi = boot.interval((1, 0.02), "rmse", 0.9)
    assert np.array_equal([lo, hi], np.quantile(want["rmse"][:, 0], [0.05, 0.95])) and lo <= metrics[(1, 0.02)]["rmse"] * 1.5
    with pytest.raises(KeyError):
        boot.interval((9, 0.02))
    with pytest.raises(ValueError, match="metric"):
        boot.interval((1, 0.02), "miou")
    single, metrics = _bootstrap(sums[:, :1], np.ones((8, 1), dtype=np.int32))
    for key in single.keys:
        for m in R.METRICS:
            col = single.samples[m][:, single.keys.index(key)]
            assert (col == metrics[key][m]).all()                                               # one image: every replicate IS the point value
            assert single.pooled_samples[m][:, single.keys.index(key)] == pytest.approx(metrics[key].pooled[m], rel=1e-14)


def test_identical_configurations_do_not_differ_and_empty_images_are_not_zeros():
    one = _hand_sums(n_cfg=1, n_img=6, empty=(2, 4))
    W = G.multiplicities(6, 200, seed=9)
    W = W[(W[:, [0, 1, 3, 5]].sum(1) > 0)]                                                      # (a replicate of empty images alone has no estimate: below)
    boot, metrics = _bootstrap(np.concatenate([one, one]), W, keys=[(5, 0.02), (5, 0.1)])
    assert len(W) > 150 and (W[:, 2] + W[:, 4] > 0).any()
    for m in R.METRICS:
        assert boot.difference((5, 0.02), (5, 0.1), m) == (0.0, 0.0, 0.0, 0.0)
    assert metrics[(5, 0.02)].empty_images == [2, 4]
    kept = hdepth.bootstrap_table([metrics[(5, 0.02)]])[:, len(R.METRICS)]
    assert kept.tolist() == [1.0, 1.0, 0.0, 1.0, 0.0, 1.0]
    per = [p["rmse"] for p in metrics[(5, 0.02)].per_image if p is not None]
    col = boot.samples["rmse"][:, 0]
    assert min(per) > 0 and (col[~np.isnan(col)] >= min(per) * (1 - 1e-12)).all() and (col[~np.isnan(col)] <= max(per) * (1 + 1e-12)).all()
    only_empty = np.zeros((1, 6), dtype=np.int32); only_empty[0, 2], only_empty[0, 4] = 4, 2
    nan_boot, _ = _bootstrap(one, only_empty)
    assert all(np.isnan(nan_boot.samples[m]).all() and np.isnan(nan_boot.pooled_samples[m]).all() for m in R.METRICS)


def test_best_takes_the_smallest_error_and_the_largest_accuracy():
    sums = _hand_sums(n_cfg=1, n_img=6, empty=())
    worse = sums.copy()
    worse[0, :, 2] *= 4.0            # four times the squared error ...
    worse[0, :, 8] *= 0.5            # ... and half the d1 hits, on every image
    boot, metrics = _bootstrap(np.concatenate([worse, sums, sums]), G.multiplicities(6, 300, seed=4), keys=[(1, 0.02), (3, 0.02), (5, 0.02)])
    assert metrics[(1, 0.02)]["rmse"] == pytest.approx(2 * metrics[(3, 0.02)]["rmse"]) and metrics[(1, 0.02)]["d1"] < metrics[(3, 0.02)]["d1"]
    assert boot.best("rmse") == ((3, 0.02), [(5, 0.02)])                                        # the first of two equals; the third is tied, the first is not
    assert boot.best("d1") == ((3, 0.02), [(5, 0.02)])
    assert boot.best("abs_rel") == ((1, 0.02), [(3, 0.02), (5, 0.02)])                          # untouched: all equal, the first in key order
    d, lo, hi, share = boot.difference((1, 0.02), (3, 0.02), "rmse")
    assert d > 0 and lo > 0 and share == 1.0
    d, lo, hi, share = boot.difference((1, 0.02), (3, 0.02), "d1")
    assert d < 0 and hi < 0 and share == 0.0
    assert set(hdepth.LOWER_IS_BETTER) | {"d1", "d2", "d3"} == set(R.METRICS)


def test_finish_sums_is_finish_image_on_arrays():
    sums = _hand_sums(n_cfg=2, n_img=4, empty=(1,))
    got = hdepth.finish_sums(sums)
    for c in range(2):
        for i in range(4):
            one = hdepth.finish_image(sums[c, i])
            for m in R.METRICS:
                assert (math.isnan(got[m][c, i]) if one is None else got[m][c, i] == pytest.approx(one[m], rel=1e-14))


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------------
def test_cli_task_depth_grid_parser():
    spec = importlib.util.spec_from_file_location("hb_cli_depth_grid_cpu", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    base = ["--dataset-name", "synthetic-depth", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--task", "depth-grid"]
    a = cli.build_parser().parse_args(base + ["--grid-k", "1", "5", "--grid-beta", "0.02", "0.1", "--memory-size", "64", "--memory-sizes", "32", "64",
                                              "--leave-one-out", "--leave-one-out-images", "3", "--leave-one-out-screen", "--bootstrap", "100",
                                              "--bootstrap-seed", "5", "--bootstrap-level", "0.9", "--bootstrap-metric", "d1", "--target-grid", "2"])
    assert a.task == "depth-grid" and a.grid_k == [1, 5] and a.grid_beta == [0.02, 0.1] and a.memory_sizes == [32, 64] and a.leave_one_out
    assert a.leave_one_out_images == 3 and a.leave_one_out_screen and a.bootstrap == 100 and a.bootstrap_seed == 5 and a.bootstrap_level == 0.9
    assert a.bootstrap_metric == "d1" and a.target_grid == 2
    assert cli.build_parser().parse_args(base).bootstrap_metric == "rmse"
    assert cli.depth_grid_key((30, 0.02)) == "k=30,beta=0.02" and cli.depth_grid_key((64, 5, 0.1)) == "memory=64,k=5,beta=0.1"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--bootstrap-metric", "miou"])
    for clash in (["--frame-size", "64", "64"], ["--window-stride", "8"], ["--overclustering", "4"], ["--linear-probe"], ["--f-mem-p", "x"],
                  ["--leave-one-out-images", "3"], ["--leave-one-out-screen"], ["--memory-sizes", "10"], ["--bootstrap-seed", "3"]):
        with pytest.raises(SystemExit):
            cli.main(base + clash)


def test_hbird_depth_grid_evaluation_argument_errors():
    net = torch.nn.Identity()
    base = dict(d_model=3, patch_size=8, dataset_name="synthetic-depth", data_dir="")
    for name, value in (("frame_size", (64, 64)), ("window_stride", 8), ("return_maps", True), ("overclustering", [4]), ("linear_probe", True),
                        ("return_knn_details", True), ("f_mem_p", "x")):
        with pytest.raises(ValueError, match=f"{name} is not available for depth grids"):
            hdepth.hbird_depth_grid_evaluation(net, **base, **{name: value})
    with pytest.raises(TypeError, match="unexpected keyword"):
        hdepth.hbird_depth_grid_evaluation(net, **base, num_classes=3)
    for kw, word in ((dict(bootstrap_seed=3), "bootstrap_seed"), (dict(memory_sizes=[10]), "memory_size"), (dict(leave_one_out_images=3), "leave_one_out"),
                     (dict(leave_one_out_screen=True), "leave_one_out"), (dict(grid_k=[0]), "k=0"), (dict(grid_k=[]), "empty"),
                     (dict(grid_beta=[-0.1]), "beta"), (dict(bootstrap=0), "replicate count"), (dict(nn_method="annoy"), "nn_method"),
                     (dict(nn_params={"idx_shard": True}), "idx_shard"), (dict(nn_params={"gpu_ids": [0, 1]}), "gpu_ids")):
        with pytest.raises(ValueError, match=word):
            hdepth.hbird_depth_grid_evaluation(net, **base, **kw)
    # the single-configuration entry still refuses what it always refused
    for name, value in (("grid_k", [3]), ("grid_beta", [0.1]), ("bootstrap", 100), ("leave_one_out", True), ("memory_sizes", [10]), ("frame_size", (64, 64))):
        with pytest.raises(ValueError, match=f"{name} is not available for depth"):
            hdepth.hbird_depth_evaluation(net, **base, **{name: value})
