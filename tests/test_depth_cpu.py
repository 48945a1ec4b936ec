"""Depth estimation by retrieval without a GPU: the C ABI of include/hbird_hip_depth.h against its bindings, the documents and the build; the numpy
model of tests/depth_refs.py against hand-computed tiny cases; five wrong variants of that model, each of which must fail a named check on the
committed worlds; the host logic -- metric finishing, DepthFolderDataModule on files, argument errors, the eval.py --task depth parser."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import depth_refs as R
from hbird_mi import _lib, ops
from hbird_mi import depth as hdepth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_patch_depth_targets", "hb_depth_upsample_metrics"}
C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "float*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
           "double*": ctypes.c_void_p, "int*": ctypes.c_void_p, "void*": ctypes.c_void_p}
F32 = np.float32


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
def test_depth_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_depth.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_DEPTH)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
              | set(_lib.SIGNATURES_SCREEN) | set(_lib.SIGNATURES_EXCLUDE_SCREEN) | set(_lib.SIGNATURES_BOOTSTRAP) | set(_lib.SIGNATURES_KMEANS)
              | set(_lib.SIGNATURES_LINPROBE))
    assert not NAMES & others
    inc, before = '#include "hbird_hip_depth.h"', '#include "hbird_hip_linprobe.h"'
    assert main.count(inc) == 1 and main.index(before) < main.index(inc) < main.rindex("#ifdef __cplusplus")
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_DEPTH[name]
        assert ret == "int" and res is ctypes.c_int
        assert [C_TYPES[typ] for typ, _ in params] == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_patch_depth_targets"][1]] == ["y", "B", "H", "W", "ps", "r", "min_depth", "max_depth", "rows_out", "nonempty_out",
                                                                 "hip_stream"]
    assert [a for _, a in decl["hb_depth_upsample_metrics"][1]] == ["agg", "B", "S", "r", "h", "w", "gt", "min_depth", "max_depth", "sums_out",
                                                                    "pred_out_opt", "hip_stream"]
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define HB_DEPTH_SUM_(\w+) (\d+)", header)}
    names = [k.lower() for k, _ in sorted(slots.items(), key=lambda kv: kv[1])]
    assert ["n_nopred" if k == "nopred" else k for k in names] == list(_lib.DEPTH_SUMS) == list(R.SUMS) and sorted(slots.values()) == list(range(11))
    assert int(re.search(r"#define HB_DEPTH_NSUMS (\d+)", header).group(1)) == _lib.DEPTH_NSUMS == len(R.SUMS)
    assert int(re.search(r"#define HB_DEPTH_MAX_PS (\d+)", header).group(1)) == _lib.DEPTH_MAX_PS
    assert int(re.search(r"#define HB_DEPTH_MAX_GRID (\d+)", header).group(1)) == _lib.DEPTH_MAX_GRID
    assert "THE SUMMATION RULE" in header and "ratio of bilinears" in header
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_depth.h" in doc and all(n in doc for n in NAMES) and "HbirdDepthEvaluation" in doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "depth_targets_kernel" in design and "depth_upsample_metrics_kernel" in design and "depth_row_sums_kernel" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--task depth" in readme and "no dataset" in readme.lower() and "published" in readme


def test_depth_unit_is_built_outside_the_pinned_units_and_has_no_atomic():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hbird_depth.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_depth.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    for units in ("KNN_UNITS", "K5_UNITS", "RES_UNITS"):
        assert "hbird_depth" not in re.search(rf"^{units}\s*=(.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(csrc, "hbird_depth.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src, flags=re.S)
    assert set(kernels) == {"depth_targets_kernel", "depth_upsample_metrics_kernel", "depth_row_sums_kernel"}
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\batomic\w*\s*\(", code) and "unsafeAtomicAdd" not in code      # no atomic at all, so none on a float or a double
    assert "#pragma clang fp contract(off)" in code and "mfma" not in code.lower()


def test_depth_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused first
    for args, word in (((None, 1, 16, 16, 8, 2, 1e-3, 10.0, p, p, None), "NULL"), ((p, 1, 16, 16, 8, 3, 1e-3, 10.0, p, p, None), "divide"),
                       ((p, 1, 12, 16, 8, 2, 1e-3, 10.0, p, p, None), "multiples"), ((p, 1, -16, 16, 8, 2, 1e-3, 10.0, p, p, None), "positive"),
                       ((p, -1, 16, 16, 8, 2, 1e-3, 10.0, p, p, None), "negative"), ((p, 1, 16, 16, 8, 2, 0.0, 10.0, p, p, None), "bounds"),
                       ((p, 1, 130, 130, 65, 1, 1e-3, 10.0, p, p, None), "patch size")):
        assert L.hb_patch_depth_targets(*args) == -1 and word in _lib.last_error(), (args, _lib.last_error())
    for args, word in (((p, 1, 2, 2, 16, 16, None, 1e-3, 10.0, p, None, None), "NULL"), ((p, 1, 0, 2, 16, 16, p, 1e-3, 10.0, p, None, None), "positive"),
                       ((p, 1, 2, 2, 16, -1, p, 1e-3, 10.0, p, None, None), "positive"), ((p, 1, 2, 2, 16, 16, p, 2.0, 1.0, p, None, None), "bounds"),
                       ((p, 1, 1024, 8, 16, 16, p, 1e-3, 10.0, p, None, None), "exceeds")):
        assert L.hb_depth_upsample_metrics(*args) == -1 and word in _lib.last_error(), (args, _lib.last_error())
    assert L.hb_patch_depth_targets(None, 0, 16, 16, 8, 2, 1e-3, 10.0, None, None, None) == 0
    assert L.hb_depth_upsample_metrics(None, 0, 2, 2, 16, 16, None, 1e-3, 10.0, None, None, None) == 0


# ---- the model against hand-computed cases ---------------------------------------------------------------------------------------------------
def test_target_rows_by_hand():
    y = np.array([[[1.0, 2.0], [0.0, 3.0]]], dtype=F32)
    rows, flags = R.target_rows(y, 2, 1)
    assert rows.tolist() == [[[[1.5, 0.75]]]] and flags.tolist() == [[[1]]]                  # (1 + 2 + 3) / 4, 3 valid of 4
    rows, flags = R.target_rows(y, 2, 2)
    assert rows[0, 0, 0].tolist() == [1.0, 2.0, 0.0, 3.0, 1.0, 1.0, 0.0, 1.0]              # num cell-major, then den
    bad = np.array([[[0.0, np.nan], [np.inf, 11.0]]], dtype=F32)
    rows, flags = R.target_rows(bad, 2, 1)
    assert rows.tolist() == [[[[0.0, 0.0]]]] and flags.tolist() == [[[0]]]
    assert R.valid(np.array([1e-3, 10.0, 9.99e-4, 10.001, -1.0, np.nan, -np.inf], dtype=F32)).tolist() == [True, True, False, False, False, False, False]
    # the chain is row-major in fp32: 2^24 + 1 ties back to 2^24 three times; any other order, or float64, ends at 2^24 + 4
    big = np.array([[[2.0 ** 24, 1.0], [1.0, 1.0]]], dtype=F32)
    assert R.target_rows(big, 2, 1, hi=1e9)[0][0, 0, 0, 0] == F32(2.0 ** 24) / F32(4)
    assert R.target_rows(big[:, ::-1, ::-1].copy(), 2, 1, hi=1e9)[0][0, 0, 0, 0] == F32(2.0 ** 24 + 4) / F32(4)
    # two patches side by side, a rectangle
    two = np.array([[[1.0, 1.0, 5.0, 0.0], [1.0, 1.0, 5.0, 0.0]]], dtype=F32)
    rows, flags = R.target_rows(two, 2, 1)
    assert rows.shape == (1, 1, 2, 2) and rows[0, 0].tolist() == [[1.0, 1.0], [2.5, 0.5]]


def _agg_from_grids(num, den):
    """[G, G] cell grids of one image with S = 1, r = G -> agg [1, 1, 2 G^2]."""
    return np.concatenate([np.asarray(num, dtype=F32).reshape(-1), np.asarray(den, dtype=F32).reshape(-1)])[None, None, :]


def test_prediction_by_hand():
    i0, i1, l0, l1 = R.source_index(4, 2)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and l1.tolist() == [0.0, 0.25, 0.75, 0.25] and l0.tolist() == [1.0, 0.75, 0.25, 0.75]
    agg = _agg_from_grids([[1.0, 0.75], [1.0, 0.75]], [[1.0, 0.25], [1.0, 0.25]])            # depths 1 and 3, the second cell a quarter valid
    pred, has = R.predict(agg, 1, 2, 4, 4)
    assert has.all() and pred[0, 0, 0] == 1.0 and pred[0, 0, 1] == F32(0.9375) / F32(0.8125) and pred[0, 0, 3] == 3.0
    assert np.array_equal(pred[0, 0], pred[0, 3])
    # clamp and "no prediction"
    agg = _agg_from_grids([[12.0, 1e-4], [0.0, 0.0]], [[1.0, 1.0], [0.0, 0.0]])
    pred, has = R.predict(agg, 1, 2, 2, 2)                                                  # native size: every pixel is its cell
    assert pred[0, 0].tolist() == [10.0, F32(1e-3)] and has[0].tolist() == [[True, True], [False, False]]
    assert (pred.view(np.uint32)[0, 1] == R.NAN_BITS).all()
    cells = R.cell_grids(np.arange(2 * 2 * 8, dtype=F32).reshape(1, 4, 8), 2, 2)
    assert cells[0][0, 0].tolist() == [0.0, 1.0, 8.0, 9.0] and cells[0][0, 1].tolist() == [2.0, 3.0, 10.0, 11.0] and cells[1][0, 0, 0] == 4.0


def test_sums_and_metrics_by_hand():
    pred = np.array([[[2.0, 4.0, 5.0, 7.0]]], dtype=F32)
    has = np.array([[[True, True, True, False]]])
    gt = np.array([[[4.0, 4.5, np.nan, 3.0]]], dtype=F32)
    s, scales = R.sums(pred, has, gt)
    want = [2, 1, 4 + 0.25, 0.5 + 0.5 / 4.5, 1.0 + 0.25 / 4.5, math.log(0.5) ** 2 + math.log(4 / 4.5) ** 2, math.log(0.5) + math.log(4 / 4.5),
            math.log10(2) + abs(math.log10(4 / 4.5)), 1, 1, 1]
    assert s[0] == pytest.approx(want, rel=1e-14)
    assert scales[0, 1] == pytest.approx(math.log(2) + 2 * math.log(4) + math.log(4.5), rel=1e-14)      # sum of |ln p| + |ln g|
    m = R.finish(s[0])
    assert m["rmse"] == pytest.approx(math.sqrt(4.25 / 2)) and m["d1"] == 0.5 and m["abs_rel"] == pytest.approx(want[3] / 2)
    assert m["silog"] == pytest.approx(math.sqrt(want[5] / 2 - (want[6] / 2) ** 2))


# ---- wrong variants must fail a named check --------------------------------------------------------------------------------------------------
def check_holes_do_not_bias(predict):
    """A plane at 4 m seen through holes is still at 4 m wherever there is a prediction."""
    rng = np.random.default_rng(1)
    den = rng.uniform(0.1, 1.0, (6, 6)).astype(F32)
    den[rng.random((6, 6)) < 0.3] = 0.0
    pred, has = predict(_agg_from_grids(F32(4.0) * den, den), 1, 6, 48, 48)
    return bool(has.any() and (np.abs(pred[has] - 4.0) <= 1e-5).all())


def check_ratio_of_bilinears(predict):
    pred, _ = predict(_agg_from_grids([[1.0, 0.75], [1.0, 0.75]], [[1.0, 0.25], [1.0, 0.25]]), 1, 2, 4, 4)
    return bool(pred[0, 0, 1] == F32(0.9375) / F32(0.8125))


def check_clamped(predict):
    ok = True
    for S, r, h, w in ((2, 2, 16, 16), (3, 1, 37, 53)):
        agg, _ = R.agg_world(3, S, r, h, w, seed=9)
        raw, has = R.predict(agg, S, r, h, w, variant="no_clamp")
        assert (raw[has] > R.MAX_DEPTH).any()                                               # the world reaches beyond the range (below it: by hand, above)
        pred, has = predict(agg, S, r, h, w)
        ok = ok and bool((pred[has] >= F32(R.MIN_DEPTH)).all() and (pred[has] <= F32(R.MAX_DEPTH)).all())
    return ok


def check_half_pixel_centres(predict):
    pred, _ = predict(_agg_from_grids([[1.0, 2.0], [1.0, 2.0]], [[1.0, 1.0], [1.0, 1.0]]), 1, 2, 4, 4)
    return pred[0, 0].tolist() == [1.0, 1.25, 1.75, 2.0]


def check_invalid_gt_is_not_counted(sums):
    agg, gt = R.agg_world(3, 3, 2, 37, 53, seed=4)
    pred, has = R.predict(agg, 3, 2, 37, 53)
    s, _ = sums(pred, has, gt)
    return bool(np.isfinite(s).all() and (s[:, 0] + s[:, 1] == R.valid(gt).sum(axis=(1, 2))).all())


PREDICT_CHECKS = (check_holes_do_not_bias, check_ratio_of_bilinears, check_clamped, check_half_pixel_centres)


def test_the_model_passes_every_named_check():
    assert all(c(R.predict) for c in PREDICT_CHECKS) and check_invalid_gt_is_not_counted(R.sums)


@pytest.mark.parametrize("variant,check", [("den_ignored", check_holes_do_not_bias), ("ratio_first", check_ratio_of_bilinears), ("no_clamp", check_clamped),
                                           ("align_corners", check_half_pixel_centres), ("invalid_gt", check_invalid_gt_is_not_counted)])
def test_wrong_variants_fail_their_check(variant, check):
    if variant == "invalid_gt":
        assert not check(lambda *a: R.sums(*a, variant=variant))
    else:
        assert not check(lambda *a: R.predict(*a, variant=variant))


# ---- host logic ------------------------------------------------------------------------------------------------------------------------------
def test_metric_finishing_reports_empty_images_and_unpredicted_pixels():
    rng = np.random.default_rng(2)
    agg, gt = R.agg_world(3, 3, 1, 24, 24, seed=6)
    gt[1] = np.nan                                                                          # an image without ground truth
    pred, has = R.predict(agg, 3, 1, 24, 24)
    sums, _ = R.sums(pred, has, gt)
    res = hdepth.finish_metrics(sums)
    head, pooled, per, n_nopred, empty = R.metrics(sums)
    assert isinstance(res, dict) and set(res) == set(R.METRICS) == set(hdepth.METRICS)
    assert res.empty_images == empty == [1] and res.per_image[1] is None and res.n_nopred == n_nopred > 0
    assert all(res[m] == pytest.approx(head[m], rel=1e-14) and res.pooled[m] == pytest.approx(pooled[m], rel=1e-14) for m in R.METRICS)
    two = [res.per_image[0], res.per_image[2]]
    assert res["rmse"] == pytest.approx((two[0]["rmse"] + two[1]["rmse"]) / 2) and res["rmse"] != pytest.approx(res.pooled["rmse"], rel=1e-6)
    nothing = hdepth.finish_metrics(np.zeros((2, _lib.DEPTH_NSUMS)))
    assert all(math.isnan(v) for v in nothing.values()) and nothing.pooled is None and nothing.empty_images == [0, 1]
    assert rng is not None


def test_depth_folder_data_module_reads_npy_and_png(tmp_path):
    from PIL import Image
    from hbird_mi.data.synthetic_depth import DepthFolderDataModule, get_depth_dataset
    rng = np.random.default_rng(0)
    depths = {}
    for split, stems in (("train", ["a", "b", "c"]), ("val", ["d", "e"])):
        os.makedirs(tmp_path / split / "images"); os.makedirs(tmp_path / split / "depth")
        for i, stem in enumerate(stems):
            Image.fromarray(rng.integers(0, 255, (24, 32, 3), dtype=np.uint8)).save(tmp_path / split / "images" / f"{stem}.png")
            d = rng.uniform(0.5, 9.0, (24, 32)).astype(F32)
            d[:4, :4] = 0.0
            if i % 2 == 0:
                np.save(tmp_path / split / "depth" / f"{stem}.npy", d)
            else:
                mm = np.round(d * 1000).astype(np.uint16)
                Image.fromarray(mm).save(tmp_path / split / "depth" / f"{stem}.png")
                d = mm.astype(F32) / F32(1000.0)
            depths[stem] = d
    dm = DepthFolderDataModule(str(tmp_path), batch_size=2, num_workers=0, input_size=16)
    assert dm.get_train_dataset_size() == 3 and len(dm.val) == 2
    batches = list(dm.train_dataloader())
    assert [tuple(x.shape) for x, _ in batches] == [(2, 3, 16, 16), (1, 3, 16, 16)] and batches[0][1].shape == (2, 1, 16, 16)
    for (x, y), stems in zip(batches, (["a", "b"], ["c"])):
        assert y.dtype == torch.float32
        for yi, stem in zip(y[:, 0].numpy(), stems):
            assert np.isin(yi, depths[stem]).all()                                          # nearest: no value is invented
            assert (yi[:2, :2] == 0.0).all() and yi[8, 8] > 0                               # the hole is still top-left: no flip
    assert isinstance(get_depth_dataset("depth-folder", str(tmp_path), 2, 0, 16), DepthFolderDataModule)
    assert get_depth_dataset("synthetic-depth*0.5", "", 4, 0, 32).get_train_dataset_size() == 16
    with pytest.raises(ValueError, match="Unknown depth dataset"):
        get_depth_dataset("voc", "", 2, 0, 16)
    os.remove(tmp_path / "val" / "depth" / "e.png")
    with pytest.raises(RuntimeError, match="same stem"):
        DepthFolderDataModule(str(tmp_path), batch_size=2, num_workers=0, input_size=16)


def test_synthetic_depth_world_has_holes_and_colour_determines_depth():
    from hbird_mi.data.synthetic_depth import SyntheticDepthDataModule
    dm = SyntheticDepthDataModule(batch_size=4, input_size=32, n_train=8, n_val=4)
    x, y = dm.train_dataloader().batches[0]
    assert x.shape == (4, 3, 32, 32) and y.shape == (4, 1, 32, 32) and y.dtype == torch.float32
    ok = R.valid(y.numpy())
    assert 0.5 < ok.mean() < 1.0 and np.isnan(y.numpy()).any() and (y.numpy() == 0).any() and (np.nan_to_num(y.numpy()[:, :, -1], nan=99.0) > 10).all()
    again = SyntheticDepthDataModule(batch_size=4, input_size=32, n_train=8, n_val=4).train_dataloader().batches[0]
    assert torch.equal(again[0], x) and torch.equal(torch.nan_to_num(again[1]), torch.nan_to_num(y))
    with pytest.raises(ValueError, match="multiple"):
        SyntheticDepthDataModule(input_size=30)


def test_argument_errors_name_the_argument():
    net = torch.nn.Identity()
    for kw, word in ((dict(nn_params={"idx_shard": True}), "idx_shard"), (dict(nn_params={"gpu_ids": [0, 1]}), "gpu_ids"),
                     (dict(memory_size=10), "dataset_size"), (dict(n_neighbours=0), "n_neighbours"), (dict(beta=-1.0), "beta"),
                     (dict(target_grid=0), "target_grid"), (dict(target_grid=1.5), "target_grid"), (dict(min_depth=0.0), "min_depth"),
                     (dict(max_depth=float("inf")), "max_depth"), (dict(device="cpu"), "device")):
        with pytest.raises(ValueError, match=word):
            hdepth.HbirdDepthEvaluation(net, [], **kw)
    base = dict(d_model=3, patch_size=8, dataset_name="synthetic-depth", data_dir="")
    for name, value in (("frame_size", (64, 64)), ("window_stride", 8), ("grid_k", [3]), ("grid_beta", [0.1]), ("bootstrap", 100),
                        ("leave_one_out", True), ("memory_sizes", [10]), ("overclustering", [4]), ("linear_probe", True)):
        with pytest.raises(ValueError, match=f"{name} is not available for depth"):
            hdepth.hbird_depth_evaluation(net, **base, **{name: value})
    with pytest.raises(TypeError, match="unexpected keyword"):
        hdepth.hbird_depth_evaluation(net, **base, num_classes=3)
    with pytest.raises(ValueError, match="float32"):
        ops.patch_depth_targets(torch.zeros((1, 8, 8), dtype=torch.float64), 8)
    with pytest.raises(ValueError, match="target_grid"):
        ops.patch_depth_targets(torch.zeros((1, 8, 8)), 8, 3)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        ops.patch_depth_targets(torch.zeros((1, 8, 8)), 8)


def test_cli_task_depth_parser():
    spec = importlib.util.spec_from_file_location("hb_cli_depth_cpu", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    base = ["--dataset-name", "synthetic-depth", "--data-dir", "", "--d-model", "3", "--patch-size", "8"]
    a = cli.build_parser().parse_args(base)
    assert a.task == "segmentation" and a.target_grid == 1 and a.min_depth == 1e-3 and a.max_depth == 10.0 and a.depth_scale == 1000.0
    a = cli.build_parser().parse_args(base + ["--task", "depth", "--target-grid", "4", "--min-depth", "0.1", "--max-depth", "80"])
    assert a.task == "depth" and a.target_grid == 4 and a.min_depth == 0.1 and a.max_depth == 80.0
    for bad in (["--task", "pose"], ["--target-grid", "0"], ["--min-depth", "0"], ["--max-depth", "inf"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)
    for clash in (["--grid-k", "3"], ["--bootstrap", "10"], ["--frame-size", "64", "64"], ["--memory-sizes", "10"], ["--leave-one-out"],
                  ["--overclustering", "4"], ["--linear-probe"]):
        with pytest.raises(SystemExit):
            cli.main(base + ["--task", "depth"] + clash)
    assert isinstance(cli.build_model(a), torch.nn.Module)                                  # the self-check's patch-pooling stand-in
