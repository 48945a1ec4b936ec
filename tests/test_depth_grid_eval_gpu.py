"""HbirdDepthEvaluation.evaluate_grid / evaluate_leave_one_out / DepthBootstrap, hbird_depth_grid_evaluation and eval.py --task depth-grid on the
GPU, in the world of tests/test_depth_eval_gpu.py (32 px, ps 8, S 4, 8 training and 4 validation images, pooling extractor and tiny ViT).

Everything is held to the single-configuration route, bit for bit: a grid's configuration IS `from_index(index, n_neighbours=k, beta=beta)
.evaluate(...)`, a leave-one-out image IS `evaluate` on `select_rows(all rows but that image's)`, and the bootstrap IS the numpy estimator of
tests/depth_grid_refs.py on the pass's own `.sums` with the device's own multiplicities."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import depth_grid_refs as G
import depth_refs as R
import test_depth_eval_gpu as E
from hbird_mi import depth as hdepth
from hbird_mi import ops

pytestmark = pytest.mark.gpu

S, VAL, TRAIN = E.S, E.VAL, E.TRAIN
KS, BETAS = [1, 3, 5], [0.02, 0.1]
CONFIGS = [(k, b) for k in KS for b in BETAS]


def _bits(sums):
    return np.ascontiguousarray(sums, dtype=np.float64).view(np.int64)


def _single(ev, index, k, beta, loader):
    one = hdepth.HbirdDepthEvaluation.from_index(ev.feature_extractor, index, n_neighbours=k, beta=beta, target_grid=ev.target_grid)
    return one.evaluate(loader, S)


def _count_calls(obj, name, calls):
    real = getattr(obj, name)
    def wrapped(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    setattr(obj, name, wrapped)


@pytest.mark.parametrize("which,r", [("pool", 1), ("vit", 2)])
def test_every_grid_configuration_is_the_separate_evaluation_from_one_search_per_batch(cuda_device, which, r):
    ev = E._build(E._pool() if which == "pool" else E._vit(), target_grid=r)
    want = {(k, b): _single(ev, ev.index, k, b, VAL) for k, b in CONFIGS}
    calls = []
    for name in ("search_aggregate_grid", "search_aggregate", "search", "aggregate_grid"):
        _count_calls(ev.index, name, calls)
    _count_calls(ev, "_tokens", calls)
    res = ev.evaluate_grid(VAL, S, n_neighbours=[5, 1, 3, 3], betas=[0.1, 0.02])
    assert calls == ["_tokens", "search_aggregate_grid"] * len(VAL)                             # tokens once, ONE search per batch
    assert list(res) == CONFIGS
    for key in CONFIGS:
        assert isinstance(res[key], hdepth.DepthMetrics) and np.array_equal(_bits(res[key].sums), _bits(want[key].sums)), key
        assert dict(res[key]) == dict(want[key]) and res[key].pooled == want[key].pooled and res[key].n_nopred == want[key].n_nopred
    own = ev.evaluate_grid(VAL, S)                                                              # the evaluator's own (k, beta): a grid of one
    assert list(own) == [(ev.n_neighbours, ev.beta)] and np.array_equal(_bits(own[(5, 0.02)].sums), _bits(want[(5, 0.02)].sums))
    # the configurations do differ in this world -- but for k = 1, where the one weight is 1 whatever beta is
    assert len({_bits(want[key].sums).tobytes() for key in CONFIGS}) == len(CONFIGS) - 1
    assert np.array_equal(_bits(want[(1, 0.02)].sums), _bits(want[(1, 0.1)].sums))
    ev.index.close()


def test_more_than_sixteen_configurations(cuda_device):
    ev = E._build(E._pool(), target_grid=2)
    ks, betas = [1, 2, 3, 4, 5, 6], [0.02, 0.05, 0.1]
    res = ev.evaluate_grid(VAL, S, n_neighbours=ks, betas=betas)
    assert list(res) == [(k, b) for k in ks for b in betas]
    for key in ((1, 0.02), (4, 0.05), (6, 0.1)):
        assert np.array_equal(_bits(res[key].sums), _bits(_single(ev, ev.index, *key, VAL).sums)), key
    ev.index.close()


def test_views_of_a_bounded_build(cuda_device):
    big = E._build(E._pool(), train=E.TRAIN_HOLE, target_grid=2, memory_size=8 * 6, dataset_size=8)
    views = {16: big.memory_view(16), 32: big.memory_view(32)}
    res = big.evaluate_grid(VAL, S, n_neighbours=[1, 3], betas=BETAS, views=views)
    assert list(res) == [(size, k, b) for size in (16, 32) for k in (1, 3) for b in BETAS]
    for (size, k, b), got in res.items():
        assert np.array_equal(_bits(got.sums), _bits(_single(big, views[size].index, k, b, VAL).sums)), (size, k, b)
    assert np.array_equal(_bits(res[(32, 3, 0.02)].sums), _bits(hdepth.HbirdDepthEvaluation.from_index(
        big.feature_extractor, views[32].index, n_neighbours=3, target_grid=2).evaluate(VAL, S).sums))
    other = E._build(E._pool(), target_grid=1)
    for bad, word in (({"x": other}, "'x'"), ({7: object()}, "7"), ({}, "empty")):
        with pytest.raises(ValueError, match=word):
            big.evaluate_grid(VAL, S, views=bad)
        with pytest.raises(ValueError, match=word):
            big.evaluate_leave_one_out(E.TRAIN_HOLE, S, views=bad)
    for ev in (big, other, *views.values()):
        ev.index.close()


def _all_but(ev, image):
    groups = ev.row_groups()
    return torch.nonzero(groups != image).reshape(-1)


def _images(batches):
    return [(x[i:i + 1], y[i:i + 1]) for x, y in batches for i in range(x.shape[0])]


@pytest.mark.parametrize("which,epochs,ks", [("pool", 1, KS), ("vit", 2, [3])])
def test_leave_one_out_is_the_evaluation_without_the_images_own_rows(cuda_device, which, epochs, ks):
    ev = E._build(E._pool() if which == "pool" else E._vit(), target_grid=2, augmentation_epoch=epochs)
    groups = ev.row_groups()
    assert groups.shape == (epochs * 8 * S * S,) and groups.dtype == torch.int32
    if epochs == 2:                                                                            # an image's rows lie in two ranges
        rows = torch.nonzero(groups == 3).reshape(-1)
        assert rows.tolist() == list(range(3 * 16, 4 * 16)) + list(range(8 * 16 + 3 * 16, 8 * 16 + 4 * 16))
    res = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=ks, betas=BETAS)
    assert list(res) == [(k, b) for k in ks for b in BETAS] and all(len(m.per_image) == 8 for m in res.values())
    for i, image in enumerate(_images(TRAIN)):
        rest = ev.index.select_rows(_all_but(ev, i))
        assert rest.ntotal == epochs * 7 * S * S
        for key, got in res.items():
            assert np.array_equal(_bits(got.sums[i]), _bits(_single(ev, rest, *key, [image]).sums[0])), (i, key)
        rest.close()
    screened = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=ks, betas=BETAS, screen=True)
    assert isinstance(ev.loo_screen_served, int) and 0 <= ev.loo_screen_served <= len(TRAIN)
    assert all(np.array_equal(_bits(screened[key].sums), _bits(res[key].sums)) for key in res)    # the same floats
    ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=ks, betas=BETAS, screen=False)
    assert ev.loo_screen_served == 0
    cut = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=ks, betas=BETAS, max_images=5)         # stops inside the second batch
    assert all(np.array_equal(_bits(cut[key].sums), _bits(res[key].sums[:5])) for key in res)
    with pytest.raises(ValueError, match="more than the 8 images"):
        ev.evaluate_leave_one_out(list(TRAIN) + [TRAIN[0]], S, n_neighbours=ks, betas=BETAS)
    with pytest.raises(ValueError, match="max_images"):
        ev.evaluate_leave_one_out(TRAIN, S, max_images=0)
    ev.index.close()


def test_leave_one_out_on_views_and_on_a_bank_without_geometry(cuda_device):
    big = E._build(E._pool(), train=E.TRAIN_HOLE, target_grid=1, memory_size=8 * 6, dataset_size=8)
    view = big.memory_view(24)
    assert view.row_groups().tolist() == [i for i in range(8) for _ in range(3)] and view._leave_one_out_images() == 8
    res = big.evaluate_leave_one_out(E.TRAIN_HOLE, S, n_neighbours=[1, 3], views={24: view, 48: big})
    alone = view.evaluate_leave_one_out(E.TRAIN_HOLE, S, n_neighbours=[1, 3])
    assert all(np.array_equal(_bits(res[(24, k, b)].sums), _bits(alone[(k, b)].sums)) for k, b in alone)
    image = _images(E.TRAIN_HOLE)[6]
    rest = view.index.select_rows(_all_but(view, 6))
    assert np.array_equal(_bits(res[(24, 3, 0.02)].sums[6]), _bits(_single(big, rest, 3, 0.02, [image]).sums[0]))
    rest.close()
    bare = hdepth.HbirdDepthEvaluation.from_index(big.feature_extractor, view.index, n_neighbours=3)
    with pytest.raises(ValueError, match="set_row_groups"):
        bare.evaluate_leave_one_out(E.TRAIN_HOLE, S)
    with pytest.raises(ValueError, match="24 rows"):
        bare.set_row_groups(torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="integers"):
        bare.set_row_groups(torch.zeros(24))
    bare.set_row_groups(view.row_groups())
    given = bare.evaluate_leave_one_out(E.TRAIN_HOLE, S, n_neighbours=[1, 3])
    assert all(np.array_equal(_bits(given[key].sums), _bits(alone[key].sums)) for key in alone)
    for ev in (big, view):
        ev.index.close()


def test_bootstrap_is_the_numpy_estimator_on_the_sums_with_the_devices_multiplicities(cuda_device):
    ev = E._build(E._vit(), target_grid=2)
    plain = ev.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS)
    boot = ev.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=(64, 5))
    assert isinstance(boot, hdepth.DepthBootstrap) and boot.keys == CONFIGS and boot.seed == 5 and boot.n_images == 4
    for key in CONFIGS:                                                                         # the plain pass, float for float
        assert dict(boot.metrics[key]) == dict(plain[key]) and np.array_equal(_bits(boot.metrics[key].sums), _bits(plain[key].sums))
    W = ops.bootstrap_multiplicities(4, 5, 64).cpu().numpy()
    want, want_pooled = G.depth_bootstrap(np.stack([plain[key].sums for key in CONFIGS]), W)
    for m in R.METRICS:
        assert boot.samples[m].shape == (64, len(CONFIGS))
        assert np.array_equal(_bits(boot.samples[m]), _bits(want[m])) and np.array_equal(_bits(boot.pooled_samples[m]), _bits(want_pooled[m])), m
    again = ev.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=(64, 5))
    other = ev.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=(64, 6))
    assert all(np.array_equal(_bits(again.samples[m]), _bits(boot.samples[m])) for m in R.METRICS)
    assert any(not np.array_equal(_bits(other.samples[m]), _bits(boot.samples[m])) for m in R.METRICS)
    for step in (1, 7):                                                                         # the pass size does not enter
        cut = hdepth.depth_bootstrap(CONFIGS, plain, 64, 5, ev.gpu_device, _pass_replicates=step)
        assert all(np.array_equal(_bits(cut.samples[m]), _bits(boot.samples[m])) and
                   np.array_equal(_bits(cut.pooled_samples[m]), _bits(boot.pooled_samples[m])) for m in R.METRICS)
    lo, hi = boot.interval((5, 0.02), "rmse")
    assert lo <= plain[(5, 0.02)]["rmse"] <= hi and boot.best("rmse")[0] in CONFIGS and boot.best("d1")[0] in CONFIGS
    loo = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=[3], bootstrap=16)                    # ... and over the training images
    assert loo.n_images == 8 and loo.samples["rmse"].shape == (16, 1) and loo.seed == hdepth.hboot.DEFAULT_SEED
    ev.index.close()


def test_the_one_call_function_and_the_cli(cuda_device, tmp_path):
    kw = dict(d_model=3, patch_size=8, dataset_name="synthetic-depth", data_dir="", batch_size=8, input_size=64, device="cuda", n_neighbours=5,
              ftr_extr_fn=lambda m, x: (torch.nn.functional.avg_pool2d(x, 8).flatten(2).transpose(1, 2).contiguous(), None))
    single = hdepth.hbird_depth_evaluation(E._Identity(), target_grid=2, **kw)
    res = hdepth.hbird_depth_grid_evaluation(E._Identity(), target_grid=2, grid_k=[1, 5], grid_beta=[0.02, 0.1], **kw)
    assert list(res) == [(1, 0.02), (1, 0.1), (5, 0.02), (5, 0.1)] and hdepth.last_run_info["bank_rows"] == 32 * 64
    assert np.array_equal(_bits(res[(5, 0.02)].sums), _bits(single.sums)) and dict(res[(5, 0.02)]) == dict(single)
    torch.manual_seed(1)
    sized = hdepth.hbird_depth_grid_evaluation(E._Identity(), target_grid=2, grid_k=[1, 5], memory_size=32 * 16, memory_sizes=[32 * 4, 32 * 16, 32 * 99],
                                               leave_one_out=True, leave_one_out_images=6, bootstrap=20, bootstrap_seed=3, **kw)
    assert isinstance(sized, hdepth.DepthBootstrap) and sized.keys == [(128, 1, 0.02), (128, 5, 0.02), (512, 1, 0.02), (512, 5, 0.02)]
    assert sized.n_images == 6 and sized.seed == 3 and sized.samples["d1"].shape == (20, 4)
    # the single-configuration entry still refuses all of it
    for clash in (dict(frame_size=(128, 128)), dict(window_stride=32), dict(grid_k=[3]), dict(grid_beta=[0.1]), dict(bootstrap=10),
                  dict(leave_one_out=True), dict(memory_sizes=[64])):
        with pytest.raises(ValueError, match=f"{next(iter(clash))} is not available for depth"):
            hdepth.hbird_depth_evaluation(E._Identity(), **kw, **clash)
    spec = importlib.util.spec_from_file_location("hb_cli_depth_grid", os.path.join(E.ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    base = ["--task", "depth-grid", "--dataset-name", "synthetic-depth", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64",
            "--batch-size", "8", "--device", "cuda", "--n-neighbours", "5", "--target-grid", "2", "--out", out, "--log-level", "WARNING"]
    cli.main(base + ["--grid-k", "1", "5", "--grid-beta", "0.02", "0.1", "--bootstrap", "50", "--bootstrap-seed", "9", "--bootstrap-metric", "d1"])
    js = json.load(open(out))
    assert js["task"] == "depth-grid" and js["headline"] == "k=5,beta=0.02" and all(js[m] == res[(5, 0.02)][m] for m in R.METRICS)
    assert set(js["depth_grid"]) == {"k=1,beta=0.02", "k=1,beta=0.1", "k=5,beta=0.02", "k=5,beta=0.1"}
    assert all(js["depth_grid"]["k=1,beta=0.1"][m] == res[(1, 0.1)][m] for m in R.METRICS) and js["depth_grid"]["k=1,beta=0.1"]["pooled"] == res[(1, 0.1)].pooled
    assert all(len(js[f"{m}_ci"]) == 2 and js[f"{m}_ci"][0] <= js[f"{m}_ci"][1] for m in ("rmse", "abs_rel", "d1"))
    assert js["grid_best"] in js["depth_grid"] and set(js["grid_indistinguishable_from_best"]) <= set(js["depth_grid"])
    assert js["bootstrap"] == {"replicates": 50, "seed": 9, "level": 0.95, "metric": "d1", "n_images": 16} and js["n_images"] == 16 and "miou" not in js
    cli.main(base + ["--memory-size", "512", "--memory-sizes", "128", "512", "--leave-one-out", "--leave-one-out-images", "4"])
    js = json.load(open(out))
    assert set(js["depth_grid"]) == {"memory=128,k=5,beta=0.02", "memory=512,k=5,beta=0.02"} and js["headline"] == "memory=512,k=5,beta=0.02"
    assert js["leave_one_out"] is True and js["n_images"] == 4 and "rmse_ci" not in js and "grid_best" not in js
