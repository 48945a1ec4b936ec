"""HbirdEvaluation.evaluate_grid / hbird_evaluation(grid_k=, grid_beta=) / eval.py --grid-k --grid-beta on the GPU, in the 64-px, C = 5,
24-image world of tests/test_memory_views_gpu.py: every (k, beta) of a grid out of one validation pass with one search per batch must be,
float for float, what a separately built evaluator with that n_neighbours and beta returns."""
import copy
import importlib.util
import json
import os

import pytest
import torch

import test_memory_views_gpu as W
from hbird_mi.hbird_eval import HbirdEvaluation
from test_memory_views_gpu import C, N_IMG, S, TRAIN, VAL, _build, _built, _extractor, _synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, BETAS = (3, 10, 40), (0.02, 0.1)


def _separate(k, beta, **nn_params):
    torch.manual_seed(1234)
    kw = {} if beta is None else {"beta": beta}
    return HbirdEvaluation(_extractor(), TRAIN, num_classes=C, n_neighbours=k, augmentation_epoch=1, device="cuda", nn_method="hip",
                           nn_params=dict(nn_params), memory_size=None, dataset_size=N_IMG, **kw)


def test_grid_equals_separately_built_evaluators(cuda_device):
    ev = _built(None)
    grid = ev.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS)
    assert list(grid) == [(k, b) for k in KS for b in BETAS] and all(isinstance(v, float) for v in grid.values())
    for (k, b), v in grid.items():
        one = _separate(k, b)
        assert one.beta == b and one.n_neighbours == k
        assert v == one.evaluate(VAL, S), (k, b)
    assert len(set(grid.values())) >= 2, grid            # the grid's knobs move the result in this world
    assert all(0.0 < v <= 1.0 for v in grid.values())
    # any order, repeats: the same grid
    assert ev.evaluate_grid(VAL, S, n_neighbours=[40, 3, 10, 3], betas=[0.1, 0.02]) == grid


def test_grid_over_views_runs_the_extractor_once_per_batch(cuda_device):
    big = _built(N_IMG * 40)
    views = {"9of40": big.memory_view(memory_size=N_IMG * 9), "40of40": big}
    calls = []
    hook = _extractor().model.register_forward_hook(lambda *a: calls.append(1))
    try:
        big.evaluate(VAL, S)
        per_pass = len(calls)                       # the ViT's forward calls of ONE validation pass
        got = big.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, views=views)
    finally:
        hook.remove()
    assert per_pass >= len(VAL) and len(calls) == 2 * per_pass, (per_pass, len(calls))
    assert list(got) == [(key, k, b) for key in views for k in KS for b in BETAS]
    for key, view in views.items():
        own = view.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS)
        for (k, b), v in own.items():
            assert got[(key, k, b)] == v, (key, k, b)
    assert got[("9of40", 10, 0.02)] != got[("40of40", 10, 0.02)]
    assert got[("9of40", 10, 0.02)] == views["9of40"].evaluate(VAL, S)      # K_NN = 10, beta = 0.02: the view's plain evaluation


def test_grid_on_a_multi_index_equals_the_single_index(cuda_device):
    single = _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS)
    multi = _build(None, gpu_ids=[0, 0], idx_shard=True)
    assert type(multi.index).__name__ == "HipMultiIndex" and multi.index.shard
    assert multi.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS) == single
    multi.index.close()


def test_grid_refusals_and_defaults(cuda_device):
    ev = _built(None)
    with pytest.raises(ValueError, match="window"):
        ev.evaluate_grid(VAL, S, n_neighbours=KS, window=(64, 64))
    with pytest.raises(ValueError, match="return_knn_details"):
        ev.evaluate_grid(VAL, S, n_neighbours=KS, return_knn_details=True)
    ranked = copy.copy(ev)
    ranked.world, ranked.rank = 2, 0                        # an evaluator of a torch.distributed world (replicas) ...
    with pytest.raises(ValueError, match="torch.distributed"):
        ranked.evaluate_grid(VAL, S, n_neighbours=KS)
    sharded = copy.copy(ev)
    sharded.sharded = True                                  # ... and a row-sharded one
    with pytest.raises(ValueError, match="torch.distributed"):
        sharded.evaluate_grid(VAL, S, n_neighbours=KS)
    with pytest.raises(ValueError, match="torch.distributed"):
        ev.evaluate_grid(VAL, S, n_neighbours=KS, views={"a": ranked})
    for bad in (dict(n_neighbours=[]), dict(n_neighbours=[0]), dict(n_neighbours=[2049]), dict(betas=[0.0]), dict(betas=[float("nan")]),
                dict(betas=[float("inf")]), dict(n_neighbours=[1.5]), dict(views={})):
        with pytest.raises(ValueError):
            ev.evaluate_grid(VAL, S, **bad)
    # the defaults are the evaluator's own n_neighbours and beta: its plain evaluation
    plain = ev.evaluate(VAL, S)
    assert ev.beta == 0.02 and ev.evaluate_grid(VAL, S) == {(W.K_NN, 0.02): plain}
    # beta = 0.02 given explicitly is today's evaluator; another beta is carried by from_index and memory_view
    assert _separate(W.K_NN, 0.02).evaluate(VAL, S) == plain == _separate(W.K_NN, None).evaluate(VAL, S)
    warm = _separate(W.K_NN, 0.1)
    assert warm.beta == 0.1 and warm.memory_view(rows=[0, 1, 2]).beta == 0.1
    assert HbirdEvaluation.from_index(_extractor(), warm.index, C, W.K_NN, device="cuda", beta=0.1).beta == 0.1
    assert warm.evaluate(VAL, S) == ev.evaluate_grid(VAL, S, betas=0.1)[(W.K_NN, 0.1)]
    for beta in (0.0, -1.0, float("nan"), float("inf"), "0.02"):
        with pytest.raises(ValueError, match="beta"):
            HbirdEvaluation.from_index(_extractor(), ev.index, C, W.K_NN, device="cuda", beta=beta)


def test_hbird_evaluation_grid(cuda_device):
    """The synthetic data module: 32 training images; 640 -> K = 20 rows per image, 160 -> K = 5."""
    grid = _synthetic(grid_k=[3, 10], grid_beta=[0.02, 0.1])
    assert list(grid) == [(3, 0.02), (3, 0.1), (10, 0.02), (10, 0.1)] and all(isinstance(v, float) and 0.0 < v <= 1.0 for v in grid.values())
    only_k = _synthetic(grid_k=[30, 3])
    assert list(only_k) == [(3, 0.02), (30, 0.02)] and only_k[(30, 0.02)] == _synthetic() and only_k[(3, 0.02)] == grid[(3, 0.02)]
    assert list(_synthetic(grid_beta=[0.1])) == [(30, 0.1)]
    sweep = _synthetic(memory_size=640, memory_sizes=[160, 640, 10 ** 6], grid_k=[3, 10], grid_beta=[0.02, 0.1])
    assert list(sweep) == [160, 640] and all(list(v) == list(grid) for v in sweep.values())
    for size in (160, 640):
        assert sweep[size] == _synthetic(memory_size=size, grid_k=[3, 10], grid_beta=[0.02, 0.1]), size
    with pytest.raises(ValueError, match="return_knn_details"):
        _synthetic(grid_k=[3], return_knn_details=True)


def test_cli_grid(cuda_device, tmp_path):
    spec = importlib.util.spec_from_file_location("hb_cli_grid", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    cli.main(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64", "--batch-size", "8",
              "--device", "cuda", "--nn-method", "hip", "--grid-k", "3", "10", "--grid-beta", "0.02", "0.1", "--out", out, "--log-level", "WARNING"])
    res = json.load(open(out))
    assert set(res["miou_grid"]) == {"k=3,beta=0.02", "k=3,beta=0.1", "k=10,beta=0.02", "k=10,beta=0.1"}
    assert all(0.0 < v <= 1.0 for v in res["miou_grid"].values()) and res["miou"] == res["miou_grid"]["k=3,beta=0.02"]
    assert "miou_by_memory_size" not in res and res["n_neighbours"] == 30
