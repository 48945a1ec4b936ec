"""evaluate_grid(bootstrap=) / evaluate_leave_one_out(bootstrap=) / hbird_evaluation(bootstrap=) / eval.py --bootstrap on the GPU, in the 64-px,
C = 5, 24-image world of tests/test_memory_views_gpu.py: the mIoU floats are those of the pass without bootstrap=, the point row is the same
quantity under the identity matching (within G * 2^-52: a sequential against a pairwise sum), and the replicates are paired -- a column does
not depend on which other configurations or views were evaluated with it."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

from hbird_mi import bootstrap as hboot
from test_memory_views_gpu import C, N_IMG, S, TRAIN, VAL, _built, _synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, BETAS = (3, 10, 40), (0.02, 0.1)
R = 200
BOUND = C * 2.0 ** -52


def _q(level):
    """The quantile pair of a two-sided interval, as the definition writes it."""
    return [(1 - level) / 2, (1 + level) / 2]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _grid_boot():
    return _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=R)


@functools.lru_cache(maxsize=None)
def _grid_plain():
    return _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS)


def test_grid_bootstrap_carries_the_grid_floats_and_the_identity_point_row(cuda_device):
    mb, plain = _grid_boot(), _grid_plain()
    assert isinstance(mb, hboot.MiouBootstrap) and type(plain) is dict
    assert mb.keys == list(plain) == [(k, b) for k in KS for b in BETAS] and list(mb.miou) == mb.keys
    assert mb.miou == plain                                             # float for float
    assert mb.n_images == sum(x.shape[0] for x, _ in VAL) and mb.seed == hboot.DEFAULT_SEED
    assert mb.samples.dtype == np.float64 and mb.samples.shape == (R, len(mb.keys))
    point = mb.point.cpu().numpy()
    assert mb.point.is_cuda and point.dtype == np.float64
    for c, key in enumerate(mb.keys):
        assert abs(point[c] - mb.miou[key]) <= BOUND, key
    assert mb.matching_is_identity == {key: True for key in mb.keys}
    assert (mb.samples.std(axis=0) > 0).all() and ((mb.samples > 0) & (mb.samples <= 1)).all()     # the replicates move
    # the same seed: the same bits; another seed: other samples, the same floats
    again = _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=(R, hboot.DEFAULT_SEED))
    other = _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=(R, 7))
    assert np.array_equal(_bits(again.samples), _bits(mb.samples)) and again.miou == mb.miou
    assert other.seed == 7 and not np.array_equal(other.samples, mb.samples) and other.miou == mb.miou
    assert np.array_equal(_bits(other.point.cpu().numpy()), _bits(point))


def test_bootstrap_none_is_the_plain_dict(cuda_device):
    assert type(_built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=None)) is dict
    assert _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=None) == _grid_plain()
    for bad in (0, -1, 1.5, (1 << 20) + 1, (10, -1)):
        with pytest.raises(ValueError, match="bootstrap"):
            _built(None).evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=bad)


def test_a_subset_of_the_grid_returns_the_same_columns(cuda_device):
    mb = _grid_boot()
    sub = _built(None).evaluate_grid(VAL, S, n_neighbours=(10,), betas=(0.1,), bootstrap=R)
    assert sub.keys == [(10, 0.1)] and sub.samples.shape == (R, 1)
    assert np.array_equal(_bits(sub.samples[:, 0]), _bits(mb.samples[:, mb.keys.index((10, 0.1))]))
    two = _built(None).evaluate_grid(VAL, S, n_neighbours=(3, 40), betas=(0.02,), bootstrap=R)
    for c, key in enumerate(two.keys):
        assert np.array_equal(_bits(two.samples[:, c]), _bits(mb.samples[:, mb.keys.index(key)])), key


def test_views_columns_equal_each_views_own_run(cuda_device):
    big = _built(N_IMG * 40)
    views = {"9of40": big.memory_view(memory_size=N_IMG * 9), "40of40": big}
    got = big.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, views=views, bootstrap=R)
    assert got.keys == [(key, k, b) for key in views for k in KS for b in BETAS]
    assert got.miou == big.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, views=views)
    for key, view in views.items():
        own = view.evaluate_grid(VAL, S, n_neighbours=KS, betas=BETAS, bootstrap=R)
        for c, (k, b) in enumerate(own.keys):
            assert np.array_equal(_bits(own.samples[:, c]), _bits(got.samples[:, got.keys.index((key, k, b))])), (key, k, b)
            assert own.miou[(k, b)] == got.miou[(key, k, b)]
    d, lo, hi, share = got.difference(("40of40", 10, 0.02), ("9of40", 10, 0.02))
    assert d == got.miou[("40of40", 10, 0.02)] - got.miou[("9of40", 10, 0.02)] and lo <= hi and 0.0 <= share <= 1.0
    views["9of40"].index.close()


def test_interval_difference_and_best_agree_with_numpy(cuda_device):
    mb = _grid_boot()
    s = mb.samples
    for c, key in enumerate(mb.keys):
        assert np.array_equal(mb.interval(key), np.quantile(s[:, c], _q(0.95)))
        assert np.array_equal(mb.interval(key, 0.8), np.quantile(s[:, c], _q(0.8)))
    a, b = mb.keys[2], mb.keys[5]
    d = s[:, 2] - s[:, 5]
    assert mb.difference(a, b, 0.9) == (mb.miou[a] - mb.miou[b], *np.quantile(d, _q(0.9)).tolist(), float((d > 0).mean()))
    top, tied = mb.best()
    vals = [mb.miou[k] for k in mb.keys]
    assert top == mb.keys[int(np.argmax(vals))]
    want = []
    for c, key in enumerate(mb.keys):
        lo, hi = np.quantile(s[:, mb.keys.index(top)] - s[:, c], _q(0.95))
        if key != top and lo <= 0 <= hi:
            want.append(key)
    assert tied == want


def test_leave_one_out_bootstrap(cuda_device):
    ev = _built(None)
    plain = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS)
    mb = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS, bootstrap=(R, 11))
    assert type(plain) is dict and isinstance(mb, hboot.MiouBootstrap)
    assert mb.miou == plain and mb.keys == list(plain) and mb.n_images == N_IMG and mb.seed == 11
    point = mb.point.cpu().numpy()
    for c, key in enumerate(mb.keys):
        assert abs(point[c] - mb.miou[key]) <= BOUND, key
    assert mb.samples.shape == (R, len(plain)) and (mb.samples.std(axis=0) > 0).all()
    few = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS, max_images=6, bootstrap=(R, 11))
    assert few.n_images == 6 and few.miou == ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS, max_images=6)


def test_hbird_evaluation_and_cli_bootstrap(cuda_device, tmp_path):
    grid = _synthetic(grid_k=[3, 10])
    mb = _synthetic(grid_k=[3, 10], bootstrap=100, bootstrap_seed=5)
    assert isinstance(mb, hboot.MiouBootstrap) and mb.miou == grid and mb.seed == 5 and mb.samples.shape == (100, 2)
    one = _synthetic(bootstrap=100)
    assert one.keys == [(30, 0.02)] and one.miou[(30, 0.02)] == _synthetic() and one.seed == hboot.DEFAULT_SEED
    sized = _synthetic(memory_size=640, memory_sizes=[160, 640], bootstrap=100)
    assert sized.keys == [(160, 30, 0.02), (640, 30, 0.02)]
    assert {k[0]: v for k, v in sized.miou.items()} == _synthetic(memory_size=640, memory_sizes=[160, 640])
    with pytest.raises(ValueError, match="bootstrap_seed needs bootstrap"):
        _synthetic(bootstrap_seed=5)
    spec = importlib.util.spec_from_file_location("hb_cli_bootstrap", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    cli.main(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64", "--batch-size", "8",
              "--device", "cuda", "--nn-method", "hip", "--grid-k", "3", "10", "--bootstrap", "100", "--bootstrap-seed", "5",
              "--bootstrap-level", "0.9", "--out", out, "--log-level", "WARNING"])
    res = json.load(open(out))
    assert set(res["miou_grid"]) == set(res["miou_grid_ci"]) == {"k=3,beta=0.02", "k=10,beta=0.02"}
    assert res["grid_best"] in res["miou_grid"] and set(res["grid_indistinguishable_from_best"]) <= set(res["miou_grid"]) - {res["grid_best"]}
    assert res["miou"] == res["miou_grid"]["k=3,beta=0.02"] and len(res["miou_ci"]) == 2 and res["miou_ci"][0] <= res["miou_ci"][1]
    assert res["miou_ci"] == res["miou_grid_ci"]["k=3,beta=0.02"]
    assert res["bootstrap"]["replicates"] == 100 and res["bootstrap"]["seed"] == 5 and res["bootstrap"]["level"] == 0.9
    out1 = str(tmp_path / "one.json")
    cli.main(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64", "--batch-size", "8",
              "--device", "cuda", "--nn-method", "hip", "--bootstrap", "50", "--out", out1, "--log-level", "WARNING"])
    res1 = json.load(open(out1))
    assert "miou_ci" in res1 and "miou_grid_ci" not in res1 and "grid_best" not in res1 and "miou_grid" not in res1
