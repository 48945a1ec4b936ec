"""hbird_mi.depth.HbirdDepthEvaluation / hbird_depth_evaluation / eval.py --task depth on the GPU, in a 32-px synthetic depth world (ps = 8, S = 4,
8 training and 4 validation images) with the patch-pooling extractor and tests/tiny_vit.py.

The restatement takes the engine's own neighbour lists (`index.search`) and restates everything after them from tests/depth_refs.py.  With
k = 1 K5's arithmetic is exact in any implementation (one weight, expf(0) / 1 = 1): the aggregated row IS the neighbour's label row and the
prediction is compared bit for bit.  With k > 1 the weights go through the device's expf, which numpy's does not reproduce to the bit, so
there the aggregated rows are held to the project's float64 restatement of K5 within its derived bound (tests/test_aggregate_paths_gpu.py),
and the prediction is the model's on those rows, bit for bit."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import depth_refs as R
import test_depth_gpu as T
from hbird_mi import depth as hdepth
from hbird_mi.data.synthetic_depth import SyntheticDepthDataModule
from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
from tiny_vit import TinyQKVViT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX, PS, S, BS = 32, 8, 4, 4
WORLD = SyntheticDepthDataModule(batch_size=BS, input_size=PX, n_train=8, n_val=4, block=PS, seed=3)
TRAIN, VAL = WORLD.train_dataloader().batches, WORLD.val_dataloader().batches


def _with_empty_patch(batches):
    """The training batches with patch (0, 0) of every batch's first image made a hole: an empty patch, the bounded build's sentinel."""
    out = []
    for x, y in batches:
        y = y.clone()
        y[0, 0, :PS, :PS] = 0.0
        out.append((x, y))
    return out


TRAIN_HOLE = _with_empty_patch(TRAIN)


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x


def _pool_fn(model, imgs):
    return torch.nn.functional.avg_pool2d(imgs, PS).flatten(2).transpose(1, 2).contiguous(), None


@functools.lru_cache(maxsize=None)
def _pool():
    return FeatureExtractorSimple(_Identity(), ftr_extr_fn=_pool_fn, eval_spatial_resolution=S, d_model=3)


@functools.lru_cache(maxsize=None)
def _vit():
    return FeatureExtractor(TinyQKVViT(d=16, ps=PS, seed=3).cuda().eval(), eval_spatial_resolution=S, d_model=16)


def _build(extractor, train=TRAIN, **kw):
    torch.manual_seed(1234)                       # the bounded build's noise comes from torch's CPU generator
    kw.setdefault("n_neighbours", 5)
    return hdepth.HbirdDepthEvaluation(extractor, train, device="cuda", **kw)


def _bank_labels(ev):
    return ev.index.gather_labels(np.arange(ev.index.ntotal))


def _u32(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("which,r,k", [("pool", 1, 1), ("vit", 2, 1), ("vit", 1, 5), ("pool", PS, 5)])
def test_evaluate_equals_the_restatement(cuda_device, which, r, k):
    import test_aggregate_paths_gpu as K5
    ev = _build(_pool() if which == "pool" else _vit(), target_grid=r, n_neighbours=k)
    res = ev.evaluate(VAL, S, return_maps=True)
    labels, norms = _bank_labels(ev), ev.index.copy_norms().cpu().numpy()
    assert labels.shape == (8 * S * S, 2 * r * r) and ev.index.label_denominator == 0
    want_sums, worst = [], 0.0
    for (x, y), got in zip(VAL, res.maps):
        feats = ev._tokens(x)
        B, N, D = feats.shape
        q = feats.reshape(B * N, D).contiguous()
        idx, dist = ev.index.search(q, k)
        idx, dist, qn = idx.cpu().numpy(), dist.cpu().numpy(), q.cpu().numpy()
        agg = ev.aggregate(feats).cpu().numpy().reshape(B * N, -1)
        if k == 1:
            assert np.array_equal(_u32(agg), _u32(labels[idx[:, 0]]))                  # the whole restatement is numpy
        else:
            ref, _, logits = K5.reference(qn, idx, dist, norms, 0, labels, 0, ev.beta, "ip")
            tol = K5.tolerance(qn, idx, dist, norms, 0, logits, k, ev.beta, "ip", float(np.abs(labels).max()))
            assert (np.abs(agg - ref) <= tol[:, None]).all()
        gt = y[:, 0].numpy()
        pred, has = R.predict(agg.reshape(B, N, -1), S, r, PX, PX)
        assert np.array_equal(_u32(got), pred.view(np.uint32))
        sums, _ = R.sums(pred, has, gt)
        want_sums.append(sums)
        lo = sum(len(s) for s in want_sums) - B
        worst = max(worst, T._check_sums(res.sums[lo:lo + B], pred, has, gt, (which, r, k)))
    assert worst <= T.LOG_TOL
    head, pooled, per, n_nopred, empty = R.metrics(res.sums)
    assert set(res) == set(R.METRICS) and all(res[m] == pytest.approx(head[m], rel=1e-12) for m in R.METRICS)
    assert all(res.pooled[m] == pytest.approx(pooled[m], rel=1e-12) for m in R.METRICS)
    assert len(res.per_image) == 4 and res.n_nopred == n_nopred and res.empty_images == empty == []
    assert res.n_pixels == int(np.concatenate(want_sums)[:, 0].sum()) > 0
    again = ev.evaluate(VAL, S)
    assert again.maps is None and np.array_equal(again.sums.view(np.int64), res.sums.view(np.int64))      # the same bits again
    ev.index.close()


def test_planted_identity(cuda_device):
    """r = ps, h = S ps, the validation set IS the training set, k = 1: every patch finds itself, and every valid pixel its own depth.
    (Pixel noise of unit variance on the images, so that no two patches of one texture have tokens a rounding apart.)"""
    g = torch.Generator().manual_seed(11)
    train = [(x + torch.randn(x.shape, generator=g), y) for x, y in TRAIN]
    ev = _build(_vit(), train=train, target_grid=PS, n_neighbours=1)
    res = ev.evaluate(train, S, return_maps=True)
    n_valid = 0
    for (x, y), pred in zip(train, res.maps):
        gt = y[:, 0].numpy()
        ok = R.valid(gt)
        n_valid += int(ok.sum())
        assert np.array_equal(_u32(pred)[ok], _u32(gt)[ok])
        assert np.isnan(pred.numpy()[~ok]).all()                                       # a hole in the bank is a pixel without a prediction
    assert res["rmse"] == 0.0 and res["d1"] == 1.0 and res["abs_rel"] == 0.0 and res.pooled["rmse"] == 0.0
    assert res.n_nopred == 0 and res.n_pixels == n_valid and res.empty_images == []
    ev.index.close()


def test_retrieval_beats_the_training_mean(cuda_device):
    ev = _build(_pool(), target_grid=1, n_neighbours=5)
    res = ev.evaluate(VAL, S)
    train = np.concatenate([y[:, 0].numpy() for _, y in TRAIN])
    mean = float(train[R.valid(train)].astype(np.float64).mean())
    base = []
    for _, y in VAL:
        for g in y[:, 0].numpy():
            ok = R.valid(g)
            base.append(float(np.sqrt(((mean - g[ok].astype(np.float64)) ** 2).mean())))
    print(f"retrieval rmse {res['rmse']:.4f}, training-mean rmse {np.mean(base):.4f}")
    assert res["rmse"] < float(np.mean(base))                                          # colour determines depth in this world
    assert 0.0 < res["d1"] <= 1.0 and res.n_pixels > 0
    ev.index.close()


def test_bounded_memory_replays_the_cpu_random_stream(cuda_device):
    K, r = 5, 2
    ev = _build(_pool(), train=TRAIN_HOLE, target_grid=r, memory_size=8 * K, dataset_size=8)
    assert ev.num_sampled_features == K and ev.index.ntotal == 8 * K
    torch.manual_seed(1234)
    want_rows = []
    for (x, y), got in zip(TRAIN_HOLE, ev.sampled_patches):
        rows, nonempty = R.target_rows(y[:, 0].numpy(), PS, r)
        ne = nonempty.reshape(BS, S * S)
        assert ne[0, 0] == 0 and ne.sum() == BS * S * S - 1
        noise = torch.rand(int(ne.sum())).numpy()                                      # one draw per non-empty patch, in batch order
        scores = np.full((BS, S * S), np.float32(1e6))
        scores[ne != 0] = np.float32(1.0) * noise
        pick = np.argsort(scores, axis=1, kind="stable")[:, :K]                        # K smallest, ascending, ties to the lower patch
        assert np.array_equal(got.numpy(), pick)
        assert not (pick[0] == 0).any()                                                # the empty patch is never sampled
        want_rows.append(rows.reshape(BS, S * S, -1)[np.arange(BS)[:, None], pick].reshape(BS * K, -1))
    assert np.array_equal(_u32(_bank_labels(ev)), _u32(np.concatenate(want_rows)))
    ev.index.close()


def test_from_index_on_a_memory_view_is_the_bank_built_at_that_size(cuda_device):
    big = _build(_pool(), train=TRAIN_HOLE, target_grid=2, memory_size=8 * 6, dataset_size=8)
    view = big.memory_view(8 * 2)
    direct = _build(_pool(), train=TRAIN_HOLE, target_grid=2, memory_size=8 * 2, dataset_size=8)
    assert view.index.ntotal == direct.index.ntotal == 16
    ids = np.arange(16)
    assert np.array_equal(_u32(view.index.reconstruct(ids)), _u32(direct.index.reconstruct(ids)))
    assert np.array_equal(_u32(_bank_labels(view)), _u32(_bank_labels(direct)))
    a, b = view.evaluate(VAL, S), direct.evaluate(VAL, S)
    assert dict(a) == dict(b) and np.array_equal(a.sums.view(np.int64), b.sums.view(np.int64)) and a.pooled == b.pooled
    with pytest.raises(ValueError, match="memory_view"):
        big.memory_view(8 * 7)
    with pytest.raises(ValueError, match="memory_view"):
        _build(_pool()).memory_view(16)
    # a hand-made index works the same way; anything but a HipFlatIndex is refused
    hand = hdepth.HbirdDepthEvaluation.from_index(_pool(), direct.index, n_neighbours=5, target_grid=2)
    assert dict(hand.evaluate(VAL, S)) == dict(b)
    with pytest.raises(ValueError, match="HipFlatIndex"):
        hdepth.HbirdDepthEvaluation.from_index(_pool(), object())
    for ev in (big, view, direct):
        ev.index.close()


def test_hbird_depth_evaluation_and_the_cli(cuda_device, tmp_path):
    kw = dict(d_model=3, patch_size=8, dataset_name="synthetic-depth", data_dir="", batch_size=8, input_size=64, device="cuda", n_neighbours=5,
              ftr_extr_fn=lambda m, x: (torch.nn.functional.avg_pool2d(x, 8).flatten(2).transpose(1, 2).contiguous(), None))
    res = hdepth.hbird_depth_evaluation(_Identity(), target_grid=2, **kw)
    assert isinstance(res, hdepth.DepthMetrics) and set(res) == set(R.METRICS) and len(res.per_image) == 16
    assert 0.0 < res["rmse"] < 10.0 and 0.0 < res["d1"] <= 1.0 and hdepth.last_run_info["bank_rows"] == 32 * 64
    for clash in (dict(frame_size=(128, 128)), dict(window_stride=32), dict(grid_k=[3]), dict(grid_beta=[0.1]), dict(bootstrap=10),
                  dict(leave_one_out=True), dict(memory_sizes=[64])):
        with pytest.raises(ValueError, match=next(iter(clash))):
            hdepth.hbird_depth_evaluation(_Identity(), **kw, **clash)
    spec = importlib.util.spec_from_file_location("hb_cli_depth", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    cli.main(["--task", "depth", "--dataset-name", "synthetic-depth", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64",
              "--batch-size", "8", "--device", "cuda", "--n-neighbours", "5", "--target-grid", "2", "--min-depth", "0.001", "--max-depth", "10",
              "--out", out, "--log-level", "WARNING"])
    js = json.load(open(out))
    assert js["task"] == "depth" and all(js[m] == res[m] for m in R.METRICS) and js["pooled"] == res.pooled
    assert js["n_nopred"] == res.n_nopred and js["empty_images"] == [] and js["n_images"] == 16 and js["target_grid"] == 2 and "miou" not in js
