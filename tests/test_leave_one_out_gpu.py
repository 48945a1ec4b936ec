"""HbirdEvaluation.evaluate_leave_one_out / hbird_evaluation(leave_one_out=True) / eval.py --leave-one-out on the GPU: a synthetic data module
with 6 training images of 32 px (S = 4: 16 patches each) and tests/tiny_vit.py.  The leave-one-out mIoU of every (k, beta) must be, float for
float, the mIoU accumulated image by image from `memory_view(rows=all rows but that image's)` with `search_aggregate_grid`."""
import copy
import functools
import importlib.util
import json
import os

import pytest
import torch

from hbird_mi.data.synthetic import SyntheticSegDataModule
from hbird_mi.hbird_eval import HbirdEvaluation, hbird_evaluation
from hbird_mi.models import FeatureExtractor
from hbird_mi.utils.eval_metrics import PredsmIoU
from test_memory_views_gpu import _PoolViT, _pool_fn
from tiny_vit import TinyQKVViT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, PX, PS, D, N_IMG, BATCH = 5, 32, 8, 16, 6, 4
S = PX // PS
N = S * S
KS, BETAS = (3, 10, 40), (0.02, 0.1)
DATA = SyntheticSegDataModule(batch_size=BATCH, input_size=PX, num_classes=C, n_train=N_IMG, n_val=4, seed=5)
TRAIN = DATA.train_dataloader()          # batches of 4 + 2 images, the same in every pass (shuffle=False)


@functools.lru_cache(maxsize=None)
def _extractor():
    return FeatureExtractor(TinyQKVViT(d=D, ps=PS, seed=3).cuda().eval(), eval_spatial_resolution=S, d_model=D)


@functools.lru_cache(maxsize=None)
def _built(memory_size, aug):
    torch.manual_seed(1234)
    return HbirdEvaluation(_extractor(), TRAIN, num_classes=C, n_neighbours=10, augmentation_epoch=aug, device="cuda", nn_method="hip",
                           nn_params={}, memory_size=memory_size, dataset_size=N_IMG)


def _by_views(ev, ks, betas, max_images=None, ignore_index=255):
    """The definition: image by image, the bank without that image's rows (a memory_view), one search_aggregate_grid, one metric per (k, beta)."""
    groups = ev.row_groups()
    configs = [(k, b) for k in ks for b in betas]
    metrics = [PredsmIoU(C, C, ignore_index=ignore_index, device=ev.gpu_device, store_reordered_preds=False) for _ in configs]
    seen = 0
    with torch.no_grad():
        for x, y in TRAIN:
            feats = ev._tokens(x.cuda())              # the batch's tokens, as the evaluator computes them
            y = (y.cuda() * 255).long()
            for b in range(x.shape[0]):
                if max_images is not None and seen >= max_images:
                    break
                view = ev.memory_view(rows=torch.nonzero(groups != seen).reshape(-1))
                lh = view.index.search_aggregate_grid(feats[b].contiguous(), ks, betas)
                for i, m in enumerate(metrics):
                    m.update_from_label_hat(y[b:b + 1], lh[i].view(1, N, -1), S)
                view.index.close()
                seen += 1
    return {cfg: m.compute(is_global_zero=True, sync_distributed=False, return_reordered=False)[0] for cfg, m in zip(configs, metrics)}


def test_row_groups_follow_the_build_geometry(cuda_device):
    ev = _built(None, 2)
    g = ev.row_groups()
    assert ev._dataset_images == N_IMG and ev.index.ntotal == 2 * N_IMG * N and g.dtype == torch.int32
    assert g.tolist() == [i for _ in range(2) for i in range(N_IMG) for _ in range(N)]          # (epoch, image) blocks: the groups interleave
    small = _built(N_IMG * 9, 1)
    assert small.row_groups().tolist() == [i for i in range(N_IMG) for _ in range(9)]
    view = small.memory_view(memory_size=N_IMG * 5)
    assert view.row_groups().tolist() == [i for i in range(N_IMG) for _ in range(5)]
    assert view.index.row_groups.cpu().tolist() == view.row_groups().tolist()                    # the view's index carries them
    sub = ev.memory_view(images=[1, 4])
    assert sub.row_groups().tolist() == [i for _ in range(2) for i in (1, 4) for _ in range(N)]  # the images keep their numbers
    sub.index.close(); view.index.close()


def test_leave_one_out_equals_the_views_image_by_image_with_interleaved_groups(cuda_device):
    ev = _built(None, 2)
    got = ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS)
    assert list(got) == [(k, b) for k in KS for b in BETAS] and all(isinstance(v, float) and 0.0 < v <= 1.0 for v in got.values())
    assert got == _by_views(ev, KS, BETAS)
    assert ev.index.last_exclusion()["gmax"] == 2 * N
    # without the exclusion every query finds its own patch (the bank holds the training images twice): another number
    plain = ev.evaluate_grid(TRAIN, S, n_neighbours=KS, betas=BETAS)
    assert plain != got and plain[(3, 0.02)] > got[(3, 0.02)]
    # the defaults are the evaluator's own n_neighbours and beta
    assert ev.evaluate_leave_one_out(TRAIN, S) == {(10, 0.02): got[(10, 0.02)]}


def test_leave_one_out_on_a_bounded_bank_max_images_and_views(cuda_device):
    big = _built(N_IMG * 12, 1)
    assert big.num_sampled_features == 12
    got = big.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS)
    assert got == _by_views(big, KS, BETAS)
    # max_images stops the pass early, also inside a batch
    for n in (1, 4, 5):
        assert big.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS, max_images=n) == _by_views(big, KS, BETAS, max_images=n), n
    assert big.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS, max_images=100) == got
    # views: the memory sizes of one bank out of one pass
    small = big.memory_view(memory_size=N_IMG * 5)
    views = {"5of12": small, "12of12": big}
    both = big.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS, views=views)
    assert list(both) == [(key, k, b) for key in views for k in KS for b in BETAS]
    own = small.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS)
    assert own == _by_views(small, KS, BETAS)
    for (k, b), v in own.items():
        assert both[("5of12", k, b)] == v and both[("12of12", k, b)] == got[(k, b)]
    assert both[("5of12", 10, 0.02)] != both[("12of12", 10, 0.02)]
    small.index.close()


def test_leave_one_out_refusals(cuda_device):
    ev = _built(None, 2)
    with pytest.raises(ValueError, match="window"):
        ev.evaluate_leave_one_out(TRAIN, S, window=(32, 32))
    with pytest.raises(ValueError, match="more than the 6 images"):
        ev.evaluate_leave_one_out(list(TRAIN) + list(TRAIN)[:1], S)
    with pytest.raises(ValueError, match="max_images"):
        ev.evaluate_leave_one_out(TRAIN, S, max_images=0)
    with pytest.raises(ValueError):
        ev.evaluate_leave_one_out(TRAIN, S, views={})
    ranked = copy.copy(ev)
    ranked.world, ranked.rank = 2, 0
    with pytest.raises(ValueError, match="torch.distributed"):
        ranked.evaluate_leave_one_out(TRAIN, S)
    with pytest.raises(ValueError, match="torch.distributed"):
        ev.evaluate_leave_one_out(TRAIN, S, views={"a": ranked})
    sharded = copy.copy(ev)
    sharded.sharded = True
    with pytest.raises(ValueError, match="torch.distributed"):
        sharded.evaluate_leave_one_out(TRAIN, S)
    torch.manual_seed(1234)
    multi = HbirdEvaluation(_extractor(), TRAIN, num_classes=C, n_neighbours=10, augmentation_epoch=1, device="cuda", nn_method="hip",
                            nn_params={"gpu_ids": [0, 0]}, memory_size=None, dataset_size=N_IMG)
    assert type(multi.index).__name__ == "HipMultiIndex"
    with pytest.raises(ValueError, match="several GPUs"):
        multi.evaluate_leave_one_out(TRAIN, S)
    multi.index.close()
    # a bank without geometry has no row groups until they are given
    bare = HbirdEvaluation.from_index(_extractor(), ev.index, C, 10, device="cuda")
    with pytest.raises(ValueError, match="set_row_groups"):
        bare.row_groups()
    with pytest.raises(ValueError, match="set_row_groups"):
        bare.evaluate_leave_one_out(TRAIN, S)
    with pytest.raises(ValueError, match="rows"):
        bare.set_row_groups(torch.zeros(5, dtype=torch.int64))
    bare.set_row_groups(ev.row_groups())
    assert bare.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS) == ev.evaluate_leave_one_out(TRAIN, S, n_neighbours=KS, betas=BETAS)


def _synthetic(**kw):
    """The project's synthetic data module at 6 training images (32 x 0.1875), 32 px, pooled-pixel tokens."""
    torch.manual_seed(77)
    return hbird_evaluation(_PoolViT(), d_model=3, patch_size=8, dataset_name="synthetic*0.1875", data_dir="", batch_size=4, input_size=32,
                            device="cuda", n_neighbours=5, nn_method="hip", ftr_extr_fn=_pool_fn, **kw)


def test_hbird_evaluation_leave_one_out(cuda_device):
    plain = _synthetic(leave_one_out=True)
    assert isinstance(plain, float) and 0.0 < plain <= 1.0 and plain != _synthetic()
    grid = _synthetic(leave_one_out=True, grid_k=[3, 5], grid_beta=[0.02, 0.1])
    assert list(grid) == [(3, 0.02), (3, 0.1), (5, 0.02), (5, 0.1)] and grid[(5, 0.02)] == plain
    few = _synthetic(leave_one_out=True, leave_one_out_images=2, grid_k=[3, 5])
    assert list(few) == [(3, 0.02), (5, 0.02)] and few != {k: grid[k] for k in few}
    sweep = _synthetic(leave_one_out=True, memory_size=6 * 12, memory_sizes=[6 * 5, 6 * 12, 10 ** 6])
    assert list(sweep) == [30, 72] and all(isinstance(v, float) for v in sweep.values())
    assert sweep[72] == _synthetic(leave_one_out=True, memory_size=72)
    gsweep = _synthetic(leave_one_out=True, memory_size=72, memory_sizes=[30, 72], grid_k=[3, 5])
    assert list(gsweep) == [30, 72] and gsweep[72][(5, 0.02)] == sweep[72] and gsweep[30][(5, 0.02)] == sweep[30]
    with pytest.raises(ValueError, match="return_knn_details"):
        _synthetic(leave_one_out=True, return_knn_details=True)
    with pytest.raises(ValueError, match="sliding windows"):
        _synthetic(leave_one_out=True, frame_size=(64, 64))


def test_cli_leave_one_out(cuda_device, tmp_path):
    spec = importlib.util.spec_from_file_location("hb_cli_loo", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8"])
    assert a.leave_one_out is False and a.leave_one_out_images is None
    out = str(tmp_path / "res.json")
    base = ["--dataset-name", "synthetic*0.1875", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "32", "--batch-size", "4",
            "--device", "cuda", "--nn-method", "hip", "--n-neighbours", "5", "--out", out, "--log-level", "WARNING"]
    cli.main(base + ["--leave-one-out", "--leave-one-out-images", "4", "--grid-k", "3", "5"])
    res = json.load(open(out))
    assert res["leave_one_out"] is True and set(res["miou_grid"]) == {"k=3,beta=0.02", "k=5,beta=0.02"}
    assert all(0.0 < v <= 1.0 for v in res["miou_grid"].values()) and res["miou"] == res["miou_grid"]["k=5,beta=0.02"]
    cli.main(base + ["--leave-one-out"])
    one = json.load(open(out))
    assert one["leave_one_out"] is True and "miou_grid" not in one and 0.0 < one["miou"] <= 1.0
    cli.main(base)
    assert "leave_one_out" not in json.load(open(out))
