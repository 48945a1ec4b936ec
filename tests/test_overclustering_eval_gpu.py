"""HbirdEvaluation.evaluate_overclustering / hbird_evaluation(overclustering=) / eval.py --overclustering on the GPU, in the 64-px, C = 5,
24-image world of tests/test_memory_views_gpu.py with K in {C, 2 C + 1}: the pass must equal a torch restatement built from parts tested
elsewhere -- the same tokens normalised, KMeansResult.assign, F.one_hot, F.interpolate(bilinear), argmax, PredsmIoU.update, compute with the
mode named.  The upsampling factor is 8 and the inputs are one-hot, so every bilinear weight and product is exact in fp32 whatever the order
of the arithmetic: the confusion matrices must be equal as integers and the mIoU as a float."""
import copy
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

from hbird_mi import ops
from hbird_mi.utils.eval_metrics import PredsmIoU
from test_memory_views_gpu import C, S, VAL, _build, _built, _synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, SEED, ITERS = (C, 2 * C + 1), 3, 8
MODES = {"hungarian": dict(many_to_one=False, precision_based=False), "many_to_one": dict(many_to_one=True, precision_based=False),
         "many_to_one_precision": dict(many_to_one=True, precision_based=True)}


def _restated(ev, K):
    """The confusion matrix [C, K] of the restatement, as a PredsmIoU."""
    fit = ev.kmeans(K, seed=SEED, max_iter=ITERS)
    m = PredsmIoU(K, C, ignore_index=255, device=ev.gpu_device, store_reordered_preds=False)
    with torch.no_grad():
        for x, y in VAL:
            y = (y.to(ev.gpu_device) * 255).long()
            feats = ev._tokens(x)
            B, N, D = feats.shape
            ids = fit.assign(ops.normalize_rows(feats.reshape(B * N, D).contiguous()))
            one_hot = F.one_hot(ids.clamp(min=0), K).float() * (ids >= 0).unsqueeze(1)
            up = F.interpolate(one_hot.view(B, S, S, K).permute(0, 3, 1, 2), size=tuple(y.shape[-2:]), mode="bilinear")
            m.update(y, up.argmax(dim=1, keepdim=True))
    fit.close()
    return m


def test_overclustering_equals_the_torch_restatement(cuda_device):
    ev = _built(None)
    got = ev.evaluate_overclustering(VAL, S, list(KS), seed=SEED, max_iter=ITERS)
    assert list(got) == list(KS) and all(isinstance(v, float) and 0.0 < v <= 1.0 for v in got.values())
    assert [ev.last_overclustering[K]["matching"] for K in KS] == ["hungarian", "many_to_one_precision"]      # K = C, K > C
    details = dict(ev.last_overclustering)
    for K in KS:
        m = _restated(ev, K)
        conf = details[K]["confusion"]
        assert conf.dtype == torch.int64 and tuple(conf.shape) == (C, K) and torch.equal(conf, m._conf_mat.cpu())
        assert int(conf.sum()) == sum(int(y.numel()) for _, y in VAL)                  # (no 255 in this world: every pixel is counted)
        assert got[K] == m.compute(is_global_zero=True, return_reordered=False, **MODES[details[K]["matching"]])[0]
        # matching= overrides the choice; the counts do not change
        for mode, kw in MODES.items():
            forced = ev.evaluate_overclustering(VAL, S, K, seed=SEED, max_iter=ITERS, matching=mode)
            assert list(forced) == [K] and ev.last_overclustering[K]["matching"] == mode
            assert torch.equal(ev.last_overclustering[K]["confusion"], conf)
            assert forced[K] == m.compute(is_global_zero=True, return_reordered=False, **kw)[0], (K, mode)
        assert details[K]["n_iter"] >= 1 and len(details[K]["history"]) == details[K]["n_iter"]
    # any order, repeats: the same dict
    assert ev.evaluate_overclustering(VAL, S, [KS[1], KS[0], KS[1]], seed=SEED, max_iter=ITERS) == got
    # the two protocols give different figures in this world
    assert got[KS[1]] != got[KS[0]]


def test_overclustering_refusals(cuda_device):
    ev = _built(None)
    with pytest.raises(ValueError, match="window"):
        ev.evaluate_overclustering(VAL, S, C, window=(64, 64))
    with pytest.raises(ValueError, match="return_knn_details"):
        ev.evaluate_overclustering(VAL, S, C, return_knn_details=True)
    ranked = copy.copy(ev)
    ranked.world, ranked.rank = 2, 0
    sharded = copy.copy(ev)
    sharded.sharded = True
    for bad in (ranked, sharded):
        with pytest.raises(ValueError, match="torch.distributed"):
            bad.evaluate_overclustering(VAL, S, C)
        with pytest.raises(ValueError, match="torch.distributed"):
            bad.kmeans(C)
    for bad in (dict(n_clusters=[]), dict(n_clusters=0), dict(n_clusters=[2049]), dict(n_clusters=[1.5]), dict(n_clusters=ev.index.ntotal + 1),
                dict(n_clusters=C, matching="best"), dict(n_clusters=C, max_iter=0)):
        with pytest.raises(ValueError):
            ev.evaluate_overclustering(VAL, S, **bad)
    multi = _build(None, gpu_ids=[0, 0], idx_shard=True)
    assert type(multi.index).__name__ == "HipMultiIndex"
    with pytest.raises(ValueError, match="HipMultiIndex"):
        multi.evaluate_overclustering(VAL, S, C)
    multi.index.close()


def test_hbird_evaluation_overclustering(cuda_device):
    """The synthetic data module: 32 training images of 64 patches, 3-dimensional pooled tokens."""
    res = _synthetic(overclustering=[9, 4], overclustering_seed=1, overclustering_iters=5)
    assert list(res) == [4, 9] and all(isinstance(v, float) and 0.0 < v <= 1.0 for v in res.values())
    assert _synthetic(overclustering=[4], overclustering_seed=1, overclustering_iters=5) == {4: res[4]}
    for clash in (dict(grid_k=[3]), dict(grid_beta=[0.1]), dict(memory_size=640, memory_sizes=[160]), dict(leave_one_out=True), dict(bootstrap=10),
                  dict(return_knn_details=True), dict(frame_size=(128, 128))):
        with pytest.raises(ValueError, match="overclustering is not available with"):
            _synthetic(overclustering=[4], **clash)
    with pytest.raises(ValueError):
        _synthetic(overclustering=[0])


def test_cli_overclustering(cuda_device, tmp_path):
    spec = importlib.util.spec_from_file_location("hb_cli_clusters", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    cli.main(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64", "--batch-size", "8",
              "--device", "cuda", "--nn-method", "hip", "--overclustering", "9", "4", "--overclustering-seed", "1", "--overclustering-iters", "5",
              "--out", out, "--log-level", "WARNING"])
    res = json.load(open(out))
    assert list(res["miou_overclustering"]) == ["clusters=4", "clusters=9"]
    assert all(0.0 < v <= 1.0 for v in res["miou_overclustering"].values()) and res["miou"] == res["miou_overclustering"]["clusters=4"]
    assert "miou_grid" not in res and "miou_by_memory_size" not in res
