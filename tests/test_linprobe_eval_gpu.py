"""HbirdEvaluation.evaluate_linear_probe / hbird_evaluation(linear_probe=True) / eval.py --linear-probe on the GPU, in the 64-px, C = 5, 24-image
world of tests/test_memory_views_gpu.py with tests/tiny_vit.py.  The restatement takes the engine's fitted Wb read back, then parts tested
elsewhere: the validation tokens normalised, the chain logits of tests/linprobe_refs.py, oracle.upsample_argmax (K6 evaluates its formula in
its order of operations: the class maps are equal), oracle.confusion_matrix and the identity matching -- the confusion matrices must be equal
as integers and the mIoU as a float."""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import linprobe_refs as R
import oracle
from hbird_mi import ops
from hbird_mi.utils.eval_metrics import PredsmIoU
from test_memory_views_gpu import C, D, S, VAL, _build, _built, _synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2 = 1e-2


def test_linear_probe_evaluation_equals_the_restatement(cuda_device):
    ev = _built(None)
    got = ev.evaluate_linear_probe(VAL, S, l2=L2)
    info = ev.last_linear_probe
    assert isinstance(got, float) and 0.0 < got <= 1.0
    assert info["state"] in ("converged", "stalled") and info["rows_used"] == ev.index.ntotal and info["rows_skipped"] == 0
    assert len(info["history"]) == info["n_iter"] + 1 and info["history"][-1]["loss"] == info["loss"] < info["history"][0]["loss"]
    Wb = info["Wb"].numpy()
    assert Wb.shape == (C, D + 1) and Wb.dtype == np.float32
    conf = np.zeros((C, C), dtype=np.int64)
    m = PredsmIoU(C, C, ignore_index=255, device=ev.gpu_device, store_reordered_preds=False)
    mo = oracle.PredsMIoUOracle(C, C, 255)
    with torch.no_grad():
        for x, y in VAL:
            yi = (y * 255).long()
            feats = ev._tokens(x)
            B, N, _ = feats.shape
            rows = ops.normalize_rows(feats.reshape(B * N, D).contiguous()).cpu().numpy()
            z, skip = R.chain_logits(rows, Wb)
            assert not skip.any()
            pred = oracle.upsample_argmax(z.reshape(B, N, C), S, yi.shape[-2], yi.shape[-1])
            conf += oracle.confusion_matrix(yi.numpy(), pred, C, C, 255)
            m.update(yi.to(ev.gpu_device), torch.from_numpy(pred).to(ev.gpu_device))
            mo.update(yi.numpy(), pred)
    assert info["confusion"].dtype == torch.int64 and np.array_equal(info["confusion"].numpy(), conf)
    assert int(conf.sum()) == sum(int(y.numel()) for _, y in VAL)                          # (no 255 in this world: every pixel is counted)
    assert got == m.compute(is_global_zero=True, return_reordered=False, linear_probe=True)[0]   # the identity matching: the same float
    assert abs(got - mo.compute(linear_probe=True)[0]) < 1e-12
    # the fit is the same fit again (this world's masks are random cells: there is little to learn, the figure is near chance)
    assert ev.evaluate_linear_probe(VAL, S, l2=L2) == got and torch.equal(ev.last_linear_probe["Wb"], info["Wb"])
    # a probe of a memory view is a probe of an ordinary index
    view = ev.memory_view(images=list(range(12)))
    half = view.evaluate_linear_probe(VAL, S, l2=L2)
    assert 0.0 < half <= 1.0 and view.last_linear_probe["rows_used"] == view.index.ntotal == ev.index.ntotal // 2


def test_linear_probe_evaluation_refusals(cuda_device):
    ev = _built(None)
    with pytest.raises(ValueError, match="window"):
        ev.evaluate_linear_probe(VAL, S, window=(64, 64))
    with pytest.raises(ValueError, match="return_knn_details"):
        ev.evaluate_linear_probe(VAL, S, return_knn_details=True)
    ranked = copy.copy(ev)
    ranked.world, ranked.rank = 2, 0
    sharded = copy.copy(ev)
    sharded.sharded = True
    for bad in (ranked, sharded):
        with pytest.raises(ValueError, match="torch.distributed"):
            bad.evaluate_linear_probe(VAL, S)
        with pytest.raises(ValueError, match="torch.distributed"):
            bad.linear_probe()
    for bad in (dict(l2=-1.0), dict(gtol=float("nan")), dict(max_iter=-1), dict(max_iter=1.5)):
        with pytest.raises(ValueError):
            ev.evaluate_linear_probe(VAL, S, **bad)
    multi = _build(None, gpu_ids=[0, 0], idx_shard=True)
    assert type(multi.index).__name__ == "HipMultiIndex"
    with pytest.raises(ValueError, match="HipMultiIndex"):
        multi.evaluate_linear_probe(VAL, S)
    multi.index.close()


def test_hbird_evaluation_and_cli_linear_probe(cuda_device, tmp_path):
    """The synthetic data module: 32 training images of 64 patches, 3-dimensional pooled tokens."""
    from hbird_mi import hbird_eval as he
    res = _synthetic(linear_probe=True, linear_probe_l2=L2)
    fit = dict(he.last_run_info["linear_probe_fit"])
    assert isinstance(res, float) and 0.0 < res <= 1.0
    assert set(fit) == {"state", "iterations", "loss", "rows_used", "rows_skipped"} and fit["rows_used"] == 32 * 64 and fit["rows_skipped"] == 0
    assert _synthetic(linear_probe=True, linear_probe_l2=L2, linear_probe_gtol=1e-5, linear_probe_iters=200) == res
    for clash in (dict(grid_k=[3]), dict(grid_beta=[0.1]), dict(memory_size=640, memory_sizes=[160]), dict(leave_one_out=True), dict(bootstrap=10),
                  dict(return_knn_details=True), dict(frame_size=(128, 128)), dict(overclustering=[4])):
        with pytest.raises(ValueError, match="linear_probe is not available with"):
            _synthetic(linear_probe=True, **clash)
    spec = importlib.util.spec_from_file_location("hb_cli_probe", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    cli.main(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64", "--batch-size", "8",
              "--device", "cuda", "--nn-method", "hip", "--linear-probe", "--linear-probe-l2", str(L2), "--linear-probe-gtol", "1e-5",
              "--linear-probe-iters", "200", "--out", out, "--log-level", "WARNING"])
    js = json.load(open(out))
    assert 0.0 < js["miou_linear_probe"] <= 1.0 and js["miou"] == js["miou_linear_probe"]
    assert set(js["linear_probe_fit"]) == set(fit) and js["linear_probe_fit"]["rows_used"] == 32 * 64
    assert js["linear_probe_fit"]["state"] in ("converged", "stalled", "max_iter") and js["linear_probe_fit"]["iterations"] >= 1
    assert "miou_overclustering" not in js and "miou_grid" not in js
