"""HbirdEvaluation at n_neighbours = 600 against fixture G11: the reference's own HbirdEvaluation on the same world
(tests/golden/gen_golden_bigk.py; 1,280 bank rows, 512 queries, 5 classes -- up to a tenth of a query's softmax weight lies beyond
rank 256, so an engine that stops there misses half of label_hat by more than the 5e-5 allowed below)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import ReplayExtractor
from hbird_mi.hbird_eval import HbirdEvaluation

pytestmark = pytest.mark.gpu


def g11_case(golden_dir):
    g = np.load(f"{golden_dir}/g11_bigk_evaluate.npz")
    C, D, H, ps, nb, B, k, ign = g["cfg"].tolist()
    as_y = lambda m: torch.from_numpy(m.astype(np.float32) / np.float32(255.0))          # ToTensor's mask / 255, as the generator's loaders
    train = [(torch.zeros((B, 3, H, H)), as_y(g[f"train_mask_{i}"])) for i in range(nb)]
    val = [(torch.zeros((B, 3, H, H)), as_y(g[f"val_mask_{i}"])) for i in range(2)]
    return dict(g=g, C=C, D=D, H=H, S=H // ps, B=B, k=k, ign=ign, train=train, val=val,
                tr_tok=[g[f"train_tok_{i}"] for i in range(nb)], va_tok=[g[f"val_tok_{i}"] for i in range(2)])


def evaluator(c, evaluations=1, k=None, **nn_params):
    torch.set_rng_state(torch.from_numpy(c["g"]["rng_state"]))
    method = nn_params.pop("nn_method", "hip")
    return HbirdEvaluation(ReplayExtractor(c["tr_tok"] + c["va_tok"] * evaluations, c["S"], c["D"]), c["train"], num_classes=c["C"],
                           n_neighbours=c["k"] if k is None else k, device="cuda:0", nn_method=method, nn_params=nn_params)


@pytest.mark.parametrize("nn_method", ["hip", "faiss"])
def test_evaluate_at_600_neighbours_matches_the_reference(cuda_device, golden_dir, nn_method):
    c = g11_case(golden_dir)
    g = c["g"]
    assert c["k"] == 600
    ev = evaluator(c, evaluations=2, nn_method=nn_method)
    assert np.array_equal(ev.label_memory.numpy(), g["label_memory"])
    assert np.abs(ev.feature_memory.numpy() - g["feature_memory"]).max() <= 2.5e-7
    j_fused = ev.evaluate(c["val"], c["S"], ignore_index=c["ign"])                               # search_aggregate_bigk
    jac, det = ev.evaluate(c["val"], c["S"], return_knn_details=True, ignore_index=c["ign"])    # search, then aggregate_bigk
    print(f"G11 {nn_method}: jac {jac:.5f} (fused {j_fused:.5f}), reference {float(g['jac']):.5f}")
    assert j_fused == jac
    assert abs(jac - float(g["jac"])) < 1e-4, (jac, float(g["jac"]))
    lh = det["knns_ca_labels"].numpy()
    assert lh.shape == g["knns_ca_labels"].shape
    diff = np.abs(lh - g["knns_ca_labels"])
    print(f"G11 {nn_method}: label_hat max |diff| {diff.max():.2e}, share within 5e-5 {(diff < 5e-5).mean():.5f}")
    assert (diff < 5e-5).mean() > 0.999, (diff < 5e-5).mean()
    assert det["knns"].shape == (2 * c["B"], c["S"] ** 2, c["k"], c["D"]) and det["knns_labels"].shape == (2 * c["B"], c["S"] ** 2, c["k"], c["C"])


def test_neighbour_count_limits(cuda_device, golden_dir):
    c = g11_case(golden_dir)
    for k in (0, 2049):
        with pytest.raises(ValueError, match="2048"):
            evaluator(c, k=k)
    ev = evaluator(c, k=2048)                       # more neighbours than bank rows: the tail of every list is missing and carries no weight
    j_all = ev.evaluate(c["val"], c["S"], ignore_index=c["ign"])
    ev = evaluator(c, k=1280)                       # exactly every row
    assert ev.evaluate(c["val"], c["S"], ignore_index=c["ign"]) == j_all
    with pytest.raises(ValueError, match="2048"):
        HbirdEvaluation.from_index(ev.feature_extractor, ev.index, c["C"], n_neighbours=2049)
    again = HbirdEvaluation.from_index(ReplayExtractor(c["va_tok"], c["S"], c["D"]), ev.index, c["C"], n_neighbours=600, device="cuda:0")
    assert abs(again.evaluate(c["val"], c["S"], ignore_index=c["ign"]) - float(c["g"]["jac"])) < 1e-4


def test_windowed_evaluation_at_600_neighbours(cuda_device, golden_dir):
    """The sliding-window path (`frame_size` of hbird_evaluation -> evaluate(window=...)): one window that covers the frame goes through
    _windowed_cluster_map and gives the plain evaluation's mIoU."""
    c = g11_case(golden_dir)
    ev = evaluator(c, evaluations=2)
    plain = ev.evaluate(c["val"], c["S"], ignore_index=c["ign"])
    tiled = ev.evaluate(c["val"], c["S"], ignore_index=c["ign"], window=(c["H"], c["H"]))
    assert tiled == plain and abs(plain - float(c["g"]["jac"])) < 1e-4      # (equal, as test_one_window_per_frame_equals_the_plain_path holds for k <= 256)


@pytest.mark.parametrize("shard,extra", [(True, {}), (True, {"label_shard": True}), (False, {})], ids=["shards", "shards-label_shard", "replicas"])
def test_several_indices_in_one_process_at_600_neighbours(cuda_device, golden_dir, shard, extra):
    """gpu_ids = [0, 0, 0]: three row shards or three replicas on the one GPU, merge and aggregation (aggregate_bigk) on the home handle
    -- the single index's bank, neighbours, label_hat bits and mIoU, as
    test_eval_gpu.py::test_evaluator_drives_several_gpus_in_one_process claims for k <= 256."""
    c = g11_case(golden_dir)
    outs = []
    for ids in ([0], [0, 0, 0]):
        ev = evaluator(c, evaluations=2, nn_method="faiss", gpu_ids=ids, idx_shard=shard, **extra)
        if len(ids) > 1:
            rows = ev.index.shard_rows
            assert len(rows) == 3 and ((sum(rows) == 1280 and min(rows) > 0) if shard else rows == [1280] * 3), rows
        j_fused = ev.evaluate(c["val"], c["S"], ignore_index=c["ign"])
        jac, det = ev.evaluate(c["val"], c["S"], return_knn_details=True, ignore_index=c["ign"])
        assert j_fused == jac
        outs.append((ev.feature_memory, ev.label_memory, jac, det))
    (f1, l1, j1, d1), (f3, l3, j3, d3) = outs
    assert torch.equal(f1, f3) and torch.equal(l1, l3) and j1 == j3
    for key in ("knns", "knns_labels", "knns_ca_labels"):
        assert torch.equal(d1[key], d3[key]), key
    assert abs(j1 - float(c["g"]["jac"])) < 1e-4
