"""k beyond 256 over several ranks and several handles, after tests/test_dist_gpu.py: the ranks share cuda:0 and talk over gloo.

World 2 cuts G11's five training batches 3 / 2 (ragged shards of 768 and 512 rows, both shorter than k = 1024: every list ends in missing
entries); world 8 leaves ranks 5 .. 7 with empty shards.  The merged lists of a sharded search must be the single index's -- ids and
distance bits -- also where world x k is past hb_merge_topk's staging (8 x 1024: hb_bigk_merge_topk_packed), and the sharded evaluation
its mIoU."""
from __future__ import annotations

import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

KS = (600, 1024)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _indexed(c):
    """G11's batches for an IndexedReplayExtractor (a rank of a sharded build skips the batches it does not own)."""
    tok = {}
    for i, (x, _) in enumerate(c["train"]):
        x[0, 0, 0, 0] = float(i); tok[i] = c["tr_tok"][i]
    for i, (x, _) in enumerate(c["val"]):
        x[0, 0, 0, 0] = float(1000 + i); tok[1000 + i] = c["va_tok"][i]
    return tok


def _worker(rank, world, port, golden_dir, metric, label_shard, ret):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "open-hummingbird-eval_amd"), os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as td
    td.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from helpers import IndexedReplayExtractor
    from test_bigk_eval_gpu import g11_case
    from hbird_mi.hbird_eval import HbirdEvaluation
    from hbird_mi.nn.search_hip import HipFlatIndex, _merge_fits_lds, _METRICS
    c = g11_case(golden_dir)
    g = c["g"]
    torch.set_rng_state(torch.from_numpy(g["rng_state"]))
    ev = HbirdEvaluation(IndexedReplayExtractor(_indexed(c), c["S"], c["D"]), c["train"], num_classes=c["C"], n_neighbours=c["k"],
                         device="cuda:0", nn_method="faiss", nn_params={"idx_shard": True, "label_shard": label_shard, "distance_measure": metric})
    ok = ev.sharded and ev.label_shard == label_shard and ev.total_rows == 1280
    fm = ev.feature_memory
    # the whole bank on every rank, from the shards' own rows, in ONE index: what the sharded search has to reproduce
    rows = [None] * world
    td.all_gather_object(rows, fm.numpy())
    ok = ok and [r.shape[0] for r in rows] == ret["rows"]
    one = HipFlatIndex(c["D"], _METRICS[metric], 0)
    one.add(torch.from_numpy(np.concatenate(rows)).cuda())
    q = torch.from_numpy(np.concatenate(c["va_tok"]).reshape(-1, c["D"])).cuda()
    for k in KS:
        ok = ok and (_merge_fits_lds(world, k) == (not (world == 8 and k == 1024)))     # 8 x 1024 is past the old kernel's staging: the new one's
        idx, dist = ev.find_neighbours(q, k)
        ridx, rdist = one.search(q, k)
        ok = ok and torch.equal(idx, ridx) and torch.equal(dist.view(torch.int32), rdist.view(torch.int32))
        ok = ok and int((ridx >= 0).sum()) == q.shape[0] * min(k, 1280)
    jac = ev.evaluate(c["val"], c["S"], ignore_index=c["ign"])
    jac_d, det = ev.evaluate(c["val"], c["S"], return_knn_details=True, ignore_index=c["ign"])
    ok = ok and jac == jac_d
    if rank < 2 and metric == "dot_product":            # validation batch `rank` (round-robin) against the reference's label_hat
        B = c["B"]
        lh = det["knns_ca_labels"].numpy()
        ok = ok and (np.abs(lh - g["knns_ca_labels"][rank * B:(rank + 1) * B]) < 5e-5).mean() > 0.999
    ret[rank] = (bool(ok), float(jac))
    td.destroy_process_group()


def _single_index_jac(golden_dir, metric):
    from test_bigk_eval_gpu import evaluator, g11_case
    c = g11_case(golden_dir)
    ev = evaluator(c, nn_method="faiss", distance_measure=metric)
    return ev.evaluate(c["val"], c["S"], ignore_index=c["ign"]), float(c["g"]["jac"])


@pytest.mark.parametrize("world,metric,label_shard", [(2, "dot_product", False), (2, "l2", True), (8, "dot_product", True), (8, "l2", False)])
def test_sharded_search_and_evaluation_beyond_256(cuda_device, golden_dir, world, metric, label_shard):
    single, ref = _single_index_jac(golden_dir, metric)
    if metric == "dot_product":
        assert abs(single - ref) < 1e-4
    ret = mp.Manager().dict()
    ret["rows"] = [768, 512] if world == 2 else [256] * 5 + [0] * 3
    mp.spawn(_worker, args=(world, _free_port(), golden_dir, metric, label_shard, ret), nprocs=world, join=True)
    assert all(ret[r][0] for r in range(world)), dict(ret)
    jacs = {ret[r][1] for r in range(world)}
    assert len(jacs) == 1, jacs                           # every rank reports the same (all-reduced) mIoU
    jac = jacs.pop()
    print(f"G11 world {world} {metric} label_shard={label_shard}: jac {jac:.6f}, single index {single:.6f}")
    if label_shard:     # the partial sums add up in another order than the single kernel's chain: label_hat within rounding, not on bits
        assert abs(jac - single) < 1e-4
    else:
        assert jac == single


@pytest.mark.parametrize("metric", ["dot_product", "l2"])
def test_c_abi_multi_handle_search_at_1024(cuda_device, metric):
    """hb_multi_search through ctypes, cuda:0 listed three times (ragged shards): its host merge at k = 1024 against hb_index_search on
    one handle -- ids and distance bits; replicas too; k = 2049 is refused with the limit in the message."""
    import golden_inputs as gi
    from hbird_mi import _lib
    from hbird_mi.nn.search_hip import HipFlatIndex
    L = _lib.lib()
    M, D, nq, k = 4000, 64, 300, 1024
    bank = gi.unit_bank(M, D, seed=5)
    q = gi.vit_like_queries(nq, D, seed=6)
    m = 0 if metric == "dot_product" else 1
    one = HipFlatIndex(D, m, 0)
    one.add(bank)
    ridx, rdist = one.search(q, k)
    assert (ridx >= 0).all()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for shard in (1, 0):
        h = ctypes.c_void_p()
        _lib.check(L.hb_multi_create(D, m, (ctypes.c_int * 3)(0, 0, 0), 3, shard, ctypes.byref(h)))
        try:
            _lib.check(L.hb_multi_reserve(h, M))
            for a, b in ((0, 1000), (1000, 2777), (2777, M)):
                _lib.check(L.hb_multi_add(h, ptr(np.ascontiguousarray(bank[a:b])), b - a, 0))
            idx = np.empty((nq, k), np.int64); dist = np.empty((nq, k), np.float32)
            _lib.check(L.hb_multi_search(h, ptr(q), nq, k, ptr(idx), ptr(dist)))
            assert np.array_equal(idx, ridx) and np.array_equal(dist.view(np.uint32), rdist.view(np.uint32)), f"shard={shard}"
            assert L.hb_multi_search(h, ptr(q), nq, 2049, ptr(idx), ptr(dist)) != 0 and b"2048" in L.hb_last_error()
        finally:
            L.hb_multi_free(h)


@pytest.mark.parametrize("shard", [True, False])
def test_plugin_takes_1024_neighbours_on_a_sharded_index(cuda_device, shard):
    """NearestNeighborSearchHIP.find_nearest_neighbors with gpu_ids = [0, 0, 0]: k up to 2048 like a single index, 2049 a ValueError."""
    import golden_inputs as gi
    from hbird_mi.nn.search_hip import NearestNeighborSearchHIP
    M, D, nq = 3000, 48, 200
    fm = torch.from_numpy(gi.unit_bank(M, D, seed=8))
    q = torch.from_numpy(gi.vit_like_queries(nq, D, seed=9)).cuda()
    one = NearestNeighborSearchHIP(fm, n_neighbors=30, distance_measure="l2", gpu_ids=[0])
    nn = NearestNeighborSearchHIP(fm, n_neighbors=30, distance_measure="l2", idx_shard=shard, gpu_ids=[0, 0, 0])
    for k in (257, 1024, 2048):
        ridx, rdist = one.find_nearest_neighbors(q, k)
        idx, dist = nn.find_nearest_neighbors(q, k)
        assert torch.equal(idx, ridx) and torch.equal(dist.view(torch.int32), rdist.view(torch.int32)), k
    for bad in (0, 2049):
        with pytest.raises(ValueError, match="2048"):
            nn.find_nearest_neighbors(q, bad)
        with pytest.raises(ValueError, match="2048"):
            one.find_nearest_neighbors(q, bad)
