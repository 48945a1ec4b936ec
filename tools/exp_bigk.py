"""Workloads behind profiles/r10/README.md (k beyond 256), one mode and k per process, meant to run under `rocprofv3 --kernel-trace --stats`:
  split K   search_aggregate_bigk on 2,074,072 x 384, C = 21, 12,544 queries, three steps
  k5 K      hb_index_aggregate against hb_bigk_aggregate, 21,904 queries, C = 151 as uint16 counts, a table of 2 M rows, alternating
  merge K   hb_merge_topk against hb_bigk_merge_topk, 8 parts x K, 21,904 queries, alternating
usage: python tools/exp_bigk.py split|k5|merge K"""
import ctypes, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-hummingbird-eval_amd")]
import torch
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

mode, k = sys.argv[1], int(sys.argv[2])
dev = torch.device("cuda:0")
torch.manual_seed(0)
P = 196


def fill(ix, M, D, C, chunk=262144):
    ix.set_label_denominator(P)
    ix.reserve(M)
    Pt = torch.tensor(float(P), device=dev)
    for lo in range(0, M, chunk):
        n = min(chunk, M - lo)
        ix.add(torch.randn(n, D, device=dev), normalize=True)
        ix.add_labels(torch.randint(0, P + 1, (n, C), device=dev).float() / Pt)
    ix.set_num_classes(C)


if mode == "split":
    M, D, C, nq, steps = 2_074_072, 384, 21, 12_544, 3
    ix = HipFlatIndex(D, 0, 0); fill(ix, M, D, C)
    q = torch.randn(nq, D, device=dev)
    torch.cuda.synchronize()
    for _ in range(steps):
        lh = ix.search_aggregate_bigk(q, k)
    torch.cuda.synchronize()
    print("split", k, "steps", steps, "path", ix.last_search_path(), float(lh.sum()))
elif mode == "k5":
    M, D, C, nq, reps = 2_000_000, 16, 151, 21_904, 5
    ix = HipFlatIndex(D, 0, 0); fill(ix, M, D, C)
    q = torch.randn(nq, D, device=dev)
    idx = torch.randint(0, M, (nq, k), device=dev)
    dist = torch.rand(nq, k, device=dev) * 0.04 + 0.5
    torch.cuda.synchronize()
    for _ in range(reps + 1):
        a = ix.aggregate(q, idx, dist); b = ix.aggregate_bigk(q, idx, dist)
    torch.cuda.synchronize()
    print("k5", k, "bits equal", bool(torch.equal(a.view(torch.int32), b.view(torch.int32))))
elif mode == "merge":
    parts, nq, reps = 8, 21_904, 5
    sc = torch.randn(parts, nq, k, device=dev).sort(dim=-1, descending=True).values.contiguous()
    # ids ascending along every list: equal scores (random fp32 values do collide) then stand in id order, the new kernel's precondition
    ids = (torch.randint(1, 5, (parts, nq, k), device=dev).cumsum(dim=-1) * parts + torch.arange(parts, device=dev)[:, None, None]).contiguous()
    L = _lib.lib(); p = lambda t: ctypes.c_void_p(t.data_ptr()); s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = [(torch.empty(nq, k, dtype=torch.int64, device=dev), torch.empty(nq, k, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(reps + 1):
        _lib.check(L.hb_merge_topk(p(sc), p(ids), parts, nq, k, 0, p(o[0][0]), p(o[0][1]), s))
        _lib.check(L.hb_bigk_merge_topk(p(sc), p(ids), parts, nq, k, 0, p(o[1][0]), p(o[1][1]), s))
    torch.cuda.synchronize()
    print("merge", k, "equal", bool(torch.equal(o[0][0], o[1][0]) and torch.equal(o[0][1], o[1][1])), "rows that differ", int((o[0][0] != o[1][0]).any(dim=1).sum()))
