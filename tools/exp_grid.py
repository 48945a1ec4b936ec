"""Evaluation grids: what one search_aggregate_grid costs against the separate calls it replaces.  HIP events on the index's stream, medians
after warm-up, the two sides alternating inside every repetition.
  (a) the nk * nb search_aggregate(q, k, beta) calls of the grid            (b) one search_aggregate_grid
  (c) K5 alone on the lists of one search at max(ks): nk * nb aggregate launches on contiguous prefixes against one aggregate_grid
usage: exp_grid.py [ROWS D NQ]      (default: cfg-2, 2,074,072 x 384, 12,544 queries; class counts 21 and 151 as uint16 counts, P = 256)
One JSON line per table; EXP_GRID_OUT=file collects them."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "open-hummingbird-eval_amd"), ROOT]
import numpy as np
import torch
from hbird_mi.nn.search_hip import HipFlatIndex, grid_plan

OUT = os.environ.get("EXP_GRID_OUT")
KS, BETAS = (10, 30, 90), (0.01, 0.02, 0.05, 0.1)
WARM, REPS = 2, 5


def emit(d):
    print(json.dumps(d), flush=True)
    if OUT:
        open(OUT, "a").write(json.dumps(d) + "\n")


def ms_of(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def table(M, D, NQ, C, P=256):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    ix = HipFlatIndex(D, 0, 0); ix.use_current_stream(); ix.set_label_denominator(P); ix.reserve(M)
    for lo in range(0, M, 500_000):
        n = min(500_000, M - lo)
        ix.add(torch.randn((n, D), generator=g, device="cuda"), normalize=True)
        cnt = torch.zeros((n, C), device="cuda"); cnt[:, 0] = P - 3; cnt[torch.arange(n), torch.randint(1, C, (n,), generator=g, device="cuda")] = 3
        ix.add_labels(cnt / P)
    ix.set_num_classes(C)
    q = torch.randn((NQ, D), generator=g, device="cuda")
    plan = grid_plan(KS, BETAS)

    def separate():
        return [ix.search_aggregate(q, k, beta=b) for k, b in plan.configs]

    def grid():
        return ix.search_aggregate_grid(q, KS, BETAS)

    idx, dist = ix.search(q, KS[-1])
    prefixes = {k: (idx[:, :k].contiguous(), dist[:, :k].contiguous()) for k in KS}

    def k5_separate():
        return [ix.aggregate(q, *prefixes[k], beta=b) for k, b in plan.configs]

    def k5_grid():
        return ix.aggregate_grid(q, idx, dist, KS, BETAS)

    t = {"a": [], "b": [], "c12": [], "c1": [], "search90": []}
    same = None
    for it in range(WARM + REPS):
        ta, sep = ms_of(separate)
        tb, one = ms_of(grid)
        tc12, _ = ms_of(k5_separate)
        tc1, _ = ms_of(k5_grid)
        ts, _ = ms_of(lambda: ix.search(q, KS[-1]))
        if same is None:        # faster and different is not faster: the grid's slabs are the separate calls' bits
            same = all(torch.equal(one[i].view(torch.int32), sep[i].view(torch.int32)) for i in range(len(sep)))
        if it >= WARM:
            for key, v in zip(("a", "b", "c12", "c1", "search90"), (ta, tb, tc12, tc1, ts)):
                t[key].append(v)
    path = ix.last_search_path()
    ix.set_timing(True); ix.search(q, KS[-1]); torch.cuda.synchronize()
    clock = ix.kernel_clock()
    med = {k: float(np.median(v)) for k, v in t.items()}
    emit({"rows": M, "d": D, "queries": NQ, "classes": C, "ks": KS, "betas": BETAS, "configs": len(plan.configs), "bits_equal": bool(same),
          "a_separate_search_aggregate_ms": med["a"], "b_search_aggregate_grid_ms": med["b"], "b_over_a": med["b"] / med["a"],
          "search_at_90_ms": med["search90"], "c_k5_separate_ms": med["c12"], "c_k5_grid_ms": med["c1"], "c_grid_over_separate": med["c1"] / med["c12"],
          "samples_ms": {k: [round(x, 3) for x in v] for k, v in t.items()}, "search_path": path, "kernel_clock": clock,
          "device": torch.cuda.get_device_name(0)})
    ix.close()


if __name__ == "__main__":
    M, D, NQ = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (2_074_072, 384, 12_544)
    assert torch.cuda.is_available(), "exp_grid.py measures on the GPU"
    for C in (21, 151):
        table(M, D, NQ, C)
