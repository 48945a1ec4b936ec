"""Excluding searches: what search_excluding(q, k, qgroups) costs against the plain search of the same index at k and at need = k + gmax.
HIP events on the index's stream, medians after warm-up, the three sides alternating inside every repetition.
  rows are dealt to groups of G consecutive rows (an image's patches); the queries are bank rows plus noise, each excluding its row's own
  group, as a training image does in a leave-one-image-out pass (on isotropic rows only the query's own row is sure to top its list).
Per (G): ms of search(k), search(need), search_excluding(k); the rungs, how many queries reached rung 1, which path served the last rung.
usage: exp_exclude.py [ROWS D NQ [K]]      (default: cfg-2, 2,074,072 x 384, 12,544 queries, k = 30; groups of 196 and 967 rows)
One JSON line per table; EXP_EXCLUDE_OUT=file collects them."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "open-hummingbird-eval_amd"), ROOT]
import numpy as np
import torch
from hbird_mi.nn.search_hip import HipFlatIndex, exclude_plan

OUT = os.environ.get("EXP_EXCLUDE_OUT")
GROUPS = (196, 967)
WARM, REPS = 2, 5


def emit(d):
    print(json.dumps(d), flush=True)
    if OUT:
        open(OUT, "a").write(json.dumps(d) + "\n")


def ms_of(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main(M, D, NQ, K):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    ix = HipFlatIndex(D, 0, 0); ix.use_current_stream(); ix.reserve(M)
    for lo in range(0, M, 500_000):
        ix.add(torch.randn((min(500_000, M - lo), D), generator=g, device="cuda"), normalize=True)
    src = torch.randint(0, M, (NQ,), generator=g, device="cuda")
    q = ix.reconstruct(src) + 0.05 * torch.randn((NQ, D), generator=g, device="cuda") / D ** 0.5
    for G in GROUPS:
        ix.set_row_groups(torch.arange(M, device="cuda") // G)
        qg = (src // G).to(torch.int32)
        gmax = min(G, M)
        rungs = exclude_plan(K, gmax)
        need = K + gmax
        t = {"search_k": [], "search_need": [], "excluding": []}
        info = path = None
        for it in range(WARM + REPS):
            a, _ = ms_of(lambda: ix.search(q, K))
            b, (ni, _) = ms_of(lambda: ix.search(q, need))
            path_need = ix.last_search_path()
            c, (ei, _) = ms_of(lambda: ix.search_excluding(q, K, qg))
            info, path = ix.last_exclusion(), ix.last_search_path()
            if it >= WARM:
                t["search_k"].append(a); t["search_need"].append(b); t["excluding"].append(c)
        # the result against its definition: the first K entries of the list at need whose group is not the query's
        rows = torch.arange(M, device="cuda") // G
        keep = rows[ni.clamp(min=0)] != qg[:, None].long()
        pos = torch.cumsum(keep, 1) - 1
        want = torch.full_like(ei, -1)
        sel = keep & (pos < K)
        want[torch.nonzero(sel)[:, 0], pos[sel]] = ni[sel]
        emit({"rows": M, "d": D, "nq": NQ, "k": K, "group_rows": G, "gmax": info["gmax"], "need": need, "rungs": rungs,
              "ms_search_k": float(np.median(t["search_k"])), "ms_search_need": float(np.median(t["search_need"])),
              "ms_search_excluding": float(np.median(t["excluding"])), "rungs_run": info["rungs"], "rung1_queries": info["rung1_queries"],
              "kf_last": info["kf"], "path_last_rung": path, "path_search_need": path_need, "equals_filtered_list_at_need": bool(torch.equal(ei, want))})
    ix.close()


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(*(a[:3] if len(a) >= 3 else (2_074_072, 384, 12_544)), a[3] if len(a) > 3 else 30)
