#!/usr/bin/env python3
"""hb_index_search of two or more builds of libhbird_hip.so side by side in one process (tools/ab_k5.py's pattern: one ctypes.CDLL handle per
library, seeded inputs generated once).  For changes to the kNN launcher that must not change a result word, a path decision or the speed.

usage: ab_knn.py bits lib1.so lib2.so ...   per case ids and distances as uint32 words, hb_index_schedule_info, hb_last_search_path and the two
                                            fp16 counters of every library against the first library's; one case per branch of the launcher's
                                            plan, at the smallest shape that reaches it
       ab_knn.py time lib1.so lib2.so ...   whole searches at the project's measured sizes: HIP events around 20 back-to-back
                                            hb_index_search calls, median of 9 repetitions after 3 warm-ups, the libraries alternating inside
                                            every repetition (name the first library twice, as two files, for the A/A spread: the resolution)
One JSON line per case; AB_KNN_OUT=file collects them.  `bits` exits with status 1 on any difference."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "open-hummingbird-eval_amd"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
from hbird_mi import _lib as sigs
from ab_k5 import Lib, dev, p

OUT = os.environ.get("AB_KNN_OUT")


def emit(d):
    print(json.dumps(d), flush=True)
    if OUT:
        open(OUT, "a").write(json.dumps(d) + "\n")


class KnnLib(Lib):
    def __init__(self, path):      # (not Lib's: an older build lacks the newest entries, which no case here calls)
        self.path, self.L = path, ctypes.CDLL(path)
        for table in (sigs.SIGNATURES, sigs.SIGNATURES_CENTRE):
            for name, (res, args) in table.items():
                fn = getattr(self.L, name, None)
                if fn is not None:
                    fn.restype = res; fn.argtypes = args

    def bank(self, D, metric, rows):
        h = ctypes.c_void_p()
        self.ok(self.L.hb_index_create(D, metric, 0, ctypes.byref(h)))
        self.ok(self.L.hb_index_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        for lo in range(0, rows.shape[0], 262144):
            r = rows[lo:lo + 262144].contiguous()
            self.ok(self.L.hb_index_add(h, p(r), r.shape[0], 1, 1))
        return h

    def search(self, h, q, k, idx, dist):
        self.ok(self.L.hb_index_search(h, p(q), q.shape[0], k, 0, p(idx), p(dist), 1))

    def reports(self, h):
        L, info, a, b, n = self.L, (ctypes.c_int64 * 8)(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        self.ok(L.hb_index_schedule_info(h, info))
        self.ok(L.hb_last_search_path(h, ctypes.byref(a), ctypes.byref(b)))
        out = {"schedule_info": list(info), "path": [a.value, b.value]}
        self.ok(L.hb_index_last_fp16_escalated(h, ctypes.byref(n))); out["escalated"] = n.value
        self.ok(L.hb_index_last_fp16_fallbacks(h, ctypes.byref(n))); out["fallbacks"] = n.value
        return out


def planted(g, M, D, nq, offset=0.0):
    """Random rows with two planted near-duplicate clusters (150 and 400 rows) and queries aimed at them: the fp16 chain's certificates fail
    there, so the second fp16 pass and the fp32 search of what is left both run.  offset: a common component (the centred copy's case)."""
    rows = torch.randn((M, D), generator=g, device=dev) + offset
    q = torch.randn((nq, D), generator=g, device=dev) + offset
    if M >= 40_000:
        c1, c2 = rows[7].clone(), rows[8].clone()
        rows[1000:1150] = c1 + 1e-4 * torch.randn((150, D), generator=g, device=dev)
        rows[30_000:30_400] = c2 + 1e-4 * torch.randn((400, D), generator=g, device=dev)
        q[:60] = c1 + 1e-3 * torch.randn((60, D), generator=g, device=dev)
        q[60:100] = c2 + 1e-3 * torch.randn((40, D), generator=g, device=dev)
    return rows, q


def bits(libs):
    L = lambda name, *a: (lambda l, h: l.ok(getattr(l.L, name)(h, *a)))
    shares = (ctypes.c_double * 8)(1.1, 0.9, 1.05, 0.95, 1.0, 1.0, 1.2, 0.8)
    f16 = lambda state, copy: [L("hb_index_set_fp16", state), L("hb_index_set_rerank_copy", copy)]
    small, two, wide = (5000, 64, 300), (66_000, 64, 300), (60_000, 128, 700)      # (rows, D, queries); `two`: 2 x 258 tiles >= 256 workgroups
    cases = [      # (what, shape, k, settings)
        ("lists k=5", small, 5, []), ("small pools k=30", small, 30, []), ("pools k=90", small, 90, []),
        ("LDS-staged small lists D=40", (5000, 40, 300), 30, []), ("LDS-staged pools D=40 k=90", (5000, 40, 300), 90, []),
        ("fp32 clusters 2x2, lists", two, 30, [L("hb_index_set_cluster", 2, 2, -1)]), ("fp32 clusters 2x2, pools", two, 90, [L("hb_index_set_cluster", 2, 2, -1)]),
        ("fp32 clusters 2x2, LDS-staged", two, 30, [L("hb_index_set_cluster", 2, 2, -1), L("hb_index_set_variant", 4)]),
        ("fp16 clusters 2x2 shared", two, 30, [L("hb_index_set_fp16", 1), L("hb_index_set_cluster", 2, 2, -1), L("hb_index_set_cluster_sharing", 2)]),
        ("variant 3", small, 30, [L("hb_index_set_variant", 3)]), ("variant 4", small, 30, [L("hb_index_set_variant", 4)]),
        ("variant 4 k=90", small, 90, [L("hb_index_set_variant", 4)]), ("variant 6", small, 30, [L("hb_index_set_variant", 6)]),
        ("phases off k=90", small, 90, [L("hb_index_set_search_options", 0, 0)]), ("small_limit 1", small, 30, [L("hb_index_set_search_options", 1, 1)]),
        ("given shares", two, 30, [L("hb_index_set_xcd_weights", 2, shares)]), ("given shares k=90", two, 90, [L("hb_index_set_xcd_weights", 2, shares)]),
        ("fp16 state 1, rerank copy", wide, 30, f16(1, 1)), ("fp16 state 1, no rerank copy", wide, 30, f16(1, 2)),
        ("fp16 state 1, no escalation", wide, 30, f16(1, 1) + [L("hb_index_set_fp16_escalation", 1)]),
        ("fp16 state 2 below its bound", wide, 30, f16(2, 1)), ("fp16 state 2, rerank copy", (66_000, 384, 700), 30, f16(2, 1)),
        ("fp16 state 2, no rerank copy", (66_000, 384, 700), 30, f16(2, 2)), ("fp16 state 1 k=90", wide, 90, f16(1, 0)),
        ("fp16 centred", wide, 30, f16(1, 1) + [L("hb_index_set_fp16_centre", 1)]),
        ("fp16 centred, no rerank copy", wide, 30, f16(1, 2) + [L("hb_index_set_fp16_centre", 1)]),
        ("k=300", small, 300, []), ("k=600", small, 600, []), ("k=300 on a use_fp16 index", wide, 300, f16(1, 0)),
        ("a bank of one tile", (200, 64, 300), 30, []), ("a bank of one tile k=5", (200, 64, 300), 5, []), ("an empty bank", (0, 64, 300), 30, []),
    ]
    bad = 0
    worlds = {}
    for what, shape, k, settings in cases:
        M, D, nq = shape
        centred = "centred" in what
        if (shape, centred) not in worlds:
            g = torch.Generator(device=dev); g.manual_seed(7 + M + D)
            worlds[(shape, centred)] = planted(g, M, D, nq, offset=0.5 if centred else 0.0)
        rows, q = worlds[(shape, centred)]
        for metric in (0, 1):
            outs, reps = [], []
            for l in libs:
                h = l.bank(D, metric, rows)
                for s in settings:
                    s(l, h)
                idx, dist = torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), device=dev)
                for _ in range(2):      # (twice: the second search runs on the cached work list and on the copies the first one made)
                    l.search(h, q, k, idx, dist)
                torch.cuda.synchronize()
                outs.append(torch.cat([idx.view(torch.int32).flatten(), dist.view(torch.int32).flatten()]))
                reps.append(l.reports(h))
                l.L.hb_index_free(h)
            diff = [int((o != outs[0]).sum()) for o in outs]
            rdiff = [int(r != reps[0]) for r in reps]
            bad += sum(diff) + sum(rdiff)
            emit({"mode": "bits", "case": what, "metric": metric, "rows": M, "d": D, "nq": nq, "k": k, "words": outs[0].numel(), "reports": reps[0],
                  "differing_words_vs_first": dict(zip((os.path.basename(l.path) for l in libs), diff)),
                  "differing_reports_vs_first": dict(zip((os.path.basename(l.path) for l in libs), rdiff))})
    emit({"mode": "bits", "total_differences": bad})
    return 1 if bad else 0


def time_legs(libs, warm=3, reps=9, inner=20):
    names = [os.path.basename(l.path) for l in libs]
    # (the last leg once more with equal XCD shares: every library calibrates shares of its own from its own launches' stamps, so at that size
    # the libraries otherwise run on different work lists)
    # copy: hb_index_set_rerank_copy (0: automatic -- the fp16 legs re-rank from the row-major copy; 2: from the fragment tiles)
    for M, D, nq, k, fp16, equal, copy in ((20_000, 384, 784, 30, 0, 0, 0), (50_176, 384, 12_544, 30, 0, 0, 0), (300_000, 768, 21_904, 30, 1, 0, 0),
                                           (300_000, 768, 21_904, 30, 1, 1, 0), (300_000, 768, 21_904, 30, 1, 0, 2)):
        g = torch.Generator(device=dev); g.manual_seed(11)
        rows, q = torch.randn((M, D), generator=g, device=dev), torch.randn((nq, D), generator=g, device=dev)
        hs = [l.bank(D, 0, rows) for l in libs]
        for l, h in zip(libs, hs):
            l.ok(l.L.hb_index_set_fp16(h, fp16))
            if copy:
                l.ok(l.L.hb_index_set_rerank_copy(h, copy))
            if equal:
                l.ok(l.L.hb_index_set_xcd_weights(h, 1, None))
        idx, dist = torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), device=dev)
        t = [[] for _ in libs]
        for it in range(warm + reps):
            for i, (l, h) in enumerate(zip(libs, hs)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    l.search(h, q, k, idx, dist)
                e1.record(); torch.cuda.synchronize()
                if it >= warm:
                    t[i].append(e0.elapsed_time(e1) / inner)
        med = [float(np.median(v)) for v in t]
        emit({"mode": "time", "leg": f"{M} x {D}, {nq} queries, k={k}, set_fp16({fp16})" + (", equal shares" if equal else "") + (f", set_rerank_copy({copy})" if copy else ""), "median_ms": dict(zip(names, (round(m, 4) for m in med))),
              "over_first": dict(zip(names, (round(m / med[0], 4) for m in med))),
              "min_max_ms": dict(zip(names, ([round(min(v), 4), round(max(v), 4)] for v in t))), "reports": [l.reports(h) for l, h in zip(libs, hs)]})
        for l, h in zip(libs, hs):
            l.L.hb_index_free(h)
    return 0


if __name__ == "__main__":
    assert len(sys.argv) >= 4 and sys.argv[1] in ("bits", "time"), __doc__
    torch.cuda.set_device(0)
    libs = [KnnLib(path) for path in sys.argv[2:]]
    sys.exit(bits(libs) if sys.argv[1] == "bits" else time_legs(libs))
