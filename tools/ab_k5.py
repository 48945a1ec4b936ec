#!/usr/bin/env python3
"""K5 of two or more builds of libhbird_hip.so side by side in one process (tools/ab_lib.py's pattern: one ctypes.CDLL handle per library,
seeded inputs generated once), through hb_index_aggregate, hb_bigk_aggregate, hb_bigk_aggregate_partial and hb_index_aggregate_grid.

usage: ab_k5.py bits lib1.so lib2.so ...   every output of every library against the first library's, as uint32 words
       ab_k5.py time lib1.so lib2.so ...   HIP-event medians per library at the workload's own size, the libraries alternating inside
                                           every repetition (name the first library twice, as two files, for the A/A spread)
One JSON line per case; AB_K5_OUT=file collects them.  `bits` exits with status 1 when a word differs."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "open-hummingbird-eval_amd")]
import numpy as np
import torch
from hbird_mi import _lib as sigs

OUT = os.environ.get("AB_K5_OUT")
dev = torch.device("cuda", 0)
p = lambda t: ctypes.c_void_p(t.data_ptr())


def emit(d):
    print(json.dumps(d), flush=True)
    if OUT:
        open(OUT, "a").write(json.dumps(d) + "\n")


class Lib:
    def __init__(self, path):
        self.path, self.L = path, ctypes.CDLL(path)
        for table in (sigs.SIGNATURES, sigs.SIGNATURES_GRID):
            for name, (res, args) in table.items():
                fn = getattr(self.L, name); fn.restype = res; fn.argtypes = args

    def ok(self, rc):
        assert rc == 0, f"{self.path}: {self.L.hb_last_error().decode()}"

    def index(self, D, metric, rows, labels, P):
        """An index holding `rows` [M, D] (normalised on the way in) and `labels` [M, C], as counts of denominator P when P > 0."""
        L, h = self.L, ctypes.c_void_p()
        self.ok(L.hb_index_create(D, metric, 0, ctypes.byref(h)))
        self.ok(L.hb_index_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if P:
            self.ok(L.hb_index_set_label_denominator(h, P))
        self.ok(L.hb_index_reserve(h, rows.shape[0]))
        for lo in range(0, rows.shape[0], 262144):
            r, l = rows[lo:lo + 262144].contiguous(), labels[lo:lo + 262144].contiguous()
            self.ok(L.hb_index_add(h, p(r), r.shape[0], 1, 1))
            self.ok(L.hb_index_add_labels(h, p(l), l.shape[0], l.shape[1], 1))
        return h

    # the four entries, each -> its output tensor (out: one to write into, so that a timed call allocates nothing)
    def aggregate(self, h, C, q, idx, dist, beta, bigk=False, out=None):
        out = torch.empty((q.shape[0], C), device=dev) if out is None else out
        self.ok((self.L.hb_bigk_aggregate if bigk else self.L.hb_index_aggregate)(h, p(q), q.shape[0], p(idx), p(dist), idx.shape[1], 0, beta, p(out), 1))
        return out

    def partial(self, h, C, q, idx, dist, beta, norms):
        out = torch.empty((q.shape[0], C), device=dev)
        self.ok(self.L.hb_bigk_aggregate_partial(h, p(q), q.shape[0], p(idx), p(dist), idx.shape[1], 0, beta, p(norms), norms.shape[0], p(out)))
        return out

    def grid(self, h, C, q, idx, dist, ks, betas, out=None):
        out = torch.empty((len(ks) * len(betas), q.shape[0], C), device=dev) if out is None else out
        ka, ba = (ctypes.c_int * len(ks))(*ks), (ctypes.c_float * len(betas))(*betas)
        self.ok(self.L.hb_index_aggregate_grid(h, p(q), q.shape[0], p(idx), p(dist), idx.shape[1], 0, ka, len(ks), ba, len(betas), p(out), 1))
        return out


def table(g, M, C, P):
    """Label rows [M, C]: multiples of 1 / P (what K2 produces), or for P = 0 any fp32 values in [0, 1)."""
    if P:
        # (a tensor as the divisor: a true division, (float)j / (float)P; dividing by a Python number may multiply by a rounded 1 / P)
        return torch.randint(0, P + 1, (M, C), generator=g, device=dev).float() / torch.tensor(float(P), device=dev)
    return torch.rand((M, C), generator=g, device=dev)


def lists(g, M, nq, k, metric, holes):
    """Neighbour lists as a search leaves them in value range; `holes`: some -1 entries and ids outside the table (the bit check)."""
    idx = torch.randint(0, M, (nq, k), generator=g, device=dev)
    dist = torch.rand((nq, k), generator=g, device=dev) * 0.04 + 0.5
    if metric == 1:
        dist = 2.0 - 2.0 * dist
    if holes:
        r = torch.rand((nq, k), generator=g, device=dev)
        idx = torch.where(r < 0.03, torch.full_like(idx, -1), idx)
        idx = torch.where(r > 0.98, idx + M, idx)
    return idx, dist.contiguous()


def bits(libs):
    M, D, nq, bad = 5000, 16, 300, 0
    g = torch.Generator(device=dev); g.manual_seed(7)
    rows = torch.randn((M, D), generator=g, device=dev)
    q = 3.0 * torch.randn((nq, D), generator=g, device=dev)
    norms = torch.rand((M,), generator=g, device=dev) + 0.5          # hb_bigk_aggregate_partial: everybody's norms
    for name, C, P in (("fp32 C=21 grouped", 21, 0), ("counts C=151 P=196 wide", 151, 196), ("counts C=70 P=4096 generic, dividing", 70, 4096)):
        lab = table(g, M, C, P)
        for metric in (0, 1):
            hs = [l.index(D, metric, rows, lab, P) for l in libs]
            runs = []      # (what, function of (lib, handle))
            for k in (30, 256, 600, 2048):
                idx, dist = lists(g, M, nq, k, metric, holes=True)
                if k <= 256:
                    runs.append((f"hb_index_aggregate k={k}", lambda l, h, a=(idx, dist): l.aggregate(h, C, q, *a, 0.02)))
                runs.append((f"hb_bigk_aggregate k={k}", lambda l, h, a=(idx, dist): l.aggregate(h, C, q, *a, 0.02, bigk=True)))
                runs.append((f"hb_bigk_aggregate_partial k={k}", lambda l, h, a=(idx, dist): l.partial(h, C, q, *a, 0.02, norms)))
            idx, dist = lists(g, M, nq, 90, metric, holes=True)
            runs.append(("hb_index_aggregate_grid 3x4 k_max=90", lambda l, h, a=(idx, dist): l.grid(h, C, q, *a, (10, 30, 90), (0.01, 0.02, 0.05, 0.1))))
            for what, fn in runs:
                outs = [fn(l, h).view(torch.int32) for l, h in zip(libs, hs)]
                torch.cuda.synchronize()
                diff = [int((o != outs[0]).sum()) for o in outs]
                bad += sum(diff)
                emit({"mode": "bits", "table": name, "metric": metric, "entry": what, "words": outs[0].numel(), "finite": bool(torch.isfinite(outs[0].view(torch.float32)).all()),
                      "differing_words_vs_first": dict(zip((os.path.basename(l.path) for l in libs), diff))})
            for l, h in zip(libs, hs):
                l.L.hb_index_free(h)
    emit({"mode": "bits", "total_differing_words": bad})
    return 1 if bad else 0


def time_legs(libs, warm=3, reps=9, inner=4):
    g = torch.Generator(device=dev); g.manual_seed(11)
    D = 16                                           # K5 reads the queries only for their norms
    names = [os.path.basename(l.path) for l in libs]

    def run(what, fns):
        t = [[] for _ in libs]
        for it in range(warm + reps):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record(); torch.cuda.synchronize()
                if it >= warm:
                    t[i].append(e0.elapsed_time(e1) / inner)
        med = [float(np.median(v)) for v in t]
        emit({"mode": "time", "leg": what, "median_ms": dict(zip(names, (round(m, 4) for m in med))),
              "over_first": dict(zip(names, (round(m / med[0], 4) for m in med))),
              "min_max_ms": dict(zip(names, ([round(min(v), 4), round(max(v), 4)] for v in t)))})

    # tools/exp_bigk.py k5: 21,904 queries, C = 151 as counts of P = 196, a table of 2 M rows
    M, C, P, nq = 2_000_000, 151, 196, 21_904
    rows, lab = torch.randn((M, D), generator=g, device=dev), table(g, M, C, P)
    hs = [l.index(D, 0, rows, lab, P) for l in libs]
    q = torch.randn((nq, D), generator=g, device=dev)
    o = torch.empty((nq, C), device=dev)
    for k in (30, 256, 600):
        idx, dist = lists(g, M, nq, k, 0, holes=False)
        if k <= 256:
            run(f"hb_index_aggregate k={k} C=151 P=196 nq={nq}", [lambda l=l, h=h: l.aggregate(h, C, q, idx, dist, 0.02, out=o) for l, h in zip(libs, hs)])
        run(f"hb_bigk_aggregate k={k} C=151 P=196 nq={nq}", [lambda l=l, h=h: l.aggregate(h, C, q, idx, dist, 0.02, bigk=True, out=o) for l, h in zip(libs, hs)])
    for l, h in zip(libs, hs):
        l.L.hb_index_free(h)
    # tools/exp_grid.py (c): K5 alone on lists of 90, 3 x 4 configurations, 12,544 queries, 2,074,072 rows, counts of P = 256
    M, P, nq = 2_074_072, 256, 12_544
    rows = torch.randn((M, D), generator=g, device=dev)
    q = torch.randn((nq, D), generator=g, device=dev)
    idx, dist = lists(g, M, nq, 90, 0, holes=False)
    for C in (21, 151):
        lab = table(g, M, C, P)
        hs = [l.index(D, 0, rows, lab, P) for l in libs]
        o = torch.empty((12, nq, C), device=dev)
        run(f"hb_index_aggregate_grid 3x4 k_max=90 C={C} P=256 nq={nq}", [lambda l=l, h=h: l.grid(h, C, q, idx, dist, (10, 30, 90), (0.01, 0.02, 0.05, 0.1), out=o) for l, h in zip(libs, hs)])
        for l, h in zip(libs, hs):
            l.L.hb_index_free(h)
    return 0


if __name__ == "__main__":
    assert len(sys.argv) >= 4 and sys.argv[1] in ("bits", "time"), __doc__
    torch.cuda.set_device(0)
    libs = [Lib(path) for path in sys.argv[2:]]
    sys.exit(bits(libs) if sys.argv[1] == "bits" else time_legs(libs))
