#!/usr/bin/env python3
"""Measurements of the linear probe over the resident bank (profiles/r29/README.md):

  python tools/exp_linprobe.py --dry          # the plan of both shapes (FLOP, bytes, segments, chunks); touches no GPU
  python tools/exp_linprobe.py small          # 2,074,072 x 384, C = 21
  python tools/exp_linprobe.py big            # 10 M x 768, C = 151
  python tools/exp_linprobe.py small --evals 2 --no-fit --no-torch     # a short run to put under a kernel trace for per-kernel times

Per shape: one evaluation of loss and gradient (hb_linprobe_loss_grad, whole call, by HIP events), the route a user takes today on the same
device (torch fp32 matmul + log_softmax + matmul on chunks of `reconstruct`ed rows and gathered labels), and a whole fit.  One JSON line per
measurement.  Per-kernel times come from a kernel trace of the short run."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))

SHAPES = {"small": (2_074_072, 384, 21, 196), "big": (10_000_000, 768, 151, 196)}
PEAK_TF = 157.3
CHUNK = 262144


def out(**kw):
    print(json.dumps(kw), flush=True)


def plan(name):
    rows, D, C, P = SHAPES[name]
    dp, cp, xs = (D + 15) // 16 * 16, (C + 31) // 32 * 32, (D + 1 + 31) // 32 * 32
    t = -(-rows // 256)
    seg_rows = 256 * max(1, -(-t // 512))
    nseg = -(-rows // seg_rows)
    chunk_segs = min(nseg, max(1, (1 << 30) // (seg_rows * (cp + xs) * 4)))
    flop = 2 * rows * dp * cp + 2 * rows * xs * cp
    return dict(shape=name, rows=rows, D=D, C=C, Dp=dp, Cp=cp, Xs=xs, seg_rows=seg_rows, segments=nseg, chunk_segments=chunk_segs,
                chunks=-(-nseg // chunk_segs), workspace_mb=round(chunk_segs * (seg_rows * (cp + xs) + cp * xs) * 4 / 2 ** 20, 1),
                tflop_per_eval=round(flop / 1e12, 3), ms_at_peak=round(flop / (PEAK_TF * 1e9), 2), bank_gb=round(rows * dp * 4 / 1e9, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="?", choices=sorted(SHAPES))
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--fit-iters", type=int, default=20)
    args = ap.parse_args()
    if args.dry or args.shape is None:
        for name in sorted(SHAPES):
            out(**plan(name))
        return

    import numpy as np
    import torch
    from hbird_mi import linear_probe as LP
    from hbird_mi import ops
    from hbird_mi.nn.search_hip import HipFlatIndex

    rows, D, C, P = SHAPES[args.shape]
    info = plan(args.shape)
    out(**info)
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn((C, D), generator=g, device="cuda"), dim=1)
    bank = HipFlatIndex(D, 0, 0)
    bank.reserve(rows)
    bank.set_label_denominator(P)
    t0 = time.time()
    for r in range(0, rows, 500000):
        m = min(500000, rows - r)
        cls = torch.randint(0, C, (m,), generator=g, device="cuda")
        x = ops.normalize_rows(centres[cls] + torch.randn((m, D), generator=g, device="cuda") * (0.5 / D ** 0.5))
        j2 = torch.randint(0, P // 2 + 1, (m,), generator=g, device="cuda")
        other = torch.randint(0, C, (m,), generator=g, device="cuda")
        counts = torch.zeros((m, C), dtype=torch.float32, device="cuda")
        counts.scatter_add_(1, cls.view(-1, 1), (P - j2).float().view(-1, 1))
        counts.scatter_add_(1, other.view(-1, 1), j2.float().view(-1, 1))
        bank.add(x, normalize=False)
        bank.add_labels((counts.double() / float(P)).float())      # (the GPU's fp32 division is not the correctly rounded one the counts need)
    bank.set_num_classes(C)
    torch.cuda.synchronize()
    out(step="build", seconds=round(time.time() - t0, 2))
    Wb = (torch.randn((C, D + 1), generator=g, device="cuda") * 0.5).contiguous()

    def timed(fn, reps, warm=1):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    res = {}

    def engine():
        res["r"] = LP.loss_grad(bank, Wb, 1e-3)

    med, lo, hi = timed(engine, args.evals)
    out(step="loss_grad", ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), tflops=round(info["tflop_per_eval"] / med * 1e3, 2),
        share_of_peak=round(info["tflop_per_eval"] / med * 1e3 / PEAK_TF, 3), bank_gb_per_s=round(2 * info["bank_gb"] / med * 1e3, 1),
        loss=res["r"].loss, used=res["r"].used)
    again = LP.loss_grad(bank, Wb, 1e-3)
    out(step="same_bits", equal=bool(np.array_equal(again.grad.view(np.uint64), res["r"].grad.view(np.uint64)) and again.loss == res["r"].loss))

    if not args.no_torch:
        W, b = Wb[:, 1:].contiguous(), Wb[:, 0].contiguous()

        def torch_route():
            G = torch.zeros((C, D), device="cuda")
            gb = torch.zeros((C,), device="cuda")
            loss = torch.zeros((), dtype=torch.float64, device="cuda")
            for r in range(0, rows, CHUNK):
                ids = torch.arange(r, min(rows, r + CHUNK), device="cuda")
                x, y = bank.reconstruct(ids), bank.gather_labels(ids)
                logp = torch.log_softmax(x @ W.T + b, dim=1)
                s = y.sum(dim=1, keepdim=True)
                loss += -(y * logp).sum().double()
                Rm = s * logp.exp() - y
                G += Rm.T @ x
                gb += Rm.sum(dim=0)
            res["t"] = (float(loss) / rows, G, gb)

        med_t, lo_t, hi_t = timed(torch_route, max(2, args.evals // 2))
        out(step="torch_route", ms=round(med_t, 2), ms_min=round(lo_t, 2), ms_max=round(hi_t, 2), engine_over_torch=round(med / med_t, 3),
            data_loss=res["t"][0])
        gt = torch.cat([res["t"][2].view(-1, 1), res["t"][1]], dim=1).double().cpu().numpy() / rows + 1e-3 * Wb.double().cpu().numpy()
        out(step="torch_agreement", max_abs_gradient_difference=float(np.abs(gt - res["r"].grad).max()), gradient_max=float(np.abs(res["r"].grad).max()))

    if not args.no_fit:
        torch.cuda.synchronize()
        t0 = time.time()
        probe = LP.linear_probe_fit(bank, l2=1e-3, gtol=1e-5, max_iter=args.fit_iters)
        torch.cuda.synchronize()
        out(step="fit", seconds=round(time.time() - t0, 2), iterations=probe.n_iter, state=probe.state, loss=probe.history[-1]["loss"],
            gmax=probe.history[-1]["gmax"])
        probe.close()
    bank.close()


if __name__ == "__main__":
    main()
