#!/usr/bin/env python3
"""Measurements of the image-level linear probe over the resident bank (profiles/r36/README.md):

  python tools/exp_linprobe_class.py --dry           # the plan of both shapes (FLOP, bytes, segments, chunks); touches no GPU
  python tools/exp_linprobe_class.py c1000           # 1,280,000 x 768, C = 1000
  python tools/exp_linprobe_class.py c256            # 1,280,000 x 768, C = 256
  python tools/exp_linprobe_class.py c1000 --evals 3 --no-torch     # a short run to put under a kernel trace for per-kernel times

Per shape: one evaluation of loss and gradient (hb_linprobe_class_loss_grad, whole call, by HIP events), the logits entry alone (the class
sweeps without the two softmax passes), and the route a user takes today on the same device (torch fp32 matmul + log_softmax + matmul on
chunks of `reconstruct`ed rows).  One JSON line per measurement; shares of the fp32 MFMA peak are given at 2400 MHz and at the kernel clock
read right after the timed loop.  Per-kernel times come from a kernel trace of the short run; HBIRD_HIP_LIB names an experiment build of
the library (the backward A/B of profiles/r36/README.md: `make varu UNIT=hbird_linprobe NAME=narrow` on a copy of hbird_linprobe.hip whose
hb_lp_backward never takes the wide form)."""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))

SHAPES = {"c1000": (1_280_000, 768, 1000), "c256": (1_280_000, 768, 256)}
PEAK_TF = 157.3                 # fp32 MFMA peak at PEAK_MHZ
PEAK_MHZ = 2400.0
CHUNK = 65536


def out(**kw):
    print(json.dumps(kw), flush=True)


def plan(name):
    rows, D, C = SHAPES[name]
    dp, cp, xs = (D + 15) // 16 * 16, (C + 31) // 32 * 32, (D + 1 + 31) // 32 * 32
    t = -(-rows // 256)
    seg_rows = 256 * max(1, -(-t // 512))
    nseg = -(-rows // seg_rows)
    chunk_segs = min(nseg, max(1, (1 << 30) // (seg_rows * (cp + xs) * 4)))
    fwd, bwd = 2 * rows * dp * cp, 2 * rows * xs * cp
    sweeps = -(-cp // 256)
    return dict(shape=name, rows=rows, D=D, C=C, Dp=dp, Cp=cp, Xs=xs, seg_rows=seg_rows, segments=nseg, chunk_segments=chunk_segs,
                chunks=-(-nseg // chunk_segs), sweeps=sweeps, tflop_forward=round(fwd / 1e12, 3), tflop_backward=round(bwd / 1e12, 3),
                ms_at_peak=round((fwd + bwd) / (PEAK_TF * 1e9), 2), bank_gb=round(rows * dp * 4 / 1e9, 2),
                bank_read_gb_forward=round(sweeps * rows * dp * 4 / 1e9, 2), softmax_pass_gb=round(4 * rows * cp * 4 / 1e9, 2))


def clock_mhz():
    """The kernel clock of GPU 0 as `rocm-smi --showclocks` reads it now, MHz, or None."""
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", text)
        return float(m.group(1)) if m else None
    except Exception:                                    # (a figure beside the timings, not a condition of them)
        return None


def shares(tflop, ms):
    """dict(share_of_peak at 2400 MHz, clock_mhz, share_of_peak_at_clock): the fraction of the fp32 MFMA peak of `tflop` done in `ms`."""
    tf, mhz = tflop / ms * 1e3, clock_mhz()
    return dict(tflops=round(tf, 2), share_of_peak=round(tf / PEAK_TF, 3), clock_mhz=mhz,
                share_of_peak_at_clock=None if not mhz else round(tf / (PEAK_TF * mhz / PEAK_MHZ), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="?", choices=sorted(SHAPES))
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if args.dry or args.shape is None:
        for name in sorted(SHAPES):
            out(**plan(name))
        return

    import numpy as np
    import torch
    from hbird_mi import _lib
    from hbird_mi import linear_probe as LP
    from hbird_mi import ops
    from hbird_mi.nn.search_hip import HipFlatIndex

    rows, D, C = SHAPES[args.shape]
    info = plan(args.shape)
    out(lib=os.path.relpath(_lib.LIB_PATH, ROOT), **info)
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn((C, D), generator=g, device="cuda"), dim=1)
    bank = HipFlatIndex(D, 0, 0)
    bank.reserve(rows)
    labels = torch.empty((rows,), dtype=torch.int32, device="cuda")
    t0 = time.time()
    for r in range(0, rows, 320000):
        m = min(320000, rows - r)
        cls = torch.randint(0, C, (m,), generator=g, device="cuda")
        bank.add(ops.normalize_rows(centres[cls] + torch.randn((m, D), generator=g, device="cuda") * (0.5 / D ** 0.5)), normalize=False)
        labels[r:r + m] = cls.to(torch.int32)
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
        res["r"] = LP.class_loss_grad(bank, labels, Wb, 1e-3)

    total = info["tflop_forward"] + info["tflop_backward"]
    med, lo, hi = timed(engine, args.evals)
    out(step="class_loss_grad", ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), **shares(total, med), loss=res["r"].loss,
        used=res["r"].used)
    again = LP.class_loss_grad(bank, labels, Wb, 1e-3)
    out(step="same_bits", equal=bool(np.array_equal(again.grad.view(np.uint64), res["r"].grad.view(np.uint64)) and again.loss == res["r"].loss))

    def sweeps_only():                                   # (allocates and writes [rows, C] logits: the sweeps' work and their write, no softmax pass)
        res["z"] = None
        res["z"] = LP.class_logits_of(bank, Wb)

    med_z, lo_z, hi_z = timed(sweeps_only, max(2, args.evals // 2))
    res["z"] = None
    out(step="class_logits", ms=round(med_z, 2), ms_min=round(lo_z, 2), ms_max=round(hi_z, 2), **shares(info["tflop_forward"], med_z))

    if not args.no_torch:
        W, b = Wb[:, 1:].contiguous(), Wb[:, 0].contiguous()
        y64 = labels.to(torch.int64)

        def torch_route():
            G = torch.zeros((C, D), device="cuda")
            gb = torch.zeros((C,), device="cuda")
            loss = torch.zeros((), dtype=torch.float64, device="cuda")
            for r in range(0, rows, CHUNK):
                ids = torch.arange(r, min(rows, r + CHUNK), device="cuda")
                x, y = bank.reconstruct(ids), y64[r:r + CHUNK]
                logp = torch.log_softmax(x @ W.T + b, dim=1)
                loss += -logp.gather(1, y.view(-1, 1)).sum().double()
                Rm = logp.exp()
                Rm.scatter_add_(1, y.view(-1, 1), torch.full((y.numel(), 1), -1.0, device="cuda"))
                G += Rm.T @ x
                gb += Rm.sum(dim=0)
            res["t"] = (float(loss) / rows, G, gb)

        med_t, lo_t, hi_t = timed(torch_route, max(2, args.evals // 2))
        out(step="torch_route", ms=round(med_t, 2), ms_min=round(lo_t, 2), ms_max=round(hi_t, 2), engine_over_torch=round(med / med_t, 3),
            data_loss=res["t"][0], clock_mhz=clock_mhz())
        gt = torch.cat([res["t"][2].view(-1, 1), res["t"][1]], dim=1).double().cpu().numpy() / rows + 1e-3 * Wb.double().cpu().numpy()
        out(step="torch_agreement", max_abs_gradient_difference=float(np.abs(gt - res["r"].grad).max()), gradient_max=float(np.abs(res["r"].grad).max()))
    bank.close()


if __name__ == "__main__":
    main()
