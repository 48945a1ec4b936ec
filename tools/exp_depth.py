#!/usr/bin/env python3
"""Measurements of the depth kernels (profiles/r30/README.md), one JSON line each; HIP events around whole calls, median (min - max):

  python tools/exp_depth.py kernels             # hb_patch_depth_targets and hb_depth_upsample_metrics on a cfg-3-shaped batch (B = 16, S = 37,
                                                # 518 px) at r = 1 and r = 14, beside a torch route on the same device
  python tools/exp_depth.py aggregate [--rows N]  # search_aggregate over one bank with C = 2 and C = 392 fp32 label rows, beside the
                                                # segmentation table (C = 151 counts of denominator 196)

The torch route is a yardstick, not a reference: F.interpolate of both grids, the divide, the clamp and the masked reductions."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=reps)


def torch_targets(y, ps, r, lo, hi):
    import torch
    ok = torch.isfinite(y) & (y >= lo) & (y <= hi)
    s = ps // r
    num = torch.nn.functional.avg_pool2d(torch.where(ok, y, torch.zeros_like(y))[:, None], s)
    den = torch.nn.functional.avg_pool2d(ok.float()[:, None], s)
    return num, den


def torch_metrics(agg, S, r, gt, lo, hi):
    import torch
    B = agg.shape[0]
    g = agg.view(B, S, S, 2, r, r).permute(0, 3, 1, 4, 2, 5).reshape(B, 2, S * r, S * r)
    up = torch.nn.functional.interpolate(g, size=gt.shape[-2:], mode="bilinear", align_corners=False)
    N, Dn = up[:, 0], up[:, 1]
    has = Dn > 0
    p = (N / Dn).clamp(lo, hi).double()
    gd = gt.double()
    m = (torch.isfinite(gt) & (gt >= lo) & (gt <= hi) & has)
    p, gd = torch.where(m, p, torch.ones_like(p)), torch.where(m, gd, torch.ones_like(gd))
    d, dl = p - gd, torch.log(p) - torch.log(gd)
    ratio = torch.maximum(p / gd, gd / p)
    terms = [m.double(), d * d, d.abs() / gd, d * d / gd, dl * dl, dl, (torch.log10(p) - torch.log10(gd)).abs(), (m & (ratio < 1.25)).double(),
             (m & (ratio < 1.25 ** 2)).double(), (m & (ratio < 1.25 ** 3)).double()]
    return torch.stack([t.sum(dim=(1, 2)) for t in terms], 1)


def kernels(args):
    import torch
    from hbird_mi import ops
    B, S, ps = 16, 37, 14
    H = S * ps
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.rand((B, H, H), generator=g, device="cuda") * 9.0 + 0.5
    y[torch.rand((B, H, H), generator=g, device="cuda") < 0.1] = 0.0
    gt = y.roll(3, 1).contiguous()
    for r in (1, 14):
        rows, _ = ops.patch_depth_targets(y, ps, r)
        agg = rows.view(B, S * S, -1).contiguous()
        mb = (y.numel() + rows.numel()) * 4 / 1e6
        out(what="hb_patch_depth_targets", r=r, B=B, S=S, px=H, mbytes=round(mb, 1), **timed(lambda: ops.patch_depth_targets(y, ps, r), args.reps))
        out(what="torch targets (avg_pool2d of masked depth and of the mask)", r=r, **timed(lambda: torch_targets(y, ps, r, 1e-3, 10.0), args.reps))
        out(what="hb_depth_upsample_metrics", r=r, B=B, S=S, px=H, mbytes=round((agg.numel() + gt.numel()) * 4 / 1e6, 1),
            **timed(lambda: ops.depth_upsample_metrics(agg, S, r, gt), args.reps))
        out(what="hb_depth_upsample_metrics + pred_out", r=r, **timed(lambda: ops.depth_upsample_metrics(agg, S, r, gt, want_map=True), args.reps))
        out(what="torch route (interpolate both grids, divide, clamp, masked float64 reductions)", r=r,
            **timed(lambda: torch_metrics(agg, S, r, gt, 1e-3, 10.0), args.reps))
        sums, _ = ops.depth_upsample_metrics(agg, S, r, gt)
        ref = torch_metrics(agg, S, r, gt, 1e-3, 10.0)
        out(what="engine against the torch route: n equal, largest relative difference of sq / abs_rel", r=r,
            n_equal=bool(torch.equal(sums[:, 0], ref[:, 0])), rel=float(((sums[:, 2:4] - ref[:, 1:3]).abs() / ref[:, 1:3]).max()))


def aggregate(args):
    import torch
    from hbird_mi import ops
    from hbird_mi.nn.search_hip import HipFlatIndex
    rows, D, k, nq = args.rows, 768, 30, 16 * 37 * 37
    g = torch.Generator(device="cuda").manual_seed(2)
    q = torch.randn((nq, D), generator=g, device="cuda")
    for C, P, name in ((2, 0, "depth r = 1 (C = 2, fp32)"), (392, 0, "depth r = 14 (C = 392, fp32)"), (151, 196, "segmentation (C = 151, counts of 196)")):
        ix = HipFlatIndex(D, 0, 0)
        ix.reserve(rows)
        ix.set_label_denominator(P)
        g2 = torch.Generator(device="cuda").manual_seed(3)
        for r0 in range(0, rows, 250000):
            m = min(250000, rows - r0)
            ix.add(torch.randn((m, D), generator=g2, device="cuda"), normalize=True)
            if P:
                lab = torch.zeros((m, C), device="cuda")
                lab[torch.arange(m, device="cuda"), torch.randint(0, C, (m,), generator=g2, device="cuda")] = 1.0
            else:
                lab = torch.rand((m, C), generator=g2, device="cuda")
            ix.add_labels(lab)
        ix.set_num_classes(C)
        out(what="search_aggregate", table=name, rows=rows, D=D, nq=nq, k=k, **timed(lambda: ix.search_aggregate(q, k, beta=0.02), args.reps, warmup=2))
        idx, dist = ix.search(q, k)
        out(what="search alone", table=name, **timed(lambda: ix.search(q, k), args.reps, warmup=1))
        out(what="aggregate alone (K5)", table=name, **timed(lambda: ix.aggregate(q, idx, dist, beta=0.02), args.reps, warmup=1))
        ix.close()
        del ix
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "aggregate"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=2_000_000)
    args = ap.parse_args()
    (kernels if args.what == "kernels" else aggregate)(args)


if __name__ == "__main__":
    main()
