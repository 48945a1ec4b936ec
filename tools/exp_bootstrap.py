#!/usr/bin/env python3
"""Measurements of the bootstrap path (profiles/r25/README.md), by HIP events:

  python tools/exp_bootstrap.py reduce    # the reduction and the composite at ADE20K- and VOC-shaped tables, against numpy on the CPUs
  python tools/exp_bootstrap.py collect   # per-batch cost of collecting (class map + per-image counts) against the fused kernel alone

One JSON line per measurement."""
from __future__ import annotations

import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hbird_mi import ops  # noqa: E402

INT_VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9        # CUs x SIMDs x lanes x clock: one 32-bit VALU op per lane and cycle (MI355X_MICROARCH: 2.4 GHz peak)


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def table(N, n_cfg, G, pixels, seed):
    """Synthetic per-image counts: every image holds ~8 classes, `pixels` pixels split among (tp, fp, fn)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((N, n_cfg, G, 3), dtype=np.int32)
    for i in range(N):
        cls = rng.choice(G, size=min(8, G), replace=False)
        t[i][:, cls, :] = rng.integers(0, pixels // 24, size=(n_cfg, len(cls), 3))
    return t.reshape(N, n_cfg * 3 * G)


def reduce_main():
    R = 10000
    for name, N, G, n_cfg in (("ade20k", 2000, 150, 16), ("voc", 1449, 21, 16)):
        cols = n_cfg * 3 * G
        stats_h = table(N, n_cfg, G, 512 * 512, 1)
        stats = torch.from_numpy(stats_h).cuda()
        mads = R * N * cols
        Rw = 2048                                                     # the reduction alone, on a W that fits beside its counts
        W = ops.bootstrap_multiplicities(N, 1, Rw)
        med, lo, hi = timed(lambda: ops.bootstrap_counts(stats, W))
        rate = Rw * N * cols / (med * 1e-3)
        print(json.dumps({"what": "reduction", "shape": name, "n_img": N, "G": G, "n_cfg": n_cfg, "cols": cols, "R": Rw, "ms_median": med, "ms_min": lo,
                          "ms_max": hi, "mads_per_s": rate, "share_of_int_valu_lane_rate": rate / INT_VALU_LANE_OPS}), flush=True)
        med, lo, hi = timed(lambda: ops.bootstrap_multiplicities(N, 1, Rw))
        print(json.dumps({"what": "multiplicities", "shape": name, "R": Rw, "ms_median": med, "ms_min": lo, "ms_max": hi}), flush=True)
        med, lo, hi = timed(lambda: ops.bootstrap_miou(stats, n_cfg, G, 1, R), reps=3, warm=1)
        print(json.dumps({"what": "composite", "shape": name, "R": R, "ms_median": med, "ms_min": lo, "ms_max": hi, "mads": mads,
                          "mads_per_s": mads / (med * 1e-3), "share_of_int_valu_lane_rate": mads / (med * 1e-3) / INT_VALU_LANE_OPS}), flush=True)
        # numpy on 16 threads: 160 replicates (10 per thread) of the same product and epilogue, scaled to R
        Rb, threads = 160, 16
        Wh = W[:Rb].cpu().numpy()
        s64 = stats_h.astype(np.int64)

        def part(t):
            c = Wh[t * 10:(t + 1) * 10].astype(np.int64) @ s64
            c = c.reshape(10, n_cfg, G, 3).astype(np.float64)
            return (c[..., 0] / np.maximum(c[..., 0] + c[..., 1] + c[..., 2], 1e-8)).sum(axis=-1) / G
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(part, range(threads)))
            t0 = time.perf_counter()
            list(pool.map(part, range(threads)))
            dt = time.perf_counter() - t0
        print(json.dumps({"what": "numpy_16_threads", "shape": name, "R_measured": Rb, "s_measured": dt, "s_scaled_to_R": dt * R / Rb, "R": R,
                          "mads_per_s": Rb * N * cols / dt}), flush=True)


def collect_main():
    B, S, px, n_cfg = 16, 37, 518, 16
    for C in (21, 150):
        g = torch.Generator().manual_seed(C)
        lh = torch.rand((n_cfg, B, S * S, C), generator=g).cuda()
        cells = torch.randint(0, C, (B, 1, (px + 36) // 37, (px + 36) // 37), generator=g)
        gt = cells.repeat_interleave(37, dim=2).repeat_interleave(37, dim=3)[:, :, :px, :px].contiguous().cuda()
        gt[:, :, ::50, :] = 255
        conf = torch.zeros((n_cfg, C, C), dtype=torch.int64, device="cuda")
        tab = torch.zeros((B, n_cfg * 3 * C), dtype=torch.int32, device="cuda")

        def fused_only():
            for c in range(n_cfg):
                ops.upsample_argmax_confusion(lh[c], S, gt, conf[c], 255, want_map=False)

        def collecting():
            for c in range(n_cfg):
                pred = ops.upsample_argmax_confusion(lh[c], S, gt, conf[c], 255, want_map=True)
                ops.image_class_counts(gt, pred, C, 255, out=tab.view(-1)[c * 3 * C:], row_stride=n_cfg * 3 * C)

        def counts_only(pred=ops.upsample_argmax(lh[0], S, px, px)):
            for c in range(n_cfg):
                ops.image_class_counts(gt, pred, C, 255, out=tab.view(-1)[c * 3 * C:], row_stride=n_cfg * 3 * C)
        for name, fn in (("fused_kernel_alone", fused_only), ("with_map_and_image_counts", collecting), ("image_counts_alone", counts_only)):
            med, lo, hi = timed(fn)
            print(json.dumps({"what": name, "C": C, "B": B, "S": S, "px": px, "n_cfg": n_cfg, "ms_median_all_cfgs": med, "ms_min": lo, "ms_max": hi}),
                  flush=True)


if __name__ == "__main__":
    {"reduce": reduce_main, "collect": collect_main}[sys.argv[1] if len(sys.argv) > 1 else "reduce"]()
