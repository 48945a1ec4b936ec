#!/usr/bin/env python3
"""Measurements of k-means over the resident bank (profiles/r28/README.md), by HIP events:

  python tools/exp_kmeans.py small     # 2 M x 384, K in {21, 500}
  python tools/exp_kmeans.py big       # 10 M x 768, K in {150, 500, 2048}
  python tools/exp_kmeans.py k6        # the fused upsample + argmax + confusion kernel on one-hot inputs of K channels, per batch

Per (bank, K): one iteration split into assign (hb_kmeans_assign over the whole bank) and accumulate (hb_kmeans_accumulate + centroids), and
a whole fit of a few iterations; against two yardsticks in the same process: a torch baseline on the same device (chunked mm + argmax +
index_add_ on a row-major copy of the rows) and, for accumulate, a device-to-device copy of the bank's bytes (the bandwidth yardstick: one
read and one write of them).  One JSON line per measurement."""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hbird_mi import kmeans as KM  # noqa: E402
from hbird_mi import ops  # noqa: E402
from hbird_mi.nn.search_hip import HipFlatIndex  # noqa: E402

CHUNK = 131072


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def out(**kw):
    print(json.dumps(kw), flush=True)


def build(rows, D, seed, keep_rows):
    """A bank of `rows` unit rows around 256 planted centres (+ noise of the centres' own size); with keep_rows also its row-major copy."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn((256, D), generator=g, device="cuda"), dim=1)
    bank = HipFlatIndex(D, 0, 0)
    bank.reserve(rows)
    kept = torch.empty((rows, D), dtype=torch.float32, device="cuda") if keep_rows else None
    for r in range(0, rows, 500000):
        m = min(500000, rows - r)
        x = centres[torch.randint(0, 256, (m,), generator=g, device="cuda")] + torch.randn((m, D), generator=g, device="cuda") / D ** 0.5
        x = ops.normalize_rows(x)
        bank.add(x, normalize=False)
        if keep_rows:
            kept[r:r + m] = x
    torch.cuda.synchronize()
    return bank, kept


def torch_assign(x, c):
    """Chunked mm + argmax: the nearest centroid by q.c - |c|^2 / 2."""
    half = 0.5 * (c * c).sum(dim=1)
    a = torch.empty((x.shape[0],), dtype=torch.int64, device=x.device)
    for r in range(0, x.shape[0], CHUNK):
        a[r:r + CHUNK] = (x[r:r + CHUNK] @ c.T - half).argmax(dim=1)
    return a


def torch_update(x, a, K):
    sums = torch.zeros((K, x.shape[1]), dtype=torch.float32, device=x.device)
    for r in range(0, x.shape[0], CHUNK):
        sums.index_add_(0, a[r:r + CHUNK], x[r:r + CHUNK])
    counts = torch.bincount(a, minlength=K)
    return sums / counts.clamp(min=1).unsqueeze(1)


def bank_main(rows, D, Ks, fit_iters=5):
    t0 = time.perf_counter()
    bank, x = build(rows, D, 1, keep_rows=True)
    bank_bytes = rows * ((D + 15) // 16 * 16) * 4              # the fragment tiles: rows x padded width
    out(what="bank_built", rows=rows, D=D, s=time.perf_counter() - t0, bank_bytes=bank_bytes)
    src = torch.empty((bank_bytes // 4,), dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), reps=5, warm=2)
    out(what="d2d_copy_of_bank_bytes", rows=rows, D=D, ms_median=copy_ms[0], ms_min=copy_ms[1], ms_max=copy_ms[2],
        read_plus_write_bytes_per_s=2 * bank_bytes / (copy_ms[0] * 1e-3))
    del src, dst
    for K in Ks:
        init = KM.initial_centroids(bank, K, None, 0)
        cent = HipFlatIndex(D, 1, 0)
        cent.set_fp16(0)
        cent.add(init, normalize=False)
        a, _ = KM.assign_rows(bank, cent)
        ms = timed(lambda: KM.assign_rows(bank, cent), reps=3, warm=1)
        out(what="assign", rows=rows, D=D, K=K, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2], flops=2.0 * rows * D * K,
            tflops=2.0 * rows * D * K / (ms[0] * 1e-3) / 1e12)
        sums = torch.zeros((K, D), dtype=torch.int64, device="cuda"); counts = torch.zeros((K,), dtype=torch.int64, device="cuda")

        def acc():
            sums.zero_(); counts.zero_()
            KM.accumulate(bank, a, K, sums=sums, counts=counts)
        ms = timed(acc, reps=5, warm=2)
        out(what="accumulate", rows=rows, D=D, K=K, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2], bank_read_bytes_per_s=bank_bytes / (ms[0] * 1e-3),
            accumulate_over_copy=ms[0] / copy_ms[0])
        ms = timed(lambda: KM.centroids_from_sums(sums, counts, init), reps=5, warm=2)
        out(what="centroids", K=K, D=D, ms_median=ms[0])
        # the torch baseline on the same rows
        a_t = torch_assign(x, init)
        agree = float((a_t == a.long()).float().mean().item())
        ms = timed(lambda: torch_assign(x, init), reps=3, warm=1)
        out(what="torch_assign", rows=rows, D=D, K=K, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2], agreement_with_engine=agree)
        ms = timed(lambda: torch_update(x, a_t, K), reps=3, warm=1)
        out(what="torch_update_index_add", rows=rows, D=D, K=K, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2])
        del a_t
        cent.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = KM.kmeans_fit(bank, K, init=init, max_iter=fit_iters)
        torch.cuda.synchronize()
        out(what="fit", rows=rows, D=D, K=K, max_iter=fit_iters, n_iter=res.n_iter, converged=res.converged, s=time.perf_counter() - t0,
            changed=[h["changed"] for h in res.history], empty=[h["empty"] for h in res.history])
    bank.close()


def k6_main():
    B, S, px, C = 16, 37, 518, 150
    g = torch.Generator().manual_seed(1)
    cells = torch.randint(0, C, (B, 1, (px + 36) // 37, (px + 36) // 37), generator=g)
    gt = cells.repeat_interleave(37, dim=2).repeat_interleave(37, dim=3)[:, :, :px, :px].contiguous().cuda()
    for K in (150, 500, 2048):
        ids = torch.randint(0, K, (B * S * S,), generator=g).cuda()
        conf = torch.zeros((C, K), dtype=torch.int64, device="cuda")

        def step():
            one_hot = (ids.view(-1, 1) == torch.arange(K, device="cuda").view(1, -1)).to(torch.float32)
            ops.upsample_argmax_confusion(one_hot.view(B, S * S, K), S, gt, conf, 255, want_map=False)
        ms = timed(step, reps=5, warm=2)
        out(what="one_hot_plus_fused_k6_k7_per_batch", B=B, S=S, px=px, C=C, K=K, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2])


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "small"
    if mode == "small":
        bank_main(2_000_000, 384, (21, 500))
    elif mode == "big":
        bank_main(10_000_000, 768, (150, 500, 2048))
    elif mode == "tiny":                                      # a rehearsal of the script itself
        bank_main(20_000, 64, (5,), fit_iters=2)
    else:
        k6_main()
