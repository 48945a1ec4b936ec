#!/usr/bin/env python3
"""Measurements of the depth grids (profiles/r31/README.md) on one MI355X; every time is the median (min - max) of repeated whole calls by HIP
events after warm-ups, and every comparator is the route the code had before the grid entries existed:

  python tools/exp_depth_grid.py [--out profiles/r31] [--rows 2000000] [--reps 20]

  1. ops.depth_upsample_metrics_grid at 16 and at 4 configurations against that many calls of ops.depth_upsample_metrics, on the cfg-3-shaped
     batch (B = 16, S = 37, 518 px) at r = 1 and r = 14 -- with the slabs compared bit for bit at the sizes timed;
  2. one HbirdDepthEvaluation.evaluate_grid batch of 16 configurations against 16 evaluate batches on the same bank (--rows x 768, r = 1);
  3. ops.bootstrap_weighted_sums at 654 images x 16 configurations x 21 columns with 10,000 replicates against numpy's W @ table;
  4. hipcc's resource report of the unit's kernels.

Writes README.md and exp_depth_grid.json into --out.  Needs a GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))


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


def cell(t):
    return f"{t['median_ms']:.3f} ms ({t['min_ms']:.3f} - {t['max_ms']:.3f})"


def metric_kernels(reps):
    import torch
    from hbird_mi import ops
    B, S, ps = 16, 37, 14
    H = S * ps
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.rand((B, H, H), generator=g, device="cuda") * 9.0 + 0.5
    y[torch.rand((B, H, H), generator=g, device="cuda") < 0.1] = 0.0
    gt = y.roll(3, 1).contiguous()
    rows = []
    for r in (1, 14):
        # 16 slabs: the target rows of 16 shifted copies of the depth maps (what 16 configurations would have aggregated, in shape and range)
        agg = torch.stack([ops.patch_depth_targets(y.roll(c, 2).contiguous(), ps, r)[0].view(B, S * S, -1) for c in range(16)]).contiguous()
        for n_cfg in (16, 4):
            a = agg[:n_cfg].contiguous()
            loop = lambda: [ops.depth_upsample_metrics(a[c], S, r, gt) for c in range(n_cfg)]
            fused = lambda: ops.depth_upsample_metrics_grid(a, S, r, gt)
            want = torch.stack([s for s, _ in loop()])
            got, _ = fused()
            t_loop, t_fused = timed(loop, reps), timed(fused, reps)       # alternated below as well: the second pair guards against drift
            t_loop2, t_fused2 = timed(loop, reps), timed(fused, reps)
            rows.append(dict(what="depth_upsample_metrics_grid against the loop of calls", r=r, n_cfg=n_cfg, B=B, S=S, px=H,
                             bits_equal=bool(torch.equal(got.view(torch.int64), want.view(torch.int64))), loop=t_loop, grid=t_fused,
                             loop_again=t_loop2, grid_again=t_fused2,
                             ratio=round(min(t_loop["median_ms"], t_loop2["median_ms"]) / max(t_fused["median_ms"], t_fused2["median_ms"]), 2)))
            print(json.dumps(rows[-1]), flush=True)
        del agg
    return rows


def evaluator_batch(n_rows, reps):
    import torch
    from hbird_mi import depth as hdepth
    from hbird_mi.models import FeatureExtractorSimple
    from hbird_mi.nn.search_hip import HipFlatIndex
    B, S, D, px = 16, 37, 768, 518
    g = torch.Generator(device="cuda").manual_seed(2)
    ix = HipFlatIndex(D, 0, 0)
    ix.reserve(n_rows)
    ix.set_label_denominator(0)
    for r0 in range(0, n_rows, 250000):
        m = min(250000, n_rows - r0)
        ix.add(torch.randn((m, D), generator=g, device="cuda"), normalize=True)
        den = torch.rand((m, 1), generator=g, device="cuda")
        ix.add_labels(torch.cat([den * (torch.rand((m, 1), generator=g, device="cuda") * 9.0 + 0.5), den], 1).contiguous())
    ix.set_num_classes(2)
    tokens = torch.randn((B, S * S, D), generator=g, device="cuda")
    gt = torch.rand((B, 1, px, px), generator=g, device="cuda") * 9.0 + 0.5
    extractor = FeatureExtractorSimple(torch.nn.Identity(), ftr_extr_fn=lambda m, x: (x, None), eval_spatial_resolution=S, d_model=D)
    ks, betas = [5, 10, 20, 30], [0.01, 0.02, 0.05, 0.1]
    ev = hdepth.HbirdDepthEvaluation.from_index(extractor, ix, n_neighbours=30, beta=0.02)
    singles = [hdepth.HbirdDepthEvaluation.from_index(extractor, ix, n_neighbours=k, beta=b) for k in ks for b in betas]
    loader = [(tokens, gt)]
    grid = ev.evaluate_grid(loader, S, n_neighbours=ks, betas=betas)
    same = all((grid[(one.n_neighbours, one.beta)].sums == one.evaluate(loader, S).sums).all() for one in singles)
    t_loop = timed(lambda: [one.evaluate(loader, S) for one in singles], reps, warmup=1)
    t_grid = timed(lambda: ev.evaluate_grid(loader, S, n_neighbours=ks, betas=betas), reps, warmup=1)
    row = dict(what="one evaluate_grid batch of 16 configurations against 16 evaluate batches", bank_rows=n_rows, D=D, B=B, S=S, px=px, r=1,
               ks=ks, betas=betas, sums_equal=bool(same), loop=t_loop, grid=t_grid, ratio=round(t_loop["median_ms"] / t_grid["median_ms"], 2))
    print(json.dumps(row), flush=True)
    ix.close()
    return row


def weighted_sums(reps):
    import numpy as np
    import torch
    from hbird_mi import ops
    n_img, cols, R = 654, 16 * 21, 10000
    rng = np.random.default_rng(3)
    table = rng.standard_normal((n_img, cols)) * 10.0 ** rng.uniform(-3, 3, (n_img, cols))
    t = torch.from_numpy(table).cuda()
    W = ops.bootstrap_multiplicities(n_img, 7, R)
    Wh = W.cpu().numpy()
    t_dev = timed(lambda: ops.bootstrap_weighted_sums(t, W), reps)
    t_both = timed(lambda: ops.bootstrap_weighted_sums(t, ops.bootstrap_multiplicities(n_img, 7, R)).cpu(), reps)
    host = []
    for _ in range(max(3, reps // 4)):
        t0 = time.perf_counter()
        ref = Wh.astype(np.float64) @ table
        host.append((time.perf_counter() - t0) * 1e3)
    got = ops.bootstrap_weighted_sums(t, W).cpu().numpy()
    row = dict(what="bootstrap_weighted_sums against numpy W @ table", n_img=n_img, cols=cols, R=R, device=t_dev,
               device_with_draws_and_copy_back=t_both,
               numpy=dict(median_ms=round(statistics.median(host), 3), min_ms=round(min(host), 3), max_ms=round(max(host), 3), reps=len(host)),
               numpy_threads=os.environ.get("OMP_NUM_THREADS", "unset"),
               largest_relative_difference_to_numpy=float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))),
               ratio=round(statistics.median(host) / t_dev["median_ms"], 2))
    print(json.dumps(row), flush=True)
    return row


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "hbird_depth_grid.hip"), "-o", os.path.join(tmp, "unit.o")], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            z = re.match(r"_Z(\d+)", name)          # _Z<length><name><parameter types>
            if z:
                name = name[z.end():z.end() + int(z.group(1))]
            out[name] = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("static_lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def clock_note():
    try:
        p = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)       # read only
        lines = [ln.strip() for ln in p.stdout.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(lines[:2]) or "not reported"
    except Exception as e:      # noqa: BLE001 -- a note, not a measurement
        return f"not read ({type(e).__name__})"


def readme(res):
    k, e, w, rs = res["metric_kernels"], res["evaluator_batch"], res["weighted_sums"], res["resources"]
    lines = ["# Round 31: depth grids", "",
             f"One MI355X ({res['device']}), `tools/exp_depth_grid.py --rows {e['bank_rows']} --reps {res['reps']}`: whole calls by HIP events after warm-ups,",
             "median (min - max).  Raw figures: `exp_depth_grid.json`.  Clocks as the box reported them before the run: " + res["clock"] + ".",
             "Every comparator is the route the parent commit had: a loop of single calls.  No dataset is on any of our machines: nothing here is a depth accuracy.", "",
             "## `hb_depth_upsample_metrics_grid` against the loop of `hb_depth_upsample_metrics` calls (B = 16, S = 37, 518 x 518 px)", "",
             "| r | configurations | the loop of calls | one grid call | again: loop | again: grid | loop / grid (the loop's faster median over the grid's slower) | slabs equal bit for bit |",
             "|---|---|---|---|---|---|---|---|"]
    for row in k:
        lines.append(f"| {row['r']} | {row['n_cfg']} | {cell(row['loop'])} | {cell(row['grid'])} | {cell(row['loop_again'])} | {cell(row['grid_again'])} | "
                     f"**{row['ratio']}x** | {'yes' if row['bits_equal'] else 'NO'} |")
    lines += ["", "## One `evaluate_grid` batch of 16 configurations against 16 `evaluate` batches", "",
              f"Bank: {e['bank_rows']:,} x {e['D']} random rows with C = 2 fp32 label rows (r = 1); one batch of {e['B']} x {e['S']}^2 tokens, {e['px']} px maps;",
              f"k in {e['ks']} x beta in {e['betas']}.  Tokens are given (no ViT in either route).", "",
              "| route | time |", "|---|---|", f"| 16 x `from_index(k, beta).evaluate` | {cell(e['loop'])} |", f"| one `evaluate_grid` | {cell(e['grid'])} |", "",
              f"Ratio **{e['ratio']}x**; every configuration's sums equal the single route's: {'yes' if e['sums_equal'] else 'NO'}.", "",
              f"## `bootstrap_weighted_sums`: {w['n_img']} images x {w['cols']} columns, {w['R']:,} replicates", "",
              "| route | time |", "|---|---|", f"| the kernel (W and the table resident) | {cell(w['device'])} |",
              f"| ... with the draws (`bootstrap_multiplicities`) and the copy back | {cell(w['device_with_draws_and_copy_back'])} |",
              f"| numpy `W.astype(float64) @ table` (OMP_NUM_THREADS = {w['numpy_threads']}) | {cell(w['numpy'])} |", "",
              f"numpy over the kernel: {w['ratio']}x.  The kernel exists for defined, paired bits (a BLAS product sums in its own order: largest relative",
              f"difference to it {w['largest_relative_difference_to_numpy']:.1e}); it is not a bottleneck either way.", "",
              "## hipcc's resource report (`-Rpass-analysis=kernel-resource-usage`, gfx950)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | static LDS B | waves/SIMD |", "|---|---|---|---|---|---|---|"]
    for name, v in rs.items():
        lines.append(f"| `{name}` | {v.get('vgprs')} | {v.get('agprs')} | {v.get('sgprs')} | {v.get('scratch_bytes_per_lane')} | {v.get('static_lds_bytes')} | "
                     f"{v.get('occupancy_waves_per_simd')} |")
    lines += ["", "`depth_grid_metrics_kernel` takes its LDS dynamically: per configuration of a group 88 B per wave of partials and four staged rows of the",
              "column window (16 B per cell column), at most 64 KiB per workgroup.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31"))
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("exp_depth_grid.py measures on a GPU; none is visible")
    os.makedirs(args.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, clock=clock_note(), resources=resources())
    res["metric_kernels"] = metric_kernels(args.reps)
    res["weighted_sums"] = weighted_sums(args.reps)
    res["evaluator_batch"] = evaluator_batch(args.rows, max(3, args.reps // 4))
    with open(os.path.join(args.out, "exp_depth_grid.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(f"wrote {args.out}/README.md and exp_depth_grid.json")


if __name__ == "__main__":
    main()
