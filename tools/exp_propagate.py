#!/usr/bin/env python3
"""Timing of ops.propagate_labels (profiles/r32/README.md) on one MI355X against a torch route in the same process, at the DAVIS shape of a
ViT-S/8 or ViT-B/8: a 60 x 106 grid (480 x 848 px), 8 context frames, radius 12, k = 5, d = 384 and 768:

  python tools/exp_propagate.py [--out profiles/r32] [--reps 20]

The torch route is DINO's own shape: one matmul of the frame's tokens against all context tokens, the window mask (built once, outside the
timed call, as DINO caches it), topk, softmax, and one matmul of the scattered weights with the label rows.  Every time is the median
(min - max) of whole calls by HIP events after warm-ups.  Also times the two mask entries at 480 x 848 and prints hipcc's resource report of
the propagate unit.  Writes README.md and exp_propagate.json into --out.  Needs a GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))

GH, GW, N_CTX, RADIUS, K, C, TEMP = 60, 106, 8, 12, 5, 4, 0.1


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


def window_mask(device):
    import torch
    y, x = torch.arange(GH, device=device), torch.arange(GW, device=device)
    cy, cx = torch.meshgrid(y, x, indexing="ij")
    cy, cx = cy.reshape(-1), cx.reshape(-1)
    one = ((cy[:, None] - cy[None, :]).abs() <= RADIUS) & ((cx[:, None] - cx[None, :]).abs() <= RADIUS)        # [N, N]
    return one.repeat(1, N_CTX)                                                                                # [N, n_ctx * N]


def propagate(d, reps):
    import torch
    from hbird_mi import ops
    N = GH * GW
    g = torch.Generator(device="cuda").manual_seed(d)
    feat = ops.normalize_rows(torch.randn((N_CTX, N, d), generator=g, device="cuda"))
    q = ops.normalize_rows(feat[3] + 0.5 * torch.randn((N, d), generator=g, device="cuda"))      # a frame that resembles its context
    lab = torch.rand((N_CTX, N, C), generator=g, device="cuda")
    slots, radii = list(range(N_CTX)), [RADIUS] * N_CTX
    mask = window_mask("cuda")
    ctx, lab_flat = feat.view(N_CTX * N, d), lab.view(N_CTX * N, C)

    def torch_route():
        s = q @ ctx.T
        s.masked_fill_(~mask, float("-inf"))
        v, i = s.topk(K, dim=1)
        w = torch.softmax(v / TEMP, dim=1)
        return torch.zeros_like(s).scatter_(1, i, w) @ lab_flat

    def kernel():
        return ops.propagate_labels(q, feat, lab, slots, radii, (GH, GW), k=K, temperature=TEMP)
    diff = float((kernel() - torch_route()).abs().max())
    t_kernel, t_torch = timed(kernel, reps), timed(torch_route, reps)
    t_kernel2, t_torch2 = timed(kernel, reps), timed(torch_route, reps)                 # the second pair guards against drift
    window = (2 * RADIUS + 1) ** 2
    row = dict(d=d, grid=[GH, GW], n_ctx=N_CTX, radius=RADIUS, k=K, c=C, kernel=t_kernel, torch=t_torch, kernel_again=t_kernel2, torch_again=t_torch2,
               ratio_torch_over_kernel=round(min(t_torch["median_ms"], t_torch2["median_ms"]) / max(t_kernel["median_ms"], t_kernel2["median_ms"]), 2),
               largest_difference_to_torch=diff, dense_over_window=round(N / window, 2),
               useful_gflop=round(2.0 * N * N_CTX * window * d / 1e9, 2))
    row["useful_tflops"] = round(row["useful_gflop"] / max(t_kernel["median_ms"], t_kernel2["median_ms"]), 2)
    print(json.dumps(row), flush=True)
    return row


def masks(reps):
    import torch
    from hbird_mi import ops
    H, W, B, n = 480, 848, 8, 3
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.rand((B, GH * GW, n + 1), generator=g, device="cuda")
    gt = torch.randint(0, n + 1, (B, H // 16, W // 16), generator=g, device="cuda").repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    pred = ops.mask_upsample_argmax(rows, (GH, GW), H, W)
    out = dict(B=B, h=H, w=W, n_objects=n, bound_px=8,
               upsample_argmax_channel_norm=timed(lambda: ops.mask_upsample_argmax(rows, (GH, GW), H, W, True), reps),
               upsample_argmax_plain=timed(lambda: ops.mask_upsample_argmax(rows, (GH, GW), H, W, False), reps),
               jf_counts=timed(lambda: ops.mask_jf_counts(pred, gt, n, 8), reps))
    print(json.dumps(out), flush=True)
    return out


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    out, name = {}, None
    for unit in ("hbird_propagate.hip", "hbird_maskmetrics.hip"):
        with tempfile.TemporaryDirectory() as tmp:
            p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
                                os.path.join(csrc, unit), "-o", os.path.join(tmp, "unit.o")], capture_output=True, text=True)
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                z = re.match(r"_Z(\d+)", name)          # _Z<length><name><parameter types>
                if z:
                    name = name[z.end():z.end() + int(z.group(1))]
                out[name] = {}
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                             ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"),
                             ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and name:
                    out[name][key] = int(m.group(1))
    return out


def readme(res):
    lines = ["# Round 32: video label propagation", "",
             f"One MI355X ({res['device']}), `tools/exp_propagate.py --reps {res['reps']}`: whole calls by HIP events after warm-ups, median (min - max).",
             "Raw figures: `exp_propagate.json`.  No dataset is on any of our machines: nothing here is a J&F figure, and no J&F figure of this engine has",
             "been held to a published one.", "",
             f"## `propagate_labels` against a torch route ({GH} x {GW} grid, {N_CTX} context frames, radius {RADIUS}, k = {K}, c = {C})", "",
             "The torch route, in the same process on the same tensors: `q @ ctx.T` over all context tokens, `masked_fill_` with the window mask (built",
             "once outside the timed call), `topk`, `softmax`, and `scatter_` + `@` with the label rows -- DINO's own shape.  It multiplies the whole",
             "frame against the whole context: `dense / window` times the arithmetic the window needs.", "",
             "| d | the kernel | the torch route | again: kernel | again: torch | torch / kernel (torch's faster median over the kernel's slower) | dense / window | "
             "useful TFLOP/s of the kernel | largest difference to torch |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res["propagate"]:
        lines.append(f"| {r['d']} | {cell(r['kernel'])} | {cell(r['torch'])} | {cell(r['kernel_again'])} | {cell(r['torch_again'])} | **{r['ratio_torch_over_kernel']}x** | "
                     f"{r['dense_over_window']} | {r['useful_tflops']} | {r['largest_difference_to_torch']:.1e} |")
    m = res["masks"]
    lines += ["", "Useful arithmetic counts every (query, key) pair inside a window once (2 d flop); the kernel also scores the keys of a tile's grown",
              "rectangle that lie outside a query's own window (a 4 x 8 tile grown by 12: 28 x 32 keys per context frame for 625 useful ones per query).",
              "What bounds the kernel, from its shape (no counter was collected): 210 workgroups for 256 CUs, two waves per SIMD, each on one",
              "dependent MFMA chain whose key loads from HBM only the other wave hides; 80 shuffles and up to 32 serial list pushes per score tile.", "",
              f"## The mask entries (B = {m['B']}, {m['h']} x {m['w']} px, {m['n_objects']} objects, bound {m['bound_px']} px)", "", "| entry | time |", "|---|---|",
              f"| `mask_upsample_argmax`, channel norm (three launches and a synchronisation) | {cell(m['upsample_argmax_channel_norm'])} |",
              f"| `mask_upsample_argmax`, plain | {cell(m['upsample_argmax_plain'])} |", f"| `mask_jf_counts` | {cell(m['jf_counts'])} |", "",
              "## hipcc's resource report (`-Rpass-analysis=kernel-resource-usage`, gfx950)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | static LDS B | waves/SIMD |", "|---|---|---|---|---|---|---|"]
    for name, v in res["resources"].items():
        lines.append(f"| `{name}` | {v.get('vgprs')} | {v.get('agprs')} | {v.get('sgprs')} | {v.get('scratch_bytes_per_lane')} | {v.get('static_lds_bytes')} | "
                     f"{v.get('occupancy_waves_per_simd')} |")
    lines += ["", "`propagate_kernel` takes its LDS dynamically: 32 query rows of d (+ 4) floats and, per wave (8, or 4 where 8 do not fit), 32 lists of k (score, id) pairs.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("exp_propagate.py measures on a GPU; none is visible")
    os.makedirs(args.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, resources=resources())
    res["propagate"] = [propagate(d, args.reps) for d in (384, 768)]
    res["masks"] = masks(args.reps)
    with open(os.path.join(args.out, "exp_propagate.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(f"wrote {args.out}/README.md and exp_propagate.json")


if __name__ == "__main__":
    main()
