#!/usr/bin/env python3
"""Row f5, measured on the CPU: would a bf16 copy of the bank (storage_dtype 2 of SURVEY 8b) or a 3 x bf16 split of the rows serve the
certified candidate pass that the fp16 copy serves (csrc/hbird_knn_f16.hip: fp16 top-k', exact fp32 re-rank, per-query certificate
"exact k-th best > k'-th candidate score + E")?

For a cfg-2-sized bank (2,074,072 x 384: the token-level segmentation world of tests/parity_report.py, and the bench's random unit
rows) and a 768-d bank, per precision (operands rounded, products accumulated in fp32 like the MFMA does):
  * E = the rigorous bound on |low-precision score - fp32 chain score| that the certificate needs
        (both operands rounded: 2 u per product, Cauchy-Schwarz over the row, u = 2^-11 fp16 / 2^-8 bf16; + n x 2.4e-7 for the fp32
        accumulation of n products, the same margin rerank_kernel uses; 3 x bf16: six products per k, 3 x 2^-24 for the dropped ones),
  * the share of queries whose certificate passes with k' = 64 / 128 / 256 candidates (k = 30),
  * the measured max |score error| / E (how loose the bound is).
Test infrastructure (uses the oracle's helpers); writes profiles/r04/lowprec_certificate.json.  ~2 min on 8 cores.

`--worlds [--gpu-log FILE]`: the table of tests/f16_screen_worlds.py instead -- the adversarial rounding_world and the ViT-shaped worlds through the CPU
model of the screen (screen_model): mean pairwise cosine, cosine of the rank-30 neighbour, gap(k -> k') / E, the certified share at k' = 64 and 256
and the measured max |score error| / E -- into profiles/r08/fp16_certificate_worlds.json; FILE: the output of tests/test_f16_certificate_gpu.py
(-s), whose `F16WORLD {json}` lines (escalated / fallback shares on the GPU) are kept beside the table.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-hummingbird-eval_amd"), os.path.join(ROOT, "tests")]
import numpy as np   # noqa: E402
import torch         # noqa: E402
import oracle        # noqa: E402
import golden_inputs as gi   # noqa: E402

K, KC = 30, (64, 128, 256)


def token_world(n_images, D, C=21, H=224, ps=16, seed=11):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((C, D)).astype(np.float32)
    out = []
    for i in range(0, n_images, 512):
        b = min(512, n_images - i)
        y = gi.random_masks(b, H, H, C, 1000 + i, with_255=True)
        y[y == 255] = 0
        hist = oracle.patch_label_hist(y, ps, C).reshape(-1, C)
        out.append(hist @ cent + 0.5 * rng.standard_normal((hist.shape[0], D)).astype(np.float32))
    return np.concatenate(out).astype(np.float32)


def rounded(x, prec):
    if prec == "fp16":
        return [x.half().float()]
    if prec == "bf16":
        return [x.bfloat16().float()]
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = (x - h - m).bfloat16().float()
    return [h, m, l]


def scores(qs, bs):
    """sum of the kept partial products, fp32 accumulation (1 term, or the six of a 3 x bf16 split: hh hm mh hl lh mm)."""
    if len(qs) == 1:
        return qs[0] @ bs[0].T
    s = qs[0] @ bs[0].T
    for i, j in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 1)):
        s += qs[i] @ bs[j].T
    return s


def bound(prec, qn, bmax, D):
    if prec == "fp16":      # (with the fp16-subnormal term of the kernels' bound: an absolute 2^-25 per component, both operands)
        return qn * bmax * (1.05 / 1024.0 + D * 2.4e-7) + (qn + bmax) * D ** 0.5 * 6e-8
    if prec == "bf16":
        return qn * bmax * (1.05 / 128.0 + D * 2.4e-7)
    return qn * bmax * (3.0 * 2.0 ** -24 * 1.05 + 6 * D * 2.4e-7)


def run(name, bank, q):
    torch.set_num_threads(os.cpu_count() or 8)
    b = torch.from_numpy(bank); b = b / b.norm(dim=1, keepdim=True)
    qq = torch.from_numpy(q)
    D = b.shape[1]
    exact = (qq.double() @ b.double().T).float() if b.shape[0] * qq.shape[0] < 3e8 else qq @ b.T   # the ranking reference
    ex_top = exact.topk(K, dim=1).values[:, K - 1]            # exact k-th best
    qn = qq.norm(dim=1); bmax = float(b.norm(dim=1).max())
    res = {"bank_rows": int(b.shape[0]), "dim": int(D), "queries": int(qq.shape[0]), "k": K,
           "mean_gap_rank_k_to_rank_kc": {str(kc): float((ex_top - exact.topk(kc, dim=1).values[:, kc - 1]).mean()) for kc in KC},
           "mean_query_norm": float(qn.mean())}
    for prec in ("fp16", "bf16", "bf16x3"):
        t0 = time.time()
        s = scores(rounded(qq, prec), rounded(b, prec))
        E = bound(prec, qn, bmax, D)
        err = (s - exact).abs().max(dim=1).values
        top = s.topk(max(KC), dim=1).values
        r = {"mean_E": float(E.mean()), "max_err_over_E": float((err / E).max()), "seconds": round(time.time() - t0, 1)}
        for kc in KC:
            # the exact k-th best among the candidates is >= the global exact k-th best only if the true top-k are candidates; the
            # certificate as rerank_kernel states it: (exact k-th best of the candidates) > kc-th candidate score + E
            cand = s.topk(kc, dim=1).indices
            ex_c = torch.gather(exact, 1, cand).topk(K, dim=1).values[:, K - 1]
            ok = ex_c > top[:, kc - 1] + E
            r[f"certified_share_kc{kc}"] = float(ok.float().mean())
            r[f"true_topk_in_candidates_kc{kc}"] = float((ex_c == ex_top).float().mean())
        res[prec] = r
        print(name, prec, r, flush=True)
    return res


def main():
    out = {}
    rng = np.random.default_rng(0)
    nq = 768
    tw = token_world(10_582, 384)
    out["token_world_2074072x384"] = run("token_world", tw, token_world(8, 384, seed=11)[rng.permutation(8 * 196)[:nq]] if False else
                                         (tw[rng.permutation(tw.shape[0])[:nq]] + 0.5 * rng.standard_normal((nq, 384)).astype(np.float32)))
    del tw
    bank = rng.standard_normal((2_074_072, 384), dtype=np.float32)
    out["random_2074072x384"] = run("random384", bank, 3.0 * rng.standard_normal((nq, 384), dtype=np.float32))
    bank = rng.standard_normal((1_500_000, 768), dtype=np.float32)
    out["random_1500000x768"] = run("random768", bank, 3.0 * rng.standard_normal((512, 768), dtype=np.float32))
    out["reading"] = ("bf16 operands carry 8 x the rounding of fp16 (u = 2^-8 vs 2^-11), so E is ~7 x larger and the certificate -- which "
                      "must clear the gap between rank k and rank k' -- passes for few or no queries even with k' = 256; fp16 passes "
                      "everywhere with k' = 64.  A 3 x bf16 split costs six MFMAs per product for an E that the fp32 accumulation term "
                      "(6 D x 2.4e-7) keeps within ~2 x of fp16's: no candidate pass can use it better than the fp16 copy.")
    os.makedirs(os.path.join(ROOT, "profiles", "r04"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "r04", "lowprec_certificate.json"), "w"), indent=1)


def world_row(W, metric=0, k=K):
    import f16_screen_worlds as fw
    b64, q64 = W["bank"].astype(np.float64), W["queries"].astype(np.float64)
    bn, qn = b64 / np.linalg.norm(b64, axis=1, keepdims=True), q64 / np.linalg.norm(q64, axis=1, keepdims=True)
    sub = bn[np.random.default_rng(0).permutation(bn.shape[0])[:2000]]
    c = sub @ sub.T
    cos_q = qn @ bn.T
    row = {"bank_rows": int(b64.shape[0]), "dim": int(b64.shape[1]), "queries": int(q64.shape[0]), "k": k, "metric": "l2" if metric else "dot_product",
           "mean_pairwise_cosine": float((c.sum() - np.trace(c)) / (c.size - c.shape[0])),
           "rank_k_cosine_mean": float(np.sort(cos_q, axis=1)[:, -k].mean())}
    for kc in (64, 256):
        m = fw.screen_model(W["queries"], W["bank"], k, kc, metric)
        row[f"gap_k_to_kc{kc}_over_E_median"] = float(np.median(m["gap_over_E"]))
        row[f"certified_share_kc{kc}"] = float(m["certified"][1.0].mean())
        row[f"true_topk_in_candidates_kc{kc}"] = float(m["contained"].mean())
        row["max_err_over_E"] = float(m["err_over_E"].max())
        assert not m["wrong"][1.0].any()
    return row


def worlds_main(gpu_log=None):
    import f16_screen_worlds as fw
    out = {"cpu_model": {}}
    for D in (64, 384, 768):
        for metric in (0, 1):
            W = fw.rounding_world(D, K, 64, 10, 300, (0.5, 0.7, 0.8, 0.9, 0.95), metric=metric, seed=D + metric, n_background=4096)
            W = dict(W, queries=W["queries"][:W["n_groups"]])
            out["cpu_model"][f"rounding_world_d{D}_{'l2' if metric else 'ip'}"] = world_row(W, metric)
    for name, make in fw.VIT_WORLDS.items():
        for D in (128, 768):
            out["cpu_model"][f"{name}_20000x{D}"] = world_row(make(20_000, D, 128, seed=31))
            print(name, D, out["cpu_model"][f"{name}_20000x{D}"], flush=True)
    if gpu_log:
        out["gpu"] = [json.loads(line.split("F16WORLD ", 1)[1]) for line in open(gpu_log) if "F16WORLD " in line]
    out["reading"] = ("rounding_world: fp16 errors of 0.76-0.91 E with gaps below E and a true neighbour outside the candidates -- nothing certifies, as it "
                      "must.  The ViT-shaped worlds stay far inside E (max error 0.03-0.17 E) except massive activations (0.53-0.71 E: a few dimensions "
                      "carry the norm, and Cauchy-Schwarz is nearly tight on them); there the gap between rank k and rank 64 is 0.2-0.5 E and no query "
                      "certifies at k' = 64: the second pass and the adaptive use carry such banks.  GPU rows: subnormal bank components are kept by the "
                      "fp16 MFMA (subnormal_world certifies), near_limit_world's queries with a component at 65504 have ||q|| > 65504 and go to the fp32 "
                      "kernel by rule (half of them).")
    os.makedirs(os.path.join(ROOT, "profiles", "r08"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "r08", "fp16_certificate_worlds.json"), "w"), indent=1)


if __name__ == "__main__":
    if "--worlds" in sys.argv:
        worlds_main(sys.argv[sys.argv.index("--gpu-log") + 1] if "--gpu-log" in sys.argv else None)
    else:
        main()
