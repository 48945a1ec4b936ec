"""Pins the CPU oracle against fixtures produced by the reference's own Python (tests/golden/gen_golden.py).

CPU only.  These tests are what makes the oracle trustworthy as the checker of the HIP path.
"""
import os

import numpy as np
import pytest

import golden_inputs as gi
import oracle


def _load(golden_dir, name):
    return np.load(f"{golden_dir}/{name}")


def test_g1_patchify(golden_dir):
    g = _load(golden_dir, "g12_patchify_softlabels.npz")
    for name in "abc":
        for C in (21, 151):
            y, ps = g[f"y_{name}_{C}"], int(g[f"ps_{name}_{C}"])
            assert np.array_equal(oracle.patchify_gt(y, ps), g[f"patches_{name}_{C}"])


def test_g2_soft_labels_bit_exact(golden_dir):
    g = _load(golden_dir, "g12_patchify_softlabels.npz")
    for name in "abc":
        for C in (21, 151):
            y, ps = g[f"y_{name}_{C}"], int(g[f"ps_{name}_{C}"])
            lab = oracle.patch_label_hist(y, ps, C)
            ref = g[f"label_{name}_{C}"]
            assert lab.shape == ref.shape
            assert np.array_equal(lab.view(np.uint32), ref.view(np.uint32))   # count/P rounding identical


def test_patch_label_hist_rejects_out_of_range():
    y = np.full((1, 1, 8, 8), 255, dtype=np.int64)
    with pytest.raises(ValueError):
        oracle.patch_label_hist(y, 4, 21)


def test_g3_cross_attention(golden_dir):
    g = _load(golden_dir, "g3_cross_attention.npz")
    for name in ("small", "vitS"):
        out = oracle.cross_attention(g[f"q_{name}"], g[f"k_{name}"], g[f"v_{name}"], beta=0.02)
        ref = g[f"out_{name}"]
        # the oracle works in float64; torch's fp32 bmm/softmax differs by rounding only
        assert np.abs(out - ref).max() < 2e-5, np.abs(out - ref).max()
        assert np.allclose(out.sum(-1), 1.0, atol=1e-5)


def test_g4_knn_definition(golden_dir):
    g = _load(golden_dir, "g4_knn.npz")
    for name in ("ip32", "l2_32", "ip384"):
        M, D, B, N, k, C = g[f"shape_{name}"].tolist()
        metric = str(g[f"metric_{name}"])
        bank = gi.unit_bank(M, D, seed=41)
        lab = gi.labels_from_masks(M, C, 196, seed=42)
        q = gi.vit_like_queries(B * N, D, seed=43)
        if name == "ip32":
            bank[1234] = bank[77]; bank[4000] = bank[77]; q[0] = 5.0 * bank[77]
        i64, d64 = oracle.knn_f64(q, bank, k, metric)
        assert np.array_equal(i64, g[f"idx_{name}"])
        assert np.allclose(d64, g[f"dist_{name}"], rtol=1e-6, atol=1e-6)
        # gather semantics of hbird_eval.py:631-637
        kf, kl = oracle.gather_neighbours(i64, bank, lab, B, N)
        assert np.array_equal(kl, g[f"kl_{name}"])
        assert np.allclose(kf.sum(-1), g[f"kf_rowsum_{name}"], atol=1e-5)
        # the fp32 chain flavour agrees with the float64 definition except at near-ties
        i32, d32 = oracle.knn_chain_f32(q, bank, k, metric)
        sign = 1.0 if metric == "dot_product" else -1.0
        rep = oracle.near_tie_report(i32, i64, sign * d64)
        assert rep["excused_rate"] == 1.0 and rep["set_rate"] >= 0.99, rep
        if name == "ip32":   # exact ties resolved by lower id in both flavours
            assert i64[0, :3].tolist() == [77, 1234, 4000] and i32[0, :3].tolist() == [77, 1234, 4000]


def test_chain_oracle_is_a_sequential_fmaf_chain():
    """The AVX2 kernel must equal the textbook definition: acc = fmaf(q_k, b_k, acc), k ascending."""
    import math
    if not hasattr(math, "fma"):
        # python < 3.13: emulate fmaf via float64 (exact product of two fp32 fits in float64; the sum with an
        # fp32 accumulator is then rounded twice only when the float64 sum is inexact, which we detect)
        def fmaf(a, b, c):
            p = np.float64(a) * np.float64(b)
            s = p + np.float64(c)
            return np.float32(s)
    else:
        def fmaf(a, b, c):
            return np.float32(math.fma(float(a), float(b), float(c)))
    rng = np.random.default_rng(0)
    # small integers / dyadic values: every fma is exact in float64, so the emulation is exact too
    bank = (rng.integers(-8, 9, size=(50, 24)) / 8.0).astype(np.float32)
    q = (rng.integers(-16, 17, size=(7, 24)) / 4.0).astype(np.float32)
    idx, dist = oracle.knn_chain_f32(q, bank, 5)
    for i in range(q.shape[0]):
        sc = []
        for b in range(bank.shape[0]):
            acc = np.float32(0)
            for kk in range(q.shape[1]):
                acc = fmaf(q[i, kk], bank[b, kk], acc)
            sc.append(acc)
        sc = np.array(sc, dtype=np.float32)
        order = np.lexsort((np.arange(len(sc)), -sc))[:5]
        assert np.array_equal(order, idx[i]) and np.array_equal(sc[order], dist[i])


def test_knn_oracle_edge_cases():
    bank = gi.unit_bank(10, 8, seed=1)
    q = gi.vit_like_queries(3, 8, seed=2)
    for fn in (oracle.knn_chain_f32, oracle.knn_f64):
        idx, dist = fn(q, bank, 12)
        assert (idx[:, 10:] == -1).all() and np.isneginf(dist[:, 10:]).all()
        idx, dist = fn(q, bank, 12, "l2")
        assert (idx[:, 10:] == -1).all() and np.isposinf(dist[:, 10:]).all()
        assert (np.diff(dist[:, :10], axis=1) >= 0).all()
        idx, _ = fn(q, bank, 3, "dot_product", 1000)
        assert idx.min() >= 1000
    idx, dist = oracle.knn_chain_f32(q[:0], bank, 4)
    assert idx.shape == (0, 4)


def test_g5_sample_features(golden_dir):
    g = _load(golden_dir, "g5_sample.npz")
    for name in "ab":
        ps, C, K, seed = g[f"cfg_{name}"].tolist()
        y, feats, r = g[f"y_{name}"], g[f"feats_{name}"], g[f"r_{name}"]
        pt = oracle.patchify_gt(y, ps)
        assert oracle.sample_num_nonempty(pt, C).sum() == r.shape[0]
        sidx, _ = oracle.sample_patches(pt, C, K, r)
        assert np.array_equal(sidx, g[f"sidx_{name}"])
        sf = np.take_along_axis(feats, sidx[:, :, None], axis=1)
        assert np.array_equal(sf, g[f"sfeat_{name}"])


def _replay_memory(g, name):
    """Rebuild the bank exactly as hbird_eval.py:283-369 does, with the oracle's pieces."""
    C, D, H, ps, nb, B, k, mem, aug, ign = g[f"cfg_{name}"].tolist()
    import torch
    S = H // ps
    K = None if mem < 0 else max(1, mem // max(1, nb * B * aug))
    if K is not None:
        torch.set_rng_state(torch.from_numpy(g[f"rng_state_{name}"]))
    feats, labs = [], []
    for _ in range(aug):
        for i in range(nb):
            y = np.rint(g[f"train_y_{name}_{i}"] * 255.0).astype(np.int64)     # (y*255).long(), 309
            y[y == 255] = 0                                                      # 310
            tok = g[f"train_tok_{name}_{i}"]
            lab = oracle.patch_label_hist(y, ps, C).reshape(B, S * S, C)         # 317-320
            if K is None:
                feats.append(oracle.normalize_rows(tok).reshape(-1, D))          # 324-325
                labs.append(lab.reshape(-1, C))
            else:
                pt = oracle.patchify_gt(y, ps)
                nz = int(oracle.sample_num_nonempty(pt, C).sum())
                r = torch.rand(nz).numpy()                                       # 500
                sidx, _ = oracle.sample_patches(pt, C, K, r)
                sf = np.take_along_axis(tok, sidx[:, :, None], axis=1)           # 515
                feats.append(oracle.normalize_rows(sf).reshape(-1, D))           # 335
                labs.append(np.take_along_axis(lab, sidx[:, :, None], axis=1).reshape(-1, C))   # 344
    return np.concatenate(feats), np.concatenate(labs), (C, D, H, ps, nb, B, k, mem, aug, ign)


@pytest.mark.parametrize("name", ["unb", "bnd", "trim", "ade"])
def test_g6_create_memory(golden_dir, name):
    g = _load(golden_dir, "g67_memory_evaluate.npz")
    fm, lm, _ = _replay_memory(g, name)
    ref_f, ref_l = g[f"feature_memory_{name}"], g[f"label_memory_{name}"]
    assert fm.shape == ref_f.shape and lm.shape == ref_l.shape       # incl. the trimmed bounded case
    assert np.array_equal(lm, ref_l)
    # torch's fp32 norm reduction order differs from the oracle's float64 accumulation: <= 2 ulp
    assert np.abs(fm - ref_f).max() <= 2.5e-7, np.abs(fm - ref_f).max()


@pytest.mark.parametrize("name", ["unb", "bnd", "trim", "ade"])
def test_g7_evaluate(golden_dir, name):
    g = _load(golden_dir, "g67_memory_evaluate.npz")
    C, D, H, ps, nb, B, k, mem, aug, ign = g[f"cfg_{name}"].tolist()
    S = H // ps
    fm, lm = g[f"feature_memory_{name}"], g[f"label_memory_{name}"]     # identical bank for both paths
    metric = oracle.PredsMIoUOracle(C, C, ignore_index=ign)
    lhs, cms = [], []
    for i in range(2):
        tok = g[f"val_tok_{name}_{i}"]
        y = np.rint(g[f"val_y_{name}_{i}"] * 255.0).astype(np.int64)          # hbird_eval.py:219
        idx, _ = oracle.knn_f64(tok.reshape(-1, D), fm, k)
        kf, kl = oracle.gather_neighbours(idx, fm, lm, B, S * S)
        lh = oracle.cross_attention(tok, kf, kl)
        cm = oracle.upsample_argmax(lh, S, H, H)
        metric.update(y, cm)
        lhs.append(lh); cms.append(cm)
    lh = np.concatenate(lhs)
    assert np.abs(lh - g[f"label_hat_{name}"]).max() < 2e-5
    cm = np.concatenate(cms)
    agree = (cm == g[f"cluster_map_{name}"]).mean()
    assert agree > 0.999, agree        # argmax can flip only where two classes are within rounding
    if name == "unb":
        up = oracle.upsample_bilinear(g[f"label_hat_{name}"].reshape(-1, S, S, C).transpose(0, 3, 1, 2), H, H)
        assert np.abs(up - g[f"upsampled_{name}"]).max() < 1e-6
    miou = metric.compute()[0]
    assert abs(miou - float(g[f"jac_{name}"])) < 1e-4, (miou, float(g[f"jac_{name}"]))


def test_g8_predsmiou(golden_dir):
    g = _load(golden_dir, "g8_predsmiou.npz")
    for name in ("c5", "c21", "ade"):
        C, n, ign = g[f"cfg_{name}"].tolist()
        gt, pred = g[f"gt_{name}"], g[f"pred_{name}"]
        m = oracle.PredsMIoUOracle(C, C, ignore_index=ign)
        m.update(gt.reshape(2, -1), pred.reshape(2, -1))
        assert np.array_equal(m.conf, g[f"conf_{name}"])
        for mode, kw in {"hung": {}, "m2o": {"many_to_one": True},
                         "m2o_prec": {"many_to_one": True, "precision_based": True}, "lin": {"linear_probe": True}}.items():
            miou, tp, fp, fn, _ = m.compute(**kw)
            assert abs(miou - float(g[f"miou_{name}_{mode}"])) < 1e-12
            assert tp == g[f"tp_{name}_{mode}"].tolist()
            assert fp == g[f"fp_{name}_{mode}"].tolist()
            assert fn == g[f"fn_{name}_{mode}"].tolist()


def test_knn_f64_oracle_against_torch_float64_topk():
    """The float64 definition of the flat search (what stands in for faiss's GpuIndexFlatIP / L2) against an
    independent implementation: torch's float64 matmul / cdist + topk.  Random data has no exact ties, so positions must agree."""
    import torch
    M, D, nq, k = 3000, 96, 64, 30
    bank = gi.unit_bank(M, D, seed=21)
    q = gi.vit_like_queries(nq, D, seed=22)
    b64, q64 = torch.from_numpy(bank).double(), torch.from_numpy(q).double()
    idx, dist = oracle.knn_f64(q, bank, k)
    s, i = (q64 @ b64.T).topk(k, dim=1)
    assert np.array_equal(idx, i.numpy()) and np.abs(dist - s.numpy()).max() < 1e-12
    idx, dist = oracle.knn_f64(q, bank, k, "l2")
    d2 = ((q64[:, None, :] - b64[None, :, :]) ** 2).sum(-1)
    s, i = d2.topk(k, dim=1, largest=False)
    assert np.array_equal(idx, i.numpy()) and np.abs(dist - s.numpy()).max() < 1e-9
    # the fp32 chain oracle returns the same SET except at near-ties of fp32 rounding (profiles/LABBOOK.md: 97.9 % ordered at cfg-2 scale)
    idx32, _ = oracle.knn_chain_f32(q, bank, k, "l2")
    assert np.mean([len(set(a) & set(b)) for a, b in zip(idx32, idx)]) > k - 0.5


def test_create_memory_with_two_patch_sizes_golden_g10(golden_dir):
    """G10: the reference's _create_memory over training batches of two input sizes (patch_size recomputed per batch, hbird_eval.py:313-314).
    The oracle's restatement of one batch -- 255 -> 0, patch label histogram with THAT batch's patch size, eps-free normalisation of the
    tokens -- concatenated in loader order is the reference's bank, bit for bit in the labels."""
    g = np.load(os.path.join(golden_dir, "g10_mixed_patch_sizes.npz"))
    C, D, S, B, k = g["cfg"].tolist()
    feats, labs = [], []
    for i in range(4):
        y = np.round(g[f"train_y_{i}"] * 255).astype(np.int64)
        y[y == 255] = 0
        ps = y.shape[-1] // S
        labs.append(oracle.patch_label_hist(y, ps, C).reshape(-1, C))
        feats.append(oracle.normalize_rows(g[f"train_tok_{i}"].reshape(-1, D)))
    assert {labs[0].max() * 64 % 1, labs[1].max() * 256 % 1} == {0.0}          # values j / 64 and j / 256
    assert np.array_equal(np.concatenate(labs), g["label_memory"])
    assert np.abs(np.concatenate(feats) - g["feature_memory"]).max() <= 2.5e-7


def _definition_by_torch_float64(q, bank, k, metric):
    """The flat search's definition, independent of oracle/: scores by torch float64 (matmul / explicit squared differences), order by
    numpy lexsort on (score best-first, id ascending) -- torch.topk promises no order among equal values."""
    import torch
    b64, q64 = torch.from_numpy(bank).double(), torch.from_numpy(q).double()
    if metric == "dot_product":
        sc = (q64 @ b64.T).numpy(); key = -sc
    else:
        sc = torch.stack([((qq[None, :] - b64) ** 2).sum(-1) for qq in q64]).numpy(); key = sc
    ids = np.arange(bank.shape[0])
    order = np.stack([np.lexsort((ids, key[r]))[:k] for r in range(q.shape[0])])
    return order, np.take_along_axis(sc, order, axis=1)


@pytest.mark.parametrize("D", [384, 768, 1024])
@pytest.mark.parametrize("k", [30, 90])
@pytest.mark.parametrize("metric", ["dot_product", "l2"])
def test_knn_definition_pinned_by_torch_float64_at_the_baseline_widths(D, k, metric):
    """the golden fixture G4 runs the reference's plumbing around a stand-in backend that answers with the oracle's own
    knn_f64, so it cannot pin the search itself.  Here the definition is pinned independently at every width and k the BASELINE configs
    use, both metrics: oracle.knn_f64 must equal torch-float64 scores ordered by (score, id), and the fp32 chain oracle -- the bit-exact
    target of the HIP kernel -- must return the same neighbours except where fp32 rounding swaps near-ties."""
    M, nq = 4000, 24
    bank = gi.unit_bank(M, D, seed=100 + D)
    q = gi.vit_like_queries(nq, D, seed=200 + k)
    want_i, want_s = _definition_by_torch_float64(q, bank, k, metric)
    idx, dist = oracle.knn_f64(q, bank, k, metric)
    assert np.array_equal(idx, want_i) and np.abs(dist - want_s).max() < 1e-9 * max(1.0, np.abs(want_s).max())
    i32, d32 = oracle.knn_chain_f32(q, bank, k, metric)
    assert np.mean([len(set(a) & set(b)) for a, b in zip(i32, want_i)]) > k - 0.6
    assert np.abs(d32.astype(np.float64) - np.take_along_axis(
        (q.astype(np.float64) @ bank.astype(np.float64).T) if metric == "dot_product" else
        ((q.astype(np.float64)[:, None, :] - bank.astype(np.float64)[None, :, :]) ** 2).sum(-1), i32, axis=1)).max() < 2e-6 * max(1.0, np.abs(want_s).max()) * D ** 0.5


@pytest.mark.parametrize("metric", ["dot_product", "l2"])
def test_knn_definition_exact_ties_lower_id_first(metric):
    """Tie order is part of THIS engine's definition (ties -> lower id; Faiss-GPU's order among equal distances is unspecified and has never
    been observed here): small-integer rows with many exact duplicates make every score exact in fp32 and float64 alike, so the float64
    oracle, the fp32 chain oracle and the independent torch-float64 + lexsort definition must agree id for id."""
    rng = np.random.default_rng(9)
    M, D, nq, k = 1500, 48, 40, 30
    base = rng.integers(-3, 4, size=(60, D)).astype(np.float32)
    bank = base[rng.integers(0, 60, size=M)]                      # ~25 exact copies of each of 60 rows
    q = rng.integers(-2, 3, size=(nq, D)).astype(np.float32)
    want_i, want_s = _definition_by_torch_float64(q, bank, k, metric)
    for fn in (oracle.knn_f64, oracle.knn_chain_f32):
        idx, dist = fn(q, bank, k, metric)
        assert np.array_equal(idx, want_i), fn.__name__
        assert np.array_equal(dist.astype(np.float64), want_s), fn.__name__
    assert (np.diff(want_i, axis=1)[np.diff(want_s, axis=1) == 0] > 0).all()      # inside a tie the ids ascend


def test_knn_oracles_non_finite_scores_never_enter_a_list():
    """The rule the kernels are held to (tests/test_edge_gpu.py), stated on the CPU: a NaN or -inf score is never listed, +inf is an
    ordinary best score, fewer than k listed rows leave id -1 / -inf (IP), +inf (L2) -- against a numpy restatement."""
    rng = np.random.default_rng(5)
    M, D, nq, k = 400, 16, 12, 10
    bank = gi.unit_bank(M, D, seed=31)
    bank[[3, 77, 399]] = np.nan                          # a zero token through the eps-free normalisation (hbird_eval.py:324)
    bank[:, 5] = np.abs(bank[:, 5]) + 1e-3
    q = gi.vit_like_queries(nq, D, seed=32)
    q[1, 2] = np.nan; q[2, 5] = np.inf; q[3, 5] = -np.inf; q[4, 0] = np.inf
    for fn, dt in ((oracle.knn_chain_f32, np.float32), (oracle.knn_f64, np.float64)):
        idx, dist = fn(q, bank, k)
        with np.errstate(invalid="ignore", over="ignore"):
            sc = (q.astype(np.float64) @ bank.astype(np.float64).T)
        for r in range(nq):
            ok = np.flatnonzero(sc[r] > -np.inf)         # NaN compares false
            order = ok[np.lexsort((ok, -sc[r][ok]))][:k]
            want = np.full(k, -1); want[:len(order)] = order
            if r in (2, 4):                              # +inf scores tie: lower ids first, and only rows whose product is +inf
                assert np.isposinf(dist[r][idx[r] >= 0]).all()
            if np.isfinite(sc[r][ok]).all() or r in (2, 3):
                assert np.array_equal(idx[r] >= 0, want >= 0), (fn.__name__, r)
                if r not in (2, 4):
                    assert set(idx[r][idx[r] >= 0]) == set(want[want >= 0])
        assert (idx[1] == -1).all() and np.isneginf(dist[1]).all()          # NaN query: nothing
        assert (idx[3] == -1).all()                                          # every score -inf: nothing
        assert (idx[2] == np.arange(k) + (np.arange(k) >= 3)).all()          # all +inf: lowest ids, the NaN row 3 skipped
        assert not np.isin(idx, [3, 77, 399]).any()
