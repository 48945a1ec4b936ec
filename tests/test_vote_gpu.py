"""hb_knn_vote and hb_vote_counts (include/hbird_hip_vote.h) on the GPU against tests/vote_refs.py.

Counting worlds: all scores of a query are equal, so every e is expf(0) = 1.0f, votes are small integers (exact in fp32 and in the float64
model alike) and class ties are frequent: predictions AND votes equal the model's everywhere, no exclusions.

Gaussian world: the votes are held to the float64 model within a bound, the predictions outside an exemption that the bound defines.

THE BOUND on a vote, per query and configuration (k, T), first order in U = 2^-24, from the operation sequence of the header:
  * logit_j = s_j / T: one fp32 division (the temperature's own conversion to fp32 is in the model too) -- U |logit_j|; the same for mx;
  * e_j = expf(logit_j - mx): the subtraction rounds at U |logit_j - mx| <= U spread, expf adds about 2 U relative and its argument
    reduction another U spread: relative to e_j, delta_j <= U (2 max|logit| + 2 spread + 2);
  * the chain of a class with m positions: m - 1 additions, each U relative to a partial sum: (m - 1) U relative, m <= k.
  So a vote v of m terms moves by at most v U (2 max|logit| + 2 spread + m + 1).  The test asserts the form of
  propagate_refs.aggregate_bound with unit labels, U (2 max|logit| + 2 spread + 2 k + 6) per query over the list cut to k columns
  (vote_refs.vote_bound; test_vote_cpu.py holds the two functions to each other).  For a vote up to 1 that is the derived bound with room to
  spare.  For a larger vote -- a class with many near neighbours at T = 1.0 reaches 36 in this world -- it is TIGHTER than the derivation,
  which grows with v: the assertion is the stricter of the two, never the wider.  The ratio each configuration reaches is printed before it
  is asserted; the worst on these seeds is 0.84 (seed 2, k = 20, T = 1.0)."""
import functools

import numpy as np
import pytest
import torch

import vote_refs as R
from hbird_mi import _lib, ops

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.tensor(a).cuda()


def run(idx, score, labels, C, ks, temps, topn, id_base=0, want_votes=True):
    return ops.knn_vote(dev(idx), dev(score), dev(labels), C, ks, temps, topn=topn, id_base=id_base, want_votes=want_votes)


# ---- counting worlds: bit-exact --------------------------------------------------------------------------------------------------------------
COUNT_KS = {5: (1, 2, 5), 70: (1, 7, 64, 65, 70), 300: (3, 64, 256, 257, 300)}      # around a wave, a lane round and the list's end
ID_BASE = {5: 0, 70: 1000, 300: 1 << 33}


@functools.lru_cache(maxsize=None)
def counting_case(k_list, C):
    idx, score, labels = R.counting_world(k_list * 10 + C, 37, k_list, C, id_base=ID_BASE[k_list])
    want = {topn: R.grid(idx, score, labels, C, COUNT_KS[k_list], (0.07, 1.0), topn, id_base=ID_BASE[k_list]) for topn in (1, 5, 8)}
    for a in (idx, score, labels):
        a.setflags(write=False)
    return idx, score, labels, want


@pytest.mark.parametrize("topn", [1, 5, 8])
@pytest.mark.parametrize("C", [3, 1000])
@pytest.mark.parametrize("k_list", [5, 70, 300])
def test_counting_world_equals_the_model(cuda_device, k_list, C, topn):
    idx, score, labels, want = counting_case(k_list, C)
    ks, base = COUNT_KS[k_list], ID_BASE[k_list]
    cls = R.classes(idx, labels, base)
    assert (idx == -1).any() and (labels < 0).any() and (cls[3] == -1).all() and (idx[3] >= 0).any(), "tails, unlabelled rows, an all-unlabelled list"
    assert ((idx >= 0) & ((idx - base < 0) | (idx - base >= labels.shape[0]))).any(), "ids outside [id_base, id_base + n_rows)"
    pred, votes = run(idx, score, labels, C, ks, (0.07, 1.0), topn, id_base=base)
    assert pred.shape == votes.shape == (len(ks) * 2, 37, topn) and pred.dtype == torch.int32
    pred, votes = pred.cpu().numpy(), votes.cpu().numpy()
    ties = 0
    for cfg, (p_ref, v_ref) in enumerate(want[topn]):
        assert np.array_equal(pred[cfg], p_ref), f"cfg {cfg}: {(pred[cfg] != p_ref).sum()} predictions differ from the model's"
        assert np.array_equal(u32(votes[cfg]), u32(v_ref.astype(np.float32))), f"cfg {cfg}: vote bits differ from the model's"
        assert np.array_equal(v_ref, np.round(v_ref)), "votes of a counting world are integers"
        ties += int(((v_ref[:, :-1] == v_ref[:, 1:]) & (p_ref[:, 1:] >= 0)).sum()) if topn > 1 else 0
    assert (pred[:, 3] == -1).all() and (pred[:, 5] == -1).all() and not votes[:, 3].any(), "nothing takes part: all -1 / 0"
    if topn > 1 and k_list > 5:
        assert ties > 20, "the world has too few class ties to see the tie rule"
    if topn == 8 and C == 3:
        assert (pred[:, :, 3:] == -1).all() and not votes[:, :, 3:].any(), "three classes: the tail of eight slots is -1 / 0.0"


@pytest.mark.parametrize("k_list,ks", [(600, (1, 256, 257, 512, 513, 600)), (2048, (255, 1024, 2047, 2048))])
def test_long_lists_equal_the_model(cuda_device, k_list, ks):
    """Beyond 512 positions a thread holds eight of them (the kernel's third instantiation), up to the limit of 2048."""
    idx, score, labels = R.counting_world(k_list, 9, k_list, 40, id_base=7)
    pred, votes = run(idx, score, labels, 40, ks, (0.07, 1.0), 8, id_base=7)
    for cfg, (p_ref, v_ref) in enumerate(R.grid(idx, score, labels, 40, ks, (0.07, 1.0), 8, id_base=7)):
        assert np.array_equal(pred[cfg].cpu().numpy(), p_ref), f"cfg {cfg}: predictions differ from the model's"
        assert np.array_equal(u32(votes[cfg]), u32(v_ref.astype(np.float32))), f"cfg {cfg}: vote bits differ from the model's"
    assert float(votes.max()) >= 16, "forty classes over hundreds of positions: chains of sixteen terms and more"
    with pytest.raises(_lib.HbirdHipError, match="limit"):
        ops.knn_vote(torch.zeros((2, 2049), dtype=torch.int64).cuda(), torch.zeros((2, 2049)).cuda(), dev(labels), 40, (1,), (0.07,))


# ---- the Gaussian world ------------------------------------------------------------------------------------------------------------------------
G_KS, G_TS, G_C, G_KLIST = (1, 5, 20, 70), (0.07, 1.0), 10, 70


@functools.lru_cache(maxsize=None)
def gaussian_case(seed):
    bank, labels, q, qlabels = R.gaussian_world(seed)
    idx, score = R.lists(q, bank, G_KLIST)
    model = []
    for k in G_KS:
        for T in G_TS:
            v, present = R.vote(idx, score, labels, G_C, k, T)
            bound = R.vote_bound(idx, score, labels, k, T)
            model.append((k, T, v, present, bound, R.top(v, present, 5), R.exempt(v, present, bound)))
    for a in (idx, score, labels, qlabels):
        a.setflags(write=False)
    return idx, score, labels, qlabels, model


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gaussian_world_against_the_float64_model(cuda_device, seed):
    idx, score, labels, qlabels, model = gaussian_case(seed)
    assert idx.shape == (203, 70) and labels.shape == (600,) and (idx >= 0).all()
    pred, votes = run(idx, score, labels, G_C, G_KS, G_TS, 5)
    pred, votes = pred.cpu().numpy(), votes.cpu().numpy().astype(np.float64)
    assert len(model) == pred.shape[0] == 8
    for cfg, (k, T, v, present, bound, (p_ref, v_ref), ex) in enumerate(model):
        c, _, n = R.counts(p_ref, qlabels, G_C)
        if k >= 5:      # the world is imperfect, so a wrong rule shows: to two decimals top-1 spans 0.43 .. 0.70, top-5 0.81 .. 0.99 (k = 1 has one class)
            assert 0.43 <= round(c[0] / n, 2) <= 0.70 and 0.81 <= round(c[4] / n, 2) <= 0.99, (k, T, c / n)
        same = (pred[cfg] == p_ref).all(axis=1)
        err = np.abs(votes[cfg] - v_ref).max(axis=1)
        print(f"seed {seed} k={k} T={T}: top1 {c[0] / n:.3f} top5 {c[4] / n:.3f}, worst |vote - model| / bound = {np.max(err[same] / bound[same]):.3f}, "
              f"exempt {int(ex.sum())}, predictions that differ {int((~same).sum())}")
        assert ex.sum() <= 0.02 * ex.size, f"{ex.sum()} exempt queries: more than 2 %"
        assert (same | ex).all(), f"k={k} T={T}: {(~same & ~ex).sum()} predictions differ from the model's outside the exemption"
        assert (err[same] <= bound[same]).all(), f"k={k} T={T}: {(err[same] > bound[same]).sum()} queries beyond the bound"
        # a ranked vote of an exempt query still lies within the bound of the model's vote of the class the engine ranked there
        for i in np.flatnonzero(~same):
            got_c = pred[cfg][i]
            assert (np.abs(votes[cfg][i][got_c >= 0] - v[i][got_c[got_c >= 0]]) <= bound[i]).all()


def test_every_configuration_has_the_bits_of_its_own_call(cuda_device):
    idx, score, labels, _, _ = gaussian_case(1)
    ks, temps = (1, 5, 20, 70), (0.05, 0.07, 0.5, 1.0)
    pred, votes = run(idx, score, labels, G_C, ks, temps, 5)
    assert pred.shape[0] == 16 == _lib.VOTE_MAX_CONFIGS
    again_p, again_v = run(idx, score, labels, G_C, ks, temps, 5)
    assert torch.equal(pred, again_p) and np.array_equal(u32(votes), u32(again_v)), "two calls give the same bits"
    plain = run(idx, score, labels, G_C, ks, temps, 5, want_votes=False)
    assert torch.equal(pred, plain), "the predictions do not depend on the optional output"
    for ik, k in enumerate(ks):
        for it, T in enumerate(temps):
            p1, v1 = run(np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(score[:, :k]), labels, G_C, (k,), (T,), 5)
            cfg = ik * len(temps) + it
            assert torch.equal(pred[cfg], p1[0]) and np.array_equal(u32(votes[cfg]), u32(v1[0])), (k, T)


def test_refusals_before_any_launch(cuda_device):
    idx, score, labels, _, _ = gaussian_case(1)
    for kw, word in ((dict(ks=(5, 5)), "ascending"), (dict(ks=(5, 71)), "k_list"), (dict(temps=(0.0,)), "temperature"), (dict(topn=9), "topn"),
                     (dict(C=0), "C must"), (dict(ks=tuple(range(1, 18))), "configurations")):
        args = dict(ks=(1, 5), temps=(0.07,), topn=5, C=G_C)
        args.update(kw)
        with pytest.raises(_lib.HbirdHipError, match=word):
            run(idx, score, labels, args["C"], args["ks"], args["temps"], args["topn"])
    empty = ops.knn_vote(dev(idx[:0]), dev(score[:0]), dev(labels), G_C, (1,), (0.07,))
    assert empty.shape == (1, 0, 5)


# ---- the counts ----------------------------------------------------------------------------------------------------------------------------------
def _tables(n_cfg, topn, C):
    return (torch.zeros((n_cfg, topn), dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int64).cuda(),
            torch.zeros((n_cfg, C, 2), dtype=torch.int64).cuda())


@pytest.mark.parametrize("topn", [1, 5])
def test_counts_equal_the_model_and_accumulate(cuda_device, topn):
    idx, score, labels, qlabels, _ = gaussian_case(2)
    qlabels = qlabels.copy()
    qlabels[::7] = -1                                        # counted nowhere
    pred = run(idx, score, labels, G_C, G_KS, G_TS, topn, want_votes=False)
    pred_h = pred.cpu().numpy()
    counts, n, per = _tables(8, topn, G_C)
    ops.vote_counts(pred, dev(qlabels), G_C, counts, n, per)
    for cfg in range(8):
        c, pc, nn = R.counts(pred_h[cfg], qlabels, G_C)
        assert np.array_equal(counts[cfg].cpu().numpy(), c) and np.array_equal(per[cfg].cpu().numpy(), pc) and int(n) == nn == (qlabels >= 0).sum()
    # two accumulated batches equal one call on their concatenation; class_io_opt NULL leaves the rest as it is
    c2, n2, _ = _tables(8, topn, G_C)
    cut = 77
    ops.vote_counts(pred[:, :cut].contiguous(), dev(qlabels[:cut]), G_C, c2, n2)
    ops.vote_counts(pred[:, cut:].contiguous(), dev(qlabels[cut:]), G_C, c2, n2)
    assert torch.equal(c2, counts) and torch.equal(n2, n)
    ops.vote_counts(pred, dev(qlabels), G_C, c2, n2)
    assert torch.equal(c2, 2 * counts) and int(n2) == 2 * int(n)
    bad = qlabels.copy()
    bad[11] = G_C
    before = c2.clone()
    with pytest.raises(ValueError, match="query label"):
        ops.vote_counts(pred, dev(bad), G_C, c2, n2)
    assert torch.equal(c2, before), "a refused call counts nothing"
