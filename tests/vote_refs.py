"""numpy restatement of include/hbird_hip_vote.h (image-level k-NN classification): plain numpy, no engine code.  `vote` works in float64 over
neighbour lists (those of `oracle.knn_chain_f32`: `lists`), `top` applies the ranking rule, `counts` does the counting.  `variant=` switches
ONE definition to a plausible wrong one; tests/test_vote_cpu.py holds each of them to a named check it must fail."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
VARIANTS = ("tie_high_class", "uniform_weights", "k_counts_labelled", "unlabelled_is_class0", "temperature_multiplies")


def lists(q, bank, k):
    """The exact inner-product lists (idx int64 [nq, k], score fp32 [nq, k]) with the engine's chain bits and lower-id ties."""
    import oracle
    return oracle.knn_chain_f32(q, bank, k, "dot_product")


def classes(idx, labels, id_base=0, variant=None):
    """[nq, k_list] int64: the class of every position that takes part, -1 elsewhere."""
    idx = np.asarray(idx, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    row = idx - id_base
    ok = (idx >= 0) & (row >= 0) & (row < labels.shape[0])
    lab = labels[np.where(ok, row, 0)]
    if variant == "unlabelled_is_class0":
        lab = np.where(lab < 0, 0, lab)
    return np.where(ok & (lab >= 0), lab, -1)


def _window(cls_row, k, variant):
    """The positions configuration k looks at: the first k POSITIONS of the list."""
    if variant == "k_counts_labelled":
        return np.flatnonzero(cls_row >= 0)[:k]
    return np.arange(min(k, cls_row.shape[0]))


def vote(idx, score, labels, C, k, T, id_base=0, variant=None, dtype=np.float64):
    """-> (votes [nq, C] `dtype`, present [nq, C] bool).  float64: the model; float32: the stated operation sequence restated in numpy
    (np.exp in the place of expf)."""
    cls = classes(idx, labels, id_base, variant)
    score = np.asarray(score, dtype=F32)
    nq = cls.shape[0]
    votes, present = np.zeros((nq, C), dtype=dtype), np.zeros((nq, C), dtype=bool)
    Tf = dtype(F32(T))
    for i in range(nq):
        pos = _window(cls[i], k, variant)
        pos = pos[cls[i][pos] >= 0]
        if not pos.size:
            continue
        s = score[i][pos].astype(dtype)
        logit = (s * Tf if variant == "temperature_multiplies" else s / Tf).astype(dtype)
        e = np.exp((logit - logit[0]).astype(dtype)).astype(dtype)
        if variant == "uniform_weights":
            e = np.ones_like(e)
        for j, c in enumerate(cls[i][pos]):                 # ascending j: the chain
            votes[i, c] = dtype(votes[i, c] + e[j])
            present[i, c] = True
    return votes, present


def top(votes, present, topn, variant=None):
    """The ranking: classes present, vote descending, ties to the LOWER class id -> (pred [nq, topn] int32, v [nq, topn]); tail -1 / 0."""
    nq, C = votes.shape
    pred = np.full((nq, topn), -1, dtype=np.int32)
    v = np.zeros((nq, topn), dtype=votes.dtype)
    for i in range(nq):
        cs = np.flatnonzero(present[i])
        tie = cs if variant == "tie_high_class" else -cs
        order = cs[np.lexsort((-tie, -votes[i][cs]))][:topn]           # last key first: vote descending, then the class
        pred[i, :order.size] = order
        v[i, :order.size] = votes[i][order]
    return pred, v


def predict(idx, score, labels, C, k, T, topn, id_base=0, variant=None, dtype=np.float64):
    votes, present = vote(idx, score, labels, C, k, T, id_base, variant, dtype)
    return top(votes, present, topn, variant)


def grid(idx, score, labels, C, ks, temps, topn, id_base=0, variant=None, dtype=np.float64):
    """[(pred, v)] in the configuration order cfg = ik * nt + it."""
    return [predict(idx, score, labels, C, k, T, topn, id_base, variant, dtype) for k in ks for T in temps]


def counts(pred, qlabels, C):
    """pred [nq, topn], qlabels [nq] (-1: counted nowhere) -> (counts [topn] int64, per_class [C, 2] int64, n)."""
    pred, qlabels = np.asarray(pred), np.asarray(qlabels, dtype=np.int64)
    topn = pred.shape[1]
    out, per = np.zeros(topn, dtype=np.int64), np.zeros((C, 2), dtype=np.int64)
    n = 0
    for i, lab in enumerate(qlabels):
        if lab < 0:
            continue
        n += 1
        per[lab, 0] += 1
        per[lab, 1] += int(pred[i, 0] == lab)
        for t in range(topn):
            out[t] += int(lab in pred[i, :t + 1])
    return out, per, n


def metrics(counts_row, per_class, n):
    """-> (top1, topn accuracy, mean per class over the classes that have queries), float64."""
    seen = per_class[:, 0] > 0
    return counts_row[0] / n, counts_row[-1] / n, float(np.mean(per_class[seen, 1] / per_class[seen, 0]))


def vote_bound(idx, score, labels, k, T, id_base=0):
    """Per query: U * (2 max|logit| + 2 spread + 2 k + 6) over the positions of the list cut to k columns that take part -- the bound of
    propagate_refs.aggregate_bound with unit labels (tests/test_vote_gpu.py states the derivation).  0 where nothing takes part."""
    cls = classes(idx, labels, id_base)[:, :k]
    score = np.asarray(score, dtype=F32)[:, :k]
    Tf = float(F32(T))
    out = np.zeros(cls.shape[0])
    for i in range(cls.shape[0]):
        keep = cls[i] >= 0
        if keep.any():
            logit = score[i][keep].astype(np.float64) / Tf
            out[i] = U * (2 * np.abs(logit).max() + 2 * (logit.max() - logit.min()) + 2 * cls.shape[1] + 6)
    return out


def exempt(votes, present, bound):
    """Queries at which a prediction may differ from the model's: two adjacent votes in the model's ranking of the classes present (all of
    them, not only the first topn) lie within the bound of each other."""
    out = np.zeros(votes.shape[0], dtype=bool)
    for i in range(votes.shape[0]):
        v = np.sort(votes[i][present[i]])
        out[i] = v.size > 1 and bool((np.diff(v) <= bound[i]).any())
    return out


# ---- worlds ------------------------------------------------------------------------------------------------------------------------------------
def gaussian_world(seed, n=600, nq=203, d=32, C=10, noise=2.5):
    """Class centroid + `noise` sigma of isotropic noise, rows normalised -> (bank [n, d], labels [n] int32, q [nq, d], qlabels [nq] int32)."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((C, d))
    labels, qlabels = rng.integers(0, C, n), rng.integers(0, C, nq)
    bank = cent[labels] + noise * rng.standard_normal((n, d))
    q = cent[qlabels] + noise * rng.standard_normal((nq, d))
    bank = (bank / np.linalg.norm(bank, axis=1, keepdims=True)).astype(F32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    return bank, labels.astype(np.int32), q, qlabels.astype(np.int32)


def counting_world(seed, nq, k_list, C, n_rows=5000, id_base=0):
    """All scores of a query are equal: every e is 1.0f, votes are integers, class ties are frequent.  Lists with -1 / -inf tails, unlabelled
    rows, ids outside [id_base, id_base + n_rows), query 3 with a list that is all unlabelled, query 5 with an empty list.
    -> (idx [nq, k_list] int64, score fp32, labels [n_rows] int32)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, n_rows).astype(np.int32)
    labels[rng.random(n_rows) < 0.1] = -1
    unl = np.flatnonzero(labels < 0)
    idx = rng.integers(0, n_rows, (nq, k_list)).astype(np.int64) + id_base
    out = rng.random((nq, k_list)) < 0.05
    idx[out] = np.where(rng.random(out.sum()) < 0.5, id_base + n_rows + rng.integers(0, 50, out.sum()), np.maximum(id_base - 1 - rng.integers(0, 50, out.sum()), 0))
    score = np.repeat((rng.integers(1, 9, nq) / 8.0).astype(F32)[:, None], k_list, axis=1)
    tail = rng.integers(0, k_list + 1, nq)                  # the list's length
    tail[::4] = k_list
    tail[3:4] = k_list
    for i in range(nq):
        idx[i, tail[i]:] = -1
        score[i, tail[i]:] = -np.inf
    if nq > 3:
        idx[3] = np.where(idx[3] >= 0, unl[rng.integers(0, unl.size, k_list)] + id_base, -1)
    if nq > 5:
        idx[5], score[5] = -1, -np.inf
    return idx, score, labels
