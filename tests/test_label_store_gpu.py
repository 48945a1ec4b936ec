"""The label table's transitions that no other GPU test walks (csrc/hbird_labels.h, csrc/hbird_labels.hip): a borrowed table on an index that
holds covering own rows of another content -- fp32, then counts, then given back -- and hb_index_add_from into an emptied destination whose
previous label rows had the other storage form and another class count.  Expectations come from freshly built indexes and numpy, never from the
index under test.  (C, P) = (21, 0): fp32 rows, K5's group form; (151, 196): count rows of the padded stride 152, the 16-byte gather."""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

D, N, NQ, K, BETA = 32, 300, 64, 8, 0.2
# K5 in fp32 against float64: the softmax's argument cos / beta is at most 1 / beta in size and allowed 8 ulp (the division by the norms'
# product, the one by beta, expf's own error), which a weight carries as a relative error and the normalisation doubles; the sums of the
# weights and of k weighted values <= 1 add an ulp of 1 per term
TOL = (2 * 8 / BETA + K + 2) * 2.0 ** -24
FORMS = [(21, 0), (151, 196)]


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _world():
    rng = np.random.default_rng(2027)
    x = rng.standard_normal((N, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((NQ, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return x, q


def _labels(C, seed):
    return gi.labels_from_masks(N, C, 196, seed=seed)      # values j / 196: storable as fp32 and as counts of 196


def _index(x, lab, C, P):
    ix = HipFlatIndex(D, 0, 0)
    if P:
        ix.set_label_denominator(P)
    ix.add(torch.from_numpy(x).cuda(), normalize=False)
    if lab is not None:
        ix.add_labels(torch.from_numpy(lab).cuda()); ix.set_num_classes(C)
    return ix


@pytest.mark.parametrize("C,P", FORMS)
def test_borrowed_tables_are_read_while_borrowed_and_the_own_rows_after(cuda_device, C, P):
    x, q = _world()
    own, other = _labels(C, 1), _labels(C, 2)
    counts = torch.from_numpy(np.rint(other.astype(np.float64) * 196).astype(np.uint16).view(np.int16)).cuda()
    assert np.array_equal((counts.cpu().numpy().view(np.uint16).astype(np.float32) / np.float32(196)), other)
    qd = torch.from_numpy(q).cuda()
    ix = _index(x, own, C, P)
    idx, dist = ix.search(qd, K)
    norms = ix.copy_norms()
    # the expectations: a fresh index with the own rows, and fresh ones without label rows that borrow each table
    want_own = _index(x, own, C, P).aggregate(qd, idx, dist, BETA)
    fresh32 = _index(x, None, C, 0)
    fresh32.set_label_table(torch.from_numpy(other).cuda(), fresh32.copy_norms())
    want32 = fresh32.aggregate(qd, idx, dist, BETA)
    fresh16 = _index(x, None, C, 0)
    fresh16.set_label_count_table(counts, fresh16.copy_norms(), 196)
    want16 = fresh16.aggregate(qd, idx, dist, BETA)
    # ... which numpy confirms to be the two contents (float64 softmax over cosines / beta; unit rows: the score is the cosine)
    w = np.exp((dist.cpu().numpy().astype(np.float64) - 1.0) / BETA)
    w /= w.sum(axis=1, keepdims=True)
    for got, lab in ((want_own, own), (want32, other), (want16, other)):
        ref = np.einsum("qk,qkc->qc", w, lab[idx.cpu().numpy()].astype(np.float64))
        assert np.abs(got.cpu().numpy() - ref).max() < TOL      # (5.4e-6; the two contents differ by tenths)
    assert not np.array_equal(_bits(want_own), _bits(want32))

    assert np.array_equal(_bits(ix.aggregate(qd, idx, dist, BETA)), _bits(want_own))
    ix.set_label_table(torch.from_numpy(other).cuda(), norms)
    assert np.array_equal(_bits(ix.aggregate(qd, idx, dist, BETA)), _bits(want32))
    ix.set_label_count_table(counts, norms, 196)
    assert np.array_equal(_bits(ix.aggregate(qd, idx, dist, BETA)), _bits(want16))
    ix.set_label_table(None, None)
    assert np.array_equal(_bits(ix.aggregate(qd, idx, dist, BETA)), _bits(want_own))
    assert np.array_equal(_bits(ix.search_aggregate(qd, K, BETA)), _bits(want_own))
    assert np.array_equal(_bits(ix.gather_labels(torch.arange(N, device="cuda"))), own.view(np.int32))      # the own rows were never touched
    assert ix.label_denominator == P


@pytest.mark.parametrize("C,P", FORMS)
def test_add_from_into_an_emptied_index_of_the_other_form_and_class_count(cuda_device, C, P):
    x, q = _world()
    qd = torch.from_numpy(q).cuda()
    lab = _labels(C, 3)
    src = _index(x, lab, C, P)
    (C0, P0), = [f for f in FORMS if f != (C, P)]
    dst = _index(x, _labels(C0, 4), C0, P0)      # 300 rows of the other form: its buffer would seem to "fit" what follows
    dst.reset()
    rng = np.random.default_rng(5)
    ids = rng.integers(0, N, size=200)
    ids[:3] = (N - 1, 0, N - 1)
    dst.add_from(src, torch.from_numpy(ids[:120]))            # adopts (C, P), drops the old buffer
    dst.add_from(src, torch.from_numpy(ids[120:]).cuda())     # appends to rows of its own form now
    fresh = _index(x[ids], lab[ids], C, P)
    assert dst.ntotal == 200 and dst.num_classes == C and dst.label_denominator == P
    every = torch.arange(200, device="cuda")
    assert np.array_equal(_bits(dst.gather_labels(every)), lab[ids].view(np.int32))
    assert np.array_equal(_bits(fresh.gather_labels(every)), lab[ids].view(np.int32))
    if P:
        want = np.rint(lab[ids].astype(np.float64) * P).astype(np.uint16)
        assert np.array_equal(dst.copy_label_counts().cpu().numpy().view(np.uint16), want)
    want_hat, want_idx, want_dist = fresh.search_aggregate(qd, K, BETA, want_neighbours=True)
    hat, idx, dist = dst.search_aggregate(qd, K, BETA, want_neighbours=True)
    assert np.array_equal(idx.cpu().numpy(), want_idx.cpu().numpy()) and np.array_equal(_bits(dist), _bits(want_dist))
    assert np.array_equal(_bits(hat), _bits(want_hat))
