"""Sub-bank views, the host side (no GPU): the row lists of hbird_mi/views.py, the nesting claim they rest on, and the C-ABI surface of
hb_index_add_from / hb_index_select_rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bank_refs as R
import oracle
from hbird_mi import _lib
from hbird_mi.views import per_image_rows, view_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_per_image_rows_is_the_reference_rule():
    """max(1, memory_size // max(1, dataset_size * augmentation_epoch)), hbird_eval.py:146-147."""
    for m, ds, aug in ((102400, 10582, 1), (1024000, 10582, 1), (10240000, 10582, 2), (24 * 40, 24, 1), (24 * 9, 24, 2), (5, 24, 1), (0, 24, 1),
                       (100, 0, 1), (7, 1, 7)):
        assert per_image_rows(m, ds, aug) == max(1, m // max(1, ds * aug))
    assert per_image_rows(102400, 10582, 1) == 9 and per_image_rows(5, 24, 1) == 1 and per_image_rows(0, 24, 3) == 1    # the floors
    assert per_image_rows(100, 0, 1) == 100                                                                              # max(1, denom)
    assert per_image_rows(24 * 40, 24) == 40                                                                             # one epoch by default


def _naive(starts, per_block=None, blocks=None):
    n = len(starts) - 1
    keep = range(n) if blocks is None else sorted(blocks)
    out = []
    for b in keep:
        length = starts[b + 1] - starts[b]
        take = length if per_block is None else min(per_block, length)
        out.extend(range(starts[b], starts[b] + take))
    return out


def test_view_rows_against_a_naive_loop():
    ragged = [0, 5, 5, 12, 13, 20, 49, 50]          # blocks of 5, 0, 7, 1, 7, 29, 1 rows
    even = list(range(0, 49 * 6 + 1, 49))
    for starts in (ragged, even):
        n = len(starts) - 1
        for per_block in (None, 0, 1, 3, 7, 1000):                     # 1000: larger than every block
            for blocks in (None, [], [n - 1, 0, 2], [3], list(range(n))[::-1]):   # out of order; empty selection
                got = view_rows(starts, per_block=per_block, blocks=blocks)
                assert got.dtype == torch.int64 and got.dim() == 1
                assert got.tolist() == _naive(starts, per_block, blocks), (starts, per_block, blocks)
    assert view_rows([0]).numel() == 0 and view_rows([0, 0, 0], per_block=4).numel() == 0
    assert view_rows(torch.tensor(even), per_block=7).tolist() == _naive(even, 7)     # the selection of the GPU tests: blocks of 49, first 7
    with pytest.raises(ValueError):
        view_rows(even, blocks=[1, 3, 1])            # a block listed twice
    with pytest.raises(ValueError):
        view_rows(even, blocks=[6])
    with pytest.raises(ValueError):
        view_rows(even, blocks=[-1])
    with pytest.raises(ValueError):
        view_rows([0, 4, 2])
    with pytest.raises(ValueError):
        view_rows(even, per_block=-1)


def _label_world(seed, with_empty):
    """B = 4 images of S x S = 36 patches of 2 x 2 pixels, C = 5.  with_empty: whole patches of the value that the soft labels cannot hold
    (label rows of zeros, as hbird_eval.py:490 sees a patch without any class)."""
    rng = np.random.default_rng(seed)
    B, S, C, ps = 4, 6, 5, 2
    y = rng.integers(0, C, size=(B, 1, S * ps, S * ps), dtype=np.int64)
    y[:, :, : 2 * ps] = 1                  # two patch rows of one class: equal scores before the noise
    lab = R.label_hist(y, ps, C).reshape(B, S * S, C)
    if with_empty:
        empty = rng.random((B, S * S)) < 0.25
        empty[0, :5] = True
        lab[empty] = 0.0
    return y, lab, B, S, C, ps


def test_bounded_selection_for_a_smaller_k_is_a_prefix_of_the_bigger_one():
    """The nesting claim memory_view(memory_size=) rests on: the noise does not depend on K, the K smallest in ascending order with ties to the
    lower patch index are the first K of the K' >= K smallest (hbird_eval.py:497-511).  Quantised noise makes many noisy scores tie."""
    # oracle.py's restatement (it indexes by class id: no empty patches)
    y, lab, B, S, C, ps = _label_world(3, with_empty=False)
    pt = oracle.patchify_gt(y, ps)
    nz = int(oracle.sample_num_nonempty(pt, C).sum())
    assert nz == B * S * S
    r = np.random.default_rng(4).choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=nz)
    big, noisy = oracle.sample_patches(pt, C, 11, r)
    small, noisy3 = oracle.sample_patches(pt, C, 3, r)
    assert np.array_equal(noisy, noisy3)
    picked = np.take_along_axis(noisy, big, axis=1)
    assert (picked[:, 1:] == picked[:, :-1]).any(), "the world holds no tied scores among the selected patches"
    assert big.shape == (B, 11) and small.shape == (B, 3) and np.array_equal(small, big[:, :3])
    for K in range(1, 12):
        assert np.array_equal(oracle.sample_patches(pt, C, K, r)[0], big[:, :K])
    # ... and the label-row restatement (tests/bank_refs.py), which can express empty patches: they draw no noise and sort last
    y, lab, B, S, C, ps = _label_world(5, with_empty=True)
    scores, nonempty, nzc, _ = R.patch_scores(lab)
    assert (nonempty == 0).any() and int(nzc.sum()) < B * S * S
    r = np.random.default_rng(6).choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=int(nzc.sum()))
    r_off = np.concatenate([[0], np.cumsum(nzc)[:-1]])
    big, noisy = R.patch_select(scores, nonempty, r, r_off, 11)
    small, _ = R.patch_select(scores, nonempty, r, r_off, 3)
    picked = np.take_along_axis(noisy, big, axis=1)
    assert (picked[:, 1:] == picked[:, :-1]).any()
    assert np.array_equal(small, big[:, :3])
    # in bank rows: image b's block of 11 starts at 11 b, the bank for K = 3 is view_rows' prefix selection of the bank for K = 11
    rows_big = (big + np.arange(B)[:, None] * S * S).reshape(-1)
    rows_small = (small + np.arange(B)[:, None] * S * S).reshape(-1)
    ids = view_rows(np.arange(B + 1) * 11, per_block=3).numpy()
    assert np.array_equal(rows_big[ids], rows_small)


def test_view_entries_are_declared_exported_and_bound():
    L = _lib.lib()
    names = {"hb_index_add_from", "hb_index_select_rows"}
    assert set(_lib.SIGNATURES_SELECT) == names
    header = open(os.path.join(ROOT, "include", "hbird_hip_select.h")).read()
    assert set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", header)) == names
    assert '#include "hbird_hip_select.h"' in open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes == _lib.SIGNATURES_SELECT[n][1] and n in doc
    # a NULL handle is an error, never a dereference (no GPU is touched)
    out = ctypes.c_void_p()
    assert L.hb_index_add_from(None, None, None, 1, 0) != 0 and b"NULL" in L.hb_last_error()
    assert L.hb_index_select_rows(None, None, 1, 0, ctypes.byref(out)) != 0 and b"NULL" in L.hb_last_error() and not out.value
    assert L.hb_index_select_rows(None, None, 1, 0, None) != 0 and b"NULL" in L.hb_last_error()
    from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex
    from hbird_mi.hbird_eval import HbirdEvaluation, hbird_evaluation
    import inspect
    assert callable(HipFlatIndex.add_from) and callable(HipFlatIndex.select_rows) and callable(HipMultiIndex.select_rows)
    assert list(inspect.signature(HbirdEvaluation.memory_view).parameters)[1:] == ["memory_size", "images", "rows", "rows_per_image", "n_neighbours"]
    assert list(inspect.signature(hbird_evaluation).parameters)[-1] == "memory_sizes"
    with pytest.raises(ValueError, match="single-index"):
        HipMultiIndex.select_rows(object.__new__(HipMultiIndex), [0])


def test_row_ids_must_be_integers():
    """Float or bool ids are refused, not truncated (no GPU is touched)."""
    import numpy as np
    from hbird_mi.nn.search_hip import HipFlatIndex
    ix = object.__new__(HipFlatIndex)
    ix.device = 0
    for bad in (np.array([1.5]), [0.0, 1.0], torch.tensor([1.0]), torch.tensor([True, False]), np.array([True])):
        with pytest.raises(ValueError, match="integers"):
            ix._ids64(bad)
    for good, want in ((np.array([3, 1], dtype=np.int32), [3, 1]), ([2, 2], [2, 2]), (torch.tensor([[4], [5]], dtype=torch.int16), [4, 5]), ([], [])):
        on_dev, t = ix._ids64(good)
        assert not on_dev and t.dtype == torch.int64 and t.is_contiguous() and t.tolist() == want
    ix._h = None                 # (nothing to free)
