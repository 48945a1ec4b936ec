"""merge_sorted_parts_kernel (csrc/hbird_bigk.hip: hb_bigk_merge_topk / hb_bigk_merge_topk_packed) against bank_refs.merge, the numpy
restatement of the merge's definition, on shapes up to 16 x 2048 -- past the parts * k the LDS-staged hb_merge_topk takes.

Inputs are `merge_inputs` of tests/test_bank_paths_gpu.py brought into the form the new kernel's PRECONDITION names: every list sorted
best-first by (score descending / distance ascending, id ascending) with its missing entries (id < 0) at its tail only.  merge_inputs
leaves the "missing" pattern's -1 entries scattered through a list, so `sorted_lists` moves them to the tail (present entries keep
their order, the missing ones keep their junk scores), and `assert_precondition` checks every list on the host.

Ids are compared as integers, scores on bits; the plain entry, the packed one (minimal part_bytes and + 64), the Python wrappers (which
pick the old kernel while parts * k fits its staging) and, where the old kernel takes the shape, old against new.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import bank_refs as R
from test_bank_paths_gpu import MERGE_LDS, MergeCase, _dev, assert_bits, assert_ints, merge_inputs, merge_lds_bytes

pytestmark = pytest.mark.gpu

SHAPES = ((2, 257, 300), (8, 300, 300), (3, 2048, 2), (8, 1024, 64), (16, 2048, 1), (16, 30, 10000))      # (parts, k, nq)
PATTERNS = ("random", "interleaved", "equal", "zeros", "dup", "missing", "allmissing")


def sorted_lists(val, idx):
    """Missing entries to the tail of every list, everything else in place (a stable partition along k)."""
    order = np.argsort(idx < 0, axis=-1, kind="stable")
    return np.ascontiguousarray(np.take_along_axis(val, order, axis=-1)), np.ascontiguousarray(np.take_along_axis(idx, order, axis=-1))


def assert_precondition(val, idx, metric):
    miss = idx < 0
    assert not (miss[..., :-1] & ~miss[..., 1:]).any(), "a present entry follows a missing one"
    both = ~miss[..., 1:]                                   # pairs of present neighbours
    a, b = val[..., :-1], val[..., 1:]
    better = (a < b) if metric == 1 else (a > b)
    tie = (a == b) & (idx[..., :-1] <= idx[..., 1:])        # (-0.0 == +0.0)
    assert (better | tie | ~both).all(), "a list is not sorted by (score, id)"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _call(entry, *args):
    from hbird_mi import _lib
    assert entry(*args) == 0, _lib.last_error()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "p{}-k{}-nq{}".format(*s))
def test_sorted_merge_against_the_definition(cuda_device, shape, pattern):
    import torch
    from hbird_mi import _lib
    from hbird_mi.nn.search_hip import merge_topk, merge_topk_packed
    L = _lib.lib()
    parts, k, nq = shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for metric in (0, 1):
        c = MergeCase(metric, parts, k, nq, pattern)
        val, idx = sorted_lists(*merge_inputs(c, 900 + SHAPES.index(shape) * 10 + PATTERNS.index(pattern)))
        assert_precondition(val, idx, metric)
        if pattern == "missing":
            assert (idx[..., -1] < 0).all() and (idx[..., 0] >= 0).any()
        if pattern == "dup":
            assert np.array_equal(idx[0], idx[1])
        ridx, rval = R.merge(val, idx, metric)
        dval, didx = _dev(val), _dev(idx)
        # the plain entry
        gidx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        gval = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
        _call(L.hb_bigk_merge_topk, _ptr(dval), _ptr(didx), parts, nq, k, metric, _ptr(gidx), _ptr(gval), stream)
        assert_ints(gidx, ridx, f"sorted merge {c}: ids")
        assert_bits(gval, rval, f"sorted merge {c}: scores")
        # the old kernel, where it takes the shape
        if merge_lds_bytes(parts, k) <= MERGE_LDS:
            oidx, oval = torch.empty_like(gidx), torch.empty_like(gval)
            _call(L.hb_merge_topk, _ptr(dval), _ptr(didx), parts, nq, k, metric, _ptr(oidx), _ptr(oval), stream)
            assert torch.equal(oidx, gidx) and torch.equal(oval.view(torch.int32), gval.view(torch.int32)), f"{c}: old and new kernel differ"
        # the Python wrapper (old kernel while parts * k fits, the new one beyond)
        widx, wval = merge_topk(dval, didx, metric)
        assert_ints(widx, ridx, f"merge_topk {c}: ids")
        assert_bits(wval, rval, f"merge_topk {c}: scores")
        # packed lists: [nq * k int64 ids][nq * k fp32 scores], `part_bytes` apart -- minimal, and with 64 bytes of padding
        nk = nq * k
        least = int(L.hb_packed_list_bytes(nq, k))
        for part_bytes in (least, least + 64):
            raw = np.full((parts, part_bytes), 0xA5, dtype=np.uint8)
            for p in range(parts):
                raw[p, :nk * 8] = idx[p].reshape(-1).view(np.uint8)
                raw[p, nk * 8:nk * 12] = val[p].reshape(-1).view(np.uint8)
            draw = _dev(raw).view(-1)
            pidx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            pval = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
            _call(L.hb_bigk_merge_topk_packed, _ptr(draw), part_bytes, parts, nq, k, metric, _ptr(pidx), _ptr(pval), stream)
            assert_ints(pidx, ridx, f"packed sorted merge {c}, part_bytes {part_bytes}: ids")
            assert_bits(pval, rval, f"packed sorted merge {c}, part_bytes {part_bytes}: scores")
            widx, wval = merge_topk_packed(draw, part_bytes, parts, nq, k, metric)
            assert_ints(widx, ridx, f"merge_topk_packed {c}, part_bytes {part_bytes}: ids")
            assert_bits(wval, rval, f"merge_topk_packed {c}, part_bytes {part_bytes}: scores")


def test_sorted_merge_error_surface(cuda_device):
    import torch
    from hbird_mi import _lib
    L = _lib.lib()
    val = torch.zeros((2, 2, 4), dtype=torch.float32, device="cuda")
    idx = torch.zeros((2, 2, 4), dtype=torch.int64, device="cuda")
    oi = torch.full((2, 4), -7, dtype=torch.int64, device="cuda")
    od = torch.full((2, 4), -7.0, dtype=torch.float32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for parts, k, metric, what in ((0, 4, 0, "parts must be in [1, 64]"), (65, 4, 0, "parts must be in [1, 64]"), (2, 0, 0, "k must be in [1, 2048]"),
                                   (2, 2049, 0, "k must be in [1, 2048]"), (2, 4, 2, "metric must be")):
        assert L.hb_bigk_merge_topk(_ptr(val), _ptr(idx), parts, 2, k, metric, _ptr(oi), _ptr(od), s) != 0 and what in _lib.last_error()
        assert L.hb_bigk_merge_topk_packed(_ptr(val), 4096, parts, 2, k, metric, _ptr(oi), _ptr(od), s) != 0 and what in _lib.last_error()
    assert L.hb_bigk_merge_topk_packed(_ptr(val), 2 * 4 * 12 - 8, 2, 2, 4, 0, _ptr(oi), _ptr(od), s) != 0 and "part_bytes" in _lib.last_error()
    assert L.hb_bigk_merge_topk(None, _ptr(idx), 2, 2, 4, 0, _ptr(oi), _ptr(od), s) != 0 and "NULL" in _lib.last_error()
    torch.cuda.synchronize()
    assert (oi == -7).all() and (od == -7.0).all()
