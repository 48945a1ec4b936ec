"""K5 over a grid of (k, beta) configurations from one neighbour list per query (aggregate_grid_kernel, csrc/hbird_grid.hip; neighbour
resolution and count decode shared with aggregate_kernel in csrc/hbird_k5_dev.h) through
HipFlatIndex.aggregate_grid / search_aggregate_grid.

Configuration (k, beta) is `aggregate` applied to the first k POSITIONS of the list, whatever they hold, and must have its bits.  Inputs,
the float64 reference and its bound are those of tests/test_aggregate_paths_gpu.py: `_run_case` builds the index of a case in its table
form and calls `aggregate`; here it runs with a HipFlatIndex whose `aggregate` also remembers the call, so the very same index and device
tensors reach `aggregate_grid`.

 1. bits: every AggCase, ks = the distinct values of {1, max(1, k // 3), k - 1, k} that are >= 1 on a list of stride k, betas = (the
    case's, 0.05); a list longer than the largest k; 16 configurations; a non-finite label row beyond a configuration's k.
 2. definition, independent of the old kernel: the same outputs within tolerance(...) of reference(...) on the prefix.
 3. the fused entry = search at the largest k + aggregate_grid, and returns that search's neighbours.
 4. the prefix property the feature rests on (passes without the feature): search(q, k_max)[:, :k] is search(q, k), bit for bit, on a
    bank whose ties cross every cut.
 5. k beyond 256 and grids of more than 16 configurations.
 6. the error surface: nothing is launched half-way.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import test_aggregate_paths_gpu as A
from test_aggregate_paths_gpu import AggCase, _labels, _queries, _rows, reference, tolerance

pytestmark = pytest.mark.gpu

BETA2 = 0.05


def _ks_of(k):
    return sorted({v for v in (1, max(1, k // 3), k - 1, k) if v >= 1})


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _recorded_case(c, seed):
    """`A._run_case` with a HipFlatIndex that keeps the arguments of its `aggregate` call: (index, q, idx, dist, beta, id_base) on the device
    and everything `_run_case` returns on the host."""
    from hbird_mi.nn import search_hip
    calls = []

    class Recording(search_hip.HipFlatIndex):
        def aggregate(self, q, idx, dist, beta=0.02, id_base=0):
            calls.append((self, q, idx, dist, beta, id_base))
            return super().aggregate(q, idx, dist, beta=beta, id_base=id_base)

    plain = search_hip.HipFlatIndex
    search_hip.HipFlatIndex = Recording
    try:
        host = A._run_case(c, seed)
    finally:
        search_hip.HipFlatIndex = plain
    return calls[-1], host


@functools.lru_cache(maxsize=None)
def _grid_of_case(i):
    """Case i of A.CASES: the grid's output (once, shared by the bit and the definition test) with what both compare it to."""
    from hbird_mi.nn.search_hip import grid_plan
    c = A.CASES[i]
    (ix, q, idx, dist, beta, id_base), host = _recorded_case(c, 3000 + i)
    plan = grid_plan(_ks_of(c.k), (c.beta, BETA2))
    assert idx.shape[1] == c.k and plan.ks[-1] == c.k
    got = ix.aggregate_grid(q, idx, dist, plan.ks, plan.betas, id_base=id_base)
    old = [ix.aggregate(q, idx[:, :k].contiguous(), dist[:, :k].contiguous(), beta=b, id_base=id_base) for k, b in plan.configs]
    return c, plan, got, old, host


def test_the_ks_cross_the_lane_and_group_boundaries():
    """The cut positions of the case list cross 64 / 65 (the lane-strided softmax) and, in the grouped form, G * 8 (one unrolled step)."""
    cuts = {(c.C, k) for c in A.CASES for k in _ks_of(c.k)}
    assert {63, 64, 65} <= {k for _, k in cuts} and {255, 256} <= {k for _, k in cuts}
    grouped = [(64 // C * 8, k) for C, k in cuts if C <= 32]
    crossed = {C for C in {C for C, _ in cuts if C <= 32}
               if any(k < 64 // C * 8 for CC, k in cuts if CC == C) and any(k > 64 // C * 8 for CC, k in cuts if CC == C)}
    assert grouped and {3, 21, 32} <= crossed, crossed       # (G = 21, 3 and 2 neighbour groups)
    assert all(len(_ks_of(c.k)) * 2 <= 16 for c in A.CASES)


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=[A.case_id(c) for c in A.CASES])
def test_grid_bits_equal_aggregate_on_the_prefix(cuda_device, i):
    import torch
    c, plan, got, old, _ = _grid_of_case(i)
    assert tuple(got.shape) == (len(plan.configs), A.NQ, c.C)
    for n, (k, b) in enumerate(plan.configs):
        assert torch.equal(_bits(got[n]), _bits(old[n])), \
            f"k={k} beta={b}: {int((_bits(got[n]) != _bits(old[n])).sum())} of {old[n].numel()} values differ, max |diff| {float((got[n] - old[n]).abs().max()):.3e}"
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=[A.case_id(c) for c in A.CASES])
def test_grid_against_float64_on_the_prefix(cuda_device, i):
    c, plan, got, _, host = _grid_of_case(i)
    _, _, _, _, h, idx, dist, norms, base = host
    out = got.cpu().numpy()
    for n, (k, b) in enumerate(plan.configs):
        ref, w, logits = reference(h["q"], idx[:, :k], dist[:, :k], norms, base, h["labels"], base, b, c.metric)
        tol = tolerance(h["q"], idx[:, :k], dist[:, :k], norms, base, logits, k, b, c.metric, float(h["labels"].max()))
        err = np.abs(out[n].astype(np.float64) - ref).max(axis=1)
        ratio = err / tol
        j = int(ratio.argmax())
        print(f"K5 grid {A.case_id(c)} k={k} beta={b}: max err {err.max():.3e}, max err / bound {ratio.max():.3f}")
        assert ratio.max() <= 1.0, f"k={k} beta={b}, query {j} (pattern {j % A.NQ_PATTERNS}): |grid - float64| = {err[j]:.3e} > bound {tol[j]:.3e}"
        empty = ~(w > 0).any(axis=1)
        assert not out[n][empty].any(), "a prefix of only -1 must give exactly 0"


# one case per body of the kernel, on lists longer than the largest k and with all 16 accumulator sets in use
BODIES = [AggCase("grouped", "own_f32", 21, 200, "ip", 0.07, 30, 0), AggCase("wide", "own_u16_196", 151, 90, "l2", 0.02, 1, 4096),
          AggCase("generic", "ext_f32", 65, 256, "ip", 0.07, 1, 0), AggCase("generic", "ext_u16_mis", 152, 100, "l2", 0.07, 30, 0)]


@pytest.mark.parametrize("c", BODIES, ids=A.case_id)
@pytest.mark.parametrize("shape", ["stride", "sixteen"])
def test_grid_on_a_longer_list_and_with_16_configurations(cuda_device, c, shape):
    """stride: k_list > ks[-1] (the row stride is not the largest k); sixteen: 4 x 4 configurations, ks across 64 / 65."""
    import torch
    from hbird_mi.nn.search_hip import grid_plan
    (ix, q, idx, dist, _, id_base), _ = _recorded_case(c, 4000 + c.C)
    ks, betas = ((7, c.k // 3, c.k - 11), (c.beta, BETA2)) if shape == "stride" else ((1, 9, 64, 65), (0.01, 0.02, 0.05, 0.1))
    plan = grid_plan(ks, betas)
    assert plan.ks[-1] < idx.shape[1] and len(plan.launches) == 1 and (shape == "stride" or len(plan.configs) == 16)
    got = ix.aggregate_grid(q, idx, dist, ks, betas, id_base=id_base)
    for n, (k, b) in enumerate(plan.configs):
        old = ix.aggregate(q, idx[:, :k].contiguous(), dist[:, :k].contiguous(), beta=b, id_base=id_base)
        assert torch.equal(_bits(got[n]), _bits(old)), (k, b)
    assert float(got.abs().max()) > 0


@pytest.mark.parametrize("C", [21, 151])
def test_a_position_beyond_k_does_not_touch_the_accumulator(cuda_device, C):
    """An fp32 table may hold non-finite values: a row with inf / nan that a list names only beyond position k must leave configuration k
    finite (a zero weight would turn it into nan) -- and configuration k_list, which includes it, is aggregate's non-finite answer."""
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(C)
    n, k_list, bad = 300, 40, 17
    labels, _ = _labels(n, C, 196, rng)
    labels[bad, 0::2] = np.inf
    labels[bad, 1::2] = np.nan
    ix = HipFlatIndex(A.D, 0, 0)
    ix.add(torch.from_numpy(_rows(n, rng)).cuda()); ix.add_labels(torch.from_numpy(labels).cuda()); ix.set_num_classes(C)
    q = torch.from_numpy(_queries(1.0, rng)).cuda()
    idx = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(n), [bad]), (A.NQ, k_list))).cuda()
    idx[:, 25] = bad
    dist = torch.rand((A.NQ, k_list), device="cuda")
    got = ix.aggregate_grid(q, idx, dist, (8, 25, 26, 40), (0.02, 0.1))
    assert bool(torch.isfinite(got[:4]).all()) and float(got[:4].abs().max()) > 0        # k = 8 and k = 25: the row is not among them
    assert not bool(torch.isfinite(got[4:]).any())
    for n_, (k, b) in enumerate([(k, b) for k in (8, 25, 26, 40) for b in (0.02, 0.1)]):
        old = ix.aggregate(q, idx[:, :k].contiguous(), dist[:, :k].contiguous(), beta=b)
        if k <= 25:
            assert torch.equal(_bits(got[n_]), _bits(old)), (k, b)
        else:                   # (inf and nan in the same places; a nan's payload is not part of the contract)
            assert torch.equal(torch.isnan(got[n_]), torch.isnan(old)) and torch.equal(torch.isinf(got[n_]), torch.isinf(old)), (k, b)


# ---------------------------------------------------------------- the fused entry

def _bank_index(n, d, C, metric, rng, P=196, counts=True):
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    b = rng.standard_normal((n, d))
    b *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(b, axis=1, keepdims=True)
    labels, _ = _labels(n, C, P, rng)
    ix = HipFlatIndex(d, 0 if metric == "ip" else 1, 0)
    if counts:
        ix.set_label_denominator(P)
    ix.add(torch.from_numpy(b.astype(np.float32)).cuda()); ix.add_labels(torch.from_numpy(labels).cuda()); ix.set_num_classes(C)
    return ix


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("C", [21, 151])
@pytest.mark.parametrize("n,ks", [(3000, (7, 30, 33, 90)), (20, (10, 20, 25, 30))], ids=["3000rows", "20rows"])
def test_fused_entry_is_one_search_then_the_grid(cuda_device, C, metric, n, ks):
    """37 queries (not a multiple of 4), ks across the LDS-list / pool boundary of the search at 32; the 20-row bank leaves the tail of
    every list missing (id -1)."""
    import torch
    rng = np.random.default_rng(C * 100 + n)
    d, nq, betas = 32, 37, (0.02, 0.1)
    ix = _bank_index(n, d, C, metric, rng)
    q = torch.from_numpy((3.0 * rng.standard_normal((nq, d))).astype(np.float32)).cuda()
    lh, idx, dist = ix.search_aggregate_grid(q, ks, betas, want_neighbours=True)
    sidx, sdist = ix.search(q, ks[-1])
    assert torch.equal(idx, sidx) and torch.equal(_bits(dist), _bits(sdist))
    assert int((idx >= 0).sum()) == nq * min(ks[-1], n) and bool((idx[:, min(ks[-1], n):] == -1).all())
    again = ix.aggregate_grid(q, sidx, sdist, ks, betas)
    assert tuple(lh.shape) == (len(ks) * len(betas), nq, C) and torch.equal(_bits(lh), _bits(again))
    assert torch.equal(_bits(ix.search_aggregate_grid(q, ks, betas)), _bits(lh))
    # every configuration is the separate fused call the grid replaces
    for i, (k, b) in enumerate([(k, b) for k in ks for b in betas]):
        assert torch.equal(_bits(lh[i]), _bits(ix.search_aggregate(q, k, beta=b))), (k, b)
    # host arrays in, host arrays out
    hl, hi, hd = ix.search_aggregate_grid(q.cpu().numpy(), ks, betas, want_neighbours=True)
    assert isinstance(hl, np.ndarray) and np.array_equal(hl.view(np.uint32), lh.cpu().numpy().view(np.uint32))
    assert np.array_equal(hi, idx.cpu().numpy()) and np.array_equal(hd.view(np.uint32), dist.cpu().numpy().view(np.uint32))
    assert float(lh.abs().max()) > 0.1


# ---------------------------------------------------------------- the prefix property

@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("k,k_max", [(30, 90), (32, 33), (90, 256)])
def test_the_best_k_are_the_first_k_of_the_best_k_max(cuda_device, k, k_max, metric):
    """Small-integer rows, every row seven times in the bank (7 divides no cut): scores tie exactly, within a row's copies and between rows,
    across every cut of every query."""
    import torch
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(k_max)
    d, nq = 32, 37
    base = rng.integers(-2, 3, (430, d)).astype(np.float32)
    bank = np.tile(base, (7, 1))[rng.permutation(3010)]
    ix = HipFlatIndex(d, 0 if metric == "ip" else 1, 0)
    ix.add(torch.from_numpy(bank).cuda())
    q = torch.from_numpy(rng.integers(-2, 3, (nq, d)).astype(np.float32)).cuda()
    bi, bd = ix.search(q, k_max)
    si, sd = ix.search(q, k)
    assert k % 7 and bool((bd[:, k - 1] == bd[:, k]).all()), "the ties must cross the cut"
    assert torch.equal(bi[:, :k], si) and torch.equal(_bits(bd[:, :k]), _bits(sd))
    assert bool((bi >= 0).all()) and bool((bi[:, 1:] != bi[:, :-1]).all())


# ---------------------------------------------------------------- beyond 256, more than 16 configurations

def test_a_k_beyond_256_costs_no_second_search(cuda_device):
    import torch
    rng = np.random.default_rng(300)
    ix = _bank_index(2000, A.D, 21, "ip", rng)
    q = torch.from_numpy(_queries(3.0, rng)).cuda()
    lh, idx, dist = ix.search_aggregate_grid(q, (30, 300), (0.02, 0.1), want_neighbours=True)
    assert tuple(lh.shape) == (4, A.NQ, 21) and tuple(idx.shape) == (A.NQ, 300)
    for i, (k, b) in enumerate([(30, 0.02), (30, 0.1), (300, 0.02), (300, 0.1)]):
        want = ix.search_aggregate(q, k, beta=b) if k <= 256 else ix.search_aggregate_bigk(q, k, beta=b)
        assert torch.equal(_bits(lh[i]), _bits(want)), (k, b)
    # the same through aggregate_grid on the given lists, with the small ks cut into more than one launch
    ks, betas = (5, 30, 64, 200, 256, 300), (0.02, 0.05, 0.1)
    got = ix.aggregate_grid(q, idx, dist, ks, betas)
    for i, (k, b) in enumerate([(k, b) for k in ks for b in betas]):
        want = ix.search_aggregate(q, k, beta=b) if k <= 256 else ix.search_aggregate_bigk(q, k, beta=b)
        assert torch.equal(_bits(got[i]), _bits(want)), (k, b)


@pytest.mark.parametrize("C", [21, 151])
def test_a_5_by_5_grid_is_two_launches_with_the_per_configuration_results(cuda_device, C):
    import torch
    from hbird_mi.nn.search_hip import grid_plan
    rng = np.random.default_rng(55 + C)
    ix = _bank_index(2000, A.D, C, "l2", rng)
    q = torch.from_numpy(_queries(3.0, rng)).cuda()
    ks, betas = (90, 3, 64, 17, 65), (0.1, 0.01, 0.02, 0.05, 1.0)          # any order: the grid is sorted
    plan = grid_plan(ks, betas)
    assert len(plan.launches) == 2 and len(plan.configs) == 25
    lh = ix.search_aggregate_grid(q, ks, betas)
    assert tuple(lh.shape) == (25, A.NQ, C)
    for i, (k, b) in enumerate(plan.configs):
        assert torch.equal(_bits(lh[i]), _bits(ix.search_aggregate(q, k, beta=b))), (k, b)


# ---------------------------------------------------------------- errors

def test_grid_error_surface(cuda_device):
    """Bad grids are refused with the C side's message before anything is launched: the output of a failing call is untouched and the
    next valid call returns the right bits."""
    import ctypes
    import torch
    from hbird_mi import _lib
    from hbird_mi.nn.search_hip import HipFlatIndex
    rng = np.random.default_rng(7)
    n, C, k_list = 300, 21, 40
    ix = _bank_index(n, A.D, C, "ip", rng, counts=False)
    q = torch.from_numpy(_queries(1.0, rng)).cuda()
    idx, dist = ix.search(q, k_list)
    good = ix.aggregate_grid(q, idx, dist, (10, 40), (0.02,))
    want = [ix.aggregate(q, idx[:, :k].contiguous(), dist[:, :k].contiguous(), beta=0.02) for k in (10, 40)]
    assert torch.equal(_bits(good[0]), _bits(want[0])) and torch.equal(_bits(good[1]), _bits(want[1]))

    def c_entry(ks, betas, lists=(idx, dist), index=ix):
        """hb_index_aggregate_grid itself (the Python layer orders and checks a grid before it gets there)."""
        out = torch.full((len(ks) * len(betas), A.NQ, C), 7.0, device="cuda")
        index._grid_call(q, lists[0], lists[1], ks, betas, 0, out)
        return out

    def fused(ks, betas, index=ix):
        out = torch.full((max(1, len(ks) * len(betas)), A.NQ, C), 7.0, device="cuda")
        ka, ba = (ctypes.c_int * len(ks))(*ks), (ctypes.c_float * len(betas))(*betas)
        rc = _lib.lib().hb_index_search_aggregate_grid(index._h, ctypes.c_void_p(q.data_ptr()), A.NQ, 0, ka, len(ks), ba, len(betas),
                                                       ctypes.c_void_p(out.data_ptr()), None, None, 1)
        torch.cuda.synchronize()
        return rc, _lib.last_error(), out

    bare = HipFlatIndex(A.D, 0, 0)
    bare.add(torch.from_numpy(_rows(n, rng)).cuda()); bare.set_num_classes(C)
    nan, inf = float("nan"), float("inf")
    bad = [((30, 10), (0.02,), "strictly ascending"), ((10, 10), (0.02,), "strictly ascending"), ((0, 10), (0.02,), "must be positive"),
           ((10, 41), (0.02,), "exceeds k_list"), (tuple(range(1, 18)), (0.02,), "at most 16"), ((1, 2, 3), (0.01, 0.02, 0.03, 0.04, 0.05, 0.06), "at most 16")]
    bad += [((10,), (b,), "finite and positive") for b in (0.0, -1.0, nan, inf)] + [((10,), (0.02, nan), "finite and positive")]
    for ks, betas, msg in bad:
        with pytest.raises(ValueError, match=msg):
            c_entry(ks, betas)
        if "k_list" not in msg:
            rc, err, out = fused(ks, betas)
            assert rc != 0 and msg in err and bool((out == 7.0).all()), (ks, betas, err)
        again = c_entry((10, 40), (0.02,))
        assert torch.equal(_bits(again), _bits(good)), (ks, betas)
    with pytest.raises(ValueError, match="largest k must be <= 256"):
        c_entry((10, 257), (0.02,), lists=ix.search(q, 257))
    rc, err, out = fused((10, 257), (0.02,))
    assert rc != 0 and "largest k must be <= 256" in err and bool((out == 7.0).all())
    with pytest.raises(ValueError, match="label rows missing"):
        c_entry((10, 40), (0.02,), index=bare)
    rc, err, out = fused((10, 40), (0.02,), index=bare)
    assert rc != 0 and "label rows missing" in err and bool((out == 7.0).all())
    # the Python layer: the same refusals before the library is reached (it sorts a grid, so order and repeats are not errors there)
    for ks, betas in [((10, 41), (0.02,)), ((10,), (0.0,)), ((10,), (nan,)), ((10,), (inf,)), ((10,), (-1.0,)), ((0,), (0.02,)), ((), (0.02,))]:
        with pytest.raises(ValueError):
            ix.aggregate_grid(q, idx, dist, ks, betas)
    with pytest.raises(ValueError, match="label rows missing"):
        bare.search_aggregate_grid(q, (10, 40), (0.02,))
    with pytest.raises(ValueError, match="label rows missing"):
        bare.aggregate_grid(q, idx, dist, (10, 40), (0.02,))
    assert torch.equal(_bits(ix.aggregate_grid(q, idx, dist, (40, 10, 10), (0.02, 0.02))), _bits(good))
    assert torch.equal(_bits(ix.search_aggregate_grid(q, (10, 40), (0.02,))), _bits(good))
