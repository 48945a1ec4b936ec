"""Depth estimation by retrieval on the GPU (include/hbird_hip_depth.h, hbird_mi/ops.py) against the numpy model of tests/depth_refs.py: target rows
and flags on bits, predictions and the no-prediction mask on bits, counts exactly, the non-log sums within the any-order float64 summation
bound, the log-based sums within 4 x the deviation measured on the MI355X (profiles/r30/README.md); the summation order; the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import depth_refs as R
from hbird_mi import _lib, ops

pytestmark = pytest.mark.gpu

# rtol of n and the three non-log sums: summing at most 2^22 non-negative float64 terms in any order stays within (2^22 - 1) u of the exact
# sum, u = 2^-53: 4.7e-10, twice that between two orders
RTOL = 1e-9
# The log-based sums.  The device's float64 log / log10 and numpy's differ in the last place of single logarithms, so these are held to the model
# within 4 x the largest deviation measured on the MI355X over every case below and the worlds of tests/test_depth_eval_gpu.py -- |got - model|
# over the scale of the sum's rounding errors (depth_refs.sums: a term ln p - ln g carries the error of two logarithms however small it is):
# 2.00e-16 (at S = 16, r = 8, 128 x 128; profiles/r30/README.md), so the bound is 8.0e-16
MEASURED_LOG_DEV = 2.00e-16
LOG_TOL = 4 * MEASURED_LOG_DEV


def _live():
    c, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hb_debug_live_allocations(ctypes.byref(c), ctypes.byref(b)))
    return c.value, b.value


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- targets -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("ps,r", R.TARGET_SHAPES)
def test_target_rows_and_flags_equal_the_model_bit_for_bit(cuda_device, ps, r, S):
    y = R.depth_maps(2, S, ps, r, seed=100 * ps + 10 * r + S)
    want_rows, want_flags = R.target_rows(y, ps, r)
    assert want_rows[0, 0, 0, r * r] == 0.0 and want_flags[0, 0, 0] == (r > 1) and want_flags[-1, -1, -1] == 0      # the invalid cell (r = 1: it is its patch), the invalid patch
    assert want_rows[0, 0, 1, r * r:].min() == 1.0                                                          # ... and the wholly valid patch
    rows, flags = ops.patch_depth_targets(torch.from_numpy(y).cuda(), ps, r)
    assert rows.shape == (2, S, S, 2 * r * r) and flags.dtype == torch.int32
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(want_rows))


def test_target_rows_respect_other_bounds_and_rectangles(cuda_device):
    y = R.depth_maps(2, 3, 8, 2, seed=7)[:, :16, :]                      # H = 16, W = 24
    want_rows, want_flags = R.target_rows(y, 8, 2, lo=2.0, hi=6.0)
    rows, flags = ops.patch_depth_targets(torch.from_numpy(np.ascontiguousarray(y)).cuda(), 8, 2, min_depth=2.0, max_depth=6.0)
    assert np.array_equal(flags.cpu().numpy(), want_flags) and np.array_equal(_bits(rows.cpu().numpy()), _bits(want_rows))


# ---- prediction ----------------------------------------------------------------------------------------------------------------------------
def _check_sums(got, pred, has, gt, tag):
    want, scales = R.sums(pred, has, gt)
    dev = 0.0
    for b in range(got.shape[0]):
        for i in (0, 1, 8, 9, 10):
            assert got[b, i] == want[b, i], (tag, b, R.SUMS[i])                      # counts: exact integers in float64
        for i in (2, 3, 4):
            assert abs(got[b, i] - want[b, i]) <= RTOL * abs(want[b, i]), (tag, b, R.SUMS[i], got[b, i], want[b, i])
        for i, scale in zip((5, 6, 7), scales[b]):
            if scale > 0:
                dev = max(dev, abs(got[b, i] - want[b, i]) / scale)
            else:
                assert got[b, i] == want[b, i] == 0.0
    return dev


@pytest.mark.parametrize("S,r,h,w", R.prediction_cases(), ids=lambda v: str(v))
def test_prediction_mask_and_sums_equal_the_model(cuda_device, S, r, h, w):
    B = 3
    agg, gt = R.agg_world(B, S, r, h, w, seed=S * 1000 + r * 100 + h)
    pred, has = R.predict(agg, S, r, h, w)
    if S * r > 1:
        assert has.any() and not has[0].all()                           # image 0's block leaves pixels without a prediction
    before = _live()
    sums, got = ops.depth_upsample_metrics(torch.from_numpy(agg).cuda(), S, r, torch.from_numpy(gt).cuda(), want_map=True)
    assert _live() == before
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint32) == R.NAN_BITS, ~has)
    assert np.array_equal(got.view(np.uint32), pred.view(np.uint32))
    dev = _check_sums(sums.cpu().numpy(), pred, has, gt, (S, r, h, w))
    print(f"depth log-sum deviation S={S} r={r} h={h} w={w}: {dev:.3e}")
    assert dev <= LOG_TOL


# ---- order ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,r,h,w", [(3, 2, 37, 300), (16, 1, 224, 224)])
def test_sums_do_not_depend_on_the_call(cuda_device, S, r, h, w):
    B = 4
    agg, gt = R.agg_world(B, S, r, h, w, seed=5)
    a, g = torch.from_numpy(agg).cuda(), torch.from_numpy(gt).cuda()
    first, pred = ops.depth_upsample_metrics(a, S, r, g, want_map=True)
    again, _ = ops.depth_upsample_metrics(a, S, r, g, want_map=True)
    bare, none = ops.depth_upsample_metrics(a, S, r, g)
    assert none is None
    assert torch.equal(first.view(torch.int64), again.view(torch.int64)) and torch.equal(first.view(torch.int64), bare.view(torch.int64))
    for b in range(B):
        one, p1 = ops.depth_upsample_metrics(a[b:b + 1], S, r, g[b:b + 1], want_map=True)
        assert torch.equal(one.view(torch.int64), first[b:b + 1].view(torch.int64))
        assert torch.equal(p1.view(torch.int32), pred[b:b + 1].view(torch.int32))


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_minus_one_with_a_message_and_allocate_nothing(cuda_device):
    L = _lib.lib()
    y = torch.zeros((1, 16, 16), device="cuda")
    rows, flags = torch.zeros((1, 2, 2, 8), device="cuda"), torch.zeros((1, 2, 2), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    before = _live()
    for args, word in (((None, 1, 16, 16, 8, 2, 1e-3, 10.0, p(rows), p(flags), None), "NULL"),
                       ((p(y), 1, 16, 16, 8, 2, 1e-3, 10.0, None, p(flags), None), "NULL"),
                       ((p(y), 1, 16, 16, 8, 2, 1e-3, 10.0, p(rows), None, None), "NULL"),
                       ((p(y), 1, 16, 16, 8, 3, 1e-3, 10.0, p(rows), p(flags), None), "divide"),
                       ((p(y), 1, 16, 16, 8, 0, 1e-3, 10.0, p(rows), p(flags), None), "target_grid"),
                       ((p(y), 1, 12, 16, 8, 2, 1e-3, 10.0, p(rows), p(flags), None), "multiples"),
                       ((p(y), 1, 16, 12, 8, 2, 1e-3, 10.0, p(rows), p(flags), None), "multiples"),
                       ((p(y), 1, 0, 16, 8, 2, 1e-3, 10.0, p(rows), p(flags), None), "positive"),
                       ((p(y), -1, 16, 16, 8, 2, 1e-3, 10.0, p(rows), p(flags), None), "negative"),
                       ((p(y), 1, 16, 16, 0, 1, 1e-3, 10.0, p(rows), p(flags), None), "patch size"),
                       ((p(y), 1, 128, 128, 128, 1, 1e-3, 10.0, p(rows), p(flags), None), "patch size"),
                       ((p(y), 1, 16, 16, 8, 2, 0.0, 10.0, p(rows), p(flags), None), "bounds"),
                       ((p(y), 1, 16, 16, 8, 2, 5.0, 1.0, p(rows), p(flags), None), "bounds"),
                       ((p(y), 1, 16, 16, 8, 2, 1e-3, float("inf"), p(rows), p(flags), None), "bounds")):
        assert L.hb_patch_depth_targets(*args) == -1 and word in _lib.last_error() and "hb_patch_depth_targets" in _lib.last_error(), (args, _lib.last_error())
        assert _live() == before
    agg, gt = torch.zeros((1, 4, 8), device="cuda"), torch.ones((1, 16, 16), device="cuda")
    sums, pred = torch.zeros((1, _lib.DEPTH_NSUMS), dtype=torch.float64, device="cuda"), torch.zeros((1, 16, 16), device="cuda")
    for args, word in (((None, 1, 2, 2, 16, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "NULL"),
                       ((p(agg), 1, 2, 2, 16, 16, None, 1e-3, 10.0, p(sums), p(pred), None), "NULL"),
                       ((p(agg), 1, 2, 2, 16, 16, p(gt), 1e-3, 10.0, None, p(pred), None), "NULL"),
                       ((p(agg), 1, 0, 2, 16, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "positive"),
                       ((p(agg), 1, 2, -1, 16, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "positive"),
                       ((p(agg), 1, 2, 2, 0, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "positive"),
                       ((p(agg), 1, 2, 2, 16, 0, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "positive"),
                       ((p(agg), -2, 2, 2, 16, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "negative"),
                       ((p(agg), 1, 4096, 2, 16, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None), "exceeds"),
                       ((p(agg), 1, 2, 2, 16, 16, p(gt), -1.0, 10.0, p(sums), p(pred), None), "bounds"),
                       ((p(agg), 1, 2, 2, 16, 16, p(gt), float("nan"), 10.0, p(sums), p(pred), None), "bounds")):
        assert L.hb_depth_upsample_metrics(*args) == -1 and word in _lib.last_error() and "hb_depth_upsample_metrics" in _lib.last_error(), (args, _lib.last_error())
        assert _live() == before
    # empty calls are no errors, and a good call leaves the count as it was
    assert L.hb_patch_depth_targets(None, 0, 16, 16, 8, 2, 1e-3, 10.0, None, None, None) == 0
    assert L.hb_depth_upsample_metrics(None, 0, 2, 2, 16, 16, None, 1e-3, 10.0, None, None, None) == 0
    assert L.hb_patch_depth_targets(p(y), 1, 16, 16, 8, 2, 1e-3, 10.0, p(rows), p(flags), None) == 0
    assert L.hb_depth_upsample_metrics(p(agg), 1, 2, 2, 16, 16, p(gt), 1e-3, 10.0, p(sums), p(pred), None) == 0
    torch.cuda.synchronize()
    assert _live() == before
    assert sums.cpu().numpy()[0, 1] == 256.0 and bool(torch.isnan(pred).all())        # agg of zeros: no pixel has a prediction
    for bad in (dict(y=torch.zeros((1, 16, 16), dtype=torch.float64, device="cuda")), dict(y=torch.zeros((16, 16), device="cuda"))):
        with pytest.raises(ValueError, match="float32"):
            ops.patch_depth_targets(bad["y"], 8)
    with pytest.raises(ValueError, match="target_grid"):
        ops.patch_depth_targets(y, 8, 3)
    with pytest.raises(ValueError, match="agg must be"):
        ops.depth_upsample_metrics(agg, 2, 1, gt)
    with pytest.raises(ValueError, match="gt must be"):
        ops.depth_upsample_metrics(agg, 2, 2, gt[0])
