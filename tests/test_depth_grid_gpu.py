"""Depth grids on the GPU (include/hbird_hip_depth_grid.h, hbird_mi/ops.py): `depth_upsample_metrics_grid` against `depth_upsample_metrics` slab by
slab and bit for bit -- the definition --, and once against the numpy model with tests/test_depth_gpu.py's own tolerances;
`bootstrap_weighted_sums` against the numpy chain of tests/depth_grid_refs.py bit for bit, whatever the passes R is cut into."""
import ctypes

import numpy as np
import pytest
import torch

import depth_grid_refs as G
import depth_refs as R
import test_depth_gpu as T
from hbird_mi import _lib, ops

pytestmark = pytest.mark.gpu

# the prediction cases of tests/test_depth_gpu.py, and the ones that stress the loop over configurations
EXTRA = [(2, 1, 40, 40),         # a band taller than 16 rows: several row chunks
         (4, 2, 16, 300),        # two column chunks, the last one ragged
         (8, 2, 12, 12),         # downsampling, h < S r
         (3, 1, 7, 65),          # one lane past a wave
         (37, 8, 12, 12)]        # a column window of 296 cells: 16 configurations' staged rows exceed the LDS, the stage is re-used
CASES = R.prediction_cases() + EXTRA
NOPRED = 1                       # the slab without any prediction


def _i64(t):
    return t.view(torch.int64)


def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("S,r,h,w", CASES, ids=lambda v: str(v))
def test_every_slab_has_the_bits_of_the_single_call(cuda_device, S, r, h, w):
    B, n_cfg = 3, 16
    agg, gt = G.grid_world(n_cfg, B, S, r, h, w, seed=S * 1000 + r * 100 + h, nopred_slab=NOPRED)
    a, g = torch.from_numpy(agg).cuda(), torch.from_numpy(gt).cuda()
    single = [ops.depth_upsample_metrics(a[c], S, r, g, want_map=True) for c in range(n_cfg)]
    want_sums, want_maps = torch.stack([s for s, _ in single]), torch.stack([p for _, p in single])
    assert bool(torch.isnan(want_maps[NOPRED]).all()) and float(want_sums[NOPRED, :, 0].sum()) == 0.0
    assert float(want_sums[NOPRED, :, 1].sum()) == float(R.valid(gt).sum())                    # every valid pixel of that slab is without a prediction
    if S * r > 1:
        assert bool(torch.isnan(want_maps[0, 0]).any()) and not bool(torch.isnan(want_maps[0]).all())        # image 0's hole block
    before = T._live()
    sums, maps = ops.depth_upsample_metrics_grid(a, S, r, g, want_map=True)
    assert T._live() == before
    assert sums.shape == (n_cfg, B, _lib.DEPTH_NSUMS) and maps.shape == (n_cfg, B, h, w)
    assert torch.equal(_i64(sums), _i64(want_sums)) and torch.equal(_i32(maps), _i32(want_maps))
    again, _ = ops.depth_upsample_metrics_grid(a, S, r, g, want_map=True)
    bare, none = ops.depth_upsample_metrics_grid(a, S, r, g)
    assert none is None and torch.equal(_i64(again), _i64(sums)) and torch.equal(_i64(bare), _i64(sums))
    for n in (1, 3):                                                    # fewer configurations: the same slabs
        s_n, m_n = ops.depth_upsample_metrics_grid(a[:n], S, r, g, want_map=True)
        assert torch.equal(_i64(s_n), _i64(want_sums[:n])) and torch.equal(_i32(m_n), _i32(want_maps[:n]))
    for b in range(B):                                                  # an image's slabs do not depend on the images beside it
        s_b, m_b = ops.depth_upsample_metrics_grid(a[:, b:b + 1].contiguous(), S, r, g[b:b + 1], want_map=True)
        assert torch.equal(_i64(s_b), _i64(want_sums[:, b:b + 1])) and torch.equal(_i32(m_b), _i32(want_maps[:, b:b + 1]))
    assert T._live() == before


def test_seventeen_configurations_go_through_in_two_chunks(cuda_device):
    S, r, h, w = 3, 2, 37, 53
    agg, gt = G.grid_world(17, 2, S, r, h, w, seed=17, nopred_slab=16)
    a, g = torch.from_numpy(agg).cuda(), torch.from_numpy(gt).cuda()
    sums, maps = ops.depth_upsample_metrics_grid(a, S, r, g, want_map=True)
    for c in range(17):
        s1, m1 = ops.depth_upsample_metrics(a[c], S, r, g, want_map=True)
        assert torch.equal(_i64(sums[c]), _i64(s1)) and torch.equal(_i32(maps[c]), _i32(m1)), c
    L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    before = T._live()
    assert L.hb_depth_upsample_metrics_grid(p(a), 17, 2, S, r, h, w, p(g), 1e-3, 10.0, p(sums), None, None) == -1 and "n_cfg" in _lib.last_error()
    assert L.hb_depth_upsample_metrics_grid(p(a), 0, 2, S, r, h, w, p(g), 1e-3, 10.0, p(sums), None, None) == -1 and "n_cfg" in _lib.last_error()
    assert L.hb_depth_upsample_metrics_grid(p(a), 16, 70000, S, r, h, w, p(g), 1e-3, 10.0, p(sums), None, None) == -1 and "grid too large" in _lib.last_error()
    assert T._live() == before
    with pytest.raises(ValueError, match="agg must be"):
        ops.depth_upsample_metrics_grid(a[0], S, r, g)
    with pytest.raises(ValueError, match="gt must be"):
        ops.depth_upsample_metrics_grid(a, S, r, g[:1])


def test_one_case_against_the_numpy_model(cuda_device):
    S, r, h, w, B, n_cfg = 16, 2, 37, 53, 3, 3
    agg, gt = G.grid_world(n_cfg, B, S, r, h, w, seed=23, nopred_slab=NOPRED)
    sums, maps = ops.depth_upsample_metrics_grid(torch.from_numpy(agg).cuda(), S, r, torch.from_numpy(gt).cuda(), want_map=True)
    sums, maps = sums.cpu().numpy(), maps.cpu().numpy()
    for c in range(n_cfg):
        pred, has = R.predict(agg[c], S, r, h, w)
        assert np.array_equal(maps[c].view(np.uint32), pred.view(np.uint32))
        dev = T._check_sums(sums[c], pred, has, gt, ("grid", c))
        print(f"depth grid log-sum deviation, slab {c}: {dev:.3e}")
        assert dev <= T.LOG_TOL


# ---- the resampling reduction --------------------------------------------------------------------------------------------------------------
def _hand_made_W(n_img, R_):
    """Rows with zeros, ones and one large count (2^20 draws of one image), beside a row of zeros."""
    W = np.zeros((R_, n_img), dtype=np.int32)
    for rr in range(R_):
        W[rr, rr % n_img] = 1 << 20
        W[rr, (3 * rr + 1) % n_img] += 1
    if R_ > 1:
        W[R_ - 1] = 0
    return W


@pytest.mark.parametrize("n_img,cols,R_", [(1, 1, 1), (7, 21, 5), (300, 337, 257), (33, 256, 64)])
def test_weighted_sums_equal_the_chain_bit_for_bit_whatever_the_passes(cuda_device, n_img, cols, R_):
    table = G.spread_table(n_img, cols, seed=n_img + cols)
    t = torch.from_numpy(table).cuda()
    drawn = ops.bootstrap_multiplicities(n_img, 20240229, R_)
    assert drawn.dtype == torch.int32 and bool((drawn.sum(1) == n_img).all())
    for W in (drawn, torch.from_numpy(_hand_made_W(n_img, R_)).cuda()):
        want = G.weighted_sums(table, W.cpu().numpy())
        if W is drawn and n_img > 1:                                    # the order shows on this input
            assert not np.array_equal(want, G.weighted_sums(table, W.cpu().numpy(), variant="descending"))
        got = ops.bootstrap_weighted_sums(t, W)
        assert got.shape == (R_, cols) and got.dtype == torch.float64
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))
        for step in (1, 100):
            parts = torch.cat([ops.bootstrap_weighted_sums(t, W[r0:r0 + step]) for r0 in range(0, R_, step)])
            assert torch.equal(_i64(parts), _i64(got)), step


def test_weighted_sums_propagate_non_finite_values_and_refuse_bad_shapes(cuda_device):
    table = np.array([[1.0, np.inf, np.nan], [2.0, 3.0, 4.0]])
    W = np.array([[0, 1], [2, 0], [1, 1]], dtype=np.int32)
    got = ops.bootstrap_weighted_sums(torch.from_numpy(table).cuda(), torch.from_numpy(W).cuda()).cpu().numpy()
    want = G.weighted_sums(table, W)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert np.isnan(got[0, 1]) and got[1, 1] == np.inf and got[0, 0] == 2.0                      # 0 * inf is NaN, as IEEE says
    t = torch.from_numpy(table).cuda()
    assert ops.bootstrap_weighted_sums(t, torch.zeros((0, 2), dtype=torch.int32, device="cuda")).shape == (0, 3)
    for bad_t, bad_w in ((t.float(), torch.from_numpy(W).cuda()), (t, torch.from_numpy(W).cuda().long()), (t, torch.zeros((2, 3), dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError, match="bootstrap_weighted_sums"):
            ops.bootstrap_weighted_sums(bad_t, bad_w)
