"""hb_propagate_labels, hb_mask_upsample_argmax and hb_mask_jf_counts (include/hbird_hip_propagate.h) on the GPU against tests/propagate_refs.py.

Lists and score bits equal the model's: ids and uint32 views, every entry, no exclusions.  The aggregated rows are held to the float64 model
on the engine's own lists within a derived bound.  Maps and counts are bit-defined or integers: equal everywhere.

THE BOUND on an aggregated row, per query, first order in U = 2^-24 (as tests/test_aggregate_paths_gpu.py::tolerance derives K5's):
  * logit_j = s_j / temperature: one fp32 division, and the temperature's own conversion to fp32 is in the model too -- U |logit_j|;
  * e_j = expf(logit_j - mx): the subtraction rounds at U |logit_j - mx| <= U spread, expf adds about 2 U relative and its argument
    reduction another U spread: with the logit's own error, delta_j <= U (|logit_j| + 2 spread + 2).  A perturbation delta_j of the logits
    moves the row by sum_j w_j (delta_j - mean delta) label_j: at most 2 max|delta| max|label| -- 2 U max|logit| + 4 U spread + 4 U at worst,
    of which the common part cancels; the bound keeps 2 max|logit| + 2 spread + 4;
  * den: k - 1 additions, and one division per weight: (k - 1) U + U relative on every weight, a relative error of the row: k U;
  * the row: k fmaf steps: k U sum_j w_j |label_j| <= k U max|label|;
  * the final comparison's own rounding of the fp32 result: 2 U.
  |got - ref| <= max|label| * U * (2 max|logit| + 2 spread + 2 k + 6).
A dropped neighbour and a label off by one pixel share must move the median query by more than 20 x that bound, or the case sees nothing."""
import functools

import numpy as np
import pytest
import torch

import propagate_refs as R
from hbird_mi import _lib, ops

pytestmark = pytest.mark.gpu

# (grid, d, k, pool slots, slots, radii, nan): slots out of order, one listed twice (exact ties), radii mixed per context position
CASES = {
    "7x11-d64-k5-ctx3": ((7, 11), 64, 5, 3, [2, 0, 2], [1, 0, 1], None),
    "13x9-d388-k32-ctx8": ((13, 9), 388, 32, 6, [3, 1, 0, 2, 1, 4, 5, 0], [12, -1, 0, 1, 12, 1, 0, -1], None),
    "1x40-d4-k1-ctx1": ((1, 40), 4, 1, 1, [0], [-1], None),
    "7x11-d4-k32-r0": ((7, 11), 4, 32, 2, [1], [0], None),                       # k larger than the candidate count (1)
    "13x9-d64-k5-nan-ctx": ((13, 9), 64, 5, 2, [1, 0], [12, 12], "ctx"),
    "1x40-d388-k5-nan-q": ((1, 40), 388, 5, 3, [2, 1], [1, -1], "q"),
    "7x11-d388-k1-ctx8": ((7, 11), 388, 1, 8, [7, 6, 5, 4, 3, 2, 1, 0], [1] * 8, None),
    "13x9-d4-k5-free": ((13, 9), 4, 5, 2, [0, 1], [-1, -1], None),
    "7x11-d64-k32-ctx2-dup": ((7, 11), 64, 32, 2, [1, 1], [1, 12], None),
    "7x11-d1024-k32-r1": ((7, 11), 1024, 32, 1, [0], [1], None),                 # the largest staging: query rows without padding
}
C, TEMP = 5, 0.1


@functools.lru_cache(maxsize=None)
def case(name):
    grid, d, k, pool, slots, radii, nan = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    N = grid[0] * grid[1]
    q, feat = R.unit_rows(rng, N, d), R.unit_rows(rng, pool, N, d)
    lab = rng.integers(0, 65, size=(pool, N, C)).astype(np.float32) / np.float32(64)          # pixel shares of an 8 x 8 patch
    if nan == "ctx":
        feat[slots[0], N // 2] = np.nan
    if nan == "q":
        q[N // 3] = np.nan
    idx, score = R.lists(q, feat, slots, radii, grid, k)
    for a in (q, feat, lab, idx, score):
        a.setflags(write=False)
    return dict(grid=grid, d=d, k=k, slots=slots, radii=radii, nan=nan, N=N, q=q, feat=feat, lab=lab, idx=idx, score=score)


def run(c, want=True, k=None):
    return ops.propagate_labels(torch.tensor(c["q"]).cuda(), torch.tensor(c["feat"]).cuda(), torch.tensor(c["lab"]).cuda(), c["slots"],
                                c["radii"], c["grid"], k=k or c["k"], temperature=TEMP, want_neighbours=want)


def u32(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_and_rows(cuda_device, name):
    c = case(name)
    k, N = c["k"], c["N"]
    out, idx, score = run(c)
    idx_h = idx.cpu().numpy()
    assert np.array_equal(idx_h, c["idx"]), f"{(idx_h != c['idx']).sum()} ids differ from the model's"
    assert np.array_equal(u32(score), u32(c["score"])), "score bits differ from the model's"
    if c["nan"] == "q":
        i = N // 3
        assert (idx_h[i] == -1).all() and np.array_equal(u32(out[i]), np.zeros(C, dtype=np.uint32)), "a NaN query lists nothing and gives zeros"
    if c["nan"] == "ctx":
        assert not (idx_h == N // 2).any(), "a NaN context row is never a neighbour"      # (context position 0: id = cell)
    if name == "7x11-d4-k32-r0":
        assert (idx_h[:, 0] == np.arange(N)).all() and (idx_h[:, 1:] == -1).all() and np.isneginf(score.cpu().numpy()[:, 1:]).all()
    # the aggregated rows: float64 model on the engine's lists
    got = out.cpu().numpy().astype(np.float64)
    ref = R.aggregate(idx_h, score.cpu().numpy(), c["lab"], c["slots"], N, TEMP)
    tol = R.aggregate_bound(idx_h, score.cpu().numpy(), c["lab"], TEMP)
    err = np.abs(got - ref).max(axis=1)
    print(f"{name}: worst |got - ref| / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all(), f"{(err > tol).sum()} rows beyond the bound, worst {np.max(err / np.maximum(tol, 1e-300)):.2f} x"
    if k == 1:
        rows = np.stack([c["lab"][c["slots"][j // N], j % N] if j >= 0 else np.zeros(C, np.float32) for j in idx_h[:, 0]])
        assert np.array_equal(u32(out), u32(rows)), "with k = 1 the row is the neighbour's label row"
    elif name != "7x11-d4-k32-r0":
        live = (idx_h >= 0).sum(axis=1) >= 2
        drop = idx_h.copy()
        last = (idx_h >= 0).sum(axis=1) - 1                              # the least-weighted neighbour is the list's last
        drop[np.arange(N), np.maximum(last, 0)] = -1
        r_drop = R.aggregate(drop, score.cpu().numpy(), c["lab"], c["slots"], N, TEMP)
        shifted = c["lab"].astype(np.float64).copy()
        shifted[..., -1] += 1.0 / 64
        r_shift = R.aggregate(idx_h, score.cpu().numpy(), shifted, c["slots"], N, TEMP)
        s_drop = float(np.median((np.abs(r_drop - ref).max(axis=1) / np.maximum(tol, 1e-300))[live]))
        s_shift = float(np.median((np.abs(r_shift - ref).max(axis=1) / np.maximum(tol, 1e-300))[live]))
        assert s_drop > 20 and s_shift > 20, f"the case cannot see a dropped neighbour ({s_drop:.1f} x) or a label off by one ({s_shift:.1f} x)"


@pytest.mark.parametrize("name", ["7x11-d64-k5-ctx3", "13x9-d388-k32-ctx8"])
def test_two_calls_same_bits_with_and_without_lists(cuda_device, name):
    c = case(name)
    a, ia, sa = run(c)
    b, ib, sb = run(c)
    plain = run(c, want=False)
    assert np.array_equal(u32(a), u32(b)) and torch.equal(ia, ib) and np.array_equal(u32(sa), u32(sb))
    assert np.array_equal(u32(a), u32(plain)), "the rows do not depend on the optional outputs"


def test_refusals_before_any_launch(cuda_device):
    c = case("7x11-d64-k5-ctx3")
    q, feat, lab = (torch.tensor(c[n]).cuda() for n in ("q", "feat", "lab"))
    with pytest.raises(_lib.HbirdHipError, match="slot"):
        ops.propagate_labels(q, feat, lab, [0, 3], [1, 1], c["grid"])
    with pytest.raises(_lib.HbirdHipError, match="limit"):
        ops.propagate_labels(q, feat, lab, [0], [1], c["grid"], k=33)
    with pytest.raises(_lib.HbirdHipError, match="temperature"):
        ops.propagate_labels(q, feat, lab, [0], [1], c["grid"], temperature=0.0)
    with pytest.raises(ValueError):
        ops.propagate_labels(q[:, :3], feat, lab, [0], [1], c["grid"])
    with pytest.raises(ValueError):
        ops.mask_jf_counts(torch.zeros((1, 4, 4), dtype=torch.int32).cuda(), torch.zeros((1, 4, 4), dtype=torch.int64).cuda(), 1, 1)
    with pytest.raises(_lib.HbirdHipError, match="bound_px"):
        ops.mask_jf_counts(torch.zeros((1, 4, 4), dtype=torch.int64).cuda(), torch.zeros((1, 4, 4), dtype=torch.int64).cuda(), 1, 33)


# ---- the label map -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def label_rows(grid, c, B=2):
    rng = np.random.default_rng(grid[0] * 100 + grid[1] + c)
    x = rng.random((B, grid[0] * grid[1], c)).astype(np.float32)
    x[0, :, 0] *= np.float32(0.3)
    if c >= 3:
        x[:, :, 1] = 0.0                                     # a channel that is all zero
        x[:, :, 2] = np.float32(0.37)                        # a constant positive channel
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("grid,hw,c", [((6, 8), (48, 64), 3), ((7, 11), (53, 90), 11), ((1, 1), (5, 3), 1), ((7, 11), (53, 90), 64), ((6, 8), (48, 64), 1),
                                       ((1, 1), (5, 3), 3)])
def test_label_map_equals_the_model(cuda_device, grid, hw, c, norm):
    x = label_rows(grid, c)
    got = ops.mask_upsample_argmax(torch.tensor(x).cuda(), grid, hw[0], hw[1], channel_norm=norm).cpu().numpy()
    want = R.label_map(x, grid, hw[0], hw[1], norm=norm)
    assert got.shape == want.shape and np.array_equal(got, want), f"{(got != want).sum()} of {want.size} pixels differ"
    if c >= 3 and grid != (1, 1):
        other = R.label_map(x, grid, hw[0], hw[1], norm=not norm)
        assert not np.array_equal(want, other), "the case cannot tell the two channel_norm settings apart"


# ---- J and F counts ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_world(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    n = 4
    pred, gt = R.blobs(rng, 3, h, w, n), R.blobs(rng, 3, h, w, n)
    gt[:, :, :] = np.where(rng.random(gt.shape) < 0.7, pred, gt)             # correlated maps: matches and misses
    pred[pred == 3] = 0                                                      # object 3 absent from pred
    gt[gt == 4] = 0                                                          # object 4 absent from gt
    pred[0][(pred[0] == 0)] = 2                                              # object 2 touches every image edge in image 0 ...
    pred[0, 0, :] = 2; pred[0, -1, :] = 2; pred[0, :, 0] = 2; pred[0, :, -1] = 2
    gt[0, 0, :] = 2; gt[0, -1, :] = 2; gt[0, :, 0] = 2; gt[0, :, -1] = 2     # ... in both maps
    pred.setflags(write=False); gt.setflags(write=False)
    return pred, gt, n


@pytest.mark.parametrize("bound", [0, 1, 3, 32])
@pytest.mark.parametrize("hw", [(48, 64), (53, 90)])
def test_jf_counts_equal_the_model(cuda_device, hw, bound):
    pred, gt, n = blob_world(*hw)
    assert (pred == 3).sum() == 0 and (gt == 3).sum() > 0 and (gt == 4).sum() == 0 and (pred == 4).sum() > 0
    got = ops.mask_jf_counts(torch.tensor(pred).cuda(), torch.tensor(gt).cuda(), n, bound)
    again = ops.mask_jf_counts(torch.tensor(pred).cuda(), torch.tensor(gt).cuda(), n, bound)
    want = R.jf_counts(pred, gt, n, bound)
    assert got.shape == (3, n, 6) and np.array_equal(got.cpu().numpy(), want), f"counts differ:\n{got.cpu().numpy() - want}"
    assert torch.equal(got, again)
    if bound == 0:
        assert (want[..., 4] < want[..., 2]).any() and (want[..., 5] < want[..., 3]).any(), "the world cannot see the tolerance"
