"""The linear probe on the GPU (include/hbird_hip_linprobe.h, hbird_mi/linear_probe.py) against the numpy model of tests/linprobe_refs.py: logits on
bits, residuals and loss against float64 from the device's own logits, the gradient inside an fma chain's textbook bound of the float64 gradient
of the device's own residuals and the same bits twice, the fit against the float64 optimum.  The worlds are the smallest at which a path can go
wrong: a padded width (72 -> 80), C on both sides of 32 and at 151 (count rows of stride 152), rows no multiple of 32 or 256, three segments with
a last one of one row.

Past the first bank-size seams (the case lists below are held to the dispatch arithmetic by tests/test_bank_task_seams_cpu.py, without a GPU):
R.TILE_WORLDS run every class-tile instantiation of the forward kernel at both ends of its tile, CHUNK_CASES run the workspace chunk loop through
hb_linprobe_set_workspace and hold every output to the default workspace's bits, R.BIG_WORLD has segments of 512 rows, a ragged last one and rows
at j = 1 and 2 of the loss tree."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import linprobe_refs as R
from hbird_mi import _lib
from hbird_mi import linear_probe as LP
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

pytestmark = pytest.mark.gpu

ALL_WORLDS = [(w, 16) for w in R.WORLDS] + [(R.WIDE_WORLD, 196), (R.SEGMENT_WORLD, 16)]
TILE_CASES = [(w, 16) for w in R.TILE_WORLDS]
BIG_CASE = (R.BIG_WORLD, 16)
CT8_WORLD = R.TILE_WORLDS[12]                    # C = 256: eight class tiles, the largest residual stride
# (world, P, segments the workspace holds): three chunks of one segment; 2 + 1; two chunks at ct = 8; 85 chunks of three segments and one of two
CHUNK_CASES = [(R.SEGMENT_WORLD, 16, 1), (R.SEGMENT_WORLD, 16, 2), (CT8_WORLD, 16, 1), (R.BIG_WORLD, 16, 3)]
L2 = R.FIT_L2


def _world(spec, P):
    return R.big_world() if spec == R.BIG_WORLD else R.world(spec, P)


def seg_bytes(spec):
    """Bytes of one segment in the workspace (hb_linprobe_loss_grad): seg_rows * (cp + xs) * 4, cp = 32 ceil(C / 32), xs = 32 ceil((D + 1) / 32)."""
    C, D, rows = spec[:3]
    return R.partition(rows)[0] * (32 * -(-C // 32) + 32 * -(-(D + 1) // 32)) * 4


@contextlib.contextmanager
def _workspace(nbytes):
    _lib.check(_lib.lib().hb_linprobe_set_workspace(int(nbytes)))
    try:
        yield
    finally:
        _lib.check(_lib.lib().hb_linprobe_set_workspace(0))


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _bank(x, y=None, P=0):
    ix = HipFlatIndex(x.shape[1], 0, 0)
    ix.add(torch.from_numpy(np.ascontiguousarray(x)).cuda(), normalize=False)
    if y is not None:
        if P:
            ix.set_label_denominator(P)
        ix.add_labels(torch.from_numpy(np.ascontiguousarray(y)).cuda())
        ix.set_num_classes(y.shape[1])
    return ix


def _live():
    c, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hb_debug_live_allocations(ctypes.byref(c), ctypes.byref(b)))
    return c.value, b.value


def _params(w, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((w["C"], w["D"] + 1)) * scale).astype(np.float32)


def _with_a_hole(w):
    x = w["x"].copy()
    if not np.isfinite(x).all():                               # (R.big_world brings its own, past row 65,536)
        return x
    x[min(37, x.shape[0] - 1), 5] = np.nan
    return x


# ---- 1. logits on bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, P", ALL_WORLDS + TILE_CASES + [BIG_CASE], ids=str)
def test_logits_equal_the_chain_model_on_bits_and_a_nan_row_is_skipped(cuda_device, spec, P):
    w = _world(spec, P)
    x, Wb = _with_a_hole(w), _params(w, 1)
    want, skip = R.chain_logits(x, Wb)
    assert skip.sum() == 1 and not want[skip].any()
    for denominator in (0, P):                                 # the fp32 table and the counts
        bank = _bank(x, w["y"], denominator)
        z = LP.logits_of(bank, Wb)
        assert np.array_equal(_bits(z), _bits(want)), denominator
        r = LP.loss_grad(bank, Wb, L2)
        assert (r.used, r.skipped) == (x.shape[0] - 1, 1)
        bank.close()
    plain = _bank(x)                                           # any index: labels are not needed
    assert np.array_equal(_bits(LP.logits_of(plain, Wb)), _bits(want))
    plain.close()


@pytest.mark.parametrize("C, D, rows", [(3, 16, 33), (33, 72, 257), (151, 384, 600)])
def test_logits_on_integer_worlds_are_the_float64_logits(cuda_device, C, D, rows):
    x, Wb = R.integer_world(C, D, rows, seed=C + D)
    bank = _bank(x)
    z = LP.logits_of(bank, Wb).cpu().numpy()
    assert np.array_equal(z.astype(np.float64), R.logits64(x, Wb))
    bank.close()


# ---- 2. residuals and loss against float64 from the device's logits ------------------------------------------------------------------------------
def _objective_errors(w, P, Wb):
    """(largest relative error of p behind the residuals, relative error of the data loss) of one evaluation."""
    x = _with_a_hole(w)
    bank = _bank(x, w["y"], P)
    z = LP.logits_of(bank, Wb).cpu().numpy()
    r = LP.loss_grad(bank, Wb, L2, return_residuals=True)
    bank.close()
    skip = R.skipped_rows(x)
    o = R.objective(z, x, w["y"], Wb, L2, skip)
    got = r.residuals.cpu().numpy().astype(np.float64)
    assert not got[skip].any()
    s = w["y"].astype(np.float64).sum(axis=1)
    # R = fma(s, p, -y) is one rounding of its own: u |R|; what is left is the error of s p, relative to s p
    excess = np.maximum(np.abs(got - o["R"]) - 2.0 ** -24 * np.abs(o["R"]), 0.0)[~skip]
    p_rel = float((excess / (s[:, None] * o["p"])[~skip]).max())
    l_rel = abs((r.loss - R.regulariser(Wb, L2)[0]) - o["data"]) / o["data"]
    return p_rel, l_rel


def test_residuals_and_loss_equal_float64_from_the_device_logits_within_four_times_the_measured_error(cuda_device):
    """Measured on one MI355X (profiles/r29/README.md): R.MEASURED_P_REL and R.MEASURED_L_REL; held at 4 x."""
    worst_p = worst_l = 0.0
    for spec, P in ALL_WORLDS:
        w = R.world(spec, P)
        for Wb in (_params(w, 2), _params(w, 3, 4.0)):
            p_rel, l_rel = _objective_errors(w, P, Wb)
            print(f"linprobe objective {spec} P={P}: p_rel={p_rel:.3e} l_rel={l_rel:.3e}")
            worst_p, worst_l = max(worst_p, p_rel), max(worst_l, l_rel)
    print(f"linprobe objective worst: p_rel={worst_p:.3e} l_rel={worst_l:.3e}")
    assert worst_p <= R.BOUND_P_REL and worst_l <= R.BOUND_L_REL


@pytest.mark.parametrize("spec, P", TILE_CASES + [BIG_CASE], ids=str)
def test_residuals_and_loss_on_the_tile_worlds_and_the_big_world_within_four_times_their_measured_error(cuda_device, spec, P):
    """As above at C up to 256 and at 131,195 rows, against R.MEASURED_P_REL_WIDE and R.MEASURED_L_REL_WIDE (profiles/r34/README.md), measured
    on these worlds against the float64 objective of the device's own logits.  On the big world the reference sums 131,194 float64 row
    losses: a loss tree that loses its rows at j >= 1 is off by about a half, not by 1e-8."""
    w = _world(spec, P)
    for Wb in (_params(w, 2), _params(w, 3, 4.0)):
        p_rel, l_rel = _objective_errors(w, P, Wb)
        print(f"linprobe objective {spec} P={P}: p_rel={p_rel:.3e} l_rel={l_rel:.3e}")
        assert p_rel <= R.BOUND_P_REL_WIDE and l_rel <= R.BOUND_L_REL_WIDE


def test_loss_tree_adds_the_device_row_losses_at_tree_indices_0_1_and_2(cuda_device):
    """The loss against the float64 sum of the DEVICE's row losses, in the form test_kmeans_gpu.py uses for the inertia (first-order bound of a
    float64 sum).  The ABI returns no row losses; a row's loss is a function of the row alone, so a one-row bank at l2 = 0 returns it exactly
    (one value through the tree, divided by 1).  The big world keeps 96 live rows -- at j = 0, 1 and 2 of the tree, its first and last row
    and both sides of 65,536 and 131,072 among them -- and every other row is non-finite, so its loss is the tree's sum of those 96."""
    w = R.big_world()
    Wb = _params(w, 7)
    g = np.random.default_rng(8)
    keep = np.unique(np.concatenate([[0, 65535, 65536, 131071, 131072, R.BIG_ROWS - 1], g.integers(0, 65536, 34), g.integers(65536, 131072, 40),
                                     g.integers(131072, R.BIG_ROWS, 16)]))
    keep = keep[keep != R.BIG_HOLE]
    x = w["x"].copy()
    x[np.setdiff1d(np.arange(R.BIG_ROWS), keep), 0] = np.nan
    bank = _bank(x, w["y"], 16)
    r = LP.loss_grad(bank, Wb, 0.0)
    bank.close()
    assert (r.used, r.skipped) == (len(keep), R.BIG_ROWS - len(keep))
    losses = []
    for row in keep:
        one = _bank(x[row:row + 1], w["y"][row:row + 1], 16)
        losses.append(LP.loss_grad(one, Wb, 0.0).loss)
        one.close()
    exact = math.fsum(losses) / len(keep)
    print(f"linprobe loss tree: {len(keep)} live rows, loss {r.loss!r}, float64 sum of the device's row losses / n {exact!r}")
    assert min(losses) > 0 and abs(r.loss - exact) <= R.BIG_ROWS * 2.0 ** -52 * exact


# ---- 3. the gradient ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, P", ALL_WORLDS + TILE_CASES + [BIG_CASE], ids=str)
def test_gradient_is_the_float64_gradient_of_the_device_residuals_within_the_chain_bound_and_the_same_bits_again(cuda_device, spec, P):
    w = _world(spec, P)
    x, Wb = _with_a_hole(w), _params(w, 4)
    skip = R.skipped_rows(x)
    bank, twin = _bank(x, w["y"], P), _bank(x, w["y"], 0)
    before = _live()
    r = LP.loss_grad(bank, Wb, L2, return_residuals=True)
    resid = r.residuals.cpu().numpy()
    again = LP.loss_grad(bank, Wb, L2)
    fp32 = LP.loss_grad(twin, Wb, L2)
    assert r.grad.shape == (w["C"], w["D"] + 1) and r.grad.dtype == np.float64
    assert np.array_equal(_bits(r.grad), _bits(again.grad)) and r.loss == again.loss              # two calls: equal bits
    assert np.array_equal(_bits(r.grad), _bits(fp32.grad)) and r.loss == fp32.loss                # counts and their fp32 twin: equal bits
    _assert_gradient_within_the_chain_bound(r, resid, x, skip, Wb, spec)
    assert _live() == before                                   # every buffer of the calls is gone
    bank.close(); twin.close()


def _assert_gradient_within_the_chain_bound(r, resid, x, skip, Wb, tag):
    aug = np.concatenate([np.ones((x.shape[0], 1)), np.where(skip[:, None], 0.0, x.astype(np.float64))], axis=1)
    sums = resid.astype(np.float64).T @ aug
    g64 = sums / r.used + L2 * Wb.astype(np.float64)
    # the chain's bound, and the float64 sums on both sides of the comparison (this test's own dot product over the rows: rows x 2^-53 at the
    # worst; the engine's segment adds, division and l2 term: a few units more)
    mass = np.abs(resid.astype(np.float64)).T @ np.abs(aug) / r.used
    bound = R.gradient_bound(resid, x, skip) + x.shape[0] * 2.0 ** -52 * (mass + L2 * np.abs(Wb))
    err = np.abs(r.grad - g64)
    print(f"linprobe gradient {tag}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    # ... and the model's segment order gives the same gradient within float64 rounding of the model's own fma emulation
    seg = R.segment_gradient(resid, x, skip, Wb, L2)
    assert (np.abs(seg - r.grad) <= 2 * bound).all()


# ---- 3b. the workspace chunk loop: nothing depends on it ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, P, segs", CHUNK_CASES, ids=str)
def test_workspace_chunks_do_not_show_in_any_output(cuda_device, spec, P, segs):
    """hb_linprobe_set_workspace makes the host loop run in chunks of `segs` segments (a.row0 > 0: residuals, staged rows, skip flags and row
    losses by their chunk-local or bank-wide index, the float64 accumulator carried across chunks); gradient, loss, used rows and residuals
    equal the default workspace's on bits, and the gradient is inside the float64 bound on its own."""
    w = _world(spec, P)
    x, Wb = _with_a_hole(w), _params(w, 5)
    skip = R.skipped_rows(x)
    assert len(R.chunks(x.shape[0], segs)) > 1 and len(R.chunks(x.shape[0], (1 << 30) // seg_bytes(spec))) == 1
    bank = _bank(x, w["y"], P)
    before = _live()
    whole = LP.loss_grad(bank, Wb, L2, return_residuals=True)
    with _workspace(segs * seg_bytes(spec)):
        parts = LP.loss_grad(bank, Wb, L2, return_residuals=True)
    with _workspace(segs * seg_bytes(spec) + seg_bytes(spec) - 1):      # one byte short of another segment: the same chunks
        ragged = LP.loss_grad(bank, Wb, L2)
    assert np.array_equal(_bits(parts.grad), _bits(whole.grad)) and np.array_equal(_bits(ragged.grad), _bits(whole.grad))
    assert parts.loss == whole.loss == ragged.loss and parts.used == whole.used == ragged.used == x.shape[0] - 1
    resid = parts.residuals.cpu().numpy()
    assert np.array_equal(_bits(resid), _bits(whole.residuals))
    _assert_gradient_within_the_chain_bound(parts, resid, x, skip, Wb, f"{spec} in chunks of {segs}")
    del whole, parts
    assert _live() == before
    bank.close()


def test_a_workspace_below_one_segment_is_one_segment_and_the_setter_refuses_negative_values(cuda_device):
    w = R.world(R.SEGMENT_WORLD)
    Wb = _params(w, 6)
    bank = _bank(w["x"], w["y"], 16)
    whole = LP.loss_grad(bank, Wb, L2)
    with _workspace(1):
        tiny = LP.loss_grad(bank, Wb, L2)
    assert np.array_equal(_bits(tiny.grad), _bits(whole.grad)) and tiny.loss == whole.loss
    assert _lib.lib().hb_linprobe_set_workspace(-1) != 0 and "hb_linprobe_set_workspace" in _lib.last_error()
    after = LP.loss_grad(bank, Wb, L2)                         # the refused call changed nothing
    assert np.array_equal(_bits(after.grad), _bits(whole.grad))
    bank.close()


# ---- 4. the fit -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", R.WORLDS, ids=str)
def test_fit_converges_to_the_float64_optimum_and_classifies_like_it(cuda_device, spec):
    w = R.fit_world(spec)
    bank = _bank(w["x"], w["y"], 16)
    before = _live()
    probe = LP.linear_probe_fit(bank, l2=R.FIT_L2, gtol=R.FIT_GTOL)
    assert _live() == before
    assert probe.state == "converged" and probe.rows_used == w["x"].shape[0] and probe.rows_skipped == 0
    assert len(probe.history) == probe.n_iter + 1 and probe.history[-1]["gmax"] <= R.FIT_GTOL
    Wb = probe.Wb.cpu().numpy()
    g64 = R.objective64(w["x"], w["y"], Wb, R.FIT_L2)["grad"]
    print(f"linprobe fit {spec}: {probe.n_iter} iterations, float64 gmax {np.abs(g64).max():.3e}")
    assert np.abs(g64).max() <= 2 * R.FIT_GTOL
    thr = 2.0 * np.sqrt(2.0) * float(np.linalg.norm(g64)) / R.FIT_L2
    judged = w["val_margin"] > thr
    assert (~judged).mean() <= R.VAL_CAP
    z = probe.logits(torch.from_numpy(w["xv"]).cuda())
    assert tuple(z.shape) == (w["xv"].shape[0], w["C"])
    got = z.argmax(dim=1).cpu().numpy()
    assert np.array_equal(got[judged], w["val_argmax"][judged])
    z3 = probe.logits(torch.from_numpy(w["xv"]).cuda().view(4, -1, w["D"]))      # [B, N, D] -> [B, N, C]
    assert tuple(z3.shape) == (4, w["xv"].shape[0] // 4, w["C"]) and torch.equal(z3.view(-1, w["C"]), z)
    probe.close(); bank.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(cuda_device):
    w = R.world(R.WORLDS[0])
    bank, plain = _bank(w["x"], w["y"], 16), _bank(w["x"])
    L = _lib.lib()
    multi = HipMultiIndex(16, 0, [0, 0], shard=True)
    for call in (lambda: LP.linear_probe_fit(multi), lambda: LP.loss_grad(multi, _params(w, 1), L2), lambda: LP.logits_of(multi, _params(w, 1))):
        with pytest.raises(ValueError, match="HipMultiIndex"):
            call()
    multi.close()
    before = _live()
    with pytest.raises(ValueError, match=r"\[1, 256\]"):
        LP.logits_of(plain, np.zeros((257, 17), dtype=np.float32))
    with pytest.raises(ValueError, match="no label row"):
        LP.linear_probe_fit(plain)
    with pytest.raises(ValueError, match="no label row"):
        LP.loss_grad(plain, _params(w, 1), L2)
    with pytest.raises(ValueError, match="differs from the label table's 3 classes"):
        LP.loss_grad(bank, np.zeros((4, 17), dtype=np.float32), L2)
    with pytest.raises(ValueError, match=r"\[C, 17\]"):
        LP.loss_grad(bank, np.zeros((3, 16), dtype=np.float32), L2)
    # the C entries themselves: outputs untouched, nothing allocated
    wb = torch.zeros(257, 17, device="cuda")
    out = torch.full((600, 257), 7.0, device="cuda")
    grad = torch.full((257, 17), 7.0, dtype=torch.float64, device="cuda")
    loss, used = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for C, msg in ((257, "[1, 256]"), (0, "[1, 256]")):
        assert L.hb_linprobe_logits(bank._h, p(wb), C, p(out)) != 0 and msg in _lib.last_error()
        assert L.hb_linprobe_loss_grad(bank._h, p(wb), C, 0.01, ctypes.byref(loss), p(grad), ctypes.byref(used), None) != 0 and msg in _lib.last_error()
    assert L.hb_linprobe_loss_grad(bank._h, p(wb), 4, 0.01, ctypes.byref(loss), p(grad), ctypes.byref(used), None) != 0 and "differs" in _lib.last_error()
    assert L.hb_linprobe_loss_grad(plain._h, p(wb), 3, 0.01, ctypes.byref(loss), p(grad), ctypes.byref(used), None) != 0 and "no label row" in _lib.last_error()
    assert L.hb_linprobe_loss_grad(bank._h, p(wb), 3, 0.01, ctypes.byref(loss), None, ctypes.byref(used), None) != 0 and "NULL pointer" in _lib.last_error()
    empty = HipFlatIndex(16, 0, 0)
    assert L.hb_linprobe_logits(empty._h, p(wb), 3, p(out)) != 0 and "empty" in _lib.last_error()
    assert L.hb_linprobe_loss_grad(empty._h, p(wb), 3, 0.01, ctypes.byref(loss), p(grad), ctypes.byref(used), None) != 0 and "empty" in _lib.last_error()
    empty.close()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((grad == 7.0).all()) and loss.value == -1.0 and used.value == -1
    assert _live() == before
    bank.close(); plain.close()
