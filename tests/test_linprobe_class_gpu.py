"""The image-level linear probe on the GPU (include/hbird_hip_linprobe_class.h, hbird_mi/linear_probe.py, hbird_mi/ops.py) against the numpy
model of tests/linprobe_class_refs.py: logits on bits at every class-sweep shape, one definition with the segmentation probe at C <= 256 (equal
bits on the one-hot twin bank), skipped rows, residuals and loss against float64 from the device's own logits, the gradient inside an fma
chain's bound of the float64 gradient of the device's own residuals and the same bits twice, workspace chunks, the big seam once, the fit
against the float64 optimum, the top-n kernel against numpy lexsort, refusals.  The case lists are held to the sweep and chunk arithmetic by
tests/test_linprobe_class_cpu.py, without a GPU."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import linprobe_class_refs as K
import linprobe_refs as R
from hbird_mi import _lib, ops
from hbird_mi import linear_probe as LP
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

pytestmark = pytest.mark.gpu
L2 = R.FIT_L2


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


@contextlib.contextmanager
def _workspace(nbytes):
    _lib.check(_lib.lib().hb_linprobe_set_workspace(int(nbytes)))
    try:
        yield
    finally:
        _lib.check(_lib.lib().hb_linprobe_set_workspace(0))


def _world(C, D, rows, hole=37):
    return K.class_world(C, D, rows, R.BIG_HOLE if rows == R.BIG_ROWS else hole)      # (the big world's hole is R.big_world's, past row 65,536)


def _params(C, D, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((C, D + 1)) * scale).astype(np.float32)


# ---- 1. logits on bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, D", [(C, 16) for C in K.LOGIT_CS] + list(K.LOGIT_WIDE), ids=str)
def test_logits_equal_the_chain_model_on_bits_at_every_sweep_shape_and_a_nan_row_is_skipped(cuda_device, C, D):
    w = _world(C, D, K.ROWS)
    x, Wb = w["x"], _params(C, D, 1)
    want, skip = R.chain_logits(x, Wb)
    assert skip.sum() == 1 and not want[skip].any()
    bank = _bank(x)
    z = LP.class_logits_of(bank, Wb)
    assert np.array_equal(_bits(z), _bits(want))
    if C <= _lib.LINPROBE_MAX_C:                               # ... and the segmentation probe's entry gives the same bits
        assert np.array_equal(_bits(LP.logits_of(bank, Wb)), _bits(want))
    bank.close()


@pytest.mark.parametrize("C, D, rows", [(257, 16, 33), (513, 72, 257), (1000, 384, 300)])
def test_logits_on_integer_worlds_are_the_float64_logits(cuda_device, C, D, rows):
    x, Wb = R.integer_world(C, D, rows, seed=C + D)
    bank = _bank(x)
    z = LP.class_logits_of(bank, Wb).cpu().numpy()
    assert np.array_equal(z.astype(np.float64), R.logits64(x, Wb))
    bank.close()


# ---- 2. one definition at every C ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.TWIN_CS)
def test_class_ids_and_the_one_hot_twin_bank_give_equal_bits(cuda_device, C):
    w = _world(C, 16, K.ROWS, None)
    Wb, y = _params(C, 16, 2), K.one_hot(w["cls"], C)
    bank = _bank(w["x"])
    r = LP.class_loss_grad(bank, w["cls"], Wb, L2, return_residuals=True)
    assert (r.used, r.skipped) == (K.ROWS, 0)
    for twin in (_bank(w["x"], y, 0), _bank(w["x"], y, 16)):      # an fp32 table; counts with P = 16
        t = LP.loss_grad(twin, Wb, L2, return_residuals=True)
        assert r.loss == t.loss and r.used == t.used
        assert np.array_equal(_bits(r.grad), _bits(t.grad)) and np.array_equal(_bits(r.residuals), _bits(t.residuals))
        twin.close()
    bank.close()


# ---- 3. skips -----------------------------------------------------------------------------------------------------------------------------------
def test_a_row_without_a_label_is_skipped_like_a_non_finite_row_and_a_label_out_of_range_is_refused(cuda_device):
    C, D = 257, 16
    w = _world(C, D, K.ROWS)
    x, cls, Wb = w["x"], w["cls"].copy(), _params(C, D, 3)
    cls[101] = -1
    bank = _bank(x)
    r = LP.class_loss_grad(bank, cls, Wb, 0.0, return_residuals=True)
    assert (r.used, r.skipped) == (K.ROWS - 2, 2)
    resid = r.residuals.cpu().numpy()
    assert not resid[[37, 101]].any() and resid[[36, 38, 100, 102]].any(axis=1).all()
    keep = np.setdiff1d(np.arange(K.ROWS), [37, 101])
    losses = []
    for row in keep:                                           # a one-row bank at l2 = 0 returns the device's row loss exactly
        one = _bank(x[row:row + 1])
        losses.append(LP.class_loss_grad(one, cls[row:row + 1], Wb, 0.0).loss)
        one.close()
    exact = math.fsum(losses) / len(keep)
    assert min(losses) > 0 and abs(r.loss - exact) <= K.ROWS * 2.0 ** -52 * exact
    # a label equal to C, and a label -2: refused with outputs untouched
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wb = torch.from_numpy(Wb).cuda()
    grad = torch.full((C, D + 1), 7.0, dtype=torch.float64, device="cuda")
    res = torch.full((K.ROWS, C), 7.0, device="cuda")
    before = _live()
    for bad in (C, -2):
        lab = torch.from_numpy(cls.astype(np.int32)).cuda()
        lab[200] = bad
        loss, used = ctypes.c_double(-1.0), ctypes.c_int64(-1)
        assert L.hb_linprobe_class_loss_grad(bank._h, p(lab), p(wb), C, 0.0, ctypes.byref(loss), p(grad), ctypes.byref(used), p(res)) != 0
        assert f"outside [-1, {C})" in _lib.last_error()
        torch.cuda.synchronize()
        assert bool((grad == 7.0).all()) and bool((res == 7.0).all()) and loss.value == -1.0 and used.value == -1
        with pytest.raises(ValueError, match="outside"):
            LP.class_loss_grad(bank, lab, Wb, 0.0)
    assert _live() == before
    bank.close()


# ---- 4. residuals and loss against float64 from the device's logits --------------------------------------------------------------------------------
def _objective_errors(C, D, Wb):
    """(largest relative error of p behind the residuals, relative error of the data loss) of one evaluation."""
    w = _world(C, D, K.ROWS)
    x, cls = w["x"], w["cls"]
    bank = _bank(x)
    z = LP.class_logits_of(bank, Wb).cpu().numpy()
    r = LP.class_loss_grad(bank, cls, Wb, L2, return_residuals=True)
    bank.close()
    skip = K.skipped(x, cls)
    o = K.objective(z, x, cls, Wb, L2)
    got = r.residuals.cpu().numpy().astype(np.float64)
    assert not got[skip].any()
    # R = p - [c == y] is one rounding of its own: u |R|; what is left is the error of p, relative to p
    excess = np.maximum(np.abs(got - o["R"]) - 2.0 ** -24 * np.abs(o["R"]), 0.0)[~skip]
    p_rel = float((excess / o["p"][~skip]).max())
    l_rel = abs((r.loss - R.regulariser(Wb, L2)[0]) - o["data"]) / o["data"]
    return p_rel, l_rel


@pytest.mark.parametrize("C", K.OBJECTIVE_CS)
def test_residuals_and_loss_equal_float64_from_the_device_logits_within_four_times_the_measured_error(cuda_device, C):
    """Measured on one MI355X (profiles/r36/README.md): K.MEASURED_P_REL_CLASS and K.MEASURED_L_REL_CLASS; held at 4 x."""
    for Wb in (_params(C, 16, 2), _params(C, 16, 3, 4.0)):
        p_rel, l_rel = _objective_errors(C, 16, Wb)
        print(f"linprobe class objective C={C}: p_rel={p_rel:.3e} l_rel={l_rel:.3e}")
        assert p_rel <= 4 * K.MEASURED_P_REL_CLASS and l_rel <= 4 * K.MEASURED_L_REL_CLASS


# ---- 5. the gradient ------------------------------------------------------------------------------------------------------------------------------
def _assert_gradient_within_the_chain_bound(r, resid, x, skip, Wb, l2, tag):
    aug = np.concatenate([np.ones((x.shape[0], 1)), np.where(skip[:, None], 0.0, x.astype(np.float64))], axis=1)
    g64 = resid.astype(np.float64).T @ aug / r.used + l2 * Wb.astype(np.float64)
    mass = np.abs(resid.astype(np.float64)).T @ np.abs(aug) / r.used
    bound = R.gradient_bound(resid, x, skip) + x.shape[0] * 2.0 ** -52 * (mass + l2 * np.abs(Wb))
    err = np.abs(r.grad - g64)
    print(f"linprobe class gradient {tag}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()


def _gradient_case(C, D, rows, seed=4):
    w = _world(C, D, rows)
    x, cls, Wb = w["x"], w["cls"], _params(C, D, seed)
    skip = K.skipped(x, cls)
    bank = _bank(x)
    before = _live()
    r = LP.class_loss_grad(bank, cls, Wb, L2, return_residuals=True)
    resid = r.residuals.cpu().numpy()
    again = LP.class_loss_grad(bank, cls, Wb, L2)
    assert r.grad.shape == (C, D + 1) and r.grad.dtype == np.float64 and r.used == rows - 1
    assert np.array_equal(_bits(r.grad), _bits(again.grad)) and r.loss == again.loss              # two calls: equal bits
    _assert_gradient_within_the_chain_bound(r, resid, x, skip, Wb, L2, (C, D, rows))
    del r, again
    assert _live() == before                                   # every buffer of the calls is gone
    bank.close()


@pytest.mark.parametrize("C, D", [(C, 16) for C in K.OBJECTIVE_CS] + list(K.GRADIENT_WIDE), ids=str)
def test_gradient_is_the_float64_gradient_of_the_device_residuals_within_the_chain_bound_and_the_same_bits_again(cuda_device, C, D):
    _gradient_case(C, D, K.ROWS)


# ---- 6. the workspace chunk loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, D, rows", K.CHUNK_CASES, ids=str)
def test_workspace_chunks_do_not_show_in_any_output(cuda_device, C, D, rows):
    w = _world(C, D, rows)
    x, cls, Wb = w["x"], w["cls"], _params(C, D, 5)
    seg = K.seg_bytes(C, D, rows)
    bank = _bank(x)
    before = _live()
    whole = LP.class_loss_grad(bank, cls, Wb, L2, return_residuals=True)
    with _workspace(seg):
        parts = LP.class_loss_grad(bank, cls, Wb, L2, return_residuals=True)
    with _workspace(seg + seg - 1):                            # one byte short of another segment: the same chunks
        ragged = LP.class_loss_grad(bank, cls, Wb, L2, return_residuals=True)
    for other in (parts, ragged):
        assert np.array_equal(_bits(other.grad), _bits(whole.grad)) and other.loss == whole.loss and other.used == whole.used == rows - 1
        assert np.array_equal(_bits(other.residuals), _bits(whole.residuals))
    del whole, parts, ragged, other
    assert _live() == before
    bank.close()


# ---- 7. the big seam, once ----------------------------------------------------------------------------------------------------------------------
def test_gradient_at_the_big_seam(cuda_device):
    _gradient_case(*K.BIG_CASE)


# ---- 8. the fit ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, l2", K.FIT_CASES, ids=str)
def test_fit_converges_to_the_float64_optimum_and_classifies_like_it(cuda_device, spec, l2):
    w = K.fit_world(spec, l2)
    bank = _bank(w["x"])
    before = _live()
    probe = LP.linear_probe_fit_classes(bank, w["cls"], w["C"], l2=l2, gtol=K.FIT_GTOL)
    assert _live() == before
    assert probe.state == "converged" and probe.rows_used == w["x"].shape[0] and probe.rows_skipped == 0
    assert len(probe.history) == probe.n_iter + 1 and probe.history[-1]["gmax"] <= K.FIT_GTOL
    Wb = probe.Wb.cpu().numpy()
    g64 = R.objective64(w["x"], w["y"], Wb, l2)["grad"]
    print(f"linprobe class fit {spec}: {probe.n_iter} iterations, float64 gmax {np.abs(g64).max():.3e}")
    assert np.abs(g64).max() <= 2 * K.FIT_GTOL
    thr = 2.0 * np.sqrt(2.0) * float(np.linalg.norm(g64)) / l2
    judged = w["val_margin"] > thr
    assert (~judged).mean() <= R.VAL_CAP
    z = probe.logits(torch.from_numpy(w["xv"]).cuda())
    assert tuple(z.shape) == (w["xv"].shape[0], w["C"])
    assert np.array_equal(z.argmax(dim=1).cpu().numpy()[judged], w["val_argmax"][judged])
    warm = LP.linear_probe_fit_classes(bank, w["cls"], w["C"], l2=l2, gtol=K.FIT_GTOL, Wb0=probe.Wb)      # a warm start at the answer
    assert warm.state == "converged" and warm.n_iter == 0 and torch.equal(warm.Wb, probe.Wb)
    probe.close(); warm.close(); bank.close()


# ---- 9. hb_logits_topn ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, topn", [(3, 5), (64, 1), (65, 8), (1000, 5)])
def test_logits_topn_equals_numpy_lexsort_with_ties_and_a_nan_column(cuda_device, C, topn):
    g = np.random.default_rng(90 + C)
    z = g.standard_normal((37, C)).astype(np.float32)
    z[:, C // 2] = np.nan                                      # a NaN column
    z[1] = np.round(z[1])                                      # ties
    z[2] = 0.5
    z[3, ::2] = -0.0; z[3, 1::2] = 0.0                         # -0 == 0: a tie
    z[4] = np.nan                                              # no number at all: all -1
    z[5, : max(1, C - 2)] = np.nan                             # fewer numbers than topn
    z[6] = -np.inf; z[6, C - 1] = np.inf                       # infinities are numbers
    pred = ops.logits_topn(torch.from_numpy(z).cuda(), topn).cpu().numpy()
    want = K.topn(z, topn)
    assert pred.dtype == np.int32 and np.array_equal(pred, want)
    assert (want[4] == -1).all() and (C >= topn or (want[:, C:] == -1).all())
    empty = ops.logits_topn(torch.empty((0, C), device="cuda"), topn)
    assert tuple(empty.shape) == (0, topn)
    assert _lib.lib().hb_logits_topn(None, 0, C, topn, None, None) != 0      # nq == 0 returns 0 only for valid arguments
    dummy = torch.zeros(1, device="cuda")
    assert _lib.lib().hb_logits_topn(ctypes.c_void_p(dummy.data_ptr()), 0, C, topn, ctypes.c_void_p(dummy.data_ptr()), None) == 0


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(cuda_device):
    C, D = 257, 16
    w = _world(C, D, K.ROWS)
    bank = _bank(w["x"])
    Wb = _params(C, D, 1)
    multi = HipMultiIndex(16, 0, [0, 0], shard=True)
    for call in (lambda: LP.linear_probe_fit_classes(multi, w["cls"], C), lambda: LP.class_loss_grad(multi, w["cls"], Wb, L2),
                 lambda: LP.class_logits_of(multi, Wb)):
        with pytest.raises(ValueError, match="HipMultiIndex"):
            call()
    multi.close()
    before = _live()
    with pytest.raises(ValueError, match=r"\[1, 16384\]"):
        LP.class_logits_of(bank, np.zeros((16385, D + 1), dtype=np.float32))
    with pytest.raises(ValueError, match=r"\[1, 16384\]"):
        LP.linear_probe_fit_classes(bank, w["cls"], 16385)
    with pytest.raises(ValueError, match="299 labels for a bank of 300 rows"):
        LP.class_loss_grad(bank, w["cls"][:-1], Wb, L2)
    with pytest.raises(ValueError, match="integer"):
        LP.class_loss_grad(bank, w["cls"].astype(np.float32), Wb, L2)
    with pytest.raises(ValueError, match=r"\[C, 17\]"):
        LP.class_loss_grad(bank, w["cls"], np.zeros((C, D), dtype=np.float32), L2)
    with pytest.raises(ValueError, match="topn"):
        ops.logits_topn(torch.zeros((4, 8), device="cuda"), 9)
    # the C entries themselves: outputs untouched, nothing allocated
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    wb = torch.zeros(C, D + 1, device="cuda")
    lab = torch.zeros(K.ROWS, dtype=torch.int32, device="cuda")
    out = torch.full((K.ROWS, C), 7.0, device="cuda")
    grad = torch.full((C, D + 1), 7.0, dtype=torch.float64, device="cuda")
    pred = torch.full((K.ROWS, 8), 7, dtype=torch.int32, device="cuda")
    loss, used = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    args = (ctypes.byref(loss), p(grad), ctypes.byref(used), None)
    for bad_c in (16385, 0):
        assert L.hb_linprobe_class_logits(bank._h, p(wb), bad_c, p(out)) != 0 and "[1, 16384]" in _lib.last_error()
        assert L.hb_linprobe_class_loss_grad(bank._h, p(lab), p(wb), bad_c, 0.01, *args) != 0 and "[1, 16384]" in _lib.last_error()
        assert L.hb_logits_topn(p(out), K.ROWS, bad_c, 5, p(pred), None) != 0 and "[1, 16384]" in _lib.last_error()
    assert L.hb_linprobe_class_logits(None, p(wb), C, p(out)) != 0 and "NULL index handle" in _lib.last_error()
    assert L.hb_linprobe_class_logits(bank._h, None, C, p(out)) != 0 and "NULL pointer" in _lib.last_error()
    assert L.hb_linprobe_class_loss_grad(None, p(lab), p(wb), C, 0.01, *args) != 0 and "NULL index handle" in _lib.last_error()
    assert L.hb_linprobe_class_loss_grad(bank._h, None, p(wb), C, 0.01, *args) != 0 and "NULL pointer" in _lib.last_error()
    assert L.hb_linprobe_class_loss_grad(bank._h, p(lab), p(wb), C, 0.01, ctypes.byref(loss), None, ctypes.byref(used), None) != 0
    assert "NULL pointer" in _lib.last_error()
    for bad_top in (0, 9):
        assert L.hb_logits_topn(p(out), K.ROWS, C, bad_top, p(pred), None) != 0 and "topn outside [1, 8]" in _lib.last_error()
    assert L.hb_logits_topn(None, K.ROWS, C, 5, p(pred), None) != 0 and "NULL pointer" in _lib.last_error()
    empty = HipFlatIndex(16, 0, 0)
    assert L.hb_linprobe_class_logits(empty._h, p(wb), C, p(out)) != 0 and "empty" in _lib.last_error()
    assert L.hb_linprobe_class_loss_grad(empty._h, p(lab), p(wb), C, 0.01, *args) != 0 and "empty" in _lib.last_error()
    empty.close()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((grad == 7.0).all()) and bool((pred == 7).all()) and loss.value == -1.0 and used.value == -1
    assert _live() == before
    bank.close()


# ---- 10. the evaluator ------------------------------------------------------------------------------------------------------------------------------
def _row_means(x):
    return x.mean(dim=3).reshape(x.shape[0], -1)               # a tiny feature: the mean of every image row per channel, [B, 3 S]


def test_evaluator_counts_equal_numpy_from_the_probe_logits_and_the_cli_reports_them(cuda_device, tmp_path, capsys):
    import importlib.util
    import json
    import os

    from hbird_mi import classify as hclassify
    from hbird_mi.data.classify import SyntheticClassifyDataModule
    dm = SyntheticClassifyDataModule(batch_size=16, input_size=32, num_classes=12, n_train=192, n_val=60, noise=0.5)
    ev = hclassify.HbirdKnnClassification(_row_means, 12, n_neighbours=(1,), topn=5).build(dm.train_dataloader())
    val = [(x, y.clone()) for x, y in dm.val_dataloader()]
    val[1][1][3] = -1                                          # an unlabelled query
    l2s = (1e-3, 1e-2)
    res = ev.evaluate_linear_probe(val, l2s=l2s)
    assert res.l2s == list(l2s) and (res.n, res.skipped) == (59, 1) and set(res.fits) == set(l2s)
    assert all(f["state"] == "converged" and f["rows_used"] == 192 and f["rows_skipped"] == 0 for f in res.fits.values())
    # the same fits by hand (descending l2, warm-started), probe.logits + numpy top-n + numpy counts
    qlab = np.concatenate([y.numpy() for _, y in val])
    warm, want = None, {}
    for v in sorted(l2s, reverse=True):
        probe = ev.fit_linear_probe(l2=v, Wb0=warm)
        warm = probe.Wb
        z = np.concatenate([probe.logits(_row_means(x.cuda())).cpu().numpy() for x, _ in val])      # (logits normalises the rows)
        want[v] = K.counts(K.topn(z, 5), qlab, 12)
        probe.close()
    for i, v in enumerate(l2s):
        c, per, n = want[v]
        assert np.array_equal(res.counts[i], c) and np.array_equal(res.class_counts[i], per) and n == res.n
        assert res.top1[v] == c[0] / n and res.topn[v] == c[-1] / n
        seen = per[:, 0] > 0
        assert res.mean_per_class[v] == float(np.mean(per[seen, 1] / per[seen, 0]))
    assert res.best() == max(((v, res.top1[v]) for v in l2s), key=lambda t: t[1]) and res.top1[res.best()[0]] > 0.5
    # two l2 values out of one pass equal two separate calls
    for i, v in enumerate(l2s):
        one = ev.evaluate_linear_probe(val, l2s=(v,))
        assert one.fits[v]["state"] == "converged" and np.array_equal(one.counts[0], res.counts[i]) and np.array_equal(one.class_counts[0], res.class_counts[i])
    view = ev.memory_view(images=np.arange(0, 192, 2))         # a label-subset probe is an ordinary instance
    sub = view.evaluate_linear_probe(val, l2s=(1e-2,))
    assert sub.n == 59 and sub.fits[1e-2]["rows_used"] == 96 and 0.0 <= sub.top1[1e-2] <= 1.0
    view.close()
    with pytest.raises(ValueError, match="l2s"):
        ev.evaluate_linear_probe(val, l2s=(1e-3, 1e-3))
    ev.close()
    # the command-line front end
    spec = importlib.util.spec_from_file_location("hbird_cli_linear", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = tmp_path / "linear.json"
    cli.main(["--task", "linear-classify", "--probe-l2", "1e-2", "1e-3", "--top-n", "3", "--dataset-name", "synthetic-classify", "--data-dir", "",
              "--d-model", "3", "--patch-size", "8", "--input-size", "32", "--out", str(out)])
    capsys.readouterr()
    js = json.loads(out.read_text())
    keys = ["l2=0.01", "l2=0.001"]
    assert js["task"] == "linear-classify" and js["top_n"] == 3 and js["n"] + js["skipped"] == 60
    for name in ("top1", "top3", "mean_per_class", "fits"):
        assert list(js[name]) == keys, name
    assert set(js["fits"]["l2=0.01"]) == {"state", "n_iter", "rows_used", "rows_skipped"} and js["best"]["key"] in keys
    assert js["best"]["top1"] == max(js["top1"].values())
