"""The image-level linear probe of include/hbird_hip_linprobe_class.h restated in plain numpy on top of tests/linprobe_refs.py, the case lists of
tests/test_linprobe_class_gpu.py and the arithmetic they are held to (tests/test_linprobe_class_cpu.py).  No engine code.

  one_hot(cls, C)                    the label rows of the twin bank: float32 [rows, C], a row of label -1 all zeros
  skipped(x, cls)                    a row is skipped for a non-finite component or for label -1
  objective(z, x, cls, Wb, l2)       linprobe_refs.objective on the one-hot rows with that skip mask: s = 1, l = lse - z[y], R = p - [c == y]
  class_world(C, D, rows, hole)      unit rows around class centres with one non-finite row, and their class ids
  sweeps(C)                          the class tiles of every sweep of the forward (groups of SWEEP_TILES = 8 tiles of 32 classes)
  backward_waves(C, D)               (class-tile groups, column-tile groups, tiles in the last of each) of the backward wave tile at cp > 256
  topn(z, n)                         hb_logits_topn by numpy lexsort
  fit_world(spec, l2)                a hard-label world with the restated fit, the float64 optimum by float64 L-BFGS, and its cap

Bounds of test 4 (residuals and loss against float64 from the device's own logits, C in {257, 513, 1000}, parameters of scale 1 and 4),
measured on one MI355X (profiles/r36/README.md) as linprobe_refs.MEASURED_P_REL was: the largest relative error of p behind a residual and of
the data loss; the test holds 4 x these, because the device's expf / logf may move with the ROCm version.
"""
import functools

import numpy as np

import linprobe_refs as R

MEASURED_P_REL_CLASS = 3.22e-6   # C = 1000 at parameters of scale 4 (257: 2.80e-6, 513: 2.83e-6; scale 1: 1.12e-6 .. 1.35e-6)
MEASURED_L_REL_CLASS = 1.75e-8   # C = 1000 at parameters of scale 1 (257: 1.25e-8, 513: 1.67e-8)

SWEEP_TILES = 8                  # LPC_SWEEP: class tiles of one forward sweep
MAX_C = 16384                    # HB_LINPROBE_CLASS_MAX_C
BWD_WIDE = (4, 2)                # class tiles x column tiles of a backward wave at cp > 256 (LP_BWD_WIDE_CTW, LP_BWD_WIDE_DTW)
ROWS = 300                       # two forward workgroups, two segments (linprobe_refs.TILE_ROWS)

# test 1: both ends of the first class group (256, 257: one live class in the second sweep), of the second (512, 513), every remainder sweep
# of 1 .. 7 tiles after a full one (256 + 32 k) and as the only one (32 k), a ragged last tile (3, 33, 151, 1000)
LOGIT_CS = (3, 33, 64, 96, 128, 151, 160, 192, 224, 256, 257, 288, 320, 352, 384, 416, 448, 480, 512, 513, 1000)
LOGIT_WIDE = ((257, 72), (300, 384))                       # (C, D): width padded to 80, and a wide bank
TWIN_CS = (3, 33, 151, 256)                                # test 2: the existing kernel's range
OBJECTIVE_CS = (257, 513, 1000)                            # tests 4 and 5
GRADIENT_WIDE = ((1000, 72), (513, 384))                   # test 5: ragged column-tile pairs (3, 13) and a ragged class-tile group (17 = 4 x 4 + 1)
CHUNK_CASES = ((257, 16, 513), (1000, 16, ROWS))           # test 6: (C, D, rows)
BIG_CASE = (257, 16, R.BIG_ROWS)                           # test 7
# test 8: (C, D, rows, n_val, seed, sigma), l2
FIT_CASES = (((300, 72, 3000, 1024, 72, 0.1), 1e-4), ((257, 72, 3000, 1024, 73, 0.1), 1e-4), ((5, 16, 600, 1024, 71, 0.3), 1e-2))
FIT_GTOL = 1e-5
OPTIMUM_GTOL = 1e-9


@functools.lru_cache(maxsize=None)
def class_world(C, D, rows, hole=37):
    """dict(x float32 [rows, D] unit rows around C class centres (sigma 0.2) with ONE non-finite row `hole`, cls int64 [rows], C, D): the
    hard-label worlds of the GPU tests, drawn as linprobe_refs.draw_world draws its rows but without a [rows, C] count table."""
    g = np.random.default_rng(1000 + C + D)
    centres = R._unit(g.standard_normal((C, D)))
    cls = g.integers(0, C, rows)
    x = R._unit(centres[cls].astype(np.float64) + 0.2 * g.standard_normal((rows, D)))
    if hole is not None:
        x[hole, 5] = np.nan
    return dict(x=x, cls=cls, C=C, D=D)


def one_hot(cls, C):
    cls = np.asarray(cls)
    y = np.zeros((cls.shape[0], C), dtype=np.float32)
    keep = cls >= 0
    y[np.flatnonzero(keep), cls[keep]] = 1.0
    return y


def skipped(x, cls):
    return R.skipped_rows(x) | (np.asarray(cls) < 0)


def objective(z, x, cls, Wb, l2):
    """float64 from the logits z: linprobe_refs.objective with one-hot rows; a row of label -1 is skipped like a non-finite one."""
    return R.objective(z, x, one_hot(cls, np.asarray(Wb).shape[0]), Wb, l2, skipped(x, cls))


def sweeps(C):
    ct = -(-C // 32)
    return [min(SWEEP_TILES, ct - t0) for t0 in range(0, ct, SWEEP_TILES)]


def backward_waves(C, D):
    """At cp > 256: (groups of class tiles, tiles in the last group, groups of column tiles, tiles in the last group)."""
    ct, dt = -(-C // 32), -(-(D + 1) // 32)
    return -(-ct // BWD_WIDE[0]), ct - (-(-ct // BWD_WIDE[0]) - 1) * BWD_WIDE[0], -(-dt // BWD_WIDE[1]), dt - (-(-dt // BWD_WIDE[1]) - 1) * BWD_WIDE[1]


def seg_bytes(C, D, rows):
    """Bytes of one segment in the workspace: seg_rows * (cp + xs) * 4."""
    return R.partition(rows)[0] * (32 * -(-C // 32) + 32 * -(-(D + 1) // 32)) * 4


def topn(z, n):
    """pred int32 [nq, n]: logit descending, ties to the lower class id, a NaN never written, -1 in the tail."""
    z = np.asarray(z, dtype=np.float32)
    out = np.full((z.shape[0], n), -1, dtype=np.int32)
    for q in range(z.shape[0]):
        ok = np.flatnonzero(~np.isnan(z[q]))
        order = ok[np.lexsort((ok, -z[q][ok].astype(np.float64)))][:n]
        out[q, :len(order)] = order
    return out


def counts(pred, qlabels, C):
    """hb_vote_counts for one configuration by numpy: (counts [topn], class_counts [C, 2], n)."""
    pred, qlabels = np.asarray(pred), np.asarray(qlabels)
    lab = qlabels >= 0
    hit = (pred == qlabels[:, None]) & lab[:, None]
    per = np.zeros((C, 2), dtype=np.int64)
    np.add.at(per[:, 0], qlabels[lab], 1)
    np.add.at(per[:, 1], qlabels[lab & (pred[:, 0] == qlabels)], 1)
    return np.cumsum(hit.sum(axis=0)).astype(np.int64), per, int(lab.sum())


# ---- the fit on hard labels ------------------------------------------------------------------------------------------------------------------
def optimum64_lbfgs(x, y, l2):
    """The float64 model's optimum by float64 L-BFGS to ||g||_inf <= OPTIMUM_GTOL (the exact Hessian of 300 x 73 parameters is out of reach)."""
    C, Da = y.shape[1], x.shape[1] + 1
    w, _, _, state = R.lbfgs(lambda v: (lambda o: (o["loss"], o["grad"]))(R.objective64(x, y, v, l2)), np.zeros((C, Da)), OPTIMUM_GTOL, 5000)
    assert state == "converged", state
    return w


@functools.lru_cache(maxsize=None)
def fit_world(spec, l2):
    """The world `spec` with y the one-hot of cls: the restated fit (fp32 forward), the float64 optimum, the validation rows the fit test may
    judge; asserts the cap (linprobe_refs.VAL_CAP) for the restated fit."""
    w = dict(R.world(spec))
    w["y"] = one_hot(w["cls"], w["C"])
    Wb, _, n_iter, state = R.fit_fp32_forward(w["x"], w["y"], l2=l2, gtol=FIT_GTOL)
    w.update(restated=Wb, restated_state=state, restated_iters=n_iter, optimum=optimum64_lbfgs(w["x"], w["y"], l2), l2=l2)
    zv = R.logits64(w["xv"], w["optimum"])
    w["val_margin"], w["val_argmax"] = R.top2_margin(zv), zv.argmax(axis=1)
    w["restated_left_out"] = R.assert_cap(w["val_margin"], R.margin_threshold(w["x"], w["y"], Wb, l2), spec)
    return w
