"""The linear probe of include/hbird_hip_linprobe.h restated in plain numpy, and the worlds the tests run it on.  No engine code.

  partition(ntotal)             the segment rule: (seg_rows, nseg)
  chain_logits(x, Wb)           z fp32: oracle.knn_chain_f32 on the augmented vectors [1, x] . [b, w] (the chain starts at fma(1, b, 0) = b);
                                a row with a non-finite component: all zeros, skipped
  objective(z, x, y, Wb, l2, skipped)  float64 from GIVEN logits: loss, gradient, residuals R, probabilities p, row losses l
  segment_gradient(R, x, skipped, Wb, l2)  the engine's gradient order given residuals: per segment an fp32 fmaf chain over ascending rows from
                                0, the partials added in float64 in ascending segment order, / n, + l2 Wb
  chunks(ntotal, workspace_segs), chunked_sums(...)  the host loop over workspace chunks, and the float64 sums as that loop walks them (with
                                two wrong variants for tests/test_bank_task_seams_cpu.py)
  lbfgs(fun, x0, gtol, max_iter)  the fit's loop restated; fit_fp32_forward: that loop on an fp32 forward; optimum64: the float64 optimum

The pieces reach each other through the module's names (row_mass, used_rows, regulariser, add_segments, chain_logits), so a test can swap one for
a wrong variant.

Bounds of tests/test_linprobe_gpu.py (test 2), measured on one MI355X over the committed worlds (profiles/r29/README.md): the largest relative
error of p behind a residual and of the data loss against float64 numpy from the device's logits; the tests hold 4 x these (the device's exp
and log may move with the ROCm version).
"""
import functools

import numpy as np

import oracle

MEASURED_P_REL = 2.78e-6   # (151, 16, 600) at parameters of scale 4; the four committed worlds alone: 2.76e-6
MEASURED_L_REL = 1.61e-8   # (151, 16, 600) at parameters of scale 1; the four committed worlds alone: 1.44e-8
BOUND_P_REL, BOUND_L_REL = 4 * MEASURED_P_REL, 4 * MEASURED_L_REL

MAX_SEGS = 512
LBFGS_MEMORY, ARMIJO_C1, MAX_HALVINGS, CURVATURE_EPS = 10, 1e-4, 30, 1e-10
FIT_L2, FIT_GTOL = 1e-2, 1e-5
VAL_CAP = 0.02             # at most this share of a world's validation rows may lie under the margin threshold


def partition(ntotal):
    t = -(-ntotal // 256)
    seg_rows = 256 * max(1, -(-t // MAX_SEGS))
    return seg_rows, -(-ntotal // seg_rows)


def skipped_rows(x):
    return ~np.isfinite(np.asarray(x, dtype=np.float32)).all(axis=1)


def chain_logits(x, Wb):
    """-> (z float32 [rows, C], skipped bool [rows])."""
    x, Wb = np.asarray(x, dtype=np.float32), np.asarray(Wb, dtype=np.float32)
    skip = skipped_rows(x)
    aug = np.concatenate([np.ones((x.shape[0], 1), dtype=np.float32), np.where(skip[:, None], np.float32(0), x)], axis=1)
    C = Wb.shape[0]
    idx, score = oracle.knn_chain_f32(aug, Wb, C)
    z = np.empty((x.shape[0], C), dtype=np.float32)
    np.put_along_axis(z, idx, score, axis=1)
    z[skip] = 0.0
    return z, skip


def row_mass(y):
    return y.sum(axis=1)


def used_rows(skipped):
    return int((~skipped).sum())


def regulariser(Wb, l2):
    """-> (value, gradient): (l2 / 2) sum Wb^2 over weights AND bias."""
    Wb = np.asarray(Wb, dtype=np.float64)
    return 0.5 * l2 * float((Wb * Wb).sum()), l2 * Wb


def add_segments(partials):
    total = np.zeros_like(partials[0], dtype=np.float64)
    for p in partials:                                   # ascending segments
        total = total + p.astype(np.float64)
    return total


def objective(z, x, y, Wb, l2, skipped=None):
    """float64 throughout, from the logits z -> dict(loss, grad [C, D + 1], R, p, l, data (the loss without its l2 term), n)."""
    z, y = np.asarray(z).astype(np.float64), np.asarray(y).astype(np.float64)
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    skipped = skipped_rows(x) if skipped is None else skipped
    keep = ~skipped
    s = row_mass(y)
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    p = np.exp(z - lse[:, None])
    l = np.where(keep, s * lse - (y * z).sum(axis=1), 0.0)
    R = np.where(keep[:, None], s[:, None] * p - y, 0.0)
    n = used_rows(skipped)
    aug = np.concatenate([np.ones((x64.shape[0], 1)), np.where(keep[:, None], x64, 0.0)], axis=1)
    reg, reg_grad = regulariser(Wb, l2)
    data = float(l.sum()) / n
    return dict(loss=data + reg, grad=R.T @ aug / n + reg_grad, R=R, p=p, l=l, data=data, n=n)


def logits64(x, Wb):
    x64 = np.where(skipped_rows(x)[:, None], 0.0, np.asarray(x, dtype=np.float32).astype(np.float64))
    Wb = np.asarray(Wb, dtype=np.float64)
    return x64 @ Wb[:, 1:].T + Wb[:, 0]


def objective64(x, y, Wb, l2):
    """The float64 model: float64 logits into `objective`."""
    return objective(logits64(x, Wb), x, y, Wb, l2)


def _fma32(a, b, c):
    """fp32 fma on arrays: the float64 product of two fp32 values is exact; one float64 add, then the rounding to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def segment_partials_by_rows(R, x, skipped):
    """[nseg] arrays float32 [C, D + 1]: per segment the fmaf chain over ascending rows of R[r][c] * [1, x[r]][j], started at 0."""
    R, x = np.asarray(R, dtype=np.float32), np.asarray(x, dtype=np.float32)
    aug = np.concatenate([np.ones((x.shape[0], 1), dtype=np.float32), x], axis=1)
    aug[skipped] = 0.0
    seg_rows, nseg = partition(x.shape[0])
    out = []
    for j in range(nseg):
        acc = np.zeros((R.shape[1], aug.shape[1]), dtype=np.float32)
        for r in range(j * seg_rows, min(x.shape[0], (j + 1) * seg_rows)):
            acc = _fma32(R[r][:, None], aug[r][None, :], acc)
        out.append(acc)
    return out


def segment_partials(R, x, skipped):
    """segment_partials_by_rows with all segments advancing together: step i takes row j * seg_rows + i of every segment j (the same fma on
    the same operands in the same order per segment; rows past the end are the exact zeros that the engine's padding rows are).
    tests/test_linprobe_cpu.py holds the two forms to each other on bits."""
    R, x = np.asarray(R, dtype=np.float32), np.asarray(x, dtype=np.float32)
    aug = np.concatenate([np.ones((x.shape[0], 1), dtype=np.float32), x], axis=1)
    aug[skipped] = 0.0
    seg_rows, nseg = partition(x.shape[0])
    pad = nseg * seg_rows - x.shape[0]
    Rp = np.concatenate([R, np.zeros((pad, R.shape[1]), dtype=np.float32)]).reshape(nseg, seg_rows, R.shape[1])
    Ap = np.concatenate([aug, np.zeros((pad, aug.shape[1]), dtype=np.float32)]).reshape(nseg, seg_rows, aug.shape[1])
    acc = np.zeros((nseg, R.shape[1], aug.shape[1]), dtype=np.float32)
    for i in range(seg_rows):
        acc = _fma32(Rp[:, i, :, None], Ap[:, i, None, :], acc)
    return list(acc)


def segment_gradient(R, x, skipped, Wb, l2):
    return add_segments(segment_partials(R, x, skipped)) / used_rows(skipped) + regulariser(Wb, l2)[1]


def chunks(ntotal, workspace_segs):
    """The host loop of hb_linprobe_loss_grad: [(row0, rows, segments)] of every workspace chunk when the workspace holds `workspace_segs`
    segments (None: all of them); a chunk is at least one segment."""
    seg_rows, nseg = partition(ntotal)
    per = nseg if workspace_segs is None else min(nseg, max(1, workspace_segs))
    out = []
    for seg0 in range(0, nseg, per):
        segs, row0 = min(per, nseg - seg0), seg0 * seg_rows
        out.append((row0, min(ntotal, row0 + segs * seg_rows) - row0, segs))
    return out


def chunked_sums(R, x, skipped, workspace_segs=None, staged_from_row_0=False, segment_cut=None):
    """sum_r R[r][c] [1, x[r]][j] in float64 as the host loop walks it: chunk by chunk, segment by segment, residuals and staged rows by their
    chunk-local index.  The two switches are WRONG variants for tests/test_bank_task_seams_cpu.py: a chunk whose staged rows restart at bank
    row 0, and a segment whose row loop ends after `segment_cut` rows."""
    R64, x64 = np.asarray(R).astype(np.float64), np.asarray(x, dtype=np.float32).astype(np.float64)
    aug = np.concatenate([np.ones((x64.shape[0], 1)), np.where(skipped[:, None], 0.0, x64)], axis=1)
    seg_rows = partition(x64.shape[0])[0]
    total = np.zeros((R64.shape[1], aug.shape[1]))
    for row0, rows, segs in chunks(x64.shape[0], workspace_segs):
        x0 = 0 if staged_from_row_0 else row0
        for j in range(segs):
            a, b = j * seg_rows, min(rows, j * seg_rows + (seg_rows if segment_cut is None else min(seg_rows, segment_cut)))
            total += R64[row0 + a:row0 + b].T @ aug[x0 + a:x0 + b]
    return total


def gradient_bound(R, x, skipped):
    """Per entry gamma_n sum |R x| / n, gamma_n = n_seg u / (1 - n_seg u), u = 2^-24, n_seg the segment length: an fma chain's textbook bound."""
    R64, x64 = np.abs(np.asarray(R).astype(np.float64)), np.asarray(x, dtype=np.float32).astype(np.float64)
    aug = np.abs(np.concatenate([np.ones((x64.shape[0], 1)), np.where(skipped[:, None], 0.0, x64)], axis=1))
    seg_rows = min(partition(x64.shape[0])[0], x64.shape[0])
    nu = seg_rows * 2.0 ** -24
    return nu / (1 - nu) * (R64.T @ aug) / used_rows(skipped)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------
def lbfgs(fun, x0, gtol, max_iter):
    """-> (x, history [(loss, ||g||_inf)], n_iter, state)."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    history, S, Y, n_iter = [(float(f), float(np.abs(g).max()))], [], [], 0
    while True:
        if np.abs(g).max() <= gtol:
            return x, history, n_iter, "converged"
        if n_iter >= max_iter:
            return x, history, n_iter, "max_iter"
        q, alphas = g.copy(), []
        for s, y in zip(reversed(S), reversed(Y)):
            a = float(np.vdot(s, q)) / float(np.vdot(y, s))
            alphas.append(a)
            q -= a * y
        if S:
            q *= float(np.vdot(S[-1], Y[-1])) / float(np.vdot(Y[-1], Y[-1]))
        for (s, y), a in zip(zip(S, Y), reversed(alphas)):
            q += (a - float(np.vdot(y, q)) / float(np.vdot(y, s))) * s
        d = -q
        gd = float(np.vdot(g, d))
        if not gd < 0:
            d, S, Y = -g, [], []
            gd = float(np.vdot(g, d))
        t = 1.0 / float(np.linalg.norm(g)) if n_iter == 0 else 1.0
        for _ in range(MAX_HALVINGS + 1):
            xn = x + t * d
            fn, gn = fun(xn)
            if fn <= f + ARMIJO_C1 * t * gd:
                break
            t *= 0.5
        else:
            return x, history, n_iter, "stalled"
        s, y = xn - x, gn - g
        if float(np.vdot(y, s)) > CURVATURE_EPS * float(np.linalg.norm(y)) * float(np.linalg.norm(s)):
            S.append(s); Y.append(y)
            S, Y = S[-LBFGS_MEMORY:], Y[-LBFGS_MEMORY:]
        x, f, g = xn, fn, gn
        n_iter += 1
        history.append((float(f), float(np.abs(g).max())))


def fit_fp32_forward(x, y, l2=FIT_L2, gtol=FIT_GTOL, max_iter=200):
    """The engine's fit with a numpy fp32 forward: every evaluation rounds Wb to fp32 and takes fp32 logits."""
    x = np.asarray(x, dtype=np.float32)

    def fun(w):
        Wb = w.astype(np.float32)
        z = x @ Wb[:, 1:].T + Wb[:, 0]
        o = objective(z, x, y, Wb, l2)
        return o["loss"], o["grad"]

    w, history, n_iter, state = lbfgs(fun, np.zeros((y.shape[1], x.shape[1] + 1)), gtol, max_iter)
    return w.astype(np.float32), history, n_iter, state


def optimum64(x, y, l2=FIT_L2):
    """The float64 model's optimum, ||g||_inf <= 1e-11: L-BFGS, then Newton steps on the exact Hessian."""
    C, Da = y.shape[1], x.shape[1] + 1
    w = lbfgs(lambda v: (lambda o: (o["loss"], o["grad"]))(objective64(x, y, v, l2)), np.zeros((C, Da)), 1e-7, 500)[0]
    aug = np.concatenate([np.ones((x.shape[0], 1)), np.asarray(x, dtype=np.float32).astype(np.float64)], axis=1)
    for _ in range(8):
        o = objective64(x, y, w, l2)
        if np.abs(o["grad"]).max() <= 1e-12:
            break
        s, p = row_mass(np.asarray(y, dtype=np.float64)), o["p"]
        H = np.zeros((C, Da, C, Da))
        for c in range(C):
            for c2 in range(c, C):
                wgt = s * ((p[:, c] if c == c2 else 0.0) - p[:, c] * p[:, c2]) / o["n"]
                blk = (aug * wgt[:, None]).T @ aug
                H[c, :, c2, :] = blk
                H[c2, :, c, :] = blk.T
        H = H.reshape(C * Da, C * Da) + l2 * np.eye(C * Da)
        w = w - np.linalg.solve(H, o["grad"].reshape(-1)).reshape(C, Da)
    assert np.abs(objective64(x, y, w, l2)["grad"]).max() <= 1e-11
    return w


def top2_margin(z):
    part = np.partition(np.asarray(z, dtype=np.float64), -2, axis=1)      # (two classes at the least)
    return part[:, -1] - part[:, -2]


def margin_threshold(x, y, Wb, l2=FIT_L2):
    """thr = 2 sqrt(2) ||g64(Wb)||_2 / l2: L is l2-strongly convex, so ||Wb - W*|| <= ||g|| / l2, and ||[1, x]|| = sqrt(2) on unit rows; a logit
    moves by at most sqrt(2) ||Wb - W*||, a margin by twice that."""
    return 2.0 * np.sqrt(2.0) * float(np.linalg.norm(objective64(x, y, Wb, l2)["grad"])) / l2


# ---- worlds ------------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = v.astype(np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def draw_world(C, D, rows, n_val, seed, sigma, P=16):
    """-> dict(x float32 [rows, D] unit rows, counts int64 [rows, C] of denominator P, y float32 = counts / P, cls, xv float32 [n_val, D], P)."""
    g = np.random.default_rng(seed)
    centres = _unit(g.standard_normal((C, D)))
    cls = g.integers(0, C, rows)
    x = _unit(centres[cls].astype(np.float64) + sigma * g.standard_normal((rows, D)))
    j2, other = g.integers(0, P // 2 + 1, rows), g.integers(0, C, rows)
    counts = np.zeros((rows, C), dtype=np.int64)
    np.add.at(counts, (np.arange(rows), cls), P - j2)
    np.add.at(counts, (np.arange(rows), other), j2)
    cls_v = g.integers(0, C, n_val)
    xv = _unit(centres[cls_v].astype(np.float64) + sigma * g.standard_normal((n_val, D)))
    y = (counts.astype(np.float32) / np.float32(P)).astype(np.float32)
    return dict(x=x, counts=counts, y=y, cls=cls, xv=xv, P=P, C=C, D=D)


# (C, D, rows, n_val, seed, sigma): D not a multiple of 16 (72 -> 80), C on both sides of 32, rows no multiple of 32 or 256
WORLDS = [(3, 16, 600, 1024, 21, 0.3), (33, 16, 4000, 1024, 22, 0.2), (3, 72, 4000, 1024, 23, 0.15), (21, 72, 2000, 1024, 24, 0.12)]
WIDE_WORLD = (151, 16, 600, 64, 25, 0.2)          # P = 196: count rows of stride 152
SEGMENT_WORLD = (3, 16, 513, 64, 26, 0.3)         # three segments, the last one of one row: the smallest row count with three

# The bank-size seams.  BIG_ROWS = 131,195 = 4,099 row tiles of 32 and 27 rows = 512 blocks of 256 and 123 rows:
#   linear probe (partition): t = ceil(131,195 / 256) = 513 > MAX_SEGS, so seg_rows = 256 * ceil(513 / 512) = 512 and nseg = ceil(131,195 / 512) = 257,
#     the last segment of 131,195 - 256 * 512 = 123 rows; the loss tree has rows with j = 1 (r >= 65,536) and, for r >= 131,072, j = 2
#   k-means (km_segments of tests/kmeans_refs.py): nt = 4,100 row tiles, segs = min(128, ceil(4,100 / 16)) = 128, seg_tiles = ceil(4,100 / 128) = 33:
#     124 full segments (4,092 tiles), one of 8 tiles and three empty ones; 33 tiles are two trips of 32 with all four slots live
# (tests/test_linprobe_cpu.py and tests/test_kmeans_cpu.py assert this arithmetic.)
BIG_ROWS = 131195
BIG_HOLE = 100003                                  # the one non-finite row of a big world: past row 65,536 (tree index j = 1)
BIG_WORLD = (3, 16, BIG_ROWS, 64, 27, 0.3)

# Class tiles: CT = ceil(C / 32) from 1 to 8 at both ends of every tile (C = 32 CT: the `t * 32 + i < C` masks stop masking; C = 32 CT + 1:
# one live class in the last tile), on 300 rows (nine row tiles and 12 rows, two forward workgroups, two segments); (256, 72): width padded to
# 80, g8 = 10, two LDS staging rounds of the largest Wb; (225, 384): a wide bank.  Count rows (P = 16) have their stride padded to 8.
TILE_ROWS = 300
TILE_WORLDS = [(C, 16, TILE_ROWS, 8, 40 + i, 0.2) for i, C in enumerate((32, 64, 65, 96, 97, 128, 160, 161, 192, 193, 224, 225, 256, 129))] + [
    (256, 72, TILE_ROWS, 8, 60, 0.15), (225, 384, TILE_ROWS, 8, 61, 0.1)]      # (C = 33, the low end of two tiles, is in WORLDS)

# Residuals and loss on TILE_WORLDS and BIG_WORLD (C up to 256), measured as MEASURED_P_REL and MEASURED_L_REL were (profiles/r34/README.md):
MEASURED_P_REL_WIDE = 2.98e-6   # (224, 16, 300) at parameters of scale 4
MEASURED_L_REL_WIDE = 1.98e-8   # (225, 384, 300) at parameters of scale 1
BOUND_P_REL_WIDE, BOUND_L_REL_WIDE = 4 * MEASURED_P_REL_WIDE, 4 * MEASURED_L_REL_WIDE


@functools.lru_cache(maxsize=None)
def world(spec, P=16):
    return draw_world(*spec, P=P)


@functools.lru_cache(maxsize=None)
def big_world():
    """BIG_WORLD with its one non-finite row, BIG_HOLE."""
    w = dict(world(BIG_WORLD))
    w["x"] = w["x"].copy()
    w["x"][BIG_HOLE, 5] = np.nan
    return w


@functools.lru_cache(maxsize=None)
def fit_world(spec):
    """A committed world with the restated fit, the float64 optimum and the validation rows the fit test may judge; asserts the cap."""
    w = dict(world(spec))
    Wb, history, n_iter, state = fit_fp32_forward(w["x"], w["y"])
    w.update(restated=Wb, restated_state=state, restated_iters=n_iter, optimum=optimum64(w["x"], w["y"]))
    w["val_margin"] = top2_margin(logits64(w["xv"], w["optimum"]))
    w["val_argmax"] = logits64(w["xv"], w["optimum"]).argmax(axis=1)
    thr = margin_threshold(w["x"], w["y"], Wb)
    w["restated_left_out"] = assert_cap(w["val_margin"], thr, spec)
    return w


def assert_cap(margins, thr, spec=None):
    """The worlds' own condition: at most VAL_CAP of the validation rows have a float64 top-2 margin under thr.  -> the share that has."""
    left_out = float((np.asarray(margins) <= thr).mean())
    assert left_out <= VAL_CAP, (spec, left_out)
    return left_out


def integer_world(C, D, rows, seed):
    """Entries in {-2 .. 2} / 2 for rows, weights and biases: every product and partial sum is exact in fp32, float64 logits are the answer."""
    g = np.random.default_rng(seed)
    return (g.integers(-2, 3, (rows, D)) / 2.0).astype(np.float32), (g.integers(-2, 3, (C, D + 1)) / 2.0).astype(np.float32)
