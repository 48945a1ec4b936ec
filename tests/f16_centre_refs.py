"""Definitions of what the CONVERSION behind the centred fp16 screen leaves (csrc/hbird_f16_centre.hip; read out by
HipFlatIndex.last_centre() / hb_index_last_centre), in plain numpy.  Nothing here knows of partitions, waves, shuffle trees or atomics; the
one tile-aware helper is `detile16`, which undoes the layout that include/hbird_hip_centre.h states for the two raw fp16 arrays.

Apart from mu and t every quantity is defined as a function of the PREVIOUS stage's read-out value (mu.mu and ||mu|| from the device's mu,
the differences and g from the device's mu, init16 from the device's t and g, ...), so each kernel is held to bits on its own and one ulp
upstream does not smear downstream.

    valid rows   real (row < ntotal) and every component finite
    mu           float64 column mean over the valid rows -> fp32; 0 on [D, n_mu).  Exact worlds (small integers x 2^-5 [+ a common integer]:
                 every float64 partial sum in any order is exact): bits.  Float worlds: |mu - ref| <= ulp32(ref) + N 2^-52 mean|b[:, k]|
                 (the float64 summation bound -- N - 1 additions, each within 2^-53 of the running sum of absolute values -- and one rounding)
    mu.mu        float64 k-ascending sum of the exact products of the device's mu -> fp32;  ||mu|| = sqrt of that sum, rounded UP to fp32
    d            fl32(b - mu); its fp16 image np.float16(d): round to nearest even, subnormals kept; columns >= D are zero
    g            the chain g = fmaf(mu_k, d_k, g), k ascending, with bank_refs.fma_f32 (correctly rounded: NOT a float64 multiply-add and a cast)
    cmax         max over the real rows of roundup32(sqrt(sum_k d_k^2)) (float64, k ascending); a NaN row counts for nothing, an infinite one
                 gives +inf; over EVERY row converted since mu was derived
    c_q          the chain c = fmaf(q_k, mu_k, c), k ascending
    t            fsum(finite c_q) / (nq mu.mu) -> fp32, nq counting ALL queries.  |t - ref| <= ulp32(ref) + 2^-52 sum|c_q| / mu.mu; exact worlds: bits
    q - t mu     from the device's t: fma_f32(-t, mu_k, q_k), its fp16 image, ||.|| rounded up; the padding queries up to 256 are zero vectors
    init16       fma_f32(t, g, binit) on real rows (binit: 0 for inner product, -|b|^2 / 2 by oracle.chain_sqnorm for L2; a row whose binit is
                 -inf keeps -inf); -inf on every row from ntotal to the next multiple of 256

`check_conversion` / `check_queries` return {assertion name: message}, EMPTY when the read-out is right; the GPU file and the host model of
tests/test_f16_centre_readout_cpu.py share them."""
from __future__ import annotations

import collections
import functools
import math

import numpy as np

import bank_refs
import oracle

F32 = np.float32
PARTS = 128          # row-tile partitions of the column sums (the case-list guard restates the launch arithmetic from it)

CONVERSION_NAMES = ("rows", "mu", "mu_padding", "mu2", "mu_norm", "tiles", "tile_padding", "g", "cmax", "init16", "init16_padding")
QUERY_NAMES = ("n", "cq", "t", "q_tiles", "q_padding", "qcn")
SCENARIO_NAMES = ("level", "deterministic")      # what the scenario runners add: the pass a read-out belongs to; equal bits from two builds


# ---- primitives --------------------------------------------------------------------------------------------------------------------------------
def roundup32(x64) -> np.ndarray:
    """The smallest fp32 number >= x (float64 in; NaN stays NaN)."""
    x64 = np.asarray(x64, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = x64.astype(F32)
        low = f.astype(np.float64) < x64
        return np.where(low, np.nextafter(f, F32(np.inf)), f).astype(F32)


def ulp32(x) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def same_bits(a, b) -> np.ndarray:
    """Elementwise: the same bits, or both NaN (a NaN's payload is no part of any definition here)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    eq = a.view(u) == b.view(u)
    if a.dtype.kind == "f":
        eq = eq | (np.isnan(a) & np.isnan(b))
    return eq


def f16_bits(x32) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x32, dtype=F32).astype(np.float16).view(np.uint16)


def _f16_same(got_u16, want_u16) -> np.ndarray:
    return same_bits(got_u16.view(np.float16), want_u16.view(np.float16))


def sqsum64(d32) -> np.ndarray:
    """float64 k-ascending sum of d_k^2 per row (the squares of fp32 numbers are exact in float64)."""
    d = np.asarray(d32, dtype=F32).astype(np.float64)
    s = np.zeros(d.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(d.shape[1]):
            s = s + d[:, k] * d[:, k]
    return s


def chain_dot(a, b) -> np.ndarray:
    """c = fmaf(a_k, b_k, c), k ascending, per row of a [n, D] against b [D] or [n, D]."""
    a = np.asarray(a, dtype=F32)
    b = np.broadcast_to(np.asarray(b, dtype=F32), a.shape)
    c = np.zeros(a.shape[0], dtype=F32)
    for k in range(a.shape[1]):
        c = bank_refs.fma_f32(a[:, k], b[:, k], c)
    return c


def detile16(raw, n_rows, dp16) -> np.ndarray:
    """raw uint16 [n_rows * dp16] in the tile layout of include/hbird_hip_centre.h -> uint16 [n_rows, dp16] (n_rows a multiple of 32)."""
    assert n_rows % 32 == 0 and dp16 % 8 == 0 and raw.size == n_rows * dp16
    return np.ascontiguousarray(raw.reshape(n_rows // 32, dp16 // 8, 32, 8).transpose(0, 2, 1, 3).reshape(n_rows, dp16))


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------------
def valid_rows(bank) -> np.ndarray:
    return np.isfinite(np.asarray(bank, dtype=F32)).all(axis=1)


def mean_ref(bank):
    """-> (mu fp32 [D], tolerance float64 [D] of a float world) over the valid rows of bank."""
    b = np.asarray(bank, dtype=F32)[valid_rows(bank)].astype(np.float64)
    n = b.shape[0]
    if n == 0:
        return np.zeros(bank.shape[1], F32), np.zeros(bank.shape[1])
    mu = (b.sum(axis=0) / n).astype(F32)
    return mu, ulp32(mu) + n * 2.0 ** -52 * np.abs(b).mean(axis=0)


def mu_scalars(mu):
    """(mu.mu fp32, ||mu|| fp32 rounded up) of an fp32 vector."""
    m2 = 0.0
    for v in np.asarray(mu, dtype=F32).astype(np.float64):
        m2 = m2 + v * v
    return F32(m2), roundup32(math.sqrt(m2))[()]


def differences(x, mu) -> np.ndarray:
    """fl32(x - mu) on the D columns of x."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x - np.asarray(mu, dtype=F32)[None, :x.shape[1]]).astype(F32)


def row_norms_up(d32) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return roundup32(np.sqrt(sqsum64(d32)))


def cmax_ref(d32) -> np.float32:
    cn = row_norms_up(d32)
    cn = np.where(np.isnan(cn), F32(0.0), cn)
    return F32(cn.max()) if cn.size else F32(0.0)


def binit_ref(bank, metric) -> np.ndarray:
    bank = np.asarray(bank, dtype=F32)
    if metric != 1:
        return np.zeros(bank.shape[0], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(-0.5) * oracle.chain_sqnorm(np.ascontiguousarray(bank))).astype(F32)


def init16_ref(t, g, binit) -> np.ndarray:
    v = bank_refs.fma_f32(np.broadcast_to(F32(t), g.shape), g, binit)
    return np.where(np.isneginf(binit), F32(-np.inf), v).astype(F32)


def t_ref(cq, nq, mu2):
    """-> (t fp32, tolerance float64)"""
    cq = np.asarray(cq, dtype=F32).astype(np.float64)
    fin = cq[np.isfinite(cq)]
    m2 = float(F32(mu2))
    if not m2 > 0.0:
        return F32(0.0), 0.0
    t = F32(math.fsum(fin) / (float(nq) * m2))
    if not np.isfinite(t):
        return F32(0.0), 0.0
    return t, float(ulp32(t)) + 2.0 ** -52 * float(np.abs(fin).sum()) / m2


def centred_queries(q, mu, t) -> np.ndarray:
    """fma_f32(-t, mu_k, q_k) per component."""
    q = np.asarray(q, dtype=F32)
    nt = np.broadcast_to(F32(-F32(t)), q.shape)
    return bank_refs.fma_f32(nt, np.broadcast_to(np.asarray(mu, dtype=F32)[None, :q.shape[1]], q.shape), q)


# ---- the assertions ----------------------------------------------------------------------------------------------------------------------------
def _first(mask):
    return tuple(int(v[0]) for v in np.nonzero(mask))


def check_conversion(readout, bank, metric, mean_rows=None, exact=False, what=""):
    """The bank side of a read-out against the definitions -> {name: message}.  bank: every row converted since mu was derived (fp32 [rows, D],
    as stored); mean_rows: the leading rows mu was derived from (default: all of them).  Names: CONVERSION_NAMES."""
    bank = np.ascontiguousarray(bank, dtype=F32)
    N, D = bank.shape
    R = readout
    bad = {}

    def note(name, msg):
        bad.setdefault(name, f"{what}{name}: {msg}")
    dp16, n_mu = R["dp16"], R["n_mu"]
    if R["rows"] != N or dp16 != (D + 127) // 128 * 128 or n_mu < dp16 or R["g"].size != (N + 31) // 32 * 32 or R["init16"].size != (N + 255) // 256 * 256 \
            or R["bank16"].size != R["g"].size * dp16 or R["mu"].size != n_mu:
        note("rows", f"rows {R['rows']} dp16 {dp16} n_mu {n_mu} g {R['g'].size} init16 {R['init16'].size} bank16 {R['bank16'].size} for a bank of {N} x {D}")
        return bad
    mu = R["mu"]
    # mu
    ref_mu, tol = mean_ref(bank[:N if mean_rows is None else mean_rows])
    if exact:
        ok = same_bits(mu[:D], ref_mu)
    else:
        ok = np.abs(mu[:D].astype(np.float64) - ref_mu.astype(np.float64)) <= tol
    if not ok.all():
        k = _first(~ok)[0]
        note("mu", f"column {k}: {mu[k]!r}, the float64 mean of the valid rows is {ref_mu[k]!r} ({'bits' if exact else f'tolerance {tol[k]:.3g}'})")
    if (mu[D:].view(np.uint32) != 0).any():
        note("mu_padding", f"mu is not +0 on the padding dimension {D + _first(mu[D:].view(np.uint32) != 0)[0]}")
    # mu.mu, ||mu|| from the device's mu
    m2, mun = mu_scalars(mu)
    if not same_bits(np.array([R["mu2"]], F32), np.array([m2], F32)).all():
        note("mu2", f"mu.mu {R['mu2']!r}, from the read-out mu {m2!r}")
    if not same_bits(np.array([R["mu_norm"]], F32), np.array([mun], F32)).all():
        note("mu_norm", f"||mu|| {R['mu_norm']!r}, the read-out mu's norm rounded up is {mun!r}")
    # d and its fp16 image
    d = differences(bank, mu)
    got16 = detile16(R["bank16"], R["g"].size, dp16)[:N]
    okt = _f16_same(got16[:, :D], f16_bits(d))
    if not okt.all():
        r, k = _first(~okt)
        note("tiles", f"row {r} (row tile {r // 32}) component {k}: fp16 bits {got16[r, k]:#06x}, np.float16(fl32(b - mu)) has {f16_bits(d)[r, k]:#06x}")
    if (got16[:, D:] != 0).any():
        r, k = _first(got16[:, D:] != 0)
        note("tile_padding", f"row {r}: the padding component {D + k} holds {got16[r, D + k]:#06x}")
    # g
    g = chain_dot(d, mu[:D])
    okg = same_bits(R["g"][:N], g)
    if not okg.all():
        r = _first(~okg)[0]
        note("g", f"row {r} (row tile {r // 32}): {R['g'][r]!r}, the fmaf chain over fl32(b - mu) gives {g[r]!r}")
    # cmax
    cm = cmax_ref(d)
    if not same_bits(np.array([R["cmax"]], F32), np.array([cm], F32)).all():
        note("cmax", f"{R['cmax']!r}, the maximum over the {N} converted rows (rounded up) is {cm!r}")
    # init16 from the device's t and g
    want = init16_ref(R["t"], R["g"][:N], binit_ref(bank, metric))
    oki = same_bits(R["init16"][:N], want)
    if not oki.all():
        r = _first(~oki)[0]
        note("init16", f"row {r}: {R['init16'][r]!r}, fmaf(t = {R['t']!r}, g, binit) = {want[r]!r}")
    if not np.isneginf(R["init16"][N:]).all():
        note("init16_padding", f"row {N + _first(~np.isneginf(R['init16'][N:]))[0]} beyond the bank's {N} rows is not -inf")
    return bad


def check_queries(readout, queries, nq_all=None, exact=False, derive_t=True, what=""):
    """The query side of a read-out -> {name: message}.  queries: the fp32 queries of the pass the read-out belongs to.  derive_t=False (the
    second pass, which keeps the caller's t): t is taken as it is.  nq_all: the count in t's denominator (default: every query).  Names:
    QUERY_NAMES."""
    q = np.ascontiguousarray(queries, dtype=F32)
    nq, D = q.shape
    R = readout
    bad = {}

    def note(name, msg):
        bad.setdefault(name, f"{what}{name}: {msg}")
    dp16 = R["dp16"]
    nqp = (nq + 255) // 256 * 256
    if R["n"] != nq or R["cq"].size != nq or R["qcn"].size != nq or R["q16"].size != nqp * dp16:
        note("n", f"n {R['n']} cq {R['cq'].size} qcn {R['qcn'].size} q16 {R['q16'].size} for {nq} queries")
        return bad
    mu = R["mu"]
    cq = chain_dot(q, mu[:D])
    okc = same_bits(R["cq"], cq)
    if not okc.all():
        i = _first(~okc)[0]
        note("cq", f"query {i}: {R['cq'][i]!r}, the fmaf chain q.mu gives {cq[i]!r}")
    if derive_t:
        t, tol = t_ref(R["cq"], nq if nq_all is None else nq_all, R["mu2"])
        ok = same_bits(np.array([R["t"]], F32), np.array([t], F32)).all() if exact else abs(float(R["t"]) - float(t)) <= tol
        if not ok:
            note("t", f"{R['t']!r}, sum of the finite c_q over (nq mu.mu) is {t!r} ({'bits' if exact else f'tolerance {tol:.3g}'})")
    dq = centred_queries(q, mu, R["t"])
    got16 = detile16(R["q16"], nqp, dp16)
    okt = _f16_same(got16[:nq, :D], f16_bits(dq))
    if not okt.all():
        i, k = _first(~okt)
        note("q_tiles", f"query {i} component {k}: fp16 bits {got16[i, k]:#06x}, np.float16(fmaf(-t, mu, q)) has {f16_bits(dq)[i, k]:#06x}")
    pad = got16.copy()
    pad[:nq, :D] = 0
    if (pad != 0).any():
        i, k = _first(pad != 0)
        note("q_padding", f"query row {i} component {k} (beyond {nq} queries x {D}) holds {got16[i, k]:#06x}")
    qcn = row_norms_up(dq)
    okn = same_bits(R["qcn"], qcn)
    if not okn.all():
        i = _first(~okn)[0]
        note("qcn", f"query {i}: ||q - t mu|| {R['qcn'][i]!r}, rounded up from the float64 sum {qcn[i]!r}")
    return bad


# ---- the worlds and the case list of tests/test_f16_centre_readout_gpu.py -----------------------------------------------------------------------
def float_world(N, D, nq, seed=0, q_shift=20.0):
    """Massive-activation-like: standard normal rows, three dimensions shifted by +40 (queries: by q_shift)."""
    rng = np.random.default_rng([seed, N, D, 7])
    bank = rng.standard_normal((N, D), dtype=F32)
    q = rng.standard_normal((nq, D), dtype=F32)
    dims = [1, D // 2, D - 2]
    bank[:, dims] += F32(40.0)
    q[:, dims] += F32(q_shift)
    return {"bank": bank, "queries": q, "exact": False}


def exact_world(N, D, nq, seed=0, offset=2, q_offset=1):
    """Integers in [-8, 8] x 2^-5 plus a common integer: every float64 partial sum of a column, in any order, is exact."""
    rng = np.random.default_rng([seed, N, D, 8])
    bank = (rng.integers(-8, 9, size=(N, D)).astype(F32) / F32(32.0) + F32(offset)).astype(F32)
    q = (rng.integers(-8, 9, size=(nq, D)).astype(F32) / F32(32.0) + F32(q_offset)).astype(F32)
    return {"bank": bank, "queries": q, "exact": True}


@functools.lru_cache(maxsize=None)
def world(kind, N, D, nq, seed=0):
    return float_world(N, D, nq, seed) if kind == "float" else exact_world(N, D, nq, seed)


Fresh = collections.namedtuple("Fresh", "N D metric kind nq")
K = 10                                # neighbours of every search of the read-out tests (k' = 64)
FRESH_SHAPES = ((1000, 40), (1000, 128), (5000, 136), (20000, 64))
FRESH_CASES = tuple(Fresh(N, D, m, kind, 70) for (N, D) in FRESH_SHAPES for kind in ("float", "exact")
                    for m in ((0, 1) if (N, D) in ((1000, 40), (5000, 136)) else ((0,) if kind == "float" else (1,))))
QUERY_SHAPES = (1, 70, 300)           # nq: one partial 64-block; two blocks, three row tiles; two 256-tiles, five 64-blocks
APPEND = {"reserve": 6000, "first": 3000, "more": 1500, "D": 64, "big_from": 1000, "big_scale": 8.0, "beyond": 2000, "after_reset": 1000}
TWO_SEARCHES = {"N": 5000, "D": 64, "nq": 70}
SECOND_PASS = {"N": 5000, "D": 64, "nq": 64, "k": 30, "clusters": 16, "cluster_rows": 80}
VIEW = {"N": 5000, "D": 136, "take": 2000}


def invalid_rows_world(seed=3):
    """1,000 x 40 with NaN rows in the first tile, in the last tile and as row 0; `bank_inf`: the same bank with row 600 finite but for one +inf
    component instead of NaN."""
    W = float_world(1000, 40, 70, seed)
    b = W["bank"].copy()
    b[[0, 5, 31, 500, 600, 993, 999]] = np.nan
    b[17, 3] = np.nan                   # one component is enough
    binf = b.copy()
    binf[600] = W["bank"][600]          # (the same valid rows as in `bank`: the same mean, bit for bit)
    binf[600, 7] = np.inf
    return {"bank": b, "bank_inf": binf, "queries": W["queries"], "exact": False}


def append_world(seed=4):
    a = APPEND
    W = float_world(a["reserve"] + a["beyond"] + a["after_reset"], a["D"], 70, seed)
    rows = W["bank"]
    first, more = rows[:a["first"]], rows[a["first"]:a["first"] + a["more"]].copy()
    more[a["big_from"]:] *= F32(a["big_scale"])
    beyond = rows[a["first"] + a["more"]:a["reserve"] + a["beyond"]]      # 3,500 rows: 8,000 in all, beyond the reservation of 6,000
    small = (rows[-a["after_reset"]:] * F32(0.25)).astype(F32)
    return {"first": first, "more": more, "beyond": beyond, "after_reset": small, "queries": W["queries"]}


def second_pass_world(seed=6):
    """Rows with three dimensions at +40.  A quarter of the queries each own a tight cluster of 80 > k' = 64 near-identical rows, reached through a
    dimension of their own that every other query and row leaves at zero: their k-th and k'-th neighbours lie closer than E' (no first
    certificate), and to every other query the cluster is one ordinary row repeated.  (By tests/test_f16_centre_cpu.centred_model no query of
    this world lies within 1.0 E' of its certificate's threshold: the failing set does not depend on an ulp.)"""
    s = SECOND_PASS
    rng = np.random.default_rng([seed, 9])
    N, D, nq, ncl, crow = s["N"], s["D"], s["nq"], s["clusters"], s["cluster_rows"]
    bank = rng.standard_normal((N, D), dtype=F32)
    q = rng.standard_normal((nq, D), dtype=F32)
    own = np.arange(2, 2 + ncl)
    bank[:, own] = 0
    q[:, own] = 0
    for c in range(ncl):
        lo = 100 + c * crow
        bank[lo:lo + crow] = bank[lo][None, :] + F32(1e-4) * rng.standard_normal((crow, D), dtype=F32)
        bank[lo:lo + crow, own] = 0
        bank[lo:lo + crow, own[c]] = F32(16.0)
        q[2 * c, own[c]] = F32(16.0)
    dims = [1, D // 2, D - 2]
    bank[:, dims] += F32(40.0)
    q[:, dims] += F32(20.0)
    return {"bank": bank, "queries": q, "exact": False, "owners": np.arange(0, 2 * ncl, 2)}


def zero_mean_world(N=1000, D=40, nq=16, seed=6):
    rng = np.random.default_rng([seed, 10])
    half = rng.integers(-8, 9, size=(N // 2, D)).astype(F32) / F32(32.0)
    bank = np.empty((N, D), F32)
    bank[0::2], bank[1::2] = half, -half
    return {"bank": bank, "queries": rng.standard_normal((nq, D), dtype=F32), "exact": True}


def launch_regime(N, D):
    """The launch arithmetic of the conversion, restated (hbird_f16_centre.hip, hb_index_create): what a bank of N x D reaches."""
    nrt = (N + 31) // 32
    per = (nrt + PARTS - 1) // PARTS
    used = (nrt + per - 1) // per
    g8 = (D + 15) // 16 * 16 // 8
    dp16 = (D + 127) // 128 * 128
    return {"row_tiles": nrt, "per": per, "empty_partitions": PARTS - used, "ragged_last_partition": nrt % per != 0, "g8": g8, "dp16": dp16,
            "zero_groups": dp16 // 8 - g8, "last_tile_rows": N - (nrt - 1) * 32, "tiles_mod_8": nrt % 8,
            "wave0_trips": (per + 3) // 4, "wave3_trips": max(0, (per - 3 + 3) // 4)}


# ---- the scenarios: one index-like object per run (the GPU file wraps HipFlatIndex, the CPU file its host model) --------------------------------
# make(D, metric) -> an object with reserve(n), add(rows), reset(), search(queries, k), set_escalation(on), certified() (the first certificates
# of the last search), last_centre(queries=True), select_rows(ids) and close().  Every runner returns {assertion name: message}.
def _merge(bad, more):
    for name, msg in more.items():
        bad.setdefault(name, msg)
    return bad


def _note(bad, name, msg):
    bad.setdefault(name, f"{name}: {msg}")


def run_fresh(make, c):
    W = world(c.kind, c.N, c.D, c.nq)
    ix = make(c.D, c.metric)
    ix.set_escalation(False)           # (no second pass: the caller's arrays stay)
    ix.add(W["bank"]); ix.search(W["queries"], K)
    R = ix.last_centre()
    bad = {}
    if R["level"] != 0:
        _note(bad, "level", f"{R['level']} after a caller's search")
    _merge(bad, check_conversion(R, W["bank"], c.metric, exact=W["exact"]))
    _merge(bad, check_queries(R, W["queries"], exact=W["exact"]))
    again = make(c.D, c.metric)                      # a second build of the same bank: equal bits
    again.set_escalation(False)
    again.add(W["bank"]); again.search(W["queries"], K)
    R2 = again.last_centre(queries=False)
    if not (same_bits(R["mu"], R2["mu"]).all() and same_bits(R["g"], R2["g"]).all() and R["cmax"].view(np.uint32) == R2["cmax"].view(np.uint32)):
        _note(bad, "deterministic", "two builds of the same bank differ in mu, g or cmax")
    ix.close(); again.close()
    return bad


def run_invalid_rows(make, metric):
    W = invalid_rows_world()
    bad = {}
    ix = make(40, metric)
    ix.set_escalation(False)
    ix.add(W["bank"]); ix.search(W["queries"], K)
    R = ix.last_centre()
    if not np.isfinite(R["cmax"]):
        _note(bad, "cmax", f"{R['cmax']!r} on a bank whose invalid rows are all NaN rows")
    _merge(bad, check_conversion(R, W["bank"], metric, what="NaN rows: "))
    _merge(bad, check_queries(R, W["queries"], what="NaN rows: "))
    jx = make(40, metric)
    jx.set_escalation(False)
    jx.add(W["bank_inf"]); jx.search(W["queries"], K)
    Ri = jx.last_centre()
    if not (np.isposinf(Ri["cmax"])):
        _note(bad, "cmax", f"{Ri['cmax']!r} with an infinite component in row 600: no certificate may pass")
    if not same_bits(Ri["mu"], R["mu"]).all():
        _note(bad, "mu", "the row with an infinite component has moved the mean")
    _merge(bad, check_conversion(Ri, W["bank_inf"], metric, what="+inf component: "))
    ix.close(); jx.close()
    return bad


def run_append_capacity_reset(make, metric):
    a, W = APPEND, append_world()
    q = W["queries"]
    bad = {}
    ix = make(a["D"], metric)
    ix.set_escalation(False)
    ix.reserve(a["reserve"]); ix.add(W["first"]); ix.search(q, K)
    R0 = ix.last_centre()
    _merge(bad, check_conversion(R0, W["first"], metric, what="first rows: "))
    ix.add(W["more"]); ix.search(q, K)
    R1 = ix.last_centre()
    both = np.concatenate([W["first"], W["more"]])
    if not same_bits(R1["mu"], R0["mu"]).all():
        _note(bad, "mu", "after the append mu is no longer the first rows' (the old rows' tiles were made with it)")
    _merge(bad, check_conversion(R1, both, metric, mean_rows=a["first"], what="after the append: "))
    _merge(bad, check_queries(R1, q, what="after the append: "))
    if not float(R1["cmax"]) > 4.0 * float(R0["cmax"]):
        _note(bad, "cmax", f"{R1['cmax']!r} after rows of 8 x the norm, {R0['cmax']!r} before")
    ix.add(W["beyond"]); ix.search(q, K)              # beyond the reservation: the copy is dropped, mu anew over all rows
    R2 = ix.last_centre()
    everything = np.concatenate([both, W["beyond"]])
    _merge(bad, check_conversion(R2, everything, metric, what="after the capacity change: "))
    if same_bits(R2["mu"], R0["mu"]).all():
        _note(bad, "mu", "after the capacity change mu is still the first rows'")
    ix.reset(); ix.add(W["after_reset"]); ix.search(q, K)
    R3 = ix.last_centre()
    _merge(bad, check_conversion(R3, W["after_reset"], metric, what="after the reset: "))
    _merge(bad, check_queries(R3, q, what="after the reset: "))
    ix.close()
    return bad


def run_two_searches(make, metric):
    s = TWO_SEARCHES
    W = world("float", s["N"], s["D"], s["nq"], 11)
    A = W["queries"]
    B = float_world(s["N"], s["D"], s["nq"], 12, q_shift=-10.0)["queries"]
    bad = {}
    ix = make(s["D"], metric)
    ix.set_escalation(False)
    ix.add(W["bank"]); ix.search(A, K)
    RA = ix.last_centre()
    _merge(bad, check_queries(RA, A, what="search A: "))
    ix.search(B, K)
    RB = ix.last_centre()
    if RB["t"] == RA["t"]:
        _note(bad, "t", f"{RB['t']!r} after both searches: the two query sets no longer differ in their means")
    _merge(bad, check_queries(RB, B, what="search B: "))
    _merge(bad, check_conversion(RB, W["bank"], metric, what="search B: "))
    ix.close()
    return bad


def query_shape_sets(D=40):
    out = []
    for nq in QUERY_SHAPES:
        q = float_world(64, D, nq, 20 + nq)["queries"].copy()
        if nq > 1:
            q[nq // 2, 3] = np.nan                   # out of t's sum, in its denominator
        out.append(q)
    return out


def run_query_shapes(make, metric):
    W = world("float", 1000, 40, 70)
    bad = {}
    ix = make(40, metric)
    ix.set_escalation(False)
    ix.add(W["bank"])
    for q in query_shape_sets():
        ix.search(q, K)
        R = ix.last_centre()
        _merge(bad, check_queries(R, q, what=f"nq = {q.shape[0]}: "))
        _merge(bad, check_conversion(R, W["bank"], metric, what=f"nq = {q.shape[0]}: "))
    ix.close()
    return bad


def run_second_pass(make, metric=0):
    s, W = SECOND_PASS, second_pass_world()
    q, k = W["queries"], s["k"]
    bad = {}
    ix = make(s["D"], metric)
    ix.add(W["bank"]); ix.set_escalation(False); ix.search(q, k)
    R0 = ix.last_centre()
    F = np.flatnonzero(np.asarray(ix.certified()) == 0)
    if not 0 < F.size < q.shape[0]:
        _note(bad, "n", f"{F.size} of {q.shape[0]} first certificates failed: no second pass over a PART of the queries")
        return bad
    _merge(bad, check_queries(R0, q, what="level 0: "))
    jx = make(s["D"], metric)
    jx.add(W["bank"]); jx.set_escalation(True); jx.search(q, k)
    R1 = jx.last_centre()
    if R1["level"] != 1:
        _note(bad, "level", f"{R1['level']} after a search whose second pass ran")
    if R1["n"] != F.size:
        _note(bad, "n", f"{R1['n']} queries in the second pass, {F.size} first certificates failed")
        return bad
    if not same_bits(R1["cq"], R0["cq"][F]).all():
        _note(bad, "cq", "the second pass' c_q are not the level-0 values of the failing queries in ascending order")
    if not same_bits(R1["qcn"], R0["qcn"][F]).all():
        _note(bad, "qcn", "the second pass' ||q - t mu|| are not the level-0 values of the failing queries in ascending order")
    if R1["t"].view(np.uint32) != R0["t"].view(np.uint32):
        _note(bad, "t", f"{R1['t']!r} after the second pass, {R0['t']!r} before it")
    if not same_bits(R1["init16"], R0["init16"]).all():
        _note(bad, "init16", "the second pass has changed init16")
    _merge(bad, check_queries(R1, q[F], derive_t=False, what="level 1: "))
    _merge(bad, check_conversion(R1, W["bank"], metric, what="level 1: "))
    ix.close(); jx.close()
    return bad


def run_view(make, metric=0):
    v = VIEW
    W = world("float", v["N"], v["D"], 70)
    ids = np.sort(np.random.default_rng(13).choice(v["N"], v["take"], replace=False))
    bad = {}
    ix = make(v["D"], metric)
    ix.set_escalation(False)
    ix.add(W["bank"]); ix.search(W["queries"], K)
    view = ix.select_rows(ids)
    view.set_escalation(False)
    view.search(W["queries"], K)
    R = view.last_centre()
    _merge(bad, check_conversion(R, W["bank"][ids], metric, what="view: "))
    _merge(bad, check_queries(R, W["queries"], what="view: "))
    if same_bits(R["mu"], ix.last_centre(queries=False)["mu"]).all():
        _note(bad, "mu", "the view's mu is its source's")
    view.close(); ix.close()
    return bad
