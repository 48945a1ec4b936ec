"""The references of tests/f16_centre_refs.py held to what they promise, on the CPU.

`HostModel` restates the state machine of csrc/hbird_f16_centre.hip and its callers in plain numpy -- capacity, the lazy copy, rows appended
behind it, reset, the caller's pass and the second pass -- and fills a read-out in the layout of include/hbird_hip_centre.h (its tiler is
written from the header's formula, one index at a time; the references' de-tiler is a reshape).  The scenarios of f16_centre_refs.py (the ones
the GPU file runs on HipFlatIndex) must find nothing to complain about on the faithful model, and each WRONG variant below must fail the named
assertion on those same inputs.  The table of profiles/r19/README.md is this file's MUTATIONS.

The case-list guard restates the launch arithmetic of the conversion and fails when the GPU file's case list stops reaching a regime of its
table (the manner of tests/test_bank_paths_cpu.py)."""
import ctypes
import math

import numpy as np
import pytest

import bank_refs
import f16_centre_refs as R
import f16_pass_refs as P
import oracle
import test_f16_centre_cpu as cm

F32 = np.float32


# ---- the tiler, from the header's formula ---------------------------------------------------------------------------------------------------------
def tile16(rows_u16, dp16):
    """uint16 [n, dp16] -> raw [n * dp16]: component k of row r sits at ((r / 32 * (dp16 / 8) + k / 8) * 32 + r % 32) * 8 + k % 8."""
    n = rows_u16.shape[0]
    assert n % 32 == 0 and rows_u16.shape[1] == dp16
    r, k = np.meshgrid(np.arange(n), np.arange(dp16), indexing="ij")
    off = ((r // 32 * (dp16 // 8) + k // 8) * 32 + r % 32) * 8 + k % 8
    raw = np.full(n * dp16, 0xDEAD, dtype=np.uint16)
    raw[off.ravel()] = rows_u16.ravel()
    return raw


@pytest.mark.parametrize("n,dp16", [(32, 128), (96, 256), (1024, 128)])
def test_the_detiler_undoes_the_headers_layout(n, dp16):
    rng = np.random.default_rng(n + dp16)
    x = rng.integers(0, 65536, size=(n, dp16)).astype(np.uint16)
    raw = tile16(x, dp16)
    assert np.array_equal(R.detile16(raw, n, dp16), x)
    # ... and the formula is the one centre_bank_kernel writes: f16x8 index rt * g16 * 64 + gg * 32 + i, eight halves each, g16 = dp16 / 16
    rt, gg, i, j = 1 if n > 32 else 0, 3, 17, 5
    assert raw[((rt * (dp16 // 16) * 64) + gg * 32 + i) * 8 + j] == x[rt * 32 + i, 8 * gg + j]


# ---- fmaf is not a float64 multiply-add and a cast -------------------------------------------------------------------------------------------------
def test_fma_f32_differs_from_the_naive_emulation_at_an_fp32_midpoint():
    """a b = 2^-24 - 2^-54, c = 1 + 2^-23 (odd last bit): the exact a b + c lies 2^-54 BELOW the midpoint of c and its successor, so fmaf gives c.
    The float64 sum rounds to the midpoint itself, and the cast breaks the tie to even: the successor."""
    a, b, c = F32(1.0 + 2.0 ** -15), F32((1.0 - 2.0 ** -15) * 2.0 ** -24), F32(1.0 + 2.0 ** -23)
    assert float(a) * float(b) == 2.0 ** -24 - 2.0 ** -54                       # exact in float64
    naive = F32(float(a) * float(b) + float(c))
    right = bank_refs.fma_f32(np.array([a]), np.array([b]), np.array([c]))[0]
    assert right == c and naive == np.nextafter(c, F32(2.0)) and naive != right
    assert R.chain_dot(np.array([[1.0, a]], F32), np.array([c, b], F32))[0] == c   # the chains of the references go through it


def test_roundup32_is_the_smallest_fp32_not_below():
    x = np.array([1.0, 1.0 + 2.0 ** -40, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23, 0.0, np.inf, 3.0e38 * 2.0], np.float64)
    up = R.roundup32(x)
    assert (up.astype(np.float64) >= x).all() and (np.nextafter(up, F32(-np.inf)).astype(np.float64)[[1, 2]] < x[[1, 2]]).all()
    assert up[0] == 1.0 and up[1] == up[2] == up[3] == F32(1.0 + 2.0 ** -23) and up[4] == 0.0 and np.isposinf(up[5])
    assert np.isnan(R.roundup32(np.array([np.nan]))[0])


# ---- the host model --------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # name: (the scenario that must catch it, the assertion that must fail)
    "mean_over_padded_rows": ("fresh", "mu"),
    "nan_row_zeroed": ("invalid", "mu"),
    "cmax_first_conversion_only": ("append", "cmax"),
    "cmax_kept_across_reset": ("append", "cmax"),
    "mu_norm_to_nearest": ("norms", "mu_norm"),
    "cmax_to_nearest": ("norms", "cmax"),
    "qcn_to_nearest": ("fresh", "qcn"),
    "g_from_fp16_differences": ("fresh", "g"),
    "init16_from_previous_t": ("two_searches", "init16"),
    "t_over_finite_queries": ("query_shapes", "t"),
    "mu_padding_nonzero": ("fresh", "mu_padding"),
    "query_padding_nonzero": ("fresh", "q_padding"),
    "init16_padding_finite": ("fresh", "init16_padding"),
    "append_with_new_mean": ("append", "mu"),
    # beyond the issue's list
    "second_pass_rederives_t": ("second_pass", "t"),
    "tiles_to_fp16_truncated": ("fresh", "tiles"),
    "view_keeps_source_mean": ("view", "mu"),
}


def _up(x64, nearest):
    return np.asarray(x64, np.float64).astype(F32) if nearest else R.roundup32(x64)


class HostModel:
    """What the library does, call by call, in numpy.  `mut`: one name of MUTATIONS (None: faithful)."""

    def __init__(self, D, metric, mut=None):
        self.D, self.metric, self.mut = D, metric, mut
        self.dp, self.dp16 = (D + 15) // 16 * 16, (D + 127) // 128 * 128
        self.cap = 0
        self.bank = np.zeros((0, D), F32)
        self.f16_cap, self.f16_rows = -1, 0
        self.c_cap, self.active, self.rows = -1, False, 0
        self.mu = None
        self.cmax, self.t = F32(0.0), F32(0.0)
        self.escalation = True
        self.q = None
        self._cert = None
        self._forced_mu = None

    # -- the bank
    @property
    def ntotal(self):
        return self.bank.shape[0]

    def reserve(self, n):
        self.cap = max(self.cap, (n + 255) // 256 * 256)

    def add(self, rows):
        rows = np.ascontiguousarray(rows, F32)
        if self.ntotal + rows.shape[0] > self.cap:
            self.reserve(max(self.ntotal + rows.shape[0], self.cap + self.cap // 2))
        self.bank = np.concatenate([self.bank, rows])
        self.q = None

    def reset(self):
        self.bank = np.zeros((0, self.D), F32)
        self.f16_rows, self.rows, self.q = 0, 0, None

    def select_rows(self, ids):
        view = HostModel(self.D, self.metric, self.mut)
        view.add(self.bank[np.asarray(ids)])
        if self.mut == "view_keeps_source_mean":
            view._forced_mu = self.mu.copy()
        return view

    def set_escalation(self, on):
        self.escalation = bool(on)

    def close(self):
        pass

    # -- the copy
    def _stored(self, lo, hi):
        """fp32 rows [lo, hi) of the tiles: zero rows beyond the bank"""
        out = np.zeros((hi - lo, self.D), F32)
        n = max(0, min(hi, self.ntotal) - lo)
        out[:n] = self.bank[lo:lo + n]
        return out

    def _derive_mean(self):
        b = self.bank
        ok = np.isfinite(b).all(axis=1)
        if self.metric == 1:
            with np.errstate(invalid="ignore", over="ignore"):
                ok &= (F32(-0.5) * oracle.chain_sqnorm(b)) > -np.inf
        if self.mut == "nan_row_zeroed":
            s, n = np.where(ok[:, None], b, F32(0.0)).astype(np.float64).sum(axis=0), b.shape[0]
        else:
            s, n = b[ok].astype(np.float64).sum(axis=0), int(ok.sum())
        if self.mut == "mean_over_padded_rows":
            n = (b.shape[0] + 31) // 32 * 32
        mu = np.zeros(self.dp16, F32)
        if n > 0:
            mu[:self.D] = (s / n).astype(F32)
        if self.mut == "mu_padding_nonzero" and self.dp16 > self.D:
            mu[self.D:] = mu[0]
        if self._forced_mu is not None:
            mu = self._forced_mu
        self.mu = mu
        m2 = 0.0
        for v in mu.astype(np.float64):
            m2 = m2 + v * v
        self.mu2, self.mu_norm = F32(m2), _up(math.sqrt(m2), self.mut == "mu_norm_to_nearest")[()]
        if self.mut != "cmax_kept_across_reset":
            self.cmax = F32(0.0)
        self.t = F32(0.0)
        self.active = bool(np.isfinite(self.mu_norm) and self.mu2 > 0)

    def _fma(self, a, b, c):
        return bank_refs.fma_f32(a, b, c)

    def _chain(self, a, b):
        c = np.zeros(a.shape[0], F32)
        for k in range(a.shape[1]):
            c = self._fma(a[:, k], np.broadcast_to(b[..., k], c.shape), c)
        return c

    def _to16(self, x32):
        if self.mut == "tiles_to_fp16_truncated":
            with np.errstate(over="ignore", invalid="ignore"):
                h = x32.astype(np.float16)
                over = np.abs(h.astype(F32)) > np.abs(x32)
                return np.where(over, np.nextafter(h, np.float16(0.0)), h).view(np.uint16)
        return R.f16_bits(x32)

    def _convert(self):
        if self.c_cap != self.cap or self.mu is None:
            self.c_cap, self.active, self.rows, self.q = self.cap, False, 0, None
            self.g = np.zeros(self.cap, F32)
            self.init16 = np.full(self.cap, -np.inf, F32)
            assert self.f16_rows == 0
        fresh = self.f16_rows == 0
        if fresh or self.mut == "append_with_new_mean":
            keep = self.cmax
            self._derive_mean()
            if not fresh:
                self.cmax = keep
        if not self.active:
            return False
        lo, hi = self.f16_rows // 32 * 32, (self.ntotal + 31) // 32 * 32
        x = self._stored(lo, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.zeros((hi - lo, self.dp16), F32)
            d[:, :self.D] = x - self.mu[None, :self.D]
        self.t16[lo:hi] = self._to16(d)
        dg = d.astype(np.float16).astype(F32) if self.mut == "g_from_fp16_differences" else d
        with np.errstate(invalid="ignore", over="ignore"):
            self.g[lo:hi] = self._chain(dg[:, :self.dp], self.mu[None, :self.dp])
        real = d[:max(0, self.ntotal - lo)]
        n2 = np.zeros(real.shape[0])
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(self.dp):
                n2 = n2 + real[:, k].astype(np.float64) ** 2
            cn = _up(np.sqrt(n2), self.mut == "cmax_to_nearest")
        cn = np.where(np.isnan(cn), F32(0.0), cn)
        if cn.size and not (self.mut == "cmax_first_conversion_only" and not fresh):
            self.cmax = max(self.cmax, F32(cn.max()))
        self.rows = self.ntotal
        return True

    def _upkeep(self):
        if self.f16_cap != self.cap:
            self.t16 = np.zeros((self.cap, self.dp16), np.uint16)
            self.f16_cap, self.f16_rows = self.cap, 0
        if self.f16_rows < self.ntotal:
            self._convert()
            self.f16_rows = self.ntotal

    # -- the query side
    def _binit(self, n):
        out = np.full(n, -np.inf, F32)
        b = self.bank
        with np.errstate(invalid="ignore", over="ignore"):
            out[:b.shape[0]] = F32(-0.5) * oracle.chain_sqnorm(b) if self.metric == 1 else F32(0.0)
        return out

    def _queries(self, q, first):
        nq = q.shape[0]
        qp = np.zeros((nq, self.dp), F32)
        qp[:, :self.D] = q
        with np.errstate(invalid="ignore", over="ignore"):
            cq = self._chain(qp, self.mu[None, :self.dp])
        if first or self.mut == "second_pass_rederives_t":
            t_before = self.t
            fin = np.isfinite(cq)
            den = float(fin.sum() if self.mut == "t_over_finite_queries" else nq) * float(self.mu2)
            t = F32(math.fsum(cq[fin].astype(np.float64)) / den) if self.mu2 > 0 and den > 0 else F32(0.0)
            self.t = t if np.isfinite(t) else F32(0.0)
            n = (self.ntotal + 255) // 256 * 256
            binit = self._binit(n)
            if self.mut == "init16_padding_finite":
                binit = np.where(np.arange(n) >= self.ntotal, F32(0.0), binit)
            t_used = t_before if self.mut == "init16_from_previous_t" else self.t
            v = self._fma(np.broadcast_to(F32(t_used), (n,)), self.g[:n], binit)
            self.init16[:n] = np.where(np.isneginf(binit), F32(-np.inf), v)
        nqp = (nq + 255) // 256 * 256
        d = np.zeros((nqp, self.dp16), F32)
        d[:nq, :self.dp] = self._fma(np.broadcast_to(F32(-self.t), qp.shape), np.broadcast_to(self.mu[None, :self.dp], qp.shape), qp)
        if self.mut == "query_padding_nonzero":
            d[nq:, :self.dp] = F32(-self.t) * self.mu[None, :self.dp]
        n2 = np.zeros(nq)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(self.dp):
                n2 = n2 + d[:nq, k].astype(np.float64) ** 2
            qcn = _up(np.sqrt(n2), self.mut == "qcn_to_nearest")
        self.q = {"n": nq, "level": 0 if first else 1, "cq": cq, "qcn": qcn, "q16": tile16(R.f16_bits(d), self.dp16)}

    def search(self, q, k):
        q = np.ascontiguousarray(q, F32)
        self.q, self._cert = None, None
        self._upkeep()
        self._last = (q, k)
        if not self.active:
            return
        self._queries(q, True)
        if self.escalation and self.ntotal >= 4096 and P.kc_of(k) < 256:
            F = np.flatnonzero(~self.certified())
            if F.size:
                self._queries(q[F], False)

    def certified(self):
        """The first certificates by the CPU restatement of the pass (tests/test_f16_centre_cpu.centred_model): the model runs no pass of its own."""
        if self._cert is None:
            q, k = self._last
            self._cert = cm.centred_model(q, self.bank, k, P.kc_of(k), self.metric)["certified"][1.05]
        return self._cert

    def last_centre(self, queries=True):
        if not (self.active and self.rows > 0):
            raise RuntimeError("hb_index_last_centre: no active centred copy")
        n_g, n_init = (self.rows + 31) // 32 * 32, (self.rows + 255) // 256 * 256
        out = {"rows": self.rows, "dp16": self.dp16, "n_mu": self.dp16, "n": self.q["n"] if self.q else 0, "level": self.q["level"] if self.q else -1,
               "mu": self.mu.copy(), "cmax": F32(self.cmax), "mu_norm": F32(self.mu_norm), "mu2": F32(self.mu2), "t": F32(self.t),
               "g": self.g[:n_g].copy(), "init16": self.init16[:n_init].copy(), "bank16": tile16(self.t16[:n_g], self.dp16)}
        if queries:
            if not self.q:
                raise RuntimeError("hb_index_last_centre: the last search of a caller did not run centred")
            out.update(cq=self.q["cq"], qcn=self.q["qcn"], q16=self.q["q16"])
        return out


def _make(mut=None):
    return lambda D, metric: HostModel(D, metric, mut)


def _run_norms(make):
    """Every fresh world: a norm rounded to nearest differs from the one rounded up on about half of them."""
    bad = {}
    for c in R.FRESH_CASES:
        W = R.world(c.kind, c.N, c.D, c.nq)
        ix = make(c.D, c.metric)
        ix.set_escalation(False)
        ix.add(W["bank"]); ix.search(W["queries"], R.K)
        for name, msg in R.check_conversion(ix.last_centre(), W["bank"], c.metric, exact=W["exact"]).items():
            bad.setdefault(name, msg)
    return bad


SCENARIOS = {
    "fresh": lambda make: R.run_fresh(make, R.FRESH_CASES[0]),
    "invalid": lambda make: R.run_invalid_rows(make, 0),
    "append": lambda make: R.run_append_capacity_reset(make, 1),
    "two_searches": lambda make: R.run_two_searches(make, 1),
    "query_shapes": lambda make: R.run_query_shapes(make, 0),
    "second_pass": lambda make: R.run_second_pass(make, 0),
    "view": lambda make: R.run_view(make, 0),
    "norms": _run_norms,
}


@pytest.mark.parametrize("c", R.FRESH_CASES, ids=lambda c: f"{c.N}x{c.D}-m{c.metric}-{c.kind}")
def test_the_faithful_model_passes_every_fresh_case(c):
    assert R.run_fresh(_make(), c) == {}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", ["invalid", "append", "two_searches", "query_shapes", "view"])
def test_the_faithful_model_passes_the_state_machine_scenarios(name, metric):
    run = {"invalid": R.run_invalid_rows, "append": R.run_append_capacity_reset, "two_searches": R.run_two_searches,
           "query_shapes": R.run_query_shapes, "view": R.run_view}[name]
    assert run(_make(), metric) == {}


def test_the_second_pass_world_leaves_a_part_of_the_queries_uncertified_and_the_model_passes():
    s, W = R.SECOND_PASS, R.second_pass_world()
    m = cm.centred_model(W["queries"], W["bank"], s["k"], P.kc_of(s["k"]), 0)
    share = 1.0 - float(m["certified"][1.05].mean())
    print(f"second_pass_world: {share:.3f} of the queries uncertified by the CPU restatement")
    assert 0.10 <= share <= 0.90
    assert s["N"] >= 4096 and P.kc_of(s["k"]) < 256
    assert R.run_second_pass(_make(), 0) == {}


def test_the_zero_mean_world_has_no_centred_copy():
    W = R.zero_mean_world()
    assert (W["bank"].astype(np.float64).sum(axis=0) == 0).all()
    ix = HostModel(W["bank"].shape[1], 0)
    ix.add(W["bank"]); ix.search(W["queries"], R.K)
    with pytest.raises(RuntimeError, match="no active centred copy"):
        ix.last_centre()


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_every_wrong_variant_fails_its_named_assertion(mut):
    scenario, name = MUTATIONS[mut]
    bad = SCENARIOS[scenario](_make(mut))
    print(f"MUTATION {mut}: scenario {scenario}, fails {sorted(bad)}")
    assert name in bad, f"{mut} is not caught by `{name}` on the {scenario} scenario (fails: {sorted(bad)})"


# ---- the case list reaches what its table names ----------------------------------------------------------------------------------------------------
def test_the_case_list_reaches_every_regime_of_the_conversion():
    L = {s: R.launch_regime(*s) for s in R.FRESH_SHAPES}
    a = L[(1000, 40)]
    assert a["row_tiles"] == 32 < R.PARTS and a["per"] == 1 and a["empty_partitions"] == 96 and a["last_tile_rows"] == 8
    assert a["g8"] == 6 and a["dp16"] == 128 and a["zero_groups"] == 10 and a["dp16"] > a["g8"] * 8
    b = L[(1000, 128)]
    assert b["g8"] * 8 == b["dp16"] == 128 and b["zero_groups"] == 0
    c = L[(5000, 136)]
    assert c["row_tiles"] == 157 and c["per"] == 2 and c["ragged_last_partition"] and c["empty_partitions"] == 49
    assert c["g8"] == 18 and c["dp16"] == 256 and c["tiles_mod_8"] != 0
    d = L[(20000, 64)]
    assert d["per"] == 5 and d["wave0_trips"] == 2 and d["wave3_trips"] == 1
    # both metrics on the first and third shapes, a float and an exact world on every shape
    for shape in R.FRESH_SHAPES:
        kinds = {(x.kind, x.metric) for x in R.FRESH_CASES if (x.N, x.D) == shape}
        assert {k for k, _ in kinds} == {"float", "exact"}
        if shape in ((1000, 40), (5000, 136)):
            assert kinds == {("float", 0), ("float", 1), ("exact", 0), ("exact", 1)}
    # the append: a copy that ends inside a row tile, appended rows within the reservation, then beyond it
    ap = R.APPEND
    assert ap["first"] % 32 != 0 and ap["first"] + ap["more"] <= ap["reserve"] and ap["first"] + ap["more"] == 4500
    W = R.append_world()
    assert W["first"].shape[0] + W["more"].shape[0] + W["beyond"].shape[0] > (ap["reserve"] + 255) // 256 * 256
    assert W["after_reset"].shape[0] == 1000 and 1000 % 256 != 0
    big = np.sqrt((W["more"][ap["big_from"]:].astype(np.float64) ** 2).sum(axis=1)).min()
    assert big > 4.0 * np.sqrt((W["first"].astype(np.float64) ** 2).sum(axis=1)).max()
    # invalid rows: row 0, the first tile, the last tile; the +inf component in a row of its own
    V = R.invalid_rows_world()
    nan_rows = np.flatnonzero(np.isnan(V["bank"]).any(axis=1))
    assert 0 in nan_rows and ((nan_rows > 0) & (nan_rows < 32)).any() and (nan_rows >= 992).any()
    inf_rows = np.flatnonzero(np.isinf(V["bank_inf"]).any(axis=1))
    assert inf_rows.size == 1 and not np.isnan(V["bank_inf"][inf_rows[0]]).any() and np.array_equal(R.valid_rows(V["bank"]), R.valid_rows(V["bank_inf"]))
    # the query shapes: blocks of 64, row tiles of 32, tiles of 256
    assert R.QUERY_SHAPES == (1, 70, 300)
    blocks = [(-(-n // 64), n % 64 != 0, -(-n // 32), -(-n // 256)) for n in R.QUERY_SHAPES]
    assert blocks[0] == (1, True, 1, 1) and blocks[1] == (2, True, 3, 1) and blocks[2] == (5, True, 10, 2)
    sets = R.query_shape_sets()
    assert [int(np.isnan(q).any(axis=1).sum()) for q in sets] == [0, 1, 1]
    # two searches: the query sets differ in their means along mu
    assert R.TWO_SEARCHES["N"] == 5000 and R.SECOND_PASS["N"] >= 4096 and R.VIEW == {"N": 5000, "D": 136, "take": 2000}


# ---- the entry ------------------------------------------------------------------------------------------------------------------------------------
def test_last_centre_is_bound_and_refuses_without_a_gpu():
    from hbird_mi import _lib
    from hbird_mi.nn import search_hip
    L = _lib.lib()
    info = (ctypes.c_int64 * 8)()
    assert L.hb_index_last_centre(None, None, None, None, None, None, None, None, None, info) != 0 and b"NULL index handle" in L.hb_last_error()
    assert callable(search_hip.HipFlatIndex.last_centre)
