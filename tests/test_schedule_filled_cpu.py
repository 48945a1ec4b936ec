"""The FILLED clustered work list (hb_build_clustered with `filled`, through hb_schedule_plan_filled): the leftover r = nqt mod cq query
tiles of a ragged last query group are dealt as rows of other shapes with the same member count CS = cq cb -- r as a sum of powers of two,
a part of 2^i tiles as units of (2^i query tiles) x (CS / 2^i consecutive bank tiles) -- so that no member idles for a whole row.

Every check is a function of its own over the returned list, and every one of them is shown a mutated list that it must reject."""
import ctypes

import numpy as np
import pytest

from hbird_mi import _lib

SHARES = (1.02, 0.98, 1.01, 0.99, 1.0, 1.0, 1.03, 0.97)
COLS = dict(blk=0, q=1, b0=2, n=3, slot=4, first=5, stride=6, tile0=7, next=8, member=9)


def plan_filled(nqt, nbt, G, panel, cq, cb, phased=False, share=True, weights=None, limit=0, d=768):
    """-> dict: segs [n, 10] as hb_schedule_plan returns them, the statistics, the cut clocks and bounds [cut][block]."""
    L = _lib.lib()
    stats = (ctypes.c_int64 * 12)()
    n_cuts = ctypes.c_int(0)
    w = (ctypes.c_double * 8)(*weights) if weights is not None else None
    _lib.check(L.hb_schedule_plan_filled(nqt, nbt, G, panel, d, cq, cb, int(phased), int(share), w, limit, None, 0, stats, None, 0, ctypes.byref(n_cuts), None))
    nseg, nc, g = stats[1], n_cuts.value, stats[0]
    segs = np.zeros((nseg, 10), dtype=np.int32)
    clocks = np.zeros(max(nc, 1), dtype=np.int32)
    bounds = np.zeros((max(nc, 1), g), dtype=np.int32)
    _lib.check(L.hb_schedule_plan_filled(nqt, nbt, G, panel, d, cq, cb, int(phased), int(share), w, limit, segs.ctypes.data_as(ctypes.c_void_p), nseg, stats,
                                         clocks.ctypes.data_as(ctypes.c_void_p), nc, ctypes.byref(n_cuts), bounds.ctypes.data_as(ctypes.c_void_p)))
    return dict(segs=segs, nqt=nqt, nbt=nbt, G=int(g), slots=int(stats[2]), panel=int(stats[3]), max_slots=int(stats[4]), cq=int(stats[7]) // 16,
                cb=int(stats[7]) % 16, filled=int(stats[8]), idle=int(stats[9]), member_ticks=int(stats[10]), refused=int(stats[11]),
                clocks=clocks[:nc].copy(), bounds=bounds[:nc].copy())


def plan_old(nqt, nbt, G, panel, cq, cb, phased=False, share=True, weights=None, d=768):
    """The same search through the entry points of old -> segs."""
    L = _lib.lib()
    stats = (ctypes.c_int64 * 8)()
    n_cuts = ctypes.c_int(0)

    def call(buf, n):
        p = buf.ctypes.data_as(ctypes.c_void_p) if buf is not None else None
        if weights is not None:
            w = (ctypes.c_double * 8)(*weights)
            return L.hb_schedule_plan_weighted(nqt, nbt, G, panel, d, cq, cb, int(share) + 2 * int(phased), w, p, n, stats)
        if share:
            return L.hb_schedule_plan_shared(nqt, nbt, G, panel, d, cq, cb, int(phased), p, n, stats)
        if phased:
            return L.hb_schedule_plan_phased(nqt, nbt, G, panel, d, cq, cb, p, n, stats, None, 0, ctypes.byref(n_cuts), None)
        return L.hb_schedule_plan(nqt, nbt, G, panel, d, cq, cb, p, n, stats)
    _lib.check(call(None, 0))
    segs = np.zeros((stats[1], 10), dtype=np.int32)
    _lib.check(call(segs, stats[1]))
    return segs


def expand(P):
    """One row per (segment, tile): block, cluster, member, query tile, bank tile, tick, stride."""
    s = P["segs"]
    n = s[:, COLS["n"]].astype(np.int64)
    rep = np.repeat(np.arange(len(s)), n)
    j = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    return dict(blk=s[rep, 0], cl=s[rep, 9] // 32, m=s[rep, 9] % 32, q=s[rep, 1].astype(np.int64), bt=s[rep, 2] + s[rep, 6].astype(np.int64) * j,
                tick=s[rep, 7] + j, stride=s[rep, 6])


# ---- the checks -------------------------------------------------------------------------------------------------------------------------
def check_cover(P):
    e = expand(P)
    assert (e["q"] >= 0).all() and (e["q"] < P["nqt"]).all() and (e["bt"] >= 0).all() and (e["bt"] < P["nbt"]).all()
    cover = np.bincount(e["q"] * P["nbt"] + e["bt"], minlength=P["nqt"] * P["nbt"])
    assert (cover == 1).all(), "every (query tile, bank tile) pair exactly once"


def check_slots(P):
    """A slot is one block and one query tile, started once (`first`) ahead of its continuations, with ascending bank tiles."""
    s = P["segs"]
    assert (s[:, 3] > 0).all() and (np.diff(s[:, 0]) >= 0).all()       # segments are grouped by block
    order = np.argsort(s[:, 4], kind="stable")
    t = s[order]
    new = np.r_[True, t[1:, 4] != t[:-1, 4]]
    assert sorted(set(t[:, 4].tolist())) == list(range(P["slots"]))
    assert (t[new, 5] == 1).all() and (t[~new, 5] == 0).all(), "`first` marks exactly a slot's first segment"
    same = ~new[1:]
    assert (t[1:, 0][same] == t[:-1, 0][same]).all() and (t[1:, 1][same] == t[:-1, 1][same]).all(), "one block, one query tile per slot"
    last = t[:-1, 2] + t[:-1, 6] * (t[:-1, 3] - 1)
    assert (t[1:, 2][same] > last[same]).all(), "bank tiles of a slot must ascend"
    per_q = np.bincount(t[new, 1], minlength=P["nqt"])
    assert per_q.max() == P["max_slots"]


def check_clocks(P):
    s = P["segs"]
    same = s[1:, 0] == s[:-1, 0]
    assert (s[1:, 7][same] >= (s[:-1, 7] + s[:-1, 3])[same]).all(), "a block's clock never runs backwards"
    assert (s[:, 8] >= s[:, 7] + s[:, 3]).all()
    assert (s[:-1, 8][same] == s[1:, 7][same]).all() and (s[:-1, 8][~same] == 0x7FFFFFFF).all() and s[-1, 8] == 0x7FFFFFFF


def check_xcd(P):
    """Whole clusters per XCD (blocks equal mod 8 share one), every member once."""
    s = P["segs"]
    CS = P["cq"] * P["cb"]
    per_xcd = P["G"] // CS // 8
    cl, m = s[:, 9] // 32, s[:, 9] % 32
    assert (s[:, 9] >= 0).all() and (m < CS).all() and (cl < P["G"] // CS).all()
    assert (s[:, 0] % 8 == cl // per_xcd).all(), "the members of a cluster are on one XCD"
    blocks = {}
    for b, c, mm in set(zip(s[:, 0].tolist(), cl.tolist(), m.tolist())):
        assert blocks.setdefault((c, mm), b) == b
    assert len(set(blocks.values())) == len(blocks)


def check_ticks(P):
    """At every tick the busy members of a cluster hold pairs of ONE unit of some shape (CS / bw query ways) x (bw bank ways), bw = their common
    stride: member m has query way m / bw and bank way m mod bw, so q - m / bw and bank tile - m mod bw are the unit's own and equal for
    all (equal bank way: the same bank tile, equal query way: the same query tile)."""
    e = expand(P)
    CS = P["cq"] * P["cb"]
    assert (CS % e["stride"] == 0).all()
    T = int(e["tick"].max()) + 1
    key = e["cl"].astype(np.int64) * T + e["tick"]
    order = np.argsort(key, kind="stable")
    key = key[order]
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    for name, v in (("stride", e["stride"]), ("query tile", e["q"] - e["m"] // e["stride"]), ("bank tile", e["bt"] - e["m"] % e["stride"])):
        v = v[order].astype(np.int64)
        assert (np.minimum.reduceat(v, start) == np.maximum.reduceat(v, start)).all(), f"one unit per tick: {name}"
    km = key * 32 + e["m"][order]
    assert len(np.unique(km)) == len(km), "a member holds one pair per tick"
    # a unit lies inside one panel and starts at a multiple of its bank ways there
    base = (e["bt"] - e["m"] % e["stride"]) % P["panel"]
    assert (base % e["stride"] == 0).all()


def check_cuts(P):
    """All members of a cluster are cut at the same phase clocks: what a member runs before a cut ends before anything a member runs after it."""
    s = P["segs"]
    CS = P["cq"] * P["cb"]
    off = np.searchsorted(s[:, 0], np.arange(P["G"] + 1))
    cl_of = {int(b): int(c) for b, c in zip(s[:, 0], s[:, 9] // 32)}
    assert len(P["clocks"]) == len(P["bounds"])
    for p in range(len(P["clocks"])):
        before, after = {}, {}
        for b in range(P["G"]):
            if off[b] == off[b + 1]:
                continue
            i = off[b] + P["bounds"][p][b]
            assert off[b] <= i <= off[b + 1]
            c = cl_of[b]
            if i > off[b]:
                before[c] = max(before.get(c, 0), int(s[i - 1, 7] + s[i - 1, 3]))
            if i < off[b + 1]:
                after[c] = min(after.get(c, 1 << 31), int(s[i, 7]))
        for c in before:
            assert before[c] <= after.get(c, 1 << 31), "the members of a cluster are cut at one clock"
    return CS


def rows_of(nqt, cq, cb, filled):
    rows = [(cq, cb)] * (nqt // cq)
    r = nqt % cq
    if r and not filled:
        rows.append((cq, cb))
    part = cq // 2
    while filled and part >= 1:
        if r & part:
            rows.append((part, cq * cb // part))
        part //= 2
    return rows


def expected_idle(P, filled=True):
    """Member ticks without a pair: per panel and row the ways of its partial last unit beyond the panel's end -- and, unfilled, the query
    ways of the last group beyond the last tile."""
    idle = 0
    rows = rows_of(P["nqt"], P["cq"], P["cb"], filled)
    for b0 in range(0, P["nbt"], P["panel"]):
        pp = min(P["panel"], P["nbt"] - b0)
        for qw, bw in rows:
            idle += -(-pp // bw) * qw * bw
        idle -= pp * P["nqt"]
    return idle


def check_idle(P):
    s = P["segs"]
    CS = P["cq"] * P["cb"]
    ends = np.zeros(P["G"] // CS, dtype=np.int64)
    np.maximum.at(ends, s[:, 9] // 32, s[:, 7] + s[:, 3])
    assert P["member_ticks"] == ends.sum() * CS
    assert P["idle"] == P["member_ticks"] - P["nqt"] * P["nbt"]
    assert P["idle"] == expected_idle(P, filled=bool(P["filled"]))
    if P["filled"]:      # at most one unit per leftover row and panel, and the rule of old for a partial last bank group
        npanels = -(-P["nbt"] // P["panel"])
        assert P["idle"] <= npanels * len(rows_of(P["nqt"], P["cq"], P["cb"], True)) * (CS - 1)


def check_xcd_ticks(P):
    """Equal shares: the unit list of a panel is cut into eight ranges that differ by at most one unit."""
    s = P["segs"]
    CS = P["cq"] * P["cb"]
    NC = P["G"] // CS
    ends = np.zeros(NC, dtype=np.int64)
    np.maximum.at(ends, s[:, 9] // 32, s[:, 7] + s[:, 3])
    per = ends.reshape(8, NC // 8).sum(axis=1)
    npanels = -(-P["nbt"] // P["panel"])
    assert per.max() - per.min() <= npanels, per


CHECKS = [check_cover, check_slots, check_clocks, check_xcd, check_ticks, check_cuts, check_idle]

CASES = [(86, 39063, 256, 0, 8, 1, True), (49, 8102, 256, 0, 4, 1, False), (49, 8102, 256, 0, 4, 2, False), (86, 4883, 256, 0, 8, 1, False),
         (7, 1001, 64, 0, 2, 2, False), (5, 333, 32, 7, 2, 2, False), (3, 4, 256, 0, 2, 2, False)] + \
        [(8 * 3 + r, 300, 64, 0, 8, 1, bool(r & 1)) for r in range(1, 8)]


@pytest.mark.parametrize("share,weights", [(True, None), (False, None), (True, SHARES), (False, SHARES)])
@pytest.mark.parametrize("nqt,nbt,G,panel,cq,cb,phased", CASES)
def test_filled_list_invariants(nqt, nbt, G, panel, cq, cb, phased, share, weights):
    P = plan_filled(nqt, nbt, G, panel, cq, cb, phased=phased, share=share, weights=weights)
    if G % (8 * cq * cb) != 0 or nqt * nbt < G:
        assert (P["cq"], P["cb"], P["filled"]) == (1, 1, 0)
        return
    assert (P["cq"], P["cb"]) == (cq, cb) and P["filled"] == (1 if nqt % cq else 0) and not P["refused"]
    for check in CHECKS:
        check(P)
    if weights is None:
        check_xcd_ticks(P)
    # the strides are those of the rows: cb for the full groups, CS / 2^i for the parts of r
    want = {bw for _, bw in rows_of(nqt, cq, cb, True)}
    assert set(P["segs"][:, 6].tolist()) == want


def test_headline_idle_share():
    """86 query tiles as 8 x 1: 2 of 88 member slots idle in the list of old, below 0.2 % in the filled one; 16 slots for a tile of the 2 x 4 row."""
    P = plan_filled(86, 39063, 256, 0, 8, 1, phased=True)
    assert P["filled"] == 1 and P["panel"] == 128
    assert P["idle"] / P["member_ticks"] < 0.002
    old = plan_filled(86, 39063, 256, 0, 8, 1, phased=True, limit=1)      # (refused: the list of old with its statistics)
    assert old["refused"] == 1 and old["filled"] == 0
    assert abs(old["idle"] / old["member_ticks"] - 2 / 88) < 1e-3
    assert P["member_ticks"] < old["member_ticks"] * (1 - 0.02)
    assert P["max_slots"] == 16


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("phased", [True, False])
@pytest.mark.parametrize("nqt,nbt,G,panel,cq,cb", [(88, 4883, 256, 0, 8, 1), (48, 8102, 256, 0, 4, 2), (6, 1001, 64, 0, 2, 2), (24, 300, 64, 0, 8, 1), (6, 333, 32, 7, 2, 2)])
def test_nothing_left_over_is_the_old_list(nqt, nbt, G, panel, cq, cb, phased, share):
    P = plan_filled(nqt, nbt, G, panel, cq, cb, phased=phased, share=share)
    assert P["filled"] == 0 and np.array_equal(P["segs"], plan_old(nqt, nbt, G, panel, cq, cb, phased=phased, share=share))
    Pw = plan_filled(nqt, nbt, G, panel, cq, cb, phased=phased, share=share, weights=SHARES)
    assert np.array_equal(Pw["segs"], plan_old(nqt, nbt, G, panel, cq, cb, phased=phased, share=share, weights=SHARES))


@pytest.mark.parametrize("nqt,nbt,G,panel,cq,cb,phased", [(86, 4883, 256, 0, 8, 1, True), (49, 8102, 256, 0, 4, 2, False), (7, 1001, 64, 0, 2, 2, True)])
def test_fallback_at_the_slot_bound(nqt, nbt, G, panel, cq, cb, phased):
    P = plan_filled(nqt, nbt, G, panel, cq, cb, phased=phased)
    assert P["filled"] == 1
    at = plan_filled(nqt, nbt, G, panel, cq, cb, phased=phased, limit=P["max_slots"])
    assert at["filled"] == 1 and at["refused"] == 0 and np.array_equal(at["segs"], P["segs"])
    below = plan_filled(nqt, nbt, G, panel, cq, cb, phased=phased, limit=P["max_slots"] - 1)
    assert below["filled"] == 0 and below["refused"] == 1 and below["max_slots"] < P["max_slots"]
    assert np.array_equal(below["segs"], plan_old(nqt, nbt, G, panel, cq, cb, phased=phased))
    check_idle(below)


@pytest.mark.parametrize("nqt,cq,cb", [(7, 8, 1), (2, 8, 1), (2, 4, 2), (3, 4, 1)])
def test_fewer_query_tiles_than_query_ways_keep_the_old_list(nqt, cq, cb):
    P = plan_filled(nqt, 79, 64, 0, cq, cb, phased=True)
    assert (P["cq"], P["cb"], P["filled"], P["refused"]) == (cq, cb, 0, 0)
    assert np.array_equal(P["segs"], plan_old(nqt, 79, 64, 0, cq, cb, phased=True))
    check_idle(P)


def test_the_gpu_tests_lists():
    """What tests/test_schedule_filled_gpu.py runs: 79 bank tiles in one panel on 64 workgroups, and 86 x 1,172 tiles as 8 x 1."""
    for nqt, cq, cb in [(7, 4, 2), (11, 8, 1), (11, 4, 2), (14, 8, 1), (14, 4, 2)]:
        for phased in (True, False):
            P = plan_filled(nqt, 79, 64, 0, cq, cb, phased=phased, d=64)
            assert P["filled"] == 1 and P["panel"] >= 79 and P["idle"] < 3 * cq * cb
            for check in CHECKS:
                check(P)
    P = plan_filled(86, 1172, 256, 0, 8, 1, phased=True)
    assert P["filled"] == 1 and P["max_slots"] == 16 and P["idle"] * 500 < P["member_ticks"]
    for check in CHECKS:
        check(P)


def test_which_searches_ask_for_the_filled_list():
    """hb_knn_plan_clusters through hb_knn_plan_replay (out[19]): the fp16 candidate pass wherever its clusters are on and a query tile is left
    over -- automatically and in mode 3, not in modes 1 and 2 --, never the fp32 kernels, never with fewer tiles than query ways."""
    import test_knn_plan_cpu as KP

    def ask(**kw):
        v = dict(KP.BASE, **kw)
        a = (ctypes.c_int64 * len(KP.IN))(*[v[n] for n in KP.IN])
        o = (ctypes.c_int64 * 20)()
        assert _lib.lib().hb_knn_plan_replay(a, len(KP.IN), o, 20) == 0
        return dict(cq=int(o[9]), cb=int(o[10]), xs=int(o[14]), filled=int(o[19]))
    big = dict(f16=1, ntotal=10_000_000, g8=96, dp=768, dp16=768)
    assert ask(nq=21_904, **big) == dict(cq=8, cb=1, xs=1, filled=1)                      # the headline, automatic
    assert ask(nq=21_904, xcd_share=3, **big) == dict(cq=8, cb=1, xs=1, filled=1)
    assert ask(nq=21_904, xcd_share=2, **big) == dict(cq=8, cb=1, xs=1, filled=0)
    assert ask(nq=21_904, xcd_share=1, **big) == dict(cq=8, cb=1, xs=0, filled=0)
    assert ask(nq=88 * 256, **big) == dict(cq=8, cb=1, xs=1, filled=0)                    # nothing left over
    assert ask(nq=12_544, **dict(big, ntotal=5_000_000)) == dict(cq=4, cb=2, xs=1, filled=1)
    assert ask(nq=21_904, force_cq=8, force_cb=1, f16=1, ntotal=300_000, g8=96, dp=768, dp16=768) == dict(cq=8, cb=1, xs=1, filled=1)
    assert ask(nq=7 * 256, force_cq=8, force_cb=1, xcd_share=3, f16=1, ntotal=20_000 * 16) == dict(cq=8, cb=1, xs=1, filled=0)
    assert ask(nq=21_904, force_cq=2, force_cb=4, xcd_share=3, ntotal=10_000_000, g8=96, dp=768, dp16=768)["filled"] == 0      # the fp32 kernel
    assert ask(nq=21_904, ntotal=10_000_000, g8=96, dp=768, dp16=768)["filled"] == 0


def test_slot_limit_of_a_filled_list():
    """hb_fill_slot_limit as the launcher's kernels have it: pool_floor_kernel gathers max_slots x klw floats per wave in 144 KiB / 4 waves
    (phased searches), the merge reaches (48 KiB / 8 B / klw) slots per group x (48 KiB / 8 B / kc) groups.  Seen through the lists it refuses:
    the headline's filled list has 16 slots per leftover tile, which k = 30 (klw 192: 48) and k = 90 (klw 384: 24) take."""
    P = plan_filled(86, 39063, 256, 0, 8, 1, phased=True, limit=144 * 1024 // 16 // 384)
    assert P["filled"] == 1 and P["max_slots"] == 16 <= 144 * 1024 // 16 // 384 == 24
    assert plan_filled(86, 39063, 256, 0, 8, 1, phased=True, limit=144 * 1024 // 16 // 512 - 3)["refused"] == 1      # (15: one short)


# ---- every check rejects a list that breaks it -----------------------------------------------------------------------------------------------
def small():
    return plan_filled(8 * 3 + 6, 300, 64, 0, 8, 1, phased=True)      # r = 6: a 4 x 2 row and a 2 x 4 row


def leftover(P, stride):
    return np.flatnonzero(P["segs"][:, 6] == stride)


def test_checks_accept_the_small_list():
    P = small()
    for check in CHECKS + [check_xcd_ticks]:
        check(P)


def test_cover_rejects_a_leftover_pair_dealt_twice():
    P = small()
    i = leftover(P, 4)[0]
    dup = P["segs"][i].copy()
    dup[3] = 1
    P["segs"] = np.insert(P["segs"], i + 1, dup, axis=0)
    with pytest.raises(AssertionError, match="exactly once"):
        check_cover(P)


def test_ticks_reject_a_row_with_the_wrong_stride():
    P = small()
    P["segs"][leftover(P, 2), 6] = 1      # the 4 x 2 row strided like the full groups
    with pytest.raises(AssertionError, match="one unit per tick"):
        check_ticks(P)


def test_ticks_reject_a_member_one_tick_ahead():
    P = small()
    blk = P["segs"][leftover(P, 4)[0], 0]
    P["segs"][P["segs"][:, 0] == blk, 7] += 1
    with pytest.raises(AssertionError, match="one unit per tick"):
        check_ticks(P)


def test_ticks_reject_a_member_on_another_query_tile():
    P = small()
    i = leftover(P, 2)[0]
    P["segs"][i, 1] += 1 if P["segs"][i, 1] + 1 < P["nqt"] else -1
    with pytest.raises(AssertionError, match="one unit per tick"):
        check_ticks(P)


def test_slots_reject_two_owners_and_descending_tiles():
    P = small()
    s = P["segs"]
    i = leftover(P, 4)[0]
    other = np.flatnonzero((s[:, 0] != s[i, 0]) & (s[:, 1] == s[i, 1]))[0]
    s[other, 4] = s[i, 4]; s[other, 5] = 0
    with pytest.raises(AssertionError):
        check_slots(P)
    P = small()
    s = P["segs"]
    cont = np.flatnonzero(s[:, 5] == 0)[0]
    s[cont, 2] = 0
    with pytest.raises(AssertionError, match="ascend"):
        check_slots(P)


def test_clocks_reject_a_clock_that_runs_backwards():
    P = small()
    s = P["segs"]
    i = np.flatnonzero(s[1:, 0] == s[:-1, 0])[0] + 1
    s[i, 7] = s[i - 1, 7]
    with pytest.raises(AssertionError):
        check_clocks(P)


def test_xcd_rejects_a_member_on_another_xcd():
    P = small()
    s = P["segs"]
    blk = s[leftover(P, 4)[0], 0]
    s[s[:, 0] == blk, 0] = blk + 1 if blk % 8 != 7 else blk - 1
    with pytest.raises(AssertionError):
        check_xcd(P)


def test_cuts_reject_a_member_cut_one_segment_late():
    P = small()
    assert len(P["clocks"]) >= 2
    s = P["segs"]
    off = np.searchsorted(s[:, 0], np.arange(P["G"] + 1))
    blk = next(b for b in range(P["G"]) if 0 < P["bounds"][0][b] and off[b] + P["bounds"][0][b] + 1 < off[b + 1])
    P["bounds"][0][blk] += 1
    with pytest.raises(AssertionError, match="cut at one clock"):
        check_cuts(P)


def test_idle_rejects_the_old_lists_count_and_xcd_ticks_a_long_range():
    P = small()
    P["idle"] = expected_idle(P, filled=False)
    with pytest.raises(AssertionError):
        check_idle(P)
    P = small()
    s = P["segs"]
    last = s[:, 9] // 32 == P["G"] // 8 - 1      # the last cluster runs more ticks longer than the panels' rounding allows
    s[last, 7] += -(-P["nbt"] // P["panel"]) + 1
    with pytest.raises(AssertionError):
        check_xcd_ticks(P)
