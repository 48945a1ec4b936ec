"""The kNN launcher's shape plan (csrc/hbird_calibrate.cpp: hb_knn_plan_shape / _clusters / _kernel) without a GPU, through
hb_knn_plan_replay.  Which kernel a search runs on, on pools or lists, with which clusters, phased or not, is host arithmetic over the
search's sizes and the index's override fields: a slip there is a silent slowdown that the parity tests cannot see (every path returns
the same bits).  Every row pins one rule; the expected values are written out by hand from the launcher's rules as they stood when the
plan was still inline in hb_launch_knn, each threshold taken from both sides by the smallest step (one bank tile or one query tile).

The base shape: D = 384 (48 fp32 stages per tile, 24 fp16 ones), 256 workgroups, and 65,536 queries = 256 query tiles, so that
"stages per workgroup" is simply bank tiles x 48."""
import ctypes

import pytest

from hbird_mi import _lib

IN = ["f16", "wide_first", "esc", "ceil", "k", "nq", "ntotal", "g8", "dp", "dp16", "num_cu", "force_G", "force_panel", "force_cq", "force_cb",
      "variant", "small_limit", "phases_on", "xcd_balance", "xcd_share", "sync_lag", "cl_state", "cl_choice", "sched_G"]
OUT = ["kc", "wide", "klw", "small_pools", "nqt", "nbt", "G", "fam", "balance", "cq", "cb", "auto_cluster", "panel", "phased", "xs", "lag",
       "kernel", "sched_G", "small"]
BASE = dict(f16=0, wide_first=0, esc=0, ceil=0, k=30, nq=65536, ntotal=196 * 256, g8=48, dp=384, dp16=384, num_cu=256, force_G=0, force_panel=0,
            force_cq=0, force_cb=0, variant=0, small_limit=0, phases_on=1, xcd_balance=0, xcd_share=0, sync_lag=-1, cl_state=0, cl_choice=1, sched_G=0)
D40 = dict(g8=6, dp=48, dp16=64)      # D = 40: six stages per tile, no multiple of four
# kernels (hb_knn_kernel): the LDS-staged ones, and the register-resident forms BD + 4 wide + 2 clustered + 1 small
F16, LISTS, LISTS_COLD, POOLS, LISTS_CL, POOLS_CL, CEIL, BD = 0, 1, 2, 3, 4, 5, 6, 8
BD_SMALL, BD_CL, BD_POOLS, BD_POOLS_SMALL, BD_POOLS_CL = BD + 1, BD + 2, BD + 4, BD + 5, BD + 6


def plan(**kw):
    assert not set(kw) - set(IN), set(kw) - set(IN)
    v = dict(BASE, **kw)
    a = (ctypes.c_int64 * len(IN))(*[v[n] for n in IN])
    o = (ctypes.c_int64 * len(OUT))()
    assert _lib.lib().hb_knn_plan_replay(a, len(IN), o, len(OUT)) == 0
    return dict(zip(OUT, [int(x) for x in o]))


def tiles(n):
    return dict(ntotal=n * 256)


CASES = [
    # ---- lists or small pools (k <= 32 on a small shape: pools from k = 8) ----
    ("k=7 keeps the sorted LDS lists", dict(k=7), dict(small_pools=0, wide=0, kc=7, klw=32, phased=0, small=1, kernel=BD_SMALL)),
    ("k=8 is the first small-pool k", dict(k=8), dict(small_pools=1, wide=1, kc=8, klw=192, phased=1, small=1, kernel=BD_POOLS_SMALL)),
    ("k=32 is the last small-pool k", dict(k=32), dict(small_pools=1, wide=1, kc=32, klw=192, kernel=BD_POOLS_SMALL)),
    ("k=33 is a pool search of its own (k > HB_KL), not a small-pool one", dict(k=33), dict(small_pools=0, wide=1, kc=33, klw=192, small=1, kernel=BD_POOLS_SMALL)),
    ("variant 4 (LDS-staged kernels only) has no small pools", dict(variant=4), dict(small_pools=0, wide=0, klw=32, kernel=LISTS_COLD)),
    ("variant 6 keeps the lists on the register-resident kernel", dict(variant=6), dict(small_pools=0, wide=0, kernel=BD_SMALL)),
    ("variant 3 takes the small pools like the default", dict(variant=3), dict(small_pools=1, kernel=BD_POOLS_SMALL)),
    ("g8 % 4 != 0 (D = 40): no register-resident kernel, no small pools", D40, dict(small_pools=0, wide=0, kernel=LISTS_COLD)),
    ("a forced cluster with cq > 1 has no small pools", dict(force_cq=2, force_cb=1), dict(small_pools=0, wide=0, cq=2, cb=1, lag=16, xs=0, small=0, kernel=BD_CL)),
    ("the fp16 candidate pass is no small-pool search", dict(f16=1), dict(small_pools=0, wide=1, kc=64, klw=192, fam=1, kernel=F16, phased=1)),
    ("a ceiling pass is no small-pool search", dict(ceil=1), dict(small_pools=0, wide=1, kc=30, klw=192, kernel=CEIL)),
    # ---- pool capacity: at least 2 kc and kc + 128, in 64s, at most HB_POOL_MAX = 512 ----
    ("klw for kc = 8", dict(k=8), dict(kc=8, klw=192)),
    ("klw for kc = 64", dict(f16=1, k=30), dict(kc=64, klw=192)),
    ("klw for kc = 192", dict(f16=1, k=96), dict(kc=192, klw=384)),
    ("klw for kc = 256: HB_POOL_MAX", dict(f16=1, k=128), dict(kc=256, klw=512)),
    ("klw for an fp32 k = 256: HB_POOL_MAX", dict(k=256), dict(kc=256, klw=512, wide=1)),
    # ---- kc = 2k rounded up to 8, at least 64 ----
    ("kc for k = 33 is 72, not 128", dict(f16=1, k=33), dict(kc=72, klw=256)),
    ("kc for k = 128", dict(f16=1, k=128), dict(kc=256)),
    ("the second fp16 pass takes the widest list", dict(f16=1, esc=1), dict(kc=256, klw=512, phased=0)),
    ("a wide-first search takes the widest list", dict(f16=1, wide_first=1), dict(kc=256, klw=512, phased=1)),
    # ---- the stage bounds (bank tiles x 48 stages) ----
    ("small_shape: 2,499 tiles = 119,952 stages", tiles(2499), dict(small_pools=1, small=1, kernel=BD_POOLS_SMALL)),
    ("small_shape: 2,500 tiles = 120,000 stages", tiles(2500), dict(small_pools=0, wide=0, small=1, kernel=BD_SMALL)),
    ("small (lists): 8,333 tiles = 399,984 stages", tiles(8333), dict(small=1, kernel=BD_SMALL)),
    ("small (lists): 8,334 tiles = 400,032 stages", tiles(8334), dict(small=0, kernel=BD)),
    ("small (k > 32): 1,041 tiles = 49,968 stages", dict(k=64, **tiles(1041)), dict(small=1, kernel=BD_POOLS_SMALL)),
    ("small (k > 32): 1,042 tiles = 50,016 stages", dict(k=64, **tiles(1042)), dict(small=0, kernel=BD_POOLS)),
    ("a caller's small_limit 100,000: 2,083 tiles = 99,984", dict(small_limit=100000, **tiles(2083)), dict(small_pools=1, small=1, kernel=BD_POOLS_SMALL)),
    ("a caller's small_limit 100,000: 2,084 tiles = 100,032", dict(small_limit=100000, **tiles(2084)), dict(small_pools=0, small=0, kernel=BD)),
    ("a caller's small_limit 500,000 moves `small` ...", dict(small_limit=500000, **tiles(8334)), dict(small=1, kernel=BD_SMALL)),
    ("... but small_shape stays at 120,000", dict(small_limit=500000, **tiles(2500)), dict(small_pools=0)),
    ("... and k > 32 at 50,000", dict(small_limit=500000, k=64, **tiles(1042)), dict(small=0)),
    # ---- calibrated shares ----
    ("balance: 624 tiles = 29,952 stages", tiles(624), dict(balance=0)),
    ("balance: 625 tiles = 30,000 stages", tiles(625), dict(balance=1)),
    ("balance needs G % 8 == 0", dict(force_G=250, **tiles(625)), dict(G=250, balance=0)),
    ("equal shares: no balance", dict(xcd_balance=1, **tiles(625)), dict(balance=0)),
    ("given shares apply at any size", dict(xcd_balance=2), dict(balance=1)),
    # ---- the fp16 candidate kernel's clusters: from 70,000 stages of dp16 / 16 = 24 per tile ----
    ("fp16 clusters: 2,916 tiles = 69,984 stages", dict(f16=1, **tiles(2916)), dict(cq=1, cb=1, xs=0, lag=0, auto_cluster=0)),
    ("fp16 clusters: 2,917 tiles = 70,008 stages", dict(f16=1, **tiles(2917)), dict(cq=8, cb=1, xs=1, lag=16, auto_cluster=0, kernel=F16)),
    ("fp16 clusters only on variant 0", dict(f16=1, variant=3, **tiles(2917)), dict(cq=1, cb=1)),
    # ---- the fp32 kernel's automatic clusters: from 1,000,000 stages, and as measured ----
    ("fp32 clusters: 20,833 tiles = 999,984 stages", tiles(20833), dict(cq=1, cb=1, auto_cluster=0, kernel=BD)),
    ("fp32 clusters: 20,834 tiles, measuring with", tiles(20834), dict(cq=2, cb=4, auto_cluster=1, xs=0, lag=16, kernel=BD_CL)),
    ("fp32 clusters: measuring without", dict(cl_state=1, **tiles(20834)), dict(cq=1, cb=1, auto_cluster=1, kernel=BD)),
    ("fp32 clusters: decided, kept", dict(cl_state=2, cl_choice=1, **tiles(20834)), dict(cq=2, cb=4, auto_cluster=1)),
    ("fp32 clusters: decided, dropped", dict(cl_state=2, cl_choice=0, **tiles(20834)), dict(cq=1, cb=1, auto_cluster=1)),
    ("fp32 clusters with equal shares: nothing measures, they stay on", dict(xcd_balance=1, cl_state=1, **tiles(20834)), dict(cq=2, cb=4, auto_cluster=1)),
    ("fp32 clusters with equal shares: a decision holds all the same", dict(xcd_balance=1, cl_state=2, cl_choice=0, **tiles(20834)), dict(cq=1, cb=1)),
    ("fp32 clusters: not for pools", dict(k=64, **tiles(20834)), dict(cq=1, cb=1, auto_cluster=0)),
    ("fp32 clusters: not beside the LDS-staged kernel's shapes (D = 40)", dict(D40, ntotal=170000 * 256), dict(cq=1, cb=1, auto_cluster=0, kernel=LISTS)),
    # ---- a shape that does not fit falls back to 1 x 1 ----
    ("G % (8 cq cb) != 0", dict(force_cq=2, force_cb=4, force_G=96), dict(G=96, cq=1, cb=1, lag=0)),
    ("the same shape where it fits", dict(force_cq=2, force_cb=4, force_G=128), dict(G=128, cq=2, cb=4, lag=16)),
    ("fewer pairs than workgroups", dict(force_cq=2, force_cb=2, nq=256, **tiles(100)), dict(cq=1, cb=1, sched_G=100)),
    ("a ceiling pass runs unclustered on the CEIL kernel, whatever is forced", dict(ceil=1, force_cq=2, force_cb=2), dict(cq=1, cb=1, kernel=CEIL, wide=1, phased=1)),
    ("the LDS-staged clustered kernels (variant 4)", dict(variant=4, force_cq=2, force_cb=2), dict(kernel=LISTS_CL)),
    ("... and for pools", dict(variant=4, k=64, force_cq=2, force_cb=2), dict(kernel=POOLS_CL)),
    ("... and unclustered pools", dict(variant=4, k=64), dict(kernel=POOLS)),
    # ---- XCD-level sharing of the query tiles, the sync lag ----
    ("xs automatic: on for the fp16 kernel's clusters", dict(f16=1, xcd_share=0, **tiles(2917)), dict(xs=1)),
    ("xs 1: off", dict(f16=1, xcd_share=1, **tiles(2917)), dict(xs=0)),
    ("xs 2: on", dict(f16=1, xcd_share=2, **tiles(2917)), dict(xs=1)),
    ("xs automatic: off for the fp32 kernel's clusters", dict(force_cq=2, force_cb=1, xcd_share=0), dict(xs=0)),
    ("xs 2: on for them too", dict(force_cq=2, force_cb=1, xcd_share=2), dict(xs=1)),
    ("xs needs clusters", dict(xcd_share=2), dict(xs=0)),
    ("a caller's sync lag", dict(force_cq=2, force_cb=1, sync_lag=5), dict(lag=5)),
    ("sync lag 0 turns the sync off", dict(force_cq=2, force_cb=1, sync_lag=0), dict(lag=0)),
    # ---- phases: pools of a caller's search only ----
    ("phased: a caller's pool search", dict(k=64), dict(phased=1)),
    ("phased: not the second fp16 pass", dict(f16=1, esc=1), dict(phased=0)),
    ("phased: not the fp32 search of what is left", dict(k=64, esc=2), dict(phased=0)),
    ("phased: switched off", dict(k=64, phases_on=0), dict(phased=0)),
    ("phased: never the lists", dict(k=7), dict(phased=0)),
    # ---- the grid ----
    ("a partial last query tile, a partial last bank tile", dict(nq=257, ntotal=257), dict(nqt=2, nbt=2, G=256, sched_G=4)),
    ("a caller's panel", dict(force_panel=7), dict(panel=7)),
    # ---- `small` divides by the WORK LIST's workgroups: with fewer pairs than workgroups a list has one workgroup per pair, so 100 pairs are
    # 48 stages per workgroup (not 100 / 256 = 0) ----
    ("sc.G < G: 48 stages are not below a limit of 48", dict(nq=256, small_limit=48, **tiles(100)), dict(G=256, sched_G=100, small=0, small_pools=0, kernel=BD)),
    ("sc.G < G: ... and below one of 49", dict(nq=256, small_limit=49, **tiles(100)), dict(G=256, sched_G=100, small=1, small_pools=1, kernel=BD_POOLS_SMALL)),
    ("a cached list of other workgroups decides by its own count", dict(nq=256, small_limit=48, sched_G=4, **tiles(6)), dict(sched_G=4, small=0)),
    ("... 6 pairs on 6 workgroups", dict(nq=256, small_limit=49, sched_G=6, **tiles(6)), dict(sched_G=6, small=1)),
]


@pytest.mark.parametrize("rule,inputs,expect", CASES, ids=[c[0] for c in CASES])
def test_plan_rule(rule, inputs, expect):
    got = plan(**inputs)
    assert {n: got[n] for n in expect} == expect, (rule, got)


def test_fresh_work_list_has_the_workgroups_the_plan_assumes():
    """hb_knn_plan_replay's default for the work list's workgroup count is what hb_build_schedule gives a fresh list: held equal here."""
    L = _lib.lib()
    for nq, nb, G in ((256, 100, 256), (257, 1, 256), (512, 196, 256), (256, 6, 4), (256, 300, 304)):
        stats = (ctypes.c_int64 * 8)()
        assert L.hb_schedule_plan(nq // 256 + (nq % 256 > 0), nb, G, 0, 384, 1, 1, None, 0, stats) == 0
        assert plan(nq=nq, force_G=G, **tiles(nb))["sched_G"] == stats[0]


def test_bad_arguments():
    L = _lib.lib()
    a = (ctypes.c_int64 * len(IN))(*[BASE[n] for n in IN])
    o = (ctypes.c_int64 * len(OUT))()
    assert L.hb_knn_plan_replay(None, len(IN), o, len(OUT)) < 0
    assert L.hb_knn_plan_replay(a, len(IN) - 2, o, len(OUT)) < 0
    assert L.hb_knn_plan_replay(a, len(IN), o, len(OUT) - 1) < 0
    a[4] = 0      # k
    assert L.hb_knn_plan_replay(a, len(IN), o, len(OUT)) < 0
