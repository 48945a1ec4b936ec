"""The automatic state of the fp16 setting (HB_FP16_AUTO, what a new index starts in): which exact searches take the certified fp16 screen.
The decision is plain host code (csrc/hbird_calibrate.cpp, hb_screen_choose) behind a replay entry, fed here with imagined searches: no GPU.
(The host-only sanitizer build exports it too: `make -C csrc plan_asan`, then HBIRD_HIP_LIB=<that library> HBIRD_PLAN_ONLY=1 and -k "not null_handle": the report entry lives in the full library.)"""
import ctypes

import pytest

from hbird_mi import _lib

AUTO = 3
FP32, SCREEN = 0, 1
WHY = {name: i for i, name in enumerate(["explicit_fp32", "explicit_fp16", "auto", "k", "ceiling", "work", "small", "pinned", "env", "memory",
                                         "overflow", "adaptive"])}
GB = 10 ** 9
DEVICE = 288 * GB


def _stages(rows, nq, d, workgroups=256):
    """k8 stages per workgroup as the launcher counts them: (query tiles x bank tiles) // workgroups x (D padded to 16) / 8."""
    return (-(-nq // 256)) * (-(-rows // 256)) // workgroups * ((d + 15) // 16 * 16 // 8)


def choose(setting=AUTO, pinned=0, env_off=0, k=30, ceiling=0, rows=10_000_000, nq=21_904, d=768, stages=None, overflow=0, have_copy=0,
           declined=0, free=None, total=DEVICE):
    """-> (screen?, reason) for one imagined search; the bank's capacity is its row count, the device is empty but for the bank."""
    bank = rows * d * 4
    copy = rows * ((d + 127) // 128 * 128) * 2
    free = total - bank if free is None else free
    why = ctypes.c_int(-1)
    rc = _lib.lib().hb_exact_screen_replay(setting, pinned, env_off, k, ceiling, rows, nq, d, _stages(rows, nq, d) if stages is None else stages,
                                           overflow, have_copy, declined, free, total, bank, copy, ctypes.byref(why))
    assert rc in (0, 1), rc
    return rc, why.value


def test_the_headline_shape_takes_the_screen_and_a_small_search_does_not():
    assert choose() == (SCREEN, WHY["auto"])                                          # 10 M x 768, 21,904 queries, k = 30
    assert choose(k=90) == (SCREEN, WHY["auto"])
    assert choose(rows=2_000_000) == (SCREEN, WHY["auto"])                            # 252 k stages per workgroup
    # smoke()'s shape, a bench-sized small bank, and a search just under the big-search bound: the fp32 kernel, as before
    assert choose(rows=5000, d=384, nq=392) == (FP32, WHY["work"])
    assert choose(rows=300_000, d=384, nq=12_544) == (FP32, WHY["small"])
    assert _stages(238_000, 21_904, 768) < 30000 <= _stages(239_000, 21_904, 768)
    assert choose(rows=238_000) == (FP32, WHY["small"])
    assert choose(rows=239_000) == (SCREEN, WHY["auto"])
    assert choose(stages=29_999) == (FP32, WHY["small"]) and choose(stages=30_000) == (SCREEN, WHY["auto"])


def test_what_keeps_an_automatic_index_on_the_fp32_kernel():
    assert choose(k=128) == (SCREEN, WHY["auto"])
    assert choose(k=129) == (FP32, WHY["k"])
    assert choose(k=256, ceiling=1) == (FP32, WHY["k"]) and choose(k=100, ceiling=1) == (FP32, WHY["ceiling"])    # a later pass of a search with k > 256
    assert choose(pinned=1) == (FP32, WHY["pinned"])           # set_variant / _tuning / _cluster / _cluster_sharing / _xcd_weights / _search_options
    assert choose(env_off=1) == (FP32, WHY["env"])             # HBIRD_EXACT_SCREEN=0
    assert choose(setting=0) == (FP32, WHY["explicit_fp32"])   # the caller asked for the fp32 kernel
    assert choose(overflow=1) == (FP32, WHY["overflow"])
    assert choose(rows=4000, nq=10 ** 7) == (FP32, WHY["work"])                       # fewer than 4,096 rows
    # state 2's bound: rows x queries x D >= 1.5e10 x (k' / 64)^2 -- k = 128 means k' = 256: sixteen times the work of k = 30
    assert choose(rows=1_000_000, nq=300, d=768, k=128, stages=10 ** 6) == (FP32, WHY["work"])
    assert choose(rows=1_000_000, nq=300, d=768, k=30, stages=10 ** 6) == (SCREEN, WHY["auto"])


def test_the_copy_only_where_it_leaves_the_device_room():
    bank, copy = 10_000_000 * 768 * 4, 10_000_000 * 768 * 2
    floor = max(DEVICE // 16, 2 << 30)
    assert choose(free=copy + floor + 1) == (SCREEN, WHY["auto"])
    assert choose(free=copy + floor) == (FP32, WHY["memory"])                         # free memory must stay ABOVE the copy + the reserve
    assert choose(free=0) == (FP32, WHY["memory"])
    # fp32 tiles + fp16 tiles within 55 % of the device: a 64 GB device takes the 10 M x 768 bank (30.7 GB) but not its copy beside it
    assert bank + copy > 64 * GB // 100 * 55
    assert choose(total=64 * GB, free=64 * GB - bank) == (FP32, WHY["memory"])
    assert choose(rows=27_700_000) == (SCREEN, WHY["auto"])                           # the whole ADE20K bank: 85 + 42.5 GB of 288
    assert choose(rows=40_000_000, free=DEVICE) == (FP32, WHY["memory"])              # 123 + 61 GB: beyond 55 %
    # a small device's reserve is 2 GiB, not 1/16 of it
    small_bank, small_copy = 1_000_000 * 768 * 4, 1_000_000 * 768 * 2
    assert choose(rows=1_000_000, total=16 * GB, free=small_copy + (2 << 30) + 1) == (SCREEN, WHY["auto"])
    assert choose(rows=1_000_000, total=16 * GB, free=small_copy + (2 << 30)) == (FP32, WHY["memory"])
    assert small_bank + small_copy <= 16 * GB // 100 * 55
    # "no room at this capacity" is remembered (memory is not asked again), and a copy that exists is used whatever is free now
    assert choose(declined=1) == (FP32, WHY["memory"])
    assert choose(have_copy=1, free=0) == (SCREEN, WHY["auto"])
    assert choose(have_copy=1, declined=1, pinned=1) == (FP32, WHY["pinned"])


@pytest.mark.parametrize("setting", [1, 2])
def test_the_explicit_states_keep_their_rules(setting):
    """hb_index_set_fp16(1 | 2): what pins, the environment, the big-search bound and memory do not apply (no memory is the search's error there)."""
    for kw in ({}, {"pinned": 1}, {"env_off": 1}, {"free": 0}, {"declined": 1}, {"stages": 10}, {"total": 64 * GB}, {"overflow": 1}):
        assert choose(setting=setting, **kw) == (SCREEN, WHY["explicit_fp16"]), kw      # (an overflowing bank is found out by the conversion itself)
    assert choose(setting=setting, k=129) == (FP32, WHY["k"])
    assert choose(setting=setting, ceiling=1) == (FP32, WHY["ceiling"])
    small = dict(rows=5000, d=384, nq=392)
    assert choose(setting=setting, **small) == ((SCREEN, WHY["explicit_fp16"]) if setting == 1 else (FP32, WHY["work"]))
    assert choose(setting=setting, rows=4000, nq=10 ** 7)[0] == (SCREEN if setting == 1 else FP32)


def test_bad_arguments_are_refused():
    why = ctypes.c_int(0)
    L = _lib.lib()
    assert L.hb_exact_screen_replay(4, 0, 0, 30, 0, 1000, 10, 64, 1, 0, 0, 0, 1, 1, 1, 1, ctypes.byref(why)) < 0
    assert L.hb_exact_screen_replay(AUTO, 0, 0, 0, 0, 1000, 10, 64, 1, 0, 0, 0, 1, 1, 1, 1, ctypes.byref(why)) < 0
    assert L.hb_exact_screen_replay(AUTO, 0, 0, 30, 0, 1000, 10, 64, 1, 0, 0, 0, 1, 1, 1, 1, None) < 0


def test_last_search_path_rejects_a_null_handle_and_null_outputs():
    """hb_last_search_path validates its pointers before it reads the index (error code + hb_last_error, never a dereference)."""
    L = _lib.lib()
    path, why = ctypes.c_int(0), ctypes.c_int(0)
    assert L.hb_last_search_path(None, ctypes.byref(path), ctypes.byref(why)) != 0
    assert b"NULL" in L.hb_last_error()
