"""Which indexes get the re-rank's row copy of the bank (hb_index_set_rerank_copy; csrc/hbird_calibrate.cpp, hb_rerank_copy_choose) behind its
replay entry, fed with imagined banks and devices: no GPU.  Every figure follows from the rule's constants -- banks of up to 16e9 bytes, the
three copies (fp32 tiles, fp16 tiles at half of them, the rows) within 55 % of the device, free memory above the copy plus the larger of 1/16
of the device and 2 GiB -- none is measured."""
import pytest

from hbird_mi import _lib

GB, GIB = 10 ** 9, 1 << 30
DEVICE = 288 * GB
AUTO, ALWAYS, NEVER = 0, 1, 2


def choose(rows=None, d=768, setting=AUTO, bank=None, need=None, free=None, total=DEVICE):
    """-> 1 (the copy is made) or 0 for a bank of rows x d (d a multiple of 32: a row of the copy is a row of the tiles); all of the device free."""
    bank = rows * d * 4 if bank is None else bank
    need = bank if need is None else need
    rc = _lib.lib().hb_rerank_copy_replay(setting, bank, need, total if free is None else free, total)
    assert rc in (0, 1), rc
    return rc


def test_banks_of_up_to_16_gb_get_the_copy_on_an_empty_288_gb_device():
    assert choose(300_000) == 1                  # 0.92 GB
    assert choose(5_200_000) == 1                # 15.97 GB
    assert choose(5_300_000) == 0                # 16.28 GB
    assert choose(10_000_000) == 0               # 30.7 GB: the flagship bank holds 1.5 x the bank, not 2.5 x
    assert choose(bank=16 * GB) == 1 and choose(bank=16 * GB + 4) == 0


def test_the_three_copies_stay_within_55_percent_of_the_device():
    bank = 5_200_000 * 768 * 4
    three = bank + bank // 2 + bank
    assert choose(5_200_000, total=64 * GIB) == 0                 # 39.9 GB of 68.7: 58 %
    fits = -(-three // 55) * 100                                  # the smallest total (a multiple of 100) with total / 100 * 55 >= the three copies
    assert fits // 100 * 55 >= three > (fits - 100) // 100 * 55
    assert choose(5_200_000, total=fits) == 1
    assert choose(5_200_000, total=fits - 100) == 0


@pytest.mark.parametrize("total, rows", [(DEVICE, 5_200_000), (DEVICE, 300_000), (24 * GIB, 300_000)])
def test_free_memory_must_exceed_the_copy_plus_the_spare(total, rows):
    need = rows * 768 * 4
    spare = max(total // 16, 2 * GIB)
    assert (spare == 2 * GIB) == (total == 24 * GIB)              # both arms of the maximum are walked
    assert choose(rows, free=need + spare - 1, total=total) == 0
    assert choose(rows, free=need + spare, total=total) == 0      # (strictly above)
    assert choose(rows, free=need + spare + 1, total=total) == 1


def test_the_explicit_settings_ask_nothing():
    for rows, free in ((300_000, None), (10_000_000, None), (27_700_000, 0), (300_000, 0)):
        assert choose(rows, setting=ALWAYS, free=free) == 1
        assert choose(rows, setting=NEVER, free=free) == 0


def test_bad_arguments_are_refused():
    L = _lib.lib()
    b = 300_000 * 768 * 4
    assert L.hb_rerank_copy_replay(0, b, b, DEVICE, DEVICE) == 1
    assert L.hb_rerank_copy_replay(-1, b, b, DEVICE, DEVICE) < 0
    assert L.hb_rerank_copy_replay(3, b, b, DEVICE, DEVICE) < 0
    assert L.hb_rerank_copy_replay(0, 0, b, DEVICE, DEVICE) < 0
    assert L.hb_rerank_copy_replay(0, b, 0, DEVICE, DEVICE) < 0
    assert L.hb_rerank_copy_replay(0, b, b, DEVICE, 0) < 0
    assert L.hb_rerank_copy_replay(0, b, b, DEVICE + 1, DEVICE) < 0      # more free than there is
