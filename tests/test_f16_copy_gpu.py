"""The PLAIN fp16 copy of the certified screen on its own output (HipFlatIndex.last_fp16_copy(): the raw fp16 tiles of the bank and of the
last plain pass' queries, the sticky overflow flag and its host image) against tests/f16_second_pass_refs.py: every component of every real
row equals numpy's astype(float16) of the fp32 value on bits -- one round-to-nearest-even conversion, subnormals kept, which is what the
certificate's h = 2^-11 assumes --, every padding component and row is zero, and the flag says "some finite |x| > 65504 was converted since the
last reset".  The pass scores of tests/test_f16_candidates_gpu.py see the copy only through sums of fp16-representable values (exact worlds)
or within an accumulation bound (float worlds): neither sees one bad element, a rounding mode or a flushed subnormal."""
import numpy as np
import pytest
import torch

import f16_centre_refs as CR
import f16_second_pass_refs as SR
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu
K = 10
UNFLAGGED = tuple(v for v in SR.EDGE_VALUES if v not in SR.EDGE_FLAGGED)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _index(dev, D, metric=0, fp16=1, escalation=False):
    ix = HipFlatIndex(D, metric, 0)
    ix.set_fp16(fp16)
    if fp16:
        ix.set_fp16_escalation(escalation)
    return ix


def _queries(nq, D, seed=9):
    return np.random.default_rng([seed, nq, D]).standard_normal((nq, D), dtype=np.float32)


def _clean(bad, what):
    assert not bad, f"{what}: " + " | ".join(bad.values())


def _held_answer(dev, bank, q, metric=0):
    held = _index(dev, bank.shape[1], metric, 0)
    held.add(torch.from_numpy(bank).to(dev))
    want = held.search(torch.from_numpy(q).to(dev), K)
    assert held.last_search_path()["path"] == "fp32"
    held.close()
    return want


@pytest.mark.parametrize("flagged", [False, True], ids=["in-range", "beyond-range"])
@pytest.mark.parametrize("N,D", [(1000, 40), (1000, 128), (1000, 136)], ids=lambda v: str(v))
def test_every_component_is_one_round_to_nearest_even_conversion(cuda_device, N, D, flagged):
    """1,000 x 40: a ragged last row tile (1,000 = 31 x 32 + 8) and zero-filled 8-groups up to dp16 = 128; x 128: no padding; x 136: dp16 = 256.
    Edge values at known places: +-65504, -0.0, 2^-24, 2^-25 (ties to 0), 3 x 2^-25 (ties to 2^-23), 6e-8, 1 + 2^-11 and 1 + 3 x 2^-11 (ties to
    even), +-inf and NaN (no flag); beyond-range adds 65519 (rounds to 65504, still flagged), 65520 and 1e5."""
    bank, planted = SR.copy_world(N, D, seed=D, edges=SR.EDGE_VALUES if flagged else UNFLAGGED)
    q = _queries(70, D)
    ix = _index(cuda_device, D)
    ix.add(torch.from_numpy(bank).to(cuda_device))
    got = ix.search(torch.from_numpy(q).to(cuda_device), K)
    C = ix.last_fp16_copy(queries=not flagged)
    assert C["dp16"] == (D + 127) // 128 * 128 and C["bank16"].size == 1024 * C["dp16"]
    _clean(SR.check_copy(C, bank, int(flagged)), f"{N} x {D}")
    t = CR.detile16(C["bank16"], 1024, C["dp16"])
    for r, c, v in planted:                       # (named one by one: check_copy reports the first difference only)
        assert CR.same_bits(t[r, c:c + 1].view(np.float16), SR.f16_rne([v]).view(np.float16)).all(), f"{v!r} at row {r} column {c}: {t[r, c]:#06x}"
    path = ix.last_search_path()
    if flagged:
        assert (path["path"], path["reason"]) == ("fp32", "overflow") and C["level"] == -1 and C["n"] == 0, path
        with pytest.raises(_lib.HbirdHipError, match="did not run the plain fp16 candidate pass"):
            ix.last_fp16_copy()
    else:
        assert path["path"] == "fp16_chain" and (C["n"], C["level"]) == (70, 0), (path, C["n"], C["level"])
        _clean(SR.check_copy(C, q, None, key="q16"), f"queries of {N} x {D}")
    assert _same(got, _held_answer(cuda_device, bank, q)), f"{N} x {D}: the search differs from the fp32 kernel's answer"
    ix.close()


def test_rows_appended_behind_a_copy_that_ends_inside_a_row_tile(cuda_device):
    D = 40
    first, _ = SR.copy_world(1000, D, seed=1, edges=UNFLAGGED)
    more, _ = SR.copy_world(200, D, seed=2, edges=(2.0 ** -24, -65504.0))
    q = torch.from_numpy(_queries(70, D)).to(cuda_device)
    ix = _index(cuda_device, D)
    ix.reserve(2048)
    ix.add(torch.from_numpy(first).to(cuda_device)); ix.search(q, K)
    C = ix.last_fp16_copy()
    assert C["rows"] == 1000 and C["rows"] % 32 == 8
    _clean(SR.check_copy(C, first, 0), "before the append")
    ix.add(torch.from_numpy(more).to(cuda_device))
    C = ix.last_fp16_copy(queries=False)                    # the copy is behind the bank until the next search; its query side went with the add
    assert (C["rows"], C["n"], C["level"]) == (1000, 0, -1)
    with pytest.raises(_lib.HbirdHipError, match="did not run the plain fp16 candidate pass"):
        ix.last_fp16_copy()
    ix.search(q, K)
    both = np.concatenate([first, more])
    _clean(SR.check_copy(ix.last_fp16_copy(), both, 0), "after the append")
    assert _same(ix.search(q, K), _held_answer(cuda_device, both, q.cpu().numpy()))
    ix.close()


def test_the_flag_is_sticky_until_reset_and_an_overflowing_row_sends_the_bank_to_fp32(cuda_device):
    D = 128
    first, _ = SR.copy_world(1000, D, seed=3)
    over, _ = SR.copy_world(40, D, seed=4)
    over[17, 5] = np.float32(-7.0e4)
    clean, _ = SR.copy_world(60, D, seed=5)
    qn = _queries(70, D)
    q = torch.from_numpy(qn).to(cuda_device)
    ix = _index(cuda_device, D)
    ix.reserve(2048)
    ix.add(torch.from_numpy(first).to(cuda_device)); ix.search(q, K)
    assert ix.last_search_path()["path"] == "fp16_chain" and ix.last_fp16_copy()["flag"] == 0
    ix.add(torch.from_numpy(over).to(cuda_device))
    got = ix.search(q, K)
    p = ix.last_search_path()
    assert (p["path"], p["reason"]) == ("fp32", "overflow") and ix.last_fp16_fallbacks() == 70, p
    bank = np.concatenate([first, over])
    C = ix.last_fp16_copy(queries=False)
    _clean(SR.check_copy(C, bank, 1), "after the overflowing row")
    assert _same(got, _held_answer(cuda_device, bank, qn))
    # sticky: rows within the range behind it leave the flag where it is
    ix.add(torch.from_numpy(clean).to(cuda_device)); ix.search(q, K)
    bank = np.concatenate([bank, clean])
    _clean(SR.check_copy(ix.last_fp16_copy(queries=False), bank, 1), "after clean rows behind the overflowing one")
    assert ix.last_search_path()["reason"] == "overflow"
    # reset: flag and rows are 0, on the device and on the host; the next bank starts anew
    ix.reset()
    C = ix.last_fp16_copy(queries=False)
    assert (C["rows"], C["flag"], C["flag_host"], C["bank16"].size, C["n"], C["level"]) == (0, 0, 0, 0, 0, -1)
    ix.add(torch.from_numpy(clean).to(cuda_device)); ix.search(q, K)
    assert ix.last_search_path()["path"] == "fp16_chain"
    _clean(SR.check_copy(ix.last_fp16_copy(), clean, 0), "after the reset")
    ix.close()


def test_a_capacity_change_drops_the_copy_and_the_next_search_rebuilds_it(cuda_device):
    D = 136
    bank, _ = SR.copy_world(1000, D, seed=6, edges=UNFLAGGED)
    q = torch.from_numpy(_queries(70, D)).to(cuda_device)
    ix = _index(cuda_device, D)
    with pytest.raises(_lib.HbirdHipError, match="no fp16 copy for this bank"):       # nothing searched yet
        ix.last_fp16_copy()
    ix.add(torch.from_numpy(bank).to(cuda_device))
    with pytest.raises(_lib.HbirdHipError, match="no fp16 copy for this bank"):
        ix.last_fp16_copy()
    ix.search(q, K)
    first = ix.last_fp16_copy()
    ix.reserve(5000)
    with pytest.raises(_lib.HbirdHipError, match="no fp16 copy for this bank"):
        ix.last_fp16_copy(queries=False)
    ix.search(q, K)
    C = ix.last_fp16_copy()
    _clean(SR.check_copy(C, bank, 0), "after the capacity change")
    assert np.array_equal(C["bank16"], first["bank16"]) and np.array_equal(C["q16"], first["q16"])
    # the centred form is hb_index_last_centre's; an fp32 search leaves the copy and takes the query side
    ix.set_fp16(0); ix.search(q, K)
    assert ix.last_fp16_copy(queries=False)["level"] == -1
    ix.set_fp16(1); ix.set_fp16_centre(True); ix.search(q, K)
    assert ix.fp16_centre_info()["centred"]
    with pytest.raises(_lib.HbirdHipError, match="the fp16 copy is centred"):
        ix.last_fp16_copy(queries=False)
    assert _lib.lib().hb_index_last_fp16_copy(ix._h, None, None, None) != 0 and "info is NULL" in _lib.last_error()
    ix.close()


@pytest.mark.parametrize("nq", [1, 70, 300])
def test_the_query_tiles_of_a_callers_pass(cuda_device, nq):
    """nq = 1: one query in a tile of 256 zero vectors; 70; 300: two query tiles."""
    D = 40
    bank, _ = SR.copy_world(1000, D, seed=7)
    q, _ = SR.copy_world(nq, D, seed=8, edges=(65504.0, -0.0, 2.0 ** -24, 2.0 ** -25, 1 + 2.0 ** -11) if nq > 1 else (2.0 ** -25,))
    ix = _index(cuda_device, D)
    ix.add(torch.from_numpy(bank).to(cuda_device))
    got = ix.search(torch.from_numpy(q).to(cuda_device), K)
    C = ix.last_fp16_copy()
    assert (C["n"], C["level"]) == (nq, 0) and C["q16"].size == (nq + 255) // 256 * 256 * 128
    _clean(SR.check_copy(C, q, None, key="q16"), f"{nq} queries")
    assert _same(got, _held_answer(cuda_device, bank, q))
    ix.close()


def test_the_query_tiles_of_the_second_pass_are_the_failing_queries_ascending(cuda_device):
    c = next(x for x in SR.CASES if x.name == "rounding100")
    W = SR.case_world(c)
    ix = _index(cuda_device, c.D, c.metric, 1, escalation=True)
    ix.add(torch.from_numpy(W["bank"]).to(cuda_device))
    ix.search(torch.from_numpy(W["queries"]).to(cuda_device), c.k)
    S, C = ix.last_screen_seeds(), ix.last_fp16_copy()
    assert S["n1"] >= 10 and (C["n"], C["level"]) == (S["n1"], 1)
    _clean(SR.check_copy(C, W["queries"][S["queries1"]], None, key="q16"), "the second pass' query tiles")
    _clean(SR.check_copy(C, W["bank"], 0), "the bank's tiles")
    ix.close()


def _copy_info(ix):
    """The sizes and flags alone (no tiles: the copy of a 300,000 x 768 bank is 460 MB) -> dict, or the refusal's message."""
    import ctypes
    info = (ctypes.c_int64 * 8)()
    if _lib.lib().hb_index_last_fp16_copy(ix._h, None, None, info) != 0:
        return _lib.last_error()
    return {"rows": int(info[0]), "flag": int(info[3]), "flag_host": int(info[4]), "n": int(info[5]), "level": int(info[6])}


def test_an_appended_overflowing_row_makes_the_automatic_state_drop_its_copy(cuda_device):
    """300,000 x 768 with 21,904 queries: where an index left in its automatic state takes the screen (tests/test_exact_screen_gpu.py).  A row
    with one finite value beyond the fp16 range arrives behind the copy: the next search converts it, finds the flag, runs on the fp32 kernel
    with reason `overflow`, and the automatic state -- nobody asked for this copy -- drops it; the flag's host image keeps the bank on the fp32
    kernel.  An index at set_fp16(1) keeps its copy, with the flag and its image at 1."""
    M, D, NQ, k = 300_000, 768, 21_904, 30
    g = torch.Generator(device=cuda_device); g.manual_seed(7)
    bank = torch.nn.functional.normalize(torch.randn((M, D), generator=g, device=cuda_device), dim=1)
    q = 3.0 * torch.randn((NQ, D), generator=g, device=cuda_device)
    row = bank[:1].clone(); row[0, 17] = 70_000.0
    auto, forced, held = HipFlatIndex(D, 0, 0), _index(cuda_device, D), _index(cuda_device, D, fp16=0)
    for ix in (auto, forced, held):
        ix.reserve(M + 256); ix.add(bank)
    auto.search(q, k); forced.search(q, k)
    assert auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"} and forced.last_search_path()["path"] == "fp16_chain"
    assert _copy_info(forced) == {"rows": M, "flag": 0, "flag_host": 0, "n": NQ, "level": 0}, _copy_info(forced)
    a = _copy_info(auto)                                          # (its query side may be a second pass': escalation is on)
    assert (a["rows"], a["flag"], a["flag_host"]) == (M, 0, 0) and a["level"] in (0, 1), a
    for ix in (auto, forced, held):
        ix.add(row)
    want = held.search(q, k)
    for _ in range(2):                                            # the second search decides by the host image alone: there is no copy to convert
        assert _same(auto.search(q, k), want)
        assert auto.last_search_path() == {"path": "fp32", "reason": "overflow"}
        assert "no fp16 copy for this bank" in _copy_info(auto), _copy_info(auto)
    for _ in range(2):
        assert _same(forced.search(q, k), want)
        p = forced.last_search_path()
        assert (p["path"], p["reason"]) == ("fp32", "overflow"), p
        assert _copy_info(forced) == {"rows": M + 1, "flag": 1, "flag_host": 1, "n": 0, "level": -1}, _copy_info(forced)
    # reset: the automatic index may screen again
    auto.reset(); auto.add(bank); auto.search(q, k)
    assert auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"} and _copy_info(auto)["flag"] == 0
    for ix in (auto, forced, held):
        ix.close()
