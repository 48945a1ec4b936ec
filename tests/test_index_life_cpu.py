"""tests/index_life.py without a GPU: what the committed lives reach, from the generator alone, and the driver against fake indexes built
from numpy and the oracle -- the clean fake passes every life, and each of three planted faults (FakeIndex) is caught at the step where it
first changes an answer.

The pair table leaves out what cannot exist: an excluding reader needs a row-group table that covers the rows, so its most recent mutator is
never an append, a reset or an add_from (index_life.NO_GROUPS_AFTER) -- those are the `excluding_after_add` refusal instead."""
import pytest

import index_life as L

LIVES = L.committed_lives()
N_SINGLE = len(L.PLAIN_SEEDS) + len(L.STEERED_SEEDS)


def test_the_seed_list_is_what_the_suite_runs():
    assert len(L.PLAIN_SEEDS) == 12 and len(L.STEERED_SEEDS) == 4 and len(L.PAIR_SEEDS) == 2
    assert len(LIVES) == 20 and len({head["seed"] for head, _ in LIVES}) == 20
    for a, b in L.PAIR_SEEDS:
        assert L.generate(a, big=False, length=L.PAIR_LENGTH)[0]["D"] != L.generate(b, big=False, length=L.PAIR_LENGTH)[0]["D"]
    assert L.generate(101) == L.generate(101)          # a seed is a life


def test_every_mutator_reader_pair_occurs():
    pairs, _ = L.coverage(LIVES)
    missing = sorted(set(L.possible_pairs(steered=True)) - pairs)
    assert not missing, f"{len(missing)} (most recent mutator, reader) pairs never occur: {missing[:10]}"
    # steering calls only in the lives flagged for them: fp32_pinned is sticky
    for head, ops in LIVES:
        assert head["steered"] or not any(op["kind"] in L.STEERING for op in ops)


@pytest.mark.parametrize("condition", L.CONDITIONS)
def test_some_life_reaches(condition):
    assert condition in L.coverage(LIVES)[1]


def test_the_lives_cover_the_sizes_and_stay_small():
    seen = {n: set() for n in ("D", "C", "P", "metric", "nq", "k", "chunk", "fp16")}
    for head, ops in LIVES:
        assert len(ops) <= L.MAX_OPS and L.max_rows((head, ops)) <= L.MAX_ROWS, head
        for n in ("D", "C", "P", "metric"):
            seen[n].add(head[n])
        for op in ops:
            if op["kind"] in L.READERS and "nq" in op:
                seen["nq"].add(op["nq"])
                seen["k"] |= {op["k"]} if "k" in op else set(op["ks"])
            if op["op"] == "add":
                seen["chunk"].add(op["n"])
            if op["op"] == "set_fp16":
                seen["fp16"].add(op["mode"])
    assert seen["D"] == set(L.DS) and seen["C"] == set(L.CS) and seen["P"] == {0, L.P_COUNTS} and seen["metric"] == {0, 1}
    assert seen["nq"] >= set(L.NQS) and seen["k"] >= set(L.KS) and seen["fp16"] == {0, 1, 2}
    assert seen["chunk"] >= {1, 5, 31, 32, 33, 255, 256, 257, 1000, 3000}
    assert any(L.max_rows(life) >= 4096 for life in LIVES) and any(op["op"] == "reset" and op["n"] == 10 for _, ops in LIVES for op in ops)


def _run(i, make):
    if i < N_SINGLE:
        return L.run_life(make, LIVES[i])
    j = N_SINGLE + 2 * (i - N_SINGLE)
    return L.run_interleaved(make, LIVES[j:j + 2])


@pytest.mark.parametrize("i", range(N_SINGLE + len(L.PAIR_SEEDS)))
def test_the_clean_fake_passes(i):
    make, fired = L.fake_factory(None)
    _run(i, make)
    assert not fired


@pytest.mark.parametrize("fault", L.FAULTS)
def test_a_planted_fault_is_caught_at_its_step(fault):
    """The driver fails in at least one life, and wherever it fails, at the first step at which the fault changed an answer."""
    caught = 0
    for life in LIVES[:N_SINGLE]:
        clock = {}

        class Clocked(L.Env):
            def step(self, i):
                clock["step"] = i

        make, fired = L.fake_factory(fault, clock)
        try:
            L.run_life(make, life, Clocked())
        except L.LifeFailure as e:
            assert fired and e.step == fired[0], (life[0]["seed"], e.step, fired[:3])
            assert f"life {life[0]['seed']}, step {e.step}" in str(e) and "since the last reset" in str(e)
            caught += 1
        else:
            assert not fired, f"life {life[0]['seed']}: the fault changed the answers of steps {fired[:5]} and no check noticed"
    assert caught >= 1


def test_a_life_prints_without_running(capsys):
    import runpy
    import sys
    argv = sys.argv
    sys.argv = ["index_life.py", "103", "7"]
    try:
        runpy.run_module("index_life", run_name="__main__")
    finally:
        sys.argv = argv
    out = capsys.readouterr().out
    assert out.startswith("life {'seed': 103") and "  6  " in out and "  7  " not in out
