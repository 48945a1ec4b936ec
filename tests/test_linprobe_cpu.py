"""The linear probe without a GPU: the C ABI of include/hbird_hip_linprobe.h against its bindings, the documents and the build; the numpy model
of tests/linprobe_refs.py against central differences; five wrong variants of that model, each of which must fail a named check; the restated
fit on every committed world, whose generator asserts its own cap."""
import ctypes
import os
import re

import numpy as np
import pytest

import linprobe_refs as R
from hbird_mi import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_linprobe_partition", "hb_linprobe_logits", "hb_linprobe_loss_grad", "hb_linprobe_set_workspace"}
C_TYPES = {"hb_index_t*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float*": ctypes.c_void_p,
           "const float*": ctypes.c_void_p, "double*": ctypes.c_void_p}
HOST_OUT = {("hb_linprobe_partition", "seg_rows"): ctypes.POINTER(ctypes.c_int64), ("hb_linprobe_partition", "nseg"): ctypes.POINTER(ctypes.c_int),
            ("hb_linprobe_loss_grad", "loss_host"): ctypes.POINTER(ctypes.c_double), ("hb_linprobe_loss_grad", "used_host"): ctypes.POINTER(ctypes.c_int64)}


def _declarations(header):
    out = {}
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for ret, name, args in re.findall(r"^\s*(\w+)\s+(hb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.M):
        params = []
        for a in args.split(","):
            typ, arg = a.strip().rsplit(" ", 1)
            params.append((re.sub(r"\s*\*", "*", typ.strip()), arg))
        out[name] = (ret, params)
    return out


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_linprobe_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_linprobe.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_LINPROBE)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
              | set(_lib.SIGNATURES_SCREEN) | set(_lib.SIGNATURES_EXCLUDE_SCREEN) | set(_lib.SIGNATURES_BOOTSTRAP) | set(_lib.SIGNATURES_KMEANS))
    assert not NAMES & others
    inc, before = '#include "hbird_hip_linprobe.h"', '#include "hbird_hip_kmeans.h"'
    assert main.count(inc) == 1 and main.index(before) < main.index(inc) < main.rindex("#ifdef __cplusplus")
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_LINPROBE[name]
        assert ret == "int" and res is ctypes.c_int
        want = [HOST_OUT[(name, arg)] if (name, arg) in HOST_OUT else C_TYPES[typ] for typ, arg in params]
        assert want == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_linprobe_partition"][1]] == ["ntotal", "seg_rows", "nseg"]
    assert [a for _, a in decl["hb_linprobe_logits"][1]] == ["ix", "Wb", "C", "out"]
    assert [a for _, a in decl["hb_linprobe_loss_grad"][1]] == ["bank", "Wb", "C", "l2", "loss_host", "grad", "used_host", "resid_opt"]
    assert decl["hb_linprobe_set_workspace"][1] == [("int64_t", "bytes")]
    assert int(re.search(r"#define HB_LINPROBE_MAX_C (\d+)", header).group(1)) == _lib.LINPROBE_MAX_C == 256
    assert int(re.search(r"#define HB_LINPROBE_MAX_SEGS (\d+)", header).group(1)) == _lib.LINPROBE_MAX_SEGS == R.MAX_SEGS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_linprobe.h" in doc and all(n in doc for n in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "linprobe_forward_kernel" in design and "linprobe_backward_kernel" in design and "hb_linprobe_partition" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "linear_probe_fit" in readme and "not tuned" in readme and "memory_view" in readme


def test_linprobe_unit_is_built_outside_the_pinned_units_names_its_kernels_apart_and_has_no_float_atomic():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hbird_linprobe.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_linprobe.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    for units in ("KNN_UNITS", "K5_UNITS", "RES_UNITS"):
        assert "hbird_linprobe" not in re.search(rf"^{units}\s*=(.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(csrc, "hbird_linprobe.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src, flags=re.S)
    assert {"linprobe_forward_kernel", "linprobe_backward_kernel", "linprobe_reduce_kernel", "linprobe_retile_kernel", "linprobe_stage_rows_kernel"} <= set(kernels)
    assert all(k.startswith("linprobe_") for k in kernels)
    assert "rocblas" not in src.lower() and "hipblas" not in src.lower()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\batomic\w*\s*\(", code) and "unsafeAtomicAdd" not in code      # no atomic at all, so none on a float or a double
    assert "kmeans_" not in code and '#include "hbird_k5_dev.h"' in code
    assert "mfma_f32_32x32x2f32" in code and "ds_swizzle" in code


def test_linprobe_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    loss, used = ctypes.c_double(0), ctypes.c_int64(0)
    assert L.hb_linprobe_logits(None, None, 3, None) != 0 and "NULL index handle" in _lib.last_error()
    assert L.hb_linprobe_loss_grad(None, None, 3, 0.0, ctypes.byref(loss), None, ctypes.byref(used), None) != 0 and "NULL index handle" in _lib.last_error()
    rows, n = ctypes.c_int64(0), ctypes.c_int(0)
    assert L.hb_linprobe_partition(100, None, ctypes.byref(n)) != 0 and "NULL pointer" in _lib.last_error()
    assert L.hb_linprobe_partition(0, ctypes.byref(rows), ctypes.byref(n)) != 0 and "positive" in _lib.last_error()
    assert L.hb_linprobe_set_workspace(-1) != 0 and "hb_linprobe_set_workspace" in _lib.last_error()
    assert L.hb_linprobe_set_workspace(65536) == 0 and L.hb_linprobe_set_workspace(0) == 0


def test_partition_is_the_written_rule_and_the_model_restates_it():
    L = _lib.lib()
    rows, n = ctypes.c_int64(0), ctypes.c_int(0)
    sizes = [1, 255, 256, 257, 512, 513, 600, 4000, 256 * 512, 256 * 512 + 1, 2074072, 10_000_000, 2 ** 31 + 5]
    for ntotal in sizes:
        assert L.hb_linprobe_partition(ntotal, ctypes.byref(rows), ctypes.byref(n)) == 0
        assert (rows.value, n.value) == R.partition(ntotal), ntotal
        assert rows.value % 256 == 0 and 1 <= n.value <= 512 and (n.value - 1) * rows.value < ntotal <= n.value * rows.value
    assert R.partition(513) == (256, 3) and R.partition(512) == (256, 2)      # 513: the smallest bank of three segments
    assert R.partition(10_000_000) == (19712, 508)


# ---- the model against float64 central differences ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [R.WORLDS[0], R.SEGMENT_WORLD], ids=str)
def test_model_gradient_equals_central_differences(spec):
    w = R.world(spec)
    x, y = w["x"].copy(), w["y"].astype(np.float64) * np.random.default_rng(1).uniform(0.5, 1.5, (w["x"].shape[0], 1))      # (row masses off 1)
    x[7, 3] = np.nan                                           # one skipped row
    g = np.random.default_rng(2)
    Wb = g.standard_normal((w["C"], w["D"] + 1)) * 0.5
    o = R.objective64(x, y, Wb, 1e-2)
    assert o["n"] == x.shape[0] - 1
    for _ in range(12):
        c, j = int(g.integers(0, w["C"])), int(g.integers(0, w["D"] + 1))
        h = 1e-5
        up, dn = Wb.copy(), Wb.copy()
        up[c, j] += h; dn[c, j] -= h
        fd = (R.objective64(x, y, up, 1e-2)["loss"] - R.objective64(x, y, dn, 1e-2)["loss"]) / (2 * h)
        assert abs(fd - o["grad"][c, j]) <= 1e-8 * max(1.0, abs(fd)), (c, j)


def test_segment_gradient_equals_the_float64_gradient_within_its_bound():
    for spec in (R.WORLDS[0], R.SEGMENT_WORLD):
        w = R.world(spec)
        Wb = (np.random.default_rng(3).standard_normal((w["C"], w["D"] + 1)) * 0.5).astype(np.float32)
        z, skip = R.chain_logits(w["x"], Wb)
        o = R.objective(z, w["x"], w["y"], Wb, 1e-2, skip)
        R32 = o["R"].astype(np.float32)
        seg = R.segment_gradient(R32, w["x"], skip, Wb, 1e-2)
        exact = R.objective(z, w["x"], w["y"], Wb, 1e-2, skip)
        g64 = R32.astype(np.float64).T @ np.concatenate([np.ones((z.shape[0], 1)), w["x"].astype(np.float64)], axis=1) / exact["n"] + 1e-2 * Wb
        assert (np.abs(seg - g64) <= R.gradient_bound(R32, w["x"], skip) + 1e-18).all()


# ---- named checks of the model, and the wrong variants that must fail them -------------------------------------------------------------------
def check_chain_starts_at_the_bias():
    # b = 1, two products of 2^-24: started at b every step rounds back to 1 (ties to even); started at 0 the sum is 1 + 2^-23
    x = np.array([[2.0 ** -12, 2.0 ** -12]], dtype=np.float32)
    Wb = np.array([[1.0, 2.0 ** -12, 2.0 ** -12], [0.5, 1.0, 1.0]], dtype=np.float32)
    z, skip = R.chain_logits(x, Wb)
    assert z[0, 0] == np.float32(1.0) and not skip.any(), "chain_from_bias"


def check_rows_weigh_by_their_label_mass():
    w = R.world(R.WORLDS[0])
    Wb = np.random.default_rng(4).standard_normal((w["C"], w["D"] + 1))
    o = R.objective64(w["x"], np.zeros_like(w["y"]), Wb, 0.0)      # rows without label mass weigh nothing
    assert o["loss"] == 0.0 and not o["grad"].any(), "label_mass"


def check_mean_is_over_the_used_rows():
    w = R.world(R.WORLDS[0])
    Wb = np.random.default_rng(5).standard_normal((w["C"], w["D"] + 1))
    x = w["x"].copy()
    x[[5, 77], 2] = np.nan
    keep = np.ones(x.shape[0], dtype=bool); keep[[5, 77]] = False
    a, b = R.objective64(x, w["y"], Wb, 1e-2), R.objective64(w["x"][keep], w["y"][keep], Wb, 1e-2)
    assert a["n"] == b["n"] == x.shape[0] - 2, "mean_over_used"
    assert abs(a["loss"] - b["loss"]) <= 1e-13 * abs(b["loss"]) and np.abs(a["grad"] - b["grad"]).max() <= 1e-13, "mean_over_used"


def check_bias_is_regularised():
    w = R.world(R.WORLDS[0])
    Wb = np.zeros((w["C"], w["D"] + 1)); Wb[:, 0] = [1.0, -2.0, 0.5]
    o = R.objective64(w["x"], np.zeros_like(w["y"]), Wb, 0.1)
    assert abs(o["loss"] - 0.05 * 5.25) <= 1e-15 and np.allclose(o["grad"][:, 0], 0.1 * Wb[:, 0], rtol=0, atol=1e-15), "bias_regularised"


def check_segments_are_added_in_ascending_order():
    rows, D = 513, 2                                           # three segments: rows 0 .. 255, 256 .. 511, 512
    x = np.zeros((rows, D), dtype=np.float32)
    Rm = np.zeros((rows, 1), dtype=np.float32)
    Rm[0, 0], Rm[256, 0], Rm[512, 0] = 1.0, 1e20, -1e20       # (1 + 1e20) - 1e20 = 0 in float64; the 1 added last stays
    g = R.segment_gradient(Rm, x, np.zeros(rows, dtype=bool), np.zeros((1, D + 1)), 0.0)
    assert g[0, 0] == 0.0, "segment_order"


CHECKS = [check_chain_starts_at_the_bias, check_rows_weigh_by_their_label_mass, check_mean_is_over_the_used_rows, check_bias_is_regularised,
          check_segments_are_added_in_ascending_order]


def test_the_model_passes_its_named_checks():
    for check in CHECKS:
        check()


def _chain_started_at_zero(x, Wb):
    Wb = np.asarray(Wb, dtype=np.float32)
    z, skip = ORIGINAL["chain_logits"](x, np.concatenate([np.zeros((Wb.shape[0], 1), dtype=np.float32), Wb[:, 1:]], axis=1))
    z = (z + Wb[:, 0][None, :]).astype(np.float32)
    z[skip] = 0.0
    return z, skip


def _mass_dropped(y):
    return np.ones(y.shape[0])


def _mean_over_all_rows(skipped):
    return int(skipped.shape[0])


def _bias_unregularised(Wb, l2):
    Wb = np.asarray(Wb, dtype=np.float64).copy()
    Wb[:, 0] = 0.0
    return 0.5 * l2 * float((Wb * Wb).sum()), l2 * Wb


def _segments_in_descending_order(partials):
    return ORIGINAL["add_segments"](partials[::-1])


ORIGINAL = {name: getattr(R, name) for name in ("chain_logits", "row_mass", "used_rows", "regulariser", "add_segments")}
MUTANTS = [("chain_logits", _chain_started_at_zero, check_chain_starts_at_the_bias, "chain_from_bias"),
           ("row_mass", _mass_dropped, check_rows_weigh_by_their_label_mass, "label_mass"),
           ("used_rows", _mean_over_all_rows, check_mean_is_over_the_used_rows, "mean_over_used"),
           ("regulariser", _bias_unregularised, check_bias_is_regularised, "bias_regularised"),
           ("add_segments", _segments_in_descending_order, check_segments_are_added_in_ascending_order, "segment_order")]


@pytest.mark.parametrize("target, wrong, check, name", MUTANTS, ids=[m[1].__name__.lstrip("_") for m in MUTANTS])
def test_a_wrong_variant_fails_its_named_check(monkeypatch, target, wrong, check, name):
    monkeypatch.setattr(R, target, wrong)
    with pytest.raises(AssertionError, match=name):
        check()
    monkeypatch.undo()
    check()


# ---- the restated fit, and the worlds' own condition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", R.WORLDS, ids=str)
def test_restated_fit_converges_and_the_world_holds_its_cap(spec):
    w = R.fit_world(spec)                                      # (asserts the cap: at most 2 % of the validation rows under the threshold)
    assert w["restated_state"] == "converged" and 1 <= w["restated_iters"] <= 60
    g = R.objective64(w["x"], w["y"], w["restated"], R.FIT_L2)["grad"]
    assert np.abs(g).max() <= 2 * R.FIT_GTOL
    assert np.abs(R.objective64(w["x"], w["y"], w["optimum"], R.FIT_L2)["grad"]).max() <= 1e-11
    assert (w["counts"].sum(axis=1) == w["P"]).all() and w["counts"].max() <= w["P"]
    assert np.abs(np.linalg.norm(w["x"].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_a_world_that_breaks_the_cap_is_refused_by_its_generator():
    margins = np.linspace(0.0, 1.0, 1000)                      # 2.1 % of the rows at or under 0.0205
    assert R.assert_cap(margins, 0.0195) == 0.02
    with pytest.raises(AssertionError):
        R.assert_cap(margins, 0.0205, "a world whose validation margins crowd the threshold")


def test_the_wide_and_the_segment_world_are_what_they_are_for():
    w = R.world(R.WIDE_WORLD, 196)
    assert w["C"] == 151 and (w["counts"].sum(axis=1) == 196).all() and (151 + 7) // 8 * 8 == 152
    assert R.partition(R.world(R.SEGMENT_WORLD)["x"].shape[0]) == (256, 3)


def test_the_big_world_and_the_tile_worlds_are_what_they_are_for():
    n = R.BIG_ROWS
    assert R.BIG_WORLD[:3] == (3, 16, n) and -(-n // 256) == 513 and R.partition(n) == (512, 257) and n - 256 * 512 == 123
    assert n > 2 * 65536 and 65536 < R.BIG_HOLE < n            # the loss tree: rows at j = 1 and 2; the non-finite row past 65,536
    w = R.big_world()
    assert np.flatnonzero(R.skipped_rows(w["x"])).tolist() == [R.BIG_HOLE] and np.isfinite(R.world(R.BIG_WORLD)["x"]).all()
    assert R.chunks(n, None) == [(0, n, 257)]
    three = R.chunks(n, 3)
    assert len(three) == 86 and three[-1] == (255 * 512, n - 255 * 512, 2) and all(c == (i * 1536, 1536, 3) for i, c in enumerate(three[:-1]))
    assert R.chunks(513, 1) == [(0, 256, 1), (256, 256, 1), (512, 1, 1)] and R.chunks(513, 2) == [(0, 512, 2), (512, 1, 1)] and R.chunks(513, 0) == R.chunks(513, 1)
    tiles = {}
    for C, D, rows, n_val, seed, sigma in R.TILE_WORLDS:
        assert rows == R.TILE_ROWS == 9 * 32 + 12 and R.partition(rows) == (256, 2)
        tiles.setdefault(-(-C // 32), set()).add(C)
        w = R.world((C, D, rows, n_val, seed, sigma))
        assert w["counts"].shape == (rows, C) and (w["counts"].sum(axis=1) == 16).all()
    assert sorted(tiles) == [1, 2, 3, 4, 5, 6, 7, 8] and all(32 * ct in cs for ct, cs in tiles.items())          # every tile count with its tile full ...
    assert all(32 * (ct - 1) + 1 in cs for ct, cs in tiles.items() if ct > 2)                                     # ... and with one class in its last tile
    assert (256, 72) in {w[:2] for w in R.TILE_WORLDS} and (225, 384) in {w[:2] for w in R.TILE_WORLDS}
    assert len(set(w[4] for w in R.TILE_WORLDS)) == len(R.TILE_WORLDS)


def test_segment_partials_in_step_equal_the_row_by_row_form_on_bits():
    for spec, hole in ((R.WORLDS[0], 37), (R.SEGMENT_WORLD, 512), (R.TILE_WORLDS[2], 299)):
        w = R.world(spec)
        x = w["x"].copy(); x[hole, 3] = np.nan
        Wb = (np.random.default_rng(7).standard_normal((w["C"], w["D"] + 1)) * 0.5).astype(np.float32)
        z, skip = R.chain_logits(x, Wb)
        R32 = R.objective(z, x, w["y"], Wb, 1e-2, skip)["R"].astype(np.float32)
        fast, slow = R.segment_partials(R32, x, skip), R.segment_partials_by_rows(R32, x, skip)
        assert len(fast) == len(slow) == R.partition(x.shape[0])[1]
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(fast, slow))
