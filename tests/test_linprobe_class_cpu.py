"""The image-level linear probe without a GPU: the C ABI of include/hbird_hip_linprobe_class.h against its bindings, the exported symbols, the
documents and the build; the NULL-handle refusals; the numpy restatement of tests/linprobe_class_refs.py against hand-computed cases; the fit
worlds' cap; the case lists of tests/test_linprobe_class_gpu.py held to the class-sweep, wave-tile and workspace-chunk arithmetic; the
eval.py --task linear-classify parser with its refusals."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import linprobe_class_refs as K
import linprobe_refs as R
from hbird_mi import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
NAMES = {"hb_linprobe_class_logits", "hb_linprobe_class_loss_grad", "hb_logits_topn"}
V = ctypes.c_void_p
C_TYPES = {"hb_index_t*": V, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float*": V, "const float*": V, "double*": V,
           "const int32_t*": V, "int32_t*": V, "void*": V}
HOST_OUT = {"loss_host": ctypes.POINTER(ctypes.c_double), "used_host": ctypes.POINTER(ctypes.c_int64)}


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


def test_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_linprobe_class.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_LINPROBE_CLASS)
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    inc = '#include "hbird_hip_linprobe_class.h"'
    assert main.count(inc) == 1 and main.index('#include "hbird_hip_depth.h"') < main.index(inc) < main.rindex("#ifdef __cplusplus")
    for other in ("hbird_hip.h", "hbird_hip_linprobe.h"):      # two test files parse these for their own entries
        assert not any(n in open(os.path.join(ROOT, "include", other)).read() for n in NAMES), other
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_LINPROBE_CLASS[name]
        assert ret == "int" and res is ctypes.c_int
        assert [HOST_OUT.get(arg) or C_TYPES[typ] for typ, arg in params] == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_linprobe_class_logits"][1]] == ["ix", "Wb", "C", "out"]
    assert [a for _, a in decl["hb_linprobe_class_loss_grad"][1]] == ["bank", "labels", "Wb", "C", "l2", "loss_host", "grad", "used_host", "resid_opt"]
    assert [a for _, a in decl["hb_logits_topn"][1]] == ["logits", "nq", "C", "topn", "pred", "hip_stream"]
    assert int(re.search(r"#define HB_LINPROBE_CLASS_MAX_C (\d+)", header).group(1)) == _lib.LINPROBE_CLASS_MAX_C == K.MAX_C == 16384
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {n for n in re.findall(r"\b(hb_(?:linprobe_class|logits)_\w+)", exported)} == NAMES
    for words in ("THIS ENGINE'S OWN", "not DINO's SGD recipe", "No dataset is on our machines", "SKIPPED", "ds_swizzle", "16, 8, 4, 2, 1",
                  "one rounding", "LOWER class id", "THE SEGMENT RULE", "No floating-point atomic"):
        assert words in header, words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_linprobe_class.h" in doc and all(n in doc for n in NAMES)
    assert all(n in doc for n in ("class_logits_of", "class_loss_grad", "linear_probe_fit_classes", "logits_topn", "evaluate_linear_probe",
                                  "fit_linear_probe", "LinearClassMetrics", "hbird_linear_classification"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Image-level linear probe" in design and "linprobe_class_forward_kernel" in design and "linprobe_backward_wide_kernel" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "round 36" in readme and "--task linear-classify" in readme and "not DINO's SGD recipe" in readme
    assert "exp_linprobe_class.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_unit_is_built_outside_the_pinned_units_and_has_no_float_atomic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hbird_linprobe_class.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_linprobe_class.h" in hdrs and "hbird_linprobe_dev.h" in hdrs
    for units in ("KNN_UNITS", "K5_UNITS", "RES_UNITS"):
        assert "hbird_linprobe" not in re.search(rf"^{units}\s*=(.*)$", mk, flags=re.M).group(1)
    src = re.sub(r"//.*", "", open(os.path.join(CSRC, "hbird_linprobe_class.hip")).read())
    kernels = set(re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src, flags=re.S))
    assert kernels == {"linprobe_class_forward_kernel", "linprobe_class_check_kernel", "logits_topn_kernel"}
    assert "rocblas" not in src.lower() and "hipblas" not in src.lower() and "unsafeAtomicAdd" not in src
    calls = re.findall(r"\b(atomic\w+)\s*\(\s*([^,]+),", src)                                   # the one atomic works on the integer flag
    assert calls == [("atomicOr", "flag")] and "int32_t* __restrict__ flag" in src
    assert "mfma_f32_32x32x2f32" in src and "ds_swizzle" in src and '#include "hbird_linprobe_dev.h"' in src
    assert f"#define LPC_SWEEP {K.SWEEP_TILES}" in src
    # the backward kernels stay in hbird_linprobe.hip, the wide wave tile among them
    old = open(os.path.join(CSRC, "hbird_linprobe.hip")).read()
    assert "linprobe_backward_wide_kernel" in old and f"#define LP_BWD_WIDE_CTW {K.BWD_WIDE[0]}" in old and f"#define LP_BWD_WIDE_DTW {K.BWD_WIDE[1]}" in old
    assert re.search(r"if \(ct > 8\)[^\n]*\n\s*linprobe_backward_wide_kernel<", old)      # cp <= 256 stays on the kernel it had


def test_entries_refuse_null_handles_and_pointers_before_any_launch():
    L = _lib.lib()
    loss, used = ctypes.c_double(0), ctypes.c_int64(0)
    assert L.hb_linprobe_class_logits(None, None, 3, None) != 0 and "NULL index handle" in _lib.last_error()
    assert L.hb_linprobe_class_loss_grad(None, None, None, 3, 0.0, ctypes.byref(loss), None, ctypes.byref(used), None) != 0
    assert "NULL index handle" in _lib.last_error()
    assert L.hb_logits_topn(None, 4, 3, 1, None, None) != 0 and "NULL pointer" in _lib.last_error()
    fake = ctypes.c_void_p(256)                                # never dereferenced: the refusals come first
    for C, topn, nq, msg in ((0, 1, 4, "[1, 16384]"), (16385, 1, 4, "[1, 16384]"), (3, 0, 4, "topn outside [1, 8]"), (3, 9, 4, "topn outside [1, 8]"),
                             (3, 1, -1, "negative")):
        assert L.hb_logits_topn(fake, nq, C, topn, fake, None) != 0 and msg in _lib.last_error(), (C, topn, nq)
    assert L.hb_logits_topn(fake, 0, 3, 5, fake, None) == 0    # an empty call


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def test_the_hard_label_objective_is_the_soft_one_on_one_hot_rows_and_skips_unlabelled_rows():
    w = K.class_world(5, 16, 40, hole=7)
    cls = w["cls"].copy(); cls[11] = -1
    Wb = np.random.default_rng(1).standard_normal((5, 17))
    z = R.logits64(w["x"], Wb)
    o = K.objective(z, w["x"], cls, Wb, 1e-2)
    keep = np.setdiff1d(np.arange(40), [7, 11])
    assert o["n"] == 38 and not o["R"][[7, 11]].any() and not o["l"][[7, 11]].any()
    lse = np.log(np.exp(z[keep]).sum(axis=1))
    assert np.allclose(o["l"][keep], lse - z[keep, cls[keep]], rtol=1e-13, atol=0)
    want = np.exp(z[keep] - lse[:, None]); want[np.arange(38), cls[keep]] -= 1.0
    assert np.allclose(o["R"][keep], want, rtol=1e-12, atol=1e-15)
    assert K.one_hot(np.array([2, -1, 0]), 3).tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]


def test_topn_and_counts_restate_the_definitions_on_hand_computed_cases():
    nan = np.nan
    z = np.array([[0.5, 2.0, 2.0, -1.0], [nan, nan, 1.0, nan], [nan, nan, nan, nan], [-0.0, 0.0, -np.inf, np.inf]], dtype=np.float32)
    assert K.topn(z, 3).tolist() == [[1, 2, 0], [2, -1, -1], [-1, -1, -1], [3, 0, 1]]
    assert K.topn(z[:, :2], 3)[0].tolist() == [1, 0, -1]       # C < topn: the tail holds -1
    pred = np.array([[1, 2, 0], [2, 0, 1], [0, 1, 2], [2, 1, 0]])
    c, per, n = K.counts(pred, np.array([2, 2, -1, 0]), 3)
    assert c.tolist() == [1, 2, 3] and n == 3 and per.tolist() == [[1, 0], [0, 0], [2, 1]]


# ---- the fit worlds' cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, l2", K.FIT_CASES, ids=str)
def test_restated_fit_converges_and_the_world_holds_its_cap(spec, l2):
    w = K.fit_world(spec, l2)                                  # (asserts the cap: at most 2 % of the validation rows under the threshold)
    assert w["restated_state"] == "converged" and 1 <= w["restated_iters"] <= 60 and w["restated_left_out"] <= R.VAL_CAP
    assert np.abs(R.objective64(w["x"], w["y"], w["restated"], l2)["grad"]).max() <= 2 * K.FIT_GTOL
    assert np.abs(R.objective64(w["x"], w["y"], w["optimum"], l2)["grad"]).max() <= K.OPTIMUM_GTOL
    assert (w["y"].sum(axis=1) == 1).all() and (w["y"].argmax(axis=1) == w["cls"]).all()
    assert np.abs(np.linalg.norm(w["x"].astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- the GPU case lists against the dispatch arithmetic ------------------------------------------------------------------------------------------
def test_the_gpu_cases_reach_every_sweep_every_wave_tile_shape_and_the_chunk_loop():
    assert K.sweeps(3) == [1] and K.sweeps(256) == [8] and K.sweeps(257) == [8, 1] and K.sweeps(512) == [8, 8] and K.sweeps(513) == [8, 8, 1]
    assert K.sweeps(1000) == [8, 8, 8, 8] and K.sweeps(K.MAX_C) == [8] * 64
    alone = {s[0] for s in map(K.sweeps, K.LOGIT_CS) if len(s) == 1}
    later = {s[-1] for s in map(K.sweeps, K.LOGIT_CS) if len(s) > 1}
    assert alone == later == set(range(1, 9))                  # every instantiation of a sweep, as the first and as a later one
    for C in (256, 257, 512, 513):                             # both ends of the first two class groups
        assert C in K.LOGIT_CS
    assert any(C % 32 for C in K.LOGIT_CS) and 1000 % 32 == 8  # ragged last tiles
    assert {D for _, D in K.LOGIT_WIDE} == {72, 384} and all(C > 256 for C, _ in K.LOGIT_WIDE)
    assert R.partition(K.ROWS) == (256, 2) and -(-K.ROWS // 256) == 2 and K.ROWS % 32
    assert all(C <= _lib.LINPROBE_MAX_C for C in K.TWIN_CS) and {3, 33, 151, 256} == set(K.TWIN_CS)
    assert all(C > 256 for C in K.OBJECTIVE_CS)
    # the backward wave tile at cp > 256: (groups of class tiles, tiles in the last, groups of column tiles, tiles in the last)
    assert K.backward_waves(1000, 72) == (8, 4, 2, 1) and K.backward_waves(513, 384) == (5, 1, 7, 1) and K.backward_waves(257, 16) == (3, 1, 1, 1)
    shapes = {K.backward_waves(C, D)[1::2] for C, D in list(K.GRADIENT_WIDE) + [(C, 16) for C in K.OBJECTIVE_CS]}
    assert {(4, 1), (1, 1)} <= shapes                          # a full and a ragged class group, each beside a ragged column pair
    # workspace chunks: three segments, and two at the largest residual stride of the cases
    for C, D, rows in K.CHUNK_CASES:
        seg = K.seg_bytes(C, D, rows)
        nseg = R.partition(rows)[1]
        assert nseg >= 2 and len(R.chunks(rows, seg // seg)) == nseg and len(R.chunks(rows, (2 * seg - 1) // seg)) == nseg
        assert len(R.chunks(rows, (1 << 30) // seg)) == 1
    assert R.partition(513) == (256, 3) and K.seg_bytes(257, 16, 513) == 256 * (288 + 32) * 4 and K.seg_bytes(1000, 16, 300) == 256 * (1024 + 32) * 4
    C, D, rows = K.BIG_CASE
    assert (C, D, rows) == (257, 16, R.BIG_ROWS) and R.partition(rows) == (512, 257) and rows > 2 * 65536
    w = K.class_world(C, D, rows, R.BIG_HOLE)
    assert np.flatnonzero(K.skipped(w["x"], w["cls"])).tolist() == [R.BIG_HOLE]
    assert len(K.FIT_CASES) == 3 and all(l2 == (1e-2 if spec[0] == 5 else 1e-4) for spec, l2 in K.FIT_CASES)
    assert K.MEASURED_P_REL_CLASS < 1e-5 and K.MEASURED_L_REL_CLASS < 1e-7


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_the_other_tasks_options_and_the_other_tasks_refuse_probe_l2(capsys):
    spec = importlib.util.spec_from_file_location("hbird_cli_linear_cpu", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--dataset-name", "synthetic-classify", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "32"]
    a = cli.build_parser().parse_args(base + ["--task", "linear-classify", "--probe-l2", "1e-2", "1e-3", "--top-n", "3"])
    assert a.task == "linear-classify" and a.probe_l2 == [1e-2, 1e-3] and a.top_n == 3
    assert cli.probe_key(1e-3) == "l2=0.001"
    for bad in (["--grid-k", "5"], ["--grid-temperature", "0.1"], ["--leave-one-out"], ["--linear-probe"], ["--n-neighbours", "5"], ["--top-n", "9"],
                ["--probe-l2", "1e-3", "1e-3"], ["--probe-l2", "-1"], ["--memory-sizes", "10"], ["--video-radius", "3"]):
        with pytest.raises(SystemExit):
            cli.main(base + ["--task", "linear-classify"] + bad)
    for task in ([], ["--task", "knn-classify"], ["--task", "depth"], ["--task", "video"]):
        with pytest.raises(SystemExit):
            cli.main(base + task + ["--probe-l2", "1e-3"])
        assert "--probe-l2 needs --task linear-classify" in capsys.readouterr().err
