"""Excluding searches without a GPU: the C ABI of include/hbird_hip_exclude.h against its bindings and INTEGRATION.md, the rung rule through
hb_exclude_plan_replay, and `filter_reference`, a numpy restatement of the filter's definition that shares nothing with the kernel (the GPU
tests in test_exclude_gpu.py hold the kernel to it)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex, NearestNeighborSearchHIP, exclude_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_index_set_row_groups", "hb_index_search_excluding", "hb_exclude_filter", "hb_index_last_exclusion", "hb_exclude_plan_replay"}
C_TYPES = {"hb_index_t*": ctypes.c_void_p, "const hb_index_t*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "const int64_t*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p,
           "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "float": ctypes.c_float}
HOST_ARRAYS = {"rungs": ctypes.POINTER(ctypes.c_int), "out[4]": ctypes.POINTER(ctypes.c_int64)}       # host arrays: typed pointers


def filter_reference(idx, dist, id_base, groups, qgroups, k, pad):
    """The definition of the filter, entry by entry: of list i, the entries with id >= 0 whose row (id - id_base) lies outside the table or in
    another group than qgroups[i] (or any group when qgroups[i] == -1) survive, in order; the first k go out, -1 / pad fill the tail.
    complete[i] = at least k survivors, or a negative id anywhere in the list.  -> (out_idx [nq, k], out_dist [nq, k], complete [nq])."""
    nq, n_rows = len(idx), len(groups)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_d = np.full((nq, k), pad, dtype=np.float32)
    complete = np.zeros(nq, dtype=np.int32)
    for i in range(nq):
        kept = []
        for j in range(idx.shape[1]):
            e = int(idx[i, j])
            if e < 0:
                continue
            row = e - id_base
            if qgroups[i] != -1 and 0 <= row < n_rows and groups[row] == qgroups[i]:
                continue
            kept.append(j)
        for o, j in enumerate(kept[:k]):
            out_i[i, o] = idx[i, j]
            out_d[i, o] = dist[i, j]
        complete[i] = 1 if len(kept) >= k or bool((idx[i] < 0).any()) else 0
    return out_i, out_d, complete


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


def test_exclude_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_exclude.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    inc = '#include "hbird_hip_exclude.h"'
    assert inc in main and main.index(inc) > main.index('#include "hbird_hip_grid.h"') > main.index('#include "hbird_hip_select.h"')
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_EXCLUDE)
    assert not NAMES & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_CENTRE))
    for name in NAMES:                      # hbird_hip.h points at the entries, it does not declare them
        assert name in main and not re.search(name + r"\s*\(", main)
    L = _lib.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_EXCLUDE[name]
        assert ret == "int" and res is ctypes.c_int
        want = [HOST_ARRAYS[arg] if arg in HOST_ARRAYS else C_TYPES[typ] for typ, arg in params]
        assert want == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res and f"`{name}`" in doc
    assert [a for _, a in decl["hb_index_set_row_groups"][1]] == ["ix", "groups", "n", "n_groups", "on_device"]
    assert [a for _, a in decl["hb_index_search_excluding"][1]] == ["ix", "q", "nq", "k", "id_base", "qgroups", "out_idx", "out_dist", "io_on_device"]
    assert [a for _, a in decl["hb_exclude_filter"][1]] == ["idx", "dist", "nq", "k_list", "id_base", "groups", "n_rows", "qgroups", "k", "pad",
                                                            "out_idx", "out_dist", "out_complete", "hip_stream"]
    assert [a for _, a in decl["hb_index_last_exclusion"][1]] == ["ix", "out[4]"]
    assert [a for _, a in decl["hb_exclude_plan_replay"][1]] == ["k", "gmax", "rungs", "max_rungs"]


def test_exclude_unit_is_built_outside_the_pinned_units_and_names_its_kernels_apart():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hbird_exclude.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_exclude" not in re.search(r"^KNN_UNITS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_exclude" not in re.search(r"^K5_UNITS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_exclude.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(csrc, "hbird_exclude.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src)
    assert {"exclude_filter_kernel", "exclude_group_sizes_kernel"} <= set(kernels) and len(kernels) >= 3
    assert not [k for k in kernels if k.startswith(("knn_", "aggregate_", "rerank_"))]


def test_exclude_entries_refuse_null_handles_with_a_message():
    L = _lib.lib()
    g = (ctypes.c_int32 * 2)(0, 0)
    out = (ctypes.c_int64 * 4)()
    assert L.hb_index_set_row_groups(None, g, 2, 1, 0) != 0 and b"NULL" in L.hb_last_error()
    assert L.hb_index_search_excluding(None, None, 1, 30, 0, None, None, None, 0) != 0 and b"NULL" in L.hb_last_error()
    assert L.hb_index_last_exclusion(None, out) != 0 and b"NULL" in L.hb_last_error()
    assert L.hb_exclude_filter(None, None, 1, 30, 0, None, 0, None, 30, 0.0, None, None, None, None) != 0 and b"NULL" in L.hb_last_error()
    for bad in ((1, 0, 1), (1, 2049, 1), (1, 30, 0), (1, 30, 2049), (-1, 30, 30)):       # (nq, k_list, k): refused before the pointers are looked at
        assert L.hb_exclude_filter(None, None, bad[0], bad[1], 0, None, 0, None, bad[2], 0.0, None, None, None, None) != 0


@pytest.mark.parametrize("k,gmax,want", [
    (30, 196, [226]), (30, 226, [256]), (30, 227, [256, 257]), (30, 300, [256, 330]), (255, 300, [512, 555]), (300, 100, [400]),
    (30, 2018, [256, 2048]), (30, 0, [30]), (1, 1, [2]), (128, 128, [256]), (128, 129, [256, 257]), (129, 127, [256]), (129, 128, [257]),
    (256, 256, [512]), (256, 257, [512, 513]), (2048, 0, [2048]), (1024, 1024, [2048])])
def test_rung_rule_through_the_replay(k, gmax, want):
    rungs = (ctypes.c_int * 2)(-7, -7)
    n = _lib.lib().hb_exclude_plan_replay(k, gmax, rungs, 2)
    assert n == len(want) and [rungs[i] for i in range(n)] == want
    assert exclude_plan(k, gmax) == want                      # Python calls the replay, it does not restate the rule
    r0 = 256 * -(-(k + min(k, gmax)) // 256)
    assert want == ([k + gmax] if r0 >= k + gmax else [r0, k + gmax])


@pytest.mark.parametrize("k,gmax", [(30, 2019), (1, 2048), (2048, 1), (1000, 1049)])
def test_rung_rule_refuses_need_beyond_the_limit(k, gmax):
    L = _lib.lib()
    rungs = (ctypes.c_int * 2)(-7, -7)
    assert L.hb_exclude_plan_replay(k, gmax, rungs, 2) < 0
    msg = L.hb_last_error().decode()
    assert f"k = {k}" in msg and f"gmax = {gmax}" in msg and "2048" in msg and "memory_size" in msg and "epochs" in msg
    assert list(rungs) == [-7, -7]
    with pytest.raises(ValueError, match="memory_size"):
        exclude_plan(k, gmax)


def test_rung_rule_refuses_bad_arguments():
    L = _lib.lib()
    rungs = (ctypes.c_int * 2)()
    assert L.hb_exclude_plan_replay(0, 5, rungs, 2) < 0 and L.hb_exclude_plan_replay(2049, 0, rungs, 2) < 0
    assert L.hb_exclude_plan_replay(30, -1, rungs, 2) < 0
    assert L.hb_exclude_plan_replay(30, 300, rungs, 1) < 0 and L.hb_exclude_plan_replay(30, 300, None, 2) < 0
    assert L.hb_exclude_plan_replay(30, 100, rungs, 1) == 1 and rungs[0] == 130


def test_python_surface():
    for meth in ("set_row_groups", "search_excluding", "search_aggregate_excluding", "search_aggregate_grid_excluding", "last_exclusion"):
        assert callable(getattr(HipFlatIndex, meth)) and callable(getattr(HipMultiIndex, meth))
    assert "not supported" in HipMultiIndex.search_excluding.__doc__.lower()
    assert list(inspect.signature(HipFlatIndex.set_row_groups).parameters)[1:] == ["groups", "n_groups"]
    assert list(inspect.signature(HipFlatIndex.search_excluding).parameters)[1:] == ["q", "k", "qgroups", "id_base"]
    assert list(inspect.signature(HipFlatIndex.search_aggregate_excluding).parameters)[1:] == ["q", "k", "qgroups", "beta", "id_base", "want_neighbours"]
    assert list(inspect.signature(HipFlatIndex.search_aggregate_grid_excluding).parameters)[1:5] == ["q", "ks", "betas", "qgroups"]
    assert list(inspect.signature(NearestNeighborSearchHIP.find_nearest_neighbors_excluding).parameters)[1:] == ["q", "qgroups", "k"]
    multi = HipMultiIndex.__new__(HipMultiIndex)
    for meth in ("search_excluding", "search_aggregate_excluding", "search_aggregate_grid_excluding", "set_row_groups"):
        with pytest.raises(ValueError, match="single-index"):
            getattr(multi, meth)(None, 1, None)
    multi.indexes = []          # (so that the finaliser finds what it closes)


def test_filter_reference_on_a_hand_made_case():
    groups = np.array([0, 0, 1, -1, 2], dtype=np.int32)
    idx = np.array([[10, 11, 12, 13, 14, 99], [12, 10, -1, -1, -1, -1], [10, 11, 12, 13, 14, 99], [10, 11, 12, 13, 14, 99]], dtype=np.int64)
    dist = np.arange(24, dtype=np.float32).reshape(4, 6)
    oi, od, comp = filter_reference(idx, dist, 10, groups, np.array([0, 1, -1, 7], dtype=np.int32), 3, -np.inf)
    assert oi.tolist() == [[12, 13, 14], [10, -1, -1], [10, 11, 12], [10, 11, 12]]
    assert od.tolist() == [[2.0, 3.0, 4.0], [7.0, -np.inf, -np.inf], [12.0, 13.0, 14.0], [18.0, 19.0, 20.0]]
    assert comp.tolist() == [1, 1, 1, 1]
    oi, _, comp = filter_reference(idx[:1], dist[:1], 10, groups, np.array([0], dtype=np.int32), 5, np.inf)
    assert oi.tolist() == [[12, 13, 14, 99, -1]] and comp.tolist() == [0]          # the id outside the table is kept; 4 survivors < 5, no -1
