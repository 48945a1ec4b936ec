"""Video label propagation without a GPU: the C ABI of include/hbird_hip_propagate.h against its bindings, the documents and the build; the
refusals of the three entries through ctypes (nothing is launched, no device pointer is dereferenced); the numpy restatement of
tests/propagate_refs.py against hand-computed cases and six wrong variants of it, each of which must fail a named check; the host logic of
hbird_mi/video.py (the ring's context order, `VideoMetrics` from a counts table), `VideoFolderDataModule` on files written into tmp_path, and
the eval.py --task video parser with its refusals."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import propagate_refs as R
from hbird_mi import _lib, ops
from hbird_mi import video as hvideo
from hbird_mi.data import video as vdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
NAMES = {"hb_propagate_labels", "hb_mask_upsample_argmax", "hb_mask_jf_counts"}
V = ctypes.c_void_p
C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "float*": V, "const float*": V, "int64_t*": V, "const int64_t*": V,
           "void*": V, "const int*": ctypes.POINTER(ctypes.c_int)}


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


def _cli():
    spec = importlib.util.spec_from_file_location("hbird_cli_propagate", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "hbird_hip_propagate.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_PROPAGATE)
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    assert "hbird_hip_propagate.h" not in main and not any(n in main for n in NAMES)             # the header stands on its own
    assert "hbird_hip.h" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S) and 'extern "C"' in header
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_PROPAGATE[name]
        assert ret == "int" and res is ctypes.c_int
        assert [C_TYPES[typ] for typ, _ in params] == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
    assert [a for _, a in decl["hb_propagate_labels"][1]] == ["q", "feat_pool", "label_pool", "pool_slots", "slots", "radii", "n_ctx", "gh", "gw", "d", "c",
                                                               "k", "temperature", "out_labels", "out_idx_opt", "out_score_opt", "hip_stream"]
    assert [a for _, a in decl["hb_mask_upsample_argmax"][1]] == ["labels", "B", "gh", "gw", "c", "h", "w", "channel_norm", "out", "hip_stream"]
    assert [a for _, a in decl["hb_mask_jf_counts"][1]] == ["pred", "gt", "B", "h", "w", "n_objects", "bound_px", "counts_out", "hip_stream"]
    for macro, value in (("HB_PROPAGATE_MAX_K", _lib.PROPAGATE_MAX_K), ("HB_PROPAGATE_MAX_CTX", _lib.PROPAGATE_MAX_CTX), ("HB_PROPAGATE_MAX_C", _lib.PROPAGATE_MAX_C),
                         ("HB_PROPAGATE_MAX_D", _lib.PROPAGATE_MAX_D), ("HB_JF_MAX_BOUND", _lib.JF_MAX_BOUND), ("HB_JF_NCOUNTS", len(_lib.JF_COUNTS))):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert (_lib.PROPAGATE_MAX_K, _lib.PROPAGATE_MAX_CTX, _lib.PROPAGATE_MAX_C, _lib.JF_MAX_BOUND) == (32, 32, 64, 32) and _lib.PROPAGATE_MAX_D >= 1024
    for i, word in enumerate(_lib.JF_COUNTS):
        assert int(re.search(rf"#define HB_JF_{word.upper()} (\d+)", header).group(1)) == i
    assert _lib.JF_COUNTS == R.COUNTS
    assert "THIS ENGINE'S OWN" in header and "no J&F figure" in header
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hbird_hip_propagate.h" in doc and all(n in doc for n in NAMES) and "HbirdVideoEvaluation" in doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Video label propagation" in design and all(n in design for n in NAMES)
    assert all(k in design for k in ("propagate_kernel", "mask_argmax_kernel", "jf_counts_kernel"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--task video" in readme and "round 32" in readme and "NEAREST" in readme
    assert "exp_propagate.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_units_are_built_outside_the_pinned_units_and_have_no_float_atomic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_propagate.hip" in srcs and "hbird_maskmetrics.hip" in srcs
    assert "hbird_hip_propagate.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    for units in ("KNN_UNITS", "K5_UNITS", "RES_UNITS"):
        line = re.search(rf"^{units}\s*=(.*)$", mk, flags=re.M).group(1)
        assert "hbird_propagate" not in line and "hbird_maskmetrics" not in line
    prop = re.sub(r"//.*", "", open(os.path.join(CSRC, "hbird_propagate.hip")).read())
    mask = re.sub(r"//.*", "", open(os.path.join(CSRC, "hbird_maskmetrics.hip")).read())
    assert set(re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", prop, flags=re.S)) == {"propagate_kernel"}
    assert set(re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", mask, flags=re.S)) == {"mask_extrema_kernel", "mask_argmax_kernel", "mask_extrema_init_kernel",
                                                                                     "jf_counts_kernel"}
    assert not re.search(r"\batomic\w*\s*\(", prop) and "unsafeAtomicAdd" not in prop and "unsafeAtomicAdd" not in mask
    assert "mfma_f32_32x32x2f32" in prop and "mfma" not in mask.lower()
    assert "#pragma clang fp contract(off)" in prop and "#pragma clang fp contract(off)" in mask
    # every atomic of the mask unit works on an integer: the unsigned extrema keys, the LDS counters, the 64-bit counts
    calls = re.findall(r"\b(atomic\w+)\s*\(\s*([^,]+),", mask)
    assert calls and {c for c, _ in calls} <= {"atomicMin", "atomicMax", "atomicAdd"}
    for _, target in calls:
        assert target.strip() in ("e", "e + 1", "&cnt[i]") or target.strip().startswith("counts +"), target
    assert re.search(r"unsigned\*\s*e\s*=", mask) and re.search(r"__shared__ unsigned cnt\[", mask) and "unsigned long long* __restrict__ counts" in mask


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_every_entry_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = V(4096)                       # never dereferenced: every call below is refused first
    names = ("q", "feat", "lab", "pool", "slots", "radii", "n_ctx", "gh", "gw", "d", "c", "k", "temp", "out", "idx", "score", "stream")
    good = (p, p, p, 3, _ints(0, 2), _ints(1, -1), 2, 6, 8, 64, 3, 5, 0.1, p, None, None, None)

    def prop(**kw):
        assert set(kw) <= set(names)
        return tuple(kw.get(n, v) for n, v in zip(names, good))
    nan, inf = float("nan"), float("inf")
    cases = [(prop(q=None), "NULL"), (prop(feat=None), "NULL"), (prop(lab=None), "NULL"), (prop(out=None), "NULL"), (prop(slots=None), "NULL"),
             (prop(radii=None), "NULL"), (prop(idx=p), "NULL"), (prop(score=p), "NULL"),
             (prop(pool=0), "positive"), (prop(n_ctx=0), "positive"), (prop(gh=0), "positive"), (prop(gw=-1), "positive"), (prop(d=0), "positive"),
             (prop(c=0), "positive"), (prop(k=0), "positive"),
             (prop(k=33), "limit"), (prop(n_ctx=33), "limit"), (prop(c=65), "limit"), (prop(d=_lib.PROPAGATE_MAX_D + 4), "limit"),
             (prop(gh=1 << 15, gw=1 << 15), "limit"), (prop(d=6), "multiple of 4"), (prop(d=62), "multiple of 4"),
             (prop(temp=0.0), "temperature"), (prop(temp=-1.0), "temperature"), (prop(temp=nan), "temperature"), (prop(temp=inf), "temperature"),
             (prop(q=V(4100)), "aligned"), (prop(slots=_ints(0, 3)), "slot"), (prop(slots=_ints(-1, 0)), "slot")]
    for args, word in cases:
        assert L.hb_propagate_labels(*args) == -1, args
        assert word in _lib.last_error() and "hb_propagate_labels" in _lib.last_error(), (args, _lib.last_error())
    good_up = (p, 2, 6, 8, 3, 48, 64, 1, p, None)
    for at, value, word in ((0, None, "NULL"), (8, None, "NULL"), (1, 0, "positive"), (2, 0, "positive"), (3, -1, "positive"), (4, 0, "positive"),
                            (5, 0, "positive"), (6, 0, "positive"), (4, 65, "limit")):
        args = good_up[:at] + (value,) + good_up[at + 1:]
        assert L.hb_mask_upsample_argmax(*args) == -1, args
        assert word in _lib.last_error() and "hb_mask_upsample_argmax" in _lib.last_error(), (args, _lib.last_error())
    good_jf = (p, p, 2, 48, 64, 3, 2, p, None)
    for at, value, word in ((0, None, "NULL"), (1, None, "NULL"), (7, None, "NULL"), (2, 0, "positive"), (3, 0, "positive"), (4, -3, "positive"),
                            (5, 0, "positive"), (6, -1, "limit"), (6, 33, "limit")):
        args = good_jf[:at] + (value,) + good_jf[at + 1:]
        assert L.hb_mask_jf_counts(*args) == -1, args
        assert word in _lib.last_error() and "hb_mask_jf_counts" in _lib.last_error(), (args, _lib.last_error())


def test_wrappers_check_shapes_and_dtypes_without_a_gpu():
    q, feat, lab = torch.zeros(6, 8), torch.zeros(2, 6, 8), torch.zeros(2, 6, 3)
    for bad in (dict(q=q.double()), dict(q=q[:5]), dict(feat=feat[:, :5]), dict(lab=lab[:1]), dict(slots=[0, 1], radii=[1]), dict(slots=[], radii=[])):
        kw = dict(q=q, feat=feat, lab=lab, slots=[0], radii=[1])
        kw.update(bad)
        with pytest.raises(ValueError, match="propagate_labels"):
            ops.propagate_labels(kw["q"], kw["feat"], kw["lab"], kw["slots"], kw["radii"], (2, 3))
    with pytest.raises(ValueError, match="mask_upsample_argmax"):
        ops.mask_upsample_argmax(torch.zeros(1, 5, 3), (2, 3), 8, 8)
    with pytest.raises(ValueError, match="mask_jf_counts"):
        ops.mask_jf_counts(torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, 5, dtype=torch.int64), 1, 1)
    with pytest.raises(ValueError, match="mask_jf_counts"):
        ops.mask_jf_counts(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 1, 1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.propagate_labels(q, feat, lab, [0], [1], (2, 3))


# ---- the model against hand-computed cases -------------------------------------------------------------------------------------------------
def test_candidates_of_a_2x3_grid():
    assert R.candidates(2, 3, [0], 0, 0).tolist() == [0]
    assert R.candidates(2, 3, [1], 0, 0).tolist() == [0, 1, 3, 4]
    assert R.candidates(2, 3, [1], 1, 2).tolist() == [1, 2, 4, 5]
    assert R.candidates(2, 3, [-1], 1, 1).tolist() == [0, 1, 2, 3, 4, 5]
    assert R.candidates(2, 3, [0, 1, -1], 0, 0).tolist() == [0, 6, 7, 9, 10, 12, 13, 14, 15, 16, 17]


def _hand_world():
    """2 x 3 grid, d = 4: cell i of slot 0 is the unit vector e_(i % 4), of slot 1 a 0.6 / 0.8 mix; the query frame equals slot 0."""
    eye = np.eye(4, dtype=np.float32)
    s0 = np.stack([eye[i % 4] for i in range(6)])
    s1 = np.stack([np.float32(0.6) * eye[i % 4] + np.float32(0.8) * eye[(i + 1) % 4] for i in range(6)]).astype(np.float32)
    lab = np.zeros((2, 6, 2), dtype=np.float32)
    lab[0, :, 0] = np.arange(6) / 8.0
    lab[0, :, 1] = 1 - lab[0, :, 0]
    lab[1, :, 0] = 1.0
    return s0.copy(), np.stack([s0, s1]), lab


def test_lists_and_rows_by_hand():
    q, feat, lab = _hand_world()
    # radius 0, k larger than the candidate count: the cell itself at score 1, then padding; the row is the cell's label row
    out, idx, score = R.propagate(q, feat, lab, [0], [0], (2, 3), 3, 0.1)
    assert idx.tolist() == [[i, -1, -1] for i in range(6)]
    assert np.array_equal(score[:, 0], np.ones(6, np.float32)) and np.isneginf(score[:, 1:]).all()
    assert np.array_equal(out, lab[0].astype(np.float64))
    # radius 1 around cell (0, 0): candidates 0, 1, 3, 4 with scores e0 . e_(i % 4) = 1, 0, 0, 1: the tie 0 / 4 goes to the lower id, then 1 before 3
    _, idx, score = R.propagate(q, feat, lab, [0], [1], (2, 3), 4, 0.1)
    assert idx[0].tolist() == [0, 4, 1, 3] and score[0].tolist() == [1.0, 1.0, 0.0, 0.0]
    # unrestricted: cell (1, 2) = e1 matches cells 1 and 5
    _, idx, score = R.propagate(q, feat, lab, [0], [-1], (2, 3), 2, 0.1)
    assert idx[5].tolist() == [1, 5] and score[5].tolist() == [1.0, 1.0]
    # one slot listed at two context positions: an exact tie, the lower id (context position 0) first; equal weights give the row back
    out, idx, score = R.propagate(q, feat, lab, [0, 0], [0, 0], (2, 3), 2, 0.1)
    assert idx.tolist() == [[i, 6 + i] for i in range(6)] and np.array_equal(score[:, 0], score[:, 1])
    assert np.allclose(out, lab[0], atol=1e-15)
    # two slots, the weights by hand: scores 1 and 0.6 at temperature 0.1 -> w = 1 / (1 + exp(-4)), on label rows [i / 8, 1 - i / 8] and [1, 0]
    out, idx, score = R.propagate(q, feat, lab, [0, 1], [0, 0], (2, 3), 2, 0.1)
    assert idx.tolist() == [[i, 6 + i] for i in range(6)] and np.array_equal(score[:, 1], np.full(6, np.float32(0.6)))
    T = float(np.float32(0.1))
    w = 1.0 / (1.0 + np.exp((float(np.float32(0.6)) - 1.0) / T))
    assert np.allclose(out[:, 0], w * np.arange(6) / 8.0 + (1 - w), atol=1e-14)
    # a NaN context row is never a neighbour; a NaN query lists nothing and gives zeros
    feat2 = feat.copy(); feat2[0, 0] = np.nan
    _, idx, _ = R.propagate(q, feat2, lab, [0], [-1], (2, 3), 6, 0.1)
    assert not (idx == 0).any() and (idx[:, -1] == -1).all()
    q2 = q.copy(); q2[3] = np.nan
    out, idx, _ = R.propagate(q2, feat, lab, [0], [-1], (2, 3), 2, 0.1)
    assert (idx[3] == -1).all() and not out[3].any()


SQUARE = np.zeros((4, 4), dtype=bool)
SQUARE[2:, 2:] = True                     # touches the last row and the last column


def test_boundary_map_and_dilation_by_hand():
    assert R.bmap(SQUARE).astype(int).tolist() == [[0, 0, 0, 0], [0, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 0]]
    inner = np.zeros((4, 4), dtype=bool); inner[1:3, 1:3] = True
    b = R.bmap(inner)
    assert b.astype(int).tolist() == [[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    assert R.dilate(b, 1).astype(int).tolist() == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]]
    assert np.array_equal(R.dilate(b, 0), b)
    dot = np.zeros((7, 7), dtype=bool); dot[3, 3] = True
    assert R.dilate(dot, 1).sum() == 5 and R.dilate(dot, 2).sum() == 13 and R.dilate(dot, 3).sum() == 29
    pred, gt = np.zeros((1, 4, 4), np.int64), np.zeros((1, 4, 4), np.int64)
    pred[0][inner] = 1; gt[0][SQUARE] = 1
    # bmap(P) has 8 pixels, bmap(G) 5; they share (1, 2) and (2, 1); within one pixel (a plus) only (0, 0) of bmap(P) finds no pixel of bmap(G)
    assert R.jf_counts(pred, gt, 1, 0)[0, 0].tolist() == [1, 7, 8, 5, 2, 2]
    assert R.jf_counts(pred, gt, 1, 1)[0, 0].tolist() == [1, 7, 8, 5, 7, 5]


def test_f_measure_empty_cases():
    counts = np.array([[0, 5, 0, 4, 0, 0], [0, 5, 4, 0, 0, 0], [0, 0, 0, 0, 0, 0], [2, 4, 4, 4, 2, 3]])
    for fn in (R.jf_from_counts, hvideo.jf_from_counts):
        J, F = fn(counts)
        assert J.tolist() == [0.0, 0.0, 1.0, 0.5]
        assert F[:3].tolist() == [0.0, 0.0, 1.0] and abs(F[3] - 0.6) < 1e-15
    assert R.bound_px(480, 854) == hvideo.boundary_bound(480, 854) == 8 and R.bound_px(48, 64) == 1 and hvideo.boundary_bound(53, 90) == 1


# ---- six wrong variants, each against a named check ----------------------------------------------------------------------------------------
def check_square_window(variant):
    q, feat, lab = R.small_world()
    idx, _ = R.lists(q, feat, [0], [1], (3, 4), 12, variant)
    assert (idx[5] >= 0).sum() == 9 and 0 in idx[5]             # cell (1, 1): the 3 x 3 window with its corners


def check_topk_over_the_union(variant):
    q, feat, lab = R.small_world()
    idx, score = R.lists(q, feat, [0, 1, 2], [-1, -1, -1], (3, 4), 2, variant)
    assert idx.shape == (12, 2)
    ctx = feat.reshape(36, -1).astype(np.float64)
    assert np.array_equal(idx, np.argsort(-(q.astype(np.float64) @ ctx.T), axis=1, kind="stable")[:, :2])


def check_ties_to_the_lower_id(variant):
    q, feat, lab = R.small_world()
    idx, score = R.lists(q, feat, [1, 1], [0, 0], (3, 4), 2, variant)
    assert idx.tolist() == [[i, 12 + i] for i in range(12)]


def _norm_world():
    rng = np.random.default_rng(4)
    x = rng.random((1, 12, 3)).astype(np.float32)
    x[0, :, 0] = x[0, :, 0] * np.float32(0.2) + np.float32(0.5)        # a strong, flat background channel
    x[0, :, 1:] *= np.float32(0.4)
    return x


def check_norm_after_the_upsample(variant):
    x = _norm_world()
    got = R.label_map(x, (3, 4), 17, 23, norm=True, variant=variant)
    v = R.upsample(x, (3, 4), 17, 23)[0]
    n = np.stack([((ch - ch.min()) / (ch.max() - ch.min())).astype(np.float32) for ch in v])
    assert np.array_equal(got[0], n.argmax(0))
    assert not np.array_equal(got, R.label_map(x, (3, 4), 17, 23, norm=False))


def check_bmap_edge_rule(variant):
    assert R.bmap(SQUARE, variant).astype(int).tolist() == [[0, 0, 0, 0], [0, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 0]]


def check_disk_dilation(variant):
    dot = np.zeros((7, 7), dtype=bool); dot[3, 3] = True
    assert R.dilate(dot, 2, variant).sum() == 13


CHECKS = {"round_window": check_square_window, "per_frame_topk": check_topk_over_the_union, "tie_high": check_ties_to_the_lower_id,
          "norm_on_grid": check_norm_after_the_upsample, "bmap_no_edge_rule": check_bmap_edge_rule, "square_dilation": check_disk_dilation}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_each_wrong_variant_fails_its_check(variant):
    assert set(CHECKS) == set(R.VARIANTS)
    for check in CHECKS.values():
        check(None)                                              # the definitions pass every check
    with pytest.raises(AssertionError):
        CHECKS[variant](variant)


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------
def test_ring_context_order():
    assert hvideo.ring_context(1, 3) == ([0], [0])
    assert hvideo.ring_context(3, 3) == ([0, 1, 2], [0, 1, 2])
    assert hvideo.ring_context(4, 3) == ([0, 1, 2, 3], [0, 1, 2, 3])
    assert hvideo.ring_context(5, 3) == ([0, 2, 3, 4], [0, 2, 3, 1])                 # frame 4 took frame 1's slot
    assert hvideo.ring_context(8, 3) == ([0, 5, 6, 7], [0, 2, 3, 1])
    assert hvideo.ring_context(9, 0) == ([0], [0])
    for n_last in (0, 1, 3, 7):
        for t in range(1, 20):
            frames, slots = hvideo.ring_context(t, n_last)
            assert (frames, slots) == R.ring_context(t, n_last)
            assert len(set(slots)) == len(slots) == 1 + min(t - 1, n_last) and max(slots) <= n_last
    with pytest.raises(ValueError):
        hvideo.ring_context(0, 3)


def test_video_metrics_from_a_counts_table():
    a = np.array([[[2, 4, 4, 4, 2, 3], [0, 0, 0, 0, 0, 0]], [[3, 4, 4, 4, 4, 4], [0, 5, 4, 0, 0, 0]]])     # 2 frames, 2 objects
    b = np.array([[[1, 4, 2, 2, 1, 1]]])                                                                 # 1 frame, 1 object
    m = hvideo.VideoMetrics({"a": a, "b": b}, skipped=[("c", "2 frames")])
    # object a/1: J 0.5, 0.75, F 0.6, 1; object a/2: J 1, 0, F 1, 0; object b/1: J 0.25, F 0.5
    assert [(r["sequence"], r["object"]) for r in m.per_object] == [("a", 1), ("a", 2), ("b", 1)]
    assert [r["J_mean"] for r in m.per_object] == [0.625, 0.5, 0.25]
    assert np.allclose([r["F_mean"] for r in m.per_object], [0.8, 0.5, 0.5], atol=1e-15)
    assert [r["J_recall"] for r in m.per_object] == [0.5, 0.5, 0.0] and [r["F_recall"] for r in m.per_object] == [1.0, 0.5, 0.0]
    assert abs(m["J_mean"] - (0.625 + 0.5 + 0.25) / 3) < 1e-15 and abs(m["F_mean"] - 0.6) < 1e-15        # over objects, not over sequences
    assert abs(m["J&F"] - 0.5 * (m["J_mean"] + m["F_mean"])) < 1e-15 and set(m) == {"J_mean", "J_recall", "F_mean", "F_recall", "J&F"}
    assert m.per_sequence["a"]["J_mean"] == 0.5625 and m.per_sequence["a"]["n_objects"] == 2 and m.per_sequence["b"]["n_frames"] == 1
    assert m.skipped == [("c", "2 frames")]
    want = R.video_metrics({"a": a, "b": b})
    assert all(abs(m[k] - want[k]) < 1e-15 for k in want)
    with pytest.raises(ValueError):
        hvideo.VideoMetrics({"a": a[:, :, :5]})


def test_evaluator_refuses_bad_settings_without_a_gpu():
    net = torch.nn.Identity()
    for kw in (dict(n_neighbours=0), dict(n_neighbours=33), dict(n_last_frames=-1), dict(n_last_frames=32), dict(radius=-2), dict(temperature=0.0),
               dict(temperature=float("nan")), dict(first_frame_radius=-2), dict(device="cpu")):
        with pytest.raises(ValueError):
            hvideo.HbirdVideoEvaluation(net, 8, **kw)
    with pytest.raises(ValueError):
        hvideo.HbirdVideoEvaluation(net, 0)


def test_synthetic_video_world():
    w = vdata.SyntheticVideoDataModule(n_sequences=2, n_frames=6, seed=3)
    again = vdata.SyntheticVideoDataModule(n_sequences=2, n_frames=6, seed=3)
    seqs = list(w.sequences())
    assert len(seqs) == len(w) == 2
    for (name, frames, ann), (_, f2, a2) in zip(seqs, again.sequences()):
        assert frames.shape == (6, 3, 48, 64) and ann.shape == (6, 48, 64) and ann.dtype == torch.int64 and frames.dtype == torch.float32
        assert torch.equal(frames, f2) and torch.equal(ann, a2)
        assert set(ann[0].unique().tolist()) <= {0, 1, 2} and int(ann[0].max()) >= 1
        assert not torch.equal(ann[0], ann[-1])                                       # the objects move
    assert isinstance(vdata.get_video_dataset("synthetic-video"), vdata.SyntheticVideoDataModule)
    with pytest.raises(ValueError):
        vdata.get_video_dataset("davis")
    with pytest.raises(ValueError):
        vdata.SyntheticVideoDataModule(n_frames=40)


def test_video_folder_on_written_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    h0, w0 = 20, 30
    for seq, n_frames in (("bear", 3), ("camel", 4)):
        os.makedirs(tmp_path / "JPEGImages" / "480p" / seq)
        os.makedirs(tmp_path / "Annotations" / "480p" / seq)
        for t in range(n_frames):
            Image.fromarray(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)).save(tmp_path / "JPEGImages" / "480p" / seq / f"{t:05d}.jpg")
            a = np.zeros((h0, w0), dtype=np.uint8)
            a[2:10, 3 + t:12 + t] = 1
            a[12:18, 20:28] = 2
            m = Image.fromarray(a, mode="P")
            m.putpalette([0, 0, 0, 255, 0, 0, 0, 255, 0] + [0] * (253 * 3))
            if not (seq == "camel" and t == 3):                                       # the last frame of camel has no annotation file
                m.save(tmp_path / "Annotations" / "480p" / seq / f"{t:05d}.png")
    assert vdata.resized_hw(h0, w0, 16, 8) == (16, 24) and vdata.resized_hw(480, 854, 480, 16) == (480, 848)
    dm = vdata.get_video_dataset("video-folder", str(tmp_path), input_size=16, patch_size=8)
    assert dm.names == ["bear", "camel"]
    seqs = list(dm.sequences())
    assert [s[0] for s in seqs] == ["bear", "camel"] and [s[1].shape[0] for s in seqs] == [3, 4]
    for name, frames, ann in seqs:
        assert frames.shape[1:] == (3, 16, 24) and ann.shape[1:] == (16, 24) and ann.dtype == torch.int64 and frames.dtype == torch.float32
        assert set(ann[0].unique().tolist()) == {0, 1, 2}                             # NEAREST: no id is invented
    assert not seqs[1][2][3].any()
    os.makedirs(tmp_path / "ImageSets" / "2017")
    (tmp_path / "ImageSets" / "2017" / "val.txt").write_text("camel\n")
    assert vdata.VideoFolderDataModule(str(tmp_path), 16, 8).names == ["camel"]
    (tmp_path / "ImageSets" / "2017" / "val.txt").write_text("camel\nzebra\n")
    with pytest.raises(RuntimeError, match="zebra"):
        vdata.VideoFolderDataModule(str(tmp_path), 16, 8)
    with pytest.raises(RuntimeError, match="not found"):
        vdata.VideoFolderDataModule(str(tmp_path / "JPEGImages"), 16, 8)


def test_cli_video_parser_and_refusals(capsys):
    cli = _cli()
    base = ["--dataset-name", "synthetic-video", "--data-dir", "", "--d-model", "3", "--patch-size", "8"]
    a = cli.build_parser().parse_args(base + ["--task", "video"])
    assert (a.task, a.video_last_frames, a.video_radius, a.video_first_frame_radius, a.video_temperature, a.no_channel_norm) == ("video", 7, 12, None, 0.1, False)
    assert a.n_neighbours == 30 and isinstance(a.n_neighbours, cli._DefaultInt)       # 5 for this task unless given (main_video)
    a = cli.build_parser().parse_args(base + ["--task", "video", "--video-last-frames", "0", "--video-radius", "-1", "--video-first-frame-radius", "3",
                                              "--video-temperature", "0.07", "--no-channel-norm", "--n-neighbours", "30"])
    assert (a.video_last_frames, a.video_radius, a.video_first_frame_radius, a.video_temperature, a.no_channel_norm) == (0, -1, 3, 0.07, True)
    assert not isinstance(a.n_neighbours, cli._DefaultInt)
    for bad in (["--video-last-frames", "-1"], ["--video-radius", "-2"], ["--video-temperature", "0"], ["--task", "videos"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + ["--task", "video"] + bad)
    for bad, word in ((["--grid-k", "1", "5"], "--grid-k"), (["--bootstrap", "100"], "--bootstrap"), (["--memory-size", "100"], "--memory-size"),
                      (["--leave-one-out"], "--leave-one-out"), (["--linear-probe"], "--linear-probe"), (["--nn-method", "faiss"], "--nn-method"),
                      (["--target-grid", "2"], "--target-grid"), (["--frame-size", "64", "64"], "--frame-size"), (["--train-fs", "x.txt"], "--train-fs")):
        with pytest.raises(SystemExit):
            cli.main(base + ["--task", "video"] + bad)
        assert word in capsys.readouterr().err and True
    for task in ([], ["--task", "depth"]):
        for opt in (["--video-radius", "3"], ["--video-last-frames", "2"], ["--no-channel-norm"], ["--video-temperature", "0.5"],
                    ["--video-first-frame-radius", "-1"]):
            with pytest.raises(SystemExit):
                cli.main(base + task + opt)
            assert "needs --task video" in capsys.readouterr().err
