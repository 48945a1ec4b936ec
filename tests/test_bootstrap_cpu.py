"""Bootstrap intervals without a GPU: the restatements of tests/bootstrap_refs.py against their own definitions and against one wrong variant
each (the GPU tests hold the kernels to these restatements), the C ABI of include/hbird_hip_bootstrap.h against its bindings, the arithmetic
of `MiouBootstrap` on hand-made samples, and eval.py's flags and JSON fields."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import bootstrap_refs as br
from hbird_mi import _lib
from hbird_mi import bootstrap as hboot
from hbird_mi.utils.eval_metrics import PredsmIoU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hb_image_class_counts", "hb_bootstrap_multiplicities", "hb_bootstrap_counts", "hb_bootstrap_miou"}
C_TYPES = {"const int64_t*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p,
           "double*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}


def _eval_module():
    spec = importlib.util.spec_from_file_location("hbird_eval_cli", os.path.join(ROOT, "eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the resampler ------------------------------------------------------------------------------------------------------------------------
def test_resampler_rows_sum_to_n_and_the_vector_form_is_the_integer_definition():
    for N in (1, 24, 1000, 32768):
        W = br.multiplicities(br.SEED, 3, 4, N)
        assert W.shape == (4, N) and W.dtype == np.int32 and (W.sum(axis=1) == N).all() and W.min() >= 0
        d = br.draws(br.SEED, 5, N)
        assert d.min() >= 0 and d.max() < N
        for j in sorted({0, 1 % N, N // 2, N - 1}):
            assert int(d[j]) == br.draw_int(br.SEED, 5, j, N)
    # splitmix64's published first outputs for the state 0 (the stream of Vigna's splitmix64.c is splitmix(0), splitmix(gamma), ...)
    assert br.splitmix_int(0) == 0xE220A8397B1DCDAF and br.splitmix_int(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_resampler_moments_at_the_committed_seed():
    assert br.SEED == hboot.DEFAULT_SEED
    R, N = 4096, 24
    W = br.multiplicities(br.SEED, 0, R, N)
    assert (W.sum(axis=1) == N).all()
    # a multiplicity is Binomial(N, 1/N): mean 1, variance 1 - 1/N; 0.1 is about 6.5 sigma of the mean of R of them
    assert 0.1 / np.sqrt((1 - 1 / N) / R) > 6.5
    assert np.abs(W.mean(axis=0) - 1.0).max() < 0.1
    assert len({tuple(row) for row in W[:64]}) == 64        # replicates differ


def test_draws_that_depend_on_the_configuration_fail_the_comparison():
    good = br.multiplicities(br.SEED, 0, 7, 24)
    assert np.array_equal(good, br.multiplicities(br.SEED, 0, 7, 24, cfg=None))
    assert np.array_equal(good[5:7], br.multiplicities(br.SEED, 5, 2, 24))       # ... nor on where a chunk of replicates starts
    assert not np.array_equal(good, br.multiplicities(br.SEED, 0, 7, 24, cfg=1))


# ---- counts --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "blocks"])
def test_image_counts_restatement_and_the_fp_on_gt_variant(kind):
    G = 5
    gt, pred = br.maps(3, 37, 53, G, kind, seed=11)
    got = br.image_counts(gt, pred, G, ignore=255)
    assert got.shape == (3, G, 3) and not got[1].any() and got[0].any() and got[2].any()
    # pixel by pixel, from the definition
    want = np.zeros((3, G, 3), dtype=np.int64)
    for b in range(3):
        for g, p in zip(gt[b].reshape(-1).tolist(), pred[b].reshape(-1).tolist()):
            if g == 255 or not (0 <= g < G and 0 <= p < G):
                continue
            if g == p:
                want[b, g, 0] += 1
            else:
                want[b, p, 1] += 1
                want[b, g, 2] += 1
    assert np.array_equal(got, want)
    assert got[:, :, 1].sum() == got[:, :, 2].sum()                                # every miss is one fp and one fn
    wrong = br.image_counts(gt, pred, G, ignore=255, fp_on_gt=True)
    assert not np.array_equal(wrong, want) and np.array_equal(wrong[:, :, [0, 2]], want[:, :, [0, 2]])


def test_a_32_bit_accumulator_fails_the_comparison():
    stats = np.full((8, 6), 2 ** 31 - 1, dtype=np.int32)
    W = br.multiplicities(br.SEED, 0, 5, 8)
    good = br.counts(W, stats)
    assert (good == 8 * (2 ** 31 - 1)).all() and good.min() > 2 ** 32
    assert not np.array_equal(br.counts(W, stats, acc32=True), good)


def test_a_pairwise_mean_fails_the_bit_comparison_and_stays_within_the_bound():
    G, n_cfg = 151, 3
    stats = br.stats_table(1000, n_cfg, G, seed=7, absent_class=4)
    cnt = br.counts(br.multiplicities(br.SEED, 0, 33, 1000), stats)
    seq, pair = br.miou_rows(cnt, n_cfg, G), br.miou_rows(cnt, n_cfg, G, pairwise=True)
    assert not np.array_equal(seq, pair)
    assert np.abs(seq - pair).max() <= G * 2.0 ** -52
    # ... and the pairwise form is PredsmIoU._miou_from_counts
    c = cnt.reshape(33, n_cfg, G, 3)
    assert pair[2, 1] == PredsmIoU._miou_from_counts(c[2, 1, :, 0], c[2, 1, :, 1], c[2, 1, :, 2])
    # the sequential form, one scalar at a time
    s = 0.0
    for g in range(G):
        tp, fp, fn = (float(v) for v in c[4, 2, g])
        s = s + tp / max(tp + fp + fn, 1e-8)
    assert seq[4, 2] == s / G


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
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


def test_bootstrap_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "hbird_hip_bootstrap.h")).read()
    main = open(os.path.join(ROOT, "include", "hbird_hip.h")).read()
    decl = _declarations(header)
    assert set(decl) == NAMES == set(_lib.SIGNATURES_BOOTSTRAP)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_CENTRE) | set(_lib.SIGNATURES_SELECT) | set(_lib.SIGNATURES_GRID) | set(_lib.SIGNATURES_EXCLUDE)
              | set(_lib.SIGNATURES_SCREEN) | set(_lib.SIGNATURES_EXCLUDE_SCREEN))
    assert not NAMES & others
    assert "hbird_hip_bootstrap.h" not in main and not [n for n in NAMES if n in main]     # a header of its own
    L = _lib.lib()
    for name, (ret, params) in decl.items():
        res, argtypes = _lib.SIGNATURES_BOOTSTRAP[name]
        assert ret == "int" and res is ctypes.c_int
        assert [C_TYPES[typ] for typ, _ in params] == argtypes, (name, params)
        fn = getattr(L, name)
        assert fn.argtypes == argtypes and fn.restype is res
        assert params[-1] == ("void*", "stream")
    assert [a for _, a in decl["hb_image_class_counts"][1]] == ["gt", "pred", "B", "h", "w", "G", "ignore", "has_ignore", "out", "row_stride", "stream"]
    assert [a for _, a in decl["hb_bootstrap_multiplicities"][1]] == ["n_img", "seed", "r0", "R", "out", "stream"]
    assert [a for _, a in decl["hb_bootstrap_counts"][1]] == ["stats", "n_img", "cols", "W", "R", "out", "stream"]
    assert [a for _, a in decl["hb_bootstrap_miou"][1]] == ["stats", "n_img", "n_cfg", "G", "seed", "R", "out_point", "out_samples", "chunk_replicates",
                                                            "stream"]
    assert int(re.search(r"#define HB_BOOTSTRAP_MAX_IMAGES (\d+)", header).group(1)) == _lib.BOOTSTRAP_MAX_IMAGES == 32768
    assert int(re.search(r"#define HB_BOOTSTRAP_MAX_REPLICATES (\d+)", header).group(1)) == _lib.BOOTSTRAP_MAX_REPLICATES == 1 << 20


def test_bootstrap_unit_is_built_outside_the_pinned_units_and_names_its_kernels_apart():
    csrc = os.path.join(ROOT, "open-hummingbird-eval_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hbird_bootstrap.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_bootstrap" not in re.search(r"^KNN_UNITS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_bootstrap" not in re.search(r"^K5_UNITS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "hbird_hip_bootstrap.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(csrc, "hbird_bootstrap.hip")).read()
    kernels = re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src)
    assert {"image_class_counts_kernel", "bootstrap_multiplicities_kernel", "bootstrap_counts_kernel", "bootstrap_miou_kernel"} <= set(kernels)
    assert not [k for k in kernels if k.startswith(("knn_", "aggregate_", "rerank_"))]
    assert "rocblas" not in src.lower() and "hipblas" not in src.lower()


def test_bootstrap_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.hb_bootstrap_multiplicities(_lib.BOOTSTRAP_MAX_IMAGES + 1, 1, 0, 1, None, None) != 0
    assert "32769 images" in _lib.last_error() and "32768" in _lib.last_error()
    assert L.hb_bootstrap_multiplicities(24, 1, (1 << 20) - 1, 2, None, None) != 0 and "2^20" in _lib.last_error()
    assert L.hb_bootstrap_counts(None, 4, 4, None, 1, None, None) != 0 and "NULL" in _lib.last_error()
    assert L.hb_bootstrap_miou(None, 4, 1, 5, 1, 1, None, None, 0, None) != 0 and "NULL" in _lib.last_error()
    assert L.hb_image_class_counts(None, None, 1, 4, 4, 5, 0, 0, None, 15, None) != 0 and "NULL" in _lib.last_error()


# ---- MiouBootstrap --------------------------------------------------------------------------------------------------------------------------
def _hand_made():
    rng = np.random.default_rng(3)
    base = rng.normal(0.5, 0.02, size=400)
    samples = np.stack([base, base + 0.05 + rng.normal(0, 0.001, 400), base + 0.049 + rng.normal(0, 0.01, 400), base - 0.2], axis=1)
    keys = [(3, 0.02), (10, 0.02), (10, 0.1), (40, 0.02)]
    miou = {keys[0]: 0.5, keys[1]: 0.55, keys[2]: 0.549, keys[3]: 0.3}
    return hboot.MiouBootstrap(keys=keys, miou=miou, point=torch.tensor([0.5, 0.55, 0.549, 0.3], dtype=torch.float64), samples=samples, seed=9,
                               n_images=24, matching_is_identity={k: True for k in keys})


def test_miou_bootstrap_arithmetic_on_hand_made_samples():
    mb = _hand_made()
    s = mb.samples
    assert np.array_equal(mb.interval((10, 0.02)), np.quantile(s[:, 1], [(1 - 0.95) / 2, (1 + 0.95) / 2]))
    assert np.array_equal(mb.interval((3, 0.02), level=0.5), np.quantile(s[:, 0], [(1 - 0.5) / 2, (1 + 0.5) / 2]))
    d, lo, hi, share = mb.difference((10, 0.02), (3, 0.02))
    q = np.quantile(s[:, 1] - s[:, 0], [(1 - 0.95) / 2, (1 + 0.95) / 2])
    assert d == 0.55 - 0.5 and (lo, hi) == (q[0], q[1]) and share == 1.0 and lo > 0
    # the paired interval of the difference is far tighter than the two marginal intervals suggest
    assert hi - lo < 0.1 * (mb.interval((10, 0.02))[1] - mb.interval((10, 0.02))[0])
    _, lo2, hi2, share2 = mb.difference((10, 0.02), (10, 0.1))
    assert lo2 < 0 < hi2 and share2 == float((s[:, 1] > s[:, 2]).mean())
    assert mb.best() == ((10, 0.02), [(10, 0.1)])
    with pytest.raises(KeyError):
        mb.interval((11, 0.02))


def test_parse_bootstrap():
    assert hboot.parse_bootstrap(None) is None
    assert hboot.parse_bootstrap(200) == (200, hboot.DEFAULT_SEED) and hboot.parse_bootstrap((50, 7)) == (50, 7)
    assert hboot.parse_bootstrap((50, None)) == (50, hboot.DEFAULT_SEED)
    for bad in (0, -3, 2.5, (1 << 20) + 1, True, (5,), (5, -1), (5, 1 << 64)):
        with pytest.raises(ValueError):
            hboot.parse_bootstrap(bad)


# ---- eval.py --------------------------------------------------------------------------------------------------------------------------------
def test_eval_cli_flags_and_json_fields(capsys):
    ev = _eval_module()
    base = ["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8"]
    a = ev.build_parser().parse_args(base)
    assert a.bootstrap is None and a.bootstrap_seed is None and a.bootstrap_level == 0.95
    a = ev.build_parser().parse_args(base + ["--bootstrap", "500", "--bootstrap-seed", "7", "--bootstrap-level", "0.9"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level) == (500, 7, 0.9)
    for bad in (["--bootstrap", "0"], ["--bootstrap-level", "1.0"], ["--bootstrap-level", "0"]):
        with pytest.raises(SystemExit):
            ev.build_parser().parse_args(base + bad)
    with pytest.raises(SystemExit):
        ev.main(base + ["--bootstrap-seed", "7"])
    assert "--bootstrap-seed needs --bootstrap" in capsys.readouterr().err
    mb = _hand_made()
    head = ev.headline_key(mb.keys, 10, None)
    assert head == (10, 0.02) and ev.headline_key(mb.keys, 30, None) == (3, 0.02)
    out = ev.bootstrap_summary(mb, 0.95, head)
    assert set(out) == {"miou_ci", "bootstrap", "miou_grid_ci", "grid_best", "grid_indistinguishable_from_best"}
    assert out["miou_ci"] == list(mb.interval(head)) and set(out["miou_grid_ci"]) == {ev.grid_key(*k) for k in mb.keys}
    assert out["grid_best"] == "k=10,beta=0.02" and out["grid_indistinguishable_from_best"] == ["k=10,beta=0.1"]
    assert out["bootstrap"] == {"replicates": 400, "seed": 9, "level": 0.95, "n_images": 24, "matching_is_identity": True}
    assert ev.bootstrap_as_plain(mb, True, False) == mb.miou and ev.bootstrap_as_plain(mb, False, False) == 0.5
    # one configuration: an interval, no grid fields; memory sizes: keys carry the size
    one = hboot.MiouBootstrap(keys=[(30, 0.02)], miou={(30, 0.02): 0.5}, point=mb.point[:1], samples=mb.samples[:, :1], seed=9, n_images=24,
                              matching_is_identity={(30, 0.02): False})
    out1 = ev.bootstrap_summary(one, 0.9, (30, 0.02))
    assert set(out1) == {"miou_ci", "bootstrap"} and out1["bootstrap"]["matching_is_identity"] is False
    sized = hboot.MiouBootstrap(keys=[(96, 30, 0.02), (216, 30, 0.02)], miou={(96, 30, 0.02): 0.4, (216, 30, 0.02): 0.5}, point=mb.point[:2],
                                samples=mb.samples[:, [0, 1]], seed=9, n_images=24, matching_is_identity={(96, 30, 0.02): True, (216, 30, 0.02): True})
    assert ev.headline_key(sized.keys, 30, 216) == (216, 30, 0.02) and ev.headline_key(sized.keys, 30, 500) == (216, 30, 0.02)
    assert ev.bootstrap_summary(sized, 0.95, (216, 30, 0.02))["grid_best"] == "memory_size=216,k=30,beta=0.02"
    assert ev.bootstrap_as_plain(sized, False, True) == {96: 0.4, 216: 0.5}
    assert ev.bootstrap_as_plain(sized, True, True) == {96: {(30, 0.02): 0.4}, 216: {(30, 0.02): 0.5}}
