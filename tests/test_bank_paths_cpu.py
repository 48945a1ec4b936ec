"""tests/bank_refs.py against `oracle` and against itself, the launch arithmetic of the bank-side kernels restated so that the case lists
of tests/test_bank_paths_gpu.py provably reach every regime, the argument checks that come before any GPU call, and -- on the host,
before any GPU time is spent -- the proof that the committed inputs can see the errors they are meant to catch: for each kernel a
deliberately wrong variant of its reference disagrees with the right one on at least one committed case.
"""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bank_refs as R
import oracle
import test_bank_paths_gpu as G

F32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "open-hummingbird-eval_amd", "csrc")


# ---------------------------------------------------------------- the references against `oracle` and against each other

def test_label_hist_agrees_with_the_oracle():
    for i, c in enumerate(G.K2_CASES):
        y = G.k2_mask(c, 100 + i)
        ref = R.label_hist(y, c.ps, c.C, c.map255)
        y0 = np.where(y == 255, 0, y) if c.map255 else y
        assert np.array_equal(ref.view(np.uint32), oracle.patch_label_hist(y0, c.ps, c.C).view(np.uint32)), c
        counts = R.label_counts(y, c.ps, c.C, c.map255)
        assert (counts.sum(axis=-1) == c.ps * c.ps).all() and ref.shape == (c.B, c.H // c.ps, c.W // c.ps, c.C)
        if c.C > 255:                                  # 255 is a legal class there: mapped to 0 with map255, kept without
            assert (y == 255).any() and (counts[..., 255].sum() == 0) == c.map255
    with pytest.raises(R.ClassRange):
        R.label_hist(np.full((1, 1, 2, 2), 255), 2, 64)
    assert R.label_hist(np.full((1, 1, 2, 2), 255), 2, 64, map255=True)[0, 0, 0, 0] == 1.0
    with pytest.raises(ValueError):
        oracle.patch_label_hist(np.full((1, 1, 2, 2), 64), 2, 64)


def test_patch_scores_and_select_agree_with_the_oracle_where_no_patch_is_empty():
    """oracle.sample_patches indexes by class id and cannot express an empty patch; on masks (no empties) the two definitions agree."""
    rng = np.random.default_rng(5)
    for ps, C, B, S, K in ((4, 21, 3, 6, 10), (2, 151, 2, 9, 81), (7, 5, 4, 5, 1)):
        y = rng.integers(0, min(C, 9), size=(B, 1, S * ps, S * ps), dtype=np.int64)
        lab = R.label_hist(y, ps, C).reshape(B, S * S, C)
        scores, nonempty, nz, _ = R.patch_scores(lab)
        assert nz.tolist() == [S * S] * B and nonempty.all()
        r = rng.random(B * S * S, dtype=F32)
        pt = oracle.patchify_gt(y, ps)
        oidx, oscores = oracle.sample_patches(pt, C, K, np.ones_like(r))
        assert np.array_equal(scores, oscores)
        idx, noisy = R.patch_select(scores, nonempty, r, np.arange(B) * S * S, K)
        oidx, onoisy = oracle.sample_patches(pt, C, K, r)
        assert np.array_equal(idx, oidx) and np.array_equal(noisy.view(np.uint32), onoisy.view(np.uint32))
        assert np.array_equal(oracle.sample_num_nonempty(pt, C), nz)


def test_presence_is_ieee_greater_than_zero():
    lab = G.k3a_special_rows()
    scores, nonempty, nz, freq = R.patch_scores(lab)
    assert nonempty.tolist() == [[0, 0, 0, 1, 1, 1, 0], [0, 0, 1, 0, 0, 0, 1]] and nz.tolist() == [3, 2]
    assert freq.tolist() == [[1, 0, 0, 3, 0], [1, 0, 0, 0, 2]]
    assert scores[0].tolist() == [1e6, 1e6, 1e6, 3.0, 4.0, 3.0, 1e6] and scores[1, 2] == 2.0 and scores[1, 6] == 3.0


def test_tie_products_collide_exactly_in_fp32():
    scores, nonempty, r, r_off = G.k3b_tie_inputs()
    assert all(F32(a) * F32(b) == F32(2.0) for a, b in ((4, 0.5), (8, 0.25), (2, 1.0), (16, 0.125)))
    noisy = R.noisy_scores(scores, nonempty, r, r_off)
    vals, counts = np.unique(noisy, return_counts=True)
    assert vals.tolist() == [2.0, 4.0, 1e6] and counts.tolist() == [300, 244, 56]


def test_normalized_agrees_with_the_oracle_and_ambiguous_rows_are_rare():
    """The K1 inputs of the GPU file: the share of rows where the order of the double sum could move a rounded norm is at most
    0.01 % of each input (the condition under which the GPU comparison is on bits), and on every other row the pairwise sum used
    here, the sequential sum of the oracle and an 8-way strided sum give the same norm."""
    total = flagged = 0
    inputs = [G.k1_rows(D) for D in G.K1_D] + [G.k1_rows(D, seed=3) for D in G.K1_FORM_D] + [G.k1_rows(D, seed=4)[:700] for D in G.K1_OFFSET_D]
    inputs += [G.scaled_rows(sum(G.K1_GROWTH_PIECES), D, 7000 + D) for D in G.K1_GROWTH_D] + [G.k1_rows(D, seed=2)[:3] for D in G.K1_GROWTH_D]
    n_big, d_big = G.K1_BIG_HOST
    rng = np.random.default_rng(123)
    big = rng.standard_normal((n_big, d_big), dtype=F32)
    big *= np.exp(rng.normal(0.0, 1.0, size=(n_big, 1))).astype(F32)
    inputs += [big[lo:lo + 1000] for lo in (0, (256 << 20) // (d_big * 4) - 500, n_big - 1000)]
    for x in inputs:
        for normalize in (True, False):
            amb = R.ambiguous(x, normalize)
            assert amb.mean() <= 1e-4, (x.shape, normalize, int(amb.sum()))
            total += len(x)
            flagged += int(amb.sum())
        ok = ~R.ambiguous(x, True)
        assert np.array_equal(R.normalized(x)[ok].view(np.uint32), oracle.normalize_rows(x)[ok].view(np.uint32))
        x64 = x.astype(np.float64) ** 2
        pad = (-x.shape[1]) % 8
        strided = np.pad(x64, ((0, 0), (0, pad))).reshape(len(x), -1, 8).sum(axis=1).sum(axis=1)
        assert np.array_equal(np.sqrt(strided).astype(F32)[ok], R.norm32(x)[ok])
    assert total > 80000 and flagged <= total * 1e-4
    x = G.scaled_rows(50, 40, 1)
    assert np.array_equal(R.stored_norm(x, False), R.norm32(x)) and np.array_equal(R.stored_rows(x, False), x)
    assert np.isnan(R.normalized(np.zeros((1, 4), dtype=F32))).all()
    assert R.ulp_distance(F32([1.0, -0.0, 1.0]), F32([np.nextafter(F32(1.0), F32(2.0)), 0.0, 1.0])).tolist() == [1, 0, 0]


def _merge_slow(val, idx, metric):
    """The merge, one query at a time with Python's sorted()."""
    parts, nq, k = val.shape
    oi, od = np.empty((nq, k), dtype=np.int64), np.empty((nq, k), dtype=F32)
    for q in range(nq):
        cand = [(bool(idx[p, q, j] < 0), 0.0 if idx[p, q, j] < 0 else float(val[p, q, j] if metric == 1 else -val[p, q, j]) + 0.0,
                 0 if idx[p, q, j] < 0 else int(idx[p, q, j]), p * k + j, p, j) for p in range(parts) for j in range(k)]
        for slot, (miss, _, _, _, p, j) in enumerate(sorted(cand)[:k]):
            oi[q, slot] = -1 if miss else idx[p, q, j]
            od[q, slot] = (np.inf if metric == 1 else -np.inf) if miss else val[p, q, j]
    return oi, od


def test_merge_reference_against_a_per_query_sort():
    for i, c in enumerate(G.MERGE_CASES):
        val, idx = G.merge_inputs(c, 600 + i)
        key = val if c.metric == 1 else -val
        present = idx >= 0
        if c.pattern not in ("missing", "allmissing"):      # each part's list is sorted best first, as a search leaves it
            assert (np.diff(key, axis=-1) >= 0).all() and present.all()
        if c.parts * c.k * c.nq > 400000:
            val, idx = val[:, :40], idx[:, :40]
        ri, rd = R.merge(val, idx, c.metric)
        si, sd = _merge_slow(val, idx, c.metric)
        assert np.array_equal(ri, si) and np.array_equal(rd.view(np.uint32), sd.view(np.uint32)), c
    # the rules, one by one: missing last whatever it carries; -0.0 == +0.0 (the id decides); the same id twice, in part order
    val = F32([[[5.0, np.inf]], [[-0.0, 1.0]], [[0.0, 0.0]]])
    idx = np.array([[[7, -1]], [[9, 3]], [[4, 9]]])
    ri, rd = R.merge(val, idx, 0)
    assert ri.tolist() == [[7, 3]] and rd.tolist() == [[5.0, 1.0]]
    ri, rd = R.merge(val, idx, 1)
    assert ri.tolist() == [[4, 9]] and np.signbit(rd).tolist() == [[False, True]]
    ri, rd = R.merge(F32([[[1.0]], [[2.0]]]), np.array([[[-1]], [[-5]]]), 1)
    assert ri.tolist() == [[-1]] and rd.tolist() == [[np.inf]]


def test_fma_reference_is_correctly_rounded():
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.standard_normal(4000).astype(F32) * F32(10.0) ** rng.integers(-20, 20, 4000).astype(F32),
                        F32([1.0, 1.0 + 2.0 ** -23, 3.0, 0.5])])
    c = np.concatenate([np.abs(rng.standard_normal(4000)).astype(F32) * F32(10.0) ** rng.integers(-20, 20, 4000).astype(F32),
                        F32([2.0 ** -25, 2.0 ** -24, 2.0 ** -48, 2.0 ** -30])])
    got = R.fma_f32(F32(-2.0), s, c)
    for a, b, g in zip(s.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(-2) * Fraction(a) + Fraction(b)
        lo, hi = np.nextafter(F32(g), F32(-np.inf)), np.nextafter(F32(g), F32(np.inf))
        err = abs(Fraction(g) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert (np.float32(g).view(np.uint32) & 1) == 0 or err == 0          # a tie goes to the even mantissa
    q = G.k1_queries(24, nq=3)
    d = R.scores_to_l2(F32([[-np.inf, 0.0, 1e30]] * 3), q)
    assert np.isinf(d[:, 0]).all() and np.array_equal(d[:, 1], oracle.chain_sqnorm(q)) and (d[:, 2] == 0).all() and not np.signbit(d).any()


# ---------------------------------------------------------------- the dispatch, restated from the launch code

K1L_MAX_D = 1152                                   # hbird_layout.hip: K1L_MAX_D
HB_KC = 16                                         # hbird_schedule.h:11 (Dp = D rounded up to HB_KC, hbird_capi.hip:72)


def k1_plan(D, aligned=True, form=0):
    """hb_launch_rows_to_tiles (hbird_layout.hip:240-255): the LDS form for g_layout_form == 0 (forms 0, 8, 16, 32 of
    hb_set_layout_form), D % 16 == 0, D == Dp, D <= K1L_MAX_D and a 16-byte aligned source; rows per workgroup forced by the form or
    32 / 16 / 8 by the width (D <= 192, D <= 828, else); the first form otherwise."""
    dp = (D + HB_KC - 1) // HB_KC * HB_KC
    if form != 1 and D % 16 == 0 and D == dp and D <= K1L_MAX_D and aligned:
        rows = form if form > 1 else (32 if D <= 192 else 16 if D <= 828 else 8)
        assert rows * (D + 4) * 4 <= 160 * 1024
        return f"lds{rows}"
    return "first"


def k1_first_form_norm_branch(D, aligned):
    """rows_to_tiles_kernel pass 1 (hbird_layout.hip:45-62): groups of four for D % 4 == 0 -- by one 16-byte load from an aligned row, by
    four 4-byte loads otherwise --, the strided scalar loop for every other width."""
    return ("quad16" if aligned else "quad4") if D % 4 == 0 else "scalar"


def test_k1_cases_reach_every_form_and_declare_what_the_launcher_picks():
    assert set(G.K1_REGIME) == set(G.K1_D)
    for D in G.K1_D:
        assert k1_plan(D) == G.K1_REGIME[D], D
    # every GPU case of a width runs a normalised bank, a plain bank and queries of that width (check_index searches every index)
    possible = {k1_plan(D) for D in range(1, 2049)}
    assert possible == {"first", "lds32", "lds16", "lds8"} == set(G.K1_REGIME.values())
    # both sides of every boundary
    for lo, hi in ((192, 208), (816, 832), (1152, 1168)):
        assert lo in G.K1_D and hi in G.K1_D and k1_plan(lo) != k1_plan(hi) and all(k1_plan(d) in ("first", k1_plan(lo)) for d in range(lo, hi))
    assert any(D < 8 for D in G.K1_D) and any(D % 8 and D > 8 for D in G.K1_D) and any(D % 16 == 8 for D in G.K1_D)
    # the first form for each of its reasons: width not a multiple of 16, width beyond the LDS form, unaligned source, forced
    first = [D for D in G.K1_D if k1_plan(D) == "first"]
    assert any(D % 16 for D in first) and any(D % 16 == 0 and D > K1L_MAX_D for D in first)
    assert {k1_first_form_norm_branch(D, True) for D in first} == {"quad16", "scalar"}
    assert all(k1_plan(D, aligned=False) == "first" for D in G.K1_OFFSET_D)
    assert {k1_first_form_norm_branch(D, False) for D in G.K1_OFFSET_D} == {"quad4"}
    assert any(k1_plan(D) != "first" for D in G.K1_OFFSET_D) and any(k1_plan(D) == "first" for D in G.K1_OFFSET_D)
    # forced forms: every rows-per-workgroup choice at every forced width, and the first form where the LDS form would apply
    assert set(G.K1_FORMS) == {0, 1, 8, 16, 32}
    assert {k1_plan(D, form=f) for D in G.K1_FORM_D for f in G.K1_FORMS} == {"first", "lds8", "lds16", "lds32"}
    assert all(k1_plan(D) != "first" for D in G.K1_FORM_D) and max(G.K1_FORM_D) == K1L_MAX_D
    # appends behind every row0 % 32, pieces that span row tiles, and a host add beyond one 256 MiB staging chunk
    starts = np.concatenate([[0], np.cumsum(G.K1_PIECES)[:-1]])
    assert {0, 1} == set((starts % 32).tolist()) and max(G.K1_PIECES) > 256 and {1, 31, 32, 33, 255, 257, 1000} == set(G.K1_PIECES)
    gstarts = np.concatenate([[0], np.cumsum(G.K1_GROWTH_PIECES)[:-1]])
    assert set((gstarts % 32).tolist()) == set(range(32))                   # a piece behind every row0 % 32
    caps, cap, total = [], 256, 0                                           # hb_index_add grows to max(need, 1.5 x capacity), in tiles of 256 rows
    for n in G.K1_GROWTH_PIECES:
        total += n
        if total > cap:
            cap = (max(total, cap + cap // 2) + 255) // 256 * 256
            caps.append(cap)
    assert len(caps) >= 2
    assert {k1_plan(D) for D in G.K1_GROWTH_D} == {"first", "lds32", "lds16", "lds8"}     # ... in every form
    n, D = G.K1_BIG_HOST
    assert n * D * 4 > 256 << 20 and k1_plan(D) == "lds8"


def test_dynamic_lds_of_k1_and_k3b_stays_16_byte_aligned():
    """rows_to_tiles_lds_kernel (which reads and writes its dynamic LDS as float4) and patch_select_kernel each declare exactly ONE static
    __shared__ array beside the dynamic one, and its size -- from the declared type and extent, for every instantiated ROWS -- is a multiple
    of 16 bytes, so the dynamic array keeps its 16-byte alignment wherever the compiler places the static one.  A second static array, a
    wider element type or another extent is what fails here."""
    sizeof = {"float": 4, "int": 4, "unsigned": 4, "double": 8, "int64_t": 8, "char": 1, "short": 2, "uint16_t": 2}

    def static_shared(path, kernel):
        src = open(os.path.join(CSRC, path)).read()
        body = src[src.index(kernel):]
        body = body[:body.index("\n}\n")]
        assert body.count("__shared__") == 2 and "extern __shared__ __attribute__((aligned(16)))" in body       # the dynamic array + one static
        (decl,) = re.findall(r"^\s*__shared__\s+(\w+)\s+(\w+)\[(\w+)\];", body, flags=re.M)
        return decl

    typ, name, extent = static_shared("hbird_layout.hip", "void rows_to_tiles_lds_kernel(")
    assert (name, extent) == ("s_scale", "ROWS")
    layout = open(os.path.join(CSRC, "hbird_layout.hip")).read()
    rows = {int(r) for r in re.findall(r"rows_to_tiles_lds_kernel<(?:true|false), (?:true|false), (\d+)>", layout)}
    assert rows == {8, 16, 32}
    assert sorted(sizeof[typ] * r for r in rows) == [32, 64, 128] and all(sizeof[typ] * r % 16 == 0 for r in rows)
    typ, name, extent = static_shared("hbird_bank.hip", "void patch_select_kernel(")
    assert name == "wave_sum" and sizeof[typ] * int(extent) == 16


HIPCC = shutil.which("hipcc") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc: reads the disassembly of hbird_layout.hip")
def test_k1_first_form_reads_unaligned_rows_by_single_dword_loads(tmp_path):
    """The compiler merges four adjacent 4-byte loads into one global_load_dwordx4 whatever the pointer's alignment, which folds the
    aligned and the unaligned arm of rows_to_tiles_kernel's pass 1 into one.  The unaligned arm's loads are therefore volatile; here the
    disassembly of both bank instantiations (the project's flags) must hold: a loop whose only vector-memory loads are four volatile
    (sc0 sc1) SINGLE-dword loads at offsets 0 / 4 / 8 / 12, no volatile load wider than a dword anywhere, and the 16-byte load of the
    aligned arm in another block.  The query instantiation needs no norm and holds neither."""
    out = str(tmp_path / "layout.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(CSRC, "hbird_layout.hip"), "-o", out],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    asm = open(out).read()
    bodies = {}
    for m in re.finditer(r"^(_Z20rows_to_tiles_kernelILb([01])ELb([01])EE\w+):.*?^\s+s_endpgm", asm, flags=re.M | re.S):
        bodies[(m.group(2), m.group(3))] = m.group(0)
    assert set(bodies) == {("1", "1"), ("0", "1"), ("0", "0")}
    load = re.compile(r"^\s+((?:flat|global|buffer)_load_\w+)\s+(.*)$", flags=re.M)
    for key, body in bodies.items():
        loads = [(op, args) for op, args in load.findall(body)]
        volatile = [(op, args) for op, args in loads if "sc0 sc1" in args]
        assert all(op.endswith("_load_dword") for op, _ in volatile), (key, volatile)          # never dwordx2 / x3 / x4
        if key == ("0", "0"):
            assert not volatile and not any("dwordx4" in op for op, _ in loads)
            continue
        blocks = re.split(r"^\.LBB\w+:.*$", body, flags=re.M)
        quad = [b for b in blocks if sum("sc0 sc1" in a for _, a in load.findall(b)) == 4]
        assert len(quad) == 1, key
        in_loop = load.findall(quad[0])
        assert len(in_loop) == 4 and all(op.endswith("_load_dword") for op, _ in in_loop), (key, in_loop)
        offsets = sorted(int(re.search(r"offset:(-?\d+)", a).group(1)) if "offset:" in a else 0 for _, a in in_loop)
        assert [o - offsets[0] for o in offsets] == [0, 4, 8, 12], (key, offsets)
        wide = [b for b in blocks if any(op == "global_load_dwordx4" for op, _ in load.findall(b))]
        assert len(wide) == 1 and wide[0] is not quad[0], key
        assert re.search(r"v_and_b32_e32 v\d+, 15, v\d+", body), key                            # the test of the pointer's low four bits


def test_k2_cases_reach_every_loop_regime():
    seen = set()
    for c in G.K2_CASES:
        P, n = c.ps * c.ps, c.B * (c.H // c.ps) * (c.W // c.ps)
        regime = ("P<=64" if P <= 64 else "P>64", "C<=64" if c.C <= 64 else "C>64", n % 4 != 0)     # hbird_bank.hip:25-39, :20-21
        assert regime == (c.p_regime, c.c_regime, c.tail), c
        assert c.H % c.ps == 0 and c.W % c.ps == 0 and c.C * 16 <= 60000                         # hbird_bank.hip:44-47
        seen.add(regime)
    assert {(p, q) for p, q, _ in seen} == {(p, q) for p in ("P<=64", "P>64") for q in ("C<=64", "C>64")}
    assert {t for _, _, t in seen} == {True, False}
    cs = G.K2_CASES
    assert {1, 2, 7, 8, 14, 16, 32} <= {c.ps for c in cs} and {1, 2, 21, 63, 64, 65, 151, 256, 300, 3750} <= {c.C for c in cs}
    counts = {c.B * (c.H // c.ps) * (c.W // c.ps) for c in cs}
    assert {1, 2, 3, 5} <= counts and max(counts) > 4000
    assert any(c.H != c.W for c in cs) and any(c.pattern == "one" for c in cs)
    assert {(c.map255, c.C > 255) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
    assert max(c.C for c in cs) * 16 == 60000


def k3a_plan(SS, C):
    """hb_patch_scores: ceil(SS * C / K3_CHUNK) workgroups per image in the frequency pass (hbird_bank.hip:197); a boundary falls inside a
    label row when a multiple of K3_CHUNK below SS * C is not a multiple of C (the `e % C` of patch_freq_kernel, :88)."""
    n = SS * C
    chunks = (n + G.K3_CHUNK - 1) // G.K3_CHUNK
    return chunks, any((j * G.K3_CHUNK) % C for j in range(1, chunks))


def test_k3a_cases_reach_every_chunk_regime():
    for c in G.K3A_CASES + G.K3A_WORKSPACE:
        assert k3a_plan(c.SS, c.C) == (c.chunks, c.boundary_in_row), c
        assert c.C * 4 <= 60000 and c.B <= 65535
    cs = G.K3A_CASES
    sizes = {c.SS * c.C for c in cs}
    assert G.K3_CHUNK in sizes and G.K3_CHUNK + 1 in sizes and min(sizes) < G.K3_CHUNK and max(sizes) > 8 * G.K3_CHUNK
    assert {1, 21, 151, 257, 1000} <= {c.C for c in cs} and {1, 21, 151, 257, 1000} & {c.C for c in cs if c.boundary_in_row} >= {21, 151, 257, 1000}
    assert {1, 5, 63, 64, 65, 196, 1369} <= {c.SS for c in cs} and {1, 3, 16} <= {c.B for c in cs}
    assert {c.empties for c in cs} == {"none", "some", "image"}
    assert any(c.boundary_in_row and c.empties != "none" for c in cs) and any(c.C > 256 and c.chunks > 1 for c in cs)
    # score pass: K3_PATCHES = 64 patches per workgroup (hbird_bank.hip:93): one, exactly one, and a partly filled last one
    assert any(c.SS < 64 for c in cs) and any(c.SS == 64 for c in cs) and any(c.SS > 64 and c.SS % 64 for c in cs)
    for i, c in enumerate(cs):
        lab = G.k3a_label(c, 200 + i)
        ne = R.patch_scores(lab)[1]
        if c.empties == "none":
            assert ne.all()
        else:
            assert not ne.all()
        if c.empties == "image":
            assert not ne[c.B - 1].any()


def test_k3b_cases_reach_every_block_and_round_regime():
    cs = G.K3B_CASES
    blocks = {c.SS: (c.SS + 255) // 256 for c in cs}                        # hbird_bank.hip:214 (grid) and :141 (rounds of the prefix count)
    assert {1, 2} <= set(blocks.values()) and max(blocks.values()) == 17 and {1, 63, 256, 257, 1369, 4097} == set(blocks)
    for c in cs:
        assert 0 <= c.K <= c.SS and c.SS * 4 <= 60000                        # hbird_bank.hip:211-212
    for SS in blocks:
        ks = {c.K for c in cs if c.SS == SS}
        assert 1 in ks and SS in ks and (SS == 1 or len(ks) >= 3), SS
    assert {c.pattern for c in cs} == {"all", "rand70", "fourth", "round0", "last", "none"}
    assert {c.want_scores for c in cs} == {True, False} and any(c.gap for c in cs) and any(not c.gap for c in cs)
    # the prefix count matters when a non-empty patch of a later round follows empties of an earlier one
    assert sum(c.SS > 256 and c.pattern in ("rand70", "fourth", "round0") for c in cs) >= 5
    for i, c in enumerate(cs):
        scores, nonempty, r, r_off = G.k3b_inputs(c, 400 + i)
        counts = nonempty.sum(axis=1)
        assert len(set(np.diff(np.concatenate([r_off, [r_off[-1] + counts[-1]]])).tolist())) > 1 or c.SS == 1   # non-uniform r_off
        assert r_off[-1] + counts[-1] <= len(r)
        if c.pattern == "none":
            assert counts[0] == 0


def test_merge_cases_stay_within_the_lds_limit_and_cover_the_lists():
    cs = G.MERGE_CASES
    for c in cs:
        assert G.merge_lds_bytes(c.parts, c.k) <= G.MERGE_LDS, c               # hbird_knn.hip:467-468
    assert max(G.merge_lds_bytes(c.parts, c.k) for c in cs) > 0.8 * G.MERGE_LDS
    assert {c.metric for c in cs} == {0, 1} and {1, 2, 3, 8, 16} == {c.parts for c in cs}
    assert {1, 30, 64, 256, 2048} == {c.k for c in cs} and {1, 300, 10000} == {c.nq for c in cs}
    for pattern in ("random", "equal", "interleaved", "dup", "missing", "allmissing", "zeros"):
        assert {c.metric for c in cs if c.pattern == pattern} == {0, 1}, pattern
    assert any(c.k == 2048 and c.parts == 2 for c in cs) and any(c.parts * c.k % 64 for c in cs)
    nk = {n * k for n, k in G.SCORE_SHAPES}
    assert {1, 255, 256, 257} <= nk


# ---------------------------------------------------------------- argument checks that come before any GPU call

def test_bank_entries_refuse_bad_shapes_without_a_gpu():
    """Each entry fails with a message naming itself and the argument, before any launch or allocation (no GPU is touched: this runs
    on a machine without one)."""
    from hbird_mi import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = (
        ("hb_patch_scores", (p, 2, 0, 5, p, p, p, None), "SS"),
        ("hb_patch_scores", (p, 2, -3, 5, p, p, p, None), "SS"),
        ("hb_patch_scores", (p, 2, 4, 0, p, p, p, None), "C"),
        ("hb_patch_scores", (p, 2, 4, -1, p, p, p, None), "C"),
        ("hb_patch_scores", (p, -1, 4, 5, p, p, p, None), "B"),
        ("hb_patch_scores", (None, 2, 4, 5, p, p, p, None), "NULL"),
        ("hb_patch_select", (p, p, p, p, 2, 4, -1, p, None, None), "K"),
        ("hb_patch_select", (p, p, p, p, 2, 0, 0, p, None, None), "SS"),
        ("hb_patch_select", (p, p, p, p, -2, 4, 1, p, None, None), "B"),
        ("hb_patch_select", (p, p, p, p, 2, 4, 5, p, None, None), "K"),
        ("hb_patch_select", (p, None, p, p, 2, 4, 1, p, None, None), "NULL"),
        ("hb_gather_rows", (p, 4, 0, p, 2, p, None), "width"),
        ("hb_gather_rows", (p, 4, -8, p, 2, p, None), "width"),
        ("hb_gather_rows", (p, 4, 8, p, -2, p, None), "n"),
        ("hb_gather_rows", (p, -4, 8, p, 2, p, None), "src_rows"),
        ("hb_gather_rows", (p, 4, 8, None, 2, p, None), "NULL"),
        ("hb_normalize_rows", (p, 2, 0, p, None), "d"),
        ("hb_normalize_rows", (p, 2, -4, p, None), "d"),
        ("hb_normalize_rows", (p, -2, 4, p, None), "n"),
        ("hb_normalize_rows", (None, 2, 4, p, None), "NULL"),
        ("hb_merge_topk", (p, p, 2, -1, 4, 0, p, p, None), "nq"),
        ("hb_merge_topk", (p, p, 2, 1, 4, 2, p, p, None), "metric"),
        ("hb_merge_topk", (p, p, 0, 1, 4, 0, p, p, None), "bad shape"),
        ("hb_merge_topk_packed", (p, 64, 2, -1, 4, 0, p, p, None), "nq"),
        ("hb_merge_topk_packed", (p, 64, 2, 1, 4, 7, p, p, None), "metric"),
        ("hb_patch_label_hist", (p, -1, 8, 8, 2, 5, 0, p, None), "B"),
        ("hb_patch_label_hist", (p, 1, 8, 8, 2, 0, 0, p, None), "C"),
        ("hb_patch_label_hist", (p, 1, -8, 8, 2, 5, 0, p, None), "H"),
        ("hb_patch_label_hist", (p, 1, 8, 8, 0, 5, 0, p, None), "patch size"),
        ("hb_patch_label_hist", (p, 1, 8, 8, 3, 5, 0, p, None), "patch size"),
        ("hb_patch_label_hist", (None, 1, 8, 8, 2, 5, 0, p, None), "NULL"),
    )
    for name, args, word in calls:
        assert getattr(L, name)(*args) != 0, (name, args)
        msg = L.hb_last_error().decode()
        assert msg.startswith(name + ":") and word in msg, (name, word, msg)
    # empty work is not an error
    assert L.hb_patch_scores(None, 0, 4, 5, None, None, None, None) == 0
    assert L.hb_patch_select(None, None, None, None, 0, 4, 2, None, None, None) == 0
    assert L.hb_gather_rows(None, 0, 8, None, 0, None, None) == 0
    assert L.hb_normalize_rows(None, 0, 8, None, None) == 0
    assert L.hb_merge_topk(None, None, 2, 0, 4, 1, None, None, None) == 0 and L.hb_merge_topk(None, None, 2, 0, 4, 9, None, None, None) == 0
    assert L.hb_merge_topk_packed(None, 0, 2, 0, 4, 1, None, None, None) == 0 and L.hb_merge_topk_packed(None, 0, 2, 0, 4, 9, None, None, None) == 0
    assert L.hb_patch_label_hist(None, 0, 8, 8, 2, 5, 0, None, None) == 0


def test_patch_select_refuses_wrong_dtypes_before_it_asks_for_a_gpu():
    import torch
    from hbird_mi import ops
    s, ne = torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int32)
    r, off = torch.zeros(8), torch.zeros(2, dtype=torch.int64)
    bad = ((s.double(), ne, r, off, "scores"), (s, ne.long(), r, off, "nonempty"), (s, ne, r.double(), off, "r must"), (s, ne, r, off.int(), "r_off"),
           (s, ne[:, :3], r, off, "nonempty"), (s, ne, r, off[:1], "r_off"), (s[0], ne[0], r, off, "[B, SS]"), (s, ne, r.view(2, 4), off, "one-dimensional"),
           (s.numpy(), ne, r, off, "scores"))
    for *args, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.patch_select(*args, 1)
    with pytest.raises(RuntimeError, match="CUDA tensors required"):      # well-formed CPU tensors: refused for the device, as before
        ops.patch_select(s, ne, r, off, 1)


# ---------------------------------------------------------------- sensitivity: wrong variants disagree on the committed cases

def _wrong_label_hist(y, ps, C, map255):
    """K2 multiplying by the reciprocal instead of dividing."""
    return R.label_counts(y, ps, C, map255).astype(F32) * (F32(1.0) / F32(ps * ps))


def _wrong_scores_chunk_start(label):
    """K3a taking the class from the offset inside the chunk: (e - e0) % C."""
    B, SS, C = label.shape
    flat = (label.reshape(B, -1) > 0)
    e = np.arange(SS * C)
    cls = (e % G.K3_CHUNK) % C
    freq = np.stack([np.bincount(cls[flat[b]], minlength=C) for b in range(B)])
    pres = label > 0
    score = np.stack([pres[b].astype(np.int64) @ freq[b] for b in range(B)])
    return np.where(pres.any(axis=2), score.astype(F32), R.SENTINEL).astype(F32)


def _wrong_scores_denormals_flushed(label):
    lab = np.where(np.abs(label) < F32(1e-30), F32(0.0), label)
    return R.patch_scores(lab)[0]


def _wrong_select(scores, nonempty, r, r_off, K, how):
    out = scores.copy()
    for b in range(scores.shape[0]):
        ne = np.flatnonzero(nonempty[b])
        if how == "prefix restarts every round":
            rank = np.array([np.count_nonzero(nonempty[b, (p // 256) * 256:p]) for p in ne], dtype=np.int64)
        elif how == "prefix dropped":
            rank = np.array([np.count_nonzero(nonempty[b, (p // 64) * 64:p]) for p in ne], dtype=np.int64)
        else:
            rank = np.arange(len(ne))
        out[b, ne] = scores[b, ne] * r[r_off[b] + rank]
    if how == "ties reversed":
        SS = out.shape[1]
        return (SS - 1 - np.argsort(out[:, ::-1], axis=1, kind="stable"))[:, :K]
    return np.argsort(out, axis=1, kind="stable")[:, :K]


def test_wrong_k2_and_k3a_variants_are_seen_by_the_cases():
    seen = 0
    for i, c in enumerate(G.K2_CASES):
        y = G.k2_mask(c, 100 + i)
        seen += not np.array_equal(R.label_hist(y, c.ps, c.C, c.map255), _wrong_label_hist(y, c.ps, c.C, c.map255))
    assert seen >= 3
    seen = 0
    for i, c in enumerate(G.K3A_CASES):
        lab = G.k3a_label(c, 200 + i)
        differs = not np.array_equal(R.patch_scores(lab)[0], _wrong_scores_chunk_start(lab))
        assert differs == c.boundary_in_row or not differs, c
        seen += differs
    assert seen == sum(c.boundary_in_row for c in G.K3A_CASES) >= 5
    lab = G.k3a_special_rows()
    assert not np.array_equal(R.patch_scores(lab)[0], _wrong_scores_denormals_flushed(lab))


def test_wrong_k3b_variants_are_seen_by_the_cases():
    for how in ("prefix restarts every round", "prefix dropped"):
        seen = 0
        for i, c in enumerate(G.K3B_CASES):
            scores, nonempty, r, r_off = G.k3b_inputs(c, 400 + i)
            seen += not np.array_equal(R.patch_select(scores, nonempty, r, r_off, c.K)[0], _wrong_select(scores, nonempty, r, r_off, c.K, how))
        assert seen >= 5, how
    scores, nonempty, r, r_off = G.k3b_tie_inputs()
    for K in (7, 299, 301, 560):
        assert not np.array_equal(R.patch_select(scores, nonempty, r, r_off, K)[0], _wrong_select(scores, nonempty, r, r_off, K, "ties reversed"))


def test_wrong_k1_and_score_variants_are_seen_by_the_cases():
    differs = 0
    for D in G.K1_D:
        x = G.k1_rows(D)
        n32_float = np.sqrt((x * x).sum(axis=1, dtype=F32)).astype(F32)            # the norm accumulated in fp32
        differs += not np.array_equal(n32_float, R.norm32(x))
    assert differs >= len(G.K1_D) - 4
    for nq, k in G.SCORE_SHAPES[1:]:
        q, s = G.score_lists(nq, k, 24, nq * 10 + k)
        unclamped = R.fma_f32(F32(-2.0), s, oracle.chain_sqnorm(q)[:, None])
        unclamped = np.where(s == -np.inf, F32(np.inf), unclamped)
        assert (unclamped < 0).any() and not np.array_equal(unclamped.view(np.uint32), R.scores_to_l2(s, q).view(np.uint32))
        assert np.isinf(R.scores_to_l2(s, q)).any()


def _wrong_merge(val, idx, metric, how):
    parts, nq, k = val.shape
    cd = val.transpose(1, 0, 2).reshape(nq, parts * k)
    ci = idx.transpose(1, 0, 2).reshape(nq, parts * k)
    missing = ci < 0
    key = (cd if metric == 1 and how != "sign dropped" else -cd) + F32(0)
    pos = np.broadcast_to(np.arange(parts * k), ci.shape)
    idkey = -ci if how == "ids reversed" else ci
    if how == "missing not last":
        order = np.lexsort((pos, idkey, key), axis=-1)[:, :k]
    else:
        order = np.lexsort((pos, np.where(missing, 0, idkey), np.where(missing, 0, key), missing), axis=-1)[:, :k]
    oi, od = np.take_along_axis(ci, order, axis=1), np.take_along_axis(cd, order, axis=1)
    return np.where(oi < 0, -1, oi), np.where(oi < 0, F32(np.inf) if metric == 1 else F32(-np.inf), od).astype(F32)


def test_wrong_merge_variants_are_seen_by_the_cases():
    seen = {"missing not last": set(), "ids reversed": set(), "sign dropped": set()}
    for i, c in enumerate(G.MERGE_CASES):
        val, idx = G.merge_inputs(c, 600 + i)
        if c.nq > 300:
            val, idx = val[:, :300], idx[:, :300]
        ri, rd = R.merge(val, idx, c.metric)
        for how in seen:
            wi, wd = _wrong_merge(val, idx, c.metric, how)
            if not (np.array_equal(ri, wi) and np.array_equal(rd.view(np.uint32), wd.view(np.uint32))):
                seen[how].add((c.metric, c.pattern))
    assert {(0, "missing"), (1, "missing")} <= seen["missing not last"]
    assert {p for _, p in seen["ids reversed"]} >= {"equal", "interleaved", "zeros"}
    assert {m for m, _ in seen["sign dropped"]} == {1} and len(seen["sign dropped"]) >= 4
