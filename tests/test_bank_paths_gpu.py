"""The kernels around the search -- K2 (patch soft labels), K3a / K3b (bounded-memory patch sampling), gather / normalise rows, K1
(append into fragment tiles) with its read-back, the query-side constants, scores -> distances and the merge of sharded results --
on every launch path against tests/bank_refs.py, the numpy restatement of their definitions.

Every comparison is on bits (fp32 viewed as uint32) or integers.  The one exception is a K1 row that bank_refs.ambiguous flags --
the order of the double-precision norm sum could change the rounded norm there; 2 ulp are allowed on such a row, and
tests/test_bank_paths_cpu.py holds their share to at most 0.01 % of every K1 input, from the reference alone.  normalize_rows gets no
such allowance: its test requires that the reference flags no row of its inputs, and compares every row on bits.

The case lists are module-level tuples: tests/test_bank_paths_cpu.py restates the launch arithmetic and fails when a list stops
reaching a regime, or when a case declares a regime the launcher would not pick.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import pytest

import bank_refs as R
import oracle

pytestmark = pytest.mark.gpu

F32 = np.float32
METRIC_NAME = {0: "dot_product", 1: "l2"}


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(_np(a), dtype=F32).view(np.uint32)


def assert_bits(got, ref, what=""):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ; first at {first}: got {_np(got)[first]!r} "
                             f"(0x{g[first]:08x}), reference {np.asarray(ref)[first]!r} (0x{r[first]:08x})")


def assert_ints(got, ref, what=""):
    g, r = _np(got), np.asarray(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ; first at {first}: got {g[first]}, reference {r[first]}")


# ================================================================ K2: patch_label_hist_kernel

# p_regime / c_regime: the trip counts of the kernel's lane loops (one pass or several); tail: the last workgroup has idle waves
K2Case = namedtuple("K2Case", "ps C B H W map255 pattern p_regime c_regime tail")
K2_CASES = (
    K2Case(1, 1, 1, 1, 1, False, "one", "P<=64", "C<=64", True),          # 1 patch
    K2Case(2, 2, 1, 2, 4, False, "random", "P<=64", "C<=64", True),       # 2 patches
    K2Case(7, 21, 1, 7, 21, True, "random", "P<=64", "C<=64", True),      # 3 patches
    K2Case(8, 63, 1, 8, 40, False, "random", "P<=64", "C<=64", True),     # 5 patches
    K2Case(8, 64, 2, 16, 32, True, "random", "P<=64", "C<=64", False),
    K2Case(14, 64, 2, 42, 70, False, "random", "P>64", "C<=64", True),
    K2Case(16, 65, 3, 64, 48, False, "random", "P>64", "C>64", False),
    K2Case(32, 151, 2, 96, 64, True, "random", "P>64", "C>64", False),
    K2Case(2, 151, 1, 6, 10, False, "one", "P<=64", "C>64", True),
    K2Case(14, 256, 1, 28, 14, True, "random", "P>64", "C>64", True),     # map255 with C > 255: 255 is a legal class and still becomes 0
    K2Case(16, 300, 2, 32, 48, True, "random", "P>64", "C>64", False),
    K2Case(8, 300, 1, 16, 24, False, "random", "P<=64", "C>64", True),    # 255 stays 255
    K2Case(16, 3750, 1, 32, 32, False, "random", "P>64", "C>64", False),  # the LDS limit
    K2Case(1, 21, 1, 3, 5, True, "random", "P<=64", "C<=64", True),       # one pixel per patch
    K2Case(14, 21, 3, 518, 518, True, "random", "P>64", "C<=64", True),   # the big one: 4,107 patches
    K2Case(32, 2, 1, 64, 32, False, "one", "P>64", "C<=64", True),
)


def k2_mask(c, seed):
    rng = np.random.default_rng(seed)
    if c.pattern == "one":
        return np.full((c.B, 1, c.H, c.W), c.C - 1, dtype=np.int64)
    y = rng.integers(0, c.C, size=(c.B, 1, c.H, c.W), dtype=np.int64)
    if c.map255 or c.C > 255:
        y[rng.random(y.shape) < 0.1] = 255
    return y


@pytest.mark.parametrize("i", range(len(K2_CASES)), ids=lambda i: "ps{0}-C{1}-{2}x{3}x{4}".format(*K2_CASES[i][:5]))
def test_k2_soft_labels_on_bits(cuda_device, i):
    from hbird_mi import ops
    c = K2_CASES[i]
    y = k2_mask(c, 100 + i)
    ref = R.label_hist(y, c.ps, c.C, c.map255)
    got = ops.patch_label_hist(_dev(y), c.ps, c.C, map255=c.map255)
    assert_bits(got, ref, f"K2 {c}")
    assert np.array_equal(_np(got).astype(np.float64).sum(axis=-1), ref.astype(np.float64).sum(axis=-1))


def test_k2_class_range_errors_and_the_error_word_is_cleared(cuda_device):
    """Classes outside [0, C) raise HbirdClassRangeError (F.one_hot raises for them) -- also one beyond 32 bits, which must not alias
    into range -- and the next valid call on the same device succeeds: the per-device error word is cleared."""
    from hbird_mi import _lib, ops
    good = k2_mask(K2_CASES[5], 7)
    c = K2_CASES[5]
    ref = R.label_hist(good, c.ps, c.C)
    for bad_value, C in ((-1, 64), (64, 64), (255, 64), (2 ** 40 + 3, 64), (2 ** 32, 64), (-2 ** 32 + 1, 64)):
        y = good.copy()
        y[1, 0, 17, 33] = bad_value
        with pytest.raises(R.ClassRange):
            R.label_hist(y, c.ps, C)
        with pytest.raises(_lib.HbirdClassRangeError):
            ops.patch_label_hist(_dev(y), c.ps, C)
        assert_bits(ops.patch_label_hist(_dev(good), c.ps, c.C), ref, f"valid call after the refused class {bad_value}")
    # plain errors: no class involved
    for kwargs, msg in ((dict(patch_size=14, num_classes=3751), "too many classes"), (dict(patch_size=5, num_classes=64), "multiples of the patch size")):
        with pytest.raises(_lib.HbirdHipError, match=msg) as e:
            ops.patch_label_hist(_dev(good), **kwargs)
        assert not isinstance(e.value, _lib.HbirdClassRangeError)
    assert_bits(ops.patch_label_hist(_dev(good), c.ps, c.C), ref, "valid call after the plain errors")


# ================================================================ K3a: patch_freq_kernel + patch_scores_kernel

K3_CHUNK = 8192
# chunks: workgroups of the frequency pass per image; boundary_in_row: a chunk boundary falls inside a label row
K3aCase = namedtuple("K3aCase", "B SS C P empties chunks boundary_in_row")
K3A_CASES = (
    K3aCase(1, 1, 21, 16, "none", 1, False),
    K3aCase(1, 1, 21, 16, "image", 1, False),            # the only patch is empty
    K3aCase(3, 5, 1000, 16, "some", 1, False),           # below one chunk, C > 256
    K3aCase(1, 63, 21, 49, "some", 1, False),
    K3aCase(3, 64, 21, 49, "image", 1, False),
    K3aCase(1, 64, 128, 64, "some", 1, False),           # SS * C == K3_CHUNK
    K3aCase(1, 8192, 1, 4, "some", 1, False),            # the same with C = 1
    K3aCase(1, 8193, 1, 4, "some", 2, False),            # one above
    K3aCase(3, 65, 151, 196, "some", 2, True),
    K3aCase(16, 196, 151, 196, "image", 4, True),
    K3aCase(3, 196, 257, 196, "some", 7, True),
    K3aCase(1, 1369, 1000, 196, "some", 168, True),
    K3aCase(3, 1369, 21, 196, "image", 4, True),
    K3aCase(1, 65, 257, 16, "none", 3, True),
)


def k3a_label(c, seed):
    """Label rows as K2 writes them (float32(j) / float32(P), a palette of up to 12 classes per image so that classes repeat across
    patches), with whole rows zeroed: 30 % of the patches ("some"), and the whole last image on top ("image")."""
    rng = np.random.default_rng(seed)
    label = np.zeros((c.B, c.SS, c.C), dtype=F32)
    for b in range(c.B):
        pal = rng.choice(c.C, size=min(c.C, 12), replace=False)
        pix = pal[rng.integers(0, len(pal), size=(c.SS, c.P))]
        counts = np.zeros((c.SS, c.C), dtype=np.int64)
        np.add.at(counts, (np.arange(c.SS)[:, None], pix), 1)
        label[b] = counts.astype(F32) / F32(c.P)
        if c.empties != "none":
            label[b, rng.random(c.SS) < 0.3] = 0.0
    if c.empties == "image":
        label[c.B - 1] = 0.0
    return label


def _check_k3a(label, what):
    from hbird_mi import ops
    scores, nonempty, nz = ops.patch_scores(_dev(label))
    rs, rne, rnz, _ = R.patch_scores(label)
    assert_ints(nonempty, rne, f"{what}: nonempty")
    assert_ints(nz, rnz, f"{what}: nz_count")
    assert_bits(scores, rs, f"{what}: scores")


@pytest.mark.parametrize("i", range(len(K3A_CASES)), ids=lambda i: "B{0}-SS{1}-C{2}-{4}".format(*K3A_CASES[i]))
def test_k3a_scores_with_empty_patches_and_chunk_boundaries(cuda_device, i):
    c = K3A_CASES[i]
    _check_k3a(k3a_label(c, 200 + i), f"K3a {c}")


def k3a_special_rows():
    """Hand-made rows for `presence = label > 0` in IEEE arithmetic: -0.0, a negative, NaN and +0.0 are absent; 1e-45 (the smallest
    denormal) is present.  K2 never writes such values; K3a reads whatever label table it is given."""
    lab = np.zeros((2, 7, 5), dtype=F32)
    lab[0, 0] = [-0.0, 0, 0, 0, -0.0]            # empty
    lab[0, 1] = [0, -0.25, 0, 0, 0]              # empty: negative
    lab[0, 2] = [0, 0, np.nan, 0, 0]             # empty: NaN
    lab[0, 3] = [0, 0, 0, 1e-45, 0]              # non-empty: the smallest denormal
    lab[0, 4] = [0.5, 0, 0, 0.5, 0]
    lab[0, 5] = [0, 0, 0, 1.0, 0]
    lab[1, 2] = [-1.0, np.nan, -0.0, 0, 1e-45]   # one present class among absent ones
    lab[1, 6] = [np.inf, 0, 0, 0, 1.0]
    return lab


def test_k3a_presence_is_ieee_greater_than_zero(cuda_device):
    lab = k3a_special_rows()
    rs, rne, rnz, freq = R.patch_scores(lab)
    assert rne[0].tolist() == [0, 0, 0, 1, 1, 1, 0] and rnz.tolist() == [3, 2] and freq[0].tolist() == [1, 0, 0, 3, 0]
    _check_k3a(lab, "K3a hand-made rows")


K3A_WORKSPACE = (K3aCase(16, 196, 151, 196, "some", 4, True), K3aCase(1, 5, 21, 16, "some", 1, False),
                 K3aCase(3, 65, 1000, 16, "image", 8, True))


def test_k3a_frequency_workspace_is_reused_correctly(cuda_device):
    """The [B, C] class-frequency workspace is kept per (device, stream): a big call, a smaller one, a bigger one again, then the same
    on a second stream -- stale counts of an earlier call must never reach a later one."""
    torch = _torch()
    labels = [k3a_label(c, 300 + j) for j, c in enumerate(K3A_WORKSPACE)]
    assert K3A_WORKSPACE[1].B * K3A_WORKSPACE[1].C < K3A_WORKSPACE[0].B * K3A_WORKSPACE[0].C < K3A_WORKSPACE[2].B * K3A_WORKSPACE[2].C
    for j, lab in enumerate(labels):
        _check_k3a(lab, f"default stream, call {j}")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for j in (1, 2, 0, 1):
            _check_k3a(labels[j], f"second stream, call {j}")
    side.synchronize()
    _check_k3a(labels[0], "default stream again")


# ================================================================ K3b: patch_select_kernel

# three images per case: the first follows `pattern`, the others are "rand70" and "all" (so r_off is never uniform)
K3bCase = namedtuple("K3bCase", "SS K pattern gap want_scores")
K3B_CASES = (
    K3bCase(1, 1, "all", 0, True),
    K3bCase(1, 1, "none", 2, False),
    K3bCase(63, 1, "rand70", 0, True),
    K3bCase(63, 63, "fourth", 3, False),
    K3bCase(63, 20, "last", 0, True),
    K3bCase(256, 30, "rand70", 0, False),
    K3bCase(256, 256, "last", 1, True),
    K3bCase(256, 1, "none", 0, True),
    K3bCase(257, 100, "round0", 0, True),
    K3bCase(257, 257, "all", 5, False),
    K3bCase(257, 1, "fourth", 0, True),
    K3bCase(1369, 100, "rand70", 0, False),
    K3bCase(1369, 1369, "fourth", 2, True),
    K3bCase(1369, 1, "round0", 0, True),
    K3bCase(1369, 400, "none", 0, False),
    K3bCase(4097, 500, "rand70", 7, True),
    K3bCase(4097, 4097, "last", 0, False),
    K3bCase(4097, 100, "round0", 0, True),
    K3bCase(4097, 1, "all", 0, False),
)


def k3b_pattern(name, SS, rng):
    ne = np.zeros(SS, dtype=np.int32)
    if name == "all":
        ne[:] = 1
    elif name == "rand70":
        ne[rng.random(SS) < 0.7] = 1
    elif name == "fourth":
        ne[::4] = 1
    elif name == "round0":                       # the first 256-patch round holds no non-empty patch
        ne[256:] = 1
    elif name == "last":
        ne[-1] = 1
    else:
        assert name == "none"
    return ne


def k3b_inputs(c, seed):
    rng = np.random.default_rng(seed)
    pats = (c.pattern, "rand70", "all")
    nonempty = np.stack([k3b_pattern(p, c.SS, rng) for p in pats])
    scores = rng.integers(1, 60, size=nonempty.shape).astype(F32)
    scores[nonempty == 0] = R.SENTINEL
    counts = nonempty.sum(axis=1)
    r_off = (np.concatenate([[0], np.cumsum(counts)[:-1]]) + c.gap * np.arange(len(pats))).astype(np.int64)
    r = rng.random(int(counts.sum()) + c.gap * len(pats) + 1, dtype=F32)
    return scores, nonempty, r, r_off


@pytest.mark.parametrize("i", range(len(K3B_CASES)), ids=lambda i: "SS{0}-K{1}-{2}-gap{3}".format(*K3B_CASES[i]))
def test_k3b_selection_with_empty_patches(cuda_device, i):
    from hbird_mi import ops
    c = K3B_CASES[i]
    scores, nonempty, r, r_off = k3b_inputs(c, 400 + i)
    ref_idx, ref_noisy = R.patch_select(scores, nonempty, r, r_off, c.K)
    out = ops.patch_select(_dev(scores), _dev(nonempty), _dev(r), _dev(r_off), c.K, want_scores=c.want_scores)
    if c.want_scores:
        assert_bits(out[1], ref_noisy, f"K3b {c}: noisy scores")
        out = out[0]
    assert_ints(out, ref_idx, f"K3b {c}: selected patches")


def k3b_tie_inputs():
    """Integer scores times power-of-two noise that collide exactly (4 * 1/2 = 8 * 1/4 = 2 * 1 = 16 * 1/8 = 2.0 in fp32), in runs across
    the wave and round boundaries, and runs of un-noised sentinels: the order among equals is the patch index."""
    SS = 600
    s4, n4 = np.array([4, 8, 2, 16], dtype=F32), np.array([0.5, 0.25, 1.0, 0.125], dtype=F32)
    scores = np.tile(s4, SS // 4).astype(F32)
    nonempty = np.ones(SS, dtype=np.int32)
    nonempty[100:140] = 0
    nonempty[250:262] = 0
    nonempty[511:515] = 0
    scores[nonempty == 0] = R.SENTINEL
    ne_pos = np.flatnonzero(nonempty)
    r = np.zeros(len(ne_pos), dtype=F32)
    for j, p in enumerate(ne_pos):
        r[j] = n4[p % 4]
    r[300:] *= F32(2.0)                          # a second plateau (4.0) behind the first
    return scores[None], nonempty[None], r, np.zeros(1, dtype=np.int64)


def test_k3b_exact_ties_go_to_the_lower_patch(cuda_device):
    from hbird_mi import ops
    scores, nonempty, r, r_off = k3b_tie_inputs()
    SS = scores.shape[1]
    noisy = R.noisy_scores(scores, nonempty, r, r_off)
    assert sorted(set(noisy[0].tolist())) == [2.0, 4.0, 1e6]
    for K in (1, 7, 299, 301, 560, SS):
        ref_idx, _ = R.patch_select(scores, nonempty, r, r_off, K)
        got = ops.patch_select(_dev(scores), _dev(nonempty), _dev(r), _dev(r_off), K)
        assert_ints(got, ref_idx, f"K3b ties, K = {K}")
    ref_idx, _ = R.patch_select(scores, nonempty, r, r_off, SS)
    for lo, hi in ((0, 300), (300, 544), (544, 600)):          # inside a plateau the patch index ascends
        assert (np.diff(ref_idx[0, lo:hi]) > 0).all()


def test_k3b_writes_every_slot_of_every_image(cuda_device):
    """The C entry, out_idx pre-filled with -7 and out_scores absent: every one of the K slots of every image is written."""
    from hbird_mi import _lib
    torch = _torch()
    c = K3bCase(1369, 1369, "rand70", 4, False)
    scores, nonempty, r, r_off = k3b_inputs(c, 77)
    for K in (1, 100, c.SS):
        ref_idx, _ = R.patch_select(scores, nonempty, r, r_off, K)
        out = torch.full((scores.shape[0], K), -7, dtype=torch.int64, device="cuda")
        ds, dn, dr, do = _dev(scores), _dev(nonempty), _dev(r), _dev(r_off)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().hb_patch_select(p(ds), p(dn), p(dr), p(do), scores.shape[0], c.SS, K, p(out), None,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert_ints(out, ref_idx, f"K3b through the C entry, K = {K}")


def test_k3b_refuses_wrong_dtypes_and_shapes(cuda_device):
    """The wrapper hands bare pointers to the C entry: another dtype would be read as noise, so it is refused (ValueError)."""
    from hbird_mi import ops
    scores, nonempty, r, r_off = k3b_inputs(K3B_CASES[2], 5)
    ds, dn, dr, do = _dev(scores), _dev(nonempty), _dev(r), _dev(r_off)
    for args in ((ds.double(), dn, dr, do), (ds, dn.long(), dr, do), (ds, dn, dr.double(), do), (ds, dn, dr, do.int()),
                 (ds, dn[:, :-1], dr, do), (ds, dn, dr, do[:-1]), (ds.view(-1), dn.view(-1), dr, do), (ds, dn, dr.view(1, -1), do)):
        with pytest.raises(ValueError, match="patch_select"):
            ops.patch_select(*args, 1)
    assert_ints(ops.patch_select(ds, dn, dr, do, 5), R.patch_select(scores, nonempty, r, r_off, 5)[0], "valid call afterwards")


# ================================================================ the bounded-bank chain: K2 -> K3a -> K3b -> gather -> normalise

def test_bounded_bank_chain_on_bits(cuda_device):
    """Masks with an ignore region (255): patches that lie wholly inside it are turned into empties (their label rows zeroed), the rest
    goes through the bounded-memory build.  The bank's rows and labels against the chain of references, bit for bit."""
    from hbird_mi import ops
    torch = _torch()
    rng = np.random.default_rng(11)
    B, ps, S, C, D, K = 4, 14, 12, 21, 48, 50
    y = rng.integers(0, 6, size=(B, 1, S * ps, S * ps), dtype=np.int64) + rng.integers(0, 15, size=(B, 1, 1, 1))
    y[:, :, :5 * ps, 2 * ps:9 * ps] = 255
    y[3, :, :, :] = 255                                                   # an image without a labelled pixel
    y[2, :, 40:, :] = 255
    feats = (rng.standard_normal((B, S * S, D)) * np.exp(rng.normal(0, 1, size=(B, S * S, 1)))).astype(F32)
    ignored = (y == 255).reshape(B, S, ps, S, ps).all(axis=(2, 4)).reshape(B, S * S)
    assert 0 < ignored[0].sum() < S * S and ignored[3].all()

    lab_ref = R.label_hist(y, ps, C, map255=True).reshape(B, S * S, C)
    lab_ref[ignored] = 0.0
    sc_ref, ne_ref, nz_ref, _ = R.patch_scores(lab_ref)
    r_off = np.concatenate([[0], np.cumsum(nz_ref)[:-1]]).astype(np.int64)
    r = rng.random(int(nz_ref.sum()), dtype=F32)
    sidx_ref, _ = R.patch_select(sc_ref, ne_ref, r, r_off, K)
    rows_ref = (sidx_ref + np.arange(B)[:, None] * (S * S)).reshape(-1)
    bank_ref = R.normalized(feats.reshape(-1, D)[rows_ref])
    blab_ref = lab_ref.reshape(-1, C)[rows_ref]

    lab = ops.patch_label_hist(_dev(y), ps, C, map255=True).view(B, S * S, C)
    lab = lab * (~_dev(ignored)).to(torch.float32)[:, :, None]
    assert_bits(lab, lab_ref, "chain: labels")
    scores, nonempty, nz = ops.patch_scores(lab)
    assert_ints(nz, nz_ref, "chain: nz_count")
    sidx = ops.patch_select(scores, nonempty, _dev(r), _dev(r_off), K)
    assert_ints(sidx, sidx_ref, "chain: sampled patches")
    rows = (sidx + torch.arange(B, device="cuda")[:, None] * (S * S)).reshape(-1)
    bank = ops.normalize_rows(ops.gather_rows(_dev(feats).reshape(-1, D), rows))
    assert_bits(bank, bank_ref, "chain: bank rows")
    assert_bits(ops.gather_rows(lab.reshape(-1, C), rows), blab_ref, "chain: bank labels")


# ================================================================ gather_rows / normalize_rows

ROW_WIDTHS = (1, 63, 64, 65, 384, 1000, 1536)
ROW_COUNTS = (1, 3, 4, 5, 1001)


def scaled_rows(n, D, seed):
    """Gaussian rows with log-normal row scales."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)) * np.exp(rng.normal(0.0, 1.0, size=(n, 1)))).astype(F32)


@pytest.mark.parametrize("width", ROW_WIDTHS)
def test_gather_rows_with_foreign_and_duplicate_ids(cuda_device, width):
    from hbird_mi import ops
    rows = 37
    src = scaled_rows(rows, width, width)
    rng = np.random.default_rng(width)
    for n in ROW_COUNTS:
        ids = rng.integers(0, rows, size=n).astype(np.int64)
        special = np.array([-1, rows, 2 ** 33, -2 ** 40, rows - 1, 0, 5, 5, 2 ** 62], dtype=np.int64)
        m = min(n, len(special))
        ids[rng.permutation(n)[:m]] = special[:m] if n < len(special) else special
        ok = (ids >= 0) & (ids < rows)
        ref = np.where(ok[:, None], src[np.where(ok, ids, 0)], F32(0.0))
        assert_bits(ops.gather_rows(_dev(src), _dev(ids)), ref, f"gather_rows width {width}, n {n}")
    ids = np.array([-1, rows, 2 ** 33], dtype=np.int64)              # every special id at least once, whatever n drew
    assert not _np(ops.gather_rows(_dev(src), _dev(ids))).any()
    ids = np.array([7, 7, 36, 7], dtype=np.int64)
    assert_bits(ops.gather_rows(_dev(src), _dev(ids)), src[ids], "duplicates")


@pytest.mark.parametrize("width", ROW_WIDTHS)
def test_normalize_rows_on_bits(cuda_device, width):
    """x / n32 with the norm accumulated in double: a zero row gives NaN (no eps, as the definition), rows of 1e20 stay finite -- the
    fp32 norm of the upstream definition would overflow there (1e40 > FLT_MAX) and give zeros -- and denormal rows keep their norm."""
    from hbird_mi import ops
    for n in ROW_COUNTS:
        x = scaled_rows(n, width, 1000 + n)
        x[0] = 1e20
        if n > 2:
            x[1] = 0.0
            x[2] = F32(3e-42) * np.sign(x[2] + F32(1e-30))
        ref = R.normalized(x)
        assert not R.ambiguous(x, normalize=False)[~np.isnan(ref).any(axis=1)].any()      # no row whose norm depends on the sum's order
        got = _np(ops.normalize_rows(_dev(x)))
        assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
        if n > 2:
            assert np.isnan(got[1]).all() and np.isnan(ref[1]).all()
            assert np.isfinite(got[2]).all() and np.abs(got[2]).max() > 0
            got[1] = 0.0
            ref[1] = 0.0
        assert_bits(got, ref, f"normalize_rows width {width}, n {n}")


# ================================================================ K1: rows_to_tiles_kernel / rows_to_tiles_lds_kernel

K1_D = (1, 3, 7, 8, 20, 48, 100, 192, 208, 384, 400, 768, 816, 832, 1024, 1152, 1168, 1536)
# what the launcher picks for an aligned source without a forced form: the first form, or the LDS form with 32 / 16 / 8 rows per workgroup
K1_REGIME = {1: "first", 3: "first", 7: "first", 8: "first", 20: "first", 48: "lds32", 100: "first", 192: "lds32", 208: "lds16", 384: "lds16",
             400: "lds16", 768: "lds16", 816: "lds16", 832: "lds8", 1024: "lds8", 1152: "lds8", 1168: "first", 1536: "first"}
K1_PIECES = (1, 31, 32, 33, 255, 257, 1000)      # appended one behind the other: every row0 % 32, pieces that span row tiles
K1_GROWTH_PIECES = (30, 7, 300, 1000) + (33,) * 32   # past the reservation twice, then a piece behind every row0 % 32
K1_GROWTH_D = (20, 48, 384, 1024, 1536)          # the first form, lds32, lds16, lds8, the first form beyond the LDS form's widths
K1_FORMS = (1, 0, 8, 16, 32)                     # hb_set_layout_form
K1_FORM_D = (48, 192, 384, 1152)
K1_OFFSET_D = (20, 100, 384, 1024)               # device sources 1, 2 and 3 floats off a 16-byte boundary
K1_BIG_HOST = (70000, 1024)                      # one host add beyond the 256 MiB staging chunk


def k1_rows(D, seed=0):
    return scaled_rows(sum(K1_PIECES), D, 5000 + D + seed)


def k1_queries(D, nq=16, seed=0):
    return np.random.default_rng(9000 + D + seed).standard_normal((nq, D)).astype(F32)


def _index(D, metric):
    from hbird_mi.nn.search_hip import HipFlatIndex
    return HipFlatIndex(D, metric, 0)


def _add_pieces(ix, x, normalize, pieces=K1_PIECES, host_every=3):
    at = 0
    for j, n in enumerate(pieces):
        pc = x[at:at + n]
        ix.add(np.ascontiguousarray(pc) if j % host_every == host_every - 1 else _dev(pc), normalize=normalize)
        at += n
    assert at == len(x)


def check_index(ix, x, normalize, metric, what, k=5):
    """reconstruct against the stored rows, copy_norms against their norms (ambiguous rows: 2 ulp), ntotal, and a k-nearest search
    against the fmaf-chain oracle over the index's own rows -- the search is what sees the per-row constant of the L2 metric."""
    torch = _torch()
    n, D = x.shape
    assert ix.ntotal == n, what
    ref_rows, ref_norm = R.stored_rows(x, normalize), R.stored_norm(x, normalize)
    amb = R.ambiguous(x, normalize)
    assert amb.mean() <= 1e-4, what
    rows = _np(ix.reconstruct(torch.arange(n, device="cuda")))
    norms = _np(ix.copy_norms())
    assert (R.ulp_distance(rows[amb], ref_rows[amb]) <= 2).all() and (R.ulp_distance(norms[amb], ref_norm[amb]) <= 2).all(), what
    assert_bits(rows[~amb], ref_rows[~amb], f"{what}: stored rows")
    assert_bits(norms[~amb], ref_norm[~amb], f"{what}: stored norms")
    q = k1_queries(D)
    kk = min(k, n)
    idx, dist = ix.search(_dev(q), kk)
    ridx, rdist = oracle.knn_chain_f32(q, rows, kk, METRIC_NAME[metric])
    assert_ints(idx, ridx, f"{what}: neighbours")
    assert_bits(dist, rdist, f"{what}: distances")
    return rows, norms


@pytest.mark.parametrize("D", K1_D)
def test_k1_append_pieces_on_bits(cuda_device, D):
    x = k1_rows(D)
    for metric in (0, 1):
        for normalize in (True, False):
            ix = _index(D, metric)
            _add_pieces(ix, x, normalize)
            check_index(ix, x, normalize, metric, f"K1 D = {D}, metric {metric}, normalize {normalize}")
            ix.close()


@pytest.mark.parametrize("D", K1_GROWTH_D)
def test_k1_growth_reset_and_short_banks(cuda_device, D):
    """An index created small and grown past its reservation twice keeps its old rows; k beyond the rows returns -1 (the padding rows
    of the last tile never surface); after reset() only the new rows are found."""
    x = scaled_rows(sum(K1_GROWTH_PIECES), D, 7000 + D)
    for metric in (0, 1):
        ix = _index(D, metric)
        ix.reserve(40)
        _add_pieces(ix, x, True, pieces=K1_GROWTH_PIECES)
        check_index(ix, x, True, metric, f"K1 growth D = {D}, metric {metric}")
        ix.reset()
        assert ix.ntotal == 0
        y = k1_rows(D, seed=2)[:3]
        ix.add(_dev(y), normalize=False)
        rows, _ = check_index(ix, y, False, metric, f"K1 after reset D = {D}, metric {metric}")
        q = k1_queries(D)
        idx, dist = ix.search(_dev(q), 5)
        ridx, rdist = oracle.knn_chain_f32(q, rows, 3, METRIC_NAME[metric])
        assert_ints(_np(idx)[:, :3], ridx, "k > ntotal: the rows that exist")
        assert_bits(_np(dist)[:, :3], rdist, "k > ntotal: their distances")
        assert (_np(idx)[:, 3:] == -1).all()
        assert np.isinf(_np(dist)[:, 3:]).all()
        ix.close()


@pytest.mark.parametrize("D", K1_FORM_D)
def test_k1_every_layout_form_against_the_definition(cuda_device, D):
    from hbird_mi import _lib
    x = k1_rows(D, seed=3)
    try:
        for form in K1_FORMS:
            _lib.check(_lib.lib().hb_set_layout_form(form))
            for metric, normalize in ((1, True), (0, False)):
                ix = _index(D, metric)
                _add_pieces(ix, x, normalize)
                check_index(ix, x, normalize, metric, f"K1 form {form}, D = {D}, metric {metric}, normalize {normalize}")
                ix.close()
    finally:
        _lib.check(_lib.lib().hb_set_layout_form(0))


@pytest.mark.parametrize("D", K1_OFFSET_D)
def test_k1_unaligned_device_source_gives_the_aligned_bits(cuda_device, D):
    """A CUDA tensor view that starts 1, 2 or 3 floats into its allocation is contiguous and reaches K1 as it is: same stored rows,
    norms and search results as the 16-byte aligned source, bit for bit."""
    torch = _torch()
    x = k1_rows(D, seed=4)[:700]
    n = len(x)
    for metric, normalize in ((1, True), (0, False)):
        ix = _index(D, metric)
        ix.add(_dev(x), normalize=normalize)
        rows0, norms0 = check_index(ix, x, normalize, metric, f"K1 aligned D = {D}")
        ix.close()
        for off in (1, 2, 3):
            buf = torch.zeros(n * D + 8, dtype=torch.float32, device="cuda")
            view = buf[off:off + n * D].view(n, D)
            view.copy_(_dev(x))
            assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
            ix = _index(D, metric)
            ix.add(view, normalize=normalize)
            rows, norms = check_index(ix, x, normalize, metric, f"K1 source off by {off} floats, D = {D}")
            assert_bits(rows, rows0, f"off by {off}: rows")
            assert_bits(norms, norms0, f"off by {off}: norms")
            ix.close()


def test_k1_host_add_beyond_one_staging_chunk(cuda_device):
    """70,000 x 1024 fp32 rows are 273 MiB: a host add stages them in two chunks.  Same stored rows and norms as the same rows added
    from the device in one launch; the first and last 1,000 rows also against the definition."""
    torch = _torch()
    n, D = K1_BIG_HOST
    assert n * D * 4 > 256 << 20
    rng = np.random.default_rng(123)
    x = rng.standard_normal((n, D), dtype=F32)
    x *= np.exp(rng.normal(0.0, 1.0, size=(n, 1))).astype(F32)
    ids = torch.arange(n, device="cuda")
    a = _index(D, 1)
    a.add(x, normalize=True)
    b = _index(D, 1)
    b.add(_dev(x), normalize=True)
    assert a.ntotal == b.ntotal == n
    ra, rb = a.reconstruct(ids), b.reconstruct(ids)
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert torch.equal(a.copy_norms().view(torch.int32), b.copy_norms().view(torch.int32))
    chunk = (256 << 20) // (D * 4)
    for lo in (0, chunk - 500, n - 1000):
        part = x[lo:lo + 1000]
        amb = R.ambiguous(part)
        assert amb.mean() <= 1e-4
        assert_bits(_np(ra[lo:lo + 1000])[~amb], R.stored_rows(part, True)[~amb], f"host add, rows from {lo}")
        assert_bits(_np(a.copy_norms()[lo:lo + 1000])[~amb], R.stored_norm(part, True)[~amb], f"host add, norms from {lo}")
    q = k1_queries(D)
    ia, da = a.search(_dev(q), 5)
    ib, db = b.search(_dev(q), 5)
    assert_ints(ia, _np(ib), "host add: neighbours")
    assert_bits(da, _np(db), "host add: distances")
    a.close()
    b.close()


# ================================================================ hb_index_reconstruct (tiles_to_rows_kernel)

RECONSTRUCT_BASES = (0, 10 ** 9)
RECONSTRUCT_COUNTS = (1, 3, 4, 5)


@pytest.mark.parametrize("D", (20, 384))
def test_reconstruct_ids_inside_and_outside_the_bank(cuda_device, D):
    """ids are global (row + id_base).  -1 and every id outside [id_base, id_base + ntotal) -- on either side -- give zero rows."""
    n = 70
    x = scaled_rows(n, D, 31)
    ix = _index(D, 0)
    ix.add(_dev(x))
    for base in RECONSTRUCT_BASES:
        ids = np.array([-1, base, base + n - 1, base + n, base + n + 31, base - 1, base + 2 ** 40, base + 33, -2 ** 50, base + 64, base + 95,
                        base + 10 ** 6], dtype=np.int64)
        local = ids - base
        ok = (ids >= 0) & (local >= 0) & (local < n)
        assert ok.sum() == 4
        ref = np.where(ok[:, None], x[np.where(ok, local, 0)], F32(0.0))
        for dev in (True, False):
            got = ix.reconstruct(_dev(ids) if dev else ids, id_base=base)
            assert_bits(got, ref, f"reconstruct id_base {base}, device ids {dev}")
            for m in RECONSTRUCT_COUNTS:
                for lo in (0, 1, 5):
                    got = ix.reconstruct(_dev(ids[lo:lo + m]) if dev else ids[lo:lo + m], id_base=base)
                    assert_bits(got, ref[lo:lo + m], f"reconstruct id_base {base}, n {m} from {lo}, device ids {dev}")
    # an id_base far below zero: the difference id - id_base must not wrap into the bank
    for base in (-2 ** 63 + 5, -2 ** 62, -1):
        got = ix.reconstruct(np.array([0, 5, n - 1, 2 ** 62, -1], dtype=np.int64), id_base=base)
        ref = np.zeros((5, D), dtype=F32)
        if base == -1:
            ref[0], ref[1] = x[1], x[6]
        assert_bits(got, ref, f"reconstruct id_base {base}")
    ix.close()


def test_reconstruct_and_score_conversion_refuse_negative_counts(cuda_device):
    from hbird_mi import _lib
    ix = _index(20, 1)
    ix.add(_dev(scaled_rows(40, 20, 3)))
    L = _lib.lib()
    buf = _torch().zeros(64, dtype=_torch().float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert L.hb_index_reconstruct(ix._h, p, -1, 0, p, 1) != 0 and "hb_index_reconstruct: n is negative" in _lib.last_error()
    assert L.hb_index_distances_from_scores(ix._h, p, -1, 1, p) != 0 and "hb_index_distances_from_scores: nq is negative" in _lib.last_error()
    assert L.hb_index_distances_from_scores(ix._h, p, 1, 0, p) != 0 and "hb_index_distances_from_scores: k must be positive" in _lib.last_error()
    assert L.hb_index_aggregate(ix._h, p, -1, p, p, 3, 0, ctypes.c_float(0.02), p, 1) != 0 and "hb_index_aggregate: nq is negative" in _lib.last_error()
    assert L.hb_index_aggregate(ix._h, p, 1, p, p, 0, 0, ctypes.c_float(0.02), p, 1) != 0 and "hb_index_aggregate: k must be positive" in _lib.last_error()
    assert L.hb_index_aggregate(ix._h, p, 0, p, p, 0, 0, ctypes.c_float(0.02), p, 1) == 0          # no queries: empty work, whatever k
    assert L.hb_index_distances_from_scores(ix._h, p, 0, 0, p) == 0
    assert L.hb_index_aggregate_partial(ix._h, p, -1, p, p, 3, 0, ctypes.c_float(0.02), p, 40, p) != 0 and "hb_index_aggregate_partial: nq is negative" in _lib.last_error()
    assert_bits(ix.reconstruct(np.array([0, 39])), scaled_rows(40, 20, 3)[[0, 39]], "valid call afterwards")
    ix.close()


# ================================================================ query side: rows_to_tiles (queries), query_aux_kernel, scores_to_l2_kernel

@pytest.mark.parametrize("D", (384, 20))
def test_l2_search_with_an_unaligned_query_tensor(cuda_device, D):
    torch = _torch()
    bank = scaled_rows(900, D, 41)
    q = k1_queries(D, nq=77, seed=1)
    ix = _index(D, 1)
    ix.add(_dev(bank))
    ridx, rdist = oracle.knn_chain_f32(q, bank, 5, "l2")
    for off in (0, 1):
        buf = torch.zeros(q.size + 8, dtype=torch.float32, device="cuda")
        view = buf[off:off + q.size].view(q.shape)
        view.copy_(_dev(q))
        assert view.data_ptr() % 16 == 4 * off
        idx, dist = ix.search(view, 5)
        assert_ints(idx, ridx, f"queries off by {off} floats: neighbours")
        assert_bits(dist, rdist, f"queries off by {off} floats: distances")
    ix.close()


def test_query_workspace_after_a_bigger_search(cuda_device):
    """1,024 queries scaled by 1e12 (finite scores and norms) leave their tiles in the index's query workspace; 300 ordinary queries
    on the same index then get the bits of a fresh index."""
    D = 64
    bank = scaled_rows(2000, D, 51)
    big = (k1_queries(D, nq=1024, seed=2) * F32(1e12)).astype(F32)
    q = k1_queries(D, nq=300, seed=3)
    for metric in (1, 0):
        ix = _index(D, metric)
        ix.add(_dev(bank))
        idx, dist = ix.search(_dev(big), 8)
        assert np.isfinite(_np(dist)).all()
        ridx, rdist = oracle.knn_chain_f32(big, bank, 8, METRIC_NAME[metric])
        assert_ints(idx, ridx, "scaled queries: neighbours")
        assert_bits(dist, rdist, "scaled queries: distances")
        idx, dist = ix.search(_dev(q), 8)
        fresh = _index(D, metric)
        fresh.add(_dev(bank))
        fidx, fdist = fresh.search(_dev(q), 8)
        assert_ints(idx, _np(fidx), "after the bigger search: neighbours")
        assert_bits(dist, _np(fdist), "after the bigger search: distances")
        ridx, rdist = oracle.knn_chain_f32(q, bank, 8, METRIC_NAME[metric])
        assert_ints(idx, ridx, "ordinary queries: neighbours")
        assert_bits(dist, rdist, "ordinary queries: distances")
        ix.close()
        fresh.close()


SCORE_SHAPES = ((1, 1), (51, 5), (256, 1), (257, 1), (64, 4))     # nq * k = 1, 255, 256, 257, 256


def score_lists(nq, k, D, seed):
    """Hand-made ordering scores: ordinary ones, -inf (a missing neighbour), values just above |q|^2 / 2 (the unclamped distance would be
    negative), exactly |q|^2 / 2 and +-0."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, D)).astype(F32)
    half = (oracle.chain_sqnorm(q) * F32(0.5))[:, None]
    s = (half - rng.random((nq, k), dtype=F32) * F32(3.0)).astype(F32)
    kind = rng.integers(0, 6, size=(nq, k))
    s = np.where(kind == 1, F32(-np.inf), s)
    s = np.where(kind == 2, half * F32(1.0 + 1e-6), s)
    s = np.where(kind == 3, half, s)
    s = np.where(kind == 4, F32(-0.0), s)
    if nq * k >= 6:
        flat = s.reshape(-1)
        flat[:6] = [flat[0], -np.inf, half[0, 0] * F32(1.001), half[0, 0], 0.0, -0.0]
        flat[0] = half[0, 0] - F32(1.0)
    return q, np.ascontiguousarray(s, dtype=F32)


@pytest.mark.parametrize("nq,k", SCORE_SHAPES)
def test_distances_from_scores_clamp_and_missing(cuda_device, nq, k):
    D = 24
    q, s = score_lists(nq, k, D, nq * 10 + k)
    ref = R.scores_to_l2(s, q)
    assert not (ref < 0).any() and not np.signbit(ref).any()
    ix = _index(D, 1)
    ix.add(_dev(scaled_rows(10, D, 1)))
    got = ix.distances_from_scores(_dev(q), _dev(s.copy()))
    assert_bits(got, ref, f"distances_from_scores nq {nq}, k {k}")
    ix.close()
    ip = _index(D, 0)
    ip.add(_dev(scaled_rows(10, D, 1)))
    assert_bits(ip.distances_from_scores(_dev(q), _dev(s.copy())), s, "inner product: untouched")
    ip.close()


def test_a_query_equal_to_a_bank_row_is_at_distance_plus_zero(cuda_device):
    D = 100
    bank = scaled_rows(500, D, 61)
    q = bank[[3, 250, 499]].copy()
    ix = _index(D, 1)
    ix.add(_dev(bank))
    idx, sc = ix.search_scores(_dev(q), 4)
    ref = R.scores_to_l2(_np(sc), q)
    dist = ix.distances_from_scores(_dev(q), sc.clone())
    assert_bits(dist, ref, "distances of the sharded path")
    idx1, dist1 = ix.search(_dev(q), 4)
    assert_bits(dist1, ref, "distances of the single-index path")
    assert _np(idx1)[:, 0].tolist() == [3, 250, 499]
    assert not np.signbit(_np(dist1)).any() and (_np(dist1) >= 0).all()
    ix.close()


# ================================================================ merge_parts_kernel: hb_merge_topk / hb_merge_topk_packed

MERGE_LDS = 60000
MergeCase = namedtuple("MergeCase", "metric parts k nq pattern")
MERGE_CASES = (
    MergeCase(0, 1, 1, 1, "random"),
    MergeCase(1, 1, 30, 300, "missing"),
    MergeCase(0, 2, 30, 10000, "random"),
    MergeCase(1, 2, 30, 10000, "interleaved"),
    MergeCase(1, 3, 64, 300, "random"),
    MergeCase(0, 3, 64, 300, "equal"),
    MergeCase(0, 8, 256, 1, "random"),
    MergeCase(1, 8, 256, 300, "missing"),
    MergeCase(0, 16, 256, 1, "interleaved"),
    MergeCase(1, 16, 30, 300, "dup"),
    MergeCase(0, 2, 2048, 1, "missing"),
    MergeCase(1, 2, 2048, 1, "random"),
    MergeCase(0, 16, 1, 300, "zeros"),
    MergeCase(1, 8, 1, 10000, "equal"),
    MergeCase(0, 3, 30, 300, "dup"),
    MergeCase(1, 3, 30, 300, "zeros"),
    MergeCase(0, 8, 64, 300, "allmissing"),
    MergeCase(1, 2, 64, 1, "allmissing"),
    MergeCase(0, 8, 30, 300, "missing"),
    MergeCase(1, 16, 64, 1, "equal"),
    MergeCase(0, 2, 64, 300, "interleaved"),
)


def merge_inputs(c, seed):
    """Synthetic per-part lists [parts, nq, k], each sorted best first as a search leaves them (ties by id)."""
    rng = np.random.default_rng(seed)
    P, nq, k = c.parts, c.nq, c.k
    shape = (P, nq, k)
    if c.pattern == "interleaved":                   # few distinct scores; part p holds the ids = p mod parts
        val = rng.integers(0, 4, size=shape).astype(F32) * F32(0.5)
        idx = np.broadcast_to(np.arange(k)[None, None, :] * P + np.arange(P)[:, None, None], shape)
    elif c.pattern == "equal":
        val = np.full(shape, 1.5, dtype=F32)
        idx = np.stack([rng.permutation(P * k).reshape(P, k) for _ in range(min(nq, 8))], axis=1)[:, np.arange(nq) % min(nq, 8)]
    elif c.pattern == "zeros":
        val = np.where(rng.random(shape) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
        idx = np.stack([rng.permutation(P * k).reshape(P, k) for _ in range(min(nq, 8))], axis=1)[:, np.arange(nq) % min(nq, 8)]
    else:
        val = rng.standard_normal(shape).astype(F32)
        if c.metric == 1:
            val = np.abs(val)
        idx = np.stack([rng.permutation(P * k * 3)[:P * k].reshape(P, k) for _ in range(min(nq, 8))], axis=1)[:, np.arange(nq) % min(nq, 8)]
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if c.pattern == "dup" and P > 1:                 # part 1 found the same rows as part 0
        idx[1], val[1] = idx[0], val[0]
    key = val if c.metric == 1 else -val
    order = np.lexsort((idx, key), axis=-1)
    val, idx = np.take_along_axis(val, order, axis=-1), np.take_along_axis(idx, order, axis=-1)
    if c.pattern == "missing":                       # missing neighbours that carry +inf / -inf / very good / very bad / zero scores
        miss = rng.random(shape) < 0.3
        miss[:, :, -1] = True
        junk = np.array([np.inf, -np.inf, 1e30, -1e30, 0.0], dtype=F32)[rng.integers(0, 5, size=shape)]
        val, idx = np.where(miss, junk, val).astype(F32), np.where(miss, -1 - (rng.integers(0, 3, size=shape)), idx)
    if c.pattern == "allmissing":
        idx[:] = -1
    return np.ascontiguousarray(val, dtype=F32), np.ascontiguousarray(idx, dtype=np.int64)


def merge_lds_bytes(parts, k):
    n = parts * k
    return (n * 4 + 15) // 16 * 16 + n * 8          # hb_launch_merge_parts


@pytest.mark.parametrize("i", range(len(MERGE_CASES)), ids=lambda i: "m{0}-p{1}-k{2}-nq{3}-{4}".format(*MERGE_CASES[i]))
def test_merge_plain_and_packed_against_the_definition(cuda_device, i):
    from hbird_mi import _lib
    from hbird_mi.nn.search_hip import merge_topk, merge_topk_packed
    torch = _torch()
    c = MERGE_CASES[i]
    val, idx = merge_inputs(c, 600 + i)
    ridx, rval = R.merge(val, idx, c.metric)
    gidx, gval = merge_topk(_dev(val), _dev(idx), c.metric)
    assert_ints(gidx, ridx, f"merge {c}: ids")
    assert_bits(gval, rval, f"merge {c}: scores")
    # packed lists: [nq * k int64 ids][nq * k fp32 scores], `part_bytes` apart -- minimal, and with 64 bytes of padding
    nk = c.nq * c.k
    least = int(_lib.lib().hb_packed_list_bytes(c.nq, c.k))
    assert least >= nk * 12 and least % 16 == 0
    for part_bytes in (least, least + 64):
        raw = np.full((c.parts, part_bytes), 0xA5, dtype=np.uint8)
        for p in range(c.parts):
            raw[p, :nk * 8] = idx[p].reshape(-1).view(np.uint8)
            raw[p, nk * 8:nk * 12] = val[p].reshape(-1).view(np.uint8)
        pidx, pval = merge_topk_packed(_dev(raw).view(-1), part_bytes, c.parts, c.nq, c.k, c.metric)
        assert_ints(pidx, ridx, f"packed merge {c}, part_bytes {part_bytes}: ids")
        assert_bits(pval, rval, f"packed merge {c}, part_bytes {part_bytes}: scores")
    del torch


def test_merge_beyond_the_lds_limit_fails_and_writes_nothing(cuda_device):
    from hbird_mi import _lib
    torch = _torch()
    assert merge_lds_bytes(2, 2048) <= MERGE_LDS < merge_lds_bytes(3, 2048)
    val = torch.zeros((3, 2, 2048), dtype=torch.float32, device="cuda")
    idx = torch.zeros((3, 2, 2048), dtype=torch.int64, device="cuda")
    oi = torch.full((2, 2048), -7, dtype=torch.int64, device="cuda")
    od = torch.full((2, 2048), -7.0, dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for metric in (0, 1):
        rc = _lib.lib().hb_merge_topk(p(val), p(idx), 3, 2, 2048, metric, p(oi), p(od), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0 and "parts*k too large" in _lib.last_error()
    torch.cuda.synchronize()
    assert (oi == -7).all() and (od == -7.0).all()
