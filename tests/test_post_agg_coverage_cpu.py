"""The case lists of test_aggregate_paths_gpu.py and test_post_paths_gpu.py reach every launch path of K5, K6 and K7 (no GPU needed).

The dispatch decisions are restated here from the launch code, with their sources; each GPU case's declared branch must be what the
launcher picks, and the lists together must reach every branch, table form, rows-per-chunk choice and confusion-counting path.  A
case list that loses a path fails here, before any GPU time is spent.
"""
import math

import numpy as np

import oracle
import test_aggregate_paths_gpu as agg
import test_post_paths_gpu as post

# ---------------------------------------------------------------- K5: hb_launch_aggregate (csrc/hbird_aggregate.hip, body in csrc/hbird_k5_dev.h)

AGG_LUT = 2048                                     # K5_LUT of hbird_k5_dev.h


def agg_table(form, C):
    """(uint16?, row stride in elements, 16-byte aligned base?, P) of a table form.
    Own rows: hb_label_store::view (hbird_labels.h, called by hb_k5_table_choose of hbird_aggregate.hip) with stride() = counts padded to 8,
    device allocations aligned.  Borrowed rows: its `borrowed()` branch -- dense [n, C], stride C."""
    P = agg.FORM_P[form]
    if form == "own_f32":
        return False, C, True, 0
    if form.startswith("own_u16"):
        return True, (C + 7) & ~7, True, P
    if form == "ext_f32":
        return False, C, True, 0
    return True, C, form != "ext_u16_mis", P


def agg_branch(form, C):
    """aggregate_kernel's body (k5_body, hbird_k5_dev.h): C <= 32 first, then `U16 && wide` with hb_k5_table_choose's `wide` --
    stride % 8 == 0, 16-byte aligned base, 0 < P <= K5_LUT, 32 < C <= 512 -- else the generic loop."""
    u16, stride, aligned, P = agg_table(form, C)
    if C <= 32:
        return "grouped"
    wide_ok = stride % 8 == 0 and aligned and 0 < P <= AGG_LUT and 32 < C <= 512
    return "wide" if u16 and wide_ok else "generic"


def agg_table_label(form, C):
    """Table forms as the issue of this coverage names them: borrowed count tables split by C % 8."""
    if form == "ext_u16":
        return "ext_u16_c8" if C % 8 == 0 else "ext_u16_odd"
    return form


def test_k5_cases_declare_the_branch_the_launcher_picks():
    for c in agg.CASES + agg.SHARD_CASES:
        assert agg_branch(c.form, c.C) == c.branch, agg.case_id(c)


def test_k5_cases_reach_every_branch_with_every_table_form():
    forms = list(agg.FORM_P)
    possible = {(agg_branch(f, C), agg_table_label(f, C)) for f in forms for C in range(1, 1025)}
    hit = {(c.branch, agg_table_label(c.form, c.C)) for c in agg.CASES}
    assert possible - hit == set(), f"branch x table form pairs no case reaches: {sorted(possible - hit)}"
    assert len(possible) == 16
    assert {c.branch for c in agg.SHARD_CASES} == {"grouped", "wide", "generic"}


def test_k5_cases_cover_the_value_lists():
    cs = agg.CASES
    assert {1, 2, 3, 21, 31, 32, 33, 64, 65, 151, 152, 512, 513, 1000} <= {c.C for c in cs}
    assert {1, 7, 8, 9, 63, 64, 65, 90, 200, 256} <= {c.k for c in cs}
    assert {c.metric for c in cs} == {"ip", "l2"} and {c.beta for c in cs} == {0.02, 0.07, 1.0}
    for m in ("ip", "l2"):
        assert {c.qs for c in cs if c.metric == m} == {1, 30, 300, 1000}, m
    assert any(c.id_base and c.form.startswith("own") for c in cs)
    assert max(c.k for c in cs) <= 256 and all(c.k <= 256 for c in agg.SHARD_CASES)
    assert 0 in agg.SHARD_ROWS and len(set(agg.SHARD_ROWS)) == 3
    assert {21, 151, 1000} == {C for C, _ in agg.FUSED_CASES} and {30, 256} == {k for _, k in agg.FUSED_CASES}


def test_k5_neighbour_patterns_and_sensitivity_on_the_host():
    """The neighbour-list patterns appear in every case, and the float64 reference of every case moves by more than 20 x its
    tolerance when a neighbour is dropped or a class is one count off (host norms stand in for the index's stored ones)."""
    for i, c in enumerate(agg.CASES):
        h = agg.make_case(c, i + 1)
        norms = np.linalg.norm(h["bank"].astype(np.float64), axis=1).astype(np.float32)
        base = c.id_base if c.form.startswith("own") else 4321
        idx, dist = agg._neighbours(h["rng"], c.k, h["n"], base, c.beta, c.metric, h["q"], norms.astype(np.float64))
        pat = np.arange(agg.NQ) % agg.NQ_PATTERNS
        assert (idx[pat == 4] == -1).all()
        if c.k > 2:
            assert (idx[pat == 1][:, 0] == -1).all() and (idx[pat == 3][:, -1] == -1).all()
            assert ((idx[pat == 5] >= base + h["n"]).any(axis=1)).all()
            assert all(len(set(r)) < len(r) for r in idx[pat == 6])
        ref, w, logits = agg.reference(h["q"], idx, dist, norms, base, h["labels"], base, c.beta, c.metric)
        tol = agg.tolerance(h["q"], idx, dist, norms, base, logits, c.k, c.beta, c.metric, float(h["labels"].max()))
        s_drop, s_shift = agg._sensitivity(h["q"], idx, dist, norms, base, h["labels"], base, c.beta, c.metric, h["P"], ref, w, tol)
        assert s_drop > 20 and s_shift > 20, (agg.case_id(c), s_drop, s_shift)


# ---------------------------------------------------------------- K6 / K7: hb_launch_upsample_argmax_confusion, hb_launch_confusion
# (csrc/hbird_post.hip)

K6_HIST_BYTES = 16 * 1024                          # hbird_post.hip:51


def source_rows(S, n):
    """Upper source index of every output row, fp32 as in the launcher (hbird_post.hip:198-205)."""
    s = np.float32(S) / np.float32(n)
    f = np.maximum(s * (np.arange(n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    return np.minimum(np.floor(f).astype(np.int64), S - 1)


def k6_plan(S, C, h, w, G=0, P=0):
    """The launch arithmetic of hb_launch_upsample_argmax_confusion: tallest band (hbird_post.hip:199-207), rows per chunk R -- the
    option with the fewest padded rows, 16 first on ties (:208-225) -- chunks (:226), block width (:229), staged columns and classes per
    LDS pass (:231-232), and where the confusion counts go (:233-245: a G x P histogram within 16 KiB, else 2^8 or 2^9 hash entries)."""
    bands = np.unique(source_rows(S, h), return_counts=True)[1]
    maxband = int(bands.max())
    R, best = 16, None
    for r in (16, 14, 12, 10, 8):
        cost = int(sum((n + r - 1) // r * (r + 1) for n in bands))
        if best is None or cost < best:
            best, R = cost, r
    chunks = (maxband + R - 1) // R
    waves = (w + 63) // 64
    blocks_x = (waves + 3) // 4
    bw = (waves + blocks_x - 1) // blocks_x * 64
    ncols = min(S, math.ceil(bw * S / w) + 2)
    cmax = max(1, min(C, (64 * 1024) // (2 * ncols * 4)))
    hbits = None
    if G:
        if G * P * 4 <= K6_HIST_BYTES:
            hbits = 0
        else:
            hbits = 8
            while hbits < 9 and (8 << (hbits + 1)) <= 2 * ncols * cmax * 4:
                hbits += 1
    return dict(maxband=maxband, R=R, chunks=chunks, bw=bw, ncols=ncols, cmax=cmax, passes=-(-C // cmax), hbits=hbits)


def confusion_paths(c, seed):
    """Which counting paths of upsample_argmax_kernel's confusion tail (hbird_post.hip:127-184) the fused case takes.  Per workgroup
    (<= R rows of a band x bw columns) and wave row: up to 8 leader rounds (:161-171); after round 3 a leader that stands alone among
    more than 16 ungrouped lanes ends the rounds and the rest go straight to the matrix (the noise shortcut, :168, tables only);
    everything else goes through count() (:139-148).  A workgroup whose count() calls bring more distinct pairs than the table has
    entries must overflow to global atomics (:147)."""
    lh, gt = post.fused_inputs(c, seed)
    pred = oracle.upsample_argmax(lh, c.S, c.h, c.w)
    p = k6_plan(c.S, c.C, c.h, c.w, c.G, c.P)
    hb = p["hbits"]
    paths = {"hist" if hb == 0 else f"hash{hb}"}
    g = gt[:, 0]
    valid = (g >= 0) & (g < c.G) & (pred[:, 0] < c.P)
    if c.ignore is not None:
        valid &= g != c.ignore
    key = np.where(valid, g * c.P + pred[:, 0], -1)
    rows = source_rows(c.S, c.h)
    for b in range(c.B):
        for j in np.unique(rows):
            band = np.flatnonzero(rows == j)
            for r0 in range(0, len(band), p["R"]):
                chunk = band[r0:r0 + p["R"]]
                for xs in range(0, c.w, p["bw"]):
                    counted = set()
                    for y in chunk:
                        for x0 in range(xs, min(xs + p["bw"], c.w), 64):
                            k = key[b, y, x0:x0 + 64]
                            todo = k >= 0
                            noise = False
                            for rnd in range(8):
                                if not todo.any():
                                    break
                                k0 = k[np.flatnonzero(todo)[0]]
                                same = (k == k0) & todo
                                if rnd >= 3 and hb and same.sum() == 1 and todo.sum() > 16:
                                    noise = True
                                    break
                                counted.add(int(k0))
                                todo &= ~same
                            if noise:
                                paths.add("noise")
                            else:
                                counted.update(int(v) for v in k[todo])
                    if hb and len(counted) > (1 << hb):
                        paths.add("overflow")
    return paths


def test_k6_cases_reach_every_launch_path():
    plans = [k6_plan(c.S, c.C, c.h, c.w) for c in post.K6_CASES]
    assert {p["R"] for p in plans} == {8, 10, 12, 14, 16}
    assert any(p["maxband"] > 16 for p in plans) and any(p["chunks"] > 2 for p in plans)
    assert any(p["passes"] >= 2 for p in plans) and any(p["passes"] >= 3 for p in plans)
    assert any(c.S == 1 for c in post.K6_CASES) and any(c.w < 64 for c in post.K6_CASES)
    assert any(c.h < c.S for c in post.K6_CASES) and any(c.w < c.S for c in post.K6_CASES)
    assert {2, 7, 37, 64} <= {c.S for c in post.K6_CASES} and {1, 2, 151} <= {c.C for c in post.K6_CASES}
    for c in post.K6_CASES + post.FUSED_CASES:
        assert c.C * c.h * c.w <= 4e7, c
    p = k6_plan(37, 1000, 128, 128)                 # the ties across passes in test_k6_ties_go_to_the_lowest_class
    assert p["cmax"] == 221 and p["passes"] == 5
    assert k6_plan(64, 1000, 5, 896)["passes"] == 3


def test_fused_cases_reach_every_confusion_path():
    paths, plans = set(), []
    for i, c in enumerate(post.FUSED_CASES):
        paths |= confusion_paths(c, 100 + i)
        plans.append(k6_plan(c.S, c.C, c.h, c.w, c.G, c.P))
    assert {"hist", "hash8", "hash9", "overflow", "noise"} <= paths, paths
    G, P = {c.G for c in post.FUSED_CASES}, {c.P for c in post.FUSED_CASES}
    assert {21, 64, 65, 151, 300} <= {c.G for c in post.FUSED_CASES if c.G == c.P}
    assert any(c.G < c.P for c in post.FUSED_CASES) and any(c.G > c.P for c in post.FUSED_CASES)
    assert {c.pattern for c in post.FUSED_CASES} == {"one", "rects", "noise", "checker"}
    assert {c.ignore for c in post.FUSED_CASES} == {None, 255, 0}
    assert any(p["passes"] >= 2 for p in plans) and G and P


def test_k7_cases_straddle_the_lds_limit():
    use_lds = [G * P * 4 <= 120 * 1024 for G, P in post.K7_CASES]     # hbird_post.hip:381
    sq = [(G, P) for G, P in post.K7_CASES if G == P]
    nsq = [(G, P) for G, P in post.K7_CASES if G != P]
    assert {G * P * 4 <= 120 * 1024 for G, P in sq} == {True, False}
    assert {G * P * 4 <= 120 * 1024 for G, P in nsq} == {True, False}
    assert any(use_lds) and not all(use_lds)
