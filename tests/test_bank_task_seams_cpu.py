"""The case lists of test_linprobe_gpu.py and test_kmeans_gpu.py reach every bank-size seam of the linear probe and of k-means (no GPU needed).

The host code of csrc/hbird_linprobe.hip and csrc/hbird_kmeans.hip changes shape with the bank's row count and the class count; the dispatch
arithmetic is restated here with its sources, and the GPU case lists together must reach every forward instantiation at both ends of its class
tile, every backward grid depth with both tails, segments of 256 rows and longer, one and several workspace chunks with a ragged last one, all
four accumulate slots, a second trip, an empty trailing segment, several workgroups of the counting kernels, a split default staging chunk and a
tree index j >= 1 in both units.  Then four wrong variants of the numpy models -- a chunk that restarts at row 0, a segment cut at 256 rows, an
accumulate that stops after one trip or after slot 1 -- must move the result on the new worlds by more than 20 x the bound the GPU tests assert
(k-means: by at least one integer).  A case list that loses a seam fails here, before any GPU time is spent.
"""
import numpy as np

import kmeans_refs as KR
import linprobe_refs as LR
import test_kmeans_gpu as km
import test_linprobe_gpu as lp

# ---------------------------------------------------------------- the linear probe (csrc/hbird_linprobe.hip)
LP_ROWS = 256                                      # hbird_linprobe.hip:20, rows of a forward workgroup
LP_BWD_CTW = 2                                     # :22, class tiles of a backward wave
LP_TREE_ROWS = 256 * 256                           # :24 and :282, rows of one pass of the loss tree
WORKSPACE = 1 << 30                                # HB_LINPROBE_WORKSPACE, include/hbird_hip_linprobe.h


def lp_plan(C, D, rows, workspace=WORKSPACE):
    """hb_linprobe_loss_grad's launch arithmetic (:404-407 and the chunk loop :422-432; lp_forward :305-320; lp_backward :322-330)."""
    ct = -(-C // 32)                                                       # lp_params::make: the forward instantiation <CT>
    cp, xs = 32 * ct, 32 * -(-(D + 1) // 32)
    seg_rows, nseg = LR.partition(rows)
    seg_bytes = seg_rows * (cp + xs) * 4
    chunk_segs = min(nseg, max(1, workspace // seg_bytes))
    chunks = LR.chunks(rows, chunk_segs)
    if ct == 1:                                                            # linprobe_backward_kernel<1>, gridDim.z = 1
        bwd, grid_z, tails = 1, 1, {1}
    else:                                                                  # <2>: nt = min(2, ct - 2 z) per z
        bwd, grid_z = LP_BWD_CTW, -(-ct // LP_BWD_CTW)
        tails = {min(LP_BWD_CTW, ct - LP_BWD_CTW * z) for z in range(grid_z)}
    return dict(ct=ct, full_tile=C == 32 * ct, one_in_last_tile=C == 32 * (ct - 1) + 1, cp=cp, xs=xs, g8=-(-D // 8), lds=ct * 8 * 1024,
                seg_rows=seg_rows, nseg=nseg, seg_bytes=seg_bytes, chunks=chunks, row0s=[c[0] for c in chunks], bwd=bwd, grid_z=grid_z, tails=tails,
                fwd_blocks=-(-rows // LP_ROWS), tree_j=(rows - 1) // LP_TREE_ROWS)


def lp_cases():
    """(spec, workspace bytes) of every loss_grad evaluation the GPU tests make."""
    whole = [(spec, WORKSPACE) for spec, P in lp.ALL_WORLDS + lp.TILE_CASES + [lp.BIG_CASE]]
    return whole + [(spec, segs * lp.seg_bytes(spec)) for spec, P, segs in lp.CHUNK_CASES]


def test_seg_bytes_of_the_gpu_tests_is_the_launchers():
    for spec, P, segs in lp.CHUNK_CASES:
        assert lp.seg_bytes(spec) == lp_plan(*spec[:3])["seg_bytes"]
    assert lp.seg_bytes(LR.SEGMENT_WORLD) == 65536


def test_probe_cases_reach_every_forward_instantiation_at_both_ends():
    plans = [lp_plan(*spec[:3], workspace=ws) for spec, ws in lp_cases()]
    for ct in range(1, 9):
        mine = [p for p in plans if p["ct"] == ct]
        assert any(p["full_tile"] for p in mine), f"no case with C = {32 * ct}"
        assert any(p["one_in_last_tile"] for p in mine) or ct == 1, f"no case with C = {32 * (ct - 1) + 1}"
    assert max(p["lds"] for p in plans) == 64 * 1024                       # <8>: the default limit of dynamic LDS, exactly
    assert any(p["ct"] == 8 and p["g8"] > 8 for p in plans)                # ... staged in two rounds (LP_GC = 8 column groups at a time)
    assert any(p["ct"] >= 7 and p["g8"] == 48 for p in plans)              # a wide bank under many class tiles
    assert all(p["fwd_blocks"] >= 2 for p in plans if p["ct"] > 2)         # more than one forward workgroup, a ragged last one
    assert all(spec[2] % 32 for spec, _ in lp.TILE_CASES + [lp.BIG_CASE])


def test_probe_cases_reach_every_backward_grid_depth_with_both_tails():
    plans = [lp_plan(*spec[:3], workspace=ws) for spec, ws in lp_cases()]
    assert {p["grid_z"] for p in plans if p["bwd"] == 2} == {1, 2, 3, 4} and {p["bwd"] for p in plans} == {1, 2}
    for z in (2, 3, 4):                                                    # (ct = 2 z - 1 and 2 z; at z = 1 the one-tile tail is kernel <1>'s)
        assert {t for p in plans if p["bwd"] == 2 and p["grid_z"] == z for t in p["tails"]} == {1, 2}, z
    assert {p["xs"] for p in plans} >= {32, 96, 416}                       # gridDim.x = 1, 3 and 13 column tiles


def test_probe_cases_reach_long_segments_chunk_counts_and_the_loss_tree():
    plans = {(spec, ws): lp_plan(*spec[:3], workspace=ws) for spec, ws in lp_cases()}
    assert {p["seg_rows"] for p in plans.values()} == {256, 512}
    big = plans[(LR.BIG_WORLD, WORKSPACE)]
    assert (big["seg_rows"], big["nseg"], len(big["chunks"]), big["tree_j"]) == (512, 257, 1, 2) and big["chunks"][0][1] % 512 == 123
    counts = sorted(len(p["chunks"]) for p in plans.values())
    assert counts[0] == 1 and {2, 3, 86} <= set(counts)
    chunked = [p for p in plans.values() if len(p["chunks"]) > 1]
    assert any(p["chunks"][-1][2] < p["chunks"][0][2] for p in chunked)   # a last chunk of fewer segments ...
    assert all(p["chunks"][-1][1] % LP_ROWS for p in chunked)             # ... and of a ragged row count, every time
    assert any(p["ct"] == 8 for p in chunked) and any(p["seg_rows"] == 512 for p in chunked)
    assert any(max(p["row0s"]) >= LP_TREE_ROWS for p in chunked)          # chunk offsets past one pass of the tree
    by_case = {(spec, segs): plans[(spec, segs * lp.seg_bytes(spec))] for spec, P, segs in lp.CHUNK_CASES}
    assert [c[2] for c in by_case[(LR.SEGMENT_WORLD, 1)]["chunks"]] == [1, 1, 1] and [c[2] for c in by_case[(LR.SEGMENT_WORLD, 2)]["chunks"]] == [2, 1]
    last = by_case[(LR.BIG_WORLD, 3)]["chunks"]
    assert len(last) == 86 and last[-1][2] == 2
    assert {lp_plan(*spec[:3])["tree_j"] for spec, _ in lp_cases()} == {0, 2}


# ---------------------------------------------------------------- k-means (csrc/hbird_kmeans.hip)
KM_CHUNK_ROWS = 131072                             # HB_KMEANS_CHUNK_ROWS, include/hbird_hip_kmeans.h
KM_TREE_ROWS = 256 * 256                           # hbird_kmeans.hip:23 and :143


def km_blocks(n, per_block, cap):
    return max(1, min(cap, -(-n // per_block)))                            # :190


def km_plan(row0, n):
    """km_accumulate's launch (:234-248) and the kernel's walk (:36-46)."""
    rt_begin, rt_end, segs, seg_tiles = KR.km_segments(row0, n)
    walk = KR.walked_tiles(row0, n)
    empty = [s for s in range(segs) if rt_begin + s * seg_tiles >= rt_end]
    return dict(nt=rt_end - rt_begin, segs=segs, seg_tiles=seg_tiles, slots={u for _, _, _, u, _ in walk}, trips={p for *_, p in walk},
                empty_segments=empty, tiles=sorted(t for t, *_ in walk), count_blocks=km_blocks(n, 4096, 1024))


def km_stage_chunks(n, chunk_rows):
    chunk = max(1, min(chunk_rows, n) if chunk_rows > 0 else min(n, KM_CHUNK_ROWS))      # km_stage::ensure, :196
    return [(r, min(chunk, n - r)) for r in range(0, n, chunk)]


def test_restated_walk_covers_every_tile_once_at_any_range():
    g = np.random.default_rng(1)
    for row0, n in [(0, 1), (0, 4000), (5, 70), (0, KR.BIG_ROWS)] + km.BIG_SPLITS + [(int(a), int(b)) for a, b in zip(g.integers(0, 60000, 20), g.integers(1, 71000, 20))]:
        p = km_plan(row0, n)
        assert p["tiles"] == list(range(row0 >> 5, (row0 + n + 31) >> 5)), (row0, n)


def test_kmeans_cases_reach_every_slot_a_second_trip_and_an_empty_segment():
    whole = km_plan(0, KR.BIG_ROWS)                                        # _check_update at BIG_UPDATE_K, the big fit, the whole call of the split test
    assert (whole["nt"], whole["segs"], whole["seg_tiles"]) == (4100, 128, 33)
    assert whole["slots"] == {0, 1, 2, 3} and whole["trips"] == {0, 1} and len(whole["empty_segments"]) == 3
    assert set(km.BIG_UPDATE_K) == {5, 2048}                               # the smallest and the largest LDS table (128 KiB) under that walk
    assert whole["count_blocks"] == 33 and km_blocks(4000, 4096, 1024) == 1      # kmeans_counts_kernel and kmeans_changed_kernel: atomics of 33 workgroups meet
    small = km_plan(0, 4000)                                               # what the suite had: slots 0 and 1, one trip
    assert small["slots"] == {0, 1} and small["trips"] == {0} and not small["empty_segments"]
    splits = [km_plan(r, n) for r, n in km.BIG_SPLITS]
    assert all(r % 32 for r, n in km.BIG_SPLITS[1:]) and (km.BIG_SPLITS[1][0] + km.BIG_SPLITS[1][1]) % 32 and KR.BIG_ROWS % 32
    assert (km.BIG_SPLITS[1][0] + km.BIG_SPLITS[1][1]) >> 5 == (KR.BIG_ROWS - 1) >> 5      # the middle range ends inside the bank's last tile
    assert splits[0]["slots"] == {0, 1, 2} and splits[0]["seg_tiles"] == 17 and splits[1]["slots"] == {0, 1, 2} and splits[2]["nt"] == 1
    assert km.BIG_SPLITS[0][1] > 65536 and splits[0]["nt"] >= 2049         # slot 2 alone: a range of more than 65,536 rows


def test_kmeans_cases_split_the_default_staging_chunk_and_reach_the_tree():
    assert km.BIG_ASSIGN_CHUNKS == (0, 64 * 1024)
    assert km_stage_chunks(KR.BIG_ROWS, 0) == [(0, 131072), (131072, 123)] and len(km_stage_chunks(KR.BIG_ROWS, 64 * 1024)) == 3
    assert km_stage_chunks(4000, 0) == [(0, 4000)]                         # what the suite had
    row0, n = km.BIG_SAMPLE
    assert n == 4096 and row0 < KM_CHUNK_ROWS < row0 + n == KR.BIG_ROWS
    assert (KR.BIG_ROWS - 1) // KM_TREE_ROWS == 2 and KR.BIG_HOLE // KM_TREE_ROWS == 1


# ---------------------------------------------------------------- wrong variants of the models, on the new worlds
def _residuals(w, x, seed):
    Wb = (np.random.default_rng(seed).standard_normal((w["C"], w["D"] + 1))).astype(np.float32)
    z, skip = LR.chain_logits(x, Wb)
    return LR.objective(z, x, w["y"], Wb, 1e-2, skip)["R"].astype(np.float32), skip


def test_a_chunk_that_restarts_at_row_0_moves_the_gradient_by_more_than_20_bounds():
    for spec, P, segs in lp.CHUNK_CASES:
        w = LR.big_world() if spec == LR.BIG_WORLD else LR.world(spec, P)
        x = w["x"]
        R32, skip = _residuals(w, x, 5)
        n = LR.used_rows(skip)
        right = LR.chunked_sums(R32, x, skip, segs) / n
        assert np.abs(right - LR.chunked_sums(R32, x, skip) / n).max() <= 1e-12                     # the chunks do not show in the right model
        wrong = LR.chunked_sums(R32, x, skip, segs, staged_from_row_0=True) / n
        moved = np.abs(wrong - right) / LR.gradient_bound(R32, x, skip)
        assert moved[:, 1:].max() > 20, (spec, segs, moved.max())                                   # (column 0, the staged ones, can only tell by a skipped row)


def test_a_segment_cut_at_256_rows_moves_the_big_gradient_by_more_than_20_bounds():
    w = LR.big_world()
    R32, skip = _residuals(w, w["x"], 5)
    n = LR.used_rows(skip)
    bound = LR.gradient_bound(R32, w["x"], skip)
    for segs in (None, 3):
        right = LR.chunked_sums(R32, w["x"], skip, segs) / n
        wrong = LR.chunked_sums(R32, w["x"], skip, segs, segment_cut=256) / n
        assert (np.abs(wrong - right) / bound).max() > 20, segs
    # ... and on the small worlds, whose segments are 256 rows, the cut is no cut: only the big world can tell
    s = LR.world(LR.SEGMENT_WORLD)
    R32, skip = _residuals(s, s["x"], 5)
    assert np.array_equal(LR.chunked_sums(R32, s["x"], skip, None, segment_cut=256), LR.chunked_sums(R32, s["x"], skip))


def test_an_accumulate_that_stops_early_moves_the_big_sums_by_whole_integers():
    g = np.random.default_rng(20 + 5)
    x = g.uniform(-1, 1, (KR.BIG_ROWS, km.BIG_D)).astype(np.float32)
    a = np.where(g.random(KR.BIG_ROWS) < 0.1, -1, g.integers(0, 5, KR.BIG_ROWS)).astype(np.int32)
    S = KR.integer_sums(x, a, 5)[0]
    assert np.array_equal(KR.walked_sums(x, a, 5), S)
    one_trip, two_slots = KR.walked_sums(x, a, 5, trips=1), KR.walked_sums(x, a, 5, slots=2)
    assert np.abs(one_trip - S).min() >= 1 and np.abs(two_slots - S).min() >= 1                     # every one of the K x D sums moves
    # ... while at the sizes the suite had neither variant shows: only the big bank can tell
    xs, as_ = x[:4000], a[:4000]
    assert np.array_equal(KR.walked_sums(xs, as_, 5, trips=1), KR.integer_sums(xs, as_, 5)[0])
    assert np.array_equal(KR.walked_sums(xs, as_, 5, slots=2), KR.integer_sums(xs, as_, 5)[0])
    # the split ranges of the GPU test each lose tiles to a walk that stops after slot 1
    for row0, n in km.BIG_SPLITS[:2]:
        masked = np.full(KR.BIG_ROWS, -1, dtype=np.int32); masked[row0:row0 + n] = a[row0:row0 + n]
        assert not np.array_equal(KR.walked_sums(x, a, 5, row0, n, slots=2), KR.integer_sums(x, masked, 5)[0])
