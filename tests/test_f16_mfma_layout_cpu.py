"""The lane / register algebra of the 16x16x32 stage loop of the fp16 candidate kernel (csrc/hbird_knn_f16.hip), restated on the host.

A wave tile is 32 queries x 256 bank rows.  The shared tile epilogue (hbird_knn_dev.h: HB_SCAN_REG) assumes the layout of the 32x32x16
MFMA: lane l owns query l & 31, and accumulator register acc[t][4 g + j] (t = 0..7, g = 0..3, j = 0..3) is tile row
32 t + 8 g + 4 h + j with h = l >> 5.

The 16x16x32 loop sums the same tile as 16 row fragments f = 2 t + f' of 16 rows times 2 query fragments b of 16 queries.  One MFMA leaves,
in lane (s = l >> 4, n = l & 15), register j: query 16 b + n, MFMA row 4 s + j of its fragment; it lives in register 8 f' + 4 b + j of
acc[t].  The bank fragment's MFMA row m is fed tile row rho(f', m) = 16 f' + 8 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3).  At a tile's end one
v_permlane16_swap per register pair (8 f' + j, 8 f' + 4 + j) exchanges the ODD 16-lane rows of the first with the EVEN rows of the second.
This file enumerates all 64 lanes x 128 registers and asserts that the result is the epilogue's layout, does the same for the pre-swap
layout of the row-init values, and shows that each of four wrong variants fails a named assertion."""
import numpy as np
import pytest


def rho(fp, m):
    return 16 * fp + 8 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3)


def mfma_layout(rho_fn=rho):
    """Pre-swap contents: (query, row) [64 lanes, 8 t, 16 registers] as the MFMAs leave them."""
    query = np.empty((64, 8, 16), dtype=np.int64)
    row = np.empty((64, 8, 16), dtype=np.int64)
    for l in range(64):
        s, n = l >> 4, l & 15
        for t in range(8):
            for fp in range(2):
                for b in range(2):
                    for j in range(4):
                        r = 8 * fp + 4 * b + j
                        query[l, t, r] = 16 * b + n
                        row[l, t, r] = 32 * t + rho_fn(fp, 4 * s + j)
    return query, row


def permlane16_swap(x, y, parity="odd_first_even_second"):
    """v_permlane16_swap_b32 on two registers [64 lanes, ...]: rows of 16 lanes; the odd rows of x change places with the even rows of y."""
    x, y = x.copy(), y.copy()
    for p in range(2):
        if parity == "odd_first_even_second":
            a, b = slice(32 * p + 16, 32 * p + 32), slice(32 * p, 32 * p + 16)
        else:                                   # mutation: the even rows of x with the odd rows of y
            a, b = slice(32 * p, 32 * p + 16), slice(32 * p + 16, 32 * p + 32)
        tmp = x[a].copy()
        x[a] = y[b]
        y[b] = tmp
    return x, y


def swap_tile(v, parity="odd_first_even_second", do_swap=True):
    """F2_SWAP_TILE on [64, 8, 16]: register pairs (8 f' + j, 8 f' + 4 + j)."""
    v = v.copy()
    if not do_swap:
        return v
    for fp in range(2):
        for j in range(4):
            a, b = 8 * fp + j, 8 * fp + 4 + j
            v[:, :, a], v[:, :, b] = permlane16_swap(v[:, :, a], v[:, :, b], parity)
    return v


def epilogue_layout():
    """What the shared epilogue assumes: the 32x32x16 MFMA's (query, row) [64, 8, 16]."""
    query = np.empty((64, 8, 16), dtype=np.int64)
    row = np.empty((64, 8, 16), dtype=np.int64)
    for l in range(64):
        h = l >> 5
        for t in range(8):
            for g in range(4):
                for j in range(4):
                    query[l, t, 4 * g + j] = l & 31
                    row[l, t, 4 * g + j] = 32 * t + 8 * g + 4 * h + j
    return query, row


def init_rows(layout="pre_swap"):
    """F2_INIT_TILE: the tile row whose init value lane l writes into acc[t][r], [64, 8, 16].  The kernel reads the f32x4 quad
    8 t + 4 f' + ri with ri = 2 (s & 1) + (s >> 1) and writes its four values to registers 8 f' + j and 8 f' + 4 + j."""
    row = np.empty((64, 8, 16), dtype=np.int64)
    for l in range(64):
        s, h = l >> 4, l >> 5
        ri = 2 * (s & 1) + (s >> 1)
        for t in range(8):
            if layout == "pre_swap":
                for fp in range(2):
                    for j in range(4):
                        row[l, t, 8 * fp + j] = row[l, t, 8 * fp + 4 + j] = 4 * (8 * t + 4 * fp + ri) + j
            else:                               # mutation: the 32x32x16 loop's init (the post-swap layout)
                for g in range(4):
                    for j in range(4):
                        row[l, t, 4 * g + j] = 4 * (8 * t + 2 * g + h) + j
    return row


def check(rho_fn=rho, parity="odd_first_even_second", do_swap=True, init_layout="pre_swap"):
    """-> the names of the assertions that fail: lane_owns_one_query, rows_match_epilogue, tile_covered_once, init_matches_mfma_rows."""
    bad = []
    q_pre, r_pre = mfma_layout(rho_fn)
    q, r = swap_tile(q_pre, parity, do_swap), swap_tile(r_pre, parity, do_swap)
    q_ref, r_ref = epilogue_layout()
    if not np.array_equal(q, q_ref):
        bad.append("lane_owns_one_query")
    if not np.array_equal(r, r_ref):
        bad.append("rows_match_epilogue")
    seen = np.zeros((32, 256), dtype=np.int64)
    np.add.at(seen, (q.reshape(-1), r.reshape(-1)), 1)
    if not (seen == 1).all():
        bad.append("tile_covered_once")
    # the init value must be that of the row the MFMAs then sum into the register, before any swap
    if not np.array_equal(init_rows(init_layout), r_pre):
        bad.append("init_matches_mfma_rows")
    return bad


def test_all_lanes_and_registers_land_on_the_epilogue_layout():
    q_pre, r_pre = mfma_layout()
    assert q_pre.shape == (64, 8, 16) and q_pre.size == 64 * 128
    assert check() == []
    # rho is a permutation of every half tile, and the b128 lane groups of the LDS read (four groups of 16 lanes) hit 16 distinct
    # 16-byte columns of the 256-byte bank row
    assert sorted(rho(0, m) for m in range(16)) == list(range(16)) and sorted(rho(1, m) for m in range(16)) == list(range(16, 32))
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    for g in groups:
        offs = [((l >> 5) * 1024 + (((l >> 4) & 1) * 32 + rho(0, l & 15)) * 16) % 256 for l in g]
        assert sorted(offs) == list(range(0, 256, 16)), (g, offs)


def test_query_fragment_offsets_cover_the_stage_blocks():
    # lane (c, n) of fragment b reads k-chunk c of query 16 b + n: block c >> 1, half c & 1 of [h][i][8 halves]
    seen = set()
    for b in range(2):
        for l in range(64):
            c, n = l >> 4, l & 15
            off = (c >> 1) * 1024 + ((c & 1) * 32 + n) * 16 + 256 * b
            blk, rest = divmod(off, 1024)
            hh, i = divmod(rest // 16, 32)
            assert (2 * blk + hh, i) == (c, 16 * b + n)
            seen.add(off)
    assert sorted(seen) == list(range(0, 2048, 16))


@pytest.mark.parametrize("kw, must_fail", [
    (dict(rho_fn=lambda fp, m: 16 * fp + 8 * ((m >> 2) & 1) + (m & 3)), {"rows_match_epilogue", "tile_covered_once"}),
    (dict(parity="even_first_odd_second"), {"lane_owns_one_query"}),
    (dict(do_swap=False), {"lane_owns_one_query", "rows_match_epilogue"}),
    (dict(init_layout="post_swap"), {"init_matches_mfma_rows"}),
], ids=["rho_without_4x_m_shr_3", "swap_of_the_wrong_parity", "no_swap", "init_in_post_swap_layout"])
def test_each_mutation_fails_its_named_assertion(kw, must_fail):
    bad = set(check(**kw))
    assert must_fail <= bad, (kw, bad)
    if "init_layout" in kw:
        assert bad == must_fail          # the accumulators themselves are untouched by a wrong init layout
