"""Sub-bank views on the GPU: hb_index_add_from / hb_index_select_rows (csrc/hbird_select.hip) through HipFlatIndex.add_from / select_rows.

A view must hold the selected rows of its source BIT FOR BIT -- tiles, norms, L2 row constants, label rows in their stored form -- whatever
the destination's fill (empty, a ragged row0, a capacity growth between two calls), and must search like an index built from those rows."""
import functools

import numpy as np
import pytest
import torch

import f16_screen_worlds as fw
import golden_inputs as gi
import oracle
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex, k5
from hbird_mi.views import view_rows

pytestmark = pytest.mark.gpu

N, BLOCK, KEEP, NQ = 1000, 49, 7, 64
METRIC_NAME = {0: "dot_product", 1: "l2"}
# (D, metric) -> (classes, label denominator; 0 = fp32 rows).  D = 20: Dp = 32 (padded k); counts: C = 21 -> stride 24, C = 151 -> 152;
# fp32 rows: C = 21 (84-byte rows, copied as floats) and C = 20 (80-byte rows, copied as 16-byte pieces)
SOURCES = {(20, 0): (21, 64), (20, 1): (151, 64), (384, 0): (21, 0), (384, 1): (20, 0), (384, 2): (21, 64)}
NAN_ROWS = (50, 777)


def _i32(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).contiguous().view(torch.int32).cpu()


def _rows(D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[900:] *= 8.0                      # rows of 8 x the norm
    x[NAN_ROWS[0]] = np.nan
    x[NAN_ROWS[1], 3] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def _source(D, variant):
    """1,000 rows (31 row tiles and a ragged one), label rows, NaN rows; variant 0 / 1 = the metric, 2 = inner product with count labels."""
    metric = variant if variant < 2 else 0
    C, P = SOURCES[(D, variant)]
    x = _rows(D, 100 + D + variant)
    lab = gi.labels_from_masks(N, C, 64, seed=7 + variant)
    ix = HipFlatIndex(D, metric, 0)
    if P:
        ix.set_label_denominator(P)
    ix.add(torch.from_numpy(x[:900]).cuda(), normalize=False)
    ix.add(torch.from_numpy(x[900:]).cuda(), normalize=False)
    ix.add_labels(torch.from_numpy(lab).cuda()); ix.set_num_classes(C)
    all_ids = torch.arange(N, device="cuda")
    ref = {"rows": ix.reconstruct(all_ids), "norms": ix.copy_norms(), "lab": ix.gather_labels(all_ids),
           "counts": ix.copy_label_counts() if P else None}
    assert np.array_equal(_i32(ref["rows"]).numpy(), _i32(x).numpy())
    torch.cuda.synchronize()
    return ix, ref, metric, C, P


def _selection(name):
    rng = np.random.default_rng(11)
    if name == "prefix":                # per-image prefixes: blocks of 49, first 7 (the last block is ragged)
        return view_rows(list(range(0, N, BLOCK)) + [N], per_block=KEEP)
    if name == "perm":
        return torch.from_numpy(rng.permutation(N))
    if name == "dup":
        ids = rng.integers(0, N, size=300)
        ids[10:20] = ids[0]; ids[299] = N - 1; ids[298] = 0
        return torch.from_numpy(ids)
    if name == "whole":
        return torch.arange(N)
    assert name == "none"
    return torch.zeros(0, dtype=torch.int64)


def _pre_rows(D, C, P):
    """45 rows (row0 % 32 = 13) that a destination holds from add() before the view rows arrive."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((45, D)).astype(np.float32)
    return x, gi.labels_from_masks(45, C, 64, seed=3)


def _build(regime, src, ids, D, metric, C, P, on_device):
    ids_in = ids.cuda() if on_device else ids
    if regime == "select":
        return src.select_rows(ids_in), None
    dst = HipFlatIndex(D, metric, 0)
    if regime == "two_calls":           # 37 + the rest: the second call starts at row0 % 32 = 5 and, beyond 256 rows, grows the capacity
        dst.add_from(src, ids_in[:37]); dst.add_from(src, ids_in[37:])
        return dst, None
    assert regime == "after_add"
    x, lab = _pre_rows(D, C, P)
    if P:
        dst.set_label_denominator(P)
    dst.add(torch.from_numpy(x).cuda(), normalize=False)
    dst.add_labels(torch.from_numpy(lab).cuda()); dst.set_num_classes(C)
    pre = {"rows": dst.reconstruct(torch.arange(45, device="cuda")), "norms": dst.copy_norms(),
           "lab": dst.gather_labels(torch.arange(45, device="cuda")), "counts": dst.copy_label_counts() if P else None}
    dst.add_from(src, ids_in)
    return dst, pre


@pytest.mark.parametrize("regime", ["select", "two_calls", "after_add"])
@pytest.mark.parametrize("D,variant", sorted(SOURCES))
def test_view_holds_the_selected_rows_bit_for_bit(cuda_device, D, variant, regime):
    src, ref, metric, C, P = _source(D, variant)
    for si, name in enumerate(("prefix", "perm", "dup", "whole", "none")):
        ids = _selection(name)
        view, pre = _build(regime, src, ids, D, metric, C, P, on_device=(si + variant) % 2 == 0)
        what = f"D={D} variant={variant} {regime} {name}"
        n_pre = 0 if pre is None else 45
        assert view.ntotal == n_pre + ids.numel(), what
        if view.ntotal == 0:
            view.close()
            continue
        idc = ids.cuda()
        want = {key: (ref[key][idc] if pre is None else torch.cat([pre[key], ref[key][idc]])) for key in ("rows", "norms", "lab")}
        all_ids = torch.arange(view.ntotal, device="cuda")
        assert torch.equal(_i32(view.reconstruct(all_ids)), _i32(want["rows"])), what
        assert torch.equal(_i32(view.copy_norms()), _i32(want["norms"])), what
        if ids.numel() == 0:            # (no rows arrived: the label table is whatever the destination had)
            view.close()
            continue
        assert view.label_denominator == P and view.num_classes == C, what
        assert torch.equal(_i32(view.gather_labels(all_ids)), _i32(want["lab"])), what
        if P:
            wc = ref["counts"][idc] if pre is None else torch.cat([pre["counts"], ref["counts"][idc]])
            got = view.copy_label_counts()
            assert got.shape == (view.ntotal, C) and torch.equal(got.cpu(), wc.cpu()), what
        view.close()
    assert src.ntotal == N and torch.equal(_i32(src.copy_norms()), _i32(ref["norms"]))        # the source is untouched


def _oracle_equal(got, q, rows, k, metric, what):
    ridx, rdist = oracle.knn_chain_f32(q, rows, k, METRIC_NAME[metric])
    assert np.array_equal(got[0].cpu().numpy(), ridx), f"{what}: ids differ from the oracle's on the selected rows"
    assert np.array_equal(got[1].cpu().numpy().view(np.uint32), rdist.view(np.uint32)), f"{what}: distance bits differ"
    return ridx


@pytest.mark.parametrize("D,variant", [(20, 0), (20, 1), (384, 1), (384, 2)])
def test_view_searches_like_an_index_of_those_rows(cuda_device, D, variant):
    """ids and distance bits of the oracle on src.reconstruct(ids), k = 30 and k = 300 (the big-k path); label_hat bits of an index built the
    staged way (reconstruct + add + gather_labels + add_labels); padding: nothing is found beyond the view's rows."""
    src, ref, metric, C, P = _source(D, variant)
    q = gi.vit_like_queries(NQ, D, seed=21)
    qc = torch.from_numpy(q).cuda()
    for name, regime in (("prefix", "select"), ("perm", "two_calls"), ("dup", "select"), ("prefix", "after_add")):
        ids = _selection(name)
        view, pre = _build(regime, src, ids, D, metric, C, P, on_device=True)
        rows = ref["rows"][ids.cuda()] if pre is None else torch.cat([pre["rows"], ref["rows"][ids.cuda()]])
        rows_np = rows.cpu().numpy()
        staged = HipFlatIndex(D, metric, 0)
        if P:
            staged.set_label_denominator(P)
        idc = ids.cuda()
        if pre is not None:
            staged.add(pre["rows"], normalize=False); staged.add_labels(pre["lab"])
        staged.add(src.reconstruct(idc), normalize=False); staged.add_labels(src.gather_labels(idc)); staged.set_num_classes(C)
        n_valid = int((~np.isnan(rows_np).any(axis=1)).sum())
        for k in (30, 300):
            what = f"D={D} variant={variant} {regime} {name} k={k}"
            got = view.search(qc, k)
            ridx = _oracle_equal(got, q, rows_np, k, metric, what)
            assert int(got[0].max()) < view.ntotal, what
            if k > n_valid:             # fewer rows than k: id -1 past them, never a padding row
                assert (ridx[:, n_valid:] == -1).all() and (got[0][:, n_valid:] == -1).all() and (got[0][:, :n_valid] >= 0).all(), what
            lh = k5(view, "search_aggregate", k)(qc, k)
            lh_staged = k5(staged, "search_aggregate", k)(qc, k)
            assert torch.equal(_i32(lh), _i32(lh_staged)), f"{what}: label_hat differs from the staged index's"
        view.close(); staged.close()


def test_the_screen_runs_on_a_view(cuda_device):
    """8,192 x 64 rows selected from 20,000: the fp16 copy (plain, then centred) is made lazily from the view's own tiles; fp32 bits."""
    D, M, n, k = 64, 20_000, 8192, 30
    bank = gi.unit_bank(M, D, seed=31)
    q = gi.vit_like_queries(256, D, seed=32)
    src = HipFlatIndex(D, 0, 0)
    src.add(torch.from_numpy(bank).cuda())
    ids = torch.from_numpy(np.sort(np.random.default_rng(33).permutation(M)[:n]))
    view = src.select_rows(ids.cuda())
    assert view.ntotal == n
    qc = torch.from_numpy(q).cuda()
    view.set_fp16(0)
    want = view.search(qc, k)
    assert view.last_search_path()["path"] == "fp32"
    _oracle_equal(want, q, bank[ids.numpy()], k, 0, "fp32 kernel on the view")
    for centre in (False, True):
        view.set_fp16(1)
        if centre:
            view.set_fp16_centre(True)
        got = view.search(qc, k)
        path = view.last_search_path()
        assert path["path"] in ("fp16_chain", "fp16_wide") and path["reason"] == "explicit_fp16", path      # the candidate pass ran
        assert torch.equal(got[0], want[0]) and torch.equal(_i32(got[1]), _i32(want[1])), f"centre={centre}: differs from the fp32 kernel's answer"
    view.close(); src.close()


def test_bmax_follows_add_from(cuda_device):
    """The certificate's bound takes the largest row norm of the bank.  500 small-norm rows are add()ed first, then an adversarial bank of
    8 x that norm arrives through add_from: with a stale bmax the bound would be eight times too small for those rows and a decoy would be
    returned in a hidden neighbour's place."""
    D, k, kc, gaps = 64, 30, 64, (0.5, 0.7, 0.8, 0.9, 0.95)
    W = fw.rounding_world(D, k, kc, 10, 300, gaps, seed=91, n_background=2500, n_queries_background=54, bank_scale=8.0)
    G = W["n_groups"]
    m = fw.screen_model(W["queries"][:G], W["bank"], k, kc, 0)
    assert int((~m["contained"]).sum()) == G          # every planted query has a true neighbour outside the fp16 candidates
    norm = float(np.sqrt((W["bank"][W["hidden_ids"][0][0]].astype(np.float64) ** 2).sum())) / 8.0
    filler = np.random.default_rng(92).standard_normal((500, D)).astype(np.float32)
    filler *= np.float32(norm) / np.linalg.norm(filler, axis=1, keepdims=True)
    src = HipFlatIndex(D, 0, 0)
    src.add(torch.from_numpy(W["bank"]).cuda())
    both = np.concatenate([filler, W["bank"]])
    q = torch.from_numpy(W["queries"]).cuda()
    for screen in (0, 1):
        dst = HipFlatIndex(D, 0, 0)
        dst.set_fp16(screen)
        dst.add(torch.from_numpy(filler).cuda())
        if screen:
            dst.search(q, k)           # the fp16 copy exists, and bmax is the filler's, before the big rows arrive
        dst.add_from(src, torch.arange(W["bank"].shape[0], device="cuda"))
        got = dst.search(q, k)
        assert dst.last_search_path()["path"] == ("fp16_chain" if screen else "fp32")
        _oracle_equal((got[0][:G], got[1][:G]), W["queries"][:G], both, k, 0, f"set_fp16({screen})")
        if screen:
            assert torch.equal(got[0], want[0]) and torch.equal(_i32(got[1]), _i32(want[1]))
            assert dst.last_fp16_escalated() >= G
        else:
            want = got
        ids = got[0].cpu().numpy()
        for i, hid in enumerate(W["hidden_ids"]):
            assert np.isin(np.asarray(hid) + 500, ids[i]).all(), f"set_fp16({screen}): query {i} lost its hidden neighbour"
        dst.close()
    src.close()


def test_errors_leave_the_destination_unchanged(cuda_device):
    D, C, P = 20, 21, 64
    src, ref, metric, _, _ = _source(D, 0)
    x, lab = _pre_rows(D, C, P)
    dst = HipFlatIndex(D, 0, 0)
    dst.set_label_denominator(P)
    dst.add(torch.from_numpy(x).cuda()); dst.add_labels(torch.from_numpy(lab).cuda()); dst.set_num_classes(C)
    q = torch.from_numpy(gi.vit_like_queries(NQ, D, seed=41)).cuda()
    before = dst.search_aggregate(q, 10, want_neighbours=True)
    rows_before = dst.reconstruct(torch.arange(45, device="cuda"))

    def other(d=D, metric=0, c=C, p=P, rows=100, label_rows=100):
        o = HipFlatIndex(d, metric, 0)
        if p:
            o.set_label_denominator(p)
        o.add(torch.from_numpy(_rows(d, 1)[:rows]).cuda())
        if label_rows:
            o.add_labels(torch.from_numpy(gi.labels_from_masks(label_rows, c, p or 64, seed=2)).cuda()); o.set_num_classes(c)
        return o

    bad = [(src, torch.tensor([3, N, 5])), (src, torch.tensor([3, N, 5]).cuda()), (src, torch.tensor([-1])), (src, torch.tensor([0, 1, -1]).cuda()),
           (dst, torch.tensor([0])),                                  # src is dst
           (other(d=24), torch.tensor([0])), (other(metric=1), torch.tensor([0])),
           (other(p=16), torch.tensor([0])),                          # another label denominator
           (other(c=20), torch.tensor([0])),                          # another class count
           (other(label_rows=60), torch.tensor([10, 70]))]            # label rows end before the id
    for s, ids in bad:
        with pytest.raises(ValueError):
            dst.add_from(s, ids)
        assert dst.ntotal == 45
    with pytest.raises(ValueError):
        src.select_rows(torch.tensor([N]))
    with pytest.raises(ValueError):
        src.select_rows(torch.tensor([5, -1]).cuda())
    multi = HipMultiIndex(D, 0, [0, 0], shard=True)
    with pytest.raises(ValueError, match="single-index"):
        multi.select_rows(torch.tensor([0]))
    with pytest.raises(ValueError, match="single-index"):
        dst.add_from(multi, torch.tensor([0]))
    multi.close()
    after = dst.search_aggregate(q, 10, want_neighbours=True)
    assert dst.ntotal == 45 and dst.copy_label_counts().shape[0] == 45
    assert torch.equal(_i32(dst.reconstruct(torch.arange(45, device="cuda"))), _i32(rows_before))
    for a, b in zip(before, after):
        assert torch.equal(_i32(a) if a.dtype == torch.float32 else a.cpu(), _i32(b) if b.dtype == torch.float32 else b.cpu())
    # ... and a good call still works afterwards
    dst.add_from(src, torch.tensor([1, 2, 3]))
    assert dst.ntotal == 48 and torch.equal(_i32(dst.reconstruct(torch.arange(45, 48, device="cuda"))), _i32(ref["rows"][1:4]))
    for s, _ in bad[5:]:
        s.close()
    dst.close()
