"""`NearestNeighborSearchHIP`: the exact flat kNN backend on MI355X.

Drop-in for the reference's `NearestNeighborSearchFaiss` (hbird/nn/search_faiss.py:6-90): same
constructor keywords, same `find_nearest_neighbors(q, k=None) -> (indices, distances)` contract, same
exception types -- but the arithmetic is libhbird_hip.so's fused MFMA top-k kernel instead of
faiss-gpu.  One process drives ONE GPU; with torch.distributed initialised, `idx_shard=True` row-shards
the bank over the ranks (faiss.IndexShards, search_faiss.py:53-63) and merges the per-rank top-k after an
RCCL all-gather, `idx_shard=False` keeps a full replica per rank (faiss.IndexReplicas, 65-74).
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from typing import Optional, Tuple

import numpy as np
import torch

from hbird_mi import _lib
from hbird_mi.nn.search_base import NearestNeighborSearchBase

_METRICS = {"dot_product": 0, "l2": 1, "euclidean": 1}
MAX_K = 256          # of the LDS-resident entries (hb_index_search_aggregate / _aggregate / _aggregate_partial, hb_merge_topk): HB_MAX_K_AGGREGATE
MAX_K_SEARCH = 2048  # of every search, aggregation and merge -- faiss-gpu's own limit (the reference forwards any k, search_faiss.py:84-85): HB_MAX_K
_MERGE_LDS = 60000   # bytes of LDS the old merge kernel stages parts * k candidates in (hb_launch_merge_parts)


def k5(index, name: str, k: int):
    """THE routing between the two K5 families: `name` ("search_aggregate" / "aggregate" / "aggregate_partial") of a HipFlatIndex for this
    k -- the LDS-resident entry up to 256 (launch for launch what it always was), its `_bigk` twin beyond (hb_bigk_*).  A HipMultiIndex
    has no twins: its methods come back as they are and route through here on its aggregation handle."""
    return getattr(index, name + "_bigk" if k > MAX_K and hasattr(index, name + "_bigk") else name)


def check_k(k: int, what: str = "k"):
    """1 <= k <= 2048 or the ValueError faiss-gpu raises for its k-select limit."""
    if not 1 <= k <= MAX_K_SEARCH:
        raise ValueError(f"{what}={k} outside the supported range [1, {MAX_K_SEARCH}] (faiss-gpu's own limit)")


GridPlan = namedtuple("GridPlan", "ks betas configs launches")


def grid_plan(ks, betas, max_configs: int = _lib.GRID_MAX_CONFIGS) -> GridPlan:
    """The grid of an aggregation over (k, beta) configurations, validated, ordered and cut into launches.  Pure Python.

    `ks`, `betas`: a number or an iterable of numbers each; duplicates are dropped, both are sorted ascending.  ValueError for an empty list, a k
    that is not an integer in [1, 2048] and a beta that is not a finite positive number.
    -> GridPlan(ks, betas, configs, launches):
       configs   THE configuration order: [(k, beta) for k in ks for beta in betas] -- row i of every [nk * nb, nq, C] result is configs[i]
       launches  [(ks_part, betas_part, rows)]: rectangles of at most `max_configs` configurations (what one hb_index_aggregate_grid call
                 takes: ascending ks_part x betas_part over the same neighbour list), rows[ik * len(betas_part) + ib] = the row of that
                 configuration in `configs`.  Whole k rows go together, as many as fit; a grid with more than `max_configs` betas is cut along
                 the betas as well.  Concatenating the launches' rows in launch order gives 0 .. len(configs) - 1 when the betas are not cut."""
    def as_list(v, what):
        if isinstance(v, (str, bytes)):
            raise ValueError(f"{what} must be a number or a list of numbers, got {v!r}")
        try:
            out = list(v)
        except TypeError:
            out = [v]
        if not out:
            raise ValueError(f"{what} is empty: the grid needs at least one value")
        return out

    k_out = []
    for k in as_list(ks, "ks"):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"k={k!r} is not an integer")
        check_k(int(k))
        k_out.append(int(k))
    b_out = []
    for b in as_list(betas, "betas"):
        if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)):
            raise ValueError(f"beta={b!r} is not a number")
        b = float(b)
        if not (math.isfinite(b) and b > 0.0):
            raise ValueError(f"beta={b!r}: every beta must be finite and positive")
        b_out.append(b)
    k_out, b_out = sorted(set(k_out)), sorted(set(b_out))
    nb = len(b_out)
    configs = [(k, b) for k in k_out for b in b_out]
    b_step = min(nb, max_configs)
    k_step = max(1, max_configs // b_step)
    launches = []
    for k0 in range(0, len(k_out), k_step):
        kp = k_out[k0:k0 + k_step]
        for b0 in range(0, nb, b_step):
            bp = b_out[b0:b0 + b_step]
            launches.append((tuple(kp), tuple(bp), [(k0 + i) * nb + b0 + j for i in range(len(kp)) for j in range(len(bp))]))
    return GridPlan(tuple(k_out), tuple(b_out), configs, launches)


def exclude_plan(k: int, gmax: int):
    """The rungs (list lengths) of an excluding search for k and the largest group's size -- hb_exclude_plan_replay, the rule the
    engine itself runs (csrc/hbird_calibrate.cpp); no GPU.  ValueError when k + gmax exceeds 2048."""
    rungs = (ctypes.c_int * 2)()
    n = _lib.lib().hb_exclude_plan_replay(int(k), int(gmax), rungs, 2)
    if n < 0:
        raise ValueError(_lib.last_error())
    return [int(rungs[i]) for i in range(n)]


def _new(like, shape, dtype):
    """An uninitialised output beside `like`: a tensor on its device for a CUDA tensor, a numpy array otherwise (dtype: a torch dtype)."""
    if isinstance(like, torch.Tensor) and like.is_cuda:
        return torch.empty(shape, dtype=dtype, device=like.device)
    return np.empty(shape, dtype=np.int64 if dtype == torch.int64 else np.float32)


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return ctypes.c_void_p(t.data_ptr())
    return ctypes.c_void_p(t.ctypes.data)


class HipFlatIndex:
    """Thin owner of one `hb_index_t*` (one GPU)."""

    def __init__(self, d: int, metric: int, device: int):
        self._h = ctypes.c_void_p()
        self.d, self.metric, self.device = int(d), int(metric), int(device)
        self._fp16_centre = False
        L = _lib.lib()
        rc = L.hb_index_create(self.d, self.metric, self.device, ctypes.byref(self._h))
        if rc != 0:
            msg = _lib.last_error()
            # same exception types as search_faiss.py:16 (no GPU) and :25 (bad GPU id)
            if "no GPUs" in msg:
                raise RuntimeError("No GPUs available for the HIP index.")
            raise ValueError(msg)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().hb_index_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ntotal(self) -> int:
        return int(_lib.lib().hb_index_ntotal(self._h))

    def use_current_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().hb_index_set_stream(self._h, ctypes.c_void_p(s)))

    def reserve(self, n: int):
        _lib.check(_lib.lib().hb_index_reserve(self._h, int(n)))

    def reset(self):
        _lib.check(_lib.lib().hb_index_reset(self._h))
        self._groups, self._n_groups = None, 0      # (hb_index_reset clears the row-group table)

    def add(self, x, normalize: bool = False):
        """x: float32 [n, d], numpy / CPU tensor (host path) or CUDA tensor on this GPU (device path)."""
        on_dev, x = self._as_f32(x)
        assert x.shape[1] == self.d, f"expected [n, {self.d}] rows, got {tuple(x.shape)}"
        _lib.check(_lib.lib().hb_index_add(self._h, _ptr(x), x.shape[0], int(on_dev), int(bool(normalize))))

    def add_labels(self, lab):
        on_dev, lab = self._as_f32(lab)
        _lib.check(_lib.lib().hb_index_add_labels(self._h, _ptr(lab), lab.shape[0], lab.shape[1], int(on_dev)))

    def _as_f32(self, x):
        if isinstance(x, torch.Tensor):
            x = x.detach()
            if x.dtype != torch.float32:
                x = x.float()
            x = x.contiguous()
            if x.is_cuda:
                assert x.device.index == self.device, "tensor lives on another GPU than the index"
                return True, x
            return False, x
        return False, np.ascontiguousarray(x, dtype=np.float32)

    def search_scores(self, q, k: int, id_base: int = 0, out=None):
        """Like `search`, but the second output holds the ORDERING scores (larger is better; L2: q.b - |b|^2/2), the
        input of a cross-shard merge (hb_index_set_score_output); convert with `distances_from_scores`."""
        lib = _lib.lib()
        _lib.check(lib.hb_index_set_score_output(self._h, 1))
        try:
            return self.search(q, k, id_base, out=out)
        finally:
            _lib.check(lib.hb_index_set_score_output(self._h, 0))

    def distances_from_scores(self, q: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
        """Merged ordering scores [nq,k] (CUDA) -> the metric's distances, in place (no-op for the inner product)."""
        assert q.is_cuda and scores.is_cuda and scores.is_contiguous() and scores.dtype == torch.float32
        q = q.contiguous().float()
        _lib.check(_lib.lib().hb_index_distances_from_scores(self._h, _ptr(q), q.shape[0], scores.shape[1], _ptr(scores)))
        return scores

    def search(self, q, k: int, id_base: int = 0, out=None):
        """-> (idx int64 [nq,k], dist float32 [nq,k]); torch CUDA tensors for CUDA queries, numpy otherwise.
        out = (idx, dist): contiguous CUDA tensors to write into (e.g. the views of a dist.PackedTopK)."""
        on_dev, q = self._as_f32(q)
        nq = q.shape[0]
        if out is not None:
            idx, dist = out
            assert on_dev and idx.is_cuda and dist.is_cuda and idx.is_contiguous() and dist.is_contiguous()
            assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and tuple(idx.shape) == tuple(dist.shape) == (nq, k)
        else:
            idx, dist = _new(q, (nq, k), torch.int64), _new(q, (nq, k), torch.float32)
        _lib.check(_lib.lib().hb_index_search(self._h, _ptr(q), nq, int(k), int(id_base), _ptr(idx), _ptr(dist),
                                               int(on_dev)))
        return idx, dist

    # K5 on one GPU: each method and its `_bigk` twin (k beyond 256, up to 2048: same arguments, same results, for k <= 256 the same bits)
    # are one implementation that takes the C entry; `k5()` above routes between the twins.
    def _search_aggregate(self, entry, q, k, beta, id_base, want_neighbours):
        on_dev, q = self._as_f32(q)
        nq = q.shape[0]
        out = _new(q, (nq, self.num_classes), torch.float32)
        idx = _new(q, (nq, k), torch.int64) if want_neighbours else None
        dist = _new(q, (nq, k), torch.float32) if want_neighbours else None
        _lib.check(entry(self._h, _ptr(q), nq, int(k), int(id_base), float(beta), _ptr(out), _ptr(idx), _ptr(dist), int(on_dev)))
        return (out, idx, dist) if want_neighbours else out

    def _aggregate(self, entry, q, idx, dist, beta, id_base):
        assert q.is_cuda and idx.is_cuda and dist.is_cuda
        q = q.contiguous().float(); idx = idx.contiguous(); dist = dist.contiguous()
        out = _new(q, (q.shape[0], self.num_classes), torch.float32)
        _lib.check(entry(self._h, _ptr(q), q.shape[0], _ptr(idx), _ptr(dist), idx.shape[1], int(id_base), float(beta), _ptr(out), 1))
        return out

    def _aggregate_partial(self, entry, q, idx, dist, norms_all, beta, id_base):
        assert q.is_cuda and idx.is_cuda and dist.is_cuda and norms_all.is_cuda
        q = q.contiguous().float(); idx = idx.contiguous(); dist = dist.contiguous(); norms_all = norms_all.contiguous().float()
        if self.ntotal == 0:                 # an empty shard owns no neighbour
            return torch.zeros((q.shape[0], self.num_classes), dtype=torch.float32, device=q.device)
        out = _new(q, (q.shape[0], self.num_classes), torch.float32)
        _lib.check(entry(self._h, _ptr(q), q.shape[0], _ptr(idx), _ptr(dist), idx.shape[1], int(id_base), float(beta), _ptr(norms_all),
                         norms_all.shape[0], _ptr(out)))
        return out

    def search_aggregate(self, q, k: int, beta: float = 0.02, id_base: int = 0, want_neighbours: bool = False):
        return self._search_aggregate(_lib.lib().hb_index_search_aggregate, q, k, beta, id_base, want_neighbours)

    def aggregate(self, q, idx, dist, beta: float = 0.02, id_base: int = 0):
        """Label aggregation on given neighbours (CUDA tensors)."""
        return self._aggregate(_lib.lib().hb_index_aggregate, q, idx, dist, beta, id_base)

    def aggregate_partial(self, q, idx, dist, norms_all: torch.Tensor, beta: float = 0.02, id_base: int = 0):
        """Label-sharded aggregation: the softmax-weighted label sum over the neighbours THIS index owns (global ids id_base ..),
        with the weights of the full neighbour list (norms_all: the bank-row norms of all rows, global ids from 0).  The sum
        over the shards (an all-reduce) is label_hat."""
        return self._aggregate_partial(_lib.lib().hb_index_aggregate_partial, q, idx, dist, norms_all, beta, id_base)

    def search_aggregate_bigk(self, q, k: int, beta: float = 0.02, id_base: int = 0, want_neighbours: bool = False):
        return self._search_aggregate(_lib.lib().hb_bigk_search_aggregate, q, k, beta, id_base, want_neighbours)

    def aggregate_bigk(self, q, idx, dist, beta: float = 0.02, id_base: int = 0):
        return self._aggregate(_lib.lib().hb_bigk_aggregate, q, idx, dist, beta, id_base)

    def aggregate_partial_bigk(self, q, idx, dist, norms_all: torch.Tensor, beta: float = 0.02, id_base: int = 0):
        return self._aggregate_partial(_lib.lib().hb_bigk_aggregate_partial, q, idx, dist, norms_all, beta, id_base)

    # evaluation grids (hb_index_aggregate_grid / hb_index_search_aggregate_grid, csrc/hbird_grid.hip): every (k, beta) of a grid from ONE list
    # per query -- the best k of a query are the first k entries of its best k_max, bit for bit, and beta only enters after the search
    def _grid_call(self, q, idx, dist, kp, bp, id_base, out):
        """One launch: configurations kp x bp (at most 16) on the lists idx / dist [nq, k_list], into out [len(kp) * len(bp), nq, C]."""
        ka, ba = (ctypes.c_int * len(kp))(*kp), (ctypes.c_float * len(bp))(*bp)
        _lib.check(_lib.lib().hb_index_aggregate_grid(self._h, _ptr(q), q.shape[0], _ptr(idx), _ptr(dist), idx.shape[1], int(id_base),
                                                       ka, len(kp), ba, len(bp), _ptr(out), 1), ValueError)
        return out

    def aggregate_grid(self, q, idx, dist, ks, betas, id_base: int = 0):
        """Label aggregation of every configuration of `grid_plan(ks, betas)` on given neighbours (CUDA tensors; idx / dist [nq, k_list] with
        k_list >= max(ks)): -> [nk * nb, nq, C], row i the result of `aggregate` on the first k positions of the lists for (k, beta) =
        grid_plan(ks, betas).configs[i] -- its bits.  Up to k = 256 the configurations go 16 to a launch on the lists as they are; a k beyond 256
        is served by `aggregate_bigk` on a contiguous prefix copy.  ValueError for a bad grid and for lists shorter than the largest k."""
        plan = grid_plan(ks, betas)
        assert q.is_cuda and idx.is_cuda and dist.is_cuda
        q = q.contiguous().float(); idx = idx.contiguous(); dist = dist.contiguous()
        k_list = idx.shape[1]
        if plan.ks[-1] > k_list:
            raise ValueError(f"aggregate_grid: the largest k ({plan.ks[-1]}) exceeds k_list ({k_list}), the length of the given lists")
        nq, nb = q.shape[0], len(plan.betas)
        out = torch.empty((len(plan.configs), nq, self.num_classes), dtype=torch.float32, device=q.device)
        small = [k for k in plan.ks if k <= MAX_K]
        if small:
            if k_list > MAX_K:            # the list-resident entry takes strides up to 256: the prefix every small k lives in
                idx_s, dist_s = idx[:, :small[-1]].contiguous(), dist[:, :small[-1]].contiguous()
            else:
                idx_s, dist_s = idx, dist
            launches = grid_plan(small, plan.betas).launches
            for kp, bp, rows in launches:
                whole = len(launches) == 1 and len(small) == len(plan.ks)
                part = out if whole else torch.empty((len(rows), nq, out.shape[2]), dtype=torch.float32, device=q.device)
                self._grid_call(q, idx_s, dist_s, kp, bp, id_base, part)
                if not whole:
                    out[torch.as_tensor(rows, device=q.device)] = part       # (the rows of the small ks come first in the whole grid too)
        for ik, k in enumerate(plan.ks):
            if k > MAX_K:
                idx_k, dist_k = idx[:, :k].contiguous(), dist[:, :k].contiguous()
                for ib, beta in enumerate(plan.betas):
                    out[ik * nb + ib] = self.aggregate_bigk(q, idx_k, dist_k, beta=beta, id_base=id_base)
        return out

    def search_aggregate_grid(self, q, ks, betas, id_base: int = 0, want_neighbours: bool = False):
        """ONE search at max(ks), then `aggregate_grid`: -> [nk * nb, nq, C] (and the [nq, max(ks)] neighbour lists); numpy in, numpy out.
        A grid of one launch with max(ks) <= 256 is the fused entry hb_index_search_aggregate_grid."""
        plan = grid_plan(ks, betas)
        on_dev, q = self._as_f32(q)
        nq, kmax, c = q.shape[0], plan.ks[-1], self.num_classes
        if len(plan.launches) == 1 and kmax <= MAX_K:
            out = _new(q, (len(plan.configs), nq, c), torch.float32)
            idx = _new(q, (nq, kmax), torch.int64) if want_neighbours else None
            dist = _new(q, (nq, kmax), torch.float32) if want_neighbours else None
            ka, ba = (ctypes.c_int * len(plan.ks))(*plan.ks), (ctypes.c_float * len(plan.betas))(*plan.betas)
            _lib.check(_lib.lib().hb_index_search_aggregate_grid(self._h, _ptr(q), nq, int(id_base), ka, len(plan.ks), ba, len(plan.betas),
                                                                  _ptr(out), _ptr(idx), _ptr(dist), int(on_dev)), ValueError)
            return (out, idx, dist) if want_neighbours else out
        qd = q if on_dev else torch.from_numpy(q).cuda(self.device)
        idx, dist = self.search(qd, kmax, id_base)
        out = self.aggregate_grid(qd, idx, dist, plan.ks, plan.betas, id_base=id_base)
        if not on_dev:
            out, idx, dist = out.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
        return (out, idx, dist) if want_neighbours else out

    # searches that exclude one row group per query (hb_index_set_row_groups / hb_index_search_excluding, csrc/hbird_exclude.hip): leave-one-
    # image-out evaluation -- the best k rows outside a group are the first k non-excluded entries of the best k + gmax, bit for bit
    def set_row_groups(self, groups, n_groups: Optional[int] = None):
        """The row-group table: groups[ntotal] integers, a value in [0, n_groups) names the row's group, -1 = in no group (never excluded);
        None clears it.  n_groups defaults to max(groups) + 1.  Keeps a device copy (`row_groups`).  ValueError for a value outside the range."""
        if groups is None:
            _lib.check(_lib.lib().hb_index_set_row_groups(self._h, None, 0, 0, 0))
            self._groups, self._n_groups = None, 0
            return
        g = torch.as_tensor(groups)
        if g.numel() and (g.dtype.is_floating_point or g.dtype.is_complex or g.dtype == torch.bool):
            raise ValueError(f"row groups must be integers, got {g.dtype}")
        g = g.detach().reshape(-1).to(device=torch.device("cuda", self.device), dtype=torch.int32).contiguous()
        if n_groups is None:
            n_groups = int(g.max().item()) + 1 if g.numel() else 0
        _lib.check(_lib.lib().hb_index_set_row_groups(self._h, _ptr(g), g.numel(), int(n_groups), 1), ValueError)
        self._groups, self._n_groups = (g if g.numel() else None), (int(n_groups) if g.numel() else 0)

    @property
    def row_groups(self) -> Optional[torch.Tensor]:
        """The device copy of the row-group table (int32 [n]) or None."""
        return getattr(self, "_groups", None)

    def _hand_groups(self, src: "HipFlatIndex", ids, appended: bool):
        """After rows `ids` of `src` arrived here: the view of src's group table, groups[ids], through set_row_groups."""
        sg = src.row_groups
        if sg is None or ids.numel() == 0:
            return
        if sg.numel() != src.ntotal:      # rows were added since set_row_groups: the table is behind the rows (an id beyond it must not index it)
            return
        part = sg[ids.to(sg.device)]
        mine = self.row_groups
        if appended and mine is not None and mine.numel() + part.numel() == self.ntotal:
            part = torch.cat([mine, part])
        if part.numel() == self.ntotal:
            self.set_row_groups(part, max(src._n_groups, getattr(self, "_n_groups", 0)))

    def search_excluding(self, q, k: int, qgroups, id_base: int = 0):
        """-> (idx int64 [nq,k], dist float32 [nq,k]) as `search`, over the rows whose group differs from qgroups[i] (-1: exclude nothing):
        original row ids, and the bits of `search` on `select_rows(the allowed rows, ascending)`.  ValueError for a missing or short table, a
        group id outside the range and k + (largest group) > 2048 -- raised before anything is searched."""
        on_dev, q = self._as_f32(q)
        nq = q.shape[0]
        qg = torch.as_tensor(qgroups).detach().reshape(-1)
        if qg.numel() != nq:
            raise ValueError(f"search_excluding: {qg.numel()} query groups for {nq} queries")
        if qg.numel() and (qg.dtype.is_floating_point or qg.dtype == torch.bool):
            raise ValueError(f"query groups must be integers, got {qg.dtype}")
        qg = qg.to(device=q.device if on_dev else "cpu", dtype=torch.int32).contiguous()
        idx, dist = _new(q, (nq, k), torch.int64), _new(q, (nq, k), torch.float32)
        _lib.check(_lib.lib().hb_index_search_excluding(self._h, _ptr(q), nq, int(k), int(id_base), _ptr(qg), _ptr(idx), _ptr(dist), int(on_dev)),
                   ValueError)
        return idx, dist

    def last_exclusion(self) -> dict:
        """Of the last excluding search: rungs run, queries sent to rung 1, the list length of the last rung run, the largest group's size."""
        out = (ctypes.c_int64 * 4)()
        _lib.check(_lib.lib().hb_index_last_exclusion(self._h, out))
        return {"rungs": int(out[0]), "rung1_queries": int(out[1]), "kf": int(out[2]), "gmax": int(out[3])}

    def set_exclusion_screen(self, on: bool = True):
        """Excluding searches on the certified fp16 screen (hb_index_set_exclude_screen, include/hbird_hip_exclude_screen.h): where k <= 128,
        k + (largest group) > 128 and the index's own choice for a plain search at k is the candidate pass, the re-rank drops the query's group
        among the candidates of a search at k -- the cost of a plain search -- and only what fails both certificates goes through the rungs.
        Same ids and distance bits either way.  Off by default."""
        _lib.check(_lib.lib().hb_index_set_exclude_screen(self._h, int(bool(on))))

    def last_exclusion_screen(self) -> dict:
        """Of the last excluding search (hb_index_last_exclusion_screen): served by the screen (0 / 1), the reason when not ("off", "k", "need",
        "path", "empty"), kc of level 0, queries certified at level 0, sent to and certified at the second pass, sent to the rungs, centred."""
        out = (ctypes.c_int64 * 8)()
        _lib.check(_lib.lib().hb_index_last_exclusion_screen(self._h, out))
        return {"served": int(out[0]), "reason": _lib.EXCL_SCREEN_REASONS.get(int(out[1]), str(int(out[1]))), "kc": int(out[2]),
                "certified0": int(out[3]), "second_pass": int(out[4]), "certified1": int(out[5]), "rung_queries": int(out[6]), "centred": int(out[7])}

    def exclude_rerank(self, q, cand_rows, pass_scores, qgroups, k: int, id_base: int = 0):
        """The excluding re-rank kernel alone on given candidate lists (hb_index_exclude_rerank): device tensors q [nq, d] float32, cand_rows
        [nq, kc] int64 and pass_scores [nq, kc] float32 as `last_screen` hands them out, qgroups [nq] int32.
        -> (idx [nq, k], dist [nq, k], certified [nq] uint8, kth [nq], floor [nq]).  ValueError where the entry refuses."""
        nq, kc = cand_rows.shape
        idx, dist = _new(q, (nq, k), torch.int64), _new(q, (nq, k), torch.float32)
        cert, kth, flo = _new(q, (nq,), torch.uint8), _new(q, (nq,), torch.float32), _new(q, (nq,), torch.float32)
        _lib.check(_lib.lib().hb_index_exclude_rerank(self._h, _ptr(q), nq, _ptr(cand_rows), _ptr(pass_scores), int(kc), _ptr(qgroups), int(k),
                                                      int(id_base), _ptr(idx), _ptr(dist), _ptr(cert), _ptr(kth), _ptr(flo)), ValueError)
        return idx, dist, cert, kth, flo

    def last_exclusion_seeds(self) -> dict:
        """What an excluding search that the screen served handed on besides `last_screen_seeds` (hb_index_last_exclusion_seeds): groups1 int32
        [n1], the second pass' query groups as gathered on the device (the order of queries1), and left int64 [n_left], the level-0 query numbers
        handed to the rungs, ascending.  Raises when the last search was not a served excluding one, or after reset / add / a capacity change."""
        lib = _lib.lib()
        info = (ctypes.c_int64 * 2)()
        _lib.check(lib.hb_index_last_exclusion_seeds(self._h, None, None, 0, 0, info))
        n1, n_left = int(info[0]), int(info[1])
        groups1, left = np.empty(n1, dtype=np.int32), np.empty(n_left, dtype=np.int64)
        _lib.check(lib.hb_index_last_exclusion_seeds(self._h, _ptr(groups1) if n1 else None, _ptr(left) if n_left else None, n1, n_left, info))
        return {"n1": n1, "n_left": n_left, "groups1": groups1, "left": left}

    def _excluding_lists(self, q, k, qgroups, id_base):
        on_dev, q = self._as_f32(q)
        qd = q if on_dev else torch.from_numpy(q).cuda(self.device)
        idx, dist = self.search_excluding(qd, k, torch.as_tensor(qgroups).to(qd.device), id_base)
        return on_dev, qd, idx, dist

    def search_aggregate_excluding(self, q, k: int, qgroups, beta: float = 0.02, id_base: int = 0, want_neighbours: bool = False):
        """`search_excluding`, then `aggregate` (beyond k = 256 its big-k form) on the lists: the bits of `search_aggregate` on the view of the
        allowed rows, given that the label rows of this index cover its rows."""
        on_dev, qd, idx, dist = self._excluding_lists(q, k, qgroups, id_base)
        out = k5(self, "aggregate", k)(qd, idx, dist, beta=beta, id_base=id_base)
        if not on_dev:
            out, idx, dist = out.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
        return (out, idx, dist) if want_neighbours else out

    def search_aggregate_grid_excluding(self, q, ks, betas, qgroups, id_base: int = 0, want_neighbours: bool = False):
        """ONE excluding search at max(ks), then `aggregate_grid` (the big-k prefix route included): -> [nk * nb, nq, C] as
        `search_aggregate_grid`, every configuration with the bits of the single `search_aggregate_excluding` call."""
        plan = grid_plan(ks, betas)
        on_dev, qd, idx, dist = self._excluding_lists(q, plan.ks[-1], qgroups, id_base)
        out = self.aggregate_grid(qd, idx, dist, plan.ks, plan.betas, id_base=id_base)
        if not on_dev:
            out, idx, dist = out.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
        return (out, idx, dist) if want_neighbours else out

    @property
    def num_classes(self) -> int:
        return int(self._c) if hasattr(self, "_c") else self._query_c()

    def _query_c(self):
        raise RuntimeError("labels were not added to this index")

    def set_num_classes(self, c: int):
        self._c = int(c)

    def reconstruct(self, ids, id_base: int = 0):
        on_dev = isinstance(ids, torch.Tensor) and ids.is_cuda
        ids = ids.contiguous().to(torch.int64) if on_dev else np.ascontiguousarray(np.asarray(ids), dtype=np.int64)
        n = ids.numel() if on_dev else ids.size
        out = _new(ids, (n, self.d), torch.float32)
        _lib.check(_lib.lib().hb_index_reconstruct(self._h, _ptr(ids), n, int(id_base), _ptr(out), int(on_dev)))
        return out

    def gather_labels(self, ids):
        on_dev = isinstance(ids, torch.Tensor) and ids.is_cuda
        c = self.num_classes
        ids = ids.contiguous().to(torch.int64) if on_dev else np.ascontiguousarray(np.asarray(ids), dtype=np.int64)
        n = ids.numel() if on_dev else ids.size
        out = _new(ids, (n, c), torch.float32)
        _lib.check(_lib.lib().hb_index_gather_labels(self._h, _ptr(ids), n, 0, _ptr(out), int(on_dev)))
        return out

    # sub-bank views (hb_index_add_from / hb_index_select_rows, csrc/hbird_select.hip): rows of one index gathered into another on the device
    def _ids64(self, ids):
        """ids -> (on_device, contiguous int64 tensor [n]); integer ids only (a float or bool array is refused, not truncated); a CUDA
        tensor must live on this index's GPU."""
        if not isinstance(ids, torch.Tensor):
            arr = np.asarray(ids)
            if arr.size and not np.issubdtype(arr.dtype, np.integer):
                raise ValueError(f"row ids must be integers, got {arr.dtype}")
            return False, torch.from_numpy(np.ascontiguousarray(arr.reshape(-1), dtype=np.int64))
        if ids.numel() and (ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool):
            raise ValueError(f"row ids must be integers, got {ids.dtype}")
        ids = ids.detach().reshape(-1).to(torch.int64).contiguous()
        if ids.is_cuda and ids.device.index != self.device:
            raise ValueError("ids live on another GPU than the index")
        return ids.is_cuda, ids

    def add_from(self, src: "HipFlatIndex", ids):
        """Append rows `ids` (host or device int64 tensor; any order, duplicates allowed) of `src` to this index, tile to tile: tiles, norms and
        the L2 row constants verbatim, label rows in their stored form when `src` holds them.  ValueError for an id outside `src`, for
        `src is self`, and for indexes that differ in width, metric, device, class count or label denominator -- the index is then unchanged."""
        if not isinstance(src, HipFlatIndex):
            raise ValueError("add_from: views are single-index (the source must be a HipFlatIndex)")
        on_dev, ids = self._ids64(ids)
        _lib.check(_lib.lib().hb_index_add_from(self._h, src._h, _ptr(ids), ids.numel(), int(on_dev)), ValueError)
        if hasattr(src, "_c") and ids.numel() and int(_lib.lib().hb_index_nlabels(src._h)) > 0:
            self._c = src._c           # label rows came along: the destination's class count is the source's (an emptied one adopted it)
        self._hand_groups(src, ids, appended=True)

    def select_rows(self, ids) -> "HipFlatIndex":
        """A NEW index holding rows `ids` of this one (hb_index_select_rows): 1 x its rows of memory, label rows included; its fp16 state,
        calibration and workspace are its own (a new index's).  ValueError for an id outside this index."""
        on_dev, ids = self._ids64(ids)
        view = HipFlatIndex.__new__(HipFlatIndex)
        view._h = ctypes.c_void_p()
        view.d, view.metric, view.device = self.d, self.metric, self.device
        view._fp16_centre = False
        _lib.check(_lib.lib().hb_index_select_rows(self._h, _ptr(ids), ids.numel(), int(on_dev), ctypes.byref(view._h)), ValueError)
        if hasattr(self, "_c"):
            view._c = self._c
        view._hand_groups(self, ids, appended=False)
        return view

    def copy_norms(self) -> torch.Tensor:
        """L2 norms of this shard's stored rows (CUDA tensor [ntotal])."""
        out = torch.empty((self.ntotal,), dtype=torch.float32, device=torch.device("cuda", self.device))
        if self.ntotal:
            _lib.check(_lib.lib().hb_index_copy_norms(self._h, _ptr(out), 1))
        return out

    def set_label_denominator(self, P: int):
        """Every label value is j / P (P = patch_size ** 2: one_hot(...).mean over a patch's P pixels, hbird_eval.py:319-320): the
        index then stores the uint16 counts j -- half the table -- and hands back the same fp32 values.  Before the first label row."""
        _lib.check(_lib.lib().hb_index_set_label_denominator(self._h, int(P)))

    def labels_to_fp32(self):
        """The stored counts back to fp32 rows, in place (hb_index_labels_to_fp32): a bank whose batches come in a second patch size."""
        _lib.check(_lib.lib().hb_index_labels_to_fp32(self._h))

    @property
    def label_denominator(self) -> int:
        P = ctypes.c_int(0)
        _lib.check(_lib.lib().hb_index_label_denominator(self._h, ctypes.byref(P)))
        return int(P.value)

    def copy_label_counts(self) -> torch.Tensor:
        """This shard's label rows as counts: int16 tensor [nlabels, C] holding the uint16 bit patterns (CUDA)."""
        n = int(_lib.lib().hb_index_nlabels(self._h))
        out = torch.empty((n, self.num_classes), dtype=torch.int16, device=torch.device("cuda", self.device))
        if n:
            _lib.check(_lib.lib().hb_index_copy_label_counts(self._h, _ptr(out), 1))
        return out

    def set_label_count_table(self, counts: torch.Tensor, norms: torch.Tensor, P: int, id_base: int = 0):
        """set_label_table for a table held as counts (int16 tensor of uint16 bit patterns, denominator P)."""
        counts = counts.contiguous(); norms = norms.contiguous().float()
        assert counts.is_cuda and norms.is_cuda and counts.dtype == torch.int16 and counts.shape[0] == norms.shape[0]
        self._tables = (counts, norms)     # keep alive: the index only borrows the pointers
        self._c = int(counts.shape[1])
        _lib.check(_lib.lib().hb_index_set_label_count_table(self._h, _ptr(counts), _ptr(norms), counts.shape[0], counts.shape[1],
                                                             int(P), int(id_base)))

    def set_label_table(self, labels: Optional[torch.Tensor], norms: Optional[torch.Tensor], id_base: int = 0):
        """Borrow all-gathered label / norm tables that cover global ids [id_base, id_base + n)."""
        if labels is None:
            self._tables = None
            _lib.check(_lib.lib().hb_index_set_label_table(self._h, None, None, 0, 0, 0))
            return
        labels = labels.contiguous().float(); norms = norms.contiguous().float()
        assert labels.is_cuda and norms.is_cuda and labels.shape[0] == norms.shape[0]
        self._tables = (labels, norms)     # keep alive: the index only borrows the pointers
        self._c = int(labels.shape[1])
        _lib.check(_lib.lib().hb_index_set_label_table(self._h, _ptr(labels), _ptr(norms), labels.shape[0],
                                                       labels.shape[1], int(id_base)))

    def set_timing(self, on: bool):
        _lib.check(_lib.lib().hb_index_set_timing(self._h, int(on)))

    def last_knn_ms(self) -> float:
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().hb_index_last_knn_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def set_tuning(self, workgroups: int = 0, panel_tiles: int = 0):
        _lib.check(_lib.lib().hb_index_set_tuning(self._h, int(workgroups), int(panel_tiles)))

    def set_fp16(self, enable):
        """fp16 candidate pass + exact fp32 re-rank (GpuIndexFlatConfig.useFloat16 of the reference).  True / 1: always;
        2: only where it is faster than the fp32 kernel -- banks of at least 4,096 rows with rows x queries x D >= 1.5e10 x (k' / 64)^2 (same results
        either way).  False / 0: the fp32 kernel, no fp16 copy.  "auto": the state a new index starts in -- big exact searches take the certified
        fp16 screen where it is known to pay and its copy fits (hb_index_set_fp16, include/hbird_hip.h; last_search_path() says what ran)."""
        if isinstance(enable, str):
            if enable != "auto":
                raise ValueError(f"set_fp16: {enable!r} (False / True / 2 / 'auto')")
            mode = 3                          # HB_FP16_AUTO
        else:
            mode = 2 if enable == 2 and enable is not True else int(bool(enable))
        _lib.check(_lib.lib().hb_index_set_fp16(self._h, mode))

    SEARCH_PATHS = ("fp32", "fp16_chain", "fp16_wide")
    SEARCH_REASONS = ("explicit_fp32", "explicit_fp16", "auto", "k", "ceiling", "work", "small", "pinned", "env", "memory", "overflow", "adaptive")

    def last_search_path(self) -> dict:
        """What served the last search (hb_last_search_path): the fp32 kernel, the fp16 chain or one wide fp16 pass, and why (HB_WHY_*)."""
        path, why = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.lib().hb_last_search_path(self._h, ctypes.byref(path), ctypes.byref(why)))
        out = {"path": self.SEARCH_PATHS[path.value], "reason": self.SEARCH_REASONS[why.value]}
        if self._fp16_centre:                 # (the field exists while centring is switched on: an index left alone reports what it always did)
            out["centred"] = self.fp16_centre_info()["last_search_centred"]
        return out

    def set_fp16_centre(self, on: bool = True):
        """The fp16 candidate copy in its mean-centred form (hb_index_set_fp16_centre, include/hbird_hip_centre.h): the pass runs on q - t mu and
        b - mu, so the certificate's bound scales with the centred norms -- banks with massive activations certify at the first pass.  Same results
        (the fp32 search's bits) on or off; off on a new index.  A change drops the fp16 copy, the next screened search rebuilds it."""
        _lib.check(_lib.lib().hb_index_set_fp16_centre(self._h, int(bool(on))))
        self._fp16_centre = bool(on)

    def fp16_centre_info(self) -> dict:
        """hb_index_fp16_centre_info: centred (the copy holds centred rows), mu_norm, cmax = max ||b - mu||, bmax = max ||b||, t of the last centred
        search, rows converted with mu, the setting, and whether the last search ran centred."""
        out = (ctypes.c_double * 8)()
        _lib.check(_lib.lib().hb_index_fp16_centre_info(self._h, out))
        return {"centred": bool(out[0]), "mu_norm": float(out[1]), "cmax": float(out[2]), "bmax": float(out[3]), "t": float(out[4]),
                "rows": int(out[5]), "setting": bool(out[6]), "last_search_centred": bool(out[7])}

    def last_centre(self, queries: bool = True) -> dict:
        """What the centred conversion left (hb_index_last_centre, include/hbird_hip_centre.h), as numpy arrays.  Bank side: mu float32 [n_mu],
        cmax / mu_norm / mu2 / t (numpy float32 scalars, the device's four), g float32 [32 ceil(rows / 32)], init16 float32 [256 ceil(rows / 256)],
        bank16 uint16 (the raw fp16 tiles of the converted row tiles; layout in the header), rows, dp16, n_mu.  Query side, of the last centred
        pass: n, level (0: the caller's pass, 1: the second pass over its uncertified queries), cq / qcn float32 [n], q16 uint16 (raw tiles of
        256 ceil(n / 256) queries).  queries=False reads the bank side only (n = 0, level = -1 when the query side is not valid).  Raises
        when there is no active centred copy, and with queries=True when the last search of a caller did not run centred or the bank has changed
        since."""
        lib = _lib.lib()
        info = (ctypes.c_int64 * 8)()
        _lib.check(lib.hb_index_last_centre(self._h, None, None, None, None, None, None, None, None, info))
        rows, dp16, n_mu, n, level, n_g, n_init, n_qpad = (int(v) for v in info)
        mu, sc = np.empty(n_mu, dtype=np.float32), np.empty(4, dtype=np.float32)
        g, init16 = np.empty(n_g, dtype=np.float32), np.empty(n_init, dtype=np.float32)
        bank16 = np.empty(n_g * dp16, dtype=np.uint16)
        out = {"rows": rows, "dp16": dp16, "n_mu": n_mu, "n": n, "level": level}
        if queries:
            cq, qcn, q16 = np.empty(max(n, 1), dtype=np.float32), np.empty(max(n, 1), dtype=np.float32), np.empty(max(n_qpad * dp16, 1), dtype=np.uint16)
            _lib.check(lib.hb_index_last_centre(self._h, _ptr(mu), _ptr(sc), _ptr(g), _ptr(init16), _ptr(bank16), _ptr(cq), _ptr(qcn), _ptr(q16), info))
            out.update(cq=cq[:n], qcn=qcn[:n], q16=q16[:n_qpad * dp16])
        else:
            _lib.check(lib.hb_index_last_centre(self._h, _ptr(mu), _ptr(sc), _ptr(g), _ptr(init16), _ptr(bank16), None, None, None, info))
        out.update(mu=mu, cmax=sc[0], mu_norm=sc[1], mu2=sc[2], t=sc[3], g=g, init16=init16, bank16=bank16)
        return out

    def last_fp16_fallbacks(self) -> int:
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().hb_index_last_fp16_fallbacks(self._h, ctypes.byref(n)))
        return int(n.value)

    def last_fp16_escalated(self) -> int:
        """Queries of the last use_fp16 search whose first certificate failed (they got the second, wider fp16 pass; last_fp16_fallbacks():
        those that reached the fp32 kernel)."""
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().hb_index_last_fp16_escalated(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_fp16_escalation(self, on: bool = True):
        """use_fp16: uncertified queries get a second fp16 pass (k' = 256, seeded floors) before the fp32 kernel (default), or go straight to it."""
        _lib.check(_lib.lib().hb_index_set_fp16_escalation(self._h, 0 if on else 1))

    def last_screen(self) -> dict:
        """What the level-0 fp16 candidate pass of the last search left (hb_index_last_screen, include/hbird_hip_screen.h), as numpy arrays:
        rows int64 [nq, kc] (bank rows without id_base, -1: none), scores float32 [nq, kc] (the kernel's own pass scores; centred: without
        c_q), certified uint8 [nq] (the first certificates), and nq, kc, klw, centred.  Raises when the last search did not take the fp16
        path, when its second pass has overwritten the lists (set_fp16_escalation(False) keeps them), or after reset / add."""
        lib = _lib.lib()
        info = (ctypes.c_int64 * 4)()
        _lib.check(lib.hb_index_last_screen(self._h, None, None, None, 0, info))
        nq, kc = int(info[0]), int(info[1])
        rows, scores, cert = np.empty((nq, kc), dtype=np.int64), np.empty((nq, kc), dtype=np.float32), np.empty(nq, dtype=np.uint8)
        _lib.check(lib.hb_index_last_screen(self._h, _ptr(rows), _ptr(scores), _ptr(cert), nq, info))
        return {"rows": rows, "scores": scores, "certified": cert, "nq": nq, "kc": kc, "centred": bool(info[2]), "klw": int(info[3])}

    def last_screen_seeds(self) -> dict:
        """What the chain behind the first candidate pass left (hb_index_last_screen_seeds, include/hbird_hip_screen.h), as numpy arrays.
        Level 0: kth0 / floor0 float32 [nq], certified0 uint8 [nq].  Level 1, where a second fp16 pass ran (n1 > 0; else empty arrays):
        queries1 int64 [n1] (ascending level-0 query numbers), seed1 float32 [n1] (as gathered on the device), rows1 int64 [n1, kc1] and
        scores1 float32 [n1, kc1] (that pass' merged lists, conventions of last_screen), certified1 uint8 [n1], kth1 float32 [n1]; and nq,
        kc0, klw0, n1, kc1, klw1, centred, n2 (queries that reached the fp32 kernel).  After an excluding search that the screen served: kth0 /
        kth1 over the ALLOWED candidates of the unmasked lists, n2 the queries handed to the rungs (`last_exclusion_seeds`).  Raises when the
        last search did not take the fp16 path, or after reset / add / a capacity change."""
        lib = _lib.lib()
        info = (ctypes.c_int64 * 8)()
        _lib.check(lib.hb_index_last_screen_seeds(self._h, *([None] * 9), 0, 0, info))
        nq, kc0, n1, kc1 = (int(info[i]) for i in range(4))
        kth0, floor0, cert0 = np.empty(nq, dtype=np.float32), np.empty(nq, dtype=np.float32), np.empty(nq, dtype=np.uint8)
        queries1, seed1 = np.empty(n1, dtype=np.int64), np.empty(n1, dtype=np.float32)
        rows1, scores1 = np.empty((n1, kc1), dtype=np.int64), np.empty((n1, kc1), dtype=np.float32)
        cert1, kth1 = np.empty(n1, dtype=np.uint8), np.empty(n1, dtype=np.float32)
        lvl1 = [_ptr(a) if n1 else None for a in (queries1, seed1, rows1, scores1, cert1, kth1)]
        _lib.check(lib.hb_index_last_screen_seeds(self._h, _ptr(kth0), _ptr(floor0), _ptr(cert0), *lvl1, nq, n1, info))
        return {"nq": nq, "kc0": kc0, "klw0": int(info[7]), "n1": n1, "kc1": kc1, "klw1": int(info[4]), "centred": bool(info[5]), "n2": int(info[6]),
                "kth0": kth0, "floor0": floor0, "certified0": cert0, "queries1": queries1, "seed1": seed1, "rows1": rows1, "scores1": scores1,
                "certified1": cert1, "kth1": kth1}

    def last_fp16_copy(self, queries: bool = True) -> dict:
        """The plain fp16 copy (hb_index_last_fp16_copy, include/hbird_hip_screen.h): bank16 uint16 (the raw fp16 tiles of the converted row
        tiles; layout in hbird_hip_centre.h), rows, dp16, flag (the device's sticky overflow flag) and flag_host (its host image); of the last
        plain candidate pass n, level (0: the caller's, 1: the second pass; -1 and n = 0 when not valid) and, with queries=True, q16 uint16
        (raw tiles of 256 ceil(n / 256) queries).  Raises while there is no plain copy, and with queries=True when the last search of a caller
        did not run the plain pass or the bank has changed since."""
        lib = _lib.lib()
        info = (ctypes.c_int64 * 8)()
        _lib.check(lib.hb_index_last_fp16_copy(self._h, None, None, info))
        rows, dp16, n_g, _, _, n, _, n_qpad = (int(v) for v in info)
        bank16 = np.empty(n_g * dp16, dtype=np.uint16)
        q16 = np.empty(max(n_qpad * dp16, 1), dtype=np.uint16)
        _lib.check(lib.hb_index_last_fp16_copy(self._h, _ptr(bank16) if n_g else None, _ptr(q16) if queries else None, info))
        out = {"rows": rows, "dp16": dp16, "flag": int(info[3]), "flag_host": int(info[4]), "n": n, "level": int(info[6]), "bank16": bank16}
        if queries:
            out["q16"] = q16[:n_qpad * dp16]
        return out

    def set_variant(self, variant: int):
        _lib.check(_lib.lib().hb_index_set_variant(self._h, int(variant)))

    def set_search_options(self, phases: bool = True, small_limit_stages: int = 0):
        """A/B switches (same results): pool searches in one launch instead of phases; the size below which a search is "small"."""
        _lib.check(_lib.lib().hb_index_set_search_options(self._h, int(bool(phases)), int(small_limit_stages)))

    def set_xcd_weights(self, mode: int = 0, w8=None):
        """Work share per XCD group (blocks equal mod 8) of every panel of the work list (speed only, same results): mode 0 = calibrated from
        the workgroups' own durations (default), 1 = equal shares, 2 = the eight shares `w8`."""
        arr = None if w8 is None else (ctypes.c_double * 8)(*[float(v) for v in w8])
        _lib.check(_lib.lib().hb_index_set_xcd_weights(self._h, int(mode), arr))

    def xcd_weights(self, fp16_kernel: bool = False):
        """(the eight shares in use by the fp32 kernels / by the fp16 candidate kernel, calibration rounds so far)"""
        arr = (ctypes.c_double * 8)(); r = ctypes.c_int(0)
        _lib.check(_lib.lib().hb_index_xcd_weights(self._h, int(bool(fp16_kernel)), arr, ctypes.byref(r)))
        return [float(v) for v in arr], int(r.value)

    def wg_stamps(self):
        """After a search with set_timing(True): int64 array [workgroups, 3] = (start, end) in 100 MHz ticks relative to the earliest start,
        XCC id -- of the last kNN launch (hb_index_wg_stamps)."""
        buf = np.zeros((1024, 4), dtype=np.uint32)
        g = ctypes.c_int(0)
        _lib.check(_lib.lib().hb_index_wg_stamps(self._h, _ptr(buf), 1024, ctypes.byref(g)))
        t = buf[: g.value].astype(np.int64)
        if t.size:
            t0 = t[:, 0].min()
            t[:, 0] = (t[:, 0] - t0) & 0xFFFFFFFF; t[:, 1] = (t[:, 1] - t0) & 0xFFFFFFFF
        return t[:, :3]

    def kernel_clock(self) -> dict:
        """Clock of the last stamped kNN launch without a profiler attached (hb_index_kernel_clock): median / slowest / fastest workgroup in
        GHz (shader cycles per real-time tick) and the launch's span in ms; zeros when the launch did not stamp."""
        out = (ctypes.c_double * 4)()
        _lib.check(_lib.lib().hb_index_kernel_clock(self._h, out))
        return {"ghz": float(out[0]), "ghz_min": float(out[1]), "ghz_max": float(out[2]), "span_ms": float(out[3])}

    def xcd_stats(self, fp16_kernel: bool = False) -> dict:
        """State of the share calibration (hb_index_xcd_stats): rounds, the guard's lock / reverts, stamp sets read / rejected, shortest launch
        with the best / the current shares (ms), work lists built for this index."""
        out = (ctypes.c_double * 12)()
        _lib.check(_lib.lib().hb_index_xcd_stats(self._h, int(bool(fp16_kernel)), out))
        keys = ["rounds", "locked", "reverts", "samples", "rejected"]
        d = {k: int(out[i]) for i, k in enumerate(keys)}
        d.update({"best_span_ms": float(out[5]), "cur_span_ms": float(out[6]), "work_lists_built": int(out[7]), "xcd_map_moves": int(out[8]),
                  "xcd_of_block0": int(out[9]), "clusters_kept": int(out[10]), "clustered_minus_unclustered_ms": float(out[11])})
        return d

    def set_rerank_copy(self, mode: int = 0):
        """use_fp16 searches: a second, row-major fp32 copy of the bank for the exact re-rank (speed only; 0 automatic -- made for banks of up
        to 16 GB when 2.5 x the bank stays within 55 % of the device's memory: beyond that it buys under 2 % --, 1 always, 2 never)."""
        _lib.check(_lib.lib().hb_index_set_rerank_copy(self._h, int(mode)))

    def rerank_copy_bytes(self) -> int:
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().hb_index_rerank_copy_bytes(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_cluster(self, cluster_q: int = 0, cluster_b: int = 0, sync_lag: int = -1):
        """L2-sharing clusters of the work list (speed only, opt-in): 0 x 0 / 1 x 1 off, e.g. 2 x 2; sync_lag in stages."""
        _lib.check(_lib.lib().hb_index_set_cluster(self._h, int(cluster_q), int(cluster_b), int(sync_lag)))

    def set_cluster_sharing(self, mode: int = 0):
        """How a clustered work list is dealt (speed only): 0 automatic, 1 per-cluster ranges, 2 XCD-level query-tile sharing, 3 the same with
        the leftover query tiles of a ragged last group dealt as rows of other shapes (the filled list; fp16 candidate pass)."""
        _lib.check(_lib.lib().hb_index_set_cluster_sharing(self._h, int(mode)))

    def cluster_stats(self) -> dict:
        out = (ctypes.c_int64 * 4)()
        _lib.check(_lib.lib().hb_index_cluster_stats(self._h, out))
        return {"checks": int(out[0]), "waits": int(out[1]), "timeouts": int(out[2])}

    def schedule_info(self) -> dict:
        out = (ctypes.c_int64 * 8)()
        _lib.check(_lib.lib().hb_index_schedule_info(self._h, out))
        keys = ["workgroups", "segments", "slots", "panel_tiles", "max_slots_per_qtile", "query_tiles", "bank_tiles"]
        d = dict(zip(keys, list(out)[:7]))
        d["cluster"] = [int(out[7]) // 16, int(out[7]) % 16]
        fill = (ctypes.c_int64 * 4)()
        _lib.check(_lib.lib().hb_last_schedule_fill(self._h, fill))
        d["filled"] = int(fill[0]); d["idle_member_ticks"] = int(fill[1]); d["member_ticks"] = int(fill[2])
        if fill[3]:
            d["fill_refused"] = 1      # (a filled list was asked for and would have broken the slot limit: the list of old ran)
        return d


def _merge_fits_lds(parts: int, k: int) -> bool:
    """parts * k candidates fit the old merge kernel's LDS staging (hb_launch_merge_parts' own test)."""
    n = parts * k
    return (n * 4 + 15) // 16 * 16 + n * 8 <= _MERGE_LDS


def merge_topk(dist_parts: torch.Tensor, idx_parts: torch.Tensor, metric: int):
    """[parts, nq, k] CUDA tensors -> merged (idx [nq,k], dist [nq,k]); hb_merge_topk while parts * k fits its LDS staging, beyond that
    hb_bigk_merge_topk, whose lists must be sorted best-first with the missing entries last (what a search returns)."""
    parts, nq, k = dist_parts.shape
    dist_parts = dist_parts.contiguous(); idx_parts = idx_parts.contiguous()
    idx = torch.empty((nq, k), dtype=torch.int64, device=dist_parts.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=dist_parts.device)
    s = torch.cuda.current_stream(dist_parts.device).cuda_stream
    entry = _lib.lib().hb_merge_topk if _merge_fits_lds(parts, k) else _lib.lib().hb_bigk_merge_topk
    _lib.check(entry(_ptr(dist_parts), _ptr(idx_parts), parts, nq, k, int(metric), _ptr(idx), _ptr(dist), ctypes.c_void_p(s)))
    return idx, dist


def merge_topk_packed(recv: torch.Tensor, part_bytes: int, parts: int, nq: int, k: int, metric: int):
    """The gathered buffer of a dist.PackedTopK (CUDA, `parts` packed lists part_bytes apart) -> merged (idx, dist);
    hb_merge_topk_packed reads it in place (hb_bigk_merge_topk_packed where parts * k is beyond its staging: sorted lists, see merge_topk)."""
    assert recv.is_cuda and recv.is_contiguous() and recv.numel() * recv.element_size() >= parts * part_bytes
    idx = torch.empty((nq, k), dtype=torch.int64, device=recv.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=recv.device)
    s = torch.cuda.current_stream(recv.device).cuda_stream
    entry = _lib.lib().hb_merge_topk_packed if _merge_fits_lds(parts, k) else _lib.lib().hb_bigk_merge_topk_packed
    _lib.check(entry(_ptr(recv), int(part_bytes), int(parts), int(nq), int(k), int(metric), _ptr(idx), _ptr(dist), ctypes.c_void_p(s)))
    return idx, dist


class HipMultiIndex:
    """Several `hb_index_t` of ONE process behind the `HipFlatIndex` interface: what the reference's single-process call
    does with faiss (search_faiss.py:50-76).  `shard=True` = faiss.IndexShards (53-63): contiguous row ranges with
    successive ids, one per listed GPU, every GPU searches all queries, the [nq, k] lists are peer-copied to the first
    GPU and merged there on the ordering scores (the single-index bits).  `shard=False` = faiss.IndexReplicas (65-74):
    every GPU holds all rows, the queries are split.  One host thread per index (faiss `threaded=True`, 57).

    The FIRST listed device is the home device: queries arrive there, results are returned there, and the label rows
    and bank-row norms of ALL rows live there (the aggregation runs on it; 6.2 GB at BASELINE cfg-3).  A GPU may be
    listed more than once (several indices on one device: how the 1-GPU test boxes exercise this path)."""

    def __init__(self, d: int, metric: int, devices, shard: bool):
        assert len(devices) >= 1
        self.d, self.metric, self.devices, self.shard = int(d), int(metric), [int(g) for g in devices], bool(shard)
        self.device = self.devices[0]
        self.home = torch.device("cuda", self.device)
        self.indexes = [HipFlatIndex(d, metric, g) for g in self.devices]
        self.agg = HipFlatIndex(d, metric, self.device)        # row-less handle: aggregation against the home tables
        # peer access between the home device and every other listed GPU (xGMI on one node): without it a cross-device copy is staged
        # through pinned host memory explicitly -- one warning, same results
        self._staged = set()
        for g in sorted(set(self.devices)):
            if g != self.device and torch.cuda.is_available() and not (torch.cuda.can_device_access_peer(self.device, g)
                                                                         and torch.cuda.can_device_access_peer(g, self.device)):
                self._staged.add(g)
        if self._staged:
            import warnings
            warnings.warn(f"HipMultiIndex: no peer access between cuda:{self.device} and {sorted(self._staged)}: rows, queries and neighbour "
                          "lists are staged through host memory (slower copies, same results)", RuntimeWarning, stacklevel=2)
        self._warned_no_plan = False
        self._label_P = 0               # > 0: label rows are kept as int16 counts j of values j / P (set_label_denominator)
        self._quota = None              # shard mode: planned rows per shard (reserve); None = everything into the first
        self._labels = None             # [cap, C] on the home device, co-indexed with the global row ids
        self._nlab = 0
        self._norms = None              # [ntotal] on the home device (rebuilt lazily after adds)
        self._pool = None
        self._c = None
        self._fallbacks = 0

    # -- bookkeeping ------------------------------------------------------------------------------------------------
    def close(self):
        for ix in self.indexes + [self.agg]:
            ix.close()
        if self._pool is not None:
            self._pool.shutdown(wait=False)
            self._pool = None

    @property
    def ntotal(self) -> int:
        return sum(ix.ntotal for ix in self.indexes) if self.shard else self.indexes[0].ntotal

    @property
    def shard_rows(self):
        return [ix.ntotal for ix in self.indexes]

    @property
    def shard_bases(self):
        if not self.shard:
            return [0] * len(self.indexes)
        out, b = [], 0
        for ix in self.indexes:
            out.append(b); b += ix.ntotal
        return out

    @property
    def num_classes(self) -> int:
        if self._c is None:
            raise RuntimeError("labels were not added to this index")
        return self._c

    def set_num_classes(self, c: int):
        self._c = int(c)

    def use_current_stream(self):
        """Work on the home device follows the caller's current stream there; the per-GPU searches run on their worker
        threads' streams and are synchronised before their lists are handed over."""
        self.agg.use_current_stream()

    def set_fp16(self, enable):
        for ix in self.indexes:
            ix.set_fp16(enable)

    def set_rerank_copy(self, mode: int = 0):
        for ix in self.indexes:
            ix.set_rerank_copy(mode)

    def set_fp16_centre(self, on: bool = True):
        """HipFlatIndex.set_fp16_centre on every shard / replica: each derives the mean of its own rows (the merged lists are the same bits)."""
        for ix in self.indexes:
            ix.set_fp16_centre(on)

    def fp16_centre_info(self) -> list:
        return [ix.fp16_centre_info() for ix in self.indexes]

    def last_fp16_fallbacks(self) -> int:
        return self._fallbacks

    def schedule_info(self) -> dict:
        return self.indexes[0].schedule_info()

    def reserve(self, n: int):
        """Plan for n rows in all: shard mode cuts them into equal contiguous ranges (the last shard also takes whatever
        arrives beyond the plan)."""
        n = max(1, int(n))
        if self.shard:
            per = (n + len(self.indexes) - 1) // len(self.indexes)
            self._quota = per
            for ix in self.indexes:
                ix.reserve(per)
        else:
            for ix in self.indexes:
                ix.reserve(n)

    def reset(self):
        for ix in self.indexes:
            ix.reset()
        self._nlab, self._norms = 0, None
        self.agg.set_label_table(None, None)

    # -- bank build -------------------------------------------------------------------------------------------------
    def _on(self, i):
        return torch.cuda.device(torch.device("cuda", self.devices[i]))

    def _move(self, t: torch.Tensor, dev: torch.device) -> torch.Tensor:
        """t on `dev`: a peer copy (xGMI) where the two GPUs can reach each other, else staged through the host."""
        if not t.is_cuda or t.device == dev:
            return t.to(dev)
        if t.device.index in self._staged or dev.index in self._staged:
            return t.cpu().to(dev)             # (.cpu() synchronises the source stream; the upload is ordered on the destination's)
        return t.to(dev)

    def _put(self, i, x, normalize):
        """Rows x (CUDA tensor on any device, CPU tensor or numpy) appended to index i on ITS device and stream."""
        ix = self.indexes[i]
        with self._on(i):
            if isinstance(x, torch.Tensor) and x.is_cuda and x.device.index != self.devices[i]:
                x = self._move(x, torch.device("cuda", self.devices[i]))   # peer copy (xGMI), ordered by torch's streams
            ix.use_current_stream()
            ix.add(x, normalize=normalize)

    def add(self, x, normalize: bool = False):
        self._norms = None
        n = x.shape[0]
        if not self.shard:
            for i in range(len(self.indexes)):
                self._put(i, x, normalize)
            return
        if self._quota is None and len(self.indexes) > 1 and not self._warned_no_plan:
            import warnings
            warnings.warn("HipMultiIndex.add in shard mode without reserve(): no row plan exists, every row goes to the first GPU "
                          f"(cuda:{self.devices[0]}) and the other {len(self.indexes) - 1} search empty shards -- correct results, "
                          "nothing sharded.  Call reserve(total_rows) first (HbirdEvaluation does when the loader has a length or "
                          "memory_size is set).", RuntimeWarning, stacklevel=2)
            self._warned_no_plan = True
        lo = 0
        while lo < n:
            i = len(self.indexes) - 1
            if self._quota is None:
                i = 0
            else:
                for j, ix in enumerate(self.indexes[:-1]):
                    if ix.ntotal < self._quota:
                        i = j
                        break
            room = n - lo
            if self._quota is not None and i < len(self.indexes) - 1:
                room = min(room, self._quota - self.indexes[i].ntotal)
            self._put(i, x[lo:lo + room], normalize)
            lo += room

    def set_label_denominator(self, P: int):
        """As HipFlatIndex.set_label_denominator: the home device's label table holds int16 counts (P <= 32767)."""
        if self._nlab and int(P) != self._label_P:
            raise RuntimeError("set_label_denominator: the index already holds label rows")
        if not 0 <= int(P) <= 32767:
            raise ValueError("set_label_denominator: P must be in [0, 32767]")
        if (int(P) == 0) != (self._label_P == 0):
            self._labels = None         # fp32 values <-> int16 counts: a table kept by reset() has the other form's dtype
        self._label_P = int(P)

    def labels_to_fp32(self):
        """As HipFlatIndex.labels_to_fp32: int16 counts j -> fp32 values j / P (float32 division: the quotient K2 computed), denominator 0."""
        if self._label_P and self._labels is not None:
            self._labels = self._labels.to(torch.float32) / torch.tensor(float(self._label_P), device=self._labels.device)
        self._label_P = 0

    @property
    def label_denominator(self) -> int:
        return self._label_P

    def add_labels(self, lab):
        """label_memory rows (hbird_eval.py:329, 354) of the rows just added, in global row order, on the home device."""
        if not isinstance(lab, torch.Tensor):
            lab = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.float32))
        lab = lab.detach().float()
        n, c = lab.shape
        self._c = int(c)
        need = self._nlab + n
        dt = torch.int16 if self._label_P else torch.float32
        if self._labels is None or self._labels.shape[0] < need or self._labels.shape[1] != c or self._labels.dtype != dt:
            planned = (self._quota * len(self.indexes)) if (self.shard and self._quota) else 0
            cap = max(need, planned, 0 if self._labels is None else self._labels.shape[0] * 3 // 2)
            grown = torch.empty((cap, c), dtype=dt, device=self.home)
            if self._nlab:
                grown[:self._nlab] = self._labels[:self._nlab]
            self._labels = grown
        lab = lab.to(self.home)
        if self._label_P:
            # (a 0-dim TENSOR divisor: torch turns a division by a Python scalar into a multiplication by its reciprocal on the GPU,
            # which rounds differently from the (float)j / (float)P that K2 and the library compute)
            Pt = torch.tensor(float(self._label_P), device=lab.device)
            cnt = torch.round(lab * Pt)
            if not bool(((cnt / Pt) == lab).all()):       # same exactness rule as the library (labels_to_counts_kernel)
                raise RuntimeError(f"label rows are not multiples of 1 / {self._label_P} (set_label_denominator): store them as fp32 instead")
            lab = cnt.to(torch.int16)
        self._labels[self._nlab:need] = lab
        self._nlab = need
        self._norms = None

    def _tables(self):
        """(labels [ntotal, C], norms [ntotal]) on the home device, handed to the aggregation handle."""
        if self._norms is None:
            n = self.ntotal
            with torch.cuda.device(self.home):
                if self.shard:
                    parts = []
                    for i, ix in enumerate(self.indexes):
                        with self._on(i):
                            ix.use_current_stream()
                            nr = ix.copy_norms()
                            torch.cuda.current_stream(nr.device).synchronize()
                        parts.append(self._move(nr, self.home))
                    self._norms = torch.cat(parts) if parts else torch.zeros(0, device=self.home)
                else:
                    with self._on(0):
                        self.indexes[0].use_current_stream()
                        self._norms = self.indexes[0].copy_norms()
                        torch.cuda.current_stream(self.home).synchronize()
                if self._labels is not None and self._nlab >= n and n > 0:
                    if self._label_P:
                        self.agg.set_label_count_table(self._labels[:n], self._norms, self._label_P, 0)
                    else:
                        self.agg.set_label_table(self._labels[:n], self._norms, 0)
        return (None if self._labels is None else self._labels[:self.ntotal]), self._norms

    def copy_norms(self) -> torch.Tensor:
        return self._tables()[1]

    # -- search -----------------------------------------------------------------------------------------------------
    def _threads(self):
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=len(self.indexes), thread_name_prefix="hbird-gpu")
        return self._pool

    def _search(self, q, k: int, id_base: int, scores: bool):
        if isinstance(q, torch.Tensor) and q.is_cuda:
            q = q.detach().float().contiguous()
        else:
            q = torch.as_tensor(np.ascontiguousarray(q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else q,
                                                     dtype=np.float32)).to(self.home)
        n = len(self.indexes)
        nq = q.shape[0]
        bases = self.shard_bases
        # q is complete before other devices' streams (and the workers' own streams on q's device) read it
        torch.cuda.current_stream(q.device).synchronize()
        # ... and so is every index: the workers run on THEIR threads' current streams (the default streams), while add() / peer
        # copies were enqueued on the CALLER's current stream of each device -- not the same when the bank was built under a
        # torch.cuda.stream(...) context
        for d in set(self.devices):
            torch.cuda.current_stream(torch.device("cuda", d)).synchronize()

        def run(i):
            index, dev = self.indexes[i], torch.device("cuda", self.devices[i])
            with torch.cuda.device(dev):
                if self.shard:
                    qi = q if dev == q.device else self._move(q, dev)
                else:
                    a, b = (nq * i) // n, (nq * (i + 1)) // n       # replicas: a slice of the queries each
                    qi = q[a:b] if dev == q.device else self._move(q[a:b], dev)
                index.use_current_stream()
                # shards always return ordering scores: the merge must see what the single index orders by
                idx, d = (index.search_scores if (self.shard or scores) else index.search)(qi.contiguous(), k, id_base + bases[i])
                fb = index.last_fp16_fallbacks()
                torch.cuda.current_stream(dev).synchronize()
                idx, d = self._move(idx, self.home), self._move(d, self.home)   # peer copy of the [nq, k] lists (xGMI)
                # the copy was enqueued on THIS thread's current streams (torch runs a peer copy on the source device's stream and
                # makes the destination's wait for it), the caller merges on its own: the lists must have landed before the
                # worker hands them over
                torch.cuda.current_stream(dev).synchronize()
                torch.cuda.current_stream(self.home).synchronize()
                return idx, d, fb

        parts = list(self._threads().map(run, range(n)))
        self._fallbacks = sum(p[2] for p in parts)
        with torch.cuda.device(self.home):
            if not self.shard:
                return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            idx, sc = merge_topk(torch.stack([p[1] for p in parts]), torch.stack([p[0] for p in parts]), 0)
            if scores:
                return idx, sc
            qh = q if q.device == self.home else q.to(self.home)
            self.agg.use_current_stream()
            return idx, self.agg.distances_from_scores(qh, sc.contiguous())

    def search(self, q, k: int, id_base: int = 0, out=None):
        host = not (isinstance(q, torch.Tensor) and q.is_cuda)
        idx, dist = self._search(q, k, id_base, False)
        if out is not None:
            out[0].copy_(idx); out[1].copy_(dist)
            return out
        return (idx.cpu().numpy(), dist.cpu().numpy()) if host else (idx, dist)

    def search_scores(self, q, k: int, id_base: int = 0, out=None):
        idx, sc = self._search(q, k, id_base, True)
        if out is not None:
            out[0].copy_(idx); out[1].copy_(sc)
            return out
        return idx, sc

    def distances_from_scores(self, q, scores):
        return self.agg.distances_from_scores(q, scores)

    def aggregate(self, q, idx, dist, beta: float = 0.02, id_base: int = 0):
        self._tables()
        with torch.cuda.device(self.home):
            self.agg.use_current_stream()
            return k5(self.agg, "aggregate", idx.shape[1])(q.to(self.home), idx, dist, beta=beta, id_base=id_base)

    def search_aggregate(self, q, k: int, beta: float = 0.02, id_base: int = 0, want_neighbours: bool = False):
        """K4 on every GPU, merge on the home device, K5 there (hb_index_aggregate on the merged lists)."""
        host = not (isinstance(q, torch.Tensor) and q.is_cuda)
        if host:
            q = (q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32))).to(self.home)
        idx, dist = self._search(q, k, id_base, False)
        out = self.aggregate(q.float().contiguous(), idx, dist, beta=beta, id_base=id_base)
        if host:
            out, idx, dist = out.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
        return (out, idx, dist) if want_neighbours else out

    def aggregate_grid(self, q, idx, dist, ks, betas, id_base: int = 0):
        """HipFlatIndex.aggregate_grid on the aggregation handle (the home device's tables)."""
        self._tables()
        with torch.cuda.device(self.home):
            self.agg.use_current_stream()
            return self.agg.aggregate_grid(q.to(self.home), idx, dist, ks, betas, id_base=id_base)

    def search_aggregate_grid(self, q, ks, betas, id_base: int = 0, want_neighbours: bool = False):
        """K4 on every GPU at max(ks), merge on the home device as for `search_aggregate`, the grid's K5 there."""
        plan = grid_plan(ks, betas)
        host = not (isinstance(q, torch.Tensor) and q.is_cuda)
        if host:
            q = (q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32))).to(self.home)
        idx, dist = self._search(q, plan.ks[-1], id_base, False)
        out = self.aggregate_grid(q.float().contiguous(), idx, dist, plan.ks, plan.betas, id_base=id_base)
        if host:
            out, idx, dist = out.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
        return (out, idx, dist) if want_neighbours else out

    # -- row access (return_knn_details, persistence) -------------------------------------------------------------------
    def reconstruct(self, ids, id_base: int = 0):
        host = not (isinstance(ids, torch.Tensor) and ids.is_cuda)
        ids_h = (torch.as_tensor(np.asarray(ids)) if host else ids).to(self.home).to(torch.int64).contiguous().view(-1)
        if not self.shard:
            with self._on(0):
                self.indexes[0].use_current_stream()
                out = self.indexes[0].reconstruct(ids_h, id_base)
        else:
            out = torch.zeros((ids_h.numel(), self.d), dtype=torch.float32, device=self.home)
            bases = self.shard_bases
            for i, ix in enumerate(self.indexes):
                lo = id_base + bases[i]
                own = (ids_h >= lo) & (ids_h < lo + ix.ntotal)
                if ix.ntotal == 0:
                    continue
                with self._on(i):
                    dev = torch.device("cuda", self.devices[i])
                    mine = self._move(torch.where(own, ids_h, torch.full_like(ids_h, -1)), dev)
                    ix.use_current_stream()
                    part = ix.reconstruct(mine, lo)                 # rows of other shards (id -1) come back as zeros
                    torch.cuda.current_stream(dev).synchronize()
                    part = self._move(part, self.home)
                    torch.cuda.current_stream(dev).synchronize()
                out += part
        return out.cpu().numpy() if host else out

    def gather_labels(self, ids):
        from hbird_mi import ops
        host = not (isinstance(ids, torch.Tensor) and ids.is_cuda)
        ids_h = (torch.as_tensor(np.asarray(ids)) if host else ids).to(self.home).to(torch.int64).contiguous().view(-1)
        with torch.cuda.device(self.home):
            if self._label_P:       # counts -> the fp32 values (float32 division: the very quotient K2 computed)
                ok = (ids_h >= 0) & (ids_h < self._nlab)
                out = self._labels[:self._nlab][ids_h.clamp(0, max(0, self._nlab - 1))].to(torch.float32) / torch.tensor(float(self._label_P), device=self.home)
                out[~ok] = 0.0
            else:
                out = ops.gather_rows(self._labels[:self._nlab], ids_h)
        return out.cpu().numpy() if host else out

    def set_label_table(self, labels, norms, id_base: int = 0):
        raise RuntimeError("HipMultiIndex keeps its own label table on the home device")

    def _no_exclusion(self, *args, **kwargs):
        """Excluding searches (HipFlatIndex.search_excluding and its fused forms) are NOT supported on a sharded or replicated bank: the
        row-group table and the rungs belong to one index on one GPU.  Always raises ValueError."""
        raise ValueError("HipMultiIndex: excluding searches are single-index (one HipFlatIndex on one GPU); sharded and replicated banks have none")

    set_row_groups = search_excluding = search_aggregate_excluding = search_aggregate_grid_excluding = last_exclusion = _no_exclusion
    set_exclusion_screen = last_exclusion_screen = last_exclusion_seeds = _no_exclusion

    def select_rows(self, ids):
        raise ValueError("HipMultiIndex.select_rows: views are single-index (one HipFlatIndex on one GPU); sharded and replicated banks have none")


class NearestNeighborSearchHIP(NearestNeighborSearchBase):
    """Exact flat search on MI355X behind the reference's plugin interface.

    Keyword surface of search_faiss.py:7: `distance_measure` ("dot_product" | "l2" | "euclidean"),
    `idx_shard`, `use_fp16` (fp16 candidate pass + exact fp32 re-rank: same answers as fp32, several times
    faster), `gpu_ids`.  With `use_fp16=False` the index stays in its automatic state: big exact searches take the same certified screen
    where it pays and its fp16 copy (half the bank again) fits; `exact_screen=False` holds it to fp32 kernels and fp32 memory only.
    Unknown keywords are swallowed like the reference's **kwargs.  Like the Faiss class it does not call
    the base constructor (search_faiss.py:7-32) and copies the bank to the GPU(s) at construction (78-81).

    GPUs.  In ONE process (the reference's call shape) the plugin drives every GPU of `gpu_ids` (default: all, as
    search_faiss.py:19-20) with one `hb_index_t` per entry and one host thread per index (faiss `threaded=True`, 57):
    `idx_shard=True` cuts the bank into contiguous row ranges with successive ids (faiss.IndexShards, 53-63) -- every
    GPU searches all queries on its range, the [nq, k] lists are copied to the first GPU (peer copy over xGMI) and
    merged there by hb_merge_topk on the ordering scores, which reproduces the single-index result bit for bit;
    `idx_shard=False` puts a full replica on every GPU and splits the queries (faiss.IndexReplicas, 65-74).
    Under torch.distributed (one process per GPU) each rank drives its own GPU only and `idx_shard=True` shards over
    the RANKS instead (RCCL all-gather of the packed lists + merge).
    """

    def __init__(self, feature_memory, n_neighbors=30, distance_measure="dot_product", idx_shard=False,
                 use_fp16=False, gpu_ids=None, **kwargs):
        self.n_neighbors = n_neighbors
        self.distance_measure = distance_measure.lower()
        self.idx_shard = idx_shard
        self.use_fp16 = use_fp16
        self.exact_screen = bool(kwargs.pop("exact_screen", True))     # use_fp16=False: the index's automatic state (True) or the fp32 kernel only (False)
        self.fp16_centre = bool(kwargs.pop("fp16_centre", False))     # the fp16 copy in its mean-centred form (set_fp16_centre): same results, a tighter certificate on ViT-shaped banks
        self.exclude_screen = bool(kwargs.pop("exclude_screen", False))     # excluding searches on the certified fp16 screen (set_exclusion_screen): same results
        self.rerank_copy = int(kwargs.pop("rerank_copy", 0))     # use_fp16 only: the re-rank's row-major copy of the bank (0 automatic, 1 always, 2 never)
        self.embed_d = feature_memory.size(1)

        self.n_gpus = _lib.device_count()
        if self.n_gpus < 1:
            raise RuntimeError("No GPUs available for the HIP index.")            # search_faiss.py:15-16
        if gpu_ids is None:
            gpu_ids = list(range(self.n_gpus))
        else:
            for gpu_id in gpu_ids:                                                 # search_faiss.py:22-25
                if gpu_id >= self.n_gpus or gpu_id < 0:
                    raise ValueError(f"Invalid GPU ID: {gpu_id}. Available GPUs: 0-{self.n_gpus - 1}")
        self.gpu_ids = list(gpu_ids)

        self.rank, self.world = 0, 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.rank, self.world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        cur = torch.cuda.current_device() if torch.cuda.is_available() else self.gpu_ids[0]
        if self.world > 1:
            # one process per GPU: this rank's GPU is the current torch device when it is listed, else the first listed
            self.local_gpus = [cur if cur in self.gpu_ids else self.gpu_ids[0]]
        else:
            self.local_gpus = list(self.gpu_ids)
        self.gpu = self.local_gpus[0]
        self.id_base = 0
        self.indexes = self._initialize_index()
        self.index = self.indexes[0]           # the first shard / replica (the only one with a single GPU)
        self._pool = None
        self._add_features_to_index(feature_memory)

    def _initialize_index(self):
        if self.distance_measure not in _METRICS:
            raise ValueError(f"Unsupported distance measure: {self.distance_measure}")   # search_faiss.py:48
        self.multi = None
        if len(self.local_gpus) > 1:
            self.multi = HipMultiIndex(self.embed_d, _METRICS[self.distance_measure], self.local_gpus, shard=bool(self.idx_shard))
            out = self.multi.indexes
        else:
            out = [HipFlatIndex(self.embed_d, _METRICS[self.distance_measure], self.local_gpus[0])]
        for index in out:
            index.set_fp16(2 if self.use_fp16 else "auto" if self.exact_screen else 0)  # search_faiss.py:40; only where it pays
            index.set_rerank_copy(self.rerank_copy)
            if self.fp16_centre:
                index.set_fp16_centre(True)
            if self.exclude_screen and isinstance(index, HipFlatIndex):
                index.set_exclusion_screen(True)
        return out

    def _add_features_to_index(self, feature_memory):
        M = feature_memory.size(0)
        lo, hi = 0, M
        if self.idx_shard and self.world > 1:
            # contiguous row ranges, successive ids (faiss.IndexShards.add, search_faiss.py:56-63)
            per = (M + self.world - 1) // self.world
            lo, hi = min(M, self.rank * per), min(M, (self.rank + 1) * per)
        self.id_base = lo
        target = self.multi if self.multi is not None else self.index
        target.reserve(max(hi - lo, 1))       # several local GPUs + idx_shard: equal contiguous ranges, successive ids
        target.add(feature_memory[lo:hi])
        self.shard_bases = [lo + b for b in self.multi.shard_bases] if self.multi is not None else [lo]

    def find_nearest_neighbors(self, q, k=None):
        if k is None:
            k = self.n_neighbors
        # faiss-gpu raises for k > 2048 (its k-select limit); so does every index here, one GPU or sharded (beyond 256 in ceil(k / 256)
        # passes, the shards' lists merged by hb_bigk_merge_topk where they outgrow hb_merge_topk's staging)
        check_k(k)
        if isinstance(q, torch.Tensor) and q.is_cuda:
            idx, dist = self._search_device(q, k)
            return idx, dist
        q_np = q.cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)   # search_faiss.py:88
        if (self.idx_shard and self.world > 1) or self.multi is not None:
            idx, dist = self._search_device(torch.from_numpy(np.ascontiguousarray(q_np, dtype=np.float32)).cuda(self.gpu), k)
            return idx.cpu().numpy(), dist.cpu().numpy()
        indices, distances = self.index.search(q_np, k, self.id_base)
        return indices, distances                                                  # (I, D) order: search_faiss.py:89-90

    def find_nearest_neighbors_excluding(self, q, qgroups, k=None):
        """`find_nearest_neighbors` over the rows whose group (index.set_row_groups) differs from qgroups[i]; one GPU, no torch.distributed
        sharding (ValueError otherwise)."""
        if k is None:
            k = self.n_neighbors
        check_k(k)
        if self.multi is not None or (self.idx_shard and self.world > 1):
            raise ValueError("find_nearest_neighbors_excluding: excluding searches are single-index (one GPU, no sharding)")
        if isinstance(q, torch.Tensor) and q.is_cuda:
            self.index.use_current_stream()
            return self.index.search_excluding(q, k, qgroups, self.id_base)
        q_np = q.cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)
        return self.index.search_excluding(q_np, k, qgroups, self.id_base)

    def _search_local(self, q: torch.Tensor, k: int, id_base_unused: int = 0, scores: bool = False):
        """All local GPUs on q (a CUDA tensor) -> (idx, dist | ordering scores) on the first GPU."""
        if self.multi is not None:
            return (self.multi.search_scores if scores else self.multi.search)(q, k, self.id_base)
        self.index.use_current_stream()
        return (self.index.search_scores if scores else self.index.search)(q, k, self.id_base)

    def _search_device(self, q: torch.Tensor, k: int):
        if self.idx_shard and self.world > 1:
            from hbird_mi import dist as hdist
            self.index.use_current_stream()
            return hdist.sharded_search(lambda qq, kk, base: self._search_local(qq, kk, base, scores=True), merge_topk, q, k,
                                        self.id_base, _METRICS[self.distance_measure],
                                        finish=self.index.distances_from_scores, merge_packed=merge_topk_packed)
        return self._search_local(q, k)
