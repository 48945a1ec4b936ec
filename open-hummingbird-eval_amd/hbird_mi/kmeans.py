"""k-means over a resident bank (include/hbird_hip_kmeans.h, csrc/hbird_kmeans.hip): the clustering of the overclustering protocol.

The assignment step is the engine's exact k = 1 search on an L2 index of the centroids (ties to the lower id, -1 for a row with a non-finite
component); the update sums Q(x) = rint(x * 2^30) in int64, so centroids are the same bits every run, whatever the chunking.  Every
arithmetic step runs in libhbird_hip.so; torch holds memory only.

A duplicated initial row leaves the higher-id twin empty in the first iteration (the lower id takes every tie): an empty cluster keeps its
centroid and is counted in `history`; it is not re-seeded, and wins rows again only if they come to lie nearer to it than to its moved twin.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

HISTORY_FIELDS = ("changed", "empty", "unassigned", "inertia")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _single_index(index, who: str) -> HipFlatIndex:
    if isinstance(index, HipMultiIndex):
        raise ValueError(f"{who}: k-means runs on one HipFlatIndex -- a HipMultiIndex (row shards or replicas) is not supported yet")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise ValueError(f"{who}: not available under torch.distributed (sharded banks are not supported yet)")
    if not isinstance(index, HipFlatIndex):
        raise ValueError(f"{who}: expected a HipFlatIndex, got {type(index).__name__}")
    return index


def check_n_clusters(n_clusters, ntotal: Optional[int] = None, who: str = "kmeans_fit") -> int:
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)):
        raise ValueError(f"{who}: n_clusters must be an integer, got {n_clusters!r}")
    K = int(n_clusters)
    if K < 1 or K > _lib.KMEANS_MAX_K:
        raise ValueError(f"{who}: n_clusters must be in [1, {_lib.KMEANS_MAX_K}], got {K}")
    if ntotal is not None and K > ntotal:
        raise ValueError(f"{who}: n_clusters = {K} exceeds the bank's {ntotal} rows")
    return K


def assign_rows(bank: HipFlatIndex, cent: HipFlatIndex, row0: int = 0, n: Optional[int] = None, chunk_rows: int = 0, want_dist: bool = True):
    """hb_kmeans_assign: the bank's rows row0 .. row0 + n - 1 against the centroid index -> (assign int32 [n], dist float32 [n] or None)."""
    n = bank.ntotal - int(row0) if n is None else int(n)
    dev = torch.device("cuda", bank.device)
    a = torch.empty((max(n, 0),), dtype=torch.int32, device=dev)
    d = torch.empty((max(n, 0),), dtype=torch.float32, device=dev) if want_dist else None
    _lib.check(_lib.lib().hb_kmeans_assign(bank._h, cent._h, int(row0), n, int(chunk_rows), _p(a), _p(d)), ValueError)
    return a, d


def accumulate(bank: HipFlatIndex, assign: torch.Tensor, n_clusters: int, row0: int = 0, sums: Optional[torch.Tensor] = None,
               counts: Optional[torch.Tensor] = None):
    """hb_kmeans_accumulate: (sums int64 [K, d], counts int64 [K]) of the rows row0 .. row0 + len(assign) - 1, added to `sums` / `counts` when given."""
    K = check_n_clusters(n_clusters, who="accumulate")
    dev = torch.device("cuda", bank.device)
    if assign.dtype != torch.int32 or not assign.is_cuda or assign.device != dev or assign.dim() != 1:
        raise ValueError("accumulate: assign must be a one-dimensional int32 tensor on the bank's device")
    assign = assign.contiguous()
    if sums is None:
        sums = torch.zeros((K, bank.d), dtype=torch.int64, device=dev)
    if counts is None:
        counts = torch.zeros((K,), dtype=torch.int64, device=dev)
    if (sums.dtype != torch.int64 or counts.dtype != torch.int64 or tuple(sums.shape) != (K, bank.d) or tuple(counts.shape) != (K,)
            or not sums.is_contiguous() or not counts.is_contiguous() or sums.device != dev or counts.device != dev):
        raise ValueError(f"accumulate: sums must be int64 [{K}, {bank.d}] and counts int64 [{K}], contiguous, on the bank's device")
    _lib.check(_lib.lib().hb_kmeans_accumulate(bank._h, _p(assign), int(row0), assign.numel(), K, _p(sums), _p(counts)), ValueError)
    return sums, counts


def centroids_from_sums(sums: torch.Tensor, counts: torch.Tensor, prev: torch.Tensor):
    """hb_kmeans_centroids: -> (centroids float32 [K, d], empty clusters); an empty cluster keeps its row of `prev`."""
    K, d = sums.shape
    if (sums.dtype != torch.int64 or counts.dtype != torch.int64 or prev.dtype != torch.float32 or tuple(counts.shape) != (K,)
            or tuple(prev.shape) != (K, d) or not (sums.is_cuda and counts.is_cuda and prev.is_cuda)):
        raise ValueError("centroids_from_sums: sums int64 [K, d], counts int64 [K] and prev float32 [K, d] on one GPU")
    sums, counts, prev = sums.contiguous(), counts.contiguous(), prev.contiguous()
    out = torch.empty_like(prev)
    ne = ctypes.c_int64(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(sums.device).cuda_stream)
    _lib.check(_lib.lib().hb_kmeans_centroids(_p(sums), _p(counts), int(K), int(d), _p(prev), _p(out), ctypes.byref(ne), stream), ValueError)
    return out, int(ne.value)


@dataclass
class KMeansResult:
    """centroids float32 [K, D] and counts int64 [K] (CUDA): the update of the last assignment; assignments int32 [ntotal] (CUDA) or None;
    history: one dict per iteration (changed, empty, unassigned: ints; inertia: float); n_iter; converged."""
    centroids: torch.Tensor
    counts: torch.Tensor
    assignments: Optional[torch.Tensor]
    history: list
    n_iter: int
    converged: bool
    _index: Optional[HipFlatIndex] = field(default=None, repr=False, compare=False)

    @property
    def n_clusters(self) -> int:
        return int(self.centroids.shape[0])

    def centroid_index(self) -> HipFlatIndex:
        """The cached L2 index of the centroids (fp32 kernel), built at the first call."""
        if self._index is None:
            ix = HipFlatIndex(int(self.centroids.shape[1]), 1, self.centroids.device.index)
            ix.set_fp16(0)
            ix.add(self.centroids, normalize=False)
            self._index = ix
        return self._index

    def assign(self, x: torch.Tensor, return_distances: bool = False):
        """Cluster ids int64 [n] of ALREADY NORMALISED rows x [n, D] (a CUDA tensor on the centroids' GPU): the k = 1 search on the centroid
        index -- the nearest centroid, the lower id on ties, -1 for a row with a non-finite component."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 2 or x.shape[1] != self.centroids.shape[1]:
            raise ValueError(f"KMeansResult.assign: expected a CUDA tensor [n, {self.centroids.shape[1]}]")
        ix = self.centroid_index()
        ix.use_current_stream()
        idx, dist = ix.search(x, 1)
        return (idx.view(-1), dist.view(-1)) if return_distances else idx.view(-1)

    def close(self) -> None:
        if self._index is not None:
            self._index.close()
            self._index = None


def initial_centroids(index: HipFlatIndex, n_clusters: int, init=None, seed: int = 0) -> torch.Tensor:
    """float32 [K, D] on the index's GPU: a [K, D] tensor as given, the bank's rows at the given ids, or by default the rows at
    torch.randperm(ntotal, generator=torch.Generator().manual_seed(seed))[:K] (CPU generator)."""
    K, dev = n_clusters, torch.device("cuda", index.device)
    if init is None:
        init = torch.randperm(index.ntotal, generator=torch.Generator().manual_seed(int(seed)))[:K]
    t = init if isinstance(init, torch.Tensor) else torch.as_tensor(np.asarray(init))
    if t.dim() == 2:
        if tuple(t.shape) != (K, index.d) or not t.dtype.is_floating_point:
            raise ValueError(f"kmeans_fit: init must be a float [{K}, {index.d}] tensor or {K} row ids, got {t.dtype} {tuple(t.shape)}")
        return t.detach().to(dev, torch.float32).contiguous().clone()
    if t.dim() != 1 or t.numel() != K or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"kmeans_fit: init must be a float [{K}, {index.d}] tensor or {K} integer row ids")
    ids = t.detach().to("cpu", torch.int64)
    if K and (int(ids.min()) < 0 or int(ids.max()) >= index.ntotal):
        raise ValueError(f"kmeans_fit: init row ids must lie in [0, {index.ntotal})")
    return index.reconstruct(ids.to(dev)).contiguous()


def kmeans_fit(index, n_clusters: int, init=None, seed: int = 0, max_iter: int = 20, chunk_rows: int = 0,
               return_assignments: bool = False) -> KMeansResult:
    """Lloyd's k-means on the rows of `index` (hb_kmeans_fit).  `init`: a [K, D] tensor or K row ids; default: the rows at the first K entries
    of a seeded CPU permutation.  `chunk_rows`: rows per staging chunk of the assignment (0: automatic).  ValueError for a HipMultiIndex, under
    torch.distributed, and for n_clusters outside [1, 2048] or beyond the bank's rows."""
    index = _single_index(index, "kmeans_fit")
    K = check_n_clusters(n_clusters, index.ntotal)
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"kmeans_fit: max_iter must be a positive integer, got {max_iter!r}")
    if chunk_rows < 0:
        raise ValueError("kmeans_fit: chunk_rows must not be negative")
    dev = torch.device("cuda", index.device)
    with torch.cuda.device(dev):
        index.use_current_stream()
        start = initial_centroids(index, K, init, seed)
        cent = torch.empty_like(start)
        counts = torch.empty((K,), dtype=torch.int64, device=dev)
        assign = torch.empty((index.ntotal,), dtype=torch.int32, device=dev) if return_assignments else None
        hist = (ctypes.c_double * (4 * int(max_iter)))()
        iters, conv = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.lib().hb_kmeans_fit(index._h, K, _p(start), int(max_iter), int(chunk_rows), _p(cent), _p(counts), _p(assign), hist,
                                            ctypes.byref(iters), ctypes.byref(conv)), ValueError)
    history = [{name: (float if name == "inertia" else int)(hist[4 * i + j]) for j, name in enumerate(HISTORY_FIELDS)} for i in range(iters.value)]
    return KMeansResult(cent, counts, assign, history, int(iters.value), bool(conv.value))
