"""Image-level k-NN classification (the weighted k-NN column of DINO / iBOT / DINOv2: ImageNet top-1 at k = 10 / 20 / 100 / 200, T = 0.07) on
the device: include/hbird_hip_vote.h holds the definition, which is this engine's own -- DINO's eval_knn.py restated from memory; no accuracy
of this engine has been held to a published one.

One image-level feature per image goes, normalised, into ONE inner-product `HipFlatIndex`; the class ids stay beside it in an int32 device
tensor (one integer per bank row, no dense label rows).  Per validation batch: the features normalised (`ops.normalize_rows`), ONE
`index.search` at the largest k, then `ops.knn_vote` + `ops.vote_counts` once per launch of `grid_plan(ks, temperatures)` -- a query's best k
are the first k of its best k_max and T only enters after the search, so one search serves the whole (k, T) table.  Only the count tables
reach the host.  One process, one device.

The linear-probe column stands beside it (`fit_linear_probe`, `evaluate_linear_probe`, `hbird_linear_classification`): a softmax head on the
same bank rows and class ids, include/hbird_hip_linprobe_class.h -- again this engine's own definition (L2-penalised, full-batch L-BFGS, not
DINO's SGD recipe with batch norm), with no accuracy held to a published one.
"""
from __future__ import annotations

import math
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from hbird_mi import _lib, ops
from hbird_mi.nn.search_hip import HipFlatIndex, exclude_plan, grid_plan


class KnnClassMetrics:
    """The accuracies of a (k, T) grid out of the count tables: `top1`, `topn` (the label among the first `n_top` predictions) and
    `mean_per_class` (the mean over the classes that have queries of the class's own top-1) are dicts keyed (k, T); `n` labelled queries
    were scored, `skipped` unlabelled ones (class id -1) were not -- they are counted, never dropped silently.  `best()` -> ((k, T), top1) of
    the best top-1, the first such configuration in grid order on a tie.  With n == 0 every figure is NaN."""

    def __init__(self, configs, counts, class_counts, n: int, skipped: int = 0):
        self.configs = [(int(k), float(T)) for k, T in configs]
        self.counts = np.asarray(counts, dtype=np.int64)
        self.class_counts = np.asarray(class_counts, dtype=np.int64)
        if self.counts.ndim != 2 or self.counts.shape[0] != len(self.configs) or self.counts.shape[1] < 1:
            raise ValueError(f"KnnClassMetrics: counts must be [{len(self.configs)} configurations, topn >= 1], got {self.counts.shape}")
        if self.class_counts.ndim != 3 or self.class_counts.shape[0] != len(self.configs) or self.class_counts.shape[2] != 2:
            raise ValueError(f"KnnClassMetrics: class_counts must be [{len(self.configs)}, C, 2], got {self.class_counts.shape}")
        self.n, self.skipped, self.n_top = int(n), int(skipped), int(self.counts.shape[1])
        self.top1: Dict[Tuple[int, float], float] = {}
        self.topn: Dict[Tuple[int, float], float] = {}
        self.mean_per_class: Dict[Tuple[int, float], float] = {}
        for i, key in enumerate(self.configs):
            self.top1[key] = self.counts[i, 0] / self.n if self.n else float("nan")
            self.topn[key] = self.counts[i, -1] / self.n if self.n else float("nan")
            seen = self.class_counts[i, :, 0] > 0
            self.mean_per_class[key] = float(np.mean(self.class_counts[i, seen, 1] / self.class_counts[i, seen, 0])) if seen.any() else float("nan")

    def best(self) -> Tuple[Tuple[int, float], float]:
        if not self.n:
            raise ValueError("best: no labelled query was scored")
        key = max(self.configs, key=lambda c: (self.top1[c], -self.configs.index(c)))
        return key, self.top1[key]


class LinearClassMetrics:
    """The accuracies of the image-level linear probe, one configuration per l2: `top1`, `topn` and `mean_per_class` are dicts keyed by l2
    (`KnnClassMetrics`' definitions on the same count tables); `n` labelled queries were scored, `skipped` unlabelled ones (class id -1) were
    not -- they are counted, never dropped silently; `fits[l2]` = dict(state, n_iter, rows_used, rows_skipped) of that l2's fit.  `best()` ->
    (l2, top1) of the best top-1, the first such l2 in the order given on a tie.  With n == 0 every figure is NaN."""

    def __init__(self, l2s, counts, class_counts, n: int, skipped: int, fits):
        table = KnnClassMetrics([(i, 1.0) for i in range(len(l2s))], counts, class_counts, n, skipped)
        self.l2s = [float(v) for v in l2s]
        self.counts, self.class_counts, self.n, self.skipped, self.n_top = table.counts, table.class_counts, table.n, table.skipped, table.n_top
        self.top1 = {v: table.top1[(i, 1.0)] for i, v in enumerate(self.l2s)}
        self.topn = {v: table.topn[(i, 1.0)] for i, v in enumerate(self.l2s)}
        self.mean_per_class = {v: table.mean_per_class[(i, 1.0)] for i, v in enumerate(self.l2s)}
        self.fits = {float(k): dict(v) for k, v in fits.items()}

    def best(self) -> Tuple[float, float]:
        if not self.n:
            raise ValueError("best: no labelled query was scored")
        key = max(self.l2s, key=lambda v: (self.top1[v], -self.l2s.index(v)))
        return key, self.top1[key]


def _pooled(feature_fn, pool: Optional[str]) -> Callable[[torch.Tensor], torch.Tensor]:
    """feature_fn as `imgs -> [B, D]`: a callable as it is; an extractor with `forward_features(imgs) -> (tokens [B, N, D], _)` gives the mean
    of its patch tokens (pool="mean", the only pooling there is -- CLS-token models pass their own callable)."""
    if pool not in (None, "mean"):
        raise ValueError(f"pool={pool!r}: only 'mean' (the mean of the patch tokens) is known; CLS-token models pass their own callable")
    if hasattr(feature_fn, "forward_features"):
        def mean_tokens(imgs):
            tokens, _ = feature_fn.forward_features(imgs)
            return tokens.float().mean(dim=1)
        return mean_tokens
    if pool is not None:
        raise ValueError("pool='mean' needs an extractor with forward_features; a plain callable returns [B, D] itself")
    if not callable(feature_fn):
        raise ValueError(f"feature_fn must be a callable imgs -> [B, D] or a FeatureExtractor, got {type(feature_fn).__name__}")
    return feature_fn


class HbirdKnnClassification:
    """`feature_fn(imgs [B,3,H,W]) -> [B, D]`, or a `FeatureExtractor` for the mean of its patch tokens.  `n_neighbours` and `temperatures`: a
    value or a list each, the (k, T) grid (`grid_plan`: sorted, duplicates dropped).  nn_params: use_fp16 / fp16_centre / rerank_copy as
    for the other evaluators; an L2 distance_measure is refused -- the weights are defined on cosine similarities -- and so are idx_shard
    and several gpu_ids (one HipFlatIndex, no HipMultiIndex)."""

    def __init__(self, feature_fn, num_classes: int, n_neighbours=(10, 20, 100, 200), temperatures=(0.07,), topn: int = 5,
                 nn_params: Optional[Dict[str, Any]] = None, device: torch.device | str = "cuda", pool: Optional[str] = None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= _lib.VOTE_MAX_CLASSES:
            raise ValueError(f"num_classes={num_classes!r} must be an integer in [1, {_lib.VOTE_MAX_CLASSES}]")
        if isinstance(topn, bool) or not isinstance(topn, (int, np.integer)) or not 1 <= int(topn) <= _lib.VOTE_MAX_TOP:
            raise ValueError(f"topn={topn!r} must be an integer in [1, {_lib.VOTE_MAX_TOP}]")
        self.plan = grid_plan(n_neighbours, temperatures, max_configs=_lib.VOTE_MAX_CONFIGS)      # (its betas are the temperatures here)
        nn_params = dict(nn_params or {})
        distance = str(nn_params.get("distance_measure", "dot_product")).lower()
        if distance != "dot_product":
            raise ValueError(f"distance_measure={distance!r} is not available for k-NN classification: the vote's weights exp(sim / T) are defined "
                             "on cosine similarities (normalised rows, inner product)")
        if nn_params.get("idx_shard", False):
            raise ValueError("HbirdKnnClassification: nn_params['idx_shard'] is not available (one HipFlatIndex, no HipMultiIndex)")
        gpu_ids = nn_params.get("gpu_ids")
        if gpu_ids is not None and len(gpu_ids) != 1:
            raise ValueError("HbirdKnnClassification: nn_params['gpu_ids'] must name one GPU (one HipFlatIndex, no HipMultiIndex)")
        self.nn_params, self.num_classes, self.n_top = nn_params, int(num_classes), int(topn)
        self.feature_fn = _pooled(feature_fn, pool)
        self.device = device
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device={device!r}: the k-NN classification runs on a GPU")
        if not torch.cuda.is_available():
            raise RuntimeError("HbirdKnnClassification needs an MI355X: the HIP path has no CPU fallback")
        self.gpu = dev.index if dev.index is not None else torch.cuda.current_device()
        if gpu_ids is not None and int(gpu_ids[0]) != self.gpu:
            raise ValueError(f"HbirdKnnClassification: nn_params['gpu_ids']={list(gpu_ids)} and device={device!r} name different GPUs")
        self.gpu_device = torch.device("cuda", self.gpu)
        if isinstance(feature_fn, torch.nn.Module):
            feature_fn.to(self.gpu_device).eval()
        self.index: Optional[HipFlatIndex] = None
        self.labels: Optional[torch.Tensor] = None            # int32 [ntotal] on the device: the class of every bank row, -1 = unlabelled
        self.row_groups: Optional[torch.Tensor] = None        # int32 [ntotal] (CPU): the dataset image of every bank row, where known
        self.n_images, self.augmentation_epoch = 0, 1

    @property
    def ks(self) -> Tuple[int, ...]:
        return self.plan.ks

    @property
    def temperatures(self) -> Tuple[float, ...]:
        return self.plan.betas

    # ---- the bank ----------------------------------------------------------------------------------------------------------------------------
    def _new_index(self, d: int) -> HipFlatIndex:
        index = HipFlatIndex(int(d), 0, self.gpu)             # inner product
        if self.nn_params.get("use_fp16", False):
            index.set_fp16(2)
            index.set_rerank_copy(int(self.nn_params.get("rerank_copy", 0)))
        if self.nn_params.get("fp16_centre", False):
            index.set_fp16_centre(True)
        return index

    def _features(self, x: torch.Tensor) -> torch.Tensor:
        f = self.feature_fn(x.to(self.gpu_device))
        if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] != x.shape[0]:
            raise ValueError(f"feature_fn returned {tuple(getattr(f, 'shape', ()))} for {x.shape[0]} images: expected [B, D] (one feature per image)")
        return f.to(self.gpu_device, dtype=torch.float32).contiguous()

    def _class_ids(self, y, who: str) -> torch.Tensor:
        y = torch.as_tensor(y).detach().reshape(-1).cpu()
        if y.numel() and (y.dtype.is_floating_point or y.dtype == torch.bool):
            raise ValueError(f"{who}: class ids must be integers, got {y.dtype}")
        if y.numel() and (int(y.min()) < -1 or int(y.max()) >= self.num_classes):
            raise ValueError(f"{who}: a class id lies outside [-1, {self.num_classes}) (-1: unlabelled)")
        return y.to(torch.int32)

    def build(self, train_loader, augmentation_epoch: int = 1) -> "HbirdKnnClassification":
        """Fills the bank: one normalised row per (epoch, image), its class id beside it, one row group per dataset image (the i-th image of
        every epoch's pass is image i)."""
        if isinstance(augmentation_epoch, bool) or not isinstance(augmentation_epoch, int) or augmentation_epoch < 1:
            raise ValueError(f"augmentation_epoch={augmentation_epoch!r} must be an integer >= 1")
        if self.index is not None:
            raise ValueError("build: this classifier already holds a bank")
        labels, groups, n_images = [], [], 0
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for _ in range(augmentation_epoch):
                seen = 0
                for x, y in train_loader:
                    y = self._class_ids(y, "build")
                    feats = self._features(x)
                    if y.numel() != feats.shape[0]:
                        raise ValueError(f"build: {y.numel()} class ids for {feats.shape[0]} images")
                    if self.index is None:
                        self.index = self._new_index(feats.shape[1])
                    self.index.use_current_stream()
                    self.index.add(feats, normalize=True)
                    labels.append(y)
                    groups.append(torch.arange(seen, seen + y.numel(), dtype=torch.int32))
                    seen += y.numel()
                n_images = max(n_images, seen)
            if self.index is None:
                raise ValueError("build: the training loader is empty")
            self.labels = torch.cat(labels).to(self.gpu_device)
            self.row_groups, self.n_images, self.augmentation_epoch = torch.cat(groups), n_images, augmentation_epoch
            self.index.set_row_groups(self.row_groups, n_images)
            torch.cuda.synchronize(self.gpu_device)
        return self

    @classmethod
    def from_index(cls, index, labels, feature_fn, num_classes: int, n_neighbours=(10, 20, 100, 200), temperatures=(0.07,), topn: int = 5,
                   row_groups=None, device: torch.device | str = "cuda", pool: Optional[str] = None) -> "HbirdKnnClassification":
        """A classifier over a bank that is already resident: `index` an inner-product `HipFlatIndex` of normalised rows, `labels` its class
        ids ([ntotal] integers, -1 = unlabelled).  `row_groups` ([ntotal] integers: the dataset image of every row) makes leave-one-out and
        `memory_view(images=)` available; nothing is built."""
        if not isinstance(index, HipFlatIndex):
            raise ValueError(f"from_index: index must be a HipFlatIndex, got {type(index).__name__} (HipMultiIndex is not available)")
        if index.metric != 0:
            raise ValueError("from_index: the index must be an inner-product index: the vote's weights are defined on cosine similarities")
        self = cls(feature_fn, num_classes, n_neighbours, temperatures, topn, None, device, pool)
        if index.device != self.gpu:
            raise ValueError(f"from_index: the index lives on GPU {index.device}, device={device!r} names GPU {self.gpu}")
        y = self._class_ids(labels, "from_index")
        if y.numel() != index.ntotal:
            raise ValueError(f"from_index: {y.numel()} class ids for a bank of {index.ntotal} rows")
        self.index, self.labels = index, y.to(self.gpu_device)
        if row_groups is not None:
            g = torch.as_tensor(row_groups).detach().reshape(-1).cpu()
            if g.numel() != index.ntotal or (g.numel() and (g.dtype.is_floating_point or g.dtype == torch.bool)):
                raise ValueError(f"from_index: row_groups must be {index.ntotal} integers")
            self.row_groups, self.n_images = g.to(torch.int32), int(g.max()) + 1 if g.numel() else 0
            with torch.cuda.device(self.gpu_device):
                index.use_current_stream()
                index.set_row_groups(self.row_groups, self.n_images)
        return self

    def memory_view(self, images=None, rows=None) -> "HbirdKnnClassification":
        """A classifier on the gathered rows of this bank and their labels (`select_rows`: 1 % / 10 % label subsets out of one build).
        `images=`: the dataset images to keep -- every row of theirs, in bank order; `rows=`: the bank rows themselves, in the order given.
        The view's rows keep their images (leave-one-out)."""
        if self.index is None:
            raise ValueError("memory_view: the bank is empty (build first)")
        if (images is None) == (rows is None):
            raise ValueError("memory_view: give images= or rows=, one of them")
        if images is not None:
            if self.row_groups is None:
                raise ValueError("memory_view: images= needs the image of every row (a bank built here, or from_index(row_groups=))")
            keep = torch.as_tensor(images, dtype=torch.int64).reshape(-1)
            if keep.numel() and (int(keep.min()) < 0 or int(keep.max()) >= self.n_images):
                raise ValueError(f"memory_view: an image lies outside [0, {self.n_images})")
            ids = torch.nonzero(torch.isin(self.row_groups.to(torch.int64), keep)).reshape(-1)
        else:
            ids = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
        if not ids.numel():
            raise ValueError("memory_view: no row is kept")
        with torch.cuda.device(self.gpu_device):
            self.index.use_current_stream()
            index = self.index.select_rows(ids)               # (ValueError for a row outside the bank)
        view = HbirdKnnClassification.from_index(index, self.labels[ids.to(self.gpu_device)].cpu(), self.feature_fn, self.num_classes, self.plan.ks,
                                                 self.plan.betas, self.n_top, None if self.row_groups is None else self.row_groups[ids], self.device)
        view.n_images, view.augmentation_epoch = self.n_images, self.augmentation_epoch
        return view

    # ---- evaluation --------------------------------------------------------------------------------------------------------------------------
    def _pass(self, who: str, loader, limit: Optional[int] = None, cut: bool = False) -> KnnClassMetrics:
        if self.index is None or self.index.ntotal == 0:
            raise ValueError(f"{who}: the bank is empty")
        excluding = limit is not None
        plan, C, topn = self.plan, self.num_classes, self.n_top
        kmax = plan.ks[-1]
        parts = []                                            # per launch of the grid: its count tables
        for ks_part, temps_part, rows in plan.launches:
            n_cfg = len(rows)
            parts.append((ks_part, temps_part, rows, torch.zeros((n_cfg, topn), dtype=torch.int64, device=self.gpu_device),
                          torch.zeros(1, dtype=torch.int64, device=self.gpu_device),
                          torch.zeros((n_cfg, C, 2), dtype=torch.int64, device=self.gpu_device)))
        seen = 0
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for x, y in loader:
                if excluding and cut and seen >= limit:
                    break
                if excluding and cut and seen + x.shape[0] > limit:
                    x, y = x[:limit - seen], y[:limit - seen]
                if excluding and seen + x.shape[0] > limit:
                    raise ValueError(f"{who}: the loader yields more than the {limit} images the bank was built from (it must yield the bank's "
                                     "images, in the order of the build pass)")
                qlab = self._class_ids(y, who).to(self.gpu_device)
                q = ops.normalize_rows(self._features(x))
                if qlab.numel() != q.shape[0]:
                    raise ValueError(f"{who}: {qlab.numel()} class ids for {q.shape[0]} images")
                self.index.use_current_stream()
                if excluding:
                    qgroups = torch.arange(seen, seen + q.shape[0], dtype=torch.int32, device=self.gpu_device)
                    idx, score = self.index.search_excluding(q, kmax, qgroups)
                else:
                    idx, score = self.index.search(q, kmax)   # ONE search: every k is a prefix of its lists, T enters after it
                seen += q.shape[0]
                for ks_part, temps_part, _, counts, n, per_class in parts:
                    pred = ops.knn_vote(idx, score, self.labels, C, ks_part, temps_part, topn=topn)
                    ops.vote_counts(pred, qlab, C, counts, n, per_class)
        if not seen:
            raise ValueError(f"{who}: the loader is empty")
        counts = np.zeros((len(plan.configs), topn), dtype=np.int64)
        per_class = np.zeros((len(plan.configs), C, 2), dtype=np.int64)
        for _, _, rows, c, _, pc in parts:
            counts[rows], per_class[rows] = c.cpu().numpy(), pc.cpu().numpy()
        n = int(parts[0][4].item())
        return KnnClassMetrics(plan.configs, counts, per_class, n, seen - n)

    def evaluate(self, val_loader) -> KnnClassMetrics:
        """Every (k, T) of the grid out of ONE pass over the loader and one search per batch."""
        return self._pass("evaluate", val_loader)

    def evaluate_leave_one_out(self, train_loader, max_images: Optional[int] = None) -> KnnClassMetrics:
        """`evaluate` of the bank ON ITS OWN TRAINING IMAGES: `train_loader` yields the bank's images in the order of the build pass, the
        i-th image seen queries with group i and its search excludes every bank row of that image (`search_excluding`) -- so (k, T) can be
        chosen on the training split.  `max_images`: stop after that many images.  ValueError, in `exclude_plan`'s words, when the largest
        k + the rows of the largest image (the epochs of the build) exceeds 2048, and for a bank whose rows' images are not known."""
        if max_images is not None and int(max_images) < 1:
            raise ValueError("evaluate_leave_one_out: max_images must be positive")
        if self.index is None or self.index.ntotal == 0:
            raise ValueError("evaluate_leave_one_out: the bank is empty")
        if self.row_groups is None:
            raise ValueError("evaluate_leave_one_out: the image of every bank row is not known (from_index without row_groups=)")
        g = self.row_groups[self.row_groups >= 0].to(torch.int64)
        gmax = int(torch.bincount(g).max()) if g.numel() else 0
        exclude_plan(self.plan.ks[-1], gmax)                  # ValueError: k + the largest group beyond 2048
        limit = self.n_images if max_images is None else min(self.n_images, int(max_images))
        return self._pass("evaluate_leave_one_out", train_loader, limit=limit, cut=max_images is not None)

    # ---- the linear probe (include/hbird_hip_linprobe_class.h) ------------------------------------------------------------------------------
    def fit_linear_probe(self, l2: float = 1e-3, gtol: float = 1e-5, max_iter: int = 200, Wb0=None):
        """`linear_probe.linear_probe_fit_classes` on the bank's rows and `self.labels`: a softmax head with an L2 penalty on the normalised
        features, by full-batch L-BFGS (this engine's own definition -- not DINO's SGD recipe with batch norm; no accuracy has been held to
        a published one).  Rows of label -1 take no part.  -> `LinearProbe`; the caller closes it."""
        from hbird_mi.linear_probe import linear_probe_fit_classes
        if self.index is None or self.index.ntotal == 0:
            raise ValueError("fit_linear_probe: the bank is empty")
        with torch.cuda.device(self.gpu_device):
            return linear_probe_fit_classes(self.index, self.labels, self.num_classes, l2=l2, gtol=gtol, max_iter=max_iter, Wb0=Wb0)

    def evaluate_linear_probe(self, val_loader, l2s=(1e-3,), gtol: float = 1e-5, max_iter: int = 200) -> LinearClassMetrics:
        """The linear-probe column beside `evaluate`'s k-NN column.  One head per l2 (at most 16, duplicates refused) is fitted on the bank,
        in DESCENDING l2 order, each warm-started from the one before; then ONE pass over the loader scores them all: per batch
        each probe's `logits(features)` (`ops.normalize_rows`, then the logits entry) -> `ops.logits_topn` -> `ops.vote_counts`.  Only the count tables reach the host.
        A `memory_view(...)` is an ordinary instance, so label-subset probes need no code; choosing l2 on a held-out part of the training
        split is `memory_view(images=kept).evaluate_linear_probe(loader_of_the_other_images, l2s=...)`."""
        who = "evaluate_linear_probe"
        l2s = [float(v) for v in (l2s if isinstance(l2s, (list, tuple)) else [l2s])]
        if not l2s or len(l2s) > _lib.VOTE_MAX_CONFIGS or len(set(l2s)) != len(l2s) or not all(np.isfinite(v) and v >= 0 for v in l2s):
            raise ValueError(f"{who}: l2s must be 1 to {_lib.VOTE_MAX_CONFIGS} different non-negative numbers, got {l2s}")
        if self.index is None or self.index.ntotal == 0:
            raise ValueError(f"{who}: the bank is empty")
        C, topn = self.num_classes, self.n_top
        probes, fits, warm = {}, {}, None
        try:
            for v in sorted(l2s, reverse=True):
                probes[v] = self.fit_linear_probe(l2=v, gtol=gtol, max_iter=max_iter, Wb0=warm)
                warm = probes[v].Wb
                fits[v] = dict(state=probes[v].state, n_iter=probes[v].n_iter, rows_used=probes[v].rows_used, rows_skipped=probes[v].rows_skipped)
            counts = torch.zeros((len(l2s), topn), dtype=torch.int64, device=self.gpu_device)
            per_class = torch.zeros((len(l2s), C, 2), dtype=torch.int64, device=self.gpu_device)
            n = torch.zeros(1, dtype=torch.int64, device=self.gpu_device)
            seen = 0
            with torch.no_grad(), torch.cuda.device(self.gpu_device):
                for x, y in val_loader:
                    qlab = self._class_ids(y, who).to(self.gpu_device)
                    q = self._features(x)                    # (`LinearProbe.logits` normalises the rows: `ops.normalize_rows`, once)
                    if qlab.numel() != q.shape[0]:
                        raise ValueError(f"{who}: {qlab.numel()} class ids for {q.shape[0]} images")
                    seen += q.shape[0]
                    pred = torch.stack([ops.logits_topn(probes[v].logits(q), topn) for v in l2s])      # [n_cfg, nq, topn]: one configuration per l2
                    ops.vote_counts(pred, qlab, C, counts, n, per_class)
            if not seen:
                raise ValueError(f"{who}: the loader is empty")
            return LinearClassMetrics(l2s, counts.cpu().numpy(), per_class.cpu().numpy(), int(n.item()), seen - int(n.item()), fits)
        finally:
            for probe in probes.values():
                probe.close()

    def close(self) -> None:
        if self.index is not None:
            self.index.close()


last_run_info: Dict[str, Any] = {}


def hbird_knn_classification(model, d_model: int, patch_size: int, dataset_name: str, data_dir: str, batch_size: int = 64, input_size: int = 224,
                             augmentation_epoch: int = 1, device: str | torch.device = "cuda", n_neighbours=(10, 20, 100, 200),
                             temperatures=(0.07,), topn: int = 5, nn_params: Optional[Dict[str, Any]] = None, ftr_extr_fn=None, feature_fn=None,
                             num_workers: int = 8, leave_one_out: bool = False, leave_one_out_images: Optional[int] = None) -> KnnClassMetrics:
    """The function form: dataset_name "synthetic-classify[*frac]" or "class-folder[*frac]" (hbird_mi/data/classify.py).  The image-level
    feature is `feature_fn(imgs) -> [B, D]` where given, else the mean of the patch tokens of the model wrapped as `hbird_evaluation` wraps it.
    With `leave_one_out` the bank is scored on its own training images instead of the validation split."""
    from hbird_mi.data.classify import get_classify_dataset
    from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
    if leave_one_out_images is not None and not leave_one_out:
        raise ValueError("leave_one_out_images needs leave_one_out")
    dataset = get_classify_dataset(dataset_name, data_dir, batch_size, num_workers, input_size)
    if feature_fn is None:
        S = max(1, int(input_size) // int(patch_size))
        if ftr_extr_fn is None:
            feature_fn = FeatureExtractor(model, eval_spatial_resolution=S, d_model=d_model)
        else:
            feature_fn = FeatureExtractorSimple(model, ftr_extr_fn=ftr_extr_fn, eval_spatial_resolution=S, d_model=d_model)
    ev = HbirdKnnClassification(feature_fn, dataset.get_num_classes(), n_neighbours=n_neighbours, temperatures=temperatures, topn=topn,
                                nn_params=nn_params, device=device)
    try:
        ev.build(dataset.train_dataloader(), augmentation_epoch=augmentation_epoch)
        last_run_info.clear()
        last_run_info.update(bank_rows=int(ev.index.ntotal), num_classes=int(ev.num_classes))
        if leave_one_out:
            return ev.evaluate_leave_one_out(dataset.train_dataloader(), max_images=leave_one_out_images)
        return ev.evaluate(dataset.val_dataloader())
    finally:
        ev.close()


def hbird_linear_classification(model, d_model: int, patch_size: int, dataset_name: str, data_dir: str, batch_size: int = 64, input_size: int = 224,
                                augmentation_epoch: int = 1, device: str | torch.device = "cuda", l2s=(1e-3,), gtol: float = 1e-5,
                                max_iter: int = 200, topn: int = 5, nn_params: Optional[Dict[str, Any]] = None, ftr_extr_fn=None,
                                feature_fn=None, num_workers: int = 8) -> LinearClassMetrics:
    """The function form of `HbirdKnnClassification.evaluate_linear_probe`: datasets and features as `hbird_knn_classification` takes them; one
    softmax head per l2, fitted on the bank of training images and scored on the validation split."""
    from hbird_mi.data.classify import get_classify_dataset
    from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
    dataset = get_classify_dataset(dataset_name, data_dir, batch_size, num_workers, input_size)
    if feature_fn is None:
        S = max(1, int(input_size) // int(patch_size))
        if ftr_extr_fn is None:
            feature_fn = FeatureExtractor(model, eval_spatial_resolution=S, d_model=d_model)
        else:
            feature_fn = FeatureExtractorSimple(model, ftr_extr_fn=ftr_extr_fn, eval_spatial_resolution=S, d_model=d_model)
    ev = HbirdKnnClassification(feature_fn, dataset.get_num_classes(), n_neighbours=(1,), topn=topn, nn_params=nn_params, device=device)
    try:
        ev.build(dataset.train_dataloader(), augmentation_epoch=augmentation_epoch)
        last_run_info.clear()
        last_run_info.update(bank_rows=int(ev.index.ntotal), num_classes=int(ev.num_classes))
        return ev.evaluate_linear_probe(dataset.val_dataloader(), l2s=l2s, gtol=gtol, max_iter=max_iter)
    finally:
        ev.close()
