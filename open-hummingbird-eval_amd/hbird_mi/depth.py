"""Depth estimation by retrieval: the Hummingbird evaluation's second task (monocular depth, e.g. NYUv2) on the engine of the first.

The bank is an ordinary `HipFlatIndex` whose label rows are fp32 values -- per cell of a patch the sum of its valid depths and its valid
share, both over the cell's area (`ops.patch_depth_targets`, include/hbird_hip_depth.h).  A query's neighbours are combined by the same
cosine-softmax (`search_aggregate`, K5 unchanged: the certified fp16 screen, memory views and bounded sampling all apply), and
`ops.depth_upsample_metrics` turns the aggregated rows into a depth map -- the ratio of the two bilinearly upsampled grids, clamped -- and
deterministic per-image error sums, which `finish_metrics` turns into rmse, abs_rel, sq_rel, rmse_log, silog, log10, d1, d2, d3.
`evaluate` scores one (k, beta) per pass; `evaluate_grid` / `evaluate_leave_one_out` score a whole grid -- and the memory views of one bank --
from one search per batch (`ops.depth_upsample_metrics_grid`, include/hbird_hip_depth_grid.h), and `DepthBootstrap` carries paired bootstrap
replicates over the images (`ops.bootstrap_weighted_sums`).

No dataset is bundled and no figure of this module has been held to a published one.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from hbird_mi import _lib, ops, views
from hbird_mi import bootstrap as hboot
from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
from hbird_mi.nn.search_hip import HipFlatIndex, _METRICS, check_k, k5

METRICS = ("rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "log10", "d1", "d2", "d3")
SENTINEL = 1e6          # the bounded build's score of an empty patch (the reference's, hbird_eval.py:493)
last_run_info: Dict[str, Any] = {}


def finish_image(s) -> Optional[Dict[str, float]]:
    """One float64 row of sums (the order of `_lib.DEPTH_SUMS`) -> the metrics, None when no pixel was scored (n == 0).
    silog is Eigen's scale-invariant log error with lambda = 1, sqrt(mean(dl^2) - mean(dl)^2), not multiplied by 100."""
    s = [float(v) for v in s]
    n = s[0]
    if n <= 0:
        return None
    return {"rmse": math.sqrt(s[2] / n), "abs_rel": s[3] / n, "sq_rel": s[4] / n, "rmse_log": math.sqrt(s[5] / n),
            "silog": math.sqrt(max(0.0, s[5] / n - (s[6] / n) ** 2)), "log10": s[7] / n, "d1": s[8] / n, "d2": s[9] / n, "d3": s[10] / n}


class DepthMetrics(dict):
    """The headline metrics: the mean over images with n > 0 of the per-image metrics (the depth literature's convention); NaN when there is
    no such image.  `.per_image` (None for an image with n == 0), `.pooled` (the metrics of the summed sums, None when nothing was scored),
    `.n_nopred` (valid ground-truth pixels without a prediction), `.empty_images` (the images with n == 0: reported, never dropped silently),
    `.sums` (float64 [n_img, 11]: the input a bootstrap needs), `.maps` (the predictions, with return_maps)."""

    def __init__(self, sums: np.ndarray, maps: Optional[List[torch.Tensor]] = None):
        sums = np.asarray(sums, dtype=np.float64).reshape(-1, _lib.DEPTH_NSUMS)
        self.sums = sums
        self.per_image = [finish_image(s) for s in sums]
        kept = [m for m in self.per_image if m is not None]
        super().__init__({k: (float(np.mean([m[k] for m in kept])) if kept else float("nan")) for k in METRICS})
        self.pooled = finish_image(sums.sum(0)) if len(sums) else None
        self.n_nopred = int(sums[:, 1].sum())
        self.n_pixels = int(sums[:, 0].sum())
        self.empty_images = [i for i, m in enumerate(self.per_image) if m is None]
        self.maps = maps


def finish_metrics(sums) -> DepthMetrics:
    return DepthMetrics(sums)


def _check_bounds(min_depth, max_depth):
    lo, hi = float(min_depth), float(max_depth)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f"min_depth={min_depth!r}, max_depth={max_depth!r}: the bounds must be finite with 0 < min_depth <= max_depth")
    return lo, hi


def _check_grid(target_grid) -> int:
    if isinstance(target_grid, bool) or not isinstance(target_grid, (int, np.integer)) or target_grid < 1:
        raise ValueError(f"target_grid={target_grid!r} must be a positive integer (a divisor of the patch size)")
    return int(target_grid)


def _depth_maps(y: torch.Tensor, device) -> torch.Tensor:
    """A loader's depth batch, [B,1,H,W] or [B,H,W], as contiguous float32 [B,H,W] on the GPU."""
    if y.dim() == 4 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 3:
        raise ValueError(f"a depth batch must be [B,1,H,W] or [B,H,W], got {tuple(y.shape)}")
    return y.to(device=device, dtype=torch.float32).contiguous()


class HbirdDepthEvaluation:
    """Build a depth bank from `train_loader` and evaluate validation images against it.  One `HipFlatIndex` only: several GPUs
    (nn_params gpu_ids / idx_shard -> HipMultiIndex) and torch.distributed raise ValueError.

    `memory_size` (with `dataset_size`): the reference's bounded memory -- per (epoch, image) K = memory_size // (dataset_size * epochs)
    patches; every non-empty patch (any valid pixel) scores 1, an empty one the sentinel 1e6, the score is multiplied by a uniform draw from
    torch's CPU generator in the reference's order (one `torch.rand(non-empty patches of the batch)` per batch), the K smallest are kept in
    ascending order (`ops.patch_select`).  Unbounded: every patch of every image, S x S rows per image."""

    def __init__(self, feature_extractor: torch.nn.Module, train_loader, n_neighbours: int = 30, beta: float = 0.02, target_grid: int = 1,
                 min_depth: float = 1e-3, max_depth: float = 10.0, augmentation_epoch: int = 1, device: torch.device | str = "cuda",
                 nn_params: Optional[Dict[str, Any]] = None, memory_size: Optional[int] = None, dataset_size: Optional[int] = None) -> None:
        nn_params = dict(nn_params or {})
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise ValueError("HbirdDepthEvaluation: torch.distributed is not available for depth (one process, one GPU)")
        if nn_params.get("idx_shard", False):
            raise ValueError("HbirdDepthEvaluation: nn_params['idx_shard'] is not available for depth (one HipFlatIndex, no HipMultiIndex)")
        gpu_ids = nn_params.get("gpu_ids")
        if gpu_ids is not None and len(gpu_ids) != 1:
            raise ValueError("HbirdDepthEvaluation: nn_params['gpu_ids'] must name one GPU for depth (one HipFlatIndex, no HipMultiIndex)")
        if memory_size is not None and dataset_size is None:
            raise ValueError("dataset_size must be provided when memory_size is set.")
        self._common(feature_extractor, n_neighbours, beta, target_grid, min_depth, max_depth, device)
        if gpu_ids is not None and int(gpu_ids[0]) != self.gpu:
            raise ValueError(f"HbirdDepthEvaluation: nn_params['gpu_ids']={list(gpu_ids)} and device={device!r} name different GPUs")
        distance = str(nn_params.get("distance_measure", "dot_product")).lower()
        if distance not in _METRICS:
            raise ValueError(f"Unsupported distance measure: {distance}")
        self.nn_params = nn_params
        self.augmentation_epoch = int(augmentation_epoch)
        self.memory_size, self._dataset_size = memory_size, dataset_size
        self.num_sampled_features: Optional[int] = None
        if memory_size is not None:
            self.num_sampled_features = views.per_image_rows(memory_size, dataset_size, self.augmentation_epoch)
        self.index = HipFlatIndex(self.feature_extractor.d_model, _METRICS[distance], self.gpu)
        self.index.set_label_denominator(0)                   # fp32 label rows
        self.index.set_num_classes(2 * self.target_grid ** 2)
        if nn_params.get("use_fp16", False):
            self.index.set_fp16(2)
            self.index.set_rerank_copy(int(nn_params.get("rerank_copy", 0)))
        if nn_params.get("fp16_centre", False):
            self.index.set_fp16_centre(True)
        self._bank_block_starts: Optional[List[int]] = [0]
        self.sampled_patches: List[torch.Tensor] = []         # bounded build: the patch ids kept per batch, [bs, K] (CPU)
        t0 = time.perf_counter()
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            self._create_memory(train_loader)
            torch.cuda.synchronize(self.gpu_device)
        self.bank_build_s = time.perf_counter() - t0

    def _common(self, feature_extractor, n_neighbours, beta, target_grid, min_depth, max_depth, device):
        check_k(n_neighbours, "n_neighbours")
        if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not (math.isfinite(beta) and beta > 0):
            raise ValueError(f"beta={beta!r}: the softmax temperature must be a finite positive number")
        self.n_neighbours, self.beta = int(n_neighbours), float(beta)
        self.target_grid = _check_grid(target_grid)
        self.min_depth, self.max_depth = _check_bounds(min_depth, max_depth)
        self.device = device
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device={device!r}: the depth evaluation runs on a GPU")
        if not torch.cuda.is_available():
            raise RuntimeError("HbirdDepthEvaluation needs an MI355X: the HIP path has no CPU fallback")
        self.gpu = dev.index if dev.index is not None else torch.cuda.current_device()
        self.gpu_device = torch.device("cuda", self.gpu)
        self.feature_extractor = feature_extractor.to(self.gpu_device).eval()
        self._row_groups: Optional[torch.Tensor] = None       # leave-one-out: the image of every bank row where the caller gave it (set_row_groups) ...
        self._loo_images: Optional[int] = None                # ... or a memory_view inherited it, with the image count of the bank it was cut from
        self._row_groups_on_index = False
        self.loo_screen_served = 0

    @classmethod
    def from_index(cls, feature_extractor: torch.nn.Module, index, n_neighbours: int = 30, beta: float = 0.02, target_grid: int = 1,
                   min_depth: float = 1e-3, max_depth: float = 10.0, device: torch.device | str = "cuda") -> "HbirdDepthEvaluation":
        """An evaluator over a depth bank that is already resident in a `HipFlatIndex` (rows and 2 r^2-channel fp32 label rows added by the
        caller, a `select_rows` view, a saved bank added back): nothing is built."""
        if not isinstance(index, HipFlatIndex):
            raise ValueError(f"from_index: index must be a HipFlatIndex, got {type(index).__name__} (HipMultiIndex is not available for depth)")
        self = cls.__new__(cls)
        self._common(feature_extractor, n_neighbours, beta, target_grid, min_depth, max_depth, device)
        if index.device != self.gpu:
            raise ValueError(f"from_index: the index lives on GPU {index.device}, device={device!r} names GPU {self.gpu}")
        if index.label_denominator != 0:
            raise ValueError("from_index: a depth bank holds fp32 label rows (label denominator 0)")
        self.index = index
        self.index.set_num_classes(2 * self.target_grid ** 2)
        self.nn_params, self.augmentation_epoch, self.memory_size, self._dataset_size = {}, 1, None, None
        self.num_sampled_features, self._bank_block_starts, self.sampled_patches, self.bank_build_s = None, None, [], 0.0
        return self

    # ---- bank build ------------------------------------------------------------------------------------------------------------------------
    def _tokens(self, x: torch.Tensor) -> torch.Tensor:
        feats, _ = self.feature_extractor.forward_features(x.to(self.gpu_device))
        return feats.to(self.gpu_device, dtype=torch.float32).contiguous()

    def _create_memory(self, train_loader) -> None:
        S = self.feature_extractor.eval_spatial_resolution
        C2 = 2 * self.target_grid ** 2
        for _ in range(self.augmentation_epoch):
            for x, y in train_loader:
                y = _depth_maps(y, self.gpu_device)
                bs, H, W = y.shape
                if H != W or H % S or x.shape[-1] != H:
                    raise ValueError(f"training batches must be square with a side that is a multiple of {S} patches, got image {tuple(x.shape)} depth {tuple(y.shape)}")
                ps = H // S
                if ps % self.target_grid:
                    raise ValueError(f"target_grid={self.target_grid} does not divide the patch size {ps}")
                rows, nonempty = ops.patch_depth_targets(y, ps, self.target_grid, self.min_depth, self.max_depth)
                feats = self._tokens(x)
                D = feats.shape[-1]
                self.index.use_current_stream()
                if self.memory_size is None:
                    self.index.add(feats.reshape(-1, D), normalize=True)
                    self.index.add_labels(rows.reshape(-1, C2))
                    kept = S * S
                else:
                    K = int(self.num_sampled_features)
                    ne = nonempty.reshape(bs, S * S)
                    nz_host = ne.sum(1).cpu().tolist()
                    total_nz = int(sum(nz_host))
                    r = torch.rand(total_nz) if total_nz > 0 else torch.zeros(0)        # the CPU stream, one draw per non-empty patch in batch order
                    r_off = torch.tensor([0] + nz_host[:-1], dtype=torch.int64).cumsum(0)
                    scores = torch.where(ne != 0, torch.ones((), device=ne.device), torch.full((), SENTINEL, device=ne.device)).float().contiguous()
                    sidx = ops.patch_select(scores, ne.contiguous(), r.to(self.gpu_device), r_off.to(self.gpu_device), K)
                    self.sampled_patches.append(sidx.cpu())
                    pick = (sidx + torch.arange(bs, device=sidx.device)[:, None] * (S * S)).reshape(-1)
                    self.index.add(ops.gather_rows(feats.reshape(-1, D), pick), normalize=True)
                    self.index.add_labels(ops.gather_rows(rows.reshape(-1, C2), pick))
                    kept = K
                last = self._bank_block_starts[-1]
                self._bank_block_starts.extend(last + kept * (i + 1) for i in range(bs))

    def memory_view(self, memory_size: int) -> "HbirdDepthEvaluation":
        """The bank a bounded build at a smaller `memory_size` would hold -- the first K_m rows of every (epoch, image) block, as
        `HbirdEvaluation.memory_view` (hbird_mi/views.py) -- as a new evaluator made the `from_index` way."""
        if self.memory_size is None or self._bank_block_starts is None:
            raise ValueError("memory_view: memory_size= needs a bank built here, bounded (with memory_size set)")
        per_block = views.per_image_rows(int(memory_size), self._dataset_size, self.augmentation_epoch)
        if per_block > int(self.num_sampled_features):
            raise ValueError(f"memory_view: memory_size={memory_size} keeps {per_block} rows per image, the bank was built with {self.num_sampled_features}")
        ids = views.view_rows(self._bank_block_starts, per_block=per_block)
        with torch.cuda.device(self.gpu_device):
            self.index.use_current_stream()
            index = self.index.select_rows(ids)
        view = HbirdDepthEvaluation.from_index(self.feature_extractor, index, self.n_neighbours, self.beta, self.target_grid, self.min_depth,
                                               self.max_depth, self.device)
        view._row_groups = self.row_groups()[torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu()]      # the view's rows keep their images (leave-one-out)
        view._loo_images = self._leave_one_out_images()
        return view

    # ---- leave-one-image-out: which image a bank row came from (HbirdEvaluation's protocol, hbird_eval.py) --------------------------------------
    def set_row_groups(self, groups) -> None:
        """The dataset image of every bank row, given by the caller (int tensor [ntotal], -1 = no image): for a `from_index` bank, which has no
        build geometry to derive it from."""
        g = torch.as_tensor(groups).detach().reshape(-1).cpu()
        if g.numel() and (g.dtype.is_floating_point or g.dtype == torch.bool):
            raise ValueError(f"set_row_groups: groups must be integers, got {g.dtype}")
        if g.numel() != self.index.ntotal:
            raise ValueError(f"set_row_groups: {g.numel()} groups for a bank of {self.index.ntotal} rows")
        self._row_groups, self._row_groups_on_index, self._loo_images = g.to(torch.int32), False, None

    def _dataset_images(self) -> int:
        """Images of one epoch of the build pass (0 without geometry)."""
        starts = self._bank_block_starts
        return 0 if starts is None else (len(starts) - 1) // max(1, int(self.augmentation_epoch))

    def row_groups(self) -> torch.Tensor:
        """int32 [ntotal] (CPU): the dataset image of every bank row.  Bank blocks are appended in (epoch, image) order, block b belongs to
        image b % images -- with augmentation_epoch > 1 an image's rows are not one range.  ValueError on a `from_index` bank (no build
        geometry) unless `set_row_groups` gave the table; a `memory_view` carries its rows' images."""
        if self._row_groups is not None:
            return self._row_groups
        n_img = self._dataset_images()
        if not n_img:
            raise ValueError("row_groups: this bank was not built here (from_index): it has no geometry -- call set_row_groups(tensor)")
        st = torch.as_tensor(self._bank_block_starts, dtype=torch.int64)
        g = torch.repeat_interleave(torch.arange(st.numel() - 1, dtype=torch.int64) % n_img, st[1:] - st[:-1]).to(torch.int32)
        if g.numel() != self.index.ntotal:
            raise ValueError(f"row_groups: the build geometry covers {g.numel()} rows, the bank holds {self.index.ntotal}")
        return g

    def _leave_one_out_images(self) -> int:
        """How many images a leave-one-out pass may see: the images of the build (a view: of the bank it was cut from)."""
        if self._loo_images is not None:
            return int(self._loo_images)
        g = self.row_groups()                 # (ValueError: a bank without geometry and without a given table)
        return self._dataset_images() if self._row_groups is None else int(g.max().item()) + 1 if g.numel() else 0

    def _groups_to_index(self) -> None:
        """The row-group table onto the index (once; again after set_row_groups)."""
        g = self.row_groups()
        have = self.index.row_groups
        if have is None or have.numel() != g.numel() or not self._row_groups_on_index:
            self.index.set_row_groups(g, max(self._leave_one_out_images(), int(g.max().item()) + 1 if g.numel() else 0))
            self._row_groups_on_index = True

    # ---- evaluation ------------------------------------------------------------------------------------------------------------------------
    def aggregate(self, feats: torch.Tensor) -> torch.Tensor:
        """feats [B, S*S, D] -> the aggregated rows [B, S*S, 2 r^2]."""
        B, N, D = feats.shape
        self.index.use_current_stream()
        k = self.n_neighbours
        return k5(self.index, "search_aggregate", k)(feats.reshape(B * N, D).contiguous(), k, beta=self.beta, id_base=0).view(B, N, -1)

    def evaluate(self, val_loader, eval_spatial_resolution: int, return_maps: bool = False) -> DepthMetrics:
        S = int(eval_spatial_resolution)
        if self.index.ntotal == 0:
            raise ValueError("evaluate: the bank is empty")
        all_sums, maps = [], []
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for x, y in val_loader:
                gt = _depth_maps(y, self.gpu_device)
                feats = self._tokens(x)
                if feats.shape[1] != S * S:
                    raise ValueError(f"the extractor returned {feats.shape[1]} tokens per image, eval_spatial_resolution={S} expects {S * S}")
                sums, pred = ops.depth_upsample_metrics(self.aggregate(feats), S, self.target_grid, gt, self.min_depth, self.max_depth,
                                                        want_map=return_maps)
                all_sums.append(sums.cpu().numpy())
                if return_maps:
                    maps.append(pred.cpu())
        if not all_sums:
            raise ValueError("evaluate: the validation loader is empty")
        return DepthMetrics(np.concatenate(all_sums), maps if return_maps else None)

    # ---- grids, views, leave-one-out and the paired bootstrap ("Depth grids") --------------------------------------------
    def _grid_banks(self, who: str, views) -> Dict[Any, "HbirdDepthEvaluation"]:
        banks = {None: self} if views is None else dict(views)
        if not banks:
            raise ValueError(f"{who}: views is empty")
        for key, ev in banks.items():
            if not isinstance(ev, HbirdDepthEvaluation):
                raise ValueError(f"{who}: views[{key!r}] is not an HbirdDepthEvaluation")
            if (ev.gpu_device, ev.target_grid, ev.min_depth, ev.max_depth) != (self.gpu_device, self.target_grid, self.min_depth, self.max_depth):
                raise ValueError(f"{who}: views[{key!r}] differs from this evaluator in device, target_grid or depth bounds")
            if ev.index.ntotal == 0:
                raise ValueError(f"{who}: the bank of views[{key!r}] is empty")
        return banks

    def _grid_pass(self, who: str, loader, S: int, plan, banks, views, bootstrap, limit: Optional[int] = None, cut: bool = False):
        """The loop both grid passes share: tokens once per batch, one search per batch and bank at the largest k, one
        `depth_upsample_metrics_grid` per batch and bank.  `limit` (leave-one-out: the searches exclude the query's image): the images the
        pass may see; `cut`: it stops there (max_images) instead of refusing a loader that yields more."""
        excluding = limit is not None
        boot = hboot.parse_bootstrap(bootstrap)
        n_cfg = len(plan.configs)
        sums = {key: [] for key in banks}                     # per bank: [n_cfg, B, 11] per batch
        seen = 0
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for x, y in loader:
                if excluding and cut and seen >= limit:
                    break
                if excluding and cut and seen + x.shape[0] > limit:
                    x, y = x[:limit - seen], y[:limit - seen]
                if excluding and seen + x.shape[0] > limit:
                    raise ValueError(f"{who}: the loader yields more than the {limit} images the bank was built from (it must yield the "
                                     "bank's images, in the order of the build pass)")
                gt = _depth_maps(y, self.gpu_device)
                feats = self._tokens(x)
                B, N, D = feats.shape
                if N != S * S:
                    raise ValueError(f"the extractor returned {N} tokens per image, eval_spatial_resolution={S} expects {S * S}")
                q = feats.reshape(B * N, D).contiguous()
                qgroups = torch.arange(seen, seen + B, dtype=torch.int32, device=q.device).repeat_interleave(N) if excluding else None
                seen += B
                for key, ev in banks.items():
                    ev.index.use_current_stream()
                    if excluding:
                        agg = ev.index.search_aggregate_grid_excluding(q, plan.ks, plan.betas, qgroups, id_base=0)
                        self.loo_screen_served += ev.index.last_exclusion_screen()["served"]
                    else:
                        agg = ev.index.search_aggregate_grid(q, plan.ks, plan.betas, id_base=0)      # [configs, B * N, 2 r^2]: one search
                    s, _ = ops.depth_upsample_metrics_grid(agg.view(n_cfg, B, N, -1), S, self.target_grid, gt, self.min_depth, self.max_depth)
                    sums[key].append(s.cpu().numpy())
        if not seen:
            raise ValueError(f"{who}: the loader is empty")
        keys, metrics = [], {}
        for key in banks:
            per_cfg = np.concatenate(sums[key], axis=1)       # [n_cfg, n_img, 11]
            for c, (k, beta) in enumerate(plan.configs):
                keys.append((k, beta) if views is None else (key, k, beta))
                metrics[keys[-1]] = DepthMetrics(per_cfg[c])
        return metrics if boot is None else depth_bootstrap(keys, metrics, boot[0], boot[1], self.gpu_device)

    def evaluate_grid(self, val_loader, eval_spatial_resolution: int, n_neighbours=None, betas=None, views=None, bootstrap=None):
        """`evaluate` for every (k, beta) of a grid out of ONE pass over the loader: per batch the tokens once, every bank searched ONCE at the
        largest k (`search_aggregate_grid`), one `ops.depth_upsample_metrics_grid` per batch and bank.  Every configuration's `.sums` has the
        bits of `from_index(index, n_neighbours=k, beta=beta).evaluate(...)`.
        `n_neighbours`, `betas`: a value or a list each (duplicates dropped, sorted; `grid_plan`); default: the evaluator's own.
        `views={key: HbirdDepthEvaluation}`: the banks to evaluate -- evaluators on this one's device with its target_grid and bounds, typically
        the `memory_view`s of one bank; anything else raises ValueError naming the key.
        -> {(k, beta): DepthMetrics}, with `views` {(key, k, beta): DepthMetrics}; with `bootstrap=R` or `(R, seed)` a `DepthBootstrap`."""
        from hbird_mi.nn.search_hip import grid_plan
        banks = self._grid_banks("evaluate_grid", views)
        plan = grid_plan(self.n_neighbours if n_neighbours is None else n_neighbours, self.beta if betas is None else betas)
        return self._grid_pass("evaluate_grid", val_loader, int(eval_spatial_resolution), plan, banks, views, bootstrap)

    def evaluate_leave_one_out(self, loader, eval_spatial_resolution: int, n_neighbours=None, betas=None, views=None,
                               max_images: Optional[int] = None, screen: Optional[bool] = None, bootstrap=None):
        """`evaluate_grid` of the bank ON ITS OWN TRAINING IMAGES (`HbirdEvaluation.evaluate_leave_one_out`'s protocol): `loader` yields the
        bank's images in the order of the build pass, the i-th image seen queries with group i and every search excludes the bank rows of the
        query's own image (`search_aggregate_grid_excluding`) -- so (k, beta, target_grid, memory size) can be chosen without the validation
        split.  For every image and configuration the sums are those of `evaluate` on `select_rows(all rows but that image's)`.
        `views`: the `memory_view`s of this bank (they carry their rows' images).  `max_images`: stop after that many images.
        `screen`: True / False switches the certified fp16 screen for excluding searches on / off on every bank of the pass, None leaves the
        indexes as they are; same floats either way.  `self.loo_screen_served` counts the searches (batch x bank) the screen served.
        ValueError when more images arrive than the bank was built from, and for a bank without geometry (`row_groups`)."""
        from hbird_mi.nn.search_hip import grid_plan
        if max_images is not None and int(max_images) < 1:
            raise ValueError("evaluate_leave_one_out: max_images must be positive")
        banks = self._grid_banks("evaluate_leave_one_out", views)
        n_images = self._leave_one_out_images()
        for ev in banks.values():
            with torch.cuda.device(self.gpu_device):
                ev.index.use_current_stream()
                ev._groups_to_index()
                if screen is not None:
                    ev.index.set_exclusion_screen(bool(screen))
        self.loo_screen_served = 0
        plan = grid_plan(self.n_neighbours if n_neighbours is None else n_neighbours, self.beta if betas is None else betas)
        limit = n_images if max_images is None else min(n_images, int(max_images))
        return self._grid_pass("evaluate_leave_one_out", loader, int(eval_spatial_resolution), plan, banks, views, bootstrap, limit=limit,
                               cut=max_images is not None)


# ---- the paired bootstrap over images --------------------------------------------------------------------------------------------------------
LOWER_IS_BETTER = ("rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "log10")      # d1, d2, d3: higher is better
BOOT_COLS = len(METRICS) + 1 + _lib.DEPTH_NSUMS      # per configuration: the nine per-image metrics, the kept flag, the eleven raw sums
BOOT_W_BYTES = 256 << 20                             # a pass's multiplicities stay within this


def finish_sums(s: np.ndarray) -> Dict[str, np.ndarray]:
    """`finish_image` on arrays: float64 [..., 11] -> {metric: float64 [...]}, NaN where n <= 0.  Plain numpy float64 operations, one
    rounding each (the square of the mean log difference is a product)."""
    s = np.asarray(s, dtype=np.float64)
    n = np.where(s[..., 0] > 0, s[..., 0], np.nan)
    mean_log = s[..., 6] / n
    return {"rmse": np.sqrt(s[..., 2] / n), "abs_rel": s[..., 3] / n, "sq_rel": s[..., 4] / n, "rmse_log": np.sqrt(s[..., 5] / n),
            "silog": np.sqrt(np.maximum(0.0, s[..., 5] / n - mean_log * mean_log)), "log10": s[..., 7] / n, "d1": s[..., 8] / n,
            "d2": s[..., 9] / n, "d3": s[..., 10] / n}


def bootstrap_table(metrics: List[DepthMetrics]) -> np.ndarray:
    """The image-major float64 table [n_img, n_cfg * BOOT_COLS] the resampler walks: per configuration the nine per-image metrics (0.0
    where the image has n == 0), the kept flag (1.0 / 0.0) and the eleven raw sums."""
    n_img = len(metrics[0].per_image)
    table = np.zeros((n_img, len(metrics), BOOT_COLS), dtype=np.float64)
    for c, m in enumerate(metrics):
        if len(m.per_image) != n_img:
            raise ValueError("bootstrap: the configurations have seen different image counts")
        for i, per in enumerate(m.per_image):
            if per is not None:
                table[i, c, :len(METRICS)] = [per[k] for k in METRICS]
                table[i, c, len(METRICS)] = 1.0
        table[:, c, len(METRICS) + 1:] = m.sums
    return table.reshape(n_img, -1)


@dataclass
class DepthBootstrap:
    """R paired bootstrap replicates over the images of every configuration of a depth grid: one row of image multiplicities
    (`ops.bootstrap_multiplicities`: the rows the mIoU bootstrap draws for the same seed and image count) serves all configurations.
    `samples[metric]`: the headline estimator -- the mean of the per-image metric over the resampled images that scored a pixel (NaN when
    none did); `pooled_samples[metric]`: the metric of the resampled sums.  Both float64 [R, n_cfg], column c = keys[c]."""
    keys: List[tuple]
    metrics: Dict[tuple, DepthMetrics]        # what the pass returns without bootstrap=
    samples: Dict[str, np.ndarray]
    pooled_samples: Dict[str, np.ndarray]
    seed: int
    n_images: int

    def _col(self, key) -> int:
        try:
            return self.keys.index(key)
        except ValueError:
            raise KeyError(key) from None

    @staticmethod
    def _metric(metric: str) -> str:
        if metric not in METRICS:
            raise ValueError(f"metric={metric!r}: one of {', '.join(METRICS)}")
        return metric

    def interval(self, key, metric: str = "rmse", level: float = 0.95) -> np.ndarray:
        return np.quantile(self.samples[self._metric(metric)][:, self._col(key)], [(1 - level) / 2, (1 + level) / 2])

    def difference(self, a, b, metric: str = "rmse", level: float = 0.95) -> Tuple[float, float, float, float]:
        """(metric[a] - metric[b], lo, hi, share of replicates with a > b) on the paired columns."""
        s = self.samples[self._metric(metric)]
        d = s[:, self._col(a)] - s[:, self._col(b)]
        lo, hi = np.quantile(d, [(1 - level) / 2, (1 + level) / 2])
        return self.metrics[a][metric] - self.metrics[b][metric], float(lo), float(hi), float((d > 0).mean())

    def best(self, metric: str = "rmse", level: float = 0.95):
        """(the best key -- the smallest rmse, abs_rel, sq_rel, rmse_log, silog, log10, the largest d1, d2, d3; the first one in key order
        among equals --, [keys whose paired difference interval to it contains 0])."""
        sign = 1.0 if self._metric(metric) in LOWER_IS_BETTER else -1.0
        top = min(self.keys, key=lambda k: sign * self.metrics[k][metric])
        tied = []
        for k in self.keys:
            if k == top:
                continue
            _, lo, hi, _ = self.difference(top, k, metric, level)
            if lo <= 0.0 <= hi:
                tied.append(k)
        return top, tied


def finish_bootstrap(keys: List[tuple], metrics: Dict[tuple, DepthMetrics], resampled: np.ndarray, seed: int) -> DepthBootstrap:
    """`resampled` float64 [R, n_cfg * BOOT_COLS] = W x `bootstrap_table` -> the replicates, finished in float64 numpy: headline = resampled
    metric column / resampled kept column, pooled = `finish_sums` of the resampled sums."""
    out = np.asarray(resampled, dtype=np.float64).reshape(-1, len(keys), BOOT_COLS)
    nm = len(METRICS)
    with np.errstate(invalid="ignore", divide="ignore"):
        samples = {m: out[:, :, i] / out[:, :, nm] for i, m in enumerate(METRICS)}      # 0 / 0: no resampled image scored a pixel -> NaN
        pooled = finish_sums(out[:, :, nm + 1:])
    return DepthBootstrap(keys=list(keys), metrics=dict(metrics), samples=samples, pooled_samples=pooled, seed=int(seed),
                          n_images=len(metrics[keys[0]].per_image))


def depth_bootstrap(keys: List[tuple], metrics: Dict[tuple, DepthMetrics], R: int, seed: int, device, _pass_replicates: int = 0) -> DepthBootstrap:
    """The estimator: `ops.bootstrap_weighted_sums` over `bootstrap_table`, R replicates in passes whose multiplicities stay within 256 MiB
    (`_pass_replicates` (tests): replicates per pass; the result does not depend on it), finished on the host (`finish_bootstrap`)."""
    table = bootstrap_table([metrics[k] for k in keys])
    n_img = table.shape[0]
    step = int(_pass_replicates) if _pass_replicates else max(1, BOOT_W_BYTES // (4 * n_img))
    out = np.empty((R, table.shape[1]), dtype=np.float64)
    with torch.cuda.device(device):
        dev_table = torch.from_numpy(table).to(device)
        for r0 in range(0, R, step):
            W = ops.bootstrap_multiplicities(n_img, seed, min(step, R - r0), r0=r0, device=device)
            out[r0:r0 + W.shape[0]] = ops.bootstrap_weighted_sums(dev_table, W).cpu().numpy()
    return finish_bootstrap(keys, metrics, out, seed)


_NOT_FOR_DEPTH = ("frame_size", "window_stride", "grid_k", "grid_beta", "bootstrap", "bootstrap_seed", "leave_one_out", "memory_sizes",
                  "overclustering", "linear_probe", "return_knn_details", "f_mem_p", "l_mem_p")


def hbird_depth_evaluation(model, d_model: int, patch_size: int, dataset_name: str, data_dir: str, batch_size: int = 64, input_size: int = 224,
                           augmentation_epoch: int = 1, device: str | torch.device = "cuda", n_neighbours: int = 30, beta: float = 0.02,
                           nn_method: str = "hip", nn_params: Optional[Dict[str, Any]] = None, ftr_extr_fn=None, memory_size: Optional[int] = None,
                           num_workers: int = 8, target_grid: int = 1, min_depth: float = 1e-3, max_depth: float = 10.0,
                           depth_scale: float = 1000.0, train_fs_path: Optional[str] = None, val_fs_path: Optional[str] = None,
                           return_maps: bool = False, **not_for_depth) -> DepthMetrics:
    """`hbird_evaluation` for depth: dataset_name "synthetic-depth[*frac]" or "depth-folder[*frac]" (hbird_mi/data/synthetic_depth.py).
    Sliding windows (frame_size, window_stride), grids (grid_k, grid_beta), bootstrap, leave_one_out, memory_sizes and the other protocols of
    `hbird_evaluation` raise ValueError naming the argument."""
    for name, value in not_for_depth.items():
        if name not in _NOT_FOR_DEPTH:
            raise TypeError(f"hbird_depth_evaluation() got an unexpected keyword argument '{name}'")
        if value is not None and value is not False:
            raise ValueError(f"{name} is not available for depth")
    if nn_method not in ("hip", "faiss", "scann"):
        raise ValueError(f"nn_method={nn_method!r}: only hip, faiss and scann are known")
    S = input_size // patch_size
    if ftr_extr_fn is None:
        extractor = FeatureExtractor(model, eval_spatial_resolution=S, d_model=d_model)
    else:
        extractor = FeatureExtractorSimple(model, ftr_extr_fn=ftr_extr_fn, eval_spatial_resolution=S, d_model=d_model)
    from hbird_mi.data.synthetic_depth import get_depth_dataset
    dataset = get_depth_dataset(dataset_name, data_dir, batch_size, num_workers, input_size, depth_scale, max_depth, train_fs_path, val_fs_path)
    ev = HbirdDepthEvaluation(extractor, dataset.train_dataloader(), n_neighbours=n_neighbours, beta=beta, target_grid=target_grid,
                              min_depth=min_depth, max_depth=max_depth, augmentation_epoch=augmentation_epoch, device=device, nn_params=nn_params,
                              memory_size=memory_size, dataset_size=dataset.get_train_dataset_size())
    last_run_info.clear()
    last_run_info.update(bank_build_s=float(ev.bank_build_s), bank_rows=int(ev.index.ntotal))
    try:
        return ev.evaluate(dataset.val_dataloader(), S, return_maps=return_maps)
    finally:
        ev.index.close()


_NOT_FOR_DEPTH_GRIDS = ("frame_size", "window_stride", "return_maps", "overclustering", "linear_probe", "return_knn_details", "f_mem_p", "l_mem_p")


def hbird_depth_grid_evaluation(model, d_model: int, patch_size: int, dataset_name: str, data_dir: str, batch_size: int = 64, input_size: int = 224,
                                augmentation_epoch: int = 1, device: str | torch.device = "cuda", n_neighbours: int = 30, beta: float = 0.02,
                                nn_method: str = "hip", nn_params: Optional[Dict[str, Any]] = None, ftr_extr_fn=None,
                                memory_size: Optional[int] = None, num_workers: int = 8, target_grid: int = 1, min_depth: float = 1e-3,
                                max_depth: float = 10.0, depth_scale: float = 1000.0, train_fs_path: Optional[str] = None,
                                val_fs_path: Optional[str] = None, grid_k=None, grid_beta=None, memory_sizes=None, leave_one_out: bool = False,
                                leave_one_out_images: Optional[int] = None, leave_one_out_screen: bool = False, bootstrap: Optional[int] = None,
                                bootstrap_seed: Optional[int] = None, **not_for_grids):
    """`hbird_depth_evaluation` over a grid: `grid_k` / `grid_beta` (either or both; the other defaults to `n_neighbours` / `beta`) out of ONE
    pass with one search per batch (`HbirdDepthEvaluation.evaluate_grid`); `memory_sizes=[...]`: every listed size <= `memory_size` on a
    `memory_view` of the one bank built at `memory_size`; `leave_one_out=True`: the scores come from the TRAIN loader, every image excluding
    its own rows (`evaluate_leave_one_out`; `leave_one_out_images=N` stops after N images, `leave_one_out_screen=True` lets the certified
    fp16 screen serve the excluding searches); `bootstrap=R` (`bootstrap_seed=`): a `DepthBootstrap` instead of the dict.
    -> {(k, beta): DepthMetrics}, with `memory_sizes` {(size, k, beta): DepthMetrics}.  Sliding windows (frame_size, window_stride), maps and the
    segmentation protocols raise ValueError naming the argument; several GPUs and torch.distributed as for `HbirdDepthEvaluation`."""
    for name, value in not_for_grids.items():
        if name not in _NOT_FOR_DEPTH_GRIDS:
            raise TypeError(f"hbird_depth_grid_evaluation() got an unexpected keyword argument '{name}'")
        if value is not None and value is not False:
            raise ValueError(f"{name} is not available for depth grids")
    if nn_method not in ("hip", "faiss", "scann"):
        raise ValueError(f"nn_method={nn_method!r}: only hip, faiss and scann are known")
    if bootstrap is None and bootstrap_seed is not None:
        raise ValueError("bootstrap_seed needs bootstrap")
    if memory_sizes is not None and memory_size is None:
        raise ValueError("memory_sizes needs memory_size: the bank is built once, at memory_size, and the listed sizes are views of it")
    if not leave_one_out and (leave_one_out_images is not None or leave_one_out_screen):
        raise ValueError("leave_one_out_images and leave_one_out_screen need leave_one_out")
    from hbird_mi.nn.search_hip import grid_plan
    grid_plan(n_neighbours if grid_k is None else grid_k, beta if grid_beta is None else grid_beta)      # a bad grid fails before the bank is built
    boot = None if bootstrap is None else hboot.parse_bootstrap(bootstrap, bootstrap_seed)
    S = input_size // patch_size
    if ftr_extr_fn is None:
        extractor = FeatureExtractor(model, eval_spatial_resolution=S, d_model=d_model)
    else:
        extractor = FeatureExtractorSimple(model, ftr_extr_fn=ftr_extr_fn, eval_spatial_resolution=S, d_model=d_model)
    from hbird_mi.data.synthetic_depth import get_depth_dataset
    dataset = get_depth_dataset(dataset_name, data_dir, batch_size, num_workers, input_size, depth_scale, max_depth, train_fs_path, val_fs_path)
    ev = HbirdDepthEvaluation(extractor, dataset.train_dataloader(), n_neighbours=n_neighbours, beta=beta, target_grid=target_grid,
                              min_depth=min_depth, max_depth=max_depth, augmentation_epoch=augmentation_epoch, device=device, nn_params=nn_params,
                              memory_size=memory_size, dataset_size=dataset.get_train_dataset_size())
    last_run_info.clear()
    last_run_info.update(bank_build_s=float(ev.bank_build_s), bank_rows=int(ev.index.ntotal))
    sized = None
    try:
        if memory_sizes is not None:
            sized = {}
            for size in memory_sizes:
                size = int(size)
                if size <= memory_size and size not in sized:
                    sized[size] = ev if size == memory_size else ev.memory_view(size)
        grid = dict(n_neighbours=grid_k, betas=grid_beta, views=sized, bootstrap=boot)
        if leave_one_out:
            return ev.evaluate_leave_one_out(dataset.train_dataloader(), S, max_images=leave_one_out_images,
                                             screen=True if leave_one_out_screen else None, **grid)
        return ev.evaluate_grid(dataset.val_dataloader(), S, **grid)
    finally:
        for view in (sized or {}).values():
            if view is not ev:
                view.index.close()
        ev.index.close()
