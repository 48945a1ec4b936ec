"""Depth estimation by retrieval: the Hummingbird evaluation's second task (monocular depth, e.g. NYUv2) on the engine of the first.

The bank is an ordinary `HipFlatIndex` whose label rows are fp32 values -- per cell of a patch the sum of its valid depths and its valid
share, both over the cell's area (`ops.patch_depth_targets`, include/hbird_hip_depth.h).  A query's neighbours are combined by the same
cosine-softmax (`search_aggregate`, K5 unchanged: the certified fp16 screen, memory views and bounded sampling all apply), and
`ops.depth_upsample_metrics` turns the aggregated rows into a depth map -- the ratio of the two bilinearly upsampled grids, clamped -- and
deterministic per-image error sums, which `finish_metrics` turns into rmse, abs_rel, sq_rel, rmse_log, silog, log10, d1, d2, d3.

No dataset is bundled and no figure of this module has been held to a published one.
"""
from __future__ import annotations

import math
import time
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from hbird_mi import _lib, ops, views
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
        return HbirdDepthEvaluation.from_index(self.feature_extractor, index, self.n_neighbours, self.beta, self.target_grid, self.min_depth,
                                               self.max_depth, self.device)

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
