"""Paired bootstrap over images for mIoU grids (not in the reference; DESIGN.md section 4, "Bootstrap intervals").

Every configuration of a grid is evaluated on the same images in the same order, and mIoU is a function of per-class pixel counts that add
over images.  `ImageCountCollector` keeps those counts per image -- the table stats[n_img][n_cfg * 3 G] -- and `MiouBootstrap` carries what
the resampling kernels (csrc/hbird_bootstrap.hip) make of it: R replicates of every configuration's mIoU, drawn with the SAME image
multiplicities for all of them, so that two grid points can be compared on their paired difference.
The replicates use the identity matching of prediction to ground-truth classes (`PredsmIoU.compute(linear_probe=True)`); `miou` is the
Hungarian-matched figure the evaluator has always returned.  They describe the same quantity where the matching IS the identity
(`matching_is_identity`), which it is whenever the predictions are better than a permutation of themselves.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from hbird_mi import ops

logger = logging.getLogger(__name__)

DEFAULT_SEED = 20240229       # tests/test_bootstrap_cpu.py holds the resampler's restatement to its moments at this seed


def parse_bootstrap(bootstrap, seed: Optional[int] = None) -> Optional[Tuple[int, int]]:
    """None | R | (R, seed) -> None | (R, seed)."""
    if bootstrap is None:
        return None
    if isinstance(bootstrap, (tuple, list)):
        if len(bootstrap) != 2:
            raise ValueError("bootstrap must be a replicate count R or a pair (R, seed)")
        R, seed = bootstrap
    else:
        R = bootstrap
    if isinstance(R, bool) or int(R) != R or not 1 <= int(R) <= (1 << 20):
        raise ValueError(f"bootstrap: the replicate count must be an integer in [1, 2^20], got {R!r}")
    seed = DEFAULT_SEED if seed is None else int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("bootstrap: the seed must fit 64 unsigned bits")
    return int(R), seed


class ImageCountCollector:
    """The growing image-major table stats[n_img][n_cfg * 3 G] (int32, on the device): `add(cfg, gt, pred_map)` writes the (tp, fp, fn)
    blocks of one batch's images for configuration `cfg`; the image index is the running count of images in loader order, kept per
    configuration (every configuration must see every batch)."""

    def __init__(self, num_classes: int, n_cfg: int, ignore_index: Optional[int], device, capacity: Optional[int] = None):
        self.num_classes, self.n_cfg = int(num_classes), int(n_cfg)
        if self.num_classes < 1 or self.n_cfg < 1:
            raise ValueError("ImageCountCollector: num_classes and n_cfg must be positive")
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.device = torch.device(device)
        self.cols = self.n_cfg * 3 * self.num_classes
        self._seen = [0] * self.n_cfg
        self._table = torch.zeros((max(int(capacity or 0), 16), self.cols), dtype=torch.int32, device=self.device)

    @classmethod
    def for_loader(cls, loader, num_classes: int, n_cfg: int, ignore_index: Optional[int], device) -> "ImageCountCollector":
        """Capacity from len(loader.dataset) where the loader has one (else the table grows geometrically)."""
        try:
            cap = len(loader.dataset)
        except (AttributeError, TypeError):
            cap = None
        return cls(num_classes, n_cfg, ignore_index, device, capacity=cap)

    def _reserve(self, rows: int) -> None:
        if rows <= self._table.shape[0]:
            return
        grown = torch.zeros((max(rows, 2 * self._table.shape[0]), self.cols), dtype=torch.int32, device=self.device)
        grown[:self._table.shape[0]] = self._table
        self._table = grown

    @torch.no_grad()
    def add(self, cfg: int, gt: torch.Tensor, pred_map: torch.Tensor) -> None:
        if not 0 <= cfg < self.n_cfg:
            raise ValueError(f"ImageCountCollector.add: configuration {cfg} outside [0, {self.n_cfg})")
        B = int(gt.shape[0])
        if B == 0:
            return
        row = self._seen[cfg]
        self._reserve(row + B)
        block = 3 * self.num_classes
        ops.image_class_counts(gt, pred_map, self.num_classes, self.ignore_index,
                               out=self._table.view(-1)[row * self.cols + cfg * block:], row_stride=self.cols)
        self._seen[cfg] = row + B

    @property
    def n_images(self) -> int:
        if len(set(self._seen)) != 1:
            raise RuntimeError(f"ImageCountCollector: the configurations have seen different image counts {self._seen}")
        return self._seen[0]

    def stats(self) -> torch.Tensor:
        """int32 [n_images, n_cfg * 3 G] (a view of the table)."""
        return self._table[:self.n_images]


@dataclass
class MiouBootstrap:
    keys: List[tuple]
    miou: Dict[tuple, float]                  # what evaluate_grid returns without bootstrap= (PredsmIoU.compute, Hungarian matching)
    point: torch.Tensor                       # float64 [n_cfg] on the device: the identity-matching mIoU on all images
    samples: np.ndarray                       # float64 [R, n_cfg]: column c = replicates of keys[c], rows paired across columns
    seed: int
    n_images: int
    matching_is_identity: Dict[tuple, bool]   # False: `samples` (identity matching) and `miou` (Hungarian) differ in kind for that key

    def _col(self, key) -> int:
        try:
            return self.keys.index(key)
        except ValueError:
            raise KeyError(key) from None

    def interval(self, key, level: float = 0.95) -> np.ndarray:
        return np.quantile(self.samples[:, self._col(key)], [(1 - level) / 2, (1 + level) / 2])

    def difference(self, a, b, level: float = 0.95) -> Tuple[float, float, float, float]:
        """(miou[a] - miou[b], lo, hi, share of replicates with a > b) on the paired columns."""
        d = self.samples[:, self._col(a)] - self.samples[:, self._col(b)]
        lo, hi = np.quantile(d, [(1 - level) / 2, (1 + level) / 2])
        return self.miou[a] - self.miou[b], float(lo), float(hi), float((d > 0).mean())

    def best(self, level: float = 0.95):
        """(arg-max key of miou, [keys whose paired difference interval to it contains 0])."""
        top = max(self.keys, key=lambda k: self.miou[k])       # the first maximum in key order
        tied = []
        for k in self.keys:
            if k == top:
                continue
            _, lo, hi, _ = self.difference(top, k, level)
            if lo <= 0.0 <= hi:
                tied.append(k)
        return top, tied


def finish(keys: List[tuple], metrics, collector: ImageCountCollector, R: int, seed: int, _chunk_replicates: int = 0) -> MiouBootstrap:
    """`metrics[c]`: the PredsmIoU of keys[c] (its total confusion matrix accumulated as ever); -> the MiouBootstrap of the pass."""
    if len(keys) != len(metrics) or len(keys) != collector.n_cfg:
        raise ValueError("bootstrap.finish: keys, metrics and the collector's configurations differ in number")
    n = collector.n_images
    if n < 1:
        raise ValueError("bootstrap: the loader yielded no image")
    miou, identity = {}, {}
    for key, m in zip(keys, metrics):
        miou[key] = m.compute(is_global_zero=True, sync_distributed=False, return_reordered=False)[0]
        identity[key] = bool(np.array_equal(m._hungarian_mapping(), np.arange(m.num_pred_classes)))
        if not identity[key]:
            logger.warning("bootstrap: the Hungarian matching of %r is not the identity; its replicates describe the identity matching, "
                           "its mIoU does not", key)
    with torch.cuda.device(collector.device):
        point, samples = ops.bootstrap_miou(collector.stats(), collector.n_cfg, collector.num_classes, seed, R, _chunk_replicates)
    return MiouBootstrap(keys=list(keys), miou=miou, point=point, samples=samples.cpu().numpy(), seed=int(seed), n_images=n,
                         matching_is_identity=identity)
