"""Row lists of sub-bank views: which rows of a built bank make up the bank of a smaller memory size or of an image subset.

Pure host code (no GPU): the lists feed `HipFlatIndex.select_rows` / `HbirdEvaluation.memory_view`.

Why a smaller bank is a row subset of a bigger one.  The bounded build keeps, per (epoch, image), the K patches with the smallest noisy
scores, K = `per_image_rows(...)` (reference hbird_eval.py:146-147), in ascending score order with ties to the lower patch index
(`ops.patch_select`; hbird_eval.py:497-511).  The noise `torch.rand(total_nz)` is drawn per batch and does not depend on K, and the K
smallest entries of one fixed vector, in order, are the first K of its K' >= K smallest.  So the bank for memory_size m is the first K_m
rows of every block of K_M rows of the bank for M >= m, row for row and bit for bit.  In the unbounded build every (epoch, image) block is
the image's S x S patches, and an image subset is simply those blocks.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch


def per_image_rows(memory_size: int, dataset_size: int, augmentation_epoch: int = 1) -> int:
    """Patches kept per (epoch, image) by the bounded build: the reference's rule, hbird_eval.py:146-147."""
    denom = int(dataset_size) * int(augmentation_epoch)
    return max(1, int(memory_size) // max(1, denom))


def view_rows(block_starts, per_block: Optional[int] = None, blocks: Optional[Iterable[int]] = None) -> torch.Tensor:
    """Row ids (int64 tensor) of a view.  `block_starts`: the [n_blocks + 1] cumulative row offsets of the (epoch, image) blocks in build
    order.  `per_block` keeps the first min(per_block, len) rows of each block; `blocks` keeps only those blocks -- in ascending block order
    whatever order they were listed in (a view keeps the build's row order); a block listed twice is refused."""
    starts = torch.as_tensor(block_starts, dtype=torch.int64).reshape(-1)
    if starts.numel() < 1:
        raise ValueError("view_rows: block_starts needs at least one entry (n_blocks + 1 cumulative offsets)")
    lens = starts[1:] - starts[:-1]
    if bool((lens < 0).any()):
        raise ValueError("view_rows: block_starts must not decrease")
    n_blocks = lens.numel()
    if blocks is None:
        keep = torch.arange(n_blocks, dtype=torch.int64)
    else:
        keep = torch.as_tensor(list(blocks) if not isinstance(blocks, torch.Tensor) else blocks, dtype=torch.int64).reshape(-1)
        if keep.numel() and (int(keep.min()) < 0 or int(keep.max()) >= n_blocks):
            raise ValueError(f"view_rows: a block index lies outside [0, {n_blocks})")
        keep = torch.sort(keep).values
        if keep.numel() > 1 and bool((keep[1:] == keep[:-1]).any()):
            raise ValueError("view_rows: a block is listed twice")
    take = lens[keep]
    if per_block is not None:
        if int(per_block) < 0:
            raise ValueError("view_rows: per_block must not be negative")
        take = take.clamp(max=int(per_block))
    total = int(take.sum())
    if total == 0:
        return torch.zeros(0, dtype=torch.int64)
    # row = start of its block + position within the block
    first = torch.cumsum(take, 0) - take                       # output offset of every kept block
    owner = torch.repeat_interleave(torch.arange(keep.numel(), dtype=torch.int64), take)
    return starts[keep][owner] + (torch.arange(total, dtype=torch.int64) - first[owner])
