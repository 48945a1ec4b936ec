"""Data modules of the depth evaluation (hbird_mi/depth.py): loaders yield `(x [B,3,H,W] float, y [B,1,H,W] float32 = depth in metres)`; a
value that is not finite or lies outside [min_depth, max_depth] is a hole (include/hbird_hip_depth.h, "valid depth").

  * "synthetic-depth"  -- `SyntheticDepthDataModule`: a procedural world where colour determines depth (no files; the tests and the CLI's
                          self-check), and
  * a folder of images with same-stem depth files -- `DepthFolderDataModule` (NYUv2 and the like, once converted: the conversion from the
    dataset's own .mat is the user's).
"""
from __future__ import annotations

import os
import random
from typing import List, Optional, Tuple

import numpy as np
import torch

from .synthetic import _Loader


class SyntheticDepthDataModule:
    """T textures, each with a colour prototype and a depth profile -- a plane `base + gx * u + gy * v` over the local coordinates (u, v) in
    [0, 1) of a `block` x `block`-pixel tile (gx = gy = 0: fronto-parallel; else a ramp).  An image is a grid of tiles with random textures;
    its RGB pixels are prototype[texture] + noise, its depth the tile's profile.  So a patch's colour determines its depth profile and
    retrieval is informative.  Every image carries holes: a rectangle of zeros, a sprinkle of NaN, a strip beyond `max_depth`.
    Deterministic (own torch.Generator)."""

    def __init__(self, batch_size: int = 8, input_size: int = 64, n_textures: int = 6, n_train: int = 32, n_val: int = 16, block: int = 8,
                 train_fraction: float = 1.0, seed: int = 0, max_depth: float = 10.0, holes: bool = True):
        if isinstance(input_size, (tuple, list)):
            raise ValueError("SyntheticDepthDataModule: input_size must be one square side (sliding windows are not available for depth)")
        if input_size % block:
            raise ValueError(f"SyntheticDepthDataModule: input_size={input_size} must be a multiple of block={block}")
        self.batch_size, self.input_size, self.block, self.holes, self.max_depth = batch_size, int(input_size), int(block), holes, float(max_depth)
        self.n_train = max(1, int(round(n_train * train_fraction)))
        self.n_val = n_val
        g = torch.Generator().manual_seed(seed)
        self.proto = torch.randn((n_textures, 3), generator=g)
        self.base = 1.0 + 7.0 * torch.rand((n_textures,), generator=g)                   # metres
        slope = 1.5 * (torch.rand((n_textures, 2), generator=g) - 0.5)
        slope[::2] = 0.0                                                                 # every other texture is a fronto-parallel plane
        self.slope = slope
        self._train = self._make(self.n_train, g)
        self._val = self._make(self.n_val, g)

    def _make(self, n, g):
        H, bl = self.input_size, self.block
        T = self.proto.shape[0]
        uv = (torch.arange(H) % bl).float() / bl
        out = []
        for b0 in range(0, n, self.batch_size):
            bs = min(self.batch_size, n - b0)
            tex = torch.randint(0, T, (bs, H // bl, H // bl), generator=g).repeat_interleave(bl, 1).repeat_interleave(bl, 2)
            y = self.base[tex] + self.slope[tex][..., 0] * uv[None, None, :] + self.slope[tex][..., 1] * uv[None, :, None]
            x = self.proto[tex].permute(0, 3, 1, 2) + 0.1 * torch.randn((bs, 3, H, H), generator=g)
            if self.holes:
                for b in range(bs):
                    y0, x0 = (int(v) for v in torch.randint(0, H - bl, (2,), generator=g))
                    y[b, y0:y0 + bl + 3, x0:x0 + bl // 2 + 1] = 0.0                      # a sensor hole
                    y[b, H - 2:, :] = self.max_depth + 5.0                               # beyond the range
                y[torch.rand(y.shape, generator=g) < 0.01] = float("nan")
            out.append((x.float(), y.float().unsqueeze(1).contiguous()))
        return out

    def get_train_dataset_size(self):
        return self.n_train

    def train_dataloader(self):
        return _Loader(self._train)

    def val_dataloader(self):
        return _Loader(self._val)


# ---- folders -------------------------------------------------------------------------------------------------------------------------------
_IMG_EXT = (".jpg", ".jpeg", ".png")


class DepthFolder(torch.utils.data.Dataset):
    """<root>/<split>/images/<stem>.{jpg,jpeg,png} with <root>/<split>/depth/<stem>.npy (float32 metres, [H,W]) or <stem>.png (16-bit, metres =
    value / depth_scale; 0 stays 0, a hole).  The image goes through folder.py's tensor conversion (bilinear resize, ImageNet normalisation),
    the depth is resized NEAREST -- no value is invented between two surfaces -- and neither is flipped, cropped or rescaled."""

    def __init__(self, root: str, split: str, input_size: int, depth_scale: float = 1000.0, file_set: Optional[List[str]] = None):
        from .folder import open_store
        self.store, self.split, self.size, self.depth_scale = open_store(root), split, int(input_size), float(depth_scale)
        if not (self.store.isdir(f"{split}/images") and self.store.isdir(f"{split}/depth")):
            raise RuntimeError(f"Dataset not found or corrupted: no {split}/images and {split}/depth under {root}")
        depth = {os.path.splitext(f)[0]: f for f in self.store.listdir(f"{split}/depth") if f.lower().endswith((".npy", ".png"))}
        self.pairs: List[Tuple[str, str]] = []
        for f in self.store.listdir(f"{split}/images"):
            stem, ext = os.path.splitext(f)
            if ext.lower() not in _IMG_EXT or (file_set is not None and stem not in file_set):
                continue
            if stem not in depth:
                raise RuntimeError(f"Dataset not found or corrupted: {split}/images/{f} has no depth file of the same stem")
            self.pairs.append((f"{split}/images/{f}", f"{split}/depth/{depth[stem]}"))
        if not self.pairs:
            raise RuntimeError(f"Dataset not found or corrupted: no {split} samples under {root}")

    def __len__(self):
        return len(self.pairs)

    def read_depth(self, rel: str) -> np.ndarray:
        with self.store.open(rel) as f:
            if rel.lower().endswith(".npy"):
                import io
                d = np.load(io.BytesIO(f.read()), allow_pickle=False)
            else:
                from PIL import Image
                img = Image.open(f)
                img.load()
                d = np.asarray(img).astype(np.float32) / np.float32(self.depth_scale)
        if d.ndim != 2:
            raise ValueError(f"{rel}: a depth map must be [H, W], got {d.shape}")
        return np.ascontiguousarray(d, dtype=np.float32)

    def __getitem__(self, i):
        from PIL import Image
        from .folder import _to_tensor_img, _wh
        ip, dp = self.pairs[i]
        with self.store.open(ip) as f:
            img = Image.open(f).convert("RGB")
        d = Image.fromarray(self.read_depth(dp), mode="F").resize(_wh(self.size), Image.NEAREST)
        return _to_tensor_img(img.resize(_wh(self.size), Image.BILINEAR)), torch.from_numpy(np.array(d, dtype=np.float32)).unsqueeze(0)


class DepthFolderDataModule:
    def __init__(self, data_dir: str, batch_size: int, num_workers: int, input_size: int, depth_scale: float = 1000.0, train_fraction: float = 1.0,
                 train_fs_path: Optional[str] = None, val_fs_path: Optional[str] = None):
        from .folder import read_file_set
        if isinstance(input_size, (tuple, list)):
            raise ValueError("DepthFolderDataModule: input_size must be one square side (sliding windows are not available for depth)")
        self.batch_size, self.num_workers = batch_size, num_workers
        self.train = DepthFolder(data_dir, "train", input_size, depth_scale, read_file_set(train_fs_path) if train_fs_path else None)
        if train_fraction < 1.0:
            random.shuffle(self.train.pairs)
            self.train.pairs = self.train.pairs[: max(1, int(len(self.train.pairs) * train_fraction))]
        self.val = DepthFolder(data_dir, "val", input_size, depth_scale, read_file_set(val_fs_path) if val_fs_path else None)

    def get_train_dataset_size(self):
        return len(self.train)

    def _loader(self, ds):
        return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=False, num_workers=self.num_workers, drop_last=False,
                                           pin_memory=torch.cuda.is_available())

    def train_dataloader(self):
        return self._loader(self.train)

    def val_dataloader(self):
        return self._loader(self.val)


def get_depth_dataset(dataset_name: str, data_dir: str, batch_size: int, num_workers: int, input_size: int, depth_scale: float = 1000.0,
                      max_depth: float = 10.0, train_fs_path: Optional[str] = None, val_fs_path: Optional[str] = None):
    """"synthetic-depth[*frac]" or "depth-folder[*frac]" (a `DepthFolderDataModule` over data_dir) -> the data module."""
    name, frac = dataset_name, 1.0
    if "*" in dataset_name:
        name, f = dataset_name.split("*")
        frac = float(f)
    name = name.strip().lower()
    if name == "synthetic-depth":
        return SyntheticDepthDataModule(batch_size=batch_size, input_size=input_size, train_fraction=frac, max_depth=max_depth)
    if name == "depth-folder":
        return DepthFolderDataModule(data_dir, batch_size, num_workers, input_size, depth_scale, frac, train_fs_path, val_fs_path)
    raise ValueError(f"Unknown depth dataset name: {dataset_name} (synthetic-depth | depth-folder)")
