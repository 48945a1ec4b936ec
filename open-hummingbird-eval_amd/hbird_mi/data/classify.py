"""Data modules of the image-level k-NN classification (hbird_mi/classify.py): `train_dataloader()` / `val_dataloader()` yield
`(images [B,3,H,W] float, class ids [B] int64)`; a class id of -1 marks an unlabelled image (kept out of the vote as a bank row, counted as
skipped as a query).

  * "synthetic-classify" -- `SyntheticClassifyDataModule`: the mean colour plus a texture frequency determines the class (no files; the tests
                            and the CLI's self-check), and
  * "class-folder"       -- `ClassFolderDataModule`: <root>/{train,val}/<class name>/*.{png,jpg,jpeg,npy}, classes in sorted name order.
"""
from __future__ import annotations

import math
import os
import random
from typing import List, Optional, Tuple

import numpy as np
import torch

from .synthetic import _Loader

_COLOURS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0))
_IMG_EXT = (".png", ".jpg", ".jpeg", ".npy")


class SyntheticClassifyDataModule:
    """num_classes classes; class c has the mean colour _COLOURS[c % 6] and horizontal stripes of 1 + c // 6 periods per image (amplitude
    0.5), so that colour and texture frequency together determine the class.  Every pixel gets `noise` sigma of Gaussian noise and every
    image a random phase: at noise = 0 a pooled feature separates the classes perfectly, a larger `noise` makes the task imperfect.
    Deterministic per seed (own torch.Generator)."""

    def __init__(self, batch_size: int = 16, input_size: int = 32, num_classes: int = 12, n_train: int = 192, n_val: int = 60, noise: float = 0.5,
                 train_fraction: float = 1.0, seed: int = 0):
        if isinstance(input_size, (tuple, list)) or int(input_size) < 8:
            raise ValueError(f"SyntheticClassifyDataModule: input_size={input_size!r} must be one square side of at least 8 pixels")
        if not 1 <= int(num_classes) <= 6 * (int(input_size) // 4):
            raise ValueError(f"SyntheticClassifyDataModule: num_classes={num_classes} must lie in [1, {6 * (int(input_size) // 4)}] at input_size={input_size}")
        if not (isinstance(noise, (int, float)) and math.isfinite(noise) and noise >= 0):
            raise ValueError(f"SyntheticClassifyDataModule: noise={noise!r} must be a finite number >= 0")
        self.batch_size, self.input_size, self.num_classes, self.noise = int(batch_size), int(input_size), int(num_classes), float(noise)
        self.n_train, self.n_val = max(1, int(round(n_train * train_fraction))), int(n_val)
        g = torch.Generator().manual_seed(seed)
        self._train = self._make(self.n_train, g)
        self._val = self._make(self.n_val, g)

    def _make(self, n: int, g) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        S = self.input_size
        col = torch.tensor(_COLOURS)
        rows = torch.arange(S, dtype=torch.float32) / S
        out = []
        for b0 in range(0, n, self.batch_size):
            bs = min(self.batch_size, n - b0)
            y = torch.randint(0, self.num_classes, (bs,), generator=g)
            phase = torch.rand((bs,), generator=g)
            freq = (1 + y // len(_COLOURS)).float()
            stripes = 0.5 * torch.sin(2.0 * math.pi * (freq[:, None] * rows[None, :] + phase[:, None]))          # [bs, S]: one value per image row
            x = col[y % len(_COLOURS)][:, :, None, None] + stripes[:, None, :, None] + self.noise * torch.randn((bs, 3, S, S), generator=g)
            out.append((x.float().contiguous(), y.to(torch.int64)))
        return out

    def get_train_dataset_size(self) -> int:
        return self.n_train

    def get_num_classes(self) -> int:
        return self.num_classes

    def train_dataloader(self):
        return _Loader(self._train)

    def val_dataloader(self):
        return _Loader(self._val)


# ---- folders -------------------------------------------------------------------------------------------------------------------------------
class ClassFolder(torch.utils.data.Dataset):
    """The files of one split, class by class in sorted name order, files in sorted order inside a class.  .png / .jpg go through folder.py's
    tensor conversion (bilinear resize to input_size, ImageNet normalisation); a .npy file holds a float image [3, H, W] that is used as it
    is (resized bilinear where its size differs)."""

    def __init__(self, root: str, split: str, classes: List[str], input_size: int):
        from .folder import open_store
        self.store, self.split, self.classes, self.size = open_store(root), split, list(classes), int(input_size)
        self.samples: List[Tuple[str, int]] = []
        for c, name in enumerate(self.classes):
            files = sorted(f for f in self.store.listdir(f"{split}/{name}") if f.lower().endswith(_IMG_EXT))
            self.samples += [(f"{split}/{name}/{f}", c) for f in files]
        if not self.samples:
            raise RuntimeError(f"Dataset not found or corrupted: no {split} images under {root}")

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        rel, c = self.samples[i]
        with self.store.open(rel) as f:
            if rel.lower().endswith(".npy"):
                import io
                a = np.load(io.BytesIO(f.read()), allow_pickle=False)
                if a.ndim != 3 or a.shape[0] != 3:
                    raise ValueError(f"{rel}: an image file must hold [3, H, W], got {a.shape}")
                x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
                if tuple(x.shape[1:]) != (self.size, self.size):
                    x = torch.nn.functional.interpolate(x[None], size=(self.size, self.size), mode="bilinear", align_corners=False)[0]
            else:
                from PIL import Image
                from .folder import _to_tensor_img, _wh
                x = _to_tensor_img(Image.open(f).convert("RGB").resize(_wh(self.size), Image.BILINEAR))
        return x, c


def _class_names(store, split: str) -> List[str]:
    return sorted(n for n in store.listdir(split) if store.isdir(f"{split}/{n}"))


class ClassFolderDataModule:
    """<root>/train/<class name>/* and <root>/val/<class name>/*: the class ids are the positions of the class names in sorted order, the same
    in both splits -- a class present in one split only is an error that names it."""

    def __init__(self, data_dir: str, batch_size: int, num_workers: int, input_size: int, train_fraction: float = 1.0):
        from .folder import open_store
        if isinstance(input_size, (tuple, list)):
            raise ValueError("ClassFolderDataModule: input_size must be one square side")
        store = open_store(data_dir)
        if not (store.isdir("train") and store.isdir("val")):
            raise RuntimeError(f"Dataset not found or corrupted: no train and val folders under {data_dir}")
        tr, va = _class_names(store, "train"), _class_names(store, "val")
        only = sorted(set(tr) ^ set(va))
        if only:
            raise RuntimeError("Dataset not found or corrupted: " + ", ".join(f"class {n!r} is present in {'train' if n in tr else 'val'} only" for n in only))
        if not tr:
            raise RuntimeError(f"Dataset not found or corrupted: no class folders under {data_dir}/train")
        self.classes, self.batch_size, self.num_workers = tr, int(batch_size), int(num_workers)
        self.train = ClassFolder(data_dir, "train", tr, input_size)
        if train_fraction < 1.0:
            random.shuffle(self.train.samples)
            self.train.samples = sorted(self.train.samples[: max(1, int(len(self.train.samples) * train_fraction))], key=lambda s: (s[1], s[0]))
        self.val = ClassFolder(data_dir, "val", tr, input_size)

    def get_train_dataset_size(self) -> int:
        return len(self.train)

    def get_num_classes(self) -> int:
        return len(self.classes)

    def _loader(self, ds):
        return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=False, num_workers=self.num_workers, drop_last=False,
                                           pin_memory=torch.cuda.is_available())

    def train_dataloader(self):
        return self._loader(self.train)

    def val_dataloader(self):
        return self._loader(self.val)


def get_classify_dataset(dataset_name: str, data_dir: str = "", batch_size: int = 64, num_workers: int = 8, input_size: int = 224, **synthetic):
    """"synthetic-classify[*frac]" (input_size and `synthetic` go to the world) or "class-folder[*frac]" -> the data module."""
    name, frac = dataset_name, 1.0
    if "*" in dataset_name:
        name, f = dataset_name.split("*")
        frac = float(f)
    name = name.strip().lower()
    if name == "synthetic-classify":
        return SyntheticClassifyDataModule(batch_size=batch_size, input_size=input_size, train_fraction=frac, **synthetic)
    if name == "class-folder":
        if synthetic:
            raise TypeError(f"get_classify_dataset: {sorted(synthetic)} are arguments of the synthetic world")
        return ClassFolderDataModule(data_dir, batch_size, num_workers, input_size, frac)
    raise ValueError(f"Unknown classification dataset name: {dataset_name} (synthetic-classify | class-folder)")
