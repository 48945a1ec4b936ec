"""Data modules of the video evaluation (hbird_mi/video.py): `sequences()` yields `(name, frames [T,3,H,W] float, annotations [T,H,W] int64)`
with H and W multiples of the patch size; the objects of a sequence are the ids 1 .. n of its first annotation, 0 is background.

  * "synthetic-video" -- `SyntheticVideoDataModule`: coloured rectangles drift over a noisy background, so that colour determines the object
                         (no files; the tests and the CLI's self-check), and
  * "video-folder"    -- `VideoFolderDataModule`: the DAVIS layout, JPEGImages/<res>/<seq>/*.jpg with Annotations/<res>/<seq>/*.png (palette
                         index = object id) and an optional ImageSets/2017/val.txt.
"""
from __future__ import annotations

import os
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch

# background first; the objects' colours are far from it and from each other (cosine <= 0)
_PALETTE = ((1.0, 1.0, 1.0), (2.0, -1.0, -1.0), (-1.0, 2.0, -1.0), (-1.0, -1.0, 2.0), (-2.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, -2.0))


class SyntheticVideoDataModule:
    """n_sequences sequences of n_frames frames, H x W = frame_size (H != W by default): n_objects rectangles of colour _PALETTE[id] + noise drift
    `step` pixels per frame over a background of colour _PALETTE[0] + noise; a later object covers an earlier one.  A rectangle travels
    several times its own size over a sequence, so copying the first annotation to every frame scores badly while a patch's colour still
    says which object it belongs to.  Deterministic (own torch.Generator)."""

    def __init__(self, n_sequences: int = 2, n_frames: int = 10, frame_size: Tuple[int, int] = (48, 64), n_objects: int = 2, step: int = 4,
                 rect: Tuple[int, int] = (16, 16), noise: float = 0.1, seed: int = 0):
        H, W = (int(v) for v in frame_size)
        if not 1 <= n_objects < len(_PALETTE):
            raise ValueError(f"SyntheticVideoDataModule: n_objects={n_objects} must lie in [1, {len(_PALETTE) - 1}]")
        if rect[0] > H or rect[1] + step * (n_frames - 1) > W:
            raise ValueError(f"SyntheticVideoDataModule: a {rect[0]} x {rect[1]} rectangle drifting {step} px over {n_frames} frames leaves a {H} x {W} frame")
        self.n_sequences, self.n_frames, self.frame_size, self.n_objects, self.step, self.rect, self.noise = (
            n_sequences, n_frames, (H, W), n_objects, int(step), (int(rect[0]), int(rect[1])), float(noise))
        g = torch.Generator().manual_seed(seed)
        self._seqs = [self._make(i, g) for i in range(n_sequences)]

    def _make(self, i: int, g) -> Tuple[str, torch.Tensor, torch.Tensor]:
        (H, W), T, (rh, rw) = self.frame_size, self.n_frames, self.rect
        pal = torch.tensor(_PALETTE)
        travel = self.step * (T - 1)
        ann = torch.zeros((T, H, W), dtype=torch.int64)
        for o in range(1, self.n_objects + 1):
            y0 = int(torch.randint(0, H - rh + 1, (1,), generator=g))
            x0 = int(torch.randint(0, W - rw - travel + 1, (1,), generator=g))
            back = bool(torch.randint(0, 2, (1,), generator=g))           # right to left
            for t in range(T):
                x = x0 + (travel - self.step * t if back else self.step * t)
                ann[t, y0:y0 + rh, x:x + rw] = o
        frames = pal[ann].permute(0, 3, 1, 2) + self.noise * torch.randn((T, 3, H, W), generator=g)
        return f"synthetic-{i:02d}", frames.float().contiguous(), ann

    def sequences(self) -> Iterator[Tuple[str, torch.Tensor, torch.Tensor]]:
        return iter(self._seqs)

    def __len__(self):
        return len(self._seqs)


# ---- folders -------------------------------------------------------------------------------------------------------------------------------
def resized_hw(h: int, w: int, input_size: int, patch_size: int) -> Tuple[int, int]:
    """The frame size after the resize: the short side becomes input_size, and both sides the nearest multiples of the patch size (at least one
    patch)."""
    scale = float(input_size) / float(min(h, w))
    return tuple(max(patch_size, int(round(v * scale / patch_size)) * patch_size) for v in (h, w))


class VideoFolderDataModule:
    """<root>/JPEGImages/<res>/<seq>/<frame>.jpg and <root>/Annotations/<res>/<seq>/<frame>.png (palette index = object id).  The sequences
    are those of <root>/ImageSets/2017/val.txt where it exists (or of `val_fs_path`), else every folder under JPEGImages/<res>, in sorted order.
    Frames are resized BILINEAR so that the short side is `input_size` and both sides are multiples of the patch size, and go through
    folder.py's tensor conversion (ImageNet normalisation); annotations are resized NEAREST.  A frame without an annotation file (the
    toolkit's test splits carry the first one only) gets a map of zeros."""

    def __init__(self, data_dir: str, input_size: int, patch_size: int, resolution: str = "480p", val_fs_path: Optional[str] = None):
        from .folder import open_store, read_file_set
        self.store, self.input_size, self.patch_size, self.res = open_store(data_dir), int(input_size), int(patch_size), resolution
        self.img_root, self.ann_root = f"JPEGImages/{resolution}", f"Annotations/{resolution}"
        if not (self.store.isdir(self.img_root) and self.store.isdir(self.ann_root)):
            raise RuntimeError(f"Dataset not found or corrupted: no {self.img_root} and {self.ann_root} under {data_dir}")
        split = "ImageSets/2017/val.txt"
        if val_fs_path:
            names = read_file_set(val_fs_path)
        elif self.store.isdir("ImageSets/2017") and "val.txt" in self.store.listdir("ImageSets/2017"):
            with self.store.open(split) as f:
                data = f.read()
            names = [ln.strip() for ln in (data.decode() if isinstance(data, bytes) else data).splitlines() if ln.strip()]
        else:
            names = sorted(n for n in self.store.listdir(self.img_root) if self.store.isdir(f"{self.img_root}/{n}"))
        for n in names:
            if not self.store.isdir(f"{self.img_root}/{n}"):
                raise RuntimeError(f"Dataset not found or corrupted: sequence {n!r} has no folder under {self.img_root}")
        if not names:
            raise RuntimeError(f"Dataset not found or corrupted: no sequences under {data_dir}/{self.img_root}")
        self.names: List[str] = names

    def __len__(self):
        return len(self.names)

    def load(self, name: str) -> Tuple[str, torch.Tensor, torch.Tensor]:
        from PIL import Image
        from .folder import _to_tensor_img, _wh
        files = sorted(f for f in self.store.listdir(f"{self.img_root}/{name}") if f.lower().endswith((".jpg", ".jpeg", ".png")))
        if not files:
            raise RuntimeError(f"Dataset not found or corrupted: sequence {name!r} holds no frames")
        have = set(self.store.listdir(f"{self.ann_root}/{name}")) if self.store.isdir(f"{self.ann_root}/{name}") else set()
        frames, anns, hw = [], [], None
        for f in files:
            with self.store.open(f"{self.img_root}/{name}/{f}") as fh:
                img = Image.open(fh).convert("RGB")
            if hw is None:
                hw = resized_hw(img.height, img.width, self.input_size, self.patch_size)
            frames.append(_to_tensor_img(img.resize(_wh(hw), Image.BILINEAR)))
            png = os.path.splitext(f)[0] + ".png"
            if png in have:
                with self.store.open(f"{self.ann_root}/{name}/{png}") as fh:
                    m = Image.open(fh)
                    m.load()
                if m.mode not in ("P", "L", "I", "1"):
                    raise ValueError(f"{self.ann_root}/{name}/{png}: an annotation must be a palette or grey image (index = object id), got mode {m.mode}")
                anns.append(torch.from_numpy(np.array(m.resize(_wh(hw), Image.NEAREST), dtype=np.int64)))
            else:
                anns.append(torch.zeros(hw, dtype=torch.int64))
        return name, torch.stack(frames).contiguous(), torch.stack(anns).contiguous()

    def sequences(self) -> Iterator[Tuple[str, torch.Tensor, torch.Tensor]]:
        for name in self.names:
            yield self.load(name)


def get_video_dataset(dataset_name: str, data_dir: str = "", input_size: int = 480, patch_size: int = 16, val_fs_path: Optional[str] = None,
                      resolution: str = "480p", **synthetic):
    """"synthetic-video" (input_size is not used: the world has its own frame size) or "video-folder" -> the data module."""
    name = dataset_name.strip().lower()
    if name == "synthetic-video":
        return SyntheticVideoDataModule(**synthetic)
    if name == "video-folder":
        if synthetic:
            raise TypeError(f"get_video_dataset: {sorted(synthetic)} are arguments of the synthetic world")
        return VideoFolderDataModule(data_dir, input_size, patch_size, resolution, val_fs_path)
    raise ValueError(f"Unknown video dataset name: {dataset_name} (synthetic-video | video-folder)")
