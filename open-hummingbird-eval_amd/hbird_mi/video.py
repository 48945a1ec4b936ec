"""Semi-supervised video object segmentation by label propagation (the DAVIS-2017 J&F column of DINO and of most papers that use
Hummingbird), on the device: include/hbird_hip_propagate.h holds the definitions, which are this engine's own -- DINO's
eval_video_segmentation.py and the DAVIS-2017 toolkit restated from memory; no J&F figure has been held to a published one.

Per sequence: every frame's tokens (normalised rows), a pool of 1 + n_last_frames frames -- slot 0 the first frame with the patch shares of
its annotation as label rows (`ops.patch_label_hist`: the project's convention; DINO samples the annotation NEAREST), slots 1.. a ring of
the last predicted frames -- and for every later frame ONE `ops.propagate_labels` call over [first frame] + [the last frames, oldest first],
whose output rows go unnormalised into the ring.  The rows become label maps (`ops.mask_upsample_argmax`) and the maps the six counts per
object (`ops.mask_jf_counts`) in batches; the host finishes J and F in float64.  One process, one device.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from hbird_mi import _lib, ops


def ring_context(t: int, n_last_frames: int) -> Tuple[List[int], List[int]]:
    """The context of frame t >= 1 as (frames, pool slots): the first frame, then the last min(t - 1, n_last_frames) frames, oldest first.
    Frame u >= 1 lives in slot 1 + (u - 1) % n_last_frames."""
    if t < 1 or n_last_frames < 0:
        raise ValueError(f"ring_context: t={t} must be >= 1 and n_last_frames={n_last_frames} >= 0")
    frames = [0] + list(range(max(1, t - n_last_frames), t))
    return frames, [0 if u == 0 else 1 + (u - 1) % n_last_frames for u in frames]


def boundary_bound(h: int, w: int) -> int:
    """bound_px of the boundary measure: ceil(0.008 * the frame's diagonal)."""
    return int(math.ceil(0.008 * math.hypot(h, w)))


def jf_from_counts(counts) -> Tuple[np.ndarray, np.ndarray]:
    """counts [..., 6] in the order of _lib.JF_COUNTS -> (J, F) float64 [...] with the empty cases of include/hbird_hip_propagate.h."""
    c = np.asarray(counts, dtype=np.float64)
    inter, union, nfg, ngt, fgm, gtm = (c[..., i] for i in range(6))
    J = np.where(union == 0, 1.0, inter / np.maximum(union, 1.0))
    p = np.where(nfg > 0, fgm / np.maximum(nfg, 1.0), 1.0)
    r = np.where(ngt > 0, gtm / np.maximum(ngt, 1.0), 1.0)
    p = np.where((nfg > 0) & (ngt == 0), 0.0, p)
    r = np.where((nfg == 0) & (ngt > 0), 0.0, r)
    F = np.where(p + r == 0, 0.0, 2.0 * p * r / np.where(p + r == 0, 1.0, p + r))
    return J, F


class VideoMetrics(dict):
    """{"J_mean", "J_recall", "F_mean", "F_recall", "J&F"}: means over all objects of all sequences (the DAVIS-2017 semi-supervised protocol)
    of the per-object means over frames 1 .. T - 2; recall is the share of those frames with a measure > 0.5.
    `.per_object` [{"sequence", "object", "J_mean", "J_recall", "F_mean", "F_recall", "n_frames"}], `.per_sequence` {name: the five figures over
    the sequence's objects, "n_objects", "n_frames"}, `.skipped` [(name, reason)] -- sequences that could not be scored are listed, never dropped
    silently -- and `.maps` {name: [T - 1, H, W] int64 (frames 1 .. T - 1, CPU)} where asked for."""

    def __init__(self, counts: Dict[str, np.ndarray], skipped: Optional[List[Tuple[str, str]]] = None, maps: Optional[Dict[str, torch.Tensor]] = None):
        super().__init__()
        self.counts = {name: np.asarray(c, dtype=np.int64) for name, c in counts.items()}
        self.skipped, self.maps = list(skipped or []), maps
        self.per_object: List[Dict[str, Any]] = []
        self.per_sequence: Dict[str, Dict[str, Any]] = {}
        keys = ("J_mean", "J_recall", "F_mean", "F_recall")
        for name, c in self.counts.items():
            if c.ndim != 3 or c.shape[2] != len(_lib.JF_COUNTS) or c.shape[0] < 1 or c.shape[1] < 1:
                raise ValueError(f"VideoMetrics: the counts of {name!r} must be [frames >= 1, objects >= 1, {len(_lib.JF_COUNTS)}], got {c.shape}")
            J, F = jf_from_counts(c)
            rows = []
            for o in range(c.shape[1]):
                rows.append({"sequence": name, "object": o + 1, "J_mean": float(J[:, o].mean()), "J_recall": float((J[:, o] > 0.5).mean()),
                             "F_mean": float(F[:, o].mean()), "F_recall": float((F[:, o] > 0.5).mean()), "n_frames": int(c.shape[0])})
            self.per_object += rows
            seq = {k: float(np.mean([r[k] for r in rows])) for k in keys}
            seq.update({"J&F": 0.5 * (seq["J_mean"] + seq["F_mean"]), "n_objects": int(c.shape[1]), "n_frames": int(c.shape[0])})
            self.per_sequence[name] = seq
        for k in keys:
            self[k] = float(np.mean([r[k] for r in self.per_object])) if self.per_object else float("nan")
        self["J&F"] = 0.5 * (self["J_mean"] + self["F_mean"])


class HbirdVideoEvaluation:
    """`feature_extractor.forward_features(frames [b,3,H,W]) -> (tokens [b, (H / ps)(W / ps), D], _)`; frames need not be square (extractors
    that only take squares are fed square frames).  first_frame_radius=None means the same as `radius`; -1 means unrestricted.
    Token rows whose width is no multiple of 4 are padded with zero columns after the normalisation (a zero adds nothing to a score's chain)."""

    def __init__(self, feature_extractor: torch.nn.Module, patch_size: int, n_neighbours: int = 5, temperature: float = 0.1, n_last_frames: int = 7,
                 radius: int = 12, first_frame_radius: Optional[int] = None, channel_norm: bool = True, device: torch.device | str = "cuda"):
        for name, v, lo in (("patch_size", patch_size, 1), ("n_neighbours", n_neighbours, 1), ("n_last_frames", n_last_frames, 0), ("radius", radius, -1)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"{name}={v!r} must be an integer >= {lo}")
        if n_neighbours > _lib.PROPAGATE_MAX_K:
            raise ValueError(f"n_neighbours={n_neighbours} exceeds {_lib.PROPAGATE_MAX_K}")
        if 1 + n_last_frames > _lib.PROPAGATE_MAX_CTX:
            raise ValueError(f"n_last_frames={n_last_frames}: the context holds at most {_lib.PROPAGATE_MAX_CTX} frames with the first one")
        if first_frame_radius is not None and (isinstance(first_frame_radius, bool) or not isinstance(first_frame_radius, int) or first_frame_radius < -1):
            raise ValueError(f"first_frame_radius={first_frame_radius!r} must be None, -1 (unrestricted) or a radius >= 0")
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (math.isfinite(temperature) and temperature > 0):
            raise ValueError(f"temperature={temperature!r}: the softmax temperature must be a finite positive number")
        self.patch_size, self.n_neighbours, self.temperature, self.n_last_frames = patch_size, n_neighbours, float(temperature), n_last_frames
        self.radius = radius
        self.first_frame_radius = radius if first_frame_radius is None else first_frame_radius
        self.channel_norm = bool(channel_norm)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device={device!r}: the video evaluation runs on a GPU")
        if not torch.cuda.is_available():
            raise RuntimeError("HbirdVideoEvaluation needs an MI355X: the HIP path has no CPU fallback")
        self.gpu_device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.feature_extractor = feature_extractor.to(self.gpu_device).eval()

    # ---- one sequence ------------------------------------------------------------------------------------------------------------------------
    def tokens(self, frames: torch.Tensor, frame_batch: int = 8) -> torch.Tensor:
        """frames [T,3,H,W] -> normalised token rows [T, N, D'] fp32 on the device, D' = D rounded up to a multiple of 4 with zero columns."""
        T, _, H, W = frames.shape
        ps = self.patch_size
        N = (H // ps) * (W // ps)
        out = []
        for b0 in range(0, T, frame_batch):
            feats, _ = self.feature_extractor.forward_features(frames[b0:b0 + frame_batch].to(self.gpu_device))
            if feats.dim() != 3 or feats.shape[1] != N:
                raise ValueError(f"the feature extractor returned tokens of shape {tuple(feats.shape)} for {H} x {W} frames: expected "
                                 f"(H / ps)(W / ps) = {N} tokens per frame at patch size {ps} (does the extractor drop its class token?)")
            out.append(ops.normalize_rows(feats.to(self.gpu_device, dtype=torch.float32).contiguous()))
        tok = torch.cat(out, dim=0)
        pad = -tok.shape[2] % 4
        if pad:
            tok = torch.nn.functional.pad(tok, (0, pad))
        return tok.contiguous()

    def propagate_sequence(self, frames: torch.Tensor, first_annotation: torch.Tensor, n_objects: int, frame_batch: int = 8,
                           want_neighbours: bool = False):
        """-> rows [T - 1, N, n_objects + 1] fp32 (frames 1 .. T - 1) -- and with `want_neighbours` the per-frame (idx, score) lists too."""
        T, _, H, W = frames.shape
        ps, c = self.patch_size, n_objects + 1
        if H % ps or W % ps:
            raise ValueError(f"frames are {H} x {W}: both sides must be multiples of the patch size {ps}")
        if c > _lib.PROPAGATE_MAX_C:
            raise ValueError(f"{n_objects} objects: at most {_lib.PROPAGATE_MAX_C - 1}")
        gh, gw = H // ps, W // ps
        N = gh * gw
        tok = self.tokens(frames, frame_batch)
        feat_pool = torch.zeros((1 + self.n_last_frames, N, tok.shape[2]), dtype=torch.float32, device=self.gpu_device)
        label_pool = torch.zeros((1 + self.n_last_frames, N, c), dtype=torch.float32, device=self.gpu_device)
        feat_pool[0] = tok[0]
        ann0 = first_annotation.to(self.gpu_device, dtype=torch.int64).view(1, 1, H, W)
        label_pool[0] = ops.patch_label_hist(ann0, ps, c).view(N, c)
        rows = torch.empty((T - 1, N, c), dtype=torch.float32, device=self.gpu_device)
        lists = []
        for t in range(1, T):
            _, slots = ring_context(t, self.n_last_frames)
            radii = [self.first_frame_radius] + [self.radius] * (len(slots) - 1)
            got = ops.propagate_labels(tok[t], feat_pool, label_pool, slots, radii, (gh, gw), k=self.n_neighbours, temperature=self.temperature,
                                       want_neighbours=want_neighbours)
            if want_neighbours:
                lists.append((got[1], got[2]))
                got = got[0]
            rows[t - 1] = got
            if self.n_last_frames:
                slot = 1 + (t - 1) % self.n_last_frames           # (the oldest ring frame's slot: this call, enqueued before, has read it)
                feat_pool[slot] = tok[t]
                label_pool[slot] = got
        return (rows, lists) if want_neighbours else rows

    def evaluate(self, sequences: Iterable, frame_batch: int = 8, return_maps: bool = False) -> VideoMetrics:
        """sequences yield (name, frames [T,3,H,W] float, annotations [T,H,W] int64); objects are the ids 1 .. n of the first annotation."""
        counts: Dict[str, np.ndarray] = {}
        skipped: List[Tuple[str, str]] = []
        maps: Optional[Dict[str, torch.Tensor]] = {} if return_maps else None
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for name, frames, ann in sequences:
                if frames.dim() != 4 or ann.dim() != 3 or ann.shape[0] != frames.shape[0] or tuple(ann.shape[1:]) != tuple(frames.shape[2:]):
                    raise ValueError(f"sequence {name!r}: frames [T,3,H,W] and annotations [T,H,W] disagree: {tuple(frames.shape)} and {tuple(ann.shape)}")
                if name in counts:
                    raise ValueError(f"sequence {name!r} came twice")
                T, _, H, W = frames.shape
                ann = ann.to(torch.int64)
                n = int(ann[0].max()) if ann[0].numel() else 0
                if T < 3:
                    skipped.append((name, f"{T} frames: the measures are means over frames 1 .. T - 2"))
                    continue
                if n < 1 or int(ann[0].min()) < 0:
                    skipped.append((name, "the first annotation holds no object id >= 1" if n < 1 else "the first annotation holds a negative id"))
                    continue
                rows = self.propagate_sequence(frames, ann[0], n, frame_batch)
                bound = boundary_bound(H, W)
                if bound > _lib.JF_MAX_BOUND:
                    raise ValueError(f"sequence {name!r}: {H} x {W} frames give a boundary tolerance of {bound} px, beyond {_lib.JF_MAX_BOUND}")
                gt = ann.to(self.gpu_device)
                seq_counts, seq_maps = [], []
                for b0 in range(0, T - 1, frame_batch):
                    b1 = min(T - 1, b0 + frame_batch)
                    pred = ops.mask_upsample_argmax(rows[b0:b1], (H // self.patch_size, W // self.patch_size), H, W, self.channel_norm)
                    e = min(b1, T - 2)                              # rows[i] is frame i + 1; the last frame is not scored
                    if e > b0:
                        seq_counts.append(ops.mask_jf_counts(pred[:e - b0], gt[b0 + 1:e + 1].contiguous(), n, bound).cpu().numpy())
                    if return_maps:
                        seq_maps.append(pred.cpu())
                counts[name] = np.concatenate(seq_counts, axis=0)
                if return_maps:
                    maps[name] = torch.cat(seq_maps, dim=0)
        return VideoMetrics(counts, skipped, maps)


last_run_info: Dict[str, Any] = {}


def hbird_video_evaluation(model, d_model: int, patch_size: int, dataset_name: str, data_dir: str, input_size: int = 480, frame_batch: int = 8,
                           device: str | torch.device = "cuda", n_neighbours: int = 5, temperature: float = 0.1, n_last_frames: int = 7,
                           radius: int = 12, first_frame_radius: Optional[int] = None, channel_norm: bool = True, ftr_extr_fn=None,
                           val_fs_path: Optional[str] = None, resolution: str = "480p", return_maps: bool = False) -> VideoMetrics:
    """The function form: dataset_name "synthetic-video" or "video-folder" (hbird_mi/data/video.py), the model wrapped as `hbird_evaluation`
    wraps it."""
    from hbird_mi.data.video import get_video_dataset
    from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
    S = max(1, int(input_size) // int(patch_size))
    if ftr_extr_fn is None:
        extractor = FeatureExtractor(model, eval_spatial_resolution=S, d_model=d_model)
    else:
        extractor = FeatureExtractorSimple(model, ftr_extr_fn=ftr_extr_fn, eval_spatial_resolution=S, d_model=d_model)
    dataset = get_video_dataset(dataset_name, data_dir, input_size=input_size, patch_size=patch_size, val_fs_path=val_fs_path, resolution=resolution)
    ev = HbirdVideoEvaluation(extractor, patch_size, n_neighbours=n_neighbours, temperature=temperature, n_last_frames=n_last_frames, radius=radius,
                              first_frame_radius=first_frame_radius, channel_norm=channel_norm, device=device)
    res = ev.evaluate(dataset.sequences(), frame_batch=frame_batch, return_maps=return_maps)
    last_run_info.clear()
    last_run_info.update(n_sequences=len(res.per_sequence), n_objects=len(res.per_object))
    return res
