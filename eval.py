#!/usr/bin/env python3
"""Command-line front end (counterpart of the reference's eval.py:369-505): same flags, plus `--nn-method hip`.

  python eval.py --dataset-name voc --data-dir /data/VOCSegmentation --d-model 384 --patch-size 16 \\
      --input-size 224 --batch-size 64 --device cuda --nn-method hip --checkpoint dino_vits16.pth --timm-model vit_small_patch16_224
  python eval.py --dataset-name synthetic --data-dir "" --d-model 3 --patch-size 8 --input-size 64 --device cuda   # self-check
  python eval.py --task depth --dataset-name synthetic-depth --data-dir "" --d-model 3 --patch-size 8 --input-size 64   # depth self-check
  python eval.py --task depth-grid --grid-k 1 5 30 --grid-beta 0.02 0.1 --bootstrap 1000 --dataset-name synthetic-depth --data-dir "" \\
      --d-model 3 --patch-size 8 --input-size 64                                                                      # ... over a (k, beta) grid
  python eval.py --task knn-classify --dataset-name synthetic-classify --data-dir "" --d-model 3 --patch-size 8 --input-size 32   # image-level k-NN
  python eval.py --task linear-classify --probe-l2 1e-2 1e-3 --dataset-name synthetic-classify --data-dir "" --d-model 3 --patch-size 8 \\
      --input-size 32                                                                                                 # ... and the linear probe
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import random
import sys
import time
from typing import Any, Dict, List, Optional

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "open-hummingbird-eval_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _positive_int(v: str) -> int:
    i = int(v)
    if i <= 0:
        raise argparse.ArgumentTypeError("must be a positive integer")
    return i


def _positive_float(v: str) -> float:
    f = float(v)
    if not (f > 0 and f != float("inf")):
        raise argparse.ArgumentTypeError("must be a finite positive number")
    return f


def _non_negative_float(v: str) -> float:
    f = float(v)
    if not (f >= 0 and f != float("inf")):
        raise argparse.ArgumentTypeError("must be a finite non-negative number")
    return f


def grid_key(k: int, beta: float) -> str:
    """How a configuration of --grid-k / --grid-beta is keyed in the result JSON."""
    return f"k={int(k)},beta={float(beta)!r}"


def _level(v: str) -> float:
    f = float(v)
    if not 0.0 < f < 1.0:
        raise argparse.ArgumentTypeError("must lie strictly between 0 and 1")
    return f


def bootstrap_key(key) -> str:
    """How a MiouBootstrap key -- (k, beta), with --memory-sizes (size, k, beta) -- is keyed in the result JSON."""
    return grid_key(*key) if len(key) == 2 else f"memory_size={int(key[0])}," + grid_key(*key[1:])


def headline_key(keys, n_neighbours: int, memory_size):
    """The key behind the JSON's `miou`: the built bank's own size when listed (else the largest), the plain run's (k, 0.02) when the grid
    holds it (else the grid's first)."""
    keys = list(keys)
    if len(keys[0]) == 3:
        sizes = [k[0] for k in keys]
        size = memory_size if memory_size in sizes else max(sizes)
        keys = [k for k in keys if k[0] == size]
    want = (int(n_neighbours), 0.02)
    return next((k for k in keys if tuple(k[-2:]) == want), keys[0])


def bootstrap_summary(mb, level: float, head) -> Dict[str, Any]:
    """The JSON fields of --bootstrap out of a hbird_mi.bootstrap.MiouBootstrap."""
    out: Dict[str, Any] = {"miou_ci": [float(v) for v in mb.interval(head, level)],
                           "bootstrap": {"replicates": int(mb.samples.shape[0]), "seed": int(mb.seed), "level": float(level),
                                         "n_images": int(mb.n_images), "matching_is_identity": bool(all(mb.matching_is_identity.values()))}}
    if len(mb.keys) > 1:
        best, tied = mb.best(level)
        out["miou_grid_ci"] = {bootstrap_key(k): [float(v) for v in mb.interval(k, level)] for k in mb.keys}
        out["grid_best"] = bootstrap_key(best)
        out["grid_indistinguishable_from_best"] = [bootstrap_key(k) for k in tied]
    return out


def bootstrap_as_plain(mb, gridded: bool, sized: bool):
    """The value hbird_evaluation returns WITHOUT bootstrap= for the same flags, out of mb.miou."""
    if sized:
        by = {}
        for (size, k, b), v in mb.miou.items():
            by.setdefault(size, {})[(k, b)] = v
        return by if gridded else {size: next(iter(res.values())) for size, res in by.items()}
    return dict(mb.miou) if gridded else next(iter(mb.miou.values()))


def _non_negative_int(v: str) -> int:
    n = int(v)
    if n < 0:
        raise argparse.ArgumentTypeError(f"{v!r} must be >= 0")
    return n


def _radius(v: str) -> int:
    n = int(v)
    if n < -1:
        raise argparse.ArgumentTypeError(f"{v!r} must be a radius >= 0, or -1 for an unrestricted window")
    return n


class _DefaultInt(int):
    """An integer default that can be told from the same value typed on the command line (--n-neighbours: 30, and 5 with --task video)."""


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Hummingbird retrieval evaluation on MI355X (hbird_mi.hbird_evaluation).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--dataset-name", required=True, help="voc | ade20k | cityscapes | synthetic, optionally 'name*0.2'")
    p.add_argument("--data-dir", required=True)
    p.add_argument("--d-model", type=_positive_int, required=True)
    p.add_argument("--patch-size", type=_positive_int, required=True)
    p.add_argument("--batch-size", type=_positive_int, default=64)
    p.add_argument("--input-size", type=_positive_int, default=224)
    p.add_argument("--frame-size", type=_positive_int, nargs=2, default=None, metavar=("H", "W"),
                   help="deliver H x W frames and process them through --input-size sliding windows (not in the reference)")
    p.add_argument("--window-stride", type=_positive_int, default=None, help="stride of the sliding windows (default: input size)")
    p.add_argument("--augmentation-epoch", type=_positive_int, default=1)
    p.add_argument("--num-workers", type=int, default=8)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--amp", action="store_true", help="accepted for compatibility (unused, as in the reference)")
    p.add_argument("--n-neighbours", type=_positive_int, default=_DefaultInt(30), help="(--task video: 5 unless given)")
    p.add_argument("--nn-method", choices=["hip", "faiss", "scann"], default="hip")
    p.add_argument("--nn-param", action="append", default=[], metavar="KEY=VALUE")
    p.add_argument("--memory-size", type=int, default=None)
    p.add_argument("--memory-sizes", type=_positive_int, nargs="+", default=None, metavar="N",
                   help="memory-size sweep out of ONE bank build (not in the reference): the bank is built at --memory-size, every listed "
                        "size up to it is evaluated on a view of that bank; the result JSON then also carries miou_by_memory_size")
    p.add_argument("--grid-k", type=_positive_int, nargs="+", default=None, metavar="N",
                   help="sweep over n_neighbours out of ONE validation pass with one search per batch (not in the reference); the result JSON "
                        "then carries miou_grid, keyed 'k=30,beta=0.02' (with --memory-sizes: miou_grid_by_memory_size)")
    p.add_argument("--grid-beta", type=_positive_float, nargs="+", default=None, metavar="B",
                   help="sweep over the softmax temperature of the label aggregation (0.02 in the reference), see --grid-k")
    p.add_argument("--leave-one-out", action="store_true",
                   help="score on the TRAINING images instead of the validation split (not in the reference): every training image queries the "
                        "bank with its own rows excluded, so --grid-k / --grid-beta / --memory-sizes can be chosen without tuning on validation data")
    p.add_argument("--leave-one-out-images", type=_positive_int, default=None, metavar="N", help="stop the leave-one-out pass after N images")
    p.add_argument("--leave-one-out-screen", action="store_true",
                   help="with --leave-one-out: the certified fp16 screen serves the excluding searches where it applies (same scores; the cost of "
                        "plain searches at k instead of searches at k + the largest image's rows)")
    p.add_argument("--bootstrap", type=_positive_int, default=None, metavar="R",
                   help="R paired bootstrap replicates over the evaluated images (not in the reference): the result JSON gains miou_ci, and "
                        "with a grid or --memory-sizes miou_grid_ci, grid_best and grid_indistinguishable_from_best")
    p.add_argument("--bootstrap-seed", type=int, default=None, metavar="S", help="the resampler's seed (default: the library's)")
    p.add_argument("--bootstrap-level", type=_level, default=0.95, metavar="L", help="coverage of the percentile intervals")
    p.add_argument("--overclustering", type=_positive_int, nargs="+", default=None, metavar="K",
                   help="the overclustering protocol instead of the retrieval one (not in the reference's CLI): k-means over the bank into K "
                        "clusters, clusters matched to classes (Hungarian for K <= classes, many-to-one on precision beyond); the result JSON "
                        "then carries miou_overclustering, keyed 'clusters=K'")
    p.add_argument("--overclustering-seed", type=int, default=0, metavar="S", help="seed of the k-means initialisation")
    p.add_argument("--overclustering-iters", type=_positive_int, default=20, metavar="N", help="iteration limit of k-means")
    p.add_argument("--linear-probe", action="store_true",
                   help="the linear-head protocol instead of the retrieval one (not in the reference's CLI): a softmax head fitted on the bank "
                        "by L-BFGS, scored with the identity matching; the result JSON then carries miou_linear_probe and linear_probe_fit")
    p.add_argument("--linear-probe-l2", type=float, default=1e-3, metavar="X", help="l2 weight of the fit (a definition, not tuned on real data)")
    p.add_argument("--linear-probe-gtol", type=float, default=1e-5, metavar="X", help="the fit stops once the gradient's largest entry is this small")
    p.add_argument("--linear-probe-iters", type=int, default=200, metavar="N", help="iteration limit of the fit")
    p.add_argument("--task", choices=["segmentation", "depth", "depth-grid", "video", "knn-classify", "linear-classify"], default="segmentation",
                   help="knn-classify: the weighted k-NN classifier on image-level features (hbird_mi.classify; not in the reference) -- "
                        "--dataset-name synthetic-classify | class-folder (train/<class>/*, val/<class>/* under --data-dir), --grid-k (default 10 20 "
                        "100 200) x --grid-temperature (default 0.07) from one search per batch; the result JSON carries top1, top5 and "
                        "mean_per_class keyed 'k=20,T=0.07', best, n and skipped.  video: semi-supervised video object segmentation by label propagation (hbird_mi.video; not in the reference) -- "
                        "--dataset-name synthetic-video | video-folder (the DAVIS layout under --data-dir); the result JSON carries J_mean, J_recall, "
                        "F_mean, F_recall, J&F and per_sequence.  depth: monocular depth by retrieval (hbird_mi.depth; not in the reference's CLI) -- the bank stores each patch's local depth "
                        "values, the result JSON carries rmse, abs_rel, sq_rel, rmse_log, silog, log10, d1, d2, d3 (means of per-image metrics), "
                        "pooled, n_nopred and empty_images; --dataset-name synthetic-depth | depth-folder.  depth-grid: the same task over "
                        "--grid-k / --grid-beta / --memory-sizes from one pass, with --leave-one-out and --bootstrap (hbird_depth_grid_evaluation); "
                        "the result JSON carries depth_grid, keyed 'k=30,beta=0.02' (with --memory-sizes 'memory=N,k=30,beta=0.02')")
    p.add_argument("--bootstrap-metric", choices=["rmse", "abs_rel", "sq_rel", "rmse_log", "silog", "log10", "d1", "d2", "d3"], default="rmse",
                   help="--task depth-grid with --bootstrap: the metric grid_best and grid_indistinguishable_from_best are decided on")
    p.add_argument("--target-grid", type=_positive_int, default=1, metavar="R",
                   help="--task depth: R x R depth cells per patch (R divides the patch size; the patch size itself is the full-resolution label patch)")
    p.add_argument("--min-depth", type=_positive_float, default=1e-3, metavar="A", help="--task depth: smallest valid depth, metres")
    p.add_argument("--max-depth", type=_positive_float, default=10.0, metavar="B", help="--task depth: largest valid depth, metres")
    p.add_argument("--depth-scale", type=_positive_float, default=1000.0, metavar="X", help="--task depth: units per metre of 16-bit PNG depth files")
    p.add_argument("--video-last-frames", type=_non_negative_int, default=7, metavar="N", help="--task video: predicted frames kept as context")
    p.add_argument("--video-radius", type=_radius, default=12, metavar="R", help="--task video: window radius in cells around the query (-1: unrestricted)")
    p.add_argument("--video-first-frame-radius", type=_radius, default=None, metavar="R",
                   help="--task video: window radius on the first frame (default: --video-radius; -1: unrestricted)")
    p.add_argument("--video-temperature", type=_positive_float, default=0.1, metavar="T", help="--task video: softmax temperature of the propagation")
    p.add_argument("--grid-temperature", type=_positive_float, nargs="+", default=None, metavar="T",
                   help="--task knn-classify: the temperatures of the vote's weights exp(similarity / T) (default 0.07)")
    p.add_argument("--top-n", type=_positive_int, default=None, metavar="N",
                   help="--task knn-classify: predictions ranked per image, at most 8 (default 5: the JSON's top5 is the label among the first N)")
    p.add_argument("--probe-l2", type=_non_negative_float, nargs="+", default=None, metavar="L",
                   help="--task linear-classify: the l2 weights of the softmax head, one fit each, at most 16 (default 1e-3: a definition, not tuned)")
    p.add_argument("--no-channel-norm", action="store_true", help="--task video: argmax without the per-channel min-max normalisation of the label maps")
    p.add_argument("--ignore-index", type=int, default=255)
    p.add_argument("--train-fs", dest="train_fs_path", type=str, default=None)
    p.add_argument("--val-fs", dest="val_fs_path", type=str, default=None)
    p.add_argument("--timm-model", type=str, default=None)
    p.add_argument("--dinov2", type=str, choices=["vits14", "vitb14", "vitl14", "vitg14"], default=None)
    p.add_argument("--checkpoint", type=str, default=None)
    p.add_argument("--f-mem-p", type=str, default=None, help="feature-memory file: saved after the bank build; with --l-mem-p "
                   "and both files present the bank is loaded instead of rebuilt (the reference's f_mem_p, never reachable from its CLI)")
    p.add_argument("--l-mem-p", type=str, default=None, help="label-memory file (see --f-mem-p)")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--out", type=str, default=None)
    p.add_argument("--log-level", choices=["DEBUG", "INFO", "WARNING", "ERROR"], default="INFO")
    return p


def parse_nn_params(kv_list: List[str]) -> Dict[str, Any]:
    """KEY=VALUE -> bool / int / float / str (reference eval.py:444-462)."""
    out: Dict[str, Any] = {}
    for kv in kv_list:
        if "=" not in kv:
            raise argparse.ArgumentTypeError(f"Invalid --nn-param '{kv}'. Use KEY=VALUE.")
        k, v = (s.strip() for s in kv.split("=", 1))
        if v.lower() in {"true", "false"}:
            out[k] = v.lower() == "true"
        else:
            for cast in (int, float):
                try:
                    out[k] = cast(v)
                    break
                except ValueError:
                    continue
            else:
                out[k] = v
        # a comma-separated list of GPU ids (`gpu_ids=0,1,2,3`; a single id has become an int above): the reference's parser has no
        # list form, its Faiss class iterates over whatever it gets (search_faiss.py:22)
        if k == "gpu_ids":
            val = out[k]
            out[k] = [val] if isinstance(val, int) else [int(t) for t in str(val).strip("[]").split(",") if t.strip()]
    return out


def set_seed(seed: Optional[int]) -> None:
    if seed is None:
        return
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class _PatchPool(torch.nn.Module):
    """Stand-in 'backbone' for the synthetic self-check: average-pools patches of the input image."""

    def __init__(self, patch):
        super().__init__()
        self.patch = patch

    def forward(self, x):
        return torch.nn.functional.avg_pool2d(x, self.patch).flatten(2).transpose(1, 2)


def build_model(args) -> torch.nn.Module:
    if args.dataset_name.split("*")[0] in ("synthetic", "synthetic-depth", "synthetic-video", "synthetic-classify") and not (args.timm_model or args.dinov2):
        return _PatchPool(args.patch_size)
    if args.dinov2:
        model = torch.hub.load("facebookresearch/dinov2", f"dinov2_{args.dinov2}")          # eval.py:213 (needs a hub cache)
    elif args.timm_model:
        import timm
        model = timm.create_model(args.timm_model, pretrained=args.checkpoint is None, num_classes=0)
    else:
        raise SystemExit("one of --timm-model / --dinov2 is required for real datasets")
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        sd = sd.get("state_dict", sd.get("model", sd))
        missing, unexpected = model.load_state_dict(sd, strict=False)
        logging.info("checkpoint loaded (missing %d, unexpected %d keys)", len(missing), len(unexpected))
    return model


def default_ftr_extr_fn(model, imgs):
    """Token extraction of the reference CLI (eval.py:262-309): prefer x_norm_patchtokens, else drop CLS."""
    out = model.forward_features(imgs) if hasattr(model, "forward_features") else model(imgs)
    if isinstance(out, dict):
        out = out.get("x_norm_patchtokens", next(iter(out.values())))
    if out.dim() == 3:
        n = out.shape[1]
        r = int(round((n - 1) ** 0.5))
        if int(round(n ** 0.5)) ** 2 != n and r * r == n - 1:
            out = out[:, 1:]
    return out, None


DEPTH_EXCLUDES = ("frame_size", "window_stride", "memory_sizes", "grid_k", "grid_beta", "leave_one_out", "bootstrap", "overclustering",
                  "linear_probe", "f_mem_p", "l_mem_p")


def main_depth(parser, args) -> None:
    """--task depth: hbird_mi.depth.hbird_depth_evaluation and its JSON."""
    for name in DEPTH_EXCLUDES:
        if getattr(args, name):
            parser.error(f"--{name.replace('_', '-')} is not available with --task depth")
    logging.basicConfig(level=getattr(logging, args.log_level), force=True)
    set_seed(args.seed)
    from hbird_mi import depth as hdepth
    model = build_model(args)
    t0 = time.time()
    res = hdepth.hbird_depth_evaluation(model, d_model=args.d_model, patch_size=args.patch_size, dataset_name=args.dataset_name,
                                        data_dir=args.data_dir, batch_size=args.batch_size, input_size=args.input_size,
                                        augmentation_epoch=args.augmentation_epoch, device=args.device, n_neighbours=args.n_neighbours,
                                        nn_method=args.nn_method, nn_params=parse_nn_params(args.nn_param), ftr_extr_fn=default_ftr_extr_fn,
                                        memory_size=args.memory_size, num_workers=args.num_workers, target_grid=args.target_grid,
                                        min_depth=args.min_depth, max_depth=args.max_depth, depth_scale=args.depth_scale,
                                        train_fs_path=args.train_fs_path, val_fs_path=args.val_fs_path)
    summary = {"task": "depth", **{k: float(v) for k, v in res.items()}, "pooled": res.pooled, "n_nopred": res.n_nopred,
               "n_pixels": res.n_pixels, "n_images": len(res.per_image), "empty_images": res.empty_images, "target_grid": args.target_grid,
               "min_depth": args.min_depth, "max_depth": args.max_depth, "seconds": round(time.time() - t0, 3), "nn_method": args.nn_method,
               "dataset": args.dataset_name, "n_neighbours": args.n_neighbours, **hdepth.last_run_info}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f)


DEPTH_GRID_EXCLUDES = ("frame_size", "window_stride", "overclustering", "linear_probe", "f_mem_p", "l_mem_p")


def depth_grid_key(key) -> str:
    """How a configuration of --task depth-grid -- (k, beta), with --memory-sizes (size, k, beta) -- is keyed in the result JSON."""
    return grid_key(*key) if len(key) == 2 else f"memory={int(key[0])}," + grid_key(*key[1:])


def main_depth_grid(parser, args) -> None:
    """--task depth-grid: hbird_mi.depth.hbird_depth_grid_evaluation and its JSON."""
    for name in DEPTH_GRID_EXCLUDES:
        if getattr(args, name):
            parser.error(f"--{name.replace('_', '-')} is not available with --task depth-grid")
    if (args.leave_one_out_images is not None or args.leave_one_out_screen) and not args.leave_one_out:
        parser.error("--leave-one-out-images and --leave-one-out-screen need --leave-one-out")
    if args.memory_sizes and args.memory_size is None:
        parser.error("--memory-sizes needs --memory-size")
    logging.basicConfig(level=getattr(logging, args.log_level), force=True)
    set_seed(args.seed)
    from hbird_mi import depth as hdepth
    model = build_model(args)
    t0 = time.time()
    res = hdepth.hbird_depth_grid_evaluation(model, d_model=args.d_model, patch_size=args.patch_size, dataset_name=args.dataset_name,
                                             data_dir=args.data_dir, batch_size=args.batch_size, input_size=args.input_size,
                                             augmentation_epoch=args.augmentation_epoch, device=args.device, n_neighbours=args.n_neighbours,
                                             nn_method=args.nn_method, nn_params=parse_nn_params(args.nn_param), ftr_extr_fn=default_ftr_extr_fn,
                                             memory_size=args.memory_size, num_workers=args.num_workers, target_grid=args.target_grid,
                                             min_depth=args.min_depth, max_depth=args.max_depth, depth_scale=args.depth_scale,
                                             train_fs_path=args.train_fs_path, val_fs_path=args.val_fs_path, grid_k=args.grid_k,
                                             grid_beta=args.grid_beta, memory_sizes=args.memory_sizes, leave_one_out=args.leave_one_out,
                                             leave_one_out_images=args.leave_one_out_images, leave_one_out_screen=args.leave_one_out_screen,
                                             bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed)
    boot = res if args.bootstrap else None
    metrics = boot.metrics if boot is not None else res
    head = headline_key(list(metrics), args.n_neighbours, args.memory_size)
    summary = {"task": "depth-grid", **{k: float(v) for k, v in metrics[head].items()}, "headline": depth_grid_key(head),
               "depth_grid": {depth_grid_key(key): {**{k: float(v) for k, v in m.items()}, "pooled": m.pooled, "n_nopred": m.n_nopred,
                                                    "empty_images": m.empty_images} for key, m in metrics.items()},
               "n_images": len(metrics[head].per_image), "target_grid": args.target_grid, "min_depth": args.min_depth, "max_depth": args.max_depth,
               "seconds": round(time.time() - t0, 3), "nn_method": args.nn_method, "dataset": args.dataset_name, "n_neighbours": args.n_neighbours,
               **hdepth.last_run_info}
    if args.leave_one_out:
        summary["leave_one_out"] = True
    if boot is not None:
        level, metric = args.bootstrap_level, args.bootstrap_metric
        best, tied = boot.best(metric, level)
        summary.update({f"{m}_ci": [float(v) for v in boot.interval(head, m, level)] for m in ("rmse", "abs_rel", "d1")})
        summary.update(grid_best=depth_grid_key(best), grid_indistinguishable_from_best=[depth_grid_key(k) for k in tied],
                       bootstrap={"replicates": int(boot.samples[metric].shape[0]), "seed": int(boot.seed), "level": float(level),
                                  "metric": metric, "n_images": int(boot.n_images)})
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f)


VIDEO_EXCLUDES = DEPTH_EXCLUDES + ("memory_size", "leave_one_out_images", "leave_one_out_screen", "train_fs_path")
VIDEO_ONLY = {"video_last_frames": 7, "video_radius": 12, "video_first_frame_radius": None, "video_temperature": 0.1, "no_channel_norm": False}


def main_video(parser, args) -> None:
    """--task video: hbird_mi.video.hbird_video_evaluation and its JSON."""
    for name in VIDEO_EXCLUDES:
        if getattr(args, name):
            parser.error(f"--{name.replace('_', '-').replace('-path', '')} is not available with --task video")
    if args.nn_method != "hip" or args.nn_param:
        parser.error("--nn-method and --nn-param are not available with --task video (the propagation has one kernel)")
    if args.augmentation_epoch != 1 or args.target_grid != 1:
        parser.error("--augmentation-epoch and --target-grid are not available with --task video")
    k = 5 if isinstance(args.n_neighbours, _DefaultInt) else int(args.n_neighbours)
    logging.basicConfig(level=getattr(logging, args.log_level), force=True)
    set_seed(args.seed)
    from hbird_mi import video as hvideo
    model = build_model(args)
    t0 = time.time()
    res = hvideo.hbird_video_evaluation(model, d_model=args.d_model, patch_size=args.patch_size, dataset_name=args.dataset_name,
                                        data_dir=args.data_dir, input_size=args.input_size, frame_batch=args.batch_size, device=args.device,
                                        n_neighbours=k, temperature=args.video_temperature, n_last_frames=args.video_last_frames,
                                        radius=args.video_radius, first_frame_radius=args.video_first_frame_radius,
                                        channel_norm=not args.no_channel_norm, ftr_extr_fn=default_ftr_extr_fn, val_fs_path=args.val_fs_path)
    summary = {"task": "video", **{key: float(v) for key, v in res.items()}, "per_sequence": res.per_sequence,
               "skipped": [list(s) for s in res.skipped], "n_objects": len(res.per_object), "n_neighbours": k,
               "temperature": args.video_temperature, "last_frames": args.video_last_frames, "radius": args.video_radius,
               "first_frame_radius": args.video_radius if args.video_first_frame_radius is None else args.video_first_frame_radius,
               "channel_norm": not args.no_channel_norm, "seconds": round(time.time() - t0, 3), "dataset": args.dataset_name}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f)


KNN_EXCLUDES = ("frame_size", "window_stride", "memory_size", "grid_beta", "bootstrap", "overclustering", "linear_probe", "f_mem_p", "l_mem_p",
                "leave_one_out_screen", "train_fs_path", "val_fs_path")
KNN_ONLY = {"grid_temperature": None, "top_n": None}


def classify_key(k: int, T: float) -> str:
    """How a configuration of --task knn-classify is keyed in the result JSON."""
    return f"k={int(k)},T={float(T)!r}"


def main_knn_classify(parser, args) -> None:
    """--task knn-classify: hbird_mi.classify.hbird_knn_classification and its JSON."""
    if args.memory_sizes:
        parser.error("--memory-sizes is not available with --task knn-classify: the bank holds one row per image (label subsets: "
                     "HbirdKnnClassification.memory_view)")
    for name in KNN_EXCLUDES:
        if getattr(args, name):
            parser.error(f"--{name.replace('_', '-').replace('-path', '')} is not available with --task knn-classify")
    if not isinstance(args.n_neighbours, _DefaultInt):
        parser.error("--n-neighbours is not available with --task knn-classify: give --grid-k")
    if args.nn_method != "hip":
        parser.error("--nn-method is not available with --task knn-classify (the vote reads the HIP index's lists)")
    if args.target_grid != 1:
        parser.error("--target-grid is not available with --task knn-classify")
    if args.leave_one_out_images is not None and not args.leave_one_out:
        parser.error("--leave-one-out-images needs --leave-one-out")
    top_n = 5 if args.top_n is None else args.top_n
    if top_n > 8:
        parser.error("--top-n: at most 8 predictions are ranked per image")
    ks = args.grid_k or [10, 20, 100, 200]
    temps = args.grid_temperature or [0.07]
    logging.basicConfig(level=getattr(logging, args.log_level), force=True)
    set_seed(args.seed)
    from hbird_mi import classify as hclassify
    model = build_model(args)
    t0 = time.time()
    res = hclassify.hbird_knn_classification(model, d_model=args.d_model, patch_size=args.patch_size, dataset_name=args.dataset_name,
                                             data_dir=args.data_dir, batch_size=args.batch_size, input_size=args.input_size,
                                             augmentation_epoch=args.augmentation_epoch, device=args.device, n_neighbours=ks, temperatures=temps,
                                             topn=top_n, nn_params=parse_nn_params(args.nn_param), ftr_extr_fn=default_ftr_extr_fn,
                                             num_workers=args.num_workers, leave_one_out=args.leave_one_out,
                                             leave_one_out_images=args.leave_one_out_images)
    best, best_top1 = res.best() if res.n else (None, float("nan"))
    summary = {"task": "knn-classify", "top1": {classify_key(*c): float(res.top1[c]) for c in res.configs},
               f"top{top_n}": {classify_key(*c): float(res.topn[c]) for c in res.configs},
               "mean_per_class": {classify_key(*c): float(res.mean_per_class[c]) for c in res.configs},
               "best": None if best is None else {"key": classify_key(*best), "top1": float(best_top1)}, "n": res.n, "skipped": res.skipped,
               "top_n": top_n, "seconds": round(time.time() - t0, 3), "dataset": args.dataset_name, **hclassify.last_run_info}
    if args.leave_one_out:
        summary["leave_one_out"] = True
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f)


def probe_key(l2: float) -> str:
    """How a configuration of --task linear-classify is keyed in the result JSON."""
    return f"l2={float(l2)!r}"


def main_linear_classify(parser, args) -> None:
    """--task linear-classify: hbird_mi.classify.hbird_linear_classification and its JSON."""
    if args.memory_sizes:
        parser.error("--memory-sizes is not available with --task linear-classify: the bank holds one row per image (label subsets: "
                     "HbirdKnnClassification.memory_view)")
    for name in KNN_EXCLUDES + ("grid_k", "leave_one_out", "leave_one_out_images"):
        if getattr(args, name):
            parser.error(f"--{name.replace('_', '-').replace('-path', '')} is not available with --task linear-classify")
    if not isinstance(args.n_neighbours, _DefaultInt):
        parser.error("--n-neighbours is not available with --task linear-classify")
    if args.nn_method != "hip":
        parser.error("--nn-method is not available with --task linear-classify (the head is fitted on the HIP index)")
    if args.target_grid != 1:
        parser.error("--target-grid is not available with --task linear-classify")
    top_n = 5 if args.top_n is None else args.top_n
    if top_n > 8:
        parser.error("--top-n: at most 8 predictions are ranked per image")
    l2s = args.probe_l2 or [1e-3]
    if len(l2s) > 16 or len(set(l2s)) != len(l2s):
        parser.error("--probe-l2: 1 to 16 different values")
    logging.basicConfig(level=getattr(logging, args.log_level), force=True)
    set_seed(args.seed)
    from hbird_mi import classify as hclassify
    model = build_model(args)
    t0 = time.time()
    res = hclassify.hbird_linear_classification(model, d_model=args.d_model, patch_size=args.patch_size, dataset_name=args.dataset_name,
                                                data_dir=args.data_dir, batch_size=args.batch_size, input_size=args.input_size,
                                                augmentation_epoch=args.augmentation_epoch, device=args.device, l2s=l2s,
                                                gtol=args.linear_probe_gtol, max_iter=args.linear_probe_iters, topn=top_n,
                                                nn_params=parse_nn_params(args.nn_param), ftr_extr_fn=default_ftr_extr_fn,
                                                num_workers=args.num_workers)
    best, best_top1 = res.best() if res.n else (None, float("nan"))
    summary = {"task": "linear-classify", "top1": {probe_key(v): float(res.top1[v]) for v in res.l2s},
               f"top{top_n}": {probe_key(v): float(res.topn[v]) for v in res.l2s},
               "mean_per_class": {probe_key(v): float(res.mean_per_class[v]) for v in res.l2s},
               "fits": {probe_key(v): res.fits[v] for v in res.l2s},
               "best": None if best is None else {"key": probe_key(best), "top1": float(best_top1)}, "n": res.n, "skipped": res.skipped,
               "top_n": top_n, "seconds": round(time.time() - t0, 3), "dataset": args.dataset_name, **hclassify.last_run_info}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f)


def main(argv: Optional[List[str]] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.bootstrap_seed is not None and not args.bootstrap:
        parser.error("--bootstrap-seed needs --bootstrap")
    if args.task == "knn-classify":
        for name, default in VIDEO_ONLY.items():
            if getattr(args, name) != default:
                parser.error(f"--{name.replace('_', '-')} needs --task video")
        if args.probe_l2 is not None:
            parser.error("--probe-l2 needs --task linear-classify")
        return main_knn_classify(parser, args)
    if args.task == "linear-classify":
        for name, default in VIDEO_ONLY.items():
            if getattr(args, name) != default:
                parser.error(f"--{name.replace('_', '-')} needs --task video")
        if args.grid_temperature is not None:
            parser.error("--grid-temperature needs --task knn-classify")
        return main_linear_classify(parser, args)
    if args.probe_l2 is not None:
        parser.error("--probe-l2 needs --task linear-classify")
    for name, default in KNN_ONLY.items():
        if getattr(args, name) != default:
            parser.error(f"--{name.replace('_', '-')} needs --task knn-classify")
    if args.task == "video":
        return main_video(parser, args)
    for name, default in VIDEO_ONLY.items():
        if getattr(args, name) != default:
            parser.error(f"--{name.replace('_', '-')} needs --task video")
    if args.task == "depth":
        return main_depth(parser, args)
    if args.task == "depth-grid":
        return main_depth_grid(parser, args)
    logging.basicConfig(level=getattr(logging, args.log_level), force=True)
    nn_params = parse_nn_params(args.nn_param)
    set_seed(args.seed)
    from hbird_mi.hbird_eval import hbird_evaluation
    model = build_model(args)
    t0 = time.time()
    result = hbird_evaluation(model, d_model=args.d_model, patch_size=args.patch_size, dataset_name=args.dataset_name,
                              data_dir=args.data_dir, batch_size=args.batch_size, input_size=args.input_size,
                              augmentation_epoch=args.augmentation_epoch, device=args.device, return_knn_details=False,
                              n_neighbours=args.n_neighbours, nn_method=args.nn_method, nn_params=nn_params,
                              ftr_extr_fn=default_ftr_extr_fn, memory_size=args.memory_size,
                              num_workers=args.num_workers, ignore_index=args.ignore_index,
                              train_fs_path=args.train_fs_path, val_fs_path=args.val_fs_path,
                              frame_size=tuple(args.frame_size) if args.frame_size else None,
                              window_stride=args.window_stride, f_mem_p=args.f_mem_p, l_mem_p=args.l_mem_p,
                              **({"memory_sizes": args.memory_sizes} if args.memory_sizes else {}),
                              **({"leave_one_out": True, "leave_one_out_images": args.leave_one_out_images, "leave_one_out_screen": args.leave_one_out_screen}
                                 if args.leave_one_out else {}),
                              **({"grid_k": args.grid_k, "grid_beta": args.grid_beta} if args.grid_k or args.grid_beta else {}),
                              **({"bootstrap": args.bootstrap, "bootstrap_seed": args.bootstrap_seed} if args.bootstrap else {}),
                              **({"overclustering": args.overclustering, "overclustering_seed": args.overclustering_seed,
                                  "overclustering_iters": args.overclustering_iters} if args.overclustering else {}),
                              **({"linear_probe": True, "linear_probe_l2": args.linear_probe_l2, "linear_probe_gtol": args.linear_probe_gtol,
                                  "linear_probe_iters": args.linear_probe_iters} if args.linear_probe else {}))
    from hbird_mi import hbird_eval as _he
    boot_fields: Dict[str, Any] = {}
    if args.bootstrap:
        boot_fields = bootstrap_summary(result, args.bootstrap_level, headline_key(result.keys, args.n_neighbours, args.memory_size))
        result = bootstrap_as_plain(result, bool(args.grid_k or args.grid_beta), bool(args.memory_sizes))
    by_size = grid = grid_by_size = clusters = None
    if args.overclustering:      # the headline figure: the smallest K's
        clusters = {f"clusters={k}": float(v) for k, v in result.items()}
        result = next(iter(result.values()))
    if args.grid_k or args.grid_beta:
        def headline(res):      # the configuration the plain run evaluates when the grid holds it, else the grid's first
            return res.get((args.n_neighbours, 0.02), next(iter(res.values()))) if res else float("nan")
        if args.memory_sizes:
            grid_by_size = {str(size): {grid_key(k, b): float(v) for (k, b), v in res.items()} for size, res in result.items()}
            result = {size: headline(res) for size, res in result.items()}
        else:
            grid = {grid_key(k, b): float(v) for (k, b), v in result.items()}
            result = headline(result)
    if args.memory_sizes:
        by_size = {str(k): float(v) for k, v in result.items()}
        # the headline figure: the built bank's own size when it was listed, else the largest listed one
        result = result[args.memory_size] if args.memory_size in result else result[max(result)] if result else float("nan")
    summary = {"miou": float(result), "seconds": round(time.time() - t0, 3), "nn_method": args.nn_method,
               "dataset": args.dataset_name, "n_neighbours": args.n_neighbours, **_he.last_run_info}
    if args.leave_one_out:
        summary["leave_one_out"] = True
    if by_size is not None:
        summary["miou_by_memory_size"] = by_size
    if grid is not None:
        summary["miou_grid"] = grid
    if grid_by_size is not None:
        summary["miou_grid_by_memory_size"] = grid_by_size
    if clusters is not None:
        summary["miou_overclustering"] = clusters
    if args.linear_probe:      # (linear_probe_fit comes with last_run_info)
        summary["miou_linear_probe"] = float(result)
    summary.update(boot_fields)
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f)


if __name__ == "__main__":
    main()
