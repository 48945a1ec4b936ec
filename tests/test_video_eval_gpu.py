"""hbird_mi.video.HbirdVideoEvaluation / hbird_video_evaluation / eval.py --task video on the GPU, in the synthetic video world (48 x 64 frames,
ps = 8: a 6 x 8 grid; two rectangles drifting 4 px per frame) with the patch-pooling extractor and tests/tiny_vit.py.

The restatement takes the engine's own neighbour lists per frame (`propagate_sequence(..., want_neighbours=True)`) and restates everything
after them from tests/propagate_refs.py.  With k = 1 the aggregation is exact in any implementation (one weight, expf(0) / 1 = 1): the row IS
the neighbour's label row, so the whole run -- the ring included -- is compared bit for bit.  With k = 5 the weights go through the device's
expf: there every frame's rows are held to the float64 model on the engine's own pool within the bound of tests/test_propagate_gpu.py, and the
maps are the model's on the engine's rows.  The lists themselves are the model's on the engine's tokens, which pins the ring's context order."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import propagate_refs as R
from hbird_mi import video as hvideo
from hbird_mi.data.video import SyntheticVideoDataModule
from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
from tiny_vit import TinyQKVViT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS, H, W, GRID = 8, 48, 64, (6, 8)
N = GRID[0] * GRID[1]
LAST, RADIUS, TEMP = 3, 2, 0.1
WORLD = SyntheticVideoDataModule(n_sequences=2, n_frames=8, frame_size=(H, W), n_objects=2, step=4, seed=5)       # T = 8 > LAST + 2: the ring wraps


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x


def _pool_fn(model, imgs):
    return torch.nn.functional.avg_pool2d(imgs, PS).flatten(2).transpose(1, 2).contiguous(), None


@functools.lru_cache(maxsize=None)
def _extractor(which):
    if which == "pool":
        return FeatureExtractorSimple(_Identity(), ftr_extr_fn=_pool_fn, eval_spatial_resolution=GRID[0], d_model=3)
    return FeatureExtractor(TinyQKVViT(d=16, ps=PS, seed=3).cuda().eval(), eval_spatial_resolution=GRID[0], d_model=16)


def _ev(which, k, **kw):
    kw.setdefault("radius", RADIUS)
    return hvideo.HbirdVideoEvaluation(_extractor(which), PS, n_neighbours=k, temperature=TEMP, n_last_frames=LAST, device="cuda", **kw)


def _u32(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.uint32)


def _patch_shares(ann0, c):
    """ops.patch_label_hist restated: the share of every id among a patch's pixels (a count over ps^2: exact in fp32)."""
    a = np.asarray(ann0).reshape(GRID[0], PS, GRID[1], PS).transpose(0, 2, 1, 3).reshape(N, PS * PS)
    return np.stack([(a == o).sum(axis=1) for o in range(c)], axis=1).astype(np.float32) / np.float32(PS * PS)


@pytest.mark.parametrize("which,k", [("pool", 1), ("vit", 1), ("pool", 5), ("vit", 5)])
def test_evaluate_equals_the_restatement(cuda_device, which, k):
    ev = _ev(which, k)
    res = ev.evaluate(WORLD.sequences(), frame_batch=3, return_maps=True)
    assert not res.skipped and set(res.per_sequence) == {name for name, _, _ in WORLD.sequences()}
    want_counts = {}
    for name, frames, ann in WORLD.sequences():
        T, n = frames.shape[0], int(ann[0].max())
        c = n + 1
        tok = ev.tokens(frames, 3).cpu().numpy()
        rows, lists = ev.propagate_sequence(frames, ann[0], n, frame_batch=3, want_neighbours=True)
        rows = rows.cpu().numpy()
        feat = np.zeros((1 + LAST, N, tok.shape[2]), dtype=np.float32)
        lab = np.zeros((1 + LAST, N, c), dtype=np.float32)
        feat[0], lab[0] = tok[0], _patch_shares(ann[0].numpy(), c)
        for t in range(1, T):
            ctx_frames, slots = R.ring_context(t, LAST)
            assert ctx_frames == [0] + list(range(max(1, t - LAST), t))
            radii = [RADIUS] * len(slots)
            idx, score = (a.cpu().numpy() for a in lists[t - 1])
            m_idx, m_score = R.lists(tok[t], feat, slots, radii, GRID, k)
            assert np.array_equal(idx, m_idx) and np.array_equal(_u32(score), _u32(m_score)), f"{name} frame {t}: the lists are not the model's"
            if k == 1:
                model_row = np.stack([lab[slots[j // N], j % N] for j in idx[:, 0]])
                assert np.array_equal(_u32(rows[t - 1]), _u32(model_row)), f"{name} frame {t}: the row is not the neighbour's label row"
                ring_row = model_row                                       # bit for bit, the ring included
            else:
                ref = R.aggregate(idx, score, lab, slots, N, TEMP)
                tol = R.aggregate_bound(idx, score, lab, TEMP)
                err = np.abs(rows[t - 1].astype(np.float64) - ref).max(axis=1)
                assert (err <= tol).all(), f"{name} frame {t}: worst {np.max(err / tol):.2f} x the bound"
                ring_row = rows[t - 1]                                     # the model goes on from the engine's rows
            slot = 1 + (t - 1) % LAST
            feat[slot], lab[slot] = tok[t], ring_row
        maps = R.label_map(rows, GRID, H, W, norm=True)
        assert np.array_equal(res.maps[name].numpy(), maps), f"{name}: the maps are not the model's on the engine's rows"
        want_counts[name] = R.jf_counts(maps[:T - 2], ann[1:T - 1].numpy(), n, R.bound_px(H, W))
        assert np.array_equal(res.counts[name], want_counts[name])
    want = R.video_metrics(want_counts)
    assert set(res) == set(want)
    for key in want:
        assert abs(res[key] - want[key]) < 1e-12, key


def test_first_frame_radius(cuda_device):
    name, frames, ann = next(iter(WORLD.sequences()))
    n = int(ann[0].max())

    def first_frame_offsets(ev):
        _, lists = ev.propagate_sequence(frames, ann[0], n, want_neighbours=True)
        worst = 0
        for idx, _ in lists:
            idx = idx.cpu().numpy()
            qy, qx = np.arange(N)[:, None] // GRID[1], np.arange(N)[:, None] % GRID[1]
            first = (idx >= 0) & (idx < N)
            dy, dx = np.abs(idx // GRID[1] - qy), np.abs(idx % GRID[1] - qx)
            worst = max(worst, int(np.where(first, np.maximum(dy, dx), 0).max()))
        return worst
    assert _ev("pool", 5).first_frame_radius == RADIUS
    assert first_frame_offsets(_ev("pool", 5)) <= RADIUS
    assert first_frame_offsets(_ev("pool", 5, first_frame_radius=-1)) > RADIUS, "an unrestricted first frame must reach beyond the window"


def test_propagation_is_informative(cuda_device):
    """A condition on the world, not a measurement of the engine: a float64 prototype of these definitions gave J 0.73 to 0.74 for the
    propagation and 0.13 for copying the first annotation, at radius 2, k = 5, temperature 0.1 and three last frames."""
    world = SyntheticVideoDataModule(n_sequences=3, n_frames=10, frame_size=(H, W), n_objects=2, step=4, noise=0.1, seed=0)
    res = _ev("pool", 5).evaluate(world.sequences())
    static = {}
    for name, frames, ann in world.sequences():
        T, n = ann.shape[0], int(ann[0].max())
        copies = np.repeat(ann[:1].numpy(), T - 2, axis=0)
        static[name] = R.jf_counts(copies, ann[1:T - 1].numpy(), n, R.bound_px(H, W))
    base = R.video_metrics(static)
    print(f"propagation J {res['J_mean']:.3f} F {res['F_mean']:.3f}; static copy J {base['J_mean']:.3f} F {base['F_mean']:.3f}")
    assert res["J_mean"] - base["J_mean"] >= 0.3


def test_short_sequences_are_listed(cuda_device):
    name, frames, ann = next(iter(WORLD.sequences()))
    res = _ev("pool", 5).evaluate([("two", frames[:2], ann[:2]), (name, frames[:4], ann[:4])])
    assert [s[0] for s in res.skipped] == ["two"] and list(res.per_sequence) == [name] and res.per_sequence[name]["n_frames"] == 2
    with pytest.raises(ValueError, match="tokens"):
        bad = FeatureExtractorSimple(_Identity(), ftr_extr_fn=lambda m, x: (_pool_fn(m, x)[0][:, 1:], None), eval_spatial_resolution=GRID[0], d_model=3)
        hvideo.HbirdVideoEvaluation(bad, PS, device="cuda").evaluate([(name, frames[:4], ann[:4])])


def test_front_ends_agree(cuda_device, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("hbird_cli_video", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    world = SyntheticVideoDataModule()
    extractor = FeatureExtractorSimple(cli._PatchPool(PS), ftr_extr_fn=cli.default_ftr_extr_fn, eval_spatial_resolution=GRID[0], d_model=3)
    want = hvideo.HbirdVideoEvaluation(extractor, PS, n_neighbours=5, temperature=TEMP, n_last_frames=LAST, radius=RADIUS).evaluate(world.sequences())
    got = hvideo.hbird_video_evaluation(cli._PatchPool(PS), d_model=3, patch_size=PS, dataset_name="synthetic-video", data_dir="", n_last_frames=LAST,
                                        radius=RADIUS, temperature=TEMP, ftr_extr_fn=cli.default_ftr_extr_fn)
    assert dict(got) == dict(want) and got.per_sequence == want.per_sequence
    out = tmp_path / "video.json"
    cli.main(["--task", "video", "--dataset-name", "synthetic-video", "--data-dir", "", "--d-model", "3", "--patch-size", str(PS),
              "--video-last-frames", str(LAST), "--video-radius", str(RADIUS), "--out", str(out)])
    capsys.readouterr()
    js = json.loads(out.read_text())
    assert js["task"] == "video" and js["n_neighbours"] == 5
    for key in ("J_mean", "J_recall", "F_mean", "F_recall", "J&F"):
        assert js[key] == want[key], key
    assert js["per_sequence"] == want.per_sequence
