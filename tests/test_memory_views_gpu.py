"""HbirdEvaluation.memory_view / hbird_evaluation(memory_sizes=) / eval.py --memory-sizes on the GPU: a view of a built bank must be, bit for bit,
the bank a build from scratch gives -- for a smaller memory size (the bounded build keeps per image the K smallest noisy scores in ascending
order and the noise does not depend on K: hbird_eval.py:146-147, 497-511) and for an image subset of an unbounded bank -- and evaluate to the
identical float."""
import functools
import importlib.util
import json
import os

import pytest
import torch

from hbird_mi.hbird_eval import HbirdEvaluation, hbird_evaluation
from hbird_mi.models import FeatureExtractor
from tiny_vit import TinyQKVViT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, PX, PS, D, NB, B, K_NN = 5, 64, 8, 16, 6, 4, 10
S = PX // PS
N_IMG = NB * B                  # 24 training images, 64 patches each


def _batches(n, seed):
    """n pre-made (x, y) batches of B images: masks of 4 x 4-pixel cells (so a patch mixes classes), delivered as ToTensor would (y / 255)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        cells = torch.randint(0, C, (B, 1, PX // 4, PX // 4), generator=g)
        y = cells.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)
        x = torch.randn((B, 3, PX, PX), generator=g) + y.float()
        out.append((x, y.float() / 255.0))
    return out


TRAIN = _batches(NB, 1)
VAL = _batches(2, 2)


@functools.lru_cache(maxsize=None)
def _extractor():
    return FeatureExtractor(TinyQKVViT(d=D, ps=PS, seed=3).cuda().eval(), eval_spatial_resolution=S, d_model=D)


def _build(memory_size=None, aug=1, train=None, dataset_size=N_IMG, **nn_params):
    torch.manual_seed(1234)                         # the sampling noise comes from torch's CPU generator (hbird_eval.py:500)
    return HbirdEvaluation(_extractor(), TRAIN if train is None else train, num_classes=C, n_neighbours=K_NN, augmentation_epoch=aug,
                           device="cuda", nn_method="hip", nn_params=dict(nn_params), memory_size=memory_size, dataset_size=dataset_size)


@functools.lru_cache(maxsize=None)
def _built(memory_size, aug=1):
    return _build(memory_size, aug)


def _same_bank(a, b):
    fa, fb = a.feature_memory, b.feature_memory
    la, lb = a.label_memory, b.label_memory
    return (fa.shape == fb.shape and torch.equal(fa.view(torch.int32), fb.view(torch.int32)) and la.shape == lb.shape
            and torch.equal(la.view(torch.int32), lb.view(torch.int32)))


@pytest.mark.parametrize("aug", [1, 2])
def test_memory_size_view_is_the_bank_built_from_scratch(cuda_device, aug):
    big = _built(N_IMG * aug * 40, aug)             # K = 40 of 64 patches
    assert big.num_sampled_features == 40 and big.index.ntotal == N_IMG * aug * 40
    assert big._dataset_images == N_IMG and big._bank_block_starts == list(range(0, N_IMG * aug * 40 + 1, 40))
    view = big.memory_view(memory_size=N_IMG * aug * 9)
    scratch = _build(N_IMG * aug * 9, aug)
    assert scratch.num_sampled_features == 9 and view.index.ntotal == scratch.index.ntotal == N_IMG * aug * 9
    assert view.index is not big.index and view.feature_extractor is big.feature_extractor
    assert view.index.label_denominator == scratch.index.label_denominator == PS * PS
    assert _same_bank(view, scratch)
    jv, js = view.evaluate(VAL, S), scratch.evaluate(VAL, S)
    assert isinstance(jv, float) and jv == js, (jv, js)
    assert big.index.ntotal == N_IMG * aug * 40     # the source is untouched
    # the built size itself: all rows
    assert _same_bank(big.memory_view(memory_size=N_IMG * aug * 40), big)


def test_memory_size_view_refusals(cuda_device):
    big = _built(N_IMG * 40)
    with pytest.raises(ValueError, match="built with 40"):
        big.memory_view(memory_size=N_IMG * 41)
    unbounded = _built(None)
    assert unbounded.index.ntotal == N_IMG * S * S
    with pytest.raises(ValueError, match="SAMPLED, not truncated"):
        unbounded.memory_view(memory_size=N_IMG * 9)
    with pytest.raises(ValueError):
        big.memory_view()
    with pytest.raises(ValueError):
        big.memory_view(rows=[0], images=[0])
    with pytest.raises(ValueError):
        big.memory_view(images=[N_IMG])
    with pytest.raises(ValueError):
        big.memory_view(images=[3, 3])
    with pytest.raises(ValueError):
        big.memory_view(rows=[big.index.ntotal])
    # several GPUs in one process (here: one GPU listed twice): views are single-index
    multi = _build(None, train=TRAIN[:1], dataset_size=B, gpu_ids=[0, 0])
    with pytest.raises(ValueError, match="single-index"):
        multi.memory_view(rows=[0])


def test_image_subset_view_is_the_bank_of_those_images(cuda_device):
    unbounded = _built(None)
    images = [0, 5, 6, 23]          # (each keeps its position within a batch of 4)
    view = unbounded.memory_view(images=images)
    xs = torch.stack([TRAIN[i // B][0][i % B] for i in images]); ys = torch.stack([TRAIN[i // B][1][i % B] for i in images])
    scratch = _build(None, train=[(xs, ys)], dataset_size=len(images))
    assert view.index.ntotal == len(images) * S * S and _same_bank(view, scratch)
    assert view._dataset_images == len(images) and view._bank_block_starts == scratch._bank_block_starts
    assert view.evaluate(VAL, S) == scratch.evaluate(VAL, S)
    # listed out of order: the build's row order all the same
    assert _same_bank(unbounded.memory_view(images=[23, 6, 0, 5]), scratch)
    # images= and memory_size= combine on a bounded bank: the per-image count follows the subset (dataset_size = len(images))
    big = _built(N_IMG * 40)
    both = big.memory_view(images=images, memory_size=len(images) * 9)
    fm = big.feature_memory
    want = torch.cat([fm[i * 40: i * 40 + 9] for i in images])
    assert both.num_sampled_features == 9 and torch.equal(both.feature_memory.view(torch.int32), want.view(torch.int32))


def test_rows_views_from_index_and_views_of_views(cuda_device):
    unbounded = _built(None)
    fm, lm = unbounded.feature_memory, unbounded.label_memory
    plain = HbirdEvaluation.from_index(_extractor(), unbounded.index.select_rows(torch.arange(unbounded.index.ntotal)), C, K_NN, device="cuda")
    rows = [5, 3, 3, 100, 1535]
    v = plain.memory_view(rows=rows, n_neighbours=3)
    assert v.n_neighbours == 3 and v.index.ntotal == 5
    assert torch.equal(v.feature_memory.view(torch.int32), fm[rows].view(torch.int32)) and torch.equal(v.label_memory, lm[rows])
    assert isinstance(v.evaluate(VAL, S), float)
    with pytest.raises(ValueError, match="rows_per_image"):
        plain.memory_view(images=[0])                                   # a from_index bank has no geometry ...
    with pytest.raises(ValueError):
        plain.memory_view(images=[0], rows_per_image=S * S + 1)         # ... the row count must divide evenly ...
    one = plain.memory_view(images=[2], rows_per_image=S * S)           # ... and with it an image is its S x S rows
    assert torch.equal(one.feature_memory.view(torch.int32), fm[2 * S * S: 3 * S * S].view(torch.int32))
    with pytest.raises(ValueError):
        v.memory_view(images=[0])                                       # a rows= view has no geometry either
    # a view of a view: 40 -> 20 -> 9 rows per image is the bank built at 9
    big = _built(N_IMG * 40)
    mid = big.memory_view(memory_size=N_IMG * 20)
    assert mid.num_sampled_features == 20 and mid.index.ntotal == N_IMG * 20
    small = mid.memory_view(memory_size=N_IMG * 9)
    direct = big.memory_view(memory_size=N_IMG * 9)
    assert _same_bank(small, direct)
    with pytest.raises(ValueError, match="built with 20"):
        mid.memory_view(memory_size=N_IMG * 21)
    # nn_params' screen settings carry over
    fp = _build(N_IMG * 40, use_fp16=True, fp16_centre=True, rerank_copy=2)
    vfp = fp.memory_view(memory_size=N_IMG * 9)
    assert vfp.nn_params == {"use_fp16": True, "fp16_centre": True, "rerank_copy": 2} and _same_bank(vfp, direct)
    assert vfp.evaluate(VAL, S) == direct.evaluate(VAL, S)


class _PoolViT(torch.nn.Module):
    def forward(self, x):
        return x


def _pool_fn(model, imgs):
    t = torch.nn.functional.avg_pool2d(imgs, 8)
    return t.flatten(2).transpose(1, 2).contiguous(), None


def _synthetic(**kw):
    torch.manual_seed(77)
    return hbird_evaluation(_PoolViT(), d_model=3, patch_size=8, dataset_name="synthetic", data_dir="", batch_size=8, input_size=64,
                            device="cuda", n_neighbours=30, nn_method="hip", ftr_extr_fn=_pool_fn, **kw)


def test_hbird_evaluation_memory_sizes(cuda_device):
    """The synthetic data module has 32 training images: 640 -> K = 20, 160 -> K = 5, 32 -> K = 1."""
    sweep = _synthetic(memory_size=640, memory_sizes=[160, 640, 32, 10 ** 6])
    assert list(sweep) == [160, 640, 32]                    # sizes beyond the built one are left out
    for size, miou in sweep.items():
        assert isinstance(miou, float) and miou == _synthetic(memory_size=size), size
    with pytest.raises(ValueError):
        _synthetic(memory_sizes=[160])                      # the bank must be built bounded
    assert isinstance(_synthetic(memory_size=160), float)   # without the keyword nothing changes


def test_cli_memory_sizes(cuda_device, tmp_path):
    spec = importlib.util.spec_from_file_location("hb_cli_views", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = str(tmp_path / "res.json")
    cli.main(["--dataset-name", "synthetic", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "64", "--batch-size", "8",
              "--device", "cuda", "--nn-method", "hip", "--memory-size", "640", "--memory-sizes", "160", "640", "--out", out,
              "--log-level", "WARNING"])
    res = json.load(open(out))
    assert set(res["miou_by_memory_size"]) == {"160", "640"} and res["miou"] == res["miou_by_memory_size"]["640"]
    assert all(0.0 < v <= 1.0 for v in res["miou_by_memory_size"].values())
