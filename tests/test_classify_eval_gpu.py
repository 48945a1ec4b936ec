"""hbird_mi.classify.HbirdKnnClassification / hbird_knn_classification / eval.py --task knn-classify on the GPU, in the synthetic
classification world (192 training and 60 validation images of 32 x 32 pixels, 12 classes, noise 0.5) with a fixed random projection of the
pixels as the image-level feature.

The projection runs in float64 on the host and is rounded to fp32 once, so the engine and the numpy pipeline see the same feature bits
whatever the batch size.  The numpy pipeline: `oracle.normalize_rows` -> `oracle.knn_chain_f32` lists -> tests/vote_refs.py (float64 votes,
the ranking rule, the counts).  The count tables must equal the pipeline's outside the exemption of tests/test_vote_gpu.py: a query where
two adjacent ranked votes of the model lie within the derived bound of each other may be predicted differently, so a count may differ by
at most the number of such queries of its configuration, which may be at most 2 % of the queries (in this world the model has none on the
validation split and one of 192 on the leave-one-out pass)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import oracle
import vote_refs as R
from hbird_mi import classify as hclassify
from hbird_mi.data.classify import SyntheticClassifyDataModule
from hbird_mi.data.synthetic import _Loader

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, D, KS, TS, TOPN = 12, 24, (1, 5, 20, 50), (0.07, 1.0), 5
WORLD = SyntheticClassifyDataModule(batch_size=16, input_size=32, num_classes=C, n_train=192, n_val=60, noise=0.5, seed=2)
_W = torch.randn((3 * 32 * 32, D), generator=torch.Generator().manual_seed(11), dtype=torch.float64) / 55.0


def feature_fn(imgs):
    """A fixed random projection of the pixels: float64 on the host, rounded to fp32 once."""
    return (imgs.detach().double().cpu().flatten(1) @ _W).float()


def _all(loader):
    xs, ys = zip(*list(loader))
    return torch.cat(xs), torch.cat(ys)


def _rebatch(x, y, bs):
    return _Loader([(x[i:i + bs], y[i:i + bs]) for i in range(0, x.shape[0], bs)])


def _classifier(**kw):
    kw.setdefault("n_neighbours", KS)
    kw.setdefault("temperatures", TS)
    return hclassify.HbirdKnnClassification(feature_fn, C, topn=TOPN, device="cuda", **kw)


@functools.lru_cache(maxsize=None)
def world():
    (xt, yt), (xv, yv) = _all(WORLD.train_dataloader()), _all(WORLD.val_dataloader())
    bank = oracle.normalize_rows(feature_fn(xt).numpy())
    q = oracle.normalize_rows(feature_fn(xv).numpy())
    return xt, yt, xv, yv, bank, q


def model_tables(idx, score, labels, qlabels, ks=KS, temps=TS):
    """-> (counts [n_cfg, topn], per_class [n_cfg, C, 2], n, exempt queries per configuration) of the numpy pipeline on given lists."""
    counts, per, ex = [], [], []
    for k in ks:
        for T in temps:
            v, present = R.vote(idx, score, labels, C, k, T)
            pred, _ = R.top(v, present, TOPN)
            c, pc, n = R.counts(pred, qlabels, C)
            counts.append(c); per.append(pc)
            ex.append(int(R.exempt(v, present, R.vote_bound(idx, score, labels, k, T)).sum()))
    return np.stack(counts), np.stack(per), n, np.array(ex)


def assert_tables(m, want, nq):
    counts, per, n, ex = want
    assert m.n == n and (ex <= 0.02 * nq).all(), f"exempt queries per configuration: {ex.tolist()}"
    assert (np.abs(m.counts - counts) <= ex[:, None]).all(), f"counts differ from the numpy pipeline's beyond the exemption {ex.tolist()}:\n{m.counts - counts}"
    assert (np.abs(m.class_counts - per) <= ex[:, None, None]).all(), "per-class counts differ from the numpy pipeline's beyond the exemption"


@functools.lru_cache(maxsize=None)
def built():
    return _classifier().build(WORLD.train_dataloader())


def test_count_tables_equal_the_numpy_pipeline(cuda_device):
    xt, yt, xv, yv, bank, q = world()
    ev = built()
    assert ev.index.ntotal == 192 and ev.labels.dtype == torch.int32 and torch.equal(ev.labels.cpu(), yt.to(torch.int32))
    assert torch.equal(ev.index.row_groups.cpu(), torch.arange(192, dtype=torch.int32)) and ev.n_images == 192
    m = ev.evaluate(WORLD.val_dataloader())
    idx, score = oracle.knn_chain_f32(q, bank, KS[-1])
    want = model_tables(idx, score, yt.numpy().astype(np.int32), yv.numpy())
    print("top1", {k: round(v, 3) for k, v in m.top1.items()}, "top5", {k: round(v, 3) for k, v in m.topn.items()}, "exempt", want[3].tolist())
    assert_tables(m, want, 60)
    assert m.configs == [(k, T) for k in KS for T in TS] and m.n == 60 and m.skipped == 0 and m.n_top == TOPN
    assert 0.3 < min(m.top1.values()) and max(m.top1.values()) < 1.0, "the world should be imperfect, and far above chance (1 / 12)"
    assert all(m.topn[c] >= m.top1[c] for c in m.configs) and m.best()[1] == max(m.top1.values())
    # batch size does not change the counts; unlabelled queries are counted as skipped, not dropped
    m7 = ev.evaluate(_rebatch(xv, yv, 7))
    assert np.array_equal(m7.counts, m.counts) and np.array_equal(m7.class_counts, m.class_counts) and m7.n == m.n
    y_some = yv.clone()
    y_some[::6] = -1
    ms = ev.evaluate(_rebatch(xv, y_some, 25))
    want_some = model_tables(idx, score, yt.numpy().astype(np.int32), y_some.numpy())
    assert ms.n == 50 and ms.skipped == 10
    assert_tables(ms, want_some, 60)
    with pytest.raises(ValueError, match="class id"):
        ev.evaluate(_rebatch(xv, torch.full_like(yv, C), 30))


def test_memory_view_equals_a_classifier_built_on_those_images(cuda_device):
    xt, yt, xv, yv, _, _ = world()
    ev = built()
    keep = torch.tensor([i for i in range(192) if i % 3 != 1])
    view = ev.memory_view(images=keep)
    alone = _classifier().build(_rebatch(xt[keep], yt[keep], 16))
    assert view.index.ntotal == alone.index.ntotal == keep.numel() and torch.equal(view.labels, alone.labels)
    assert torch.equal(view.row_groups, keep.to(torch.int32))                                    # the view's rows keep their images
    mv, ma = view.evaluate(WORLD.val_dataloader()), alone.evaluate(WORLD.val_dataloader())
    assert np.array_equal(mv.counts, ma.counts) and np.array_equal(mv.class_counts, ma.class_counts) and mv.n == ma.n == 60
    assert not np.array_equal(mv.counts, ev.evaluate(WORLD.val_dataloader()).counts), "a third of the bank gone changes nothing?"
    rows = ev.memory_view(rows=keep)
    assert np.array_equal(rows.evaluate(WORLD.val_dataloader()).counts, mv.counts)
    with pytest.raises(ValueError):
        ev.memory_view()
    with pytest.raises(ValueError):
        ev.memory_view(images=[192])
    for c in (view, alone, rows):
        c.close()


def test_leave_one_out_on_the_training_split(cuda_device):
    xt, yt, _, _, bank, _ = world()
    ev = built()
    plain = ev.evaluate(WORLD.train_dataloader())
    assert plain.top1[(1, 0.07)] == 1.0 and plain.top1[(1, 1.0)] == 1.0, "without exclusion every training image finds itself"
    # the numpy model on the excluded lists: the first k entries other than the query's own row among the best k + 1
    idx1, score1 = oracle.knn_chain_f32(bank, bank, KS[-1] + 1)
    own = idx1 == np.arange(192)[:, None]
    assert (own.sum(axis=1) == 1).all()
    order = np.argsort(own, axis=1, kind="stable")[:, :KS[-1]]                                    # the others in list order
    idx, score = np.take_along_axis(idx1, order, 1), np.take_along_axis(score1, order, 1)
    want = model_tables(idx, score, yt.numpy().astype(np.int32), yt.numpy())
    assert want[0][0, 0] < 192, "the model's leave-one-out top-1 at k = 1 must lie below 1.0 in this world"
    loo = ev.evaluate_leave_one_out(WORLD.train_dataloader())
    print("leave-one-out top1", {k: round(v, 3) for k, v in loo.top1.items()}, "exempt", want[3].tolist())
    assert_tables(loo, want, 192)
    assert loo.top1[(1, 0.07)] < 1.0 and loo.n == 192
    few = ev.evaluate_leave_one_out(WORLD.train_dataloader(), max_images=100)
    want_few = model_tables(idx[:100], score[:100], yt.numpy().astype(np.int32), yt.numpy()[:100])
    assert few.n == 100
    assert_tables(few, want_few, 100)
    with pytest.raises(ValueError, match="more than the 192 images"):
        ev.evaluate_leave_one_out(_rebatch(torch.cat([xt, xt[:5]]), torch.cat([yt, yt[:5]]), 16))
    # two epochs: an image owns two rows; k + 2 beyond 2048 is refused in exclude_plan's words before anything is searched
    two = _classifier(n_neighbours=(5, 2047), temperatures=(0.07,)).build(WORLD.train_dataloader(), augmentation_epoch=2)
    assert two.index.ntotal == 384 and torch.equal(two.row_groups, torch.arange(192, dtype=torch.int32).repeat(2))
    with pytest.raises(ValueError, match="2048"):
        two.evaluate_leave_one_out(WORLD.train_dataloader())
    two.close()
    unknown = hclassify.HbirdKnnClassification.from_index(ev.index, ev.labels.cpu(), feature_fn, C, KS, TS, TOPN)
    with pytest.raises(ValueError, match="not known"):
        unknown.evaluate_leave_one_out(WORLD.train_dataloader())


def test_cli_knn_classify_writes_the_json_keys(cuda_device, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("hbird_cli_classify", os.path.join(ROOT, "eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = tmp_path / "knn.json"
    cli.main(["--task", "knn-classify", "--dataset-name", "synthetic-classify", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "32",
              "--batch-size", "32", "--out", str(out)])
    res = json.loads(out.read_text())
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    keys = [f"k={k},T=0.07" for k in (10, 20, 100, 200)]
    for table in ("top1", "top5", "mean_per_class"):
        assert list(res[table]) == keys and all(0.0 <= res[table][k] <= 1.0 for k in keys), table
    assert res["task"] == "knn-classify" and res["n"] == 60 and res["skipped"] == 0 and res["bank_rows"] == 192
    assert res["best"]["key"] in keys and res["best"]["top1"] == max(res["top1"].values()) > 1.0 / 12
    assert all(res["top5"][k] >= res["top1"][k] for k in keys)
    out2 = tmp_path / "loo.json"
    cli.main(["--task", "knn-classify", "--dataset-name", "synthetic-classify", "--data-dir", "", "--d-model", "3", "--patch-size", "8", "--input-size", "32",
              "--grid-k", "1", "5", "--grid-temperature", "0.07", "1", "--top-n", "3", "--leave-one-out", "--leave-one-out-images", "50", "--out", str(out2)])
    loo = json.loads(out2.read_text())
    assert list(loo["top1"]) == ["k=1,T=0.07", "k=1,T=1.0", "k=5,T=0.07", "k=5,T=1.0"] and "top3" in loo and loo["n"] == 50 and loo["leave_one_out"] is True
