"""The bootstrap kernels (csrc/hbird_bootstrap.hip) against the restatements of tests/bootstrap_refs.py: per-image class counts, the resampler's
multiplicities, the 64-bit resampling reduction and the composite with its float64 epilogue.  Integers and multiplicities are compared exactly,
the composite bit for bit against the sequential restatement; the one tolerance, G * 2^-52, is the distance between a sequential and a pairwise
sum of G terms in [0, 1] divided by G (PredsmIoU._miou_from_counts sums pairwise)."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_refs as br
from hbird_mi import _lib, ops
from hbird_mi.utils.eval_metrics import PredsmIoU

pytestmark = pytest.mark.gpu

SEED = br.SEED


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _maps(G, kind):
    return br.maps(3, 37, 53, G, kind, seed=11 + G)


@functools.lru_cache(maxsize=None)
def _map_counts(G, kind):
    gt, pred = _maps(G, kind)
    return br.image_counts(gt, pred, G, ignore=255)


# ---- per-image counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "blocks"])
@pytest.mark.parametrize("G", [5, 151])
def test_image_class_counts_equal_the_restatement(cuda_device, G, kind):
    gt, pred = _maps(G, kind)
    assert (gt == 255).any() and (gt == G).any() and (gt < 0).any() and (pred < 0).any() and (pred >= G).any() and (gt[1] == 255).all()
    want = _map_counts(G, kind)
    got = ops.image_class_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, 255)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, G, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not want[1].any() and want[0].any()                       # the all-ignored image is a zero block
    # ... summed over the images: the identity matching of the total confusion matrix
    m = PredsmIoU(G, G, ignore_index=255, device=cuda_device, store_reordered_preds=False)
    m.update(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda())
    _, tp, fp, fn, _, _ = m.compute(is_global_zero=True, linear_probe=True, return_reordered=False)
    total = want.astype(np.int64).sum(axis=0)
    assert total[:, 0].tolist() == tp and total[:, 1].tolist() == fp and total[:, 2].tolist() == fn
    # without an ignore value the 255s are out of range anyway (G <= 255)
    assert np.array_equal(ops.image_class_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, None).cpu().numpy(),
                          br.image_counts(gt, pred, G, ignore=None))


@pytest.mark.parametrize("G", [5, 151])
def test_image_class_counts_write_their_blocks_and_nothing_else(cuda_device, G):
    """Two interleaved configurations in one image-major table with sentinels before, between and after every block."""
    block, front, gap, tail = 3 * G, 4, 2, 3
    rs = 2 * block + gap + tail
    buf = torch.full((front + 3 * rs + 6,), -77, dtype=torch.int32, device=cuda_device)
    offs = (front, front + block + gap)
    for off, kind in zip(offs, ("noise", "blocks")):
        gt, pred = _maps(G, kind)
        ops.image_class_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, 255, out=buf[off:], row_stride=rs)
    host = buf.cpu().numpy()
    untouched = np.ones(host.shape, dtype=bool)
    for off, kind in zip(offs, ("noise", "blocks")):
        want = _map_counts(G, kind)
        for b in range(3):
            lo = off + b * rs
            assert np.array_equal(host[lo:lo + block], want[b].reshape(-1)), (kind, b)      # written, not accumulated onto the -77s
            untouched[lo:lo + block] = False
    assert untouched.sum() == host.size - 6 * block and (host[untouched] == -77).all()
    with pytest.raises(ValueError):
        ops.image_class_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, 255, out=buf[:2 * rs + block - 1], row_stride=rs)
    with pytest.raises(ValueError, match="row_stride"):
        ops.image_class_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, 255, out=buf, row_stride=block - 1)
    assert (buf.cpu().numpy() == host).all()


def test_image_class_counts_beyond_the_lds_histogram(cuda_device):
    """G = 5000: 3 G counters do not fit the kernel's LDS budget, the counts go to the zeroed block directly."""
    G = 5000
    gt, pred = br.maps(2, 19, 23, G, "noise", seed=5)
    pred[0, 0, 8:, :] = gt[0, 0, 8:, :]                              # some hits
    buf = torch.full((2 * 3 * G + 5,), -77, dtype=torch.int32, device=cuda_device)
    ops.image_class_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, 255, out=buf, row_stride=3 * G)
    want = br.image_counts(gt, pred, G, ignore=255)
    assert want[0, :, 0].sum() > 100 and not want[1].any()
    assert np.array_equal(buf[:2 * 3 * G].cpu().numpy().reshape(2, G, 3), want) and (buf[2 * 3 * G:] == -77).all()


# ---- multiplicities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 24, 1000, 32768])
def test_multiplicities_equal_the_restatement(cuda_device, N):
    got = ops.bootstrap_multiplicities(N, SEED, 7).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (7, N)
    assert (got.astype(np.int64).sum(axis=1) == N).all()
    assert np.array_equal(got, br.multiplicities(SEED, 0, 7, N))
    whole = ops.bootstrap_multiplicities(N, SEED, 12).cpu().numpy()
    assert np.array_equal(ops.bootstrap_multiplicities(N, SEED, 7, r0=5).cpu().numpy(), whole[5:12])      # rows 5 .. 11 of a chunked call
    if N > 1:
        assert not np.array_equal(ops.bootstrap_multiplicities(N, SEED + 1, 7).cpu().numpy(), got)


def test_multiplicities_refuse_more_images_than_the_histogram_holds(cuda_device):
    with pytest.raises(_lib.HbirdHipError, match="32769 images; at most 32768"):
        ops.bootstrap_multiplicities(32769, SEED, 1)
    with pytest.raises(_lib.HbirdHipError, match="2\\^20"):
        ops.bootstrap_multiplicities(24, SEED, 2, r0=(1 << 20) - 1)


# ---- the reduction --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,G,n_cfg,R", [(24, 5, 2, 70), (1000, 151, 3, 33)])
def test_reduction_equals_the_integer_product(cuda_device, N, G, n_cfg, R):
    stats = br.stats_table(N, n_cfg, G, seed=N)
    W = br.multiplicities(SEED, 0, R, N)
    got = ops.bootstrap_counts(torch.from_numpy(stats).cuda(), torch.from_numpy(W).cuda())
    assert got.dtype == torch.int64 and tuple(got.shape) == (R, n_cfg * 3 * G)
    assert np.array_equal(got.cpu().numpy(), br.counts(W, stats))
    # any int32 weights, negative ones included: the product is signed 32 x 32 -> 64
    rng = np.random.default_rng(2)
    Wr = rng.integers(-2 ** 31, 2 ** 31, size=(5, N)).astype(np.int32)
    sr = rng.integers(-2 ** 31, 2 ** 31, size=stats.shape).astype(np.int32)
    assert np.array_equal(ops.bootstrap_counts(torch.from_numpy(sr).cuda(), torch.from_numpy(Wr).cuda()).cpu().numpy(), br.counts(Wr, sr))


def test_reduction_sums_pass_32_bits(cuda_device):
    stats = np.full((8, 7), 2 ** 31 - 1, dtype=np.int32)
    W = br.multiplicities(SEED, 0, 5, 8)
    got = ops.bootstrap_counts(torch.from_numpy(stats).cuda(), torch.from_numpy(W).cuda()).cpu().numpy()
    assert (got == 8 * (2 ** 31 - 1)).all() and got.min() > 2 ** 32
    assert np.array_equal(got, br.counts(W, stats)) and not np.array_equal(got, br.counts(W, stats, acc32=True))


# ---- the composite --------------------------------------------------------------------------------------------------------------------------
def test_composite_equals_the_sequential_restatement_bit_for_bit(cuda_device):
    N, G, n_cfg, R, absent = 24, 5, 2, 70, 2
    stats = br.stats_table(N, n_cfg, G, seed=3, absent_class=absent)
    point, samples = ops.bootstrap_miou(torch.from_numpy(stats).cuda(), n_cfg, G, SEED, R)
    assert point.dtype == samples.dtype == torch.float64 and tuple(point.shape) == (n_cfg,) and tuple(samples.shape) == (R, n_cfg)
    point, samples = point.cpu().numpy(), samples.cpu().numpy()
    cnt = br.counts(br.multiplicities(SEED, 0, R, N), stats)
    total = stats.astype(np.int64).sum(axis=0, keepdims=True)
    assert np.array_equal(_bits(samples), _bits(br.miou_rows(cnt, n_cfg, G)))
    assert np.array_equal(_bits(point), _bits(br.miou_rows(total, n_cfg, G)[0]))
    # PredsmIoU._miou_from_counts (numpy's pairwise mean) lies within G * 2^-52
    c = cnt.reshape(R, n_cfg, G, 3)
    for r in range(R):
        for k in range(n_cfg):
            assert abs(samples[r, k] - PredsmIoU._miou_from_counts(c[r, k, :, 0], c[r, k, :, 1], c[r, k, :, 2])) <= G * 2.0 ** -52
    t = total.reshape(n_cfg, G, 3)
    for k in range(n_cfg):
        assert abs(point[k] - PredsmIoU._miou_from_counts(t[k, :, 0], t[k, :, 1], t[k, :, 2])) <= G * 2.0 ** -52
    # the class absent from every image contributes 0: the sum over the other classes, still divided by G, has the same bits
    assert not c[:, :, absent, :].any()
    cf = c.astype(np.float64)
    s = np.zeros((R, n_cfg))
    for g in range(G):
        if g != absent:
            s = s + cf[..., g, 0] / np.maximum(cf[..., g, 0] + cf[..., g, 1] + cf[..., g, 2], 1e-8)
    assert np.array_equal(_bits(samples), _bits(s / np.float64(G)))
    # the same seed: the same bits; another seed: other samples; the columns move
    again = ops.bootstrap_miou(torch.from_numpy(stats).cuda(), n_cfg, G, SEED, R)[1].cpu().numpy()
    other = ops.bootstrap_miou(torch.from_numpy(stats).cuda(), n_cfg, G, SEED + 1, R)[1].cpu().numpy()
    assert np.array_equal(_bits(again), _bits(samples)) and not np.array_equal(other, samples) and samples.std(axis=0).min() > 0
    # a subset of the configurations: the same columns (the draws do not depend on them)
    sub = ops.bootstrap_miou(torch.from_numpy(np.ascontiguousarray(stats[:, 3 * G:])).cuda(), 1, G, SEED, R)[1].cpu().numpy()
    assert np.array_equal(_bits(sub[:, 0]), _bits(samples[:, 1]))


def test_composite_in_several_chunks(cuda_device):
    """R = 3000 at cols = 1359 in chunks of 700 (ragged last chunk): the same bits as in one chunk, and as the restatement on the rows
    around every chunk border."""
    N, G, n_cfg, R = 1000, 151, 3, 3000
    stats = br.stats_table(N, n_cfg, G, seed=8)
    dev = torch.from_numpy(stats).cuda()
    p1, s1 = ops.bootstrap_miou(dev, n_cfg, G, SEED, R)
    p7, s7 = ops.bootstrap_miou(dev, n_cfg, G, SEED, R, _chunk_replicates=700)
    s1, s7 = s1.cpu().numpy(), s7.cpu().numpy()
    assert np.array_equal(_bits(s1), _bits(s7)) and np.array_equal(_bits(p1.cpu().numpy()), _bits(p7.cpu().numpy()))
    for r0, n in ((0, 6), (696, 8), (1397, 6), (2796, 8), (2994, 6)):
        cnt = br.counts(br.multiplicities(SEED, r0, n, N), stats)
        assert np.array_equal(_bits(s7[r0:r0 + n]), _bits(br.miou_rows(cnt, n_cfg, G))), r0
    assert np.array_equal(_bits(p7.cpu().numpy()), _bits(br.miou_rows(stats.astype(np.int64).sum(axis=0, keepdims=True), n_cfg, G)[0]))
    with pytest.raises(_lib.HbirdHipError, match="chunk_replicates"):
        ops.bootstrap_miou(dev, n_cfg, G, SEED, 4, _chunk_replicates=-1)
