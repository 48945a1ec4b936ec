#!/usr/bin/env python3
"""Generate tests/golden/g11_bigk_evaluate.npz: the REFERENCE's own HbirdEvaluation at n_neighbours = 600.

Same machinery as gen_golden.py (its stubs, its exact float64 stand-in for the absent faiss-gpu wheel, its replaying extractor), one
world: 5 classes, D = 16, 64 x 64 images in 8 x 8 patches, 5 training batches of 4 images (1,280 bank rows), 2 validation batches (512
queries), k = 600.  With 5 classes the softmax weight beyond rank 256 reaches 0.1 for some queries: a list cut at 256 moves half of
label_hat by more than the 5e-5 the tests allow.

Runs only where the reference is present; only the data file is committed.  The file is written by `write_npz` below -- stored
members with a fixed time stamp, in a fixed order -- so that a second run reproduces it byte for byte (numpy's savez stamps every
member with the wall clock).  Masks are kept as the uint8 class maps; the loaders' float masks are mask / 255 in fp32.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bigk.py
"""
from __future__ import annotations

import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (puts the repository, tests/ and the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

NAME = "g11_bigk_evaluate.npz"
C, D, H, PS, NB, B, K, IGNORE, SEED = 5, 16, 64, 8, 5, 4, 600, 255, 111


def write_npz(path, arrays):
    """An .npz that np.load reads, reproducible byte for byte: members in the given order, stored, dated 1980-01-01."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for key, a in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            with zf.open(info, "w") as f:
                a = np.asarray(a)                                     # (ascontiguousarray would turn the 0-d jac into [1])
                np.lib.format.write_array(f, a if a.flags.c_contiguous else np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)


def main():
    gg._install_stubs()
    import golden_inputs as gi
    import hbird.hbird_eval as he
    gg._install_exact_backend()
    out = os.environ.get("HBIRD_GOLDEN_OUT") or HERE
    os.makedirs(out, exist_ok=True)
    world = gi.SegWorld(C, D, H, PS, seed=SEED)
    train = world.loader(NB, B, with_255=True)
    val = world.loader(2, B, with_255=True)
    S = H // PS
    tr_tok = [gi.patch_mean_tokens(x, PS) for x, _ in train]
    va_tok = [gi.patch_mean_tokens(x, PS) for x, _ in val]
    ext = gg.ReplayExtractor(tr_tok + va_tok, S, D)
    tl = [(torch.from_numpy(x), torch.from_numpy(y)) for x, y in train]
    vl = [(torch.from_numpy(x), torch.from_numpy(y)) for x, y in val]
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    ev = he.HbirdEvaluation(ext, tl, num_classes=C, n_neighbours=K, augmentation_epoch=1, device="cpu", nn_method="faiss", nn_params={},
                            memory_size=None, dataset_size=NB * B)
    jac, det = ev.evaluate(vl, eval_spatial_resolution=S, return_knn_details=True, ignore_index=IGNORE)
    g = {"cfg": np.array([C, D, H, PS, NB, B, K, IGNORE]), "rng_state": state.numpy(),
         "feature_memory": ev.feature_memory.numpy(), "label_memory": ev.label_memory.numpy(),
         "jac": np.float64(jac), "knns_ca_labels": det["knns_ca_labels"].numpy()}
    for tag, batches, toks in (("train", train, tr_tok), ("val", val, va_tok)):
        for i, (_, y) in enumerate(batches):
            mask = np.rint(y * 255.0).astype(np.uint8)
            assert np.array_equal(mask.astype(np.float32) / np.float32(255.0), y)
            g[f"{tag}_mask_{i}"] = mask
            g[f"{tag}_tok_{i}"] = toks[i]
    assert ev.feature_memory.shape == (NB * B * S * S, D) and det["knns_ca_labels"].shape == (2 * B, S * S, C)
    write_npz(os.path.join(out, NAME), g)
    print(f"{NAME}: jac {jac:.5f}, {os.path.getsize(os.path.join(out, NAME))} bytes")


if __name__ == "__main__":
    main()
