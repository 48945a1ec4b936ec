"""k beyond 256 without a GPU: the hb_bigk_* entries' argument checks, and fixture G11 (the reference's HbirdEvaluation at
n_neighbours = 600, tests/golden/gen_golden_bigk.py) against the oracle's own restatement of the chain."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G11 = "g11_bigk_evaluate.npz"
# where the generators look for the reference (gen_golden.py's REF; gen_golden_bigk.py imports it from there)
with open(os.path.join(ROOT, "tests", "golden", "gen_golden.py")) as _f:
    REFERENCE_DIR = re.search(r'^REF = "([^"]+)"', _f.read(), re.M).group(1)


def test_bigk_entries_reject_null_and_bad_k_without_a_gpu():
    from hbird_mi import _lib
    L = _lib.lib()
    one = (ctypes.c_char * 64)()                                    # any non-NULL address: no entry gets as far as reading it
    p = ctypes.cast(one, ctypes.c_void_p)
    null_calls = {
        "hb_bigk_search_aggregate": [(None, p, 1, 300, 0, 0.02, p, None, None, 0)],
        "hb_bigk_aggregate": [(None, p, 1, p, p, 300, 0, 0.02, p, 1)],
        "hb_bigk_aggregate_partial": [(None, p, 1, p, p, 300, 0, 0.02, p, 1, p)],
        "hb_bigk_merge_topk": [(None, p, 2, 1, 300, 0, p, p, None), (p, None, 2, 1, 300, 0, p, p, None), (p, p, 2, 1, 300, 0, None, p, None),
                               (p, p, 2, 1, 300, 0, p, None, None)],
        "hb_bigk_merge_topk_packed": [(None, 3600, 2, 1, 300, 0, p, p, None), (p, 3600, 2, 1, 300, 0, None, p, None), (p, 3600, 2, 1, 300, 0, p, None, None)],
    }
    assert set(null_calls) == {n for n in _lib.SIGNATURES if n.startswith("hb_bigk_")}
    for name, calls in null_calls.items():
        for args in calls:
            assert getattr(L, name)(*args) != 0, name
            assert b"NULL" in L.hb_last_error(), (name, L.hb_last_error())
    # the merges check their shape before they touch a device: k and parts outside the range name the limit
    for k in (0, 2049):
        assert L.hb_bigk_merge_topk(p, p, 2, 1, k, 0, p, p, None) != 0 and b"[1, 2048]" in L.hb_last_error()
        assert L.hb_bigk_merge_topk_packed(p, 1 << 20, 2, 1, k, 0, p, p, None) != 0 and b"[1, 2048]" in L.hb_last_error()
    assert L.hb_bigk_merge_topk(p, p, 65, 1, 30, 0, p, p, None) != 0 and b"[1, 64]" in L.hb_last_error()
    assert L.hb_bigk_merge_topk(p, p, 2, 0, 30, 0, None, None, None) == 0          # no queries: nothing to do, as hb_merge_topk


def test_python_limits_are_2048():
    from hbird_mi.nn import search_hip
    assert search_hip.MAX_K == 256 and search_hip.MAX_K_SEARCH == 2048
    search_hip.check_k(1); search_hip.check_k(2048)
    for k in (0, 2049):
        with pytest.raises(ValueError, match="2048"):
            search_hip.check_k(k, "n_neighbours")

    class Flat:                      # the routing: by k alone, and only where a twin exists
        aggregate, aggregate_bigk = "old", "new"

    class Multi:
        aggregate = "own"

    assert [search_hip.k5(Flat, "aggregate", k) for k in (1, 256, 257, 2048)] == ["old", "old", "new", "new"]
    assert search_hip.k5(Multi, "aggregate", 600) == "own"
    # the merge wrappers' test is the old launcher's: 4 B scores (padded to 16) + 8 B ids per candidate within 60,000 B
    assert search_hip._merge_fits_lds(2, 2048) and not search_hip._merge_fits_lds(3, 2048)
    assert search_hip._merge_fits_lds(16, 256) and search_hip._merge_fits_lds(8, 600) and not search_hip._merge_fits_lds(8, 1024)


def _g11(golden_dir):
    g = np.load(os.path.join(golden_dir, G11))
    C, D, H, ps, nb, B, k, ign = g["cfg"].tolist()
    return g, C, D, H, ps, nb, B, k, ign


def test_g11_against_the_chain_oracle(golden_dir):
    """The fp32-chain search (the kernels' bit-exact target) + float64 cross attention on G11's bank reproduce the reference's label_hat
    within 5e-5 everywhere: what the GPU tests then ask of the engine is met by the definition itself."""
    g, C, D, H, ps, nb, B, k, ign = _g11(golden_dir)
    S = H // ps
    fm, lm = g["feature_memory"], g["label_memory"]
    assert (k, fm.shape, lm.shape) == (600, (1280, D), (1280, C))
    worst, beyond = 0.0, []
    for i in range(2):
        tok = g[f"val_tok_{i}"]
        idx, dist = oracle.knn_chain_f32(tok.reshape(-1, D), fm, k)
        kf, kl = oracle.gather_neighbours(idx, fm, lm, B, S * S)
        lh = oracle.cross_attention(tok, kf, kl)
        worst = max(worst, float(np.abs(lh - g["knns_ca_labels"][i * B:(i + 1) * B]).max()))
        # the softmax weight beyond rank 256 (what a list cut at 256 loses)
        qn = tok.reshape(-1, D).astype(np.float64)
        qn /= np.maximum(np.linalg.norm(qn, axis=1, keepdims=True), 1e-12)
        bn = fm.astype(np.float64) / np.maximum(np.linalg.norm(fm.astype(np.float64), axis=1, keepdims=True), 1e-12)
        lg = np.einsum("qd,qkd->qk", qn, bn[idx]) / 0.02
        w = np.exp(lg - lg.max(axis=1, keepdims=True)); w /= w.sum(axis=1, keepdims=True)
        beyond.append(w[:, 256:].sum(axis=1))
    beyond = np.concatenate(beyond)
    print(f"G11: oracle chain vs reference label_hat max {worst:.2e}; weight beyond rank 256: max {beyond.max():.3f}, median {np.median(beyond):.1e}")
    assert worst <= 5e-5
    assert beyond.max() > 0.05, "the fixture no longer carries weight beyond rank 256"
    assert abs(float(g["jac"]) - 0.88170) < 5e-6


@pytest.mark.skipif(not os.path.isdir(REFERENCE_DIR), reason="the generator runs the reference's own code, which is not present here")
def test_g11_regenerates_byte_for_byte(golden_dir, tmp_path):
    env = dict(os.environ, HBIRD_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(golden_dir, "gen_golden_bigk.py")], check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(golden_dir, G11), "rb") as a, open(tmp_path / G11, "rb") as b:
        assert a.read() == b.read()
