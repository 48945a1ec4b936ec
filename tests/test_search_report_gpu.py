"""One report per search (csrc/hbird_report.h): every read-out of a finished search answers from the same report, so what they say about it
agrees by construction.  The image world of tests/excl_screen_refs.py (6,000 x 64 rows, 240 queries, k = 30: ECASE["image"] and
ECASE["image-l2"]) is the smallest committed world that reaches level 0, the second pass and the rungs in ONE excluding search: route_model(30,
metric)["counts"] = (184, 31, 25) for both metrics, all three positive (tests/test_exclude_seeds_gpu.py pins that the device has the model's
counts); the test asks the model again before it relies on it.

After one search_excluding on the screen: last_exclusion_screen(), last_screen_seeds(), last_exclusion_seeds(), last_fp16_escalated(),
last_fp16_fallbacks() and last_search_path() name the same level sizes.  The same search with the second pass switched off hands level 0's
failures straight to the rungs: nothing nested ran (escalated 0), the rungs get nq - certified0 queries and the level-0 lists stay readable.
A plain search afterwards leaves the reports of a fresh index given only that search, and nothing of the excluding one."""
import numpy as np
import pytest
import torch

import excl_screen_refs as X
from hbird_mi import _lib
from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu
K = 30


def _index(dev, name, escalation=True):
    c, W, groups, n_groups, qg = X.excl_case(name)
    ix = HipFlatIndex(c.D, c.metric, 0)
    ix.set_fp16(True)
    ix.set_fp16_escalation(escalation)
    ix.add(torch.from_numpy(W["bank"]).to(dev))
    ix.set_row_groups(groups, n_groups)
    ix.set_exclusion_screen(True)
    return ix


def _reports(ix):
    return {"escalated": ix.last_fp16_escalated(), "fallbacks": ix.last_fp16_fallbacks(), "path": ix.last_search_path()}


@pytest.mark.parametrize("name,metric", [("image", 0), ("image-l2", 1)])
def test_the_read_outs_of_one_search_agree(cuda_device, name, metric):
    c, W, groups, n_groups, qg = X.excl_case(name)
    assert (c.k, c.metric, c.nq) == (K, metric, 240)
    counts = X.route_model(K, metric)["counts"]
    assert all(n > 0 for n in counts) and sum(counts) == c.nq, counts      # level 0, the second pass and the rungs each get queries
    q, qgd = torch.from_numpy(W["queries"]).to(cuda_device), torch.from_numpy(qg).to(cuda_device)

    ix = _index(cuda_device, name)
    ix.search_excluding(q, K, qgd)
    es, S, Xs = ix.last_exclusion_screen(), ix.last_screen_seeds(), ix.last_exclusion_seeds()
    print("SEARCHREPORT", name, {k: v for k, v in es.items()}, {k: S[k] for k in ("nq", "kc0", "n1", "n2", "centred")}, Xs["n1"], Xs["n_left"], _reports(ix))
    assert es["served"] == 1
    assert es["kc"] == S["kc0"]
    assert es["certified0"] == S["certified0"].sum()
    assert es["second_pass"] == S["n1"] == Xs["n1"] == ix.last_fp16_escalated()
    assert es["certified1"] == S["certified1"].sum()
    assert es["rung_queries"] == Xs["n_left"] == S["n2"] == ix.last_fp16_fallbacks()
    assert es["centred"] == S["centred"]
    assert ix.last_search_path()["path"] == "fp16_chain"
    assert min(es["certified0"], es["second_pass"], es["rung_queries"]) > 0, es      # (the world does reach all three on the device)

    # the second pass switched off: level 0's failures go straight to the rungs
    ix0 = _index(cuda_device, name, escalation=False)
    ix0.search_excluding(q, K, qgd)
    e0 = ix0.last_exclusion_screen()
    assert e0["served"] == 1 and e0["second_pass"] == 0, e0
    assert ix0.last_fp16_escalated() == 0
    assert e0["rung_queries"] == c.nq - e0["certified0"] == ix0.last_fp16_fallbacks(), e0
    L0 = ix0.last_screen()
    assert L0["nq"] == c.nq and L0["kc"] == e0["kc"] and L0["certified"].sum() == e0["certified0"]
    ix0.close()

    # a plain search on the first index: the excluding search's report is gone, the plain one's is that of a fresh index
    ix.search(q, K)
    with pytest.raises(_lib.HbirdHipError, match="not an excluding one served"):
        ix.last_exclusion_seeds()
    fresh = _index(cuda_device, name)
    fresh.search(q, K)
    assert _reports(ix) == _reports(fresh), (_reports(ix), _reports(fresh))
    fresh.close()
    ix.close()
