"""The mean-centred form of the fp16 screen (hb_index_set_fp16_centre, csrc/hbird_f16_centre.hip) on the GPU.

Equality: with centring on, ids and distance BITS are those of the fp32 kernel (a second index held at set_fp16(0)) on the worlds of
tests/f16_screen_worlds.py -- the massive-activation banks the form exists for, the worlds at the ends of the fp16 range, duplicated rows (ties by
id), the rounding worlds with and without a common shift -- through both re-rank forms, with and without escalation, in mode 1 and in the automatic
state, after appends (rows of 8 x the norm included) and a reset(), on a two-shard index, and with NaN rows in the bank.

Reach (D = 128, massive activations, 20,000 rows, 128 queries, k = 30): the queries that fail their first certificate (last_fp16_escalated) are
no more than those the CPU restatement (tests/test_f16_centre_cpu.centred_model) leaves uncertified plus those it certifies by less than 0.05 E';
without centring every query fails.  D = 768 is printed and only held to "no more failures than uncentred".

Each reach case prints one line `F16CENTRE {json}`."""
import json

import numpy as np
import pytest
import torch

import f16_screen_worlds as fw
import test_f16_centre_cpu as cm
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _index(bank, metric, fp16=None, rerank=None, escalation=None, centre=False):
    ix = HipFlatIndex(bank.shape[1], metric, 0)
    ix.add(bank)
    if fp16 is not None:
        ix.set_fp16(fp16)
    if rerank is not None:
        ix.set_rerank_copy(rerank)
    if escalation is not None:
        ix.set_fp16_escalation(escalation)
    if centre:
        ix.set_fp16_centre(True)
    return ix


def _check_world(dev, W, metric, ks=(30, 90), what=""):
    """Centred searches through both re-rank forms, escalation on and off, against the fp32 kernel.  -> {(k, rerank, escalation): info}"""
    bank, q = torch.from_numpy(W["bank"]).to(dev), torch.from_numpy(W["queries"]).to(dev)
    held = _index(bank, metric, fp16=0)
    seen = {}
    for k in ks:
        want = held.search(q, k)
        assert held.last_search_path() == {"path": "fp32", "reason": "explicit_fp32"}
        for rerank in (1, 2):
            for escalation in (True, False):
                ix = _index(bank, metric, fp16=1, rerank=rerank, escalation=escalation, centre=True)
                got = ix.search(q, k)
                tag = f"{what} metric={metric} k={k} rerank_copy={rerank} escalation={escalation}"
                assert _same(got, want), f"{tag}: differs from the fp32 kernel's answer"
                path = ix.last_search_path()
                seen[(k, rerank, escalation)] = dict(ix.fp16_centre_info(), path=path["path"], reason=path["reason"], search_centred=path["centred"],
                                                     escalated=ix.last_fp16_escalated(), fallbacks=ix.last_fp16_fallbacks())
                ix.close()
    held.close()
    return seen


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [128, 768])
def test_massive_activation_worlds_equal_fp32_and_certify_at_the_first_pass(cuda_device, D, metric):
    W = fw.massive_activation_world(20000, D, 128, seed=31)
    nq = W["queries"].shape[0]
    seen = _check_world(cuda_device, W, metric, what=f"massive_activation D={D}")
    for key, s in seen.items():
        assert s["path"] == "fp16_chain" and s["search_centred"] is True and s["centred"] is True, (key, s)
    # reach at k = 30 (k' = 64)
    m = cm.centred_model(W["queries"], W["bank"], 30, 64, metric)
    allowed = int((~m["certified"][1.05] | (m["margin"][1.05] < 0.05)).sum())
    bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
    plain = _index(bank, metric, fp16=1)
    plain.search(q, 30)
    assert "centred" not in plain.last_search_path() and plain.fp16_centre_info()["centred"] is False
    plain_esc = plain.last_fp16_escalated()
    plain.close()
    esc = seen[(30, 1, True)]["escalated"]
    print("F16CENTRE " + json.dumps({"world": "massive_activation", "rows": 20000, "D": D, "metric": metric, "nq": nq, "k": 30,
                                     "first_certificate_failed_centred": esc, "first_certificate_failed_plain": plain_esc,
                                     "model_uncertified_or_within_0.05": allowed, "reached_fp32_centred": seen[(30, 1, True)]["fallbacks"],
                                     "k90_first_certificate_failed_centred": seen[(90, 1, True)]["escalated"]}))
    for key, s in seen.items():
        if key[0] == 30:
            if D == 128:
                assert s["escalated"] <= allowed, f"{key}: {s['escalated']} first certificates failed, the CPU restatement allows {allowed}"
            else:
                assert s["escalated"] <= plain_esc, (key, s["escalated"], plain_esc)
    if D == 128:
        assert plain_esc == nq, f"uncentred, {plain_esc} of {nq} queries failed the first certificate (recorded behaviour: all)"
    # fp16_centre_info against numpy
    info = seen[(30, 1, True)]
    n = m["norms"]
    assert abs(info["mu_norm"] - n["mun"]) <= 1e-5 * n["mun"], (info["mu_norm"], n["mun"])
    assert abs(info["cmax"] - n["cmax"]) <= 1e-5 * n["cmax"], (info["cmax"], n["cmax"])
    assert abs(info["t"] - n["t"]) <= 1e-5 * abs(n["t"]), (info["t"], n["t"])
    assert info["rows"] == 20000 and info["setting"] is True
    bmax = float(np.sqrt((W["bank"].astype(np.float64) ** 2).sum(axis=1)).max())
    assert abs(info["bmax"] - bmax) <= 1e-5 * bmax


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", ["shared_mean", "duplicate_background", "subnormal", "near_limit"])
def test_vit_shaped_and_range_end_worlds_equal_fp32(cuda_device, name, metric):
    W = fw.VIT_WORLDS[name](12000, 128, 96, seed=9)
    seen = _check_world(cuda_device, W, metric, what=name)
    print(name, metric, {k: (v["path"], v["reason"], v["search_centred"], v["escalated"], v["fallbacks"]) for k, v in seen.items() if k[1] == 1})


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [64, 384])
def test_rounding_worlds_with_and_without_the_common_shift_equal_fp32(cuda_device, D, metric):
    """Hidden true neighbours outside the fp16 top-k': a centred certificate that is too generous returns a decoy in their place."""
    for k in (30, 90):
        kc = min(256, max(64, (2 * k + 7) // 8 * 8))
        W = fw.rounding_world(D, k, kc, 10, 300, cm.GAPS, metric=metric, seed=4000 + D + 7 * k + metric, n_background=5000, n_queries_background=54)
        v = np.zeros(D, np.float32)
        v[np.random.default_rng(D).permutation(D)[:16]] = 0.5           # ||v|| = 2: the planted ranking moves (tests/test_f16_centre_cpu.py), the fp32 answer is the reference
        for shifted in (False, True):
            Ws = {"bank": W["bank"] + v[None, :], "queries": W["queries"] + v[None, :]} if shifted else W
            _check_world(cuda_device, Ws, metric, ks=(k,), what=f"rounding_world D={D} shifted={shifted}")
    for S in cm.shifted_rounding_worlds(D, metric):                     # ... and the shift that keeps the planted ranking (single groups, 300 rows: below 4,096 rows no second pass)
        _check_world(cuda_device, S, metric, ks=(30,), what=f"shifted single group D={D} g={S['g'][0]}")


def test_off_by_default_and_switching_back_returns_the_same_bits_and_path(cuda_device):
    W = cm._isotropic(20000, 128, 256, seed=3)
    bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
    ix = _index(bank, 0, fp16=1)
    assert ix.fp16_centre_info() == {"centred": False, "mu_norm": 0.0, "cmax": 0.0, "bmax": ix.fp16_centre_info()["bmax"], "t": 0.0, "rows": 0,
                                     "setting": False, "last_search_centred": False}
    before = ix.search(q, 30)
    path0, esc0 = ix.last_search_path(), ix.last_fp16_escalated()
    assert path0 == {"path": "fp16_chain", "reason": "explicit_fp16"}
    ix.set_fp16_centre(True)
    on = ix.search(q, 30)
    assert ix.last_search_path() == {"path": "fp16_chain", "reason": "explicit_fp16", "centred": True}
    assert _same(on, before) and ix.fp16_centre_info()["rows"] == 20000
    ix.set_fp16_centre(False)
    after = ix.search(q, 30)
    assert _same(after, before) and ix.last_search_path() == path0 and ix.last_fp16_escalated() == esc0
    assert ix.fp16_centre_info()["centred"] is False
    ix.close()
    z = _index(torch.zeros(5000, 64, device=cuda_device), 0, fp16=1, centre=True)      # an all-zero mean: the plain copy
    z.search(q[:, :64].contiguous(), 30)
    assert z.last_search_path()["centred"] is False
    z.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_appends_after_the_copy_exists_and_a_reset(cuda_device, metric):
    W = fw.massive_activation_world(30000, 128, 128, seed=5)
    bank, q = torch.from_numpy(W["bank"]).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
    ix, held = HipFlatIndex(128, metric, 0), HipFlatIndex(128, metric, 0)
    for x, mode in ((ix, 1), (held, 0)):
        x.reserve(30000); x.add(bank[:12000]); x.set_fp16(mode)      # (room for the appends: a capacity change drops the copy and derives mu anew)
    ix.set_fp16_centre(True)
    assert _same(ix.search(q, 30), held.search(q, 30))
    mu0 = ix.fp16_centre_info()["mu_norm"]
    for lo, hi, scale in ((12000, 12007, 1.0), (12007, 20000, 1.0), (20000, 24000, 8.0), (24000, 30000, 1.0)):      # (a partial tile; rows of 8 x the norm)
        rows = bank[lo:hi] * scale
        ix.add(rows); held.add(rows)
        assert _same(ix.search(q, 30), held.search(q, 30)), (lo, hi, scale)
        info = ix.fp16_centre_info()
        assert info["rows"] == hi and info["mu_norm"] == mu0 and ix.last_search_path()["centred"] is True       # the same mu for the appended rows
    assert info["cmax"] > 7.0                                          # the 8 x rows count for cmax
    ix.reset(); held.reset()
    ix.add(-bank[:9000]); held.add(-bank[:9000])                       # another bank: mu anew
    assert _same(ix.search(q, 30), held.search(q, 30))
    info = ix.fp16_centre_info()
    assert info["rows"] == 9000 and info["cmax"] < 1.0 and info["centred"] is True
    ix.close(); held.close()


def test_nan_rows_and_a_two_shard_index(cuda_device):
    W = fw.massive_activation_world(24000, 128, 128, seed=6)
    b = W["bank"].copy()
    b[[5, 77, 9000, 23999]] = np.nan
    b[4000, 3] = np.inf
    bank, q = torch.from_numpy(b).to(cuda_device), torch.from_numpy(W["queries"]).to(cuda_device)
    for metric in (0, 1):
        ix = _index(bank, metric, fp16=1, centre=True)
        held = _index(bank, metric, fp16=0)
        assert _same(ix.search(q, 30), held.search(q, 30)), f"NaN rows, metric={metric}"
        info = ix.fp16_centre_info()
        assert np.isfinite(info["mu_norm"]) and info["centred"] is True, info          # the mean skips the rows that are not finite
        ix.close(); held.close()
    clean = torch.from_numpy(W["bank"]).to(cuda_device)
    for metric in (0, 1):
        single = _index(clean, metric, fp16=0)
        want = single.search(q, 30)
        multi = HipMultiIndex(128, metric, [0, 0], shard=True)
        multi.reserve(24000); multi.add(clean); multi.set_fp16(1); multi.set_fp16_centre(True)
        got = multi.search(q, 30)
        assert _same(got, want), f"two shards, metric={metric}"
        infos = multi.fp16_centre_info()
        assert all(i["centred"] and i["rows"] == 12000 for i in infos) and infos[0]["mu_norm"] != infos[1]["mu_norm"]      # each shard its own mu
        multi.close(); single.close()


def test_the_automatic_state_and_mode_2_on_a_big_search(cuda_device):
    """21,904 queries x 1.5 M x 128: 31 k stages per workgroup, where the automatic state takes the screen."""
    g = torch.Generator(device=cuda_device); g.manual_seed(11)
    N, D, nq = 1_500_000, 128, 21_904
    def make(n):
        x = torch.randn(n, D, device=cuda_device, generator=g)
        x[:, [3, 40, 99]] = torch.tensor([60.0, -45.0, 80.0], device=cuda_device) * (1.0 + 0.1 * torch.randn(n, 3, device=cuda_device, generator=g))
        return x / x.norm(dim=1, keepdim=True)
    bank, q = make(N), 3.0 * make(nq)
    held = _index(bank, 0, fp16=0)
    want = held.search(q, 30)
    held.close()
    ix = HipFlatIndex(D, 0, 0); ix.add(bank); ix.set_fp16_centre(True)
    got = ix.search(q, 30)
    assert ix.last_search_path() == {"path": "fp16_chain", "reason": "auto", "centred": True}, ix.last_search_path()
    assert _same(got, want)
    auto_esc = ix.last_fp16_escalated()
    ix.set_fp16(2)
    seen = []
    for _ in range(3):                                             # (the adaptive use watches the failing shares from search to search)
        assert _same(ix.search(q, 30), want)
        seen.append((ix.last_search_path(), ix.last_fp16_escalated(), ix.last_fp16_fallbacks()))
    ix.set_fp16_centre(False)
    plain = []
    for _ in range(3):
        assert _same(ix.search(q, 30), want)
        plain.append((ix.last_search_path(), ix.last_fp16_escalated(), ix.last_fp16_fallbacks()))
    print("F16CENTRE " + json.dumps({"world": "massive_activation_torch", "rows": N, "D": D, "nq": nq, "auto_first_certificate_failed": auto_esc,
                                     "mode2_centred": seen, "mode2_plain": plain}))
    assert all(s[0]["path"] == "fp16_chain" and s[0]["centred"] for s in seen)
    assert auto_esc <= plain[0][1]
    ix.close()


def test_fp16_centre_through_the_evaluator(cuda_device):
    """nn_params={'fp16_centre': True}: same mIoU, same label_hat, same confusion counts."""
    from helpers import ReplayExtractor
    from hbird_mi import ops
    from hbird_mi.hbird_eval import HbirdEvaluation
    torch.manual_seed(4)
    S, D, C, B = 14, 384, 21, 64
    def tokens():
        t = torch.randn(B, S * S, D)
        t[:, :, [7, 200]] = torch.tensor([55.0, -70.0]) * (1.0 + 0.1 * torch.randn(B, S * S, 2))
        return t
    tok = [tokens() for _ in range(4)]                                    # 50,176 bank rows: mode 2 takes the screen (tests/test_eval_gpu.py)
    train = [(torch.zeros(B, 3, 16 * S, 16 * S), torch.randint(0, C, (B, 1, 16 * S, 16 * S)).float() / 255) for _ in range(4)]
    val_tok = tokens()
    val = [(torch.zeros(B, 3, 16 * S, 16 * S), torch.randint(0, C, (B, 1, 16 * S, 16 * S)).float() / 255)]
    outs = []
    for centre in (False, True):
        ev = HbirdEvaluation(ReplayExtractor([t.numpy() for t in tok] + [val_tok.numpy()], S, D), train, num_classes=C, device="cuda",
                             nn_method="faiss", nn_params={"use_fp16": True, "fp16_centre": centre})
        jac, det = ev.evaluate(val, S, return_knn_details=True)
        path = ev.index.last_search_path()
        assert path["path"] == "fp16_chain" and path.get("centred", False) is centre, path
        pred = ops.upsample_argmax(det["knns_ca_labels"].cuda().view(B, S * S, C), S, 16 * S, 16 * S).cpu().numpy().ravel()
        gt = (val[0][1] * 255).long().numpy().ravel()
        outs.append((jac, det, np.bincount(gt * C + pred, minlength=C * C)))
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1]["knns_ca_labels"], outs[1][1]["knns_ca_labels"]) and torch.equal(outs[0][1]["knns_labels"], outs[1][1]["knns_labels"])
    assert np.array_equal(outs[0][2], outs[1][2])
