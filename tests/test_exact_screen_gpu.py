"""The automatic state of the fp16 setting on the GPU: a new index sends its BIG exact searches through the certified fp16 screen (fp16
candidate pass, exact fp32 re-rank, certificate, escalation) and returns the fp32 kernel's ids and distance bits; whatever keeps a search off
the screen -- a pinned index, a bank fp16 cannot hold or certify, k > 128, no room for the fp16 copy -- ends on the fp32 kernel without an error.
(The decision itself, without a GPU: tests/test_exact_screen_cpu.py.)"""
import gc

import pytest
import torch

from hbird_mi.nn.search_hip import HipFlatIndex

pytestmark = pytest.mark.gpu

NQ = 21_904          # 86 query tiles: with 256 workgroups a D = 768 bank of 239,000 rows reaches the big-search bound (30,000 stages per workgroup)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _pair(bank, metric=0, labels=None, classes=0):
    """-> (a new index left as it is created, a second one held at set_fp16(0)) over the same rows."""
    out = []
    for hold in (False, True):
        ix = HipFlatIndex(bank.shape[1], metric, 0)
        ix.add(bank)
        if labels is not None:
            ix.add_labels(labels); ix.set_num_classes(classes)
        if hold:
            ix.set_fp16(0)
        out.append(ix)
    return out


def _normal_bank(M, D, seed, dev):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    bank = torch.nn.functional.normalize(torch.randn((M, D), generator=g, device=dev), dim=1)
    q = 3.0 * torch.randn((NQ, D), generator=g, device=dev)
    return bank, q, g


@pytest.mark.parametrize("metric", [0, 1])
def test_a_new_index_screens_big_searches_and_returns_the_fp32_bits(cuda_device, metric):
    M, D, C = 2_000_000, 768, 21
    bank, q, g = _normal_bank(M, D, 3, cuda_device)
    labels = torch.rand((M, C), generator=g, device=cuda_device)
    auto, held = _pair(bank, metric, labels, C)
    del bank
    for k in (30, 90):
        want = held.search(q, k)
        assert held.last_search_path() == {"path": "fp32", "reason": "explicit_fp32"}
        got = auto.search(q, k)
        assert auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"}, (k, auto.last_search_path())
        assert _same(got, want), f"k={k}: the screened search differs from the fp32 kernel's"
        assert auto.last_fp16_fallbacks() < NQ // 100
        lh0, i0, d0 = held.search_aggregate(q, k, want_neighbours=True)
        lh1, i1, d1 = auto.search_aggregate(q, k, want_neighbours=True)
        assert auto.last_search_path()["path"] == "fp16_chain"
        assert _same((i1, d1), (i0, d0)) and _same((i1, d1), want)
        assert torch.equal(_bits(lh1), _bits(lh0)), f"k={k}: label aggregation differs bitwise"
    # small searches stay where they were: the fp32 kernel, no reason to look at memory
    got = auto.search(q[:64], 30)
    assert auto.last_search_path() == {"path": "fp32", "reason": "small"}
    assert _same(got, held.search(q[:64], 30))
    # an explicit request for the fp32 kernel keeps meaning the fp32 kernel, and "auto" brings the default back
    auto.set_fp16(False)
    auto.search(q, 30)
    assert auto.last_search_path() == {"path": "fp32", "reason": "explicit_fp32"}
    auto.set_fp16("auto")
    assert _same(auto.search(q, 30), held.search(q, 30)) and auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"}


def test_steering_the_fp32_kernel_pins_the_index_to_it(cuda_device):
    M, D, k = 300_000, 768, 30
    bank, q, _ = _normal_bank(M, D, 5, cuda_device)
    ref = HipFlatIndex(D, 0, 0); ref.add(bank); ref.set_fp16(0)
    want = ref.search(q, k)
    pins = [("set_xcd_weights", (1,)), ("set_cluster", (2, 4, 16)), ("set_variant", (3,)), ("set_tuning", (256, 0)), ("set_cluster_sharing", (1,)),
            ("set_search_options", (True, 0)), ("set_xcd_weights", (2, [1.0, 0.9, 1.1, 1.0, 1.0, 0.95, 1.05, 1.0]))]
    for name, args in pins:
        ix = HipFlatIndex(D, 0, 0); ix.add(bank)
        ix.set_cluster(0, 0, -1); ix.set_xcd_weights(0)            # the automatic settings steer nothing
        assert _same(ix.search(q, k), want)
        assert ix.last_search_path() == {"path": "fp16_chain", "reason": "auto"}, name
        assert ix.schedule_info()["workgroups"] == 256
        getattr(ix, name)(*args)
        assert _same(ix.search(q, k), want), name
        assert ix.last_search_path() == {"path": "fp32", "reason": "pinned"}, name
        assert ix.last_fp16_fallbacks() == 0 and ix.last_fp16_escalated() == 0
        if name == "set_cluster":
            assert ix.schedule_info()["cluster"] == [2, 4]
        # ... for the rest of its life: going back to the automatic settings does not unpin, an explicit use_fp16 request still counts
        ix.set_cluster(0, 0, -1); ix.set_variant(0); ix.set_xcd_weights(0); ix.set_fp16("auto")
        ix.search(q, k)
        assert ix.last_search_path() == {"path": "fp32", "reason": "pinned"}, name
        ix.set_fp16(2)
        assert _same(ix.search(q, k), want) and ix.last_search_path() == {"path": "fp16_chain", "reason": "explicit_fp16"}
        del ix


def test_banks_and_searches_the_screen_cannot_serve_end_on_the_fp32_kernel(cuda_device):
    M, D, k = 300_000, 768, 30
    dev = cuda_device
    # (1) one finite value beyond the fp16 range (65504)
    bank, q, g = _normal_bank(M, D, 7, dev)
    bank[12_345, 17] = 70_000.0
    auto, held = _pair(bank)
    for _ in range(2):
        assert _same(auto.search(q, k), held.search(q, k))
        assert auto.last_search_path() == {"path": "fp32", "reason": "overflow"}
    # (2) k beyond the candidate pass's 128: the fp32 kernel
    bank[12_345, 17] = 0.0
    auto, held = _pair(bank)
    assert _same(auto.search(q[:4096], 200), held.search(q[:4096], 200))
    assert auto.last_search_path() == {"path": "fp32", "reason": "k"}
    del auto, held, bank
    # (3) a tight token world (class centroids + a little noise, as tests/fuzz_small.py FUZZ_TIGHT builds them): the neighbours lie closer
    # together than fp16 resolves, certificates fail, the chain escalates and the adaptive use takes over -- the fp32 bits on every path
    for sigma in (0.03, 0.3):
        cent = torch.randn((21, D), generator=g, device=dev)
        bank = cent[torch.randint(0, 21, (M,), generator=g, device=dev)] + sigma * torch.randn((M, D), generator=g, device=dev)
        bank = torch.nn.functional.normalize(bank, dim=1)
        q = cent[torch.randint(0, 21, (NQ,), generator=g, device=dev)] + sigma * torch.randn((NQ, D), generator=g, device=dev)
        auto, held = _pair(bank)
        want = held.search(q, k)
        seen = []
        for _ in range(4):
            assert _same(auto.search(q, k), want), (sigma, seen)
            seen.append((auto.last_search_path(), auto.last_fp16_escalated(), auto.last_fp16_fallbacks()))
        print(f"token world sigma {sigma}: {seen}")
        assert seen[0][0] == {"path": "fp16_chain", "reason": "auto"}
        del auto, held, bank


def test_no_room_for_the_fp16_copy_never_costs_the_answer(cuda_device):
    M, D, k = 300_000, 768, 30
    bank, q, _ = _normal_bank(M, D, 9, cuda_device)
    auto, held = _pair(bank)
    want = held.search(q, k)
    auto.search(q[:64], k)                       # (a small search: the workspace's first allocations are made, no copy yet)
    torch.cuda.synchronize(); gc.collect(); torch.cuda.empty_cache()
    free0, total = torch.cuda.mem_get_info()
    copy = 300_032 * 768 * 2                     # the capacity is padded to 256 rows
    reserve = max(total // 16, 2 << 30)
    # the rule wants free memory ABOVE the copy + the reserve: leave 256 MiB less than that (the search's own workspace still fits many times)
    hog = torch.empty(free0 - (copy + reserve) + (256 << 20), dtype=torch.uint8, device=cuda_device)
    assert torch.cuda.mem_get_info()[0] < copy + reserve
    assert _same(auto.search(q, k), want)
    assert auto.last_search_path() == {"path": "fp32", "reason": "memory"}
    assert auto.last_fp16_fallbacks() == 0 and auto.last_fp16_escalated() == 0
    del hog
    torch.cuda.synchronize(); gc.collect(); torch.cuda.empty_cache()
    # room again -- but "no room at this capacity" is remembered: no new attempt per search, and no fp16 copy appears
    free1 = torch.cuda.mem_get_info()[0]
    assert _same(auto.search(q, k), want)
    assert auto.last_search_path() == {"path": "fp32", "reason": "memory"}
    free2 = torch.cuda.mem_get_info()[0]
    assert free1 - free2 < copy // 2, (free1, free2)
    # a bank that grows asks again, under the same rule
    auto.reserve(400_000)
    auto.add(bank[:1000]); held.add(bank[:1000])
    assert _same(auto.search(q, k), held.search(q, k))
    assert auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"}
    # nothing leaks: closing both indexes gives back all they held
    auto.close(); held.close()
    del auto, held, bank, want
    torch.cuda.synchronize(); gc.collect(); torch.cuda.empty_cache()
    free3 = torch.cuda.mem_get_info()[0]
    assert free3 >= free0 + 2 * 300_032 * 768 * 4 - (64 << 20), (free0, free3)


def test_kernel_clock_after_an_escalation_describes_the_candidate_launch(cuda_device):
    """The nested searches of uncertified queries (second fp16 pass, fp32 kernel) reuse the index's workspace: they neither stamp nor count as the
    last launch, and the candidate launch's stamps are kept aside for hb_index_kernel_clock / hb_index_wg_stamps."""
    M, D, k = 300_000, 768, 30
    bank, q, g = _normal_bank(M, D, 11, cuda_device)
    # 100 rows that fp16 cannot tell apart, and queries next to them: their first certificate (k' = 64 candidates) must fail
    bank[1000:1100] = torch.nn.functional.normalize(bank[1000:1001] + 1e-5 * torch.randn((100, D), generator=g, device=cuda_device), dim=1)
    q[:300] = 3.0 * bank[1000:1001] + 1e-3 * torch.randn((300, D), generator=g, device=cuda_device)
    auto, held = _pair(bank)
    auto.set_timing(True)
    got = auto.search(q, k)
    assert auto.last_search_path() == {"path": "fp16_chain", "reason": "auto"}
    assert auto.last_fp16_escalated() >= 300, auto.last_fp16_escalated()
    info = auto.schedule_info()
    st = auto.wg_stamps()
    clock = auto.kernel_clock()
    print("escalated", auto.last_fp16_escalated(), "fell back", auto.last_fp16_fallbacks(), info, clock, "knn ms", auto.last_knn_ms())
    assert st.shape[0] == info["workgroups"] == 256 and info["query_tiles"] == 86
    assert (st[:, 1] > st[:, 0]).all(), "a workgroup of the candidate launch did not stamp"
    assert 0.5 < clock["ghz_min"] <= clock["ghz"] <= clock["ghz_max"] < 3.0
    assert 0.0 < clock["span_ms"] <= auto.last_knn_ms() * 1.05 + 0.05      # (the stamps cover the search's last phase, the events all phases)
    assert _same(got, held.search(q, k))


def test_the_plugin_leaves_the_index_automatic_unless_told_otherwise(cuda_device):
    """NearestNeighborSearchHIP: use_fp16=False keeps the index's automatic state, exact_screen=False selects the fp32 kernel and fp32 memory only,
    use_fp16=True mode 2 as before -- one answer."""
    from hbird_mi.nn.search_hip import NearestNeighborSearchHIP
    M, D, k = 300_000, 768, 30
    bank, q, _ = _normal_bank(M, D, 13, cuda_device)
    fm, qh = bank.cpu(), q.cpu()
    del bank
    got = {}
    for name, kw, want in (("default", {}, {"path": "fp16_chain", "reason": "auto"}),
                           ("fp32 only", {"exact_screen": False}, {"path": "fp32", "reason": "explicit_fp32"}),
                           ("use_fp16", {"use_fp16": True}, {"path": "fp16_chain", "reason": "explicit_fp16"}),
                           ("use_fp16 wins", {"use_fp16": True, "exact_screen": False}, {"path": "fp16_chain", "reason": "explicit_fp16"})):
        nn = NearestNeighborSearchHIP(fm, n_neighbors=k, distance_measure="dot_product", gpu_ids=[0], **kw)
        idx, dist = nn.find_nearest_neighbors(qh)
        assert nn.index.last_search_path() == want, (name, nn.index.last_search_path())
        got[name] = (torch.as_tensor(idx), torch.as_tensor(dist))
        del nn
    for name in got:
        assert _same(got[name], got["fp32 only"]), name
