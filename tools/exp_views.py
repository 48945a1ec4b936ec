"""add_from against the staged route (reconstruct + add + gather_labels + add_labels), HIP events on the index's stream, median of 5 after 2 warm-ups.
usage: exp_views.py ROWS D   |   exp_views.py sweep      (one JSON line per result; EXP_VIEWS_OUT=file collects them)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "open-hummingbird-eval_amd"), ROOT]
import numpy as np
import torch
from hbird_mi.nn.search_hip import HipFlatIndex
from hbird_mi.views import view_rows

OUT = os.environ.get("EXP_VIEWS_OUT")       # optional: a file that collects the JSON lines


def emit(d):
    print(json.dumps(d), flush=True)
    if OUT:
        open(OUT, "a").write(json.dumps(d) + "\n")


def timed(fn, setup):
    ms = []
    for it in range(7):
        state = setup()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(state); e1.record(); torch.cuda.synchronize()
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
        state.close()
    return float(np.median(ms)), ms


def shape(M, D, C=21, P=256):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    src = HipFlatIndex(D, 0, 0); src.use_current_stream(); src.set_label_denominator(P); src.reserve(M)
    for lo in range(0, M, 500_000):
        n = min(500_000, M - lo)
        src.add(torch.randn((n, D), generator=g, device="cuda"), normalize=True)
        cnt = torch.zeros((n, C), device="cuda"); cnt[:, 0] = P - 3; cnt[torch.arange(n), torch.randint(1, C, (n,), generator=g, device="cuda")] = 3
        src.add_labels(cnt / P)
    src.set_num_classes(C)
    starts = list(range(0, M, 196)) + [M]
    prefix = view_rows(starts, per_block=19).cuda()
    n = prefix.numel()
    perm = torch.randperm(M, generator=g, device="cuda")[:n].contiguous()
    dp = (D + 15) // 16 * 16
    view_bytes = n * (dp * 4 + 8 + ((C + 7) // 8 * 8) * 2)

    def setup():
        d = HipFlatIndex(D, 0, 0); d.use_current_stream(); d.set_label_denominator(P); d.reserve(n)
        return d

    def staged(ids):
        def run(d):
            for lo in range(0, n, 500_000):
                c = ids[lo:lo + 500_000]
                d.add(src.reconstruct(c), normalize=False)
                d.add_labels(src.gather_labels(c))
        return run

    for name, ids in (("prefix_196_19", prefix), ("random_permutation", perm)):
        t_new, all_new = timed(lambda d: d.add_from(src, ids), setup)
        t_old, all_old = timed(staged(ids), setup)
        emit({"rows": M, "d": D, "view_rows": n, "selection": name, "add_from_ms": t_new, "add_from_all_ms": all_new, "staged_ms": t_old,
              "staged_all_ms": all_old, "view_bytes": view_bytes, "roofline_ms_2x_view_bytes_at_8TBs": 2 * view_bytes / 8e12 * 1e3,
              "add_from_fraction_of_roofline": 2 * view_bytes / 8e12 * 1e3 / t_new, "staged_over_add_from": t_old / t_new})
    src.close()


def sweep():
    from hbird_mi.hbird_eval import hbird_evaluation

    class PoolViT(torch.nn.Module):
        def forward(self, x):
            return x

    def fn(model, imgs):
        return torch.nn.functional.avg_pool2d(imgs, 8).flatten(2).transpose(1, 2).contiguous(), None

    def call(**kw):
        torch.manual_seed(77)
        return hbird_evaluation(PoolViT(), d_model=3, patch_size=8, dataset_name="synthetic", data_dir="", batch_size=8, input_size=64,
                                device="cuda", n_neighbours=30, nn_method="hip", ftr_extr_fn=fn, **kw)
    sizes = [32, 160, 640]
    call(memory_size=640)          # warm-up
    torch.cuda.synchronize(); t0 = time.perf_counter(); one = call(memory_size=640, memory_sizes=sizes); torch.cuda.synchronize(); t1 = time.perf_counter()
    sep = {s: call(memory_size=s) for s in sizes}; torch.cuda.synchronize(); t2 = time.perf_counter()
    emit({"sweep": "synthetic data module, 32 training images, sizes 32 / 160 / 640", "memory_sizes_call_s": t1 - t0, "three_calls_s": t2 - t1,
          "miou_sweep": one, "miou_separate": sep, "identical": all(one[s] == sep[s] for s in sizes)})


if __name__ == "__main__":
    if sys.argv[1] == "sweep":
        sweep()
    else:
        shape(int(sys.argv[1]), int(sys.argv[2]))
