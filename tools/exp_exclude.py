"""Excluding searches: what search_excluding(q, k, qgroups) costs -- through the rungs and through the certified fp16 screen
(set_exclusion_screen) -- against the plain search of the same index at k and at need = k + gmax.
HIP events on the index's stream, medians after warm-up, the four sides alternating inside every repetition.
  rows are dealt to groups of G consecutive rows (an image's patches); the queries are bank rows plus noise, each excluding its row's own
  group, as a training image does in a leave-one-image-out pass.
  default bank: isotropic random rows -- only the query's own row is sure to top its list, so every query certifies at level 0: the route's
  best case.  --image-world: the recipe of tests/excl_screen_refs.py scaled to ROWS x D -- a row = its class centre (20 classes) + a x its
  image's offset + 0.6 noise, normalised, a cycling through (0, 0.15, 0.5, 2.5) over the images: a quarter of the images fill the top of
  their own queries' lists, as the patches of one image of a real ViT bank do.
Per (G): ms of search(k), search(need), search_excluding(k) with the route off and on; the rungs, how many queries reached rung 1, which path
served the last rung; the route's level counts (last_exclusion_screen).
usage: exp_exclude.py [--image-world] [--no-need] [--groups G ...] [ROWS D NQ [K]]
       (default: cfg-2, 2,074,072 x 384, 12,544 queries, k = 30; groups of 196 and 967 rows; --no-need leaves search(need) out)
One JSON line per table; EXP_EXCLUDE_OUT=file collects them."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "open-hummingbird-eval_amd"), ROOT]
import numpy as np
import torch
from hbird_mi.nn.search_hip import HipFlatIndex, exclude_plan

OUT = os.environ.get("EXP_EXCLUDE_OUT")
GROUPS = (196, 967)
WARM, REPS = 2, 5
CHUNK = 500_000


def emit(d):
    print(json.dumps(d), flush=True)
    if OUT:
        open(OUT, "a").write(json.dumps(d) + "\n")


def ms_of(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def image_rows(lo, n, D, G, centres, g):
    """Rows lo .. lo + n of the image world with images of G consecutive rows; lo is a multiple of G (a chunk holds whole images)."""
    img = torch.arange(lo, lo + n, device="cuda") // G
    first, last = int(img[0]), int(img[-1])
    off = unit(torch.randn((last - first + 1, D), generator=g, device="cuda"))
    a = torch.tensor((0.0, 0.15, 0.5, 2.5), device="cuda")[img % 4]
    cls = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    return centres[cls] + a[:, None] * off[img - first] + 0.6 * unit(torch.randn((n, D), generator=g, device="cuda"))


def main(M, D, NQ, K, image_world=False, with_need=True, groups=GROUPS):
    for G in groups:
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        ix = HipFlatIndex(D, 0, 0); ix.use_current_stream(); ix.reserve(M)
        centres = unit(torch.randn((20, D), generator=g, device="cuda"))
        step = CHUNK // G * G if image_world else CHUNK          # (whole images per chunk)
        for lo in range(0, M, step):
            n = min(step, M - lo)
            ix.add(image_rows(lo, n, D, G, centres, g) if image_world else torch.randn((n, D), generator=g, device="cuda"), normalize=True)
        src = torch.randint(0, M, (NQ,), generator=g, device="cuda")
        noise = torch.randn((NQ, D), generator=g, device="cuda")
        q = ix.reconstruct(src) + 0.05 * (unit(noise) if image_world else noise / D ** 0.5)
        ix.set_row_groups(torch.arange(M, device="cuda") // G)
        qg = (src // G).to(torch.int32)
        gmax = min(G, M)
        rungs = exclude_plan(K, gmax)
        need = K + gmax
        t = {"search_k": [], "search_need": [], "excluding": [], "excluding_screen": []}
        info = path = screen = path_need = path_screen = ni = None
        for it in range(WARM + REPS):
            a, _ = ms_of(lambda: ix.search(q, K))
            path_k = ix.last_search_path()
            b = float("nan")
            if with_need:
                b, (ni, _) = ms_of(lambda: ix.search(q, need))
                path_need = ix.last_search_path()
            ix.set_exclusion_screen(False)
            c, (ei, ed) = ms_of(lambda: ix.search_excluding(q, K, qg))
            info, path = ix.last_exclusion(), ix.last_search_path()
            ix.set_exclusion_screen(True)
            d, (si, sd) = ms_of(lambda: ix.search_excluding(q, K, qg))
            screen, path_screen, info_screen = ix.last_exclusion_screen(), ix.last_search_path(), ix.last_exclusion()
            if it >= WARM:
                t["search_k"].append(a); t["search_need"].append(b); t["excluding"].append(c); t["excluding_screen"].append(d)
        same = bool(torch.equal(ei, si) and torch.equal(ed.view(torch.int32), sd.view(torch.int32)))
        equals = None
        if with_need:      # the result against its definition: the first K entries of the list at need whose group is not the query's
            rows = torch.arange(M, device="cuda") // G
            keep = rows[ni.clamp(min=0)] != qg[:, None].long()
            pos = torch.cumsum(keep, 1) - 1
            want = torch.full_like(ei, -1)
            sel = keep & (pos < K)
            want[torch.nonzero(sel)[:, 0], pos[sel]] = ni[sel]
            equals = bool(torch.equal(ei, want))
        med = {k: float(np.median(v)) for k, v in t.items()}
        emit({"bank": "image_world" if image_world else "isotropic", "rows": M, "d": D, "nq": NQ, "k": K, "group_rows": G, "gmax": info["gmax"], "need": need,
              "rungs": rungs, "ms_search_k": med["search_k"], "ms_search_need": med["search_need"] if with_need else None,
              "ms_search_excluding": med["excluding"], "ms_search_excluding_screen": med["excluding_screen"],
              "screen_over_rungs": med["excluding_screen"] / med["excluding"], "screen_over_search_k": med["excluding_screen"] / med["search_k"],
              "rungs_run": info["rungs"], "rung1_queries": info["rung1_queries"], "kf_last": info["kf"], "path_search_k": path_k,
              "path_last_rung": path, "path_search_need": path_need, "screen": screen, "path_screen": path_screen, "screen_leftover_rungs": info_screen,
              "equals_filtered_list_at_need": equals, "screen_equals_rungs_bitwise": same})
        ix.close()
        del ix, q, src, noise
        torch.cuda.empty_cache()


if __name__ == "__main__":
    argv = sys.argv[1:]
    image_world = "--image-world" in argv
    with_need = "--no-need" not in argv
    groups = GROUPS
    if "--groups" in argv:
        i = argv.index("--groups")
        j = i + 1
        while j < len(argv) and argv[j].isdigit():
            j += 1
        groups = tuple(int(v) for v in argv[i + 1:j])
        argv = argv[:i] + argv[j:]
    a = [int(v) for v in argv if not v.startswith("--")]
    main(*(a[:3] if len(a) >= 3 else (2_074_072, 384, 12_544)), a[3] if len(a) > 3 else 30, image_world=image_world, with_need=with_need, groups=groups)
