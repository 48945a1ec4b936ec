#!/usr/bin/env python3
"""Seeded random lives of one index, a numpy model of it, and the driver that holds an index to the model on every read path.

An index (csrc/hbird_internal.h: hb_index) is not stateless between calls: about twenty device workspaces are re-carved per call and reused
at another size by the next one, and caches and sticky records (the work list, the lazy fp16 / row copies, bmax, the screen record, the
adaptive fp16 policy, the row-group count, the label capacity) stay right only if every mutator tells them.  A LIFE is a seeded sequence of
about 40 operations -- mutators, readers and refusals interleaved -- generated here without a GPU:

    Model         a plain numpy index: the rows as stored (oracle.normalize_rows where normalize=True), label rows and their form (fp32 or
                  counts over P), row groups, metric, D, C and every setting made.  Its readers ARE the expectations: oracle.knn_chain_f32 for
                  neighbour lists, the float64 K5 restatement of tests/test_aggregate_paths_gpu.py for label_hat.
    FakeIndex     the Model behind the HipFlatIndex interface (tensors in, tensors out), with three optional planted faults: the CPU tests run
                  the driver against it to show that the harness has teeth.
    generate      seed -> (head, ops): what the life picks at its start and the list of operations (plain dicts of small numbers; the arrays
                  are re-derived from (seed, step) by make_rows / make_labels / make_queries).
    run_life      drives any index factory -- HipFlatIndex on the GPU, FakeIndex on the CPU -- through the operations and checks every reader.

    python tests/index_life.py SEED [UPTO]        prints a life (its first UPTO operations) without running it
    python tests/index_life.py SEED steered       ... of a life that also draws the steering calls

No GPU is needed here and nothing of torch.cuda is touched: the device side comes in through the `Env` a caller hands to run_life.
"""
from __future__ import annotations

import hashlib
import os
import sys
from collections import OrderedDict

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "open-hummingbird-eval_amd"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402  (CPU tensors stand for device I/O in the fake; no torch.cuda call in this file)

import bank_refs as R  # noqa: E402
import oracle  # noqa: E402

F32 = np.float32
P_COUNTS = 196                       # denominator of the count form (a 14 x 14 patch)
DS = (20, 48, 64, 96)                # 20 is padded, 48 runs the LDS-staged kernel, 64 and 96 the register-fed one
CS = (5, 21, 151)                    # the grouped, generic and wide K5 bodies
NQS = (1, 37, 256, 257, 300, 700)    # both sides of the 256-query tile
KS = (1, 10, 30, 32, 33, 90, 128, 130, 300)      # lists / pools at 32, the candidate pass' limit at 128, the ceiling passes at 256
CHUNKS = (1, 5, 31, 32, 33, 255, 256, 257, 1000, 3000)
MAX_ROWS, MAX_OPS = 7000, 60
BIG_NQ = 24576                       # D = 96, 6,500 rows: the least batch (a multiple of 256) at which mode 2 takes the candidate pass at k <= 32
BIG_DISTINCT = 256                   # ... made of this many distinct queries, repeated: the oracle searches them once

PLAIN_MUTATORS = ("reserve", "add", "reset", "add_from", "select_rows", "set_row_groups", "label_form", "set_fp16", "set_fp16_centre",
                  "set_rerank_copy", "set_fp16_escalation", "set_exclusion_screen", "use_current_stream")
STEERING = ("set_tuning", "set_variant", "set_cluster", "set_search_options")
EXCLUDING_READERS = ("search_excluding", "search_aggregate_excluding", "search_aggregate_grid_excluding")
READERS = ("search", "search_scores", "search_excluding", "search_aggregate", "search_aggregate_bigk", "search_aggregate_grid",
           "search_aggregate_excluding", "search_aggregate_grid_excluding", "aggregate", "aggregate_grid", "reconstruct", "gather_labels",
           "copy_norms", "ntotal")
REFUSALS = ("k_zero", "k_2049", "aggregate_257", "excluding_after_add", "group_out_of_range", "grid_unsorted")
REFUSAL_TEXT = {"multi_excluding": "excluding searches are single-index", "k_zero": "k must be in [1, 2048]", "k_2049": "k must be in [1, 2048]", "aggregate_257": "k must be in [1, 256]",
                "excluding_after_add": "rows were added or removed since", "group_out_of_range": "outside [-1, ",
                "grid_unsorted": "ks must be strictly ascending"}
# a mutator that leaves the row-group table behind the rows cannot be the LAST mutator before a valid excluding search
NO_GROUPS_AFTER = ("add", "reset", "add_from")


def possible_pairs(steered: bool):
    """(most recent mutator kind, reader kind) pairs a life can contain."""
    muts = PLAIN_MUTATORS + (STEERING if steered else ())
    return [(m, r) for m in muts for r in READERS if not (m in NO_GROUPS_AFTER and r in EXCLUDING_READERS)]


# ---------------------------------------------------------------- arrays, re-derived from (seed, step)

def _rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def centre(seed, D):
    v = _rng(seed, 0, 7).standard_normal(D)
    return (v / np.linalg.norm(v)).astype(F32)


def _unit(rng, n, D):
    b = rng.standard_normal((n, D))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return b


def make_rows(seed, step, n, D, normalize=False, spread=False, plant=False):
    """Rows of an append: unit directions (x 3 where the append normalises, norms 0.5 .. 2 with spread), a few exact duplicates of row 0, with
    plant a 150-row cluster within 1e-4 of the life's centre.  Rows whose rounded norm depends on the order of a double sum
    (bank_refs.ambiguous: the one case K1 is allowed 2 ulp) are drawn again, so the stored rows have one answer."""
    rng = _rng(seed, step, 1)
    x = _unit(rng, n, D)
    if normalize:
        x *= 3.0
    elif spread:
        x *= rng.uniform(0.5, 2.0, (n, 1))
    x = x.astype(F32)
    if n >= 8:
        x[rng.integers(1, n, size=min(6, n // 4))] = x[0]
    if plant and n >= 200:
        a = int(rng.integers(0, n - 150))
        v = centre(seed, D)[None, :] + 1e-4 * rng.standard_normal((150, D))
        x[a:a + 150] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    for _ in range(16):
        bad = R.ambiguous(x, normalize)
        if not bad.any():
            break
        x[bad] = (_unit(rng, int(bad.sum()), D) * (3.0 if normalize else 1.0)).astype(F32)
    assert not R.ambiguous(x, normalize).any()
    return x


def make_labels(seed, step, n, C):
    """Dense label rows j / 196 as fp32 quotients (what K2 produces): valid in both forms."""
    j = _rng(seed, step, 2).integers(0, P_COUNTS + 1, (n, C))
    return (j.astype(F32) / F32(P_COUNTS)).astype(F32)


def make_queries(seed, step, nq, D, aim=False, every=False):
    """Unnormalised queries; with aim the first 40 point at the life's centre (the planted cluster).  BIG_NQ queries are BIG_DISTINCT
    distinct ones, repeated."""
    if nq == BIG_NQ:
        return np.ascontiguousarray(np.tile(make_queries(seed, step, BIG_DISTINCT, D, aim, True), (BIG_NQ // BIG_DISTINCT, 1)))
    rng = _rng(seed, step, 3)
    q = (3.0 * rng.standard_normal((nq, D))).astype(F32)
    if aim:
        m = nq if every else min(40, nq)
        q[:m] = (4.0 * centre(seed, D)[None, :] + 1e-3 * rng.standard_normal((m, D))).astype(F32)
    return q


def make_groups(seed, step, n, big):
    """Row groups: runs of 64 rows (ids 1 ..), a few rows in no group, with big the rows 0 .. 299 as ONE group 0 (k + 300 > 256: rung 1)."""
    g = (np.arange(n, dtype=np.int32) // 64) + 1
    g[_rng(seed, step, 4).integers(0, n, size=max(1, n // 50))] = -1
    if big and n >= 400:
        g[:300] = 0
    return g, int(g.max()) + 1


def make_qgroups(seed, step, nq, n_groups, bad=False):
    rng = _rng(seed, step, 5)
    pool = np.unique(np.concatenate([[-1, 0, min(1, n_groups - 1)], rng.integers(0, n_groups, size=3)])).astype(np.int32)
    qg = pool[rng.integers(0, len(pool), size=nq)]
    if bad:
        qg[nq // 2] = n_groups
    return qg.astype(np.int32)


def make_ids(seed, step, n, m, foreign):
    rng = _rng(seed, step, 6)
    ids = rng.integers(0, max(n, 1), size=m).astype(np.int64)
    if m >= 4:
        ids[1] = ids[0]
    if foreign and m >= 8:
        ids[2], ids[3], ids[5] = -1, n, n + 5
    return ids


# ---------------------------------------------------------------- expectations

_MEMO: "OrderedDict[tuple, tuple]" = OrderedDict()


def _digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).view(np.uint8).reshape(-1).data, digest_size=12).digest()


def knn(q, rows, k, metric):
    """oracle.knn_chain_f32, remembered by content (the fakes and the driver ask the same question); repeated queries are searched once."""
    q = np.ascontiguousarray(q, dtype=F32)
    if q.shape[0] == BIG_NQ:
        reps = BIG_NQ // BIG_DISTINCT
        assert np.array_equal(q[:BIG_DISTINCT], q[-BIG_DISTINCT:])
        i, d = knn(q[:BIG_DISTINCT], rows, k, metric)
        return np.tile(i, (reps, 1)), np.tile(d, (reps, 1))
    key = (_digest(q), q.shape, _digest(rows), rows.shape, int(k), int(metric))
    if key not in _MEMO:
        if rows.shape[0] == 0:
            out = (np.full((q.shape[0], k), -1, np.int64), np.full((q.shape[0], k), np.inf if metric else -np.inf, F32))
        else:
            out = oracle.knn_chain_f32(q, rows, int(k), "l2" if metric else "dot_product", 0)
        _MEMO[key] = out
        while len(_MEMO) > 256:
            _MEMO.popitem(last=False)
    i, d = _MEMO[key]
    return i.copy(), d.copy()


def _k5():
    import test_aggregate_paths_gpu as k5      # the project's float64 restatement of K5 and its bound (numpy only)
    return k5


def words(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _setting(name):
    def f(self, *a, **kw):
        self.settings[name] = (a, kw)
    f.__name__ = name
    return f


class Model:
    """One index in numpy.  Mutators carry the names and arguments of HipFlatIndex's; readers take and return numpy arrays."""

    def __init__(self, d, metric, device=0):
        self.d, self.metric, self.device = int(d), int(metric), int(device)
        self.rows = np.zeros((0, self.d), F32)
        self.labels = None
        self.P, self.C, self.cap = 0, 0, 0
        self.groups, self.n_groups = None, 0          # the table as set, and how many rows it covered
        self.settings = OrderedDict()
        self.version = 0

    # -- mutators
    @property
    def ntotal(self):
        return int(self.rows.shape[0])

    @property
    def nlabels(self):
        return 0 if self.labels is None else int(self.labels.shape[0])

    def _changed(self):
        self.version += 1

    def reserve(self, n):
        self.cap = max(self.cap, (int(n) + 255) // 256 * 256)
        self._changed()

    def _grow(self, n):
        if self.ntotal + n > self.cap:
            self.reserve(max(self.ntotal + n, self.cap + self.cap // 2))

    def reset(self):
        self.rows = np.zeros((0, self.d), F32)
        self.labels = None
        self.groups, self.n_groups = None, 0
        self._changed()

    def add(self, x, normalize=False):
        x = np.ascontiguousarray(_np(x), dtype=F32)
        self._grow(x.shape[0])
        self.rows = np.concatenate([self.rows, oracle.normalize_rows(x) if normalize else x])
        self._changed()

    def add_labels(self, lab):
        lab = np.ascontiguousarray(_np(lab), dtype=F32)
        self.labels = lab.copy() if self.nlabels == 0 else np.concatenate([self.labels, lab])
        self.C = int(lab.shape[1])
        self._changed()

    def set_num_classes(self, c):
        self.C = int(c)

    @property
    def num_classes(self):
        return self.C

    def set_label_denominator(self, P):
        if self.nlabels and int(P) != self.P:
            raise RuntimeError("hb_index_set_label_denominator: the index already holds label rows")
        self.P = int(P)
        self._changed()

    def labels_to_fp32(self):
        self.P = 0
        self._changed()

    @property
    def label_denominator(self):
        return self.P

    def set_row_groups(self, groups, n_groups=None):
        if groups is None:
            self.groups, self.n_groups = None, 0
        else:
            g = np.asarray(_np(groups)).reshape(-1).astype(np.int32)
            self.groups, self.n_groups = g, (int(g.max()) + 1 if n_groups is None else int(n_groups))
        self._changed()

    def _hand_groups(self, src, ids, appended):
        """HipFlatIndex._hand_groups: groups[ids] of a source whose table covers its rows"""
        if src.groups is None or len(ids) == 0 or len(src.groups) != src.ntotal:
            return
        part = src.groups[ids]
        if appended and self.groups is not None and len(self.groups) + len(part) == self.ntotal:
            part = np.concatenate([self.groups, part])
        if len(part) == self.ntotal:
            self.groups, self.n_groups = part, max(src.n_groups, self.n_groups)

    def add_from(self, src, ids):
        ids = np.asarray(_np(ids)).reshape(-1).astype(np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= src.ntotal):
            raise ValueError(f"hb_index_add_from: an id lies outside [0, {src.ntotal}) (the source's rows)")
        self._grow(len(ids))
        if src.nlabels:
            if self.ntotal == 0:
                self.P, self.C = src.P, src.C
            self.labels = src.labels[ids].copy() if self.nlabels == 0 else np.concatenate([self.labels, src.labels[ids]])
        self.rows = np.concatenate([self.rows, src.rows[ids]])
        self._hand_groups(src, ids, True)
        self._changed()

    def select_rows(self, ids):
        view = type(self)(self.d, self.metric, self.device)
        if self.nlabels:
            view.P, view.C = self.P, self.C
        ids_h = np.asarray(_np(ids)).reshape(-1).astype(np.int64)
        view.reserve(len(ids_h))
        view.add_from(self, ids_h)
        view.groups, view.n_groups = None, 0
        view._hand_groups(self, ids_h, False)
        return view

    def use_current_stream(self):
        pass

    def close(self):
        pass

    set_fp16, set_fp16_centre, set_rerank_copy = _setting("set_fp16"), _setting("set_fp16_centre"), _setting("set_rerank_copy")
    set_fp16_escalation, set_exclusion_screen = _setting("set_fp16_escalation"), _setting("set_exclusion_screen")
    set_tuning, set_variant, set_cluster, set_search_options = [_setting(n) for n in STEERING]

    # -- readers
    def norms(self):
        return R.norm32(self.rows)

    def copy_norms(self):
        return self.norms()

    def _lists(self, q, k, rows_of=None):
        """(ids, dist) of the best k rows, local ids; rows_of: the ascending row numbers searched (None: all)"""
        rows = self.rows if rows_of is None else self.rows[rows_of]
        i, d = knn(q, rows, k, self.metric)
        if rows_of is not None:
            i = np.where(i >= 0, rows_of[np.clip(i, 0, max(len(rows_of) - 1, 0))] if len(rows_of) else -1, -1)
        return i, d

    @staticmethod
    def _check_k(k, who="hb_index_search", top=2048):
        if not 1 <= int(k) <= top:
            raise RuntimeError(f"{who}: k must be in [1, {top}]")

    def search(self, q, k, id_base=0):
        self._check_k(k)
        i, d = self._lists(q, k)
        return np.where(i >= 0, i + int(id_base), -1), d

    def search_excluding(self, q, k, qgroups, id_base=0):
        self._check_k(k, "hb_index_search_excluding")
        if self.groups is None or len(self.groups) == 0:
            raise ValueError("hb_index_search_excluding: the index has no row-group table (hb_index_set_row_groups)")
        if len(self.groups) != self.ntotal:
            raise ValueError(f"hb_index_search_excluding: the row-group table covers {len(self.groups)} rows, the bank holds {self.ntotal} "
                             "(rows were added or removed since hb_index_set_row_groups: set the table again)")
        gmax = int(np.bincount(self.groups[self.groups >= 0], minlength=1).max())
        if k + gmax > 2048:
            raise ValueError("hb_exclude_plan_replay: k + gmax exceeds 2048")
        qg = np.asarray(qgroups).reshape(-1).astype(np.int64)
        if ((qg < -1) | (qg >= self.n_groups)).any():
            raise ValueError(f"hb_index_search_excluding: a query names a group outside [-1, {self.n_groups})")
        idx = np.empty((len(qg), k), np.int64)
        dist = np.empty((len(qg), k), F32)
        for g in np.unique(qg):
            sel = np.flatnonzero(qg == g)
            allowed = None if g < 0 else np.flatnonzero(self.groups != g)     # ascending: ties keep their order
            idx[sel], dist[sel] = self._lists(q[sel], k, allowed)
        return np.where(idx >= 0, idx + int(id_base), -1), dist

    def _label_hat(self, q, idx, dist, beta, id_base):
        out = _k5().reference(q, idx, dist, self.norms(), id_base, self.labels[:self.ntotal], id_base, beta, "l2" if self.metric else "ip")[0]
        return out.astype(F32)

    def _need_labels(self, who):
        if self.nlabels < self.ntotal or self.nlabels == 0:
            raise RuntimeError(f"{who}: label rows missing (hb_index_add_labels)")

    def aggregate(self, q, idx, dist, beta=0.02, id_base=0):
        if idx.shape[1] > 256:
            raise RuntimeError("hb_index_search_aggregate: k must be <= 256")
        return self._label_hat(q, idx, dist, beta, id_base)

    def aggregate_bigk(self, q, idx, dist, beta=0.02, id_base=0):
        return self._label_hat(q, idx, dist, beta, id_base)

    def search_aggregate(self, q, k, beta=0.02, id_base=0, want_neighbours=False, top=256):
        self._check_k(k)
        self._check_k(k, "hb_index_search_aggregate", top)
        self._need_labels("hb_index_search_aggregate")
        i, d = self.search(q, k, id_base)
        out = self._label_hat(q, i, d, beta, id_base)
        return (out, i, d) if want_neighbours else out

    def search_aggregate_bigk(self, q, k, beta=0.02, id_base=0, want_neighbours=False):
        return self.search_aggregate(q, k, beta, id_base, want_neighbours, top=2048)

    def _grid_call(self, q, idx, dist, kp, bp, id_base, out=None):
        if any(b <= a for a, b in zip(kp, kp[1:])):
            raise ValueError("hb_index_aggregate_grid: ks must be strictly ascending (no repeats)")
        return np.stack([self._label_hat(q, idx[:, :k], dist[:, :k], b, id_base) for k in kp for b in bp])

    def aggregate_grid(self, q, idx, dist, ks, betas, id_base=0):
        from hbird_mi.nn.search_hip import grid_plan
        plan = grid_plan(ks, betas)
        if plan.ks[-1] > idx.shape[1]:
            raise ValueError(f"aggregate_grid: the largest k ({plan.ks[-1]}) exceeds k_list ({idx.shape[1]}), the length of the given lists")
        return self._grid_call(q, idx, dist, plan.ks, plan.betas, id_base)

    def search_aggregate_grid(self, q, ks, betas, id_base=0, want_neighbours=False):
        self._need_labels("hb_index_search_aggregate_grid")
        i, d = self.search(q, max(ks), id_base)
        out = self.aggregate_grid(q, i, d, ks, betas, id_base)
        return (out, i, d) if want_neighbours else out

    def search_aggregate_excluding(self, q, k, qgroups, beta=0.02, id_base=0, want_neighbours=False):
        i, d = self.search_excluding(q, k, qgroups, id_base)
        out = self._label_hat(q, i, d, beta, id_base)
        return (out, i, d) if want_neighbours else out

    def search_aggregate_grid_excluding(self, q, ks, betas, qgroups, id_base=0, want_neighbours=False):
        i, d = self.search_excluding(q, max(ks), qgroups, id_base)
        out = self.aggregate_grid(q, i, d, ks, betas, id_base)
        return (out, i, d) if want_neighbours else out

    def _gather(self, table, ids, id_base=0):
        r = np.asarray(ids).reshape(-1).astype(np.int64) - int(id_base)
        ok = (r >= 0) & (r < table.shape[0])
        out = np.zeros((len(r), table.shape[1]), F32)
        out[ok] = table[r[ok]]
        return out

    def reconstruct(self, ids, id_base=0):
        return self._gather(self.rows, ids, id_base)

    def gather_labels(self, ids):
        return self._gather(self.labels, ids)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


# ---------------------------------------------------------------- the fake index

FAULTS = ("stale_append", "host_previous", "sticky_pools")


class FakeIndex(Model):
    """The Model behind HipFlatIndex's interface: a torch tensor among the arguments stands for device I/O (tensors come back), numpy for the
    host path.  fault: one of FAULTS --
      stale_append    searches ignore the rows of the last append until a reset
      host_previous   the host path returns the previous call's lists when that call was larger
      sticky_pools    the k > 32 path is used whenever the previous search at this (query tiles, bank tiles) used it; on a k <= 32 call it
                      loses the last entry of every list to the next best row
    `fired` collects clock["step"] of every call a fault changed."""
    fault = None
    clock = None

    def __init__(self, d, metric, device=0):
        super().__init__(d, metric, device)
        self.fired = self.fired_sink if getattr(self, "fired_sink", None) is not None else []
        self._visible, self._prev, self._pools, self._host, self._depth = None, None, {}, False, 0

    def reset(self):
        super().reset()
        self._visible = None

    def add(self, x, normalize=False):
        before = self.ntotal
        super().add(x, normalize)
        if self.fault == "stale_append" and before > 0:
            self._visible = before

    def last_search_path(self):
        return {"path": "fp32", "reason": "explicit_fp32"}

    def _lists(self, q, k, rows_of=None):
        clean = super()._lists(q, k, rows_of)
        out = clean
        if self.fault == "stale_append" and self._visible is not None:
            seen = np.arange(self._visible) if rows_of is None else rows_of[rows_of < self._visible]
            out = super()._lists(q, k, seen)
        if self.fault == "sticky_pools":
            key = ((q.shape[0] + 255) // 256, (self.ntotal + 255) // 256)
            pools = k > 32 or self._pools.get(key, False)
            if pools and k <= 32:
                i, d = super()._lists(q, k + 1, rows_of)
                out = (np.delete(i, k - 1, axis=1), np.delete(d, k - 1, axis=1))
            self._pools[key] = pools
        if self.fault == "host_previous":
            prev, self._prev = self._prev, clean
            if self._host and prev is not None and prev[0].shape[0] >= q.shape[0] and prev[0].shape[1] >= k and prev[0].size > q.shape[0] * k:
                out = (prev[0][:q.shape[0], :k].copy(), prev[1][:q.shape[0], :k].copy())
        if out is not clean and not (np.array_equal(out[0], clean[0]) and np.array_equal(words(out[1]), words(clean[1]))):
            self.fired.append(None if self.clock is None else self.clock.get("step"))
        return out

    def search_scores(self, q, k, id_base=0):
        return self.search(q, k, id_base)          # (a fake: its scores are its distances, and distances_from_scores leaves them)

    def distances_from_scores(self, q, scores):
        return scores

    @staticmethod
    def _wrap(name):
        inner = getattr(Model, name)

        def f(self, *args, **kwargs):
            dev = any(isinstance(a, torch.Tensor) for a in args) or any(isinstance(a, torch.Tensor) for a in kwargs.values())
            if self._depth:             # (a reader built on another reader: the caller's I/O side stands)
                return inner(self, *args, **kwargs)
            self._host, self._depth = not dev, 1
            try:
                out = inner(self, *[_np(a) if isinstance(a, torch.Tensor) else a for a in args],
                            **{n: _np(a) if isinstance(a, torch.Tensor) else a for n, a in kwargs.items()})
            finally:
                self._depth = 0
            if not dev:
                return out
            return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out) if isinstance(out, tuple) else torch.from_numpy(np.ascontiguousarray(out))
        f.__name__ = name
        return f


for _name in ("search", "search_excluding", "aggregate", "aggregate_bigk", "search_aggregate", "search_aggregate_bigk", "_grid_call", "aggregate_grid",
              "search_aggregate_grid", "search_aggregate_excluding", "search_aggregate_grid_excluding", "reconstruct", "gather_labels"):
    setattr(FakeIndex, _name, FakeIndex._wrap(_name))
FakeIndex.copy_norms = lambda self: torch.from_numpy(Model.copy_norms(self))


def fake_factory(fault=None, clock=None):
    """-> (make_index, fired): a factory of FakeIndex with this fault, and the list its indexes report to"""
    fired = []
    cls = type("FakeIndex_" + (fault or "clean"), (FakeIndex,), {"fault": fault, "clock": clock, "fired_sink": fired})
    return cls, fired


# ---------------------------------------------------------------- the generator

class _Shadow:
    """What the generator must know of the index to emit only valid operations and intended refusals: sizes and flags, no data."""

    def __init__(self, D, metric, C, P):
        self.D, self.metric, self.C, self.P = D, metric, C, P
        self.n = self.cap = 0
        self.groups_n, self.n_groups, self.gmax = 0, 0, 0      # rows the table covers (0: none)
        self.fp16 = "auto"
        self.lists_k = 0        # length of the lists a search left for `aggregate` / `aggregate_grid` (0: none)
        self.last_mut = None

    def grow(self, n):
        if self.n + n > self.cap:
            self.cap = (max(self.n + n, self.cap + self.cap // 2) + 255) // 256 * 256
        self.n += n


def generate(seed, steered=False, big=None, length=None):
    """-> (head, ops).  head: D, metric, C, P, fp16 (the life plants the near-duplicate cluster and aims queries at it), steered, big (the life
    holds the BIG_NQ batches that let the adaptive mode-2 policy reach its wide-first pass).  ops: dicts with "op", the mutator / reader /
    refusal kind in "kind", and the small numbers run_life needs."""
    rng = _rng(seed, 99)
    big = (seed % 6 == 5 and not steered) if big is None else big
    D = 96 if big else DS[seed % 4]
    head = dict(seed=seed, D=D, metric=int(rng.integers(0, 2)) if not big else 0, C=CS[(seed // 2) % 3], P=P_COUNTS if seed % 2 else 0,
                fp16=bool(seed % 3 != 1) or big, steered=bool(steered), big=bool(big))
    s = _Shadow(D, head["metric"], head["C"], head["P"])
    ops = []
    pairs = possible_pairs(steered)
    # this life's share of the pair table: the steered lives deal the steering pairs among themselves first
    mine = [p for j, p in enumerate(p for p in pairs if (p[0] in STEERING) == steered) if j % (4 if steered else 12) == seed % (4 if steered else 12)]
    if steered:
        mine += [p for j, p in enumerate(p for p in pairs if p[0] not in STEERING) if j % 43 == seed % 43]
    mine = [mine[i] for i in rng.permutation(len(mine))]
    if length is not None:
        mine = mine[:length]

    def emit(op, kind=None, **kw):
        ops.append(dict(op=op, kind=kind or op, **kw))

    def pick(seq):
        return seq[int(rng.integers(0, len(seq)))]

    def add(n=None, **kw):
        if n is None:
            n = CHUNKS[(seed + len(ops)) % len(CHUNKS)]
        if s.n + n > MAX_ROWS - 500:
            reset(pick((300, 1000)))          # (a full bank: a new one first)
        crosses = s.n + n > s.cap
        emit("add", n=n, host=bool(rng.integers(0, 2)), normalize=bool(rng.integers(0, 2)), spread=bool(rng.integers(0, 2)),
             plant=bool(head["fp16"] and n >= 200 and kw.get("plant", n >= 1000)), crosses=crosses, ends_in_tile=(s.n + n) % 32 != 0)
        s.grow(n)
        s.last_mut = "add"

    def reset(n=None):
        n = n or pick((10, 300, 1000, 3000, 4257))
        other = bool(rng.integers(0, 2))
        if other:
            s.C = CS[(CS.index(s.C) + 1) % 3]
            s.P = 0 if s.P else P_COUNTS
        emit("reset", n=n, C=s.C, P=s.P, other=other, smaller=n < s.n, plant=bool(head["fp16"] and n >= 1000),
             host=bool(rng.integers(0, 2)), normalize=bool(rng.integers(0, 2)))
        s.n = 0
        s.grow(n)
        s.groups_n = s.n_groups = s.gmax = 0
        s.last_mut = "reset"

    def set_groups(big_group=None):
        big_group = bool(rng.integers(0, 2)) if big_group is None else big_group
        big_group = big_group and s.n >= 400
        emit("set_row_groups", big=big_group)
        s.groups_n, s.n_groups, s.gmax = s.n, (s.n - 1) // 64 + 2, 300 if big_group else 64
        s.last_mut = "set_row_groups"

    def mutate(kind):
        if kind == "add":
            return add()
        if kind == "reset":
            return reset()
        if kind == "set_row_groups":
            return set_groups()
        if kind == "reserve":
            above = bool(rng.integers(0, 2))
            n = s.cap + 256 * int(rng.integers(1, 4)) if above else max(1, s.n // 2)
            emit("reserve", n=n, above=above)
            s.cap = max(s.cap, (n + 255) // 256 * 256)
        elif kind == "add_from":
            m = 200
            if s.n + m > MAX_ROWS - 500:
                reset(pick((300, 1000)))
            emit("add_from", n_src=300, m=m, host=bool(rng.integers(0, 2)))
            s.grow(m)
        elif kind == "select_rows":
            m = max(1, (s.n * 7) // 10)
            emit("select_rows", m=m, host=bool(rng.integers(0, 2)))
            covered = s.groups_n == s.n and s.groups_n > 0
            s.n, s.cap = m, (m + 255) // 256 * 256
            s.groups_n = m if covered else 0
            s.gmax //= 2          # (a lower bound of what seven rows in ten leave of the largest group)
            if not covered:
                s.n_groups = s.gmax = 0
            s.fp16 = "auto"
        elif kind == "label_form":
            emit("label_form", to_fp32=bool(s.P))
            s.P = 0
        elif kind == "set_fp16":
            s.fp16 = pick((0, 1, 2, 1))
            emit("set_fp16", mode=s.fp16)
        elif kind == "set_fp16_centre":
            emit("set_fp16_centre", on=bool(rng.integers(0, 2)))
        elif kind == "set_rerank_copy":
            emit("set_rerank_copy", mode=int(rng.integers(0, 3)))
        elif kind == "set_fp16_escalation":
            emit("set_fp16_escalation", on=bool(rng.integers(0, 2)))
        elif kind == "set_exclusion_screen":
            emit("set_exclusion_screen", on=bool(rng.integers(0, 2)))
        elif kind == "use_current_stream":
            emit("use_current_stream", side=bool(rng.integers(0, 2)))
        elif kind == "set_tuning":
            emit("set_tuning", workgroups=pick((0, 17, 64, 256)), panel_tiles=0)
        elif kind == "set_variant":
            emit("set_variant", variant=pick((0, 3, 4, 6)))
        elif kind == "set_cluster":
            emit("set_cluster", cluster=pick(((0, 0, -1), (2, 2, 4), (2, 4, 16))))
        elif kind == "set_search_options":
            emit("set_search_options", phases=bool(rng.integers(0, 2)))
        else:
            raise KeyError(kind)
        s.last_mut = kind

    def read(kind, nq=None, k=None, host=None, base=None):
        nq = nq or pick(NQS)
        host = bool(rng.integers(0, 2)) if host is None else host
        aim = head["fp16"]
        if kind in ("search", "search_scores"):
            k = k or pick(KS)
            base = (pick((0, 0, 1 << 40, -5)) if kind == "search" else 0) if base is None else base
            emit(kind, nq=nq, k=k, host=host and kind == "search", id_base=base, aim=aim)
            if base == 0:
                s.lists_k = k if nq <= 700 else 0
        elif kind == "search_excluding":
            k = k or pick((1, 10, 30, 33, 90, 130))
            emit(kind, nq=nq, k=k, host=host, id_base=pick((0, 1000)), aim=aim, need=k + s.gmax)
        elif kind == "search_aggregate":
            emit(kind, nq=nq, k=k or pick((1, 10, 30, 32, 33, 90, 128, 130)), host=host, beta=pick((0.02, 0.07)), id_base=pick((0, 1000)), aim=aim)
        elif kind == "search_aggregate_bigk":
            emit(kind, nq=min(nq, 300), k=300, host=host, beta=0.02, id_base=0, aim=aim)
        elif kind == "search_aggregate_grid":
            emit(kind, nq=nq, ks=pick(((1, 10, 30), (10, 33, 90), (30, 300), (5, 32))), betas=pick(((0.02,), (0.02, 0.07))), host=host, id_base=0, aim=aim)
        elif kind == "search_aggregate_excluding":
            k = pick((10, 30, 90))
            emit(kind, nq=min(nq, 300), k=k, host=host, beta=0.02, id_base=0, aim=aim, need=k + s.gmax)
        elif kind == "search_aggregate_grid_excluding":
            ks = pick(((1, 10, 30), (10, 33)))
            emit(kind, nq=min(nq, 300), ks=ks, betas=(0.02, 0.07), host=host, id_base=0, aim=aim, need=max(ks) + s.gmax)
        elif kind in ("aggregate", "aggregate_grid"):
            if not 0 < s.lists_k <= 256:
                read("search", k=pick((10, 33, 90)), host=False, base=0)
                ops[-1]["kind"] = "(lists)"                     # (serves the next reader: not counted as this pair's reader)
            if kind == "aggregate":
                emit(kind, beta=pick((0.02, 0.07)))
            else:
                emit(kind, ks=tuple(sorted({1, max(1, s.lists_k // 2), s.lists_k})), betas=(0.02, 0.07))
        elif kind in ("reconstruct", "gather_labels"):
            emit(kind, m=pick((1, 37, 300)), host=host, foreign=True)
        else:
            emit(kind)       # copy_norms, ntotal
        ops[-1]["after"] = s.last_mut

    def refuse(kind):
        if kind in ("k_zero", "k_2049"):
            emit("refuse", kind, nq=37, k=0 if kind == "k_zero" else 2049, host=bool(rng.integers(0, 2)))
        elif kind == "aggregate_257":
            emit("refuse", kind, nq=37, k=257)
        elif kind == "excluding_after_add":
            set_groups(False)
            add(5)
            emit("refuse", kind, nq=37, k=10)
        elif kind == "group_out_of_range":
            if s.groups_n != s.n or s.n == 0:
                set_groups(False)
            emit("refuse", kind, nq=37, k=10, host=bool(rng.integers(0, 2)))
        elif kind == "grid_unsorted":
            if not 0 < s.lists_k <= 256:
                read("search", k=33, host=False, base=0)
                ops[-1]["kind"] = "(lists)"
            emit("refuse", kind, ks=(min(10, s.lists_k), 1))
        # after each refusal the next valid reader must be right
        if kind == "group_out_of_range":
            read("search_excluding", nq=37, k=10)
        else:
            read("search", nq=37)
        ops[-1]["after_refusal"] = kind

    # the bank: a capacity, then appends up to a few thousand rows (4,096 is the least at which the second fp16 pass exists)
    emit("reserve", n=pick((1000, 4096, 5000)), above=True)
    s.cap = (ops[-1]["n"] + 255) // 256 * 256
    if big:
        add(3000, plant=False); add(3000, plant=False); add(500, plant=True)
    else:
        add(3000 if head["fp16"] else pick((1000, 3000)))
        add(pick((1000, 257, 1000)) if head["fp16"] else pick(CHUNKS))
        if head["fp16"]:
            add(pick((5, 31, 257)))
            emit("set_fp16", mode=1); s.fp16 = 1
            emit("set_rerank_copy", mode=1)
    # the sizes that follow one another: 37 queries after 700, k = 10 after k = 300, the host path after a larger device call; then lists and
    # pools back to back at one (query tiles, bank tiles)
    read("search", nq=700, k=300, host=False)
    read("search", nq=37, k=10, host=True)
    read("search", nq=300, k=33, host=False)
    read("search", nq=300, k=32, host=False)
    if big:
        emit("set_fp16", mode=2); s.fp16 = 2
        for _ in range(3):
            read("search", nq=BIG_NQ, k=10, host=False, base=0)
    refusals = [REFUSALS[(seed + j) % len(REFUSALS)] for j in range(2)]
    for j, (m, r) in enumerate(mine):
        if r in EXCLUDING_READERS and m != "set_row_groups" and (s.groups_n != s.n or s.n == 0 or j % 3 == 0):
            set_groups(big_group=(seed + j) % 2 == 0)
        mutate(m)
        assert r not in EXCLUDING_READERS or (s.groups_n == s.n and s.n > 0), (seed, m, r)
        read(r)
        if refusals and j % 4 == 3:
            refuse(refusals.pop())
    for kind in refusals:
        refuse(kind)
    assert len(ops) <= MAX_OPS, (seed, len(ops))
    return head, ops


def describe(op):
    return op["op"] + ("" if op["kind"] in (op["op"], None) else f"[{op['kind']}]") + "(" + ", ".join(
        f"{n}={v}" for n, v in op.items() if n not in ("op", "kind", "after", "after_refusal", "crosses", "ends_in_tile", "smaller", "other", "need", "above")) + ")"


# ---------------------------------------------------------------- the driver

class Env:
    """What run_life needs from the side that owns the device.  The defaults serve the fakes: a CPU tensor stands for a device tensor."""
    paths = None                # a list: last_search_path()["path"] of every kNN reader with k <= 128 is appended

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def sync(self):
        pass

    def stream(self, side):     # make the side stream (or the default one again) the current stream
        pass

    def step(self, i):
        pass

    def done(self):
        pass


class LifeFailure(AssertionError):
    def __init__(self, seed, step, op, since_reset, what):
        self.seed, self.step, self.op = seed, step, op
        super().__init__(f"life {seed}, step {step}: {describe(op)}: {what}\n  since the last reset:\n    " + "\n    ".join(since_reset))


def _default_settings(ix, steering=False):
    return [(n, a, kw) for n, (a, kw) in ix.settings.items() if steering or n not in STEERING]


def run_life(make_index, life, env=None, upto=None):
    """Run the life `(head, ops)` on make_index(D, metric, 0) and hold every reader to the model.  -> {path name: readers it served}.
    Raises LifeFailure(seed, step, op, ops since the last reset, what differs)."""
    hist = {}
    for _ in life_steps(make_index, life, env, hist, upto):
        pass
    return hist


def run_interleaved(make_index, lives, envs=None):
    """Several lives on indexes of their own, alternating operation by operation.  -> one histogram per life."""
    envs = envs or [Env() for _ in lives]
    hists = [{} for _ in lives]
    runs = [life_steps(make_index, life, env, hist) for life, env, hist in zip(lives, envs, hists)]
    try:
        live = list(runs)
        while live:
            for r in list(live):
                try:
                    next(r)
                except StopIteration:
                    live.remove(r)
    finally:
        for r in runs:
            r.close()
    return hists


def life_steps(make_index, life, env=None, hist=None, upto=None):
    """The driver as a generator: one operation per step (its number is yielded); the indexes are closed when it ends or is closed."""
    env = env or Env()
    hist = {} if hist is None else hist
    head, ops = life
    seed, D, metric = head["seed"], head["D"], head["metric"]
    model = Model(D, metric)
    ix = make_index(D, metric, 0)
    opened = [ix]
    fresh = {"version": None, "ix": None, "model": None}
    lists = {}
    since = []
    step = -1
    if head["P"]:
        ix.set_label_denominator(head["P"]); model.set_label_denominator(head["P"])

    def fail(what):
        raise LifeFailure(seed, step, ops[step], since, what)

    def same_lists(got, want, what):
        gi_, gd = _np(got[0]), _np(got[1])
        if gi_.shape != want[0].shape or not np.array_equal(gi_, want[0]):
            bad = np.argwhere(gi_ != want[0])[:1] if gi_.shape == want[0].shape else gi_.shape
            fail(f"{what}: neighbour ids differ from the oracle's (first at {bad})")
        if not np.array_equal(words(gd), words(want[1])):
            fail(f"{what}: distance words differ from the oracle's (first at {np.argwhere(words(gd) != words(want[1]))[:1]})")

    def the_fresh():
        """an index built from the model: same rows, label form and settings except steering"""
        if fresh["version"] != (id(model), model.version, tuple(model.settings.items())):
            if fresh["ix"] is not None:
                fresh["ix"].close()
            f = make_index(D, metric, 0)
            for n, a, kw in _default_settings(model):
                getattr(f, n)(*a, **kw)
            if model.P:
                f.set_label_denominator(model.P)
            if model.ntotal:
                f.reserve(model.ntotal)
                f.add(env.dev(model.rows))
                if model.nlabels:
                    f.add_labels(env.dev(model.labels)); f.set_num_classes(model.C)
            if model.groups is not None and len(model.groups) == model.ntotal and model.ntotal:
                f.set_row_groups(model.groups, model.n_groups)
            env.sync()
            fresh.update(version=(id(model), model.version, tuple(model.settings.items())), ix=f)
        fresh["ix"].use_current_stream()          # (its caller's tensors live on the current stream, which a life may have changed)
        return fresh["ix"]

    def label_hat(got, call, q, idx, dist, k, beta, id_base, what):
        """bit for bit the fresh index's, and within the float64 bound of the K5 restatement on the returned lists"""
        got = _np(got)
        again = call(the_fresh())
        env.sync()              # (the fresh index works on a stream of its own: before its output is read)
        again = _np(again)
        if not np.array_equal(words(got), words(again)):
            fail(f"{what}: label_hat differs from the same call on a fresh index ({int((words(got) != words(again)).sum())} words)")
        k5 = _k5()
        name = "l2" if metric else "ip"
        norms, labels = model.norms(), model.labels[:model.ntotal]
        ref, _, logits = k5.reference(q, idx, dist, norms, id_base, labels, id_base, beta, name)
        tol = k5.tolerance(q, idx, dist, norms, id_base, logits, k, beta, name, float(labels.max()) if labels.size else 1.0)
        err = np.abs(got.astype(np.float64) - ref).max(axis=1)
        if not (err <= tol).all():
            i = int((err / tol).argmax())
            fail(f"{what}: |label_hat - float64| = {err[i]:.3e} > bound {tol[i]:.3e} at query {i}")

    def grid_hat(got, call, q, idx, dist, ks, betas, id_base, what):
        from hbird_mi.nn.search_hip import grid_plan
        plan = grid_plan(ks, betas)
        got = _np(got)
        again = call(the_fresh())
        env.sync()
        again = _np(again)
        if got.shape != again.shape or not np.array_equal(words(got), words(again)):
            fail(f"{what}: the grid differs from the same call on a fresh index")
        k5 = _k5()
        name = "l2" if metric else "ip"
        norms, labels = model.norms(), model.labels[:model.ntotal]
        for row, (k, beta) in enumerate(plan.configs):
            ref, _, logits = k5.reference(q, idx[:, :k], dist[:, :k], norms, id_base, labels, id_base, beta, name)
            tol = k5.tolerance(q, idx[:, :k], dist[:, :k], norms, id_base, logits, k, beta, name, float(labels.max()) if labels.size else 1.0)
            err = np.abs(got[row].astype(np.float64) - ref).max(axis=1)
            if not (err <= tol).all():
                fail(f"{what}: configuration (k={k}, beta={beta}): |label_hat - float64| exceeds its bound by {(err / tol).max():.2f} x")

    def note_path(k):
        if k <= 128 and hasattr(ix, "last_search_path"):
            p = ix.last_search_path()["path"]
            hist[p] = hist.get(p, 0) + 1
            if env.paths is not None:
                env.paths.append(p)

    try:
        for step, op in enumerate(ops[:upto]):
            env.step(step)
            o, kind = op["op"], op["kind"]
            since.append(f"{step}: {describe(op)}")
            io = (lambda a: a) if op.get("host") else env.dev
            if o == "reserve":
                ix.reserve(op["n"]); model.reserve(op["n"])
            elif o in ("add", "reset"):
                if o == "reset":
                    del since[:-1]
                    ix.reset(); model.reset()
                    for x in (ix, model):
                        if x.label_denominator != op["P"]:
                            x.set_label_denominator(op["P"])
                x = make_rows(seed, step, op["n"], D, op["normalize"], op.get("spread", False), op["plant"])
                lab = make_labels(seed, step, op["n"], op["C"] if o == "reset" else model.C or head["C"])
                ix.add(io(x), normalize=op["normalize"]); model.add(x, op["normalize"])
                ix.add_labels(io(lab)); model.add_labels(lab)
                ix.set_num_classes(lab.shape[1])
            elif o == "add_from":
                src, msrc = make_index(D, metric, 0), Model(D, metric)
                opened.append(src)
                x, lab = make_rows(seed, step, op["n_src"], D), make_labels(seed, step, op["n_src"], model.C)
                for t in (src, msrc):
                    if model.P:
                        t.set_label_denominator(model.P)
                src.use_current_stream()
                src.add(env.dev(x)); msrc.add(x)
                src.add_labels(env.dev(lab)); msrc.add_labels(lab)
                src.set_num_classes(model.C)
                ids = make_ids(seed, step, op["n_src"], op["m"], False)
                ix.add_from(src, io(ids) if not op["host"] else ids); model.add_from(msrc, ids)
            elif o == "select_rows":
                ids = np.sort(_rng(seed, step, 8).permutation(model.ntotal)[:op["m"]]).astype(np.int64)
                ix = ix.select_rows(ids if op["host"] else env.dev(ids)); model = model.select_rows(ids)
                opened.append(ix)
            elif o == "set_row_groups":
                g, ng = make_groups(seed, step, model.ntotal, op["big"])
                ix.set_row_groups(g, ng); model.set_row_groups(g, ng)
            elif o == "label_form":
                for x in (ix, model):
                    x.labels_to_fp32() if op["to_fp32"] else x.set_label_denominator(0)
            elif o == "use_current_stream":
                env.stream(op["side"]); ix.use_current_stream()
            elif o in ("set_fp16", "set_rerank_copy"):
                getattr(ix, o)(op["mode"]); getattr(model, o)(op["mode"])
            elif o in ("set_fp16_centre", "set_fp16_escalation", "set_exclusion_screen"):
                getattr(ix, o)(op["on"]); getattr(model, o)(op["on"])
            elif o == "set_tuning":
                ix.set_tuning(op["workgroups"], op["panel_tiles"]); model.set_tuning(op["workgroups"], op["panel_tiles"])
            elif o == "set_variant":
                ix.set_variant(op["variant"]); model.set_variant(op["variant"])
            elif o == "set_cluster":
                ix.set_cluster(*op["cluster"]); model.set_cluster(*op["cluster"])
            elif o == "set_search_options":
                ix.set_search_options(op["phases"]); model.set_search_options(op["phases"])
            elif o == "refuse":
                text = REFUSAL_TEXT[kind]
                q = make_queries(seed, step, op.get("nq", 37), D)
                try:
                    if kind == "multi_excluding":
                        call = lambda t: getattr(t, op["entry"])(env.dev(q), 10, env.dev(np.zeros(len(q), np.int32)))      # noqa: E731
                        want = None
                    elif kind in ("k_zero", "k_2049"):
                        call, want = (lambda t: t.search(io(q), op["k"])), (lambda: model.search(q, op["k"]))
                    elif kind == "aggregate_257":
                        call, want = (lambda t: t.search_aggregate(env.dev(q), 257)), (lambda: model.search_aggregate(q, 257))
                    elif kind in ("excluding_after_add", "group_out_of_range"):
                        qg = make_qgroups(seed, step, len(q), max(model.n_groups, 1), bad=kind == "group_out_of_range")
                        call = lambda t: t.search_excluding(io(q), op["k"], qg if op.get("host") else env.dev(qg))      # noqa: E731
                        want = lambda: model.search_excluding(q, op["k"], qg)      # noqa: E731
                    else:
                        q0, i0, d0 = lists["q"], lists["idx"], lists["dist"]
                        call = lambda t: t._grid_call(env.dev(q0), env.dev(i0), env.dev(d0), list(op["ks"]), [0.02], 0,      # noqa: E731
                                                      env.dev(np.zeros((2, len(q0), model.C), F32)))
                        want = lambda: model._grid_call(q0, i0, d0, list(op["ks"]), [0.02], 0)      # noqa: E731
                    for who, f in (("the model", want), ("the index", lambda: call(ix))):
                        if f is None:
                            continue
                        try:
                            f()
                        except (RuntimeError, ValueError) as e:
                            if text not in str(e):
                                fail(f"{who} refused with another message: {e}")
                        else:
                            fail(f"{who} did not refuse (expected: {text!r})")
                finally:
                    env.sync()
            elif o in ("search", "search_scores"):
                q = make_queries(seed, step, op["nq"], D, op["aim"])
                want = model.search(q, op["k"], op["id_base"])
                if o == "search":
                    got = ix.search(io(q), op["k"], op["id_base"])
                    env.sync()
                else:
                    qd = env.dev(q)
                    idx, sc = ix.search_scores(qd, op["k"], op["id_base"])
                    env.sync()
                    if not metric and not np.array_equal(words(_np(sc)), words(want[1])):
                        fail("the ordering scores of an inner-product search are not its distances")
                    got = (idx, ix.distances_from_scores(qd, sc.clone()))
                    env.sync()
                note_path(op["k"])
                same_lists(got, want, o)
                if op["k"] <= 256 and op["nq"] <= 700 and op["id_base"] == 0:
                    lists.update(q=q, idx=_np(got[0]).copy(), dist=_np(got[1]).copy(), id_base=0)
            elif o == "search_excluding":
                q = make_queries(seed, step, op["nq"], D, op["aim"])
                qg = make_qgroups(seed, step, op["nq"], model.n_groups)
                got = ix.search_excluding(io(q), op["k"], qg if op["host"] else env.dev(qg), op["id_base"])
                env.sync()
                same_lists(got, model.search_excluding(q, op["k"], qg, op["id_base"]), o)
            elif o in ("search_aggregate", "search_aggregate_bigk", "search_aggregate_excluding"):
                q = make_queries(seed, step, op["nq"], D, op["aim"])
                kw = dict(beta=op["beta"], id_base=op["id_base"], want_neighbours=True)
                if o == "search_aggregate_excluding":
                    qg = make_qgroups(seed, step, op["nq"], model.n_groups)
                    call = lambda t: t.search_aggregate_excluding(io(q), op["k"], qg if op["host"] else env.dev(qg), **kw)      # noqa: E731
                    want = model.search_excluding(q, op["k"], qg, op["id_base"])
                else:
                    call = lambda t: getattr(t, o)(io(q), op["k"], **kw)      # noqa: E731
                    want = model.search(q, op["k"], op["id_base"])
                out, idx, dist = call(ix)
                env.sync()
                if o == "search_aggregate":
                    note_path(op["k"])
                same_lists((idx, dist), want, o)
                label_hat(out, lambda t: call(t)[0], q, want[0], want[1], op["k"], op["beta"], op["id_base"], o)
            elif o in ("search_aggregate_grid", "search_aggregate_grid_excluding"):
                q = make_queries(seed, step, op["nq"], D, op["aim"])
                kw = dict(id_base=op["id_base"], want_neighbours=True)
                if o == "search_aggregate_grid_excluding":
                    qg = make_qgroups(seed, step, op["nq"], model.n_groups)
                    call = lambda t: t.search_aggregate_grid_excluding(io(q), op["ks"], op["betas"], qg if op["host"] else env.dev(qg), **kw)      # noqa: E731
                    want = model.search_excluding(q, max(op["ks"]), qg, op["id_base"])
                else:
                    call = lambda t: t.search_aggregate_grid(io(q), op["ks"], op["betas"], **kw)      # noqa: E731
                    want = model.search(q, max(op["ks"]), op["id_base"])
                out, idx, dist = call(ix)
                env.sync()
                same_lists((idx, dist), want, o)
                grid_hat(out, lambda t: call(t)[0], q, want[0], want[1], op["ks"], op["betas"], op["id_base"], o)
            elif o == "aggregate":
                q0, i0, d0, b0 = lists["q"], lists["idx"], lists["dist"], lists["id_base"]
                call = lambda t: t.aggregate(env.dev(q0), env.dev(i0), env.dev(d0), beta=op["beta"], id_base=b0)      # noqa: E731
                out = call(ix)
                env.sync()
                label_hat(out, call, q0, i0, d0, i0.shape[1], op["beta"], b0, o)
            elif o == "aggregate_grid":
                q0, i0, d0, b0 = lists["q"], lists["idx"], lists["dist"], lists["id_base"]
                ks = [k for k in op["ks"] if k <= i0.shape[1]] or [i0.shape[1]]
                call = lambda t: t.aggregate_grid(env.dev(q0), env.dev(i0), env.dev(d0), ks, op["betas"], id_base=b0)      # noqa: E731
                out = call(ix)
                env.sync()
                grid_hat(out, call, q0, i0, d0, ks, op["betas"], b0, o)
            elif o in ("reconstruct", "gather_labels"):
                ids = make_ids(seed, step, model.ntotal, op["m"], op["foreign"])
                got = getattr(ix, o)(ids if op["host"] else env.dev(ids))
                env.sync()
                if not np.array_equal(words(_np(got)), words(getattr(model, o)(ids))):
                    fail(f"{o}: the rows differ from the model's")
            elif o == "copy_norms":
                got, again = ix.copy_norms(), the_fresh().copy_norms()
                env.sync()
                got, again = _np(got), _np(again)
                if not np.array_equal(words(got), words(again)):
                    fail("copy_norms: differs from a fresh index's")
            elif o == "ntotal":
                if ix.ntotal != model.ntotal:
                    fail(f"ntotal: {ix.ntotal}, the model holds {model.ntotal}")
            else:
                raise KeyError(o)
            env.sync()
            if kind in PLAIN_MUTATORS + STEERING and ix.ntotal != model.ntotal:
                fail(f"after {o}: ntotal {ix.ntotal}, the model holds {model.ntotal}")
            yield step
    finally:
        env.sync()
        env.stream(False)
        for x in opened + ([fresh["ix"]] if fresh["ix"] is not None else []):
            x.close()
        env.done()


# ---------------------------------------------------------------- what a list of lives reaches (generator only)

def coverage(lives):
    """-> (pairs seen, set of named conditions some life meets).  From the operations alone."""
    pairs, met = set(), set()
    for head, ops in lives:
        last_mut, prev = None, None
        refused = None
        for op in ops:
            kind = op["kind"]
            if kind in PLAIN_MUTATORS + STEERING:
                last_mut = kind
                if kind == "add":
                    met |= ({"append_ends_inside_a_tile"} if op["ends_in_tile"] else set()) | ({"append_crosses_the_capacity"} if op["crosses"] else set())
                if kind == "reset":
                    met |= ({"reset_to_a_smaller_bank"} if op["smaller"] else set()) | ({"reset_to_another_C_and_label_form"} if op["other"] else set())
            elif op["op"] == "refuse":
                refused = kind
            elif kind in READERS or kind == "(lists)":
                if kind in READERS and last_mut is not None:
                    pairs.add((last_mut, kind))
                if refused is not None:
                    met.add("refusal_then_reader:" + refused)
                    refused = None
                if "nq" in op and "k" in op and prev is not None:
                    if op["nq"] == 37 and prev["nq"] == 700:
                        met.add("37_queries_after_700")
                    if op["k"] == 10 and prev["k"] == 300:
                        met.add("k_10_after_k_300")
                    if (op["nq"] + 255) // 256 == (prev["nq"] + 255) // 256 and (op["k"] <= 32) != (prev["k"] <= 32):
                        met.add("lists_and_pools_back_to_back")
                    if op.get("host") and not prev.get("host") and prev["nq"] * prev["k"] > op["nq"] * op["k"]:
                        met.add("host_call_after_a_larger_device_call")
                if op.get("need", 0) > 256 and kind in EXCLUDING_READERS:
                    met.add("excluding_need_beyond_256")
                prev = op if "nq" in op and "k" in op else None
            if kind in PLAIN_MUTATORS and kind in ("add", "reset", "add_from", "select_rows"):
                prev = None           # (another bank: not the same bank tiles)
    return pairs, met


CONDITIONS = ("append_ends_inside_a_tile", "append_crosses_the_capacity", "reset_to_a_smaller_bank", "reset_to_another_C_and_label_form",
              "37_queries_after_700", "k_10_after_k_300", "lists_and_pools_back_to_back", "host_call_after_a_larger_device_call",
              "excluding_need_beyond_256") + tuple("refusal_then_reader:" + r for r in REFUSALS)


def max_rows(life):
    n = top = 0
    for op in life[1]:
        if op["op"] == "reset":
            n = 0
        if op["op"] in ("add", "reset"):
            n += op["n"]
        elif op["op"] == "add_from":
            n += op["m"]
        elif op["op"] == "select_rows":
            n = op["m"]
        top = max(top, n)
    return top


# the committed lives: 12 plain, 4 steered, 2 interleaved pairs (two lives of different D, alternating operation by operation)
PLAIN_SEEDS = tuple(range(101, 113))
STEERED_SEEDS = (201, 202, 203, 204)
PAIR_SEEDS = ((301, 302), (303, 304))
PAIR_LENGTH = 9          # pairs of the table per life of an interleaved pair: they run two at a time


def committed_lives():
    return ([generate(s) for s in PLAIN_SEEDS] + [generate(s, steered=True) for s in STEERED_SEEDS]
            + [generate(s, big=False, length=PAIR_LENGTH) for pair in PAIR_SEEDS for s in pair])


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    _seed = int(sys.argv[1])
    _steered = "steered" in sys.argv[2:] or _seed in STEERED_SEEDS
    _upto = next((int(a) for a in sys.argv[2:] if a.isdigit()), None)
    _head, _ops = generate(_seed, steered=_steered)
    print("life", _head)
    for _i, _op in enumerate(_ops[:_upto]):
        print(f"{_i:3d}  {describe(_op)}" + (f"      <- after {_op['after']}" if "after" in _op else ""))
    print(f"{len(_ops)} operations, at most {max_rows((_head, _ops))} rows")
