"""Hummingbird dense-retrieval evaluation on MI355X: the counterpart of the reference's
hbird/hbird_eval.py (class HbirdEvaluation 54-637, hbird_evaluation 640-722), same public names,
arguments, return values and error behaviour -- with the whole hot path device-resident:

  bank build   ViT tokens -> fused L2-normalise + fragment-tiled append (K1), patch soft labels from the
               mask histogram (K2), optional bounded-memory sampling (K3); nothing crosses to the host
               except the uniform noise the reference draws from torch's CPU generator (hbird_eval.py:500).
  query path   tokens -> exact brute-force kNN (K4, fused fp32-MFMA top-k) -> cosine-softmax label
               aggregation (K5) -> bilinear upsample + argmax (K6) -> confusion matrix (K7); only the
               [C,C] confusion matrix reaches the host, where the Hungarian mIoU tail runs.

With torch.distributed initialised (one process per GPU, backend "nccl" = RCCL) the bank is row-sharded
over the ranks in the reference's row order (contiguous ranges of training batches, successive ids), the
validation batches are dealt round-robin to the ranks, and every search is: all-gather(queries) -> local
shard search -> all-gather(top-k) -> merge -> aggregation against the all-gathered label table.
"""
from __future__ import annotations

import logging
import os
from typing import Any, Dict, List, Optional, Tuple

import torch

from hbird_mi import bootstrap as hboot
from hbird_mi import dist as hdist
from hbird_mi import ops
from hbird_mi import tiling
from hbird_mi import views
from hbird_mi.models import FeatureExtractor, FeatureExtractorSimple
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex, check_k, k5, merge_topk, merge_topk_packed, _METRICS
from hbird_mi.utils.eval_metrics import PredsmIoU

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    def tqdm(iterator, *args, **kwargs):
        return iterator

logger = logging.getLogger(__name__)
if not logger.handlers:
    _handler = logging.StreamHandler()
    _handler.setFormatter(logging.Formatter(fmt="%(asctime)s | %(levelname)s | %(name)s: %(message)s",
                                            datefmt="%H:%M:%S"))
    logger.addHandler(_handler)
    logger.setLevel(getattr(logging, os.environ.get("HBIRD_LOG_LEVEL", "WARNING").upper(), logging.WARNING))

_NN_METHODS = ("hip", "faiss", "scann")
# what the last hbird_evaluation() call did about its bank (the CLI prints it): bank_loaded, bank_build_s, bank_rows, train_batches_loaded
last_run_info: Dict[str, Any] = {}


def _check_beta(beta) -> float:
    """The softmax temperature of the label aggregation: a finite positive number (K5 refuses anything else)."""
    import math
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"beta={beta!r}: the softmax temperature must be a finite positive number")
    return float(beta)


class HbirdEvaluation:
    """Same constructor as the reference (hbird_eval.py:97-111).

    `nn_method`: "hip" (this engine), or the reference's names "faiss" (exact flat search: identical
    semantics, served by the HIP engine) and "scann" (the reference's approximate CPU backend is not
    re-implemented; the exact HIP search is used and a warning is logged).  `nn_params` keeps the Faiss
    keywords: distance_measure, idx_shard, use_fp16, gpu_ids (search_faiss.py:7); ScaNN-only keywords are
    accepted and ignored.

    `reuse_memory` (trailing keyword, not in the reference, whose constructor always rebuilds and overwrites the files,
    hbird_eval.py:165-172): when both `f_mem_p` and `l_mem_p` name existing files the bank is LOADED from them
    (`load_memory`) and the training loader is never touched; otherwise the bank is built and saved there as in the reference.
    `bank_loaded` / `bank_build_s` say which happened and how long it took.
    `beta` (trailing keyword): the softmax temperature of the label aggregation, the reference's literal 0.02 (hbird_eval.py:575-609).
    """

    def __init__(self, feature_extractor: torch.nn.Module, train_loader, num_classes: int, n_neighbours: int = 30,
                 augmentation_epoch: int = 1, device: torch.device | str = "cpu", nn_method: str = "scann",
                 nn_params: Optional[Dict[str, Any]] = None, memory_size: Optional[int] = None,
                 dataset_size: Optional[int] = None, f_mem_p: Optional[str] = None,
                 l_mem_p: Optional[str] = None, reuse_memory: bool = False, beta: float = 0.02) -> None:
        if nn_params is None:
            nn_params = {}
        self.nn_params = nn_params
        self.device = device
        self.nn_method = nn_method
        assert self.nn_method in _NN_METHODS, "Only hip, faiss and scann are supported"   # hbird_eval.py:121
        if self.nn_method == "scann":
            logger.warning("nn_method='scann': the approximate ScaNN CPU backend is replaced by the exact HIP search")
        if not torch.cuda.is_available():
            raise RuntimeError("HbirdEvaluation needs an MI355X: the HIP path has no CPU fallback")
        dev = torch.device(device)
        self.gpu = dev.index if dev.type == "cuda" and dev.index is not None else torch.cuda.current_device()
        self.gpu_device = torch.device("cuda", self.gpu)
        self.feature_extractor = feature_extractor.to(device)
        self.feature_extractor.eval()

        self.augmentation_epoch = augmentation_epoch
        self.memory_size = memory_size
        self.n_neighbours = n_neighbours
        self.beta = _check_beta(beta)
        self.num_classes = num_classes
        self.f_mem_p = f_mem_p
        self.l_mem_p = l_mem_p
        self.num_sampled_features: Optional[int] = None
        # geometry of a bank built here (memory_view): cumulative row offsets of the (epoch, image) blocks in build order, images per epoch
        # (rows kept per block by the bounded build: num_sampled_features).  A loaded bank has none.
        self._bank_block_starts: Optional[List[int]] = None
        self._dataset_images: Optional[int] = None
        self._dataset_size = dataset_size
        self.rank, self.world = hdist.rank_world()

        distance = str(nn_params.get("distance_measure", "dot_product")).lower()
        if distance not in _METRICS:
            raise ValueError(f"Unsupported distance measure: {distance}")                 # search_faiss.py:48
        self.metric = _METRICS[distance]
        gpu_ids = nn_params.get("gpu_ids")
        n_dev = torch.cuda.device_count()
        if gpu_ids is not None:
            for g in gpu_ids:
                if g >= n_dev or g < 0:
                    raise ValueError(f"Invalid GPU ID: {g}. Available GPUs: 0-{n_dev - 1}")    # search_faiss.py:25
        # GPUs of THIS process.  One process per GPU under torch.distributed; otherwise the reference's call shape
        # (hbird_eval.py:267-281 -> search_faiss.py:19-20, 50-76): every listed GPU, ALL of them by default, as row shards
        # (idx_shard=True) or replicas -- with the extractor's GPU first, the home of labels, merge and aggregation.
        if self.world > 1:
            self.local_gpus = [self.gpu]
        else:
            ids = [int(g) for g in gpu_ids] if gpu_ids is not None else list(range(n_dev))
            if self.gpu in ids:
                ids.remove(self.gpu)
                ids.insert(0, self.gpu)
            self.local_gpus = ids or [self.gpu]
            if self.local_gpus[0] != self.gpu:
                self.gpu = self.local_gpus[0]
                self.gpu_device = torch.device("cuda", self.gpu)
        check_k(n_neighbours, "n_neighbours")        # [1, 2048]: faiss-gpu's own range (the reference hands n_neighbours straight to it)
        # idx_shard keeps the reference's default (False, search_faiss.py:7): with several ranks that means a full bank
        # replica per rank and data-parallel validation batches (faiss.IndexReplicas, 65-74); idx_shard=True row-shards
        # the bank over the ranks (faiss.IndexShards, 53-63) -- the mode for banks that should not be built N times
        self.sharded = self.world > 1 and bool(nn_params.get("idx_shard", False))
        # label_shard (with idx_shard under torch.distributed; not in the reference): label_memory stays sharded with the bank instead of
        # being replicated on every rank (6.2 GB at BASELINE cfg-3, 16.7 GB for the full ADE20K bank); only the bank-row norms are
        # replicated (4 B per row) and every search ends in one more all-reduce of [queries, classes] partial sums
        self.label_shard = self.sharded and bool(nn_params.get("label_shard", False))
        self.compress_labels = bool(nn_params.get("compress_labels", True))
        if self.world > 1:
            logger.warning("torch.distributed world of %d ranks: bank %s (nn_params['idx_shard']=%s)", self.world,
                           "row-sharded over the ranks" if self.sharded else "replicated on every rank", self.sharded)
            if self.sharded or self.memory_size is not None:
                # sharded: every rank replays the ONE random stream of the reference; replicas with a bounded memory:
                # every rank samples the SAME patches (hbird_eval.py:500), so that all replicas are the same bank and the
                # all-reduced mIoU is that of a single process, whatever the ranks' own seeds were
                self._align_cpu_rng()

        eval_spatial_resolution = self.feature_extractor.eval_spatial_resolution
        logger.info("Initializing memory: nn_method=%s, memory_size=%s, augmentation_epoch=%s", self.nn_method,
                    str(self.memory_size), self.augmentation_epoch)
        if self.memory_size is not None:
            if dataset_size is None:
                raise ValueError("dataset_size must be provided when memory_size is set.")  # hbird_eval.py:144-145
            denom = dataset_size * self.augmentation_epoch
            self.num_sampled_features = max(1, self.memory_size // max(1, denom))           # 146-147
            # rows the build will fill (the reference preallocates memory_size and trims, 156-172): what shards split
            self._planned_rows = min(self.memory_size, self.num_sampled_features * max(1, denom))

        if len(self.local_gpus) > 1:
            self.index = HipMultiIndex(self.feature_extractor.d_model, self.metric, self.local_gpus,
                                       shard=bool(nn_params.get("idx_shard", False)))
            logger.info("one process, %d GPUs %s: bank %s", len(self.local_gpus), self.local_gpus,
                        "row-sharded (faiss.IndexShards)" if self.index.shard else "replicated (faiss.IndexReplicas)")
        else:
            self.index = HipFlatIndex(self.feature_extractor.d_model, self.metric, self.gpu)
        self.index.set_num_classes(num_classes)
        if nn_params.get("use_fp16", False):          # search_faiss.py:40; certified-exact fast mode, only where it pays
            self.index.set_fp16(2)                    # (rows x queries x D >= 1.5e10 (k' / 64)^2), like the plugin: never slower than fp32
            self.index.set_rerank_copy(int(nn_params.get("rerank_copy", 0)))   # 0 automatic (when memory allows), 1 always, 2 never
        if nn_params.get("fp16_centre", False):       # the screen's fp16 copy in its mean-centred form (HipFlatIndex.set_fp16_centre): same results
            self.index.set_fp16_centre(True)
        if nn_params.get("exclude_screen", False) and isinstance(self.index, HipFlatIndex):   # excluding searches on the fp16 screen: same results
            self.index.set_exclusion_screen(True)
        self.id_base = 0            # global id of this rank's first bank row
        self.total_rows = 0         # bank rows over all ranks
        self._label_table = None    # all-gathered labels / norms in sharded mode
        self.bank_loaded = False
        import time as _time
        t0 = _time.perf_counter()
        with torch.cuda.device(self.gpu_device):
            if reuse_memory and self._reusable_memory():
                # the saved bank of an earlier run: every rank takes its row range of the one file pair
                self.batches_loaded = 0
                self.bank_loaded = self.load_memory()
            if not self.bank_loaded:
                filled = self._create_memory(train_loader, num_classes=self.num_classes,
                                             eval_spatial_resolution=eval_spatial_resolution)
                logger.info("Memory rows: %s", filled)
                self._save_memory()
                self._finalize_shards()
            torch.cuda.synchronize(self.gpu_device)
        self.bank_build_s = _time.perf_counter() - t0

    @classmethod
    def from_index(cls, feature_extractor: torch.nn.Module, index, num_classes: int, n_neighbours: int = 30,
                   device: torch.device | str = "cuda", beta: float = 0.02) -> "HbirdEvaluation":
        """An evaluator over a bank that is already resident in a `HipFlatIndex` (rows + label rows added by the caller): `evaluate` runs
        as usual, nothing is built.  Not in the reference (its bank only ever comes from `_create_memory`); used by `bench.py --e2e` to time
        the evaluation loop against the synthetic 10 M-row bank, and handy for banks produced elsewhere."""
        check_k(n_neighbours, "n_neighbours")
        self = cls.__new__(cls)
        self.beta = _check_beta(beta)
        self.nn_params, self.device, self.nn_method = {}, device, "hip"
        dev = torch.device(device)
        self.gpu = dev.index if dev.type == "cuda" and dev.index is not None else torch.cuda.current_device()
        self.gpu_device = torch.device("cuda", self.gpu)
        self.feature_extractor = feature_extractor.to(device).eval()
        self.augmentation_epoch, self.memory_size, self.n_neighbours, self.num_classes = 1, None, n_neighbours, num_classes
        self.f_mem_p = self.l_mem_p = None
        self.num_sampled_features = None
        self.rank, self.world = 0, 1
        self.metric = index.metric
        self.local_gpus = [self.gpu]
        self.sharded = self.label_shard = False
        self.compress_labels = True
        self.index = index
        self.index.set_num_classes(num_classes)
        self.id_base, self.total_rows, self._label_table = 0, index.ntotal, None
        self.bank_loaded, self.bank_build_s, self.batches_loaded = True, 0.0, 0
        self._bank_block_starts = self._dataset_images = self._dataset_size = None      # no build geometry (memory_view: rows_per_image=)
        return self

    def _align_cpu_rng(self) -> None:
        """Sharded bank build: every rank replays the reference's single CPU random stream (the sampling noise of
        hbird_eval.py:500 is drawn for EVERY batch, owned or not), so all ranks must start from rank 0's state."""
        st = torch.get_rng_state().to(self.gpu_device)
        torch.distributed.broadcast(st, 0)
        torch.set_rng_state(st.cpu())

    # ------------------------------------------------------------------------------------------------
    # bank build (reference _create_memory, hbird_eval.py:283-369)
    # ------------------------------------------------------------------------------------------------
    def _create_memory(self, train_loader, num_classes: int, eval_spatial_resolution: int) -> Optional[int]:
        S = eval_spatial_resolution
        try:
            n_batches = len(train_loader)
        except TypeError:
            n_batches = None
        total_flat = None if n_batches is None else n_batches * self.augmentation_epoch
        if self.sharded:
            if total_flat is None:
                raise ValueError("a sharded bank build needs a train_loader with a length")
            own_lo, own_hi = hdist.shard_range(total_flat, self.rank, self.world)
        else:
            own_lo, own_hi = 0, float("inf")
        if self.memory_size is not None:
            self.index.reserve(max(1, self._planned_rows // max(1, self.world if self.sharded else 1)))
        state = {"presized": self.memory_size is not None}
        # Which batches this rank must actually LOAD.  Unbounded sharded build: only its own (hdist.rank_batches fetches just those
        # index batches from a DataLoader: rank r of N decodes 1 / N of the images).  Bounded memory: every batch, because the
        # reference's one random stream (500) is consumed for every batch by an amount that depends on its masks -- all ranks
        # replay it -- and the masks only come with their images.
        need_all = self.memory_size is not None or not self.sharded
        self.batches_loaded = 0
        self._mixed_patch_sizes = False
        self._bank_block_starts = [0]
        failure = None
        with torch.no_grad():
            for ep in tqdm(range(self.augmentation_epoch), desc="Augmentation loop"):
                base = ep * (n_batches or 0)
                batches = enumerate(train_loader) if need_all else hdist.rank_batches(train_loader, lambda i, b=base: own_lo <= b + i < own_hi)
                try:
                    self._create_memory_epoch(batches, base, n_batches, own_lo, own_hi, total_flat, num_classes, S, state)
                except Exception as e:          # noqa: BLE001 -- re-raised below, on every rank
                    failure = e
                # Sharded build: a rank that raised must not leave its peers waiting in the next collective (_finalize_shards, or the
                # bounded build's aligned random stream): one all-reduce per epoch end, and all ranks go on or none
                if self.sharded:
                    flag = torch.tensor([0 if failure is None else 1], device=self.gpu_device)
                    torch.distributed.all_reduce(flag)
                    if int(flag.item()) != 0:
                        if failure is not None:
                            raise failure
                        raise RuntimeError(f"the bank build failed on another rank (epoch {ep}); this rank stops with it")
                elif failure is not None:
                    raise failure
        self.id_base = 0          # a sharded build learns its id base from the ranks' row counts (_finalize_shards)
        n_blocks = len(self._bank_block_starts) - 1
        self._dataset_images = n_blocks // max(1, self.augmentation_epoch)
        return self.index.ntotal

    def _create_memory_epoch(self, batches, base, n_batches, own_lo, own_hi, total_flat, num_classes, S, state) -> None:
        """One pass over the training batches (the body of the reference's inner loop, hbird_eval.py:306-355)."""
        presized = state["presized"]
        for bi, (x, y) in tqdm(batches, desc="Memory Creation loop"):
            flat = base + bi if n_batches is not None else self.batches_loaded
            mine = own_lo <= flat < own_hi
            self.batches_loaded += 1
            y = y.to(self.gpu_device)
            y = (y * 255).long()                                   # hbird_eval.py:309
            bs = y.shape[0]
            input_size = x.shape[-1]
            patch_size = input_size // S                          # 313-314
            if self.index.ntotal == 0 and not self._mixed_patch_sizes:
                self._set_label_denominator(patch_size * patch_size)
            elif self.index.label_denominator not in (0, patch_size * patch_size):
                # the reference recomputes patch_size per batch (313-314) and its fp32 label rows do not care; the compressed table
                # holds counts of ONE denominator: on a second one the rows stored so far go back to fp32 (one pass) and the build
                # goes on as the reference's does
                logger.warning("training batches of a second input size (patch %d x %d after label denominator %d): the label "
                               "table continues as fp32 rows", patch_size, patch_size, self.index.label_denominator)
                self.index.labels_to_fp32()
                self._mixed_patch_sizes = True
            # K2: `y[y == 255] = 0` (310) + patchify (317) + one-hot mean (319-320)
            label = ops.patch_label_hist(y, patch_size, num_classes, map255=True)   # [bs,S,S,C]
            if self.memory_size is None:
                if not presized and total_flat is not None:
                    # the unbounded bank's size is known up front (batches x images x patches; a short last
                    # batch only over-reserves): one allocation instead of geometric growth copies
                    own_batches = (min(own_hi, total_flat) - own_lo) if self.sharded else total_flat
                    self.index.reserve(max(1, int(own_batches) * bs * S * S))
                    presized = True
                feats = self._tokens(x)                            # [bs, S*S, D] on the GPU
                self.index.use_current_stream()
                self.index.add(feats.reshape(-1, feats.shape[-1]), normalize=True)   # K1 (324-329)
                self.index.add_labels(label.reshape(-1, num_classes))
                self._record_blocks(feats.shape[0], feats.shape[1])
            else:
                K = int(self.num_sampled_features)
                lab = label.reshape(bs, S * S, num_classes)
                scores, nonempty, nz = ops.patch_scores(lab)       # K3a (471-493)
                nz_host = nz.cpu().tolist()                        # 497 (.tolist() sync in the reference too)
                total_nz = sum(nz_host)
                # the CPU generator is consumed for EVERY batch, in loader order, so that all ranks
                # stay aligned with the single-process stream of the reference (500)
                r = torch.rand(total_nz) if total_nz > 0 else torch.zeros(0)
                if not mine:
                    continue
                r_off = torch.tensor([0] + nz_host[:-1], dtype=torch.int64).cumsum(0)
                sidx = ops.patch_select(scores, nonempty, r.to(self.gpu_device), r_off.to(self.gpu_device), K)
                feats = self._tokens(x)
                D = feats.shape[-1]
                rows = (sidx + torch.arange(bs, device=sidx.device)[:, None] * (S * S)).reshape(-1)
                sampled = ops.gather_rows(feats.reshape(-1, D), rows)                  # 515
                self.index.use_current_stream()
                self.index.add(sampled, normalize=True)                                # 335, 352-353
                self.index.add_labels(ops.gather_rows(lab.reshape(-1, num_classes), rows))   # 344-354
                self._record_blocks(bs, K)
        state["presized"] = presized

    def _record_blocks(self, images: int, rows_each: int) -> None:
        """Build geometry: `images` more (epoch, image) blocks of `rows_each` rows were appended (S x S unbounded, K bounded)."""
        last = self._bank_block_starts[-1]
        self._bank_block_starts.extend(last + rows_each * (i + 1) for i in range(images))

    def _set_label_denominator(self, P: int) -> None:
        """Every soft label is j / P, P = patch_size ** 2 (the mean of a one-hot over a patch's P pixels, hbird_eval.py:319-320): the
        index keeps the uint16 count j instead of the fp32 value -- half the label table (6.2 -> 3.1 GB at cfg-3, per rank when it is
        replicated) and half K5's gather traffic, the same fp32 values back.  nn_params["compress_labels"] = False keeps fp32."""
        if self.compress_labels and 0 < int(P) <= 32767 and self.index.ntotal == 0 and self.index.label_denominator != int(P):
            self.index.set_label_denominator(int(P))

    @staticmethod
    def _infer_label_denominator(lm: torch.Tensor) -> int:
        """P of a stored label_memory (rows of j / P summing to 1), or 0: the smallest positive value of a sample suggests 1 / P, the whole
        tensor is then checked exactly (chunked) -- a table that is not of that form stays fp32."""
        if lm.numel() == 0:
            return 0
        head = lm[:4096].float()
        pos = head[head > 0]
        if pos.numel() == 0:
            return 0
        P = int(round(1.0 / float(pos.min())))
        if not 0 < P <= 32767:
            return 0
        for lo in range(0, lm.shape[0], 1 << 18):
            v = lm[lo:lo + (1 << 18)].float()
            Pt = torch.tensor(float(P))
            c = torch.round(v * Pt)
            if not bool(((c / Pt) == v).all()) or bool((c < 0).any()) or bool((c > P).any()):
                return 0
        return P

    def _tokens(self, x: torch.Tensor) -> torch.Tensor:
        feats, _ = self.feature_extractor.forward_features(x.to(self.device))    # (BS, N, D)
        return feats.to(self.gpu_device, dtype=torch.float32).contiguous()

    def _finalize_shards(self) -> None:
        """Sharded mode: learn every rank's row range and replicate the (small) label / norm tables."""
        n_local = self.index.ntotal
        if not self.sharded:
            self.total_rows = n_local
            return
        counts = torch.zeros(self.world, dtype=torch.int64, device=self.gpu_device)
        counts[self.rank] = n_local
        torch.distributed.all_reduce(counts)
        counts = counts.cpu().tolist()
        self.id_base = sum(counts[:self.rank])
        self.total_rows = sum(counts)
        self.index.use_current_stream()
        nrm_all, _ = hdist.allgather_rows(self.index.copy_norms())
        norms = torch.cat([nrm_all[r, :counts[r]] for r in range(self.world)]).contiguous()
        if self.label_shard:
            self._label_table = (None, norms)          # label rows stay with their owners
            return
        # every rank agrees on the storage form (an empty shard never saw a batch: it takes the others' denominator)
        # (ranks WITH rows that disagree -- one on fp32, one on counts, or two denominators -- fall back to fp32 rows together: a MAX alone
        # would send the fp32 rank into copy_label_counts, which fails there while its peers wait in the all-gather)
        own_P = self.index.label_denominator
        pden = torch.tensor([own_P, -own_P if n_local else -(1 << 40)], dtype=torch.int64, device=self.gpu_device)
        torch.distributed.all_reduce(pden, op=torch.distributed.ReduceOp.MAX)
        p_max, p_min = int(pden[0].item()), -int(pden[1].item())
        P = p_max if (p_min == p_max or p_min == (1 << 40)) else 0
        if P == 0 and p_max > 0:
            logger.warning("ranks disagree on the label denominator (%d .. %d): the replicated label table stays fp32", p_min, p_max)
        if P > 0:      # the replicated table travels and stays as uint16 counts: half the bytes on the wire and per rank
            if n_local == 0 and self.index.label_denominator != P:
                self.index.set_label_denominator(P)
            cnt_local = (self.index.copy_label_counts() if n_local
                         else torch.zeros((0, self.num_classes), dtype=torch.int16, device=self.gpu_device))
            cnt_all, _ = hdist.allgather_rows(cnt_local.contiguous().view(torch.uint8))      # bytes: gloo has no int16 collectives
            counts_tab = torch.cat([cnt_all[r, :counts[r]] for r in range(self.world)]).contiguous().view(torch.int16)
            self._label_table = (counts_tab, norms)
            self._label_table_P = P
            self.index.set_label_count_table(counts_tab, norms, P, 0)
            return
        lab_local = (self.index.gather_labels(torch.arange(n_local, device=self.gpu_device)) if n_local
                     else torch.zeros((0, self.num_classes), device=self.gpu_device))
        lab_all, _ = hdist.allgather_rows(lab_local)
        labels = torch.cat([lab_all[r, :counts[r]] for r in range(self.world)]).contiguous()
        self._label_table = (labels, norms)
        self._label_table_P = 0
        self.index.set_label_table(labels, norms, 0)

    # ------------------------------------------------------------------------------------------------
    # bank persistence (reference 371-400): same two-tensor torch.save format
    # ------------------------------------------------------------------------------------------------
    @property
    def feature_memory(self) -> torch.Tensor:
        """This rank's bank rows as a CPU tensor [M_local, D] (the reference keeps it on the CPU, 178)."""
        n = self.index.ntotal
        if n == 0:
            return torch.zeros((0, self.index.d))
        ids = torch.arange(n, device=self.gpu_device)
        return self.index.reconstruct(ids).cpu()

    @property
    def label_memory(self) -> torch.Tensor:
        n = self.index.ntotal
        if n == 0:
            return torch.zeros((0, self.num_classes))
        return self.index.gather_labels(torch.arange(n, device=self.gpu_device)).cpu()

    def _gather_to_rank0(self, local: torch.Tensor) -> Optional[torch.Tensor]:
        """Sharded mode: the shards' rows [M_r, W] (CPU) concatenated in rank order on rank 0 (None elsewhere).  Rows
        travel GPU to GPU in chunks (send / recv work on both RCCL and gloo), so no rank stages more than a chunk."""
        td = torch.distributed
        counts = torch.zeros(self.world, dtype=torch.int64, device=self.gpu_device)
        counts[self.rank] = local.shape[0]
        td.all_reduce(counts)
        counts = counts.cpu().tolist()
        width = local.shape[1]
        chunk = max(1, (256 << 20) // (4 * max(1, width)))
        if self.rank == 0:
            out = torch.empty((sum(counts), width), dtype=torch.float32)
            out[:counts[0]] = local
            base = counts[0]
            for r in range(1, self.world):
                for lo in range(0, counts[r], chunk):
                    n = min(chunk, counts[r] - lo)
                    buf = torch.empty((n, width), dtype=torch.float32, device=self.gpu_device)
                    td.recv(buf, src=r)
                    out[base + lo: base + lo + n] = buf.cpu()
                base += counts[r]
            return out
        for lo in range(0, counts[self.rank], chunk):
            td.send(local[lo: lo + chunk].to(self.gpu_device).contiguous(), dst=0)
        return None

    def _save_memory(self) -> None:
        """`torch.save` of the two plain tensors, as the reference (hbird_eval.py:371-380).  Also under a row-sharded
        bank the files hold the WHOLE bank in the reference's row order (rank 0 writes them), so a bank saved by N
        ranks loads into one process, into the reference, or into any other number of ranks."""
        for path, name in ((self.f_mem_p, "feature"), (self.l_mem_p, "label")):
            if path is None:
                continue
            t = self.feature_memory if name == "feature" else self.label_memory
            if self.sharded:
                t = self._gather_to_rank0(t)
            if t is not None:
                torch.save(t, path)
                logger.info("Saved %s memory to: %s", name, path)
        if self.sharded and (self.f_mem_p is not None or self.l_mem_p is not None):
            torch.distributed.barrier()

    def _memory_files_exist(self) -> bool:
        return (self.f_mem_p is not None and self.l_mem_p is not None and os.path.isfile(self.f_mem_p)
                and os.path.isfile(self.l_mem_p))

    def _reusable_memory(self) -> bool:
        """May the file pair f_mem_p / l_mem_p stand in for a bank build?  (The reference always rebuilds and overwrites, hbird_eval.py:175;
        re-use is this engine's addition.)  The files must exist AND fit this run -- feature width, class count, equal row counts, and with
        memory_size set no more rows than it allows -- otherwise the bank is rebuilt with a warning.  Under torch.distributed RANK 0 decides
        and broadcasts: ranks that looked for themselves could disagree (a file system that is not shared, a half-written file) and would
        then meet in different collectives -- load_memory's and _create_memory's -- and hang."""
        ok = 0
        if self.rank == 0:
            ok = 1 if self._memory_files_exist() else 0
            if ok:
                try:
                    fm = torch.load(self.f_mem_p, mmap=True); lm = torch.load(self.l_mem_p, mmap=True)
                    why = None
                    if fm.dim() != 2 or lm.dim() != 2 or fm.shape[0] != lm.shape[0]:
                        why = f"shapes {tuple(fm.shape)} / {tuple(lm.shape)} are not [M, D] / [M, C]"
                    elif fm.shape[1] != self.feature_extractor.d_model:
                        why = f"feature width {fm.shape[1]} != the extractor's {self.feature_extractor.d_model}"
                    elif lm.shape[1] != self.num_classes:
                        why = f"{lm.shape[1]} label columns != num_classes {self.num_classes}"
                    elif self.memory_size is not None and fm.shape[0] > self.memory_size:
                        why = f"{fm.shape[0]} rows > memory_size {self.memory_size}"
                    if why is not None:
                        logger.warning("saved bank %s / %s does not fit this run (%s): rebuilding", self.f_mem_p, self.l_mem_p, why)
                        ok = 0
                except Exception as e:          # noqa: BLE001 -- an unreadable file is a reason to rebuild, not to fail
                    logger.warning("saved bank %s / %s cannot be read (%r): rebuilding", self.f_mem_p, self.l_mem_p, e)
                    ok = 0
        if self.world > 1:
            t = torch.tensor([ok], device=self.gpu_device)
            torch.distributed.broadcast(t, 0)
            ok = int(t.item())
            if ok and not self._memory_files_exist():
                raise RuntimeError(f"rank 0 decided to re-use the saved bank {self.f_mem_p} / {self.l_mem_p}, which rank {self.rank} cannot see: "
                                   "the bank files must be on a file system all ranks share")
        return bool(ok)

    def load_memory(self) -> bool:
        """Load a bank saved by `_save_memory` (or by the reference) and rebuild the index from it; under a
        row-sharded bank every rank takes its contiguous row range of the one file."""
        if self._memory_files_exist():
            fm = torch.load(self.f_mem_p, mmap=True)
            lm = torch.load(self.l_mem_p, mmap=True)
            lo, hi = hdist.shard_range(fm.shape[0], self.rank, self.world) if self.sharded else (0, fm.shape[0])
            with torch.cuda.device(self.gpu_device):
                self.index.reset()
                P = self._infer_label_denominator(lm) if self.compress_labels else 0
                if P != self.index.label_denominator:
                    self.index.set_label_denominator(P)
                self.index.reserve(max(1, hi - lo))
                self.index.add(fm[lo:hi].to(self.gpu_device), normalize=False)
                self.index.add_labels(lm[lo:hi].to(self.gpu_device))
                self._finalize_shards()
            logger.info("Loaded memory from disk.")
            return True
        for p in (self.f_mem_p, self.l_mem_p):
            if p is not None and os.path.isfile(p + ".rank0"):
                logger.warning("%s.rankN: per-rank bank files of an earlier version are no longer read -- a sharded bank is "
                               "saved as ONE reference-format file pair now (INTEGRATION.md); rebuilding", p)
        logger.warning("Memory files not found or paths not provided; skipping load.")
        return False

    # ------------------------------------------------------------------------------------------------
    # sub-bank views: the bank of a smaller memory size / of an image subset out of this one, without a ViT pass (hbird_mi/views.py)
    # ------------------------------------------------------------------------------------------------
    def _view_geometry(self, memory_size, images, rows_per_image):
        """(row ids, block starts, images per epoch, rows per image or None, dataset_size) of the view `memory_size=` / `images=` select out
        of this bank's (epoch, image) blocks; ValueError where the bank has no such view."""
        n_total = self.index.ntotal
        aug = max(1, int(self.augmentation_epoch))
        starts = self._bank_block_starts
        bounded = self.memory_size is not None and self.num_sampled_features is not None
        built_k = int(self.num_sampled_features) if bounded else None
        if rows_per_image is not None:
            rpi = int(rows_per_image)
            if rpi < 1 or n_total % rpi != 0 or (n_total // rpi) % aug != 0:
                raise ValueError(f"memory_view: {n_total} rows are not {aug} epoch(s) of whole images of rows_per_image={rows_per_image} rows")
            starts = list(range(0, n_total + 1, rpi))
            built_k = rpi if self.memory_size is not None else None
        if starts is None:
            raise ValueError("memory_view: this bank was not built here (loaded, or from_index): it has no geometry -- pass rows_per_image= or rows=")
        n_images = (len(starts) - 1) // aug
        blocks, dataset_size = None, self._dataset_size
        if images is not None:
            img = [int(i) for i in (images.tolist() if isinstance(images, torch.Tensor) else images)]
            if any(i < 0 or i >= n_images for i in img):
                raise ValueError(f"memory_view: an image index lies outside [0, {n_images})")
            blocks = [ep * n_images + i for ep in range(aug) for i in img]
            n_images = dataset_size = len(img)
        per_block = None
        if memory_size is not None:
            if built_k is None:
                raise ValueError("memory_view: memory_size= needs a bank built bounded (with memory_size set): a bounded bank keeps the patches "
                                 "with the smallest noisy scores of every image -- out of an unbounded bank it would have been SAMPLED, not truncated")
            per_block = views.per_image_rows(int(memory_size), dataset_size if dataset_size is not None else n_images, aug)
            if per_block > built_k:
                raise ValueError(f"memory_view: memory_size={memory_size} keeps {per_block} rows per image, the bank was built with {built_k}")
        ids = views.view_rows(starts, per_block=per_block, blocks=blocks)      # (a block listed twice: ValueError)
        st = torch.as_tensor(starts, dtype=torch.int64)
        lens = st[1:] - st[:-1]
        if blocks is not None:
            lens = lens[torch.as_tensor(sorted(blocks), dtype=torch.int64)]
        if per_block is not None:
            lens = lens.clamp(max=per_block)
        return ids, [0] + torch.cumsum(lens, 0).tolist(), n_images, (per_block if per_block is not None else built_k), dataset_size

    def memory_view(self, memory_size: Optional[int] = None, images=None, rows=None, rows_per_image: Optional[int] = None,
                    n_neighbours: Optional[int] = None) -> "HbirdEvaluation":
        """A new evaluator over selected rows of this bank: same extractor, its index is `self.index.select_rows(...)` (a device gather, 1 x the
        view's rows of memory), made the `from_index` way; nn_params' use_fp16 / rerank_copy / fp16_centre carry over.  Not in the reference, whose
        memory-size table and data-efficiency file sets cost one bank build per point.

        `rows=`            any row list; works on every single-index evaluator; the view has no geometry.
        `memory_size=`     only on a bank built BOUNDED: the bounded build keeps per (epoch, image) the K patches with the smallest noisy scores in
                           ascending order (hbird_eval.py:146-147, 497-511) and the noise does not depend on K, so the bank of a smaller
                           memory_size is the first K_m rows of every block -- bit for bit what a build from scratch gives.  K_m =
                           views.per_image_rows(memory_size, dataset_size, augmentation_epoch); ValueError when it exceeds the built K.  An
                           UNBOUNDED bank has no such prefix: a bounded bank of it would have been sampled, not truncated -- ValueError.
        `images=`          image indices in loader order, taken in every epoch (the view keeps the build's row order).  Combined with
                           `memory_size=` the per-image ROW COUNT follows the subset (dataset_size = len(images)); the rows are still the ones
                           the full build's noise chose -- a bounded build on the subset alone draws other noise and samples other patches.
        `rows_per_image=`  the geometry of a loaded or `from_index` bank (equal blocks; the row count must divide evenly).
        The view gets a geometry of its own, so views of views work.  ValueError under torch.distributed and with several GPUs in one process."""
        if self.world > 1 or self.sharded or len(self.local_gpus) > 1 or not isinstance(self.index, HipFlatIndex):
            raise ValueError("memory_view: views are single-index -- not available under torch.distributed or with several GPUs in one process")
        starts_new = images_new = k_new = dataset_size_new = None
        if rows is not None:
            if memory_size is not None or images is not None or rows_per_image is not None:
                raise ValueError("memory_view: rows= stands alone (no memory_size / images / rows_per_image beside it)")
            ids = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(list(rows), dtype=torch.int64)
        elif memory_size is None and images is None:
            raise ValueError("memory_view: one of memory_size=, images= or rows= is needed")
        else:
            ids, starts_new, images_new, k_new, dataset_size_new = self._view_geometry(memory_size, images, rows_per_image)
        with torch.cuda.device(self.gpu_device):
            self.index.use_current_stream()
            try:
                self._groups_to_index()            # the view's rows keep their images (leave-one-out): select_rows hands groups[ids] over
                carried = self.row_groups()
            except ValueError:
                carried = None                     # (no geometry and no table given: the view has none either)
            index = self.index.select_rows(ids)
            index.use_current_stream()
        view = HbirdEvaluation.from_index(self.feature_extractor, index, self.num_classes,
                                          n_neighbours=self.n_neighbours if n_neighbours is None else n_neighbours, device=self.device,
                                          beta=self.beta)
        view.nn_method = self.nn_method
        view.nn_params = {k: self.nn_params[k] for k in ("distance_measure", "use_fp16", "rerank_copy", "fp16_centre", "exclude_screen") if k in self.nn_params}
        if view.nn_params.get("use_fp16", False):
            index.set_fp16(2)
            index.set_rerank_copy(int(view.nn_params.get("rerank_copy", 0)))
        if view.nn_params.get("fp16_centre", False):
            index.set_fp16_centre(True)
        if view.nn_params.get("exclude_screen", False):
            index.set_exclusion_screen(True)
        view.augmentation_epoch = self.augmentation_epoch
        view.compress_labels = self.compress_labels
        view.memory_size = memory_size if memory_size is not None else self.memory_size
        view.num_sampled_features = k_new
        view._bank_block_starts, view._dataset_images = starts_new, images_new
        view._dataset_size = dataset_size_new
        view.bank_loaded = False
        if carried is not None:
            view._row_groups = carried[torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu()]
            view._row_groups_on_index = index.row_groups is not None
            view._loo_images = self._leave_one_out_images()
        return view

    # ------------------------------------------------------------------------------------------------
    # leave-one-image-out: the bank evaluated on its own training images, every query excluding the rows of the image it came from
    # (HipFlatIndex.search_excluding, csrc/hbird_exclude.hip; DESIGN.md section 4, "Leave-one-image-out searches")
    # ------------------------------------------------------------------------------------------------
    def set_row_groups(self, groups) -> None:
        """The dataset image of every bank row, given by the caller (int tensor [ntotal], -1 = no image): for a loaded or `from_index` bank,
        which has no build geometry to derive it from."""
        g = torch.as_tensor(groups).detach().reshape(-1).cpu()
        if g.numel() and (g.dtype.is_floating_point or g.dtype == torch.bool):
            raise ValueError(f"set_row_groups: groups must be integers, got {g.dtype}")
        if g.numel() != self.index.ntotal:
            raise ValueError(f"set_row_groups: {g.numel()} groups for a bank of {self.index.ntotal} rows")
        self._row_groups, self._row_groups_on_index = g.to(torch.int32), False
        self._loo_images = None

    def row_groups(self) -> torch.Tensor:
        """int32 [ntotal] (CPU): the dataset image of every bank row.  Bank blocks are appended in (epoch, image) order, block b belongs to
        image b % images -- with augmentation_epoch > 1 an image's rows are not one range.  ValueError on a loaded or `from_index` bank
        (no build geometry) unless `set_row_groups` gave the table; a `memory_view` carries its rows' images."""
        given = getattr(self, "_row_groups", None)
        if given is not None:
            return given
        starts, n_img = self._bank_block_starts, self._dataset_images
        if starts is None or not n_img:
            raise ValueError("row_groups: this bank was not built here (loaded, or from_index): it has no geometry -- call set_row_groups(tensor)")
        st = torch.as_tensor(starts, dtype=torch.int64)
        g = torch.repeat_interleave(torch.arange(st.numel() - 1, dtype=torch.int64) % int(n_img), st[1:] - st[:-1]).to(torch.int32)
        if g.numel() != self.index.ntotal:
            raise ValueError(f"row_groups: the build geometry covers {g.numel()} rows, the bank holds {self.index.ntotal}")
        return g

    def _leave_one_out_images(self) -> int:
        """How many images a leave-one-out pass may see: the images of the build (a view: of the bank it was cut from)."""
        n = getattr(self, "_loo_images", None)
        if n is None:
            g = self.row_groups()             # (ValueError: a bank without geometry and without a given table)
            n = self._dataset_images if getattr(self, "_row_groups", None) is None else int(g.max().item()) + 1 if g.numel() else 0
        return int(n)

    def _groups_to_index(self) -> None:
        """The row-group table onto the index (once; again after set_row_groups or when the bank has grown)."""
        if self.world > 1 or self.sharded or len(self.local_gpus) > 1 or not isinstance(self.index, HipFlatIndex):
            raise ValueError("leave-one-out searches are single-index -- not available under torch.distributed or with several GPUs in one process")
        g = self.row_groups()
        have = self.index.row_groups
        if have is None or have.numel() != g.numel() or not getattr(self, "_row_groups_on_index", False):
            self.index.set_row_groups(g, max(self._leave_one_out_images(), int(g.max().item()) + 1 if g.numel() else 0))
            self._row_groups_on_index = True

    def evaluate_leave_one_out(self, loader, eval_spatial_resolution: int, n_neighbours=None, betas=None, views=None, ignore_index: int = 255,
                               max_images: Optional[int] = None, window=None, screen: Optional[bool] = None, bootstrap=None):
        """`evaluate_grid` of the bank ON ITS OWN TRAINING IMAGES: `loader` yields the bank's images in the order of the build pass (the
        project's data modules do: shuffle=False), the i-th image seen queries with group i, and every search excludes the bank rows of the
        query's own image (`search_aggregate_grid_excluding`) -- so (k, beta, memory size) can be chosen without touching the validation split.
        Not in the reference.  One pass, one excluding search per batch and bank; every configuration's mIoU is what `evaluate_grid` gives when,
        image by image, the bank is replaced by its `memory_view(rows=all rows but that image's)`.
        `views={key: HbirdEvaluation}`: the `memory_view`s of this bank (they carry their rows' images).  `max_images`: stop after that many
        images (the cost control).  -> {(k, beta): mIoU}, with `views` {(key, k, beta): mIoU}.
        `screen`: True / False switches excluding searches on the certified fp16 screen (`HipFlatIndex.set_exclusion_screen`) on / off on every
        bank of the pass, None leaves the indexes as they are; same floats either way.  `self.loo_screen_served` counts the pass's searches
        (batch x bank) that the screen served.
        `bootstrap=R` or `(R, seed)`: as for `evaluate_grid` -- a `MiouBootstrap` over the images seen instead of the dict.
        ValueError when more images arrive than the bank was built from, for a bank without geometry (`row_groups`), under torch.distributed,
        with a multi-GPU index and with `window=`."""
        from hbird_mi.nn.search_hip import grid_plan
        if window is not None:
            raise ValueError("evaluate_leave_one_out: sliding windows (window=) are not supported")
        if max_images is not None and int(max_images) < 1:
            raise ValueError("evaluate_leave_one_out: max_images must be positive")
        banks = {None: self} if views is None else dict(views)
        if not banks:
            raise ValueError("evaluate_leave_one_out: views is empty")
        for key, ev in list(banks.items()) + [(None, self)]:
            if not isinstance(ev, HbirdEvaluation):
                raise ValueError(f"evaluate_leave_one_out: views[{key!r}] is not an HbirdEvaluation")
            if ev.world > 1 or ev.sharded or len(ev.local_gpus) > 1 or not isinstance(ev.index, HipFlatIndex):
                raise ValueError("evaluate_leave_one_out: excluding searches are single-index -- not available under torch.distributed or with "
                                 "several GPUs in one process")
            if ev.num_classes != self.num_classes or ev.gpu_device != self.gpu_device:
                raise ValueError(f"evaluate_leave_one_out: views[{key!r}] differs from this evaluator in class count or device")
        n_images = self._leave_one_out_images()
        for ev in banks.values():
            with torch.cuda.device(self.gpu_device):
                ev.index.use_current_stream()
                ev._groups_to_index()
                if screen is not None:
                    ev.index.set_exclusion_screen(bool(screen))
        self.loo_screen_served = 0
        plan = grid_plan(self.n_neighbours if n_neighbours is None else n_neighbours, self.beta if betas is None else betas)
        metrics = {key: [PredsmIoU(self.num_classes, self.num_classes, ignore_index=ignore_index, device=self.gpu_device,
                                   store_reordered_preds=False) for _ in plan.configs] for key in banks}
        boot = hboot.parse_bootstrap(bootstrap)
        collector = None if boot is None else hboot.ImageCountCollector(self.num_classes, len(banks) * len(plan.configs), ignore_index,
                                                                        self.gpu_device, capacity=n_images if max_images is None else min(n_images, int(max_images)))
        self.feature_extractor = self.feature_extractor.to(self.device)
        S = eval_spatial_resolution
        limit = n_images if max_images is None else min(n_images, int(max_images))
        seen = 0
        logger.info("Starting leave-one-out loop: %d configurations, %d bank(s), %d image(s)...", len(plan.configs), len(banks), limit)
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for bi, (x, y) in tqdm(self._prefetched(enumerate(loader), True), desc="Leave-one-out loop"):
                if max_images is not None and seen >= limit:
                    break
                if max_images is not None and seen + x.shape[0] > limit:
                    x, y = x[:limit - seen], y[:limit - seen]
                if seen + x.shape[0] > n_images:
                    raise ValueError(f"evaluate_leave_one_out: the loader yields more than the {n_images} images the bank was built from "
                                     "(it must yield the bank's images, in the order of the build pass)")
                y = (y.to(self.gpu_device) * 255).long()
                feats = self._tokens(x)
                B, N, D = feats.shape
                q = feats.reshape(B * N, D).contiguous()
                qgroups = torch.arange(seen, seen + B, dtype=torch.int32, device=q.device).repeat_interleave(N)
                seen += B
                for bank_i, (key, ev) in enumerate(banks.items()):
                    ev.index.use_current_stream()
                    lh = ev.index.search_aggregate_grid_excluding(q, plan.ks, plan.betas, qgroups, id_base=0)
                    self.loo_screen_served += ev.index.last_exclusion_screen()["served"]
                    for i, m in enumerate(metrics[key]):
                        self._count_batch(m, collector, bank_i * len(plan.configs) + i, y, lh[i].view(B, N, -1), S)
        if collector is not None:
            logger.info("Leave-one-out evaluation complete (%d images); bootstrapping.", seen)
            return self._finish_bootstrap(banks, plan, metrics, collector, boot, views is None)
        out = {}
        for key in banks:
            for (k, beta), m in zip(plan.configs, metrics[key]):
                jac = m.compute(is_global_zero=True, sync_distributed=False, return_reordered=False)[0]
                out[(k, beta) if views is None else (key, k, beta)] = jac
        logger.info("Leave-one-out evaluation complete (%d images).", seen)
        return out

    # ------------------------------------------------------------------------------------------------
    # query path (reference evaluate 184-265, _find_nearest_key_to_query 611-637, _cross_attention 575-609)
    # ------------------------------------------------------------------------------------------------
    def find_neighbours(self, q_flat: torch.Tensor, k: Optional[int] = None):
        """q_flat [nq, D] on the GPU -> (idx int64 [nq,k] global ids, dist [nq,k]); un-normalised queries (625)."""
        k = self.n_neighbours if k is None else k
        self.index.use_current_stream()
        if not self.sharded:
            return self.index.search(q_flat, k, id_base=self.id_base)
        return hdist.sharded_search(self.index.search_scores, merge_topk, q_flat, k, self.id_base, self.metric,
                                    finish=self.index.distances_from_scores, merge_packed=merge_topk_packed)

    def _label_hat(self, feats: torch.Tensor, want_details: bool):
        """feats [B,N,D] -> label_hat [B,N,C] (+ neighbours when details are requested)."""
        B, N, D = feats.shape
        q = feats.reshape(B * N, D).contiguous()
        k = self.n_neighbours
        self.index.use_current_stream()
        if not self.sharded and not want_details:
            lh = k5(self.index, "search_aggregate", k)(q, k, beta=self.beta, id_base=0)
            return lh.view(B, N, -1), None, None
        idx, dist = self.find_neighbours(q, k)
        lh = k5(self.index, "aggregate", k)(q, idx, dist, beta=self.beta, id_base=self.id_base)
        return lh.view(B, N, -1), idx, dist

    def _replicated_label_rows(self, ids: torch.Tensor) -> torch.Tensor:
        """label_memory.index_select(0, ids) (hbird_eval.py:633) on the table replicated over the ranks; ids outside it give zeros."""
        tab = self._label_table[0]
        if getattr(self, "_label_table_P", 0):      # uint16 counts -> the fp32 values (a float32 division: K2's own quotient)
            ok = (ids >= 0) & (ids < tab.shape[0])
            # (tensor divisor: a Python-scalar divisor becomes a multiplication by the reciprocal on the GPU -- another rounding)
            out = tab[ids.clamp(0, max(0, tab.shape[0] - 1))].to(torch.float32) / torch.tensor(float(self._label_table_P), device=tab.device)
            out[~ok] = 0.0
            return out
        return ops.gather_rows(tab, ids)

    def _gather_details(self, idx: torch.Tensor, B: int, N: int):
        k = idx.shape[1]
        flat = idx.reshape(-1)
        if self.sharded:
            # rows live on their owners: every rank reconstructs its own rows, the sum fills the rest
            own = (flat >= self.id_base) & (flat < self.id_base + self.index.ntotal)
            kf = self.index.reconstruct(torch.where(own, flat, torch.full_like(flat, -1)), id_base=self.id_base)
            torch.distributed.all_reduce(kf)
            kl = self._replicated_label_rows(flat)
        else:
            kf = self.index.reconstruct(flat)
            kl = self.index.gather_labels(flat)
        return kf.view(B, N, k, -1), kl.view(B, N, k, -1)

    def evaluate(self, val_loader, eval_spatial_resolution: int, return_knn_details: bool = False,
                 ignore_index: int = 255, window: Optional[Tuple[int, int]] = None):
        """Reference evaluate (hbird_eval.py:205-263).  `window=(win, stride)` (not in the reference): the loader
        yields frames larger than the extractor's input; every win x win window goes through the hot path and the
        windows' upsampled soft predictions are summed on the device before the argmax (hbird_mi/tiling.py)."""
        if window is not None and return_knn_details:
            raise ValueError("return_knn_details is not available with sliding windows")
        metric = PredsmIoU(self.num_classes, self.num_classes, ignore_index=ignore_index, device=self.gpu_device,
                           store_reordered_preds=False)
        self.feature_extractor = self.feature_extractor.to(self.device)
        S = eval_spatial_resolution
        knns, knns_labels, knns_ca_labels = [], [], []
        logger.info("Starting evaluation loop...")
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            if self.sharded:
                self._evaluate_sharded(val_loader, S, metric, return_knn_details, knns, knns_labels, knns_ca_labels,
                                       window)
            else:
                # replica mode (idx_shard=False) under torch.distributed: validation batches are data-parallel, and a rank loads only its own
                batches = (enumerate(val_loader) if self.world == 1
                           else hdist.rank_batches(val_loader, lambda i: i % self.world == self.rank))
                # the NEXT batch is fetched from the loader and copied to the GPU (side stream) while this one is searched; with
                # `self.profile = True` every batch's stages are timed by events (stage_times() afterwards; bench.py --e2e)
                prof = self._stage_profile = [] if getattr(self, "profile", False) else None
                for bi, (x, y) in tqdm(self._prefetched(batches, window is None), desc="Evaluation loop"):
                    _, _, h, w = x.shape
                    ev = self._mark(prof)                                           # batch on the GPU
                    y = (y.to(self.gpu_device) * 255).long()                       # 219 (255 is NOT remapped here)
                    if window is not None:
                        metric.update(y, self._windowed_cluster_map(x, S, window))
                        continue
                    feats = self._tokens(x)                                       # 217 (stays on the GPU)
                    self._mark(prof, ev)                                            # ViT forward
                    label_hat, idx, _ = self._label_hat(feats, return_knn_details)  # 224-227
                    self._mark(prof, ev)                                            # K4 + K5
                    if return_knn_details:
                        kf, kl = self._gather_details(idx, feats.shape[0], feats.shape[1])
                        knns.append(kf.cpu()); knns_labels.append(kl.cpu()); knns_ca_labels.append(label_hat.cpu())
                    metric.update_from_label_hat(y, label_hat, S)                   # 235-243 + 252: upsample + argmax + confusion counts, one kernel
                    self._mark(prof, ev)                                            # K6 + K7
        jac, tp, fp, fn, _, _ = metric.compute(is_global_zero=True, sync_distributed=self.world > 1,
                                               return_reordered=False)            # 253
        if return_knn_details:
            details = {"knns": torch.cat(knns), "knns_labels": torch.cat(knns_labels),
                       "knns_ca_labels": torch.cat(knns_ca_labels)}
            logger.info("Evaluation complete (with KNN details).")
            return jac, details
        logger.info("Evaluation complete.")
        return jac

    def evaluate_grid(self, val_loader, eval_spatial_resolution: int, n_neighbours=None, betas=None, views=None, ignore_index: int = 255,
                      window=None, return_knn_details: bool = False, bootstrap=None):
        """`evaluate` for every (k, beta) of a grid out of ONE pass over the loader (not in the reference, where every value of n_neighbours
        or of the temperature costs a full evaluation).  Per batch the tokens are computed once and every bank is searched ONCE, at the largest
        k: the engine's lists are the exact top-k under one total order with deterministic score bits, so the best k are the first k entries
        of the best k_max and beta only enters after the search (`search_aggregate_grid`; DESIGN.md section 4, "Evaluation grids").  Every
        configuration has its own metric object; its mIoU is what a separate `HbirdEvaluation(n_neighbours=k, beta=beta).evaluate(...)` returns.

        `n_neighbours`, `betas`: a value or a list each (duplicates dropped, sorted); default: the evaluator's own n_neighbours / beta.
        `views={key: HbirdEvaluation}`: the banks to evaluate -- evaluators that share this one's extractor, the `memory_view`s of one bank
        (this evaluator itself may be among them); the batch's tokens serve every bank.  Without `views` the bank is this evaluator's.
        -> {(k, beta): mIoU}, with `views` {(key, k, beta): mIoU}.
        `bootstrap=R` or `(R, seed)`: -> a `hbird_mi.bootstrap.MiouBootstrap` with those keys instead -- `.miou` is the dict above, `.samples`
        R paired bootstrap replicates over the images of every configuration's identity-matching mIoU (per-image class counts collected from
        the class maps, resampled on the device; DESIGN.md section 4, "Bootstrap intervals").  None (default): the dict, and the launches, of ever.
        Single index or a HipMultiIndex in one process.  ValueError under torch.distributed, with `window=` and with `return_knn_details`."""
        from hbird_mi.nn.search_hip import grid_plan
        if window is not None:
            raise ValueError("evaluate_grid: sliding windows (window=) are not supported; call evaluate per configuration")
        if return_knn_details:
            raise ValueError("evaluate_grid: return_knn_details is not supported; call evaluate per configuration")
        banks = {None: self} if views is None else dict(views)
        if not banks:
            raise ValueError("evaluate_grid: views is empty")
        for key, ev in banks.items():
            if not isinstance(ev, HbirdEvaluation):
                raise ValueError(f"evaluate_grid: views[{key!r}] is not an HbirdEvaluation")
            if ev.world > 1 or ev.sharded:
                raise ValueError("evaluate_grid: not available under torch.distributed (row shards or replicas): one index, or several GPUs "
                                 "in one process")
            if ev.num_classes != self.num_classes or ev.gpu_device != self.gpu_device:
                raise ValueError(f"evaluate_grid: views[{key!r}] differs from this evaluator in class count or device")
        if self.world > 1 or self.sharded:
            raise ValueError("evaluate_grid: not available under torch.distributed (row shards or replicas): one index, or several GPUs in "
                             "one process")
        plan = grid_plan(self.n_neighbours if n_neighbours is None else n_neighbours, self.beta if betas is None else betas)
        metrics = {key: [PredsmIoU(self.num_classes, self.num_classes, ignore_index=ignore_index, device=self.gpu_device,
                                   store_reordered_preds=False) for _ in plan.configs] for key in banks}
        boot = hboot.parse_bootstrap(bootstrap)
        collector = None if boot is None else hboot.ImageCountCollector.for_loader(val_loader, self.num_classes, len(banks) * len(plan.configs),
                                                                                   ignore_index, self.gpu_device)
        self.feature_extractor = self.feature_extractor.to(self.device)
        S = eval_spatial_resolution
        logger.info("Starting grid evaluation loop: %d configurations, %d bank(s)...", len(plan.configs), len(banks))
        with torch.no_grad(), torch.cuda.device(self.gpu_device):
            for bi, (x, y) in tqdm(self._prefetched(enumerate(val_loader), True), desc="Grid evaluation loop"):
                y = (y.to(self.gpu_device) * 255).long()
                feats = self._tokens(x)
                B, N, D = feats.shape
                q = feats.reshape(B * N, D).contiguous()
                for bank_i, (key, ev) in enumerate(banks.items()):
                    ev.index.use_current_stream()
                    lh = ev.index.search_aggregate_grid(q, plan.ks, plan.betas, id_base=0)        # [configs, B * N, C]: one search
                    for i, m in enumerate(metrics[key]):
                        self._count_batch(m, collector, bank_i * len(plan.configs) + i, y, lh[i].view(B, N, -1), S)
        if collector is not None:
            logger.info("Grid evaluation complete; bootstrapping.")
            return self._finish_bootstrap(banks, plan, metrics, collector, boot, views is None)
        out = {}
        for key in banks:
            for (k, beta), m in zip(plan.configs, metrics[key]):
                jac = m.compute(is_global_zero=True, sync_distributed=False, return_reordered=False)[0]
                out[(k, beta) if views is None else (key, k, beta)] = jac
        logger.info("Grid evaluation complete.")
        return out

    @staticmethod
    def _count_batch(m: PredsmIoU, collector, cfg: int, y: torch.Tensor, label_hat: torch.Tensor, S: int) -> None:
        """One configuration's batch into its metric; with a collector (bootstrap=) the fused kernel also returns the class map, whose
        per-image class counts go into the collector's table.  Without one: `update_from_label_hat`, the launches of ever."""
        if collector is None:
            m.update_from_label_hat(y, label_hat, S)
            return
        pred = ops.upsample_argmax_confusion(label_hat, S, y, m._conf_mat, m.ignore_index, want_map=True)
        collector.add(cfg, y, pred)

    @staticmethod
    def _finish_bootstrap(banks, plan, metrics, collector, boot, plain_keys: bool):
        keys = [(k, beta) if plain_keys else (key, k, beta) for key in banks for (k, beta) in plan.configs]
        return hboot.finish(keys, [m for key in banks for m in metrics[key]], collector, boot[0], boot[1])

    # -- overclustering: k-means over the bank, clusters matched to classes (hbird_mi/kmeans.py) -----------------------------------
    OVERCLUSTERING_MATCHINGS = {"hungarian": dict(many_to_one=False, precision_based=False),
                                "many_to_one": dict(many_to_one=True, precision_based=False),
                                "many_to_one_precision": dict(many_to_one=True, precision_based=True)}

    def _overclustering_checks(self, who: str) -> None:
        if self.world > 1 or self.sharded:
            raise ValueError(f"{who}: not available under torch.distributed (row shards or replicas): k-means runs on one index")
        if not isinstance(self.index, HipFlatIndex):
            raise ValueError(f"{who}: k-means runs on one HipFlatIndex -- a HipMultiIndex (row shards or replicas) is not supported yet")

    def kmeans(self, n_clusters: int, seed: int = 0, max_iter: int = 20):
        """`hbird_mi.kmeans.kmeans_fit` on this evaluator's bank (its stored rows are L2-normalised): a `KMeansResult`."""
        from hbird_mi.kmeans import kmeans_fit
        self._overclustering_checks("kmeans")
        with torch.cuda.device(self.gpu_device):
            return kmeans_fit(self.index, n_clusters, seed=seed, max_iter=max_iter)

    def evaluate_overclustering(self, val_loader, eval_spatial_resolution: int, n_clusters, seed: int = 0, max_iter: int = 20,
                                matching: Optional[str] = None, ignore_index: int = 255, window=None, return_knn_details: bool = False):
        """The overclustering protocol (not in the reference's evaluator, whose `PredsmIoU` carries its matching modes): the bank's tokens are
        clustered with k-means into K clusters, every validation token takes the cluster of its nearest centroid, the cluster map is upsampled
        like a prediction and the clusters are matched to the ground-truth classes.  `n_clusters`: a K or a list (duplicates dropped, sorted);
        one fit per K, then ONE validation pass.  Per batch: tokens -> `ops.normalize_rows` (L2 assignment depends on the norm; the retrieval
        path hands its queries over un-normalised) -> per K `KMeansResult.assign` -> one-hot fp32 [B, N, K] (an id of -1: an all-zero row) ->
        the fused upsample + argmax + confusion kernel into a `PredsmIoU(num_pred_classes=K, num_gt_classes=C)`.
        `matching`: None picks Hungarian matching for K <= C and many-to-one on precision for K > C; "hungarian", "many_to_one" and
        "many_to_one_precision" force one.  -> {K: mIoU}; `last_overclustering[K]` keeps the confusion matrix (int64 [C, K], CPU), the matching
        used and the fit's n_iter / converged / history.  ValueError with sliding windows, with return_knn_details and under torch.distributed."""
        from hbird_mi.kmeans import check_n_clusters
        who = "evaluate_overclustering"
        if window is not None:
            raise ValueError(f"{who}: sliding windows (window=) are not supported")
        if return_knn_details:
            raise ValueError(f"{who}: return_knn_details is not supported (there are no neighbours)")
        self._overclustering_checks(who)
        if matching is not None and matching not in self.OVERCLUSTERING_MATCHINGS:
            raise ValueError(f"{who}: matching={matching!r} (None, {', '.join(repr(m) for m in self.OVERCLUSTERING_MATCHINGS)})")
        ks = [n_clusters] if not isinstance(n_clusters, (list, tuple)) else list(n_clusters)
        if not ks:
            raise ValueError(f"{who}: n_clusters is empty")
        ks = sorted({check_n_clusters(k, self.index.ntotal, who) for k in ks})
        C = self.num_classes
        fits = {}
        try:
            for K in ks:
                fits[K] = self.kmeans(K, seed=seed, max_iter=max_iter)
                logger.info("k-means K=%d: %d iterations, converged=%s", K, fits[K].n_iter, fits[K].converged)
            metrics = {K: PredsmIoU(K, C, ignore_index=ignore_index, device=self.gpu_device, store_reordered_preds=False) for K in ks}
            self.feature_extractor = self.feature_extractor.to(self.device)
            S = eval_spatial_resolution
            with torch.no_grad(), torch.cuda.device(self.gpu_device):
                for bi, (x, y) in tqdm(self._prefetched(enumerate(val_loader), True), desc="Overclustering evaluation loop"):
                    y = (y.to(self.gpu_device) * 255).long()
                    feats = self._tokens(x)
                    B, N, D = feats.shape
                    q = ops.normalize_rows(feats.reshape(B * N, D).contiguous())
                    for K in ks:
                        ids = fits[K].assign(q)
                        one_hot = (ids.view(-1, 1) == torch.arange(K, device=ids.device).view(1, -1)).to(torch.float32)
                        metrics[K].update_from_label_hat(y, one_hot.view(B, N, K), S)        # K6 + K7, num_pred = K
            out, self.last_overclustering = {}, {}
            for K in ks:
                mode = matching if matching is not None else ("hungarian" if K <= C else "many_to_one_precision")
                out[K] = metrics[K].compute(is_global_zero=True, sync_distributed=False, return_reordered=False,
                                            **self.OVERCLUSTERING_MATCHINGS[mode])[0]
                self.last_overclustering[K] = dict(confusion=metrics[K]._conf_mat.cpu(), matching=mode, n_iter=fits[K].n_iter,
                                                   converged=fits[K].converged, history=fits[K].history)
        finally:
            for f in fits.values():
                f.close()
        logger.info("Overclustering evaluation complete.")
        return out

    # -- linear probe: a softmax head fitted on the bank's rows and label rows (hbird_mi/linear_probe.py) ------------------------------
    def _linear_probe_checks(self, who: str) -> None:
        if self.world > 1 or self.sharded:
            raise ValueError(f"{who}: not available under torch.distributed (row shards or replicas): the linear probe runs on one index")
        if not isinstance(self.index, HipFlatIndex):
            raise ValueError(f"{who}: the linear probe runs on one HipFlatIndex -- a HipMultiIndex (row shards or replicas) is not supported yet")

    def linear_probe(self, l2: float = 1e-3, gtol: float = 1e-5, max_iter: int = 200):
        """`hbird_mi.linear_probe.linear_probe_fit` on this evaluator's bank (normalised rows, patch soft labels): a `LinearProbe`."""
        from hbird_mi.linear_probe import linear_probe_fit
        self._linear_probe_checks("linear_probe")
        with torch.cuda.device(self.gpu_device):
            return linear_probe_fit(self.index, l2=l2, gtol=gtol, max_iter=max_iter)

    def evaluate_linear_probe(self, val_loader, eval_spatial_resolution: int, l2: float = 1e-3, gtol: float = 1e-5, max_iter: int = 200,
                              ignore_index: int = 255, window=None, return_knn_details: bool = False) -> float:
        """The linear-head protocol (the third figure this literature reports for a frozen encoder, beside retrieval and overclustering): ONE
        fit of a softmax head on the bank, ONE validation pass.  Per batch: tokens -> `LinearProbe.logits` (normalised like the bank's rows)
        -> [B, N, C] -> the unchanged fused upsample + argmax + confusion kernel (logits may be negative: class 0 starts the running maximum)
        -> `PredsmIoU(C, C)`, scored with `compute(linear_probe=True)`, the identity matching.  -> mIoU; `last_linear_probe` keeps the
        confusion matrix (int64 [C, C], CPU), the fit's state, n_iter, final loss, rows used and skipped, history, and the parameters Wb
        (float32 [C, D + 1], CPU).  ValueError with sliding windows, with return_knn_details and under torch.distributed."""
        who = "evaluate_linear_probe"
        if window is not None:
            raise ValueError(f"{who}: sliding windows (window=) are not supported")
        if return_knn_details:
            raise ValueError(f"{who}: return_knn_details is not supported (there are no neighbours)")
        self._linear_probe_checks(who)
        C = self.num_classes
        probe = self.linear_probe(l2=l2, gtol=gtol, max_iter=max_iter)
        logger.info("linear probe: %d iterations, %s, loss %.6f", probe.n_iter, probe.state, probe.history[-1]["loss"])
        try:
            metric = PredsmIoU(C, C, ignore_index=ignore_index, device=self.gpu_device, store_reordered_preds=False)
            self.feature_extractor = self.feature_extractor.to(self.device)
            S = eval_spatial_resolution
            with torch.no_grad(), torch.cuda.device(self.gpu_device):
                for bi, (x, y) in tqdm(self._prefetched(enumerate(val_loader), True), desc="Linear probe evaluation loop"):
                    y = (y.to(self.gpu_device) * 255).long()
                    metric.update_from_label_hat(y, probe.logits(self._tokens(x)), S)        # K6 + K7
            miou = metric.compute(is_global_zero=True, sync_distributed=False, return_reordered=False, linear_probe=True)[0]
            self.last_linear_probe = dict(confusion=metric._conf_mat.cpu(), state=probe.state, n_iter=probe.n_iter, loss=probe.history[-1]["loss"],
                                          rows_used=probe.rows_used, rows_skipped=probe.rows_skipped, history=probe.history, Wb=probe.Wb.cpu())
        finally:
            probe.close()
        logger.info("Linear probe evaluation complete.")
        return miou

    # -- batch prefetch + stage timing of the evaluation loop ---------------------------------------------------------------------
    def _prefetched(self, batches, to_gpu: bool):
        """(bi, (x, y)) of `batches`, one batch ahead: while the caller works on batch i, batch i + 1 is pulled from the loader (its
        workers decode in the background anyway) and -- `to_gpu` -- copied to the GPU on a side stream from pinned memory, so that neither
        the loader nor PCIe sits between two searches.  The host time spent waiting for the loader is kept in `loader_wait_s`."""
        import time as _time
        self.loader_wait_s = 0.0
        self.h2d_ms = []
        copy = torch.cuda.Stream(self.gpu_device) if to_gpu else None
        main = torch.cuda.current_stream(self.gpu_device)

        def stage(item):
            bi, (x, y) = item
            if copy is None or not isinstance(x, torch.Tensor) or x.is_cuda:
                return bi, x, y, None, None
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(copy):
                e0.record(copy)
                xd = (x if x.is_pinned() else x.pin_memory()).to(self.gpu_device, non_blocking=True)
                yd = (y if y.is_pinned() else y.pin_memory()).to(self.gpu_device, non_blocking=True) if isinstance(y, torch.Tensor) and not y.is_cuda else y
                e1.record(copy)
            return bi, xd, yd, e0, e1

        it = iter(batches)

        def pull():
            t0 = _time.perf_counter()
            try:
                item = next(it)
            except StopIteration:
                item = None
            self.loader_wait_s += _time.perf_counter() - t0
            return None if item is None else stage(item)

        nxt = pull()
        while nxt is not None:
            bi, x, y, e0, e1 = nxt
            if e1 is not None:
                main.wait_event(e1)
                x.record_stream(main)
                if isinstance(y, torch.Tensor) and y.is_cuda:
                    y.record_stream(main)
                self.h2d_ms.append((e0, e1))
            nxt = pull()                    # enqueue the next batch's copy before this one's work is enqueued
            yield bi, (x, y)

    def _mark(self, prof, ev=None):
        """Stage boundary of the profiled evaluation loop: one event on the current stream."""
        if prof is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream(self.gpu_device))
        if ev is None:
            ev = [e]
            prof.append(ev)
        else:
            ev.append(e)
        return ev

    def stage_times(self) -> Optional[Dict[str, float]]:
        """After evaluate() with `self.profile = True`: mean ms per batch of the stages (GPU time between events on the evaluation stream),
        of the prefetched H2D copies (side stream), and the host seconds spent waiting for the loader."""
        prof = getattr(self, "_stage_profile", None)
        if not prof:
            return None
        torch.cuda.synchronize(self.gpu_device)
        rows = [[ev[i].elapsed_time(ev[i + 1]) for i in range(3)] for ev in prof if len(ev) == 4]
        if not rows:
            return None
        n = len(rows)
        out = {"batches": n, "vit_forward_ms": sum(r[0] for r in rows) / n, "knn_k5_ms": sum(r[1] for r in rows) / n,
               "k6_k7_ms": sum(r[2] for r in rows) / n, "loader_wait_s_total": self.loader_wait_s}
        if self.h2d_ms:
            out["h2d_ms"] = sum(a.elapsed_time(b) for a, b in self.h2d_ms) / len(self.h2d_ms)
        return out

    def _windowed_cluster_map(self, x: torch.Tensor, S: int, window: Tuple[int, int]) -> torch.Tensor:
        """Frames x [B,3,H,W] -> class map [B,1,H,W]: hot path per window, stitched on the device."""
        win, stride = window
        B, _, h, w = x.shape
        acc = torch.zeros((B, h, w, self.num_classes), dtype=torch.float32, device=self.gpu_device)
        for y0, x0 in tiling.window_origins(h, w, win, stride):
            feats = self._tokens(x[..., y0:y0 + win, x0:x0 + win])
            label_hat, _, _ = self._label_hat(feats, False)
            ops.upsample_accumulate(label_hat, S, acc, y0, x0, win, win)
        return ops.argmax_channels(acc)

    def _evaluate_sharded(self, val_loader, S, metric, want_details, knns, knns_labels, knns_ca_labels, window=None):
        """Validation batches are dealt round-robin; all ranks step together so that every search sees all
        shards.  A rank that has run out of batches contributes zero queries.  With sliding windows the ranks also
        step window by window (all frames of a step must have the same size)."""
        n_batches = len(val_loader)
        D = self.index.d
        steps = (n_batches + self.world - 1) // self.world
        k = self.n_neighbours
        # every rank LOADS only the batches it is dealt (hdist.rank_batches: a DataLoader fetches just those index batches), and the
        # ragged query all-gather has a fixed shape when the loader's batch size is known: one collective per step, no host round
        # trip before it
        own = iter(hdist.rank_batches(val_loader, lambda i: i % self.world == self.rank))
        bsz = getattr(val_loader, "batch_size", None)
        max_rows = int(bsz) * S * S if isinstance(bsz, int) and bsz > 0 else None
        for step in range(steps):
            mine = next(own)[1] if step * self.world + self.rank < n_batches else None
            fh = fw = 0
            if window is not None:      # all ranks step through the same windows: agree on the step's frame size
                hw = torch.tensor([mine[0].shape[-2], mine[0].shape[-1]] if mine is not None else [0, 0], dtype=torch.int64, device=self.gpu_device)
                torch.distributed.all_reduce(hw, op=torch.distributed.ReduceOp.MAX)
                fh, fw = (int(v) for v in hw.cpu().tolist())
            origins = [(0, 0)] if window is None else tiling.window_origins(fh, fw, window[0], window[1])
            acc, cluster_map = None, None
            for y0, x0 in origins:
                if mine is not None:
                    x, y = mine
                    if window is not None:
                        x = x[..., y0:y0 + window[0], x0:x0 + window[0]]
                    h, w = x.shape[-2:]
                    feats = self._tokens(x)
                    B, N, _ = feats.shape
                    q = feats.reshape(B * N, D)
                else:
                    q = torch.zeros((0, D), dtype=torch.float32, device=self.gpu_device)
                qall, nq = hdist.allgather_rows(q, max_rows)      # ragged query batches, zero-padded (to the loader's batch size x tokens)
                mx = qall.shape[1]
                if mx == 0:
                    continue
                q_flat_all = qall.reshape(self.world * mx, D)
                idx, dist = self.find_neighbours(q_flat_all, k)   # collective inside
                lh_all = None
                if self.label_shard:
                    # every rank: the weights of the full lists, the label sum over the neighbours it owns; the all-reduce completes it
                    self.index.use_current_stream()
                    lh_all = k5(self.index, "aggregate_partial", k)(q_flat_all, idx, dist, self._label_table[1], beta=self.beta, id_base=self.id_base)
                    torch.distributed.all_reduce(lh_all)
                kf_all, kl_all = None, None
                if want_details:
                    # neighbour features live on their owning shard: every rank fills in its own rows, the
                    # all-reduce (sum with zeros) completes them -- a collective, so all ranks take part
                    flat = idx.reshape(-1)
                    own = (flat >= self.id_base) & (flat < self.id_base + self.index.ntotal)
                    kf_all = self.index.reconstruct(torch.where(own, flat, torch.full_like(flat, -1)),
                                                    id_base=self.id_base)
                    torch.distributed.all_reduce(kf_all)
                    kf_all = kf_all.view(self.world * mx, k, D)
                    if self.label_shard:       # neighbour label rows the same way (ids outside this shard come back as zero rows)
                        local = torch.where(own, flat - self.id_base, torch.full_like(flat, -1))
                        kl_all = (self.index.gather_labels(local) if self.index.ntotal
                                  else torch.zeros((flat.numel(), self.num_classes), device=self.gpu_device))
                        torch.distributed.all_reduce(kl_all)
                        kl_all = kl_all.view(self.world * mx, k, -1)
                if mine is None:
                    continue
                lo = self.rank * mx
                my_idx, my_dist = idx[lo:lo + q.shape[0]].contiguous(), dist[lo:lo + q.shape[0]].contiguous()
                self.index.use_current_stream()
                if self.label_shard:
                    label_hat = lh_all[lo:lo + q.shape[0]].contiguous().view(B, N, -1)
                else:
                    label_hat = k5(self.index, "aggregate", k)(q.contiguous(), my_idx, my_dist, beta=self.beta).view(B, N, -1)
                if want_details:
                    kl = (kl_all[lo:lo + q.shape[0]].reshape(B, N, k, -1) if self.label_shard
                          else self._replicated_label_rows(my_idx.reshape(-1)).view(B, N, k, -1))
                    knns.append(kf_all[lo:lo + q.shape[0]].reshape(B, N, k, D).cpu())
                    knns_labels.append(kl.cpu())
                    knns_ca_labels.append(label_hat.cpu())
                if window is None:
                    metric.update_from_label_hat((mine[1].to(self.gpu_device) * 255).long(), label_hat, S)   # K6 + K7 fused
                else:
                    if acc is None:
                        acc = torch.zeros((B, fh, fw, self.num_classes), dtype=torch.float32, device=self.gpu_device)
                    ops.upsample_accumulate(label_hat, S, acc, y0, x0, h, w)
            if mine is None:
                continue
            if window is not None:
                metric.update((mine[1].to(self.gpu_device) * 255).long(), ops.argmax_channels(acc))
        if want_details and not knns:
            z = torch.zeros(0)
            knns.append(z); knns_labels.append(z); knns_ca_labels.append(z)


def hbird_evaluation(model, d_model: int, patch_size: int, dataset_name: str, data_dir: str, batch_size: int = 64,
                     input_size: int = 224, augmentation_epoch: int = 1, device: str | torch.device = "cpu",
                     return_knn_details: bool = False, n_neighbours: int = 30, nn_method: str = "scann",
                     nn_params: Optional[Dict[str, Any]] = None, ftr_extr_fn=None,
                     memory_size: Optional[int] = None, num_workers: int = 8, ignore_index: int = 255,
                     train_fs_path: Optional[str] = None, val_fs_path: Optional[str] = None,
                     frame_size: Optional[Tuple[int, int]] = None, window_stride: Optional[int] = None,
                     f_mem_p: Optional[str] = None, l_mem_p: Optional[str] = None, grid_k=None, grid_beta=None,
                     leave_one_out: bool = False, leave_one_out_images: Optional[int] = None,
                     leave_one_out_screen: bool = False, bootstrap: Optional[int] = None, bootstrap_seed: Optional[int] = None,
                     overclustering=None, overclustering_seed: int = 0, overclustering_iters: int = 20,
                     linear_probe: bool = False, linear_probe_l2: float = 1e-3, linear_probe_gtol: float = 1e-5, linear_probe_iters: int = 200,
                     memory_sizes=None):
    """High-level entry point with the reference's signature (hbird_eval.py:640-660).

    Four trailing keywords are not in the reference: `frame_size=(H, W)` makes the datasets deliver H x W frames that
    are processed through `input_size` windows with stride `window_stride` (default: input_size, i.e. no overlap) --
    bank build from the window crops, evaluation stitched over the windows (BASELINE cfg-5, hbird_mi/tiling.py).
    `f_mem_p` / `l_mem_p`: the bank's file pair (the constructor arguments the reference never passes, hbird_eval.py:701-712):
    a first run builds the bank and saves it there, a later run with both files present loads it and skips the build --
    one bank reused across runs, for any number of ranks.
    `memory_sizes=[...]` (a fifth one): the memory-size sweep of the reference's mIoU table out of ONE bank build -- the bank is built at
    `memory_size`, every listed size <= memory_size is evaluated on a view of it (`HbirdEvaluation.memory_view`: the rows a build at that
    size would hold, bit for bit), and the call returns {size: what the call returns for that size alone}.
    `grid_k=[...]` / `grid_beta=[...]` (either or both; the other defaults to `n_neighbours` / 0.02): the sweep over n_neighbours and the softmax
    temperature out of ONE validation pass with one search per batch (`HbirdEvaluation.evaluate_grid`); the call returns {(k, beta): mIoU},
    combined with `memory_sizes` {size: {(k, beta): mIoU}} -- still one validation pass, over all sizes.  Not with sliding windows,
    return_knn_details or torch.distributed (ValueError).
    `leave_one_out=True`: the scores come from the TRAIN loader instead of the validation loader -- every training image queries the bank
    with its own rows excluded (`HbirdEvaluation.evaluate_leave_one_out`), so n_neighbours, the temperature and the memory size can be chosen
    without tuning on the validation split; `leave_one_out_images=N` stops after N images; `leave_one_out_screen=True` lets the certified fp16 screen
    serve the excluding searches (`HipFlatIndex.set_exclusion_screen`: same scores, the cost of plain searches at k).  The return shape is that of the call it
    accompanies: a float, {(k, beta): mIoU} with a grid, {size: ...} with `memory_sizes`.  Same restrictions as the grid.
    `bootstrap=R` (`bootstrap_seed=`: the resampler's seed, default `hbird_mi.bootstrap.DEFAULT_SEED`): the call returns a
    `hbird_mi.bootstrap.MiouBootstrap` -- R paired bootstrap replicates over the evaluated images of every configuration's mIoU, with
    intervals, paired differences and the configurations indistinguishable from the best.  Its keys are (k, beta), with `memory_sizes`
    (size, k, beta); a run without a grid is a grid of one configuration.  Works with `leave_one_out`; same restrictions as the grid.
    `overclustering=[K, ...]` (`overclustering_seed=`, `overclustering_iters=`: the k-means initialisation's seed and its iteration limit): the
    overclustering protocol instead of the retrieval one -- k-means over the bank, clusters matched to classes
    (`HbirdEvaluation.evaluate_overclustering`); the call returns {K: mIoU}.  Not with a grid, `memory_sizes`, `leave_one_out` or `bootstrap`,
    nor with sliding windows, return_knn_details or torch.distributed (ValueError).
    `linear_probe=True` (`linear_probe_l2=`, `linear_probe_gtol=`, `linear_probe_iters=`: the fit's l2 weight, gradient tolerance and iteration
    limit -- definitions, not values tuned on real data): the linear-head protocol instead of the retrieval one -- a softmax head fitted on the
    bank, scored with the identity matching (`HbirdEvaluation.evaluate_linear_probe`); the call returns its mIoU and `last_run_info` gains
    `linear_probe_fit`.  Same exclusions as `overclustering`, and not together with it."""
    if linear_probe:
        for name, given in (("grid_k", grid_k is not None), ("grid_beta", grid_beta is not None), ("memory_sizes", memory_sizes is not None),
                            ("leave_one_out", bool(leave_one_out)), ("bootstrap", bootstrap is not None),
                            ("return_knn_details", bool(return_knn_details)), ("frame_size", frame_size is not None),
                            ("overclustering", overclustering is not None)):
            if given:
                raise ValueError(f"linear_probe is not available with {name}")
    if overclustering is not None:
        for name, given in (("grid_k", grid_k is not None), ("grid_beta", grid_beta is not None), ("memory_sizes", memory_sizes is not None),
                            ("leave_one_out", bool(leave_one_out)), ("bootstrap", bootstrap is not None),
                            ("return_knn_details", bool(return_knn_details)), ("frame_size", frame_size is not None)):
            if given:
                raise ValueError(f"overclustering is not available with {name}")
        from hbird_mi.kmeans import check_n_clusters
        overclustering = [overclustering] if not isinstance(overclustering, (list, tuple)) else list(overclustering)
        if not overclustering:
            raise ValueError("overclustering is empty")
        for k in overclustering:
            check_n_clusters(k, who="overclustering")
    if bootstrap is None and bootstrap_seed is not None:
        raise ValueError("bootstrap_seed needs bootstrap")
    if leave_one_out and (return_knn_details or frame_size is not None):
        raise ValueError("leave_one_out is not available with return_knn_details or sliding windows (frame_size)")
    if memory_sizes is not None and memory_size is None:
        raise ValueError("memory_sizes needs memory_size: the bank is built once, at memory_size, and the listed sizes are views of it")
    if nn_params is None:
        nn_params = {}
    eval_spatial_resolution = input_size // patch_size                                   # 671
    if ftr_extr_fn is None:
        feature_extractor = FeatureExtractor(model, eval_spatial_resolution=eval_spatial_resolution, d_model=d_model)
    else:
        feature_extractor = FeatureExtractorSimple(model, ftr_extr_fn=ftr_extr_fn,
                                                   eval_spatial_resolution=eval_spatial_resolution, d_model=d_model)
    from hbird_mi.data import get_dataset
    window = None
    if frame_size is not None:
        fh, fw = int(frame_size[0]), int(frame_size[1])
        window = (input_size, int(window_stride) if window_stride else input_size)
        if fh < input_size or fw < input_size:
            raise ValueError(f"frame_size {frame_size} smaller than the {input_size} x {input_size} window")
    elif window_stride is not None:
        raise ValueError("window_stride needs frame_size")
    dataset, ignore_index_local = get_dataset(dataset_name, data_dir, batch_size, num_workers,
                                              input_size if window is None else (fh, fw), train_fs_path, val_fs_path)
    dataset_size = dataset.get_train_dataset_size()
    num_classes = dataset.get_num_classes()
    train_loader = dataset.train_dataloader()
    val_loader = dataset.val_dataloader()
    if window is not None:
        train_loader = tiling.WindowedLoader(train_loader, window[0], window[1], frame_hw=(fh, fw))
        dataset_size *= train_loader.windows_per_frame()       # every window is a bank image
    evaluator = HbirdEvaluation(feature_extractor, train_loader, num_classes=num_classes, n_neighbours=n_neighbours,
                                augmentation_epoch=augmentation_epoch, device=device, nn_method=nn_method,
                                nn_params=nn_params, memory_size=memory_size, dataset_size=dataset_size,
                                f_mem_p=f_mem_p, l_mem_p=l_mem_p, reuse_memory=True)
    effective_ignore = ignore_index if ignore_index != 255 else ignore_index_local        # 715
    last_run_info.clear()
    last_run_info.update(bank_loaded=bool(evaluator.bank_loaded), bank_build_s=float(evaluator.bank_build_s),
                         bank_rows=int(evaluator.total_rows), train_batches_loaded=int(evaluator.batches_loaded))
    if linear_probe:
        miou = evaluator.evaluate_linear_probe(val_loader, eval_spatial_resolution, l2=linear_probe_l2, gtol=linear_probe_gtol,
                                               max_iter=linear_probe_iters, ignore_index=effective_ignore)
        fit = evaluator.last_linear_probe
        last_run_info.update(linear_probe_fit=dict(state=fit["state"], iterations=int(fit["n_iter"]), loss=float(fit["loss"]),
                                                   rows_used=int(fit["rows_used"]), rows_skipped=int(fit["rows_skipped"])))
        return miou
    if overclustering is not None:
        return evaluator.evaluate_overclustering(val_loader, eval_spatial_resolution, overclustering, seed=overclustering_seed,
                                                 max_iter=overclustering_iters, ignore_index=effective_ignore)
    if bootstrap is not None:
        ks, bs = n_neighbours if grid_k is None else grid_k, evaluator.beta if grid_beta is None else grid_beta
        sized = None
        if memory_sizes is not None:
            sized = {}
            for size in memory_sizes:
                size = int(size)
                if size > memory_size or size in sized:
                    continue
                sized[size] = evaluator if size == memory_size else evaluator.memory_view(
                    memory_size=size, rows_per_image=evaluator.num_sampled_features if evaluator.bank_loaded else None)
        try:
            if leave_one_out:
                return evaluator.evaluate_leave_one_out(train_loader, eval_spatial_resolution, n_neighbours=ks, betas=bs, views=sized,
                                                        ignore_index=effective_ignore, max_images=leave_one_out_images,
                                                        screen=True if leave_one_out_screen else None, bootstrap=(bootstrap, bootstrap_seed))
            return evaluator.evaluate_grid(val_loader, eval_spatial_resolution, n_neighbours=ks, betas=bs, views=sized,
                                           ignore_index=effective_ignore, window=window, return_knn_details=return_knn_details,
                                           bootstrap=(bootstrap, bootstrap_seed))
        finally:
            for ev in (sized or {}).values():
                if ev is not evaluator:
                    ev.index.close()
    if leave_one_out:
        gridded = grid_k is not None or grid_beta is not None
        loo = dict(n_neighbours=grid_k if grid_k is not None else n_neighbours, betas=grid_beta if grid_beta is not None else evaluator.beta,
                   ignore_index=effective_ignore, max_images=leave_one_out_images,
                   screen=True if leave_one_out_screen else None)
        if memory_sizes is None:
            res = evaluator.evaluate_leave_one_out(train_loader, eval_spatial_resolution, **loo)
            return res if gridded else next(iter(res.values()))
        views = {}
        for size in memory_sizes:
            size = int(size)
            if size > memory_size or size in views:
                continue
            views[size] = evaluator if size == memory_size else evaluator.memory_view(
                memory_size=size, rows_per_image=evaluator.num_sampled_features if evaluator.bank_loaded else None)
        results = {size: {} for size in views}
        try:
            if views:
                for (size, k, beta), v in evaluator.evaluate_leave_one_out(train_loader, eval_spatial_resolution, views=views, **loo).items():
                    results[size][(k, beta)] = v
        finally:
            for ev in views.values():
                if ev is not evaluator:
                    ev.index.close()
        return results if gridded else {size: next(iter(res.values())) for size, res in results.items()}
    if grid_k is not None or grid_beta is not None:
        grid = dict(n_neighbours=n_neighbours if grid_k is None else grid_k, betas=evaluator.beta if grid_beta is None else grid_beta,
                    ignore_index=effective_ignore, window=window, return_knn_details=return_knn_details)
        if memory_sizes is None:
            return evaluator.evaluate_grid(val_loader, eval_spatial_resolution, **grid)
        views = {}
        for size in memory_sizes:
            size = int(size)
            if size > memory_size or size in views:
                continue
            views[size] = evaluator if size == memory_size else evaluator.memory_view(
                memory_size=size, rows_per_image=evaluator.num_sampled_features if evaluator.bank_loaded else None)
        results = {size: {} for size in views}
        try:
            if views:
                for (size, k, beta), v in evaluator.evaluate_grid(val_loader, eval_spatial_resolution, views=views, **grid).items():
                    results[size][(k, beta)] = v
        finally:
            for ev in views.values():
                if ev is not evaluator:
                    ev.index.close()
        return results
    if memory_sizes is None:
        return evaluator.evaluate(val_loader, eval_spatial_resolution=eval_spatial_resolution,
                                  return_knn_details=return_knn_details, ignore_index=effective_ignore, window=window)
    results = {}
    for size in memory_sizes:
        size = int(size)
        if size > memory_size or size in results:
            continue
        # (a bank loaded from its file pair has no recorded geometry: its blocks are the K rows per image this memory_size keeps)
        ev = evaluator if size == memory_size else evaluator.memory_view(
            memory_size=size, rows_per_image=evaluator.num_sampled_features if evaluator.bank_loaded else None)
        results[size] = ev.evaluate(val_loader, eval_spatial_resolution=eval_spatial_resolution,
                                    return_knn_details=return_knn_details, ignore_index=effective_ignore, window=window)
        if ev is not evaluator:
            ev.index.close()
    return results
