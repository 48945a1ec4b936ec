"""The linear probe (include/hbird_hip_linprobe.h, csrc/hbird_linprobe.hip): a softmax segmentation head fitted on a resident bank -- its
stored rows x[r] against its patch soft labels y[r][c].

One evaluation of the objective and its gradient is one call into libhbird_hip.so over the whole bank (`loss_grad`); the optimiser, L-BFGS in
float64 numpy, runs on the host (`linear_probe_fit`).  Parameters travel as Wb [C, D + 1] fp32: Wb[c, 0] the bias, Wb[c, 1 + k] the weight.

  logits   z[r][c] = the k-ascending fp32 fmaf chain of x[r][k] * w[c][k] started at b[c]; a row with a non-finite component is skipped
  loss     L = (1 / n) sum_r (s lse(z) - y . z) + (l2 / 2) sum Wb^2, s = sum_c y[c], n the rows not skipped; the bias is regularised too
  gradient float64 sums of fp32 segment chains, the segments a function of the row count alone: the same bits every evaluation

The fit: L-BFGS with memory 10 from Wb = 0; the first step length is 1 / ||g||_2, later ones start at 1; Armijo backtracking (c1 = 1e-4,
at most 30 halvings); a pair (s, y) is kept when y . s > 1e-10 ||y|| ||s||; every evaluation rounds Wb to fp32.  It ends `converged` when
||g||_inf <= gtol, `stalled` when the line search is exhausted (fp32 noise in the Armijo test; a reported state, not an error), `max_iter`
otherwise.  The defaults l2 = 1e-3, gtol = 1e-5, max_iter = 200 are definitions, not values tuned on real data.

The image-level probe (include/hbird_hip_linprobe_class.h, csrc/hbird_linprobe_class.hip) is the same head on ONE class id per row instead of a
label row, for up to 16384 classes: `class_logits_of`, `class_loss_grad`, `linear_probe_fit_classes`.  A row of label -1 is skipped like a
non-finite row; for C <= 256 the bits are those of `loss_grad` on the one-hot label table.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from hbird_mi import _lib, ops
from hbird_mi.nn.search_hip import HipFlatIndex, HipMultiIndex

LBFGS_MEMORY, ARMIJO_C1, MAX_HALVINGS, CURVATURE_EPS = 10, 1e-4, 30, 1e-10
LossGrad = namedtuple("LossGrad", "loss grad used skipped residuals")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _single_index(index, who: str) -> HipFlatIndex:
    if isinstance(index, HipMultiIndex):
        raise ValueError(f"{who}: the linear probe runs on one HipFlatIndex -- a HipMultiIndex (row shards or replicas) is not supported yet")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise ValueError(f"{who}: not available under torch.distributed (sharded banks are not supported yet)")
    if not isinstance(index, HipFlatIndex):
        raise ValueError(f"{who}: expected a HipFlatIndex, got {type(index).__name__}")
    return index


def partition(ntotal: int):
    """hb_linprobe_partition: (seg_rows, nseg), the gradient's row segments for a bank of `ntotal` rows."""
    rows, n = ctypes.c_int64(0), ctypes.c_int(0)
    _lib.check(_lib.lib().hb_linprobe_partition(int(ntotal), ctypes.byref(rows), ctypes.byref(n)), ValueError)
    return int(rows.value), int(n.value)


def _params(Wb, d: int, dev: torch.device, who: str) -> torch.Tensor:
    t = Wb if isinstance(Wb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(Wb), dtype=np.float32))
    if t.dim() != 2 or t.shape[1] != d + 1 or not t.dtype.is_floating_point:
        raise ValueError(f"{who}: Wb must be a float [C, {d + 1}] array (bias, then the {d} weights), got {tuple(t.shape)}")
    if t.shape[0] < 1 or t.shape[0] > _lib.LINPROBE_MAX_C:
        raise ValueError(f"{who}: C must be in [1, {_lib.LINPROBE_MAX_C}], got {t.shape[0]}")
    return t.detach().to(dev, torch.float32).contiguous()


def logits_of(index, Wb) -> torch.Tensor:
    """hb_linprobe_logits: z float32 [ntotal, C] (CUDA) of every stored row of `index` (any index; labels are not needed)."""
    index = _single_index(index, "logits_of")
    dev = torch.device("cuda", index.device)
    w = _params(Wb, index.d, dev, "logits_of")
    with torch.cuda.device(dev):
        index.use_current_stream()
        out = torch.empty((index.ntotal, w.shape[0]), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().hb_linprobe_logits(index._h, _p(w), int(w.shape[0]), _p(out)), ValueError)
    return out


def loss_grad(index, Wb, l2: float, return_residuals: bool = False) -> LossGrad:
    """hb_linprobe_loss_grad: one evaluation over the whole bank -> LossGrad(loss float, grad float64 numpy [C, D + 1], used, skipped rows,
    residuals float32 [ntotal, C] CUDA or None)."""
    index = _single_index(index, "loss_grad")
    dev = torch.device("cuda", index.device)
    w = _params(Wb, index.d, dev, "loss_grad")
    if not np.isfinite(float(l2)) or float(l2) < 0:
        raise ValueError(f"loss_grad: l2 must be a non-negative number, got {l2!r}")
    C = int(w.shape[0])
    with torch.cuda.device(dev):
        index.use_current_stream()
        n = index.ntotal
        grad = torch.empty((C, index.d + 1), dtype=torch.float64, device=dev)
        resid = torch.empty((n, C), dtype=torch.float32, device=dev) if return_residuals else None
        loss, used = ctypes.c_double(0.0), ctypes.c_int64(0)
        _lib.check(_lib.lib().hb_linprobe_loss_grad(index._h, _p(w), C, float(l2), ctypes.byref(loss), _p(grad), ctypes.byref(used), _p(resid)),
                   ValueError)
    return LossGrad(float(loss.value), grad.cpu().numpy(), int(used.value), n - int(used.value), resid)


# ---- the image-level probe: one class id per row, any class count up to HB_LINPROBE_CLASS_MAX_C (include/hbird_hip_linprobe_class.h) ----------
def _class_params(Wb, d: int, dev: torch.device, who: str) -> torch.Tensor:
    t = Wb if isinstance(Wb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(Wb), dtype=np.float32))
    if t.dim() != 2 or t.shape[1] != d + 1 or not t.dtype.is_floating_point:
        raise ValueError(f"{who}: Wb must be a float [C, {d + 1}] array (bias, then the {d} weights), got {tuple(t.shape)}")
    if t.shape[0] < 1 or t.shape[0] > _lib.LINPROBE_CLASS_MAX_C:
        raise ValueError(f"{who}: C must be in [1, {_lib.LINPROBE_CLASS_MAX_C}], got {t.shape[0]}")
    return t.detach().to(dev, torch.float32).contiguous()


def _class_labels(labels, ntotal: int, dev: torch.device, who: str) -> torch.Tensor:
    t = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{who}: labels must be a 1-d integer array (one class id per bank row, -1 = unlabelled), got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] != ntotal:
        raise ValueError(f"{who}: {t.shape[0]} labels for a bank of {ntotal} rows")
    if t.dtype != torch.int32:                           # (an id beyond int32 must not wrap into the valid range)
        if t.numel() and (int(t.min()) < -(2 ** 31) or int(t.max()) >= 2 ** 31):
            raise ValueError(f"{who}: a label does not fit int32")
    return t.detach().to(dev, torch.int32).contiguous()


def class_logits_of(index, Wb) -> torch.Tensor:
    """hb_linprobe_class_logits: z float32 [ntotal, C] (CUDA) of every stored row of `index`, C up to 16384: `logits_of`'s bits."""
    index = _single_index(index, "class_logits_of")
    dev = torch.device("cuda", index.device)
    w = _class_params(Wb, index.d, dev, "class_logits_of")
    with torch.cuda.device(dev):
        index.use_current_stream()
        out = torch.empty((index.ntotal, w.shape[0]), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().hb_linprobe_class_logits(index._h, _p(w), int(w.shape[0]), _p(out)), ValueError)
    return out


def class_loss_grad(index, labels, Wb, l2: float, return_residuals: bool = False) -> LossGrad:
    """hb_linprobe_class_loss_grad: one evaluation over the whole bank against `labels` ([ntotal] integers in [0, C), -1 = the row is skipped)
    -> LossGrad as `loss_grad` returns it.  The bank needs no label table."""
    index = _single_index(index, "class_loss_grad")
    dev = torch.device("cuda", index.device)
    w = _class_params(Wb, index.d, dev, "class_loss_grad")
    y = _class_labels(labels, index.ntotal, dev, "class_loss_grad")
    if not np.isfinite(float(l2)) or float(l2) < 0:
        raise ValueError(f"class_loss_grad: l2 must be a non-negative number, got {l2!r}")
    C = int(w.shape[0])
    with torch.cuda.device(dev):
        index.use_current_stream()
        n = index.ntotal
        grad = torch.empty((C, index.d + 1), dtype=torch.float64, device=dev)
        resid = torch.empty((n, C), dtype=torch.float32, device=dev) if return_residuals else None
        loss, used = ctypes.c_double(0.0), ctypes.c_int64(0)
        _lib.check(_lib.lib().hb_linprobe_class_loss_grad(index._h, _p(y), _p(w), C, float(l2), ctypes.byref(loss), _p(grad), ctypes.byref(used),
                                                          _p(resid)), ValueError)
    return LossGrad(float(loss.value), grad.cpu().numpy(), int(used.value), n - int(used.value), resid)


def lbfgs(fun, x0: np.ndarray, gtol: float, max_iter: int):
    """The fit's loop on `fun(x) -> (loss, grad)` (float64 arrays of x0's shape) -> (x, history [(loss, ||g||_inf)], n_iter, state)."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    history, S, Y, n_iter = [(float(f), float(np.abs(g).max()))], [], [], 0
    while True:
        if np.abs(g).max() <= gtol:
            return x, history, n_iter, "converged"
        if n_iter >= max_iter:
            return x, history, n_iter, "max_iter"
        q, alphas = g.copy(), []
        for s, y in zip(reversed(S), reversed(Y)):
            a = float(np.vdot(s, q)) / float(np.vdot(y, s))
            alphas.append(a)
            q -= a * y
        if S:
            q *= float(np.vdot(S[-1], Y[-1])) / float(np.vdot(Y[-1], Y[-1]))
        for (s, y), a in zip(zip(S, Y), reversed(alphas)):
            q += (a - float(np.vdot(y, q)) / float(np.vdot(y, s))) * s
        d = -q
        gd = float(np.vdot(g, d))
        if not gd < 0:                                   # (not a descent direction: steepest descent, the memory dropped)
            d, S, Y = -g, [], []
            gd = float(np.vdot(g, d))
        t = 1.0 / float(np.linalg.norm(g)) if n_iter == 0 else 1.0
        for _ in range(MAX_HALVINGS + 1):
            xn = x + t * d
            fn, gn = fun(xn)
            if fn <= f + ARMIJO_C1 * t * gd:
                break
            t *= 0.5
        else:
            return x, history, n_iter, "stalled"
        s, y = xn - x, gn - g
        if float(np.vdot(y, s)) > CURVATURE_EPS * float(np.linalg.norm(y)) * float(np.linalg.norm(s)):
            S.append(s); Y.append(y)
            S, Y = S[-LBFGS_MEMORY:], Y[-LBFGS_MEMORY:]
        x, f, g = xn, fn, gn
        n_iter += 1
        history.append((float(f), float(np.abs(g).max())))


@dataclass
class LinearProbe:
    """weights float32 [C, D] and bias float32 [C] (CUDA); history: one dict(loss, gmax) per iterate, the start included; n_iter: the steps
    taken; state: "converged", "stalled" or "max_iter"; rows_used / rows_skipped: the bank's rows in the fit / with a non-finite component."""
    weights: torch.Tensor
    bias: torch.Tensor
    history: list
    n_iter: int
    state: str
    rows_used: int
    rows_skipped: int
    l2: float = 0.0
    _scratch: Optional[HipFlatIndex] = field(default=None, repr=False, compare=False)

    @property
    def num_classes(self) -> int:
        return int(self.weights.shape[0])

    @property
    def Wb(self) -> torch.Tensor:
        """The parameters as the C ABI takes them: float32 [C, D + 1], the bias in column 0."""
        return torch.cat([self.bias.view(-1, 1), self.weights], dim=1).contiguous()

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        """z float32 [..., C] of the tokens x [..., D] (a CUDA tensor on the probe's GPU): the rows are normalised with `ops.normalize_rows`,
        appended to a cached scratch index (`reset()`, `add` at `set_fp16(0)`) and handed to hb_linprobe_logits -- the bank's own arithmetic
        (hb_linprobe_class_logits, the same bits, for a probe of more than 256 classes)."""
        D = int(self.weights.shape[1])
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() < 2 or x.shape[-1] != D:
            raise ValueError(f"LinearProbe.logits: expected a CUDA tensor [..., {D}]")
        if x.device != self.weights.device:
            raise ValueError("LinearProbe.logits: x lives on another GPU than the probe")
        rows = ops.normalize_rows(x.reshape(-1, D).contiguous())
        if rows.shape[0] == 0:
            return torch.empty(tuple(x.shape[:-1]) + (self.num_classes,), dtype=torch.float32, device=x.device)
        if self._scratch is None:
            self._scratch = HipFlatIndex(D, 0, self.weights.device.index)
            self._scratch.set_fp16(0)
        ix = self._scratch
        with torch.cuda.device(x.device):
            ix.use_current_stream()
            ix.reset()
            ix.add(rows, normalize=False)
            z = logits_of(ix, self.Wb) if self.num_classes <= _lib.LINPROBE_MAX_C else class_logits_of(ix, self.Wb)
        return z.view(tuple(x.shape[:-1]) + (self.num_classes,))

    def close(self) -> None:
        if self._scratch is not None:
            self._scratch.close()
            self._scratch = None


def linear_probe_fit(index, l2: float = 1e-3, gtol: float = 1e-5, max_iter: int = 200) -> LinearProbe:
    """Fit the softmax head on the rows and label rows of `index` (see the module's text).  ValueError for a HipMultiIndex, under
    torch.distributed, for a bank without label rows for every row, or more than 256 classes."""
    index = _single_index(index, "linear_probe_fit")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f"linear_probe_fit: max_iter must be a non-negative integer, got {max_iter!r}")
    if not (np.isfinite(float(l2)) and float(l2) >= 0 and np.isfinite(float(gtol)) and float(gtol) >= 0):
        raise ValueError("linear_probe_fit: l2 and gtol must be non-negative numbers")
    try:
        C, D = int(index.num_classes), index.d
    except RuntimeError:                                 # (HipFlatIndex.num_classes: "labels were not added to this index")
        C, D = 0, index.d
    if C < 1:
        raise ValueError("linear_probe_fit: the bank has no label rows")
    if C > _lib.LINPROBE_MAX_C:
        raise ValueError(f"linear_probe_fit: C must be in [1, {_lib.LINPROBE_MAX_C}], got {C}")
    used = [0, 0]

    def fun(x):
        r = loss_grad(index, x.astype(np.float32), l2)
        used[:] = [r.used, r.skipped]
        return r.loss, r.grad

    x, history, n_iter, state = lbfgs(fun, np.zeros((C, D + 1), dtype=np.float64), float(gtol), int(max_iter))
    dev = torch.device("cuda", index.device)
    wb = torch.from_numpy(x.astype(np.float32)).to(dev)
    return LinearProbe(wb[:, 1:].contiguous(), wb[:, 0].contiguous(), [dict(loss=f, gmax=g) for f, g in history], n_iter, state, used[0], used[1],
                       float(l2))


def linear_probe_fit_classes(index, labels, num_classes: int, l2: float = 1e-3, gtol: float = 1e-5, max_iter: int = 200, Wb0=None) -> LinearProbe:
    """Fit the softmax head on the rows of `index` against one class id per row (`labels`: [ntotal] integers in [0, num_classes), -1 = the row
    takes no part): the image-level linear probe, for up to 16384 classes.  The same L-BFGS and the same `LinearProbe` as `linear_probe_fit`;
    `Wb0` ([num_classes, D + 1], bias first) is a warm start, None starts at 0.  The defaults are definitions, not values tuned on real data.
    The definition is this engine's own -- an L2-penalised softmax head on normalised features by full-batch L-BFGS, not DINO's SGD recipe with
    batch norm; no accuracy has been held to a published one.  ValueError for a HipMultiIndex and under torch.distributed."""
    index = _single_index(index, "linear_probe_fit_classes")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f"linear_probe_fit_classes: max_iter must be a non-negative integer, got {max_iter!r}")
    if not (np.isfinite(float(l2)) and float(l2) >= 0 and np.isfinite(float(gtol)) and float(gtol) >= 0):
        raise ValueError("linear_probe_fit_classes: l2 and gtol must be non-negative numbers")
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= _lib.LINPROBE_CLASS_MAX_C:
        raise ValueError(f"linear_probe_fit_classes: C must be in [1, {_lib.LINPROBE_CLASS_MAX_C}], got {num_classes!r}")
    C, D = int(num_classes), index.d
    dev = torch.device("cuda", index.device)
    y = _class_labels(labels, index.ntotal, dev, "linear_probe_fit_classes")
    if Wb0 is None:
        x0 = np.zeros((C, D + 1), dtype=np.float64)
    else:
        x0 = _class_params(Wb0, D, dev, "linear_probe_fit_classes").cpu().numpy().astype(np.float64)
        if x0.shape[0] != C:
            raise ValueError(f"linear_probe_fit_classes: Wb0 has {x0.shape[0]} classes, num_classes is {C}")
    used = [0, 0]

    def fun(x):
        r = class_loss_grad(index, y, x.astype(np.float32), l2)
        used[:] = [r.used, r.skipped]
        return r.loss, r.grad

    x, history, n_iter, state = lbfgs(fun, x0, float(gtol), int(max_iter))
    wb = torch.from_numpy(x.astype(np.float32)).to(dev)
    return LinearProbe(wb[:, 1:].contiguous(), wb[:, 0].contiguous(), [dict(loss=f, gmax=g) for f, g in history], n_iter, state, used[0], used[1],
                       float(l2))
