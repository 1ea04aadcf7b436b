"""Grouped (k-fold, leave-one-group-out) cross-validation from ONE factorisation of the training covariance.

With P = Ky^-1, alpha = P (y - mean) and a fold F (an index set), the held-out distribution of the fold is
    p(y_F | y_-F) = N(y_F - P_FF^-1 alpha_F, P_FF^-1),     cv = sum_F [-1/2 alpha_F' P_FF^-1 alpha_F + 1/2 log|P_FF|] - (N / 2) log 2 pi
(folds of one point: the leave-one-out quantities of ``linalg.ExactLOOFunction``; one fold of everything: the marginal likelihood).
The reference has no counterpart (optim/mll_noise_continuation.py:54 names a LOOCV criterion and never evaluates it).

:class:`FoldIndex` normalises what a caller gives as folds (an int k or one integer label per row) into CSR arrays, grouped into
BUCKETS by padded size on the fixed ladder ``LADDER``; :func:`fold_solves` runs the per-bucket batched sequence — gpp_cv_blocks, then
the existing batched factorisation, inverse and triangular products on the batch of small problems (P_FF, alpha_F).  Padded storage
stays within a constant factor of sum m_F^2 and the launch count is bounded by the ladder, not by the number of folds.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .errors import NotPSDError

__all__ = ["FoldIndex", "group_labels", "fold_solves", "fold_gradient_factors", "check_infos", "MAX_FOLD", "LADDER"]

#: largest fold: the limit of gpp_potrf_batched (the leaf-step factorisation, gpp_api.hip BLK_MAX)
MAX_FOLD = 6144
#: padded fold sizes; a fold goes into the first bucket that holds it
LADDER = (32, 128, 512, 2048, MAX_FOLD)
#: most folds one batched sequence takes (the batched entry points take at most 65535 problems per launch)
MAX_BATCH = 32768


def _labels_to_numpy(labels) -> np.ndarray:
    if isinstance(labels, torch.Tensor):
        if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise TypeError(f"fold labels must be integers (got {labels.dtype})")
        arr = labels.detach().cpu().numpy()
    else:
        arr = np.asarray(labels)
        if arr.dtype.kind not in "iu":
            raise TypeError(f"fold labels must be integers (got dtype {arr.dtype})")
    return arr


class FoldIndex:
    """The folds of a cross-validation over N rows as CSR arrays: ``idx`` (N indices, ascending inside a fold) and ``off``
    (nfolds + 1 offsets), folds ordered by label; every row is in exactly one fold.

    ``folds``: an int k — a random partition into k folds whose sizes differ by at most one, drawn from the CPU ``generator`` (or from
    ``seed``) — or a 1-D vector of N integer labels (tensor or numpy; any integers), rows with equal labels forming a fold; or a
    FoldIndex of the same N, returned as it is.  Everything here is host work: the errors are raised before a device is touched."""

    def __init__(self, folds, N: int, generator: Optional[torch.Generator] = None, seed: int = 0):
        N = int(N)
        if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
            k = int(folds)
            if k < 1 or k > N:
                raise ValueError(f"k-fold cross-validation needs 1 <= k <= N (got k = {k}, N = {N})")
            if generator is None:
                generator = torch.Generator(device="cpu")
                generator.manual_seed(int(seed))
            perm = torch.randperm(N, generator=generator).numpy()
            labels = np.empty(N, dtype=np.int64)
            labels[perm] = np.arange(N) % k  # fold j gets ceil((N - j) / k) rows
        else:
            labels = _labels_to_numpy(folds)
            if labels.ndim != 1 or labels.shape[0] != N:
                raise ValueError(f"fold labels must be a vector of length N = {N} (got shape {tuple(labels.shape)})")
            labels = labels.astype(np.int64, copy=False) if labels.dtype != np.uint64 else labels
        order = np.argsort(labels, kind="stable")  # by label, ascending index inside a label
        sorted_labels = labels[order]
        starts = np.flatnonzero(np.r_[True, sorted_labels[1:] != sorted_labels[:-1]]) if N > 0 else np.zeros(0, dtype=np.int64)
        self.N = N
        self.idx = order.astype(np.int32)
        self.off = np.r_[starts, N].astype(np.int32)
        self.sizes = np.diff(self.off)
        self.labels = sorted_labels[starts]
        self.nfolds = int(self.sizes.shape[0])
        if self.nfolds and int(self.sizes.max()) > MAX_FOLD:
            f = int(self.sizes.argmax())
            raise ValueError(f"fold {f} (label {int(self.labels[f])}) has {int(self.sizes[f])} rows: a fold holds at most {MAX_FOLD} "
                             "(the limit of the batched factorisation)")
        self._buckets: Optional[List[SimpleNamespace]] = None
        self._device: Dict[str, List[SimpleNamespace]] = {}

    @staticmethod
    def make(folds, N: int, generator: Optional[torch.Generator] = None) -> "FoldIndex":
        if isinstance(folds, FoldIndex):
            if folds.N != int(N):
                raise ValueError(f"the folds index {folds.N} rows, the model has {int(N)}")
            return folds
        return FoldIndex(folds, N, generator=generator)

    def fold(self, f: int) -> np.ndarray:
        return self.idx[self.off[f]:self.off[f + 1]]

    def buckets(self) -> List[SimpleNamespace]:
        """Host description of the non-empty buckets, in ladder order (batches of at most ``MAX_BATCH`` folds): ``mp`` the padded size,
        ``folds`` the fold numbers, ``sizes`` their sizes, ``idx`` / ``off`` the bucket's own CSR list (``idx`` holds original rows),
        ``pos`` the place f * mp + a of every entry of ``idx`` in a (nfolds, mp) padded vector, ``base`` the bucket's first row in a
        stacked S."""
        if self._buckets is None:
            out, base, lo = [], 0, 0
            for mp in LADDER:
                members = np.flatnonzero((self.sizes > lo) & (self.sizes <= mp))
                lo = mp
                for c0 in range(0, members.shape[0], MAX_BATCH):
                    fs = members[c0:c0 + MAX_BATCH]
                    sizes = self.sizes[fs]
                    off = np.r_[0, np.cumsum(sizes)].astype(np.int32)
                    idx = np.concatenate([self.fold(int(f)) for f in fs]).astype(np.int32)
                    local = np.arange(idx.shape[0]) - np.repeat(off[:-1], sizes)
                    pos = np.repeat(np.arange(fs.shape[0], dtype=np.int64), sizes) * _vec_stride(mp) + local
                    out.append(SimpleNamespace(mp=mp, folds=fs, sizes=sizes, idx=idx, off=off, pos=pos, base=base))
                    base += int(idx.shape[0])
            self._buckets = out
        return self._buckets

    def on(self, device) -> List[SimpleNamespace]:
        """The buckets with their index arrays on ``device`` (cached per device)."""
        key = str(torch.device(device))
        got = self._device.get(key)
        if got is None:
            got = []
            for b in self.buckets():
                got.append(SimpleNamespace(mp=b.mp, nf=int(b.folds.shape[0]), folds=b.folds, base=b.base, rows=int(b.idx.shape[0]),
                                           idx=torch.from_numpy(b.idx).to(device), off=torch.from_numpy(b.off).to(device),
                                           gather=torch.from_numpy(b.idx.astype(np.int64)).to(device),
                                           pos=torch.from_numpy(b.pos).to(device),
                                           fold_ids=torch.from_numpy(b.folds.astype(np.int64)).to(device)))
            self._device[key] = got
        return got


def _vec_stride(n: int) -> int:
    return n + (n & 1)  # GppContext.batched_vector


def group_labels(X, columns: Sequence[int]) -> np.ndarray:
    """One integer label per row of X, equal for rows that agree in the given columns: the folds of "leave one categorical level
    combination out" (``columns = list(qual_dict)``) or "leave one source out" (the source column)."""
    arr = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
    if arr.ndim != 2:
        raise ValueError("group_labels takes a 2-D array of inputs")
    cols = [int(c) for c in columns]
    if not cols:
        raise ValueError("group_labels needs at least one column")
    _, inverse = np.unique(arr[:, cols], axis=0, return_inverse=True)
    return np.asarray(inverse).reshape(-1).astype(np.int64)


def fold_solves(gctx, Linv: torch.Tensor, alpha: torch.Tensor, folds: FoldIndex, keep_factors: bool = False):
    """The per-fold solves of one evaluation, one batched sequence per bucket, all enqueued without a host wait:
    gpp_cv_blocks (P_FF, identity-padded) -> potrf_batched (P_FF = U'U) -> trtri_batched (Linv_F = U^-T) -> mll_reduce_batched
    (z = Linv_F alpha_F, quad = z'z, logdet = 2 sum log U_ii) -> alpha_batched (-a = Linv_F' z = P_FF^-1 alpha_F) -> loo_scalars_batched
    (diag P_FF^-1 = the column sums of squares of Linv_F).

    Returns (a, d, terms, infos, kept): ``a`` (N, dcv/dalpha; the held-out mean is y + a) and ``d`` (N, the held-out variances) in
    the original row order, ``terms`` (nfolds,) the per-fold values -quad / 2 + logdet / 2 in fold order, ``infos`` a list of
    (bucket, int32 status per fold) still on the device, and with ``keep_factors`` per bucket (Linv_F batch, z, a) for the gradient."""
    dev = Linv.device
    N = folds.N
    f64 = dict(dtype=torch.float64, device=dev)
    a_full, d_full = torch.empty(N, **f64), torch.empty(N, **f64)
    terms = torch.empty(folds.nfolds, **f64)
    infos, kept = [], []
    for b in folds.on(dev):
        blocks, Li, T = (gctx.batched_buffer(b.nf, b.mp) for _ in range(3))
        gctx.cv_blocks(Linv, b.idx, b.off, blocks)
        info = torch.zeros(b.nf, dtype=torch.int32, device=dev)
        gctx.potrf_batched(blocks, Li, info)
        gctx.trtri_batched(blocks, Li, T)
        del T
        r, z, na, d = (gctx.batched_vector(b.nf, b.mp) for _ in range(4))
        r.zero_()
        _flat(r)[b.pos] = alpha.index_select(0, b.gather)
        out3 = torch.empty(b.nf, 3, **f64)
        gctx.mll_reduce_batched(blocks, Li, r, z, out3)
        gctx.alpha_batched(Li, z, na)
        gctx.loo_scalars_batched(Li, r, None, d)
        a_full[b.gather] = -_flat(na).index_select(0, b.pos)
        d_full[b.gather] = _flat(d).index_select(0, b.pos)
        terms[b.fold_ids] = 0.5 * out3[:, 1] - 0.5 * out3[:, 0]
        infos.append((b, info))
        if keep_factors:
            kept.append((b, Li, z, na, out3))
    return a_full, d_full, terms, infos, kept


def _flat(v: torch.Tensor) -> torch.Tensor:
    """The (B, sv) allocation behind a ``batched_vector`` view, flattened: entry f * sv + a is element a of problem f."""
    B, n = v.shape
    return v.as_strided((B * v.stride(0),), (1,), v.storage_offset())


def check_infos(infos, folds: FoldIndex) -> None:
    """Raise ``NotPSDError`` naming the first fold whose block did not factor.  No jitter is retried on a fold block: a jittered
    P_FF has no meaning (the outer factorisation keeps the package's one jitter-retry driver)."""
    for b, info in infos:
        host = info.cpu().numpy()
        bad = np.flatnonzero(host)
        if bad.shape[0]:
            f = int(b.folds[int(bad[0])])
            raise NotPSDError(f"cross-validation: the block P_FF of fold {f} (label {int(folds.labels[f])}, {int(folds.sizes[f])} rows) is "
                              f"not positive definite (leading minor {int(host[bad[0]])})")


def fold_gradient_factors(b, Li: torch.Tensor, z: torch.Tensor, na: torch.Tensor, out3: torch.Tensor) -> torch.Tensor:
    """G_F = (Linv_F - c z a_F') / sqrt 2 with c = (sqrt(1 + quad) - 1) / quad (1/2 at quad = 0), so that G_F' G_F =
    (a_F a_F' + P_FF^-1) / 2 = dcv/dP_FF; element-wise on the bucket's batch, into a fresh batched buffer (Li's mirror is dropped)."""
    c = 1.0 / (torch.sqrt(1.0 + out3[:, 0]) + 1.0)  # = (sqrt(1 + quad) - 1) / quad without the division: 1/2 at quad = 0
    G = torch.empty((Li.shape[0], Li.shape[1], Li.stride(1)), dtype=Li.dtype, device=Li.device)[:, :, :Li.shape[2]]
    G.copy_(torch.tril(Li))
    # -c z a' = +c z (na)'
    G.add_((c[:, None] * z)[:, :, None] * na[:, None, :])
    G.mul_(1.0 / math.sqrt(2.0))
    return G
