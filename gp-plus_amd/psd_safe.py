"""The jitter-retry policy of every factorisation in the package, in one place and free of launches: it restates
gpytorch.utils.cholesky.psd_safe_cholesky [3P] — try the matrix as it is, then with cholesky_jitter * 10^i on its diagonal for
i < cholesky_max_tries, warn when jitter was needed, raise ``NotPSDError`` when none sufficed, ``NanError`` for NaN/Inf inputs.
``psd_safe_batched`` is the policy of the batched evaluations: per element, silent, NaN instead of an exception.
The callers keep what is theirs — the launches, their order, the wait for the status word — in an ``attempt(jitter)`` closure;
this module needs neither a GPU nor the library."""
from __future__ import annotations

import warnings
from typing import Callable, List, Optional, Tuple

import torch

from . import settings
from .backend import INFO_PANEL_TIMEOUT, panel_timed_out
from .errors import NanError, NotPSDError

__all__ = ["jitter_schedule", "psd_safe", "psd_safe_batched", "inputs_nan_probe"]


def jitter_schedule() -> List[float]:
    """[0, j, 10 j, ...]: the diagonal additions tried in turn (settings.cholesky_jitter, settings.cholesky_max_tries)."""
    return [0.0] + [settings.cholesky_jitter.value() * (10 ** i) for i in range(settings.cholesky_max_tries.value())]


def inputs_nan_probe(U, w, sf2, tau) -> Callable[[], None]:
    """The probe of an evaluation's inputs: raises ``NanError`` naming those that hold a NaN or an Inf."""
    def probe():
        bad = [n for n, t in (("inputs", U), ("weights", w), ("outputscale", sf2), ("noise", tau)) if not torch.isfinite(t).all()]
        if bad:
            raise NanError(f"cholesky: NaN/Inf in {', '.join(bad)} of the covariance")
    return probe


def psd_safe(ctx, attempt: Callable[[float], int], nan_probe: Optional[Callable[[], None]] = None,
             on_timeout: Callable = panel_timed_out) -> float:
    """Walk the schedule with ``attempt(jitter)``, which factors and returns the status word (0, LAPACK's failing leading minor,
    or a time-out status), and return the jitter that succeeded.  A time-out is not a statement about the matrix:
    ``on_timeout(ctx, info)`` answers it (the default switches the cooperative path that gave up off, or raises when there is none
    left to switch) and the same jitter is attempted again.  ``nan_probe()`` runs once, after a failure without jitter."""
    schedule = jitter_schedule()
    info = 0
    for jit in schedule:
        info = attempt(jit)
        while info >= INFO_PANEL_TIMEOUT:
            on_timeout(ctx, info)
            info = attempt(jit)
        if info == 0:
            if jit > 0:
                warnings.warn(f"A not p.d., added jitter of {jit:.1e} to the diagonal", RuntimeWarning)
            return jit
        if jit == 0.0 and nan_probe is not None:
            nan_probe()
    raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {schedule[-1]:.1e} "
                      f"(leading minor {info}).")


def psd_safe_batched(B: int, device, attempt: Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]):
    """The schedule for B problems factored together.  ``attempt(extra)`` factors all of them with ``extra`` ((B, 1) fp64 on
    ``device``, zero at first) added to each one's diagonal and returns the boolean mask ``ok`` (B,) on the device and the status
    words on the host, waited for.  An element that failed takes the schedule's next jitter, the others keep theirs; the walk ends
    when every host word is 0 or the schedule is spent.  No warning and no exception: the caller turns what is still failing into
    NaN (one bad restart must not stop the others).  Returns the last attempt's ``(ok, host words)``."""
    jitters = jitter_schedule()[1:]  # (the first attempt is the unjittered one)
    extra = torch.zeros(B, 1, dtype=torch.float64, device=device)
    for nxt in jitters + [None]:
        ok, info_host = attempt(extra)
        if nxt is None or bool((info_host == 0).all()):
            break
        extra = torch.where(ok.unsqueeze(1), extra, torch.full_like(extra, nxt))
    return ok, info_host
