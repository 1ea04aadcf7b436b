"""The jitter-retry policy of every factorisation in the package, in one place and free of launches: it restates
gpytorch.utils.cholesky.psd_safe_cholesky [3P] — try the matrix as it is, then with cholesky_jitter * 10^i on its diagonal for
i < cholesky_max_tries, warn when jitter was needed, raise ``NotPSDError`` when none sufficed, ``NanError`` for NaN/Inf inputs.
The callers keep what is theirs — the launches, their order, the wait for the status word — in an ``attempt(jitter)`` closure;
this module needs neither a GPU nor the library."""
from __future__ import annotations

import warnings
from typing import Callable, List, Optional

import torch

from . import settings
from .backend import INFO_PANEL_TIMEOUT, panel_timed_out
from .errors import NanError, NotPSDError

__all__ = ["jitter_schedule", "psd_safe", "inputs_nan_probe"]


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
