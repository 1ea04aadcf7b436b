"""Active learning by expected variance reduction: the next q runs of a simulator are the candidates whose observation most reduces
the emulator's posterior variance over a reference set (Cohn 1996, "ALC"; integrated mean squared error over the reference set).
The greedy batch of ``GP_Plus.variance_reduction``'s criterion.  No reference counterpart: the reference's acquisition functions
(AFs.py) serve optimisation, and scoring by refit costs a factorisation per candidate."""
from __future__ import annotations

from typing import Tuple

import torch

__all__ = ["select_by_variance_reduction", "select_run_by_variance_reduction"]


def select_by_variance_reduction(model, q: int, Xcand, Xref, weights=None, cost=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``q`` rows of ``Xcand`` picked greedily: each round takes the candidate with the largest expected reduction of the weighted
    posterior variance over ``Xref`` given the picks so far (with ``cost``, M_c positive numbers, the largest reduction per unit
    cost), then accounts for it — no value is observed and nothing is factorised, the posterior variance does not depend on the
    values.  Returns (indices into ``Xcand`` in pick order, the gains in y^2 units, undivided by the cost); the gains add up to the
    reduction ``model.condition_on`` of all q picks would give.  A multi-fidelity user passes candidates of several sources,
    reference rows of the high-fidelity source and the cost of each candidate's source.  ``ValueError`` for q < 1 or q > M_c and
    for everything ``variance_reduction`` refuses.  The loop it closes: score -> pick -> run -> ``condition_on`` -> score."""
    if int(q) < 1:
        raise ValueError(f"select_by_variance_reduction: q must be at least 1 (got {q})")
    _, picks, gains = model._variance_reduction(Xcand, Xref, weights, q=int(q), cost=cost)
    return picks, gains


def _run_cost(cost, name: str, Mc: int) -> torch.Tensor:
    c = torch.as_tensor(cost, dtype=torch.float64).detach().cpu().reshape(-1)
    if c.numel() not in (1, Mc):
        raise ValueError(f"select_run_by_variance_reduction: {name} must be a scalar or one cost per candidate ({Mc}); got {c.numel()}")
    if not bool(torch.isfinite(c).all()) or bool((c <= 0).any()):
        raise ValueError(f"select_run_by_variance_reduction: {name} must be finite and positive")
    return c.expand(Mc)


def select_run_by_variance_reduction(model_or_posterior, Xcand, Xref, weights=None, gradient=True, cost_value=1.0,
                                     cost_gradient=2.0) -> Tuple[int, bool, torch.Tensor]:
    """The next run of a simulator that can also return gradients (an adjoint solver): ONE pick among the rows of ``Xcand`` and the
    two run types, by the largest expected variance reduction over ``Xref`` per unit cost.  ``model_or_posterior``: a fitted
    ``GP_Plus`` or a ``GradientEnhancedPosterior``; ``gradient``: True or the length-p bool mask of the components a gradient run
    returns (``variance_reduction``'s argument; the default gradient noise); ``cost_value`` / ``cost_gradient``: the cost of a run
    that returns y alone and of one that returns y and the gradient, scalars or M_c-vectors, positive.  Returns (the index into
    ``Xcand``, whether the pick is a gradient run, the gains (M_c, 2) in y^2 units, undivided: column 0 the value alone, column 1 with
    the gradient).  Ties go to the cheaper run type, then to the lower index.  The loop it closes: score -> pick -> run ->
    ``condition_on`` (and ``condition_on_gradients``) -> score.  ``ValueError`` for costs that are not positive or of another length
    and for everything ``variance_reduction`` refuses.  Greedy batches of gradient runs are out of scope."""
    if gradient is None:
        raise ValueError("select_run_by_variance_reduction: gradient must be True or a bool mask (for runs that return y alone use "
                         "select_by_variance_reduction)")
    Mc = int(Xcand.shape[0]) if hasattr(Xcand, "shape") and len(Xcand.shape) > 0 else 0
    cv, cg = _run_cost(cost_value, "cost_value", max(Mc, 1)), _run_cost(cost_gradient, "cost_gradient", max(Mc, 1))
    with_g, value = model_or_posterior.variance_reduction(Xcand, Xref, weights=weights, gradient=gradient)
    gains = torch.stack([value, with_g], 1)
    rank = gains / torch.stack([cv, cg], 1).to(gains.device)
    best = int(torch.argmax(rank.T.reshape(-1)))  # (type-major: a tie goes to the value run, then to the lower index)
    return best % Mc, best >= Mc, gains
