"""Thompson sampling on pathwise posterior draws: the next q points of a Bayesian optimisation are the minimisers of q independent
draws of the posterior FUNCTION (Thompson 1933; for Gaussian processes by decoupled/pathwise sampling, Wilson et al. 2020).  No
reference counterpart: the reference's acquisition functions (AFs.py) score candidates on ``predict`` only."""
from __future__ import annotations

from typing import Dict, Optional

import torch

__all__ = ["thompson_sample"]


def thompson_sample(model, q: int, lower, upper, fixed: Optional[Dict[int, float]] = None, num_features: int = 2048,
                    generator: Optional[torch.Generator] = None, **minimize_kw) -> torch.Tensor:
    """``q`` points (q x p, on the model's device) inside the box [lower, upper], each the minimiser of its own posterior draw
    (the maximiser with ``maximize=True``): ``model.sample_paths(q, ...).minimize(...).x``.  ``fixed`` gives the values of the
    categorical and source columns; ``generator`` (a CPU ``torch.Generator``) seeds the draws and the candidate points; further
    keywords go to :meth:`~gpplus_amd.pathwise.PosteriorPaths.minimize`.  The draws live in the model's scaled target space, as
    ``sample_y``'s do."""
    paths = model.sample_paths(size=int(q), num_features=num_features, generator=generator)
    return paths.minimize(lower, upper, fixed=fixed, generator=generator, **minimize_kw).x
