"""The batched leave-one-out objective, the parts that need no GPU: the three entry points are declared and bound, and the batched
driver validates its ``objective`` before it touches a device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("gpp_loo_scalars_batched", "gpp_sym_rowscale_batched", "gpp_loo_grad_reduce_batched")


def test_batched_loo_entry_points_are_declared_and_bound():
    from gpplus_amd import _lib

    with open(os.path.join(ROOT, "include", "gpp.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib._SIGNATURES and hasattr(lib, name), name
    # the argument counts of the bindings are those of the declarations
    for name in SYMBOLS:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_context_has_the_batched_loo_wrappers():
    from gpplus_amd.backend import GppContext

    for name in ("loo_scalars_batched", "sym_rowscale_batched", "loo_grad_reduce_batched"):
        assert callable(getattr(GppContext, name)), name


def test_batched_module_exports_the_loo_function():
    from gpplus_amd import batched

    assert "BatchedLOOFunction" in batched.__all__ and "batched_loo" in batched.__all__
    assert issubclass(batched.BatchedLOOFunction, torch.autograd.Function) and callable(batched.batched_loo)


def test_batched_driver_rejects_an_unknown_objective_before_touching_a_device():
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import BatchedObjective, fit_model_torch_batched

    fx = dict(np.load(os.path.join(GOLD, "c1_borehole_n500.npz")))
    m = GP_Plus(torch.tensor(fx["Xtrain"][:40]), torch.tensor(fx["ytrain"][:40]), dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="objective"):
        fit_model_torch_batched(m, num_iter=1, objective="loocv")
    with pytest.raises(ValueError, match="objective"):
        BatchedObjective(m, 2, objective="loocv")
    assert BatchedObjective(m, 2).objective == "mll" and BatchedObjective(m, 2, objective="loo").objective == "loo"
