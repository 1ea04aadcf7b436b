"""The batched gradient-enhanced objective without a GPU: the three batched entry points' declarations, the drivers' argument errors
(raised before a device is touched) and the routing predicate of ``GP_Plus.fit(objective="gek")``, which is judged at the N + q rows of
the joint matrix."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradpost_reference as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: name -> number of arguments of its declaration in include/gpp.h
SYMBOLS = {"gpp_cross_kernel_dx_batched": 21, "gpp_kernel_dxdx_batched": 24, "gpp_gek_grad_reduce_batched": 28}


def test_the_three_symbols_are_declared_exported_and_bound():
    from gpplus_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    lib = _lib.load()
    for name, nargs in SYMBOLS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        assert name in _lib.exported_symbols()
        restype, argtypes = _lib._SIGNATURES[name]
        assert len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes == argtypes
    # the single-problem entry points keep their declarations
    for name, nargs in (("gpp_cross_kernel_dx", 14), ("gpp_kernel_dxdx", 14), ("gpp_gek_grad_reduce", 20)):
        assert len(_lib._SIGNATURES[name][1]) == nargs, name


def _cpu_model():
    from gpplus_amd.models import GP_Plus

    fx = gr.load_fixture("c3_borehole_mixed_n100.npz")
    X, y = gr.fixture_xy(fx, 30)
    return GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cpu", qual_dict={0: 5, 5: 5}), \
        gr.fixture_test_rows(fx, 3)


def test_the_batched_drivers_refuse_a_gek_fit_without_gradients_before_a_device_is_touched():
    from gpplus_amd.optim import BatchedObjective, fit_model_torch_batched

    m, xg = _cpu_model()
    with pytest.raises(ValueError, match="gradients"):
        fit_model_torch_batched(m, objective="gek")
    with pytest.raises(ValueError, match="gradients"):
        BatchedObjective(m, 2, "gek")
    with pytest.raises(ValueError, match="gek"):
        BatchedObjective(m, 2, "mll", gradients=(xg, torch.ones(3, int(m.quant_index.numel()), dtype=torch.float64)))
    # bad gradient data are a ValueError of the validation, on the host as well
    with pytest.raises(ValueError):
        fit_model_torch_batched(m, objective="gek", gradients=(xg[:, :-1], torch.ones(3, int(m.quant_index.numel()), dtype=torch.float64)))


def test_a_valid_objective_counts_the_gradient_observations():
    from gpplus_amd.optim import BatchedObjective

    m, xg = _cpu_model()
    p = int(m.quant_index.numel())
    dY = torch.ones(xg.shape[0], p, dtype=torch.float64)
    obj = BatchedObjective(m, 2, "gek", gradients=(xg, dY))
    assert obj.num_data == 30 + 3 * p and obj.gek is not None and obj.gek.selection is None
    observed = torch.zeros(3, p, dtype=torch.bool)
    observed[:, 0] = True
    obj = BatchedObjective(m, 2, "gek", gradients=(xg, dY, None, observed))
    assert obj.num_data == 30 + 3 and obj.gek.selection.q == 3
    assert BatchedObjective(m, 2, "mll").num_data == 30


def test_the_routing_predicate_is_judged_at_n_plus_q(monkeypatch):
    """A stub model with N <= BATCHED_MAX_N < N + q: batched by its N alone, sequential at the size of its joint matrix."""
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim.mll_batched import BATCHED_MAX_N

    N, q = 6000, 200
    assert N <= BATCHED_MAX_N < N + q
    stub = SimpleNamespace(train_targets=torch.zeros(N), calibration_id=[], tkwargs={"device": torch.device("cpu")})
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 50, 1 << 50))
    assert GP_Plus._restarts_fit_one_batch(stub, 65) is True
    assert GP_Plus._restarts_fit_one_batch(stub, 65, N) is True
    assert GP_Plus._restarts_fit_one_batch(stub, 65, N + q) is False
    # the memory bound is taken at that size too: three B x n x n buffers against a third of what is free
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (3 * 3 * 65 * 1008 * 1008 * 8, 1 << 50))
    assert GP_Plus._restarts_fit_one_batch(stub, 65, 1000) is True
    assert GP_Plus._restarts_fit_one_batch(stub, 65, 1100) is False
