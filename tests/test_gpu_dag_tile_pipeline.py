"""The ticket list's big tile (gpp_dag_f64 runs ``gemm_tile<2,64,64,0,16,2,2>`` with the pipelined clean loop) through the public
path, at the sizes where the list's tile forms differ (tests/dag_tile_cases.py): the factor and the inverse against the same call
with the list off — launches per product, whose kernels compute the same sums in another tile order — and the factor's bytes
against the hash recorded from the commit BEFORE the executor took the pipelined loop (tests/golden/dag_tile_pipeline_sha.json,
written by tools/dag_tile_sha.py): a tile's arithmetic depends neither on the work-group that runs it nor on how its loads are
scheduled, so the bytes must not move.

Tolerances are those of the list-against-launches comparisons in tests/test_gpu_kernels_r3.py: 1e-12 of the factor's largest entry,
1e-10 of the inverse's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dag_tile_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _list_on(gpu_ctx):
    """Both the cooperative panel and the list on (an earlier test's time-out recovery may have switched them off), put back after."""
    from gpplus_amd.backend import OPT_COOP_PANEL, OPT_DAG_SCHED

    was = (gpu_ctx.coop_panel, gpu_ctx.dag_sched)
    gpu_ctx.set_option(OPT_COOP_PANEL, 1)
    gpu_ctx.set_option(OPT_DAG_SCHED, 1)
    yield
    gpu_ctx.set_option(OPT_COOP_PANEL, int(was[0]))
    gpu_ctx.set_option(OPT_DAG_SCHED, int(was[1]))


@pytest.mark.parametrize("n", dc.SIZES)
def test_list_factor_and_inverse(gpu_ctx, n):
    A0, L0 = dc.factor_and_inverse(gpu_ctx, n, list_on=False)
    U0, X0 = torch.triu(A0), torch.tril(L0)
    del A0, L0
    A1, L1 = dc.factor_and_inverse(gpu_ctx, n, list_on=True)
    # the executor really ran, over this matrix, to the end of its list, with the whole inverse inside it, and nobody raised the
    # abort word (the status word, checked in factor_and_inverse, carries no time-out bits either)
    rows, inv_rows, ntasks, abort, tickets = dc.list_state(gpu_ctx)
    print(f"n={n}: list of {ntasks} tasks, inverse rows {inv_rows}, abort word {abort}, tickets taken {tickets}")
    assert rows == n and inv_rows == n
    assert abort == 0 and tickets >= ntasks > 0
    U1, X1 = torch.triu(A1), torch.tril(L1)
    du = float((U0 - U1).abs().max()) / float(U0.abs().max())
    dx = float((X0 - X1).abs().max()) / float(X0.abs().max())
    print(f"n={n}: list against launches: factor {du:.3e} (bound 1e-12), inverse {dx:.3e} (bound 1e-10)")
    assert du <= 1e-12
    assert dx <= 1e-10
    assert float((torch.triu(L1, 1) - X1.T.triu(1)).abs().max()) == 0.0  # the mirror is exact
    del U0, X0, U1, X1, L1
    sha = dc.factor_sha256(A1, n)
    print(f"n={n}: sha256 {sha}")
    assert sha == dc.golden()[n]
