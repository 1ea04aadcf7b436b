"""The batched leave-one-out objective (batched.batched_loo: gpp_loo_scalars_batched, gpp_sym_rowscale_batched, the batched TN GEMM,
gpp_loo_grad_reduce_batched), the drivers on top of it (optim.BatchedObjective / fit_model_torch_batched with objective="loo", their
graph replay) and GP_Plus.fit(objective="loo"), against the dense fp64 CPU reference of tests/loo_reference.py, the eager path
(linalg.exact_loo) and the sequential driver.

Tolerances are the project's: 1e-5 relative for the value, 1e-5 of max|g| per gradient vector.  Every test
prints its observed errors before asserting (pytest -s shows them).
"""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loo_reference import KIND_MATERN52, KIND_RBF, loo_autograd, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-5
B = 5

# (N, D, kind, d_split, S, dU, shared U): one partial 64-tile with grp = None; across the 128-tile of sym_rowscale with feature
# gradients; odd N (padded row stride, the odd-column prologue of gpp_loo_rows); several tiles with sU = 0
CASES = [
    (63, 3, KIND_RBF, 0, 1, 0, True),
    (130, 4, KIND_MATERN52, 2, 2, 4, False),
    (301, 5, KIND_RBF, 0, 3, 2, False),
    (777, 8, KIND_MATERN52, 3, 3, 0, True),
]


def _element(inp, b):
    """Parameter set b of a case: the inputs of ``make_inputs`` with w, sf2, tau scaled and the mean shifted."""
    return dict(inp, w=inp["w"] * (0.6 + 0.2 * b), sf2=inp["sf2"] * (0.5 + 0.25 * b), tau=inp["tau"] * (1.0 + 0.5 * b),
                mean=inp["mean"] + 0.05 * b)


@functools.lru_cache(maxsize=None)
def _reference(N, D, kind, d_split, S):
    """The B parameter sets of one case and their autograd references, computed once and shared (read-only)."""
    inp = make_inputs(N, D, seed=2000 + N + D, S=S)
    elems = [_element(inp, b) for b in range(B)]
    return inp, elems, [loo_autograd(**e, kind=kind, d_split=d_split) for e in elems]


def _leaves(inp, elems, shared, need_grad=True, tau_override=None):
    N = inp["U"].shape[0]
    stack = lambda k: torch.stack([e[k] for e in elems])  # noqa: E731
    tau = stack("tau") if tau_override is None else tau_override
    t = dict(U=inp["U"].clone() if shared else inp["U"].repeat(len(elems), 1, 1), w=stack("w"), sf2=stack("sf2"), tau=tau,
             mean=stack("mean"), y=inp["y"].repeat(len(elems), 1))
    assert t["y"].shape == (len(elems), N)
    return {k: v.to("cuda").requires_grad_(need_grad) for k, v in t.items()}


def _evaluate(inp, elems, kind, d_split, dU, shared, need_grad=True, tau_override=None):
    """One batched_loo evaluation: (values (B,), gradients as CPU tensors with a leading batch dimension; U's only when per element)."""
    from gpplus_amd.batched import batched_loo

    lv = _leaves(inp, elems, shared, need_grad, tau_override)
    grp = None if inp["grp"] is None else inp["grp"].to("cuda")
    val = batched_loo(lv["U"], lv["w"], lv["sf2"], lv["tau"], lv["mean"], lv["y"], grp, kind, d_split, dU)
    if not need_grad:
        return val.detach().cpu(), None
    torch.nansum(val).backward()
    return val.detach().cpu(), {k: v.grad.detach().cpu() for k, v in lv.items()}


def _check_element(b, val, grads, ref_val, ref_grads, dU, shared, label):
    """Element b of a batched result against one reference (value, gradient dict): prints, then returns the list of violations."""
    bad = []
    err = abs(val[b].item() - ref_val.item()) / abs(ref_val.item())
    print(f"{label}[{b}]: value {val[b].item():.12f} ref {ref_val.item():.12f} rel err {err:.2e}")
    if not err <= RTOL:
        bad.append((label, b, "value", err))
    for name, ref in ref_grads.items():
        if name == "U":
            if shared or dU == 0:  # (a shared U carries the SUM of the elements' gradients; the shared cases ask for none)
                assert torch.count_nonzero(grads["U"]) == 0
                continue
            got = grads["U"][b]
            assert torch.count_nonzero(got[:, dU:]) == 0  # only the leading dU feature columns carry a gradient
            got, ref = got[:, :dU], ref[:, :dU]
        else:
            got = grads[name][b].reshape(ref.shape)
        e, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        print(f"{label}[{b}]: d{name}: max err {e:.3e} of max|g| {scale:.3e} ({e / scale:.2e})")
        if not e <= RTOL * scale:
            bad.append((label, b, name, e, scale))
    return bad


def _eager(elem, grp, kind, d_split, dU):
    """linalg.exact_loo on one element alone: (value, gradients) as CPU tensors."""
    from gpplus_amd.linalg import KernelSpec, exact_loo

    lv = {k: elem[k].to("cuda").requires_grad_(True) for k in ("U", "w", "sf2", "tau", "mean", "y")}
    val = exact_loo(lv["U"], KernelSpec(lv["w"], lv["sf2"], kind, d_split), lv["tau"], lv["mean"], lv["y"], grp, n_grad_dims=dU)
    val.backward()
    return val.detach().cpu(), {k: v.grad.detach().cpu() for k, v in lv.items()}


@pytest.mark.parametrize("N,D,kind,d_split,S,dU,shared", CASES)
def test_batched_loo_matches_autograd_and_the_eager_path(gpu_ctx, N, D, kind, d_split, S, dU, shared):
    """Test 1: every element's value and gradients (w, sf2, tau, mean, y, U[:, :dU]) against autograd through the dense inverse (the
    hard assertion) and against linalg.exact_loo on that element alone (printed: rounding level, the batched path factors in leaf
    steps)."""
    inp, elems, refs = _reference(N, D, kind, d_split, S)
    label = f"N={N} D={D} kind={kind} S={S} dU={dU}"
    val, grads = _evaluate(inp, elems, kind, d_split, dU, shared)
    bad = []
    for b in range(B):
        bad += _check_element(b, val, grads, *refs[b], dU, shared, label)
    grp = None if inp["grp"] is None else inp["grp"].to("cuda")
    worst = 0.0
    for b in range(B):
        v1, g1 = _eager(elems[b], grp, kind, d_split, dU)
        dv = abs(val[b].item() - v1.item()) / abs(v1.item())
        worst = max(worst, dv)
        for name in ("w", "sf2", "tau", "mean", "y") + (("U",) if not shared and dU > 0 else ()):
            a, e = grads[name][b].reshape(g1[name].shape), g1[name]
            worst = max(worst, (a - e).abs().max().item() / e.abs().max().item())
    print(f"{label}: batched against linalg.exact_loo, largest difference (value relative, gradients of max|g|): {worst:.2e}")
    assert not bad, bad


@pytest.mark.parametrize("N", [1, 64, 65, 200])
def test_batched_entry_points_equal_the_single_problem_ones_bitwise(gpu_ctx, N):
    """Test 2: gpp_loo_scalars_batched and gpp_sym_rowscale_batched alone at B = 3 against the single-problem entry points on each
    element (same arithmetic, same order: bitwise), and nothing outside an element's [0, N) x [0, N) / [0, N) is written."""
    from gpplus_amd.backend import row_stride, square_buffer

    nb, ld, sv = 3, row_stride(N), N + (N & 1)
    rng = np.random.default_rng(40 + N)
    dev = "cuda"
    nan = float("nan")

    # -- loo_scalars --------------------------------------------------------------------------------------------------------
    Li_base = torch.full((nb, N, ld), nan, dtype=torch.float64, device=dev)
    Li = Li_base[:, :, :N]
    M = rng.standard_normal((nb, N, N)) + 2.0 * np.eye(N)
    Li.copy_(torch.from_numpy(np.where(np.triu(np.ones((N, N), dtype=bool)), M, np.nan)))  # nothing below the diagonal is read
    vec_in = lambda a: torch.from_numpy(np.pad(a, ((0, 0), (0, sv - N)), constant_values=np.nan)).to(dev)[:, :N]  # noqa: E731
    alpha, y = vec_in(rng.standard_normal((nb, N))), vec_in(rng.standard_normal((nb, N)))
    bases = [torch.full((nb, sv), nan, dtype=torch.float64, device=dev) for _ in range(5)]
    d, mu, s2, a, sb = (t[:, :N] for t in bases)
    val_base = torch.full((nb + 2,), nan, dtype=torch.float64, device=dev)
    gpu_ctx.loo_scalars_batched(Li, alpha, y, d, mu=mu, s2=s2, a=a, sqrtb=sb, loo=val_base[:nb])
    assert bool(torch.isnan(val_base[nb:]).all())
    for t in bases:
        assert bool(torch.isnan(t[:, N:]).all()) and bool(torch.isfinite(t[:, :N]).all())
    for b in range(nb):
        one = [torch.empty(N, dtype=torch.float64, device=dev) for _ in range(5)]
        v1 = torch.empty(1, dtype=torch.float64, device=dev)
        gpu_ctx.loo_scalars(Li[b], alpha[b].contiguous(), y[b].contiguous(), one[0], mu=one[1], s2=one[2], a=one[3], sqrtb=one[4],
                            loo=v1)
        for name, got, want in zip(("d", "mu", "s2", "a", "sqrtb"), (d, mu, s2, a, sb), one):
            assert torch.equal(got[b], want), (name, b)
        assert torch.equal(val_base[b:b + 1], v1), b
    # y = None (the training path): the same d, a, sqrtb and value
    bases2 = [torch.full((nb, sv), nan, dtype=torch.float64, device=dev) for _ in range(3)]
    val2 = torch.empty(nb, dtype=torch.float64, device=dev)
    gpu_ctx.loo_scalars_batched(Li, alpha, None, bases2[0][:, :N], a=bases2[1][:, :N], sqrtb=bases2[2][:, :N], loo=val2)
    for got, want in zip(bases2, (bases[0], bases[3], bases[4])):
        assert torch.equal(got[:, :N], want[:, :N]) and bool(torch.isnan(got[:, N:]).all())
    assert torch.equal(val2, val_base[:nb])

    # -- sym_rowscale -------------------------------------------------------------------------------------------------------
    A = rng.standard_normal((nb, N, N))
    s = rng.uniform(0.5, 2.0, (nb, N))
    Ki_base = torch.full((nb, N, ld), nan, dtype=torch.float64, device=dev)
    Ki = Ki_base[:, :, :N]
    Ki.copy_(torch.from_numpy(np.where(np.tril(np.ones((N, N), dtype=bool)), A, np.nan)))  # nothing above the diagonal is read
    sd = vec_in(s)
    out_base = torch.full((nb, N, ld), nan, dtype=torch.float64, device=dev)
    out = out_base[:, :, :N]
    gpu_ctx.sym_rowscale_batched(Ki, sd, out)
    assert bool(torch.isnan(out_base[:, :, N:]).all())  # row slack untouched
    for b in range(nb):
        one = square_buffer(N, dev)
        one.fill_(nan)
        gpu_ctx.sym_rowscale(Ki[b], sd[b].contiguous(), one)
        assert torch.equal(out[b], one), b
        sym = np.tril(A[b]) + np.tril(A[b], -1).T
        assert np.array_equal(out[b].cpu().numpy(), s[b][:, None] * sym)  # one multiplication per entry: exact


def test_batched_loo_is_bitwise_repeatable(gpu_ctx):
    """Test 3: two calls on the same inputs agree bit for bit in the value and every gradient, and the value does not depend on
    whether a gradient was asked for."""
    N, D, kind, d_split, S, dU, shared = CASES[2]
    inp, elems, _ = _reference(N, D, kind, d_split, S)
    v1, g1 = _evaluate(inp, elems, kind, d_split, dU, shared)
    v2, g2 = _evaluate(inp, elems, kind, d_split, dU, shared)
    v3, _ = _evaluate(inp, elems, kind, d_split, dU, shared, need_grad=False)
    print(f"repeat: max |dv| {float((v1 - v2).abs().max()):.1e}, without a gradient {float((v1 - v3).abs().max()):.1e}")
    assert torch.equal(v1, v2) and torch.equal(v1, v3)
    for name in g1:
        assert torch.equal(g1[name], g2[name]), name


def test_one_bad_element_returns_nan_and_leaves_the_others_alone(gpu_ctx):
    """Test 4: element 2 with a negative "noise" is not positive definite under the whole jitter schedule: NaN, all-zero gradients;
    the other elements still meet the tolerance of test 1."""
    N, D, kind, d_split, S, dU, shared = CASES[2]
    inp, elems, refs = _reference(N, D, kind, d_split, S)
    tau = torch.stack([e["tau"] for e in elems])
    tau[2] = -5.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        val, grads = _evaluate(inp, elems, kind, d_split, dU, shared, tau_override=tau)
    print("values with element 2 indefinite:", val.tolist())
    assert bool(torch.isnan(val[2])) and bool(torch.isfinite(val[[0, 1, 3, 4]]).all())
    for name, g in grads.items():
        assert float(g[2].abs().max()) == 0.0, name
    bad = []
    for b in (0, 1, 3, 4):
        bad += _check_element(b, val, grads, *refs[b], dU, shared, "one bad element")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _toy_model(kind, n=260, seed=0):
    """The small models of tests/test_gpu_model.py: plain, mixed (a categorical input through the latent map), multi-fidelity."""
    from gpplus_amd.models import GP_Plus

    rng = np.random.default_rng(seed)
    if kind == "plain":
        X = rng.uniform(0, 1, (n, 4))
        y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2
        return GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cuda")
    X = np.stack([rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.integers(0, 3, n).astype(float)], 1)
    y = np.sin(3 * X[:, 0]) + X[:, 1] + 0.3 * X[:, 2]
    kw = dict(multiple_noise=True, m_gp="multiple_constant") if kind == "multi_fidelity" else {}
    return GP_Plus(torch.tensor(X), torch.tensor(y), qual_dict={2: 3}, dtype=torch.float64, device="cuda", **kw)


@pytest.mark.parametrize("kind", ["plain", "mixed", "multi_fidelity"])
def test_batched_loo_objective_matches_the_model(gpu_ctx, kind):
    """Test 5: optim.BatchedObjective(m, 5, objective="loo") against LeaveOneOutPseudoLikelihood evaluated run by run: the loss and
    every parameter gradient."""
    from gpplus_amd.gpcore import LeaveOneOutPseudoLikelihood
    from gpplus_amd.optim import BatchedObjective
    from gpplus_amd.utils import set_seed

    set_seed(1)
    m = _toy_model(kind)
    obj = BatchedObjective(m, B, objective="loo")
    obj.sample_restarts()
    loss = obj.loss()
    loss.sum().backward()
    loo = LeaveOneOutPseudoLikelihood(m.likelihood, m)
    bad, worst_v, worst_g = [], 0.0, 0.0
    for b in range(B):
        st = m.state_dict()
        st.update(obj.row(b))
        m.load_state_dict(st)
        m.train()
        for p in m.parameters():
            p.grad = None
        one = -loo(m(*m.train_inputs), m.train_targets)
        one.backward()
        ev = abs(one.item() - loss[b].item()) / abs(one.item())
        worst_v = max(worst_v, ev)
        if not ev <= RTOL:
            bad.append((b, "loss", ev))
        for name, p in m.named_parameters():
            if p.requires_grad:
                e = (obj.theta[name].grad[b] - p.grad).abs().max().item()
                scale = p.grad.abs().max().item()
                worst_g = max(worst_g, e / scale)
                if not e <= RTOL * scale:
                    bad.append((b, name, e, scale))
    print(f"{kind}: batched LOO objective against the model run by run: loss rel {worst_v:.2e}, gradients of max|g| {worst_g:.2e}")
    assert not bad, bad


def _fit_pair_model():
    from gpplus_amd.utils import set_seed

    set_seed(5)
    return _toy_model("mixed", n=200, seed=3)


def test_fit_model_torch_batched_loo_follows_the_sequential_driver(gpu_ctx):
    """Test 6: the same starts, the same Adam trajectories and the same winner as fit_model_torch(objective="loo")."""
    from gpplus_amd.optim import fit_model_torch, fit_model_torch_batched
    from gpplus_amd.utils import set_seed

    ma, mb = _fit_pair_model(), _fit_pair_model()
    set_seed(9)
    fa, ha = fit_model_torch(ma, num_restarts=3, num_iter=30, verbose=False, objective="loo")
    set_seed(9)
    fb, hb = fit_model_torch_batched(mb, num_restarts=3, num_iter=30, objective="loo")
    assert len(ha) == len(hb) == 4 and [len(h) for h in ha] == [len(h) for h in hb]
    dev = max(abs(x - y_) / abs(x) for a, b in zip(ha, hb) for x, y_ in zip(a, b))
    wa, wb = int(np.argmin([h[-1] for h in ha])), int(np.argmin([h[-1] for h in hb]))
    print(f"batched against sequential LOO fit: largest relative deviation of a loss {dev:.2e}; winners {wa} / {wb}; "
          f"final loss {fa:.12f} / {fb:.12f} (rel {abs(fa - fb) / abs(fa):.2e})")
    assert dev <= RTOL
    assert wa == wb and abs(fa - fb) <= RTOL * abs(fa)


def test_batched_loo_replayed_graph_equals_the_eager_loop(gpu_ctx):
    """Test 7: the LOO step replayed as one HIP graph against the same launches issued eagerly: histories and final state bit for
    bit, every step served by the graph."""
    from gpplus_amd import settings
    from gpplus_amd.optim import fit_model_torch_batched
    from gpplus_amd.utils import set_seed

    def fit(on):
        m = _fit_pair_model()
        set_seed(9)
        with settings.graphed_objective(on):
            f, h = fit_model_torch_batched(m, num_restarts=3, num_iter=40, objective="loo")
        return f, h, m.state_dict(), fit_model_torch_batched.last_graph

    f1, h1, s1, g1 = fit(True)
    f0, h0, s0, g0 = fit(False)
    print(f"graphed LOO fit: {None if g1 is None else (g1.replays, g1.declined)} (replays, declined); final {f1!r} against eager {f0!r}")
    assert g0 is None and g1 is not None and g1.replays > 0 and g1.declined == 0
    assert f1 == f0 and h1 == h0
    for k, v in s0.items():
        if torch.is_tensor(v):
            assert torch.equal(s1[k], v), k


def test_gp_plus_fit_with_the_loo_objective_takes_the_batched_route(gpu_ctx):
    """Test 8: GP_Plus.fit(objective="loo") on the mixed borehole fixture (N = 100): 65 restarts advancing together; and under
    settings.batched_restarts(False) the sequential, eager loop."""
    from gpplus_amd import settings
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import fit_model_torch, fit_model_torch_batched
    from gpplus_amd.utils import set_seed

    fx = dict(np.load(os.path.join(GOLD, "c3_borehole_mixed_n100.npz")))

    def model():
        set_seed(2)
        X = fx["Xtrain" if "Xtrain" in fx else "Utrain"]
        return GP_Plus(torch.tensor(X), torch.tensor(fx["ytrain"]), qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cuda")

    m = model()
    fit_model_torch_batched.last_graph = fit_model_torch.last_graph = "untouched"
    out = m.fit(optim_type="adam_torch", objective="loo")
    assert isinstance(out, tuple) and len(out) == 2
    best, histories = out
    lens = [len(h) for h in histories]
    print(f"GP_Plus.fit(objective='loo'): {len(histories)} runs of {min(lens)}..{max(lens)} losses; start {histories[0][0]:.6f}, "
          f"best {best:.6f}; graph {fit_model_torch_batched.last_graph}")
    assert len(histories) == 65 and all(0 < n <= 100 for n in lens)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert np.isfinite(best) and best < histories[0][0]
    g = fit_model_torch_batched.last_graph
    assert g is not None and g != "untouched" and g.replays > 0  # the batched driver ran, its step replayed as a graph
    assert fit_model_torch.last_graph == "untouched"             # ... and the sequential one did not

    # the sequential route (any other optim_type: a warning and 4 restarts, as for the MLL)
    m = model()
    fit_model_torch_batched.last_graph = "untouched"
    with settings.batched_restarts(False), pytest.warns(UserWarning, match="adam_torch"):
        best_s, hist_s = m.fit(objective="loo")
    print(f"sequential: {len(hist_s)} runs, best {best_s:.6f}")
    assert len(hist_s) == 5 and np.isfinite(best_s)
    assert fit_model_torch.last_graph is None and fit_model_torch_batched.last_graph == "untouched"
