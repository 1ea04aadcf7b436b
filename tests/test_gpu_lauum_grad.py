"""``gpp_lauum_grad``: the LAUUM whose epilogue is the gradient reduction, against an extended-precision host evaluation.

The yardstick is the existing ``gpp_lauum`` + ``gpp_grad_reduce`` pair's OWN error against the same reference on the same inputs:
the fused sums regroup the same terms by 128 x 128 tiles and nothing else, so each output's error may be at most 4 x the pair's,
with a floor of 64 eps x sum |terms| (taken from the reference) where the pair happens to land closer than that."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _sq(n):
    from gpplus_amd.backend import square_buffer

    m = square_buffer(n, "cuda")
    m.fill_(float("nan"))
    return m


@functools.lru_cache(maxsize=None)
def _matrix(n):
    """Well-scaled lower-triangular Linv (entries ~ 1/sqrt(n)), alpha, and Ky^-1 = Linv^T Linv in long double."""
    rng = np.random.default_rng(1000 + n)
    L = np.tril(rng.standard_normal((n, n))) / np.sqrt(n)
    L[np.diag_indices(n)] = rng.uniform(0.5, 1.5, n)
    alpha = rng.standard_normal(n)
    Ll = L.astype(LD)
    Kinv = Ll.T @ Ll
    W = 0.5 * (np.outer(alpha.astype(LD), alpha.astype(LD)) - Kinv)
    return L, alpha, W


@functools.lru_cache(maxsize=None)
def _case(n, d, S):
    """Inputs and the long-double reference of the three sums gpp_grad_tiles documents (lower triangle, mult = 2 below the
    diagonal), each with the sum of its terms' magnitudes."""
    L, alpha, W = _matrix(n)
    rng = np.random.default_rng(7 * n + 31 * d + S)
    U = rng.standard_normal((n, d))
    w = rng.uniform(0.05, 0.6, d)
    sf2 = float(rng.uniform(0.5, 1.5))
    grp = rng.permutation(np.arange(n) % S).astype(np.int32)  # scattered labels, every group present
    Ul, wl = U.astype(LD), w.astype(LD)
    diff2 = (Ul[:, None, :] - Ul[None, :, :]) ** 2
    k = np.exp(-(diff2 * wl).sum(-1))
    mult = np.tril(np.full((n, n), 2.0, dtype=LD), -1) + np.eye(n, dtype=LD)
    G = mult * W * k
    ref, mag = [], []
    for q in range(d):
        t = G * LD(sf2) * (-diff2[:, :, q])
        ref.append(t.sum())
        mag.append(np.abs(t).sum())
    ref.append(G.sum())
    mag.append(np.abs(G).sum())
    Wd = np.diag(W)
    for s in range(S):
        ref.append(Wd[grp == s].sum())
        mag.append(np.abs(Wd[grp == s]).sum())
    return L, alpha, U, w, sf2, grp, np.array(ref, dtype=LD), np.array(mag, dtype=LD)


def _device_inputs(n, d, S):
    L, alpha, U, w, sf2, grp, ref, mag = _case(n, d, S)
    Li = _sq(n)
    Li.copy_(_dev(L + np.tril(L, -1).T))  # the inverse factor with its mirror, as gpp_trtri leaves it
    return dict(Li=Li, U=_dev(U), w=_dev(w), sf2=torch.tensor([sf2], dtype=torch.float64, device="cuda"), grp=_dev(grp),
                alpha=_dev(alpha)), ref, mag


def _outs(d, S):
    return [torch.full((k,), float("nan"), dtype=torch.float64, device="cuda") for k in (d, 1, S)]


def _flat(outs):
    return np.concatenate([o.cpu().numpy() for o in outs]).astype(LD)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("d", [1, 8, 16])
@pytest.mark.parametrize("n", [129, 300, 640])
def test_fused_against_long_double(gpu_ctx, n, d, S):
    x, ref, mag = _device_inputs(n, d, S)
    fused = _outs(d, S)
    assert gpu_ctx.lauum_grad(x["Li"], x["U"], x["w"], x["sf2"], x["grp"], S, x["alpha"], 0, *fused)
    again = _outs(d, S)
    assert gpu_ctx.lauum_grad(x["Li"], x["U"], x["w"], x["sf2"], x["grp"], S, x["alpha"], 0, *again)
    for a, b in zip(fused, again):
        assert torch.equal(a, b), "two fused launches must agree bitwise"

    Ki = _sq(n)
    gpu_ctx.lauum(x["Li"], Ki)
    pair = _outs(d, S)
    gpu_ctx.grad_reduce(x["U"], x["w"], x["sf2"], x["grp"], S, x["alpha"], Ki, 0, *pair, None)

    e_fused = np.abs(_flat(fused) - ref)
    e_pair = np.abs(_flat(pair) - ref)
    floor = 64 * EPS * mag
    bound = np.maximum(4 * e_pair, floor)
    names = [f"g_w[{q}]" for q in range(d)] + ["g_sf2"] + [f"g_tau[{s}]" for s in range(S)]
    ratio = e_fused / np.maximum(e_pair, LD(1e-300))
    print(f"n={n} d={d} S={S}: max fused/pair error ratio {float(ratio.max()):.3g}, "
          f"max fused error / (eps * sum|terms|) {float((e_fused / (EPS * mag)).max()):.3g}, "
          f"pair {float((e_pair / (EPS * mag)).max()):.3g}")
    bad = [(names[i], float(e_fused[i]), float(e_pair[i]), float(floor[i])) for i in range(len(names)) if not e_fused[i] <= bound[i]]
    assert not bad, bad


def test_not_supported_cases(gpu_ctx):
    """Matern kinds, D = 17 and feature gradients return the not-supported code: nothing is enqueued, the outputs keep their bits."""
    from gpplus_amd.backend import KIND_MATERN32, KIND_MATERN52

    n = 300
    for d, kind, dU in ((8, KIND_MATERN32, 0), (8, KIND_MATERN52, 0), (17, 0, 0), (8, 0, 1)):
        rng = np.random.default_rng(d)
        x, _, _ = _device_inputs(n, 8, 1)
        U = _dev(rng.standard_normal((n, d)))
        w = _dev(rng.uniform(0.1, 0.5, d))
        outs = _outs(d, 1)
        assert gpu_ctx.lauum_grad(x["Li"], U, w, x["sf2"], x["grp"], 1, x["alpha"], dU, *outs, kind=kind) is False
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)


def _mll_grads(n, d, kind, d_split, grad_U, seed=0):
    from gpplus_amd.linalg import KernelSpec, exact_mll

    g = torch.Generator(device="cpu").manual_seed(seed)
    U = torch.rand(n, d, generator=g, dtype=torch.float64).cuda().requires_grad_(grad_U)
    w = torch.full((d,), 2.0 / d, dtype=torch.float64, device="cuda").requires_grad_(True)
    sf2 = torch.tensor(0.9, dtype=torch.float64, device="cuda").requires_grad_(True)
    tau = torch.tensor([1e-2, 3e-2], dtype=torch.float64, device="cuda").requires_grad_(True)
    mean = torch.zeros(n, dtype=torch.float64, device="cuda")
    y = torch.sin(3.0 * U.detach().sum(1))
    grp = (torch.arange(n, device="cuda") % 2).to(torch.int32)
    loss = exact_mll(U, KernelSpec(w, sf2, kind, d_split), tau, mean, y, grp)
    loss.backward()
    out = [loss.detach().clone(), w.grad.clone(), sf2.grad.clone(), tau.grad.clone()]
    if grad_U:
        out.append(U.grad.clone())
    return out


@pytest.mark.parametrize("d,kind,d_split,grad_U", [(4, 1, 2, False), (17, 0, 0, False), (4, 0, 0, True)])
def test_dispatch_keeps_unsupported_cases_bitwise(monkeypatch, gpu_ctx, d, kind, d_split, grad_U):
    """Above the dispatcher's threshold the cases the fused entry does not take give the numbers of the lauum + grad_reduce pair."""
    from gpplus_amd import linalg

    n = linalg.FUSED_GRAD_MIN_N + 128
    got = _mll_grads(n, d, kind, d_split, grad_U)
    monkeypatch.setattr(linalg, "FUSED_GRAD_MIN_N", 10 ** 9)  # the pair, unconditionally
    want = _mll_grads(n, d, kind, d_split, grad_U)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_dispatch_takes_the_fused_entry(monkeypatch, gpu_ctx):
    """RBF, D <= 16, no feature gradients above the threshold: the fused entry runs (and says so), the loss keeps its bits and the
    gradients agree with the pair's to the accuracy of either."""
    from gpplus_amd import linalg

    n = linalg.FUSED_GRAD_MIN_N + 128
    taken = []
    real = type(gpu_ctx).lauum_grad

    def spy(self, *a, **k):
        r = real(self, *a, **k)
        taken.append(r)
        return r

    monkeypatch.setattr(type(gpu_ctx), "lauum_grad", spy)
    got = _mll_grads(n, 8, 0, 0, False)
    assert taken == [True]
    monkeypatch.setattr(linalg, "FUSED_GRAD_MIN_N", 10 ** 9)
    want = _mll_grads(n, 8, 0, 0, False)
    assert taken == [True]
    assert torch.equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):  # (test_gpu_kernels.py's tolerances for gpp_grad_reduce; the accuracy test is the one above)
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7 * float(b.abs().max()) + 1e-12)
