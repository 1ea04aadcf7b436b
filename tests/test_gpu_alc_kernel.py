"""gpp_post_cross_sq alone on the GPU: out[c] = sum_r omega_r (sf2 k(Uc_c, Ur_r) - Vc_c . Vr_r)^2 on random V of realistic magnitude,
against long double under a DERIVED bound, bitwise repeatability, row independence, and what the binding and the C entry refuse.

Bound.  Per entry the computed cross-covariance errs by at most e = gemm_reference.error_bound(Vc, Vr^T) + kernel_gen_error (the
product in any summation order plus the generator), and the subtraction, the square, the weight and the M_r-term sum in any order cost
at most (M_r + 4) 2^-53 of sum_r omega_r c^2 (2 u for the rounded difference entering a square, u each for the square and the
weight's fma, (M_r - 1) u for the sum, first order):
    |out - ref| <= sum_r omega_r (2 |c| e + e^2) + (M_r + 4) 2^-53 sum_r omega_r c^2.
Every case prints observed / bound before it asserts (pytest -s)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402
from pathwise_reference import kernel_gen_error, kernel_matrix  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = LD(2.0) ** -53
MCS, MRS, KS, DS, KINDS = (1, 127, 129, 300), (1, 128, 257), (1, 15, 17, 130), (1, 8, 64), (0, 1, 2)


def _cases():
    """Every (M_c, M_r) pair twice, the other factors cycled so that every K, D, kind and omega mode meets every M_r (one, one full and
    three column tiles), every (kind, D) pair occurs, and the largest shape runs with K = 130 and D = 64."""
    out = []
    for (a, Mc), (b, Mr), rep in itertools.product(enumerate(MCS), enumerate(MRS), range(2)):
        out.append((Mc, Mr, KS[(a + 2 * rep + b) % 4], DS[(a + rep + b) % 3], KINDS[(a + 2 * rep + 2 * b) % 3], bool((a + rep) % 2)))
    for kind, D in itertools.product(KINDS, DS):
        if not any(c[4] == kind and c[3] == D for c in out):
            out.append((129, 257, 17, D, kind, True))
    out.append((300, 257, 130, 64, 2, True))
    return out


CASES = _cases()


def test_the_cases_cover_the_shapes():
    for vals, col in ((MCS, 0), (MRS, 1), (KS, 2), (DS, 3), (KINDS, 4), ((False, True), 5)):
        assert {c[col] for c in CASES} == set(vals)
    assert {(c[0], c[1]) for c in CASES} == set(itertools.product(MCS, MRS))
    assert {(c[4], c[3]) for c in CASES} == set(itertools.product(KINDS, DS))
    for Mr in MRS:  # the finish order: every K and every omega mode with one, one full and three column tiles
        assert {c[2] for c in CASES if c[1] == Mr} == set(KS) and {c[5] for c in CASES if c[1] == Mr} == {False, True}


class _Problem:
    """Operands on the host (float64) and on the device: V in buffers with leading dimension K + 6 rounded to even and NaN behind
    column K; ``vt``: the transposed operands (K x points, leading dimension points + 6 rounded to even, NaN behind)."""

    def __init__(self, Mc, Mr, K, D, kind, weighted, seed, vt=False):
        rng = np.random.default_rng(seed)
        self.Mc, self.Mr, self.K, self.D, self.kind, self.vt = Mc, Mr, K, D, kind, vt
        self.d_split = 0 if kind == 0 else D // 2
        self.Uc, self.Ur = rng.uniform(size=(Mc, D)), rng.uniform(size=(Mr, D))
        self.w = rng.uniform(0.5, 2.0, size=D) / D
        self.sf2 = 1.7
        # |v|^2 around 0.5 sf2: the posterior variance sf2 - |v|^2 of a point half explained by the data
        self.Vc = rng.standard_normal((Mc, K)) * np.sqrt(0.5 * self.sf2 / K)
        self.Vr = rng.standard_normal((Mr, K)) * np.sqrt(0.5 * self.sf2 / K)
        self.omega = rng.uniform(0.0, 2.0, size=Mr) if weighted else None

    def stored(self, V, dev):
        X = V.T if self.vt else V
        ld = X.shape[1] + 6 + (X.shape[1] & 1)
        buf = torch.full((X.shape[0], ld), float("nan"), dtype=torch.float64, device=dev)
        buf[:, :X.shape[1]] = torch.tensor(X)
        assert ld % 2 == 0 and buf.data_ptr() % 16 == 0
        return buf[:, :X.shape[1]]

    def run(self, ctx, out=None, **change):
        dev = ctx.device
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
        if out is None:
            out = torch.full((self.Mc + 3,), float("nan"), dtype=torch.float64, device=dev)
        args = dict(Uc=t(self.Uc), Ur=t(self.Ur), w=t(self.w), sf2=t([self.sf2]), Vc=self.stored(self.Vc, dev),
                    Vr=self.stored(self.Vr, dev), K=self.K, out=out, omega=None if self.omega is None else t(self.omega),
                    kind=self.kind, d_split=self.d_split, transposed=self.vt)
        args.update(change)
        ctx.post_cross_sq(**args)
        torch.cuda.synchronize()
        return out

    def reference(self):
        om = np.ones(self.Mr, dtype=LD) if self.omega is None else self.omega.astype(LD)
        G = kernel_matrix(self.Uc, self.Ur, self.w, self.sf2, self.kind, self.d_split)
        c = G - self.Vc.astype(LD) @ self.Vr.astype(LD).T
        e = gr.error_bound(self.Vc, self.Vr.T, 0, 0, 1.0, 0.0, np.zeros((self.Mc, self.Mr))) + \
            kernel_gen_error(self.Uc, self.Ur, self.w, self.sf2, self.kind, self.d_split)
        ref = (c * c) @ om
        bound = (2 * np.abs(c) * e + e * e) @ om + (self.Mr + 4) * U53 * ref
        return ref, bound


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


@pytest.mark.parametrize("Mc,Mr,K,D,kind,weighted", CASES)
def test_against_long_double_under_the_derived_bound(gpu_ctx, Mc, Mr, K, D, kind, weighted):
    P = _Problem(Mc, Mr, K, D, kind, weighted, seed=1000 + Mc + 7 * Mr + 13 * K + D + kind)
    out = P.run(gpu_ctx)
    ref, bound = P.reference()
    got = out[:Mc].cpu().numpy().astype(LD)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"Mc {Mc} Mr {Mr} K {K} D {D} kind {kind} omega {weighted}: observed / bound = {ratio:.3f} "
          f"(max relative error {float((np.abs(got - ref) / ref).max()):.2e})")
    assert bool(torch.isnan(out[Mc:]).all()), "written behind M_c"
    assert np.all(np.isfinite(got.astype(np.float64))) and ratio <= 1.0, ratio
    again = P.run(gpu_ctx)
    assert torch.equal(_bits(out[:Mc]), _bits(again[:Mc])), "two launches differ"


@pytest.mark.parametrize("K,D,kind", [(15, 8, 0), (130, 64, 2), (17, 1, 1)])
def test_transposed_operands_meet_the_same_bound(gpu_ctx, K, D, kind):
    P = _Problem(300, 257, K, D, kind, True, seed=77 + K, vt=True)
    out = P.run(gpu_ctx)
    ref, bound = P.reference()
    got = out[:300].cpu().numpy().astype(LD)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"transposed K {K} D {D} kind {kind}: observed / bound = {ratio:.3f}")
    assert bool(torch.isnan(out[300:]).all()) and ratio <= 1.0, ratio
    assert torch.equal(_bits(out[:300]), _bits(P.run(gpu_ctx)[:300]))


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("K,D,kind", [(130, 8, 0), (17, 64, 2)])
def test_a_candidate_scores_the_same_alone_and_at_another_row(gpu_ctx, K, D, kind, vt):
    P = _Problem(300, 257, K, D, kind, True, seed=5 + K, vt=vt)
    full = P.run(gpu_ctx)
    perm = np.random.default_rng(9).permutation(300)  # row i of the shuffled call is candidate perm[i]
    Q = _Problem(300, 257, K, D, kind, True, seed=5 + K, vt=vt)
    Q.Uc, Q.Vc = P.Uc[perm], P.Vc[perm]
    moved = Q.run(gpu_ctx)
    assert torch.equal(_bits(moved[:300]), _bits(full[:300][torch.tensor(perm)])), "the score depends on the row"
    for i in (0, 127, 128, 299):
        S = _Problem(1, 257, K, D, kind, True, seed=5 + K, vt=vt)
        S.Uc, S.Vc, S.Ur, S.Vr, S.w, S.omega = P.Uc[i:i + 1], P.Vc[i:i + 1], P.Ur, P.Vr, P.w, P.omega
        alone = S.run(gpu_ctx)
        assert torch.equal(_bits(alone[:1]), _bits(full[i:i + 1])), f"candidate {i} scores differently alone"


def test_binding_refuses_before_any_launch(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import NO_WORKSPACE, OP_POST_CROSS

    Mc, Mr, K = 129, 257, 17
    P = _Problem(Mc, Mr, K, 8, 1, True, seed=3)
    dev = gpu_ctx.device
    out = torch.full((Mc,), float("nan"), dtype=torch.float64, device=dev)
    odd = torch.zeros((Mc, K + 2), dtype=torch.float64, device=dev)[:, :K]           # leading dimension 19
    off = torch.zeros(Mc * (K + 1) + 1, dtype=torch.float64, device=dev)[1:].view(Mc, K + 1)[:, :K]  # 8 bytes off a 16-byte line
    assert odd.stride(0) % 2 == 1 and off.data_ptr() % 16 == 8 and off.stride(0) % 2 == 0
    bad = {"odd leading dimension": dict(Vc=odd), "misaligned": dict(Vc=off), "dtype": dict(Vc=torch.zeros((Mc, K + 1), dtype=torch.float32, device=dev)[:, :K]),
           "dtype of the features": dict(Uc=torch.zeros((Mc, 8), dtype=torch.float32, device=dev)),
           "short omega": dict(omega=torch.ones(Mr - 1, dtype=torch.float64, device=dev)),
           "short out": dict(out=out[:Mc - 1]), "rows of Vc": dict(Vc=P.stored(P.Vc, dev)[:Mc - 1]),
           "K beyond the operand": dict(K=K + 1)}
    for what, change in bad.items():
        with pytest.raises(GppError):
            P.run(gpu_ctx, **{"out": out, **change})
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # no workspace on the handle: the C entry point itself reports it and enqueues nothing
    lib, h = gpu_ctx.lib, gpu_ctx.h
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    Uc, Ur, w, sf2, om, Vc, Vr = t(P.Uc), t(P.Ur), t(P.w), t([P.sf2]), t(P.omega), P.stored(P.Vc, dev), P.stored(P.Vr, dev)
    need = lib.gpp_workspace_bytes(h, OP_POST_CROSS, Mr, Mc, 0, 0)
    small = torch.empty(need - 512, dtype=torch.uint8, device=dev)

    def raw():
        return lib.gpp_post_cross_sq(h, Uc.data_ptr(), Mc, Ur.data_ptr(), Mr, 8, w.data_ptr(), sf2.data_ptr(), 1, 4, Vc.data_ptr(),
                                     Vc.stride(0), Vr.data_ptr(), Vr.stride(0), K, 0, om.data_ptr(), out.data_ptr())
    try:
        assert lib.gpp_set_workspace(h, small.data_ptr(), small.numel()) == 0
        assert raw() == NO_WORKSPACE
        assert lib.gpp_set_workspace(h, None, 0) == 0
        assert raw() == NO_WORKSPACE
    finally:
        gpu_ctx._ws = None  # the context attaches a workspace of its own at the next call that needs one
        lib.gpp_set_workspace(h, None, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the C entry's own argument checks, and the same problem once the operands are right
    assert lib.gpp_post_cross_sq(h, Uc.data_ptr(), Mc, Ur.data_ptr(), Mr, 8, w.data_ptr(), sf2.data_ptr(), 1, 4, Vc.data_ptr(),
                                 Vc.stride(0) + 1, Vr.data_ptr(), Vr.stride(0), K, 0, om.data_ptr(), out.data_ptr()) == -11
    assert lib.gpp_post_cross_sq(h, Uc.data_ptr(), Mc, Ur.data_ptr(), Mr, 65, w.data_ptr(), sf2.data_ptr(), 1, 4, Vc.data_ptr(),
                                 Vc.stride(0), Vr.data_ptr(), Vr.stride(0), K, 0, om.data_ptr(), out.data_ptr()) == -6
    P.run(gpu_ctx, out=out)
    ref, bound = P.reference()
    assert float((np.abs(out.cpu().numpy().astype(LD) - ref) / bound).max()) <= 1.0
