"""gpp_post_cross_min alone on the GPU: out[c, k] = min_r (m_r + nodes_k scale_c (sf2 k(Uc_c, Ur_r) - Vc_c . Vr_r)) on random V of
realistic magnitude (tests/test_gpu_alc_kernel.py's operands), against long double under a DERIVED bound, the masking of the columns
beyond M_r, bitwise repeatability, independence of the candidate's row and of the ORDER of the reference rows, and what the binding and
the C entry refuse.

Bound.  Per entry the computed cross-covariance errs by at most e_cr = gemm_reference.error_bound(Vc, Vr^T) + kernel_gen_error (the
product in any summation order plus the generator).  The kernel rounds t_ck = nodes_k scale_c once (relative error u = 2^-53) and forms
fma(c, t, m_r) with one rounding of the result, |result| <= |m_r| + |t c|:
    |val - (m_r + t c_cr)| <= |t| e_cr + u |t c_cr| + u (|m_r| + |t c_cr|)        (first order)
and the minimum over r is exact and 1-Lipschitz in the sup norm, so
    |out[c, k] - ref[c, k]| <= max_r [ |t_ck| e_cr + u (2 |t_ck c_cr| + |m_r|) ].
Every case prints observed / bound before it asserts (pytest -s)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402
import kg_reference as kg  # noqa: E402
from pathwise_reference import kernel_gen_error, kernel_matrix  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = LD(2.0) ** -53
MCS, MRS, KS, DS, KINDS, QS = (1, 127, 129, 300), (1, 128, 257), (1, 15, 17, 130), (1, 8, 64), (0, 1, 2), (1, 2, 17, 64)


def _cases():
    """Every (M_c, M_r) pair; Q follows M_c, so every Q meets one, one full and three column tiles; K, D, kind and the operand form
    are cycled; then whatever (kind, D) pair is still missing, and the largest shape with K = 130, D = 64, Q = 64 in both forms."""
    out = []
    for (a, Mc), (b, Mr) in itertools.product(enumerate(MCS), enumerate(MRS)):
        out.append((Mc, Mr, KS[(a + b) % 4], DS[(a + b) % 3], KINDS[(a + 2 * b) % 3], QS[a], bool((a + b) % 2)))
    for kind, D in itertools.product(KINDS, DS):
        if not any(c[4] == kind and c[3] == D for c in out):
            out.append((129, 257, 17, D, kind, 17, D == 8))
    out += [(300, 257, 130, 64, 2, 64, False), (300, 257, 130, 64, 2, 64, True)]
    return out


CASES = _cases()


def test_the_cases_cover_the_shapes():
    for vals, col in ((MCS, 0), (MRS, 1), (KS, 2), (DS, 3), (KINDS, 4), (QS, 5), ((False, True), 6)):
        assert {c[col] for c in CASES} == set(vals)
    assert {(c[0], c[1]) for c in CASES} == set(itertools.product(MCS, MRS))
    assert {(c[4], c[3]) for c in CASES} == set(itertools.product(KINDS, DS))
    assert {(c[5], c[1]) for c in CASES} == set(itertools.product(QS, MRS))


class _Problem:
    """Operands on the host (float64) and on the device: V in buffers with leading dimension K + 6 rounded to even and NaN behind
    column K; ``vt``: the transposed operands (K x points, leading dimension points + 6 rounded to even, NaN behind)."""

    def __init__(self, Mc, Mr, K, D, kind, Q, seed, vt=False):
        rng = np.random.default_rng(seed)
        self.Mc, self.Mr, self.K, self.D, self.kind, self.Q, self.vt = Mc, Mr, K, D, kind, Q, vt
        self.d_split = 0 if kind == 0 else D // 2
        self.Uc, self.Ur = rng.uniform(size=(Mc, D)), rng.uniform(size=(Mr, D))
        self.w = rng.uniform(0.5, 2.0, size=D) / D
        self.sf2 = 1.7
        # |v|^2 around 0.5 sf2: the posterior variance sf2 - |v|^2 of a point half explained by the data
        self.Vc = rng.standard_normal((Mc, K)) * np.sqrt(0.5 * self.sf2 / K)
        self.Vr = rng.standard_normal((Mr, K)) * np.sqrt(0.5 * self.sf2 / K)
        self.m = rng.uniform(0.0, 1.0, size=Mr)  # shifted means: non-negative, the smallest one 0
        self.m -= self.m.min()
        self.scale = 1.0 / np.sqrt(rng.uniform(0.3, 1.5, size=Mc) * self.sf2)  # 1 / sqrt(s_c)
        self.nodes = kg.nodes(Q)[0].astype(np.float64)

    def stored(self, V, dev):
        X = V.T if self.vt else V
        ld = X.shape[1] + 6 + (X.shape[1] & 1)
        buf = torch.full((X.shape[0], ld), float("nan"), dtype=torch.float64, device=dev)
        buf[:, :X.shape[1]] = torch.tensor(X)
        assert ld % 2 == 0 and buf.data_ptr() % 16 == 0
        return buf[:, :X.shape[1]]

    def run(self, ctx, flat=None, **change):
        """Returns the flat output buffer: M_c Q results and 5 canaries behind them."""
        dev = ctx.device
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
        if flat is None:
            flat = torch.full((self.Mc * self.Q + 5,), float("nan"), dtype=torch.float64, device=dev)
        args = dict(Uc=t(self.Uc), Ur=t(self.Ur), w=t(self.w), sf2=t([self.sf2]), Vc=self.stored(self.Vc, dev),
                    Vr=self.stored(self.Vr, dev), K=self.K, m=t(self.m), scale=t(self.scale), nodes=t(self.nodes),
                    out=flat[:self.Mc * self.Q].view(self.Mc, self.Q), kind=self.kind, d_split=self.d_split, transposed=self.vt)
        args.update(change)
        ctx.post_cross_min(**args)
        torch.cuda.synchronize()
        return flat

    def result(self, flat):
        return flat[:self.Mc * self.Q].view(self.Mc, self.Q)

    def reference(self):
        """(ref, bound, argmin), each M_c x Q."""
        G = kernel_matrix(self.Uc, self.Ur, self.w, self.sf2, self.kind, self.d_split)
        c = G - self.Vc.astype(LD) @ self.Vr.astype(LD).T
        e = gr.error_bound(self.Vc, self.Vr.T, 0, 0, 1.0, 0.0, np.zeros((self.Mc, self.Mr))) + \
            kernel_gen_error(self.Uc, self.Ur, self.w, self.sf2, self.kind, self.d_split)
        m = self.m.astype(LD)
        ref, bound, arg = (np.zeros((self.Mc, self.Q), dtype=LD), np.zeros((self.Mc, self.Q), dtype=LD),
                           np.zeros((self.Mc, self.Q), dtype=np.int64))
        for k in range(self.Q):
            t = (LD(self.nodes[k]) * self.scale.astype(LD))[:, None]  # M_c x 1
            val = m[None, :] + t * c
            ref[:, k], arg[:, k] = val.min(1), val.argmin(1)
            bound[:, k] = (np.abs(t) * e + U53 * (2 * np.abs(t * c) + np.abs(m)[None, :])).max(1)
        return ref, bound, arg


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _ratio(P, flat, ref, bound):
    got = P.result(flat).cpu().numpy().astype(LD)
    assert np.all(np.isfinite(got.astype(np.float64)))
    err = np.abs(got - ref)
    # (a zero bound — node 0 against m_r = 0 — admits a zero error only)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf)).max())


@pytest.mark.parametrize("Mc,Mr,K,D,kind,Q,vt", CASES)
def test_against_long_double_under_the_derived_bound(gpu_ctx, Mc, Mr, K, D, kind, Q, vt):
    P = _Problem(Mc, Mr, K, D, kind, Q, seed=2000 + Mc + 7 * Mr + 13 * K + D + kind + 3 * Q, vt=vt)
    flat = P.run(gpu_ctx)
    ref, bound, _ = P.reference()
    ratio = _ratio(P, flat, ref, bound)
    print(f"Mc {Mc} Mr {Mr} K {K} D {D} kind {kind} Q {Q} transposed {vt}: observed / bound = {ratio:.3f} "
          f"(bound up to {float(bound.max()):.2e}, results in [{float(ref.min()):.3f}, {float(ref.max()):.3f}])")
    assert bool(torch.isnan(flat[Mc * Q:]).all()), "written behind out[M_c Q]"
    assert ratio <= 1.0, ratio
    again = P.run(gpu_ctx)
    assert torch.equal(_bits(flat[:Mc * Q]), _bits(again[:Mc * Q])), "two launches differ"


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("Mr", [1, 129, 200, 257])
def test_columns_beyond_the_reference_set_never_win(gpu_ctx, Mr, vt):
    """Every m_r >= 1 and |t c| <= tc = 1e-3 max |z_k| max scale_c max |c_cr| (a few 1e-2, taken from the long-double c): every
    result is at least 1 - tc, while a column beyond M_r that entered as 0 would give a result of at most tc.  Then the true
    minimiser is made the LAST valid column of the edge tile."""
    P = _Problem(130, Mr, 17, 8, 1, 17, seed=40 + Mr, vt=vt)
    P.m = 1.0 + np.random.default_rng(Mr).uniform(size=Mr)
    P.scale = P.scale * 1e-3
    flat = P.run(gpu_ctx)
    ref, bound, _ = P.reference()
    ratio = _ratio(P, flat, ref, bound)
    low = float(P.result(flat).min())
    c = kernel_matrix(P.Uc, P.Ur, P.w, P.sf2, P.kind, P.d_split) - P.Vc.astype(LD) @ P.Vr.astype(LD).T
    tc = float(np.abs(P.nodes).max() * P.scale.max() * np.abs(c).max())
    print(f"Mr {Mr} transposed {vt}: every m >= 1, |t c| <= {tc:.4f}: smallest result {low:.6f}, observed / bound = {ratio:.3f}")
    assert tc < 0.1 and low >= 1.0 - tc and ratio <= 1.0
    P.m[Mr - 1] = -5.0
    flat = P.run(gpu_ctx)
    ref, bound, arg = P.reference()
    ratio = _ratio(P, flat, ref, bound)
    print(f"Mr {Mr} transposed {vt}: minimiser in the last valid column: observed / bound = {ratio:.3f}")
    assert np.all(arg == Mr - 1) and float(P.result(flat).max()) < -4.9 and ratio <= 1.0


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("K,D,kind,Q", [(130, 8, 0, 17), (17, 64, 2, 64)])
def test_rows_and_the_order_of_the_reference_set_do_not_matter(gpu_ctx, K, D, kind, Q, vt):
    P = _Problem(300, 257, K, D, kind, Q, seed=5 + K, vt=vt)
    full = P.result(P.run(gpu_ctx))
    perm = np.random.default_rng(9).permutation(300)  # row i of the shuffled call is candidate perm[i]
    S = _Problem(300, 257, K, D, kind, Q, seed=5 + K, vt=vt)
    S.Uc, S.Vc, S.scale = P.Uc[perm], P.Vc[perm], P.scale[perm]
    moved = S.result(S.run(gpu_ctx))
    assert torch.equal(_bits(moved), _bits(full[torch.tensor(perm)])), "the result depends on the candidate's row"
    for i in (0, 127, 128, 299):
        S = _Problem(1, 257, K, D, kind, Q, seed=5 + K, vt=vt)
        S.Uc, S.Vc, S.scale, S.Ur, S.Vr, S.w, S.m = P.Uc[i:i + 1], P.Vc[i:i + 1], P.scale[i:i + 1], P.Ur, P.Vr, P.w, P.m
        alone = S.result(S.run(gpu_ctx))
        assert torch.equal(_bits(alone), _bits(full[i:i + 1])), f"candidate {i} scores differently alone"
    rperm = np.random.default_rng(10).permutation(257)
    S = _Problem(300, 257, K, D, kind, Q, seed=5 + K, vt=vt)
    S.Ur, S.Vr, S.m = P.Ur[rperm], P.Vr[rperm], P.m[rperm]
    shuffled = S.result(S.run(gpu_ctx))
    assert torch.equal(_bits(shuffled), _bits(full)), "the result depends on the order of the reference rows"


def test_binding_refuses_before_any_launch(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import NO_WORKSPACE, OP_POST_CROSS_MIN

    Mc, Mr, K, Q = 129, 257, 17, 5
    P = _Problem(Mc, Mr, K, 8, 1, Q, seed=3)
    dev = gpu_ctx.device
    flat = torch.full((Mc * Q + 5,), float("nan"), dtype=torch.float64, device=dev)
    out = flat[:Mc * Q].view(Mc, Q)
    odd = torch.zeros((Mc, K + 2), dtype=torch.float64, device=dev)[:, :K]           # leading dimension 19
    off = torch.zeros(Mc * (K + 1) + 1, dtype=torch.float64, device=dev)[1:].view(Mc, K + 1)[:, :K]  # 8 bytes off a 16-byte line
    assert odd.stride(0) % 2 == 1 and off.data_ptr() % 16 == 8 and off.stride(0) % 2 == 0
    ones = lambda n: torch.ones(n, dtype=torch.float64, device=dev)  # noqa: E731
    bad = {"odd leading dimension": dict(Vc=odd), "misaligned": dict(Vc=off),
           "dtype": dict(Vc=torch.zeros((Mc, K + 1), dtype=torch.float32, device=dev)[:, :K]),
           "dtype of the features": dict(Uc=torch.zeros((Mc, 8), dtype=torch.float32, device=dev)),
           "short m": dict(m=ones(Mr - 1)), "short scale": dict(scale=ones(Mc - 1)), "dtype of the nodes": dict(nodes=ones(Q).float()),
           "no nodes": dict(nodes=ones(0)), "65 nodes": dict(nodes=ones(65), out=torch.zeros((Mc, 65), dtype=torch.float64, device=dev)),
           "out for other nodes": dict(out=torch.zeros((Mc, Q + 1), dtype=torch.float64, device=dev)),
           "short out": dict(out=out[:Mc - 1]), "rows of Vc": dict(Vc=P.stored(P.Vc, dev)[:Mc - 1]),
           "K beyond the operand": dict(K=K + 1)}
    for what, change in bad.items():
        with pytest.raises(GppError):
            P.run(gpu_ctx, **{"flat": flat, **change})
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat).all())
    # no workspace on the handle: the C entry point itself reports it and enqueues nothing
    lib, h = gpu_ctx.lib, gpu_ctx.h
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    Uc, Ur, w, sf2, Vc, Vr = t(P.Uc), t(P.Ur), t(P.w), t([P.sf2]), P.stored(P.Vc, dev), P.stored(P.Vr, dev)
    m, scale, nodes = t(P.m), t(P.scale), t(P.nodes)
    need = lib.gpp_workspace_bytes(h, OP_POST_CROSS_MIN, Mr, Mc, 0, Q)
    assert need >= 2 * 3 * 128 * Q * 8
    small = torch.empty(need - 512, dtype=torch.uint8, device=dev)

    def raw(D=8, ldc=None, q=Q, nodes_ptr=None):
        return lib.gpp_post_cross_min(h, Uc.data_ptr(), Mc, Ur.data_ptr(), Mr, D, w.data_ptr(), sf2.data_ptr(), 1, 4, Vc.data_ptr(),
                                      Vc.stride(0) if ldc is None else ldc, Vr.data_ptr(), Vr.stride(0), K, 0, m.data_ptr(),
                                      scale.data_ptr(), nodes.data_ptr() if nodes_ptr is None else nodes_ptr, q, out.data_ptr())
    try:
        assert lib.gpp_set_workspace(h, small.data_ptr(), small.numel()) == 0
        assert raw() == NO_WORKSPACE
        assert lib.gpp_set_workspace(h, None, 0) == 0
        assert raw() == NO_WORKSPACE
    finally:
        gpu_ctx._ws = None  # the context attaches a workspace of its own at the next call that needs one
        lib.gpp_set_workspace(h, None, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat).all())
    # the C entry's own argument checks, and the same problem once the operands are right
    assert raw(ldc=Vc.stride(0) + 1) == -11 and raw(D=65) == -6 and raw(q=0) == -20 and raw(q=65) == -20
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat).all())
    P.run(gpu_ctx, flat=flat)
    ref, bound, _ = P.reference()
    assert _ratio(P, flat, ref, bound) <= 1.0 and bool(torch.isnan(flat[Mc * Q:]).all())
