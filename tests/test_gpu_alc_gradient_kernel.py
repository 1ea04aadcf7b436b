"""gpp_post_cross_lin_sq alone on the GPU: out[i] = sum_r omega_r (g_i(r) - Vf_i . Vr_r)^2 for rows that observe the linear functional
a_i0 f + sum_j a_ij df/du_{d0+j} at Uf_i, on random V of realistic magnitude and standard-normal coefficients (some exact zeros, some
rows (1, 0, ..., 0)), against long double under a DERIVED bound; then each property gpp.h states: bit for bit gpp_post_cross_sq on
value rows, repeatability, row independence, the exact zeros of w_d = 0 and of coincident points, the extents (NaN behind column K of
V, behind column 1 + nd of A and behind out), and every refusal code with the output untouched.

Bound (first order in u = 2^-53, as tests/test_gpu_alc_kernel.py and tests/pathwise_grad_reference.py).  The kernel forms
    c = fma(a_0 sf2, k, -acc);  c = fma(m_0, lin_0, c);  c = fma(m_1, lin_1, c),      lin_f = sum_{j in f} t_j df_j  (fmas, order of j)
with t_j = fl(a_j 2 fl(sqrt(w_j))) and df_j = fl(sa_j - sb_j) of the staged s = fl(u fl(sqrt(w_j))).  Its error e per entry is at most
    gemm_reference.error_bound(Vf, Vr^T)                                        the product, any summation order
  + |a_0| (kernel_gen_error + 2 u G)                                            the generator; the rounded a_0 sf2 (slack: u)
  + sum_f ( |lin_f| dm_f + |m_f| dlin_f )                                       dm_f = pathwise_grad_reference.kernel_multiplier_errors
  + 3 u (|a_0| G + |Vf| |Vr|^T + sum_f |m_f| L_f)                               the three fmas, each on a partial sum below this size
    dlin_f = sum_{j in f} |a_j| 2 w_j (3 u (|ua_j| + |ub_j|) + 4 u |ua_j - ub_j|) + (n_f + 1) u L_f,   L_f = sum_{j in f} |a_j| 2 w_j |ua_j - ub_j|
(the staged values carry 3 u each and their difference another u, as pathwise_reference._dr2 counts them; t_j carries 3 u: square
root 2 u, product u; the n_f fmas of the sum add (n_f + 1) u of the sum of magnitudes).  Then, exactly as for gpp_post_cross_sq,
    |out - ref| <= sum_r omega_r (2 |c| e + e^2) + (M_r + 4) u sum_r omega_r c^2.
Every case prints observed / bound before it asserts (pytest -s)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402
from pathwise_grad_reference import kernel_multiplier_errors, kernel_multipliers  # noqa: E402
from pathwise_reference import _split, kernel_gen_error, kernel_matrix  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = LD(2.0) ** -53
MFS, MRS, KS, DS, KINDS = (1, 127, 129, 300), (1, 128, 257), (1, 15, 17, 130), (1, 8, 64), (0, 1, 2)
#: (d0, nd) per D.  D = 8 (d_split 4): all, the Matern factor alone past the split, one RBF direction; D = 64 (d_split 32): across the
#: 16-dim staging chunk, and across chunk and split
DNS = {1: ((0, 1),), 8: ((0, 8), (5, 3), (2, 1)), 64: ((10, 12), (26, 12))}


def _cases():
    """The shape cycle of tests/test_gpu_alc_kernel.py with the directions of each D cycled along, then every (kind, D, directions)
    triple the cycle missed at 129 x 257, K = 17."""
    out = []
    for i, ((a, Mf), (b, Mr), rep) in enumerate(itertools.product(enumerate(MFS), enumerate(MRS), range(2))):
        D = DS[(a + rep + b) % 3]
        out.append((Mf, Mr, KS[(a + 2 * rep + b) % 4], D, KINDS[(a + 2 * rep + 2 * b) % 3], bool((a + rep) % 2), DNS[D][i % len(DNS[D])]))
    for kind, D in itertools.product(KINDS, DS):
        for dn in DNS[D]:
            if not any(c[4] == kind and c[3] == D and c[6] == dn for c in out):
                out.append((129, 257, 17, D, kind, True, dn))
    out.append((300, 257, 130, 64, 2, True, (26, 12)))
    return out


CASES = _cases()


def test_the_cases_cover_the_shapes():
    for vals, col in ((MFS, 0), (MRS, 1), (KS, 2), (DS, 3), (KINDS, 4), ((False, True), 5)):
        assert {c[col] for c in CASES} == set(vals)
    assert {(c[0], c[1]) for c in CASES} == set(itertools.product(MFS, MRS))
    assert {(c[4], c[3], c[6]) for c in CASES} == {(k, D, dn) for k in KINDS for D in DS for dn in DNS[D]}
    for Mr in MRS:  # the finish order: every K and every omega mode with one, one full and three column tiles
        assert {c[2] for c in CASES if c[1] == Mr} == set(KS) and {c[5] for c in CASES if c[1] == Mr} == {False, True}
    for D, dns in DNS.items():
        for d0, nd in dns:
            assert 0 <= d0 and nd >= 1 and d0 + nd <= D
    assert any(d0 < 4 < d0 + nd for d0, nd in DNS[8]) and any(d0 >= 4 for d0, _ in DNS[8]) and any(d0 + nd <= 4 for d0, nd in DNS[8])
    assert any(d0 < 16 < d0 + nd <= 32 for d0, nd in DNS[64]) and any(d0 < 32 < d0 + nd for d0, nd in DNS[64])


class _Problem:
    """Operands on the host (float64) and on the device: V in buffers with leading dimension K + 6 rounded to even and NaN behind
    column K (``vt``: the transposed operands, NaN behind the points); A with leading dimension 1 + nd + 3 and NaN behind 1 + nd."""

    def __init__(self, Mf, Mr, K, D, kind, weighted, dn, seed, vt=False):
        rng = np.random.default_rng(seed)
        self.Mf, self.Mr, self.K, self.D, self.kind, self.vt = Mf, Mr, K, D, kind, vt
        self.d0, self.nd = dn
        self.d_split = 0 if kind == 0 else D // 2
        self.Uf, self.Ur = rng.uniform(size=(Mf, D)), rng.uniform(size=(Mr, D))
        self.w = rng.uniform(0.5, 2.0, size=D) / D
        self.sf2 = 1.7
        self.Vf = rng.standard_normal((Mf, K)) * np.sqrt(0.5 * self.sf2 / K)
        self.Vr = rng.standard_normal((Mr, K)) * np.sqrt(0.5 * self.sf2 / K)
        self.omega = rng.uniform(0.0, 2.0, size=Mr) if weighted else None
        A = rng.standard_normal((Mf, 1 + self.nd))
        A[rng.uniform(size=A.shape) < 0.15] = 0.0  # exact zeros
        A[::5] = 0.0
        A[::5, 0] = 1.0  # value rows
        self.A = A

    def stored(self, V, dev):
        X = V.T if self.vt else V
        ld = X.shape[1] + 6 + (X.shape[1] & 1)
        buf = torch.full((X.shape[0], ld), float("nan"), dtype=torch.float64, device=dev)
        buf[:, :X.shape[1]] = torch.tensor(X)
        assert ld % 2 == 0 and buf.data_ptr() % 16 == 0
        return buf[:, :X.shape[1]]

    def stored_A(self, dev):
        buf = torch.full((self.A.shape[0], self.A.shape[1] + 3), float("nan"), dtype=torch.float64, device=dev)
        buf[:, :self.A.shape[1]] = torch.tensor(self.A)
        return buf[:, :self.A.shape[1]]

    def args(self, dev, out=None):
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
        if out is None:
            out = torch.full((self.Mf + 3,), float("nan"), dtype=torch.float64, device=dev)
        return dict(Uf=t(self.Uf), Ur=t(self.Ur), w=t(self.w), sf2=t([self.sf2]), A=self.stored_A(dev), d0=self.d0, nd=self.nd,
                    Vf=self.stored(self.Vf, dev), Vr=self.stored(self.Vr, dev), K=self.K, out=out,
                    omega=None if self.omega is None else t(self.omega), kind=self.kind, d_split=self.d_split, transposed=self.vt)

    def run(self, ctx, out=None, **change):
        args = self.args(ctx.device, out)
        args.update(change)
        ctx.post_cross_lin_sq(**args)
        torch.cuda.synchronize()
        return args["out"]

    def run_value(self, ctx):
        """gpp_post_cross_sq on the same operands (what a row (1, 0, ..., 0) must equal bit for bit)."""
        a = self.args(ctx.device)
        ctx.post_cross_sq(Uc=a["Uf"], Ur=a["Ur"], w=a["w"], sf2=a["sf2"], Vc=a["Vf"], Vr=a["Vr"], K=self.K, out=a["out"], omega=a["omega"],
                          kind=self.kind, d_split=self.d_split, transposed=self.vt)
        torch.cuda.synchronize()
        return a["out"]

    def reference(self):
        Uf, Ur, w, sf2, kind, ds = self.Uf, self.Ur, self.w, self.sf2, self.kind, self.d_split
        om = np.ones(self.Mr, dtype=LD) if self.omega is None else self.omega.astype(LD)
        A = self.A.astype(LD)
        G = kernel_matrix(Uf, Ur, w, sf2, kind, ds)
        m = kernel_multipliers(Uf, Ur, w, sf2, kind, ds)
        dm = kernel_multiplier_errors(Uf, Ur, w, sf2, kind, ds)
        split = _split(self.D, kind, ds)
        shape = (self.Mf, self.Mr)
        lin = [np.zeros(shape, dtype=LD) for _ in m]
        L = [np.zeros(shape, dtype=LD) for _ in m]
        stag = [np.zeros(shape, dtype=LD) for _ in m]
        n_f = [0 for _ in m]
        for j in range(self.nd):
            d = self.d0 + j
            f = 0 if d < split else 1
            diff = Uf[:, d, None].astype(LD) - Ur[None, :, d].astype(LD)
            mag = np.abs(Uf[:, d, None]).astype(LD) + np.abs(Ur[None, :, d]).astype(LD)
            coef = 2 * LD(w[d]) * A[:, 1 + j, None]
            lin[f] += coef * diff
            L[f] += np.abs(coef * diff)
            stag[f] += np.abs(coef) * (3 * U53 * mag + 4 * U53 * np.abs(diff))
            n_f[f] += 1
        a0 = A[:, 0, None]
        acc = self.Vf.astype(LD) @ self.Vr.astype(LD).T
        c = a0 * G - acc
        e = gr.error_bound(self.Vf, self.Vr.T, 0, 0, 1.0, 0.0, np.zeros(shape)) + \
            np.abs(a0) * (kernel_gen_error(Uf, Ur, w, sf2, kind, ds) + 2 * U53 * G)
        size = np.abs(a0) * G + np.abs(self.Vf).astype(LD) @ np.abs(self.Vr).astype(LD).T
        for f in range(len(m)):
            c = c + m[f] * lin[f]
            dlin = stag[f] + (n_f[f] + 1) * U53 * L[f]
            e = e + np.abs(lin[f]) * dm[f] + np.abs(m[f]) * dlin
            size = size + np.abs(m[f]) * L[f]
        e = e + 3 * U53 * size
        ref = (c * c) @ om
        bound = (2 * np.abs(c) * e + e * e) @ om + (self.Mr + 4) * U53 * ref
        return ref, bound


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _seed(Mf, Mr, K, D, kind, dn):
    return 2000 + Mf + 7 * Mr + 13 * K + D + kind + 31 * dn[0] + 57 * dn[1]


@pytest.mark.parametrize("Mf,Mr,K,D,kind,weighted,dn", CASES)
def test_against_long_double_under_the_derived_bound(gpu_ctx, Mf, Mr, K, D, kind, weighted, dn):
    P = _Problem(Mf, Mr, K, D, kind, weighted, dn, seed=_seed(Mf, Mr, K, D, kind, dn))
    out = P.run(gpu_ctx)
    ref, bound = P.reference()
    got = out[:Mf].cpu().numpy().astype(LD)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"Mf {Mf} Mr {Mr} K {K} D {D} kind {kind} omega {weighted} d0, nd {dn}: observed / bound = {ratio:.3f} "
          f"(max relative error {float((np.abs(got - ref) / ref).max()):.2e})")
    assert bool(torch.isnan(out[Mf:]).all()), "written behind M_f"
    assert np.all(np.isfinite(got.astype(np.float64))) and ratio <= 1.0, ratio
    again = P.run(gpu_ctx)
    assert torch.equal(_bits(out[:Mf]), _bits(again[:Mf])), "two launches differ"
    value = P.run_value(gpu_ctx)
    rows = torch.arange(0, Mf, 5)
    assert torch.equal(_bits(out[:Mf][rows]), _bits(value[:Mf][rows])), "a row (1, 0, ..., 0) is not gpp_post_cross_sq's value"


@pytest.mark.parametrize("K,D,kind,dn", [(15, 8, 0, (0, 8)), (130, 64, 2, (26, 12)), (17, 1, 1, (0, 1)), (17, 8, 1, (5, 3)),
                                         (130, 64, 1, (10, 12)), (15, 8, 2, (2, 1))])
def test_transposed_operands_meet_the_same_bound(gpu_ctx, K, D, kind, dn):
    P = _Problem(300, 257, K, D, kind, True, dn, seed=77 + K + D, vt=True)
    out = P.run(gpu_ctx)
    ref, bound = P.reference()
    got = out[:300].cpu().numpy().astype(LD)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"transposed K {K} D {D} kind {kind} d0, nd {dn}: observed / bound = {ratio:.3f}")
    assert bool(torch.isnan(out[300:]).all()) and ratio <= 1.0, ratio
    assert torch.equal(_bits(out[:300]), _bits(P.run(gpu_ctx)[:300]))
    rows = torch.arange(0, 300, 5)
    assert torch.equal(_bits(out[:300][rows]), _bits(P.run_value(gpu_ctx)[:300][rows]))


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("K,D,kind,dn", [(130, 8, 0, (0, 8)), (17, 64, 2, (26, 12)), (15, 8, 1, (5, 3))])
def test_all_value_rows_are_post_cross_sq_bit_for_bit(gpu_ctx, K, D, kind, dn, vt):
    P = _Problem(300, 257, K, D, kind, True, dn, seed=11 + K, vt=vt)
    P.A[:] = 0.0
    P.A[:, 0] = 1.0
    P.A[1::2, 1:] = -0.0  # a zero of either sign
    assert torch.equal(_bits(P.run(gpu_ctx)[:300]), _bits(P.run_value(gpu_ctx)[:300]))


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("K,D,kind,dn", [(130, 8, 0, (0, 8)), (17, 64, 2, (26, 12))])
def test_a_row_scores_the_same_alone_and_at_another_index(gpu_ctx, K, D, kind, dn, vt):
    P = _Problem(300, 257, K, D, kind, True, dn, seed=5 + K, vt=vt)
    full = P.run(gpu_ctx)
    perm = np.random.default_rng(9).permutation(300)  # row i of the shuffled call is row perm[i]
    Q = _Problem(300, 257, K, D, kind, True, dn, seed=5 + K, vt=vt)
    Q.Uf, Q.Vf, Q.A = P.Uf[perm], P.Vf[perm], P.A[perm]
    moved = Q.run(gpu_ctx)
    assert torch.equal(_bits(moved[:300]), _bits(full[:300][torch.tensor(perm)])), "the score depends on the row"
    for i in (0, 127, 128, 299):
        S = _Problem(1, 257, K, D, kind, True, dn, seed=5 + K, vt=vt)
        S.Uf, S.Vf, S.A, S.Ur, S.Vr, S.w, S.omega = P.Uf[i:i + 1], P.Vf[i:i + 1], P.A[i:i + 1], P.Ur, P.Vr, P.w, P.omega
        alone = S.run(gpu_ctx)
        assert torch.equal(_bits(alone[:1]), _bits(full[i:i + 1])), f"row {i} scores differently alone"


@pytest.mark.parametrize("kind,D,dn,dead", [(0, 8, (0, 8), 3), (1, 8, (0, 8), 6), (2, 64, (26, 12), 33), (2, 64, (10, 12), 12)])
def test_a_feature_of_weight_zero_contributes_an_exact_zero(gpu_ctx, kind, D, dn, dead):
    P = _Problem(129, 257, 17, D, kind, True, dn, seed=21 + D + kind)
    P.w[dead] = 0.0
    P.A[:, 1 + dead - dn[0]] = np.random.default_rng(2).standard_normal(129) * 1e6  # whatever multiplies the dead direction
    with_coef = P.run(gpu_ctx)
    P.A[:, 1 + dead - dn[0]] = 0.0
    without = P.run(gpu_ctx)
    assert bool(torch.isfinite(with_coef[:129]).all())
    assert torch.equal(_bits(with_coef[:129]), _bits(without[:129]))
    ref, bound = P.reference()
    assert float((np.abs(without[:129].cpu().numpy().astype(LD) - ref) / bound).max()) <= 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_coincident_points_are_finite_with_an_exact_zero_derivative_part(gpu_ctx, kind):
    D, dn = 8, (0, 8)
    P = _Problem(130, 1, 17, D, kind, False, dn, seed=31 + kind)
    P.Uf[:] = P.Ur[0]  # every row's point is the one reference point
    got = P.run(gpu_ctx)
    assert bool(torch.isfinite(got[:130]).all())
    P.A[:, 1:] = 0.0
    assert torch.equal(_bits(got[:130]), _bits(P.run(gpu_ctx)[:130]))
    # among other reference points: finite, and within the bound (whose reference has an exact 0 there as well)
    Q = _Problem(130, 257, 17, D, kind, True, dn, seed=41 + kind)
    Q.Uf[:100] = Q.Ur[:100]
    out = Q.run(gpu_ctx)
    ref, bound = Q.reference()
    assert bool(torch.isfinite(out[:130]).all())
    assert float((np.abs(out[:130].cpu().numpy().astype(LD) - ref) / bound).max()) <= 1.0


def test_binding_and_entry_refuse_before_any_launch(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import NO_WORKSPACE, OP_POST_CROSS_LIN

    Mf, Mr, K, D, d0, nd = 129, 257, 17, 8, 5, 3
    P = _Problem(Mf, Mr, K, D, 1, True, (d0, nd), seed=3)
    dev = gpu_ctx.device
    out = torch.full((Mf,), float("nan"), dtype=torch.float64, device=dev)
    odd = torch.zeros((Mf, K + 2), dtype=torch.float64, device=dev)[:, :K]           # leading dimension 19
    off = torch.zeros(Mf * (K + 1) + 1, dtype=torch.float64, device=dev)[1:].view(Mf, K + 1)[:, :K]  # 8 bytes off a 16-byte line
    assert odd.stride(0) % 2 == 1 and off.data_ptr() % 16 == 8 and off.stride(0) % 2 == 0
    bad = {"odd leading dimension": dict(Vf=odd), "misaligned": dict(Vf=off),
           "dtype": dict(Vf=torch.zeros((Mf, K + 1), dtype=torch.float32, device=dev)[:, :K]),
           "dtype of the features": dict(Uf=torch.zeros((Mf, D), dtype=torch.float32, device=dev)),
           "dtype of A": dict(A=torch.zeros((Mf, 1 + nd), dtype=torch.float32, device=dev)),
           "narrow A": dict(A=torch.zeros((Mf, nd), dtype=torch.float64, device=dev)),
           "rows of A": dict(A=torch.zeros((Mf - 1, 1 + nd), dtype=torch.float64, device=dev)),
           "strided A": dict(A=torch.zeros((Mf, 2 * (1 + nd)), dtype=torch.float64, device=dev)[:, ::2]),
           "directions beyond D": dict(d0=6), "no direction": dict(nd=0), "negative d0": dict(d0=-1),
           "short omega": dict(omega=torch.ones(Mr - 1, dtype=torch.float64, device=dev)),
           "short out": dict(out=out[:Mf - 1]), "rows of Vf": dict(Vf=P.stored(P.Vf, dev)[:Mf - 1]),
           "K beyond the operand": dict(K=K + 1)}
    for what, change in bad.items():
        with pytest.raises(GppError):
            P.run(gpu_ctx, **{"out": out, **change})
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the C entry point itself: no workspace on the handle, then each argument code, nothing enqueued by any of them
    lib, h = gpu_ctx.lib, gpu_ctx.h
    a = P.args(dev, out)
    good = dict(h=h, Uf=a["Uf"].data_ptr(), Mf=Mf, Ur=a["Ur"].data_ptr(), Mr=Mr, D=D, w=a["w"].data_ptr(), sf2=a["sf2"].data_ptr(),
                kind=1, d_split=4, d0=d0, nd=nd, A=a["A"].data_ptr(), lda=a["A"].stride(0), Vf=a["Vf"].data_ptr(), ldf=a["Vf"].stride(0),
                Vr=a["Vr"].data_ptr(), ldr=a["Vr"].stride(0), K=K, vt=0, omega=a["omega"].data_ptr(), out=out.data_ptr())

    def raw(**change):
        return lib.gpp_post_cross_lin_sq(*{**good, **change}.values())

    need = lib.gpp_workspace_bytes(h, OP_POST_CROSS_LIN, Mr, Mf, 0, 0)
    assert need >= 3 * 2 * 128 * 8
    small = torch.empty(need - 512, dtype=torch.uint8, device=dev)
    try:
        assert lib.gpp_set_workspace(h, small.data_ptr(), small.numel()) == 0
        assert raw() == NO_WORKSPACE
        assert lib.gpp_set_workspace(h, None, 0) == 0
        assert raw() == NO_WORKSPACE
    finally:
        gpu_ctx._ws = None  # the context attaches a workspace of its own at the next call that needs one
        lib.gpp_set_workspace(h, None, 0)
    gpu_ctx.ensure_workspace(OP_POST_CROSS_LIN, Mr, Mf, 0, 0)
    codes = [(-1, dict(h=None)), (-2, dict(Uf=None)), (-3, dict(Mf=0)), (-4, dict(Ur=None)), (-5, dict(Mr=0)), (-6, dict(D=65)),
             (-6, dict(D=0)), (-7, dict(w=None)), (-8, dict(sf2=None)), (-9, dict(kind=3)), (-10, dict(d_split=D + 1)),
             (-11, dict(d0=-1)), (-11, dict(d0=D)), (-12, dict(nd=0)), (-12, dict(nd=4)), (-13, dict(A=None)), (-14, dict(lda=nd)),
             (-15, dict(Vf=None)), (-15, dict(ldf=good["ldf"] + 1)), (-15, dict(ldf=K - 1)), (-15, dict(Vf=good["Vf"] + 8)),
             (-17, dict(Vr=None)), (-17, dict(ldr=good["ldr"] + 1)), (-19, dict(K=0)), (-20, dict(vt=2)), (-22, dict(out=None))]
    assert {c for c, _ in codes} == {-1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12, -13, -14, -15, -17, -19, -20, -22}
    for code, change in codes:
        assert raw(**change) == code, (code, change)
    assert raw(omega=None) == 0  # (NULL omega is all ones, not a refusal)
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    for code, change in codes:
        assert raw(**change) == code
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    P.run(gpu_ctx, out=out)
    ref, bound = P.reference()
    assert float((np.abs(out.cpu().numpy().astype(LD) - ref) / bound).max()) <= 1.0
