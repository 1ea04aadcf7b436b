"""``MultivariateNormal`` with a lazy covariance (gpytorch.distributions.MultivariateNormal subset).

``log_prob`` is the hot operator: for a :class:`LazyKernelMatrix` covariance it runs the fused HIP pipeline of
``linalg.exact_mll`` (reference: [3P] MultivariateNormal.log_prob -> inv_quad_logdet reached from
optim/mll_torch.py:116); dense covariances (predictive distributions) go through ``linalg.dense_log_prob``.

``rsample`` / ``sample`` (gpytorch MultivariateNormal.rsample, reached from models/gp_plus.py:985-998 ``sample_y``) draw
loc + Z U with U the upper Cholesky factor of the covariance (``linalg.mvn_root``), made once per covariance object.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .. import settings
from .kernels import DiagNoise, LazyKernelMatrix


class DenseCovariance:
    """Dense (M x M) covariance produced lazily by a builder, with a cheap diagonal; used for predictive MVNs."""

    def __init__(self, diag, builder=None, added_diag: Optional[torch.Tensor] = None, n: Optional[int] = None,
                 upper_builder=None):
        # ``diag``: the diagonal, or a callable producing it on first use (a prediction asked for its mean only never pays the
        # O(M N^2) product behind the variance); ``n``: the size, needed while the diagonal does not exist yet;
        # ``upper_builder(A, added, jitter)``: writes the covariance + diag(added) + jitter I into the upper triangle of the
        # square buffer A (what ``root`` factors); without it the dense matrix is copied there
        self._diag, self._builder, self._added = diag, builder, added_diag
        self._n = n if n is not None else diag.shape[0]
        self._dense = None
        self._upper = upper_builder
        self._root = None

    @property
    def shape(self):
        return torch.Size([self._n, self._n])

    def _diagonal(self) -> torch.Tensor:
        if callable(self._diag):
            self._diag = self._diag()
        return self._diag

    def diag(self):
        d = self._diagonal()
        return d if self._added is None else d + self._added

    def add_diag_vector(self, v: torch.Tensor) -> "DenseCovariance":
        added = v if self._added is None else self._added + v
        # (the diagonal stays lazy: a draw at the training inputs needs no V = K_*N L^-T)
        out = DenseCovariance(self._diag, self._builder, added, n=self._n, upper_builder=self._upper)
        out._dense = self._dense
        return out

    def evaluate(self) -> torch.Tensor:
        if self._dense is None:
            if self._builder is None:
                raise RuntimeError("this covariance only carries its diagonal")
            self._dense = self._builder()
        if self._added is None:
            return self._dense
        out = self._dense.clone()
        out.diagonal().add_(self._added)
        return out

    to_dense = evaluate

    def root(self, device) -> torch.Tensor:
        """Upper Cholesky factor U of this covariance (U^T U = Sigma, jitter schedule of ``linalg.mvn_root``), in the upper
        triangle of an n x n buffer; made on first use and kept."""
        if self._root is None:
            from ..linalg import mvn_root

            if self._upper is not None:
                build = lambda A, jit: self._upper(A, self._added, jit)  # noqa: E731
            else:
                build = _dense_builder(self.evaluate())
            self._root = mvn_root(build, self._n, device)[0]
        return self._root

    def __add__(self, other):
        if isinstance(other, DiagNoise):
            return self.add_diag_vector(other.diag())
        return NotImplemented


def _dense_builder(dense: torch.Tensor):
    """``build_upper`` of a covariance that exists as a dense matrix: a copy (the factorisation works in place)."""
    def build(A, jit):
        A.copy_(dense)
        if jit:
            A.diagonal().add_(jit)
    return build


def _kernel_root(cov: LazyKernelMatrix) -> torch.Tensor:
    """Upper Cholesky factor of a square lazy kernel matrix (the prior, or the prior predictive after a likelihood), built
    tile by tile into the upper triangle (gpp_kernel_build) and factored; kept on the matrix object."""
    root = getattr(cov, "_root", None)
    if root is None:
        from ..backend import UPLO_UPPER, get_context
        from ..linalg import _as_f64, mvn_root

        if not cov.is_square:
            raise RuntimeError("sampling needs a square covariance")
        dev = cov.U1.device
        gctx = get_context(dev)
        U, spec = _as_f64(cov.U1.detach(), dev), cov.spec
        w, sf2 = _as_f64(spec.w.detach(), dev), _as_f64(spec.sf2.detach().reshape(1), dev)
        tau = None if cov.tau is None else _as_f64(cov.tau.detach().reshape(-1), dev)
        grp = None if cov.grp is None else cov.grp.to(torch.int32)

        def build(A, jit):
            gctx.kernel_build(U, w, sf2, tau, grp, A, jitter=jit, kind=spec.kind, d_split=spec.d_split, uplo=UPLO_UPPER)

        root = mvn_root(build, U.shape[0], dev)[0]
        cov._root = root
    return root


class MultivariateNormal:
    def __init__(self, mean: torch.Tensor, covariance_matrix):
        self.loc = mean
        self._covar = covariance_matrix
        self._tensor_root = None  # (a plain tensor covariance cannot carry its factor)

    # -- accessors -------------------------------------------------------------------------------
    @property
    def mean(self):
        return self.loc

    @property
    def lazy_covariance_matrix(self):
        return self._covar

    @property
    def covariance_matrix(self):
        return self._covar if torch.is_tensor(self._covar) else self._covar.evaluate()

    @property
    def variance(self):
        d = self._covar.diagonal() if torch.is_tensor(self._covar) else self._covar.diag()
        return d.clamp_min(settings.min_variance.value())

    @property
    def stddev(self):
        return self.variance.sqrt()

    @property
    def event_shape(self):
        return self.loc.shape[-1:]

    def confidence_region(self):
        s2 = self.stddev * 2
        return self.loc - s2, self.loc + s2

    # -- the hot operator ------------------------------------------------------------------------
    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        cov = self._covar
        if isinstance(cov, LazyKernelMatrix):
            if not cov.is_square:
                raise RuntimeError("log_prob needs a square covariance")
            if cov.tau is None:
                raise RuntimeError("log_prob of a noise-free kernel matrix: apply the likelihood first")
            from ..linalg import exact_mll

            return exact_mll(cov.U1, cov.spec, cov.tau, self.loc, value, cov.grp, cov.n_grad_dims, calib=cov.calib)
        from ..linalg import dense_log_prob

        dense = cov if torch.is_tensor(cov) else cov.evaluate()
        return dense_log_prob(dense, (value - self.loc).to(torch.float64))

    def loo_log_prob(self, value: torch.Tensor) -> torch.Tensor:
        """Leave-one-out log pseudo-likelihood sum_i log p(value_i | value_-i) of a (noisy) lazy kernel covariance
        (``linalg.exact_loo``; gpytorch's LeaveOneOutPseudoLikelihood computes it from the same distribution)."""
        cov = self._covar
        if not isinstance(cov, LazyKernelMatrix):
            raise NotImplementedError("loo_log_prob needs the lazy kernel covariance of a training evaluation")
        if not cov.is_square:
            raise RuntimeError("loo_log_prob needs a square covariance")
        if cov.tau is None:
            raise RuntimeError("loo_log_prob of a noise-free kernel matrix: apply the likelihood first")
        if cov.calib is not None:
            raise NotImplementedError("loo_log_prob: the objective has no gradient by calibration parameters")
        from ..linalg import exact_loo

        return exact_loo(cov.U1, cov.spec, cov.tau, self.loc, value, cov.grp, cov.n_grad_dims)

    def cv_log_prob(self, value: torch.Tensor, folds) -> torch.Tensor:
        """Grouped cross-validation log pseudo-likelihood sum_F log p(value_F | value_-F) of a (noisy) lazy kernel covariance for
        ``folds`` — an int k, one integer label per row, or a ``cv.FoldIndex`` (``linalg.exact_cv``: every fold from one
        factorisation)."""
        cov = self._covar
        if not isinstance(cov, LazyKernelMatrix):
            raise NotImplementedError("cv_log_prob needs the lazy kernel covariance of a training evaluation")
        if not cov.is_square:
            raise RuntimeError("cv_log_prob needs a square covariance")
        if cov.tau is None:
            raise RuntimeError("cv_log_prob of a noise-free kernel matrix: apply the likelihood first")
        if cov.calib is not None:
            raise NotImplementedError("cv_log_prob: the objective has no gradient by calibration parameters")
        from ..linalg import exact_cv

        return exact_cv(cov.U1, cov.spec, cov.tau, self.loc, value, folds, cov.grp, cov.n_grad_dims)

    def gek_log_prob(self, value: torch.Tensor, gradient_data) -> torch.Tensor:
        """Joint log-density log N([value - mean; r_g] | 0, Kj) of ``value`` and of observed gradients, for a (noisy) lazy kernel
        covariance (``linalg.exact_gek_mll``).  ``gradient_data`` = (Ug, r_g, noise, d0, nd): the feature rows of the gradient points
        from the same ``forward`` of the model, the Mg x nd gradients in scaled units, their variances in scaled units squared or
        None for the default nugget, and the range of differentiated features; optionally a sixth entry, the
        ``backend.GradientSelection`` of the observed entries, with r_g and noise holding those q entries alone."""
        cov = self._covar
        if not isinstance(cov, LazyKernelMatrix):
            raise NotImplementedError("gek_log_prob needs the lazy kernel covariance of a training evaluation")
        if not cov.is_square:
            raise RuntimeError("gek_log_prob needs a square covariance")
        if cov.tau is None:
            raise RuntimeError("gek_log_prob of a noise-free kernel matrix: apply the likelihood first")
        if cov.calib is not None:
            raise NotImplementedError("gek_log_prob: the objective has no gradient by calibration parameters")
        from ..linalg import exact_gek_mll

        Ug, r_g, noise, d0, nd = gradient_data[:5]
        sel = gradient_data[5] if len(gradient_data) > 5 else None
        dU = cov.n_grad_dims
        if dU is None:
            dU = int(d0) if (cov.U1.requires_grad or Ug.requires_grad) else 0
        return exact_gek_mll(cov.U1, Ug, cov.spec, cov.tau, self.loc, value, r_g, noise, cov.grp, d0, nd, min(int(dU), int(d0)),
                             sel=sel)

    # -- sampling --------------------------------------------------------------------------------
    def root_factor(self) -> torch.Tensor:
        """Upper Cholesky factor U of the covariance (U^T U = Sigma; an M x M view whose strict lower triangle is not part of
        it), the one ``rsample`` draws with: made on first use and kept on the covariance object."""
        cov = self._covar
        with torch.no_grad():
            if isinstance(cov, LazyKernelMatrix):
                return _kernel_root(cov)
            if isinstance(cov, DenseCovariance):
                return cov.root(self.loc.device)
            if self._tensor_root is None:
                from ..linalg import mvn_root

                self._tensor_root = mvn_root(_dense_builder(cov.to(torch.float64)), cov.shape[-1], self.loc.device)[0]
            return self._tensor_root

    def rsample(self, sample_shape=torch.Size(), base_samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Draws of shape ``sample_shape + (M,)``: loc + Z U, Z = ``base_samples`` (that shape) or standard normals drawn on the
        distribution's device in float64 (``torch.manual_seed`` reproduces them).  The draws carry no autograd graph."""
        from ..linalg import mvn_draw

        M = self.loc.shape[-1]
        if self.loc.dim() != 1:
            raise NotImplementedError("batched distributions are outside the exact-GP hot path")
        sample_shape = torch.Size(sample_shape)
        with torch.no_grad():
            if base_samples is None:
                Z = torch.randn(sample_shape + (M,), dtype=torch.float64, device=self.loc.device)
            else:
                if tuple(base_samples.shape) != tuple(sample_shape) + (M,):
                    raise RuntimeError(f"base_samples of shape {tuple(base_samples.shape)} for draws of shape "
                                       f"{tuple(sample_shape) + (M,)}")
                Z = base_samples.detach().to(device=self.loc.device, dtype=torch.float64)
            U = self.root_factor()
            out = mvn_draw(U, self.loc.detach(), Z.reshape(-1, M))
            return out.reshape(sample_shape + (M,)).to(self.loc.dtype)

    def sample(self, sample_shape=torch.Size(), base_samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)

    def __repr__(self):
        return f"MultivariateNormal(loc: {tuple(self.loc.shape)})"
