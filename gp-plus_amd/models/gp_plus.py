"""``GP_Plus``: GP+'s model class (reference: models/gp_plus.py:46-1461) for the deterministic exact-GP path, on the
HIP back end.  Same constructor signature, ``fit`` / ``predict`` / ``evaluation`` / ``score`` / ``get_params`` API,
buffers and state_dict keys.

What runs differently from the reference, by design:
  * ``forward`` returns a LAZY covariance (features U, weights w, outputscale): nothing N x N is allocated in Python;
    the reference's per-pass ``Sigma_sum`` moment matching (gp_plus.py:396,474-482) is the identity for the single
    deterministic pass and is dropped;
  * the two O(N) interpreter loops per forward (``transform_categorical`` gp_plus.py:1085, ``multi_mean``
    gp_plus.py:532-534) become one cached integer index + gather;
  * the model is placed on ``device`` at construction (the reference moves it in ``fit``, gp_plus.py:562).
Out of scope (raise ``NotImplementedError``): probabilistic embedding / calibration (stochastic multi-pass
ensembles), neural-network and polynomial mean functions, plotting (``visualize_latent``, ``sample_y(plot=True)``), Sobol
indices, botorch glue, gradients through the joint predictive covariance (``predict_with_grad`` differentiates the mean and
the variance diagonal) and gradients through posterior draws (``sample_y`` returns draws without an autograd graph).
What this build offers in the place of the multi-pass ensembles: ``fit(keep_restarts=K)`` keeps the K best restarts of a batched
fit as ``restart_ensemble``, an ``ensemble.HyperparameterEnsemble`` whose ``predict`` mixes the members' posteriors by the same
moment matching (law of total variance), all members in one launch (gpp_predict_gen_batched).  The probabilistic embedding itself —
sampling the latent map per pass — stays out of scope.
"""
import math
import warnings
from itertools import product
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from .. import kernels
from ..gpcore import ConstantMean, MultivariateNormal, NormalPrior, Positive, ZeroMean
from ..gpcore import metrics as gpmetrics
from ..optim import fit_model_torch
from ..preprocessing import setlevels
from ..priors import MollifiedUniformPrior
from ..utils import data_type_check, set_seed  # noqa: F401
from ..likelihoods_noise.multifidelity import Multifidelity_likelihood
from .gpregression import GPR, _check_weights

_QUANT_CLASSES = ['Rough_RBF', 'RBFKernel', 'Matern32Kernel', 'Matern12Kernel', 'Matern52Kernel']  # gp_plus.py:150


class ActiveSubspace:
    """What ``GP_Plus.active_subspace`` returns: the matrix C = sum_a w_a (g_a g_a^T + S_a), its eigen-decomposition (eigenvalues
    descending, eigenvectors as columns), its two parts and its diagonal (the derivative-based sensitivity measures)."""
    __slots__ = ("matrix", "eigenvalues", "eigenvectors", "mean_part", "cov_part", "sensitivity")

    def __init__(self, matrix, eigenvalues, eigenvectors, mean_part, cov_part, sensitivity):
        self.matrix, self.eigenvalues, self.eigenvectors = matrix, eigenvalues, eigenvectors
        self.mean_part, self.cov_part, self.sensitivity = mean_part, cov_part, sensitivity

    def __repr__(self):
        return f"ActiveSubspace(p={self.matrix.shape[0]}, eigenvalues={self.eigenvalues.tolist()})"


def _rough_transform(x):
    return 2.0 ** (-0.5) * torch.pow(10, -x / 2)


def _rough_inv_transform(x):
    # the reference registers -2 log10(x/2) (gp_plus.py:252), which is NOT the inverse of the transform; kept as is
    return -2.0 * torch.log10(x / 2.0)


class GP_Plus(GPR):
    def __init__(self, train_x: torch.Tensor, train_y: torch.Tensor, dtype=torch.float, device="cpu", qual_dict={},
                 multiple_noise=False, lb_noise: float = 1e-8, fix_noise: bool = False, fix_noise_val: float = 1e-5,
                 quant_correlation_class: str = 'Rough_RBF', fixed_length_scale: bool = False,
                 fixed_length_scale_val=torch.tensor([1.0]), encoding_type='one-hot', embedding_dim: int = 2,
                 separate_embedding=[], embedding_type='deterministic', NN_layers_embedding: list = [],
                 m_gp='single_constant', m_gp_ref='zero', NN_layers_m_gp=[], calibration_type='deterministic',
                 calibration_id=[], mean_prior_cal=None, std_prior_cal=None, interval_score=False, num_pass_train=1,
                 num_pass_pred=1, seed_number=1) -> None:
        # parameters and buffers are created directly in ``dtype`` (the reference creates fp32 parameters and casts
        # in fit(), gp_plus.py:562 / SURVEY.md B-4); with dtype=float64 initial values such as lengthscale=1 are exact
        _prev_default = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            self._construct(train_x, train_y, dtype, device, qual_dict, multiple_noise, lb_noise, fix_noise, fix_noise_val,
                            quant_correlation_class, fixed_length_scale, fixed_length_scale_val, encoding_type,
                            embedding_dim, separate_embedding, embedding_type, NN_layers_embedding, m_gp, m_gp_ref,
                            NN_layers_m_gp, calibration_type, calibration_id, mean_prior_cal, std_prior_cal, interval_score,
                            num_pass_train, num_pass_pred, seed_number)
        finally:
            torch.set_default_dtype(_prev_default)

    def _construct(self, train_x, train_y, dtype, device, qual_dict, multiple_noise, lb_noise, fix_noise, fix_noise_val,
                   quant_correlation_class, fixed_length_scale, fixed_length_scale_val, encoding_type, embedding_dim,
                   separate_embedding, embedding_type, NN_layers_embedding, m_gp, m_gp_ref, NN_layers_m_gp,
                   calibration_type, calibration_id, mean_prior_cal, std_prior_cal, interval_score, num_pass_train,
                   num_pass_pred, seed_number) -> None:
        self.mean_prior_cal = [0 for _ in calibration_id] if mean_prior_cal is None else mean_prior_cal
        self.std_prior_cal = [1 for _ in calibration_id] if std_prior_cal is None else std_prior_cal
        self.interval_score = interval_score
        self.tkwargs = {'dtype': dtype, 'device': torch.device(device)}
        self.fixed_length_scale_val = fixed_length_scale_val.to(**self.tkwargs) if fixed_length_scale else None

        train_x = data_type_check(train_x)
        train_y = data_type_check(train_y)
        # argument validation: gp_plus.py:141-182
        if not isinstance(qual_dict, dict):
            raise ValueError("qual_dict should be a dictionary.")
        if multiple_noise not in [True, False]:
            raise ValueError("multiple_noise should be either True or False.")
        if not isinstance(embedding_dim, int):
            raise ValueError("embedding_dim should be an integer.")
        if quant_correlation_class not in _QUANT_CLASSES:
            raise ValueError("quant_correlation_class should be 'Rough_RBF', 'RBFKernel', 'Matern32Kernel', 'Matern12Kernel','Matern52Kernel'.")
        if fix_noise not in [True, False]:
            raise ValueError("fix_noise should be either True or False.")
        if not isinstance(NN_layers_embedding, list) or not all(isinstance(i, int) for i in NN_layers_embedding):
            raise ValueError("NN_layers_embedding should be a list of integers representing the number of neurons in each layer.")
        if encoding_type != 'one-hot':
            raise ValueError("encoding_type should be 'one-hot'.")
        if embedding_type not in ['deterministic', 'probabilistic']:
            raise ValueError("embedding_type should be either 'deterministic' or 'probabilistic'.")
        if not isinstance(separate_embedding, list) or not all(isinstance(i, int) for i in separate_embedding):
            raise ValueError("separate_embedding should be a list with integers showing the number of categorical inputs to be considered in a separate manifold in each layer.")
        if not isinstance(NN_layers_m_gp, list) or not all(isinstance(i, int) for i in NN_layers_m_gp):
            raise ValueError("NN_layers_m_gp should be a list with integers representing the number of neurons in each layer for the mean function.")
        if not isinstance(calibration_id, list) or not all(isinstance(i, int) for i in calibration_id):
            raise ValueError("calibration_id should be a list where each entry shows the column number in the dataset that the calibration parameters are assigned to.")
        # scope of this build
        if quant_correlation_class == 'Matern12Kernel':
            # passes the reference's validation (gp_plus.py:150) and then fails at gp_plus.py:236-241, because
            # kernels/matern.py:4-8 defines Matern32Kernel and Matern52Kernel only: same error, raised before any work
            raise RuntimeError("%s not an allowed kernel" % quant_correlation_class)
        if embedding_type == 'probabilistic' or calibration_type in ('probabilistic', 'probabelistic'):
            raise NotImplementedError("probabilistic embedding/calibration (stochastic multi-pass ensembles, "
                                      "gp_plus.py:387-392,414-461) is outside the exact-GP hot path of this build")
        if len(calibration_id) > 0:
            # deterministic calibration (gp_plus.py:311-320,440-461): every id names a quantitative column of train_x
            ncol = train_x.shape[-1]
            for n in calibration_id:
                if n < 0 or n >= ncol or n in qual_dict:
                    raise ValueError(f"calibration_id: column {n} is not a quantitative column of train_x "
                                     "(a calibration parameter stands in a quantitative input)")
            if len(set(calibration_id)) != len(calibration_id):
                raise ValueError("calibration_id: a column is listed twice")
            if (ncol - 1) not in qual_dict or qual_dict[ncol - 1] < 2:
                raise ValueError("calibration needs the data source as the last, categorical column of train_x "
                                 "(the calibrated rows are those of source 0)")
            if len(self.mean_prior_cal) != len(calibration_id) or len(self.std_prior_cal) != len(calibration_id):
                raise ValueError("mean_prior_cal and std_prior_cal need one entry per calibration_id")
        if len(separate_embedding) > 0:
            raise NotImplementedError("separate_embedding is effectively broken in the reference (SURVEY.md B-5)")
        if m_gp not in ('single_constant', 'single_zero', 'multiple_constant'):
            raise NotImplementedError(f"mean function '{m_gp}' is outside this build's scope "
                                      "(single_constant, single_zero, multiple_constant are supported)")

        train_x = self.fill_nan_with_mean(train_x, calibration_id)
        self.seed = seed_number
        self.calibration_id = calibration_id
        self.calibration_source_index = 0
        self.calibration_type = calibration_type
        if len(calibration_id) > 0:
            # gp_plus.py:318-320: the calibrated source's entries in the calibrated columns are unknown (NaN is the expected way to
            # say so; fill_nan_with_mean has put the column mean there) and are zeroed: theta stands there in every forward
            rows = torch.where(train_x[:, -1] == self.calibration_source_index)[0]
            for n in calibration_id:
                train_x[rows, n] = torch.zeros_like(train_x[rows, n])
        # index bookkeeping: gp_plus.py:190-217
        qual_dict_list = list(qual_dict.keys())
        all_index = set(range(train_x.shape[-1]))
        quant_index = sorted(all_index.difference(qual_dict_list))
        num_levels_per_var = list(qual_dict.values())
        lm_columns = list(set(qual_dict_list).difference(separate_embedding))
        qual_kernel_columns = [*separate_embedding, lm_columns] if len(lm_columns) > 0 else separate_embedding
        train_y = train_y.reshape(-1)
        noise_indices = list(range(0, num_levels_per_var[-1])) if multiple_noise else []
        if len(qual_dict_list) == 1 and num_levels_per_var[0] < 2:
            quant_index = quant_index + [qual_dict_list[0]]
            qual_dict_list = []
            qual_kernel_columns = []
            embedding_dim = 0
        elif len(qual_dict_list) == 0:
            embedding_dim = 0

        # kernel assembly: gp_plus.py:219-303
        qual_kernels = []
        if len(qual_dict_list) > 0:
            for i in range(len(qual_kernel_columns)):
                k = kernels.RBFKernel(active_dims=torch.arange(embedding_dim) + embedding_dim * i)
                k.initialize(**{'lengthscale': 1.0})
                k.raw_lengthscale.requires_grad_(False)
                qual_kernels.append(k)
        quant_correlation_class_name = quant_correlation_class
        if quant_correlation_class_name == 'Rough_RBF':
            quant_correlation_class = 'RBFKernel'  # gp_plus.py:229-230
        if len(quant_index) == 0:
            correlation_kernel = qual_kernels[0]
            for i in range(1, len(qual_kernels)):
                correlation_kernel *= qual_kernels[i]
        else:
            try:
                quant_cls = getattr(kernels, quant_correlation_class)
            except AttributeError:
                raise RuntimeError("%s not an allowed kernel" % quant_correlation_class)
            active = len(qual_kernel_columns) * embedding_dim + torch.arange(len(quant_index))
            if quant_correlation_class_name == 'RBFKernel':
                constraint = Positive(transform=torch.exp, inv_transform=torch.log)
                prior = MollifiedUniformPrior(math.log(0.1), math.log(10))
            else:
                constraint = Positive(transform=_rough_transform, inv_transform=_rough_inv_transform)
                prior = NormalPrior(-3.0, 3.0)
            quant_kernel = quant_cls(ard_num_dims=len(quant_index), active_dims=active, lengthscale_constraint=constraint)
            quant_kernel.register_prior('lengthscale_prior', prior, 'raw_lengthscale')
            if len(qual_dict_list) > 0:
                temp = qual_kernels[0]
                for i in range(1, len(qual_kernels)):
                    temp *= qual_kernels[i]
                correlation_kernel = temp * quant_kernel
            else:
                correlation_kernel = quant_kernel

        super(GP_Plus, self).__init__(train_x=train_x, train_y=train_y, noise_indices=noise_indices,
                                      correlation_kernel=correlation_kernel, fix_noise=fix_noise,
                                      fix_noise_val=fix_noise_val, lb_noise=lb_noise)

        self.register_buffer('quant_index', torch.tensor(quant_index, dtype=torch.long))
        self.register_buffer('qual_dict_list', torch.tensor(qual_dict_list, dtype=torch.long))
        self.qual_kernel_columns = qual_kernel_columns
        self.num_levels_per_var = num_levels_per_var
        self.embedding_dim = embedding_dim
        self.encoding_type = encoding_type
        self.embedding_type = embedding_type
        self.perm, self.zeta, self.perm_dict, self.A_matrix = [], [], [], []
        self.count = train_x.size()[0]
        self.num_pass_train, self.num_pass_pred = num_pass_train, num_pass_pred
        self._cat_cache = {}
        # calibration parameters (gp_plus.py:311-320): Theta_<n>.constant with a NormalPrior of its own; feature column of the k-th one
        # = embedding dims + position of column n among the quantitative columns (the reference's embeddings.size(1) + n whenever
        # the categorical columns come last, which it assumes)
        self._calib_pos = [quant_index.index(n) for n in calibration_id]
        self._calib_cache, self._calib_cols = None, {}
        for n, mean_prior, std_prior in zip(calibration_id, self.mean_prior_cal, self.std_prior_cal):
            setattr(self, 'Theta_' + str(n), ConstantMean(prior=NormalPrior(float(mean_prior), float(std_prior))))
        if len(qual_kernel_columns) > 0:
            for i in range(len(qual_kernel_columns)):
                if type(qual_kernel_columns[i]) == int:
                    cat = [self.num_levels_per_var[qual_dict_list.index(qual_kernel_columns[i])]]
                else:
                    cat = [self.num_levels_per_var[qual_dict_list.index(k)] for k in qual_kernel_columns[i]]
                num = sum(cat)
                zeta, perm, perm_dict = self.zeta_matrix(num_levels=cat, embedding_dim=self.embedding_dim)
                self.zeta.append(zeta)
                self.perm.append(perm)
                self.perm_dict.append(perm_dict)
                model_temp = FFNN(self, input_size=num, num_classes=embedding_dim, layers=NN_layers_embedding,
                                  name='latent' + str(qual_kernel_columns[i]))
                self.A_matrix.append(model_temp)

        if fixed_length_scale:
            self.covar_module.base_kernel.raw_lengthscale.data = self.fixed_length_scale_val
            self.covar_module.base_kernel.raw_lengthscale.requires_grad = False
        # mean functions: gp_plus.py:366-382
        self.m_gp = m_gp
        self.m_gp_ref = m_gp_ref
        self.num_sources = int(torch.max(train_x[:, -1]))
        size = train_x.shape[1]
        if self.m_gp.startswith('single'):
            self.single_m_gp_register(size, m_gp_type=self.m_gp, wm='mean_module')
        else:
            self.multi_m_gp_register(train_x, ['multiple_constant'], self.m_gp_ref)
        self.to(**self.tkwargs)

    # ------------------------------------------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)  # encoder weights are registered on this module, so they move too
        self._cat_cache = {}
        self._calib_cache, self._calib_cols = None, {}
        if hasattr(self, 'likelihood') and hasattr(self.likelihood, 'fidel_indices') and torch.is_tensor(self.likelihood.fidel_indices):
            self.likelihood.fidel_indices = fn(self.likelihood.fidel_indices)
        return out

    def _features(self, x: torch.Tensor):
        """gp_plus.py:408-437: x_new = cat([A(zeta[index]), x[:, quant_index]]); returns (x_new, #leading manifold dims)."""
        dev = self.tkwargs['device']
        if len(self.qual_kernel_columns) == 0:
            return x.to(dev), 0
        i = len(self.qual_kernel_columns) - 1  # the reference embeds only the last group
        # The O(N) level lookup runs once for the TRAINING inputs (same tensor object every forward of a fit, B-6) and
        # every time for anything else.  The key is the object's identity, never its address: the caching allocator
        # hands a freed test batch's address to the next one of the same shape.
        is_train = self.train_inputs is not None and len(self.train_inputs) > 0 and x is self.train_inputs[0]
        key = ('train', x._version, self.training) if is_train else None
        zeta_rows = self._cat_cache.get(key) if key is not None else None
        if zeta_rows is None:
            xc = x[:, self.qual_kernel_columns[i]].clone().type(torch.int64)
            zeta_rows = self.transform_categorical(x=xc, perm_dict=self.perm_dict[i], zeta=self.zeta[i]).to(**self.tkwargs)
            if key is not None:
                self._cat_cache = {key: zeta_rows}
        emb = self.A_matrix[i](zeta_rows)
        xq = x[..., self.quant_index.long()].to(**self.tkwargs)
        if len(self.calibration_id) > 0:
            # gp_plus.py:439-461: theta_k into the rows of the calibrated source, in training and in eval mode, for any x (the
            # membership comes from THIS x's last column).  The values enter as constants: the gradient by theta is
            # CalibratedMLLFunction's own (``_calibration``), not a feature gradient
            member = self._calibration_rows(x)[0]
            pos = self._calib_pos
            xq[:, pos] = torch.where(member.unsqueeze(1), self._theta_vector().detach().unsqueeze(0), xq[:, pos])
        x_new = torch.cat([emb, xq], dim=-1)
        return x_new, emb.shape[-1]

    def _theta_vector(self):
        """The calibration parameters (C,), autograd-connected to ``Theta_<n>.constant``, in ``calibration_id`` order."""
        return torch.cat([getattr(self, 'Theta_' + str(n)).constant.reshape(1) for n in self.calibration_id]).to(**self.tkwargs)

    def _calibration(self, x, dz):
        """What the training objective needs besides the features of ``x`` (``linalg.Calibration``): theta, the membership of the
        rows and the feature column of each parameter."""
        from ..linalg import Calibration

        cols = self._calib_cols.get(dz)
        if cols is None:
            cols = torch.tensor([dz + pos for pos in self._calib_pos], dtype=torch.int32, device=self.tkwargs['device'])
            self._calib_cols[dz] = cols
        return Calibration(self._theta_vector(), self._calibration_rows(x)[1], cols)

    def _calibration_rows(self, x):
        """(membership of ``x``'s rows in the calibrated source as bool, the same as int32) on the model's device; computed once for
        the training inputs (the same tensor object in every forward of a fit), every time for anything else."""
        dev = self.tkwargs['device']
        is_train = self.train_inputs is not None and len(self.train_inputs) > 0 and x is self.train_inputs[0]
        cached = getattr(self, '_calib_cache', None)
        if is_train and cached is not None and cached[0] is x and cached[1] == x._version:
            return cached[2]
        member = (x[:, -1] == self.calibration_source_index).to(dev)
        out = (member, member.to(torch.int32).contiguous())
        if is_train:
            self._calib_cache = (x, x._version, out)
        return out

    def _refuse_calibrated(self, what: str, why: str):
        if len(self.calibration_id) > 0:
            raise NotImplementedError(f"{what} is not available for a model with calibration parameters: {why}")

    def calibration_result(self, mean_train=None, std_train=None):
        """gp_plus.py:934-956: the estimated calibration parameters ``{n: theta_n}``, a float per id.  With the column means and
        standard deviations the inputs were standardised by, ``theta_n * std_train[n] + mean_train[n]``: the parameter in the units
        of the data."""
        if (mean_train is None) != (std_train is None):
            raise ValueError("calibration_result: give both mean_train and std_train, or neither")
        out = {}
        for n in self.calibration_id:
            theta = float(getattr(self, 'Theta_' + str(n)).constant.detach().reshape(-1)[0])
            out[n] = theta if mean_train is None else theta * float(std_train[n]) + float(mean_train[n])
        return out

    #: the restarts kept by the last ``fit(keep_restarts=K)`` as an ``ensemble.HyperparameterEnsemble``; None otherwise
    restart_ensemble = None

    def forward(self, x: torch.Tensor) -> MultivariateNormal:
        """gp_plus.py:386-484 (deterministic single pass)."""
        if x.dim() > 2:
            raise NotImplementedError("batched inputs are outside the exact-GP hot path")
        x_forward_raw = x
        x_new, dz = self._features(x)
        if self.m_gp.startswith('multi'):
            mean_x = self.multi_mean(x_new, x_forward_raw).to(**self.tkwargs)
        else:
            mean_x = self.single_mean(x_new).to(**self.tkwargs)
        covar_x = self.covar_module(x_new)
        covar_x.n_grad_dims = dz if x_new.requires_grad else 0
        if len(self.calibration_id) > 0 and self.training:
            covar_x.calib = self._calibration(x, dz)
        return MultivariateNormal(mean_x, covar_x)

    # ---- mean functions ------------------------------------------------------------------------------
    def single_m_gp_register(self, size=1, m_gp_type='single_zero', wm='mean_module'):
        if m_gp_type == 'single_constant':
            setattr(self, wm, ConstantMean(prior=NormalPrior(0., 1)))
        elif m_gp_type == 'single_zero':
            setattr(self, wm, ZeroMean())
        else:
            raise NotImplementedError(m_gp_type)

    def multi_m_gp_register(self, train_x, supported_multi_m_gp_functions, m_gp_ref):
        size = train_x.shape[1]
        if self.m_gp in supported_multi_m_gp_functions:
            for i in range(self.num_sources + 1):
                m_gp_type = 'single_' + m_gp_ref if i == 0 else 'single' + self.m_gp[8:]
                self.single_m_gp_register(size, m_gp_type=m_gp_type, wm='mean_module_' + str(i))

    def single_mean(self, x):
        return getattr(self, 'mean_module')(x)

    def multi_mean(self, x, x_forward_raw):
        """gp_plus.py:529-534, without the per-row module calls: mean_i = constant of source int(x_raw[i, -1])."""
        src = x_forward_raw[:, -1].to(torch.int64)
        mean_x = torch.zeros(x.shape[0], dtype=self.tkwargs['dtype'], device=x.device)
        for s in range(self.num_sources + 1):
            mod = getattr(self, 'mean_module_' + str(s))
            if isinstance(mod, ConstantMean):
                mean_x = torch.where(src.to(x.device) == s, mod.constant.to(mean_x).expand(x.shape[0]), mean_x)
        return mean_x

    # ---- fit -----------------------------------------------------------------------------------------
    def fit(self, add_prior: bool = True, num_restarts: int = 64, theta0_list: Optional[List[np.ndarray]] = None,
            jac: bool = True, options: Dict = {}, n_jobs: int = -1, method='L-BFGS-B', constraint=False, bounds=False,
            regularization_parameter: List[int] = [0, 0], optim_type='scipy', objective: str = "mll", folds=None,
            gradients=None, keep_restarts: int = 0):
        """gp_plus.py:547-599.  On a GPU device the reference always ends in ``fit_model_torch`` (64 restarts for
        'adam_torch', otherwise a warning and 4 restarts) — reproduced here.  The CPU branches
        (scipy / continuation drivers) do not exist in this build: the exact-GP path only runs on the MI355X.
        ``objective``: "mll" (the exact marginal log-likelihood, as the reference) or "loo" (the leave-one-out log
        pseudo-likelihood).  Both take the same route: all restarts advance together, one batched evaluation per Adam step replayed
        as a HIP graph, while the problem is small enough (see below); otherwise, and under ``settings.batched_restarts(False)``,
        the restarts run one after the other, the leave-one-out objective then with every evaluation eager.
        ``objective="cv"`` with ``folds=`` (an int k, one integer label per training row — ``cv.group_labels`` makes them from
        columns of X — or a ``cv.FoldIndex``) maximises the grouped cross-validation log pseudo-likelihood: always the sequential,
        eager route.  ``objective="gek"`` with ``gradients=(Xg, dY)``, ``(Xg, dY, noise)`` or ``(Xg, dY, noise, observed)`` —
        the arguments of ``condition_on_gradients`` — trains on the joint marginal likelihood of the targets and of the observed
        gradients (``gpcore.GradientEnhancedMarginalLogLikelihood``).  It takes the batched route too, under the conditions above
        evaluated at n = N + q rows (q observed gradient entries), every step an eager batched evaluation
        (``batched.batched_gek_mll``; no replayed graph); otherwise, and under ``settings.batched_restarts(False)``, the restarts run
        one after the other.  Afterwards ``condition_on_gradients`` on the same data gives the gradient-enhanced posterior at the
        fitted hyperparameters.
        ``keep_restarts=K`` (batched routes only) keeps the K restarts with the smallest finite last loss instead of discarding all
        but the winner: afterwards ``self.restart_ensemble`` is an ``ensemble.HyperparameterEnsemble`` of them with
        ``weights="posterior"``, member 0 the winner that is loaded into the model (fewer members when fewer restarts end finite);
        without the keyword it is None.  The fit itself — iterates, return value, loaded parameters — is the same either way.  On a
        route that is not batched ("cv", N above the batched kernels' range or memory, ``settings.batched_restarts(False)``, a
        calibrated model) ``keep_restarts > 0`` raises ``NotImplementedError`` before any fitting starts."""
        from ..optim.mll_torch import check_objective_folds, check_objective_gradients
        folds = check_objective_folds(objective, folds, int(self.train_targets.shape[0]))
        gradients = check_objective_gradients(objective, gradients)
        keep_restarts = int(keep_restarts)
        if keep_restarts < 0:
            raise ValueError(f"keep_restarts must be 0 or a positive count (got {keep_restarts})")
        rows = int(self.train_targets.shape[0])
        if objective == "gek":
            # the joint matrix has n = N + q rows, q the observed gradient entries: the batched route is judged at that size
            dY = torch.as_tensor(gradients[1])
            observed = gradients[3] if len(gradients) == 4 else None
            rows += int(dY.numel() if observed is None else torch.as_tensor(observed).expand(dY.shape).sum())
        if keep_restarts > 0:
            why = self._restarts_not_batched(objective, rows)  # (host work only: no device is touched)
            if why is not None:
                raise NotImplementedError(f"keep_restarts is available on the batched restarts only: {why}")
        self.restart_ensemble = None
        if objective != "mll":
            self._refuse_calibrated(f'objective="{objective}"', "only the exact marginal likelihood has a gradient by theta")
        if optim_type == 'adam_torch_batched':
            self._refuse_calibrated("optim_type='adam_torch_batched'", "the batched restarts have no gradient by theta")
        print("## Learning the model's parameters has started ##")
        if self.tkwargs['device'].type != 'cuda':
            raise RuntimeError("this build evaluates the marginal likelihood only on an MI355X (device='cuda'); "
                               "there is no CPU path")
        if optim_type in ('adam_torch', 'adam_torch_batched'):
            restarts = 64  # gp_plus.py:557
        else:
            warnings.warn('The model is built to run on CUDA (GPU), but the current optimization type is invalid for '
                          'this configuration. So, the optimizer is now using adam_torch to train the model.')
            restarts = 4   # gp_plus.py:566
        # The reference runs the restarts one after the other.  Here they advance together (one batched evaluation per Adam
        # iteration: same start points in the same RNG order, same per-run optimiser and early stop, same winner —
        # optim/mll_batched.py) while the problem is small enough for that to pay and for the B x 3 N^2 workspace to fit;
        # settings.batched_restarts(False) restores the sequential loop, 'adam_torch_batched' asks for the batched one.
        if objective == "cv":
            batched = False
        elif objective == "gek":
            batched = self._restarts_fit_one_batch(restarts + 1, rows)
        else:
            batched = optim_type == 'adam_torch_batched' or self._restarts_fit_one_batch(restarts + 1)
        extra = {k: v for k, v in (("folds", folds), ("gradients", gradients)) if v is not None}
        if batched:
            from ..optim import fit_model_torch_batched
            out = fit_model_torch_batched(self, lr_default=0.01, num_iter=100, num_restarts=restarts, break_steps=50,
                                          objective=objective, keep=keep_restarts, **extra)
            kept = fit_model_torch_batched.last_restarts
            if kept is not None and kept.losses.numel() > 0:
                from ..ensemble import HyperparameterEnsemble
                self.restart_ensemble = HyperparameterEnsemble(self, kept.states, losses=kept.losses, weights="posterior",
                                                               num_data=kept.num_data)
        else:
            if keep_restarts > 0:
                raise NotImplementedError("keep_restarts is available on the batched restarts only: the restarts of this fit do "
                                          "not fit the device's free memory as one batch")
            out = fit_model_torch(model=self, model_param_groups=None, lr_default=0.01, num_iter=100,
                                  num_restarts=restarts, break_steps=50, objective=objective, **extra)
        print("## Learning the model's parameters is successfully finished ##")
        return out

    def _restarts_not_batched(self, objective: str, n: int) -> Optional[str]:
        """Why the restarts of a fit with ``n`` factored rows cannot take the batched route, as far as the host can tell (None: the
        device's free memory decides, ``_restarts_fit_one_batch``)."""
        from .. import settings as gpp_settings
        from ..optim.mll_batched import BATCHED_MAX_N

        if objective == "cv":
            return 'objective="cv" has no batched form'
        if len(self.calibration_id) > 0:
            return "the batched restarts have no gradient by calibration parameters"
        if not gpp_settings.batched_restarts.value():
            return "settings.batched_restarts is off"
        if n > BATCHED_MAX_N:
            return f"{n} rows are beyond the batched kernels' range ({BATCHED_MAX_N})"
        return None

    def _restarts_fit_one_batch(self, B: int, n: Optional[int] = None) -> bool:
        """True when ``B`` restarts of this model should be evaluated together: batched restarts enabled, N within the batched
        kernels' range, and three B x N x N fp64 buffers within a third of the device memory that is free right now.  ``n``: the
        rows of the matrix that is factored where that is not N (objective="gek": N + q with q gradient observations)."""
        from .. import settings as gpp_settings
        from ..backend import row_stride
        from ..optim.mll_batched import BATCHED_MAX_N

        if not gpp_settings.batched_restarts.value() or len(self.calibration_id) > 0:
            return False  # (calibration parameters: the batched evaluation has no gradient by theta)
        N = int(self.train_targets.shape[0]) if n is None else int(n)
        if N > BATCHED_MAX_N:
            return False
        need = 3 * B * N * row_stride(N) * 8
        free, _ = torch.cuda.mem_get_info(self.tkwargs['device'])
        return need <= free // 3

    def fill_nan_with_mean(self, train_x, cal_ID):
        if torch.isnan(train_x).any():
            if len(cal_ID) == 0:
                print("There are NaN values in the data, which will be filled with column-wise mean values.")
            else:
                print("There are NaN values in the data, which will be estimated in calibration process")
            col_means = torch.nanmean(train_x, dim=0)
            nan_indices = torch.isnan(train_x)
            train_x[nan_indices] = col_means.repeat(train_x.shape[0], 1)[nan_indices]
        return train_x

    # ---- prediction / evaluation -----------------------------------------------------------------------
    def predict(self, Xtest, return_std=True, include_noise=True):
        Xtest = data_type_check(Xtest)
        with torch.no_grad():
            return super().predict(Xtest.to(self.tkwargs['device']), return_std=return_std, include_noise=include_noise)

    def predict_with_grad(self, Xtest, return_std=True, include_noise=True):
        """gp_plus.py:626-628: ``predict`` without ``torch.no_grad()``.  The mean and std are autograd-connected to Xtest's
        quantitative columns (categorical columns get zero gradient, as the reference's index lookup gives) and to the model's
        parameters, with gpytorch's default detach_test_caches (Ky and alpha constant); backward by gpp_cross_grad."""
        from .. import settings as gpp_settings

        Xtest = data_type_check(Xtest)
        with gpp_settings.differentiable_predictions(True):
            return super().predict(Xtest.to(self.tkwargs['device']), return_std=return_std, include_noise=include_noise)

    def loo_predict(self):
        """Leave-one-out predictions at the training points: ``(mean, std)`` of p(y_i | X, y_-i) for every i, in the units of the
        training targets, from the cached factorisation in O(N^2) — mu_i = y_i - alpha_i / (Ky^-1)_ii, sigma_i^2 = 1 / (Ky^-1)_ii
        (Rasmussen & Williams 5.4.2), the diagonal read off the inverse factor by gpp_loo_scalars.  The variance is that of the
        held-out OBSERVATION (its noise included)."""
        from ..linalg import loo_moments

        self.eval()
        with torch.no_grad():
            cache = self._ensure_prediction_cache()
            mu, s2 = loo_moments(cache, self.train_targets)
            return self.y_min + self.y_std * mu, s2.sqrt() * torch.abs(self.y_std)

    def cv_predict(self, folds, return_std=True, generator=None):
        """Held-out predictions at the training points under grouped cross-validation: the mean (and std) of p(y_F | X, y_-F) at
        every row of every fold F, in the units and conventions of ``loo_predict`` (training-target units, the held-out
        observation's noise included).  ``folds``: an int k (a random partition drawn from the CPU ``generator``, or a fixed seed),
        one integer label per training row (``cv.group_labels(X, columns)`` for leave-one-level-combination-out or
        leave-one-source-out), or a ``cv.FoldIndex``.  From the cached factorisation: mu_F = y_F - P_FF^-1 alpha_F and
        diag(P_FF^-1) with P = Ky^-1, every fold in one batched sequence per size bucket (gpp_cv_blocks); nothing is factored again."""
        from ..cv import FoldIndex
        from ..linalg import cv_moments

        folds = FoldIndex.make(folds, int(self.train_targets.shape[0]), generator=generator)
        self.eval()
        with torch.no_grad():
            cache = self._ensure_prediction_cache()
            mu, s2 = cv_moments(cache, self.train_targets, folds)
            mean = self.y_min + self.y_std * mu
            return (mean, s2.sqrt() * torch.abs(self.y_std)) if return_std else mean

    def _check_new_rows(self, X):
        """``condition_on``: every categorical level and — where sources carry a mean or a noise of their own — every source of the
        new rows must occur in the training data (the level lookup renumbers the levels of [training; new] rows jointly: an unseen
        one would shift the training rows' own)."""
        cat = [int(c) for c in self.qual_dict_list.tolist()]
        cols = list(cat)
        # (not hasattr(likelihood, 'fidel_indices'): GPR.predict leaves that attribute on a single-noise likelihood too)
        if (self.m_gp.startswith('multi') or isinstance(self.likelihood, Multifidelity_likelihood)) and X.shape[1] - 1 not in cols:
            cols.append(X.shape[1] - 1)
        if not cols:
            return
        tr = self.train_inputs[0]
        seen = getattr(self, '_seen_levels', None)  # (the training rows' values per column, read from the device once)
        if seen is None or seen[0] is not tr or seen[1] != tr._version:
            host = tr.detach().cpu()
            seen = (tr, tr._version, {c: set(host[:, c].tolist()) for c in cols})
            self._seen_levels = seen
        Xh = X.detach().cpu()
        for c in cols:
            new = set(Xh[:, c].tolist()) - seen[2][c]
            if new:
                what = "categorical level" if c in cat else "source"
                raise ValueError(f"condition_on: column {c} holds a {what} the model has not seen: {sorted(new)}")

    def _after_copy(self, child):
        import weakref

        for enc in child.A_matrix:  # (a deep copy keeps a weak reference as it is: the encoders would read THIS model's weights)
            object.__setattr__(enc, '_owner', weakref.ref(child))
        child._cat_cache = {}
        child.__dict__.pop('_seen_levels', None)
        child._calib_cache, child._calib_cols = None, {}

    # ---- posterior of the gradient -------------------------------------------------------------------
    def _gradient_rows(self, X, what: str):
        """The rows of ``predict_gradient`` / ``active_subspace``, validated on the host."""
        X = self._alc_rows(X, "Xtest" if what == "predict_gradient" else "X", what)
        if int(self.quant_index.numel()) == 0:
            raise ValueError(f"{what}: the model has no quantitative input column to differentiate")
        return X

    def _gradient_operands(self, X, what: str):
        """(cache, feature rows, first differentiated feature, their count) for the validated rows ``X``."""
        p = int(self.quant_index.numel())
        from ..gpcore.module import Module

        cache, _, _ = self._score_preamble(what, ())
        with torch.no_grad():  # (the rows go to the device after the cache is built, not before as the scores' row sets do)
            Us = Module.__call__(self, X.to(self.train_inputs[0])).lazy_covariance_matrix.U1
        return cache, Us, Us.shape[1] - p, p

    def predict_gradient(self, Xtest, return_std=True, return_cov=False):
        """Posterior of the gradient of the latent f with respect to the quantitative input columns at the rows of ``Xtest``:
        grad f(x) | data ~ N(g(x), S(x)), closed form for a GP.  Returns the mean (M, p) — and the std (M, p) of its components
        with ``return_std``, or instead the covariance (M, p, p) with ``return_cov`` — in the units of y per unit of the model's
        input column, columns in ``quant_index`` order.  The categorical columns are not differentiated and do not appear in the
        output.  This is the distribution ``predict_with_grad`` has no access to (autograd gives the slope of the posterior mean
        and std, not the spread of the slope).  Observation noise has no derivative and is never added; every supported prior
        mean has zero gradient in these columns.  std = sqrt(max(var, 0)) |y_std|; the covariance is returned unclamped, times
        y_std^2, bitwise symmetric.  The outputs carry no autograd graph.

        Nothing is factorised: the mean alone is one gpp_kernel_apply_grad call against the cached alpha, O(M N); the spread costs
        one product of the derivative cross block (gpp_cross_kernel_dx) with the cached inverse factor, O(N^2 M p), in chunks of
        ``linalg.GRAD_CHUNK_BYTES``, and gpp_point_gram for the covariance.  The model is put in eval mode and is otherwise
        untouched; a warm cache is reused, a model returned by ``condition_on`` included.  No reference counterpart.

        ``ValueError`` before any device work: wrong column count, an empty set, NaN / inf, a categorical level or source the model
        has not seen, a model without a quantitative column.  ``NotImplementedError`` under ``settings.sharded_evaluation`` or a
        graph capture."""
        from ..linalg import gradient_from_cache

        self._refuse_calibrated("predict_gradient", "the gradient by a calibrated column has no meaning on the calibrated source")
        cache, Us, d0, p = self._gradient_operands(self._gradient_rows(Xtest, "predict_gradient"), "predict_gradient")
        scale = self.y_std.detach().to(torch.float64)
        with torch.no_grad():
            if return_cov:
                mean, cov = gradient_from_cache(cache, Us, d0, p, "cov")
                return mean * scale, cov * scale ** 2
            if return_std:
                mean, var = gradient_from_cache(cache, Us, d0, p, "std")
                return mean * scale, var.clamp_min(0.0).sqrt() * scale.abs()
            return gradient_from_cache(cache, Us, d0, p, "mean") * scale

    def active_subspace(self, X, weights=None):
        """Active-subspace matrix C = E_x[grad f grad f^T] = sum_a w_a (g_a g_a^T + S_a) of the posterior over the rows of ``X``
        (``weights``: non-negative, not all zero, one per row; default 1 / M each), with (g_a, S_a) the gradient's posterior mean
        and covariance of ``predict_gradient``: the posterior expectation of the matrix, not the matrix of the posterior mean.
        Its leading eigenvectors are the directions of the quantitative inputs the response varies along; its diagonal holds the
        derivative-based global sensitivity measures nu_j.  Returns an ``ActiveSubspace`` with ``matrix`` (p x p, symmetric),
        ``eigenvalues`` (descending) and ``eigenvectors`` (columns) from ``torch.linalg.eigh``, ``mean_part`` = sum w g g^T,
        ``cov_part`` = sum w S and ``sensitivity`` = diag(matrix), in y^2 per squared input unit, ``quant_index`` order.  The
        per-point matrices are never stored (gpp_point_gram sums them).  Validation and refusals as in ``predict_gradient``, and
        ``ValueError`` for weights that are negative, not finite, all zero or of the wrong length."""
        from ..linalg import gradient_from_cache

        self._refuse_calibrated("active_subspace", "the gradient by a calibrated column has no meaning on the calibrated source")
        X = self._gradient_rows(X, "active_subspace")
        weights = _check_weights("active_subspace", weights, X.shape[0], "rows")
        cache, Us, d0, p = self._gradient_operands(X, "active_subspace")
        with torch.no_grad():
            mean_part, cov_part = gradient_from_cache(cache, Us, d0, p, "sum",
                                                      omega=None if weights is None else weights.to(Us.device))
            scale = self.y_std.detach().to(torch.float64) ** 2
            mean_part, cov_part = mean_part * scale, cov_part * scale
            matrix = mean_part + cov_part
            evals, evecs = torch.linalg.eigh(matrix)
            return ActiveSubspace(matrix=matrix, eigenvalues=evals.flip(0), eigenvectors=evecs.flip(1), mean_part=mean_part,
                                  cov_part=cov_part, sensitivity=torch.diagonal(matrix).clone())

    def variance_reduction(self, Xcand, Xref, weights=None, gradient=None, gradient_noise=None):
        """Active learning by expected variance reduction (``GPR.variance_reduction``, documented there), for runs that return y
        alone or y AND gradient components — the question an adjoint solver raises: is the gradient worth its cost here?

        ``gradient=None``: the scores of one noisy function value per row of ``Xcand`` (M_c), today's path, bit for bit.
        ``gradient=True`` (all p quantitative columns) or a length-p bool mask in ``quant_index`` order (the same components at
        every candidate): the pair (scores of a run that returns y and those components of dy/dx, scores of the value alone),
        M_c each, in y^2 units.  ``gradient_noise``: the variance of the gradient components in (y per input unit)^2 — a scalar, a
        length-p row or (M_c, p); entries under a False of the mask are not read; ``None`` takes
        ``gradient_enhanced.GRADIENT_NUGGET_REL`` times the prior curvature, as ``condition_on_gradients`` does.  The value's noise
        is that of the candidate's own source.  The score is the reduction ``condition_on`` followed by
        ``condition_on_gradients(..., observed=mask)`` at that row would give, whatever the observed values; nothing is conditioned
        and nothing is factorised: ``linalg.variance_reduction_block`` whitens the 1 + p' functionals of each candidate and one
        gpp_post_cross_lin_sq launch per chunk of candidates sums the squared posterior cross-covariances.
        Dividing the two scores by the two costs answers the question (``bayesian_optimizations.
        select_run_by_variance_reduction``).  No reference counterpart.

        ``ValueError`` before any device work, in addition to ``GPR.variance_reduction``'s: a model without a quantitative column,
        ``gradient=False``, a mask of another length or type or without a True, ``gradient_noise`` without ``gradient``, of a
        shape that does not broadcast, negative or not finite.  ``errors.NotPSDError`` when a candidate's block is not positive
        definite (it names the candidate): pass more gradient noise.  ``NotImplementedError`` for a model with calibration
        parameters, under ``settings.sharded_evaluation`` or a graph capture."""
        if gradient is None and gradient_noise is None:
            return super().variance_reduction(Xcand, Xref, weights)
        from ..gradient_enhanced import variance_reduction_of_runs

        self._refuse_calibrated("variance_reduction with gradient=", "the gradient by a calibrated column has no meaning on the "
                                "calibrated source")
        return variance_reduction_of_runs(self, None, Xcand, Xref, weights, gradient, gradient_noise)

    def condition_on_gradients(self, X, dY, noise=None, observed=None):
        """Gradient-enhanced Kriging on the fitted model: a ``GradientEnhancedPosterior`` of this model's training data plus observed
        gradients, made by bordering the cached factorisation in O(N^2 q), q = Mg p, without refactorising
        (``linalg.append_gradients_to_cache``: gpp_cross_kernel_dx, gpp_kernel_dxdx, gpp_chol_append).  ``X``: (Mg, columns of the
        training inputs), the points the gradients were observed at — rows of any source: gradients of a cheap source inform the
        others through the latent map like any other row.  ``dY``: (Mg, p), d y / d x over the quantitative columns in
        ``quant_index`` order, in y per input unit, as ``predict_gradient`` returns them; every supported prior mean is constant,
        so the gradients' prior mean is 0.  ``noise``: the variance of those observations in (y per input unit)^2, a scalar or
        anything that broadcasts to (Mg, p); ``None`` takes ``gradient_enhanced.GRADIENT_NUGGET_REL`` = 1e-6 times the prior
        curvature of each direction (the prior variance of that gradient component).  ``observed``: partial gradients — a bool
        mask that broadcasts to (Mg, p) (a length-p row: the same directions at every point) of the components of ``dY`` that were
        observed, as an adjoint gives them for the design variables only.  Entries of ``dY`` and ``noise`` under a False are not
        read and may be NaN or inf; q is then the number of True entries, every limit counts q, and both derivative blocks are
        built at that size (gpp_cross_kernel_dx_sel, gpp_kernel_dxdx_sel).  A point without an observed component is a
        ``ValueError``: drop the row.  Without a mask NaN is refused — it never means "missing".

        The receiver's data, parameters and cache are not modified (it is put in eval mode, as by ``predict``; without a cache it
        is factorised first).  The returned object holds a detached copy of the model without the N x N factors and offers
        ``predict(Xtest, return_std=True, include_noise=True)`` and ``predict_gradient(Xtest, return_std=True)`` in this model's
        conventions and units, ``variance_reduction`` (this model's, ``gradient=`` included), ``num_function_rows``,
        ``num_gradient_points``, ``num_gradient_observations`` (q) and ``observed`` — nothing else: no further appends, no sampling,
        LOO / CV, knowledge gradient or ``return_cov``, no training on the gradient data.  No reference
        counterpart.

        ``ValueError`` before any kernel runs: wrong column count or shapes, NaN / inf, Mg = 0, a categorical level or source the
        model has not seen, negative noise, a model without a quantitative column, a mask of the wrong shape or type or with an empty
        row, q > min(N, 2048).  ``errors.NotPSDError``
        when the gradient observations' Schur complement is not positive definite (duplicate points without noise): pass a larger
        ``noise``; the receiver stays usable.  ``NotImplementedError`` under ``settings.sharded_evaluation`` or a graph capture."""
        from ..gradient_enhanced import condition_on_gradients

        self._refuse_calibrated("condition_on_gradients", "gradient observations by a calibrated column are not defined")
        return condition_on_gradients(self, X, dY, noise, observed)

    def noise_value(self):
        return self.likelihood.noise_covar.noise.detach() * self.y_std ** 2

    def score(self, Xtest, ytest, plot_MSE=False, title=None, seperate_levels=False):
        """gp_plus.py:634-660 without the matplotlib part."""
        Xtest, ytest = data_type_check(Xtest), data_type_check(ytest)
        ytest = ytest.reshape(-1).to(self.tkwargs['device'])
        ypred = self.predict(Xtest.to(self.tkwargs['device']), return_std=False)
        mse = ((ytest.reshape(-1) - ypred) ** 2).mean()
        noise = self.noise_value()
        print('################MSE######################')
        print(f'MSE = {mse:.5f}')
        print('################Noise####################')
        print(f'The estimated noise parameter (varaince) is {noise}')
        print(f'The estimated noise std is {np.sqrt(noise.cpu())}')
        print('#########################################')
        return mse

    def evaluation(self, Xtest, ytest, verbose=True):
        """gp_plus.py:889-932: NLL (joint predictive density / M), MSE, MAE, RRMSE, interval score."""
        Xtest, ytest = data_type_check(Xtest), data_type_check(ytest)
        self.eval()
        dev = self.tkwargs['device']
        ytest = ytest.reshape(-1).to(dev)
        Xtest = Xtest.to(dev)
        ytest_sc = (ytest - self.y_min) / self.y_std
        with torch.no_grad():
            f_dist = self(Xtest)  # factors the training covariance with the TRAINING noise groups if not cached yet
            if hasattr(self.likelihood, 'fidel_indices'):
                self.likelihood.fidel_indices = Xtest[:, -1]  # the test points' own sources, as GPR.predict does
            trained_pred_dist = self.likelihood(f_dist)
            final_nlpd = gpmetrics.negative_log_predictive_density(trained_pred_dist, ytest_sc.to(torch.float64))
            final_mse = gpmetrics.mean_squared_error(trained_pred_dist, ytest_sc, squared=True)
            final_mae = gpmetrics.mean_absolute_error(trained_pred_dist, ytest_sc)
            alpha = 0.05
            mu_low, mu_up = trained_pred_dist.confidence_region()
            out = mu_up - mu_low
            out = out + (ytest_sc > mu_up) * 2 / alpha * (ytest_sc - mu_up)
            out = out + (ytest_sc < mu_low) * 2 / alpha * (mu_low - ytest_sc)
            IS = out.mean()
            final_mse = final_mse * (self.y_std) ** 2
            final_mae = final_mae * torch.abs(self.y_std)
            IS = IS * torch.abs(self.y_std)
            RRMSE = torch.sqrt(final_mse / torch.var(ytest))
        results = {'NLL': final_nlpd, 'MSE': final_mse, 'MAE': final_mae, 'RRMSE': RRMSE, 'IS': IS}
        if verbose:
            from tabulate import tabulate
            table_data = [['Negative Log-Likelihood (NLL)', final_nlpd], ['Mean Squared Error (MSE)', final_mse],
                          ['Mean Absolute Error  (MAE)', final_mae], ['Relative Root Mean Square Error (RRMSE)', RRMSE],
                          ['Interval Score (IS)', IS]]
            print(tabulate(table_data, headers=['Metric', 'Value'], tablefmt='fancy_grid', colalign=("left", "left")))
        return results

    def get_params(self, name=None):
        params = {n: value for n, value in self.named_parameters()}
        print('###################Parameters###########################')
        if name is None:
            print(params)
            return params
        key = {'Mean': 'mean_module.constant', 'Sigma': 'covar_module.raw_outputscale',
               'Noise': 'likelihood.noise_covar.raw_noise'}.get(name)
        if name == 'Omega':
            for n in params.keys():
                if 'raw_lengthscale' in n and params[n].numel() > 1:
                    key = n
        print(params[key])
        return params[key]

    def sample_y(self, size=1, X=None, plot=False):
        """gp_plus.py:985-998: ``size`` draws of ``likelihood(self(X))`` in eval mode, shape (size, len(X)), in the scaled
        target space (no un-scaling), at the training inputs by default.  At the training inputs the covariance is built as
        T - T Ky^-1 T + diag(noise) from the cached factor (gpp_post_cov_train); elsewhere as Kss + diag(noise) - V V^T."""
        if plot:
            raise NotImplementedError("plotting (visual/) is out of scope of this build; plot the returned draws instead")
        X = self.train_inputs[0] if X is None else data_type_check(X).to(self.tkwargs['device'])
        self.eval()
        with torch.no_grad():
            out = self._likelihood_of_rows(self(X), X)  # (the points' own sources, as evaluation() does)
            return out.sample(sample_shape=torch.Size([size]))

    def sample_paths(self, size=1, num_features=2048, generator=None):
        """``size`` draws of the posterior FUNCTION as a :class:`~gpplus_amd.pathwise.PosteriorPaths` (Matheron's rule on
        ``num_features`` random Fourier features of the prior): built once from the cached factor in O(N^2 size), then
        ``paths(X)`` evaluates every draw at any inputs in O(N + num_features) per point and draw — the same function at every
        call, which ``sample_y`` (a fresh vector per call, O(M^3)) cannot offer.  The draws are of the latent function, without
        observation noise, in the scaled target space of ``sample_y``, and carry no autograd graph.  ``generator``: a CPU
        ``torch.Generator`` (all random numbers are drawn on the CPU: one seed gives the same paths everywhere); None draws from
        torch's default generator.  No reference counterpart."""
        from ..pathwise import PosteriorPaths

        self.eval()
        with torch.no_grad():
            cache = self._ensure_prediction_cache()
        return PosteriorPaths(self, cache, size=size, num_features=num_features, generator=generator)

    def get_latent_space(self):
        if len(self.qual_dict_list) > 0:
            return [self.A_matrix[i](self.zeta[i].to(**self.tkwargs)).detach() for i in range(len(self.qual_kernel_columns))]
        print('No categorical Variable, No latent positions')
        return None

    def visualize_latent(self, *args, **kwargs):
        raise NotImplementedError("plotting (visual/) is out of scope of this build; use get_latent_space()")

    def Sobol(self, N: int = 10000, batch: int = 8192):
        """Main (S) and total (ST) Sobol sensitivity indices of the posterior mean, each of shape (1, p)
        (gp_plus.py:1148-1224): Saltelli's scheme on a 2p-dimensional Sobol sequence, p + 2 batched predictions of N
        points each from the cached factorisation (``gpp_cross_kernel`` + ``gpp_predict`` in chunks of ``batch`` rows, so
        N = 1e5 at N_train = 2e4 never materialises more than batch x N_train doubles).

        Differences from the reference, both forced: the sequence comes from ``scipy.stats.qmc.Sobol`` (unscrambled,
        origin skipped — the reference's ``sobol_seq`` package is not a dependency of this build), and EVERY categorical
        column is mapped to its level grid (the reference returns from inside its loop after the first categorical
        column, and returns nothing at all for a purely quantitative model)."""
        from scipy.stats import qmc

        if N < 1e5:
            warnings.warn('Increase N for accuracy!')
        X = self.train_inputs[0].detach().cpu().to(torch.float64)
        p = X.shape[1]
        gen = qmc.Sobol(d=2 * p, scramble=False)
        gen.fast_forward(1)
        sequence = torch.from_numpy(gen.random(N))
        mins, maxs = X.min(dim=0)[0], X.max(dim=0)[0]
        halves = []
        for part in (sequence[:, p:], sequence[:, :p]):
            scaled = mins + (maxs - mins) * part
            for j, col in enumerate(self.qual_dict_list):
                scaled[:, col] = (part[:, col] * (self.num_levels_per_var[j] - 1)).round()
            halves.append(scaled)
        A, B = halves

        def f(Z):
            out = [self.predict(Z[i:i + batch], return_std=False).detach().cpu().to(torch.float64).reshape(-1)
                   for i in range(0, Z.shape[0], batch)]
            return torch.cat(out).numpy().reshape(-1, 1)

        FA, FB = f(A), f(B)
        S, ST = np.zeros((p, 1)), np.zeros((p, 1))
        for i in range(p):
            ABi = A.clone()
            ABi[:, i] = B[:, i]
            Fi = f(ABi)
            S[i, :] = np.sum(FB * (Fi - FA), axis=0) / N
            ST[i, :] = np.sum((FA - Fi) ** 2, axis=0) / (2 * N)
        varY = np.var(np.concatenate([FA, FB]), axis=0)
        return (S / varY).T, (ST / varY).T

    # ---- categorical encoding ---------------------------------------------------------------------------
    def zeta_matrix(self, num_levels, embedding_dim: int, batch_shape=torch.Size()):
        """gp_plus.py:1027-1073."""
        if any([i == 1 for i in num_levels]):
            raise ValueError('Categorical variable has only one level!')
        if embedding_dim == 1:
            raise RuntimeWarning('1D latent variables are difficult to optimize!')
        for level in num_levels:
            if embedding_dim > level - 0:
                raise RuntimeWarning('The LV dimension can atmost be num_levels-1. '
                                     'Setting it to %s in place of %s' % (level - 1, embedding_dim))
        perm = torch.tensor(list(product(*[torch.arange(l).tolist() for l in num_levels])), dtype=torch.int64)
        perm_dic = {}
        for i, row in enumerate(perm):
            perm_dic.setdefault(str(row.tolist()), i)
        perm_one_hot = torch.concat([torch.nn.functional.one_hot(perm[:, i]) for i in range(perm.size()[1])], axis=1)
        return perm_one_hot, perm, perm_dic

    def transform_categorical(self, x: torch.Tensor, perm_dict=[], zeta=[]):
        """gp_plus.py:1077-1095: level combination -> row of zeta, through a vectorised mixed-radix index (the
        reference's str(row)->dict lookup enumerates itertools.product in exactly that order)."""
        if x.dim() == 1:
            x = x.reshape(-1, 1)
        if self.training is False:
            # reference: x = setlevels(x) on the joint [train; test] categorical block (gp_plus.py:1081-1082 under
            # ExactGP's eval-mode forward on cat([train_x, x])).  Equivalent here: levels from train + x together.
            i = len(self.qual_kernel_columns) - 1
            tr = self.train_inputs[0][:, self.qual_kernel_columns[i]].to(torch.int64).reshape(-1, x.shape[1]).cpu()
            joint = setlevels(torch.cat([tr, x.cpu()], dim=0))
            x = torch.as_tensor(joint)[tr.shape[0]:].to(torch.int64)
        levels = [int(l) for l in self.perm[0].max(dim=0).values + 1] if len(self.perm) else []
        xc = x.cpu()
        if bool((xc < 0).any()) or any(bool((xc[:, c] >= levels[c]).any()) for c in range(xc.shape[1])):
            raise ValueError("The categorical input (or source indices) are not defined properly. "
                             "They should be integer values starting from zero. To solve the issue, "
                             "you can use the 'setlevels' function, which is a preprocessing function.")
        index = torch.zeros(xc.shape[0], dtype=torch.int64)
        for c in range(xc.shape[1]):  # itertools.product order = mixed radix, last column fastest
            index = index * levels[c] + xc[:, c]
        return zeta[index, :]


# ---------------------------------------------------------------------------------------------------------
class _TallLinear(torch.autograd.Function):
    """``x @ w.T`` for a TALL constant input x (N x L one-hot rows of the categorical levels, no gradient) and a small weight
    (d_z x L): the forward is the library GEMM; the weight gradient ``g.T @ x`` is a (d_z x N)(N x L) product with a 2 x 10 result and
    K = N, for which the BLAS picks one work-group (284 us at N = 10 000, 1.4 % of a C3 evaluation: profiles/EXPERIMENTS.md, round
    5).  Here it is 64 batched partial products over row blocks + one sum: a fixed summation order, ~15 us."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        return nn.functional.linear(x, w)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        n, nb = x.shape[0], 64
        m = (n // nb) * nb
        gw = torch.bmm(g[:m].reshape(nb, m // nb, g.shape[1]).transpose(1, 2), x[:m].reshape(nb, m // nb, x.shape[1])).sum(0)
        if m < n:
            gw = gw + g[m:].t() @ x[m:]
        return None, gw


def _linear_tall(x, w):
    """The manifold map of the training rows: the batched-gradient form for tall constant inputs on a GPU, F.linear otherwise."""
    # (above the batched-restart range, N <= 6144, whose driver vectorises the model's own code with vmap: plain ops there)
    if x.dim() == 2 and x.shape[0] > 6144 and not x.requires_grad and x.is_cuda and w.dim() == 2:
        return _TallLinear.apply(x, w)
    return nn.functional.linear(x, w)


class Linear_MAP(nn.Linear):
    """gp_plus.py:1456-1461."""

    def forward(self, input, transform=lambda x: x):
        if self.bias is None:
            return _linear_tall(input, transform(self.weight))
        return nn.functional.linear(input, transform(self.weight), self.bias)


class FFNN(nn.Module):
    """Deterministic manifold encoder (gp_plus.py:1227-1265): bias-free linear map (no hidden layers) or tanh MLP.
    As in the reference the weights are parameters OF THE GP MODEL (registered under the reference's names with N(0,1)
    priors); this module only remembers those names and reads the live tensors from its owner at call time, so the
    encoder follows ``model.to(...)`` / ``load_state_dict`` (a CPU->GPU move re-creates Parameter objects)."""

    def __init__(self, GP_Plus, input_size, num_classes, layers, name):
        super(FFNN, self).__init__()
        import weakref

        object.__setattr__(self, '_owner', weakref.ref(GP_Plus))
        self.hidden_num = len(layers)
        self.weight_names = []

        def _register(pname, prior_name, fan_in, fan_out):
            init = nn.Linear(fan_in, fan_out, bias=False)  # same default initialisation as the reference's nn.Linear
            GP_Plus.register_parameter(pname, nn.Parameter(init.weight.detach().clone()))
            GP_Plus.register_prior(name=prior_name, prior=NormalPrior(0., 1), param_or_closure=pname)
            self.weight_names.append(pname)

        if self.hidden_num > 0:
            _register(str(name) + 'fci', 'latent_prior_fci', input_size, layers[0])
            for i in range(1, self.hidden_num):
                _register(str(name) + 'h' + str(i), 'latent_prior' + str(i), layers[i - 1], layers[i])
            _register(str(name) + 'fce', 'latent_prior_fce', layers[-1], num_classes)
        else:
            _register(name, 'latent_prior_' + name, input_size, num_classes)

    def _weights(self):
        owner = self._owner()
        return [getattr(owner, n) for n in self.weight_names]

    def forward(self, x, transform=lambda x: x):
        ws = self._weights()
        if self.hidden_num > 0:
            for w in ws[:-1]:
                x = torch.tanh(nn.functional.linear(x, w))
            return nn.functional.linear(x, ws[-1])
        return _linear_tall(x, transform(ws[0]))
