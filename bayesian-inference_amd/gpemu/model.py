"""DeviceModel: one emulation group resident on one MI355X (a libgpemu model handle)."""
from __future__ import annotations

import ctypes as C
import math
import sys

import numpy as np

from . import _lib
from ._lib import as_f64, check, ptr

RBF, MATERN = 0, 1
LOWRANK, EXACT = 0, 1


class DeviceModel:
    """Owns a ``gpemu_model`` handle.

    Arrays follow the results dict of the reference (ref: emulation.py:181-192):
    ``X_train`` = GaussianProcessRegressor.X_train_, per-PC ``ls/const/noise`` = kernel_
    hyper-parameters, ``alpha`` = alpha_, ``L`` = L_, ``components`` = pca.components_[:k],
    ``scaler_mean/scale`` = StandardScaler, ``cov_unexplained`` = ref: emulation.py:246-249.
    """

    def __init__(self, X_train, ls, alpha, L, components, scaler_mean, scaler_scale,
                 kernel_kind=RBF, nu=np.inf, const=None, noise=None, cov_unexplained=None, device=None):
        _lib.require_device()
        device = _lib.resolve_device(device)
        X_train = as_f64(X_train)
        N, d = X_train.shape
        ls = as_f64(ls)
        k = ls.shape[0]
        components = as_f64(components)
        F = components.shape[1]
        ls = as_f64(ls, (k, d))
        alpha = as_f64(alpha, (k, N))
        L = as_f64(L, (k, N, N))
        components = as_f64(components, (k, F))
        scaler_mean = as_f64(scaler_mean, (F,))
        scaler_scale = as_f64(scaler_scale, (F,))
        const_a = None if const is None else as_f64(const, (k,))
        noise_a = None if noise is None else as_f64(noise, (k,))
        cu = None if cov_unexplained is None else as_f64(cov_unexplained, (F, F))
        kind_arg, nu_arg = _lib.kernel_args(kernel_kind, nu)
        h = C.c_void_p()
        check(_lib.lib().gpemu_model_create(
            C.byref(h), int(device), N, d, F, k, kind_arg,
            nu_arg, int(const is not None), int(noise is not None),
            ptr(X_train), ptr(ls), ptr(const_a), ptr(noise_a), ptr(alpha), ptr(L), ptr(components),
            ptr(scaler_mean), ptr(scaler_scale), ptr(cu)))
        self._h = h
        self.N, self.d, self.F, self.k, self.device = N, d, F, k, int(device)
        self._lik_key = None
        self.prior_box = None            # (lo, hi) of the last likelihood_setup
        # host copies of the back-projection (k F + 2 F doubles): sobol_indices forms its quadratic forms with them
        self._projection = (components.copy(), scaler_scale.copy(), scaler_mean.copy())

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().gpemu_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def sync(self):
        check(_lib.lib().gpemu_model_sync(self._h))

    def profile(self, enable=True):
        """Bracket every launch of the two hot kernels with HIP events (bench.py roofline leg)."""
        check(_lib.lib().gpemu_model_profile(self._h, int(bool(enable))))

    def profile_read(self):
        """{'trmm_vsq': (ms_total, launches), 'kstar': (ms_total, launches), 'live': (proposals inside the prior box,
        proposals) of the samplers' compacted half-steps since ``profile`` was called (``DeviceSampler.live_fraction``)}"""
        ms = np.zeros(2)
        n = np.zeros(2, dtype=np.int64)
        live = np.zeros(2, dtype=np.int64)
        check(_lib.lib().gpemu_model_profile_read(self._h, ptr(ms), ptr(n)))
        check(_lib.lib().gpemu_model_live_counts(self._h, ptr(live)))
        return {"trmm_vsq": (float(ms[0]), int(n[0])), "kstar": (float(ms[1]), int(n[1])),
                "live": (int(live[0]), int(live[1]))}

    # -- host-buffer API -----------------------------------------------------------------------
    def _X(self, X):
        X = np.array(X, ndmin=2, dtype=np.float64)
        X = np.ascontiguousarray(X)
        if X.shape[1] != self.d:
            raise ValueError(f"expected {self.d} parameters per row, got {X.shape[1]}")
        return X

    @staticmethod
    def _finite(X):
        """sklearn's GaussianProcessRegressor.predict validates its input (check_array: ValueError on NaN / inf; skl
        utils/validation.py), which is what the reference's predict path goes through (ref: emulation.py:497).  The
        cross-kernel on the matrix cores does not propagate a NaN coordinate into K_* (only into the mean), so the
        host entry points refuse non-finite queries the way the reference does.  log_posterior is not affected: a NaN
        parameter fails the box prior (-inf), as in ref: log_posterior.py:63-64."""
        if not np.isfinite(X).all():
            raise ValueError("Input X contains NaN or infinity.")
        return X

    def gp_predict(self, X):
        """(B,k) predictive means and variances of the k PCs (ref: emulation.py:494-499)."""
        X = self._finite(self._X(X))
        B = X.shape[0]
        mean = np.empty((B, self.k))
        var = np.empty((B, self.k))
        check(_lib.lib().gpemu_gp_predict(self._h, B, ptr(X), ptr(mean), ptr(var)))
        return mean, var

    def gp_predict_cov(self, X, X2=None, workspace_bytes=0):
        """Joint predictive covariance of every PC (skl _gpr.py:367-469, predict(X, return_cov=True)): ``mean``
        (M1, k) and ``cov`` (k, M1, M2) = kernel_(X, X2) - V1^T V2.  ``X2=None``: the symmetric form on X (the White
        noise on the diagonal, the output symmetric bit for bit).  ``workspace_bytes`` caps the device workspace
        (0: sized from free memory); the result does not depend on it."""
        X = self._finite(self._X(X))
        M1 = X.shape[0]
        X2a = None if X2 is None else self._finite(self._X(X2))
        M2 = M1 if X2a is None else X2a.shape[0]
        mean = np.empty((M1, self.k))
        cov = np.empty((self.k, M1, M2))
        check(_lib.lib().gpemu_gp_predict_cov(self._h, M1, ptr(X), M2, ptr(X2a), int(workspace_bytes), ptr(mean),
                                              ptr(cov)))
        return mean, cov

    def gp_sample(self, X, z):
        """Draws of every PC's GP at X (skl _gpr.py:498-531, sample_y): ``draws`` (k, M, n) = mean_p +
        chol(C_p + tau_p I) z_p for the standard normals ``z`` (k, M, n), and ``tau`` (k,), the jitter each PC's
        factor needed (0 first, then 1e-12 mean(diag C_p) 10^i, i = 0 .. 6).  Raises ``fit.LinAlgError`` if a PC's
        covariance is not positive definite at the last rung."""
        from .fit import LinAlgError
        X = self._finite(self._X(X))
        M = X.shape[0]
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.ndim != 3 or z.shape[0] != self.k or z.shape[1] != M or z.shape[2] < 1:
            raise ValueError(f"z must have shape ({self.k}, {M}, n_draws >= 1), got {z.shape}")
        n = z.shape[2]
        draws = np.empty((self.k, M, n))
        tau = np.empty(self.k)
        rc = _lib.lib().gpemu_gp_sample(self._h, M, ptr(X), n, ptr(z), ptr(draws), ptr(tau))
        if rc > 0:
            raise LinAlgError(_lib.last_error())
        check(rc)
        return draws, tau

    def predict_full(self, X, n_div=None):
        """central_value (B,F), cov (B,F,F) as ref: emulation.py:466-548 (n_div defaults to B)."""
        X = self._finite(self._X(X))
        B = X.shape[0]
        cv = np.empty((B, self.F))
        cov = np.empty((B, self.F, self.F))
        check(_lib.lib().gpemu_predict_full(self._h, B, ptr(X), float(B if n_div is None else n_div),
                                            ptr(cv), ptr(cov)))
        return cv, cov

    def expected_information_gain(self, X, features, y_err=None, cov=None, emulator_cov="mean", n_outer=4096, seed=0,
                                  exclude_self=False, batch=4096, workspace_bytes=0):
        """The expected information gain (``gpemu.experiment``) of measuring the observables ``features``
        (indices into this model's F features) with uncertainty ``y_err`` or ``cov``, given samples ``X (S, d)`` of the
        parameters: the result dict of ``gpemu.experiment.expected_information_gain`` with ``means`` this emulator's
        central values at X (``predict_full(n_div=1)``, in batches).  ``emulator_cov='mean'`` adds the average over the
        rows of the emulator's feature-space covariance (truncation term included) to the measurement's covariance, which
        stays constant as the estimator requires; ``'none'`` uses the measurement's alone.  A likelihood covariance that
        depends on theta -- the emulator's own, row by row -- is out of scope."""
        from . import experiment
        cand = dict(features=features, y_err=y_err, cov=cov)
        return experiment.chain_expected_information_gain([self], self._finite(self._X(X)), [cand], n_outer=n_outer,
                                                          seed=seed, emulator_cov=emulator_cov, exclude_self=exclude_self,
                                                          batch=batch, workspace_bytes=workspace_bytes)["results"][0]

    @staticmethod
    def check_folds(fold, N):
        """The fold labels as an int32 vector [N] and their number; ValueError unless every label is in
        [0, n_folds), every fold is non-empty and 2 <= n_folds <= N (n_folds = max label + 1)."""
        fold = np.asarray(fold)
        if fold.shape != (N,):
            raise ValueError(f"fold must hold one label per design point ({N}), got shape {fold.shape}")
        if fold.size and not np.issubdtype(fold.dtype, np.integer):
            if not np.all(np.isfinite(fold)) or not np.all(fold == np.round(fold)):
                raise ValueError("fold labels must be integers")
        fold = fold.astype(np.int64)
        if fold.min() < 0:
            raise ValueError("fold labels must be >= 0")
        n_folds = int(fold.max()) + 1
        if n_folds < 2:
            raise ValueError("cross-validation needs at least 2 folds")
        if n_folds > N:
            raise ValueError(f"more folds ({n_folds}) than design points ({N})")
        empty = np.flatnonzero(np.bincount(fold, minlength=n_folds) == 0)
        if empty.size:
            raise ValueError(f"fold {int(empty[0])} is empty")
        return np.ascontiguousarray(fold, dtype=np.int32), n_folds

    def cross_validate(self, y_train, fold):
        """Cross-validation at the fitted hyper-parameters.

        ``y_train`` (N, k) = the group's ``Y_pca_truncated``; ``fold`` (N,) = fold label of every design point
        (0 .. n_folds - 1, every fold non-empty).  Each point is predicted by the GP of its PC refitted to the points
        of the other folds with theta (``kernel_``), the scaler and the PCA held at the full-data fit -- what
        ``GaussianProcessRegressor(kernel=gp.kernel_, alpha=alpha, optimizer=None).fit(X[R], y[R])
        .predict(X[I], return_std=True)`` gives.  Returns ``mean_pc`` (N, k), ``var_pc`` (N, k) (std squared),
        ``central_value`` (N, F) and ``variance`` (N, F), the diagonal of the reference's ``cov`` of one sample
        (ref: emulation.py:466-548)."""
        fold, n_folds = self.check_folds(fold, self.N)
        y = as_f64(y_train, (self.N, self.k))
        mean = np.empty((self.N, self.k))
        var = np.empty((self.N, self.k))
        cv = np.empty((self.N, self.F))
        vo = np.empty((self.N, self.F))
        check(_lib.lib().gpemu_model_cross_validate(self._h, n_folds, fold.ctypes.data_as(C.c_void_p), ptr(y),
                                                    ptr(mean), ptr(var), ptr(cv), ptr(vo)))
        return mean, var, cv, vo

    # -- posterior-predictive summaries ---------------------------------------------------
    def posterior_predictive(self, X, probabilities=(0.05, 0.5, 0.95), workspace_bytes=0):
        """Per-feature summaries of the group's prediction over the rows of ``X`` (S, d) -- typically the flattened
        chain: a dict with ``mean`` (F,), ``variance_parameters`` (F,) (population variance of the central value over
        the rows), ``variance_emulator`` (F,) (mean over the rows of the emulator variance of one sample, the diagonal
        of the reference's ``cov``, ref: emulation.py:466-548), ``variance`` (their sum: the law of total variance),
        ``quantiles`` (nq, F) of the central value (``np.quantile(..., method='linear')`` of exact device order
        statistics) and ``probabilities``.  ``probabilities=None`` or empty skips the quantiles.  Rows are not checked
        against a prior box; non-finite rows are refused as in ``gp_predict``.  ``workspace_bytes`` caps the device
        workspace (0: sized from free memory); the result, bit for bit, does not depend on it."""
        X = self._finite(self._X(X))
        plan = QuantilePlan(X.shape[0], probabilities)
        mean, vp, ve = np.empty(self.F), np.empty(self.F), np.empty(self.F)
        order = np.empty((self.F, max(plan.ranks.size, 1)))
        check(_lib.lib().gpemu_posterior_predictive(self._h, X.shape[0], ptr(X), int(plan.ranks.size), ptr(plan.ranks),
                                                    int(workspace_bytes), ptr(mean), ptr(vp), ptr(ve), ptr(order)))
        return plan.result(mean, vp, ve, order)

    def posterior_predictive_dev(self, dX_ptr, n_blocks, block_rows, block_stride_rows, ranks, dmean_ptr, dvar_param_ptr,
                                 dvar_emu_ptr, dorder_ptr, workspace_bytes=0, stream=None):
        """The device-pointer entry: row r of the S = n_blocks * block_rows rows is read at ``dX + ((r // block_rows) *
        block_stride_rows + r % block_rows) * d``; ``ranks`` is a host int64 array (may be empty), the outputs device
        pointers (0: not wanted).  ``stream``: see ``_stream`` (None: torch's current stream).  Waits for the stream
        before it returns."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        vp = lambda a: C.c_void_p(a) if a else None
        check(_lib.lib().gpemu_posterior_predictive_dev(
            self._h, C.c_void_p(dX_ptr), int(n_blocks), int(block_rows), int(block_stride_rows), int(ranks.size),
            ptr(ranks) if ranks.size else None, int(workspace_bytes), vp(dmean_ptr), vp(dvar_param_ptr), vp(dvar_emu_ptr),
            vp(dorder_ptr), C.c_void_p(self._stream(stream)[0])))

    def posterior_predictive_weighted(self, X, q, probabilities=(0.05, 0.5, 0.95), workspace_bytes=0):
        """``posterior_predictive`` of the rows of ``X`` (S, d) under every row of the fixed-point weights ``q`` (R_w, S)
        (``gpemu.reweight.fixed_weights``): a list with one dict per weight row, the keys of
        ``posterior_predictive`` plus ``total_weight`` (the integer ``Q = sum_s q_s``).  ``mean``, the two variances and
        ``variance`` are the weighted ones; ``quantiles`` (nq, F) are the inverted weighted ECDF of the central value at
        ``max(1, ceil(p Q))``, elements of the sample as ``gpemu.reweight.weighted_quantile``'s (not interpolated).  The
        result, bit for bit, does not depend on ``workspace_bytes``."""
        from . import reweight as RW
        X = self._finite(self._X(X))
        S = int(X.shape[0])
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(q)), dtype=np.uint64)
        if q.ndim != 2 or q.shape[1] != S or not 1 <= q.shape[0] <= RW.MAX_SCENARIOS:
            raise ValueError(f"q must be (R_w, {S}) with R_w in [1, {RW.MAX_SCENARIOS}]")
        R_w, Q = int(q.shape[0]), RW._totals(q)
        if np.any(Q == 0):
            raise ValueError("a weight row is all zero")
        p = np.zeros(0) if probabilities is None else np.asarray(probabilities, dtype=np.float64).reshape(-1).copy()
        tgt = RW.targets(p, Q) if p.size else np.zeros((R_w, 0), dtype=np.uint64)
        mean, vp, ve = (np.empty((R_w, self.F)) for _ in range(3))
        quant = np.empty((R_w, self.F, max(p.size, 1)))
        check(_lib.lib().gpemu_posterior_predictive_weighted(
            self._h, S, ptr(X), R_w, ptr(q), int(p.size), ptr(tgt) if p.size else None, int(workspace_bytes), ptr(mean),
            ptr(vp), ptr(ve), ptr(quant) if p.size else None))
        return weighted_postpred_result(mean, vp, ve, quant, p, Q)

    def posterior_predictive_weighted_dev(self, dX_ptr, n_blocks, block_rows, block_stride_rows, q, targets, dmean_ptr,
                                          dvar_param_ptr, dvar_emu_ptr, dquantiles_ptr, workspace_bytes=0, stream=None):
        """The device-pointer entry: the rows as ``posterior_predictive_dev`` reads them, ``q`` an int64 device tensor
        (R_w, S) of the fixed-point weights, ``targets`` a host uint64 array (R_w, n_targets) (may be empty), the outputs
        device pointers to (R_w, F) and (R_w, F, n_targets) (0: not wanted).  ``stream``: see ``_stream`` (None: torch's
        current stream), passed with ``workspace_bytes`` in a ``gpemu_call_ctx``.  Waits for the stream."""
        targets = np.ascontiguousarray(targets, dtype=np.uint64)
        R_w, nt = int(q.shape[0]), (int(targets.shape[1]) if targets.size else 0)
        vp = lambda a: C.c_void_p(a) if a else None
        ctx = _lib.CallCtx(self._stream(stream)[0], int(workspace_bytes))
        check(_lib.lib().gpemu_posterior_predictive_weighted_dev(
            self._h, C.c_void_p(dX_ptr), int(n_blocks), int(block_rows), int(block_stride_rows), R_w,
            C.c_void_p(q.data_ptr()), int(q.shape[1]), nt, ptr(targets) if nt else None, vp(dmean_ptr), vp(dvar_param_ptr),
            vp(dvar_emu_ptr), vp(dquantiles_ptr), C.byref(ctx)))

    # -- global sensitivity ----------------------------------------------------------------
    def design(self, reference, candidates, **kw):
        """``gpemu.design.Design`` of this one group: the sequential-design criterion (integrated variance reduction;
        DESIGN.md §4.32) over ``reference`` (S, d) and ``candidates`` (M, d); keywords as ``Design``'s."""
        from .design import Design
        return Design([self], reference, candidates, **kw)

    def _base_pair(self, A, B):
        A, B = self._finite(self._X(A)), self._finite(self._X(B))
        if A.shape != B.shape:
            raise ValueError(f"A and B must have the same shape, got {A.shape} and {B.shape}")
        return A, B

    def mean_pick_freeze(self, A, B):
        """PC means (d + 2, n, k) of the rows of ``A`` (slot 0), of ``B`` (slot 1) and of the pick-freeze rows
        ``AB_i`` = A with column i from B (slot 2 + i), without K_* or the variance GEMM."""
        A, B = self._base_pair(A, B)
        n = A.shape[0]
        Z = np.empty((self.d + 2, n, self.k))
        check(_lib.lib().gpemu_gp_mean_pick_freeze(self._h, n, ptr(A), ptr(B), ptr(Z)))
        return Z

    def sobol_moments(self, A, B, n_batches=16, workspace_bytes=0):
        """The moments of the pick-freeze PC means per batch of rows (row r in batch ``r * n_batches // n``), about
        the returned ``pivot`` (k,): a dict with ``count`` (T,), ``sumA``, ``sumB`` (T, k), ``C2`` (T, k, k),
        ``sumD`` (T, d, k), ``M`` and ``D`` (T, d, k, k) as include/gpemu.h defines them, and ``n``, ``n_batches``.
        ``workspace_bytes`` caps the chunk of PC means (0: sized from free memory); the result, bit for bit, does not
        depend on it."""
        A, B = self._base_pair(A, B)
        return self._sobol_moments(_lib.lib().gpemu_sobol_moments, A.shape[0], ptr(A), ptr(B), n_batches, workspace_bytes)

    def sobol_moments_dev(self, dA_ptr, dB_ptr, n, n_batches=16, workspace_bytes=0, stream=None):
        """``sobol_moments`` of base matrices resident on the device (``dA``, ``dB``: n x d doubles); the moments come
        back to the host.  Works on ``stream`` (``_stream``: None is torch's current stream, 0 the model's own) and waits for
        it.  Rows are not checked."""
        return self._sobol_moments(_lib.lib().gpemu_sobol_moments_dev, int(n), C.c_void_p(dA_ptr), C.c_void_p(dB_ptr),
                                   n_batches, workspace_bytes, C.c_void_p(self._stream(stream)[0]))

    def _sobol_moments(self, fn, n, A, B, n_batches, workspace_bytes, *tail):
        T, d, k = int(n_batches), self.d, self.k
        if not 1 <= T <= n:
            raise ValueError(f"n_batches must be in 1 .. n = {n}, got {n_batches}")
        out = {"pivot": np.empty(k), "count": np.empty(T, dtype=np.int64), "sumA": np.empty((T, k)),
               "sumB": np.empty((T, k)), "C2": np.empty((T, k, k)), "sumD": np.empty((T, d, k)),
               "M": np.empty((T, d, k, k)), "D": np.empty((T, d, k, k))}
        check(fn(self._h, n, A, B, T, int(workspace_bytes), ptr(out["pivot"]), ptr(out["count"]), ptr(out["sumA"]),
                 ptr(out["sumB"]), ptr(out["C2"]), ptr(out["sumD"]), ptr(out["M"]), ptr(out["D"]), *tail))
        out["n"], out["n_batches"] = n, T
        return out

    def sobol_moments_pairs(self, A, B, pairs=None, n_batches=16, workspace_bytes=0):
        """``sobol_moments`` (the same bytes) and the moments of the pair rows ``AB_ij`` = A with columns i < j from B
        (DESIGN.md §4.45): ``pairs`` (P, 2), ``sumD2`` (T, P, k), ``M2`` and ``D2`` (T, P, k, k) as include/gpemu.h
        defines them.  ``pairs=None``: all i < j in the order of ``gpemu.marginals.pair_indices``.  The workspace holds
        8 (d + 2 + P) k bytes per base row; the result, bit for bit, does not depend on it nor on which other pairs
        are asked for."""
        from . import sensitivity
        A, B = self._base_pair(A, B)
        n, T, d, k = A.shape[0], int(n_batches), self.d, self.k
        pairs = sensitivity.check_pairs(pairs, d)
        if not 1 <= T <= n:
            raise ValueError(f"n_batches must be in 1 .. n = {n}, got {n_batches}")
        P = pairs.shape[0]
        p32 = np.ascontiguousarray(pairs, dtype=np.int32)
        out = {"pivot": np.empty(k), "count": np.empty(T, dtype=np.int64), "sumA": np.empty((T, k)),
               "sumB": np.empty((T, k)), "C2": np.empty((T, k, k)), "sumD": np.empty((T, d, k)),
               "M": np.empty((T, d, k, k)), "D": np.empty((T, d, k, k)), "sumD2": np.empty((T, P, k)),
               "M2": np.empty((T, P, k, k)), "D2": np.empty((T, P, k, k))}
        check(_lib.lib().gpemu_sobol_moments_pairs(
            self._h, n, ptr(A), ptr(B), T, P, ptr(p32), int(workspace_bytes),
            *[ptr(out[key]) for key in ("pivot", "count", "sumA", "sumB", "C2", "sumD", "M", "D", "sumD2", "M2", "D2")]))
        out["n"], out["n_batches"], out["pairs"] = n, T, pairs
        return out

    def sobol_indices(self, A, B, n_batches=16, workspace_bytes=0, second_order=False, pairs=None):
        """First-order and total-effect Sobol' indices of every feature over the rows of ``A`` and ``B``, with
        batch-means standard errors: ``gpemu.sensitivity.indices_from_moments`` of ``sobol_moments`` with the
        components and the scaler the model was created with.  ``second_order=True`` adds the keys of
        ``gpemu.sensitivity.pair_indices_from_moments`` for ``pairs`` (None: all i < j) from ``sobol_moments_pairs``;
        the first-order keys keep their bytes."""
        from . import sensitivity
        if not second_order:
            if pairs is not None:
                raise ValueError("pairs needs second_order=True")
            return sensitivity.indices_from_moments(self.sobol_moments(A, B, n_batches, workspace_bytes), *self._projection)
        mom = self.sobol_moments_pairs(A, B, pairs, n_batches, workspace_bytes)
        out = sensitivity.indices_from_moments(mom, *self._projection)
        out.update(sensitivity.pair_indices_from_moments(mom, *self._projection))
        return out

    def likelihood_setup(self, y_exp, y_err, lo, hi, n_div=1.0, block_start=None, cov=None, sys_sources=None):
        """Data, box prior and the observable block boundaries of this group (``block_start`` =
        first feature of each observable plus F at the end; None = a single block).  ``y_exp`` of shape (C, F):
        one data vector per chain of a multi-chain sampler (closure tests), all against the same ``y_err``.

        Correlated uncertainties: ``cov`` (F, F) is the data covariance inside the observable blocks
        in place of ``diag(y_err**2)`` (zero across blocks); ``sys_sources`` (S, F), S <= 16, are this group's columns
        of fully correlated systematic sources.  With sources, evaluate all groups together (``logpost_groups``)."""
        y_exp = np.ascontiguousarray(y_exp, dtype=np.float64)
        if cov is None and sys_sources is None:
            if y_exp.ndim == 2:
                return self._likelihood_setup_chains(y_exp, y_err, lo, hi, n_div, block_start)
            y_exp = as_f64(y_exp, (self.F,))
            y_err = as_f64(y_err, (self.F,))
            lo = as_f64(lo, (self.d,))
            hi = as_f64(hi, (self.d,))
            bs = None
            nb = 0
            if block_start is not None:
                bs = np.ascontiguousarray(block_start, dtype=np.int64)
                nb = bs.size - 1
            check(_lib.lib().gpemu_likelihood_setup(self._h, ptr(y_exp), ptr(y_err), ptr(lo), ptr(hi),
                                                    float(n_div), nb, ptr(bs)))
            self._lik_key = (float(n_div), None if bs is None else tuple(bs.tolist()))
            self.prior_box = (lo.copy(), hi.copy())
            return
        n_chains = y_exp.shape[0] if y_exp.ndim == 2 else 1
        y_exp = as_f64(y_exp.reshape(n_chains, -1), (n_chains, self.F))
        y_err = as_f64(y_err, (self.F,))
        lo = as_f64(lo, (self.d,))
        hi = as_f64(hi, (self.d,))
        covd = None if cov is None else as_f64(cov, (self.F, self.F))
        S = 0
        src = None
        if sys_sources is not None:
            src = np.ascontiguousarray(sys_sources, dtype=np.float64)
            if src.ndim != 2 or src.shape[1] != self.F:
                raise ValueError(f"sys_sources must have shape (S, {self.F}), got {src.shape}")
            S = src.shape[0]
        bs, nb = None, 0
        if block_start is not None:
            bs = np.ascontiguousarray(block_start, dtype=np.int64)
            nb = bs.size - 1
        check(_lib.lib().gpemu_likelihood_setup_cov(self._h, int(n_chains), ptr(y_exp), ptr(y_err), ptr(covd), int(S),
                                                    ptr(src) if S > 0 else None, ptr(lo), ptr(hi), float(n_div), nb,
                                                    ptr(bs)))
        self._lik_key = (float(n_div), None if bs is None else tuple(bs.tolist()))
        self.prior_box = (lo.copy(), hi.copy())

    def _likelihood_setup_chains(self, y_exp, y_err, lo, hi, n_div, block_start):
        n_chains = y_exp.shape[0]
        y_exp = as_f64(y_exp, (n_chains, self.F))
        y_err = as_f64(y_err, (self.F,))
        lo = as_f64(lo, (self.d,))
        hi = as_f64(hi, (self.d,))
        bs, nb = None, 0
        if block_start is not None:
            bs = np.ascontiguousarray(block_start, dtype=np.int64)
            nb = bs.size - 1
        check(_lib.lib().gpemu_likelihood_setup_chains(self._h, int(n_chains), ptr(y_exp), ptr(y_err), ptr(lo), ptr(hi),
                                                       float(n_div), nb, ptr(bs)))
        self._lik_key = (float(n_div), None if bs is None else tuple(bs.tolist()))
        self.prior_box = (lo.copy(), hi.copy())

    def logpost(self, X, mode=LOWRANK):
        X = self._X(X)
        B = X.shape[0]
        out = np.empty(B)
        check(_lib.lib().gpemu_logpost(self._h, B, ptr(X), ptr(out), int(mode)))
        return out

    # -- per-observable log-likelihood terms -------------------------------------------
    @property
    def n_observable_blocks(self):
        """Observable blocks of the last ``likelihood_setup`` (``GpemuError`` -4 before it)."""
        n = C.c_int64()
        check(_lib.lib().gpemu_model_observable_blocks(self._h, C.byref(n)))
        return int(n.value)

    def _block_features(self):
        """Features of every observable block of the last ``likelihood_setup``: ``(n_obs,)``."""
        bs = getattr(self, "_lik_key", (None, None))[1]
        return np.array([self.F], dtype=np.int64) if bs is None else np.diff(np.asarray(bs, dtype=np.int64))

    def loglik_pointwise(self, X, normalised=False, chain=0):
        """``T (n_obs, B)``: the log-likelihood term of every observable block for the rows of ``X (B, d)`` -- the terms
        whose sum, for a row inside the prior box, is ``logpost`` (the same normalisation: no 2 pi constant;
        ``normalised`` adds ``-(F_o / 2) log 2 pi`` per block).  A likelihood: the box is not applied; a row with a
        non-finite coordinate gives NaN.  ``chain``: the data vector of a setup with several.  A setup with
        ``sys_sources`` raises ``GpemuError`` (code -5): the sources span the blocks."""
        X = self._X(X)
        T = np.empty((self.n_observable_blocks, X.shape[0]))
        check(_lib.lib().gpemu_loglik_pointwise(self._h, int(chain), X.shape[0], ptr(X), ptr(T)))
        if normalised:
            T -= 0.5 * math.log(2.0 * math.pi) * self._block_features()[:, None]
        return T

    def loglik_pointwise_dev(self, dX_ptr, n_blocks, block_rows, block_stride_rows, dT_ptr, ldt, chain=0, stream=None):
        """The device-pointer entry: rows in the block layout of ``posterior_predictive_dev``, ``T`` block-major with
        ``ldt >= n_blocks * block_rows`` doubles per observable.  Waits for the stream before it returns."""
        check(_lib.lib().gpemu_loglik_pointwise_dev(self._h, int(chain), C.c_void_p(dX_ptr), int(n_blocks), int(block_rows),
                                                    int(block_stride_rows), C.c_void_p(dT_ptr), int(ldt),
                                                    C.c_void_p(self._stream(stream)[0])))

    # -- derivatives with respect to the parameters -------------------------------------
    def gp_predict_grad(self, X):
        """``mean`` (B, k), ``var`` (B, k) and their Jacobians ``dmean`` (B, k, d), ``dvar`` (B, k, d) with respect to
        the query.  ``dvar`` is 0 where the variance was clipped at 0.  RBF and Matern nu = 1.5 / 2.5 / inf; other nu
        raise ``GpemuError`` (code -5).  Non-finite queries are refused as in ``gp_predict``."""
        X = self._finite(self._X(X))
        B = X.shape[0]
        mean = np.empty((B, self.k))
        var = np.empty((B, self.k))
        dmean = np.empty((B, self.k, self.d))
        dvar = np.empty((B, self.k, self.d))
        check(_lib.lib().gpemu_gp_predict_grad(self._h, B, ptr(X), ptr(mean), ptr(var), ptr(dmean), ptr(dvar)))
        return mean, var, dmean, dvar

    def logpost_grad(self, X, mode=LOWRANK):
        """``lp`` (B,) and ``grad`` (B, d) of the log-posterior after ``likelihood_setup``; rows outside the open box
        (a NaN parameter included) give ``lp = -inf`` and ``grad = 0``."""
        X = self._X(X)
        B = X.shape[0]
        lp = np.empty(B)
        grad = np.empty((B, self.d))
        check(_lib.lib().gpemu_logpost_grad(self._h, B, ptr(X), ptr(lp), ptr(grad), int(mode)))
        return lp, grad

    def logpost_grad_dev(self, dX_ptr, B, dlp_ptr, dgrad_ptr, mode=LOWRANK, stream=None):
        """``logpost_grad`` on device pointers.  ``stream`` as in ``logpost_dev`` (see ``_stream``)."""
        st, settle = self._stream(stream)
        check(_lib.lib().gpemu_logpost_grad_dev(self._h, int(B), C.c_void_p(dX_ptr), C.c_void_p(dlp_ptr),
                                                C.c_void_p(dgrad_ptr), int(mode), C.c_void_p(st)))
        settle()

    # -- device-pointer API (torch tensors on this device) ----------------------------------------------
    def _stream(self, stream):
        """``(handle, settle)`` of a ``_dev`` call.  ``stream`` is a stream handle as an integer -- 0: the model's own
        stream, which is a non-blocking one: not ordered with any torch stream, torch's default stream included; the
        caller synchronises before the call and ``sync()`` after it -- or None: torch's current stream on this device.
        Torch's default stream is the null stream, whose handle 0 the model-bound entries read as "the model's own
        stream": it is then waited for on the host before the call, and ``settle()`` waits for the model's stream after
        it, so that the call reads what the caller's torch work wrote and torch work that follows reads its results.  On
        any other torch stream the call is enqueued there and nothing waits.  Without torch in the process None is 0."""
        nothing = lambda: None
        if stream is not None:
            return int(stream), nothing
        torch = sys.modules.get("torch")
        if torch is None or not torch.cuda.is_initialized():
            return 0, nothing
        s = torch.cuda.current_stream(torch.device("cuda", self.device))
        if s.cuda_stream:
            return int(s.cuda_stream), nothing
        s.synchronize()
        return 0, self.sync

    def logpost_dev(self, dX_ptr, B, dout_ptr, mode=LOWRANK, stream=None):
        """``logpost`` on device pointers.  ``stream`` (see ``_stream``): None is torch's current stream -- on a side
        stream the call is enqueued there and does not wait; on torch's default stream it blocks the host, before and
        after.  A loop that must stay asynchronous there passes ``stream=0`` (the model's own stream) and orders it
        itself with ``sync()``."""
        st, settle = self._stream(stream)
        check(_lib.lib().gpemu_logpost_dev(self._h, int(B), C.c_void_p(dX_ptr), C.c_void_p(dout_ptr),
                                           int(mode), C.c_void_p(st)))
        settle()

    def gp_predict_dev(self, dX_ptr, B, dmean_ptr, dvar_ptr, stream=None):
        """``gp_predict`` on device pointers.  ``stream`` as in ``logpost_dev`` (see ``_stream``)."""
        st, settle = self._stream(stream)
        check(_lib.lib().gpemu_gp_predict_dev(self._h, int(B), C.c_void_p(dX_ptr), C.c_void_p(dmean_ptr),
                                              C.c_void_p(dvar_ptr), C.c_void_p(st)))
        settle()

    def gp_predict_cov_dev(self, dX1_ptr, M1, dX2_ptr, M2, dmean_ptr, dcov_ptr, workspace_bytes=0, stream=None):
        """``gp_predict_cov`` on device pointers (0: no X2 / no mean).  ``stream``: see ``_stream``; the entry waits for
        its stream before it returns."""
        st, settle = self._stream(stream)
        check(_lib.lib().gpemu_gp_predict_cov_dev(self._h, int(M1), C.c_void_p(dX1_ptr), int(M2),
                                                  C.c_void_p(dX2_ptr) if dX2_ptr else None, int(workspace_bytes),
                                                  C.c_void_p(dmean_ptr) if dmean_ptr else None, C.c_void_p(dcov_ptr),
                                                  C.c_void_p(st)))
        settle()

    def predict_full_dev(self, dX_ptr, B, n_div, dcv_ptr, dcov_ptr, stream=None):
        """``predict_full`` on device pointers.  ``stream`` as in ``logpost_dev`` (see ``_stream``)."""
        st, settle = self._stream(stream)
        check(_lib.lib().gpemu_predict_full_dev(self._h, int(B), C.c_void_p(dX_ptr), float(n_div),
                                                C.c_void_p(dcv_ptr), C.c_void_p(dcov_ptr), C.c_void_p(st)))
        settle()


def logpost_groups(models, X, mode=LOWRANK):
    """log-posterior of the rows of X summed over the emulation groups ``models`` (DeviceModel, one device, one
    parameter box), evaluated together: the term of correlated sources (``likelihood_setup(sys_sources=...)``) spans
    the groups, so with sources this is not the sum of the groups' ``logpost``."""
    models = list(models)
    if not models:
        raise ValueError("logpost_groups needs at least one model")
    X = models[0]._X(X)
    B = X.shape[0]
    out = np.empty(B)
    hs = (C.c_void_p * len(models))(*[m.handle for m in models])
    check(_lib.lib().gpemu_logpost_groups(hs, len(models), B, ptr(X), ptr(out), int(mode)))
    return out


def logpost_groups_grad(models, X, mode=LOWRANK):
    """``lp`` (B,) and ``grad`` (B, d) of the log-posterior summed over the emulation groups ``models`` (one device, one
    parameter box).  Groups with correlated sources are declined (``GpemuError``, code -5)."""
    models = list(models)
    if not models:
        raise ValueError("logpost_groups_grad needs at least one model")
    X = models[0]._X(X)
    B = X.shape[0]
    lp = np.empty(B)
    grad = np.empty((B, models[0].d))
    hs = (C.c_void_p * len(models))(*[m.handle for m in models])
    check(_lib.lib().gpemu_logpost_groups_grad(hs, len(models), B, ptr(X), ptr(lp), ptr(grad), int(mode)))
    return lp, grad


class QuantilePlan:
    """The order statistics a set of probabilities needs from S samples, and the assembly of a posterior-predictive
    result from the library's outputs (``gpemu.select``: numpy's ``linear`` virtual index and ``_lerp``)."""

    def __init__(self, S, probabilities):
        from . import select
        self.probabilities = (np.zeros(0) if probabilities is None
                              else np.asarray(probabilities, dtype=np.float64).reshape(-1).copy())
        if self.probabilities.size:
            self.ranks, self.ilo, self.ihi, self.t = select._bracket(int(S), self.probabilities)
        else:
            self.ranks = np.zeros(0, dtype=np.int64)

    def quantiles(self, order):
        """``order`` (F, n_ranks) -> (nq, F)."""
        from . import select
        if not self.probabilities.size:
            return np.zeros((0, order.shape[0]))
        return select.lerp(order[:, self.ilo].T, order[:, self.ihi].T, self.t[:, None])

    def result(self, mean, var_param, var_emu, order):
        return {"mean": mean, "variance_parameters": var_param, "variance_emulator": var_emu,
                "variance": var_param + var_emu, "quantiles": self.quantiles(order),
                "probabilities": self.probabilities}


def weighted_postpred_result(mean, var_param, var_emu, quantiles, probabilities, Q):
    """One dict per weight row from ``gpemu_posterior_predictive_weighted``'s outputs ``(R_w, F)`` and
    ``(R_w, F, nq)``: ``posterior_predictive``'s keys plus ``total_weight``."""
    p = np.asarray(probabilities, dtype=np.float64).reshape(-1)
    out = []
    for w in range(mean.shape[0]):
        qs = np.ascontiguousarray(quantiles[w, :, :p.size].T) if p.size else np.zeros((0, mean.shape[1]))
        out.append({"mean": mean[w], "variance_parameters": var_param[w], "variance_emulator": var_emu[w],
                    "variance": var_param[w] + var_emu[w], "quantiles": qs, "probabilities": p.copy(),
                    "total_weight": int(Q[w])})
    return out


POSTPRED_FIXED_BYTES = 32 << 20    # GPEMU_POSTPRED_FIXED_BYTES


def postpred_workspace_bytes(S, k, n_features):
    """``workspace_bytes`` with which ``posterior_predictive`` of S rows holds ``n_features`` features at a time (a
    multiple of 16 below F): the resident PC arrays, the fixed scratch, 8 S bytes per feature (include/gpemu.h)."""
    return 16 * int(S) * int(k) + POSTPRED_FIXED_BYTES + 8 * int(S) * int(n_features)


POSTPRED_PATHS = ("whole", "feature_blocked", "feature_block", "select_pass")    # enum gpemu_postpred_path


def postpred_path_counts():
    """Counters of enum gpemu_postpred_path (selection and posterior-predictive reduction), as an int64 array."""
    out = np.zeros(8, dtype=np.int64)
    n = _lib.lib().gpemu_postpred_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()


def hmc_path_counts():
    """Counters of enum gpemu_hmc_path (the HMC sampler's launches and the chain moments), as an int64 array."""
    out = np.zeros(8, dtype=np.int64)
    n = _lib.lib().gpemu_hmc_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()


def grad_path_counts():
    """Counters of enum gpemu_grad_path (the derivative launches), as an int64 array."""
    out = np.zeros(8, dtype=np.int64)
    n = _lib.lib().gpemu_grad_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()


def src_path_counts():
    """Counters of enum gpemu_src_path (the correlated-source launches), as an int64 array."""
    out = np.zeros(8, dtype=np.int64)
    n = _lib.lib().gpemu_src_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()
