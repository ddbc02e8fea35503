"""Sequential design: where should the expensive model be run next?  

Active learning in Cohn's sense -- integrated variance reduction -- at the fitted hyper-parameters.  For an emulation
group with PCs p, the two-set GP posterior covariance ``c_p`` (no noise), a reference set ``x_s`` with weights
``omega_s`` (posterior samples, or a space-filling sample of the prior box) and candidates ``x_c``:

    IV      = sum_p w_p sum_s omega_s c_p(x_s, x_s)
    A(c)    = sum_p w_p [sum_s omega_s c_p(x_s, x_c)^2] / (c_p(x_c, x_c) + tau_p)

``A(c)`` is the amount by which a model run at ``x_c`` (carrying noise variance ``tau_p``) lowers ``IV``.  ``w_p =
sum_f fw_f (scale_f components[p, f])^2`` carries the PCs' variances to the observables (``pc_weights``); the
truncation covariance does not depend on the design and drops out.  A PC whose denominator is at or below
``min_variance * kernel_.diag_p`` contributes exactly 0.  ``Design.select`` picks greedily: after each pick every
covariance is conditioned on it, by a rank-one update that the device keeps as one more row of its GEMM operands.
Hyper-parameters are not refitted between picks.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import check, ptr
from .rows import DeviceRows          # reference rows that already lie in device memory (a stored chain in place)

MAX_PICKS = 256
MAX_ROWS = 4194240
PATH_NAMES = ("scores", "chunk", "dp8", "dp16", "kind_rbf", "kind_m05", "kind_m15", "kind_m25", "kind_nu", "column")


def path_counts():
    """{name: count} of the design launches so far (enum gpemu_design_path)."""
    out = np.zeros(len(PATH_NAMES), dtype=np.int64)
    n = _lib.lib().gpemu_design_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    if n < 0:
        check(n)
    return dict(zip(PATH_NAMES, out.tolist()))


def pc_weights(model_or_arrays, feature_weights=None):
    """``w_p = sum_f fw_f (scaler_scale_f components[p, f])^2``, (k,): the weight of PC p's variance in ``sum_f fw_f
    var(observable f)``.  ``model_or_arrays``: a ``DeviceModel`` or ``(components (k, F), scaler_scale (F,))``.
    ``feature_weights`` (F,), default 1; ``1 / y_err^2`` counts variance in units of the data's."""
    if hasattr(model_or_arrays, "_projection"):
        comp, scale = model_or_arrays._projection[0], model_or_arrays._projection[1]
    else:
        comp, scale = model_or_arrays[0], model_or_arrays[1]
    comp = np.asarray(comp, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if comp.ndim != 2 or comp.shape[1] != scale.size:
        raise ValueError(f"components {comp.shape} and scaler_scale {scale.shape} do not match")
    fw = np.ones(scale.size) if feature_weights is None else np.asarray(feature_weights, dtype=np.float64).reshape(-1)
    if fw.size != scale.size:
        raise ValueError(f"expected {scale.size} feature weights, got {fw.size}")
    if not (np.isfinite(fw).all() and (fw >= 0).all()):
        raise ValueError("feature weights must be finite and >= 0")
    return ((comp * scale[None, :]) ** 2) @ fw


def _rows(what, X, d):
    X = np.ascontiguousarray(np.array(X, ndmin=2, dtype=np.float64))
    if X.ndim != 2 or X.shape[1] != d:
        raise ValueError(f"{what}: expected rows of {d} parameters, got shape {X.shape}")
    if not 1 <= X.shape[0] <= MAX_ROWS:
        raise ValueError(f"{what}: between 1 and {MAX_ROWS} rows, got {X.shape[0]}")
    if not np.isfinite(X).all():
        raise ValueError(f"{what} contains NaN or infinity")
    return X


def _nonneg(what, v, n):
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if v.size != n:
        raise ValueError(f"{what}: expected {n} values, got {v.size}")
    if not (np.isfinite(v).all() and (v >= 0).all()):
        raise ValueError(f"{what} must be finite and >= 0")
    return v


class _GroupDesign:
    """One ``gpemu_design`` handle: one emulation group."""

    def __init__(self, model, reference, weights, candidates, pcw, tau, min_variance, max_picks, workspace_bytes):
        self.k, self.M, self.pcw = model.k, candidates.shape[0], pcw
        h = C.c_void_p()
        L = _lib.lib()
        if isinstance(reference, DeviceRows):
            import torch
            dc = torch.from_numpy(candidates).to(torch.device("cuda", model.device))
            torch.cuda.current_stream(dc.device).synchronize()
            check(L.gpemu_design_create_dev(C.byref(h), model.handle, C.c_void_p(reference.address),
                                            *reference.layout[1:], ptr(weights), self.M, C.c_void_p(dc.data_ptr()), ptr(pcw),
                                            ptr(tau), float(min_variance), int(max_picks), int(workspace_bytes),
                                            reference.stream))
            del dc      # the handle holds its own copy
        else:
            check(L.gpemu_design_create(C.byref(h), model.handle, reference.shape[0], ptr(reference), ptr(weights), self.M,
                                        ptr(candidates), ptr(pcw), ptr(tau), float(min_variance), int(max_picks),
                                        int(workspace_bytes)))
        self._h, self._model = h, model       # the model must outlive the handle

    def scores(self, per_pc=False):
        s = np.empty(self.M)
        spc = np.empty((self.k, self.M)) if per_pc else None
        check(_lib.lib().gpemu_design_scores(self._h, ptr(s), ptr(spc)))
        return (s, spc) if per_pc else s

    def condition(self, i):
        check(_lib.lib().gpemu_design_condition(self._h, int(i)))

    def state(self, den=False):
        """(iv (k,), den (k, M) or None, picks so far)"""
        iv = np.empty(self.k)
        dn = np.empty((self.k, self.M)) if den else None
        n = C.c_int64()
        check(_lib.lib().gpemu_design_state(self._h, ptr(iv), ptr(dn), C.byref(n)))
        return iv, dn, int(n.value)

    def integrated_variance(self):
        return float(np.dot(self.pcw, self.state()[0]))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().gpemu_design_destroy(self._h)
            self._h = None


class Design:
    """The design criterion of one or several emulation groups over one reference set and one candidate set.

    ``models``: ``DeviceModel``s (one device handle each).  ``reference`` (S, d) host rows, or ``DeviceRows``;
    ``weights`` (S,) >= 0, normalised by the call (default 1 / S).  ``candidates`` (M, d).  ``feature_weights``: one
    (F_g,) vector per group (None entries: 1), or one merged vector together with ``feature_columns``, the groups'
    columns in it (what ``SortEmulationGroupObservables.group_layout`` returns: the way ``predict`` merges).  ``tau``:
    the noise variance of a new run per PC -- one (k_g,) vector per group, default the White level of each PC (0
    without one).  ``max_picks`` bounds the points that can be conditioned on; ``workspace_bytes`` the device memory
    of each group's handle (0: half of what is free); the results do not depend on it.

    Every argument is checked before the first device call.  A context manager; ``close()`` is idempotent."""

    def __init__(self, models, reference, candidates, weights=None, feature_weights=None, tau=None, min_variance=1e-6,
                 max_picks=32, workspace_bytes=0, feature_columns=None):
        self._groups = []
        models = list(models)
        if not models:
            raise ValueError("at least one model")
        d = models[0].d
        if any(m.d != d for m in models):
            raise ValueError("the models differ in their parameters")
        if d > 16 or any(m.k > 64 for m in models):
            raise ValueError("at most 16 parameters and 64 PCs per group")
        if isinstance(reference, DeviceRows):
            if reference.rows > MAX_ROWS:          # (the layout itself is DeviceRows' check)
                raise ValueError(f"reference: between 1 and {MAX_ROWS} rows, got {reference.rows}")
            S = reference.rows
        else:
            reference = _rows("reference", reference, d)
            S = reference.shape[0]
        candidates = _rows("candidates", candidates, d)
        if weights is not None:
            weights = _nonneg("weights", weights, S)
            if not weights.sum() > 0:
                raise ValueError("weights must have a positive sum")
        min_variance, max_picks, workspace_bytes = float(min_variance), int(max_picks), int(workspace_bytes)
        if not (np.isfinite(min_variance) and min_variance >= 0):
            raise ValueError("min_variance must be finite and >= 0")
        if not 0 <= max_picks <= MAX_PICKS:
            raise ValueError(f"max_picks must be in [0, {MAX_PICKS}]")
        if workspace_bytes < 0:
            raise ValueError("workspace_bytes must be >= 0")
        fws = self._split(feature_weights, feature_columns, models)
        pcws = [np.ascontiguousarray(pc_weights(m, fw)) for m, fw in zip(models, fws)]
        if tau is None:
            taus = [None] * len(models)
        else:
            taus = [tau] if len(models) == 1 and np.ndim(tau[0]) == 0 else list(tau)
            if len(taus) != len(models):
                raise ValueError("tau: one vector per group")
            taus = [None if t is None else _nonneg("tau", t, m.k) for t, m in zip(taus, models)]
        self.candidates, self.d, self.max_picks = candidates, d, max_picks
        self.picks = []
        try:
            for m, pcw, t in zip(models, pcws, taus):
                self._groups.append(_GroupDesign(m, reference, weights, candidates, pcw, t, min_variance, max_picks,
                                                 workspace_bytes))
        except Exception:
            self.close()
            raise

    @staticmethod
    def _split(feature_weights, feature_columns, models):
        if feature_weights is None:
            return [None] * len(models)
        if feature_columns is not None:
            fw = np.asarray(feature_weights, dtype=np.float64).reshape(-1)
            cols = list(feature_columns)
            if len(cols) != len(models):
                raise ValueError("feature_columns: one index array per group")
            return [fw[np.asarray(c, dtype=np.int64)] for c in cols]
        if len(models) == 1 and np.ndim(feature_weights[0]) == 0:
            return [feature_weights]
        fws = list(feature_weights)
        if len(fws) != len(models):
            raise ValueError("feature_weights: one vector per group, or a merged vector with feature_columns")
        return fws

    @classmethod
    def from_groups(cls, groups, candidates):
        """A Design over ready group handles (objects with ``scores()``, ``condition(i)``, ``integrated_variance()``,
        ``close()``)."""
        self = cls.__new__(cls)
        self._groups = list(groups)
        self.candidates = np.array(candidates, ndmin=2, dtype=np.float64)
        self.d, self.max_picks, self.picks = self.candidates.shape[1], MAX_PICKS, []
        return self

    # -- lifetime ------------------------------------------------------------------------------------------------
    def close(self):
        for g in self.__dict__.get("_groups", []):
            g.close()
        self._groups = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the criterion -------------------------------------------------------------------------------------------
    def scores_per_group(self):
        """(n_groups, M)"""
        return np.stack([g.scores() for g in self._groups])

    def scores(self):
        """(M,): the groups' scores added in group order"""
        per = self.scores_per_group()
        out = per[0].copy()
        for row in per[1:]:
            out += row
        return out

    def condition(self, i):
        """Condition every group on a model run at candidate ``i``."""
        i = int(i)
        if not 0 <= i < self.candidates.shape[0]:
            raise IndexError(f"candidate {i} outside [0, {self.candidates.shape[0]})")
        if len(self.picks) >= self.max_picks:
            raise ValueError(f"more picks than max_picks = {self.max_picks}")
        for g in self._groups:
            g.condition(i)
        self.picks.append(i)

    def integrated_variance(self):
        """sum over groups and PCs of w_p IV_p, groups added in order"""
        out = 0.0
        for g in self._groups:
            out += g.integrated_variance()
        return out

    def select(self, q):
        """Greedy batch of ``q`` points: ``indices (q,)``, ``points (q, d)``, ``gain (q,)`` (the score of each pick when
        it was picked), ``integrated_variance (q + 1,)`` (before the first pick and after each) and ``first_scores
        (M,)``.  Ties of the best score go to the lowest index.  When no candidate has a positive score -- every one is
        under the floor, the emulator is exact on all of them -- nothing is left to gain: the selection stops with a
        warning and the arrays hold the picks made so far.  A NaN score raises ValueError."""
        q = int(q)
        if q < 0 or len(self.picks) + q > self.max_picks:
            raise ValueError(f"{q} more picks exceed max_picks = {self.max_picks}")
        idx, gain, iv, first = [], [], [self.integrated_variance()], None
        for j in range(q):
            s = self.scores()
            if first is None:
                first = s.copy()
            if np.isnan(s).any():
                raise ValueError("a design score is NaN")
            i = int(np.argmax(s))          # the first of equal maxima
            if not s[i] > 0.0:
                warnings.warn(f"design: no candidate lowers the integrated variance after {j} picks; stopping")
                break
            self.condition(i)
            idx.append(i)
            gain.append(float(s[i]))
            iv.append(self.integrated_variance())
        if first is None:
            first = self.scores()
        idx = np.array(idx, dtype=np.int64)
        return {"indices": idx, "points": self.candidates[idx].copy(), "gain": np.array(gain, dtype=np.float64),
                "integrated_variance": np.array(iv), "first_scores": first}


def default_candidates(lo, hi, reference_rows, n_candidates, seed=0):
    """The default candidate set: ``n_candidates - n_candidates // 2`` points of the prior box (the A matrix of
    ``gpemu.sensitivity.base_samples``: a scrambled Sobol' sequence, which keeps the design able to leave the
    posterior's bulk) followed by ``n_candidates // 2`` rows of the reference set drawn without replacement by
    ``numpy.random.default_rng(seed)`` (all of them if there are fewer): where the posterior lives."""
    from .sensitivity import base_samples
    n_ref = min(int(n_candidates) // 2, 0 if reference_rows is None else len(reference_rows))
    n_box = int(n_candidates) - n_ref
    parts = []
    if n_box > 0:
        parts.append(base_samples(n_box, lo, hi, seed=seed)[0])
    if n_ref > 0:
        rows = np.asarray(reference_rows, dtype=np.float64)
        pick = np.sort(np.random.default_rng(seed).choice(len(rows), size=n_ref, replace=False))
        parts.append(rows[pick])
    return np.ascontiguousarray(np.concatenate(parts))
