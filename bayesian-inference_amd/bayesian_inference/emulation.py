"""Drop-in replacement of ``bayesian_inference.emulation`` with the arithmetic on an MI355X.

Same public names, arguments and return shapes as the reference module
(ref: src/bayesian_inference/emulation.py): ``fit_emulators``, ``fit_emulator_group``,
``read_emulators``, ``write_emulators``, ``compute_emulator_cov_unexplained``,
``compute_emulator_group_cov_unexplained``, ``nd_block_diag``, ``SortEmulationGroupObservables``,
``predict``, ``predict_emulation_group``, ``EmulationGroupConfig``, ``EmulationConfig``.

What runs where
  * standardise + PCA, GP fit (kernel matrix, Cholesky, LML + gradient), GP predict, the
    back-projection and the covariance assembly run in libgpemu (HIP, gfx950) via ``gpemu``;
  * configuration parsing, HDF5 / pickle I/O and the observable bookkeeping are host Python, as in
    the reference.  ``data_IO`` is imported lazily from the reference package (it is untouched).
The results dict has the reference's keys; the objects in it are ``gpemu.estimators`` classes
(same attribute names as the sklearn objects, picklable without scikit-learn).

Deliberate differences (results identical): ``compute_emulator_cov_unexplained`` returns the dict it
builds (the reference forgets the ``return``, ref: emulation.py:214-224, so callers got ``None`` and
recomputed the matrix on every predict call).
"""
from __future__ import annotations

import logging
import os
import pickle
from pathlib import Path
from typing import Any

import numpy as np
import yaml

from gpemu import estimators
from gpemu.model import DeviceModel

logger = logging.getLogger(__name__)


def _data_IO():
    """The reference's data_IO module (HDF5 readers; out of scope here and left untouched)."""
    from bayesian_inference import data_IO
    return data_IO


####################################################################################################
def _rank_world():
    """(rank, world); joins the launcher's process group on first use (``gpemu.dist``)."""
    from gpemu import dist as gdist
    return gdist.rank_world()


def fit_emulators(emulation_config: "EmulationConfig") -> None:
    """PCA + GP fit for every emulation group; writes one pickle per group (ref: emulation.py:38-50).

    One process per GPU (torch.distributed initialised): the groups are independent, group i is fitted and
    written by rank i % world on its own GPU; all ranks leave together so that the next stage finds every file."""
    rank, world = _rank_world()
    for i, (name, group_config) in enumerate(emulation_config.emulation_groups_config.items()):
        if i % world != rank:
            continue
        result = fit_emulator_group(group_config)
        if result:   # an existing emulator is not overwritten (ref: emulation.py:46-48)
            write_emulators(config=group_config, output_dict=result)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def build_kernel(config) -> estimators.ARDKernel:
    """Kernel prototype in the order of ``kernels.active`` (ref: emulation.py:129-162)."""
    par = config.analysis_config['parameterization'][config.parameterization]
    lo, hi = np.array(par['min'], dtype=np.float64), np.array(par['max'], dtype=np.float64)
    kw: dict[str, Any] = {}
    kind = None
    for kernel_type, kernel_args in config.active_kernels.items():
        if kernel_type in ("matern", "rbf"):
            length_scale = hi - lo
            bounds = np.outer(length_scale, tuple(kernel_args['length_scale_bounds_factor']))
            kind = estimators.MATERN_KIND if kernel_type == "matern" else estimators.RBF_KIND
            kw.update(length_scale=length_scale, length_scale_bounds=bounds)
            if kernel_type == "matern":
                kw["nu"] = kernel_args['nu']
        elif kernel_type == "constant":
            kw.update(constant_value=kernel_args["constant_value"],
                      constant_value_bounds=kernel_args["constant_value_bounds"])
        elif kernel_type == "noise":
            kw.update(noise_level=kernel_args["args"]["noise_level"],
                      noise_level_bounds=kernel_args["args"]["noise_level_bounds"])
    if kind is None:
        raise ValueError("Must provide exactly one of 'matern', 'rbf' kernel")
    return estimators.ARDKernel(kind, **kw)


def fit_emulator_group(config: "EmulationGroupConfig") -> dict[str, Any]:
    """Standardise, PCA, fit one GP per retained PC (ref: emulation.py:53-192).  Returns the results dict
    (schema in SURVEY 8b), or {} when a pickle exists and ``force_retrain`` is off."""
    target = Path(config.emulation_outputfile)
    if target.exists():
        if not config.force_retrain:
            logger.info(f'{target} exists; keeping it (force_retrain is off)')
            return {}
        target.unlink()
        logger.info(f'{target} deleted (force_retrain)')

    io = _data_IO()
    observables = io.predictions_matrix_from_h5(config.output_dir, filename=config.observables_filename,
                                                observable_filter=config.observable_filter)
    n_keep = config.n_pc
    n_calc = config.max_n_components_to_calculate           # None: all min(N, F) components
    logger.info('Scaling + PCA on the device' + ('' if n_calc is None else f' (first {n_calc} components)') + '...')
    scaler, pca, scores = estimators.scale_and_pca(observables, n_components=n_calc)
    kept_scores = scores[:, :n_keep]
    back_projected = kept_scores @ pca.components_[:n_keep]
    logger.info(f'  {n_keep} components explain {pca.explained_variance_ratio_[:n_keep].sum():.6f} of the variance')

    design = io.design_array_from_h5(config.output_dir, filename=config.observables_filename)
    logger.info(f'Fitting {n_keep} GPs on {design.shape[0]} design points x {design.shape[1]} parameters '
                f'({config.n_restarts} restarts each)...')
    # the GPs and their restarts are independent optimisations: they run concurrently on the device
    emulators = estimators.fit_gps(design, kept_scores, build_kernel(config), alpha=config.alpha,
                                   n_restarts_optimizer=config.n_restarts, copy_X_train=False)
    for index, gp in enumerate(emulators):
        logger.info(f'  PC {index}: {gp.kernel_}')

    results = {
        'PCA': {
            'Y': observables,
            'Y_pca': scores,
            'Y_pca_truncated': kept_scores,
            'Y_reconstructed_truncated': back_projected,
            'Y_reconstructed_truncated_unscaled': scaler.inverse_transform(back_projected),
            'pca': pca,
            'scaler': scaler,
        },
        'emulators': emulators,
    }
    if config.cross_validation:
        cv = cross_validate_emulator_group(config, results)
        logger.info(f'{cv["n_folds"]}-fold cross-validation at the fitted hyper-parameters:')
        for index, mz2 in enumerate(cv['mean_z2_pc']):
            logger.info(f'  PC {index}: mean(z^2) = {mz2:.4g}')
        logger.info(f'  observables: RMSE {np.sqrt(np.mean(cv["residual"] ** 2)):.4g}, '
                    f'mean(z^2) {np.nanmean(cv["z"] ** 2):.4g}, '
                    f'coverage {cv["coverage"]:.3f} at confidence {cv["confidence"]}')
        results['cross_validation'] = cv
    return results


####################################################################################################
# Cross-validation of the emulators at their fitted hyper-parameters.  The analysis YAML's
# `cross_validation` / `cross_validation_k` keys (ref: config/jet_substructure.yaml, emulator_parameters), which the
# reference declares but never reads.
def kfold_labels(N: int, k: int) -> np.ndarray:
    """Fold label of each of N design points as sklearn.model_selection.KFold(n_splits=k) without shuffling deals
    them: contiguous folds in design order, the first N % k folds one point larger.  k = N: leave-one-out."""
    N, k = int(N), int(k)
    if k < 2:
        raise ValueError(f"cross_validation_k must be at least 2, got {k}")
    if k > N:
        raise ValueError(f"cross_validation_k = {k} exceeds the number of design points ({N})")
    sizes = np.full(k, N // k, dtype=np.int64)
    sizes[:N % k] += 1
    return np.repeat(np.arange(k, dtype=np.int32), sizes)


def _closure_confidence(config) -> float:
    """The analysis' closure `confidence` (ref: config/jet_substructure.yaml, closure parameters); 0.9 if absent."""
    try:
        conf = config.analysis_config['parameters']['closure']['confidence']
    except (KeyError, TypeError):
        return 0.9
    if isinstance(conf, (list, tuple)):
        conf = conf[0]
    return float(conf)


def _cv_summary(out: dict, Y: np.ndarray, confidence: float) -> dict:
    """Residuals and their summary (host numpy) of merged or per-group cross-validation results."""
    from statistics import NormalDist
    residual = Y - out['central_value']
    with np.errstate(divide='ignore', invalid='ignore'):
        z = residual / np.sqrt(out['variance'])
    bound = NormalDist().inv_cdf(0.5 + 0.5 * confidence)
    out.update(residual=residual, z=z,
               rmse=np.sqrt(np.mean(residual ** 2, axis=0)),
               mean_z2=np.mean(z ** 2, axis=0),
               coverage=float(np.mean(np.abs(z) <= bound)),
               confidence=float(confidence))
    return out


def cross_validate_emulator_group(config: "EmulationGroupConfig", results: dict[str, Any],
                                  n_folds: int | None = None) -> dict[str, Any]:
    """k-fold cross-validation of one group's emulators on the device (``DeviceModel.cross_validate``).

    Each design point is predicted by its PCs' GPs refitted to the other folds with the hyper-parameters held at the
    fitted ``kernel_`` and the scaler and PCA held at the full-data fit (no re-optimisation per fold):
    ``GaussianProcessRegressor(kernel=gp.kernel_, alpha=alpha, optimizer=None).fit(X[R], y[R])
    .predict(X[I], return_std=True)``, back-projected as ``predict_emulation_group`` does for one sample.
    ``n_folds`` defaults to the group's ``cross_validation_k``; the folds are ``kfold_labels``.

    Returns ``fold`` (N,), ``n_folds``, ``mean_pc`` / ``var_pc`` (N, n_pc), ``central_value`` / ``variance`` (N, F),
    ``residual`` = Y - central_value, ``z`` = residual / sqrt(variance), per feature ``rmse`` and ``mean_z2``, per PC
    ``mean_z2_pc``, per point ``chi2_pc`` = sum_p (y_pc - mean_pc)^2 / var_pc, and ``coverage``, the fraction of |z|
    inside the two-sided normal interval of the closure ``confidence``."""
    k = config.cross_validation_k if n_folds is None else n_folds
    y_pc = np.asarray(results['PCA']['Y_pca_truncated'], dtype=np.float64)[:, :config.n_pc]
    fold = kfold_labels(y_pc.shape[0], k)
    dm = device_model_for(results, config.n_pc)
    mean_pc, var_pc, cv, variance = dm.cross_validate(y_pc, fold)
    with np.errstate(divide='ignore', invalid='ignore'):
        z2_pc = (y_pc - mean_pc) ** 2 / var_pc
    out = dict(fold=fold, n_folds=int(k), mean_pc=mean_pc, var_pc=var_pc, central_value=cv, variance=variance,
               mean_z2_pc=np.mean(z2_pc, axis=0), chi2_pc=np.sum(z2_pc, axis=1))
    return _cv_summary(out, np.asarray(results['PCA']['Y'], dtype=np.float64), _closure_confidence(config))


def cross_validate(emulation_config: "EmulationConfig", emulation_results: dict[str, dict[str, Any]] | None = None,
                   n_folds: int | None = None) -> dict[str, Any]:
    """Cross-validation of every emulation group (``cross_validate_emulator_group``), merged into the full observable
    order by the conversion ``predict`` uses.  The groups share the design, so they share the folds.

    Returns ``fold``, ``n_folds``, per group ``mean_pc`` / ``var_pc`` / ``chi2_pc`` ({group: array}), the merged
    ``central_value`` / ``variance`` / ``residual`` / ``z`` (N, F_total), per feature ``rmse`` / ``mean_z2``, the
    per-point ``chi2_pc`` summed over groups (``chi2_pc_total``) and ``coverage``."""
    emulation_config._need_groups("cross-validation")
    emulation_results = emulation_results or {}
    per_group = {}
    for name, group_config in emulation_config.emulation_groups_config.items():
        results = emulation_results.get(name)
        if results is None:
            results = read_emulators(group_config)
        res = cross_validate_emulator_group(group_config, results, n_folds)
        res['Y'] = np.asarray(results['PCA']['Y'], dtype=np.float64)
        per_group[name] = res
    sorter = emulation_config.sort_observables_in_matrix
    # a sorter of its own: convert() fixes the value types it merges on first use
    merged = SortEmulationGroupObservables(sorter.emulation_group_to_observable_matrix, sorter.shape).convert(
        {name: {'central_value': r['central_value'], 'variance': r['variance'], 'Y': r['Y']}
         for name, r in per_group.items()})
    first = next(iter(per_group.values()))
    confidence = _closure_confidence(next(iter(emulation_config.emulation_groups_config.values())))
    out = dict(fold=first['fold'], n_folds=first['n_folds'],
               mean_pc={n: r['mean_pc'] for n, r in per_group.items()},
               var_pc={n: r['var_pc'] for n, r in per_group.items()},
               chi2_pc={n: r['chi2_pc'] for n, r in per_group.items()},
               chi2_pc_total=np.sum([r['chi2_pc'] for r in per_group.values()], axis=0),
               central_value=merged['central_value'], variance=merged['variance'])
    return _cv_summary(out, merged['Y'], confidence)


####################################################################################################
def read_emulators(config: "EmulationGroupConfig") -> dict[str, Any]:
    return pickle.loads(Path(config.emulation_outputfile).read_bytes())


def write_emulators(config: "EmulationGroupConfig", output_dict: dict[str, Any]) -> None:
    target = Path(config.emulation_outputfile)
    target.parent.mkdir(parents=True, exist_ok=True)
    # written under a private name and moved into place: a reader (or another rank) never sees half a pickle
    scratch = target.with_name(f'{target.name}.{os.getpid()}.tmp')
    scratch.write_bytes(pickle.dumps(output_dict))
    os.replace(scratch, target)


####################################################################################################
def compute_emulator_cov_unexplained(emulation_config, emulation_results) -> dict[str, np.ndarray]:
    """Truncation covariance of every group (ref: emulation.py:214-224; returned here, see module doc)."""
    if not emulation_results:
        emulation_results = emulation_config.read_all_emulator_groups()
    return {name: compute_emulator_group_cov_unexplained(cfg, emulation_results.get(name))
            for name, cfg in emulation_config.emulation_groups_config.items()}


def compute_emulator_group_cov_unexplained(emulation_group_config, emulation_group_result) -> np.ndarray:
    """S_{>k} diag(explained_variance_{>k}) S_{>k}^T (ref: emulation.py:227-251): one F x F x (n_comp - k)
    product on the device's f64 matrix cores (``gpemu_truncation_cov``), computed once per group."""
    return estimators.truncation_covariance(emulation_group_result['PCA']['pca'], emulation_group_config.n_pc)


####################################################################################################
def nd_block_diag(arrays):
    """Stack (..., r_i, c_i) blocks on the diagonal of a (..., sum r, sum c) array (ref: emulation.py:254-270)."""
    lead = np.amax(np.array([a.shape[:-2] for a in arrays]), axis=0) if arrays[0].ndim > 2 else ()
    rows = sum(a.shape[-2] for a in arrays)
    cols = sum(a.shape[-1] for a in arrays)
    out = np.zeros(tuple(lead) + (rows, cols))
    r = c = 0
    for a in arrays:
        out[..., r:r + a.shape[-2], c:c + a.shape[-1]] = a
        r += a.shape[-2]
        c += a.shape[-1]
    return out


class SortEmulationGroupObservables:
    """Mapping between the per-group matrices and the globally sorted observable order
    (ref: emulation.py:274-406).  ``emulation_group_to_observable_matrix`` is
    {observable: (group, slice in the merged matrix, slice in the group matrix)} in sorted order."""

    def __init__(self, emulation_group_to_observable_matrix, shape):
        self.emulation_group_to_observable_matrix = emulation_group_to_observable_matrix
        self.shape = tuple(shape)
        self._available_value_types = None

    @classmethod
    def learn_mapping(cls, emulation_config: "EmulationConfig") -> "SortEmulationGroupObservables":
        data_IO = _data_IO()
        prediction_key = "Prediction"
        all_observables = data_IO.read_dict_from_h5(emulation_config.output_dir, 'observables.h5')
        position = 0
        observable_slices = {}
        for key in data_IO.sorted_observable_list_from_dict(all_observables[prediction_key]):
            n_bins = all_observables[prediction_key][key]['y'].shape[0]
            observable_slices[key] = slice(position, position + n_bins)
            position += n_bins
        mapping = {}
        for group_name, group_config in emulation_config.emulation_groups_config.items():
            keys = data_IO.sorted_observable_list_from_dict(all_observables[prediction_key],
                                                            observable_filter=group_config.observable_filter)
            group_bin = 0
            for key in keys:
                sl = observable_slices[key]
                width = sl.stop - sl.start
                mapping[key] = (group_name, sl, slice(group_bin, group_bin + width))
                group_bin += width
        mapping = {k: mapping[k] for k in observable_slices}
        last = list(observable_slices)[-1]
        n_design = all_observables[prediction_key][last]['y'].shape[1]
        return cls(mapping, (n_design, observable_slices[last].stop))

    def group_layout(self, group_name):
        """(columns of this group in the merged matrix, observable block starts inside the group)."""
        entries = sorted(((sg.start, so, sg) for (g, so, sg) in self.emulation_group_to_observable_matrix.values()
                          if g == group_name), key=lambda e: e[0])
        cols = np.concatenate([np.arange(so.start, so.stop) for _, so, _ in entries])
        starts = [sg.start for _, _, sg in entries] + [entries[-1][2].stop]
        return cols, np.array(starts, dtype=np.int64)

    def convert(self, group_matrices):
        if self._available_value_types is None:
            self._available_value_types = set(vt for group in group_matrices.values() for vt in group)
        output = {}
        if "cov" in self._available_value_types:
            blocks = {}
            for _, (group_name, slice_out, slice_group) in self.emulation_group_to_observable_matrix.items():
                blocks[slice_out.start] = group_matrices[group_name]["cov"][:, slice_group, slice_group]
            output["cov"] = nd_block_diag([blocks[s] for s in sorted(blocks)])
        for value_type in self._available_value_types:
            if value_type == "cov":
                continue
            out = None
            for _, (group_name, slice_out, slice_group) in self.emulation_group_to_observable_matrix.items():
                m = group_matrices[group_name][value_type]
                if out is None:
                    out = np.zeros((m.shape[0], *self.shape[1:]))
                out[:, slice_out] = m[:, slice_group]
            output[value_type] = out
        return output


####################################################################################################
# Device models are built once per (results dict, n_pc, truncation covariance) and reused (the reference rebuilds
# nothing either: its sklearn objects live in the dict).  The cache holds at most GPEMU_MODEL_CACHE entries
# (default 4), least recently used first out; an evicted model is released as soon as no sampler uses it.
_DEVICE_MODELS: "dict[tuple[int, int], tuple[Any, np.ndarray | None, DeviceModel]]" = {}


def _model_cache_limit() -> int:
    return max(1, int(os.environ.get("GPEMU_MODEL_CACHE", "4")))


def release_device_models() -> None:
    """Forget every cached device model (their HBM is freed once nothing else refers to them)."""
    _DEVICE_MODELS.clear()


def device_model_for(results: dict[str, Any], n_pc: int, cov_unexplained: np.ndarray | None = None) -> DeviceModel:
    """The DeviceModel (GP factors, PCA, scaler resident in HBM) of one emulation group's results dict."""
    key = (id(results), int(n_pc))
    hit = _DEVICE_MODELS.get(key)
    if hit is not None and hit[0] is results:
        same_cov = (hit[1] is cov_unexplained) or (
            hit[1] is not None and cov_unexplained is not None and np.array_equal(hit[1], cov_unexplained))
        if same_cov:
            _DEVICE_MODELS[key] = _DEVICE_MODELS.pop(key)      # most recently used last
            return hit[2]
    emulators = results['emulators'][:n_pc]
    pca, scaler = results['PCA']['pca'], results['PCA']['scaler']
    k0 = emulators[0].kernel_
    given = cov_unexplained
    if cov_unexplained is None:
        cov_unexplained = estimators.truncation_covariance(pca, n_pc)
    dm = DeviceModel(
        X_train=emulators[0].X_train_,
        ls=np.stack([e.kernel_.length_scale for e in emulators]),
        alpha=np.stack([e.alpha_ for e in emulators]),
        L=np.stack([e.L_ for e in emulators]),
        components=pca.components_[:n_pc], scaler_mean=scaler.mean_, scaler_scale=scaler.scale_,
        kernel_kind=k0.kind, nu=k0.nu,
        const=np.array([e.kernel_.constant_value for e in emulators]) if k0.has_const else None,
        noise=np.array([e.kernel_.noise_level for e in emulators]) if k0.has_noise else None,
        cov_unexplained=cov_unexplained)
    _DEVICE_MODELS.pop(key, None)
    _DEVICE_MODELS[key] = (results, given, dm)
    while len(_DEVICE_MODELS) > _model_cache_limit():
        _DEVICE_MODELS.pop(next(iter(_DEVICE_MODELS)))
    return dm


def predict(parameters, emulation_config: "EmulationConfig", merge_predictions_over_groups: bool = True,
            emulation_group_results: dict[str, dict[str, Any]] | None = None,
            emulator_cov_unexplained: dict | None = None, return_jacobian: bool = False) -> dict[str, np.ndarray]:
    """{'central_value': (B,F), 'cov': (B,F,F)} over all groups (ref: emulation.py:410-462).

    ``return_jacobian=True`` adds ``'jacobian'`` (B, F, d), ``J[b, f, i] = d central_value[b, f] / d x_i =
    scale_f sum_p components[p, f] d m_p / d x_i`` from the analytic GP Jacobian on the device,
    merged over the groups like ``central_value``.  ``central_value`` and ``cov`` come from the same calls either
    way: the flag does not change their bits.  RBF and Matern nu = 1.5 / 2.5 / inf kernels only."""
    emulation_group_results = emulation_group_results or {}
    emulator_cov_unexplained = emulator_cov_unexplained or {}
    predict_output = {}
    jacobians = {}
    for group_name, group_config in emulation_config.emulation_groups_config.items():
        group_result = emulation_group_results.get(group_name)
        if group_result is None:
            group_result = read_emulators(group_config)
        cov_un = emulator_cov_unexplained[group_name] if emulator_cov_unexplained else None
        predict_output[group_name] = predict_emulation_group(parameters, group_result, group_config,
                                                             emulator_group_cov_unexplained=cov_un)
        if return_jacobian:
            jacobians[group_name] = group_jacobian(parameters, group_result, group_config, cov_un)
    if not merge_predictions_over_groups:
        for group_name, jac in jacobians.items():
            predict_output[group_name]['jacobian'] = jac
        return predict_output
    sorter = emulation_config.sort_observables_in_matrix
    output = sorter.convert(group_matrices=predict_output)
    if return_jacobian:
        output['jacobian'] = merge_jacobians(sorter, jacobians)
    return output


def group_jacobian(parameters, results, emulation_group_config, emulator_group_cov_unexplained=None) -> np.ndarray:
    """(B, F, d) Jacobian of one group's central values: the device's d m_p / d x back-projected through the PCA and
    the scaler, as ``central_value = (m @ components) * scale + mean`` is."""
    parameters = np.array(parameters, ndmin=2, dtype=np.float64)
    n_pc = emulation_group_config.n_pc
    dm = device_model_for(results, n_pc, emulator_group_cov_unexplained)
    dmean = dm.gp_predict_grad(parameters)[2]
    return backproject_jacobian(dmean, results['PCA']['pca'].components_[:n_pc], results['PCA']['scaler'].scale_)


def backproject_jacobian(dmean, components, scale) -> np.ndarray:
    """dmean (B, k, d), components (k, F), scale (F,) -> (B, F, d)"""
    return np.einsum('bpi,pf->bfi', np.asarray(dmean), np.asarray(components)) * np.asarray(scale)[None, :, None]


def merge_jacobians(sorter, jacobians) -> np.ndarray:
    """The groups' (B, F_g, d) Jacobians in the merged observable order, (B, F, d): ``convert``'s rule for
    ``central_value`` with one more axis."""
    out = None
    for _, (group_name, slice_out, slice_group) in sorter.emulation_group_to_observable_matrix.items():
        jac = jacobians[group_name]
        if out is None:
            out = np.zeros((jac.shape[0], *sorter.shape[1:], jac.shape[2]))
        out[:, slice_out, :] = jac[:, slice_group, :]
    return out


def sensitivity(parameters, emulation_config: "EmulationConfig",
                emulation_group_results: dict[str, dict[str, Any]] | None = None) -> np.ndarray:
    """Normalised sensitivities (B, F, d): ``d O_f / d x_i * x_i / O_f`` at each row of ``parameters``, from the
    analytic Jacobian -- the quantity the reference's sensitivity plot approximates with a 10 % forward difference
    (ref: plot_qhat.py:172-183, 204-258)."""
    parameters = np.array(parameters, ndmin=2, dtype=np.float64)
    out = predict(parameters, emulation_config, emulation_group_results=emulation_group_results, return_jacobian=True)
    return normalised_sensitivity(out['jacobian'], parameters, out['central_value'])


def normalised_sensitivity(jacobian, parameters, central_value) -> np.ndarray:
    """J[b, f, i] x[b, i] / O[b, f]"""
    return np.asarray(jacobian) * np.asarray(parameters)[:, None, :] / np.asarray(central_value)[:, :, None]


POSTERIOR_PREDICTIVE_PROBABILITIES = (0.05, 0.5, 0.95)
_PP_VECTORS = ('mean', 'variance_parameters', 'variance_emulator', 'variance')


def scatter_feature_rows(sorter, rows) -> np.ndarray:
    """The groups' per-feature rows ``{group: (R, F_g)}`` in the merged observable order of ``predict``, (R, F):
    ``convert``'s rule for ``central_value``.  A sorter that has no mapping of its own (a stand-in that only implements
    ``convert``) converts every matrix as a ``central_value``."""
    mapping = getattr(sorter, 'emulation_group_to_observable_matrix', None)
    if mapping is None:
        return np.asarray(sorter.convert({name: {'central_value': m} for name, m in rows.items()})['central_value'])
    merged = np.zeros((next(iter(rows.values())).shape[0], sorter.shape[1]))
    for _, (group_name, slice_out, slice_group) in mapping.items():
        merged[:, slice_out] = rows[group_name][:, slice_group]
    return merged


def merge_posterior_predictive(sorter, group_results) -> dict[str, np.ndarray]:
    """The groups' posterior-predictive summaries in the merged observable order of ``predict``: every entry is per
    feature, so the merge is a scatter -- ``convert``'s rule for ``central_value``, applied to the (F,) vectors and the
    (nq, F) quantiles stacked as the rows of one matrix.  A sorter that has no mapping of its own (a stand-in that only
    implements ``convert``) converts that matrix as a ``central_value``."""
    first = next(iter(group_results.values()))
    rows = {name: np.vstack([g[key] for key in _PP_VECTORS] + [g['quantiles']]) for name, g in group_results.items()}
    merged = scatter_feature_rows(sorter, rows)
    out = {key: merged[i].copy() for i, key in enumerate(_PP_VECTORS)}
    out['quantiles'] = merged[len(_PP_VECTORS):].copy()
    out['probabilities'] = np.array(first['probabilities'], dtype=np.float64)
    return out


def posterior_predictive(parameters, emulation_config: "EmulationConfig",
                         emulation_group_results: dict[str, dict[str, Any]] | None = None,
                         emulator_cov_unexplained: dict | None = None,
                         probabilities=POSTERIOR_PREDICTIVE_PROBABILITIES,
                         merge_predictions_over_groups: bool = True, weights=None) -> dict[str, Any]:
    """What the calibrated model predicts for every observable bin, from ALL rows of ``parameters`` (S, d) --
    typically the flattened chain -- instead of the few hundred draws the reference's plots push through ``predict``
    (ref: plot_mcmc.py:343-371): ``mean``, ``variance_parameters`` (spread of the central value over the rows),
    ``variance_emulator`` (mean emulator variance of one sample, the diagonal of ``predict``'s ``cov`` with one row per
    call), ``variance`` (their sum), ``quantiles`` (nq, F) and ``probabilities``, in the observable order of
    ``predict``.  Reduced on the device per group (``DeviceModel.posterior_predictive``).

    ``weights``: fixed-point importance weights ``q`` (R_w, S) of a reweighted chain (``gpemu.reweight.fixed_weights``)
    -- the bands under another prior or other data without a rerun (``DeviceModel.posterior_predictive_weighted``,
    DESIGN.md §4.43).  The result is then a list with one such dict per weight row, ``total_weight`` added; the
    quantiles are the inverted weighted ECDF, elements of the sample."""
    parameters = np.array(parameters, ndmin=2, dtype=np.float64)
    emulation_group_results = emulation_group_results or {}
    emulator_cov_unexplained = emulator_cov_unexplained or {}
    per_group = {}
    for group_name, group_config in emulation_config.emulation_groups_config.items():
        group_result = emulation_group_results.get(group_name)
        if group_result is None:
            group_result = read_emulators(group_config)
        cov_un = emulator_cov_unexplained[group_name] if emulator_cov_unexplained else None
        dm = device_model_for(group_result, group_config.n_pc, cov_un)
        if weights is None:
            per_group[group_name] = dm.posterior_predictive(parameters, probabilities=probabilities)
        else:
            per_group[group_name] = dm.posterior_predictive_weighted(parameters, weights, probabilities=probabilities)
    if not merge_predictions_over_groups:
        return per_group
    if weights is None:
        return merge_posterior_predictive(emulation_config.sort_observables_in_matrix, per_group)
    merged = []
    for w in range(len(next(iter(per_group.values())))):
        rows = {name: g[w] for name, g in per_group.items()}
        out = merge_posterior_predictive(emulation_config.sort_observables_in_matrix, rows)
        out['total_weight'] = next(iter(rows.values()))['total_weight']
        merged.append(out)
    return merged


_GS_MATRICES = ('first_order', 'total', 'first_order_se', 'total_se')
_GS_VECTORS = ('variance', 'mean')


def merge_global_sensitivity(sorter, group_results) -> dict[str, Any]:
    """The groups' Sobol' results in the merged observable order of ``predict``: the (d, F_g) index matrices and the
    (F_g,) vectors stacked as the rows of one matrix and scattered as ``merge_posterior_predictive`` scatters."""
    first = next(iter(group_results.values()))
    d = first['first_order'].shape[0]
    rows = {name: np.vstack([g[key] for key in _GS_MATRICES] + [g[key][None, :] for key in _GS_VECTORS])
            for name, g in group_results.items()}
    merged = scatter_feature_rows(sorter, rows)
    out = {key: merged[i * d:(i + 1) * d].copy() for i, key in enumerate(_GS_MATRICES)}
    for i, key in enumerate(_GS_VECTORS):
        out[key] = merged[len(_GS_MATRICES) * d + i].copy()
    out['n'], out['n_batches'] = first['n'], first['n_batches']
    return out


_GS_PAIR_MATRICES = ('closed_pair', 'interaction', 'total_pair', 'closed_pair_se', 'interaction_se', 'total_pair_se')


def merge_global_sensitivity_pairs(sorter, group_results) -> dict[str, Any]:
    """The groups' second-order results ((P, F_g) per key, the same ``pairs`` in every group) in the merged observable
    order of ``predict``, scattered as ``merge_global_sensitivity`` scatters."""
    first = next(iter(group_results.values()))
    P = first['closed_pair'].shape[0]
    rows = {name: np.vstack([g[key] for key in _GS_PAIR_MATRICES]) for name, g in group_results.items()}
    merged = scatter_feature_rows(sorter, rows)
    out = {key: merged[i * P:(i + 1) * P].copy() for i, key in enumerate(_GS_PAIR_MATRICES)}
    out['pairs'] = np.array(first['pairs'], dtype=np.int64)
    return out


def global_sensitivity(emulation_config: "EmulationConfig", n: int = 4096, seed: int = 0, method: str = 'sobol',
                       box=None, n_batches: int = 16,
                       emulation_group_results: dict[str, dict[str, Any]] | None = None,
                       second_order: bool = False, pairs=None) -> dict[str, Any]:
    """Global, variance-based sensitivities of every observable bin over a parameter box: ``first_order`` (d, F), the
    share of the emulated observable's variance that parameter i explains alone, ``total`` (d, F), its share with all
    interactions, their batch-means standard errors ``first_order_se`` / ``total_se``, ``variance`` and ``mean`` (F,)
    of the emulated central value over the box, ``n``, ``n_batches`` and ``parameter_names``, in the observable order
    of ``predict`` -- the global counterpart of ``sensitivity`` (the reference's only sensitivity is a 10 % forward
    difference at one point, ref: plot_qhat.py:172-258).  ``box`` = (lo, hi) defaults to the prior box of the
    parameterisation, the one ``mcmc.run_mcmc`` samples in; a sub-box restricts the analysis.  One pair of base
    matrices (``gpemu.sensitivity.base_samples``) is shared by all groups; reduced on the device per group
    (``DeviceModel.sobol_indices``).

    ``second_order=True`` adds, for ``pairs`` (P, 2) of parameters i < j (None: all of them), ``pairs`` and the (P, F)
    arrays ``closed_pair`` (the share both explain together), ``interaction`` (= closed_pair - S_i - S_j, the share
    they explain only jointly: with which parameter a large ``total - first_order`` interacts), ``total_pair`` and
    their ``_se`` (``gpemu.sensitivity.pair_indices_from_moments``), from the same base pair;
    ``gpemu.sensitivity.interacting_pairs`` picks the pairs worth asking for from a first-order result."""
    from gpemu import sensitivity as gs
    if pairs is not None and not second_order:
        raise ValueError("pairs needs second_order=True")
    par = emulation_config.analysis_config['parameterization'][emulation_config.parameterization]
    lo, hi = (par['min'], par['max']) if box is None else box
    A, B = gs.base_samples(n, lo, hi, seed=seed, method=method)
    emulation_group_results = emulation_group_results or {}
    per_group = {}
    for group_name, group_config in emulation_config.emulation_groups_config.items():
        group_result = emulation_group_results.get(group_name)
        if group_result is None:
            group_result = read_emulators(group_config)
        dm = device_model_for(group_result, group_config.n_pc)
        if second_order:
            per_group[group_name] = dm.sobol_indices(A, B, n_batches=n_batches, second_order=True, pairs=pairs)
        else:
            per_group[group_name] = dm.sobol_indices(A, B, n_batches=n_batches)
    out = merge_global_sensitivity(emulation_config.sort_observables_in_matrix, per_group)
    if second_order:
        out.update(merge_global_sensitivity_pairs(emulation_config.sort_observables_in_matrix, per_group))
    out['parameter_names'] = [str(name) for name in par['names']]
    return out


def gather_feature_rows(sorter, merged, group_names) -> dict[str, np.ndarray]:
    """The inverse of ``scatter_feature_rows`` for one vector: ``merged`` (F,) in the observable order of ``predict``
    -> ``{group: (F_g,)}`` in each group's own order.  A sorter that has no mapping of its own (a stand-in that only
    implements ``convert``) serves one group, which takes the whole vector."""
    merged = np.asarray(merged, dtype=np.float64).reshape(-1)
    mapping = getattr(sorter, 'emulation_group_to_observable_matrix', None)
    group_names = list(group_names)
    if mapping is None:
        if len(group_names) != 1:
            raise ValueError("a sorter without a mapping serves one group")
        return {group_names[0]: merged.copy()}
    if merged.size != sorter.shape[1]:
        raise ValueError(f"expected {sorter.shape[1]} merged feature weights, got {merged.size}")
    width = {name: 0 for name in group_names}
    for _, (group_name, _, slice_group) in mapping.items():
        width[group_name] = max(width[group_name], slice_group.stop)
    out = {name: np.zeros(width[name]) for name in group_names}
    for _, (group_name, slice_out, slice_group) in mapping.items():
        out[group_name][slice_group] = merged[slice_out]
    return out


def design_sets(lo, hi, reference=None, candidates=None, n_reference=4096, n_candidates=2048, seed=0):
    """``(reference (S, d), candidates (M, d))`` of a design proposal.  ``reference=None``: ``n_reference`` points
    filling the prior box (the B matrix of ``gpemu.sensitivity.base_samples(n_reference, lo, hi, seed)``) -- plain
    integrated-variance design.  ``candidates=None``: ``gpemu.design.default_candidates`` -- box points (the A matrix of
    a sequence of its own, so no candidate coincides with a reference point by construction) and, when a reference set
    was given, a seeded subsample of its rows."""
    from gpemu import design as _design, sensitivity as gs
    given = reference is not None
    if not given:
        reference = gs.base_samples(n_reference, lo, hi, seed=seed)[1]
    reference = np.ascontiguousarray(np.array(reference, ndmin=2, dtype=np.float64))
    if candidates is None:
        candidates = _design.default_candidates(lo, hi, reference if given else None, n_candidates, seed=seed)
    return reference, np.ascontiguousarray(np.array(candidates, ndmin=2, dtype=np.float64))


def propose_design_points(emulation_config: "EmulationConfig", n_points: int, reference=None, candidates=None,
                          n_reference: int = 4096, n_candidates: int = 2048, seed: int = 0, feature_weights=None,
                          emulation_group_results: dict[str, dict[str, Any]] | None = None, **design_kwargs) -> dict[str, Any]:
    """Where should the model be run next?  ``n_points`` design points chosen greedily from ``candidates`` so that each
    lowers the emulators' integrated predictive variance over ``reference`` the most, at the fitted hyper-parameters
    (``gpemu.design.Design.select``) -- what the reference leaves to the user once cross-validation says
    the emulator limits the analysis.  ``reference``: (S, d) rows the variance is integrated over (posterior samples
    put the points where the posterior lives); None: ``n_reference`` points filling the prior box.  ``candidates``:
    (M, d); None: ``design_sets``' default.  ``feature_weights`` (F,) in the observable order of ``predict`` (default
    1; ``1 / y_err^2`` counts variance in units of the data's) is split over the groups the way ``predict`` merges
    them.  Returns ``points`` (q, d), ``indices``, ``gain``, ``integrated_variance`` (q + 1,), ``first_scores`` (M,),
    ``candidates`` and ``parameter_names``."""
    from gpemu import design as _design
    par = emulation_config.analysis_config['parameterization'][emulation_config.parameterization]
    reference, candidates = design_sets(par['min'], par['max'], reference, candidates, n_reference, n_candidates, seed)
    emulation_group_results = emulation_group_results or {}
    names = list(emulation_config.emulation_groups_config)
    models = []
    for group_name in names:
        group_config = emulation_config.emulation_groups_config[group_name]
        group_result = emulation_group_results.get(group_name)
        if group_result is None:
            group_result = read_emulators(group_config)
        models.append(device_model_for(group_result, group_config.n_pc))
    fws = None
    if feature_weights is not None:
        split = gather_feature_rows(emulation_config.sort_observables_in_matrix, feature_weights, names)
        fws = [split[name] for name in names]
    design_kwargs.setdefault('max_picks', max(int(n_points), 1))
    with _design.Design(models, reference, candidates, feature_weights=fws, **design_kwargs) as ds:
        out = ds.select(n_points)
    out['candidates'] = candidates
    out['parameter_names'] = [str(name) for name in par['names']]
    return out


def predict_emulation_group(parameters, results, emulation_group_config, emulator_group_cov_unexplained=None):
    """Central values (B,F) and covariances (B,F,F) of one group (ref: emulation.py:466-548).
    The truncation covariance is divided by the number of rows passed, like the reference
    (ref: emulation.py:531-532)."""
    parameters = np.array(parameters, ndmin=2, dtype=np.float64)
    dm = device_model_for(results, emulation_group_config.n_pc, emulator_group_cov_unexplained)
    cv, cov = dm.predict_full(parameters, n_div=parameters.shape[0])
    return {'central_value': cv, 'cov': cov}


####################################################################################################
class _Base:
    """Attribute bag (the reference derives its config classes from common_base.CommonBase)."""

    def __init__(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self, key, value)

    def set_attribute(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self, key, value)

    def __str__(self):
        body = '\n .  '.join(f'{k} = {v}' for k, v in self.__dict__.items())
        return f"[i] {self.__class__.__name__} with \n .  {body}"


_TOP_LEVEL_KEYS = ('observable_table_dir', 'observable_config_dir', 'observables_filename')


def _read_yaml(path):
    with open(path, 'r') as handle:
        return yaml.safe_load(handle)


def _check_kernels(active):
    """The reference's validity rules for the ``kernels`` block (ref: emulation.py:583-603)."""
    base = [name for name in ('matern', 'rbf') if name in active]
    assert len(base) == 1, "Must provide exactly one of 'matern', 'rbf' kernel"
    noise = active.get('noise')
    if noise is None:
        return
    assert 'type' in noise and 'args' in noise, "Noise configuration must have keys 'type' and 'args'"
    if noise['type'] != 'white':
        raise ValueError("Unsupported noise kernel")
    assert set(noise['args']) == {'noise_level', 'noise_level_bounds'}, \
        "Must provide arguments 'noise_level' and 'noise_level_bounds' for white noise kernel"


class EmulationGroupConfig(_Base):
    """Settings of one emulation group from the analysis YAML (ref: emulation.py:551-622); the attribute
    names are the reference's.  ``emulation_group_name=None`` reads an un-grouped ``emulators`` block."""

    def __init__(self, analysis_name='', parameterization='', analysis_config='', config_file='',
                 emulation_group_name: str | None = None):
        self.analysis_name, self.parameterization = analysis_name, parameterization
        self.analysis_config, self.config_file = analysis_config, config_file
        top = _read_yaml(config_file)
        for key in _TOP_LEVEL_KEYS:
            setattr(self, key, top[key])

        block = analysis_config['parameters']['emulators']
        if emulation_group_name is not None:
            block = block[emulation_group_name]
        self.force_retrain, self.n_pc = block['force_retrain'], block['n_pc']
        self.max_n_components_to_calculate = block.get('max_n_components_to_calculate')
        self.n_restarts, self.alpha = block['GPR']['n_restarts'], block['GPR']['alpha']
        # k-fold cross-validation at the fitted hyper-parameters after the fit; absent = off
        self.cross_validation = bool(block.get('cross_validation', False))
        self.cross_validation_k = block.get('cross_validation_k', 5)
        if self.cross_validation and (isinstance(self.cross_validation_k, bool) or
                                      not isinstance(self.cross_validation_k, (int, np.integer)) or
                                      self.cross_validation_k < 2):
            raise ValueError(f"cross_validation_k must be an integer >= 2, got {self.cross_validation_k!r}")

        kernels = block['kernels']
        self.active_kernels = {name: kernels[name] for name in kernels['active']}     # order of `active` is kept
        _check_kernels(self.active_kernels)

        wanted, unwanted = block.get('observable_list', []), block.get('observable_exclude_list', [])
        self.observable_filter = None
        if wanted or unwanted:
            self.observable_filter = _data_IO().ObservableFilter(include_list=wanted, exclude_list=unwanted)

        self.output_dir = os.path.join(top['output_dir'], f'{analysis_name}_{parameterization}')
        pickle_name = 'emulation.pkl' if emulation_group_name is None else f'emulation_group_{emulation_group_name}.pkl'
        self.emulation_outputfile = os.path.join(self.output_dir, pickle_name)


class EmulationConfig(_Base):
    """The emulation groups of one analysis (ref: emulation.py:624-709); attribute and method names kept."""

    def __init__(self, analysis_name: str, parameterization: str, config_file, analysis_config=None,
                 emulation_groups_config=None):
        self.analysis_name, self.parameterization = analysis_name, parameterization
        self.config_file = Path(config_file)
        self.analysis_config = {} if analysis_config is None else analysis_config
        self.emulation_groups_config = {} if emulation_groups_config is None else emulation_groups_config
        self.config = _read_yaml(self.config_file)
        for key in _TOP_LEVEL_KEYS:
            setattr(self, key, self.config[key])
        self.output_dir = os.path.join(self.config['output_dir'], f'{analysis_name}_{parameterization}')
        self._observable_filter = None
        self._sort_observables_in_matrix = None

    @classmethod
    def from_config_file(cls, analysis_name: str, parameterization: str, config_file, analysis_config):
        self = cls(analysis_name=analysis_name, parameterization=parameterization, config_file=config_file,
                   analysis_config=analysis_config)
        for group in analysis_config['parameters']['emulators']:
            self.emulation_groups_config[group] = EmulationGroupConfig(
                analysis_name=analysis_name, parameterization=parameterization, analysis_config=analysis_config,
                config_file=self.config_file, emulation_group_name=group)
        return self

    def _need_groups(self, what):
        if not self.emulation_groups_config:
            raise ValueError(f"Need to specify emulation groups to provide {what}")

    def read_all_emulator_groups(self):
        return {name: read_emulators(cfg) for name, cfg in self.emulation_groups_config.items()}

    @property
    def observable_filter(self):
        """Union of the groups' filters plus the global exclude list (built once)."""
        if self._observable_filter is None:
            self._need_groups("an observable filter")
            keep: list[str] = []
            drop: list[str] = self.config.get('global_observable_exclude_list', [])
            for group in self.emulation_groups_config.values():
                keep += group.observable_filter.include_list
                drop += group.observable_filter.exclude_list
            self._observable_filter = _data_IO().ObservableFilter(include_list=keep, exclude_list=drop)
        return self._observable_filter

    @property
    def sort_observables_in_matrix(self) -> SortEmulationGroupObservables:
        if self._sort_observables_in_matrix is None:
            self._need_groups("an sorting for observable group observables")
            self._sort_observables_in_matrix = SortEmulationGroupObservables.learn_mapping(self)
        return self._sort_observables_in_matrix
