"""Drop-in replacement of ``bayesian_inference.mcmc`` (ref: src/bayesian_inference/mcmc.py).

Public surface kept: ``run_mcmc(config, closure_index=-1)``, ``credible_interval``, ``map_parameters``,
``LoggingEnsembleSampler`` and ``MCMCConfig`` (same attribute names), and the on-disk results -- ``mcmc.h5``
with ``chain``, ``acceptance_fraction``, ``log_prob``, ``autocorrelation_time`` (+ the closure extras) and the
pickled sampler.  What changes is where the work happens: the ensemble, the stretch move and the
log-posterior live on the GPU(s) (``gpemu.sampler.EnsembleSampler``) instead of an emcee sampler feeding a
multiprocessing pool (ref: mcmc.py:77-85).  One process per GPU under ``torch.distributed``: the production
chain shards its walkers over the ranks, closure chains run whole, one per rank.
"""
from __future__ import annotations

import logging
import os
import pickle
import re
from pathlib import Path

import numpy as np
import yaml

from bayesian_inference import emulation, log_posterior
from gpemu import dist as gdist
from gpemu.sampler import EnsembleSampler, walkers_independent

logger = logging.getLogger(__name__)

_MCMC_KEYS = ("n_walkers", "n_burn_steps", "n_sampling_steps", "n_logging_steps")


def _data_IO():
    from bayesian_inference import data_IO
    return data_IO


def _rank_world():
    """(rank, world); joins the launcher's process group on first use (the reference's steering script
    initialises none)."""
    return gdist.rank_world()


def _rank():
    return _rank_world()[0]


def closure_owner(closure_index, world):
    """Closure tests (ref: steer_analysis.py:168-183) are independent chains, one per validation design
    point: with one process per GPU every rank walks the caller's loop, rank ``closure_index % world``
    runs that chain whole on its GPU and writes its own ``closure/results/<index>/`` files, the others skip
    it -- N chains in flight on N GPUs, no communication.  GPEMU_CLOSURE_REPLICAS=0 restores walker
    sharding for closure runs too."""
    if closure_index < 0 or world <= 1 or os.environ.get("GPEMU_CLOSURE_REPLICAS", "1") == "0":
        return None
    return closure_index % world


def _same_on_all_ranks(arr):
    """Rank 0's copy of ``arr`` on every rank (identity without torch.distributed)."""
    return gdist.rank0_array(arr)


def _best_distinct(sampler, count):
    """Positions of the ``count`` highest *distinct* log-probabilities seen so far (the reference restarts the
    second burn-in stage from them, ref: mcmc.py:99)."""
    _, first_seen = np.unique(sampler.flatlnprobability, return_index=True)   # ascending in log-probability
    return sampler.flatchain[first_seen[-count:]]


####################################################################################################
# Closure tests as ONE batched run.  The reference's loop (ref: steer_analysis.py:168-183) calls
# run_mcmc(config, closure_index=i) once per validation design point; the chains are independent and share the
# emulators.  The first call a rank receives runs ALL of that rank's closure chains stacked in one multi-chain
# device sampler and writes every chain's files; the later calls find their chain done and return.
#   * only the call for the FIRST index this rank owns starts a batch (the reference's loop starts at 0); it always
#     reruns, so a second closure pass in the same process -- e.g. after re-fitting the emulators -- produces fresh
#     files like the reference's; a call for any other index that no batch has produced runs that chain alone;
#   * a finished index is handed out once: asking for the same index again reruns it;
#   * the batch is keyed on the emulator files' modification times as well, so chains of older emulators never count.
_closure_done: "dict[tuple, set]" = {}


def _closure_key(config):
    stamps = []
    try:
        for group in config.analysis_config['parameters']['emulators']:
            path = os.path.join(config.output_dir, f'emulation_group_{group}.pkl')
            stamps.append((path, os.path.getmtime(path) if os.path.exists(path) else None))
    except (KeyError, TypeError):
        pass
    return (config.output_dir, config.analysis_name, config.parameterization, tuple(stamps))


def _closure_sub_batches(config, indices, n_par):
    """Split ``indices`` so that one stacked run's chain storage (C x steps x W x (d + 1) doubles on the device, and
    again on the host) stays within GPEMU_CLOSURE_CHAIN_GIB (default 16)."""
    budget = float(os.environ.get("GPEMU_CLOSURE_CHAIN_GIB", "16")) * 2 ** 30
    steps = max(config.n_sampling_steps, config.n_burn_steps)
    per_chain = 8.0 * steps * config.n_walkers * (n_par + 1)
    n = max(1, int(budget // max(per_chain, 1.0)))
    return [indices[i:i + n] for i in range(0, len(indices), n)]


def _closure_batch_enabled():
    return os.environ.get("GPEMU_CLOSURE_BATCH", "1") != "0"


def _closure_indices(config, first, rank, world):
    """Closure indices this rank still has to run, from ``first`` on (validation_indices of the analysis)."""
    lo, hi = config.analysis_config['validation_indices']
    return [j for j in range(first, hi - lo) if closure_owner(j, world) in (None, rank)]


def _with_data_covariance(config, data):
    """``data`` with the arrays of ``parameters.mcmc.data_covariance`` (an ``.npz`` holding ``cov`` (F, F) and / or
    ``sys_sources`` (S, F) in the merged, filtered observable order) added; without the key, ``data``
    itself."""
    path = getattr(config, 'data_covariance', None)
    if not path:
        return data
    with np.load(path) as npz:
        extra = {key: np.array(npz[key], dtype=np.float64) for key in ('cov', 'sys_sources') if key in npz.files}
    if not extra:
        raise ValueError(f"{path}: parameters.mcmc.data_covariance holds neither 'cov' nor 'sys_sources'")
    data = dict(data)
    data.update(extra)
    return data


def _run_closure_batch(config, indices):
    """The chains of ``indices`` (ref: mcmc.py:34-134 each) as one stacked run: per chain the reference's pseudo-data
    draw and start positions (numpy's global state, in the reference's order), its two-stage burn-in with the
    restart from its own best points, production, and its own ``closure/results/<index>/`` outputs."""
    from gpemu.sampler import DeviceSampler
    box = config.analysis_config['parameterization'][config.parameterization]
    lower, upper = box['min'], box['max']
    n_par, n_walk, n_ch = len(box['names']), config.n_walkers, len(indices)
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=config.analysis_name, parameterization=config.parameterization,
        analysis_config=config.analysis_config, config_file=config.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    io = _data_IO()
    datas, starts = [], []
    for j in indices:           # the reference's order of draws: pseudo-data of chain j, then its start positions
        datas.append(io.data_array_from_h5(config.output_dir, 'observables.h5', pseudodata_index=j,
                                           observable_filter=emu_cfg.observable_filter))
        starts.append(np.random.uniform(lower, upper, (n_walk, n_par)))
    y_err = np.asarray(datas[0]['y_err'], dtype=np.float64)
    for dat in datas[1:]:
        if not np.array_equal(np.asarray(dat['y_err'], dtype=np.float64), y_err):
            raise ValueError("closure chains must share the experimental uncertainties to be stacked")
    log_posterior.initialize_pool_variables(lower, upper, emu_cfg, emu_results, _with_data_covariance(config, datas[0]),
                                            truncation_cov)
    models = log_posterior.device_models_for_chains(np.stack([np.asarray(dat['y'], dtype=np.float64) for dat in datas]))
    seeds = [int(np.random.randint(0, 2 ** 31 - 1)) for _ in indices]
    sampler = DeviceSampler(models, n_walk, seeds=seeds)
    logger.info(f'Closure tests {indices[0]}..{indices[-1]}: {n_ch} chains x {n_walk} walkers stacked in one sampler')

    def per_chain(arr):         # (steps, C W, ...) -> list of (steps, W, ...)
        return [arr[:, c * n_walk:(c + 1) * n_walk] for c in range(n_ch)]

    def advance(X0, steps):
        # emcee's initial-state checks, per chain (the single-chain path makes them in EnsembleSampler.advance)
        for c, x0 in enumerate(X0):
            if not walkers_independent(x0):
                raise ValueError(f"closure chain {indices[c]}: Initial state has a large condition number. Make sure "
                                 "that your walkers are linearly independent for the best performance")
        sampler.set_state(np.concatenate(X0))
        if np.any(np.isnan(sampler.get_state()[1])):
            raise ValueError("The initial log_prob was NaN")
        done = 0
        while done < steps:
            block = min(config.n_logging_steps - done % config.n_logging_steps, steps - done)
            sampler.run(block)
            done += block
            if done % config.n_logging_steps == 0 or done == steps:
                nacc, it, _ = sampler.counts()
                frac = nacc / float(max(it, 1))
                logger.info(f'  step {done}: acceptance fraction over {n_ch} chains: mean {frac.mean()}, '
                            f'min {frac.min()}, max {frac.max()}')

    first_stage = config.n_burn_steps // 2
    advance(starts, first_stage)
    chain, lps = sampler.get_chain()
    restart = []
    for c, (ch, lp) in enumerate(zip(per_chain(chain), per_chain(lps))):     # ref: mcmc.py:99, per chain
        _, first_seen = np.unique(lp.reshape(-1), return_index=True)
        restart.append(ch.reshape(-1, n_par)[first_seen[-n_walk:]])
    sampler.reset()
    advance(restart, config.n_burn_steps - first_stage)
    state = sampler.get_state()[0]
    sampler.reset()
    advance([state[c * n_walk:(c + 1) * n_walk] for c in range(n_ch)], config.n_sampling_steps)
    chain, lps = sampler.get_chain()
    nacc, iters, _ = sampler.counts()
    # every chain's autocorrelation time from the chain as it sits on the device (its own walkers only)
    taus = []
    for c in range(n_ch):
        try:
            taus.append(sampler.integrated_time(w0=c * n_walk, nw=n_walk))
        except Exception as err:
            logger.info(f'No autocorrelation time (closure {indices[c]}): {err}')
            taus.append(None)
    diags = []
    for c in range(n_ch):           # where the chain lies: before the sampler goes
        part = {}
        _add_diagnostics(config, part, lambda c=c: sampler.diagnostics(chain=c), label=f'closure chain {indices[c]}')
        _add_marginals(config, part, lambda c=c, **kw: sampler.marginals(chain=c, **kw),
                       label=f'closure chain {indices[c]}')
        _add_loo(config, part, lambda c=c, **kw: sampler.loo(chain=c, **kw), label=f'closure chain {indices[c]}')
        _add_reweight(config, part, lambda c=c, **kw: sampler.reweight(chain=c, **kw), label=f'closure chain {indices[c]}',
                      emu_cfg=emu_cfg)
        _add_information_gain(config, part, lambda c=c, **kw: sampler.information_gain(chain=c, **kw),
                              label=f'closure chain {indices[c]}')
        _add_expected_information_gain(config, part, lambda c=c, **kw: sampler.expected_information_gain(chain=c, **kw),
                                       label=f'closure chain {indices[c]}')
        diags.append(part)
    sampler.close()

    validation_design = io.design_array_from_h5(config.output_dir, filename='observables.h5', validation_set=True)
    for c, j in enumerate(indices):
        cfg_j = MCMCConfig(analysis_name=config.analysis_name, parameterization=config.parameterization,
                           analysis_config=config.analysis_config, config_file=config.config_file, closure_index=j)
        one = LoggingEnsembleSampler(n_walk, n_par, log_posterior.log_posterior, seed=seeds[c], sharded=False)
        one._cache = (per_chain(chain)[c].copy(), per_chain(lps)[c].copy(),
                      nacc[c * n_walk:(c + 1) * n_walk].copy(), iters)
        one._frozen = True
        tau = taus[c]
        results = {'chain': one.get_chain(), 'acceptance_fraction': one.acceptance_fraction,
                   'log_prob': one.get_log_prob(), 'autocorrelation_time': tau,
                   'design_point': validation_design[j], 'experimental_pseudodata': datas[c]}
        results.update(diags[c])
        _add_posterior_predictive(config, results, emu_cfg, emu_results, truncation_cov)
        logger.info(f'Writing {cfg_j.mcmc_outputfile}')
        io.write_dict_to_h5(results, cfg_j.mcmc_output_dir, 'mcmc.h5', verbose=True)
        pickle_path = Path(cfg_j.sampler_outputfile)
        pickle_path.parent.mkdir(parents=True, exist_ok=True)
        pickle_path.write_bytes(pickle.dumps(one))


def run_mcmc(config, closure_index=-1):
    """Calibrate the parameters against the data (or, for ``closure_index >= 0``, against the pseudo-data
    of that validation point) with the affine-invariant ensemble sampler (ref: mcmc.py:34-134)."""
    rank, world = _rank_world()
    owner = closure_owner(closure_index, world)
    if owner is not None and owner != rank:
        logger.info(f'closure test {closure_index}: runs on rank {owner}')
        return
    alone = owner is not None          # this rank runs the whole chain by itself
    if getattr(config, 'sampler', 'stretch') == 'hmc':
        reason = hmc_unsupported(config, closure_index, world)
        if reason:
            raise ValueError(f"parameters.mcmc.sampler: hmc: {reason} -- no step has been taken")
        return _run_hmc(config, closure_index)
    if getattr(config, 'n_temperatures', 1) > 1:
        # parallel tempering runs on one GPU: rank 0 (or the closure chain's owner) runs it, the other ranks return;
        # a tempered closure chain runs by itself (not stacked with the other closure points)
        if world > 1 and not alone and rank != 0:
            logger.info('tempered run: runs on rank 0')
            return
        _warn_find_map_not_read(config, 'the tempered run')
        return _run_tempered(config, closure_index)
    if closure_index >= 0 and (alone or world == 1) and _closure_batch_enabled() \
            and 'validation_indices' in config.analysis_config:
        key = _closure_key(config)
        done = _closure_done.setdefault(key, set())
        owned = _closure_indices(config, 0, rank, world)
        if owned and closure_index == owned[0] and log_posterior.chains_can_stack(config):
            for stale in [k for k in _closure_done if k[:3] == key[:3] and k != key]:
                del _closure_done[stale]
            done.clear()                      # a new pass: everything reruns, like the reference
            _warn_find_map_not_read(config, 'the stacked closure chains')
            n_par = len(config.analysis_config['parameterization'][config.parameterization]['names'])
            for batch in _closure_sub_batches(config, owned, n_par):
                _run_closure_batch(config, batch)
                done.update(batch)
            done.discard(closure_index)
            return
        if closure_index in done:
            done.discard(closure_index)       # handed out once; a repeated request reruns the chain by itself
            logger.info(f'closure test {closure_index}: already run with the stacked chains')
            return

    box = config.analysis_config['parameterization'][config.parameterization]
    lower, upper = box['min'], box['max']
    n_par = len(box['names'])
    n_walk = config.n_walkers

    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=config.analysis_name, parameterization=config.parameterization,
        analysis_config=config.analysis_config, config_file=config.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)

    io = _data_IO()
    data = io.data_array_from_h5(config.output_dir, 'observables.h5', pseudodata_index=closure_index,
                                 observable_filter=emu_cfg.observable_filter)
    if closure_index >= 0 and world > 1 and not alone:
        # walker-sharded closure run: the pseudo-data carries random smearing (ref: data_IO.py:371), so every
        # rank conditions on rank 0's draw
        data = dict(data)
        for key in ('y', 'y_err'):
            data[key] = _same_on_all_ranks(np.asarray(data[key], dtype=np.float64))

    # upstream copies this state into every pool worker (ref: mcmc.py:77-78); here it goes to the device once
    data = _with_data_covariance(config, data)
    log_posterior.initialize_pool_variables(lower, upper, emu_cfg, emu_results, data, truncation_cov)
    if getattr(config, 'find_map', False):
        # what the gradient path declines is known now: say so before a step is taken, not after production
        reason = find_map_unsupported(emu_cfg, emu_results)
        if reason:
            raise ValueError(f"parameters.mcmc.find_map: {reason}; remove the key (or the unsupported setting) -- "
                             "no step has been taken")
    sampler = LoggingEnsembleSampler(n_walk, n_par, log_posterior.log_posterior, sharded=False if alone else None)
    logger.info(f'Sampler ready: {n_walk} walkers, {n_par} parameters, {sampler.world_size} GPU process(es)')

    start = np.random.uniform(lower, upper, (n_walk, n_par))       # ref: mcmc.py:88
    if not alone:
        start = _same_on_all_ranks(start)

    # burn-in in two stages; the second restarts from the best distinct points of the first
    first_stage = config.n_burn_steps // 2
    logger.info(f'Burn-in, stage 1 ({first_stage} steps)...')
    sampler.run_mcmc(start, first_stage, n_logging_steps=config.n_logging_steps)
    restart = _best_distinct(sampler, n_walk)
    sampler.reset()
    logger.info(f'Burn-in, stage 2 ({config.n_burn_steps - first_stage} steps) from the best {n_walk} points...')
    state = sampler.run_mcmc(restart, config.n_burn_steps - first_stage, n_logging_steps=config.n_logging_steps)
    sampler.reset()

    logger.info(f'Production ({config.n_sampling_steps} steps)...')
    sampler.run_mcmc(state[0], config.n_sampling_steps, n_logging_steps=config.n_logging_steps)

    if rank != 0 and not alone:
        return
    try:
        tau = sampler.get_autocorr_time()
    except Exception as err:        # chain too short for a reliable estimate (emcee's AutocorrError upstream)
        logger.info(f'No autocorrelation time: {err}')
        tau = None
    results = {'chain': sampler.get_chain(), 'acceptance_fraction': sampler.acceptance_fraction,
               'log_prob': sampler.get_log_prob(), 'autocorrelation_time': tau}
    _add_diagnostics(config, results, sampler.get_diagnostics)
    _add_marginals(config, results, sampler.get_marginals)
    _add_loo(config, results, lambda **kw: sampler.get_loo(models=log_posterior.device_models(n_div=1.0), **kw))
    _add_reweight(config, results,
                  lambda **kw: sampler.get_reweighted(models=log_posterior.device_models(n_div=1.0), **kw),
                  emu_cfg=emu_cfg)
    _add_information_gain(config, results, sampler.get_information_gain)
    _add_expected_information_gain(config, results, lambda **kw: sampler.get_expected_information_gain(
        models=log_posterior.device_models(n_div=1.0), **kw))
    if closure_index >= 0:
        validation_design = io.design_array_from_h5(config.output_dir, filename='observables.h5', validation_set=True)
        results['design_point'] = validation_design[closure_index]
        results['experimental_pseudodata'] = data
    if getattr(config, 'find_map', False):
        # parameters.mcmc.find_map: the maximum from the production chain's best distinct points (the pool still holds
        # this run's data); three more entries in mcmc.h5, none without the key
        logger.info('Maximising the log-posterior from the best points of the chain...')
        try:
            found = find_map_on_pool(lower, upper, n_starts=min(32, n_walk), chain=results['chain'],
                                     log_prob=results['log_prob'])
        except Exception as err:     # the chain is worth more than the maximum: it is written either way
            logger.warning(f'parameters.mcmc.find_map: the maximisation failed ({err!r}); mcmc.h5 is written without '
                           'map_parameters, map_log_prob and map_hessian')
        else:
            results['map_parameters'] = found['map_parameters']
            results['map_log_prob'] = np.float64(found['map_log_prob'])
            results['map_hessian'] = found['hessian']
    _add_posterior_predictive(config, results, emu_cfg, emu_results, truncation_cov)
    _write_outputs(config, results, sampler, io)


def _write_outputs(config, results, sampler, io):
    """mcmc.h5 and the pickled sampler of one run."""
    # the two big outputs -- mcmc.h5 (ref: mcmc.py:125) and the pickled sampler (ref: mcmc.py:131-132), ~0.5 GB each at
    # the shipped length -- are written side by side: the file writes release the interpreter lock
    logger.info(f'Writing {config.mcmc_outputfile}')
    pickle_path = Path(config.sampler_outputfile)
    pickle_path.parent.mkdir(parents=True, exist_ok=True)

    def write_pickle():
        with open(pickle_path, 'wb') as handle:
            pickle.dump(sampler, handle, protocol=pickle.HIGHEST_PROTOCOL)     # streamed: no 0.5 GB bytes object first

    import threading
    failure = []

    def guarded():
        try:
            write_pickle()
        except BaseException as err:     # re-raised in the caller's thread
            failure.append(err)
    side = threading.Thread(target=guarded, name='gpemu-sampler-pickle')
    side.start()
    try:
        io.write_dict_to_h5(results, config.mcmc_output_dir, 'mcmc.h5', verbose=True)
    finally:
        side.join()
    if failure:
        raise failure[0]
    logger.info('MCMC finished.')


####################################################################################################
# Parallel tempering: optional keys under parameters.mcmc -- n_temperatures (absent or 1: the path
# above), t_max, swap_every, prior_rung.  Rung 0 samples the posterior and is what mcmc.h5 and the pickle hold, with the
# same keys and shapes as an untempered run; the ladder adds the log-evidence (thermodynamic integration).
def _run_tempered(config, closure_index):
    from gpemu.sampler import TemperedSampler
    from gpemu.tempering import geometric_ladder
    box = config.analysis_config['parameterization'][config.parameterization]
    lower, upper = box['min'], box['max']
    n_par, n_walk, n_temp = len(box['names']), config.n_walkers, config.n_temperatures
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=config.analysis_name, parameterization=config.parameterization,
        analysis_config=config.analysis_config, config_file=config.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    io = _data_IO()
    data = io.data_array_from_h5(config.output_dir, 'observables.h5', pseudodata_index=closure_index,
                                 observable_filter=emu_cfg.observable_filter)
    data = _with_data_covariance(config, data)
    log_posterior.initialize_pool_variables(lower, upper, emu_cfg, emu_results, data, truncation_cov)
    betas = geometric_ladder(n_temp, config.t_max, prior_rung=config.prior_rung)
    seed = int(np.random.randint(0, 2 ** 31 - 1))          # drawn where the untempered path's sampler draws its seed
    sampler = TemperedSampler(log_posterior.log_posterior._gpemu_device_models(), n_walk, betas, seed=seed,
                              swap_every=config.swap_every)
    logger.info(f'Tempered sampler ready: {n_temp} temperatures x {n_walk} walkers, {n_par} parameters, '
                f'betas {np.array2string(betas, precision=4)}, swaps every {config.swap_every} step(s)')
    start = np.random.uniform(lower, upper, (n_temp * n_walk, n_par))       # ref: mcmc.py:88, for every rung

    def advance(X0, steps):
        if X0 is not None:
            if not walkers_independent(np.asarray(X0).reshape(n_temp, n_walk, n_par)[0]):
                raise ValueError("Initial state has a large condition number. Make sure that your walkers are "
                                 "linearly independent for the best performance")
            sampler.set_state(X0)
            if np.any(np.isnan(sampler.get_state()[1])):
                raise ValueError("The initial log_prob was NaN")
        done = 0
        while done < steps:
            block = min(config.n_logging_steps - done % config.n_logging_steps, steps - done)
            sampler.run(block)
            done += block
            if done % config.n_logging_steps == 0 or done == steps:
                frac = sampler.acceptance_fraction[0]
                logger.info(f'  step {done}: acceptance fraction (beta = 1): mean {frac.mean()}, std {frac.std()}, '
                            f'min {frac.min()}, max {frac.max()}; swap acceptance '
                            f'{np.array2string(sampler.tswap_acceptance_fraction, precision=3)}')

    first_stage = config.n_burn_steps // 2
    logger.info(f'Burn-in, stage 1 ({first_stage} steps)...')
    advance(start, first_stage)
    # only rung 0 restarts from its best distinct points (ref: mcmc.py:99); the hotter rungs continue
    X = sampler.get_state()[0]
    if first_stage > 0:
        chain0, lp0 = sampler.get_chain(temp=0)
        _, first_seen = np.unique(lp0.reshape(-1), return_index=True)
        X[0] = chain0.reshape(-1, n_par)[first_seen[-n_walk:]]
    sampler.reset()
    logger.info(f'Burn-in, stage 2 ({config.n_burn_steps - first_stage} steps) from the best {n_walk} points...')
    advance(X, config.n_burn_steps - first_stage)
    sampler.reset()
    logger.info(f'Production ({config.n_sampling_steps} steps)...')
    advance(None, config.n_sampling_steps)

    chain, lps = sampler.get_chain(temp=0)
    nacc, iters, _ = sampler.counts()
    try:
        tau = sampler.integrated_time(temp=0)
    except Exception as err:        # chain too short for a reliable estimate (emcee's AutocorrError upstream)
        logger.info(f'No autocorrelation time: {err}')
        tau = None
    diag = {}
    _add_diagnostics(config, diag, lambda: sampler.diagnostics(temp=0), label='production chain (beta = 1)')
    _add_marginals(config, diag, lambda **kw: sampler.marginals(temp=0, **kw), label='production chain (beta = 1)')
    _add_loo(config, diag, lambda **kw: sampler.loo(temp=0, **kw), label='production chain (beta = 1)')
    _add_reweight(config, diag, lambda **kw: sampler.reweight(temp=0, **kw), label='production chain (beta = 1)',
                  emu_cfg=emu_cfg)
    _add_information_gain(config, diag, lambda **kw: sampler.information_gain(temp=0, **kw),
                          label='production chain (beta = 1)')
    _add_expected_information_gain(config, diag, lambda **kw: sampler.expected_information_gain(temp=0, **kw),
                                   label='production chain (beta = 1)')
    mean_ll = sampler.mean_log_likelihood()
    log_z, dlog_z = sampler.log_evidence_estimate()
    swap_frac = sampler.tswap_acceptance_fraction
    sampler.close()
    logger.info(f'log-evidence {log_z} +- {dlog_z}; swap acceptance {np.array2string(swap_frac, precision=3)}')

    one = LoggingEnsembleSampler(n_walk, n_par, log_posterior.log_posterior, seed=seed, sharded=False)
    one._cache = (chain, lps, nacc[:n_walk].copy(), iters)
    one._frozen = True
    one.betas, one.log_evidence, one.log_evidence_error = betas, float(log_z), float(dlog_z)
    one.mean_log_likelihood, one.temperature_swap_acceptance_fraction = mean_ll, swap_frac
    results = {'chain': one.get_chain(), 'acceptance_fraction': one.acceptance_fraction,
               'log_prob': one.get_log_prob(), 'autocorrelation_time': tau,
               'betas': betas, 'log_evidence': np.float64(log_z), 'log_evidence_error': np.float64(dlog_z),
               'mean_log_likelihood': mean_ll, 'temperature_swap_acceptance_fraction': swap_frac}
    results.update(diag)
    if closure_index >= 0:
        validation_design = io.design_array_from_h5(config.output_dir, filename='observables.h5', validation_set=True)
        results['design_point'] = validation_design[closure_index]
        results['experimental_pseudodata'] = data
    _add_posterior_predictive(config, results, emu_cfg, emu_results, truncation_cov)
    _write_outputs(config, results, one, io)


####################################################################################################
# Hamiltonian Monte Carlo: optional parameters.mcmc.sampler: hmc (absent or "stretch": the paths
# above), with hmc_n_leapfrog, hmc_target_accept, hmc_step_size.  n_walkers independent chains; n_burn_steps of warm-up
# (step size and diagonal metric adapt), n_sampling_steps of production.  mcmc.h5 keeps the keys and shapes of a
# stretch-move run and adds hmc_step_size, hmc_inverse_metric, hmc_divergences.
def hmc_unsupported(config, closure_index, world):
    """Why ``sampler: hmc`` cannot run this configuration, or None.  Decided before anything is loaded."""
    if getattr(config, 'n_temperatures', 1) > 1:
        return "it cannot be combined with parallel tempering (n_temperatures > 1)"
    if world > 1:
        return f"it runs on one GPU, this job has {world} ranks"
    if closure_index >= 0 and _closure_batch_enabled() and 'validation_indices' in config.analysis_config:
        return ("closure chains are stacked in one stretch-move sampler; run them one by one with GPEMU_CLOSURE_BATCH=0 "
                "or use the stretch sampler")
    return None


def _run_hmc(config, closure_index):
    from gpemu.sampler import HMCSampler
    box = config.analysis_config['parameterization'][config.parameterization]
    lower, upper = box['min'], box['max']
    n_par, n_walk = len(box['names']), config.n_walkers
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=config.analysis_name, parameterization=config.parameterization,
        analysis_config=config.analysis_config, config_file=config.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    io = _data_IO()
    data = io.data_array_from_h5(config.output_dir, 'observables.h5', pseudodata_index=closure_index,
                                 observable_filter=emu_cfg.observable_filter)
    data = _with_data_covariance(config, data)
    log_posterior.initialize_pool_variables(lower, upper, emu_cfg, emu_results, data, truncation_cov)
    # what the gradient path declines is known now: say so before a step is taken
    reason = find_map_unsupported(emu_cfg, emu_results)
    if reason:
        raise ValueError(f"parameters.mcmc.sampler: hmc: {reason}; use the stretch sampler -- no step has been taken")
    seed = int(np.random.randint(0, 2 ** 31 - 1))          # drawn where the stretch path's sampler draws its seed
    sampler = HMCSampler(log_posterior.log_posterior._gpemu_device_models(), n_walk, n_leapfrog=config.hmc_n_leapfrog,
                         step_size=config.hmc_step_size, seed=seed)
    logger.info(f'HMC sampler ready: {n_walk} chains, {n_par} parameters, {config.hmc_n_leapfrog} leapfrog steps')
    start = np.random.uniform(lower, upper, (n_walk, n_par))       # ref: mcmc.py:88
    sampler.set_state(start)
    if np.any(np.isnan(sampler.get_state()[1])):
        raise ValueError("The initial log_prob was NaN")
    # The burn-in keeps the reference's two stages (ref: mcmc.py:88-101).  Uniform starts lie far out in the tails of a
    # narrow posterior, where the one step size the chains share -- adapted to their MEAN accept probability -- is too
    # large for the curvature: such a chain would reject every proposal, also after the warm-up.  So the first half
    # adapts the step size only, from the uniform starts, and the second half, the three-stage warm-up proper, restarts
    # every chain from the best distinct points seen so far, as the stretch path's second stage does.
    first_stage = config.n_burn_steps // 2
    if first_stage > 0:
        logger.info(f'Burn-in, stage 1 ({first_stage} iterations, step size only)...')
        sampler.adapt(True, config.hmc_target_accept)
        sampler.run(first_stage)
        chain1, lp1 = sampler.get_chain()
        _, first_seen = np.unique(lp1.reshape(-1), return_index=True)      # ascending in log-probability
        best = chain1.reshape(-1, n_par)[first_seen[-n_walk:]]
        if best.shape[0] == n_walk:          # (fewer distinct points than chains: the chains go on from where they are)
            sampler.set_state(best)
        sampler.reset()
    logger.info(f'Warm-up ({config.n_burn_steps - first_stage} iterations, target accept probability '
                f'{config.hmc_target_accept})...')
    warm = sampler.warmup(config.n_burn_steps - first_stage, target_accept=config.hmc_target_accept)
    logger.info(f"  step size {warm['step_size']}, mean accept probability {warm['mean_accept_prob']}, "
                f"{warm['divergences']} divergences")
    logger.info(f'Production ({config.n_sampling_steps} iterations)...')
    done = 0
    while done < config.n_sampling_steps:
        block = min(config.n_logging_steps - done % config.n_logging_steps, config.n_sampling_steps - done)
        sampler.run(block)
        done += block
        if done % config.n_logging_steps == 0 or done == config.n_sampling_steps:
            frac = sampler.acceptance_fraction
            logger.info(f'  step {done}: acceptance fraction: mean {frac.mean()}, std {frac.std()}, min {frac.min()}, '
                        f'max {frac.max()}; divergences {int(sampler.divergences.sum())}')
    chain, lps = sampler.get_chain()
    nacc, iters, _ = sampler.counts()
    try:
        tau = sampler.integrated_time()
    except Exception as err:        # chain too short for a reliable estimate (emcee's AutocorrError upstream)
        logger.info(f'No autocorrelation time: {err}')
        tau = None
    diag = {}
    _add_diagnostics(config, diag, sampler.diagnostics)
    _add_marginals(config, diag, sampler.marginals)
    _add_loo(config, diag, sampler.loo)
    _add_reweight(config, diag, sampler.reweight, emu_cfg=emu_cfg)
    _add_information_gain(config, diag, sampler.information_gain)
    _add_expected_information_gain(config, diag, sampler.expected_information_gain)
    step_size, inverse_metric, divergences = sampler.step_size, sampler.inverse_metric, sampler.divergences
    sampler.close()

    one = LoggingEnsembleSampler(n_walk, n_par, log_posterior.log_posterior, seed=seed, sharded=False)
    one._cache = (chain, lps, nacc.copy(), iters)
    one._frozen = True
    one.hmc_step_size, one.hmc_inverse_metric, one.hmc_divergences = step_size, inverse_metric, divergences
    results = {'chain': one.get_chain(), 'acceptance_fraction': one.acceptance_fraction,
               'log_prob': one.get_log_prob(), 'autocorrelation_time': tau,
               'hmc_step_size': np.float64(step_size), 'hmc_inverse_metric': inverse_metric, 'hmc_divergences': divergences}
    results.update(diag)
    if closure_index >= 0:
        validation_design = io.design_array_from_h5(config.output_dir, filename='observables.h5', validation_set=True)
        results['design_point'] = validation_design[closure_index]
        results['experimental_pseudodata'] = data
    if getattr(config, 'find_map', False):
        logger.info('Maximising the log-posterior from the best points of the chain...')
        try:
            found = find_map_on_pool(lower, upper, n_starts=min(32, n_walk), chain=results['chain'],
                                     log_prob=results['log_prob'])
        except Exception as err:     # the chain is worth more than the maximum: it is written either way
            logger.warning(f'parameters.mcmc.find_map: the maximisation failed ({err!r}); mcmc.h5 is written without '
                           'map_parameters, map_log_prob and map_hessian')
        else:
            results['map_parameters'] = found['map_parameters']
            results['map_log_prob'] = np.float64(found['map_log_prob'])
            results['map_hessian'] = found['hessian']
    _add_posterior_predictive(config, results, emu_cfg, emu_results, truncation_cov)
    _write_outputs(config, results, one, io)


####################################################################################################
def posterior_predictive_settings(mc):
    """(on, probabilities) from the ``parameters.mcmc`` mapping: ``posterior_predictive`` (default off) and the
    optional ``posterior_predictive_probabilities`` (default 0.05, 0.5, 0.95; each in [0, 1])."""
    on = bool(mc.get('posterior_predictive', False))
    probs = mc.get('posterior_predictive_probabilities')
    if probs is None:
        probs = emulation.POSTERIOR_PREDICTIVE_PROBABILITIES
    probs = tuple(float(p) for p in np.atleast_1d(np.asarray(probs, dtype=np.float64)))
    if not probs or not all(0.0 <= p <= 1.0 for p in probs):
        raise ValueError("parameters.mcmc.posterior_predictive_probabilities must be probabilities in [0, 1], got "
                         f"{probs}")
    return on, probs


def diagnostics_settings(mc):
    """``parameters.mcmc.diagnostics`` (default off) from the ``parameters.mcmc`` mapping: rank-normalised split-R-hat,
    bulk / tail ESS, the ESS of the mean and its Monte Carlo standard error of the production chain into mcmc.h5."""
    on = mc.get('diagnostics', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.diagnostics must be true or false, got {on!r}")
    return bool(on)


DIAGNOSTICS_KEYS = ('rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean')
RHAT_THRESHOLD = 1.01      # Vehtari et al. (2021)


def _add_diagnostics(config, results, compute, label='production chain'):
    """With ``parameters.mcmc.diagnostics``: the five ``(d,)`` arrays of ``compute()`` (a sampler's ``diagnostics`` on
    the chain where it lies) into the results that go to mcmc.h5, one log line, and a warning where max R-hat exceeds
    1.01.  The walkers of a stretch ensemble are not independent chains: R-hat compares walkers there."""
    if not getattr(config, 'diagnostics', False):
        return
    try:
        diag = compute()
    except Exception as err:         # e.g. fewer than 8 stored steps: the chain is written either way
        logger.warning(f'parameters.mcmc.diagnostics: not computed ({err!r}); mcmc.h5 is written without '
                       + ', '.join(DIAGNOSTICS_KEYS))
        return
    for key in DIAGNOSTICS_KEYS:
        results[key] = np.asarray(diag[key], dtype=np.float64)
    from gpemu.diagnostics import log_line
    line, warn = log_line(diag, label=f"Diagnostics of the {label} ({diag['n_chains']} split chains x "
                                      f"{diag['n_draws']} draws)")
    logger.info(line)
    if warn:
        logger.warning(f"max R-hat {np.nanmax(results['rhat']):.4f} > {RHAT_THRESHOLD}: the chains have not mixed")


def _stored_chain(config, closure_index, discard, thin):
    """``(config, chain)``: steps ``[discard::thin]`` of the chain stored in mcmc.h5, ``(steps, walkers, d)`` -- with
    ``closure_index >= 0`` that of closure chain ``closure_index``, under the configuration rebuilt for it."""
    if closure_index >= 0:
        config = MCMCConfig(analysis_name=config.analysis_name, parameterization=config.parameterization,
                            analysis_config=config.analysis_config, config_file=config.config_file,
                            closure_index=closure_index)
    if int(discard) < 0 or int(thin) < 1:
        raise ValueError("discard must be >= 0 and thin >= 1")
    stored = _data_IO().read_dict_from_h5(config.mcmc_output_dir, 'mcmc.h5')
    chain = np.asarray(stored['chain'], dtype=np.float64)[int(discard)::int(thin)]
    if chain.shape[0] == 0:
        raise ValueError("no stored steps after discard")
    return config, chain


def diagnostics(config, closure_index=-1, discard=0, thin=1):
    """The five diagnostics (``gpemu.diagnostics.summary``) of the chain stored in mcmc.h5 (of closure chain
    ``closure_index``, if >= 0), steps ``[discard::thin]``, every walker as a chain."""
    _, chain = _stored_chain(config, closure_index, discard, thin)
    from gpemu import diagnostics as _diag
    return _diag.summary(np.ascontiguousarray(chain))


def marginals_settings(mc, default_confidence=None):
    """``(on, (bins_1d, bins_2d), confidence, kde)`` from the ``parameters.mcmc`` mapping: ``marginals`` (true or false,
    default off) and the optional ``marginals_bins`` (``[bins_1d, bins_2d]``, default 100 and 50),
    ``marginals_confidence`` (a list of levels in (0, 1); default ``[default_confidence]`` -- the configuration's
    ``confidence``, if it has one -- else 0.9) and ``marginals_kde`` (true or false, default on).  DESIGN.md §4.29."""
    on = mc.get('marginals', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.marginals must be true or false, got {on!r}")
    kde = mc.get('marginals_kde', True)
    if not isinstance(kde, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.marginals_kde must be true or false, got {kde!r}")
    bins = mc.get('marginals_bins', (100, 50))
    ok = isinstance(bins, (list, tuple)) and len(bins) == 2 and all(
        isinstance(b, (int, np.integer)) and not isinstance(b, (bool, np.bool_)) for b in bins)
    if not ok or not (1 <= bins[0] <= 4096 and 1 <= bins[1] <= 256):
        raise ValueError("parameters.mcmc.marginals_bins must be [bins_1d, bins_2d], integers in [1, 4096] and [1, 256], "
                         f"got {bins!r}")
    conf = mc.get('marginals_confidence')
    if conf is None:
        conf = [0.9 if default_confidence is None else default_confidence]
    try:
        ok = isinstance(conf, (list, tuple)) and len(conf) > 0 and all(
            not isinstance(c, (bool, np.bool_)) and 0.0 < float(c) < 1.0 for c in conf)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"parameters.mcmc.marginals_confidence must be a list of levels in (0, 1), got {conf!r}")
    return bool(on), (int(bins[0]), int(bins[1])), tuple(float(c) for c in conf), bool(kde)


def marginals_kde2d_settings(mc):
    """``(on, n_grid, covariance)`` from the ``parameters.mcmc`` mapping: ``marginals_kde2d`` (true or false, default
    off: the 2-D kernel densities of all parameter pairs beside the other marginals), ``marginals_kde2d_grid`` (points
    per axis, an integer in [1, 512], default 100) and ``marginals_kde2d_covariance`` (``full`` -- scipy's
    ``gaussian_kde`` on a sheared grid -- or ``diagonal``, default ``full``).  DESIGN.md §4.33."""
    on = mc.get('marginals_kde2d', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.marginals_kde2d must be true or false, got {on!r}")
    grid = mc.get('marginals_kde2d_grid', 100)
    if not isinstance(grid, (int, np.integer)) or isinstance(grid, (bool, np.bool_)) or not 1 <= grid <= 512:
        raise ValueError(f"parameters.mcmc.marginals_kde2d_grid must be an integer in [1, 512], got {grid!r}")
    cov = mc.get('marginals_kde2d_covariance', 'full')
    if cov not in ('full', 'diagonal'):
        raise ValueError(f"parameters.mcmc.marginals_kde2d_covariance must be 'full' or 'diagonal', got {cov!r}")
    return bool(on), int(grid), str(cov)


MARGINALS_KEYS = ('edges_1d', 'edges_2d', 'hist_1d', 'pairs', 'hist_2d', 'n_inside', 'confidence', 'hpd')
MARGINALS_KDE_KEYS = ('kde_grid', 'kde_density', 'kde_bandwidth')
MARGINALS_KDE2D_KEYS = ('kde2d_pairs', 'kde2d_shear', 'kde2d_bandwidth', 'kde2d_grid_a', 'kde2d_grid_b', 'kde2d_density')


def _marginals_kwargs(config):
    """The arguments of ``DeviceSampler.marginals`` / ``gpemu.marginals.summary`` from the configuration: the prior box
    of the parameterization and the ``marginals_*`` settings (the 2-D density's only where it is on)."""
    box = config.analysis_config['parameterization'][config.parameterization]
    kw = dict(lower=np.asarray(box['min'], dtype=np.float64), upper=np.asarray(box['max'], dtype=np.float64),
              bins_1d=config.marginals_bins[0], bins_2d=config.marginals_bins[1],
              confidence=config.marginals_confidence, kde=config.marginals_kde)
    if getattr(config, 'marginals_kde2d', False):
        kw.update(kde2d=True, n_grid_2d=config.marginals_kde2d_grid, covariance_2d=config.marginals_kde2d_covariance)
    return kw


def _add_marginals(config, results, compute, label='production chain'):
    """With ``parameters.mcmc.marginals``: ``marginal_<key>`` for the keys of ``compute(**kwargs)`` (a sampler's
    ``marginals`` on the chain where it lies) into the results that go to mcmc.h5 -- histogram counts as int64, the
    rest float64 -- and one log line."""
    if not getattr(config, 'marginals', False):
        return
    keys = MARGINALS_KEYS + (MARGINALS_KDE_KEYS if config.marginals_kde else ())
    kwargs = _marginals_kwargs(config)
    out = None
    if kwargs.get('kde2d'):          # the 2-D densities fail on their own (e.g. two linearly dependent parameters)
        try:
            out = compute(**kwargs)
            keys = keys + MARGINALS_KDE2D_KEYS
        except ValueError as err:
            logger.warning(f'parameters.mcmc.marginals_kde2d: not computed ({err!r}); mcmc.h5 is written without '
                           + ', '.join(f'marginal_{k}' for k in MARGINALS_KDE2D_KEYS))
            kwargs = {k: v for k, v in kwargs.items() if k not in ('kde2d', 'n_grid_2d', 'covariance_2d')}
    try:
        if out is None:
            out = compute(**kwargs)
    except ValueError as err:        # e.g. too few stored samples for a level: the chain is written either way (a
        # device failure is not caught: it ends the run)
        logger.warning(f'parameters.mcmc.marginals: not computed ({err!r}); mcmc.h5 is written without '
                       + ', '.join(f'marginal_{k}' for k in keys))
        return
    for key in keys:
        results[f'marginal_{key}'] = np.asarray(out[key])
    n = int(np.asarray(results['marginal_n_inside']).max(initial=0))
    logger.info(f"Marginals of the {label}: {out['hist_1d'].shape[1]} / {out['hist_2d'].shape[-1]}^2 bins, "
                f"{out['pairs'].shape[0]} pairs, HPD at {list(config.marginals_confidence)}, up to {n} samples in "
                "the box")


def marginals(config, closure_index=-1, discard=0, thin=1):
    """The marginals (``gpemu.marginals.summary``) of the chain stored in mcmc.h5 (of closure chain ``closure_index``,
    if >= 0), steps ``[discard::thin]``, all walkers, with the configuration's box and ``marginals_*`` settings."""
    config, chain = _stored_chain(config, closure_index, discard, thin)
    from gpemu import marginals as _marg
    return _marg.summary(np.ascontiguousarray(chain.reshape(-1, chain.shape[-1])), **_marginals_kwargs(config))


def loo_settings(mc):
    """``(on, leave_out)`` from the ``parameters.mcmc`` mapping: ``loo`` (true or false, default off) and the optional
    ``loo_leave_out``, a non-empty list of non-empty lists of observable labels -- the classes of observables left out
    together (default: every observable on its own).  DESIGN.md §4.31."""
    on = mc.get('loo', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.loo must be true or false, got {on!r}")
    groups = mc.get('loo_leave_out')
    if groups is not None:
        ok = isinstance(groups, (list, tuple)) and len(groups) > 0 and all(
            isinstance(g, (list, tuple)) and len(g) > 0 and all(isinstance(v, str) and v for v in g) for g in groups)
        if not ok:
            raise ValueError("parameters.mcmc.loo_leave_out must be a non-empty list of non-empty lists of observable "
                             f"labels, got {groups!r}")
        groups = [[str(v) for v in g] for g in groups]
    return bool(on), groups


LOO_KEYS = ('labels', 'elpd_loo', 'p_loo', 'pareto_k', 'k_threshold', 'ess_w', 'elpd_waic', 'p_waic', 'lppd', 'se')
LOO_SHIFT_KEYS = ('loo_mean', 'loo_sd', 'shift')


def _loo_kwargs(config):
    """``leave_out`` (rows of the terms, from the labels of ``parameters.mcmc.loo_leave_out``) and the observable
    labels for ``DeviceSampler.loo`` / ``gpemu.loo.chain_loo``, on the pool's state."""
    labels = log_posterior.observable_labels()
    rows = None
    if getattr(config, 'loo_leave_out', None):
        rows = []
        for group in config.loo_leave_out:
            for name in group:
                if labels.count(name) != 1:
                    raise ValueError(f"parameters.mcmc.loo_leave_out names {name!r}; the observables are {labels}")
            rows.append([labels.index(name) for name in group])
    return labels, rows


def _loo_entries(out, labels, rows):
    """the ``loo_*`` entries of mcmc.h5 from a loo table: the observables by name"""
    names = labels if rows is None else ['+'.join(labels[o] for o in g) for g in rows]
    entries = {'loo_labels': np.array(names)}
    for key in LOO_KEYS[1:-1]:
        entries[f'loo_{key}'] = np.asarray(out[key], dtype=np.float64)
    entries['loo_se'] = np.float64(out['se'])
    for key in LOO_SHIFT_KEYS:
        if key in out:
            entries['loo_' + key.replace('loo_', 'weighted_')] = np.asarray(out[key], dtype=np.float64)
    return entries


def _add_loo(config, results, compute, label='production chain'):
    """With ``parameters.mcmc.loo``: the ``loo_*`` entries of ``compute(leave_out=...)`` (a sampler's ``loo`` on the
    chain where it lies) into the results that go to mcmc.h5, one log line, and a warning where a Pareto k-hat
    exceeds its threshold."""
    if not getattr(config, 'loo', False):
        return
    try:
        labels, rows = _loo_kwargs(config)
        out = compute(leave_out=rows)
        entries = _loo_entries(out, labels, rows)
    except Exception as err:         # the chain is worth more than the table: it is written either way
        logger.warning(f'parameters.mcmc.loo: not computed ({err!r}); mcmc.h5 is written without the loo_* entries')
        return
    results.update(entries)
    logger.info(f"PSIS-LOO of the {label}: elpd_loo {out['elpd_loo_total']:.3f} +- {out['se']:.3f}, p_loo "
                f"{out['p_loo_total']:.3f} over {out['n_obs']} observables, {out['n_samples']} samples; largest Pareto "
                f"k-hat {np.max(out['pareto_k']):.3f}")
    if np.any(out['warning']):
        bad = [str(n) for n, w in zip(entries['loo_labels'], out['warning']) if w]
        logger.warning(f"Pareto k-hat above {out['k_threshold'][0]:.2f} for {bad}: their leave-one-out estimates are "
                       "not reliable")


def loo(config, closure_index=-1, discard=0, thin=1):
    """The ``loo_*`` entries (``gpemu.loo.chain_loo``) of the chain stored in mcmc.h5 (of closure chain
    ``closure_index``, if >= 0, against its stored pseudo-data), steps ``[discard::thin]``, all walkers."""
    cfg, chain = _stored_chain(config, closure_index, discard, thin)
    box = cfg.analysis_config['parameterization'][cfg.parameterization]
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=cfg.analysis_name, parameterization=cfg.parameterization,
        analysis_config=cfg.analysis_config, config_file=cfg.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    io = _data_IO()
    if closure_index >= 0:
        data = io.read_dict_from_h5(cfg.mcmc_output_dir, 'mcmc.h5')['experimental_pseudodata']
    else:
        data = io.data_array_from_h5(cfg.output_dir, 'observables.h5', pseudodata_index=-1,
                                     observable_filter=emu_cfg.observable_filter)
    log_posterior.initialize_pool_variables(box['min'], box['max'], emu_cfg, emu_results,
                                            _with_data_covariance(cfg, data), truncation_cov)
    from gpemu import loo as _loo
    labels, rows = _loo_kwargs(cfg)
    out = _loo.chain_loo(log_posterior.device_models(n_div=1.0), np.ascontiguousarray(chain.reshape(-1, chain.shape[-1])),
                         leave_out=rows)
    return _loo_entries(out, labels, rows)


def reweight_settings(mc):
    """The scenarios of ``parameters.mcmc.reweight`` (default: none): ``None`` without the key, else a list of ``(name,
    priors)``.  The key takes either ``{reference_prior: true}`` -- one scenario ``reference_prior``: log-uniform for
    every parameter whose name contains ``c_`` (ref: plot_qhat.py:313-316), ``priors`` ``None`` here -- or a list of
    named scenarios ``{name: <word>, priors: {<parameter name>: {kind: flat | log_uniform | normal | log_normal, a: ..,
    b: ..}}}`` (``a``, ``b`` for ``normal`` and ``log_normal``); parameters not named stay flat.  DESIGN.md §4.39."""
    spec = mc.get('reweight')
    if spec is None or spec is False:
        return None
    if isinstance(spec, dict):
        on = spec.get('reference_prior')
        if set(spec) != {'reference_prior'} or not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"parameters.mcmc.reweight must be {{reference_prior: true}} or a list of named scenarios, "
                             f"got {spec!r}")
        return [('reference_prior', None)] if on else None
    if not isinstance(spec, (list, tuple)) or len(spec) == 0:
        raise ValueError(f"parameters.mcmc.reweight must be {{reference_prior: true}} or a non-empty list of named "
                         f"scenarios, got {spec!r}")
    out = []
    for sc in spec:
        ok = isinstance(sc, dict) and set(sc) == {'name', 'priors'} and isinstance(sc['name'], str) and \
            re.fullmatch(r'[A-Za-z0-9_]+', sc['name']) and isinstance(sc['priors'], dict) and len(sc['priors']) > 0
        if not ok:
            raise ValueError("every scenario of parameters.mcmc.reweight needs a name (letters, digits, _) and priors, a "
                             f"mapping from parameter names, got {sc!r}")
        priors = {}
        for par, e in sc['priors'].items():
            if not isinstance(e, dict) or not set(e) <= {'kind', 'a', 'b'} or e.get('kind') not in REWEIGHT_KINDS:
                raise ValueError(f"scenario {sc['name']!r}: the prior of {par!r} needs a kind among {REWEIGHT_KINDS} and, "
                                 f"for normal and log_normal, a and b; got {e!r}")
            if e['kind'] in ('normal', 'log_normal'):
                a, b = e.get('a'), e.get('b')
                num = all(isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v) for v in (a, b))
                if not num or not b > 0:
                    raise ValueError(f"scenario {sc['name']!r}: {par!r} needs a finite a and a finite b > 0, got {e!r}")
            priors[str(par)] = dict(e)
        if sc['name'] in [n for n, _ in out]:
            raise ValueError(f"parameters.mcmc.reweight names scenario {sc['name']!r} twice")
        out.append((sc['name'], priors))
    return out


def reweight_summaries_settings(mc):
    """``parameters.mcmc.reweight_summaries`` (default: none): ``None`` without the key, else ``{'hpd': [levels] or None,
    'kde': bool, 'posterior_predictive': bool}`` -- the weighted highest-density intervals, 1-D kernel densities and
    posterior-predictive bands of every scenario of ``parameters.mcmc.reweight``.  The key takes a
    mapping with any of ``hpd`` (a non-empty list of confidence levels in (0, 1)), ``kde`` and ``posterior_predictive``
    (true or false); unknown sub-keys, and the key without ``parameters.mcmc.reweight``, are a ValueError."""
    spec = mc.get('reweight_summaries')
    if spec is None:
        return None
    if not isinstance(spec, dict) or not set(spec) <= set(REWEIGHT_SUMMARIES):
        raise ValueError(f"parameters.mcmc.reweight_summaries takes a mapping with {REWEIGHT_SUMMARIES}, got {spec!r}")
    if reweight_settings(mc) is None:
        raise ValueError("parameters.mcmc.reweight_summaries needs parameters.mcmc.reweight: there is no scenario to "
                         "summarise")
    out = {'hpd': None, 'kde': False, 'posterior_predictive': False}
    for key in ('kde', 'posterior_predictive'):
        v = spec.get(key, False)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"parameters.mcmc.reweight_summaries.{key} must be true or false, got {v!r}")
        out[key] = bool(v)
    hpd = spec.get('hpd')
    if hpd is not None:
        ok = isinstance(hpd, (list, tuple)) and len(hpd) > 0 and all(
            isinstance(c, (int, float)) and not isinstance(c, bool) and 0.0 < float(c) < 1.0 for c in hpd)
        if not ok:
            raise ValueError("parameters.mcmc.reweight_summaries.hpd must be a non-empty list of confidence levels in "
                             f"(0, 1), got {hpd!r}")
        out['hpd'] = [float(c) for c in hpd]
    return out


REWEIGHT_SUMMARIES = ('hpd', 'kde', 'posterior_predictive')
REWEIGHT_PP_KEYS = ('mean', 'variance_parameters', 'variance_emulator', 'quantiles')
REWEIGHT_KINDS = ('flat', 'log_uniform', 'normal', 'log_normal')
REWEIGHT_KEYS = ('pareto_k', 'k_threshold', 'ess_w', 'reliable', 'log_mean_ratio', 'log_evidence_ratio', 'mean', 'sd',
                 'shift', 'quantiles', 'hist_1d', 'hist_2d', 'hist_1d_q', 'hist_2d_q', 'Q')
REWEIGHT_SHARED_KEYS = ('probabilities', 'edges_1d', 'edges_2d', 'pairs')


def _reweight_kwargs(config, scenarios=None):
    """``(names, priors, lower, upper)`` for ``DeviceSampler.reweight`` / ``gpemu.reweight.chain_reweight``: the
    scenarios of the configuration (or ``scenarios``, in ``reweight_settings``' form) by parameter index."""
    from gpemu import reweight as _rw
    box = config.analysis_config['parameterization'][config.parameterization]
    par = [str(n) for n in box['names']]
    scenarios = config.reweight if scenarios is None else scenarios
    if not scenarios:
        raise ValueError('no reweighting scenario')
    names, priors = [], []
    for name, spec in scenarios:
        if spec is None:
            priors.append(_rw.reference_prior(par))
        else:
            row = {}
            for pname, e in spec.items():
                if par.count(pname) != 1:
                    raise ValueError(f"parameters.mcmc.reweight names {pname!r}; the parameters are {par}")
                row[par.index(pname)] = e
            priors.append(row)
        names.append(name)
    return names, priors, np.asarray(box['min'], dtype=np.float64), np.asarray(box['max'], dtype=np.float64)


def _reweight_summary_kwargs(config):
    """the options of ``parameters.mcmc.reweight_summaries`` as keywords of a sampler's ``reweight``"""
    summ = getattr(config, 'reweight_summaries', None) or {}
    kw = {}
    if summ.get('hpd') is not None:
        kw['hpd'] = list(summ['hpd'])
    if summ.get('kde'):
        kw['kde'] = True
    if summ.get('posterior_predictive'):
        kw['posterior_predictive'] = True
    return kw


def _pp_merger(emu_cfg):
    """the bands of the groups' models (in the groups' order) into the merged observable order of ``predict``"""
    def merge(per_model):
        return emulation.merge_posterior_predictive(emu_cfg.sort_observables_in_matrix,
                                                    dict(zip(emu_cfg.emulation_groups_config, per_model)))
    return merge


def _reweight_summary_entries(out, names, merge_pp=None):
    """the entries of ``parameters.mcmc.reweight_summaries``: ``reweight_hpd_confidence`` and, per scenario,
    ``reweight_<name>_hpd``, ``reweight_<name>_kde_{grid,density,bandwidth}``,
    ``reweight_<name>_pp_{mean,variance_parameters,variance_emulator,quantiles}`` -- those the scenarios' dicts hold"""
    entries = {}
    if 'hpd' in out[0]:
        entries['reweight_hpd_confidence'] = np.asarray(out[0]['hpd_confidence'])
    for name, res in zip(names, out):
        if 'hpd' in res:
            entries[f'reweight_{name}_hpd'] = np.asarray(res['hpd'])
        for key in ('grid', 'density', 'bandwidth'):
            if f'kde_{key}' in res:
                entries[f'reweight_{name}_kde_{key}'] = np.asarray(res[f'kde_{key}'])
        pp = res.get('posterior_predictive')
        if pp is not None:
            pp = merge_pp(pp) if isinstance(pp, list) else pp
            for key in REWEIGHT_PP_KEYS:
                entries[f'reweight_{name}_pp_{key}'] = np.asarray(pp[key])
    return entries


def _reweight_entries(out, names):
    """the ``reweight_*`` entries of mcmc.h5 from the scenarios' dicts: ``reweight_names``, the shared
    ``reweight_probabilities``, ``reweight_edges_1d``, ``reweight_edges_2d``, ``reweight_pairs`` and, per scenario,
    ``reweight_<name>_<key>`` for the ``REWEIGHT_KEYS`` (``log_evidence_ratio``: NaN where there is none)"""
    entries = {'reweight_names': np.array(names)}
    for key in REWEIGHT_SHARED_KEYS:
        entries[f'reweight_{key}'] = np.asarray(out[0][key])
    for name, res in zip(names, out):
        for key in REWEIGHT_KEYS:
            v = res[key]
            if key == 'log_evidence_ratio' and v is None:
                v = np.nan
            if key == 'Q':
                v = np.uint64(v)
            entries[f'reweight_{name}_{key}'] = np.asarray(v)
    return entries


def _add_reweight(config, results, compute, label='production chain', emu_cfg=None):
    """With ``parameters.mcmc.reweight``: the ``reweight_*`` entries of ``compute(priors=..., lower=..., upper=...)`` (a
    sampler's ``reweight`` on the chain where it lies) into the results that go to mcmc.h5, one log line per scenario,
    and a warning where a Pareto k-hat exceeds its threshold: that scenario needs its own run.  With
    ``parameters.mcmc.reweight_summaries`` the same call carries its options and their entries are added (``emu_cfg``:
    the emulation configuration, for the merged observable order of the bands); where they fail, that is logged and the
    ``reweight_*`` entries are those of a run without the key."""
    if not getattr(config, 'reweight', None):
        return
    try:
        names, priors, lower, upper = _reweight_kwargs(config)
        more, extra_entries = _reweight_summary_kwargs(config), {}
        if more:
            try:
                out = compute(priors=priors, lower=lower, upper=upper, **more)
                extra_entries = _reweight_summary_entries(out, names, None if emu_cfg is None else _pp_merger(emu_cfg))
            except Exception as err:
                logger.warning(f'parameters.mcmc.reweight_summaries: not computed ({err!r}); mcmc.h5 is written without '
                               'its entries')
                more = {}
        if not more:
            out = compute(priors=priors, lower=lower, upper=upper)
        entries = dict(_reweight_entries(out, names), **extra_entries)
    except Exception as err:         # the chain is worth more than the table: it is written either way
        logger.warning(f'parameters.mcmc.reweight: not computed ({err!r}); mcmc.h5 is written without the reweight_* '
                       'entries')
        return
    results.update(entries)
    for name, res in zip(names, out):
        logger.info(f"Reweighting of the {label} to {name!r}: Pareto k-hat {res['pareto_k']:.3f}, effective sample size "
                    f"{res['ess_w']:.1f}, largest shift {np.max(np.abs(res['shift'])):.3f} sd")
        if not res['reliable']:
            logger.warning(f"Pareto k-hat {res['pareto_k']:.3f} above {res['k_threshold']:.2f} for scenario {name!r}: the "
                           "reweighted posterior is not reliable, this scenario needs its own run")


def reweight(config, closure_index=-1, discard=0, thin=1, priors=None, reference_prior=False, hpd=None, kde=None,
             posterior_predictive=None, **summary_kw):
    """The ``reweight_*`` entries (``gpemu.reweight.summary``) of the chain stored in mcmc.h5 (of closure chain
    ``closure_index``, if >= 0), steps ``[discard::thin]``, all walkers, inside the configuration's box.  The scenarios
    are those of ``parameters.mcmc.reweight`` unless ``priors`` (that key's list form) or ``reference_prior=True`` gives
    others.  ``hpd``, ``kde``, ``posterior_predictive``: the options of ``parameters.mcmc.reweight_summaries`` (default:
    that key's) and their entries; the bands come from ``emulation.posterior_predictive(weights=...)``.
    ``summary_kw``: ``probabilities``, ``bins_1d``, ``bins_2d``, ``smooth``."""
    cfg, chain = _stored_chain(config, closure_index, discard, thin)
    more = _reweight_summary_kwargs(cfg)
    for key, v in (('hpd', hpd), ('kde', kde), ('posterior_predictive', posterior_predictive)):
        if v is not None:
            more[key] = v
    want_pp = bool(more.pop('posterior_predictive', False))
    if not more.get('kde', True):
        more.pop('kde')
    scenarios = None
    if reference_prior:
        scenarios = reweight_settings({'reweight': {'reference_prior': True}})
    elif priors is not None:
        scenarios = reweight_settings({'reweight': priors})
    from gpemu import reweight as _rw
    names, pri, lower, upper = _reweight_kwargs(cfg, scenarios)
    x = np.ascontiguousarray(chain.reshape(-1, chain.shape[-1]))
    L = _rw.log_ratio(x, priors=pri, lower=lower, upper=upper)
    log_norm = _rw.log_prior_norm(*_rw.check_priors(pri, x.shape[1], lower, upper), lower, upper)
    extra = None
    if want_pp:
        emu_cfg = emulation.EmulationConfig.from_config_file(
            analysis_name=cfg.analysis_name, parameterization=cfg.parameterization,
            analysis_config=cfg.analysis_config, config_file=cfg.config_file)
        emu_results = emu_cfg.read_all_emulator_groups()
        truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
        probs = summary_kw.get('probabilities', emulation.POSTERIOR_PREDICTIVE_PROBABILITIES)

        def extra(q, Q):
            merged = emulation.posterior_predictive(x, emu_cfg, emulation_group_results=emu_results,
                                                    emulator_cov_unexplained=truncation_cov, probabilities=probs, weights=q)
            return [{'posterior_predictive': m} for m in merged]
    out = _rw.summary(x, L, lower, upper, log_norm=log_norm, extra=extra, **more, **summary_kw)
    return dict(_reweight_entries(out, names), **_reweight_summary_entries(out, names))


def information_gain_settings(mc):
    """``(on, k, max_points)`` from the ``parameters.mcmc`` mapping: ``information_gain`` (true or false, default off: how
    many nats the data taught about every parameter, every pair and all of them jointly), ``information_gain_k`` (the
    neighbour the estimator uses, an integer in [1, 16], default 4) and ``information_gain_max_points`` (the most evenly
    spaced rows of the chain it is taken over, an integer >= 2, default 65536).  DESIGN.md §4.35."""
    on = mc.get('information_gain', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.information_gain must be true or false, got {on!r}")
    k = mc.get('information_gain_k', 4)
    if not isinstance(k, (int, np.integer)) or isinstance(k, (bool, np.bool_)) or not 1 <= k <= 16:
        raise ValueError(f"parameters.mcmc.information_gain_k must be an integer in [1, 16], got {k!r}")
    n = mc.get('information_gain_max_points', 65536)
    if not isinstance(n, (int, np.integer)) or isinstance(n, (bool, np.bool_)) or not 2 <= n < 2 ** 31:
        raise ValueError(f"parameters.mcmc.information_gain_max_points must be an integer in [2, 2^31), got {n!r}")
    return bool(on), int(k), int(n)


INFORMATION_GAIN_KEYS = ('masks', 'dims', 'nats', 'bits', 'se', 'n_used', 'copies', 'n_points', 'k', 'joint',
                         'per_parameter', 'pairs', 'per_pair')


def _information_gain_kwargs(config):
    """The arguments of ``DeviceSampler.information_gain`` / ``gpemu.information.information_gain`` from the
    configuration: the prior box of the parameterization and the ``information_gain_*`` settings.  The drop-in allows
    copies -- an unthinned ensemble chain always holds them -- and reports their number instead."""
    box = config.analysis_config['parameterization'][config.parameterization]
    return dict(lower=np.asarray(box['min'], dtype=np.float64), upper=np.asarray(box['max'], dtype=np.float64),
                k=config.information_gain_k, max_points=config.information_gain_max_points, allow_copies=True)


def _information_gain_entries(out):
    """the ``information_gain_*`` entries of mcmc.h5 from a result: the subsets as bit masks over the parameters"""
    ent = {'masks': np.array([sum(1 << j for j in s) for s in out['subsets']], dtype=np.int64)}
    for key in ('dims', 'n_used', 'copies', 'pairs'):
        ent[key] = np.asarray(out[key], dtype=np.int64)
    for key in ('nats', 'bits', 'se', 'per_parameter', 'per_pair'):
        ent[key] = np.asarray(out[key], dtype=np.float64)
    ent['n_points'], ent['k'] = np.int64(out['n_points']), np.int64(out['k'])
    ent['joint'] = np.float64(out['joint'])
    return {f'information_gain_{key}': ent[key] for key in INFORMATION_GAIN_KEYS}


def _add_information_gain(config, results, compute, label='production chain'):
    """With ``parameters.mcmc.information_gain``: the ``information_gain_*`` entries of ``compute(**kwargs)`` (a
    sampler's ``information_gain`` on the chain where it lies) into the results that go to mcmc.h5, one log line, and a
    warning where more than a tenth of the rows are copies (the estimate then wants a thinned chain)."""
    if not getattr(config, 'information_gain', False):
        return
    try:
        out = compute(**_information_gain_kwargs(config))
        entries = _information_gain_entries(out)
    except Exception as err:         # the chain is worth more than the number: it is written either way
        logger.warning(f'parameters.mcmc.information_gain: not computed ({err!r}); mcmc.h5 is written without the '
                       'information_gain_* entries')
        return
    results.update(entries)
    top = int(np.nanargmax(out['per_parameter'])) if np.any(np.isfinite(out['per_parameter'])) else 0
    logger.info(f"Information gain of the {label}: joint {out['joint']:.3f} nats ({out['joint'] / np.log(2.0):.3f} bits) "
                f"over {out['n_points']} rows, k = {out['k']}; most about parameter {top} "
                f"({out['per_parameter'][top]:.3f} nats)")
    if np.any(np.asarray(out['copies']) > 0.1 * out['n_points']):
        logger.warning(f"information gain: up to {int(np.max(out['copies']))} copies among {out['n_points']} rows: thin "
                       "the chain by its autocorrelation time for a reliable estimate")


def information_gain(config, closure_index=-1, discard=0, thin=1):
    """The ``information_gain_*`` entries (``gpemu.information.information_gain``) of the chain stored in mcmc.h5 (of
    closure chain ``closure_index``, if >= 0), steps ``[discard::thin]``, all walkers, with the configuration's box and
    ``information_gain_*`` settings."""
    cfg, chain = _stored_chain(config, closure_index, discard, thin)
    from gpemu import information as _info
    kw = _information_gain_kwargs(cfg)
    lower, upper = kw.pop('lower'), kw.pop('upper')
    return _information_gain_entries(_info.information_gain(
        np.ascontiguousarray(chain.reshape(-1, chain.shape[-1])), lower, upper, **kw))


def expected_information_gain_settings(mc):
    """``(on, scale, n_outer, n_inner)`` from the ``parameters.mcmc`` mapping: ``expected_information_gain`` (true or
    false, default off: the expected information gain of an independent repeat of every observable's measurement),
    ``eig_scale`` (the repeat's uncertainties as a multiple of the present ones, a number > 0, default 1.0),
    ``eig_n_outer`` (simulated outcomes, an integer in [1, 2^31), default 4096) and ``eig_n_inner`` (the most evenly
    spaced rows of the chain in the inner sample, an integer in [2, 2^31), default 16384).  DESIGN.md §4.38."""
    on = mc.get('expected_information_gain', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"parameters.mcmc.expected_information_gain must be true or false, got {on!r}")
    scale = mc.get('eig_scale', 1.0)
    if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"parameters.mcmc.eig_scale must be a finite number > 0, got {scale!r}")
    n_outer = mc.get('eig_n_outer', 4096)
    if not isinstance(n_outer, (int, np.integer)) or isinstance(n_outer, (bool, np.bool_)) or not 1 <= n_outer < 2 ** 31:
        raise ValueError(f"parameters.mcmc.eig_n_outer must be an integer in [1, 2^31), got {n_outer!r}")
    n_inner = mc.get('eig_n_inner', 16384)
    if not isinstance(n_inner, (int, np.integer)) or isinstance(n_inner, (bool, np.bool_)) or not 2 <= n_inner < 2 ** 31:
        raise ValueError(f"parameters.mcmc.eig_n_inner must be an integer in [2, 2^31), got {n_inner!r}")
    return bool(on), float(scale), int(n_outer), int(n_inner)


EIG_KEYS = ('labels', 'nats', 'se', 'ess_mean', 'saturated')


def _eig_kwargs(config, scale=None, observables=None):
    """The arguments of ``DeviceSampler.expected_information_gain`` /
    ``gpemu.experiment.chain_expected_information_gain`` from the configuration and the pool's state: the candidates
    (``log_posterior.measurement_candidates``) and the ``eig_*`` settings."""
    scale = config.eig_scale if scale is None else scale
    return dict(candidates=log_posterior.measurement_candidates(scale=scale, observables=observables),
                n_outer=config.eig_n_outer, n_inner=config.eig_n_inner)


def _eig_entries(out):
    """the ``eig_*`` entries of mcmc.h5 from a ranking, in the order of the candidates"""
    return {'eig_labels': np.array(out['labels']), 'eig_nats': np.asarray(out['eig_nats'], dtype=np.float64),
            'eig_se': np.asarray(out['se'], dtype=np.float64), 'eig_ess_mean': np.asarray(out['ess_mean'], dtype=np.float64),
            'eig_saturated': np.asarray(out['saturated'], dtype=np.int64)}


def _add_expected_information_gain(config, results, compute, label='production chain'):
    """With ``parameters.mcmc.expected_information_gain``: the ``eig_*`` entries of ``compute(**kwargs)`` (a sampler's
    ``expected_information_gain`` on the chain where it lies) into the results that go to mcmc.h5, one log line, and a
    warning where an estimate is at its cap."""
    if not getattr(config, 'expected_information_gain', False):
        return
    try:
        out = compute(**_eig_kwargs(config))
        entries = _eig_entries(out)
    except Exception as err:         # the chain is worth more than the table: it is written either way
        logger.warning(f'parameters.mcmc.expected_information_gain: not computed ({err!r}); mcmc.h5 is written without '
                       'the eig_* entries')
        return
    results.update(entries)
    best = out['table'][0]
    logger.info(f"Expected information gain of a repeat at {config.eig_scale:g} x the present uncertainties, {label}: most "
                f"from {best['label']!r} ({best['eig_nats']:.3f} +- {best['se']:.3f} nats) among {len(out['labels'])} "
                f"observables; {best['n_outer']} outcomes against {best['n_inner']} rows")
    if np.any(out['saturated']):
        bad = [str(n) for n, w in zip(out['labels'], out['saturated']) if w]
        logger.warning(f"expected information gain at its cap (log n_inner - 3, or fewer than 16 effective rows) for {bad}: "
                       "lower bounds at best; raise parameters.mcmc.eig_n_inner")


def expected_information_gain(config, closure_index=-1, discard=0, thin=1, scale=None, observables=None):
    """The ``eig_*`` entries (``gpemu.experiment``) of the chain stored in mcmc.h5 (of closure chain
    ``closure_index``, if >= 0), steps ``[discard::thin]``, all walkers: for every observable label (or every entry of
    ``observables``: a label, or a list of labels measured together) the expected information gain of an independent
    repeat of that measurement with ``scale`` (default: ``parameters.mcmc.eig_scale``) times its present
    uncertainties, a dense covariance block where the data has one, the emulators' mean covariance added."""
    cfg, chain = _stored_chain(config, closure_index, discard, thin)
    box = cfg.analysis_config['parameterization'][cfg.parameterization]
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=cfg.analysis_name, parameterization=cfg.parameterization,
        analysis_config=cfg.analysis_config, config_file=cfg.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    data = _data_IO().data_array_from_h5(cfg.output_dir, 'observables.h5', pseudodata_index=-1,
                                         observable_filter=emu_cfg.observable_filter)
    log_posterior.initialize_pool_variables(box['min'], box['max'], emu_cfg, emu_results,
                                            _with_data_covariance(cfg, data), truncation_cov)
    from gpemu import experiment as _exp
    from gpemu.information import selected_rows
    kw = _eig_kwargs(cfg, scale=scale, observables=observables)
    rows = np.ascontiguousarray(chain.reshape(-1, chain.shape[-1]))
    rows = np.ascontiguousarray(rows[selected_rows(rows.shape[0], kw.pop('n_inner'))])
    return _eig_entries(_exp.chain_expected_information_gain(log_posterior.device_models(n_div=1.0), rows, **kw))


def propose_design_points(config, closure_index=-1, discard=0, thin=None, n_points=8, n_reference=4096,
                          n_candidates=2048, candidates=None, seed=0, feature_weights=None, **design_kwargs):
    """``emulation.propose_design_points`` with the chain stored in mcmc.h5 (of closure chain ``closure_index``, if
    >= 0) as the reference set: steps ``[discard::thin]``, all walkers; ``thin=None``: the smallest thinning that keeps
    at most ``n_reference`` rows.  ``feature_weights`` defaults to ``1 / y_err^2`` of the run's data (the closure
    chain's stored pseudo-data), so that emulator variance counts in units of the data's."""
    thin_read = 1 if thin is None else int(thin)
    cfg, chain = _stored_chain(config, closure_index, discard, thin_read)
    if thin is None:
        rows = chain.shape[0] * chain.shape[1]
        chain = chain[::max(1, -(-rows // max(1, int(n_reference))))]
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=cfg.analysis_name, parameterization=cfg.parameterization,
        analysis_config=cfg.analysis_config, config_file=cfg.config_file)
    if feature_weights is None:
        io = _data_IO()
        if closure_index >= 0:
            data = io.read_dict_from_h5(cfg.mcmc_output_dir, 'mcmc.h5')['experimental_pseudodata']
        else:
            data = io.data_array_from_h5(cfg.output_dir, 'observables.h5', pseudodata_index=-1,
                                         observable_filter=emu_cfg.observable_filter)
        feature_weights = design_feature_weights(data['y_err'])
    return emulation.propose_design_points(
        emu_cfg, n_points, reference=np.ascontiguousarray(chain.reshape(-1, chain.shape[-1])), candidates=candidates,
        n_candidates=n_candidates, seed=seed, feature_weights=feature_weights,
        emulation_group_results=emu_cfg.read_all_emulator_groups(), **design_kwargs)


def design_feature_weights(y_err):
    """``1 / y_err^2`` per feature; a feature without a positive, finite uncertainty gets weight 0."""
    y_err = np.asarray(y_err, dtype=np.float64).reshape(-1)
    ok = np.isfinite(y_err) & (y_err > 0)
    return np.where(ok, 1.0 / np.where(ok, y_err, 1.0) ** 2, 0.0)


POSTERIOR_PREDICTIVE_KEYS = ('mean', 'variance_parameters', 'variance_emulator', 'quantiles', 'probabilities')


def _add_posterior_predictive(config, results, emu_cfg, emu_results, truncation_cov):
    """With ``parameters.mcmc.posterior_predictive``: ``posterior_predictive_<key>`` of the production chain into the
    results that go to mcmc.h5 (``variance`` is the sum of the two parts and is not stored)."""
    if not getattr(config, 'posterior_predictive', False):
        return
    chain = np.asarray(results['chain'], dtype=np.float64)
    logger.info(f'Posterior-predictive bands from {chain.shape[0] * chain.shape[1]} samples...')
    out = emulation.posterior_predictive(chain.reshape(-1, chain.shape[-1]), emu_cfg, emulation_group_results=emu_results,
                                         emulator_cov_unexplained=truncation_cov,
                                         probabilities=config.posterior_predictive_probabilities)
    for key in POSTERIOR_PREDICTIVE_KEYS:
        results[f'posterior_predictive_{key}'] = out[key]


def posterior_predictive(config, closure_index=-1, discard=0, thin=1,
                         probabilities=emulation.POSTERIOR_PREDICTIVE_PROBABILITIES):
    """``emulation.posterior_predictive`` of the chain stored in mcmc.h5 (of closure chain ``closure_index``, if >= 0),
    steps ``[discard::thin]``, all walkers."""
    config, chain = _stored_chain(config, closure_index, discard, thin)
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=config.analysis_name, parameterization=config.parameterization,
        analysis_config=config.analysis_config, config_file=config.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    return emulation.posterior_predictive(chain.reshape(-1, chain.shape[-1]), emu_cfg, emulation_group_results=emu_results,
                                          emulator_cov_unexplained=truncation_cov, probabilities=probabilities)


def credible_interval(samples, confidence=0.9, interval_type='quantile'):
    """(low, high) of a 1-D sample array (ref: mcmc.py:137-164).

    'quantile': equal tails.  'hpd': the narrowest interval holding ``confidence`` of the samples, searched
    over the windows that drop i points at the bottom and ``n_out - i`` at the top.
    """
    x = np.asarray(samples)
    if interval_type == 'quantile':
        tail = 0.5 * (1.0 - confidence)
        return np.quantile(x, [tail, 1.0 - tail])
    if interval_type == 'hpd':
        n_out = int((1 - confidence) * x.size)           # points left outside the interval
        ordered = np.sort(x)
        bottoms, tops = ordered[:n_out], ordered[x.size - n_out:]
        narrowest = int(np.argmin(tops - bottoms))
        return bottoms[narrowest], tops[narrowest]
    raise ValueError(f"unknown interval_type {interval_type!r}")


def map_parameters(posterior, method='quantile'):
    """Point estimate per parameter: the mean of the samples inside the central 1 % quantile band of that
    parameter's marginal (ref: mcmc.py:167-184).  ``posterior``: (n_samples, n_parameters)."""
    if method != 'quantile':
        raise ValueError(f"unknown method {method!r}")
    half_band = 0.005
    estimate = np.empty(posterior.shape[1])
    for j, column in enumerate(np.asarray(posterior).T):
        q_lo, q_hi = np.quantile(column, [0.5 - half_band, 0.5 + half_band])
        estimate[j] = column[(column >= q_lo) & (column <= q_hi)].mean()
    return estimate


def find_map_unsupported(emulation_config, emulation_results):
    """Why ``log_posterior_and_gradient`` would decline the state ``initialize_pool_variables`` has just set, or None:
    fully correlated sources in the data, or a group whose kernel has no derivative path (Matern nu other than 1.5,
    2.5, inf).  Decided on the host, from the data and the emulators' kernels."""
    if log_posterior.data_covariance()[1] is not None:
        return "the data carry fully correlated sources (sys_sources), which have no gradient path"
    for name, cfg in emulation_config.emulation_groups_config.items():
        kernel = emulation_results[name]['emulators'][0].kernel_
        nu = float(getattr(kernel, 'nu', np.inf))
        if int(kernel.kind) == 1 and not (np.isinf(nu) or nu in (1.5, 2.5)):
            return f"emulation group {name!r} has a Matern kernel of nu = {nu:g}; gradients need nu = 1.5, 2.5 or inf (RBF)"
    return None


def _warn_find_map_not_read(config, what):
    """``parameters.mcmc.find_map`` is read by the untempered, unstacked ``run_mcmc`` only: say so where it is set and
    another path runs (``find_map(config, closure_index)`` afterwards gives the same from the written mcmc.h5)."""
    if getattr(config, 'find_map', False):
        logger.warning(f'parameters.mcmc.find_map is not read by {what}: mcmc.h5 will hold no map_* entries; call '
                       'mcmc.find_map(config, closure_index) on the written chain instead')


def find_map_on_pool(lower, upper, n_starts=32, starts=None, chain=None, log_prob=None, hessian=True):
    """The maximum of the log-posterior on the state ``log_posterior.initialize_pool_variables`` set.
    Starts: ``starts`` (n, d) if given; else the positions of the ``n_starts`` highest distinct log-probabilities of a
    stored ``chain`` (steps, walkers, d) / ``log_prob`` (steps, walkers); else uniform draws in the box (numpy's global
    state).  All starts advance in lock step (``gpemu.mapfit``), one batched device evaluation of value and analytic
    gradient per round.  Returns ``gpemu.mapfit.find_map``'s dict."""
    from gpemu import mapfit
    lower = np.asarray(lower, dtype=np.float64)
    upper = np.asarray(upper, dtype=np.float64)
    if starts is None:
        if chain is not None and log_prob is not None:
            starts = mapfit.best_distinct(chain, log_prob, n_starts)
        else:
            starts = np.random.uniform(lower, upper, (int(n_starts), lower.size))
    return mapfit.find_map(log_posterior.log_posterior_and_gradient, starts, lower, upper, hessian=hessian)


def find_map(config, closure_index=-1, n_starts=32, starts=None):
    """The MAP point of the analysis of ``config`` (or of the closure test ``closure_index``): a maximum of the
    log-posterior by L-BFGS-B on the device's analytic gradient, where ``map_parameters`` gives a per-coordinate
    marginal median.  The starts come from ``mcmc.h5`` of the run if it exists (the ``n_starts`` best distinct points of
    its chain), else they are uniform in the box.  Returns a dict with ``map_parameters`` (d,), ``map_log_prob``,
    ``all_parameters`` (n_starts, d), ``all_log_prob``, ``status``, ``nfev`` (per start) and ``hessian`` (d, d), the
    second derivatives of the log-posterior from central differences of the gradient with the step
    ``h_i = 1e-4 (max_i - min_i)``: at the maximum, except that a coordinate closer than ``2 h_i`` to a face of the box
    has its pair of points centred ``2 h_i`` inside that face, so that column is the derivative at that shifted point
    (``gpemu.mapfit.central_hessian``).  A maximum ON a face has no two-sided second derivative there."""
    box = config.analysis_config['parameterization'][config.parameterization]
    lower, upper = box['min'], box['max']
    emu_cfg = emulation.EmulationConfig.from_config_file(
        analysis_name=config.analysis_name, parameterization=config.parameterization,
        analysis_config=config.analysis_config, config_file=config.config_file)
    emu_results = emu_cfg.read_all_emulator_groups()
    truncation_cov = emulation.compute_emulator_cov_unexplained(emu_cfg, emu_results)
    io = _data_IO()
    chain = log_prob = None
    stored = None
    if os.path.exists(config.mcmc_outputfile):
        stored = io.read_dict_from_h5(config.mcmc_output_dir, 'mcmc.h5')
        chain, log_prob = stored.get('chain'), stored.get('log_prob')
    if closure_index >= 0 and stored is not None and 'experimental_pseudodata' in stored:
        data = stored['experimental_pseudodata']           # the draw the chain was conditioned on
    else:
        data = io.data_array_from_h5(config.output_dir, 'observables.h5', pseudodata_index=closure_index,
                                     observable_filter=emu_cfg.observable_filter)
    data = _with_data_covariance(config, data)
    log_posterior.initialize_pool_variables(lower, upper, emu_cfg, emu_results, data, truncation_cov)
    return find_map_on_pool(lower, upper, n_starts=n_starts, starts=starts, chain=chain, log_prob=log_prob)


####################################################################################################
class LoggingEnsembleSampler(EnsembleSampler):
    """Ensemble sampler that reports the acceptance fraction every ``n_logging_steps`` steps
    (ref: mcmc.py:187-204)."""

    def run_mcmc(self, X0, n_sampling_steps, n_logging_steps=100, **kwargs):
        logger.info(f'  running {self.nwalkers} walkers for {n_sampling_steps} steps')
        state, done = None, 0
        # advance in blocks that end on the logging steps, so that the device runs ahead of the host
        while done < n_sampling_steps:
            block = min(n_logging_steps - done % n_logging_steps, n_sampling_steps - done)
            # (the ensemble itself is only wanted at the end: the shipped settings log every 10 steps, and two blocking
            # downloads per block were a tenth of a 50 000-step run)
            state = self.advance(X0 if done == 0 else None, block, want_state=done + block >= n_sampling_steps, **kwargs)
            done += block
            if done % n_logging_steps == 0 or done == n_sampling_steps:
                frac = self.acceptance_fraction
                logger.info(f'  step {done}: acceptance fraction: mean {frac.mean()}, std {frac.std()}, '
                            f'min {frac.min()}, max {frac.max()}')
        return state


####################################################################################################
class MCMCConfig:
    """Settings of one MCMC run, read from the analysis YAML (ref: mcmc.py:207-245; same attribute names)."""

    def __init__(self, analysis_name='', parameterization='', analysis_config='', config_file='',
                 closure_index=-1, **kwargs):
        self.set_attribute(**kwargs)
        self.analysis_name, self.parameterization = analysis_name, parameterization
        self.analysis_config, self.config_file = analysis_config, config_file

        with open(config_file, 'r') as handle:
            top = yaml.safe_load(handle)
        for key in ('observable_table_dir', 'observable_config_dir', 'observables_filename'):
            setattr(self, key, top[key])
        for key in _MCMC_KEYS:
            setattr(self, key, analysis_config['parameters']['mcmc'][key])
        # parallel tempering (optional keys; absent or n_temperatures = 1: the untempered sampler)
        mc = analysis_config['parameters']['mcmc']
        self.n_temperatures = int(mc.get('n_temperatures', 1) or 1)
        self.t_max = float(mc.get('t_max', 1e5))
        self.swap_every = int(mc.get('swap_every', 1))
        self.prior_rung = bool(mc.get('prior_rung', True))
        # the sampler (optional): "stretch" (default, the reference's) or "hmc" with its three optional settings
        self.sampler = str(mc.get('sampler', 'stretch') or 'stretch').lower()
        if self.sampler not in ('stretch', 'hmc'):
            raise ValueError(f"parameters.mcmc.sampler must be 'stretch' or 'hmc', got {mc.get('sampler')!r}")
        self.hmc_n_leapfrog = int(mc.get('hmc_n_leapfrog', 8))
        self.hmc_target_accept = float(mc.get('hmc_target_accept', 0.8))
        self.hmc_step_size = float(mc.get('hmc_step_size', 0.1))
        if self.sampler == 'hmc' and not (self.hmc_n_leapfrog >= 1 and 0.0 < self.hmc_target_accept < 1.0
                                          and self.hmc_step_size > 0.0):
            raise ValueError("parameters.mcmc: hmc_n_leapfrog must be >= 1, hmc_target_accept in (0, 1) and hmc_step_size > 0")
        # correlated experimental uncertainties (optional): an .npz of 'cov' and / or 'sys_sources', a relative path
        # taken from the directory of the configuration file
        dc = mc.get('data_covariance')
        if dc and not os.path.isabs(str(dc)):
            dc = os.path.join(os.path.dirname(os.path.abspath(config_file)), str(dc))
        self.data_covariance = str(dc) if dc else None
        # the MAP point after production (optional, default off): map_parameters, map_log_prob, map_hessian in mcmc.h5
        self.find_map = bool(mc.get('find_map', False))
        # per-bin posterior-predictive bands from the whole production chain (optional, default off): five more
        # entries in mcmc.h5, none without the key
        self.posterior_predictive, self.posterior_predictive_probabilities = posterior_predictive_settings(mc)
        # convergence diagnostics of the production chain (optional, default off): rhat, ess_bulk, ess_tail, ess_mean and
        # mcse_mean in mcmc.h5, none without the key
        self.diagnostics = diagnostics_settings(mc)
        # the data of a corner plot from the whole production chain (optional, default off): marginal_* in mcmc.h5,
        # none without the key
        self.marginals, self.marginals_bins, self.marginals_confidence, self.marginals_kde = marginals_settings(
            mc, getattr(self, 'confidence', None))
        # ... and the 2-D kernel densities of all parameter pairs beside them (optional, default off): marginal_kde2d_*
        self.marginals_kde2d, self.marginals_kde2d_grid, self.marginals_kde2d_covariance = marginals_kde2d_settings(mc)
        # per-observable PSIS-LOO / WAIC and the observable-influence table of the production chain (optional, default
        # off): loo_* in mcmc.h5, none without the key
        self.loo, self.loo_leave_out = loo_settings(mc)
        # the posterior under other priors, from the production chain (optional, default none): reweight_* in mcmc.h5,
        # none without the key
        self.reweight = reweight_settings(mc)
        self.reweight_summaries = reweight_summaries_settings(mc)
        # how many nats the data taught about each parameter, each pair and all of them jointly (optional, default off):
        # information_gain_* in mcmc.h5, none without the key
        self.information_gain, self.information_gain_k, self.information_gain_max_points = information_gain_settings(mc)
        # which measurement would constrain the parameters most: the expected information gain of an independent repeat
        # of every observable (optional, default off): eig_* in mcmc.h5, none without the key
        self.expected_information_gain, self.eig_scale, self.eig_n_outer, self.eig_n_inner = \
            expected_information_gain_settings(mc)

        # <output_dir>/<analysis>_<parameterization>[/closure/results/<index>]/{mcmc.h5, mcmc_sampler.pkl}
        self.output_dir = os.path.join(top['output_dir'], f'{analysis_name}_{parameterization}')
        self.emulation_outputfile = os.path.join(self.output_dir, 'emulation.pkl')
        self.mcmc_output_dir = self.output_dir if closure_index < 0 else \
            os.path.join(self.output_dir, f'closure/results/{closure_index}')
        self.mcmc_outputfilename = 'mcmc.h5'
        self.mcmc_outputfile = os.path.join(self.mcmc_output_dir, self.mcmc_outputfilename)
        self.sampler_outputfile = os.path.join(self.mcmc_output_dir, 'mcmc_sampler.pkl')

        # parameter names are used as (raw) plot labels downstream
        par = self.analysis_config['parameterization'][self.parameterization]
        par['names'] = [str(name) for name in par['names']]

    def set_attribute(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self, key, value)
