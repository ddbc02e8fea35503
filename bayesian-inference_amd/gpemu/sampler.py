"""Stretch-move ensemble samplers.

``DeviceSampler``    the ensemble lives on one MI355X (libgpemu ``gpemu_sampler_*``); with
                     ``torch.distributed`` initialised the proposing half is sharded over the ranks
                     and the new log-probabilities are all-gathered (RCCL over xGMI) per half-step.
``HostEnsemble``     the same move for an arbitrary Python ``log_prob_fn`` (the emcee calling
                     convention the reference uses, ref: mcmc.py:83-85), vectorised over the
                     proposing half; also shardable over ranks (any torch.distributed backend).
``EnsembleSampler``  emcee-compatible facade (the subset the reference touches: ref: mcmc.py:83-116,
                     187-204, plot_mcmc.py) that picks the device path when ``log_prob_fn`` is bound
                     to device models.
"""
from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np

from . import _lib
from ._lib import as_f64, check, ptr
from .rows import DeviceRows


def shard_bounds(n, world, rank):
    """Contiguous block of ``ceil(n/world)`` proposals per rank: (lo, hi, per)."""
    per = (n + world - 1) // world
    lo = min(rank * per, n)
    hi = min(lo + per, n)
    return lo, hi, per


class AutocorrError(Exception):
    """Raised when the chain is too short for a reliable estimate (emcee.autocorr.AutocorrError)."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super().__init__(*args, **kwargs)


def _next_pow_two(n):
    i = 1
    while i < n:
        i = i << 1
    return i


def _rfft(a, n):
    """Real-input FFT along axis 0, on all host threads where scipy's pocketfft is there."""
    try:
        import scipy.fft
        return scipy.fft.rfft(a, n=n, axis=0, workers=-1)
    except Exception:
        return np.fft.rfft(a, n=n, axis=0)


def _irfft(a, n):
    try:
        import scipy.fft
        return scipy.fft.irfft(a, n=n, axis=0, workers=-1)
    except Exception:
        return np.fft.irfft(a, n=n, axis=0)


def function_1d(x):
    """Normalised autocorrelation function of a 1-D series via FFT (emcee.autocorr.function_1d)."""
    x = np.atleast_1d(x)
    n = _next_pow_two(len(x))
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[: len(x)].real
    acf /= acf[0]
    return acf


def _check_tolerance(tau_est, n_t, tol, quiet):
    """``tau_est``, unless the chain of ``n_t`` steps is shorter than ``tol`` times one of them: then emcee's
    AutocorrError, or with ``quiet`` its message as a warning (emcee.autocorr.integrated_time)."""
    flag = tol * tau_est > n_t
    if np.any(flag):
        msg = ("The chain is shorter than {0} times the integrated autocorrelation time for {1} "
               "parameter(s). Use this estimate with caution and run a longer chain!\n"
               ).format(tol, np.sum(flag))
        msg += "N/{0} = {1:.0f};\ntau: {2}".format(tol, n_t / tol, tau_est)
        if not quiet:
            raise AutocorrError(tau_est, msg)
        logging.getLogger(__name__).warning(msg)            # emcee logs the message when quiet (autocorr.py)
    return tau_est


def _check_run(rc):
    """The status of a call that ran the chain: 1 is a NaN log-probability, raised as emcee raises it."""
    if rc == 1:
        raise ValueError("Probability function returned NaN")
    check(rc)


def integrated_time(x, c=5, tol=50, quiet=False):
    """Integrated autocorrelation time per dimension with Sokal's window
    (emcee.autocorr.integrated_time; x has shape (steps, walkers, ndim))."""
    x = np.atleast_1d(x)
    if x.ndim == 1:
        x = x[:, np.newaxis, np.newaxis]
    if x.ndim == 2:
        x = x[:, :, np.newaxis]
    n_t, n_w, n_d = x.shape
    tau_est = np.empty(n_d)
    windows = np.empty(n_d, dtype=int)
    n2 = 2 * _next_pow_two(n_t)
    chunk = max(1, min(n_w, (64 << 20) // (16 * n2)))          # walkers per batched transform (~64 MB of complex128)
    for d in range(n_d):
        f = np.zeros(n_t)
        for k0 in range(0, n_w, chunk):
            # function_1d for a block of walkers in one batched real-input FFT over all host threads (emcee transforms
            # walker by walker with a complex FFT: the same numbers to rounding), added walker by walker in its order
            xc = x[:, k0:k0 + chunk, d]
            ft = _rfft(xc - np.mean(xc, axis=0), n2)
            acf = _irfft(ft * np.conjugate(ft), n2)[:n_t]
            acf /= acf[0]
            for k in range(acf.shape[1]):
                f += acf[:, k]
        f /= n_w
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(len(taus)) < c * taus
        windows[d] = np.argmin(m) if np.any(m) else len(taus) - 1
        tau_est[d] = taus[windows[d]]
    return _check_tolerance(tau_est, n_t, tol, quiet)


# ------------------------------------------------------------------------------------------------
class DeviceSampler:
    """Ensemble resident on the device; log-posterior = sum over the given DeviceModels."""

    def __init__(self, models, n_walkers, a=2.0, seed=0, seeds=None):
        """``seeds`` (a sequence): that many INDEPENDENT chains of ``n_walkers`` walkers each, stacked in one
        sampler and evaluated in the same launches (the closure tests of ref: steer_analysis.py:168-183); chain c is
        the chain ``DeviceSampler(models, n_walkers, a, seed=seeds[c])`` produces on data vector c of the models'
        ``likelihood_setup(y_exp (C, F), ...)``.  State and chain arrays then hold ``C * n_walkers`` walkers,
        chain after chain."""
        _lib.require_device()
        self.models = list(models)
        arr = (C.c_void_p * len(self.models))(*[m.handle for m in self.models])
        self._h, self.n_chains = self._create(arr, int(n_walkers), float(a), seed, seeds)
        self.walkers_per_chain = int(n_walkers)
        self.W, self.d = int(n_walkers) * self.n_chains, self.models[0].d
        # proposals of each half, chain after chain (the library's set sizes: ceil / floor of n_walkers / 2 per chain)
        self.ns = ((int(n_walkers) + 1) // 2 * self.n_chains, int(n_walkers) // 2 * self.n_chains)
        self.device = self.models[0].device
        self.last_transport = None       # what the last run_sharded call really took: "peer" / "rccl" / "torch" / "single" / "replicated"
        self.transport_info = {}         # self-test results, communicator sizes, fall-back reasons

    def _create(self, arr, n_walkers, a, seed, seeds):
        """The library handle and the number of stacked chains."""
        h = C.c_void_p()
        if seeds is None:
            check(_lib.lib().gpemu_sampler_create(C.byref(h), arr, len(self.models), n_walkers, a,
                                                  C.c_uint64(int(seed) & (2 ** 64 - 1))))
            return h, 1
        sd = np.array([int(v) & (2 ** 64 - 1) for v in seeds], dtype=np.uint64)
        check(_lib.lib().gpemu_sampler_create_chains(C.byref(h), arr, len(self.models), n_walkers, a,
                                                     ptr(sd), int(sd.size)))
        return h, int(sd.size)

    def close(self):
        for h in self.__dict__.pop("_comms", {}).values():
            if h is not None:
                _lib.lib().gpemu_comm_destroy(h)
        if getattr(self, "_h", None):
            _lib.lib().gpemu_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, X0, logp0=None):
        X0 = as_f64(X0, (self.W, self.d))
        lp = None if logp0 is None else as_f64(logp0, (self.W,))
        check(_lib.lib().gpemu_sampler_set_state(self._h, ptr(X0), ptr(lp)))

    def get_state(self):
        X = np.empty((self.W, self.d))
        lp = np.empty(self.W)
        check(_lib.lib().gpemu_sampler_get_state(self._h, ptr(X), ptr(lp)))
        return X, lp

    def reset(self):
        check(_lib.lib().gpemu_sampler_reset(self._h))

    def reserve(self, steps):
        """Grow the device chain buffer for ``steps`` more stored steps now (otherwise it grows on demand)."""
        check(_lib.lib().gpemu_sampler_reserve_chain(self._h, int(steps)))

    def run(self, steps, store=True):
        _check_run(_lib.lib().gpemu_sampler_run(self._h, int(steps), int(bool(store))))

    def step_host_rng(self, inds, zz, rint, logu, store=True):
        inds = np.ascontiguousarray(inds, dtype=np.int32)
        zz = as_f64(np.concatenate(zz), (self.W,))
        logu = as_f64(np.concatenate(logu), (self.W,))
        rint = np.ascontiguousarray(np.concatenate(rint), dtype=np.int64)
        _check_run(_lib.lib().gpemu_sampler_step_host_rng(self._h, ptr(inds), ptr(zz), ptr(rint), ptr(logu),
                                                          int(bool(store))))

    def counts(self):
        nacc = np.zeros(self.W, dtype=np.int64)
        it, cl = C.c_int64(), C.c_int64()
        check(_lib.lib().gpemu_sampler_get_counts(self._h, ptr(nacc), C.byref(it), C.byref(cl)))
        return nacc, int(it.value), int(cl.value)

    @property
    def live_counts(self):
        """``(live, proposals)``: of the ``proposals`` stretch proposals the compacted half-step has formed since the
        sampler was created, the ``live`` ones lay inside the prior box and were evaluated.  ``(0, 0)`` where the
        half-step does not compact (stacked or tempered chains, several groups, correlated sources, halves of at most
        128 proposals, ``GPEMU_NO_COMPACT=1``)."""
        out = np.zeros(2, dtype=np.int64)
        check(_lib.lib().gpemu_sampler_live_counts(self._h, ptr(out)))
        return int(out[0]), int(out[1])

    @property
    def live_fraction(self):
        """Share of the compacted half-steps' proposals that lay inside the prior box (``live_counts``); ``None`` where
        nothing was compacted."""
        live, n = self.live_counts
        return live / n if n else None

    def get_chain(self, first=0, n=None):
        _, _, cl = self.counts()
        n = cl - first if n is None else n
        chain = np.empty((n, self.W, self.d))
        lp = np.empty((n, self.W))
        check(_lib.lib().gpemu_sampler_get_chain(self._h, int(first), int(n), ptr(chain), ptr(lp)))
        return chain, lp

    # -- summaries of the stored chain, read where it lies ------------------------------------
    def _chain_walkers(self, chain):
        """(first walker, walkers) of the chain the summaries are taken over."""
        if self.n_chains == 1:
            if chain not in (None, 0):
                raise IndexError(f"chain index {chain} outside [0, 1)")
            return 0, self.W
        if chain is None:
            raise ValueError(f"this sampler stacks {self.n_chains} chains: pass chain=<index>")
        c = int(chain)
        if not 0 <= c < self.n_chains:
            raise IndexError(f"chain index {chain} outside [0, {self.n_chains})")
        return c * self.walkers_per_chain, self.walkers_per_chain

    def chain_ptr(self, first=0):
        """``(device address of step first of the chain [steps][W][d], steps from there on)``; valid until the next
        run, reserve, reset or restore."""
        p, n = C.c_void_p(), C.c_int64()
        check(_lib.lib().gpemu_sampler_chain_ptr(self._h, int(first), C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def _stored_view(self, discard, thin, chain, stream=None):
        """The stored chain ``get_chain()[discard::thin]`` of ``chain`` as ``DeviceRows``: from walker w0 of step discard
        on, a block is the chain's walkers of one kept step."""
        discard, thin = int(discard), int(thin)
        if thin < 1 or discard < 0:
            raise ValueError("discard must be >= 0 and thin >= 1")
        w0, nw = self._chain_walkers(chain)
        if discard >= self.counts()[2]:
            raise ValueError("no stored steps after discard")
        base, n = self.chain_ptr(discard)
        return DeviceRows(base + 8 * w0 * self.d, (n + thin - 1) // thin, nw, thin * self.W, stream, device=self.device, d=self.d)

    def _models(self, models):
        """``models`` (default: the sampler's groups) as a list, each on the sampler's parameters and device."""
        models = self.models if models is None else list(models)
        for m in models:
            if m.d != self.d or m.device != self.device:
                raise ValueError("model and sampler differ in parameters or device")
        return models

    def _baseline(self, discard, thin, rows):
        """``chain_moments`` for the view of every walker of every step from ``discard`` on, else None (uniform weights)."""
        whole = thin == 1 and rows.block_rows == self.W
        return (lambda: self.chain_moments(discard)) if whole else None

    def posterior_predictive(self, models=None, discard=0, thin=1, probabilities=(0.05, 0.5, 0.95), chain=None,
                             workspace_bytes=0):
        """``DeviceModel.posterior_predictive`` of the stored chain ``get_chain()[discard::thin]`` (all walkers of the
        chain, flattened step by step), read in place on the device: a list with one result dict per model of
        ``models`` (default: the sampler's groups).  Stacked samplers take ``chain=<index>``.  A sharded run stores
        the whole chain on every rank (every rank accepts identically), so each rank may call this on its own."""
        import torch
        from .model import QuantilePlan
        rows = self._stored_view(discard, thin, chain)
        plan = QuantilePlan(rows.rows, probabilities)
        models = self._models(models)
        dev = torch.device("cuda", self.device)
        out = []
        for m in models:
            bufs = torch.empty((3 + max(plan.ranks.size, 1), m.F), dtype=torch.float64, device=dev)
            order = bufs[3:].reshape(-1)          # [F][n_ranks] as the library writes it
            m.posterior_predictive_dev(*rows.layout, plan.ranks, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                       order.data_ptr() if plan.ranks.size else 0, workspace_bytes=workspace_bytes)
            h = bufs.cpu().numpy()
            out.append(plan.result(h[0].copy(), h[1].copy(), h[2].copy(),
                                   h[3:].reshape(-1)[:m.F * max(plan.ranks.size, 1)].reshape(m.F, -1).copy()))
        return out

    def parameter_quantiles(self, probabilities, discard=0, chain=None):
        """``np.quantile(get_chain()[discard:].reshape(-1, d), probabilities, axis=0)``: (nq, d), from exact order
        statistics selected on the device.  The whole ensemble is read in place (parameter j = the elements of stride
        d of the device chain); one chain of a stacked sampler is not a single stride, so its walkers are copied out
        first and selected from that copy."""
        from . import select
        rows = self._stored_view(discard, 1, chain)
        src, n, nw, S = rows.address, rows.n_blocks, rows.block_rows, rows.rows
        if nw != self.W:
            x = np.empty((n, nw, self.d))
            lp = np.empty((n, nw))
            w0 = self._chain_walkers(chain)[0]
            check(_lib.lib().gpemu_sampler_get_chain_walkers(self._h, int(discard), n, w0, nw, ptr(x), ptr(lp)))
            return select.quantile(x.reshape(-1, self.d), probabilities, axis=0, device=self.device)
        import torch
        ranks, ilo, ihi, t = select._bracket(S, probabilities)
        dout = torch.empty((self.d, ranks.size), dtype=torch.float64, device=torch.device("cuda", self.device))
        check(_lib.lib().gpemu_select_dev(self.device, self.d, S, C.c_void_p(src), 1, self.d, int(ranks.size), ptr(ranks),
                                          C.c_void_p(dout.data_ptr()), None))
        sel = dout.cpu().numpy()
        q = select.lerp(sel[:, ilo].T, sel[:, ihi].T, t[:, None])
        return q[0] if np.ndim(probabilities) == 0 else q

    def chain_moments(self, discard=0, n=None):
        """``(mean (d,), var (d,))`` of the stored steps ``[discard, discard + n)`` pooled over all walkers --
        ``x = get_chain()[discard:discard + n].reshape(-1, d)``, ``x.mean(0)``, ``x.var(0)`` -- computed on the device
        in two passes with sums in a fixed order; the chain stays where it is."""
        _, _, cl = self.counts()
        n = cl - int(discard) if n is None else int(n)
        mean, var = np.empty(self.d), np.empty(self.d)
        check(_lib.lib().gpemu_sampler_chain_moments(self._h, int(discard), n, ptr(mean), ptr(var)))
        return mean, var

    def diagnostics(self, discard=0, thin=1, chain=None):
        """Rank-normalised split-R-hat, bulk / tail ESS, the ESS of the mean and its Monte Carlo standard error
        (``gpemu.diagnostics.summary``) of the stored chain ``get_chain()[discard::thin]``, read in
        place on the device: a dict of ``(d,)`` arrays plus ``n_chains`` and ``n_draws``.  Every walker counts as a
        chain.  The walkers of a stretch ensemble are NOT independent chains -- each move uses the other half of the
        ensemble -- so R-hat here compares walkers with each other, and ``ess_*`` does not replace emcee's integrated
        autocorrelation time (``integrated_time``) for an ensemble; the chains of an ``HMCSampler`` are independent and
        the statistics mean what they mean in Stan.  Stacked samplers take ``chain=<index>``."""
        from .diagnostics import Diag
        _, n, nw, _ = self._stored_view(discard, thin, chain).layout
        with Diag.from_sampler(self._h, int(discard), n, int(thin), self._chain_walkers(chain)[0], nw, self.d) as h:
            return h.summary()

    def marginals(self, lower=None, upper=None, bins_1d=100, bins_2d=50, confidence=(0.9,), kde=True, n_grid=200,
                  discard=0, thin=1, chain=None, kde2d=False, n_grid_2d=100, covariance_2d="full"):
        """Marginal histograms, highest-density intervals and kernel densities (``gpemu.marginals.summary``; DESIGN.md
        §4.29) of the stored chain ``get_chain()[discard::thin].reshape(-1, d)``, taken where it lies: one dict with
        ``edges_1d``, ``edges_2d``, ``hist_1d``, ``pairs``, ``hist_2d``, ``n_inside``, ``confidence``, ``hpd (n_levels,
        d, 2)`` and, with ``kde``, ``kde_grid``, ``kde_density``, ``kde_bandwidth``.  The box defaults to the prior box
        of the sampler's models.  The histograms read the chain in place, thinned or stacked; the sort and the density
        read one parameter as one stride, so a view of several strided blocks (a thinned chain, one chain of a stacked
        sampler) is first copied to a dense device buffer.  With ``kde2d``: the 2-D kernel densities of all pairs
        (``gpemu.marginals.kde_2d``) on ``n_grid_2d`` points per axis, ``covariance_2d`` ``"full"`` or
        ``"diagonal"``, as ``kde2d_pairs``, ``kde2d_shear``, ``kde2d_bandwidth``, ``kde2d_grid_a``, ``kde2d_grid_b`` and
        ``kde2d_density``; they read the same view in place, thinned or stacked.  Stacked samplers take ``chain=<index>``."""
        from . import marginals as M
        rows = self._stored_view(discard, thin, chain)
        lower, upper = self._box_or_prior(self.models, lower, upper)
        return M.summary_view(rows, lower, upper, bins_1d, bins_2d, confidence, kde, n_grid, kde2d, n_grid_2d,
                              covariance_2d)

    def _data_chain(self, chain):
        """The data vector of the models' likelihood setup that ``chain`` of this sampler was run on."""
        return 0 if self.n_chains == 1 else int(chain)

    def loo(self, models=None, discard=0, thin=1, chain=None, leave_out=None, shifts=True, r_eff=None,
            workspace_bytes=0):
        """PSIS-LOO, WAIC and the observable-influence table (``gpemu.loo``) of the stored chain
        ``get_chain()[discard::thin]``, read in place on the device: ``gpemu.loo.summary`` of the per-observable
        log-likelihood terms of ``models`` (default: the sampler's groups), their rows concatenated in ``predict``'s
        observable order, plus ``labels`` ``"g<group>o<block>"``.  ``leave_out`` sums rows first (a class of observables
        left out together).  With ``shifts``: ``mean``, ``sd`` ``(d,)`` of the chain, ``loo_mean``, ``loo_sd`` ``(n_obs,
        d)`` under each row's leave-one-out weights and ``shift = (loo_mean - mean) / sd`` -- how far leaving an observable
        out moves each parameter, in posterior standard deviations.  Stacked samplers take ``chain=<index>`` (scored
        against that chain's own data vector)."""
        from . import loo as LO
        rows = self._stored_view(discard, thin, chain)
        models = self._models(models)
        T = LO.pointwise_dev(models, rows, self._data_chain(chain))
        return LO.from_terms(T, LO.default_labels(models), rows, leave_out, shifts, r_eff, workspace_bytes,
                             baseline=self._baseline(discard, thin, rows))

    def reweight(self, priors=None, models_new=None, discard=0, thin=1, chain=None, lower=None, upper=None,
                 posterior_predictive=False, models=None, **summary_kw):
        """The posterior under another prior or under other data, from the stored chain ``get_chain()[discard::thin]``
        read in place on the device (``gpemu.reweight.summary``): a list with one dict per scenario.
        ``priors``: a list of prior scenarios (``gpemu.reweight.check_priors``) inside the box, which defaults to the
        prior box of the sampler's models; ``models_new``: the sampler's emulators with another ``likelihood_setup`` (a
        data scenario: one row, or added to every prior scenario).  ``summary_kw``: ``probabilities``, ``bins_1d``,
        ``bins_2d``, ``smooth``, ``r_eff``, and ``hpd`` (confidence levels), ``kde`` for the weighted highest-density
        intervals and 1-D densities.  With ``posterior_predictive`` every scenario's dict gains
        ``posterior_predictive``: a list with one dict per model of ``models`` (default: the sampler's groups), the
        weighted bands of ``DeviceModel.posterior_predictive_weighted`` on the same view under the scenario's weights,
        at ``probabilities``.  The log-ratios, moments and histograms read the view as it lies, thinned or
        stacked; the quantiles read one parameter as one stride, so a view of several strided blocks is first copied to
        a dense device buffer, as ``marginals`` does.  Stacked samplers take ``chain=<index>``."""
        from . import reweight as RW
        if priors is None and models_new is None:
            raise ValueError("pass priors, models_new or both")
        rows = self._stored_view(discard, thin, chain)
        lower, upper = self._box_or_prior(self.models, lower, upper)
        L, log_norm = None, None
        if priors is not None:
            tables = RW.check_priors(priors, self.d, lower, upper)
            L = RW.log_prior_dev(self.device, *rows.layout, self.d, tables, np.asarray(lower, dtype=np.float64))
            if models_new is None:
                log_norm = RW.log_prior_norm(*tables, lower, upper)
        if models_new is not None:
            D = RW.data_log_ratio_dev(self.models, models_new, rows, self._data_chain(chain))
            L = D if L is None else L + D
        extra = None
        if posterior_predictive:
            pp_models = self._models(models)
            probs = summary_kw.get("probabilities", (0.05, 0.5, 0.95))
            extra = lambda q, Q: RW.bands_of_view(pp_models, rows, q, Q, probs, summary_kw.get("workspace_bytes", 0))
        return RW.summary_view(rows, L, lower, upper, log_norm=log_norm, baseline=self._baseline(discard, thin, rows),
                               extra=extra, **summary_kw)

    @staticmethod
    def _box_or_prior(models, lower, upper):
        """``(lower, upper)``, each defaulting to the prior box of ``models`` (``reweight.chain_reweight`` calls this too)."""
        if lower is None or upper is None:
            box = getattr(models[0], "prior_box", None)
            if box is None:
                raise ValueError("no prior box is known (likelihood_setup has not been called): pass lower and upper")
            lower, upper = (box[0] if lower is None else lower), (box[1] if upper is None else upper)
        return lower, upper

    def information_gain(self, lower=None, upper=None, k=4, discard=0, thin=1, chain=None, max_points=65536, subsets=None,
                         allow_copies=False, workspace_bytes=0):
        """How many nats the data taught about every parameter, every pair and all of them jointly
        (``gpemu.information.information_gain``): ``KL(posterior || prior)`` of the stored chain
        ``get_chain()[discard::thin].reshape(-1, d)`` under the uniform prior on the box (default: the prior box of the
        sampler's models), from at most ``max_points`` evenly spaced rows, read in place on the device, thinned or
        stacked.  An ensemble chain repeats states (a rejected move keeps the walker where it was): thin it by its
        autocorrelation time, or pass ``allow_copies``.  Stacked samplers take ``chain=<index>``."""
        from . import information as IG
        rows = self._stored_view(discard, thin, chain)
        lower, upper = self._box_or_prior(self.models, lower, upper)
        return IG.gain_of_view(rows, lower, upper, k=k, subsets=subsets, max_points=max_points,
                               allow_copies=allow_copies, workspace_bytes=workspace_bytes)

    def expected_information_gain(self, candidates, discard=0, thin=1, chain=None, n_inner=16384, n_outer=4096, seed=0,
                                  emulator_cov="mean", exclude_self=False, models=None, workspace_bytes=0):
        """Which measurement would constrain the parameters most, given this posterior
        (``gpemu.experiment.chain_expected_information_gain``): the expected information gain of every
        candidate (dicts with ``features``, ``y_err`` or ``cov`` and an optional ``label``), compared on common random
        numbers and sorted.  The inner sample is at most ``n_inner`` evenly spaced rows of the stored chain
        ``get_chain()[discard::thin].reshape(-1, d)``, gathered where the chain lies; the candidates' features index the
        features of ``models`` (default: the sampler's groups) concatenated in their order, the order
        ``emulation.predict`` returns.  Stacked samplers take ``chain=<index>``."""
        from . import experiment as EX, information as IG
        models = self._models(models)
        layout = self._stored_view(discard, thin, chain).layout
        rows, skipped = IG.unit_rows_dev(self.device, *layout, self.d, None, None, int(n_inner))
        if skipped:
            raise ValueError(f"{skipped} selected rows of the chain have a non-finite coordinate")
        return EX.chain_expected_information_gain(models, rows.cpu().numpy(), candidates, n_outer=n_outer, seed=seed,
                                                  emulator_cov=emulator_cov, exclude_self=exclude_self,
                                                  workspace_bytes=workspace_bytes)

    def kl_divergence(self, other, lower=None, upper=None, k=4, discard=0, thin=1, chain=None, max_points=65536,
                      subsets=None, allow_copies=False, other_chain=None, workspace_bytes=0):
        """``D(this chain || other)`` in nats (``gpemu.information.kl_divergence``) for every subset of
        the parameters, in the unit coordinates of the box (default: the prior box of this sampler's models).  ``other``:
        a sampler on the same device -- its stored chain ``[discard::thin]``, chain ``other_chain`` (default ``chain``) of
        a stacked one, read in place -- or rows ``(m, d)`` / ``(steps, walkers, d)`` as a host array or a device tensor."""
        from . import information as IG
        rows = self._stored_view(discard, thin, chain)
        lower, upper = self._box_or_prior(self.models, lower, upper)
        if isinstance(other, DeviceSampler):
            if other.d != self.d or other.device != self.device:
                raise ValueError("the two samplers differ in parameters or device")
            oc = other_chain if other_chain is not None else (chain if other.n_chains > 1 else None)
            other = other._stored_view(discard, thin, oc)
        return IG.divergence_of_views(rows, other, lower, upper, k=k, subsets=subsets, max_points=max_points,
                                      allow_copies=allow_copies, workspace_bytes=workspace_bytes)

    def propose_design(self, n_points, candidates=None, n_candidates=2048, n_reference=4096, discard=0, thin=None,
                       chain=None, seed=0, models=None, **kw):
        """Where to run the model next, given this posterior: ``gpemu.design.Design.select(n_points)`` (DESIGN.md
        §4.32) with the stored chain ``get_chain()[discard::thin]`` as the reference set, read in place on the device.
        ``thin=None``: the smallest thinning that keeps at most ``n_reference`` rows.  ``candidates=None``:
        ``gpemu.design.default_candidates`` -- ``n_candidates - n_candidates // 2`` Sobol' points of the models' prior
        box, then ``n_candidates // 2`` of the reference rows drawn with ``seed``.  Further keywords go to ``Design``
        (``feature_weights``, ``tau``, ``min_variance``, ``workspace_bytes``, ...).  The result of ``select`` plus
        ``candidates``, ``thin`` and ``n_reference_rows``.  Stacked samplers take ``chain=<index>``."""
        from . import design as DS
        models = self.models if models is None else list(models)
        w0, nw = self._chain_walkers(chain)
        if thin is None:
            steps = self.counts()[2] - int(discard)
            thin = max(1, -(-steps * nw // max(1, int(n_reference))))
        ref = self._stored_view(discard, thin, chain, _lib.current_stream(self.device))
        if candidates is None:
            box = getattr(models[0], "prior_box", None)
            if box is None:
                raise ValueError("no prior box is known (likelihood_setup has not been called): pass candidates")
            rows = self.get_chain(int(discard))[0][::int(thin), w0:w0 + nw].reshape(-1, self.d)
            candidates = DS.default_candidates(box[0], box[1], rows, n_candidates, seed=seed)
        kw.setdefault("max_picks", max(int(n_points), 1))
        with DS.Design(models, ref, candidates, **kw) as ds:
            out = ds.select(n_points)
            out["candidates"] = ds.candidates
        out["thin"], out["n_reference_rows"] = int(thin), ref.rows
        return out

    def acf_block(self, lag0, n_lags, first=0, n=None, w0=0, nw=None):
        """Walker-averaged normalised autocorrelation function, lags [lag0, lag0 + n_lags), of the chain stored on
        the device: (n_lags, d).  ``lag0`` a multiple of 16, the first block of an estimate at 0."""
        _, _, cl = self.counts()
        n = cl - first if n is None else n
        nw = self.W - w0 if nw is None else nw
        f = np.empty((int(n_lags), self.d))
        check(_lib.lib().gpemu_sampler_acf(self._h, int(first), int(n), int(w0), int(nw), int(lag0), int(n_lags), ptr(f)))
        return f

    def integrated_time(self, first=0, n=None, w0=0, nw=None, c=5, tol=50, quiet=False, block=256):
        """emcee.autocorr.integrated_time of the stored chain (rows [first, first + n), walkers [w0, w0 + nw)) WITHOUT
        bringing it to the host: the lag products are formed on the device, ``block`` lags at a time, until Sokal's
        window (the first M with M >= c tau(M)) has closed for every parameter -- a few hundred lags instead of FFTs over
        the whole chain.  Same estimate as ``gpemu.sampler.integrated_time`` (rounding apart)."""
        _, _, cl = self.counts()
        n_t = int(cl - first if n is None else n)
        d = self.d
        tau_est = np.full(d, np.nan)
        windows = np.full(d, -1, dtype=int)
        run = np.zeros(d)                    # cumulative sum of f so far
        lag0 = 0
        while lag0 < n_t and np.any(windows < 0):
            nl = int(min(block, n_t - lag0))
            f = self.acf_block(lag0, nl, first=first, n=n_t, w0=w0, nw=nw)
            cs = run[None, :] + np.cumsum(f, axis=0)
            taus = 2.0 * cs - 1.0
            if lag0 == 0:
                tau_first = taus[0].copy()
            idx = lag0 + np.arange(nl)
            for dd in range(d):
                if windows[dd] >= 0:
                    continue
                closed = ~(idx < c * taus[:, dd])           # NaN compares False: the window "closes" at once, as in emcee
                if np.any(closed):
                    m = int(np.argmax(closed))
                    windows[dd] = lag0 + m
                    tau_est[dd] = taus[m, dd]
                elif lag0 + nl >= n_t:
                    # never closed (idx < c tau at every lag): emcee's auto_window takes np.argmin of an all-True mask,
                    # i.e. window 0 and tau = taus[0] (which then fails the tol test: the short-chain AutocorrError).
                    # (A NaN series is the other case: its mask has no True entry, emcee returns len - 1 there and a
                    # NaN tau; here the window "closes" at lag 0 with the same NaN.)
                    windows[dd] = 0
                    tau_est[dd] = tau_first[dd]
            run = cs[-1]
            lag0 += nl
            block = min(block * 2, 4096)
        return _check_tolerance(tau_est, n_t, tol, quiet)

    # -- multi-GPU: one process per GPU, the ensemble replicated, proposals sharded -------------
    def _rccl_comm_agreed(self, group):
        """RCCL communicator owned by the library (one per sampler and process group), bootstrapped through
        torch.distributed -- or None on EVERY rank if any rank cannot provide it, so that all ranks take the same
        transport.  Every rank goes through the same sequence of collectives whatever fails locally:
          1. rank 0 makes the 128-byte id; it is broadcast together with a status byte (zeroed id + 0 on failure);
          2. every rank probes that it can load librccl; the ranks vote (all-reduce MIN) BEFORE anyone enters
             ncclCommInitRank, which would otherwise wait for the ranks that could not follow;
          3. the ranks join, run one all-gather of their indices through the new communicator, and vote again."""
        import warnings
        import torch
        import torch.distributed as dist
        key = id(group) if group is not None else 0
        comms = self.__dict__.setdefault("_comms", {})
        if key in comms:
            return comms[key]
        L = _lib.lib()
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        dev = torch.device("cuda", self.device)
        bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        path = bundled.encode() if os.path.exists(bundled) else None   # the copy torch already loaded
        err = None

        def vote(ok):
            t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
            return int(t.item()) == 1

        def give_up(reason):
            warnings.warn(f"library-owned RCCL communicator unavailable ({reason}); using torch.distributed's all-gather")
            self.transport_info["rccl_fallback_reason"] = str(reason)
            comms[key] = None
            return None

        # 1. the id, always broadcast
        ident = (C.c_char * 128)()
        status = 1
        if rank == 0:
            try:
                check(L.gpemu_comm_unique_id(path, C.cast(ident, C.c_void_p)))
            except Exception as e:
                err, status = e, 0
                ident = (C.c_char * 128)()
        t = torch.tensor(list(ident.raw) + [status], dtype=torch.uint8, device=dev)
        src = dist.get_global_rank(group, 0) if group is not None else 0
        dist.broadcast(t, src=src, group=group)
        raw = bytes(t.cpu().tolist())
        if raw[128] == 0:
            return give_up(repr(err) if err is not None else "rank 0 could not create the id")
        # 2. can this rank load the library?  (an id of its own, thrown away, exercises dlopen + the symbols)
        try:
            scratch = (C.c_char * 128)()
            check(L.gpemu_comm_unique_id(path, C.cast(scratch, C.c_void_p)))
            loadable = True
        except Exception as e:
            err, loadable = e, False
        if not vote(loadable):
            return give_up(repr(err) if err is not None else "another rank cannot load librccl")
        # 3. join, self-check, vote
        comm = None
        try:
            buf = C.create_string_buffer(raw[:128], 128)
            h = C.c_void_p()
            check(L.gpemu_comm_create(C.byref(h), int(self.device), int(rank), int(world), C.cast(buf, C.c_void_p), path))
            comm = h
            src_t = torch.full((1,), float(rank), dtype=torch.float64, device=dev)
            dst_t = torch.full((world,), -1.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            check(L.gpemu_comm_all_gather(comm, C.c_void_p(src_t.data_ptr()), C.c_void_p(dst_t.data_ptr()), 1, None))
            torch.cuda.synchronize(dev)
            if dst_t.cpu().tolist() != [float(r) for r in range(world)]:
                raise RuntimeError(f"RCCL all-gather self-check returned {dst_t.cpu().tolist()}")
            good = True
        except Exception as e:      # ncclCommInitRank failure, wrong data ...
            err, good = e, False
        if vote(good):
            comms[key] = comm
            r_seen, w_seen = C.c_int(-1), C.c_int(-1)
            L.gpemu_comm_dims(comm, C.byref(r_seen), C.byref(w_seen))
            self.transport_info["rccl_ranks_seen"] = int(w_seen.value)      # ncclCommCount of the new communicator
            return comm
        if comm is not None:
            L.gpemu_comm_destroy(comm)
        return give_up(repr(err) if err is not None else "another rank failed the self-check")

    def _peer_ready(self, group):
        """Exchange the ranks' gather-buffer IPC handles (once per sampler and group) so that every rank can
        store its log-probabilities straight into the others' memory.  True on every rank, or False on every
        rank (the ranks vote), e.g. when the model is outside the fused run's limits or IPC is unavailable."""
        import torch
        import torch.distributed as dist
        key = id(group) if group is not None else 0
        cache = self.__dict__.setdefault("_peer_ok", {})
        if key in cache:
            return cache[key]
        L = _lib.lib()
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        where = torch.device("cuda", self.device) if dist.get_backend(group) == "nccl" else torch.device("cpu")
        # ranks sharing this GPU (one-GPU rehearsals): the library then checks that all their launches fit on it
        # together; one rank per GPU -- the production layout -- needs no such rule
        import hashlib
        import socket
        bus = C.create_string_buffer(64)
        check(L.gpemu_device_bus_id(int(self.device), bus, 64))
        key16 = hashlib.sha256(socket.gethostname().encode() + b"/" + bus.value).digest()[:16]
        mykey = torch.tensor(list(key16), dtype=torch.uint8, device=where)
        keys = torch.zeros(16 * world, dtype=torch.uint8, device=where)
        dist.all_gather_into_tensor(keys, mykey, group=group)
        keys = bytes(keys.cpu().tolist())
        share = sum(1 for r in range(world) if keys[16 * r:16 * r + 16] == key16)
        check(L.gpemu_sampler_peer_share(self._h, int(share)))
        self.transport_info["ranks_on_this_device"] = int(share)
        mine = (C.c_char * 64)()
        ok = 1
        stage = "ok"
        if L.gpemu_sampler_peer_export(self._h, C.cast(mine, C.c_void_p)) != 0:
            ok, stage = 0, "export: " + _lib.last_error()
        t = torch.tensor(list(mine.raw), dtype=torch.uint8, device=where)
        everyone = torch.zeros(64 * world, dtype=torch.uint8, device=where)
        dist.all_gather_into_tensor(everyone, t, group=group)
        if ok:
            raw = bytes(everyone.cpu().tolist())
            buf = C.create_string_buffer(raw, 64 * world)
            if L.gpemu_sampler_peer_import(self._h, int(world), int(rank), C.cast(buf, C.c_void_p)) != 0:
                ok, stage = 0, "import: " + _lib.last_error()
        # the data path itself, before a chain depends on it: every rank stores a token into every rank's buffer and
        # waits (bounded) for all tokens in its own -- a mapping that opens but does not carry stores (or carries them
        # too late) makes the ranks fall back to the collective transports together instead of losing an exchange
        dist.barrier(group=group)
        if ok and L.gpemu_sampler_peer_selftest(self._h) != 0:
            ok, stage = 0, "selftest: " + _lib.last_error()
        # every rank's result, for the record (bench.py prints it), and the vote
        mine_ok = torch.tensor([ok], dtype=torch.int32, device=where)
        all_ok = torch.zeros(world, dtype=torch.int32, device=where)
        dist.all_gather_into_tensor(all_ok, mine_ok, group=group)
        per_rank = [int(v) for v in all_ok.cpu().tolist()]
        cache[key] = all(v == 1 for v in per_rank)
        self.transport_info.update(peer_selftest_per_rank=per_rank, peer_ranks_seen=sum(per_rank),
                                   peer_local_stage=stage, peer_vote=cache[key])
        return cache[key]

    def worth_sharding(self):
        """Is a half-step of this sampler large enough for walker sharding to pay?  Arithmetic of one half-step on one
        GPU, sum over the groups of k Npad^2 x proposals (the triangular GEMM), against GPEMU_SHARD_MIN_GFLOP
        (default 1.0).  Measured: C3 (5.4 GFLOP per half-step) 116 us on one GPU against 36 us for a rank's share of 8;
        the shipped three-group shape (0.27 GFLOP) 42 us on one GPU against 59 us through the fused half-step at ANY world
        size (profiles/r04_shipped_shape_step.txt) -- below about 1 GFLOP the step is launch latency, which sharding adds
        to."""
        gflop = sum(m.k * (-(-m.N // 128) * 128) ** 2 for m in self.models) * self.ns[0] / self.n_chains / 1e9
        return gflop >= float(os.environ.get("GPEMU_SHARD_MIN_GFLOP", "1.0"))

    def _run_peer_block(self, steps, store, vote):
        """One block of steps through the fused peer-store run with a way back: the chain state is snapshot on the
        device first; if the run fails with a LOST EXCHANGE on any rank (``vote(ok)``: every rank's outcome, all-reduced
        -- the ranks must take the same branch), every rank restores the snapshot and False is returned: the caller
        reruns the block over another transport.  True: the block is done.  A NaN log-probability is the model's, not
        the transport's: raised as emcee raises it."""
        L = _lib.lib()
        check(L.gpemu_sampler_snapshot(self._h))
        rc = L.gpemu_sampler_run_peer(self._h, int(steps), int(bool(store)))
        lost = rc == -4 and "timed out" in _lib.last_error()            # GPEMU_ERR_STATE from the bounded waits
        if rc != 0 and rc != 1 and not lost:
            vote(False)                                                  # (the peers must not wait for this rank's vote)
            check(rc)
        if vote(rc in (0, 1)):
            _check_run(rc)
            return True
        check(L.gpemu_sampler_restore(self._h))
        return False

    def run_emulated(self, steps, world, store=False):
        """Timing aid (bench.py's ``scaling_model``): rank 0's share of a ``world``-rank sharded run on this GPU through
        the fused two-launch half-step, without a process group or communicator (the entries of the other ranks' shares
        are pre-filled, so the exchange costs its local part only).  NOT a valid chain."""
        self.last_transport = "emulated"
        check(_lib.lib().gpemu_sampler_run_sharded(self._h, None, int(steps), int(bool(store)), int(world)))

    def run_sharded(self, steps, store=True, group=None, force=False, emulate_world=None, transport=None):
        """Same chain as ``run`` (every rank draws identical randomness); rank r evaluates its
        block of each half's proposals and the log-probabilities are exchanged.

        transport "peer" (default where it applies: up to 8 emulation groups of up to 64 PCs, launches that fit
        on the chip at once): a front launch + one triangular GEMM per group per half-step, every new
        log-probability stored straight into all ranks' memory (xGMI peer stores, no collective):
        ``gpemu_sampler_run_peer``.  transport "rccl" (backend "nccl"): the loop runs
        inside the library on its own RCCL communicator with one all-gather per half-step
        (``gpemu_sampler_run_sharded``).  transport "torch": per-phase calls with torch.distributed's all-gather
        (staged through the host on non-nccl backends).  GPEMU_SHARDED_TRANSPORT overrides the default.
        """
        import torch
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        if world == 1 and not force:
            self.last_transport = "single"
            return self.run(steps, store)
        L = _lib.lib()
        dev = torch.device("cuda", self.device)
        on_device = dist.get_backend(group) == "nccl"
        if transport is None and "GPEMU_SHARDED_TRANSPORT" not in os.environ and not emulate_world and not self.worth_sharding():
            # A small model: a half-step on ONE GPU is a handful of ~10 us launches (the reference's shipped shape:
            # 84 us per step), and the two-launch fused half-step every transport of a sharded run pays is slower than
            # that (119 us at the same shape, before any hop): sharding would be a regression.  Every rank holds the whole
            # ensemble and draws the same randomness, so each simply runs the chain itself -- the same chain, no exchange.
            self.last_transport = "replicated"
            self.transport_info["requested"] = "replicated (small model: below GPEMU_SHARD_MIN_GFLOP per half-step)"
            return self.run(steps, store)
        transport = transport or os.environ.get("GPEMU_SHARDED_TRANSPORT", "peer")
        self.transport_info["requested"] = transport
        if transport == "peer" and not emulate_world:
            if world > 1 and self._peer_ready(group):
                # the ranks enter every fused run together: all launches of the previous run (their gather-slot
                # hand-backs included) have completed everywhere before anyone stores into a peer's buffer again
                dist.barrier(group=group)
                self.last_transport = "peer"

                def vote(ok):
                    where = dev if on_device else torch.device("cpu")
                    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=where)
                    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
                    return int(t.item()) == 1
                if self._run_peer_block(int(steps), bool(store), vote):
                    return None
                # a peer's values did not arrive in time on some rank: every rank is back at the state before the block
                # (restored from the device snapshot) and the block is rerun over the collective transport; the peer
                # stores are not trusted again for this sampler
                self.__dict__.setdefault("_peer_ok", {})[id(group) if group is not None else 0] = False
                self.transport_info["peer_blocks_recovered"] = self.transport_info.get("peer_blocks_recovered", 0) + 1
                logging.getLogger(__name__).warning(
                    "sharded run: a peer exchange was lost; the block of %d steps is rerun over the collective transport "
                    "from the state before it (same random stream: the chain is that of an unbroken run)", int(steps))
            else:
                self.transport_info["fallback_from_peer"] = True
            transport = "rccl"
        elif transport == "peer":
            transport = "rccl"          # the emulation switch lives in gpemu_sampler_run_sharded
        if on_device and transport == "rccl":
            comm = self._rccl_comm_agreed(group)
            if comm is None:
                transport = "torch"
        if on_device and transport == "rccl":
            self.last_transport = "rccl"
            _check_run(L.gpemu_sampler_run_sharded(self._h, comm, int(steps), int(bool(store)), int(emulate_world or 0)))
            return None
        self.last_transport = "torch"
        # a dedicated (non-null) torch stream carries the library's launches AND the collectives, so
        # they are ordered by the stream; torch's default stream has handle 0, which the C ABI reads
        # as "use the handle's own stream"
        if getattr(self, "_tstream", None) is None:
            self._tstream = torch.cuda.Stream(device=dev)
        stream = self._tstream
        stream.wait_stream(torch.cuda.current_stream(dev))
        check(L.gpemu_sampler_set_stream(self._h, C.c_void_p(stream.cuda_stream)))
        if store:
            check(L.gpemu_sampler_reserve_chain(self._h, int(steps)))
        if emulate_world:   # measurement aid: do one rank's share of an `emulate_world`-GPU run (results are NOT a valid chain)
            bounds = [shard_bounds(self.ns[h], int(emulate_world), 0) for h in (0, 1)]
            bounds = [(lo, hi, self.ns[h]) for h, (lo, hi, _p) in enumerate(bounds)]
        else:
            bounds = [shard_bounds(self.ns[h], world, rank) for h in (0, 1)]
        with torch.cuda.stream(stream):
            # emulation: proposals nobody evaluates carry -inf, i.e. are rejected
            mine = [torch.full((b[2],), float("-inf") if emulate_world else 0.0, dtype=torch.float64, device=dev)
                    for b in bounds]
            full = [torch.zeros(b[2] * world, dtype=torch.float64, device=dev) for b in bounds]
        try:
          with torch.cuda.stream(stream):
            for _ in range(int(steps)):
                check(L.gpemu_sampler_begin_step(self._h))
                for h in (0, 1):
                    lo, hi, _per = bounds[h]
                    check(L.gpemu_sampler_half_propose_eval(self._h, h, lo, hi, C.c_void_p(mine[h].data_ptr())))
                    if on_device:
                        dist.all_gather_into_tensor(full[h], mine[h], group=group)
                    else:
                        host_mine = mine[h].cpu()
                        host_full = torch.empty(full[h].shape, dtype=torch.float64)
                        dist.all_gather_into_tensor(host_full, host_mine, group=group)
                        full[h].copy_(host_full)
                    check(L.gpemu_sampler_half_accept(self._h, h, C.c_void_p(full[h].data_ptr()), int(bool(store))))
                check(L.gpemu_sampler_end_step(self._h, int(bool(store))))
            _check_run(L.gpemu_sampler_check(self._h))
        finally:
            stream.synchronize()
            L.gpemu_sampler_set_stream(self._h, None)


# ------------------------------------------------------------------------------------------------
# Philox keys of the rungs of a TemperedSampler without explicit seeds: rung t uses seed + t * RUNG_KEY_STRIDE (mod 2^64),
# so rung 0 draws what DeviceSampler(models, n_walkers, seed=seed) draws
RUNG_KEY_STRIDE = 0x9E3779B97F4A7C15


class TemperedSampler(DeviceSampler):
    """Parallel-tempered stretch-move ensemble on one GPU (emcee 2's ``PTSampler`` with a stretch move
    per rung): ``len(betas)`` rungs of ``n_walkers`` walkers, stacked in one sampler on the models' single data vector.
    Rung t accepts with its log-likelihood difference scaled by ``betas[t]`` and, every ``swap_every`` steps (0: never),
    exchanges states with rung t - 1 column by column.  ``betas[0]`` must be 1 (rung 0 samples the posterior).
    Without ``seeds``, rung t's Philox key is ``seed + t * RUNG_KEY_STRIDE`` (mod 2^64).  State and chain arrays are
    shaped ``(T, n_walkers, ...)``; the stored log-probabilities are the untempered log-likelihoods."""

    def __init__(self, models, n_walkers, betas, a=2.0, seed=0, seeds=None, swap_every=1):
        betas = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        if seeds is None:
            seeds = [(int(seed) + t * RUNG_KEY_STRIDE) & (2 ** 64 - 1) for t in range(betas.size)]
        if len(seeds) != betas.size:
            raise ValueError(f"{len(seeds)} seeds for {betas.size} temperatures")
        self._betas_init, self.swap_every = betas, int(swap_every)
        super().__init__(models, n_walkers, a=a, seeds=seeds)
        self.n_temps, self.betas = self.n_chains, betas.copy()

    def _create(self, arr, n_walkers, a, seed, seeds):
        h = C.c_void_p()
        sd = np.array([int(v) & (2 ** 64 - 1) for v in seeds], dtype=np.uint64)
        b = self._betas_init
        check(_lib.lib().gpemu_sampler_create_tempered(C.byref(h), arr, len(self.models), n_walkers, a, ptr(sd), ptr(b),
                                                       int(b.size), self.swap_every))
        return h, int(b.size)

    def set_betas(self, betas):
        """A new ladder (same length; e.g. after a burn-in)."""
        b = as_f64(np.asarray(betas, dtype=np.float64).reshape(-1), (self.n_temps,))
        check(_lib.lib().gpemu_sampler_set_betas(self._h, ptr(b)))
        self.betas = b.copy()

    def set_state(self, X0, logp0=None):
        """``X0`` of shape ``(T * n_walkers, d)`` or ``(T, n_walkers, d)``."""
        X0 = np.asarray(X0, dtype=np.float64).reshape(self.W, self.d)
        super().set_state(X0, None if logp0 is None else np.asarray(logp0, dtype=np.float64).reshape(self.W))

    def get_state(self):
        """``(X (T, n_walkers, d), ll (T, n_walkers))``."""
        X, lp = super().get_state()
        return X.reshape(self.n_temps, -1, self.d), lp.reshape(self.n_temps, -1)

    def get_chain(self, temp=None, discard=0):
        """``(chain (steps, T, n_walkers, d), ll (steps, T, n_walkers))`` of the stored steps from ``discard`` on, or
        those of rung ``temp`` alone (``(steps, n_walkers, d)``, ``(steps, n_walkers)``)."""
        if temp is None:
            chain, lp = DeviceSampler.get_chain(self, first=int(discard))
            n, Wc = chain.shape[0], self.walkers_per_chain
            return chain.reshape(n, self.n_temps, Wc, self.d), lp.reshape(n, self.n_temps, Wc)
        t = int(temp)
        if not 0 <= t < self.n_temps:
            raise IndexError(f"temperature index {temp} outside [0, {self.n_temps})")
        # only this rung's walkers leave the device (a strided copy), not the whole ladder
        _, _, cl = self.counts()
        n, Wc = cl - int(discard), self.walkers_per_chain
        chain, lp = np.empty((n, Wc, self.d)), np.empty((n, Wc))
        check(_lib.lib().gpemu_sampler_get_chain_walkers(self._h, int(discard), int(n), t * Wc, Wc, ptr(chain), ptr(lp)))
        return chain, lp

    def _chain_walkers(self, chain):
        """The summaries of a tempered sampler are those of rung 0, the posterior (``chain`` = another rung)."""
        t = 0 if chain is None else int(chain)
        if not 0 <= t < self.n_temps:
            raise IndexError(f"temperature index {chain} outside [0, {self.n_temps})")
        return t * self.walkers_per_chain, self.walkers_per_chain

    def run_sharded(self, steps, store=True, group=None, force=False, emulate_world=None, transport=None):
        """Tempered runs are single-GPU (``run``); the library declines its sharded and peer runs, and the per-phase
        transport is declined here."""
        raise _lib.GpemuError(-5, "tempered samplers run on one GPU (TemperedSampler.run); sharded runs are not supported")

    @property
    def acceptance_fraction(self):
        """Stretch-move acceptance per rung and walker, ``(T, n_walkers)``."""
        nacc, it, _ = self.counts()
        return (nacc / float(max(it, 1))).reshape(self.n_temps, -1)

    def swap_counts(self):
        """(accepted, attempted) swaps since the last reset, ``(T - 1, n_walkers)`` each: row t is the pair (t, t+1)."""
        shape = (self.n_temps - 1, self.walkers_per_chain)
        acc, tried = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        check(_lib.lib().gpemu_sampler_get_swap_counts(self._h, ptr(acc), ptr(tried)))
        return acc, tried

    @property
    def tswap_acceptance_fraction(self):
        """Swap acceptance of each neighbouring rung pair, ``(T - 1,)`` (0 before any attempt)."""
        acc, tried = self.swap_counts()
        return acc.sum(axis=1) / np.maximum(tried.sum(axis=1), 1).astype(np.float64)

    def mean_log_likelihood(self, discard=0):
        """Mean stored log-likelihood of every rung over the steps from ``discard`` on, ``(T,)`` (on the device)."""
        _, _, cl = self.counts()
        n = cl - int(discard)
        if n < 1:
            raise ValueError(f"no stored steps after discarding {discard} of {cl}")
        out = np.empty(self.n_temps)
        check(_lib.lib().gpemu_sampler_mean_loglik(self._h, int(discard), int(n), ptr(out)))
        return out

    def log_evidence_estimate(self, discard=0):
        """``(logZ, dlogZ)`` by thermodynamic integration over the ladder (gpemu.tempering); Z is the evidence under
        the normalised uniform prior on the box."""
        from .tempering import thermodynamic_integration_log_evidence
        return thermodynamic_integration_log_evidence(self.betas, self.mean_log_likelihood(discard))

    def diagnostics(self, temp=0, discard=0, thin=1):
        """``DeviceSampler.diagnostics`` of one rung (default: rung 0, the posterior), its walkers as the chains.  They
        are the walkers of a stretch ensemble that also swaps states with its neighbours: not independent chains."""
        return DeviceSampler.diagnostics(self, discard=discard, thin=thin, chain=int(temp))

    def marginals(self, temp=0, **kw):
        """``DeviceSampler.marginals`` of one rung (default: rung 0, the posterior)."""
        return DeviceSampler.marginals(self, chain=int(temp), **kw)

    def _data_chain(self, chain):
        return 0   # the rungs share the models' single data vector

    def loo(self, temp=0, **kw):
        """``DeviceSampler.loo`` of one rung (default: rung 0, the posterior)."""
        return DeviceSampler.loo(self, chain=int(temp), **kw)

    def reweight(self, temp=0, **kw):
        """``DeviceSampler.reweight`` of one rung (default: rung 0, the posterior)."""
        return DeviceSampler.reweight(self, chain=int(temp), **kw)

    def information_gain(self, temp=0, **kw):
        """``DeviceSampler.information_gain`` of one rung (default: rung 0, the posterior)."""
        return DeviceSampler.information_gain(self, chain=int(temp), **kw)

    def expected_information_gain(self, candidates, temp=0, **kw):
        """``DeviceSampler.expected_information_gain`` of one rung (default: rung 0, the posterior)."""
        return DeviceSampler.expected_information_gain(self, candidates, chain=int(temp), **kw)

    def kl_divergence(self, other, temp=0, other_temp=0, **kw):
        """``DeviceSampler.kl_divergence`` of one rung (default: rung 0, the posterior) against ``other``: rung
        ``other_temp`` of another tempered sampler (or of this one: how far a hotter rung is from the posterior), the
        chain of an untempered sampler, or rows."""
        oc = int(other_temp) if isinstance(other, TemperedSampler) else None
        return DeviceSampler.kl_divergence(self, other, chain=int(temp), other_chain=oc, **kw)

    def propose_design(self, n_points, temp=0, **kw):
        """``DeviceSampler.propose_design`` of one rung (default: rung 0, the posterior)."""
        return DeviceSampler.propose_design(self, n_points, chain=int(temp), **kw)

    def integrated_time(self, temp=0, first=0, n=None, c=5, tol=50, quiet=False, block=256):
        """emcee's integrated autocorrelation time of rung ``temp``, estimated on the device."""
        Wc = self.walkers_per_chain
        return DeviceSampler.integrated_time(self, first=first, n=n, w0=int(temp) * Wc, nw=Wc, c=c, tol=tol,
                                             quiet=quiet, block=block)


# ------------------------------------------------------------------------------------------------
class HMCSampler(DeviceSampler):
    """``n_chains`` independent Hamiltonian Monte Carlo chains in lock step on one GPU, on the
    analytic gradient of the log-posterior (``DeviceModel.logpost_grad``'s path).  Chain w is walker w of the stored
    chain, so ``get_chain``, ``chain_ptr``, ``integrated_time``, ``posterior_predictive``, ``parameter_quantiles``,
    ``chain_moments`` and snapshot / restore work as on a ``DeviceSampler``.  Trajectories reflect at the faces of the
    prior box.  ``warmup`` adapts the step size (dual averaging, on the device) and the diagonal metric; ``run``
    then samples with both fixed.  Kernels the gradient declines (Matern 0.5, general nu), correlated systematic
    sources and several data vectors are declined at construction; sharded runs are not supported."""

    def __init__(self, models, n_chains, n_leapfrog=8, step_size=0.1, jitter=None, seed=0):
        from . import hmc as _hmc
        self.n_leapfrog = int(n_leapfrog)
        self._eps0 = float(step_size)
        self.jitter = _hmc.DEFAULT_JITTER if jitter is None else float(jitter)
        super().__init__(models, n_chains, seed=seed)
        self._prior_var = self.inverse_metric

    def _create(self, arr, n_walkers, a, seed, seeds):
        if seeds is not None:
            raise ValueError("an HMC sampler takes one seed: its chains are independent already")
        h = C.c_void_p()
        check(_lib.lib().gpemu_sampler_create_hmc(C.byref(h), arr, len(self.models), n_walkers, self.n_leapfrog, self._eps0,
                                                  self.jitter, C.c_uint64(int(seed) & (2 ** 64 - 1))))
        return h, 1

    @property
    def step_size(self):
        e = C.c_double()
        check(_lib.lib().gpemu_sampler_hmc_get_step_size(self._h, C.byref(e)))
        return float(e.value)

    @step_size.setter
    def step_size(self, eps):
        check(_lib.lib().gpemu_sampler_hmc_set_step_size(self._h, float(eps)))

    @property
    def inverse_metric(self):
        m = np.empty(self.d)
        check(_lib.lib().gpemu_sampler_hmc_get_metric(self._h, ptr(m)))
        return m

    @inverse_metric.setter
    def inverse_metric(self, minv):
        check(_lib.lib().gpemu_sampler_hmc_set_metric(self._h, ptr(as_f64(minv, (self.d,)))))

    def adapt(self, on, target_accept=None):
        """Switch the device's dual averaging of the step size on (restarting it at the current step size) or off
        (freezing the step size at the averaged one)."""
        from . import hmc as _hmc
        t = _hmc.DEFAULT_TARGET_ACCEPT if target_accept is None else float(target_accept)
        check(_lib.lib().gpemu_sampler_hmc_adapt(self._h, int(bool(on)), t))

    def stats(self):
        """dict: ``accepted``, ``divergences`` (per chain, since the last reset), ``mean_accept_prob`` (over the
        iterations since then) and ``last_accept_prob`` (of the last iteration)."""
        acc, div = np.zeros(self.W, dtype=np.int64), np.zeros(self.W, dtype=np.int64)
        mean, last = C.c_double(), C.c_double()
        check(_lib.lib().gpemu_sampler_hmc_stats(self._h, ptr(acc), ptr(div), C.byref(mean), C.byref(last)))
        return dict(accepted=acc, divergences=div, mean_accept_prob=float(mean.value), last_accept_prob=float(last.value))

    @property
    def divergences(self):
        return self.stats()["divergences"]

    @property
    def acceptance_fraction(self):
        nacc, it, _ = self.counts()
        return nacc / float(max(it, 1))

    def draws(self, step):
        """What iteration ``step`` of the device's random stream draws: ``(z (W, d), u_accept (W,), u_jitter (W,))``."""
        z, ua, uj = np.empty((self.W, self.d)), np.empty(self.W), np.empty(self.W)
        check(_lib.lib().gpemu_sampler_hmc_draws(self._h, C.c_uint64(int(step)), ptr(z), ptr(ua), ptr(uj)))
        return z, ua, uj

    def step_host_rng(self, p0, logu, eps_w, store=True):
        """One iteration with the caller's momenta ``p0 (W, d)``, log-uniforms and per-chain step sizes."""
        p0, logu, eps_w = as_f64(p0, (self.W, self.d)), as_f64(logu, (self.W,)), as_f64(eps_w, (self.W,))
        _check_run(_lib.lib().gpemu_sampler_hmc_step_host_rng(self._h, ptr(p0), ptr(logu), ptr(eps_w), int(bool(store))))

    def warmup(self, n_warmup, target_accept=None, adapt_metric=True):
        """``n_warmup`` iterations of the three-stage warm-up (``gpemu.hmc.warmup_schedule``) from the current state.
        The step size adapts on the device after every iteration; the host is heard only at the ends of the metric
        windows.  Afterwards step size and metric are fixed, and the warm-up's chain and counters are dropped
        (``reset``); returns dict ``step_size``, ``inverse_metric``, ``mean_accept_prob``, ``divergences`` (of the
        warm-up)."""
        from . import hmc as _hmc
        self.reset()
        self.adapt(True, target_accept)
        for n, set_metric in _hmc.warmup_schedule(n_warmup):
            set_metric = set_metric and adapt_metric
            _, _, before = self.counts()
            self.run(n, store=set_metric)
            if set_metric:
                _, var = self.chain_moments(discard=before, n=n)
                self.inverse_metric = _hmc.regularised_metric(var, n, self._prior_var)
                self.adapt(True, target_accept)          # the averaging restarts at the step size reached
        self.adapt(False)
        st = self.stats()
        out = dict(step_size=self.step_size, inverse_metric=self.inverse_metric, mean_accept_prob=st["mean_accept_prob"],
                   divergences=int(st["divergences"].sum()))
        self.reset()
        return out

    def run_sharded(self, steps, store=True, group=None, force=False, emulate_world=None, transport=None):
        raise _lib.GpemuError(-5, "HMC samplers run on one GPU (HMCSampler.run); sharded runs are not supported")


# ------------------------------------------------------------------------------------------------
class HostEnsemble:
    """Stretch move for an arbitrary vectorised ``log_prob_fn(X (n,d)) -> (n,)`` on the host.

    Randomness: numpy ``RandomState`` consumed in emcee's order (choice, shuffle, rand, randint,
    rand...).  With torch.distributed initialised (``sharded=True``) rank r evaluates its block of
    the proposals and the values are all-gathered; every rank keeps the whole ensemble.
    """

    def __init__(self, n_walkers, ndim, log_prob_fn, a=2.0, seed=None, sharded=False, group=None):
        if n_walkers < 2 * ndim:
            raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than twice "
                               "the number of dimensions.")
        self.W, self.d, self.fn, self.a = n_walkers, ndim, log_prob_fn, a
        self.random = np.random.RandomState(seed)
        self.sharded, self.group = sharded, group
        self.X = None
        self.lp = None
        self.reset()

    def reset(self):
        self.chain, self.lps = [], []
        self.naccepted = np.zeros(self.W, dtype=np.int64)
        self.iterations = 0

    def _eval(self, q):
        if not self.sharded:
            return np.asarray(self.fn(q), dtype=np.float64).reshape(-1)
        import torch
        import torch.distributed as dist
        world, rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        lo, hi, per = shard_bounds(q.shape[0], world, rank)
        mine = torch.zeros(per, dtype=torch.float64)
        if hi > lo:
            mine[: hi - lo] = torch.from_numpy(np.asarray(self.fn(q[lo:hi]), dtype=np.float64).reshape(-1))
        full = torch.zeros(per * world, dtype=torch.float64)
        dist.all_gather_into_tensor(full, mine, group=self.group)
        return full.numpy()[: q.shape[0]].copy()

    def set_state(self, X0, logp0=None):
        self.X = np.array(X0, dtype=np.float64)
        if self.X.shape != (self.W, self.d):
            raise ValueError("incompatible input dimensions")
        self.lp = self._eval(self.X) if logp0 is None else np.array(logp0, dtype=np.float64)
        if np.any(np.isnan(self.lp)):
            raise ValueError("The initial log_prob was NaN")

    def step(self, store=True):
        rs, W, a = self.random, self.W, self.a
        rs.choice(1, p=[1.0])
        inds = np.arange(W) % 2
        rs.shuffle(inds)
        for split in range(2):
            S1 = inds == split
            s, c = self.X[S1], self.X[~S1]
            ns, nc = s.shape[0], c.shape[0]
            zz = ((a - 1.0) * rs.rand(ns) + 1) ** 2.0 / a
            factors = (self.d - 1.0) * np.log(zz)
            rint = rs.randint(nc, size=(ns,))
            q = c[rint] - (c[rint] - s) * zz[:, None]
            new_lp = self._eval(q)
            if np.any(np.isnan(new_lp)):
                raise ValueError("Probability function returned NaN")
            with np.errstate(divide="ignore"):
                logu = np.log(np.array([rs.rand() for _ in range(ns)]))
            acc = factors + new_lp - self.lp[S1] > logu
            widx = np.flatnonzero(S1)[acc]
            self.X[widx] = q[acc]
            self.lp[widx] = new_lp[acc]
            self.naccepted[widx] += 1
        self.iterations += 1
        if store:
            self.chain.append(self.X.copy())
            self.lps.append(self.lp.copy())

    def run(self, steps, store=True):
        for _ in range(int(steps)):
            self.step(store)


# ------------------------------------------------------------------------------------------------
def walkers_independent(coords):
    """emcee's initial-state check: the walker cloud must span the space (condition number <= 1e8)."""
    if not np.all(np.isfinite(coords)):
        return False
    C = coords - np.mean(coords, axis=0)[None, :]
    C_colmax = np.amax(np.abs(C), axis=0)
    if np.any(C_colmax == 0):
        return False
    C = C / C_colmax
    C = C / np.sqrt(np.sum(C ** 2, axis=0))
    return np.linalg.cond(C.astype(float)) <= 1e8


class State:
    """Minimal emcee.State: ``coords``, ``log_prob``; unpacks / indexes like emcee's
    (``sampler.run_mcmc(...)[0]`` is the coordinate array, ref: mcmc.py:101)."""

    def __init__(self, coords, log_prob=None, blobs=None, random_state=None):
        self.coords = np.atleast_2d(np.asarray(coords, dtype=np.float64))
        self.log_prob = log_prob
        self.blobs = blobs
        self.random_state = random_state

    def __iter__(self):
        return iter((self.coords, self.log_prob, self.random_state))

    def __getitem__(self, i):
        return (self.coords, self.log_prob, self.random_state)[i]

    def __len__(self):
        return 3


class EnsembleSampler:
    """emcee.EnsembleSampler look-alike (the subset the reference uses: ref: mcmc.py:83-116, 187-204 and
    plot_mcmc.py): stretch move a = 2, red/blue split re-drawn every step.

    * ``log_prob_fn`` bound to device models (``bayesian_inference.log_posterior.log_posterior`` carries a
      ``_gpemu_device_models`` hook): the ensemble lives on the GPU (``DeviceSampler``); with
      torch.distributed initialised the proposals are sharded over the ranks.
    * any other callable: host stretch move (``HostEnsemble``), one call per walker like emcee
      (``vectorize=True`` passes the whole half-ensemble), ``pool.map`` if a pool is given.
    """

    def __init__(self, nwalkers, ndim, log_prob_fn, pool=None, a=2.0, seed=None, vectorize=False,
                 args=None, kwargs=None, sharded=None, **_ignored):
        self.nwalkers, self.ndim = int(nwalkers), int(ndim)
        self._sharded = sharded          # None: shard whenever torch.distributed has more than one rank
        self.log_prob_fn = log_prob_fn
        self.pool = pool
        self.a = float(a)
        self.vectorize = vectorize
        self._args, self._kwargs = tuple(args or ()), dict(kwargs or {})
        self._seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self._impl = None
        self._cache = None

    # -- backends -------------------------------------------------------------------------------
    @property
    def world_size(self):
        if self._sharded is False:       # an independent chain on this rank (replica parallelism)
            return 1
        from . import dist as gdist
        dist = gdist._dist()             # None in a single process that never imported torch (no ~1 s import)
        if dist is not None and dist.is_initialized():
            return dist.get_world_size()
        return 1

    def _call_rows(self, q):
        f = self.log_prob_fn
        if self.vectorize:
            return np.asarray(f(q, *self._args, **self._kwargs), dtype=np.float64).reshape(-1)
        mapper = self.pool.map if self.pool is not None else map
        vals = list(mapper(_RowCall(f, self._args, self._kwargs), list(q)))
        return np.array([float(np.asarray(v).reshape(-1)[0]) for v in vals])

    def _ensure(self):
        if self._impl is not None:
            return
        if self.world_size > 1:
            # a sharded chain needs the same random stream on every rank (the ranks only exchange
            # log-probabilities): rank 0's seed wins, whether it was given or drawn from numpy's global state
            from . import dist as gdist
            self._seed = gdist.rank0_int(self._seed)
        hook = getattr(self.log_prob_fn, "_gpemu_device_models", None)
        if hook is not None:
            self._impl = DeviceSampler(hook(), self.nwalkers, a=self.a, seed=self._seed)
            self._device = True
        else:
            self._impl = HostEnsemble(self.nwalkers, self.ndim, self._call_rows, a=self.a, seed=self._seed,
                                      sharded=self.world_size > 1)
            self._device = False

    # -- running ----------------------------------------------------------------------------------
    def advance(self, initial_state, nsteps, store=True, want_state=True):
        """Run ``nsteps`` steps (from ``initial_state`` if given, else from the current state).  ``want_state`` = False:
        the ensemble is not downloaded and None is returned (the blocks between two log lines of a long run)."""
        self._ensure()
        self._cache = None
        if initial_state is not None:
            X0 = initial_state.coords if isinstance(initial_state, State) else np.asarray(initial_state, dtype=np.float64)
            if X0.shape != (self.nwalkers, self.ndim):
                raise ValueError("incompatible input dimensions")
            if self.nwalkers < 2 * self.ndim:
                raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than twice the "
                                   "number of dimensions.")
            if not walkers_independent(X0):
                raise ValueError("Initial state has a large condition number. Make sure that your walkers are "
                                 "linearly independent for the best performance")
            self._impl.set_state(X0)
            lp0 = self._impl.get_state()[1] if self._device else self._impl.lp
            if np.any(np.isnan(lp0)):
                raise ValueError("The initial log_prob was NaN")
        if self._device and self.world_size > 1:
            self._impl.run_sharded(nsteps, store)
        else:
            self._impl.run(nsteps, store)
        if not want_state:
            return None
        if self._device:
            X, lp = self._impl.get_state()
        else:
            X, lp = self._impl.X.copy(), self._impl.lp.copy()
        return State(X, log_prob=lp)

    def run_mcmc(self, initial_state, nsteps, **kwargs):
        return self.advance(initial_state, nsteps, **kwargs)

    def sample(self, initial_state, iterations=1, store=True, **_ignored):
        """Generator over single steps (emcee's ``sample``)."""
        state = None
        for i in range(int(iterations)):
            state = self.advance(initial_state if i == 0 else None, 1, store=store)
            yield state

    def reset(self):
        self._cache = None
        if self._impl is not None:
            self._impl.reset()

    # -- results ----------------------------------------------------------------------------------
    def _results(self):
        if self._cache is None:
            if self.__dict__.get("_frozen") or self._impl is None:
                chain = np.empty((0, self.nwalkers, self.ndim)); lp = np.empty((0, self.nwalkers))
                nacc = np.zeros(self.nwalkers, dtype=np.int64); it = 0
            elif self._device:
                chain, lp = self._impl.get_chain()
                nacc, it, _ = self._impl.counts()
            else:
                h = self._impl
                chain = np.stack(h.chain) if h.chain else np.empty((0, self.nwalkers, self.ndim))
                lp = np.stack(h.lps) if h.lps else np.empty((0, self.nwalkers))
                nacc, it = h.naccepted.copy(), h.iterations
            self._cache = (chain, lp, nacc, it)
        return self._cache

    def _counts(self):
        """(accepted per walker, iterations) without the chain: the reference logs the acceptance fraction every
        ``n_logging_steps`` (ref: mcmc.py:98-107), and a download of the whole chain so far each time was 0.4 s of a
        3.4 s ``run_mcmc`` at C3."""
        if self._cache is not None:
            return self._cache[2], self._cache[3]
        if self.__dict__.get("_frozen") or self._impl is None:
            return np.zeros(self.nwalkers, dtype=np.int64), 0
        if self._device:
            nacc, it, _ = self._impl.counts()
            return nacc, it
        return self._impl.naccepted.copy(), self._impl.iterations

    @property
    def iteration(self):
        return self._counts()[1]

    @staticmethod
    def _thin(v, discard, thin, flat):
        v = v[discard + thin - 1::thin]
        if flat:
            v = v.reshape((-1,) + v.shape[2:])
        return v

    def get_chain(self, discard=0, thin=1, flat=False):
        return self._thin(self._results()[0], discard, thin, flat)

    def get_log_prob(self, discard=0, thin=1, flat=False):
        return self._thin(self._results()[1], discard, thin, flat)

    @property
    def flatchain(self):
        return self.get_chain(flat=True)

    @property
    def flatlnprobability(self):
        return self.get_log_prob(flat=True)

    @property
    def acceptance_fraction(self):
        nacc, it = self._counts()
        return nacc / float(max(it, 1))

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        # the chain still lives on the device: estimate there (no FFTs over a 500 MB host copy); GPEMU_ACF_HOST=1 or a
        # thinned / unpickled sampler takes the host routine
        if (self._impl is not None and getattr(self, "_device", False) and thin == 1 and not self.__dict__.get("_frozen")
                and not os.environ.get("GPEMU_ACF_HOST")):
            kw = {k: kwargs[k] for k in ("c", "tol", "quiet") if k in kwargs}
            if set(kwargs) <= {"c", "tol", "quiet"}:
                return self._impl.integrated_time(first=int(discard), **kw)
        return thin * integrated_time(self.get_chain(discard=discard, thin=thin), **kwargs)

    def get_diagnostics(self, discard=0, thin=1):
        """``gpemu.diagnostics.summary`` of ``get_chain(discard=discard, thin=thin)``, every walker as a chain, computed
        on the device -- in place while the chain still lives there, from the host copy otherwise.  The walkers of the
        stretch ensemble are not independent chains: R-hat compares walkers, and ``ess_*`` does not replace
        ``get_autocorr_time`` (emcee's tau)."""
        discard, thin = int(discard), int(thin)
        if self._impl is not None and getattr(self, "_device", False) and not self.__dict__.get("_frozen"):
            return self._impl.diagnostics(discard=discard + thin - 1, thin=thin)
        from . import diagnostics
        return diagnostics.summary(np.ascontiguousarray(self.get_chain(discard=discard, thin=thin)))

    def get_marginals(self, discard=0, thin=1, **kw):
        """``gpemu.marginals.summary`` of ``get_chain(discard=discard, thin=thin, flat=True)`` (``lower``, ``upper``,
        ``bins_1d``, ``bins_2d``, ``confidence``, ``kde``, ``n_grid``, ``kde2d``, ``n_grid_2d``, ``covariance_2d``), computed
        on the device -- in place while the chain still lives there (the box defaults to the prior box), from the host
        copy otherwise (``lower`` and ``upper`` are then required)."""
        discard, thin = int(discard), int(thin)
        if self._impl is not None and getattr(self, "_device", False) and not self.__dict__.get("_frozen"):
            return self._impl.marginals(discard=discard + thin - 1, thin=thin, **kw)
        from . import marginals
        if kw.get("lower") is None or kw.get("upper") is None:
            raise ValueError("the chain is on the host: pass lower and upper")
        return marginals.summary(np.ascontiguousarray(self.get_chain(discard=discard, thin=thin, flat=True)), **kw)

    def get_loo(self, discard=0, thin=1, models=None, **kw):
        """``DeviceSampler.loo`` of ``get_chain(discard=discard, thin=thin)`` (``leave_out``, ``shifts``, ``r_eff``): in
        place while the chain still lives on the device, from the host copy otherwise (``models`` are then required:
        the device models with the likelihood set up)."""
        discard, thin = int(discard), int(thin)
        if self._impl is not None and getattr(self, "_device", False) and not self.__dict__.get("_frozen"):
            return self._impl.loo(models=models, discard=discard + thin - 1, thin=thin, **kw)
        from . import loo
        if models is None:
            raise ValueError("the chain is on the host: pass the device models")
        return loo.chain_loo(models, self.get_chain(discard=discard, thin=thin, flat=True), **kw)

    def get_reweighted(self, discard=0, thin=1, models=None, **kw):
        """``DeviceSampler.reweight`` of ``get_chain(discard=discard, thin=thin)`` (``priors``, ``models_new``, ``lower``,
        ``upper``, ``probabilities``, ``bins_1d``, ``bins_2d``, ``smooth``, ``r_eff``, ``hpd``, ``kde``,
        ``posterior_predictive``): in place while the chain still lives on the device, from the host copy otherwise
        (``models`` are then required: the device models with the likelihood set up).  With ``posterior_predictive`` the
        bands are those of ``models`` (default: the sampler's groups)."""
        discard, thin = int(discard), int(thin)
        if self._impl is not None and getattr(self, "_device", False) and not self.__dict__.get("_frozen"):
            if kw.get("posterior_predictive") and models is not None:
                kw = dict(kw, models=models)
            return self._impl.reweight(discard=discard + thin - 1, thin=thin, **kw)
        from . import reweight
        if models is None:
            raise ValueError("the chain is on the host: pass the device models")
        return reweight.chain_reweight(models, self.get_chain(discard=discard, thin=thin, flat=True), **kw)

    def get_information_gain(self, discard=0, thin=1, **kw):
        """``gpemu.information.information_gain`` of ``get_chain(discard=discard, thin=thin, flat=True)`` (``lower``,
        ``upper``, ``k``, ``max_points``, ``subsets``, ``allow_copies``): in place while the chain still lives on the
        device (the box defaults to the prior box), from the host copy otherwise (``lower`` and ``upper`` are then
        required)."""
        discard, thin = int(discard), int(thin)
        if self._impl is not None and getattr(self, "_device", False) and not self.__dict__.get("_frozen"):
            return self._impl.information_gain(discard=discard + thin - 1, thin=thin, **kw)
        from . import information
        if kw.get("lower") is None or kw.get("upper") is None:
            raise ValueError("the chain is on the host: pass lower and upper")
        lower, upper = kw.pop("lower"), kw.pop("upper")
        return information.information_gain(np.ascontiguousarray(self.get_chain(discard=discard, thin=thin, flat=True)),
                                            lower, upper, **kw)

    def get_expected_information_gain(self, candidates, discard=0, thin=1, models=None, **kw):
        """``DeviceSampler.expected_information_gain`` of ``get_chain(discard=discard, thin=thin)`` (``n_inner``,
        ``n_outer``, ``seed``, ``emulator_cov``, ``exclude_self``): the rows gathered in place while the chain still lives
        on the device, taken from the host copy otherwise (``models`` are then required)."""
        discard, thin = int(discard), int(thin)
        if self._impl is not None and getattr(self, "_device", False) and not self.__dict__.get("_frozen"):
            return self._impl.expected_information_gain(candidates, models=models, discard=discard + thin - 1, thin=thin,
                                                        **kw)
        from . import experiment, information
        if models is None:
            raise ValueError("the chain is on the host: pass the device models")
        x = self.get_chain(discard=discard, thin=thin, flat=True)
        rows = information.selected_rows(x.shape[0], kw.pop("n_inner", 16384))
        return experiment.chain_expected_information_gain(models, np.ascontiguousarray(x[rows]), candidates, **kw)

    # -- pickling (ref: mcmc.py:131-132 pickles the sampler) --------------------------------------
    def __getstate__(self):
        st = dict(self.__dict__)
        st["_cache"] = self._results()
        st["_impl"] = None
        st["pool"] = None
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._frozen = True

class _RowCall:
    def __init__(self, f, args, kwargs):
        self.f, self.args, self.kwargs = f, args, kwargs

    def __call__(self, x):
        return self.f(x, *self.args, **self.kwargs)
