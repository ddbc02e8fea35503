"""Device resources (tests only): what tests/test_gpu_devmem.py runs beyond the tables it borrows, and the ledger
helpers.  The model- and sampler-bound operations are those of tests/reuse_cases.py, the ``_dev`` one-shots the
device-wide rows of tests/stream_cases.py; this module adds the host one-shots that have no row there, the chain
summaries of a sampler, the fit, diag and design handles, the table of warm allocation counts, and the proxy that
watches every library call of a borrowed test for a refusal that allocates.

The ledger (csrc/devledger.h) is read through ``gpemu._lib.devmem_stats``; every reading here is taken after
``gc.collect()`` and checks ``allocs - frees == live_blocks`` on the way.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import gc
import types

import numpy as np

import reuse_cases as R
import stream_cases as SC

ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -4, -5          # include/gpemu.h
LIVE = ("live_blocks", "live_bytes", "live_streams", "live_events")
WALK_CASES = ("general", "wide", "sources")
MIN_WALK_COMPARED = 12        # (case, operation) walks of every case that really compared bits after every refusal


# ---- the ledger ------------------------------------------------------------------------------------------------------
def reading():
    """the ledger after a garbage collection; its books balance at every reading"""
    from gpemu import _lib
    gc.collect()
    s = _lib.devmem_stats()
    assert s["allocs"] - s["frees"] == s["live_blocks"], f"the ledger's books do not balance: {s}"
    assert min(s.values()) >= 0, s
    return s


def live(s):
    return tuple(s[k] for k in LIVE)


def assert_back_to(base, what):
    now = reading()
    assert live(now) == live(base), (f"{what}: the ledger did not return to its baseline: "
                                     + ", ".join(f"{k} {base[k]} -> {now[k]}" for k in LIVE if now[k] != base[k]))
    return now


def allocs_of(fn):
    """(result of fn(), device allocations it made)"""
    from gpemu import _lib
    a0 = _lib.devmem_stats()["allocs"]
    out = fn()
    return out, _lib.devmem_stats()["allocs"] - a0


def refused(fn):
    """fn() must raise the library's error of a refused allocation; returns the message"""
    from gpemu._lib import GpemuError
    try:
        fn()
    except GpemuError as e:
        assert e.code == ERR_HIP and "refused" in str(e), f"expected the refusal, got {e.code}: {e}"
        return str(e)
    raise AssertionError("the call went through although an allocation was refused")


@contextlib.contextmanager
def disarmed_after():
    """whatever happens inside, no refusal stays armed"""
    from gpemu import _lib
    try:
        yield
    finally:
        _lib.devmem_refuse_nth(0)


# ---- a proxy of the library that watches refusals --------------------------------------------------------------------
class Watch:
    """Stands in for the loaded library while a borrowed test runs: every call whose integer result is negative -- the
    library declined it -- is recorded with the ledger before and after.  ``refusals``: (name, code, moved)."""

    def __init__(self, real):
        self._real = real
        self.refusals = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("gpemu_") or name in ("gpemu_last_error", "gpemu_devmem_stats", "gpemu_version"):
            return fn

        def call(*args):
            before = self._stats()
            rc = fn(*args)
            if isinstance(rc, int) and rc < 0:
                after = self._stats()
                self.refusals.append((name, rc, {k: (before[k], after[k]) for k in before if before[k] != after[k]}))
            return rc
        return call

    def _stats(self):
        from gpemu import _lib
        out = (C.c_int64 * 16)()
        n = self._real.gpemu_devmem_stats(out, 16)
        return {k: int(out[i]) for i, k in enumerate(_lib.DEVMEM_STATS[:n])}


@contextlib.contextmanager
def watching():
    from gpemu import _lib
    real = _lib.lib()
    w = Watch(real)
    _lib._lib = w
    try:
        yield w
    finally:
        _lib._lib = real


# ---- host one-shots without a row in stream_cases ---------------------------------------------------------------------
def _g(tag):
    import zlib
    return np.random.default_rng(zlib.crc32(f"devmem/{tag}".encode()))


S1, D1 = 257, 3                       # the shapes of stream_cases' device-wide rows
LO1, HI1 = np.zeros(D1), np.ones(D1)


def _x():
    return _g("x").uniform(0.1, 1.0, (S1, D1))


def _pca_fit():
    from gpemu.fit import pca_fit
    return R.flatten(pca_fit(_g("pca").normal(size=(9, 4))))


def _truncation_cov():
    from gpemu.fit import truncation_cov
    q, _ = np.linalg.qr(_g("trunc").normal(size=(6, 6)))
    return (truncation_cov(q, np.linspace(2.0, 0.1, 6), 2),)


def _kernel_matrix():
    from gpemu.fit import kernel_matrix
    return (kernel_matrix(_g("kmat").uniform(size=(20, 3)), np.log([0.5, 0.7, 0.9, 1.0, 1e-3]), 0, np.inf, True, True),)


def _cholesky():
    from gpemu.fit import cholesky
    a = _g("chol").normal(size=(20, 20))
    return (cholesky(a @ a.T + 20.0 * np.eye(20)),)


def _select():
    from gpemu import select
    return (select.order_statistics(_x(), [0, 128, 256], axis=0),)


def _rank():
    from gpemu import select
    return (select.rankdata(_x(), axis=0),)


def _hpd():
    from gpemu import marginals as M
    return (M.hpd_intervals(_x(), 0.9),)


def _kde1d():
    from gpemu import marginals as M
    return R.flatten(M.kde_1d(_x(), n_grid=16))


def _kde2d():
    from gpemu import marginals as M
    return R.flatten(M.kde_2d(_x(), n_grid=16))


def _marginal_hist():
    from gpemu import marginals as M
    return R.flatten(M.histograms(_x(), LO1, HI1, 8, 4))


def _psis():
    from gpemu import loo
    return R.flatten(loo.psis(-0.5 * _g("psis").normal(size=(3, S1)) ** 2 - 1.0, return_weights=True))


def _knn_dist():
    from gpemu import information as IG
    return R.flatten(IG.knn_distances(_x(), k=4))


def _pair_lse():
    from gpemu import experiment as EX
    g = _g("pairlse")
    return R.flatten(EX.pair_lse(g.normal(size=(33, 5)), g.normal(size=(S1, 5))))


_PRIORS = [[("normal", 0.5, 0.2), 0, 0], {1: ("normal", 0.4, 0.3)}]


def _logprior():
    from gpemu import reweight as RW
    return (RW.log_ratio(_x(), priors=_PRIORS, lower=LO1, upper=HI1),)


def _q():
    return _g("q").integers(2 ** 39, 2 ** 40, (1, S1)).astype(np.uint64)


def _weighted_select():
    from gpemu import reweight as RW
    return (RW.weighted_quantile(_x(), [0.05, 0.5, 0.95], _q()),)


def _weighted_hist():
    from gpemu import reweight as RW
    return R.flatten(RW.weighted_histograms(_x(), LO1, HI1, _q(), 8, 4))


def _q2():
    """two weight rows: the loops over the weight rows of the weighted intervals and densities run twice"""
    return _g("q2").integers(2 ** 39, 2 ** 40, (2, S1)).astype(np.uint64)


def _weighted_hpd():
    from gpemu import reweight as RW
    return (RW.weighted_hpd(_x(), (0.5, 0.9), _q2()),)


def _weighted_kde1d():
    from gpemu import reweight as RW
    return R.flatten(RW.weighted_kde_1d(_x(), _q2(), n_grid=16))


# Every host one-shot of include/gpemu.h -- first parameter `int device`, no stream, no ctx -- has an entry here under its
# name: tests/test_devmem_tables_host.py holds the table to the header.
HOST_ONE_SHOTS = {
    "gpemu_pca_fit": _pca_fit, "gpemu_truncation_cov": _truncation_cov, "gpemu_kernel_matrix": _kernel_matrix,
    "gpemu_cholesky": _cholesky, "gpemu_select": _select, "gpemu_rank": _rank, "gpemu_hpd": _hpd, "gpemu_kde1d": _kde1d,
    "gpemu_kde2d": _kde2d, "gpemu_marginal_hist": _marginal_hist, "gpemu_psis": _psis, "gpemu_knn_dist": _knn_dist,
    "gpemu_pair_lse": _pair_lse, "gpemu_logprior": _logprior, "gpemu_weighted_select": _weighted_select,
    "gpemu_weighted_hist": _weighted_hist, "gpemu_weighted_hpd": _weighted_hpd, "gpemu_weighted_kde1d": _weighted_kde1d,
}
# (gp_predict_cov, the fourth, is an operation of reuse_cases)
WALK_ONE_SHOTS = ("gpemu_pca_fit", "gpemu_kde2d", "gpemu_weighted_hpd")

DEVICE_WIDE_ROWS = [r for r in SC.ROWS if r.family == SC.DEVICE_WIDE and not r.omitted]


def run_wide_row(row):
    return SC.quiet(row, None, None, row.inputs(None, 0))[0]


# ---- the fit handle (the shape of test_gpu_fit_paths.py's first batch: N = 129, d = 3, Matern 1.5) ---------------------
def fit_problem():
    import fit_cases as FC
    c = FC.FitCase("devmem", 129, 3, FC.M, 1.5, True, True, jitter=0.0)
    ps = [FC.problem(c, seed=s) for s in range(3)]
    ys = np.stack([ps[z % 3].y for z in range(5)])
    thetas = np.stack([ps[z % 3].theta for z in range(5)])
    return c, ps[0].X, ys, thetas


def device_fit(c, X):
    from gpemu.fit import DeviceFit
    return DeviceFit(X, kernel_kind=c.kind, nu=c.nu, has_const=c.const, has_noise=c.noise, jitter=c.jitter)


FIT_STEPS = {
    "lml": lambda f, ys, th: R.flatten(f.lml(ys[0], th[0])),
    "lml_batch_1": lambda f, ys, th: R.flatten(f.lml_batch(ys[:1], th[:1])),
    "lml_batch_5": lambda f, ys, th: R.flatten(f.lml_batch(ys, th)),
    "factor": lambda f, ys, th: R.flatten(f.factor(ys[0], th[0])),
}


# ---- the diag and design handles ---------------------------------------------------------------------------------------
def diag_chain():
    return _g("diag").normal(size=(16, 4, D1))


def diag_calls(h):
    """a gpemu_diag handle through its calls"""
    out = []
    for kind in (1, 2):
        out += list(R.flatten(h.transform(kind)))
    out += list(R.flatten(h.value_range())) + list(R.flatten(h.series())) + list(R.flatten(h.acov(0, 8)))
    out += list(R.flatten(h.pooled())) + list(R.flatten(h.summary()))
    return tuple(out)


def diag_run():
    from gpemu.diagnostics import Diag
    with Diag(diag_chain()) as h:
        return diag_calls(h)


def design_run(dm, P):
    """a gpemu_design handle through scores, condition and state"""
    ref, cand = R.design_inputs(P)
    with dm.design(ref, cand, max_picks=4) as dg:
        s0 = dg.scores()
        dg.condition(int(np.argmax(s0)))
        return (s0, dg.scores()) + R.flatten(dg._groups[0].state(den=True))


# ---- the chain summaries of a sampler: at most 64 steps x 24 walkers ---------------------------------------------------
CHAIN_STEPS, CHAIN_W = 48, 24


def _candidates(P):
    f = np.arange(min(3, P.F))
    return [dict(features=f, y_err=P.y_err[f], label="a"), dict(features=f[:1], y_err=P.y_err[f[:1]], label="b")]


def _chain0(ds):
    """the two summaries a TemperedSampler does not wrap take the rung as a chain index"""
    return {"chain": 0} if ds.n_chains > 1 else {}


def _normal_prior(P):
    """one scenario: a normal prior on the first parameter, centred in the box, a quarter of its width wide"""
    return [{0: ("normal", float(P.lo[0] + P.hi[0]) / 2, float(P.hi[0] - P.lo[0]) / 4)}]


CHAIN_METHODS = {
    "posterior_predictive": lambda ds, P: ds.posterior_predictive(**_chain0(ds)),
    "parameter_quantiles": lambda ds, P: ds.parameter_quantiles([0.05, 0.5, 0.95], **_chain0(ds)),
    "diagnostics": lambda ds, P: ds.diagnostics(),
    "marginals": lambda ds, P: ds.marginals(bins_1d=8, bins_2d=4, n_grid=16, kde2d=True, n_grid_2d=16),
    "marginals_thinned": lambda ds, P: ds.marginals(bins_1d=8, bins_2d=4, n_grid=16, thin=2),
    "loo": lambda ds, P: ds.loo(),
    "reweight": lambda ds, P: ds.reweight(priors=_normal_prior(P), bins_1d=8, bins_2d=4),
    "reweight_thinned": lambda ds, P: ds.reweight(priors=_normal_prior(P), bins_1d=8, bins_2d=4, thin=2),
    # the weighted intervals, densities and bands of DESIGN.md §4.43 on the scenario's weights
    "reweight_summaries": lambda ds, P: ds.reweight(priors=_normal_prior(P), bins_1d=8, bins_2d=4, hpd=(0.9,), kde=True,
                                                    n_grid=16, posterior_predictive=True),
    "information_gain": lambda ds, P: ds.information_gain(allow_copies=True),
    "kl_divergence": lambda ds, P: ds.kl_divergence(R.rows(P, "devmem_kl", 200), allow_copies=True),
    "expected_information_gain": lambda ds, P: ds.expected_information_gain(_candidates(P), n_inner=256, n_outer=64),
    "propose_design": lambda ds, P: ds.propose_design(2, n_candidates=32, n_reference=128),
    "integrated_time": lambda ds, P: ds.integrated_time(quiet=True),
}
NO_LOO = ("sources",)                 # the per-observable terms decline correlated sources (reuse_cases.DECLINES)


def chain_sampler(dm, P, kind="stretch"):
    """a sampler of CHAIN_W walkers with CHAIN_STEPS stored steps"""
    if kind == "stretch":
        ds = R.stretch_sampler(dm, P, CHAIN_W, seed=13)
    elif kind == "tempered":
        ds = R.tempered_sampler(dm, P, CHAIN_W)
    else:
        ds = R.hmc_sampler(dm, P, 16)
    try:
        ds.run(CHAIN_STEPS)
    except BaseException:
        ds.close()
        raise
    return ds


# ---- the drop-in's model cache ---------------------------------------------------------------------------------------
def dropin_results(model):
    """what bayesian_inference.emulation.device_model_for reads of a results dict, from an oracle group model"""
    from oracle import gp_oracle as O
    spec = model.spec
    ems = [types.SimpleNamespace(
        X_train_=model.X_train, alpha_=gp.alpha, L_=gp.L,
        kernel_=types.SimpleNamespace(length_scale=gp.ls, kind=spec.kind, nu=spec.nu, has_const=spec.has_const,
                                      has_noise=spec.has_noise, constant_value=getattr(gp, "const", 0.0),
                                      noise_level=getattr(gp, "noise", 0.0))) for gp in model.gps]
    pca = types.SimpleNamespace(components_=model.components)
    scaler = types.SimpleNamespace(mean_=model.scaler_mean, scale_=model.scaler_scale)
    return {"emulators": ems, "PCA": {"pca": pca, "scaler": scaler}}, O.cov_unexplained(model)


# ---- warm allocation counts ------------------------------------------------------------------------------------------
# The device allocations of the THIRD of three identical calls on one live handle (a quiet device, the shapes of the rows
# and operations named).  0: everything the call needs is in the handle's workspace by then.  A positive count is a
# temporary that lives for the call (a DevScope): the entry waits for its stream before it returns, and its workspace is
# sized by the call's arguments.  The counts are what the code allocates at these shapes, read from the csrc file named;
# the test asserts them exactly, so that none of them grows unseen.
WARM_MODEL_DEV = {
    # include/gpemu.h: "do not synchronise" -- nothing of these may live for the call only
    "gpemu_gp_predict_dev": 0,
    "gpemu_predict_full_dev": 0,
    "gpemu_logpost_dev": 0,
    "gpemu_gp_predict_grad_dev": 0,
    "gpemu_logpost_grad_dev": 0,
    # the entries that wait for their stream: workspace that goes with the call
    # k_pcov.hip predict_cov: K_*^T and V of both sides and the product (5; the symmetric form 3), + the variances of
    # gpemu_gp_predict_cov_dev's mean (1): two calls of the row, (5 + 1) + 3
    "gpemu_gp_predict_cov_dev": 9,
    # k_postpred.hip: Mpc, Vpc, the staging rows of a view that is not dense, part, vbar, mu, W (7), and the 10 of the
    # select it runs (gpemu_select_dev, a device-wide row of its own)
    "gpemu_posterior_predictive_dev": 17,
    # k_postpred.hip pp_reduce under weights: Mpc, Vpc, the staging rows of a view that is not dense, part, vbar, mu, the
    # weight totals dQ, W (8); the weighted select runs once per weight row on the rows of W, each time with the 10 of
    # k_select.hip select_rows (prefix, trem, slotpre, slot, over, nslot, nan, hist, the targets, their permutation):
    # 8 + 2 * 10 for the row's two weight rows.  (weight_totals and weighted_rowmean of k_wsummary.hip allocate nothing.)
    "gpemu_posterior_predictive_weighted_dev": 28,
    # k_sobol.hip gpemu_sobol_moments_dev: Z, part, dpivot, dout, dstart, dfirst
    "gpemu_sobol_moments_dev": 6,
    # k_loo.hip gpemu_loglik_pointwise_dev: Mpc, Vpc and the staging rows of a view that is not dense
    "gpemu_loglik_pointwise_dev": 3,
}
# the three samplers after reserve(): a run allocates nothing
WARM_SAMPLER_RUN = {"stretch": 0, "tempered": 0, "hmc": 0}

# The host-array forms and the handles built on a model (the operations of reuse_cases), third of three identical calls:
# the inputs and outputs they stage in a DevScope, the handles they create and close inside the call.  One count per
# operation; a case whose launch path differs in what it stages has its own entry under (case, operation).
_LOGPOST = 2                          # gpemu_logpost: the rows and the result
_STRETCH = 19 + 1 + 2 + 1             # sampler_fill, set_state's staging rows, the chain pair, get_state's staging rows
WARM_HOST = dict(
    {f"logpost_{B}": _LOGPOST for B in R.LOGPOST_B},
    logpost_exact=_LOGPOST, logpost_2049=_LOGPOST,
    gp_predict=3,                     # rows, mean, var
    predict_full=3,                   # rows, central value, covariance
    gp_predict_cov=17,                # two calls: (X, X2, mean, cov) + predict_cov's 5 + 1, then (X, mean, cov) + 3 + 1
    gp_sample=17,                     # rows, mean, cov, z, draws; predict_cov's 3 + 1; sample_from_cov's 8
    gp_predict_grad=5,                # rows, mean, var and their two derivatives
    logpost_grad=3,                   # rows, lp, gradient
    loglik_pointwise=4,               # rows, terms; the device entry's Mpc, Vpc
    posterior_predictive=21,          # rows and the four results; the device entry's 6 (a dense view) + the select's 10
    # rows, weights and the four results (6); the device entry's 7 (a dense view: no staging rows) + the weighted
    # select's 10 for each of the two weight rows
    posterior_predictive_weighted=33,
    mean_pick_freeze=3,               # A, B, Z
    sobol_moments=8,                  # A, B; the device entry's 6
    cross_validate=14,                # folds, offsets, y, mean, var, the two observable-space results; cross_validate's 7
    expected_information_gain=14,     # gp_predict's 3; the pair log-sum-exp's 7 and its centre, the staged predictions
    design=18,                        # the two staged row sets, the handle's 15 fields, the create call's K_*^T
    logpost_dev=0,                    # the caller's tensors: nothing of the library's lives for the call
    stretch_24=_STRETCH, stretch_300=_STRETCH, stretch_300_no_compact=_STRETCH, phase_api=_STRETCH,
    hmc=_STRETCH + 12,                # + hmc_fill's fields
    tempered=_STRETCH + 4,            # + the ladder's fields
    run_peer=_STRETCH + 2,            # + the gather buffer and the table of the peers' buffers (k_front.hip)
)


def warm_host_count(case, opn):
    return WARM_HOST.get((case, opn), WARM_HOST.get(opn))
