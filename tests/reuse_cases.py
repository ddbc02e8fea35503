"""Handle reuse (tests only): the cases and the operations of tests/test_gpu_handle_reuse.py.

A case is a model and a likelihood setup, there for one family of launch paths.  An operation is a named closure
``(dm, P) -> tuple of arrays`` with its own fixed, seeded inputs: it depends on nothing but the model and the likelihood
setup, so that the same operation on a freshly created handle is its reference, bit for bit.  The table covers every
model-level entry point of gpemu/model.py and every handle built on a model.  Where include/gpemu.h documents that an
entry declines a case, DECLINES lists the (case, operation) pair with the error code; no other pair may fail.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import golden_util as GU
import path_cases as PC
from oracle import gp_oracle as O

R, M = O.RBF, O.MATERN
ERR_STATE, ERR_UNSUPPORTED = -4, -5                  # include/gpemu.h

_GENERAL = PC.Case("general", 130, 3, 3, 128, R, np.inf, False)
CASES = {
    # Npad 256, general three-launch path, small- and large-batch GEMM, compaction above 128 proposals
    "general": _GENERAL,
    # k_halfstep.hip at B <= 128 with k ceil(B / 32) >= 64 (B = 33, 128), the general path just below it (B = 32)
    "halfstep": PC.Case("halfstep", 65, 4, 32, 128, R, np.inf, False, nblk=2),
    # 16-wide rows, direct cross-kernel, tasks kernel
    "wide": PC.Case("wide", 64, 12, 5, 128, M, 0.75, False, nblk=6),
    # k > 16 (LDS likelihood), general-nu call frame
    "lds_nu": PC.Case("lds_nu", 64, 2, 17, 128, M, 2.0, True),
    # ticketed tasks kernel, term buffer growth
    "tasks10": PC.Case("tasks10", 300, 3, 5, 128, R, np.inf, False, nblk=10),
    # k_srccorr.hip, accept moved to the sources' launch: dense cov inside 2 blocks + 4 sys_sources
    "sources": dataclasses.replace(_GENERAL, name="sources", nblk=2),
    # chain-aware constants, variant_B: y_exp of shape (3, F)
    "chains": dataclasses.replace(_GENERAL, name="chains"),
}
CASE_IDS = list(CASES)
MIN_COMPARED = 16                                  # operations of every case that must really compare


@dataclass
class Problem:
    name: str
    case: PC.Case
    model: object
    lo: np.ndarray
    hi: np.ndarray
    setup: dict                                      # keywords of DeviceModel.likelihood_setup
    Y: np.ndarray                                    # (3, F) data vectors (the setups of one vector take the first)
    y_err: np.ndarray
    block_start: np.ndarray

    @property
    def d(self):
        return self.case.d

    @property
    def k(self):
        return self.case.k

    @property
    def F(self):
        return self.y_err.size

    @property
    def n_chains(self):
        return self.setup["y_exp"].shape[0] if np.ndim(self.setup["y_exp"]) == 2 else 1


def _rng(P, tag):
    return np.random.default_rng(zlib.crc32(f"{P.name}/{tag}".encode()))


def block_cov(y_err, block_start, rho=0.3):
    """a dense covariance inside the observable blocks (equicorrelated), zero across them; exactly symmetric"""
    F = y_err.size
    cov = np.zeros((F, F))
    for o in range(len(block_start) - 1):
        a, b = int(block_start[o]), int(block_start[o + 1])
        cov[a:b, a:b] = rho * np.outer(y_err[a:b], y_err[a:b])
    cov[np.arange(F), np.arange(F)] = y_err ** 2
    return cov


def setup_variant(P, kind, n_div=1.0):
    """keywords of likelihood_setup for one of the setups a model is walked through (test_likelihood_resetup) and the
    cases are built from: 'chains' (3 vectors), 'single' (one vector, the case's blocks), 'sources' (dense cov inside 2
    blocks + 4 sources), 'diagonal' (no block_start), 'blocks2', 'block1'"""
    F = P.F
    two = np.array([0, F // 2, F], dtype=np.int64)
    base = dict(y_err=P.y_err, lo=P.lo, hi=P.hi, n_div=float(n_div))
    if kind == "chains":
        return dict(base, y_exp=P.Y.copy(), block_start=P.block_start)
    if kind == "single":
        return dict(base, y_exp=P.Y[0].copy(), block_start=P.block_start)
    if kind == "sources":
        bs = P.block_start if len(P.block_start) == 3 else two
        src = 0.3 * P.y_err * np.random.default_rng(41).normal(size=(4, F))
        return dict(base, y_exp=P.Y[0].copy(), block_start=bs, cov=block_cov(P.y_err, bs), sys_sources=src)
    if kind == "diagonal":
        return dict(base, y_exp=P.Y[0].copy())
    if kind == "blocks2":
        return dict(base, y_exp=P.Y[0].copy(), block_start=two)
    if kind == "block1":
        return dict(base, y_exp=P.Y[0].copy(), block_start=np.array([0, F], dtype=np.int64))
    raise KeyError(kind)


@lru_cache(maxsize=None)
def problem(name):
    c = CASES[name]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Y = np.stack([y_exp, y_exp + 0.03 * rng.normal(size=y_exp.size), y_exp - 0.04 * rng.normal(size=y_exp.size)])
    P = Problem(name, c, model, lo, hi, {}, Y, y_err, bs)
    P.setup = setup_variant(P, {"sources": "sources", "chains": "chains"}.get(name, "single"))
    return P


def apply_setup(dm, setup):
    kw = dict(setup)
    dm.likelihood_setup(kw.pop("y_exp"), kw.pop("y_err"), kw.pop("lo"), kw.pop("hi"), kw.pop("n_div"), **kw)


def fresh(P, setup=None):
    """a newly created model handle given only this likelihood setup"""
    dm = GU.device_model(P.model)
    apply_setup(dm, P.setup if setup is None else setup)
    return dm


# ---- inputs ----------------------------------------------------------------------------------------------------------
def rows(P, tag, B, inner=0.0):
    """B seeded rows inside the prior box (shrunk by `inner` of its width on every side)"""
    w = P.hi - P.lo
    return _rng(P, tag).uniform(P.lo + inner * w, P.hi - inner * w, (B, P.d))


def logpost_rows(P, B):
    """rows all over the box, every seventh outside it, one on a face, one with a NaN coordinate"""
    X = rows(P, f"logpost{B}", B)
    X[5::7, 0] = P.hi[0] + 0.25 * (P.hi[0] - P.lo[0])
    if B > 40:
        X[40, P.d - 1] = np.nan
        X[23, 0] = P.lo[0]
    return X


def walkers(P, tag, W):
    return rows(P, tag, W, inner=0.02)


def seeds_of(P, seed):
    """the seed keywords of a stretch sampler: one chain per data vector of the setup"""
    return dict(seed=seed) if P.n_chains == 1 else dict(seeds=[seed + 101 * c for c in range(P.n_chains)])


# ---- results ---------------------------------------------------------------------------------------------------------
def flatten(x):
    """any nesting of dicts, sequences, arrays and numbers as a tuple of arrays (labels and other text left out)"""
    if isinstance(x, dict):
        return tuple(a for key in sorted(x) for a in flatten(x[key]))
    if isinstance(x, (list, tuple)):
        return tuple(a for v in x for a in flatten(v))
    if isinstance(x, (str, bytes)) or x is None:
        return ()
    a = np.asarray(x)
    return () if a.dtype.kind in "OUS" else (a,)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.int64), b.view(np.int64))       # NaN patterns and signed zeros included
    return np.array_equal(a, b)


def sampler_result(ds):
    """chain, log-probabilities, state and counts of any sampler handle, flat (walker after walker)"""
    from gpemu import _lib
    from gpemu.sampler import DeviceSampler as DS
    rc = _lib.lib().gpemu_sampler_check(ds._h)
    X, lp = DS.get_state(ds)
    nacc, it, cl = DS.counts(ds)
    chain, lpchain = DS.get_chain(ds)
    return (chain, lpchain, X, lp, nacc, np.array([it, cl, rc], dtype=np.int64),
            np.array(DS.live_counts.fget(ds), dtype=np.int64))


# ---- the operations --------------------------------------------------------------------------------------------------
def _logpost(B, mode=0):
    return lambda dm, P: (dm.logpost(logpost_rows(P, B), mode=mode),)


def _gp_predict(dm, P):
    return dm.gp_predict(rows(P, "gp_predict", 100))


def _predict_full(dm, P):
    return dm.predict_full(rows(P, "predict_full", 33))


def _gp_predict_cov(dm, P):
    X, X2 = rows(P, "pcov1", 40), rows(P, "pcov2", 25)
    return dm.gp_predict_cov(X, X2) + dm.gp_predict_cov(X)


def _gp_sample(dm, P):
    z = _rng(P, "gp_sample_z").normal(size=(P.k, 20, 3))
    return dm.gp_sample(rows(P, "gp_sample", 20), z)


def _gp_predict_grad(dm, P):
    return dm.gp_predict_grad(rows(P, "gp_predict_grad", 70))


def _logpost_grad(dm, P):
    return dm.logpost_grad(logpost_rows(P, 70))


def _loglik_pointwise(dm, P):
    return (dm.loglik_pointwise(logpost_rows(P, 100), chain=P.n_chains - 1),)


def _posterior_predictive(dm, P):
    return flatten(dm.posterior_predictive(rows(P, "postpred", 300)))


def postpred_weights(P, S, R_w=2):
    """R_w rows of integer weights in [2^39, 2^40): a row of S <= 512 of them adds up to less than 2^49, far below the
    2^53 that include/gpemu.h asks of a row's total"""
    return _rng(P, "postpred_w_q").integers(2 ** 39, 2 ** 40, (R_w, S)).astype(np.uint64)


def _posterior_predictive_weighted(dm, P):
    """The weighted bands under two weight rows, one dict per row (total_weight among its arrays).  The problems here have
    6 and 8 features, which always fit the workspace at once: only the whole-features path runs.  The feature-blocked one
    stays with the 40-feature model of tests/test_gpu_wsummary.py."""
    return flatten(dm.posterior_predictive_weighted(rows(P, "postpred_w", 300), postpred_weights(P, 300)))


def _mean_pick_freeze(dm, P):
    return (dm.mean_pick_freeze(rows(P, "sobolA", 64), rows(P, "sobolB", 64)),)


def _sobol_moments(dm, P):
    return flatten(dm.sobol_moments(rows(P, "sobolA", 64), rows(P, "sobolB", 64), n_batches=4))


def _cross_validate(dm, P):
    y = _rng(P, "cv_y").normal(size=(P.case.N, P.k))
    return dm.cross_validate(y, np.arange(P.case.N) % 5)


def _eig(dm, P):
    f = np.arange(min(3, P.F))
    return flatten(dm.expected_information_gain(rows(P, "eig", 256), f, y_err=P.y_err[f], n_outer=128, seed=3))


def design_inputs(P):
    return rows(P, "design_ref", 200), rows(P, "design_cand", 70)


def _design(dm, P):
    ref, cand = design_inputs(P)
    with dm.design(ref, cand, max_picks=4) as dg:
        s0 = dg.scores()
        dg.condition(int(np.argmax(s0)))
        return s0, dg.scores(), np.array([dg.integrated_variance()])


def _logpost_dev(dm, P):
    """the rows sit inside a wider tensor: rows 17 .. 17 + B of a tensor of B + 40, the output inside another"""
    import torch
    B = 90
    dev = torch.device("cuda", dm.device)
    wide = torch.full((B + 40, P.d), float("nan"), dtype=torch.float64, device=dev)
    wide[17:17 + B] = torch.from_numpy(logpost_rows(P, B)).to(dev)
    out = torch.full((B + 9,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    dm.logpost_dev(wide[17:].data_ptr(), B, out[4:].data_ptr())
    dm.sync()
    return (out.cpu().numpy(),)


def stretch_sampler(dm, P, W, seed=11):
    from gpemu.sampler import DeviceSampler
    ds = DeviceSampler([dm], W, **seeds_of(P, seed))
    ds.set_state(walkers(P, f"stretch{W}", W * P.n_chains))
    return ds


def _stretch(W, no_compact=False):
    def op(dm, P):
        old = os.environ.pop("GPEMU_NO_COMPACT", None)
        if no_compact:
            os.environ["GPEMU_NO_COMPACT"] = "1"
        try:
            ds = stretch_sampler(dm, P, W)
            try:
                ds.run(3)
                return sampler_result(ds)
            finally:
                ds.close()
        finally:
            os.environ.pop("GPEMU_NO_COMPACT", None)
            if old is not None:
                os.environ["GPEMU_NO_COMPACT"] = old
    return op


def hmc_sampler(dm, P, W=16):
    from gpemu.sampler import HMCSampler
    hs = HMCSampler([dm], W, n_leapfrog=3, step_size=0.05, seed=8)
    hs.set_state(walkers(P, "hmc", W))
    return hs


def _hmc(dm, P):
    hs = hmc_sampler(dm, P)
    try:
        hs.run(2)
        return sampler_result(hs) + flatten(hs.stats())
    finally:
        hs.close()


def tempered_sampler(dm, P, W=24):
    from gpemu.sampler import TemperedSampler
    ts = TemperedSampler([dm], W, [1.0, 0.5], seed=5, swap_every=1)
    ts.set_state(walkers(P, "tempered", 2 * W))
    return ts


def _tempered(dm, P):
    ts = tempered_sampler(dm, P)
    try:
        ts.run(2)
        return sampler_result(ts)
    finally:
        ts.close()


def phase_steps(ds, steps, slices=3):
    """`steps` steps through the per-phase API, every half cut into `slices` slices (the all-gather: a concatenation)"""
    import torch
    from gpemu import _lib
    from gpemu.sampler import shard_bounds
    L = _lib.lib()
    dev = torch.device("cuda", ds.device)
    _lib.check(L.gpemu_sampler_reserve_chain(ds._h, steps))
    for _ in range(steps):
        _lib.check(L.gpemu_sampler_begin_step(ds._h))
        for h in (0, 1):
            n = ds.ns[h]
            per = shard_bounds(n, slices, 0)[2]
            full = torch.zeros(per * slices, dtype=torch.float64, device=dev)
            for r in range(slices):
                l0, h0, _ = shard_bounds(n, slices, r)
                mine = torch.zeros(per, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()              # (the fill runs on torch's stream, the evaluation on the sampler's)
                _lib.check(L.gpemu_sampler_half_propose_eval(ds._h, h, l0, h0, C.c_void_p(mine.data_ptr())))
                torch.cuda.synchronize()
                full[r * per:(r + 1) * per] = mine
            torch.cuda.synchronize()
            _lib.check(L.gpemu_sampler_half_accept(ds._h, h, C.c_void_p(full.data_ptr()), 1))
        _lib.check(L.gpemu_sampler_end_step(ds._h, 1))


def _phase(dm, P):
    ds = stretch_sampler(dm, P, 70, seed=31)
    try:
        phase_steps(ds, 2)
        return sampler_result(ds)
    finally:
        ds.close()


def _peer(dm, P):
    """gpemu_sampler_run_peer with a one-rank import: the fused two-launch half-step"""
    from gpemu import _lib
    L = _lib.lib()
    ds = stretch_sampler(dm, P, 24, seed=7)
    try:
        h = (C.c_char * 64)()
        _lib.check(L.gpemu_sampler_peer_export(ds._h, C.cast(h, C.c_void_p)))
        _lib.check(L.gpemu_sampler_peer_import(ds._h, 1, 0, C.cast(h, C.c_void_p)))
        _lib.check(L.gpemu_sampler_run_peer(ds._h, 2, 1))
        return sampler_result(ds)
    finally:
        ds.close()


@dataclass
class Op:
    name: str
    fn: object
    only: tuple = ()                                 # the cases it runs on (empty: all)


LOGPOST_B = (1, 32, 33, 64, 65, 128, 129, 257, 600)
OPS = [Op(f"logpost_{B}", _logpost(B)) for B in LOGPOST_B] + [
    Op("logpost_exact", _logpost(50, mode=1)),
    Op("logpost_2049", _logpost(2049), only=("general",)),
    Op("gp_predict", _gp_predict),
    Op("predict_full", _predict_full),
    Op("gp_predict_cov", _gp_predict_cov),
    Op("gp_sample", _gp_sample),
    Op("gp_predict_grad", _gp_predict_grad),
    Op("logpost_grad", _logpost_grad),
    Op("loglik_pointwise", _loglik_pointwise),
    Op("posterior_predictive", _posterior_predictive),
    Op("posterior_predictive_weighted", _posterior_predictive_weighted),
    Op("mean_pick_freeze", _mean_pick_freeze),
    Op("sobol_moments", _sobol_moments),
    Op("cross_validate", _cross_validate),
    Op("expected_information_gain", _eig),
    Op("design", _design),
    Op("logpost_dev", _logpost_dev),
    Op("stretch_24", _stretch(24)),
    Op("stretch_300", _stretch(300)),
    Op("stretch_300_no_compact", _stretch(300, no_compact=True)),
    Op("hmc", _hmc),
    Op("tempered", _tempered),
    Op("phase_api", _phase),
    Op("run_peer", _peer),
]
OP = {op.name: op for op in OPS}


def ops_of(name):
    return [op for op in OPS if not op.only or name in op.only]


# (case, operation) -> the error code include/gpemu.h documents for it
DECLINES = {
    # derivatives: RBF and Matern nu = 1.5, 2.5, inf only; no correlated sources, one data vector ("derivatives with
    # respect to the parameters"); the HMC sampler declines at create whatever gpemu_logpost_grad declines
    ("wide", "gp_predict_grad"): ERR_UNSUPPORTED,
    ("wide", "logpost_grad"): ERR_UNSUPPORTED,
    ("wide", "hmc"): ERR_UNSUPPORTED,
    ("lds_nu", "gp_predict_grad"): ERR_UNSUPPORTED,
    ("lds_nu", "logpost_grad"): ERR_UNSUPPORTED,
    ("lds_nu", "hmc"): ERR_UNSUPPORTED,
    ("sources", "logpost_grad"): ERR_UNSUPPORTED,
    ("sources", "hmc"): ERR_UNSUPPORTED,
    ("chains", "logpost_grad"): ERR_UNSUPPORTED,
    ("chains", "hmc"): ERR_UNSUPPORTED,
    # the peer transport: d <= 7 parameters, one chain, no correlated sources (gpemu_sampler_peer_export)
    ("wide", "run_peer"): ERR_UNSUPPORTED,
    ("sources", "run_peer"): ERR_UNSUPPORTED,
    ("chains", "run_peer"): ERR_UNSUPPORTED,
    # GPEMU_LOGPOST_EXACT with n_src > 0 (gpemu_likelihood_setup_cov); the per-observable terms with sources
    ("sources", "logpost_exact"): ERR_UNSUPPORTED,
    ("sources", "loglik_pointwise"): ERR_UNSUPPORTED,
    # a tempered sampler on a group set up with several data vectors (gpemu_sampler_create_tempered)
    ("chains", "tempered"): ERR_STATE,
}


def run_op(op, dm, P):
    """('ok', arrays) or ('declined', code, message): only the library's own refusal counts as a decline"""
    from gpemu._lib import GpemuError
    try:
        return ("ok", tuple(np.array(a, copy=True) for a in flatten(op.fn(dm, P))))
    except GpemuError as e:
        return ("declined", e.code, str(e))


def assert_same(case, op, got, want, what):
    """`got` (a used handle) against `want` (a fresh one): the same arrays bit for bit, or the documented decline with
    the same code and message.  Returns True where arrays were compared."""
    code = DECLINES.get((case, op.name))
    if code is not None:
        assert want[0] == "declined" and want[1] == code, f"{case}/{op.name}: a fresh handle should decline with {code}: {want[:2]}"
        assert got == want, f"{case}/{op.name} ({what}): {got} on the used handle, {want} on a fresh one"
        return False
    assert want[0] == "ok", f"{case}/{op.name}: failed on a fresh handle: {want[1:]}"
    assert got[0] == "ok", f"{case}/{op.name} ({what}): failed on the used handle: {got[1:]}"
    assert len(got[1]) == len(want[1]) and len(want[1]) > 0, f"{case}/{op.name} ({what}): {len(got[1])} arrays, {len(want[1])} fresh"
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        if not same_bits(a, b):
            bad = np.flatnonzero(~((a == b) | ((a != a) & (b != b))).reshape(-1)) if a.shape == b.shape else []
            raise AssertionError(f"{case}/{op.name} ({what}): array {i} of shape {a.shape} differs from a fresh handle's "
                                 f"in {len(bad)} elements, first at {bad[:5]}")
    return True
