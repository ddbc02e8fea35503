"""The device autocorrelation estimate (csrc/k_acf.hip: gpemu_sampler_acf, DeviceSampler.integrated_time) and the pooled
chain moments (k_rows.hip: moments_to_host) against the extended-precision reference and the a-priori bounds of
tests/acf_ref.py, on planted chains: the samplers run n_t stored steps on the smallest models of tests/path_cases.py
and the stored chain is then overwritten through chain_ptr with the series of the case.

What the device gave on an MI355X (worst err / bound of f per data kind): see DESIGN.md 4.10.  No row left its bound.
Constant series: NaN at every lag (acf_constant_mean_kernel); constant rows of the pooled moments: variance within
e_mu^2, exactly 0 only where the mean comes out exact (R = 1 always does)."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import acf_ref as A
import golden_util as GU
import path_cases as PC
from gpemu import _lib
from gpemu import sampler as S

pytestmark = pytest.mark.gpu

MODEL_OF_D = {1: "n17_d1_m25", 2: "n64_nu2_const", 7: "n16_d7_m15_const", 16: "w16_ks5_m05_direct_small"}
WORST = {}                       # data kind -> worst err / bound of f seen so far (printed by the tests that add to it)


class _Raw:
    def __init__(self, address, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(address), False),
                                         "version": 2}


_MODELS = {}


def _model(d):
    if d not in _MODELS:
        c = [x for x in PC.cases() if x.name == MODEL_OF_D[d]][0]
        model, lo, hi, y_exp, y_err, bs, _ = PC.problem(c)
        dm = GU.device_model(model)
        dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
        _MODELS[d] = (dm, lo, hi)
    return _MODELS[d]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for dm, _, _ in _MODELS.values():
        dm.close()
    _MODELS.clear()


def _start(lo, hi, W, seed):
    return np.random.default_rng(seed).uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), (W, lo.size))


def _plant(ds, wide):
    """overwrite the stored chain with ``wide[steps][W][d]``, in place"""
    import torch
    base, n = ds.chain_ptr(0)
    assert (n, ds.W, ds.d) == wide.shape
    dev = torch.device("cuda", ds.device)
    chain = torch.as_tensor(_Raw(base, wide.shape), device=dev)
    chain.copy_(torch.from_numpy(np.array(wide)).to(dev))
    torch.cuda.synchronize()


def _sampler(row, kind="stretch"):
    """a sampler of row.width walkers that has stored row.first + row.n_t steps and holds the row's chain"""
    dm, lo, hi = _model(row.d)
    W, per = row.width, row.width // row.chains
    if kind == "hmc":
        ds = S.HMCSampler([dm], W, n_leapfrog=1, step_size=0.05, seed=row.seed)
    elif kind == "tempered":
        ds = S.TemperedSampler([dm], per, np.linspace(1.0, 0.2, row.chains), seed=row.seed)
    elif row.chains == 1:
        ds = S.DeviceSampler([dm], W, seed=row.seed)
    else:
        ds = S.DeviceSampler([dm], per, seeds=[row.seed + 100 * c for c in range(row.chains)])
    ds.set_state(_start(lo, hi, W, row.seed))
    ds.run(row.first + row.n_t)
    _plant(ds, A.data(row)[0])
    return ds


def _tau_slack(windows, tau):
    """the rounding of the host's float64 running sum of f, which the bound of tau (2 sum df) does not count: w + 1 adds,
    each relative to a partial sum of at most (1 + |tau|) / 2, doubled"""
    return 2.0 * (windows + 1) * A.U * (1.0 + np.abs(tau))


def _args(row):
    return dict(first=row.first, n=row.n_t, w0=row.w0, nw=row.nw)


def _blocks(ds, row, blocks=None):
    return np.concatenate([ds.acf_block(l0, n, **_args(row)) for l0, n in (blocks or row.blocks)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _raw_acf(ds, first, n, w0, nw, lag0, n_lags, rows=None):
    """(return code, f_out) of the C entry; f_out is pre-filled with a sentinel"""
    f = np.full((int(rows or n_lags), ds.d), -777.0)
    rc = _lib.lib().gpemu_sampler_acf(ds._h, int(first), int(n), int(w0), int(nw), int(lag0), int(n_lags), _lib.ptr(f))
    return rc, f


def _hold(row, got, lags=None):
    """got within the bound of the reference at ``lags`` (default: the first rows of it); NaN exactly where it is"""
    f, df = A.ref(row).f(row.n_lags if lags is None else int(np.max(lags)) + 1)
    if lags is not None:
        f, df = f[lags], df[lags]
    q, same_nan = A.err_over_bound(got, f[:got.shape[0]], df[:got.shape[0]])
    WORST[row.kind] = max(WORST.get(row.kind, 0.0), q)
    assert same_nan, f"{row.name}: NaN where the reference is finite, or the reverse"
    assert q <= 1.0, f"{row.name}: f leaves its bound, err / bound = {q:.3g}"
    return q


# ---- 1. the bound on f, 3. tau and the windows, and the bits of a second call and of a partition -------------------------
@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_f_tau_and_windows_within_the_bounds(row):
    R = A.ref(row)
    ds = _sampler(row)
    try:
        got = _blocks(ds, row)
        q = _hold(row, got)
        print(f"\n{row.name}: err / bound of f = {q:.3g}; worst per data kind so far "
              + ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))
        # 2. a second call, and any partition into blocks at multiples of 16, give the same bits
        assert np.array_equal(_bits(_blocks(ds, row)), _bits(got))
        if row.lags == "blocks":
            assert np.array_equal(_bits(_blocks(ds, row, [(0, row.n_lags)])), _bits(got))
            part = [(l0, min(48, row.n_lags - l0)) for l0 in range(0, row.n_lags, 48)]
            assert np.array_equal(_bits(_blocks(ds, row, part)), _bits(got))
        # 3. Sokal's windows of the device's f are the reference's; tau within its bound, by either block size
        windows, tau, dtau, margins, _ = R.tau()
        L = max(len(m) for m in margins)
        fdev = _blocks(ds, row, [(0, L)]) if L <= A.MAX_LAGS else got
        w_dev, _, _ = A.sokal(fdev, row.n_t)
        assert np.array_equal(w_dev, windows), (w_dev, windows)
        fin = np.isfinite(tau)
        for block in (16, 256):
            t_dev = ds.integrated_time(quiet=True, block=block, **_args(row))
            assert np.array_equal(np.isnan(t_dev), ~fin), (t_dev, tau)
            assert np.all(np.abs(t_dev - tau)[fin] <= (dtau + _tau_slack(windows, tau))[fin]), (t_dev, tau, dtau)
        # 4. a constant series makes its parameter NaN at every lag and no other
        stuck = A.stuck_parameters(row)
        assert np.array_equal(np.flatnonzero(np.isnan(got).all(axis=0)), np.array(stuck, dtype=int))
        assert not np.isnan(np.delete(got, np.array(stuck, dtype=int), axis=1)).any()
    finally:
        ds.close()


def test_short_chain_error_carries_the_tau_of_the_reference():
    row = A.ROW["n127_s259_phi95_blocks"]           # tau ~ 10 of 127 steps: shorter than 50 tau
    windows, tau, dtau, _, _ = A.ref(row).tau()
    ds = _sampler(row)
    try:
        with pytest.raises(S.AutocorrError) as err:
            ds.integrated_time(**_args(row))
        assert np.all(np.abs(err.value.tau - tau) <= dtau + _tau_slack(windows, tau))
    finally:
        ds.close()


@pytest.mark.parametrize("kind", ["tempered", "hmc"])
def test_tau_through_the_tempered_and_the_hmc_sampler(kind):
    """TemperedSampler.integrated_time(temp=1) reads rung 1's walkers of the stacked chain; an HMCSampler's chains are
    the walkers.  Planted chains, the reference's windows and tau within its bound."""
    if kind == "tempered":
        row = A.Row("tempered_rung1", 130, 37, 7, w0=37, W=74, chains=2, seed=31)
    else:
        row = A.Row("hmc_chains", 130, 37, 7, seed=32)
    R = A.ref(row)
    windows, tau, dtau, margins, _ = R.tau()
    assert R.conditioned and np.all(np.isfinite(tau))
    ds = _sampler(row, kind)
    try:
        for block in (16, 256):
            t_dev = ds.integrated_time(temp=1, quiet=True, block=block) if kind == "tempered" else \
                ds.integrated_time(quiet=True, block=block)
            assert np.all(np.abs(t_dev - tau) <= dtau + _tau_slack(windows, tau)), (t_dev, tau, dtau)
        L = max(len(m) for m in margins)
        fdev = ds.acf_block(0, L, **_args(row))
        _hold(row, fdev, np.arange(L))
        assert np.array_equal(A.sokal(fdev, row.n_t)[0], windows)
    finally:
        ds.close()


# ---- 2. bits --------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_ensemble_around_the_block_or_on_a_power_of_two():
    base = A.ROW["n130_w5_first3_blocks"]
    ds = _sampler(base)
    got = _blocks(ds, base)
    ds.close()
    # the same series as the whole ensemble of an nw-walker sampler, from step 0
    alone = A.Row("alone", base.n_t, base.nw, base.d, seed=base.seed)
    dm, lo, hi = _model(base.d)
    d2 = S.DeviceSampler([dm], base.nw, seed=1)
    d2.set_state(_start(lo, hi, base.nw, 1))
    d2.run(base.n_t)
    _plant(d2, A.data(base)[1])
    same = _blocks(d2, dataclasses.replace(alone, lags="blocks"))
    d2.close()
    assert np.array_equal(_bits(same), _bits(got)), "walkers [5, 42) of 48 and a 37-walker sampler differ"
    # x 2^-400 and x 2^400: every operation scales exactly
    for name in ("n130_w5_scale_dn", "n130_w5_scale_up"):
        row = A.ROW[name]
        assert np.array_equal(A.data(row)[1], A.data(base)[1] * 2.0 ** (-400 if row.kind == "scale_dn" else 400))
        ds = _sampler(row)
        scaled = _blocks(ds, row)
        ds.close()
        assert np.array_equal(_bits(scaled), _bits(got)), name


# ---- 5. a continuation of an estimate whose chain has changed ------------------------------------------------------------
def _snapshot_run_restore(ds):
    _lib.check(_lib.lib().gpemu_sampler_snapshot(ds._h))
    ds.run(5)
    _lib.check(_lib.lib().gpemu_sampler_restore(ds._h))


@pytest.mark.parametrize("change", ["reset_and_run", "snapshot_run_restore", "further_run", "reserve"])
def test_a_lag_block_after_the_chain_changed_is_refused(change):
    """After a lag-0 block, a lag-16 block with the same (first, n, w0, nw) would be normalised by the old chain's means
    and lag-0 products: whatever bumps the chain's epoch ends the estimate with GPEMU_ERR_STATE, before any launch."""
    row = A.Row("stale", 130, 37, 7, seed=41)
    other = A.Row("stale_other", 130, 37, 7, phi=0.95, seed=42)
    a = (row.first, row.n_t, row.w0, row.nw)
    ds = _sampler(row)
    try:
        rc, _ = _raw_acf(ds, *a, 0, 16)
        assert rc == 0
        rc, cont = _raw_acf(ds, *a, 16, 16)
        assert rc == 0
        _hold(row, cont, np.arange(16, 32))
        {"reset_and_run": lambda: (ds.reset(), ds.run(row.n_t)),
         "snapshot_run_restore": lambda: _snapshot_run_restore(ds),
         "further_run": lambda: ds.run(3),
         "reserve": lambda: ds.reserve(5000)}[change]()
        steps = ds.counts()[2]
        wide = np.array(A.data(other)[0])
        if steps > row.n_t:
            wide = np.concatenate([wide, wide[:steps - row.n_t]])
        _plant(ds, wide)                                  # another chain lies in those rows now
        rc, f = _raw_acf(ds, *a, 16, 16)
        assert rc == -4, f"a stale continuation returned {rc}"
        assert np.all(f == -777.0), "a refused call wrote its output"
        assert "lag 0" in _lib.last_error()
        rc, _ = _raw_acf(ds, *a, 0, 16)
        assert rc == 0
        rc, cont = _raw_acf(ds, *a, 16, 16)
        assert rc == 0
        _hold(other, cont, np.arange(16, 32))
        # other arguments than the estimate's: the argument error it always was
        rc, f = _raw_acf(ds, row.first, row.n_t - 1, row.w0, row.nw, 16, 16)
        assert rc == -1 and np.all(f == -777.0)
    finally:
        ds.close()


# ---- 6. argument edges ------------------------------------------------------------------------------------------------------
def test_argument_edges_are_refused_before_any_launch():
    row = A.ROW["n4100_lag_cap"]
    a = (row.first, row.n_t, row.w0, row.nw)
    ds = _sampler(row)
    try:
        whole = ds.acf_block(0, 4096, **_args(row))
        rc, f = _raw_acf(ds, *a, 0, 32)
        assert rc == 0 and np.array_equal(_bits(f), _bits(whole[:32]))
        bad = [("n_lags = 4097", (*a, 0, 4097)),
               ("lag0 = 8", (*a, 8, 16)),
               ("walkers past W", (row.first, row.n_t, 1, 2, 16, 16)),
               ("rows past the chain", (row.first + 1, row.n_t, row.w0, row.nw, 16, 16))]
        for what, args in bad:
            rc, f = _raw_acf(ds, *args)
            assert rc == -1 and np.all(f == -777.0), what
            # nothing was launched and nothing forgotten: the estimate goes on where it was
            rc, f = _raw_acf(ds, *a, 16, 16)
            assert rc == 0 and np.array_equal(_bits(f), _bits(whole[16:32])), what
    finally:
        ds.close()
    row = A.ROW["n17_nw257_first3_17"]
    a = (row.first, row.n_t, row.w0, row.nw)
    ds = _sampler(row)
    try:
        rc, whole = _raw_acf(ds, *a, 0, row.n_t)          # n_lags = n_t is accepted
        assert rc == 0
        _hold(row, whole)
        rc, f = _raw_acf(ds, *a, 0, row.n_t + 1)
        assert rc == -1 and np.all(f == -777.0)
        rc, f = _raw_acf(ds, *a, 16, 1)
        assert rc == 0 and np.array_equal(_bits(f), _bits(whole[16:17]))
    finally:
        ds.close()


# ---- 7. the pooled moments ------------------------------------------------------------------------------------------------
def _moments_hold(what, x, mean, var):
    m, v = A.pooled_moments(x)
    em, ev = A.pooled_bounds(x)
    qm = float(np.max(np.abs(mean - m.astype(np.float64)) / em))
    with np.errstate(invalid="ignore", divide="ignore"):
        dv = np.abs(var - v.astype(np.float64))
        qv = float(np.max(np.where(dv == 0.0, 0.0, dv / ev)))
    assert qm <= 1.0 and qv <= 1.0, f"{what}: err / bound of the mean {qm:.3g}, of the variance {qv:.3g}"
    return qm, qv


@pytest.mark.parametrize("kind", A.MOMENT_KINDS)
def test_marginal_moments_dev_within_the_bound(kind):
    import torch
    from gpemu import marginals as M
    dev = torch.device("cuda", 0)
    worst = (0.0, 0.0)
    for R in A.MOMENT_ROWS:
        for d in A.MOMENT_D:
            x = A.moment_rows(R, d, kind)
            t = torch.from_numpy(np.array(x)).to(dev)
            mean, var = M._moments_dev(0, t.data_ptr(), R, d)
            q = _moments_hold(f"{kind} R = {R} d = {d}", x, mean, var)
            worst = (max(worst[0], q[0]), max(worst[1], q[1]))
            if R == 1:
                assert np.all(var == 0.0)
    print(f"\npooled moments, {kind}: worst err / bound of the mean {worst[0]:.3g}, of the variance {worst[1]:.3g}")


def test_moments_of_constant_rows():
    """Constant rows: the bound of the variance is e_mu^2.  The code gives the square of its mean's rounding error --
    exactly 0 where the mean comes out exact, within the bound elsewhere."""
    import torch
    from gpemu import marginals as M
    exact = []
    for R in A.MOMENT_ROWS:
        x = np.full((R, 7), 0.1) * (1.0 + np.arange(7))
        t = torch.from_numpy(x).to(torch.device("cuda", 0))
        mean, var = M._moments_dev(0, t.data_ptr(), R, 7)
        em, ev = A.pooled_bounds(x)
        assert np.all(np.abs(mean - x[0]) <= em) and np.all(var <= ev) and np.all(var >= 0.0)
        exact.append((R, int(np.sum(var == 0.0))))
    print("\nconstant rows: parameters of 7 with variance exactly 0, per R:", exact)
    assert exact[0] == (1, 7)


# (W, steps) of the samplers whose stored chain has R = W * steps rows.  R = 1 cannot be had (a sampler has at least two
# walkers) and 257 * 1024 + 3 is prime: 513 * 513 = 257 * 1024 + 1 takes its place (257 partials, one strided add).
CHAIN_SHAPES = ((15, 17), (33, 31), (32, 32), (41, 25), (513, 513))


@pytest.mark.parametrize("d", A.MOMENT_D)
def test_chain_moments_within_the_bound(d):
    dm, lo, hi = _model(d)
    worst = {}
    for W, steps in CHAIN_SHAPES:
        ds = S.DeviceSampler([dm], W, seed=W)
        try:
            ds.set_state(_start(lo, hi, W, W))
            ds.run(steps)
            for kind in A.MOMENT_KINDS:
                x = A.moment_rows(W * steps, d, kind)
                _plant(ds, x.reshape(steps, W, d))
                q = _moments_hold(f"{kind} W = {W} steps = {steps} d = {d}", x, *ds.chain_moments())
                worst[kind] = tuple(max(a, b) for a, b in zip(worst.get(kind, (0.0, 0.0)), q))
            # a sub-range of the steps
            x = A.moment_rows(W * steps, d, "ar1").reshape(steps, W, d)
            _plant(ds, x)
            if steps > 3:
                _moments_hold("sub-range", x[2:steps - 1].reshape(-1, d), *ds.chain_moments(discard=2, n=steps - 3))
        finally:
            ds.close()
    print(f"\nchain moments d = {d}: worst err / bound (mean, variance) per data kind",
          {k: (f"{v[0]:.3g}", f"{v[1]:.3g}") for k, v in worst.items()})
