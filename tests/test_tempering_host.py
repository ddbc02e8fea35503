"""Host tests of parallel tempering: the ladder, the thermodynamic-integration evidence against quadrature, the CPU
tempered reference (tests/pt_ref.py) against the analytic tempered variances, and the new library symbols."""
import numpy as np
import pytest
from scipy import integrate, stats

import pt_ref

from gpemu import _lib
from gpemu.tempering import geometric_ladder, thermodynamic_integration_log_evidence


def test_geometric_ladder_endpoints_and_order():
    b = geometric_ladder(8, 1e4, prior_rung=True)
    assert b.shape == (8,) and b[0] == 1.0 and b[-1] == 0.0
    np.testing.assert_allclose(b[-2], 1e-4, rtol=1e-12)
    assert np.all(np.diff(b) < 0)
    b = geometric_ladder(8, 1e4, prior_rung=False)
    assert b.shape == (8,) and b[0] == 1.0
    np.testing.assert_allclose(b[-1], 1e-4, rtol=1e-12)
    np.testing.assert_allclose(b, 1e4 ** (-np.arange(8) / 7.0), rtol=1e-14)
    np.testing.assert_array_equal(geometric_ladder(2, 10.0), [1.0, 0.0])
    np.testing.assert_array_equal(geometric_ladder(4, 1.0, prior_rung=False), np.ones(4))


@pytest.mark.parametrize("args", [(1, 10.0), (65, 10.0), (2.5, 10.0), (True, 10.0), (4, 0.5), (4, np.inf),
                                  (4, np.nan)])
def test_geometric_ladder_rejects_bad_arguments(args):
    with pytest.raises(ValueError):
        geometric_ladder(*args)


# 1-D Gaussian likelihood N(y; theta, sigma^2), uniform prior on [-A, A]
Y, SIGMA, A = 0.2, 0.5, 1.0


def _loglik(theta):
    return -0.5 * ((Y - theta) / SIGMA) ** 2 - np.log(np.sqrt(2 * np.pi) * SIGMA)


def _mean_ll(beta):
    """<log L>_beta under p_beta ~ L^beta on the box, by quadrature."""
    w = lambda t: np.exp(beta * (_loglik(t) - _loglik(Y)))
    num = integrate.quad(lambda t: _loglik(t) * w(t), -A, A, points=[Y], limit=200)[0]
    den = integrate.quad(w, -A, A, points=[Y], limit=200)[0]
    return num / den


def _exact_log_z():
    return np.log((stats.norm.cdf((A - Y) / SIGMA) - stats.norm.cdf((-A - Y) / SIGMA)) / (2 * A))


def _ti(n_hot):
    betas = np.concatenate([geometric_ladder(n_hot, 100.0, prior_rung=False), [0.0]])      # n_hot rungs + beta = 0
    return thermodynamic_integration_log_evidence(betas, [_mean_ll(b) for b in betas])


def test_thermodynamic_integration_matches_closed_form():
    log_z, dlog_z = _ti(64)
    assert abs(log_z - _exact_log_z()) < 1e-3
    assert dlog_z < 1e-3
    # the error estimate shrinks as the ladder is refined
    errs = [_ti(n)[1] for n in (8, 16, 32, 64)]
    assert all(e1 < e0 for e0, e1 in zip(errs, errs[1:])), errs


def test_thermodynamic_integration_ordering_and_no_prior_rung():
    betas = np.array([1.0, 0.5, 0.1])
    logls = np.array([-1.0, -2.0, -5.0])
    z, dz = thermodynamic_integration_log_evidence(betas, logls)
    z2, dz2 = thermodynamic_integration_log_evidence(betas[::-1], logls[::-1])
    assert (z, dz) == (z2, dz2)
    # no beta = 0 rung: the hottest rung's mean stands in for it
    b = np.array([1.0, 0.5, 0.1, 0.0])
    l = np.array([-1.0, -2.0, -5.0, -5.0])
    assert z == pytest.approx(-np.sum(0.5 * (l[1:] + l[:-1]) * np.diff(b)), rel=1e-14)
    with pytest.raises(ValueError):
        thermodynamic_integration_log_evidence([1.0, 0.5], [1.0])


def test_pt_ref_rung_variances():
    """The CPU reference samples p_beta ~ N(y, sigma^2 / beta) on each rung (box wide enough not to truncate)."""
    sigma, y, box = 1.0, 0.0, 30.0
    betas = np.array([1.0, 0.5, 0.25, 0.25])

    def ll(q):
        q = np.atleast_2d(q)[:, 0]
        out = -0.5 * ((q - y) / sigma) ** 2
        return np.where((q > -box) & (q < box), out, -np.inf)

    T, Wc, steps, burn = betas.size, 64, 1500, 300
    rng = np.random.default_rng(5)
    X0 = rng.uniform(-3, 3, size=(T, Wc, 1))
    chain, lps, nacc, sacc, stry = pt_ref.run(X0, ll, betas, [11, 12, 13, 14], steps, swap_every=1)
    assert np.all(stry == steps) and np.all(sacc > 0)
    for t in range(T):
        x = chain[burn:, t, :, 0]
        var = x.var()
        # a few hundred independent samples per rung at tau ~ 10: a 25 % band is many standard errors wide
        assert abs(var / (sigma ** 2 / betas[t]) - 1.0) < 0.25, (t, var)
        np.testing.assert_allclose(lps[burn:, t], ll(x.reshape(-1, 1)).reshape(x.shape), rtol=1e-12)


def test_new_symbols_are_bound():
    names = set(_lib.exported_symbols())
    for s in ("gpemu_sampler_create_tempered", "gpemu_sampler_set_betas", "gpemu_sampler_get_swap_counts",
              "gpemu_sampler_mean_loglik"):
        assert s in names
