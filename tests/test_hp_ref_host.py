"""CPU: the extended-precision reference of tests/hp_ref.py and its error bound.

- the reference agrees with 40-digit mpmath arithmetic on small shapes;
- calibration: honest float64 arithmetic (the oracle) stays inside the bound on every shape of the GPU path sweep;
- sensitivity: a numpy restatement of the device's algorithm with one injected tile bug leaves the bound on every
  sweep shape, where the suite's old criterion (max |dev - oracle| < 1e-8 max |oracle|, rtol 1e-8 for the
  log-posterior) lets many of them through.  The counts are printed (pytest -s).
"""
import math

import mpmath
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import hp_ref as H
import matern_nu_ref as MR
import path_cases as PC
from oracle import gp_oracle as O

LD = np.longdouble


def _sweep():
    out = []
    for c in PC.cases():
        model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
        Xq, rep, cols = PC.queries(c, model, lo, hi, rng)
        out.append((c, model, lo, hi, y_exp, y_err, bs, Xq[cols], cols))
    return out


@pytest.fixture(scope="module")
def sweep():
    return _sweep()


def _ratio(err, bound):
    err = np.abs(np.asarray(err, dtype=np.float64))
    return np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))


# ---- against mpmath ------------------------------------------------------------------------------------------------------
def _mp(x):
    """a longdouble as an mpf, exactly (25 significant digits cover the 64-bit significand)"""
    return mpmath.mpf(np.format_float_scientific(LD(x), precision=25, unique=False))


def _mp_kernel(r, spec, const):
    if spec.kind == O.RBF:
        v = mpmath.exp(-r * r / 2)
    elif spec.nu == 0.5:
        v = mpmath.exp(-r)
    elif spec.nu == 1.5:
        t = r * mpmath.sqrt(3)
        v = (1 + t) * mpmath.exp(-t)
    elif spec.nu == 2.5:
        t = r * mpmath.sqrt(5)
        v = (1 + t + t * t / 3) * mpmath.exp(-t)
    else:
        nu = mpmath.mpf(spec.nu)
        t = mpmath.sqrt(2 * nu) * (r if r > 0 else mpmath.mpf(np.finfo(float).eps))
        v = 2 ** (1 - nu) / mpmath.gamma(nu) * t ** nu * mpmath.besselk(nu, t)
    return v + (const if spec.has_const else 0)


@pytest.mark.parametrize("N,d,kind,nu,const", [(7, 2, O.RBF, np.inf, False), (16, 3, O.MATERN, 0.5, True),
                                               (25, 1, O.MATERN, 1.5, False), (40, 4, O.MATERN, 2.5, True),
                                               (12, 2, O.MATERN, 2.0, False)])
def test_reference_agrees_with_mpmath(N, d, kind, nu, const):
    c = PC.Case("mp", N, d, 2, 6, kind, nu, const)
    model, lo, hi, _, _, _, rng = PC.problem(c)
    Xq = np.vstack([model.X_train[0], model.X_train[N - 1] + 1e-7, rng.uniform(lo, hi, (4, d))])
    gp = model.gps[0]
    pc = H.PCRef(Xq, model.X_train, gp, model.spec)
    mpmath.mp.dps = 40
    Lm = mpmath.matrix(gp.L.tolist())
    # the Bessel part is scipy's in float64 for general nu (hp_ref docstring): 1e-14 there, 1e-16 elsewhere
    tol = 1e-14 if c.general_nu else 1e-16
    for b in range(Xq.shape[0]):
        ks = []
        for j in range(N):
            r = mpmath.sqrt(mpmath.fsum(((mpmath.mpf(float(Xq[b, i])) - mpmath.mpf(float(model.X_train[j, i])))
                                         / mpmath.mpf(float(gp.ls[i]))) ** 2 for i in range(d)))
            ks.append(_mp_kernel(r, model.spec, mpmath.mpf(gp.const)))
        mean = mpmath.fsum(kj * mpmath.mpf(float(a)) for kj, a in zip(ks, gp.alpha))
        V = mpmath.lu_solve(Lm, mpmath.matrix(ks))
        var = mpmath.mpf(pc.kdiag) - mpmath.fsum(v * v for v in V)
        scale_m = float(mpmath.fsum(abs(kj * mpmath.mpf(float(a))) for kj, a in zip(ks, gp.alpha)))
        k_err = max(abs(float(ks[j] - _mp(pc.K[b, j])) / max(float(ks[j]), 1e-300)) for j in range(N))
        assert k_err < tol, (b, k_err)
        assert abs(float(mean - _mp(pc.mean[b]))) < tol * scale_m
        assert abs(float(var - _mp(pc.var_raw[b]))) < tol * pc.kdiag


# ---- calibration: float64 arithmetic stays inside the bound ------------------------------------------------------------
def test_oracle_inside_the_bound(sweep):
    worst = {}
    for c, model, lo, hi, y_exp, y_err, bs, X, cols in sweep:
        mean, var, mb, vb, _ = pred = H.gp_predict(X, model)
        with MR.general_nu():
            mo, vo = O.gp_predict_all(X, model)
        rm, rv = _ratio(mo - np.asarray(mean, float), mb), _ratio(vo - np.asarray(var, float), vb)
        lp, lb, _ = H.log_posterior(X, model, lo, hi, y_exp, y_err, bs, pred=pred)
        if c.nblk == 1:
            with MR.general_nu():
                lpo = np.array([O.log_posterior(X[i], {"g": model}, lo, hi, y_exp, y_err)[0] for i in range(len(X))])
        else:
            st = O.lowrank_setup_blocks(model, y_exp, y_err, bs)
            lpo = np.array([O.loglik_lowrank_blocks(mo[i], vo[i], st) for i in range(len(X))])
            lpo[~np.all((X > lo) & (X < hi), axis=1)] = -np.inf
        assert np.array_equal(np.isfinite(lpo), np.isfinite(np.asarray(lp, float))), c.name
        ins = np.isfinite(lpo)
        rl = _ratio(lpo[ins] - np.asarray(lp, float)[ins], lb[ins])
        worst[c.name] = (rm.max(), rv.max(), rl.max() if rl.size else 0.0)
        assert rm.max() <= 1 and rv.max() <= 1 and (rl.size == 0 or rl.max() <= 1), (c.name, worst[c.name])
    print("\nerr / bound of the float64 oracle (mean, var, lp):")
    for n, w in worst.items():
        print(f"  {n:28s} {w[0]:.2e} {w[1]:.2e} {w[2]:.2e}")


# ---- sensitivity: injected tile bugs -------------------------------------------------------------------------------------
def _device_restatement(model, X, ref_pcs):
    """float64 restatement of the device's predict: W = L^-1 once, V = W K_*^T, var = kdiag - sum V^2"""
    out = []
    for gp, pc in zip(model.gps, ref_pcs):
        K = np.asarray(pc.K, dtype=np.float64)
        W = solve_triangular(gp.L, np.eye(gp.L.shape[0]), lower=True, check_finite=False)
        out.append((K, W, pc.kdiag))
    return out


def _var_of(Vs, kds):
    return np.stack([np.maximum(kd - np.sum(V * V, axis=0), 0.0) for V, kd in zip(Vs, kds)], axis=1)


def test_bound_flags_every_injected_bug(sweep):
    caught, old_missed, total = {}, {}, {}

    def record(bug, flagged, old_ok):
        total[bug] = total.get(bug, 0) + 1
        caught[bug] = caught.get(bug, 0) + int(flagged)
        old_missed[bug] = old_missed.get(bug, 0) + int(old_ok)

    failures = []
    for c, model, lo, hi, y_exp, y_err, bs, X, cols in sweep:
        mean, var, mb, vb, pcs = pred = H.gp_predict(X, model)
        var64 = np.asarray(var, dtype=np.float64)
        parts = _device_restatement(model, X, pcs)
        Vs = [W @ K.T for K, W, _ in parts]
        kds = [kd for _, _, kd in parts]

        def check_var(bug, Vb):
            vbug = _var_of(Vb, kds)
            flagged = bool(np.any(np.abs(vbug - var64) > vb))
            old_ok = bool(np.max(np.abs(vbug - var64)) < 1e-8 * max(np.max(np.abs(var64)), 1e-300))
            record(bug, flagged, old_ok)
            if not flagged:
                failures.append((c.name, bug))

        N = c.N
        for r in sorted({r for r in PC.EDGE_ROWS if r < N} | {N - 1}):
            Vb = [V.copy() for V in Vs]
            for V in Vb:
                V[r] = 0.0
            check_var(f"drop V row {'N-1' if r == N - 1 else r}", Vb)
        for cc in sorted({x for x in PC.EDGE_COLS if x < c.B} | {c.B - 1}):
            j = int(np.searchsorted(cols, cc))
            if j == len(cols) or cols[j] != cc or cc == 0:
                continue
            Vb = [V.copy() for V in Vs]
            for V in Vb:
                V[:, j] = 0.0
            check_var(f"drop query column {'B-1' if cc == c.B - 1 else cc}", Vb)
        j0 = (N - 1) // 32 * 32
        Vb = []
        for (K, W, _), V in zip(parts, Vs):
            V2 = V.copy()
            V2[j0:] = W[j0:, :j0] @ K[:, :j0].T
            Vb.append(V2)
        check_var("omit the last partial K-tile", Vb)

        if c.nblk > 1:
            setups = H.lowrank_setup_blocks(model, y_exp, y_err, bs)
            inside = np.all((X > lo) & (X < hi), axis=1)
            lp, lb, _ = H.log_posterior(X, model, lo, hi, y_exp, y_err, bs, pred=pred)
            lp64 = np.asarray(lp, float)
            for bug, st in (("block o uses block o+1's constants", [setups[1]] + setups[1:]),
                            ("drop one observable block", setups[1:])):
                lpb, _, _, _ = H.loglik_blocks(mean, var, st)
                lpb = np.asarray(lpb, float)
                d = np.abs(lpb[inside] - lp64[inside])
                flagged = bool(np.any(d > lb[inside]))
                old_ok = bool(np.all(d < 1e-8 * np.abs(lp64[inside])))
                record(bug, flagged, old_ok)
                if not flagged:
                    failures.append((c.name, bug))
    print("\ninjected bug: shapes / caught by the bound / missed by the old 1e-8 criterion")
    for bug in total:
        print(f"  {bug:40s} {total[bug]:3d} {caught[bug]:3d} {old_missed[bug]:3d}")
    assert not failures, failures
