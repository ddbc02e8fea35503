"""CPU: the extended-precision reference of tests/hp_ref.py and its error bound.

- the reference agrees with 40-digit mpmath arithmetic on small shapes;
- calibration: honest float64 arithmetic (the oracle) stays inside the bound on every shape of the GPU path sweep;
- sensitivity: a numpy restatement of the device's algorithm with one injected tile bug leaves the bound on every
  sweep shape, where the suite's old criterion (max |dev - oracle| < 1e-8 max |oracle|, rtol 1e-8 for the
  log-posterior) lets many of them through.  The counts are printed (pytest -s);
- the distance factors are 8 for d <= 8; the wide cases (9 .. 16 parameters) cover their paths with every special
  placed, and every injected 16-wide bug (a sum over 8 coordinates, a wide coordinate read with the 8-wide stride or
  length scale, a box check of lanes 0 .. 7) leaves the bound on a wide shape; which of them test_gpu_wide_d.py's
  tolerances let through is printed.
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
        mean, var, mb, vb, _ = pred = H.gp_predict(X, model, input_rounding=c.ls_bounds)
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
        mean, var, mb, vb, pcs = pred = H.gp_predict(X, model, input_rounding=c.ls_bounds)
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


# ---- 9 .. 16 parameters ----------------------------------------------------------------------------------------------------
WIDE = [c for c in PC.cases() if c.d > PC.DPAD]


def test_distance_factors():
    """the d-dependent distance factors: exactly the 8-wide constant for d <= 8 (every existing bound unchanged), and
    what the longer sums of the 16-wide instances need"""
    for d in range(1, PC.DPAD + 1):
        assert H.c_x(d) == H.c_x_direct(d) == H.C_X8 == 8.0, d
    assert [H.kstar_ksteps(d) for d in (7, 8, 9, 11, 12, 15, 16)] == [2, 3, 3, 3, 4, 4, 5]
    assert [H.c_x(d) for d in (9, 11, 12, 15, 16)] == [8 * 10 / 9, 8 * 12 / 9, 8 * 13 / 9, 8 * 16 / 9, 8 * 17 / 9]
    assert [H.c_x_direct(d) for d in (9, 12, 16)] == [9.0, 12.0, 16.0]
    # test_gpu_predict_cov's references at d = 9, 10 and 16 pin the 8-wide factor: their bounds do not grow
    c = PC.Case("f", 20, 16, 1, 4, O.MATERN, 0.5, False)
    model, lo, hi, _, _, _, rng = PC.problem(c)
    X = np.vstack([model.X_train[:2] + 1e-9, rng.uniform(lo, hi, (2, 16))])
    gp = model.gps[0]
    k8, dk8 = H.kstar(X, model.X_train, gp, model.spec, cx=H.C_X8)
    k, dk = H.kstar(X, model.X_train, gp, model.spec)
    assert np.array_equal(k, k8) and np.all(dk >= dk8) and np.any(dk > dk8)


def test_wide_cases_cover_their_paths_and_place_every_special():
    """the wide cases take every path the sweep is there for, at every wide k-step count, on shapes that do not depend
    on the CU count; queries() places all of their specials (the box-edge walkers of coordinates 8 .. 15 included)"""
    paths, wide = set(), set()
    for c in WIDE:
        n, free = PC.special_count(c)
        assert n <= free, f"{c.name}: {n} specials for {free} free columns"
        paths |= PC.predict_paths(c, 256) | PC.logpost_paths(c, 256)
        wide |= {p for p, v in PC.wide_paths(c).items() if v}
        assert PC.wide_paths(c)["KSTAR_KSTEPS2"] == PC.wide_paths(c)["KSTAR_KSTEPS3"] == 0
        model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
        Xq, rep, cols = PC.queries(c, model, lo, hi, rng)
        mid = 0.5 * (lo + hi)
        for j in range(c.d):
            on = (Xq[cols, j] == (lo[j] if j % 2 == 0 else hi[j])) & np.all(np.delete(Xq[cols] == mid, j, axis=1), axis=1)
            assert on.any(), f"{c.name}: no box-edge walker on coordinate {j}"
    assert {"WIDE_KSTAR_KSTEPS3", "WIDE_KSTAR_KSTEPS4", "WIDE_KSTAR_KSTEPS5"} <= wide
    # what the CU count can change is the set of paths (TRMM_*_XCD / _LPT / _FEW_ITEMS): the paths the wide cases are
    # there for are taken at the MI355X's count and at others alike
    need = {"KSTAR_SMALL", "KSTAR_BIG", "KSTAR_DIRECT", "LOGLIK_LOWRANK", "LOGLIK_TASKS_ONE", "LOGLIK_TASKS_MULTI",
            "LOGLIK_TASKS_MULTI_BIG", "TRMM_DMA_WHOLE", "TRMM_DMA_PIECES", "PREDICT_PASS"}
    for ncu in (256, 304, 80, 8):
        got = set().union(*(PC.predict_paths(c, ncu) | PC.logpost_paths(c, ncu) for c in WIDE))
        assert need <= got, (ncu, need - got)
        assert any(p.startswith("TRMM_SMALL") for p in got) and any(p.startswith("TRMM_DMA") for p in got), ncu
    assert any(c.kind == O.MATERN and c.nu == 0.5 for c in WIDE)
    assert any(c.general_nu and c.nu < 1 for c in WIDE)
    assert any(c.kind == O.RBF and c.const for c in WIDE)
    assert any(c.B > PC.MAX_CHUNK for c in WIDE)


OLD_WIDE_D = (9, 10, 12, 15, 16)     # the parameter counts of test_gpu_wide_d.py's CASES


def _old_wide_box_catches(d):
    """for the printout only: whether test_gpu_wide_d.py's queries (B = 100 and 300, every 7th row outside the box on
    ONE random coordinate, seed B + d, N = 200) put that coordinate on a lane >= 8, the only way they can see a box
    check of lanes 0 .. 7.  It replays that file's RNG calls and goes stale if they change; None at a d it has no
    case for"""
    if d not in OLD_WIDE_D:
        return None
    out = False
    for B in (100, 300):
        rng = np.random.default_rng(B + d)
        rng.uniform(np.zeros(d), np.ones(d), (B, d))
        rng.integers(0, 200, len(range(1, B, 5)))
        out |= int(rng.integers(0, d)) >= 8
    return out


def _k64(Xq, X_train, ls, spec, const, bug=None):
    """float64 K_* from the coordinates (honest arithmetic), or with one injected 16-wide bug"""
    d = Xq.shape[1]
    q = Xq.copy()
    if bug == "query rows read with the 8-wide stride":
        pad = np.zeros((len(Xq) + 1, 16))
        pad[:len(Xq), :d] = Xq
        flat = pad.ravel()
        q = np.stack([flat[8 * b: 8 * b + d] for b in range(len(Xq))])
    lq, lx = np.array(ls, dtype=float), np.array(ls, dtype=float)
    if bug == "coordinate j >= 8 scaled by ls[j - 8]":
        lq[8:] = lx[8:] = ls[:d - 8]
    diff = q[:, None, :] / lq - X_train[None, :, :] / lx
    r2 = np.sum(diff * diff, axis=2)
    r2_8 = np.sum(diff[:, :, :8] ** 2, axis=2)
    if bug == "r2 over coordinates 0..7 (expanded form)":
        r2 = r2_8
    if bug == "direct distance over coordinates 0..7" and H._is_direct(spec):
        u = X_train / ls
        cen = 0.5 * (u.min(axis=0) + u.max(axis=0))
        nq = np.sum((Xq / ls - cen) ** 2, axis=1)
        r2 = np.where(r2 < 1e-7 * (nq[:, None] + 1.0), r2_8, r2)
    return H._base64(r2, spec) + (const if spec.has_const else 0.0)


def _fma(a, b, c):
    """one rounding of a * b + c (the product and sum in longdouble, then rounded to float64)"""
    return np.asarray(np.asarray(a, LD) * np.asarray(b, LD) + np.asarray(c, LD), dtype=np.float64)


def _kstar_expanded(Xq, X_train, gp, spec):
    """float64 restatement of the device's base kernel values (kstar_host.h: build_kstar_operands; predict_dev.h:
    kstar_mfma_block, kstar_value4): centred, scaled operands, the product as a chain of one rounding per product-add
    in slot order, |q'|^2 by lane chains and two cross-lane adds, r^2 = fma(acc, -2, |q'|^2) (the RBF's exponent
    acc - 1/2 |q'|^2 in units of ln 2 / 2^TB), the direct distance for the near pairs of nu < 1; the kernel of that
    r^2 in longdouble (the evaluation's own error is the bound's EPS term)"""
    d = X_train.shape[1]
    ls = np.asarray(gp.ls, dtype=np.float64)
    ks = H.kstar_ksteps(d)
    rbf = spec.kind == O.RBF or np.isinf(spec.nu)
    s = math.sqrt(64 / 0.6931471805599453) if rbf else 1.0          # KSTAR_TB = 6
    u = X_train / ls
    cen = 0.5 * (u.min(axis=0) + u.max(axis=0))
    v = _fma(Xq, s / ls, -s * cen)
    xa = (u - cen) * s
    aug = np.asarray(-0.5 * np.sum(xa.astype(LD) ** 2, axis=1), dtype=np.float64)
    acc = np.zeros((len(Xq), len(X_train)))
    for i in range(d):
        acc = _fma(v[:, i][:, None], xa[:, i][None, :], acc)
    acc = acc + aug[None, :]
    parts = []
    for lq in range(4):
        p = np.zeros(len(Xq))
        for st in range(ks):
            if 4 * st + lq < d:
                p = _fma(v[:, 4 * st + lq], v[:, 4 * st + lq], p)
        parts.append(p)
    part = (parts[0] + parts[1]) + (parts[2] + parts[3])
    if rbf:
        return np.exp(np.asarray(acc + (-0.5 * part)[:, None], dtype=LD) * (LD(0.6931471805599453) / 64))
    r2 = np.maximum(_fma(acc, -2.0, part[:, None]), 0.0)
    if spec.nu < 1.0:
        near = r2 < 1e-7 * (part[:, None] + 1.0)
        r2d = np.zeros_like(r2)
        for i in range(d):
            df = _fma(Xq[:, i][:, None], 1.0 / ls[i], -(X_train[:, i] / ls[i])[None, :])
            r2d = _fma(df, df, r2d)
        r2 = np.where(near, r2d, r2)
    return H._base_ld(np.asarray(r2, dtype=LD), spec)


def test_expanded_form_restatement_inside_the_bound(sweep):
    """the device's expanded form, restated (_kstar_expanded), stays within dk per K_* entry on every wide shape; the
    largest err/dk of every shape is printed (the 8-wide ones for comparison: their factor C_X8 is not changed here)"""
    print("\nexpanded-form restatement: largest K_* err / dk")
    for c, model, lo, hi, y_exp, y_err, bs, X, cols in sweep:
        worst = 0.0
        for gp in model.gps:
            K, dk = H.kstar(X, model.X_train, gp, model.spec, input_rounding=c.ls_bounds)
            base = K - (LD(gp.const) if model.spec.has_const else LD(0))
            worst = max(worst, _ratio(np.asarray(_kstar_expanded(X, model.X_train, gp, model.spec) - base), dk).max())
        print(f"  {c.name:36s} d = {c.d:2d}  {worst:.3g}")
        if c.d > PC.DPAD:
            assert worst <= 1.0, (c.name, worst)


WIDE_BUGS = {   # injected bug -> the wide shapes it applies to
    "r2 over coordinates 0..7 (expanded form)": lambda c: True,
    "direct distance over coordinates 0..7": lambda c: c.kind == O.MATERN and c.nu < 1.0,
    "coordinate j >= 8 scaled by ls[j - 8]": lambda c: True,
    "query rows read with the 8-wide stride": lambda c: True,
    "box check on lanes 0..7 only": lambda c: True,
}


def test_bound_flags_every_wide_bug(sweep):
    """on the wide shapes: the float64 restatement (K_* from the coordinates, W = L^-1, V = W K_*^T) stays inside the
    bound, and every injected 16-wide bug leaves it on at least one shape; the old criterion of test_gpu_wide_d.py
    (mean 1e-8 max(1, max|mean|), var 1e-8, log-posterior rtol 1e-8 with its own queries) is printed beside it"""
    rows = {}
    for c, model, lo, hi, y_exp, y_err, bs, X, cols in sweep:
        if c.d <= PC.DPAD:
            continue
        mean, var, mb, vb, pcs = pred = H.gp_predict(X, model, input_rounding=c.ls_bounds)
        lp, lb, setups = H.log_posterior(X, model, lo, hi, y_exp, y_err, bs, pred=pred)
        m64, v64 = np.asarray(mean, float), np.asarray(var, float)

        def predict(bug):
            ms, vs = [], []
            for gp, pc in zip(model.gps, pcs):
                K = _k64(X, model.X_train, gp.ls, model.spec, gp.const, bug)
                W = solve_triangular(gp.L, np.eye(gp.L.shape[0]), lower=True, check_finite=False)
                V = W @ K.T
                ms.append(K @ gp.alpha)
                vs.append(np.maximum(pc.kdiag - np.sum(V * V, axis=0), 0.0))
            return np.stack(ms, axis=1), np.stack(vs, axis=1)

        m0, v0 = predict(None)
        assert np.all(_ratio(m0 - m64, mb) <= 1) and np.all(_ratio(v0 - v64, vb) <= 1), c.name
        for bug, applies in WIDE_BUGS.items():
            if not applies(c):
                continue
            if bug == "box check on lanes 0..7 only":
                inside = np.all((X > lo) & (X < hi), axis=1)
                flagged = bool(np.any(np.all((X[:, :8] > lo[:8]) & (X[:, :8] < hi[:8]), axis=1) != inside))
                old = _old_wide_box_catches(c.d)
                if old is None:
                    continue
                old_ok = not old
            else:
                mbug, vbug = predict(bug)
                flagged = bool(np.any(np.abs(mbug - m64) > mb) or np.any(np.abs(vbug - v64) > vb))
                old_ok = bool(np.max(np.abs(mbug - m64)) < 1e-8 * max(1.0, np.max(np.abs(m64)))
                              and np.max(np.abs(vbug - v64)) < 1e-8)
            r = rows.setdefault(bug, [0, 0, 0, []])
            r[0] += 1
            r[1] += int(flagged)
            r[2] += int(old_ok)
            if flagged and old_ok:
                r[3].append(c.name)
    print("\nwide injected bug: shapes / caught by the bound / let through by test_gpu_wide_d.py's tolerances")
    for bug, (n, caught, old, names) in rows.items():
        print(f"  {bug:42s} {n:3d} {caught:3d} {old:3d}  {names}")
    assert set(rows) == set(WIDE_BUGS)
    assert all(r[1] > 0 for r in rows.values()), {b: r[:3] for b, r in rows.items()}
