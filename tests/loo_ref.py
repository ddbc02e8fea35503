"""Reference of the per-observable log-likelihood terms, PSIS-LOO, WAIC and the weighted parameter moments (tests only,
CPU, numpy / scipy): the specification of DESIGN.md 4.31 step by step in ``np.longdouble``, with an a-priori bound of
the device's float64 algorithm beside every quantity.

Terms.  ``terms`` takes hp_ref's extended-precision predict and, one observable block at a time, hp_ref's
``lowrank_setup_blocks`` / ``loglik_blocks`` / ``loglik_bound``: T[o][s] and its bound for that block alone.

PSIS of one row V (float64).  ``x = (-V) - max(-V)`` is formed in float64 -- one rounding, the same on the device: x IS
the data of the smoothing, so the tail, the cutoff and the ties are exact (integers / bits).  Everything after is
longdouble:
    M = ceil(min(S/5, 3 sqrt(S/r_eff))), x_c = max(x_(max(S-M-1, 0)), log DBL_MIN), tail = {x > x_c}, n of them;
    n <= 4: k-hat = inf, raw weights;
    t_i = exp(x_(i)) - exp(x_c); m = 30 + floor(sqrt(n)); b_j = (1 - sqrt(m/(j - 1/2)))/(3 t_[floor(n/4 + 1/2)]) + 1/t_[n];
    k_j = mean log1p(-b_j t_i); L_j = n (log(-b_j/k_j) - k_j - 1); w_j = 1/sum_i exp(L_i - L_j); weights below 10 eps
    dropped, the rest renormalised; b-bar = sum w_j b_j; k = mean log1p(-b-bar t_i); sigma = -k/b-bar;
    k-hat = (n k + 5)/(n + 10);
    tail element i: min(0, log(exp(x_c) + sigma expm1(-k-hat log1p(-p_i))/k-hat)), p_i = (i + 1/2)/n (k-hat = 0: the
    limit -sigma log1p(-p_i)); tied raw values share the mean of their positions' values; log-sum-exp normalisation.

Bounds.  ``u = 2^-53``.  The same sums over absolute values times ``C u``; ``EPS_FN = 4 u`` per exp / log / log1p / expm1;
first-order propagation L_j -> w_j -> b-bar -> k-hat -> smoothed tail -> log-sum-exp, every derivative analytic:
    dt_i = EPS_FN (exp(x_i) + exp(x_c)) + u t_i
    db_j, dk_j, dL_j from the formulas above, term by term
    w = softmax(L):  dw_j = w_j (sum_i w_i (dL_i + dL_j + u |L_i - L_j| + EPS_FN) + C u)
    the cut at 10 eps: a weight near the threshold may be kept on one side and dropped on the other; it moves b-bar by
    at most m 10 eps max|b_j| (and the renormalisation by as much again), added to db-bar: no branch needs excluding
    the smoothed value in log space (nothing overflows): log q_i = log sigma - log k-hat + log|expm1(z_i)|, z_i =
    -k-hat l_i, d log|expm1(z)|/dz = -1/expm1(-z); d log(exp(x_c) + q)/d log q = q/(exp(x_c) + q); a value that stays
    above 0 by more than its error is truncated to exactly 0 on both sides: bound 0.  Every bound is finite.
    a log-sum-exp moves by at most the weighted mean of its terms' errors, plus the sum's own (C_S u + EPS_FN) and the
    logarithm's.
A sum over n samples in the device's tree (16 serial adds per lane, a 6-level butterfly, 4 waves, the chunks of 4096 in
order) has depth 16 + 6 + 3 + ceil(n/4096): ``c_sum(n) = C + ceil(n/4096)`` with hp_ref's ``C = 64``.  A serial sum of
L tied positions: ``max(C, L) u``.  Constants are fixed here, once."""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "tests/loo_ref.py needs an extended np.longdouble (x87 80-bit or better)"

U = 2.0 ** -53
C = 64.0
EPS_FN = 4 * U
CUT = 10 * 2.0 ** -52
LOG_TINY = float(np.log(np.finfo(np.float64).tiny))
SUM_CHUNK = 4096


def c_sum(n):
    return C + math.ceil(n / SUM_CHUNK)


# ---- terms -----------------------------------------------------------------------------------------------------------
def setup_blocks(model, y_exp, y_err, block_start, n_div=1.0, cov=None):
    """hp_ref.lowrank_setup_blocks; a dense within-observable data covariance ``cov`` replaces diag(y_err^2)"""
    import hp_ref as H
    from oracle import gp_oracle as O
    if cov is None:
        return H.lowrank_setup_blocks(model, y_exp, y_err, block_start, n_div)
    s = model.scaler_scale.astype(LD)
    cun = O.cov_unexplained(model).astype(LD) + np.asarray(cov, dtype=LD) * LD(n_div) / np.outer(s, s)
    return H.lowrank_setup_blocks(model, y_exp, np.zeros_like(y_err), block_start, n_div, cov_unexpl=cun)


def terms(model, X, y_exp, y_err, block_start, n_div=1.0, cov=None, pred=None):
    """(T [n_obs, S] longdouble, bound [n_obs, S] float64): every block's term by hp_ref on that block's setup alone.
    No prior box.  pred: hp_ref.gp_predict(X, model) if at hand"""
    import hp_ref as H
    mean, var, mb, vb, _ = pred if pred is not None else H.gp_predict(np.asarray(X, dtype=np.float64), model)
    setups = setup_blocks(model, y_exp, y_err, block_start, n_div, cov)
    T, B = [], []
    for st in setups:
        lp, _, _, _ = H.loglik_blocks(mean, var, [st])
        T.append(lp)
        B.append(H.loglik_bound(mean, var, mb, vb, [st]))
    return np.stack(T), np.stack(B)


# ---- the generalised Pareto fit -----------------------------------------------------------------------------------------
def gpdfit(t, dt=None):
    """Zhang & Stephens (2009) as ArviZ's _gpdfit restates it, on the ascending tail t (longdouble): (k-hat, sigma) and,
    with dt (the bound of t's error, float64), (dk-hat, dsigma)."""
    t = np.asarray(t, dtype=LD)
    n = t.size
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1, dtype=LD)
    iq = int(n / 4.0 + 0.5) - 1
    cj = 1 - np.sqrt(LD(m) / (j - LD(0.5)))
    b = cj / (3 * t[iq]) + 1 / t[-1]
    a = -b[:, None] * t[None, :]                       # [m, n]
    lt = np.log1p(a)
    k = lt.mean(axis=1)
    L = n * (np.log(-(b / k)) - k - 1)
    with np.errstate(over="ignore"):
        w = 1 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
    keep = w >= CUT
    wk = np.where(keep, w, 0)
    tot = wk.sum()
    wn = wk / tot
    bbar = np.sum(wn * b)
    lb = np.log1p(-bbar * t)
    kk = lb.mean()
    sigma = -kk / bbar
    khat = (n * kk + 5) / (n + 10)
    if dt is None:
        return khat, sigma
    f = lambda v: np.asarray(v, dtype=np.float64)
    dt = f(dt)
    tf, bf, kf, Lf, wf, wnf = f(t), f(b), f(k), f(L), f(w), f(wn)
    cs = c_sum(n)
    db = np.abs(f(cj)) / (3 * tf[iq]) * (dt[iq] / tf[iq] + 4 * U) + (1 / tf[-1]) * (dt[-1] / tf[-1] + 2 * U) + U * np.abs(bf)
    af = f(a)
    da = np.abs(bf)[:, None] * dt[None, :] + tf[None, :] * db[:, None] + U * np.abs(af)
    dterm = da / (1 + af) + EPS_FN * np.abs(f(lt))
    dk = (dterm.sum(axis=1) + cs * U * np.abs(f(lt)).sum(axis=1)) / n + U * np.abs(kf)
    lg = np.abs(f(np.log(-(b / k))))
    dL = n * (db / np.abs(bf) + dk / np.abs(kf) + 2 * U + EPS_FN * lg + dk + 3 * U * (lg + np.abs(kf) + 1)) + U * np.abs(Lf)
    with np.errstate(over="ignore", invalid="ignore"):
        sm = np.where(np.isfinite(wf), wf, 0.0)
        sm = sm / sm.sum()
        dLij = dL[None, :] + dL[:, None] + U * np.abs(Lf[None, :] - Lf[:, None]) + EPS_FN
        E = np.sum(sm[None, :] * np.where(sm[None, :] > 0, dLij, 0.0), axis=1)
    dw = wf * (E + (C + m) * U)
    totf = float(tot)
    dwk = np.where(f(keep) > 0, dw, 0.0)
    dwn = (dwk + wnf * dwk.sum()) / totf + (m + 2) * U * wnf
    cut = m * CUT * np.max(np.abs(bf))
    dbbar = np.sum(dwn * np.abs(bf) + wnf * db) + (m + 1) * U * np.sum(wnf * np.abs(bf)) + 2 * cut
    bb = float(bbar)
    ab = -bb * tf
    dab = abs(bb) * dt + tf * dbbar + U * np.abs(ab)
    dtb = dab / (1 + ab) + EPS_FN * np.abs(f(lb))
    dkk = (dtb.sum() + cs * U * np.abs(f(lb)).sum()) / n + U * abs(float(kk))
    dsigma = abs(float(sigma)) * (dkk / abs(float(kk)) + dbbar / abs(bb) + 2 * U)
    dkhat = n * dkk / (n + 10) + 4 * U * (abs(float(khat)) + 1)
    return khat, sigma, dkhat, dsigma


def gpinv(p, khat, sigma):
    """the quantile function of the fitted distribution at p (longdouble)"""
    l1 = np.log1p(-np.asarray(p, dtype=LD))
    if khat == 0:
        return -sigma * l1
    return sigma * np.expm1(-khat * l1) / khat


def gpd_quantile_sample(n, k, sigma=1.0):
    """exact quantile samples t_i = sigma expm1(-k log1p(-p_i))/k, p_i = (i + 1/2)/n, ascending (longdouble)"""
    p = (np.arange(n, dtype=LD) + LD(0.5)) / n
    return gpinv(p, LD(k), LD(sigma))


def tail_size(S, r_eff=1.0):
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / r_eff))))


# ---- PSIS / WAIC of one row ----------------------------------------------------------------------------------------------
def _lse(e, de):
    """(log-sum-exp of e (longdouble), its bound): the weighted mean of de and of the exponent's rounding, the sum's
    C_S u + EPS_FN, the logarithm's EPS_FN and the final addition"""
    mx = e.max()
    ex = np.exp(e - mx)
    A = ex.sum()
    val = mx + np.log(A)
    p = np.asarray(ex / A, dtype=np.float64)
    ef = np.asarray(e, dtype=np.float64)
    d = _wsum(p, de + U * np.abs(ef - float(mx))) + c_sum(e.size) * U + EPS_FN \
        + EPS_FN * abs(float(np.log(A))) + U * (abs(float(mx)) + abs(float(val)))
    return val, d


def _wsum(p, de):
    """sum p de over the elements of non-zero weight (a bound may be infinite where a smoothed quantile overflows)"""
    with np.errstate(invalid="ignore"):
        return float(np.sum(np.where(p > 0, p * de, 0.0)))


def psis_row(V, r_eff=1.0):
    """dict of the row's statistics (longdouble / ints; ``logw`` [S] in the input's order) and ``bound``, a dict of
    float64 bounds under the same names.  A row with a NaN: every statistic NaN, n_tail = -1."""
    V = np.asarray(V, dtype=np.float64)
    S = V.size
    nanv = LD(np.nan)
    if not np.isfinite(V).all():                        # a NaN or an infinity: x = min(V) - V is undefined
        out = {k: nanv for k in ("elpd_loo", "lppd", "p_loo", "pareto_k", "ess_w", "p_waic", "elpd_waic", "cutoff")}
        out.update(n_tail=-1, logw=np.full(S, np.nan, dtype=LD), bound=None)
        return out
    x = (-V) - np.max(-V)                               # float64: the data of the smoothing
    M = tail_size(S, r_eff)
    xs = np.sort(x)
    xc = max(float(xs[max(S - M - 1, 0)]), LOG_TINY)
    tail = x > xc
    n = int(tail.sum())
    lw = x.astype(LD)
    dlw = np.zeros(S)
    khat, dkhat = LD(np.inf), 0.0
    if n > 4:
        idx = np.where(tail)[0]
        order = np.argsort(x[idx], kind="stable")
        xt = x[idx][order]
        exc = np.exp(LD(xc))
        ex = np.exp(xt.astype(LD))
        t = ex - exc
        dt = EPS_FN * np.asarray(ex + exc, dtype=np.float64) + U * np.asarray(t, dtype=np.float64)
        khat, sigma, dkhat, dsigma = gpdfit(t, dt)
        p = (np.arange(n, dtype=LD) + LD(0.5)) / n
        q = gpinv(p, khat, sigma)
        sm = np.log(exc + q)
        # the bound of the smoothed values
        kf, sf = float(khat), float(sigma)
        pf = np.asarray(p, dtype=np.float64)
        l1 = np.log1p(-pf)
        dl = 2 * U * pf / (1 - pf) + EPS_FN * np.abs(l1)
        if kf == 0.0:
            qf = np.asarray(q, dtype=np.float64)
            dq = np.abs(qf) * (dsigma / abs(sf) + 2 * U) + abs(sf) * dl + 0.5 * abs(sf) * l1 * l1 * dkhat
            share = np.asarray(q / (exc + q), dtype=np.float64)
            dsm = share * dq / np.abs(qf) + (1 - share) * EPS_FN + 2 * U + EPS_FN * np.abs(np.asarray(sm, dtype=np.float64))
        else:
            # in log space, so that nothing overflows: log q = log sigma - log k-hat + log |expm1(z)|, z = -k-hat l;
            # d log|expm1(z)| / dz = e^z / (e^z - 1) = -1 / expm1(-z)
            z = -kf * l1
            dz = np.abs(l1) * dkhat + abs(kf) * dl + U * np.abs(z)
            dlogq = dsigma / abs(sf) + dkhat / abs(kf) + np.abs(1 / np.expm1(-z)) * dz + EPS_FN + 4 * U
            share = np.asarray(q / (exc + q), dtype=np.float64)          # d log(exc + q) / d log q
            dsm = share * dlogq + (1 - share) * EPS_FN + 2 * U + EPS_FN * np.abs(np.asarray(sm, dtype=np.float64))
        # truncation at the largest raw ratio: where the value less its error is still above 0 both sides give exactly 0
        # (also where the device's expm1 overflows to +inf); elsewhere min(., 0) is 1-Lipschitz
        dsm = np.where(np.asarray(sm, dtype=np.float64) - dsm > 0, 0.0, dsm)
        sm = np.minimum(sm, 0)
        # tied raw values share the mean of their positions' values
        smt, dsmt = sm.copy(), dsm.copy()
        a = 0
        while a < n:
            b = a + 1
            while b < n and xt[b] == xt[a]:
                b += 1
            if b - a > 1:
                smt[a:b] = sm[a:b].sum() / (b - a)
                dsmt[a:b] = dsm[a:b].mean() + (max(C, b - a) + 1) * U * float(np.abs(sm[a:b]).mean())
            a = b
        lw[idx[order]] = smt
        dlw[idx[order]] = dsmt
    lsew, dlsew = _lse(lw, dlw)
    logw = lw - lsew
    dlogw = dlw + dlsew + U * np.abs(np.asarray(logw, dtype=np.float64))
    VL = V.astype(LD)
    e = lw + VL
    le, dle = _lse(e, dlw + U * np.abs(np.asarray(e, dtype=np.float64)))
    elpd = le - lsew
    delpd = dle + dlsew + U * abs(float(elpd))
    lv, dlv = _lse(VL, np.zeros(S))
    logS = np.log(LD(S))
    lppd = lv - logS
    dlppd = dlv + EPS_FN * float(logS) + U * abs(float(lppd))
    # the weights' effective sample size A^2 / Q
    w = np.exp(logw)
    wf = np.asarray(w, dtype=np.float64)
    ess = 1 / np.sum(w * w)
    mxw = float(lw.max())
    rel = dlw + U * np.abs(np.asarray(lw, dtype=np.float64) - mxw) + EPS_FN
    dA = _wsum(wf, rel) + c_sum(S) * U
    w2 = wf * wf / float(np.sum(wf * wf))
    dQ = 2 * _wsum(w2, rel) + (c_sum(S) + 2) * U
    dess = float(ess) * (2 * dA + dQ + 4 * U)
    # WAIC: the sample variance with divisor S - 1
    mean = VL.mean()
    dev = VL - mean
    ssq = np.sum(dev * dev)
    Vf = np.abs(V)
    dmean = c_sum(S) * U * float(Vf.sum()) / S + U * abs(float(mean))
    devf = np.abs(np.asarray(dev, dtype=np.float64))
    dssq = float(np.sum(2 * devf * (dmean + U * (devf + Vf)) + 2 * U * devf * devf)) + c_sum(S) * U * float(ssq)
    if S > 1:
        pw = ssq / (S - 1)
        dpw = dssq / (S - 1) + 2 * U * float(pw)
    else:
        pw, dpw = nanv, 0.0
    out = dict(elpd_loo=elpd, lppd=lppd, p_loo=lppd - elpd, pareto_k=khat, n_tail=n, ess_w=ess, p_waic=pw,
               elpd_waic=lppd - pw, cutoff=LD(xc), logw=logw)
    out["bound"] = dict(elpd_loo=delpd, lppd=dlppd, p_loo=delpd + dlppd + U * abs(float(lppd - elpd)), pareto_k=dkhat,
                        ess_w=dess, p_waic=dpw, elpd_waic=dlppd + dpw + (U * abs(float(lppd - pw)) if S > 1 else 0.0),
                        logw=dlogw)
    return out


def psis(T, r_eff=None):
    """psis_row of every row of T [R, S]: a list of dicts"""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    r = np.broadcast_to(np.asarray(1.0 if r_eff is None else r_eff, dtype=np.float64), (T.shape[0],))
    return [psis_row(T[i], float(r[i])) for i in range(T.shape[0])]


def k_threshold(S):
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf


# ---- weighted moments ------------------------------------------------------------------------------------------------
def weighted_moments(X, logw):
    """(mean, var, dmean, dvar), each [R, d]: sum w x / sum w and sum w (x - mean)^2 / sum w, w = exp(logw [R, S]), of
    the rows X [S, d]; longdouble values, float64 bounds"""
    X = np.asarray(X, dtype=np.float64)
    S = X.shape[0]
    w = np.exp(np.atleast_2d(np.asarray(logw, dtype=np.float64)).astype(LD))     # [R, S]
    XL = X.astype(LD)
    sw = w.sum(axis=1)
    mean = (w @ XL) / sw[:, None]
    dev = XL[None, :, :] - mean[:, None, :]
    var = np.einsum("rs,rsj->rj", w, dev * dev) / sw[:, None]
    wf, swf = np.asarray(w, dtype=np.float64), np.asarray(sw, dtype=np.float64)
    cs = c_sum(S)
    rel = (cs + 2) * U + EPS_FN
    absx = (wf @ np.abs(X)) / swf[:, None]
    meanf = np.abs(np.asarray(mean, dtype=np.float64))
    dmean = rel * (absx + meanf) + U * meanf
    devf = np.abs(np.asarray(dev, dtype=np.float64))
    varf = np.asarray(var, dtype=np.float64)
    lin = np.einsum("rs,rsj->rj", wf, 2 * devf * (dmean[:, None, :] + U * (np.abs(X)[None] + meanf[:, None, :]))) / swf[:, None]
    dvar = lin + (2 * rel + 3 * U) * varf
    return mean, var, dmean, dvar


# ---- inputs of the tests ------------------------------------------------------------------------------------------------
def synthetic_rows(R, S, c, seed):
    """rows -c z^2 of standard normals: light (c = 0.05) to infinite-variance (c = 1.5) importance ratios"""
    rng = np.random.default_rng(seed)
    return -c * rng.standard_normal((R, S)) ** 2


def metropolis_rows(R, S, seed, repeat=4, c=0.5):
    """every value repeated ``repeat`` times in runs, as a Metropolis chain repeats its state: ties everywhere, also at
    the cutoff"""
    rng = np.random.default_rng(seed)
    base = -c * rng.standard_normal((R, (S + repeat - 1) // repeat)) ** 2
    return np.ascontiguousarray(np.repeat(base, repeat, axis=1)[:, :S])


def wide_rows(R, S, seed):
    """ratios that span more than 700 in the log: the tail underflows into exp(x_c), the cutoff is the log DBL_MIN clamp"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-5.0, 0.0, (R, S))
    low = max(1, tail_size(S) // 2)                    # fewer than the tail asks for: the cutoff falls among the rest
    for r in range(R):
        V[r, rng.choice(S, low, replace=False)] = rng.uniform(-1500.0, -800.0, low)
    return V
