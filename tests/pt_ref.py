"""CPU reference of the parallel-tempered stretch-move sampler, built on oracle.sampler_oracle's
Philox stream: rung t draws its stretch moves from PhiloxStream(seeds[t]) exactly as a one-chain device sampler does,
accepts with its log-likelihood difference scaled by betas[t], and after step s (when (s + 1) % swap_every == 0)
swaps states with rung t - 1 column by column, hot to cold, with the uniform of Philox(w, 5, s_lo, s_hi; seeds[t])."""
from __future__ import annotations

import numpy as np

from oracle.sampler_oracle import PhiloxStream, philox4x32_10, u01


def tempered_stretch_step(X, lp, draws, log_prob_fn, beta):
    """One red/blue stretch step of one rung in place (oracle.sampler_oracle.stretch_step with the tempered test).
    Returns the accepted mask (W,)."""
    inds, zz, rint, logu = draws
    W, ndim = X.shape
    accepted = np.zeros(W, dtype=bool)
    for split in range(2):
        S1 = inds == split
        s, c = X[S1], X[~S1]
        z = zz[split]
        factors = (ndim - 1.0) * np.log(z)
        q = c[rint[split]] - (c[rint[split]] - s) * z[:, None]
        new_lp = np.asarray(log_prob_fn(q), dtype=np.float64)
        if np.any(np.isnan(new_lp)):
            raise ValueError("Probability function returned NaN")
        old = lp[S1]
        if beta == 1.0:
            acc = factors + new_lp - old > logu[split]
        else:
            # the infinite cases explicitly (internal.h: tempered_accept): a non-finite proposal is rejected, a walker
            # at -inf takes any finite one; only finite differences are scaled by beta
            fin = np.isfinite(new_lp)
            from_out = old == -np.inf
            diff = np.where(fin & ~from_out, new_lp - np.where(from_out, 0.0, old), 0.0)
            acc = fin & (from_out | (factors + beta * diff > logu[split]))
        js = np.flatnonzero(S1)[acc]
        accepted[js] = True
        X[js] = q[acc]
        lp[js] = new_lp[acc]
    return accepted


def swap_uniforms(seed, Wc, step):
    lo, hi = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
    r = philox4x32_10(np.arange(Wc, dtype=np.uint32), 5, lo, hi, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return u01(r[0], r[1])


def swap_pass(X, lp, betas, seeds, step, nswap_acc, nswap_try):
    """The swap pass after step ``step`` in place: X (T, Wc, d), lp (T, Wc), counters (T - 1, Wc)."""
    T, Wc = lp.shape
    for t in range(T - 1, 0, -1):
        with np.errstate(divide="ignore"):
            logu = np.log(swap_uniforms(seeds[t], Wc, step))
        nswap_try[t - 1] += 1
        fin = np.isfinite(lp[t]) & np.isfinite(lp[t - 1])
        with np.errstate(invalid="ignore"):
            acc = fin & (logu < (betas[t - 1] - betas[t]) * (lp[t] - lp[t - 1]))
        nswap_acc[t - 1] += acc
        X[t, acc], X[t - 1, acc] = X[t - 1, acc].copy(), X[t, acc].copy()
        lp[t, acc], lp[t - 1, acc] = lp[t - 1, acc].copy(), lp[t, acc].copy()


def run(X0, log_prob_fn, betas, seeds, steps, swap_every=1, a=2.0):
    """X0 (T, Wc, d).  Returns chain (steps, T, Wc, d), ll (steps, T, Wc), stretch accepts (T, Wc), swap accepts and
    attempts (T - 1, Wc)."""
    X = np.array(X0, dtype=np.float64)
    T, Wc, d = X.shape
    lp = np.stack([np.asarray(log_prob_fn(X[t]), dtype=np.float64) for t in range(T)])
    streams = [PhiloxStream(int(sd), a=a) for sd in seeds]
    chain = np.empty((steps, T, Wc, d))
    lps = np.empty((steps, T, Wc))
    nacc = np.zeros((T, Wc), dtype=np.int64)
    sacc = np.zeros((T - 1, Wc), dtype=np.int64)
    stry = np.zeros((T - 1, Wc), dtype=np.int64)
    for s in range(steps):
        for t in range(T):
            nacc[t] += tempered_stretch_step(X[t], lp[t], streams[t].draw(Wc), log_prob_fn, float(betas[t]))
        if swap_every > 0 and (s + 1) % swap_every == 0:
            swap_pass(X, lp, betas, seeds, s, sacc, stry)
        chain[s] = X
        lps[s] = lp
    return chain, lps, nacc, sacc, stry
