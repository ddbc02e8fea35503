"""Reference for the chain diagnostics (numpy and scipy only): rank-normalised split-R-hat, bulk / tail ESS and the ESS
of the mean of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), as ArviZ's ``_rhat_rank`` / ``_ess`` compute them.
It is the specification the device is held to; it imports nothing from the library.

For one parameter and a segment ``x[n][M]``: ``split(x)`` is ``[N][2M]`` (N = n // 2, rows [0, N) next to rows
[n - N, n); split chain (h, m) is column h M + m), ``zscore`` the normal scores of the pooled average ranks.  Sums run
in extended precision (np.longdouble), so that the reference's own rounding is far below the a-priori bounds of the
device's (``acov_bound``, ``moment_bounds``)."""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

U = 2.0 ** -53
KINDS = ("rank_z", "folded_rank_z", "le_05", "le_95", "identity")
Z_KINDS = ("rank_z", "folded_rank_z")
# the cases of the GPU tests: (n, M, d) x seeds
SHAPES = ((9, 5, 1), (64, 5, 3), (301, 7, 3), (1200, 24, 16))
SEEDS = (2, 3, 4, 5)


def metropolis(n, M, d, seed, scale=1.2):
    """Synthetic random-walk Metropolis chains ``[n][M][d]`` on a unit normal target, every (chain, parameter) on its
    own: rejected moves repeat the value, so ties are the rule."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, M, d))
    cur = rng.standard_normal((M, d))
    for t in range(n):
        prop = cur + scale * rng.standard_normal((M, d))
        acc = np.log(rng.random((M, d))) < 0.5 * (cur * cur - prop * prop)
        cur = np.where(acc, prop, cur)
        x[t] = cur
    return x


def split(x):
    n = x.shape[0]
    N = n // 2
    return np.concatenate([x[:N], x[n - N:]], axis=1)


def rank_prob(y):
    r = rankdata(y.reshape(-1), method="average").reshape(y.shape)
    return (r - 0.375) / (y.size + 0.25)


def zscore(y):
    return ndtri(rank_prob(y))


def transformed(x, kind):
    """The split, transformed series ``[N][2M]`` of one parameter ``x[n][M]``."""
    if kind == "identity":
        return split(x)
    if kind == "rank_z":
        return zscore(split(x))
    if kind == "folded_rank_z":
        return zscore(split(np.abs(x - np.median(x))))
    if kind in ("le_05", "le_95"):
        q = np.quantile(x, 0.05 if kind == "le_05" else 0.95)
        return split((x <= q).astype(np.float64))
    raise ValueError(kind)


def moments(y):
    """(grand mean, W = mean ddof-1 chain variance, b = ddof-1 variance of the chain means), extended precision."""
    yl = y.astype(np.longdouble)
    N, K = y.shape
    m = yl.sum(axis=0) / N
    c = yl - m
    W = ((c * c).sum(axis=0) / (N - 1)).sum() / K
    gm = m.sum() / K
    b = ((m - gm) ** 2).sum() / (K - 1) if K > 1 else np.longdouble(0)
    return float(gm), float(W), float(b)


def centred(y):
    """y minus its chain means, in extended precision."""
    yl = y.astype(np.longdouble)
    return yl - yl.sum(axis=0) / y.shape[0]


def autocov(y, lag, c=None):
    """g[lag]: the mean over the chains of the biased autocovariance 1/N sum_t c[t] c[t + lag] (c = centred(y))."""
    N, K = y.shape
    c = centred(y) if c is None else c
    return float((c[:N - lag] * c[lag:]).sum() / (np.longdouble(N) * K))


def acov_bound(y, lag, z_cap=0.0, c=None):
    """A-priori bound of the device's error in g[lag]: gamma_N on the centred products, (8 N 2^-53 + 2 z_cap) times
    1/(N K) sum |c[t]| |c[t + lag]| -- the 8 covers the centring, fma contraction and the chunked order; z_cap is the
    relative deviation allowed to each normal score (0 for the identity and indicator kinds)."""
    N, K = y.shape
    c = np.abs(y - y.mean(axis=0)) if c is None else c
    return (8.0 * N * U + 2.0 * z_cap) * float((c[:N - lag] * c[lag:]).sum()) / (N * K)


def moment_bounds(y, z_cap=0.0):
    """The same form for (grand mean, W, b).  A chain mean is off by at most e = (8 N 2^-53 + z_cap) mean_t max(|y|, 1)
    (a normal score's deviation is measured in units of max(|z|, 1)); W is a sum of non-negative centred squares; b is a
    sum over the K chains of (m_k - mean)^2 with every m_k, and the mean, off by e: |delta b| <= 1/(K - 1) sum_k
    (4 e |m_k - mean| + 4 e^2) + 8 K 2^-53 b."""
    N, K = y.shape
    e = (8.0 * N * U + z_cap) * float(np.maximum(np.abs(y), 1.0 if z_cap else 0.0).mean(axis=0).max())
    gm, W, b = moments(y)
    m = y.mean(axis=0)
    bb = float((4.0 * e * np.abs(m - gm) + 4.0 * e * e).sum()) / max(K - 1, 1) + 8.0 * K * U * b
    return e + 8.0 * K * U * abs(gm), (8.0 * N * U + 2.0 * z_cap) * W, bb


def plain_rhat(y, W=None, b=None):
    N = y.shape[0]
    if float(y.max() - y.min()) < 1e-15:
        return float("nan")
    if W is None:
        _, W, b = moments(y)
    return math.sqrt(((N - 1.0) / N * W + b) / W)


def scan(N, K, g, mean_var, b):
    """The Geyer scan of the issue, on ``g(t)`` (a callable).  Returns ``(ess, max_t, trace)``: trace holds every
    branch decision with the margin it was taken by."""
    var_plus = mean_var * (N - 1.0) / N
    if K > 1:
        var_plus += b
    rho_of = lambda t: 1.0 - (mean_var - g(t)) / var_plus    # noqa: E731
    trace = []

    def decide(v, strict):
        taken = v > 0.0 if strict else v >= 0.0
        trace.append((bool(taken), abs(v)))
        return taken

    rho = np.zeros(N + 2)
    rho[0] = even = 1.0
    rho[1] = odd = rho_of(1)
    t = 1
    while t < N - 3 and decide(even + odd, True):
        even, odd = rho_of(t + 1), rho_of(t + 2)
        if decide(even + odd, False):
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if decide(even, True):
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if decide((rho[t + 1] + rho[t + 2]) - (rho[t - 1] + rho[t]), True):
            rho[t + 1] = rho[t + 2] = (rho[t - 1] + rho[t]) / 2.0
        t += 2
    tau = -1.0 + 2.0 * float(np.sum(rho[:max_t + 1])) + rho[max_t + 1]
    floor = 1.0 / math.log10(N * K)
    trace.append((tau > floor, abs(tau - floor)))
    tau = max(tau, floor)
    return N * K / tau, max_t, trace


def plain_ess(y):
    N, K = y.shape
    if float(y.max() - y.min()) < 1e-15:
        return float(N * K)
    _, W, b = moments(y)
    cache, c = {}, centred(y)

    def g(t):
        if t not in cache:
            cache[t] = autocov(y, t, c)
        return cache[t]
    return scan(N, K, g, W, b)[0]


def diagnostics_1d(x):
    """The five diagnostics of one parameter ``x[n][M]``."""
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        return {k: float("nan") for k in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")}
    y = {k: transformed(x, k) for k in KINDS}
    ess_mean = plain_ess(y["identity"])
    return {"rhat": float(np.maximum(plain_rhat(y["rank_z"]), plain_rhat(y["folded_rank_z"]))),
            "ess_bulk": plain_ess(y["rank_z"]),
            "ess_tail": min(plain_ess(y["le_05"]), plain_ess(y["le_95"])),
            "ess_mean": ess_mean,
            "mcse_mean": float(np.std(x, ddof=1)) / math.sqrt(ess_mean)}


def diagnostics(chain):
    """``dict`` of ``(d,)`` arrays for a chain ``[n][M][d]``."""
    chain = np.asarray(chain, dtype=np.float64)
    per = [diagnostics_1d(chain[:, :, dd]) for dd in range(chain.shape[2])]
    return {k: np.array([p[k] for p in per]) for k in per[0]}


# ---- the cases of the GPU tests, with everything the comparisons need ----------------------------------------------
@functools.lru_cache(maxsize=None)
def case(shape, seed):
    """For the chain ``metropolis(*shape, seed)``: per parameter and kind the transformed series, its moments, the lags
    g[0 .. max_t + 2] the scan reads (and two more), the a-priori bounds, and the diagnostics."""
    n, M, d = shape
    x = metropolis(n, M, d, seed)
    out = {"x": x, "N": n // 2, "K": 2 * M, "kinds": [], "diag": diagnostics(x)}
    for dd in range(d):
        per = {}
        for k in KINDS:
            y = transformed(x[:, :, dd], k)
            N, K = y.shape
            gm, W, b = moments(y)
            cache, cl = {}, centred(y)

            def g(t, y=y, cache=cache, cl=cl):
                if t not in cache:
                    cache[t] = autocov(y, t, cl)
                return cache[t]
            ess, max_t, trace = scan(N, K, g, W, b)
            L = min(N, max_t + 3)
            per[k] = {"y": y, "moments": (gm, W, b), "g": np.array([g(t) for t in range(L)]), "max_t": max_t,
                      "ess": ess, "trace": trace}
        out["kinds"].append(per)
    return out


def case_bounds(c, z_cap):
    """Per parameter and kind: ``(moment bounds, g bounds[0 .. L))`` with ``z_cap`` on the two rank kinds."""
    out = []
    for per in c["kinds"]:
        o = {}
        for k, v in per.items():
            zc = z_cap if k in Z_KINDS else 0.0
            ca = np.abs(v["y"] - v["y"].mean(axis=0))
            o[k] = (moment_bounds(v["y"], zc), np.array([acov_bound(v["y"], t, zc, ca) for t in range(v["g"].size)]))
        out.append(o)
    return out


def perturbed(c, z_cap, n_patterns=8, seed=0):
    """Reruns the scans of ``case`` c with g, mean_var and b moved by +- their bounds under ``n_patterns`` random sign
    patterns.  Returns ``(dev, same_branches, min_margin)``: the largest deviation of each diagnostic ``(d,)``, whether
    every perturbed scan took the branches of the unperturbed one, and the smallest margin of any decision."""
    rng = np.random.default_rng(seed)
    N, K, x = c["N"], c["K"], c["x"]
    d = x.shape[2]
    bounds = case_bounds(c, z_cap)
    dev = {k: np.zeros(d) for k in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")}
    same, margin = True, math.inf
    for dd in range(d):
        per, base = c["kinds"][dd], {k: c["diag"][k][dd] for k in dev}
        sd = float(np.std(x[:, :, dd], ddof=1))
        for v in per.values():
            margin = min(margin, min(m for _, m in v["trace"]))
        for _ in range(n_patterns):
            ess, rh = {}, {}
            for k, v in per.items():
                (_, eW, eb), eg = bounds[dd][k]
                gm, W, b = v["moments"]
                W2 = W + eW * rng.choice((-1.0, 1.0))
                b2 = b + eb * rng.choice((-1.0, 1.0))
                g2 = v["g"] + eg * rng.choice((-1.0, 1.0), size=eg.size)
                if float(v["y"].max() - v["y"].min()) < 1e-15:
                    ess[k], rh[k] = float(N * K), float("nan")
                    continue
                try:
                    e, _, trace = scan(N, K, lambda t, g2=g2: g2[t], W2, b2)
                except IndexError:          # the scan went on beyond the lags the unperturbed one read
                    same = False
                    continue
                same &= [t for t, _ in trace] == [t for t, _ in v["trace"]]
                ess[k], rh[k] = e, math.sqrt(((N - 1.0) / N * W2 + b2) / W2)
            sd2 = sd * (1.0 + 8.0 * x.shape[0] * x.shape[1] * U * rng.choice((-1.0, 1.0)))
            if len(ess) < len(per):
                continue
            got = {"rhat": float(np.maximum(rh["rank_z"], rh["folded_rank_z"])), "ess_bulk": ess["rank_z"],
                   "ess_tail": min(ess["le_05"], ess["le_95"]), "ess_mean": ess["identity"],
                   "mcse_mean": sd2 / math.sqrt(ess["identity"])}
            for k in dev:
                if np.isfinite(base[k]):
                    dev[k][dd] = max(dev[k][dd], abs(got[k] - base[k]))
    return dev, same, margin
