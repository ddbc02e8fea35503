"""numpy restatement of the device HMC sampler (csrc/k_hmc.hip): the specification the tests hold the
device to (tests only, CPU).

One iteration of chain w, state (x, lp, g = grad lp(x)), diagonal inverse metric minv, box (lo, hi):

    eps_w = eps (1 + jitter (2 u_j - 1))            p = z / sqrt(minv)            K_old = 1/2 sum minv p^2
    L times:   p += 1/2 eps_w g;   x += eps_w minv p;   (x, p) = fold(x, p);   lp, g = target(x);   p += 1/2 eps_w g
    H = -lp + K;   accept iff log u < H_old - H_new
    divergence (rejected, counted): lp_new != -inf and (H_new not finite or H_new - H_old > 1000)
    on reject x, lp, g stay.  Outside the open box (a coordinate exactly on a face after the fold) lp = -inf, g = 0.

fold (Neal 2011, 5.1, in closed form):  w = hi - lo;  t = fmod(x - lo, 2 w), + 2 w if negative;
    x = lo + (2 w - t if t > w else t);   p = -p where t > w.

Random stream: Philox4x32-10 (Salmon et al. 2011), counter (w, tag, step_lo, step_hi), key = (seed_lo, seed_hi);
u01(hi, lo) = ((hi << 32 | lo) >> 11) 2^-53.  Tag 6: u_accept = u01(x, y), u_j = u01(z, w).  Tag 8 + j: the normal pair
(2j, 2j + 1):  u1 = u01(x, y), u2 = u01(z, w), rad = sqrt(-2 log(1 - u1)), z_2j = rad cos(2 pi u2), z_2j+1 = rad sin(2 pi u2).

Dual averaging of the step size (Hoffman & Gelman 2014, algorithm 5), fed with the mean over the chains of
min(1, exp(H_old - H_new)) (0 for a divergence):  gamma = 0.05, t0 = 10, kappa = 0.75, mu = log(10 eps_start):
    m += 1;  Hbar = (1 - 1/(m + t0)) Hbar + (target - alpha) / (m + t0);  log eps = mu - sqrt(m) / gamma Hbar;
    log eps_bar = m^-kappa log eps + (1 - m^-kappa) log eps_bar;  the next iteration runs at eps = exp(log eps).

The target of the trajectory tests is grad_ref.reference (gradient, and its a-priori bound) and hp_ref.log_posterior
(lp), summed over the groups.  ``reference_run`` also reruns the chains with every gradient component moved by
+-grad_bound (N_PATTERNS random sign patterns, fixed per chain and component over the run): the largest deviation of
those runs from the unperturbed one, per iteration, is what a device whose gradients are within the bound can show.
"""
from __future__ import annotations

import functools
import os

import numpy as np

import golden_util as GU
import grad_ref as G
import hp_ref as H
import path_cases as PC

MASK = np.uint64(0xFFFFFFFF)
GAMMA, T0, KAPPA = 0.05, 10.0, 0.75
DIVERGENT = 1000.0
N_PATTERNS = 8
TOL_FACTOR = 4.0           # covers the sign patterns not drawn (the device's gradients sit far inside the bound)
MIN_MARGIN = 1e-6          # every accept decision of a comparison run is at least this far from its threshold


# ---- random stream ----------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the four output words (uint64 arrays holding 32-bit values) of counter (c0, c1, c2, c3) under key (k0, k1)"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & MASK, (p0 >> s32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + w0) & MASK, (k1 + w1) & MASK
    return c


def u01(hi, lo):
    v = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return (v >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def draws(W, d, seed, step):
    """(z [W, d], u_accept [W], u_jitter [W]) of iteration ``step`` of the stream keyed by ``seed``"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    s0, s1 = step & 0xFFFFFFFF, step >> 32
    w = np.arange(W, dtype=np.uint64)
    r = philox4x32_10(w, 6, s0, s1, k0, k1)
    ua, uj = u01(r[0], r[1]), u01(r[2], r[3])
    z = np.empty((W, d))
    for j in range((d + 1) // 2):
        r = philox4x32_10(w, 8 + j, s0, s1, k0, k1)
        u1, u2 = u01(r[0], r[1]), u01(r[2], r[3])
        rad = np.sqrt(-2.0 * np.log(1.0 - u1))
        z[:, 2 * j] = rad * np.cos(2.0 * np.pi * u2)
        if 2 * j + 1 < d:
            z[:, 2 * j + 1] = rad * np.sin(2.0 * np.pi * u2)
    return z, ua, uj


# ---- the move ---------------------------------------------------------------------------------------------------------
def fold(x, p, lo, hi):
    """(x, p, reflected) after the closed-form reflection; ``reflected``: where the momentum changed sign"""
    w = hi - lo
    t = np.fmod(x - lo, 2.0 * w)
    t = np.where(t < 0.0, t + 2.0 * w, t)
    back = t > w
    return lo + np.where(back, 2.0 * w - t, t), np.where(back, -p, p), back


def bounce(x, p, lo, hi, max_bounces=10000):
    """the same reflection one face at a time, for scalars (the test of ``fold``): (x, sign of p, bounces)"""
    sign, n = 1.0, 0
    while (x < lo or x > hi) and n < max_bounces:
        x = 2.0 * lo - x if x < lo else 2.0 * hi - x
        sign, n = -sign, n + 1
    return x, sign * p, n


def leapfrog(target, x, p, g, eps_w, minv, lo, hi, L):
    """L leapfrog steps from (x, p) with g = grad lp(x): (x, p, lp, g, reflections per chain)"""
    e = np.asarray(eps_w, dtype=np.float64).reshape(-1, 1)
    n_reflect, lp = np.zeros(x.shape[0], dtype=np.int64), None
    for _ in range(L):
        p = p + 0.5 * e * g
        x = x + e * minv * p
        x, p, back = fold(x, p, lo, hi)
        n_reflect += back.sum(axis=1)
        lp, g = target(x)
        p = p + 0.5 * e * g
    return x, p, lp, g, n_reflect


def iterate(target, x, lp, g, p0, logu, eps_w, minv, lo, hi, L):
    """one iteration of every chain: dict x, lp, g (the new state), accept, divergent, accept_prob, dh, reflections
    (momentum sign changes per chain)"""
    kin0 = 0.5 * np.sum(minv * p0 * p0, axis=1)
    xn, pn, lpn, gn, n_reflect = leapfrog(target, x, p0, g, eps_w, minv, lo, hi, L)
    kin1 = 0.5 * np.sum(minv * pn * pn, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        h0, h1 = -lp + kin0, -lpn + kin1
        dh = h0 - h1
        div = (lpn != -np.inf) & (~np.isfinite(h1) | (h1 - h0 > DIVERGENT))
        acc = ~div & (logu < dh)
        ap = np.where(div | np.isnan(dh), 0.0, np.minimum(1.0, np.exp(np.minimum(dh, 0.0))))
    a = acc[:, None]
    return dict(x=np.where(a, xn, x), lp=np.where(acc, lpn, lp), g=np.where(a, gn, g), accept=acc, divergent=div,
                accept_prob=ap, dh=dh, reflections=n_reflect)


def dual_averaging(eps_start, accept_probs, target):
    """the step sizes after each of the iterations whose mean accept probabilities are given, and eps_bar at the end"""
    mu, hbar, leb, out = np.log(10.0 * eps_start), 0.0, 0.0, []
    for m, alpha in enumerate(accept_probs, start=1):
        hbar = (1.0 - 1.0 / (m + T0)) * hbar + (target - alpha) / (m + T0)
        le = mu - np.sqrt(m) / GAMMA * hbar
        eta = m ** -KAPPA
        leb = eta * le + (1.0 - eta) * leb
        out.append(np.exp(le))
    return np.array(out), float(np.exp(leb))


# ---- the targets ------------------------------------------------------------------------------------------------------
class Target:
    """lp (float64, -inf outside the open box), gradient (0 there) and its a-priori bound of the rows of X, summed over
    the groups [(model, y_exp, y_err, block_start)]; ``signs`` [B, d]: the gradient is moved by signs * bound"""

    def __init__(self, groups, lo, hi, signs=None):
        self.groups, self.lo, self.hi, self.signs = groups, lo, hi, signs
        self.calls = 0

    def __call__(self, X):
        self.calls += 1
        B, d = X.shape
        inside = np.all((X > self.lo) & (X < self.hi), axis=1)
        lp, g, gb = np.zeros(B, H.LD), np.zeros((B, d), H.LD), np.zeros((B, d))
        Xs = np.where(inside[:, None], X, 0.5 * (self.lo + self.hi))      # rows outside: any point; their results are dropped
        for model, y_exp, y_err, bs in self.groups:
            ref = G.reference(Xs, model, y_exp, y_err, bs)
            pred = (ref["mean"], ref["var"], ref["mean_bound"], ref["var_bound"], None)
            lp += H.log_posterior(Xs, model, self.lo, self.hi, y_exp, y_err, bs, pred=pred)[0]
            g += ref["grad"]
            gb += ref["grad_bound"]
        lp = np.where(inside, np.asarray(lp, dtype=np.float64), -np.inf)
        g = np.asarray(g, dtype=np.float64)
        if self.signs is not None:
            g = g + self.signs * gb
        return lp, np.where(inside[:, None], g, 0.0)


def quadratic_target(center, prec):
    """lp = -1/2 (x - c)^T diag(prec) (x - c): the host tests' target"""
    def f(X):
        r = X - center
        return -0.5 * np.sum(prec * r * r, axis=1), -prec * r
    return f


# ---- the trajectory cases of tests/test_gpu_hmc.py ----------------------------------------------------------------------
W_MAX, N_LEAPFROG, N_ITER, JITTER = 33, 3, 6, 0.1
# step size (dimensionless, in units of the metric's scale) and seed per case: chosen so that six iterations of three
# steps show accepts, rejects and reflections, with every decision MIN_MARGIN away from its threshold (test_hmc_host.py
# asserts it for every case)
TRAJECTORY_CASES = {
    "n17_d1_m25": dict(eps=0.5, seed=11),
    "n16_d7_m15_const": dict(eps=0.45, seed=12),
    "w16_ks5_rbf_const_two_passes": dict(eps=0.3, seed=13),
    "g7_three_groups": dict(eps=0.03, seed=14),
}


@functools.lru_cache(maxsize=None)
def trajectory_problem(name):
    """dict groups [(model, y_exp, y_err, block_start)], lo, hi of a trajectory case"""
    if name == "g7_three_groups":
        g = GU.load("g7_shipped_config")
        names, _, block_start, cols = GU.g7_groups(g)
        models = GU.g7_models(g)
        groups = [(models[n], g["y_exp"][cols[n]], g["y_err"][cols[n]], np.asarray(block_start[n], dtype=np.int64)) for n in names]
        return dict(groups=groups, lo=np.asarray(g["lo"], dtype=np.float64), hi=np.asarray(g["hi"], dtype=np.float64))
    c = [x for x in PC.cases() if x.name == name][0]
    model, lo, hi, y_exp, y_err, bs, _ = PC.problem(c)
    return dict(groups=[(model, y_exp, y_err, bs)], lo=lo, hi=hi)


def trajectory_start(name):
    """X0 [W_MAX, d]: uniform in the box, every third row with one coordinate within one step of a face"""
    pr = trajectory_problem(name)
    lo, hi = pr["lo"], pr["hi"]
    d = lo.size
    rng = np.random.default_rng(1000 + TRAJECTORY_CASES[name]["seed"])
    X0 = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (W_MAX, d))
    for w in range(0, W_MAX, 3):
        j = (w // 3) % d
        off = rng.uniform(1e-3, 2e-2) * (hi[j] - lo[j])
        X0[w, j] = lo[j] + off if (w // 3) % 2 == 0 else hi[j] - off
    return X0


def trajectory_draws(name, it):
    """(p0 [W_MAX, d], logu, eps_w) of iteration ``it``: what the device draws at step ``it`` with the case's seed"""
    pr, cs = trajectory_problem(name), TRAJECTORY_CASES[name]
    lo, hi = pr["lo"], pr["hi"]
    minv = (hi - lo) ** 2 / 12.0
    z, ua, uj = draws(W_MAX, lo.size, cs["seed"], it)
    with np.errstate(divide="ignore"):
        return z / np.sqrt(minv), np.log(ua), cs["eps"] * (1.0 + JITTER * (2.0 * uj - 1.0))


RUN_ARRAYS = ("chain", "lp", "accept", "divergent", "margin", "div_margin", "deviation")
RUN_COUNTS = ("reflections", "flips")
# the cases whose reference run is a recorded fixture (tests/golden/hmc_ref_<case>.npz, written by running this file):
# the three-group shape's 41 PCs on 200 design points cost 60 ms per row and call in grad_ref, minutes for the run.
# tests/test_hmc_host.py recomputes a part of it
RECORDED = ("g7_three_groups",)


def compute_reference_run(name, chains=W_MAX, n_iter=N_ITER, n_patterns=N_PATTERNS):
    """The unperturbed run of the first ``chains`` chains and ``n_patterns`` perturbed ones, as one stacked batch: dict
    chain [n_iter, chains, d], lp, accept, divergent (bool), margin (|log u - dH|), div_margin (|H_new - H_old - 1000|)
    [n_iter, chains], deviation [n_iter, chains] (the largest |x_perturbed - x| over the patterns and the coordinates,
    in units of the box width), reflections (momentum sign changes of the unperturbed chains), flips (accept or
    divergence decisions of a perturbed run that differ from the unperturbed one's)"""
    pr, cs = trajectory_problem(name), TRAJECTORY_CASES[name]
    lo, hi = pr["lo"], pr["hi"]
    d, V, W = lo.size, n_patterns + 1, chains
    minv = (hi - lo) ** 2 / 12.0
    rng = np.random.default_rng(2000 + cs["seed"])
    signs = np.concatenate([np.zeros((W, d)), rng.choice([-1.0, 1.0], (n_patterns, W_MAX, d))[:, :W].reshape(-1, d)])
    target = Target(pr["groups"], lo, hi, signs)
    x = np.tile(trajectory_start(name)[:W], (V, 1))
    lp, g = target(x)
    out = {k: [] for k in RUN_ARRAYS}
    out.update(reflections=0, flips=0)
    for it in range(n_iter):
        p0, logu, eps_w = (np.tile(a[:W], (V, 1) if a.ndim == 2 else V) for a in trajectory_draws(name, it))
        r = iterate(target, x, lp, g, p0, logu, eps_w, minv, lo, hi, N_LEAPFROG)
        x, lp, g = r["x"], r["lp"], r["g"]
        xs = x.reshape(V, W, d)
        acc, div = r["accept"].reshape(V, W), r["divergent"].reshape(V, W)
        out["chain"].append(xs[0].copy())
        out["lp"].append(lp[:W].copy())
        out["accept"].append(acc[0].copy())
        out["divergent"].append(div[0].copy())
        with np.errstate(invalid="ignore"):
            out["margin"].append(np.abs(logu[:W] - r["dh"][:W]))
            out["div_margin"].append(np.abs(-r["dh"][:W] - DIVERGENT))
        out["deviation"].append(np.max(np.abs(xs[1:] - xs[0]) / (hi - lo), axis=(0, 2)) if V > 1 else np.zeros(W))
        out["flips"] += int(np.sum(acc[1:] != acc[0]) + np.sum(div[1:] != div[0]))
        out["reflections"] += int(r["reflections"][:W].sum())
    for k in RUN_ARRAYS:
        out[k] = np.stack(out[k])
    return out


def _recorded_path(name):
    return os.path.join(GU.GOLDEN_DIR, f"hmc_ref_{name}.npz")


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """``compute_reference_run(name)``, computed once per process -- or, for the RECORDED cases, read from the fixture"""
    if name in RECORDED:
        with np.load(_recorded_path(name), allow_pickle=False) as f:
            out = {k: f[k] for k in RUN_ARRAYS}
            out.update({k: int(f[k]) for k in RUN_COUNTS})
            assert float(f["eps"]) == TRAJECTORY_CASES[name]["eps"] and int(f["seed"]) == TRAJECTORY_CASES[name]["seed"]
        return out
    return compute_reference_run(name)


def tolerance(run, chains):
    """per iteration, in units of the box width: TOL_FACTOR times the largest deviation of the perturbed runs of the
    first ``chains`` chains"""
    return TOL_FACTOR * run["deviation"][:, :chains].max(axis=1)


if __name__ == "__main__":      # python tests/hmc_ref.py: (re)write the recorded runs
    for case in RECORDED:
        res = compute_reference_run(case)
        np.savez_compressed(_recorded_path(case), eps=TRAJECTORY_CASES[case]["eps"], seed=TRAJECTORY_CASES[case]["seed"],
                            **{k: res[k] for k in RUN_ARRAYS + RUN_COUNTS})
        print(case, "accepts", int(res["accept"].sum()), "divergences", int(res["divergent"].sum()), "reflections",
              res["reflections"], "flips", res["flips"], "min margin", float(np.nanmin(res["margin"])))
