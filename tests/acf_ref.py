"""Extended-precision reference of the device autocorrelation estimate (``csrc/k_acf.hip``: ``gpemu_sampler_acf``, driven
by ``DeviceSampler.integrated_time``) and of the pooled chain moments (``k_rows.hip``: ``moments_to_host``), each with an
a-priori error bound of the device's algorithm; a float64 emulation of the device's own order of operations; and the
table of cases the host and GPU tests share (tests only, CPU, numpy only; it imports nothing from the library).

Reference.  From a chain block ``x[n_t][nw][d]`` (float64), in ``np.longdouble`` (x87 80-bit, unit roundoff 2^-64), for
every series s = (w, dd):

    mean_s = 1/n_t sum_t x_t,   y = x - mean_s,   a_s[l] = sum_{t < n_t - l} y_t y_{t+l},   r_s[l] = a_s[l] / a_s[0],
    f[l][dd] = 1/nw sum_w r_(w,dd)[l]

and then Sokal's window and tau exactly as ``DeviceSampler.integrated_time`` decides them (``sokal``): tau(l) = 2 sum_{k
<= l} f[k] - 1, the window is the first l that is NOT ``l < c tau(l)`` (a NaN closes it at once), and a window that never
closes in the n_t lags answers window 0 and tau(0), as emcee's ``auto_window`` does.  The margin ``|l - c tau(l)|`` of
every decision read is recorded.

Constant series.  A series whose values are all equal (a walker that never moved in the range; every series at n_t = 1)
has y = 0 exactly, a[0] = 0 and r = 0 / 0: its parameter's f is NaN at every lag.  That is the defined behaviour; the
reference sets it without trusting its own rounding of the mean.

Error bound per f[l][dd].  ``u = 2^-53``, N = n_t.  The factor 8 is the one of ``diag_ref.acov_bound``: these are the
same kernels and the same chunked order (four interleaved accumulators per chunk, at most 8 chunks added serially, fma
accumulation of the products), and a sum of N rounded terms errs by at most gamma_N ~ N u times the sum of the absolute
terms (Higham, Accuracy and Stability, ch. 3); 8 N covers the sum, the division, the subtraction of the mean and the fma.

- mean:         e_mu = 8 N u mean_t |x_t|.
- lag product:  the device's centred value is y_t + eps_t with |eps_t| <= e_mu (the same eps for every t, but nothing
                below uses that), so (y_t + eps)(y_{t+l} + eps) - y_t y_{t+l} is at most e_mu (|y_t| + |y_{t+l}|) + e_mu^2:
                    da[l] = 8 N u sum |y_t||y_{t+l}| + e_mu sum_{t < N - l} (|y_t| + |y_{t+l}|) + (N - l) e_mu^2.
                The second and third terms are the centring error that ``acov_bound`` does not need for z-scores.
- ratio:        (a + da) / (a0 + da0) - a / a0, with |da0| <= da[0] < a[0], plus the rounding of the division:
                    dr[l] = (da[l] + |r[l]| da[0]) / (a[0] - da[0]) + u |r[l]|.
                A case must have a[0] > 2 da[0] for every non-constant series (``Ref.conditioned``): a condition on the
                inputs, asserted on the CPU.
- walker mean:  thread t adds the walkers t, t + 256, ... (ceil(nw / 256) adds), the wave butterfly has 6 levels, the
                4 wave partials take 3 adds, then one division: at most ceil(nw / 256) + 10 roundings, each relative to
                a partial sum that is at most sum_w |r|:
                    df = 1/nw sum_w dr + (ceil(nw / 256) + 10) u 1/nw sum_w |r|.
- tau:          2 sum_{l <= window} df[l].

Emulation (``emulate``).  A float64 replay of the device's order for the host tests and for choosing inputs -- it is
NOT an oracle for the GPU tests: the four accumulators per chunk ``(a0 + a1) + (a2 + a3)``; ``nchunk`` / ``tchunk`` as
``gpemu_sampler_acf`` sets them; chunk partials added serially in chunk order; fma accumulation of the lag products in
step order within a chunk; the strided adds, the xor butterfly 32 .. 1 and the left-to-right wave combination of the
walker mean; a constant series centred to exact zeros (``acf_constant_mean_kernel``; ``constant_fix=False`` replays the
kernels without it).  Python has no fma here: ``fma`` is Dekker's exact product plus an 80-bit three-term sum, correctly
rounded except in rare near-ties.  ``MISTAKES`` names the defects that can be planted in it.

Pooled moments (``pooled_moments``, ``pooled_bounds``): mean and population variance of rows ``[R][d]``, in the form of
``diag_ref.moment_bounds``: e_mu = 8 R u mean|x|; variance: 8 R u var + 2 e_mu mean|x - mu| + e_mu^2.  (The device sums
256 strided partials per 1024-row block through a tree and then the block sums through the same tree: far fewer than R
roundings on any path.)
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "tests/acf_ref.py needs an extended np.longdouble (x87 80-bit or better)"
U = 2.0 ** -53
C_SUM = 8.0                      # diag_ref.acov_bound's factor
ACF_LPT, ACF_TCHUNKS, MAX_LAGS = 16, 8, 4096        # sampler_internal.h, gpemu_sampler_acf
MOM_ROWS = 1024                  # rows_dev.h
SOKAL_C = 5


# ---- the cases -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Row:
    name: str
    n_t: int
    nw: int
    d: int
    kind: str = "ar1"            # ar1 | plus1e6 | scale_dn | scale_up | stuck_walker | stuck_param
    phi: float = 0.5
    w0: int = 0
    W: int = 0                   # walkers of the ensemble the block lies in (0: nw, the whole ensemble)
    chains: int = 1              # stacked chains of the sampler that holds it (W = chains * walkers per chain)
    first: int = 0
    lags: str = "all"            # all | one | 17 | blocks  (blocks: 16, 32, the rest)
    seed: int = 0

    @property
    def width(self):
        return self.W or self.nw

    @property
    def n_lags(self):
        return {"all": min(self.n_t, MAX_LAGS), "one": 1, "17": min(17, self.n_t), "blocks": min(self.n_t, MAX_LAGS)}[self.lags]

    @property
    def blocks(self):
        """(lag0, n_lags) of the calls the row asks for"""
        L = self.n_lags
        if self.lags != "blocks":
            return [(0, L)]
        out, l0 = [], 0
        for n in (16, 32, L):
            n = min(n, L - l0)
            if n > 0:
                out.append((l0, n))
                l0 += n
        return out


KINDS = ("ar1", "plus1e6", "scale_dn", "scale_up", "stuck_walker", "stuck_param")
# The smallest shapes that reach each edge: n_t around the 16 lags per thread and the 8 chunks (130: three empty
# trailing chunks; 1000: lags longer than a chunk; 4100: the 4096-lag cap), S = nw d across 256 ((37, 7), (33, 16)),
# nw > 256 ((257, 1), (300, 2)), w0 = 5 with odd nw inside a stacked ensemble, first = 3, and every lag request.
ROWS = (
    Row("n1_all_constant", 1, 37, 7, seed=1),
    Row("n15_one_series", 15, 1, 1, W=2, seed=2),
    Row("n16_s259", 16, 37, 7, seed=3),
    Row("n17_s528", 17, 33, 16, seed=4),
    Row("n127_one_series_first3", 127, 1, 1, W=2, first=3, phi=0.95, seed=5),
    Row("n128_nw257", 128, 257, 1, seed=6),
    Row("n129_s528_blocks", 129, 33, 16, lags="blocks", seed=7),
    Row("n130_nw300", 130, 300, 2, seed=8),
    Row("n130_w5_first3_blocks", 130, 37, 7, w0=5, W=48, chains=3, first=3, lags="blocks", seed=9),
    Row("n1000_s259_phi95", 1000, 37, 7, phi=0.95, seed=10),
    Row("n1000_one_series_17", 1000, 1, 1, W=2, lags="17", seed=11),
    Row("n1000_nw257_one_lag", 1000, 257, 1, lags="one", phi=0.95, seed=12),
    Row("n4100_lag_cap", 4100, 1, 1, W=2, phi=0.95, seed=13),
    Row("n130_plus1e6", 130, 37, 7, kind="plus1e6", seed=14),
    Row("n1000_plus1e6_w5", 1000, 37, 7, kind="plus1e6", w0=5, W=48, chains=3, lags="17", seed=15),
    Row("n130_w5_scale_dn", 130, 37, 7, kind="scale_dn", w0=5, W=48, chains=3, first=3, lags="blocks", seed=9),
    Row("n130_w5_scale_up", 130, 37, 7, kind="scale_up", w0=5, W=48, chains=3, first=3, lags="blocks", seed=9),
    Row("n127_stuck_walker", 127, 37, 7, kind="stuck_walker", seed=16),
    Row("n130_stuck_walker_nw300", 130, 300, 2, kind="stuck_walker", seed=17),
    Row("n130_stuck_param", 130, 37, 7, kind="stuck_param", seed=18),
    Row("n17_nw257_first3_17", 17, 257, 1, first=3, lags="17", seed=19),
    Row("n129_nw257_w5", 129, 257, 1, w0=5, W=264, chains=2, seed=20),
    Row("n128_s528_w5_first3_blocks", 128, 33, 16, w0=5, W=40, chains=2, first=3, lags="blocks", seed=21),
    Row("n15_nw300_one_lag", 15, 300, 2, lags="one", seed=22),
    Row("n127_s259_phi95_blocks", 127, 37, 7, phi=0.95, lags="blocks", seed=23),
)
ROW = {r.name: r for r in ROWS}
# Constants tried for a stuck walker.  At n_t = 17 none leaves a residue: the chunked sum is 16 c (exact) + c, one
# rounding of 17 c, and fl(fl(n c) / n) = c for every n = 2^i + 2^j (Kahan); so the stuck rows use n_t = 127 and 130.
STUCK_CANDIDATES = (0.1, 0.3, 0.7, 1.1, 2.3)
STUCK_PARAMS = (1, 3)            # the parameters in which the stuck walker (or, the first only, every walker) sits still
STUCK_WALKER = 2


def ar1(n_t, nw, d, phi, rng):
    """AR(1) series with unit stationary variance, every (walker, parameter) with its own offset and scale"""
    e = rng.standard_normal((n_t, nw, d))
    x = np.empty((n_t, nw, d))
    x[0] = e[0]
    s = math.sqrt(1.0 - phi * phi)
    for t in range(1, n_t):
        x[t] = phi * x[t - 1] + s * e[t]
    return x * rng.uniform(0.5, 2.0, (nw, d)) + rng.uniform(-3.0, 3.0, (nw, d))


def chunking(n_t):
    """(nchunk, tchunk) of gpemu_sampler_acf"""
    nchunk = min(ACF_TCHUNKS, (n_t + ACF_LPT - 1) // ACF_LPT)
    per = (n_t + nchunk - 1) // nchunk
    return nchunk, (per + ACF_LPT - 1) // ACF_LPT * ACF_LPT


def series_mean_dev(x):
    """the device's mean of the series x[n_t][S], float64, acf_sum_kernel + acf_mean_kernel's order"""
    n_t = x.shape[0]
    nchunk, tchunk = chunking(n_t)
    tot = np.zeros(x.shape[1])
    for c in range(nchunk):
        t0, t1 = c * tchunk, min((c + 1) * tchunk, n_t)
        a = np.zeros((4, x.shape[1]))
        t = t0
        while t + 4 <= t1:
            a += x[t:t + 4]
            t += 4
        while t < t1:
            a[0] += x[t]
            t += 1
        tot = tot + ((a[0] + a[1]) + (a[2] + a[3]))
    return tot / float(n_t)


def constant_residue(c, n_t):
    """the device's mean of n_t copies of c, minus c: non-zero where the plain kernels leave a rounding residue"""
    return float(series_mean_dev(np.full((n_t, 1), float(c)))[0] - float(c))


@functools.lru_cache(maxsize=None)
def stuck_value(n_t):
    """the first of STUCK_CANDIDATES whose constant series the plain kernels do not centre to zero at n_t steps"""
    for c in STUCK_CANDIDATES:
        if constant_residue(c, n_t) != 0.0:
            return c
    raise AssertionError(f"no candidate leaves a residue at n_t = {n_t}")


@functools.lru_cache(maxsize=None)
def data(row):
    """``(wide, x)``: the stored chain ``wide[first + n_t][W][d]`` the sampler is given and the block ``x[n_t][nw][d]``
    (a view of it) the estimate is asked for.  Rows and walkers outside the block hold other series, 50 times larger."""
    rng = np.random.default_rng(1000 + row.seed)
    x = ar1(row.n_t, row.nw, row.d, row.phi, rng)
    if row.kind == "plus1e6":
        x = x + 1e6
    elif row.kind == "scale_dn":
        x = x * 2.0 ** -400
    elif row.kind == "scale_up":
        x = x * 2.0 ** 400
    elif row.kind == "stuck_walker":
        for k, dd in enumerate(STUCK_PARAMS):
            if dd < row.d:
                x[:, STUCK_WALKER, dd] = stuck_value(row.n_t) * (k + 1)
    elif row.kind == "stuck_param":
        x[:, :, STUCK_PARAMS[0]] = stuck_value(row.n_t) * (1.0 + np.arange(row.nw))[None, :]
    wide = 50.0 * ar1(row.first + row.n_t, row.width, row.d, 0.5, np.random.default_rng(5000 + row.seed))
    wide[row.first:, row.w0:row.w0 + row.nw] = x
    wide.setflags(write=False)
    return wide, wide[row.first:, row.w0:row.w0 + row.nw]


def stuck_parameters(row):
    """the parameters whose f is NaN by definition"""
    if row.n_t == 1:
        return tuple(range(row.d))
    if row.kind == "stuck_walker":
        return tuple(dd for dd in STUCK_PARAMS if dd < row.d)
    if row.kind == "stuck_param":
        return (STUCK_PARAMS[0],)
    return ()


# ---- the reference -----------------------------------------------------------------------------------------------------
def sokal(f, n_t, c=SOKAL_C):
    """Sokal's window and tau of ``f[L][d]`` (lags 0 .. L - 1 of a chain of n_t steps) as DeviceSampler.integrated_time
    decides them: ``(windows (d,), tau (d,), margins)``, margins[dd] the |l - c tau(l)| of every decision read.  Raises
    IndexError where a window is still open at lag L < n_t (more lags are needed)."""
    f = np.asarray(f)
    L, d = f.shape
    taus = 2.0 * np.cumsum(f.astype(LD), axis=0) - 1.0
    windows, tau, margins = np.zeros(d, dtype=int), np.full(d, np.nan), []
    for dd in range(d):
        m = []
        for l in range(L):
            t = taus[l, dd]
            m.append(float(abs(l - c * t)) if np.isfinite(t) else math.inf)
            if not l < c * t:
                windows[dd], tau[dd] = l, float(t)
                break
        else:
            if L < n_t:
                raise IndexError("window still open")
            windows[dd], tau[dd] = 0, float(taus[0, dd])
        margins.append(m)
    return windows, tau, margins


class Ref:
    """The reference of one block ``x[n_t][nw][d]``: ``f``, ``df`` (float64, [L][d]) for lags 0 .. L - 1, grown on demand."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        self.n_t, self.nw, self.d = self.x.shape
        xl = self.x.reshape(self.n_t, -1).astype(LD)
        self.const = np.all(self.x.reshape(self.n_t, -1) == self.x.reshape(self.n_t, -1)[0], axis=0)
        self.mean = xl.sum(axis=0) / self.n_t
        self.y = xl - self.mean
        self.y[:, self.const] = 0.0
        self.ay = np.abs(self.y).astype(np.float64)
        self.e_mu = C_SUM * self.n_t * U * np.abs(self.x.reshape(self.n_t, -1)).mean(axis=0)
        self.a = np.zeros((0, self.y.shape[1]), dtype=LD)
        self.da = np.zeros((0, self.y.shape[1]))

    def _grow(self, L):
        L = min(L, self.n_t)
        l0 = self.a.shape[0]
        if L <= l0:
            return
        N, y, ay, e = self.n_t, self.y, self.ay, self.e_mu
        a, da = np.empty((L - l0, y.shape[1]), dtype=LD), np.empty((L - l0, y.shape[1]))
        for l in range(l0, L):
            a[l - l0] = (y[:N - l] * y[l:]).sum(axis=0)
            da[l - l0] = (C_SUM * N * U * (ay[:N - l] * ay[l:]).sum(axis=0)
                          + e * (ay[:N - l].sum(axis=0) + ay[l:].sum(axis=0)) + (N - l) * e * e)
        self.a, self.da = np.concatenate([self.a, a]), np.concatenate([self.da, da])

    @property
    def conditioned(self):
        """a[0] > 2 da[0] for every non-constant series"""
        self._grow(1)
        return bool(np.all(self.a[0][~self.const].astype(np.float64) > 2.0 * self.da[0][~self.const]))

    def series(self, L):
        """(r, dr) [L][S]: the normalised series and their bounds; NaN for a constant series"""
        self._grow(L)
        a, da = self.a[:L], self.da[:L]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = a / a[0]
            r[:, self.const] = np.nan
            r64 = r.astype(np.float64)
            a0 = a[0].astype(np.float64)
            dr = (da + np.abs(r64) * da[0]) / (a0 - da[0]) + U * np.abs(r64)
        return r, dr

    def f(self, L):
        """(f, df) [L][d] in float64"""
        r, dr = self.series(L)
        L = r.shape[0]
        r3, dr3 = r.reshape(L, self.nw, self.d), dr.reshape(L, self.nw, self.d)
        f = (r3.sum(axis=1) / self.nw).astype(np.float64)
        depth = math.ceil(self.nw / 256) + 10
        df = dr3.sum(axis=1) / self.nw + depth * U * np.abs(r3.astype(np.float64)).sum(axis=1) / self.nw
        return f, df

    def tau(self, c=SOKAL_C):
        """``(windows, tau, dtau, margins, dread)``: Sokal's windows, the lags grown until every one has closed"""
        L = min(self.n_t, 64)
        while True:
            f, df = self.f(L)
            try:
                w, tau, margins = sokal(f, self.n_t, c)
                break
            except IndexError:
                L = min(self.n_t, 2 * L)
        # tau is held to the bound of the lags up to its window (a window that never closed answers tau(0)); the
        # decisions are held to the bound of every lag they read (dread)
        dtau = np.array([2.0 * df[:w[dd] + 1, dd].sum() for dd in range(self.d)])
        dread = np.array([2.0 * df[:len(margins[dd]), dd].sum() for dd in range(self.d)])
        return w, tau, dtau, margins, dread


@functools.lru_cache(maxsize=None)
def ref(row):
    return Ref(data(row)[1])


# ---- float64 emulation of the device's order ---------------------------------------------------------------------------
MISTAKES = ("drop_last_step", "shift_lags", "no_zero_padding", "ld_of_block", "divide_by_nw_plus_1", "skip_walkers_256",
            "other_series_lag0")


def _two_prod(a, b):
    """p + e = a b exactly (Dekker / Veltkamp), float64 arrays"""
    p = a * b
    sa = a * 134217729.0
    ah = sa - (sa - a)
    al = a - ah
    sb = b * 134217729.0
    bh = sb - (sb - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def fma(a, b, c):
    """round(a b + c) in float64: the exact product as p + e, the exact p + c as s + t, then s + (t + e) in 80 bits"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                  np.asarray(c, dtype=np.float64))
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return (s.astype(LD) + (t.astype(LD) + e.astype(LD))).astype(np.float64)


def emulate(wide, first, n_t, w0, nw, lags, mistake=None, constant_fix=True):
    """f[len(lags)][d] as the kernels of k_acf.hip form it for rows [first, first + n_t), walkers [w0, w0 + nw) of the
    stored chain ``wide[steps][W][d]``, in float64 and in their order.  ``mistake``: one of MISTAKES, planted."""
    assert mistake is None or mistake in MISTAKES
    wide = np.asarray(wide, dtype=np.float64)
    W, d = wide.shape[1], wide.shape[2]
    S = nw * d
    flat = wide.reshape(-1)
    ld = nw * d if mistake == "ld_of_block" else W * d
    base = first * W * d + w0 * d
    x = flat[base + np.arange(n_t)[:, None] * ld + np.arange(S)[None, :]]            # chain[t * ld + s]
    nchunk, tchunk = chunking(n_t)
    mu = series_mean_dev(x)
    if constant_fix:
        const = np.all(x == x[0], axis=0)
        mu = np.where(const, x[0], mu)
    y = x - mu
    lags = np.asarray(lags, dtype=np.int64)
    lag_read = np.where(lags >= ACF_LPT, lags + 1, lags) if mistake == "shift_lags" else lags   # thread 0 keeps its lags
    acf = np.zeros((lags.size, S))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(nchunk):
            t0, t1 = c * tchunk, min((c + 1) * tchunk, n_t)
            if mistake == "drop_last_step":
                t1 -= 1
            acc = np.zeros((lags.size, S))
            for t in range(t0, t1):
                idx = t - lag_read
                lagged = np.where((idx >= 0)[:, None], y[np.clip(idx, 0, n_t - 1)], 0.0)
                if mistake == "no_zero_padding" and c == 0:
                    lagged = y[np.clip(idx, 0, n_t - 1)]
                acc = fma(y[t][None, :], lagged, acc)
            acf = acf + acc
        # lag 0 for the normalisation: the same sum
        acf0 = np.zeros(S)
        for c in range(nchunk):
            t0, t1 = c * tchunk, min((c + 1) * tchunk, n_t)
            if mistake == "drop_last_step":
                t1 -= 1
            acc = np.zeros(S)
            for t in range(t0, t1):
                acc = fma(y[t], y[t], acc)
            acf0 = acf0 + acc
        if mistake == "other_series_lag0":
            acf0 = np.roll(acf0, -1)
        with np.errstate(divide="ignore"):
            r = (acf / acf0).reshape(lags.size, nw, d)
        # acf_walker_mean_kernel: thread t adds walkers t, t + 256, ...; butterfly 32 .. 1 per wave; waves left to right
        part = np.zeros((lags.size, 256, d))
        for w in range(nw):
            if mistake == "skip_walkers_256" and w >= 256:
                break
            part[:, w % 256] = part[:, w % 256] + r[:, w]
        v = part.reshape(lags.size, 4, 64, d)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ off]
        ws = v[:, :, 0]
        out = ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]
        return out / float(nw + 1 if mistake == "divide_by_nw_plus_1" else nw)


def emu_lags(row):
    """the lags the emulation is run at: all the row asks for where that is cheap, else those at the edges (the first
    two threads, the chunk ends, the last lags) and every 37th"""
    L = row.n_lags
    if row.n_t * L * row.nw * row.d <= 3_000_000:
        return np.arange(L)
    _, tchunk = chunking(row.n_t)
    pick = set(range(min(L, 34))) | set(range(0, L, 37)) | {L - 1, L - 2, L - 3}
    for c in range(1, ACF_TCHUNKS):
        pick |= {c * tchunk - 1, c * tchunk, c * tchunk + 1}
    return np.array(sorted(l for l in pick if 0 <= l < L))


def emulate_row(row, mistake=None, constant_fix=True, lags=None):
    wide, _ = data(row)
    lags = emu_lags(row) if lags is None else lags
    return lags, emulate(wide, row.first, row.n_t, row.w0, row.nw, lags, mistake, constant_fix)


def err_over_bound(got, f, df):
    """the largest |got - f| / df over the finite entries of f, and whether got is NaN exactly where f is"""
    fin = np.isfinite(f)
    same_nan = bool(np.array_equal(np.isnan(got), np.isnan(f)))
    if not fin.any():
        return 0.0, same_nan
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(got - f)[fin] / df[fin]
    q = np.where(np.isnan(q), np.inf, q)             # a NaN where the reference is finite is outside any bound
    return float(q.max()), same_nan


# ---- pooled moments ---------------------------------------------------------------------------------------------------
def pooled_moments(x):
    """(mean, population variance) [d] of the rows x[R][d], extended precision"""
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    R = xl.shape[0]
    mean = xl.sum(axis=0) / R
    c = xl - mean
    return mean, (c * c).sum(axis=0) / R


def pooled_bounds(x):
    """(mean bound, variance bound) [d]: 8 R u mean|x|; 8 R u var + 2 e_mu mean|x - mu| + e_mu^2 (module docstring)"""
    x = np.asarray(x, dtype=np.float64)
    R = x.shape[0]
    mean, var = pooled_moments(x)
    e = C_SUM * R * U * np.abs(x).mean(axis=0)
    dev = np.abs(x.astype(LD) - mean).mean(axis=0).astype(np.float64)
    return e, C_SUM * R * U * var.astype(np.float64) + 2.0 * e * dev + e * e


MOMENT_ROWS = (1, 255, 1023, 1024, 1025, 257 * 1024 + 3)
MOMENT_D = (1, 7, 16)
MOMENT_KINDS = ("ar1", "plus1e6", "scale_dn", "scale_up")


@functools.lru_cache(maxsize=None)
def moment_rows(R, d, kind):
    """R rows of d parameters: independent normal draws with a scale and an offset per parameter"""
    rng = np.random.default_rng(R + 31 * d)
    x = rng.standard_normal((R, d)) * rng.uniform(0.5, 2.0, d) + rng.uniform(-3.0, 3.0, d)
    x = {"ar1": x, "plus1e6": x + 1e6, "scale_dn": x * 2.0 ** -400, "scale_up": x * 2.0 ** 400}[kind]
    x.setflags(write=False)
    return x
