"""Extended-precision reference of gpemu.experiment: the pairwise log-sum-exp from direct differences
in ``np.longdouble``, the nested Monte Carlo estimator of the expected information gain on top of it, the linear-Gaussian
closed form, and the error bound of the device kernel derived from its own operations (``pairlse_bound``)."""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53            # unit roundoff of fp64
CHUNK = 2048              # the kernel's constants, repeated here on purpose: the tests compare them with the module's
TILE_COLS = 128
TILE_ROWS = 64


def _log_weights(Y, Z, i0, i1):
    """a[i][j] = -|y_i - z_j|^2 / 2 of rows [i0, i1) from the differences, in longdouble"""
    d = Y[i0:i1, None, :] - Z[None, :, :]
    return -0.5 * np.einsum("ijf,ijf->ij", d, d)


def _row_blocks(n, S, F, limit=1 << 21):
    step = max(1, limit // max(1, S * F))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def _exclude(a, self_index, i0):
    if self_index is not None:
        for r in range(a.shape[0]):
            j = int(self_index[i0 + r])
            if j >= 0:
                a[r, j] = -np.inf
    return a


def pairlse_ref(Y, Z, self_index=None):
    """dict of ``m``, ``s1``, ``s2``, ``lse``, ``ess`` (longdouble, each ``(n,)``) of ``a_ij = -|y_i - z_j|^2 / 2`` with pair
    ``(i, self_index[i])`` left out; a row with nothing left: ``m = lse = -inf``, ``s1 = s2 = ess = 0``."""
    Y, Z = np.asarray(Y, dtype=LD), np.asarray(Z, dtype=LD)
    n, S, F = Y.shape[0], Z.shape[0], Y.shape[1]
    out = {k: np.zeros(n, dtype=LD) for k in ("m", "s1", "s2", "lse", "ess")}
    for i0, i1 in _row_blocks(n, S, F):
        a = _exclude(_log_weights(Y, Z, i0, i1), self_index, i0)
        m = a.max(axis=1)
        live = m > -np.inf
        w = np.where(live[:, None], np.exp(a - np.where(live, m, 0)[:, None]), 0)
        s1, s2 = w.sum(axis=1), (w * w).sum(axis=1)
        out["m"][i0:i1], out["s1"][i0:i1], out["s2"][i0:i1] = m, s1, s2
        with np.errstate(divide="ignore", invalid="ignore"):
            out["lse"][i0:i1] = np.where(live, m + np.log(np.where(live, s1, 1)), -np.inf)
            out["ess"][i0:i1] = np.where(live, s1 * s1 / np.where(live, s2, 1), 0)
    return out


def pairlse_bound(Y, Z, centre, self_index=None):
    """``(bound_lse (n,), bound_ess_rel (n,))``: the most the device's ``lse`` may differ from the exact value, absolutely,
    and its ``ess`` relatively, counted from the kernel's own operations (u = 2^-53, gamma_k = k u / (1 - k u)).

    The error of one log-weight.  With yc = y - centre, zc = z - centre exact, Hy = |yc|^2 / 2, Hz = |zc|^2 / 2:
      * centring: one rounding per element, |d^_f - d_f| <= u (|yc_f| + |zc_f|) for the difference of the centred rows,
        so | |d^|^2 - |d|^2 | / 2 <= u sum_f (|yc_f| + |zc_f|)^2 <= 4 u (Hy + Hz);
      * norms: an fma chain of F terms of one sign and an exact halving, gamma_F Hy and gamma_F Hz;
      * the MFMA chain of K = 4 ceil(F / 4) products, gamma_(K + 1) sum |yc_f zc_f| <= gamma_(K + 1) (Hy + Hz);
      * the epilogue (y.z - Hy) - Hz, two roundings of quantities below 2 (Hy + Hz): 4 u (Hy + Hz).
    E_ij = u (F + K + 9) (Hy_i + Hz_j) / (1 - (K + 1) u): absolute, as DESIGN 4.38 states.
    lse is monotone in every a with d lse / d a_j = p_j (the softmax weights), so the perturbation moves it by at most
    log sum_j p_j exp(E_ij) =: Da; the same with q_j (the softmax of 2 a) and 2 E_ij moves log s2 by at most Da2.

    The sums, relative to s1.  An element reaches the row's sum as exp(a_j - m) of the running maximum, times the rescale
    factors exp(m_old - m_new) of the tiles (at most CHUNK / 128), of the 4 butterfly stages, of the merge of the two
    waves and of the nchunk - 1 chunk merges: R stages.  The differences have one sign and telescope: their roundings add
    to u |a_j - M| in the exponent, sum_j p_j |a_j - M| u over the row.  Every exp is within 1 ulp = 2 u, every product
    with a factor one rounding: own exp 2 u, per stage 3 u.  Additions of positives: 4 per tile and lane, then one per
    stage but the tile rescales: A = 4 CHUNK / 128 + 5 + nchunk - 1, gamma_A.
        R1 = gamma_A + (2 + 3 R) u + u sum_j p_j |a_j - M|.
    s2 adds e^2 by fma (counted in A), e^2 carries twice e's error; a stage scales by sc sc or (s2 e) e: two roundings and
    twice the exp error, 6 u:   R2 = gamma_A + (4 + 6 R) u + 2 u sum_j q_j |a_j - M|.
    Underflow: a term below the smallest denormal is dropped, S 2^-1074 relative to s1 >= 1 (not representable: ignored).

    lse = fl(M + fl(log s1)), log within 1 ulp:  bound_lse = 1.1 (Da + log1p(R1) + 2 u |log s1| + u |lse|);
    ess = fl(fl(s1 s1) / s2):                    bound_ess_rel = 1.1 (2 (expm1(Da) + R1) + expm1(Da2) + R2 + 2 u).
    The 10 % are for the products of these terms.  A row with every pair left out is exact: both bounds 0."""
    Y, Z, c = np.asarray(Y, dtype=LD), np.asarray(Z, dtype=LD), np.asarray(centre, dtype=LD)
    n, S, F = Y.shape[0], Z.shape[0], Y.shape[1]
    K = 4 * ((F + 3) // 4)
    nchunk = (S + CHUNK - 1) // CHUNK
    stages = CHUNK // TILE_COLS + 5 + nchunk - 1
    adds = 4 * (CHUNK // TILE_COLS) + 5 + nchunk - 1
    gamma_a = adds * U / (1.0 - adds * U)
    Hy, Hz = 0.5 * ((Y - c) ** 2).sum(axis=1), 0.5 * ((Z - c) ** 2).sum(axis=1)
    ea = LD(U * (F + K + 9) / (1.0 - (K + 1) * U))
    b_lse, b_ess = np.zeros(n), np.zeros(n)
    for i0, i1 in _row_blocks(n, S, F):
        a = _exclude(_log_weights(Y, Z, i0, i1), self_index, i0)
        m = a.max(axis=1)
        for r in np.nonzero(m > -np.inf)[0]:
            ar = a[r] - m[r]
            keep = ar > -np.inf
            ar, E = ar[keep], ea * (Hy[i0 + r] + Hz[keep])
            w = np.exp(ar)
            s1, s2 = w.sum(), (w * w).sum()
            p, q = w / s1, w * w / s2
            da, da2 = np.log((p * np.exp(E)).sum()), np.log((q * np.exp(2 * E)).sum())
            r1 = gamma_a + (2 + 3 * stages) * U + U * (p * -ar).sum()
            r2 = gamma_a + (4 + 6 * stages) * U + 2 * U * (q * -ar).sum()
            lse = m[r] + np.log(s1)
            b_lse[i0 + r] = float(1.1 * (da + np.log1p(r1) + 2 * U * abs(np.log(s1)) + U * abs(lse)))
            b_ess[i0 + r] = float(1.1 * (2 * (np.expm1(da) + r1) + np.expm1(da2) + r2 + 2 * U))
    return b_lse, b_ess


def selected_rows(S, max_points):
    n = min(int(S), int(max_points))
    return (np.arange(n, dtype=np.int64) * int(S)) // n


def whiten_ref(means, cov=None, y_err=None):
    m = np.asarray(means, dtype=np.float64)
    if cov is None:
        return m / np.broadcast_to(np.asarray(y_err, dtype=np.float64), (m.shape[1],))[None, :]
    return np.linalg.solve(np.linalg.cholesky(np.asarray(cov, dtype=np.float64)), m.T).T


def eig_ref(means, cov=None, y_err=None, n_outer=4096, seed=0, noise=None, exclude_self=False):
    """The nested estimator on the reference: dict of ``eig_nats``, ``se``, ``terms``, ``ess_mean``, ``ess_min``, ``lse``,
    ``ess``, ``log_n_inner`` (floats and float64 arrays), and ``Y``, ``Z``, ``eps``, ``self_index`` as used."""
    Z = np.ascontiguousarray(whiten_ref(means, cov, y_err))
    S, F = Z.shape
    rows = selected_rows(S, n_outer)
    eps = (np.random.default_rng(seed).standard_normal((rows.size, F)) if noise is None
           else np.ascontiguousarray(np.asarray(noise, dtype=np.float64)[:, :F]))
    Y = np.ascontiguousarray(Z[rows] + eps)
    self_index = rows if exclude_self else None
    ref = pairlse_ref(Y, Z, self_index)
    n_inner = S - (1 if exclude_self else 0)
    terms = -0.5 * (eps.astype(LD) ** 2).sum(axis=1) - ref["lse"] + LD(math.log(n_inner))
    n = rows.size
    return {"eig_nats": float(terms.mean()), "se": float(terms.std(ddof=1) / math.sqrt(n)) if n > 1 else math.nan,
            "terms": terms.astype(np.float64), "ess_mean": float(ref["ess"].mean()), "ess_min": float(ref["ess"].min()),
            "lse": ref["lse"], "ess": ref["ess"], "log_n_inner": math.log(n_inner), "Y": Y, "Z": Z, "eps": eps,
            "self_index": self_index}


def linear_gaussian_case(d, F, S, seed, scale=1.0):
    """``(means (S, F), closed form)``: theta ~ N(0, I_d), m(theta) = scale A theta with A (F, d) ~ N(0, 1 / d), unit noise;
    the expected information gain is ``log det(I + scale^2 A A^T) / 2``."""
    rng = np.random.default_rng(1000 + seed)
    A = scale * rng.standard_normal((F, d)) / math.sqrt(d)
    theta = rng.standard_normal((S, d))
    return theta @ A.T, 0.5 * float(np.linalg.slogdet(np.eye(F) + A @ A.T)[1])
