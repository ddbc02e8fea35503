"""Extended-precision reference of the device scaler + PCA (csrc/k_pca.hip, gpemu_pca_fit) and of the
truncation covariance (gpemu_truncation_cov), with a-priori error bounds of the device's algorithm and certificates
computed from a decomposition's outputs alone (tests only, CPU).  Written in the style of cv_hp_ref.py.

Every assertion is of one of two kinds, and no threshold is read from k_pca.hip or from a measured device value.

KIND A -- outputs that are well defined, against a reference in ``np.longdouble`` (x87 80-bit) computed from Y alone:
the scaler's mean / variance / scale by sklearn's formulas (``_is_constant_feature`` evaluated in longdouble), the PCA
mean, the centred matrix Xc, and an SVD of Xc by a plain cyclic one-sided Jacobi, vectorised over the disjoint pairs
of a tournament round and iterated until the largest cosine is below 1e-18 (or, where m-term longdouble dot products
cannot resolve that, until it has stopped falling below 4 sqrt(m) 2^-63; the value reached is kept in ``cos_max`` and
its effect n cos_max sigma_1 is part of every bound).

KIND B -- certificates of a decomposition (S = Y_pca, C = components, all min(N, F) of them), formed in extended
precision by split-operand products (``xmatmul``): the cosines between columns of S, E = C C^T - I, R = Xc - S C.

Bounds.  u = 2^-53, eps = 2^-52, first order, one rounded operation at a time.  Work orientation: m = max(N, F) rows,
n = min(N, F) columns (the transpose is factored when N < F).

1. scaler_mean.  A sequential sum of N terms in row order and one division: ``|d mean| <= N u sum|y| / N``.
2. scaler_var, the corrected two-pass formula with T = mean + delta (|delta| <= item 1): t_i = fl(y_i - T);
   ``sq = sum t_i^2`` and ``corr = sum t_i`` sequentially; ``var = (sq - corr^2 / N) / N``.  In exact arithmetic the
   formula gives the variance whatever T is, so delta enters through the sizes of the t_i only:
       ``d sq <= (N + 2) u sum t^2``  (t's own rounding twice, the product, N - 1 additions),
       ``d corr <= N u sum|t|``,  ``|corr| <= N delta + d corr``,
       ``d var <= ((N + 2) u sum t^2 + 2 |corr| d corr / N + 2 u corr^2 / N + u unnorm) / N + u var``
   with |t_i| <= |y_i - mean| + delta.
3. scaler_scale = sqrt(var): ``d var / (2 sqrt(var)) + u scale``; exactly 1 for a constant feature.  The
   constant-feature decision itself is a decision: a case keeps every column a factor 100 away from sklearn's
   threshold ``N eps var + (N mean eps)^2`` (``Reference.const_margin``), and the device's must equal the reference's.
4. pca_mean.  The device standardises with ITS mean and scale, ``Ys = fl(fl(y - mean^) / scale^)``, and sums the column
   sequentially.  The exact pca mean is 0; the device's carries the scaler mean's error: with a_i = |xc_i| + delta / scale
       ``|d pca_mean| <= delta / scale + (N + 3) u mean_i(a_i)``.
5. The centred matrix the device factors.  The constant shift delta / scale cancels in the centring; what is left is
   the scale's relative error rho = d scale / scale (a column scaling) and roundings:
       ``|d Xc_ij| <= (rho_j + u) |xc_ij| + 2 u a_ij + (N + 2) u mean_i(a_ij)``;   eta_in = the Frobenius norm of it.
6. One encounter of two blocks (2 PB columns; PB = 16, or 32 when n > 1024, as DESIGN 4.7 documents): X <- X J on the
   matrix cores, one fma chain of 2 PB terms per element, J accumulated in float64 from at most inner (2 PB - 1)
   rotations per column (inner = 2 at PB = 32; at PB = 16 one in sweeps 0 .. 17 and two from sweep 18 on, so the 30
   sweeps the bounds take count 18 at inner = 1 and 12 at inner = 2: beta below is that average).
   - product: ``|fl(X J) - X J| <= 2 PB u |X||J|``, in Frobenius norm ``<= 2 PB u sqrt(2 PB) ||X||_F``
     (``|| |J| ||_2 <= ||J||_F = sqrt(2 PB)``);
   - one rotation applied to a pair of entries (two products and a sum each): ``2 sqrt(2) u`` of the pair's norm;
     (c, s) from 1 / sqrt by a hardware seed and two Newton steps: c within 3.5 u, s = c t one more, so
     ``|c^2 + s^2 - 1| <= 9 u``: 4.5 u in norm.  ROT_U = 8 covers the two.  A column of J takes part in
     inner (2 PB - 1) rotations: ``||J - Q||_F <= sqrt(2 PB) 8 u inner (2 PB - 1)`` for an exactly orthogonal Q.
   ``beta = sqrt(2 PB) u (2 PB + 8 inner (2 PB - 1))`` is the backward error of one encounter relative to the pair's
   Frobenius norm.  A sweep has nb - 1 rounds (nb blocks, rounded up to even), each of which meets every column once,
   and the bounds take SWEEPS = 30 of them (the tests assert n_sweeps <= 30, so a kernel cannot loosen its bound by
   sweeping longer): ``rounds = 30 (nb - 1)``,
       data part:      ``X_final = (Xc^ + dX) Q``,  ``||dX||_F <= rounds beta ||Xc||_F``      (Q exactly orthogonal)
       rotation part:  ``V_final = Q + dV``,          ``||dV||_F <= rounds beta sqrt(n)``.
7. The stopping rule DESIGN 4.7 documents: the largest |cos| met in the last sweep <= 4 sqrt(m) eps, on Gram entries
   the device sums on the matrix cores: rows in 64-row chunks, dealt to 4 waves (a quarter of every chunk each, one
   fma chain per wave), the waves added in order, then up to 8 row splits added in order.  A chain is at most
   ceil(m / 64) * 16 fmas long, so ``|d g| <= (16 ceil(m / 64) + 3 + 7) u |x|.|y|`` and
       ``tau = 4 sqrt(m) eps + (16 ceil(m / 64) + 10) u``
   bounds every cosine between two data columns that are not both residue (item 8).  Non-orthogonality of that size
   is a backward error ``sigma_1 n tau / 2`` (``S^ = Q (I + Coff)^(1/2)``, ``||Coff||_2 <= n tau``).
8. Residue.  Columns shorter than ``4 sqrt(m) eps ||Xc||_F`` are not rotated against each other; the
   threshold is taken from the longdouble Xc.  Such columns are left out of the cosine check.
9. Host assembly: a column norm is a sequential sum of m squares and a root, (m + 3) u relative; a division by it u.

   From 5, 6, 7, 9 (Weyl):  ``|d sigma_i| <= eta_sigma_i = eta_in + rounds beta ||Xc||_F + sigma_i (n tau / 2 + (m + 3) u)``,
   so explained_variance is held to ``(2 sigma_i eta_sigma_i + eta_sigma_i^2) / (N - 1) + 3 u ev_i``: ABSOLUTE at the
   scale sigma_1^2 u, not relative -- the apply step mixes the columns of a block pair through a J that carries
   rounding, so a small column inherits error at the scale of the largest (and the scaler has equilibrated the
   columns already).  The ratio's denominator is the squared Frobenius norm, which orthogonal transformations keep:
   ``d total <= (2 ||Xc||_F eta_F + eta_F^2) / (N - 1) + (n + 3) u total`` with eta_F = eta_in + rounds beta ||Xc||_F
   + ||Xc||_F (m + 3) u.
   Singular vectors (Wedin's sin-theta theorem, first order; the gap of a simple singular value of a rectangular
   matrix is ``min(sigma_i, min_{j != i} |sigma_i - sigma_j|)``): with eta_A = eta_in + rounds beta ||Xc||_F +
   sigma_1 n tau / 2,
       ``||d v_i|| <= vec_b_i = 2 eta_A / gap_i + rounds beta sqrt(n) + (m + 4) u``
   for the unit vector on either side; a component is held to vec_b_i elementwise and a score column to
   ``sigma_i vec_b_i + eta_sigma_i``.  Only the k = n_pc leading ones are compared, and a case must keep each of them a
   factor 1.5 away from every other singular value (``Reference.min_gap_factor``).
10. The truncation covariance from the device's own components and variances, against
   ``Xc^T Xc / (N - 1) - sum_{i < k} lambda_i v_i v_i^T`` in longdouble.  With Xc = S C + R and S^T S = D (I + Coff) D:
   ``||Xc^T Xc - C^T D^2 C|| <= sigma_1^2 n tau + 2 sigma_1 ||R|| (+ second order)``, ||R|| <= R_b below; the leading part
   moves by ``sum_{i<k} (d lambda_i + 2 lambda_i vec_b_i)``; the product itself is item 11.
11. gpemu_truncation_cov alone: lambda_r v_rg rounded once, then one fma chain of K = n_comp - n_pc terms:
   ``|d cov_fg| <= (K + 2) u sum_r |v_rf| |lambda_r| |v_rg|``.

Certificate bounds (Kind B), from the same items:
   - cosines between data columns that are not both residue: ``<= tau``;
   - orthogonality of the rotation part: ``||.||_F <= 2 rounds beta sqrt(n) (1 + 1e-3)`` (+ (m + 4) u sqrt(n) where the
     host normalised the rows);
   - ``||R||_F <= R_b = eta_in + rounds beta (||Xc||_F + sigma_1 sqrt(n)) + 4 u ||Xc||_F``.
     Both are held as whole-matrix Frobenius norms.  Per column the same items give no more: one encounter perturbs a
     column by at most beta times the Frobenius norm of its PAIR, which is bounded by ||Xc||_F (sqrt(n) for the rotation
     part) and by nothing smaller that is known beforehand, so the provable bound of a column equals the bound of the
     total and "largest column <= bound" is implied by it.  The largest column norms are reported (``_info``).
   - forward bound.  Let S' C' keep the columns that are not residue, S' = S^ D with unit columns S^, x_S = the
     Frobenius norm of the off-diagonal cosines of S', x_E = ||C' C'^T - I||_F, R' = Xc - S' C'.  Ostrowski (the
     multiplicative form: sigma_i(A B) lies between sigma_i(A) sigma_min(B) and sigma_i(A) sigma_max(B)) on
     S' C' = S^ D (C' C'^T)^(1/2) W, W with orthonormal rows, gives sigma_i(S' C') / d_i between
     sqrt((1 - x_S)(1 - x_E)) and sqrt((1 + x_S)(1 + x_E)); Weyl gives |sigma_i(Xc) - sigma_i(S' C')| <= ||R'||_2.  So
         ``|sigma_i(Xc) - d_i| <= ||R'||_F + d_i ((x_S + x_E) / 2 + (x_S + x_E)^2)``       (d sorted, 0 beyond the kept ones)
     which is asserted against the reference spectrum wherever a reference exists.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
SWEEPS = 30                  # the sweep count the bounds take (and the tests assert)
SECOND_INNER_FROM = 18       # from this sweep on the PB = 16 instance makes two inner sweeps per encounter
ROT_U = 8.0                  # item 6: one rotation, in units of u
GAP_FACTOR = 1.5             # item 9: separation a case must give its leading singular values
CONST_MARGIN = 100.0         # item 3
REF_COS = 1e-18


# ---- the device's documented launch geometry ----------------------------------------------------------------
@dataclass(frozen=True)
class Geometry:
    N: int
    F: int
    m: int
    n: int
    transposed: bool
    PB: int
    nb: int
    inner: int

    @property
    def rounds(self):
        return SWEEPS * (self.nb - 1)

    @property
    def inner_mean(self):
        """inner sweeps per encounter averaged over the SWEEPS sweeps the bounds take: the PB = 16 instance makes one in
        sweeps 0 .. 17 and two from sweep 18 on, the PB = 32 instance always two"""
        if self.PB != 16:
            return float(self.inner)
        return (SECOND_INNER_FROM * 1 + (SWEEPS - SECOND_INNER_FROM) * 2) / SWEEPS

    @property
    def beta(self):
        """item 6, averaged over the sweeps, so that rounds * beta is the sum over all encounters"""
        pp = 2 * self.PB
        return math.sqrt(pp) * U * (pp + ROT_U * self.inner_mean * (pp - 1))

    @property
    def tau(self):
        return 4.0 * math.sqrt(self.m) * EPS + (16 * math.ceil(self.m / 64) + 10) * U

    def residue_threshold(self, fro):
        return 4.0 * math.sqrt(self.m) * EPS * float(fro)


def geometry(N, F):
    tw = N < F
    m, n = (F, N) if tw else (N, F)
    PB = 16 if n <= 1024 else 32
    nb = max(2, 2 * math.ceil(n / (2 * PB)))
    return Geometry(N=N, F=F, m=m, n=n, transposed=tw, PB=PB, nb=nb, inner=1 if PB == 16 else 2)


# ---- extended-precision pieces ------------------------------------------------------------------------------------------
def scaler_ld(Y):
    """(mean, var, scale, constant, margin) by sklearn's StandardScaler formulas in longdouble; margin = how many times
    the variance lies above (not constant) or below (constant) the _is_constant_feature threshold"""
    Y = np.asarray(Y, dtype=LD)
    N = Y.shape[0]
    mean = Y.sum(axis=0) / LD(N)
    var = ((Y - mean) ** 2).sum(axis=0) / LD(N)
    eps = LD(EPS)
    thr = LD(N) * eps * var + (LD(N) * mean * eps) ** 2
    constant = var <= thr
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(constant, np.where(var > 0, thr / var, np.inf), np.where(thr > 0, var / thr, np.inf))
    scale = np.sqrt(var)
    scale = np.where(constant | (scale == 0), LD(1), scale)
    return mean, var, scale, constant, margin.astype(np.float64)


def centred_ld(Y):
    """(Xc, pca_mean) in longdouble: standardise, centre"""
    mean, _, scale, _, _ = scaler_ld(Y)
    Ys = (np.asarray(Y, dtype=LD) - mean) / scale
    pm = Ys.sum(axis=0) / LD(Ys.shape[0])
    return Ys - pm, pm


def jacobi_svd_ld(A, tol=REF_COS, max_sweeps=60):
    """Thin SVD of A (m x n, m >= n) in longdouble by cyclic one-sided Jacobi, the n / 2 disjoint pairs of a tournament
    round rotated together.  Returns (W, V, sigma, cos_max, sweeps): W = A V with mutually orthogonal columns sorted by
    norm, sigma their norms.  Columns shorter than 4 sqrt(m) eps_ld ||A||_F (exact zeros included) are not rotated
    against each other."""
    W = np.array(A, dtype=LD)
    m, n = W.shape
    V = np.eye(n, dtype=LD)
    eps_ld = float(np.finfo(LD).eps)
    floor = 4.0 * math.sqrt(m) * eps_ld
    noise2 = (LD(floor) * np.sqrt((W * W).sum())) ** 2
    npl = n + (n & 1)
    history = []
    for sweep in range(max_sweeps):
        players = list(range(npl))
        worst = 0.0
        for _ in range(npl - 1):
            p = np.array(players[:npl // 2])
            q = np.array(players[npl // 2:][::-1])
            keep = (p < n) & (q < n)
            p, q = p[keep], q[keep]
            players = [players[0], players[-1]] + players[1:-1]
            if p.size == 0:
                continue
            Wp, Wq = W[:, p], W[:, q]
            a, b, g = (Wp * Wp).sum(axis=0), (Wq * Wq).sum(axis=0), (Wp * Wq).sum(axis=0)
            den = np.sqrt(a * b)
            live = (den > 0) & (g != 0) & ((a > noise2) | (b > noise2))
            if not live.any():
                continue
            cosv = np.where(live, np.abs(g) / np.where(den > 0, den, LD(1)), LD(0))
            worst = max(worst, float(cosv.max()))
            gs = np.where(live, g, LD(1))
            zeta = (b - a) / (2 * gs)
            t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            t = np.where(live, t, LD(0))
            c = 1 / np.sqrt(1 + t * t)
            s = c * t
            W[:, p], W[:, q] = c * Wp - s * Wq, s * Wp + c * Wq
            Vp, Vq = V[:, p], V[:, q]
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
        history.append(worst)
        if worst < tol:
            break
        # m-term longdouble dot products resolve a cosine to about sqrt(m) eps_ld: stop where it no longer falls
        if worst < floor and len(history) >= 2 and worst >= 0.5 * history[-2]:
            break
    else:
        raise RuntimeError(f"jacobi_svd_ld: no convergence, largest cosine {history[-1]:.3e}")
    sigma = np.sqrt((W * W).sum(axis=0))
    order = np.argsort(-sigma, kind="stable")
    return W[:, order], V[:, order], sigma[order], history[-1], len(history)


# ---- split-operand products --------------------------------------------------------------------------------------------
def _split3(A, axis, T):
    """A = head + mid + rest along the inner dimension `axis`: head and mid are integers below 2^T times a power of two
    fixed per slice (2^(e - T), 2^(e - 2 T) with max|slice| < 2^e), so products of two of them sum exactly in float64"""
    amax = np.max(np.abs(A), axis=axis, keepdims=True)
    _, e = np.frexp(amax)
    s1, s2 = np.ldexp(1.0, T - e), np.ldexp(1.0, 2 * T - e)
    head = np.trunc(A * s1) / s1
    t = A - head
    mid = np.trunc(t * s2) / s2
    return head, mid, t - mid


def xmatmul(A, B):
    """A @ B (float64 operands) to about 2^-62 of rowmax|A| colmax|B| K, as longdouble: the rows of A and the columns of
    B are split into pieces of T = floor((52 - ceil(log2 K)) / 2) bits, the float64 BLAS products of two such pieces are
    exact, and the nine products are added smallest first in longdouble."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    K = A.shape[1]
    assert B.shape[0] == K
    if K == 0:
        return np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    T = (52 - max(1, math.ceil(math.log2(max(K, 2))))) // 2
    a, b = _split3(A, 1, T), _split3(B, 0, T)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for i, j in ((2, 2), (1, 2), (2, 1), (0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)):
        out += (a[i] @ b[j]).astype(LD)
    return out


def xgram(S):
    """S^T S in extended precision"""
    return xmatmul(np.ascontiguousarray(S.T), S)


# ---- the reference and its bounds -------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Reference:
    geo: Geometry
    n_pc: int
    flip_u: bool
    scaler_mean: np.ndarray      # longdouble (F,)
    scaler_var: np.ndarray
    scaler_scale: np.ndarray
    constant: np.ndarray         # bool (F,)
    const_margin: np.ndarray     # float64 (F,)
    pca_mean: np.ndarray
    Xc: np.ndarray               # longdouble (N, F)
    sigma: np.ndarray            # longdouble (n,)
    components: np.ndarray       # longdouble (n, F), signed by the rule; rows of (numerically) zero sigma are not defined
    scores: np.ndarray           # longdouble (N, n)
    ev: np.ndarray
    evr: np.ndarray              # NaN where the total variance is exactly 0
    flip_argmax: np.ndarray      # int64 (n_pc,)
    flip_second: np.ndarray      # runner-up index per leading component
    flip_decided: np.ndarray     # bool (n_pc,): the two largest |entries| differ by more than twice the bound
    cos_max: float
    ref_sweeps: int
    fro: float
    min_gap_factor: float
    trunc_cov: np.ndarray        # longdouble (F, F): Xc^T Xc / (N - 1) - sum_{i < n_pc} lambda_i v_i v_i^T
    # bounds (float64)
    mean_b: np.ndarray
    var_b: np.ndarray
    scale_b: np.ndarray
    pmean_b: np.ndarray
    eta_in: float
    ev_b: np.ndarray
    evr_b: np.ndarray
    vec_b: np.ndarray            # (n_pc,)
    score_b: np.ndarray          # (n_pc,)
    E_b: float
    R_b: float
    trunc_b: float               # scalar part of item 10 (the product's own term is added per element)


def _f(x):
    return np.asarray(x, dtype=np.float64)


def scaler_bounds(Y, mean, var, scale, constant):
    """items 1-5: (mean_b, var_b, scale_b, pmean_b, dXc) from the longdouble statistics"""
    Yl = np.asarray(Y, dtype=LD)
    N = Yl.shape[0]
    mean_b = N * U * _f(np.abs(Yl).sum(axis=0)) / N
    t = _f(np.abs(Yl - mean)) + mean_b
    sum_t2, sum_t = (t * t).sum(axis=0), t.sum(axis=0)
    d_corr = N * U * sum_t
    corr = N * mean_b + d_corr
    unnorm = _f(var) * N
    var_b = ((N + 2) * U * sum_t2 + 2 * corr * d_corr / N + 2 * U * corr ** 2 / N + U * unnorm) / N + U * _f(var)
    sc = _f(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale_b = np.where(constant, 0.0, var_b / (2 * np.sqrt(_f(var))) + U * sc)
    rho = scale_b / sc
    xc = _f(np.abs((Yl - mean) / scale))           # |ys|; the exact pca mean is 0 (to the reference's rounding)
    a = xc + mean_b / sc
    pmean_b = mean_b / sc + (N + 3) * U * a.mean(axis=0)
    dXc = (rho + U) * xc + 2 * U * a + (N + 2) * U * a.mean(axis=0)
    return mean_b, var_b, scale_b, pmean_b, dXc


def _flip(components, scores, k, flip_u, vec_b, score_b):
    """the sign rule on the k leading components: (argmax, runner-up, decided, sign)"""
    arg, second, decided, sign = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, bool), np.ones(k)
    for i in range(k):
        row = scores[:, i] if flip_u else components[i]
        mag = _f(np.abs(row))
        order = np.argsort(-mag, kind="stable")
        arg[i] = order[0]
        second[i] = order[1] if mag.size > 1 else order[0]
        b = score_b[i] if flip_u else vec_b[i]
        decided[i] = mag.size == 1 or mag[order[0]] - mag[order[1]] > 2 * b
        sign[i] = -1.0 if row[arg[i]] < 0 else 1.0
    return arg, second, decided, sign


def reference(Y, n_pc, flip_u=False):
    """The Kind A reference of one case (min(N, F) <= ~100: the longdouble Jacobi is O(m n^2) per sweep in numpy)."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    N, F = Y.shape
    geo = geometry(N, F)
    m, n = geo.m, geo.n
    mean, var, scale, constant, margin = scaler_ld(Y)
    Xc, pm = centred_ld(Y)
    mean_b, var_b, scale_b, pmean_b, dXc = scaler_bounds(Y, mean, var, scale, constant)
    eta_in = float(np.sqrt((dXc * dXc).sum()))
    A = Xc.T if geo.transposed else Xc
    W, V, sigma, cos_max, sweeps = jacobi_svd_ld(A)
    fro = float(np.sqrt((Xc * Xc).sum()))
    s1 = float(sigma[0])
    live = sigma > 0
    Wn = np.where(live, W / np.where(live, sigma, LD(1)), LD(0))
    if geo.transposed:
        components, scores = Wn.T.copy(), V * sigma
    else:
        components, scores = V.T.copy(), W.copy()
    ev = sigma * sigma / LD(N - 1)
    total = (Xc * Xc).sum() / LD(N - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        evr = ev / total if total > 0 else np.full(n, np.nan, dtype=LD)

    # items 6-9
    rounds, beta, tau = geo.rounds, geo.beta, geo.tau
    eta_ref = s1 * n * cos_max                     # the reference's own non-orthogonality, as a backward error
    eta_jac = rounds * beta * fro
    sg = _f(sigma)
    eta_sigma = eta_in + eta_jac + eta_ref + sg * (n * tau / 2 + (m + 3) * U)
    ev_b = (2 * sg * eta_sigma + eta_sigma ** 2) / (N - 1) + 3 * U * _f(ev)
    eta_F = eta_in + eta_jac + eta_ref + fro * (m + 3) * U
    tot = float(total)
    total_b = (2 * fro * eta_F + eta_F ** 2) / (N - 1) + (n + 3) * U * tot
    with np.errstate(divide="ignore", invalid="ignore"):
        evr_b = ev_b / tot + _f(ev) * total_b / tot ** 2 + U * _f(evr) if tot > 0 else np.zeros(n)
    eta_A = eta_in + eta_jac + eta_ref + s1 * n * tau / 2
    k = int(n_pc)
    gap, factor = np.full(k, np.inf), np.inf
    for i in range(k):
        others = np.delete(sg, i)
        if others.size:
            gap[i] = min(sg[i], float(np.min(np.abs(sg[i] - others))))
            big, small = np.maximum(sg[i], others), np.minimum(sg[i], others)
            with np.errstate(divide="ignore"):
                factor = min(factor, float(np.min(np.where(small > 0, big / np.where(small > 0, small, 1.0), np.inf))))
        else:
            gap[i] = sg[i]
    vec_b = 2 * eta_A / gap + rounds * beta * math.sqrt(n) + (m + 4) * U
    score_b = sg[:k] * vec_b + eta_sigma[:k]
    arg, second, decided, sign = _flip(components, scores, k, flip_u, vec_b, score_b)
    components[:k] *= sign[:, None].astype(LD)
    scores[:, :k] *= sign[None, :].astype(LD)

    E_b = 2 * rounds * beta * math.sqrt(n) * (1 + 1e-3) + (m + 4) * U * math.sqrt(n)
    R_b = eta_in + rounds * beta * (fro + s1 * math.sqrt(n)) + 4 * U * fro
    lead = (components[:k].T * ev[:k]) @ components[:k]
    trunc = Xc.T @ Xc / LD(N - 1) - lead
    trunc_b = (s1 * s1 * n * tau + 2 * s1 * R_b + R_b ** 2) / (N - 1) + float(np.sum(ev_b[:k] + 2 * _f(ev[:k]) * vec_b))
    return Reference(geo=geo, n_pc=k, flip_u=flip_u, scaler_mean=mean, scaler_var=var, scaler_scale=scale,
                     constant=constant, const_margin=margin, pca_mean=pm, Xc=Xc, sigma=sigma, components=components,
                     scores=scores, ev=ev, evr=evr, flip_argmax=arg, flip_second=second, flip_decided=decided,
                     cos_max=cos_max, ref_sweeps=sweeps, fro=fro, min_gap_factor=factor, trunc_cov=trunc,
                     mean_b=mean_b, var_b=var_b, scale_b=scale_b, pmean_b=pmean_b, eta_in=eta_in, ev_b=ev_b, evr_b=evr_b,
                     vec_b=vec_b, score_b=score_b, E_b=E_b, R_b=R_b, trunc_b=trunc_b)


# ---- Kind A -------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 and x / 0 = inf"""
    err, bound = _f(err), np.broadcast_to(_f(bound), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def ratios_a(out, ref: Reference, trunc=None):
    """{output: max |out - reference| / bound} over the Kind A outputs; `out` as gpemu.fit.pca_fit returns it (all
    min(N, F) components); `trunc` = truncation_cov(out components, out explained_variance, n_pc) if it was formed"""
    k, n = ref.n_pc, ref.geo.n
    r = {
        "scaler_mean": _ratio(np.abs(out["scaler_mean"] - ref.scaler_mean), ref.mean_b),
        "scaler_var": _ratio(np.abs(out["scaler_var"] - ref.scaler_var), ref.var_b),
        "scaler_scale": _ratio(np.abs(out["scaler_scale"] - ref.scaler_scale), ref.scale_b),
        "pca_mean": _ratio(np.abs(out["pca_mean"] - ref.pca_mean), ref.pmean_b),
        "explained_variance": _ratio(np.abs(out["explained_variance"][:n] - ref.ev), ref.ev_b),
    }
    if np.isnan(_f(ref.evr)).all():
        r["explained_variance_ratio"] = 0.0 if np.isnan(out["explained_variance_ratio"][:n]).all() else np.inf
    else:
        r["explained_variance_ratio"] = _ratio(np.abs(out["explained_variance_ratio"][:n] - ref.evr), ref.evr_b)
    if k:
        comp, sc = out["components"][:k], out["Y_pca"][:, :k]
        # the sign is the rule's (flip_violations); the vectors are compared up to it
        s = np.where(np.sum(_f(ref.components[:k]) * comp, axis=1) < 0, -1.0, 1.0)
        r["components"] = _ratio(np.abs(comp * s[:, None] - ref.components[:k]), ref.vec_b[:, None])
        r["scores"] = _ratio(np.abs(sc * s[None, :] - ref.scores[:, :k]), ref.score_b[None, :])
    if trunc is not None:
        C, lam = np.abs(out["components"][k:n]), np.abs(out["explained_variance"][k:n])
        own = (n - k + 2) * U * ((C.T * lam) @ C)
        r["truncation_cov"] = _ratio(np.abs(trunc - ref.trunc_cov), ref.trunc_b + own)
    return r


def flip_violations(out, ref: Reference):
    """the sign decisions of the leading components: the index, and the sign it implies"""
    bad = []
    for i in range(ref.n_pc):
        got = int(out["flip_argmax"][i])
        allowed = {int(ref.flip_argmax[i])} if ref.flip_decided[i] else {int(ref.flip_argmax[i]), int(ref.flip_second[i])}
        if got not in allowed:
            bad.append(f"flip_argmax[{i}] = {got}, the reference allows {sorted(allowed)}")
        # the rule on the decomposition's own output: the pick attains the largest magnitude of the row it was made on,
        # and is the FIRST index that does (sklearn's argmax).  The signed outputs have the magnitudes the decision saw,
        # except the u rule's scores of a transposed factorisation, which are the deciding entries times sigma: a
        # rounded product can tie two entries that differed, so there only the maximum is asserted.
        mag = np.abs(out["Y_pca"][:, i] if ref.flip_u else out["components"][i])
        first = int(np.argmax(mag))
        if mag[got] != mag[first]:
            bad.append(f"flip_argmax[{i}] = {got} is not at the largest |entry| of its own output ({first})")
        elif got != first and not (ref.flip_u and ref.geo.transposed):
            bad.append(f"flip_argmax[{i}] = {got}: the tie with index {first} must go to the first index")
        at = out["Y_pca"][got, i] if ref.flip_u else out["components"][i, got]
        if not at >= 0:
            bad.append(f"component {i} is negative ({at:.3e}) at its deciding index {got}")
        if ref.flip_decided[i] and np.sum(_f(ref.components[i]) * out["components"][i]) <= 0:
            bad.append(f"component {i} has the sign opposite to the reference's although the decision is clear")
    return bad


def decision_violations(out, ref: Reference):
    """the constant-feature decision: scale exactly 1 where the reference calls the feature constant, and only there
    (a non-constant column whose scale happens to be 1 would need var = 1 exactly: the case table has none)"""
    dev = out["scaler_scale"] == 1.0
    want = np.asarray(ref.constant)
    return [f"feature {j}: device constant={bool(dev[j])}, reference {bool(want[j])}" for j in np.flatnonzero(dev != want)]


def violations_a(out, ref, trunc=None):
    bad = [f"{name}: error / bound = {v:.3g}" for name, v in ratios_a(out, ref, trunc).items() if not v <= 1.0]
    return bad + flip_violations(out, ref) + decision_violations(out, ref)


# ---- Kind B -------------------------------------------------------------------------------------------------------------
def certificates(out, Xc, geo: Geometry, sigma_ref=None):
    """{check: value / bound} of a decomposition from its outputs (all min(N, F) components) and the longdouble Xc;
    with sigma_ref (a reference spectrum) also the forward bound.  Also returned under "_info": the raw figures."""
    m, n, N, F = geo.m, geo.n, geo.N, geo.F
    S, C = np.ascontiguousarray(out["Y_pca"][:, :n]), np.ascontiguousarray(out["components"][:n])
    Xc = np.asarray(Xc, dtype=LD)
    fro = float(np.sqrt((Xc * Xc).sum()))
    thr = geo.residue_threshold(fro)
    G = xgram(S)
    d = np.sqrt(np.diag(G))
    kept = _f(d) > thr
    nk = int(kept.sum())
    rounds, beta, tau = geo.rounds, geo.beta, geo.tau
    rot_b = 2 * rounds * beta * math.sqrt(n) * (1 + 1e-3) + (m + 4) * U * math.sqrt(n)
    s1 = float(d.max()) if n else 0.0
    info = {"residue": n - nk, "threshold": thr, "fro": fro}

    def cosines(Gm, live):
        dd = np.sqrt(np.diag(Gm))
        den = np.outer(dd, dd)
        with np.errstate(divide="ignore", invalid="ignore"):
            cm = np.where(den > 0, Gm / np.where(den > 0, den, LD(1)), LD(0))
        cm = cm[np.ix_(live, live)].copy()
        np.fill_diagonal(cm, 0)
        return cm

    def fnorm(M):
        return float(np.sqrt((M * M).sum()))

    cosS = cosines(G, kept)
    CCt = xmatmul(C, np.ascontiguousarray(C.T))
    E = CCt - np.eye(n, dtype=LD)
    E_kept = E[np.ix_(kept, kept)]
    x_S, x_E = fnorm(cosS), fnorm(E_kept)
    if geo.transposed:
        # data columns = rows of C (normalised by the host); rotation part = columns of S (scaled by sigma: cosines are
        # scale-free, and defined for every column that is not exactly zero)
        data_cos = cosines(CCt, kept)
        rot_norm = fnorm(cosines(G, _f(d) > 0))
        info["norm_err"] = float(np.max(np.abs(np.diag(E_kept)))) if nk else 0.0
    else:
        data_cos = cosS
        rot_norm = fnorm(E)
    cmax = float(np.max(np.abs(data_cos))) if nk > 1 else 0.0
    R = Xc - xmatmul(S, C)
    Rn = float(np.sqrt((R * R).sum()))
    Rk = Xc - xmatmul(S[:, kept], C[kept]) if nk < n else R
    Rkn = float(np.sqrt((Rk * Rk).sum()))
    info.update(cos_max=cmax, rot_norm=rot_norm, R=Rn, R_kept=Rkn, x_S=x_S, x_E=x_E,
                R_col_max=float(np.sqrt((R * R).sum(axis=0).max())) if R.size else 0.0,
                E_col_max=float(np.sqrt((E * E).sum(axis=0).max())) if E.size else 0.0)
    r = {"cosines": cmax / tau, "rotation_orthogonality": rot_norm / rot_b, "_info": info}
    r["_R"] = Rn
    if sigma_ref is not None:
        dk = np.sort(_f(d[kept]))[::-1]
        dfull = np.concatenate([dk, np.zeros(n - nk)])
        x = x_S + x_E
        fwd = Rkn + dfull * (x / 2 + x * x)
        err = np.abs(_f(sigma_ref) - dfull)
        r["forward"] = _ratio(err, fwd * (1 + 1e-6) + 4 * float(np.finfo(LD).eps) * s1 * n)
        info["forward_bound_rel"] = float(np.max(fwd) / s1) if s1 > 0 else 0.0
    return r


def R_bound_without_reference(Y, geo: Geometry):
    """item 5 + the R_b of the module docstring for a case that has no longdouble SVD: sigma_1 <= ||Xc||_F"""
    mean, var, scale, constant, _ = scaler_ld(Y)
    dXc = scaler_bounds(Y, mean, var, scale, constant)[4]
    eta_in = float(np.sqrt((dXc * dXc).sum()))
    Xc, _ = centred_ld(Y)
    fro = float(np.sqrt((Xc * Xc).sum()))
    return eta_in + geo.rounds * geo.beta * fro * (1 + math.sqrt(geo.n)) + 4 * U * fro


def violations_b(cert, R_b):
    r = {k: v for k, v in cert.items() if not k.startswith("_")}
    r["R"] = cert["_R"] / R_b if R_b > 0 else (0.0 if cert["_R"] == 0 else np.inf)
    return r, [f"{name}: value / bound = {v:.3g}" for name, v in r.items() if not v <= 1.0]


# ---- gpemu_truncation_cov alone (item 11) ------------------------------------------------------------------------------
def truncation_cov_ld(components, ev, n_pc):
    """(S_{>k} diag(ev_{>k}) S_{>k}^T in longdouble, its elementwise bound) from the float64 operands"""
    C = np.asarray(components, dtype=LD)[n_pc:]
    lam = np.asarray(ev, dtype=LD)[n_pc:]
    K = C.shape[0]
    val = (C.T * lam) @ C
    bound = (K + 2) * U * _f((np.abs(C).T * np.abs(lam)) @ np.abs(C))
    return val, bound
