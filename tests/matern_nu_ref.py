"""CPU restatement of the Matern kernel of general smoothness nu, for the tests (numpy + scipy.special.kv).

sklearn's Matern (skl kernels.py:1708-1781): nu in {0.5, 1.5, 2.5} closed forms, nu = inf exp(-d^2 / 2), else
    K = 2^(1 - nu) / Gamma(nu) t^nu K_nu(t),  t = sqrt(2 nu) d,  d = 0 -> eps (kernels.py:1725-1733),
and, on the training set, the diagonal filled with 1 (kernels.py:1735-1737); GaussianProcessRegressor (skl _gpr.py)
does the rest.  The oracle (oracle/gp_oracle.py) knows the closed forms only: ``general_nu()`` lends it this base
kernel for the duration of a ``with`` block, so that its fit / predict / log-posterior restatements serve every nu.
The gradient sklearn takes by a forward difference (kernels.py:1767-1774, ``_approx_fprime``, step 1e-10) is
restated here as that difference of ``lml``.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
from scipy.linalg import cho_solve, cholesky
from scipy.special import gamma, kv

from oracle import gp_oracle as O

CLOSED = (0.5, 1.5, 2.5)


def matern(dists, nu):
    """base kernel from euclidean distances (skl kernels.py:1715-1733)"""
    dists = np.asarray(dists, dtype=np.float64)
    if nu == 0.5:
        return np.exp(-dists)
    if nu == 1.5:
        K = dists * math.sqrt(3)
        return (1.0 + K) * np.exp(-K)
    if nu == 2.5:
        K = dists * math.sqrt(5)
        return (1.0 + K + K ** 2 / 3.0) * np.exp(-K)
    if np.isinf(nu):
        return np.exp(-(dists ** 2) / 2.0)
    K = dists.copy()
    K[K == 0.0] += np.finfo(float).eps
    tmp = math.sqrt(2 * nu) * K
    K.fill((2 ** (1.0 - nu)) / gamma(nu))
    K *= tmp ** nu
    K *= kv(nu, tmp)
    return K


_orig_base = O._base_from_dists


def _base(dists, spec):
    if spec.kind == O.MATERN and spec.nu not in CLOSED:
        return matern(dists, spec.nu)
    return _orig_base(dists, spec)


@contextlib.contextmanager
def general_nu():
    """the oracle's base kernel extended to every nu (without gradients: see lml_grad_fd)"""
    O._base_from_dists = _base
    try:
        yield
    finally:
        O._base_from_dists = _orig_base


def kernel_matrix(X, theta, spec, jitter=0.0):
    """kernel_(X) + jitter I (the library's gpemu_kernel_matrix)"""
    with general_nu():
        ls, const, noise = O.split_theta(np.asarray(theta), X.shape[1], spec)
        K = O.kernel_train(X, ls, spec, const, noise)
    K[np.diag_indices_from(K)] += jitter
    return K


def lml(X, y, theta, spec, jitter=1e-10):
    """log_marginal_likelihood(theta) (skl _gpr.py:580-613); -inf where K is not positive definite"""
    K = kernel_matrix(X, theta, spec, jitter)
    try:
        L = cholesky(K, lower=True, check_finite=False)
    except np.linalg.LinAlgError:
        return -np.inf
    a = cho_solve((L, True), y, check_finite=False)
    return -0.5 * y.dot(a) - np.log(np.diag(L)).sum() - X.shape[0] / 2 * np.log(2 * np.pi)


def lml_grad_central(X, y, theta, spec, h=1e-5, jitter=1e-10):
    """central difference of lml in theta (the check on the device's analytic gradient)"""
    theta = np.asarray(theta, dtype=np.float64)
    g = np.empty_like(theta)
    for i in range(theta.size):
        e = np.zeros_like(theta)
        e[i] = h
        g[i] = (lml(X, y, theta + e, spec, jitter) - lml(X, y, theta - e, spec, jitter)) / (2 * h)
    return g


def lml_grad_fd(X, y, theta, spec, jitter=1e-10):
    """sklearn's gradient for the general nu: the kernel's forward difference with step 1e-10 (kernels.py:1767-1774)
    carried through skl _gpr.py:625-647 (the kernel's constant and noise parts exactly)"""
    N, d = X.shape
    theta = np.asarray(theta, dtype=np.float64)
    with general_nu():
        ls, const, noise = O.split_theta(theta, d, spec)
        K = O.kernel_train(X, ls, spec, const, noise)
        Kb = O.kernel_train(X, ls, O.KernelSpec(spec.kind, spec.nu, False, False), 0.0, 0.0)
        dK = []
        for i in range(d):
            ls2 = np.exp(np.log(ls) + 1e-10 * (np.arange(d) == i))
            dK.append((O.kernel_train(X, ls2, O.KernelSpec(spec.kind, spec.nu, False, False), 0.0, 0.0) - Kb) / 1e-10)
    if spec.has_const:
        dK.append(np.full((N, N), const))
    if spec.has_noise:
        dK.append(noise * np.eye(N))
    K[np.diag_indices_from(K)] += jitter
    L = cholesky(K, lower=True, check_finite=False)
    a = cho_solve((L, True), y, check_finite=False)
    inner = np.outer(a, a) - cho_solve((L, True), np.eye(N), check_finite=False)
    return np.array([0.5 * np.einsum("ij,ji->", inner, G) for G in dK])
