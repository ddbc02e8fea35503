"""-m gpu: every launch path of the fit side against the extended-precision reference of tests/fit_ref.py.

Each case of tests/fit_cases.py names the path it is there for; the dispatch rules restated there say which paths an
evaluation must take, and gpemu_fit_path_counts deltas show that it did.  Per element, |dev - ref| <= bound for K, the
Cholesky residual, W = L^-1, K^-1, alpha, the log-marginal likelihood and every gradient component; batches are checked
member by member; a workspace filled with NaN bytes before an evaluation must change nothing.  The largest err/bound per
family is printed (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as FR
import path_cases as PC
from gpemu import _lib
from gpemu.fit import DeviceFit, LinAlgError, cholesky, kernel_matrix

pytestmark = pytest.mark.gpu

LD = np.longdouble
ENV_KEYS = ("GPEMU_CHOL_PANEL", "GPEMU_CHOL_HEADS_ONE_XCD", "GPEMU_CHOL_LOOKAHEAD")


WIDE = ("FIT_KMAT", "FIT_GRAD")    # of enum gpemu_wide_path (path_cases.WIDE_PATHS)
ALL_PATH = dict(FC.FIT_PATH, **{"WIDE_" + p: len(FC.FIT_PATHS) + i for i, p in enumerate(WIDE)})


def counts():
    """gpemu_fit_path_counts, then gpemu_wide_path_counts' FIT_KMAT and FIT_GRAD (the keys of ALL_PATH)"""
    out = np.zeros(len(FC.FIT_PATHS), dtype=np.int64)
    n = _lib.lib().gpemu_fit_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    assert n == len(FC.FIT_PATHS), "enum gpemu_fit_path and tests/fit_cases.FIT_PATHS disagree"
    wide = np.zeros(len(PC.WIDE_PATHS), dtype=np.int64)
    n = _lib.lib().gpemu_wide_path_counts(wide.ctypes.data_as(C.POINTER(C.c_int64)), wide.size)
    assert n == len(PC.WIDE_PATHS), "enum gpemu_wide_path and tests/path_cases.WIDE_PATHS disagree"
    return np.concatenate([out, wide[[PC.WIDE_PATH[p] for p in WIDE]]])


def assert_deltas(delta, expected, what):
    got = {p: int(delta[ALL_PATH[p]]) for p in expected}
    assert got == expected, f"{what}: path counts {got}, expected {expected}"


def within(what, dev, ref, bound):
    err = FR.err_ld(dev, ref) if ref is not None else np.abs(np.asarray(dev, dtype=np.float64))
    r = FR.ratio(err, bound)
    worst = np.unravel_index(np.argmax(r), r.shape) if r.ndim else ()
    assert np.all(np.isfinite(np.asarray(dev, dtype=np.float64))), f"{what}: not finite"
    assert r.max() <= 1.0, (f"{what}: max err/bound {r.max():.3g} at {worst}: dev {np.asarray(dev)[worst]!r} "
                            f"ref {None if ref is None else float(np.asarray(ref)[worst])!r} "
                            f"bound {np.asarray(bound)[worst]:.3g}")
    return float(r.max())


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def device_fit(c, p):
    return DeviceFit(p.X, kernel_kind=c.kind, nu=c.nu, has_const=c.const, has_noise=c.noise, jitter=c.jitter)


def check_member(what, ref, p, Ld, Wd, Kid, lml, grad):
    """one problem of an evaluation, per element, against its FitRef; returns the ratios"""
    N = ref.N
    out = {}
    R, B = FR.chol_residual(p, Ld, np.arange(N))
    out["L_res"] = within(what + " L residual", R, None, B)
    aW, aL = np.abs(Wd), np.abs(Ld)
    out["W"] = within(what + " W", Wd, FR.tri_inv_ld(Ld), FR.g(N) * (aW @ (aL @ aW)))
    R, B = FR.inverse_residual(Wd, Ld, np.arange(N))
    out["W_res"] = within(what + " W residual", R, None, B)
    tri = np.tril_indices(N)
    out["Kinv"] = within(what + " K^-1", Kid[tri], ref.Kinv[tri], ref.d_Kinv[tri])
    out["lml"] = within(what + " lml", lml, ref.lml, ref.d_lml)
    out["grad"] = within(what + " grad", grad, ref.grad, ref.d_grad)
    return out


CASES = FC.cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_fit_path_against_extended_reference(c, monkeypatch):
    p = FC.problem(c)
    ref = FR.FitRef(p) if c.full else None
    set_env(monkeypatch, c.env)
    N = c.N

    c0 = counts()
    K = kernel_matrix(p.X, p.theta, c.kind, c.nu, c.const, c.noise, c.jitter)
    d = counts() - c0
    assert_deltas(d, FC.kmat_paths(c), c.name + " kernel_matrix")

    f = device_fit(c, p)
    c0 = counts()
    lml, grad = f.lml(p.y, p.theta)
    assert_deltas(counts() - c0, FC.fit_paths(c), c.name + " lml")
    Ld, Wd, Kid = f.workspace("L"), f.workspace("W"), f.workspace("Kinv")
    c0 = counts()
    L2, alpha, lml2 = f.factor(p.y, p.theta)
    assert_deltas(counts() - c0, FC.fit_paths(c, grad=False), c.name + " factor")
    assert np.array_equal(L2, Ld) and lml2 == lml, "factor and lml disagree on the same evaluation"
    f.close()

    ratios = {}
    if c.full:
        ratios["K"] = within("K", K, ref.K, ref.dK)
        ratios["alpha"] = within("alpha", alpha, ref.alpha, ref.d_alpha)
        ratios.update(check_member(c.name, ref, p, Ld, Wd, Kid, lml, grad))
    else:
        # the large shapes: residuals on every row at a 64-row block edge and at N - 1
        rows = FR.edge_rows(N)
        K_rows, dK_rows = FR.kernel_rows(p, rows)
        ratios["K"] = within("K rows", K[rows], K_rows, dK_rows)
        R, B = FR.chol_residual(p, Ld, rows)
        ratios["L_res"] = within("L residual", R, None, B)
        R, B = FR.inverse_residual(Wd, Ld, rows)
        ratios["W_res"] = within("W residual", R, None, B)
        assert np.all(np.isfinite(Kid[np.tril_indices(N)])) and np.all(np.isfinite(grad)) and np.isfinite(lml)
    print(f"\nRATIOS {c.name} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def batch_problems(c, n_distinct):
    ps = [FC.problem(c, seed=s) for s in range(n_distinct)]
    for p in ps[1:]:
        p.X = ps[0].X            # one design per handle: the members differ in target and theta
    # a member whose kernel matrix is numerically indefinite (no jitter on these handles): length scales of 1e6 box
    # widths (1e12 for nu < 1, whose kernel leaves 1 as r^(2 nu)) and no noise to speak of make K the all-ones matrix
    # to 1e-12, and rounding turns a pivot non-positive
    bad_theta = ps[0].theta.copy()
    bad_theta[:c.d] = np.log(1e12 if c.nu < 1 else 1e6)
    bad_theta[-1] = -80.0
    return ps, bad_theta


@pytest.mark.parametrize("nb,N,kind,nu,env,d", [
    (3, 129, FC.M, 1.5, {}, 3),
    (8, 273, FC.R, np.inf, {}, 3),
    (8, 320, FC.M, 2.0, {"GPEMU_CHOL_PANEL": "0"}, 3),
    (41, 449, FC.M, 2.5, {}, 3),                   # 41 x 8 blocks > 320: the three-launch steps inside the fit
    (5, 200, FC.M, 2.5, {}, 16),                   # 16-wide members
], ids=["nb3_n129", "nb8_n273", "nb8_n320_nu2_steps", "nb41_n449_steps", "nb5_n200_d16"])
def test_fit_batch_members_against_extended_reference(nb, N, kind, nu, env, d, monkeypatch):
    c = FC.FitCase(f"batch{nb}", N, d, kind, nu, True, True, jitter=0.0)
    ps, bad_theta = batch_problems(c, 3)
    refs = [FR.FitRef(p) for p in ps]
    bad = nb // 2
    src = [z % 3 for z in range(nb)]
    ys = np.stack([ps[s].y for s in src])
    thetas = np.stack([ps[s].theta for s in src])
    thetas[bad] = bad_theta
    set_env(monkeypatch, env)
    f = device_fit(c, ps[0])
    c0 = counts()
    lml, grad, info = f.lml_batch(ys, thetas)
    assert_deltas(counts() - c0, FC.fit_paths(c, nb=nb, env=env), f"batch of {nb}")
    assert info[bad] > 0 and np.all(np.delete(info, bad) == 0), info
    ws = {}
    for z in range(nb):
        if z == bad:
            continue
        ws[z] = (f.workspace("L", z), f.workspace("W", z), f.workspace("Kinv", z))
    f.close()
    worst = {}
    for z, (Ld, Wd, Kid) in ws.items():
        s = src[z]
        first = src.index(s) if src.index(s) != bad else [q for q in range(nb) if src[q] == s and q != bad][0]
        if z != first:
            # the same inputs in another slot of the batch: the same bits
            for a, b in zip(ws[first], (Ld, Wd, Kid)):
                assert np.array_equal(a, b), f"batch member {z} differs from member {first}"
            assert lml[z] == lml[first] and np.array_equal(grad[z], grad[first])
            continue
        r = check_member(f"batch {nb} member {z}", refs[s], ps[s], Ld, Wd, Kid, lml[z], grad[z])
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\nRATIOS batch{nb}_n{N}_d{d} " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("N,kind,nu,env", [
    (273, FC.M, 1.5, {}),
    (320, FC.M, 0.7, {}),
    (1000, FC.R, np.inf, {"GPEMU_CHOL_PANEL": "0"}),
], ids=["n273_m15_panel", "n320_nu07_ragged", "n1000_rbf_steps"])
def test_fit_reads_only_what_it_wrote(N, kind, nu, env, monkeypatch):
    """a workspace full of NaN bytes before the evaluation (single and batch, with gradient; again after a non-positive
    definite evaluation on the same handle) gives the bits of a fresh handle"""
    set_env(monkeypatch, env)
    c = FC.FitCase("poison", N, 4, kind, nu, True, True, jitter=0.0)
    ps, bad_theta = batch_problems(c, 3)
    ys = np.stack([p.y for p in ps])
    thetas = np.stack([p.theta for p in ps])
    fresh = device_fit(c, ps[0])
    l1, g1 = fresh.lml(ps[0].y, ps[0].theta)
    ws1 = [fresh.workspace(w) for w in ("L", "W", "Kinv")]
    lb, gb, ib = fresh.lml_batch(ys, thetas)
    wsb = [fresh.workspace(w, 2) for w in ("L", "W", "Kinv")]
    fresh.close()
    assert np.all(ib == 0)

    f = device_fit(c, ps[0])
    f.lml_batch(ys, thetas)              # the workspace holds three problems
    for rnd in range(2):
        if rnd == 1:
            with pytest.raises(LinAlgError):
                f.lml(ps[0].y, bad_theta)
        f.poison()
        l2, g2 = f.lml(ps[0].y, ps[0].theta)
        assert np.isfinite(l2) and np.all(np.isfinite(g2))
        assert l2 == l1 and np.array_equal(g2, g1), f"round {rnd}: single evaluation after poison differs"
        for a, w in zip(ws1, ("L", "W", "Kinv")):
            b = f.workspace(w)
            assert np.all(np.isfinite(b)) and np.array_equal(a, b), f"round {rnd}: {w} after poison differs"
        f.poison()
        lb2, gb2, ib2 = f.lml_batch(ys, thetas)
        assert np.all(ib2 == 0) and np.array_equal(lb2, lb) and np.array_equal(gb2, gb), f"round {rnd}: batch differs"
        for a, w in zip(wsb, ("L", "W", "Kinv")):
            assert np.array_equal(a, f.workspace(w, 2)), f"round {rnd}: batch member 2 {w} after poison differs"
    f.close()


@pytest.mark.parametrize("N", [65, 320, 1000])
def test_standalone_cholesky_residual(N):
    """gpemu_cholesky: always the three-launch steps; |A - L L^T| <= g(N) |L||L^T| per element"""
    c = FC.FitCase("chol", N, 3, FC.M, 2.5, True, True)
    p = FC.problem(c)
    A, _ = FR.kernel_rows(p, np.arange(N))
    A = np.asarray(A, dtype=np.float64)
    c0 = counts()
    Ld = cholesky(A)
    assert_deltas(counts() - c0, {"CHOL_STEPS": -(-N // 256), "CHOL_PANEL": 0, "CHOL_LOOKAHEAD": 0}, "cholesky")
    R = np.abs(A.astype(LD) - Ld.astype(LD) @ Ld.T.astype(LD)).astype(np.float64)
    aL = np.abs(Ld)
    r = within(f"cholesky N={N} residual", R, None, FR.g(N) * (aL @ aL.T))
    print(f"\nRATIOS cholesky_n{N} L_res={r:.3g}")
