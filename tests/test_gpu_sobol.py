"""-m gpu tests of the global (Sobol') sensitivity on the device (gpemu_gp_mean_pick_freeze, gpemu_sobol_moments,
DeviceModel.sobol_indices, emulation.global_sensitivity) against tests/sobol_ref.py: the
extended-precision pick-freeze means of tests/hp_ref.py with the distance factor of the kernel's form
(``sobol_ref.c_x_pf``), their moments and estimators in longdouble, and the tolerances that follow from the per-row
bounds.  Every reference is computed once per case (``sobol_ref.case_means``); smaller n are prefixes of its rows.

Figures measured on an MI355X are printed by every test before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import sobol_ref as R

pytestmark = pytest.mark.gpu

CASE_NAMES = sorted(R.CASES)
SIZES = (1, 2, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def _dm(name):
    import golden_util as GU
    return GU.device_model(R.case(name)[0])


def _f64(x):
    return np.asarray(x, dtype=np.float64)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pick_freeze_means_against_the_extended_precision_reference(name):
    model, lo, hi, A, B = R.case(name)
    dm, (Zr, eps) = _dm(name), R.case_means(name)
    d, k = A.shape[1], model.n_pc
    worst = 0.0
    for n in SIZES:
        Z = dm.mean_pick_freeze(A[:n], B[:n])
        assert Z.shape == (d + 2, n, k)
        ratio = np.abs(_f64(Z - Zr[:, :n])) / eps[:, :n]
        worst = max(worst, float(ratio.max()))
        print(f"{name} n={n}: max |Z - ref| / eps = {ratio.max():.3e} (planted rows: {ratio[:, :2].max():.3e})")
        assert np.all(ratio <= 1.0), (name, n)
    # the A and B blocks against gp_predict's means (another distance form): within the sum of the two bounds
    import hp_ref as H
    import pp_ref as P
    n = 65
    X = np.concatenate([A[:n], B[:n]])
    with P.oracle_for(model.spec):
        _, _, mb, _, _ = H.gp_predict(X, model)
    mean, _ = dm.gp_predict(X)
    Z = dm.mean_pick_freeze(A[:n], B[:n])
    diff = np.abs(np.concatenate([Z[0], Z[1]]) - mean)
    bound = mb + np.concatenate([eps[0, :n], eps[1, :n]])
    print(f"{name}: A, B blocks vs gp_predict: max diff / (sum of bounds) = {np.max(diff / bound):.3e}; "
          f"worst mean ratio over all n {worst:.3e}")
    assert np.all(diff <= bound)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_moments_against_the_longdouble_moments_about_the_returned_pivot(name):
    model, lo, hi, A, B = R.case(name)
    dm, (Zr, eps) = _dm(name), R.case_means(name)
    n = R.moment_rows(name)
    for T in (1, 4, 16):
        out = dm.sobol_moments(A[:n], B[:n], n_batches=T)
        assert np.array_equal(out["count"], np.bincount(R.batch_of(n, T), minlength=T))
        # the pivot is the mean over the first min(n, 1024) rows of A and B (any value near it serves)
        z0 = _f64(np.concatenate([Zr[0, :n], Zr[1, :n]]).mean(axis=0))
        assert np.all(np.abs(out["pivot"] - z0) <= 1e-9 * (1 + np.abs(z0)))
        ref = R.moments(Zr[:, :n], out["pivot"], T)
        tol = R.moment_tolerances(Zr[:, :n], eps[:, :n], out["pivot"], T)
        for key in ("sumA", "sumB", "C2", "sumD", "M", "D"):
            err = np.abs(_f64(out[key] - ref[key]))
            print(f"{name} n={n} T={T} {key}: max err {err.max():.3e}, max err / tol {np.max(err / tol[key]):.3e}")
            assert np.all(err <= tol[key]), (name, T, key)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_indices_against_the_reference_estimators(name):
    model, lo, hi, A, B = R.case(name)
    dm, (Zr, eps) = _dm(name), R.case_means(name)
    n = R.moment_rows(name)
    d, F = A.shape[1], model.components.shape[1]
    for T in (1, 16):
        out = dm.sobol_indices(A[:n], B[:n], n_batches=T)
        pivot = dm.sobol_moments(A[:n], B[:n], n_batches=T)["pivot"]
        ref, tol = R.indices(Zr[:, :n], eps[:, :n], model, pivot, T)
        print(f"{name} n={n} T={T}: max tol(V) / V = {tol['cond']:.3e}, min V = {_f64(ref['variance']).min():.3e}")
        assert tol["cond"] <= 1e-9
        assert out["first_order"].shape == (d, F) and out["total"].shape == (d, F)
        assert out["variance"].shape == (F,) and out["mean"].shape == (F,)
        assert out["n"] == n and out["n_batches"] == T
        keys = ["first_order", "total", "variance", "mean"] + (["first_order_se", "total_se"] if T > 1 else [])
        for key in keys:
            err = np.abs(_f64(out[key] - ref[key]))
            print(f"{name} n={n} T={T} {key}: max err {err.max():.3e}, max tol {tol[key].max():.3e}, "
                  f"max err / tol {np.max(err / tol[key]):.3e}")
            assert np.all(err <= tol[key]), (name, T, key)
        if T == 1:
            assert np.all(np.isnan(out["first_order_se"])) and np.all(np.isnan(out["total_se"]))


def test_b_equal_a_gives_exact_zeros():
    for name in ("rbf_d6", "matern05_d6", "rbf_d16"):
        model, lo, hi, A, B = R.case(name)
        dm = _dm(name)
        n = 65
        Z = dm.mean_pick_freeze(A[:n], A[:n])
        assert all(np.array_equal(Z[s], Z[0]) for s in range(1, Z.shape[0]))
        m = dm.sobol_moments(A[:n], A[:n], n_batches=4)
        for key in ("M", "D", "sumD"):
            assert not m[key].any(), key
        out = dm.sobol_indices(A[:n], A[:n], n_batches=4)
        assert not out["first_order"].any() and not out["total"].any()
        assert np.all(out["variance"] > 0)
        print(f"{name}: B = A: M, D, sum D, first_order and total are identically 0")


def test_permuting_the_parameters_permutes_the_indices():
    import golden_util as GU
    from oracle import gp_oracle as O
    name = "matern15_d6"
    model, lo, hi, A, B = R.case(name)
    dm, (Zr, eps) = _dm(name), R.case_means(name)
    n = R.moment_rows(name)
    perm = np.array([3, 0, 5, 1, 4, 2])
    gps = [O.GP(ls=gp.ls[perm], const=gp.const, noise=gp.noise, alpha=gp.alpha, L=gp.L) for gp in model.gps]
    pm = O.GroupModel(X_train=np.ascontiguousarray(model.X_train[:, perm]), spec=model.spec, gps=gps,
                      components=model.components, explained_variance=model.explained_variance,
                      scaler_mean=model.scaler_mean, scaler_scale=model.scaler_scale, n_pc=model.n_pc)
    dp = GU.device_model(pm)
    a = dm.sobol_indices(A[:n], B[:n], n_batches=4)
    b = dp.sobol_indices(np.ascontiguousarray(A[:n][:, perm]), np.ascontiguousarray(B[:n][:, perm]), n_batches=4)
    pivot = dm.sobol_moments(A[:n], B[:n], n_batches=4)["pivot"]
    _, tol = R.indices(Zr[:, :n], eps[:, :n], model, pivot, 4)
    for key in ("first_order", "total"):
        err = np.abs(b[key] - a[key][perm])
        print(f"permuted {key}: max err {err.max():.3e}, max err / (2 tol) {np.max(err / (2 * tol[key][perm])):.3e}")
        assert np.all(err <= 2 * tol[key][perm])            # each side within tol of its own exact value
    assert np.all(np.abs(b["variance"] - a["variance"]) <= 2 * tol["variance"])
    dp.close()


def _same(a, b, keys):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def test_results_do_not_depend_on_the_workspace_or_the_run():
    from gpemu.sensitivity import SOBOL_PATHS, sobol_path_counts, sobol_workspace_bytes
    name = "rbf_d6"
    model, lo, hi, _, _ = R.case(name)
    dm = _dm(name)
    n, T, d, k = 4096 + 33, 16, 6, model.n_pc
    rng = np.random.default_rng(5)
    A, B = rng.uniform(lo, hi, (n, d)), rng.uniform(lo, hi, (n, d))
    mkeys = ("pivot", "count", "sumA", "sumB", "C2", "sumD", "M", "D")
    ikeys = ("first_order", "total", "first_order_se", "total_se", "variance", "mean")
    whole = dm.sobol_moments(A, B, n_batches=T)
    _same(whole, dm.sobol_moments(A, B, n_batches=T), mkeys)
    iwhole = dm.sobol_indices(A, B, n_batches=T)
    _same(iwhole, dm.sobol_indices(A, B, n_batches=T), ikeys)
    ic, ik, iw = (SOBOL_PATHS.index(x) for x in ("call", "chunk", "whole"))
    # batches of 258 / 259 rows are two slices of ~129 rows: chunks are whole slices, their edges fall inside batches
    for rows, chunks in ((n, 1), (2100, 2), (1000, 5)):
        c0 = sobol_path_counts()
        out = dm.sobol_moments(A, B, n_batches=T, workspace_bytes=sobol_workspace_bytes(rows, d, k))
        c1 = sobol_path_counts() - c0
        print(f"workspace for {rows} rows: counters {dict(zip(SOBOL_PATHS, c1.tolist()))}")
        assert c1[ic] == 1 and c1[ik] == chunks and c1[iw] == (chunks == 1)
        assert c1[SOBOL_PATHS.index("dp8")] == chunks + 1 and c1[SOBOL_PATHS.index("kind0")] == chunks + 1
        _same(whole, out, mkeys)
        _same(iwhole, dm.sobol_indices(A, B, n_batches=T, workspace_bytes=sobol_workspace_bytes(rows, d, k)), ikeys)


def test_error_paths_of_the_abi_leave_the_model_usable():
    from gpemu import _lib
    from gpemu._lib import ptr
    from gpemu.sensitivity import sobol_path_counts
    name = "rbf_d6"
    model, lo, hi, A, B = R.case(name)
    dm = _dm(name)
    L = _lib.lib()
    d, k, n = 6, model.n_pc, 8
    A8, B8 = np.ascontiguousarray(A[:n]), np.ascontiguousarray(B[:n])
    Z = np.empty((d + 2, n, k))

    def moments(n_, A_, B_, T):
        o = [np.zeros(k), np.zeros(max(T, 1), dtype=np.int64), np.zeros((max(T, 1), k)), np.zeros((max(T, 1), k)),
             np.zeros((max(T, 1), k, k)), np.zeros((max(T, 1), d, k)), np.zeros((max(T, 1), d, k, k)),
             np.zeros((max(T, 1), d, k, k))]
        return L.gpemu_sobol_moments(dm.handle, n_, ptr(A_), ptr(B_), T, 0, *[ptr(x) for x in o])

    bad = A8.copy()
    bad[3, 2] = np.nan
    inf = B8.copy()
    inf[0, 0] = np.inf
    calls = {
        "pick_freeze n = 0": lambda: L.gpemu_gp_mean_pick_freeze(dm.handle, 0, ptr(A8), ptr(B8), ptr(Z)),
        "pick_freeze NaN row": lambda: L.gpemu_gp_mean_pick_freeze(dm.handle, n, ptr(bad), ptr(B8), ptr(Z)),
        "pick_freeze null": lambda: L.gpemu_gp_mean_pick_freeze(dm.handle, n, ptr(A8), None, ptr(Z)),
        "moments n = 0": lambda: moments(0, A8, B8, 1),
        "moments n_batches = 0": lambda: moments(n, A8, B8, 0),
        "moments n_batches > n": lambda: moments(n, A8, B8, n + 1),
        "moments NaN row": lambda: moments(n, bad, B8, 2),
        "moments inf row": lambda: moments(n, A8, inf, 2),
    }
    c0 = sobol_path_counts()
    for label, call in calls.items():
        rc = call()
        msg = _lib.last_error()
        print(f"{label}: rc {rc}, '{msg}'")
        assert rc != 0 and msg, label
    assert np.array_equal(sobol_path_counts(), c0)   # no launch
    with pytest.raises(ValueError):
        dm.sobol_moments(A8, B8, n_batches=n + 1)
    with pytest.raises(ValueError):
        dm.mean_pick_freeze(bad, B8)
    with pytest.raises(ValueError):
        dm.sobol_indices(A8, B8[:4])
    # a model whose d or k is out of range cannot be created (gpemu_model_create refuses d > 16 and k > 64)
    Zr, eps = R.case_means(name)
    assert np.all(np.abs(np.asarray(dm.mean_pick_freeze(A8, B8) - Zr[:, :n], dtype=np.float64)) <= eps[:, :n])


class _GroupCfg:
    def __init__(self, n_pc):
        self.n_pc = n_pc


class _EmuCfg:
    def __init__(self, groups, sorter, analysis_config, parameterization):
        self.emulation_groups_config = groups
        self.sort_observables_in_matrix = sorter
        self.analysis_config = analysis_config
        self.parameterization = parameterization


def test_global_sensitivity_equals_the_groups_indices_scattered_by_the_sorter(tmp_path):
    """emulation.global_sensitivity on the shipped three-group fixture: the per-group sobol_indices on the shared base
    matrices, scattered into the observable order of ``predict``, byte for byte; parameter names from the YAML"""
    import yaml

    import dropin_util as DU
    import golden_util as GU
    from bayesian_inference import emulation
    from gpemu import sensitivity
    g = GU.load("g7_shipped_config")
    names, mapping, block_start, cols = GU.g7_groups(g)
    sorter = emulation.SortEmulationGroupObservables(mapping, tuple(int(v) for v in g["map_shape"]))
    res = {}
    for n in names:
        sub = {k[len(n) + 1:]: v for k, v in g.items() if k.startswith(n + "_")}
        sub.update(design=g["design"], gpr_alpha=g["gpr_alpha"])
        res[n] = DU.results_at_golden_theta(sub)
    d = g["lo"].size
    pnames = [f"par_{i}" for i in range(d)]
    path = tmp_path / "analysis.yaml"
    path.write_text(yaml.safe_dump({"parameterization": {"exponential": {
        "names": pnames, "min": [float(v) for v in g["lo"]], "max": [float(v) for v in g["hi"]]}}}))
    analysis = yaml.safe_load(path.read_text())
    emu_cfg = _EmuCfg({n: _GroupCfg(int(g[n + "_n_pc"])) for n in names}, sorter, analysis, "exponential")
    n_rows, T = 700, 8
    out = emulation.global_sensitivity(emu_cfg, n=n_rows, seed=3, n_batches=T, emulation_group_results=res)
    A, B = sensitivity.base_samples(n_rows, g["lo"], g["hi"], seed=3, method="sobol")
    F = sorter.shape[1]
    assert out["first_order"].shape == (d, F) and out["total"].shape == (d, F) and out["mean"].shape == (F,)
    assert out["parameter_names"] == pnames and out["n"] == n_rows and out["n_batches"] == T
    covered = np.zeros(F, dtype=bool)
    for _, (grp, so, sg) in mapping.items():
        dm = emulation.device_model_for(res[grp], emu_cfg.emulation_groups_config[grp].n_pc)
        own = dm.sobol_indices(A, B, n_batches=T)
        for key in ("first_order", "total", "first_order_se", "total_se"):
            assert np.array_equal(out[key][:, so], own[key][:, sg], equal_nan=True), key
        for key in ("variance", "mean"):
            assert np.array_equal(out[key][so], own[key][sg]), key
        covered[so] = True
    assert covered.all()
    # the merged order is predict's: the mean over the 2 n base rows of predict's central values
    cv = np.concatenate([emulation.predict(X[i:i + 100], emu_cfg, emulation_group_results=res)["central_value"]
                         for X in (A, B) for i in range(0, n_rows, 100)])
    assert np.all(np.abs(out["mean"] - cv.mean(axis=0)) <= 1e-9 * np.abs(cv).max())
    print(f"three shipped groups: F = {F}, largest total index {np.nanmax(out['total']):.3f}, "
          f"largest first-order standard error {np.nanmax(out['first_order_se']):.3e}")
    # a sub-box is a `box` argument; 'random' another method
    sub = emulation.global_sensitivity(emu_cfg, n=64, method="random", n_batches=4, emulation_group_results=res,
                                       box=(g["lo"], 0.5 * (g["lo"] + g["hi"])))
    assert sub["first_order"].shape == (d, F) and np.all(sub["variance"] >= 0)
    emulation.release_device_models()
