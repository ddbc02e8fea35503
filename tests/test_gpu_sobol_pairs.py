"""-m gpu tests of the second-order Sobol' indices on the device (gpemu_sobol_moments_pairs,
DeviceModel.sobol_moments_pairs / sobol_indices(second_order=True), emulation.global_sensitivity(second_order=True);
DESIGN.md §4.45) against tests/sobol_pairs_ref.py: the extended-precision means of the explicitly built pair rows with
the distance factor of the kernel's walk (``sobol_pairs_ref.c_x_pp``), their moments and indices in longdouble, and
the tolerances that follow from the per-row bounds.  Every reference is computed once per case
(``sobol_pairs_ref.case_means``); smaller n are prefixes of its rows.

The C entry returns moments, not means.  With one row per batch (n_batches = n) a batch's ``sumD2`` is the single
difference fl(z(AB_ij) - z(A)) and ``mean_pick_freeze`` returns the device's z(A) itself, so the pair mean is
z(A) + sumD2 up to the one rounding u |D_ij| of that subtraction, which the means' test adds to the row's bound.

Figures measured on an MI355X are printed by every test before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import sobol_pairs_ref as PR
import sobol_ref as R

pytestmark = pytest.mark.gpu

CASE_NAMES = sorted(PR.CASES)
SIZES = (1, 63, 64, 65, 257)                  # the wave's row tile and the slice edge
FIRST = ("pivot", "count", "sumA", "sumB", "C2", "sumD", "M", "D")
SECOND = ("sumD2", "M2", "D2")
PAIR_INDEX_KEYS = ("closed_pair", "interaction", "total_pair", "closed_pair_se", "interaction_se", "total_pair_se")
U = R.U


@functools.lru_cache(maxsize=None)
def _dm(name):
    import golden_util as GU
    return GU.device_model(PR.case(name)[0])


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _same(a, b, keys):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pair_means_against_the_extended_precision_reference(name):
    model, lo, hi, A, B, pairs = PR.case(name)
    dm, (Zr, eps) = _dm(name), PR.case_means(name)
    d, k, P = A.shape[1], model.n_pc, len(pairs)
    worst = 0.0
    for n in SIZES:
        out = dm.sobol_moments_pairs(A[:n], B[:n], pairs, n_batches=n)
        assert out["sumD2"].shape == (n, P, k) and out["M2"].shape == (n, P, k, k) and out["D2"].shape == (n, P, k, k)
        assert np.array_equal(out["pairs"], pairs) and np.array_equal(out["count"], np.ones(n, dtype=np.int64))
        _same(out, dm.sobol_moments(A[:n], B[:n], n_batches=n), FIRST)          # the first order's bytes
        zA = dm.mean_pick_freeze(A[:n], B[:n])[0]                               # the device's z(A)
        Zp = zA[None] + out["sumD2"].transpose(1, 0, 2)                         # (P, n, k); exact in longdouble below
        err = np.abs(_f64((np.asarray(zA, dtype=PR.LD)[None] + out["sumD2"].transpose(1, 0, 2)) - Zr[2 + d:, :n]))
        bound = eps[2 + d:, :n] + U * np.abs(out["sumD2"].transpose(1, 0, 2))
        ratio = err / bound
        worst = max(worst, float(ratio.max()))
        planted = ratio[0, PR.PLANT_ROW].max() if n > PR.PLANT_ROW else float("nan")
        print(f"{name} n={n}: max |z(AB_ij) - ref| / eps = {ratio.max():.3e} (the row planted on a training point: "
              f"{planted:.3e})")
        assert Zp.shape == (P, n, k) and np.all(ratio <= 1.0), (name, n)
    print(f"{name}: worst pair-mean ratio over all n {worst:.3e}")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pair_moments_against_the_longdouble_moments_about_the_returned_pivot(name):
    model, lo, hi, A, B, pairs = PR.case(name)
    dm, (Zr, eps) = _dm(name), PR.case_means(name)
    n, d = PR.moment_rows(name), A.shape[1]
    for T in (1, 4, 16):
        out = dm.sobol_moments_pairs(A[:n], B[:n], pairs, n_batches=T)
        assert np.array_equal(out["count"], np.bincount(R.batch_of(n, T), minlength=T))
        _same(out, dm.sobol_moments(A[:n], B[:n], n_batches=T), FIRST)
        ref = PR.moments(Zr[:, :n], d, out["pivot"], T)
        tol = PR.moment_tolerances(Zr[:, :n], eps[:, :n], d, out["pivot"], T)
        for key in FIRST[2:] + SECOND:
            err = np.abs(_f64(out[key] - ref[key]))
            print(f"{name} n={n} T={T} {key}: max err {err.max():.3e}, max err / tol {np.max(err / tol[key]):.3e}")
            assert np.all(err <= tol[key]), (name, T, key)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pair_indices_against_the_reference_estimators(name):
    model, lo, hi, A, B, pairs = PR.case(name)
    dm, (Zr, eps) = _dm(name), PR.case_means(name)
    n, F, P = PR.moment_rows(name), model.components.shape[1], len(pairs)
    for T in (1, 16):
        out = dm.sobol_indices(A[:n], B[:n], n_batches=T, second_order=True, pairs=pairs)
        first = dm.sobol_indices(A[:n], B[:n], n_batches=T)
        for key in first:                                                       # the first-order keys keep their bytes
            assert np.array_equal(out[key], first[key], equal_nan=True), key
        assert set(out) == set(first) | set(PAIR_INDEX_KEYS) | {"pairs"} and np.array_equal(out["pairs"], pairs)
        pivot = dm.sobol_moments(A[:n], B[:n], n_batches=T)["pivot"]
        ref, tol = PR.indices(Zr[:, :n], eps[:, :n], model, pairs, pivot, T)
        print(f"{name} n={n} T={T}: max tol(V) / V = {tol['cond']:.3e}")
        assert tol["cond"] <= 1e-9
        for key in PAIR_INDEX_KEYS[:3] + (PAIR_INDEX_KEYS[3:] if T > 1 else ()):
            assert out[key].shape == (P, F)
            err = np.abs(_f64(out[key] - ref[key]))
            print(f"{name} n={n} T={T} {key}: max err {err.max():.3e}, max tol {tol[key].max():.3e}, "
                  f"max err / tol {np.max(err / tol[key]):.3e}")
            assert np.all(err <= tol[key]), (name, T, key)
        if T == 1:
            assert all(np.all(np.isnan(out[key])) for key in PAIR_INDEX_KEYS[3:])


def test_b_equal_a_gives_exact_zeros_and_a_shared_column_the_first_order_row():
    for name in ("rbf_d6", "matern05_d6", "matern_nu12_d5", "rbf_d16"):
        model, lo, hi, A, B, pairs = PR.case(name)
        dm = _dm(name)
        n = 65
        m = dm.sobol_moments_pairs(A[:n], A[:n], pairs, n_batches=4)
        for key in SECOND + ("sumD", "M", "D"):
            assert not m[key].any(), (name, key)
        out = dm.sobol_indices(A[:n], A[:n], n_batches=4, second_order=True, pairs=pairs)
        assert not out["closed_pair"].any() and not out["total_pair"].any() and not out["interaction"].any()
        # B shares column c with A: AB_cj IS AB_j and AB_ic IS AB_i, so their moments are the first-order ones' bits
        for c in sorted({int(pairs[0, 0]), int(pairs[-1, 1])}):
            Bs = np.array(B[:n])
            Bs[:, c] = A[:n, c]
            m = dm.sobol_moments_pairs(A[:n], Bs, pairs, n_batches=4)
            hit = 0
            for q, (i, j) in enumerate(pairs):
                if c in (i, j):
                    o = j if c == i else i
                    for k2, k1 in (("sumD2", "sumD"), ("M2", "M"), ("D2", "D")):
                        assert m[k2][:, q].tobytes() == m[k1][:, o].tobytes(), (name, c, (i, j), k2)
                    hit += 1
            assert hit >= 1 and not m["D"][:, c].any()
        print(f"{name}: B = A: sumD2, M2, D2 identically 0; a shared column gives M and D of the other index, bit for bit")


def test_permuting_the_parameters_permutes_the_pairs():
    import golden_util as GU
    from oracle import gp_oracle as O
    name = "matern15_d6"
    model, lo, hi, A, B, pairs = PR.case(name)
    dm, (Zr, eps) = _dm(name), PR.case_means(name)
    n = PR.moment_rows(name)
    perm = np.array([3, 0, 5, 1, 4, 2])                     # new parameter a is old parameter perm[a]
    gps = [O.GP(ls=gp.ls[perm], const=gp.const, noise=gp.noise, alpha=gp.alpha, L=gp.L) for gp in model.gps]
    pm = O.GroupModel(X_train=np.ascontiguousarray(model.X_train[:, perm]), spec=model.spec, gps=gps,
                      components=model.components, explained_variance=model.explained_variance,
                      scaler_mean=model.scaler_mean, scaler_scale=model.scaler_scale, n_pc=model.n_pc)
    dp = GU.device_model(pm)
    a = dm.sobol_indices(A[:n], B[:n], n_batches=4, second_order=True)
    b = dp.sobol_indices(np.ascontiguousarray(A[:n][:, perm]), np.ascontiguousarray(B[:n][:, perm]), n_batches=4,
                         second_order=True)
    pivot = dm.sobol_moments(A[:n], B[:n], n_batches=4)["pivot"]
    _, tol = PR.indices(Zr[:, :n], eps[:, :n], model, pairs, pivot, 4)
    where = {(int(i), int(j)): q for q, (i, j) in enumerate(a["pairs"])}
    old = np.array([where[tuple(sorted((int(perm[i]), int(perm[j]))))] for i, j in b["pairs"]])
    assert sorted(old.tolist()) == list(range(len(pairs)))
    for key in ("closed_pair", "interaction", "total_pair"):
        err = np.abs(b[key] - a[key][old])
        print(f"permuted {key}: max err {err.max():.3e}, max err / (2 tol) {np.max(err / (2 * tol[key][old])):.3e}")
        assert np.all(err <= 2 * tol[key][old])             # each side within tol of its own exact value
    dp.close()


def test_results_do_not_depend_on_the_workspace_the_run_or_the_other_pairs():
    from gpemu.sensitivity import (SOBOL_PAIRS_PATHS, sobol_pairs_path_counts, sobol_pairs_workspace_bytes,
                                   sobol_path_counts)
    name = "rbf_d6"
    model, lo, hi, _, _, pairs = PR.case(name)
    dm = _dm(name)
    n, T, d, k, P = 4096 + 33, 16, 6, model.n_pc, len(pairs)
    rng = np.random.default_rng(5)
    A, B = rng.uniform(lo, hi, (n, d)), rng.uniform(lo, hi, (n, d))
    ikeys = PAIR_INDEX_KEYS + ("first_order", "total", "first_order_se", "total_se", "variance", "mean")
    whole = dm.sobol_moments_pairs(A, B, n_batches=T)
    assert np.array_equal(whole["pairs"], pairs)            # None: all i < j in the order of marginals.pair_indices
    _same(whole, dm.sobol_moments_pairs(A, B, n_batches=T), FIRST + SECOND)
    iwhole = dm.sobol_indices(A, B, n_batches=T, second_order=True)
    _same(iwhole, dm.sobol_indices(A, B, n_batches=T, second_order=True), ikeys)
    ix = {x: SOBOL_PAIRS_PATHS.index(x) for x in SOBOL_PAIRS_PATHS}
    # batches of 258 / 259 rows are two slices of ~129 rows: chunks are whole slices, their edges fall inside batches
    for rows, chunks in ((n, 1), (2100, 2), (1000, 5)):
        ws = sobol_pairs_workspace_bytes(rows, d, k, P)
        c0, f0 = sobol_pairs_path_counts(), sobol_path_counts()
        out = dm.sobol_moments_pairs(A, B, n_batches=T, workspace_bytes=ws)
        c1 = sobol_pairs_path_counts() - c0
        print(f"workspace for {rows} rows: counters {dict(zip(SOBOL_PAIRS_PATHS, c1.tolist()))}")
        assert c1[ix["call"]] == 1 and c1[ix["chunk"]] == chunks and c1[ix["whole"]] == (chunks == 1)
        assert c1[ix["dp8"]] == chunks and c1[ix["kind0"]] == chunks        # one launch of the pair kernel per chunk
        assert c1.sum() == 1 + 3 * chunks + (chunks == 1)
        assert np.array_equal(sobol_path_counts(), f0)                      # the first order's counters do not move
        _same(whole, out, FIRST + SECOND)
        _same(iwhole, dm.sobol_indices(A, B, n_batches=T, workspace_bytes=ws, second_order=True), ikeys)
    # a subset of the pairs, in another order: the same bytes for those pairs as in the all-pairs call
    sub = np.array([(4, 5), (0, 3), (1, 2), (0, 5)])
    where = [int(np.flatnonzero((pairs == p).all(axis=1))[0]) for p in sub]
    out = dm.sobol_moments_pairs(A, B, sub, n_batches=T)
    _same(whole, out, FIRST)
    for key in SECOND:
        assert out[key].tobytes() == np.ascontiguousarray(whole[key][:, where]).tobytes(), key
    isub = dm.sobol_indices(A, B, n_batches=T, second_order=True, pairs=sub)
    for key in PAIR_INDEX_KEYS:
        assert isub[key].tobytes() == np.ascontiguousarray(iwhole[key][where]).tobytes(), key
    c0 = sobol_pairs_path_counts()
    _same(whole, dm.sobol_moments(A, B, n_batches=T), FIRST)               # gpemu_sobol_moments' bytes ...
    assert np.array_equal(sobol_pairs_path_counts(), c0)                   # ... and it does not move the new counters


def test_the_wide_and_general_instances_count_their_own_paths():
    from gpemu.sensitivity import SOBOL_PAIRS_PATHS, sobol_pairs_path_counts
    for name, dp, kind in (("matern25_d9", "dp16", "kind3"), ("matern_nu12_d5", "dp8", "kind4"), ("matern05_d6", "dp8", "kind1"),
                           ("matern15_d6", "dp8", "kind2"), ("rbf_d16", "dp16", "kind0")):
        model, lo, hi, A, B, pairs = PR.case(name)
        c0 = sobol_pairs_path_counts()
        _dm(name).sobol_moments_pairs(A[:65], B[:65], pairs, n_batches=2)
        c1 = dict(zip(SOBOL_PAIRS_PATHS, (sobol_pairs_path_counts() - c0).tolist()))
        assert c1 == dict({x: 0 for x in SOBOL_PAIRS_PATHS}, call=1, chunk=1, whole=1, **{dp: 1, kind: 1}), (name, c1)


def test_a_call_between_two_predicts_changes_neither():
    name = "rbf_const_d8"
    model, lo, hi, A, B, pairs = PR.case(name)
    dm = _dm(name)
    X = np.ascontiguousarray(A[:97])
    m0, v0 = dm.gp_predict(X)
    a = dm.sobol_moments_pairs(A[:129], B[:129], pairs, n_batches=4)
    m1, v1 = dm.gp_predict(X)
    b = dm.sobol_moments_pairs(A[:129], B[:129], pairs, n_batches=4)
    assert m0.tobytes() == m1.tobytes() and v0.tobytes() == v1.tobytes()
    _same(a, b, FIRST + SECOND)


def test_refusals_launch_nothing_leave_the_ledger_balanced_and_the_model_usable():
    import devmem_cases as DC
    from gpemu import _lib
    from gpemu._lib import ptr
    from gpemu.sensitivity import sobol_pairs_path_counts, sobol_path_counts
    name = "rbf_d6"
    model, lo, hi, A, B, pairs = PR.case(name)
    dm = _dm(name)
    L = _lib.lib()
    d, k, n = 6, model.n_pc, 8
    A8, B8 = np.ascontiguousarray(A[:n]), np.ascontiguousarray(B[:n])
    base = DC.reading()
    good = dm.sobol_moments_pairs(A8, B8, pairs, n_batches=2)
    DC.assert_back_to(base, "a call")

    def call(n_=n, A_=A8, B_=B8, T=2, prs=((0, 1), (2, 5)), np_=None, handle=None):
        p32 = np.ascontiguousarray(np.array(prs, dtype=np.int32).reshape(-1, 2))
        P, T1 = max(len(p32), 1), max(T, 1)
        o = [np.zeros(k), np.zeros(T1, dtype=np.int64), np.zeros((T1, k)), np.zeros((T1, k)), np.zeros((T1, k, k)),
             np.zeros((T1, d, k)), np.zeros((T1, d, k, k)), np.zeros((T1, d, k, k)), np.zeros((T1, P, k)),
             np.zeros((T1, P, k, k)), np.zeros((T1, P, k, k))]
        return L.gpemu_sobol_moments_pairs(handle or dm.handle, n_, ptr(A_), ptr(B_), T, len(p32) if np_ is None else np_,
                                           ptr(p32), 0, *[ptr(x) for x in o])

    assert call() == 0
    bad = A8.copy()
    bad[3, 2] = np.nan
    inf = B8.copy()
    inf[0, 0] = np.inf
    one = R.case("rbf_d1")
    import golden_util as GU
    d1 = GU.device_model(one[0])
    A1d, B1d = np.ascontiguousarray(one[3][:n]), np.ascontiguousarray(one[4][:n])
    calls = {
        "n = 0": lambda: call(n_=0),
        "n_batches = 0": lambda: call(T=0),
        "n_batches > n": lambda: call(T=n + 1),
        "n_pairs = 0": lambda: call(np_=0),
        "index = d": lambda: call(prs=((0, 6),)),
        "negative index": lambda: call(prs=((-1, 2),)),
        "i == j": lambda: call(prs=((2, 2),)),
        "i > j": lambda: call(prs=((3, 1),)),
        "a repeated pair": lambda: call(prs=((0, 1), (2, 5), (0, 1))),
        "NaN row": lambda: call(A_=bad),
        "inf row": lambda: call(B_=inf),
        "d == 1": lambda: call(A_=A1d, B_=B1d, prs=((0, 1),), handle=d1.handle),
    }
    base = DC.reading()
    c0, f0 = sobol_pairs_path_counts(), sobol_path_counts()
    for label, fn in calls.items():
        rc = fn()
        msg = _lib.last_error()
        print(f"{label}: rc {rc}, '{msg}'")
        assert rc == DC.ERR_ARG and msg, label
        now = DC.assert_back_to(base, label)
        assert now["allocs"] == base["allocs"], label                       # not even an allocation
    assert np.array_equal(sobol_pairs_path_counts(), c0) and np.array_equal(sobol_path_counts(), f0)   # no launch
    for kw in (dict(pairs=[(1, 1)]), dict(pairs=[(0, 6)]), dict(pairs=[(0, 1), (0, 1)]), dict(n_batches=n + 1)):
        with pytest.raises(ValueError):
            dm.sobol_moments_pairs(A8, B8, **kw)
    with pytest.raises(ValueError):
        d1.sobol_moments_pairs(A1d, B1d)
    with pytest.raises(ValueError):
        dm.sobol_indices(A8, B8, pairs=[(0, 1)])                            # pairs without second_order
    d1.close()
    _same(good, dm.sobol_moments_pairs(A8, B8, pairs, n_batches=2), FIRST + SECOND)       # the model is usable, same bits


def test_global_sensitivity_second_order_equals_the_groups_results_scattered_by_the_sorter(tmp_path):
    """emulation.global_sensitivity(second_order=True) on the shipped three-group fixture (golden G7): the per-group
    results on the shared base matrices, scattered into the observable order of ``predict``, byte for byte; without
    the keyword the result is today's"""
    import yaml

    import dropin_util as DU
    import golden_util as GU
    from bayesian_inference import emulation
    from gpemu import sensitivity
    from test_gpu_sobol import _EmuCfg, _GroupCfg
    g = GU.load("g7_shipped_config")
    names, mapping, block_start, cols = GU.g7_groups(g)
    sorter = emulation.SortEmulationGroupObservables(mapping, tuple(int(v) for v in g["map_shape"]))
    res = {}
    for n in names:
        sub = {k[len(n) + 1:]: v for k, v in g.items() if k.startswith(n + "_")}
        sub.update(design=g["design"], gpr_alpha=g["gpr_alpha"])
        res[n] = DU.results_at_golden_theta(sub)
    d = g["lo"].size
    path = tmp_path / "analysis.yaml"
    path.write_text(yaml.safe_dump({"parameterization": {"exponential": {
        "names": [f"par_{i}" for i in range(d)], "min": [float(v) for v in g["lo"]], "max": [float(v) for v in g["hi"]]}}}))
    emu_cfg = _EmuCfg({n: _GroupCfg(int(g[n + "_n_pc"])) for n in names}, sorter, yaml.safe_load(path.read_text()),
                      "exponential")
    n_rows, T = 300, 8
    pairs = [(0, d - 1), (1, 2), (0, 1)]
    plain = emulation.global_sensitivity(emu_cfg, n=n_rows, seed=3, n_batches=T, emulation_group_results=res)
    out = emulation.global_sensitivity(emu_cfg, n=n_rows, seed=3, n_batches=T, emulation_group_results=res,
                                       second_order=True, pairs=pairs)
    assert set(out) == set(plain) | set(PAIR_INDEX_KEYS) | {"pairs"} and out["pairs"].tolist() == [list(p) for p in pairs]
    for key in plain:
        assert np.array_equal(out[key], plain[key], equal_nan=True) if isinstance(plain[key], np.ndarray) \
            else out[key] == plain[key], key
    A, B = sensitivity.base_samples(n_rows, g["lo"], g["hi"], seed=3, method="sobol")
    F = sorter.shape[1]
    covered = np.zeros(F, dtype=bool)
    for _, (grp, so, sg) in mapping.items():
        dm = emulation.device_model_for(res[grp], emu_cfg.emulation_groups_config[grp].n_pc)
        own = dm.sobol_indices(A, B, n_batches=T, second_order=True, pairs=pairs)
        for key in PAIR_INDEX_KEYS:
            assert out[key].shape == (len(pairs), F)
            assert np.array_equal(out[key][:, so], own[key][:, sg], equal_nan=True), key
        covered[so] = True
    assert covered.all()
    allp = emulation.global_sensitivity(emu_cfg, n=64, n_batches=4, emulation_group_results=res, second_order=True)
    assert allp["closed_pair"].shape == (d * (d - 1) // 2, F)
    print(f"three shipped groups: F = {F}, largest interaction {np.nanmax(out['interaction']):.3f}, "
          f"largest interaction standard error {np.nanmax(out['interaction_se']):.3e}")
    emulation.release_device_models()
