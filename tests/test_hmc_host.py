"""Host tests of the HMC sampler's specification (tests/hmc_ref.py): the closed-form reflection, the
leapfrog's reversibility and order, dual averaging, the warm-up schedule, the ABI -- and the conditions that make the
device comparison of tests/test_gpu_hmc.py decisive for every case it runs."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import hmc_ref as R


# ---- reflection -------------------------------------------------------------------------------------------------------
def test_closed_form_fold_equals_bounce_by_bounce_reflection():
    rng = np.random.default_rng(0)
    lo, hi = -0.7, 1.9
    w = hi - lo
    # inside, just outside either face, many widths away on both sides
    xs = np.concatenate([rng.uniform(lo, hi, 50), lo - rng.uniform(0, 3 * w, 100), hi + rng.uniform(0, 3 * w, 100),
                         lo + w * rng.uniform(-40, 40, 200)])
    ps = rng.normal(size=xs.size)
    xf, pf, back = R.fold(xs, ps, lo, hi)
    n_multi = 0
    for x, p, a, b, fl in zip(xs, ps, xf, pf, back):
        xb, pb, n = R.bounce(x, p, lo, hi)
        n_multi += n > 1
        assert abs(a - xb) <= 64 * np.finfo(float).eps * max(abs(x), w), (x, a, xb)
        assert b == pb and fl == (n % 2 == 1), (x, n)
        assert lo <= a <= hi
    assert n_multi > 100, "the test must see several bounces"
    # vector box, as the sampler uses it
    lo3, hi3 = np.array([0.0, -1.0, 2.0]), np.array([1.0, 1.0, 2.5])
    X = rng.uniform(-5, 5, (64, 3))
    P = rng.normal(size=(64, 3))
    Xf, Pf, _ = R.fold(X, P, lo3, hi3)
    for i in range(64):
        for j in range(3):
            xb, pb, _ = R.bounce(X[i, j], P[i, j], lo3[j], hi3[j])
            assert abs(Xf[i, j] - xb) < 1e-13 and Pf[i, j] == pb


def test_a_point_on_a_face_is_outside_the_open_box():
    lo, hi = np.array([0.0]), np.array([1.0])
    x, p, _ = R.fold(np.array([[2.0], [-2.0], [1.0]]), np.ones((3, 1)), lo, hi)
    assert x[0, 0] == 0.0 and x[1, 0] == 0.0 and x[2, 0] == 1.0


# ---- leapfrog ---------------------------------------------------------------------------------------------------------
def _quadratic(d=3, seed=1):
    rng = np.random.default_rng(seed)
    lo, hi = -np.ones(d) * 4.0, np.ones(d) * 4.0
    target = R.quadratic_target(rng.uniform(-0.5, 0.5, d), rng.uniform(0.5, 3.0, d))
    return rng, lo, hi, target, (hi - lo) ** 2 / 12.0


def test_leapfrog_is_reversible_also_through_reflections():
    rng, lo, hi, target, minv = _quadratic()
    W, L = 40, 7
    x0 = rng.uniform(lo, hi, (W, 3))
    x0[:10, 0] = hi[0] - 1e-3                    # these reflect at once
    p0 = rng.normal(size=(W, 3)) / np.sqrt(minv)
    p0[:10, 0] = np.abs(p0[:10, 0])
    eps = np.full(W, 0.2)
    _, g0 = target(x0)
    x1, p1, _, g1, nref = R.leapfrog(target, x0, p0, g0, eps, minv, lo, hi, L)
    assert nref.sum() >= 10
    x2, p2, _, _, _ = R.leapfrog(target, x1, -p1, g1, eps, minv, lo, hi, L)
    assert np.max(np.abs(x2 - x0)) < 1e-12 and np.max(np.abs(-p2 - p0)) < 1e-12


def test_energy_error_scales_as_eps_squared():
    rng, lo, hi, target, minv = _quadratic()
    lo, hi = lo * 100, hi * 100                 # no reflection: the plain integrator
    W = 64
    x0 = rng.uniform(-1, 1, (W, 3))
    p0 = rng.normal(size=(W, 3)) / np.sqrt(minv)
    lp0, g0 = target(x0)
    errs = []
    for eps, L in ((0.02, 16), (0.01, 32), (0.005, 64)):          # the same trajectory length
        x1, p1, lp1, _, _ = R.leapfrog(target, x0, p0, g0, np.full(W, eps), minv, lo, hi, L)
        h0 = -lp0 + 0.5 * np.sum(minv * p0 * p0, axis=1)
        h1 = -lp1 + 0.5 * np.sum(minv * p1 * p1, axis=1)
        errs.append(np.max(np.abs(h1 - h0)))
    assert 3.5 < errs[0] / errs[1] < 4.5 and 3.5 < errs[1] / errs[2] < 4.5, errs


def test_iterate_accept_reject_and_divergence_rules():
    rng, lo, hi, target, minv = _quadratic()
    W = 6
    x = rng.uniform(-1, 1, (W, 3))
    lp, g = target(x)
    p0 = rng.normal(size=(W, 3)) / np.sqrt(minv)
    eps = np.full(W, 0.1)
    base = R.iterate(target, x, lp, g, p0, np.full(W, -np.inf), eps, minv, lo, hi, 4)
    assert base["accept"].all() and not base["divergent"].any()
    none = R.iterate(target, x, lp, g, p0, np.full(W, np.inf), eps, minv, lo, hi, 4)
    assert not none["accept"].any() and np.array_equal(none["x"], x) and np.array_equal(none["g"], g)

    def steep(X):                                # an energy error far beyond 1000
        l, gg = target(X)
        return l - 1e6 * np.sum((X - x[: len(X)]) ** 2, axis=1), gg
    div = R.iterate(steep, x, lp, g, p0, np.full(W, -np.inf), eps, minv, lo, hi, 1)
    assert div["divergent"].all() and not div["accept"].any() and np.all(div["accept_prob"] == 0.0)

    def nan_lp(X):
        l, gg = target(X)
        return l * np.nan, gg
    bad = R.iterate(nan_lp, x, lp, g, p0, np.full(W, -np.inf), eps, minv, lo, hi, 1)
    assert bad["divergent"].all() and not bad["accept"].any()

    def on_face(X):                              # lp = -inf: the ordinary reject, not a divergence
        l, gg = target(X)
        return np.full_like(l, -np.inf), gg * 0.0
    face = R.iterate(on_face, x, lp, g, p0, np.full(W, -np.inf), eps, minv, lo, hi, 1)
    assert not face["divergent"].any() and not face["accept"].any() and np.all(face["accept_prob"] == 0.0)


# ---- adaptation -------------------------------------------------------------------------------------------------------
def test_dual_averaging_equals_the_hand_written_recurrence_and_the_package_copy():
    from gpemu import hmc
    alphas = [0.31, 0.95, 0.99, 0.4, 0.77, 0.85, 0.6, 0.92, 0.81, 0.79, 0.8, 0.83]
    eps0, target = 0.25, 0.8
    got, eps_bar = R.dual_averaging(eps0, alphas, target)
    # algorithm 5 of Hoffman & Gelman 2014, written out
    mu, hbar, leb = np.log(10 * eps0), 0.0, 0.0
    state = hmc.dual_averaging_start(eps0)
    for m, a in enumerate(alphas, start=1):
        hbar = (1 - 1 / (m + 10.0)) * hbar + (1 / (m + 10.0)) * (target - a)
        le = mu - (np.sqrt(m) / 0.05) * hbar
        leb = m ** -0.75 * le + (1 - m ** -0.75) * leb
        assert abs(got[m - 1] - np.exp(le)) <= 1e-15 * np.exp(le)
        state = hmc.dual_averaging_update(state, a, target)
        assert abs(state[0] - np.exp(le)) <= 1e-15 * np.exp(le)
    assert abs(eps_bar - np.exp(leb)) <= 1e-15 * eps_bar and abs(np.exp(state[1]) - eps_bar) <= 1e-15 * eps_bar
    assert (hmc.GAMMA, hmc.T0, hmc.KAPPA, hmc.MU_FACTOR) == (R.GAMMA, R.T0, R.KAPPA, 10.0)
    assert hmc.DIVERGENCE_THRESHOLD == R.DIVERGENT
    # low acceptance shrinks the step, high acceptance grows it
    assert R.dual_averaging(0.1, [0.1] * 20, 0.8)[1] < 0.1 < R.dual_averaging(0.1, [1.0] * 20, 0.8)[1]


def test_warmup_schedule():
    from gpemu import hmc
    for n in (1, 19, 20, 100, 150, 1000, 1234):
        blocks = hmc.warmup_schedule(n)
        assert sum(b for b, _ in blocks) == n and all(b > 0 for b, _ in blocks)
        if n >= 20:
            assert not blocks[0][1] and not blocks[-1][1] and any(m for _, m in blocks)
            assert blocks[0][0] == round(0.15 * n) and blocks[-1][0] == round(0.10 * n)
            wins = [b for b, m in blocks if m]
            assert all(b2 >= 2 * b1 for b1, b2 in zip(wins, wins[1:])), wins
    assert hmc.warmup_schedule(0) == []
    assert hmc.warmup_schedule(1000) == [(150, False), (25, True), (50, True), (100, True), (575, True), (100, False)]
    v = hmc.regularised_metric(np.array([2.0]), 95, np.array([10.0]))
    assert abs(v[0] - (2.0 * 0.95 + 1e-3 * 10.0 * 0.05)) < 1e-15


# ---- random stream ----------------------------------------------------------------------------------------------------
def test_philox_restated_in_numpy_equals_the_library_copy():
    from gpemu import _lib
    L = _lib.lib()
    out = (C.c_uint32 * 4)()
    rng = np.random.default_rng(3)
    for _ in range(20):
        c = [int(v) for v in rng.integers(0, 2 ** 32, 4)]
        k = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        assert L.gpemu_philox4x32(*c, *k, out) == 0
        mine = R.philox4x32_10(*c, *k)
        assert [int(v) for v in mine] == list(out)


def test_normal_draws_have_unit_moments_and_distinct_streams():
    z, ua, uj = R.draws(4096, 7, seed=5, step=3)
    assert z.shape == (4096, 7) and abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.03
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.05 and abs(np.corrcoef(z[:, 5], z[:, 6])[0, 1]) < 0.05
    assert np.all((ua >= 0) & (ua < 1)) and np.all((uj >= 0) & (uj < 1)) and abs(np.corrcoef(ua, uj)[0, 1]) < 0.05
    z2, _, _ = R.draws(4096, 7, seed=5, step=4)
    assert not np.array_equal(z, z2)
    z3, _, _ = R.draws(100, 7, seed=5, step=3)
    assert np.array_equal(z3, z[:100]), "a chain's draws depend on its index only, not on the number of chains"


# ---- ABI --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["gpemu_sampler_create_hmc", "gpemu_sampler_hmc_set_metric", "gpemu_sampler_hmc_get_metric",
               "gpemu_sampler_hmc_set_step_size", "gpemu_sampler_hmc_get_step_size", "gpemu_sampler_hmc_adapt",
               "gpemu_sampler_hmc_step_host_rng", "gpemu_sampler_hmc_stats", "gpemu_sampler_hmc_draws",
               "gpemu_sampler_chain_moments", "gpemu_hmc_path_counts"]
HMC_PATHS = ["BEGIN", "BEGIN_HOST_RNG", "LEAPFROG", "FINISH", "ADAPT", "ACCEPT_MEAN", "MOMENTS"]


def test_new_entry_points_are_declared_bound_and_exported():
    from gpemu import _lib, model, sampler
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared and n in _lib.exported_symbols() and hasattr(L, n), n
    for n in HMC_PATHS:
        assert "GPEMU_HMC_PATH_" + n in hdr
    out = np.zeros(8, dtype=np.int64)
    assert L.gpemu_hmc_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), 8) == len(HMC_PATHS)
    assert len(model.hmc_path_counts()) == len(HMC_PATHS)
    for n in ("warmup", "run", "step_size", "inverse_metric", "divergences", "acceptance_fraction", "chain_moments"):
        assert hasattr(sampler.HMCSampler, n), n
    assert callable(sampler.DeviceSampler.chain_moments)


# ---- what keeps the device comparison honest --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TRAJECTORY_CASES))
def test_reference_runs_decide_every_case(name):
    """for each case (and both numbers of chains the device test runs): accepts, rejects and reflections occur; every
    accept decision and every divergence decision is MIN_MARGIN away from its threshold, and none of the runs with the
    gradients moved by their bound decides differently -- so the device may not either, and no case is left out"""
    run = R.reference_run(name)
    d = R.trajectory_problem(name)["lo"].size
    assert run["chain"].shape == (R.N_ITER, R.W_MAX, d)
    for W in (24, R.W_MAX):
        acc = run["accept"][:, :W]
        assert acc.any() and (~acc).any(), (name, W, int(acc.sum()))
    assert run["reflections"] >= 1
    with np.errstate(invalid="ignore"):
        assert not np.any(run["margin"] < R.MIN_MARGIN), float(np.nanmin(run["margin"]))
        assert not np.any(run["div_margin"] < R.MIN_MARGIN)
    assert run["flips"] == 0
    assert np.all(run["deviation"] < 1e-3), "the perturbed runs stay beside the unperturbed one"
    lo, hi = R.trajectory_problem(name)["lo"], R.trajectory_problem(name)["hi"]
    assert np.all((run["chain"] > lo) & (run["chain"] < hi))
    X0 = R.trajectory_start(name)
    near = np.min(np.minimum(X0 - lo, hi - X0) / (hi - lo), axis=1) < 0.02
    assert near.sum() >= 8, "starts within one step of a face"
    print(f"\nHMC REF {name}: accepts {int(run['accept'].sum())} / {run['accept'].size}, divergences "
          f"{int(run['divergent'].sum())}, reflections {run['reflections']}, min margin {float(np.nanmin(run['margin'])):.3g}, "
          f"deviation per iteration {run['deviation'].max(axis=1)}")


@pytest.mark.parametrize("name", R.RECORDED)
def test_recorded_reference_run_is_what_hmc_ref_computes(name):
    """the fixture's first two iterations of chains 0 .. 2 recomputed, with one perturbed run beside them (the first of
    the fixture's sign patterns: its deviation cannot exceed the recorded maximum over all of them)"""
    rec = R.reference_run(name)
    part = R.compute_reference_run(name, chains=3, n_iter=2, n_patterns=1)
    lo, hi = R.trajectory_problem(name)["lo"], R.trajectory_problem(name)["hi"]
    assert np.array_equal(part["accept"], rec["accept"][:2, :3]) and np.array_equal(part["divergent"], rec["divergent"][:2, :3])
    assert np.max(np.abs(part["chain"] - rec["chain"][:2, :3]) / (hi - lo)) < 1e-13
    assert np.allclose(part["lp"], rec["lp"][:2, :3], rtol=1e-12, atol=0)
    assert np.all(part["deviation"] <= rec["deviation"][:2, :3] * (1 + 1e-6) + 1e-18)
