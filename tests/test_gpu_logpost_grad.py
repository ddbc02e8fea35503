"""-m gpu tests of the derivative path: gpemu_gp_predict_grad, gpemu_logpost_grad,
gpemu_logpost_groups_grad against tests/grad_ref.py's extended-precision reference and a-priori bounds; determinism,
refusals, the box; the drop-in functions and the MAP certificate on the shipped three-group golden G7."""
from __future__ import annotations

import math
import types

import numpy as np
import pytest
import scipy.optimize

import dropin_util as DU
import golden_util as GU
import grad_ref as G
import hp_ref as H
import path_cases as PC
from gpemu import _lib
from gpemu import model as M
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble
GRAD_PATHS = ["CHUNK", "LOGLIK", "CONTRACT_8", "CONTRACT_16", "JACOBIAN_8", "JACOBIAN_16"]
GP = {n: i for i, n in enumerate(GRAD_PATHS)}
GRAD_CHUNK = 1024
CASES, SKIPPED = G.sweep_cases()


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def counts():
    c = M.grad_path_counts()
    assert len(c) == len(GRAD_PATHS), "enum gpemu_grad_path and GRAD_PATHS disagree"
    return c


def within(what, dev, ref, bound):
    """asserts |dev - ref| <= bound in every element; returns the largest err / bound"""
    dev = np.asarray(dev, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), dev.shape)
    err = np.abs(dev.astype(LD) - ref).astype(np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (f"{what}: max err/bound {ratio.max():.3g} at {worst}: dev {dev[worst]!r} "
                                f"ref {float(np.asarray(ref)[worst])!r} bound {bound[worst]:.3g}")
    return float(ratio.max())


def check_against_reference(name, dm, model, Xq, cols, lo, hi, y_exp, y_err, bs, input_rounding=False):
    """logpost_grad on all of Xq and gp_predict_grad on the reference rows, against hp_ref (lp) and grad_ref (the
    rest).  Where the reference cannot tell whether the device clipped a variance (|var_raw| <= var_bound) the device's
    own branch, read from its dvar, selects the reference's: a result within bound of either branch passes."""
    X = Xq[cols]
    B, d = Xq.shape
    wide = d > 8
    c0 = counts()
    lp_d, g_d = dm.logpost_grad(Xq)
    dc = counts() - c0
    chunks = math.ceil(B / GRAD_CHUNK)
    assert dc[GP["CHUNK"]] == chunks and dc[GP["LOGLIK"]] == chunks, dc
    assert dc[GP["CONTRACT_16" if wide else "CONTRACT_8"]] == chunks and dc[GP["CONTRACT_8" if wide else "CONTRACT_16"]] == 0
    assert dc[GP["JACOBIAN_8"]] == 0 and dc[GP["JACOBIAN_16"]] == 0
    fin = np.all(np.isfinite(X), axis=1)
    c0 = counts()
    m_d, v_d, dm_d, dv_d = dm.gp_predict_grad(X[fin])
    dc = counts() - c0
    assert dc[GP["JACOBIAN_16" if wide else "JACOBIAN_8"]] == math.ceil(fin.sum() / GRAD_CHUNK) and dc[GP["LOGLIK"]] == 0
    Xf = X[fin]
    dev_clipped = (v_d == 0.0) & np.all(dv_d == 0.0, axis=2)       # a clipped variance is exactly 0, and so is its derivative
    ref = G.reference(Xf, model, y_exp, y_err, bs, clip_choice=dev_clipped)
    amb = ref["ambiguous"]
    assert np.array_equal(dev_clipped[~amb], ref["clipped"][~amb]), "the device's branch where the reference's is beyond doubt"
    ratios = {"mean": within("mean", m_d, ref["mean"], ref["mean_bound"]),
              "var": within("var", v_d, ref["var"], ref["var_bound"]),
              "dmean": within("dmean", dm_d, ref["dmean"], ref["dmean_bound"]),
              "dvar": within("dvar", dv_d, ref["dvar"], ref["dvar_bound"])}
    assert np.all(v_d[dev_clipped & ref["clipped"]] == 0.0)
    # lp: hp_ref's reference and bound, as gpemu_logpost is held to
    lp, lb, _ = H.log_posterior(Xf, model, lo, hi, y_exp, y_err, bs, input_rounding=input_rounding)
    inside = np.isfinite(np.asarray(lp, dtype=np.float64))
    lpc, gc = lp_d[cols][fin], g_d[cols][fin]
    assert np.array_equal(np.isfinite(lpc), inside) and np.all(lpc[~inside] == -np.inf), "-inf rows"
    assert np.all(gc[~inside] == 0.0), "rows outside the box must have a zero gradient"
    assert np.all(lp_d[cols][~fin] == -np.inf) and np.all(g_d[cols][~fin] == 0.0)
    if inside.any():
        ratios["lp"] = within("lp", lpc[inside], lp[inside], lb[inside])
        ratios["grad"] = within("grad", gc[inside], ref["grad"][inside], ref["grad_bound"][inside])
    print(f"\nGRAD RATIOS {name} " + " ".join(f"{n}={r:.3g}" for n, r in ratios.items())
          + f" ambiguous={int(amb.sum())} clipped={int(dev_clipped.sum())}")
    return ref, ratios, lp_d, g_d


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_sweep_against_extended_reference(idx):
    c = G.sweep_cases(num_cu())[0][idx]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Xq, rep, cols = PC.queries(c, model, lo, hi, rng)
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    _, _, lp_d, g_d = check_against_reference(c.name, dm, model, Xq, cols, lo, hi, y_exp, y_err, bs, c.ls_bounds)
    # the same query at the edge columns of every tile, in every chunk: the same bits
    assert np.all(lp_d[rep] == lp_d[rep[0]]) and np.all(g_d[rep] == g_d[rep[0]]), "repeated query differs across columns"
    dm.close()


def test_general_nu_cases_are_skipped_and_counted():
    assert len(SKIPPED) == 3 and len(CASES) + len(SKIPPED) == len(PC.cases())


def test_clip_case_either_branch():
    model, lo, hi, y_exp, y_err, bs, Xq = G.clip_case()
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    ref, _, _, _ = check_against_reference("clip case", dm, model, Xq, np.arange(len(Xq)), lo, hi, y_exp, y_err, bs)
    sure = ~ref["ambiguous"]
    assert (sure & ref["clipped"]).any() and (sure & ~ref["clipped"]).any()
    dm.close()


def _mid_model():
    c = [x for x in CASES if x.name == "n300_tasks_multi"][0]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    return c, model, dm, lo, hi, rng


def test_determinism_alone_in_a_batch_and_across_a_chunk_boundary():
    c, model, dm, lo, hi, rng = _mid_model()
    x = rng.uniform(lo, hi, c.d)
    alone = dm.logpost_grad(x[None])
    again = dm.logpost_grad(x[None])
    assert np.array_equal(alone[0], again[0]) and np.array_equal(alone[1], again[1])
    ja = dm.gp_predict_grad(x[None])
    for at in (7, 299, GRAD_CHUNK - 1, GRAD_CHUNK, 1099):     # inside the first chunk, its last row, the second's first, the end
        Xb = rng.uniform(lo, hi, (1100, c.d))
        Xb[at] = x
        lp, g = dm.logpost_grad(Xb)
        lp2, g2 = dm.logpost_grad(Xb)
        assert np.array_equal(lp, lp2) and np.array_equal(g, g2), "the same call twice"
        assert lp[at] == alone[0][0] and np.array_equal(g[at], alone[1][0]), f"row {at} of 1100 differs from the row alone"
        jb = dm.gp_predict_grad(Xb)
        for a, b in zip(ja, jb):
            assert np.array_equal(a[0], b[at])
    dm.close()


def test_box_rows_and_their_neighbours():
    c, model, dm, lo, hi, rng = _mid_model()
    X = rng.uniform(lo, hi, (9, c.d))
    ref_lp, ref_g = dm.logpost_grad(X)
    Y = X.copy()
    Y[1, 0] = lo[0]                       # on the edge
    Y[3, 1] = hi[1]
    Y[4, 2] = hi[2] + 1.0                 # outside
    Y[6, 0] = np.nan                      # fails the box prior
    Y[7, 1] = -np.inf
    bad = [1, 3, 4, 6, 7]
    lp, g = dm.logpost_grad(Y)
    assert np.all(lp[bad] == -np.inf) and np.all(g[bad] == 0.0)
    good = [0, 2, 5, 8]
    assert np.array_equal(lp[good], ref_lp[good]) and np.array_equal(g[good], ref_g[good]), "neighbours of a row outside"
    assert np.array_equal(np.isfinite(lp), np.isfinite(dm.logpost(Y))), "the box of the value call"
    with pytest.raises(ValueError):
        dm.gp_predict_grad(Y)
    dm.close()


def _refused(call):
    c0 = counts()
    with pytest.raises(_lib.GpemuError) as ei:
        call()
    assert ei.value.code == -5, ei.value
    assert np.array_equal(counts(), c0), "a refused call must not launch"
    return str(ei.value)


def test_refusals():
    by_name = {c.name: c for c in PC.cases()}
    X1 = None
    for name, word in (("n15_d8_ksteps3_m05", "nu = 0.5"), ("n63_nu075_direct", "nu = 0.75")):
        c = by_name[name]
        model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
        dm = GU.device_model(model)
        dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
        X1 = rng.uniform(lo, hi, (5, c.d))
        before = dm.logpost(X1)
        assert word in _refused(lambda: dm.logpost_grad(X1))
        assert word in _refused(lambda: dm.gp_predict_grad(X1))
        assert word in _refused(lambda: M.logpost_groups_grad([dm], X1))
        assert np.array_equal(dm.logpost(X1), before), "logpost after a refused gradient call"
        dm.close()
    # a group with sources, and the exact form
    c, model, dm, lo, hi, rng = _mid_model()
    X = rng.uniform(lo, hi, (5, c.d))
    before = dm.logpost(X)
    assert "EXACT" in _refused(lambda: dm.logpost_grad(X, mode=M.EXACT))
    assert "EXACT" in _refused(lambda: M.logpost_groups_grad([dm], X, mode=M.EXACT))
    assert np.array_equal(dm.logpost(X), before)
    _, _, _, y_exp, y_err, bs, _ = PC.problem(c)
    F = len(y_exp)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs, sys_sources=0.05 * np.ones((1, F)))
    before = M.logpost_groups([dm], X)
    assert "sources" in _refused(lambda: dm.logpost_grad(X))
    assert "sources" in _refused(lambda: M.logpost_groups_grad([dm], X))
    assert np.array_equal(M.logpost_groups([dm], X), before)
    # a likelihood set up for several data vectors (the stacked closure chains)
    dm.likelihood_setup(np.stack([y_exp, y_exp + 0.01]), y_err, lo, hi, 1.0, block_start=bs)
    assert "data vectors" in _refused(lambda: dm.logpost_grad(X))
    assert "data vectors" in _refused(lambda: M.logpost_groups_grad([dm], X))
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    lp_back, _ = dm.logpost_grad(X)
    assert np.all(np.isfinite(lp_back)), "a single data vector again: the path runs"
    dm.close()


def test_dense_within_observable_data_covariance():
    """cov inside the observable blocks changes the setup constants only: lp and grad against the reference built on
    grad_ref.setups_with_cov; cov = diag(y_err^2) gives the bits of the setup without cov"""
    c, model, dm, lo, hi, rng = _mid_model()
    _, _, _, y_exp, y_err, bs, _ = PC.problem(c)
    X = rng.uniform(lo, hi, (24, c.d))
    plain = dm.logpost_grad(X)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs, cov=np.diag(y_err ** 2))
    same = dm.logpost_grad(X)
    assert np.array_equal(plain[0], same[0]) and np.array_equal(plain[1], same[1])
    F = len(y_err)
    i = np.arange(F)
    obs = np.searchsorted(np.asarray(bs)[1:], i, side="right")
    cov = np.where(obs[:, None] == obs[None, :], np.outer(y_err, y_err) * np.exp(-np.abs(i[:, None] - i[None, :]) / 3.0), 0.0)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs, cov=cov)
    lp_d, g_d = dm.logpost_grad(X)
    assert np.max(np.abs(g_d - plain[1])) > 1e-3, "the covariance must matter"
    setups = G.setups_with_cov(model, y_exp, cov, bs)
    ref = G.reference(X, model, y_exp, y_err, bs, setups=setups)
    mean, var, mb, vb, _ = H.gp_predict(X, model)
    lp_ref = H.loglik_blocks(mean, var, setups)[0]
    lb = H.loglik_bound(mean, var, mb, vb, setups)
    r_lp = within("lp with cov", lp_d, lp_ref, lb)
    r_g = within("grad with cov", g_d, ref["grad"], ref["grad_bound"])
    within("the value call's lp with cov", dm.logpost(X), lp_ref, lb)
    print(f"\nGRAD RATIOS dense covariance lp={r_lp:.3g} grad={r_g:.3g}")
    dm.close()


# ---- the shipped three-group shape (golden G7) ----------------------------------------------------------------------
class _GroupCfg:
    def __init__(self, n_pc):
        self.n_pc = n_pc


class _EmuCfg:
    def __init__(self, groups, sorter):
        self.emulation_groups_config = groups
        self.sort_observables_in_matrix = sorter


def _sub(g, name):
    sub = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_")}
    sub.update(design=g["design"], gpr_alpha=g["gpr_alpha"])
    return sub


def _shipped():
    from bayesian_inference import emulation
    g = GU.load("g7_shipped_config")
    names, mapping, block_start, cols = GU.g7_groups(g)
    sorter = emulation.SortEmulationGroupObservables(mapping, tuple(int(v) for v in g["map_shape"]))
    res = {n: DU.results_at_golden_theta(_sub(g, n)) for n in names}
    cfgs = {n: _GroupCfg(int(g[n + "_n_pc"])) for n in names}
    return g, names, mapping, block_start, cols, res, _EmuCfg(cfgs, sorter)


def _ref_model(res, n_pc):
    """the reference's view of what the drop-in uploads for a results dict: the emulators' own X_train_, kernel_,
    alpha_ and L_, the PCA and the scaler"""
    emus = res["emulators"][:n_pc]
    k0 = emus[0].kernel_
    spec = O.KernelSpec(kind=k0.kind, nu=k0.nu, has_const=k0.has_const, has_noise=k0.has_noise)
    gps = [types.SimpleNamespace(ls=np.asarray(e.kernel_.length_scale, dtype=np.float64),
                                 const=float(e.kernel_.constant_value) if k0.has_const else 0.0,
                                 noise=float(e.kernel_.noise_level) if k0.has_noise else 0.0,
                                 alpha=np.asarray(e.alpha_, dtype=np.float64), L=np.asarray(e.L_, dtype=np.float64))
           for e in emus]
    pca, scaler = res["PCA"]["pca"], res["PCA"]["scaler"]
    return O.GroupModel(X_train=np.asarray(emus[0].X_train_, dtype=np.float64), spec=spec, gps=gps,
                        components=pca.components_, explained_variance=pca.explained_variance_,
                        scaler_mean=scaler.mean_, scaler_scale=scaler.scale_, n_pc=n_pc)


def test_groups_gradient_is_the_sum_of_the_group_references():
    g = GU.load("g7_shipped_config")
    names, mapping, block_start, cols = GU.g7_groups(g)
    models = GU.g7_models(g)
    dms = []
    for n in names:
        dm = GU.device_model(models[n])
        dm.likelihood_setup(g["y_exp"][cols[n]], g["y_err"][cols[n]], g["lo"], g["hi"], 1.0, block_start=block_start[n])
        dms.append(dm)
    X = g["Xq"][:12]
    lp_d, g_d = M.logpost_groups_grad(dms, X)
    lp_ref, lp_b = np.zeros(len(X), LD), np.zeros(len(X))
    g_ref, g_b, g_abs = np.zeros(X.shape, LD), np.zeros(X.shape), np.zeros(X.shape)
    for n in names:
        bs = np.asarray(block_start[n], dtype=np.int64)
        ref = G.reference(X, models[n], g["y_exp"][cols[n]], g["y_err"][cols[n]], bs)
        assert not ref["ambiguous"].any() and not ref["clipped"].any()
        lp, lb, _ = H.log_posterior(X, models[n], g["lo"], g["hi"], g["y_exp"][cols[n]], g["y_err"][cols[n]], bs)
        lp_ref += lp
        lp_b += lb
        g_ref += ref["grad"]
        g_b += ref["grad_bound"]
        g_abs += np.abs(np.asarray(ref["grad"], dtype=np.float64))
        # one group alone equals its own reference as well
        lp1, g1 = dms[names.index(n)].logpost_grad(X)
        within(f"{n} grad", g1, ref["grad"], ref["grad_bound"])
    assert np.all(np.isfinite(lp_d))
    r_lp = within("groups lp", lp_d, lp_ref, lp_b + 4 * H.U * np.abs(np.asarray(lp_ref, float)))
    r_g = within("groups grad", g_d, g_ref, g_b + 4 * H.U * g_abs)        # (the groups' terms are added in turn: 2 adds)
    print(f"\nGRAD RATIOS G7 groups lp={r_lp:.3g} grad={r_g:.3g}")
    for dm in dms:
        dm.close()


def test_dropin_jacobian_and_sensitivity_on_the_shipped_shape():
    from bayesian_inference import emulation
    g, names, mapping, block_start, cols, res, emu_cfg = _shipped()
    X = g["Xq"][:6]
    plain = emulation.predict(X, emu_cfg, emulation_group_results=res)
    out = emulation.predict(X, emu_cfg, emulation_group_results=res, return_jacobian=True)
    assert np.array_equal(plain["central_value"], out["central_value"]) and np.array_equal(plain["cov"], out["cov"])
    assert set(plain) == {"central_value", "cov"} and set(out) == {"central_value", "cov", "jacobian"}
    F, d = plain["central_value"].shape[1], X.shape[1]
    assert out["jacobian"].shape == (len(X), F, d)
    J_ref, J_b = np.zeros((len(X), F, d), LD), np.zeros((len(X), F, d))
    for n in names:
        k = emu_cfg.emulation_groups_config[n].n_pc
        rm = _ref_model(res[n], k)
        jr = G.gp_jacobian(X, rm)
        comp, s = rm.components[:k], rm.scaler_scale
        jg = np.einsum("bpi,pf->bfi", jr["dmean"], comp.astype(LD)) * s.astype(LD)[None, :, None]
        ja = np.einsum("bpi,pf->bfi", np.abs(np.asarray(jr["dmean"], float)), np.abs(comp)) * s[None, :, None]
        jb = np.einsum("bpi,pf->bfi", jr["dmean_bound"], np.abs(comp)) * s[None, :, None] + (k + 4) * H.U * ja
        for _, (grp, so, sg) in mapping.items():
            if grp == n:
                J_ref[:, so, :] = jg[:, sg, :]
                J_b[:, so, :] = jb[:, sg, :]
    r = within("jacobian", out["jacobian"], J_ref, J_b)
    S = emulation.sensitivity(X, emu_cfg, emulation_group_results=res)
    assert np.array_equal(S, emulation.normalised_sensitivity(out["jacobian"], X, out["central_value"]))
    print(f"\nGRAD RATIOS G7 jacobian={r:.3g}")
    emulation.release_device_models()


def test_find_map_certificate_on_the_shipped_shape():
    """find_map on G7's data, certified the way the fit is (dropin_util.certify_fit_against_reference)."""
    from bayesian_inference import emulation, log_posterior, mcmc
    g, names, mapping, block_start, cols, res, emu_cfg = _shipped()
    lo, hi = np.asarray(g["lo"], dtype=np.float64), np.asarray(g["hi"], dtype=np.float64)
    d = lo.size
    log_posterior.initialize_pool_variables(lo, hi, emu_cfg, res, {"y": g["y_exp"], "y_err": g["y_err"]}, None)
    try:
        np.random.seed(7)
        sampler = mcmc.LoggingEnsembleSampler(32, d, log_posterior.log_posterior)
        sampler.run_mcmc(np.random.uniform(lo, hi, (32, d)), 80, n_logging_steps=40)
        chain, lp_chain = sampler.get_chain(), sampler.get_log_prob()
        found = mcmc.find_map_on_pool(lo, hi, n_starts=16, chain=chain, log_prob=lp_chain)
        assert found["all_parameters"].shape == (16, d) and found["status"].shape == (16,) and found["nfev"].shape == (16,)
        x_map = found["map_parameters"]
        assert np.all(x_map > lo) and np.all(x_map < hi)

        refs = {n: _ref_model(res[n], emu_cfg.emulation_groups_config[n].n_pc) for n in names}
        cus = {n: emulation.compute_emulator_group_cov_unexplained(emu_cfg.emulation_groups_config[n], res[n]) for n in names}

        def reference(x, bound=False):
            """(lp, grad[, lp bound]) of the three groups at x, extended precision"""
            lp, lb, gr = LD(0), 0.0, np.zeros(d, LD)
            for n in names:
                bs = np.asarray(block_start[n], dtype=np.int64)
                ye, yr = g["y_exp"][cols[n]], g["y_err"][cols[n]]
                ref = G.reference(x[None], refs[n], ye, yr, bs, cov_unexpl=cus[n])
                lp += ref["lp"][0]
                gr += ref["grad"][0]
                if bound:
                    lb += H.log_posterior(x[None], refs[n], lo, hi, ye, yr, bs, cov_unexpl=cus[n])[1][0]
            return (lp, gr, lb) if bound else (lp, gr)

        # (i) no worse than the chain's best point (both values within bound of the reference there)
        best = np.unravel_index(np.argmax(lp_chain), lp_chain.shape)
        _, _, lb_best = reference(chain[best], bound=True)
        print(f"\n[MAP] chain best {lp_chain[best]:.6f}, map_log_prob {found['map_log_prob']:.6f}, nfev {found['nfev'].tolist()}, "
              f"status {found['status'].tolist()}")
        assert found["map_log_prob"] >= lp_chain[best] - 2 * lb_best
        # (ii) the device's value at the MAP is the reference's
        lp_ref, g_ref, lb = reference(x_map, bound=True)
        lp_dev = log_posterior.log_posterior_and_gradient(x_map[None])[0][0]
        assert lp_dev == found["map_log_prob"]
        within("lp at the MAP", np.array([lp_dev]), np.array([lp_ref]), np.array([lb + 4 * H.U * abs(float(lp_ref))]))

        # (iii) the reference's arithmetic stops there: L-BFGS-B from x within one iteration, gain below ftol
        from gpemu import mapfit
        bounds = mapfit.open_box_bounds(lo, hi)

        def neg(x):
            lp, gr = reference(np.asarray(x, dtype=np.float64))
            return -float(lp), -np.asarray(gr, dtype=np.float64)

        def stops_at(x):
            f0 = neg(x)[0]
            r = scipy.optimize.minimize(neg, x, method="L-BFGS-B", jac=True, bounds=bounds, options={"maxiter": 3})
            gain = (f0 - r.fun) / max(abs(f0), 1.0)
            print(f"[MAP] reference-driven L-BFGS-B: {r.nit} iteration(s), gain {gain / DU.FTOL:.3g} ftol, status {r.status}")
            return r.status == 0 and r.nit <= 1 and gain <= DU.FTOL
        assert stops_at(x_map), "the MAP is not a point L-BFGS-B stops at in the reference's arithmetic"
        # teeth: one posterior standard deviation along one coordinate is rejected
        Hm = found["hessian"]
        assert Hm.shape == (d, d)
        sig = np.sqrt(np.diag(np.linalg.inv(-Hm)))
        i = int(np.argmax(np.minimum(x_map - lo, hi - x_map) / sig))      # the coordinate with the most room
        step = sig[i] if x_map[i] + sig[i] < hi[i] else -sig[i]
        x_off = x_map.copy()
        x_off[i] += step
        assert lo[i] < x_off[i] < hi[i]
        drop = found["map_log_prob"] - log_posterior.log_posterior_and_gradient(x_off[None])[0][0]
        print(f"[MAP] one sigma along coordinate {i}: lp drops by {drop:.3f}")
        assert drop > 0.2, "half a unit in the quadratic approximation, never less: far more than ftol"
        assert not stops_at(x_off), "the certificate accepts a point one standard deviation from the MAP"
    finally:
        log_posterior.initialize_pool_variables(None, None, None, None, None, None)


def _g1_analysis(tmp_path, monkeypatch, sys_sources=False):
    """the G1 fixture through the drop-in's YAML route: fitted emulators, (path, analysis, written, h5io)"""
    from bayesian_inference import emulation
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    written = {}
    io = DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    io.read_dict_from_h5 = lambda output_dir, filename, verbose=True: h5io.read_dict_from_h5(output_dir, filename)
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    if sys_sources:
        np.savez(tmp_path / "dcov.npz", sys_sources=0.05 * np.ones((1, g["y_exp"].shape[0])))
        analysis["parameters"]["mcmc"]["data_covariance"] = "dcov.npz"
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(1)
    emulation.fit_emulators(ec)
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    return path, analysis, written, h5io


USUAL = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}


def test_run_mcmc_find_map_key_with_a_declined_configuration_costs_no_chain(tmp_path, monkeypatch):
    """find_map: true with fully correlated sources (no gradient path): run_mcmc says so BEFORE the first step -- no
    sampler is built, nothing is run and lost; without the key the same configuration samples and writes as ever"""
    import os
    from bayesian_inference import log_posterior, mcmc
    path, analysis, written, h5io = _g1_analysis(tmp_path, monkeypatch, sys_sources=True)
    analysis["parameters"]["mcmc"]["find_map"] = True
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    built = []
    real = mcmc.LoggingEnsembleSampler

    class Counting(real):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)
    monkeypatch.setattr(mcmc, "LoggingEnsembleSampler", Counting)
    with pytest.raises(ValueError, match="find_map.*sys_sources"):
        mcmc.run_mcmc(cfg)
    assert not built and not os.path.exists(cfg.mcmc_outputfile), "refused before any sampling"
    monkeypatch.setattr(mcmc, "LoggingEnsembleSampler", real)       # (the sampler is pickled: the real class again)
    analysis["parameters"]["mcmc"]["find_map"] = False
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    np.random.seed(2)
    mcmc.run_mcmc(cfg)
    assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == USUAL
    log_posterior.initialize_pool_variables(None, None, None, None, None, None)


def test_run_mcmc_writes_the_chain_when_the_maximisation_fails(tmp_path, monkeypatch, caplog):
    """an error inside the maximisation (here: injected) after production: mcmc.h5 and the pickle are written with the
    usual entries, the failure is logged"""
    import logging
    import os
    from bayesian_inference import log_posterior, mcmc
    path, analysis, written, h5io = _g1_analysis(tmp_path, monkeypatch)
    analysis["parameters"]["mcmc"]["find_map"] = True
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)

    def broken(*a, **k):
        raise RuntimeError("injected failure of the gradient path")
    monkeypatch.setattr(mcmc, "find_map_on_pool", broken)
    np.random.seed(2)
    with caplog.at_level(logging.WARNING, logger=mcmc.logger.name):
        mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == USUAL and back["chain"].shape[0] == cfg.n_sampling_steps
    assert os.path.exists(cfg.sampler_outputfile)
    assert any("injected failure" in r.getMessage() and "without" in r.getMessage() for r in caplog.records)
    log_posterior.initialize_pool_variables(None, None, None, None, None, None)


def test_run_mcmc_find_map_key_and_find_map_from_the_stored_chain(tmp_path, monkeypatch):
    """parameters.mcmc.find_map: absent, mcmc.h5 holds the four usual entries; true, three more, and the maximum is no
    worse than the chain's best point.  mcmc.find_map(config) then starts from the stored chain."""
    from bayesian_inference import emulation, log_posterior, mcmc
    from gpemu import h5io
    g = GU.load("g1_rbf_noise")
    written = {}
    io = DU.install_fake_data_IO(g["Y"], g["design"], g["y_exp"], g["y_err"], written)
    io.read_dict_from_h5 = lambda output_dir, filename, verbose=True: h5io.read_dict_from_h5(output_dir, filename)
    path, analysis = DU.write_config(tmp_path, n_pc=5, n_restarts=0)
    ec = emulation.EmulationConfig.from_config_file("test_analysis", "exponential", path, analysis)
    ec._sort_observables_in_matrix = None
    np.random.seed(1)
    emulation.fit_emulators(ec)
    monkeypatch.setattr(emulation.EmulationConfig, "sort_observables_in_matrix",
                        property(lambda self: DU.TrivialSort("main")))
    monkeypatch.setattr(emulation.EmulationConfig, "observable_filter", property(lambda self: None))
    usual = {"chain", "acceptance_fraction", "log_prob", "autocorrelation_time"}
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.find_map is False
    np.random.seed(2)
    mcmc.run_mcmc(cfg)
    assert set(h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)) == usual
    analysis["parameters"]["mcmc"]["find_map"] = True
    cfg = mcmc.MCMCConfig("test_analysis", "exponential", analysis, path)
    assert cfg.find_map is True
    np.random.seed(2)
    mcmc.run_mcmc(cfg)
    back = h5io.read_dict_from_h5(cfg.mcmc_output_dir, cfg.mcmc_outputfilename)
    assert set(back) == usual | {"map_parameters", "map_log_prob", "map_hessian"}
    box = analysis["parameterization"]["exponential"]
    lo, hi = np.asarray(box["min"], float), np.asarray(box["max"], float)
    d = lo.size
    x = back["map_parameters"]
    assert x.shape == (d,) and np.all(x > lo) and np.all(x < hi)
    assert back["map_hessian"].shape == (d, d) and np.array_equal(back["map_hessian"], back["map_hessian"].T)
    # the start with the chain's best log-probability cannot end below it (the value call's and this path's lp differ
    # in rounding only: 1e-9 relative is far above both bounds)
    best = float(np.max(back["log_prob"]))
    assert float(back["map_log_prob"]) >= best - 1e-9 * max(1.0, abs(best))
    lp_at, _ = log_posterior.log_posterior_and_gradient(x[None])
    assert lp_at[0] == float(back["map_log_prob"])
    found = mcmc.find_map(cfg, n_starts=8)
    assert found["all_parameters"].shape == (8, d) and found["status"].shape == (8,) and found["nfev"].shape == (8,)
    assert found["map_log_prob"] >= best - 1e-9 * max(1.0, abs(best))
    assert found["hessian"].shape == (d, d)
    print(f"\n[MAP] run_mcmc key: chain best {best:.6f}, map {float(back['map_log_prob']):.6f}; find_map from mcmc.h5 "
          f"{found['map_log_prob']:.6f}, status {found['status'].tolist()}")
    log_posterior.initialize_pool_variables(None, None, None, None, None, None)
