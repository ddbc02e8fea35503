"""-m gpu: the sequential-design criterion (gpemu_design_*) against the extended-precision reference of
tests/design_ref.py, candidate by candidate within its a-priori bound: first-round scores for every kernel kind and
padded width, weights, the greedy conditioning, the workspace's chunking, several groups, the samplers' stored chains
and the unfused composition of gpemu_gp_predict_cov.

The candidates of every case hold a training row (0), a duplicate pair (1, 2) and a far point (last)."""
import math

import numpy as np
import pytest

import design_ref as DR
import golden_util as GU
import matern_nu_ref as R
from gpemu import _lib
from gpemu import design as DS
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble

KERNELS = {"rbf": (O.RBF, math.inf), "m05": (O.MATERN, 0.5), "m15": (O.MATERN, 1.5), "m25": (O.MATERN, 2.5),
           "nu075": (O.MATERN, 0.75), "nuinf": (O.MATERN, math.inf)}


def synth(kernel, cn, d, N, k=2, seed=0):
    """a GroupModel fitted at fixed theta on a random design in [0, 1]^d (noise-free forms: jitter 1e-8)"""
    kind, nu = KERNELS[kernel]
    rng = np.random.default_rng(seed + 1000 * d + N)
    X = rng.uniform(0.0, 1.0, (N, d))
    spec = O.KernelSpec(kind=kind, nu=nu, has_const=cn, has_noise=cn)
    gps = []
    for p in range(k):
        ls = 0.35 * math.sqrt(d) * (1.0 + 0.3 * p) * rng.uniform(0.8, 1.25, d)
        y = np.sin(X @ rng.normal(size=d) * 3.0) + 0.1 * p
        theta = np.log(np.r_[ls, [0.7] if cn else [], [0.01] if cn else []])
        with R.general_nu():
            gps.append(O.gp_fit_at_theta(X, y, theta, spec, 1e-10 if cn else 1e-8))
    F = 3
    return O.GroupModel(X_train=X, spec=spec, gps=gps, components=rng.normal(size=(k, F)),
                        explained_variance=np.ones(k), scaler_mean=np.zeros(F), scaler_scale=np.ones(F), n_pc=k)


def queries(model, M, seed, special=True):
    """M rows in and around the design; with `special`: a training row (0), a duplicate pair (1, 2), one far query"""
    d = model.X_train.shape[1]
    X = np.random.default_rng(seed).uniform(-0.1, 1.1, (M, d))
    if special and M >= 4:
        X[0] = model.X_train[3]
        X[2] = X[1]
        X[-1] = 4.0
    return X


def sets(model, S, M, seed=1):
    return queries(model, S, seed, special=False), queries(model, M, seed + 1)


def check_scores(what, dev, ref, allow_near=0):
    """dev [M] against DesignRef.scores(): every candidate within its bound; one whose den lies within its own bound of
    the floor may also have fallen on the other side of it (score 0, or the unfloored quotient)"""
    score, bound, near, _ = ref.scores()
    err = np.abs(np.asarray(dev, dtype=LD) - score).astype(np.float64)
    ok = err <= bound
    loose = near & ~ok
    top = float(np.max(score))
    rel = np.max(np.where(np.isfinite(bound), bound, 0.0)) / top if top > 0 else 0.0
    print(f"{what}: max err / bound {np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))):.3g}, "
          f"max bound / top score {rel:.3g}, near the floor: {int(near.sum())}")
    assert int(near.sum()) <= allow_near, f"{what}: {int(near.sum())} candidates lie within their bound of the floor"
    bad = np.flatnonzero(~ok & ~loose)
    assert bad.size == 0, (f"{what}: candidate {bad[0]}: dev {dev[bad[0]]!r} ref {float(score[bad[0]])!r} "
                           f"bound {bound[bad[0]]:.3g}")
    assert np.all(np.asarray(dev)[(np.asarray(score, dtype=np.float64) == 0.0) & ~near] == 0.0), f"{what}: floor rule"
    return score, bound


# ---- 1. first-round scores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 6, 8, 9, 16])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_scores_within_the_bound(kernel, d):
    """N = 50, S = 130, M = 70: three row tiles and two column tiles, neither a multiple of 64"""
    model = synth(kernel, True, d, 50)
    Xref, Xcand = sets(model, 130, 70)
    dm = GU.device_model(model)
    try:
        with dm.design(Xref, Xcand) as ds:
            dev = ds.scores()
            per = ds._groups[0].scores(per_pc=True)[1]
        ref = DR.DesignRef(model, Xref, Xcand)
        score, bound = check_scores(f"{kernel} d={d}", dev, ref)
        assert np.max(bound / np.asarray(score, dtype=np.float64)) <= 1.2e-7      # noisy: no candidate is left out
        total = per[0].copy()
        for row in per[1:]:
            total += row
        assert np.array_equal(total, dev)                          # the PCs' terms, added in index order
    finally:
        dm.close()


@pytest.mark.parametrize("kernel,d,N,S,M", [("m25", 6, 150, 130, 70), ("rbf", 6, 1000, 300, 130)])
def test_scores_at_larger_designs(kernel, d, N, S, M):
    """N = 150 crosses the 128 padding of the model; N = 1000 is the flagship design size (one PC: the reference's
    substitution in extended precision takes seconds per PC there)"""
    model = synth(kernel, True, d, N, k=1 if N >= 1000 else 2)
    Xref, Xcand = sets(model, S, M)
    Xcand[3] = model.X_train[N - 1]
    dm = GU.device_model(model)
    try:
        with dm.design(Xref, Xcand) as ds:
            dev = ds.scores()
        check_scores(f"{kernel} N={N}", dev, DR.DesignRef(model, Xref, Xcand))
    finally:
        dm.close()


@pytest.mark.parametrize("kernel,d,N", [("rbf", 6, 150), ("m25", 2, 50)])
def test_noise_free_models_and_the_floor(kernel, d, N):
    """tau = 0 and no White level: the training-row candidate (den ~ 1e-8, the fit's jitter) is under the floor and
    scores exactly 0 on the device and in the reference, as does every other candidate the reference puts under the
    floor (CPU run of these seeds: no candidate lies within its bound of the floor)"""
    model = synth(kernel, False, d, N)
    Xref, Xcand = sets(model, 130, 70)
    dm = GU.device_model(model)
    try:
        with dm.design(Xref, Xcand) as ds:
            dev = ds.scores()
            den = ds._groups[0].state(den=True)[1]
        ref = DR.DesignRef(model, Xref, Xcand)
        check_scores(f"noise-free {kernel}", dev, ref, allow_near=1)
        assert dev[0] == 0.0 and float(ref.scores()[0][0]) == 0.0
        assert np.all(np.abs(den[:, 0]) < 1e-6) and np.all(dev >= 0.0)
    finally:
        dm.close()


# ---- 2. weights ---------------------------------------------------------------------------------------------------------
def test_weights():
    model = synth("m15", True, 6, 50)
    Xref, Xcand = sets(model, 130, 70)
    w = np.random.default_rng(3).uniform(0.1, 2.0, 130)
    w[17] = 0.0
    fw = np.array([0.5, 2.0, 1.0])
    dm = GU.device_model(model)
    try:
        with dm.design(Xref, Xcand, weights=w, feature_weights=fw, tau=[0.02, 0.0]) as ds:
            dev = ds.scores()
        ref = DR.DesignRef(model, Xref, Xcand, weights=w, tau=[0.02, 0.0], pcw=DR.pc_weights(model, fw))
        score, bound = check_scores("non-uniform weights", dev, ref)
        assert np.array_equal(DS.pc_weights(dm, fw), DR.pc_weights(model, fw))
        # a row of weight 0 is the same call without the row, within the two bounds
        keep = np.arange(130) != 17
        with dm.design(Xref[keep], Xcand, weights=w[keep], feature_weights=fw, tau=[0.02, 0.0]) as ds:
            without = ds.scores()
        assert np.all(np.abs(without - dev) <= 2 * bound)
        # scaling the weights by a constant changes nothing, bit for bit.  The constant is a power of two: the call
        # normalises by the sum in index order, and only then are c w_s and the sum both exact multiples
        with dm.design(Xref, Xcand, weights=4.0 * w, feature_weights=fw, tau=[0.02, 0.0]) as ds:
            assert np.array_equal(ds.scores(), dev)
    finally:
        dm.close()


# ---- 3. conditioning ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,d,tau", [("rbf", 6, None), ("m25", 9, [0.0, 0.0]), ("nu075", 6, None)])
def test_conditioning_over_five_picks(kernel, d, tau):
    model = synth(kernel, True, d, 50)
    Xref, Xcand = sets(model, 130, 70)
    dm = GU.device_model(model)
    try:
        ref = DR.DesignRef(model, Xref, Xcand, tau=tau)
        with dm.design(Xref, Xcand, tau=None if tau is None else [tau], max_picks=5) as ds:
            g = ds._groups[0]
            picks = []
            for rnd in range(5):
                dev = ds.scores()
                score, bound = check_scores(f"{kernel} round {rnd}", dev, ref)
                s64 = np.asarray(score, dtype=np.float64)
                pick = int(np.argmax(dev))
                assert s64[pick] + bound[pick] >= np.max(s64 - bound), f"round {rnd}: pick {pick} is not certified"
                iv0, den0, n = g.state(den=True)
                assert n == rnd
                rden, rdden = ref.den()
                assert np.all(np.abs(np.asarray(den0, dtype=LD) - rden).astype(np.float64) <= rdden)
                riv, rdiv = ref.iv()
                assert np.all(np.abs(np.asarray(iv0, dtype=LD) - riv).astype(np.float64) <= rdiv)
                total0, dtotal0 = ref.integrated_variance()
                before = ds.integrated_variance()
                ds.condition(pick)
                ref.condition(pick)
                after = ds.integrated_variance()
                total1, dtotal1 = ref.integrated_variance()
                assert abs((before - after) - dev[pick]) <= bound[pick] + dtotal0 + dtotal1, f"round {rnd}: IV drop"
                picks.append(pick)
                if tau is not None:
                    assert ds.scores()[pick] == 0.0, "a pick with tau = 0 must score 0 afterwards"
            assert len(set(picks)) == 5 and ds.picks == picks
            with pytest.raises(ValueError):
                ds.condition(0)                                    # beyond max_picks
            assert _lib.lib().gpemu_design_condition(g._h, 0) == -1
            assert _lib.lib().gpemu_design_condition(g._h, 70) == -1
    finally:
        dm.close()


def test_select_is_the_loop_of_scores_and_condition():
    model = synth("rbf", True, 6, 50)
    Xref, Xcand = sets(model, 130, 70)
    dm = GU.device_model(model)
    try:
        with dm.design(Xref, Xcand, max_picks=20) as ds:
            out = ds.select(18)                                    # past one 16-row k-tile of picks
        with dm.design(Xref, Xcand, max_picks=20) as ds:
            first = ds.scores()
            for j, i in enumerate(out["indices"]):
                s = ds.scores()
                assert int(np.argmax(s)) == i and s[i] == out["gain"][j]
                ds.condition(i)
                assert ds.integrated_variance() == out["integrated_variance"][j + 1]
        assert np.array_equal(first, out["first_scores"]) and np.array_equal(out["points"], Xcand[out["indices"]])
        assert np.all(np.diff(out["integrated_variance"]) < 0) and len(set(out["indices"].tolist())) == 18
    finally:
        dm.close()


# ---- 4. memory ------------------------------------------------------------------------------------------------------------
def run_twice(dm, Xref, Xcand, ws):
    """(first-round scores, scores after one pick, chunks per scores call) under workspace_bytes = ws"""
    before = DS.path_counts()
    with dm.design(Xref, Xcand, workspace_bytes=ws) as ds:
        s = ds.scores()
        ds.condition(int(np.argmax(s)))
        s2 = ds.scores()
    after = DS.path_counts()
    chunks = (after["chunk"] - before["chunk"]) // 2
    assert after["scores"] - before["scores"] == 2 and after["column"] - before["column"] == 1
    assert after["dp8"] - before["dp8"] == after["kind_rbf"] - before["kind_rbf"] == 2 * chunks
    return s, s2, chunks


def test_the_workspace_bounds_memory_and_does_not_change_the_bits():
    """S = 4096, M = 2048, k = 2, N = 50: the S x M matrix of both PCs would be 134 MB; 32 MiB suffice.  Same bits for
    32 MiB, 256 MiB and the default, and between two runs"""
    model = synth("rbf", True, 6, 50)
    Xref, Xcand = sets(model, 4096, 2048)
    dm = GU.device_model(model)
    try:
        base = run_twice(dm, Xref, Xcand, 32 << 20)
        for ws in (256 << 20, 0, 32 << 20):
            got = run_twice(dm, Xref, Xcand, ws)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2] == 1, ws
        with pytest.raises(_lib.GpemuError) as e:
            dm.design(Xref, Xcand, workspace_bytes=4 << 20)
        assert e.value.code == -1 and "bytes are needed" in str(e.value)
        score, bound, _, _ = DR.DesignRef(model, Xref[:64], Xcand[:6]).scores()      # a spot check of the layout
        with dm.design(Xref[:64], Xcand[:6]) as ds:
            assert np.all(np.abs(ds.scores() - np.asarray(score, dtype=np.float64)) <= bound)
    finally:
        dm.close()


def test_chunks_of_candidate_tiles_give_the_same_bits():
    """k = 3: the smallest workspace the call accepts (the operands, and the create call's work array of N64 x S64
    doubles, which the partials then reuse) holds the partials of 1344 of the 2048 candidates: two chunks"""
    model = synth("rbf", True, 6, 50, k=3)
    Xref, Xcand = sets(model, 4096, 2048)
    k, Kcap, Sp, Mp, d = 3, 64 + 32, 4096, 2048, 6
    least = (k * Kcap * (Sp + Mp) + k * Sp + 2 * k * Mp + Sp + Mp + (Sp + Mp) * d + 64 * Sp) * 8
    dm = GU.device_model(model)
    try:
        whole = run_twice(dm, Xref, Xcand, 0)
        parts = run_twice(dm, Xref, Xcand, least)
        assert whole[2] == 1 and parts[2] == 2
        assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])
        with pytest.raises(_lib.GpemuError) as e:
            dm.design(Xref, Xcand, workspace_bytes=least - 8)
        assert e.value.code == -1 and str(least) in str(e.value)
    finally:
        dm.close()


# ---- 5. groups and samplers -------------------------------------------------------------------------------------------------
def test_three_groups_are_the_sum_of_the_groups():
    g = GU.load("g7_shipped_config")
    models = GU.g7_models(g)
    names, _, _, cols = GU.g7_groups(g)
    dms = [GU.device_model(models[n]) for n in names]
    try:
        X = models[names[0]].X_train
        rng = np.random.default_rng(8)
        lo, hi = X.min(axis=0), X.max(axis=0)
        Xref, Xcand = rng.uniform(lo, hi, (200, X.shape[1])), rng.uniform(lo, hi, (70, X.shape[1]))
        Xcand[0] = X[3]
        F = sum(len(cols[n]) for n in names)
        fw = rng.uniform(0.5, 2.0, F)
        with DS.Design(dms, Xref, Xcand, feature_weights=fw, feature_columns=[cols[n] for n in names]) as ds:
            total, per = ds.scores(), ds.scores_per_group()
            iv = ds.integrated_variance()
        want, want_iv = None, 0.0
        for i, (n, dm) in enumerate(zip(names, dms)):
            with dm.design(Xref, Xcand, feature_weights=fw[cols[n]]) as one:
                s = one.scores()
                want_iv += one.integrated_variance()
            assert np.array_equal(s, per[i])
            want = s.copy() if want is None else want + s
        assert np.array_equal(total, want) and iv == want_iv
        ref = DR.DesignRef(models[names[1]], Xref, Xcand, pcw=DR.pc_weights(models[names[1]], fw[cols[names[1]]]))
        check_scores("G7 group 1", per[1], ref, allow_near=1)
    finally:
        for dm in dms:
            dm.close()


def test_propose_design_reads_the_stored_chain_in_place():
    from gpemu.sampler import DeviceSampler
    model = synth("rbf", True, 6, 50)
    rng = np.random.default_rng(9)
    d, W = 6, 16
    lo, hi = np.zeros(d), np.ones(d)
    y_err = np.array([0.05, 0.1, 0.2])
    y = np.stack([np.zeros(3), 0.1 * np.ones(3)])
    dm = GU.device_model(model)
    try:
        dm.likelihood_setup(y[0], y_err, lo, hi, 1.0)
        s = DeviceSampler([dm], W, seed=3)
        s.set_state(rng.uniform(0.2, 0.8, (W, d)))
        s.run(40)
        chain, _ = s.get_chain()
        out = s.propose_design(3, n_candidates=70, n_reference=200, discard=4, seed=5)
        assert out["thin"] == 3 and out["n_reference_rows"] == 12 * W              # 36 steps x 16 walkers -> every third
        rows = chain[4::3].reshape(-1, d)
        cand = DS.default_candidates(lo, hi, rows, 70, seed=5)
        assert np.array_equal(out["candidates"], cand)
        with dm.design(rows, cand, max_picks=3) as ds:
            want = ds.select(3)
        for key in ("indices", "gain", "integrated_variance", "first_scores", "points"):
            assert np.array_equal(out[key], want[key]), key
        s.close()
        dm.likelihood_setup(y, y_err, lo, hi, 1.0)
        st = DeviceSampler([dm], W, seeds=[7, 8])
        st.set_state(rng.uniform(0.2, 0.8, (2 * W, d)))
        st.run(12)
        chain, _ = st.get_chain()
        with pytest.raises(ValueError):
            st.propose_design(2)
        out = st.propose_design(2, candidates=cand, thin=2, chain=1, feature_weights=1.0 / y_err ** 2)
        with dm.design(chain[::2, W:].reshape(-1, d), cand, max_picks=2, feature_weights=1.0 / y_err ** 2) as ds:
            want = ds.select(2)
        for key in ("indices", "gain", "integrated_variance", "first_scores"):
            assert np.array_equal(out[key], want[key]), key
        st.close()
    finally:
        dm.close()


# ---- 6. the unfused route ---------------------------------------------------------------------------------------------------
def test_fused_scores_equal_the_composition_of_predict_cov():
    model = synth("m25", True, 8, 150)
    Xref, Xcand = sets(model, 130, 70)
    dm = GU.device_model(model)
    try:
        with dm.design(Xref, Xcand) as ds:
            fused = ds.scores()
        _, Csc = dm.gp_predict_cov(Xref, Xcand)
        _, Ccc = dm.gp_predict_cov(Xcand, Xcand.copy())
        ref = DR.DesignRef(model, Xref, Xcand)
        pcw = DS.pc_weights(dm)
        unfused = np.zeros(70, dtype=LD)
        ub = np.zeros(70)
        for p, pc in enumerate(ref.pcs):
            num = np.sum((Csc[p].astype(LD) ** 2) / LD(130), axis=0)
            den = np.diag(Ccc[p]).astype(LD) + LD(pc.tau)
            unfused += LD(pcw[p]) * num / den
            # the composition's own error: the same elements' bounds (cov_ref) through the same quotient
            ub += pcw[p] * pc.terms()[1]
        _, bound, _, _ = ref.scores()
        assert np.all(np.abs(np.asarray(fused, dtype=LD) - unfused).astype(np.float64) <= bound + ub)
    finally:
        dm.close()


# ---- 7. the C ABI's checks come before any launch ------------------------------------------------------------------------------
def test_abi_argument_checks():
    import ctypes as C
    model = synth("rbf", True, 6, 50)
    dm = GU.device_model(model)
    try:
        L = _lib.lib()
        X, Xc, w, pcw = np.zeros((4, 6)), np.ones((5, 6)), np.ones(4), np.ones(2)
        h = C.c_void_p()
        p = _lib.ptr

        def create(S=4, Xr=X, wr=w, M=5, Xq=Xc, pw=pcw, tau=None, mv=1e-6, mp=4, ws=0):
            return L.gpemu_design_create(C.byref(h), dm.handle, S, p(Xr), p(wr), M, p(Xq), p(pw), p(tau), mv, mp, ws)
        before = DS.path_counts()
        bad = X.copy()
        bad[1, 2] = np.nan
        for kw in (dict(S=0), dict(M=0), dict(Xr=bad), dict(Xq=np.full((5, 6), np.inf)), dict(wr=np.array([1.0, -1, 1, 1])),
                   dict(wr=np.zeros(4)), dict(pw=np.array([1.0, np.nan])), dict(tau=np.array([-1.0, 0.0])), dict(mv=-1.0),
                   dict(mp=257), dict(mp=-1), dict(ws=-1), dict(ws=1024)):
            assert create(**kw) == -1 and not h.value, kw
        assert "bytes are needed" in _lib.last_error()
        assert create() == 0 and h.value
        s = np.empty(5)
        assert L.gpemu_design_scores(h, p(s), None) == 0 and np.all(np.isfinite(s))
        assert L.gpemu_design_scores(h, None, None) == -1
        assert L.gpemu_design_condition(h, 5) == -1 and L.gpemu_design_condition(h, -1) == -1
        assert L.gpemu_design_destroy(h) == 0 and L.gpemu_design_destroy(None) == 0
        assert DS.path_counts()["scores"] == before["scores"] + 1
    finally:
        dm.close()
