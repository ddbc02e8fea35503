"""CPU: the sequential-design reference (tests/design_ref.py) against brute-force refits, the PC weights against the
oracle's predict, the selection rules of ``gpemu.design.Design`` on stub handles, the argument checks that come before
any device call, the C ABI's declarations and the drop-in's merging and defaults."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import cov_ref as CR
import design_ref as DR
import golden_util as GU
from gpemu import design as DS
from oracle import gp_oracle as O

LD = np.longdouble


def small_model(d=3, N=40, k=2, seed=0):
    """RBF + const + noise 0.01 fitted at fixed theta on a random design in [0, 1]^d"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    spec = O.KernelSpec(kind=O.RBF, nu=math.inf, has_const=True, has_noise=True)
    gps = []
    for p in range(k):
        ls = 0.35 * math.sqrt(d) * (1.0 + 0.3 * p) * rng.uniform(0.8, 1.25, d)
        y = np.sin(X @ rng.normal(size=d) * 3.0) + 0.1 * p
        gps.append(O.gp_fit_at_theta(X, y, np.log(np.r_[ls, 0.7, 0.01]), spec, 1e-10))
    F = 4
    return O.GroupModel(X_train=X, spec=spec, gps=gps, components=rng.normal(size=(k, F)),
                        explained_variance=np.ones(k), scaler_mean=np.zeros(F), scaler_scale=rng.uniform(0.5, 2.0, F),
                        n_pc=k)


# ---- 1. the criterion and its recursion against refits -----------------------------------------------------------------
def test_score_is_the_drop_of_the_integrated_variance_after_a_refit_over_four_rounds():
    """d = 3, N = 40, S = 60, M = 25: at every round the score of EVERY candidate equals IV - IV(refit with the picks so
    far and the candidate appended, fixed theta), to 1e-10 of the largest score; non-uniform weights, a per-feature
    weight and the default tau (the White level)"""
    model = small_model()
    rng = np.random.default_rng(1)
    Xref, Xcand = rng.uniform(0, 1, (60, 3)), rng.uniform(-0.1, 1.1, (25, 3))
    w = rng.uniform(0.2, 1.0, 60)
    pcw = DR.pc_weights(model, rng.uniform(0.5, 2.0, 4))
    ref = DR.DesignRef(model, Xref, Xcand, weights=w, pcw=pcw)
    picks = []
    worst = 0.0
    for rnd in range(4):
        score = ref.scores()[0]
        iv, _ = ref.integrated_variance()
        base = DR.brute_force_iv(model, Xref, w, Xcand[picks], pcw=pcw)
        top = float(np.max(score))
        assert abs(float(iv - base)) <= 1e-10 * top, (rnd, float(iv), float(base))
        for c in range(25):
            drop = base - DR.brute_force_iv(model, Xref, w, Xcand[picks + [c]], pcw=pcw)
            dev = abs(float(drop - score[c]))
            worst = max(worst, dev / top)
            assert dev <= 1e-10 * top, (rnd, c, float(drop), float(score[c]))
        c = int(np.argmax(score))
        ref.condition(c)
        picks.append(c)
    print(f"largest deviation over all candidates and rounds: {worst:.3g} of the largest score")
    assert len(set(picks)) == 4


def test_a_wrong_tau_or_a_dropped_term_is_caught_at_that_tolerance():
    model = small_model()
    rng = np.random.default_rng(2)
    Xref, Xcand = rng.uniform(0, 1, (60, 3)), rng.uniform(0, 1, (25, 3))
    good = DR.DesignRef(model, Xref, Xcand).scores()[0]
    bad = DR.DesignRef(model, Xref, Xcand, tau=[0.0101, 0.01]).scores()[0]
    assert float(np.max(np.abs(good - bad))) > 1e-6 * float(np.max(good))


def test_reference_blocks_are_cov_refs():
    model = small_model(N=20)
    rng = np.random.default_rng(3)
    Xref, Xcand = rng.uniform(0, 1, (9, 3)), rng.uniform(0, 1, (5, 3))
    ref = DR.DesignRef(model, Xref, Xcand)
    for pc, gp in zip(ref.pcs, model.gps):
        sc = CR.PCCov(Xref, Xcand, model.X_train, gp, model.spec)
        cc = CR.PCCov(Xcand, Xcand.copy(), model.X_train, gp, model.spec)
        ss = CR.PCCov(Xref, Xref.copy(), model.X_train, gp, model.spec)
        assert np.array_equal(pc.Csc, sc.C) and np.allclose(pc.dSc, sc.bound, rtol=1e-12, atol=0)
        assert np.array_equal(pc.Ccc, cc.C) and np.allclose(pc.dCc, cc.bound, rtol=1e-12, atol=0)
        assert abs(float(pc.iv - np.mean(np.diag(ss.C)))) < 1e-17
        assert pc.div >= float(np.mean(np.diag(ss.bound)))


# ---- 2. the PC weights ---------------------------------------------------------------------------------------------------
def test_pc_weights_carry_the_pc_variances_to_the_oracles_predict():
    g = GU.load("g1_matern25_const_noise")
    model = GU.group_model(g)
    k, F = model.n_pc, model.components.shape[1]
    rng = np.random.default_rng(4)
    X = rng.uniform(model.X_train.min(axis=0), model.X_train.max(axis=0), (3, model.X_train.shape[1]))
    fw = rng.uniform(0.5, 2.0, F)
    trunc = O.cov_unexplained(model) * np.outer(model.scaler_scale, model.scaler_scale)
    _, var = O.gp_predict_all(X, model)
    for fwi in (None, fw):
        w = DS.pc_weights((model.components[:k], model.scaler_scale), fwi)
        assert w.shape == (k,) and np.allclose(w, DR.pc_weights(model, fwi), rtol=1e-13, atol=0)
        f = np.ones(F) if fwi is None else fwi
        for i in range(3):
            cov = O.predict_group(X[i:i + 1], model)["cov"][0]
            want = float(np.sum(f * (np.diag(cov) - np.diag(trunc))))
            assert abs(float(w @ var[i]) - want) <= 1e-10 * abs(want)
    with pytest.raises(ValueError):
        DS.pc_weights((model.components[:k], model.scaler_scale), np.ones(F + 1))
    with pytest.raises(ValueError):
        DS.pc_weights((model.components[:k], model.scaler_scale), -np.ones(F))


# ---- 3. selection rules on stub handles -----------------------------------------------------------------------------------
class Stub:
    """a group handle whose scores are a table per round"""

    def __init__(self, rounds, iv0=10.0):
        self.rounds, self.j, self.iv, self.picked, self.closed = [np.asarray(r, dtype=np.float64) for r in rounds], 0, iv0, [], 0

    def scores(self):
        return self.rounds[self.j].copy()

    def condition(self, i):
        self.iv -= self.rounds[self.j][i]
        self.picked.append(i)
        self.j += 1

    def integrated_variance(self):
        return self.iv

    def close(self):
        self.closed += 1


def test_select_ties_go_to_the_lowest_index_and_gains_are_the_scores_at_pick_time():
    a = Stub([[1.0, 3.0, 3.0, 0.5], [0.25, 0.0, 2.0, 2.0], [0.5, 0.0, 0.0, 0.5]])
    cand = np.arange(8.0).reshape(4, 2)
    with DS.Design.from_groups([a], cand) as ds:
        out = ds.select(3)
    assert out["indices"].tolist() == [1, 2, 0] and a.picked == [1, 2, 0]
    assert out["gain"].tolist() == [3.0, 2.0, 0.5]
    assert out["integrated_variance"].tolist() == [10.0, 7.0, 5.0, 4.5]
    assert np.array_equal(out["points"], cand[[1, 2, 0]]) and out["first_scores"].tolist() == [1.0, 3.0, 3.0, 0.5]
    assert a.closed == 1
    ds.close()
    assert a.closed == 1                      # idempotent


def test_select_adds_the_groups_in_order_and_conditions_all_of_them():
    a, b = Stub([[1.0, 2.0], [0.0, 1.0]]), Stub([[4.0, 1.0], [0.0, 0.5]], iv0=1.0)
    ds = DS.Design.from_groups([a, b], np.zeros((2, 1)))
    assert ds.scores().tolist() == [5.0, 3.0] and ds.scores_per_group().tolist() == [[1.0, 2.0], [4.0, 1.0]]
    out = ds.select(2)
    assert out["indices"].tolist() == [0, 1] and a.picked == b.picked == [0, 1]
    assert out["integrated_variance"].tolist() == [11.0, 6.0, 4.5]


def test_select_stops_when_every_candidate_is_under_the_floor():
    a = Stub([[0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [9.0, 9.0, 9.0]])
    ds = DS.Design.from_groups([a], np.zeros((3, 1)))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = ds.select(3)
    assert out["indices"].tolist() == [1] and out["gain"].tolist() == [2.0] and len(rec) == 1
    assert out["integrated_variance"].shape == (2,)
    nan = DS.Design.from_groups([Stub([[0.0, np.nan]])], np.zeros((2, 1)))
    with pytest.raises(ValueError):
        nan.select(1)
    with pytest.raises(IndexError):
        DS.Design.from_groups([Stub([[1.0]])], np.zeros((1, 1))).condition(1)


# ---- 4. argument errors come before any device call --------------------------------------------------------------------------
class NoDevice:
    """stands in for a DeviceModel; touching its handle is the device call that must not happen"""
    d, k, device = 3, 2, 0
    _projection = (np.ones((2, 4)), np.ones(4), np.zeros(4))

    @property
    def handle(self):
        raise AssertionError("a device call was made before the arguments were checked")


@pytest.mark.parametrize("kw", [
    dict(reference=np.zeros((0, 3))), dict(reference=np.zeros((4, 2))), dict(candidates=np.zeros((5, 4))),
    dict(reference=np.full((4, 3), np.nan)), dict(candidates=np.full((4, 3), np.inf)),
    dict(weights=[1.0, -1.0, 1.0, 1.0]), dict(weights=[0.0] * 4), dict(weights=[1.0, np.nan, 1.0, 1.0]),
    dict(weights=[1.0] * 3), dict(max_picks=-1), dict(max_picks=257), dict(min_variance=-1e-6),
    dict(min_variance=np.nan), dict(workspace_bytes=-1), dict(tau=[[0.1, -0.1]]), dict(tau=[[0.1]]),
    dict(feature_weights=[np.ones(3)]), dict(feature_weights=[-np.ones(4)]),
])
def test_argument_errors_are_raised_before_any_device_call(kw):
    args = dict(reference=np.zeros((4, 3)), candidates=np.ones((5, 3)))
    args.update(kw)
    with pytest.raises(ValueError):
        DS.Design([NoDevice()], **args)


def test_more_parameters_or_pcs_than_the_kernels_hold_are_refused():
    class Wide(NoDevice):
        d = 17

    class Deep(NoDevice):
        k = 65
    with pytest.raises(ValueError):
        DS.Design([Wide()], np.zeros((4, 17)), np.zeros((4, 17)))
    with pytest.raises(ValueError):
        DS.Design([Deep()], np.zeros((4, 3)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        DS.Design([], np.zeros((4, 3)), np.zeros((4, 3)))


# ---- 5. the C ABI's declarations -------------------------------------------------------------------------------------------
NEW = ("gpemu_design_create", "gpemu_design_create_dev", "gpemu_design_scores", "gpemu_design_condition",
       "gpemu_design_state", "gpemu_design_destroy", "gpemu_design_path_counts")


def test_new_symbols_are_declared_bound_and_exported():
    from gpemu import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(L, name), name
    enum = re.search(r"enum gpemu_design_path \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"GPEMU_DESIGN_PATH_([A-Z0-9_]+?)\b", enum)
    assert [n.lower() for n in names[:-1]] == list(DS.PATH_NAMES) and names[-1] == "COUNT"
    out = np.zeros(32, dtype=np.int64)
    import ctypes as C
    assert L.gpemu_design_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), 32) == len(DS.PATH_NAMES)
    src = open(os.path.join(root, "bayesian-inference_amd", "csrc", "Makefile")).read()
    assert "k_design.hip" in src


# ---- 6. the drop-in's merging and defaults -----------------------------------------------------------------------------------
def test_feature_weights_are_split_the_way_predict_merges():
    import dropin_util as DU
    from bayesian_inference import emulation
    from test_posterior_predictive_host import _FakeSorter          # two groups of different F, interleaved
    merged = np.arange(9.0) + 1.0
    split = emulation.gather_feature_rows(_FakeSorter(), merged, ["A", "B"])
    assert split["A"].tolist() == [1, 2, 3, 8, 9] and split["B"].tolist() == [4, 5, 6, 7]
    back = emulation.scatter_feature_rows(_FakeSorter(), {n: v[None, :] for n, v in split.items()})[0]
    assert np.array_equal(back, merged)
    assert emulation.gather_feature_rows(DU.TrivialSort("main"), merged, ["main"])["main"].tolist() == merged.tolist()
    with pytest.raises(ValueError):
        emulation.gather_feature_rows(_FakeSorter(), merged[:-1], ["A", "B"])


def test_design_sets_defaults():
    from bayesian_inference import emulation
    from gpemu.sensitivity import base_samples
    lo, hi = [0.0, -1.0], [1.0, 3.0]
    ref, cand = emulation.design_sets(lo, hi, n_reference=64, n_candidates=16, seed=3)
    assert np.array_equal(ref, base_samples(64, lo, hi, seed=3)[1])       # the box: plain integrated-variance design
    assert np.array_equal(cand, base_samples(16, lo, hi, seed=3)[0])
    assert not {tuple(r) for r in ref} & {tuple(c) for c in cand}
    chain = np.random.default_rng(0).uniform(lo, hi, (40, 2))
    ref2, cand2 = emulation.design_sets(lo, hi, reference=chain, n_candidates=16, seed=3)
    assert np.array_equal(ref2, chain) and cand2.shape == (16, 2)
    assert np.array_equal(cand2[:8], base_samples(8, lo, hi, seed=3)[0])
    rows = {tuple(r) for r in chain}
    assert all(tuple(c) in rows for c in cand2[8:]) and len({tuple(c) for c in cand2[8:]}) == 8
    assert np.array_equal(cand2, emulation.design_sets(lo, hi, reference=chain, n_candidates=16, seed=3)[1])
    few = emulation.design_sets(lo, hi, reference=chain[:3], n_candidates=16, seed=3)[1]
    assert few.shape == (16, 2) and np.array_equal(few[13:], chain[:3])
    mine = np.zeros((2, 2))
    assert np.array_equal(emulation.design_sets(lo, hi, reference=chain, candidates=mine)[1], mine)


def test_the_drop_in_hands_the_merged_sets_and_weights_to_design(monkeypatch):
    """both drop-in calls on stand-ins for the configuration, the stored chain and ``Design``: what reaches ``Design``"""
    from bayesian_inference import emulation, mcmc
    from test_posterior_predictive_host import _FakeSorter
    seen = {}

    class FakeDesign:
        def __init__(self, models, reference, candidates, feature_weights=None, **kw):
            seen.update(models=models, reference=reference, candidates=candidates, fw=feature_weights, kw=kw)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            seen["closed"] = True

        def select(self, q):
            return {"indices": np.arange(q), "points": seen["candidates"][:q], "gain": np.ones(q),
                    "integrated_variance": np.ones(q + 1), "first_scores": np.zeros(len(seen["candidates"]))}

    class GroupCfg:
        def __init__(self, n_pc):
            self.n_pc = n_pc

    class Cfg:
        analysis_config = {"parameterization": {"par": {"min": [0.0, 0.0], "max": [1.0, 2.0], "names": ["a", "b"]}}}
        parameterization, analysis_name, config_file = "par", "ana", "file"
        emulation_groups_config = {"A": GroupCfg(2), "B": GroupCfg(3)}
        sort_observables_in_matrix = _FakeSorter()

        def read_all_emulator_groups(self):
            return {"A": "resA", "B": "resB"}

    from gpemu import design as gd
    monkeypatch.setattr(gd, "Design", FakeDesign)
    monkeypatch.setattr(emulation, "device_model_for", lambda res, n_pc, cov=None: (res, n_pc))
    out = emulation.propose_design_points(Cfg(), 3, n_reference=32, n_candidates=8, seed=1,
                                          feature_weights=np.arange(9.0), emulation_group_results=Cfg().read_all_emulator_groups())
    assert seen["models"] == [("resA", 2), ("resB", 3)] and seen["closed"]
    assert seen["reference"].shape == (32, 2) and seen["candidates"].shape == (8, 2) and seen["kw"] == {"max_picks": 3}
    assert [f.tolist() for f in seen["fw"]] == [[0, 1, 2, 7, 8], [3, 4, 5, 6]]
    assert out["parameter_names"] == ["a", "b"] and out["indices"].tolist() == [0, 1, 2]
    assert np.array_equal(out["candidates"], seen["candidates"])
    for key in ("points", "indices", "gain", "integrated_variance", "first_scores", "candidates", "parameter_names"):
        assert key in out
    emulation.propose_design_points(Cfg(), 2, emulation_group_results=Cfg().read_all_emulator_groups())
    assert seen["fw"] is None and seen["reference"].shape == (4096, 2) and seen["candidates"].shape == (2048, 2)

    # mcmc: the stored chain is the reference set, thinned to at most n_reference rows; 1 / y_err^2 by default
    chain = np.random.default_rng(0).uniform(0, 1, (50, 4, 2))
    y_err = np.array([0.5, 2.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 4.0])
    monkeypatch.setattr(mcmc, "_stored_chain", lambda config, ci, discard, thin: (config, chain[discard::thin]))
    monkeypatch.setattr(emulation.EmulationConfig, "from_config_file", classmethod(lambda cls, **kw: Cfg()))

    class IO:
        @staticmethod
        def data_array_from_h5(*a, **k):
            return {"y": np.zeros(9), "y_err": y_err}
    monkeypatch.setattr(mcmc, "_data_IO", lambda: IO)
    Cfg.output_dir = "out"
    Cfg.observable_filter = None
    mcmc.propose_design_points(Cfg(), discard=10, n_points=2, n_reference=64, n_candidates=8)
    assert np.array_equal(seen["reference"], chain[10::3].reshape(-1, 2))       # 160 rows -> every third step: 56
    assert [f.tolist() for f in seen["fw"]] == [[4.0, 0.25, 0.0, 1.0, 1 / 16], [1.0, 1.0, 1.0, 1.0]]
    mcmc.propose_design_points(Cfg(), discard=10, thin=5, n_points=2, n_candidates=8, feature_weights=np.ones(9))
    assert np.array_equal(seen["reference"], chain[10::5].reshape(-1, 2)) and seen["fw"][1].tolist() == [1.0] * 4
    assert mcmc.design_feature_weights([2.0, 0.0, np.inf, np.nan]).tolist() == [0.25, 0.0, 0.0, 0.0]
