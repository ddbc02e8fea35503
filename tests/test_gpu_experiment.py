"""Device checks of gpemu.experiment: the pairwise log-sum-exp kernel against the longdouble reference
within the error bound derived from its own operations (experiment_ref.pairlse_bound), the excluded pair, determinism,
argument errors, and the estimators built on it -- the module function, the model's and the sampler's."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import experiment_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 2), (64, 128, 4), (65, 129, 5), (63, R.CHUNK - 1, 7), (130, R.CHUNK + 1, 33),
          (17, 2 * R.CHUNK + 3, 130), (257, 300, 64)]


def _others():
    """the counters of the families a pairwise log-sum-exp has no business with"""
    from gpemu import diagnostics, information, marginals as M, model as gmodel, sensitivity
    return (M.path_counts(), M.kde2d_path_counts(), diagnostics.path_counts(),
            information.path_counts(), gmodel.postpred_path_counts().tolist(), gmodel.hmc_path_counts().tolist(),
            gmodel.grad_path_counts().tolist(), sensitivity.sobol_path_counts().tolist())


def _rows(n, S, F, seed):
    """Rows 1e3 sigma away from the origin in every coordinate (centring matters), coordinate 0 at scale 1e-3 and the last
    at scale 30 (for F > 1; its differences of some 40 make most pairs of a row underflow against the nearest), every
    seventh row of Y an exact copy of a row of Z, and a tenth of the rows of Z another 100 sigma away (underflow to 0
    against every row of Y)."""
    rng = np.random.default_rng(seed)
    scale = np.ones(F)
    scale[0] = 1e-3
    if F > 1:
        scale[-1] = 30.0
    offset = 1e3 * scale
    Z = offset + scale * rng.standard_normal((S, F))
    Y = offset + scale * rng.standard_normal((n, F))
    Z[::10] += 100.0 * scale
    Y[::7] = Z[(3 * np.arange(0, n, 7) + 1) % S]
    return np.ascontiguousarray(Y), np.ascontiguousarray(Z)


@functools.lru_cache(maxsize=None)
def _case(n, S, F):
    """the rows, the reference and the bound of one shape: computed once, shared, never written to"""
    Y, Z = _rows(n, S, F, seed=n + S + F)
    ref = R.pairlse_ref(Y, Z)
    b_lse, b_ess = R.pairlse_bound(Y, Z, Z.mean(axis=0))
    for a in (Y, Z, b_lse, b_ess, *ref.values()):
        a.setflags(write=False)
    return Y, Z, ref, b_lse, b_ess


def _within(lse, ess, ref, b_lse, b_ess, what):
    dead = np.isneginf(ref["lse"].astype(np.float64))
    assert np.array_equal(np.isneginf(lse), dead) and np.all(ess[dead] == 0.0), what
    assert np.all(np.isfinite(lse[~dead])) and np.all(np.isfinite(ess)), what
    e_lse = np.abs((lse[~dead] - ref["lse"][~dead]).astype(np.float64))
    e_ess = np.abs((ess[~dead] / ref["ess"][~dead] - 1).astype(np.float64))
    print(f"{what}: lse error max {e_lse.max(initial=0):.3e} (bound {b_lse[~dead].max(initial=0):.3e}, largest share "
          f"{np.max(e_lse / b_lse[~dead], initial=0):.3f}); ess relative error max {e_ess.max(initial=0):.3e} (bound "
          f"{b_ess[~dead].max(initial=0):.3e}, largest share {np.max(e_ess / b_ess[~dead], initial=0):.3f})")
    assert np.all(e_lse <= b_lse[~dead]), what
    assert np.all(e_ess <= b_ess[~dead]), what


def test_constants_are_the_references():
    from gpemu import experiment as E
    assert (E.CHUNK, E.TILE_ROWS) == (R.CHUNK, R.TILE_ROWS)


@pytest.mark.parametrize("n,S,F", SHAPES)
def test_pair_lse_within_the_bound_of_its_operations(n, S, F):
    """lse absolutely and ess relatively against the longdouble reference (direct differences), each row within
    ``experiment_ref.pairlse_bound`` -- the roundings of the centring, the norms, the MFMA chain of 4 ceil(F / 4) terms,
    the epilogue, exp at 1 ulp, the positive sums and the rescale and merge stages, plus 10 %; see its docstring.  No
    tolerance is chosen: the bound is a function of the rows.  The shapes: one pair; less than a tile; exactly one tile
    of rows and columns; one more than a tile in n, S and a k-step in F; one column short of a chunk; one column more
    than a chunk with three k-tiles (F = 33) and three row blocks; three chunks with a ragged last one and 9 k-tiles;
    five row blocks."""
    from gpemu import experiment as E
    Y, Z, ref, b_lse, b_ess = _case(n, S, F)
    before = E.path_counts()
    lse, ess = E.pair_lse(Y, Z)
    after = E.path_counts()
    assert after["PARTIAL"] == before["PARTIAL"] + 1 and after["MERGE"] == before["MERGE"] + 1
    assert after["CENTRE"] == before["CENTRE"] + 2 and after["ROW_BATCH"] == before["ROW_BATCH"] + 1
    _within(lse, ess, ref, b_lse, b_ess, f"(n, S, F) = ({n}, {S}, {F})")
    # the copies: every seventh row has a column at distance exactly 0
    assert np.all(ref["m"][::7] == 0)


def test_self_index_leaves_out_exactly_the_named_pair():
    """Rows that are exact copies of a column, with that column left out: against the reference with the pair excluded
    (which the host tests hold to deleting the column) within the bound, and three rows against the reference on Z with
    the column deleted.  The named columns lie in the first tile, at a chunk's end and in the last, ragged chunk."""
    from gpemu import experiment as E
    n, S, F = 70, R.CHUNK + 5, 5
    Y, Z = _rows(n, S, F, seed=5)
    self_index = np.full(n, -1, dtype=np.int64)
    self_index[::3] = np.array([0, 127, R.CHUNK - 1, R.CHUNK, S - 1, S - 3])[np.arange(len(self_index[::3])) % 6]
    named = np.nonzero(self_index >= 0)[0]
    Y[named] = Z[self_index[named]]
    ref = R.pairlse_ref(Y, Z, self_index)
    b_lse, b_ess = R.pairlse_bound(Y, Z, Z.mean(axis=0), self_index)
    lse, ess = E.pair_lse(Y, Z, self_index=self_index)
    _within(lse, ess, ref, b_lse, b_ess, "self_index")
    assert np.all(ref["m"][named] < 0)                 # the copy is gone: the maximum is no longer 0
    for i in named[[0, 2, 4]]:
        one = R.pairlse_ref(Y[i:i + 1], np.delete(Z, self_index[i], axis=0))
        assert abs(float(lse[i] - one["lse"][0])) <= b_lse[i] and abs(float(ess[i] / one["ess"][0] - 1)) <= b_ess[i]
    # without the index the copies count
    lse0, _ = E.pair_lse(Y, Z)
    assert np.all(lse0[named] > lse[named]) and np.array_equal(np.delete(lse0, named), np.delete(lse, named))


def test_all_excluded_row_is_minus_infinity_without_nan():
    from gpemu import experiment as E
    Y, Z = np.array([[1.0, 2.0], [0.5, 0.5], [3.0, -1.0]]), np.array([[0.25, 0.75]])
    lse, ess = E.pair_lse(Y, Z, self_index=np.array([0, -1, 0]))
    assert np.isneginf(lse[0]) and np.isneginf(lse[2]) and ess[0] == 0.0 and ess[2] == 0.0
    assert lse[1] == pytest.approx(-0.5 * (0.25 ** 2 + 0.25 ** 2), abs=1e-15) and ess[1] == 1.0
    assert not np.isnan(lse).any() and not np.isnan(ess).any()


def test_bits_do_not_depend_on_the_run_the_batching_the_entry_or_a_passed_centre():
    import torch
    from gpemu import experiment as E
    n, S, F = 257, 300, 64
    Y, Z, _, _, _ = _case(n, S, F)
    first = E.pair_lse(Y, Z)
    again = E.pair_lse(Y, Z)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    per = E.block_bytes(S, F)
    for blocks, batches in ((5, 1), (3, 2), (1, 5)):
        before = E.path_counts()
        out = E.pair_lse(Y, Z, workspace_bytes=blocks * per + per // 2)
        after = E.path_counts()
        assert after["ROW_BATCH"] - before["ROW_BATCH"] == batches == after["PARTIAL"] - before["PARTIAL"]
        assert after["CENTRE"] - before["CENTRE"] == batches + 1
        assert out[0].tobytes() == first[0].tobytes() and out[1].tobytes() == first[1].tobytes()
    with pytest.raises(Exception, match="out of memory"):
        E.pair_lse(Y, Z, workspace_bytes=per - 1)
    # the device entry in place, on rows inside wider tensors
    dev = torch.device("cuda", 0)
    Yw = torch.full((n, F + 3), float("nan"), dtype=torch.float64, device=dev)
    Zw = torch.full((S, F + 5), float("nan"), dtype=torch.float64, device=dev)
    Yw[:, :F], Zw[:, 2:2 + F] = torch.tensor(Y, device=dev), torch.tensor(Z, device=dev)
    dY, dZ = Yw[:, :F], Zw[:, 2:2 + F]
    assert dY.stride(0) == F + 3 and dZ.stride(0) == F + 5 and dZ.data_ptr() != Zw.data_ptr()
    dl, de = E.pair_lse(dY, dZ)
    assert dl.is_cuda and dl.cpu().numpy().tobytes() == first[0].tobytes() and de.cpu().numpy().tobytes() == first[1].tobytes()
    # the centre the library computes, passed back
    centre = E.centre_dev(dZ)
    assert np.allclose(centre.cpu().numpy(), Z.mean(axis=0), rtol=1e-13, atol=0)
    dl2, de2 = E.pair_lse(dY, dZ, centre=centre)
    assert torch.equal(dl2, dl) and torch.equal(de2, de)
    hl, he = E.pair_lse(Y, Z, centre=centre.cpu().numpy())
    assert hl.tobytes() == first[0].tobytes() and he.tobytes() == first[1].tobytes()


def test_invalid_arguments_return_before_any_launch():
    import torch
    from gpemu import _lib, experiment as E
    L = _lib.lib()
    Y, Z = np.zeros((4, 3)), np.zeros((5, 3))
    lse, ess = np.zeros(4), np.zeros(4)
    E.pair_lse(Y, Z)                                   # the device is initialised before the counters are read
    before, others = E.path_counts(), _others()
    p = _lib.ptr

    def host(n=4, S=5, F=3, self_index=None, ws=0, y=Y, out=lse):
        return L.gpemu_pair_lse(0, n, S, F, p(y), p(Z), p(self_index), None, ws, p(out), p(ess))

    assert host() == 0
    mid = E.path_counts()
    assert mid != before
    for kw in (dict(n=0), dict(S=0), dict(F=0), dict(n=-1), dict(n=2 ** 31), dict(S=2 ** 31), dict(ws=-1),
               dict(self_index=np.array([0, 5, -1, -1], dtype=np.int64)),
               dict(self_index=np.array([0, -2, -1, -1], dtype=np.int64)), dict(y=None), dict(out=None)):
        assert host(**kw) == -1, kw
        assert "bad argument" in _lib.last_error()
    dev = torch.device("cuda", 0)
    dY, dZ = torch.zeros((4, 3), dtype=torch.float64, device=dev), torch.zeros((5, 3), dtype=torch.float64, device=dev)
    dl = torch.zeros(4, dtype=torch.float64, device=dev)
    bad_self = torch.tensor([0, 1, 5, -1], dtype=torch.int64, device=dev)

    def device(ldy=3, ldz=3, dself=None):
        return L.gpemu_pair_lse_dev(0, 4, 5, 3, C.c_void_p(dY.data_ptr()), ldy, C.c_void_p(dZ.data_ptr()), ldz,
                                    None if dself is None else C.c_void_p(dself.data_ptr()), None, 0,
                                    C.c_void_p(dl.data_ptr()), None, _lib.current_stream(dev))

    assert device(ldy=2) == -1 and device(ldz=2) == -1 and device(dself=bad_self) == -1
    assert L.gpemu_pairlse_centre_dev(0, 5, 3, C.c_void_p(dZ.data_ptr()), 2, C.c_void_p(dl.data_ptr()), None) == -1
    assert E.path_counts() == mid and _others() == others
    assert device() == 0                               # ess may be null
    with pytest.raises(IndexError):
        E.pair_lse(Y, Z, self_index=[0, 1, 2, 5])
    with pytest.raises(ValueError):
        E.pair_lse(Y, np.zeros((5, 2)))
    assert E.path_counts()["PARTIAL"] == mid["PARTIAL"] + 1


def test_expected_information_gain_is_the_reference_estimator_on_the_same_noise():
    """The linear-Gaussian case (d, F, S, n) = (6, 8, 4096, 1024).  Term i is -|eps_i|^2 / 2 - lse_i + log S: the first
    and the last are formed on the host from the same numbers in both, in double here and in longdouble there (F + 2
    roundings of |eps|^2 / 2 and two of the sum: (F + 4) u max(|eps_i|^2 / 2, |term_i|, |lse_i|) each), and lse_i is
    within the kernel's bound b_i.  The mean of n terms adds one relative rounding per addition, n u |mean| at most.
    So |eig - ref| <= mean_i(b_i) + (F + 4) u mean_i(|eps_i|^2 / 2 + |lse_i| + |term_i|) + n u mean_i |term_i|, and every
    term is within its own share."""
    from gpemu import experiment as E
    d, F, S, n = 6, 8, 4096, 1024
    means, exact = R.linear_gaussian_case(d, F, S, seed=0)
    ref = R.eig_ref(means, y_err=1.0, n_outer=n, seed=0)
    out = E.expected_information_gain(means, y_err=np.ones(F), n_outer=n, seed=0)

    def bounds(ref):
        b_lse, _ = R.pairlse_bound(ref["Y"], ref["Z"], ref["Z"].mean(axis=0), ref["self_index"])
        half = 0.5 * (ref["eps"] ** 2).sum(axis=1)
        b_terms = b_lse + (F + 4) * R.U * (half + np.abs(ref["lse"].astype(np.float64)) + np.abs(ref["terms"]))
        return b_terms, b_terms.mean() + n * R.U * np.abs(ref["terms"]).mean()

    b_terms, bound = bounds(ref)
    e_terms = np.abs(out["terms"] - ref["terms"])
    print(f"eig {out['eig_nats']:.6f} (reference {ref['eig_nats']:.6f}, closed form {exact:.6f}, se {out['se']:.4f}); "
          f"error {abs(out['eig_nats'] - ref['eig_nats']):.3e}, bound {bound:.3e}; terms' largest share "
          f"{np.max(e_terms / b_terms):.3f}")
    assert np.all(e_terms <= b_terms)
    assert abs(out["eig_nats"] - ref["eig_nats"]) <= bound
    assert out["se"] == pytest.approx(ref["se"], rel=1e-9) and out["ess_mean"] == pytest.approx(ref["ess_mean"], rel=1e-9)
    assert (out["n_outer"], out["n_inner"], out["saturated"]) == (n, S, False)
    assert out["eig_bits"] == out["eig_nats"] / math.log(2.0) and out["log_n_inner"] == math.log(S)
    assert abs(out["eig_nats"] - exact) <= 4 * out["se"]
    # the outer rows left out of their own inner sums
    ref_x = R.eig_ref(means, y_err=1.0, n_outer=n, seed=0, exclude_self=True)
    out_x = E.expected_information_gain(means, y_err=1.0, n_outer=n, seed=0, exclude_self=True)
    assert out_x["n_inner"] == S - 1 and abs(out_x["eig_nats"] - ref_x["eig_nats"]) <= bounds(ref_x)[1]
    assert out_x["eig_nats"] > out["eig_nats"]
    # a dense covariance: the same candidate written as cov
    out_c = E.expected_information_gain(means, cov=np.eye(F), n_outer=n, seed=0)
    assert out_c["eig_nats"] == out["eig_nats"]


def test_rank_measurements_orders_candidates_on_common_noise():
    from gpemu import experiment as E
    means, _ = R.linear_gaussian_case(6, 8, 2048, seed=1)      # closed forms: some 1.0, 2.2, 0.35 and 2.0 nats
    cands = [dict(features=[0, 1, 2], y_err=1.0, label="three"), dict(features=[0, 1, 2], y_err=0.5, label="three, halved"),
             dict(features=[0], y_err=1.0), dict(features=list(range(8)), cov=np.eye(8), label="all")]
    out = E.rank_measurements(means, cands, n_outer=256, seed=3)
    assert out["labels"] == ["three", "three, halved", "candidate 2", "all"]
    assert [r["label"] for r in out["table"]] == [out["labels"][i] for i in out["order"]]
    assert np.all(np.diff(out["eig_nats"][out["order"]]) <= 0)
    assert out["eig_nats"][1] > out["eig_nats"][0] > out["eig_nats"][2] and out["eig_nats"][3] > out["eig_nats"][0]
    noise = np.random.default_rng(3).standard_normal((256, 8))
    for c, cand in enumerate(cands):
        f = cand["features"]
        one = E.expected_information_gain(means[:, f], y_err=cand.get("y_err"), cov=cand.get("cov"), n_outer=256,
                                          noise=noise[:, :len(f)])
        assert one["eig_nats"] == out["eig_nats"][c]
    assert np.array_equal(E.rank_measurements(means, cands, n_outer=256, seed=3)["eig_nats"], out["eig_nats"])


@functools.lru_cache(maxsize=None)
def _small_model():
    """gpemu.synthetic's problem at N = 40 design points, F = 12 features, 3 PCs (its d = 6 parameters), on the device"""
    import golden_util as GU
    model, prob, _ = GU.fixed_theta_model(40, 12, 3, seed=2)
    dm = GU.device_model(model)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
    return dm, prob


def test_model_method_is_the_module_function_on_predict_full():
    """Both emulator_cov modes against the module function fed with predict_full's outputs: the central values of the
    candidate's features, and for 'mean' the candidate's covariance plus the average of the emulator's (truncation
    term included: n_div = 1).  The same operations on the same numbers: the same bits."""
    from gpemu import experiment as E, synthetic
    dm, prob = _small_model()
    X = synthetic.make_walkers(600, seed=4, lo=prob["lo"], hi=prob["hi"])
    feats = [7, 2, 3, 11]
    y_err = 0.5 * prob["y_err"][feats]
    cv, cov = dm.predict_full(X, n_div=1.0)
    emu = (cov.sum(axis=0) / X.shape[0])[np.ix_(feats, feats)]
    assert np.all(np.diagonal(emu) > 0)
    none = dm.expected_information_gain(X, feats, y_err=y_err, emulator_cov="none", n_outer=200, seed=5)
    want = E.expected_information_gain(cv[:, feats], y_err=y_err, n_outer=200, seed=5)
    assert none["eig_nats"] == want["eig_nats"] and none["terms"].tobytes() == want["terms"].tobytes()
    mean = dm.expected_information_gain(X, feats, y_err=y_err, n_outer=200, seed=5)
    want = E.expected_information_gain(cv[:, feats], cov=np.diag(y_err) @ np.diag(y_err).T + emu, n_outer=200, seed=5)
    assert mean["eig_nats"] == want["eig_nats"] and mean["terms"].tobytes() == want["terms"].tobytes()
    assert mean["eig_nats"] < none["eig_nats"]          # the emulator's uncertainty blurs the measurement
    assert (mean["n_outer"], mean["n_inner"]) == (200, 600)
    # a dense covariance of the measurement, and batches of the rows: the means are the same rows
    dense = np.diag(y_err ** 2) + 0.25 * np.outer(y_err, y_err)
    a = dm.expected_information_gain(X, feats, cov=dense, emulator_cov="none", n_outer=200, seed=5)
    b = dm.expected_information_gain(X, feats, cov=dense, emulator_cov="none", n_outer=200, seed=5, batch=256)
    assert a["eig_nats"] == b["eig_nats"] == E.expected_information_gain(cv[:, feats], cov=dense, n_outer=200,
                                                                        seed=5)["eig_nats"]
    with pytest.raises(ValueError, match="emulator_cov"):
        dm.expected_information_gain(X, feats, y_err=y_err, emulator_cov="rows")
    with pytest.raises(IndexError):
        dm.expected_information_gain(X, [12], y_err=1.0)


def test_sampler_method_is_the_module_function_on_the_downloaded_chain():
    """32 walkers, 64 steps: the candidates ranked on the chain where it lies equal, bit for bit, the module function on
    get_chain() -- the same selected rows, predict_full on them, the emulators' mean covariance added."""
    from gpemu import experiment as E, information as I, synthetic
    from gpemu.sampler import DeviceSampler
    dm, prob = _small_model()
    s = DeviceSampler([dm], 32, seed=9)
    s.set_state(synthetic.make_walkers(32, seed=6, lo=prob["lo"], hi=prob["hi"]))
    s.run(64)
    cands = [dict(features=[0, 1, 2, 3], y_err=prob["y_err"][:4], label="first four"),
             dict(features=[8, 9], y_err=0.5 * prob["y_err"][8:10]), dict(features=list(range(12)), y_err=prob["y_err"])]
    for discard, thin, n_inner in ((0, 1, 16384), (10, 3, 300)):
        got = s.expected_information_gain(cands, discard=discard, thin=thin, n_inner=n_inner, n_outer=128, seed=2)
        rows = s.get_chain()[0][discard::thin].reshape(-1, dm.d)
        X = np.ascontiguousarray(rows[I.selected_rows(rows.shape[0], n_inner)])
        cv, cov = dm.predict_full(X, n_div=1.0)
        emu = cov.sum(axis=0) / X.shape[0]
        full = [dict(features=c["features"], label=c.get("label", f"candidate {i}"),
                     cov=np.diag(np.asarray(c["y_err"])) @ np.diag(np.asarray(c["y_err"])).T
                     + emu[np.ix_(c["features"], c["features"])]) for i, c in enumerate(cands)]
        want = E.rank_measurements(cv, full, n_outer=128, seed=2)
        assert got["labels"] == want["labels"] == ["first four", "candidate 1", "candidate 2"]
        assert got["eig_nats"].tobytes() == want["eig_nats"].tobytes() and got["se"].tobytes() == want["se"].tobytes()
        assert np.array_equal(got["order"], want["order"]) and got["results"][0]["n_inner"] == X.shape[0]
        assert got["eig_nats"][2] >= got["eig_nats"][0]      # all twelve features hold the first four
    s.close()
