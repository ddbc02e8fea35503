"""Host-side checks of the expected information gain (gpemu/experiment.py): the longdouble reference
estimator against the linear-Gaussian closed form, saturation, the excluded pair, argument and settings validation, the
common random numbers of a ranking and the exported symbols.  No device is needed."""
import math
import os
import re

import numpy as np
import pytest

import experiment_ref as R


@pytest.mark.parametrize("d,F,S,n", [(2, 3, 4096, 1024), (6, 8, 4096, 1024)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_estimator_reproduces_the_linear_gaussian_closed_form(d, F, S, n, seed):
    """theta ~ N(0, I_d), m = A theta with A ~ N(0, 1 / d), unit noise: log det(I + A A^T) / 2 within 4 se (a numpy trial
    landed within 2 se in all six cases).  A bound on the estimator at these seeds, not on the kernel."""
    from gpemu import experiment as E
    means, exact = R.linear_gaussian_case(d, F, S, seed)
    ref = R.eig_ref(means, y_err=1.0, n_outer=n, seed=seed)
    print(f"d = {d}, F = {F}, seed {seed}: estimate {ref['eig_nats']:.4f}, closed form {exact:.4f}, se {ref['se']:.4f}, "
          f"mean ess {ref['ess_mean']:.0f}")
    assert abs(ref["eig_nats"] - exact) <= 4.0 * ref["se"]
    # the module's host side turns the same inner sums into the same result
    out = E.estimate(ref["lse"].astype(np.float64), ref["ess"].astype(np.float64), ref["eps"], S)
    assert out["eig_nats"] == pytest.approx(ref["eig_nats"], abs=1e-12) and out["se"] == pytest.approx(ref["se"], rel=1e-10)
    assert not out["saturated"] and out["n_outer"] == n and out["n_inner"] == S
    assert np.array_equal(ref["Y"], E.whiten(means, E.whitening_factor(F, y_err=1.0))[E.selected_rows(S, n)]
                          + E.outer_noise(n, F, seed))


def test_saturated_fires_for_a_candidate_beyond_log_n_inner():
    """A candidate whose closed form (some 24 nats) exceeds log S = 8.3: the estimate sits at its cap, every outer row is
    carried by itself alone, and the result says so.  A modest candidate at the same sizes does not."""
    from gpemu import experiment as E
    S, n = 4096, 256
    means, exact = R.linear_gaussian_case(6, 8, S, 0, scale=60.0)
    assert exact > math.log(S)
    ref = R.eig_ref(means, y_err=1.0, n_outer=n, seed=0)
    out = E.estimate(ref["lse"].astype(np.float64), ref["ess"].astype(np.float64), ref["eps"], S)
    assert out["saturated"] and out["eig_nats"] <= out["log_n_inner"] + 1e-9 and out["ess_mean"] < E.MIN_ESS
    assert out["eig_nats"] > out["log_n_inner"] - E.SATURATION_MARGIN
    means, _ = R.linear_gaussian_case(6, 8, S, 0)
    ref = R.eig_ref(means, y_err=1.0, n_outer=n, seed=0)
    assert not E.estimate(ref["lse"].astype(np.float64), ref["ess"].astype(np.float64), ref["eps"], S)["saturated"]
    # either condition alone is enough
    lse, eps = np.full(4, math.log(10 ** 6) - 1.0), np.zeros((4, 1))            # 1 nat
    assert E.estimate(lse, np.full(4, 15.0), eps, 10 ** 6)["saturated"]
    assert not E.estimate(lse, np.full(4, 17.0), eps, 10 ** 6)["saturated"]
    assert E.estimate(lse - 11.0, np.full(4, 17.0), eps, 10 ** 6)["saturated"]      # 12 nats > log(10^6) - 3 = 10.8


def test_reference_exclude_self_equals_deleting_the_column():
    from gpemu import experiment as E
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((40, 3))
    Y = Z[::4] + 0.5 * rng.standard_normal((10, 3))
    Y[3] = Z[12]
    self_index = np.arange(0, 40, 4)
    self_index[5] = -1
    ref = R.pairlse_ref(Y, Z, self_index)
    for i in range(10):
        Zi = Z if self_index[i] < 0 else np.delete(Z, self_index[i], axis=0)
        one = R.pairlse_ref(Y[i:i + 1], Zi)
        for key in ("m", "s1", "s2", "lse", "ess"):
            assert float(abs(ref[key][i] - one[key][0])) <= 1e-17 * max(1.0, float(abs(one[key][0]))), (i, key)
    plain = R.pairlse_ref(Y, Z)
    assert plain["lse"][3] > ref["lse"][3] and plain["lse"][5] == ref["lse"][5]
    # every pair left out
    dead = R.pairlse_ref(Y[:2], Z[:1], np.array([0, -1]))
    assert np.isneginf(dead["lse"][0]) and dead["ess"][0] == 0 and np.isfinite(dead["lse"][1]) and dead["ess"][1] == 1
    # the estimator's exclude_self path: S' = S - 1 and the outer rows' own columns
    means = rng.standard_normal((64, 2))
    ex = R.eig_ref(means, y_err=1.0, n_outer=16, seed=1, exclude_self=True)
    assert np.array_equal(ex["self_index"], R.selected_rows(64, 16)) and ex["log_n_inner"] == math.log(63)
    assert np.array_equal(ex["self_index"], E.selected_rows(64, 16))
    assert np.array_equal(ex["self_index"], E.check_self_index(ex["self_index"], 16, 64))


def test_bound_is_zero_for_dead_rows_and_small_otherwise():
    from gpemu import experiment as E
    assert (R.CHUNK, R.TILE_ROWS) == (E.CHUNK, E.TILE_ROWS)         # the bound counts the kernel's chunks and tiles
    rng = np.random.default_rng(0)
    Z = 1e3 + rng.standard_normal((50, 6))
    Y = 1e3 + rng.standard_normal((5, 6))
    b_lse, b_ess = R.pairlse_bound(Y, Z, Z.mean(axis=0))
    assert np.all((b_lse > 0) & (b_lse < 1e-12)) and np.all((b_ess > 0) & (b_ess < 1e-12))
    b_lse, b_ess = R.pairlse_bound(Y[:1], Z[:1], Z[0], np.array([0]))
    assert b_lse[0] == 0 and b_ess[0] == 0


def test_argument_validation():
    from gpemu import experiment as E
    m = np.random.default_rng(0).standard_normal((32, 3))
    with pytest.raises(ValueError, match="exactly one"):
        E.whitening_factor(3)
    with pytest.raises(ValueError, match="exactly one"):
        E.whitening_factor(3, cov=np.eye(3), y_err=1.0)
    with pytest.raises(ValueError, match="y_err"):
        E.whitening_factor(3, y_err=[1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="symmetric"):
        E.whitening_factor(3, cov=np.eye(2))
    with pytest.raises(ValueError, match="symmetric"):
        E.whitening_factor(2, cov=np.array([[1.0, 0.5], [0.0, 1.0]]))
    with pytest.raises(ValueError, match="positive definite"):
        E.whitening_factor(2, cov=np.array([[1.0, 2.0], [2.0, 1.0]]))
    L = E.whitening_factor(2, cov=np.array([[4.0, 1.0], [1.0, 2.0]]))
    assert np.allclose(L @ L.T, [[4.0, 1.0], [1.0, 2.0]]) and L[0, 1] == 0
    assert np.allclose(E.whiten(m[:, :2], L) @ L.T, m[:, :2])
    assert np.array_equal(E.whiten(m, E.whitening_factor(3, y_err=[1.0, 2.0, 4.0])), m / [1.0, 2.0, 4.0])
    for bad in (0, -1, 1.5, 2 ** 31):
        with pytest.raises(ValueError, match="n_outer"):
            E.check_n_outer(bad)
    with pytest.raises(ValueError, match="noise"):
        E.outer_noise(4, 3, noise=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="noise"):
        E.outer_noise(4, 3, noise=np.zeros((5, 3)))
    with pytest.raises(IndexError):
        E.check_self_index([0, 3], 2, 3)
    with pytest.raises(IndexError):
        E.check_self_index([0, -2], 2, 3)
    with pytest.raises(ValueError):
        E.check_self_index([0.0, 1.0], 2, 3)
    with pytest.raises(ValueError):
        E.check_self_index([0], 2, 3)
    assert E.check_self_index(None, 2, 3) is None and E.check_self_index([-1, 2], 2, 3).dtype == np.int64
    with pytest.raises(ValueError):
        E.check_shapes(0, 1, 1)
    with pytest.raises(ValueError):
        E.check_shapes(1, 2 ** 31, 1)
    with pytest.raises(ValueError, match="finite"):
        E.expected_information_gain(np.full((4, 2), np.nan), y_err=1.0)
    with pytest.raises(ValueError, match="exclude_self"):
        E.expected_information_gain(np.zeros((1, 2)), y_err=1.0, exclude_self=True)
    with pytest.raises(ValueError):
        E.pair_lse(np.zeros((2, 3)), np.zeros((2, 2)))
    for cands, err in (([], ValueError), ([dict(y_err=1.0)], ValueError), ([dict(features=[0, 3], y_err=1.0)], IndexError),
                       ([dict(features=[0, 0], y_err=1.0)], ValueError), ([dict(features=[0])], ValueError),
                       ([dict(features=[0], y_err=1.0, cov=[[1.0]])], ValueError),
                       ([dict(features=[0], y_err=1.0, sigma=2.0)], ValueError), ([dict(features=[0.5], y_err=1.0)], ValueError)):
        with pytest.raises(err):
            E.check_candidates(cands, 3)
    assert E.block_bytes(1, 1) == 8 * 64 * (17 + 3) and E.block_bytes(2049, 17) == 8 * 64 * (33 + 6)


def test_rank_measurements_uses_common_random_numbers(monkeypatch):
    """Candidate c is handed the first F_c columns of ONE normal array drawn from the seed: nested columns, the same for
    a repeated call.  The device call is replaced by the reference, so the rule is checked without a device."""
    from gpemu import experiment as E
    seen = []

    def fake_pair_lse(Y, Z, self_index=None, centre=None, device=None, workspace_bytes=0):
        seen.append((Y.copy(), Z.copy()))
        ref = R.pairlse_ref(Y, Z, self_index)
        return ref["lse"].astype(np.float64), ref["ess"].astype(np.float64)

    monkeypatch.setattr(E, "pair_lse", fake_pair_lse)
    means, _ = R.linear_gaussian_case(3, 5, 256, 0)
    cands = [dict(features=[0, 1, 2], y_err=1.0, label="a"), dict(features=[4], y_err=0.5), dict(features=[3, 1, 0, 2, 4],
                                                                                                 cov=2.0 * np.eye(5))]
    out = E.rank_measurements(means, cands, n_outer=64, seed=7)
    noise = np.random.default_rng(7).standard_normal((64, 5))
    rows = E.selected_rows(256, 64)
    for (Y, Z), cand in zip(seen, cands):
        f = cand["features"]
        sd = cand.get("y_err", math.sqrt(2.0))
        assert np.allclose(Z, means[:, f] / sd, rtol=1e-15, atol=0)
        assert np.array_equal(Y, Z[rows] + noise[:, :len(f)])
    assert out["labels"] == ["a", "candidate 1", "candidate 2"]
    assert list(out["order"]) == list(np.argsort(-out["eig_nats"], kind="stable"))
    assert [r["index"] for r in out["table"]] == list(out["order"])
    again = E.rank_measurements(means, cands, n_outer=64, seed=7)
    assert np.array_equal(again["eig_nats"], out["eig_nats"]) and np.array_equal(seen[3][0], seen[0][0])
    other = E.rank_measurements(means, cands, n_outer=64, seed=8)
    assert not np.array_equal(other["eig_nats"], out["eig_nats"])
    for r, ref_seed in ((out["results"][0], 7),):
        one = R.eig_ref(means[:, [0, 1, 2]], y_err=1.0, n_outer=64, noise=noise)
        assert r["eig_nats"] == pytest.approx(one["eig_nats"], abs=1e-12)


def test_drop_in_settings_validation():
    from bayesian_inference import mcmc
    assert mcmc.expected_information_gain_settings({}) == (False, 1.0, 4096, 16384)
    assert mcmc.expected_information_gain_settings({"expected_information_gain": True, "eig_scale": 0.5, "eig_n_outer": 100,
                                                    "eig_n_inner": 2000}) == (True, 0.5, 100, 2000)
    assert mcmc.expected_information_gain_settings({"eig_scale": 2}) == (False, 2.0, 4096, 16384)
    for bad in ({"expected_information_gain": 1}, {"expected_information_gain": "yes"}, {"eig_scale": 0.0},
                {"eig_scale": -1.0}, {"eig_scale": float("inf")}, {"eig_scale": "1"}, {"eig_scale": True},
                {"eig_n_outer": 0}, {"eig_n_outer": 1.5}, {"eig_n_outer": True}, {"eig_n_outer": 2 ** 31},
                {"eig_n_inner": 1}, {"eig_n_inner": 2.0}, {"eig_n_inner": 2 ** 31}):
        with pytest.raises(ValueError, match="parameters.mcmc"):
            mcmc.expected_information_gain_settings(bad)


def test_new_symbols_paths_and_constants():
    from gpemu import _lib
    from gpemu import experiment as E
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpemu.h")).read()
    declared = set(re.findall(r"\b(gpemu_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("gpemu_pair_lse", "gpemu_pair_lse_dev", "gpemu_pairlse_centre_dev", "gpemu_pairlse_path_counts"):
        assert name in declared and name in _lib.exported_symbols() and hasattr(L, name), name
    enum = re.search(r"enum gpemu_pairlse_path \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"GPEMU_PAIRLSE_PATH_([A-Z0-9_]+?)\b", enum)
    assert names[:-1] == list(E.PATHS) == ["CENTRE", "PARTIAL", "MERGE", "ROW_BATCH"]
    assert names[-1] == "COUNT"
    assert int(re.search(r"#define GPEMU_PAIRLSE_CHUNK (\d+)", hdr).group(1)) == E.CHUNK == R.CHUNK
    assert int(re.search(r"#define GPEMU_PAIRLSE_TILE_ROWS (\d+)", hdr).group(1)) == E.TILE_ROWS == R.TILE_ROWS
    out = (E.C.c_int64 * 8)()
    assert L.gpemu_pairlse_path_counts(out, 8) == len(E.PATHS)
    assert L.gpemu_pairlse_path_counts(None, 8) == -1
