"""-m gpu tests of the weighted bands, highest-density intervals and densities of a reweighted chain
(gpemu_posterior_predictive_weighted*, gpemu_weighted_hpd*, gpemu_weighted_kde1d*) against
tests/wsummary_ref.py.  Figures measured on an MI355X are printed by every test before it asserts (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import marginals_ref as MR
import reuse_cases as R
import wsummary_ref as WR

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
POOL = 8192
CHUNK = 2048            # rows per predict pass of the reduction (csrc/k_postpred.hip: PP_CHUNK)
U = 2.0 ** -53
ERR_ARG = -1


def _ledger():
    from gpemu import _lib
    s = _lib.devmem_stats()
    return s["live_blocks"], s["live_bytes"], s["allocs"] - s["frees"]


# ---- weights ---------------------------------------------------------------------------------------------------------
def _log_uniform_q(S, seed):
    """one row of fixed-point weights of a log-uniform scenario on rows in [0.1, 1]^3, made on the device"""
    import torch
    from gpemu import reweight as RW
    u = torch.from_numpy(np.random.default_rng(seed).uniform(0.1, 1.0, (S, 3))).cuda()
    L = RW.log_prior_dev(0, u.data_ptr(), 1, S, S, 3, RW.check_priors([[1, 1, 1]], 3, [0.1] * 3, [1.0] * 3), [0.1] * 3)
    _, lw = RW.logmeanexp_dev(L, normalise=True)
    q, _ = RW.fixed_weights_dev(lw)
    return q.cpu().numpy().view(np.uint64)[0]


@functools.lru_cache(maxsize=None)
def _weights(S):
    """q (3, S) uint64: equal weights, the log-uniform scenario, 90 % zeros"""
    rng = np.random.default_rng(1000 + S)
    equal = np.full(S, (1 << 52) // S, dtype=np.uint64)
    sparse = rng.integers(1, (1 << 52) // S, S).astype(np.uint64)
    sparse[rng.random(S) < 0.9] = 0
    if not sparse.any():
        sparse[S // 2] = 12345
    q = np.stack([equal, _log_uniform_q(S, S), sparse])
    assert np.all(q.sum(axis=1, dtype=np.uint64) < (1 << 53))
    return q


# ---- 1. bands --------------------------------------------------------------------------------------------------------
class _Case:
    """a device model and a pool of rows inside its box: "general" (d = 3) and "wide" (d = 12) of tests/reuse_cases.py, whose
    6 and 8 features always fit the workspace at once, and "rbf40", the 40-feature model of
    tests/test_gpu_posterior_predictive.py, which the feature-blocked path needs (a block is 16 features)"""

    def __init__(self, name):
        import golden_util as GU
        import pp_ref
        from oracle import gp_oracle as O
        if name == "rbf40":
            self.d, self.k = 6, 3
            spec = O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)
            model, lo, hi = pp_ref.problem(100, self.d, 40, self.k, spec, seed=0)
            self.dm, self.X = GU.device_model(model), np.random.default_rng(11).uniform(lo, hi, (POOL, self.d))
        else:
            P = R.problem(name)
            self.d, self.k, self.dm, self.X = P.d, P.k, R.fresh(P), R.rows(P, "wsummary", POOL)
        self.F = self.dm.F


@functools.lru_cache(maxsize=None)
def _model(name):
    c = _Case(name)
    return c, c.dm, c.X


@functools.lru_cache(maxsize=None)
def _chunk(name, r0, nb):
    """predict_full's central values (nb, F) and variances (nb, F) of pool rows [r0, r0 + nb): the launches of one
    predict pass of the reduction"""
    _, dm, X = _model(name)
    cv, cov = dm.predict_full(X[r0:r0 + nb], n_div=1.0)
    return cv, np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2))


def _per_sample(name, S):
    parts = [_chunk(name, r0, min(CHUNK, S - r0)) for r0 in range(0, S, CHUNK)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _same(a, b):
    for key in ("mean", "variance_parameters", "variance_emulator", "variance", "quantiles"):
        assert a[key].tobytes() == b[key].tobytes(), key


def _check_bands(out, cv, s2, q, k, label):
    """one weight row against the extended-precision weighted sums of predict_full's central values and variances.

    D = wsummary_ref.tree_depth(S) additions lie on the longest path of the reduction's tree (a lane's 16 fused
    multiply-adds, 6 butterfly levels, 3 over the waves, the chunks in order); the division by Q, and for the centred
    moment the difference (twice, it is squared) and the product with q, round once each: (D + 3) u sum q |term| / Q.
      variance_parameters: the device centres at ITS mean, off by at most the mean's bound b: + b^2 (the cross term
        vanishes at the exact mean).
      variance_emulator: the sum runs over the PC variances and the linear form adds k fused multiply-adds and
        cov_unexplained: D + k + 1 on the path; the reference's own terms, predict_full's variances, carry the k + 1
        additions and the products by scale^2 of their own evaluation in double, (k + 4) u of each (all terms >= 0)."""
    S = cv.shape[0]
    D = WR.tree_depth(S)
    worst = {}
    m, mabs = WR.weighted_sums(cv, q)
    bm = (D + 3) * U * mabs
    err = np.abs(out["mean"].astype(np.longdouble) - m)
    worst["mean"] = float(np.max(err / np.maximum(bm, np.finfo(float).tiny)))
    v, _ = WR.weighted_sums((cv.astype(np.longdouble) - m) ** 2, q)
    bv = (D + 3) * U * v + bm * bm
    errv = np.abs(out["variance_parameters"].astype(np.longdouble) - v)
    worst["variance_parameters"] = float(np.max(errv / np.maximum(bv, np.finfo(float).tiny))) if np.any(bv > 0) else 0.0
    e, _ = WR.weighted_sums(s2, q)
    be = (D + k + 1 + 3) * U * e + (k + 4) * U * e
    erre = np.abs(out["variance_emulator"].astype(np.longdouble) - e)
    worst["variance_emulator"] = float(np.max(erre / be))
    print(f"{label}: error / bound " + ", ".join(f"{a} {b:.3e}" for a, b in worst.items()))
    assert np.all(err <= bm), "mean"
    assert np.all(errv <= bv), "variance_parameters"
    assert np.all(erre <= be), "variance_emulator"
    assert np.array_equal(out["variance"], out["variance_parameters"] + out["variance_emulator"])
    assert out["total_weight"] == int(q.sum(dtype=np.uint64))
    return worst


@pytest.mark.parametrize("name,S", [("general", 1), ("general", 255), ("general", 4096), ("general", 4097),
                                    ("general", 8192), ("wide", 4097), ("rbf40", 1), ("rbf40", 255), ("rbf40", 4096),
                                    ("rbf40", 4097), ("rbf40", 8192)])
def test_bands_on_both_paths_against_the_reference(name, S):
    from gpemu import reweight as RW
    from gpemu.model import postpred_workspace_bytes
    P, dm, X = _model(name)
    q = _weights(S)
    cv, s2 = _per_sample(name, S)
    c0, l0 = RW.wsummary_path_counts(), _ledger()
    whole = dm.posterior_predictive_weighted(X[:S], q, PROBS)
    c1 = RW.wsummary_path_counts()
    blocked = dm.posterior_predictive_weighted(X[:S], q, PROBS, workspace_bytes=postpred_workspace_bytes(S, P.k, 16))
    c2 = RW.wsummary_path_counts()
    assert _ledger() == l0
    print(f"{name} S={S}: counters whole {({n: c1[n] - c0[n] for n in c1 if c1[n] != c0[n]})}, "
          f"blocked {({n: c2[n] - c1[n] for n in c2 if c2[n] != c1[n]})}")
    nblocks = -(-P.F // 16)             # the second call's workspace holds 16 features
    assert c1["BANDS_WHOLE"] - c0["BANDS_WHOLE"] == 1 and c1["BANDS_FEATURE_BLOCKED"] == c0["BANDS_FEATURE_BLOCKED"]
    assert c2["BANDS_FEATURE_BLOCKED"] - c1["BANDS_FEATURE_BLOCKED"] == (nblocks > 1)
    assert c2["BANDS_WHOLE"] - c1["BANDS_WHOLE"] == (nblocks == 1)
    assert c2["ROW_REDUCE"] - c1["ROW_REDUCE"] == 1 + 2 * nblocks
    assert len(whole) == 3
    for w in range(3):
        _same(whole[w], blocked[w])
        ref = WR.weighted_quantiles(cv, q[w], PROBS)
        differ = int(np.sum(whole[w]["quantiles"].view(np.uint64) != ref.view(np.uint64)))
        print(f"{name} S={S} row {w}: quantiles that differ from the reference's bits: {differ} of {ref.size}")
        assert whole[w]["quantiles"].tobytes() == ref.tobytes()
        _check_bands(whole[w], cv, s2, q[w], P.k, f"{name} S={S} row {w}")
    again = dm.posterior_predictive_weighted(X[:S], q, PROBS)
    for w in range(3):
        _same(whole[w], again[w])
    # how the weight rows are grouped into launches does not matter: a row alone gives its bits
    alone = dm.posterior_predictive_weighted(X[:S], q[1:2], PROBS)
    _same(whole[1], alone[0])


def test_bands_of_a_thinned_block_view_in_place():
    import torch
    from gpemu import reweight as RW
    P, dm, _ = _model("general")
    nb, br, bs = 16, 4, 6
    S = nb * br
    buf = R.rows(R.problem("general"), "wsummary_view", nb * bs)
    t = torch.from_numpy(buf).cuda()
    rows = np.ascontiguousarray(buf.reshape(nb, bs, P.d)[:, :br].reshape(S, P.d))
    q = _weights(S)
    dq = torch.from_numpy(q.view(np.int64)).cuda()
    tgt = RW.targets(PROBS, q.sum(axis=1, dtype=np.uint64))
    mean, vp, ve = (torch.full((3, P.F), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    qt = torch.full((3, P.F, len(PROBS)), float("nan"), dtype=torch.float64, device="cuda")
    # (a model keeps the schedules of a batch size it meets for the first time: the ledger is read around a second call)
    for _ in range(2):
        l0 = _ledger()
        dm.posterior_predictive_weighted_dev(t.data_ptr(), nb, br, bs, dq, tgt, mean.data_ptr(), vp.data_ptr(),
                                             ve.data_ptr(), qt.data_ptr())
    assert _ledger() == l0
    host = dm.posterior_predictive_weighted(rows, q, PROBS)
    for w in range(3):
        assert mean[w].cpu().numpy().tobytes() == host[w]["mean"].tobytes()
        assert vp[w].cpu().numpy().tobytes() == host[w]["variance_parameters"].tobytes()
        assert ve[w].cpu().numpy().tobytes() == host[w]["variance_emulator"].tobytes()
        assert np.ascontiguousarray(qt[w].cpu().numpy().T).tobytes() == host[w]["quantiles"].tobytes()
    cv, cov = dm.predict_full(rows, n_div=1.0)
    for w in range(3):
        ref = WR.weighted_quantiles(cv, q[w], PROBS)
        assert host[w]["quantiles"].tobytes() == ref.tobytes()
        _check_bands(host[w], cv, np.diagonal(cov, axis1=1, axis2=2), q[w], P.k, f"view row {w}")


def test_bands_with_power_of_two_weights_are_the_unweighted_bits():
    """q_s = 2^39 at S = 8192: scaling by a power of two is exact and the tree is the same"""
    P, dm, X = _model("general")
    q = np.full((1, POOL), 1 << 39, dtype=np.uint64)
    got = dm.posterior_predictive_weighted(X, q, PROBS)[0]
    plain = dm.posterior_predictive(X, probabilities=PROBS)
    assert got["total_weight"] == 1 << 52
    assert got["mean"].tobytes() == plain["mean"].tobytes()
    assert got["variance_emulator"].tobytes() == plain["variance_emulator"].tobytes()
    rel = np.max(np.abs(got["variance_parameters"] - plain["variance_parameters"]) / plain["variance_parameters"])
    print(f"2^39 weights: variance_parameters against the unweighted one, max relative difference {rel:.3e}")


def test_bands_with_all_weight_on_one_sample():
    P, dm, X = _model("general")
    S, at = 4097, 4000
    q = np.zeros((1, S), dtype=np.uint64)
    q[0, at] = 1 << 52
    got = dm.posterior_predictive_weighted(X[:S], q, PROBS)[0]
    cv, _ = _per_sample("general", S)
    assert got["mean"].tobytes() == cv[at].tobytes()
    assert np.all(got["variance_parameters"] == 0.0)
    for i in range(len(PROBS)):
        assert got["quantiles"][i].tobytes() == cv[at].tobytes()


# ---- 2. highest-density intervals ------------------------------------------------------------------------------------
HPD_SIZES = (1, 2, 2047, 2048, 2049, 4097, 65537)


def _hpd_rows(S):
    """V (6, S): continuous, one decimal (heavy ties), all equal, with a NaN, with +inf, continuous again"""
    rng = np.random.default_rng(77 + S)
    V = np.stack([rng.normal(size=S), np.round(rng.normal(size=S), 1), np.full(S, 0.25), rng.normal(size=S),
                  rng.normal(size=S), rng.gamma(2.0, size=S)])
    V[3, S // 2] = np.nan
    V[4, S // 3] = np.inf
    V[1, : max(S // 50, 1)] = -0.0         # zeros of both signs among the ties
    return np.ascontiguousarray(V)


def _hpd_weights(S):
    """q (4, S): equal, log-uniform, 90 % zeros with zero weight at both ends of every row's order, one sample"""
    q3 = _weights(S)
    one = np.zeros(S, dtype=np.uint64)
    one[S // 2] = 1 << 52
    return np.ascontiguousarray(np.vstack([q3, one[None]]))


def _hpd_targets(q):
    from gpemu import reweight as RW
    Q = q.sum(axis=1, dtype=np.uint64)
    t = RW.targets([0.68, 0.9], Q)
    return np.array([[1, int(Q[w]), int(Q[w]) + 1] + [int(v) for v in t[w]] for w in range(len(Q))], dtype=np.uint64)


def _hpd_ref(V, q, tgt):
    out = np.empty((q.shape[0], V.shape[0], tgt.shape[1], 2))
    for w in range(q.shape[0]):
        for v in range(V.shape[0]):
            for l in range(tgt.shape[1]):
                out[w, v, l] = WR.hpd(V[v], q[w], int(tgt[w, l]))
    return out


def _call_hpd(V, q, tgt):
    from gpemu import _lib
    out = np.full((q.shape[0], V.shape[0], tgt.shape[1], 2), -1.0)
    _lib.check(_lib.lib().gpemu_weighted_hpd(0, V.shape[0], V.shape[1], _lib.ptr(V), q.shape[0], _lib.ptr(q), tgt.shape[1],
                                             _lib.ptr(tgt), _lib.ptr(out)))
    return out


def _bits(a):
    """the bytes with every NaN as one NaN"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


@pytest.mark.parametrize("S", HPD_SIZES)
def test_hpd_is_the_reference_bit_for_bit(S):
    V, q = _hpd_rows(S), _hpd_weights(S)
    if S > 2:       # zero weights at both ends of the continuous rows
        for v in (0, 5):
            order = np.argsort(V[v])
            q[2, order[:3]] = 0
            q[2, order[-3:]] = 0
        if not q[2].any():
            q[2, S // 2] = 999
    tgt = _hpd_targets(q)
    l0 = _ledger()
    got = _call_hpd(V, q, tgt)
    assert _ledger() == l0
    ref = _hpd_ref(V, q, tgt)
    bad = int(np.sum(np.frombuffer(_bits(got), dtype=np.uint64) != np.frombuffer(_bits(ref), dtype=np.uint64)))
    print(f"weighted hpd S={S}: {bad} of {got.size} ends differ from the reference")
    assert _bits(got) == _bits(ref)
    assert np.all(np.isnan(got[:, 3])) and np.all(np.isnan(got[:, 4]))          # the NaN row, the +inf row
    assert np.all(np.isnan(got[:, :, 2]))                                      # t = Q + 1
    assert not np.any(np.isnan(got[:, (0, 1, 2, 5)][:, :, (0, 1, 3, 4)]))
    assert _bits(_call_hpd(V, q, tgt)) == _bits(got)


@pytest.mark.parametrize("S", (2049, 65537))
def test_hpd_under_equal_weights_is_the_unweighted_interval(S):
    from gpemu import marginals as M
    V = _hpd_rows(S)
    c = (1 << 52) // S
    n_out = M.n_outside([0.68, 0.9], S)
    q = np.full((1, S), c, dtype=np.uint64)
    tgt = np.ascontiguousarray((c * (S - n_out + 1)).astype(np.uint64)[None])
    got = _call_hpd(V, q, tgt)[0]
    plain = M.hpd_intervals(V.T, [0.68, 0.9]).transpose(1, 0, 2)
    assert _bits(got) == _bits(plain)


def test_hpd_on_a_chain_in_place_in_two_batches():
    """R_v = 3 parameters of a [S][d] chain, elem_stride = d; a workspace of one pair at a time gives the same bytes, and
    less than one pair is an out-of-memory error with the sizes"""
    import torch
    from gpemu import _lib
    from gpemu import reweight as RW
    S, d = 4097, 3
    x = np.ascontiguousarray(_hpd_rows(S)[[0, 1, 5]].T)
    q = _weights(S)
    Q = q.sum(axis=1, dtype=np.uint64)
    t = torch.from_numpy(x).cuda()
    dq = torch.from_numpy(q.view(np.int64)).cuda()
    host = RW.weighted_hpd(x, [0.68, 0.9], q, Q)
    assert host.shape == (3, 2, d, 2)
    c0, l0 = RW.wsummary_path_counts(), _ledger()
    dev = RW.weighted_hpd(t, [0.68, 0.9], dq, Q)
    c1 = RW.wsummary_path_counts()
    assert _ledger() == l0
    assert dev.tobytes() == host.tobytes()
    assert c1["HPD_SORT_BATCH"] - c0["HPD_SORT_BATCH"] == 1 and c1["HPD_PLACE"] - c0["HPD_PLACE"] == 3
    per_pair = 24 * S + 1032 * -(-S // 2048) + 16 * 2 * -(-S // 4096) + 4          # include/gpemu.h
    two = RW.weighted_hpd(t, [0.68, 0.9], dq, Q, workspace_bytes=2 * per_pair)
    c2 = RW.wsummary_path_counts()
    assert c2["HPD_SORT_BATCH"] - c1["HPD_SORT_BATCH"] == 2 and c2["HPD_PLACE"] - c1["HPD_PLACE"] == 6
    assert two.tobytes() == host.tobytes()
    for w in range(3):
        for j in range(d):
            for l, c in enumerate((0.68, 0.9)):
                assert tuple(host[w, l, j]) == WR.hpd(x[:, j], q[w], int(RW.targets([c], Q[w:w + 1])[0, 0]))
    with pytest.raises(_lib.GpemuError, match=rf"out of memory.*{per_pair} bytes"):
        RW.weighted_hpd(t, [0.68, 0.9], dq, Q, workspace_bytes=per_pair - 1)
    assert _ledger() == l0


# ---- 3. kernel density -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 8191, 8192, 8193))
@pytest.mark.parametrize("G", (1, 1024, 1025))
def test_kde_within_the_error_bound(S, G):
    """The unweighted kernel's bound (tests/test_gpu_marginals.py: test_kde_within_the_error_bound, c = 0.55 (depth + 8) in
    units of eps = 2 u) with one more rounding per term for the product with q: c + 0.55, as 1.1 u / 2 eps.  (The kernel
    fuses that product into the addition, so it stays inside.)"""
    from gpemu import reweight as RW
    rng = np.random.default_rng(S * 5 + G)
    d = 1
    x = rng.normal(0.3, 1.7, (S, d))
    q = _weights(S)
    sd = np.where(x.std(axis=0) > 0, x.std(axis=0), 1.0)
    h = np.ascontiguousarray(np.outer([1e-3, 0.3, 10.0], sd))                   # (R_w, d)
    grid = np.stack([[np.linspace(x[:, j].min() - 3 * h[w, j], x[:, j].max() + 3 * h[w, j], G) for j in range(d)]
                     for w in range(3)])
    l0 = _ledger()
    got = RW.weighted_kde_1d(x, q, grid=grid, bandwidth=h)
    assert _ledger() == l0
    assert got["density"].shape == (3, d, G)
    assert RW.weighted_kde_1d(x, q, grid=grid, bandwidth=h)["density"].tobytes() == got["density"].tobytes()
    worst = 0.0
    eps = np.finfo(np.float64).eps
    for w in range(3):
        for j in range(d):
            ref = WR.kde(x[:, j], q[w], grid[w, j], h[w, j])
            tol = (MR.kde_bound_factor(S) + 0.55) * eps * (ref + 1.0 / (np.sqrt(2.0 * np.pi) * h[w, j]))
            err = np.abs(got["density"][w, j].astype(np.longdouble) - ref)
            worst = max(worst, float(np.max(err / tol)))
    print(f"weighted kde S={S} G={G}: worst error / bound = {worst:.3e}")
    assert worst <= 1.0


def test_kde_with_power_of_two_weights_is_the_unweighted_density_and_device_tensors_give_the_same_bytes():
    import torch
    from gpemu import marginals as M
    from gpemu import reweight as RW
    S, d = 8192, 3
    x = np.random.default_rng(5).normal(size=(S, d))
    q = np.full((1, S), 1 << 39, dtype=np.uint64)
    plain = M.kde_1d(x, n_grid=1025)
    got = RW.weighted_kde_1d(x, q, grid=plain["grid"], bandwidth=plain["bandwidth"])
    assert got["density"][0].tobytes() == plain["density"].tobytes()
    q3 = _weights(S)
    host = RW.weighted_kde_1d(x, q3)
    c0 = RW.wsummary_path_counts()
    dev = RW.weighted_kde_1d(torch.from_numpy(x).cuda(), torch.from_numpy(q3.view(np.int64)).cuda())
    assert RW.wsummary_path_counts()["KDE"] - c0["KDE"] == 1
    for key in ("grid", "density", "bandwidth"):
        assert dev[key].tobytes() == host[key].tobytes(), key
    # a sample of weight 0 contributes nothing, whatever its value
    x2 = x.copy()
    x2[q3[2] == 0] = np.nan
    a = RW.weighted_kde_1d(x, q3[2:3], grid=host["grid"][2], bandwidth=host["bandwidth"][2])
    b = RW.weighted_kde_1d(x2, q3[2:3], grid=host["grid"][2], bandwidth=host["bandwidth"][2])
    assert a["density"].tobytes() == b["density"].tobytes()


def test_default_bandwidth_is_scipys():
    from gpemu import reweight as RW
    S = 4097
    x = np.random.default_rng(8).normal(size=(S, 2))
    q = _weights(S)
    got = RW.weighted_kde_1d(x, q, n_grid=64)
    for w in range(3):
        wn = q[w].astype(np.float64) / q[w].sum(dtype=np.uint64)
        for j in range(2):
            ref = WR.scipy_bandwidth(x[:, j], wn)
            print(f"bandwidth row {w} parameter {j}: {got['bandwidth'][w, j]:.17g} against scipy's {ref:.17g}")
            assert abs(got["bandwidth"][w, j] - ref) <= 1e-12 * ref


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_return_err_arg_and_leave_the_ledger_alone():
    """(On a model of its own, closed at the end: tests/test_gpu_devmem.py runs this test again with every library call
    watched, and demands the ledger back where it was.)"""
    P = R.problem("general")
    dm = R.fresh(P)
    try:
        _refusals(P, dm, R.rows(P, "wsummary", 257))
    finally:
        dm.close()


def _refusals(P, dm, X):
    import torch
    from gpemu import _lib
    L = _lib.lib()
    S = 257
    V = torch.from_numpy(_hpd_rows(S)[[0, 1, 5]].copy()).cuda()
    q = _weights(S)
    q65 = torch.from_numpy(np.ascontiguousarray(np.tile(q[:1], (65, 1))).view(np.int64)).cuda()
    dq = torch.from_numpy(q.view(np.int64)).cuda()
    tgt = np.ascontiguousarray(np.full((65, 2), 5, dtype=np.uint64))
    zero = tgt.copy()
    zero[0, 1] = 0
    out = torch.empty((65 * 3 * 2 * 2 + 65 * 3 * 4,), dtype=torch.float64, device="cuda")
    grid, h = np.zeros((65, 3, 4)), np.ones((65, 3))
    bad_h = h.copy()
    bad_h[0, 1] = np.inf
    dX = torch.from_numpy(X[:S].copy()).cuda()
    mean = torch.empty((65, P.F), dtype=torch.float64, device="cuda")
    vp, p = C.c_void_p, _lib.ptr
    ctx = _lib.call_ctx(0)

    def hpd(R_w, dq_, t):
        return L.gpemu_weighted_hpd_dev(0, 3, S, vp(V.data_ptr()), S, 1, R_w, dq_, S, 2, p(t), vp(out.data_ptr()),
                                        C.byref(ctx))

    def kde(R_w, dq_, h_):
        return L.gpemu_weighted_kde1d_dev(0, 3, S, vp(V.data_ptr()), S, 1, R_w, dq_, S, 4, p(grid), p(h_),
                                          vp(out.data_ptr()), C.byref(ctx))

    def bands(R_w, dq_, t):
        return L.gpemu_posterior_predictive_weighted_dev(dm._h, vp(dX.data_ptr()), 1, S, S, R_w, dq_, S, 2, p(t),
                                                         vp(mean.data_ptr()), None, None, vp(out.data_ptr()), C.byref(ctx))

    d3, d65 = vp(dq.data_ptr()), vp(q65.data_ptr())
    calls = {"hpd R_w=0": lambda: hpd(0, d3, tgt), "hpd R_w=65": lambda: hpd(65, d65, tgt),
             "hpd target 0": lambda: hpd(3, d3, zero), "hpd null weights": lambda: hpd(3, None, tgt),
             "kde R_w=0": lambda: kde(0, d3, h), "kde R_w=65": lambda: kde(65, d65, h),
             "kde non-finite h": lambda: kde(3, d3, bad_h), "kde null weights": lambda: kde(3, None, h),
             "bands R_w=0": lambda: bands(0, d3, tgt), "bands R_w=65": lambda: bands(65, d65, tgt),
             "bands target 0": lambda: bands(3, d3, zero), "bands null weights": lambda: bands(3, None, tgt)}
    for name, call in calls.items():
        l0 = _ledger()
        rc = call()
        print(f"{name}: {rc} ({_lib.last_error()})")
        assert rc == ERR_ARG and _ledger() == l0, name
    assert bands(3, d3, tgt) == 0       # the model keeps the schedules of a batch size it meets for the first time
    for call in (lambda: hpd(3, d3, tgt), lambda: kde(3, d3, h), lambda: bands(3, d3, tgt)):
        l0 = _ledger()
        assert call() == 0 and _ledger() == l0
