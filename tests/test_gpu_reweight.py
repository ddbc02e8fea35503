"""-m gpu tests of the importance reweighting and the weighted summaries on the device (gpemu_logprior*,
gpemu_logmeanexp_dev, gpemu_weights_fixed_dev, gpemu_weighted_select*, gpemu_weighted_hist*, gpemu.reweight; DESIGN.md
§4.39) against tests/reweight_ref.py.  The weights are integers whose sums are exact, so quantiles and histograms are
compared bit for bit, from the q the device produced; the log-prior and the quantisation are held to bounds counted from
their roundings.

Figures measured on an MI355X are printed by every test before it asserts (run with -s)."""
import ctypes as C
import math

import numpy as np
import pytest

import reweight_ref as RR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ONE = 1 << 52


@pytest.fixture(scope="module", autouse=True)
def counters_at_start():
    from gpemu import reweight as R
    return R.path_counts()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _q_dev(q):
    return _dev(np.ascontiguousarray(q, dtype=np.uint64).view(np.int64))


def _device_weights(R_w, S, seed, spread=2.0):
    """normalised log-weights of a random log-ratio, quantised ON THE DEVICE: (q (R_w, S) uint64, Q, q as a tensor)"""
    from gpemu import reweight as R
    rng = np.random.default_rng(seed)
    l = spread * rng.normal(size=(R_w, S))
    _, lw = R.logmeanexp_dev(_dev(l), normalise=True)
    qd, Q = R.fixed_weights_dev(lw)
    return qd.cpu().numpy().view(np.uint64), Q, qd


def _select(x_rows, qd, tgt, layout, workspace_bytes=0):
    """x_rows (R_v, S) through the device in the chain layout (elem_stride = R_v) or dense (row_stride = S)"""
    from gpemu import reweight as R
    R_v, S = x_rows.shape
    if layout == "chain":
        t = _dev(x_rows.T)
        return R.weighted_quantile_dev(0, t.data_ptr(), R_v, S, 1, R_v, qd, tgt, workspace_bytes)
    t = _dev(x_rows)
    return R.weighted_quantile_dev(0, t.data_ptr(), R_v, S, S, 1, qd, tgt, workspace_bytes)


def _check_select(x_rows, q, qd, tgt, layout, **kw):
    got = _select(x_rows, qd, tgt, layout, **kw)
    assert got.shape == (q.shape[0], x_rows.shape[0], tgt.shape[1])
    for w in range(q.shape[0]):
        for v in range(x_rows.shape[0]):
            want = RR.weighted_select_fast(x_rows[v], q[w], tgt[w])
            assert np.array_equal(got[w, v], want), (w, v, np.flatnonzero(got[w, v] != want)[:5], got[w, v][:4], want[:4])
    return got


def _targets(Q, n, rng):
    """n targets per weight row: the ends 1 and Q, the median, the rest uniform in [1, Q], in no order"""
    out = np.empty((len(Q), n), dtype=np.uint64)
    for w, Qw in enumerate(Q):
        t = [1, int(Qw), (int(Qw) + 1) // 2] + [int(v) for v in rng.integers(1, int(Qw) + 1, max(n - 3, 0))]
        out[w] = rng.permutation(np.array(t[:n] if n >= 3 else t[2:2 + n], dtype=np.uint64))
    return out


# ---- 1. weighted select ---------------------------------------------------------------------------------------------------
# every S, R_v, layout, R_w and n_targets of the issue at least once; 63 | 64 | 65 straddle a wave, 2049 a workgroup's
# 256-element rounds, 4097 a slice of 4096
SELECT_SHAPES = [(1, 1, "chain", 1, 1), (2, 3, "dense", 1, 1), (63, 9, "chain", 3, 16), (64, 1, "dense", 3, 17),
                 (65, 3, "chain", 1, 40), (2049, 9, "chain", 3, 17), (2049, 3, "dense", 1, 16), (4097, 9, "dense", 3, 40),
                 (4097, 1, "chain", 1, 1), (4097, 3, "chain", 3, 16)]


@pytest.mark.parametrize("S,R_v,layout,R_w,nt", SELECT_SHAPES)
def test_weighted_select_equals_the_reference_on_every_shape(S, R_v, layout, R_w, nt):
    rng = np.random.default_rng(S * 37 + R_v * 5 + nt)
    q, Q, qd = _device_weights(R_w, S, S + nt)
    assert np.array_equal(Q, q.sum(axis=1, dtype=np.uint64))
    x = rng.normal(size=(R_v, S))
    _check_select(x, q, qd, _targets(Q, nt, rng), layout)


def _value_rows(S, rng):
    base = rng.normal(size=40)
    tiny = 1.0 + np.arange(S) % 7 * 2.0 ** -52                                  # differ in the last mantissa bits only
    m = rng.random(S)
    zeros = np.where(m < 0.4, -0.0, np.where(m < 0.8, 0.0, rng.normal(size=S)))    # +-0 among other values
    return np.stack([rng.normal(size=S), np.full(S, -3.25), rng.permutation(tiny), -np.abs(rng.normal(size=S)),
                     rng.normal(size=S) * 10.0 ** rng.uniform(-300, 300, S), zeros, base[rng.integers(0, 40, S)]])


@pytest.mark.parametrize("layout", ["chain", "dense"])
def test_weighted_select_on_every_kind_of_value_row(layout):
    """random, all equal, last mantissa bits, negative, mixed signs over 600 decades, +-0, 40 repeated rows"""
    S = 2049
    rng = np.random.default_rng(7)
    x = _value_rows(S, rng)
    q, Q, qd = _device_weights(2, S, 11)
    got = _check_select(x, q, qd, _targets(Q, 17, rng), layout)
    assert np.all(got[:, 1] == -3.25) and np.all(np.isin(got[:, 6], x[6]))


def test_weighted_select_under_psis_weights_and_small_workspaces():
    from gpemu import reweight as R
    S = 4097
    rng = np.random.default_rng(3)
    l = 1.5 * rng.standard_t(4, size=(3, S))
    st = R.weights(_dev(l))
    assert np.all(np.isfinite(st["pareto_k"]))
    qd, Q = R.fixed_weights_dev(st["log_weights"])
    q = qd.cpu().numpy().view(np.uint64)
    x = rng.normal(size=(9, S))
    tgt = R.targets([0.05, 0.5, 0.95], Q)
    want = _check_select(x, q, qd, tgt, "chain")
    for ws in (40000, 5 * 33288):               # one pair per batch, five pairs per batch: the same elements
        assert np.array_equal(_check_select(x, q, qd, tgt, "chain", workspace_bytes=ws), want)
    print(f"PSIS weights, S = {S}: pareto_k {st['pareto_k']}, Q - 2^52 = {[int(v) - ONE for v in Q]}")


def test_weighted_select_on_every_kind_of_weights():
    S = 2049
    rng = np.random.default_rng(5)
    x = np.stack([rng.normal(size=S), rng.normal(size=40)[rng.integers(0, 40, S)]])
    ps = np.array([0.0, 0.05, 0.3333, 0.5, 0.95, 1.0])
    # all equal: numpy's unweighted inverted CDF (p S is no integer for these p, or p is an end)
    for c in (1, 12345, ONE // S):
        q = np.full((1, S), c, dtype=np.uint64)
        tgt = np.array([[RR.target(p, c * S) for p in ps]], dtype=np.uint64)
        got = _check_select(x, q, _q_dev(q), tgt, "dense")
        for v in range(2):
            assert np.array_equal(got[0, v], np.quantile(x[v], ps, method="inverted_cdf"))
    # one sample holds all of Q: every target returns it
    q = np.zeros((1, S), dtype=np.uint64)
    q[0, 1234] = ONE
    got = _check_select(x, q, _q_dev(q), np.array([[1, ONE // 2, ONE]], dtype=np.uint64), "chain")
    assert np.all(got[0, 0] == x[0, 1234]) and np.all(got[0, 1] == x[1, 1234])
    # half of the weights are 0: such a sample is never the answer
    q, Q, _ = _device_weights(1, S, 21)
    q = q.copy()
    q[0, rng.permutation(S)[:S // 2]] = 0
    Q = q.sum(axis=1, dtype=np.uint64)
    got = _check_select(x, q, _q_dev(q), _targets(Q, 40, rng), "chain")
    assert np.all(np.isin(got[0, 0], x[0][q[0] > 0]))
    # targets exactly at a cumulative weight c_k and at c_k + 1: the first returns element k, the second the next one
    order = np.argsort(x[0], kind="stable")
    cum = np.cumsum(q[0][order], dtype=np.uint64)
    ks = rng.choice(np.flatnonzero((q[0][order] > 0) & (cum < Q[0])), 20, replace=False)
    tgt = np.concatenate([cum[ks], cum[ks] + np.uint64(1)])[None, :]
    got = _check_select(x[:1], q, _q_dev(q), tgt, "dense")
    assert np.array_equal(got[0, 0, :20], x[0][order][ks]) and np.all(got[0, 0, 20:] > got[0, 0, :20])
    # above the total weight there is no element; a NaN in a value row answers every target of that row
    got = _select(x[:1], _q_dev(q), np.array([[int(Q[0]) + 1, int(Q[0])]], dtype=np.uint64), "dense")
    assert np.isnan(got[0, 0, 0]) and got[0, 0, 1] == x[0][q[0] > 0].max()
    xn = x.copy()
    xn[1, 7] = np.nan
    got = _select(xn, _q_dev(q), np.array([[1, int(Q[0])]], dtype=np.uint64), "chain")
    assert np.all(np.isnan(got[0, 1])) and np.all(np.isfinite(got[0, 0]))


# ---- 2. weighted histograms ---------------------------------------------------------------------------------------------------
def _box(d, rng):
    lo = rng.uniform(-2.0, 0.0, d)
    return lo, lo + rng.uniform(0.5, 3.0, d)


def _check_hist(x, q, lo, hi, nb1, nb2, group_bins=0):
    from gpemu import marginals as M
    from gpemu import reweight as R
    got = R.weighted_histograms(_dev(x), lo, hi, _q_dev(q), nb1, nb2, group_bins=group_bins)
    d = x.shape[1]
    assert got["hist_1d_q"].dtype == np.uint64 and got["hist_1d_q"].shape == (q.shape[0], d, nb1)
    assert got["hist_2d_q"].shape == (q.shape[0], d * (d - 1) // 2, nb2, nb2)
    assert np.array_equal(got["pairs"], M.pair_indices(d))
    for w in range(q.shape[0]):
        h1, h2, wi = RR.hist_ref(x, q[w], got["edges_1d"], got["edges_2d"])
        assert np.array_equal(got["hist_1d_q"][w], h1), np.argwhere(got["hist_1d_q"][w] != h1)[:5]
        assert np.array_equal(got["hist_2d_q"][w], h2), np.argwhere(got["hist_2d_q"][w] != h2)[:5]
        assert np.array_equal(got["w_inside"][w], wi)
    return got


# (S, d, nb1, nb2, R_w, group_bins): every d and bin count of the issue; one sweep (d = 1, 2), groups of whole pairs with
# the 1-D bins beside the last (5, 100, 50), sweeps of their own for the 1-D bins (4096 bins: four parameters a sweep),
# pairs in bands (256^2 bins: four bands a pair), and small group_bins that force more groups and bands on small shapes
HIST_SHAPES = [(65, 1, 1, 1, 1, 0), (2049, 2, 7, 7, 3, 0), (4097, 5, 100, 50, 2, 0), (257, 9, 4096, 256, 1, 0),
               (2049, 16, 100, 50, 1, 0), (63, 16, 7, 256, 1, 0), (2049, 5, 4096, 7, 2, 0), (2049, 5, 100, 50, 2, 5000),
               (2049, 9, 7, 50, 1, 50), (1, 2, 1, 1, 1, 0), (100003, 2, 100, 50, 1, 0)]


@pytest.mark.parametrize("S,d,nb1,nb2,R_w,group_bins", HIST_SHAPES)
def test_weighted_histograms_equal_numpy_on_every_shape(S, d, nb1, nb2, R_w, group_bins):
    rng = np.random.default_rng(S * 131 + d * 7 + nb1)
    lo, hi = _box(d, rng)
    x = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (S, d))      # a few per cent outside the box
    q, _, _ = _device_weights(R_w, S, S + d)
    _check_hist(x, q, lo, hi, nb1, nb2, group_bins)


def test_weighted_histograms_on_edges_outside_and_under_equal_weights():
    from gpemu import marginals as M
    rng = np.random.default_rng(9)
    S, d, nb = 2049, 3, 4
    lo, hi = np.array([-1.0, -2.0, 0.0]), np.array([1.0, 2.0, 3.0])
    e = M.bin_edges(lo, hi, nb)
    on_edge = np.stack([e[j][rng.integers(0, nb + 1, S)] for j in range(d)], axis=1)       # lo and hi included
    ulp = np.nextafter(on_edge, np.where(rng.random((S, d)) < 0.5, -np.inf, np.inf))
    outside = rng.uniform(lo - (hi - lo), hi + (hi - lo), (S, d))
    outside[0], outside[1] = lo, hi
    special = rng.uniform(lo, hi, (S, d))
    m = rng.random((S, d))
    special[m < 0.1], special[(m >= 0.1) & (m < 0.2)], special[(m >= 0.2) & (m < 0.3)] = np.nan, np.inf, -0.0
    q, Q, _ = _device_weights(2, S, 31)
    for x in (on_edge, ulp, outside, special):
        got = _check_hist(x, q, lo, hi, nb, nb)
    got = _check_hist(on_edge, q, lo, hi, nb, nb)
    assert np.all(got["w_inside"] == Q[:, None])
    # equal weights q_s = c: c times the counts of gpemu_marginal_hist
    for c in (1, 977, ONE // S):
        qc = np.full((1, S), c, dtype=np.uint64)
        got = _check_hist(outside, qc, lo, hi, 100, 50)
        cnt = M.histograms(outside, lo, hi, 100, 50)
        assert np.array_equal(got["hist_1d_q"][0], cnt["hist_1d"].astype(np.uint64) * np.uint64(c))
        assert np.array_equal(got["hist_2d_q"][0], cnt["hist_2d"].astype(np.uint64) * np.uint64(c))
        assert np.array_equal(got["w_inside"][0], cnt["n_inside"].astype(np.uint64) * np.uint64(c))
    # every sample in one bin: the worst case for the LDS atomics
    xs = np.full((100003, 2), 0.4)
    qs, Qs, _ = _device_weights(1, 100003, 33)
    got = _check_hist(xs, qs, np.zeros(2), np.ones(2), 100, 50)
    assert got["hist_1d_q"].max() == Qs[0] and got["hist_2d_q"].max() == Qs[0]


def test_weighted_summaries_read_a_thinned_view_in_place():
    from gpemu import marginals as M
    from gpemu import reweight as R
    rng = np.random.default_rng(5)
    steps, W, d = 61, 48, 8
    lo, hi = _box(d, rng)
    buf = rng.uniform(lo - 0.02, hi + 0.02, (steps, W, d))
    t = _dev(buf)
    e1, e2 = M.bin_edges(lo, hi, 100), M.bin_edges(lo, hi, 50)
    n_blocks = (steps + 2) // 3                      # thinned by 3: block_stride_rows = 3 W > block_rows = W
    rows = buf[::3].reshape(-1, d)
    q, Q, qd = _device_weights(2, rows.shape[0], 41)
    h1, h2, wi = R.weighted_hist_dev(0, t.data_ptr(), n_blocks, W, 3 * W, d, qd, e1, e2)
    for w in range(2):
        r1, r2, rw = RR.hist_ref(rows, q[w], e1, e2)
        assert np.array_equal(h1[w], r1) and np.array_equal(h2[w], r2) and np.array_equal(wi[w], rw)
    # the first half of the walkers of every step: one chain of a stacked sampler
    n2 = steps
    rows2 = buf[:, :W // 2].reshape(-1, d)
    q2, _, qd2 = _device_weights(1, rows2.shape[0], 43)
    h1, h2, wi = R.weighted_hist_dev(0, t.data_ptr(), n2, W // 2, W, d, qd2, e1, e2)
    r1, r2, rw = RR.hist_ref(rows2, q2[0], e1, e2)
    assert np.array_equal(h1[0], r1) and np.array_equal(h2[0], r2) and np.array_equal(wi[0], rw)


# ---- 3. the log-prior kernel ----------------------------------------------------------------------------------------------
def _prior_case(d, R, seed):
    """a box and R scenarios with all four kinds mixed.  Parameters alternate between a box below 1, a box above 1 and a
    box around 0 (kinds 0 and 2 only).  The log-normal kind goes to the boxes above 1 only: there -log x and the quadratic
    share a sign, which is what the bound's count of roundings per term assumes (below 1 the two parts of that term
    cancel and no multiple of |f_i| bounds the rounding of its parts)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.empty(d), np.empty(d)
    kind, a, b = np.zeros((R, d), dtype=np.int32), np.zeros((R, d)), np.ones((R, d))
    for i in range(d):
        lo[i], hi[i] = [(0.05, 0.9), (1.1, 30.0), (-3.0, 2.0)][i % 3]
        allowed = [(0, 1, 2), (0, 1, 2, 3), (0, 2)][i % 3]
        kind[:, i] = rng.choice(allowed, R)
    if d == 1:
        lo[0], hi[0] = 1.1, 30.0
        kind[:, 0] = rng.choice((0, 1, 2, 3), R)
        kind[:min(R, 4), 0] = np.arange(4)[:min(R, 4)][::-1]
    a[:] = rng.uniform(-1.0, 2.0, (R, d))
    b[:] = rng.uniform(0.3, 3.0, (R, d))
    return lo, hi, kind, a, b


@pytest.mark.parametrize("d", [1, 6, 9, 16])
@pytest.mark.parametrize("R", [1, 5, 64])
def test_log_prior_against_the_extended_precision_reference(d, R):
    """|L - L_ref| <= (d + 8) 2^-53 sum_i |f_i|: a 1-ulp fp64 log, at most 4 roundings per term, d - 1 additions"""
    from gpemu import reweight as Rw
    lo, hi, kind, a, b = _prior_case(d, R, 100 * d + R)
    rng = np.random.default_rng(d + R)
    steps, W = 23, 48
    buf = rng.uniform(lo, hi, (steps, W, d))
    t = _dev(buf)
    worst = 0.0
    views = {"dense": (1, steps * W, steps * W, buf.reshape(-1, d)), "thinned": ((steps + 2) // 3, W, 3 * W, buf[::3].reshape(-1, d)),
             "stacked": (steps, W // 2, W, buf[:, :W // 2].reshape(-1, d))}
    for name, (n_blocks, nw, stride, rows) in views.items():
        L = Rw.log_prior_dev(0, t.data_ptr(), n_blocks, nw, stride, d, (kind, a, b), lo).cpu().numpy()
        ref, A = RR.log_prior(rows, kind, a, b)
        assert L.shape == ref.shape
        err = np.abs(L.astype(np.longdouble) - ref).astype(np.float64)
        bound = (d + 8) * U * A.astype(np.float64)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst = max(worst, ratio)
        print(f"log-prior d = {d}, R = {R}, {name}: worst error / bound {ratio:.3f}")
        assert np.all(err <= bound), (name, ratio)
    # the host entry gives the same bits; a flat scenario is exactly 0
    spec = [[(int(k), float(x), float(y)) for k, x, y in zip(kr, ar, br)] for kr, ar, br in zip(kind, a, b)]
    host = Rw.log_ratio(buf.reshape(-1, d), priors=spec, lower=lo, upper=hi)
    dev = Rw.log_prior_dev(0, t.data_ptr(), 1, steps * W, steps * W, d, (kind, a, b), lo).cpu().numpy()
    assert host.tobytes() == dev.tobytes()
    flat = Rw.log_ratio(_dev(buf.reshape(-1, d)), priors=[[0] * d], lower=lo, upper=hi).cpu().numpy()
    assert np.all(flat == 0.0)


# ---- 4. quantisation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 255, 2049, 100003])
def test_fixed_point_weights(S):
    """|q - rint(expl(lw) 2^52)| <= 1 (a 1-ulp exp, an exact scaling by a power of two, one rint); Q is the integer sum"""
    from gpemu import reweight as R
    rng = np.random.default_rng(S)
    l = 3.0 * rng.normal(size=(3, S))
    l[1] = 0.0                                                  # equal weights
    if S > 1:
        l[2, 0] = -800.0                                        # exp underflows: weight 0
    _, lw = R.logmeanexp_dev(_dev(l), normalise=True)
    qd, Q = R.fixed_weights_dev(lw)
    q = qd.cpu().numpy().view(np.uint64)
    want = RR.quantise(lw.cpu().numpy())
    diff = np.abs(q.astype(np.int64) - want.astype(np.int64))
    print(f"S = {S}: largest |q - ref| {diff.max()}, Q - 2^52 = {[int(v) - ONE for v in Q]}")
    assert diff.max() <= 1
    assert [int(v) for v in Q] == [int(r.astype(object).sum()) for r in q]
    # normalised up to the roundings: every lw is off by at most 2 u (|l| + |lse|) and the tree's (depth + 4) u, every w
    # by one more u, every q by a half
    lse = np.abs(np.logaddexp.reduce(l, axis=1)).max()
    e = 2 * U * (np.abs(l).max() + lse) + (16 + 6 + 3 + (S + 4095) // 4096 + 5) * U
    assert all(abs(int(v) - ONE) <= ONE * e + S / 2 + 1 for v in Q)
    if S > 1:
        assert q[2, 0] == 0
    # the host form returns the same integers
    qh, Qh = R.fixed_weights(lw.cpu().numpy())
    assert qh.dtype == np.uint64 and np.array_equal(qh, q) and np.array_equal(Qh, Q)


# ---- 5. composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [63, 4097, 20000])
def test_weights_compose_psis_and_the_fixed_tree_log_sum_exp(S):
    from scipy.special import logsumexp
    from gpemu import loo
    from gpemu import reweight as R
    rng = np.random.default_rng(S)
    l = np.stack([rng.normal(size=S), 2.5 * rng.standard_t(3, size=S), -np.log(rng.uniform(0.05, 3.0, S)) + 700.0])
    dl = _dev(l)
    st = R.weights(dl)
    neg = -dl
    ps = loo.psis_dev(0, neg.data_ptr(), 3, S, S, 1, None, True)
    assert st["log_weights"].cpu().numpy().tobytes() == ps["log_weights"].cpu().numpy().tobytes()
    assert st["pareto_k"].tobytes() == ps["pareto_k"].tobytes() and st["ess_w"].tobytes() == ps["ess_w"].tobytes()
    host = R.weights(l)
    assert host["log_weights"].tobytes() == st["log_weights"].cpu().numpy().tobytes()
    assert host["log_mean_ratio"].tobytes() == st["log_mean_ratio"].tobytes()
    # log mean ratio: S positive terms (a 1-ulp exp of a rounded difference: 3 u each) through a fixed tree of depth
    # 16 + 6 + 3 + chunks additions, a 1-ulp log, the additions of the maximum and of log S (rounded itself)
    depth = 16 + 6 + 3 + (S + 4095) // 4096
    want = logsumexp(l.astype(np.longdouble), axis=1) - np.log(np.longdouble(S))
    err = np.abs(st["log_mean_ratio"].astype(np.longdouble) - want).astype(np.float64)
    bound = (depth + 3) * U + 4 * U * (np.abs(l).max(axis=1) + math.log(S) + np.abs(want.astype(np.float64)))
    print(f"S = {S}: log_mean_ratio error / bound {err / bound}")
    assert np.all(err <= bound)
    # smooth = False: l - logsumexp(l), from the same tree
    raw = R.weights(dl, smooth=False)
    lw = raw["log_weights"].cpu().numpy()
    lse = st["log_mean_ratio"] + math.log(S)
    assert np.all(np.abs(lw - (l - lse[:, None])) <= 4 * U * (np.abs(l) + np.abs(lse[:, None])))
    assert np.all(np.isnan(raw["pareto_k"])) and raw["log_mean_ratio"].tobytes() == st["log_mean_ratio"].tobytes()
    w = np.exp(lw.astype(np.longdouble))
    assert np.allclose(raw["ess_w"], (1.0 / (w * w).sum(axis=1)).astype(np.float64), rtol=1e-12)


# ---- 6. statistical truth ---------------------------------------------------------------------------------------------------
NEAR, FAR = (np.array([0.8, -0.6]), 2.0), (np.array([6.0, 6.0]), 1.0)


def _gaussian_case(a_off, b_scale, seed=2024):
    """x ~ N(m, s^2) in d = 2, S = 20000, reweighted to normal(a, b) priors with b = b_scale s, a = m + a_off s: the exact
    posterior is Gaussian with precision 1 / s^2 + 1 / b^2.  NEAR: b = 2 s, a within s of m.  FAR: a prior as narrow as
    the chain, 6 s away (with b = 2 s the reference's k-hat is 0.35 even there: such a wide prior hardly pulls)."""
    rng = np.random.default_rng(seed)
    m, s = np.array([0.7, -1.2]), np.array([0.5, 1.5])
    x = m + s * rng.normal(size=(20000, 2))
    a, b = m + a_off * s, b_scale * s
    var_post = 1.0 / (1.0 / s ** 2 + 1.0 / b ** 2)
    mean_post = var_post * (m / s ** 2 + a / b ** 2)
    lo, hi = m - 12 * s, m + 12 * s
    return x, [[("normal", a[0], b[0]), ("normal", a[1], b[1])]], lo, hi, mean_post, np.sqrt(var_post)


def test_statistical_truth_holds_in_the_reference_alone():
    """no device: the numpy reference (tests/loo_ref.py's smoothing) satisfies the assertions of the next test with the
    same seed -- k-hat -0.90 and 2.03 against the threshold 0.7"""
    import loo_ref as LR

    def ratios(case):
        x, spec, lo, hi, mean_post, sd_post = _gaussian_case(*case)
        (_, a0, b0), (_, a1, b1) = spec[0]
        return x, -(x[:, 0] - a0) ** 2 / (2 * b0 ** 2) - (x[:, 1] - a1) ** 2 / (2 * b1 ** 2), mean_post, sd_post
    x, l, mean_post, sd_post = ratios(NEAR)
    out = LR.psis_row(-l)
    w = np.exp(np.asarray(out["logw"], dtype=np.float64))
    ess = 1.0 / np.sum(w * w)
    assert np.all(np.abs(w @ x / w.sum() - mean_post) <= 5 * sd_post / math.sqrt(ess)), (w @ x, mean_post, ess)
    assert float(out["pareto_k"]) < LR.k_threshold(20000)
    assert float(LR.psis_row(-ratios(FAR)[1])["pareto_k"]) > LR.k_threshold(20000)


def test_statistical_truth_of_a_gaussian_reweighted_to_gaussian_priors():
    from gpemu import loo
    from gpemu import reweight as R
    x, spec, lo, hi, mean_post, sd_post = _gaussian_case(*NEAR)
    L = R.log_ratio(_dev(x), priors=spec, lower=lo, upper=hi)
    out = R.summary(_dev(x), L, lo, hi, bins_1d=100, bins_2d=50)[0]
    print(f"near prior: pareto_k {out['pareto_k']:.3f}, ess_w {out['ess_w']:.0f}, mean {out['mean']}, exact {mean_post}, "
          f"sd {out['sd']}, exact {sd_post}")
    assert out["k_threshold"] == loo.k_threshold(20000) and out["pareto_k"] < out["k_threshold"] and out["reliable"]
    assert np.all(np.abs(out["mean"] - mean_post) <= 5 * sd_post / math.sqrt(out["ess_w"]))
    assert out["quantiles"].shape == (3, 2) and np.all(np.diff(out["quantiles"], axis=0) > 0)
    assert out["hist_1d"].dtype == np.float64 and np.all(out["hist_1d_q"].sum(axis=1) <= out["Q"])
    assert np.array_equal(out["hist_1d"], out["hist_1d_q"].astype(np.float64) / out["Q"])
    # the prior 6 s away: the tail of the ratios is too heavy for this chain
    x, spec, lo, hi, _, _ = _gaussian_case(*FAR)
    L = R.log_ratio(_dev(x), priors=spec, lower=lo, upper=hi)
    far = R.summary(_dev(x), L, lo, hi)[0]
    print(f"far prior: pareto_k {far['pareto_k']:.3f}, ess_w {far['ess_w']:.1f}")
    assert far["reliable"] is False and far["pareto_k"] > far["k_threshold"]


def test_summary_equals_the_reference_from_the_devices_weights_and_the_host_entries():
    from gpemu import reweight as R
    rng = np.random.default_rng(8)
    S, d = 4097, 5
    lo, hi = np.full(d, 0.05), np.array([3.0, 10.0, 1.5, 100.0, 2.0])
    base = rng.uniform(lo, hi, (S // 3, d))
    x = base[rng.integers(0, base.shape[0], S)]                 # repeated rows, as a chain has
    spec = [R.reference_prior(["a", "c_1", "c_2", "b", "c_3"]), {0: ("normal", 1.0, 0.8), 3: ("log_normal", 2.0, 1.0)}]
    tables = R.check_priors(spec, d, lo, hi)
    log_norm = R.log_prior_norm(*tables, lo, hi)
    L = R.log_ratio(_dev(x), priors=spec, lower=lo, upper=hi)
    dev = R.summary(_dev(x), L, lo, hi, bins_1d=100, bins_2d=50, log_norm=log_norm)
    host = R.summary(x, L.cpu().numpy(), lo, hi, bins_1d=100, bins_2d=50, log_norm=log_norm)
    st = R.weights(L)
    qd, Q = R.fixed_weights_dev(st["log_weights"])
    q = qd.cpu().numpy().view(np.uint64)
    for r, (a, b) in enumerate(zip(dev, host)):
        for key in ("pareto_k", "ess_w", "log_mean_ratio", "log_evidence_ratio", "Q"):
            assert a[key] == b[key], key
        for key in ("mean", "sd", "quantiles", "hist_1d_q", "hist_2d_q", "hist_1d", "hist_2d", "shift"):
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
        assert a["Q"] == int(Q[r])
        for j in range(d):
            assert np.array_equal(a["quantiles"][:, j], RR.weighted_quantile(x[:, j], q[r], (0.05, 0.5, 0.95)))
        h1, h2, _ = RR.hist_ref(x, q[r], a["edges_1d"], a["edges_2d"])
        assert np.array_equal(a["hist_1d_q"], h1) and np.array_equal(a["hist_2d_q"], h2)
        mean, var = RR.moments(x, q[r])
        assert np.allclose(a["mean"], mean, rtol=1e-10) and np.allclose(a["sd"], np.sqrt(var), rtol=1e-8)
        assert np.allclose(a["shift"], (a["mean"] - x.mean(axis=0)) / x.std(axis=0), rtol=0, atol=1e-10)
        assert a["log_evidence_ratio"] == a["log_mean_ratio"] + float(np.sum(np.log(hi - lo))) - log_norm[r]
    assert dev[0]["log_mean_ratio"] != dev[1]["log_mean_ratio"]


# ---- 7. arguments and paths -------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    from gpemu import _lib
    from gpemu import reweight as R
    L = _lib.lib()
    S, d = 64, 2
    x = _dev(np.random.default_rng(0).uniform(0.5, 2.0, (S, d)))
    out = _dev(np.zeros((2, S)))
    qd = _q_dev(np.ones((1, S), dtype=np.uint64))
    kind, a, b = np.array([[1, 2]], dtype=np.int32), np.zeros((1, 2)), np.ones((1, 2))
    lo, e = np.array([0.5, 0.5]), np.array([[0.0, 1.0, 2.0]] * 2)
    before = R.path_counts()
    P = _lib.ptr
    V = lambda t: C.c_void_p(t.data_ptr())

    def logprior(d_=d, R_=1, kind_=kind, a_=a, b_=b, lo_=lo, ldl=S):
        return L.gpemu_logprior_dev(0, V(x), 1, S, S, d_, R_, P(kind_), P(a_), P(b_), P(lo_), V(out), ldl, None)
    assert logprior(d_=0) == -1 and logprior(d_=17) == -1 and logprior(R_=0) == -1 and logprior(R_=65) == -1
    assert logprior(kind_=np.array([[4, 0]], dtype=np.int32)) == -1
    assert logprior(lo_=np.array([0.0, 0.5])) == -1                        # log-uniform with a lower bound of 0
    assert logprior(b_=np.array([[1.0, 0.0]])) == -1 and logprior(b_=np.array([[1.0, -1.0]])) == -1
    assert logprior(a_=np.array([[0.0, np.nan]])) == -1 and logprior(b_=np.array([[1.0, np.inf]])) == -1
    assert logprior(ldl=S - 1) == -1
    assert "lower bound" in _lib.last_error() or "ldl" in _lib.last_error()
    assert L.gpemu_logmeanexp_dev(0, 0, S, V(out), S, V(out), None, None) == -1
    assert L.gpemu_logmeanexp_dev(0, 1, S, V(out), S - 1, V(out), None, None) == -1
    assert L.gpemu_weights_fixed_dev(0, 1, 0, V(out), S, V(qd), S, V(qd), None) == -1
    assert L.gpemu_weights_fixed_dev(0, 1, S, V(out), S, V(qd), S - 1, V(qd), None) == -1
    t1 = np.array([1], dtype=np.uint64)

    def select(R_v=d, S_=S, rs=1, es=d, R_w=1, ldq=S, nt=1, t=t1, ws=0):
        return L.gpemu_weighted_select_dev(0, R_v, S_, V(x), rs, es, R_w, V(qd), ldq, nt, P(t), V(out), ws, None)
    assert select(R_v=0) == -1 and select(S_=0) == -1 and select(rs=0) == -1 and select(es=0) == -1 and select(R_w=0) == -1
    assert select(ldq=S - 1) == -1 and select(nt=0) == -1 and select(ws=-1) == -1
    assert select(t=np.array([0], dtype=np.uint64)) == -1                  # a target below 1
    assert select(t=np.array([(1 << 53) + 1], dtype=np.uint64)) == -1
    h = _dev(np.zeros(64, dtype=np.int64))

    def hist(d_=d, R_w=1, ldq=S, nb1=2, e1=e, nb2=2, e2=e, gb=0):
        return L.gpemu_weighted_hist_dev(0, V(x), 1, S, S, d_, R_w, V(qd), ldq, nb1, P(e1), nb2, P(e2), gb, V(h), V(h),
                                         V(h), None)
    assert hist(d_=17) == -1 and hist(R_w=0) == -1 and hist(ldq=S - 1) == -1 and hist(nb1=0) == -1 and hist(nb1=4097) == -1
    assert hist(nb2=0) == -1 and hist(nb2=257) == -1 and hist(gb=1) == -1 and hist(gb=18433) == -1
    assert hist(e1=np.array([[0.0, 1.0, 1.0]] * 2)) == -1 and hist(e2=np.array([[0.0, np.inf, 2.0]] * 2)) == -1
    assert R.path_counts() == before
    for bad in (dict(priors=[[1, 1]], lower=[0.0, 0.5], upper=[2, 2]), dict(priors=[[("normal", 0, 0), 0]], lower=lo, upper=[2, 2]),
                dict(priors=[[{"kind": "flat", "lower": 1.0}, 0]], lower=lo, upper=[2, 2]), dict(priors=None)):
        with pytest.raises(ValueError):
            R.log_ratio(x, **bad)
    assert R.path_counts() == before


def test_every_path_ran(counters_at_start):
    """last in the file: every member of gpemu_reweight_path_counts increased over the file's run (one small call of each
    first, so that the test also stands alone)"""
    from gpemu import reweight as R
    x = np.random.default_rng(0).uniform(0.5, 2.0, (65, 2))
    out = R.summary(_dev(x), R.log_ratio(_dev(x), priors=[[1, 2 * 0]], lower=[0.5, 0.5], upper=[2.0, 2.0]), [0.5, 0.5], [2.0, 2.0],
                    bins_1d=4, bins_2d=3)
    assert out[0]["Q"] > 0
    now = R.path_counts()
    print({k: now[k] - counters_at_start[k] for k in now})
    assert set(now) == set(R.PATHS)
    for k in R.PATHS:
        assert now[k] > counters_at_start[k], k
