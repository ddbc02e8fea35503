"""-m gpu tests of the k-th neighbour information estimators (csrc/k_knn.hip, gpemu/information.py)
against the numpy reference tests/information_ref.py, through the C ABI and the module.

Tolerances (derived, not tuned), d_p the coordinates of the subset, n the rows:
* r2 against the longdouble reference: |delta| <= (d_p + 3) 2^-52 r2 -- one rounding per difference (2 ulp in its
  square), non-negative terms in an fma chain (one rounding each, d_p in all), the reference's own rounding to float64;
* zeros, n_used, n_short, copies: exact;
* sum log r2: |delta| <= 2^-52 (n (d_p + 3) + (log2 n + 2) sum |log r2_i|) -- the distances' error through the log, one
  ulp of every log, and a tree of depth log2 n;
* unit-box rows: the bits of numpy's expression;
* an estimate: (d_p / 2) / n_used of the sum's bound, plus 8 ulp of the magnitudes of its four terms (psi(N), psi(k),
  log c_d from two libraries, the products and the sum)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import information_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _I():
    from gpemu import information as I
    return I


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _subsets_for(d):
    if d == 6:
        return R.default_subsets(6)
    subs = [tuple(range(d)), (d - 1,)]
    if d >= 8:
        subs += [(0, d - 1), (1, 3, 6), (0, 2, 3, 5, 7)]
    if d == 9:
        subs += [(0, 1, 2, 4, 5, 6, 8)]
    if d == 16:
        subs += [(0, 3, 7, 12, 15), tuple(range(0, 16, 2)) + (1, 5), tuple(range(13)), tuple(range(2, 16))]
    return subs


def _check_r2(r2, zeros, ref_r2, ref_zeros, subsets):
    assert np.array_equal(zeros, ref_zeros)
    for p, s in enumerate(subsets):
        want = ref_r2[p].astype(np.float64)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(r2[p]), np.isnan(want)) and np.array_equal(np.isinf(r2[p]), np.isinf(want)), s
        err = np.abs(r2[p][fin].astype(R.LD) - ref_r2[p][fin])
        assert np.all(err <= (len(s) + 3) * EPS * ref_r2[p][fin]), (s, float(err.max()))


def _check_sums(r2_dev, zeros_dev, ref_r2, ref_zeros, subsets, nu2_dev=None, ref_nu2=None):
    I = _I()
    counts, sums = I.logsum_dev(0, r2_dev, zeros_dev, nu2_dev)
    rc, rs, rabs = R.log_sums(ref_r2, ref_zeros, ref_nu2)
    assert np.array_equal(counts, rc)
    n = ref_r2.shape[1]
    for p, s in enumerate(subsets):
        bound = EPS * (n * (len(s) + 3) * (1 if ref_nu2 is None else 2) + (math.log2(n) + 2) * float(rabs[p]))
        assert abs(R.LD(sums[p, 0]) - rs[p, 0]) <= bound, (s, float(sums[p, 0]), float(rs[p, 0]), bound)
        # the squares: each v carries the bound's relative share; 2 |v| delta v summed, and the tree
        v_max = float(np.sqrt(rs[p, 1])) + 1.0
        assert abs(R.LD(sums[p, 1]) - rs[p, 1]) <= 2.0 * v_max * bound + EPS * (math.log2(n) + 2) * float(rs[p, 1])
    return counts, sums


@functools.lru_cache(maxsize=None)
def _case(nq, d, k, seed=0):
    u = np.random.default_rng(1000 * d + nq + seed).random((nq, d))
    subs = _subsets_for(d)
    return (u, subs) + R.knn(u, None, k, subs)


@pytest.mark.parametrize("nq,d,k", [(1, 1, 1), (4, 6, 4), (5, 6, 4), (16, 8, 16), (17, 9, 16), (255, 6, 4), (256, 8, 5),
                                    (257, 9, 1), (1000, 16, 16), (1000, 6, 4), (1000, 1, 5)])
def test_self_search_against_the_reference(nq, d, k):
    """The host entry and the device entry give the same bits, within the derived bound of the reference; nq = k leaves
    every row short (+inf), nq = k + 1 none."""
    I = _I()
    u, subs, ref_r2, ref_zeros = _case(nq, d, k)
    r2, zeros = I.knn_distances(u, k=k, subsets=subs)
    assert r2.shape == zeros.shape == (len(subs), nq) and zeros.dtype == np.int32
    _check_r2(r2, zeros, ref_r2, ref_zeros, subs)
    assert np.all(np.isinf(r2)) == (nq <= k)
    dr2, dzeros = I.knn_distances(_dev(u), k=k, subsets=subs)
    assert dr2.cpu().numpy().tobytes() == r2.tobytes() and dzeros.cpu().numpy().tobytes() == zeros.tobytes()
    counts, _ = _check_sums(dr2, dzeros, ref_r2, ref_zeros, subs)
    assert np.all(counts[:, 0] + counts[:, 1] == nq) and np.all(counts[:, 2] == nq)
    assert np.all(counts[:, 1] == (nq if nq <= k else 0))


@pytest.mark.parametrize("nr", [255, 256, 257, 513])
@pytest.mark.parametrize("k", [4, 5])
def test_cross_search_around_the_reference_tile(nr, k):
    """nr one below, at and one above the LDS tile (and two tiles and one), nr != nq, UQ != UR: no copies."""
    I = _I()
    assert I.REF_TILE == 256
    rng = np.random.default_rng(nr)
    uq, ur = rng.random((100, 3)), rng.random((nr, 3))
    subs = R.default_subsets(3)
    ref_r2, ref_zeros = R.knn(uq, ur, k, subs)
    r2, zeros = I.knn_distances(uq, ur, k=k, subsets=subs)
    assert not zeros.any()
    _check_r2(r2, zeros, ref_r2, ref_zeros, subs)
    dr2, dzeros = I.knn_distances(_dev(uq), _dev(ur), k=k, subsets=subs)
    assert dr2.cpu().numpy().tobytes() == r2.tobytes() and not dzeros.cpu().numpy().any()


@pytest.mark.parametrize("nq,d,k", [(1000, 6, 4), (1000, 16, 16), (5, 6, 4), (257, 9, 1)])
def test_every_split_gives_the_same_bits(nq, d, k):
    """Z forced to 1, 2, 3 and 7 (and chosen by the library): r2 and zeros bit for bit -- the k smallest of a set do not
    depend on its order; with 5 references some of 7 splits are empty."""
    I = _I()
    u, subs, _, _ = _case(nq, d, k)
    du = _dev(u)
    base = None
    for z in (1, 2, 3, 7, 0):
        c0 = I.path_counts()
        r2, zeros = I.knn_distances(du, k=k, subsets=subs, splits=z)
        c1 = I.path_counts()
        got = (r2.cpu().numpy().tobytes(), zeros.cpu().numpy().tobytes())
        base = got if base is None else base
        assert got == base, z
        if z > 1:
            assert c1["MERGE"] - c0["MERGE"] == c1["SEARCH"] - c0["SEARCH"] > 0
        if z == 1:
            assert c1["MERGE"] == c0["MERGE"]
    h2, hz = I.knn_distances(u, k=k, subsets=subs, splits=3)          # the host entry takes the argument too
    assert (h2.tobytes(), hz.tobytes()) == base


def test_copies_are_counted_and_are_no_neighbours():
    """Every third row repeated twice, interleaved with the rest: zeros and r2 equal the reference's, the copies are the
    known count, and the module refuses the rows unless told to allow them."""
    I = _I()
    rng = np.random.default_rng(7)
    base = rng.random((300, 3))
    x = np.concatenate([base, base[::3], base[::3]])[rng.permutation(500)]
    subs = R.default_subsets(3)
    ref_r2, ref_zeros = R.knn(x, None, 4, subs)
    assert sorted(np.unique(ref_zeros[-1]).tolist()) == [1, 3]
    r2, zeros = I.knn_distances(x, k=4, subsets=subs)
    _check_r2(r2, zeros, ref_r2, ref_zeros, subs)
    lo, hi = np.zeros(3), np.ones(3)
    with pytest.raises(ValueError, match="thin the chain by its autocorrelation time"):
        I.information_gain(x, lo, hi)
    out = I.information_gain(x, lo, hi, allow_copies=True)
    assert out["n_points"] == 500 and np.all(out["copies"] == 100 * 3 * 2) and np.all(out["n_used"] == 500)
    ref = R.information_gain(x, lo, hi)
    assert np.array_equal(out["copies"], ref["copies"])
    with pytest.raises(ValueError, match="fewer than k = 16 distinct neighbours"):
        I.information_gain(x[:12], lo, hi, k=16, allow_copies=True)


def test_ties_among_neighbours_on_a_lattice():
    """Points on a lattice: many references at exactly the k-th distance.  Which of them the list keeps does not change
    the k-th value."""
    I = _I()
    g = np.arange(9) / 8.0
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[np.random.default_rng(3).permutation(729)]
    subs = [(0, 1, 2), (0, 2), (1,)]
    for k in (1, 4, 6, 7):
        ref_r2, ref_zeros = R.knn(x, None, k, subs)
        for splits in (0, 3):
            r2, zeros = I.knn_distances(x, k=k, subsets=subs, splits=splits)
            assert np.array_equal(zeros, ref_zeros) and np.array_equal(r2, ref_r2.astype(np.float64))
    c = int(np.flatnonzero(np.all(x == 0.5, axis=1))[0])          # the centre, k = 7: past its 6 face neighbours
    assert ref_zeros[1, c] == 9 and ref_zeros[2, c] == 81 and ref_r2[0, c] == 2.0 / 64.0


def test_a_row_with_nan_is_counted_and_passed_over():
    import torch
    I = _I()
    rng = np.random.default_rng(11)
    x = rng.uniform(-2.0, 3.0, (400, 4))
    x[17, 2] = np.nan
    x[250, 0] = np.inf
    lo, hi = np.full(4, -2.0), np.full(4, 3.0)
    dx = _dev(x)
    U, skipped = I.unit_rows_dev(0, dx.data_ptr(), 1, 400, 400, 4, lo, hi, 400)
    uref, sref = R.unit_rows(x, lo, hi)
    assert skipped == sref == 2 and U.cpu().numpy().tobytes() == uref.tobytes()
    assert torch.isnan(U[17]).all() and torch.isnan(U[250]).all()
    subs = R.default_subsets(4)
    ref_r2, ref_zeros = R.knn(uref, None, 4, subs)
    r2, zeros = I.knn_distances(U, k=4, subsets=subs)
    r2, zeros = r2.cpu().numpy(), zeros.cpu().numpy()
    _check_r2(r2, zeros, ref_r2, ref_zeros, subs)
    assert np.all(np.isnan(r2[:, [17, 250]])) and not zeros[:, [17, 250]].any() and np.isfinite(np.delete(r2, [17, 250], 1)).all()
    for rows in (x, dx):
        out = I.information_gain(rows, lo, hi)
        assert out["n_points"] == 398 and np.all(out["n_used"] == 398) and not out["copies"].any()
    # a NaN in one coordinate of a row given as it is: only the subsets that hold the coordinate pass the row over
    u = uref.copy()
    u[17] = rng.random(4)
    u[17, 2] = np.nan
    ref_r2, ref_zeros = R.knn(u, None, 4, subs)
    r2, zeros = I.knn_distances(u, k=4, subsets=subs)
    _check_r2(r2, zeros, ref_r2, ref_zeros, subs)
    assert [bool(np.isnan(r2[p, 17])) for p in range(len(subs))] == [2 in s for s in subs]


@pytest.mark.parametrize("discard,thin,chain", [(0, 1, 0), (3, 1, 1), (5, 3, 1)])
def test_views_of_a_stored_chain_equal_the_dense_copy(discard, thin, chain):
    """A thinned and a stacked-chain view of a short DeviceSampler run against the module function on the dense copy of
    the same rows: bit for bit."""
    from test_gpu_row_views import WC, _stacked
    I = _I()
    s, dm, full, lo, hi = _stacked()
    d = lo.size
    rows = np.ascontiguousarray(full[discard::thin][:, chain * WC:(chain + 1) * WC]).reshape(-1, d)
    kw = dict(k=2, allow_copies=True, subsets=[(0,), (2, 5), tuple(range(d))])
    got = s.information_gain(discard=discard, thin=thin, chain=chain, **kw)
    for want in (I.information_gain(rows, lo, hi, **kw), I.information_gain(_dev(rows), lo, hi, **kw)):
        assert got["subsets"] == want["subsets"] and got["n_points"] == want["n_points"] == rows.shape[0]
        for key in ("nats", "bits", "se", "n_used", "copies", "per_parameter", "per_pair", "pairs", "dims"):
            assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
        assert got["joint"] == want["joint"] and np.isfinite(got["joint"])
    assert got["copies"].min() > 0                  # an ensemble chain repeats states
    with pytest.raises(ValueError, match="thin the chain"):
        s.information_gain(discard=discard, thin=thin, chain=chain, k=2)
    # the divergence of the chain from itself thinned, from the other chain and from rows on the host
    other = np.ascontiguousarray(full[discard::thin][:, (1 - chain) * WC:(2 - chain) * WC]).reshape(-1, d)
    got = s.kl_divergence(s, discard=discard, thin=thin, chain=chain, other_chain=1 - chain, **kw)
    for want in (I.kl_divergence(rows, other, lo, hi, **kw), s.kl_divergence(other, discard=discard, thin=thin, chain=chain, **kw)):
        for key in ("nats", "se", "n_used", "copies"):
            assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
        assert got["m_points"] == want["m_points"] == other.shape[0]


def test_a_block_stride_that_is_no_multiple_of_d():
    """Steps padded to 14 doubles, 4 walkers of d = 3 (tests/test_gpu_row_views.py): walkers [1, 4) of every second step."""
    I = _I()
    n, stride, d = 16, 14, 3
    x = np.random.default_rng(5).normal(size=(n, 4, d))
    padded = np.full((n, stride), np.nan)
    padded[:, :4 * d] = x.reshape(n, 4 * d)
    dev = _dev(padded)
    lo, hi = np.full(d, -5.0), np.full(d, 5.0)
    U, skipped = I.unit_rows_dev(0, dev.data_ptr() + 8 * d, 8, 3, None, d, lo, hi, 10 ** 6, block_stride=2 * stride)
    want, _ = R.unit_rows(np.ascontiguousarray(x[::2, 1:4]).reshape(-1, d), lo, hi)
    assert skipped == 0 and U.shape == (24, d) and U.cpu().numpy().tobytes() == want.tobytes()


def test_max_points_selects_the_documented_rows():
    I = _I()
    rng = np.random.default_rng(13)
    x = rng.uniform(0.0, 2.0, (1000, 2))
    lo, hi = np.zeros(2), np.full(2, 2.0)
    dx = _dev(x)
    for n in (1, 7, 333, 1000, 5000):
        sel = R.selected_rows(1000, n)
        assert sel.size == min(n, 1000) and sel[0] == 0 and np.all(np.diff(sel) >= 1)
        U, skipped = I.unit_rows_dev(0, dx.data_ptr(), 1, 1000, 1000, 2, lo, hi, n)
        assert skipped == 0 and U.cpu().numpy().tobytes() == ((x[sel] - lo) * (1.0 / (hi - lo))).tobytes()
    out = I.information_gain(dx, lo, hi, max_points=333, subsets=[(0, 1)])
    ref = I.information_gain(x[R.selected_rows(1000, 333)], lo, hi, subsets=[(0, 1)])
    assert out["n_points"] == 333 and out["nats"].tobytes() == ref["nats"].tobytes()


def test_path_counters_move_as_documented():
    I = _I()
    u = _dev(np.random.default_rng(2).random((600, 6)))
    _, masks = I.check_subsets(None, 6)                             # widths 1, 2 and 6: three launches
    c0 = I.path_counts()
    r2, zeros = I.knn_dist_dev(0, u, None, masks, 4, splits=1)
    c1 = I.path_counts()
    assert {k: c1[k] - c0[k] for k in I.PATHS} == {"UNIT_ROWS": 0, "SEARCH": 3, "MERGE": 0, "SUBSET_BATCH": 3, "LOGSUM": 0}
    # two splits whose lists hold one subset at a time: a batch, a search and a merge per subset
    per_list = (8 * 4 + 4) * 600
    b2, bz = I.knn_dist_dev(0, u, None, masks, 4, splits=2, workspace_bytes=2 * per_list)
    c2 = I.path_counts()
    assert {k: c2[k] - c1[k] for k in I.PATHS} == {"UNIT_ROWS": 0, "SEARCH": 22, "MERGE": 22, "SUBSET_BATCH": 22, "LOGSUM": 0}
    assert b2.cpu().numpy().tobytes() == r2.cpu().numpy().tobytes() and bz.cpu().numpy().tobytes() == zeros.cpu().numpy().tobytes()
    with pytest.raises(Exception, match="out of memory"):
        I.knn_dist_dev(0, u, None, masks, 4, splits=2, workspace_bytes=per_list)
    assert I.path_counts() == c2
    I.logsum_dev(0, r2, zeros)
    I.unit_rows_dev(0, u.data_ptr(), 1, 600, 600, 6, np.zeros(6), np.ones(6), 600)
    c3 = I.path_counts()
    assert {k: c3[k] - c2[k] for k in I.PATHS} == {"UNIT_ROWS": 1, "SEARCH": 0, "MERGE": 0, "SUBSET_BATCH": 0, "LOGSUM": 1}


def test_argument_errors_return_before_any_launch():
    from gpemu import _lib
    from gpemu._lib import ptr
    I = _I()
    L = _lib.lib()
    u = np.random.default_rng(1).random((32, 4))
    r2, zeros = np.empty((2, 32)), np.empty((2, 32), dtype=np.int32)

    def call(d=4, k=4, masks=(3, 8), nq=32, nr=32, splits=0, ws=0):
        m = np.array(masks, dtype=np.uint32)
        return L.gpemu_knn_dist(0, nq, nr, d, ptr(u), None, m.size, ptr(m), k, splits, ws, ptr(r2), ptr(zeros))

    assert call() == 0, _lib.last_error()
    c0 = I.path_counts()
    bad = [dict(k=0), dict(k=17), dict(masks=(3, 0)), dict(masks=(3, 16)), dict(masks=(1 << 31,)), dict(d=17), dict(d=0),
           dict(nq=0), dict(nr=0), dict(nr=31), dict(splits=-1), dict(splits=65), dict(ws=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw                                    # GPEMU_ERR_ARG
        assert "bad argument" in _lib.last_error(), kw
    du, dr2, dz = _dev(u), _dev(r2), _dev(zeros)
    m = np.array([3], dtype=np.uint32)
    for k, d in ((0, 4), (17, 4), (4, 17)):
        assert L.gpemu_knn_dist_dev(0, 32, 32, d, C.c_void_p(du.data_ptr()), None, 1, ptr(m), k, 0, 0,
                                    C.c_void_p(dr2.data_ptr()), C.c_void_p(dz.data_ptr()), None) == -1
    skipped = C.c_int64(0)
    lo, hi = np.zeros(4), np.ones(4)
    for d, lower, n in ((17, lo, 32), (4, hi, 32), (4, lo, 33), (4, lo, 0)):
        assert L.gpemu_unit_rows_dev(0, C.c_void_p(du.data_ptr()), 1, 32, 32 * 4, d, ptr(lower), ptr(hi), n,
                                     C.c_void_p(dr2.data_ptr()), C.byref(skipped), None) == -1
    assert I.path_counts() == c0


def _estimate_bound(subs, n_used, sabs, n, terms, two=False):
    """the module's estimate against the reference's: (d_p / 2) / n_used of the sum's bound plus 8 ulp of the terms"""
    out = []
    for p, s in enumerate(subs):
        bsum = EPS * (n * (len(s) + 3) * (2 if two else 1) + (math.log2(n) + 2) * float(sabs[p]))
        out.append(0.5 * len(s) / n_used * bsum + 8 * EPS * float(np.sum(np.abs(terms[p]))))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _gauss_reference():
    x = 0.5 + 0.05 * np.random.default_rng(0).standard_normal((4096, 3))
    y = 0.52 + 0.07 * np.random.default_rng(1).standard_normal((4096, 3))
    subs = [(0, 1, 2), (1,)]
    lo, hi = np.zeros(3), np.ones(3)
    rho2, zeros = R.knn(x, None, 4, subs)                         # (the box is the unit box: u = x, bit for bit)
    nu2, _ = R.knn(x, y, 4, subs)
    H, se = R.entropy_from(rho2, subs, 4, 4096)
    nats, kse = R.divergence_from(rho2, nu2, subs, 4096, 4096)
    return (x, y, subs, lo, hi, {"nats": -H, "se": se, "r2": rho2, "zeros": zeros},
            {"nats": nats, "se": kse, "rho2": rho2, "nu2": nu2})


def test_information_gain_of_the_gaussian_equals_the_references_estimate():
    """x = 0.5 + 0.05 N(0, I), d = 3, n = 4096, k = 4: the module's estimate (host rows and device rows, the same bits)
    against the reference's brute force, to the derived tolerance.  That the estimate is near the analytic value is
    tests/test_information_host.py's business."""
    from scipy.special import digamma
    I = _I()
    x, _, subs, lo, hi, ref, _ = _gauss_reference()
    out = I.information_gain(x, lo, hi, subsets=subs)
    dev = I.information_gain(_dev(x), lo, hi, subsets=subs)
    for key in ("nats", "se", "n_used", "copies"):
        assert np.asarray(out[key]).tobytes() == np.asarray(dev[key]).tobytes(), key
    _, _, sabs = R.log_sums(ref["r2"])
    terms = [[digamma(4096), digamma(4), R.log_unit_ball(len(s)), ref["nats"][p]] for p, s in enumerate(subs)]
    bound = _estimate_bound(subs, 4096, sabs, 4096, terms)
    print("gain", out["nats"], ref["nats"], np.abs(out["nats"] - ref["nats"]), bound)
    assert np.all(np.abs(out["nats"] - ref["nats"]) <= bound)
    assert np.allclose(out["se"], ref["se"], rtol=1e-9, atol=0)       # a difference of sums of squares: not a bound
    assert out["joint"] == out["nats"][0] and out["per_parameter"][1] == out["nats"][1] and np.isnan(out["per_parameter"][0])
    assert np.allclose(out["bits"], out["nats"] / math.log(2.0), rtol=4 * EPS, atol=0)
    assert abs(out["joint"] - R.gaussian_gain(3, 0.05)) <= max(4 * out["se"][0], 0.1)


def test_kl_divergence_of_two_gaussians_equals_the_references_estimate():
    I = _I()
    x, y, subs, lo, hi, _, ref = _gauss_reference()
    out = I.kl_divergence(x, y, lo, hi, subsets=subs)
    dev = I.kl_divergence(_dev(x), _dev(y), lo, hi, subsets=subs)
    for key in ("nats", "se", "n_used", "copies"):
        assert np.asarray(out[key]).tobytes() == np.asarray(dev[key]).tobytes(), key
    _, _, sabs = R.log_sums(ref["rho2"], None, ref["nu2"])
    terms = [[math.log(4096 / 4095.0), ref["nats"][p]] for p in range(len(subs))]
    bound = _estimate_bound(subs, 4096, sabs, 4096, terms, two=True)
    print("kl", out["nats"], ref["nats"], np.abs(out["nats"] - ref["nats"]), bound)
    assert np.all(np.abs(out["nats"] - ref["nats"]) <= bound)
    assert out["n_points"] == out["m_points"] == 4096
    assert abs(out["joint"] - R.gaussian_kl(3, 0.05, 0.07, 0.02)) <= max(4 * out["se"][0], 0.1)
    # a derived quantity against samples of its prior, as 1-column arrays, in their own coordinates
    one = I.kl_divergence(x[:, 0], y[:, 0], subsets=[(0,)])
    r1 = R.kl_divergence(x[:, :1], y[:, :1], np.zeros(1), np.ones(1), subsets=[(0,)])
    _, _, sabs = R.log_sums(r1["rho2"], None, r1["nu2"])
    assert abs(one["nats"][0] - r1["nats"][0]) <= _estimate_bound([(0,)], 4096, sabs, 4096, [[1e-3, r1["nats"][0]]], two=True)[0]
