"""-m gpu tests that the counted and the weighted form of the radix select (k_select.hip) and of the histogram sweep
(k_marginal.hip) are one algorithm: gpemu_select_dev against gpemu_weighted_select_dev under unit
weights and targets rank + 1, gpemu_marginal_hist_dev against gpemu_weighted_hist_dev under the constant weight 3, and
both against numpy, at the smallest shapes where merging the two copies could go wrong.

Every comparison is == on integers or on the bits of doubles (on values where -0 and +0 are tied); nothing is skipped or
compared within a tolerance.

Not covered: the 16-bit counters' row cap (at most 65280 rows per workgroup of a counted sweep) binds only above
1024 x 65280 = 6.7e7 rows, far beyond a quick test, and stays uncovered as before."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN_BITS = np.uint64(0x7FF8000000000000)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. select ------------------------------------------------------------------------------------------------------------
def _select_both(t, off, R, S, row_stride, elem_stride, ranks):
    """(counted (R, n), weighted under unit weights and targets rank + 1 (R, n)) of the R rows of S elements at element
    offset `off` of the device tensor t"""
    import torch
    from gpemu import _lib, reweight as RW
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    base = t.data_ptr() + 8 * off
    out = torch.empty((R, len(ranks)), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().gpemu_select_dev(0, R, S, C.c_void_p(base), row_stride, elem_stride, len(ranks), _lib.ptr(ranks),
                                           C.c_void_p(out.data_ptr()), _lib.current_stream(0)))
    ones = torch.ones((1, S), dtype=torch.int64, device="cuda")
    tgt = (ranks + 1).astype(np.uint64)[None, :]
    w = RW.weighted_quantile_dev(0, base, R, S, row_stride, elem_stride, ones, tgt)
    assert w.shape == (1, R, len(ranks))
    return out.cpu().numpy(), w[0]


def _rank_sets(S, rng):
    """rank 0, rank S - 1, one rank twice, and 17 ranks (more than a group of 16) in no order, the ends among them"""
    mid = S // 2
    many = np.concatenate([[0, S - 1, mid, mid], rng.integers(0, S, 13)])
    return [[0], [S - 1], [mid, mid], rng.permutation(many)]


@pytest.mark.parametrize("layout", ["dense", "chain"])
@pytest.mark.parametrize("R", [1, 513])
@pytest.mark.parametrize("S", [1, 255, 4097])
def test_select_is_the_weighted_select_under_unit_weights(S, R, layout):
    """S: one element, less than a workgroup's round, more than a slice of 4096; R: one row, more than a batch of 512;
    dense rows and the parameters of a chain [S][d] (elem_stride = d; R = 1: parameter 1 of d = 3)"""
    rng = np.random.default_rng(1000 * S + 2 * R + (layout == "chain"))
    x = rng.normal(size=(R, S))
    if layout == "dense":
        args = (_dev(x), 0, R, S, S, 1)
    elif R == 1:
        chain = rng.normal(size=(S, 3))
        chain[:, 1] = x[0]
        args = (_dev(chain), 1, 1, S, 1, 3)
    else:
        args = (_dev(x.T), 0, R, S, 1, R)
    xs = np.sort(x, axis=1)
    for ranks in _rank_sets(S, rng):
        counted, weighted = _select_both(*args, ranks)
        want = xs[:, np.asarray(ranks, dtype=np.int64)]
        print(f"S {S} R {R} {layout} ranks {len(ranks)}: counted != numpy {np.count_nonzero(_bits(counted) != _bits(want))}, "
              f"weighted != counted {np.count_nonzero(_bits(weighted) != _bits(counted))}")
        assert np.array_equal(_bits(counted), _bits(want))
        assert np.array_equal(_bits(weighted), _bits(counted))


@pytest.mark.parametrize("S", [255, 4097])
def test_select_on_equal_values_signed_zeros_and_a_nan(S):
    rng = np.random.default_rng(S)
    equal = np.full(S, -3.25)
    m = rng.random(S)
    zeros = np.where(m < 0.4, -0.0, np.where(m < 0.8, 0.0, rng.normal(size=S)))
    with_nan = rng.normal(size=S)
    with_nan[S // 3] = np.nan
    x = np.stack([equal, zeros, with_nan, rng.normal(size=S)])
    for ranks in _rank_sets(S, rng):
        counted, weighted = _select_both(_dev(x), 0, 4, S, S, 1, ranks)
        r = np.asarray(ranks, dtype=np.int64)
        for got in (counted, weighted):
            assert np.array_equal(_bits(got[0]), _bits(equal[r]))
            assert np.array_equal(got[1], np.sort(zeros)[r])          # on values: -0 and +0 are tied, either may come back
            assert np.all(_bits(got[2]) == NAN_BITS)                  # a NaN in the row: NaN for every rank
            assert np.array_equal(_bits(got[3]), _bits(np.sort(x[3])[r]))
        assert np.array_equal(_bits(weighted[[0, 2, 3]]), _bits(counted[[0, 2, 3]]))


# ---- 2. histograms --------------------------------------------------------------------------------------------------------
WEIGHT = 3


def _edges(d, nb, rng):
    """strictly increasing, unevenly spaced edges per parameter: (d, nb + 1)"""
    steps = rng.uniform(0.5, 1.5, size=(d, nb))
    e = np.concatenate([np.zeros((d, 1)), np.cumsum(steps, axis=1)], axis=1)
    return np.ascontiguousarray(-1.0 + 2.0 * e / e[:, -1:])


def _rows(S, d, e1, e2, rng):
    """rows that spill over the box on both sides, with values exactly on outer and inner edges of both sets of edges and
    NaNs, at random places"""
    x = rng.normal(scale=0.7, size=(S, d))
    for k in range(d):
        special = np.concatenate([e1[k, [0, -1, e1.shape[1] // 2]], e2[k, [0, -1, e2.shape[1] // 2]], [np.nan]])
        hit = rng.random(S) < 0.2
        x[hit, k] = rng.choice(special, size=np.count_nonzero(hit))
    return x


def _numpy_hists(x, e1, e2):
    d = x.shape[1]
    h1 = np.stack([np.histogram(x[~np.isnan(x[:, k]), k], bins=e1[k])[0] for k in range(d)]).astype(np.int64)
    h2 = []
    for i in range(d):
        for j in range(i + 1, d):
            ok = ~(np.isnan(x[:, i]) | np.isnan(x[:, j]))     # a NaN lies in no bin
            h2.append(np.histogram2d(x[ok, i], x[ok, j], bins=(e2[i], e2[j]))[0])
    h2 = np.asarray(h2, dtype=np.int64).reshape(len(h2), e2.shape[1] - 1, e2.shape[1] - 1)
    return h1, h2


def _check_hists(x, view, e1, e2, group_counters=0, group_bins=0):
    """x: the logical rows (S, d); view = (device tensor, n_blocks, block_rows, block_stride_rows)"""
    import torch
    from gpemu import marginals as M, reweight as RW
    t, n_blocks, block_rows, stride = view
    S, d = x.shape
    assert S == n_blocks * block_rows
    q = torch.full((1, S), WEIGHT, dtype=torch.int64, device="cuda")
    c0, r0 = M.path_counts(), RW.path_counts()
    h1, h2, ni = M._hist_dev(0, t.data_ptr(), n_blocks, block_rows, stride, d, e1, e2, group_counters)
    w1, w2, wi = RW.weighted_hist_dev(0, t.data_ptr(), n_blocks, block_rows, stride, d, q, e1, e2, group_bins)
    c1, r1 = M.path_counts(), RW.path_counts()
    n1, n2 = _numpy_hists(x, e1, e2)
    print(f"S {S} d {d} bins {e1.shape[1] - 1}/{e2.shape[1] - 1}: inside {ni.tolist()} of {S}; 1-D bins != numpy "
          f"{np.count_nonzero(h1 != n1)}, 2-D {np.count_nonzero(h2 != n2)}; weighted != 3 x counted "
          f"{np.count_nonzero(w1[0] != 3 * h1.astype(np.uint64))}, {np.count_nonzero(w2[0] != 3 * h2.astype(np.uint64))}")
    assert h1.dtype == np.int64 and w1.dtype == np.uint64
    assert np.array_equal(h1, n1) and np.array_equal(h2, n2) and np.array_equal(ni, n1.sum(axis=1))
    assert np.array_equal(w1[0], np.uint64(WEIGHT) * h1.astype(np.uint64))
    assert np.array_equal(w2[0], np.uint64(WEIGHT) * h2.astype(np.uint64))
    assert np.array_equal(wi[0], np.uint64(WEIGHT) * ni.astype(np.uint64))
    return ({k: c1[k] - c0[k] for k in ("HIST_SWEEP", "PAIR_GROUP")},
            {k: r1[k] - r0[k] for k in ("WHIST_SWEEP", "WHIST_PAIR_GROUP")})


@pytest.mark.parametrize("d", [1, 6, 9, 16])
@pytest.mark.parametrize("S", [1, 1025, 70000])
def test_hist_is_the_weighted_hist_under_equal_weights(S, d):
    """d: no pair, both register layouts of the 2-D indices (d <= 8, d > 8) and the widest row; S: one row, more than the
    1024 threads of a workgroup, more than a workgroup's rows (18 workgroups)"""
    rng = np.random.default_rng(100 * S + d)
    e1, e2 = _edges(d, 37, rng), _edges(d, 11, rng)
    x = _rows(S, d, e1, e2, rng)
    _check_hists(x, (_dev(x), 1, S, S), e1, e2)


def test_hist_forms_agree_on_a_thinned_block_view():
    """1000 blocks of 5 rows, 13 rows apart: the stride is no multiple of the block, the rows between are never read"""
    rng = np.random.default_rng(5)
    d, n_blocks, block_rows, stride = 6, 1000, 5, 13
    e1, e2 = _edges(d, 37, rng), _edges(d, 11, rng)
    x = _rows(n_blocks * block_rows, d, e1, e2, rng)
    buf = np.full((n_blocks * stride, d), 0.123)           # inside the box: a row read by mistake is counted
    for b in range(n_blocks):
        buf[b * stride:b * stride + block_rows] = x[b * block_rows:(b + 1) * block_rows]
    _check_hists(x, (_dev(buf), n_blocks, block_rows, stride), e1, e2)


def test_hist_forms_agree_where_only_the_weighted_one_is_banded():
    """nb2 = 136: 136^2 = 18496 bins of a pair exceed the 18432 64-bit bins of a weighted sweep (two bands per pair) and
    fit the 73728 counters of a counted one (the three pairs in one sweep)"""
    rng = np.random.default_rng(6)
    d, S = 3, 5000
    e1, e2 = _edges(d, 37, rng), _edges(d, 136, rng)
    x = _rows(S, d, e1, e2, rng)
    counted, weighted = _check_hists(x, (_dev(x), 1, S, S), e1, e2)
    assert counted == {"HIST_SWEEP": 1, "PAIR_GROUP": 1}
    assert weighted == {"WHIST_SWEEP": 6, "WHIST_PAIR_GROUP": 6}


def test_hist_forms_agree_over_several_sweeps():
    """group_counters = 121 = nb2^2: one pair per counted sweep; group_bins = 40 < 121: bands of 3 of the 11 first
    indices, four per pair; the 1-D bins beside the last sweep where they fit and in sweeps of their own"""
    rng = np.random.default_rng(7)
    d, S = 6, 5000
    e1, e2 = _edges(d, 37, rng), _edges(d, 11, rng)
    x = _rows(S, d, e1, e2, rng)
    counted, weighted = _check_hists(x, (_dev(x), 1, S, S), e1, e2, group_counters=121, group_bins=40)
    # counted: 15 sweeps of one pair (no room beside the last: 121 - 121 < 37), then the six parameters three at a time
    assert counted == {"HIST_SWEEP": 17, "PAIR_GROUP": 15}
    # weighted: 15 pairs x 4 bands; beside the last band (2 x 11 = 22 bins) 18 bins are no room for 37; six sweeps of one
    assert weighted == {"WHIST_SWEEP": 66, "WHIST_PAIR_GROUP": 60}
