"""-m gpu tests of the exact selection on the device (gpemu_select / gpemu_select_dev, gpemu.select): every order
statistic equals np.sort's element as a double; quantiles equal np.quantile(method='linear') within 2 ulp of the larger
bracketing element (one rounding of the weight, one of the lerp expression), exactly where the virtual index is an
integer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (7, 1000), (2000, 1000), (1, 2 ** 24 + 3), (500, 100003)]


def _ranks_sets(S, rng):
    """0 and S - 1, neighbouring pairs, duplicated ranks, 16 ranks at once"""
    sets = [[0, S - 1]]
    a = int(rng.integers(0, max(S - 1, 1)))
    sets.append([a, min(a + 1, S - 1), S // 2, min(S // 2 + 1, S - 1)])
    sets.append([S // 3, S // 3, S - 1, S // 3, 0, 0])
    sets.append(sorted(int(v) for v in rng.integers(0, S, 16))[::-1])
    return sets


def _data(kind, R, S, rng):
    if kind == "normal":
        return rng.normal(size=(R, S))
    if kind == "duplicates":
        return rng.integers(0, 8, (R, S)).astype(np.float64)
    if kind == "all_equal":
        return np.repeat(rng.normal(size=(R, 1)), S, axis=1)
    if kind == "low_bits":      # values that differ only in the low 11 bits
        base = np.float64(1.2345678901234567).view(np.uint64) & ~np.uint64(0x7FF)
        return (base | rng.integers(0, 2048, (R, S)).astype(np.uint64)).view(np.float64)
    if kind == "negative":
        return -np.abs(rng.normal(size=(R, S))) * 1e3
    if kind == "mixed_sign":
        return rng.normal(size=(R, S)) * 10.0 ** rng.integers(-300, 300, (R, S))
    if kind == "subnormal":
        return rng.integers(0, 2 ** 40, (R, S)).astype(np.int64).view(np.float64) * rng.choice([-1.0, 1.0], (R, S))
    if kind == "inf":
        v = rng.normal(size=(R, S))
        v[rng.random((R, S)) < 0.2] = np.inf
        v[rng.random((R, S)) < 0.2] = -np.inf
        return v
    if kind == "zeros":
        v = rng.normal(size=(R, S))
        v[rng.random((R, S)) < 0.4] = 0.0
        v[rng.random((R, S)) < 0.3] = -0.0
        return v
    raise KeyError(kind)


KINDS = ["normal", "duplicates", "all_equal", "low_bits", "negative", "mixed_sign", "subnormal", "inf", "zeros"]


def _check(v, ranks):
    from gpemu import select
    got = select.order_statistics(v, ranks, axis=-1)
    want = np.sort(v, axis=-1)[:, ranks].T
    assert got.shape == want.shape
    bad = ~(got == want)
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


@pytest.mark.parametrize("R,S", SHAPES)
def test_order_statistics_equal_sort_on_every_shape(R, S):
    rng = np.random.default_rng(R * 31 + S)
    v = _data("normal", R, S, rng)
    sets = _ranks_sets(S, rng)
    if R * S > 10 ** 7:      # the two large shapes: the 16 ranks with the extremes appended, in one call
        sets = [sets[3] + sets[0] + sets[1]]
    for ranks in sets:
        _check(v, ranks)


@pytest.mark.parametrize("kind", KINDS)
def test_order_statistics_equal_sort_on_every_kind_of_data(kind):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    for R, S in [(3, 2), (7, 1000), (40, 5003)]:
        v = _data(kind, R, S, rng)
        for ranks in _ranks_sets(S, rng):
            _check(v, ranks)


def test_subnormals_are_subnormal():
    v = _data("subnormal", 4, 100, np.random.default_rng(0))
    assert np.all(np.abs(v) < np.finfo(np.float64).tiny)


def test_a_row_with_a_nan_is_nan_and_leaves_the_others():
    from gpemu import select
    rng = np.random.default_rng(5)
    v = rng.normal(size=(9, 3001))
    v[2, 17] = np.nan
    v[7, 3000] = -np.nan
    ranks = [0, 1500, 3000, 1500]
    got = select.order_statistics(v, ranks)
    want = np.sort(v, axis=-1)[:, ranks].T
    assert np.isnan(got[:, [2, 7]]).all()
    keep = [r for r in range(9) if r not in (2, 7)]
    assert np.array_equal(got[:, keep], want[:, keep])


def test_more_ranks_than_one_group():
    rng = np.random.default_rng(6)
    v = rng.normal(size=(5, 4099))
    _check(v, [int(r) for r in rng.integers(0, 4099, 41)])


def test_strided_dev_form_on_a_chain_tensor():
    import torch
    from gpemu import _lib, select
    rng = np.random.default_rng(7)
    T, W, d = 37, 24, 7
    chain = rng.normal(size=(T, W, d))
    dchain = torch.as_tensor(chain, device="cuda:0")
    want = np.sort(chain.reshape(-1, d), axis=0)
    ranks = np.array([0, T * W - 1, 100, 101, 400, 400], dtype=np.int64)
    # the raw entry: parameter j is "row" j, row stride 1, element stride d
    dout = torch.empty((d, ranks.size), dtype=torch.float64, device="cuda:0")
    _lib.check(_lib.lib().gpemu_select_dev(0, d, T * W, C.c_void_p(dchain.data_ptr()), 1, d, ranks.size,
                                           _lib.ptr(ranks), C.c_void_p(dout.data_ptr()), None))
    assert np.array_equal(dout.cpu().numpy(), want[ranks].T)
    # the tensor entry of gpemu.select reads the same view in place
    got = select.order_statistics(dchain.reshape(-1, d), ranks, axis=0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want[ranks])
    q = select.quantile(dchain.reshape(-1, d), [0.05, 0.5, 0.95], axis=0).cpu().numpy()
    _assert_quantile(chain.reshape(-1, d).T, [0.05, 0.5, 0.95], q.T)


def _assert_quantile(v, probs, got):
    """v (R, S), got (R, nq): within 2 ulp of max(|a|, |b|) of the bracketing pair; exact at integer indices"""
    from gpemu import select
    want = np.quantile(v, probs, axis=-1, method="linear").T
    S = v.shape[-1]
    lo, hi, t = select.virtual_index(S, probs)
    srt = np.sort(v, axis=-1)
    a, b = srt[:, lo], srt[:, hi]
    tol = 2 * np.spacing(np.maximum(np.abs(a), np.abs(b)))
    err = np.abs(got - want)
    print("quantile: max err / tol", float(np.max(err / tol)))
    assert np.all(err <= tol)
    exact = t == 0
    assert np.array_equal(got[:, exact], a[:, exact])


@pytest.mark.parametrize("R,S", [(7, 1000), (3, 2), (1, 1), (50, 100003), (11, 101)])
def test_quantile_against_numpy(R, S):
    from gpemu import select
    rng = np.random.default_rng(S)
    v = rng.normal(size=(R, S)) * 10.0 ** rng.integers(-3, 4, (R, 1))
    probs = [0.0, 0.05, 0.16, 0.25, 0.5, 0.84, 0.95, 1.0, 1.0 / 3.0]
    _assert_quantile(v, probs, select.quantile(v, probs, axis=-1).T)
    assert select.quantile(v, 0.5).shape == (R,)


def test_quantile_integer_virtual_index_is_exact():
    from gpemu import select
    rng = np.random.default_rng(9)
    v = rng.normal(size=(6, 101))        # (S - 1) p is an integer for p = j / 100
    probs = [0.0, 0.05, 0.5, 0.95, 1.0]
    got = select.quantile(v, probs)
    want = np.sort(v, axis=-1)[:, [0, 5, 50, 95, 100]].T
    assert np.array_equal(got, want)


def test_invalid_arguments_return_err_arg():
    from gpemu import _lib
    L = _lib.lib()
    v = np.arange(12.0).reshape(3, 4)
    out = np.empty((3, 2))
    for ranks in ([-1, 0], [0, 4], [2 ** 40, 0]):
        r = np.array(ranks, dtype=np.int64)
        assert L.gpemu_select(0, 3, 4, _lib.ptr(v), 2, _lib.ptr(r), _lib.ptr(out)) == -1
    r = np.array([0, 0], dtype=np.int64)
    assert L.gpemu_select(0, 3, 0, _lib.ptr(v), 2, _lib.ptr(r), _lib.ptr(out)) == -1      # S = 0
    assert L.gpemu_select(0, 0, 4, _lib.ptr(v), 2, _lib.ptr(r), _lib.ptr(out)) == -1
    assert L.gpemu_select(0, 3, 4, _lib.ptr(v), 0, _lib.ptr(r), _lib.ptr(out)) == -1
    assert L.gpemu_select_dev(0, 3, 4, _lib.ptr(v), 0, 1, 2, _lib.ptr(r), _lib.ptr(out), None) == -1   # row stride 0
    assert L.gpemu_select(0, 3, 4, _lib.ptr(v), 2, _lib.ptr(r), _lib.ptr(out)) == 0


def test_select_pass_counter_counts_eight_passes_per_group():
    from gpemu import select
    from gpemu.model import POSTPRED_PATHS, postpred_path_counts
    i = POSTPRED_PATHS.index("select_pass")
    v = np.random.default_rng(3).normal(size=(4, 300))
    c0 = postpred_path_counts()[i]
    select.order_statistics(v, [1, 2, 3])
    assert postpred_path_counts()[i] - c0 == 8
    select.order_statistics(np.zeros((4, 300)), list(range(17)))      # all equal: the same passes, two groups of ranks
    assert postpred_path_counts()[i] - c0 == 8 + 16
