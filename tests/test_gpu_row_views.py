"""-m gpu tests of what the summaries of a stored chain share (csrc/k_rows.hip, rows_dev.h; DeviceSampler._stored_view):
one view of the chain behind the four sampler summaries, a block stride that is no multiple of d, the host forms of the
row functions against their device forms, and the one device check.  Every comparison is the one the feature's own test
file makes for that quantity: bitwise, but for the interpolated parameter quantiles (two spacings of the bracketing order
statistics, tests/test_gpu_posterior_predictive.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
WC, STEPS = 8, 40                                  # walkers per chain, stored steps
VIEWS = [(0, 1, 0), (3, 1, 1), (5, 3, 1)]          # (discard, thin, chain)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _all_path_counts():
    from gpemu import _lib
    L, out = _lib.lib(), []
    for fam in ("", "fit_", "wide_", "src_", "grad_", "postpred_", "hmc_", "diag_", "sobol_", "marginal_"):
        buf = (C.c_int64 * 64)()
        n = getattr(L, f"gpemu_{fam}path_counts")(buf, 64)
        out.append(list(buf[:n]))
    return out


# ---- 1. one view, four summaries -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stacked():
    """(sampler of 2 chains x 8 walkers with 40 stored steps, its model, the chain on the host, lo, hi)"""
    import golden_util as GU
    import path_cases as PC
    from gpemu.sampler import DeviceSampler
    c = [x for x in PC.cases() if x.name == "n16_d7_m15_const"][0]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    dm = GU.device_model(model)
    dm.likelihood_setup(np.stack([y_exp, y_exp * 1.01]), y_err, lo, hi, 1.0, block_start=bs)
    s = DeviceSampler([dm], WC, seeds=[3, 4])
    s.set_state(rng.uniform(lo, hi, (2 * WC, lo.size)))
    s.run(STEPS)
    return s, dm, s.get_chain()[0], lo, hi


@pytest.mark.parametrize("discard,thin,chain", VIEWS)
def test_one_view_four_summaries(discard, thin, chain):
    from gpemu import diagnostics as D
    from gpemu import select
    from test_gpu_marginals import _same_marginals
    from test_gpu_posterior_predictive import _same
    s, dm, full, lo, hi = _stacked()
    d = lo.size
    steps = np.ascontiguousarray(full[discard::thin][:, chain * WC:(chain + 1) * WC])
    rows = steps.reshape(-1, d)

    got = s.posterior_predictive(discard=discard, thin=thin, chain=chain, probabilities=PROBS)
    assert len(got) == 1
    _same(dm.posterior_predictive(rows, probabilities=PROBS), got[0])

    # (parameter_quantiles has no thin: every step from discard on)
    unthinned = np.ascontiguousarray(full[discard:][:, chain * WC:(chain + 1) * WC]).reshape(-1, d)
    got, want = s.parameter_quantiles(PROBS, discard=discard, chain=chain), select.quantile(unthinned, PROBS, axis=0)
    ilo, ihi, _ = select.virtual_index(unthinned.shape[0], PROBS)
    srt = np.sort(unthinned, axis=0)
    assert got.shape == want.shape == (len(PROBS), d)
    assert np.all(np.abs(got - want) <= 2 * np.spacing(np.maximum(np.abs(srt[ilo]), np.abs(srt[ihi]))))

    got, want = s.diagnostics(discard=discard, thin=thin, chain=chain), D.summary(steps)
    for k in D.KEYS:
        assert _bits(got[k]) == _bits(want[k]), k
    assert got["n_chains"] == 2 * WC and got["n_draws"] == steps.shape[0] // 2

    got = s.marginals(bins_1d=9, bins_2d=4, confidence=(0.5, 0.9), n_grid=17, discard=discard, thin=thin, chain=chain)
    _same_marginals(got, rows, lo, hi, (9, 4), (0.5, 0.9), 17)


def test_a_single_block_of_a_stacked_chain_is_read_where_it_lies():
    """The last step of chain 1: 8 rows in one block of a 16-walker ensemble.  One block is dense by ``RowsView::dense()``
    whatever its stride, so the sort and the density read the chain itself, no dense copy.  The two summaries that accept 8
    rows (the diagnostics need 8 steps; confidence 0.9 leaves int(0.1 * 8) = 0 rows outside and is refused)."""
    from test_gpu_marginals import _same_marginals
    from test_gpu_posterior_predictive import _same
    s, dm, full, lo, hi = _stacked()
    discard, thin, chain = STEPS - 1, 1, 1
    view = s._stored_view(discard, thin, chain)
    assert (view.n_blocks, view.block_rows, view.rows) == (1, WC, WC) and WC < s.W
    assert view.dense and view.columns() is view
    rows = np.ascontiguousarray(full[discard::thin][:, chain * WC:(chain + 1) * WC]).reshape(-1, lo.size)
    assert rows.shape[0] == WC

    got = s.posterior_predictive(discard=discard, thin=thin, chain=chain, probabilities=PROBS)
    assert len(got) == 1
    _same(dm.posterior_predictive(rows, probabilities=PROBS), got[0])

    got = s.marginals(bins_1d=9, bins_2d=4, confidence=(0.5, 0.75), n_grid=17, discard=discard, thin=thin, chain=chain)
    _same_marginals(got, rows, lo, hi, (9, 4), (0.5, 0.75), 17)


def test_views_without_steps_or_outside_the_chains_are_refused():
    s = _stacked()[0]
    calls = (s.posterior_predictive, lambda **kw: s.parameter_quantiles(PROBS, **kw), s.diagnostics, s.marginals)
    for call in calls:
        with pytest.raises(ValueError):
            call(discard=STEPS, chain=0)
        with pytest.raises(IndexError):
            call(chain=2)


# ---- 2. a block stride that is no multiple of d ------------------------------------------------------------------------
@pytest.mark.parametrize("w0,nw", [(0, 4), (1, 3)])
def test_diag_of_steps_padded_to_a_stride_that_is_no_multiple_of_d(w0, nw):
    import torch
    from gpemu import _lib
    from gpemu import diagnostics as D
    n, stride, d = 16, 14, 3
    x = np.random.default_rng(5).normal(size=(n, 4, d))
    x[0:15:5, 1, 2] = x[1:16:5, 2, 2]                             # ties
    padded = np.full((n, stride), np.nan)
    padded[:, :4 * d] = x.reshape(n, 4 * d)
    dev = torch.as_tensor(padded, device="cuda:0")
    h = C.c_void_p()
    _lib.check(_lib.lib().gpemu_diag_create_dev(C.byref(h), 0, C.c_void_p(dev.data_ptr()), n, stride, w0, nw, d, 0,
                                                _lib.current_stream(0)))
    with D.Diag(_handle=h, _shape=(n, nw, d), _keep=dev) as got, D.Diag(np.ascontiguousarray(x[:, w0:w0 + nw])) as want:
        a, b = got.pooled(), want.pooled()
        for k in a:
            assert np.all(np.isfinite(a[k])) and _bits(a[k]) == _bits(b[k]), k
        for u, v in zip(got.transform(D.FOLDED_RANK_Z), want.transform(D.FOLDED_RANK_Z)):
            assert np.all(np.isfinite(u)) and _bits(u) == _bits(v)
        assert _bits(got.series()) == _bits(want.series())


# ---- 3. the host forms are the device forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 1), (3, 257), (2, 2049)])
def test_host_wrappers_equal_the_device_calls(R, S):
    import torch
    from gpemu import _lib
    from gpemu._lib import check, ptr
    L = _lib.lib()
    v = np.random.default_rng(R * 1000 + S).normal(size=(R, S))
    v[:, ::4] = np.round(v[:, ::4], 1)
    if R > 1:
        v[R - 1, S // 3] = np.nan                   # one row holds a NaN
    dv = torch.as_tensor(v, device="cuda:0")
    st = _lib.current_stream(0)

    def dev_out(*shape):
        return torch.full(shape, -7.0, dtype=torch.float64, device="cuda:0")

    ranks = np.unique(np.array([0, S // 2, S - 1], dtype=np.int64))
    host, dout = np.empty((R, ranks.size)), dev_out(R, ranks.size)
    check(L.gpemu_select(0, R, S, ptr(v), ranks.size, ptr(ranks), ptr(host)))
    check(L.gpemu_select_dev(0, R, S, C.c_void_p(dv.data_ptr()), S, 1, ranks.size, ptr(ranks), C.c_void_p(dout.data_ptr()), st))
    assert _bits(host) == _bits(dout.cpu().numpy())

    host, dout = np.empty((R, S)), dev_out(R, S)
    check(L.gpemu_rank(0, R, S, ptr(v), ptr(host)))
    check(L.gpemu_rank_dev(0, R, S, C.c_void_p(dv.data_ptr()), S, 1, C.c_void_p(dout.data_ptr()), 0, st))
    assert _bits(host) == _bits(dout.cpu().numpy())
    if R > 1:
        assert np.all(np.isnan(host[R - 1])) and np.all(np.isfinite(host[:R - 1]))

    n_out = np.unique(np.array([1, max(1, S // 10)], dtype=np.int64))
    host, dout = np.empty((R, n_out.size, 2)), dev_out(R, n_out.size, 2)
    check(L.gpemu_hpd(0, R, S, ptr(v), n_out.size, ptr(n_out), ptr(host)))
    check(L.gpemu_hpd_dev(0, R, S, C.c_void_p(dv.data_ptr()), S, 1, n_out.size, ptr(n_out), C.c_void_p(dout.data_ptr()), 0, st))
    assert _bits(host) == _bits(dout.cpu().numpy())

    G = 5
    grid = np.ascontiguousarray(np.broadcast_to(np.linspace(-2.0, 2.0, G), (R, G)))
    bw = np.full(R, 0.3)                            # explicit: S = 1 has no default bandwidth
    host, dout = np.empty((R, G)), dev_out(R, G)
    check(L.gpemu_kde1d(0, R, S, ptr(v), G, ptr(grid), ptr(bw), ptr(host)))
    check(L.gpemu_kde1d_dev(0, R, S, C.c_void_p(dv.data_ptr()), S, 1, G, ptr(grid), ptr(bw), C.c_void_p(dout.data_ptr()), st))
    assert _bits(host) == _bits(dout.cpu().numpy())
    assert np.all(host[0] > 0.0)


# ---- 4. the device check is one function -------------------------------------------------------------------------------
def test_every_file_refuses_a_device_that_is_not_there_before_any_launch():
    from gpemu import _lib
    from gpemu._lib import check, ptr
    L = _lib.lib()
    v, out3, one = np.zeros((2, 3)), np.zeros((2, 3)), np.array([1], dtype=np.int64)
    name = C.create_string_buffer(128)
    theta, K = np.zeros(4), np.zeros((2, 2))        # d = 3 length scales and the noise
    Y, pca = np.arange(12.0).reshape(4, 3) ** 2, [np.zeros(16) for _ in range(8)]
    calls = {
        "gpemu_device_name": lambda dev: L.gpemu_device_name(dev, name, 128),
        "gpemu_select": lambda dev: L.gpemu_select(dev, 2, 3, ptr(v), 1, ptr(one), ptr(out3)),
        "gpemu_rank": lambda dev: L.gpemu_rank(dev, 2, 3, ptr(v), ptr(out3)),
        "gpemu_hpd": lambda dev: L.gpemu_hpd(dev, 2, 3, ptr(v), 1, ptr(one), ptr(out3)),
        "gpemu_kernel_matrix": lambda dev: L.gpemu_kernel_matrix(dev, 2, 3, ptr(v), ptr(theta), 4, 0, 0.0, 0, 1, 1e-10, ptr(K)),
        "gpemu_pca_fit": lambda dev: L.gpemu_pca_fit(dev, 4, 3, ptr(Y), 2, *(ptr(a) for a in pca), None, None),
    }
    before = _all_path_counts()
    for fn, call in calls.items():
        assert call(0) == 0, (fn, _lib.last_error())            # the arguments are good: only the device is refused below
    launched = _all_path_counts()
    for dev in (-1, _lib.device_count()):
        for fn, call in calls.items():
            with pytest.raises(_lib.GpemuError) as err:
                check(call(dev))
            assert err.value.code == -1, fn                    # GPEMU_ERR_ARG
            assert f"device {dev} out of range (have {_lib.device_count()})" in str(err.value), fn
    assert _all_path_counts() == launched and launched != before
