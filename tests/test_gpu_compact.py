"""-m gpu tests of the sampler's compacted half-step: with the switch on, the proposals are formed and
tested against the prior box first and only those inside it get cross-kernel rows and GEMM columns; GPEMU_NO_COMPACT=1
evaluates every proposal as before.  The two forms must agree BIT FOR BIT in chain rows, log-probability rows, state and
acceptance counts -- at a live count that changes every half-step, at forced live counts around every 64- and 128-column
boundary, with proposals exactly on a face of the box -- and the samplers outside the scheme's scope must run as before."""
import ctypes as C

import numpy as np
import pytest

import golden_util as GU
from oracle import gp_oracle as O
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu

N, K, D, F, W = 130, 3, 3, 12, 520        # Npad 256: four row blocks; halves of 260: 5 column blocks, 15 (PC, block) groups
LO, HI = np.full(D, 0.2), np.full(D, 0.8)    # the prior: the middle 60 % per coordinate of the unit cube
Z_OUT = 1.0e6                                # a stretch that throws any proposal out of the cube


def _path_counts():
    from gpemu import _lib
    out = np.zeros(32, dtype=np.int64)
    n = _lib.lib().gpemu_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    return out[:n].copy()


@pytest.fixture(scope="module")
def small():
    """130 design points in the unit cube, 3 PCs, RBF + noise at fixed hyper-parameters: (oracle model, problem)."""
    rng = np.random.default_rng(0)
    design = rng.uniform(0.0, 1.0, (N, D))
    Y = np.tanh(design @ rng.normal(size=(D, F))) + 0.01 * rng.normal(size=(N, F))
    mean, scale, _ = O.scaler_fit(Y)
    pca = O.pca_fit((Y - mean) / scale)
    spec = O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=False, has_noise=True)
    theta = np.log(np.r_[np.full(D, 0.5), 0.05])
    gps = [O.gp_fit_at_theta(design, pca["Y_pca"][:, i], theta, spec, 1e-10) for i in range(K)]
    model = O.GroupModel(X_train=design, spec=spec, gps=gps, components=pca["components"],
                         explained_variance=pca["explained_variance"], scaler_mean=mean, scaler_scale=scale, n_pc=K)
    prob = dict(y_exp=Y[0] + 0.05, y_err=rng.uniform(0.01, 0.2, F), Y=Y)
    return model, prob


def _device_model(small, **kw):
    model, prob = small
    dm = GU.device_model(model)
    dm.likelihood_setup(kw.pop("y_exp", prob["y_exp"]), prob["y_err"], LO, HI, 1.0, **kw)
    return dm


def _form(monkeypatch, on):
    if on:
        monkeypatch.delenv("GPEMU_NO_COMPACT", raising=False)
    else:
        monkeypatch.setenv("GPEMU_NO_COMPACT", "1")


def _snapshot(ds, stored):
    X, lp = ds.get_state()
    nacc, it, cl = ds.counts()
    out = dict(X=X, lp=lp, nacc=nacc, it=it, cl=cl)
    if stored:
        out["chain"], out["lpchain"] = ds.get_chain()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)    # bit for bit (-inf == -inf; no NaN on these runs)


def _inside(q):
    return np.all((q > LO) & (q < HI), axis=1)


@pytest.mark.parametrize("store", [True, False])
def test_device_rng_steps_equal_uncompacted(small, monkeypatch, store):
    """6 steps of the device stream from walkers all over the unit cube: the live count changes every half-step."""
    from gpemu.sampler import DeviceSampler
    seed, steps = 0xC0FFEE, 6
    X0 = np.random.default_rng(5).uniform(0.0, 1.0, (W, D))
    got, paths, live = {}, {}, {}
    for on in (True, False):
        _form(monkeypatch, on)
        dm = _device_model(small)
        ds = DeviceSampler([dm], W, seed=seed)
        ds.set_state(X0)
        p0 = _path_counts()
        ds.run(steps, store=store)
        paths[on] = _path_counts() - p0
        got[on] = _snapshot(ds, store)
        live[on] = (ds.live_counts, ds.live_fraction)
        assert dm.profile_read()["live"] == ds.live_counts               # the model's entry: this sampler is its only one
        ds.close()
        dm.close()
    _assert_same(got[True], got[False])
    np.testing.assert_array_equal(paths[True], paths[False])          # keyed by the launch shape, not by the live count
    assert live[False] == ((0, 0), None)
    assert live[True][0][1] == steps * W
    if store:
        # the in-box proposals of every half, formed on the host from the stream's draws and the stored states
        stream, prev, n_in = SO.PhiloxStream(seed), X0, 0
        for t in range(steps):
            inds, zz, rint, _ = stream.draw(W)
            cur = got[True]["chain"][t]
            mid = np.where((inds == 0)[:, None], cur, prev)             # after half 0: only its walkers have moved
            for h, X in ((0, prev), (1, mid)):
                s, c = X[inds == h], X[inds != h]
                n_in += int(np.sum(_inside(c[rint[h]] - (c[rint[h]] - s) * zz[h][:, None])))
            prev = cur
        assert live[True][0] == (n_in, steps * W)
        assert live[True][1] == n_in / (steps * W)
        assert 0.2 < live[True][1] < 0.95                               # (the case is about a changing count)


def _forced_draws(half, count, other, rng):
    """One step's host draws that leave exactly `count` proposals of `half` (and `other` of the other half) inside the
    box when every walker is: z = 1 proposes the walker's own position, Z_OUT a point far outside."""
    inds = (np.arange(W) % 2).astype(np.int32)
    rng.shuffle(inds)
    ns = (W + 1) // 2, W // 2
    zz, rint, logu = [], [], []
    for h in range(2):
        z = np.full(ns[h], Z_OUT)
        z[rng.permutation(ns[h])[:count if h == half else other]] = 1.0
        zz.append(z)
        rint.append(rng.integers(0, W - ns[h], ns[h]).astype(np.int64))
        logu.append(np.log(rng.uniform(0.0, 1.0, ns[h])))
    return inds, zz, rint, logu


@pytest.mark.parametrize("half", [0, 1])
def test_forced_live_counts(small, monkeypatch, half):
    """Live counts of 0, 1, around every 64- and 128-column boundary and all 260, forced through the host-RNG step."""
    from gpemu.sampler import DeviceSampler
    X0 = np.random.default_rng(7).uniform(0.3, 0.7, (W, D))             # every walker well inside the box
    dm = _device_model(small)
    lp0 = dm.logpost(X0)
    assert np.all(np.isfinite(lp0))
    ds = {on: DeviceSampler([dm], W, seed=1) for on in (True, False)}
    other = 100
    for count in (0, 1, 63, 64, 65, 128, 129, 255, 256, W // 2):
        draws = _forced_draws(half, count, other, np.random.default_rng(1000 + count))
        got = {}
        for on in (True, False):
            _form(monkeypatch, on)
            ds[on].reset()
            ds[on].set_state(X0, lp0)
            before = ds[on].live_counts
            ds[on].step_host_rng(*draws)                                # (raises on a NaN flag)
            got[on] = _snapshot(ds[on], True)
            after = ds[on].live_counts
            assert (after[0] - before[0], after[1] - before[1]) == ((count + other, W) if on else (0, 0)), (count, on)
        _assert_same(got[True], got[False])
        sel = draws[0] == half
        if count == 0:                                                  # nothing of this half moved, nothing was flagged
            np.testing.assert_array_equal(got[True]["X"][sel], X0[sel])
            np.testing.assert_array_equal(got[True]["lp"][sel], lp0[sel])
            np.testing.assert_array_equal(got[True]["chain"][0][sel], X0[sel])
            assert not np.any(got[True]["nacc"][sel])
    for s in ds.values():
        s.close()
    dm.close()


def test_proposals_on_the_faces_are_outside(small, monkeypatch):
    """A proposal with a coordinate exactly on lo, and one exactly on hi, is outside the (open) box in both forms."""
    from gpemu.sampler import DeviceSampler
    X0 = np.random.default_rng(9).uniform(0.3, 0.7, (W, D))
    inds = (np.arange(W) % 2).astype(np.int32)
    # walkers 0, 2 (set 0) and their partners 1, 3 (set 1) share the face coordinate: q = c - (c - s) z is exactly on it
    X0[[0, 1], 0] = LO[0]
    X0[[2, 3], 2] = HI[2]
    ns = W // 2
    rint = [np.zeros(ns, dtype=np.int64), np.zeros(ns, dtype=np.int64)]
    rint[0][:2] = [0, 1]          # proposal i of half 0 is walker 2 i; member r of the other set is walker 2 r + 1
    rint[1][:2] = [0, 1]          # ... and the other way round: the four face walkers propose onto their faces
    rint[0][2:] = np.arange(2, ns)
    rint[1][2:] = np.arange(2, ns)
    zz = [np.full(ns, 1.0), np.full(ns, 1.0)]
    zz[0][:2] = zz[1][:2] = 1.75
    logu = [np.log(np.random.default_rng(3).uniform(0.0, 1.0, ns)) for _ in range(2)]
    dm = _device_model(small)
    lp0 = dm.logpost(X0)
    assert np.all(np.isneginf(lp0[:4])) and np.all(np.isfinite(lp0[4:]))
    got = {}
    for on in (True, False):
        _form(monkeypatch, on)
        ds = DeviceSampler([dm], W, seed=1)
        ds.set_state(X0, lp0)
        ds.step_host_rng(inds, zz, rint, logu)
        got[on] = _snapshot(ds, True)
        if on:
            assert ds.live_counts == (W - 4, W)
        ds.close()
    dm.close()
    _assert_same(got[True], got[False])
    np.testing.assert_array_equal(got[True]["X"][:4], X0[:4])
    assert not np.any(got[True]["nacc"][:4])


def _run_both(monkeypatch, make, steps=3):
    got, paths, live = {}, {}, {}
    for on in (True, False):
        _form(monkeypatch, on)
        ds, closers = make()
        p0 = _path_counts()
        ds.run(steps)
        paths[on] = _path_counts() - p0
        got[on] = _snapshot(ds, True)
        live[on] = (ds.live_counts, ds.live_fraction)
        ds.close()
        for c in closers:
            c.close()
    _assert_same(got[True], got[False])
    np.testing.assert_array_equal(paths[True], paths[False])
    return live


@pytest.mark.parametrize("kind", ["tempered", "stacked", "sources"])
def test_outside_the_scope_runs_as_before(small, monkeypatch, kind):
    """A tempered sampler, two stacked chains and a model with correlated sources, switch on: today's launches (the path
    counters of the switch off), today's bits, and nothing compacted."""
    from gpemu.sampler import DeviceSampler, TemperedSampler
    _, prob = small
    rng = np.random.default_rng(11)
    X0 = rng.uniform(0.0, 1.0, (2 * W, D))
    src = 0.05 * rng.normal(size=(2, F))

    def make():
        if kind == "tempered":
            dm = _device_model(small)
            ds = TemperedSampler([dm], W, [1.0, 0.5], seed=3, swap_every=1)
            ds.set_state(X0)
        elif kind == "stacked":
            dm = _device_model(small, y_exp=np.stack([prob["y_exp"], prob["Y"][1] + 0.05]))
            ds = DeviceSampler([dm], W, seeds=[3, 4])
            ds.set_state(X0)
        else:
            dm = _device_model(small, sys_sources=src)
            ds = DeviceSampler([dm], W, seed=3)
            ds.set_state(X0[:W])
        return ds, [dm]

    live = _run_both(monkeypatch, make)
    assert live[True] == ((0, 0), None) and live[False] == ((0, 0), None)


@pytest.fixture(scope="module")
def c3():
    """N = 1000, 10 PCs on the device (the benchmark's shape): every CU a GEMM worker, so that the live blocks are dealt
    to the XCDs by cost, the cross-kernel follows that deal, and few blocks have every item halved."""
    model, prob, _ = GU.fixed_theta_model(1000, 500, 10, seed=0)
    dm = GU.device_model(model)
    dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
    yield dm, prob
    dm.close()


def test_headline_size_forced_counts(c3, monkeypatch):
    """Every live block count 0 .. 8 of the benchmark's shape, and the counts next to each boundary, forced in both
    halves: a dropped or doubled item of a count's schedule or cross-kernel map leaves a stale or missing partial sum."""
    from gpemu import synthetic
    from gpemu.sampler import DeviceSampler
    dm, prob = c3
    lo, hi = prob["lo"], prob["hi"]
    Wb = 1024
    X0 = synthetic.make_walkers(Wb, seed=1, lo=lo + 0.1 * (hi - lo), hi=hi - 0.1 * (hi - lo))
    lp0 = dm.logpost(X0)
    ds = {on: DeviceSampler([dm], Wb, seed=1) for on in (True, False)}
    for count in (0, 1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512):
        rng = np.random.default_rng(2000 + count)
        inds = (np.arange(Wb) % 2).astype(np.int32)
        rng.shuffle(inds)
        zz, rint, logu = [], [], []
        for h in range(2):
            z = np.full(Wb // 2, Z_OUT)
            z[rng.permutation(Wb // 2)[:count]] = 1.0
            zz.append(z)
            rint.append(rng.integers(0, Wb // 2, Wb // 2).astype(np.int64))
            logu.append(np.log(rng.uniform(0.0, 1.0, Wb // 2)))
        got = {}
        for on in (True, False):
            _form(monkeypatch, on)
            ds[on].reset()
            ds[on].set_state(X0, lp0)
            before = ds[on].live_counts
            ds[on].step_host_rng(inds, zz, rint, logu)
            got[on] = _snapshot(ds[on], True)
            after = ds[on].live_counts
            assert (after[0] - before[0], after[1] - before[1]) == ((2 * count, Wb) if on else (0, 0)), (count, on)
        _assert_same(got[True], got[False])
    for s in ds.values():
        s.close()


def test_headline_size_equal_uncompacted(c3, monkeypatch):
    """N = 1000, 10 PCs, 1024 walkers (the benchmark's shape: XCD-aware schedules, 8 column blocks): 3 steps."""
    from gpemu import synthetic
    from gpemu.sampler import DeviceSampler
    dm, prob = c3
    X0 = synthetic.make_walkers(1024, seed=1)
    got, live = {}, {}
    for on in (True, False):
        _form(monkeypatch, on)
        ds = DeviceSampler([dm], 1024, a=2.0, seed=1)
        ds.set_state(X0)
        ds.run(3)
        got[on] = _snapshot(ds, True)
        live[on] = ds.live_counts
        ds.close()
    _assert_same(got[True], got[False])
    assert live[False] == (0, 0) and live[True][1] == 3 * 1024 and 0 < live[True][0] < 3 * 1024
