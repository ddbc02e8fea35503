"""-m gpu tests of the sampler's compacted half-step: with the switch on, the proposals are formed and
tested against the prior box first and only those inside it get cross-kernel rows and GEMM columns; GPEMU_NO_COMPACT=1
evaluates every proposal as before.  The two forms must agree BIT FOR BIT in chain rows, log-probability rows, state and
acceptance counts -- at a live count that changes every half-step, at forced live counts around every 64- and 128-column
boundary, with proposals exactly on a face of the box -- and the samplers outside the scheme's scope must run as before."""
import contextlib
import ctypes as C
import dataclasses

import numpy as np
import pytest

import golden_util as GU
import matern_nu_ref as R
from chain_compare import compare_chains
from oracle import gp_oracle as O
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu

N, K, D, F, W = 130, 3, 3, 12, 520        # Npad 256: four row blocks; halves of 260: 5 column blocks, 15 (PC, block) groups
LO, HI = np.full(D, 0.2), np.full(D, 0.8)    # the prior: the middle 60 % per coordinate of the unit cube
Z_OUT = 1.0e6                                # a stretch that throws any proposal out of the cube
TASK_BLOCKS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 12]    # nine observable blocks: the likelihood's tasks kernel at any batch (8 or more)
TWO_BLOCKS = [0, 5, 12]                      # two: the tasks kernel up to 256 proposals only (halves of 260 are compacted)


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


def _forced_draws(half, count, other, rng, W=W):
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


@pytest.mark.parametrize("kind", ["tempered", "stacked", "sources", "groups", "blocks"])
def test_outside_the_scope_runs_as_before(small, monkeypatch, kind):
    """A tempered sampler, two stacked chains, a model with correlated sources, two emulation groups and a model whose
    nine observable blocks take the likelihood's tasks kernel, switch on: today's launches (the path counters of the
    switch off), today's bits, and nothing compacted."""
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
        elif kind == "groups":
            dms = [_device_model(small), _device_model(small, y_exp=prob["Y"][1] + 0.05)]
            ds = DeviceSampler(dms, W, seed=3)
            ds.set_state(X0[:W])
            return ds, dms
        elif kind == "blocks":
            dm = _device_model(small, block_start=TASK_BLOCKS)
            ds = DeviceSampler([dm], W, seed=3)
            ds.set_state(X0[:W])
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


# ---------------------------------------------------------------------------------------------------------------------
# The compacted step against the CPU restatement (oracle/sampler_oracle.py: stretch_step on the same draws, with
# gp_oracle.log_posterior), at the kernel kinds, widths, PC counts, chunkings and sizes the tests above do not reach.
# Two forms of one library agree bit for bit even where both are wrong in the same way (a stale row that both read, a
# likelihood that takes the wrong column in both); the oracle shares no code with either.
class _Case:
    """An oracle emulation group with its data and prior box: the device model of it, and the oracle's log-posterior."""

    def __init__(self, model, y_exp, y_err, lo, hi, block_start=None, oracle_ctx=contextlib.nullcontext):
        self.model, self.y_exp, self.y_err, self.lo, self.hi = model, y_exp, y_err, np.asarray(lo), np.asarray(hi)
        self.block_start, self.ctx = block_start, oracle_ctx
        self.d = self.lo.size
        self.cov_un = O.cov_unexplained(model)
        self.mapping = None
        if block_start is not None:     # the reference's merge keeps the covariance inside an observable's block only
            self.mapping = {f"o{i}": ("g", slice(a, b), slice(a, b)) for i, (a, b) in enumerate(zip(block_start, block_start[1:]))}

    def device(self):
        dm = GU.device_model(self.model)
        dm.likelihood_setup(self.y_exp, self.y_err, self.lo, self.hi, 1.0, block_start=self.block_start)
        return dm

    def lp(self, X):
        """O.log_posterior of every row as a batch of one.  (It divides the truncation covariance by the number of in-box
        rows of its batch, the reference's n_samples quirk; the sampler evaluates every proposal with n_samples = 1, so
        the batch is given that many times the covariance.)"""
        X = np.atleast_2d(X)
        n = max(1, int(np.count_nonzero(self.inside(X))))
        with self.ctx():
            return O.log_posterior(X, {"g": self.model}, self.lo, self.hi, self.y_exp, self.y_err, self.mapping,
                                   {"g": self.cov_un * float(n)})

    def inside(self, q):
        return np.all((q > self.lo) & (q < self.hi), axis=1)


class _Margins:
    """The oracle's own accept margins |factor + lp_new - lp_old - log u| of the in-box proposals.  The device's
    log-probabilities are held to 1e-8 of the oracle's, so a decision is only the same by right where the margin is well
    above 1e-8 max |lp|: a case asserts 100 times that, on the host, and gets another seed if it does not hold."""

    def __init__(self):
        self.least, self.max_lp = np.inf, 0.0

    def add(self, d, draws, lp_before, new_lp):
        inds, zz, _, logu = draws
        for h in range(2):
            live = np.isfinite(new_lp[h])
            if not np.any(live):
                continue
            old = lp_before[inds == h][live]
            with np.errstate(invalid="ignore"):
                m = np.abs((d - 1.0) * np.log(zz[h][live]) + new_lp[h][live] - old - logu[h][live])
            self.least = min(self.least, float(np.min(m)))
            self.max_lp = max(self.max_lp, float(np.max(np.abs(new_lp[h][live]))), float(np.max(np.abs(old[np.isfinite(old)]), initial=0.0)))

    def check(self):
        assert self.least >= 100 * 1e-8 * self.max_lp, f"least accept margin {self.least:.3e}, max |lp| {self.max_lp:.3e}: take another seed"


def _oracle_step(case, X, lp, draws, margins):
    """SO.stretch_step in place, its margins recorded: a walker's log-probability before its half is the one before the step"""
    lp_before, seen = lp.copy(), []

    def fn(q):
        seen.append(case.lp(q))
        return seen[-1]
    acc = SO.stretch_step(X, lp, draws, fn)
    margins.add(X.shape[1], draws, lp_before, seen)
    return acc


def _oracle_run(case, X0, stream, steps, margins):
    """SO.run (chain, log-probabilities, acceptance counts) with the margins of every step"""
    X, lp = np.array(X0, dtype=np.float64), case.lp(X0)
    chain, lps, nacc = np.empty((steps,) + X.shape), np.empty((steps, X.shape[0])), np.zeros(X.shape[0], dtype=np.int64)
    for t in range(steps):
        nacc += _oracle_step(case, X, lp, stream.draw(X.shape[0]), margins)
        chain[t], lps[t] = X, lp
    return chain, lps, nacc


def _assert_equals_oracle(got, ochain, olps, onacc):
    compare_chains(got["chain"], got["lpchain"], ochain, olps)
    compare_chains(got["X"][None], got["lp"][None], ochain[-1:], olps[-1:])
    np.testing.assert_array_equal(got["nacc"], onacc)


def _forced_step(ds, X0, lp0, draws):
    """one host-RNG step of a used sampler from (X0, lp0): its snapshot, and what it added to live_counts"""
    ds.reset()
    ds.set_state(X0, lp0)
    before = ds.live_counts
    ds.step_host_rng(*draws)                                        # (raises on a NaN flag)
    after = ds.live_counts
    return _snapshot(ds, True), (after[0] - before[0], after[1] - before[1])


def _forced_against_oracle(case, dm, ds, X0, lp0, olp0, draws):
    """a forced step in the form the environment asks for, held to SO.stretch_step on the same draws; returns (snapshot, live)"""
    got, live = _forced_step(ds, X0, lp0, draws)
    Xo, lpo, margins = X0.copy(), olp0.copy(), _Margins()
    acc = _oracle_step(case, Xo, lpo, draws, margins)
    margins.check()
    _assert_equals_oracle(got, Xo[None], lpo[None], acc.astype(np.int64))
    return got, live


def _small_case(small, spec=None, block_start=None, ctx=contextlib.nullcontext):
    """the `small` fixture's design and data; with `spec`, its three PCs refitted in that kernel at fixed hyper-parameters"""
    model, prob = small
    if spec is not None:
        theta = np.log(np.r_[np.full(D, 0.5), [0.7] if spec.has_const else [], [0.05] if spec.has_noise else []])
        mean, scale, _ = O.scaler_fit(prob["Y"])
        ypca = O.pca_fit((prob["Y"] - mean) / scale)["Y_pca"]
        with ctx():
            gps = [O.gp_fit_at_theta(model.X_train, ypca[:, i], theta, spec, 1e-10) for i in range(K)]
        model = dataclasses.replace(model, spec=spec, gps=gps)
    return _Case(model, prob["y_exp"], prob["y_err"], LO, HI, block_start, ctx)


FORCED_SEED = 1000     # (the margin condition holds for these draws: _Margins)


@pytest.mark.parametrize("half", [0, 1])
def test_forced_live_counts_equal_oracle(small, half):
    """Live counts of 0, 1, around every 64- and 128-column boundary and all 260: the state after the compacted step is
    the oracle's stretch step on the same draws (positions, log-probabilities, -inf pattern, acceptances)."""
    from gpemu.sampler import DeviceSampler
    case = _small_case(small)
    X0 = np.random.default_rng(7).uniform(0.3, 0.7, (W, D))
    dm = case.device()
    lp0, olp0 = dm.logpost(X0), case.lp(X0)
    ds = DeviceSampler([dm], W, seed=1)
    other = 100
    for count in (0, 1, 63, 64, 65, 128, 129, 255, 256, W // 2):
        draws = _forced_draws(half, count, other, np.random.default_rng(FORCED_SEED + count))
        _, live = _forced_against_oracle(case, dm, ds, X0, lp0, olp0, draws)
        assert live == (count + other, W), count
    ds.close()
    dm.close()


def test_descending_and_alternating_counts(small, monkeypatch):
    """260, 65, 1, 0, 64, 256, 63 live proposals in half 0 (and the sequence backwards in half 1) on ONE sampler, another
    set of live proposals each time: after a larger count the buffers hold rows, cross-kernel blocks and partial sums of
    proposals that are dead now, and nothing of them may be read.  Both forms, bit for bit, and the oracle."""
    from gpemu.sampler import DeviceSampler
    case = _small_case(small)
    X0 = np.random.default_rng(17).uniform(0.3, 0.7, (W, D))
    dm = case.device()
    lp0, olp0 = dm.logpost(X0), case.lp(X0)
    ds = {on: DeviceSampler([dm], W, seed=1) for on in (True, False)}
    seq = (260, 65, 1, 0, 64, 256, 63)
    for i, (count, other) in enumerate(zip(seq, seq[::-1])):
        draws = _forced_draws(0, count, other, np.random.default_rng(FORCED_SEED + 100 + i))
        got = {}
        for on in (True, False):
            _form(monkeypatch, on)
            got[on], live = _forced_against_oracle(case, dm, ds[on], X0, lp0, olp0, draws)
            assert live == ((count + other, W) if on else (0, 0)), (count, on)
        _assert_same(got[True], got[False])
    for s in ds.values():
        s.close()
    dm.close()


def _stream_both_forms(case, monkeypatch, Wn, steps, seed, X0, oracle=True):
    """`steps` of the device stream in both forms (bit for bit) and, if asked, against the oracle's run of the same
    stream; returns (the compacted form's snapshot, its live_counts, its live_fraction)"""
    from gpemu.sampler import DeviceSampler
    got, live = {}, {}
    dm = case.device()
    for on in (True, False):
        _form(monkeypatch, on)
        ds = DeviceSampler([dm], Wn, seed=seed)
        ds.set_state(X0)
        ds.run(steps)
        got[on] = _snapshot(ds, True)
        live[on] = (ds.live_counts, ds.live_fraction)
        ds.close()
    dm.close()
    _assert_same(got[True], got[False])
    assert live[False] == ((0, 0), None)
    if oracle:
        margins = _Margins()
        ochain, olps, onacc = _oracle_run(case, X0, SO.PhiloxStream(seed), steps, margins)
        margins.check()
        _assert_equals_oracle(got[True], ochain, olps, onacc)
    return got[True], live[True][0], live[True][1]


def _compacted_in_box(case, Wn, seed, X0, chain):
    """(in-box proposals, proposals) of the chunks the half-step compacts, formed on the host from the stream's draws and
    the stored states: a half of more than 128 proposals goes in chunks of 2048, and a chunk of at most 128 runs as ever"""
    stream, prev, n_in, n_all = SO.PhiloxStream(seed), X0, 0, 0
    for cur in chain:
        inds, zz, rint, _ = stream.draw(Wn)
        mid = np.where((inds == 0)[:, None], cur, prev)                 # after half 0: only its walkers have moved
        for h, X in ((0, prev), (1, mid)):
            s, c = X[inds == h], X[inds != h]
            inside = case.inside(c[rint[h]] - (c[rint[h]] - s) * zz[h][:, None])
            if inside.size > 128:
                for lo in range(0, inside.size, 2048):
                    if inside[lo:lo + 2048].size > 128:
                        n_in += int(np.sum(inside[lo:lo + 2048]))
                        n_all += inside[lo:lo + 2048].size
        prev = cur
    return n_in, n_all


KINDS = {  # the cross-kernel's instances: RBF (with the constant term), the closed-form Materns, and kind 4 in its
    # direct-distance (nu < 1) and table (nu >= 1) branches
    "rbf_const": O.KernelSpec(kind=O.RBF, nu=np.inf, has_const=True, has_noise=True),
    "matern_0p5": O.KernelSpec(kind=O.MATERN, nu=0.5, has_const=False, has_noise=True),
    "matern_1p5": O.KernelSpec(kind=O.MATERN, nu=1.5, has_const=False, has_noise=True),
    "matern_2p5": O.KernelSpec(kind=O.MATERN, nu=2.5, has_const=False, has_noise=True),
    "matern_0p75": O.KernelSpec(kind=O.MATERN, nu=0.75, has_const=False, has_noise=True),
    "matern_3p5": O.KernelSpec(kind=O.MATERN, nu=3.5, has_const=False, has_noise=True),
}
KIND_SEED = {"rbf_const": 0xC0FFEE, "matern_0p5": 0xC0FFEE, "matern_1p5": 0xC0FFEE, "matern_2p5": 0xC0FFEE,
             "matern_0p75": 0xC0FFEE, "matern_3p5": 0xC0FFEE}


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_kinds_compacted(small, monkeypatch, kind):
    """Every kernel kind of the cross-kernel with halves of 260 (the Matern sampler tests elsewhere have halves of at most
    128, which never compact): 3 steps of the device stream from walkers all over the unit cube."""
    spec = KINDS[kind]
    general = spec.kind == O.MATERN and spec.nu not in (0.5, 1.5, 2.5)
    case = _small_case(small, spec, ctx=R.general_nu if general else contextlib.nullcontext)
    X0 = np.random.default_rng(5).uniform(0.0, 1.0, (W, D))
    _, counts, frac = _stream_both_forms(case, monkeypatch, W, 3, KIND_SEED[kind], X0)
    assert counts[1] == 3 * W and 0.2 < frac < 0.95


@pytest.fixture(scope="module")
def wide():
    """12 parameters (the 16-wide instance of propose_compact_kernel), 130 design points, 3 PCs: test_gpu_wide_d's builder"""
    from test_gpu_wide_d import _problem
    model, prob = _problem(N, 12, F, K, seed=52)
    return _Case(model, prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"])


def test_wide_forced_counts_equal_oracle(wide, monkeypatch):
    from gpemu.sampler import DeviceSampler
    case = wide
    span = case.hi - case.lo
    X0 = np.random.default_rng(27).uniform(case.lo + 0.3 * span, case.hi - 0.3 * span, (W, case.d))
    dm = case.device()
    lp0, olp0 = dm.logpost(X0), case.lp(X0)
    assert np.all(np.isfinite(lp0))
    ds = {on: DeviceSampler([dm], W, seed=1) for on in (True, False)}
    for count in (0, 1, 64, 65, 129, W // 2):
        draws = _forced_draws(0, count, 100, np.random.default_rng(FORCED_SEED + 200 + count))
        got = {}
        for on in (True, False):
            _form(monkeypatch, on)
            got[on], live = _forced_against_oracle(case, dm, ds[on], X0, lp0, olp0, draws)
            assert live == ((count + 100, W) if on else (0, 0)), (count, on)
        _assert_same(got[True], got[False])
    for s in ds.values():
        s.close()
    dm.close()


def test_wide_proposals_on_the_faces_are_outside(wide, monkeypatch):
    """The face test at 12 parameters, the face coordinates (9 on lo, 11 on hi) in the upper half of the 16-wide rows."""
    from gpemu.sampler import DeviceSampler
    case = wide
    span = case.hi - case.lo
    X0 = np.random.default_rng(29).uniform(case.lo + 0.3 * span, case.hi - 0.3 * span, (W, case.d))
    inds = (np.arange(W) % 2).astype(np.int32)
    X0[[0, 1], 9] = case.lo[9]
    X0[[2, 3], 11] = case.hi[11]
    ns = W // 2
    rint = [np.arange(ns, dtype=np.int64), np.arange(ns, dtype=np.int64)]     # proposal i of a half pairs walkers 2 i, 2 i + 1
    zz = [np.full(ns, 1.0), np.full(ns, 1.0)]
    zz[0][:2] = zz[1][:2] = 1.75
    logu = [np.log(np.random.default_rng(3).uniform(0.0, 1.0, ns)) for _ in range(2)]
    draws = (inds, zz, rint, logu)
    dm = case.device()
    lp0, olp0 = dm.logpost(X0), case.lp(X0)
    assert np.all(np.isneginf(lp0[:4])) and np.all(np.isfinite(lp0[4:]))
    got = {}
    for on in (True, False):
        _form(monkeypatch, on)
        ds = DeviceSampler([dm], W, seed=1)
        got[on], live = _forced_against_oracle(case, dm, ds, X0, lp0, olp0, draws)
        assert live == ((W - 4, W) if on else (0, 0))
        ds.close()
    dm.close()
    _assert_same(got[True], got[False])
    np.testing.assert_array_equal(got[True]["X"][:4], X0[:4])
    assert not np.any(got[True]["nacc"][:4])


CHUNK_SEED = {258: 0xC0FFEE, 256: 0xC0FFEE, 521: 0xC0FFEE, 4097: 0xC0FFEE, 4352: 0xC0FFEE, 4354: 0xC0FFEE}


@pytest.mark.parametrize("Wn", [258, 256, 521, 4097, 4352, 4354])
def test_chunks_and_sizes(small, monkeypatch, Wn):
    """Halves of 129 (the smallest compacted launch: 2 column blocks, every item halved) and of 128 (never compacted),
    unequal halves, and halves that go in two chunks: 2048 + 1 and 2048 + 128 (the second chunk as ever) and 2048 + 129
    (the second chunk compacted, at two column blocks).  2 steps of the device stream."""
    case = _small_case(small)
    X0 = np.random.default_rng(Wn).uniform(0.0, 1.0, (Wn, D))
    got, counts, _ = _stream_both_forms(case, monkeypatch, Wn, 2, CHUNK_SEED[Wn], X0, oracle=Wn in (258, 4352))
    assert counts == _compacted_in_box(case, Wn, CHUNK_SEED[Wn], X0, got["chain"])
    expect = {258: 2 * 258, 256: 0, 521: 2 * 521, 4097: 2 * 4096, 4352: 2 * 4096, 4354: 2 * 4354}[Wn]
    assert counts[1] == expect and (expect == 0 or 0 < counts[0] < expect)


@pytest.mark.parametrize("k", [17, 40])
def test_many_pcs_compacted(monkeypatch, k):
    """17 PCs (the likelihood's 32-wide register form) and 40 (its LDS form) read their sums through slot_of"""
    from gpemu.sampler import DeviceSampler
    model, prob, _ = GU.fixed_theta_model(N, 60, k, seed=3)
    span = prob["hi"] - prob["lo"]
    case = _Case(model, prob["y_exp"], prob["y_err"], prob["lo"] + 0.2 * span, prob["hi"] - 0.2 * span)
    rng = np.random.default_rng(31 + k)
    X0 = rng.uniform(case.lo + 0.1 * span, case.hi - 0.1 * span, (W, case.d))
    dm = case.device()
    lp0, olp0 = dm.logpost(X0), case.lp(X0)
    ds = DeviceSampler([dm], W, seed=1)
    for count in (0, 65, W // 2):
        draws = _forced_draws(1, count, 100, np.random.default_rng(FORCED_SEED + 300 + count))
        _, live = _forced_against_oracle(case, dm, ds, X0, lp0, olp0, draws)
        assert live == (count + 100, W), count           # (the compacted form ran)
    ds.close()
    dm.close()
    Xs = rng.uniform(prob["lo"], prob["hi"], (W, case.d))
    _, counts, _ = _stream_both_forms(case, monkeypatch, W, 3, 0xC0FFEE, Xs, oracle=False)
    assert counts[1] == 3 * W and 0 < counts[0] < 3 * W


def test_two_observable_blocks_compacted(small):
    """Two observable blocks and 260 proposals per half: more rows than the tasks kernel takes at fewer than 8 blocks, so
    the blocks' likelihood of one wave per proposal runs compacted."""
    from gpemu.sampler import DeviceSampler
    case = _small_case(small, block_start=TWO_BLOCKS)
    X0 = np.random.default_rng(37).uniform(0.3, 0.7, (W, D))
    dm = case.device()
    lp0, olp0 = dm.logpost(X0), case.lp(X0)
    ds = DeviceSampler([dm], W, seed=1)
    for count in (1, 129):
        draws = _forced_draws(0, count, 100, np.random.default_rng(FORCED_SEED + 450 + count))   # (+ 400: a margin of 9e-5 at 129)
        _, live = _forced_against_oracle(case, dm, ds, X0, lp0, olp0, draws)
        assert live == (count + 100, W), count
    ds.close()
    dm.close()


def _forced_forms(monkeypatch, dm, Wn, X0, counts, seed0):
    """each count forced in both halves, in the default form, forms 0 and 1 and uncompacted: bit for bit"""
    from gpemu.sampler import DeviceSampler
    lp0 = dm.logpost(X0)
    variants = ("default", "0", "1", "off")
    ds = {v: DeviceSampler([dm], Wn, seed=1) for v in variants}
    for count in counts:
        draws = _forced_draws(0, count, count, np.random.default_rng(seed0 + count), W=Wn)
        got = {}
        for v in variants:
            _form(monkeypatch, v != "off")
            if v in ("0", "1"):
                monkeypatch.setenv("GPEMU_COMPACT_FORM", v)
            else:
                monkeypatch.delenv("GPEMU_COMPACT_FORM", raising=False)
            got[v], live = _forced_step(ds[v], X0, lp0, draws)
            assert live == ((2 * count, Wn) if v != "off" else (0, 0)), (count, v)
        monkeypatch.delenv("GPEMU_COMPACT_FORM", raising=False)
        for v in variants[1:]:
            _assert_same(got["default"], got[v])
    for s in ds.values():
        s.close()


def test_forced_forms_small(small, monkeypatch):
    """GPEMU_COMPACT_FORM = 0 (the whole batch's schedule, also the fall-back of the others) and 1 (its placement without
    the dead blocks) against the default form and the uncompacted step"""
    dm = _device_model(small)
    X0 = np.random.default_rng(41).uniform(0.3, 0.7, (W, D))
    _forced_forms(monkeypatch, dm, W, X0, (1, 65, 129, 260), 3000)
    dm.close()


def test_forced_forms_headline_size(c3, monkeypatch):
    """the same at the benchmark's shape, where the default form deals the live blocks to the XCDs by cost"""
    from gpemu import synthetic
    dm, prob = c3
    lo, hi = prob["lo"], prob["hi"]
    X0 = synthetic.make_walkers(1024, seed=1, lo=lo + 0.1 * (hi - lo), hi=hi - 0.1 * (hi - lo))
    _forced_forms(monkeypatch, dm, 1024, X0, (1, 65, 193, 321, 449), 4000)
