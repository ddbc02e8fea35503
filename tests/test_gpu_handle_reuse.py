"""-m gpu: a used model handle must give a fresh handle's bits.

One gpemu_model lives for a whole analysis and is called in arbitrary order by logpost, predict, gradients, the samplers,
the chain summaries and the design, which share state that lives on the handle and not in the call: the workspace (its
capacity is the row stride of K_*^T, its padding rows keep what an earlier call left), the per-model caches (schedules,
likelihood constants keyed by n_div, bounded with eviction), fields a sampler writes on the model during a call, and the
handles of several samplers on one model.  Every assertion here is bit equality (np.array_equal on the int64 view, NaN
patterns included) with the same call on a freshly created handle; the fresh handle's values are held to the
extended-precision references elsewhere (test_gpu_paths.py, test_gpu_wide_d.py, test_gpu_srccorr.py, ...).  The cases and
the operations are in tests/reuse_cases.py.
"""
import numpy as np
import pytest

import golden_util as GU
import reuse_cases as RC

pytestmark = pytest.mark.gpu

_FRESH = {}


def fresh_results(name):
    """every operation of the case on its own freshly created handle (computed once, shared, left unchanged)"""
    if name not in _FRESH:
        P = RC.problem(name)
        out = {}
        for op in RC.ops_of(name):
            dm = RC.fresh(P)
            out[op.name] = RC.run_op(op, dm, P)
            dm.close()
        _FRESH[name] = out
    return _FRESH[name]


def on_fresh(P, fn, setup=None):
    dm = RC.fresh(P, setup)
    try:
        return fn(dm)
    finally:
        dm.close()


def assert_bits(what, got, want):
    got, want = RC.flatten(got), RC.flatten(want)
    assert len(got) == len(want) and len(want) > 0, f"{what}: {len(got)} arrays, {len(want)} on a fresh handle"
    for i, (a, b) in enumerate(zip(got, want)):
        assert RC.same_bits(a, b), f"{what}: array {i} (shape {np.shape(a)}) differs from a fresh handle's"


# ---- 1. order independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.CASE_IDS)
def test_order_independence(name):
    """every operation in table order, in reverse and in two seeded shuffles on ONE long-lived handle: the workspace grows
    (B = 1 -> 600 -> 2049) and is reused far below its capacity (stride Bcap != round_up(B)), every cache hits and misses,
    cur_nchunk passes between the launch families"""
    P = RC.problem(name)
    ops = RC.ops_of(name)
    want = fresh_results(name)
    orders = {"table": list(range(len(ops))), "reverse": list(range(len(ops)))[::-1]}
    for seed in (1, 2):
        orders[f"shuffle{seed}"] = [int(i) for i in np.random.default_rng(seed).permutation(len(ops))]
    dm = RC.fresh(P)
    try:
        for label, order in orders.items():
            _run_in_order(name, P, dm, ops, order, want, label)
    finally:
        dm.close()


def _run_in_order(name, P, dm, ops, order, want, label):
    """the operations in this order on the used handle, each against its fresh result; every pair either compares or is a
    documented decline, and at least MIN_COMPARED of them compare"""
    compared = 0
    for pos, i in enumerate(order):
        op = ops[i]
        got = RC.run_op(op, dm, P)
        before = [ops[j].name for j in order[max(0, pos - 3):pos]]
        compared += RC.assert_same(name, op, got, want[op.name], f"order {label}, after {before}")
    assert compared >= RC.MIN_COMPARED, f"{name}: only {compared} operations compare"
    assert compared + sum(1 for op in ops if (name, op.name) in RC.DECLINES) == len(ops)


# ---- 2. padding dirtied by legitimate calls ------------------------------------------------------------------------------
def _raw_gp_predict(dm, X):
    """gpemu_gp_predict itself: the C entry does not check the rows (DeviceModel.gp_predict refuses non-finite ones)"""
    from gpemu import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    mean, var = np.empty((X.shape[0], dm.k)), np.empty((X.shape[0], dm.k))
    _lib.check(_lib.lib().gpemu_gp_predict(dm.handle, X.shape[0], _lib.ptr(X), _lib.ptr(mean), _lib.ptr(var)))
    return mean, var


def _sampler_200(dm, P):
    ds = RC.stretch_sampler(dm, P, 200, seed=17)
    try:
        ds.run(2)
        return RC.sampler_result(ds)
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["general", "halfstep", "wide"])
def test_padding_dirtied_by_legitimate_calls(name):
    """B = 128 with rows 100 .. 127 NaN, +inf, 1e300 and far outside the box, then B = 100 and 97 and a sampler with
    halves of 100 that reuse those rows of Xq / K_*^T: everything as on a fresh handle, no NaN flag in the sampler"""
    P = RC.problem(name)
    far = P.hi + 3.0 * (P.hi - P.lo)
    dm = RC.fresh(P)
    try:
        for label, poison in (("nan", np.nan), ("inf", np.inf), ("1e300", 1e300), ("outside", far)):
            X = RC.rows(P, f"dirty_{label}", 128)
            X[100:] = poison
            assert_bits(f"{name}: logpost with {label} rows", dm.logpost(X), on_fresh(P, lambda f: f.logpost(X)))
            assert_bits(f"{name}: gp_predict with {label} rows", _raw_gp_predict(dm, X),
                        on_fresh(P, lambda f: _raw_gp_predict(f, X)))
            for B in (100, 97):
                Xb = RC.rows(P, f"after_{label}_{B}", B)
                assert_bits(f"{name}: logpost({B}) after {label} rows", dm.logpost(Xb), on_fresh(P, lambda f: f.logpost(Xb)))
                assert_bits(f"{name}: gp_predict({B}) after {label} rows", dm.gp_predict(Xb),
                            on_fresh(P, lambda f: f.gp_predict(Xb)))
            got = _sampler_200(dm, P)
            assert got[5][2] == 0, f"{name}: the sampler flagged a NaN log-probability after {label} rows"
            assert np.all(np.isfinite(got[1])), f"{name}: non-finite stored log-probabilities after {label} rows"
            assert_bits(f"{name}: sampler after {label} rows", got, on_fresh(P, lambda f: _sampler_200(f, P)))
    finally:
        dm.close()


# ---- 3. likelihood re-setup ----------------------------------------------------------------------------------------------
def _resetup_results(dm, P, chains):
    Q = RC.Problem(P.name, P.case, P.model, P.lo, P.hi, dict(y_exp=P.Y[:chains] if chains > 1 else P.Y[0]), P.Y, P.y_err,
                   P.block_start)                    # (the sampler's chains follow the setup's data vectors)
    ds = RC.stretch_sampler(dm, Q, 300, seed=23)
    try:
        ds.run(2)
        return (dm.logpost(RC.logpost_rows(P, 33)), dm.logpost(RC.logpost_rows(P, 129))) + RC.sampler_result(ds)
    finally:
        ds.close()


def _pending_sampler(dm, P, chains):
    """a sampler created now and run after the next setup"""
    from gpemu.sampler import DeviceSampler
    return DeviceSampler([dm], 300, **(dict(seed=29) if chains == 1 else dict(seeds=[29, 30, 31][:chains])))


def _run_pending(ds, P):
    ds.set_state(RC.walkers(P, "pending", ds.W))
    ds.run(2)
    return RC.sampler_result(ds)


def test_likelihood_resetup():
    """one model walked through the setups; after each, logpost and a 2-step sampler equal a fresh model given only that
    setup, and so does a sampler created BEFORE the setup and run after it: a call uses the setup current at the call
    (include/gpemu.h).  n_div runs through 70 values: the cache of likelihood constants holds 64 and drops the oldest, so
    `n_div = 1 again` is a miss that rebuilds an evicted entry.  The setups after it are the cache HITS, each swapping
    G / g0 / scal to an entry other than the current one: the newest (70), the rebuilt one (1), one that survived in the
    middle of the vector the evictions shifted (30); then the same under sources, whose hits swap W / Q / w0 too."""
    from gpemu._lib import GpemuError
    P = RC.problem("general")
    V = lambda kind, n_div=1.0: RC.setup_variant(P, kind, n_div=n_div)
    # (label, setup, data vectors, checked in full)
    walk = [("chains", V("chains"), 3, True), ("single", V("single"), 1, True), ("sources", V("sources"), 1, True),
            ("diagonal", V("diagonal"), 1, True), ("blocks2", V("blocks2"), 1, True), ("block1", V("block1"), 1, True),
            ("chains again", V("chains"), 3, True)]      # (a one-chain sampler created before it: vector 0)
    checked_divs = {1, 2, 3, 64, 65, 66, 70}             # the others enter the cache all the same
    walk += [(f"n_div={v}", V("block1", float(v)), 1, v in checked_divs) for v in range(1, 71)]
    walk += [("n_div=1 again (rebuilt)", V("block1", 1.0), 1, True)]
    walk += [(f"n_div={v} (hit)", V("block1", float(v)), 1, True) for v in (70, 1, 30)]
    walk += [(f"sources n_div={v}", V("sources", float(v)), 1, True) for v in (1, 2)]
    walk += [(f"sources n_div={v} (hit)", V("sources", float(v)), 1, True) for v in (1, 2)]
    dm = RC.fresh(P, walk[0][1])
    pending, pending_chains = None, 0
    try:
        for label, setup, chains, full in walk:
            RC.apply_setup(dm, setup)
            if not full:
                continue
            assert_bits(f"after setup {label}", _resetup_results(dm, P, chains),
                        on_fresh(P, lambda f: _resetup_results(f, P, chains), setup))
            if pending is not None:
                # created under the previous setup, run under this one: 3 stacked chains on what is now ONE data vector
                # serve every chain with it; one chain on three vectors uses vector 0
                got = _run_pending(pending, P)
                pending.close()
                pending = None

                def alone(f):
                    ds = _pending_sampler(f, P, pending_chains)
                    try:
                        return _run_pending(ds, P)
                    finally:
                        ds.close()
                # (one chain cannot be CREATED on three vectors: its reference is a model given vector 0 alone)
                want = on_fresh(P, alone, setup if pending_chains >= chains else dict(setup, y_exp=setup["y_exp"][0].copy()))
                assert_bits(f"a sampler of {pending_chains} chain(s) created before setup {label}", got, want)
                if pending_chains != chains:         # every chain on one vector (the only one, or vector 0 of three): the
                    X, lp = got[2], got[3]           # model's own log-posterior of the state
                    ref = dm.logpost(X)
                    fin = np.isfinite(ref)
                    assert np.array_equal(np.isfinite(lp), fin)
                    np.testing.assert_allclose(lp[fin], ref[fin], rtol=1e-9)
            pending, pending_chains = _pending_sampler(dm, P, chains), chains
        # fewer data vectors than a live sampler has chains: refused before anything is copied or launched, the sampler
        # is left as it was
        RC.apply_setup(dm, V("chains"))
        stacked = _pending_sampler(dm, P, 3)
        stacked.set_state(RC.walkers(P, "pending", stacked.W))
        before = RC.sampler_result(stacked)
        RC.apply_setup(dm, dict(V("chains"), y_exp=P.Y[:2].copy()))
        for call in (lambda: stacked.set_state(RC.walkers(P, "refused", stacked.W)), lambda: stacked.run(1)):
            with pytest.raises(GpemuError) as err:
                call()
            assert err.value.code == RC.ERR_STATE
        assert_bits("a refused sampler's state", RC.sampler_result(stacked), before)
        stacked.close()
    finally:
        if pending is not None:
            pending.close()
        dm.close()


# ---- 4. handles sharing a model, interleaved -----------------------------------------------------------------------------
NAMES = ("stretch", "hmc", "tempered", "design")


class Party:
    """the four kinds of handle on one set of models, each advanced one step or one pick at a time"""

    def __init__(self, dms, lo, hi, names, W):
        from gpemu.design import Design
        from gpemu.sampler import DeviceSampler, HMCSampler, TemperedSampler
        rng = np.random.default_rng(77)
        w = hi - lo
        box = lambda n: rng.uniform(lo + 0.02 * w, hi - 0.02 * w, (n, lo.size))
        X0 = {"stretch": box(W), "hmc": box(16), "tempered": box(48)}
        ref, cand = box(200), box(70)
        self.h, self.scores = {}, []
        if "stretch" in names:
            self.h["stretch"] = DeviceSampler(dms, W, seed=11)
        if "hmc" in names:
            self.h["hmc"] = HMCSampler(dms, 16, n_leapfrog=3, step_size=0.05, seed=8)
        if "tempered" in names:
            self.h["tempered"] = TemperedSampler(dms, 24, [1.0, 0.5], seed=5, swap_every=1)
        if "design" in names:
            self.h["design"] = Design(dms, ref, cand, max_picks=8)
        for n in ("stretch", "hmc", "tempered"):
            if n in self.h:
                self.h[n].set_state(X0[n])

    def step(self, name):
        if name == "design":
            s = self.h[name].scores()
            self.scores.append(s)
            self.h[name].condition(int(np.argmax(s)))
        else:
            self.h[name].run(1)

    def result(self, name):
        if name == "design":
            return tuple(self.scores) + (self.h[name].scores(),)
        return RC.sampler_result(self.h[name])

    def close(self):
        for h in self.h.values():
            h.close()


def _interleaved(make_models, lo, hi, W, between):
    """the four handles round-robin on one set of models, with `between(dms, i)` called twice a round, against each
    handle alone on fresh models"""
    ROUNDS = 3
    alone = {}
    for n in NAMES:
        dms = make_models()
        p = Party(dms, lo, hi, (n,), W)
        for _ in range(ROUNDS):
            p.step(n)
        alone[n] = p.result(n)
        p.close()
        for dm in dms:
            dm.close()
    dms = make_models()
    p = Party(dms, lo, hi, NAMES, W)
    i = 0
    for _ in range(ROUNDS):
        for j, n in enumerate(NAMES):
            p.step(n)
            if j in (0, 2):
                between(dms, i)
                i += 1
    for n in NAMES:
        assert_bits(f"{n} handle interleaved with the others", p.result(n), alone[n])
    p.close()
    for dm in dms:
        dm.close()


def test_handles_sharing_one_model():
    """a compacted stretch sampler, an HMC sampler, a tempered sampler and a design handle on ONE model, advanced in
    turn, while logpost at a batch larger than any so far frees and reallocates the workspace between their steps"""
    P = RC.problem("general")

    def between(dms, i):
        B = 700 + 160 * i
        X = RC.rows(P, f"between{B}", B)
        assert_bits(f"logpost({B}) between the handles' steps", dms[0].logpost(X), on_fresh(P, lambda f: f.logpost(X)))

    _interleaved(lambda: [RC.fresh(P)], P.lo, P.hi, 300, between)


def test_handles_sharing_three_groups():
    """the same over the three-group set (5 / 11 / 25 PCs): the groups' workspaces are driven from group 0's stream;
    logpost on group 0 regrows its workspace, logpost on group 2's model alone goes between the steps too"""
    from gpemu import synthetic
    groups = [GU.fixed_theta_model(150, F, k, seed=gi) for gi, (F, k) in enumerate([(40, 5), (60, 11), (90, 25)])]
    lo, hi = groups[0][1]["lo"], groups[0][1]["hi"]

    def one(gi):
        model, prob, _ = groups[gi]
        dm = GU.device_model(model)
        dm.likelihood_setup(prob["y_exp"], prob["y_err"], prob["lo"], prob["hi"], 1.0)
        return dm

    def make_models():
        return [one(gi) for gi in range(3)]

    def fresh_logpost(gi, X):
        dm = one(gi)
        try:
            return dm.logpost(X)
        finally:
            dm.close()

    def between(dms, i):
        B = 300 + 130 * i
        X = synthetic.make_walkers(B, seed=40 + i, lo=lo, hi=hi)
        assert_bits(f"logpost({B}) on group 0 between the steps", dms[0].logpost(X), fresh_logpost(0, X))
        X2 = synthetic.make_walkers(77 + 64 * i, seed=60 + i, lo=lo, hi=hi)
        assert_bits("logpost on group 2 alone between the steps", dms[2].logpost(X2), fresh_logpost(2, X2))

    _interleaved(make_models, lo, hi, 200, between)


# ---- 5. close and re-create ----------------------------------------------------------------------------------------------
def test_close_and_recreate():
    """a model destroyed and another case created in the same process, five times over: the process-wide state (the set
    of kernels allowed large dynamic LDS, the thread's deal table of the tasks kernel) does not remember the last model"""
    picks = ("logpost_33", "logpost_128", "logpost_257", "logpost_600", "gp_predict", "loglik_pointwise", "stretch_24",
             "stretch_300", "run_peer")
    first = {}
    for rnd in range(5):
        for name in ("tasks10", "halfstep"):
            P = RC.problem(name)
            dm = RC.fresh(P)
            try:
                for opn in picks:
                    got = RC.run_op(RC.OP[opn], dm, P)
                    if rnd == 0:
                        assert got[0] == "ok", f"{name}/{opn}: {got[1:]}"
                        first[name, opn] = got
                    else:
                        RC.assert_same(name, RC.OP[opn], got, first[name, opn], f"creation {rnd + 1}")
            finally:
                dm.close()
