"""-m gpu: the library's device resources balance, and an allocation that is refused costs nothing and breaks nothing.

csrc/devmem.h owns every device allocation of the library and feeds one ledger (csrc/devledger.h): live blocks and
bytes, allocations and frees so far, live streams and events.  gpemu_devmem_refuse_nth makes the n-th allocation from
now fail on the host, before the allocator is called.  With the two, every early return of an allocation is reachable:
  a. balance   -- every operation of tests/reuse_cases.py, every device-wide row of tests/stream_cases.py, the host
                  one-shots, the fit / diag / design handles, the samplers' chain summaries, snapshot / restore / reset
                  and the drop-in's model cache leave the ledger where they found it once everything is closed;
  b. a call the library declines allocates nothing (reuse_cases.DECLINES and the bad arguments of the feature tests,
                  watched call by call while those tests run);
  c. warm      -- the third of three identical calls allocates exactly what devmem_cases' table says (0 for a sampler's
                  run after reserve and for every `_dev` entry that does not wait), and leaves the live bytes alone;
  d. the walk  -- create + likelihood_setup and every operation of three cases, armed at every j up to the number of
                  allocations they make: each j fires, raises "refused", leaks nothing, and the surviving handle then gives
                  a fresh handle's bits; the sampler's setters leave state, counts and chain as they were;
  e. the ledger itself moves up and back with a model.
Every assertion is an equality of integers or of bits.  The operations are in tests/devmem_cases.py and the tables it
borrows.
"""
import importlib
import os

import numpy as np
import pytest

import devmem_cases as DC
import golden_util as GU
import reuse_cases as RC
import stream_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _disarm():
    """no test of this module leaves a refusal armed, however it ends"""
    from gpemu import _lib
    yield
    assert not _lib.devmem_refuse_nth(0), "a test left the refusal armed"


def _lib():
    from gpemu import _lib as L
    return L


def _pairs(cases):
    return [(c, op.name) for c in cases for op in RC.ops_of(c)]


def _pid(p):
    return f"{p[0]}-{p[1]}"


# ---- e. the ledger itself ----------------------------------------------------------------------------------------------
def test_ledger_moves_with_a_model():
    P = RC.problem("general")
    base = DC.reading()
    dm = GU.device_model(P.model)
    made = DC.reading()
    assert made["live_blocks"] > base["live_blocks"] and made["live_bytes"] > base["live_bytes"]
    assert made["live_streams"] == base["live_streams"] + 1
    assert made["allocs"] - base["allocs"] >= made["live_blocks"] - base["live_blocks"]
    RC.apply_setup(dm, P.setup)
    assert DC.reading()["live_blocks"] > made["live_blocks"]
    dm.close()
    DC.assert_back_to(base, "a model created, set up and closed")
    # the two calls themselves
    L = _lib()
    assert L.lib().gpemu_devmem_stats(None, 0) == DC.ERR_ARG
    assert L.lib().gpemu_devmem_refuse_nth(-1, None) == DC.ERR_ARG
    assert L.devmem_refuse_nth(5) is False and L.devmem_refuse_nth(0) is True and L.devmem_refuse_nth(0) is False
    with L.devmem_refusing(1) as r:
        msg = DC.refused(lambda: GU.device_model(P.model))
    assert r.fired and "bytes" in msg
    DC.assert_back_to(base, "a model whose first allocation was refused")


# ---- a. balance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", _pairs(RC.CASE_IDS), ids=_pid)
def test_balance_of_every_operation(pair):
    case, opn = pair
    P = RC.problem(case)
    base = DC.reading()
    dm = RC.fresh(P)
    try:
        got = RC.run_op(RC.OP[opn], dm, P)
        again = RC.run_op(RC.OP[opn], dm, P)
    finally:
        dm.close()
    RC.assert_same(case, RC.OP[opn], again, got, "the second call on the handle")
    del got, again
    DC.assert_back_to(base, f"{case}/{opn}")


@pytest.mark.parametrize("row", DC.DEVICE_WIDE_ROWS, ids=lambda r: r.name.replace("gpemu_", ""))
def test_balance_and_warm_count_of_the_device_wide_rows(row):
    """no handle: whatever a one-shot allocates goes with the call, and the third call allocates what the first did"""
    base = DC.reading()
    counts = [DC.allocs_of(lambda: DC.run_wide_row(row))[1] for _ in range(3)]
    print(f"[devmem] {row.name}: allocations of three calls {counts}")
    DC.assert_back_to(base, row.name)
    assert counts[0] == counts[1] == counts[2], f"{row.name}: the calls allocate {counts}"


@pytest.mark.parametrize("name", list(DC.HOST_ONE_SHOTS))
def test_balance_of_the_host_one_shots(name):
    base = DC.reading()
    fn = DC.HOST_ONE_SHOTS[name]
    (first, n1), (second, n2) = DC.allocs_of(fn), DC.allocs_of(fn)
    print(f"[devmem] {name}: allocations of two calls {[n1, n2]}")
    assert n1 == n2 and n1 > 0, f"{name}: the calls allocate {[n1, n2]}"
    SC.assert_same(name, second, first)
    DC.assert_back_to(base, name)


def test_balance_of_the_fit_handle():
    c, X, ys, thetas = DC.fit_problem()
    base = DC.reading()
    f = DC.device_fit(c, X)
    made = DC.reading()
    assert made["live_streams"] == base["live_streams"] + 2 and made["live_events"] == base["live_events"] + 2
    res = {}
    for step, fn in DC.FIT_STEPS.items():
        res[step], n = DC.allocs_of(lambda: fn(f, ys, thetas))
        print(f"[devmem] DeviceFit.{step}: {n} allocations")
    # warm: every step again allocates nothing, and gives the same bits
    before = DC.reading()
    for step, fn in DC.FIT_STEPS.items():
        again, n = DC.allocs_of(lambda: fn(f, ys, thetas))
        assert n == 0, f"DeviceFit.{step}: {n} allocations on a handle that has run it"
        SC.assert_same(f"DeviceFit.{step} again", again, res[step])
    assert DC.live(DC.reading()) == DC.live(before)
    f.close()
    DC.assert_back_to(base, "a fit handle through lml, lml_batch (1, then 5 problems) and factor")


def test_balance_of_the_diag_and_design_handles():
    P = RC.problem("general")
    base = DC.reading()
    first = DC.diag_run()
    SC.assert_same("the diag handle again", DC.diag_run(), first)
    DC.assert_back_to(base, "a diag handle through its calls")
    dm = RC.fresh(P)
    mid = DC.reading()
    first = DC.design_run(dm, P)
    SC.assert_same("the design handle again", DC.design_run(dm, P), first)
    DC.assert_back_to(mid, "a design handle through scores, condition and state")
    dm.close()
    DC.assert_back_to(base, "the model of the design handle")


CHAIN_PARAMS = [(kind, m) for kind in ("stretch", "tempered", "hmc") for m in DC.CHAIN_METHODS]


@pytest.fixture(scope="module")
def chain_samplers():
    """one sampler of each kind on the general case with a stored chain, shared by the chain-summary tests"""
    P = RC.problem("general")
    made = {}

    def get(kind):
        if kind not in made:
            dm = RC.fresh(P)
            made[kind] = (dm, DC.chain_sampler(dm, P, kind))
        return made[kind]
    yield get
    for dm, ds in made.values():
        ds.close()
        dm.close()


@pytest.mark.parametrize("kind,method", CHAIN_PARAMS, ids=[f"{k}-{m}" for k, m in CHAIN_PARAMS])
def test_balance_of_the_chain_summaries(kind, method, chain_samplers):
    """a summary of the stored chain leaves nothing behind on a live sampler: its temporary diag / design handles and
    device buffers are gone when it returns; the second call gives the first's bits"""
    P = RC.problem("general")
    dm, ds = chain_samplers(kind)
    fn = DC.CHAIN_METHODS[method]
    first = RC.flatten(fn(ds, P))       # (the first call may grow the model's workspace: that belongs to the handle)
    base = DC.reading()
    second, n = DC.allocs_of(lambda: RC.flatten(fn(ds, P)))
    print(f"[devmem] {kind}.{method}: {n} allocations on the second call")
    SC.assert_same(f"{kind}.{method} again", tuple(np.asarray(a) for a in second), tuple(np.asarray(a) for a in first))
    del first, second
    DC.assert_back_to(base, f"{kind}.{method}")


@pytest.mark.parametrize("kind", ["stretch", "tempered", "hmc"])
def test_balance_of_a_sampler_through_its_life(kind):
    """create, set_state, a run that grows the chain past its first 256 steps (ensure_chain moves the buffer once),
    snapshot, run, restore, reset, run, the summaries' handles, close: the ledger is back where it was"""
    P = RC.problem("general")
    base = DC.reading()
    dm = RC.fresh(P)
    ds = {"stretch": lambda: RC.stretch_sampler(dm, P, DC.CHAIN_W, seed=13), "tempered": lambda: RC.tempered_sampler(dm, P),
          "hmc": lambda: RC.hmc_sampler(dm, P)}[kind]()
    try:
        ds.run(200)
        cap1 = DC.reading()
        ds.run(100)                      # 300 > 256 stored steps: the chain moved to a buffer twice the size
        cap2 = DC.reading()
        assert cap2["live_blocks"] == cap1["live_blocks"] and cap2["live_bytes"] > cap1["live_bytes"]
        assert cap2["allocs"] - cap1["allocs"] == 2 and cap2["frees"] - cap1["frees"] == 2
        L = _lib().lib()
        _lib().check(L.gpemu_sampler_snapshot(ds._h))
        kept = RC.sampler_result(ds)
        ds.run(3)
        _lib().check(L.gpemu_sampler_restore(ds._h))
        RC.assert_same("general", RC.Op("restore", None), ("ok", RC.sampler_result(ds)), ("ok", kept), "after restore")
        ds.reset()
        ds.run(2)
        assert ds.counts()[2] == 2
    finally:
        ds.close()
    # (what the runs grew on the model -- its workspace, its schedules -- belongs to the model and goes with it)
    after = DC.reading()
    assert after["live_streams"] == base["live_streams"] + 1 and after["live_events"] == base["live_events"]
    dm.close()
    DC.assert_back_to(base, f"a {kind} sampler through its life, and its model")


def test_balance_of_the_dropin_model_cache(monkeypatch):
    """GPEMU_MODEL_CACHE=1 and three models in turn: the two that were evicted are gone from the ledger"""
    em = importlib.import_module("bayesian_inference.emulation")
    monkeypatch.setenv("GPEMU_MODEL_CACHE", "1")
    em.release_device_models()
    base = DC.reading()
    one = None
    results = []
    for name in ("general", "tasks10", "halfstep"):
        P = RC.problem(name)
        res, cov = DC.dropin_results(P.model)
        results.append(res)              # (the cache keys on the dict's identity: keep them alive)
        before = DC.reading()
        dm = em.device_model_for(res, P.k, cov)
        assert em.device_model_for(res, P.k, cov) is dm
        X = RC.rows(P, "dropin_cache", 9)
        assert np.all(np.isfinite(dm.gp_predict(X)[0]))
        del dm
        now = DC.reading()
        if one is None:
            one = now["live_streams"] - before["live_streams"]
            assert one == 1
        # exactly one model is resident after each: the one before it was evicted and released
        assert now["live_streams"] == base["live_streams"] + 1, f"after {name}: {now['live_streams'] - base['live_streams']} models live"
    em.release_device_models()
    DC.assert_back_to(base, "three models through a cache of one")


# ---- b. a call the library declines allocates nothing ---------------------------------------------------------------------
def _assert_refusals_moved_nothing(what, w, at_least):
    moved = [r for r in w.refusals if r[2]]
    print(f"[devmem] {what}: {len(w.refusals)} declined calls watched")
    assert not moved, f"{what}: declined calls that moved the ledger: {moved}"
    assert len(w.refusals) >= at_least, f"{what}: only {len(w.refusals)} declined calls were seen, expected {at_least}"


@pytest.mark.parametrize("pair", sorted(RC.DECLINES), ids=_pid)
def test_a_documented_decline_allocates_nothing(pair):
    case, opn = pair
    P = RC.problem(case)
    base = DC.reading()
    dm = RC.fresh(P)
    try:
        with DC.watching() as w:
            got = RC.run_op(RC.OP[opn], dm, P)
        assert got[0] == "declined" and got[1] == RC.DECLINES[pair], got[:2]
        assert [r for r in w.refusals if r[1] == RC.DECLINES[pair]], w.refusals
        _assert_refusals_moved_nothing(f"{case}/{opn}", w, 1)
    finally:
        dm.close()
    DC.assert_back_to(base, f"{case}/{opn} declined")


# the feature tests that list the library's argument refusals, and how many declined calls each makes at least
BORROWED = [("test_gpu_design", "test_abi_argument_checks", 16), ("test_gpu_predict_cov", "test_abi_argument_checks", 4),
            ("test_gpu_cross_validation", "test_bad_folds_refused", 4), ("test_gpu_srccorr", "test_documented_errors", 5),
            ("test_gpu_logpost_grad", "test_refusals", 10),
            ("test_gpu_wsummary", "test_refusals_return_err_arg_and_leave_the_ledger_alone", 12)]


@pytest.mark.parametrize("module,test,at_least", BORROWED, ids=[f"{m}-{t}" for m, t, _ in BORROWED])
def test_an_argument_refusal_allocates_nothing(module, test, at_least):
    """the feature test itself runs, with every library call watched: the same bad arguments, none restated here"""
    fn = getattr(importlib.import_module(module), test)
    base = DC.reading()
    with DC.watching() as w:
        fn()
    _assert_refusals_moved_nothing(f"{module}.{test}", w, at_least)
    DC.assert_back_to(base, f"{module}.{test}")


# ---- c. warm calls --------------------------------------------------------------------------------------------------------
WARM_ROWS = [(r, c) for r in SC.ROWS if r.name in DC.WARM_MODEL_DEV for c in r.cases]


@pytest.mark.parametrize("row,case", WARM_ROWS, ids=[SC.param_id(rc) for rc in WARM_ROWS])
def test_warm_dev_entries(row, case):
    P = RC.problem(case)
    dm = RC.fresh(P)
    try:
        inputs = row.inputs(P, 0)
        counts, bytes_after, res = [], [], []
        for _ in range(3):
            out, n = DC.allocs_of(lambda: SC.quiet(row, P, dm, inputs)[0])
            counts.append(n)
            res.append(out)
            bytes_after.append(DC.reading()["live_bytes"])
        print(f"[devmem] {row.name} on {case}: allocations of three calls {counts}")
        SC.assert_same(f"{row.name} third call", res[2], res[0])
        assert bytes_after[2] == bytes_after[1], f"{row.name}: live bytes {bytes_after}"
        assert counts[2] == DC.WARM_MODEL_DEV[row.name], (
            f"{row.name} on {case}: the third call made {counts[2]} allocations, the table says {DC.WARM_MODEL_DEV[row.name]}")
    finally:
        dm.close()


UNDECLINED = [p for p in _pairs(DC.WALK_CASES) if p not in RC.DECLINES]


@pytest.mark.parametrize("pair", UNDECLINED, ids=_pid)
def test_warm_host_forms(pair):
    """the host-array forms stage their inputs and outputs in a scope of the call: the third call allocates exactly what
    the table says, frees all of it, and the live bytes stay (the declined pairs: test_a_documented_decline_...)"""
    case, opn = pair
    P = RC.problem(case)
    dm = RC.fresh(P)
    try:
        counts, bytes_after = [], []
        for _ in range(3):
            got, n = DC.allocs_of(lambda: RC.run_op(RC.OP[opn], dm, P))
            assert got[0] == "ok", got[1:]
            counts.append(n)
            bytes_after.append(DC.reading()["live_bytes"])
        print(f"[devmem] WARM {case} {opn} {counts}")
        assert bytes_after[2] == bytes_after[1], f"{case}/{opn}: live bytes {bytes_after}"
        want = DC.warm_host_count(case, opn)
        assert counts[2] == want, f"{case}/{opn}: the third call made {counts[2]} allocations, the table says {want}"
    finally:
        dm.close()


@pytest.mark.parametrize("kind", ["stretch", "tempered", "hmc"])
def test_warm_sampler_run(kind):
    P = RC.problem("general")
    dm = RC.fresh(P)
    ds = {"stretch": lambda: RC.stretch_sampler(dm, P, 300), "tempered": lambda: RC.tempered_sampler(dm, P),
          "hmc": lambda: RC.hmc_sampler(dm, P)}[kind]()
    try:
        ds.reserve(16)
        counts, bytes_after = [], []
        for _ in range(3):
            _, n = DC.allocs_of(lambda: ds.run(4))
            counts.append(n)
            bytes_after.append(DC.reading()["live_bytes"])
        print(f"[devmem] {kind}.run after reserve: allocations of three calls {counts}")
        assert bytes_after[2] == bytes_after[1]
        assert counts[2] == DC.WARM_SAMPLER_RUN[kind], f"{kind}: the third run made {counts[2]} allocations"
        assert counts[1] == 0 and counts[0] == 0, f"{kind}: a run after reserve allocated {counts}"
    finally:
        ds.close()
        dm.close()


# ---- d. the refusal walk --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.WALK_CASES)
def test_walk_create_and_setup(case):
    P = RC.problem(case)
    base = DC.reading()
    dm, A = DC.allocs_of(lambda: RC.fresh(P))
    X = RC.logpost_rows(P, 33)
    want = dm.logpost(X)
    dm.close()
    DC.assert_back_to(base, f"{case}: create + likelihood_setup")
    assert A > 20
    print(f"[devmem] {case}: create + likelihood_setup make {A} allocations")
    L = _lib()
    for j in range(1, A + 1):
        made = []

        def seq():
            made.append(GU.device_model(P.model))
            RC.apply_setup(made[0], P.setup)
        with L.devmem_refusing(j) as r:
            msg = DC.refused(seq)
        assert r.fired, f"{case}: the refusal armed at {j} of {A} did not fire"
        assert "bytes" in msg
        if made:
            # the model survived its setup's refusal: the setup again, and it computes what a fresh one does
            RC.apply_setup(made[0], P.setup)
            assert RC.same_bits(made[0].logpost(X), want), f"{case}: logpost after the setup refused at {j}"
            made[0].close()
        del made
        DC.assert_back_to(base, f"{case}: create + likelihood_setup refused at allocation {j} of {A}")


def test_walk_resetup_of_a_live_model():
    """a model that HAS a likelihood is given another one and an allocation of that setup is refused: the handle must say
    it has no likelihood (not launch on half a setup), and take the next setup as a fresh handle does"""
    from gpemu._lib import GpemuError
    P = RC.problem("general")
    other = RC.setup_variant(P, "sources")
    X = RC.logpost_rows(P, 33)
    want = {}
    for kind, setup in (("single", P.setup), ("sources", other)):
        dm = RC.fresh(P, setup)
        want[kind] = dm.logpost(X)
        dm.close()
    base = DC.reading()
    dm = RC.fresh(P)
    _, A = DC.allocs_of(lambda: RC.apply_setup(dm, other))
    dm.close()
    assert A >= 8
    L = _lib()
    for j in range(1, A + 1):
        dm = RC.fresh(P)
        with L.devmem_refusing(j) as r:
            DC.refused(lambda: RC.apply_setup(dm, other))
        assert r.fired
        with pytest.raises(GpemuError) as e:
            dm.logpost(X)
        assert e.value.code == DC.ERR_STATE, f"refused at {j}: logpost on half a setup gave {e.value}"
        RC.apply_setup(dm, other)
        assert RC.same_bits(dm.logpost(X), want["sources"]), f"the setup after one refused at {j}"
        RC.apply_setup(dm, P.setup)
        assert RC.same_bits(dm.logpost(X), want["single"])
        dm.close()
        DC.assert_back_to(base, f"re-setup refused at allocation {j} of {A}")


@pytest.mark.parametrize("pair", _pairs(DC.WALK_CASES), ids=_pid)
def test_walk_every_operation(pair):
    case, opn = pair
    op = RC.OP[opn]
    P = RC.problem(case)
    L = _lib()
    base = DC.reading()
    dm = RC.fresh(P)
    want, A = DC.allocs_of(lambda: RC.run_op(op, dm, P))
    dm.close()
    DC.assert_back_to(base, f"{case}/{opn}")
    print(f"[devmem] WALK {case} {opn}: {A} allocations on a fresh handle")
    compared = 0
    for j in range(1, A + 1):
        dm = RC.fresh(P)
        try:
            with L.devmem_refusing(j) as r:
                got = RC.run_op(op, dm, P)
            assert r.fired, f"{case}/{opn}: the refusal armed at {j} of {A} did not fire"
            assert got[0] == "declined" and got[1] == DC.ERR_HIP and "refused" in got[2], (
                f"{case}/{opn}: armed at {j} of {A}, the operation gave {got[:2]}: {got[2] if got[0] == 'declined' else ''}")
            again = RC.run_op(op, dm, P)
            compared += RC.assert_same(case, op, again, want, f"after the refusal of allocation {j} of {A}")
        finally:
            dm.close()
        DC.assert_back_to(base, f"{case}/{opn} refused at allocation {j} of {A}")
    if pair not in RC.DECLINES:
        # a walk that refused nothing, or compared no bits after a refusal, is no walk
        assert A > 0 and compared == A, f"{case}/{opn}: {A} allocations, {compared} comparisons after a refusal"


@pytest.mark.parametrize("case", DC.WALK_CASES)
def test_walk_really_compares(case):
    """a table of declines cannot pass as a walk: every pair that is not a documented decline refuses at least one
    allocation and compares bits after each (asserted in the walk itself), and there are enough of them"""
    n = sum(1 for p in UNDECLINED if p[0] == case)
    assert n >= DC.MIN_WALK_COMPARED, f"{case}: only {n} operations are walked and compared"


def _state_of(ds):
    return RC.sampler_result(ds)


SETTERS = [(k, s) for k in ("stretch", "tempered", "hmc")
           for s in ("set_state", "set_betas", "reserve", "snapshot", "restore", "run_growing")
           if s != "set_betas" or k == "tempered"]       # (only a tempered sampler has a ladder)


@pytest.mark.parametrize("kind,setter", SETTERS, ids=[f"{k}-{s}" for k, s in SETTERS])
def test_walk_sampler_setters(kind, setter):
    """a refusal inside a setter leaves state, counts and chain as they were, and the next unarmed run gives the chain of
    a sampler that never saw it (the promise of ensure_chain's comment, and of set_state's)"""
    P = RC.problem("general")
    L = _lib()
    lib = L.lib()
    W = {"stretch": 300, "tempered": 48, "hmc": 16}[kind]
    X1 = RC.walkers(P, f"devmem_setter_{kind}", W)

    def make(dm):
        return {"stretch": lambda: RC.stretch_sampler(dm, P, 300), "tempered": lambda: RC.tempered_sampler(dm, P),
                "hmc": lambda: RC.hmc_sampler(dm, P)}[kind]()

    def prepare(ds):
        """the state the setter is called in: `run_growing` and `restore` after steps that filled the first buffer"""
        if setter == "run_growing":
            ds.run(255)
        elif setter == "restore":
            ds.run(2)
            L.check(lib.gpemu_sampler_snapshot(ds._h))
            ds.run(2)
        else:
            ds.run(2)

    def call(ds):
        if setter == "set_state":
            ds.set_state(X1)
        elif setter == "set_betas":
            ds.set_betas([1.0, 0.25])
        elif setter == "reserve":
            ds.reserve(1000)
        elif setter == "snapshot":
            L.check(lib.gpemu_sampler_snapshot(ds._h))
        elif setter == "restore":
            L.check(lib.gpemu_sampler_restore(ds._h))
        else:
            ds.run(4)

    def after(ds):
        if setter == "snapshot":         # the snapshot must be usable: two steps, back, the same two steps
            ds.run(2)
            L.check(lib.gpemu_sampler_restore(ds._h))
        ds.run(3)
        return _state_of(ds)

    base = DC.reading()
    dm = RC.fresh(P)
    ds = make(dm)
    prepare(ds)
    _, A = DC.allocs_of(lambda: call(ds))
    want = after(ds)
    ds.close()
    dm.close()
    DC.assert_back_to(base, f"{kind}.{setter}")
    print(f"[devmem] {kind}.{setter}: {A} allocations")
    for j in range(1, A + 1):
        dm = RC.fresh(P)
        ds = make(dm)
        try:
            prepare(ds)
            before = _state_of(ds)
            with L.devmem_refusing(j) as r:
                DC.refused(lambda: call(ds))
            assert r.fired
            RC.assert_same("general", RC.Op(setter, None), ("ok", _state_of(ds)), ("ok", before),
                           f"{kind}: state, counts and chain after {setter} refused at allocation {j} of {A}")
            call(ds)
            RC.assert_same("general", RC.Op(setter, None), ("ok", after(ds)), ("ok", want),
                           f"{kind}: the run after {setter} was refused at allocation {j} of {A} and then repeated")
        finally:
            ds.close()
            dm.close()
        DC.assert_back_to(base, f"{kind}.{setter} refused at {j} of {A}")


@pytest.mark.parametrize("kind", ["stretch", "tempered", "hmc"])
def test_walk_first_set_state(kind):
    """the FIRST set_state of a sampler evaluates the walkers on a model that has no workspace yet: a refusal in that
    evaluation comes after the new positions were staged, and must still leave the state the call found"""
    from gpemu.sampler import DeviceSampler, HMCSampler, TemperedSampler
    P = RC.problem("general")
    L = _lib()
    make = {"stretch": lambda dm: DeviceSampler([dm], 300, seed=11),
            "tempered": lambda dm: TemperedSampler([dm], 24, [1.0, 0.5], seed=5, swap_every=1),
            "hmc": lambda dm: HMCSampler([dm], 16, n_leapfrog=3, step_size=0.05, seed=8)}[kind]
    X0 = RC.walkers(P, f"devmem_first_{kind}", {"stretch": 300, "tempered": 48, "hmc": 16}[kind])

    def after(ds):
        ds.run(3)
        return RC.sampler_result(ds)
    base = DC.reading()
    dm = RC.fresh(P)
    ds = make(dm)
    _, A = DC.allocs_of(lambda: ds.set_state(X0))
    want = after(ds)
    ds.close()
    dm.close()
    DC.assert_back_to(base, f"{kind}: the first set_state")
    print(f"[devmem] {kind}: the first set_state makes {A} allocations")
    # its staging rows, and the model's workspace (8 buffers) or, for HMC, the two workspaces of the gradient path
    assert A >= (3 if kind == "hmc" else 9)
    for j in range(1, A + 1):
        dm = RC.fresh(P)
        ds = make(dm)
        try:
            before = RC.sampler_result(ds)
            with L.devmem_refusing(j) as r:
                DC.refused(lambda: ds.set_state(X0))
            assert r.fired
            RC.assert_same("general", RC.Op("set_state", None), ("ok", RC.sampler_result(ds)), ("ok", before),
                           f"{kind}: the state after the first set_state was refused at allocation {j} of {A}")
            ds.set_state(X0)
            RC.assert_same("general", RC.Op("set_state", None), ("ok", after(ds)), ("ok", want),
                           f"{kind}: the run after the first set_state was refused at {j} of {A} and repeated")
        finally:
            ds.close()
            dm.close()
        DC.assert_back_to(base, f"{kind}: the first set_state refused at {j} of {A}")


def test_walk_fit_batch_growth():
    """DeviceFit.lml_batch growing from 1 to 5 problems: every allocation of the regrow refused in turn; the handle then
    evaluates the 5, and the 1 again, as a handle that never saw a refusal"""
    c, X, ys, thetas = DC.fit_problem()
    L = _lib()
    base = DC.reading()
    f = DC.device_fit(c, X)
    one = DC.FIT_STEPS["lml_batch_1"](f, ys, thetas)
    five, A = DC.allocs_of(lambda: DC.FIT_STEPS["lml_batch_5"](f, ys, thetas))
    f.close()
    assert A >= 14
    _, A0 = DC.allocs_of(lambda: DC.device_fit(c, X).close())
    print(f"[devmem] DeviceFit: {A0} allocations at create, {A} to grow from 1 to 5 problems")
    for j in range(1, A0 + 1):
        with L.devmem_refusing(j) as r:
            DC.refused(lambda: DC.device_fit(c, X))
        assert r.fired
        DC.assert_back_to(base, f"DeviceFit create refused at {j} of {A0}")
    for j in range(1, A + 1):
        f = DC.device_fit(c, X)
        try:
            SC.assert_same("lml_batch of 1", DC.FIT_STEPS["lml_batch_1"](f, ys, thetas), one)
            with L.devmem_refusing(j) as r:
                DC.refused(lambda: DC.FIT_STEPS["lml_batch_5"](f, ys, thetas))
            assert r.fired
            SC.assert_same(f"lml_batch of 1 after the regrow refused at {j}", DC.FIT_STEPS["lml_batch_1"](f, ys, thetas), one)
            SC.assert_same(f"lml_batch of 5 after the regrow refused at {j}", DC.FIT_STEPS["lml_batch_5"](f, ys, thetas), five)
        finally:
            f.close()
        DC.assert_back_to(base, f"DeviceFit regrow refused at {j} of {A}")


def _walk_plain(name, fn):
    """fn() armed at every one of its allocations: each fires and raises, nothing leaks, and fn() then gives its bits"""
    L = _lib()
    base = DC.reading()
    want, A = DC.allocs_of(fn)
    DC.assert_back_to(base, name)
    assert A > 0
    print(f"[devmem] WALK {name}: {A} allocations")
    for j in range(1, A + 1):
        with L.devmem_refusing(j) as r:
            DC.refused(fn)
        assert r.fired, f"{name}: the refusal armed at {j} of {A} did not fire"
        DC.assert_back_to(base, f"{name} refused at allocation {j} of {A}")
        SC.assert_same(f"{name} after the refusal at {j}", fn(), want)
    return A


@pytest.mark.parametrize("name", DC.WALK_ONE_SHOTS + ("diag",))
def test_walk_one_shots_and_the_diag_handle(name):
    _walk_plain(name, DC.diag_run if name == "diag" else DC.HOST_ONE_SHOTS[name])


def test_walk_the_design_handle():
    P = RC.problem("general")
    dm = RC.fresh(P)
    try:
        _walk_plain("design", lambda: DC.design_run(dm, P))
        SC.assert_same("logpost after the design walk", (dm.logpost(RC.logpost_rows(P, 33)),),
                       (DC_fresh_logpost(P),))
    finally:
        dm.close()


def DC_fresh_logpost(P):
    dm = RC.fresh(P)
    try:
        return dm.logpost(RC.logpost_rows(P, 33))
    finally:
        dm.close()
