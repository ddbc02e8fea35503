"""Every entry point that takes a ``void *stream``, or a ``gpemu_call_ctx`` that holds one, must work on the stream it
is given (tests/stream_cases.py: the table and the gate).  The rest of the suite only ever passes torch's default
stream, whose handle is NULL: the device-wide entries then run on the null stream, which serialises with almost
everything, and the model-bound ones fall back to the model's own stream, with a synchronisation around every call -- a
launch on the wrong stream, an input read before the stream has reached it or a wait for the wrong stream cannot show
there.

One-sided: a launch that goes to another stream than the one it was given is caught because that stream is not held
up by the gate.  On a device whose streams share a few hardware queues (4 here), a wrong stream that happens to share
the gate's queue is held up with it and the mistake stays hidden in that run; every row therefore runs on two freshly
created streams, which makes that unlikely, not impossible.  A failure here is a defect; a pass is evidence.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import golden_util as GU
import reuse_cases as R
import stream_cases as SC

pytestmark = pytest.mark.gpu


def _problem(case):
    return (None, None) if case is None else (R.problem(case), R.fresh(R.problem(case)))


def _reference(row, P, dm):
    """true inputs, decoy inputs, the quiet device's results and outputs; the decoy must give other bytes"""
    true, decoy = row.inputs(P, 0), row.inputs(P, 1)
    want, like = SC.quiet(row, P, dm, true)
    other, _ = SC.quiet(row, P, dm, decoy)
    assert SC.differs(want, other), f"{row.name}: the decoy inputs give the bytes of the true ones: the gate shows nothing"
    return true, decoy, want, like


def _sweep(row, case, streams, null=False):
    P, dm = _problem(case)
    try:
        true, decoy, want, like = _reference(row, P, dm)
        for i, s in enumerate(streams()):
            got = SC.gated(row, P, dm, true, decoy, s, like, null=null)
            SC.assert_same(f"{row.name} on {'NULL, torch default stream gated' if null else f'side stream {i}'}", got, want)
    finally:
        if dm is not None:
            if getattr(dm, "other_data", None) is not None:
                dm.other_data.close()
            dm.close()


def _two_streams():
    import torch
    return [torch.cuda.Stream(), torch.cuda.Stream()]


def _default_stream():
    import torch
    return [torch.cuda.default_stream()]


# ---- a. every row on two fresh side streams ---------------------------------------------------------------------------
@pytest.mark.parametrize("rc", SC.sweep_params((SC.MODEL_BOUND, SC.DEVICE_WIDE, SC.SAMPLER_COMM)), ids=SC.param_id)
def test_entry_works_on_the_stream_it_is_given(rc):
    """Behind a closed gate on a side stream the entry gives, bit for bit, what it gives on a quiet device with the
    default stream argument (one-sided: see the module docstring)."""
    _sweep(rc[0], rc[1], _two_streams)


# ---- b. NULL as documented --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [rc for rc in SC.sweep_params((SC.DEVICE_WIDE, SC.HANDLE_CREATING))
                                if rc[0].null_means == SC.NULL_NULL], ids=SC.param_id)
def test_null_is_the_null_stream(rc):
    """"NULL = the null stream": with the gate on torch's default stream -- the null stream -- and NULL passed, the same
    bytes."""
    _sweep(rc[0], rc[1], _default_stream, null=True)


def _w_logpost(st, T, out, P, dm):
    o = out((SC.B_BIG,))
    dm.logpost_dev(T["X"].data_ptr(), SC.B_BIG, o.data_ptr())
    return (o,)


def _w_gp_predict(st, T, out, P, dm):
    m, v = out((SC.B_BIG, P.k)), out((SC.B_BIG, P.k))
    dm.gp_predict_dev(T["X"].data_ptr(), SC.B_BIG, m.data_ptr(), v.data_ptr())
    return m, v


def _w_gp_predict_cov(st, T, out, P, dm):
    m, c = out((SC.B_SMALL, P.k)), out((P.k, SC.B_SMALL, SC.B_SMALL))
    dm.gp_predict_cov_dev(T["X"].data_ptr(), SC.B_SMALL, 0, SC.B_SMALL, m.data_ptr(), c.data_ptr())
    return m, c


def _w_predict_full(st, T, out, P, dm):
    cv, cov = out((SC.B_SMALL, P.F)), out((SC.B_SMALL, P.F, P.F))
    dm.predict_full_dev(T["X"].data_ptr(), SC.B_SMALL, 1.0, cv.data_ptr(), cov.data_ptr())
    return cv, cov


def _w_logpost_grad(st, T, out, P, dm):
    lp, g = out((SC.B_BIG,)), out((SC.B_BIG, P.d))
    dm.logpost_grad_dev(T["X"].data_ptr(), SC.B_BIG, lp.data_ptr(), g.data_ptr())
    return lp, g


def _w_postpred(st, T, out, P, dm):
    nb, br, bs = SC.VIEW
    o = [out((P.F,)), out((P.F,)), out((P.F,)), out((P.F, 3))]
    dm.posterior_predictive_dev(T["X"].data_ptr(), nb, br, bs, SC.i64(0, 31, 63), *[a.data_ptr() for a in o])
    return tuple(o)


def _w_sobol(st, T, out, P, dm):
    return R.flatten(dm.sobol_moments_dev(T["A"].data_ptr(), T["B"].data_ptr(), SC.B_SMALL, n_batches=2))


def _w_pointwise(st, T, out, P, dm):
    nb, br, bs = SC.VIEW
    o = out((dm.n_observable_blocks, nb * br))
    dm.loglik_pointwise_dev(T["X"].data_ptr(), nb, br, bs, o.data_ptr(), nb * br)
    return (o,)


def _w_data_log_ratio(st, T, out, P, dm):
    """reweight.data_log_ratio_dev: the model against a second handle of the same emulators with other data"""
    from gpemu import reweight
    from gpemu.rows import DeviceRows
    nb, br, bs = SC.VIEW
    if getattr(dm, "other_data", None) is None:        # (made by the quiet run, closed by _sweep)
        dm.other_data = R.fresh(P, dict(P.setup, y_exp=P.Y[1].copy()))
    return (reweight.data_log_ratio_dev([dm], [dm.other_data], DeviceRows(T["X"].data_ptr(), nb, br, bs, device=0)),)


def _w_design(st, T, out, P, dm):
    """design with DeviceRows, as DeviceSampler.propose_design makes them"""
    from gpemu import _lib
    from gpemu.design import DeviceRows
    nb, br, bs = SC.VIEW
    ref = DeviceRows(T["ref"].data_ptr(), nb, br, bs, stream=_lib.current_stream(0))
    with dm.design(ref, T["cand"].cpu().numpy(), max_picks=4) as dg:
        s0 = dg.scores()
        dg.condition(int(np.argmax(s0)))
        return s0, dg.scores(), np.array([dg.integrated_variance()])


def _wrapper(name, like, run, waits):
    """a row of the Python level: the inputs and the documentation of `like`, the call as a user makes it"""
    base = SC.ROW[like]
    return SC.Row(name, base.family, base.null_means, waits, base.doc, inputs=base.inputs, run=run)


WRAPPERS = [
    _wrapper("DeviceModel.logpost_dev", "gpemu_logpost_dev", _w_logpost, False),
    _wrapper("DeviceModel.gp_predict_dev", "gpemu_gp_predict_dev", _w_gp_predict, False),
    _wrapper("DeviceModel.gp_predict_cov_dev", "gpemu_gp_predict_cov_dev", _w_gp_predict_cov, True),
    _wrapper("DeviceModel.predict_full_dev", "gpemu_predict_full_dev", _w_predict_full, False),
    _wrapper("DeviceModel.logpost_grad_dev", "gpemu_logpost_grad_dev", _w_logpost_grad, False),
    _wrapper("DeviceModel.posterior_predictive_dev", "gpemu_posterior_predictive_dev", _w_postpred, True),
    _wrapper("DeviceModel.sobol_moments_dev", "gpemu_sobol_moments_dev", _w_sobol, True),
    _wrapper("DeviceModel.loglik_pointwise_dev", "gpemu_loglik_pointwise_dev", _w_pointwise, True),
    _wrapper("reweight.data_log_ratio_dev", "gpemu_loglik_pointwise_dev", _w_data_log_ratio, True),
    _wrapper("design(DeviceRows)", "gpemu_design_create_dev", _w_design, True),
]


@pytest.mark.parametrize("which", ["default", "side"])
@pytest.mark.parametrize("row", WRAPPERS, ids=lambda r: r.name)
def test_python_wrapper_is_ordered_with_torchs_current_stream(row, which):
    """The wrappers that take device tensors, called as a user calls them -- no stream argument -- with the gate on
    torch's current stream: the default stream, then a side stream.  On the default stream the wrapper may wait (its
    handle, 0, means "the model's own stream" to a model-bound entry, so the wrapper has to wait for it on the host);
    the result must be that of the true inputs either way."""
    import dataclasses
    row = dataclasses.replace(row, waits=True) if which == "default" else row
    _sweep(row, "general", _default_stream if which == "default" else lambda: _two_streams()[:1])


# ---- the sampler's wrappers: the chain rows of a view, in place ----------------------------------------------------
class _Raw:
    def __init__(self, address, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(address), False),
                                         "version": 2}


def _s_postpred(ds, dm, P):
    return R.flatten(ds.posterior_predictive())


def _s_loo(ds, dm, P):
    out = ds.loo()
    return R.flatten({k: out[k] for k in out if k != "labels"})


def _s_information_gain(ds, dm, P):
    return R.flatten(ds.information_gain(k=2, allow_copies=True))


def _s_propose_design(ds, dm, P):
    return R.flatten(ds.propose_design(2, candidates=R.rows(P, "stream_propose", 40), thin=1))


@pytest.mark.parametrize("which", ["default", "side"])
@pytest.mark.parametrize("op", [_s_postpred, _s_loo, _s_information_gain, _s_propose_design], ids=lambda f: f.__name__[3:])
def test_sampler_summary_is_ordered_with_torchs_current_stream(op, which):
    """DeviceSampler.posterior_predictive, .loo, .information_gain and .propose_design read the stored chain in place.
    The chain rows are the device input here: decoy rows lie in the chain buffer, and the true rows are copied over them
    on torch's current stream behind the gate."""
    import torch
    P = R.problem("general")
    dm = R.fresh(P)
    ds = R.stretch_sampler(dm, P, 8)
    try:
        ds.run(16)
        want = R.flatten(op(ds, dm, P))
        base, n = ds.chain_ptr(0)
        chain = torch.as_tensor(_Raw(base, (n, ds.W, P.d)), device=torch.device("cuda", 0))
        true = chain.clone()
        decoy = torch.from_numpy(R.rows(P, "stream_decoy_chain", n * ds.W).reshape(n, ds.W, P.d)).to(chain.device)
        chain.copy_(decoy)
        torch.cuda.synchronize()
        other = R.flatten(op(ds, dm, P))
        assert SC.differs(want, other), "the decoy chain gives the bytes of the true one"
        s = torch.cuda.default_stream() if which == "default" else torch.cuda.Stream()
        cycles = int(SC.calibrate() * SC.GATE_MS)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            chain.copy_(true, non_blocking=True)
            assert not s.query(), "the gate had opened before the call"
            got = R.flatten(op(ds, dm, P))
            s.synchronize()
        SC.assert_same(f"{op.__name__[3:]} on torch's {which} stream", got, want)
    finally:
        ds.close()
        dm.close()


# ---- c. a regrow of the workspace under a queued launch ---------------------------------------------------------------
def _op_logpost(mode):
    def dev(dm, B, X, out, st):
        o = out((B,))
        dm.logpost_dev(X.data_ptr(), B, o.data_ptr(), mode=mode, stream=st)
        return (o,)
    return dev, lambda dm, X: (dm.logpost(X, mode=mode),)


def _dev_gp_predict(dm, B, X, out, st):
    m, v = out((B, dm.k)), out((B, dm.k))
    dm.gp_predict_dev(X.data_ptr(), B, m.data_ptr(), v.data_ptr(), stream=st)
    return m, v


def _dev_logpost_grad(dm, B, X, out, st):
    lp, g = out((B,)), out((B, dm.d))
    dm.logpost_grad_dev(X.data_ptr(), B, lp.data_ptr(), g.data_ptr(), stream=st)
    return lp, g


REGROW_OPS = {
    "logpost_lowrank": _op_logpost(0),
    "logpost_exact": _op_logpost(1),
    "gp_predict": (_dev_gp_predict, lambda dm, X: dm.gp_predict(X)),
    "logpost_grad": (_dev_logpost_grad, lambda dm, X: dm.logpost_grad(X)),
}


@pytest.mark.parametrize("case", ["general", "tasks10"])
@pytest.mark.parametrize("op", list(REGROW_OPS))
def test_workspace_regrow_under_a_queued_launch(op, case):
    """A first call of B = 33 on a side stream behind a closed gate, then, without waiting, one of B = 130 on the same
    stream: the workspace of the model (and, for `tasks10`, the term buffer of the ticketed likelihood) has to regrow
    while the first call's launches are still queued and own the old buffers.  Then the same B = 130 through the
    host-pointer form, on the handle's own stream.  All three must be a fresh handle's results."""
    import torch
    dev_op, host_op = REGROW_OPS[op]
    P = R.problem(case)
    Xs = {B: R.rows(P, f"stream_regrow{B}", B) for B in (SC.B_SMALL, SC.B_BIG)}
    decoys = {B: R.rows(P, f"stream_regrow_decoy{B}", B) for B in Xs}
    want, like = {}, {}
    for B in Xs:                                       # every reference from a handle of its own
        dm = R.fresh(P)
        try:
            T = SC._device({"X": Xs[B]})
            o = SC.Outs()
            torch.cuda.synchronize()
            res = dev_op(dm, B, T["X"], o, 0)
            torch.cuda.synchronize()
            want[B], like[B] = SC._host(res), o.made
            want["host"] = tuple(np.array(a, copy=True) for a in host_op(dm, Xs[B]))
        finally:
            dm.close()
    dm = R.fresh(P)
    try:
        s = torch.cuda.Stream()
        T = {B: SC._device({"X": decoys[B]})["X"] for B in Xs}
        src = {B: SC._device({"X": Xs[B]})["X"] for B in Xs}
        outs = {B: SC.Outs([SC.blank(t.shape, t.dtype) for t in like[B]]) for B in Xs}
        cycles = int(SC.calibrate() * SC.GATE_MS)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            for B in Xs:
                T[B].copy_(src[B], non_blocking=True)
            assert not s.query(), "the gate had opened before the first call"
            first = dev_op(dm, SC.B_SMALL, T[SC.B_SMALL], outs[SC.B_SMALL], s.cuda_stream)
            assert not s.query(), "the first call waited for the stream, or the gate is too short: nothing was queued"
            second = dev_op(dm, SC.B_BIG, T[SC.B_BIG], outs[SC.B_BIG], s.cuda_stream)
            host = tuple(np.array(a, copy=True) for a in host_op(dm, Xs[SC.B_BIG]))
            first, second = [tuple(t.clone() for t in r) for r in (first, second)]
            s.synchronize()
        SC.assert_same(f"{op}/{case}: B = 33, queued under the regrow", SC._host(first), want[SC.B_SMALL])
        SC.assert_same(f"{op}/{case}: B = 130, after the regrow", SC._host(second), want[SC.B_BIG])
        SC.assert_same(f"{op}/{case}: B = 130, host form on the handle's own stream", host, want["host"])
    finally:
        dm.close()


# ---- d. the entries that create a handle ----------------------------------------------------------------------------
@pytest.mark.parametrize("rc", SC.sweep_params((SC.HANDLE_CREATING,)), ids=SC.param_id)
def test_handle_created_behind_a_gate(rc):
    """gpemu_diag_create_dev and gpemu_design_create_dev behind a closed gate on a side stream: the summaries read from
    the handle afterwards are those of a handle created from the same rows on a quiet device."""
    _sweep(rc[0], rc[1], _two_streams)


# ---- e. the sampler on a stream of the caller's -------------------------------------------------------------------------
def _general_groups():
    P = R.problem("general")
    return [R.fresh(P)], R.walkers(P, "stream_sampler", SC.SAMPLER_W)


def _shipped_groups():
    from gpemu import synthetic
    g = GU.load("g7_shipped_config")
    names, _, block_start, cols = GU.g7_groups(g)
    models = GU.g7_models(g)
    dms = []
    for n in names:
        dm = GU.device_model(models[n])
        dm.likelihood_setup(g["y_exp"][cols[n]], g["y_err"][cols[n]], g["lo"], g["hi"], 1.0, block_start=block_start[n])
        dms.append(dm)
    return dms, synthetic.make_walkers(SC.SAMPLER_W, seed=11, lo=g["design"].min(0), hi=g["design"].max(0))


def _chain_of(groups, stream_of):
    """20 steps on `stream_of()` (None: the sampler's own), then 5 more after set_stream(NULL): the results after each"""
    from gpemu import _lib
    from gpemu.sampler import DeviceSampler
    dms, X0 = groups()
    ds = DeviceSampler(dms, SC.SAMPLER_W, seed=2026)
    try:
        s = stream_of()
        if s is not None:
            _lib.check(_lib.lib().gpemu_sampler_set_stream(ds._h, C.c_void_p(s.cuda_stream)))
        ds.set_state(X0)
        ds.run(20)                                     # (the first step grows every group's workspace, on that stream)
        a = R.sampler_result(ds)
        _lib.check(_lib.lib().gpemu_sampler_set_stream(ds._h, None))
        ds.run(5)
        return a, R.sampler_result(ds)
    finally:
        ds.close()
        for dm in dms:
            dm.close()


@pytest.mark.parametrize("groups", [_shipped_groups, _general_groups], ids=["shipped3", "general"])
def test_sampler_on_a_side_stream_gives_the_same_chain(groups):
    """gpemu_sampler_set_stream to a torch side stream, 20 steps at W = 64 on fresh handles: chain, log-probabilities and
    acceptance counts have the bits of the run on the sampler's own stream; after set_stream(NULL) 5 further steps
    continue the unbroken chain."""
    import torch
    own20, own25 = _chain_of(groups, lambda: None)
    side20, side25 = _chain_of(groups, torch.cuda.Stream)
    SC.assert_same("20 steps on a side stream", side20, own20)
    SC.assert_same("5 more steps after set_stream(NULL)", side25, own25)
