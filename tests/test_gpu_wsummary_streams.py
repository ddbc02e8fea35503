"""The ``_dev`` entries of the weighted chain summaries with ``ctx == NULL``.  Their rows stand in the
table of tests/stream_cases.py like every other entry with a stream -- tests/test_streams_host.py finds them by their
``const gpemu_call_ctx *`` -- and tests/test_gpu_streams.py runs them behind the gate on the stream of their ctx, and with
``ctx->stream == NULL`` on the null stream.  What the table cannot express stays here: the NULL POINTER in place of the ctx,
which include/gpemu.h defines as stream NULL and workspace_bytes 0."""
from __future__ import annotations

import dataclasses
import time

import numpy as np
import pytest

import reuse_cases as R
import stream_cases as SC

pytestmark = pytest.mark.gpu


def _null_ctx(st):
    assert not st, "this row passes ctx == NULL"
    return None


def _null_row(name, run_of):
    return dataclasses.replace(SC.ROW[name], run=run_of(_null_ctx))


NULL_ROWS = [_null_row("gpemu_weighted_hpd_dev", SC.weighted_hpd_run), _null_row("gpemu_weighted_kde1d_dev", SC.weighted_kde_run)]


def _sweep(row, case, streams, null=False):
    P, dm = (None, None) if case is None else (R.problem(case), R.fresh(R.problem(case)))
    try:
        true, decoy = row.inputs(P, 0), row.inputs(P, 1)
        want, like = SC.quiet(row, P, dm, true)
        other, _ = SC.quiet(row, P, dm, decoy)
        assert SC.differs(want, other), f"{row.name}: the decoy inputs give the bytes of the true ones"
        for i, s in enumerate(streams()):
            got = SC.gated(row, P, dm, true, decoy, s, like, null=null)
            SC.assert_same(f"{row.name} on {'ctx == NULL, torch default stream gated' if null else f'side stream {i}'}",
                           got, want)
    finally:
        if dm is not None:
            dm.close()


@pytest.mark.parametrize("row", NULL_ROWS, ids=lambda r: r.name)
def test_null_ctx_is_the_null_stream(row):
    import torch
    _sweep(row, None, lambda: [torch.cuda.default_stream()], null=True)


# ---- ctx == NULL for the entry bound to a model: the model's own stream -------------------------------------------------
# The queue that stands in for the gate: non-waiting log-posteriors of B_QUEUE rows on the model's stream, in front of the
# call that writes the rows.  Their number is measured, as stream_cases.calibrate measures the gate: QUEUE_PROBE of them
# are timed, the queue grows per call by the device's time less the host's, and it is made QUEUE_FACTOR times as long as
# the bands' whole run on a quiet device, at most QUEUE_MAX calls.  Measured on an MI355X: 10 us a call for the host, 22 us
# for the device, 0.77 ms for the bands.  The runtime does not take any number of commands in flight: 512 calls were
# queued in 5.1 ms and left the stream busy for 5.9 ms more, but 675 took the host 18 ms and left no queue behind, as did
# 88 calls of 2049 rows (28 us and 112 us each while only 16 are queued).  Hence small calls, a modest factor and a cap;
# a queue that has drained all the same fails the test's premise, it does not pass.
B_QUEUE, QUEUE_PROBE, QUEUE_FACTOR, QUEUE_MAX = SC.B_BIG, 64, 4, 512


def _queue(dm, n_calls, ballast, lp):
    """n_calls log-posteriors on the model's own stream (stream NULL), nothing waited for"""
    L = SC._L()
    for _ in range(n_calls):
        SC._ck(L.gpemu_logpost_dev(dm.handle, B_QUEUE, SC._vp(ballast), SC._vp(lp), 0, None))


def _queue_length(dm, ballast, lp, quiet_s):
    """how many calls keep the model's stream busy for QUEUE_FACTOR times `quiet_s` after the last one was queued"""
    import torch
    _queue(dm, 1, ballast, lp)                                    # (the workspace of this batch size)
    dm.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _queue(dm, QUEUE_PROBE, ballast, lp)
    t1 = time.perf_counter()
    dm.sync()
    t2 = time.perf_counter()
    host, device = (t1 - t0) / QUEUE_PROBE, (t2 - t0) / QUEUE_PROBE
    n = QUEUE_MAX
    if device > host:
        n = min(QUEUE_MAX, max(QUEUE_PROBE, int(np.ceil(QUEUE_FACTOR * quiet_s / (device - host)))))
    print(f"[streams] the model's stream: a queued log-posterior of {B_QUEUE} rows takes the host {1e6 * host:.1f} us "
          f"and the device {1e6 * device:.1f} us; {n} of them for {QUEUE_FACTOR} x {1e3 * quiet_s:.3f} ms")
    return n


def test_null_ctx_is_the_models_stream():
    """gpemu_posterior_predictive_weighted_dev with ctx == NULL works on the model's own stream and waits for it.

    That stream is a non-blocking one of the library's, and include/gpemu.h gives the caller no handle of it: torch can
    put neither a sleep nor a copy there, so the gate of tests/stream_cases.py cannot close it.  What can be ordered on it
    is the library's own work, and that is the gate here: the rows the bands read are WRITTEN on the model's stream, over
    decoy rows, by a gpemu_gp_predict_dev with stream NULL (documented not to wait; k = d in the "general" problem, so its
    PC means are a valid array of rows) behind a queue of non-waiting log-posteriors; the bands follow at once with
    ctx == NULL, and their outputs are read as soon as the call returns, with no synchronisation of the test's own.
    They must be the bytes of a quiet device, where the same call runs with ``ctx->stream == NULL`` after everything has
    been waited for.  A launch on another stream is not held up by the queue and reads the decoy; a call that does not
    wait for the model's stream leaves NaN in the outputs.

    The premise is checked with bits, as ``closed_before`` is in the gate: right before the call, copies of the rows are
    queued on torch's streams (two fresh ones and the default stream: a stream that shares the hardware queue of the
    model's is held up with it), which the queue does not hold up.  At least one must still show the decoy -- the
    model's stream had not reached the write when the call was made -- or the run fails as one that proves nothing.
    After the call the rows must be the true ones: the queue did write them."""
    import torch
    P = R.problem("general")
    assert P.k == P.d, "the PC means of gpemu_gp_predict_dev serve as rows: k = d"
    row = SC.ROW["gpemu_posterior_predictive_weighted_dev"]
    null_row = _null_row(row.name, SC.weighted_bands_run)
    L = SC._L()
    dm = R.fresh(P)
    try:
        inputs = {seed: row.inputs(P, seed) for seed in (0, 1)}
        n = inputs[0]["X"].shape[0]
        ballast = SC._device({"X": R.rows(P, "wsummary_null_queue", B_QUEUE)})["X"]
        lp, var = SC.blank((B_QUEUE,), torch.float64), SC.blank((n, P.k), torch.float64)
        # the rows of both seeds as the model's stream writes them, on a quiet device
        made = {}
        for seed in (0, 1):
            src, rows = SC._device({"X": inputs[seed]["X"]})["X"], SC.blank((n, P.d), torch.float64)
            torch.cuda.synchronize()
            SC._ck(L.gpemu_gp_predict_dev(dm.handle, n, SC._vp(src), SC._vp(rows), SC._vp(var), None))
            dm.sync()
            made[seed] = rows.cpu().numpy()
            assert np.all(np.isfinite(made[seed]))
        assert not R.same_bits(made[0], made[1])
        true = {"X": made[0], "q": inputs[0]["q"]}
        want, like = SC.quiet(row, P, dm, true)                  # (ctx->stream == NULL)
        other, _ = SC.quiet(row, P, dm, {"X": made[1], "q": inputs[0]["q"]})
        assert SC.differs(want, other), "the decoy rows give the bytes of the true ones: the queue shows nothing"
        tq = time.perf_counter()
        quiet_null = SC.quiet(null_row, P, dm, true)[0]
        tq = time.perf_counter() - tq                            # (with the upload of the inputs: an upper bound)
        SC.assert_same("ctx == NULL on a quiet device", quiet_null, want)
        n_queue = _queue_length(dm, ballast, lp, tq)

        T = SC._device({"X": made[1], "q": inputs[0]["q"]})      # the decoy
        src = SC._device({"X": inputs[0]["X"]})["X"]             # what the true rows are made from
        o = SC.Outs([SC.blank(t.shape, t.dtype) for t in like])
        watchers = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()]
        seen = [SC.blank(T["X"].shape, T["X"].dtype) for _ in watchers]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _queue(dm, n_queue, ballast, lp)
        SC._ck(L.gpemu_gp_predict_dev(dm.handle, n, SC._vp(src), SC._vp(T["X"]), SC._vp(var), None))
        for s, copy in zip(watchers, seen):
            with torch.cuda.stream(s):
                copy.copy_(T["X"], non_blocking=True)
        t1 = time.perf_counter()
        res = null_row.run(0, T, o, P, dm)
        t2 = time.perf_counter()
        got = SC._host(res)                                      # (no synchronisation of ours: the call has waited)
        torch.cuda.synchronize()
        still_decoy = [R.same_bits(c.cpu().numpy(), made[1]) for c in seen]
        print(f"[streams] ctx == NULL on the model's stream: {n_queue} + 1 calls queued in {1e3 * (t1 - t0):.3f} ms, the bands "
              f"returned {1e3 * (t2 - t1):.3f} ms later ({1e3 * tq:.3f} ms on a quiet device); the rows were still the "
              f"decoy for {sum(still_decoy)} of {len(seen)} watching streams")
        assert any(still_decoy), (f"the queue of {n_queue} calls on the model's stream had drained before the call could be "
                                  f"made ({1e3 * (t1 - t0):.3f} ms after its first one): the run proves nothing")
        SC.assert_same("the rows the queue writes", (T["X"].cpu().numpy(),), (made[0],))
        SC.assert_same("ctx == NULL behind the queue of the model's own stream", got, want)
    finally:
        dm.close()

