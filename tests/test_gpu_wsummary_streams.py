"""The ``_dev`` entries of the weighted chain summaries behind the gate of tests/stream_cases.py.  They
take their stream in a ``gpemu_call_ctx``, not as a ``void *stream`` parameter, so the table there does not name them:
the rows are built here and go through the same ``quiet`` / ``gated`` runs, with the byte-equality and ``query()``
conditions of tests/test_gpu_streams.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import reuse_cases as R
import stream_cases as SC

pytestmark = pytest.mark.gpu

S, RW = SC.S_WIDE, 2


def _ctx(st):
    from gpemu import _lib
    return _lib.CallCtx(int(st) or None, 0)


def _in_Vq(P, seed):
    """3 value rows and 2 rows of fixed-point weights in [2^39, 2^40): a row's total lies in [2^47, 2^48)"""
    q = SC._rng(seed, "wq").integers(2 ** 39, 2 ** 40, (RW, S)).astype(np.int64)
    return {"V": np.ascontiguousarray(SC._unit_rows(seed, "wV").T), "q": q}


TARGETS = np.ascontiguousarray(np.tile(np.array([1, 2 ** 45, 2 ** 47], dtype=np.uint64), (RW, 1)))
GRID = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.1, 9), (RW * 3, 1)))
H = np.full(RW * 3, 0.05)


def _hpd(ctx_of):
    def run(st, T, out, P, dm):
        o = out((RW, 3, 3, 2))
        ctx = ctx_of(st)
        SC._ck(SC._L().gpemu_weighted_hpd_dev(0, 3, S, SC._vp(T["V"]), S, 1, RW, SC._vp(T["q"]), S, 3, SC._vp(TARGETS),
                                              SC._vp(o), None if ctx is None else C.byref(ctx)))
        return (o,)
    return run


def _kde(ctx_of):
    def run(st, T, out, P, dm):
        o = out((RW, 3, 9))
        ctx = ctx_of(st)
        SC._ck(SC._L().gpemu_weighted_kde1d_dev(0, 3, S, SC._vp(T["V"]), S, 1, RW, SC._vp(T["q"]), S, 9, SC._vp(GRID),
                                                SC._vp(H), SC._vp(o), None if ctx is None else C.byref(ctx)))
        return (o,)
    return run


def _in_model_view(P, seed):
    nb, br, bs = SC.VIEW
    q = SC._rng(seed, "wq_view").integers(2 ** 39, 2 ** 40, (RW, nb * br)).astype(np.int64)
    return dict(SC._in_model_view(P, seed), q=q)


def _bands(st, T, out, P, dm):
    nb, br, bs = SC.VIEW
    tg = np.ascontiguousarray(np.tile(np.array([1, 2 ** 44, 2 ** 45], dtype=np.uint64), (RW, 1)))
    o = [out((RW, P.F)), out((RW, P.F)), out((RW, P.F)), out((RW, P.F, 3))]
    ctx = _ctx(st)
    SC._ck(SC._L().gpemu_posterior_predictive_weighted_dev(dm.handle, SC._vp(T["X"]), nb, br, bs, RW, SC._vp(T["q"]), nb * br,
                                                           3, SC._vp(tg), *[SC._vp(a) for a in o], C.byref(ctx)))
    return tuple(o)


def _null_ctx(st):
    assert not st, "this row passes ctx == NULL"
    return None


ROWS = [
    SC.Row("gpemu_weighted_hpd_dev", inputs=_in_Vq, run=_hpd(_ctx), **SC._WIDE),
    SC.Row("gpemu_weighted_kde1d_dev", inputs=_in_Vq, run=_kde(_ctx), **SC._WIDE),
    SC.Row("gpemu_posterior_predictive_weighted_dev", inputs=_in_model_view, run=_bands, cases=("general", "wide"),
           **SC._M_WAIT),
]
NULL_ROWS = [
    SC.Row("gpemu_weighted_hpd_dev", inputs=_in_Vq, run=_hpd(_null_ctx), **SC._WIDE),
    SC.Row("gpemu_weighted_kde1d_dev", inputs=_in_Vq, run=_kde(_null_ctx), **SC._WIDE),
]


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


@pytest.mark.parametrize("rc", [(r, c) for r in ROWS for c in (r.cases or (None,))], ids=SC.param_id)
def test_entry_works_on_the_stream_of_its_ctx(rc):
    import torch
    _sweep(rc[0], rc[1], lambda: [torch.cuda.Stream(), torch.cuda.Stream()])


@pytest.mark.parametrize("row", NULL_ROWS, ids=lambda r: r.name)
def test_null_ctx_is_the_null_stream(row):
    import torch
    _sweep(row, None, lambda: [torch.cuda.default_stream()], null=True)
