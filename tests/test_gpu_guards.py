"""Every *_dev entry point writes only its outputs, at edge shapes (tests/guard_cases.py: the arena and the gate;
tests/stream_cases.py: the table, ``edge_shapes`` beside every row).

  test_outputs_guards_and_prefill   (a)-(c), (e), (f): guards, inputs, results against the quiet device, two prefills of
                                    the outputs, nothing written by a call that declines
  test_results_ignore_the_guards    (d): the guards around the inputs, and the gap rows of a view, hold NaN and then the
                                    row's decoy
  test_padding_is_left_alone        the rows with an output's leading dimension, at ld = n + 1 and n + 7
  test_the_sweep_ran                conditions: every row ran at three shapes at least, one no multiple of 32; at most one
                                    (row, shape) in ten declined; the shapes run and declined are printed per row

A model is built once per problem and shared by the rows and shapes that use it (tests/test_gpu_handle_reuse.py holds
a used handle to a fresh handle's bits).

Wall time of the whole file on an MI355X, measured on the first runs: 21.4 s for 1 309 cases over 641 (row, shape) pairs,
12 s of it the first model and the start of the device; a case takes 2 to 60 ms.  637 pairs ran and 4 declined, each
before any write: gpemu_kde2d_dev and gpemu_pair_moments_dev at d = 1, gpemu_diag_create_dev at views of 1 and 3 steps.
"""
import collections

import pytest

import guard_cases as G
import reuse_cases as R
import stream_cases as SC

pytestmark = pytest.mark.gpu

_MODELS, _REFERENCE = {}, {}
RAN, DECLINED = collections.defaultdict(list), collections.defaultdict(list)


@pytest.fixture(scope="module", autouse=True)
def _models():
    yield
    for dm in _MODELS.values():
        dm.close()
    _MODELS.clear()
    _REFERENCE.clear()


def _model(case):
    if case is None:
        return None, None
    if case not in _MODELS:
        _MODELS[case] = R.fresh(R.problem(case))
    return R.problem(case), _MODELS[case]


def _setup(row, case, sh):
    """the problem, the model, the true and decoy inputs and the reference of a (row, case, shape), the last made once"""
    P, dm = _model(case)
    true, decoy = row.inputs(P, 0), row.inputs(P, 1)
    key = (row.name, case, sh)
    if key not in _REFERENCE:
        _REFERENCE[key] = G.reference_device(row, P, dm, true)
    return P, dm, true, decoy, _REFERENCE[key]


@pytest.mark.parametrize("rcs", G.sweep(), ids=G.sweep_id)
def test_outputs_guards_and_prefill(rcs):
    row, case, sh = rcs
    with SC.shaped(sh):
        P, dm, true, _, want = _setup(row, case, sh)
        declined, found = G.gate_outputs(row, P, dm, true, G.sweep_id(rcs), want)
    (DECLINED if declined is not None else RAN)[SC.param_id(rcs[:2])].append(sh)
    G.report(found)


@pytest.mark.parametrize("rcs", G.sweep(), ids=G.sweep_id)
def test_results_ignore_the_guards(rcs):
    row, case, sh = rcs
    with SC.shaped(sh):
        P, dm, true, decoy, want = _setup(row, case, sh)
        _, found = G.gate_input_guards(row, P, dm, true, decoy, G.sweep_id(rcs), want)
    G.report(found)


@pytest.mark.parametrize("rcs", G.padded_sweep(), ids=G.sweep_id)
def test_padding_is_left_alone(rcs):
    """the results are those of the quiet device at ld = n: the padding columns are part of the guard"""
    import dataclasses
    row, case, sh = rcs
    with SC.shaped(dataclasses.replace(sh, pad=0)):
        P, dm, true, decoy, want = _setup(row, case, dataclasses.replace(sh, pad=0))
    with SC.shaped(sh):
        declined, found = G.gate_outputs(row, P, dm, true, G.sweep_id(rcs), want)
        _, more = G.gate_input_guards(row, P, dm, true, decoy, G.sweep_id(rcs), want)
    assert declined is None, f"{G.sweep_id(rcs)}: declined with {declined}: the header admits ld > n"
    G.report(found + more)


def test_the_sweep_ran():
    """after the sweep above (the file's order): what ran and what declined, per row"""
    if not RAN and not DECLINED:
        print("[guards] the sweep did not run in this session: nothing to count")
        return
    pairs = declined = 0
    for rc in SC.sweep_params(G.FAMILIES):
        if rc[1] is not None and rc[1] not in rc[0].cases[:G.GUARD_CASES]:
            continue
        key = SC.param_id(rc)
        ran, dec = RAN.get(key, []), DECLINED.get(key, [])
        print(f"[guards] {key}: ran {', '.join(map(str, ran)) or '-'}; declined {', '.join(map(str, dec)) or '-'}")
        pairs, declined = pairs + len(ran) + len(dec), declined + len(dec)
        if len(ran) + len(dec) < len(rc[0].edge_shapes):
            continue                                             # (a selection of the sweep ran: nothing to conclude)
        if rc[0].family != SC.SAMPLER_COMM:
            assert len(ran) >= 3, f"{key}: ran at {len(ran)} shapes only"
            sizes = [sh.VIEW[0] * sh.VIEW[1] if sh.VIEW != SC.Shape().VIEW or rc[0].gaps else
                     (sh.B_SMALL if rc[1] is not None else sh.S) for sh in ran]
            assert any(n % 32 for n in sizes), f"{key}: every shape it ran at is a multiple of 32: {sizes}"
    print(f"[guards] {pairs} (row, shape) pairs, {declined} declined")
    assert 10 * declined <= pairs, f"{declined} of {pairs} (row, shape) pairs declined: more than one in ten"
