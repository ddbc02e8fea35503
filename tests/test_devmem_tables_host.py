"""The tables of tests/devmem_cases.py against include/gpemu.h (no GPU, no library): every host one-shot of the header
-- a prototype whose first parameter is ``int device`` and that takes neither a ``void *stream`` nor a
``const gpemu_call_ctx *`` -- is a key of HOST_ONE_SHOTS, which tests/test_gpu_devmem.py runs for its balance, or is exempted
here by name with a reason; and every table that is keyed by a name of another table has that name.  So a new host
one-shot, a new model-bound ``_dev`` entry or a new operation of tests/reuse_cases.py cannot be added without its row.
The header's parser is the one of tests/stream_cases.py, which tests/test_streams_host.py uses too."""
from __future__ import annotations

import re

import devmem_cases as DC
import reuse_cases as RC
import stream_cases as SC

# prototypes with a leading `int device` that are no one-shot computation: {name: why HOST_ONE_SHOTS has no entry}
NOT_A_ONE_SHOT = {
    "gpemu_device_name": "a device query: no allocation of the library's, nothing for the ledger to balance",
    "gpemu_device_bus_id": "a device query: no allocation of the library's, nothing for the ledger to balance",
    "gpemu_device_memory": "a device query (hipMemGetInfo): no allocation of the library's",
}


def _host_one_shots(text):
    found = set(SC.stream_prototypes(text))                      # a stream or a ctx: a row of stream_cases instead
    return {name for name, (_, params) in SC.all_prototypes(text).items()
            if re.match(r"\s*int\s+device\s*(,|$)", params) and name not in found}


def test_every_host_one_shot_of_the_header_has_a_row():
    text = SC.header_text()
    one_shots = _host_one_shots(text)
    assert len(one_shots) >= 21 and "gpemu_select" in one_shots and "gpemu_select_dev" not in one_shots, sorted(one_shots)
    assert not set(NOT_A_ONE_SHOT) & set(DC.HOST_ONE_SHOTS), "exempted and in the table"
    assert all(isinstance(why, str) and why.strip() for why in NOT_A_ONE_SHOT.values())
    missing = one_shots - set(DC.HOST_ONE_SHOTS) - set(NOT_A_ONE_SHOT)
    assert not missing, (f"host one-shots of include/gpemu.h without an entry in devmem_cases.HOST_ONE_SHOTS (and not "
                         f"exempted in NOT_A_ONE_SHOT): {sorted(missing)}")
    gone = (set(DC.HOST_ONE_SHOTS) | set(NOT_A_ONE_SHOT)) - one_shots
    assert not gone, f"entries of HOST_ONE_SHOTS or NOT_A_ONE_SHOT that are no host one-shot of the header: {sorted(gone)}"
    assert all(callable(fn) for fn in DC.HOST_ONE_SHOTS.values())


def test_the_walked_one_shots_are_in_the_table():
    assert set(DC.WALK_ONE_SHOTS) <= set(DC.HOST_ONE_SHOTS), sorted(set(DC.WALK_ONE_SHOTS) - set(DC.HOST_ONE_SHOTS))
    assert "gpemu_weighted_hpd" in DC.WALK_ONE_SHOTS        # the one-shot with the most workspace blocks


def test_every_model_bound_row_has_a_warm_count():
    """the device-wide rows need none (three equal counts are demanded of them); a model-bound one is asserted exactly"""
    bound = {r.name for r in SC.ROWS if r.family == SC.MODEL_BOUND and not r.omitted}
    assert "gpemu_posterior_predictive_weighted_dev" in bound
    assert bound == set(DC.WARM_MODEL_DEV), (f"model-bound rows without a warm count: {sorted(bound - set(DC.WARM_MODEL_DEV))}; "
                                             f"counts without a row: {sorted(set(DC.WARM_MODEL_DEV) - bound)}")
    assert all(isinstance(n, int) and n >= 0 for n in DC.WARM_MODEL_DEV.values())


def test_every_operation_has_a_warm_host_count():
    ops = {op.name for op in RC.OPS}
    assert "posterior_predictive_weighted" in ops
    named = {k if isinstance(k, str) else k[1] for k in DC.WARM_HOST}
    assert ops == named, (f"operations of reuse_cases without a count in devmem_cases.WARM_HOST: {sorted(ops - named)}; "
                          f"counts without an operation: {sorted(named - ops)}")
    for case in DC.WALK_CASES:
        for op in RC.ops_of(case):
            assert isinstance(DC.warm_host_count(case, op.name), int), (case, op.name)
