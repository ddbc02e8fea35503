"""The table of tests/stream_cases.py against include/gpemu.h: it names every prototype that takes a ``void *stream`` or
carries its stream in a ``const gpemu_call_ctx *``, and what it says about NULL and about waiting stands in the header's
own comments -- so a new ``_dev`` entry cannot be added without a row, which tests/test_gpu_streams.py then runs on a
stream of its own.  A prototype named ``*_dev`` that shows neither spelling must be exempted here by name, with a reason.

Limitation: a row's quotes are looked for in the whole section of its prototype (from the last ``/* ----`` banner), because
most families state their contract once ("Every _dev form works on `stream` ...").  A new entry added to an existing
section therefore finds its neighbours' sentences there; what holds it to them is its row and the GPU run behind the
gate, not this file."""
from __future__ import annotations

import re

import pytest

import stream_cases as SC

_text, _prototypes = SC.header_text, SC.stream_prototypes       # (the header's parser lives beside the table)


def _squash(s):
    """comment leaders and line breaks out: the words alone"""
    return re.sub(r"\s+", " ", re.sub(r"(?m)^\s*\*\s?", " ", s.replace("/*", " ").replace("*/", " ")))


def _section(text, offset):
    """the header from the last ``/* ----`` section line before `offset` up to the end of the prototype there"""
    start = text.rfind("/* ----", 0, offset)
    return text[max(start, 0):text.index(";", offset)]


def _conventions(text):
    return text[:text.index("#ifndef GPEMU_H")]


WEIGHTED_DEV = ("gpemu_posterior_predictive_weighted_dev", "gpemu_weighted_hpd_dev", "gpemu_weighted_kde1d_dev")
# a prototype named *_dev that takes neither a stream nor a ctx: {name: why it needs no row}
DEV_WITHOUT_A_STREAM = {}


def test_the_table_names_every_prototype_with_a_stream():
    text = _text()
    protos = _prototypes(text)
    by_stream, by_ctx = SC.prototypes_with(text, SC.STREAM_PARAM), SC.prototypes_with(text, SC.CTX_PARAM)
    assert len(by_stream) == 35 and len(by_ctx) == 3 and not set(by_stream) & set(by_ctx), (sorted(by_stream), sorted(by_ctx))
    assert len(protos) == 38 and "gpemu_logpost_dev" in protos and "gpemu_sampler_set_stream" in protos, sorted(protos)
    assert set(WEIGHTED_DEV) <= set(by_ctx), f"not found by their ctx: {sorted(set(WEIGHTED_DEV) - set(by_ctx))}"
    names = [r.name for r in SC.ROWS]
    assert len(set(names)) == len(names), "a row twice"
    assert set(names) == set(protos), (f"without a row: {sorted(set(protos) - set(names))}; "
                                       f"rows without a prototype: {sorted(set(names) - set(protos))}")


def test_every_dev_prototype_is_found_or_exempted_by_name():
    """a ``_dev`` entry whose stream is spelled a third way would slip past the table: it must be found by one of the two
    spellings, or stand in DEV_WITHOUT_A_STREAM with the reason"""
    text = _text()
    dev = {n for n in SC.all_prototypes(text) if n.endswith("_dev")}
    assert len(dev) == 36, sorted(dev)             # the 38 less gpemu_sampler_set_stream and gpemu_comm_all_gather
    unseen = dev - set(_prototypes(text))
    assert unseen == set(DEV_WITHOUT_A_STREAM), (
        f"*_dev prototypes with neither a `void *stream` nor a `const gpemu_call_ctx *`, and no exemption: "
        f"{sorted(unseen - set(DEV_WITHOUT_A_STREAM))}; exempted but found or gone: {sorted(set(DEV_WITHOUT_A_STREAM) - unseen)}")
    assert all(isinstance(why, str) and why.strip() for why in DEV_WITHOUT_A_STREAM.values())


def test_only_the_all_gather_is_left_out_of_the_sweep():
    omitted = {r.name: r.omitted for r in SC.ROWS if r.omitted}
    assert list(omitted) == ["gpemu_comm_all_gather"] and "RCCL" in omitted["gpemu_comm_all_gather"]
    swept = {r.name for r, _ in SC.sweep_params((SC.MODEL_BOUND, SC.DEVICE_WIDE, SC.HANDLE_CREATING, SC.SAMPLER_COMM))}
    assert swept == {r.name for r in SC.ROWS} - set(omitted)
    for r in SC.ROWS:
        assert r.omitted or (callable(r.run) and callable(r.inputs)), r.name
        assert r.family in (SC.MODEL_BOUND, SC.DEVICE_WIDE, SC.HANDLE_CREATING, SC.SAMPLER_COMM), r.name
        assert (r.family == SC.MODEL_BOUND) <= bool(r.cases), f"{r.name}: a model-bound row without a problem"
        assert set(r.cases) <= {"general", "wide", "tasks10", "sources"}, r.name


@pytest.mark.parametrize("row", SC.ROWS, ids=lambda r: r.name)
def test_the_rows_words_stand_in_the_header(row):
    """every quote of the row in the Conventions block or in the prototype's own section, and the row's two fields in
    agreement with its quotes"""
    text = _text()
    where = {"conventions": _squash(_conventions(text)), "section": _squash(_section(text, _prototypes(text)[row.name]))}
    assert row.doc, row.name
    for quote, place in row.doc:
        assert _squash(quote).strip() in where[place], f"{row.name}: {quote!r} is not in the header's {place}"
    said = " ".join(q for q, _ in row.doc)
    assert row.null_means in said, f"{row.name}: no quote says {row.null_means!r}"
    says_waits = any(w in said for w in ("waits for it", "is waited for", "wait for it"))
    says_not = any(w in said for w in (SC.NOWAIT, "does not wait"))
    assert says_waits != says_not, f"{row.name}: the quotes must say either that it waits or that it does not"
    assert row.waits == says_waits, f"{row.name}: waits = {row.waits}, the header says otherwise"
    if any(p == "conventions" for _, p in row.doc):
        assert row.name in where["conventions"], f"{row.name} is not named in the Conventions block"


def test_the_header_says_one_thing():
    """the Conventions block no longer gives one rule for every *_dev function: it names the entries that do not
    synchronise and sends the rest to their sections"""
    conv = _squash(_conventions(_text()))
    assert "NULL = the handle's own stream" not in conv
    assert "every other *_dev entry waits for its stream" in conv
    nowait = sorted(r.name for r in SC.ROWS if not r.waits and not r.omitted)
    assert nowait == sorted(["gpemu_gp_predict_dev", "gpemu_predict_full_dev", "gpemu_logpost_dev",
                             "gpemu_gp_predict_grad_dev", "gpemu_logpost_grad_dev"])
    for name in nowait:
        assert name in conv
