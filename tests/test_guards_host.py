"""The guard gate of tests/guard_cases.py, without a device:
  - the gate can fail: a stand-in entry in Python over a host arena makes, in turn, each mistake the gate is there for,
    and each is reported with the right array, side and offset (the writes stay inside the arena by construction);
  - the table is complete: every *_dev prototype of include/gpemu.h has a row with edge shapes (or a reason to be left
    out), every ld* / stride parameter is known to address an input or is swept with padding, and the inputs of every
    device-wide row obey the header's argument rules at every edge shape;
  - the header says what the gate holds the library to.
"""
import dataclasses
import re

import numpy as np
import pytest

import guard_cases as G
import stream_cases as SC

ROWS, COLS = 5, 7


def _inputs(seed):
    return {"x": np.random.default_rng(seed).uniform(1.0, 2.0, (ROWS, COLS))}


def _entry(mistake=None):
    """out0[ROWS][COLS] (ld = COLS + pad) = 2 x, out1 (host) = the column sums of x; ``mistake``: what it does wrong"""
    def run(st, T, out, P, dm):
        x = T["x"]
        ld = COLS + SC.PAD
        if mistake == "declines at once":
            out((ROWS, COLS), ld=ld)
            raise G.Declined(-1)
        o, h = out((ROWS, COLS), ld=ld), out.host((COLS,))
        if mistake == "declines after a write":
            o[0, 0] = 3.0
            raise G.Declined(-1)
        held = float(o[0, 1])
        if mistake in ("unwritten", "declared unwritten"):        # every element but the last
            o[:-1, :] = 2.0 * x[:-1]
            o[-1, :-1] = 2.0 * x[-1, :-1]
        else:
            o[:, :] = 2.0 * x
        h[:] = x.sum(axis=0)
        if mistake == "before":
            G.poke(o.ctypes.data - 8, 0.0)
        elif mistake == "after":
            G.poke(o.ctypes.data + ROWS * ld * 8 + 16, float("nan"))
        elif mistake == "padding":
            G.poke(o.ctypes.data + (2 * ld + COLS) * 8, 1.0)
        elif mistake == "host after":
            G.poke(h.ctypes.data + COLS * 8, 1.0)
        elif mistake == "input":
            x[1, 2] = 0.0
        elif mistake == "reads a guard":
            o[0, 0] = 2.0 * G.peek(x.ctypes.data + x.nbytes)
        elif mistake == "adds to its output":
            o[0, 1] += held
        return o, h
    return run


def _row(mistake=None, **kw):
    return SC.Row("stand_in_dev", SC.DEVICE_WIDE, SC.NULL_NULL, True, (), inputs=lambda P, seed: _inputs(seed),
                  run=_entry(mistake), **kw)


def _gate(mistake, pad=1, **kw):
    """the findings of both gates for the stand-in with ``mistake``, against the sound stand-in's results"""
    with SC.shaped(SC.Shape(pad=pad)):
        want = G.reference_host(_row(), _inputs(0))
        row = _row(mistake, **kw)
        _, a = G.gate_outputs(row, None, None, _inputs(0), "stand_in_dev pad=1", want, on_device=False)
        _, b = G.gate_input_guards(row, None, None, _inputs(0), _inputs(1), "stand_in_dev pad=1", want, on_device=False)
    return a, b


def test_a_sound_entry_passes():
    for pad in (0, 1, 7):
        a, b = _gate(None, pad=pad)
        assert not a and not b, [str(f) for f in a + b]


LAST = ((ROWS - 1) * COLS + COLS - 1) * 8
PLANTED = [
    # mistake, the gate that must see it, kind, array, side, byte offset
    ("before", "outputs", "guard", "out0", G.BEFORE, 8),
    ("after", "outputs", "guard", "out0", G.AFTER, 16),
    ("padding", "outputs", "guard", "out0", G.PADDING, (2 * (COLS + 1) + COLS) * 8),
    ("host after", "outputs", "guard", "out1(host)", G.AFTER, 0),
    ("input", "outputs", "input", "x", "", (1 * COLS + 2) * 8),
    ("reads a guard", "inputs", "result", "result0", "", 0),
    ("unwritten", "outputs", "unwritten", "out0", "", LAST),
    ("adds to its output", "outputs", "prefill", "out0", "", 8),
    ("declines after a write", "outputs", "decline", "out0", "", 0),
]


@pytest.mark.parametrize("mistake,gate,kind,array,side,offset", PLANTED, ids=[p[0].replace(" ", "_") for p in PLANTED])
def test_the_gate_reports_a_planted_mistake(mistake, gate, kind, array, side, offset):
    a, b = _gate(mistake)
    found = a if gate == "outputs" else b
    hits = [f for f in found if (f.kind, f.array, f.side, f.offset) == (kind, array, side, offset)]
    assert hits, f"{mistake}: not reported as {kind} of {array} {side} at {offset}: {[str(f) for f in found]}"
    for f in hits:
        assert "stand_in_dev pad=1" in str(f) and array.split("(")[0].replace("result", "result ") in str(f) and str(offset) in str(f), str(f)
    if kind in ("guard", "input"):          # such a mistake is seen under either gate
        assert any(f.kind == kind and f.array == array for f in b), [str(f) for f in b]


def test_a_guard_read_changes_the_result_under_one_fill_at_least():
    """(d): a load past the end of an input that reaches a result differs under the NaN fill or under the decoy"""
    _, b = _gate("reads a guard")
    assert {f.kind for f in b} == {"result"} and len(b) == 2, [str(f) for f in b]


def test_declared_unwritten_elements_pass_and_must_stay():
    def mask(k, shape):
        m = np.zeros(shape, dtype=bool)
        if k == 0:
            m[-1, -1] = True
        return m
    want_row = _row("declared unwritten", unwritten=mask)
    with SC.shaped(SC.Shape(pad=1)):
        A = G.guarded(want_row, None, None, _inputs(0), "w", "nan", on_device=False)
        B = G.guarded(want_row, None, None, _inputs(0), "w", "finite", on_device=False)
        assert not A.findings + B.findings + G.prefill_findings("w", want_row, A, B)
        sound = _row(None, unwritten=mask)                         # writes what it declares unwritten
        A = G.guarded(sound, None, None, _inputs(0), "w", "nan", on_device=False)
        B = G.guarded(sound, None, None, _inputs(0), "w", "finite", on_device=False)
        found = G.prefill_findings("w", sound, A, B)
    assert [(f.kind, f.array, f.offset) for f in found] == [("unwritten", "out0", LAST)], [str(f) for f in found]


def test_a_clean_decline_passes_and_a_decline_the_reference_does_not_share_fails():
    with SC.shaped(SC.Shape(pad=1)):
        row = _row("declines at once")
        code, found = G.gate_outputs(row, None, None, _inputs(0), "d", G.reference_host(row, _inputs(0)), on_device=False)
        assert code == -1 and not found, [str(f) for f in found]
        _, found = G.gate_outputs(row, None, None, _inputs(0), "d", G.reference_host(_row(), _inputs(0)), on_device=False)
    assert found and all(f.kind == "result" for f in found)


def test_arrays_are_8_but_not_16_byte_aligned_and_guards_are_wide_enough():
    a = G.Arena(G.HOST_BYTES, G.SALT_HOST, False)
    blocks = [a.carve(f"b{i}", "output", shape, dt, 0, ld=ld) for i, (shape, dt, ld) in enumerate(
        (((3, 5), np.float64, None), ((7,), np.int32, None), ((2, 9), np.int64, 16), ((40000,), np.float64, None), ((1,), np.float64, None)))]
    end = 0
    for b in blocks:
        assert b.view.ctypes.data % 16 == 8
        need = max(G.GUARD_MIN, 2 * 4 * b.units) + 8
        assert 4 * b.band >= need and 4 * (b.start - end) >= need, b.name
        end = b.start + b.units
    assert 4 * b.band <= 8 * a.nwords - 4 * end
    assert not a.check("fresh")
    words = G.pattern(1024, G.SALT_HOST)
    assert len(set(words.tolist())) == 1024 and not np.isnan(words.view(np.float64)).all()


# ---- the table ---------------------------------------------------------------------------------------------------------
def _dev_prototypes():
    return {n: p for n, (_, p) in SC.all_prototypes(SC.header_text()).items() if n.endswith("_dev")}


def test_every_dev_prototype_has_edge_shapes():
    for name in _dev_prototypes():
        assert name in SC.ROW, f"{name}: a *_dev prototype without a row in tests/stream_cases.py"
        r = SC.ROW[name]
        assert r.omitted or r.edge_shapes, f"{name}: no edge_shapes: the guard sweep does not run it"
    for r in SC.ROWS:
        assert r.omitted or r.edge_shapes, f"{r.name}: no edge_shapes"
    swept = {r.name for r, _, _ in G.sweep()}
    assert swept == {r.name for r in SC.ROWS if not r.omitted}


def test_every_leading_dimension_is_an_inputs_or_swept_with_padding():
    padded = {(r.name, sh.pad) for r, _, sh in G.padded_sweep()}
    for name, params in _dev_prototypes().items():
        lds = re.findall(r"\b(ld\w*|\w*stride\w*)\b", params)
        row = SC.ROW[name]
        for p in lds:
            assert (p in SC.INPUT_LD.get(name, ())) != (p in row.out_ld), \
                f"{name}: `{p}` must be listed in INPUT_LD (it addresses an input) or in the row's out_ld, not both"
        assert set(SC.INPUT_LD.get(name, ())) | set(row.out_ld) == set(lds), f"{name}: {lds}"
        if row.out_ld:
            assert {(name, 1), (name, 7)} <= padded, f"{name}: an output with a leading dimension, not in the padded sweep"
    assert set(SC.PADS) == {1, 7}
    assert {n for n, _ in padded} == {"gpemu_loglik_pointwise_dev", "gpemu_loo_group_rows_dev", "gpemu_logprior_dev",
                                      "gpemu_weights_fixed_dev"}


def _size(row, sh):
    """the count of rows the shape varies: of a view, of the batch, or S"""
    d = SC.Shape()
    if sh.VIEW != d.VIEW or row.gaps or row.name == "gpemu_diag_create_dev":
        return sh.VIEW[0] * sh.VIEW[1]
    return sh.B_SMALL if (sh.B_SMALL, sh.B_BIG) != (d.B_SMALL, d.B_BIG) or row.family == SC.MODEL_BOUND else sh.S


REQUIRED = {
    "S": {1, 2, 63, 64, 65, 255, 256, 257}, "chunk": {2047, 2048, 2049},
    "B": {1, 31, 32, 33, 63, 64, 65, 127, 128, 129}, "views": {(1, 1, 1), (3, 5, 5), (16, 4, 6), (17, 4, 9)},
}
CHUNKED = ("gpemu_select_dev", "gpemu_rank_dev", "gpemu_hpd_dev", "gpemu_weighted_select_dev", "gpemu_weighted_hpd_dev",
           "gpemu_psis_dev")
TAKES_D = [n for n, p in _dev_prototypes().items() if re.search(r"\bint d\b", p) and SC.ROW[n].family == SC.DEVICE_WIDE]


def test_the_edge_shapes_cover_what_the_kernels_tile_by():
    assert SC.B_BIG == 130
    for r in SC.ROWS:
        if r.omitted or r.family == SC.SAMPLER_COMM:
            continue
        sizes = [_size(r, sh) for sh in r.edge_shapes]
        assert len(set(r.edge_shapes)) >= 3 and any(n % 32 for n in sizes), f"{r.name}: {sizes}"
        views = {sh.VIEW for sh in r.edge_shapes}
        if r.gaps or r.name == "gpemu_diag_create_dev":
            assert REQUIRED["views"] <= views, r.name
        elif r.family == SC.MODEL_BOUND:
            assert REQUIRED["B"] <= {sh.B_SMALL for sh in r.edge_shapes}, r.name
        else:
            assert REQUIRED["S"] <= {sh.S for sh in r.edge_shapes}, r.name
        if r.name in CHUNKED:
            assert REQUIRED["chunk"] <= {sh.S for sh in r.edge_shapes}, r.name
        if r.name in TAKES_D:
            assert {1, 3, 16} <= {sh.D for sh in r.edge_shapes}, r.name
    pcov = [(sh.B_SMALL, sh.M2) for sh in SC.ROW["gpemu_gp_predict_cov_dev"].edge_shapes]
    assert any(m2 == 1 for _, m2 in pcov) and any(m2 < m1 for m1, m2 in pcov) and any(m2 > m1 for m1, m2 in pcov)
    assert any(m2 == m1 for m1, m2 in pcov)


WIDE = [(r, sh) for r in SC.ROWS if r.family in (SC.DEVICE_WIDE, SC.HANDLE_CREATING) and not r.cases and not r.omitted
        for sh in r.edge_shapes]


def test_the_inputs_of_the_device_wide_rows_obey_the_headers_rules_at_every_shape():
    """what can be checked without a device: the sizes the header bounds, the totals of the fixed-point weights against
    the targets, the ranks and n_out the closures derive from S"""
    for r, sh in WIDE:
        with SC.shaped(sh):
            assert 1 <= sh.S < 2 ** 31 and 1 <= sh.D <= 16 and sh.VIEW[2] >= sh.VIEW[1] >= 1 and 1 <= sh.RW <= 64, (r.name, sh)
            assert SC.EDGES1.shape == (sh.D, 9) and SC.EDGES2.shape == (sh.D, 5) and SC._W_TARGETS.shape == (sh.RW, 3)
            for seed in (0, 1):
                T = r.inputs(None, seed)
                for name, a in T.items():
                    assert np.isfinite(a).all() and a.size > 0, (r.name, sh, name)
                    if name == "q":
                        tot = a.sum(axis=1)
                        assert a.shape[1] == sh.S and (a > 0).all() and (tot >= 2 ** 47).all() and (tot < 2 ** 48).all(), (r.name, sh)
                        assert (SC._W_TARGETS <= 2 ** 47).all() and (SC._W_TARGETS >= 1).all()
                    elif name in ("V", "L", "lw", "r2", "zeros"):
                        assert a.shape[-1] == sh.S, (r.name, sh, name, a.shape)
                    elif name == "X" and not r.gaps:
                        assert a.shape == (sh.S, sh.D), (r.name, sh, a.shape)
                    elif name == "X":
                        assert a.shape == (sh.VIEW[0] * sh.VIEW[2], sh.D)
            assert 1 <= max(1, (sh.S + 5) // 10) <= sh.S and 0 <= sh.S // 2 <= sh.S - 1      # n_out of HPD, the ranks


def test_the_view_weights_reach_their_targets():
    for nb, br, bs in REQUIRED["views"]:
        q = SC._fixed_weights(np.random.default_rng(nb), 2, nb * br, 45)
        assert ((q.sum(axis=1) >= 2 ** 45) & (q.sum(axis=1) < 2 ** 46)).all() and (q > 0).all()
    assert (SC._W_VIEW_TARGETS <= 2 ** 45).all()


def test_the_default_shape_is_todays():
    d = SC.Shape()
    assert (d.S, d.D, d.VIEW, d.B_SMALL, d.B_BIG, d.RW, d.M2, d.pad) == (257, 3, (16, 4, 6), 33, 130, 2, 17, 0)
    before = {k: getattr(SC, k) for k in ("S_WIDE", "D_WIDE", "VIEW", "B_SMALL", "B_BIG", "RW2", "M2_COV", "PAD")}
    with SC.shaped(dataclasses.replace(d, S=65, D=16, pad=7)):
        assert (SC.S_WIDE, SC.D_WIDE, SC.PAD) == (65, 16, 7) and SC.EDGES1.shape == (16, 9)
    assert before == {k: getattr(SC, k) for k in before} and SC.EDGES1.shape == (3, 9)
    assert str(d) == "default" and str(dataclasses.replace(d, S=65, VIEW=(3, 5, 5))) == "S=65,VIEW=(3,5,5)"


# ---- the header ----------------------------------------------------------------------------------------------------------
CONTRACT = (
    "A call writes only the elements of its outputs that its section names",
    "It does not write padding (ld > n), gaps of a strided view, or anything before or after",
    "It does not write its inputs",
    "Its results do not depend on the previous contents of the outputs or on memory beside the inputs",
    "A declined call writes nothing",
)


def test_the_header_states_the_contract():
    text = SC.header_text()
    block = text[text.index("Conventions"):text.index("#ifndef GPEMU_H")]
    flat = re.sub(r"\s*\n \*\s*", " ", block)
    for sentence in CONTRACT:
        assert sentence in flat, f"the Conventions block of include/gpemu.h does not say: {sentence!r}"
